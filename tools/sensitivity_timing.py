"""Kernel time of k_sensitivity by HIP events (lcqp_hip_batch_sensitivity_timing) on the synthetic workload after run, beside its
algorithmic bytes: bytes_bs(np) + 2 * 8 * np * n_T + 8 * n_T (n_T + 1) / 2 per right-hand side, summed over the batch from the n_T of
every instance (the rows of its working set, counted from `side`).  DESIGN.md section 7.

usage: python tools/sensitivity_timing.py [--log FILE] [--reps 30]

--sparse: k_sparse_sensitivity (lcqp_hip_sparse_sensitivity_timing) on the sparse synthetic workload (lcqpow_amd/synth_sparse.py) after
run, nrhs = 1: n = 4096 with B = 4096 (skipped with --quick), and (512, 256, 64) with B = 1024 on the band engine and, under
LCQP_SPARSE_GENERAL=1, on the general LDL'.  Beside each, on the same handle in the same process, the time of a warm resolve of unchanged
data (refresh + homotopy, last_timing) -- the unit a finite-difference gradient pays 2 nV times.
    python tools/sensitivity_timing.py --sparse [--quick] [--log FILE] [--reps 20]

--blocked: k_sensitivity_blk (lcqp_hip_batch_sensitivity_blocked) beside k_sensitivity on the same handle in the same process, the calls
interleaved, for nrhs = 1, 16, 64, 256 on the BASELINE shape (B = 1024, n = 256, nC = 512, nComp = 64) and on (40, 20, 8) with B = 1024;
then jacobian() beside the vector call on an uploaded identity, kernel time and wall clock.
    python tools/sensitivity_timing.py --blocked [--quick] [--log FILE] [--reps 20]

--blocked --duals: jacobian_duals() (k_sensitivity_blk_dual on the unit vectors of the slot space) beside the loop of vector adjoint calls it
replaces -- one lcqp_hip_batch_adjoint call per dual position in some instance's working set -- on the BASELINE shape with B = 4 and
B = 1024 (256 with --quick), one handle, interleaved; kernel time summed over the launches, and wall clock.
    python tools/sensitivity_timing.py --blocked --duals [--quick] [--log FILE] [--reps 20]

--adjoint: lcqp_hip_batch_adjoint with all four matrix gradients on the BASELINE shape and on (40, 20, 8), B = 1024 (256 with --quick):
reduce = 1 (k_adjoint_reduce, (nV + mA) nV doubles to the host) beside reduce = 0 (k_adjoint_outer in chunks, B times as many) on the same
handle in the same process, the calls interleaved; kernel time (the sum of the call's kernels, k_sensitivity included) and wall clock.
    python tools/sensitivity_timing.py --adjoint [--quick] [--log FILE] [--reps 20]

--sparse --adjoint: lcqp_hip_sparse_adjoint with both value-array gradients on the sparse synthetic workload, (512, 256, 64) with B = 1024
(256 with --quick) on the band engine: reduce = 1 (k_sparse_adjoint_reduce, nnzQ + nnzA doubles to the host) beside reduce = 0
(k_sparse_adjoint_nnz in chunks, B times as many) on the same handle in the same process, the calls interleaved; kernel time (the sum of the
call's kernels, k_sparse_sensitivity<G, true> included) and wall clock.
    python tools/sensitivity_timing.py --sparse --adjoint [--quick] [--log FILE] [--reps 20]

--sparse --blocked: k_sparse_sensitivity_blk (sb.sensitivity_blocked(V)) beside k_sparse_sensitivity (sb.sensitivity(V)) at nrhs = 64,
interleaved, and sb.jacobian(), on the sparse synthetic workload (512, 256, 64) on the band engine with B = 1024 (256 with --quick) and
with B = 4, the few-instances case the (instance, panel) mapping is for.
    python tools/sensitivity_timing.py --sparse --blocked [--quick] [--log FILE] [--reps 20]

--sparse --blocked --general-panel: the general LDL' with its panel form off and on (SparseBatchLCQP.set_general_panel) on the SAME handle in
the same process, the calls interleaved: sensitivity_blocked at nrhs = 64 and jacobian(first=0, count=1) on the grid workload
(lcqpow_amd/synth_sparse.py::grid_pattern_arrays) at g = 44 (nC = 200, nComp = 300) and g = 128 (bench.py's grid_128), B = 1 and B = 64.
Off is the vector kernel.  --jac-reps: timed Jacobian calls (default: --reps; after the same 3 warm-up calls; 0 skips them: with the switch
off a Jacobian is nV launches of the vector kernel over the whole batch -- 16 384 per call at g = 128); --grids, --batches: other sizes.
    python tools/sensitivity_timing.py --sparse --blocked --general-panel [--grids 44,128] [--batches 1,64] [--jac-reps N] [--log FILE] [--reps 20]

--sparse --blocked --duals: sb.jacobian_duals(bounds=False) (k_sparse_sensitivity_blk_dual on the unit columns of the working set) beside the loop
of vector calls it replaces -- one sb.adjoint(0, e_r) per row r in the working set of some instance -- on one handle, interleaved; kernel time
summed over the launches.  (512, 256, 64) on the band engine with B = 4 and B = 1024 (256 with --quick), then the 44 x 44 grid on the general LDL'
with its panel form on (k_sparse_sensitivity_blk_general_dual), B = 1 and B = 64 (--batches).
    python tools/sensitivity_timing.py --sparse --blocked --duals [--quick] [--batches 1,64] [--log FILE] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402

HBM_PEAK = 8.0e12      # bytes per second, MI355X


def measure(B, nrhs, reps, n=256, nC=512, nComp=64, warmup=5):
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options())
    bt.generate_synthetic(0)
    bt.run()
    st = bt.solution()[2]
    rng = np.random.default_rng(0)
    v = rng.standard_normal((B, nrhs, n))
    ms = []
    for r in range(warmup + reps):
        dg, db, side, info = bt.sensitivity(v)
        if r >= warmup:
            ms.append(bt.sensitivity_kernel_ms())
    bt.close()
    npad = 128 * ((n + 127) // 128)
    nT = np.count_nonzero(side, axis=1).astype(np.float64)
    per_rhs = 8.0 * npad * (npad + 2) + 2 * 8.0 * npad * nT + 8.0 * nT * (nT + 1) / 2
    total = nrhs * per_rhs.sum()
    ms = np.sort(np.array(ms))
    med = float(np.median(ms))
    return dict(B=B, nrhs=nrhs, solved=sum(s["returnValue"] == 0 for s in st), flagged=int(np.count_nonzero(info)), nT_mean=float(nT.mean()),
                ms_min=float(ms[0]), ms_median=med, ms_max=float(ms[-1]), bytes=total, tbps=total / (med * 1e-3) / 1e12,
                peak_fraction=total / (med * 1e-3) / HBM_PEAK, us_per_rhs=1e3 * med / nrhs)


def measure_sparse(B, n, nC, nK, general, reps, warmup=3):
    from lcqpow_amd import synth_sparse as S
    if general:
        os.environ["LCQP_SPARSE_GENERAL"] = "1"      # read when the handle is created
    else:
        os.environ.pop("LCQP_SPARSE_GENERAL", None)
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    os.environ.pop("LCQP_SPARSE_GENERAL", None)
    for c0 in range(0, B, 1024):
        inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(c0, min(B, c0 + 1024))]
        st = lambda k: np.stack([d[k] for d in inst])
        assert sb.load(c0, len(inst), st("Qx"), st("g"), st("Ex"), lbA=st("lbA"), ubA=st("ubA")) == 0
    sb.run()
    stats = sb.solution()[2]
    v = np.random.default_rng(0).standard_normal((B, n))
    ms, warm = [], []
    for r in range(warmup + reps):
        dg, db, side, info = sb.sensitivity(v)
        if r >= warmup:
            ms.append(sb.sensitivity_kernel_ms())
    for r in range(warmup + reps):
        sb.resolve(warm=True)
        sb.synchronize()
        if r >= warmup:
            warm.append(sum(sb.last_timing()))
    engine = "general LDL', %d fronts" % sb.fronts() if sb.fronts() else "band, %d lanes" % sb.lanes()
    sb.close()
    ms, warm = np.sort(np.array(ms)), np.sort(np.array(warm))
    return dict(B=B, n=n, nC=nC, nK=nK, engine=engine, solved=sum(s["returnValue"] == 0 for s in stats), flagged=int(np.count_nonzero(info)),
                W_mean=float(np.count_nonzero(side, axis=1).mean()), ms_min=float(ms[0]), ms_median=float(np.median(ms)), ms_max=float(ms[-1]),
                warm_min=float(warm[0]), warm_median=float(np.median(warm)), warm_max=float(warm[-1]),
                fd_ratio=2.0 * n * float(np.median(warm)) / float(np.median(ms)))


def measure_blocked(B, n, nC, nComp, nrhs_list, reps, warmup=3):
    import time
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options())
    bt.generate_synthetic(0)
    bt.run()
    lines = []
    rng = np.random.default_rng(0)
    stat = lambda ms: (float(np.min(ms)), float(np.median(ms)), float(np.max(ms)))
    for nrhs in nrhs_list:
        v = rng.standard_normal((B, nrhs, n))
        vec, blk = [], []
        for r in range(warmup + reps):      # interleaved: one vector call, one blocked call
            bt.sensitivity(v)
            t0 = bt.sensitivity_kernel_ms()
            bt.sensitivity(v, blocked=True)
            t1 = bt.sensitivity_kernel_ms()
            if r >= warmup:
                vec.append(t0); blk.append(t1)
        a, b = stat(vec), stat(blk)
        lines.append("n = %d B = %d nrhs = %3d: vector kernel ms min / median / max = %.4f / %.4f / %.4f; blocked = %.4f / %.4f / %.4f; "
                     "vector median / blocked median = %.2f; blocked median below vector min: %s"
                     % (n, B, nrhs, a[0], a[1], a[2], b[0], b[1], b[2], a[1] / b[1], b[1] < a[0]))
        print(lines[-1], flush=True)
    # the Jacobian: the device's unit vectors against an uploaded identity through the vector kernel
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))
    kj, wj, kv, wv = [], [], [], []
    for r in range(1 + max(3, reps // 4)):
        t = time.perf_counter(); Jg = bt.jacobian(bounds=False)[0]; w1 = time.perf_counter() - t
        k1 = bt.sensitivity_kernel_ms()
        t = time.perf_counter(); dg = bt.sensitivity(eye)[0]; w0 = time.perf_counter() - t
        k0 = bt.sensitivity_kernel_ms()
        if r >= 1:
            kj.append(k1); wj.append(1e3 * w1); kv.append(k0); wv.append(1e3 * w0)
    sym = float(np.abs(Jg - Jg.transpose(0, 2, 1)).max())
    lines.append("n = %d B = %d jacobian(): kernel ms min / median / max = %.3f / %.3f / %.3f, wall ms median %.1f; vector kernel on an uploaded identity: "
                 "%.3f / %.3f / %.3f, wall ms median %.1f; max |jacobian - vector| = %.3g, max |Jg - Jg'| = %.3g"
                 % ((n, B) + stat(kj) + (float(np.median(wj)),) + stat(kv) + (float(np.median(wv)), float(np.abs(Jg - dg).max()), sym)))
    print(lines[-1], flush=True)
    bt.close()
    return lines


def measure_duals(B, n, nC, nComp, reps, warmup=1):
    """jacobian_duals() beside the loop of vector adjoint calls it replaces -- one call with vx = 0, vy = e_r per dual position r that is in
    the working set of some instance -- on one handle, interleaved: kernel time (summed over the launches) and wall clock"""
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options())
    bt.generate_synthetic(0)
    bt.run()
    nd = n + nC + 2 * nComp
    side = bt.sensitivity(np.zeros((B, n)))[2]
    rows = np.flatnonzero(np.any(side != 0, axis=0))
    nW = np.count_nonzero(side, axis=1)
    zero = np.zeros((B, n))
    stat = lambda ms: (float(np.min(ms)), float(np.median(ms)), float(np.max(ms)))
    kj, wj, kv, wv = [], [], [], []
    worst = 0.0
    for rep in range(warmup + reps):
        # (the bound block is [B][nd][nd] on the host: asked for with a few instances only; the kernel is the same either way)
        t = time.perf_counter(); Jyg, Jyb = bt.jacobian_duals(bounds=B <= 64)[:2]; w1 = time.perf_counter() - t
        k1 = bt.sensitivity_kernel_ms()
        k0 = 0.0
        t = time.perf_counter()
        for r in rows:
            vy = np.zeros((B, nd)); vy[:, r] = 1.0
            out = bt.adjoint(zero, vy, matrices=())
            k0 += bt.sensitivity_kernel_ms()
            if rep == 0:
                inW = side[:, r] != 0
                worst = max(worst, float(np.abs(out["dg"][inW] - Jyg[inW, r]).max(initial=0.0)))
                if Jyb is not None:
                    worst = max(worst, float(np.abs(out["db"][inW] - Jyb[inW, r]).max(initial=0.0)))
        w0 = time.perf_counter() - t
        if rep >= warmup:
            kj.append(k1); wj.append(1e3 * w1); kv.append(k0); wv.append(1e3 * w0)
    a, b = stat(kv), stat(kj)
    line = ("n = %d nC = %d nComp = %d B = %d: rows of W per instance min / mean / max = %d / %.1f / %d, %d vector calls per loop; loop of vector adjoint calls: "
            "kernel ms min / median / max = %.3f / %.3f / %.3f, wall ms median %.1f; jacobian_duals(): kernel ms = %.3f / %.3f / %.3f, wall ms median %.1f; "
            "vector median / blocked median = %.2f (kernels), %.2f (wall); max |loop - jacobian_duals| = %.3g"
            % ((n, nC, nComp, B, nW.min(), nW.mean(), nW.max(), len(rows)) + a + (float(np.median(wv)),) + b + (float(np.median(wj)),)
               + (a[1] / b[1], float(np.median(wv)) / float(np.median(wj)), worst)))
    print(line, flush=True)
    bt.close()
    return line


def duals_main(a):
    reps = a.reps
    lines = [measure_duals(B, 256, 512, 64, reps) for B in ((4, 256) if a.quick else (4, 1024))]
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("lcqp_hip_batch_jacobian_duals beside the loop of lcqp_hip_batch_adjoint calls it replaces, synthetic workload after run, one handle, "
                    "calls interleaved; %d timed repetitions after 1 warm-up repetition each\n" % reps)
            f.write("\n".join(lines) + "\n")


def measure_adjoint(B, n, nC, nComp, reps, warmup=3):
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options())
    bt.generate_synthetic(0)
    bt.run()
    rng = np.random.default_rng(0)
    vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, n + nC + 2 * nComp))
    ms = {False: [], True: []}; wall = {False: [], True: []}
    for r in range(warmup + reps):
        for reduce in (True, False):      # interleaved: both see the same drift of the clocks
            t0 = time.perf_counter()
            out = bt.adjoint(vx, vy, reduce=reduce)
            t1 = time.perf_counter()
            if r >= warmup:
                ms[reduce].append(bt.sensitivity_kernel_ms()); wall[reduce].append(1e3 * (t1 - t0))
    bt.close()
    q = lambda a: (float(np.min(a)), float(np.median(a)), float(np.max(a)))
    line = "n = %d nC = %d nComp = %d B = %d:" % (n, nC, nComp, B)
    for reduce in (True, False):
        line += " reduce = %d kernels ms min / median / max = %.4f / %.4f / %.4f, wall ms = %.2f / %.2f / %.2f;" % ((int(reduce),) + q(ms[reduce]) + q(wall[reduce]))
    line += " flagged %d" % int(np.count_nonzero(out["info"]))
    print(line, flush=True)
    return line


def measure_sparse_adjoint(B, n, nC, nK, reps, warmup=3):
    from lcqpow_amd import synth_sparse as S
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
    st = lambda k: np.stack([d[k] for d in inst])
    assert sb.load(0, B, st("Qx"), st("g"), st("Ex"), lbA=st("lbA"), ubA=st("ubA")) == 0
    sb.run()
    rng = np.random.default_rng(0)
    vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, nC + 2 * nK))
    ms = {False: [], True: []}; wall = {False: [], True: []}
    for r in range(warmup + reps):
        for reduce in (True, False):      # interleaved: both see the same drift of the clocks
            t0 = time.perf_counter()
            out = sb.adjoint(vx, vy, reduce=reduce)
            t1 = time.perf_counter()
            if r >= warmup:
                ms[reduce].append(sb.sensitivity_kernel_ms()); wall[reduce].append(1e3 * (t1 - t0))
    engine = "band, %d lanes" % sb.lanes()
    sb.close()
    q = lambda a: (float(np.min(a)), float(np.median(a)), float(np.max(a)))
    line = "n = %d nC = %d nComp = %d B = %d (%s; nnzQ %d, nnzA %d):" % (n, nC, nK, B, engine, sb.nnzQ, sb.nnzA)
    for reduce in (True, False):
        line += " reduce = %d kernels ms min / median / max = %.4f / %.4f / %.4f, wall ms = %.2f / %.2f / %.2f;" % ((int(reduce),) + q(ms[reduce]) + q(wall[reduce]))
    line += " flagged %d" % int(np.count_nonzero(out["info"]))
    print(line, flush=True)
    return line


def measure_sparse_blocked(B, n, nC, nK, nrhs, reps, warmup=3):
    """sb.sensitivity_blocked(V) (k_sparse_sensitivity, unchanged) beside sb.sensitivity(V) (k_sparse_sensitivity_blk) at nrhs vectors,
    interleaved, and sb.jacobian(), on one handle in one process; kernel time from HIP events (sensitivity_kernel_ms)"""
    from lcqpow_amd import synth_sparse as S
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
    st = lambda k: np.stack([d[k] for d in inst])
    assert sb.load(0, B, st("Qx"), st("g"), st("Ex"), lbA=st("lbA"), ubA=st("ubA")) == 0
    sb.run()
    stats = sb.solution()[2]
    v = np.random.default_rng(0).standard_normal((B, nrhs, n))
    vec, blk, jac = [], [], []
    for r in range(warmup + reps):      # interleaved: one vector call, one blocked call
        a = sb.sensitivity(v)
        t0 = sb.sensitivity_kernel_ms()
        b = sb.sensitivity_blocked(v)
        t1 = sb.sensitivity_kernel_ms()
        if r >= warmup:
            vec.append(t0); blk.append(t1)
    for r in range(warmup + reps):
        info = sb.jacobian(bounds=False)[3]
        if r >= warmup:
            jac.append(sb.sensitivity_kernel_ms())
    q = lambda ms: (float(np.min(ms)), float(np.median(ms)), float(np.max(ms)))
    line = ("n = %d nC = %d nComp = %d B = %d (band, %d lanes, panel %d) nrhs = %d: vector kernel ms min / median / max = %.4f / %.4f / %.4f; "
            "blocked = %.4f / %.4f / %.4f; vector / blocked (medians) = %.2f; us per vector and instance %.3f -> %.3f; bits equal %s; "
            "jacobian (nrhs = %d) = %.4f / %.4f / %.4f, us per column and instance %.3f; solved %d, flagged %d"
            % ((n, nC, nK, B, sb.lanes(), sb.sens_panel(), nrhs) + q(vec) + q(blk) + (np.median(vec) / np.median(blk),
               1e3 * np.median(vec) / (B * nrhs), 1e3 * np.median(blk) / (B * nrhs), bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])), n)
               + q(jac) + (1e3 * np.median(jac) / (B * n), sum(s["returnValue"] == 0 for s in stats), int(np.count_nonzero(info)))))
    sb.close()
    print(line, flush=True)
    return line


def measure_general_panel(g, nC, nK, B, nrhs, reps, jac_reps, warmup=3):
    """the general LDL' on a g x g grid: sensitivity_blocked(V) and jacobian(0, 1) with the panel form off (k_sparse_sensitivity) and on
    (k_sparse_sensitivity_blk_general), interleaved on one handle; kernel time from HIP events (sensitivity_kernel_ms)"""
    from lcqpow_amd import synth_sparse as S
    Qpat, Apat, qo, eo, info = S.grid_pattern_arrays(g, nC, nK)
    n = g * g
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    inst = [S.grid_values(i, info, (qo, eo)) for i in range(B)]
    st = lambda k: np.stack([d[k] for d in inst])
    assert sb.load(0, B, st("Qx"), st("g"), st("Ex"), lbA=st("lbA"), ubA=st("ubA")) == 0
    sb.run()
    stats = sb.solution()[2]
    v = np.random.default_rng(0).standard_normal((B, nrhs, n))
    t = {False: [], True: []}; tj = {False: [], True: []}
    out = {}
    for r in range(warmup + reps):
        for on in (False, True):
            sb.set_general_panel(on)
            out[on] = sb.sensitivity_blocked(v)
            if r >= warmup:
                t[on].append(sb.sensitivity_kernel_ms())
    for r in range((warmup + jac_reps) if jac_reps > 0 else 0):
        for on in (False, True):
            sb.set_general_panel(on)
            sb.jacobian(first=0, count=1, bounds=False)
            if r >= warmup:
                tj[on].append(sb.sensitivity_kernel_ms())
    q = lambda ms: (float(np.min(ms)), float(np.median(ms)), float(np.max(ms)))
    err = float(max(np.abs(out[True][0] - out[False][0]).max(), np.abs(out[True][1] - out[False][1]).max()))
    line = ("grid %d x %d (n = %d nC = %d nComp = %d) B = %d (general LDL', %d fronts, largest %d, panel %d) nrhs = %d: off (vector kernel) ms min / median / max = "
            "%.4f / %.4f / %.4f; on (panel kernel) = %.4f / %.4f / %.4f; off / on (medians) = %.2f; us per vector and instance %.3f -> %.3f; "
            "max |on - off| = %.3g; solved %d, flagged %d"
            % ((g, g, n, nC, nK, B, sb.fronts(), sb.max_front(), sb.sens_panel(), nrhs) + q(t[False]) + q(t[True])
               + (np.median(t[False]) / np.median(t[True]), 1e3 * np.median(t[False]) / (B * nrhs), 1e3 * np.median(t[True]) / (B * nrhs), err,
                  sum(s["returnValue"] == 0 for s in stats), int(np.count_nonzero(out[True][3])))))
    if jac_reps > 0:
        line += ("; jacobian(0, 1) (%d columns, %d timed calls): off = %.3f / %.3f / %.3f; on = %.3f / %.3f / %.3f; off / on = %.2f; us per column %.3f -> %.3f"
                 % ((n, jac_reps) + q(tj[False]) + q(tj[True]) + (np.median(tj[False]) / np.median(tj[True]), 1e3 * np.median(tj[False]) / n, 1e3 * np.median(tj[True]) / n)))
    sb.close()
    print(line, flush=True)
    return line


def measure_sparse_duals(sb, label, reps, warmup=1):
    """jacobian_duals(bounds=False) beside the loop of adjoint(0, e_r) calls over the union of the working sets, interleaved on the solved
    handle sb; kernel time from HIP events (sensitivity_kernel_ms)"""
    B, n, m = sb.B, sb.nV, sb.m
    zero = np.zeros((B, n))
    side = sb.sensitivity(zero)[2]
    rows = np.flatnonzero(np.any(side != 0, axis=0))
    nW = np.count_nonzero(side, axis=1)
    kj, kv = [], []
    worst = 0.0
    for r in range(warmup + reps):
        Jyg = sb.jacobian_duals(bounds=False)[0]
        k1 = sb.sensitivity_kernel_ms()
        k0 = 0.0
        for row in rows:
            vy = np.zeros((B, m)); vy[:, row] = 1.0
            out = sb.adjoint(zero, vy, matrices=())
            k0 += sb.sensitivity_kernel_ms()
            if r == 0:
                inW = side[:, row] != 0
                worst = max(worst, float(np.abs(out["dg"][inW] - Jyg[inW, row]).max(initial=0.0)))
        if r >= warmup:
            kj.append(k1); kv.append(k0)
    q = lambda ms: (float(np.min(ms)), float(np.median(ms)), float(np.max(ms)))
    tot = float(nW.sum())
    line = ("%s B = %d (panel %d): rows of W per instance min / mean / max = %d / %.1f / %d, %d vector calls per loop; loop of adjoint(0, e_r): kernel ms min / "
            "median / max = %.3f / %.3f / %.3f; jacobian_duals() = %.3f / %.3f / %.3f; loop / jacobian_duals (medians) = %.2f; us per row of W "
            "%.3f -> %.3f; max |loop - jacobian_duals| = %.3g"
            % ((label, B, sb.sens_panel(), nW.min(), nW.mean(), nW.max(), len(rows)) + q(kv) + q(kj)
               + (np.median(kv) / np.median(kj), 1e3 * np.median(kv) / tot, 1e3 * np.median(kj) / tot, worst)))
    print(line, flush=True)
    return line


def sparse_duals_main(a):
    from lcqpow_amd import synth_sparse as S
    lines = []
    n, nC, nK = 512, 256, 64
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    for B in ((4, 256) if a.quick else (4, 1024)):
        sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
        inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
        st = lambda k: np.stack([d[k] for d in inst])
        assert sb.load(0, B, st("Qx"), st("g"), st("Ex"), lbA=st("lbA"), ubA=st("ubA")) == 0
        sb.run()
        lines.append(measure_sparse_duals(sb, "n = %d nC = %d nComp = %d (band, %d lanes)" % (n, nC, nK, sb.lanes()), a.reps))
        sb.close()
    g, nC, nK = 44, 200, 300
    Qpat, Apat, qo, eo, info = S.grid_pattern_arrays(g, nC, nK)
    for B in [int(x) for x in a.batches.split(",")]:
        sb = la.SparseBatchLCQP(B, g * g, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
        inst = [S.grid_values(i, info, (qo, eo)) for i in range(B)]
        st = lambda k: np.stack([d[k] for d in inst])
        assert sb.load(0, B, st("Qx"), st("g"), st("Ex"), lbA=st("lbA"), ubA=st("ubA")) == 0
        sb.run()
        sb.set_general_panel(True)
        lines.append(measure_sparse_duals(sb, "grid %d x %d (n = %d nC = %d nComp = %d; general LDL', %d fronts, panel form on)" % (g, g, g * g, nC, nK, sb.fronts()), a.reps))
        sb.close()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("lcqp_hip_sparse_jacobian_duals beside the loop of lcqp_hip_sparse_adjoint calls it replaces, sparse synthetic workloads after run, one handle, "
                    "calls interleaved; %d timed repetitions after 1 warm-up repetition each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


def general_panel_main(a):
    shape = {44: (200, 300), 128: (800, 1200)}
    lines = []
    for g in [int(x) for x in a.grids.split(",")]:
        nC, nK = shape.get(g, (g * g // 10, g * g // 7))
        for B in [int(x) for x in a.batches.split(",")]:
            lines.append(measure_general_panel(g, nC, nK, B, 64, a.reps, a.jac_reps))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("the general LDL' with its panel form off (k_sparse_sensitivity) and on (k_sparse_sensitivity_blk_general), grid workload after run, one handle, "
                    "calls interleaved; %d timed calls after 3 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


def sparse_blocked_main(a):
    lines = [measure_sparse_blocked(B, 512, 256, 64, 64, a.reps) for B in ((256, 4) if a.quick else (1024, 4))]
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("k_sparse_sensitivity_blk beside k_sparse_sensitivity, sparse synthetic workload after run, one handle, calls interleaved; %d timed calls after 3 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


def sparse_adjoint_main(a):
    lines = [measure_sparse_adjoint(256 if a.quick else 1024, 512, 256, 64, a.reps)]
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("lcqp_hip_sparse_adjoint, reduce = 1 beside reduce = 0, sparse synthetic workload after run, one handle, calls interleaved; %d timed calls after 3 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


def adjoint_main(a):
    B = 256 if a.quick else 1024
    lines = [measure_adjoint(B, n, nC, nComp, a.reps) for n, nC, nComp in ((40, 20, 8), (256, 512, 64))]
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("lcqp_hip_batch_adjoint, reduce = 1 beside reduce = 0, synthetic workload after run, one handle, calls interleaved; %d timed calls after 3 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


def blocked_main(a):
    lines = []
    nr = (1, 16, 64) if a.quick else (1, 16, 64, 256)
    for B, n, nC, nComp in ((1024, 40, 20, 8), (256 if a.quick else 1024, 256, 512, 64)):
        lines += measure_blocked(B, n, nC, nComp, nr, a.reps)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("k_sensitivity_blk beside k_sensitivity, synthetic workload after run, one handle, calls interleaved; %d timed calls after 3 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


def sparse_main(a):
    shapes = [(1024, 512, 256, 64, False), (1024, 512, 256, 64, True)]
    if not a.quick:
        shapes.insert(0, (4096, 4096, 2048, 512, False))
    lines = []
    for B, n, nC, nK, general in shapes:
        r = measure_sparse(B, n, nC, nK, general, a.reps)
        lines.append("n = {n:4d} nC = {nC} nComp = {nK} B = {B:4d} ({engine}) nrhs = 1: kernel ms min / median / max = {ms_min:.4f} / {ms_median:.4f} / {ms_max:.4f}; "
                     "warm resolve of unchanged data (refresh + homotopy) ms min / median / max = {warm_min:.3f} / {warm_median:.3f} / {warm_max:.3f}; "
                     "2 nV warm re-solves / one call = {fd_ratio:.3g}; mean |W| {W_mean:.1f}; solved {solved}, flagged {flagged}".format(**r))
        print(lines[-1], flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("k_sparse_sensitivity, sparse synthetic workload after run; %d timed calls after 3 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sparse", action="store_true", help="the sparse arm's kernel beside a warm resolve of unchanged data")
    ap.add_argument("--quick", action="store_true", help="--sparse: without the n = 4096, B = 4096 batch; --blocked: B = 256 at n = 256, without nrhs = 256")
    ap.add_argument("--blocked", action="store_true", help="the blocked kernel beside the vector kernel, and the Jacobian")
    ap.add_argument("--duals", action="store_true", help="--blocked: the dual Jacobian beside the loop of vector adjoint calls it replaces (B = 4 and B = 1024; --quick: 256); with --sparse: on the sparse arm")
    ap.add_argument("--adjoint", action="store_true", help="the matrix gradients summed on the device beside the per-instance path")
    ap.add_argument("--general-panel", action="store_true", help="--sparse --blocked: the general LDL' with its panel form off and on, on one handle")
    ap.add_argument("--grids", default="44,128", help="--general-panel: grid sizes")
    ap.add_argument("--batches", default="1,64", help="--general-panel: batch sizes")
    ap.add_argument("--jac-reps", type=int, default=None, help="--general-panel: timed jacobian(0, 1) calls per setting (default: --reps; 0: none)")
    a = ap.parse_args()
    if a.jac_reps is None:
        a.jac_reps = a.reps
    if la.device_count() < 1:
        raise SystemExit("needs a GPU (no CPU fallback)")
    if a.sparse and a.adjoint:
        return sparse_adjoint_main(a)
    if a.sparse and a.blocked and a.duals:
        return sparse_duals_main(a)
    if a.sparse and a.blocked and a.general_panel:
        return general_panel_main(a)
    if a.sparse and a.blocked:
        return sparse_blocked_main(a)
    if a.sparse:
        return sparse_main(a)
    if a.blocked and a.duals:
        return duals_main(a)
    if a.blocked:
        return blocked_main(a)
    if a.adjoint:
        return adjoint_main(a)
    lines = []
    for B, nrhs in ((1024, 1), (1024, 8), (1, 1), (1, 8)):
        r = measure(B, nrhs, a.reps)
        lines.append("B = {B:5d} nrhs = {nrhs}: kernel ms min / median / max = {ms_min:.4f} / {ms_median:.4f} / {ms_max:.4f} ({us_per_rhs:.1f} us per right-hand side); "
                     "algorithmic bytes {bytes:.4g} -> {tbps:.3f} TB/s = {peak_fraction:.3f} of the HBM peak; mean n_T {nT_mean:.1f}; solved {solved}, flagged {flagged}".format(**r))
        print(lines[-1], flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("k_sensitivity, synthetic workload n = 256, nC = 512, nComp = 64 after run; %d timed calls after 5 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
