"""The blocked adjoint with gradients on y and the dual rows of the Jacobian (lcqp_hip_batch_adjoint_blocked / _jacobian_duals and the
device twins; DESIGN.md section 3a'''', "Panels with gradients on y").

Convention (include/lcqp_hip.h): K [d; mu] = [v_x; -v_y|_W] with K = [[Q, E_W'], [E_W, 0]], dg = -d, db_W = mu.

1  dg, db against numpy on the device's own working set, bound 1e-12 nV cond_2(K) max(|v_x|_inf, |v_y|_inf) per column (float64 LU refined
   with long-double residuals up to np = 512, plain float64 beyond); side / info equal the vector call's.
2  three columns against the vector adjoint within that bound; on the np = 1024 fallback to the bit.
3  column independence, bit for bit: 1, 3, 16, 17 columns, a permuted call, a second call, the zero pair, vy = None against
   sensitivity(V, blocked=True), vx = None against an explicit zero VX.
4  the dual Jacobian: Jyg[r][j] = Jb[j][r]; Jyb symmetric, its W x W block positive definite and equal to (E_W Q^-1 E_W')^-1; zeros outside W;
   equal to adjoint_blocked(None, unit vectors of W) to the bit; sub-range and chunks return the unchunked bits.
5  central differences of y*, h = 1e-6, by the method and bound of tests/test_gpu_adjoint.py::test_central_differences_lcqp; at most one
   instance in four may change its working set (on the device none of seeds 1000 .. 1007 does; not checked on the CPU oracle).
6  state and flags.      7  the device twins and BatchLCQPLayer.jacobian(duals=True).

Problems: tests/problems.py::random_lcqp with default_rng(1000 + instance), perturbStep = 0.  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch      # noqa: F401 -- before the library is first loaded: the library and torch must share one HIP runtime (lcqpow_amd.capi.lib)

import problems as P
from batch_helpers import LD, assert_same_bits, load_all, result, stack, update_all
from problems import perturbed, random_lcqp

pytestmark = pytest.mark.gpu

PANEL = 16
NRHS = 2 * PANEL + 3
ZERO_COL = 5
H_FD = 1e-6
#          n,  nC, nComp, B, box, shifted, equalities     path
SHAPES = {"np128": (40, 20, 8, 6, False, False, False),              # a ragged last panel
          "np256_box": (200, 330, 37, 3, True, False, False),        # box rows in W, pos() through boxidx
          "np384": (300, 100, 40, 2, False, False, False),           # one workgroup per CU
          "np512_big_T": (400, 300, 20, 2, False, False, True),      # n_T = 321 > 256: more than four 64-row slot blocks
          "fallback": (600, 200, 50, 2, True, True, False)}          # np = 1024: the vector kernel behind the new entry points


def rows_and_bounds(d):
    """E = [A; L; R; box rows] and the entry of the dual vector (box first) each row belongs to"""
    n, nC, nComp = d["nV"], d["nC"], d["nComp"]
    lb = d.get("lb"); ub = d.get("ub")
    lb = np.full(n, -np.inf) if lb is None else lb
    ub = np.full(n, np.inf) if ub is None else ub
    boxed = np.flatnonzero(np.isfinite(lb) | np.isfinite(ub))
    A = d["A"] if d.get("A") is not None else np.zeros((0, n))
    E = np.vstack([A, d["L"], d["R"], np.eye(n)[boxed]])
    pos = np.concatenate([n + np.arange(nC + 2 * nComp), boxed])
    return E, pos


def working_rows(ws):
    sr = ws["slot_row"][:ws["ns"]]
    return np.sort(sr[sr >= 0])


def problems_of(key):
    n, nC, nComp, B, box, shifted, eq = SHAPES[key]
    ds = []
    for b in range(B):
        d = random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, box, shifted)
        if eq:
            d["ubA"] = d["lbA"].copy()
        ds.append(d)
    return ds


def kkt_adjoint_reference(Q, EW, VX, VYW, extended):
    """tests/test_gpu_adjoint.py::kkt_adjoint_reference for the columns of VX [n][k], VYW [m][k]: dg [n][k], mu [m][k] of
    K [d; mu] = [vx; -vyW], and cond_2(K)"""
    n, m = Q.shape[0], EW.shape[0]
    K = np.zeros((n + m, n + m)); K[:n, :n] = Q; K[:n, n:] = EW.T; K[n:, :n] = EW
    rhs = np.concatenate([VX, -VYW])
    sol = np.linalg.solve(K, rhs)
    if extended:
        KL, rl, sl = K.astype(LD), rhs.astype(LD), sol.astype(LD)
        for _ in range(3):
            sl = sl + np.linalg.solve(K, (rl - KL @ sl).astype(np.float64)).astype(LD)
        sol = sl.astype(np.float64)
    ev = np.abs(np.linalg.eigvalsh(K))
    return -sol[:n], sol[n:], float(ev.max() / ev.min())


def dual_staging_bytes(su, nd, instances):
    """the staging of `instances` instances of a dual Jacobian (DESIGN.md section 3a''''): capS rows of np + nd + 2 capS doubles and one int"""
    return instances * (8 * su["capS"] * (su["np"] + nd + 2 * su["capS"]) + 4 * su["capS"])


@functools.lru_cache(maxsize=None)
def solved_case(key):
    """one solve per shape and every call the tests 1 - 4 compare"""
    import lcqpow_amd as hip
    n, nC, nComp, B, box, shifted, eq = SHAPES[key]
    nd = n + nC + 2 * nComp
    ds = problems_of(key)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    x, y, st = bt.solution()
    su = bt.read_setup(0)
    ws = [bt.read_working_set(b) for b in range(B)]
    rng = np.random.default_rng(79)
    VX, VY = rng.standard_normal((B, NRHS, n)), rng.standard_normal((B, NRHS, nd))
    VX[:, ZERO_COL] = 0.0; VY[:, ZERO_COL] = 0.0
    counts = bt.launch_counts()
    c = dict(ds=ds, st=st, ws=ws, VX=VX, VY=VY, su=su)
    c["full"] = bt.adjoint_blocked(VX, VY)
    c["ms"] = bt.sensitivity_kernel_ms()
    c["again"] = bt.adjoint_blocked(VX, VY)
    c["prefix"] = {k: bt.adjoint_blocked(VX[:, :k], VY[:, :k]) for k in (1, 3, PANEL, PANEL + 1)}
    c["perm"] = np.random.default_rng(3).permutation(NRHS)
    c["permuted"] = bt.adjoint_blocked(VX[:, c["perm"]], VY[:, c["perm"]])
    c["cols"] = (0, 7, NRHS - 1)
    c["vec"] = {k: bt.adjoint(VX[:, k], VY[:, k], matrices=()) for k in c["cols"]}
    c["novy"] = bt.adjoint_blocked(VX, None)
    c["sens"] = bt.sensitivity(VX, blocked=True)
    c["novx"] = bt.adjoint_blocked(None, VY)
    c["zerovx"] = bt.adjoint_blocked(np.zeros_like(VX), VY)
    c["jac"] = bt.jacobian()
    c["jd"] = bt.jacobian_duals()
    c["jd_ms"] = bt.sensitivity_kernel_ms()
    c["jd_nobounds"] = bt.jacobian_duals(bounds=False)
    c["jd_part"] = bt.jacobian_duals(first=1, count=B - 1)
    c["jd_one"] = bt.jacobian_duals(_staging_bytes=1)                                                   # one instance per launch
    c["jd_partial"] = bt.jacobian_duals(_staging_bytes=dual_staging_bytes(su, nd, max(1, B - 1)))      # B - 1 instances, then one
    # the unit vectors of W, in the order of the dual layout, through the panel call
    E, pos = rows_and_bounds(ds[0])
    posW = [np.sort(rows_and_bounds(ds[b])[1][working_rows(ws[b])]) for b in range(B)]
    kmax = max(len(p) for p in posW)
    U = np.zeros((B, kmax, nd))
    for b in range(B):
        U[b, np.arange(len(posW[b])), posW[b]] = 1.0
    c["posW"] = posW
    c["units"] = bt.adjoint_blocked(None, U)
    assert bt.launch_counts() == counts
    bt.close()
    return c


@functools.lru_cache(maxsize=None)
def reference_of(key):
    c = solved_case(key)
    n = SHAPES[key][0]
    out = []
    for b, d in enumerate(c["ds"]):
        E, pos = rows_and_bounds(d)
        W = working_rows(c["ws"][b])
        dg, mu, cond = kkt_adjoint_reference(d["Q"], E[W], c["VX"][b].T, c["VY"][b][:, pos[W]].T, extended=n <= 512)
        out.append(dict(E=E, pos=pos, W=W, dg=dg.T, mu=mu.T, cond=cond))
    return out


def same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, nC, nComp, B = SHAPES[key][:4]
    nd = n + nC + 2 * nComp
    dg, db, side, info = c["full"]
    vec = c["vec"][0]
    assert np.array_equal(side, vec["side"]) and np.array_equal(info, vec["info"]) and side.dtype == np.int32
    print(f"  {key}: kernel of the call with {NRHS} pairs {c['ms']:.3f} ms")
    worst = 0.0
    for b in range(B):
        r = refs[b]
        assert c["st"][b]["returnValue"] == 0 and not (info[b] & 1)
        inW = np.zeros(nd, dtype=bool); inW[r["pos"][r["W"]]] = True
        assert np.array_equal(side[b] != 0, inW) and np.all(db[b][:, ~inW] == 0.0)
        for k in range(NRHS):
            vmax = max(np.abs(c["VX"][b, k]).max(), np.abs(c["VY"][b, k]).max())
            bound = 1e-12 * n * r["cond"] * vmax
            dbr = np.zeros(nd); dbr[r["pos"][r["W"]]] = r["mu"][k]
            e_g = np.abs(dg[b, k] - r["dg"][k]).max(); e_b = np.abs(db[b, k] - dbr).max()
            if bound > 0.0:
                worst = max(worst, max(e_g, e_b) / bound)
            assert e_g <= bound and e_b <= bound, (b, k, e_g, e_b, bound)
        print(f"  {key} instance {b}: |W| = {len(r['W'])}, cond(K) = {r['cond']:.3g}")
    print(f"  {key}: worst error / bound over {B} x {NRHS} columns = {worst:.3g}")
    assert np.any(dg != c["novy"][0])      # vy does enter


# ---- 2: against the vector adjoint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_against_the_vector_adjoint(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, B = SHAPES[key][0], SHAPES[key][3]
    dg, db = c["full"][:2]
    for k in c["cols"]:
        v = c["vec"][k]
        bits = np.array_equal(dg[:, k], v["dg"]) and np.array_equal(db[:, k], v["db"])
        for b in range(B):
            bound = 1e-12 * n * refs[b]["cond"] * max(np.abs(c["VX"][b, k]).max(), np.abs(c["VY"][b, k]).max())
            e_g = np.abs(dg[b, k] - v["dg"][b]).max(); e_b = np.abs(db[b, k] - v["db"][b]).max()
            print(f"  {key} column {k} instance {b}: |blocked - vector| dg {e_g:.3g}, db {e_b:.3g}, bound {bound:.3g}")
            assert e_g <= bound and e_b <= bound
        print(f"  {key} column {k}: equal to the vector adjoint bit for bit: {bits}")
        if key == "fallback":
            assert bits


# ---- 3: columns are independent, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_columns_are_independent(hip, key):
    c = solved_case(key)
    dg, db, side, info = c["full"]
    assert same(c["again"], c["full"])
    for k, part in c["prefix"].items():
        assert np.array_equal(part[0], dg[:, :k]) and np.array_equal(part[1], db[:, :k]), k
        assert np.array_equal(part[2], side) and np.array_equal(part[3], info)
    p = c["perm"]
    assert np.array_equal(c["permuted"][0], dg[:, p]) and np.array_equal(c["permuted"][1], db[:, p])
    assert np.all(dg[:, ZERO_COL] == 0.0) and np.all(db[:, ZERO_COL] == 0.0)
    assert np.any(dg[:, ZERO_COL - 1] != 0.0) and np.any(dg[:, NRHS - 1] != 0.0) and np.any(db[:, NRHS - 1] != 0.0)
    for got, want in zip(c["novy"], c["sens"]):      # vy = None is the blocked sensitivity call
        assert got.tobytes() == want.tobytes()
    for name, got, want in zip(("dg", "db", "side", "info"), c["novx"], c["zerovx"]):      # the skipped forward substitution
        print(f"  {key} {name}: vx = None equal to vx = 0: {np.array_equal(got, want)}")
        assert np.array_equal(got, want)
    assert np.any(c["novx"][0] != 0.0)


# ---- 4: the dual Jacobian -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_dual_jacobian(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, nC, nComp, B = SHAPES[key][:4]
    nd = n + nC + 2 * nComp
    Jg, Jb, side, info = c["jac"]
    Jyg, Jyb, dside, dinfo = c["jd"]
    assert Jyg.shape == (B, nd, n) and Jyb.shape == (B, nd, nd) and np.array_equal(dside, side) and np.array_equal(dinfo, info)
    print(f"  {key}: kernels of the dual Jacobian {c['jd_ms']:.3f} ms")
    for b in range(B):
        r = refs[b]
        d = c["ds"][b]
        bound = 1e-12 * n * r["cond"]
        pw = r["pos"][r["W"]]
        inW = np.zeros(nd, dtype=bool); inW[pw] = True
        assert np.all(Jyg[b][~inW] == 0.0) and np.all(Jyb[b][~inW] == 0.0) and np.all(Jyb[b][:, ~inW] == 0.0)
        assert np.all(np.any(Jyb[b][inW] != 0.0, axis=1))
        sr = c["ws"][b]["slot_row"][:c["ws"][b]["ns"]]
        print(f"  {key} instance {b}: n_s = {len(sr)}, free slots below n_s: {np.flatnonzero(sr < 0).tolist()}")
        e_t = np.abs(Jyg[b] - Jb[b].T).max()
        sym = np.abs(Jyb[b] - Jyb[b].T).max()
        EW = r["E"][r["W"]]
        S = np.linalg.inv(EW @ np.linalg.solve(d["Q"], EW.T))
        blockWW = Jyb[b][np.ix_(pw, pw)]
        e_s = np.abs(blockWW - S).max()
        lam = np.linalg.eigvalsh(0.5 * (blockWW + blockWW.T))[0] if len(pw) else 1.0
        print(f"  {key} instance {b}: |W| = {len(pw)}, |Jyg - Jb'| {e_t:.3g}, |Jyb - Jyb'| {sym:.3g}, |Jyb_WW - (E_W Q^-1 E_W')^-1| {e_s:.3g}, "
              f"bound {bound:.3g}; smallest eigenvalue of Jyb_WW {lam:.3g}")
        assert e_t <= bound and sym <= bound and e_s <= bound and lam > 0.0
        # the unit vectors of W through the panel call: the same bits
        k = len(c["posW"][b])
        assert np.array_equal(c["posW"][b], np.sort(pw))
        assert np.array_equal(c["units"][0][b, :k], Jyg[b][c["posW"][b]]) and np.array_equal(c["units"][1][b, :k], Jyb[b][c["posW"][b]])
    # the j-th occupied slot is slot j unless a slot below n_s is free: these two cases have such slots, and without them a unit vector
    # written at slot j would pass everything above
    if key in ("np128", "np256_box"):
        assert any(np.any(w["slot_row"][:w["ns"]] < 0) for w in c["ws"])
    assert c["jd_nobounds"][1] is None and np.array_equal(c["jd_nobounds"][0], Jyg)
    for full, part, one, partial in zip(c["jd"], c["jd_part"], c["jd_one"], c["jd_partial"]):
        assert np.array_equal(part, full[1:]) and np.array_equal(one, full) and np.array_equal(partial, full)


# ---- 5: central differences of y* ----------------------------------------------------------------------------------------------------
def fd_bound_y(tol, Q, EW, vyW):
    """the y part of tests/test_gpu_adjoint.py::fd_bounds"""
    ev = np.linalg.eigvalsh(Q)
    return tol * np.sqrt(Q.shape[0] * ev[-1] / ev[0]) * np.abs(vyW).sum() / (H_FD * np.linalg.svd(EW, compute_uv=False)[-1])


@pytest.mark.parametrize("n,nC,nComp", [(40, 20, 8), (200, 330, 37)])
def test_central_differences_of_the_duals(hip, n, nC, nComp):
    B = 8
    nd = n + nC + 2 * nComp
    opt = hip.default_options(perturbStep=0)
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    load_all(bt, ds)
    bt.run()
    x0, y0, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    Jyg, Jyb, side, info = bt.jacobian_duals()
    W0 = [working_rows(bt.read_working_set(b)) for b in range(B)]
    bt.close()
    rng = np.random.default_rng(6)
    vy = rng.standard_normal((B, nd))
    # two directions: one in g; one in the bounds two active rows of A sit on (both bounds of an equality row move together)
    zg = rng.standard_normal((B, n))
    rowsA, coef = [], rng.standard_normal((B, 2))
    for b in range(B):
        act = W0[b][W0[b] < nC]
        rowsA.append(act[:2])      # (an instance with fewer active rows of A moves those it has)
    print(f"  ({n},{nC},{nComp}): active rows of A moved per instance {[len(r) for r in rowsA]}")
    assert sum(len(r) == 2 for r in rowsA) >= B // 2
    bounds = []
    for b, d in enumerate(ds):
        E, pos = rows_and_bounds(d)
        bounds.append(fd_bound_y(opt.stationarityTolerance, d["Q"], E[W0[b]], vy[b][pos[W0[b]]]))
    groups = {}
    for b in range(B):
        groups.setdefault(st[b]["rhoOpt"], []).append(b)

    def moved(b, which, sgn):
        d = dict(ds[b], x0=x0[b], y0=y0[b])
        if which == "g":
            d["g"] = d["g"] + sgn * H_FD * zg[b]
        else:
            lbA, ubA = d["lbA"].copy(), d["ubA"].copy()
            for r, cf in zip(rowsA[b], coef[b]):
                s = side[b][n + r]
                if s in (-1, 2): lbA[r] += sgn * H_FD * cf
                if s in (1, 2): ubA[r] += sgn * H_FD * cf
            d["lbA"], d["ubA"] = lbA, ubA
        return d

    def perturbed_solves(which, sgn):
        val, keep = np.zeros(B), np.zeros(B, dtype=bool)
        for rho, members in groups.items():
            o = hip.default_options(perturbStep=0, solveZeroPenaltyFirst=0, initialPenaltyParameter=rho)
            bs = hip.BatchLCQP(len(members), n, nC, nComp, opt=o)
            load_all(bs, [moved(b, which, sgn) for b in members])
            bs.run()
            xs, ys, sts = bs.solution()
            for i, b in enumerate(members):
                keep[b] = sts[i]["returnValue"] == 0 and np.array_equal(working_rows(bs.read_working_set(i)), W0[b])
                val[b] = vy[b] @ ys[i]
            bs.close()
        return val, keep

    for which in ("g", "bounds"):
        vp, kp = perturbed_solves(which, +1.0); vm, km = perturbed_solves(which, -1.0)
        keep = kp & km & (info == 0)
        fd = (vp - vm) / (2 * H_FD)
        if which == "g":
            pred = np.array([vy[b] @ (Jyg[b] @ zg[b]) for b in range(B)])
        else:
            pred = np.array([vy[b] @ (Jyb[b][:, n + rowsA[b]] @ coef[b][:len(rowsA[b])]) for b in range(B)])
        err = np.abs(fd - pred)
        for b in range(B):
            print(f"  ({n},{nC},{nComp}) d/d{which} instance {b}: fd {fd[b]:+.9e} predicted {pred[b]:+.9e} err {err[b]:.3g} "
                  f"(rel {err[b] / max(abs(pred[b]), 1e-300):.3g}) bound {bounds[b]:.3g} kept {bool(keep[b])}")
        assert np.count_nonzero(~keep) <= B // 4, keep
        assert np.all(err[keep] <= np.array(bounds)[keep])
        assert np.any(pred != 0.0)


# ---- 6: state and flags -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True])
def test_the_calls_change_nothing(hip, warm):
    n, nC, nComp, B = 40, 20, 8, 5
    nd = n + nC + 2 * nComp
    opt = hip.default_options()
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    ds2 = [perturbed(d, 300 + b) for b, d in enumerate(ds)]
    out = []
    for with_calls in (True, False):
        bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
        load_all(bt, ds)
        bt.run()
        first = result(bt)
        if with_calls:
            counts = bt.launch_counts()
            rng = np.random.default_rng(1)
            VX, VY = rng.standard_normal((B, PANEL + 2, n)), rng.standard_normal((B, PANEL + 2, nd))
            bt.adjoint_blocked(VX, VY); bt.adjoint_blocked(None, VY); bt.jacobian_duals(); bt.jacobian_duals(_staging_bytes=1)
            assert bt.launch_counts() == counts
            again = result(bt)
            assert_same_bits(first, again)
            assert np.array_equal(first["work"], again["work"])
        update_all(bt, ds2)
        bt.resolve(warm=warm)
        out.append(result(bt))
        assert bt.launch_counts() == (1, 2)
        bt.close()
    assert_same_bits(out[0], out[1])
    assert np.array_equal(out[0]["work"], out[1]["work"])


def test_flag_of_a_failed_instance(hip):
    ds = [P.warm_up_w_A(), P.infeasible(), P.warm_up_w_A()]      # lbA > ubA in the middle
    bt = hip.BatchLCQP(3, 2, 1, 1, opt=hip.default_options())
    load_all(bt, ds)
    bt.run()
    st = bt.solution()[2]
    assert st[0]["returnValue"] == 0 and st[1]["returnValue"] != 0 and st[2]["returnValue"] == 0
    VX, VY = np.ones((3, 2, 2)), np.ones((3, 2, 5))
    dg, db, side, info = bt.adjoint_blocked(VX, VY)
    Jyg, Jyb, jside, jinfo = bt.jacobian_duals()
    bt.close()
    # the same calls on a batch without the failed instance
    clean = hip.BatchLCQP(2, 2, 1, 1, opt=hip.default_options())
    load_all(clean, [ds[0], ds[2]])
    clean.run()
    assert all(s["returnValue"] == 0 for s in clean.solution()[2])
    cdg, cdb, cside, cinfo = clean.adjoint_blocked(VX[[0, 2]], VY[[0, 2]])
    cJyg, cJyb, _, _ = clean.jacobian_duals()
    clean.close()
    print("  info", info, jinfo, "without the failed instance", cinfo)
    assert info[1] == 1 and jinfo[1] == 1 and not (info[0] & 1) and not (info[2] & 1) and np.array_equal(info, jinfo)
    assert np.all(dg[1] == 0.0) and np.all(db[1] == 0.0) and np.all(Jyg[1] == 0.0) and np.all(Jyb[1] == 0.0) and np.all(side[1] == 0)
    # the neighbours keep their bits
    for got, want in ((dg, cdg), (db, cdb), (side, cside), (info, cinfo), (Jyg, cJyg), (Jyb, cJyb)):
        assert np.array_equal(got[[0, 2]], want)
    assert np.any(dg[0] != 0.0) and np.any(Jyb[0] != 0.0)


def test_a_batch_that_never_ran_is_refused(hip):
    from lcqpow_amd import capi
    n, nC, nComp = 40, 20, 8
    nd = n + nC + 2 * nComp
    d = random_lcqp(np.random.default_rng(1000), n, nC, nComp, False, False)
    bt = hip.BatchLCQP(1, n, nC, nComp)
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    vx, vy, dg, Jyg = np.ones(n), np.ones(nd), np.full(n, 7.0), np.full((nd, n), 7.0)
    L = capi.lib()
    adj = lambda: L.lcqp_hip_batch_adjoint_blocked(bt.h, 1, p(vx), p(vy), p(dg), None, None, None)
    jac = lambda: L.lcqp_hip_batch_jacobian_duals(bt.h, 0, 1, p(Jyg), None, None, None)
    assert adj() == 300 and jac() == 300
    load_all(bt, [d])
    assert adj() == 300 and jac() == 300 and np.all(dg == 7.0) and np.all(Jyg == 7.0)
    bt.run()
    assert adj() == 0 and jac() == 0 and not np.any(dg == 7.0) and not np.any(Jyg == 7.0)
    dg[:] = 7.0; Jyg[:] = 7.0
    for first, count in ((-1, 1), (0, 0), (0, -2), (0, 2), (1, 1), (2, 1)):      # outside the batch of one
        assert L.lcqp_hip_batch_jacobian_duals(bt.h, first, count, p(Jyg), None, None, None) == 100, (first, count)
    assert L.lcqp_hip_batch_jacobian_duals(bt.h, 0, 1, None, None, None, None) == 100
    assert L.lcqp_hip_batch_adjoint_blocked(bt.h, 0, p(vx), p(vy), p(dg), None, None, None) == 100
    assert L.lcqp_hip_batch_adjoint_blocked(bt.h, 1, None, None, p(dg), None, None, None) == 100
    assert L.lcqp_hip_batch_adjoint_blocked(bt.h, 1, p(vx), p(vy), None, None, None, None) == 100
    assert L.lcqp_hip_batch_adjoint_blocked(bt.h, 1, None, p(vy), p(dg), None, None, None) == 0 and not np.any(dg == 7.0)
    dg[:] = 7.0
    assert np.all(Jyg == 7.0)      # the refusals wrote nothing
    load_all(bt, [d])
    assert adj() == 300 and jac() == 300 and np.all(dg == 7.0)
    bt.close()


# ---- 7: the device twins ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["np128", "np256_box", "fallback"])
def test_device_twins_return_the_bits_of_the_host_calls(hip, key):
    import torch
    n, nC, nComp, B, box, shifted, eq = SHAPES[key]
    nd = n + nC + 2 * nComp
    ds = problems_of(key)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    rng = np.random.default_rng(80)
    k = PANEL + 3
    VX, VY = rng.standard_normal((B, k, n)), rng.standard_normal((B, k, nd))
    dev = lambda a: torch.as_tensor(a, device="cuda:0")
    host = lambda r: [None if t is None else t.cpu().numpy() for t in r]
    for vx, vy in ((VX, VY), (None, VY), (VX, None)):
        want = bt.adjoint_blocked(vx, vy)
        got = host(bt.adjoint_blocked_device(None if vx is None else dev(vx), None if vy is None else dev(vy)))
        assert same(got, want), (vx is None, vy is None)
    for name in ("jacobian", "jacobian_duals"):
        want = getattr(bt, name)()
        got = host(getattr(bt, name + "_device")())
        assert same(got, want), name
        ms = bt.sensitivity_kernel_ms()
        print(f"  {key} {name}_device: kernel {ms:.3f} ms")
        part = host(getattr(bt, name + "_device")(first=1, count=B - 1, bounds=False))
        assert part[1] is None and np.array_equal(part[0], want[0][1:]) and np.array_equal(part[2], want[2][1:])
    if n <= 512:
        # one instance per launch: the same bits, and the timing call reports the sum over the B launches like the host twin's, not the
        # last one (1 / B of it, B >= 3 here: half the host figure separates the two whatever the events' noise)
        bt._call("set_jacobian_staging", 1)
        try:
            for name in ("jacobian", "jacobian_duals"):
                want = getattr(bt, name)()
                ms_host = bt.sensitivity_kernel_ms()
                got = host(getattr(bt, name + "_device")())
                ms_dev = bt.sensitivity_kernel_ms()
                print(f"  {key} {name} in {B} chunks: kernels {ms_host:.4f} ms (host call), {ms_dev:.4f} ms (device call)")
                assert same(got, want) and ms_dev > 0.5 * ms_host
        finally:
            bt._call("set_jacobian_staging", 0)
    # refusals, as the existing _device calls refuse
    L = hip.lib()
    Jyg = torch.empty((B, nd, n), dtype=torch.float64, device="cuda:0")
    pinned = torch.empty((B, nd, n), dtype=torch.float64).pin_memory()
    assert L.lcqp_hip_batch_jacobian_duals_device(bt.h, 0, B, pinned.data_ptr(), None, None, None, None) == 100 and "Jyg: not a device pointer" in bt._last_error()
    assert L.lcqp_hip_batch_jacobian_device(bt.h, 0, B, pinned.data_ptr(), None, None, None, None) == 100 and "Jg: not a device pointer" in bt._last_error()
    pv = torch.empty((B, 1, nd), dtype=torch.float64).pin_memory()
    dg = torch.empty((B, 1, n), dtype=torch.float64, device="cuda:0")
    assert L.lcqp_hip_batch_adjoint_blocked_device(bt.h, 1, None, pv.data_ptr(), dg.data_ptr(), None, None, None, None) == 100 and "vy: not a device pointer" in bt._last_error()
    raw = torch.empty(2 * B * nd * n + 2, dtype=torch.int32, device="cuda:0")
    assert L.lcqp_hip_batch_jacobian_duals_device(bt.h, 0, B, raw[1:].data_ptr(), None, None, None, None) == 100 and "Jyg: not aligned to 8 bytes" in bt._last_error()
    assert L.lcqp_hip_batch_jacobian_duals_device(bt.h, 0, B + 1, Jyg.data_ptr(), None, None, None, None) == 100
    assert L.lcqp_hip_batch_adjoint_blocked_device(bt.h, 1, None, None, dg.data_ptr(), None, None, None, None) == 100
    bt.close()


def test_device_jacobians_of_a_sub_range_in_uneven_chunks(hip):
    """instances 1 .. 3 of five under a staging cap that holds two: a chunk of two, then a partial one, from a start that is not zero.  The
    device twins return the host calls' bits under that cap and rows 1 .. 3 of the host calls under the default cap, write nothing in front
    of or behind their range, and report the kernel time of both chunks (test_device_twins_return_the_bits_of_the_host_calls argues the half)."""
    import torch
    n, nC, nComp = SHAPES["np128"][:3]
    B, first, count = 5, 1, 3
    nd = n + nC + 2 * nComp
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    su = bt.read_setup(0)
    caps = {"jacobian": 8 * n * (n + su["np"] + nd + 2 * su["capS"]) * 2, "jacobian_duals": dual_staging_bytes(su, nd, 2)}
    rows = {"jacobian": n, "jacobian_duals": nd}
    GUARD_F, GUARD_I = -7.25, 77
    dev = torch.device("cuda", 0)
    try:
        for name in ("jacobian", "jacobian_duals"):
            for bounds in (True, False):
                bt._call("set_jacobian_staging", 0)
                whole = getattr(bt, name)(bounds=bounds)
                bt._call("set_jacobian_staging", caps[name])
                want = getattr(bt, name)(first=first, count=count, bounds=bounds)
                ms_host = bt.sensitivity_kernel_ms()
                Jg = torch.full((count + 2, rows[name], n), GUARD_F, dtype=torch.float64, device=dev)
                Jb = torch.full((count + 2, rows[name], nd), GUARD_F, dtype=torch.float64, device=dev) if bounds else None
                side = torch.full((count + 2, nd), GUARD_I, dtype=torch.int32, device=dev)
                info = torch.full((count + 2,), GUARD_I, dtype=torch.int32, device=dev)
                bt._call(name + "_device", first, count, Jg[1:].data_ptr(), Jb[1:].data_ptr() if bounds else None, side[1:].data_ptr(),
                         info[1:].data_ptr(), bt._stream())
                ms_dev = bt.sensitivity_kernel_ms()
                print(f"  {name} bounds={bounds}, chunks of 2 and 1: kernels {ms_host:.4f} ms (host call), {ms_dev:.4f} ms (device call)")
                for t, w, full, guard in ((Jg, want[0], whole[0], GUARD_F), (Jb, want[1], whole[1], GUARD_F), (side, want[2], whole[2], GUARD_I),
                                          (info, want[3], whole[3], GUARD_I)):
                    if t is None:
                        assert w is None and full is None
                        continue
                    got = t.cpu().numpy()
                    assert np.array_equal(got[1:-1], w), (name, bounds)
                    assert np.array_equal(got[1:-1], full[first:first + count]), (name, bounds)
                    assert np.all(got[0] == guard) and np.all(got[-1] == guard), (name, bounds)
                assert ms_dev > 0.5 * ms_host
    finally:
        bt._call("set_jacobian_staging", 0)
    bt.close()


def test_layer_jacobian_with_duals(hip):
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    n, nC, nComp, B = 40, 20, 8, 4
    nd = n + nC + 2 * nComp
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64, device="cuda:0", requires_grad=True)
    x, y = layer.solve(g)
    assert layer.last_path == "device"
    J = layer.jacobian(duals=True)
    assert layer.last_path == "device" and all(J[k].is_cuda for k in ("xg", "xb", "yg", "yb", "side"))
    assert J["xg"].shape == (B, n, n) and J["xb"].shape == (B, n, nd) and J["yg"].shape == (B, nd, n) and J["yb"].shape == (B, nd, nd)
    plain = layer.jacobian()      # duals=False: what it returned before, the host call's Jg on the device of g
    assert isinstance(plain, torch.Tensor) and plain.device == g.device and np.array_equal(plain.cpu().numpy(), bt.jacobian(bounds=False)[0])
    assert np.array_equal(J["xg"].cpu().numpy(), plain.cpu().numpy())
    ws = [working_rows(bt.read_working_set(b)) for b in range(B)]
    conds = []
    for b in range(B):
        E, pos = rows_and_bounds(ds[b])
        conds.append(kkt_adjoint_reference(ds[b]["Q"], E[ws[b]], np.zeros((n, 1)), np.zeros((len(ws[b]), 1)), extended=False)[2])
    # rows from autograd on (x, y): d x_k / d g and d y_r / d g for a few k and r in W
    for b in range(B):
        r = int(n + ws[b][ws[b] < nC + 2 * nComp][0])
        for out, i, blk in ((x, 3, "xg"), (y, r, "yg")):
            (row,) = torch.autograd.grad(out[b, i], g, retain_graph=True)
            err = (row[b] - J[blk][b, i]).abs().max().item()
            bound = 1e-12 * n * conds[b]      # the bound of check 1 for a unit row
            print(f"  instance {b} {blk} row {i}: |autograd - jacobian| {err:.3g}, bound {bound:.3g}")
            assert err <= bound and torch.any(row[b] != 0)
    # on the host path the same call returns host tensors with the host calls' bits
    gh = torch.tensor(stack(ds, "g"), dtype=torch.float64, requires_grad=True)
    layer.solve(gh)
    Jh = layer.jacobian(duals=True)
    assert layer.last_path == "host" and not Jh["yg"].is_cuda and np.array_equal(Jh["yg"].numpy(), bt.jacobian_duals()[0])
    bt.close()
