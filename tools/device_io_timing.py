"""Wall clock of the host-pointer entry points of the dense batch beside their device-pointer twins (DESIGN.md section 3a'''''), on ONE
handle in one process, at the BASELINE shape (B = 1024, nV = 256, nC = 512, nComp = 64; --quick: B = 128):

  load                               against load_device, Q and A shared by the batch (the host path broadcasts them first, as the torch layer does)
  update + resolve(warm) + solution  against update_device + resolve(warm) + solution_device
  adjoint, per-instance Q            against adjoint_device

Every figure is the wall clock of the calls including what makes their results usable: the host calls return finished results, the device
calls are followed by a synchronisation of the torch stream.  min / median / max over --reps calls after --warmup calls.

--sparse: the same three rows for the sparse arm (lcqp_hip_sparse_*), with per-instance value arrays, on the banded synthetic workload of
lcqpow_amd/synth_sparse.py at two shapes -- n = 4096, nC = 2048, nComp = 512 with B = 4096 and n = 512, nC = 256, nComp = 64 with B = 1024
(--quick: B = 64 each) --, followed by the kernel times of the three pack kernels (HIP events on the torch stream around load_device and
update_device; the check kernel and its status read are inside) and the bytes per second of k_sparse_pack_values.

--sparse --blocked: the full solution map of the sparse arm instead -- jacobian() + jacobian_duals() (host arrays out) against jacobian_device()
+ jacobian_duals_device() (device tensors out, DESIGN.md section 3a''''', "The sparse arm: panels and Jacobians into device arrays") on one
handle, the two pairs alternating call by call, at (512, 256, 64) with B = 64 and (64, 32, 8) with B = 1024 (--quick: B = 8 and 64) --, then
the device pair's time on the stream by HIP events beside the kernel time of its panel launches: the difference is k_sparse_scatter_panels
with the zero-fill of the dual blocks and the copies of side and info, given as a share of the pair and as bytes per second.

usage: python tools/device_io_timing.py [--sparse [--blocked]] [--quick] [--log FILE] [--reps 10] [--warmup 2]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402


def timed(call, reps, warmup):
    out = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    t = np.array(out[warmup:])
    return t.min(), float(np.median(t)), t.max()


HBM_PEAK = 8.0e12      # bytes per second of one MI355X


def sparse_rows(say, args, shape, B):
    from lcqpow_amd import synth_sparse as S
    n, nC, nK = shape
    m = nC + 2 * nK
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
    h = {k: np.stack([d[k] for d in inst]) for k in ("Qx", "g", "Ex", "lbA", "ubA")}
    del inst
    dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda:0")
    d = {k: dev(v) for k, v in h.items()}
    say(f"sparse, banded workload: B = {B}, nV = {n}, nC = {nC}, nComp = {nK}, nnzQ = {sb.nnzQ}, nnzA = {sb.nnzA}, lanes = {sb.lanes()}; "
        f"{args.reps} calls after {args.warmup}; wall clock, ms: min / median / max")

    def row(name, host, device):
        th, td = timed(host, args.reps, args.warmup), timed(device, args.reps, args.warmup)
        verdict = "" if td[1] < th[1] else "    DEVICE MEDIAN NOT BELOW HOST"
        say(f"  {name:<44s} host {th[0]:9.2f} / {th[1]:9.2f} / {th[2]:9.2f}    device {td[0]:9.2f} / {td[1]:9.2f} / {td[2]:9.2f}    median ratio {th[1] / td[1]:7.1f}{verdict}")

    def load_host():
        assert sb.load(0, B, h["Qx"], h["g"], h["Ex"], lbA=h["lbA"], ubA=h["ubA"]) == 0

    def load_device():
        assert sb.load_device(0, B, d["Qx"], d["g"], d["Ex"], lbA=d["lbA"], ubA=d["ubA"]) == 0

    row("load", load_host, load_device)
    sb.run()
    sb.synchronize()
    say("  (run on the loaded data: setup %.2f ms + homotopy %.2f ms of kernel time)" % sb.last_timing())

    def resolve_host():
        assert sb.update(0, B, h["g"], lbA=h["lbA"], ubA=h["ubA"]) == 0
        sb.resolve(warm=True)
        sb.solution()

    def resolve_device():
        assert sb.update_device(0, B, d["g"], lbA=d["lbA"], ubA=d["ubA"]) == 0
        sb.resolve(warm=True)
        sb.solution_device()

    row("update + resolve(warm) + solution", resolve_host, resolve_device)
    sb.synchronize()
    say("  (the warm re-solve alone: setup %.2f ms + homotopy %.2f ms of kernel time)" % sb.last_timing())

    rng = np.random.default_rng(0)
    vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    dvx, dvy = dev(vx), dev(vy)
    out = dict(Q=torch.empty((B, sb.nnzQ), dtype=torch.float64, device="cuda:0"), A=torch.empty((B, sb.nnzA), dtype=torch.float64, device="cuda:0"))
    row("adjoint, per-instance dQx and dAx", lambda: sb.adjoint(vx, vy), lambda: sb.adjoint_device(dvx, dvy, out=out))
    say("  (kernel time of the last adjoint_device: %.3f ms)" % sb.sensitivity_kernel_ms())

    # the pack kernels by HIP events on the torch stream: the whole call (check kernel, its status read, the pack kernels), and from the
    # difference of a load with and without value arrays the time of k_sparse_pack_values
    def events(call):
        ts = []
        for _ in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); call(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts[args.warmup:]))
    t_load = events(load_device)
    t_vec = events(lambda: sb.load_device(0, B, None, d["g"], None, lbA=d["lbA"], ubA=d["ubA"]))
    t_upd = events(lambda: sb.update_device(0, B, d["g"], lbA=d["lbA"], ubA=d["ubA"]))
    moved = 8.0 * B * (2 * sb.nnzQ + 2 * sb.nnzA) + 4.0 * sb.nnzA      # values read and written once, the map (it stays in cache)
    t_val = max(t_load - t_vec, 1e-6)
    say(f"  event time on the stream, median, ms: load_device {t_load:.3f} (k_sparse_check_vectors with the diagonal pairs + status read + k_sparse_pack_values + "
        f"k_sparse_pack_vectors), load_device without value arrays {t_vec:.3f} (check + status read + k_sparse_pack_vectors), update_device {t_upd:.3f}")
    say(f"  k_sparse_pack_values (the difference; it includes the diagonal pairs of the check kernel): {t_val:.3f} ms for {moved / 1e9:.3f} GB = "
        f"{moved / (t_val * 1e-3) / 1e9:.0f} GB/s = {100.0 * moved / (t_val * 1e-3) / HBM_PEAK:.1f} % of the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s")
    sb.close()


def blocked_rows(say, args, shape, B):
    from lcqpow_amd import synth_sparse as S
    n, nC, nK = shape
    m = nC + 2 * nK
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
    h = {k: np.stack([d[k] for d in inst]) for k in ("Qx", "g", "Ex", "lbA", "ubA")}
    del inst
    assert sb.load(0, B, h["Qx"], h["g"], h["Ex"], lbA=h["lbA"], ubA=h["ubA"]) == 0
    sb.run()
    sb.synchronize()
    say(f"sparse, banded workload: B = {B}, nV = {n}, nC = {nC}, nComp = {nK}, m = {m}, lanes = {sb.lanes()}, panel = {sb.sens_panel()}; the solution map is "
        f"B (n + m)^2 = {8.0 * B * (n + m) ** 2 / 1e6:.0f} MB; {args.reps} alternating calls of each pair after {args.warmup}; wall clock, ms: min / median / max")
    host_pair = lambda: (sb.jacobian(), sb.jacobian_duals())
    device_pair = lambda: (sb.jacobian_device(), sb.jacobian_duals_device())
    th, td = [], []
    for k in range(args.warmup + args.reps):      # host, device, host, device, ...: what the machine does meanwhile hits both
        for pair, ts in ((host_pair, th), (device_pair, td)):
            th_, _, _ = timed(pair, 1, 0)
            ts.append(th_)
    th, td = np.array(th[args.warmup:]), np.array(td[args.warmup:])
    verdict = "" if np.median(td) < np.median(th) else "    DEVICE MEDIAN NOT BELOW HOST"
    say(f"  {'jacobian + jacobian_duals':<44s} host {th.min():9.2f} / {np.median(th):9.2f} / {th.max():9.2f}    device {td.min():9.2f} / {np.median(td):9.2f} / {td.max():9.2f}"
        f"    median ratio {np.median(th) / np.median(td):7.1f}{verdict}")
    # the same bits from both pairs
    (hg, hb, hs, hi), (hyg, hyb, _, _) = host_pair()
    (dg, db, ds, di), (dyg, dyb, _, _) = device_pair()
    torch.cuda.synchronize()
    for want, got in ((hg, dg), (hb, db), (hs, ds), (hi, di), (hyg, dyg), (hyb, dyb)):
        assert want.tobytes() == got.cpu().numpy().tobytes()
    rowsW = int(np.count_nonzero(hs))
    del hg, hb, hyg, hyb, dg, db, dyg, dyb
    # the device pair on the stream: HIP events around it; the panel kernels by the library's own events
    ev, ker = [], []
    for k in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); device_pair(); e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
        sb.jacobian_device(); k1 = sb.sensitivity_kernel_ms()
        sb.jacobian_duals_device(); ker.append(k1 + sb.sensitivity_kernel_ms())
    ev, ker = np.array(ev[args.warmup:]), np.array(ker[args.warmup:])
    rest = max(float(np.median(ev) - np.median(ker)), 1e-6)
    copied = 8.0 * (n + m) * (B * n + rowsW)                 # doubles the scatter kernel reads once and writes once
    filled = 8.0 * (n + m) * B * m                           # the zero-fill of Jyg and Jyb
    say(f"  device pair on the stream, ms: HIP events {ev.min():.3f} / {np.median(ev):.3f} / {ev.max():.3f}; its panel kernels {ker.min():.3f} / {np.median(ker):.3f} / {ker.max():.3f}")
    say(f"  the rest (k_sparse_scatter_panels + zero-fill of the dual blocks + side / info + launch gaps): {rest:.3f} ms = {100.0 * rest / np.median(ev):.1f} % of the pair; "
        f"it reads {copied / 1e6:.0f} MB and writes {(copied + filled) / 1e6:.0f} MB: {(2 * copied + filled) / (rest * 1e-3) / 1e9:.0f} GB/s = "
        f"{100.0 * (2 * copied + filled) / (rest * 1e-3) / HBM_PEAK:.1f} % of the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s")
    sb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--blocked", action="store_true", help="with --sparse: jacobian() + jacobian_duals() against their device twins")
    ap.add_argument("--log")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    B, n, nC, nK = (128 if args.quick else 1024), 256, 512, 64
    nd = n + nC + 2 * nK
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write_log():
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.sparse and args.blocked:
        say("device_io_timing --sparse --blocked: the solution map of the sparse batch into host arrays and into device tensors, one handle per shape, one process")
        for shape, Bs, Bq in (((512, 256, 64), 64, 8), ((64, 32, 8), 1024, 64)):
            blocked_rows(say, args, shape, Bq if args.quick else Bs)
            write_log()
        return
    if args.sparse:
        say("device_io_timing --sparse: host entry points of the sparse batch against their device-pointer twins, one handle per shape, one process")
        for shape, Bs in (((4096, 2048, 512), 4096), ((512, 256, 64), 1024)):
            sparse_rows(say, args, shape, 64 if args.quick else Bs)
            write_log()
        return

    bt = la.BatchLCQP(B, n, nC, nK, opt=la.default_options(perturbStep=0, printLevel=0))
    bt.generate_synthetic(0)
    bt.run()
    ps = [bt.read_problem(b) for b in range(B)]
    h = {k: np.stack([p[k] for p in ps]) for k in ("Q", "g", "L", "R", "A", "lbA", "ubA")}
    Q1, A1 = h["Q"][0].copy(), h["A"][0].copy()      # one Q and one A for the batch
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")
    d = {k: dev(v) for k, v in h.items()}
    dQ1, dA1 = dev(Q1), dev(A1)
    say(f"device_io_timing: B = {B}, nV = {n}, nC = {nC}, nComp = {nK}; {args.reps} calls after {args.warmup}; wall clock, ms: min / median / max")

    def row(name, host, device):
        th, td = timed(host, args.reps, args.warmup), timed(device, args.reps, args.warmup)
        say(f"  {name:<44s} host {th[0]:9.2f} / {th[1]:9.2f} / {th[2]:9.2f}    device {td[0]:9.2f} / {td[1]:9.2f} / {td[2]:9.2f}    median ratio {th[1] / td[1]:7.1f}")

    def load_host():
        Qb = np.ascontiguousarray(np.broadcast_to(Q1, (B, n, n))); Ab = np.ascontiguousarray(np.broadcast_to(A1, (B, nC, n)))
        assert bt.load(0, B, Qb, h["g"], h["L"], h["R"], A=Ab, lbA=h["lbA"], ubA=h["ubA"]) == 0

    def load_device():
        assert bt.load_device(0, B, dQ1, d["g"], d["L"], d["R"], A=dA1, lbA=d["lbA"], ubA=d["ubA"]) == 0

    row("load, Q and A shared", load_host, load_device)
    # back to the instances' own Q and A for what follows (instance 0's A under the other instances' bounds is not a feasible problem,
    # and an infeasible instance runs the homotopy to its iteration limit)
    assert bt.load_device(0, B, d["Q"], d["g"], d["L"], d["R"], A=d["A"], lbA=d["lbA"], ubA=d["ubA"]) == 0
    bt.run()
    bt.synchronize()
    say("  (run on the loaded data: setup %.2f ms + homotopy %.2f ms of kernel time)" % bt.last_timing())

    def resolve_host():
        assert bt.update(0, B, h["g"], lbA=h["lbA"], ubA=h["ubA"]) == 0
        bt.resolve(warm=True)
        bt.solution()

    def resolve_device():
        assert bt.update_device(0, B, d["g"], lbA=d["lbA"], ubA=d["ubA"]) == 0
        bt.resolve(warm=True)
        bt.solution_device()

    row("update + resolve(warm) + solution", resolve_host, resolve_device)
    bt.synchronize()
    say("  (the warm re-solve alone: setup %.2f ms + homotopy %.2f ms of kernel time)" % bt.last_timing())

    rng = np.random.default_rng(0)
    vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, nd))
    dvx, dvy = dev(vx), dev(vy)
    out = dict(Q=torch.empty((B, n, n), dtype=torch.float64, device="cuda:0"))
    row("adjoint, per-instance Q", lambda: bt.adjoint(vx, vy, matrices=("Q",)), lambda: bt.adjoint_device(dvx, dvy, matrices=("Q",), out=out))
    say("  (kernel time of the last adjoint_device: %.3f ms)" % bt.sensitivity_kernel_ms())
    bt.close()
    write_log()


if __name__ == "__main__":
    main()
