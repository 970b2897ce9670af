"""Wall clock of the host-pointer entry points of the dense batch beside their device-pointer twins (DESIGN.md section 3a'''''), on ONE
handle in one process, at the BASELINE shape (B = 1024, nV = 256, nC = 512, nComp = 64; --quick: B = 128):

  load                               against load_device, Q and A shared by the batch (the host path broadcasts them first, as the torch layer does)
  update + resolve(warm) + solution  against update_device + resolve(warm) + solution_device
  adjoint, per-instance Q            against adjoint_device

Every figure is the wall clock of the calls including what makes their results usable: the host calls return finished results, the device
calls are followed by a synchronisation of the torch stream.  min / median / max over --reps calls after --warmup calls.

usage: python tools/device_io_timing.py [--quick] [--log FILE] [--reps 10] [--warmup 2]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
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
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
