"""One model, B initial conditions: an ordinary dense batch loaded with shared=15 (leg a) against a batch that holds one set of
matrices (leg b), at the headline shape.  Per leg: setup ms and homotopy-kernel ms (last_timing), LCQPs/s of run() wall to wall, and
device_bytes; minimum / median / maximum over the timed runs after the warm-up runs.  One JSON line per leg.
    python tools/shared_bench.py [--batch 1024] [--runs 7] [--warmup 2] [--legs ab]
Q, A, L, R are instance 0's of a generated batch; g is each instance's own draw; lbA / ubA are instance 0's widened per instance (below).
--legs a runs on a build without shared batches too (the parent commit's)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--legs", default="ab")
ap.add_argument("--shape", type=int, nargs=3, default=(256, 512, 64))
args = ap.parse_args()

import torch      # noqa: E402 -- before the library is first loaded: one HIP runtime
import lcqpow_amd as la      # noqa: E402

n, nC, nComp = args.shape
B = args.batch
opt = la.default_options(printLevel=0)
src = la.BatchLCQP(B, n, nC, nComp, opt=opt)
src.generate_synthetic(0)
src.synchronize()
probs = [src.read_problem(b) for b in range(B)]
src.close()
dev = torch.device("cuda", 0)
mats = {k: torch.as_tensor(probs[0][k], device=dev) for k in ("Q", "A", "L", "R")}
# g is the generator's draw of each instance.  Its bounds are not taken over: the generator places lbA, ubA of instance b around
# A_b x*_b, and around the one A of this model they would leave most instances infeasible.  Instance b gets the model's own bounds
# widened by the half widths of its own draw: feasible where instance 0 is, different for every instance, the generator's widths --
# not the generator's distribution of bounds.
lo0, hi0 = probs[0]["lbA"], probs[0]["ubA"]
half = [0.5 * (p["ubA"] - p["lbA"]) for p in probs]
vecs = {"g": torch.as_tensor(np.stack([p["g"] for p in probs]), device=dev),
        "lbA": torch.as_tensor(np.stack([lo0 - (h if b else 0.0) for b, h in enumerate(half)]), device=dev),
        "ubA": torch.as_tensor(np.stack([hi0 + (h if b else 0.0) for b, h in enumerate(half)]), device=dev)}


def stats3(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


for leg in args.legs:
    bt = la.BatchLCQP(B, n, nC, nComp, opt=opt, **({"shared_matrices": True} if leg == "b" else {}))
    rc = bt.load_device(0, B, mats["Q"], vecs["g"], mats["L"], mats["R"], A=mats["A"], lbA=vecs["lbA"], ubA=vecs["ubA"])
    assert rc == 0, (rc, bt._last_error())
    setup, solve, rate = [], [], []
    for k in range(args.warmup + args.runs):
        bt.synchronize()
        t0 = time.perf_counter()
        bt.run()
        bt.synchronize()
        t1 = time.perf_counter()
        if k >= args.warmup:
            s, h = bt.last_timing()
            setup.append(s); solve.append(h); rate.append(B / (t1 - t0))
    _, _, st = bt.solution()
    print(json.dumps(dict(leg=leg, shared=leg == "b", batch=B, shape=[n, nC, nComp], runs=args.runs, setup_ms=stats3(setup), homotopy_ms=stats3(solve),
                          lcqps_per_s=stats3(rate), device_bytes=bt.device_bytes() if hasattr(bt, "device_bytes") else None, solved=sum(s["returnValue"] == 0 for s in st))), flush=True)
    bt.close()
