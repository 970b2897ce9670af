"""Re-solve measurements: the benchmark shape, B = 1024, generate_synthetic, the 2 % recipe applied on the host.
Per step, from HIP events (last_timing) and the wall clock around update / load + launch + collect:
  (a) load + run as today, (b) update + resolve(cold), (c) update + resolve(warm), with the mean and maximum iterate count of (c).
Warm-up steps are excluded.  Writes one JSON file.
    python tools/resolve_bench.py [--batch 1024] [--steps 5] [--warmup 2] [--out profiles/round7/resolve/resolve_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "round7", "resolve", "resolve_bench.json"))
    a = ap.parse_args()
    B, n, nC, nComp = a.batch, 256, 512, 64
    opt = la.default_options(printLevel=0)
    bt = la.BatchLCQP(B, n, nC, nComp, opt=opt)
    bt.generate_synthetic(0)
    bt.run()
    bt.synchronize()
    probs = [bt.read_problem(b) for b in range(B)]
    mats = {k: np.stack([p[k] for p in probs]) for k in ("Q", "L", "R", "A")}
    vec = {k: np.stack([p[k] for p in probs]) for k in ("g", "lbA", "ubA")}
    rng = np.random.default_rng(0)

    def step_vectors(v):
        shift = 0.02 * (v["ubA"] - v["lbA"]) * rng.standard_normal(v["lbA"].shape)
        return dict(g=v["g"] * (1.0 + 0.02 * rng.standard_normal(v["g"].shape)), lbA=v["lbA"] + shift, ubA=v["ubA"] + shift)

    def measure(kind):
        nonlocal vec
        rows = []
        for k in range(a.warmup + a.steps):
            vec = step_vectors(vec)
            t0 = time.perf_counter()
            if kind == "load_run":
                assert bt.load(0, B, mats["Q"], vec["g"], mats["L"], mats["R"], A=mats["A"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
                bt.run()
            else:
                assert bt.update(0, B, vec["g"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
                bt.resolve(warm=(kind == "update_resolve_warm"))
            _, _, st = bt.solution()
            wall = (time.perf_counter() - t0) * 1e3
            setup_ms, solve_ms = bt.last_timing()
            it = [s["iterTotal"] for s in st]
            if k >= a.warmup:
                rows.append(dict(wall_ms=wall, setup_ms=setup_ms, solve_ms=solve_ms, iter_mean=float(np.mean(it)), iter_max=int(max(it)),
                                 solved=int(sum(s["returnValue"] == 0 for s in st))))
        out = {key: float(np.mean([r[key] for r in rows])) for key in ("wall_ms", "setup_ms", "solve_ms", "iter_mean")}
        out.update(iter_max=max(r["iter_max"] for r in rows), solved_min=min(r["solved"] for r in rows), steps=rows)
        return out

    res = dict(batch=B, shape=[n, nC, nComp], steps=a.steps, warmup=a.warmup)
    for kind in ("load_run", "update_resolve_cold", "update_resolve_warm"):
        res[kind] = measure(kind)
        r = res[kind]
        print(f"{kind:22s} wall {r['wall_ms']:8.1f} ms   setup/refresh {r['setup_ms']:7.3f} ms   homotopy {r['solve_ms']:7.2f} ms   "
              f"iterates mean {r['iter_mean']:.1f} max {r['iter_max']}   solved >= {r['solved_min']}/{B}")
    res["launch_counts"] = list(bt.launch_counts())
    bt.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
