"""Re-solve measurements: the benchmark shape, B = 1024, generate_synthetic, the 2 % recipe applied on the host.
Per step, from HIP events (last_timing) and the wall clock around update / load + launch + collect:
  (a) load + run as today, (b) update + resolve(cold), (c) update + resolve(warm), with the mean and maximum iterate count of (c).
Warm-up steps are excluded.  Writes one JSON file.
    python tools/resolve_bench.py [--batch 1024] [--steps 5] [--warmup 2] [--out profiles/round7/resolve/resolve_bench.json]
--sparse: the sparse arm instead (lcqpow_amd/synth_sparse.py at --n, default 4096; --batch instances): on ONE handle, per step, run on the
data in place (the baseline: k_sparse_setup + homotopy), update + resolve(cold) and update + resolve(warm), with last_timing and the
iterate means of each.
    python tools/resolve_bench.py --sparse [--batch 4096] [--n 4096] [--steps 3] [--warmup 1] [--out ...]
--matrices: the matrices move too ("New matrices"): per step Q, A, L, R by the 2 % recipe of
tests/test_gpu_matrix_resolve.py and the vectors as above; on ONE handle, update_matrices + update + resolve(warm), then load + run of the
same data (what a caller had to do before update_matrices existed).  Setup + homotopy milliseconds from HIP events as min / median / max
over the steps, the wall clock, and the iterate counts of both.
    python tools/resolve_bench.py --matrices [--batch 1024] [--steps 10] [--warmup 1] [--out ...]
--sparse --matrices: the same on the sparse arm ("New matrices: the sparse arm"): per step the value arrays Qx, Ax by
the 2 % recipe of tests/test_gpu_sparse_value_resolve.py and the vectors as above; on ONE handle, update_values + update + resolve(warm),
then load + run of the same data.
    python tools/resolve_bench.py --sparse --matrices [--batch 1024] [--n 4096] [--steps 5] [--warmup 1] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402


def sparse_main(a):
    from lcqpow_amd import synth_sparse as S
    B, n = a.batch, a.n
    nC, nK = n // 2, n // 8
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    g = np.zeros((B, n)); lbA = np.zeros((B, nC)); ubA = np.zeros((B, nC))
    for c0 in range(0, B, 1024):                              # host staging: 1024 instances are 0.4 GB of values at n = 4096
        inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(c0, min(B, c0 + 1024))]
        c1 = c0 + len(inst)
        g[c0:c1] = [d["g"] for d in inst]; lbA[c0:c1] = [d["lbA"] for d in inst]; ubA[c0:c1] = [d["ubA"] for d in inst]
        assert sb.load(c0, len(inst), np.stack([d["Qx"] for d in inst]), g[c0:c1], np.stack([d["Ex"] for d in inst]), lbA=lbA[c0:c1], ubA=ubA[c0:c1]) == 0
    rng = np.random.default_rng(0)
    vec = dict(g=g, lbA=lbA, ubA=ubA)
    # per step: the warm re-solve first -- it starts from the solution of the data one 2 % move back --, then the two cold solves of the same data
    kinds = ("update_resolve_warm", "run", "update_resolve_cold")
    rows = {k: [] for k in kinds}
    sb.run(); sb.synchronize()
    for k in range(a.warmup + a.steps):
        shift = 0.02 * (vec["ubA"] - vec["lbA"]) * rng.standard_normal(vec["lbA"].shape)
        vec = dict(g=vec["g"] * (1.0 + 0.02 * rng.standard_normal(vec["g"].shape)), lbA=vec["lbA"] + shift, ubA=vec["ubA"] + shift)
        for kind in kinds:      # run: the same handle, the data the warm step has just put in place (a full setup + a cold homotopy)
            t0 = time.perf_counter()
            if kind == "run":
                sb.run()
            else:
                assert sb.update(0, B, vec["g"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
                sb.resolve(warm=(kind == "update_resolve_warm"))
            _, _, st = sb.solution()
            wall = (time.perf_counter() - t0) * 1e3
            setup_ms, solve_ms = sb.last_timing()
            it = [s["iterTotal"] for s in st]
            if k >= a.warmup:
                rows[kind].append(dict(wall_ms=wall, setup_ms=setup_ms, solve_ms=solve_ms, iter_mean=float(np.mean(it)), iter_max=int(max(it)),
                                       solved=int(sum(s["returnValue"] == 0 for s in st))))
    res = dict(arm="sparse", batch=B, shape=[n, nC, nK], lanes=sb.lanes(), steps=a.steps, warmup=a.warmup)
    for kind in ("run", "update_resolve_cold", "update_resolve_warm"):
        r = {key: float(np.mean([q[key] for q in rows[kind]])) for key in ("wall_ms", "setup_ms", "solve_ms", "iter_mean")}
        r.update(iter_max=max(q["iter_max"] for q in rows[kind]), solved_min=min(q["solved"] for q in rows[kind]), steps=rows[kind])
        res[kind] = r
        print(f"{kind:22s} wall {r['wall_ms']:8.1f} ms   setup/refresh {r['setup_ms']:7.3f} ms   homotopy {r['solve_ms']:8.2f} ms   "
              f"iterates mean {r['iter_mean']:.1f} max {r['iter_max']}   solved >= {r['solved_min']}/{B}")
    res["launch_counts"] = list(sb.launch_counts())
    sb.close()
    return res


def sparse_matrices_main(a):
    from lcqpow_amd import synth_sparse as S
    B, n = a.batch, a.n
    nC, nK = n // 2, n // 8
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
    val = dict(Qx=np.stack([d["Qx"] for d in inst]), Ax=np.stack([d["Ex"] for d in inst]))
    vec = {k: np.stack([d[k] for d in inst]) for k in ("g", "lbA", "ubA")}
    del inst
    assert sb.load(0, B, val["Qx"], vec["g"], val["Ax"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
    sb.run(); sb.synchronize()
    qrow, qcol = Qpat.indices, np.repeat(np.arange(n), np.diff(Qpat.indptr))      # CSC: row and column of every stored entry of Q
    rng = np.random.default_rng(0)
    eps = 0.02
    kinds = ("update_values_resolve_warm", "load_run")
    rows = {k: [] for k in kinds}
    for k in range(a.warmup + a.steps):
        s = 1.0 + eps * rng.standard_normal((B, n))
        val = dict(Qx=val["Qx"] * s[:, qrow] * s[:, qcol], Ax=val["Ax"] * (1.0 + eps * rng.standard_normal(val["Ax"].shape)))
        shift = eps * (vec["ubA"] - vec["lbA"]) * rng.standard_normal(vec["lbA"].shape)
        vec = dict(g=vec["g"] * (1.0 + eps * rng.standard_normal(vec["g"].shape)), lbA=vec["lbA"] + shift, ubA=vec["ubA"] + shift)
        for kind in kinds:      # the warm re-solve first: it starts from the solution of the data one 2 % move back
            t0 = time.perf_counter()
            if kind == "load_run":
                assert sb.load(0, B, val["Qx"], vec["g"], val["Ax"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
                sb.run()
            else:
                assert sb.update_values(0, B, **val) == 0
                assert sb.update(0, B, vec["g"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
                sb.resolve(warm=True)
            _, _, st = sb.solution()
            wall = (time.perf_counter() - t0) * 1e3
            setup_ms, solve_ms = sb.last_timing()
            it = [q["iterTotal"] for q in st]
            if k >= a.warmup:
                rows[kind].append(dict(wall_ms=wall, setup_ms=setup_ms, solve_ms=solve_ms, kernels_ms=setup_ms + solve_ms, iter_mean=float(np.mean(it)),
                                       iter_max=int(max(it)), solved=int(sum(q["returnValue"] == 0 for q in st))))
    res = dict(mode="sparse matrices", batch=B, shape=[n, nC, nK], lanes=sb.lanes(), steps=a.steps, warmup=a.warmup, eps=eps)
    summarise(res, rows, kinds, B)
    res["launch_counts"] = list(sb.launch_counts())
    sb.close()
    return res


def summarise(res, rows, kinds, B):
    """min / median / max of the HIP-event milliseconds and the iterate counts of every kind into res, and one printed line each"""
    for kind in kinds:
        r = {}
        for key in ("kernels_ms", "setup_ms", "solve_ms", "wall_ms"):
            v = [q[key] for q in rows[kind]]
            r[key] = dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)))
        r.update(iter_mean=float(np.mean([q["iter_mean"] for q in rows[kind]])), iter_max=max(q["iter_max"] for q in rows[kind]),
                 solved_min=min(q["solved"] for q in rows[kind]), steps=rows[kind])
        res[kind] = r
        km, sm, hm = r["kernels_ms"], r["setup_ms"], r["solve_ms"]
        print(f"{kind:30s} setup + homotopy {km['min']:7.2f} / {km['median']:7.2f} / {km['max']:7.2f} ms (min / median / max; setup {sm['median']:.2f}, "
              f"homotopy {hm['median']:.2f})   wall {r['wall_ms']['median']:8.1f} ms   iterates mean {r['iter_mean']:.1f} max {r['iter_max']}   "
              f"solved >= {r['solved_min']}/{B}")


def matrices_main(a):
    B, n, nC, nComp = a.batch, 256, 512, 64
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options(printLevel=0))
    bt.generate_synthetic(0)
    bt.run()
    bt.synchronize()
    probs = [bt.read_problem(b) for b in range(B)]
    mats = {k: np.stack([p[k] for p in probs]) for k in ("Q", "L", "R", "A")}
    vec = {k: np.stack([p[k] for p in probs]) for k in ("g", "lbA", "ubA")}
    rng = np.random.default_rng(0)
    eps = 0.02
    kinds = ("update_matrices_resolve_warm", "load_run")
    rows = {k: [] for k in kinds}
    for k in range(a.warmup + a.steps):
        s = 1.0 + eps * rng.standard_normal((B, n))
        mats = dict(Q=mats["Q"] * s[:, :, None] * s[:, None, :], A=mats["A"] * (1.0 + eps * rng.standard_normal((B, nC, n), dtype=np.float32)),
                    L=mats["L"] * (1.0 + eps * rng.standard_normal((B, nComp, 1))), R=mats["R"] * (1.0 + eps * rng.standard_normal((B, nComp, 1))))
        shift = eps * (vec["ubA"] - vec["lbA"]) * rng.standard_normal(vec["lbA"].shape)
        vec = dict(g=vec["g"] * (1.0 + eps * rng.standard_normal(vec["g"].shape)), lbA=vec["lbA"] + shift, ubA=vec["ubA"] + shift)
        for kind in kinds:      # the warm re-solve first: it starts from the solution of the data one 2 % move back
            t0 = time.perf_counter()
            if kind == "load_run":
                assert bt.load(0, B, mats["Q"], vec["g"], mats["L"], mats["R"], A=mats["A"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
                bt.run()
            else:
                assert bt.update_matrices(0, B, **mats) == 0
                assert bt.update(0, B, vec["g"], lbA=vec["lbA"], ubA=vec["ubA"]) == 0
                bt.resolve(warm=True)
            _, _, st = bt.solution()
            wall = (time.perf_counter() - t0) * 1e3
            setup_ms, solve_ms = bt.last_timing()
            it = [q["iterTotal"] for q in st]
            if k >= a.warmup:
                rows[kind].append(dict(wall_ms=wall, setup_ms=setup_ms, solve_ms=solve_ms, kernels_ms=setup_ms + solve_ms, iter_mean=float(np.mean(it)),
                                       iter_max=int(max(it)), solved=int(sum(q["returnValue"] == 0 for q in st))))
    res = dict(mode="matrices", batch=B, shape=[n, nC, nComp], steps=a.steps, warmup=a.warmup, eps=eps)
    summarise(res, rows, kinds, B)
    res["launch_counts"] = list(bt.launch_counts())
    bt.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", action="store_true", help="new matrices per step: update_matrices (with --sparse: update_values) + resolve(warm) against load + run")
    ap.add_argument("--sparse", action="store_true", help="the sparse arm: run against resolve(cold) and resolve(warm) on one handle")
    ap.add_argument("--n", type=int, default=4096, help="--sparse: variables per instance (nC = n / 2, nComp = n / 8)")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "round7", "resolve", "resolve_bench.json"))
    a = ap.parse_args()
    if a.sparse or a.matrices:
        res = sparse_matrices_main(a) if (a.sparse and a.matrices) else (sparse_main(a) if a.sparse else matrices_main(a))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("written", a.out)
        return
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
