"""Load once, then K steps of new vectors + warm re-solve: a batch of controllers that solve the same LCQP matrices
again and again with a new linear term and new bounds.
    python examples/resolve_sequence.py [B=256] [steps=5]
    python examples/resolve_sequence.py [B=256] [steps=5] sparse     the same on the sparse arm (lcqp_hip_sparse_update / _resolve): the banded
                                                                     synthetic workload at n = 512, iterate counts per step
    python examples/resolve_sequence.py [B=256] [steps=5] matrices   the matrices move too, 2 % per step (an outer loop that re-linearises):
                                                                     update_matrices + update, then the warm re-solve sets up again
                                                                     around the last solution and working set
    python examples/resolve_sequence.py [B=256] [steps=5] sparse matrices   the value arrays Qx, Ax of the sparse arm move too, 2 % per step:
                                                                     update_values + update, then the warm re-solve (k_sparse_setup_warm)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402


def sparse_leg(B, steps, matrices=False):
    from lcqpow_amd import synth_sparse as S
    n, nC, nK = 512, 256, 64
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Apat, opt=la.default_options(perturbStep=0, printLevel=0))
    g = np.stack([d["g"] for d in inst]); lbA = np.stack([d["lbA"] for d in inst]); ubA = np.stack([d["ubA"] for d in inst])
    Qx, Ax = np.stack([d["Qx"] for d in inst]), np.stack([d["Ex"] for d in inst])
    qrow, qcol = Qpat.indices, np.repeat(np.arange(n), np.diff(Qpat.indptr))      # CSC: row and column of every stored entry of Q
    rc = sb.load(0, B, Qx, g, Ax, lbA=lbA, ubA=ubA)     # the matrices go to the device once
    if rc != 0:
        raise RuntimeError(f"load failed with code {rc}")
    sb.run()
    _, _, st = sb.solution()
    setup_ms, solve_ms = sb.last_timing()
    print(f"sparse, first solve: {np.mean([s['iterTotal'] for s in st]):.1f} iterates per LCQP, setup {setup_ms:.2f} ms + homotopy {solve_ms:.2f} ms")
    rng = np.random.default_rng(0)
    for step in range(1, steps + 1):
        g = g * (1.0 + 0.02 * rng.standard_normal(g.shape))
        shift = 0.02 * (ubA - lbA) * rng.standard_normal(lbA.shape)
        lbA, ubA = lbA + shift, ubA + shift
        if matrices:      # Q o s s' keeps symmetry and definiteness; every stored entry of [A; L; R] moves on its own
            s = 1.0 + 0.02 * rng.standard_normal((B, n))
            Qx = Qx * s[:, qrow] * s[:, qcol]
            Ax = Ax * (1.0 + 0.02 * rng.standard_normal(Ax.shape))
            rc = sb.update_values(0, B, Qx=Qx, Ax=Ax)      # (an array that is left out stays as the batch holds it)
            if rc != 0:
                raise RuntimeError(f"update_values failed with code {rc}: {la.capi.last_error()}")
        rc = sb.update(0, B, g, lbA=lbA, ubA=ubA)
        if rc != 0:
            raise RuntimeError(f"update failed with code {rc}")
        sb.resolve(warm=True)
        _, _, st = sb.solution()
        refresh_ms, solve_ms = sb.last_timing()
        it = [s["iterTotal"] for s in st]
        ok = sum(s["returnValue"] == 0 for s in st)
        print(f"sparse, step {step}: {ok}/{B} solved, iterates mean {np.mean(it):.1f} max {max(it)}, refresh {refresh_ms:.3f} ms + homotopy {solve_ms:.2f} ms")
    print("sparse, launches (full setups, homotopy launches):", sb.launch_counts())
    sb.close()


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if len(sys.argv) > 3 and sys.argv[3] == "sparse":
        sparse_leg(B, steps, matrices=len(sys.argv) > 4 and sys.argv[4] == "matrices")
        return
    matrices = len(sys.argv) > 3 and sys.argv[3] == "matrices"
    n, nC, nComp = 256, 512, 64
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options(printLevel=0))
    bt.generate_synthetic(0)          # stands for load(): the matrices go to the device once
    bt.run()
    _, _, st = bt.solution()
    setup_ms, solve_ms = bt.last_timing()
    print(f"first solve: {np.mean([s['iterTotal'] for s in st]):.1f} iterates per LCQP, setup {setup_ms:.2f} ms + homotopy {solve_ms:.2f} ms")
    probs = [bt.read_problem(b) for b in range(B)]
    g = np.stack([p["g"] for p in probs]); lbA = np.stack([p["lbA"] for p in probs]); ubA = np.stack([p["ubA"] for p in probs])
    mats = {k: np.stack([p[k] for p in probs]) for k in ("Q", "L", "R", "A")} if matrices else None
    rng = np.random.default_rng(0)
    for step in range(1, steps + 1):
        g = g * (1.0 + 0.02 * rng.standard_normal(g.shape))
        shift = 0.02 * (ubA - lbA) * rng.standard_normal(lbA.shape)
        lbA, ubA = lbA + shift, ubA + shift
        if matrices:
            s = 1.0 + 0.02 * rng.standard_normal((B, n))
            mats = dict(Q=mats["Q"] * s[:, :, None] * s[:, None, :], A=mats["A"] * (1.0 + 0.02 * rng.standard_normal(mats["A"].shape)),
                        L=mats["L"] * (1.0 + 0.02 * rng.standard_normal((B, nComp, 1))), R=mats["R"] * (1.0 + 0.02 * rng.standard_normal((B, nComp, 1))))
        t0 = time.perf_counter()
        if matrices:
            rc = bt.update_matrices(0, B, **mats)      # (a matrix that is left out stays as the batch holds it)
            if rc != 0:
                raise RuntimeError(f"update_matrices failed with code {rc}: {la.capi.last_error()}")
        rc = bt.update(0, B, g, lbA=lbA, ubA=ubA)
        if rc != 0:
            raise RuntimeError(f"update failed with code {rc}: {la.capi.last_error()}")
        bt.resolve(warm=True)
        _, _, st = bt.solution()
        wall = (time.perf_counter() - t0) * 1e3
        refresh_ms, solve_ms = bt.last_timing()
        it = [s["iterTotal"] for s in st]
        ok = sum(s["returnValue"] == 0 for s in st)
        print(f"step {step}: {ok}/{B} solved, iterates mean {np.mean(it):.1f} max {max(it)}, {'setup' if matrices else 'refresh'} {refresh_ms:.3f} ms + homotopy {solve_ms:.2f} ms, "
              f"{wall:.1f} ms with update and read-back")
    print("launches (full setups, homotopy launches):", bt.launch_counts())
    bt.close()


if __name__ == "__main__":
    main()
