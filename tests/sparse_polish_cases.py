"""The inputs of the sparse polish audit, shared by tests/test_sparse_polish_audit_ref.py (a float64 model climbs them) and
tests/test_gpu_sparse_polish_audit.py (the device does): instances with scipy matrices as tests/problems.py builds them, their stacked
bounds, their dense form, and the options of a rung."""
import numpy as np

import problems as PR


def stacked_bounds(d):
    """l, u over the rows of E = [A; L; R] as the device stores them"""
    nK = d["nComp"]
    lbL = d["lbL"] if d.get("lbL") is not None else np.zeros(nK)
    lbR = d["lbR"] if d.get("lbR") is not None else np.zeros(nK)
    return np.concatenate([d["lbA"], lbL, lbR]), np.concatenate([d["ubA"], np.full(2 * nK, np.inf)])


def dense_case(d):
    l, u = stacked_bounds(d)
    return dict(Q=d["Q"].toarray(), E=d["E"].toarray(), g=np.asarray(d["g"], dtype=float), l=l, u=u,
                x0=np.asarray(d["x0"], dtype=float) if d.get("x0") is not None else np.zeros(d["nV"]))


def band_instances(count=3, shape=(64, 32, 8)):
    """Instances of the sparse synthetic workload with the bounds of the rows of A edited so that every row class occurs -- r % 8: 0 an equality
    (lbA == ubA), 1 lower only, 2 upper only, 3 free, 4 a tight two-sided row, 5 .. 7 the workload's wide two-sided rows -- the rows of A scaled
    over three decades together with their bounds (the same feasible set; a rule that drops |E_r| is wrong by that factor), and shifted
    complementarity bounds lbL = 0.01, lbR = 0.02.  The one-sided rows are moved so that they are violated at the unconstrained minimiser:
    the ladder enters rows, drops rows and has unchanged trials."""
    import scipy.sparse as sp
    n, nC, nK = shape
    out = []
    for b in range(count):
        d = PR.sparse_instance(b, n, nC, nK)
        rng = np.random.default_rng(700 + b)
        lbA, ubA = d["lbA"].copy(), d["ubA"].copy()
        A = d["E"].tocsr()[:nC].toarray()
        xu = -np.linalg.solve(d["Q"].toarray(), d["g"])
        ax = A @ xu
        for r in range(nC):
            k = r % 8
            mid = 0.5 * (lbA[r] + ubA[r])
            if k == 0: lbA[r] = ubA[r] = mid
            elif k == 1: lbA[r], ubA[r] = max(lbA[r], ax[r] + 0.05 * (1 + r % 3)), np.inf
            elif k == 2: lbA[r], ubA[r] = -np.inf, min(ubA[r], ax[r] - 0.05 * (1 + r % 3))
            elif k == 3: lbA[r], ubA[r] = -np.inf, np.inf
            elif k == 4: lbA[r], ubA[r] = mid - 0.02, mid + 0.02
        f = np.concatenate([10.0 ** rng.uniform(-1.5, 1.5, nC), np.ones(2 * nK)])
        E = (sp.diags(f) @ d["E"]).tocsc()
        E.sort_indices()
        assert np.array_equal(E.indices, d["E"].indices) and np.array_equal(E.indptr, d["E"].indptr)
        out.append(dict(d, E=E, lbA=lbA * f[:nC], ubA=ubA * f[:nC], lbL=np.full(nK, 0.01), lbR=np.full(nK, 0.02)))
    return out


SEMI = (22, 23)      # no equality row of band_instances touches them (rows 10 .. 12 do: upper only, free, tight) and no complementarity row


def semidefinite_instances(count=3, shape=(64, 32, 8)):
    """band_instances with a Hessian that is only semidefinite INSIDE its pattern: variables 22 and 23 are cut from their neighbours (the
    entries stay in the pattern, with the value zero) and get the block [[2, 2], [2, 2]]; g is equal on the two, so the objective is flat,
    not unbounded, along e_22 - e_23.  The diagonal is healthy -- the host, which judges definiteness by the diagonal ratios, still offers
    the light regularisation -- but the second of the two pivots is 2 deltaS whatever the ordering (at trial 0 no row that touches them is
    active): the pivot test fails on a VARIABLE, which makes the safe pair permanent for the instance (bigReg)."""
    out = []
    i, j = SEMI
    for d in band_instances(count, shape):
        Q = d["Q"].tolil(copy=True)
        for a, b in ((i - 1, i), (j, j + 1)):
            Q[a, b] = 0.0; Q[b, a] = 0.0
        Q[i, i] = Q[j, j] = Q[i, j] = Q[j, i] = 2.0
        Qc = d["Q"].copy()
        Qc.data = _values_in_pattern(Q, d["Q"])      # the pattern is the batch's: the cut entries stay, as zeros
        g = d["g"].copy(); g[j] = g[i]
        out.append(dict(d, Q=Qc, g=g))
    return out


def _values_in_pattern(M, pat):
    """the values of M at the stored entries of the CSC matrix pat, in its order (explicit zeros kept)"""
    M = M.tocsr()
    cols = np.repeat(np.arange(pat.shape[1]), np.diff(pat.indptr))
    return np.asarray(M[pat.indices, cols]).ravel()


def circle_instances(count=3):
    return PR.circle_instances(count)


def ladder_options(make, k):
    """the options of rung k: exactly k trials of the first QP, no ADMM, the run ends behind that QP"""
    return make(maxTrials=k, maxRounds=1, admmFirst=0, admmHot=0, maxIterations=0, perturbStep=0, printLevel=0)
