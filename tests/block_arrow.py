"""The block-arrow LCQPs of the minimum-degree tests (tests/test_sparse_min_degree.py, tests/test_gpu_sparse_min_degree.py): K small blocks
coupled through s shared variables -- a two-stage problem.  The KKT graph has a small diameter: a breadth-first level holds a node of nearly
every block, so nested dissection finds separators hundreds of nodes wide, where an elimination by minimum degree needs fronts of a few
dozen rows.

  nV = K nb + s, nC = 2 K, nComp = K.  Block b holds the variables b nb .. b nb + nb - 1, the shared variables are K nb + j.
  Q: tridiagonal inside each block, diagonal on the shared variables, both triangles.
  Row 2 b + r of A (r = 0, 1): block variables (3 r) mod nb and (3 r + 1) mod nb, shared variables (4 b + 2 r) mod s and (4 b + 2 r + 1) mod s.
  L row b: block variable nb / 2.  R row b: block variable nb - 1 and shared variable (7 b) mod s.

Values as problems.grid_lcqp takes them: a diagonally dominant Hessian, bounds around a point that satisfies the complementarity so that
every row class occurs (equalities, rows active at a bound, rows with slack), the rows of A scaled over three decades."""
import numpy as np

SEED = 3      # with it the sparse oracle returns 0 on every instance the tests use (asserted in tests/test_sparse_min_degree.py)


def block_arrow(K, nb, s, inst=0, seed=SEED):
    """instance `inst` on the pattern (K, nb, s): dict(nV, nC, nComp, Q, E (scipy CSC, sorted), A, L, R, g, lbA, ubA)"""
    import scipy.sparse as sp
    rng = np.random.default_rng([seed, K, nb, s, inst])
    n, nC = K * nb + s, 2 * K
    var = lambda b, i: b * nb + i
    sh = lambda j: K * nb + (j % s)
    rows, cols, vals = [], [], []
    diag = np.zeros(n)
    for b in range(K):
        for i in range(nb - 1):
            v = -rng.uniform(0.5, 1.0)
            rows += [var(b, i), var(b, i + 1)]; cols += [var(b, i + 1), var(b, i)]; vals += [v, v]
            diag[var(b, i)] += -v; diag[var(b, i + 1)] += -v
    diag += rng.uniform(0.5, 1.5, n)      # strictly dominant
    rows += list(range(n)); cols += list(range(n)); vals += list(diag)
    Q = sp.csc_matrix((vals, (rows, cols)), shape=(n, n))
    # a point that satisfies the complementarity: L_b x = 0 or R_b x = 0, the other one positive
    xs = rng.uniform(-1, 1, n)
    xs[K * nb:] = rng.uniform(0.1, 1.0, s)
    Lr, Lc, Rr, Rc = [], [], [], []
    for b in range(K):
        Lr.append(b); Lc.append(var(b, nb // 2))
        Rr += [b, b]; Rc += [var(b, nb - 1), sh(7 * b)]
        if rng.random() < 0.5:
            xs[var(b, nb // 2)] = 0.0; xs[var(b, nb - 1)] = rng.uniform(0.1, 1.0)
        else:
            xs[var(b, nb // 2)] = rng.uniform(0.1, 1.0); xs[var(b, nb - 1)] = -xs[sh(7 * b)]
    Lm = sp.csc_matrix((np.ones(K), (Lr, Lc)), shape=(K, n)); Rm = sp.csc_matrix((np.ones(2 * K), (Rr, Rc)), shape=(K, n))
    ar, ac, av = [], [], []
    for b in range(K):
        for r in range(2):
            k = 2 * b + r
            scale = 10.0 ** rng.uniform(-1.5, 1.5)      # three decades
            cs = sorted({var(b, (3 * r) % nb), var(b, (3 * r + 1) % nb), sh(4 * b + 2 * r), sh(4 * b + 2 * r + 1)})
            for c in cs:
                ar.append(k); ac.append(c); av.append(scale * rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.5))
    A = sp.csc_matrix((av, (ar, ac)), shape=(nC, n))
    ax = A @ xs
    rs = np.asarray(abs(A).sum(axis=1)).ravel()
    lo = ax - rs * rng.uniform(0.1, 1, nC); hi = ax + rs * rng.uniform(0.1, 1, nC)
    cls = np.arange(nC) % 8      # 0: an equality, 1: the point on the lower bound, 2: on the upper bound, else slack on both sides
    lo = np.where((cls == 0) | (cls == 1), ax, lo); hi = np.where((cls == 0) | (cls == 2), ax, hi)
    E = sp.vstack([A, Lm, Rm]).tocsc()
    Q.sort_indices(); E.sort_indices()
    return dict(nV=n, nC=nC, nComp=K, Q=Q, A=A, L=Lm, R=Rm, E=E, g=rng.uniform(-2, 2, n), lbA=lo, ubA=hi)


def arrow_ordering(K, nb, s):
    """an elimination order of the KKT nodes for the oracle's general LDL' (w = -1), written from the definition of the pattern and independent
    of the product's analysis: block after block (its variables, then its two rows of A, its row of L, its row of R), the shared variables last"""
    n, nC = K * nb + s, 2 * K
    perm = []
    for b in range(K):
        perm += [b * nb + i for i in range(nb)] + [n + 2 * b, n + 2 * b + 1, n + nC + b, n + nC + K + b]
    perm += [K * nb + j for j in range(s)]
    assert sorted(perm) == list(range(n + nC + 2 * K))
    return np.array(perm, dtype=np.int32)


def write_case(path, d, general=0, lanes=0):
    """the pattern of d as whitespace-separated integers, as tests/cpp/sparse_pattern_test.cpp and min_degree_test.cpp read it:
    nV nC nComp general lanes, Qp, nnz(Q), Qi, Ap, nnz(A), Ai"""
    Q, E = d["Q"].tocsc(), d["E"].tocsc()
    Q.sort_indices(); E.sort_indices()
    parts = [np.array([d["nV"], d["nC"], d["nComp"], general, lanes]), Q.indptr, [Q.indptr[-1]], Q.indices, E.indptr, [E.indptr[-1]], E.indices]
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(int(v)) for v in p) for p in parts) + "\n")


def oracle_solve(oracle, d, perm, **opt):
    """the sparse oracle's general LDL' on d in the ordering perm"""
    Qr, Er = d["Q"].tocsr(), d["E"].tocsr()
    return oracle.sparse_lcqp_solve(d["nV"], d["nC"], d["nComp"], Qr, d["g"], Er, lbA=d["lbA"], ubA=d["ubA"], perm=perm, w=-1, kb=0,
                                    opt=oracle.default_options(perturbStep=0, **opt))
