"""Plain numpy references for the KKT factorisations and solves of the sparse arm (tests/test_gpu_sparse_factor.py holds the device to them,
tests/test_sparse_kkt_ref.py holds them to their own bound on the CPU).  Nothing here restates the oracle's factorisations: a dense matrix
built from the scipy matrices of the problem, a right-looking LDL' without pivoting, and the block elimination of the bordered engine.

The bound (Higham's gamma form for LDL' without pivoting plus the two triangular solves, valid for any summation order; the constant doubled
for the stored reciprocals 1 / D; the count taken with N terms, safe for fronts as for bands):

    |b - K x| <= (6 N + 8) eps (Wm |x| + |b|),      Wm = |L| |D| |L'|,  eps = 2^-52,  N the dimension of K

componentwise, the residual evaluated in long double, everything in the ordering the factorisation ran in."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
GROWTH_CAP = 1e6      # max(Wm |x|) / max(|K| |x|): beyond it the bound would hide a failure


def ref_dtype(N):
    """long double up to N = 1024, float64 beyond (as tests/test_gpu_setup.py)"""
    return LD if N <= 1024 else np.float64


def kkt_dense(d, dprim, ddual, use):
    """[Q + dprim I, E_use'; E_use, -diag(ddual)] in node order (variables, then the rows of E = [A; L; R]) as a dense float64 matrix, from the
    scipy matrices d["Q"], d["E"].  A row outside `use` has the diagonal -1 and no entries.  ddual: a scalar or one value per row."""
    Q = np.asarray(d["Q"].todense(), dtype=np.float64); E = np.asarray(d["E"].todense(), dtype=np.float64)
    n, m = Q.shape[0], E.shape[0]
    use = np.asarray(use).astype(bool)
    dd = np.broadcast_to(np.asarray(ddual, dtype=np.float64), (m,))
    K = np.zeros((n + m, n + m))
    K[:n, :n] = Q + float(dprim) * np.eye(n)
    Eu = np.where(use[:, None], E, 0.0)
    K[n:, :n] = Eu; K[:n, n:] = Eu.T
    K[n + np.arange(m), n + np.arange(m)] = np.where(use, -dd, -1.0)
    return K


def ldl_nopivot(Kperm, dt):
    """Right-looking LDL' without pivoting of the symmetric matrix Kperm (already in the ordering to factorise in), in dtype dt.
    Returns (L unit lower, D, Wm = |L| |D| |L'| in float64).  A step updates only the rows its column reaches: the arithmetic of the dense
    loop, without the products with exact zeros."""
    A = np.array(Kperm, dtype=dt); N = A.shape[0]
    L = np.eye(N, dtype=dt); D = np.zeros(N, dtype=dt)
    for j in range(N):
        D[j] = A[j, j]
        idx = j + 1 + np.flatnonzero(A[j + 1:, j])
        if idx.size:
            l = A[idx, j] / D[j]
            L[idx, j] = l
            A[np.ix_(idx, idx)] -= np.outer(l, A[idx, j])
    aL = np.abs(L).astype(np.float64)
    Wm = (aL * np.abs(D).astype(np.float64)[None, :]) @ aL.T
    return L, D, Wm


def ldl_solve(L, D, B):
    """x with L D L' x = B (columns of B), forward and backward by columns, in the dtype of L"""
    X = np.array(B, dtype=L.dtype); N = L.shape[0]
    if X.ndim == 1:
        return ldl_solve(L, D, X[:, None])[:, 0]
    for j in range(N):
        idx = j + 1 + np.flatnonzero(L[j + 1:, j])
        if idx.size:
            X[idx] -= np.outer(L[idx, j], X[j])
    X /= D[:, None]
    for j in range(N - 1, -1, -1):
        idx = j + 1 + np.flatnonzero(L[j + 1:, j])
        if idx.size:
            X[j] -= L[idx, j] @ X[idx]
    return X


def bordered_ref(Kperm, kb, B):
    """The block elimination of the bordered engine in float64, written plainly: K = [Bd U'; U C] with the last kb positions the border;
    LDL' of Bd, W = U inv(Bd), S = C - W U', LDL' of S; then per right-hand side (columns of B) the band solve, the border unknowns from S,
    the band part corrected by W.  Returns the solutions."""
    K = np.asarray(Kperm, dtype=np.float64); N = K.shape[0]; Nb = N - kb
    Bd, U, Cc = K[:Nb, :Nb], K[Nb:, :Nb], K[Nb:, Nb:]
    L, D, _ = ldl_nopivot(Bd, np.float64)
    W = ldl_solve(L, D, U.T).T
    Ls, Ds, _ = ldl_nopivot(Cc - W @ U.T, np.float64)
    X = np.array(B, dtype=np.float64)
    X[:Nb] = ldl_solve(L, D, X[:Nb])
    X[Nb:] = ldl_solve(Ls, Ds, X[Nb:] - U @ X[:Nb])
    X[:Nb] -= W.T @ X[Nb:]
    return X


def residual_and_bound(Kperm, Wm, X, B):
    """(|B - K X|, (6 N + 8) eps (Wm |X| + |B|)), both in long double, for solutions X of right-hand sides B (columns), all in the ordering of Kperm"""
    N = Kperm.shape[0]
    X = np.asarray(X, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    res = np.abs(B.astype(LD) - Kperm.astype(LD) @ X.astype(LD))
    # (both sides stay in long double: solutions of unit vectors decay to 1e-300 along a band, where a float64 bound underflows to zero)
    return res, LD((6 * N + 8) * EPS) * (Wm.astype(LD) @ np.abs(X).astype(LD) + np.abs(B).astype(LD))


def growth(Kperm, Wm, X):
    """max(Wm |x|) / max(|K| |x|) per right-hand side"""
    aX = np.abs(np.asarray(X, dtype=np.float64))
    return (Wm @ aX).max(axis=0) / (np.abs(Kperm) @ aX).max(axis=0)


# ---- right-hand sides and working sets -------------------------------------------------------------------------------------------------
def rhs_set(N, seed, unit=True):
    """columns: 8 seeded random vectors, one whose entries span 12 decades, and for N <= 320 the N unit vectors"""
    rng = np.random.default_rng(seed)
    cols = [rng.standard_normal((N, 8)), (rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-6, 6, N))[:, None]]
    if unit and N <= 320:
        cols.append(np.eye(N))
    return np.hstack(cols)


def working_sets(m, seed, coupling=()):
    """name -> 0/1 flags [m]: empty, all rows, every third row, a seeded random half; with coupling rows, each of them out (of all rows) and
    alone in (with the random half)"""
    rng = np.random.default_rng(seed)
    half = (rng.random(m) < 0.5).astype(np.int32)
    sets = {"empty": np.zeros(m, dtype=np.int32), "all": np.ones(m, dtype=np.int32), "third": (np.arange(m) % 3 == 0).astype(np.int32), "half": half}
    for r in coupling:
        out = np.ones(m, dtype=np.int32); out[r] = 0
        inn = half.copy(); inn[list(coupling)] = 0; inn[r] = 1
        sets["row %d out" % r] = out; sets["row %d in" % r] = inn
    return sets


def regularisations(opt, scale, m, classes=None):
    """name -> (dprim, ddual [m]): the product's three pairs from its options and the instance's scale = max |Q_ii|.  admm: sigma scale with
    1 / (rho scale) on the rows of `classes` == 0 and 1 / (rho scale rhoEqMult) on the others (every second row without classes), as inequality
    and equality rows get"""
    eq = (np.arange(m) % 2 == 1) if classes is None else np.asarray(classes).astype(bool)
    rho = opt.admmRho * scale
    return {"safe": (opt.proxBig * scale, np.full(m, 1e-9 / scale)),
            "light": (opt.proxSmall * scale, np.full(m, 1e-14 / scale)),
            "admm": (opt.admmSigma * scale, np.where(eq, 1.0 / (rho * opt.rhoEqMult), 1.0 / rho))}


# ---- the input families -----------------------------------------------------------------------------------------------------------------
def synthetic(shape, B, span=6):
    import problems as P
    n, nC, nK = shape
    return [P.sparse_instance(b, n, nC, nK, span=span) for b in range(B)]


def coupled(shape, B, extra):
    """the banded synthetic pattern plus `extra` coupling rows over every variable, as test_sparse_banded_pattern_with_coupling_rows builds it;
    the coupling rows are rows nC .. nC + extra - 1 of E"""
    import scipy.sparse as sp
    import problems as P
    n, nC, nK = shape
    rng = np.random.default_rng(5)
    out = []
    for b in range(B):
        d = P.sparse_instance(b, n, nC, nK)
        E = d["E"].tocsr()
        rows = rng.uniform(0.5, 1.5, (extra, n)) / n
        A2 = sp.vstack([E[:nC], sp.csr_matrix(rows), E[nC:]], format="csc")
        A2.sort_indices()
        xs = np.linalg.lstsq(E[:nC].toarray(), 0.5 * (d["lbA"] + d["ubA"]), rcond=None)[0]
        mid = rows @ xs
        out.append(dict(Q=d["Q"], E=A2, g=d["g"], lbA=np.concatenate([d["lbA"], mid - 5.0]), ubA=np.concatenate([d["ubA"], mid + 0.05 * (b + 1)]),
                        nV=n, nC=nC + extra, nComp=nK))
    return out


def circle(N, B):
    """examples/OptimizeOnCircle.cpp with N segments: two variables and a row in the border.  Instances differ in the values of the rows."""
    import scipy.sparse as sp
    import problems as P
    d = P.circle(N)
    rng = np.random.default_rng(9)
    out = []
    for b in range(B):
        Q = sp.csc_matrix(d["Q"]); E = sp.csc_matrix(np.vstack([d["A"], d["L"], d["R"]]))
        Q.sort_indices(); E.sort_indices()
        if b > 0:
            E.data = E.data * rng.uniform(0.8, 1.25, E.data.size)
        out.append(dict(Q=Q, E=E, g=np.asarray(d["g"], dtype=float), lbA=np.asarray(d["lbA"], dtype=float), ubA=np.asarray(d["ubA"], dtype=float),
                        x0=np.asarray(d["x0"], dtype=float), nV=d["nV"], nC=d["nC"], nComp=d["nComp"]))
    return out


def dense_rows(B, n=200, nC=40, nK=8):
    """forty dense rows over two hundred variables (test_sparse_pattern_with_dense_rows_runs_on_the_general_ldl): one front of more than 64 rows"""
    import scipy.sparse as sp
    out = []
    for b in range(B):
        rng = np.random.default_rng(b)
        A = rng.standard_normal((nC, n)) / np.sqrt(n)
        L = np.zeros((nK, n)); R = np.zeros((nK, n))
        L[np.arange(nK), np.arange(nK)] = 1; R[np.arange(nK), nK + np.arange(nK)] = 1
        xs = rng.uniform(0.2, 1.0, n); xs[nK:2 * nK] = 0.0
        Q = sp.csc_matrix(np.diag(rng.uniform(1, 2, n))); E = sp.csc_matrix(np.vstack([A, L, R]))
        Q.sort_indices(); E.sort_indices()
        out.append(dict(nV=n, nC=nC, nComp=nK, Q=Q, E=E, g=rng.uniform(-1, 1, n), lbA=A @ xs - rng.uniform(0.1, 1, nC), ubA=A @ xs + rng.uniform(0.1, 1, nC)))
    return out


def grid(g, nK, nC, B):
    """problems.grid_lcqp: one pattern (seed 0), the values of Q and E scaled per instance"""
    import problems as P
    d0 = P.grid_lcqp(g, nK, nC)
    out = []
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        Q = d0["Q"].copy(); E = d0["E"].copy()
        Q.sort_indices(); E.sort_indices()
        if b > 0:
            s = rng.uniform(0.9, 1.1, Q.shape[0])
            Q = (Q.multiply(s[:, None]).multiply(s[None, :])).tocsc(); Q.sort_indices()      # a congruence: still symmetric positive definite
            E.data = E.data * rng.uniform(0.8, 1.25, E.data.size)
        out.append(dict(nV=d0["nV"], nC=d0["nC"], nComp=d0["nComp"], Q=Q, E=E, g=d0["g"], lbA=d0["lbA"], ubA=d0["ubA"]))
    return out


def scale_of(d):
    return float(np.abs(d["Q"].diagonal()).max())


def row_classes(d):
    """1 for the rows the ADMM weights treat as equalities (lbA == ubA), 0 elsewhere (rows of L and R: inequalities)"""
    m = d["E"].shape[0]
    c = np.zeros(m, dtype=np.int32)
    c[:d["nC"]] = (d["lbA"] == d["ubA"])
    return c


# name -> the inputs of one family: make(B) -> instances; B: instances of the GPU batch; general: the general LDL' takes it; coupling: the rows
# of E that are coupling rows; polish: the working sets used with the two polish pairs; span / env: how the GPU test creates the batch.
# The ADMM-like pair goes with every working set.  The polish pairs (1e-9 and 1e-14 relative on the rows) go only with the sets for which
# tests/test_sparse_kkt_ref.py shows the growth cap to hold: with every row, or a random half of them, in the set these patterns have
# leading blocks with more rows than variables (a complementarity row pins the first variable of two constraint rows), a row pivot of the
# size of its regularisation follows, and max(Wm |x|) / max(|K| |x|) reaches 1e7 .. 1e13 -- a bound that loose would hide a failure.
_THIN = ("empty", "third")
_ANY = ("empty", "all", "third", "half")
FAMILIES = {
    "small": dict(make=lambda B: synthetic((64, 32, 8), B), B=11, general=False, coupling=(), polish=_THIN),
    "mid": dict(make=lambda B: synthetic((512, 256, 64), B), B=5, general=False, coupling=(), polish=_THIN),
    "small span 10": dict(make=lambda B: synthetic((64, 32, 8), B, span=10), B=11, general=False, coupling=(), polish=_THIN),
    "mid span 10": dict(make=lambda B: synthetic((512, 256, 64), B, span=10), B=5, general=False, coupling=(), polish=_THIN),
    "small span 18": dict(make=lambda B: synthetic((64, 32, 8), B, span=18), B=11, general=False, coupling=(), polish=_THIN),
    "mid span 18": dict(make=lambda B: synthetic((512, 256, 64), B, span=18), B=5, general=False, coupling=(), polish=_THIN),
    "coupled 1": dict(make=lambda B: coupled((128, 64, 16), B, 1), B=6, general=False, coupling=(64,), polish=_THIN),
    "coupled 3": dict(make=lambda B: coupled((128, 64, 16), B, 3), B=10, general=False, coupling=(64, 65, 66), polish=_THIN),
    "circle 20": dict(make=lambda B: circle(20, B), B=6, general=False, coupling=(20,), polish=_ANY + ("row 20 out", "row 20 in")),
    "circle 100": dict(make=lambda B: circle(100, B), B=6, general=False, coupling=(100,), polish=("empty",)),
    "dense rows": dict(make=lambda B: dense_rows(B), B=4, general=True, coupling=(), polish=_ANY),
    "grid 12": dict(make=lambda B: grid(12, 40, 30, B), B=4, general=True, coupling=(), polish=("empty", "all")),
    "grid 30": dict(make=lambda B: grid(30, 150, 100, B), B=4, general=True, coupling=(), polish=("empty", "all")),
    "small general": dict(make=lambda B: synthetic((64, 32, 8), B), B=11, general=True, coupling=(), polish=_THIN),
}


def plan(name, inst):
    """The FACTOR calls of a family: [(regularisation name, [(set name, use [m]) per instance])].  Instance b takes set number b of the sets
    its regularisation goes with (cyclically; the seeded half differs between instances), so that the lane groups of a wavefront part."""
    fam = FAMILIES[name]
    out = []
    for rname in ("safe", "light", "admm"):
        if rname == "light" and fam["general"]:
            continue      # the general LDL' never runs at the light level (no ordering of it puts the rows behind their variables: lightOK = 0)
        per = []
        for b, d in enumerate(inst):
            sets = working_sets(d["E"].shape[0], 11 + b, coupling=fam["coupling"])
            names = [s for s in sets if rname == "admm" or s in fam["polish"]]
            sn = names[b % len(names)]
            per.append((sn, sets[sn]))
        out.append((rname, per))
    return out
