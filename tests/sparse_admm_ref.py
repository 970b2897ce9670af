"""Plain numpy reference of the ADMM rounds of the sparse arm (sp_prepare_vectors, sp_ph_round, sp_admm in
lcqpow_amd/csrc/lcqp_sparse_solver.hpp), a sibling of tests/admm_ref.py: OSQP's iteration (Stellato et al., Math. Prog. Comp. 12, 2020,
algorithm 1) in the REDUCED form K = Q + sigma I + E' diag(rho) E with a dense long-double Cholesky factor.  The device iterates in the KKT
form [Q + sigma I, E'; E, -diag(1 / rho)] [xt; nu] = [sigma x - g; z - y / rho] through a sparse LDL' in an ordering of its own; eliminating
nu = rho (E xt - z) + y gives K xt = sigma x - g + E'(rho z - y) and zt = z + (nu - y) / rho = E xt, so the two agree and the reference
shares neither the solve nor the ordering with the device (admm_kkt below is that KKT form, for the CPU checks of tests/test_admm_ref.py).
Nothing here comes from oracle/.

The conventions of the sparse arm differ from the dense ones in one place: a free row (both bounds infinite) has the weight 1e-6 admmRho
scale instead of 0 and is recognised by its bounds: z+ = zr, y+ = 0.  A round starts with z = clip(E x, l, u) and y = 0 on the free rows.
"""
import numpy as np

import admm_ref as A
from test_gpu_setup import chol_ref

LD = np.longdouble
KS = (1, 5, 20)


def rho_vector(opt, scale, l, u):
    """rho of every row: admmRho scale; 1e-6 of it for a free row; times rhoEqMult where l == u.  float64, the device's products."""
    rho = opt.admmRho * scale
    rv = np.full(len(l), rho)
    rv[l == u] = rho * opt.rhoEqMult
    rv[np.isinf(l) & np.isinf(u)] = 1e-6 * rho
    return rv


def free_rows(l, u):
    return np.isinf(l) & np.isinf(u)


def admm(Q, E, g, l, u, rhov, sigma, alpha, x0, y0, k, dt=LD, keep=()):
    """k iterations of
        xt = K^-1 (sigma x - g + E'(rho z - y))
        zr = alpha E xt + (1 - alpha) z
        a free row: z+ = zr, y+ = 0;   any other: z+ = clip(zr + y / rho, l, u), y+ = y + rho (zr - z+)
        x+ = alpha xt + (1 - alpha) x
    from x = x0, y = y0 (0 on the free rows), z = clip(E x0, l, u).  Returns (x, y, z), or with keep a dict of them by iteration count."""
    Q = Q.astype(dt); E = E.astype(dt); g = g.astype(dt); rho = rhov.astype(dt)
    lo = l.astype(dt); hi = u.astype(dt)
    sigma = dt(sigma); alpha = dt(alpha)
    L = chol_ref(A.K(Q, E, sigma, rhov, dt), dt)
    free = free_rows(l, u)
    x = x0.astype(dt).copy()
    y = np.where(free, dt(0), y0.astype(dt))
    z = np.clip(E @ x, lo, hi)
    kept = {}
    for it in range(1, k + 1):
        xt = A.chol_solve(L, sigma * x - g + E.T @ (rho * z - y))
        zr = alpha * (E @ xt) + (1 - alpha) * z
        zn = np.where(free, zr, np.clip(zr + y / rho, lo, hi))
        y = np.where(free, dt(0), y + rho * (zr - zn))
        x = alpha * xt + (1 - alpha) * x
        z = zn
        if it in keep:
            kept[it] = (x, y, z)
    return kept if keep else (x, y, z)


def admm_kkt(Q, E, g, l, u, rhov, sigma, alpha, x0, y0, k, dt, perm, keep=()):
    """the same iteration in the device's form: the KKT matrix factorised once by an LDL' without pivoting in the ordering perm
    (tests/sparse_kkt_ref.py), in dtype dt, one solve per iteration, no refinement"""
    import sparse_kkt_ref as S
    n, m = Q.shape[0], E.shape[0]
    Kk = np.zeros((n + m, n + m), dtype=dt)
    Kk[:n, :n] = Q.astype(dt) + dt(sigma) * np.eye(n, dtype=dt)
    Kk[n:, :n] = E.astype(dt); Kk[:n, n:] = E.T.astype(dt)
    rho = rhov.astype(dt)
    Kk[n + np.arange(m), n + np.arange(m)] = -(dt(1) / rho)
    perm = np.asarray(perm)
    Lf, Df, _ = S.ldl_nopivot(Kk[np.ix_(perm, perm)], dt)
    g = g.astype(dt); lo = l.astype(dt); hi = u.astype(dt); sigma = dt(sigma); alpha = dt(alpha)
    Ed = E.astype(dt)
    free = free_rows(l, u)
    x = x0.astype(dt).copy()
    y = np.where(free, dt(0), y0.astype(dt))
    z = np.clip(Ed @ x, lo, hi)
    kept = {}
    for it in range(1, k + 1):
        b = np.concatenate([sigma * x - g, z - y / rho])
        s = np.zeros(n + m, dtype=dt)
        s[perm] = S.ldl_solve(Lf, Df, b[perm])
        xt, nu = s[:n], s[n:]
        zt = z + (nu - y) / rho
        zr = alpha * zt + (1 - alpha) * z
        zn = np.where(free, zr, np.clip(zr + y / rho, lo, hi))
        y = np.where(free, dt(0), y + rho * (zr - zn))
        x = alpha * xt + (1 - alpha) * x
        z = zn
        if it in keep:
            kept[it] = (x, y, z)
    return kept if keep else (x, y, z)


def iterate_bounds(n, condK, k, x, y, z, rhov, l, u):
    """the form of check C of tests/test_gpu_admm.py: 1e-12 n cond_2(K) k max(1, |x|, |z|, |y| / min rho), the minimum over the rows that
    carry a multiplier (y is 0 on the free rows); returns the bound of x and z and the one of the rows of y (times rho_r)"""
    live = ~free_rows(l, u)
    size = max(1.0, float(np.abs(x).max()), float(np.abs(z).max()), float(np.abs(y).max()) / float(rhov[live].min()))
    b = 1e-12 * n * condK * k * size
    return b, b * rhov


def iterate_errors(dev, ref, b, by):
    """(name, error, bound) of xa, ya, za; dev and ref are (x, y, z)"""
    return [(nm, np.abs(np.asarray(a, dtype=LD) - c.astype(LD)), bd) for nm, a, c, bd in zip(("xa", "ya", "za"), dev, ref, (b, by, b))]


# ---- the cases of tests/test_gpu_sparse_admm.py (and of the float64 condition in tests/test_admm_ref.py) -----------------------------------
def dense(d):
    return np.asarray(d["Q"].todense(), dtype=np.float64), np.asarray(d["E"].todense(), dtype=np.float64)


def rebound(d, seed, shrink=1.0):
    """instance d with the bounds of its A rows rewritten as admm_ref.stacked_bounds does (equalities, one-sided, free and two-sided rows that
    clip) around A xs for a seeded point xs, and a seeded start (x0, y0); the rows of L and R keep [0, inf)"""
    rng = np.random.default_rng(seed)
    n, nC = d["nV"], d["nC"]
    _, E = dense(d)
    xs = 0.5 * rng.standard_normal(n)
    lo, hi = A.stacked_bounds(rng, E[:nC] @ xs)
    mid = E[:nC] @ xs
    lo = np.where(np.isfinite(lo), mid - shrink * (mid - lo), lo); hi = np.where(np.isfinite(hi), mid + shrink * (hi - mid), hi)
    out = dict(d, lbA=lo, ubA=hi, x0=0.5 * rng.standard_normal(n), y0=0.5 * rng.standard_normal(E.shape[0]))
    return out


def stacked(d, lbA=None, ubA=None):
    """(l, u) of the rows of [A; L; R]"""
    k2 = 2 * d["nComp"]
    return (np.concatenate([d["lbA"] if lbA is None else lbA, np.zeros(k2)]), np.concatenate([d["ubA"] if ubA is None else ubA, np.full(k2, np.inf)]))


def _synthetic(shape, B, span=6):
    import sparse_kkt_ref as S
    return [rebound(d, 4000 + 10 * b + span) for b, d in enumerate(S.synthetic(shape, B, span=span))]


def _circle(B):
    """the bordered circle (every row of A an equality at 1 in the example, a Hessian of 5e-12 on all but two variables): milder than the
    others, or no polish of the first QP settles -- most rows keep their equality, every tenth becomes two-sided around 1, a few one-sided,
    one free; the start is the example's own point, perturbed"""
    import sparse_kkt_ref as S
    out = []
    for b, d in enumerate(S.circle(100, B)):
        rng = np.random.default_rng(5000 + b)
        lo, hi = d["lbA"].copy(), d["ubA"].copy()
        two = np.arange(3, 100, 10)
        lo[two] -= rng.uniform(0.01, 0.05, len(two)); hi[two] += rng.uniform(0.01, 0.05, len(two))
        lo[15] = -np.inf; hi[45] = np.inf; lo[75] = -np.inf
        lo[7 + b] = -np.inf; hi[7 + b] = np.inf
        out.append(dict(d, lbA=lo, ubA=hi, x0=d["x0"] + 0.01 * rng.standard_normal(d["nV"]), y0=0.1 * rng.standard_normal(d["E"].shape[0])))
    return out


# name -> (make, env): the instances of the batch, the environment the handle is created under
CASES = {
    "small": (lambda: _synthetic((64, 32, 8), 6), {}),
    "small pool 4": (lambda: _synthetic((64, 32, 8), 6), {"LCQP_SPARSE_POOL": "4"}),
    "small span 10": (lambda: _synthetic((64, 32, 8), 6, span=10), {}),
    "small span 18": (lambda: _synthetic((64, 32, 8), 6, span=18), {}),
    "circle 100": (lambda: _circle(3), {}),
    "small general": (lambda: _synthetic((64, 32, 8), 6), {"LCQP_SPARSE_GENERAL": "1"}),
    "mid": (lambda: _synthetic((512, 256, 64), 2), {}),
}


def move_classes(d, seed):
    """new A bounds that move rows between the classes: some two-sided rows become equalities, some equalities two-sided, a two-sided row
    free and the free rows two-sided"""
    rng = np.random.default_rng(seed)
    lo, hi = d["lbA"].copy(), d["ubA"].copy()
    two = np.flatnonzero(np.isfinite(lo) & np.isfinite(hi) & (lo < hi))
    eq = np.flatnonzero(lo == hi)
    free = np.flatnonzero(np.isinf(lo) & np.isinf(hi))
    mid = 0.5 * (lo[two] + hi[two])
    lo[two[0::4]] = hi[two[0::4]] = mid[0::4]
    lo[two[1]] = -np.inf; hi[two[1]] = np.inf
    lo[eq[0::2]] -= rng.uniform(0.1, 0.5, len(eq[0::2])); hi[eq[0::2]] += rng.uniform(0.1, 0.5, len(eq[0::2]))
    lo[free] = -rng.uniform(0.5, 1.0, len(free)); hi[free] = rng.uniform(0.5, 1.0, len(free))
    return lo, hi


def same_classes(d, seed):
    """new A bounds with every row in its class: the finite bounds shifted a little"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-0.05, 0.05, len(d["lbA"]))
    return d["lbA"] + s, d["ubA"] + s
