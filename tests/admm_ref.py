"""Plain numpy reference of the ADMM fallback of the dense subsolver (qp_build_K, qp_admm, qp_adapt_rho, qp_certificate in
lcqpow_amd/csrc/lcqp_dev.hpp), written from the formulas: OSQP's iteration (Stellato et al., Math. Prog. Comp. 12, 2020, algorithm 1 with
the linear system reduced to K = Q + sigma I + E' diag(rho) E), its rho update (section 5.2) and its certificates (section 3.4).  Nothing
here comes from oracle/, which restates the device's code line by line.

Every function takes the dtype of its arithmetic: np.longdouble (80-bit) is the reference the device is held to, np.float64 the run that
shows how far a correct double-precision implementation may lie from it (tests/test_admm_ref.py).  The one exception is rho_vector: the
device's rho vector is compared bit for bit, so it is formed with the same two float64 products.
"""
import numpy as np

from test_gpu_setup import chol_ref, tri_inv      # long-double Cholesky factor and triangular inverse, plain loops

LD = np.longdouble


def rho_vector(opt, scale, l, u):
    """rho of every stacked row: admmRho scale; 0 for a free row; times rhoEqMult where l == u.  float64, the device's two products."""
    rho = opt.admmRho * scale
    rv = np.full(len(l), rho)
    rv[l == u] = rho * opt.rhoEqMult
    rv[np.isinf(l) & np.isinf(u)] = 0.0
    return rv


def K(Q, E, sigma, rhov, dt=LD):
    """Q + sigma I + E' diag(rhov) E"""
    Q = Q.astype(dt); E = E.astype(dt)
    return Q + dt(sigma) * np.eye(Q.shape[0], dtype=dt) + E.T @ (rhov.astype(dt)[:, None] * E)


def K_magnitude(Q, E, sigma, rhov, dt=LD):
    """|Q| + sigma I + |E|' diag(rhov) |E|: the sum of the magnitudes of the terms of every entry of K"""
    return K(np.abs(Q), np.abs(E), sigma, rhov, dt)


def chol_solve(L, b):
    """K^-1 b from the lower factor L of K, by forward and backward substitution in the dtype of L"""
    n = L.shape[0]
    y = np.zeros(n, dtype=L.dtype)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    U = np.ascontiguousarray(L.T)
    x = np.zeros(n, dtype=L.dtype)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


def admm(Q, E, g, l, u, rhov, sigma, alpha, x0, y0, k, dt=LD, keep=(), z0=None):
    """k iterations of
        xt = K^-1 (sigma x - g + E'(rho z - y))
        zr = alpha E xt + (1 - alpha) z
        rho_r > 0: z+ = clip(zr + y / rho, l, u), y+ = y + rho (zr - z+);   rho_r = 0 (a free row): z+ = zr, y+ = 0
        x+ = alpha xt + (1 - alpha) x
    from x = x0, y = y0 (0 on the free rows), z = clip(E x0, l, u) (z0: continue from that z instead).  Returns x, y, z and the change dx, dy of the last iteration; with keep,
    a dict of these five after each iteration count listed in keep (all <= k)."""
    Q = Q.astype(dt); E = E.astype(dt); g = g.astype(dt); rho = rhov.astype(dt)
    lo = l.astype(dt); hi = u.astype(dt)
    sigma = dt(sigma); alpha = dt(alpha)
    L = chol_ref(K(Q, E, sigma, rhov, dt), dt)
    pos = rhov > 0
    rs = np.where(pos, rho, dt(1))
    x = x0.astype(dt).copy()
    y = np.where(pos, y0.astype(dt), dt(0))
    z = np.clip(E @ x, lo, hi) if z0 is None else z0.astype(dt)
    dx = np.zeros_like(x); dy = np.zeros_like(y)
    kept = {}
    for it in range(1, k + 1):
        xt = chol_solve(L, sigma * x - g + E.T @ (rho * z - y))
        zr = alpha * (E @ xt) + (1 - alpha) * z
        zn = np.where(pos, np.clip(zr + y / rs, lo, hi), zr)
        yn = np.where(pos, y + rho * (zr - zn), dt(0))
        xn = alpha * xt + (1 - alpha) * x
        dx, dy = xn - x, yn - y
        x, y, z = xn, yn, zn
        if it in keep:
            kept[it] = (x, y, z, dx, dy)
    return kept if keep else (x, y, z, dx, dy)


def adapt_factor(Q, E, g, x, y, z, dt=LD):
    """sqrt( (|E x - z| / max(|E x|, |z|)) / (|Q x + g + E'y| / max(|Q x|, |E'y|, |g|)) ) in infinity norms, clipped to [1e-3, 1e3], and
    whether the update is applied (the factor above 5 or below 1 / 5)"""
    Q = Q.astype(dt); E = E.astype(dt); g = g.astype(dt)
    x = x.astype(dt); y = y.astype(dt); z = z.astype(dt)
    nrm = lambda v: np.abs(v).max() if v.size else dt(0)
    tiny = dt(1e-30)
    ex, qx, ety = E @ x, Q @ x, E.T @ y
    num = nrm(ex - z) / max(nrm(ex), nrm(z), tiny)
    den = nrm(qx + g + ety) / max(nrm(qx), nrm(ety), nrm(g), tiny)
    fac = np.sqrt(num / max(den, tiny))
    fac = min(max(fac, dt(1e-3)), dt(1e3))
    return fac, bool(fac > 5 or fac < 0.2)


def certificate(Q, E, g, l, u, dy, dx, eps=1e-4, dt=LD):
    """OSQP's certificates from the change of the last iteration.  Primal infeasibility (4): no component of dy pushes against an infinite
    bound by more than eps |dy|, u'dy+ + l'dy- <= -eps |dy| and |E'dy| <= eps |dy|.  Unboundedness (5): g'dx <= -eps |dx|,
    |Q dx| <= eps |dx| and E dx within eps |dx| of the recession cone of [l, u].  Returns (flag, comparisons): every comparison that
    was evaluated as (name, value, threshold), so that a caller can see how far each lies from its threshold."""
    Q = Q.astype(dt); E = E.astype(dt); g = g.astype(dt); dy = dy.astype(dt); dx = dx.astype(dt)
    comps = []
    ny = np.abs(dy).max() if dy.size else dt(0)
    if ny > 1e-30:
        thr = dt(eps) * ny
        up, dn = dy > 0, dy < 0
        free = np.concatenate([dy[up & ~np.isfinite(u)], -dy[dn & ~np.isfinite(l)]])
        comps += [("dy against an infinite bound", v, thr) for v in free]
        bad = bool((free > thr).any())
        fu, fl = up & np.isfinite(u), dn & np.isfinite(l)
        sup = (u[fu].astype(dt) * dy[fu]).sum() + (l[fl].astype(dt) * dy[fl]).sum()
        if not bad:
            comps.append(("support function", -sup, thr))
            if sup <= -thr:
                v = np.abs(E.T @ dy).max()
                comps.append(("|E'dy|", v, thr))
                if v <= thr:
                    return 4, comps
    nx = np.abs(dx).max()
    if nx > 1e-30:
        thr = dt(eps) * nx
        gd = g @ dx
        comps.append(("-g'dx", -gd, thr))
        if gd <= -thr:
            v = np.abs(Q @ dx).max()
            comps.append(("|Q dx|", v, thr))
            if v <= thr:
                e = E @ dx
                rows = np.concatenate([e[np.isfinite(u)], -e[np.isfinite(l)]])
                comps += [("E dx against a finite bound", v, thr) for v in rows]
                if not (rows > thr).any():
                    return 5, comps
    return 0, comps


def fallback_rounds(Q, E, g, l, u, rhov, sigma, alpha, rounds, dt=LD):
    """the ADMM state along the fallback rounds of a solve from x = 0 whose polishes all fail (the polish writes none of it): 10, 20, 40 ...
    iterations (400 at the most), each followed by the rho update, and from the second of them on by the certificate, which ends the
    solve.  Returns (flag, comparisons of the last certificate, rounds run, rhov at the end)."""
    n = Q.shape[0]
    x = np.zeros(n, dtype=dt); y = np.zeros(len(l), dtype=dt); z = None
    rhov = rhov.copy(); k = 10
    for r in range(1, rounds + 1):
        x, y, z, dx, dy = admm(Q, E, g, l, u, rhov, sigma, alpha, x, y, k, dt, z0=z)
        fac, applied = adapt_factor(Q, E, g, x, y, z, dt)
        if applied:
            rhov = rhov * float(fac)
        if r >= 2:
            flag, comps = certificate(Q, E, g, l, u, dy, dx, dt=dt)
            if flag:
                return flag, comps, r, rhov
        k = min(2 * k, 400)
    return 0, [], rounds, rhov


def clearance(comps):
    """the smallest factor between a comparison's value and its threshold, in either direction (values <= 0 are infinitely far below)"""
    worst = np.inf
    for _, v, thr in comps:
        v = float(v); thr = float(thr)
        if v > 0:
            worst = min(worst, max(v / thr, thr / v))
    return worst


# ---- the cases of tests/test_gpu_admm.py (and of the float64 condition in tests/test_admm_ref.py) ------------------------------------------
def stacked_bounds(rng, ax):
    """bounds of the rows with values ax at a feasible point: one eighth equalities, one eighth one-sided (alternately lower and upper), one
    sixteenth (at least one) free, the rest two-sided at a distance 0.1 ... 1 -- so that ADMM clips on some rows and not on others"""
    m = len(ax)
    lo = ax - rng.uniform(0.1, 1.0, m); hi = ax + rng.uniform(0.1, 1.0, m)
    kind = rng.permutation(m)
    ne = m // 8; n1 = m // 8; nf = max(1, m // 16)
    eq, one, free = kind[:ne], kind[ne:ne + n1], kind[ne + n1:ne + n1 + nf]
    lo[eq] = hi[eq] = ax[eq]
    lo[one[0::2]] = -np.inf; hi[one[1::2]] = np.inf
    lo[free] = -np.inf; hi[free] = np.inf
    return lo, hi


def box_bounds(rng, xs):
    """a box on a quarter of the variables (an even number of them), lower, upper or both"""
    n = len(xs)
    lb = np.full(n, -np.inf); ub = np.full(n, np.inf)
    sel = rng.choice(n, 2 * (n // 8), replace=False)
    for j, i in enumerate(sel):
        if j % 3 != 1: lb[i] = xs[i] - rng.uniform(0.1, 1.0)
        if j % 3 != 0: ub[i] = xs[i] + rng.uniform(0.1, 1.0)
    return lb, ub


def qp_case(n, m, seed):
    """Q = M'M / n + I (cond about 5), A Gaussian / sqrt(n), bounds around the feasible point xs"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    d = dict(n=n, m=m, Q=M.T @ M / n + np.eye(n), A=rng.standard_normal((m, n)) / np.sqrt(n), g=rng.standard_normal(n))
    xs = rng.standard_normal(n)
    d["lbA"], d["ubA"] = stacked_bounds(rng, d["A"] @ xs)
    d["lb"], d["ub"] = box_bounds(rng, xs)
    d["x0"] = 0.5 * rng.standard_normal(n); d["y0"] = 0.5 * rng.standard_normal(n + m)
    return d


def lcqp_case(n, nC, nComp, seed):
    """the same family with complementarity rows: L, R rows of the identity on distinct variables, bounded below by 0"""
    rng = np.random.default_rng(seed)
    d = qp_case(n, nC, seed)
    p = rng.permutation(n)
    d["L"] = np.zeros((nComp, n)); d["R"] = np.zeros((nComp, n))
    for i in range(nComp):
        d["L"][i, p[(2 * i) % n]] = rng.uniform(0.5, 2.0); d["R"][i, p[(2 * i + 1) % n]] = rng.uniform(0.5, 2.0)
    d.update(nC=nC, nComp=nComp)
    return d


def batch_data(B, n, nC, nComp):
    """the distinct instances of a batch case: instance b holds data[b % len(data)] (three data sets at the most)"""
    return [lcqp_case(n, nC, nComp, 1000 * n + j) for j in range(min(B, 3))]


def stacked(d):
    """(E, l, u) of a case as the device stacks them: [A; L; R; rows of I for the variables with a finite box bound, ascending]"""
    n = d["n"]
    rows, lo, hi = [d["A"]], [d["lbA"]], [d["ubA"]]
    if "L" in d:
        k = d["nComp"]
        rows += [d["L"], d["R"]]; lo += [np.zeros(2 * k)]; hi += [np.full(2 * k, np.inf)]
    fin = np.flatnonzero(np.isfinite(d["lb"]) | np.isfinite(d["ub"]))
    rows.append(np.eye(n)[fin]); lo.append(d["lb"][fin]); hi.append(d["ub"][fin])
    return np.vstack(rows), np.concatenate(lo), np.concatenate(hi)


def start_duals(d, y0):
    """ya at the start of a solve that is given y0 in the layout of the solution (box duals first, then the rows): -y0 in stacked order"""
    n = d["n"]
    fin = np.flatnonzero(np.isfinite(d["lb"]) | np.isfinite(d["ub"]))
    return -np.concatenate([y0[n:], y0[fin]])


QP_CASES = [(40, 30, 1), (200, 333, 2), (300, 100, 3), (600, 90, 4)]                    # (n, m, seed)
BATCH_CASES = [(6, 64, 96, 16), (3, 200, 330, 37), (1040, 100, 60, 16), (2, 256, 700, 100)]   # (B, n, nC, nComp)
KS = (1, 5, 20)                 # iteration counts of check C
K_ADAPT = 15                    # check D: 5 + 10 iterations, then the rho update
# check D, chosen with this file on the CPU (tests/test_admm_ref.py asserts them): (case, admmRho, +1: factor > 5, -1: < 0.2, 0: not applied)
QP_RHO_CASES = [(QP_CASES[1], 0.1, +1), (QP_CASES[1], 1.0, 0), (QP_CASES[1], 30.0, -1), (QP_CASES[2], 10.0, -1)]
BATCH_RHO_CASES = [(BATCH_CASES[0], 0.01, +1), (BATCH_CASES[0], 3.0, 0), (BATCH_CASES[1], 0.03, +1)]
F_SEED, F_N, F_M = 16, 150, 180      # check F: problems.certificate_qps(F_SEED, F_N, F_M, box=True)


def direction(fac, applied):
    """+1, -1, 0 as above; the factor lies at least 10 % away from both thresholds, so that rounding cannot decide the branch"""
    f = float(fac)
    assert not (0.9 * 5 < f < 1.1 * 5) and not (0.9 * 0.2 < f < 1.1 * 0.2), f
    return 0 if not applied else (1 if f > 5 else -1)


# ---- the bounds of tests/test_gpu_admm.py, stated once (tests/test_admm_ref.py holds a float64 run of this file to 1e-2 of them) -----------
def cond2(Kmat):
    ev = np.linalg.eigvalsh(np.asarray(Kmat, dtype=np.float64))
    return float(ev[-1] / ev[0])


def factor_bound(L, Q, E, sigma, rhov):
    """check B, entry by entry: 1e-12 (n + mE) (|L||L'| + |Q| + sigma I + |E|' diag(rho) |E|); an entry of K is itself a sum over mE rows"""
    aL = np.abs(L)
    return 1e-12 * (Q.shape[0] + E.shape[0]) * (aL @ aL.T + K_magnitude(Q, E, sigma, rhov, L.dtype.type))


def iterate_bounds(n, condK, k, x, y, z, rhov):
    """check C: the solve bound 1e-12 n cond_2(K) times the iteration count and the size of the iterates (y measured in units of z: divided
    by the smallest positive rho).  Returns the bound of the x- and z-sized quantities and the one of the rows of y (times rho_r)."""
    pos = rhov[rhov > 0]
    size = max(1.0, float(np.abs(x).max()), float(np.abs(z).max()), float(np.abs(y).max()) / float(pos.min()))
    b = 1e-12 * n * condK * k * size
    return b, b * rhov


def iterate_errors(dev, ref, rhov, b, by):
    """(name, error, bound) of the five quantities of check C; dev and ref are (x, y, z, dx, dy)"""
    names = ("xa", "ya", "za", "dx", "dy")
    bounds = (b, by, b, b, by)
    return [(nm, np.abs(np.asarray(a, dtype=LD) - c.astype(LD)), bd) for nm, a, c, bd in zip(names, dev, ref, bounds)]
