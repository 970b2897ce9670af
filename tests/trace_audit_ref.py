"""Direct reference for the per-iterate scalars of the homotopy loop (the trace of storeSteps), in np.longdouble, with no solver in the loop.

Everything a trace row records -- (|stat|inf, phi, rho, alpha, objective, merit, |p|inf, QP iterations) and x_k -- can be recomputed from the
recorded x_k and the problem data alone.  audit() does that for one instance and holds every recorded value to the recomputed one.  It imports
neither the library nor the oracle: one reference serves the dense arm, the sparse arm (densify the problem first) and the CPU oracle.

Notation: x_k row k of the trace, x_{-1} = x_start, d_k = x_k - x_{k-1}, rho_k = scalars[k][2], alpha_k = scalars[k][3], p_k = d_k / alpha_k,
C = L'R + R'L and g_phi = -(L'lbR + R'lbL) formed here in long double, eps = 2^-53.

Quantities (the names used in records and failures):
  rho      rho_0 == rho_start and rho_{k+1} in {rho_k, rho_k f, (rho_k f) f} exactly (f = penaltyUpdateFactor; a Leyffer update and a
           stationarity update can fall in one pass).  The products are formed in float64 and one factor at a time, as updatePenalty forms
           them in every loop (rho *= f, twice for a double update).  A product formed in long double and compared unrounded, as this audit
           did at first, is the same number for f = 2 but not for f = 10 from rho = 0.01 (0.01 * 10 in long double is not the float64 0.1):
           it refused every update of a correct trace; and rho_k f^2 with f^2 formed first is one rounding where the loops make two.
  obj      g'x_k + x_k'Q x_k / 2
  phi      (L x_k - lbL)'(R x_k - lbR), the direct form (the loops use the expanded one: phi_const + g_phi'x + x'Cx / 2)
  merit    obj + rho_k (L x_k)'(R x_k)
  step     max|d_k| == alpha_k scalars[k][6]
  alpha    k >= 1: q = d_k'(Q + rho_k C) d_k, l = d_k'((Q + rho_k C) x_{k-1} + gtil_k); since d_k = alpha_k p_k, a recorded alpha_k < 1 is right
           exactly when q > 0, l < 0 and -l / q = 1, and alpha_k == 1 exactly when q <= 0 or l >= 0 or -l / q >= 1.  Decided by the intervals
           l +- dl, q +- dq; a row with dl / |l| + dq / |q| > 0.1 is undecidable (the end of an inner loop, |p| ~ 1e-8): counted, not asserted.
           gtil_k by gtil_rule: "after_first_update" is g until rho has changed within this run and g + rho_k g_phi afterwards (what
           initializeSolver / updatePenalty of the reference do), "always" is g + rho_k g_phi.
  stat     QP k was solved with the linear term g_k = rho_k C x_{k-1} + gtil_k, so the dual terms of the stationarity cancel exactly:
           |alpha_k rho_k C p_k - (1 - alpha_k) Q p_k|_inf; row 0 of a cold run with solveZeroPenaltyFirst (its QP had the linear term g):
           |rho_0 C x_0|_inf; row 0 otherwise: |rho_0 C d_0|_inf -- up to the residual the subsolver verified its QP to, res_tol (1 + |g_k|_inf).
  decisions  the Leyffer history, the penalty updates, iterOuter, iterTotal, the sum of the QP iterations, rhoOpt, the return value and the
           returned x, replayed from the RECORDED stat, phi and rho (which `phi` and `stat` have held to the reference).  A comparison whose
           two sides lie within their audit bound of each other may go either way.  A run that ended with MAX_ITERATIONS_REACHED or
           MAX_PENALTY_REACHED is replayed to its last row like any other: the row must not converge, its penalty updates (a stationarity
           update included: the limits are tested behind it) must be allowed by its stat and phi, the limit named by the return value must
           be exceeded, none may have been exceeded at an earlier row, and iterations go before the penalty when both are.
  counters (AuditResult; what a test asserts to know its option set reached its branch): leyffer_fired, rows whose replayed Leyffer outcome
           is {True}; window_shifts, rows that found the Leyffer window full (it is shifted by one and the new phi appended);
           updates and double_updates, penalty updates in all and rows followed by two; row0_penalty, whether row 0 was audited as the
           solution of a QP that carries the penalty (no zero-penalty QP: solveZeroPenaltyFirst = 0 or a warm run), and cx0 = |rho_0 C x_start|inf,
           the term that QP's linear part has beyond g~.

Bounds: no free constants.  Every sum of m products gets the standard a priori bound gamma_m sum|terms|, gamma_m = m eps / (1 - m eps), evaluated in
long double from the absolute values of the same operands; m is the length of the longest chain, n + the most non-zeros of a row of C or Q + 8.
Carried quantities (Q x_k everywhere, C x_k where carried_C says so) are sums of the previous and the new product: their sum|terms| takes the
maximum over rows k and k - 1.  MARGIN = 4 over the a priori bound: the a priori bound holds for ONE evaluation in ANY order, and a recorded value
is compared with a reference that has roundings of its own, was formed in the expanded rather than the direct form (twice the terms), and on the
carried path mixes two products -- a factor of 4 covers these by construction, whatever the order of evaluation.  Two more terms are not roundings
of the loop but what the audit itself cannot know: d_k is alpha_k p_k only up to the rounding of x_k = x_{k-1} + alpha_k p_k, eps |x_k| per
component, and with perturbStep each x_{k-1} moved by +-2.221e-16 per component before the step.  Both enter where d_k stands for alpha_k p_k.
"""
import numpy as np

LD = np.longdouble
EPS = LD(2) ** -53
MARGIN = LD(4)
PERTURB = LD(2.221e-16)      # perturbStep: x += {-1, 0, 1} * 2.221e-16 per component
QUANTITIES = ("rho", "obj", "phi", "merit", "step", "alpha", "stat", "decisions")
RULES = ("after_first_update", "always")


class AuditError(AssertionError):
    """raised by audit(check=True); .result holds the AuditResult with every failure"""

    def __init__(self, result):
        self.result = result
        head = "; ".join("%s row %s: %s" % f for f in result.failures[:6])
        AssertionError.__init__(self, "%d trace audit failure(s): %s" % (len(result.failures), head))


class AuditResult:
    def __init__(self):
        self.records = []        # per row: {quantity: (recorded, reference, bound)}; "alpha": (alpha, -l / q or nan, relative interval width, verdict)
        self.failures = []       # (quantity, row or None, text)
        self.undecidable = 0     # rows k >= 1 whose step length the intervals do not decide
        self.decided = 0
        self.leyffer_fired = 0   # the counters: see the module docstring
        self.window_shifts = 0
        self.updates = 0
        self.double_updates = 0
        self.row0_penalty = False
        self.cx0 = 0.0

    def failed(self):
        return sorted({f[0] for f in self.failures})

    def fail(self, quantity, row, text):
        self.failures.append((quantity, row, text))


def _o(opt, name):
    return opt[name] if isinstance(opt, dict) else getattr(opt, name)


def _steps(rho, f):
    """rho, rho f, (rho f) f in float64, one factor at a time (updatePenalty: rho *= f)"""
    rho, f = float(rho), float(f)
    return (rho, rho * f, (rho * f) * f)


def _gamma(m):
    m = LD(m)
    return m * EPS / (LD(1) - m * EPS)


def _vec(d, key, size, fill=0.0):
    v = d.get(key)
    return np.full(size, fill, dtype=LD) if v is None else np.asarray(v, dtype=np.float64).astype(LD)


def complementarity_matrix(L, R):
    """C = L'R + R'L in long double, row by row over the non-zeros of L and R (one-hot rows cost nothing)"""
    n = L.shape[1]
    C = np.zeros((n, n), dtype=LD)
    for i in range(L.shape[0]):
        a, b = np.nonzero(L[i])[0], np.nonzero(R[i])[0]
        if a.size and b.size:
            blk = np.outer(L[i, a], R[i, b])
            C[np.ix_(a, b)] += blk
            C[np.ix_(b, a)] += blk.T
    return C


def audit(d, opt, scalars, xs, x_start, rho_start, warm, gtil_rule, res_tol, stats=None, x_ret=None, carried_C=False, check=True):
    """Audit one instance's trace (see the module docstring).  d: a problem dict in the layout of tests/problems.py (dense Q, L, R, g and
    optionally lbL, lbR); opt: the options the run had (an object or a dict with the reference's option names); scalars [len][8] and
    xs [len][n]: the trace; x_start: x_{-1} (None: zeros); rho_start: the penalty the run started at; warm: a warm re-solve (no zero-penalty
    QP); gtil_rule: see `alpha`; res_tol: the subsolver's verification tolerance.  stats (dict with iterTotal, iterOuter, subproblemIter,
    rhoOpt, returnValue) and x_ret (the returned x) feed `decisions`; carried_C: C x_k follows the steps by linearity.
    Returns an AuditResult; with check, raises AuditError when any quantity failed."""
    assert gtil_rule in RULES
    res = AuditResult()
    n = int(d["nV"])
    Q = np.asarray(d["Q"], dtype=np.float64).astype(LD)
    L = np.asarray(d["L"], dtype=np.float64).astype(LD); R = np.asarray(d["R"], dtype=np.float64).astype(LD)
    nK = L.shape[0]
    g = _vec(d, "g", n)
    lbL, lbR = _vec(d, "lbL", nK), _vec(d, "lbR", nK)
    C = complementarity_matrix(L, R)
    gphi = -(L.T @ lbR + R.T @ lbL)
    aQ, aC, aL, aR = np.abs(Q), np.abs(C), np.abs(L), np.abs(R)
    m_chain = n + int(max((Q != 0).sum(axis=1).max(), (C != 0).sum(axis=1).max())) + 8
    G = MARGIN * _gamma(m_chain)
    f = LD(_o(opt, "penaltyUpdateFactor"))
    perturb = bool(_o(opt, "perturbStep"))
    zero_first = bool(_o(opt, "solveZeroPenaltyFirst")) and not warm
    sc = np.asarray(scalars, dtype=np.float64)
    X = np.asarray(xs, dtype=np.float64).astype(LD)
    K = len(sc)
    x_prev = np.zeros(n, dtype=LD) if x_start is None else np.asarray(x_start, dtype=np.float64).astype(LD)
    rho_start = LD(rho_start)
    res_tol = LD(res_tol)

    if K == 0:
        res.fail("decisions", None, "empty trace")
    T_prev = None      # sum|terms| of row k - 1 (the carried products)
    phi_bounds, stat_bounds = [], []
    for k in range(K):
        x = X[k]
        rho, alpha = LD(sc[k, 2]), LD(sc[k, 3])
        rec = {}
        ax, axp = np.abs(x), np.abs(x_prev)
        dk = x - x_prev
        # ---- rho sequence
        if k == 0:
            if rho != rho_start:
                res.fail("rho", 0, "rho_0 = %r, started at %r" % (float(rho), float(rho_start)))
        else:
            r0 = LD(sc[k - 1, 2])
            if float(rho) not in _steps(r0, f):
                res.fail("rho", k, "rho_k / rho_{k-1} = %r not in {1, f, f^2}" % float(rho / r0))
        rec["rho"] = (float(rho), float(rho_start if k == 0 else sc[k - 1, 2]), 0.0)
        # ---- sum|terms| of this row's products, and with the row before for the carried ones
        Qx, Cx = Q @ x, C @ x
        Lx, Rx = L @ x, R @ x
        T = dict(obj=np.abs(g) @ ax + ax @ (aQ @ ax) / 2,
                 pen=(aL @ ax) @ (aR @ ax),
                 phi=(aL @ ax + np.abs(lbL)) @ (aR @ ax + np.abs(lbR)))
        Tc = dict(T) if T_prev is None else {key: max(T[key], T_prev[key]) for key in T}
        T_obj = Tc["obj"]
        T_phi = Tc["phi"] if carried_C else T["phi"]
        T_pen = Tc["pen"] if carried_C else T["pen"]
        # ---- objective, phi, merit
        obj = g @ x + x @ Qx / 2
        phi = (Lx - lbL) @ (Rx - lbR)
        merit = obj + rho * (Lx @ Rx)
        rec["obj"] = (sc[k, 4], obj, G * T_obj)
        rec["phi"] = (sc[k, 1], phi, G * T_phi)
        rec["merit"] = (sc[k, 5], merit, G * (T_obj + rho * T_pen))
        # ---- step norm: x_k = x_{k-1} (+ perturbation) + alpha_k p_k, p_k = x_new - x_{k-1}: three roundings of size eps (|x_k| + |x_{k-1}|)
        a_eff = LD(1) if k == 0 else alpha
        dx_unknown = EPS * (ax + axp) + (PERTURB if (perturb and k >= 1) else LD(0))      # what d_k can differ from alpha_k p_k by
        rec["step"] = (float(a_eff * LD(sc[k, 6])), np.abs(dk).max(), MARGIN * _gamma(3) * (ax + axp).max() + (PERTURB if (perturb and k >= 1) else LD(0)))
        if k == 0 and not (sc[0, 3] == 1.0):
            res.fail("alpha", 0, "alpha_0 = %r, not 1" % sc[0, 3])
        # ---- the linear term of QP k and gtil_k
        updated = rho != rho_start
        gt = g + rho * gphi if (gtil_rule == "always" or updated) else g
        if k == 0 and not warm:
            gt = g      # a cold run starts with gtil = g (initializeSolver :966-967)
        gk = g if (k == 0 and zero_first) else rho * (C @ x_prev) + gt
        if k == 0:
            res.row0_penalty = not zero_first
            res.cx0 = float(np.abs(rho * (C @ x_prev)).max())
        # ---- step length
        if k >= 1:
            Kd = Q @ dk + rho * (C @ dk)
            grad = Qx_prev + rho * Cx_prev + gt
            q, l = dk @ Kd, dk @ grad
            ad = np.abs(dk)
            axn = np.abs(x_prev + dk / alpha) if alpha > 0 else axp      # |x_new|: Q p_k and (carried) C p_k are differences of two products
            # the loop's own evaluation (q_k = alpha^-2 q and l_k = alpha^-1 l, scaled to d_k) ...
            dq = G * (alpha * (ad @ ((aQ + rho * aC) @ (axn + axp))) + ad @ ((aQ + rho * aC) @ ad))
            dl = G * (ad @ ((aQ + rho * aC) @ np.maximum(axp, axpp) + np.abs(gt)))
            # ... and d_k against alpha_k p_k
            dq += 2 * (dx_unknown @ np.abs(Kd))
            dl += dx_unknown @ (np.abs(grad) + (aQ + rho * aC) @ ad)
            rel = (dl / abs(l) if l != 0 else LD(np.inf)) + (dq / abs(q) if q != 0 else LD(np.inf))
            ratio = float(-l / q) if q != 0 else float("nan")
            verdict = "undecidable"
            if not (0 < alpha <= 1):
                verdict = "bad"
            elif q + dq <= 0 or l - dl >= 0:
                verdict = "ok" if alpha == 1 else "bad"
            elif rel <= LD(0.1):
                lo, hi = (abs(l) - dl) / (q + dq), (abs(l) + dl) / (q - dq)
                if not (q > 0 and l < 0):
                    verdict = "bad"
                elif alpha < 1:
                    verdict = "ok" if lo <= 1 <= hi else "bad"
                else:
                    verdict = "ok" if hi >= 1 else "bad"
            if verdict == "undecidable":
                res.undecidable += 1
            else:
                res.decided += 1
            if verdict == "bad":
                res.fail("alpha", k, "alpha = %r but -l / q = %r (q = %.3e +- %.1e, l = %.3e +- %.1e)" % (float(alpha), ratio, float(q), float(dq), float(l), float(dl)))
            rec["alpha"] = (float(alpha), ratio, float(rel), verdict)
        # ---- stationarity
        if k == 0:
            sv = rho * Cx if zero_first else rho * (C @ dk)
            terms = rho * (aC @ (ax + axp)) + aQ @ (2 * ax) + 2 * np.abs(gt)
            dxu = LD(0) * ax
        else:
            pk = dk / alpha
            sv = alpha * rho * (C @ pk) - (1 - alpha) * (Q @ pk)
            axn = np.abs(x_prev + pk)
            terms = aQ @ (ax + axn + axp) + rho * (aC @ (ax + axp)) + 2 * np.abs(gt)
            # d_k / alpha_k against p_k: rho C and (1 - alpha) / alpha Q of the rounding of x_k, Q / alpha of the perturbation (it moved x_{k-1}, not x_new)
            dxu = rho * (aC @ dx_unknown) + ((1 - alpha) / alpha) * (aQ @ (EPS * (ax + axp))) + ((aQ @ np.full(n, PERTURB, dtype=LD)) / alpha if perturb else 0)
        b_stat = (G * terms + dxu).max() + res_tol * (1 + np.abs(gk).max())
        rec["stat"] = (sc[k, 0], np.abs(sv).max(), b_stat)
        for name in ("obj", "phi", "merit", "step", "stat"):
            r, ref, b = rec[name]
            if not (abs(LD(r) - ref) <= b):
                res.fail(name, k, "recorded %.17g, reference %.17g, |diff| %.3e > bound %.3e" % (float(r), float(ref), float(abs(LD(r) - ref)), float(b)))
            rec[name] = (float(r), float(ref), float(b))
        phi_bounds.append(rec["phi"][2]); stat_bounds.append(rec["stat"][2])
        res.records.append(rec)
        axpp = axp      # |x_{k-2}| of the next row: the carried products of its step length mix rows k - 1 and k - 2
        x_prev, Qx_prev, Cx_prev, T_prev = x, Qx, Cx, T

    if stats is not None and K > 0:
        _replay(res, opt, sc, phi_bounds, stat_bounds, rho_start, stats, X, x_ret)
    if check and res.failures:
        raise AuditError(res)
    return res


def _cmp_lt(a, b, tol):
    """a < b as the loop decides it: True / False, or None when the two sides lie within tol of each other"""
    if abs(a - b) <= tol:
        return None
    return bool(a < b)


def _replay(res, opt, sc, phi_b, stat_b, rho_start, stats, X, x_ret):
    """the decisions of runSolver's loop (src/LCQProblem.cpp:444-560, leyfferCheckPositive :1275-1313) from the recorded stat, phi, rho"""
    K = len(sc)
    nd, eta = int(_o(opt, "nDynamicPenalty")), float(_o(opt, "etaDynamicPenalty"))
    ctol, stol = float(_o(opt, "complementarityTolerance")), float(_o(opt, "stationarityTolerance"))
    f, max_rho, max_it = float(_o(opt, "penaltyUpdateFactor")), float(_o(opt, "maxPenaltyParameter")), int(_o(opt, "maxIterations"))
    ret = int(stats["returnValue"])
    if int(stats["iterTotal"]) != K:
        res.fail("decisions", None, "iterTotal %d, trace has %d rows" % (stats["iterTotal"], K))
    if int(round(sc[:, 7].sum())) != int(stats["subproblemIter"]) or np.any(sc[:, 7] != np.round(sc[:, 7])):
        res.fail("decisions", None, "sum of the QP iterations %r, subproblemIter %d" % (sc[:, 7].sum(), stats["subproblemIter"]))
    hist = []      # (phi, bound)
    outer = 0
    for k in range(K):
        stat, phi, rho = sc[k, 0], sc[k, 1], sc[k, 2]
        last = k == K - 1
        # the sets of outcomes the comparisons allow
        ley = {False}
        if nd > 0:
            if len(hist) < nd:
                pass
            else:
                res.window_shifts += 1
                small = _cmp_lt(phi, ctol, phi_b[k])
                below = [_cmp_lt(phi, eta * h, phi_b[k] + eta * hb) for h, hb in hist]
                if small is True or any(b is True for b in below):
                    ley = {False}
                elif small is None or any(b is None for b in below):
                    ley = {False, True}
                else:
                    ley = {True}
        st_small = _cmp_lt(stat, stol, stat_b[k])
        ph_small = _cmp_lt(phi, ctol, phi_b[k])
        conv = {True} if (st_small is True and ph_small is True) else ({False} if (st_small is False or ph_small is False) else {False, True})
        stat_upd = {True} if (st_small is True and ph_small is False) else ({False} if (st_small is False or ph_small is True) else {False, True})
        allowed = {int(a) + int(b) for a in ley for b in stat_upd}
        rho_next = float(stats["rhoOpt"]) if last else sc[k + 1, 2]
        u = [j for j, r in enumerate(_steps(rho, f)) if rho_next == r]
        u = u[0] if u else None
        if last:
            if (ret == 0) not in conv:
                res.fail("decisions", k, "last row: stat %.3e phi %.3e, returnValue %d" % (stat, phi, ret))
            if ret == 0:
                allowed = {int(a) for a in ley}      # converged: no stationarity update behind the Leyffer check
        elif conv == {True}:
            res.fail("decisions", k, "row converges (stat %.3e, phi %.3e) but the run went on" % (stat, phi))
        if u is None or u not in allowed:
            res.fail("decisions", k, "%d penalty update(s) after the row (rho %r -> %r), the recorded stat %.3e and phi %.3e allow %s"
                     % (-1 if u is None else u, rho, rho_next, stat, phi, sorted(allowed)))
            u = 0 if u is None else u
        outer += u
        res.leyffer_fired += ley == {True}
        res.updates += u
        res.double_updates += u == 2
        if u > 0 and nd > 0:
            hist = []
        elif nd > 0:
            hist.append((phi, phi_b[k]))
            hist = hist[-nd:]
        if not last and (k + 1 > max_it or rho_next > max_rho):
            res.fail("decisions", k, "the run went on past maxIterations / maxPenaltyParameter")
        if last and ret == 200 and not K > max_it:
            res.fail("decisions", k, "MAX_ITERATIONS_REACHED after %d iterates" % K)
        if last and ret == 201 and not rho_next > max_rho:
            res.fail("decisions", k, "MAX_PENALTY_REACHED at rho %r" % rho_next)
        if last and ret == 201 and K > max_it:
            res.fail("decisions", k, "MAX_PENALTY_REACHED after %d iterates: maxIterations is tested first" % K)
    if outer != int(stats["iterOuter"]):
        res.fail("decisions", None, "iterOuter %d, the rho sequence has %d updates" % (stats["iterOuter"], outer))
    if x_ret is not None and not np.array_equal(np.asarray(x_ret, dtype=np.float64), np.asarray(X[-1], dtype=np.float64)):
        res.fail("decisions", K - 1, "the last row is not the returned x bit for bit")


def last_qp_duals(d, scalars, xs, x_start, rho_start, y, layout, res_tol):
    """Are the returned duals y those of the last QP solved?  For a cold run without perturbStep that ended at row K - 1 (K >= 2) without
    converging, so that y is untransformed.  QP k has the linear term g_k = rho_k C x_{k-1} + gtil_k (rule "after_first_update") and the
    solution xnew_k = x_{k-1} + d_k / alpha_k; its multipliers satisfy Q xnew_k + g_k - E'y_E - y_box = 0 up to the subsolver's
    res_tol (1 + |g_k|inf).  layout "dense": y = [box (nV), A, L, R]; "sparse": y = [A, L, R].  Returns (residual of QP K - 1, its bound,
    residual of QP K - 2): the bound is res_tol (1 + |g_k|inf) plus MARGIN gamma_m sum|terms| of the residual's own sums plus what xnew_k
    cannot be known to from the trace, eps (|x_k| + |x_{k-1}|) / alpha_k per component, through |Q|."""
    n, nC, nK = int(d["nV"]), int(d["nC"]), int(d["nComp"])
    Q = np.asarray(d["Q"], dtype=np.float64).astype(LD)
    L = np.asarray(d["L"], dtype=np.float64).astype(LD); R = np.asarray(d["R"], dtype=np.float64).astype(LD)
    A = np.asarray(d["A"], dtype=np.float64).reshape(nC, n).astype(LD) if nC else np.zeros((0, n), dtype=LD)
    E = np.vstack([A, L, R])
    g, lbL, lbR = _vec(d, "g", n), _vec(d, "lbL", nK), _vec(d, "lbR", nK)
    C = complementarity_matrix(L, R)
    gphi = -(L.T @ lbR + R.T @ lbL)
    y = np.asarray(y, dtype=np.float64).astype(LD)
    ybox, yE = (y[:n], y[n:]) if layout == "dense" else (np.zeros(n, dtype=LD), y)
    sc = np.asarray(scalars, dtype=np.float64)
    X = np.asarray(xs, dtype=np.float64).astype(LD)
    K = len(sc)
    assert K >= 2 and yE.size == nC + 2 * nK
    start = np.zeros(n, dtype=LD) if x_start is None else np.asarray(x_start, dtype=np.float64).astype(LD)
    G = MARGIN * _gamma(n + E.shape[0] + int((C != 0).sum(axis=1).max()) + 8)

    def residual(k):
        xp = X[k - 1] if k >= 1 else start
        rho, alpha = LD(sc[k, 2]), LD(sc[k, 3])
        xn = xp + (X[k] - xp) / alpha
        gt = g + rho * gphi if rho != LD(rho_start) else g
        gk = rho * (C @ xp) + gt
        r = Q @ xn + gk - E.T @ yE - ybox
        terms = np.abs(Q) @ np.abs(xn) + rho * (np.abs(C) @ np.abs(xp)) + np.abs(gt) + np.abs(E).T @ np.abs(yE) + np.abs(ybox)
        unknown = np.abs(Q) @ (EPS * (np.abs(X[k]) + np.abs(xp)) / alpha)
        return float(np.abs(r).max()), float((G * terms + unknown).max() + LD(res_tol) * (1 + np.abs(gk).max()))

    r, bound = residual(K - 1)
    return r, bound, residual(K - 2)[0]


def audit_batch(bt, ds, which, opt, x_start, rho_start, warm, gtil_rule, res_tol, label, carried_C=False, densify=None, expect_ret=0):
    """audit() on the instances `which` of a solved batch handle bt (BatchLCQP or SparseBatchLCQP; the traces and statistics come through its
    solution() and trace()): ds the problem dicts (densify: dict -> dense layout, for the sparse arm), x_start None or one start per
    instance, rho_start a number or one per instance.  Prints one line per instance and the worst |recorded - reference| / bound per
    quantity; asserts that every instance passed and returned expect_ret (0: converged).  Returns {instance: AuditResult}."""
    x, _, st = bt.solution()
    worst, out = {}, {}
    for b in which:
        sc, xs = bt.trace(b)
        d = densify(ds[b]) if densify else ds[b]
        r = audit(d, opt, sc, xs, None if x_start is None else x_start[b], rho_start if np.isscalar(rho_start) else rho_start[b], warm, gtil_rule,
                  res_tol, stats=st[b], x_ret=x[b], carried_C=carried_C, check=False)
        for rec in r.records:
            for q in ("obj", "phi", "merit", "step", "stat"):
                got, ref, bound = rec[q]
                worst[q] = max(worst.get(q, 0.0), abs(got - ref) / bound if bound > 0 else 0.0)
        print(f"    {label} instance {b}: ret {st[b]['returnValue']} rows {len(sc)} rho -> {st[b]['rhoOpt']:g} step length decided {r.decided} undecidable {r.undecidable}"
              + "".join(f"\n      FAIL {f}" for f in r.failures))
        assert not r.failures, (label, b, r.failures)
        assert st[b]["returnValue"] == expect_ret, (label, b, st[b])
        out[b] = r
    print(f"    {label}: worst |recorded - reference| / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return out


def refuted_by_step_length(bt, ds, which, opt, x_start, rho_start, warm, gtil_rule, res_tol, carried_C=False, densify=None):
    """the instances whose trace fails `alpha` (and nothing else) when audited under gtil_rule: a rule for g~ is a claim the step lengths can refute"""
    x, _, st = bt.solution()
    hit = []
    for b in which:
        sc, xs = bt.trace(b)
        r = audit(densify(ds[b]) if densify else ds[b], opt, sc, xs, x_start[b], rho_start[b], warm, gtil_rule, res_tol, stats=st[b], x_ret=x[b],
                  carried_C=carried_C, check=False)
        assert set(r.failed()) <= {"alpha"}, (b, r.failures)
        if r.failures:
            hit.append(b)
    return hit
