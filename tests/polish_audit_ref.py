"""Reference for the dense subsolver's active-set polish, trial by trial, in np.longdouble, with no solver in the loop.

qp_polish (lcqpow_amd/csrc/lcqp_dev.hpp; the oracle's twin: oracle/lcqp_oracle.c, qp_polish) is audited from recorded STATES.  A state
S_k is what a solve that was allowed exactly k trials left behind (maxRounds = 1, no ADMM, maxTrials = k: the polish gives up after its k-th
correction, or returns at the stage-2 test of its k-th trial), read back without a launch (lcqp_hip_batch_read_polish / _read_working_set; the
oracle: orc_qp_read_polish).  A state is a dict with the names of capi._read_polish: xt, xs, xref, yt, stt, l, u, spv and -- the device only --
ex, mg, rn, hotc, hotv, nHot, row_slot, slot_row, nT, ndep, r1s, gs, aty, qxn, exs.  What a state lacks is not checked (the oracle screens
nothing and stores no row norms).  This module imports neither the library nor the oracle.

The problem: min x'Qx/2 + g'x  s.t.  l <= E x <= u over the stacked rows E (k_qp_solve: [A; box rows], k_lcqp_run: [A; L; R; box rows]).
Signs are the code's (OSQP's): stationarity is -g - Qx - E'y = 0 (qp_polish, stage 2), a row on its lower bound has y <= 0, on its upper y >= 0.

check_state -- invariants of any state:
  rn       |rn_r - |E_r|_2| <= MARGIN gamma_n |E_r|_2 and rn_r >= |E_r|_2 (1 - MARGIN gamma_n)          (wg_row_norms, lcqp_wg.hpp:379-413)
  hot      hotc / hotv are exactly the rows with one non-zero, column and value bit for bit; nHot is their count          (:399-409, :808-814)
  active   no active row carries a screening margin: mg = -1 (:839, :929), or -- a row that entered in the state's last trial, whose margin is
           written only by the next trial's step (a) (:892-893) -- what stage 1 read it with, never above 1e-10; check_transition holds the rows
           that were active before and after the trial to exactly -1.  y = 0 on inactive rows
  screen   NO SCREENED ROW IS UNSAFE: an inactive row with mg_r > 1e-10 (the rows stage 1 does not read, :845) has the true slack
           min(E_r xs - (l_r - ftol), (u_r + ftol) - E_r xs), ftol = feasTol (1 + |E_r xs|), at least mg_r - gamma_{n+2} (|E_r||xs| + |b_r|),
           b_r the bound the minimum is taken at.  xs = V_XS, the x of the last sweep: the margins belong to it (sweep_distance, :766-775; the fresh
           margins of :894 and :929 are taken at the same x).  No free constant and no MARGIN: the kernel's own 1e-13 |x| and shrinkF terms
           (:759, :774) are what make it hold.
  factor   ex_r of a row in the factor equals its bound bit for bit (:1141); row_slot and slot_row are inverse to each other; nT is the number
           of active rows when ndep = 0

replay_transition -- trial number t >= 1 (0-based, :792) from S_t with a sweep over ALL rows:
  leave    LOWER with y > ytol or UPPER with y < -ytol, ytol = feasTol (1 + |g|_inf) (:838, :1180): a comparison of two recorded doubles, replayed
           exactly
  enter    e_r = E_r x in long double for every row that is inactive after the leaving step, screened or not: e_r < l_r - ftol enters LOWER,
           e_r > u_r + ftol enters UPPER (:889-894).  With the cap (polishes that start from an empty set, :784, :818; more than max(n/8, 16)
           violated rows, :871-872) only rows at or above the cut of twelve bisection steps on [0, largest violation] enter (:873-880).
           A row whose e_r lies within MARGIN gamma_{n+2} |E_r||x| of its threshold -- or whose violation lies that close to a midpoint the
           bisection visits, each midpoint being uncertain by the bound of the largest violation -- is UNDECIDABLE: counted, not asserted.  A
           bisection count that the uncertain rows could carry across the cap leaves every violated row of that trial undecidable.
  stage 2  runs when nothing changed (:913-916).  r1 = -g - Qx - E'y - spv (x - xref) (:922), tolerance max(resTol (1 + |g|_inf),
           64 * 2.221e-16 max_i (|g_i| + |Qx|_i + |E'y|_i)) (:939-940); rows: |b_r - E_r x|, counted only above 16 * 2.221e-16 (|b_r| + rn_r |x|_2)
           (:950-951), against resTol (1 + max|b_r|) (:964).  Outcomes: "refine" (:964-965; never in the last trial a polish is allowed),
           "anchor" (xref moves to x, :967-969), "accept" (:971-979), "correct" (a full correction).  Every comparison is decided by the
           interval [value - bound, value + bound] with bound = MARGIN gamma_m sum|terms|; an open comparison makes the outcome "undecidable".
check_transition holds S_{t+1} to the replay: the status of every decidable row; accept <=> the solve returned 0; xref moved exactly on "anchor".

check_point -- (x, y_W) of a state solves [[Q + spv I, E_W'], [E_W, 0]] [x; y_W] = [-g + spv xref; b_W] (every correction, full or predicted,
  is an exact Newton step of the proximal QP, :703-717): float64 LU refined with long-double residuals, error against
  1e-12 n cond_2(K_W) max(1, |x|_inf, |y|_inf), the project's bound for such solves (tests/test_gpu_sensitivity.py).  Only for ndep = 0.
check_accepted -- an accepted state (:971-977): qxn = Qx, aty = -E'y, r1s = -g - Qx - E'y, exs = Ex on the rows stage 2 read (the active ones;
  the others keep what stage 1 read earlier and are held by `screen` instead), each to MARGIN gamma_m sum|terms|; gs = g bit for bit;
  every row feasible to ftol plus that rounding, screened or not; multiplier signs to ytol.

MARGIN = 4 as in tests/trace_audit_ref.py, for the reason its docstring gives.
"""
import numpy as np

LD = np.longdouble
EPS = LD(2) ** -53
MARGIN = LD(4)
INACT, LOWER, UPPER, EQ = 0, 1, 2, 3
EPSK = 2.221e-16      # the kernel's own constant in its two rounding floors
CHECKS = ("rn", "hot", "active", "screen", "factor", "status", "stage2", "point", "stored", "feasible", "signs")


class PolishAuditError(AssertionError):
    def __init__(self, result):
        self.result = result
        head = "; ".join("%s at %s: %s" % f for f in result.failures[:6])
        AssertionError.__init__(self, "%d polish audit failure(s): %s" % (len(result.failures), head))


class PolishAudit:
    """collects failures (check, where, text) and the counts the caps are taken on"""

    def __init__(self):
        self.failures = []
        self.decisions = 0            # row decisions replayed
        self.undecidable = 0          # ... of which the intervals left open
        self.transitions = 0
        self.open_transitions = 0     # transitions with at least one open decision
        self.screened = []            # per audited state: share of the rows with mg > 1e-10
        self.ratios = []              # per audited point: error / bound of check_point
        self.outcomes = []            # per transition: stage-2 outcome or None

    def fail(self, check, where, text):
        self.failures.append((check, where, text))

    def failed(self):
        return sorted({f[0] for f in self.failures})

    def verify(self):
        if self.failures:
            raise PolishAuditError(self)
        return self


def _o(opt, name):
    return opt[name] if isinstance(opt, dict) else getattr(opt, name)


def _gamma(m):
    m = LD(m)
    return m * EPS / (LD(1) - m * EPS)


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def stacked_rows(A, lb=None, ub=None, L=None, R=None):
    """E as the kernels stack it: [A; L; R; one unit row per variable with a finite lb or ub, ascending] (float64)"""
    n = A.shape[1]
    blocks = [np.asarray(A, dtype=np.float64).reshape(-1, n)]
    if L is not None:
        blocks += [np.asarray(L, dtype=np.float64).reshape(-1, n), np.asarray(R, dtype=np.float64).reshape(-1, n)]
    if lb is not None or ub is not None:
        lo = np.full(n, -np.inf) if lb is None else np.asarray(lb, dtype=np.float64)
        hi = np.full(n, np.inf) if ub is None else np.asarray(ub, dtype=np.float64)
        idx = np.nonzero(np.isfinite(lo) | np.isfinite(hi))[0]
        blocks.append(np.eye(n)[idx])
    return np.vstack(blocks)


def _slack(E, Ea, x, l, u, feas):
    """true slack of every row at x, the bound it is taken at, and sum|terms| of E_r x"""
    e = E @ x
    ftol = feas * (LD(1) + np.abs(e))
    with np.errstate(invalid="ignore"):
        lo, hi = e - (l - ftol), (u + ftol) - e
    at_lo = lo <= hi
    b = np.where(at_lo, l, u)
    return e, np.where(at_lo, lo, hi), np.where(np.isfinite(b), np.abs(b), LD(0)), Ea @ np.abs(x)


def check_state(E, S, opt, res, where="state"):
    """invariants of any state (module docstring); E float64 [mE][n]"""
    mE, n = E.shape
    El, Ea = _ld(E), np.abs(_ld(E))
    l, u, st, y = _ld(S["l"]), _ld(S["u"]), np.asarray(S["stt"]), np.asarray(S["yt"])
    feas = LD(_o(opt, "feasTol"))
    act = st != INACT
    nz = (E != 0).sum(axis=1)
    if np.any(y[~act] != 0.0):
        res.fail("active", where, "non-zero multiplier on inactive rows %s" % np.nonzero((y != 0) & ~act)[0][:4])
    if S.get("rn") is not None and S.get("rnReady", 1):
        nrm = np.sqrt((El * El).sum(axis=1)); rn = _ld(S["rn"]); b = MARGIN * _gamma(n) * nrm
        bad = np.nonzero((np.abs(rn - nrm) > b) | (rn < nrm - b))[0]
        if bad.size:
            res.fail("rn", where, "row %d: rn %.17g, |E_r| %.17g" % (bad[0], float(rn[bad[0]]), float(nrm[bad[0]])))
    if S.get("hotc") is not None and S.get("rnReady", 1):
        hotc, hotv = np.asarray(S["hotc"]), np.asarray(S["hotv"])
        one = nz == 1
        col = np.where(one, np.argmax(E != 0, axis=1), -1)
        if not np.array_equal(hotc, col):
            res.fail("hot", where, "hotc differs from the single-non-zero rows at rows %s" % np.nonzero(hotc != col)[0][:4])
        elif not np.array_equal(hotv[one], E[one, col[one]]):
            res.fail("hot", where, "hotv differs in bits")
        if S.get("nHot") is not None and int(S["nHot"]) != int(one.sum()):
            res.fail("hot", where, "nHot %d, rows with one non-zero %d" % (S["nHot"], one.sum()))
    if S.get("mg") is not None:
        mg = np.asarray(S["mg"], dtype=np.float64)
        if np.any(mg[act] > 1e-10):
            res.fail("active", where, "active rows with a screening margin: %s" % np.nonzero(act & (mg > 1e-10))[0][:4])
        xs = _ld(S["xs"])
        e, slack, babs, terms = _slack(El, Ea, xs, l, u, feas)
        scr = ~act & (mg > 1e-10)
        res.screened.append(float(scr.sum()) / max(mE, 1))
        short = scr & (slack < _ld(mg) - _gamma(n + 2) * (terms + babs))
        if short.any():
            r = int(np.nonzero(short)[0][0])
            res.fail("screen", where, "row %d is screened with mg %.6g but its slack at xs is %.6g (%d rows)" % (r, mg[r], float(slack[r]), short.sum()))
    if S.get("row_slot") is not None:
        rs = np.asarray(S["row_slot"])
        if S.get("slot_row") is not None:
            sr = np.asarray(S["slot_row"])[:int(S["ns"])] if S.get("ns") is not None else np.asarray(S["slot_row"])
            held = np.nonzero(sr >= 0)[0]
            if not (np.array_equal(rs[sr[held]], held) and (rs >= 0).sum() == held.size):
                res.fail("factor", where, "row_slot and slot_row are not inverse to each other")
        if np.any(~act & (rs >= 0)):
            res.fail("factor", where, "inactive rows in the factor: %s" % np.nonzero(~act & (rs >= 0))[0][:4])
        if S.get("ndep") == 0 and S.get("nT") is not None and not (int(S["nT"]) == int(act.sum()) == int((rs >= 0).sum())):
            res.fail("factor", where, "nT %d, active rows %d, rows with a slot %d" % (S["nT"], act.sum(), (rs >= 0).sum()))
        if S.get("ex") is not None and not S.get("accepted", False):
            inf = rs >= 0
            bb = np.where(st == UPPER, S["u"], S["l"])
            if not np.array_equal(np.asarray(S["ex"])[inf], bb[inf]):
                res.fail("factor", where, "ex of a row in the factor is not its bound")
    return res


def _violation(e, l, u, feas):
    ftol = feas * (LD(1) + np.abs(e))
    with np.errstate(invalid="ignore"):
        return np.where(e < l - ftol, l - e, np.where(e > u + ftol, e - u, LD(0)))


def replay_transition(Q, E, g, S, opt, trial, max_trials, cap_on, res=None):
    """Trial `trial` >= 1 replayed from the state S (module docstring).  Returns dict(status: expected I_STT, open: rows left undecided,
    outcome: None (stage 2 does not run) | "accept" | "anchor" | "correct" | "refine" | "undecidable", nleave, nenter, capped)."""
    assert trial >= 1 and S.get("ndep", 0) == 0
    mE, n = E.shape
    Ql, El, gl = _ld(Q), _ld(E), _ld(g)
    Ea = np.abs(El)
    x, xref, y = _ld(S["xt"]), _ld(S["xref"]), np.asarray(S["yt"], dtype=np.float64)
    l64, u64 = np.asarray(S["l"], dtype=np.float64), np.asarray(S["u"], dtype=np.float64)
    l, u = _ld(l64), _ld(u64)
    st = np.asarray(S["stt"]).copy()
    feas64, rtol64 = float(_o(opt, "feasTol")), float(_o(opt, "resTol"))
    feas = LD(feas64)
    gsc = 1.0 + float(np.abs(np.asarray(g, dtype=np.float64)).max())      # the kernel's doubles (:1179-1180)
    ytol = feas64 * gsc
    # (a) leaving rows: recorded doubles against a double
    leave = ((st == LOWER) & (y > ytol)) | ((st == UPPER) & (y < -ytol))
    st[leave] = INACT
    yl = _ld(np.where(leave, 0.0, y))
    # (b) every inactive row
    e = El @ x
    terms = Ea @ np.abs(x)
    be = MARGIN * _gamma(n + 2) * terms * (LD(1) + feas)
    ftol = feas * (LD(1) + np.abs(e))
    ina = st == INACT
    with np.errstate(invalid="ignore"):
        dlo, dhi = (l - ftol) - e, e - (u + ftol)      # > 0: violated
    opn = ina & ((np.abs(dlo) <= be) | (np.abs(dhi) <= be))
    vlo, vhi = ina & (dlo > be), ina & (dhi > be)
    viol = _violation(e, l, u, feas)
    capped = False
    nviol_lo, nviol_hi = int((vlo | vhi).sum()), int((vlo | vhi | opn).sum())
    cap = max(n // 8, 16)
    if cap_on and nviol_hi > cap:
        if nviol_lo <= cap:
            opn = opn | vlo | vhi      # whether the cap binds is itself open
        else:
            capped = True
            cand = vlo | vhi | opn
            vmax = viol[cand].max()
            bmax = be[cand].max()
            lo_, hi_ = LD(0), vmax
            lost = False
            for _ in range(12):
                mid = LD(0.5) * (lo_ + hi_)
                sure = int((cand & (viol - be - bmax >= mid)).sum())
                maybe = int((cand & (viol + be + bmax >= mid)).sum())
                if (sure > cap) != (maybe > cap):
                    lost = True
                    break
                opn = opn | (cand & (np.abs(viol - mid) <= be + bmax))
                if sure > cap: lo_ = mid
                else: hi_ = mid
            if lost:
                opn = opn | vlo | vhi
            else:
                below = viol < lo_
                vlo, vhi = vlo & ~below, vhi & ~below
    vlo, vhi = vlo & ~opn, vhi & ~opn
    st[vlo] = LOWER
    st[vhi] = UPPER
    changed_sure = bool(leave.any() or vlo.any() or vhi.any())
    out = dict(status=st, open=opn, nleave=int(leave.sum()), nenter=int(vlo.sum() + vhi.sum()), capped=capped, outcome=None)
    if res is not None:
        res.decisions += mE
        res.undecidable += int(opn.sum())
        res.transitions += 1
        res.open_transitions += int(opn.any())
    if changed_sure:
        return out
    if opn.any():
        out["outcome"] = "undecidable"
        return out
    # (c) stage 2
    act = st != INACT
    qx = Ql @ x
    s = El.T @ yl
    ro = -gl - qx - s
    prox = LD(S["spv"]) * (x - xref)
    r1 = ro - prox
    m = n + int(act.sum()) + 4
    tsum = np.abs(gl) + np.abs(Ql) @ np.abs(x) + Ea.T @ np.abs(yl) + np.abs(prox)
    b1 = MARGIN * _gamma(m) * tsum
    cv = np.abs(gl) + np.abs(qx) + np.abs(s)
    rscale = cv.max()
    rtolS = max(LD(rtol64 * gsc), LD(64.0 * EPSK) * rscale)
    brt = LD(64.0 * EPSK) * (MARGIN * _gamma(m) * tsum).max()

    def cmp_le(val, bound, tol, btol=LD(0)):      # True / False / None (open)
        if val + bound <= tol - btol: return True
        if val - bound > tol + btol: return False
        return None

    i = int(np.argmax(np.abs(r1)))
    stat_ok = cmp_le(np.abs(r1).max(), b1.max(), rtolS, brt)
    bb = np.where(st == UPPER, u, l)
    xn = np.sqrt((x * x).sum())
    rn = _ld(S["rn"]) if S.get("rn") is not None else np.sqrt((El * El).sum(axis=1))
    rr = np.abs(np.where(act, bb - e, LD(0)))
    thr = LD(16.0 * EPSK) * (np.abs(np.where(act, bb, LD(0))) + rn * xn)
    brow = MARGIN * _gamma(n + 2) * (terms + np.abs(np.where(act, bb, LD(0))))
    sure_above = act & (rr - brow > thr)
    tol_eq = LD(rtol64) * (LD(1) + (np.abs(bb[act]).max() if act.any() else LD(0)))
    eq_hi = (rr + brow)[act].max() if act.any() else LD(0)
    eq_lo = (rr - brow)[sure_above].max() if sure_above.any() else LD(0)
    eq_ok = True if eq_hi <= tol_eq else (False if eq_lo > tol_eq else None)
    if stat_ok is False or eq_ok is False:
        out["outcome"] = "correct"
        return out
    if stat_ok is None or eq_ok is None:
        out["outcome"] = "undecidable"
        return out
    if trial + 1 < max_trials and S.get("nrefine", 0) < 2:
        slot = np.asarray(S["row_slot"]) >= 0 if S.get("row_slot") is not None else act
        if (sure_above & slot).any():
            out["outcome"] = "refine"
            return out
        if (act & slot & (rr + brow > thr)).any():      # a row of the factor that may or may not be at its floor
            out["outcome"] = "undecidable"
            return out
    orig_ok = cmp_le(np.abs(ro).max(), b1.max(), rtolS, brt)
    out["outcome"] = "undecidable" if orig_ok is None else ("accept" if orig_ok else "anchor")
    return out


def check_transition(Q, E, g, S0, S1, rc1, opt, trial, max_trials, cap_on, res, where="transition"):
    """S1 (the state after trial `trial`, rc1 the solve's return) held to the replay from S0"""
    rp = replay_transition(Q, E, g, S0, opt, trial, max_trials, cap_on, res)
    res.outcomes.append(rp["outcome"])
    if rc1 == 0 and rp["outcome"] not in ("accept", "undecidable"):
        res.fail("stage2", where, "the solve returned 0 but the replay's outcome is %s (%d left, %d entered)" % (rp["outcome"], rp["nleave"], rp["nenter"]))
        return rp
    dec = ~rp["open"]
    st1 = np.asarray(S1["stt"])
    if not np.array_equal(st1[dec], rp["status"][dec]):
        bad = np.nonzero(dec & (st1 != rp["status"]))[0]
        res.fail("status", where, "%d rows differ from the full-sweep replay, first row %d: recorded %d, replay %d (before %d)"
                 % (bad.size, bad[0], st1[bad[0]], rp["status"][bad[0]], np.asarray(S0["stt"])[bad[0]]))
    if S1.get("mg") is not None:
        stay = (np.asarray(S0["stt"]) != INACT) & (st1 != INACT)
        if np.any(np.asarray(S1["mg"])[stay] != -1.0):
            res.fail("active", where, "rows active before and after the trial with mg != -1: %s" % np.nonzero(stay & (np.asarray(S1["mg"]) != -1.0))[0][:4])
    if rp["outcome"] == "accept" and rc1 != 0:
        res.fail("stage2", where, "the replay accepts the point, the solve returned %d" % rc1)
    if rp["outcome"] == "accept" and not np.array_equal(S1["xt"], S0["xt"]):
        res.fail("stage2", where, "an accepted point moved")
    if rp["outcome"] == "undecidable":      # an open outcome still has only these consequences
        moved = not np.array_equal(np.asarray(S1["xref"]), np.asarray(S0["xref"]))
        if (moved and not np.array_equal(np.asarray(S1["xref"]), np.asarray(S0["xt"]))) or (rc1 == 0 and (moved or not np.array_equal(S1["xt"], S0["xt"]))):
            res.fail("stage2", where, "xref or x moved in a way no stage-2 outcome allows")
    else:
        want = S0["xt"] if rp["outcome"] == "anchor" else S0["xref"]
        if not np.array_equal(np.asarray(S1["xref"]), np.asarray(want)):
            res.fail("stage2", where, "xref %s" % ("did not move on a re-anchoring" if rp["outcome"] == "anchor" else "moved"))
    return rp


def kkt_point(Q, E, g, S, extended=True):
    """(x*, y*_W, W, cond_2(K_W)) of the proximal QP on the working set of S: float64 LU, refined with long-double residuals when `extended`"""
    n = Q.shape[0]
    W = np.nonzero(np.asarray(S["stt"]) != INACT)[0]
    m = W.size
    K = np.zeros((n + m, n + m))
    K[:n, :n] = np.asarray(Q, dtype=np.float64) + float(S["spv"]) * np.eye(n)
    K[:n, n:] = E[W].T
    K[n:, :n] = E[W]
    bW = np.where(np.asarray(S["stt"])[W] == UPPER, np.asarray(S["u"])[W], np.asarray(S["l"])[W])
    rhs = np.concatenate([-np.asarray(g, dtype=np.float64) + float(S["spv"]) * np.asarray(S["xref"]), bW])
    sol = np.linalg.solve(K, rhs)
    if extended:
        KL, rl, sl = K.astype(LD), rhs.astype(LD), sol.astype(LD)
        for _ in range(3):
            sl = sl + np.linalg.solve(K, (rl - KL @ sl).astype(np.float64)).astype(LD)
        sol = sl
    sv = np.linalg.svd(K, compute_uv=False)
    return sol[:n], sol[n:], W, float(sv.max() / sv.min())


def check_point(Q, E, g, S, res, where="point", extended=True):
    """the point of S against the KKT solution on its working set; returns error / bound"""
    assert S.get("ndep", 0) == 0
    n = Q.shape[0]
    xr, yr, W, cond = kkt_point(Q, E, g, S, extended)
    x, y = _ld(S["xt"]), _ld(S["yt"])[W]
    err = max(float(np.abs(x - xr).max()), float(np.abs(y - yr).max()) if W.size else 0.0)
    bound = 1e-12 * n * cond * max(1.0, float(np.abs(x).max()), float(np.abs(y).max()) if W.size else 0.0)
    res.ratios.append(err / bound)
    if not err <= bound:
        res.fail("point", where, "error %.3g against the bound %.3g (|W| = %d, cond %.3g)" % (err, bound, W.size, cond))
    return err / bound


def check_accepted(Q, E, g, S, opt, res, where="accepted"):
    """the stored hot-start state and the feasibility of ALL rows at an accepted point (module docstring)"""
    mE, n = E.shape
    Ql, El, gl = _ld(Q), _ld(E), _ld(g)
    Ea = np.abs(El)
    x, y = _ld(S["xt"]), _ld(S["yt"])
    l, u, st = _ld(S["l"]), _ld(S["u"]), np.asarray(S["stt"])
    feas = LD(_o(opt, "feasTol"))
    act = st != INACT
    na = int(act.sum())
    qx, s = Ql @ x, El.T @ y
    tq, ts = np.abs(Ql) @ np.abs(x), Ea.T @ np.abs(y)
    e, slack, babs, terms = _slack(El, Ea, x, l, u, feas)
    if S.get("qxn") is not None:
        for name, ref, b in (("qxn", qx, MARGIN * _gamma(n) * tq),
                             ("aty", -s, MARGIN * _gamma(n + na + 2) * (np.abs(gl) + tq + ts)),      # formed as g + Qx + r1 (:975)
                             ("r1s", -gl - qx - s, MARGIN * _gamma(n + na + 2) * (np.abs(gl) + tq + ts))):
            d = np.abs(_ld(S[name]) - ref)
            if np.any(d > b):
                i = int(np.argmax(d - b))
                res.fail("stored", where, "%s[%d] = %.17g, reference %.17g, bound %.3g" % (name, i, S[name][i], float(ref[i]), float(b[i])))
        if not np.array_equal(np.asarray(S["gs"]), np.asarray(g, dtype=np.float64)):
            res.fail("stored", where, "gs differs from g in bits")
        d = np.abs(_ld(S["exs"]) - e)
        b = MARGIN * _gamma(n) * terms
        if np.any(d[act] > b[act]):
            i = int(np.nonzero(act & (d > b))[0][0])
            res.fail("stored", where, "exs[%d] = %.17g, E_r x = %.17g, bound %.3g" % (i, S["exs"][i], float(e[i]), float(b[i])))
    infeas = slack < -(MARGIN * _gamma(n + 2) * (terms + babs))
    if infeas.any():
        r = int(np.nonzero(infeas)[0][0])
        res.fail("feasible", where, "row %d (%s) violates its bound by %.6g beyond ftol (%d rows)"
                 % (r, "active" if act[r] else "inactive", float(-slack[r]), infeas.sum()))
    ytol = float(_o(opt, "feasTol")) * (1.0 + float(np.abs(np.asarray(g, dtype=np.float64)).max()))
    y64 = np.asarray(S["yt"])
    if np.any((st == LOWER) & (y64 > ytol)) or np.any((st == UPPER) & (y64 < -ytol)) or np.any(~act & (y64 != 0.0)):
        res.fail("signs", where, "a multiplier has the wrong sign beyond ytol, or an inactive row has one")
    return res


def audit_ladder(Q, E, g, states, rcs, opt, cap_on, res=None, extended=True, screening=True):
    """states[k-1], rcs[k-1]: the state and return of the solve with maxTrials = k, k = 1 ... K (rcs[K-1] == 0 ends a ladder).  Every state gets
    the invariants and the point; every pair the transition; an accepted last state the stored-state checks."""
    res = res or PolishAudit()
    for k, (S, rc) in enumerate(zip(states, rcs), start=1):
        w = "S_%d" % k
        assert S.get("ndep", 0) == 0, "the cases are built to have no dependent rows"
        if not screening:
            S = {kk: v for kk, v in S.items() if kk != "mg"}
        check_state(E, dict(S, accepted=(rc == 0)), opt, res, w)
        check_point(Q, E, g, S, res, w, extended)
        if k >= 2:
            check_transition(Q, E, g, states[k - 2], S, rc, opt, k - 1, k, cap_on, res, "S_%d -> S_%d" % (k - 1, k))
        if rc == 0:
            check_accepted(Q, E, g, S, opt, res, w)
    return res


# ---- cases (shared by tests/test_polish_audit_ref.py and tests/test_gpu_polish_audit.py) -----------------------------------------------------
def polish_case(n, m, box, seed, equalities=True, violated=0.5):
    """A strictly convex QP whose rows mix the classes the polish treats differently: one-sided, two-sided, equality rows and rows with a
    single non-zero (every fifth row; their columns are distinct and carry no box bound, so no two active rows are parallel).  About a third
    of the rows (and of the box bounds) are TIGHT around the unconstrained minimiser x*, a share `violated` of them violated there; the rest
    lie 3 to 6 row norms away and stay screened; the row norms spread over three decades.  From x0 = 0 with an empty set the cold trial lands on x*, so the ladder then passes through
    trials that enter rows, trials that drop rows and unchanged trials."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    Q = B.T @ B / n + 0.5 * np.eye(n)
    Q = 0.5 * (Q + Q.T)
    g = rng.standard_normal(n)
    xs = -np.linalg.solve(Q, g)
    A = rng.standard_normal((m, n)) / np.sqrt(n)
    single = np.arange(2, m, 5)
    assert single.size <= n // 2
    A[single] = 0.0
    A[single, rng.permutation(n // 2)[:single.size]] = rng.uniform(0.5, 2.0, single.size) * rng.choice([-1.0, 1.0], single.size)
    ax = A @ xs
    nrm = np.sqrt((A * A).sum(axis=1))
    tight = rng.random(m) < 1.0 / 3.0
    lbA, ubA = np.full(m, -np.inf), np.full(m, np.inf)
    neq = 0
    for r in range(m):
        kind = r % 4      # 0: lower, 1: upper, 2: two-sided, 3: two-sided, or an equality among the first tight ones
        if tight[r]:
            d = nrm[r] * rng.uniform(0.05, 0.5) * (1.0 if rng.random() < violated else -1.0)      # > 0: violated at x*
            if kind == 3 and equalities and neq < 3:
                lbA[r] = ubA[r] = ax[r] + 0.4 * d
                neq += 1
            elif kind == 1: ubA[r] = ax[r] - d
            elif kind == 0: lbA[r] = ax[r] + d
            else: lbA[r] = ax[r] + d; ubA[r] = lbA[r] + nrm[r] * rng.uniform(0.5, 1.0)
        else:
            w = nrm[r] * rng.uniform(3.0, 6.0)
            if kind != 1: lbA[r] = ax[r] - w
            if kind != 0: ubA[r] = ax[r] + w
    # row norms over three decades (each row scaled together with its bounds: the same feasible set): a margin bookkeeping that drops |E_r|
    # is wrong by that factor
    f = 10.0 ** rng.uniform(-1.5, 1.5, m)
    A, lbA, ubA = A * f[:, None], lbA * f, ubA * f
    d = dict(n=n, m=m, Q=Q, g=g, A=A, lbA=lbA, ubA=ubA, lb=None, ub=None, xstar=xs)
    if box:
        lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
        for i in range(n // 2, n):
            if i % 3 == 2: continue
            t = rng.random() < 1.0 / 3.0
            dd = rng.uniform(0.05, 0.5) * (1.0 if rng.random() < violated else -1.0) if t else -rng.uniform(3.0, 6.0)
            lb[i] = xs[i] + dd
            if i % 3 == 0: ub[i] = lb[i] + (rng.uniform(0.5, 1.0) if t else 8.0)
        d["lb"], d["ub"] = lb, ub
    d["E"] = stacked_rows(A, d["lb"], d["ub"])
    return d


# (name, n, m, box, seed, equalities, share of the tight rows violated at x*).  The first case has no equality rows: an equality is active from the
# start (qp_solve in lcqp_dev.hpp), and the cap on entering rows is for polishes that start from an EMPTY set (qp_polish, cold entry: capOn).
QP_CASES = (("40x96-cap", 40, 96, False, 2, False, 0.7),
            ("40x96", 40, 96, False, 2, True, 0.5),
            ("200x330-box", 200, 330, True, 1, True, 0.5),
            ("300x100", 300, 100, False, 17, True, 0.5),
            ("600x200-box", 600, 200, True, 2, True, 0.5))
MAX_LADDER = 16
