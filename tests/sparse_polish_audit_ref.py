"""Reference for the active-set polish of the sparse arm, trial by trial, in np.longdouble on the densified problem, with no solver in the
loop (sp_polish_begin, sp_ph_trial, sp_ph_factor, sp_ph_correct in lcqpow_amd/csrc/lcqp_sparse_solver.hpp; the oracle's twin is sqp_polish).
This module imports neither the library nor the oracle; MARGIN = 4, gamma_k = k eps / (1 - k eps) and the failure-collecting result class
are those of tests/polish_audit_ref.py; the KKT matrix and its bound are those of tests/sparse_kkt_ref.py.  The inputs live in
tests/sparse_polish_cases.py.

The problem: min x'Qx/2 + g'x  s.t.  l <= E x <= u over E = [A; L; R].  Signs are the code's: r1 = -g - Qx - E'y; a LOWER row leaves on
y > ytol, an UPPER row on y < -ytol.

A STATE S_k is what SparseBatchLCQP.read_polish returns after a run that was allowed exactly k trials of the first QP (maxTrials = k,
maxRounds = 1, admmFirst = admmHot = 0, maxIterations = 0, perturbStep = 0).  With admmFirst = 0 the round preamble proposes the empty set
plus the equalities, so S_0 -- the polish's entry -- follows from the data: x0, y = 0, EQ where l == u (state_zero).  A QP that gives up in
sp_ph_correct leaves xt, yt behind its k-th correction, stt the set that correction used, r1 its right-hand side and ex = E x of the point
before it; a QP accepted in its k-th trial leaves the accepted point with NV_R1, NV_TMP, MV_EX of its stage 2 (maxIterations = 0 ends the
run in sp_ph_qpend's `done` branch, before r1 is shifted for the next QP).  rcs[k-1] is 0 for a rung whose QP was accepted.

Checks (the names of the failure list), each bound the rounding bound of the stated operation times MARGIN, with no free constant:
  inactive  yt == 0 exactly on rows with stt == INACT
  factor    stfValid == 1 and (stf != INACT) == (stt != INACT); (dpUsed, d2Used) is bit for bit the safe pair or the light pair of SpInfo, the
            light one only with lightOK && !bigReg; a trial that did not factorise keeps the pair
  scale     e1max = max row 1-norm of E to gamma_nnz; gs == 1 + |g|_inf and ytol == feasTol gs bit for bit; l, u are the problem's
  ex        ex_{k+1} = E x_k to gamma_{nnz_r} |E_r||x_k| per row
  status    trial k of sp_ph_trial replayed from (x_k, yt_k, stt_k): leaving rows exactly (two recorded doubles), entering rows by the
            interval e +- MARGIN gamma |E_r||x_k| (a row it leaves open is UNDECIDABLE: counted, not asserted); MI_NEW and stt_{k+1} match on
            every decidable row; trial 0 changes nothing (stt_1 == stt_0); the overshoot rule is replayed where it applies
  leave     the multiplier of every leaving row is zero in S_{k+1}
  rhs       r1_{k+1}: trial 0 or an unchanged set -- the true residual -g - Q x_k - E'yt_k; a changed set at trial > 0 -- the prediction
            sum_{leaving} E_r' yt_k[r], exactly zero on variables no leaving row touches.  Recorded, not asserted: |true residual - prediction|
            in units of dpUsed |x_k - x_{k-1}| (algebra says about one)
  correct   [x_{k+1} - x_k; (yt_{k+1} - yt_k')_W] solves [[Q + dp I, E_W'], [E_W, -d2 I]] [dx; dy] = [r1_{k+1}; b_W - ex_{k+1,W}]: the
            componentwise backward-error bound of tests/sparse_kkt_ref.py in the handle's ordering, widened by |K| eps (|x_k| + |x_{k+1}|)
            (likewise y) for the two vector operations; the bordered band gets that file's block-elimination rule, and every use of
            it is printed and recorded (SparsePolishAudit.widened)
  level     where the light pair was available and the trial factorised (plain band): the pivot test of sp_ph_factor on a long-double LDL'
            without pivoting in the device's ordering; a pivot within MARGIN gamma_N Wm_jj of its threshold is undecidable.  bigReg is the
            verdict of the variables' pivots alone: 1 where one surely fails, 0 where all surely pass -- also when a row sends the
            factorisation to the safe pair.  (`factor`: without a light attempt bigReg keeps its value; nothing clears it)
  accept    a rung that returned 0: nothing changes in the status replay, the stationarity and active-row tests hold (each decided by the
            interval of its long-double value; an open one makes the outcome undecidable), nrefine <= 2, the point did not move; a rung that
            did not return 0 is not a closed acceptable point, but for the refinement rule
  stored    accepted state: NV_TMP = Q xt, NV_R1 = -gk - Q xt - E'yt, MV_EX = E xt; xq == xt, yq == yt, st == stt bit for bit; gk == g bit
            for bit on the zero-penalty QP
  feasible, signs   accepted state: every row within ftol plus its rounding of its bounds, active rows within resTol (1 + bmax) (or their
            rounding floor), multipliers with the sign of their state to ytol
"""
import numpy as np

import sparse_kkt_ref as KR
from polish_audit_ref import EPS, EPSK, INACT, LD, LOWER, MARGIN, UPPER, EQ, PolishAudit, _gamma, _ld, _o

CHECKS = ("inactive", "factor", "scale", "ex", "status", "leave", "rhs", "correct", "level", "accept", "stored", "feasible", "signs")
EPS52 = LD(KR.EPS)


class SparsePolishAudit(PolishAudit):
    def __init__(self):
        PolishAudit.__init__(self)
        self.worst = {}          # check -> worst error / bound
        self.prediction = []     # per predicted right-hand side: |true residual - prediction|_inf / (dpUsed |dx|_inf)
        self.solve_share = []    # beside it: max |rhs - K [dx; dy]| over the variables of the correction before, in the same unit
        self.widened = []        # (where, ratio): corrections of a bordered band held to 8 x the float64 block elimination's own ratio
        self.levels = []         # per correction: 0 light, 1 safe
        self.events = dict(enter=0, leave=0, unchanged=0, accepted=0, predicted=0, factorised=0, bigReg=0)

    def ratio(self, check, err, bound, where, text=""):
        """every entry of err within bound; the worst ratio is kept"""
        err, bound = np.asarray(err, dtype=LD), np.broadcast_to(np.asarray(bound, dtype=LD), np.shape(err))
        if err.size == 0:
            return
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / bound, LD(0))
        w = float(np.nanmax(r)) if np.isfinite(r).any() or not r.size else float("inf")
        if not np.isfinite(err).all():
            w = float("inf")
        self.worst[check] = max(self.worst.get(check, 0.0), w)
        if not (np.isfinite(err).all() and (err <= bound).all()):
            i = int(np.argmax(np.where(np.isfinite(r), r, np.inf)))
            self.fail(check, where, "%s entry %d: error %.3g, bound %.3g" % (text, i, float(err.ravel()[i]), float(bound.ravel()[i])))


def state_zero(x0, l, u):
    """S_0: the entry of the first QP's polish with admmFirst = 0 (module docstring)"""
    l, u = np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)
    m = l.size
    return dict(xt=np.asarray(x0, dtype=np.float64).copy(), yt=np.zeros(m), stt=np.where(l == u, EQ, INACT).astype(np.int32), xinf=0.0, nrefine=0,
                stfValid=0, stf=np.zeros(m, dtype=np.int32), bigReg=0, zero=True)


class _Problem:
    def __init__(self, Q, E, g, l, u):
        self.Q64, self.E64 = np.asarray(Q, dtype=np.float64), np.asarray(E, dtype=np.float64)
        self.Q, self.E, self.g = _ld(Q), _ld(E), _ld(g)
        self.Qa, self.Ea = np.abs(self.Q), np.abs(self.E)
        self.g64 = np.asarray(g, dtype=np.float64)
        self.l64, self.u64 = np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)
        self.l, self.u = _ld(l), _ld(u)
        self.m, self.n = self.E.shape
        import scipy.sparse as sp
        self.sp = dict(Q=sp.csc_matrix(self.Q64), E=sp.csc_matrix(self.E64))      # what sparse_kkt_ref.kkt_dense takes
        self.nzr = (self.E64 != 0).sum(axis=1)                                   # terms of E_r x
        self.nzc = (self.Q64 != 0).sum(axis=1) + (self.E64 != 0).sum(axis=0)     # terms of (Q x)_i + (E'y)_i
        self.gr = np.array([_gamma(max(int(k), 1)) for k in self.nzr], dtype=LD)
        self.gc = np.array([_gamma(int(k) + 2) for k in self.nzc], dtype=LD)

    def Ex(self, x):
        x = _ld(x)
        return self.E @ x, MARGIN * self.gr * (self.Ea @ np.abs(x))

    def residual(self, g, x, y):
        """-g - Qx - E'y, its bound, Q x, E'y"""
        x, y, g = _ld(x), _ld(y), _ld(g)
        qx, s = self.Q @ x, self.E.T @ y
        terms = np.abs(g) + self.Qa @ np.abs(x) + self.Ea.T @ np.abs(y)
        return -g - qx - s, MARGIN * self.gc * terms, qx, s


def replay_status(P, S, opt):
    """the status test of sp_ph_trial from (x, yt, stt) of S: (new status, open rows, leaving rows, e, bound of e)"""
    feas64 = float(_o(opt, "feasTol"))
    feas = LD(feas64)
    st = np.asarray(S["stt"]).copy()
    y = np.asarray(S["yt"], dtype=np.float64)
    ytol = float(S["ytol"])
    leave = ((st == LOWER) & (y > ytol)) | ((st == UPPER) & (y < -ytol))
    e, be = P.Ex(S["xt"])
    be = be * (LD(1) + feas)
    ftol = feas * (LD(1) + np.abs(e))
    ina = st == INACT
    with np.errstate(invalid="ignore"):
        dlo, dhi = (P.l - ftol) - e, e - (P.u + ftol)      # > 0: violated
        opn = ina & ((np.abs(dlo) <= be) | (np.abs(dhi) <= be))
        vlo, vhi = ina & ~opn & (dlo > be), ina & ~opn & (dhi > be)
    new = st.copy()
    new[leave] = INACT
    new[vlo] = LOWER
    new[vhi & ~vlo] = UPPER
    return new, opn, leave, e, be


def _cmp_le(val, bound, tol, btol=LD(0)):      # True / False / None (open)
    if val + bound <= tol - btol: return True
    if val - bound > tol + btol: return False
    return None


def acceptable(P, g, S, e, be, opt):
    """the two acceptance tests of sp_ph_trial at the point of S on its set: (stationarity, active rows, loose), each True / False / None"""
    rtol = float(_o(opt, "resTol"))
    st = np.asarray(S["stt"])
    act = st != INACT
    r1, b1, qx, s = P.residual(g, S["xt"], S["yt"])
    rscale = (np.abs(_ld(g)) + np.abs(qx) + np.abs(s)).max()
    rtolS = max(LD(rtol * float(S["gs"])), LD(64.0 * EPSK) * rscale)
    stat_ok = _cmp_le(np.abs(r1).max(), b1.max(), rtolS, LD(64.0 * EPSK) * b1.max())
    if not act.any():
        return stat_ok, True, False
    bb = np.where(st == UPPER, P.u, P.l)
    bba = np.abs(np.where(act, bb, LD(0)))
    rr = np.abs(np.where(act, bb - e, LD(0)))
    thr = LD(16.0 * EPSK) * (bba + LD(float(S["e1max"])) * LD(float(np.abs(S["xt"]).max())))
    sure = act & (rr - be > thr)
    maybe = act & (rr + be > thr)
    tol_eq = LD(rtol) * (LD(1) + bba.max())
    eq_hi = (rr + be)[maybe].max() if maybe.any() else LD(0)
    eq_lo = (rr - be)[sure].max() if sure.any() else LD(0)
    eq_ok = True if eq_hi <= tol_eq else (False if eq_lo > tol_eq else None)
    loose = True if sure.any() else (None if maybe.any() else False)
    return stat_ok, eq_ok, loose


def check_state(P, S, opt, res, where, g=None, corrected=True):
    """inactive, factor, scale: invariants of any state (g: the linear term gs and ytol belong to, None: not checked)"""
    st, y = np.asarray(S["stt"]), np.asarray(S["yt"])
    if np.any(y[st == INACT] != 0.0):
        res.fail("inactive", where, "non-zero multiplier on inactive rows %s" % np.nonzero((y != 0) & (st == INACT))[0][:4])
    if corrected:
        if S["stfValid"] != 1 or not np.array_equal(np.asarray(S["stf"]) != INACT, st != INACT):
            res.fail("factor", where, "the factor in memory is not the factor of the trial's set (stfValid %d)" % S["stfValid"])
        pair = (S["dpUsed"], S["d2Used"])
        safe, light = (S["delta"], S["delta2"]), (S["deltaS"], S["delta2S"])
        if pair not in (safe, light):
            res.fail("factor", where, "(dpUsed, d2Used) = %r is neither pair of the instance" % (pair,))
        elif pair == light and not (S["lightOK"] and not S["bigReg"]):
            res.fail("factor", where, "the light pair with lightOK %d, bigReg %d" % (S["lightOK"], S["bigReg"]))
    e1 = P.Ea.sum(axis=1).max()
    res.ratio("scale", abs(LD(S["e1max"]) - e1), MARGIN * _gamma(int(P.nzr.max())) * e1, where, "e1max")
    if not (np.array_equal(S["l"], P.l64) and np.array_equal(S["u"], P.u64)):
        res.fail("scale", where, "l, u differ from the problem's bounds")
    if g is not None:
        gs = 1.0 + float(np.abs(np.asarray(g, dtype=np.float64)).max())
        if S["gs"] != gs or S["ytol"] != float(_o(opt, "feasTol")) * gs:
            res.fail("scale", where, "gs %.17g, ytol %.17g against 1 + |g|_inf = %.17g" % (S["gs"], S["ytol"], gs))


def _kkt(P, dp, d2, use):
    return KR.kkt_dense(P.sp, dp, d2, use)


def check_correction(P, S0, S1, yprime, ordering, kb, res, where):
    """`correct`: the step S0 -> S1 against the KKT system S1 records (module docstring); returns max |rhs - K [dx; dy]| over the variables"""
    n, m = P.n, P.m
    st = np.asarray(S1["stt"])
    use = st != INACT
    perm = np.asarray(ordering)
    K = _kkt(P, S1["dpUsed"], S1["d2Used"], use)
    Kp = K[np.ix_(perm, perm)]
    L, D, Wm = KR.ldl_nopivot(Kp, KR.ref_dtype(n + m))
    bb = np.where(st == UPPER, P.u, P.l)
    rhs = np.concatenate([_ld(S1["r1"]), np.where(use, bb - _ld(S1["ex"]), LD(0))])
    x0, x1, y1 = _ld(S0["xt"]), _ld(S1["xt"]), _ld(S1["yt"])
    yp = _ld(yprime)
    sol = np.concatenate([x1 - x0, np.where(use, y1 - yp, LD(0))])
    slop = np.concatenate([np.abs(x0) + np.abs(x1), np.where(use, np.abs(y1) + np.abs(yp), LD(0))]) * EPS52
    resid = np.abs(rhs - _ld(K) @ sol)[perm]
    N = n + m
    bound = LD((6 * N + 8) * KR.EPS) * (Wm.astype(LD) @ np.abs(sol)[perm] + np.abs(rhs)[perm]) + (np.abs(_ld(K)) @ slop)[perm]
    if kb and not (resid <= bound).all():      # the block-elimination rule of tests/test_gpu_sparse_factor.py
        B = rhs[perm].astype(np.float64)[:, None]
        rr, rb = KR.residual_and_bound(Kp, Wm, KR.bordered_ref(Kp, kb, B), B)
        ref_ratio = float(np.where(rb > 0, rr / np.where(rb > 0, rb, 1), 0).max())
        res.widened.append((where, ref_ratio))
        print("    %s: `correct` above the scalar bound; the float64 block elimination's own worst error / bound = %.3e" % (where, ref_ratio))
        bound = bound * LD(max(1.0, 8.0 * ref_ratio))
    res.ratio("correct", resid, bound, where, "K [dx; dy] - rhs (growth %.1e)" % float(KR.growth(Kp, Wm, sol[perm].astype(np.float64)[:, None]).max()))
    return float(np.abs(rhs - _ld(K) @ sol)[:n].max())      # the stationarity block of the residual: what the solve leaves beside dp dx


def check_level(P, S0, S1, ordering, res, where):
    """`level`: the pivot test of sp_ph_factor replayed for the set of S1 (plain band or general engine; the light pair was available before)"""
    n, m = P.n, P.m
    use = np.asarray(S1["stt"]) != INACT
    perm = np.asarray(ordering)
    Kp = _kkt(P, S1["deltaS"], S1["delta2S"], use)[np.ix_(perm, perm)]
    _, D, Wm = KR.ldl_nopivot(Kp, KR.ref_dtype(n + m))
    D = D.astype(LD)
    bD = MARGIN * _gamma(n + m) * np.diag(Wm).astype(LD)
    sc = LD(S1["scale"])
    isvar = perm < n
    isrow = ~isvar & use[np.where(isvar, 0, perm - n)]
    tv, tr = LD(1e-8) * sc, -LD(1e-8) / sc
    bad_var = isvar & (D + bD <= tv)
    bad_row = isrow & (D - bD >= tr)
    ok_all = (isvar & (D - bD > tv)) | (isrow & (D + bD < tr)) | ~(isvar | isrow)
    res.decisions += 1
    # bigReg is the variables' verdict alone (sp_ph_factor looks at every pivot of the light attempt, whatever the rows say)
    big = 1 if bad_var.any() else (0 if (ok_all | ~isvar).all() else None)
    res.events["bigReg"] += int(big == 1)
    if big is not None and S1["bigReg"] != big:
        res.fail("level", where, "bigReg %d, the variables' pivots of the long-double LDL' give %d" % (S1["bigReg"], big))
    if bad_var.any() or bad_row.any():
        want = 1
    elif ok_all.all():
        want = 0
    else:
        res.undecidable += 1
        return
    got = 0 if S1["dpUsed"] == S1["deltaS"] else 1
    if got != want:
        res.fail("level", where, "the factorisation ran at level %d, the pivot test on the long-double LDL' gives %d" % (got, want))


def check_transition(P, g, S0, S1, rc1, opt, trial, max_trials, ordering, kb, res, where):
    """trial number `trial` (0-based) from S0, held against S1, the state of the rung that was allowed trial + 1 trials (rc1: its return)"""
    n, m = P.n, P.m
    if S0.get("zero"):
        S0 = dict(S0, ytol=S1["ytol"], gs=S1["gs"], e1max=S1["e1max"])
    new, opn, leave, e, be = replay_status(P, S0, opt)
    st0, st1, new1 = np.asarray(S0["stt"]), np.asarray(S1["stt"]), np.asarray(S1["new"])
    dec = ~opn
    res.decisions += m
    res.undecidable += int(opn.sum())
    res.transitions += 1
    res.open_transitions += int(opn.any())
    # ex
    res.ratio("ex", np.abs(_ld(S1["ex"]) - e), be, where, "ex against E x_k")
    # status: what the test proposed
    if not np.array_equal(new1[dec], new[dec]):
        bad = np.nonzero(dec & (new1 != new))[0]
        res.fail("status", where, "%d rows of MI_NEW differ from the replay, first row %d: recorded %d, replay %d (before %d)"
                 % (bad.size, bad[0], new1[bad[0]], new[bad[0]], st0[bad[0]]))
    changed_sure = bool((new[dec] != st0[dec]).any())
    changed_rec = bool((new1 != st0).any())          # the open rows as the device decided them
    nact, nchg = int((new1 != INACT).sum()), int((new1 != st0).sum())
    overshoot = trial >= 2 and changed_rec and nact > n and nchg > max(n // 2, 32)
    stat_ok, eq_ok, loose = acceptable(P, g, S0, e, be, opt) if trial > 0 else (False, False, False)
    closed_ok = (not changed_sure) and not opn.any() and stat_ok is True and eq_ok is True
    open_ok = (not changed_sure) and stat_ok is not False and eq_ok is not False
    refine = loose is not False and int(S0.get("nrefine", 0)) < 2 and trial + 1 < max_trials
    if rc1 == 0:
        res.events["accepted"] += 1
        res.outcomes.append("accept" if closed_ok else "undecidable")
        if changed_sure or stat_ok is False or eq_ok is False:
            res.fail("accept", where, "the QP was accepted but the replay says changed %s, stationarity %s, active rows %s" % (changed_sure, stat_ok, eq_ok))
        if not (np.array_equal(st1, st0) and np.array_equal(S1["xt"], S0["xt"]) and np.array_equal(S1["yt"], S0["yt"])):
            res.fail("accept", where, "an accepted point or its set moved")
        if S1["bigReg"] != int(S0.get("bigReg", 0)):
            res.fail("factor", where, "bigReg changed in an accepting trial")
        if S1["nrefine"] > 2:
            res.fail("accept", where, "nrefine %d" % S1["nrefine"])
        return dict(accepted=True, e=e, be=be)
    if closed_ok and not refine:      # (a refinement -- one more correction for the active rows alone -- is the one exception)
        res.fail("accept", where, "a closed acceptable point was not accepted")
    res.outcomes.append("undecidable" if open_ok and not closed_ok else ("overshoot" if overshoot else "correct"))
    if overshoot:
        if not (np.array_equal(st1, st0) and np.array_equal(S1["xt"], S0["xt"])):
            res.fail("status", where, "the overshoot rule applies but the state moved")
        return dict(accepted=False, overshoot=True)
    # the set the correction used
    applied = trial > 0 and changed_rec
    want = new1 if applied else st0
    if not np.array_equal(st1, want):
        res.fail("status", where, "stt differs from %s at rows %s" % ("MI_NEW" if applied else "the set before (nothing is applied at trial 0 / an unchanged set)",
                                                                       np.nonzero(st1 != want)[0][:4]))
    left = applied & (new1 == INACT) & (st0 != INACT)
    if applied and not np.array_equal(left[dec], leave[dec]):
        res.fail("status", where, "leaving rows differ from the exact replay")
    if np.any(np.asarray(S1["yt"])[left] != 0.0):
        res.fail("leave", where, "leaving rows keep a multiplier: %s" % np.nonzero(left & (np.asarray(S1["yt"]) != 0))[0][:4])
    res.events["enter"] += int(((new1 != INACT) & (st0 == INACT)).sum()) if applied else 0
    res.events["leave"] += int(left.sum())
    res.events["unchanged"] += int(trial > 0 and not changed_rec)
    y0 = np.asarray(S0["yt"], dtype=np.float64)
    yprime = np.where(left, 0.0, y0)
    # rhs
    r1 = _ld(S1["r1"])
    true, btrue, _, _ = P.residual(g, S0["xt"], yprime)
    if not applied:
        res.ratio("rhs", np.abs(r1 - true), btrue, where, "r1 against the true residual")
    else:
        res.events["predicted"] += 1
        yl = _ld(np.where(left, y0, 0.0))
        pred = P.E.T @ yl
        cnt = (P.E64[left] != 0).sum(axis=0)
        bp = MARGIN * np.array([_gamma(int(k) + 1) for k in cnt], dtype=LD) * (P.Ea.T @ np.abs(yl))
        res.ratio("rhs", np.abs(r1 - pred), bp, where, "r1 against the prediction")
        if np.any(np.asarray(S1["r1"])[cnt == 0] != 0.0):
            res.fail("rhs", where, "the predicted r1 is not exactly zero on variables no leaving row touches")
        if S0.get("xprev") is not None:
            dx = float(np.abs(_ld(S0["xt"]) - _ld(S0["xprev"])).max())
            if dx > 0 and S0.get("dpUsed"):
                res.prediction.append(float(np.abs(true - pred).max()) / (float(S0["dpUsed"]) * dx))
                res.solve_share.append(float(S0.get("solve_resid", 0.0)) / (float(S0["dpUsed"]) * dx))
    # factor reuse, level, correct
    factorised = (not S0.get("stfValid")) or not np.array_equal(np.asarray(S0["stf"]) != INACT, st1 != INACT)
    res.events["factorised"] += int(factorised)
    if not factorised and (S1["dpUsed"], S1["d2Used"]) != (S0["dpUsed"], S0["d2Used"]):
        res.fail("factor", where, "the regularisation pair changed without a factorisation")
    res.levels.append(0 if S1["dpUsed"] == S1["deltaS"] else 1)
    solve_resid = check_correction(P, S0, S1, yprime, ordering, kb, res, where)
    tried_light = factorised and S1["lightOK"] and not S0.get("bigReg", 0)
    if tried_light and kb == 0:
        check_level(P, S0, S1, ordering, res, where)
    elif not tried_light and S1["bigReg"] != int(S0.get("bigReg", 0)):      # only a light attempt can set it, and nothing clears it
        res.fail("factor", where, "bigReg went from %d to %d without a light attempt" % (S0.get("bigReg", 0), S1["bigReg"]))
    return dict(accepted=False, solve_resid=solve_resid)


def check_accepted(P, S, opt, res, where, g=None):
    """stored, feasible, signs at an accepted state (g: the linear term of a zero-penalty QP, None: gk is what NV_GK holds)"""
    n, m = P.n, P.m
    feas = LD(float(_o(opt, "feasTol")))
    rtol = LD(float(_o(opt, "resTol")))
    st = np.asarray(S["stt"])
    act = st != INACT
    gk = S["gk"]
    r1, b1, qx, s = P.residual(gk, S["xt"], S["yt"])
    res.ratio("stored", np.abs(_ld(S["qx"]) - qx), MARGIN * P.gc * (P.Qa @ np.abs(_ld(S["xt"]))), where, "NV_TMP against Q xt")
    res.ratio("stored", np.abs(_ld(S["r1"]) - r1), b1, where, "NV_R1 against -gk - Q xt - E'yt")
    e, be = P.Ex(S["xt"])
    res.ratio("stored", np.abs(_ld(S["ex"]) - e), be, where, "MV_EX against E xt")
    if not (np.array_equal(S["xq"], S["xt"]) and np.array_equal(S["yq"], S["yt"]) and np.array_equal(S["st"], S["stt"])):
        res.fail("stored", where, "xq, yq, st are not the bits of xt, yt, stt")
    if g is not None and not np.array_equal(np.asarray(gk), np.asarray(g, dtype=np.float64)):
        res.fail("stored", where, "gk differs from g in bits")
    if not S["haveSolution"]:
        res.fail("stored", where, "haveSolution is not set")
    ftol = feas * (LD(1) + np.abs(e))
    with np.errstate(invalid="ignore"):
        slack = np.minimum(e - (P.l - ftol), (P.u + ftol) - e)
        babs = np.where(e - P.l <= P.u - e, np.abs(P.l), np.abs(P.u))
    babs = np.where(np.isfinite(babs), babs, LD(0))
    bs = be + MARGIN * _gamma(2) * (babs + ftol)
    infeas = slack < -bs
    if infeas.any():
        r = int(np.nonzero(infeas)[0][0])
        res.fail("feasible", where, "row %d (%s) violates its bound by %.6g beyond ftol (%d rows)" % (r, "active" if act[r] else "inactive", float(-slack[r]), infeas.sum()))
    if act.any():
        bb = np.where(st == UPPER, P.u, P.l)
        bba = np.abs(np.where(act, bb, LD(0)))
        thr = LD(16.0 * EPSK) * (bba + LD(float(S["e1max"])) * LD(float(np.abs(S["xt"]).max())))
        tol = np.maximum(rtol * (LD(1) + bba.max()), thr) + be
        rr = np.abs(np.where(act, bb - e, LD(0)))
        if np.any(act & (rr > tol)):
            r = int(np.argmax(np.where(act, rr - tol, -np.inf)))
            res.fail("feasible", where, "active row %d is %.6g from its bound" % (r, float(rr[r])))
    y, ytol = np.asarray(S["yt"]), float(S["ytol"])
    if np.any((st == LOWER) & (y > ytol)) or np.any((st == UPPER) & (y < -ytol)) or np.any(~act & (y != 0.0)):
        res.fail("signs", where, "a multiplier has the wrong sign beyond ytol, or an inactive row has one")


def audit_ladder(Q, E, g, l, u, states, rcs, opt, ordering, x0=None, kb=0, res=None):
    """states[k-1], rcs[k-1]: the state and the QP's return (0: accepted) of the run with maxTrials = k, k = 1 ... K; an accepted rung ends a
    ladder.  Returns the SparsePolishAudit with the counts, the outcomes per rung, the worst ratio per check and the prediction record."""
    res = res or SparsePolishAudit()
    P = _Problem(Q, E, g, l, u)
    prev = state_zero(np.zeros(P.n) if x0 is None else x0, l, u)
    xprev = None
    for k, (S, rc) in enumerate(zip(states, rcs), start=1):
        w = "S_%d" % k
        check_state(P, S, opt, res, w, g=g)
        out = check_transition(P, g, dict(prev, xprev=xprev), S, rc, opt, k - 1, k, ordering, kb, res, "S_%d -> S_%d" % (k - 1, k))
        if rc == 0:
            check_accepted(P, S, opt, res, w, g=g)
            break
        if out.get("overshoot"):
            break
        xprev, prev = prev["xt"], dict(S, solve_resid=out.get("solve_resid", 0.0))
    return res


def audit_accepted(Q, E, l, u, S, opt, res=None, where="accepted"):
    """an accepted state behind hot starts: stored, feasible, signs, inactive, factor (gk is what NV_GK holds)"""
    res = res or SparsePolishAudit()
    P = _Problem(Q, E, np.zeros(np.asarray(Q).shape[0]), l, u)
    check_state(P, S, opt, res, where, g=S["gk"])
    check_accepted(P, S, opt, res, where)
    return res
