"""tests/sparse_polish_audit_ref.py checked without a device.  A float64 numpy MODEL of the sparse polish (model_polish below: the trial order
and the rules of sqp_polish / sp_ph_trial, a dense np.linalg.solve of the regularised KKT system in place of the band LDL') produces the
maxTrials ladders of the cases the device test climbs (tests/test_gpu_sparse_polish_audit.py) from their problem data alone.  The reference
passes every model ladder, and each seeded corruption of one model state fails the check that holds the corrupted quantity -- and no check
of another state.

The model's ladders also fix the cases: undecidable row decisions are capped at 1 % of all decisions and open transitions at 10 %, the dense
audit's caps; the inputs (sparse_polish_cases.band_instances, the circle example) are chosen so that the model stays inside them, which
is asserted here.  The overshoot hand-over (trial >= 2, more active rows than variables, more than max(n / 2, 32) changes) is not reachable at
these shapes: the band case has m = 48 rows for n = 64 variables, and on the circle no trial changes more than 32 rows after the second."""
import numpy as np
import pytest

import sparse_kkt_ref as KR
import sparse_polish_audit_ref as R
import sparse_polish_cases as C
from polish_audit_ref import EQ, INACT, LOWER, UPPER

MAX_LADDER = 16


def options(**kw):
    import lcqpow_amd as la
    return la.default_options(**kw)


def model_polish(Q, E, g, l, u, x0, opt, max_trials, light, bug=None):
    """(state, rc): the first QP's polish from the empty set plus the equalities, allowed max_trials trials; rc 0 = accepted.  The state has
    the names of SparseBatchLCQP.read_polish.  bug = (name, trial): one seeded mistake in that trial (BUGS below), everything after it
    computed consistently from what the mistake left."""
    bug_name, bug_trial = bug or (None, -1)
    n, m = Q.shape[0], E.shape[0]
    scale = float(np.abs(np.diag(Q)).max())
    pairs = dict(delta=opt.proxBig * scale, delta2=1e-9 / scale, deltaS=opt.proxSmall * scale, delta2S=1e-14 / scale)
    dp, d2, big_reg = pairs["delta"], pairs["delta2"], 0      # the pair of the factor in memory (none yet)
    gs = 1.0 + float(np.abs(g).max())
    ytol = opt.feasTol * gs
    e1max = float(np.abs(E).sum(axis=1).max())
    x, y = np.array(x0, dtype=float), np.zeros(m)
    st = np.where(l == u, EQ, INACT).astype(np.int32)
    stf, stf_valid, nrefine, xinf, trial = np.zeros(m, dtype=np.int32), 0, 0, 0.0, 0
    r1, qx, ex, new = np.zeros(n), np.zeros(n), np.zeros(m), st.copy()

    def state(rc):
        S = dict(pairs, n=n, m=m, trial=trial, nrefine=nrefine, stfValid=stf_valid, bigReg=big_reg, haveSolution=int(rc == 0), lightOK=int(light), kb=0,
                 gs=gs, ytol=ytol, dpUsed=dp, d2Used=d2, xinf=xinf, e1max=e1max, scale=scale, xt=x.copy(), r1=r1.copy(), qx=qx.copy(), gk=g.copy(),
                 yt=y.copy(), ex=ex.copy(), l=l.copy(), u=u.copy(), stt=st.copy(), stf=stf.copy(), new=new.copy())
        S.update(xq=x.copy() if rc == 0 else np.zeros(n), yq=y.copy() if rc == 0 else np.zeros(m), st=st.copy() if rc == 0 else np.zeros(m, dtype=np.int32))
        return S, rc

    while True:
        hit = bug_name if trial == bug_trial else None
        ex_old, qx_old = ex, qx
        ex = E @ x
        ftol = opt.feasTol * (1.0 + np.abs(ex))
        ina, act = st == INACT, st != INACT
        new = st.copy()
        new[ina & (ex < l - ftol)] = LOWER
        new[ina & ~(ex < l - ftol) & (ex > u + ftol)] = UPPER
        new[((st == LOWER) & (y > ytol)) | ((st == UPPER) & (y < -ytol))] = INACT
        bb = np.where(st == UPPER, u, l)
        above = act & ~(np.abs(np.where(act, bb - ex, 0.0)) <= 16.0 * 2.221e-16 * (np.abs(np.where(act, bb, 0.0)) + e1max * xinf))
        res_eq = np.abs(bb - ex)[above].max() if above.any() else 0.0
        bmax = np.abs(bb[act]).max() if act.any() else 0.0
        if hit == "status":      # a row that is inside its bounds enters
            new[np.nonzero((st == INACT) & (new == INACT) & np.isfinite(l))[0][0]] = LOWER
        changed = int((new != st).sum())
        have_r1 = False
        if trial == 0 or not changed:
            qx = Q @ x
            s = E.T @ y
            r1 = (-g - qx) - s
            rscale = (np.abs(g) + np.abs(qx) + np.abs(s)).max()
            have_r1 = True
            if trial > 0 and np.abs(r1).max() <= max(opt.resTol * gs, 64.0 * 2.221e-16 * rscale) and res_eq <= opt.resTol * (1.0 + bmax):
                if not (above.any() and nrefine < 2 and trial + 1 < max_trials):
                    if hit == "stored":      # NV_TMP left from the sweep before
                        qx = qx_old
                    return state(0)
                nrefine += 1
        if changed and trial > 0:
            if trial >= 2 and int((new != INACT).sum()) > n and changed > max(n // 2, 32):
                return state(1)
            left = (new == INACT) & (st != INACT)
            yl = np.where(left, y, 0.0)
            if hit == "rhs":      # the largest leaving term is missing from the prediction
                yl[np.argmax(np.abs(yl))] = 0.0
            r1 = (r1 if have_r1 else np.zeros(n)) + E.T @ yl
            if hit == "leave":      # one leaving multiplier is kept
                left = left.copy(); left[np.nonzero(left)[0][0]] = False
            y = np.where(left, 0.0, y)
            st = new.copy()
        use = st != INACT
        if hit == "ex":      # E x of the trial before on the right-hand side
            ex = ex_old
        def kkt(a, b):
            K = np.zeros((n + m, n + m))
            K[:n, :n] = Q + a * np.eye(n)
            K[n:, :n] = np.where(use[:, None], E, 0.0); K[:n, n:] = K[n:, :n].T
            K[n + np.arange(m), n + np.arange(m)] = np.where(use, -b, -1.0)
            return K
        if not stf_valid or not np.array_equal(stf != INACT, use):      # a factorisation: the light pair first where it is on offer
            level = 0 if (light and not big_reg) else 1
            if level == 0:      # the pivot test, on an LDL' without pivoting in the model's ordering (variables, then rows)
                D = KR.ldl_nopivot(kkt(pairs["deltaS"], pairs["delta2S"]), np.float64)[1]
                bad_var = not (D[:n] > 1e-8 * scale).all()
                bad_row = not (D[n:][use] < -1e-8 / scale).all()
                big_reg = int(bad_var)
                level = int(bad_var or bad_row)
            dp, d2 = (pairs["delta"], pairs["delta2"]) if level else (pairs["deltaS"], pairs["delta2S"])
            stf, stf_valid = st.copy(), 1
        other = (pairs["deltaS"], pairs["delta2S"]) if dp == pairs["delta"] else (pairs["delta"], pairs["delta2"])
        K = kkt(*(other if hit == "correct" else (dp, d2)))      # "correct": the step is computed with the other pair
        rhs = np.concatenate([r1, np.where(use, np.where(st == UPPER, u, l) - ex, 0.0)])
        sol = np.linalg.solve(K, rhs)
        # (one step of refinement: LU with partial pivoting is backward stable by norm only, and the rows of E span three decades; the
        # audit's bound is the componentwise one of an LDL' without pivoting)
        sol = sol + np.linalg.solve(K, rhs - K @ sol)
        x = x + sol[:n]
        xinf = float(np.abs(x).max())
        y = np.where(use, y + sol[n:], y)
        trial += 1
        if trial >= max_trials:
            return state(1)


dense_case = C.dense_case


def model_ladder(c, opt, light, limit=MAX_LADDER):
    """the states S_1 ... S_K of fresh model runs with maxTrials = 1 ... K, K the first that is accepted (or the limit)"""
    states, rcs = [], []
    for k in range(1, limit + 1):
        S, rc = model_polish(c["Q"], c["E"], c["g"], c["l"], c["u"], c["x0"], opt, k, light)
        states.append(S); rcs.append(rc)
        if rc == 0:
            break
    return states, rcs


CASES = {"band light 0": ("band", 0, True), "band light 1": ("band", 1, True), "band light 2": ("band", 2, True), "band safe 0": ("band", 0, False),
         "semidefinite 0": ("semi", 0, True), "semidefinite 1": ("semi", 1, True), "semidefinite 2": ("semi", 2, True), "circle safe": ("circle", 0, False)}
CIRCLE_RUNGS = 5      # the circle's ladder is audited up to here; it needs no accepted rung


@pytest.fixture(scope="module")
def ladders():
    opt = options()
    inst = dict(band=C.band_instances(3), semi=C.semidefinite_instances(3), circle=C.circle_instances(1))
    out = {}
    for name, (kind, b, light) in CASES.items():
        c = dense_case(inst[kind][b])
        out[name] = (c,) + model_ladder(c, opt, light, CIRCLE_RUNGS if kind == "circle" else MAX_LADDER)
    return out


def audit(c, states, rcs, opt):
    n, m = c["Q"].shape[0], c["E"].shape[0]
    return R.audit_ladder(c["Q"], c["E"], c["g"], c["l"], c["u"], states, rcs, opt, np.arange(n + m), x0=c["x0"])


@pytest.mark.parametrize("name", list(CASES))
def test_model_ladders_pass_the_audit(ladders, name):
    c, states, rcs = ladders[name]
    res = audit(c, states, rcs, options())
    print("  %s: %d rungs, outcomes %s, open %d of %d decisions, %d of %d transitions, events %s\n    worst ratios %s\n    prediction distance %s"
          % (name, len(states), res.outcomes, res.undecidable, res.decisions, res.open_transitions, res.transitions, res.events,
             {k: "%.2e" % v for k, v in res.worst.items()}, ["%.3g" % v for v in res.prediction]))
    res.verify()
    assert res.undecidable <= 0.01 * res.decisions and res.open_transitions <= 0.1 * res.transitions
    kind, _, light = CASES[name]
    big = [S["bigReg"] for S in states]
    print("    levels %s, bigReg per state %s" % (res.levels, big))
    if kind == "semi":
        # a variable's pivot fails in the first factorisation: the safe pair from there on, for good, with the light pair still on offer
        assert all(S["lightOK"] == 1 for S in states) and big == [1] * len(states) and set(res.levels) == {1} and res.events["bigReg"] == 1
        assert all(S["dpUsed"] == S["delta"] and S["d2Used"] == S["delta2"] for S in states) and rcs[-1] == 0
    else:
        assert big == [0] * len(states) and (0 in res.levels if light else set(res.levels) == {1})
    if kind == "band":
        ev = res.events
        assert rcs[-1] == 0 and ev["enter"] > 0 and ev["leave"] > 0 and ev["unchanged"] > 0 and ev["accepted"] == 1 and ev["predicted"] > 0
    elif kind == "circle":
        assert 2 <= len(states) <= CIRCLE_RUNGS


def test_the_overshoot_rule_is_out_of_reach(ladders):
    """no transition of a model ladder meets trial >= 2 && nact > n && changed > max(n / 2, 32)"""
    for name, (c, states, rcs) in ladders.items():
        n = c["Q"].shape[0]
        prev = R.state_zero(c["x0"], c["l"], c["u"])["stt"]
        for k, S in enumerate(states):
            assert not (k >= 2 and (S["new"] != INACT).sum() > n and (S["new"] != prev).sum() > max(n // 2, 32)), (name, k)
            prev = S["stt"]


# name -> what the seeded mistake is (model_polish), and the checks it may fail: a kept multiplier is also a non-zero on an inactive row
BUGS = {"status": {"status"}, "leave": {"leave", "inactive"}, "rhs": {"rhs"}, "ex": {"ex"}, "correct": {"correct"}, "stored": {"stored"}}


@pytest.mark.parametrize("which", list(BUGS) + ["feasible"])
def test_each_corruption_fails_its_check_alone(ladders, which):
    """One mistake seeded into ONE trial of the model (a flipped row status, a leaving multiplier kept, a leaving term missing from the
    predicted r1, E x of the trial before on the right-hand side, a correction with the other regularisation pair, NV_TMP left from the sweep
    before the accepted one); everything after it is computed consistently from what it left.  The audit names that check, at the state the
    mistake was made in and at no other -- but a multiplier that stays on an inactive row stays there."""
    opt = options()
    c, states, rcs = ladders["band light 0"]
    K = len(states)
    if which == "feasible":      # an accepted state with one row moved beyond ftol
        S = states[-1]
        r = np.nonzero((S["stt"] == INACT) & np.isfinite(c["l"]))[0][0]
        e = c["E"][r] @ S["xt"]
        l = c["l"].copy(); l[r] = e + 10 * opt.feasTol * (1 + abs(e))
        # (a moved bound would enter the replay of every trial: the accepted state alone is held against the moved problem)
        res = R.SparsePolishAudit()
        R.check_accepted(R._Problem(c["Q"], c["E"], c["g"], l, c["u"]), S, opt, res, "S_%d" % K, g=c["g"])
        assert res.failed() == ["feasible"], res.failures
        return
    # the first trial > 0 in which rows leave: the right-hand side is predicted there
    t = next(k for k in range(1, K - 1) if ((states[k - 1]["stt"] != INACT) & (states[k]["stt"] == INACT)).any())
    bug = (which, K - 1 if which == "stored" else t)      # (NV_TMP is stored by the accepting trial)
    bs, brc = [], []
    for k in range(1, K + 3):
        S, rc = model_polish(c["Q"], c["E"], c["g"], c["l"], c["u"], c["x0"], opt, k, True, bug=bug)
        bs.append(S); brc.append(rc)
        if rc == 0:
            break
    res = audit(c, bs, brc, opt)
    got = {f[0] for f in res.failures}
    assert which in got and got <= BUGS[which], res.failures
    at = len(bs) if which == "stored" else t + 1      # the state the mistake shows in
    here = {"S_%d" % at, "S_%d -> S_%d" % (at - 1, at)}
    assert {f[1] for f in res.failures if f[0] == which} <= here, res.failures
    assert {f[1] for f in res.failures if f[0] != "inactive"} <= here, res.failures
