"""The active-set polish of the dense subsolver (qp_polish, lcqpow_amd/csrc/lcqp_dev.hpp) trial by trial: its state is read back without a launch
(lcqp_hip_qp_read_polish / lcqp_hip_batch_read_polish, read_working_set) after solves that were allowed exactly k trials, and every state, every
transition between two consecutive states and every accepted point is held to tests/polish_audit_ref.py -- a long-double reference that sweeps
ALL rows, so a screened row that should have entered, a margin that is too generous, a predicted correction with a wrong term and a stored
hot-start vector that does not belong to the accepted point each fail the trial that made them.  tests/test_polish_audit_ref.py checks that
reference on the CPU oracle's states.

k_qp_solve (the QP object) at np = 128, 256, 384, 1024; k_lcqp_run at shapes with the global row state (mE > 640 at np = 128; np = 384) -- where
the homotopy kernel keeps the row state in LDS (np <= 256 and mE <= 640) yt, ex, mg and stt never reach their global arrays and read_polish
returns None for them."""
import numpy as np
import pytest

import lcqpow_amd as la
import polish_audit_ref as R
import problems as P

pytestmark = pytest.mark.gpu
CASES = {c[0]: c for c in R.QP_CASES}
LADDER = dict(maxRounds=1, admmFirst=0, admmHot=0)


def qp_state(q):
    S = q.read_polish()
    ws = q.read_working_set()
    S.update(slot_row=ws["slot_row"], ns=ws["ns"])
    assert S["nT"] == ws["nT"] and np.array_equal(S["row_slot"], ws["row_slot"])
    return S


def qp_solve_k(d, k, keep=False):
    q = la.SubsolverHIP(d["n"], d["m"], d["Q"], d["A"], la.default_options(maxTrials=k, **LADDER))
    ret, it, ef = q.solve(True, d["g"], d["lbA"], d["ubA"], x0=np.zeros(d["n"]), lb=d["lb"], ub=d["ub"])
    S = qp_state(q)
    cnt = q.counters()
    assert S["mE"] == d["E"].shape[0] and np.array_equal(S["l"][:d["m"]], d["lbA"]) and S["ndep"] == 0
    assert cnt["trials"] == it == k and (ret == 0) == (ef == 0)
    if keep:
        return S, ret, cnt, q
    q.close()
    return S, ret, cnt


def paths(states):
    """what the factor update of each transition had to do, by the kernel's own rule (qp_polish in lcqp_dev.hpp, the `bulk` rule of the factor update)"""
    got = set()
    for a, b in zip(states, states[1:]):
        A, B = a["stt"] != 0, b["stt"] != 0
        nT, ndel, nadd = int(A.sum()), int((A & ~B).sum()), int((~A & B).sum())
        bulk = (nT == 0 and nadd > 0) or (ndel > 0 and ndel >= max(nT // 2, 8)) or nadd >= 16 or 3 * ndel + 7 * nadd >= 96
        got |= {"bulk"} if bulk and (ndel or nadd) else ({"delete"} if ndel else set()) | ({"append"} if nadd else set())
        got |= ({"leave"} if ndel else set()) | ({"enter"} if nadd else set()) | (set() if ndel or nadd else {"same"})
    return got


@pytest.fixture(scope="module")
def qp_ladders():
    out = {}
    for name, n, m, box, seed, eq, viol in R.QP_CASES:
        d = R.polish_case(n, m, box, seed, eq, viol)
        states, rcs, cnts = [], [], []
        for k in range(1, R.MAX_LADDER + 1):
            S, ret, cnt = qp_solve_k(d, k)
            states.append(S); rcs.append(ret); cnts.append(cnt)
            if ret == 0:
                break
        assert rcs[-1] == 0, "the ladder did not end within %d trials" % R.MAX_LADDER
        out[name] = (d, states, rcs, cnts)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_qp_object_ladder(qp_ladders, name):
    d, states, rcs, cnts = qp_ladders[name]
    opt = la.default_options(maxTrials=len(states), **LADDER)
    res = R.audit_ladder(d["Q"], d["E"], d["g"], states, rcs, opt, cap_on=not CASES[name][5], extended=d["n"] <= 512)
    print("  %s (np = %d): %d trials, outcomes %s, open row decisions %d of %d, worst point ratio %.3g, screened share %s"
          % (name, states[0]["np"], len(states), res.outcomes, res.undecidable, res.decisions, max(res.ratios), ["%.2f" % s for s in res.screened]))
    res.verify()
    assert res.undecidable <= 0.01 * res.decisions and res.open_transitions <= 0.1 * res.transitions
    assert states[0]["np"] == {40: 128, 200: 256, 300: 384, 600: 1024}[d["n"]]
    # row classes: equalities (but for the cap case), one-sided, two-sided rows and rows with a single non-zero
    l, u = states[0]["l"], states[0]["u"]
    assert (np.isinf(l) ^ np.isinf(u)).any() and (np.isfinite(l) & np.isfinite(u) & (l < u)).any() and states[0]["nHot"] > 0
    assert (l == u).any() == CASES[name][5]
    # paths: a predicted correction with leaving rows, ti_append, ti_delete, ti_bulk; an unchanged trial; most rows stay screened
    assert paths(states) == {"bulk", "delete", "append", "leave", "enter", "same"}, paths(states)
    assert cnts[-1]["factorizations"] >= 3 and min(res.screened[1:]) > 0.5


def test_qp_object_cap_rule_binds(qp_ladders):
    d, states, rcs, _ = qp_ladders["40x96-cap"]
    opt = la.default_options(maxTrials=2, **LADDER)
    assert not (states[0]["stt"] != 0).any()      # the cold trial corrected on the empty set
    rp = R.replay_transition(d["Q"], d["E"], d["g"], states[0], opt, 1, 2, cap_on=True)
    free = R.replay_transition(d["Q"], d["E"], d["g"], states[0], opt, 1, 2, cap_on=False)
    assert rp["capped"] and free["nenter"] > max(d["n"] // 8, 16) and rp["nenter"] < free["nenter"]
    assert np.array_equal(rp["status"][~rp["open"]], states[1]["stt"][~rp["open"]]) and not np.array_equal(free["status"], states[1]["stt"])


def test_ladder_is_reproducible(qp_ladders):
    d, states, rcs, _ = qp_ladders["200x330-box"]
    for k, S in enumerate(states, start=1):
        T, ret, _ = qp_solve_k(d, k)
        assert ret == rcs[k - 1]
        for key, v in S.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, T[key], equal_nan=True), (k, key)


@pytest.mark.parametrize("name", ["40x96", "600x200-box"])
def test_qp_object_hot_start(qp_ladders, name):
    """the `reuse` entry: the first trial corrects from the stored residual (r1s + (gs - g), exs) without a sweep; the margins are NaN by design
    (lcqp_hip_qp.hip voids them at every hot start), so the first stage 1 reads every inactive row"""
    d, states, rcs, _ = qp_ladders[name]
    K = len(states)
    S0, ret, _, q = qp_solve_k(d, K, keep=True)
    try:
        assert ret == 0
        g2 = d["g"] * (1 + 1e-3 * np.cos(np.arange(d["n"])))
        ret, it, ef = q.solve(False, g2, d["lbA"], d["ubA"], lb=d["lb"], ub=d["ub"])
        S = qp_state(q)
    finally:
        q.close()
    assert ret == 0 and S["ndep"] == 0 and it >= 2
    dense = S["hotc"] < 0
    read = S["work"][4] - S0["work"][4]
    print("  %s hot start: %d trials, rows of E read %d, dense rows %d (inactive at the start %d)" % (name, it, read, dense.sum(), (dense & (S0["stt"] == 0)).sum()))
    assert read >= (dense & (S0["stt"] == 0)).sum()      # trial 0 keeps the set it was handed: trial 1 reads at least these
    if it == 2 and np.array_equal(S["stt"], S0["stt"]):
        assert read == dense.sum()      # stage 1 read every inactive row, stage 2 the active ones
    res = R.PolishAudit()
    opt = la.default_options(maxTrials=K, **LADDER)
    R.check_state(d["E"], dict(S, accepted=True), opt, res, "hot")
    R.check_point(d["Q"], d["E"], g2, S, res, "hot", extended=d["n"] <= 512)
    R.check_accepted(d["Q"], d["E"], g2, S, opt, res, "hot")
    res.verify()
    assert not np.isnan(S["mg"]).any()


def test_read_back_has_no_side_effects(qp_ladders):
    d, states, _, _ = qp_ladders["40x96"]
    K = len(states)
    g2 = d["g"] * 1.01
    outs = []
    for read in (False, True):
        q = la.SubsolverHIP(d["n"], d["m"], d["Q"], d["A"], la.default_options(maxTrials=K, **LADDER))
        q.solve(True, d["g"], d["lbA"], d["ubA"], x0=np.zeros(d["n"]), lb=d["lb"], ub=d["ub"])
        if read:
            q.read_polish(); q.read_polish()
        r = q.solve(False, g2, d["lbA"], d["ubA"], lb=d["lb"], ub=d["ub"])
        outs.append((r, q.getSolution(), q.counters()))
        q.close()
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2]
    assert np.array_equal(outs[0][1][0], outs[1][1][0]) and np.array_equal(outs[0][1][1], outs[1][1][1])


# ---- k_lcqp_run with the global row state -------------------------------------------------------------------------------------------------
RUNGS = 8
RUN_SHAPES = {"np128-mE648": (96, 600, 24), "np384": (300, 100, 20)}
B = 3


def run_case(shape, seed):
    n, nC, nK = RUN_SHAPES[shape]
    ds = []
    for b in range(B):
        rng = np.random.default_rng(1000 * seed + b)
        d = P.random_lcqp(rng, n, nC, nK, box=False, shifted=True)
        xf = rng.uniform(0.2, 1, n); xf[nK:2 * nK] = 0.0      # a feasible point, complementary
        w = np.where(rng.random(nC) < 1.0 / 3.0, rng.uniform(0.05, 0.3, nC), rng.uniform(2.0, 4.0, nC))      # a third tight, the rest wide
        d["lbA"], d["ubA"] = d["A"] @ xf - w, d["A"] @ xf + w * rng.uniform(0.2, 1.0, nC)
        f = 10.0 ** rng.uniform(-1.5, 1.5, nC)      # row norms over three decades, each row scaled with its bounds
        d["A"], d["lbA"], d["ubA"] = d["A"] * f[:, None], d["lbA"] * f, d["ubA"] * f
        d["E"] = R.stacked_rows(d["A"], L=d["L"], R=d["R"])
        ds.append(d)
    return ds


def run_batch(ds, **opts):
    d0 = ds[0]
    bt = la.BatchLCQP(B, d0["nV"], d0["nC"], d0["nComp"], opt=la.default_options(printLevel=0, **opts))
    try:
        for b, d in enumerate(ds):
            assert bt.load(b, 1, d["Q"], d["g"], d["L"], d["R"], **{k: d.get(k) for k in P.KEYS}) == 0
        bt.run()
        x, y, st = bt.solution()
        states = []
        for b in range(B):
            S = bt.read_polish(b)
            ws = bt.read_working_set(b)
            S.update(slot_row=ws["slot_row"], ns=ws["ns"])
            states.append(S)
        return states, st, x, y
    finally:
        bt.close()


@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("shape", list(RUN_SHAPES))
def test_homotopy_ladder(shape, perturb):
    """maxIterations = j - 1 stops the homotopy behind its j-th accepted QP: the stored hot-start state, every row's feasibility and the margins
    that survived j - 1 hot starts inside the kernel"""
    ds = run_case(shape, 7)
    res = R.PolishAudit()
    shares, ratios = [], []
    for j in range(1, 7):
        states, st, _, _ = run_batch(ds, perturbStep=perturb, maxIterations=j - 1)
        for b, (d, S) in enumerate(zip(ds, states)):
            w = "%s j = %d instance %d" % (shape, j, b)
            assert S["rowsInLds"] == 0 and S["yt"] is not None and S["ndep"] == 0 and S["haveSolution"] == 1, w
            assert st[b]["qpSolves"] == j or st[b]["returnValue"] == 0, (w, st[b])
            if j == 1:
                assert np.array_equal(S["gs"], d["g"])      # the zero-penalty QP has the linear term g itself
            g = S["gs"]      # the linear term of QP j >= 2 (rho C x + g~) is held by tests/test_gpu_trace_audit.py
            opt = la.default_options()
            n0 = len(res.screened)
            R.check_state(d["E"], dict(S, accepted=True), opt, res, w)
            R.check_accepted(d["Q"], d["E"], g, S, opt, res, w)
            ratios.append(R.check_point(d["Q"], d["E"], g, S, res, w, extended=True))
            if j >= 2:
                shares += res.screened[n0:]
    print("  %s perturbStep %d: screened share behind hot starts min %.2f mean %.2f, worst point ratio %.3g" % (shape, perturb, min(shares), np.mean(shares), max(ratios)))
    res.verify()
    assert min(shares) > 0.2      # else the margin invariant would test nothing


@pytest.mark.parametrize("shape", list(RUN_SHAPES))
def test_homotopy_first_qp_trial_ladder(shape):
    """the transitions inside k_lcqp_run: the first QP of the homotopy with maxTrials = k"""
    ds = run_case(shape, 7)
    per = [([], []) for _ in range(B)]
    done = [False] * B
    for k in range(1, RUNGS + 1):      # the first QP of these shapes may need ADMM rounds to be accepted: the ladder audits its first RUNGS trials
        states, st, _, _ = run_batch(ds, perturbStep=0, maxIterations=0, maxTrials=k, **LADDER)
        for b in range(B):
            if not done[b]:
                assert states[b]["ndep"] == 0 and st[b]["trials"] == k and states[b]["rowsInLds"] == 0
                solved = st[b]["qpSolverExitFlag"] == 0
                per[b][0].append(states[b]); per[b][1].append(0 if solved else 203)
                done[b] = solved
        if all(done):
            break
    for b, d in enumerate(ds):
        opt = la.default_options(maxTrials=len(per[b][0]), **LADDER)
        cap_on = not (per[b][0][0]["l"] == per[b][0][0]["u"]).any()
        res = R.audit_ladder(d["Q"], d["E"], d["g"], per[b][0], per[b][1], opt, cap_on=cap_on)
        print("  %s instance %d: %d trials, outcomes %s, open row decisions %d of %d, worst point ratio %.3g" % (shape, b, len(per[b][0]), res.outcomes,
                                                                                                     res.undecidable, res.decisions, max(res.ratios)))
        res.verify()
        assert res.undecidable <= 0.01 * res.decisions and res.open_transitions <= 0.1 * res.transitions


def test_lds_row_state_is_withheld():
    """np <= 256 with at most 640 rows: the homotopy kernel's yt, ex, mg, stt live in LDS and are not returned; the rest of the state is audited"""
    n, nC, nK = 64, 96, 16
    d = P.random_lcqp(np.random.default_rng(5), n, nC, nK, box=False, shifted=True)
    bt = la.BatchLCQP(1, n, nC, nK, opt=la.default_options(printLevel=0, perturbStep=0))
    try:
        assert bt.load(0, 1, d["Q"], d["g"], d["L"], d["R"], **{k: d.get(k) for k in P.KEYS}) == 0
        bt.run()
        S = bt.read_polish(0)
        _, _, st = bt.solution()
    finally:
        bt.close()
    assert st[0]["returnValue"] == 0 and S["rowsInLds"] == 1 and all(S[k] is None for k in ("yt", "ex", "mg", "stt"))
    S.update(yt=S["yq"], stt=S["st"])      # the accepted point as qp_solve exported it
    res = R.PolishAudit()
    R.check_accepted(d["Q"], R.stacked_rows(d["A"], L=d["L"], R=d["R"]), S["gs"], S, la.default_options(), res, "LDS shape")
    res.verify()
