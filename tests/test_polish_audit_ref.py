"""tests/polish_audit_ref.py checked without a device: the audit runs on the states the CPU oracle leaves behind on the same maxTrials ladder the
device tests climb (orc_qp_read_polish returns x, y, the working set and xref also after a solve that gave up), and every check is shown to
fail -- alone -- when the one quantity it holds is corrupted in a recorded state.

The oracle screens nothing and stores no hot-start vectors, so the margin invariant and the stored-state checks have nothing to read there; for
the corruption tests a recorded state is completed with direct float64 evaluations of exactly those quantities (mg = the true slack, qxn = Q x,
...), which the audit then accepts.

Undecidable decisions are capped, not measured: at most 1 % of the row decisions of a case, at most one transition in ten with an open row
decision; the seeds of polish_audit_ref.QP_CASES are chosen so that the oracle's states stay within this (on them: none).  The stage-2 outcome
is reported separately: its a priori bound, gamma_{n + |W| + 4} (|g| + |Q||x| + |E'||y|), exceeds resTol (1 + |g|) from n ~ 100 on, so at the
larger shapes the accept decision is open by construction and only its consequences are held (check_transition)."""
import numpy as np
import pytest

import oracle_py as O
import polish_audit_ref as R

CASES = {c[0]: c for c in R.QP_CASES}


def oracle_ladder(d, hot=None):
    """the states S_1 ... S_K of fresh solves with maxTrials = 1 ... K, K the first that returns 0"""
    states, rcs = [], []
    for k in range(1, R.MAX_LADDER + 1):
        opt = O.default_options(maxRounds=1, admmFirst=0, admmHot=0, maxTrials=k)
        q = O.QP(d["Q"], d["A"], opt)
        ret, it, ef = q.solve(True, d["g"], d["lbA"], d["ubA"], x0=np.zeros(d["n"]), lb=d["lb"], ub=d["ub"])
        S = q.read_polish()
        S["ndep"] = 0
        assert S["mE"] == d["E"].shape[0] and it == k and q.counters()["trials"] == k
        states.append(S); rcs.append(ret)
        if ret == 0:
            return states, rcs, opt
    raise AssertionError("the ladder did not end within %d trials" % R.MAX_LADDER)


@pytest.fixture(scope="module")
def ladders():
    out = {}
    for name, n, m, box, seed, eq, viol in R.QP_CASES:
        d = R.polish_case(n, m, box, seed, eq, viol)
        out[name] = (d,) + oracle_ladder(d)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_states_pass_the_audit(ladders, name):
    d, states, rcs, opt = ladders[name]
    res = R.audit_ladder(d["Q"], d["E"], d["g"], states, rcs, opt, cap_on=not CASES[name][5], extended=d["n"] <= 512)
    print("  %s: %d trials, outcomes %s, open row decisions %d of %d, worst point ratio %.3g" % (name, len(states), res.outcomes, res.undecidable,
                                                                                                res.decisions, max(res.ratios)))
    res.verify()
    assert res.undecidable <= 0.01 * res.decisions and res.open_transitions <= 0.1 * res.transitions
    assert rcs[-1] == 0 and res.outcomes[-1] in ("accept", "undecidable") and len(states) >= 4
    # the ladder passes through trials that enter rows, trials that drop rows and an unchanged trial
    act = [set(np.nonzero(S["stt"])[0]) for S in states]
    assert any(b - a for a, b in zip(act, act[1:])) and any(a - b for a, b in zip(act, act[1:])) and any(a == b for a, b in zip(act, act[1:]))


def test_the_cap_binds_and_is_replayed(ladders):
    """40x96-cap starts from an empty set with more than max(n / 8, 16) rows violated at the unconstrained minimiser: the replay must find the cap
    binding, and with the cap ignored it must disagree with the recorded working set"""
    d, states, rcs, opt = ladders["40x96-cap"]
    rp = R.replay_transition(d["Q"], d["E"], d["g"], states[0], opt, 1, 2, cap_on=True)
    assert rp["capped"] and not rp["open"].any() and np.array_equal(rp["status"], states[1]["stt"])
    e = d["E"] @ states[0]["xt"]
    nviol = int(((e < states[0]["l"] - 1e-9 * (1 + abs(e))) | (e > states[0]["u"] + 1e-9 * (1 + abs(e)))).sum())
    assert nviol > 16 >= 40 // 8 and 16 < rp["nenter"] < nviol
    free = R.replay_transition(d["Q"], d["E"], d["g"], states[0], opt, 1, 2, cap_on=False)
    assert free["nenter"] == nviol and not np.array_equal(free["status"], states[1]["stt"])


def completed(d, S, opt):
    """a recorded oracle state with the device-only quantities evaluated directly in float64"""
    E, x = d["E"], S["xt"]
    e = E @ x
    ftol = opt.feasTol * (1 + np.abs(e))
    act = S["stt"] != 0
    T = dict(S, xs=x.copy(), mg=np.where(act, -1.0, np.minimum(e - (S["l"] - ftol), (S["u"] + ftol) - e)))
    qx, s = d["Q"] @ x, E.T @ S["yt"]
    T.update(qxn=qx, aty=-s, r1s=-d["g"] - qx - s, gs=d["g"].copy(), exs=e)
    return T


CORRUPTIONS = ("status", "point", "screen", "stored")


@pytest.mark.parametrize("which", CORRUPTIONS)
def test_each_corruption_fails_its_check_alone(ladders, which):
    d, states, rcs, opt = ladders["200x330-box"]
    Q, E, g = d["Q"], d["E"], d["g"]
    K = len(states)
    good = completed(d, states[-1], opt)

    def run(S_prev, S_last):
        res = R.PolishAudit()
        R.check_state(E, dict(S_last, accepted=True), opt, res)
        R.check_point(Q, E, g, S_last, res)
        R.check_transition(Q, E, g, S_prev, S_last, 0, opt, K - 1, K, False, res)
        R.check_accepted(Q, E, g, S_last, opt, res)
        return res

    assert run(states[-2], good).failed() == []
    mE = E.shape[0]
    e = E @ good["xt"]
    wide = np.nonzero((good["stt"] == 0) & (good["mg"] > 1.0))[0]
    bad = dict(good)
    if which == "status":
        # one status flipped in the state a transition is replayed FROM and TO alike would hide nothing: flip it in the later state only
        st = good["stt"].copy(); st[wide[0]] = R.LOWER
        bad["stt"] = st
        res = R.PolishAudit()
        R.check_transition(Q, E, g, states[-2], bad, 0, opt, K - 1, K, False, res)
        assert res.failed() == ["status"]
        return
    if which == "point":
        _, _, _, cond = R.kkt_point(Q, E, g, good)
        x = good["xt"].copy(); x[3] += 10 * 1e-12 * d["n"] * cond * max(1.0, np.abs(x).max(), np.abs(good["yt"]).max())
        bad["xt"] = x
        res = R.PolishAudit()
        R.check_point(Q, E, g, bad, res)
        assert res.failed() == ["point"]
        return
    if which == "screen":
        mg = good["mg"].copy(); r = wide[1]
        mg[r] = mg[r] * (1 + 1e-9)        # above the true slack by far more than the rounding of E_r x, far less than any tolerance
        bad["mg"] = mg
        res = R.PolishAudit()
        R.check_state(E, dict(bad, accepted=True), opt, res)
        assert res.failed() == ["screen"]
        assert run(states[-2], bad).failed() == ["screen"]
        return
    qxn = good["qxn"].copy(); qxn[5] += 1e-9 * max(1.0, abs(qxn[5]))
    bad["qxn"] = qxn
    assert run(states[-2], bad).failed() == ["stored"]
