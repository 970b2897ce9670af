"""Sparse arm: the active-set polish (sp_polish_begin, sp_ph_trial, sp_ph_factor, sp_ph_correct in lcqp_sparse_solver.hpp) audited trial by
trial.  States are read back without a launch (lcqp_hip_sparse_read_polish) after runs that were allowed exactly k trials of the first QP,
and every state and every transition is held to tests/sparse_polish_audit_ref.py, a long-double reference on the densified problem that
imports neither the library nor the oracle (its docstring has the checks and their bounds).

A rung is a fresh handle with maxTrials = k, maxRounds = 1, admmFirst = admmHot = 0, maxIterations = 0, perturbStep = 0; a ladder ends at the
first rung whose QP was accepted, or at the length of the model's ladder (tests/test_sparse_polish_audit_ref.py) plus two.  A rung's
return is 0 when its QP was accepted: with maxIterations = 0 the run then ends in sp_ph_qpend with MAX_ITERATIONS_REACHED (or 0), a QP that
gave up ends it with SUBPROBLEM_SOLVER_ERROR.

Cases: the band at G = 8, 16, 32, 64 (LCQP_SPARSE_LANES) and the general LDL' (LCQP_SPARSE_GENERAL) on
sparse_polish_cases.band_instances -- (64, 32, 8) with every row class, rows over three decades, shifted complementarity bounds --; the
band at G = 8 and 32 on sparse_polish_cases.semidefinite_instances, the same with a Hessian that is singular inside its pattern behind a
healthy diagonal (the [[2, 2], [2, 2]] block on variables 22, 23): the host still offers the light pair (lightOK = 1), a VARIABLE's pivot
fails in the first factorisation and sp_ph_factor makes the safe pair permanent (bigReg = 1); the bordered band on the circle example;
behind hot starts (maxIterations = 0 .. 4, perturbStep 0 and 1) the accepted states of the band at G = 8 and of the general engine.  The
overshoot hand-over (trial >= 2 && nact > n && changed > max(n / 2, 32)) is not reachable at these shapes (m = 48 < n = 64 on the band;
tests/test_sparse_polish_audit_ref.py::test_the_overshoot_rule_is_out_of_reach), so it has no case.

Every case prints its worst error / bound per check, its undecidable share, bigReg per state, the prediction-distance record and whether
the bordered band's widening rule fired (`python -m pytest tests/test_gpu_sparse_polish_audit.py -m gpu -s`).

Measured on an MI355X (16 tests, 2.3 s; worst error / bound over the three instances of a case):

    case                    rungs     ex      rhs     correct  stored  levels  bigReg  undecidable   prediction distance | solve share
    lanes 8, 16             6, 5, 5   0.073   0.100   0.183    0.073   0, 1    0       0 of 778      1 .. 1.79  |  8e-5 .. 1.32
    lanes 32, 64            6, 5, 5   0.082   0.091   0.201    0.082   0, 1    0       0 of 778      1 .. 1.79  |  1e-4 .. 0.82
    lanes 8 semidefinite    6, 5, 5   0.065   0.114   0.219    0.065   1       1       0 of 771      0.90 .. 1.87  |  7e-9 .. 0.99
    lanes 32 semidefinite   6, 5, 5   0.071   0.096   0.215    0.071   1       1       0 of 771      0.90 .. 1.87  |  7e-9 .. 0.33
    general LDL'            6, 5, 5   0.080   0.111   0.185    0.080   1       0       0 of 768      1, 9.14, 18.9, 1, 20, 1, 11.1  |  2e-8, 9.13, 0.09, 1e-8, 20, 1e-8, 11.1
    bordered band           3, 3, 3   0.108   0.044   0.209    0.089   1       0       0 of 2709     (no predicted right-hand side)
    accepted states behind hot starts (j = 1 .. 5, perturbStep 0 / 1): stored 0.073 / 0.085 (lanes 8), 0.087 / 0.083 (general LDL');
    the circle's accepted state of a default run: stored 0.089.  e1max: 0.029 of its bound.

Every band ladder has 65 entering rows, 11 leaving rows, 7 predicted right-hand sides, one unchanged trial and one accepted rung per
instance; 10 of its 16 corrections factorise, and all 10 replays of the pivot test are decidable and agree with the recorded level -- the
light pair where every pivot passes, the safe pair where a row's pivot does not (both occur on the band: levels 0, 1), and bigReg stays 0
through those, as the variables' pivots of the replay say it must.  On the semidefinite Hessian the replay of the first factorisation finds
the failing variable pivot in each of the three instances; bigReg is 1 in every state from S_1 on, every correction has dpUsed == delta, and
no later factorisation tries the light pair (`factor` rejects a light pair beside bigReg, and bigReg may change only in a light attempt).
The circle's first QP is feasible at its x0 and, without ADMM iterations in front, settles in three trials with no row entering; its
corrections and those of the general LDL' run with the safe pair and bigReg stays 0 (lightOK = 0: no light attempt).  The bordered band's
block-elimination rule (8 x the float64 block elimination's own ratio, as in tests/test_gpu_sparse_factor.py) did NOT fire: the circle's
0.209 is against the scalar bound.  Behind hot starts 10 (band) and 4 (general LDL') of the QPs j >= 2 kept their set and took two trials
and one sweep; every one of them entered through the reuse branch (SpState.reuse == 1).  No check failed: the audit found nothing to fix
in sp_ph_trial, sp_ph_factor, sp_ph_correct or sp_qp_begin.

The ratios above 0.1, and why the bounds stay:
  correct 0.18 .. 0.22 on every engine: the float64 model of tests/test_sparse_polish_audit_ref.py (LU with refinement, no LDL' at all) has
          0.15 .. 0.19 on the same ladders.  The residual of the recorded step is dominated by the rounding of the update x_{k+1} = x_k + dx
          itself, half an ulp of x_{k+1} through |K|, which the widening term |K| eps (|x_k| + |x_{k+1}|) bounds with a factor of four
          to spare -- not by the factorisation, whose share (tests/test_gpu_sparse_factor.py: 2e-3 on these patterns) is a hundred times smaller.
  rhs     0.10 .. 0.11, ex 0.108 (circle): sums of one to three terms.  A predicted component with one leaving row is ONE rounded product,
          up to half an ulp, against MARGIN gamma_2 = eight half-ulps: 0.125 is attainable, and the rows of the circle have one to three
          entries.
  prediction distance 9 .. 20 on the general LDL' (recorded, not asserted).  Measured beside it ("solve share"): what the correction before
          left on the variables, max_i |rhs - K [dx; dy]|_i in long double, in the same unit dpUsed |dx|_inf.  On the general LDL' the
          three large distances ARE that residual (9.14 | 9.13, 20 | 20, 11.1 | 11.1): the solve's rounding -- inside its bound, `correct`
          0.185 -- is larger than dpUsed |dx| in those trials, so the prediction is off by the solve and not by a missing term.  On the band
          engines the share is 1e-4 .. 1e-2 but for one trial (1.32 | distance 1.29), and the distance is 1 .. 1.9, the last one or two
          steps as the algebra says.
"""
import time

import numpy as np
import pytest

import sparse_polish_audit_ref as R
import sparse_polish_cases as C
import test_sparse_polish_audit_ref as M
from batch_helpers import assert_same_bits, environment, handle, result
from test_gpu_sparse_trace_audit import assert_engine

pytestmark = pytest.mark.gpu

B = 3
ENGINES = {
    "lanes 8": ("band", {}),
    "lanes 16": ("band", {"LCQP_SPARSE_LANES": "16"}),
    "lanes 32": ("band", {"LCQP_SPARSE_LANES": "32"}),
    "lanes 64": ("band", {"LCQP_SPARSE_LANES": "64"}),
    "lanes 8 semidefinite": ("semi", {}),
    "lanes 32 semidefinite": ("semi", {"LCQP_SPARSE_LANES": "32"}),
    "general ldl": ("band", {"LCQP_SPARSE_GENERAL": "1"}),
    "bordered band": ("circle", {}),
}
_MODEL = {}


def instances(kind):
    return dict(band=C.band_instances, semi=C.semidefinite_instances, circle=C.circle_instances)[kind](B)


def rung_limit(hip, kind, ds):
    """the longest model ladder of the case (either regularisation level) plus two"""
    if kind not in _MODEL:
        opt = hip.default_options()
        _MODEL[kind] = 2 + max(len(M.model_ladder(M.dense_case(d), opt, light)[0]) for d in ds[:1 if kind == "circle" else B] for light in (True, False))
    return _MODEL[kind]


def qp_return(hip, st):
    from lcqpow_amd import capi
    assert st["returnValue"] in (0, capi.MAX_ITERATIONS_REACHED, capi.SUBPROBLEM_SOLVER_ERROR), st
    return 1 if st["returnValue"] == capi.SUBPROBLEM_SOLVER_ERROR else 0


def climb(hip, engine, ds, limit):
    """per instance the states and returns of the rungs 1 ... K; the handle's ordering and border"""
    kind, env = ENGINES[engine]
    states, rcs = [[] for _ in ds], [[] for _ in ds]
    meta = None
    for k in range(1, limit + 1):
        with environment(env):
            sb = handle(hip, ds, C.ladder_options(hip.default_options, k))
        assert_engine(sb, " ".join(engine.split()[:2]))
        sb.run()
        sb.synchronize()
        _, _, st = sb.solution()
        meta = (sb.ordering().copy(), sb.border())
        for b in range(len(ds)):
            if rcs[b] and rcs[b][-1] == 0:
                continue
            S = sb.read_polish(b)
            rc = qp_return(hip, st[b])
            assert st[b]["trials"] == (k if rc else S["trial"] + 1) and (rc != 0) == (S["haveSolution"] == 0), (engine, b, k, st[b])
            states[b].append(S); rcs[b].append(rc)
        sb.close()
        if all(r[-1] == 0 for r in rcs):
            break
    return states, rcs, meta


def audit(hip, engine, ds, states, rcs, meta):
    opt = hip.default_options()
    total = R.SparsePolishAudit()
    for b, d in enumerate(ds):
        l, u = C.stacked_bounds(d)
        x0 = d.get("x0")
        R.audit_ladder(d["Q"].toarray(), d["E"].toarray(), d["g"], l, u, states[b], rcs[b], opt, meta[0], x0=x0, kb=meta[1], res=total)
    share = total.undecidable / max(total.decisions, 1)
    print("    %s: rungs %s, outcomes %s\n      events %s, levels %s\n      worst error / bound %s\n      undecidable %d of %d decisions (%.2f %%), open transitions %d of %d\n      prediction distance %s\n      of which the solve before left (max |rhs - K [dx; dy]| over the variables / (dpUsed |dx|)) %s\n      bigReg per state %s, widened bordered corrections %s"
          % (engine, [len(s) for s in states], total.outcomes, total.events, sorted(set(total.levels)), {k: "%.2e" % v for k, v in total.worst.items()},
             total.undecidable, total.decisions, 100 * share, total.open_transitions, total.transitions, ["%.3g" % v for v in total.prediction], ["%.3g" % v for v in total.solve_share],
             [[S["bigReg"] for S in s] for s in states], total.widened))
    total.verify()
    assert total.undecidable <= 0.01 * total.decisions and total.open_transitions <= 0.1 * total.transitions
    return total


@pytest.mark.parametrize("engine", list(ENGINES))
def test_sparse_polish_ladder(hip, engine):
    kind, env = ENGINES[engine]
    t0 = time.perf_counter()
    ds = instances(kind)
    states, rcs, meta = climb(hip, engine, ds, rung_limit(hip, kind, ds))
    t1 = time.perf_counter()
    res = audit(hip, engine, ds, states, rcs, meta)
    print("      climb %.2f s, audit %.2f s" % (t1 - t0, time.perf_counter() - t1))
    ev = res.events
    big = [S["bigReg"] for s in states for S in s]
    if kind == "semi":
        # the Hessian is singular inside its pattern behind a healthy diagonal: the light pair is on offer, a VARIABLE's pivot fails in the
        # first factorisation, and the safe pair is permanent from there on -- no later light attempt (the replay of the pivot test ran
        # once per instance and gave bigReg = 1; `factor` rejects a light pair beside bigReg in every state)
        assert all(S["lightOK"] == 1 for s in states for S in s) and big == [1] * len(big) and ev["bigReg"] == B and set(res.levels) == {1}
        assert all(S["dpUsed"] == S["delta"] and S["d2Used"] == S["delta2"] for s in states for S in s)
        assert ev["accepted"] == B and ev["enter"] > 0
        return
    assert big == [0] * len(big) and ev["bigReg"] == 0
    if kind == "band":
        # entering rows, leaving rows, a trial with an unchanged set, an accepted rung -- in every instance the last
        assert ev["enter"] > 0 and ev["leave"] > 0 and ev["unchanged"] > 0 and ev["predicted"] > 0 and ev["accepted"] == B and all(r[-1] == 0 for r in rcs)
    light = all(S["lightOK"] for s in states for S in s)
    if engine.startswith("lanes"):
        # the synthetic Hessians are safely definite: the handle offers the light pair, and the corrections ran with it
        assert light and 0 in res.levels and any(S["dpUsed"] == S["deltaS"] and S["d2Used"] == S["delta2S"] for s in states for S in s)
    else:
        # the circle's Hessian has 5e-12 on its diagonal beside 17, the general LDL' has no ordering with the rows behind their variables:
        # the safe pair
        assert not light and set(res.levels) == {1} and all(S["dpUsed"] == S["delta"] and S["d2Used"] == S["delta2"] for s in states for S in s)


def test_circle_accepted_state_of_a_default_run(hip):
    """the bordered band's accepted state: a default run (ADMM rounds in front of the polish) with maxIterations = 0"""
    ds = C.circle_instances(B)
    opt = hip.default_options(maxIterations=0, perturbStep=0, printLevel=0)
    sb = handle(hip, ds, opt)
    assert_engine(sb, "bordered band")
    sb.run()
    sb.synchronize()
    _, _, st = sb.solution()
    res = R.SparsePolishAudit()
    for b, d in enumerate(ds):
        assert qp_return(hip, st[b]) == 0, st[b]
        S = sb.read_polish(b)
        l, u = C.stacked_bounds(d)
        R.audit_accepted(d["Q"].toarray(), d["E"].toarray(), l, u, S, opt, res, "circle instance %d" % b)
        assert np.array_equal(S["gk"], d["g"]) and S["dpUsed"] == S["delta"]
    sb.close()
    print("    circle, accepted state: worst error / bound %s" % {k: "%.2e" % v for k, v in res.worst.items()})
    res.verify()


@pytest.mark.parametrize("perturb", [0, 1], ids=["carried", "perturbed"])
@pytest.mark.parametrize("engine", ["lanes 8", "general ldl"])
def test_accepted_states_behind_hot_starts(hip, engine, perturb):
    """maxIterations = j - 1, j = 1 .. 5, at the default maxTrials: the state the j-th QP's accepted trial left.  From the second QP on the
    polish takes its reuse entry (no sweep at trial 0): a QP whose set did not change took two trials and one sweep."""
    kind, env = ENGINES[engine]
    ds = instances(kind)
    res = R.SparsePolishAudit()
    prev, seen_reuse = None, 0
    for j in range(1, 6):
        opt = hip.default_options(maxIterations=j - 1, perturbStep=perturb, printLevel=0)
        with environment(env):
            sb = handle(hip, ds, opt)
        assert_engine(sb, engine)
        sb.run()
        sb.synchronize()
        _, _, st = sb.solution()
        for b, d in enumerate(ds):
            assert qp_return(hip, st[b]) == 0, (engine, j, b, st[b])
            S = sb.read_polish(b)
            l, u = C.stacked_bounds(d)
            R.audit_accepted(d["Q"].toarray(), d["E"].toarray(), l, u, S, opt, res, "%s j = %d instance %d" % (engine, j, b))
            if st[b]["qpSolves"] != j:      # the homotopy ended before its j-th QP
                continue
            assert S["reuse"] == (1 if j >= 2 else 0), (engine, j, b, S["reuse"])
            if j >= 2 and prev[b]["qpSolves"] == j - 1:
                dt, dsw = st[b]["trials"] - prev[b]["trials"], st[b]["reserved"] - prev[b]["reserved"]
                assert dt >= 2 and 1 <= dsw < dt, (engine, j, b, dt, dsw)      # the reuse entry: trial 0 has r1 in place, the accepting trial sweeps
                if dt == 2:
                    assert dsw == 1
                    seen_reuse += 1
        prev = st
        sb.close()
    print("    %s, perturbStep %d, behind hot starts: worst error / bound %s, %d QPs with an unchanged set (two trials, one sweep)"
          % (engine, perturb, {k: "%.2e" % v for k, v in res.worst.items()}, seen_reuse))
    res.verify()
    assert seen_reuse > 0


def test_ladder_is_reproducible(hip):
    """one ladder climbed twice: the same bits in every array and scalar of every state"""
    ds = instances("band")
    limit = rung_limit(hip, "band", ds)
    a, ra, _ = climb(hip, "lanes 8", ds, limit)
    b, rb, _ = climb(hip, "lanes 8", ds, limit)
    assert ra == rb
    for sa, sb_ in zip(a, b):
        for S, T in zip(sa, sb_):
            assert S.keys() == T.keys()
            for k in S:
                assert np.array_equal(S[k], T[k]), k


def test_read_polish_has_no_side_effects(hip):
    """reading twice between a run and a warm re-solve changes no bit of the re-solve"""
    ds = instances("band")
    opt = hip.default_options(perturbStep=0, printLevel=0)
    out = []
    for read in (True, False):
        sb = handle(hip, ds, opt)
        sb.run()
        if read:
            counts = sb.launch_counts()
            first = [sb.read_polish(b) for b in range(B)]
            again = [sb.read_polish(b) for b in range(B)]
            for S, T in zip(first, again):
                assert all(np.array_equal(S[k], T[k]) for k in S)
            assert sb.launch_counts() == counts
        sb.resolve(warm=True)
        out.append(result(sb))
        sb.close()
    assert_same_bits(out[0], out[1])
    assert all(s["returnValue"] == 0 for s in out[0]["st"])


def test_read_polish_before_a_run_is_refused(hip):
    ds = instances("band")
    sb = handle(hip, ds, hip.default_options(printLevel=0))
    with pytest.raises(RuntimeError, match="code 300"):
        sb.read_polish(0)
    sb.run()
    with pytest.raises(RuntimeError, match="code 100"):
        sb.read_polish(B)
    assert sb.read_polish(B - 1)["n"] == ds[0]["nV"]
    sb.close()
