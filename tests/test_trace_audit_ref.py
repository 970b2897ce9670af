"""The trace audit (tests/trace_audit_ref.py) on the CPU oracle's traces: it passes on a correct loop, it bites, and its step-length check
decides most rows.

The problems are the ones tests/test_gpu_trace_audit.py and tests/test_gpu_sparse_trace_audit.py give to the device, every instance of
every case (of the batch of 800 its eight distinct problems).  The sparse oracle records no trace, so the sparse problems go through the
dense oracle in densified form: the same LCQPs, the same homotopy.  A warm re-solve is asked of the oracle in the reference's own terms
(x0, y0 = the last solution, solveZeroPenaltyFirst = 0, initialPenaltyParameter = the last rhoOpt); its g~ is g until the first penalty
update ("after_first_update").

Undecidable rows of the step-length check (rows k >= 1 whose intervals l +- dl, q +- dq do not decide alpha_k): the cap is 40 % per
instance and at least three decided rows.  A warm re-solve after the 2 % change is two rows long (one step-length row), so an instance of a
warm group is its first run and its warm re-solve together, as the device tests audit them.  Observed on the oracle's traces: cold runs 2
to 3 rows of 30 to 49 (4 % to 9 %), the rows at the end of an inner loop where |p| ~ 1e-8 or below; the circle example 7 of 25 and 8 of 27
(28 % and 30 %: its Hessian is singular but for 5e-12 on the diagonal); the single step-length row of a warm re-solve is decided in about
half of the instances.  No problem had to be replaced; the circle's shift of lbL / lbR is a tenth of the synthetic one because the full
one makes it infeasible.

Mutations: a corrupted phi, objective, merit, stationarity norm, step norm (scalars[k][6]) or QP iteration count fails exactly its
quantity at exactly its row.  A moved x_k, alpha_k or rho_k is read by other quantities as well (x_k by everything in rows k and k + 1,
alpha_k by the step norm and the stationarity norm, rho_k by merit, stationarity and the decisions): there the test asserts that the
quantity fails and that nothing fails outside the rows and quantities that read the corrupted value.

The option sets (tests/test_gpu_trace_audit_options.py, tests/test_gpu_sparse_trace_audit_options.py: the problems and options the
device tests run, chosen here): every case passes the audit on the oracle, reaches its branch (TGO.assert_branch on the audit's counters)
and stays under the cap on every instance.  What had to be chosen for the cap, and the two cases of the circle that no input brings under
it (they run for their decisions and are exempt from it), is written where the instances are made (the two files).  The oracle's window
of 64 fills on one problem, the mid-shape instance of the general LDL' engine, and on no other."""
import numpy as np
import pytest

import problems as P
import test_gpu_sparse_trace_audit as TS
import test_gpu_sparse_trace_audit_options as TSO
import test_gpu_trace_audit as TG
import test_gpu_trace_audit_options as TGO
import trace_audit_ref as TA

RES_TOL = 1e-12      # oracle/lcqp_oracle.c, orc_options_default: resTol; qp_polish accepts at max(resTol (1 + |g|_inf), 64 eps scale)
CAP_SHARE, MIN_DECIDED = 0.4, 3

_RUNS = {}


def problem_groups():
    """name -> (list of problem dicts, warm?)"""
    groups = {}
    for name, case in list(TG.CASES.items()) + [("nch16", TG.CASE_1100)]:
        groups["dense " + name] = (lambda name=name, case=case: TG.make_instances(name, case, count=min(case[3], 8)), False)
    for shape in TG.WARM_SHAPES:
        for shifted in (False, True):
            groups["dense warm n%d%s" % (shape[0], " shifted" if shifted else "")] = (lambda shape=shape, shifted=shifted: TG.warm_instances(shape, shifted), True)
    for engine, (shape, _) in TS.ENGINES.items():
        if engine in ("lanes 16", "lanes 32", "lanes 64"):
            continue      # the problems of "lanes 8" on wider lane groups
        for shifted in (False, True):
            count = 1 if shape == "circle" else TS.B      # (the circle instances are copies of one problem)
            groups["sparse %s%s" % (engine, " shifted" if shifted else "")] = (
                lambda shape=shape, shifted=shifted, count=count: [TS.densified(d) for d in TS.sparse_instances(shape, shifted, count)], shape in TS.WARM_SHAPES)
    return groups


GROUPS = problem_groups()
SMALLEST = ["dense nch1 one-hot", "dense nch1 sweep", "dense warm n64", "dense warm n64 shifted", "sparse lanes 8", "sparse lanes 8 shifted"]


def runs(oracle, name):
    """[(d, opt, result, x_start, rho_start, warm, instance)] of a group on the oracle: the cold runs, and for a warm group the warm re-solves behind them
    (computed once, shared, never modified)"""
    if name not in _RUNS:
        make, warm = GROUPS[name]
        out = []
        for b, d in enumerate(make()):
            opt = oracle.default_options(perturbStep=0, printLevel=0)
            ro = P.oracle_solve(oracle, d, opt, trace=400)
            out.append((d, opt, ro, d.get("x0"), opt.initialPenaltyParameter, False, b))
            if warm:
                assert ro["ret"] == 0
                d2 = P.perturbed(d, 300 + b, box_too=False)
                opt2 = oracle.default_options(perturbStep=0, printLevel=0, solveZeroPenaltyFirst=0, initialPenaltyParameter=ro["stats"]["rhoOpt"])
                rw = P.oracle_solve(oracle, dict(d2, x0=ro["x"], y0=ro["y"]), opt2, trace=400)
                out.append((d2, opt2, rw, ro["x"], ro["stats"]["rhoOpt"], True, b))
        _RUNS[name] = out
    return _RUNS[name]


def audit_run(run, check=False, scalars=None, xs=None):
    d, opt, ro, x_start, rho_start, warm = run[:6]
    return TA.audit(d, opt, ro["trace_scalars"] if scalars is None else scalars, ro["trace_x"] if xs is None else xs, x_start, rho_start, warm,
                    "after_first_update", RES_TOL, stats=ro["stats"], x_ret=ro["x"], check=check)


def test_trace_layout(oracle):
    """the eight columns: |stat|inf, phi, rho, alpha, objective, merit, |p|inf, QP iterations"""
    for d, opt, ro, x_start, rho_start, warm, _ in runs(oracle, "dense nch1 sweep")[:2] + runs(oracle, "dense warm n64 shifted")[:1]:
        sc, xs = ro["trace_scalars"], ro["trace_x"]
        assert sc.shape == (ro["stats"]["iterTotal"], 8) and xs.shape == (len(sc), d["nV"])
        x = xs[-1]
        assert ro["ret"] == 0 and 0 <= sc[-1, 0] < opt.stationarityTolerance and sc[-1, 1] < opt.complementarityTolerance
        assert sc[0, 2] == rho_start and np.all(np.diff(sc[:, 2]) >= 0) and sc[-1, 2] == ro["stats"]["rhoOpt"]
        assert sc[0, 3] == 1.0 and np.all((sc[:, 3] > 0) & (sc[:, 3] <= 1))
        Lx, Rx = d["L"] @ x, d["R"] @ x
        assert abs(sc[-1, 1] - (Lx - d["lbL"]) @ (Rx - d["lbR"])) < 1e-12
        assert abs(sc[-1, 4] - (d["g"] @ x + 0.5 * x @ d["Q"] @ x)) < 1e-10
        assert abs(sc[-1, 5] - (sc[-1, 4] + sc[-1, 2] * (Lx @ Rx))) < 1e-10
        assert np.all(sc[:, 6] >= 0) and abs(sc[1, 3] * sc[1, 6] - np.abs(xs[1] - xs[0]).max()) < 1e-14
        assert np.all(sc[:, 7] == np.round(sc[:, 7])) and sc[:, 7].sum() == ro["stats"]["subproblemIter"]


@pytest.mark.parametrize("name", list(GROUPS))
def test_oracle_traces_pass_the_audit_within_the_cap(oracle, name):
    """every quantity of every row, and the share of undecidable step-length rows per instance"""
    per_instance = {}      # a warm group: the cold run and the warm re-solve behind it are one instance's rows (the device tests audit both)
    for i, run in enumerate(runs(oracle, name)):
        r = audit_run(run)
        rows = len(run[2]["trace_scalars"]) - 1
        print(f"    {name} run {i}{' (warm)' if run[5] else ''}: ret {run[2]['ret']} rows {rows + 1} step length decided {r.decided} undecidable {r.undecidable}")
        assert not r.failures, (name, i, r.failures)
        assert run[2]["ret"] == 0
        assert r.decided + r.undecidable == rows
        tot = per_instance.setdefault(run[6], [0, 0, 0])
        tot[0] += rows; tot[1] += r.decided; tot[2] += r.undecidable
    for b, (rows, decided, undecidable) in per_instance.items():
        assert undecidable <= CAP_SHARE * rows and decided >= MIN_DECIDED, (name, b, rows, decided, undecidable)


# ---- the audit must bite --------------------------------------------------------------------------------------------------------------------
COLUMN = dict(stat=0, phi=1, obj=4, merit=5)


def _middle_row(r, sc):
    """a row in the middle of the trace, not next to a penalty update (so that ten bounds on phi or stat move no decision)"""
    rho = sc[:, 2]
    for k in range(len(sc) // 2, len(sc) - 2):
        if rho[k - 1] == rho[k] == rho[k + 1] == rho[k + 2]:
            return k
    assert len(sc) < 8, "no quiet row"
    return 0      # a warm re-solve of a few rows: its first


@pytest.mark.parametrize("name", SMALLEST)
@pytest.mark.parametrize("quantity", ["stat", "phi", "obj", "merit"])
def test_a_corrupted_value_fails_exactly_its_quantity(oracle, name, quantity):
    """one recorded value of one row moved by ten times its bound"""
    for run in runs(oracle, name)[:2]:
        sc = run[2]["trace_scalars"].copy()
        base = audit_run(run)
        k = _middle_row(base, sc)
        sc[k, COLUMN[quantity]] += 10 * base.records[k][quantity][2]
        r = audit_run(run, scalars=sc)
        assert r.failed() == [quantity] and {f[1] for f in r.failures} == {k}, r.failures


@pytest.mark.parametrize("name", SMALLEST)
def test_a_corrupted_step_norm_fails_the_step(oracle, name):
    """scalars[k][6] moved by ten bounds fails `step` alone; one component of one x_k moved by 1e-10 -- the one that carries max|d_k| --
    fails `step` at that row (every other quantity of rows k and k + 1 may notice a moved x_k too; no other row does)"""
    run = runs(oracle, name)[0]
    base = audit_run(run)
    sc = run[2]["trace_scalars"].copy()
    k = _middle_row(base, sc)
    sc[k, 6] += 10 * base.records[k]["step"][2] / sc[k, 3]
    r = audit_run(run, scalars=sc)
    assert r.failed() == ["step"] and {f[1] for f in r.failures} == {k}, r.failures
    xs = run[2]["trace_x"].copy()
    dk = xs[k] - xs[k - 1]
    i = int(np.argmax(np.abs(dk)))
    xs[k, i] += 1e-10 * (1.0 if dk[i] >= 0 else -1.0)
    r = audit_run(run, xs=xs)
    assert ("step", k) in {f[:2] for f in r.failures} and {f[1] for f in r.failures} <= {k, k + 1}, r.failures


@pytest.mark.parametrize("name", SMALLEST)
def test_a_corrupted_step_length_fails_alpha(oracle, name):
    """alpha of a decided row replaced by 0.9 alpha: a full step that is recorded as a shortened one contradicts -l / q along d_k (the step
    norm and the stationarity norm, which read alpha too, may fail with it, at that row only)"""
    run = runs(oracle, name)[0]
    base = audit_run(run)
    sc = run[2]["trace_scalars"].copy()
    k = next(k for k in range(1, len(sc)) if base.records[k]["alpha"][3] == "ok" and sc[k, 3] == 1.0)
    sc[k, 3] *= 0.9
    r = audit_run(run, scalars=sc)
    assert "alpha" in r.failed() and set(r.failed()) <= {"alpha", "step", "stat"} and {f[1] for f in r.failures} == {k}, r.failures


@pytest.mark.parametrize("name", SMALLEST)
def test_a_corrupted_rho_fails_the_rho_sequence(oracle, name):
    """one rho multiplied by f once more (merit, stationarity and the replayed decisions read rho too)"""
    run = runs(oracle, name)[0]
    sc = run[2]["trace_scalars"].copy()
    k = _middle_row(audit_run(run), sc)
    sc[k, 2] *= run[1].penaltyUpdateFactor
    r = audit_run(run, scalars=sc)
    assert "rho" in r.failed() and ("rho", k + 1) in {f[:2] for f in r.failures}, r.failures
    sc = run[2]["trace_scalars"].copy()
    sc[0, 2] *= run[1].penaltyUpdateFactor
    assert ("rho", 0) in {f[:2] for f in audit_run(run, scalars=sc).failures}


@pytest.mark.parametrize("name", SMALLEST)
def test_a_corrupted_iteration_count_fails_the_decisions(oracle, name):
    run = runs(oracle, name)[0]
    sc = run[2]["trace_scalars"].copy()
    sc[len(sc) // 2, 7] += 1
    r = audit_run(run, scalars=sc)
    assert r.failed() == ["decisions"], r.failures


def test_the_replay_follows_the_stated_rules(oracle):
    """decisions: a last row that is not the returned x, a return value that contradicts the last row, a penalty update the recorded phi
    does not allow"""
    run = runs(oracle, "dense nch1 one-hot")[0]
    d, opt, ro, x_start, rho_start, warm = run[:6]
    x = ro["x"].copy(); x[0] = np.nextafter(x[0], 1.0)
    r = TA.audit(d, opt, ro["trace_scalars"], ro["trace_x"], x_start, rho_start, warm, "after_first_update", RES_TOL, stats=ro["stats"], x_ret=x, check=False)
    assert r.failed() == ["decisions"]
    r = TA.audit(d, opt, ro["trace_scalars"], ro["trace_x"], x_start, rho_start, warm, "after_first_update", RES_TOL, stats=dict(ro["stats"], returnValue=200),
                 x_ret=ro["x"], check=False)
    assert r.failed() == ["decisions"]
    sc = ro["trace_scalars"]
    up = np.nonzero(np.diff(sc[:, 2]) > 0)[0]
    assert up.size > 0
    with pytest.raises(TA.AuditError):
        TA.audit(d, opt, sc[:up[0] + 1], ro["trace_x"][:up[0] + 1], x_start, rho_start, warm, "after_first_update", RES_TOL,
                 stats=dict(ro["stats"], iterTotal=int(up[0]) + 1, subproblemIter=int(sc[:up[0] + 1, 7].sum()), rhoOpt=float(sc[up[0], 2]), returnValue=200), x_ret=None)


def test_the_gtil_rule_is_visible_to_the_step_length(oracle):
    """a warm re-solve with non-zero lbL / lbR audited under the other rule for g~ fails `alpha` and nothing else: the rule the audit is
    given is a claim the trace can refute"""
    hit = 0
    for run in runs(oracle, "dense warm n64 shifted"):
        d, opt, ro, x_start, rho_start, warm = run[:6]
        if not warm:
            continue
        r = TA.audit(d, opt, ro["trace_scalars"], ro["trace_x"], x_start, rho_start, warm, "always", RES_TOL, stats=ro["stats"], x_ret=ro["x"], check=False)
        assert set(r.failed()) <= {"alpha"}
        hit += bool(r.failures)
    assert hit > 0


# ---- the option sets of tests/test_gpu_trace_audit_options.py and test_gpu_sparse_trace_audit_options.py, on the oracle ----------------------
OPTION_CASES = [("dense " + shape, oset) for shape, oset in TGO.CASES] + [("sparse " + engine, oset) for engine, oset in TSO.CASES if engine != "lanes 32"]
_OPTION_RUNS = {}


def option_runs(oracle, group, oset):
    """[(d, opt, result, x_start, rho_start, False, instance)] of an option case: the problems the device tests load (the sparse ones
    densified, "lanes 32" being the problems of "lanes 8"), solved once by the dense oracle under the set's options"""
    if (group, oset) not in _OPTION_RUNS:
        arm, name = group.split(" ", 1)
        ds = TGO.option_instances(name, oset) if arm == "dense" else [TSO.densified(d) for d in TSO.option_instances(name, oset)]
        opt = TGO.options(oracle, oset) if arm == "dense" else TSO.options(oracle, name, oset)
        if arm == "sparse" and name == "general ldl" and oset in TSO.LONG_SETS:
            ds = ds[:1]      # (the one the device test audits)
        _OPTION_RUNS[group, oset] = [(d, opt, P.oracle_solve(oracle, d, opt, trace=400), d.get("x0"), opt.initialPenaltyParameter, False, b) for b, d in enumerate(ds)]
    return _OPTION_RUNS[group, oset]


@pytest.mark.parametrize("group,oset", OPTION_CASES, ids=["%s-%s" % c for c in OPTION_CASES])
def test_oracle_traces_pass_the_audit_under_the_options(oracle, group, oset):
    """every quantity of every row under the option set, the branch the set is there for, and the cap of undecidable rows per instance"""
    results, rets = [], []
    for run in option_runs(oracle, group, oset):
        r = audit_run(run)
        rows = len(run[2]["trace_scalars"]) - 1
        print(f"    {group}, {oset}, instance {run[6]}: ret {run[2]['ret']} rows {rows + 1} rho -> {run[2]['stats']['rhoOpt']:g} step length decided {r.decided} "
              f"undecidable {r.undecidable} Leyffer updates {r.leyffer_fired} full-window rows {r.window_shifts} penalty updates {r.updates} double {r.double_updates}")
        assert not r.failures, (group, oset, run[6], r.failures)
        assert r.decided + r.undecidable == rows
        if not (group.startswith("sparse") and (group.split(" ", 1)[1], oset) in TSO.CAP_EXEMPT):      # (the circle cut at 8 rows: TSO.CAP_EXEMPT says why)
            assert r.undecidable <= CAP_SHARE * rows and r.decided >= MIN_DECIDED, (group, oset, run[6], rows, r.decided, r.undecidable)
        results.append(r); rets.append(run[2]["ret"])
    case = (group.split(" ", 1)[1], oset)
    TGO.assert_branch(oset, results, rets, double=group.startswith("sparse") and case in TSO.DOUBLE_UPDATE, fills=group.startswith("sparse") and case in TSO.FILLS_64)


@pytest.mark.parametrize("group", ["dense nch1", "sparse lanes 8"])
@pytest.mark.parametrize("oset", list(TGO.EXPECT_RET))
def test_a_run_that_did_not_converge_returns_the_duals_of_its_last_qp(oracle, group, oset):
    """the check the device tests make on the runs that end with 200 and 201 (TA.last_qp_duals), on the oracle; and it bites: the duals in
    the stationarity of the QP before are outside the bound"""
    for run in option_runs(oracle, group, oset):
        d, opt, ro = run[:3]
        r, bound, r_before = TA.last_qp_duals(d, ro["trace_scalars"], ro["trace_x"], run[3], run[4], ro["y"], "dense", RES_TOL)
        assert r <= bound < r_before, (group, oset, run[6], r, bound, r_before)


def test_the_double_update_is_formed_one_factor_at_a_time(oracle):
    """f = 10 from rho = 0.01: rho f formed in long double is no float64 at all (the comparison the audit used to make refused every
    update of this sequence); the audit forms rho f and (rho f) f in float64 as the loops do, and refuses a rho that is one ulp off"""
    assert TA.LD(0.01) * TA.LD(10.0) != TA.LD(0.01 * 10.0)
    run = next(r for r in option_runs(oracle, "dense nch1", "6 rho 1 factor 10") if r[2]["stats"]["iterOuter"] > 0 and r[2]["trace_scalars"][-1, 2] > 1.0)
    sc = run[2]["trace_scalars"].copy()
    k = int(np.nonzero(np.diff(sc[:, 2]) > 0)[0][0]) + 1
    sc[k:, 2] = np.nextafter(sc[k:, 2], np.inf)
    assert ("rho", k) in {f[:2] for f in audit_run(run, scalars=sc).failures}


def _as_dict(opt, **kw):
    return dict({name: getattr(opt, name) for name, _ in opt._fields_}, **kw)


def test_a_corrupted_rho_after_a_leyffer_update_fails_the_decisions(oracle):
    """window of 1 (set 3).  Inside a trace rho_k is read by merit, stationarity and step length as well, so the rho that only the
    decisions read is the one behind the last row: the trace is cut behind a row whose Leyffer test fired -- the rows, statistics and
    options of the same run under maxIterations = that row, which ends there with 200 and rhoOpt = rho f -- and audits clean; with rhoOpt
    left at the rho before the update, or one factor too far, it fails `decisions` and nothing else"""
    hit = 0
    for run in option_runs(oracle, "dense nch1", "3 window of 1"):
        d, opt, ro, x_start, rho_start, warm = run[:6]
        sc, xs, f = ro["trace_scalars"], ro["trace_x"], opt.penaltyUpdateFactor
        full = audit_run(run)
        assert not full.failures
        for k in range(2, len(sc) - 1):
            cut = lambda **kw: TA.audit(d, _as_dict(opt, maxIterations=k), sc[:k + 1], xs[:k + 1], x_start, rho_start, warm, "after_first_update", RES_TOL,
                                        stats=dict(ro["stats"], iterTotal=k + 1, subproblemIter=int(sc[:k + 1, 7].sum()), returnValue=200,
                                                   iterOuter=int(round(np.log(sc[k + 1, 2] / sc[0, 2]) / np.log(f))), **kw), x_ret=xs[k], check=False)
            r = cut(rhoOpt=float(sc[k + 1, 2]))
            if r.leyffer_fired == 0 or sc[k + 1, 2] != sc[k, 2] * f or TA._cmp_lt(sc[k, 0], opt.stationarityTolerance, full.records[k]["stat"][2]) is not False:
                continue      # rows whose one update is the Leyffer update of row k itself
            assert not r.failures, r.failures
            for wrong in (float(sc[k, 2]), float(sc[k + 1, 2] * f)):
                r = cut(rhoOpt=wrong)
                assert r.failed() == ["decisions"] and {x[1] for x in r.failures} <= {k, None}, r.failures      # (None: iterOuter against the sequence)
            hit += 1
    assert hit > 0


def test_a_corrupted_last_row_of_a_run_that_hit_max_iterations_fails_the_decisions(oracle):
    """set 7, return value 200: the returned x one ulp off the last row; the last row missing from the trace; the last row recorded
    twice.  Each fails `decisions` and nothing else"""
    for run in option_runs(oracle, "dense nch1", "7 maxIterations") + option_runs(oracle, "sparse lanes 8", "7 maxIterations"):
        d, opt, ro, x_start, rho_start, warm = run[:6]
        sc, xs = ro["trace_scalars"], ro["trace_x"]
        assert ro["ret"] == 200 and len(sc) == opt.maxIterations + 1 and not audit_run(run).failures
        go = lambda sc, xs, x: TA.audit(d, opt, sc, xs, x_start, rho_start, warm, "after_first_update", RES_TOL, stats=ro["stats"], x_ret=x, check=False)
        x = ro["x"].copy()
        i = int(np.argmax(np.abs(x)))
        x[i] = np.nextafter(x[i], np.inf)
        r = go(sc, xs, x)
        assert r.failed() == ["decisions"] and {f[1] for f in r.failures} == {len(sc) - 1}, r.failures
        r = go(sc[:-1], xs[:-1], ro["x"])
        assert r.failed() == ["decisions"], r.failures
        r = go(sc[:-1], xs[:-1], xs[-2])      # ... even when the returned x is that row: 200 after maxIterations rows is one row early
        assert r.failed() == ["decisions"], r.failures
