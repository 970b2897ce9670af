"""Re-solving a loaded sparse batch with new vectors (lcqp_hip_sparse_update / lcqp_hip_sparse_resolve / lcqp_hip_sparse_launch_counts).

Cold re-solves are held to the BITS of a fresh handle that was given the same data by load and solved by run; warm re-solves to the
sparse CPU oracle asked for the same thing in the reference's own terms -- x0, y0 = its last solution, solveZeroPenaltyFirst = 0,
initialPenaltyParameter = its last rhoOpt -- with the tolerances tests/test_gpu_sparse.py uses for oracle runs started from a given
x0, y0 (1e-8 / 1e-6), and to the first-order conditions of the LCQP itself.  Warm and cold solves may end at different stationary points
(the LCQP is not convex): nothing here compares one with the other."""
import ctypes

import numpy as np
import pytest

import problems as P
from batch_helpers import assert_same_bits, handle, result, stack, update_all
from problems import MID, OPT, SMALL, circle_instances, instances, moved

pytestmark = pytest.mark.gpu

X_TOL, Y_TOL = 1e-8, 1e-6


def fresh(hip, ds, opt, trace=False):
    """a new handle, the data by load, solved by run"""
    sb = handle(hip, ds, opt)
    sb.run()
    out = result(sb, trace)
    assert sb.launch_counts() == (1, 1)
    sb.close()
    return out


# ---- the oracle, asked once per input ----------------------------------------------------------------------------------------------------
_COLD = {}


def oracle_solve(oracle, d, **kw):
    opt = oracle.default_options(perturbStep=0, **{k: kw.pop(k) for k in ("solveZeroPenaltyFirst", "initialPenaltyParameter") if k in kw})
    return oracle.sparse_lcqp_solve(d["nV"], d["nC"], d["nComp"], d["Q"].tocsr(), d["g"], d["E"].tocsr(), lbA=d["lbA"], ubA=d["ubA"], opt=opt, **kw)


def oracle_cold(oracle, shape, B):
    """the oracle's cold solves of instances 0 .. B-1 of the synthetic workload (shared by the tests of this file, never modified)"""
    for b in range(B):
        if (shape, b) not in _COLD:
            _COLD[(shape, b)] = oracle_solve(oracle, P.sparse_instance(b, *shape))
    return [_COLD[(shape, b)] for b in range(B)]


def oracle_warm(oracle, ds, last, rho=None):
    """the reference's own means of a warm start"""
    return [oracle_solve(oracle, d, x0=last[k]["x"], y0=last[k]["y"], solveZeroPenaltyFirst=0,
                         initialPenaltyParameter=last[k]["stats"]["rhoOpt"] if rho is None else rho[k]) for k, d in enumerate(ds)]


def assert_warm_parity(st, x, y, ref, cold_iters):
    for k, r in enumerate(ref):
        print(f"    instance {k}: ret {st[k]['returnValue']} iterates {st[k]['iterTotal']} (oracle {r['stats']['iterTotal']}, cold {cold_iters[k]}) "
              f"|dx| {np.abs(x[k] - r['x']).max():.2e} |dy| {np.abs(y[k] - r['y']).max():.2e}")
    for k, r in enumerate(ref):
        assert st[k]["returnValue"] == r["ret"] == 0, (k, st[k], r["stats"])
        assert np.abs(x[k] - r["x"]).max() < X_TOL and np.abs(y[k] - r["y"]).max() < Y_TOL, k
        assert abs(st[k]["iterTotal"] - r["stats"]["iterTotal"]) <= 4, (k, st[k]["iterTotal"], r["stats"]["iterTotal"])     # one inner cycle
        assert st[k]["iterTotal"] < cold_iters[k], (k, st[k]["iterTotal"], cold_iters[k])


# ---- 1: a cold re-solve is a fresh solve, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small, traced", "mid", "pools of 4", "lanes 32", "general ldl", "bordered circle", "lbL and lbR appear"])
def test_cold_resolve_is_a_fresh_solve(hip, monkeypatch, case):
    store = case == "small, traced"
    opt = hip.default_options(storeSteps=1 if store else 0, **OPT)
    if case == "pools of 4":
        monkeypatch.setenv("LCQP_SPARSE_POOL", "4")
    if case == "lanes 32":
        monkeypatch.setenv("LCQP_SPARSE_LANES", "32")
    if case == "general ldl":
        monkeypatch.setenv("LCQP_SPARSE_GENERAL", "1")
    if case == "bordered circle":
        ds1 = circle_instances(3)
        ds2 = [dict(d, g=d["g"] * (1.0 + 0.02 * np.random.default_rng(100 + b).standard_normal(d["nV"]))) for b, d in enumerate(ds1)]      # g moved only
    else:
        shape, B = {"small, traced": (SMALL, 6), "mid": (MID, 4), "pools of 4": (SMALL, 21), "lanes 32": (SMALL, 6), "general ldl": (MID, 3),
                    "lbL and lbR appear": (SMALL, 6)}[case]
        ds1 = instances(shape, B)
        ds2 = [moved(d, 100 + b) for b, d in enumerate(ds1)]
        if case == "lbL and lbR appear":
            nK = shape[2]
            ds2 = [dict(d, lbL=np.full(nK, 0.01), lbR=np.full(nK, 0.02), ubL=np.full(nK, 5.0)) for d in ds2]
    sb = handle(hip, ds1, opt)
    if case == "lanes 32": assert sb.lanes() == 32
    if case == "general ldl": assert sb.fronts() > 0
    if case == "bordered circle": assert sb.border() == 3
    if case in ("small, traced", "pools of 4", "lbL and lbR appear"): assert sb.lanes() == 8
    sb.run()
    first = result(sb, store)
    update_all(sb, ds2)
    sb.resolve()
    again = result(sb, store)
    assert sb.launch_counts() == (1, 2)                         # one setup, two homotopy launches
    setup_ms, solve_ms = sb.last_timing()
    assert setup_ms > 0 and solve_ms > 0
    sb.close()
    assert_same_bits(again, fresh(hip, ds2, opt, trace=store))
    assert not np.array_equal(first["x"], again["x"])           # (the new vectors were solved, not the old ones)


# ---- 2: rows that change their class: the ADMM KKT factor is rebuilt -----------------------------------------------------------------------
def test_changed_row_classes_rebuild_the_admm_factor(hip):
    """admmFirst = 50: every homotopy starts with fifty ADMM iterations on the factor that contains 1 / rhov, so that factor decides the
    bits.  One row of A of every instance becomes free, another an equality at the last solution; then back; then only two instances of
    the six (one wavefront: their lane groups rebuild, the others' do not)."""
    shape, B = SMALL, 6
    opt = hip.default_options(admmFirst=50, **OPT)
    ds1 = instances(shape, B)
    sb = handle(hip, ds1, opt)
    sb.run()
    first = result(sb)
    assert all(s["admmIter"] >= 50 for s in first["st"])

    def reclassed(d, x):
        lbA, ubA = d["lbA"].copy(), d["ubA"].copy()
        lbA[0], ubA[0] = -np.inf, np.inf
        lbA[1] = ubA[1] = (d["E"].tocsr()[:d["nC"]] @ x)[1]
        return dict(d, lbA=lbA, ubA=ubA)
    ds2 = [reclassed(d, first["x"][b]) for b, d in enumerate(ds1)]
    update_all(sb, ds2)
    sb.resolve()
    second = result(sb)
    assert all(s["admmIter"] >= 50 for s in second["st"])
    assert_same_bits(second, fresh(hip, ds2, opt))
    update_all(sb, ds1)
    sb.resolve()
    assert_same_bits(result(sb), first)                         # the factor of the original classes is back
    ds3 = [ds2[b] if b in (1, 4) else ds1[b] for b in range(B)]
    for b in (1, 4):
        update_all(sb, [ds3[b]], first=b)
    sb.resolve()
    third = result(sb)
    assert sb.launch_counts() == (1, 4)
    sb.close()
    assert_same_bits(third, fresh(hip, ds3, opt))


# ---- 3: partial updates ----------------------------------------------------------------------------------------------------------------------
def test_partial_update(hip):
    shape, B = SMALL, 6                                          # G = 8: all six instances share one wavefront
    opt = hip.default_options(**OPT)
    ds1 = instances(shape, B)
    sb = handle(hip, ds1, opt)
    assert sb.lanes() == 8
    sb.run()
    first = result(sb)
    ds2 = list(ds1)
    for b in range(1, B, 2):
        ds2[b] = moved(ds1[b], 100 + b)
        update_all(sb, [ds2[b]], first=b)
    sb.resolve()
    again = result(sb)
    assert sb.launch_counts() == (1, 2)
    sb.close()
    assert_same_bits(again, first, rows=range(0, B, 2))        # the even instances: the bits of run 1
    assert_same_bits(again, fresh(hip, ds2, opt))              # every instance: a fresh solve of what it now holds
    assert not any(np.array_equal(again["x"][b], first["x"][b]) for b in range(1, B, 2))


# ---- 4: warm on unchanged data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", [(SMALL, 12), (MID, 6)])
def test_warm_resolve_on_unchanged_data_is_one_iterate(hip, oracle, shape, B):
    ds = instances(shape, B)
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    x1, y1, st1 = sb.solution()
    assert all(s["returnValue"] == 0 for s in st1)
    sb.resolve(warm=True)
    x2, y2, st2 = sb.solution()
    assert sb.launch_counts() == (1, 2)
    sb.close()
    ref = oracle_warm(oracle, ds, oracle_cold(oracle, shape, B))
    for k in range(B):
        assert st2[k]["returnValue"] == ref[k]["ret"] == 0
        assert st2[k]["iterTotal"] == ref[k]["stats"]["iterTotal"] == 1, (k, st2[k]["iterTotal"], ref[k]["stats"]["iterTotal"])
        assert np.abs(x2[k] - x1[k]).max() < X_TOL and np.abs(y2[k] - y1[k]).max() < Y_TOL, k


def test_warm_resolve_on_unchanged_data_bordered_band(hip):
    """the bordered pattern of test_sparse_bordered_band_circle: the polish factor that is kept carries its border (W, the Schur complement);
    held to the handle's own previous solution"""
    ds = circle_instances(3)
    sb = handle(hip, ds, hip.default_options(**OPT))
    assert sb.border() == 3
    sb.run()
    x1, y1, st1 = sb.solution()
    assert all(s["returnValue"] == 0 for s in st1)
    sb.resolve(warm=True)
    x2, y2, st2 = sb.solution()
    sb.close()
    for k in range(3):
        assert st2[k]["returnValue"] == 0 and st2[k]["iterTotal"] == 1, st2[k]
        assert np.abs(x2[k] - x1[k]).max() < X_TOL and np.abs(y2[k] - y1[k]).max() < Y_TOL, k


# ---- 5: warm against the oracle after a 2 % move ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B,general", [(SMALL, 12, False), (MID, 6, False), (MID, 6, True)])
def test_warm_resolve_against_the_oracle(hip, oracle, monkeypatch, shape, B, general):
    if general:
        monkeypatch.setenv("LCQP_SPARSE_GENERAL", "1")
    ds = instances(shape, B)
    sb = handle(hip, ds, hip.default_options(**OPT))
    assert (sb.fronts() > 0) == general
    sb.run()
    _, _, st1 = sb.solution()
    ds2 = [moved(d, 1000 + b) for b, d in enumerate(ds)]
    update_all(sb, ds2)
    sb.resolve(warm=True)
    x, y, st = sb.solution()
    assert sb.launch_counts() == (1, 2)
    sb.close()
    assert_warm_parity(st, x, y, oracle_warm(oracle, ds2, oracle_cold(oracle, shape, B)), [s["iterTotal"] for s in st1])


# ---- 6: a chain of warm re-solves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halve_rho", [False, True])
def test_warm_resolve_chain(hip, oracle, halve_rho):
    """three steps, each 2 % of the step before; once with rho0 = half of each instance's last rhoOpt on both sides"""
    shape, B = SMALL, 12
    ds = instances(shape, B)
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    _, _, st1 = sb.solution()
    cold_iters = [s["iterTotal"] for s in st1]
    last = oracle_cold(oracle, shape, B)
    for step in range(1, 4):
        _, _, stp = sb.solution()
        ds = [moved(d, 1000 * step + b) for b, d in enumerate(ds)]
        update_all(sb, ds)
        rho_dev = np.array([0.5 * s["rhoOpt"] for s in stp]) if halve_rho else None
        rho_orc = [0.5 * r["stats"]["rhoOpt"] for r in last] if halve_rho else None
        sb.resolve(warm=True, rho0=rho_dev)
        x, y, st = sb.solution()
        last = oracle_warm(oracle, ds, last, rho_orc)
        print(f"  step {step}: iterates mean {np.mean([s['iterTotal'] for s in st]):.2f} max {max(s['iterTotal'] for s in st)}")
        assert_warm_parity(st, x, y, last, cold_iters)
    assert sb.launch_counts() == (1, 4)
    sb.close()


# ---- 7: stored statuses against moved bounds -----------------------------------------------------------------------------------------------------
def test_statuses_follow_moved_bounds(hip):
    shape, B = MID, 4
    n, nC, nK = shape
    ds = instances(shape, B)
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    x, _, st = sb.solution()
    assert all(s["returnValue"] == 0 for s in st)
    ds2, picked = [], []
    for b, d in enumerate(ds):
        Ax = d["E"].tocsr()[:nC] @ x[b]
        act = [r for r in range(nC) if min(abs(Ax[r] - d["lbA"][r]), abs(Ax[r] - d["ubA"][r])) < 1e-9]
        assert len(act) >= 2, (b, act)                          # the synthetic instances end with active rows of A
        req, rfree = act[0], act[1]
        lbA, ubA = d["lbA"].copy(), d["ubA"].copy()
        at_lo = abs(Ax[req] - lbA[req]) < 1e-9
        lbA[req] = ubA[req] = lbA[req] if at_lo else ubA[req]    # an active row becomes an equality at its active bound
        if abs(Ax[rfree] - lbA[rfree]) < 1e-9: lbA[rfree] = -np.inf
        else: ubA[rfree] = np.inf                                # the active side of another goes away
        ds2.append(dict(d, lbA=lbA, ubA=ubA)); picked.append((req, rfree))
    update_all(sb, ds2)
    sb.resolve(warm=True)
    x, y, st = sb.solution()
    assert sb.launch_counts() == (1, 2)
    sb.close()
    for b, d in enumerate(ds2):
        assert st[b]["returnValue"] == 0, st[b]
        req, rfree = picked[b]
        Qc, Ec = d["Q"].tocsr(), d["E"].tocsr()
        Ex = Ec @ x[b]
        assert y[b][rfree] == 0.0                                # the freed row left with a zero multiplier and stayed out
        assert abs(Ex[req] - d["lbA"][req]) < 1e-9
        lo = np.concatenate([d["lbA"], np.zeros(2 * nK)]); hi = np.concatenate([d["ubA"], np.full(2 * nK, np.inf)])
        stat = np.abs(Qc @ x[b] + d["g"] - Ec.T @ y[b]).max()    # the arm's dual sign (tests/test_gpu_sparse.py::test_sparse_hip_batch_properties)
        feas = max(np.maximum(lo - Ex, Ex - hi).max(), 0.0)
        compl = abs(float(Ex[nC:nC + nK] @ Ex[nC + nK:]))
        print(f"    instance {b}: iterates {st[b]['iterTotal']} stationarity {stat:.2e} infeasibility {feas:.2e} complementarity {compl:.2e}")
        assert stat < 1e-8 and feas < 1e-8 and compl < 1e-9, (b, stat, feas, compl)


# ---- 8: instances whose last run failed run cold ------------------------------------------------------------------------------------------------
def test_failed_instances_run_cold(hip):
    shape, B = SMALL, 6
    ds = instances(shape, B)
    sb = handle(hip, ds, hip.default_options(maxIterations=3, **OPT))
    sb.run()
    _, _, st = sb.solution()
    assert all(s["returnValue"] == hip.capi.MAX_ITERATIONS_REACHED for s in st)
    sb.resolve(warm=True)
    warm = result(sb)
    sb.resolve(warm=False)
    assert_same_bits(warm, result(sb))                          # on the setup in place: warm after a failed run is the cold one
    assert sb.launch_counts() == (1, 3)
    opt = hip.default_options(**OPT)
    sb.set_options(opt)
    sb.resolve(warm=True)                                       # the options changed: a full run
    again = result(sb)
    assert sb.launch_counts()[0] == 2
    sb.close()
    assert all(s["returnValue"] == 0 for s in again["st"])
    assert_same_bits(again, fresh(hip, ds, opt))


# ---- 9: refusals launch nothing ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip):
    L = hip.lib()
    shape, B = SMALL, 3
    n, nC, nK = shape
    ds = instances(shape, B)
    d = ds[0]
    sb = hip.SparseBatchLCQP(B, n, nC, nK, d["Q"], d["E"], opt=hip.default_options(**OPT))
    g = np.zeros(B * n); gp = g.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.lcqp_hip_sparse_update(sb.h, 0, 1, gp, *[None] * 8) == 300             # nothing loaded yet: LCQP_LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_resolve(sb.h, 0, None) == 300
    assert sb.load(0, B, np.stack([q["Q"].data for q in ds]), stack(ds, "g"), np.stack([q["E"].data for q in ds]), lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")) == 0
    sb.run()
    first = result(sb)
    assert sb.launch_counts() == (1, 1)
    for first_, count in ((-1, 1), (0, 0), (B - 1, 2), (B, 1), (0, 2 ** 31 - 1)):
        assert L.lcqp_hip_sparse_update(sb.h, first_, count, gp, *[None] * 8) == 100
    assert sb.update(1, 1, None, lbA=ds[1]["lbA"], ubA=ds[1]["ubA"]) == 116            # g is required (INVALID_OBJECTIVE_LINEAR_TERM)
    assert sb.update(0, 2, stack(ds[:2], "g") + 1.0, lbL=np.stack([np.zeros(nK), np.full(nK, -np.inf)])) == 120      # the whole range is checked first
    assert sb.update(1, 1, ds[1]["g"] + 1.0, lbR=np.full(nK, -np.inf)) == 120
    assert L.lcqp_hip_sparse_resolve(sb.h, 2, None) == 100 and L.lcqp_hip_sparse_resolve(sb.h, -1, None) == 100
    for bad in ([1.0, 0.0, 1.0], [-1.0, 1.0, 1.0], [1.0, 1.0, np.nan], [np.inf, 1.0, 1.0]):
        with pytest.raises(RuntimeError, match="rho0"):
            sb.resolve(warm=True, rho0=bad)
    with pytest.raises(ValueError):
        sb.update(0, 1, np.zeros(n + 1))
    with pytest.raises(ValueError):
        sb.update(0, 2, np.zeros(n))
    with pytest.raises(ValueError):
        sb.resolve(warm=True, rho0=np.ones(B + 1))
    assert sb.launch_counts() == (1, 1)                          # none of the refused calls launched anything
    sb.resolve()
    assert_same_bits(result(sb), first)                          # ... or wrote anything
    assert sb.launch_counts() == (1, 2)
    sb.close()
