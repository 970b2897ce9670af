"""Re-solving a loaded dense batch with new vectors (lcqp_hip_batch_update / lcqp_hip_batch_resolve / lcqp_hip_batch_launch_counts).

Cold re-solves are held to the BITS of a fresh batch object that was given the same data by load and solved by run; warm re-solves to the
CPU oracle asked for the same thing in the reference's own terms -- x0, y0 = its last solution, solveZeroPenaltyFirst = 0,
initialPenaltyParameter = its last rhoOpt -- with the tolerances of tests/test_gpu_parity.py, and to the first-order
conditions of the LCQP itself (tests/problems.py::lcqp_kkt_residuals).  Warm and cold solves may end at different stationary points (the
LCQP is not convex): nothing here compares one with the other."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import problems as P
from batch_helpers import assert_same_bits, load_all, result, stack, update_all
from problems import VEC_KEYS, perturbed, random_lcqp

pytestmark = pytest.mark.gpu

X_TOL, Y_TOL = 1e-9, 1e-7
SHAPES = ((64, 128, 16, 48), (256, 512, 64, 24))      # (n, nC, nComp, instances): the 72 inputs of the warm-start checks


def bt_error():
    import lcqpow_amd
    return lcqpow_amd.capi.last_error()


def fresh(hip, ds, opt, B=None, trace=False):
    """a new batch object, the data by load, solved by run"""
    with_box = ds[0].get("lb") is not None
    bt = hip.BatchLCQP(B or len(ds), ds[0]["nV"], ds[0]["nC"], ds[0]["nComp"], with_box=with_box, opt=opt)
    load_all(bt, ds)
    bt.run()
    out = result(bt, trace)
    assert bt.launch_counts() == (1, 1)
    bt.close()
    return out


# ---- 2: a cold re-solve is a fresh solve, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nC,nComp,B,box,shifted,store",
                         [(40, 20, 8, 5, False, False, True), (40, 20, 8, 5, True, True, False), (200, 330, 37, 3, True, False, False),
                          (256, 512, 64, 3, False, True, False), (300, 100, 40, 2, False, False, False), (600, 200, 50, 2, True, True, False),
                          (40, 20, 8, 800, False, True, False)])      # the last: more than three workgroups per CU -- the other build of the homotopy kernel
def test_cold_resolve_is_a_fresh_solve(hip, n, nC, nComp, B, box, shifted, store):
    rng = np.random.default_rng(n + B)
    opt = hip.default_options(storeSteps=1) if store else hip.default_options()
    base = [random_lcqp(rng, n, nC, nComp, box, shifted) for _ in range(min(B, 6))]
    ds1 = [base[b % len(base)] for b in range(B)]
    ds2 = [perturbed(d, 100 + b) for b, d in enumerate(ds1)]
    if shifted:
        ds2 = [dict(d, lbL=d["lbL"] * 0.5, lbR=d["lbR"] - 0.01) for d in ds2]
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=opt)
    load_all(bt, ds1)
    bt.run()
    first = result(bt, store)
    update_all(bt, ds2)
    bt.resolve()
    again = result(bt, store)
    assert bt.launch_counts() == (1, 2)                         # one setup, two homotopy launches
    setup_ms, solve_ms = bt.last_timing()
    assert setup_ms > 0 and solve_ms > 0
    bt.close()
    ref = fresh(hip, ds2, opt, trace=store)
    assert_same_bits(again, ref)
    assert np.array_equal(again["work"], ref["work"])
    assert not np.array_equal(first["x"], again["x"])         # (the new vectors were solved, not the old ones)


def test_cold_resolve_of_a_generated_batch(hip):
    """a batch filled by generate_synthetic: update + resolve(0) against a fresh object that loads the matrices read back from it"""
    n, nC, nComp, B = 256, 512, 64, 4
    opt = hip.default_options()
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    bt.generate_synthetic(0)
    bt.run()
    ds1 = [dict(bt.read_problem(b), nV=n, nC=nC, nComp=nComp) for b in range(B)]
    ds2 = [perturbed(d, 100 + b) for b, d in enumerate(ds1)]
    update_all(bt, ds2)
    bt.resolve()
    again = result(bt)
    assert bt.launch_counts() == (1, 2)
    bt.close()
    ref = fresh(hip, ds2, opt)
    assert_same_bits(again, ref)
    assert np.array_equal(again["work"], ref["work"])


# ---- 3: partial updates ------------------------------------------------------------------------------------------------------------
def test_partial_update(hip):
    n, nC, nComp, B = 40, 20, 8, 6
    rng = np.random.default_rng(3)
    opt = hip.default_options()
    ds1 = [random_lcqp(rng, n, nC, nComp, False, False) for _ in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    load_all(bt, ds1)
    bt.run()
    first = result(bt)
    ds2 = list(ds1)
    for b in range(1, B, 2):
        ds2[b] = perturbed(ds1[b], 100 + b)
        update_all(bt, [ds2[b]], first=b)
    bt.resolve()
    again = result(bt)
    assert_same_bits(again, first, rows=range(0, B, 2))        # the even instances: the bits of run 1
    assert_same_bits(again, fresh(hip, ds2, opt))              # every instance: a fresh solve of what it now holds
    # two update calls in descending order of `first`, the upper one with lbL / lbR, the lower one without
    ds3 = list(ds2)
    for b in (4, 5):
        ds3[b] = dict(perturbed(ds2[b], 200 + b), lbL=rng.uniform(-0.2, 0.0, nComp), lbR=rng.uniform(-0.2, 0.0, nComp))
    for b in (1, 2):
        ds3[b] = perturbed(ds2[b], 200 + b)
    update_all(bt, ds3[4:6], first=4)
    update_all(bt, ds3[1:3], first=1)
    bt.resolve()
    third = result(bt)
    assert bt.launch_counts() == (1, 3)
    bt.close()
    ref = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    for b, d in enumerate(ds3):                                  # (instance by instance: a load call takes lbL for all of its instances or none)
        load_all_one(ref, b, d)
    ref.run()
    assert_same_bits(third, result(ref))
    ref.close()


def load_all_one(bt, b, d):
    rc = bt.load(b, 1, d["Q"], d["g"], d["L"], d["R"], A=d["A"], **{k: d.get(k) for k in VEC_KEYS})
    assert rc == 0, rc


# ---- 4 - 6: warm re-solves against the oracle ----------------------------------------------------------------------------------------
def _pool():
    return ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0))))


def oracle_cold(oracle, ds):
    opt = oracle.default_options(perturbStep=0, printLevel=0)
    with _pool() as ex:
        return list(ex.map(lambda d: P.oracle_solve(oracle, d, opt), ds))


def oracle_warm(oracle, ds, last, rho=None):
    """the reference's own means of a warm start"""
    def one(k):
        r = last[k]["stats"]["rhoOpt"] if rho is None else rho[k]
        opt = oracle.default_options(perturbStep=0, printLevel=0, solveZeroPenaltyFirst=0, initialPenaltyParameter=r)
        return P.oracle_solve(oracle, dict(ds[k], x0=last[k]["x"], y0=last[k]["y"]), opt)
    with _pool() as ex:
        return list(ex.map(one, range(len(ds))))


def assert_parity(st, x, y, ref, ds):
    """what test_gpu_parity.py asserts for the cold workload, instance by instance, and the first-order conditions of every solution"""
    assert all(r["ret"] == 0 for r in ref)
    for k, r in enumerate(ref):
        print(f"    instance {k}: ret {st[k]['returnValue']} iterates {st[k]['iterTotal']} (oracle {r['stats']['iterTotal']}) "
              f"|dx| {np.abs(x[k] - r['x']).max():.2e} |dy| {np.abs(y[k] - r['y']).max():.2e}")
    assert all(s["returnValue"] == 0 for s in st)
    for k, r in enumerate(ref):
        assert np.abs(x[k] - r["x"]).max() < X_TOL and np.abs(y[k] - r["y"]).max() < Y_TOL, k
        stat, feas, compl, _ = P.lcqp_kkt_residuals(ds[k], x[k], y[k], st[k]["rhoOpt"])
        assert stat < 1e-8 and feas < 1e-8 and compl < 1e-9, (k, stat, feas, compl)
    dit = np.array([s["iterTotal"] for s in st]) - np.array([r["stats"]["iterTotal"] for r in ref])
    assert (dit % 4 == 0).mean() >= 0.99, dit                  # whole inner cycles


def synthetic_batch(hip, n, nC, nComp, B):
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0, printLevel=0))
    bt.generate_synthetic(0)
    ds = [dict(bt.read_problem(b), nV=n, nC=nC, nComp=nComp) for b in range(B)]
    return bt, ds


@pytest.mark.parametrize("n,nC,nComp,B", SHAPES)
def test_warm_resolve_on_unchanged_data_is_one_iterate(hip, oracle, n, nC, nComp, B):
    bt, ds = synthetic_batch(hip, n, nC, nComp, B)
    bt.run()
    x1, y1, st1 = bt.solution()
    assert all(s["returnValue"] == 0 for s in st1)
    bt.resolve(warm=True)
    x2, y2, st2 = bt.solution()
    assert bt.launch_counts() == (1, 2)
    bt.close()
    ref = oracle_warm(oracle, ds, oracle_cold(oracle, ds))
    for k in range(B):
        assert st2[k]["returnValue"] == ref[k]["ret"] == 0
        assert st2[k]["iterTotal"] == ref[k]["stats"]["iterTotal"] == 1, (k, st2[k]["iterTotal"], ref[k]["stats"]["iterTotal"])
        assert np.abs(x2[k] - x1[k]).max() < X_TOL and np.abs(y2[k] - y1[k]).max() < Y_TOL, k


@pytest.mark.parametrize("n,nC,nComp,B", SHAPES)
def test_warm_resolve_against_the_oracle(hip, oracle, n, nC, nComp, B):
    bt, ds = synthetic_batch(hip, n, nC, nComp, B)
    bt.run()
    ds2 = [perturbed(d, 100 + b) for b, d in enumerate(ds)]
    update_all(bt, ds2)
    bt.resolve(warm=True)
    x, y, st = bt.solution()
    bt.close()
    assert_parity(st, x, y, oracle_warm(oracle, ds2, oracle_cold(oracle, ds)), ds2)


@pytest.mark.parametrize("halve_rho", [False, True])
def test_warm_resolve_chain(hip, oracle, halve_rho):
    """five steps, each 2 % of the step before; once with rho0 = half of each instance's last rhoOpt on both sides"""
    n, nC, nComp, B = SHAPES[0]
    bt, ds = synthetic_batch(hip, n, nC, nComp, B)
    bt.run()
    last = oracle_cold(oracle, ds)
    for step in range(1, 6):
        _, _, stp = bt.solution()
        ds = [perturbed(d, 1000 * step + b) for b, d in enumerate(ds)]
        update_all(bt, ds)
        rho_dev = np.array([0.5 * s["rhoOpt"] for s in stp]) if halve_rho else None
        rho_orc = [0.5 * r["stats"]["rhoOpt"] for r in last] if halve_rho else None
        bt.resolve(warm=True, rho0=rho_dev)
        x, y, st = bt.solution()
        last = oracle_warm(oracle, ds, last, rho_orc)
        print(f"  step {step}: iterates mean {np.mean([s['iterTotal'] for s in st]):.2f} max {max(s['iterTotal'] for s in st)}")
        assert_parity(st, x, y, last, ds)
    assert bt.launch_counts() == (1, 6)
    bt.close()


# ---- 7: instances whose last run failed run cold ----------------------------------------------------------------------------------
def test_failed_instances_run_cold(hip):
    n, nC, nComp, B = 64, 128, 16, 8
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(maxIterations=3))
    bt.generate_synthetic(0)
    bt.run()
    _, _, st = bt.solution()
    assert all(s["returnValue"] == hip.capi.MAX_ITERATIONS_REACHED for s in st)
    bt.set_options(hip.default_options())
    bt.resolve(warm=True)
    again = result(bt)
    assert bt.launch_counts() == (2, 2)                         # the options changed: a second full setup
    bt.close()
    ref = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options())
    ref.generate_synthetic(0)
    ref.run()
    assert_same_bits(again, result(ref))
    ref.close()
    # ... and on the setup in place: a warm re-solve after a failed run is the cold one, bit for bit
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(maxIterations=3))
    bt.generate_synthetic(0)
    bt.run()
    bt.resolve(warm=True)
    warm = result(bt)
    bt.resolve(warm=False)
    assert_same_bits(warm, result(bt))
    assert bt.launch_counts() == (1, 3)
    bt.close()


# ---- 8: stored statuses against moved bounds ----------------------------------------------------------------------------------------
def test_statuses_follow_moved_bounds(hip):
    import test_gpu_setup as S
    n, nC, nComp, B = 64, 128, 16, 4
    bt, ds = synthetic_batch(hip, n, nC, nComp, B)
    bt.run()
    x, _, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    ds2, moved = [], []
    for b, d in enumerate(ds):
        ws = bt.read_working_set(b)
        Ax = d["A"] @ x[b]
        act = [r for r in range(nC) if ws["row_slot"][r] >= 0 and min(abs(Ax[r] - d["lbA"][r]), abs(Ax[r] - d["ubA"][r])) < 1e-9]
        assert len(act) >= 2, (b, act)                          # the synthetic instances end with active inequality rows of A
        req, rfree = act[0], act[1]
        lbA, ubA = d["lbA"].copy(), d["ubA"].copy()
        at_lo = abs(Ax[req] - lbA[req]) < 1e-9
        lbA[req] = ubA[req] = lbA[req] if at_lo else ubA[req]    # an active row becomes an equality at its active bound
        if abs(Ax[rfree] - lbA[rfree]) < 1e-9: lbA[rfree] = -np.inf
        else: ubA[rfree] = np.inf                                # the active side of another goes away
        ds2.append(dict(d, lbA=lbA, ubA=ubA)); moved.append((req, rfree))
    update_all(bt, ds2)
    bt.resolve(warm=True)
    x, y, st = bt.solution()
    assert bt.launch_counts() == (1, 2)
    for b, d in enumerate(ds2):
        assert st[b]["returnValue"] == 0, st[b]
        stat, feas, compl, _ = P.lcqp_kkt_residuals(d, x[b], y[b], st[b]["rhoOpt"])
        assert stat < 1e-8 and feas < 1e-8 and compl < 1e-9, (b, stat, feas, compl)
        ws = bt.read_working_set(b)
        req, rfree = moved[b]
        assert ws["row_slot"][rfree] < 0 and ws["row_slot"][req] >= 0
        S.check_working_set(ws, bt.read_setup(b), d["Q"], S.stacked_rows(d))
    bt.close()


# ---- 9, 1: refusals ----------------------------------------------------------------------------------------------------------------
def test_update_refuses_a_changed_box_pattern(hip):
    n, nC, nComp, B = 40, 20, 8, 3
    rng = np.random.default_rng(9)
    opt = hip.default_options()
    ds = [random_lcqp(rng, n, nC, nComp, True, False) for _ in range(B)]
    free = n - 1                                                 # one variable of every instance without a box bound
    for d in ds:
        d["lb"][free] = -np.inf; d["ub"][free] = np.inf
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=True, opt=opt)
    load_all(bt, ds)
    bt.run()
    first = result(bt)
    gains = dict(ds[1], g=ds[1]["g"] + 1.0, ub=np.where(np.arange(n) == free, 5.0, ds[1]["ub"]))
    loses = dict(ds[1], g=ds[1]["g"] + 1.0, lb=np.where(np.arange(n) == 0, -np.inf, ds[1]["lb"]), ub=np.where(np.arange(n) == 0, np.inf, ds[1]["ub"]))
    for bad, word in ((gains, "gains"), (loses, "loses")):
        rc = bt.update(0, 2, stack([ds[0], bad], "g"), **{k: stack([ds[0], bad], k) for k in VEC_KEYS})
        assert rc == 100 and word in bt_error() and "instance 1" in bt_error()      # LCQP_INVALID_ARGUMENT
    assert bt.update(1, 1, ds[1]["g"], lbA=ds[1]["lbA"], ubA=ds[1]["ubA"]) == 100       # lb / ub absent: every bound would go
    assert bt.update(1, 1, None, lb=ds[1]["lb"], ub=ds[1]["ub"]) == 116                 # g is required (INVALID_OBJECTIVE_LINEAR_TERM)
    assert bt.update(1, 1, ds[1]["g"], lb=ds[1]["lb"], ub=ds[1]["ub"], lbL=np.full(nComp, -np.inf)) == 120
    bt.resolve()
    assert_same_bits(result(bt), first)                          # nothing was written by the refused calls
    assert bt.launch_counts() == (1, 2)
    bt.close()


def test_argument_checks_precede_every_device_call(hip):
    L = hip.lib()
    n, nC, nComp, B = 12, 5, 3, 2
    bt = hip.BatchLCQP(B, n, nC, nComp)
    g = np.zeros(B * n); gp = g.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.lcqp_hip_batch_update(bt.h, 0, 1, gp, *[None] * 10) == 300            # nothing loaded yet: LCQP_LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_batch_resolve(bt.h, 0, None) == 300
    rng = np.random.default_rng(1)
    load_all(bt, [random_lcqp(rng, n, nC, nComp, False, False) for _ in range(B)])
    for first, count in ((-1, 1), (0, 0), (1, 2), (2, 1), (0, 2 ** 31 - 1)):
        assert L.lcqp_hip_batch_update(bt.h, first, count, gp, *[None] * 10) == 100
    with pytest.raises(ValueError):
        bt.update(1, 2, g)
    with pytest.raises(ValueError):
        bt.update(0, 1, np.zeros(n + 1))
    with pytest.raises(ValueError):
        bt.resolve(warm=True, rho0=np.ones(B + 1))
    for bad in ([1.0, 0.0], [-1.0, 1.0], [np.nan, 1.0], [np.inf, 1.0]):
        with pytest.raises(RuntimeError, match="rho0"):
            bt.resolve(warm=True, rho0=bad)
    assert L.lcqp_hip_batch_resolve(bt.h, 2, None) == 100
    assert bt.launch_counts() == (0, 0)                          # none of the refused calls launched anything
    bt.resolve(warm=True)                                        # no setup in place: this is run()
    assert bt.launch_counts() == (1, 1)
    _, _, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    bt.close()
