"""Dense arm: the trace audit of tests/test_gpu_trace_audit.py under every option that changes the control flow of lcqp_run (lcqp_dev.hpp).

test_gpu_trace_audit.py holds the loop to the direct long-double reference (tests/trace_audit_ref.py) under the default options only.  Here
the same audit, with the same bounds, runs under the option sets of test_lcqp_option_sweep: the first QP with the penalty in it and a given
x0 / y0, Leyffer windows of 0, 1, 12 and 64 (the capacity of hist[]), another penalty sequence, the two failing exits, loosened tolerances,
and perturbStep together with two of these.  Each case asserts through the audit's counters that it reached the branch it is there for
(assert_branch; tests/test_trace_audit_ref.py asserts the same on the CPU oracle and holds the oracle to the cap of undecidable rows).

Shapes: the smallest at which the fused pass differs -- (40, 20, 8) NCH = 1 with one-hot pairs, (200, 330, 37) with a box: NCH = 2 and the
row state in LDS, and for the sets 1, 3 and 10 the dense pairs at (300, 100, 40): NCH = 3, cNnz = -1, C x0 from the dense sweep.

Measured on an MI355X: every case 0.1 s to 0.75 s (load, run and the long-double audit), the file 8 s.  Worst |recorded - reference| / bound
over all cases: objective 0.003, phi 0.006, merit 0.003, step norm 0.11 (the two sets with perturbStep; 0.024 without), stationarity 0.33
(set 6 at (40, 20, 8); 0.31 under set 1, 0.21 to 0.23 under the others) -- all inside the 0.46 of the default-option audit.  The returned
duals of the runs that end with 200 / 201 sit at 2e-4 of their bound in the last QP's stationarity and at 760 bounds or more in the one of
the QP before.  Branch counters per case (Leyffer updates / rows that found the window full / penalty updates / double updates, summed
over the instances), (40, 20, 8) then (200, 330, 37): default 28/49/29/1 and 14/27/16/2; set 1 27/42/28/1 and 14/28/16/2; set 2 0/0/28/0
and 0/0/16/0; set 3 31/43/31/0 and 20/25/20/0; set 4 7/25/28/1 and 4/11/16/0; set 5 0/0/28/0 and 0/0/16/0 (the window of 64 never fills
on this arm's problems, asserted: no inner loop is that long); set 6 2/18/2/0 on both; set 7 8/8/9/1 and 4/4/6/2; set 8 11/11/12/1 and 4/4/6/2;
set 9 13/34/29/4 and 8/21/16/2; the dense pairs: set 1 16/32/20/4, set 3 20/27/20/0, set 10 18/34/20/2 and 20/27/20/0.
"""
import ctypes
import time

import numpy as np
import pytest

import test_gpu_trace_audit as TG
import trace_audit_ref as TA
from batch_helpers import load_all

pytestmark = pytest.mark.gpu

RES_TOL = TG.RES_TOL
LCQP_HIP_UNSUPPORTED = 901      # include/lcqp_hip.h
REFUSAL = "nDynamicPenalty > 64 unsupported"      # lcqp_host_rt.hpp, set_options: the text both arms answer with, each through its own last_error

# the dense option sets of test_lcqp_option_sweep, numbered as in DESIGN.md section 2 ("0" is the default set: its branch assertion is the Leyffer update)
OPTION_SETS = {
    "0 default": dict(),
    "1 penalty in the first QP": dict(solveZeroPenaltyFirst=0),
    "2 no window": dict(nDynamicPenalty=0),
    "3 window of 1": dict(nDynamicPenalty=1, etaDynamicPenalty=0.5),
    "4 window of 12": dict(nDynamicPenalty=12, etaDynamicPenalty=0.95),
    "5 window of 64": dict(nDynamicPenalty=64),
    "6 rho 1 factor 10": dict(initialPenaltyParameter=1.0, penaltyUpdateFactor=10.0),
    "7 maxIterations": dict(maxIterations=7),
    "8 maxPenaltyParameter": dict(maxPenaltyParameter=0.05),
    "9 loose tolerances": dict(stationarityTolerance=1e-6, complementarityTolerance=1e-9),
    "10 perturbed, penalty in the first QP": dict(perturbStep=1, solveZeroPenaltyFirst=0),
    "10 perturbed, window of 1": dict(perturbStep=1, nDynamicPenalty=1, etaDynamicPenalty=0.5),
}
GIVEN_START = ("1 penalty in the first QP", "10 perturbed, penalty in the first QP")      # shifted lbL / lbR, x0 and y0 given
EXPECT_RET = {"7 maxIterations": 200, "8 maxPenaltyParameter": 201}
# (n, nC, nComp, B, box, pairs)
SHAPES = {
    "nch1": (40, 20, 8, 4, False, "one-hot"),
    "nch2 LR": (200, 330, 37, 2, True, "one-hot"),
    "nch3 dense pairs": (300, 100, 40, 2, False, "dense"),
}
FIRST = {"nch1": 4}      # the first instance of a shape's seed sequence that is used: see option_instances
DENSE_PAIR_SETS = ("1 penalty in the first QP", "3 window of 1") + tuple(s for s in OPTION_SETS if s.startswith("10"))
CASES = [(shape, oset) for shape in SHAPES for oset in OPTION_SETS if SHAPES[shape][5] != "dense" or oset in DENSE_PAIR_SETS]


def options(mod, oset, override=None, **kw):
    """the options of a set on the library or on the oracle (perturbStep = 0 unless the set says otherwise)"""
    return mod.default_options(**dict(dict(perturbStep=0, printLevel=0, **kw), **dict(OPTION_SETS[oset], **(override or {}))))


def with_start(d, seed, ndual):
    """x0 and y0 as test_sparse_bounds_and_initial_guess draws them"""
    rng = np.random.default_rng(seed)
    return dict(d, x0=rng.uniform(-0.5, 0.5, d["nV"]), y0=rng.uniform(-0.1, 0.1, ndual))


def option_instances(shape, oset):
    """(40, 20, 8) starts at the fifth problem of its sequence: of the first four, one converges in 8 rows at rho = 0.04 -- it reaches neither
    limit of the sets 7 and 8 and, started at rho = 1, leaves two step lengths to decide -- and one needs 218 rows without a Leyffer window"""
    n, nC, nComp, B, box, pairs = SHAPES[shape]
    given = oset in GIVEN_START
    ds = TG.make_instances("options " + shape, (n, nC, nComp, B, box, given or pairs == "dense", pairs), first=FIRST.get(shape, 0))
    return [with_start(d, 40 + b, n + nC + 2 * nComp) for b, d in enumerate(ds)] if given else ds


def assert_branch(oset, results, rets, double=False, fills=False):
    """what the option set is there for, from the audit's counters (results: the AuditResults of the case's instances).  double: the case
    is known to make a double update under set 6, (rho f) f with f = 10; fills: the case is known to fill the window of 64 under set 5"""
    results = list(results)
    want = EXPECT_RET.get(oset, 0)
    assert all(r == want for r in rets), (oset, rets)
    total = lambda name: sum(getattr(r, name) for r in results)
    if oset in ("0 default", "3 window of 1", "10 perturbed, window of 1"):
        assert total("leyffer_fired") >= 1, oset
    if oset.startswith("2"):
        assert total("leyffer_fired") == 0 and total("window_shifts") == 0 and total("updates") >= 1, oset      # every update is a stationarity update
    if oset.startswith("4"):
        assert total("window_shifts") >= 1, oset
    if oset.startswith("5"):
        assert (total("window_shifts") >= 1 and total("leyffer_fired") >= 1) if fills else total("window_shifts") == 0, oset
    if oset.startswith("6"):
        assert total("updates") >= 1, oset      # (an instance that is complementary at rho = 1 needs none)
        assert total("double_updates") >= 1 or not double, oset
    if oset in GIVEN_START:
        assert all(r.row0_penalty and r.cx0 > 0 for r in results), oset
    else:
        assert not any(r.row0_penalty for r in results), oset


def run_case(hip, shape, oset):
    n, nC, nComp, B, box, pairs = SHAPES[shape]
    opt = options(hip, oset, storeSteps=1)
    assert opt.resTol == RES_TOL
    t0 = time.perf_counter()
    ds = option_instances(shape, oset)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=opt)
    load_all(bt, ds)
    bt.run()
    bt.synchronize()
    t1 = time.perf_counter()
    assert (bt.read_setup(0)["cNnz"] == -1) == (pairs == "dense")
    label = "%s, %s" % (oset, shape)
    want = EXPECT_RET.get(oset, 0)
    res = TA.audit_batch(bt, ds, range(B), opt, [d.get("x0") for d in ds], opt.initialPenaltyParameter, False, "after_first_update", RES_TOL, label, expect_ret=want)
    x, y, st = bt.solution()
    assert_branch(oset, res.values(), [s["returnValue"] for s in st])
    print(f"    {label}: Leyffer updates {sum(r.leyffer_fired for r in res.values())} full-window rows {sum(r.window_shifts for r in res.values())} "
          f"penalty updates {sum(r.updates for r in res.values())} double {sum(r.double_updates for r in res.values())}")
    if want:      # a run that did not converge returns the last row (audit_batch: bit for bit) and the duals of the last QP solved, untransformed
        for b in range(B):
            sc, xs = bt.trace(b)
            r, bound, r_before = TA.last_qp_duals(ds[b], sc, xs, ds[b].get("x0"), opt.initialPenaltyParameter, y[b], "dense", RES_TOL)
            print(f"    {label} instance {b}: the returned duals in the last QP's stationarity {r:.3e} (bound {bound:.3e}), in the QP's before {r_before:.3e}")
            assert r <= bound < r_before, (label, b, r, bound, r_before)
    bt.close()
    print(f"    {label}: load + run {t1 - t0:.2f} s, audit {time.perf_counter() - t1:.2f} s")


@pytest.mark.parametrize("shape,oset", CASES, ids=["%s-%s" % (s, o) for s, o in CASES])
def test_trace_audit_options(hip, shape, oset):
    run_case(hip, shape, oset)


def test_window_above_capacity_is_refused(hip):
    """nDynamicPenalty = 65 is more than hist[64] of the instance record holds: set_options answers LCQP_HIP_UNSUPPORTED with the dense arm's
    error text, launches nothing, and the object keeps the options it had (assert_refused runs it straight after the refusal)"""
    n, nC, nComp, B, box, pairs = SHAPES["nch1"]
    ds = option_instances("nch1", "0 default")
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=options(hip, "0 default"))
    load_all(bt, ds)
    assert_refused(hip, bt, lambda opt: hip.BatchLCQP(B, n, nC, nComp, opt=opt))
    bt.close()


def assert_refused(hip, bt, create):
    """set_options of a loaded handle bt (holding the default set) and create(opt) with nDynamicPenalty = 65, either arm.  The refused
    options also ask for maxIterations = 3: the run that follows the refusal at once, before any other set_options, converges in more
    than 4 iterates on every instance, so no part of the refused options was taken"""
    refused = hip.default_options(nDynamicPenalty=65, maxIterations=3, printLevel=0)
    counts = bt.launch_counts()
    rc = bt._sym("set_options")(bt.h, ctypes.byref(refused))
    assert rc == LCQP_HIP_UNSUPPORTED and bt._last_error() == REFUSAL, (rc, bt._last_error())
    assert bt.launch_counts() == counts
    bt.run()
    assert all(s["returnValue"] == 0 and s["iterTotal"] > 4 for s in bt.solution()[2])
    counts = bt.launch_counts()
    with pytest.raises(RuntimeError, match="set_options failed with code %d: %s" % (LCQP_HIP_UNSUPPORTED, REFUSAL)):
        create(refused)
    accepted = hip.default_options(nDynamicPenalty=64, printLevel=0)      # the capacity itself is taken
    assert bt._sym("set_options")(bt.h, ctypes.byref(accepted)) == 0
    bt.set_options(options(hip, "0 default"))
    assert bt.launch_counts() == counts
