"""Sparse arm: the per-iterate scalars of sp_ph_qpend (lcqp_sparse_solver.hpp) held to the direct long-double reference of
tests/trace_audit_ref.py, through SparseBatchLCQP.

The problems are densified for the reference (Q and the rows of E = [A; L; R]); the engines are the ones the other sparse tests select:
lane groups of 8, 16, 32 and 64 (LCQP_SPARSE_LANES on the synthetic workload at its smallest shape), the bordered band (the circle
example) and the general sparse LDL' (LCQP_SPARSE_GENERAL at the mid shape), each asserted through the handle's queries.  perturbStep = 0
is the path on which C x_k follows the steps by linearity (carried_C in the audit's bounds), perturbStep = 1 the one that forms it anew.

Measured on an MI355X (worst |recorded - reference| / bound over all rows): the carried path stays far inside its bound on every engine --
phi 0.7 % to 1.1 % of the bound, objective 0.002, merit 0.002, stationarity 0.15 -- so the carry of C x_k is sound.  Each case takes 0.1 s at the small
shape and 3.7 s at the mid shape (the long-double audit of four instances of n = 512), the file 25 s.

What the audit found here, and what was fixed with it: test_sparse_trace_audit[<engine>-perturbed-zero bounds], six cases, failed on `phi`
at the last rows of an inner loop (lanes 8, instance 1, rows 41 and 43 to 45: recorded -6.2440925543612879e-17, direct
-1.2488185142226164e-16, bound 5.5e-30; the bordered band rows 23 to 25: -6.84e-16 against -1.369e-15; the general LDL' rows 41 to 43:
-1.155e-16 against -2.310e-16): the recorded value was HALF the direct one.  With perturbStep sp_ph_qpend took C x_k from the perturbed x_k
and formed C p_k = C x_q - C x_k with it, but p_k = x_q - x_k is the unperturbed difference; after the step C x_k was short of
alpha C delta (delta the perturbation), so at a complementary x_q (x_q'C x_q = 0) phi = x'Cx / 2 came out as delta'C x_q / 2 instead of
delta'C x_q -- and at a full step the perturbation did not reach the penalty gradient rho C x_k at all.  The pass now forms C p_k from p_k
itself, as the dense kernel does."""
import time

import numpy as np
import pytest

import problems as P
import trace_audit_ref as TA
from batch_helpers import handle, update_all

pytestmark = pytest.mark.gpu

RES_TOL = 1e-12      # options.resTol as sp_polish's acceptance applies it (lcqp_sparse_solver.hpp: res_stat <= max(resTol (1 + |g|_inf), ...))
B = 4
# engine -> (shape or "circle", environment)
ENGINES = {
    "lanes 8": (P.SMALL, {}),
    "lanes 16": (P.SMALL, {"LCQP_SPARSE_LANES": "16"}),
    "lanes 32": (P.SMALL, {"LCQP_SPARSE_LANES": "32"}),
    "lanes 64": (P.SMALL, {"LCQP_SPARSE_LANES": "64"}),
    "bordered band": ("circle", {}),
    "general ldl": (P.MID, {"LCQP_SPARSE_GENERAL": "1"}),
}
WARM_SHAPES = (P.SMALL, P.MID)


def sparse_instances(shape, shifted, count=B):
    ds = P.circle_instances(count) if shape == "circle" else P.instances(shape, count)
    if shifted:      # (the circle's R variables sum to one over a hundred pairs: a tenth of the shift keeps it feasible)
        nK, s = ds[0]["nComp"], 0.1 if shape == "circle" else 1.0
        ds = [dict(d, lbL=np.full(nK, 0.01 * s), lbR=np.full(nK, 0.02 * s)) for d in ds]
    return ds


def densified(d):
    """the problem dict of tests/problems.py's dense layout from a sparse instance"""
    nC, nK = d["nC"], d["nComp"]
    E = d["E"].toarray()
    out = dict(Q=d["Q"].toarray(), g=d["g"], A=E[:nC], L=E[nC:nC + nK], R=E[nC + nK:], lbA=d["lbA"], ubA=d["ubA"], nV=d["nV"], nC=nC, nComp=nK)
    for k in ("lbL", "lbR", "x0"):
        if d.get(k) is not None:
            out[k] = d[k]
    return out


def assert_engine(sb, engine):
    if engine.startswith("lanes"):
        assert sb.lanes() == int(engine.split()[1]) and sb.border() == 0 and sb.fronts() == 0
    elif engine == "bordered band":
        assert sb.border() == 3 and sb.fronts() == 0
    else:
        assert sb.fronts() > 0


@pytest.mark.parametrize("shifted", [False, True], ids=["zero bounds", "shifted"])
@pytest.mark.parametrize("perturb", [0, 1], ids=["carried", "perturbed"])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_sparse_trace_audit(hip, monkeypatch, engine, perturb, shifted):
    shape, env = ENGINES[engine]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    opt = hip.default_options(perturbStep=perturb, storeSteps=1, printLevel=0)
    assert opt.resTol == RES_TOL
    t0 = time.perf_counter()
    ds = sparse_instances(shape, shifted)
    sb = handle(hip, ds, opt)
    assert_engine(sb, engine)
    sb.run()
    sb.synchronize()
    t1 = time.perf_counter()
    x0 = [d.get("x0") for d in ds]
    label = "%s%s%s" % (engine, " perturbed" if perturb else "", " shifted" if shifted else "")
    TA.audit_batch(sb, ds, range(B), opt, x0, opt.initialPenaltyParameter, False, "after_first_update", RES_TOL, label, carried_C=not perturb, densify=densified)
    sb.close()
    print(f"    {label}: load + run {t1 - t0:.2f} s, audit {time.perf_counter() - t1:.2f} s")


@pytest.mark.parametrize("shifted", [False, True], ids=["zero bounds", "shifted"])
@pytest.mark.parametrize("shape", WARM_SHAPES, ids=lambda s: "n%d" % s[0])
def test_sparse_trace_audit_warm(hip, shape, shifted):
    """load, run, update with the 2 % recipe, resolve(warm): the trace starts at the first run's x and rhoOpt; a warm run of the sparse
    arm starts with g~ = g + rho g_phi (sp_ph_start)"""
    opt = hip.default_options(perturbStep=0, storeSteps=1, printLevel=0)
    ds = sparse_instances(shape, shifted)
    sb = handle(hip, ds, opt)
    sb.run()
    x1, _, st1 = sb.solution()
    assert all(s["returnValue"] == 0 for s in st1)
    TA.audit_batch(sb, ds, range(B), opt, [d.get("x0") for d in ds], opt.initialPenaltyParameter, False, "after_first_update", RES_TOL,
                   "first run n%d" % shape[0], carried_C=True, densify=densified)
    ds2 = [P.moved(d, 300 + b) for b, d in enumerate(ds)]
    update_all(sb, ds2)
    sb.resolve(warm=True)
    label = "warm n%d%s" % (shape[0], " shifted" if shifted else "")
    rho1 = [s["rhoOpt"] for s in st1]
    res = TA.audit_batch(sb, ds2, range(B), opt, x1, rho1, True, "always", RES_TOL, label, carried_C=True, densify=densified)
    assert sum(r.decided for r in res.values()) >= 1, label      # the rule for g~ shows in the step lengths only: some warm row has to be decided
    if shifted:
        hit = TA.refuted_by_step_length(sb, ds2, range(B), opt, x1, rho1, True, "after_first_update", RES_TOL, carried_C=True, densify=densified)
        print(f"    {label}: the rule 'after_first_update' is refuted by the step lengths of instances {hit}")
    sb.close()
