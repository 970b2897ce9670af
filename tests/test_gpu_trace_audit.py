"""Dense arm: the per-iterate scalars of lcqp_run (lcqp_dev.hpp) held to the direct long-double reference of tests/trace_audit_ref.py.

Every instance's trace (storeSteps) is audited: rho sequence, objective, phi, merit, step norm, step length, stationarity norm and the
replayed decisions (see the reference's docstring for the quantities and where the bounds come from).  The cases walk the instantiations of
the fused pass: EPT = ceil(np / 256) entries per thread (NCH = 1: half the workgroup idle; NCH = 3: a partial last entry), the row state in
LDS (LR) or not, the 256-register "few" build and the 128-register build, C x_k from the compressed rows of C (one-hot pairs) or from a
dense sweep (dense rows of L and R: more than 8 np non-zeros in C, cNnz = -1).

n = 1100 (NCH = 16), B = 1 is kept: 0.15 s for load and run and 2.9 s for its long-double audit on an MI355X machine.  The other cases take
0.1 s to 1.5 s each, the file 10 s.  Worst |recorded - reference| / bound over all cases: objective 0.002, phi 0.005, merit 0.002, step norm
0.08, stationarity 0.46.

g~ of a warm run: the dense prologue starts with g~ = g (WARM_GTIL_RULE = "after_first_update"), the sparse arm with g + rho0 g_phi
("always"); each is audited under its own rule.  The rule shows only in the step lengths of the rows before the
first penalty update, so the warm tests assert that at least one warm row of the case is decided, and print which instances refute the
other rule.  Decided warm rows measured: n64 2, n64 shifted 16, n256 6, n256 shifted 23 (of four instances)."""
import time

import numpy as np
import pytest

import problems as P
import trace_audit_ref as TA
from batch_helpers import load_all, update_all

pytestmark = pytest.mark.gpu

RES_TOL = 1e-12      # the subsolver's verification tolerance: options.resTol (lcqp_hip.hip, lcqp_hip_options_default), applied as
#                      rtolQ = resTol (1 + |g|_inf) in qp_solve (lcqp_dev.hpp) and tested in qp_polish's "stage 2" acceptance


def dense_pairs_lcqp(rng, n, nC, nComp, box):
    """An LCQP whose complementarity rows are DENSE: L, R full rows, so C = L'R + R'L is a full matrix.  A point xs is feasible and
    complementary by construction: per pair one side sits on its lower bound at xs, the other 0.1 .. 1 above it (lbL, lbR are non-zero:
    these problems are always "shifted")."""
    M = rng.uniform(-1, 1, (n, n)); Q = M.T @ M / n + np.eye(n)
    L = rng.uniform(-1, 1, (nComp, n)) / np.sqrt(n); R = rng.uniform(-1, 1, (nComp, n)) / np.sqrt(n)
    xs = rng.uniform(0.2, 1, n)
    side = rng.random(nComp) < 0.5
    slack = rng.uniform(0.1, 1, nComp)
    lbL = L @ xs - np.where(side, 0.0, slack); lbR = R @ xs - np.where(side, slack, 0.0)
    A = rng.uniform(-1, 1, (nC, n)) / np.sqrt(n)
    d = dict(Q=Q, g=rng.uniform(-1, 1, n), L=L, R=R, A=A, lbA=A @ xs - rng.uniform(0.1, 1, nC), ubA=A @ xs + rng.uniform(0.1, 1, nC),
             lbL=lbL, lbR=lbR, nV=n, nC=nC, nComp=nComp)
    if box:
        d.update(lb=xs - 2.0, ub=np.where(rng.random(n) < 0.5, xs + 2.0, np.inf))
    return d


# (n, nC, nComp, B, box, shifted, pairs)
CASES = {
    "nch1 one-hot": (40, 20, 8, 4, False, False, "one-hot"),
    "nch1 sweep": (40, 20, 8, 4, True, True, "dense"),
    "nch2 LR": (200, 330, 37, 2, True, False, "one-hot"),
    "nch2 rows in memory": (200, 700, 37, 2, False, True, "one-hot"),
    "nch3 partial entry": (300, 100, 40, 2, False, True, "dense"),
    "nch4": (500, 200, 50, 2, True, False, "one-hot"),
    "nch8": (600, 200, 50, 1, True, True, "one-hot"),
    "128-register build": (40, 20, 8, 800, False, True, "one-hot"),
}
CASE_1100 = (1100, 300, 60, 1, False, True, "one-hot")
WARM_SHAPES = ((64, 128, 16), (256, 512, 64))
WARM_GTIL_RULE = "after_first_update"      # lcqp_run's prologue: gtil = g, warm or not (DESIGN.md section 3a says why it stays so)
WARM_B = 4


def make_instances(name, case, count=None, first=0):
    n, nC, nComp, B, box, shifted, pairs = case
    assert shifted or pairs != "dense"
    gen = (lambda rng: dense_pairs_lcqp(rng, n, nC, nComp, box)) if pairs == "dense" else (lambda rng: P.random_lcqp(rng, n, nC, nComp, box, shifted))
    seed0 = sum(ord(ch) for ch in name) * 1000
    return [gen(np.random.default_rng(seed0 + b)) for b in range(first, first + (count or B))]


def audited(case):
    """the instances of a case that are audited: all of them, of the batch of 800 eight spread over it"""
    B = case[3]
    return list(range(B)) if B <= 8 else [int(v) for v in np.linspace(0, B - 1, 8)]


def warm_instances(shape, shifted):
    n, nC, nComp = shape
    return [P.random_lcqp(np.random.default_rng(7000 + 10 * n + b + (500 if shifted else 0)), n, nC, nComp, False, shifted) for b in range(WARM_B)]


def run_case(hip, name, case, perturb=0):
    n, nC, nComp, B, box, shifted, pairs = case
    opt = hip.default_options(perturbStep=perturb, storeSteps=1, printLevel=0)
    assert opt.resTol == RES_TOL
    t0 = time.perf_counter()
    which = audited(case)
    if B > 8:      # the batch of 800: eight problems, repeated
        base = make_instances(name, case, count=8)
        ds = [base[b % 8] for b in range(B)]
    else:
        ds = make_instances(name, case)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=opt)
    load_all(bt, ds)
    bt.run()
    bt.synchronize()
    t1 = time.perf_counter()
    cnz = bt.read_setup(which[0])["cNnz"]
    assert (cnz == -1) == (pairs == "dense"), cnz      # the sweep branch exactly for the dense rows
    TA.audit_batch(bt, ds, which, opt, None, opt.initialPenaltyParameter, False, "after_first_update", RES_TOL, name)
    bt.close()
    print(f"    {name}: load + run {t1 - t0:.2f} s, audit {time.perf_counter() - t1:.2f} s")


@pytest.mark.parametrize("name", list(CASES))
def test_trace_audit(hip, name):
    run_case(hip, name, CASES[name])


def test_trace_audit_nch16(hip):
    """n = 1100: NCH = 16, EPT = 8"""
    run_case(hip, "nch16", CASE_1100)


def test_trace_audit_perturbed(hip):
    """perturbStep = 1: the identities hold unchanged, the +-2.221e-16 on x enters the bounds where d_k stands for alpha_k p_k"""
    run_case(hip, "nch2 LR perturbed", CASES["nch2 LR"], perturb=1)


@pytest.mark.parametrize("shifted", [False, True], ids=["zero bounds", "shifted"])
@pytest.mark.parametrize("shape", WARM_SHAPES, ids=lambda s: "n%d" % s[0])
def test_trace_audit_warm(hip, shape, shifted):
    """load, run, update with the 2 % recipe, resolve(warm): the warm run's trace starts at the first run's x and rhoOpt, and its row 0 has no
    zero-penalty QP behind it.  g~ of a warm run: DESIGN.md section 3a.  (A warm re-solve after a 2 % change is a few rows long; the first
    run is audited with it, and the two together are the instance's rows under the cap of tests/test_trace_audit_ref.py.)"""
    n, nC, nComp = shape
    opt = hip.default_options(perturbStep=0, storeSteps=1, printLevel=0)
    ds = warm_instances(shape, shifted)
    bt = hip.BatchLCQP(WARM_B, n, nC, nComp, opt=opt)
    load_all(bt, ds)
    bt.run()
    x1, _, st1 = bt.solution()
    assert all(s["returnValue"] == 0 for s in st1)
    TA.audit_batch(bt, ds, range(WARM_B), opt, None, opt.initialPenaltyParameter, False, "after_first_update", RES_TOL, "first run n%d" % n)
    ds2 = [P.perturbed(d, 300 + b) for b, d in enumerate(ds)]
    update_all(bt, ds2)
    bt.resolve(warm=True)
    label = "warm n%d%s" % (n, " shifted" if shifted else "")
    rho1 = [s["rhoOpt"] for s in st1]
    res = TA.audit_batch(bt, ds2, range(WARM_B), opt, x1, rho1, True, WARM_GTIL_RULE, RES_TOL, label)
    assert sum(r.decided for r in res.values()) >= 1, label      # the rule for g~ shows in the step lengths only: some warm row has to be decided
    if shifted:
        hit = TA.refuted_by_step_length(bt, ds2, range(WARM_B), opt, x1, rho1, True, "always", RES_TOL)
        print(f"    {label}: the rule 'always' is refuted by the step lengths of instances {hit}")
        assert hit, label      # measured: instances 0 and 3 at n = 64, all four at n = 256
    bt.close()

