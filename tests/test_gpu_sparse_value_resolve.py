"""Re-solving a loaded sparse batch after a change of the VALUES of its matrices (lcqp_hip_sparse_update_values / _update_values_device, then
lcqp_hip_sparse_resolve): k_sparse_pack_values alone on the range, and for a warm re-solve k_sparse_setup_warm where a run has k_sparse_setup.

As in tests/test_gpu_sparse_resolve.py: cold re-solves are held to the BITS of a fresh handle given the same data by load and solved by run;
warm re-solves to the sparse CPU oracle asked for the same thing in the reference's own terms (x0, y0 = the device's last solution,
solveZeroPenaltyFirst = 0, initialPenaltyParameter = its last rhoOpt) under that file's 1e-8 / 1e-6, iterate counts within 4 of the oracle's
and below the cold count, and to the first-order conditions of the LCQP itself on the new data (problems.lcqp_kkt_residuals, with the bounds
test_statuses_follow_moved_bounds uses: 1e-8, 1e-8, 1e-9).  Warm and cold solves may end at different stationary points: nothing compares one
with the other.

The value recipe new_values(d, seed, eps = 0.02): Q o s s' on the stored entries with s = 1 + eps z (symmetric and as definite as Q),
every stored entry of [A; L; R] times 1 + eps z', the vectors by problems.moved.  Seeds 2000 + b: the CPU oracle alone solves every one of
them warm with return value 0 in 2 - 4 iterates against 20 - 56 cold (SMALL 0 .. 20, MID 0 .. 3, the circle 0 .. 2; the same holds for Qx
alone, Ax alone and the values without new vectors on SMALL 0 .. 5).  The definiteness case uses instance 1 with s_5 = 4000: the oracle's
warm solve returns 0 in 2 iterates there and in 2 more after the original Qx is sent back."""
import torch      # noqa: F401 -- before the library is first loaded: the library and torch must share one HIP runtime (lcqpow_amd.capi.lib)

import ctypes

import numpy as np
import pytest

import problems as P
import sparse_kkt_ref as R
from batch_helpers import assert_same_bits, handle, result, stack, update_all
from problems import MID, OPT, SMALL, circle_instances, instances, moved
from test_gpu_sparse_factor import _admm_weights, _rhs, check_solves
from test_gpu_sparse_resolve import X_TOL, Y_TOL, assert_warm_parity, fresh, oracle_solve, oracle_warm

pytestmark = pytest.mark.gpu

SEED = 2000
NOT_SETUP, INVALID_ARGUMENT = 300, 100


def new_values(d, seed, eps=0.02, spike=None):
    rng = np.random.default_rng(seed)
    n = d["nV"]
    s = 1.0 + eps * rng.standard_normal(n)
    if spike is not None:
        s[spike] = 4000.0
    Q = d["Q"].copy()
    Q.data = Q.data * s[Q.indices] * s[np.repeat(np.arange(n), np.diff(Q.indptr))]
    E = d["E"].copy()
    E.data = E.data * (1.0 + eps * rng.standard_normal(E.nnz))
    return moved(dict(d, Q=Q, E=E), seed + 50000)


def qx(ds):
    return np.stack([d["Q"].data for d in ds])


def ax(ds):
    return np.stack([d["E"].data for d in ds])


def send_values(sb, ds, first=0, Q=True, A=True):
    rc = sb.update_values(first, len(ds), Qx=qx(ds) if Q else None, Ax=ax(ds) if A else None)
    assert rc == 0, (rc, sb._last_error())


def last_of(sb):
    """the device's last solution in the terms of oracle_warm"""
    x, y, st = sb.solution()
    return [dict(x=x[k], y=y[k], stats=st[k]) for k in range(len(st))], st


def assert_kkt(ds, x, y, st):
    """the first-order conditions of the LCQP itself on the data in ds (the sparse arm's y: rows A, L, R, no box)"""
    for b, d in enumerate(ds):
        n, nC, nK = d["nV"], d["nC"], d["nComp"]
        E = d["E"].toarray()
        dd = dict(nV=n, nC=nC, nComp=nK, Q=d["Q"].toarray(), g=d["g"], A=E[:nC], L=E[nC:nC + nK], R=E[nC + nK:], lbA=d["lbA"], ubA=d["ubA"])
        stat, feas, compl, sign = P.lcqp_kkt_residuals(dd, x[b], np.concatenate([np.zeros(n), y[b]]), st[b]["rhoOpt"])
        print(f"    instance {b}: stationarity {stat:.2e} infeasibility {feas:.2e} complementarity {compl:.2e} wrong-signed multiplier {sign:.2e}")
        assert stat < 1e-8 and feas < 1e-8 and compl < 1e-9 and sign < 1e-8, (b, stat, feas, compl, sign)


CASES = {"small": (SMALL, 6, None), "pools of 4": (SMALL, 21, "LCQP_SPARSE_POOL"), "lanes 32": (SMALL, 6, "LCQP_SPARSE_LANES"),
         "mid": (MID, 4, None), "general ldl": (MID, 3, "LCQP_SPARSE_GENERAL"), "bordered circle": (None, 3, None)}
HOOK_VALUE = dict(LCQP_SPARSE_POOL="4", LCQP_SPARSE_LANES="32", LCQP_SPARSE_GENERAL="1")


def make_case(monkeypatch, case):
    shape, B, hook = CASES[case]
    if hook:
        monkeypatch.setenv(hook, HOOK_VALUE[hook])
    ds1 = circle_instances(B) if shape is None else instances(shape, B)
    return ds1, [new_values(d, SEED + b) for b, d in enumerate(ds1)]


def check_engine(sb, case):
    if case == "lanes 32": assert sb.lanes() == 32
    if case == "general ldl": assert sb.fronts() > 0
    if case == "bordered circle": assert sb.border() == 3
    if case in ("small", "pools of 4"): assert sb.lanes() == 8


# ---- 1: warm against the oracle, every engine ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_warm_value_resolve_against_the_oracle(hip, oracle, monkeypatch, case):
    ds1, ds2 = make_case(monkeypatch, case)
    sb = handle(hip, ds1, hip.default_options(**OPT))
    check_engine(sb, case)
    sb.run()
    last, st1 = last_of(sb)
    assert all(s["returnValue"] == 0 for s in st1)
    send_values(sb, ds2)
    update_all(sb, ds2)
    sb.resolve(warm=True)
    x, y, st = sb.solution()
    assert sb.launch_counts() == (2, 2)                          # the warm setup counts as a setup
    setup_ms, solve_ms = sb.last_timing()
    assert setup_ms > 0 and solve_ms > 0
    sb.close()
    assert_warm_parity(st, x, y, oracle_warm(oracle, ds2, last), [s["iterTotal"] for s in st1])
    assert_kkt(ds2, x, y, st)


# ---- 2: the factors belong to the new values -------------------------------------------------------------------------------------------------
def violates(name, K, perm, sol, cols, kb):
    """the solves do NOT hold the bound of check_solves against the matrix K (for a bordered band: not even the widened one)"""
    Kp = K[np.ix_(perm, perm)]
    _, _, Wm = R.ldl_nopivot(Kp, R.ref_dtype(len(perm)))
    X, B = sol.T[perm], cols[perm]
    res, bound = R.residual_and_bound(Kp, Wm, X, B)
    if kb:
        rr, rb = R.residual_and_bound(Kp, Wm, R.bordered_ref(Kp, kb, B), B)
        bound = bound * R.LD(max(1.0, 8.0 * float(np.where(rb > 0, rr / np.where(rb > 0, rb, 1), 0).max())))
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.where(res > 0, res / bound, 0.0).max())
    print(f"    {name}: worst error / bound against the OLD values = {worst:.3e}")
    assert worst > 1.0, (name, worst)


@pytest.mark.parametrize("case", ["small", "general ldl", "bordered circle"])
def test_factors_belong_to_the_new_values(hip, monkeypatch, case):
    """the polish refines through exact residuals: a stale factor would still converge and pass the parity test.  Here the stored polish
    factor and the ADMM factor are held to the long-double LDL' of the NEW values under the bound of tests/test_gpu_sparse_factor.py -- and
    must violate it against the old ones"""
    ds1, ds2 = make_case(monkeypatch, case)
    opt = hip.default_options(**OPT)
    sb = handle(hip, ds1, opt)
    check_engine(sb, case)
    sb.run()
    send_values(sb, ds2)
    update_all(sb, ds2)
    sb.resolve(warm=True)
    _, _, st = sb.solution()
    B, N, m = len(ds2), sb.nV + sb.m, sb.m
    perm = sb.ordering()
    rhs, cols = _rhs(N, B, unit=(case == "small"))
    pol, prec = sb.kkt_probe(rhs, which=0)
    adm, arec = sb.kkt_probe(rhs, which=1)
    kb = sb.border()
    sb.close()
    picked = range(B) if case != "general ldl" else (0, B - 1)      # (N = 896: a long-double LDL' takes seconds)
    for b in picked:
        assert st[b]["returnValue"] == 0
        for d, check in ((ds2[b], True), (ds1[b], False)):
            Kp = R.kkt_dense(d, prec["dprim"][b], prec["ddual"][b], prec["use"][b])
            dd = _admm_weights(opt, d, ds2[b]["lbA"], ds2[b]["ubA"])
            Ka = R.kkt_dense(d, opt.admmSigma * R.scale_of(d), dd, np.ones(m, dtype=np.int32))
            if check:
                assert arec["dprim"][b] == opt.admmSigma * R.scale_of(d) and np.array_equal(arec["ddual"][b], dd) and arec["use"][b].all(), (case, b)
                sc = R.scale_of(d)
                assert (prec["dprim"][b], prec["ddual"][b][0]) in [(opt.proxBig * sc, 1e-9 / sc), (opt.proxSmall * sc, 1e-14 / sc)], (case, b)
                check_solves(f"{case} / polish, new values / instance {b}", Kp, perm, pol[b], cols[b], kb=kb)
                check_solves(f"{case} / ADMM, new values / instance {b}", Ka, perm, adm[b], cols[b], kb=kb)
            else:
                violates(f"{case} / polish / instance {b}", Kp, perm, pol[b], cols[b], kb)
                violates(f"{case} / ADMM / instance {b}", Ka, perm, adm[b], cols[b], kb)


# ---- 3: unchanged values are one iterate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "mid", "bordered circle"])
def test_unchanged_values_are_one_iterate(hip, monkeypatch, case):
    ds1, _ = make_case(monkeypatch, case)
    sb = handle(hip, ds1, hip.default_options(**OPT))
    sb.run()
    x1, y1, st1 = sb.solution()
    assert all(s["returnValue"] == 0 for s in st1)
    send_values(sb, ds1)
    sb.resolve(warm=True)
    x2, y2, st2 = sb.solution()
    assert sb.launch_counts() == (2, 2)
    sb.close()
    for k in range(len(ds1)):
        assert st2[k]["returnValue"] == 0 and st2[k]["iterTotal"] == 1, (k, st2[k])
        assert np.abs(x2[k] - x1[k]).max() < X_TOL, k


# ---- 4: a cold re-solve is a fresh solve, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small, traced", "pools of 4", "lanes 32", "mid", "general ldl", "bordered circle"])
def test_cold_value_resolve_is_a_fresh_solve(hip, monkeypatch, case):
    store = case == "small, traced"
    name = "small" if store else case
    opt = hip.default_options(storeSteps=1 if store else 0, **OPT)
    ds1, ds2 = make_case(monkeypatch, name)
    sb = handle(hip, ds1, opt)
    check_engine(sb, name)
    sb.run()
    first = result(sb, store)
    send_values(sb, ds2)
    update_all(sb, ds2)
    for b in (0, len(ds2) - 1):      # the values-only pack leaves what the load's leaves
        got = sb.read_problem(b)
        assert np.array_equal(got["Qx"], ds2[b]["Q"].data) and np.array_equal(got["Ax"], ds2[b]["E"].data) and np.array_equal(got["g"], ds2[b]["g"]), b
    sb.resolve()
    again = result(sb, store)
    assert sb.launch_counts() == (2, 2)                          # no setup belongs to the new values: the cold re-solve is a run
    sb.close()
    assert_same_bits(again, fresh(hip, ds2, opt, trace=store))
    assert not np.array_equal(first["x"], again["x"])


# ---- 5: partial calls --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["Qx only", "Ax only", "instances 2 .. 4"])
def test_partial_value_updates(hip, oracle, part):
    shape, B = SMALL, 6
    ds1 = instances(shape, B)
    new = [new_values(d, SEED + b) for b, d in enumerate(ds1)]
    if part == "Qx only": ds2 = [dict(d, Q=v["Q"]) for d, v in zip(ds1, new)]
    elif part == "Ax only": ds2 = [dict(d, E=v["E"]) for d, v in zip(ds1, new)]
    else: ds2 = [dict(d, Q=v["Q"], E=v["E"]) if 2 <= b < 5 else d for b, (d, v) in enumerate(zip(ds1, new))]
    sb = handle(hip, ds1, hip.default_options(**OPT))
    assert sb.lanes() == 8
    sb.run()
    last, st1 = last_of(sb)
    if part == "instances 2 .. 4": send_values(sb, ds2[2:5], first=2)
    else: send_values(sb, ds2, Q=part == "Qx only", A=part == "Ax only")
    for b in range(B):
        got = sb.read_problem(b)
        assert np.array_equal(got["Qx"], ds2[b]["Q"].data) and np.array_equal(got["Ax"], ds2[b]["E"].data), (part, b)
    sb.resolve(warm=True)                                        # (without new vectors)
    x, y, st = sb.solution()
    assert sb.launch_counts() == (2, 2)
    sb.close()
    assert_warm_parity(st, x, y, oracle_warm(oracle, ds2, last), [s["iterTotal"] for s in st1])
    assert_kkt(ds2, x, y, st)
    if part == "instances 2 .. 4":
        assert all(st[b]["iterTotal"] == 1 for b in (0, 1, 5)), [s["iterTotal"] for s in st]


# ---- 6: crossing the definiteness line ------------------------------------------------------------------------------------------------------------
def test_crossing_the_definiteness_line(hip, oracle):
    """one Q_kk of one instance grows 1.6e7-fold: min Q_ii / max Q_ii of that instance falls under 1e-6, the batch loses the light
    regularisation of the polish (and its second ordering, where the pattern has one); the original Qx brings both back.  (read_polish
    answers after a solve: lightOK is read behind the re-solve that followed the update.)"""
    shape, B, k, var = SMALL, 6, 1, 5
    opt = hip.default_options(**OPT)
    ds1 = instances(shape, B)
    ds2 = [new_values(d, SEED + b, spike=var if b == k else None) for b, d in enumerate(ds1)]
    dq = ds2[k]["Q"].diagonal()
    assert dq.min() / dq.max() < 1e-6 and np.linalg.eigvalsh(ds2[k]["Q"].toarray()).min() > 0
    sb = handle(hip, ds1, opt)
    sb.run()
    last, st1 = last_of(sb)
    cold_iters = [s["iterTotal"] for s in st1]
    assert sb.read_polish(0)["lightOK"] == 1
    perm1 = sb.ordering()
    send_values(sb, ds2)
    update_all(sb, ds2)
    perm2 = sb.ordering()
    sb.resolve(warm=True)
    assert sb.read_polish(0)["lightOK"] == 0
    last2, st2 = last_of(sb)
    x, y, _ = sb.solution()
    assert_warm_parity(st2, x, y, oracle_warm(oracle, ds2, last), cold_iters)
    # the original Qx back: definite again
    ds3 = [dict(d, Q=o["Q"]) for d, o in zip(ds2, ds1)]
    send_values(sb, ds3, A=False)
    perm3 = sb.ordering()
    sb.resolve(warm=True)
    pol = [sb.read_polish(b) for b in range(B)]
    assert all(p["lightOK"] == 1 and p["bigReg"] == 0 for p in pol), [(p["lightOK"], p["bigReg"]) for p in pol]
    x, y, st3 = sb.solution()
    assert sb.launch_counts() == (3, 3)
    assert np.array_equal(perm1, perm3)
    sb2 = hip.SparseBatchLCQP(B, *shape, ds1[0]["Q"], ds1[0]["E"], opt=opt)      # the plain ordering of this pattern: before any load
    second_ordering = not np.array_equal(sb2.ordering(), perm1)
    sb2.close()
    print(f"    the pattern has a second ordering: {second_ordering}")
    if second_ordering:
        assert not np.array_equal(perm1, perm2)
    assert_warm_parity(st3, x, y, oracle_warm(oracle, ds3, last2), cold_iters)
    # cold on the spiked values: the bits of a fresh handle
    send_values(sb, ds2, A=False)
    sb.resolve()
    again = result(sb)
    sb.close()
    assert_same_bits(again, fresh(hip, ds2, opt))


# ---- 7: the device twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [0, 3])
def test_device_twin_leaves_the_bits_of_the_host_call(hip, shared):
    shape, B = SMALL, 6
    opt = hip.default_options(**OPT)
    ds1 = instances(shape, B)
    ds2 = [new_values(d, SEED + b) for b, d in enumerate(ds1)]
    if shared:
        ds2 = [dict(d, Q=ds2[0]["Q"], E=ds2[0]["E"]) for d in ds2]      # one pair of value arrays for the batch
    out = []
    for device in (False, True):
        sb = handle(hip, ds1, opt)
        sb.run()
        if device:
            dev = torch.device("cuda", sb.device)
            T = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
            tq, ta = (T(ds2[0]["Q"].data), T(ds2[0]["E"].data)) if shared else (T(qx(ds2)), T(ax(ds2)))
            assert sb.update_values_device(0, B, Qx=tq, Ax=ta, shared=shared) == 0
            torch.cuda.synchronize()
        else:
            send_values(sb, ds2)
        got = sb.read_problem(B - 1)
        assert np.array_equal(got["Qx"], ds2[B - 1]["Q"].data) and np.array_equal(got["Ax"], ds2[B - 1]["E"].data)
        update_all(sb, ds2)
        sb.resolve(warm=True)
        out.append(result(sb))
        assert sb.launch_counts() == (2, 2)
        sb.close()
    assert all(s["returnValue"] == 0 for s in out[0]["st"])
    assert_same_bits(out[1], out[0])


# ---- 8: instances whose last run failed run cold -----------------------------------------------------------------------------------------------------
def test_failed_instances_run_cold(hip):
    shape, B = SMALL, 6
    ds1 = instances(shape, B)
    ds2 = [new_values(d, SEED + b) for b, d in enumerate(ds1)]
    opt = hip.default_options(maxIterations=3, **OPT)
    sb = handle(hip, ds1, opt)
    sb.run()
    _, _, st = sb.solution()
    assert all(s["returnValue"] == hip.capi.MAX_ITERATIONS_REACHED for s in st)
    send_values(sb, ds2)
    update_all(sb, ds2)
    sb.resolve(warm=True)                                       # k_sparse_setup_warm with no warm instance
    warm = result(sb)
    assert sb.launch_counts() == (2, 2)
    sb.close()
    assert_same_bits(warm, fresh(hip, ds2, opt))


# ---- 9: guards launch nothing ---------------------------------------------------------------------------------------------------------------------------
def test_guards_launch_nothing(hip):
    L = hip.lib()
    shape, B = SMALL, 4
    n, nC, nK = shape
    opt = hip.default_options(**OPT)
    ds1 = instances(shape, B)
    ds2 = [new_values(d, SEED + b) for b, d in enumerate(ds1)]
    sb = handle(hip, ds1, opt)
    empty = hip.SparseBatchLCQP(B, n, nC, nK, ds1[0]["Q"], ds1[0]["E"], opt=opt)      # no instance holds a problem
    sb.run()
    first = result(sb)
    assert sb.launch_counts() == (1, 1)
    DP = ctypes.POINTER(ctypes.c_double)
    Q2, A2 = qx(ds2), ax(ds2)
    qp, ap = Q2.ctypes.data_as(DP), A2.ctypes.data_as(DP)
    tq = torch.as_tensor(Q2, device=torch.device("cuda", sb.device)); ta = torch.as_tensor(A2, device=tq.device)
    dq, da = ctypes.c_void_p(tq.data_ptr()), ctypes.c_void_p(ta.data_ptr())
    host = lambda f, c, q, a, h=sb: L.lcqp_hip_sparse_update_values(h.h, f, c, q, a)
    devc = lambda f, c, sh, q, a, h=sb: L.lcqp_hip_sparse_update_values_device(h.h, f, c, sh, q, a, None)
    assert host(0, 1, None, None) == INVALID_ARGUMENT and devc(0, 1, 0, None, None) == INVALID_ARGUMENT
    for f, c in ((-1, 1), (0, 0), (B - 1, 2), (B, 1), (0, 2 ** 31 - 1)):
        assert host(f, c, qp, ap) == INVALID_ARGUMENT and devc(f, c, 0, dq, da) == INVALID_ARGUMENT
    assert host(0, B, qp, ap, empty) == NOT_SETUP and devc(1, 1, 0, dq, da, empty) == NOT_SETUP and host(B - 1, 1, qp, None, empty) == NOT_SETUP
    assert empty.launch_counts() == (0, 0)
    empty.close()
    assert devc(0, B, 4, dq, da) == INVALID_ARGUMENT and devc(0, B, -1, dq, da) == INVALID_ARGUMENT
    assert devc(0, B, 0, ctypes.c_void_p(Q2.ctypes.data), None) == INVALID_ARGUMENT      # host memory handed to the device twin
    assert devc(0, B, 0, None, ctypes.c_void_p(A2.ctypes.data)) == INVALID_ARGUMENT
    with pytest.raises(ValueError):
        sb.update_values(0, B, Qx=np.zeros(sb.nnzQ))
    with pytest.raises(ValueError):
        sb.update_values(B - 1, 2, Qx=Q2[:2])
    assert sb.launch_counts() == (1, 1)
    sb.sensitivity(np.ones((B, n)))                              # no refused call touched a mark: the solve still stands
    sb.resolve()
    assert_same_bits(result(sb), first)                          # ... or wrote anything
    assert sb.launch_counts() == (1, 2)
    # behind update_values nothing belongs to a solve until the next one
    send_values(sb, ds2)
    for call in (lambda: sb.sensitivity(np.ones((B, n))), lambda: sb.kkt_probe(np.ones((B, 1, n + sb.m)), which=1), lambda: sb.read_polish(0)):
        with pytest.raises(RuntimeError, match="code 300"):
            call()
    assert sb.launch_counts() == (1, 2)
    # a load clears the kept point: the warm re-solve is a run
    assert sb.load(0, B, Q2, stack(ds2, "g"), A2, lbA=stack(ds2, "lbA"), ubA=stack(ds2, "ubA")) == 0
    sb.resolve(warm=True)
    again = result(sb)
    assert sb.launch_counts() == (2, 3)
    sb.sensitivity(np.ones((B, n)))
    sb.close()
    assert_same_bits(again, fresh(hip, ds2, opt))


# ---- 10: the torch layer ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_torch_layer_with_warm_matrices(hip, on_device):
    """Qx.grad of the warm solve against the gradient of a layer without the switch.  The two solves are different runs that end within
    X_TOL of each other on one working set; dl/dQ_ij = -(d_i x_j + d_j x_i) / 2 with d = dl/dg from ONE matrix K0 on both sides, so the
    two differ by |d|_inf |dx|_inf <= X_TOL |d|_inf per entry, plus as much for the difference in d a right-hand side carries; 4 X_TOL
    max(1, |d|_inf) max(1, |x|_inf) covers both."""
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 4
    n, nC, nK = shape
    opt = hip.default_options(**OPT)
    ds1 = instances(shape, B)
    ds2 = [dict(d, Q=new_values(d, SEED + b)["Q"]) for b, d in enumerate(ds1)]
    dev = torch.device("cuda", 0) if on_device else torch.device("cpu")
    T = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=grad)
    w = T(np.random.default_rng(7).standard_normal((B, n)))
    g = T(stack(ds1, "g"))
    grads, xs, sides, iters = {}, {}, {}, {}
    for switch in (True, False):
        sb = handle(hip, ds1, opt)
        layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack(ds1, "lbA"), ubA=stack(ds1, "ubA")), values=dict(Qx=qx(ds1), Ax=ax(ds1)), warm_matrices=switch)
        assert layer.warm_matrices is switch
        layer.solve(g, Qx=T(qx(ds1)))
        assert sb.launch_counts() == (1, 1) and layer.last_path == ("device" if on_device else "host")
        it1 = sum(s["iterTotal"] for s in layer.stats)
        Q2 = T(qx(ds2), grad=True)
        x, _ = layer.solve(g, Qx=Q2)
        assert sb.launch_counts() == (2, 2)                      # warm: the setup around the kept point; cold: load + run
        st = layer.stats
        assert all(s["returnValue"] == 0 for s in st)
        iters[switch] = sum(s["iterTotal"] for s in st)
        print(f"    warm_matrices={switch}: iterates {it1} then {iters[switch]}")
        (w * x).sum().backward()
        grads[switch], xs[switch] = Q2.grad.cpu().numpy(), x.detach().cpu().numpy()
        dg, _, sides[switch], info = sb.sensitivity(w.cpu().numpy())
        assert np.all(info == 0)
        if switch:
            assert iters[True] < it1
            dmax = np.abs(dg).max()
            got = sb.read_problem(B - 1)
            assert np.array_equal(got["Qx"], ds2[B - 1]["Q"].data) and np.array_equal(got["Ax"], ds1[B - 1]["E"].data)
            if not on_device:
                assert np.array_equal(layer.values["Qx"], qx(ds2))      # the layer's copy is kept in step
        else:
            assert_same_bits(dict(x=xs[False], y=layer.y.detach().cpu().numpy() if on_device else layer.y, st=st), fresh(hip, ds2, opt))      # today's load + run
        sb.close()
    assert np.array_equal(sides[True], sides[False]) and np.abs(xs[True] - xs[False]).max() < X_TOL      # one point, one working set
    tol = 4 * X_TOL * max(1.0, dmax) * max(1.0, np.abs(xs[True]).max())
    err = np.abs(grads[True] - grads[False]).max()
    print(f"    |Qx.grad (warm) - Qx.grad (cold)| = {err:.3e}, bound {tol:.3e}")
    assert np.any(grads[True] != 0.0) and err <= tol


def test_warm_layer_needs_no_values_after_a_solve(hip):
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 4
    ds1 = instances(shape, B)
    ds2 = [new_values(d, SEED + b) for b, d in enumerate(ds1)]
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    for switch in (False, True):
        sb = handle(hip, ds1, hip.default_options(**OPT))
        layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack(ds1, "lbA"), ubA=stack(ds1, "ubA")), warm_matrices=switch)
        with pytest.raises(ValueError, match="values"):
            layer.solve(T(stack(ds1, "g")), Qx=T(qx(ds2)))      # no solve yet: a load, which needs both arrays
        layer.solve(T(stack(ds1, "g")))
        assert sb.launch_counts() == (1, 1)
        if switch:
            layer.solve(T(stack(ds1, "g")), Ax=T(ax(ds2)))
            assert sb.launch_counts() == (2, 2) and all(s["returnValue"] == 0 for s in layer.stats)
            assert np.array_equal(sb.read_problem(0)["Ax"], ds2[0]["E"].data) and np.array_equal(sb.read_problem(0)["Qx"], ds1[0]["Q"].data)
        else:
            with pytest.raises(ValueError, match="values"):
                layer.solve(T(stack(ds1, "g")), Ax=T(ax(ds2)))
        sb.close()
