"""Panel sensitivities and full solution Jacobians of the sparse arm (lcqp_hip_sparse_sensitivity_blocked, lcqp_hip_sparse_jacobian,
SparseBatchLCQPLayer.jacobian; DESIGN.md section 3a''', "The sparse arm").

1  dg, db of the blocked call against numpy on the device's own working set, the bound of check 1 of tests/test_gpu_sparse_sensitivity.py:
   max|delta| <= 1e-12 (nV + |W|) cond_2(K0) |v|_inf; side and info equal to the vector call's.
2  against the vector kernel: the same bound; whether the bits are equal is printed (asserted on the general LDL', which falls back).
3  column independence, bit for bit.   4  the Jacobian.   5  the calls change nothing.   6  state errors and a failed instance.   7  torch.

One solve per case; every call the tests compare is made on it once (solved_case).  The reference of the random vectors is the float64 LU
refined with long-double residuals; the reference inverse of check 4 is the plain float64 LU of the same matrix (error ~ eps cond, four
orders below the bound).  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest

from batch_helpers import assert_same_bits, environment, handle, kkt_reference, result, update_all
from problems import OPT, SMALL, instances, moved
from test_gpu_sparse_sensitivity import CASES as VECTOR_CASES, instances_of

pytestmark = pytest.mark.gpu

NOT_SETUP = 300
KEYS = ("small", "lanes 32", "pools of 4", "bordered circle", "mid", "small, general ldl")
CASES = {k: VECTOR_CASES[k] for k in KEYS}
FALLBACK = "small, general ldl"


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def solved_case(key):
    import lcqpow_amd as hip
    ds = instances_of(key)
    B, n = len(ds), ds[0]["nV"]
    with environment(CASES[key][1]):
        sb = handle(hip, ds, hip.default_options(**OPT))
    P = sb.sens_panel()
    engine = dict(lanes=sb.lanes(), fronts=sb.fronts(), border=sb.border(), panel=P)
    sb.run()
    x, y, st = sb.solution()
    nrhs = 5 if key == FALLBACK else 2 * P + 3
    rng = np.random.default_rng(78)
    V = rng.standard_normal((B, nrhs, n))
    V[:, 2] = 0.0                                   # a zero column
    counts = sb.launch_counts()
    vec = sb.sensitivity(V)
    blk = sb.sensitivity_blocked(V)
    c = dict(ds=ds, x=x, st=st, V=V, vec=vec, blk=blk, engine=engine, P=P)
    widths = sorted({1, 3, max(P, 1), max(P, 1) + 1} & set(range(1, nrhs + 1)))
    c["sub"] = {w: sb.sensitivity_blocked(np.ascontiguousarray(V[:, 1:1 + w])) for w in widths}
    perm = rng.permutation(nrhs)
    c["perm"] = perm
    c["permuted"] = sb.sensitivity_blocked(np.ascontiguousarray(V[:, perm]))
    c["again"] = sb.sensitivity_blocked(V)
    # the Jacobian: unchunked, a sub-range, one item per launch, a cap that leaves a partial last chunk
    c["jac"] = sb.jacobian()
    c["jac_ms"] = sb.sensitivity_kernel_ms()
    c["eye"] = sb.sensitivity_blocked(np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n))))
    c["jac_range"] = sb.jacobian(first=1, count=min(2, B - 1))
    c["jac_one"] = sb.jacobian(_staging_bytes=1)
    m = sb.m
    items = B * (-(-n // P)) if P else n
    item_bytes = 8 * (P * (n + m) + P * (sb.nV + m + 64 + 2 * n + m)) if P else 8 * B * (2 * n + m)      # an upper estimate of one item's staging
    per_chunk = max(2, (items + 2) // 3 + 1)
    c["partial"] = (items, per_chunk)
    c["jac_partial"] = sb.jacobian(_staging_bytes=item_bytes * per_chunk)
    assert sb.launch_counts() == counts
    sb.close()
    return c


@functools.lru_cache(maxsize=None)
def reference_of(key):
    c = solved_case(key)
    out = []
    for b, d in enumerate(c["ds"]):
        E = d["E"].toarray()
        W = np.flatnonzero(c["vec"][2][b])
        dgr, mu, cond = kkt_reference(d["Q"].toarray(), E[W], c["V"][b].T, extended=True)
        n = d["nV"]
        K = np.zeros((n + len(W),) * 2); K[:n, :n] = d["Q"].toarray(); K[:n, n:] = E[W].T; K[n:, :n] = E[W]
        Kinv = np.linalg.solve(K, np.eye(n + len(W)))
        out.append(dict(E=E, W=W, dg=np.asarray(dgr.T, dtype=np.float64), mu=np.asarray(mu.T, dtype=np.float64), cond=cond, Kinv=Kinv))
    return out


def bound_of(c, r, b, vinf):
    return 1e-12 * (c["ds"][b]["nV"] + len(r["W"])) * r["cond"] * vinf


def test_the_cases_reach_the_engines(hip):
    eng = {k: solved_case(k)["engine"] for k in KEYS}
    print(" ", eng)
    assert eng["small"]["lanes"] == 8 and eng["lanes 32"]["lanes"] == 32 and eng["bordered circle"]["border"] > 0
    assert all(eng[k]["panel"] in (4, 8) for k in KEYS if k != FALLBACK)
    assert eng[FALLBACK]["fronts"] > 0 and eng[FALLBACK]["panel"] == 0


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    dg, db, side, info = c["blk"]
    nrhs, m = c["V"].shape[1], side.shape[1]
    assert np.array_equal(side, c["vec"][2]) and np.array_equal(info, c["vec"][3])
    worst = 0.0
    for b, r in enumerate(refs):
        assert c["st"][b]["returnValue"] == 0 and not (info[b] & 1)
        bound = bound_of(c, r, b, np.abs(c["V"][b]).max())
        dbr = np.zeros((nrhs, m)); dbr[:, r["W"]] = r["mu"]
        e_g, e_b = np.abs(dg[b] - r["dg"]).max(), np.abs(db[b] - dbr).max()
        worst = max(worst, max(e_g, e_b) / bound)
        print(f"  {key} instance {b}: nrhs {nrhs}, |W| = {len(r['W'])}, cond(K0) = {r['cond']:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {bound:.3g}, info {info[b]}")
        assert e_g <= bound and e_b <= bound
    print(f"  {key}: worst error / bound = {worst:.3g}")


# ---- 2: against the vector kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_against_the_vector_kernel(hip, key):
    c, refs = solved_case(key), reference_of(key)
    for b, r in enumerate(refs):
        bound = bound_of(c, r, b, np.abs(c["V"][b]).max())
        e_g = np.abs(c["blk"][0][b] - c["vec"][0][b]).max(); e_b = np.abs(c["blk"][1][b] - c["vec"][1][b]).max()
        print(f"  {key} instance {b}: max|blocked - vector| dg {e_g:.3g} db {e_b:.3g} (bound {bound:.3g})")
        assert e_g <= bound and e_b <= bound
    equal = same(c["blk"][:2], c["vec"][:2])
    print(f"  {key}: the bits of the blocked call equal the vector kernel's: {equal}")
    if key == FALLBACK:
        assert equal


# ---- 3: column independence, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_column_independence(hip, key):
    c = solved_case(key)
    dg, db, side, info = c["blk"]
    print(f"  {key}: panel {c['P']}, widths {sorted(c['sub'])}")
    for w, got in c["sub"].items():
        assert np.array_equal(got[0], dg[:, 1:1 + w]) and np.array_equal(got[1], db[:, 1:1 + w]), w
        assert np.array_equal(got[2], side) and np.array_equal(got[3], info)
    assert np.array_equal(c["permuted"][0], dg[:, c["perm"]]) and np.array_equal(c["permuted"][1], db[:, c["perm"]])
    assert np.all(dg[:, 2] == 0.0) and np.all(db[:, 2] == 0.0) and np.any(dg[:, 1] != 0.0)
    assert same(c["again"], c["blk"])


# ---- 4: the Jacobian ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_jacobian(hip, key):
    c, refs = solved_case(key), reference_of(key)
    Jg, Jb, side, info = c["jac"]
    B, n, m = Jg.shape[0], Jg.shape[1], side.shape[1]
    assert Jb.shape == (B, n, m) and np.array_equal(side, c["vec"][2]) and np.array_equal(info, c["vec"][3])
    assert np.array_equal(Jg, c["eye"][0]) and np.array_equal(Jb, c["eye"][1])
    for b, r in enumerate(refs):
        bound = bound_of(c, r, b, 1.0)
        sym = np.abs(Jg[b] - Jg[b].T).max()
        feas = np.abs(r["E"][r["W"]] @ Jg[b]).max(initial=0.0)
        Jbr = np.zeros((n, m)); Jbr[:, r["W"]] = r["Kinv"][:n, n:]
        e_g, e_b = np.abs(Jg[b] + r["Kinv"][:n, :n]).max(), np.abs(Jb[b] - Jbr).max()
        print(f"  {key} instance {b}: asymmetry {sym:.3g}, |E_W Jg| {feas:.3g}, err Jg {e_g:.3g}, err Jb {e_b:.3g}, bound {bound:.3g}")
        assert sym <= bound and feas <= bound and e_g <= bound and e_b <= bound
    k = min(2, B - 1)
    assert same(c["jac_range"], (Jg[1:1 + k], Jb[1:1 + k], side[1:1 + k], info[1:1 + k]))
    print(f"  {key}: {c['partial'][0]} work items; chunks of 1 and of at most {c['partial'][1]}; kernel time {c['jac_ms']:.3f} ms")
    assert same(c["jac_one"], c["jac"]) and same(c["jac_partial"], c["jac"])
    assert c["jac_ms"] > 0.0


# ---- 5: no side effects ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "bordered circle"])
@pytest.mark.parametrize("warm", [True, False])
def test_the_calls_change_nothing(hip, case, warm):
    ds = instances_of(case)
    if case == "bordered circle":
        ds2 = [dict(d, g=d["g"] * (1.0 + 0.02 * np.random.default_rng(300 + b).standard_normal(d["nV"]))) for b, d in enumerate(ds)]
    else:
        ds2 = [moved(d, 300 + b) for b, d in enumerate(ds)]
    opt = hip.default_options(**OPT)
    V = np.random.default_rng(1).standard_normal((len(ds), 11, ds[0]["nV"]))
    out = []
    for with_calls in (True, False):
        with environment(CASES[case][1]):
            sb = handle(hip, ds, opt)
        sb.run()
        first = result(sb)
        if with_calls:
            counts = sb.launch_counts()
            before = sb.sensitivity(V)
            assert np.any(sb.jacobian()[0] != 0.0)
            assert np.any(sb.sensitivity_blocked(V)[0] != 0.0)
            assert same(sb.sensitivity(V), before)      # the pools the vector kernel borrows were not disturbed
            assert sb.launch_counts() == counts
            assert_same_bits(first, result(sb))
        update_all(sb, ds2)
        sb.resolve(warm=warm)
        out.append(result(sb))
        assert sb.launch_counts() == (1, 2)
        sb.close()
    assert_same_bits(out[0], out[1])


# ---- 6: state errors and a failed instance ---------------------------------------------------------------------------------------------
def test_state_errors(hip):
    L = hip.lib()
    ds = instances(SMALL, 2)
    n = SMALL[0]
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.ones((2, n)); dg = np.full((2, n), 7.0); Jg = np.full((2, n, n), 7.0)
    d = ds[0]
    sb = hip.SparseBatchLCQP(2, d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(**OPT))
    blocked = lambda: L.lcqp_hip_sparse_sensitivity_blocked(sb.h, 1, v.ctypes.data_as(dp), dg.ctypes.data_as(dp), None, None, None)
    jac = lambda: L.lcqp_hip_sparse_jacobian(sb.h, 0, 2, Jg.ctypes.data_as(dp), None, None, None)
    load = lambda: sb.load(0, 2, np.stack([q["Q"].data for q in ds]), np.stack([q["g"] for q in ds]), np.stack([q["E"].data for q in ds]),
                           lbA=np.stack([q["lbA"] for q in ds]), ubA=np.stack([q["ubA"] for q in ds]))
    assert blocked() == NOT_SETUP and jac() == NOT_SETUP      # before anything
    assert load() == 0
    assert blocked() == NOT_SETUP and jac() == NOT_SETUP and np.all(dg == 7.0) and np.all(Jg == 7.0)
    sb.run()
    assert blocked() == 0 and jac() == 0 and not np.any(dg == 7.0) and not np.any(Jg == 7.0)
    assert L.lcqp_hip_sparse_jacobian(sb.h, 1, 2, Jg.ctypes.data_as(dp), None, None, None) == 100      # first + count > B
    assert load() == 0                                        # a load since the last solve
    assert blocked() == NOT_SETUP and jac() == NOT_SETUP
    with pytest.raises(RuntimeError, match="300"):
        sb.jacobian()
    sb.close()


def test_flag_of_a_failed_instance(hip):
    """Instance 4 gets a NaN in g: its run ends with 203 (tests/test_gpu_sparse_sensitivity.py).  info = 1 and zero rows for it, the bits of
    the clean batch for its neighbours."""
    c = solved_case("small")
    ds = list(c["ds"])
    bad = 4
    g = ds[bad]["g"].copy(); g[0] = np.nan
    ds[bad] = dict(ds[bad], g=g)
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    st = sb.solution()[2]
    Jg, Jb, side, info = sb.jacobian()
    dg, db, side2, info2 = sb.sensitivity_blocked(c["V"])
    sb.close()
    print("  return values", [s["returnValue"] for s in st], "info", info)
    assert st[bad]["returnValue"] == 203 and info[bad] == 1 and info2[bad] == 1
    assert np.all(Jg[bad] == 0.0) and np.all(Jb[bad] == 0.0) and np.all(side[bad] == 0) and np.all(dg[bad] == 0.0) and np.all(db[bad] == 0.0)
    for b in range(len(ds)):
        if b != bad:
            assert st[b]["returnValue"] == 0 and info[b] == c["jac"][3][b]
            assert np.array_equal(Jg[b], c["jac"][0][b]) and np.array_equal(Jb[b], c["jac"][1][b]) and np.array_equal(side[b], c["jac"][2][b])
            assert np.array_equal(dg[b], c["blk"][0][b]) and np.array_equal(db[b], c["blk"][1][b])


# ---- 7: torch ------------------------------------------------------------------------------------------------------------------------
def test_torch_layer_jacobian(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 3
    n = shape[0]
    ds = instances(shape, B)
    stack = lambda k: np.stack([d[k] for d in ds])
    sb = handle(hip, ds, hip.default_options(**OPT))
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack("lbA"), ubA=stack("ubA")))
    g = torch.tensor(stack("g"), dtype=torch.float64, requires_grad=True)
    x = layer(g)
    J = layer.jacobian(serial=layer.solves)
    assert J.shape == (B, n, n) and J.dtype == torch.float64 and np.all(layer.info == 0)
    side = sb.sensitivity(np.ones((B, n)))[2]
    refs = []
    for b, d in enumerate(ds):
        W = np.flatnonzero(side[b])
        refs.append(kkt_reference(d["Q"].toarray(), d["E"].toarray()[W], np.eye(n)[:, :1], extended=False)[2] * 1e-12 * (n + len(W)))
    for k in (0, 7, n - 1):      # dx_k/dg: the gradient of x[:, k] by backward
        g.grad = None
        x[:, k].sum().backward(retain_graph=True)
        err = np.abs(g.grad.numpy() - J[:, k, :].numpy()).max(axis=1)
        print(f"  row {k}: max|autograd - jacobian| {err}, bound {refs}")
        assert np.all(err <= np.array(refs))
    with torch.no_grad():
        layer(g.detach() * 1.01)
    with pytest.raises(RuntimeError, match="not the layer's last one"):
        layer.jacobian(serial=1)
    sb.close()
