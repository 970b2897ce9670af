"""The panel form of the general sparse LDL' (lcqp_hip_sparse_set_general_panel; sp_general_solve_panel under
k_sparse_sensitivity_blk_general; DESIGN.md section 3a''', "The general engine"): lcqp_hip_sparse_sensitivity_blocked and
lcqp_hip_sparse_jacobian on a handle of the general engine that switched it on.

Three cases, one per class of front the panel sweep distinguishes (asserted through max_front()):
  a  "small, general ldl" of tests/test_gpu_sparse_sensitivity.py: (64, 32, 8), B = 6 under LCQP_SPARSE_GENERAL=1 -- largest front 60: every front <= 64
  b  "grid, general ldl": the 44 x 44 grid, B = 2 -- largest front 95 (9 of its 179 fronts lie in (64, 256])
  c  coupled_lcqp below: a tridiagonal Q with a symmetric dense block on 300 of its 420 variables, B = 2 -- the block is one front of 300
     rows, the other 14 fronts are <= 64 (found on the CPU with the analysis of lcqp_sparse_pattern.hpp / lcqp_sparse_general.hpp)

1  dg, db of the switched-on blocked call against numpy on the device's own working set: max|delta| <= 1e-12 (nV + |W|) cond_2(K0) |v|_inf
   (kkt_reference: float64 LU refined with long-double residuals); side and info equal to the vector call's, info = 0.
2  against the vector kernel, the same bound; whether the bits are equal is printed.   3  column independence, bit for bit.
4  the Jacobian.   5  the calls change nothing (a, b).   6  switching off again.   7  a failed instance.   8  state errors.   9  torch.

One solve per case; every call the tests compare is made on it once (solved_case).  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest

from batch_helpers import assert_same_bits, environment, handle, kkt_reference, result, update_all
from problems import OPT, SMALL, instances, moved
from test_gpu_sparse_sensitivity import CASES as VECTOR_CASES, instances_of

pytestmark = pytest.mark.gpu

NOT_SETUP, INVALID = 300, 100
PANEL = 8                     # LCQP_SPARSE_SENS_PANEL
KEYS = ("a", "b", "c")
VECTOR_KEY = {"a": "small, general ldl", "b": "grid, general ldl"}
FRONT_CLASS = {"a": (1, 64), "b": (65, 256), "c": (257, 576)}      # (c: up to GEN_MAX_FRONT)


def coupled_lcqp(n=420, nd=300, nK=12, nC=16, seed=5):
    """A tridiagonal Hessian with a symmetric dense coupling block on the variables [c0, c0 + nd): the block is a clique of the KKT graph, so
    some front of any elimination holds all of it -- with these parameters the largest front is exactly the 300 rows of the block.  Diagonally
    dominant (diagonal in [3, 4], two off-diagonals of -1, block rows of 1-norm <= 1); complementarity pairs and rows of A between near
    neighbours, as in problems.grid_lcqp."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    c0 = (n - nd) // 2
    Qd = np.zeros((n, n))
    M = rng.uniform(-1, 1, (nd, nd))
    Qd[c0:c0 + nd, c0:c0 + nd] = (M + M.T) * (0.5 / nd)
    Qd += np.diag(3.0 + rng.uniform(0, 1, n))
    for i in range(n - 1):
        Qd[i, i + 1] = Qd[i + 1, i] = -1.0
    xs = rng.uniform(-1, 1, n)
    Lm = np.zeros((nK, n)); Rm = np.zeros((nK, n))
    for k in range(nK):      # pairs of neighbours at the two ends of the chain
        i = 2 * k if k < nK // 2 else n - 2 - 2 * (k - nK // 2)
        Lm[k, i] = 1.0; Rm[k, i + 1] = 1.0
        if rng.random() < 0.5: xs[i], xs[i + 1] = 0.0, rng.uniform(0, 1)
        else: xs[i], xs[i + 1] = rng.uniform(0, 1), 0.0
    A = np.zeros((nC, n))
    for k in range(nC):
        i = int(rng.integers(0, n - 3))
        A[k, i] = rng.uniform(0.5, 1.5); A[k, i + 3] = rng.uniform(-1.5, -0.5)
    ax = A @ xs
    Q = sp.csc_matrix(Qd); E = sp.csc_matrix(np.vstack([A, Lm, Rm]))
    Q.sort_indices(); E.sort_indices()
    return dict(nV=n, nC=nC, nComp=nK, Q=Q, E=E, g=rng.uniform(-2, 2, n), lbA=ax - rng.uniform(0.1, 1, nC), ubA=ax + rng.uniform(0.1, 1, nC))


def case_of(key):
    """(instances, environment of the handle's creation)"""
    if key == "c":
        d = coupled_lcqp()
        return [d, moved(d, 11)], {}
    return instances_of(VECTOR_KEY[key]), VECTOR_CASES[VECTOR_KEY[key]][1]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def solved_case(key):
    import lcqpow_amd as hip
    ds, env = case_of(key)
    B, n = len(ds), ds[0]["nV"]
    with environment(env):
        sb = handle(hip, ds, hip.default_options(**OPT))
    engine = dict(lanes=sb.lanes(), fronts=sb.fronts(), max_front=sb.max_front(), panel_off=sb.sens_panel())
    sb.run()
    x, y, st = sb.solution()
    P = PANEL
    nrhs = 2 * P + 3                                # two full panels and a ragged one
    rng = np.random.default_rng(79)
    V = rng.standard_normal((B, nrhs, n))
    V[:, 2] = 0.0                                   # a zero column
    counts = sb.launch_counts()
    vec = sb.sensitivity(V)
    off = sb.sensitivity_blocked(V)                 # the default: the vector kernel
    sb.set_general_panel(True)
    engine["panel_on"] = sb.sens_panel()
    blk = sb.sensitivity_blocked(V)
    c = dict(ds=ds, x=x, st=st, V=V, vec=vec, off=off, blk=blk, engine=engine, P=P)
    c["sub"] = {w: sb.sensitivity_blocked(np.ascontiguousarray(V[:, 1:1 + w])) for w in (1, 3, P, P + 1)}
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
    items = B * (-(-n // P))
    Np = -(-(n + m) // 64) * 64
    item_bytes = 8 * (P * (n + m) + P * (Np + 2 * n + m))              # one item's staging as sp_panel_run sizes it: outputs + workspace
    per_chunk = max(2, (items + 2) // 3 + 1)                            # the cap below holds exactly per_chunk items
    assert per_chunk < items and items % per_chunk != 0, (items, per_chunk)      # several chunks, the last one partial
    c["partial"] = (items, per_chunk)
    c["jac_partial"] = sb.jacobian(_staging_bytes=item_bytes * per_chunk)
    c["vec_after"] = sb.sensitivity(V)
    # 6: off again
    sb.set_general_panel(False)
    c["panel_off_again"] = sb.sens_panel()
    c["off_again"] = sb.sensitivity_blocked(V)
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


@pytest.mark.parametrize("key", KEYS)
def test_the_case_reaches_its_class_and_the_switch_sets_the_panel(hip, key):
    eng = solved_case(key)["engine"]
    print(f"  {key}: {eng}")
    lo, hi = FRONT_CLASS[key]
    assert eng["lanes"] == 64 and eng["fronts"] > 0 and lo <= eng["max_front"] <= hi
    assert eng["panel_off"] == 0 and eng["panel_on"] == PANEL


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    dg, db, side, info = c["blk"]
    nrhs, m = c["V"].shape[1], side.shape[1]
    assert np.array_equal(side, c["vec"][2]) and np.array_equal(info, c["vec"][3])
    worst = 0.0
    for b, r in enumerate(refs):
        assert c["st"][b]["returnValue"] == 0 and info[b] == 0
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
        print(f"  {key} instance {b}: max|panel - vector| dg {e_g:.3g} db {e_b:.3g} (bound {bound:.3g})")
        assert e_g <= bound and e_b <= bound
    print(f"  {key}: the bits of the panel form equal the vector kernel's: {same(c['blk'][:2], c['vec'][:2])}")


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
    print(f"  {key}: {c['partial'][0]} work items; chunks of 1 and of {c['partial'][1]} with a last chunk of {c['partial'][0] % c['partial'][1]}; kernel time {c['jac_ms']:.3f} ms")
    assert same(c["jac_one"], c["jac"]) and same(c["jac_partial"], c["jac"])
    assert c["jac_ms"] > 0.0


# ---- 5: no side effects ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["a", "b"])
@pytest.mark.parametrize("warm", [True, False])
def test_the_calls_change_nothing(hip, key, warm):
    ds, env = case_of(key)
    ds2 = [moved(d, 300 + b) for b, d in enumerate(ds)]
    opt = hip.default_options(**OPT)
    V = np.random.default_rng(1).standard_normal((len(ds), 11, ds[0]["nV"]))
    out = []
    for with_calls in (True, False):
        with environment(env):
            sb = handle(hip, ds, opt)
        sb.run()
        first = result(sb)
        if with_calls:
            counts = sb.launch_counts()
            before = sb.sensitivity(V)
            sb.set_general_panel(True)
            assert sb.sens_panel() == PANEL
            assert np.any(sb.jacobian(count=1)[0] != 0.0)
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


# ---- 6: switching off again ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_switching_off_restores_the_vector_kernel(hip, key):
    c = solved_case(key)
    print(f"  {key}: sens_panel() after the switch went off: {c['panel_off_again']}")
    assert c["panel_off_again"] == 0
    assert same(c["off"], c["vec"]) and same(c["off_again"], c["vec"]) and same(c["vec_after"], c["vec"])


# ---- 7: a failed instance --------------------------------------------------------------------------------------------------------------
def test_flag_of_a_failed_instance(hip):
    """Instance 4 of case a gets a NaN in g: its run ends with 203 (tests/test_gpu_sparse_sensitivity.py).  info = 1 and zero rows for it, the
    bits of the clean batch for its neighbours."""
    c = solved_case("a")
    ds = list(c["ds"])
    bad = 4
    g = ds[bad]["g"].copy(); g[0] = np.nan
    ds[bad] = dict(ds[bad], g=g)
    with environment(case_of("a")[1]):
        sb = handle(hip, ds, hip.default_options(**OPT))
    sb.set_general_panel(True)
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


# ---- 8: state errors ---------------------------------------------------------------------------------------------------------------------
def test_state_errors(hip):
    L = hip.lib()
    ds = instances(SMALL, 2)
    n = SMALL[0]
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.ones((2, n)); dg = np.full((2, n), 7.0); Jg = np.full((2, n, n), 7.0)
    d = ds[0]
    with environment({"LCQP_SPARSE_GENERAL": "1"}):
        sb = hip.SparseBatchLCQP(2, d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(**OPT))
    assert sb.fronts() > 0 and sb.sens_panel() == 0
    assert L.lcqp_hip_sparse_set_general_panel(sb.h, 2) == INVALID and L.lcqp_hip_sparse_set_general_panel(sb.h, -1) == INVALID
    assert sb.sens_panel() == 0                                # a refused call switched nothing
    with pytest.raises(ValueError):
        sb.set_general_panel(2)
    assert L.lcqp_hip_sparse_set_general_panel(sb.h, 1) == 0 and sb.sens_panel() == PANEL
    blocked = lambda: L.lcqp_hip_sparse_sensitivity_blocked(sb.h, 1, v.ctypes.data_as(dp), dg.ctypes.data_as(dp), None, None, None)
    jac = lambda: L.lcqp_hip_sparse_jacobian(sb.h, 0, 2, Jg.ctypes.data_as(dp), None, None, None)
    load = lambda: sb.load(0, 2, np.stack([q["Q"].data for q in ds]), np.stack([q["g"] for q in ds]), np.stack([q["E"].data for q in ds]),
                           lbA=np.stack([q["lbA"] for q in ds]), ubA=np.stack([q["ubA"] for q in ds]))
    assert blocked() == NOT_SETUP and jac() == NOT_SETUP      # before anything
    assert load() == 0
    assert blocked() == NOT_SETUP and jac() == NOT_SETUP and np.all(dg == 7.0) and np.all(Jg == 7.0)
    sb.run()
    assert blocked() == 0 and jac() == 0 and not np.any(dg == 7.0) and not np.any(Jg == 7.0)
    assert L.lcqp_hip_sparse_set_general_panel(sb.h, 0) == 0 and L.lcqp_hip_sparse_set_general_panel(sb.h, 1) == 0
    assert blocked() == 0                                     # the switch does not touch the mark of the last solve
    assert load() == 0                                        # a load since the last solve
    assert blocked() == NOT_SETUP and jac() == NOT_SETUP
    with pytest.raises(RuntimeError, match="300"):
        sb.jacobian()
    sb.close()


def test_the_switch_does_nothing_on_a_band_engine(hip):
    ds = instances(SMALL, 3)
    sb = handle(hip, ds, hip.default_options(**OPT))
    assert sb.fronts() == 0 and sb.max_front() == 0
    P = sb.sens_panel()
    sb.run()
    V = np.random.default_rng(5).standard_normal((3, P + 2, SMALL[0]))
    before, jac = sb.sensitivity_blocked(V), sb.jacobian()
    for on in (True, False):
        sb.set_general_panel(on)
        assert sb.sens_panel() == P
        assert same(sb.sensitivity_blocked(V), before) and same(sb.jacobian(), jac)
    sb.close()


# ---- 9: torch --------------------------------------------------------------------------------------------------------------------------
def test_torch_layer_jacobian(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 3
    n = shape[0]
    ds = instances(shape, B)
    stack = lambda k: np.stack([d[k] for d in ds])
    with environment({"LCQP_SPARSE_GENERAL": "1"}):
        sb = handle(hip, ds, hip.default_options(**OPT))
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack("lbA"), ubA=stack("ubA")), general_panel=True)
    assert sb.fronts() > 0 and sb.sens_panel() == PANEL
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
    sb.close()
