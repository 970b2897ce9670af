"""Warm re-solves of a dense batch after a change of the MATRICES (lcqp_hip_batch_update_matrices / _update_matrices_device, then
lcqp_hip_batch_resolve; DESIGN.md section 3a, "New matrices").

The warm re-solve is held to the CPU oracle asked for the same thing in the reference's own terms on the new data -- x0, y0 = its solution
of the old data, solveZeroPenaltyFirst = 0, initialPenaltyParameter = its last rhoOpt -- with assert_parity of tests/test_gpu_resolve.py as it
stands; the inverse factor the resolve leaves to the checker of tests/test_gpu_setup.py on the NEW setup (a factor left over from the old
matrices can still converge: the polish refines through exact residuals); the cold re-solve and every refusal to the BITS of a fresh batch
object.  The data: tests/problems.py::random_lcqp from default_rng(7); the matrices move by the 2 % recipe of new_matrices(), the vectors by
perturbed().  The device sequence and the oracle's answers of a shape are made once and shared by the tests that need them."""
import ctypes

import numpy as np
import pytest
import torch      # noqa: F401 -- before the library is first loaded: the device twin needs the library and torch on one HIP runtime

import problems as P
import test_gpu_setup as S
from batch_helpers import assert_same_bits, load_all, result, stack, update_all
from problems import perturbed, random_lcqp
from test_gpu_resolve import X_TOL, Y_TOL, assert_parity, fresh, oracle_cold, oracle_warm

pytestmark = pytest.mark.gpu

# (n, nC, nComp, B, box, shifted): np = 128 with and without box rows, np = 256, np = 384 (the row state of the subsolver is not in LDS),
# and more than three workgroups per CU (the other build of the homotopy kernel)
SHAPES = ((40, 20, 8, 12, True, False), (64, 128, 16, 12, False, False), (129, 70, 20, 6, True, False), (300, 100, 40, 2, False, False),
          (40, 20, 8, 800, False, False))
IDS = ["%dx%dx%d-B%d" % s[:4] for s in SHAPES]
MATS = ("Q", "L", "R", "A")
DISTINCT = 24      # B = 800: instance b holds problem b % DISTINCT -- the oracle solves each problem once
FACTORS = 12       # instances per shape whose inverse factor is read back and checked


def new_matrices(d, seed, eps=0.02):
    """the 2 % recipe for the matrices: Q scaled symmetrically, every entry of A, every row of L and of R; drawn in that order"""
    rng = np.random.default_rng(seed)
    n, nC, nComp = d["nV"], d["nC"], d["nComp"]
    s = 1.0 + eps * rng.standard_normal(n)
    Q = d["Q"] * np.outer(s, s)
    A = d["A"] * (1.0 + eps * rng.standard_normal((nC, n)))
    L = d["L"] * (1.0 + eps * rng.standard_normal((nComp, 1)))
    R = d["R"] * (1.0 + eps * rng.standard_normal((nComp, 1)))
    return dict(d, Q=Q, A=A, L=L, R=R)


_data, _scene, _same = {}, {}, {}


def data(shape):
    """(old data, new data) of the distinct problems of a shape"""
    if shape not in _data:
        n, nC, nComp, B, box, shifted = shape
        rng = np.random.default_rng(7)
        ds1 = [random_lcqp(rng, n, nC, nComp, box, shifted) for _ in range(min(B, DISTINCT))]
        _data[shape] = (ds1, [perturbed(new_matrices(d, 500 + b), 100 + b) for b, d in enumerate(ds1)])
    return _data[shape]


def spread(ds, B):
    return [ds[b % len(ds)] for b in range(B)]


def options(hip, **kw):
    return hip.default_options(perturbStep=0, printLevel=0, **kw)


def make(hip, shape, **kw):
    n, nC, nComp, B, box = shape[:5]
    return hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=options(hip, **kw))


def update_matrices_all(bt, ds, first=0, only=MATS):
    rc = bt.update_matrices(first, len(ds), **{k: stack(ds, k) for k in only})
    assert rc == 0, (rc, bt._last_error())


def factors(bt, ds):
    """(working set, setup, Q, E) of the first FACTORS instances"""
    out = []
    for b in range(min(bt.B, FACTORS)):
        d = ds[b]
        out.append((bt.read_working_set(b), bt.read_setup(b), d["Q"], S.stacked_rows(d, d.get("lb"), d.get("ub"))))
    return out


def scene(hip, oracle, shape):
    """run on the old data, new matrices and vectors (in either order), resolve(warm=True); beside it the oracle's warm solve of the new
    data and a cold run of the new data on the device"""
    if shape not in _scene:
        B = shape[3]
        d1, d2 = data(shape)
        ds1, ds2 = spread(d1, B), spread(d2, B)
        bt = make(hip, shape)
        load_all(bt, ds1)
        bt.run()
        _, _, st1 = bt.solution()
        if SHAPES.index(shape) % 2:
            update_all(bt, ds2); update_matrices_all(bt, ds2)
        else:
            update_matrices_all(bt, ds2); update_all(bt, ds2)
        bt.resolve(warm=True)
        x, y, st = bt.solution()
        out = dict(st1=st1, x=x, y=y, st=st, counts=bt.launch_counts(), timing=bt.last_timing(), factors=factors(bt, ds2), ds2=ds2)
        bt.close()
        out["cold"] = fresh(hip, ds2, options(hip))["st"]
        ref = oracle_warm(oracle, d2, oracle_cold(oracle, d1))
        out["ref"] = spread(ref, B)
        _scene[shape] = out
    return _scene[shape]


def same_scene(hip, shape):
    """run, the SAME matrices sent again, resolve(warm=True)"""
    if shape not in _same:
        B = shape[3]
        ds1 = spread(data(shape)[0], B)
        bt = make(hip, shape)
        load_all(bt, ds1)
        bt.run()
        x1, y1, st1 = bt.solution()
        update_matrices_all(bt, ds1)
        bt.resolve(warm=True)
        x, y, st = bt.solution()
        _same[shape] = dict(x1=x1, y1=y1, st1=st1, x=x, y=y, st=st, counts=bt.launch_counts(), factors=factors(bt, ds1))
        bt.close()
    return _same[shape]


# ---- 1: against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_warm_resolve_on_new_matrices_against_the_oracle(hip, oracle, shape):
    s = scene(hip, oracle, shape)
    assert all(v["returnValue"] == 0 for v in s["st1"])
    assert s["counts"] == (2, 2)                                   # a second full setup, a second homotopy launch
    assert s["timing"][0] > 0 and s["timing"][1] > 0
    warm, cold = sum(v["iterTotal"] for v in s["st"]), sum(v["iterTotal"] for v in s["cold"])
    print(f"  iterates of the batch: warm {warm}, cold {cold}; oracle warm {sum(r['stats']['iterTotal'] for r in s['ref'])}")
    assert_parity(s["st"], s["x"], s["y"], s["ref"], s["ds2"])
    assert all(v["returnValue"] == 0 for v in s["cold"])
    assert 2 * warm <= cold


# ---- 2: no row of the old inverse factor survives -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_inverse_factor_belongs_to_the_new_setup(hip, oracle, shape):
    for ws, rs, Q, E in scene(hip, oracle, shape)["factors"]:
        assert ws["nT"] > 0
        S.check_working_set(ws, rs, Q, E)
    for ws, rs, Q, E in same_scene(hip, shape)["factors"]:
        assert ws["nT"] > 0
        S.check_working_set(ws, rs, Q, E)


# ---- 3: the same matrices, one iterate ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_same_matrices_are_one_iterate(hip, shape):
    s = same_scene(hip, shape)
    assert s["counts"] == (2, 2)
    for k in range(shape[3]):
        assert s["st1"][k]["returnValue"] == s["st"][k]["returnValue"] == 0, k
        assert s["st"][k]["iterTotal"] == 1, (k, s["st"][k])
        assert np.abs(s["x"][k] - s["x1"][k]).max() < X_TOL and np.abs(s["y"][k] - s["y1"][k]).max() < Y_TOL, k


# ---- 4: a cold re-solve is a fresh solve, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_cold_resolve_on_new_matrices_is_a_fresh_solve(hip, shape):
    B = shape[3]
    trace = B <= 12 and shape[0] <= 64
    d1, d2 = data(shape)
    ds1, ds2 = spread(d1, B), spread(d2, B)
    kw = dict(storeSteps=1) if trace else {}
    bt = make(hip, shape, **kw)
    load_all(bt, ds1)
    bt.run()
    update_matrices_all(bt, ds2); update_all(bt, ds2)
    bt.resolve(warm=False)
    again = result(bt, trace)
    assert bt.launch_counts() == (2, 2)
    for b in range(min(B, 3)):                                      # the pools hold the matrices of the new data
        got = bt.read_problem(b)
        assert all(np.array_equal(got[k], ds2[b][k]) for k in MATS), b
    bt.close()
    ref = fresh(hip, ds2, options(hip, **kw), trace=trace)
    assert_same_bits(again, ref)
    assert np.array_equal(again["work"], ref["work"])


# ---- 5: the device twin ----------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


@pytest.mark.parametrize("shared", [(), ("Q", "A")], ids=["per-instance", "Q-A-shared"])
def test_device_twin_leaves_the_bits_of_the_host_call(hip, shared, shape=SHAPES[0]):
    B = shape[3]
    d1, d2 = data(shape)
    ds1 = spread(d1, B)
    ds2 = [dict(d, **{k: d2[0][k] for k in shared}) for d in spread(d2, B)]
    a, b = make(hip, shape), make(hip, shape)
    for bt in (a, b):
        load_all(bt, ds1)
        bt.run()
    update_matrices_all(a, ds2); update_all(a, ds2)
    rc = b.update_matrices_device(0, B, **{k: dev(ds2[0][k] if k in shared else stack(ds2, k)) for k in MATS},
                                  shared=sum({"Q": 1, "A": 2}[k] for k in shared))
    assert rc == 0, (rc, b._last_error())
    update_all(b, ds2)
    for bt in (a, b):
        bt.resolve(warm=True)
    assert_same_bits(result(a), result(b))
    assert a.launch_counts() == b.launch_counts() == (2, 2)
    for i in range(B):
        pa, pb = a.read_problem(i), b.read_problem(i)
        assert all(np.array_equal(pa[k], pb[k]) for k in pa), i
        assert all(np.array_equal(pa[k], ds2[i][k]) for k in MATS), i
        sa, sb = a.read_setup(i), b.read_setup(i)
        assert all(np.array_equal(sa[k], sb[k]) for k in sa), i
    # NULL keeps a matrix: Q and R alone, on both paths, from the state above
    ds3 = [dict(d, Q=d["Q"] + 0.125 * np.eye(d["nV"]), R=1.5 * d["R"]) for d in ds2]
    update_matrices_all(a, ds3, only=("Q", "R"))
    assert b.update_matrices_device(0, B, Q=dev(stack(ds3, "Q")), R=dev(stack(ds3, "R"))) == 0
    for i in range(B):
        pa, pb = a.read_problem(i), b.read_problem(i)
        assert all(np.array_equal(pa[k], pb[k]) for k in pa), i
        assert all(np.array_equal(pa[k], ds3[i][k]) for k in MATS), i          # A and L of ds3 are those of ds2
    a.close(); b.close()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_torch_layer_takes_the_warm_path(hip, on_device, shape=SHAPES[1]):
    """BatchLCQPLayer(warm_matrices=True).solve with matrices on a solved layer: update_matrices + update + resolve(warm), to the bits of
    those calls on a second batch; the default layer loads and runs cold.  The backward of the warm solve is the adjoint of the batch."""
    from lcqpow_amd.diff import BatchLCQPLayer
    n, nC, nComp, B = shape[:4]
    d1, d2 = data(shape)
    ds1, ds2 = spread(d1, B), spread(d2, B)
    T = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, requires_grad=grad, device="cuda:0" if on_device else "cpu")
    rows = lambda ds: dict(lbA=T(stack(ds, "lbA")), ubA=T(stack(ds, "ubA")))
    ref = make(hip, shape)
    load_all(ref, ds1)
    ref.run()
    update_matrices_all(ref, ds2, only=("Q", "A")); update_all(ref, ds2)
    ref.resolve(warm=True)
    want = result(ref)
    out = {}
    for warm in (True, False):
        bt = make(hip, shape)
        load_all(bt, ds1)
        layer = BatchLCQPLayer(bt, warm_matrices=warm)
        layer.solve(T(stack(ds1, "g")), **rows(ds1))
        Q = T(stack(ds2, "Q"), True)
        x, y = layer.solve(T(stack(ds2, "g")), Q=Q, A=T(stack(ds2, "A")), **rows(ds2))
        out[warm] = (x.detach().cpu().numpy(), y.detach().cpu().numpy(), sum(s["iterTotal"] for s in layer.stats), bt.launch_counts())
        if warm:
            x.sum().backward()
            grad = bt.adjoint(np.ones((B, n)), None, matrices=("Q",))
            assert np.array_equal(Q.grad.cpu().numpy(), grad["Q"]) and np.any(grad["Q"] != 0.0)
        bt.close()
    ref.close()
    assert np.array_equal(out[True][0], want["x"]) and np.array_equal(out[True][1], want["y"])
    assert out[True][3] == out[False][3] == (2, 2)
    assert 2 * out[True][2] <= out[False][2]                      # the default is the load and the cold run


# ---- 6: instances whose last run failed run cold --------------------------------------------------------------------------------------------
def test_failed_instances_run_cold(hip, shape=SHAPES[1]):
    B = shape[3]
    d1, d2 = data(shape)
    ds1, ds2 = spread(d1, B), spread(d2, B)
    bt = make(hip, shape, maxIterations=3)
    load_all(bt, ds1)
    bt.run()
    _, _, st = bt.solution()
    failed = [b for b in range(B) if st[b]["returnValue"] != 0]
    assert failed and all(st[b]["returnValue"] == hip.capi.MAX_ITERATIONS_REACHED for b in failed)
    update_matrices_all(bt, ds2); update_all(bt, ds2)
    bt.resolve(warm=True)
    warm = result(bt)
    assert bt.launch_counts() == (2, 2)
    bt.close()
    assert_same_bits(warm, fresh(hip, ds2, options(hip, maxIterations=3)), rows=failed)


# ---- 7: guards ----------------------------------------------------------------------------------------------------------------------------------
def test_guards(hip, shape=SHAPES[0]):
    L = hip.lib()
    n, nC, nComp, B = shape[:4]
    d1, d2 = data(shape)
    ds1, ds2 = spread(d1, B), spread(d2, B)
    Q2 = stack(ds2, "Q"); qp = Q2.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bt = make(hip, shape)
    # an instance that holds no problem is refused: nothing loaded, then half of the batch loaded
    assert L.lcqp_hip_batch_update_matrices(bt.h, 0, 1, qp, None, None, None) == 300
    load_all(bt, ds1[:B // 2])
    assert L.lcqp_hip_batch_update_matrices(bt.h, 0, B, qp, None, None, None) == 300
    assert bt.update_matrices_device(B // 2 - 1, 2, Q=dev(Q2[:2])) == 300
    assert L.lcqp_hip_batch_update_matrices(bt.h, 0, B // 2, None, None, None, None) == 100      # no matrix at all
    load_all(bt, ds1)
    bt.run()
    first = result(bt)
    v = np.ones((B, n))
    assert bt.sensitivity(v)[0].shape == (B, n)
    # a bad range is refused with nothing written
    for lo, count in ((-1, 1), (0, 0), (1, B), (B, 1), (0, 2 ** 31 - 1)):
        assert L.lcqp_hip_batch_update_matrices(bt.h, lo, count, qp, None, None, None) == 100
        assert L.lcqp_hip_batch_update_matrices_device(bt.h, lo, count, 0, ctypes.c_void_p(dev(Q2).data_ptr()), None, None, None, None) == 100
    assert L.lcqp_hip_batch_update_matrices_device(bt.h, 0, B, 16, ctypes.c_void_p(dev(Q2).data_ptr()), None, None, None, None) == 100
    with pytest.raises(ValueError):
        bt.update_matrices(0, B, Q=Q2[:, :-1])
    with pytest.raises(ValueError):
        bt.update_matrices(1, B, Q=Q2)
    assert bt.sensitivity(v)[0].shape == (B, n)                     # the refused calls left the solve in place
    bt.resolve(warm=False)
    assert_same_bits(result(bt), first)
    assert bt.launch_counts() == (1, 2)
    # between update_matrices and the next solve nothing can be differentiated
    update_matrices_all(bt, ds2)
    with pytest.raises(RuntimeError, match="code 300"):
        bt.sensitivity(v)
    with pytest.raises(RuntimeError, match="code 300"):
        bt.jacobian(0, 1)
    with pytest.raises(RuntimeError, match="code 300"):
        bt.adjoint(v)
    bt.resolve(warm=True)
    assert bt.launch_counts() == (2, 3)
    assert bt.sensitivity(v)[0].shape == (B, n)
    # a load in between makes the next warm resolve a cold run: the bits of a fresh object
    update_matrices_all(bt, ds1)
    load_all(bt, ds1)
    bt.resolve(warm=True)
    assert_same_bits(result(bt), first)
    bt.close()
