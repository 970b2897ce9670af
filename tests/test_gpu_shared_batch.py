"""A dense batch that holds ONE Q, A, L, R (BatchLCQP(shared_matrices=True), lcqp_hip_batch_create_shared; DESIGN.md section 3a, "One set of
matrices").  The contract every test here holds it to: an instance of a shared batch returns the same BITS as the same problem in an
ordinary batch of the same shape loaded with the same data -- it is the same device code on the same numbers at another address.  Each test
builds both batches from one model (tests/problems.py: random_lcqp) whose instances differ in g, the constraint and box bounds, x0 and, on
every second instance, lbL / lbR.  The ordinary batch gets the matrices tiled."""
import ctypes

import numpy as np
import pytest
import torch      # noqa: F401 -- before the library is first loaded: the device twins need the library and torch on one HIP runtime

from batch_helpers import assert_same_bits, load_all, result, stack, update_all, vectors
from problems import perturbed, random_lcqp
from test_gpu_matrix_resolve import new_matrices

pytestmark = pytest.mark.gpu

# (n, nC, nComp, B, box): np = 128 with the row state in LDS; np = 256 with box bounds on a fixed subset of the variables
SHAPES = ((24, 10, 6, 5, False), (130, 20, 8, 3, True))
IDS = ["%dx%dx%d-B%d" % s[:4] for s in SHAPES]
BIG = (520, 12, 6, 2, False)      # np = 1024: the vector-kernel fallback of the blocked calls and Jacobians
MATS = ("Q", "L", "R", "A")
INVALID_ARGUMENT = 100

_models = {}


def model(shape, seed=0):
    """(base problem, its B instances): one set of matrices, per-instance vectors"""
    key = (shape, seed)
    if key not in _models:
        n, nC, nComp, B, box = shape
        rng = np.random.default_rng(11 + seed)
        base = random_lcqp(rng, n, nC, nComp, box, False)
        if box:      # a fixed subset: the upper half of the variables carries no box bound
            base["lb"][n // 2:] = -np.inf; base["ub"][n // 2:] = np.inf
        ds = []
        for b in range(B):
            d = perturbed(base, 300 + 17 * seed + b)
            shift = b % 2 == 1
            d.update(x0=0.1 * rng.standard_normal(n), lbL=-0.1 * rng.random(nComp) * shift, lbR=-0.1 * rng.random(nComp) * shift)
            ds.append(d)
        _models[key] = (base, ds)
    return _models[key]


def options(hip, **kw):
    return hip.default_options(perturbStep=0, printLevel=0, **kw)


def pair(hip, shape, ds, **kw):
    """(ordinary batch, shared batch) holding the instances ds"""
    n, nC, nComp, B, box = shape
    a = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=options(hip, **kw))
    s = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=options(hip, **kw), shared_matrices=True)
    load_all(a, ds)
    load_shared(s, ds)
    return a, s


def load_shared(s, ds, first=0, matrices=True):
    d = ds[0]
    m = {k: (d[k] if matrices else None) for k in MATS}
    rc = s.load(first, len(ds), m["Q"], stack(ds, "g"), m["L"], m["R"], A=m["A"], **vectors(s.load, ds))
    assert rc == 0, (rc, s._last_error())


def both(a, s, call):
    call(a); call(s)


def same(a, s, trace=False):
    ra, rs = result(a, trace), result(s, trace)
    assert all(st["returnValue"] == 0 for st in ra["st"]), [st["returnValue"] for st in ra["st"]]      # not two identical failures
    assert_same_bits(ra, rs)
    assert np.array_equal(ra["work"], rs["work"])


# ---- 1: run ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_run_returns_the_bits_of_an_ordinary_batch(hip, shape):
    a, s = pair(hip, shape, model(shape)[1], storeSteps=1)
    both(a, s, lambda b: b.run())
    same(a, s, trace=True)
    x = result(s)["x"]
    assert not np.array_equal(x[0], x[1])      # the instances are different problems
    a.close(); s.close()


def test_run_with_more_than_three_workgroups_per_cu(hip):
    """B = 800 at np = 128: the ordinary batch factors on k_factor's 128-register build (more than three workgroups per CU), the shared
    batch's one matrix instance on the other build, and the homotopy runs on the standard build of k_lcqp_run, not the second one"""
    shape = SHAPES[0][:3] + (800, False)
    a, s = pair(hip, shape, model(shape)[1])
    both(a, s, lambda b: b.run())
    same(a, s)
    a.close(); s.close()


# ---- 2: new vectors, cold and warm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_update_and_resolve(hip, shape):
    ds = model(shape)[1]
    a, s = pair(hip, shape, ds)
    both(a, s, lambda b: b.run())
    same(a, s)
    rho = np.linspace(0.5, 2.0, shape[3])
    for k, (warm, rho0) in enumerate(((False, None), (True, None), (True, rho))):
        ds2 = [perturbed(d, 900 + 10 * k + i) for i, d in enumerate(ds)]
        both(a, s, lambda b: update_all(b, ds2))
        both(a, s, lambda b: b.resolve(warm=warm, rho0=rho0))
        same(a, s)
    assert a.launch_counts() == s.launch_counts() == (1, 4)
    a.close(); s.close()


# ---- 3: new matrices under the stored point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_update_matrices_and_warm_resolve(hip, shape):
    base, ds = model(shape)
    B = shape[3]
    a, s = pair(hip, shape, ds)
    both(a, s, lambda b: b.run())
    same(a, s)
    new = new_matrices(base, 41)
    # a partial range is refused by the C call, and the refusal writes nothing
    dp = ctypes.POINTER(ctypes.c_double)
    Qn = np.ascontiguousarray(new["Q"])
    assert hip.lib().lcqp_hip_batch_update_matrices(s.h, 0, B - 1, Qn.ctypes.data_as(dp), None, None, None) == INVALID_ARGUMENT
    assert hip.lib().lcqp_hip_batch_update_matrices(s.h, 1, B - 1, Qn.ctypes.data_as(dp), None, None, None) == INVALID_ARGUMENT
    with pytest.raises(ValueError):
        s.update_matrices(0, B - 1, Q=new["Q"])
    # ... nothing: the setup is still valid (a refresh, no second setup), the matrices are the old ones, and a warm resolve returns the
    # bits of the ordinary batch, which saw no such call
    both(a, s, lambda b: b.resolve(warm=True))
    same(a, s)
    assert a.launch_counts() == s.launch_counts() == (1, 2)
    assert np.array_equal(s.read_problem(B - 1)["Q"], base["Q"])
    assert a.update_matrices(0, B, **{k: np.stack([new[k]] * B) for k in MATS}) == 0
    assert s.update_matrices(0, B, **{k: new[k] for k in MATS}) == 0, s._last_error()
    both(a, s, lambda b: b.resolve(warm=True))
    same(a, s)
    assert a.launch_counts() == s.launch_counts() == (2, 3)
    for b in (0, B - 1):
        assert np.array_equal(s.read_problem(b)["Q"], new["Q"]) and np.array_equal(s.read_problem(b)["A"], new["A"])
    a.close(); s.close()


# ---- 4: derivatives -------------------------------------------------------------------------------------------------------------------
def same_arrays(got, want):
    if isinstance(got, dict):
        assert got.keys() == want.keys()
        got, want = [got[k] for k in sorted(got)], [want[k] for k in sorted(want)]
    for g, w in zip(got, want):
        if g is None or w is None:
            assert g is None and w is None
        else:
            g, w = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in (g, w))
            assert np.array_equal(g, w)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_derivatives(hip, shape):
    n, nC, nComp, B, box = shape
    a, s = pair(hip, shape, model(shape)[1])
    both(a, s, lambda b: b.run())
    same(a, s)
    rng = np.random.default_rng(5)
    V = rng.standard_normal((B, 3, n)); VY = rng.standard_normal((B, 3, a.nd))
    same_arrays(s.sensitivity(V), a.sensitivity(V))
    assert np.any(s.sensitivity(V)[0] != 0.0)
    same_arrays(s.sensitivity(V, blocked=True), a.sensitivity(V, blocked=True))
    same_arrays(s.jacobian(), a.jacobian())
    same_arrays(s.jacobian_duals(), a.jacobian_duals())
    for reduce in (False, True):
        same_arrays(s.adjoint(V[:, 0], VY[:, 0], reduce=reduce), a.adjoint(V[:, 0], VY[:, 0], reduce=reduce))
    same_arrays(s.adjoint_blocked(V, VY), a.adjoint_blocked(V, VY))
    # one device twin of each family
    dev = torch.device("cuda", 0)
    tV, tVY = torch.as_tensor(V, device=dev), torch.as_tensor(VY, device=dev)
    same_arrays(s.sensitivity_device(tV), a.sensitivity_device(tV))
    same_arrays(s.jacobian_device(), a.jacobian_device())
    same_arrays(s.adjoint_device(tV[:, 0].contiguous(), tVY[:, 0].contiguous(), reduce=True), a.adjoint_device(tV[:, 0].contiguous(), tVY[:, 0].contiguous(), reduce=True))
    torch.cuda.synchronize()
    a.close(); s.close()


def test_sensitivity_and_jacobian_at_np_1024(hip):
    n, nC, nComp, B, box = BIG
    a, s = pair(hip, BIG, model(BIG)[1])
    both(a, s, lambda b: b.run())
    same(a, s)
    V = np.random.default_rng(6).standard_normal((B, 2, n))
    same_arrays(s.sensitivity(V), a.sensitivity(V))
    same_arrays(s.sensitivity(V, blocked=True), a.sensitivity(V, blocked=True))
    same_arrays(s.jacobian(first=1, count=1), a.jacobian(first=1, count=1))
    a.close(); s.close()


# ---- 5: loads in pieces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_loads_in_pieces_and_a_replaced_matrix(hip, shape):
    n, nC, nComp, B, box = shape
    base, ds = model(shape)
    a, s = pair(hip, shape, ds)
    p = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=options(hip), shared_matrices=True)
    # descending order of `first`: the matrices come with the first piece, NULL afterwards
    assert p.load(B - 1, 1, None, ds[B - 1]["g"], None, None) != 0       # no matrix in place yet: the missing-matrix code
    load_shared(p, ds[B - 1:], first=B - 1)
    load_shared(p, ds[1:B - 1], first=1, matrices=False)
    load_shared(p, ds[:1], first=0, matrices=False)
    both(a, s, lambda b: b.run())
    p.run()
    same(a, s)
    assert_same_bits(result(s), result(p))
    # a second Q replaces the matrix of every instance
    new = new_matrices(base, 43)
    d0 = dict(ds[0], Q=new["Q"])
    assert p.load(0, 1, new["Q"], d0["g"], None, None, **vectors(p.load, [d0])) == 0, p._last_error()
    ds2 = [dict(d, Q=new["Q"]) for d in ds]
    f = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=options(hip))
    load_all(f, ds2)
    f.run(); p.run()
    same(f, p)
    assert np.array_equal(p.read_problem(B - 1)["Q"], new["Q"])
    for b in (a, s, p, f):
        b.close()


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip):
    shape = SHAPES[1]
    n, nC, nComp, B, box = shape
    base, ds = model(shape)
    a, s = pair(hip, shape, ds)
    both(a, s, lambda b: b.run())
    same(a, s)
    # a differing set of box-bounded variables: instance 1, variable n - 1 gains a bound
    bad = [dict(d) for d in ds]
    bad[1]["ub"] = bad[1]["ub"].copy(); bad[1]["ub"][n - 1] = 5.0
    rc = s.load(0, B, None, stack(bad, "g"), None, None, **vectors(s.load, bad))
    assert rc == INVALID_ARGUMENT and "instance 1" in s._last_error() and "variable %d" % (n - 1) in s._last_error()
    # the device twin without the shared bit of a matrix it hands over
    dev = torch.device("cuda", 0)
    Q3 = torch.as_tensor(np.stack([base["Q"]] * B), device=dev)
    with pytest.raises(ValueError):
        s.load_device(0, B, Q3, torch.as_tensor(stack(ds, "g"), device=dev), None, None)
    v = [torch.as_tensor(stack(ds, "g"), device=dev).data_ptr()] + [None] * 10
    rc = hip.lib().lcqp_hip_batch_load_device(s.h, 0, B, 0, Q3.data_ptr(), v[0], None, None, *v[1:5], None, *v[5:], None)
    assert rc == INVALID_ARGUMENT and "shared" in s._last_error()
    rc = hip.lib().lcqp_hip_batch_update_matrices_device(s.h, 0, B, 0, Q3.data_ptr(), None, None, None, None)
    assert rc == INVALID_ARGUMENT
    with pytest.raises(RuntimeError):
        s.generate_synthetic(0)
    assert "one set of matrices" in s._last_error()
    # nothing was written, no setup was lost: a warm resolve on both is still one refresh and the same bits
    both(a, s, lambda b: b.resolve(warm=True))
    same(a, s)
    assert s.launch_counts() == (1, 2)
    a.close(); s.close()


# ---- 7: memory ------------------------------------------------------------------------------------------------------------------------
def test_device_bytes(hip):
    n, nC, nComp = 130, 20, 8
    got = {}
    for B in (1, 8):
        for shared in (False, True):
            b = hip.BatchLCQP(B, n, nC, nComp, with_box=True, shared_matrices=shared)
            got[B, shared] = b.device_bytes()
            b.close()
    assert got[1, True][1] == got[8, True][1] > 0
    assert 8 * (got[1, True][0] - got[1, True][1]) == got[8, True][0] - got[8, True][1]
    assert got[1, False][1] == got[8, False][1] == 0
    assert got[8, True][0] < got[8, False][0] and got[1, True][0] == got[1, False][0]
    b = hip.BatchLCQP(1, n, nC, nComp)
    assert hip.lib().lcqp_hip_batch_device_bytes(b.h, None) == INVALID_ARGUMENT      # a valid handle, no place for the answer
    b.close()


# ---- 8: a setup that fails, fails for every instance ---------------------------------------------------------------------------------
def test_indefinite_Q_fails_every_instance(hip):
    """Q - 3 I, as tests/test_gpu_setup.py builds its setup failure: both passes of k_factor fail"""
    shape = SHAPES[0]
    n, B = shape[0], shape[3]
    ds = [dict(d, Q=d["Q"] - 3.0 * np.eye(n)) for d in model(shape)[1]]
    a, s = pair(hip, shape, ds)
    both(a, s, lambda b: b.run())
    ra, rs = result(a), result(s)
    assert all(st["returnValue"] != 0 for st in ra["st"])
    assert [st["returnValue"] for st in ra["st"]] == [st["returnValue"] for st in rs["st"]]
    assert [a.read_setup(b)["setupFail"] for b in range(B)] == [s.read_setup(b)["setupFail"] for b in range(B)] == [3] * B
    a.close(); s.close()


def test_zero_Q_ends_as_on_an_ordinary_batch(hip):
    """a singular Q, the zero matrix: whatever the ordinary batch makes of it -- the proximal shift lets L1 exist, the solve may still
    fail -- every instance of the shared batch makes the same: codes, setup marks and, where an instance returned 0, bits"""
    shape = SHAPES[0]
    n, B = shape[0], shape[3]
    ds = [dict(d, Q=np.zeros((n, n))) for d in model(shape)[1]]
    a, s = pair(hip, shape, ds)
    both(a, s, lambda b: b.run())
    ra, rs = result(a), result(s)
    assert [st["returnValue"] for st in ra["st"]] == [st["returnValue"] for st in rs["st"]]
    assert [a.read_setup(b)["setupFail"] for b in range(B)] == [s.read_setup(b)["setupFail"] for b in range(B)]
    assert_same_bits(ra, rs)
    a.close(); s.close()


# ---- 9: the readers -------------------------------------------------------------------------------------------------------------------
def test_readers_return_the_one_set_for_every_instance(hip):
    shape = SHAPES[1]
    B = shape[3]
    base, ds = model(shape)
    a, s = pair(hip, shape, ds)
    both(a, s, lambda b: b.run())
    for b in (0, B - 1):
        pa, ps = a.read_problem(b), s.read_problem(b)
        for k in pa:
            assert np.array_equal(pa[k], ps[k]), k
        assert np.array_equal(ps["Q"], base["Q"]) and np.array_equal(ps["g"], ds[b]["g"])
        sa, ss = a.read_setup(b), s.read_setup(b)
        for k in sa:
            assert np.array_equal(sa[k], ss[k]), k
    a.close(); s.close()
