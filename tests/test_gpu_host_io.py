"""The host load / update of both arms against numpy and against recorded bits.  The host calls are the device path behind an upload
(DESIGN.md section 3a'''''), so the "same bits as the host call" cases of test_gpu_device_io.py and test_gpu_sparse_device_io.py compare
the pack kernels with themselves; this file is the independent pin.  What *_read_problem returns is compared with the numpy inputs,
exactly.  What the dense reader does not return (lb, ub, x0, y0, lbL, lbR, the list of box-bounded variables) is held through the x, y
and statistics of solves, byte for byte against tests/golden/host_io_bits.npz, recorded by tools/make_host_io_golden.py with the host
packing loops this path replaced.  No tolerance anywhere in this file."""
import torch      # noqa: F401 -- before the library is first loaded: the library and torch must share one HIP runtime (lcqpow_amd.capi.lib)

import os

import numpy as np
import pytest

import host_io_cases as H
import problems as P
from batch_helpers import stack, vectors
from problems import OPT, SMALL, instances

pytestmark = pytest.mark.gpu

INVALID_LOWER_COMPLEMENTARITY_BOUND = 120
INF = np.inf
_runs = {}


def bits(a, b):
    """the same shape and the same bytes (NaNs and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_solution(a, b):
    """x, y and the statistics of two solution() calls"""
    return bits(a[0], b[0]) and bits(a[1], b[1]) and bits(H.stats_array(a[2]), H.stats_array(b[2]))


def or_default(v, size, dflt):
    return np.full(size, dflt) if v is None else v


# ---- the dense arm ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(P.GOLDEN, "host_io_bits.npz"))


def stages(hip, case, chunked=False):
    """H.run_stages, once per case and cap"""
    if (case, chunked) not in _runs:
        _runs[case, chunked] = H.run_stages(hip, case, chunked)
    return _runs[case, chunked]


def held(case):
    """the instances the batch holds after each stage"""
    ds, ds2, ds3 = H.data(case)
    f, c = H.RANGE
    mixed = ds[:f] + ds2 + ds[f + c:]
    return dict(load=ds, range=mixed, update=ds3)


def assert_dense_pools(pools, ds):
    for b, (got, d) in enumerate(zip(pools, ds)):
        n, nC = d["nV"], d["nC"]
        want = dict(Q=d["Q"], g=d["g"], A=d["A"], L=d["L"], R=d["R"], lbA=or_default(d["lbA"], nC, -INF), ubA=or_default(d["ubA"], nC, INF))
        assert set(got) == set(want)
        for k in want:
            assert bits(got[k], np.asarray(want[k], dtype=np.float64).reshape(got[k].shape)), (b, k)


def test_the_dense_cases_cover_the_ground():
    """every optional vector present in one case and absent in another; a box on a strict subset of the variables"""
    firsts = [H.data(c)[0][0] for c in H.CASES]
    for k in H.OPTIONAL:
        assert any(d[k] is not None for d in firsts) and any(d[k] is None for d in firsts), k
    for case in H.CASES:
        for d in H.data(case)[0]:
            fin = np.isfinite(or_default(d["lb"], d["nV"], -INF)) | np.isfinite(or_default(d["ub"], d["nV"], INF))
            assert 0 < fin.sum() < d["nV"], case


@pytest.mark.parametrize("case", H.CASES, ids=H.IDS)
def test_dense_pools_equal_the_numpy_inputs(hip, case):
    _, pools = stages(hip, case)
    for stage, ds in held(case).items():
        assert_dense_pools(pools[stage], ds)


@pytest.mark.parametrize("case", H.CASES, ids=H.IDS)
def test_dense_solves_return_the_recorded_bits(hip, golden, case):
    """a load of the batch, a load of [2, 4) onto the filled batch, an update and a warm re-solve: x, y and the statistics of each solve"""
    got, _ = stages(hip, case)
    name = H.IDS[H.CASES.index(case)]
    assert len(got) == 3 * len(H.STAGES)
    for k, v in got.items():
        assert bits(v, golden[name + ": " + k]), (name, k)


@pytest.mark.parametrize("case", H.CASES, ids=H.IDS)
def test_dense_chunked_calls_leave_the_same_bits(hip, golden, case):
    """under a staging cap that cuts a call on 5 instances into chunks of 2, 2 and 1 (and one on 2 instances into 1 and 1)"""
    got, pools = stages(hip, case, chunked=True)
    _, whole = stages(hip, case)
    name = H.IDS[H.CASES.index(case)]
    for k, v in got.items():
        assert bits(v, golden[name + ": " + k]), (name, k)
    for stage in H.STAGES:
        for a, b in zip(pools[stage], whole[stage]):
            assert all(bits(a[k], b[k]) for k in a), stage


def test_dense_failing_load_leaves_the_range_untouched(hip):
    """-inf in lbL of the third instance: an invalid argument, found before anything is written"""
    case = ((129, 2, 3), "full")
    (n, nC, nK), _ = case
    ds, _, ds3 = H.data(case)
    bt = hip.BatchLCQP(H.B, n, nC, nK, with_box=True, opt=hip.default_options(perturbStep=0, printLevel=0))
    load = lambda xs: bt.load(0, H.B, *[stack(xs, k) for k in ("Q", "g", "L", "R")], A=stack(xs, "A"), **vectors(bt.load, xs))
    assert load(ds) == 0
    bt.run()
    before, pools = bt.solution(), [bt.read_problem(b) for b in range(H.B)]
    bad = [dict(d) for d in ds3]
    bad[2]["lbL"] = np.where(np.arange(nK) == 1, -INF, bad[2]["lbL"])
    assert load(bad) == INVALID_LOWER_COMPLEMENTARITY_BOUND
    for b in range(H.B):
        assert all(bits(v, pools[b][k]) for k, v in bt.read_problem(b).items()), b
    bt.run()
    after = bt.solution()
    assert same_solution(before, after)
    bt.close()


# ---- the sparse arm -----------------------------------------------------------------------------------------------------------------------
SPARSE_B = 5
SPARSE_CASES = ("small", "grid, general ldl")
SP_OPTIONAL = ("lbA", "ubA", "lbL", "ubL", "lbR", "ubR", "x0", "y0")
_sparse = {}


def sparse_data(key):
    """(full, bare, moved): SPARSE_B instances with every optional vector, the same without any, and the full ones with other vectors"""
    if key not in _sparse:
        if key == "small":
            ds = instances(SMALL, SPARSE_B)
        else:
            d = P.grid_lcqp(44, 300, 200)
            d["Q"].sort_indices(); d["E"].sort_indices()
            ds = []
            for b in range(SPARSE_B):      # one pattern, other values
                Q, E = d["Q"].copy(), d["E"].copy()
                Q.data = Q.data * (1.0 + 0.01 * b); E.data = E.data * (1.0 - 0.01 * b)
                ds.append(dict(d, Q=Q, E=E, g=d["g"] * (1.0 + 0.03 * b)))
        rng = np.random.default_rng(17)
        n, nC, nK = ds[0]["nV"], ds[0]["nC"], ds[0]["nComp"]
        full = [dict(d, lbL=rng.uniform(-0.2, 0.0, nK), lbR=rng.uniform(-0.2, 0.0, nK), ubL=rng.uniform(5.0, 6.0, nK), ubR=rng.uniform(5.0, 6.0, nK),
                     x0=rng.uniform(-0.1, 0.1, n), y0=rng.uniform(-0.1, 0.1, nC + 2 * nK)) for d in ds]
        bare = [dict(d, **{k: None for k in SP_OPTIONAL}) for d in full]
        other = [dict(d, g=d["g"] * (1.0 + 0.02 * rng.standard_normal(n)), **{k: d[k] + 0.01 * rng.uniform(-1.0, 1.0, d[k].shape) for k in SP_OPTIONAL})
                 for d in full]
        _sparse[key] = (full, bare, other)
    return _sparse[key]


def sparse_handle(hip, key):
    d = sparse_data(key)[0][0]
    sb = hip.SparseBatchLCQP(SPARSE_B, d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(**OPT))
    assert (sb.fronts() > 0) == (key != "small")
    return sb


def sparse_call(sb, f, ds, first=0, chunk=None):
    """a host load (with the value arrays) or update of ds; chunk: under the staging cap that makes the call go in chunks of that many instances"""
    args = [np.stack([d["Q"].data for d in ds]), stack(ds, "g"), np.stack([d["E"].data for d in ds])] if f == sb.load else [stack(ds, "g")]
    kw = vectors(f, ds)
    with sb._staging(None if chunk is None else H.cap_for(args + list(kw.values()), len(ds), chunk)):
        return f(first, len(ds), *args, **kw)


def assert_sparse_pools(sb, ds, y0_kept=None):
    """read_problem of every instance against the numpy inputs; an absent vector against its default (y0: zeros after a load, what the pool
    held -- y0_kept -- after an update)"""
    for b, d in enumerate(ds):
        got = sb.read_problem(b)
        nC, nK, n = d["nC"], d["nComp"], d["nV"]
        m = nC + 2 * nK
        y0 = d["y0"] if d["y0"] is not None else (np.zeros(m) if y0_kept is None else y0_kept[b])
        want = dict(Qx=d["Q"].data, Ax=d["E"].data, g=d["g"], x0=or_default(d["x0"], n, 0.0), y0=y0,
                    lE=np.concatenate([or_default(d["lbA"], nC, -INF), or_default(d["lbL"], nK, 0.0), or_default(d["lbR"], nK, 0.0)]),
                    uE=np.concatenate([or_default(d["ubA"], nC, INF), or_default(d["ubL"], nK, INF), or_default(d["ubR"], nK, INF)]),
                    lbL=or_default(d["lbL"], nK, 0.0), lbR=or_default(d["lbR"], nK, 0.0))
        assert set(got) == set(want) | {"hasY0"}
        assert got["hasY0"] == (0 if d["y0"] is None else 1), b
        for k in want:
            assert bits(got[k], np.asarray(want[k], dtype=np.float64)), (b, k)


@pytest.mark.parametrize("key", SPARSE_CASES)
def test_sparse_pools_equal_the_numpy_inputs(hip, key):
    """after a load and after an update, every vector given and every vector absent"""
    full, bare, other = sparse_data(key)
    sb = sparse_handle(hip, key)
    assert sparse_call(sb, sb.load, full) == 0
    assert_sparse_pools(sb, full)
    assert sparse_call(sb, sb.update, bare) == 0
    assert_sparse_pools(sb, bare, y0_kept=[d["y0"] for d in full])
    assert sparse_call(sb, sb.update, other) == 0
    assert_sparse_pools(sb, other)
    assert sparse_call(sb, sb.load, bare) == 0
    assert_sparse_pools(sb, bare)
    assert sparse_call(sb, sb.load, other[2:4], first=2) == 0      # a range onto the filled batch
    assert_sparse_pools(sb, bare[:2] + other[2:4] + bare[4:])
    sb.close()


@pytest.mark.parametrize("key", SPARSE_CASES)
def test_sparse_chunked_calls_leave_the_same_bits(hip, key):
    """chunks of 2, 2 and 1 instances against one chunk: the pools after a load and after an update, and for the banded case the solves"""
    full, _, other = sparse_data(key)
    a, b = sparse_handle(hip, key), sparse_handle(hip, key)
    results = []
    for ds, f in ((full, "load"), (other, "update")):
        assert sparse_call(a, getattr(a, f), ds) == 0 and sparse_call(b, getattr(b, f), ds, chunk=2) == 0
        assert_sparse_pools(b, ds)
        for i in range(SPARSE_B):
            pa, pb = a.read_problem(i), b.read_problem(i)
            assert all(pa[k] == pb[k] if k == "hasY0" else bits(pa[k], pb[k]) for k in pa), (f, i)
        if key == "small":
            for sb in (a, b):
                sb.run() if f == "load" else sb.resolve(warm=True)
            results.append((a.solution(), b.solution()))
    for ra, rb in results:
        assert same_solution(ra, rb)
    a.close(); b.close()


def test_sparse_failing_load_leaves_the_range_untouched(hip):
    full, _, other = sparse_data("small")
    sb = sparse_handle(hip, "small")
    assert sparse_call(sb, sb.load, full) == 0
    sb.run()
    before, pools = sb.solution(), [sb.read_problem(b) for b in range(SPARSE_B)]
    bad = [dict(d) for d in other]
    bad[2]["lbL"] = np.where(np.arange(bad[2]["nComp"]) == 1, -INF, bad[2]["lbL"])
    assert sparse_call(sb, sb.load, bad) == INVALID_LOWER_COMPLEMENTARITY_BOUND
    for b in range(SPARSE_B):
        got = sb.read_problem(b)
        assert all(got[k] == pools[b][k] if k == "hasY0" else bits(got[k], pools[b][k]) for k in got), b
    sb.run()
    after = sb.solution()
    assert same_solution(before, after)
    sb.close()
