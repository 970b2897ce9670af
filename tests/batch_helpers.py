"""Helpers the re-solve and sensitivity tests of both arms share (tests/test_gpu_resolve.py, test_gpu_sparse_resolve.py,
test_gpu_sensitivity.py, test_gpu_sparse_sensitivity.py).  bt: a BatchLCQP or a SparseBatchLCQP; ds: one problem dict per instance
(tests/problems.py)."""
import contextlib
import inspect
import os

import numpy as np

import problems as P

LD = np.longdouble


def stack(ds, key):
    return None if ds[0].get(key) is None else np.stack([d[key] for d in ds])


def vectors(call, ds):
    """the optional vectors of P.VEC_KEYS that `call` (a load or an update of either arm) takes, stacked over the instances"""
    return {k: stack(ds, k) for k in P.VEC_KEYS if k in inspect.signature(call).parameters}


def load_all(bt, ds):
    rc = bt.load(0, len(ds), stack(ds, "Q"), stack(ds, "g"), stack(ds, "L"), stack(ds, "R"), A=stack(ds, "A"), **vectors(bt.load, ds))
    assert rc == 0, rc


def handle(hip, ds, opt, B=None):
    """a sparse handle for the pattern of ds[0], its instances loaded"""
    d = ds[0]
    sb = hip.SparseBatchLCQP(B or len(ds), d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=opt)
    rc = sb.load(0, len(ds), np.stack([q["Q"].data for q in ds]), stack(ds, "g"), np.stack([q["E"].data for q in ds]), **vectors(sb.load, ds))
    assert rc == 0, rc
    return sb


def update_all(bt, ds, first=0):
    rc = bt.update(first, len(ds), stack(ds, "g"), **vectors(bt.update, ds))
    assert rc == 0, (rc, bt._last_error())


def result(bt, trace=False):
    """the solution and statistics of the last run; the dense arm's work counters with them"""
    x, y, st = bt.solution()
    out = dict(x=x, y=y, st=st)
    if hasattr(bt, "work_sums"):
        out["work"] = bt.work_sums()
    if trace:
        out["trace"] = [bt.trace(b) for b in range(bt.B)]
    return out


def assert_same_bits(a, b, rows=None):
    rows = range(len(a["st"])) if rows is None else rows
    for i in rows:
        assert np.array_equal(a["x"][i], b["x"][i]) and np.array_equal(a["y"][i], b["y"][i]), i
        assert a["st"][i] == b["st"][i], (i, a["st"][i], b["st"][i])
        if "trace" in a:
            assert np.array_equal(a["trace"][i][0], b["trace"][i][0]) and np.array_equal(a["trace"][i][1], b["trace"][i][1]), i
            assert len(a["trace"][i][0]) == a["st"][i]["iterTotal"]


def kkt_reference(Q, EW, V, extended):
    """dg, mu for the columns of V: K [d; mu] = [v; 0]; float64 LU, refined with long-double residuals when `extended`.  Also cond_2(K)."""
    n, m = Q.shape[0], EW.shape[0]
    K = np.zeros((n + m, n + m)); K[:n, :n] = Q; K[:n, n:] = EW.T; K[n:, :n] = EW
    rhs = np.zeros((n + m, V.shape[1])); rhs[:n] = V
    sol = np.linalg.solve(K, rhs)
    if extended:
        KL, rl, sl = K.astype(LD), rhs.astype(LD), sol.astype(LD)
        for _ in range(3):
            sl = sl + np.linalg.solve(K, (rl - KL @ sl).astype(np.float64)).astype(LD)
        sol = sl
    ev = np.abs(np.linalg.eigvalsh(K))
    return -sol[:n], sol[n:], float(ev.max() / ev.min())


@contextlib.contextmanager
def environment(env):
    """the test hooks are read when a handle is created"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def grown_and_fresh(make, V):
    """sensitivity with nrhs = 1, 3, 1 on one solved handle -- the buffers grow from a live smaller allocation and are then used below
    their size -- against the same calls on a second handle that was asked for nrhs = 3 first; make() returns a solved handle"""
    a, b = make(), make()
    counts = a.launch_counts()
    b.sensitivity(V)
    for v in (V[:, :1], V, V[:, :1]):
        for got, want in zip(a.sensitivity(v), b.sensitivity(v)):
            assert np.array_equal(got, want)
    assert np.any(a.sensitivity(V)[0] != 0.0)
    assert a.launch_counts() == counts == b.launch_counts()
    a.close(); b.close()
