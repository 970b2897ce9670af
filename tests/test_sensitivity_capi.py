"""lcqp_hip_batch_sensitivity / lcqp_hip_qp_sensitivity: the argument checks that need no device, and lcqpow_amd/diff.py without one."""
import ctypes

import numpy as np
import pytest

dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)
INVALID_ARGUMENT, NOT_SETUP = 100, 300


def buffers(n, nd, k=1):
    return np.ones((k, n)), np.full((k, n), 7.0), np.full((k, nd), 7.0), np.full(nd, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)


def untouched(dg, db, side, info):
    return np.all(dg == 7.0) and np.all(db == 7.0) and np.all(side == 7) and np.all(info == 7)


def test_argument_checks_need_no_device():
    import lcqpow_amd as la
    L = la.lib()
    v, dg, db, side, info = buffers(2, 2)
    args = lambda: (v.ctypes.data_as(dp), dg.ctypes.data_as(dp), db.ctypes.data_as(dp), side.ctypes.data_as(ip), info.ctypes.data_as(ip))
    assert L.lcqp_hip_batch_sensitivity(None, 1, *args()) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity(None, 1, *args()) == INVALID_ARGUMENT
    ms = ctypes.c_float(-1.0)
    assert L.lcqp_hip_batch_sensitivity_timing(None, ctypes.byref(ms)) == INVALID_ARGUMENT and ms.value == -1.0
    Q = np.eye(2)
    q = L.lcqp_hip_qp_create(2, 0, Q.ctypes.data_as(dp), None, None, 0)      # a host-side object: no device is touched
    assert q is not None
    q = ctypes.c_void_p(q)
    assert L.lcqp_hip_qp_sensitivity(q, 0, *args()) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity(q, -3, *args()) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity(q, 1, None, dg.ctypes.data_as(dp), None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity(q, 1, *args()) == NOT_SETUP              # before its first solve
    if la.device_count() == 0:
        it, ef = ctypes.c_int(0), ctypes.c_int(0)
        g = np.zeros(2)
        assert L.lcqp_hip_qp_solve(q, 1, ctypes.byref(it), ctypes.byref(ef), g.ctypes.data_as(dp), *[None] * 6) != 0
        assert L.lcqp_hip_qp_sensitivity(q, 1, *args()) == NOT_SETUP          # a solve that failed left nothing to differentiate
    L.lcqp_hip_qp_destroy(q)
    assert untouched(dg, db, side, info)


def test_python_wrappers_check_shapes():
    from lcqpow_amd import capi
    with pytest.raises(ValueError):
        capi._sensitivity(lambda *a: 0, np.zeros((3, 5)), 2, 5, 9)          # wrong batch
    with pytest.raises(ValueError):
        capi._sensitivity(lambda *a: 0, np.zeros((2, 4)), 2, 5, 9)          # wrong nV
    with pytest.raises(RuntimeError):
        capi._sensitivity(lambda *a: NOT_SETUP, np.zeros((2, 5)), 2, 5, 9)
    seen = {}
    dg, db, side, info = capi._sensitivity(lambda k, *a: seen.setdefault("k", k) * 0, np.zeros((2, 4, 5)), 2, 5, 9)
    assert seen["k"] == 4 and dg.shape == (2, 4, 5) and db.shape == (2, 4, 9) and side.shape == (2, 9) and info.shape == (2,)
    dg, db, side, info = capi._sensitivity(lambda *a: 0, np.zeros((2, 5)), 2, 5, 9)
    assert dg.shape == (2, 5) and db.shape == (2, 9)


def test_split_bound_derivatives():
    from lcqpow_amd import split_bound_derivatives
    nV, nC, nComp = 2, 3, 1
    #                 box      A             L    R
    side = np.array([[0, 1, -1, 2, 0, -1, -1]])
    db = np.arange(1.0, 8.0)[None]
    p = split_bound_derivatives(db, side, nV, nC, nComp)
    assert p["dlb"].tolist() == [[0, 0]] and p["dub"].tolist() == [[0, 2]]
    assert p["dlbA"].tolist() == [[3, 4, 0]] and p["dubA"].tolist() == [[0, 4, 0]]      # the equality row: its one value under both bounds
    assert p["dlbL"].tolist() == [[6]] and p["dlbR"].tolist() == [[7]] and p["dubL"].tolist() == [[0]] and p["dubR"].tolist() == [[0]]
    p3 = split_bound_derivatives(np.stack([db, 2 * db], axis=1), side, nV, nC, nComp)       # [B][k][nd]
    assert p3["dlbA"].shape == (1, 2, 3) and p3["dlbA"][0, 1].tolist() == [6, 8, 0]


def test_diff_module_has_no_cpu_fallback(monkeypatch):
    from lcqpow_amd import capi, diff
    assert issubclass(diff.LCQPSolveFunction, __import__("torch").autograd.Function)
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "_SO", "/nonexistent/liblcqpow_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diff.BatchLCQPLayer(None)
