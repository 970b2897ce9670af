"""lcqp_hip_batch_sensitivity_blocked / lcqp_hip_batch_jacobian and the QP twins: the argument checks that need no device, the shape checks
of the Python wrappers, and lcqpow_amd/diff.py without a device."""
import ctypes
import inspect

import numpy as np
import pytest

dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)
INVALID_ARGUMENT, NOT_SETUP = 100, 300


def test_the_symbols_exist():
    import lcqpow_amd as la
    L = la.lib()
    for name in ("lcqp_hip_batch_sensitivity_blocked", "lcqp_hip_batch_jacobian", "lcqp_hip_qp_sensitivity_blocked", "lcqp_hip_qp_jacobian"):
        assert callable(getattr(L, name)), name
    assert la.capi.SENS_PANEL >= 16


def test_argument_checks_need_no_device():
    import lcqpow_amd as la
    L = la.lib()
    v, dg, db = np.ones((1, 2)), np.full((2, 2), 7.0), np.full((2, 2), 7.0)
    side, info = np.full(2, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    args = lambda: (v.ctypes.data_as(dp), dg.ctypes.data_as(dp), db.ctypes.data_as(dp), side.ctypes.data_as(ip), info.ctypes.data_as(ip))
    assert L.lcqp_hip_batch_sensitivity_blocked(None, 1, *args()) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity_blocked(None, 1, *args()) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_jacobian(None, 0, 1, *args()[1:]) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_jacobian(None, *args()[1:]) == INVALID_ARGUMENT
    Q = np.eye(2)
    q = L.lcqp_hip_qp_create(2, 0, Q.ctypes.data_as(dp), None, None, 0)      # a host-side object: no device is touched
    assert q is not None
    q = ctypes.c_void_p(q)
    assert L.lcqp_hip_qp_sensitivity_blocked(q, 0, *args()) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity_blocked(q, -3, *args()) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity_blocked(q, 1, None, dg.ctypes.data_as(dp), None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity_blocked(q, 1, v.ctypes.data_as(dp), None, None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_jacobian(q, None, None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_sensitivity_blocked(q, 1, *args()) == NOT_SETUP      # before its first solve
    assert L.lcqp_hip_qp_jacobian(q, *args()[1:]) == NOT_SETUP
    L.lcqp_hip_qp_destroy(q)
    # (a batch handle does not exist without a device: the range checks of lcqp_hip_batch_jacobian and the NULL v / dg checks on a live
    # handle are in tests/test_gpu_sensitivity_blocked.py::test_a_batch_that_never_ran_is_refused)
    assert np.all(dg == 7.0) and np.all(db == 7.0) and np.all(side == 7) and np.all(info == 7)


def test_python_wrappers_check_shapes():
    import lcqpow_amd as la
    from lcqpow_amd import capi
    assert list(inspect.signature(la.BatchLCQP.sensitivity).parameters) == ["self", "v", "blocked"]
    assert inspect.signature(la.BatchLCQP.sensitivity).parameters["blocked"].default is False
    assert list(inspect.signature(la.BatchLCQP.jacobian).parameters)[:4] == ["self", "first", "count", "bounds"]
    assert inspect.signature(la.SubsolverHIP.sensitivity).parameters["blocked"].default is False and callable(la.SubsolverHIP.jacobian)
    called = []
    ok = lambda *a: called.append(a[:2]) or 0
    for first, count in ((-1, 1), (0, 0), (3, 1), (1, 3), (0, 4), (0.5, 1)):
        with pytest.raises(ValueError):
            capi._jacobian(ok, 3, 5, 9, first, count, True)
    assert not called      # every refusal came before the call
    with pytest.raises(RuntimeError):
        capi._jacobian(lambda *a: NOT_SETUP, 3, 5, 9, 0, None, True)
    Jg, Jb, side, info = capi._jacobian(ok, 3, 5, 9, 1, None, True)
    assert called == [(1, 2)] and Jg.shape == (2, 5, 5) and Jb.shape == (2, 5, 9) and side.shape == (2, 9) and info.shape == (2,)
    assert side.dtype == np.int32 and info.dtype == np.int32
    Jg, Jb, side, info = capi._jacobian(ok, 3, 5, 9, 0, 3, False)
    assert Jg.shape == (3, 5, 5) and Jb is None


def test_diff_module_has_no_cpu_fallback(monkeypatch):
    from lcqpow_amd import capi, diff
    assert callable(diff.BatchLCQPLayer.jacobian)
    src = inspect.getsource(diff.BatchLCQPLayer.jacobian)
    assert "bt.jacobian" in src and "linalg" not in src      # the library's kernel, nothing formed on the host
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "_SO", "/nonexistent/liblcqpow_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diff.BatchLCQPLayer(None)
