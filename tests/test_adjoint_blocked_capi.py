"""lcqp_hip_batch_adjoint_blocked / _jacobian_duals and the three device-pointer twins (DESIGN.md section 3a'''', "Panels with gradients on
y"): the symbols in the header, the library and capi.py, the answers that need no device, and the shape checks of the Python wrappers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)
INVALID_ARGUMENT, NOT_SETUP = 100, 300
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lcqp_hip_batch_adjoint_blocked", "lcqp_hip_batch_jacobian_duals", "lcqp_hip_batch_adjoint_blocked_device",
       "lcqp_hip_batch_jacobian_device", "lcqp_hip_batch_jacobian_duals_device")


def test_the_symbols_are_declared_exported_and_bound():
    import lcqpow_amd as la
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcqp_hip.h")).read(), flags=re.S)
    L = la.lib()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        f = getattr(L, name)
        assert callable(f) and f.argtypes is not None, name
    for method in ("adjoint_blocked", "jacobian_duals", "adjoint_blocked_device", "jacobian_device", "jacobian_duals_device"):
        assert callable(getattr(la.BatchLCQP, method)), method
    assert list(inspect.signature(la.BatchLCQP.adjoint_blocked).parameters) == ["self", "VX", "VY"]
    assert inspect.signature(la.BatchLCQP.adjoint_blocked).parameters["VY"].default is None
    assert list(inspect.signature(la.BatchLCQP.jacobian_duals).parameters) == ["self", "first", "count", "bounds", "_staging_bytes"]
    # existing signatures stay
    assert list(inspect.signature(la.BatchLCQP.sensitivity).parameters) == ["self", "v", "blocked"]
    assert list(inspect.signature(la.BatchLCQP.jacobian).parameters) == ["self", "first", "count", "bounds", "_staging_bytes"]


def test_argument_checks_need_no_device():
    import lcqpow_amd as la
    L = la.lib()
    vx, vy, dg, db = np.ones((1, 2)), np.ones((1, 5)), np.full((1, 2), 7.0), np.full((1, 5), 7.0)
    side, info = np.full(5, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    P = lambda a: a.ctypes.data_as(dp)
    I = lambda a: a.ctypes.data_as(ip)
    # the host calls: a NULL handle is an invalid argument, as for lcqp_hip_batch_sensitivity_blocked / _jacobian
    assert L.lcqp_hip_batch_adjoint_blocked(None, 1, P(vx), P(vy), P(dg), P(db), I(side), I(info)) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_adjoint_blocked(None, 1, None, None, P(dg), None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_jacobian_duals(None, 0, 1, P(dg), P(db), I(side), I(info)) == INVALID_ARGUMENT
    # the device twins: a NULL handle is LCQP_LCQPOBJECT_NOT_SETUP, as for the existing _device calls
    assert L.lcqp_hip_batch_sensitivity_device(None, 1, 1, None, None, None, None, None, None) == NOT_SETUP
    assert L.lcqp_hip_batch_adjoint_blocked_device(None, 1, None, None, None, None, None, None, None) == NOT_SETUP
    assert L.lcqp_hip_batch_jacobian_device(None, 0, 1, None, None, None, None, None) == NOT_SETUP
    assert L.lcqp_hip_batch_jacobian_duals_device(None, 0, 1, None, None, None, None, None) == NOT_SETUP
    assert np.all(dg == 7.0) and np.all(db == 7.0) and np.all(side == 7) and np.all(info == 7)
    # (a batch handle does not exist without a device: the checks on a live handle are in tests/test_gpu_adjoint_blocked.py)


class _Shape:
    """the attributes BatchLCQP._pairs reads"""
    B, nV, nd = 3, 5, 9


def test_python_wrappers_check_shapes():
    from lcqpow_amd import capi
    pairs = lambda VX, VY: capi.BatchLCQP._pairs(_Shape(), VX, VY, capi._arr)
    with pytest.raises(ValueError, match="both None"):
        pairs(None, None)
    for VX, VY in ((np.ones((3, 5)), None), (np.ones((3, 2, 4)), None), (np.ones((2, 2, 5)), None), (None, np.ones((3, 2, 5))),
                   (np.ones((3, 2, 5)), np.ones((3, 3, 9))), (np.ones((3, 0, 5)), None)):
        with pytest.raises(ValueError):
            pairs(VX, VY)
    VX, VY, k = pairs(np.ones((3, 2, 5)), np.ones((3, 2, 9)))
    assert k == 2 and VX.flags.c_contiguous and VY.dtype == np.float64
    assert pairs(None, np.ones((3, 4, 9)))[2] == 4 and pairs(np.ones((3, 1, 5)), None)[1] is None
    # the dual Jacobian goes through _jacobian with nd rows
    called = []
    ok = lambda *a: called.append(a[:2]) or 0
    Jyg, Jyb, side, info = capi._jacobian(ok, 3, 5, 9, 1, None, True, rows=9)
    assert called == [(1, 2)] and Jyg.shape == (2, 9, 5) and Jyb.shape == (2, 9, 9) and side.shape == (2, 9) and info.shape == (2,)
    assert capi._jacobian(ok, 3, 5, 9, 0, 3, False, rows=9)[1] is None
    with pytest.raises(ValueError):
        capi._jacobian(ok, 3, 5, 9, 2, 2, True, rows=9)


def test_layer_jacobian_keeps_its_default():
    from lcqpow_amd import diff
    p = inspect.signature(diff.BatchLCQPLayer.jacobian).parameters
    assert list(p) == ["self", "serial", "duals"] and p["duals"].default is False and p["serial"].default is None
    # the sparse layer has no dual blocks and keeps its signature
    assert list(inspect.signature(diff.SparseBatchLCQPLayer.jacobian).parameters) == ["self", "serial"]


class _Batch:
    """a batch object that records which Jacobian calls a layer makes"""
    B, nV, nd, device = 2, 3, 4, 0

    def __init__(self):
        self.calls = []

    def _jac(self, name, rows):
        self.calls.append(name)
        return (np.full((self.B, rows, self.nV), float(len(self.calls))), np.zeros((self.B, rows, self.nd)),
                np.zeros((self.B, self.nd), dtype=np.int32), np.zeros(self.B, dtype=np.int32))

    def jacobian(self, bounds=True):
        return self._jac("jacobian", self.nV)

    def jacobian_duals(self):
        return self._jac("jacobian_duals", self.nd)


def test_layer_jacobian_with_duals_takes_the_host_calls_for_a_host_solve():
    import torch
    from lcqpow_amd import diff
    bt = _Batch()
    layer = diff.BatchLCQPLayer(bt)
    layer.solves, layer._like = 1, (torch.float64, torch.device("cpu"))
    J = layer.jacobian(duals=True)
    assert bt.calls == ["jacobian", "jacobian_duals"] and layer.last_path == "host"
    assert J["xg"].shape == (2, 3, 3) and J["xb"].shape == (2, 3, 4) and J["yg"].shape == (2, 4, 3) and J["yb"].shape == (2, 4, 4)
    assert J["side"].shape == (2, 4) and torch.all(J["xg"] == 1.0) and torch.all(J["yg"] == 2.0) and J["yg"].dtype == torch.float64
    plain = layer.jacobian()
    assert isinstance(plain, torch.Tensor) and plain.shape == (2, 3, 3) and bt.calls[-1] == "jacobian"
    with pytest.raises(RuntimeError, match="not the layer's last one"):
        layer.jacobian(serial=7, duals=True)
