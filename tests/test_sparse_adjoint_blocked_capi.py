"""lcqp_hip_sparse_adjoint_blocked / lcqp_hip_sparse_jacobian_duals (DESIGN.md section 3a'''', "The sparse arm: panels with gradients on y") on
a box without a device: the symbols in the header, the library and capi.py, the answers that need no handle, the shape checks of the Python
wrappers, SparseBatchLCQPLayer.jacobian_full on a recording stand-in, and the signatures that stay.  (What needs a handle is in
tests/test_gpu_sparse_adjoint_blocked.py: without a GPU no sparse batch can be created.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)
INVALID_ARGUMENT = 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_are_declared_exported_and_bound():
    import lcqpow_amd as la
    L = ctypes.CDLL(la.library_path())
    for name in ("lcqp_hip_sparse_adjoint_blocked", "lcqp_hip_sparse_jacobian_duals"):
        assert hasattr(L, name), name
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcqp_hip.h")).read(), flags=re.S))
    assert ("int lcqp_hip_sparse_adjoint_blocked(lcqp_hip_sparse_t* s, int nrhs, const double* vx, const double* vy, "
            "double* dg, double* db, int* side, int* info);") in header
    assert ("int lcqp_hip_sparse_jacobian_duals(lcqp_hip_sparse_t* s, int first, int count, "
            "double* Jyg, double* Jyb, int* side, int* info);") in header
    B = la.lib()
    assert B.lcqp_hip_sparse_adjoint_blocked.argtypes == [ctypes.c_void_p, ctypes.c_int, dp, dp, dp, dp, ip, ip]
    assert B.lcqp_hip_sparse_jacobian_duals.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, dp, dp, ip, ip]


def test_bad_arguments_are_refused_before_the_handle_is_read():
    import lcqpow_amd as la
    L = la.lib()
    vx, vy, dg, db = np.ones(4), np.ones(6), np.full(24, 7.0), np.full(36, 7.0)
    side, info = np.full(6, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    rest = (db.ctypes.data_as(dp), side.ctypes.data_as(ip), info.ctypes.data_as(ip))
    xp, yp, gp = vx.ctypes.data_as(dp), vy.ctypes.data_as(dp), dg.ctypes.data_as(dp)
    assert L.lcqp_hip_sparse_adjoint_blocked(None, 1, xp, yp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_adjoint_blocked(None, 1, None, None, gp, None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian_duals(None, 0, 1, gp, *rest) == INVALID_ARGUMENT
    # The argument checks that do not need the batch size come before any use of the handle, so a block of zero bytes can stand in for one
    # (tests/test_sparse_sensitivity_blocked_capi.py).  Its B reads as 0, so every range is outside it; its zero setup mark would answer 300.
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(stand_in, ctypes.c_void_p)
    assert L.lcqp_hip_sparse_adjoint_blocked(h, 1, None, None, gp, *rest) == INVALID_ARGUMENT       # both NULL
    assert L.lcqp_hip_sparse_adjoint_blocked(h, 1, xp, yp, None, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_adjoint_blocked(h, 0, xp, yp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_adjoint_blocked(h, -2, None, yp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian_duals(h, 0, 1, None, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian_duals(h, -1, 1, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian_duals(h, 0, 0, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian_duals(h, 0, -3, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian_duals(h, 0, 1, gp, *rest) == INVALID_ARGUMENT              # first + count > B (= 0 in the stand-in)
    assert L.lcqp_hip_sparse_jacobian_duals(h, 2 ** 31 - 1, 2 ** 31 - 1, gp, *rest) == INVALID_ARGUMENT      # the sum does not wrap
    assert np.all(dg == 7.0) and np.all(db == 7.0) and np.all(side == 7) and np.all(info == 7)


class _Shape:
    """the attributes _pairs reads"""
    B, nV, nd = 3, 5, 9


def test_python_wrappers_check_shapes():
    from lcqpow_amd import capi
    assert capi.SparseBatchLCQP._pairs is capi.BatchLCQP._pairs      # one body for both arms
    pairs = lambda VX, VY: capi.SparseBatchLCQP._pairs(_Shape(), VX, VY, capi._arr)
    with pytest.raises(ValueError, match="both None"):
        pairs(None, None)
    for VX, VY in ((np.ones((3, 5)), None), (np.ones((3, 2, 4)), None), (np.ones((2, 2, 5)), None), (None, np.ones((3, 2, 5))),
                   (np.ones((3, 2, 5)), np.ones((3, 3, 9))), (np.ones((3, 0, 5)), None)):
        with pytest.raises(ValueError):
            pairs(VX, VY)
    VX, VY, k = pairs(np.ones((3, 2, 5)), np.ones((3, 2, 9)))
    assert k == 2 and VX.flags.c_contiguous and VY.dtype == np.float64
    assert pairs(None, np.ones((3, 4, 9)))[2] == 4 and pairs(np.ones((3, 1, 5)), None)[1] is None
    # the dual Jacobian goes through _jacobian with m rows
    called = []
    ok = lambda *a: called.append(a[:2]) or 0
    Jyg, Jyb, side, info = capi._jacobian(ok, 3, 5, 9, 1, None, True, rows=9)
    assert called == [(1, 2)] and Jyg.shape == (2, 9, 5) and Jyb.shape == (2, 9, 9) and side.shape == (2, 9) and info.shape == (2,)
    with pytest.raises(ValueError):
        capi._jacobian(ok, 3, 5, 9, 2, 2, True, rows=9)


def test_signatures():
    import lcqpow_amd as la
    from lcqpow_amd import diff
    S, D = la.SparseBatchLCQP, la.BatchLCQP
    assert list(inspect.signature(S.adjoint_blocked).parameters) == ["self", "VX", "VY"]
    assert inspect.signature(S.adjoint_blocked).parameters["VY"].default is None
    p = inspect.signature(S.jacobian_duals).parameters
    assert list(p) == ["self", "first", "count", "bounds", "_staging_bytes"]
    assert (p["first"].default, p["count"].default, p["bounds"].default, p["_staging_bytes"].default) == (0, None, True, None)
    assert inspect.signature(S.adjoint_blocked) == inspect.signature(D.adjoint_blocked)
    assert inspect.signature(S.jacobian_duals) == inspect.signature(D.jacobian_duals)
    p = inspect.signature(diff.SparseBatchLCQPLayer.jacobian_full).parameters
    assert list(p) == ["self", "serial"] and p["serial"].default is None
    # existing signatures stay
    assert list(inspect.signature(S.sensitivity_blocked).parameters) == ["self", "v"]
    assert list(inspect.signature(S.jacobian).parameters) == ["self", "first", "count", "bounds", "_staging_bytes"]
    assert list(inspect.signature(S.adjoint).parameters) == ["self", "vx", "vy", "matrices", "reduce", "_staging_bytes"]
    assert list(inspect.signature(diff.SparseBatchLCQPLayer.jacobian).parameters) == ["self", "serial"]
    p = inspect.signature(diff.BatchLCQPLayer.jacobian).parameters
    assert list(p) == ["self", "serial", "duals"] and p["duals"].default is False


class _Batch:
    """a batch object that records which Jacobian calls a layer makes"""
    B, nV, m, device = 2, 3, 4, 0

    def __init__(self):
        self.calls = []

    def _jac(self, name, rows):
        self.calls.append(name)
        return (np.full((self.B, rows, self.nV), float(len(self.calls))), np.zeros((self.B, rows, self.m)),
                np.full((self.B, self.m), 2, dtype=np.int32), np.arange(self.B, dtype=np.int32) * 4)

    def jacobian(self, bounds=True):
        return self._jac("jacobian", self.nV)

    def jacobian_duals(self):
        return self._jac("jacobian_duals", self.m)


def test_layer_jacobian_full_takes_the_two_host_calls():
    import torch
    from lcqpow_amd import diff
    bt = _Batch()
    layer = diff.SparseBatchLCQPLayer(bt)
    with pytest.raises(RuntimeError, match="not the layer's last one"):
        layer.jacobian_full()                                # nothing solved yet
    layer.solves, layer._like = 1, (torch.float64, torch.device("cpu"))
    J = layer.jacobian_full()
    assert bt.calls == ["jacobian", "jacobian_duals"] and layer.last_path == "host"
    assert sorted(J) == ["info", "side", "xb", "xg", "yb", "yg"]
    assert J["xg"].shape == (2, 3, 3) and J["xb"].shape == (2, 3, 4) and J["yg"].shape == (2, 4, 3) and J["yb"].shape == (2, 4, 4)
    assert J["side"].shape == (2, 4) and torch.all(J["side"] == 2) and J["info"].tolist() == [0, 4] and list(layer.info) == [0, 4]
    assert torch.all(J["xg"] == 1.0) and torch.all(J["yg"] == 2.0) and J["yg"].dtype == torch.float64
    plain = layer.jacobian()
    assert isinstance(plain, torch.Tensor) and plain.shape == (2, 3, 3) and bt.calls[-1] == "jacobian"
    with pytest.raises(RuntimeError, match="not the layer's last one"):
        layer.jacobian_full(serial=7)
