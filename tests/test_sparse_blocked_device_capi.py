"""The device-pointer twins of the sparse arm's panel calls (lcqp_hip_sparse_sensitivity_blocked_device, _adjoint_blocked_device,
_jacobian_device, _jacobian_duals_device; DESIGN.md section 3a''''', "The sparse arm: panels and Jacobians into device arrays") as far as a
machine without a GPU can hold them: declared in include/lcqp_hip.h, exported by the library, bound with argument types in capi.py, the
NULL-handle code, the methods of SparseBatchLCQP and what they refuse before any call, and SparseBatchLCQPLayer.jacobian_full on a recording
stand-in.  (What needs a handle is in tests/test_gpu_sparse_blocked_device.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

LCQPOBJECT_NOT_SETUP = 300
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, ci = ctypes.c_void_p, ctypes.c_int
DECLARATIONS = {
    "lcqp_hip_sparse_sensitivity_blocked_device": ("int lcqp_hip_sparse_sensitivity_blocked_device(lcqp_hip_sparse_t* s, int nrhs, const double* v, "
                                                   "double* dg, double* db, int* side, int* info, void* stream);", [vp, ci] + [vp] * 6),
    "lcqp_hip_sparse_adjoint_blocked_device": ("int lcqp_hip_sparse_adjoint_blocked_device(lcqp_hip_sparse_t* s, int nrhs, const double* vx, const double* vy, "
                                               "double* dg, double* db, int* side, int* info, void* stream);", [vp, ci] + [vp] * 7),
    "lcqp_hip_sparse_jacobian_device": ("int lcqp_hip_sparse_jacobian_device(lcqp_hip_sparse_t* s, int first, int count, "
                                        "double* Jg, double* Jb, int* side, int* info, void* stream);", [vp, ci, ci] + [vp] * 5),
    "lcqp_hip_sparse_jacobian_duals_device": ("int lcqp_hip_sparse_jacobian_duals_device(lcqp_hip_sparse_t* s, int first, int count, "
                                              "double* Jyg, double* Jyb, int* side, int* info, void* stream);", [vp, ci, ci] + [vp] * 5),
}


def test_the_symbols_are_declared_exported_and_bound():
    import lcqpow_amd as la
    raw = ctypes.CDLL(la.library_path())
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcqp_hip.h")).read(), flags=re.S))
    bound = la.lib()
    for name, (declaration, argtypes) in DECLARATIONS.items():
        assert hasattr(raw, name), name
        assert declaration in header, name
        assert getattr(bound, name).argtypes == argtypes, name


def test_null_handle():
    import lcqpow_amd as la
    L = la.lib()
    n = [None]
    assert L.lcqp_hip_sparse_sensitivity_blocked_device(None, 1, *n * 6) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_adjoint_blocked_device(None, 1, *n * 7) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_jacobian_device(None, 0, 1, *n * 5) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_jacobian_duals_device(None, 0, 1, *n * 5) == LCQPOBJECT_NOT_SETUP
    # the handle comes first: arguments no host twin would accept do not change the code
    assert L.lcqp_hip_sparse_sensitivity_blocked_device(None, 0, *n * 6) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_jacobian_duals_device(None, -1, 0, *n * 5) == LCQPOBJECT_NOT_SETUP


def test_the_methods_have_the_signatures_of_the_dense_twins():
    import lcqpow_amd as la
    S, D = la.SparseBatchLCQP, la.BatchLCQP
    for name in ("adjoint_blocked_device", "jacobian_device", "jacobian_duals_device"):
        assert inspect.signature(getattr(S, name)) == inspect.signature(getattr(D, name)), name
    assert list(inspect.signature(S.sensitivity_blocked_device).parameters) == ["self", "V"]
    assert list(inspect.signature(S.adjoint_blocked_device).parameters) == ["self", "VX", "VY"]
    assert inspect.signature(S.adjoint_blocked_device).parameters["VY"].default is None
    for name in ("jacobian_device", "jacobian_duals_device"):
        p = inspect.signature(getattr(S, name)).parameters
        assert list(p) == ["self", "first", "count", "bounds"] and (p["first"].default, p["count"].default, p["bounds"].default) == (0, None, True)
    # existing signatures stay
    assert list(inspect.signature(S.sensitivity_device).parameters) == ["self", "v"]
    assert list(inspect.signature(D.sensitivity_device).parameters) == ["self", "v", "blocked"]


def shell(B=2, nV=4, nC=3, nComp=1):
    """a SparseBatchLCQP without a handle: the wrappers must refuse their arguments before they would use one"""
    import lcqpow_amd
    sb = object.__new__(lcqpow_amd.SparseBatchLCQP)
    sb.B, sb.nV, sb.nC, sb.nComp, sb.device, sb.h = B, nV, nC, nComp, 0, None
    sb.m = sb.nd = sb._ndual = nC + 2 * nComp
    return sb


def test_wrappers_refuse_what_is_not_a_device_tensor():
    import torch
    sb = shell()
    B, n, m = sb.B, sb.nV, sb.m
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    with pytest.raises(ValueError, match="torch tensor"):
        sb.sensitivity_blocked_device(np.zeros((B, 3, n)))
    with pytest.raises(ValueError, match="torch tensor"):
        sb.adjoint_blocked_device(np.zeros((B, 3, n)))
    with pytest.raises(ValueError, match="torch tensor"):
        sb.adjoint_blocked_device(None, np.zeros((B, 3, m)))
    with pytest.raises(ValueError, match="both None"):
        sb.adjoint_blocked_device(None, None)
    with pytest.raises(ValueError, match="cuda:0"):
        sb.sensitivity_blocked_device(t(B, 3, n))
    with pytest.raises(ValueError, match="cuda:0"):
        sb.adjoint_blocked_device(None, t(B, 3, m))
    with pytest.raises(ValueError):      # [B][nV]: the blocked calls take [B][k][nV]
        sb.sensitivity_blocked_device(t(B, n))
    with pytest.raises(ValueError):
        sb.sensitivity_blocked_device(t(B, 0, n))
    with pytest.raises(ValueError):
        sb.adjoint_blocked_device(t(B, 3, n), t(B, 2, m))
    for call in (sb.jacobian_device, sb.jacobian_duals_device):
        with pytest.raises(ValueError, match="outside the batch"):
            call(first=1, count=B)
        with pytest.raises(ValueError, match="outside the batch"):
            call(first=-1)
        with pytest.raises(ValueError, match="outside the batch"):
            call(count=0)


class _Batch:
    """a batch object that records which Jacobian calls a layer makes; it has the host calls only"""
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


def test_layer_jacobian_full_chooses_the_path_by_the_device_of_g():
    """g on the host: the two host calls, as before.  g on the GPU of the batch: the two device twins (a stand-in without them would raise
    AttributeError: the layer does not fall back)."""
    import torch
    from lcqpow_amd import diff
    bt = _Batch()
    layer = diff.SparseBatchLCQPLayer(bt)
    layer.solves, layer._like = 1, (torch.float64, torch.device("cpu"))
    J = layer.jacobian_full()
    assert bt.calls == ["jacobian", "jacobian_duals"] and layer.last_path == "host" and sorted(J) == ["info", "side", "xb", "xg", "yb", "yg"]
    layer._like = (torch.float64, torch.device("cuda", 0))
    with pytest.raises(AttributeError, match="jacobian_device"):
        layer.jacobian_full()
    assert layer.last_path == "device" and len(bt.calls) == 2
    doc = diff.SparseBatchLCQPLayer.jacobian_full.__doc__
    assert "no device-pointer twins" not in doc and "jacobian_device" in doc
