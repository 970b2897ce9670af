"""The full adjoint of the sparse arm at the C ABI, without a device: lcqp_hip_sparse_adjoint and lcqp_hip_sparse_set_adjoint_staging are
exported with the signatures include/lcqp_hip.h documents, bound by the Python layer, and their argument checks come before any device
call and in the documented order (they answer on a box without a GPU, and before the handle is dereferenced: the handle of the checks
below is a block of zero bytes, whose zero setup mark answers LCQP_LCQPOBJECT_NOT_SETUP once the arguments pass).  What needs a solved
batch is in tests/test_gpu_sparse_adjoint.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NOT_SETUP = 100, 300
dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

SIGNATURES = {
    "lcqp_hip_sparse_adjoint": "lcqp_hip_sparse_t* s, const double* vx, const double* vy, double* dg, double* db, int* side, int* info, "
                               "int reduce, double* dQx, double* dAx",
    "lcqp_hip_sparse_set_adjoint_staging": "lcqp_hip_sparse_t* s, size_t bytes",
}


def test_symbols_are_exported_with_the_documented_signatures():
    import lcqpow_amd
    L = ctypes.CDLL(lcqpow_amd.library_path())
    src = open(os.path.join(ROOT, "include", "lcqp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, args in SIGNATURES.items():
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args
    # the binding declares the same arguments
    from lcqpow_amd import capi
    B = capi.lib()
    assert B.lcqp_hip_sparse_adjoint.argtypes == [ctypes.c_void_p, dp, dp, dp, dp, ip, ip, ctypes.c_int, dp, dp]
    assert len(B.lcqp_hip_sparse_adjoint.argtypes) == 10
    assert B.lcqp_hip_sparse_set_adjoint_staging.argtypes == [ctypes.c_void_p, ctypes.c_size_t]


def test_argument_checks_need_no_device_and_come_in_the_documented_order():
    import lcqpow_amd as la
    L = la.lib()
    n, m, nnz = 4, 6, 5
    vx = np.ones(n); vy = np.ones(m); dg = np.full(n, 7.0); db = np.full(m, 7.0)
    side, info = np.full(m, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    dQx, dAx = np.full(nnz, 7.0), np.full(nnz, 7.0)
    P = lambda a: a.ctypes.data_as(dp)
    I = lambda a: a.ctypes.data_as(ip)
    rest = (P(db), I(side), I(info))
    mats = (P(dQx), P(dAx))
    adj = L.lcqp_hip_sparse_adjoint
    stand_in = ctypes.create_string_buffer(1 << 16)      # zero bytes: never a live handle, its setup mark reads "not solved"
    fake = ctypes.cast(stand_in, ctypes.c_void_p)
    # a NULL handle
    assert adj(None, P(vx), P(vy), P(dg), *rest, 0, *mats) == INVALID_ARGUMENT
    assert adj(None, P(vx), None, P(dg), None, None, None, 1, None, None) == INVALID_ARGUMENT
    # NULL vx or dg, reduce outside 0 / 1: refused on the arguments, before the mark of the handle is looked at
    assert adj(fake, None, P(vy), P(dg), *rest, 0, *mats) == INVALID_ARGUMENT
    assert adj(fake, P(vx), P(vy), None, *rest, 0, *mats) == INVALID_ARGUMENT
    assert adj(fake, P(vx), P(vy), P(dg), *rest, 2, *mats) == INVALID_ARGUMENT
    assert adj(fake, P(vx), P(vy), P(dg), *rest, -1, *mats) == INVALID_ARGUMENT
    # then the state: good arguments on a handle that never solved
    assert adj(fake, P(vx), P(vy), P(dg), *rest, 0, *mats) == NOT_SETUP
    assert adj(fake, P(vx), None, P(dg), None, None, None, 1, None, None) == NOT_SETUP
    assert L.lcqp_hip_sparse_set_adjoint_staging(None, 1) == INVALID_ARGUMENT
    for a in (dg, db, dQx, dAx):
        assert np.all(a == 7.0)
    assert np.all(side == 7) and np.all(info == 7)
    assert not any(stand_in.raw)      # and nothing was written into the stand-in


def test_python_layer_has_the_sparse_adjoint():
    import lcqpow_amd as la
    from lcqpow_amd import diff
    assert list(inspect.signature(la.SparseBatchLCQP.adjoint).parameters) == ["self", "vx", "vy", "matrices", "reduce", "_staging_bytes"]
    assert inspect.signature(la.SparseBatchLCQP.adjoint).parameters["matrices"].default == ("Q", "A")
    assert list(inspect.signature(diff.SparseBatchLCQPLayer.solve).parameters) == ["self", "g", "Qx", "Ax", "lbA", "ubA"]
    assert "values" in inspect.signature(diff.SparseBatchLCQPLayer.__init__).parameters
    # the dense layer's solve is the one it was
    assert list(inspect.signature(diff.BatchLCQPLayer.solve).parameters) == ["self", "g", "Q", "A", "L", "R", "lbA", "ubA"]


def test_solve_with_a_matrix_tensor_needs_the_values():
    """decided before the batch object is touched: a stand-in with the sizes is enough"""
    import torch
    from lcqpow_amd import diff

    class Sizes:
        B, nV, nC, nComp, m, nnzQ, nnzA = 2, 4, 1, 1, 3, 6, 5
    layer = diff.SparseBatchLCQPLayer(Sizes(), bounds=None)
    with pytest.raises(ValueError, match="values"):
        layer.solve(torch.zeros(2, 4, dtype=torch.float64), Qx=torch.ones(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="Qx"):
        diff.SparseBatchLCQPLayer(Sizes(), values=dict(Qx=np.ones(5), Ax=np.ones(5)))
    with pytest.raises(ValueError, match="keys"):
        diff.SparseBatchLCQPLayer(Sizes(), values=dict(Qx=np.ones(6)))
    held = diff.SparseBatchLCQPLayer(Sizes(), values=dict(Qx=np.ones(6), Ax=np.ones((2, 5)))).values
    assert held["Qx"].shape == (2, 6) and held["Ax"].shape == (2, 5)
