"""lcqp_hip_sparse_sensitivity / lcqp_hip_sparse_sensitivity_timing on a box without a device: exported with the documented signatures,
bound by the Python layer, refusing bad arguments before the handle is looked at, and the sparse layout of split_bound_derivatives.
(What needs a handle -- the derivatives, the flags, the state errors -- is in tests/test_gpu_sparse_sensitivity.py: without a GPU no
sparse batch can be created.)"""
import ctypes
import inspect
import os
import re

import numpy as np

dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)
INVALID_ARGUMENT = 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_points_with_the_documented_signatures():
    import lcqpow_amd as la
    L = ctypes.CDLL(la.library_path())
    for name in ("lcqp_hip_sparse_sensitivity", "lcqp_hip_sparse_sensitivity_timing"):
        assert hasattr(L, name), name
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lcqp_hip.h")).read())
    assert ("int lcqp_hip_sparse_sensitivity(lcqp_hip_sparse_t* s, int nrhs, const double* v, double* dg, double* db, int* side, int* info);"
            in header)
    assert "int lcqp_hip_sparse_sensitivity_timing(lcqp_hip_sparse_t* s, float* kernel_ms);" in header
    B = la.lib()
    assert B.lcqp_hip_sparse_sensitivity.argtypes == [ctypes.c_void_p, ctypes.c_int, dp, dp, dp, ip, ip]
    assert B.lcqp_hip_sparse_sensitivity_timing.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]


def test_bad_arguments_are_refused_before_the_handle_is_read():
    import lcqpow_amd as la
    L = la.lib()
    v, dg, db = np.ones(4), np.full(4, 7.0), np.full(6, 7.0)
    side, info = np.full(6, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    rest = (db.ctypes.data_as(dp), side.ctypes.data_as(ip), info.ctypes.data_as(ip))
    vp, gp = v.ctypes.data_as(dp), dg.ctypes.data_as(dp)
    assert L.lcqp_hip_sparse_sensitivity(None, 1, vp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity(None, 1, vp, gp, None, None, None) == INVALID_ARGUMENT
    # The argument checks come before any use of the handle, so a block of zero bytes can stand in for one here (no sparse handle exists
    # without a device).  Were the handle read first, its zero setup mark would answer LCQP_LCQPOBJECT_NOT_SETUP (300) instead.
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(stand_in, ctypes.c_void_p)
    assert L.lcqp_hip_sparse_sensitivity(h, 1, None, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity(h, 1, vp, None, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity(h, 0, vp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity(h, -2, vp, gp, *rest) == INVALID_ARGUMENT
    ms = ctypes.c_float(-1.0)
    assert L.lcqp_hip_sparse_sensitivity_timing(None, ctypes.byref(ms)) == INVALID_ARGUMENT and ms.value == -1.0
    assert L.lcqp_hip_sparse_sensitivity_timing(h, None) == INVALID_ARGUMENT
    assert np.all(dg == 7.0) and np.all(db == 7.0) and np.all(side == 7) and np.all(info == 7)


def test_python_layer_has_the_sparse_sensitivity():
    import lcqpow_amd as la
    from lcqpow_amd import diff
    assert list(inspect.signature(la.SparseBatchLCQP.sensitivity).parameters) == ["self", "v"]
    assert callable(la.SparseBatchLCQP.sensitivity_kernel_ms)
    assert issubclass(diff.SparseBatchLCQPLayer, diff.BatchLCQPLayer) and diff.SparseBatchLCQPLayer.sparse
    assert "lb" not in diff.SparseBatchLCQPLayer.bound_keys and "lbA" in diff.SparseBatchLCQPLayer.bound_keys


def test_split_bound_derivatives_sparse_layout():
    from lcqpow_amd import split_bound_derivatives
    nV, nC, nComp = 5, 3, 2
    #                 A           L      R
    side = np.array([[1, 2, 0, -1, 0, 0, -1]])
    db = np.arange(1.0, 8.0)[None]
    p = split_bound_derivatives(db, side, nV, nC, nComp, sparse=True)
    assert p["dlb"].shape == (1, 0) and p["dub"].shape == (1, 0)                           # no box block
    assert p["dlbA"].tolist() == [[0, 2, 0]] and p["dubA"].tolist() == [[1, 2, 0]]         # the equality row: its one value under both bounds
    assert p["dlbL"].tolist() == [[4, 0]] and p["dubL"].tolist() == [[0, 0]]
    assert p["dlbR"].tolist() == [[0, 7]] and p["dubR"].tolist() == [[0, 0]]
    p3 = split_bound_derivatives(np.stack([db, 2 * db], axis=1), side, nV, nC, nComp, sparse=True)      # [B][k][m]
    assert p3["dubA"].shape == (1, 2, 3) and p3["dubA"][0, 1].tolist() == [2, 4, 0] and p3["dlbR"][0, 1].tolist() == [0, 14]
    dense = split_bound_derivatives(np.zeros((1, nV + 7)), np.zeros((1, nV + 7), dtype=int), nV, nC, nComp)
    assert dense["dlb"].shape == (1, nV) and dense["dlbR"].shape == (1, nComp)             # the default layout is unchanged
