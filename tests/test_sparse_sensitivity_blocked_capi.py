"""lcqp_hip_sparse_sens_panel / lcqp_hip_sparse_sensitivity_blocked / lcqp_hip_sparse_jacobian on a box without a device: exported with the
documented signatures, bound by the Python layer, refusing bad arguments before the handle is looked at.  (What needs a handle is in
tests/test_gpu_sparse_sensitivity_blocked.py: without a GPU no sparse batch can be created.)"""
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
    for name in ("lcqp_hip_sparse_sens_panel", "lcqp_hip_sparse_sensitivity_blocked", "lcqp_hip_sparse_jacobian"):
        assert hasattr(L, name), name
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lcqp_hip.h")).read())
    assert "#define LCQP_SPARSE_SENS_PANEL 8" in header
    assert "int lcqp_hip_sparse_sens_panel(const lcqp_hip_sparse_t* s);" in header
    assert ("int lcqp_hip_sparse_sensitivity_blocked(lcqp_hip_sparse_t* s, int nrhs, const double* v, double* dg, double* db, int* side, int* info);"
            in header)
    assert "int lcqp_hip_sparse_jacobian(lcqp_hip_sparse_t* s, int first, int count, double* Jg, double* Jb, int* side, int* info);" in header
    B = la.lib()
    assert B.lcqp_hip_sparse_sens_panel.argtypes == [ctypes.c_void_p]
    assert B.lcqp_hip_sparse_sensitivity_blocked.argtypes == [ctypes.c_void_p, ctypes.c_int, dp, dp, dp, ip, ip]
    assert B.lcqp_hip_sparse_jacobian.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, dp, dp, ip, ip]


def test_bad_arguments_are_refused_before_the_handle_is_read():
    import lcqpow_amd as la
    L = la.lib()
    v, dg, db = np.ones(4), np.full(16, 7.0), np.full(24, 7.0)
    side, info = np.full(6, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    rest = (db.ctypes.data_as(dp), side.ctypes.data_as(ip), info.ctypes.data_as(ip))
    vp, gp = v.ctypes.data_as(dp), dg.ctypes.data_as(dp)
    assert L.lcqp_hip_sparse_sens_panel(None) == 0
    assert L.lcqp_hip_sparse_sensitivity_blocked(None, 1, vp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity_blocked(None, 1, vp, gp, None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian(None, 0, 1, gp, *rest) == INVALID_ARGUMENT
    # The argument checks that do not need the batch size come before any use of the handle, so a block of zero bytes can stand in for one
    # (tests/test_sparse_sensitivity_capi.py).  Its B reads as 0, so every range is outside it; its zero setup mark would answer 300.
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(stand_in, ctypes.c_void_p)
    assert L.lcqp_hip_sparse_sensitivity_blocked(h, 1, None, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity_blocked(h, 1, vp, None, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity_blocked(h, 0, vp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_sensitivity_blocked(h, -2, vp, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian(h, 0, 1, None, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian(h, -1, 1, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian(h, 0, 0, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian(h, 0, -3, gp, *rest) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian(h, 0, 1, gp, *rest) == INVALID_ARGUMENT              # first + count > B (= 0 in the stand-in)
    assert L.lcqp_hip_sparse_jacobian(h, 2 ** 31 - 1, 2 ** 31 - 1, gp, *rest) == INVALID_ARGUMENT      # the sum does not wrap
    assert np.all(dg == 7.0) and np.all(db == 7.0) and np.all(side == 7) and np.all(info == 7)


def test_python_layer_has_the_blocked_calls():
    import lcqpow_amd as la
    from lcqpow_amd import diff
    assert list(inspect.signature(la.SparseBatchLCQP.sensitivity_blocked).parameters) == ["self", "v"]
    assert list(inspect.signature(la.SparseBatchLCQP.jacobian).parameters) == ["self", "first", "count", "bounds", "_staging_bytes"]
    assert list(inspect.signature(la.BatchLCQP.jacobian).parameters) == list(inspect.signature(la.SparseBatchLCQP.jacobian).parameters)
    assert callable(la.SparseBatchLCQP.sens_panel)
    assert "only the dense arm" not in inspect.getsource(diff.BatchLCQPLayer.jacobian)
    assert list(inspect.signature(diff.SparseBatchLCQPLayer.jacobian).parameters) == ["self", "serial"]
