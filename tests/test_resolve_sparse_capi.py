"""The re-solve entry points of the sparse arm's C ABI on a box without a device: exported, bound by the Python layer, and refusing a
NULL handle before any device call.  (What needs a handle -- ranges, rho0, the bits -- is in tests/test_gpu_sparse_resolve.py: without a
GPU no sparse batch can be created.)"""
import ctypes
import inspect

import numpy as np
import pytest


def test_library_exports_the_sparse_resolve_entry_points():
    import lcqpow_amd as la
    L = ctypes.CDLL(la.library_path())
    for name in ("lcqp_hip_sparse_update", "lcqp_hip_sparse_resolve", "lcqp_hip_sparse_launch_counts"):
        assert hasattr(L, name), name


def test_sparse_resolve_entry_points_reject_null_handles():
    import lcqpow_amd as la
    L = la.lib()
    g = np.ones(4); gp = g.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = (ctypes.c_int * 2)(-7, -7)
    assert L.lcqp_hip_sparse_update(None, 0, 1, gp, *[None] * 8) == 300            # LCQP_LCQPOBJECT_NOT_SETUP, as run
    assert L.lcqp_hip_sparse_resolve(None, 0, None) == 300 and L.lcqp_hip_sparse_resolve(None, 1, gp) == 300
    assert L.lcqp_hip_sparse_launch_counts(None, out) == 100 and (out[0], out[1]) == (-7, -7)


def test_python_layer_binds_the_sparse_resolve_entry_points():
    import lcqpow_amd as la
    L = la.lib()
    assert len(L.lcqp_hip_sparse_update.argtypes) == 12 and len(L.lcqp_hip_sparse_resolve.argtypes) == 3
    sig = inspect.signature(la.SparseBatchLCQP.update)
    assert list(sig.parameters)[:4] == ["self", "first", "count", "g"]
    assert "Qx" not in sig.parameters and "Ax" not in sig.parameters
    assert list(sig.parameters)[4:] == ["lbA", "ubA", "lbL", "ubL", "lbR", "ubR", "x0", "y0"]       # the order of load without the matrices
    assert list(inspect.signature(la.SparseBatchLCQP.resolve).parameters) == ["self", "warm", "rho0"]
    assert callable(la.SparseBatchLCQP.launch_counts)
    with pytest.raises(ValueError, match="rho0"):
        la.capi._sized("rho0", la.capi._arr(np.ones(3)), 2)
