"""The re-solve entry points of the C ABI on a box without a device: exported, bound by the Python layer, and refusing a NULL handle
before any device call.  (What needs a batch object -- ranges, rho0, the box pattern -- is in tests/test_gpu_resolve.py: without a GPU
no batch can be created.)"""
import ctypes

import numpy as np
import pytest


def test_resolve_entry_points_reject_null_handles():
    import lcqpow_amd as la
    L = la.lib()
    g = np.zeros(4); gp = g.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = (ctypes.c_int * 2)(-7, -7)
    assert L.lcqp_hip_batch_update(None, 0, 1, gp, *[None] * 10) == 300           # LCQP_LCQPOBJECT_NOT_SETUP, as run / setup
    assert L.lcqp_hip_batch_resolve(None, 0, None) == 300 and L.lcqp_hip_batch_resolve(None, 1, gp) == 300
    assert L.lcqp_hip_batch_launch_counts(None, out) == 100 and (out[0], out[1]) == (-7, -7)


def test_python_layer_binds_the_resolve_entry_points():
    import inspect
    import lcqpow_amd as la
    la.lib()
    sig = inspect.signature(la.BatchLCQP.update)
    assert list(sig.parameters)[1:4] == ["first", "count", "g"] and "Q" not in sig.parameters
    assert list(inspect.signature(la.BatchLCQP.resolve).parameters) == ["self", "warm", "rho0"]
    assert callable(la.BatchLCQP.launch_counts)
    assert "resolve" in inspect.signature(la.BatchPipeline.launch).parameters
    with pytest.raises(ValueError, match="rho0"):
        la.capi._sized("rho0", la.capi._arr(np.ones(3)), 2)
