"""The values-only update of the sparse batch at the C ABI on a box without a device: lcqp_hip_sparse_update_values and its device twin are
exported with the prototypes of include/lcqp_hip.h, bound by the Python layer, and answer a call without any array and a NULL handle with
their codes before any device call; the sparse torch layer has the warm_matrices switch, off by default.  (What needs a batch object --
ranges, instances without a problem, the bits -- is in tests/test_gpu_sparse_value_resolve.py: without a GPU no batch can be created.)"""
import ctypes
import inspect

import numpy as np

from test_matrix_resolve_capi import INVALID_ARGUMENT, NOT_SETUP, prototype


def test_the_two_symbols_have_the_documented_prototypes():
    import lcqpow_amd as la
    L = la.lib()
    DP, VP, I = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_int
    assert prototype("lcqp_hip_sparse_update_values") == ["lcqp_hip_sparse_t*", "int", "int"] + ["double*"] * 2
    assert prototype("lcqp_hip_sparse_update_values_device") == ["lcqp_hip_sparse_t*", "int", "int", "int"] + ["double*"] * 2 + ["void*"]
    assert L.lcqp_hip_sparse_update_values.argtypes == [VP, I, I] + [DP] * 2
    assert L.lcqp_hip_sparse_update_values_device.argtypes == [VP, I, I, I] + [VP] * 3
    assert list(inspect.signature(la.SparseBatchLCQP.update_values).parameters) == ["self", "first", "count", "Qx", "Ax"]
    assert list(inspect.signature(la.SparseBatchLCQP.update_values_device).parameters) == ["self", "first", "count", "Qx", "Ax", "shared"]


def test_no_array_and_null_handle_are_answered_without_a_device():
    import lcqpow_amd as la
    L = la.lib()
    v = np.ones(4); vp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    addr = ctypes.c_void_p(v.ctypes.data)      # (never dereferenced: the handle is checked first)
    # both arrays NULL: LCQP_INVALID_ARGUMENT, the first check of both calls
    assert L.lcqp_hip_sparse_update_values(None, 0, 1, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_update_values_device(None, 0, 1, 0, None, None, None) == INVALID_ARGUMENT
    # a NULL handle: LCQP_LCQPOBJECT_NOT_SETUP, as lcqp_hip_sparse_update / _update_device
    for k in range(2):
        arrays = [None] * 2
        arrays[k] = vp
        assert L.lcqp_hip_sparse_update_values(None, 0, 1, *arrays) == NOT_SETUP
        arrays[k] = addr
        assert L.lcqp_hip_sparse_update_values_device(None, 0, 1, 0, *arrays, None) == NOT_SETUP
        assert L.lcqp_hip_sparse_update_values_device(None, 0, 1, 4, *arrays, None) == NOT_SETUP      # (the handle comes before `shared`)


def test_the_sparse_layer_has_the_switch_off_by_default():
    from lcqpow_amd import diff
    p = inspect.signature(diff.SparseBatchLCQPLayer.__init__).parameters
    assert "warm_matrices" in p and p["warm_matrices"].default is False
    assert list(inspect.signature(diff.SparseBatchLCQPLayer.solve).parameters) == ["self", "g", "Qx", "Ax", "lbA", "ubA"]
