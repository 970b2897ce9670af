"""The matrix-only update of the dense batch at the C ABI on a box without a device: lcqp_hip_batch_update_matrices and its device twin
are exported with the prototypes of include/lcqp_hip.h, bound by the Python layer, and answer a call without any matrix and a NULL handle
with their codes before any device call.  (What needs a batch object -- ranges, instances without a problem, the bits -- is in
tests/test_gpu_matrix_resolve.py: without a GPU no batch can be created.)"""
import ctypes
import inspect
import os
import re

import numpy as np

INVALID_ARGUMENT, NOT_SETUP = 100, 300
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lcqp_hip.h")


def prototype(name):
    """the parameter types of `name` as the header declares it, qualifiers and parameter names dropped"""
    text = open(HEADER).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % re.escape(name), text)
    assert m, name + " is not declared in include/lcqp_hip.h"
    types = []
    for p in m.group(1).split(","):
        p = re.sub(r"\bconst\b", "", p).strip()
        types.append(re.sub(r"\s*\w+$", "", p).replace(" ", ""))
    return types


def test_the_two_symbols_have_the_documented_prototypes():
    import lcqpow_amd as la
    L = la.lib()
    DP, VP, I = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_int
    assert prototype("lcqp_hip_batch_update_matrices") == ["lcqp_hip_batch_t*", "int", "int"] + ["double*"] * 4
    assert prototype("lcqp_hip_batch_update_matrices_device") == ["lcqp_hip_batch_t*", "int", "int", "int"] + ["double*"] * 4 + ["void*"]
    assert L.lcqp_hip_batch_update_matrices.argtypes == [VP, I, I] + [DP] * 4
    assert L.lcqp_hip_batch_update_matrices_device.argtypes == [VP, I, I, I] + [VP] * 5
    assert list(inspect.signature(la.BatchLCQP.update_matrices).parameters) == ["self", "first", "count", "Q", "L", "R", "A"]
    assert list(inspect.signature(la.BatchLCQP.update_matrices_device).parameters) == ["self", "first", "count", "Q", "L", "R", "A", "shared"]
    assert not hasattr(la.SparseBatchLCQP, "update_matrices")      # the sparse twin is not built


def test_no_matrix_and_null_handle_are_answered_without_a_device():
    import lcqpow_amd as la
    L = la.lib()
    Q = np.eye(4); qp = Q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    addr = ctypes.c_void_p(Q.ctypes.data)      # (never dereferenced: the handle is checked first)
    # every matrix NULL: LCQP_INVALID_ARGUMENT, the first check of both calls
    assert L.lcqp_hip_batch_update_matrices(None, 0, 1, None, None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_update_matrices_device(None, 0, 1, 0, None, None, None, None, None) == INVALID_ARGUMENT
    # a NULL handle: LCQP_LCQPOBJECT_NOT_SETUP, as lcqp_hip_batch_update / _update_device
    for k in range(4):
        mats = [None] * 4
        mats[k] = qp
        assert L.lcqp_hip_batch_update_matrices(None, 0, 1, *mats) == NOT_SETUP
        mats[k] = addr
        assert L.lcqp_hip_batch_update_matrices_device(None, 0, 1, 0, *mats, None) == NOT_SETUP
