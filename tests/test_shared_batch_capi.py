"""The shared-matrix dense batch (lcqp_hip_batch_create_shared, lcqp_hip_batch_device_bytes, BatchLCQP(shared_matrices=True)) as far as it
can be checked without a GPU: the exported symbols, the argument checks of the C ABI that need no device, and the refusals the Python
binding makes before the C call."""
import ctypes

import numpy as np
import pytest

from test_capi_symbols import declared_functions


def test_new_symbols_are_declared_and_exported():
    import lcqpow_amd
    L = ctypes.CDLL(lcqpow_amd.library_path())
    for name in ("lcqp_hip_batch_create_shared", "lcqp_hip_batch_device_bytes"):
        assert name in declared_functions() and hasattr(L, name), name


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    import lcqpow_amd as la
    from lcqpow_amd import capi
    L = la.lib()
    assert L.lcqp_hip_batch_create_shared(0, 4, 1, 1, 0, 0) is None and "invalid" in capi.last_error()
    assert L.lcqp_hip_batch_create_shared(4, 4, -1, 1, 0, 0) is None and L.lcqp_hip_batch_create_shared(4, 0, 1, 1, 0, 0) is None
    assert L.lcqp_hip_batch_create_shared(1, 4097, 0, 1, 0, 0) is None and "4096" in capi.last_error()
    out = (ctypes.c_size_t * 2)()
    assert L.lcqp_hip_batch_device_bytes(None, out) == 300      # LCQP_LCQPOBJECT_NOT_SETUP, as the neighbouring calls answer a NULL handle
    assert L.lcqp_hip_batch_device_bytes(None, None) != 0
    if la.device_count() == 0:      # no GPU here: creating the batch must fail with the HIP error, never fall back to anything
        assert L.lcqp_hip_batch_create_shared(2, 4, 1, 1, 0, 0) is None and capi.last_error() != ""


class _Handle:
    """a BatchLCQP over no C handle: the checks under test are made before the C call, which would get a NULL handle"""
    def __new__(cls, B, n, nC, nComp, shared=True):
        from lcqpow_amd import capi
        b = object.__new__(capi.BatchLCQP)
        b.B, b.nV, b.nC, b.nComp, b.device, b.h, b.shared_matrices = B, n, nC, nComp, 0, None, shared
        b.nd = b._ndual = n + nC + 2 * nComp
        return b


def test_python_refuses_matrices_per_instance_before_the_c_call():
    B, n, nC, nK = 3, 4, 2, 1
    b = _Handle(B, n, nC, nK)
    Q3, g = np.zeros((B, n, n)), np.zeros((B, n))
    L2 = np.zeros((nK, n))
    with pytest.raises(ValueError, match="ONE matrix"):
        b.load(0, B, Q3, g, L2, L2)
    with pytest.raises(ValueError, match="ONE matrix"):
        b.load(0, B, np.eye(n), g, np.zeros((B, nK, n)), L2)
    with pytest.raises(ValueError, match="ONE matrix"):
        b.update_matrices(0, B, Q=Q3)
    with pytest.raises(ValueError, match="whole batch"):
        b.update_matrices(0, B - 1, Q=np.eye(n))
    with pytest.raises(ValueError, match="whole batch"):
        b.update_matrices(1, B - 1, Q=np.eye(n))
    # a 2-D matrix passes these checks and reaches the C call, which answers for the NULL handle
    assert b.update_matrices(0, B, Q=np.eye(n)) == 300
    assert b.load(0, B, np.eye(n), g, L2, L2) == 300
    b.h = None      # (nothing to destroy)
    # an ordinary batch still takes one matrix per instance, and sizes them so
    o = _Handle(B, n, nC, nK, shared=False)
    assert o.update_matrices(0, B - 1, Q=np.zeros((B - 1, n, n))) == 300
    with pytest.raises(ValueError, match="expected"):
        o.update_matrices(0, B, Q=np.eye(n))
