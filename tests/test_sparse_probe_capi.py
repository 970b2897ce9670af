"""The read-backs of the ADMM state and of the polish state and the product probe of the sparse arm at the C ABI, without a device
(lcqp_hip_sparse_read_admm, lcqp_hip_sparse_read_polish, lcqp_hip_sparse_product_probe): declared in include/lcqp_hip.h, exported by the built library, bound in Python, and the answers to a NULL
handle -- the only handle there is without a device."""
import ctypes

import numpy as np

from test_capi_symbols import declared_functions

NEW = ("lcqp_hip_sparse_read_admm", "lcqp_hip_sparse_read_polish", "lcqp_hip_sparse_product_probe")


def test_the_new_calls_are_declared_and_exported():
    import lcqpow_amd
    L = ctypes.CDLL(lcqpow_amd.library_path())
    names = declared_functions()
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n


def test_the_binding_has_them():
    import lcqpow_amd as la
    from lcqpow_amd import capi
    assert callable(la.SparseBatchLCQP.read_admm) and callable(la.SparseBatchLCQP.product_probe) and callable(la.SparseBatchLCQP.read_polish)
    assert len(capi.lib().lcqp_hip_sparse_read_polish.argtypes) == 7
    assert (len(la.SparseBatchLCQP.POLISH_DIMS), len(la.SparseBatchLCQP.POLISH_SCALARS)) == (15, 11)
    assert len(capi.lib().lcqp_hip_sparse_read_admm.argtypes) == 10 and len(capi.lib().lcqp_hip_sparse_product_probe.argtypes) == 8


def test_null_handle_answers_without_a_gpu():
    import lcqpow_amd as la
    L = la.lib()
    dp = ctypes.POINTER(ctypes.c_double); ip = ctypes.POINTER(ctypes.c_int)
    dims = np.full(2, -7, dtype=np.int32); scal = np.full(3, -7.0); buf = np.full(8, -7.0); ell = np.full(6, -7, dtype=np.int32)
    P = lambda a: a.ctypes.data_as(dp)
    for inst in (0, -1, 5):
        assert L.lcqp_hip_sparse_read_admm(None, inst, dims.ctypes.data_as(ip), P(scal), *[P(buf)] * 6) == 100
        assert L.lcqp_hip_sparse_read_admm(None, inst, None, None, *[None] * 6) == 100
    for wide in (0, 1, 2):
        assert L.lcqp_hip_sparse_product_probe(None, wide, *[P(buf)] * 5, ell.ctypes.data_as(ip)) == 100
    assert L.lcqp_hip_sparse_product_probe(None, 0, *[None] * 6) == 100
    assert (dims == -7).all() and (scal == -7).all() and (buf == -7).all() and (ell == -7).all()


def test_read_polish_null_handle_answers_without_a_gpu():
    """LCQP_INVALID_ARGUMENT for a NULL handle with every combination of NULL buffers; nothing is written"""
    import itertools
    import lcqpow_amd as la
    L = la.lib()
    dp = ctypes.POINTER(ctypes.c_double); ip = ctypes.POINTER(ctypes.c_int)
    dims = np.full(15, -7, dtype=np.int32); scal = np.full(11, -7.0); V = np.full(40, -7.0); Mv = np.full(40, -7.0); I = np.full(32, -7, dtype=np.int32)
    full = (dims.ctypes.data_as(ip), scal.ctypes.data_as(dp), V.ctypes.data_as(dp), Mv.ctypes.data_as(dp), I.ctypes.data_as(ip))
    for mask in itertools.product((False, True), repeat=5):
        for inst in (0, -1, 5):
            assert L.lcqp_hip_sparse_read_polish(None, inst, *[a if keep else None for a, keep in zip(full, mask)]) == 100, (mask, inst)
    assert (dims == -7).all() and (scal == -7).all() and (V == -7).all() and (Mv == -7).all() and (I == -7).all()
