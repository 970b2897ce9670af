"""The full adjoint of the dense arm at the C ABI, without a device: lcqp_hip_batch_adjoint and lcqp_hip_qp_adjoint are exported with the
signatures include/lcqp_hip.h documents, and their argument checks come before any device call (they answer on a box without a GPU, and
before the handle is dereferenced: the handle of the checks below is a block of zero bytes)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NOT_SETUP = 100, 300
dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

SIGNATURES = {
    "lcqp_hip_batch_adjoint": "lcqp_hip_batch_t* b, const double* vx, const double* vy, double* dg, double* db, int* side, int* info, "
                              "int reduce, double* dQ, double* dA, double* dL, double* dR",
    "lcqp_hip_qp_adjoint": "lcqp_hip_qp_t* qp, const double* vx, const double* vy, double* dg, double* db, int* side, int* info, "
                           "double* dQ, double* dA",
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
    # the binding declares the same number of arguments
    from lcqpow_amd import capi
    assert len(capi.lib().lcqp_hip_batch_adjoint.argtypes) == 12 and len(capi.lib().lcqp_hip_qp_adjoint.argtypes) == 9


def test_argument_checks_need_no_device():
    import lcqpow_amd as la
    L = la.lib()
    n = 4
    vx = np.ones(n); dg = np.full(n, 7.0)
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)      # never read: every call below is refused on its arguments
    P = lambda a: a.ctypes.data_as(dp)
    tail = [None] * 4
    assert L.lcqp_hip_batch_adjoint(None, P(vx), None, P(dg), None, None, None, 0, *tail) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_adjoint(fake, None, None, P(dg), None, None, None, 0, *tail) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_adjoint(fake, P(vx), None, None, None, None, None, 0, *tail) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_adjoint(fake, P(vx), None, P(dg), None, None, None, 2, *tail) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_adjoint(fake, P(vx), None, P(dg), None, None, None, -1, *tail) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_adjoint(None, P(vx), None, P(dg), None, None, None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_adjoint(fake, None, None, P(dg), None, None, None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_adjoint(fake, P(vx), None, None, None, None, None, None, None) == INVALID_ARGUMENT
    assert np.all(dg == 7.0)


def test_an_object_that_never_solved_is_refused():
    """LCQP_LCQPOBJECT_NOT_SETUP under the mark of the sensitivity calls: the QP object exists on the host before its first solve, so this
    needs no device; a batch object does (tests/test_gpu_adjoint.py has the batch that never ran, here it runs where a device is visible)"""
    import lcqpow_amd as la
    L = la.lib()
    n = 2
    Q = np.eye(n); vx = np.ones(n); dg = np.full(n, 7.0); dQ = np.full((n, n), 7.0)
    P = lambda a: a.ctypes.data_as(dp)
    q = L.lcqp_hip_qp_create(n, 0, P(Q), None, None, 0)
    assert q is not None
    assert L.lcqp_hip_qp_adjoint(ctypes.c_void_p(q), P(vx), None, P(dg), None, None, None, P(dQ), None) == NOT_SETUP
    assert L.lcqp_hip_qp_adjoint(ctypes.c_void_p(q), None, None, P(dg), None, None, None, None, None) == INVALID_ARGUMENT      # the order of the checks
    L.lcqp_hip_qp_destroy(ctypes.c_void_p(q))
    assert np.all(dg == 7.0) and np.all(dQ == 7.0)
    if la.device_count() > 0:
        bt = la.BatchLCQP(1, n, 0, 1)
        assert L.lcqp_hip_batch_adjoint(bt.h, P(vx), None, P(dg), None, None, None, 0, P(dQ), None, None, None) == NOT_SETUP
        assert L.lcqp_hip_batch_adjoint(bt.h, P(vx), None, P(dg), None, None, None, 2, P(dQ), None, None, None) == INVALID_ARGUMENT
        bt.close()
        assert np.all(dg == 7.0) and np.all(dQ == 7.0)
