"""The read-back of the ADMM fallback at the C ABI, without a device: lcqp_hip_batch_read_admm and lcqp_hip_qp_read_admm are exported with
the signatures include/lcqp_hip.h documents, and their argument errors are decided before any device call and before the handle's device
state is touched (the batch handle of the checks below is a block of zero bytes: a batch of zero instances)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NOT_SETUP = 100, 300
dp = ctypes.POINTER(ctypes.c_double)

TAIL = "int dims[6], double scal[3], double* FK, double* rhov, double* l, double* u, double* xa, double* ya, double* za, double* dy, double* dx"
SIGNATURES = {"lcqp_hip_batch_read_admm": "lcqp_hip_batch_t* b, int instance, " + TAIL, "lcqp_hip_qp_read_admm": "lcqp_hip_qp_t* qp, " + TAIL}


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
    from lcqpow_amd import capi
    assert len(capi.lib().lcqp_hip_batch_read_admm.argtypes) == 13 and len(capi.lib().lcqp_hip_qp_read_admm.argtypes) == 12
    assert callable(capi.BatchLCQP.read_admm) and callable(capi.SubsolverHIP.read_admm)


def test_argument_errors_need_no_device():
    import lcqpow_amd as la
    L = la.lib()
    dims = (ctypes.c_int * 6)(*[-7] * 6); scal = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    buf = np.full(4, 7.0); P = lambda a: a.ctypes.data_as(dp)
    fake = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)      # B = 0: every instance is out of range
    none = [None] * 9
    assert L.lcqp_hip_batch_read_admm(None, 0, dims, scal, *none) == INVALID_ARGUMENT
    assert L.lcqp_hip_batch_read_admm(None, 0, None, None, *none) == INVALID_ARGUMENT
    for inst in (0, -1, 5):
        assert L.lcqp_hip_batch_read_admm(fake, inst, dims, scal, P(buf), *[P(buf)] * 8) == INVALID_ARGUMENT
    assert L.lcqp_hip_qp_read_admm(None, dims, scal, *none) == INVALID_ARGUMENT
    # a QP object exists on the host before its first solve builds its batch: nothing to read yet
    Q = np.eye(2)
    q = L.lcqp_hip_qp_create(2, 0, P(Q), None, None, 0)
    assert q is not None
    assert L.lcqp_hip_qp_read_admm(ctypes.c_void_p(q), dims, scal, *none) == NOT_SETUP
    assert L.lcqp_hip_qp_read_admm(ctypes.c_void_p(q), dims, scal, P(buf), *[P(buf)] * 8) == NOT_SETUP
    L.lcqp_hip_qp_destroy(ctypes.c_void_p(q))
    assert list(dims) == [-7] * 6 and list(scal) == [7.0] * 3 and np.all(buf == 7.0)      # refused calls write nothing
    if la.device_count() > 0:      # a batch that holds no setup yet
        bt = la.BatchLCQP(1, 2, 0, 1)
        assert L.lcqp_hip_batch_read_admm(bt.h, 0, dims, scal, *none) == NOT_SETUP
        assert L.lcqp_hip_batch_read_admm(bt.h, 1, dims, scal, *none) == INVALID_ARGUMENT
        bt.close()
        assert list(dims) == [-7] * 6
