"""The C-ABI library loads on a CPU-only box and exports every symbol include/lcqp_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "lcqp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lcqp_hip_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_declared_symbols():
    import lcqpow_amd
    L = ctypes.CDLL(lcqpow_amd.library_path())
    names = declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), n


def test_options_default_matches_reference_defaults():
    import lcqpow_amd as la
    o = la.default_options()
    assert o.complementarityTolerance == 1e3 * 2.221e-16 and o.stationarityTolerance == 1e6 * 2.221e-16
    assert (o.initialPenaltyParameter, o.penaltyUpdateFactor, o.maxPenaltyParameter) == (0.01, 2.0, 1e8)
    assert (o.solveZeroPenaltyFirst, o.perturbStep, o.maxIterations, o.nDynamicPenalty) == (1, 1, 1000, 3)


def test_option_structs_have_identical_layout():
    import lcqpow_amd as la
    import oracle_py
    assert [f[0] for f in la.Options._fields_] == [f[0] for f in oracle_py.Options._fields_]
    assert ctypes.sizeof(la.Options) == ctypes.sizeof(oracle_py.Options)
    assert ctypes.sizeof(la.Stats) == ctypes.sizeof(oracle_py.Stats)


def test_no_product_import_of_oracle():
    """the shipped path must never route through the oracle"""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "lcqpow_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not re.search(r"#\s*include[^\n]*oracle", txt), f
                assert not re.search(r"\bimport\s+oracle_py|from\s+oracle_py", txt), f
                assert "liblcqp_oracle" not in txt and not re.search(r"\borc_[a-z_]+\s*\(", txt), f


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """argument checks of the C ABI that need no device, and the loud failure of every compute entry when none is visible"""
    import numpy as np
    import lcqpow_amd as la
    from lcqpow_amd import capi
    L = la.lib()
    assert L.lcqp_hip_batch_create(0, 4, 1, 1, 0, 0) is None and "invalid" in capi.last_error()
    assert L.lcqp_hip_batch_create(4, 4, -1, 1, 0, 0) is None
    assert L.lcqp_hip_batch_create(1, 4097, 0, 1, 0, 0) is None and "4096" in capi.last_error()
    Q = np.eye(2); dp = ctypes.POINTER(ctypes.c_double)
    assert L.lcqp_hip_qp_create(0, 0, Q.ctypes.data_as(dp), None, None, 0) is None
    assert L.lcqp_hip_qp_create(2, 1, Q.ctypes.data_as(dp), None, None, 0) is None          # nC > 0 without A
    assert L.lcqp_hip_batch_run(None) != 0 and L.lcqp_hip_batch_setup(None) != 0
    dims = (ctypes.c_int * 9)()
    assert L.lcqp_hip_batch_read_setup(None, 0, dims, *[None] * 9) != 0 and L.lcqp_hip_batch_read_working_set(None, 0, dims, *[None] * 4) != 0
    assert L.lcqp_hip_qp_read_setup(None, dims, *[None] * 9) != 0 and L.lcqp_hip_qp_read_working_set(None, dims, *[None] * 4) != 0
    assert L.lcqp_hip_batch_read_admm(None, 0, dims, *[None] * 10) != 0 and L.lcqp_hip_qp_read_admm(None, dims, *[None] * 10) != 0
    assert L.lcqp_hip_batch_read_polish(None, 0, None, *[None] * 4) == 100 and L.lcqp_hip_qp_read_polish(None, None, *[None] * 4) == 100
    assert callable(capi.BatchLCQP.read_polish) and callable(capi.SubsolverHIP.read_polish)
    assert "lcqp_hip_sparse_read_polish" in declared_functions() and L.lcqp_hip_sparse_read_polish(None, 0, None, *[None] * 4) == 100
    assert callable(capi.SparseBatchLCQP.read_polish)
    n = ctypes.c_int(0)
    if la.device_count() == 0:
        # no GPU here: creating a batch must fail with the HIP error, never fall back to anything
        assert L.lcqp_hip_batch_create(2, 4, 1, 1, 0, 0) is None and capi.last_error() != ""
        q = L.lcqp_hip_qp_create(2, 0, Q.ctypes.data_as(dp), None, None, 0)           # host-side object only
        assert q is not None
        it, ef = ctypes.c_int(0), ctypes.c_int(0)
        g = np.zeros(2)
        rc = L.lcqp_hip_qp_solve(ctypes.c_void_p(q), 1, ctypes.byref(it), ctypes.byref(ef), g.ctypes.data_as(dp), None, None, None, None, None, None)
        assert rc == capi.SUBPROBLEM_SOLVER_ERROR and ef.value != 0
        # the readers of the setup matrices and of the working set have nothing to read: an error code, no crash, the buffers untouched
        dims[0] = -7
        assert L.lcqp_hip_qp_read_setup(ctypes.c_void_p(q), dims, *[None] * 9) != 0
        assert L.lcqp_hip_qp_read_working_set(ctypes.c_void_p(q), dims, *[None] * 4) != 0
        assert L.lcqp_hip_qp_read_admm(ctypes.c_void_p(q), dims, *[None] * 10) != 0
        assert L.lcqp_hip_qp_read_polish(ctypes.c_void_p(q), ctypes.cast(dims, ctypes.POINTER(ctypes.c_int)), *[None] * 4) == 300
        assert dims[0] == -7
        L.lcqp_hip_qp_destroy(ctypes.c_void_p(q))


def test_qp_solve_failure_leaves_a_message():
    """A failing lcqp_hip_qp_solve sets exit_flag = -1, returns SUBPROBLEM_SOLVER_ERROR and leaves the failing HIP call in
    lcqp_hip_last_error().  A device index far out of range is a runtime argument error with or without a GPU: lcqp_hip_qp_create touches
    no device and succeeds, the first solve cannot build its batch.  This is the one failure a valid device-free call reaches (the message
    is lcqp_hip_batch_create's); the HIP calls of the solve behind it fail only where a device fails.
    The error is reported once: hip_fail takes it from the runtime, whose hipGetLastError() -- the check behind every launch of the
    thread, of any handle -- would otherwise hand it to the next launch."""
    import numpy as np
    import lcqpow_amd as la
    from lcqpow_amd import capi
    L = la.lib()
    Q = np.eye(2); g = np.zeros(2); dp = ctypes.POINTER(ctypes.c_double)
    assert L.lcqp_hip_qp_create(0, 0, Q.ctypes.data_as(dp), None, None, 0) is None and capi.last_error() == "invalid arguments"
    q = L.lcqp_hip_qp_create(2, 0, Q.ctypes.data_as(dp), None, None, 1 << 20)
    assert q is not None
    it, ef = ctypes.c_int(7), ctypes.c_int(7)
    rc = L.lcqp_hip_qp_solve(ctypes.c_void_p(q), 1, ctypes.byref(it), ctypes.byref(ef), g.ctypes.data_as(dp), None, None, None, None, None, None)
    assert rc == capi.SUBPROBLEM_SOLVER_ERROR and ef.value == -1 and it.value == 0
    assert capi.last_error().startswith("hipSetDevice(device): "), capi.last_error()      # not the stale message of the call before
    if la.device_count() > 0:      # (without a device every call of the runtime, hipGetLastError() included, returns hipErrorNoDevice)
        runtime = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]       # the HIP runtime the library is linked to
        assert runtime and ctypes.CDLL(runtime[0]).hipGetLastError() == 0                         # hipSuccess: nothing left for a later launch check
    L.lcqp_hip_qp_destroy(ctypes.c_void_p(q))


def test_sparse_kkt_probe_checks_its_arguments_without_a_gpu():
    """lcqp_hip_sparse_kkt_probe (test and diagnostic entry point of the sparse arm): nrhs < 1, NULL vectors, a mode other than FACTOR / STORED, a
    FACTOR call without its inputs, a STORED call with a bad slot or without its record buffers are LCQP_INVALID_ARGUMENT; with good arguments a
    NULL handle -- the only handle there is without a device -- is LCQP_LCQPOBJECT_NOT_SETUP, as a call before the first run is on a GPU
    (tests/test_gpu_sparse_factor.py).  All of it is decided before any device call."""
    import numpy as np
    import lcqpow_amd as la
    L = la.lib()
    assert "lcqp_hip_sparse_kkt_probe" in declared_functions()
    dp = ctypes.POINTER(ctypes.c_double); ip = ctypes.POINTER(ctypes.c_int)
    v = np.zeros(4); w = np.zeros(4); u = np.zeros(4, dtype=np.int32)
    d = lambda a: a.ctypes.data_as(dp)
    i = lambda a: a.ctypes.data_as(ip)
    probe = L.lcqp_hip_sparse_kkt_probe
    FACTOR, STORED = 0, 1
    good_f = (d(v), d(v), i(u), d(v), d(w), None, None, None)
    good_s = (None, None, None, d(v), d(w), d(v), d(v), i(u))
    assert probe(None, FACTOR, 0, 0, *good_f) == 100 and probe(None, STORED, 0, -1, *good_s) == 100              # nrhs < 1
    assert probe(None, FACTOR, 0, 1, d(v), d(v), i(u), None, d(w), None, None, None) == 100                        # rhs
    assert probe(None, FACTOR, 0, 1, d(v), d(v), i(u), d(v), None, None, None, None) == 100                        # sol
    assert probe(None, 2, 0, 1, *good_f) == 100 and probe(None, -1, 0, 1, *good_s) == 100                          # mode
    for k in range(3):                                                                                             # FACTOR without dprim / ddual / use
        a = list(good_f); a[k] = None
        assert probe(None, FACTOR, 0, 1, *a) == 100
    assert probe(None, STORED, 2, 1, *good_s) == 100 and probe(None, STORED, -1, 1, *good_s) == 100                # which
    for k in (5, 6, 7):                                                                                            # STORED without a record buffer
        a = list(good_s); a[k] = None
        assert probe(None, STORED, 0, 1, *a) == 100
    assert probe(None, FACTOR, 0, 1, *good_f) == 300 and probe(None, STORED, 0, 1, *good_s) == 300 and probe(None, STORED, 1, 1, *good_s) == 300
    assert w.sum() == 0.0


def test_missing_extension_fails_loudly(monkeypatch):
    """no CPU fallback: without the built HIP library the binding raises instead of computing anything"""
    import pytest
    from lcqpow_amd import capi
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "_SO", "/nonexistent/liblcqpow_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        capi.lib()
    with pytest.raises(RuntimeError):
        capi.BatchLCQP(1, 2, 0, 1)


def test_sparse_pattern_validation_needs_no_gpu():
    """lcqp_hip_sparse_create checks the CSC pattern before it touches a device: decreasing column pointers, unsorted or duplicated row
    indices, an upper-triangular Q (OSQP's own convention for P -- this surface, like the reference's, takes the full matrix) and a short
    index array are refused with a message (src/SubsolverOSQP.cpp:136-152 hands such arrays to OSQP unchecked)"""
    import numpy as np
    import lcqpow_amd as la

    class Pat:
        def __init__(self, indptr, indices):
            self.indptr, self.indices = np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32)
    n, nC, nK = 4, 0, 1
    Aok = Pat([0, 1, 2, 2, 2], [0, 1])                                  # L = e_0', R = e_1'
    Qok = Pat([0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3])
    cases = [(Pat([0, 2, 1, 5, 6], [0, 1, 0, 1, 2, 3]), Aok, "decrease"),
             (Pat([0, 2, 4, 5, 6], [1, 0, 0, 1, 2, 3]), Aok, "sorted"),
             (Pat([0, 2, 4, 5, 6], [0, 0, 0, 1, 2, 3]), Aok, "duplicates"),
             (Pat([0, 1, 3, 4, 5], [0, 0, 1, 2, 3]), Aok, "symmetric"),          # upper triangle only
             (Qok, Pat([0, 1, 2, 2, 2], [0, 7]), "out of bounds")]
    for Qp, Ap, word in cases:
        with pytest.raises(RuntimeError, match=word):
            la.SparseBatchLCQP(1, n, nC, nK, Qp, Ap)
    with pytest.raises(ValueError, match="indptr"):
        la.SparseBatchLCQP(1, n, nC, nK, Pat([0, 2, 4, 5, 6], [0, 1, 0, 1, 2]), Aok)


def test_dense_size_limit_is_reported_not_hidden():
    """Limits the reference does not have: the dense kernels take nV <= 4096 (padded sizes 128 ... 4096; round 3: 1024) and at most
    min(max(2 nV, 64), rows, 896 / 1216 / 2432 / 3264) simultaneously active rows (tests/test_gpu_parity.py::test_subsolver_active_row_capacity).  A larger
    problem is refused at creation with a message -- through the C ABI (NULL handle) and through LCQProblem (SUBPROBLEM_SOLVER_ERROR from
    runSolver, the reference's return code for a subsolver that cannot take the problem, src/SubsolverQPOASES.cpp:165-168) -- never run wrongly.
    The size check precedes any device call, so this holds on a CPU-only box too."""
    import numpy as np
    import lcqpow_amd as la
    from lcqpow_amd import capi
    L = la.lib()
    assert L.lcqp_hip_batch_create(1, 4097, 0, 1, 0, 0) is None
    assert "nV > 4096" in capi.last_error()
    h = L.lcqp_hip_batch_create(1, 4096, 0, 1, 0, 0)          # the largest size: accepted as far as the size goes (no device here: NULL for another reason)
    if h is None:
        assert "nV > 4096" not in capi.last_error()
    else:
        L.lcqp_hip_batch_destroy.argtypes = [ctypes.c_void_p]; L.lcqp_hip_batch_destroy(ctypes.c_void_p(h))
    import lcqpow_amd.lcqpow as lcqpow
    n = 4097
    p = lcqpow.LCQProblem(nV=n, nC=0, nComp=1)
    o = lcqpow.Options(); o.setPrintLevel(lcqpow.PrintLevel.NONE); p.setOptions(o)
    Lm = np.zeros((1, n)); Lm[0, 0] = 1.0; Rm = np.zeros((1, n)); Rm[0, 1] = 1.0
    assert p.loadLCQP(Q=np.eye(n), g=-np.ones(n), L=Lm, R=Rm, order="C") == 0
    assert int(p.runSolver()) == capi.SUBPROBLEM_SOLVER_ERROR
    assert "nV > 4096" in capi.last_error()
