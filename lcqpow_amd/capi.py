"""ctypes binding of the C ABI in include/lcqp_hip.h (liblcqpow_hip.so).  No CPU fallback."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LCQPOW_HIP_LIBRARY: another build of the same HIP library (experiment variants under build/ab/); there is no CPU fallback either way
_SO = os.environ.get("LCQPOW_HIP_LIBRARY") or os.path.join(_HERE, "liblcqpow_hip.so")
c_double_p = C.POINTER(C.c_double)

SEED0 = 0x4C43515000000001
SUCCESSFUL_RETURN = 0
SUBPROBLEM_SOLVER_ERROR = 203
MAX_ITERATIONS_REACHED = 200
MAX_PENALTY_REACHED = 201


class Options(C.Structure):
    """lcqp_options_t (include/lcqp_hip.h); same field order as the oracle's orc_options_t."""
    _fields_ = [
        ("complementarityTolerance", C.c_double), ("stationarityTolerance", C.c_double),
        ("initialPenaltyParameter", C.c_double), ("penaltyUpdateFactor", C.c_double),
        ("maxPenaltyParameter", C.c_double), ("etaDynamicPenalty", C.c_double),
        ("solveZeroPenaltyFirst", C.c_int), ("perturbStep", C.c_int), ("maxIterations", C.c_int),
        ("nDynamicPenalty", C.c_int), ("printLevel", C.c_int), ("storeSteps", C.c_int),
        ("perturbSeed", C.c_uint64),
        ("admmRho", C.c_double), ("admmSigma", C.c_double), ("admmAlpha", C.c_double), ("rhoEqMult", C.c_double),
        ("proxSmall", C.c_double), ("proxBig", C.c_double), ("pivotThreshold", C.c_double), ("depTau", C.c_double),
        ("feasTol", C.c_double), ("resTol", C.c_double),
        ("admmFirst", C.c_int), ("admmHot", C.c_int), ("maxTrials", C.c_int), ("maxRounds", C.c_int),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("iterTotal", C.c_int), ("iterOuter", C.c_int), ("subproblemIter", C.c_int), ("status", C.c_int),
        ("qpSolverExitFlag", C.c_int), ("returnValue", C.c_int), ("rhoOpt", C.c_double),
        ("admmIter", C.c_int), ("trials", C.c_int), ("factorizations", C.c_int), ("corrections", C.c_int),
        ("qpSolves", C.c_int), ("reserved", C.c_int),
    ]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None
_runtime = None      # "torch": the library was bound to the HIP runtime a torch of this process bundles; "system": to the one it was linked against


def _torch_hip_runtime():
    """the libamdhip64.so a torch that this process has IMPORTED ships in its own lib directory, or None (no torch imported, a torch
    without ROCm, or one that uses the system's runtime)"""
    t = sys.modules.get("torch")
    if t is None or not getattr(getattr(t, "version", None), "hip", None):
        return None
    p = os.path.join(os.path.dirname(t.__file__), "lib", "libamdhip64.so")
    return p if os.path.exists(p) else None


def library_path():
    return _SO


def request_hw_queues(n=8):
    """Ask the HIP runtime for n hardware queues (GPU_MAX_HW_QUEUES) -- an explicit call of the PROGRAM (bench.py, the examples), before
    the first HIP call of the process; the library never changes the environment by itself.  Every batch object has two HIP streams and
    the runtime maps the streams of a process onto 4 queues by default: the two slots of a BatchPipeline can land on one queue and run one
    after the other.  Returns True when the variable was set, False when the environment already holds a value (left alone)."""
    if "GPU_MAX_HW_QUEUES" in os.environ:
        return False
    os.environ["GPU_MAX_HW_QUEUES"] = str(int(n))
    return True


def lib():
    """Load liblcqpow_hip.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(f"{_SO} is missing: the HIP extension must be built (see __graft_entry__.build); "
                               "there is no CPU fallback for the product path")
        # Two HIP runtimes cannot drive one GPU from one process (the second one finds the device's address space taken and reports no
        # GPU), and a pointer is a device pointer only to the runtime that allocated it.  In a process that has imported a torch with a
        # runtime of its own, the library is therefore bound to THAT runtime: it goes into the global symbol scope first, where the
        # library's HIP calls are then resolved.  A process without torch binds to the runtime the library was linked against, as ever.
        global _runtime
        rt = _torch_hip_runtime()
        if rt:
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
        _runtime = "torch" if rt else "system"
        L = C.CDLL(_SO)
        L.lcqp_hip_last_error.restype = C.c_char_p
        L.lcqp_hip_options_default.argtypes = [C.POINTER(Options)]
        L.lcqp_hip_qp_create.restype = C.c_void_p
        L.lcqp_hip_qp_create.argtypes = [C.c_int, C.c_int, c_double_p, c_double_p, C.POINTER(Options), C.c_int]
        L.lcqp_hip_qp_clone.restype = C.c_void_p
        L.lcqp_hip_qp_clone.argtypes = [C.c_void_p]
        L.lcqp_hip_qp_destroy.argtypes = [C.c_void_p]
        L.lcqp_hip_qp_solve.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [c_double_p] * 7
        L.lcqp_hip_qp_get_solution.argtypes = [C.c_void_p, c_double_p, c_double_p]
        L.lcqp_hip_qp_get_counters.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        L.lcqp_hip_batch_create.restype = C.c_void_p
        L.lcqp_hip_batch_create.argtypes = [C.c_int] * 6
        L.lcqp_hip_batch_create_shared.restype = C.c_void_p
        L.lcqp_hip_batch_create_shared.argtypes = [C.c_int] * 6
        L.lcqp_hip_batch_device_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        L.lcqp_hip_batch_destroy.argtypes = [C.c_void_p]
        L.lcqp_hip_batch_set_options.argtypes = [C.c_void_p, C.POINTER(Options)]
        L.lcqp_hip_batch_set_overlapped.argtypes = [C.c_void_p, C.c_int]
        L.lcqp_hip_batch_load.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_double_p] * 15
        L.lcqp_hip_batch_generate_synthetic.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.lcqp_hip_batch_update.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_double_p] * 11
        L.lcqp_hip_batch_resolve.argtypes = [C.c_void_p, C.c_int, c_double_p]
        L.lcqp_hip_batch_update_matrices.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_double_p] * 4
        L.lcqp_hip_batch_update_matrices_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_void_p]
        L.lcqp_hip_batch_launch_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.lcqp_hip_batch_read_problem.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 7
        L.lcqp_hip_batch_setup.argtypes = [C.c_void_p]
        L.lcqp_hip_batch_run.argtypes = [C.c_void_p]
        L.lcqp_hip_batch_synchronize.argtypes = [C.c_void_p]
        L.lcqp_hip_batch_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.lcqp_hip_batch_get_solution.argtypes = [C.c_void_p, c_double_p, c_double_p, C.POINTER(Stats)]
        L.lcqp_hip_batch_get_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, C.POINTER(C.c_int)]
        L.lcqp_hip_batch_stream.restype = C.c_void_p
        L.lcqp_hip_batch_stream.argtypes = [C.c_void_p]
        L.lcqp_hip_batch_algorithmic_bytes.restype = C.c_double
        L.lcqp_hip_batch_algorithmic_bytes.argtypes = [C.c_void_p]
        L.lcqp_hip_batch_work_sums.argtypes = [C.c_void_p, c_double_p]
        c_int_p = C.POINTER(C.c_int)
        L.lcqp_hip_batch_read_setup.argtypes = [C.c_void_p, C.c_int, c_int_p, c_double_p] + [c_double_p] * 5 + [c_int_p, c_int_p, c_double_p]
        L.lcqp_hip_batch_read_working_set.argtypes = [C.c_void_p, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p]
        L.lcqp_hip_qp_read_setup.argtypes = [C.c_void_p, c_int_p, c_double_p] + [c_double_p] * 5 + [c_int_p, c_int_p, c_double_p]
        L.lcqp_hip_qp_read_working_set.argtypes = [C.c_void_p, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p]
        L.lcqp_hip_batch_read_admm.argtypes = [C.c_void_p, C.c_int, c_int_p, c_double_p] + [c_double_p] * 9
        L.lcqp_hip_qp_read_admm.argtypes = [C.c_void_p, c_int_p, c_double_p] + [c_double_p] * 9
        L.lcqp_hip_batch_read_polish.argtypes = [C.c_void_p, C.c_int, c_int_p, c_double_p, c_double_p, c_double_p, c_int_p]
        L.lcqp_hip_qp_read_polish.argtypes = [C.c_void_p, c_int_p, c_double_p, c_double_p, c_double_p, c_int_p]
        L.lcqp_hip_batch_sensitivity.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_batch_sensitivity_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.lcqp_hip_qp_sensitivity.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_batch_sensitivity_blocked.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_qp_sensitivity_blocked.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_batch_jacobian.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_qp_jacobian.argtypes = [C.c_void_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_batch_set_jacobian_staging.argtypes = [C.c_void_p, C.c_size_t]
        L.lcqp_hip_batch_adjoint.argtypes = [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p, C.c_int] + [c_double_p] * 4
        L.lcqp_hip_batch_load_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 15 + [C.c_void_p]
        L.lcqp_hip_batch_update_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_void_p]
        L.lcqp_hip_batch_get_solution_device.argtypes = [C.c_void_p] * 5
        L.lcqp_hip_batch_sensitivity_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.lcqp_hip_batch_adjoint_device.argtypes = [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 5
        L.lcqp_hip_batch_adjoint_blocked.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_batch_jacobian_duals.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_batch_adjoint_blocked_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.lcqp_hip_batch_jacobian_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.lcqp_hip_batch_jacobian_duals_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.lcqp_hip_qp_adjoint.argtypes = [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p] + [c_double_p] * 2
        L.lcqp_hip_util_symv.argtypes = [C.c_int, C.c_int, C.c_double] + [c_double_p] * 4
        L.lcqp_hip_util_gemv.argtypes = [C.c_int, C.c_int, C.c_int] + [c_double_p] * 3
        L.lcqp_hip_util_gemv_t.argtypes = [C.c_int, C.c_int, C.c_int] + [c_double_p] * 3
        L.lcqp_hip_util_symm_product.argtypes = [C.c_int, C.c_int, C.c_int] + [c_double_p] * 3
        L.lcqp_hip_util_rows_list.argtypes = [C.c_int, C.c_int, C.c_int, c_double_p, C.POINTER(C.c_int), C.c_int] + [c_double_p] * 4
        L.lcqp_hip_csc_create.restype = C.c_void_p
        L.lcqp_hip_csc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, C.c_int]
        L.lcqp_hip_csc_destroy.argtypes = [C.c_void_p]
        L.lcqp_hip_csc_apply.argtypes = [C.c_void_p, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, C.c_int, C.POINTER(C.c_float)]
        L.lcqp_hip_chol_solve.argtypes = [C.c_int, C.c_int] + [c_double_p] * 3 + [C.c_int, C.POINTER(C.c_float)]
        L.lcqp_hip_sparse_create.restype = C.c_void_p
        L.lcqp_hip_sparse_create.argtypes = [C.c_int] * 4 + [c_int_p] * 4 + [C.c_int]
        L.lcqp_hip_sparse_last_error.restype = C.c_char_p
        L.lcqp_hip_sparse_destroy.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_bandwidth.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_lanes.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_border.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_fronts.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_general_ordering.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_get_ordering.argtypes = [C.c_void_p, c_int_p]
        L.lcqp_hip_sparse_set_options.argtypes = [C.c_void_p, C.POINTER(Options)]
        L.lcqp_hip_sparse_load.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_double_p] * 11
        L.lcqp_hip_sparse_run.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_synchronize.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.lcqp_hip_sparse_get_solution.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_void_p]
        L.lcqp_hip_sparse_get_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, C.POINTER(C.c_int)]
        L.lcqp_hip_sparse_algorithmic_bytes.restype = C.c_double
        L.lcqp_hip_sparse_algorithmic_bytes.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_update.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_double_p] * 9
        L.lcqp_hip_sparse_update_values.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_double_p] * 2
        L.lcqp_hip_sparse_update_values_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_void_p]
        L.lcqp_hip_sparse_resolve.argtypes = [C.c_void_p, C.c_int, c_double_p]
        L.lcqp_hip_sparse_launch_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.lcqp_hip_sparse_sensitivity.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_sparse_sensitivity_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.lcqp_hip_sparse_sens_panel.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_set_general_panel.argtypes = [C.c_void_p, C.c_int]
        L.lcqp_hip_sparse_max_front.argtypes = [C.c_void_p]
        L.lcqp_hip_sparse_sensitivity_blocked.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_sparse_jacobian.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_sparse_adjoint.argtypes = [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p, C.c_int] + [c_double_p] * 2
        L.lcqp_hip_sparse_adjoint_blocked.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_sparse_jacobian_duals.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p, c_int_p]
        L.lcqp_hip_sparse_set_adjoint_staging.argtypes = [C.c_void_p, C.c_size_t]
        L.lcqp_hip_sparse_load_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_void_p]
        L.lcqp_hip_sparse_update_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_void_p]
        L.lcqp_hip_sparse_get_solution_device.argtypes = [C.c_void_p] * 5
        L.lcqp_hip_sparse_sensitivity_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.lcqp_hip_sparse_adjoint_device.argtypes = [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 3
        L.lcqp_hip_sparse_sensitivity_blocked_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.lcqp_hip_sparse_adjoint_blocked_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.lcqp_hip_sparse_jacobian_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.lcqp_hip_sparse_jacobian_duals_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.lcqp_hip_sparse_read_problem.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 9 + [c_int_p]
        L.lcqp_hip_sparse_read_admm.argtypes = [C.c_void_p, C.c_int, c_int_p, c_double_p] + [c_double_p] * 6
        L.lcqp_hip_sparse_read_polish.argtypes = [C.c_void_p, C.c_int, c_int_p, c_double_p, c_double_p, c_double_p, c_int_p]
        L.lcqp_hip_sparse_product_probe.argtypes = [C.c_void_p, C.c_int] + [c_double_p] * 5 + [c_int_p]
        L.lcqp_hip_sparse_kkt_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p, c_int_p, c_double_p, c_double_p,
                                                c_double_p, c_double_p, c_int_p]
        _lib = L
    return _lib


def last_error():
    return lib().lcqp_hip_last_error().decode()


def device_count():
    return lib().lcqp_hip_device_count()


def default_options(**kw):
    o = Options()
    lib().lcqp_hip_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _arr(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _p(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}: {last_error()}")


def _sized(name, a, size):
    """the C side reads exactly `size` doubles through the raw pointer: refuse anything else here"""
    if a is not None and a.size != size:
        raise ValueError(f"{name}: expected {size} values, got {a.size} (shape {a.shape})")
    return a


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _read_setup(call):
    """call(dims, scal, C, F1, D1, Et, MM, Cp, Ci, Cv) -> rc: the raw padded device blocks of one instance's constant matrices as numpy
    arrays (lcqp_hip_batch_read_setup).  A first call with no buffers asks for the dimensions."""
    dims = np.zeros(9, dtype=np.int32); scal = np.zeros(2)
    _check(call(_ip(dims), _p(scal), None, None, None, None, None, None, None, None), "read_setup")
    np_, nblk, mEcap, mMld, capS, capC = (int(v) for v in dims[:6])
    Cm = np.zeros((np_, np_)); F1 = np.zeros((np_, np_)); D1 = np.zeros((nblk, 64, 64)); Et = np.zeros((mEcap, np_))
    MM = np.zeros((mMld, mMld)); Cp = np.zeros(np_ + 1, dtype=np.int32); Ci = np.zeros(capC, dtype=np.int32); Cv = np.zeros(capC)
    _check(call(_ip(dims), _p(scal), _p(Cm), _p(F1), _p(D1), _p(Et), _p(MM), _ip(Cp), _ip(Ci), _p(Cv)), "read_setup")
    return dict(np=np_, nblk=nblk, mEcap=mEcap, mMld=mMld, capS=capS, capC=capC, mE=int(dims[6]), cNnz=int(dims[7]),
                setupFail=int(dims[8]), spv=float(scal[0]), scale=float(scal[1]), C=Cm, F1=F1, D1=D1, Et=Et, MM=MM, Cp=Cp, Ci=Ci, Cv=Cv)


def _read_working_set(call, capS, mE):
    """call(dims, slot_row, crow, row_slot, Ti) -> rc: the inverse factor of the working-set matrix and its maps (lcqp_hip_batch_read_working_set)"""
    dims = np.zeros(2, dtype=np.int32)
    slot_row = np.zeros(capS, dtype=np.int32); crow = np.zeros(capS, dtype=np.int32); row_slot = np.zeros(max(mE, 1), dtype=np.int32)
    Ti = np.zeros((capS, capS))
    _check(call(_ip(dims), _ip(slot_row), _ip(crow), _ip(row_slot), _p(Ti)), "read_working_set")
    return dict(nT=int(dims[0]), ns=int(dims[1]), slot_row=slot_row, crow=crow, row_slot=row_slot[:mE], Ti=Ti)


def _read_admm(call):
    """call(dims, scal, FK, rhov, l, u, xa, ya, za, dy, dx) -> rc: the state of the ADMM fallback of one instance as it lies on the device
    (lcqp_hip_batch_read_admm).  A first call with no buffers asks for the dimensions."""
    dims = np.zeros(6, dtype=np.int32); scal = np.zeros(3)
    _check(call(_ip(dims), _p(scal), *[None] * 9), "read_admm")
    np_, nblk, mEcap = (int(v) for v in dims[:3])
    FK = np.zeros((np_, np_))
    rhov, l, u, ya, za, dy = (np.zeros(mEcap) for _ in range(6))
    xa = np.zeros(np_); dx = np.zeros(np_)
    _check(call(_ip(dims), _p(scal), _p(FK), _p(rhov), _p(l), _p(u), _p(xa), _p(ya), _p(za), _p(dy), _p(dx)), "read_admm")
    return dict(np=np_, nblk=nblk, mEcap=mEcap, mE=int(dims[3]), kReady=int(dims[4]), setupFail=int(dims[5]), sigma=float(scal[0]),
                rhoAdmm=float(scal[1]), scale=float(scal[2]), FK=FK, rhov=rhov, l=l, u=u, xa=xa, ya=ya, za=za, dy=dy, dx=dx)


POLISH_V = ("xt", "xs", "xref", "r1s", "gs", "aty", "qxn", "xq")
POLISH_M = ("yt", "ex", "exs", "mg", "rn", "hotv", "ylv", "l", "u", "yq")
POLISH_I = ("stt", "st", "dep", "row_slot", "hotc")
POLISH_LDS_ROWS = ("yt", "ex", "mg", "stt")


def _read_polish(call, homotopy):
    """call(dims, scal, V, M, I) -> rc: the state of the active-set polish of one instance as it lies on the device
    (lcqp_hip_batch_read_polish).  The vectors are cut to the n variables and the mE rows.  homotopy: the handle runs k_lcqp_run, whose
    small shapes keep yt, ex, mg and stt in LDS -- those four come back as None there (rowsInLds), never as stale numbers."""
    dims = np.zeros(12, dtype=np.int32); scal = np.zeros(7)
    _check(call(_ip(dims), _p(scal), None, None, None), "read_polish")
    np_, mEcap, mE = (int(v) for v in dims[:3])
    n = int(dims[10])
    V = np.zeros((len(POLISH_V), np_)); M = np.zeros((len(POLISH_M), mEcap)); I = np.zeros((len(POLISH_I), mEcap), dtype=np.int32)
    _check(call(_ip(dims), _p(scal), _p(V), _p(M), _ip(I)), "read_polish")
    out = dict(np=np_, mEcap=mEcap, mE=mE, nT=int(dims[3]), ns=int(dims[4]), ndep=int(dims[5]), rnReady=int(dims[6]), nHot=int(dims[7]),
               haveSolution=int(dims[8]), rowsInLds=int(dims[9]), n=n, capS=int(dims[11]), spv=float(scal[0]), work=scal[1:].copy())
    out.update({k: V[i, :n].copy() for i, k in enumerate(POLISH_V)})
    out.update({k: M[i, :mE].copy() for i, k in enumerate(POLISH_M)})
    out.update({k: I[i, :mE].copy() for i, k in enumerate(POLISH_I)})
    if homotopy and out["rowsInLds"]:
        for k in POLISH_LDS_ROWS:
            out[k] = None
    return out


def _sensitivity(call, v, B, nV, nd, check=None):
    """call(nrhs, v, dg, db, side, info) -> rc; check(rc, what) raises with the error string of the caller's arm (default: the dense one).  v: [B][nV] or [B][k][nV]; returns (dg, db, side, info) with dg shaped like v, db
    [B][nd] or [B][k][nd], side [B][nd] (int32), info [B] (int32)."""
    v = _arr(v)
    single = v.ndim == 2
    if v.ndim not in (2, 3) or v.shape[0] != B or v.shape[-1] != nV or v.size == 0:
        raise ValueError(f"v: expected [{B}][{nV}] or [{B}][k][{nV}], got shape {v.shape}")
    k = 1 if single else v.shape[1]
    dg = np.zeros((B, k, nV)); db = np.zeros((B, k, nd)); side = np.zeros((B, nd), dtype=np.int32); info = np.zeros(B, dtype=np.int32)
    (check or _check)(call(k, _p(v), _p(dg), _p(db), _ip(side), _ip(info)), "sensitivity")
    return (dg[:, 0], db[:, 0], side, info) if single else (dg, db, side, info)


def _adjoint(call, vx, vy, B, nV, nd, shapes, matrices, lead, check=None):
    """call(vx, vy, dg, db, side, info, *matrix outputs in the order of `shapes`) -> rc.  vx [B][nV]; vy [B][nd] or None; shapes: name ->
    (rows, nV) of every matrix the entry point has; matrices: the names asked for; lead: () for sums over the batch, (B,) otherwise.
    Returns a dict with dg [B][nV], db [B][nd], side [B][nd], info [B] and one array per name in `matrices`."""
    vx = _arr(vx); vy = _arr(vy)
    if vx.shape != (B, nV):
        raise ValueError(f"vx: expected [{B}][{nV}], got shape {vx.shape}")
    if vy is not None and vy.shape != (B, nd):
        raise ValueError(f"vy: expected [{B}][{nd}], got shape {vy.shape}")
    unknown = set(matrices) - set(shapes)
    if unknown:
        raise ValueError(f"matrices: unknown names {sorted(unknown)} (this object has {sorted(shapes)})")
    out = dict(dg=np.zeros((B, nV)), db=np.zeros((B, nd)), side=np.zeros((B, nd), dtype=np.int32), info=np.zeros(B, dtype=np.int32))
    mats = {k: np.zeros(tuple(lead) + shp) for k, shp in shapes.items() if k in matrices}
    (check or _check)(call(_p(vx), _p(vy), _p(out["dg"]), _p(out["db"]), _ip(out["side"]), _ip(out["info"]), *[_p(mats.get(k)) for k in shapes]), "adjoint")
    out.update(mats)
    return out


SENS_PANEL = 16      # LCQP_SENS_PANEL: vectors per panel of the blocked sensitivity kernel


def _jacobian(call, B, nV, nd, first, count, bounds, check=None, rows=None):
    """call(first, count, Jg, Jb, side, info) -> rc on the instances [first, first + count) of B (count None: to the end).  Returns
    (Jg [count][nV][nV], Jb [count][nV][nd] or None, side [count][nd], info [count]); raises before any call on a range outside the batch.
    rows: the rows of the two blocks when they are not nV (the dual Jacobian: nd)."""
    if count is None:
        count = B - first
    if not (isinstance(first, (int, np.integer)) and isinstance(count, (int, np.integer))) or first < 0 or count < 1 or first + count > B:
        raise ValueError(f"jacobian: instances [{first}, {first} + {count}) are not inside the batch of {B}")
    rows = nV if rows is None else rows
    Jg = np.zeros((count, rows, nV)); Jb = np.zeros((count, rows, nd)) if bounds else None
    side = np.zeros((count, nd), dtype=np.int32); info = np.zeros(count, dtype=np.int32)
    (check or _check)(call(int(first), int(count), _p(Jg), _p(Jb), _ip(side), _ip(info)), "jacobian")
    return Jg, Jb, side, info


def _bound_slices(lo, hi, nV, nC, nComp, sparse):
    """lo / hi: db where the row sits on its lower / upper bound, zero elsewhere (numpy or torch), cut into the bound vectors"""
    a = 0 if sparse else nV
    l, r = a + nC, a + nC + nComp
    return dict(dlb=lo[..., :a], dub=hi[..., :a], dlbA=lo[..., a:l], dubA=hi[..., a:l], dlbL=lo[..., l:r], dubL=hi[..., l:r],
                dlbR=lo[..., r:], dubR=hi[..., r:])


def split_bound_derivatives(db, side, nV, nC, nComp, sparse=False):
    """db and side of a sensitivity call (the reference's dual layout: box rows first, then A, L, R; sparse=True: the layout of
    SparseBatchLCQP.sensitivity, which has no box rows -- dlb and dub are then empty) as derivatives with respect to the
    bound vectors of load / update: a dict with dlbA, dubA, dlbL, dubL, dlbR, dubR, dlb, dub, each shaped like its bound with the
    leading axes of db.  A row at its lower bound (side -1) gives its value to the lower bound's derivative, a row at its upper bound
    (+1) to the upper bound's.  An EQUALITY row (side 2, lower == upper) moves with either bound, and the ONE value db holds for it appears
    in both derivatives: it is the derivative along moving both bounds together (the only move that keeps the row an equality), so a
    caller who ties the two bounds to one parameter must count it once, not add the two entries."""
    db = np.asarray(db); side = np.asarray(side)
    sd = side if db.ndim == side.ndim else side[:, None, :]
    lo = np.where((sd == -1) | (sd == 2), db, 0.0); hi = np.where((sd == 1) | (sd == 2), db, 0.0)
    return _bound_slices(lo, hi, nV, nC, nComp, sparse)


def split_bound_derivatives_torch(db, side, nV, nC, nComp, sparse=False):
    """split_bound_derivatives on torch tensors, where they lie: the same selections, nothing through the host"""
    sd = side if db.dim() == side.dim() else side[:, None, :]
    zero = db.new_zeros(())
    lo = db.where((sd == -1) | (sd == 2), zero); hi = db.where((sd == 1) | (sd == 2), zero)
    return _bound_slices(lo, hi, nV, nC, nComp, sparse)


class SubsolverHIP:
    """Python view of the SubsolverBase-shaped QP object (include/SubsolverBase.hpp:28-58)."""

    def __init__(self, nV, nC, Q, A, opt=None, device=0):
        Q = _sized("Q", _arr(Q), nV * nV); A = _sized("A", _arr(A), nC * nV)
        if Q is None or (nC > 0 and A is None):
            raise ValueError("Q (and A when nC > 0) must be given")
        self.nV, self.nC = nV, nC
        self.opt = opt or default_options()
        self.h = lib().lcqp_hip_qp_create(nV, nC, _p(Q), _p(A), C.byref(self.opt), device)
        if not self.h:
            raise RuntimeError("lcqp_hip_qp_create failed: " + last_error())

    def clone(self):
        """lcqp_hip_qp_clone: the problem data, options, last solution and counters; the device state is built by the clone's first solve"""
        c = object.__new__(SubsolverHIP)
        c.nV, c.nC, c.opt = self.nV, self.nC, type(self.opt).from_buffer_copy(self.opt)
        c.h = lib().lcqp_hip_qp_clone(self.h)
        if not c.h:
            raise RuntimeError("lcqp_hip_qp_clone failed: " + last_error())
        return c

    def solve(self, initialSolve, g, lbA=None, ubA=None, x0=None, y0=None, lb=None, ub=None):
        it = C.c_int(0); ef = C.c_int(0)
        n, m = self.nV, self.nC
        a = [_sized(nm, _arr(v), sz) for nm, v, sz in (("g", g, n), ("lbA", lbA, m), ("ubA", ubA, m), ("x0", x0, n), ("y0", y0, n + m),
                                                       ("lb", lb, n), ("ub", ub, n))]
        ret = lib().lcqp_hip_qp_solve(self.h, int(bool(initialSolve)), C.byref(it), C.byref(ef), *[_p(v) for v in a])
        return ret, it.value, ef.value

    def getSolution(self):
        x = np.zeros(self.nV); y = np.zeros(self.nV + self.nC)
        lib().lcqp_hip_qp_get_solution(self.h, _p(x), _p(y))
        return x, y

    def sensitivity(self, v, blocked=False):
        """lcqp_hip_qp_sensitivity: derivatives of the solution of the QP last solved.  v: [nV] or [k][nV] upstream gradients dl/dx;
        returns (dg, db, side, info): dl/dg shaped like v, dl/d(bound) [nV + nC] or [k][nV + nC], side [nV + nC], info (int; 0 =
        differentiable) -- see BatchLCQP.sensitivity.  blocked: lcqp_hip_qp_sensitivity_blocked."""
        v = _arr(v)
        f = lib().lcqp_hip_qp_sensitivity_blocked if blocked else lib().lcqp_hip_qp_sensitivity
        dg, db, side, info = _sensitivity(lambda *a: f(self.h, *a), v[None], 1, self.nV, self.nV + self.nC)
        return dg[0], db[0], side[0], int(info[0])

    def jacobian(self, bounds=True):
        """lcqp_hip_qp_jacobian: (Jg [nV][nV] = dx/dg, Jb [nV][nV + nC] = dx/d(bound) or None, side [nV + nC], info) of the QP last
        solved -- see BatchLCQP.jacobian."""
        Jg, Jb, side, info = _jacobian(lambda first, count, *a: lib().lcqp_hip_qp_jacobian(self.h, *a), 1, self.nV, self.nV + self.nC, 0, 1, bounds)
        return Jg[0], (Jb[0] if bounds else None), side[0], int(info[0])

    def adjoint(self, vx, vy=None, matrices=("Q", "A")):
        """lcqp_hip_qp_adjoint: BatchLCQP.adjoint on the QP last solved.  vx [nV], vy [nV + nC] or None; returns a dict with dg [nV], db and
        side [nV + nC], info (int) and, as `matrices` asks, Q [nV][nV] and A [nC][nV] (the gradients in the matrices of the constructor)."""
        n, m = self.nV, self.nC
        vx = _arr(vx); vy = _arr(vy)
        r = _adjoint(lambda *a: lib().lcqp_hip_qp_adjoint(self.h, *a), vx[None], None if vy is None else vy[None], 1, n, n + m,
                     dict(Q=(n, n), A=(m, n)), matrices, ())
        return {k: (int(v[0]) if k == "info" else v[0] if k in ("dg", "db", "side") else v) for k, v in r.items()}

    def read_setup(self):
        """the constant matrices of the last fresh solve (test and diagnostic entry point; see BatchLCQP.read_setup)"""
        return _read_setup(lambda *a: lib().lcqp_hip_qp_read_setup(self.h, *a))

    def read_admm(self):
        """the state of the ADMM fallback as the last solve that ran it left it (test and diagnostic entry point; see BatchLCQP.read_admm)"""
        return _read_admm(lambda *a: lib().lcqp_hip_qp_read_admm(self.h, *a))

    def read_polish(self):
        """the state of the active-set polish as the last solve left it, accepted or given up (test and diagnostic entry point; see
        BatchLCQP.read_polish).  k_qp_solve works on the global row arrays: every vector is current."""
        return _read_polish(lambda *a: lib().lcqp_hip_qp_read_polish(self.h, *a), homotopy=False)

    def read_working_set(self):
        """the inverse factor the last solve left (test and diagnostic entry point; see BatchLCQP.read_working_set)"""
        dims = np.zeros(9, dtype=np.int32)
        _check(lib().lcqp_hip_qp_read_setup(self.h, _ip(dims), *[None] * 9), "read_setup")
        return _read_working_set(lambda *a: lib().lcqp_hip_qp_read_working_set(self.h, *a), int(dims[4]), int(dims[6]))

    def counters(self):
        v = [C.c_int(0) for _ in range(4)]
        lib().lcqp_hip_qp_get_counters(self.h, *[C.byref(t) for t in v])
        return dict(admm=v[0].value, trials=v[1].value, factorizations=v[2].value, corrections=v[3].value)

    def close(self):
        if self.h:
            lib().lcqp_hip_qp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_mixed(problems, opt=None, device=0):
    """A list of LCQPs of DIFFERENT shapes in one call: the Python twin of LCQPow::MixedBatchLCQProblem (lcqpow_amd/csrc/host/BatchLCQProblem.hpp).
    problems: dicts with nV, nC, nComp, Q, g, L, R and optionally lbL, ubL, lbR, ubR, A, lbA, ubA, lb, ub, x0, y0 (the argument list of
    LCQProblem::loadLCQP).  They are sorted into buckets of equal (nV, nC, nComp, box bounds or not), one BatchLCQP per bucket created for
    exactly that shape -- every instance gets the bits of its solo run -- and bucket k + 1 is created, loaded and launched while bucket k
    runs.  Within a bucket instances may differ in which optional arguments they carry.  Returns one dict per problem, in input order:
    ret (the reference's ReturnValue), x, y, stats."""
    keys = ("lbL", "ubL", "lbR", "ubR", "A", "lbA", "ubA", "lb", "ub", "x0", "y0")
    buckets = {}
    for i, d in enumerate(problems):
        box = d.get("lb") is not None or d.get("ub") is not None
        buckets.setdefault((d["nV"], d["nC"], d["nComp"], box), []).append(i)
    out = [None] * len(problems)

    def collect(bt, members):
        x, y, st = bt.solution()
        for s_, i in enumerate(members):
            out[i] = dict(ret=st[s_]["returnValue"], x=x[s_], y=y[s_], stats=st[s_])
        bt.close()

    flying = None
    for (nV, nC, nComp, box), members in buckets.items():
        bt = BatchLCQP(len(members), nV, nC, nComp, with_box=box, device=device, opt=opt)
        if len(buckets) > 1: bt.set_overlapped(True)      # its setup runs beside the homotopy of the bucket launched before it
        failed = False
        for s_, i in enumerate(members):
            d = problems[i]
            rc = bt.load(s_, 1, d["Q"], d["g"], d["L"], d["R"], **{k: d.get(k) for k in keys})
            if rc != 0:      # as LCQProblem::loadLCQP: the code is the problem's result, the others of the bucket are not run with a hole among them
                for j in members:
                    out[j] = dict(ret=int(rc) if j == i else 300, x=None, y=None, stats=None)
                failed = True
                break
        if failed:
            bt.close()
            continue
        bt.run()                       # asynchronous on the bucket's own stream
        if flying is not None:
            collect(*flying)           # the bucket before ran while this one was created and loaded
        flying = (bt, members)
    if flying is not None:
        collect(*flying)
    return out


class BatchPipeline:
    """A stream of batches over `depth` BatchLCQP objects (each has its own HIP stream; run() only launches): the host-side twin of
    LCQPow::BatchPipeline (lcqpow_amd/csrc/host/BatchLCQProblem.hpp).  acquire() hands out the object to fill next --
    a free one, else the oldest one in flight after waiting for it (its results are then read with .solution())."""

    def __init__(self, depth, batch, nV, nC, nComp, with_box=False, device=0, opt=None, over=None):
        # over: existing BatchLCQP objects to run the pipeline over (not closed by close()).  HIP maps the streams of a process onto a few
        # hardware queues (4 by default, GPU_MAX_HW_QUEUES); every batch object has two streams, so a process that keeps more than two batch
        # objects alive can find both slots of a pipeline on one queue -- and its batches run one after the other (tools/micro/pipeline_check.py:
        # 35 200 LCQPs/s with two objects alive, 30 750 with an idle third one, 34 800 again with GPU_MAX_HW_QUEUES=8)
        if "GPU_MAX_HW_QUEUES" not in os.environ:
            import warnings
            warnings.warn("BatchPipeline with the HIP runtime's default of 4 hardware queues: with more batch objects alive than the pipeline's, "
                          "two slots can share a queue and run one after the other; call lcqpow_amd.request_hw_queues() before the first HIP "
                          "call of the process, or set GPU_MAX_HW_QUEUES", RuntimeWarning, stacklevel=2)
        self.owned = over is None
        self.slots = list(over) if over is not None else [BatchLCQP(batch, nV, nC, nComp, with_box=with_box, device=device, opt=opt) for _ in range(depth)]
        if len(self.slots) > 1:
            for bt in self.slots: bt.set_overlapped(True)      # the setup of one slot runs beside the homotopy of another
        self.state = [0] * len(self.slots)          # 0 free, 1 in flight, 2 finished
        self.order = []

    def acquire(self):
        # (a slot that was handed out with results and not launched again is free again; with nothing in flight every slot is)
        self.state = [0 if s == 2 else s for s in self.state]
        if not self.order:
            self.state = [0] * len(self.slots)
        for k, s in enumerate(self.state):
            if s == 0:
                return self.slots[k], False
        k = self.order.pop(0)
        self.slots[k].synchronize()
        self.state[k] = 2
        return self.slots[k], True        # (object, it carries a finished run)

    def launch(self, bt, resolve=None, rho0=None):
        """resolve: None launches bt.run(); False / True launch bt.resolve(warm=resolve, rho0=rho0) on the setup bt holds"""
        k = self.slots.index(bt)
        if resolve is None:
            bt.run()
        else:
            bt.resolve(warm=resolve, rho0=rho0)
        self.state[k] = 1
        self.order.append(k)

    def drain(self):
        """the batches still in flight, oldest first"""
        while self.order:
            k = self.order.pop(0)
            self.slots[k].synchronize()
            self.state[k] = 0
            yield self.slots[k]

    def close(self):
        if self.owned:
            for s in self.slots:
                s.close()
        elif len(self.slots) > 1:
            for s in self.slots:
                s.set_overlapped(False)      # the caller's objects run alone again


class _Batch:
    """What BatchLCQP and SparseBatchLCQP have in common: the entry points both arms of the C ABI export under their own prefix.  A
    subclass sets _prefix ("lcqp_hip_batch_" / "lcqp_hip_sparse_"), _ndual (entries of an instance's dual vector), _last_error()
    (the arm's error string), _vectors (the vectors of a load / update in the C argument order, each with the attribute that holds its
    length), _shapes (the matrices of adjoint by name, each with the shape of one instance's gradient) and _staging_setter (the entry
    point that sets the staging cap of jacobian and adjoint).  It keeps its constructor, load / update (the argument orders differ),
    the calls whose defaults differ (adjoint, adjoint_device, sensitivity_device: their bodies are here) and the arm-only methods."""

    def _sym(self, name):
        return getattr(lib(), self._prefix + name)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with code {rc}: {self._last_error()}")

    def _call(self, name, *args):
        self._check(self._sym(name)(self.h, *args), name)

    def set_options(self, opt):
        self._call("set_options", C.byref(opt))

    def run(self):
        self._call("run")

    def resolve(self, warm=False, rho0=None):
        """*_resolve: solve again on the setup in place (asynchronous like run).  warm: instances whose last run succeeded start from
        their last solution, working set and penalty (rho0: [B] starting penalties, each finite and > 0, instead of the last rhoOpt);
        the others, and all of them without warm, start cold -- the bits of a fresh object."""
        r = _sized("rho0", _arr(rho0), self.B)
        self._call("resolve", 1 if warm else 0, _p(r))

    def launch_counts(self):
        """(full setups, homotopy launches) this object has issued"""
        out = (C.c_int * 2)()
        self._call("launch_counts", out)
        return out[0], out[1]

    def sensitivity(self, v):
        """*_sensitivity: adjoint derivatives of the x the last run / resolve returned (synchronous; DESIGN.md sections 3a', 3a'').
        v: upstream gradients dl/dx, [B][nV] or [B][k][nV].  Returns (dg, db, side, info): dg = dl/dg shaped like v; db [B][nd] or
        [B][k][nd], entry r = dl/d(the bound row r sits on) in the layout of the arm's dual vector (dense: box rows first, then A, L, R,
        nd = nV + nC + 2 nComp; sparse: A, L, R, nd = nC + 2 nComp), zero for rows outside the working set; side [B][nd]: 0 outside,
        -1 at lower, +1 at upper, 2 equality (split_bound_derivatives turns db and side into derivatives per bound vector; sparse=True
        for the sparse arm); info [B]: 0 = differentiable, else the flag bits of include/lcqp_hip.h.  The call changes nothing on the
        device."""
        return _sensitivity(lambda *a: self._sym("sensitivity")(self.h, *a), v, self.B, self.nV, self._ndual, check=self._check)

    def sensitivity_kernel_ms(self):
        """kernel time of the last sensitivity call (HIP events around k_sensitivity / k_sparse_sensitivity)"""
        ms = C.c_float(0)
        self._call("sensitivity_timing", C.byref(ms))
        return ms.value

    def synchronize(self):
        self._call("synchronize")

    def last_timing(self):
        a = C.c_float(0); b = C.c_float(0)
        self._call("last_timing", C.byref(a), C.byref(b))
        return a.value, b.value

    def solution(self):
        x = np.zeros((self.B, self.nV)); y = np.zeros((self.B, self._ndual))
        st = (Stats * self.B)()
        self._call("get_solution", _p(x), _p(y), st)
        return x, y, [s.asdict() for s in st]

    def trace(self, instance, cap=1024):
        """per-iterate (|statk|inf, phi, rho, alphak, obj, merit, |pk|inf, QP iterations) and xk of one instance (needs options.storeSteps)"""
        sc = np.zeros((cap, 8)); xs = np.zeros((cap, self.nV)); n = C.c_int(0)
        self._call("get_trace", instance, cap, _p(sc), _p(xs), C.byref(n))
        return sc[:n.value].copy(), xs[:n.value].copy()

    def algorithmic_bytes(self):
        return self._sym("algorithmic_bytes")(self.h)

    def _vector_sizes(self):
        """[(name, doubles per instance)] of the vectors of a load / update, in the C argument order"""
        return [(nm, getattr(self, attr)) for nm, attr in self._vectors]

    @staticmethod
    def _host_args(table, count, values):
        """`values` in the order of `table` [(name, doubles per instance)] as the contiguous float64 arrays of a host load / update"""
        return [_sized(nm, _arr(v), count * sz) for (nm, sz), v in zip(table, values)]

    @contextlib.contextmanager
    def _staging(self, nbytes):
        """another staging cap for the calls inside (None: the cap stays as it is), the default cap again afterwards"""
        if nbytes is not None:
            self._call(self._staging_setter, int(nbytes))
        try:
            yield
        finally:
            if nbytes is not None:
                self._call(self._staging_setter, 0)      # back to the default cap

    def jacobian(self, first=0, count=None, bounds=True, _staging_bytes=None):
        """*_jacobian: the full solution Jacobians of the instances [first, first + count) (count None: to the end) at the x the last
        run / resolve returned (synchronous; DESIGN.md section 3a''', for the sparse arm "The sparse arm" there).  Returns (Jg, Jb, side,
        info): Jg [count][nV][nV], Jg[i][k][j] = dx_k/dg_j; Jb [count][nV][nd], Jb[i][k][r] = dx_k/d(the bound row r sits on) in the
        layout of the arm's dual vector (dense: box rows first, then A, L, R, nd = nV + nC + 2 nComp; sparse: the rows of [A; L; R],
        nd = m = nC + 2 nComp), zero outside the working set (None with bounds=False); side [count][nd] and info [count] as sensitivity.
        The unit vectors are generated on the device, and the call goes in chunks under the arm's staging cap, the one adjoint uses
        (dense: chunks of instances; sparse: chunks of (instance, panel) work items; _staging_bytes: another cap for this one call,
        for tests).  The call changes nothing on the device."""
        with self._staging(_staging_bytes):
            return _jacobian(lambda *a: self._sym("jacobian")(self.h, *a), self.B, self.nV, self._ndual, first, count, bounds, check=self._check)

    def _pairs(self, VX, VY, conv):
        """the shapes of a blocked adjoint call: VX [B][k][nV] or None, VY [B][k][nd] or None, not both None; returns (VX, VY, k)"""
        VX, VY = conv(VX), conv(VY)
        if VX is None and VY is None:
            raise ValueError("adjoint_blocked: VX and VY are both None")
        k = (VX if VX is not None else VY).shape[1] if (VX if VX is not None else VY).ndim == 3 else 0
        for name, a, width in (("VX", VX, self.nV), ("VY", VY, self.nd)):
            if a is not None and (a.ndim != 3 or k < 1 or tuple(a.shape) != (self.B, k, width)):
                raise ValueError(f"{name}: expected [{self.B}][k][{width}] with k >= 1, got shape {tuple(a.shape)}")
        return VX, VY, k

    def adjoint_blocked(self, VX, VY=None):
        """*_adjoint_blocked: adjoint() without matrices for k pairs per instance, in panels on the arm's blocked kernel (DESIGN.md section
        3a''''; dense: panels of SENS_PANEL on the matrix cores, sparse: panels of sens_panel() columns per lane group).  VX [B][k][nV] = dl/dx
        or None, VY [B][k][nd] = dl/dy in the layout of solution()'s y or None (not both; entries of VY outside the working set are dropped).
        Returns (dg [B][k][nV], db [B][k][nd], side [B][nd], info [B]).  With VY None the call is the arm's blocked sensitivity call, to the
        bit; with VX None the first block is a zero panel (dense: the forward substitution is not run)."""
        VX, VY, k = self._pairs(VX, VY, _arr)
        B, n, nd = self.B, self.nV, self.nd
        dg = np.zeros((B, k, n)); db = np.zeros((B, k, nd)); side = np.zeros((B, nd), dtype=np.int32); info = np.zeros(B, dtype=np.int32)
        self._call("adjoint_blocked", k, _p(VX), _p(VY), _p(dg), _p(db), _ip(side), _ip(info))
        return dg, db, side, info

    def jacobian_duals(self, first=0, count=None, bounds=True, _staging_bytes=None):
        """*_jacobian_duals: the dual rows of the solution Jacobian of the instances [first, first + count) (count None: to the
        end).  Returns (Jyg, Jyb, side, info): Jyg [count][nd][nV], Jyg[i][r][j] = dy_r/dg_j; Jyb [count][nd][nd], Jyb[i][r][s] =
        dy_r/d(the bound row s sits on) (None with bounds=False); rows and columns outside the working set are zero.  The unit vectors of
        the working set are generated on the device; the call goes in chunks under the staging cap of jacobian (dense: chunks of instances; sparse: chunks of
        (instance, panel) work items; _staging_bytes: another cap for this one call, for tests)."""
        with self._staging(_staging_bytes):
            return _jacobian(lambda *a: self._sym("jacobian_duals")(self.h, *a), self.B, self.nV, self.nd, first, count, bounds, check=self._check,
                             rows=self.nd)

    def _adjoint_host(self, vx, vy, matrices, reduce, _staging_bytes):
        """the body of adjoint (a subclass's own: the default of `matrices` differs)"""
        with self._staging(_staging_bytes):
            f = self._sym("adjoint")
            call = lambda vx, vy, dg, db, side, info, *m: f(self.h, vx, vy, dg, db, side, info, 1 if reduce else 0, *m)
            return _adjoint(call, vx, vy, self.B, self.nV, self._ndual, self._shapes, matrices, () if reduce else (self.B,), check=self._check)

    # ---- what the device-pointer entry points of both arms share (DESIGN.md section 3a'''''): the checks of a tensor argument, the
    # stream the call is ordered behind, the range of instances, and the calls that differ in nothing but _ndual and _shapes: torch tensors
    # on the handle's device in, torch tensors out; the work is ordered behind torch.cuda.current_stream(), and what the caller enqueues
    # there next sees the results.  No copy through the host.  A subclass sets self.device.
    def _dev(self, name, t, shapes, optional=True):
        """the device address of a tensor argument (None: NULL) after the checks the C side cannot make: a float64, contiguous torch tensor
        on the handle's device of one of `shapes`; anything else raises ValueError"""
        import torch
        if t is None:
            if optional:
                return None
            raise ValueError(f"{name}: must be given")
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch tensor on the device of the batch, got {type(t).__name__}")
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous float64 tensor, got {t.dtype}{'' if t.is_contiguous() else ', not contiguous'}")
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError(f"{name}: expected a tensor on cuda:{self.device}, got one on {t.device}")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{name}: expected shape {' or '.join(str(list(s)) for s in shapes)}, got {list(t.shape)}")
        return t.data_ptr() if t.numel() else None

    def _stream(self):
        """the current torch stream of the handle's device.  Raises when the library and torch do not share one HIP runtime (lib())."""
        import torch
        lib()
        if _runtime != "torch" and _torch_hip_runtime():
            raise RuntimeError("the device-pointer entry points need the library and torch on ONE HIP runtime: import torch before the first "
                               "use of lcqpow_amd (the library was loaded first and is bound to the system's runtime)")
        return torch.cuda.current_stream(self.device).cuda_stream

    def _range(self, first, count):
        if not (isinstance(first, int) and isinstance(count, int)) or first < 0 or count <= 0 or first + count > self.B:
            raise ValueError(f"instances [{first}, {first} + {count}) outside the batch of {self.B}")

    def _device_vectors(self, count, values):
        """the device addresses of the vectors of a load_device / update_device, `values` in the order of _vectors; without g: all NULL"""
        if values[0] is None:
            return [None] * len(values)
        return [self._dev(nm, v, ((count, sz),)) for (nm, sz), v in zip(self._vector_sizes(), values)]

    def _device_matrices(self, count, named):
        """named: (name, tensor, shape of one instance's) of the matrix arguments of a load_device, in the bit order of its `shared` word.
        Returns (shared, {name: device address}): a tensor of one instance's shape is ONE for all `count` instances, its bit is set."""
        shared, ptr = 0, {}
        for bit, (nm, t, shp) in enumerate(named):
            ptr[nm] = self._dev(nm, t, (shp, (count,) + shp))
            if t is not None and t.dim() == len(shp):
                shared |= 1 << bit
        return shared, ptr

    def _results(self, lead):
        """fresh tensors for (dg, db, side, info) of a derivative call: dg lead + [nV], db lead + [nd]"""
        import torch
        dev = torch.device("cuda", self.device)
        return (torch.empty(lead + (self.nV,), dtype=torch.float64, device=dev), torch.empty(lead + (self._ndual,), dtype=torch.float64, device=dev),
                torch.empty((self.B, self._ndual), dtype=torch.int32, device=dev), torch.empty(self.B, dtype=torch.int32, device=dev))

    def solution_device(self, stats=False):
        """*_get_solution_device: (x [B][nV], y [B][nd]) as float64 tensors on the handle's device (y as solution() returns it: dense in
        the reference's dual layout, nd = nV + nC + 2 nComp; sparse nd = m, rows A, L, R), ordered behind the run on the current torch
        stream; nothing waits on the host.  stats=True: a third tensor, [B][sizeof(lcqp_stats_t)] bytes (Stats.from_buffer_copy reads
        an entry once it is on the host)."""
        import torch
        dev = torch.device("cuda", self.device)
        x = torch.empty((self.B, self.nV), dtype=torch.float64, device=dev); y = torch.empty((self.B, self._ndual), dtype=torch.float64, device=dev)
        st = torch.empty((self.B, C.sizeof(Stats)), dtype=torch.uint8, device=dev) if stats else None
        self._call("get_solution_device", x.data_ptr(), y.data_ptr(), st.data_ptr() if stats else None, self._stream())
        return (x, y, st) if stats else (x, y)

    def _sensitivity_device(self, v, *flags):
        """the body of sensitivity_device; flags: what the arm's entry point takes in front of the number of vectors"""
        import torch
        B, n = self.B, self.nV
        if isinstance(v, torch.Tensor) and v.dim() == 3 and v.shape[1] < 1:
            raise ValueError("v: no vectors")
        k = v.shape[1] if isinstance(v, torch.Tensor) and v.dim() == 3 else 1
        pv = self._dev("v", v, ((B, n), (B, k, n)), optional=False)
        dg, db, side, info = self._results((B,) if v.dim() == 2 else (B, k))
        self._call("sensitivity_device", *flags, k, pv, dg.data_ptr(), db.data_ptr(), side.data_ptr(), info.data_ptr(), self._stream())
        return dg, db, side, info

    def _adjoint_device(self, vx, vy, matrices, reduce, out):
        """the body of adjoint_device (a subclass's own: the default of `matrices` differs)"""
        import torch
        B, shapes = self.B, self._shapes
        unknown = set(matrices) - set(shapes)
        if unknown:
            raise ValueError(f"matrices: unknown names {sorted(unknown)} (this object has {sorted(shapes)})")
        pvx = self._dev("vx", vx, ((B, self.nV),), optional=False); pvy = self._dev("vy", vy, ((B, self._ndual),))
        r = dict(zip(("dg", "db", "side", "info"), self._results((B,))))
        lead = () if reduce else (B,)
        mats = {}
        for k in shapes:
            if k in matrices:
                t = (out or {}).get(k)
                if t is None:      # the kernels write every entry except those of a matrix without rows
                    t = torch.empty(lead + shapes[k], dtype=torch.float64, device=r["dg"].device)
                self._dev(k, t, (lead + shapes[k],))
                mats[k] = t
        ptrs = [mats[k].data_ptr() if k in mats and mats[k].numel() else None for k in shapes]
        self._call("adjoint_device", pvx, pvy, r["dg"].data_ptr(), r["db"].data_ptr(), r["side"].data_ptr(), r["info"].data_ptr(),
                   1 if reduce else 0, *ptrs, self._stream())
        r.update(mats)
        return r

    def adjoint_blocked_device(self, VX, VY=None):
        """*_adjoint_blocked_device: adjoint_blocked on float64 tensors of the handle's device, read where they lie; returns
        (dg, db, side, info) as tensors on that device"""
        import torch
        for name, t in (("VX", VX), ("VY", VY)):
            if t is not None and not isinstance(t, torch.Tensor):
                raise ValueError(f"{name}: expected a torch tensor on the device of the batch, got {type(t).__name__}")
        VX, VY, k = self._pairs(VX, VY, lambda t: t)
        B, n, nd = self.B, self.nV, self.nd
        pvx = self._dev("VX", VX, ((B, k, n),)); pvy = self._dev("VY", VY, ((B, k, nd),))
        dg, db, side, info = self._results((B, k))
        self._call("adjoint_blocked_device", k, pvx, pvy, dg.data_ptr(), db.data_ptr(), side.data_ptr(), info.data_ptr(), self._stream())
        return dg, db, side, info

    def _jacobian_device(self, name, rows, first, count, bounds):
        import torch
        if count is None:
            count = self.B - first
        self._range(first, count)
        n, nd = self.nV, self.nd
        dev = torch.device("cuda", self.device)
        Jg = torch.empty((count, rows, n), dtype=torch.float64, device=dev)
        Jb = torch.empty((count, rows, nd), dtype=torch.float64, device=dev) if bounds else None
        side = torch.empty((count, nd), dtype=torch.int32, device=dev); info = torch.empty(count, dtype=torch.int32, device=dev)
        self._call(name, first, count, Jg.data_ptr(), Jb.data_ptr() if bounds else None, side.data_ptr(), info.data_ptr(), self._stream())
        return Jg, Jb, side, info

    def jacobian_device(self, first=0, count=None, bounds=True):
        """*_jacobian_device: jacobian() written into tensors on the handle's device, (Jg, Jb, side, info)"""
        return self._jacobian_device("jacobian_device", self.nV, first, count, bounds)

    def jacobian_duals_device(self, first=0, count=None, bounds=True):
        """*_jacobian_duals_device: jacobian_duals() written into tensors on the handle's device, (Jyg, Jyb, side, info)"""
        return self._jacobian_device("jacobian_duals_device", self.nd, first, count, bounds)

    def close(self):
        if self.h:
            self._sym("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchLCQP(_Batch):
    """B independent dense LCQPs of one shape solved on one GPU (lcqp_hip_batch_*)."""
    _prefix = "lcqp_hip_batch_"
    _last_error = staticmethod(last_error)
    _staging_setter = "set_jacobian_staging"
    shared_matrices = False      # True: the batch holds one set of matrices (__init__)
    _vectors = (("g", "nV"), ("lbL", "nComp"), ("ubL", "nComp"), ("lbR", "nComp"), ("ubR", "nComp"), ("lbA", "nC"), ("ubA", "nC"),
                ("lb", "nV"), ("ub", "nV"), ("x0", "nV"), ("y0", "_ndual"))

    def __init__(self, batch, nV, nC, nComp, with_box=False, device=0, opt=None, shared_matrices=False):
        """shared_matrices: lcqp_hip_batch_create_shared -- the batch holds ONE Q, A, L, R, stored and set up once (DESIGN.md section 3a,
        "One set of matrices").  load / load_device / update_matrices(_device) then take 2-D matrices [rows][nV] and refuse 3-D ones; the
        set of box-bounded variables is one for the batch; everything else is as on an ordinary batch, to the bit."""
        self.B, self.nV, self.nC, self.nComp = batch, nV, nC, nComp
        self.nd = self._ndual = nV + nC + 2 * nComp
        self.device = device
        self.shared_matrices = bool(shared_matrices)
        create = lib().lcqp_hip_batch_create_shared if self.shared_matrices else lib().lcqp_hip_batch_create
        self.h = create(batch, nV, nC, nComp, int(with_box), device)
        if not self.h:
            raise RuntimeError("lcqp_hip_batch_create failed: " + last_error())
        if opt is not None:
            self.set_options(opt)

    def device_bytes(self):
        """lcqp_hip_batch_device_bytes: (bytes of device memory the handle's pools hold, the part of them held once for the batch --
        0 on an ordinary batch)."""
        out = (C.c_size_t * 2)()
        _check(lib().lcqp_hip_batch_device_bytes(self.h, out), "device_bytes")
        return int(out[0]), int(out[1])

    def _one_set(self, what, first, count, matrices, whole):
        """the refusals of a batch that holds one set of matrices, made before the C call: a matrix per instance, and (whole) a range
        that is not the batch; returns the instances the matrix arrays are sized for"""
        if not self.shared_matrices:
            return count
        for nm, m in matrices:
            if m is not None and (m.dim() if hasattr(m, "dim") else np.ndim(m)) != 2:
                raise ValueError(f"{what}: {nm} must be ONE matrix [rows][nV] -- this batch holds one set of matrices (shared_matrices=True)")
        if whole and (first != 0 or count != self.B):
            raise ValueError(f"{what}: this batch holds one set of matrices; they change for the whole batch (first=0, count={self.B})")
        return 1

    def set_overlapped(self, overlapped=True):
        """lcqp_hip_batch_set_overlapped: this object's setup runs beside another object's homotopy kernel (BatchPipeline sets it)."""
        _check(lib().lcqp_hip_batch_set_overlapped(self.h, 1 if overlapped else 0), "set_overlapped")

    def load(self, first, count, Q, g, L, R, lbL=None, ubL=None, lbR=None, ubR=None, A=None, lbA=None, ubA=None,
             lb=None, ub=None, x0=None, y0=None):
        """lcqp_hip_batch_load for instances [first, first + count).  Returns the reference's ReturnValue code (0, or e.g. 116
        INVALID_OBJECTIVE_LINEAR_TERM for g = None) like LCQProblem::loadLCQP does; a wrongly sized array raises ValueError."""
        n, nC, nK = self.nV, self.nC, self.nComp
        if first < 0 or count <= 0 or first + count > self.B:
            raise ValueError(f"instances [{first}, {first + count}) outside the batch of {self.B}")
        vec = self._vector_sizes()      # the C order: Q, g, L, R, the bounds of L and R, A, the rest
        # (a batch that holds one set of matrices takes one matrix each, or None: the one in place stays)
        nmat = self._one_set("load", first, count, (("Q", Q), ("L", L), ("R", R), ("A", A)), False)
        m = self._host_args((("Q", n * n), ("L", nK * n), ("R", nK * n), ("A", nC * n)), nmat, (Q, L, R, A))
        v = self._host_args(vec, count, (g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0))
        a = [m[0], v[0], m[1], m[2], *v[1:5], m[3], *v[5:]]
        return lib().lcqp_hip_batch_load(self.h, first, count, *[_p(v) for v in a])

    def sensitivity(self, v, blocked=False):
        """_Batch.sensitivity; blocked: lcqp_hip_batch_sensitivity_blocked, the kernel that takes the k vectors of an instance in panels
        of SENS_PANEL on the matrix cores (DESIGN.md section 3a''') -- the same results to rounding (not to the bit), faster from about
        a panel of vectors on; the default stays the vector kernel."""
        name = "sensitivity_blocked" if blocked else "sensitivity"
        return _sensitivity(lambda *a: self._sym(name)(self.h, *a), v, self.B, self.nV, self._ndual, check=self._check)

    @property
    def _shapes(self):
        n, nC, nK = self.nV, self.nC, self.nComp
        return dict(Q=(n, n), A=(nC, n), L=(nK, n), R=(nK, n))

    def adjoint(self, vx, vy=None, matrices=("Q", "A", "L", "R"), reduce=False, _staging_bytes=None):
        """lcqp_hip_batch_adjoint: the gradients of a loss that reads the x AND the y the last run / resolve returned (synchronous; DESIGN.md
        section 3a'''').  vx = dl/dx [B][nV]; vy = dl/dy [B][nd] in the dual layout, or None (entries on rows outside the working set are
        ignored).  Returns a dict: dg, db, side, info as sensitivity (one vector per instance), and under the names in `matrices` the
        gradients in Q [B][nV][nV] (symmetric), A [B][nC][nV], L and R [B][nComp][nV] -- with reduce=True their sums over the batch, [nV][nV]
        and so on, formed on the device (one matrix shared by all instances).  Rows outside the working set are zero; an instance with
        info & 1 contributes zeros.  Without reduce the matrices come in chunks of instances under the staging cap of jacobian
        (_staging_bytes: another cap for this one call, for tests).  The call changes nothing on the device."""
        return self._adjoint_host(vx, vy, matrices, reduce, _staging_bytes)

    # ---- the device-pointer entry points (DESIGN.md section 3a'''''): torch tensors on the handle's device in, torch tensors out; the work is
    # ordered behind torch.cuda.current_stream(), and what the caller enqueues there next sees the results.  No copy through the host.
    def load_device(self, first, count, Q, g, L, R, lbL=None, ubL=None, lbR=None, ubR=None, A=None, lbA=None, ubA=None,
                    lb=None, ub=None, x0=None, y0=None):
        """lcqp_hip_batch_load_device: load() from float64 torch tensors on the handle's device, packed into the pools by kernels.  A
        matrix of shape [rows][nV] is ONE matrix for all `count` instances (broadcast by the pack kernel), one of shape
        [count][rows][nV] holds one per instance; a matrix that is None stays as the batch holds it (every instance of the range must
        hold a problem then).  Returns the ReturnValue code like load; the pools hold the bytes load leaves."""
        n, nC, nK = self.nV, self.nC, self.nComp
        self._range(first, count)
        self._one_set("load_device", first, count, (("Q", Q), ("A", A), ("L", L), ("R", R)), False)
        shared, ptr = self._device_matrices(count, (("Q", Q, (n, n)), ("A", A, (nC, n)), ("L", L, (nK, n)), ("R", R, (nK, n))))
        v = self._device_vectors(count, (g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0))
        return lib().lcqp_hip_batch_load_device(self.h, first, count, shared, ptr["Q"], v[0], ptr["L"], ptr["R"], *v[1:5], ptr["A"], *v[5:],
                                                self._stream())

    def update_device(self, first, count, g, lbL=None, ubL=None, lbR=None, ubR=None, lbA=None, ubA=None, lb=None, ub=None, x0=None, y0=None):
        """lcqp_hip_batch_update_device: update() from float64 torch tensors on the handle's device.  Returns the ReturnValue code."""
        self._range(first, count)
        v = self._device_vectors(count, (g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0))
        return lib().lcqp_hip_batch_update_device(self.h, first, count, *v, self._stream())

    def update_matrices_device(self, first, count, Q=None, L=None, R=None, A=None, shared=0):
        """lcqp_hip_batch_update_matrices_device: update_matrices() from float64 torch tensors on the handle's device.  As in
        load_device a matrix of shape [rows][nV] is ONE matrix for all `count` instances; shared (bits 1, 2, 4, 8 for Q, A, L, R) may
        say so too, and must then agree with the shapes.  Returns the ReturnValue code."""
        n, nC, nK = self.nV, self.nC, self.nComp
        self._range(first, count)
        self._one_set("update_matrices_device", first, count, (("Q", Q), ("A", A), ("L", L), ("R", R)), True)
        found, ptr = self._device_matrices(count, (("Q", Q, (n, n)), ("A", A, (nC, n)), ("L", L, (nK, n)), ("R", R, (nK, n))))
        if count > 1 and shared & ~found:
            raise ValueError(f"shared = {shared}: a matrix marked as shared has the shape of one per instance")
        return lib().lcqp_hip_batch_update_matrices_device(self.h, first, count, found, ptr["Q"], ptr["L"], ptr["R"], ptr["A"], self._stream())

    def sensitivity_device(self, v, blocked=False):
        """lcqp_hip_batch_sensitivity_device: sensitivity(v, blocked) with v a float64 tensor on the handle's device, [B][nV] or
        [B][k][nV], read where it lies; returns (dg, db, side, info) as tensors on that device (side, info: int32)."""
        return self._sensitivity_device(v, 1 if blocked else 0)

    def adjoint_device(self, vx, vy=None, matrices=("Q", "A", "L", "R"), reduce=False, out=None):
        """lcqp_hip_batch_adjoint_device: adjoint(vx, vy, matrices, reduce) with float64 tensors on the handle's device in and out -- the
        matrix gradients are written by ONE launch straight into their tensors, whatever their size (no staging, no chunks).  out: tensors
        to write the matrix gradients into, by name (16-byte aligned; default: fresh ones).  Returns the dict of adjoint, of tensors."""
        return self._adjoint_device(vx, vy, matrices, reduce, out)

    def generate_synthetic(self, first_instance=0, seed0=SEED0):
        _check(lib().lcqp_hip_batch_generate_synthetic(self.h, seed0, first_instance), "generate_synthetic")

    def update(self, first, count, g, lbL=None, ubL=None, lbR=None, ubR=None, lbA=None, ubA=None, lb=None, ub=None, x0=None, y0=None):
        """lcqp_hip_batch_update: new vectors for instances [first, first + count), the matrices stay.  Returns the ReturnValue code like
        load (0; 100 INVALID_ARGUMENT when the set of box-bounded variables would change -- see last_error()); a wrongly sized array
        raises ValueError."""
        if first < 0 or count <= 0 or first + count > self.B:
            raise ValueError(f"instances [{first}, {first + count}) outside the batch of {self.B}")
        a = self._host_args(self._vector_sizes(), count, (g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0))
        return lib().lcqp_hip_batch_update(self.h, first, count, *[_p(v) for v in a])

    def update_matrices(self, first, count, Q=None, L=None, R=None, A=None):
        """lcqp_hip_batch_update_matrices: new matrices for instances [first, first + count), None: the matrix stays; the vectors, the
        stored point, the statuses and the penalties stay.  The next resolve(warm=True) sets up again on the new matrices and starts
        every instance whose last run succeeded from its last solution and working set, with an empty inverse factor; resolve() and run()
        solve the new data cold.  Returns the ReturnValue code (0; 100 INVALID_ARGUMENT without any matrix, 300 for an instance that
        holds no problem); a wrongly sized array raises ValueError."""
        n, nC, nK = self.nV, self.nC, self.nComp
        if first < 0 or count <= 0 or first + count > self.B:
            raise ValueError(f"instances [{first}, {first + count}) outside the batch of {self.B}")
        nmat = self._one_set("update_matrices", first, count, (("Q", Q), ("L", L), ("R", R), ("A", A)), True)
        a = self._host_args((("Q", n * n), ("L", nK * n), ("R", nK * n), ("A", nC * n)), nmat, (Q, L, R, A))
        return lib().lcqp_hip_batch_update_matrices(self.h, first, count, *[_p(v) for v in a])

    def read_problem(self, b):
        n, nC, nComp = self.nV, self.nC, self.nComp
        Q = np.zeros((n, n)); g = np.zeros(n); L = np.zeros((nComp, n)); R = np.zeros((nComp, n))
        A = np.zeros((nC, n)); lbA = np.zeros(nC); ubA = np.zeros(nC)
        _check(lib().lcqp_hip_batch_read_problem(self.h, b, _p(Q), _p(g), _p(L), _p(R), _p(A), _p(lbA), _p(ubA)), "read_problem")
        return dict(Q=Q, g=g, L=L, R=R, A=A, lbA=lbA, ubA=ubA)

    def read_setup(self, b):
        """Test and diagnostic entry point: the raw padded device blocks of instance b after setup() or run() -- the dimensions np, nblk,
        mEcap, mMld, capS, capC and the instance's mE, cNnz, setupFail, spv, scale; C [np][np], F1 [np][np] (the symmetric-filled factor
        of Q + spv I), D1 [nblk][64][64] (its inverted diagonal blocks), Et [mEcap][np], MM [mMld][mMld] (lower triangle) and the
        compressed rows Cp, Ci, Cv of C."""
        return _read_setup(lambda *a: lib().lcqp_hip_batch_read_setup(self.h, b, *a))

    def read_working_set(self, b):
        """Test and diagnostic entry point: nT, ns, slot_row [capS], crow [capS], row_slot [mE] and Ti [capS][capS] of instance b as the
        last run left them."""
        dims = np.zeros(9, dtype=np.int32)
        _check(lib().lcqp_hip_batch_read_setup(self.h, b, _ip(dims), *[None] * 9), "read_setup")
        return _read_working_set(lambda *a: lib().lcqp_hip_batch_read_working_set(self.h, b, *a), int(dims[4]), int(dims[6]))

    def read_admm(self, b):
        """Test and diagnostic entry point: the ADMM fallback of instance b as the last QP that ran it left it -- np, nblk, mEcap, mE,
        kReady, setupFail, sigma, rhoAdmm, scale; FK [np][np] (the symmetric-filled factor of Q + sigma I + E' diag(rhov) E, inverted
        diagonal blocks), rhov, l, u, ya, za, dy [mEcap] and xa, dx [np]."""
        return _read_admm(lambda *a: lib().lcqp_hip_batch_read_admm(self.h, b, *a))

    def read_polish(self, b):
        """Test and diagnostic entry point (launches nothing): the active-set polish of instance b as the last QP left it -- the dimensions
        np, mEcap, mE, n, capS, nT, ns, ndep, rnReady, nHot, haveSolution, rowsInLds, spv (sigma_p), work (the six work sums); xt, xs, xref,
        r1s, gs, aty, qxn, xq [n]; yt, ex, exs, mg, rn, hotv, ylv, l, u, yq [mE]; stt, st, dep, row_slot, hotc [mE].  Where the homotopy
        kernel keeps the row state in LDS (rowsInLds: np <= 256, mEcap <= 640) yt, ex, mg and stt are None: they never reach their
        global arrays when a launch ends."""
        return _read_polish(lambda *a: lib().lcqp_hip_batch_read_polish(self.h, b, *a), homotopy=True)

    def setup(self):
        _check(lib().lcqp_hip_batch_setup(self.h), "setup")

    def work_sums(self):
        """batch totals counted by the kernel: rows of Et read by the corrections, rows x slots over the corrections, bytes and number of
        the working-set updates, rows of E read by the residual sweeps, triangular solves with L1 (include/lcqp_hip.h)"""
        out = np.zeros(6)
        _check(lib().lcqp_hip_batch_work_sums(self.h, _p(out)), "work_sums")
        return out

    def stream(self):
        return lib().lcqp_hip_batch_stream(self.h)


def util_symv(alpha, A, b, c):
    A = _arr(A); b = _arr(b); c = _arr(c)
    batch, n = A.shape[0], A.shape[1]
    d = np.zeros((batch, n))
    _check(lib().lcqp_hip_util_symv(batch, n, alpha, _p(A), _p(b), _p(c), _p(d)), "util_symv")
    return d


def util_gemv(A, b):
    A = _arr(A); b = _arr(b)
    batch, m, n = A.shape
    c = np.zeros((batch, m))
    _check(lib().lcqp_hip_util_gemv(batch, m, n, _p(A), _p(b), _p(c)), "util_gemv")
    return c


def util_gemv_t(A, b):
    A = _arr(A); b = _arr(b)
    batch, m, n = A.shape
    c = np.zeros((batch, n))
    _check(lib().lcqp_hip_util_gemv_t(batch, m, n, _p(A), _p(b), _p(c)), "util_gemv_t")
    return c


def util_rows_list(A, lists, x=None, coef=None, dots0=None):
    """wg_rows through a row list (lcqp_hip_util_rows_list): A [batch][m][n], lists [batch][nlist] -> (dots [batch][m], outT [batch][n])"""
    A = _arr(A); x = _arr(x); coef = _arr(coef)
    batch, m, n = A.shape
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    dots = np.zeros((batch, m)) if dots0 is None else np.ascontiguousarray(dots0, dtype=np.float64).copy()
    out = np.zeros((batch, n))
    _check(lib().lcqp_hip_util_rows_list(batch, m, n, _p(A), lists.ctypes.data_as(C.POINTER(C.c_int)), lists.shape[1], _p(x), _p(coef),
                                         _p(dots) if x is not None else None, _p(out) if coef is not None else None), "util_rows_list")
    return dots, out


def util_symm_product(A, B):
    A = _arr(A); B = _arr(B)
    batch, m, n = A.shape
    Cm = np.zeros((batch, n, n))
    _check(lib().lcqp_hip_util_symm_product(batch, m, n, _p(A), _p(B), _p(Cm)), "util_symm_product")
    return Cm


def chol_solve(K, b, repeat=1):
    K = _arr(K); b = _arr(b)
    batch, n = K.shape[0], K.shape[1]
    x = np.zeros((batch, n)); ms = C.c_float(0)
    _check(lib().lcqp_hip_chol_solve(batch, n, _p(K), _p(b), _p(x), repeat, C.byref(ms)), "chol_solve")
    return x, ms.value


class CSCMatrix:
    """Device copy of a CSC matrix (and its transpose) for the sparse Utilities products."""

    def __init__(self, m, n, p, i, x, device=0):
        self.m, self.n = m, n
        p = np.ascontiguousarray(p, dtype=np.int32); i = np.ascontiguousarray(i, dtype=np.int32); x = _arr(x)
        ip = C.POINTER(C.c_int)
        self.h = lib().lcqp_hip_csc_create(m, n, len(x), p.ctypes.data_as(ip), i.ctypes.data_as(ip), _p(x), device)
        if not self.h:
            raise RuntimeError("lcqp_hip_csc_create failed: " + last_error())

    def apply(self, b, transposed=False, alpha=1.0, c=None, repeat=1):
        b = _arr(b); c = _arr(c)
        d = np.zeros(self.n if transposed else self.m); ms = C.c_float(0)
        _check(lib().lcqp_hip_csc_apply(self.h, int(transposed), alpha, _p(b), _p(c), _p(d), repeat, C.byref(ms)), "csc_apply")
        self.last_ms = ms.value
        return d

    def close(self):
        if self.h:
            lib().lcqp_hip_csc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SparseBatchLCQP(_Batch):
    """B independent sparse LCQPs of one sparsity pattern on one GPU (lcqp_hip_sparse_*): the reference's OSQP_SPARSE arm.
    Qpat / Apat: scipy-like CSC pattern objects with .indptr / .indices (Q full symmetric nV x nV; A the stacked [A; L; R],
    (nC + 2 nComp) x nV).  Values are loaded per instance in the CSC order of these patterns."""
    _prefix = "lcqp_hip_sparse_"
    _staging_setter = "set_adjoint_staging"
    _vectors = (("g", "nV"), ("lbA", "nC"), ("ubA", "nC"), ("lbL", "nComp"), ("ubL", "nComp"), ("lbR", "nComp"), ("ubR", "nComp"),
                ("x0", "nV"), ("y0", "_ndual"))

    def __init__(self, batch, nV, nC, nComp, Qpat, Apat, device=0, opt=None):
        self.B, self.nV, self.nC, self.nComp = batch, nV, nC, nComp
        self.m = self.nd = self._ndual = nC + 2 * nComp
        self.device = device
        self._pat = [np.ascontiguousarray(a, dtype=np.int32) for a in (Qpat.indptr, Qpat.indices, Apat.indptr, Apat.indices)]
        if self._pat[0].size != nV + 1 or self._pat[2].size != nV + 1:
            raise ValueError("pattern column pointers must have nV + 1 entries (CSC)")
        if self._pat[1].size != int(self._pat[0][-1]) or self._pat[3].size != int(self._pat[2][-1]):
            raise ValueError("pattern index arrays must have indptr[-1] entries")        # the C side reads exactly that many
        self.nnzQ, self.nnzA = int(self._pat[0][-1]), int(self._pat[2][-1])
        self.h = lib().lcqp_hip_sparse_create(batch, nV, nC, nComp, *[_ip(a) for a in self._pat], device)
        if not self.h:
            raise RuntimeError("lcqp_hip_sparse_create failed: " + self._last_error())
        if opt is not None:
            self.set_options(opt)

    @staticmethod
    def _last_error():
        return lib().lcqp_hip_sparse_last_error().decode()

    def bandwidth(self):
        return lib().lcqp_hip_sparse_bandwidth(self.h)

    def lanes(self):
        """lanes of a wavefront per instance (8, 16, 32 or 64: the smallest above the half bandwidth)"""
        return lib().lcqp_hip_sparse_lanes(self.h)

    def border(self):
        """border nodes of the bordered band: the last positions of ordering() (0: plain band)"""
        return lib().lcqp_hip_sparse_border(self.h)

    def fronts(self):
        """fronts of the general sparse LDL' (0: one of the band engines runs this pattern)"""
        return lib().lcqp_hip_sparse_fronts(self.h)

    def general_ordering(self):
        """lcqp_hip_sparse_general_ordering: 0 a band engine, 1 nested dissection, 2 minimum degree"""
        return lib().lcqp_hip_sparse_general_ordering(self.h)

    def ordering(self):
        perm = np.zeros(self.nV + self.m, dtype=np.int32)
        self._call("get_ordering", _ip(perm))
        return perm

    def kkt_probe(self, rhs, dprim=None, ddual=None, use=None, which=None):
        """Test and diagnostic entry point (lcqp_hip_sparse_kkt_probe; after a completed run / resolve): solves with a KKT factorisation of
        every instance, one solve per right-hand side, no refinement.  rhs [B][nrhs][nV + m] in node order (variables, then the rows of
        [A; L; R]); returns the solutions in the same shape.
        FACTOR mode (dprim [B], ddual [B][m], use [B][m] 0/1 given): factorises [Q + dprim I, E_use'; E_use, -diag(ddual)] (a row outside use:
        diagonal -1, no entries) into the polish slot first.  That overwrites the stored polish factor: sensitivity() then answers 300 and
        a warm resolve starts cold.  Returns sol.
        STORED mode (which = 0: the polish slot, 1: the ADMM slot): the factor as the last run left it.  Returns (sol, record) with
        record = dict(dprim [B], ddual [B][m], use [B][m]): the matrix that factor is the factor of."""
        B, N, m = self.B, self.nV + self.m, self.m
        rhs = _arr(rhs)
        if rhs.ndim != 3 or rhs.shape[0] != B or rhs.shape[2] != N or rhs.shape[1] < 1:
            raise ValueError(f"rhs: expected [{B}][nrhs][{N}], got shape {rhs.shape}")
        sol = np.zeros_like(rhs)
        if which is None:
            dp = _sized("dprim", _arr(dprim), B); dd = _sized("ddual", _arr(ddual), B * m)
            if dp is None or dd is None or use is None:
                raise ValueError("FACTOR mode needs dprim, ddual and use; STORED mode needs which")
            us = np.ascontiguousarray(use, dtype=np.int32)
            if us.size != B * m:
                raise ValueError(f"use: expected {B * m} values, got {us.size}")
            self._call("kkt_probe", 0, 0, rhs.shape[1], _p(dp), _p(dd), _ip(us), _p(rhs), _p(sol), None, None, None)
            return sol
        rp = np.zeros(B); rd = np.zeros((B, m)); ru = np.zeros((B, m), dtype=np.int32)
        self._call("kkt_probe", 1, int(which), rhs.shape[1], None, None, None, _p(rhs), _p(sol), _p(rp), _p(rd), _ip(ru))
        return sol, dict(dprim=rp, ddual=rd, use=ru)

    def sens_panel(self):
        """lcqp_hip_sparse_sens_panel: columns per panel of k_sparse_sensitivity_blk on this handle's engine; 0 where sensitivity_blocked()
        and jacobian() run the vector kernel (the general sparse LDL' before set_general_panel())"""
        return lib().lcqp_hip_sparse_sens_panel(self.h)

    def set_general_panel(self, on=True):
        """lcqp_hip_sparse_set_general_panel: on a handle of the general sparse LDL', sensitivity_blocked() and jacobian() through the panel
        kernel of that engine (off by default: the vector kernel and its bits).  No effect on a band engine.  Costs nothing and changes
        nothing on the device."""
        rc = lib().lcqp_hip_sparse_set_general_panel(self.h, int(on))
        if rc:
            raise ValueError(f"lcqp_hip_sparse_set_general_panel({on!r}) returned {rc}")
        return self

    def max_front(self):
        """lcqp_hip_sparse_max_front: the largest front of the general sparse LDL' (0: a band engine)"""
        return lib().lcqp_hip_sparse_max_front(self.h)

    def sensitivity_blocked(self, v):
        """lcqp_hip_sparse_sensitivity_blocked: sensitivity(v) -- the same arguments and results -- through the kernel that takes the k vectors
        of an instance in panels of sens_panel() columns, one lane group per (instance, panel) pair, the band factor streamed once per
        panel (DESIGN.md section 3a''', "The sparse arm"): per column the arithmetic of the vector kernel (the same results to rounding); a
        column's result does not depend on the other columns of the call, bit for bit.  (A method of its own rather than a keyword of
        sensitivity, whose signature (v) is part of this class's tested surface.)"""
        return _sensitivity(lambda *a: self._sym("sensitivity_blocked")(self.h, *a), v, self.B, self.nV, self._ndual, check=self._check)

    @property
    def _shapes(self):
        return dict(Q=(self.nnzQ,), A=(self.nnzA,))

    def adjoint(self, vx, vy=None, matrices=("Q", "A"), reduce=False, _staging_bytes=None):
        """lcqp_hip_sparse_adjoint: the gradients of a loss that reads the x AND the y the last run / resolve returned (synchronous; DESIGN.md
        section 3a'''').  vx = dl/dx [B][nV]; vy = dl/dy [B][m] in the layout of solution()'s y (rows A, L, R), or None for zero.  Returns a dict:
        dg, db, side, info as sensitivity(vx) returns them, and under "Q" / "A" the gradients on the stored entries of Q and of the stacked
        [A; L; R], in the order of load's Qx / Ax -- [B][nnz], or [nnz] summed over the batch on the device with reduce=True (one value array
        shared by the instances).  "Q" holds the symmetric derivative: entries (i, j) and (j, i) are equal.  reduce=False goes in chunks of
        instances under the staging cap (_staging_bytes: another cap for this one call, for tests).  The call changes nothing on the device."""
        return self._adjoint_host(vx, vy, matrices, reduce, _staging_bytes)

    def load(self, first, count, Qx, g, Ax, lbA=None, ubA=None, lbL=None, ubL=None, lbR=None, ubR=None, x0=None, y0=None):
        vec = self._vector_sizes()
        a = self._host_args((("Qx", self.nnzQ), vec[0], ("Ax", self.nnzA), *vec[1:]), count, (Qx, g, Ax, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0))
        return lib().lcqp_hip_sparse_load(self.h, first, count, *[_p(v) for v in a])

    def update(self, first, count, g, lbA=None, ubA=None, lbL=None, ubL=None, lbR=None, ubR=None, x0=None, y0=None):
        """lcqp_hip_sparse_update: new vectors for instances [first, first + count), the matrices stay (the argument list of load without
        Qx and Ax).  Returns the ReturnValue code like load (0; 100 for a range outside the batch, 116 for g = None, 120 for -inf in
        lbL / lbR); a wrongly sized array raises ValueError."""
        a = self._host_args(self._vector_sizes(), max(count, 0), (g, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0))
        return lib().lcqp_hip_sparse_update(self.h, first, count, *[_p(v) for v in a])

    def update_values(self, first, count, Qx=None, Ax=None):
        """lcqp_hip_sparse_update_values: new values of the matrices for instances [first, first + count) on the pattern of the handle,
        Qx [count][nnzQ] and Ax [count][nnzA] as load takes them, None: the array stays; the vectors, the stored point, the statuses and
        the penalties stay.  The next resolve(warm=True) sets up again on the new values and starts every instance whose last run
        succeeded from its last solution and working set, without its polish factor; resolve() and run() solve the new data cold.
        Returns the ReturnValue code (0; 100 INVALID_ARGUMENT without any array, 300 for an instance that holds no problem); a wrongly
        sized array raises ValueError."""
        if first < 0 or count <= 0 or first + count > self.B:
            raise ValueError(f"instances [{first}, {first + count}) outside the batch of {self.B}")
        a = self._host_args((("Qx", self.nnzQ), ("Ax", self.nnzA)), count, (Qx, Ax))
        return lib().lcqp_hip_sparse_update_values(self.h, first, count, *[_p(v) for v in a])

    # ---- the device-pointer entry points (DESIGN.md section 3a''''', "The sparse arm"): torch tensors on the handle's device in, torch tensors
    # out; the work is ordered behind torch.cuda.current_stream(), and what the caller enqueues there next sees the results.
    def load_device(self, first, count, Qx, g, Ax, lbA=None, ubA=None, lbL=None, ubL=None, lbR=None, ubR=None, x0=None, y0=None):
        """lcqp_hip_sparse_load_device: load() from float64 torch tensors on the handle's device, packed into the pools by kernels.  A
        value tensor of shape [nnz] is ONE array for all `count` instances (broadcast by the pack kernel), one of shape [count][nnz]
        holds one per instance; one that is None stays as the batch holds it (every instance of the range must hold a problem then).
        Returns the ReturnValue code like load; the pools hold the bytes load leaves."""
        self._range(first, count)
        shared, ptr = self._device_matrices(count, (("Qx", Qx, (self.nnzQ,)), ("Ax", Ax, (self.nnzA,))))
        v = self._device_vectors(count, (g, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0))
        return lib().lcqp_hip_sparse_load_device(self.h, first, count, shared, ptr["Qx"], v[0], ptr["Ax"], *v[1:], self._stream())

    def update_device(self, first, count, g, lbA=None, ubA=None, lbL=None, ubL=None, lbR=None, ubR=None, x0=None, y0=None):
        """lcqp_hip_sparse_update_device: update() from float64 torch tensors on the handle's device; the call does not drain the handle's
        stream, it is ordered behind it.  Returns the ReturnValue code."""
        self._range(first, count)
        v = self._device_vectors(count, (g, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0))
        return lib().lcqp_hip_sparse_update_device(self.h, first, count, *v, self._stream())

    def update_values_device(self, first, count, Qx=None, Ax=None, shared=0):
        """lcqp_hip_sparse_update_values_device: update_values() from float64 torch tensors on the handle's device.  As in load_device a
        value tensor of shape [nnz] is ONE array for all `count` instances; shared (bits 1, 2 for Qx, Ax) may say so too, and must then
        agree with the shapes.  Returns the ReturnValue code."""
        self._range(first, count)
        found, ptr = self._device_matrices(count, (("Qx", Qx, (self.nnzQ,)), ("Ax", Ax, (self.nnzA,))))
        if count > 1 and shared & ~found:
            raise ValueError(f"shared = {shared}: a value array marked as shared has the shape of one per instance")
        return lib().lcqp_hip_sparse_update_values_device(self.h, first, count, found, ptr["Qx"], ptr["Ax"], self._stream())

    def sensitivity_device(self, v):
        """lcqp_hip_sparse_sensitivity_device: sensitivity(v) with v a float64 tensor on the handle's device, [B][nV] or [B][k][nV], read
        where it lies; returns (dg, db, side, info) as tensors on that device (side, info: int32)."""
        return self._sensitivity_device(v)

    def sensitivity_blocked_device(self, V):
        """lcqp_hip_sparse_sensitivity_blocked_device: sensitivity_blocked(V) with V a float64 tensor on the handle's device, [B][k][nV], read
        where it lies; returns (dg [B][k][nV], db [B][k][m], side, info) as tensors on that device with the bits of the host call.  The
        panel kernel's staging goes to the tensors through k_sparse_scatter_panels on the device; adjoint_blocked_device, jacobian_device
        and jacobian_duals_device (_Batch) are the twins of the other three panel calls (DESIGN.md section 3a''''', "The sparse arm: panels
        and Jacobians into device arrays")."""
        import torch
        if not isinstance(V, torch.Tensor):
            raise ValueError(f"V: expected a torch tensor on the device of the batch, got {type(V).__name__}")
        if V.dim() != 3 or V.shape[1] < 1:
            raise ValueError(f"V: expected [{self.B}][k][{self.nV}] with k >= 1, got shape {tuple(V.shape)}")
        k = V.shape[1]
        pv = self._dev("V", V, ((self.B, k, self.nV),))
        dg, db, side, info = self._results((self.B, k))
        self._call("sensitivity_blocked_device", k, pv, dg.data_ptr(), db.data_ptr(), side.data_ptr(), info.data_ptr(), self._stream())
        return dg, db, side, info

    def adjoint_device(self, vx, vy=None, matrices=("Q", "A"), reduce=False, out=None):
        """lcqp_hip_sparse_adjoint_device: adjoint(vx, vy, matrices, reduce) with float64 tensors on the handle's device in and out -- the
        gradients on the non-zeros are written by ONE launch straight into their tensors, whatever their size (no staging, no chunks).
        out: tensors to write them into, by name ("Q": 16-byte aligned; default: fresh ones).  Returns the dict of adjoint, of tensors."""
        return self._adjoint_device(vx, vy, matrices, reduce, out)

    def read_problem(self, b):
        """Test and diagnostic entry point (lcqp_hip_sparse_read_problem): instance b as the pools hold it -- Qx [nnzQ], Ax [nnzA] in the
        order of load, g, x0 [nV], lE, uE [m] (the stacked row bounds), lbL, lbR [nComp], y0 [m], hasY0 (int)."""
        n, m, nK = self.nV, self.m, self.nComp
        d = dict(Qx=np.zeros(self.nnzQ), Ax=np.zeros(self.nnzA), g=np.zeros(n), lE=np.zeros(m), uE=np.zeros(m), lbL=np.zeros(nK), lbR=np.zeros(nK),
                 x0=np.zeros(n), y0=np.zeros(m))
        has = C.c_int(0)
        self._call("read_problem", int(b), *[_p(d[k]) for k in ("Qx", "Ax", "g", "lE", "uE", "lbL", "lbR", "x0", "y0")], C.byref(has))
        d["hasY0"] = has.value
        return d

    def read_admm(self, b):
        """Test and diagnostic entry point (lcqp_hip_sparse_read_admm; after a run / resolve; launches nothing): the state of the ADMM rounds
        of instance b as it lies on the device -- sigma, rho (= admmRho scale), scale; rhov, l, u, ya, za [m] in the row order of
        [A; L; R]; xa [nV].  The polish writes none of xa, ya, za: they are those of the last QP that ran ADMM iterations."""
        n, m = self.nV, self.m
        dims = np.zeros(2, dtype=np.int32); scal = np.zeros(3)
        d = dict(rhov=np.zeros(m), l=np.zeros(m), u=np.zeros(m), xa=np.zeros(n), ya=np.zeros(m), za=np.zeros(m))
        self._call("read_admm", int(b), _ip(dims), _p(scal), *[_p(d[k]) for k in ("rhov", "l", "u", "xa", "ya", "za")])
        d.update(n=int(dims[0]), m=int(dims[1]), sigma=float(scal[0]), rho=float(scal[1]), scale=float(scal[2]))
        return d

    POLISH_DIMS = ("n", "m", "trial", "reuse", "fact_valid", "nrefine", "round", "rc", "stfValid", "bigReg", "haveSolution", "lightOK", "kb", "general", "G")
    POLISH_SCALARS = ("gs", "ytol", "dpUsed", "d2Used", "xinf", "delta", "deltaS", "delta2", "delta2S", "e1max", "scale")
    POLISH_V = ("xt", "r1", "qx", "gk", "xq")
    POLISH_M = ("yt", "ex", "l", "u", "yq")
    POLISH_I = ("st", "stt", "stf", "new")

    def read_polish(self, b):
        """Test and diagnostic entry point (lcqp_hip_sparse_read_polish; after a run / resolve; launches nothing): the state of the
        active-set polish of instance b as it lies on the device, under the kernel's names -- the integers of POLISH_DIMS, the doubles of
        POLISH_SCALARS, xt, r1, qx (NV_TMP), gk, xq [nV], yt, ex, l, u, yq [m] in the row order of [A; L; R], and the row states st, stt,
        stf, new [m] (0 inactive, 1 lower, 2 upper, 3 equality)."""
        n, m = self.nV, self.m
        dims = np.zeros(len(self.POLISH_DIMS), dtype=np.int32); scal = np.zeros(len(self.POLISH_SCALARS))
        V = np.zeros((len(self.POLISH_V), n)); M = np.zeros((len(self.POLISH_M), m)); I = np.zeros((len(self.POLISH_I), m), dtype=np.int32)
        self._call("read_polish", int(b), _ip(dims), _p(scal), _p(V), _p(M), _ip(I))
        d = {k: int(v) for k, v in zip(self.POLISH_DIMS, dims)}
        d.update({k: float(v) for k, v in zip(self.POLISH_SCALARS, scal)})
        for names, arr in ((self.POLISH_V, V), (self.POLISH_M, M), (self.POLISH_I, I)):
            d.update({k: arr[i].copy() for i, k in enumerate(names)})
        return d

    PRODUCT_INPUTS_N = ("x", "q0", "q1", "base", "g", "xr", "c0", "c1")
    PRODUCT_INPUTS_M = ("y", "yr", "lx0", "lx1")
    PRODUCT_OUTPUTS_N = ("Qx0", "Qx1", "ETy", "r1", "Qxr", "Cx0", "Cx1", "CE0", "CE1", "CE", "CEzero")

    def product_probe(self, vn, vm, wide=False):
        """Test and diagnostic entry point (lcqp_hip_sparse_product_probe; needs only a loaded batch): the sparse products of the solver
        applied to the caller's vectors.  vn [B][8][nV] in the order of PRODUCT_INPUTS_N, vm [B][4][m] in the order of PRODUCT_INPUTS_M.
        Returns a dict: one [B][nV] array per name of PRODUCT_OUTPUTS_N (Q x0, Q x1 | base - E'y | r1 = -g - Q xr - E'yr, Q xr | C c0, C c1 |
        the swapped column gathers of lx0, lx1 | that of lx0 alone and its second sum), Ex [B][m], ETy_max, r1_max, r1_scale [B], and ell =
        (W, tails) of the row slab of Q, the row slab of E and the column slab of E.  wide: a wavefront per instance instead of lanes()."""
        B, n, m = self.B, self.nV, self.m
        vn = _sized("vn", _arr(vn), B * 8 * n); vm = _sized("vm", _arr(vm), B * 4 * m)
        on = np.zeros((B, 11, n)); om = np.zeros((B, m)); os_ = np.zeros((B, 3)); ell = np.zeros(6, dtype=np.int32)
        self._call("product_probe", 1 if wide else 0, _p(vn), _p(vm), _p(on), _p(om), _p(os_), _ip(ell))
        r = {k: on[:, i] for i, k in enumerate(self.PRODUCT_OUTPUTS_N)}
        r.update(Ex=om, ETy_max=os_[:, 0], r1_max=os_[:, 1], r1_scale=os_[:, 2], ell=dict(Q=(int(ell[0]), int(ell[1])), E=(int(ell[2]), int(ell[3])), T=(int(ell[4]), int(ell[5]))))
        return r
