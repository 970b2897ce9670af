"""The device-pointer entry points of the sparse batch (lcqp_hip_sparse_*_device, lcqp_hip_sparse_read_problem; DESIGN.md section 3a''''') as
far as a machine without a GPU can hold them: the symbols, the NULL-handle codes, and the argument checks the Python wrappers make before
any call."""
import numpy as np
import pytest

INVALID_ARGUMENT = 100
LCQPOBJECT_NOT_SETUP = 300
NAMES = ("load_device", "update_device", "get_solution_device", "sensitivity_device", "adjoint_device", "read_problem")


@pytest.fixture(scope="module")
def L():
    import lcqpow_amd
    return lcqpow_amd.lib()


def test_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, "lcqp_hip_sparse_" + name), name


def test_null_handle(L):
    n = [None]
    assert L.lcqp_hip_sparse_load_device(None, 0, 1, 0, *n * 11, None) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_update_device(None, 0, 1, *n * 9, None) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_get_solution_device(None, None, None, None, None) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_sensitivity_device(None, 1, *n * 6) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_adjoint_device(None, *n * 6, 0, *n * 3) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_sparse_read_problem(None, 0, *n * 10) == INVALID_ARGUMENT


def shell(B=2, nV=4, nC=3, nComp=1, nnzQ=6, nnzA=7):
    """a SparseBatchLCQP without a handle: the wrappers must refuse their arguments before they would use one"""
    import lcqpow_amd
    sb = object.__new__(lcqpow_amd.SparseBatchLCQP)
    sb.B, sb.nV, sb.nC, sb.nComp, sb.device, sb.h = B, nV, nC, nComp, 0, None
    sb.m = sb._ndual = nC + 2 * nComp
    sb.nnzQ, sb.nnzA = nnzQ, nnzA
    return sb


def test_wrappers_refuse_what_is_not_a_device_tensor():
    import torch
    sb = shell()
    B, n, m = sb.B, sb.nV, sb.m
    Qx, g, Ax = np.zeros((B, sb.nnzQ)), np.zeros((B, n)), np.zeros((B, sb.nnzA))
    with pytest.raises(ValueError, match="torch tensor"):
        sb.load_device(0, B, Qx, g, Ax)
    with pytest.raises(ValueError, match="torch tensor"):
        sb.load_device(0, B, None, g, None)
    with pytest.raises(ValueError, match="torch tensor"):
        sb.update_device(0, B, g.tolist())
    with pytest.raises(ValueError, match="torch tensor"):
        sb.sensitivity_device(g)
    with pytest.raises(ValueError, match="torch tensor"):
        sb.adjoint_device(g)
    # tensors, but not on the device of the batch / not float64 / not contiguous / wrongly shaped
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    with pytest.raises(ValueError, match="cuda:0"):
        sb.update_device(0, B, t(B, n))
    with pytest.raises(ValueError, match="cuda:0"):
        sb.load_device(0, B, t(sb.nnzQ), t(B, n), t(B, sb.nnzA))
    with pytest.raises(ValueError, match="float64"):
        sb.update_device(0, B, torch.zeros((B, n), dtype=torch.float32))
    with pytest.raises(ValueError, match="float64"):
        sb.adjoint_device(torch.zeros((B, n), dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        sb.sensitivity_device(t(n, B).T)
    with pytest.raises(ValueError, match="contiguous"):
        sb.load_device(0, B, t(sb.nnzQ, B).T, t(B, n), None)
    with pytest.raises(ValueError, match="outside the batch"):
        sb.update_device(1, B, t(B, n))
    with pytest.raises(ValueError, match="outside the batch"):
        sb.load_device(0, B + 1, None, t(B + 1, n), None)
    with pytest.raises(ValueError, match="no vectors"):      # a wrong shape
        sb.sensitivity_device(t(B, 0, n))
    with pytest.raises(ValueError, match="unknown names"):
        sb.adjoint_device(t(B, n), matrices=("Q", "L"))


def test_torch_twin_of_split_bound_derivatives_in_the_sparse_layout():
    import torch
    from lcqpow_amd import capi
    rng = np.random.default_rng(5)
    B, k, nV, nC, nComp = 3, 2, 4, 3, 2
    m = nC + 2 * nComp
    side = rng.integers(-1, 3, (B, m)).astype(np.int32)
    for db in (rng.standard_normal((B, m)), rng.standard_normal((B, k, m))):
        want = capi.split_bound_derivatives(db, side, nV, nC, nComp, sparse=True)
        got = capi.split_bound_derivatives_torch(torch.as_tensor(db), torch.as_tensor(side), nV, nC, nComp, sparse=True)
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(got[key].numpy(), want[key]) and not np.any(np.signbit(got[key].numpy()) != np.signbit(want[key])), key
