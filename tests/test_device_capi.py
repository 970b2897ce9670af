"""The device-pointer entry points of the dense batch (lcqp_hip_batch_*_device, DESIGN.md section 3a''''') as far as a machine without a
GPU can hold them: the symbols, the NULL-handle code, and the argument checks the Python wrappers make before any call."""
import numpy as np
import pytest

LCQPOBJECT_NOT_SETUP = 300
NAMES = ("load_device", "update_device", "get_solution_device", "sensitivity_device", "adjoint_device")


@pytest.fixture(scope="module")
def L():
    import lcqpow_amd
    return lcqpow_amd.lib()


def test_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, "lcqp_hip_batch_" + name), name


def test_null_handle_is_not_setup(L):
    n = [None]
    assert L.lcqp_hip_batch_load_device(None, 0, 1, 0, *n * 15, None) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_batch_update_device(None, 0, 1, *n * 11, None) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_batch_get_solution_device(None, None, None, None, None) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_batch_sensitivity_device(None, 0, 1, *n * 6) == LCQPOBJECT_NOT_SETUP
    assert L.lcqp_hip_batch_adjoint_device(None, *n * 6, 0, *n * 5) == LCQPOBJECT_NOT_SETUP


def shell(B=2, nV=4, nC=3, nComp=1):
    """a BatchLCQP without a handle: the wrappers must refuse their arguments before they would use one"""
    import lcqpow_amd
    bt = object.__new__(lcqpow_amd.BatchLCQP)
    bt.B, bt.nV, bt.nC, bt.nComp, bt.device, bt.h = B, nV, nC, nComp, 0, None
    bt.nd = bt._ndual = nV + nC + 2 * nComp
    return bt


def test_wrappers_refuse_what_is_not_a_device_tensor():
    import torch
    bt = shell()
    B, n, nC, nK, nd = bt.B, bt.nV, bt.nC, bt.nComp, bt.nd
    Q, g, Lm = np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, nK, n))
    with pytest.raises(ValueError, match="torch tensor"):
        bt.load_device(0, B, Q, g, Lm, Lm)
    with pytest.raises(ValueError, match="torch tensor"):
        bt.load_device(0, B, None, g, None, None)
    with pytest.raises(ValueError, match="torch tensor"):
        bt.update_device(0, B, g.tolist())
    with pytest.raises(ValueError, match="torch tensor"):
        bt.sensitivity_device(g)
    with pytest.raises(ValueError, match="torch tensor"):
        bt.adjoint_device(g)
    # tensors, but not on the device of the batch / not float64 / not contiguous / wrongly shaped
    with pytest.raises(ValueError, match="cuda:0"):
        bt.update_device(0, B, torch.zeros((B, n), dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        bt.update_device(0, B, torch.zeros((B, n), dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        bt.sensitivity_device(torch.zeros((n, B), dtype=torch.float64).T)
    with pytest.raises(ValueError, match="outside the batch"):
        bt.update_device(1, B, torch.zeros((B, n), dtype=torch.float64))
    with pytest.raises(ValueError, match="unknown names"):
        bt.adjoint_device(torch.zeros((B, n), dtype=torch.float64), matrices=("Q", "E"))


def test_torch_twin_of_split_bound_derivatives():
    import torch
    from lcqpow_amd import capi
    rng = np.random.default_rng(5)
    B, k, nV, nC, nComp = 3, 2, 4, 3, 2
    nd = nV + nC + 2 * nComp
    side = rng.integers(-1, 3, (B, nd)).astype(np.int32)
    for db in (rng.standard_normal((B, nd)), rng.standard_normal((B, k, nd))):
        want = capi.split_bound_derivatives(db, side, nV, nC, nComp)
        got = capi.split_bound_derivatives_torch(torch.as_tensor(db), torch.as_tensor(side), nV, nC, nComp)
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(got[key].numpy(), want[key]) and not np.any(np.signbit(got[key].numpy()) != np.signbit(want[key])), key
