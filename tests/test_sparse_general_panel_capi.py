"""The switch of the general sparse LDL's panel form in the C ABI (lcqp_hip_sparse_set_general_panel, lcqp_hip_sparse_max_front; DESIGN.md
section 3a''', "The general engine"): declared in include/lcqp_hip.h, exported by the built library, bound in Python, and the argument
checks that need no device."""
import ctypes

from test_capi_symbols import declared_functions

NEW = ("lcqp_hip_sparse_set_general_panel", "lcqp_hip_sparse_max_front")


def test_the_new_calls_are_declared_and_exported():
    import lcqpow_amd
    L = ctypes.CDLL(lcqpow_amd.library_path())
    names = declared_functions()
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n


def test_the_binding_has_them():
    import lcqpow_amd as la
    assert callable(la.SparseBatchLCQP.set_general_panel) and callable(la.SparseBatchLCQP.max_front)


def test_argument_checks_without_a_gpu():
    """a NULL handle -- the only one there is without a device: INVALID_ARGUMENT from the switch whatever `on`, -1 from max_front, and
    sens_panel's 0 as before"""
    import lcqpow_amd as la
    L = la.lib()
    for on in (0, 1, 2, -1):
        assert L.lcqp_hip_sparse_set_general_panel(None, on) == 100
    assert L.lcqp_hip_sparse_max_front(None) == -1
    assert L.lcqp_hip_sparse_sens_panel(None) == 0
