"""tests/sparse_products_ref.py without a device: the patterns reach the branches of g_ell they are built for (slab widths and tail flags from
their own row and column counts), and a float64 numpy evaluation of the same sums stays inside the bounds tests/test_gpu_sparse_products.py
holds the device to, on every input used there."""
import numpy as np
import pytest

import sparse_products_ref as R

# (P2: the synthetic Hessian has at most four entries per row, so only the two slabs of E take the wide form there)
WANT = {"P1": dict(Q=(4, 0), E=(4, 0), T=(4, 0)), "P2": dict(Q=(4, 0), E=(8, 0), T=(8, 0)), "P3": dict(Q=(8, 1), E=(8, 1), T=(8, 1))}


@pytest.mark.parametrize("name", list(R.PATTERNS))
def test_patterns_reach_their_branches(name):
    inst = R.PATTERNS[name]()
    d = inst[0]
    assert R.slabs(d) == WANT[name]
    n, m = d["nV"], d["Ed"].shape[0]
    assert 64 <= n <= 200
    if name == "P1":
        assert n % 32 and m % 32      # the last tile of 4 x 8 rows is ragged
    if name == "P3":
        Em = d["Ed"] != 0
        assert Em.sum(axis=1).max() > 8 and Em.sum(axis=0).max() > 8 and (d["Qd"] != 0).sum(axis=1).max() > 8 and (Em.sum(axis=0) == 0).any()
    for a, b in zip(inst, inst[1:]):
        assert not np.array_equal(a["Ed"], b["Ed"])


@pytest.mark.parametrize("name", list(R.PATTERNS))
def test_float64_stays_inside_the_bounds(name):
    inst = R.PATTERNS[name]()
    worst = 0.0
    for seed in (1, 2):
        vn, vm = R.inputs(inst, seed)
        for b, d in enumerate(inst):
            r = R.ratios(R.evaluate(d, vn[b], vm[b], np.float64), d, vn[b], vm[b])
            worst = max(worst, max(r.values()))
            assert max(r.values()) <= 1.0, (name, b, r)
    print(f"    {name}: float64 numpy against long double: worst error / bound = {worst:.3e}")
