"""The references of tests/sparse_kkt_ref.py held to their own bound on the CPU, in float64, in the orderings tests/oracle_py.py computes with
scipy (kkt_ordering for the band and bordered families, kkt_ordering_general for the others): every input family with exactly the instances,
regularisation pairs and working sets tests/test_gpu_sparse_factor.py factorises (sparse_kkt_ref.plan).  Shows that the inputs make the bound
|b - K x| <= (6 N + 8) eps (Wm |x| + |b|) neither unattainable (a float64 LDL' and the block elimination stay inside it) nor vacuous
(max(Wm |x|) / max(|K| |x|) stays under 1e6)."""
import numpy as np
import pytest

import sparse_kkt_ref as R


def _ordering(oracle, d, general):
    Qr, Er = d["Q"].tocsr(), d["E"].tocsr()
    Qr.sort_indices(); Er.sort_indices()
    if general:
        return np.asarray(oracle.kkt_ordering_general(d["nV"], Qr.indptr, Qr.indices, Er.indptr, Er.indices)), 0
    perm, w, kb = oracle.kkt_ordering(d["nV"], Qr.indptr, Qr.indices, Er.indptr, Er.indices, rows_follow=oracle.hessian_is_definite_by_diagonal(Qr))
    return np.asarray(perm), kb


@pytest.mark.parametrize("name", list(R.FAMILIES))
def test_references_stay_within_their_own_bound(oracle, name):
    fam = R.FAMILIES[name]
    inst = fam["make"](fam["B"])
    opt = oracle.default_options()
    worst, worst_g, worst_b = 0.0, 0.0, 0.0
    orders = [_ordering(oracle, d, fam["general"]) for d in inst[:1]] * len(inst)      # one pattern: one ordering
    for rname, per in R.plan(name, inst):
        for b, (d, (sname, use)) in enumerate(zip(inst, per)):
            perm, kb = orders[b]
            N = len(perm); m = d["E"].shape[0]
            dprim, ddual = R.regularisations(opt, R.scale_of(d), m)[rname]
            B = R.rhs_set(N, 7 + b, unit=False)[perm]
            K = R.kkt_dense(d, dprim, ddual, use)[np.ix_(perm, perm)]
            L, D, Wm = R.ldl_nopivot(K, np.float64)
            X = R.ldl_solve(L, D, B)
            res, bound = R.residual_and_bound(K, Wm, X, B)
            ratio = float((res / bound).max()); gr = float(R.growth(K, Wm, X).max())
            worst, worst_g = max(worst, ratio), max(worst_g, gr)
            assert ratio <= 1.0, (name, b, sname, rname, ratio)
            assert gr < R.GROWTH_CAP, (name, b, sname, rname, gr)
            if kb:
                res, bound = R.residual_and_bound(K, Wm, R.bordered_ref(K, kb, B), B)
                rb = float((res / bound).max())
                worst_b = max(worst_b, rb)
                assert rb <= 1.0, (name, b, sname, rname, rb)
    print(f"    {name}: worst error / bound = {worst:.3e} (block elimination {worst_b:.3e}), worst growth = {worst_g:.3e}")
