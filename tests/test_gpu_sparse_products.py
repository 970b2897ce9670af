"""The sparse products of the sparse arm (sp_Ex, sp_Qx2, sp_ETy, sp_residual, sp_Cx2, sp_C_from_Ex in lcqp_sparse_solver.hpp over g_ell /
sp_ell in lcqp_sparse_lane.hpp) through lcqp_hip_sparse_product_probe, which applies the routines themselves to the caller's vectors, held to
the long-double references of tests/sparse_products_ref.py under bounds that follow from the lengths of the sums (stated there; a float64
numpy evaluation stays inside them: tests/test_sparse_products_ref.py).

Which branch of g_ell a product takes is asserted, not assumed: every pattern's slab widths and tail flags are computed from its own row and
column counts (width 4 if no row is longer than 4, else 8; a tail beyond the width) and compared with what the handle reports.

  P1  tridiagonal Q, short rows and columns of E: width 4 on all three slabs, n = 70 and m = 36 leave ragged last tiles
  P2  the synthetic (64, 32, 8) pattern at span 6: width 8 on both slabs of E, no tails (its Hessian has four entries per row: Q is width 4)
  P3  coupling rows widened: tails on all three slabs (the column slab's through cmap), a variable in no row of E; at its natural lane
      width (32) and under LCQP_SPARSE_LANES = 16, 32, 64 (the band engine takes the pattern: the general LDL' is not needed)
Every pattern with B = 5 (the last wavefront partly filled), with the handle's lane group and with a wavefront per instance (the form the
streaming phases of a run use), and P1 also under LCQP_SPARSE_POOL=4.  A sweep of unit vectors holds the position maps bit for bit: each
output entry is then one stored value.  The returned maxima equal the maxima of the returned vectors bit for bit.
`python -m pytest tests/test_gpu_sparse_products.py -m gpu -s` prints the worst error / bound of every output.

Worst error / bound on an MI355X (18 tests, 1 s): Ex 0.16, Q x 0.24, base - E'y 0.26, r1 0.17, C v 0.08, C from E x 0.11, scale 0.05; the
same with the lane group and with a wavefront per instance, and under every forced lane width.  (P3 runs on lane groups of 32 at its
natural width.)  A float64 numpy evaluation: 0.26.
Mutants (the table is in tests/test_gpu_sparse_admm.py): the tail loop of g_ell starting one entry late fails the eight P3 cases of
test_products_against_the_reference and the unit-vector sweep of P3 (P1 and P2 have no tails); sp_Cx2 without the swap fails all fourteen
cases of test_products_against_the_reference on C v0 and C v1 alone.
"""
import functools

import numpy as np
import pytest

import sparse_products_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _inst(name):
    return R.PATTERNS[name]()


def _handle(hip, monkeypatch, inst, env=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    d0 = inst[0]
    # (the band engine takes all three patterns, P3 on lane groups of 32: no pattern needs LCQP_SPARSE_GENERAL)
    sb = hip.SparseBatchLCQP(len(inst), d0["nV"], d0["nC"], d0["nComp"], d0["Q"], d0["E"], opt=hip.default_options(perturbStep=0, printLevel=0))
    assert sb.fronts() == 0
    assert sb.load(0, len(inst), np.stack([d["Q"].data for d in inst]), np.stack([d["g"] for d in inst]), np.stack([d["E"].data for d in inst]),
                   lbA=np.stack([d["lbA"] for d in inst]), ubA=np.stack([d["ubA"] for d in inst])) == 0
    return sb


def check(name, sb, inst, wide, seed=1):
    vn, vm = R.inputs(inst, seed)
    out = sb.product_probe(vn, vm, wide=wide)
    assert out["ell"] == R.slabs(inst[0]), (name, out["ell"])
    worst = {}
    for b, d in enumerate(inst):
        got = {k: out[k][b] for k in R.OUTPUTS}
        got["r1_scale"] = out["r1_scale"][b]
        for k, v in R.ratios(got, d, vn[b], vm[b]).items():
            worst[k] = max(worst.get(k, 0.0), v)
        # fmax is exact: the maxima the routines return are those of the vectors they wrote
        assert out["ETy_max"][b] == np.abs(out["ETy"][b]).max() and out["r1_max"][b] == np.abs(out["r1"][b]).max(), (name, b)
        assert not out["CEzero"][b].any() and np.array_equal(out["CE"][b], out["CE0"][b])
    print(f"    {name} ({'wavefront' if wide else 'lanes %d' % sb.lanes()}): worst error / bound  " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (name, wide, bad)
    return out


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name,env", [("P1", None), ("P1", {"LCQP_SPARSE_POOL": "4"}), ("P2", None), ("P3", None), ("P3", {"LCQP_SPARSE_LANES": "16"}),
                                      ("P3", {"LCQP_SPARSE_LANES": "32"}), ("P3", {"LCQP_SPARSE_LANES": "64"})])
def test_products_against_the_reference(hip, monkeypatch, name, env, wide):
    inst = _inst(name)
    sb = _handle(hip, monkeypatch, inst, env)
    if env and "LCQP_SPARSE_LANES" in env:
        assert sb.lanes() >= int(env["LCQP_SPARSE_LANES"])
    check(name, sb, inst, wide)
    sb.close()


@pytest.mark.parametrize("name", list(R.PATTERNS))
def test_unit_vectors_return_stored_values(hip, monkeypatch, name):
    """instance b of call c gets the unit vectors of variable / row c B + b (modulo n / m): every slot of the three slabs and every tail
    entry is read for some instance, and each output is one stored value, exactly"""
    inst = _inst(name)
    sb = _handle(hip, monkeypatch, inst)
    B, n, m = len(inst), inst[0]["nV"], inst[0]["Ed"].shape[0]
    nC, nK = inst[0]["nC"], inst[0]["nComp"]
    for wide in (False, True):
        for c in range((max(n, m) + B - 1) // B):
            vn = np.zeros((B, 8, n)); vm = np.zeros((B, 4, m))
            js = [(c * B + b) % n for b in range(B)]; rs = [(c * B + b) % m for b in range(B)]
            for b in range(B):
                vn[b, 0, js[b]] = vn[b, 1, js[b]] = 1.0; vn[b, 2, (js[b] + 1) % n] = 1.0       # x, q0, q1
                vm[b, 0, rs[b]] = vm[b, 1, rs[b]] = 1.0                                          # y, yr
                vm[b, 2, nC + rs[b] % (2 * nK)] = 1.0; vm[b, 3, nC + (rs[b] + 1) % (2 * nK)] = 1.0
            out = sb.product_probe(vn, vm, wide=wide)
            for b, d in enumerate(inst):
                Q, E = d["Qd"], d["Ed"]
                sw = lambda r: r + nK if r < nC + nK else r - nK      # the row whose entries a unit lx at row r selects
                assert np.array_equal(out["Ex"][b], E[:, js[b]]), (name, wide, c, b)
                assert np.array_equal(out["Qx0"][b], Q[:, js[b]]) and np.array_equal(out["Qx1"][b], Q[:, (js[b] + 1) % n]), (name, wide, c, b)
                assert np.array_equal(out["ETy"][b], -E[rs[b]]) and np.array_equal(out["r1"][b], -E[rs[b]]) and not out["Qxr"][b].any(), (name, wide, c, b)
                assert np.array_equal(out["CE0"][b], E[sw(nC + rs[b] % (2 * nK))]) and np.array_equal(out["CE1"][b], E[sw(nC + (rs[b] + 1) % (2 * nK))]), (name, wide, c, b)
                assert out["ETy_max"][b] == np.abs(E[rs[b]]).max() == out["r1_max"][b] == out["r1_scale"][b]
    sb.close()


def test_probe_calls_leave_a_run_its_bits(hip, monkeypatch):
    """on the synthetic (64, 32, 8) batch: load, probe, run, probe, resolve = load, run, resolve, to the bit; and the probe's own outputs do
    not depend on what ran before it"""
    import sparse_kkt_ref as S
    inst = S.synthetic((64, 32, 8), 5)
    rng = np.random.default_rng(11)
    vn = rng.standard_normal((5, 8, 64)); vm = rng.standard_normal((5, 4, 48))
    runs, probes = [], []
    for probe in (False, True):
        d0 = inst[0]
        sb = hip.SparseBatchLCQP(5, 64, 32, 8, d0["Q"], d0["E"], opt=hip.default_options(perturbStep=0, printLevel=0))
        assert sb.load(0, 5, np.stack([d["Q"].data for d in inst]), np.stack([d["g"] for d in inst]), np.stack([d["E"].data for d in inst]),
                       lbA=np.stack([d["lbA"] for d in inst]), ubA=np.stack([d["ubA"] for d in inst])) == 0
        if probe:
            probes.append(sb.product_probe(vn, vm))
            probes.append(sb.product_probe(vn, vm, wide=True))
        sb.run()
        first = sb.solution()
        if probe:
            probes.append(sb.product_probe(vn, vm))
        sb.resolve(warm=True)
        second = sb.solution()
        runs.append((first, second))
        sb.close()
    for (xa, ya, sa), (xb, yb, sb_) in zip(runs[0], runs[1]):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and [s["iterTotal"] for s in sa] == [s["iterTotal"] for s in sb_]
    assert all(s["returnValue"] == 0 for s in runs[0][0][2])
    for k in R.OUTPUTS:
        assert np.array_equal(probes[0][k], probes[2][k]), k
