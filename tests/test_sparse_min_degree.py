"""CPU checks of the minimum-degree ordering of the general sparse LDL' and of the choice between it and nested dissection
(lcqpow_amd/csrc/lcqp_sparse_general.hpp: md_front_tree, build_symbolic, symbolic_violation; lcqp_sparse_pattern.hpp: order_kkt), run by
tests/cpp/min_degree_test.cpp on the block-arrow patterns of tests/block_arrow.py and on the patterns the existing tests run on the general
engine.  The sizes the analysis achieves are printed (DESIGN.md section 3c holds them)."""
import os
import subprocess

import numpy as np
import pytest

import block_arrow as BA
import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, MD = 1, 2
SIZES = ("N", "nF", "maxFront", "Lsize", "flops", "nnzL", "stackSize", "nd_nF", "nd_maxFront", "nd_Lsize", "nd_flops")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("md") / "min_degree_test")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-o", out, os.path.join(ROOT, "tests", "cpp", "min_degree_test.cpp")])
    return out


def analyse(exe, tmp_path, d, *args, general=0):
    """what the driver prints as a dict (integers where they are integers); {"error": message} for a refused pattern"""
    path = str(tmp_path / "case.txt")
    BA.write_case(path, d, general=general)
    r = subprocess.run([exe, path] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, _, val = line.partition(" ")
        if key in ("error", "violation", "note"):
            out[key] = val
        elif key in ("bound_ratio", "growth"):
            out[key] = float(val)
        elif val:
            out[key] = int(val)
    print(args, {k: out[k] for k in SIZES if k in out}, {k: out[k] for k in ("bound_ratio", "growth") if k in out})
    return out


def valid(r):
    """the Symbolic holds what the kernels take for granted (symbolic_violation: perm a permutation, pivots contiguous, fronts in postorder,
    boundary rows ascending behind the pivots, rel the same row of the parent, the update blocks a stack whose top is a front's children,
    assembly positions inside the panel and distinct), no entry of an explicit elimination lies outside the fronts, a second analysis gives
    the same arrays, and the scalar restatement of the device's loops solves a quasi-definite K in it to the componentwise bound, whose
    |L| |D| |L'| comes from the driver's own long-double reference factor in the same ordering"""
    assert r["violation"] == "none", r["violation"]
    assert r["fill_lost"] == 0 and r["fill_entries"] > 0
    assert r["deterministic"] == 1
    assert r["bound_ratio"] <= 1.0, r["bound_ratio"]


@pytest.mark.parametrize("shape,nd_fronts", [((400, 6, 32), 1462), ((512, 8, 64), None)])
def test_refused_patterns_run_on_minimum_degree(exe, tmp_path, shape, nd_fronts):
    """nested dissection needs a front of more than 576 rows on these two (refused until now): minimum degree runs them with fronts of at most
    64 rows, a valid Symbolic, at most 64 N factor entries and no more fronts than nested dissection makes"""
    d = BA.block_arrow(*shape)
    r = analyse(exe, tmp_path, d, "fill", "numeric")
    assert "error" not in r, r
    assert r["general"] == 1 and r["ordering"] == MD and r["maxFront"] <= 64
    assert r["nd_maxFront"] > 576
    valid(r)
    assert r["Lsize"] <= 64 * r["N"]
    assert r["nF"] <= r["nd_nF"] and (nd_fronts is None or r["nd_nF"] == nd_fronts)
    assert "error" in analyse(exe, tmp_path, d, "nd")      # the hook: nested dissection alone is refused as before
    assert "largest front" in analyse(exe, tmp_path, d, "nd")["error"]


def test_class_rule_switches_256_8_32(exe, tmp_path):
    """nested dissection is accepted here with a 410-row front (the class of up to 576 rows); minimum degree stays within 64 rows with fewer
    flops and fewer fronts: chosen by the class rule, and the hook `nd` gives today's analysis"""
    d = BA.block_arrow(256, 8, 32)
    r = analyse(exe, tmp_path, d, "fill", "numeric")
    assert r["general"] == 1 and r["ordering"] == MD and r["maxFront"] <= 64 and r["flops"] < r["nd_flops"]
    valid(r)
    assert r["Lsize"] <= 64 * r["N"] and r["nF"] <= r["nd_nF"] == 850
    n = analyse(exe, tmp_path, d, "nd", "fill", "numeric")
    assert n["ordering"] == ND and n["maxFront"] == 410 and n["nF"] == 850 and n["same_as_analyze"] == 1
    valid(n)


@pytest.mark.parametrize("shape,kb", [((64, 16, 32), 16), ((96, 8, 24), 11)])
def test_bordered_bands_stay(exe, tmp_path, shape, kb):
    """a border of at most 16 nodes: the bordered band as before, whatever the ordering hook says"""
    d = BA.block_arrow(*shape)
    for hook in ("auto", "nd", "md"):
        r = analyse(exe, tmp_path, d, hook)
        assert r["general"] == 0 and r["ordering"] == 0 and r["kb"] == kb and r["w"] <= 63


def _synthetic(n, nC, nK):
    Q, E = P.sparse_pattern(n, nC, nK)
    return dict(nV=n, nC=nC, nComp=nK, Q=Q, E=E)


def _grid_bench():
    import scipy.sparse as sp
    from lcqpow_amd import synth_sparse as S
    Q, E, _, _, info = S.grid_pattern_arrays(128, 800, 1200)
    mk = lambda pt: sp.csc_matrix((np.ones(pt.nnz), pt.indices, pt.indptr), shape=pt.shape)
    return dict(nV=info["n"], nC=info["nC"], nComp=info["nComp"], Q=mk(Q), E=mk(E))


def _coupled():
    from test_gpu_sparse_general_panel import coupled_lcqp
    return coupled_lcqp()


def _dense_rows(n, nC, nK):
    import scipy.sparse as sp
    L = np.zeros((nK, n)); R = np.zeros((nK, n))
    L[np.arange(nK), np.arange(nK)] = 1; R[np.arange(nK), nK + np.arange(nK)] = 1
    return dict(nV=n, nC=nC, nComp=nK, Q=sp.identity(n, format="csc"), E=sp.csc_matrix(np.vstack([np.ones((nC, n)), L, R])))


KEPT = {
    "forced general (64, 32, 8)": (lambda: _synthetic(64, 32, 8), 1),
    "grid 44": (lambda: P.grid_lcqp(44, 300, 200), 0),
    "coupled": (_coupled, 0),
    "grid_128 of bench.py": (_grid_bench, 0),
    "grid 128 of test_python_api.py": (lambda: P.grid_lcqp(128, 1200, 800), 0),      # 16 384 variables, N = 19 584
    "grid 128 with fewer rows": (lambda: P.grid_lcqp(128, 300, 200), 0),
    "forty dense rows": (lambda: _dense_rows(200, 40, 8), 0),
}


@pytest.mark.parametrize("name", sorted(KEPT))
def test_nested_dissection_kept(exe, tmp_path, name):
    """the patterns the existing tests and the benchmark run on the general engine keep nested dissection: the arrays of the analysis equal
    those of a direct call of analyze(...)"""
    make, general = KEPT[name]
    r = analyse(exe, tmp_path, make(), general=general)
    assert r["general"] == 1 and r["ordering"] == ND and r["same_as_analyze"] == 1 and r["deterministic"] == 1
    assert r["violation"] == "none", r["violation"]


def test_sixty_dense_rows_stay_refused(exe, tmp_path):
    """sixty dense rows over seven hundred variables: minimum degree would run them as seven hundred one-variable fronts under all sixty rows,
    nine times the fronts of nested dissection -- not taken (the front-count condition of order_kkt); the pattern is refused with the message it
    always had and runs on the dense kernels"""
    r = analyse(exe, tmp_path, _dense_rows(700, 60, 8))
    assert r["error"].startswith("general sparse LDL' of this pattern: largest front 701 (limit 576)") and "too dense for the sparse engine" in r["error"]
    # lcqp_hip_sparse_create appends the note: the user learns that a minimum-degree ordering fits and why it is not taken
    assert "minimum-degree ordering fits (largest front 64) but needs 699 fronts against 78" in r["note"] and "LCQP_SPARSE_ORDERING=md" in r["note"]
    m = analyse(exe, tmp_path, _dense_rows(700, 60, 8), "md")
    assert m["ordering"] == MD and m["nF"] > m["nd_nF"] and m["violation"] == "none"


def test_forced_minimum_degree_on_small_general(exe, tmp_path):
    """the hook `md` on the forced-general (64, 32, 8): many tiny fronts, a small N -- a valid Symbolic that solves to the bound"""
    r = analyse(exe, tmp_path, _synthetic(64, 32, 8), "md", "fill", "numeric", general=1)
    assert r["general"] == 1 and r["ordering"] == MD
    valid(r)
    assert analyse(exe, tmp_path, _synthetic(64, 32, 8), "md")["general"] == 0      # the hook sends no band pattern to the general engine


def test_symbols_and_binding():
    """the entry point is declared in include/lcqp_hip.h, exported by the built library and bound in Python; a NULL handle -- the only one
    there is without a device -- answers -1"""
    import ctypes
    import lcqpow_amd
    from test_capi_symbols import declared_functions
    L = ctypes.CDLL(lcqpow_amd.library_path())
    for sym in ("lcqp_hip_sparse_general_ordering",):
        assert sym in declared_functions(), sym
        assert hasattr(L, sym), sym
    assert callable(lcqpow_amd.SparseBatchLCQP.general_ordering)
    assert lcqpow_amd.lib().lcqp_hip_sparse_general_ordering(None) == -1


def test_oracle_solves_every_instance(oracle):
    """the sparse oracle alone returns 0 on every block-arrow instance the GPU tests use (tests/test_gpu_sparse_min_degree.py leaves none out)"""
    for shape, B in (((400, 6, 32), 3), ((256, 8, 32), 2)):
        perm = BA.arrow_ordering(*shape)
        for k in range(B):
            assert BA.oracle_solve(oracle, BA.block_arrow(*shape, inst=k), perm)["ret"] == 0, (shape, k)
