"""CPU checks of the sparse arm's pattern analysis (lcqpow_amd/csrc/lcqp_sparse_pattern.hpp: checks, CSR conversion, orderings, band maps,
border lists, ELL slabs), run by tests/cpp/sparse_pattern_test.cpp on the patterns the GPU tests use.  Each case is held to the orderings and
sizes recorded in tests/golden/sparse_pattern.json and to invariants that need no golden: perm is a permutation, every band entry sits where
its maps say and points back to its source, every entry at a border node is listed once, the ELL slabs reproduce the CSR rows."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_pattern.json")


def _synthetic(n, nC, nK, span=6):
    Q, E = P.sparse_pattern(n, nC, nK, span=span)
    return n, nC, nK, Q, E


def _coupling(extra, n=512, nC=256, nK=64):
    """tests/test_gpu_sparse.py::test_sparse_banded_pattern_with_coupling_rows: `extra` rows over every variable behind the rows of A"""
    import scipy.sparse as sp
    Q, E = P.sparse_pattern(n, nC, nK)
    E = E.tocsr()
    A2 = sp.vstack([E[:nC], sp.csr_matrix(np.ones((extra, n))), E[nC:]], format="csc")
    return n, nC + extra, nK, Q, A2


def _dense_rows(n, nC, nK):
    """nC dense rows over n variables, L_k = e_k, R_k = e_{nK + k}, diagonal Q (the dense-row tests of tests/test_gpu_sparse.py)"""
    import scipy.sparse as sp
    L = np.zeros((nK, n)); R = np.zeros((nK, n))
    L[np.arange(nK), np.arange(nK)] = 1; R[np.arange(nK), nK + np.arange(nK)] = 1
    return n, nC, nK, sp.identity(n, format="csc"), sp.csc_matrix(np.vstack([np.ones((nC, n)), L, R]))


def _circle():
    import scipy.sparse as sp
    d = P.circle(100)
    return d["nV"], d["nC"], d["nComp"], sp.csc_matrix(d["Q"]), sp.csc_matrix(np.vstack([d["A"], d["L"], d["R"]]))


def _grid(g, nK=300, nC=200):
    d = P.grid_lcqp(g, nK, nC)
    return d["nV"], d["nC"], d["nComp"], d["Q"], d["E"]


def _grid_bench():
    """bench.py's grid_128 object (lcqpow_amd/synth_sparse.py::grid_pattern_arrays)"""
    import scipy.sparse as sp
    from lcqpow_amd import synth_sparse as S
    Q, E, _, _, info = S.grid_pattern_arrays(128, 800, 1200)
    mk = lambda pt: sp.csc_matrix((np.ones(pt.nnz), pt.indices, pt.indptr), shape=pt.shape)
    return info["n"], info["nC"], info["nComp"], mk(Q), mk(E)


# name: (pattern, LCQP_SPARSE_GENERAL, LCQP_SPARSE_LANES)
CASES = {
    "banded_64": (lambda: _synthetic(64, 32, 8), 0, 0),
    "banded_512": (lambda: _synthetic(512, 256, 64), 0, 0),
    "banded_4096": (lambda: _synthetic(4096, 2048, 512), 0, 0),
    "banded_span10": (lambda: _synthetic(512, 256, 64, span=10), 0, 0),
    "banded_span18": (lambda: _synthetic(512, 256, 64, span=18), 0, 0),
    "circle_100": (_circle, 0, 0),
    "coupling_1": (lambda: _coupling(1), 0, 0),
    "coupling_3": (lambda: _coupling(3), 0, 0),
    "dense_rows": (lambda: _dense_rows(200, 40, 8), 0, 0),
    "grid_44": (lambda: _grid(44), 0, 0),
    "grid_64": (lambda: _grid(64), 0, 0),
    "grid_128": (_grid_bench, 0, 0),
    "too_dense": (lambda: _dense_rows(700, 60, 8), 0, 0),
    "banded_512_general_hook": (lambda: _synthetic(512, 256, 64), 1, 0),
    "banded_512_lanes_hook": (lambda: _synthetic(512, 256, 64), 0, 32),
}


def write_case(path, name):
    """the case as whitespace-separated integers: nV nC nComp general lanes, Qp, nnz(Q), Qi, Ap, nnz(A), Ai"""
    build, general, lanes = CASES[name]
    n, nC, nK, Q, E = build()
    Q, E = Q.tocsc(), E.tocsc()
    Q.sort_indices(); E.sort_indices()
    parts = [np.array([n, nC, nK, general, lanes]), Q.indptr, [Q.indptr[-1]], Q.indices, E.indptr, [E.indptr[-1]], E.indices]
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(int(v)) for v in p) for p in parts) + "\n")


def parse(out):
    """what the test driver prints -> {w, G, kb, general, nF, hasB, permA, rowsFollowA[, permB, rowsFollowB]} or {error}; perms of more than
    128 nodes as the sha256 of their int32 bytes"""
    r = {}
    for line in out.splitlines():
        key, _, val = line.partition(" ")
        if key == "error":
            return {"error": val}
        if key in ("permA", "permB"):
            p = np.array(val.split(), dtype=np.int32)
            r[key] = p.tolist() if len(p) <= 128 else hashlib.sha256(p.tobytes()).hexdigest()
        elif key in ("w", "G", "kb", "general", "nF", "hasB", "rowsFollowA", "rowsFollowB"):
            r[key] = int(val)
    return r


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pat") / "sparse_pattern_test")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-o", out, os.path.join(ROOT, "tests", "cpp", "sparse_pattern_test.cpp")])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_pattern_analysis(exe, tmp_path, name):
    """the analysis of every case gives the recorded orderings, widths and choices, and its maps, border lists and slabs hold together"""
    path = str(tmp_path / (name + ".txt"))
    write_case(path, name)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(GOLDEN) as f:
        assert parse(r.stdout) == json.load(f)[name]
    if "error" not in parse(r.stdout):
        assert "invariant failures 0" in r.stdout, r.stdout[-2000:]
