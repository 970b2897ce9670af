"""Blocked multi-vector sensitivities and Jacobians (lcqp_hip_batch_sensitivity_blocked / _jacobian and the QP twins; DESIGN.md section 3a''').

1  dg, db of the blocked kernel against numpy on the device's own working set (the reference and the bound of tests/test_gpu_sensitivity.py:
   max|delta| <= 1e-12 nV cond_2(K) |v|_inf), for nrhs in {1, 3, SENS_PANEL, SENS_PANEL + 1}; side / info equal the vector call's; on the
   fallback size the bits of the vector call.   2  the columns of a panel are independent, bit for bit.   3  blocked beside vector: twice the
   bound (both sit inside it around one reference).   4  the Jacobian.   5  the calls change nothing.   6  refusals.   7  the QP twin.   8  torch.

Problems: tests/problems.py::random_lcqp with default_rng(1000 + instance), perturbStep = 0.  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest

from batch_helpers import assert_same_bits, kkt_reference, load_all, result, stack, update_all
from problems import perturbed, random_lcqp

pytestmark = pytest.mark.gpu

PANEL = 16
#          n,  nC, nComp, B, box, shifted, equalities     path
SHAPES = {"np128": (40, 20, 8, 6, False, False, False),               # smallest size, n < one 64-block pair
          "np256": (200, 330, 37, 3, True, False, False),            # box rows through boxidx, more rows than variables
          "np384": (300, 100, 40, 2, False, False, False),           # odd block count
          "np512_big_T": (400, 300, 20, 2, False, False, True),      # ubA = lbA: n_T > 256
          "many": (40, 20, 8, 800, False, False, False),             # more workgroups than resident slots
          "fallback": (600, 200, 50, 2, True, True, False)}          # np = 1024: the vector kernel behind the new entry points
NDISTINCT = 6
NRHS = (1, 3, PANEL, PANEL + 1)


def rows_and_bounds(d):
    """E = [A; L; R; box rows] with the bounds of every row, and the entry of the dual vector (box first) each row belongs to"""
    n, nC, nComp = d["nV"], d["nC"], d["nComp"]
    lb = d.get("lb"); ub = d.get("ub")
    lb = np.full(n, -np.inf) if lb is None else lb
    ub = np.full(n, np.inf) if ub is None else ub
    boxed = np.flatnonzero(np.isfinite(lb) | np.isfinite(ub))
    A = d["A"] if d.get("A") is not None else np.zeros((0, n))
    E = np.vstack([A, d["L"], d["R"], np.eye(n)[boxed]])
    zero = np.zeros(nComp); inf = np.full(nComp, np.inf)
    get = lambda k, dflt: dflt if d.get(k) is None else d[k]
    lo = np.concatenate([get("lbA", np.full(nC, -np.inf)), get("lbL", zero), get("lbR", zero), lb[boxed]])
    hi = np.concatenate([get("ubA", np.full(nC, np.inf)), get("ubL", inf), get("ubR", inf), ub[boxed]])
    pos = np.concatenate([n + np.arange(nC + 2 * nComp), boxed])
    return E, lo, hi, pos


def working_rows(ws):
    sr = ws["slot_row"][:ws["ns"]]
    return np.sort(sr[sr >= 0])


def problems_of(key):
    n, nC, nComp, B, box, shifted, eq = SHAPES[key]
    ds = []
    for b in range(min(B, NDISTINCT)):
        d = random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, box, shifted)
        if eq:
            d["ubA"] = d["lbA"].copy()
        ds.append(d)
    return [ds[b % len(ds)] for b in range(B)]


def tiled(a, B):
    return np.tile(a, (B // len(a) + 1,) + (1,) * (a.ndim - 1))[:B]


@functools.lru_cache(maxsize=None)
def solved_case(key):
    """one solve per shape: every call the tests compare, and the working sets"""
    import lcqpow_amd as hip
    assert hip.capi.SENS_PANEL == PANEL
    n, nC, nComp, B, box, shifted, eq = SHAPES[key]
    ds = problems_of(key)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    st = bt.solution()[2]
    rng = np.random.default_rng(78)
    nref = min(B, NDISTINCT)
    V = tiled(rng.standard_normal((nref, PANEL + 1, n)), B)
    V[:, 5] = 0.0      # a zero vector inside the first panel
    counts = bt.launch_counts()
    blk = {k: bt.sensitivity(V[:, :k], blocked=True) for k in NRHS}
    vec = bt.sensitivity(V)
    perm = np.random.default_rng(3).permutation(PANEL + 1)
    permuted = bt.sensitivity(np.ascontiguousarray(V[:, perm]), blocked=True)
    alone = {j: bt.sensitivity(np.ascontiguousarray(V[:, j]), blocked=True) for j in (0, 7, PANEL)}
    nj = min(B, 3)
    jac = bt.jacobian()
    jac_part = bt.jacobian(first=1, count=2) if B >= 3 else None
    # a cap of one byte: the library clamps a chunk to one instance (np <= 512) -- nj launches and downloads
    jac_chunked = bt.jacobian(first=0, count=nj, _staging_bytes=1) if n <= 512 else None
    assert bt.launch_counts() == counts
    ws = [bt.read_working_set(b) for b in range(nref)]
    bt.close()
    return dict(ds=ds, st=st, V=V, blk=blk, vec=vec, perm=perm, permuted=permuted, alone=alone, jac=jac, jac_part=jac_part, jac_chunked=jac_chunked,
                nj=nj, ws=ws, nref=nref)


@functools.lru_cache(maxsize=None)
def reference_of(key):
    """the vectors of the call and the identity through one factorisation of K per instance"""
    c = solved_case(key)
    n = SHAPES[key][0]
    out = []
    for b in range(c["nref"]):
        d = c["ds"][b]
        E, lo, hi, pos = rows_and_bounds(d)
        W = working_rows(c["ws"][b])
        rhs = np.concatenate([c["V"][b].T, np.eye(n)], axis=1)
        dgr, mu, cond = kkt_reference(d["Q"], E[W], rhs, extended=n <= 512)
        k = PANEL + 1
        out.append(dict(E=E, pos=pos, W=W, cond=cond, dg=np.asarray(dgr.T[:k], dtype=np.float64), mu=np.asarray(mu.T[:k], dtype=np.float64),
                        Jg=np.asarray(dgr.T[k:], dtype=np.float64), Jmu=np.asarray(mu.T[k:], dtype=np.float64)))
    return out


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, nC, nComp, B = SHAPES[key][:4]
    nd = n + nC + 2 * nComp
    for k in NRHS:
        dg, db, side, info = c["blk"][k]
        assert np.array_equal(side, c["vec"][2]) and np.array_equal(info, c["vec"][3]) and side.dtype == np.int32
        worst = 0.0
        for b in range(c["nref"]):
            r = refs[b]
            assert c["st"][b]["returnValue"] == 0 and not (info[b] & 1)
            bound = 1e-12 * n * r["cond"] * np.abs(c["V"][b, :k]).max()
            dbr = np.zeros((k, nd)); dbr[:, r["pos"][r["W"]]] = r["mu"][:k]
            e_g = np.abs(dg[b] - r["dg"][:k]).max(); e_b = np.abs(db[b] - dbr).max()
            worst = max(worst, max(e_g, e_b) / bound)
            print(f"  {key} nrhs {k} instance {b}: |W| = {len(r['W'])}, cond(K) = {r['cond']:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {bound:.3g}")
            assert e_g <= bound and e_b <= bound
            inW = np.zeros(nd, dtype=bool); inW[r["pos"][r["W"]]] = True
            assert np.all(db[b][:, ~inW] == 0.0)
        print(f"  {key} nrhs {k}: worst error / bound = {worst:.3g}")
        if key == "fallback":
            assert np.array_equal(dg, c["vec"][0][:, :k]) and np.array_equal(db, c["vec"][1][:, :k])


# ---- 2: columns are independent ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_columns_are_independent(hip, key):
    c = solved_case(key)
    dg, db, side, info = c["blk"][PANEL + 1]
    pdg, pdb, pside, pinfo = c["permuted"]
    assert np.array_equal(pdg, dg[:, c["perm"]]) and np.array_equal(pdb, db[:, c["perm"]])
    assert np.array_equal(pside, side) and np.array_equal(pinfo, info)
    for j, one in c["alone"].items():
        assert np.array_equal(one[0], dg[:, j]) and np.array_equal(one[1], db[:, j]), j
    for k in NRHS:      # a shorter call is a prefix of the longer one
        assert np.array_equal(c["blk"][k][0], dg[:, :k]) and np.array_equal(c["blk"][k][1], db[:, :k])
    assert np.all(dg[:, 5] == 0.0) and np.all(db[:, 5] == 0.0)
    assert np.any(dg[:, 4] != 0.0) and np.any(dg[:, PANEL] != 0.0)


# ---- 3: blocked beside vector ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_blocked_beside_vector(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, B = SHAPES[key][0], SHAPES[key][3]
    dg, db = c["blk"][PANEL + 1][:2]
    for b in range(c["nref"]):
        bound = 2e-12 * n * refs[b]["cond"] * np.abs(c["V"][b]).max()
        e_g = np.abs(dg[b] - c["vec"][0][b]).max(); e_b = np.abs(db[b] - c["vec"][1][b]).max()
        print(f"  {key} instance {b}: max |blocked - vector| dg {e_g:.3g}, db {e_b:.3g}, twice the bound {bound:.3g}")
        assert e_g <= bound and e_b <= bound
    for b in range(c["nref"], B):      # the repeated problems of the large batch: the bits of their first copy
        k = b % c["nref"]
        assert np.array_equal(dg[b], dg[k]) and np.array_equal(db[b], db[k])
        assert np.array_equal(c["jac"][0][b], c["jac"][0][k]) and np.array_equal(c["jac"][1][b], c["jac"][1][k])


# ---- 4: the Jacobian ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_jacobian(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, nC, nComp, B = SHAPES[key][:4]
    nd = n + nC + 2 * nComp
    Jg, Jb, side, info = c["jac"]
    assert Jg.shape == (B, n, n) and Jb.shape == (B, n, nd)
    assert np.array_equal(side, c["vec"][2]) and np.array_equal(info, c["vec"][3])
    for b in range(c["nref"]):
        r = refs[b]
        bound = 1e-12 * n * r["cond"]
        Jbr = np.zeros((n, nd)); Jbr[:, r["pos"][r["W"]]] = r["Jmu"]
        e_g = np.abs(Jg[b] - r["Jg"]).max(); e_b = np.abs(Jb[b] - Jbr).max()
        sym = np.abs(Jg[b] - Jg[b].T).max()
        EW = r["E"][r["W"]]
        res = (np.abs(EW @ Jg[b].T) / np.abs(EW).sum(axis=1)[:, None]).max(initial=0.0)
        tol = 1e-12 * n * np.abs(Jg[b]).max()
        print(f"  {key} instance {b}: err Jg {e_g:.3g}, err Jb {e_b:.3g}, bound {bound:.3g}, |Jg - Jg'| {sym:.3g}, |E_r Jg'| / |E_r|_1 {res:.3g} (tol {tol:.3g})")
        assert e_g <= bound and e_b <= bound and sym <= 2 * bound and res <= tol
        inW = np.zeros(nd, dtype=bool); inW[r["pos"][r["W"]]] = True
        assert np.all(Jb[b][:, ~inW] == 0.0)
    if c["jac_part"] is not None:
        for full, part in zip(c["jac"], c["jac_part"]):
            assert np.array_equal(part, full[1:3])
    if c["jac_chunked"] is not None:
        for full, part in zip(c["jac"], c["jac_chunked"]):
            assert np.array_equal(part, full[:c["nj"]])


def test_jacobian_fallback_sub_range_and_column_chunks(hip):
    """np = 1024 has no blocked kernel: the Jacobian is the vector kernel on uploaded unit vectors, in chunks of columns under the staging
    cap, on the whole batch, with the range copied out.  The smallest shape that takes this route, held to the cases the sparse arm's general
    LDL' is held to: a sub-range, several column chunks with a partial last one, and the bits of sensitivity(identity).  The vector kernel
    treats the columns of a call independently, so every comparison is bit for bit: the host code from before the two arms shared it gave equal
    bits at np = 1024 in all four comparisons, so np.array_equal is asserted and not the bound of test_jacobian."""
    n, nC, nComp, B = 520, 40, 10, 3
    nd = n + nC + 2 * nComp
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    st = bt.solution()[2]
    su = bt.read_setup(0)
    assert su["np"] == 1024 and all(s["returnValue"] == 0 for s in st)
    counts = bt.launch_counts()
    full = bt.jacobian()
    part = bt.jacobian(first=1, count=2)
    cap = 200 * 8 * B * (n + su["np"] + nd + su["capS"])      # 200 unit vectors per launch: column chunks of 200, 200 and 120
    chunked = bt.jacobian(_staging_bytes=cap)
    one = bt.jacobian(first=2, count=1, _staging_bytes=cap + 8)      # (a cap between two multiples rounds down to the same chunks)
    eye = bt.sensitivity(np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n))))
    assert bt.launch_counts() == counts
    bt.close()
    assert full[0].shape == (B, n, n) and full[1].shape == (B, n, nd) and not np.any(full[3] & 1)
    for name, f, p, c, o, e in zip(("Jg", "Jb", "side", "info"), full, part, chunked, one, eye):
        differ = [int(np.sum(f[1:3] != p)), int(np.sum(f != c)), int(np.sum(f[2:3] != o)), int(np.sum(f != e))]
        print(f"  {name}: entries that differ from jacobian(): sub-range {differ[0]}, column chunks {differ[1]}, both {differ[2]}, sensitivity(identity) {differ[3]}")
        assert np.array_equal(p, f[1:3]) and np.array_equal(c, f) and np.array_equal(o, f[2:3]) and np.array_equal(e, f)
    assert all(np.any(full[0][b] != 0.0) for b in range(B))


def test_jacobian_in_chunks_over_a_large_batch(hip):
    c = solved_case("many")
    import lcqpow_amd as hip_
    n, nC, nComp, B = SHAPES["many"][:4]
    ds = problems_of("many")
    bt = hip_.BatchLCQP(B, n, nC, nComp, opt=hip_.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    out = bt.jacobian(_staging_bytes=8 << 20)      # about 90 KB per instance: chunks of about 90 instances, the last one partial
    bt.close()
    for full, part in zip(c["jac"], out):
        assert np.array_equal(part, full)


# ---- 5: no side effects ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nC,nComp,B,box", [(40, 20, 8, 5, False), (200, 330, 37, 3, True)])
def test_the_calls_change_nothing(hip, n, nC, nComp, B, box):
    opt = hip.default_options()
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, box, False) for b in range(B)]
    ds2 = [perturbed(d, 300 + b) for b, d in enumerate(ds)]
    out = []
    for with_call in (True, False):
        bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=opt)
        load_all(bt, ds)
        bt.run()
        first = result(bt)
        if with_call:
            counts = bt.launch_counts()
            bt.sensitivity(np.random.default_rng(1).standard_normal((B, PANEL + 2, n)), blocked=True)
            bt.jacobian()
            assert bt.launch_counts() == counts
            again = result(bt)
            assert_same_bits(first, again)
            assert np.array_equal(first["work"], again["work"])
        update_all(bt, ds2)
        bt.resolve(warm=True)
        out.append(result(bt))
        assert bt.launch_counts() == (1, 2)
        bt.close()
    assert_same_bits(out[0], out[1])
    assert np.array_equal(out[0]["work"], out[1]["work"])


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------
def test_a_batch_that_never_ran_is_refused(hip):
    from lcqpow_amd import capi
    n = 40
    d = random_lcqp(np.random.default_rng(1000), n, 20, 8, False, False)
    bt = hip.BatchLCQP(1, n, 20, 8)
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.ones(n); dg = np.full(n, 7.0); Jg = np.full((n, n), 7.0)
    sens = lambda: capi.lib().lcqp_hip_batch_sensitivity_blocked(bt.h, 1, v.ctypes.data_as(dp), dg.ctypes.data_as(dp), None, None, None)
    jac = lambda: capi.lib().lcqp_hip_batch_jacobian(bt.h, 0, 1, Jg.ctypes.data_as(dp), None, None, None)
    assert sens() == 300 and jac() == 300
    load_all(bt, [d])
    assert sens() == 300 and jac() == 300 and np.all(dg == 7.0) and np.all(Jg == 7.0)
    bt.run()
    assert sens() == 0 and jac() == 0 and not np.any(dg == 7.0) and not np.any(Jg == 7.0)
    Jg[:] = 7.0; dg[:] = 7.0
    for first, count in ((-1, 1), (0, 0), (0, -2), (0, 2), (1, 1), (2, 1)):      # outside the batch of one
        assert capi.lib().lcqp_hip_batch_jacobian(bt.h, first, count, Jg.ctypes.data_as(dp), None, None, None) == 100, (first, count)
    assert capi.lib().lcqp_hip_batch_jacobian(bt.h, 0, 1, None, None, None, None) == 100
    assert capi.lib().lcqp_hip_batch_sensitivity_blocked(bt.h, 0, v.ctypes.data_as(dp), dg.ctypes.data_as(dp), None, None, None) == 100
    assert capi.lib().lcqp_hip_batch_sensitivity_blocked(bt.h, 1, None, dg.ctypes.data_as(dp), None, None, None) == 100
    assert capi.lib().lcqp_hip_batch_sensitivity_blocked(bt.h, 1, v.ctypes.data_as(dp), None, None, None, None) == 100
    assert np.all(Jg == 7.0) and np.all(dg == 7.0)      # the refusals wrote nothing
    load_all(bt, [d])
    assert sens() == 300 and jac() == 300
    bt.run()
    bt.set_options(hip.default_options())
    assert sens() == 300 and jac() == 300
    bt.close()


def test_flag_of_a_failed_instance(hip):
    n, nC, nComp, B = 40, 20, 8, 3
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    ds[1] = dict(ds[1], g=np.full(n, np.nan))
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    st = bt.solution()[2]
    print("  return values", [s["returnValue"] for s in st])
    assert st[0]["returnValue"] == 0 and st[1]["returnValue"] != 0 and st[2]["returnValue"] == 0
    dg, db, side, info = bt.sensitivity(np.ones((B, PANEL + 1, n)), blocked=True)
    Jg, Jb, jside, jinfo = bt.jacobian()
    bt.close()
    print("  info", info, jinfo)
    assert info[1] == 1 and jinfo[1] == 1 and not (info[0] & 1) and not (info[2] & 1) and np.array_equal(info, jinfo)
    assert np.all(dg[1] == 0.0) and np.all(db[1] == 0.0) and np.all(Jg[1] == 0.0) and np.all(Jb[1] == 0.0) and np.all(side[1] == 0)
    assert np.any(dg[0] != 0.0) and np.any(Jg[2] != 0.0)


# ---- 7: the QP twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(24, 30), (2100, 60)])      # the second: np = 4096, the vector kernel behind the blocked entry points
def test_qp_twin(hip, n, m):
    rng = np.random.default_rng(n)
    Mx = rng.standard_normal((n, n)) / np.sqrt(n); Q = Mx.T @ Mx + np.eye(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n); xs = rng.standard_normal(n)
    lbA = A @ xs - rng.uniform(0.05, 0.5, m); ubA = A @ xs + rng.uniform(0.05, 0.5, m); g = 3.0 * rng.standard_normal(n)
    qh = hip.SubsolverHIP(n, m, Q, A)
    V = rng.standard_normal((PANEL + 1, n))
    dp = ctypes.POINTER(ctypes.c_double)
    dg0 = np.full((3, n), 7.0)
    assert hip.lib().lcqp_hip_qp_sensitivity_blocked(ctypes.c_void_p(qh.h), 3, V.ctypes.data_as(dp), dg0.ctypes.data_as(dp), None, None, None) == 300
    assert hip.lib().lcqp_hip_qp_jacobian(ctypes.c_void_p(qh.h), dg0.ctypes.data_as(dp), None, None, None) == 300 and np.all(dg0 == 7.0)
    ret, it, flag = qh.solve(True, g, lbA, ubA, np.zeros(n))
    assert ret == 0 and flag == 0
    dg, db, side, info = qh.sensitivity(V, blocked=True)
    vec = qh.sensitivity(V)
    # (the Jacobian of the large size would be 2100 passes of the vector kernel over a 134 MB factor in one workgroup: the batch shape
    # `fallback` covers that path at n = 600)
    Jg, Jb, jside, jinfo = qh.jacobian() if n <= 512 else (None, None, None, None)
    W = working_rows(qh.read_working_set())
    qh.close()
    assert len(W) > 0 and info == 0 and np.array_equal(side, vec[2])
    if n <= 512:
        assert jinfo == 0 and np.array_equal(jside, vec[2])
    if n > 512:
        assert np.array_equal(dg, vec[0]) and np.array_equal(db, vec[1])
    dgr, mu, cond = kkt_reference(Q, A[W], np.concatenate([V.T, np.eye(n)], axis=1) if n <= 512 else V.T, extended=n <= 512)
    dgr = np.asarray(dgr.T, dtype=np.float64); mu = np.asarray(mu.T, dtype=np.float64)
    k = PANEL + 1
    bound = 1e-12 * n * cond * np.abs(V).max()
    dbr = np.zeros((k, n + m)); dbr[:, n + W] = mu[:k]
    e_g = np.abs(dg - dgr[:k]).max(); e_b = np.abs(db - dbr).max()
    if n > 512:
        print(f"  QP n = {n}: |W| = {len(W)}, cond(K) = {cond:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {bound:.3g}")
        assert e_g <= bound and e_b <= bound
        return
    boundJ = 1e-12 * n * cond
    Jbr = np.zeros((n, n + m)); Jbr[:, n + W] = mu[k:]
    e_Jg = np.abs(Jg - dgr[k:]).max(); e_Jb = np.abs(Jb - Jbr).max(); sym = np.abs(Jg - Jg.T).max()
    print(f"  QP n = {n}: |W| = {len(W)}, cond(K) = {cond:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {bound:.3g}; "
          f"err Jg {e_Jg:.3g}, err Jb {e_Jb:.3g}, |Jg - Jg'| {sym:.3g}, bound {boundJ:.3g}")
    assert e_g <= bound and e_b <= bound
    assert e_Jg <= boundJ and e_Jb <= boundJ and sym <= 2 * boundJ


# ---- 8: torch ----------------------------------------------------------------------------------------------------------------------
def test_torch_jacobian(hip):
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    n, nC, nComp, B = 40, 20, 8, 4
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    with pytest.raises(RuntimeError, match="not the layer's last one"):
        layer.jacobian()
    w = np.random.default_rng(9).standard_normal((B, n))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64, requires_grad=True)
    x = layer(g)
    serial = layer.solves
    (torch.as_tensor(w) * x).sum().backward()
    J = layer.jacobian(serial)
    assert J.shape == (B, n, n) and J.dtype == g.dtype and J.device == g.device
    contracted = torch.einsum("bk,bkj->bj", torch.as_tensor(w), J).numpy()
    ws = [working_rows(bt.read_working_set(b)) for b in range(B)]
    for b in range(B):
        E = rows_and_bounds(ds[b])[0]
        cond = kkt_reference(ds[b]["Q"], E[ws[b]], w[b][:, None], extended=True)[2]
        bound = 2e-12 * n * cond * np.abs(w[b]).max()
        err = np.abs(contracted[b] - g.grad[b].numpy()).max()
        print(f"  instance {b}: |w' J - g.grad| {err:.3g}, twice the bound {bound:.3g}")
        assert err <= bound
    with torch.no_grad():
        layer(g.detach())
    with pytest.raises(RuntimeError, match="not the layer's last one"):
        layer.jacobian(serial)
    bt.close()
