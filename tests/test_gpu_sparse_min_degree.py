"""The general sparse LDL' in the minimum-degree ordering on the device (lcqp_sparse_general.hpp: md_front_tree; lcqp_sparse_pattern.hpp:
order_kkt; the kernels are those of nested dissection, unchanged).  Block-arrow problems of tests/block_arrow.py:

1  (400, 6, 32), B = 3: nested dissection needs a 696-row front, the handle was NULL until now.  Created, minimum degree, fronts of at most
   64 rows; x to 1e-9 and y to 1e-7 against the sparse oracle (its own general LDL' in an ordering written from the pattern's definition),
   equal return codes and statuses; the same problem through lcqpow.LCQProblem on OSQP_SPARSE reaches the sparse engine.
2  the factorisations of that handle through lcqp_hip_sparse_kkt_probe against the LDL' of tests/sparse_kkt_ref.py in the handle's ordering,
   under the componentwise bound of tests/test_gpu_sparse_factor.py: the ADMM pair and both polish pairs.
3  (256, 8, 32), B = 2: minimum degree by the class rule, nested dissection under LCQP_SPARSE_ORDERING=nd; both match the oracle.
4  warm resolve after update and after update_values, sensitivities (vector and panel form) on the (400, 6, 32) handle.
5  the forced-general (64, 32, 8), B = 6, under LCQP_SPARSE_ORDERING=md: every row class, a small N (two amalgamated fronts).

Every case is built once (functools.lru_cache) and shared; every figure and the time of every case is printed before it is asserted."""
import functools
import time

import numpy as np
import pytest

import block_arrow as BA
import sparse_kkt_ref as R
from batch_helpers import environment, handle, kkt_reference, update_all
from problems import OPT, SMALL, instances

pytestmark = pytest.mark.gpu

BIG, MID = (400, 6, 32), (256, 8, 32)
ND, MD = 1, 2


def against_oracle(oracle, ds, perm, x, y, st):
    for b, d in enumerate(ds):
        ro = BA.oracle_solve(oracle, d, perm)
        ex, ey = np.abs(x[b] - ro["x"]).max(), np.abs(y[b] - ro["y"]).max()
        print(f"    instance {b}: ret {st[b]['returnValue']} / {ro['ret']}, status {st[b]['status']} / {ro['stats']['status']}, |dx| {ex:.3g}, |dy| {ey:.3g}, "
              f"iterates {st[b]['iterTotal']} / {ro['stats']['iterTotal']}")
        assert st[b]["returnValue"] == ro["ret"] == 0 and st[b]["status"] == ro["stats"]["status"]
        assert ex < 1e-9 and ey < 1e-7


@functools.lru_cache(maxsize=None)
def solved(shape, B, ordering=None):
    """the handle of block_arrow(shape) with B instances after one run; left open for the tests that go on with it"""
    import lcqpow_amd as hip
    t0 = time.time()
    ds = [BA.block_arrow(*shape, inst=k) for k in range(B)]
    with environment({"LCQP_SPARSE_ORDERING": ordering} if ordering else {}):
        sb = handle(hip, ds, hip.default_options(**OPT))
    t1 = time.time()
    sb.run()
    x, y, st = sb.solution()
    engine = dict(lanes=sb.lanes(), fronts=sb.fronts(), ordering=sb.general_ordering(), max_front=sb.max_front(), border=sb.border())
    print(f"  {shape} B = {B} ordering {ordering}: {engine}, create + load {t1 - t0:.2f} s, run {time.time() - t1:.2f} s, timing {sb.last_timing()}")
    return dict(sb=sb, ds=ds, x=x, y=y, st=st, engine=engine)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def test_refused_pattern_runs_and_matches_the_oracle(hip, oracle):
    c = solved(BIG, 3)
    e = c["engine"]
    assert e["fronts"] > 0 and e["ordering"] == MD and 0 < e["max_front"] <= 64 and e["lanes"] == 64 and e["border"] == 0
    assert [s["returnValue"] for s in c["st"]] == [0, 0, 0]
    against_oracle(oracle, c["ds"], BA.arrow_ordering(*BIG), c["x"], c["y"], c["st"])


def test_lcqproblem_reaches_the_sparse_engine(hip):
    """the same problem in CSC form through lcqpow.LCQProblem on OSQP_SPARSE: the sparse engine (it ran densified until now), the same solution"""
    import lcqpow_amd.lcqpow as lcqpow
    t0 = time.time()
    c = solved(BIG, 3)
    d = c["ds"][0]
    wrap = lambda M: lcqpow.cscWrapper(M.shape[0], M.shape[1], M.nnz, np.asarray(M.data, dtype=float), M.indices, M.indptr)
    lcqp = lcqpow.LCQProblem(nV=d["nV"], nC=d["nC"], nComp=d["nComp"])
    options = lcqpow.Options()
    options.setPerturbStep(False)
    options.setPrintLevel(lcqpow.PrintLevel.NONE)
    options.setQPSolver(lcqpow.QPSolver.OSQP_SPARSE)
    lcqp.setOptions(options)
    Q, A, L, Rm = d["Q"].tocsc(), d["A"].tocsc(), d["L"].tocsc(), d["R"].tocsc()
    for M in (Q, A, L, Rm):
        M.sort_indices()
    assert lcqp.loadLCQP(Q=wrap(Q), g=d["g"], L=wrap(L), R=wrap(Rm), A=wrap(A), lbA=d["lbA"], ubA=d["ubA"]) == 0
    assert lcqp.runSolver() == 0
    x, y = lcqp.getPrimalSolution(), lcqp.getDualSolution()
    ex, ey = np.abs(x - c["x"][0]).max(), np.abs(y - c["y"][0]).max()
    print(f"  engine {lcqp.getLastEngine()}, |dx| {ex:.3g}, |dy| {ey:.3g} against the batch, {time.time() - t0:.2f} s")
    assert lcqp.getLastEngine() == 3
    assert ex < 1e-9 and ey < 1e-7


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_factorisations_against_numpy(hip):
    """FACTOR probes of the (400, 6, 32) handle: the ADMM pair with every row in the set, a random half and every third row; the two polish
    pairs with the empty set and every third row (the sets tests/sparse_kkt_ref.py pairs them with).  Residual in long double, the bound
    (6 N + 8) eps (|L| |D| |L'| |x| + |b|) with the reference LDL' in the handle's ordering; sparse products, N = 4032."""
    import scipy.sparse as sp
    t0 = time.time()
    c = solved(BIG, 3)
    sb, ds = c["sb"], c["ds"]
    B, n, m = len(ds), sb.nV, sb.m
    N = n + m
    perm = sb.ordering()
    opt = hip.default_options()
    cols = [R.rhs_set(N, 7 + b, unit=False) for b in range(B)]
    rhs = np.stack([cc.T for cc in cols])
    plan = {"admm": ("all", "half", "third"), "safe": ("empty", "third", "empty"), "light": ("third", "empty", "third")}
    worst = 0.0
    for rname, names in plan.items():
        regs = [R.regularisations(opt, R.scale_of(d), m, R.row_classes(d))[rname] for d in ds]
        use = np.stack([R.working_sets(m, 11 + b)[names[b]] for b in range(B)])
        sol = sb.kkt_probe(rhs, dprim=[r[0] for r in regs], ddual=np.stack([r[1] for r in regs]), use=use)
        for b, d in enumerate(ds):
            Kp = R.kkt_dense(d, regs[b][0], regs[b][1], use[b])[np.ix_(perm, perm)]
            L, D, _ = R.ldl_nopivot(Kp, R.ref_dtype(N))
            aL = sp.csr_matrix(np.abs(np.asarray(L, dtype=np.float64)))
            X, Bm = sol[b].T[perm], cols[b][perm]
            Ks = sp.coo_matrix(Kp)
            res = Bm.astype(R.LD)
            np.subtract.at(res, Ks.row, Ks.data.astype(R.LD)[:, None] * X.astype(R.LD)[Ks.col])
            wx = aL @ (np.abs(np.asarray(D, dtype=np.float64))[:, None] * (aL.T @ np.abs(X)))
            bound = R.LD((6 * N + 8) * R.EPS) * (wx.astype(R.LD) + np.abs(Bm).astype(R.LD))
            ratio = float((np.abs(res) / bound).max())
            gr = float((wx.max(axis=0) / (abs(Ks).tocsr() @ np.abs(X)).max(axis=0)).max())
            worst = max(worst, ratio)
            print(f"    {rname} / instance {b} ({names[b]}): worst error / bound = {ratio:.3e}, growth {gr:.1e}")
            assert np.isfinite(sol[b]).all() and (np.abs(res) <= bound).all()
            out = np.flatnonzero(use[b] == 0)
            assert np.array_equal(sol[b][:, n + out], -rhs[b][:, n + out])      # pivot -1, no entries: exactly -b_r
    sb.run()      # a FACTOR probe overwrites the polish factor of the last run: solved again for the tests that share the handle
    x, y, _ = sb.solution()
    assert np.array_equal(x, c["x"]) and np.array_equal(y, c["y"])
    print(f"  worst error / bound = {worst:.3e}, {time.time() - t0:.2f} s")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook,want", [(None, MD), ("nd", ND)])
def test_class_rule_and_the_hook(hip, oracle, hook, want):
    c = solved(MID, 2, hook)
    e = c["engine"]
    assert e["fronts"] > 0 and e["ordering"] == want
    assert (e["max_front"] <= 64) if want == MD else (e["max_front"] == 410 and e["fronts"] == 850)
    against_oracle(oracle, c["ds"], BA.arrow_ordering(*MID), c["x"], c["y"], c["st"])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def _fresh(hip, ds):
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    out = sb.solution()
    sb.close()
    return out


def test_warm_resolves_after_new_vectors_and_new_values(hip):
    """update + warm resolve, then update_values + warm resolve: each matches a cold solve of the same data on a fresh handle to 1e-9 / 1e-7
    with fewer iterates.  The problem is not convex: a cold solve from the origin and a warm one from the last point are only comparable
    while the cold solve of the new data ends on the complementarity branch of the old one.  The moves are sized for that with the sparse
    oracle on the CPU: with 1e-2 on g (2 % on Q) its cold solves of instance 1 change one complementarity pair, with 1e-3 (0.2 %) none."""
    t0 = time.time()
    c = solved(BIG, 3)
    sb = c["sb"]
    ds1 = [dict(d, g=d["g"] + 1e-3 * np.random.default_rng(40 + b).standard_normal(d["nV"])) for b, d in enumerate(c["ds"])]
    update_all(sb, ds1)
    sb.resolve(warm=True)
    x1, y1, st1 = sb.solution()
    ds2 = []
    for b, d in enumerate(ds1):
        s = np.random.default_rng(60 + b).uniform(0.998, 1.002, d["nV"])
        Q = d["Q"].multiply(s[:, None]).multiply(s[None, :]).tocsc(); Q.sort_indices()      # a congruence: still positive definite
        ds2.append(dict(d, Q=Q))
    assert sb.update_values(0, 3, Qx=np.stack([d["Q"].data for d in ds2])) == 0
    sb.resolve(warm=True)
    x2, y2, st2 = sb.solution()
    for tag, ds, (x, y, st) in (("vectors", ds1, (x1, y1, st1)), ("values", ds2, (x2, y2, st2))):
        xc, yc, stc = _fresh(hip, ds)
        for b in range(3):
            ex, ey = np.abs(x[b] - xc[b]).max(), np.abs(y[b] - yc[b]).max()
            print(f"    {tag} instance {b}: ret {st[b]['returnValue']} / {stc[b]['returnValue']}, |dx| {ex:.3g}, |dy| {ey:.3g}, iterates {st[b]['iterTotal']} warm / {stc[b]['iterTotal']} cold")
            assert st[b]["returnValue"] == stc[b]["returnValue"] == 0
            assert ex < 1e-9 and ey < 1e-7 and st[b]["iterTotal"] < stc[b]["iterTotal"]
    # back to the first data for the tests that share the handle
    update_all(sb, c["ds"])
    assert sb.update_values(0, 3, Qx=np.stack([d["Q"].data for d in c["ds"]])) == 0
    sb.run()
    x, y, _ = sb.solution()
    assert np.array_equal(x, c["x"]) and np.array_equal(y, c["y"])
    print(f"  {time.time() - t0:.2f} s")


def test_sensitivities_vector_and_panel(hip):
    """sensitivity(v) of every instance against numpy on the device's own working set under the bound of
    tests/test_gpu_sparse_sensitivity.py, 1e-12 (nV + |W|) cond_2(K0) |v|_inf with the instance's own K0 (dimension nV + |W|, dense); with
    set_general_panel(True), sensitivity_blocked matches the vector call under the same bound of the same instance"""
    t0 = time.time()
    c = solved(BIG, 3)
    sb, ds = c["sb"], c["ds"]
    n = sb.nV
    V = np.random.default_rng(77).standard_normal((3, 3, n))
    dg, db, side, info = sb.sensitivity(V)
    sb.set_general_panel(True)
    assert sb.sens_panel() > 0
    bg, bb, bside, binfo = sb.sensitivity_blocked(V)
    sb.set_general_panel(False)
    assert np.array_equal(side, bside) and np.array_equal(info, binfo) and not (info & 1).any()
    for b, d in enumerate(ds):
        W = np.flatnonzero(side[b])
        dgr, mu, cond = kkt_reference(d["Q"].toarray(), d["E"].toarray()[W], V[b].T, extended=True)
        bound = 1e-12 * (n + len(W)) * cond * np.abs(V[b]).max()
        dbr = np.zeros_like(db[b]); dbr[:, W] = np.asarray(mu.T, dtype=np.float64)
        e_g, e_b = np.abs(dg[b] - np.asarray(dgr.T, dtype=np.float64)).max(), np.abs(db[b] - dbr).max()
        p_g, p_b = np.abs(bg[b] - dg[b]).max(), np.abs(bb[b] - db[b]).max()
        print(f"  instance {b}: |W| = {len(W)}, cond(K0) = {cond:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, panel against vector: dg {p_g:.3g}, db {p_b:.3g}, bound {bound:.3g}")
        assert e_g <= bound and e_b <= bound
        assert p_g <= bound and p_b <= bound
    print(f"  {time.time() - t0:.2f} s")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_forced_general_small_under_minimum_degree(hip, oracle):
    t0 = time.time()
    ds = instances(SMALL, 6)
    with environment({"LCQP_SPARSE_GENERAL": "1", "LCQP_SPARSE_ORDERING": "md"}):
        sb = handle(hip, ds, hip.default_options(**OPT))
    assert sb.fronts() > 0 and sb.general_ordering() == MD and sb.lanes() == 64 and 0 < sb.max_front() <= 64
    sb.run()
    x, y, st = sb.solution()
    perm = sb.ordering()
    print(f"  fronts {sb.fronts()}, largest {sb.max_front()}")
    sb.close()
    n, nC, nK = SMALL
    for b, d in enumerate(ds):
        ro = oracle.sparse_lcqp_solve(n, nC, nK, d["Q"].tocsr(), d["g"], d["E"].tocsr(), lbA=d["lbA"], ubA=d["ubA"], perm=perm, w=-1, kb=0,
                                      opt=oracle.default_options(perturbStep=0))
        ex, ey = np.abs(x[b] - ro["x"]).max(), np.abs(y[b] - ro["y"]).max()
        print(f"    instance {b}: ret {st[b]['returnValue']} / {ro['ret']}, |dx| {ex:.3g}, |dy| {ey:.3g}")
        assert st[b]["returnValue"] == ro["ret"] and st[b]["status"] == ro["stats"]["status"]
        assert ex < 1e-9 and ey < 1e-7
    print(f"  {time.time() - t0:.2f} s")


def test_band_pattern_ignores_the_ordering_hook(hip):
    """LCQP_SPARSE_ORDERING sends no band pattern to the general engine"""
    ds = instances(SMALL, 1)
    with environment({"LCQP_SPARSE_ORDERING": "md"}):
        sb = handle(hip, ds, hip.default_options(**OPT))
    assert sb.fronts() == 0 and sb.general_ordering() == 0 and sb.max_front() == 0
    sb.close()


def test_refusal_says_that_minimum_degree_was_not_taken(hip):
    """sixty dense rows over seven hundred variables stay refused (tests/test_gpu_sparse.py); the message of create now adds that a
    minimum-degree ordering fits and why it is not taken"""
    import scipy.sparse as sp
    n, nC, nK = 700, 60, 8
    L = np.zeros((nK, n)); R = np.zeros((nK, n))
    L[np.arange(nK), np.arange(nK)] = 1; R[np.arange(nK), nK + np.arange(nK)] = 1
    with pytest.raises(RuntimeError, match="too dense for the sparse engine.*minimum-degree ordering fits .* is not taken"):
        hip.SparseBatchLCQP(1, n, nC, nK, sp.identity(n, format="csc"), sp.csc_matrix(np.vstack([np.ones((nC, n)), L, R])))
