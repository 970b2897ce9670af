"""Solution sensitivities (lcqp_hip_batch_sensitivity / lcqp_hip_qp_sensitivity, lcqpow_amd/diff.py; DESIGN.md section 3a').

1  dg, db against numpy on the device's own working set W: K = [[Q, E_W'], [E_W, 0]], K [d; mu] = [v; 0], dg = -d, db_W = mu.  The
   reference is float64 LU refined with np.longdouble residuals up to np = 512 and plain float64 beyond; bound
   max|delta| <= 1e-12 nV cond_2(K) |v|_inf (the form of the Ti'Ti S_W bound of tests/test_gpu_setup.py).
2  W is the active set by value.   3  structure that needs no reference.   4  central differences through the product's own warm
re-solve, bound stationarityTolerance |v|_1 / (h lambda_min(Q)) from the solver's exit test.   5  the call changes nothing.
6  flag bits.   7  the QP twin.   8  torch.

Problems: tests/problems.py::random_lcqp with default_rng(1000 + instance).  Every figure is printed before it is asserted."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import problems as P
from batch_helpers import assert_same_bits, grown_and_fresh, kkt_reference, load_all, result, stack, update_all
from problems import perturbed, random_lcqp

pytestmark = pytest.mark.gpu

H_FD = 1e-6
#          n,  nC, nComp, B, box, shifted, equalities     path
SHAPES = {"np128": (40, 20, 8, 6, False, False, False),
          "np256_lds_rows": (200, 330, 37, 3, True, False, False),
          "np384": (300, 100, 40, 2, False, False, False),
          "np1024": (600, 200, 50, 2, True, True, False),
          "slow_ti_apply": (400, 300, 20, 2, False, False, True),       # ubA = lbA on all 300 rows: n_T > 256
          "four_per_cu": (40, 20, 8, 800, False, False, False)}        # more than three workgroups per CU
NDISTINCT = 6


def problems_of(key):
    n, nC, nComp, B, box, shifted, eq = SHAPES[key]
    ds = []
    for b in range(min(B, NDISTINCT)):
        d = random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, box, shifted)
        if eq:
            d["ubA"] = d["lbA"].copy()
        ds.append(d)
    return [ds[b % len(ds)] for b in range(B)]


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


@functools.lru_cache(maxsize=None)
def solved_case(key):
    """one solve per shape, shared by tests 1 - 3: the solution, the working sets, and every sensitivity call the tests compare"""
    import lcqpow_amd as hip
    n, nC, nComp, B, box, shifted, eq = SHAPES[key]
    ds = problems_of(key)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    x, y, st = bt.solution()
    rng = np.random.default_rng(77)
    nref = min(B, NDISTINCT)
    V = np.tile(rng.standard_normal((nref, 3, n)), (B // nref + 1, 1, 1))[:B]
    counts = bt.launch_counts()
    dg, db, side, info = bt.sensitivity(V)
    assert bt.launch_counts() == counts
    singles = [bt.sensitivity(V[:, k]) for k in range(3)]
    alpha = 0.7
    lin = bt.sensitivity(alpha * V[:, 0] + V[:, 1])
    ws = [bt.read_working_set(b) for b in range(nref)]
    bt.close()
    return dict(ds=ds, x=x, y=y, st=st, V=V, dg=dg, db=db, side=side, info=info, singles=singles, alpha=alpha, lin=lin, ws=ws, nref=nref)


@functools.lru_cache(maxsize=None)
def reference_of(key):
    c = solved_case(key)
    n = SHAPES[key][0]
    out = []
    for b in range(c["nref"]):
        d = c["ds"][b]
        E, lo, hi, pos = rows_and_bounds(d)
        W = working_rows(c["ws"][b])
        dgr, mu, cond = kkt_reference(d["Q"], E[W], c["V"][b].T, extended=n <= 512)
        out.append(dict(E=E, lo=lo, hi=hi, pos=pos, W=W, dg=dgr.T, mu=mu.T, cond=cond))
    return out


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, nC, nComp, B = SHAPES[key][:4]
    nd = n + nC + 2 * nComp
    worst = 0.0
    for b in range(c["nref"]):
        r = refs[b]
        assert c["st"][b]["returnValue"] == 0
        assert not (c["info"][b] & 1)
        bound = 1e-12 * n * r["cond"] * np.abs(c["V"][b]).max()
        dbr = np.zeros((3, nd)); dbr[:, r["pos"][r["W"]]] = np.asarray(r["mu"], dtype=np.float64)
        e_g = np.abs(c["dg"][b] - np.asarray(r["dg"], dtype=np.float64)).max()
        e_b = np.abs(c["db"][b] - dbr).max()
        worst = max(worst, max(e_g, e_b) / bound)
        print(f"  {key} instance {b}: |W| = {len(r['W'])}, cond(K) = {r['cond']:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {bound:.3g}, info {c['info'][b]}")
        assert e_g <= bound and e_b <= bound
        # rows outside W: zero derivative and side 0; rows of W: side says which bound
        inW = np.zeros(nd, dtype=bool); inW[r["pos"][r["W"]]] = True
        assert np.all(c["db"][b][:, ~inW] == 0.0) and np.all(c["side"][b][~inW] == 0) and np.all(c["side"][b][inW] != 0)
    print(f"  {key}: worst error / bound = {worst:.3g}")
    for b in range(c["nref"], B):      # the repeated problems of the large batch: the bits of their first copy
        k = b % c["nref"]
        assert np.array_equal(c["dg"][b], c["dg"][k]) and np.array_equal(c["db"][b], c["db"][k])
        assert np.array_equal(c["side"][b], c["side"][k]) and c["info"][b] == c["info"][k]


# ---- 2: W is the active set by value -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_working_set_is_the_active_set_by_value(hip, key):
    c, refs = solved_case(key), reference_of(key)
    excluded = 0
    for b in range(c["nref"]):
        r = refs[b]
        if c["info"][b] != 0:
            excluded += 1
            print(f"  {key} instance {b}: info = {c['info'][b]}, excluded")
            continue
        ex = r["E"] @ c["x"][b]
        active = np.flatnonzero((np.abs(ex - r["lo"]) <= 1e-9) | (np.abs(ex - r["hi"]) <= 1e-9))
        print(f"  {key} instance {b}: {len(active)} rows active by value, {len(r['W'])} in W")
        assert np.array_equal(active, r["W"])
        at_lo = np.abs(ex - r["lo"]) <= 1e-9; at_hi = np.abs(ex - r["hi"]) <= 1e-9
        want = np.where(at_lo & at_hi, 2, np.where(at_hi, 1, -1))[r["W"]]
        assert np.array_equal(c["side"][b][r["pos"][r["W"]]], want)
    assert excluded <= c["nref"] // 8, excluded


# ---- 3: structure, independent of any reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_structure(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n = SHAPES[key][0]
    for k in range(3):      # nrhs = 3 in one call is three calls with nrhs = 1, bit for bit
        assert np.array_equal(c["singles"][k][0], c["dg"][:, k]) and np.array_equal(c["singles"][k][1], c["db"][:, k])
        assert np.array_equal(c["singles"][k][2], c["side"]) and np.array_equal(c["singles"][k][3], c["info"])
    for b in range(c["nref"]):
        r = refs[b]
        V, dg = c["V"][b], c["dg"][b]
        EW = r["E"][r["W"]]
        # |E_W| |dg| as norms, row by row: |E_r|_1 |dg|_inf (Hoelder's bound of the product whose rounding this is).  The entry-wise
        # product |E_r| . |dg| would be the residual itself on a row with a single non-zero, where the exact value is zero.
        res = (np.abs(EW @ dg.T) / np.abs(EW).sum(axis=1)[:, None]).max(initial=0.0)
        tol = 1e-12 * n * np.abs(dg).max()
        err1 = lambda v: 1e-12 * n * r["cond"] * np.abs(v).max()      # the entry-wise bound of test 1
        sym = abs(V[0] @ dg[1] - V[1] @ dg[0])
        sym_tol = np.abs(V[0]).sum() * err1(V[1]) + np.abs(V[1]).sum() * err1(V[0])
        a = c["alpha"]
        lin = np.abs(c["lin"][0][b] - (a * dg[0] + dg[1])).max()
        lin_tol = err1(a * V[0] + V[1]) + a * err1(V[0]) + err1(V[1])
        print(f"  {key} instance {b}: |E_r dg| / |E_r|_1 {res:.3g} (tol {tol:.3g}), symmetry {sym:.3g} (tol {sym_tol:.3g}), linearity {lin:.3g} (tol {lin_tol:.3g})")
        assert res <= tol and sym <= sym_tol and lin <= lin_tol
        assert np.any(dg != 0.0)


# ---- 4: finite differences through the product's own warm re-solve ---------------------------------------------------------------
@pytest.mark.parametrize("n,nC,nComp", [(40, 20, 8), (200, 330, 37)])
def test_finite_differences_through_warm_resolves(hip, n, nC, nComp):
    B = 8
    opt = hip.default_options(perturbStep=0)
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    load_all(bt, ds)
    bt.run()
    rng = np.random.default_rng(5)
    V = rng.standard_normal((B, n)); Z = rng.standard_normal((B, n)); ZB = rng.standard_normal((B, nC))
    dg, db, side, info = bt.sensitivity(V)
    W0 = [working_rows(bt.read_working_set(b)) for b in range(B)]
    assert all(s["returnValue"] == 0 for s in bt.solution()[2])
    sA = side[:, n:n + nC]
    lam_min = np.array([np.linalg.eigvalsh(d["Q"])[0] for d in ds])
    bound = opt.stationarityTolerance * np.abs(V).sum(axis=1) / (H_FD * lam_min)

    def resolved(ds2):
        update_all(bt, ds2)
        bt.resolve(warm=True)
        x, _, st = bt.solution()
        keep = np.array([st[b]["returnValue"] == 0 and np.array_equal(working_rows(bt.read_working_set(b)), W0[b]) for b in range(B)])
        return x, keep

    def compare(name, plus, minus, predicted):
        xp, kp = resolved(plus); xm, km = resolved(minus)
        keep = kp & km & (info == 0)
        fd = np.einsum("bi,bi->b", V, xp - xm) / (2 * H_FD)
        err = np.abs(fd - predicted)
        for b in range(B):
            print(f"  ({n},{nC},{nComp}) {name} instance {b}: fd {fd[b]:+.9e} predicted {predicted[b]:+.9e} err {err[b]:.3g} "
                  f"(rel {err[b] / max(abs(predicted[b]), 1e-300):.3g}) bound {bound[b]:.3g} kept {bool(keep[b])}")
        assert np.count_nonzero(~keep) <= B // 8, keep
        assert np.all(err[keep] <= bound[keep])

    compare("g", [dict(d, g=d["g"] + H_FD * Z[b]) for b, d in enumerate(ds)], [dict(d, g=d["g"] - H_FD * Z[b]) for b, d in enumerate(ds)],
            np.einsum("bi,bi->b", dg, Z))
    # the bound each row of W among the rows of A sits on moves by h zb (an equality row: both bounds)
    def shifted(sign):
        out = []
        for b, d in enumerate(ds):
            s = sign * H_FD * ZB[b]
            out.append(dict(d, lbA=d["lbA"] + np.where((sA[b] == -1) | (sA[b] == 2), s, 0.0), ubA=d["ubA"] + np.where((sA[b] == 1) | (sA[b] == 2), s, 0.0)))
        return out
    assert np.count_nonzero(sA) > 0
    compare("lbA/ubA", shifted(+1), shifted(-1), np.einsum("bi,bi->b", db[:, n:n + nC] * (sA != 0), ZB))
    bt.close()


# ---- 5: no side effects --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nC,nComp,B,box", [(40, 20, 8, 5, False), (200, 330, 37, 3, True)])
def test_the_call_changes_nothing(hip, n, nC, nComp, B, box):
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
            bt.sensitivity(np.random.default_rng(1).standard_normal((B, 2, n)))
            assert bt.launch_counts() == counts
            again = result(bt)      # the stored solution, statistics and work sums are the ones of the run
            assert_same_bits(first, again)
            assert np.array_equal(first["work"], again["work"])
        update_all(bt, ds2)
        bt.resolve(warm=True)
        out.append(result(bt))
        assert bt.launch_counts() == (1, 2)
        bt.close()
    assert_same_bits(out[0], out[1])
    assert np.array_equal(out[0]["work"], out[1]["work"])


def test_buffers_grow_from_a_live_allocation(hip):
    n, nC, nComp, B = 40, 20, 8, 2
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]

    def solved():
        bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
        load_all(bt, ds)
        bt.run()
        return bt
    grown_and_fresh(solved, np.random.default_rng(77).standard_normal((B, 3, n)))


# ---- 6: flags ------------------------------------------------------------------------------------------------------------------------
def test_flag_of_a_failed_instance(hip):
    ds = [P.warm_up_w_A(), P.infeasible(), P.warm_up_w_A()]
    bt = hip.BatchLCQP(3, 2, 1, 1, opt=hip.default_options())
    load_all(bt, ds)
    bt.run()
    st = bt.solution()[2]
    assert st[0]["returnValue"] == 0 and st[1]["returnValue"] != 0 and st[2]["returnValue"] == 0
    dg, db, side, info = bt.sensitivity(np.ones((3, 2)))
    bt.close()
    print("  info", info, "dg", dg.tolist())
    assert info[1] & 1 and not (info[0] & 1) and not (info[2] & 1)
    assert np.all(dg[1] == 0.0) and np.all(db[1] == 0.0) and np.all(side[1] == 0)
    assert np.any(side[0] != 0) and np.array_equal(dg[0], dg[2]) and np.array_equal(db[0], db[2])


def test_flag_of_dependent_rows(hip):
    d = P.example_data()
    bt = hip.BatchLCQP(1, d["nV"], d["nC"], d["nComp"], with_box=d.get("lb") is not None or d.get("ub") is not None, opt=hip.default_options())
    load_all(bt, [d])
    bt.run()
    assert bt.solution()[2][0]["returnValue"] == 0
    dg, db, side, info = bt.sensitivity(np.ones((1, d["nV"])))
    bt.close()
    print("  info", info)
    assert info[0] & 2 and not (info[0] & 1)
    assert np.all(np.isfinite(dg)) and np.all(np.isfinite(db))


def test_a_batch_that_never_ran_is_refused(hip):
    from lcqpow_amd import capi
    n = 40
    d = random_lcqp(np.random.default_rng(1000), n, 20, 8, False, False)
    bt = hip.BatchLCQP(1, n, 20, 8)
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.ones(n); dg = np.full(n, 7.0)
    call = lambda: capi.lib().lcqp_hip_batch_sensitivity(bt.h, 1, v.ctypes.data_as(dp), dg.ctypes.data_as(dp), None, None, None)
    assert call() == 300
    load_all(bt, [d])
    assert call() == 300 and np.all(dg == 7.0)
    bt.run()
    assert call() == 0 and not np.any(dg == 7.0)
    load_all(bt, [d])      # a load since the last solve: the stored state belongs to other data
    assert call() == 300
    bt.run()
    bt.set_options(hip.default_options())
    assert call() == 300
    bt.close()


# ---- 7: the QP twin --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(24, 30), (2100, 60)])      # the second: np = 4096, the two-copy triangular solves and combines
def test_qp_twin(hip, n, m):
    rng = np.random.default_rng(n)
    Mx = rng.standard_normal((n, n)) / np.sqrt(n); Q = Mx.T @ Mx + np.eye(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n); xs = rng.standard_normal(n)
    lbA = A @ xs - rng.uniform(0.05, 0.5, m); ubA = A @ xs + rng.uniform(0.05, 0.5, m); g = 3.0 * rng.standard_normal(n)
    qh = hip.SubsolverHIP(n, m, Q, A)
    V = rng.standard_normal((3, n))
    dp = ctypes.POINTER(ctypes.c_double)
    dg0 = np.full((3, n), 7.0)
    rc = hip.lib().lcqp_hip_qp_sensitivity(ctypes.c_void_p(qh.h), 3, V.ctypes.data_as(dp), dg0.ctypes.data_as(dp), None, None, None)
    assert rc == 300 and np.all(dg0 == 7.0)      # before its first solve
    ret, it, flag = qh.solve(True, g, lbA, ubA, np.zeros(n))
    assert ret == 0 and flag == 0
    x, y = qh.getSolution()
    dg, db, side, info = qh.sensitivity(V)
    W = working_rows(qh.read_working_set())
    one = qh.sensitivity(V[1])
    qh.close()
    assert len(W) > 0 and info == 0
    dgr, mu, cond = kkt_reference(Q, A[W], V.T, extended=n <= 512)
    bound = 1e-12 * n * cond * np.abs(V).max()
    dbr = np.zeros((3, n + m)); dbr[:, n + W] = np.asarray(mu.T, dtype=np.float64)
    e_g = np.abs(dg - np.asarray(dgr.T, dtype=np.float64)).max(); e_b = np.abs(db - dbr).max()
    print(f"  QP n = {n}: |W| = {len(W)}, cond(K) = {cond:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {bound:.3g}")
    assert e_g <= bound and e_b <= bound
    ax = A @ x
    want = np.zeros(n + m, dtype=np.int32); want[n + W] = np.where(np.abs(ax[W] - ubA[W]) < np.abs(ax[W] - lbA[W]), 1, -1)
    assert np.array_equal(side, want)
    assert np.array_equal(one[0], dg[1]) and np.array_equal(one[1], db[1])


# ---- 8: torch ------------------------------------------------------------------------------------------------------------------------
def test_torch_function(hip):
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    n, nC, nComp, B = 40, 20, 8, 4
    opt = hip.default_options(perturbStep=0)
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    load_all(bt, ds)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    rng = np.random.default_rng(9)
    w = rng.standard_normal((B, n))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64, requires_grad=True)
    x = layer(g)
    assert x.dtype == torch.float64 and x.shape == (B, n) and x.device == g.device
    assert bt.launch_counts() == (1, 1) and all(s["returnValue"] == 0 for s in layer.stats)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # every instance is differentiable: no warning
        (torch.as_tensor(w) * x).sum().backward()
    dg, db, side, info = bt.sensitivity(w)
    assert np.all(info == 0) and np.array_equal(g.grad.numpy(), dg)
    W0 = [working_rows(bt.read_working_set(b)) for b in range(B)]
    lam_min = np.array([np.linalg.eigvalsh(d["Q"])[0] for d in ds])
    bound = opt.stationarityTolerance * np.abs(w).sum(axis=1) / (H_FD * lam_min)
    g0 = g.detach()
    for k in range(5):
        z = torch.as_tensor(rng.standard_normal((B, n)))
        vals, keep = [], np.ones(B, dtype=bool)
        for sgn in (+1.0, -1.0):
            with torch.no_grad():
                xs = layer(g0 + sgn * H_FD * z)
            vals.append((torch.as_tensor(w) * xs).sum(dim=1).numpy())
            keep &= np.array([np.array_equal(working_rows(bt.read_working_set(b)), W0[b]) for b in range(B)])
        fd = (vals[0] - vals[1]) / (2 * H_FD)
        pred = (g.grad * z).sum(dim=1).numpy()
        err = np.abs(fd - pred)
        print(f"  direction {k}: err {err}, bound {bound}, kept {keep}")
        assert np.count_nonzero(~keep) <= B // 8
        assert np.all(err[keep] <= bound[keep])
    assert bt.launch_counts() == (1, 11)      # one setup; every later forward is update + warm resolve
    # gradients with respect to the bounds, and the one warning that counts flagged instances
    lbA = torch.tensor(stack(ds, "lbA"), dtype=torch.float64, requires_grad=True)
    ubA = torch.tensor(stack(ds, "ubA"), dtype=torch.float64, requires_grad=True)
    x = layer(g0, lbA, ubA)
    (torch.as_tensor(w) * x).sum().backward()
    dg, db, side, info = bt.sensitivity(w)
    parts = hip.split_bound_derivatives(db, side, n, nC, nComp)
    assert np.array_equal(lbA.grad.numpy(), parts["dlbA"]) and np.array_equal(ubA.grad.numpy(), parts["dubA"])
    assert np.count_nonzero(parts["dlbA"]) + np.count_nonzero(parts["dubA"]) == np.count_nonzero(side[:, n:n + nC])
    bt.close()


def test_torch_function_warns_about_flagged_instances(hip):
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    ds = [P.warm_up_w_A(), P.infeasible(), P.warm_up_w_A()]
    bt = hip.BatchLCQP(3, 2, 1, 1, opt=hip.default_options())
    load_all(bt, ds)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64, requires_grad=True)
    x = layer(g)
    with pytest.warns(RuntimeWarning, match="of 3 instances") as rec:
        x.sum().backward()
    assert len(rec) == 1
    assert layer.info[1] & 1 and not (layer.info[0] & 1) and not (layer.info[2] & 1) and torch.all(g.grad[1] == 0)
    bt.close()
