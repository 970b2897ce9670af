"""Solution sensitivities of the sparse arm (lcqp_hip_sparse_sensitivity, SparseBatchLCQPLayer; DESIGN.md section 3a'').

1  dg, db against numpy on the device's own working set W (from `side`): K0 = [[Q, E_W'], [E_W, 0]] dense from the CSC data,
   K0 [d; mu] = [v; 0], dg = -d, db_W = mu; float64 LU refined with np.longdouble residuals (kkt_reference of tests/batch_helpers.py); bound
   max|delta| <= 1e-12 (nV + |W|) cond_2(K0) |v|_inf.
2  W is the active set by value, and info.   3  structure that needs no reference.   4  central differences through the product's own
warm re-solves, bound stationarityTolerance |v|_1 / (h lambda_min(Q)); fixes the sign of db.   5  the call changes nothing.
6  state errors and a failed instance.   7  torch.

Shapes: the ones tests/test_gpu_sparse_resolve.py uses to reach every engine (tests/problems.py).  Every figure is printed before it is asserted."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import problems as P
from batch_helpers import assert_same_bits, environment, grown_and_fresh, handle, kkt_reference, result, update_all
from problems import MID, OPT, SMALL, circle_instances, instances, moved

pytestmark = pytest.mark.gpu

H_FD = 1e-6
NOT_SETUP = 300
#        instances                       environment                      engine
CASES = {"small": (("synth", SMALL, 6), {}),
         "lanes 32": (("synth", SMALL, 6), {"LCQP_SPARSE_LANES": "32"}),
         "pools of 4": (("synth", SMALL, 6), {"LCQP_SPARSE_POOL": "4"}),      # a ragged last pool
         "small, general ldl": (("synth", SMALL, 6), {"LCQP_SPARSE_GENERAL": "1"}),      # always the safe regularisation, and the tightest bound
         "mid": (("synth", MID, 2), {}),
         "mid, general ldl": (("synth", MID, 2), {"LCQP_SPARSE_GENERAL": "1"}),
         "grid, general ldl": (("grid", (44, 300, 200), 2), {}),
         "bordered circle": (("circle", 100, 2), {})}


def instances_of(key):
    (kind, shape, B), _ = CASES[key]
    if kind == "synth":
        return instances(shape, B)
    if kind == "circle":
        return circle_instances(B)
    d = P.grid_lcqp(*shape)
    d["Q"].sort_indices(); d["E"].sort_indices()
    return [dict(d) for _ in range(B)]


def bounds_of(d):
    nK = d["nComp"]
    return np.concatenate([d["lbA"], np.zeros(2 * nK)]), np.concatenate([d["ubA"], np.full(2 * nK, np.inf)])


@functools.lru_cache(maxsize=None)
def solved_case(key):
    """one solve per case, shared by tests 1 - 3 (and 6): the solution and every sensitivity call the tests compare"""
    import lcqpow_amd as hip
    ds = instances_of(key)
    B, n = len(ds), ds[0]["nV"]
    with environment(CASES[key][1]):
        sb = handle(hip, ds, hip.default_options(**OPT))
    engine = dict(lanes=sb.lanes(), fronts=sb.fronts(), border=sb.border())
    sb.run()
    x, y, st = sb.solution()
    V = np.random.default_rng(77).standard_normal((B, 3, n))
    counts = sb.launch_counts()
    dg, db, side, info = sb.sensitivity(V)
    singles = [sb.sensitivity(V[:, k]) for k in range(3)]
    again = sb.sensitivity(V)
    assert sb.launch_counts() == counts
    sb.close()
    return dict(ds=ds, x=x, y=y, st=st, V=V, dg=dg, db=db, side=side, info=info, singles=singles, again=again, engine=engine)


@functools.lru_cache(maxsize=None)
def reference_of(key):
    c = solved_case(key)
    out = []
    for b, d in enumerate(c["ds"]):
        E = d["E"].toarray()
        W = np.flatnonzero(c["side"][b])
        dgr, mu, cond = kkt_reference(d["Q"].toarray(), E[W], c["V"][b].T, extended=True)
        out.append(dict(E=E, W=W, dg=np.asarray(dgr.T, dtype=np.float64), mu=np.asarray(mu.T, dtype=np.float64), cond=cond))
    return out


def bound_1(c, r, b):
    return 1e-12 * (c["ds"][b]["nV"] + len(r["W"])) * r["cond"] * np.abs(c["V"][b]).max()


def test_the_cases_reach_every_engine(hip):
    eng = {k: solved_case(k)["engine"] for k in ("small", "lanes 32", "mid, general ldl", "grid, general ldl", "bordered circle")}
    print(" ", eng)
    assert eng["small"]["lanes"] == 8 and eng["lanes 32"]["lanes"] == 32
    assert eng["mid, general ldl"]["fronts"] > 0 and eng["grid, general ldl"]["fronts"] > 4 and eng["grid, general ldl"]["lanes"] == 64
    assert eng["bordered circle"]["border"] > 0


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    m = c["side"].shape[1]
    worst = 0.0
    for b, r in enumerate(refs):
        assert c["st"][b]["returnValue"] == 0 and not (c["info"][b] & 1)
        bound = bound_1(c, r, b)
        dbr = np.zeros((3, m)); dbr[:, r["W"]] = r["mu"]
        e_g = np.abs(c["dg"][b] - r["dg"]).max()
        e_b = np.abs(c["db"][b] - dbr).max()
        worst = max(worst, max(e_g, e_b) / bound)
        print(f"  {key} instance {b}: |W| = {len(r['W'])}, cond(K0) = {r['cond']:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {bound:.3g}, info {c['info'][b]}")
        assert e_g <= bound and e_b <= bound
    print(f"  {key}: worst error / bound = {worst:.3g}")


# ---- 2: W is the active set by value; the flags ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_working_set_is_the_active_set_by_value(hip, key):
    c, refs = solved_case(key), reference_of(key)
    for b, (d, r) in enumerate(zip(c["ds"], refs)):
        lo, hi = bounds_of(d)
        ex = r["E"] @ c["x"][b]
        at_lo = np.abs(ex - lo) <= 1e-9; at_hi = np.abs(ex - hi) <= 1e-9
        active = np.flatnonzero(at_lo | at_hi)
        print(f"  {key} instance {b}: {len(active)} rows active by value, {len(r['W'])} in W, info {c['info'][b]}")
        assert np.array_equal(active, r["W"])
        want = np.where(at_lo & at_hi, 2, np.where(at_hi, 1, np.where(at_lo, -1, 0)))
        assert np.array_equal(c["side"][b], want)
        if key == "bordered circle":
            assert (c["info"][b] & ~4) == 0
        else:
            assert c["info"][b] == 0


# ---- 3: structure, independent of any reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_structure(hip, key):
    c, refs = solved_case(key), reference_of(key)
    for k in range(3):      # nrhs = 3 in one call is three calls with nrhs = 1, bit for bit
        assert np.array_equal(c["singles"][k][0], c["dg"][:, k]) and np.array_equal(c["singles"][k][1], c["db"][:, k])
        assert np.array_equal(c["singles"][k][2], c["side"]) and np.array_equal(c["singles"][k][3], c["info"])
    for a, z in zip(c["again"], (c["dg"], c["db"], c["side"], c["info"])):      # a second call returns the bits of the first
        assert np.array_equal(a, z)
    for b, r in enumerate(refs):
        V = c["V"][b]
        bound = bound_1(c, r, b)
        res = np.abs(r["E"][r["W"]] @ c["dg"][b].T).max(initial=0.0)
        outside = np.ones(c["side"].shape[1], dtype=bool); outside[r["W"]] = False
        assert np.all(c["db"][b][:, outside] == 0.0)
        # v1'(dx/dg) v2 from the call with v2 against v2'(dx/dg) v1 from the call with v1
        dg1, dg2 = c["singles"][0][0][b], c["singles"][1][0][b]
        sym = abs(V[0] @ dg2 - V[1] @ dg1)
        sym_tol = (np.abs(V[0]).sum() + np.abs(V[1]).sum()) * bound
        print(f"  {key} instance {b}: |E_W dg| {res:.3g} (bound {bound:.3g}), symmetry {sym:.3g} (tol {sym_tol:.3g})")
        assert res <= bound and sym <= sym_tol
        assert np.any(c["dg"][b] != 0.0)


# ---- 4: central differences through the product's own warm re-solves -------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", [(SMALL, 4), (MID, 2)])
def test_finite_differences_through_warm_resolves(hip, shape, B):
    n, nC, nK = shape
    opt = hip.default_options(**OPT)
    ds = instances(shape, B)
    sb = handle(hip, ds, opt)
    sb.run()
    assert all(s["returnValue"] == 0 for s in sb.solution()[2])
    rng = np.random.default_rng(5)
    V = rng.standard_normal((B, n)); Z = rng.standard_normal((2, B, n)); ZB = rng.standard_normal((B, 2))
    dg, db, side, info = sb.sensitivity(V)
    assert np.all(info == 0)
    lam_min = np.array([np.linalg.eigvalsh(d["Q"].toarray())[0] for d in ds])
    bound = opt.stationarityTolerance * np.abs(V).sum(axis=1) / (H_FD * lam_min)

    def resolved(ds2):
        update_all(sb, ds2)
        sb.resolve(warm=True)
        x, _, st = sb.solution()
        side2 = sb.sensitivity(V)[2]
        return x, np.array([st[b]["returnValue"] == 0 and np.array_equal(side2[b], side[b]) for b in range(B)])

    def compare(name, plus, minus, predicted):
        xp, kp = resolved(plus); xm, km = resolved(minus)
        fd = np.einsum("bi,bi->b", V, xp - xm) / (2 * H_FD)
        err = np.abs(fd - predicted)
        for b in range(B):
            print(f"  {shape} {name} instance {b}: fd {fd[b]:+.9e} predicted {predicted[b]:+.9e} err {err[b]:.3g} "
                  f"(rel {err[b] / max(abs(predicted[b]), 1e-300):.3g}) bound {bound[b]:.3g} W kept {bool(kp[b] and km[b])}")
        assert np.all(kp & km)                     # every instance keeps W at both offsets
        assert np.all(err <= bound)

    for k in range(2):
        compare(f"g direction {k}", [dict(d, g=d["g"] + H_FD * Z[k, b]) for b, d in enumerate(ds)],
                [dict(d, g=d["g"] - H_FD * Z[k, b]) for b, d in enumerate(ds)], np.einsum("bi,bi->b", dg, Z[k]))
    # the bound two active rows of A sit on moves by h zb (an equality row: both bounds)
    rows = [np.flatnonzero(side[b, :nC])[:2] for b in range(B)]
    assert all(len(r) == 2 for r in rows), rows

    def shifted(sign):
        out = []
        for b, d in enumerate(ds):
            lbA, ubA = d["lbA"].copy(), d["ubA"].copy()
            for j, r in enumerate(rows[b]):
                if side[b, r] in (-1, 2): lbA[r] += sign * H_FD * ZB[b, j]
                if side[b, r] in (1, 2): ubA[r] += sign * H_FD * ZB[b, j]
            out.append(dict(d, lbA=lbA, ubA=ubA))
        return out
    compare("lbA/ubA", shifted(+1), shifted(-1), np.array([db[b, rows[b]] @ ZB[b] for b in range(B)]))
    sb.close()


# ---- 5: no side effects --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "mid, general ldl", "bordered circle"])
@pytest.mark.parametrize("warm", [True, False])
def test_the_call_changes_nothing(hip, case, warm):
    ds = instances_of(case)
    if case == "bordered circle":
        ds2 = [dict(d, g=d["g"] * (1.0 + 0.02 * np.random.default_rng(300 + b).standard_normal(d["nV"]))) for b, d in enumerate(ds)]
    else:
        ds2 = [moved(d, 300 + b) for b, d in enumerate(ds)]
    opt = hip.default_options(**OPT)
    out = []
    for with_call in (True, False):
        with environment(CASES[case][1]):
            sb = handle(hip, ds, opt)
        sb.run()
        first = result(sb)
        if with_call:
            counts = sb.launch_counts()
            got = sb.sensitivity(np.random.default_rng(1).standard_normal((len(ds), 2, ds[0]["nV"])))
            assert np.any(got[0] != 0.0)
            assert sb.launch_counts() == counts
            assert_same_bits(first, result(sb))      # the stored solution and statistics are the ones of the run
        update_all(sb, ds2)
        sb.resolve(warm=warm)
        out.append(result(sb))
        assert sb.launch_counts() == (1, 2)
        sb.close()
    assert_same_bits(out[0], out[1])


def test_buffers_grow_from_a_live_allocation(hip):
    ds = instances(SMALL, 2)

    def solved():
        sb = handle(hip, ds, hip.default_options(**OPT))
        sb.run()
        return sb
    grown_and_fresh(solved, np.random.default_rng(77).standard_normal((2, 3, SMALL[0])))


# ---- 6: state errors and a failed instance -------------------------------------------------------------------------------------------
def test_state_errors(hip):
    L = hip.lib()
    ds = instances(SMALL, 2)
    n = SMALL[0]
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.ones((2, n)); dg = np.full((2, n), 7.0)
    d = ds[0]
    sb = hip.SparseBatchLCQP(2, d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(**OPT))
    call = lambda: L.lcqp_hip_sparse_sensitivity(sb.h, 1, v.ctypes.data_as(dp), dg.ctypes.data_as(dp), None, None, None)
    load = lambda: sb.load(0, 2, np.stack([q["Q"].data for q in ds]), np.stack([q["g"] for q in ds]), np.stack([q["E"].data for q in ds]),
                           lbA=np.stack([q["lbA"] for q in ds]), ubA=np.stack([q["ubA"] for q in ds]))
    assert call() == NOT_SETUP                      # before anything
    assert load() == 0
    assert call() == NOT_SETUP and np.all(dg == 7.0)      # loaded, never run
    sb.run()
    assert call() == 0 and not np.any(dg == 7.0)
    update_all(sb, [moved(q, 9 + b) for b, q in enumerate(ds)])
    sb.resolve(warm=True)
    assert call() == 0                              # re-solves keep the mark
    assert load() == 0                              # a load since the last solve: the stored state belongs to other data
    assert call() == NOT_SETUP
    sb.run()
    assert call() == 0
    sb.set_options(hip.default_options(**OPT))
    assert call() == NOT_SETUP
    with pytest.raises(RuntimeError, match="300"):
        sb.sensitivity(v)
    sb.close()


def test_flag_of_a_failed_instance(hip):
    """Two instances of the six are given bad data.  Instance 4 gets a NaN in g: no trial of its polish is ever accepted and its run ends
    with LCQP_SUBPROBLEM_SOLVER_ERROR (203).  Instance 2 gets lbA > ubA on every row of A, the recipe the feature request names for a failing
    run -- but this arm's subsolver never looks at the other bound of a row it holds at one, and the run returns 0 (measured on one
    MI355X: return values [0, 0, 0, 0, 203, 0]; the same with one row, with a gap of 100 and with both bounds swapped), so for that
    instance the test can only hold the flag to the return value.  The neighbours are held to the bits of the batch without bad data."""
    c = solved_case("small")
    ds = list(c["ds"])
    crossed, bad = 2, 4
    ds[crossed] = dict(ds[crossed], lbA=ds[crossed]["ubA"] + 1.0)
    g = ds[bad]["g"].copy(); g[0] = np.nan
    ds[bad] = dict(ds[bad], g=g)
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    st = sb.solution()[2]
    dg, db, side, info = sb.sensitivity(c["V"])
    sb.close()
    print("  return values", [s["returnValue"] for s in st], "info", info)
    assert st[bad]["returnValue"] != 0 and all(st[b]["returnValue"] == 0 for b in range(len(ds)) if b not in (bad, crossed))
    assert bool(info[crossed] & 1) == (st[crossed]["returnValue"] != 0)
    for b in (bad, crossed):
        if st[b]["returnValue"] != 0:
            assert info[b] & 1
            assert np.all(dg[b] == 0.0) and np.all(db[b] == 0.0) and np.all(side[b] == 0)
    for b in range(len(ds)):      # the neighbours: the bits of the batch in which every instance solved
        if b not in (bad, crossed):
            assert info[b] == 0 and np.array_equal(dg[b], c["dg"][b]) and np.array_equal(db[b], c["db"][b]) and np.array_equal(side[b], c["side"][b])


# ---- 7: torch ------------------------------------------------------------------------------------------------------------------------
def test_torch_layer(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 4
    n, nC, nK = shape
    opt = hip.default_options(**OPT)
    ds = instances(shape, B)
    stack = lambda k: np.stack([d[k] for d in ds])
    sb = handle(hip, ds, opt)
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack("lbA"), ubA=stack("ubA")))
    rng = np.random.default_rng(9)
    w = rng.standard_normal((B, n))
    g = torch.tensor(stack("g"), dtype=torch.float64, requires_grad=True)
    x = layer(g)
    assert x.dtype == torch.float64 and x.shape == (B, n) and x.device == g.device
    assert sb.launch_counts() == (1, 1) and all(s["returnValue"] == 0 for s in layer.stats)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # every instance is differentiable: no warning
        (torch.as_tensor(w) * x).sum().backward()
    dg, db, side, info = sb.sensitivity(w)
    assert np.all(info == 0) and np.array_equal(g.grad.numpy(), dg)
    lam_min = np.array([np.linalg.eigvalsh(d["Q"].toarray())[0] for d in ds])
    bound = opt.stationarityTolerance * np.abs(w).sum(axis=1) / (H_FD * lam_min)
    g0 = g.detach()
    for k in range(5):
        z = torch.as_tensor(rng.standard_normal((B, n)))
        vals, keep = [], np.ones(B, dtype=bool)
        for sgn in (+1.0, -1.0):
            with torch.no_grad():
                xs = layer(g0 + sgn * H_FD * z)
            vals.append((torch.as_tensor(w) * xs).sum(dim=1).numpy())
            keep &= np.all(sb.sensitivity(w)[2] == side, axis=1)
        fd = (vals[0] - vals[1]) / (2 * H_FD)
        pred = (g.grad * z).sum(dim=1).numpy()
        err = np.abs(fd - pred)
        print(f"  direction {k}: err {err}, bound {bound}, W kept {keep}")
        assert np.all(keep) and np.all(err <= bound)
    assert sb.launch_counts() == (1, 11)      # one setup; every later forward is update + warm resolve
    # gradients with respect to the bounds, and the one warning that counts flagged instances
    lbA = torch.tensor(stack("lbA"), dtype=torch.float64, requires_grad=True)
    ubA = torch.tensor(stack("ubA"), dtype=torch.float64, requires_grad=True)
    x = layer(g0, lbA, ubA)
    (torch.as_tensor(w) * x).sum().backward()
    dg, db, side, info = sb.sensitivity(w)
    parts = hip.split_bound_derivatives(db, side, n, nC, nK, sparse=True)
    assert np.array_equal(lbA.grad.numpy(), parts["dlbA"]) and np.array_equal(ubA.grad.numpy(), parts["dubA"])
    assert np.count_nonzero(parts["dlbA"]) + np.count_nonzero(parts["dubA"]) == np.count_nonzero(side[:, :nC]) > 0
    sb.close()


def test_torch_layer_warns_about_flagged_instances(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    ds = instances(SMALL, 3)
    g1 = ds[1]["g"].copy(); g1[0] = np.nan      # no trial of this instance's polish is accepted: its run fails (test_flag_of_a_failed_instance)
    ds[1] = dict(ds[1], g=g1)
    stack = lambda k: np.stack([d[k] for d in ds])
    sb = handle(hip, ds, hip.default_options(**OPT))
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack("lbA"), ubA=stack("ubA")))
    g = torch.tensor(stack("g"), dtype=torch.float64, requires_grad=True)
    x = layer(g)
    with pytest.warns(RuntimeWarning, match="of 3 instances") as rec:
        x.sum().backward()
    assert len(rec) == 1
    assert layer.info[1] & 1 and not (layer.info[0] & 1) and not (layer.info[2] & 1) and torch.all(g.grad[1] == 0)
    sb.close()
