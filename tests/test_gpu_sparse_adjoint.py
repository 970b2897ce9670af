"""The full adjoint of the sparse arm (lcqp_hip_sparse_adjoint, SparseBatchLCQPLayer.solve; DESIGN.md section 3a''''): upstream gradients on x
AND y, gradients in g, the bounds and the stored entries of Q and E = [A; L; R].

Convention (include/lcqp_hip.h): Q x + g - E_W' y_W = 0, E_W x = b_W on the working set W, y as the solution call returns it.  With
K0 = [[Q, E_W'], [E_W, 0]] the adjoint system is K0 [d; mu] = [v_x; -v_y|_W] (so E_W d = -v_y|_W), dg = -d, db_W = mu, entry (i, j) of Q:
(dg_i x_j + x_i dg_j) / 2, entry (r, j) of E: -(db_r x_j + y_r dg_j) on the rows of W.  Test 1 pins the convention by a numpy stationarity
check of the returned (x, y) on W, test 7 by central differences.  "y = 0 outside W" holds for the subsolver's multipliers; the returned y
has the penalty terms removed (y_L -= rho R x, y_R -= rho L x), so a row of L or R outside W carries -rho times the residual of its pair's
other side, a row of W at its bound 0: the check is |y_r| <= rho (|E_W x - b_W|_inf + 64 eps |E|_inf |x|_inf) there (the second term: the
rounding of the device's own E x), and exactly zero on the rows of A.

1  against numpy on the device's own working set (W from `side`); dg, db: b1 = 1e-12 (nV + |W|) cond_2(K0) max(|v_x|_inf, |v_y|_inf); a matrix
   entry alpha x_j + beta dg_j: b1 (|x|_inf + |y|_inf) + eps (|alpha x_j| + |beta dg_j|).  Rows outside W: exactly zero.
2  vy = None without matrices is sb.sensitivity to the bit; vy = 0 gives the same values; launch_counts unchanged.
3  E_W dg = +v_y|_W to b1 |E_W|_inf (the error of dg meets a row of E_W: its 1-norm); the entries (i, j) and (j, i) of dQx equal to the bit;
   linearity in (v_x, v_y); other junk in v_y outside W: the same bits.
4  reduce: two calls give the same bits; equal to the float64 sum over the instances within (B - 1) eps/2 sum_b |term_b|; a failed instance
   adds zero.      5  chunking: one instance per chunk gives the unchunked bits.      6  the call changes nothing.
7  central differences, h = 1e-6, of l = v_x.x + v_y.y along a random symmetric Z_Q and a random Z_E on the patterns, on fresh handles loaded
   with the values +- h Z and started from the unperturbed solution at its final penalty.  Bounds: the ones derived in the docstring of
   tests/test_gpu_adjoint.py (x part tol |v_x|_1 / (h lambda_min(Q)), y part tol sqrt(nV cond_2(Q)) |v_y|_W|_1 / (h sigma_min(E_W)),
   tol = stationarityTolerance).  EVERY instance must keep its working set at both offsets: asserted, none skipped.  Unshifted lbL = lbR = 0.
   Seeds of the directions: default_rng(FD_SEED[shape]); checked on the CPU oracle (tests/oracle_py.py sparse_lcqp_solve, warm from the
   unperturbed solution, the same +- h Z): seeds 6, 7, 8 for SMALL with B = 4 and for MID with B = 2 -- all of them keep every working set
   (active rows by value at 1e-9) under Z_Q and under Z_E; the first one is used.
8  state errors.      9  torch: SparseBatchLCQPLayer.solve.

Cases: the ones of tests/test_gpu_sparse_sensitivity.py (they reach every engine) and one more SMALL case with three instances, an odd
count under the sum.  Every figure is printed before it is asserted."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import problems as P
from batch_helpers import assert_same_bits, environment, handle, result, stack, update_all
from problems import MID, OPT, SMALL, circle_instances, instances, moved
from test_gpu_adjoint import fd_bounds, kkt_adjoint_reference
from test_gpu_sparse_sensitivity import CASES as SENSITIVITY_CASES

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
H_FD = 1e-6
NOT_SETUP, INVALID_ARGUMENT = 300, 100
LAUNCH_BLOCK = 256      # threads of a workgroup of k_sparse_adjoint_nnz / k_sparse_adjoint_reduce
FD_SEED = {SMALL: 6, MID: 6}
CASES = dict(SENSITIVITY_CASES, **{"small, three": (("synth", SMALL, 3), {})})


def instances_of(key):
    (kind, shape, B), _ = CASES[key]
    if kind == "synth":
        return instances(shape, B)
    if kind == "circle":
        return circle_instances(B)
    d = P.grid_lcqp(*shape)
    d["Q"].sort_indices(); d["E"].sort_indices()
    return [dict(d) for _ in range(B)]


def coordinates(M):
    """(row, column) of every stored entry of a scipy CSC matrix, in the order of its value array"""
    return np.asarray(M.indices), np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))


def transposed_entry(Q):
    """for every stored entry (i, j) of the symmetric pattern of Q (CSC) the position of entry (j, i)"""
    import scipy.sparse as sp
    K = sp.csc_matrix((np.arange(1, Q.nnz + 1, dtype=np.float64), Q.indices, Q.indptr), shape=Q.shape).T.tocsc()
    K.sort_indices()
    assert np.array_equal(K.indptr, Q.indptr) and np.array_equal(K.indices, Q.indices)
    return K.data.astype(np.int64) - 1


def matrix_gradients(d, x, y, dg, db, inW):
    """the formulas of the header in numpy on the stored entries: (dQx, dAx, their alpha x_j and beta dg_j terms)"""
    qi, qj = coordinates(d["Q"]); er, ej = coordinates(d["E"])
    aq, bq = 0.5 * dg[qi], 0.5 * x[qi]
    ae, be = -db[er] * inW[er], -y[er] * inW[er]
    tq = (aq * x[qj], bq * dg[qj]); te = (ae * x[ej], be * dg[ej])
    return tq[0] + tq[1], te[0] + te[1], tq, te


@functools.lru_cache(maxsize=None)
def solved_case(key):
    """one solve per case and every adjoint call the tests 1 - 5 compare"""
    import lcqpow_amd as hip
    ds = instances_of(key)
    B, n, m = len(ds), ds[0]["nV"], ds[0]["nC"] + 2 * ds[0]["nComp"]
    with environment(CASES[key][1]):
        sb = handle(hip, ds, hip.default_options(**OPT))
    c = dict(ds=ds, engine=dict(lanes=sb.lanes(), fronts=sb.fronts(), border=sb.border()), nnz=(sb.nnzQ, sb.nnzA), alpha=0.7)
    sb.run()
    c["x"], c["y"], c["st"] = sb.solution()
    rng = np.random.default_rng(78)
    vx, vy, vx2, vy2 = rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, n)), rng.standard_normal((B, m))
    c.update(vx=vx, vy=vy, v2=(vx2, vy2))
    counts = sb.launch_counts()
    c["full"] = sb.adjoint(vx, vy)
    c["ms"] = sb.sensitivity_kernel_ms()
    c["chunked"] = sb.adjoint(vx, vy, _staging_bytes=1)
    c["red"] = sb.adjoint(vx, vy, reduce=True)
    c["red_ms"] = sb.sensitivity_kernel_ms()
    c["red2"] = sb.adjoint(vx, vy, reduce=True)
    c["some"] = sb.adjoint(vx, vy, matrices=("A",), reduce=True)
    c["sens"] = sb.sensitivity(vx)
    c["plain"] = sb.adjoint(vx, None, matrices=())
    c["zero"] = sb.adjoint(vx, np.zeros((B, m)), matrices=())
    c["second"] = sb.adjoint(vx2, vy2)
    c["lin"] = sb.adjoint(c["alpha"] * vx + vx2, c["alpha"] * vy + vy2)
    junk = vy.copy()
    outside = c["full"]["side"] == 0
    junk[outside] = 1e30 * rng.standard_normal(np.count_nonzero(outside))
    if np.any(outside):
        junk[tuple(np.argwhere(outside)[0])] = np.nan
    c["junk"] = sb.adjoint(vx, junk)
    assert sb.launch_counts() == counts
    sb.close()
    return c


@functools.lru_cache(maxsize=None)
def reference_of(key):
    c = solved_case(key)
    out = []
    for b, d in enumerate(c["ds"]):
        E = d["E"].toarray()
        W = np.flatnonzero(c["full"]["side"][b])
        dg, mu, cond = kkt_adjoint_reference(d["Q"].toarray(), E[W], c["vx"][b], c["vy"][b][W], extended=True)
        out.append(dict(E=E, W=W, dg=dg, mu=mu, cond=cond))
    return out


def bound_1(c, r, b, vx=None, vy=None):
    vx = c["vx"][b] if vx is None else vx
    vy = c["vy"][b] if vy is None else vy
    return 1e-12 * (c["ds"][b]["nV"] + len(r["W"])) * r["cond"] * max(np.abs(vx).max(), np.abs(vy).max())


def test_the_cases_reach_every_engine_and_the_ragged_sizes(hip):
    eng = {k: solved_case(k)["engine"] for k in ("small", "lanes 32", "mid, general ldl", "grid, general ldl", "bordered circle")}
    print(" ", eng)
    assert eng["small"]["lanes"] == 8 and eng["lanes 32"]["lanes"] == 32
    assert eng["mid, general ldl"]["fronts"] > 0 and eng["grid, general ldl"]["fronts"] > 4 and eng["grid, general ldl"]["lanes"] == 64
    assert eng["bordered circle"]["border"] > 0
    sizes = {k: (len(solved_case(k)["ds"]),) + solved_case(k)["nnz"] for k in CASES}
    print(" ", sizes)
    assert any(q % 2 or a % 2 for _, q, a in sizes.values())                                                  # an odd number of entries
    assert any((B * q) % LAUNCH_BLOCK or (B * a) % LAUNCH_BLOCK for B, q, a in sizes.values())                # a ragged last workgroup
    assert any(B % 2 for B, _, _ in sizes.values())


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_against_numpy_on_the_working_set(hip, key):
    import lcqpow_amd
    c, refs = solved_case(key), reference_of(key)
    f = c["full"]
    tol = lcqpow_amd.default_options(**OPT).stationarityTolerance
    m = f["side"].shape[1]
    print(f"  {key}: kernels of the per-instance call {c['ms']:.3f} ms, of the reduced call {c['red_ms']:.3f} ms")
    for b, (d, r) in enumerate(zip(c["ds"], refs)):
        x, y, W = c["x"][b], c["y"][b], r["W"]
        assert c["st"][b]["returnValue"] == 0 and not (f["info"][b] & 1)
        inW = np.zeros(m, dtype=bool); inW[W] = True
        # the convention: the returned pair is stationary on W with THIS sign of y, and carries nothing outside W
        stat = np.abs(d["Q"] @ x + d["g"] - r["E"][W].T @ y[W]).max()
        stat_bound = tol * (1.0 + np.abs(d["g"]).max())
        wrong = np.abs(d["Q"] @ x + d["g"] + r["E"][W].T @ y[W]).max()
        # outside W the subsolver's multiplier is exactly zero; the returned y is that minus the penalty term rho (R x)_i resp. rho (L x)_i
        # of the pair, whose other side is a row of W at its bound 0 (no open pair: info bit 8 is clear): rho times the residual of W
        nC, nK = d["nC"], d["nComp"]
        lo = np.concatenate([d["lbA"], np.zeros(2 * nK)]); hi = np.concatenate([d["ubA"], np.full(2 * nK, np.inf)])
        ex = r["E"] @ x
        res_W = np.abs(ex[W] - np.where(f["side"][b][W] == 1, hi[W], lo[W])).max(initial=0.0)
        y_bound = c["st"][b]["rhoOpt"] * (res_W + 64 * EPS * np.abs(r["E"]).sum(axis=1).max() * np.abs(x).max())
        y_out = np.abs(y[~inW]).max(initial=0.0); y_out_A = np.abs(y[:nC][~inW[:nC]]).max(initial=0.0)
        print(f"  {key} instance {b}: |Q x + g - E_W'y_W| {stat:.3g} (bound {stat_bound:.3g}; with the other sign {wrong:.3g}), |y| outside W {y_out:.3g} "
              f"(rows of A {y_out_A:.3g}; |E_W x - b_W| {res_W:.3g}, rho {c['st'][b]['rhoOpt']:.3g}, bound {y_bound:.3g})")
        assert stat <= stat_bound and y_out_A == 0.0 and y_out <= y_bound and not (f["info"][b] & 8)
        b1 = bound_1(c, r, b)
        dbr = np.zeros(m); dbr[W] = r["mu"]
        e_g = np.abs(f["dg"][b] - r["dg"]).max(); e_b = np.abs(f["db"][b] - dbr).max()
        refQ, refE, tq, te = matrix_gradients(d, x, y, r["dg"], dbr, inW)
        xy = np.abs(x).max() + np.abs(y).max()
        bq = b1 * xy + EPS * (np.abs(tq[0]) + np.abs(tq[1])); be = b1 * xy + EPS * (np.abs(te[0]) + np.abs(te[1]))
        rq = (np.abs(f["Q"][b] - refQ) / bq).max(); re = (np.abs(f["A"][b] - refE) / be).max()
        print(f"  {key} instance {b}: |W| = {len(W)}, cond(K0) = {r['cond']:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {b1:.3g}; "
              f"worst error / bound on the entries of Q {rq:.3g}, of E {re:.3g}; info {f['info'][b]}")
        assert e_g <= b1 and e_b <= b1 and rq <= 1.0 and re <= 1.0
        rows = coordinates(d["E"])[0]
        assert np.all(f["db"][b][~inW] == 0.0) and np.all(f["A"][b][~inW[rows]] == 0.0)
        assert np.any(f["Q"][b] != 0.0) and np.any(f["A"][b][inW[rows]] != 0.0)
        if key == "bordered circle":
            assert (f["info"][b] & ~4) == 0
        else:
            assert f["info"][b] == 0


# ---- 2: without vy and matrices the call is lcqp_hip_sparse_sensitivity ------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_plain_call_is_the_sensitivity_call(hip, key):
    c = solved_case(key)
    for name, got in zip(("dg", "db", "side", "info"), c["sens"]):
        same = c["plain"][name].tobytes() == got.tobytes(); zero = np.array_equal(c["zero"][name], got)
        print(f"  {key} {name}: vy = None equal to sensitivity to the bit: {same}; vy = 0 equal in value: {zero}")
        assert same and zero
    assert sorted(c["plain"]) == ["db", "dg", "info", "side"]
    assert np.any(c["full"]["dg"] != c["plain"]["dg"])      # and vy does enter


# ---- 3: structure -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_structure(hip, key):
    c, refs = solved_case(key), reference_of(key)
    f, a = c["full"], c["alpha"]
    t = transposed_entry(c["ds"][0]["Q"])
    assert f["Q"].tobytes() == f["Q"][:, t].tobytes() and c["red"]["Q"].tobytes() == c["red"]["Q"][t].tobytes()
    for k in f:      # junk in vy outside W changes no bit
        assert c["junk"][k].tobytes() == f[k].tobytes(), k
    for b, r in enumerate(refs):
        EW, W = r["E"][r["W"]], r["W"]
        b1 = bound_1(c, r, b)
        res = (np.abs(EW @ f["dg"][b] - c["vy"][b][W]) / np.abs(EW).sum(axis=1)).max(initial=0.0)
        vx2, vy2 = c["v2"][0][b], c["v2"][1][b]
        tol = bound_1(c, r, b, a * c["vx"][b] + vx2, a * c["vy"][b] + vy2) + a * b1 + bound_1(c, r, b, vx2, vy2)
        lin = max(np.abs(c["lin"][k][b] - (a * f[k][b] + c["second"][k][b])).max() for k in ("dg", "db"))
        xy = np.abs(c["x"][b]).max() + np.abs(c["y"][b]).max()
        linm = max(np.abs(c["lin"][k][b] - (a * f[k][b] + c["second"][k][b])).max() for k in ("Q", "A"))
        print(f"  {key} instance {b}: |E_r dg - vy_r| / |E_r|_1 {res:.3g} (bound {b1:.3g}), linearity dg, db {lin:.3g} (tol {tol:.3g}), "
              f"entries {linm:.3g} (tol {tol * xy:.3g})")
        assert res <= b1 and lin <= tol and linm <= tol * xy


# ---- 4: the sums over the batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_reduce(hip, key):
    c = solved_case(key)
    B = len(c["ds"])
    for k in ("Q", "A"):
        assert c["red"][k].tobytes() == c["red2"][k].tobytes()
        terms = c["full"][k]
        assert c["red"][k].shape == terms.shape[1:]
        want = terms.sum(axis=0)
        bound = (B - 1) * 0.5 * EPS * np.abs(terms).sum(axis=0)
        err = np.abs(c["red"][k] - want)
        ratio = (err[bound > 0] / bound[bound > 0]).max(initial=0.0)
        print(f"  {key} d{k}x: worst |reduce - sum| {err.max(initial=0.0):.3g}, worst error / bound {ratio:.3g}, zero-bound entries {np.count_nonzero(bound == 0)}")
        assert np.all(err <= bound)
    assert c["some"]["A"].tobytes() == c["red"]["A"].tobytes() and "Q" not in c["some"]
    for name in ("dg", "db", "side", "info"):
        assert np.array_equal(c["red"][name], c["full"][name])


def test_reduce_skips_a_failed_instance(hip):
    """a NaN in g of instance 1: its run ends with 203 (tests/test_gpu_sparse_sensitivity.py::test_flag_of_a_failed_instance)"""
    ds = instances(SMALL, 3)
    g1 = ds[1]["g"].copy(); g1[0] = np.nan
    ds[1] = dict(ds[1], g=g1)
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    st = sb.solution()[2]
    rng = np.random.default_rng(3)
    vx, vy = rng.standard_normal((3, SMALL[0])), rng.standard_normal((3, SMALL[1] + 2 * SMALL[2]))
    f = sb.adjoint(vx, vy); r = sb.adjoint(vx, vy, reduce=True)
    sb.close()
    print("  return values", [s["returnValue"] for s in st], "info", f["info"])
    assert st[0]["returnValue"] == 0 and st[1]["returnValue"] == 203 and st[2]["returnValue"] == 0
    assert f["info"][1] & 1 and not (f["info"][0] & 1) and not (f["info"][2] & 1)
    for k in ("Q", "A"):
        assert np.all(f[k][1] == 0.0) and np.all(np.isfinite(r[k]))
        assert np.array_equal(r[k], f[k][0] + f[k][2])
    assert np.any(r["Q"] != 0.0) and np.any(r["A"] != 0.0)


# ---- 5: chunking ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_chunks_of_one_instance_give_the_same_bits(hip, key):
    c = solved_case(key)
    for k in c["full"]:
        assert c["chunked"][k].tobytes() == c["full"][k].tobytes(), k


# ---- 6: no side effects ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "mid, general ldl", "bordered circle"])
@pytest.mark.parametrize("warm", [True, False])
def test_the_call_changes_nothing(hip, case, warm):
    ds = instances_of(case)
    if case == "bordered circle":
        ds2 = [dict(d, g=d["g"] * (1.0 + 0.02 * np.random.default_rng(300 + b).standard_normal(d["nV"]))) for b, d in enumerate(ds)]
    else:
        ds2 = [moved(d, 300 + b) for b, d in enumerate(ds)]
    opt = hip.default_options(**OPT)
    B, n, m = len(ds), ds[0]["nV"], ds[0]["nC"] + 2 * ds[0]["nComp"]
    out = []
    for with_call in (True, False):
        with environment(CASES[case][1]):
            sb = handle(hip, ds, opt)
        sb.run()
        first = result(sb)
        if with_call:
            counts = sb.launch_counts()
            rng = np.random.default_rng(1)
            vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, m))
            got = sb.adjoint(vx, vy); sb.adjoint(vx, vy, reduce=True); sb.adjoint(vx, vy, _staging_bytes=1)
            assert np.any(got["Q"] != 0.0)
            assert sb.launch_counts() == counts
            assert_same_bits(first, result(sb))      # the stored solution and statistics are the ones of the run
        update_all(sb, ds2)
        sb.resolve(warm=warm)
        out.append(result(sb))
        assert sb.launch_counts() == (1, 2)
        sb.close()
    assert_same_bits(out[0], out[1])


# ---- 7: central differences -----------------------------------------------------------------------------------------------------------
def directions(rng, d):
    """a random symmetric Z_Q on the pattern of Q and a random Z_E on the pattern of E, as value arrays in the CSC order of the patterns"""
    zq = rng.standard_normal(d["Q"].nnz)
    zq = 0.5 * (zq + zq[transposed_entry(d["Q"])])
    return zq, rng.standard_normal(d["E"].nnz)


def with_values(d, qx, ex):
    import scipy.sparse as sp
    Q = sp.csc_matrix((qx, d["Q"].indices, d["Q"].indptr), shape=d["Q"].shape)
    E = sp.csc_matrix((ex, d["E"].indices, d["E"].indptr), shape=d["E"].shape)
    return dict(d, Q=Q, E=E)


@pytest.mark.parametrize("shape,B", [(SMALL, 4), (MID, 2)])
def test_central_differences(hip, shape, B):
    n, nC, nK = shape
    m = nC + 2 * nK
    opt = hip.default_options(**OPT)
    ds = instances(shape, B)
    sb = handle(hip, ds, opt)
    sb.run()
    x0, y0, st = sb.solution()
    assert all(s["returnValue"] == 0 for s in st)
    rng = np.random.default_rng(FD_SEED[shape])
    vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    r = sb.adjoint(vx, vy)
    sb.close()
    assert np.all(r["info"] == 0)
    Z = [directions(rng, d) for d in ds]
    bounds = []
    for b, d in enumerate(ds):
        W = np.flatnonzero(r["side"][b])
        bounds.append(sum(fd_bounds(opt.stationarityTolerance, d["Q"].toarray(), d["E"].toarray()[W], vx[b], vy[b][W])))
    # the perturbed solves start at the unperturbed solution, at its final penalty: one batch per penalty value (the options are per batch)
    groups = {}
    for b in range(B):
        groups.setdefault(st[b]["rhoOpt"], []).append(b)
    print(f"  {shape}: penalties {sorted(groups)} -> instances {[groups[k] for k in sorted(groups)]}")

    def perturbed_solves(which, sgn):
        val, keep = np.zeros(B), np.zeros(B, dtype=bool)
        for rho, members in groups.items():
            o = hip.default_options(solveZeroPenaltyFirst=0, initialPenaltyParameter=rho, **OPT)
            dp = [with_values(ds[b], ds[b]["Q"].data + (sgn * H_FD * Z[b][0] if which == "Q" else 0.0),
                              ds[b]["E"].data + (sgn * H_FD * Z[b][1] if which == "A" else 0.0)) for b in members]
            dp = [dict(d, x0=x0[b], y0=y0[b]) for d, b in zip(dp, members)]
            bs = handle(hip, dp, o)
            bs.run()
            xs, ys, sts = bs.solution()
            side = bs.sensitivity(vx[members])[2]
            bs.close()
            for i, b in enumerate(members):
                keep[b] = sts[i]["returnValue"] == 0 and np.array_equal(side[i], r["side"][b])
                val[b] = vx[b] @ xs[i] + vy[b] @ ys[i]
        return val, keep

    for which, zi in (("Q", 0), ("A", 1)):
        vp, kp = perturbed_solves(which, +1.0); vm, km = perturbed_solves(which, -1.0)
        keep = kp & km
        fd = (vp - vm) / (2 * H_FD)
        pred = np.array([np.sum(r[which][b] * Z[b][zi]) for b in range(B)])
        err = np.abs(fd - pred)
        for b in range(B):
            print(f"  {shape} d{which}x instance {b}: fd {fd[b]:+.9e} predicted {pred[b]:+.9e} err {err[b]:.3g} "
                  f"(rel {err[b] / max(abs(pred[b]), 1e-300):.3g}) bound {bounds[b]:.3g} W kept {bool(keep[b])}")
        assert np.all(keep)                        # every instance keeps W at both offsets: none is skipped
        assert np.all(err <= np.array(bounds))


# ---- 8: state errors ------------------------------------------------------------------------------------------------------------------
def test_state_errors(hip):
    L = hip.lib()
    ds = instances(SMALL, 2)
    n, m = SMALL[0], SMALL[1] + 2 * SMALL[2]
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.ones((2, n)); dg = np.full((2, n), 7.0); dQx = np.full((2, ds[0]["Q"].nnz), 7.0)
    d = ds[0]
    sb = hip.SparseBatchLCQP(2, d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(**OPT))
    call = lambda reduce=0: L.lcqp_hip_sparse_adjoint(sb.h, v.ctypes.data_as(dp), None, dg.ctypes.data_as(dp), None, None, None, reduce,
                                                      dQx.ctypes.data_as(dp), None)
    load = lambda: sb.load(0, 2, np.stack([q["Q"].data for q in ds]), np.stack([q["g"] for q in ds]), np.stack([q["E"].data for q in ds]),
                           lbA=np.stack([q["lbA"] for q in ds]), ubA=np.stack([q["ubA"] for q in ds]))
    assert call() == NOT_SETUP                      # before anything
    assert load() == 0
    assert call() == NOT_SETUP and np.all(dg == 7.0) and np.all(dQx == 7.0)      # loaded, never run
    assert call(2) == INVALID_ARGUMENT and call(-1) == INVALID_ARGUMENT          # the arguments come first
    sb.run()
    assert call(2) == INVALID_ARGUMENT and np.all(dg == 7.0)
    assert call() == 0 and not np.any(dg == 7.0) and not np.any(dQx == 7.0)
    assert call(1) == 0
    assert load() == 0                              # a load since the last solve: the stored state belongs to other data
    assert call() == NOT_SETUP
    sb.run()
    assert call() == 0
    sb.set_options(hip.default_options(**OPT))
    assert call() == NOT_SETUP
    with pytest.raises(RuntimeError, match="300"):
        sb.adjoint(v)
    sb.run()
    assert call() == 0
    # a FACTOR probe overwrites the stored polish factor
    N = n + m
    sb.kkt_probe(np.ones((2, 1, N)), dprim=np.full(2, 1e-6), ddual=np.full((2, m), 1e-6), use=np.ones((2, m), dtype=np.int32))
    assert call() == NOT_SETUP
    with pytest.raises(ValueError, match="reduce|matrices|unknown"):
        sb.adjoint(v, matrices=("L",))
    sb.close()


# ---- 9: torch ------------------------------------------------------------------------------------------------------------------------
def test_torch_solve(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 4
    n, nC, nK = shape
    m = nC + 2 * nK
    opt = hip.default_options(**OPT)
    ds = instances(shape, B)
    ds = [dict(d, E=ds[0]["E"]) for d in ds]      # one E for the batch; Q, g and the bounds differ
    sb = handle(hip, ds, opt)
    Qx0, Ax0 = np.stack([d["Q"].data for d in ds]), ds[0]["E"].data
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")), values=dict(Qx=Qx0, Ax=Ax0))
    T = lambda a, grad=True: torch.tensor(a, dtype=torch.float64, requires_grad=grad)
    g, Qx, Ax = T(stack(ds, "g")), T(Qx0), T(Ax0)
    rng = np.random.default_rng(FD_SEED[shape])
    wx, wy = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    loss = lambda x, y: (torch.as_tensor(wx) * x).sum() + (torch.as_tensor(wy) * y).sum()
    x, y = layer.solve(g, Qx=Qx, Ax=Ax)
    assert x.shape == (B, n) and y.shape == (B, m) and x.dtype == torch.float64 and all(s["returnValue"] == 0 for s in layer.stats)
    xs, ys, st = sb.solution()
    assert np.array_equal(x.detach().numpy(), xs) and np.array_equal(y.detach().numpy(), ys)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        loss(x, y).backward()
    each = sb.adjoint(wx, wy, matrices=("Q",)); summed = sb.adjoint(wx, wy, matrices=("A",), reduce=True)
    assert np.all(each["info"] == 0)
    assert Qx.grad.shape == (B, sb.nnzQ) and Ax.grad.shape == (sb.nnzA,)
    assert np.array_equal(Qx.grad.numpy(), each["Q"]) and np.array_equal(Ax.grad.numpy(), summed["A"]) and np.array_equal(g.grad.numpy(), each["dg"])
    assert np.any(each["Q"] != 0.0) and np.any(summed["A"] != 0.0)
    # five random directions by central differences through the layer: a symmetric Z_Q per instance, one Z_E for the shared array
    side = each["side"]
    bound = 0.0
    for b, d in enumerate(ds):
        W = np.flatnonzero(side[b])
        bound += sum(fd_bounds(opt.stationarityTolerance, d["Q"].toarray(), d["E"].toarray()[W], wx[b], wy[b][W]))
    for k in range(5):
        zq = np.stack([directions(rng, d)[0] for d in ds]); ze = rng.standard_normal(sb.nnzA)
        vals, keep = [], np.ones(B, dtype=bool)
        for sgn in (+1.0, -1.0):
            with torch.no_grad():
                xp, yp = layer.solve(g.detach(), Qx=T(Qx0 + sgn * H_FD * zq, False), Ax=T(Ax0 + sgn * H_FD * ze, False))
            vals.append(float(loss(xp, yp)))
            keep &= np.all(sb.sensitivity(wx)[2] == side, axis=1) & np.array([s["returnValue"] == 0 for s in layer.stats])
        fd = (vals[0] - vals[1]) / (2 * H_FD)
        pred = float(np.sum(each["Q"] * zq) + np.sum(summed["A"] * ze))
        print(f"  direction {k}: fd {fd:+.9e} predicted {pred:+.9e} err {abs(fd - pred):.3g} bound {bound:.3g} W kept {keep}")
        assert np.all(keep) and abs(fd - pred) <= bound
    # without value tensors: the update + resolve of __call__
    counts = sb.launch_counts()
    layer.solve(g.detach())
    assert sb.launch_counts() == (counts[0], counts[1] + 1)
    sb.close()


def test_torch_solve_needs_the_values(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    ds = instances(SMALL, 2)
    sb = handle(hip, ds, hip.default_options(**OPT))
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64)
    with pytest.raises(ValueError, match="values"):
        layer.solve(g, Qx=torch.tensor(ds[0]["Q"].data))
    x, y = layer.solve(g)      # without a matrix tensor nothing is missing
    assert x.shape == (2, SMALL[0]) and y.shape == (2, SMALL[1] + 2 * SMALL[2]) and sb.launch_counts() == (1, 1)
    sb.close()


def test_torch_solve_warns_about_flagged_instances(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    ds = instances(SMALL, 3)
    g1 = ds[1]["g"].copy(); g1[0] = np.nan
    ds[1] = dict(ds[1], g=g1)
    sb = handle(hip, ds, hip.default_options(**OPT))
    Qx0, Ax0 = np.stack([d["Q"].data for d in ds]), np.stack([d["E"].data for d in ds])
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")), values=dict(Qx=Qx0, Ax=Ax0))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64, requires_grad=True)
    Qx = torch.tensor(Qx0, dtype=torch.float64, requires_grad=True)
    x, y = layer.solve(g, Qx=Qx)
    with pytest.warns(RuntimeWarning, match="of 3 instances") as rec:
        (x.sum() + y.sum()).backward()
    assert len(rec) == 1
    assert layer.info[1] & 1 and not (layer.info[0] & 1) and torch.all(g.grad[1] == 0) and torch.all(Qx.grad[1] == 0)
    sb.close()
