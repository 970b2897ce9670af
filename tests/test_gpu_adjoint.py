"""The full adjoint of the dense arm (lcqp_hip_batch_adjoint / lcqp_hip_qp_adjoint, BatchLCQPLayer.solve; DESIGN.md section 3a''''):
upstream gradients on x AND y, gradients in g, the bounds and the matrices Q, A, L, R.

Convention (include/lcqp_hip.h): Q x + g - E_W' y_W = 0, E_W x = b_W on the working set W.  With K = [[Q, E_W'], [E_W, 0]] the adjoint system
is K [d; mu] = [v_x; -v_y|_W] (so E_W d = -v_y|_W), dg = -d, db_W = mu, dQ = (dg x' + x dg') / 2, row r of dA / dL / dR = -(db_r x + y_r dg).

1  against numpy on the device's own working set; bound for dg, db: 1e-12 nV cond_2(K) max(|v_x|_inf, |v_y|_inf) =: b1 (the form of test 1
   of tests/test_gpu_sensitivity.py); for a matrix entry alpha x_j + beta dg_j: b1 (|x|_inf + |y|_inf) -- the errors of dg and db times the
   factor they meet -- plus eps (|alpha x_j| + |beta dg_j|), one rounding of each product and of their sum.  Rows outside W: exactly zero.
2  vy = None without matrices is bt.sensitivity to the bit; vy = 0 gives the same values.
3  E_W dg = +v_y|_W; dQ symmetric to the bit; linearity in (v_x, v_y).
4  reduce: two calls give the same bits; equal to the float64 sum over the instances within B eps sum_b |term_b|; a failed instance adds zero.
5  chunking: one instance per chunk gives the unchunked bits.      6  the call changes nothing.
7  central differences, h = 1e-6, of l = v_x.x + v_y.y along random Z_Q (symmetric), Z_A, Z_L, Z_R on fresh objects loaded with M +- h Z.
   The x part has the bound of test 4 there: tol |v_x|_1 / (h lambda_min(Q)), tol = stationarityTolerance.  The y part: a returned pair with
   stationarity residual r = Q x + g - E_W' y, |r|_inf <= tol, and E_W x = b_W differs from the exact pair of its working set by (dx, dy) with
   Q dx - E_W' dy = r, E_W dx = 0.  So dx = P r with the Q-orthogonal projector's P = Z (Z'QZ)^-1 Z', and E_W' dy = -(I - Q P) r; I - Q P is
   an orthogonal projector in the inner product of Q^-1, hence |(I - Q P) r|_2 <= sqrt(cond_2(Q)) |r|_2 <= sqrt(cond_2(Q) nV) tol, and
   |dy|_2 <= that / sigma_min(E_W).  Two solves over 2h:  |error of the y part| <= tol sqrt(nV cond_2(Q)) |v_y|_W|_1 / (h sigma_min(E_W)).
   LCQP seeds 1000 .. 1007 of both shapes were checked on the CPU oracle (tests/oracle_py.py) to keep their active sets under these
   perturbations, started from the unperturbed solution.
8  torch: BatchLCQPLayer.solve.

Problems: tests/problems.py::random_lcqp with default_rng(1000 + instance).  Every figure is printed before it is asserted."""
import functools
import warnings

import numpy as np
import pytest

import problems as P
from batch_helpers import LD, assert_same_bits, load_all, result, stack, update_all
from problems import perturbed, random_lcqp
from test_gpu_sensitivity import rows_and_bounds, working_rows

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
H_FD = 1e-6
MATS = ("Q", "A", "L", "R")
#          n,  nC, nComp, B, box, shifted     path
SHAPES = {"np128": (40, 20, 8, 6, False, False),            # nV no multiple of 16
          "np128_three": (40, 20, 8, 3, False, False),      # an odd number of instances under the sum
          "np256_box": (200, 330, 37, 3, True, False),      # box rows in pos
          "np1024": (600, 200, 50, 2, True, True)}          # the large-size launch table


def problems_of(key):
    n, nC, nComp, B, box, shifted = SHAPES[key]
    return [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, box, shifted) for b in range(B)]


def kkt_adjoint_reference(Q, EW, vx, vyW, extended):
    """dg, mu of K [d; mu] = [vx; -vyW] (batch_helpers.kkt_reference with a second block in the right-hand side), and cond_2(K)"""
    n, m = Q.shape[0], EW.shape[0]
    K = np.zeros((n + m, n + m)); K[:n, :n] = Q; K[:n, n:] = EW.T; K[n:, :n] = EW
    rhs = np.concatenate([vx, -vyW])
    sol = np.linalg.solve(K, rhs)
    if extended:
        KL, rl, sl = K.astype(LD), rhs.astype(LD), sol.astype(LD)
        for _ in range(3):
            sl = sl + np.linalg.solve(K, (rl - KL @ sl).astype(np.float64)).astype(LD)
        sol = sl.astype(np.float64)
    ev = np.abs(np.linalg.eigvalsh(K))
    return -sol[:n], sol[n:], float(ev.max() / ev.min())


def stacked(r):
    """[dQ; dA; dL; dR] of an adjoint result: [..][nd][nV], row n + e belongs to row e of E = [A; L; R]"""
    return np.concatenate([r[k] for k in MATS], axis=-2)


@functools.lru_cache(maxsize=None)
def solved_case(key):
    """one solve per shape and every adjoint call the tests 1 - 5 compare"""
    import lcqpow_amd as hip
    n, nC, nComp, B, box, shifted = SHAPES[key]
    nd = n + nC + 2 * nComp
    ds = problems_of(key)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    bt.run()
    x, y, st = bt.solution()
    rng = np.random.default_rng(78)
    vx, vy, vx2, vy2 = rng.standard_normal((B, n)), rng.standard_normal((B, nd)), rng.standard_normal((B, n)), rng.standard_normal((B, nd))
    counts = bt.launch_counts()
    c = dict(ds=ds, x=x, y=y, st=st, vx=vx, vy=vy, alpha=0.7)
    c["full"] = bt.adjoint(vx, vy)
    c["ms"] = bt.sensitivity_kernel_ms()
    c["chunked"] = bt.adjoint(vx, vy, _staging_bytes=1)
    c["red"] = bt.adjoint(vx, vy, reduce=True)
    c["red_ms"] = bt.sensitivity_kernel_ms()
    c["red2"] = bt.adjoint(vx, vy, reduce=True)
    c["some"] = bt.adjoint(vx, vy, matrices=("A",), reduce=True)
    c["sens"] = bt.sensitivity(vx)
    c["plain"] = bt.adjoint(vx, None, matrices=())
    c["zero"] = bt.adjoint(vx, np.zeros((B, nd)), matrices=())
    c["second"] = bt.adjoint(vx2, vy2)
    c["lin"] = bt.adjoint(c["alpha"] * vx + vx2, c["alpha"] * vy + vy2)
    c["v2"] = (vx2, vy2)
    assert bt.launch_counts() == counts
    c["ws"] = [bt.read_working_set(b) for b in range(B)]
    bt.close()
    return c


@functools.lru_cache(maxsize=None)
def reference_of(key):
    c = solved_case(key)
    n = SHAPES[key][0]
    out = []
    for b, d in enumerate(c["ds"]):
        E, lo, hi, pos = rows_and_bounds(d)
        W = working_rows(c["ws"][b])
        dg, mu, cond = kkt_adjoint_reference(d["Q"], E[W], c["vx"][b], c["vy"][b][pos[W]], extended=n <= 512)
        out.append(dict(E=E, pos=pos, W=W, dg=dg, mu=mu, cond=cond))
    return out


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, nC, nComp, B = SHAPES[key][:4]
    nd = n + nC + 2 * nComp
    f = c["full"]
    print(f"  {key}: kernels of the per-instance call {c['ms']:.3f} ms, of the reduced call {c['red_ms']:.3f} ms")
    for b in range(B):
        r = refs[b]
        x, y = c["x"][b], c["y"][b]
        assert c["st"][b]["returnValue"] == 0 and not (f["info"][b] & 1)
        b1 = 1e-12 * n * r["cond"] * max(np.abs(c["vx"][b]).max(), np.abs(c["vy"][b]).max())
        dbr = np.zeros(nd); dbr[r["pos"][r["W"]]] = r["mu"]
        e_g = np.abs(f["dg"][b] - r["dg"]).max(); e_b = np.abs(f["db"][b] - dbr).max()
        inW = np.zeros(nd, dtype=bool); inW[r["pos"][r["W"]]] = True
        assert np.array_equal(f["side"][b] != 0, inW)
        # the matrix gradients from the reference's dg, db and the returned x, y
        alpha = np.concatenate([0.5 * r["dg"], -dbr[n:] * inW[n:]]); beta = np.concatenate([0.5 * x, -y[n:] * inW[n:]])
        ref = alpha[:, None] * x[None, :] + beta[:, None] * r["dg"][None, :]
        bm = b1 * (np.abs(x).max() + np.abs(y).max()) + EPS * (np.abs(alpha)[:, None] * np.abs(x)[None, :] + np.abs(beta)[:, None] * np.abs(r["dg"])[None, :])
        got = stacked(f)[b]
        ratio = (np.abs(got - ref) / bm).max()
        print(f"  {key} instance {b}: |W| = {len(r['W'])}, cond(K) = {r['cond']:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, bound {b1:.3g}; "
              f"matrices: worst error {np.abs(got - ref).max():.3g}, worst error / bound {ratio:.3g}, info {f['info'][b]}")
        assert e_g <= b1 and e_b <= b1 and ratio <= 1.0
        assert np.all(f["db"][b][~inW] == 0.0) and np.all(got[n:][~inW[n:]] == 0.0)
        assert np.any(got[:n] != 0.0) and np.any(got[n:][inW[n:]] != 0.0)


# ---- 2: without vy and matrices the call is lcqp_hip_batch_sensitivity -------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_plain_call_is_the_sensitivity_call(hip, key):
    c = solved_case(key)
    for name, got in zip(("dg", "db", "side", "info"), c["sens"]):
        same = np.array_equal(c["plain"][name], got); zero = np.array_equal(c["zero"][name], got)
        print(f"  {key} {name}: vy = None equal to sensitivity: {same}; vy = 0 equal in value: {zero}")
        assert same and zero
        assert c["plain"][name].tobytes() == got.tobytes()
    assert sorted(c["plain"]) == ["db", "dg", "info", "side"]
    assert np.any(c["full"]["dg"] != c["plain"]["dg"])      # and vy does enter


# ---- 3: structure -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_structure(hip, key):
    c, refs = solved_case(key), reference_of(key)
    n, nC, nComp, B = SHAPES[key][:4]
    f, a = c["full"], c["alpha"]
    assert np.array_equal(f["Q"], f["Q"].transpose(0, 2, 1)) and np.array_equal(c["red"]["Q"], c["red"]["Q"].T)
    for b in range(B):
        r = refs[b]
        EW = r["E"][r["W"]]
        vmax = lambda vx, vy: max(np.abs(vx).max(), np.abs(vy).max())
        err1 = lambda vx, vy: 1e-12 * n * r["cond"] * vmax(vx, vy)      # the bound of test 1
        b1 = err1(c["vx"][b], c["vy"][b])
        res = (np.abs(EW @ f["dg"][b] - c["vy"][b][r["pos"][r["W"]]]) / np.abs(EW).sum(axis=1)).max(initial=0.0)
        vx2, vy2 = c["v2"][0][b], c["v2"][1][b]
        tol = err1(a * c["vx"][b] + vx2, a * c["vy"][b] + vy2) + a * b1 + err1(vx2, vy2)
        lin = np.abs(c["lin"]["dg"][b] - (a * f["dg"][b] + c["second"]["dg"][b])).max()
        xy = np.abs(c["x"][b]).max() + np.abs(c["y"][b]).max()
        linm = np.abs(stacked(c["lin"])[b] - (a * stacked(f)[b] + stacked(c["second"])[b])).max()
        print(f"  {key} instance {b}: |E_r dg - vy_r| / |E_r|_1 {res:.3g} (bound {b1:.3g}), linearity dg {lin:.3g} (tol {tol:.3g}), "
              f"matrices {linm:.3g} (tol {tol * xy:.3g})")
        assert res <= b1 and lin <= tol and linm <= tol * xy


# ---- 4: the sums over the batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_reduce(hip, key):
    c = solved_case(key)
    B = SHAPES[key][3]
    for k in MATS:
        assert c["red"][k].tobytes() == c["red2"][k].tobytes()
        terms = c["full"][k]
        want = terms.sum(axis=0)
        bound = B * EPS * np.abs(terms).sum(axis=0)
        err = np.abs(c["red"][k] - want)
        ratio = (err[bound > 0] / bound[bound > 0]).max(initial=0.0)
        print(f"  {key} d{k}: worst |reduce - sum| {err.max(initial=0.0):.3g}, worst error / bound {ratio:.3g}, zero-bound entries {np.count_nonzero(bound == 0)}")
        assert np.all(err <= bound)
    assert c["some"]["A"].tobytes() == c["red"]["A"].tobytes() and "Q" not in c["some"]
    for name in ("dg", "db", "side", "info"):
        assert np.array_equal(c["red"][name], c["full"][name])


def test_reduce_skips_a_failed_instance(hip):
    ds = [P.warm_up_w_A(), P.infeasible(), P.warm_up_w_A()]      # the recipe of test_flag_of_a_failed_instance
    bt = hip.BatchLCQP(3, 2, 1, 1, opt=hip.default_options())
    load_all(bt, ds)
    bt.run()
    st = bt.solution()[2]
    assert st[0]["returnValue"] == 0 and st[1]["returnValue"] != 0 and st[2]["returnValue"] == 0
    vx, vy = np.ones((3, 2)), np.ones((3, 5))
    f = bt.adjoint(vx, vy); r = bt.adjoint(vx, vy, reduce=True)
    bt.close()
    print("  info", f["info"], "dQ", r["Q"].tolist(), "dA", r["A"].tolist())
    assert f["info"][1] & 1 and not (f["info"][0] & 1) and not (f["info"][2] & 1)
    for k in MATS:
        assert np.all(f[k][1] == 0.0) and np.all(np.isfinite(r[k]))
        assert np.array_equal(r[k], f[k][0] + f[k][2])
    assert np.any(r["Q"] != 0.0)


# ---- 5: chunking ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_chunks_of_one_instance_give_the_same_bits(hip, key):
    c = solved_case(key)
    for k in c["full"]:
        assert c["chunked"][k].tobytes() == c["full"][k].tobytes(), k


# ---- 6: no side effects ------------------------------------------------------------------------------------------------------------
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
            rng = np.random.default_rng(1)
            vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, n + nC + 2 * nComp))
            bt.adjoint(vx, vy); bt.adjoint(vx, vy, reduce=True); bt.adjoint(vx, vy, _staging_bytes=1)
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


def test_a_batch_that_never_ran_is_refused(hip):
    n = 40
    d = random_lcqp(np.random.default_rng(1000), n, 20, 8, False, False)
    bt = hip.BatchLCQP(1, n, 20, 8)
    load_all(bt, [d])
    with pytest.raises(RuntimeError, match="code 300"):
        bt.adjoint(np.ones((1, n)))
    bt.run()
    assert np.any(bt.adjoint(np.ones((1, n)))["Q"] != 0.0)
    bt.close()


# ---- 7: central differences -----------------------------------------------------------------------------------------------------------
def directions(rng, n, nC, nComp):
    Z = dict(Q=rng.standard_normal((n, n)), A=rng.standard_normal((nC, n)), L=rng.standard_normal((nComp, n)), R=rng.standard_normal((nComp, n)))
    Z["Q"] = 0.5 * (Z["Q"] + Z["Q"].T)
    return Z


def fd_bounds(tol, Q, EW, vx, vyW):
    ev = np.linalg.eigvalsh(Q)
    bx = tol * np.abs(vx).sum() / (H_FD * ev[0])
    by = 0.0
    if len(EW):
        by = tol * np.sqrt(len(vx) * ev[-1] / ev[0]) * np.abs(vyW).sum() / (H_FD * np.linalg.svd(EW, compute_uv=False)[-1])
    return bx, by


@pytest.mark.parametrize("n,m", [(40, 28), (200, 120)])
def test_central_differences_convex_twin(hip, n, m):
    rng = np.random.default_rng(n)
    Mx = rng.standard_normal((n, n)) / np.sqrt(n); Q = Mx.T @ Mx + np.eye(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n); xs = rng.standard_normal(n)
    lbA = A @ xs - rng.uniform(0.05, 0.5, m); ubA = A @ xs + rng.uniform(0.05, 0.5, m); g = 3.0 * rng.standard_normal(n)
    vx, vy = rng.standard_normal(n), rng.standard_normal(n + m)
    Z = directions(rng, n, m, 0)
    opt = hip.default_options()

    def solved(Qm, Am):
        q = hip.SubsolverHIP(n, m, Qm, Am)
        ret, it, flag = q.solve(True, g, lbA, ubA, np.zeros(n))
        assert ret == 0 and flag == 0
        return q

    q = solved(Q, A)
    r = q.adjoint(vx, vy)
    W = working_rows(q.read_working_set())
    q.close()
    assert r["info"] == 0 and len(W) > 0 and np.array_equal(np.flatnonzero(r["side"][n:]), W)
    bx, by = fd_bounds(opt.stationarityTolerance, Q, A[W], vx, vy[n + W])
    for k in ("Q", "A"):
        val = []
        for sgn in (+1.0, -1.0):
            qs = solved(Q + sgn * H_FD * Z[k] if k == "Q" else Q, A + sgn * H_FD * Z[k] if k == "A" else A)
            x, y = qs.getSolution()
            assert np.array_equal(working_rows(qs.read_working_set()), W)      # a convex QP: no branch to lose, every case counts
            qs.close()
            val.append((vx @ x, vy @ y))
        fdx, fdy = (val[0][0] - val[1][0]) / (2 * H_FD), (val[0][1] - val[1][1]) / (2 * H_FD)
        pred = np.sum(r[k] * Z[k])
        err = abs(fdx + fdy - pred)
        print(f"  QP ({n},{m}) d{k}: fd {fdx + fdy:+.9e} (x part {fdx:+.3e}, y part {fdy:+.3e}) predicted {pred:+.9e} err {err:.3g} "
              f"(rel {err / max(abs(pred), 1e-300):.3g}) bound {bx + by:.3g} (x {bx:.3g}, y {by:.3g})")
        assert err <= bx + by


@pytest.mark.parametrize("n,nC,nComp", [(40, 20, 8), (200, 330, 37)])
def test_central_differences_lcqp(hip, n, nC, nComp):
    B = 8
    nd = n + nC + 2 * nComp
    opt = hip.default_options(perturbStep=0)
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    load_all(bt, ds)
    bt.run()
    x0, y0, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    rng = np.random.default_rng(6)
    vx, vy = rng.standard_normal((B, n)), rng.standard_normal((B, nd))
    r = bt.adjoint(vx, vy)
    W0 = [working_rows(bt.read_working_set(b)) for b in range(B)]
    bt.close()
    Z = [directions(rng, n, nC, nComp) for _ in range(B)]
    bounds = []
    for b, d in enumerate(ds):
        E, lo, hi, pos = rows_and_bounds(d)
        bounds.append(sum(fd_bounds(opt.stationarityTolerance, d["Q"], E[W0[b]], vx[b], vy[b][pos[W0[b]]])))
    # the perturbed solves start at the unperturbed solution, at its final penalty: one batch per penalty value (the options are per batch)
    groups = {}
    for b in range(B):
        groups.setdefault(st[b]["rhoOpt"], []).append(b)
    print(f"  ({n},{nC},{nComp}): penalties {sorted(groups)} -> instances {[groups[k] for k in sorted(groups)]}")

    def perturbed_solves(k, sgn):
        val, keep = np.zeros(B), np.zeros(B, dtype=bool)
        for rho, members in groups.items():
            o = hip.default_options(perturbStep=0, solveZeroPenaltyFirst=0, initialPenaltyParameter=rho)
            bs = hip.BatchLCQP(len(members), n, nC, nComp, opt=o)
            load_all(bs, [dict(ds[b], **{k: ds[b][k] + sgn * H_FD * Z[b][k]}, x0=x0[b], y0=y0[b]) for b in members])
            bs.run()
            xs, ys, sts = bs.solution()
            for i, b in enumerate(members):
                keep[b] = sts[i]["returnValue"] == 0 and np.array_equal(working_rows(bs.read_working_set(i)), W0[b])
                val[b] = vx[b] @ xs[i] + vy[b] @ ys[i]
            bs.close()
        return val, keep

    for k in MATS:
        vp, kp = perturbed_solves(k, +1.0); vm, km = perturbed_solves(k, -1.0)
        keep = kp & km & (r["info"] == 0)
        fd = (vp - vm) / (2 * H_FD)
        pred = np.array([np.sum(r[k][b] * Z[b][k]) for b in range(B)])
        err = np.abs(fd - pred)
        for b in range(B):
            print(f"  ({n},{nC},{nComp}) d{k} instance {b}: fd {fd[b]:+.9e} predicted {pred[b]:+.9e} err {err[b]:.3g} "
                  f"(rel {err[b] / max(abs(pred[b]), 1e-300):.3g}) bound {bounds[b]:.3g} kept {bool(keep[b])}")
        assert np.count_nonzero(~keep) <= B // 8, keep
        assert np.all(err[keep] <= np.array(bounds)[keep])


# ---- 8: torch ------------------------------------------------------------------------------------------------------------------------
def test_torch_solve(hip):
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    n, nC, nComp, B = 40, 20, 8, 4
    nd = n + nC + 2 * nComp
    opt = hip.default_options(perturbStep=0)
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    ds = [dict(d, Q=ds[0]["Q"], A=ds[0]["A"]) for d in ds]      # one Q and one A for the batch; g and the bounds differ
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    load_all(bt, ds)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    T = lambda a, grad=True: torch.tensor(a, dtype=torch.float64, requires_grad=grad)
    g = T(stack(ds, "g")); Q = T(ds[0]["Q"]); A = T(ds[0]["A"])
    x, y = layer.solve(g, Q=Q, A=A)
    assert x.shape == (B, n) and y.shape == (B, nd) and x.dtype == torch.float64 and all(s["returnValue"] == 0 for s in layer.stats)
    xs, ys, _ = bt.solution()
    assert np.array_equal(x.detach().numpy(), xs) and np.array_equal(y.detach().numpy(), ys)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        (x.sum() + y.square().sum()).backward()
    want = bt.adjoint(np.ones((B, n)), 2.0 * ys, matrices=("Q", "A"), reduce=True)
    assert np.all(want["info"] == 0)
    assert Q.grad.shape == (n, n) and A.grad.shape == (nC, n)
    assert np.array_equal(Q.grad.numpy(), want["Q"]) and np.array_equal(A.grad.numpy(), want["A"]) and np.array_equal(g.grad.numpy(), want["dg"])
    assert np.any(want["Q"] != 0.0) and np.any(want["A"] != 0.0)
    # per-instance tensors get [B] ... gradients; L shared in the same call
    Qb = T(stack(ds, "Q")); Lm = T(ds[0]["L"]); lbA = T(stack(ds, "lbA"))
    x, y = layer.solve(g.detach(), Q=Qb, L=Lm, lbA=lbA)
    (x.sum() + y.square().sum()).backward()
    ys = bt.solution()[1]
    each = bt.adjoint(np.ones((B, n)), 2.0 * ys, matrices=("Q",)); summed = bt.adjoint(np.ones((B, n)), 2.0 * ys, matrices=("L",), reduce=True)
    assert Qb.grad.shape == (B, n, n) and np.array_equal(Qb.grad.numpy(), each["Q"]) and np.array_equal(Lm.grad.numpy(), summed["L"])
    parts = hip.split_bound_derivatives(each["db"], each["side"], n, nC, nComp)
    assert np.array_equal(lbA.grad.numpy(), parts["dlbA"]) and np.any(parts["dlbA"] != 0.0)
    # without matrix tensors: the update + resolve of __call__
    counts = bt.launch_counts()
    x, y = layer.solve(g.detach())
    assert bt.launch_counts() == (counts[0], counts[1] + 1)
    bt.close()


def test_torch_call_is_untouched(hip):
    """layer(g) and its backward: one lcqp_hip_batch_sensitivity call, whose bits they return"""
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    n, nC, nComp, B = 40, 20, 8, 4
    ds = [random_lcqp(np.random.default_rng(1000 + b), n, nC, nComp, False, False) for b in range(B)]
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    load_all(bt, ds)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    w = np.random.default_rng(9).standard_normal((B, n))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64, requires_grad=True)
    x = layer(g)
    assert isinstance(x, torch.Tensor) and bt.launch_counts() == (1, 1)
    (torch.as_tensor(w) * x).sum().backward()
    dg, db, side, info = bt.sensitivity(w)
    assert np.all(info == 0) and g.grad.numpy().tobytes() == dg.tobytes()
    bt.close()


def test_torch_solve_warns_about_flagged_instances(hip):
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    ds = [P.warm_up_w_A(), P.infeasible(), P.warm_up_w_A()]
    bt = hip.BatchLCQP(3, 2, 1, 1, opt=hip.default_options())
    load_all(bt, ds)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=stack(ds, "lbA"), ubA=stack(ds, "ubA")))
    g = torch.tensor(stack(ds, "g"), dtype=torch.float64, requires_grad=True)
    Q = torch.tensor(stack(ds, "Q"), dtype=torch.float64, requires_grad=True)
    x, y = layer.solve(g, Q=Q)
    with pytest.warns(RuntimeWarning, match="of 3 instances") as rec:
        (x.sum() + y.sum()).backward()
    assert len(rec) == 1
    assert layer.info[1] & 1 and not (layer.info[0] & 1) and torch.all(g.grad[1] == 0) and torch.all(Q.grad[1] == 0)
    bt.close()
