"""tests/admm_ref.py, the numpy reference of the ADMM fallback, without a device and without the oracle: run to convergence it reaches the
KKT point of two small QPs, and a float64 run of the same functions stays below 1e-2 of the bounds tests/test_gpu_admm.py holds the device
to, for every case, iteration count, admmRho and adapted rho vector used there -- the condition under which a correct double-precision implementation passes those
bounds with two orders to spare, so that a failure there is a defect and not rounding."""
import functools

import numpy as np
import pytest

import admm_ref as R
import problems as P

LD = np.longdouble


class Opt:      # the ADMM options of lcqp_hip_options_default (include/lcqp_hip.h)
    admmRho, admmSigma, admmAlpha, rhoEqMult = 0.1, 1e-6, 1.6, 1e3


def test_options_are_the_library_defaults():
    import lcqpow_amd as la
    o = la.default_options()
    assert (o.admmRho, o.admmSigma, o.admmAlpha, o.rhoEqMult) == (Opt.admmRho, Opt.admmSigma, Opt.admmAlpha, Opt.rhoEqMult)


def _small_qps():
    w = P.warm_up_w_A()       # the convex QP inside it: its rows A, L, R with the bounds of the LCQP
    E = np.vstack([w["A"], w["L"], w["R"]])
    yield w["Q"], E, w["g"], np.array([-0.5, 0.0, 0.0]), np.full(3, np.inf)
    inf, _ = P.certificate_qps()
    d = dict(inf); A = d["A"][2:]                       # without its two contradicting rows: a feasible polytope
    yield d["Q"], A, d["g"], d["lbA"][2:], d["ubA"][2:]


@pytest.mark.parametrize("which", [0, 1])
def test_reference_converges_to_the_kkt_point(which):
    Q, E, g, l, u = list(_small_qps())[which]
    n = len(g)
    scale = np.abs(np.diag(Q)).max()
    rhov = R.rho_vector(Opt, scale, l, u)
    x, y, z, dx, dy = R.admm(Q, E, g, l, u, rhov, Opt.admmSigma * scale, Opt.admmAlpha, np.zeros(n), np.zeros(len(l)), 3000)
    x, y, z = (v.astype(np.float64) for v in (x, y, z))
    assert np.abs(Q @ x + g + E.T @ y).max() < 1e-9                      # stationarity (y > 0 pushes against an upper bound)
    ex = E @ x
    assert (ex >= l - 1e-9).all() and (ex <= u + 1e-9).all() and np.abs(ex - z).max() < 1e-9
    at_l, at_u = np.abs(ex - l) < 1e-8, np.abs(ex - u) < 1e-8
    assert (y[~at_u] <= 1e-9).all() and (y[~at_l] >= -1e-9).all()        # signs and complementary slackness
    assert max(np.abs(dx).max(), np.abs(dy).max()) < 1e-12
    flag, _ = R.certificate(Q, E, g, l, u, dy, dx)
    assert flag == 0


def test_certificates_of_the_reference():
    """the two certificate QPs of tests/problems.py: 4 from the contradicting rows, 5 from the free descent direction"""
    for d, want in zip(P.certificate_qps(), (4, 5)):
        n = len(d["g"])
        scale = np.abs(np.diag(d["Q"])).max()
        rhov = R.rho_vector(Opt, scale, d["lbA"], d["ubA"])
        x, y, z, dx, dy = R.admm(d["Q"], d["A"], d["g"], d["lbA"], d["ubA"], rhov, Opt.admmSigma * scale, Opt.admmAlpha, np.zeros(n),
                                 np.zeros(len(rhov)), 400)
        assert R.certificate(d["Q"], d["A"], d["g"], d["lbA"], d["ubA"], dy, dx)[0] == want


def test_adapt_factor_formula():
    """a hand-made state: |E x - z| = 2 of max(|E x|, |z|) = 4, |Q x + g + E'y| = 1 of max(...) = 8: sqrt((2 / 4) / (1 / 8)) = 2"""
    Q = np.diag([8.0, 1.0]); E = np.array([[2.0, 0.0]]); x = np.array([1.0, 0.0]); z = np.array([4.0]); y = np.array([-2.0]); g = np.array([-3.0, 0.0])
    fac, applied = R.adapt_factor(Q, E, g, x, y, z)
    assert abs(float(fac) - 2.0) < 1e-15 and not applied
    big, on = R.adapt_factor(Q, E, np.array([-3.99, 0.0]), x, y, z)           # the dual residual 100 times smaller: sqrt(400)
    assert abs(float(big) - 20.0) < 1e-11 and on
    small, on = R.adapt_factor(Q, E, g, x, y, np.array([2.001]))             # the primal residual 1e-3: sqrt((1e-3 / 2.001) * 8)
    assert abs(float(small) - np.sqrt(8e-3 / 2.001)) < 1e-12 and on


@functools.lru_cache(maxsize=None)
def _float64_ratio(kind, key):
    """worst error / bound of the float64 run against the long-double run over the iteration counts of checks B, C and D"""
    if kind == "batch":
        return max(_float64_ratio("instance", key + (j,)) for j in range(min(key[0], 3)))
    d = R.qp_case(*key) if kind == "qp" else R.batch_data(*key[:4])[key[4]]
    E, l, u = R.stacked(d)
    n = d["n"]
    scale = np.abs(np.diag(d["Q"])).max(); sigma = Opt.admmSigma * scale
    rhov = R.rho_vector(Opt, scale, l, u)
    keep = tuple(sorted(set(R.KS) | {R.K_ADAPT}))
    worst = 0.0
    Kld = R.K(d["Q"], E, sigma, rhov)
    condK = R.cond2(Kld)
    L64 = np.linalg.cholesky(R.K(d["Q"], E, sigma, rhov, np.float64))
    bound = R.factor_bound(L64, d["Q"], E, sigma, rhov)
    worst = max(worst, float((np.abs(L64.astype(LD) @ L64.T.astype(LD) - Kld) / bound).max()))
    starts = [(np.zeros(n), np.zeros(len(l)))]
    if kind == "qp":      # the QP object is also started from a given point and given duals
        starts.append((d["x0"], R.start_duals(d, d["y0"])))
    for x0, y0 in starts:
        ref = R.admm(d["Q"], E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, x0, y0, max(keep), LD, keep)
        f64 = R.admm(d["Q"], E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, x0, y0, max(keep), np.float64, keep)
        for k in keep:
            b, by = R.iterate_bounds(n, condK, k, *ref[k][:3], rhov)
            for name, err, bd in R.iterate_errors(f64[k], ref[k], rhov, b, by):
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = max(worst, float(np.where(err > 0, err / bd, 0.0).max()))
        fr, _ = R.adapt_factor(d["Q"], E, d["g"], *ref[R.K_ADAPT][:3])
        f6, _ = R.adapt_factor(d["Q"], E, d["g"], *f64[R.K_ADAPT][:3], dt=np.float64)
        worst = max(worst, abs(float(f6 / fr) - 1.0) / (1e-12 * n * condK))
    return worst


@pytest.mark.parametrize("key", R.QP_CASES + R.BATCH_CASES)
def test_float64_stays_two_orders_below_the_gpu_bounds(key):
    worst = _float64_ratio("qp" if len(key) == 3 else "batch", key)
    print(f"    float64 against long double: worst error / bound = {worst:.3e}")
    assert worst < 1e-2


def _case_ref(kind, key, rho):
    class O(Opt):
        admmRho = rho
    d = R.qp_case(*key) if kind == "qp" else R.batch_data(*key[:4])[key[4]]
    E, l, u = R.stacked(d)
    scale = np.abs(np.diag(d["Q"])).max()
    rhov = R.rho_vector(O, scale, l, u)
    return d, E, l, u, rhov, O.admmSigma * scale


def test_rho_update_cases_lie_clear_of_the_thresholds():
    """check D of tests/test_gpu_admm.py: a factor above 5, one below 0.2, one not applied, each at least 10 % from both thresholds -- for
    every instance the GPU test reads, and for the second update of the QP object's hot start (10 iterations from x = 0 at the new rho)"""
    seen = set()
    for key, rho, want in R.QP_RHO_CASES:
        d, E, l, u, rhov, sigma = _case_ref("qp", key, rho)
        n = d["n"]
        st = R.admm(d["Q"], E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, np.zeros(n), np.zeros(len(l)), R.K_ADAPT, np.float64)
        fac, applied = R.adapt_factor(d["Q"], E, d["g"], *st[:3], dt=np.float64)
        assert R.direction(fac, applied) == want
        seen.add(want)
        if applied:
            rhov = rhov * float(fac)
        st = R.admm(d["Q"], E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, np.zeros(n), np.zeros(len(l)), 10, np.float64)
        R.direction(*R.adapt_factor(d["Q"], E, d["g"], *st[:3], dt=np.float64))
    assert seen == {1, 0, -1}
    for key, rho, want in R.BATCH_RHO_CASES:
        for j in range(min(key[0], 3)):
            d, E, l, u, rhov, sigma = _case_ref("batch", key + (j,), rho)
            st = R.admm(d["Q"], E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, np.zeros(d["n"]), np.zeros(len(l)), R.K_ADAPT, np.float64)
            got = R.direction(*R.adapt_factor(d["Q"], E, d["g"], *st[:3], dt=np.float64))
            assert j > 0 or got == want


def test_certificate_cases_lie_clear_of_the_thresholds():
    """check F: the reference iterates along the fallback rounds reach flag 4 after 10 + 20 + 40 iterations and flag 5 after 10 + 20, and no
    comparison of the deciding predicate lies within a factor 10 of its threshold"""
    for d, want, rounds in zip(P.certificate_qps(R.F_SEED, R.F_N, R.F_M, box=True), (4, 5), (3, 2)):
        E, l, u = R.stacked(dict(d, n=R.F_N))
        scale = np.abs(np.diag(d["Q"])).max()
        rhov = R.rho_vector(Opt, scale, l, u)
        flag, comps, r, _ = R.fallback_rounds(d["Q"], E, d["g"], l, u, rhov, Opt.admmSigma * scale, Opt.admmAlpha, 6, np.float64)
        assert (flag, r) == (want, rounds) and R.clearance(comps) >= 10.0


def _float64_ratio_rho(kind, key, rho, hot):
    """the float64 condition for checks D and E: at the case's admmRho, the 15 iterations in front of the rho update, the factor, the
    factor of K at the rho vector the update leaves; hot (the QP object): the ten iterations of the hot start at that rho vector from
    x = 0, the second factor and K behind it"""
    d, E, l, u, rhov, sigma = _case_ref(kind, key, rho)
    n = d["n"]
    zero = (np.zeros(n), np.zeros(len(l)))
    worst = 0.0

    def ratio(err, bd):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.where(err > 0, err / bd, 0.0).max())

    for k in ((R.K_ADAPT, 10) if hot else (R.K_ADAPT,)):
        condK = R.cond2(R.K(d["Q"], E, sigma, rhov))
        ref = R.admm(d["Q"], E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, *zero, k, LD)
        f64 = R.admm(d["Q"], E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, *zero, k, np.float64)
        b, by = R.iterate_bounds(n, condK, k, *ref[:3], rhov)
        worst = max([worst] + [ratio(err, bd) for _, err, bd in R.iterate_errors(f64, ref, rhov, b, by)])
        fr, applied = R.adapt_factor(d["Q"], E, d["g"], *ref[:3])
        f6, _ = R.adapt_factor(d["Q"], E, d["g"], *f64[:3], dt=np.float64)
        worst = max(worst, abs(float(f6 / fr) - 1.0) / (1e-12 * n * condK))
        if applied:
            rhov = rhov * float(fr)
        L64 = np.linalg.cholesky(R.K(d["Q"], E, sigma, rhov, np.float64))
        worst = max(worst, ratio(np.abs(L64.astype(LD) @ L64.T.astype(LD) - R.K(d["Q"], E, sigma, rhov)), R.factor_bound(L64, d["Q"], E, sigma, rhov)))
    return worst


@pytest.mark.parametrize("case", R.QP_RHO_CASES + R.BATCH_RHO_CASES)
def test_float64_stays_two_orders_below_the_bounds_of_the_rho_update(case):
    key, rho, _ = case
    if len(key) == 3:
        worst = _float64_ratio_rho("qp", key, rho, True)
    else:
        worst = max(_float64_ratio_rho("batch", key + (j,), rho, False) for j in range(min(key[0], 3)))
    print(f"    admmRho = {rho}: float64 against long double: worst error / bound = {worst:.3e}")
    assert worst < 1e-2


# ---- the sparse arm's conventions (tests/sparse_admm_ref.py; tests/test_gpu_sparse_admm.py holds the device to it) ---------------------------
import sparse_admm_ref as SR


def test_sparse_reference_fixed_point_is_a_kkt_point():
    """with a free row at the weight 1e-6 rho: the iteration converges to the KKT point of the QP, the free row carries no multiplier and its
    z follows E x"""
    Q, E, g, l, u = list(_small_qps())[1]
    rng = np.random.default_rng(3)
    E = np.vstack([E, rng.standard_normal((1, E.shape[1]))]); l = np.append(l, -np.inf); u = np.append(u, np.inf)
    n = len(g)
    scale = np.abs(np.diag(Q)).max()
    rhov = SR.rho_vector(Opt, scale, l, u)
    assert rhov[-1] == 1e-6 * (Opt.admmRho * scale) and (rhov[:-1] >= Opt.admmRho * scale).all()
    x, y, z = (v.astype(np.float64) for v in SR.admm(Q, E, g, l, u, rhov, Opt.admmSigma * scale, Opt.admmAlpha, np.zeros(n), np.ones(len(l)), 3000))
    assert y[-1] == 0.0
    assert np.abs(Q @ x + g + E.T @ y).max() < 1e-9
    ex = E @ x
    assert (ex >= l - 1e-9).all() and (ex <= u + 1e-9).all() and np.abs(ex - z).max() < 1e-9
    at_l, at_u = np.abs(ex - l) < 1e-8, np.abs(ex - u) < 1e-8
    assert (y[~at_u] <= 1e-9).all() and (y[~at_l] >= -1e-9).all()


@functools.lru_cache(maxsize=None)
def _sparse_case(name):
    return SR.CASES[name][0]()


def _sparse_ratio(d, perm, dt):
    """worst error / bound of the device-form iteration in dtype dt (ordering perm) against the long-double reduced form, per quantity"""
    Q, E = SR.dense(d)
    l, u = SR.stacked(d)
    n = d["nV"]
    scale = np.abs(np.diag(Q)).max(); sigma = Opt.admmSigma * scale
    rhov = SR.rho_vector(Opt, scale, l, u)
    condK = R.cond2(R.K(Q, E, sigma, rhov, np.float64))
    worst = dict(xa=0.0, ya=0.0, za=0.0)
    for x0, y0 in ((np.zeros(n), np.zeros(len(l))), (d["x0"], -d["y0"])):
        ref = SR.admm(Q, E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, x0, y0, max(SR.KS), LD, SR.KS)
        got = SR.admm_kkt(Q, E, d["g"], l, u, rhov, sigma, Opt.admmAlpha, x0, y0, max(SR.KS), dt, perm, SR.KS)
        for k in SR.KS:
            b, by = SR.iterate_bounds(n, condK, k, *ref[k], rhov, l, u)
            for name, err, bd in SR.iterate_errors(got[k], ref[k], b, by):
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst[name] = max(worst[name], float(np.where(err > 0, err / bd, 0.0).max()))
    return worst


def test_sparse_kkt_form_and_reduced_form_agree_in_long_double():
    d = _sparse_case("small")[0]
    worst = _sparse_ratio(d, np.arange(d["nV"] + d["E"].shape[0]), LD)
    print(f"    KKT form against reduced form, both long double: worst error / bound = {worst}")
    assert max(worst.values()) < 1e-5       # eps of long double / eps of float64 = 5e-4 of what test_sparse_float64_... allows


@pytest.mark.parametrize("name", list(SR.CASES))
def test_sparse_float64_stays_two_orders_below_the_gpu_bounds(oracle, name):
    """a float64 run of the device's form -- the KKT matrix, an LDL' without pivoting in a fill-reducing ordering of the pattern, one solve
    per iteration, no refinement -- against the long-double reduced form: 1e-2 of the bounds of tests/test_gpu_sparse_admm.py at the most,
    for every instance, start and iteration count used there"""
    from test_sparse_kkt_ref import _ordering
    inst = _sparse_case(name)
    perm, _ = _ordering(oracle, inst[0], "general" in name)
    worst = dict(xa=0.0, ya=0.0, za=0.0)
    for d in inst:
        w = _sparse_ratio(d, perm, np.float64)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"    {name}: float64 KKT form against long double: worst error / bound = " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < 1e-2
