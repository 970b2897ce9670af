"""The ADMM fallback of the dense subsolver (qp_build_K, qp_admm, qp_adapt_rho, qp_certificate in lcqpow_amd/csrc/lcqp_dev.hpp) read back
from the device (lcqp_hip_batch_read_admm: it launches nothing) and held to tests/admm_ref.py, a long-double numpy reference written from
the formulas -- never to the oracle, which restates the same code.  A point is returned only on its true residual, so a wrong entry of L_K
or a stale factor costs rounds and never shows in x or y; and admmIter is a fixed schedule, so a wrong iteration counts the same.

The polish writes nothing of the ADMM state, so admmFirst = k, maxRounds and maxTrials = 1 fix how many iterations ran and whether a rho
update followed; every case asserts the counters that prove it (admmIter, kReady, the exit flag; in the batch the number of rebuilds
of L_K, stats.factorizations less the working-set updates the kernel counts by themselves; on the QP object the counter is held to the oracle's).

  A  rhov bit for bit, sigma and rhoAdmm, the bounds of the stacked rows in the device's order
  B  |L L' - K| <= 1e-12 (n + mE) (|L||L'| + |Q| + sigma I + |E|' diag(rho) |E|) entry by entry, L from the lower blocks of FK with the
     diagonal blocks inverted in long double; FK symmetric; exact zeros beyond n, the padding diagonal the factor of 1 + sigma
  C  xa, ya, za and dx, dy of the last step after k = 1, 5, 20 iterations: 1e-12 n cond_2(K) k max(1, |xa|, |za|, |ya| / min rho) (rows of
     ya and dy: times rho_r), from x = 0 and, on the QP object, from a given x0 and y0
  D  after 5 + 10 iterations the rho update: the factor to 1e-12 n cond_2(K), rhov to 4 ulp, FK against K at the NEW rhov, iterates
     untouched; no update: everything bit for bit as a run without the second round leaves it
  E  a hot start of the QP object keeps the adapted rho and its factor (deliberate: only a fresh setup resets them) and iterates with
     them; update + resolve on a batch (k_refresh) starts from the base rho again and rebuilds L_K; behind a refresh that no ADMM follows
     (crossed bounds end the QP on its bound check) kReady = 0 and rhov, rhoAdmm hold their base values
  F  the certificates at np = 256 with box rows: flags 4 and 5, the same from the reference's predicate on the device's own dx, dy, no
     comparison within a factor 10 of its threshold

tests/test_admm_ref.py holds a float64 run of the reference to 1e-2 of the bounds of B, C and D for every case here, so a ratio above
1e-2 below is not rounding.  Worst error / bound on an MI355X (`python -m pytest tests/test_gpu_admm.py -m gpu -s` prints them):

    A  rhov, sigma, rhoAdmm, stacked bounds    0 (exact)         B  L_K L_K' - K                        5.9e-6
    B  FK padding diagonal                     0 (exact)         C  xa 3.5e-7   ya 1.9e-7   za 1.7e-7   dx 3.5e-7   dy 1.9e-7
    D  rho factor                              4.5e-4            D  rhov = rho_vector x factor          0 (exact)
    F  closest comparison / threshold: a factor 50 (infeasible: |E'dy|), 9.2e3 (unbounded)
    (17 tests, 9 s of wall time; cond_2(K) is 270 ... 370 at admmRho = 0.1, and the bounds of C and D carry it: that is why their ratios are small)

Mutants of lcqp_dev.hpp (scratch builds, loaded through LCQPOW_HIP_LIBRARY; failing tests of this file / of the suite before it):

    1  rhov[r] dropped from the weight of the last 16-row panel in qp_build_K      16 of 17 / 12 of 304
    2  qp_adapt_rho scales rhov without rebuilding FK                              6 of 17 / 16 of 304
    3  alpha applied to xa but not to za in qp_admm                                16 of 17 / 7 of 304
    (the suite before it: the dense GPU files, 304 tests; the sparse arm shares no code with lcqp_dev.hpp.  What it catches are iterate
    counts, work counters, exit flags and return codes against the oracle, mostly of fuzz cases; none of them says where the defect is)
"""
import functools

import numpy as np
import pytest

import admm_ref as R
import problems as P
from test_gpu_setup import _chk, tri_inv

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(float).eps


# ---- references, computed once per case ---------------------------------------------------------------------------------------------------
class Ref:
    """the reference of one problem at one admmRho: the stacked rows, rho vector, K, and the states after the kept iteration counts"""

    def __init__(self, d, opt, start=None):
        self.d, self.n = d, d["n"]
        self.E, self.l, self.u = R.stacked(d)
        self.mE = len(self.l)
        self.scale = np.abs(np.diag(d["Q"])).max()
        self.sigma = opt.admmSigma * self.scale
        self.rho0 = opt.admmRho * self.scale
        self.rhov = R.rho_vector(opt, self.scale, self.l, self.u)
        self.alpha = opt.admmAlpha
        self.condK = R.cond2(R.K(d["Q"], self.E, self.sigma, self.rhov, np.float64))
        x0, y0 = start if start else (np.zeros(self.n), np.zeros(self.mE))
        keep = tuple(sorted(set(R.KS) | {R.K_ADAPT}))
        self.states = R.admm(d["Q"], self.E, d["g"], self.l, self.u, self.rhov, self.sigma, self.alpha, x0, y0, max(keep), LD, keep)

    def factor(self):
        return R.adapt_factor(self.d["Q"], self.E, self.d["g"], *self.states[R.K_ADAPT][:3])

    def with_rho(self, rhov, rho0):
        """the same problem at another rho vector (after a rho update): rhov, rho0 and cond_2(K) follow, the kept states do not"""
        import copy
        r = copy.copy(self)
        r.rhov, r.rho0, r.states = rhov, rho0, None
        r.condK = R.cond2(R.K(self.d["Q"], self.E, self.sigma, rhov, np.float64))
        return r


@functools.lru_cache(maxsize=None)
def _ref(kind, key, rho, given_start=False):
    import lcqpow_amd as la
    opt = la.default_options(admmRho=rho)
    if kind == "qp":
        d = R.qp_case(*key)
        return Ref(d, opt, (d["x0"], R.start_duals(d, d["y0"])) if given_start else None)
    return Ref(R.batch_data(*key[:4])[key[4]], opt)


# ---- the checks ------------------------------------------------------------------------------------------------------------------------------
def check_vectors(ra, ref, adapted=False):
    """A: the layout, the bounds in stacked order, and (before any rho update) rhov, sigma and rhoAdmm"""
    n, mE = ref.n, ref.mE
    assert ra["mE"] == mE <= ra["mEcap"] and ra["np"] >= n and ra["np"] == 64 * ra["nblk"] and ra["setupFail"] == 0
    assert np.array_equal(ra["l"][:mE], ref.l) and np.array_equal(ra["u"][:mE], ref.u)
    assert ra["scale"] == ref.scale and ra["sigma"] == ref.sigma
    if not adapted:
        assert ra["rhoAdmm"] == ref.rho0 and np.array_equal(ra["rhov"][:mE], ref.rhov)


def unpack_LK(ra):
    """L_K [n][n] in long double: the strict lower blocks of FK as they are, the diagonal blocks by inverting what FK holds there"""
    FK, n = ra["FK"], ra["np"]
    L = np.tril(FK).astype(LD)
    for J in range(ra["nblk"]):
        s = slice(64 * J, 64 * J + 64)
        L[s, s] = tri_inv(np.tril(FK[s, s]), LD)
    return L


def check_factor(ra, ref, rhov, tag=""):
    """B: FK factors K at the rho vector given, entry by entry; symmetric fill; padding"""
    n, npad, FK = ref.n, ra["np"], ra["FK"]
    assert ra["kReady"] == 1
    assert np.array_equal(FK, FK.T)
    off = FK - np.diag(np.diag(FK))
    assert not off[n:, :].any() and not off[:, n:].any()
    if npad > n:      # the unit diagonal of the padding plus sigma, factored with the rest and stored inverted like every diagonal block
        _chk(tag + "FK padding diagonal = 1/sqrt(1+sigma)", np.abs(np.diag(FK)[n:] * np.sqrt(1.0 + ra["sigma"]) - 1.0), 4 * EPS)
    # beyond np = 512 the products are float64, as in test_gpu_setup.py (their own error, 1e-16 (n + mE), is four orders below the bound)
    dt = LD if npad <= 512 else np.float64
    L = unpack_LK(ra)[:n, :n].astype(dt)
    Kref = R.K(ref.d["Q"], ref.E, ra["sigma"], rhov, dt)
    _chk(tag + "L_K L_K' - K", np.abs(L @ L.T - Kref), R.factor_bound(L, ref.d["Q"], ref.E, ra["sigma"], rhov))


def check_iterates(ra, ref, k, tag="", state=None, rhov=None):
    """C: the five vectors against the reference after k iterations; beyond mE and n the device holds nothing of the iteration"""
    n, mE = ref.n, ref.mE
    st = state if state is not None else ref.states[k]
    rhov = ref.rhov if rhov is None else rhov
    b, by = R.iterate_bounds(n, ref.condK, k, *st[:3], rhov)
    dev = (ra["xa"][:n], ra["ya"][:mE], ra["za"][:mE], ra["dx"][:n], ra["dy"][:mE])
    for name, err, bd in R.iterate_errors(dev, st, rhov, b, by):
        _chk(f"{tag}k = {k}: {name}", err, bd)
    assert not ra["xa"][n:].any() and not ra["dx"][n:].any()
    assert not ra["ya"][:mE][rhov == 0].any()


def check_rho_update(ra, ref, fac, applied, before, tag=""):
    """D: ra after the rho update against the reference factor; before = the read-back of a run that stopped in front of the update"""
    mE = ref.mE
    if not applied:
        assert ra["rhoAdmm"] == ref.rho0 and np.array_equal(ra["rhov"], before["rhov"]) and np.array_equal(ra["FK"], before["FK"])
        return ref.rhov
    ratio = ra["rhoAdmm"] / ref.rho0
    _chk(tag + "rho factor", abs(ratio / float(fac) - 1.0), 1e-12 * ref.n * ref.condK)
    assert (float(fac) > 5.0) == (ratio > 5.0) and (ratio > 5.0 or ratio < 0.2)
    new = ra["rhov"][:mE]
    _chk(tag + "rhov = rho_vector x factor", np.abs(new - ref.rhov * ratio), 4 * EPS * ref.rhov * ratio)
    assert not np.array_equal(ra["FK"], before["FK"])
    check_factor(ra, ref, new, tag + "new rho: ")
    return new


# ---- the QP object: k_qp_solve ---------------------------------------------------------------------------------------------------------------
def qp_solve(hip, d, k, rounds=1, rho=0.1, given_start=False, keep=False):
    n, m = d["n"], d["m"]
    opt = hip.default_options(admmFirst=k, maxRounds=rounds, maxTrials=1, admmRho=rho)
    q = hip.SubsolverHIP(n, m, d["Q"], d["A"], opt=opt)
    r = q.solve(True, d["g"], d["lbA"], d["ubA"], d["x0"] if given_start else np.zeros(n), d["y0"] if given_start else None, d["lb"], d["ub"])
    ra, cnt = q.read_admm(), q.counters()
    if keep:
        return q, r, ra, cnt
    q.close()
    return r, ra, cnt


@pytest.mark.parametrize("key,npad", list(zip(R.QP_CASES, (128, 256, 384, 1024))))
def test_qp_object_factor_and_iterates(hip, key, npad):
    """A, B and C through the QP object at np = 128, 256 (mE odd: the row tail of the weighted product), 384 (odd NCH) and 1024 (the
    NCH = 8 instantiation), from x = 0 and from a given x0 with duals y0 (ya starts at -y0 in stacked order, box rows included)"""
    d = R.qp_case(*key)
    ref = _ref("qp", key, 0.1)
    assert ref.mE % 2 == (1 if key[1] % 2 else 0) and (ref.rhov == 0).any() and (ref.l == ref.u).any()
    for k in R.KS:
        r, ra, cnt = qp_solve(hip, d, k)
        assert ra["np"] == npad and cnt["admm"] == k and ra["kReady"] == 1, (r, cnt)
        check_vectors(ra, ref)
        if k == R.KS[0]:
            check_factor(ra, ref, ref.rhov)
        check_iterates(ra, ref, k)
    ref2 = _ref("qp", key, 0.1, True)
    r, ra, cnt = qp_solve(hip, d, 5, given_start=True)
    assert cnt["admm"] == 5 and ra["kReady"] == 1
    check_vectors(ra, ref2)
    check_iterates(ra, ref2, 5, "given x0, y0: ")


# ---- the batch: k_lcqp_run ---------------------------------------------------------------------------------------------------------------------
def batch_load(hip, key, **opts):
    B, n, nC, nComp = key
    data = R.batch_data(*key)
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=True, opt=hip.default_options(perturbStep=0, maxTrials=1, **opts))
    for b in range(B):
        d = data[b % len(data)]
        assert bt.load(b, 1, d["Q"], d["g"], d["L"], d["R"], A=d["A"], lbA=d["lbA"], ubA=d["ubA"], lb=d["lb"], ub=d["ub"]) == 0
    return bt


def batch_stats(bt, total, flag=None):
    """the first QP of every instance ran exactly `total` ADMM iterations and ended the run"""
    _, _, st = bt.solution()
    for s in st:
        assert s["admmIter"] == total and s["qpSolves"] == 1 and s["iterTotal"] == 0, s
        assert flag is None or (s["qpSolverExitFlag"], s["returnValue"]) == (flag, 203), s
    return st


@pytest.mark.parametrize("key,npad,sample", [(R.BATCH_CASES[0], 128, (0, 1, 2, 5)), (R.BATCH_CASES[1], 256, (0, 1, 2)),
                                             (R.BATCH_CASES[2], 128, (0, 521, 1039)), (R.BATCH_CASES[3], 256, (0, 1))])
def test_batch_factor_and_iterates(hip, key, npad, sample):
    """A, B and C through k_lcqp_run: x0 = 0, no lbL / lbR, so the first QP's linear term is g, and maxTrials = 1, maxRounds = 1 end the run
    with it.  (6, 64, 96, 16) and (3, 200, 330, 37): the row state in LDS; B = 1040 > 3 x CU count: the build held to 128 registers;
    (2, 256, 700, 100): m_E > 640, the row state in global memory.
    Nothing the library reports tells which build of k_lcqp_run a launch took, so the 128-register case proves its path by its size alone:
    the host selects that build above three workgroups per CU, 768 on the 256 CUs of an MI355X; on a part with more than 346 CUs B = 1040
    would run the other build and this case would have to grow."""
    B = key[0]
    bt = batch_load(hip, key, admmFirst=R.KS[0], maxRounds=1)
    for k in R.KS:
        if k != R.KS[0]:
            bt.set_options(hip.default_options(perturbStep=0, maxTrials=1, admmFirst=k, maxRounds=1))
        bt.run()
        batch_stats(bt, k)
        for b in sample:
            ref = _ref("batch", key + (b % min(B, 3),), 0.1)
            ra = bt.read_admm(b)
            assert ra["np"] == npad and ra["kReady"] == 1 and (ref.mE > 640) == (key[2] > 640)
            check_vectors(ra, ref)
            if k == R.KS[0]:
                check_factor(ra, ref, ref.rhov, f"instance {b}: ")
            check_iterates(ra, ref, k, f"instance {b}: ")
    bt.close()


# ---- D and E: the rho update ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,rho,direction", R.QP_RHO_CASES)
def test_qp_object_rho_update_and_hot_start(hip, oracle, key, rho, direction):
    """D: admmFirst = 5, maxRounds = 2, maxTrials = 1 -- 5 + 10 iterations, both polishes fail (exit flag 1), qp_adapt_rho runs once.
    E: a hot start on top with the same bounds and options: round 0 has no ADMM (admmHot = 0), round 1 runs 10 iterations from the
    point the solve was given, on the rho vector and the factor the update left (kReady stays 1, nothing is rebuilt in front of them),
    and the rho update that follows it is held to the reference in the same way."""
    d = R.qp_case(*key)
    n = d["n"]
    ref = _ref("qp", key, rho)
    fac, applied = ref.factor()
    assert R.direction(fac, applied) == direction
    _, before, _ = qp_solve(hip, d, R.K_ADAPT, rounds=1, rho=rho)        # the same 15 iterations in one piece, no update behind them
    q, r, ra, cnt = qp_solve(hip, d, 5, rounds=2, rho=rho, keep=True)
    qo = oracle.QP(d["Q"], d["A"], oracle.default_options(admmFirst=5, maxRounds=2, maxTrials=1, admmRho=rho))
    ro = qo.solve(True, d["g"], d["lbA"], d["ubA"], np.zeros(n), None, d["lb"], d["ub"])
    assert r == ro and (r[0], r[2]) == (203, 1)
    co = qo.counters()
    # (the factorisation counter also counts the working-set updates of the two polishes and the QP object does not tell them apart, so it
    # is only held to the oracle's here; the rebuild itself is shown by FK != the FK before, kReady and check B at the new rhov below, and
    # counted exactly in the batch test)
    assert cnt["admm"] == R.K_ADAPT and all(cnt[c] == co[c] for c in ("admm", "trials", "factorizations")) and ra["kReady"] == 1
    check_vectors(ra, ref, adapted=True)
    check_iterates(ra, ref, R.K_ADAPT, "before the update: ")
    for v in ("xa", "ya", "za"):      # the update moves none of them: the bits of the run that stopped in front of it
        assert np.array_equal(ra[v], before[v]), v
    rhov = check_rho_update(ra, ref, fac, applied, before)
    # ---- E
    r2 = q.solve(False, d["g"], d["lbA"], d["ubA"], None, None, d["lb"], d["ub"])
    ra2, cnt2 = q.read_admm(), q.counters()
    assert (r2[0], r2[2]) == (203, 1) and cnt2["admm"] == R.K_ADAPT + 10 and ra2["kReady"] == 1
    rhov = rhov.copy()
    st = R.admm(d["Q"], ref.E, d["g"], ref.l, ref.u, rhov, ref.sigma, ref.alpha, np.zeros(n), np.zeros(ref.mE), 10)
    ref_hot = ref.with_rho(rhov, ra["rhoAdmm"])
    check_iterates(ra2, ref_hot, 10, "hot start: ", state=st, rhov=rhov)
    fac2, applied2 = R.adapt_factor(d["Q"], ref.E, d["g"], *st[:3])
    R.direction(fac2, applied2)
    print(f"    factors: {float(fac):.4g} ({'applied' if applied else 'not applied'}), hot start {float(fac2):.4g} ({'applied' if applied2 else 'not applied'})")
    check_rho_update(ra2, ref_hot, fac2, applied2, ra, "hot start: ")
    if not applied2:
        check_factor(ra2, ref_hot, rhov, "hot start, kept rho: ")
    q.close()


@pytest.mark.parametrize("key,rho,direction", R.BATCH_RHO_CASES)
def test_batch_rho_update_and_refresh(hip, oracle, key, rho, direction):
    """D through k_lcqp_run, every instance; then update + resolve on the same vectors: k_refresh puts rhov and rhoAdmm back to their base
    values and clears kReady, so the run behind it repeats the first one bit for bit -- a factor left from the adapted rho, or a rho
    vector scaled twice, would not -- without a second setup; then a refresh behind which no ADMM runs, read directly."""
    B, n, nC, nComp = key
    data = R.batch_data(*key)
    bt = batch_load(hip, key, admmFirst=R.K_ADAPT, maxRounds=1, admmRho=rho)
    bt.run()
    batch_stats(bt, R.K_ADAPT)
    before = [bt.read_admm(b) for b in range(B)]
    opt = dict(perturbStep=0, maxTrials=1, admmFirst=5, maxRounds=2, admmRho=rho)
    bt.set_options(hip.default_options(**opt))
    bt.run()
    st = batch_stats(bt, R.K_ADAPT, flag=1)
    # stats.factorizations counts the working-set updates of the polishes, which the kernel also sums by themselves (work_sums()[3]), and the
    # refactorisations of qp_adapt_rho: the difference is the number of rebuilds, one per instance whose factor is applied
    rebuilds = sum(s["factorizations"] for s in st) - int(bt.work_sums()[3])
    assert rebuilds == sum(_ref("batch", key + (b % min(B, 3),), rho).factor()[1] for b in range(B))
    first = []
    for b in range(B):
        d = data[b % len(data)]
        ref = _ref("batch", key + (b % min(B, 3),), rho)
        fac, applied = ref.factor()
        if b == 0:
            assert R.direction(fac, applied) == direction
        ro = oracle.lcqp_solve(d["Q"], d["g"], d["L"], d["R"], A=d["A"], lbA=d["lbA"], ubA=d["ubA"], lb=d["lb"], ub=d["ub"],
                               opt=oracle.default_options(**opt))
        assert ro["stats"]["factorizations"] == st[b]["factorizations"]
        ra = bt.read_admm(b)
        check_vectors(ra, ref, adapted=True)
        check_iterates(ra, ref, R.K_ADAPT, f"instance {b}, before the update: ")
        for v in ("xa", "ya", "za"):
            assert np.array_equal(ra[v], before[b][v]), v
        print(f"    instance {b}: factor {float(fac):.4g} ({'applied' if applied else 'not applied'})")
        check_rho_update(ra, ref, fac, R.direction(fac, applied) != 0, before[b], f"instance {b}: ")
        first.append(ra)
    # ---- E: the refresh
    setups = bt.launch_counts()[0]
    for b in range(B):
        d = data[b % len(data)]
        assert bt.update(b, 1, d["g"], lbA=d["lbA"], ubA=d["ubA"], lb=d["lb"], ub=d["ub"]) == 0
    bt.resolve()
    batch_stats(bt, R.K_ADAPT, flag=1)
    assert bt.launch_counts()[0] == setups
    for b in range(B):
        ra = bt.read_admm(b)
        for v in ("rhoAdmm", "kReady"):
            assert ra[v] == first[b][v]
        for v in ("rhov", "FK", "xa", "ya", "za", "dx", "dy"):
            assert np.array_equal(ra[v], first[b][v]), (b, v)
    # the state k_refresh leaves, seen directly: one row of A gets crossed bounds, so the QP behind the refresh ends on its bound check
    # (exit flag 2) before any ADMM work, and what is read is what k_refresh wrote -- kReady = 0, rhoAdmm and rhov at their base values for
    # the bounds in place -- in every instance, whether its factor had been applied or not
    for b in range(B):
        d = data[b % len(data)]
        r0 = int(np.flatnonzero(np.isfinite(d["lbA"]) & np.isfinite(d["ubA"]) & (d["lbA"] < d["ubA"]))[0])
        lo = d["lbA"].copy(); lo[r0] = d["ubA"][r0] + 1.0
        assert bt.update(b, 1, d["g"], lbA=lo, ubA=d["ubA"], lb=d["lb"], ub=d["ub"]) == 0
    bt.resolve()
    _, _, st = bt.solution()
    assert bt.launch_counts()[0] == setups
    for b in range(B):
        d = data[b % len(data)]
        ref = _ref("batch", key + (b % min(B, 3),), rho)
        r0 = int(np.flatnonzero(np.isfinite(d["lbA"]) & np.isfinite(d["ubA"]) & (d["lbA"] < d["ubA"]))[0])
        lo = ref.l.copy(); lo[r0] = ref.u[r0] + 1.0
        assert (st[b]["admmIter"], st[b]["qpSolverExitFlag"], st[b]["returnValue"]) == (0, 2, 203), st[b]
        ra = bt.read_admm(b)
        assert first[b]["kReady"] == 1 and ra["kReady"] == 0 and ra["rhoAdmm"] == ref.rho0 and ra["sigma"] == ref.sigma
        assert np.array_equal(ra["l"][:ref.mE], lo) and np.array_equal(ra["u"][:ref.mE], ref.u)
        assert np.array_equal(ra["rhov"][:ref.mE], R.rho_vector(hip.default_options(admmRho=rho), ref.scale, lo, ref.u))
    bt.close()


# ---- F: the certificates with box rows -------------------------------------------------------------------------------------------------------
F_SEED, F_N, F_M = R.F_SEED, R.F_N, R.F_M      # chosen on the CPU: tests/test_admm_ref.py asserts the clearance of the reference iterates


@pytest.mark.parametrize("which,flag,iters", [(0, 4, 70), (1, 5, 30)])
def test_certificates_with_box_rows(hip, which, flag, iters):
    """n = 150 (np = 256), 180 rows and a box on half the variables: one QP is infeasible (10 + 20 + 40 iterations until the certificate
    holds), one unbounded (10 + 20).  The device's flag, and the reference's predicate evaluated on the device's own dy and dx."""
    d = P.certificate_qps(F_SEED, F_N, F_M, box=True)[which]
    n = F_N
    q = hip.SubsolverHIP(n, F_M, d["Q"], d["A"])
    r = q.solve(True, d["g"], d["lbA"], d["ubA"], np.zeros(n), None, d["lb"], d["ub"])
    ra, cnt = q.read_admm(), q.counters()
    q.close()
    assert (r[0], r[2]) == (203, flag) and cnt["admm"] == iters and ra["np"] == 256
    E, l, u = R.stacked(dict(d, n=n))
    mE = len(l)
    assert ra["mE"] == mE == F_M + n - n // 2 and np.array_equal(ra["l"][:mE], l) and np.array_equal(ra["u"][:mE], u)
    got, comps = R.certificate(d["Q"], E, d["g"], l, u, ra["dy"][:mE], ra["dx"][:n])
    clear = R.clearance(comps)
    print(f"    flag {got}, {len(comps)} comparisons, the closest a factor {clear:.3g} from its threshold")
    assert got == flag and clear >= 10.0
