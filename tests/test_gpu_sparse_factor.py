"""The KKT factorisations and solves of the sparse arm (lcqp_sparse_factor.hpp: sp_factor_reg, sp_factor_lds, sp_general_*, band_sweep, the
sp_border_* routines, sp_solve) through lcqp_hip_sparse_kkt_probe, held to the plain numpy references of tests/sparse_kkt_ref.py -- never to
the oracle, and with nothing between the engine and the assertion: one solve per right-hand side, no refinement, no polish.

Every solve is held componentwise to  |b - K x| <= (6 N + 8) eps (Wm |x| + |b|),  Wm = |L| |D| |L'| of a long-double LDL' without pivoting
(float64 above N = 1024) in the ordering the device reports, the residual in long double (sparse_kkt_ref.py has the reasoning).  Every
assertion goes through _chk(), which prints worst error / bound (`python -m pytest tests/test_gpu_sparse_factor.py -m gpu -s`).  A ratio
above 0.1 has to be explained here before it is accepted; the bound does not move.  For the bordered band the factor is a block elimination:
where the device exceeds the scalar bound, the float64 block elimination of sparse_kkt_ref.bordered_ref is measured on the same input and
the device gets 8 x that reference's own worst ratio.  tests/test_sparse_kkt_ref.py shows on the CPU that a float64 LDL' stays inside the
bound on these inputs and that the growth max(Wm |x|) / max(|K| |x|) stays under 1e6 for them (which regularisation pair goes with which
working set follows from that: sparse_kkt_ref.FAMILIES).

Worst error / bound on an MI355X (30 tests, 30 s of wall time, most of it long-double products):

    FACTOR  register band G = 8     2.0e-3 (N = 112)   2.2e-4 (N = 896)      forced G = 16, 32, 64 on the same problems   2.2e-3
            register band G = 16    2.2e-3             2.6e-4
            LDS window    G = 32    3.4e-3             3.4e-4                circle(20), a band of half width 19          1.5e-3
            bordered band           1.2e-3 (1 row)     1.1e-3 (3 rows)       circle(100), two variables in the border     3.1e-4
            general LDL'            2.4e-3 (dense rows, 58 fronts)  5.2e-2 (12 x 12 grid, 9 fronts)  3.2e-4 (30 x 30 grid, 63 fronts)  2.5e-3 (banded, hook)
    STORED  polish and ADMM slots   2.5e-3 (small)  2.9e-4 (mid)  3.7e-4 (circle 100)  2.8e-3 / 4.6e-4 (grids)
            bordered band with 3 coupling rows, polish slot: 0.28 of the WIDENED bound in three instances.  There the solutions of unit
            vectors decay to 1e-200 and below along the band, and the correction b -= W' x_border of the block elimination leaves absolute
            errors of 1e-17 |x_border| at such entries: the float64 block elimination of bordered_ref itself is 1.2e1 .. 5.1e8 times above
            the scalar bound on the same inputs, the device stays below 8 x that (the rule above).  The FACTOR cases of the same pattern and the
            ADMM slot stay inside the scalar bound (1.1e-3).
No ratio against the scalar bound is above 0.1; the largest, 5.2e-2, is the general LDL' on the 12 x 12 grid with every row in the set at the
safe polish pair.  In the device's nested-dissection ordering that case has a growth of 3e9 (printed beside every ratio; 6e1 in the scipy
ordering of tests/test_sparse_kkt_ref.py, which is the one the growth cap is asserted in): rows are eliminated in front of their variables, the
computed factor then differs from the exact one W is taken from in more than the last bits, and the bound is loose there.  The same holds for
the polish pairs on circle(20) (growth 4e10 / 4e15 in the device's ordering, ratios 1.5e-3): for those two patterns the tight check is the
ADMM-like pair on the same sets (growth below 1e4).  Every other case has a ratio below 4e-3.

Residual and bound are compared in long double: along a band the solutions underflow float64's normal range, and a bound rounded to zero
would fail an exact answer.
"""
import numpy as np
import pytest

import sparse_kkt_ref as R

pytestmark = pytest.mark.gpu

OPT = dict(perturbStep=0, printLevel=0)


def _chk(name, err, bound):
    """every entry of err within bound; the worst ratio is printed"""
    err = np.asarray(err, dtype=R.LD); bound = np.broadcast_to(np.asarray(bound, dtype=R.LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    worst = float(ratio.max()) if err.size else 0.0
    print(f"    {name}: worst error / bound = {worst:.3e}")
    assert np.isfinite(err).all() and (err <= bound).all(), f"{name}: worst error / bound = {worst:.3e}"
    return worst


def _handle(hip, inst, **okw):
    """a batch loaded with `inst` and run once (the probe needs a completed run)"""
    d0 = inst[0]
    sb = hip.SparseBatchLCQP(len(inst), d0["nV"], d0["nC"], d0["nComp"], d0["Q"], d0["E"], opt=hip.default_options(**dict(OPT, **okw)))
    kw = dict(lbA=np.stack([d["lbA"] for d in inst]), ubA=np.stack([d["ubA"] for d in inst]))
    if "x0" in d0:
        kw["x0"] = np.stack([d["x0"] for d in inst])
    assert sb.load(0, len(inst), np.stack([d["Q"].data for d in inst]), np.stack([d["g"] for d in inst]), np.stack([d["E"].data for d in inst]), **kw) == 0
    sb.run()
    sb.synchronize()
    return sb


def _rhs(N, B, unit=True):
    """[B][nrhs][N] for the device and the columns per instance"""
    cols = [R.rhs_set(N, 7 + b, unit=unit) for b in range(B)]
    return np.stack([c.T for c in cols]), cols


_LDL = {}


def _reference(key, K):
    """(L, D, Wm) of K, computed once per matrix"""
    if key not in _LDL:
        _LDL[key] = R.ldl_nopivot(K, R.ref_dtype(K.shape[0]))
    return _LDL[key]


def check_solves(name, K, perm, sol, cols, kb=0, key=None):
    """sol [nrhs][N] (node order) of the right-hand sides cols [N][nrhs] against the matrix K (node order), in the device's ordering"""
    Kp = K[np.ix_(perm, perm)]
    _, _, Wm = _reference(key, Kp) if key is not None else R.ldl_nopivot(Kp, R.ref_dtype(len(perm)))
    X, B = sol.T[perm], cols[perm]
    res, bound = R.residual_and_bound(Kp, Wm, X, B)
    if kb and not (res <= bound).all():
        rr, rb = R.residual_and_bound(Kp, Wm, R.bordered_ref(Kp, kb, B), B)
        ref_ratio = float(np.where(rb > 0, rr / np.where(rb > 0, rb, 1), 0).max())
        print(f"    {name}: above the scalar bound; the float64 block elimination's own worst error / bound = {ref_ratio:.3e}")
        bound = bound * R.LD(max(1.0, 8.0 * ref_ratio))
    gr = float(R.growth(Kp, Wm, X).max())
    return _chk(f"{name} [growth {gr:.1e}]", res, bound), gr


def factor_family(hip, name, sb=None, inst=None, close=True):
    """FACTOR mode over the plan of a family: the bound for every instance, and the rows outside the set"""
    fam = R.FAMILIES[name]
    inst = inst or fam["make"](fam["B"])
    sb = sb or _handle(hip, inst)
    B, N, n = len(inst), sb.nV + sb.m, sb.nV
    perm = sb.ordering()
    opt = hip.default_options()
    rhs, cols = _rhs(N, B)
    worst, sols = 0.0, {}
    for rname, per in R.plan(name, inst):
        regs = [R.regularisations(opt, R.scale_of(d), sb.m)[rname] for d in inst]
        use = np.stack([u for _, u in per])
        sol = sb.kkt_probe(rhs, dprim=[r[0] for r in regs], ddual=np.stack([r[1] for r in regs]), use=use)
        sols[rname] = sol
        for b, d in enumerate(inst):
            K = R.kkt_dense(d, regs[b][0], regs[b][1], use[b])
            w, gr = check_solves(f"{name} / {rname} / instance {b} ({per[b][0]})", K, perm, sol[b], cols[b], kb=sb.border(), key=(name, rname, b, tuple(perm[:8])))
            worst = max(worst, w)
            out = np.flatnonzero(use[b] == 0)
            assert np.array_equal(sol[b][:, n + out], -rhs[b][:, n + out]), (name, rname, b)      # pivot -1, no entries: exactly -b_r
    print(f"  {name}: worst error / bound over the family = {worst:.3e}")
    if close:
        sb.close()
    return sols, rhs


# ---- FACTOR mode: every engine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lanes,engine", [("small", 8, "reg"), ("mid", 8, "reg"), ("small span 10", 16, "reg"), ("mid span 10", 16, "reg"),
                                               ("small span 18", 32, "lds"), ("mid span 18", 32, "lds")])
def test_factor_band_engines(hip, name, lanes, engine):
    """families 1 - 3: the register engine at G = 8 and G = 16, the LDS window beyond (N = 112 is no multiple of 64 and B = 11 leaves a ragged
    second wavefront; N = 896 has many 64-blocks: the gather-ahead and the ring prefetch wrap)"""
    fam = R.FAMILIES[name]
    inst = fam["make"](fam["B"])
    sb = _handle(hip, inst)
    assert (sb.lanes() == lanes if engine == "reg" else sb.lanes() in (32, 64)) and sb.bandwidth() < sb.lanes() and sb.border() == 0 and sb.fronts() == 0
    factor_family(hip, name, sb=sb, inst=inst)


@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_factor_forced_lane_widths_agree(hip, monkeypatch, lanes):
    """family 4: LCQP_SPARSE_LANES forces the wider groups on the span-6 problems; every width holds the bound, and two widths agree within
    the sum of their bounds (not in bits: the engines sum in other orders)"""
    inst = R.FAMILIES["small"]["make"](R.FAMILIES["small"]["B"])
    base, rhs = factor_family(hip, "small", inst=inst)
    monkeypatch.setenv("LCQP_SPARSE_LANES", str(lanes))
    sb = _handle(hip, inst)
    assert sb.lanes() == lanes and sb.bandwidth() == 7
    perm = sb.ordering()
    wide, _ = factor_family(hip, "small", sb=sb, inst=inst)
    opt = hip.default_options()
    for rname, per in R.plan("small", inst):
        for b, d in enumerate(inst):
            dp, dd = R.regularisations(opt, R.scale_of(d), sb.m)[rname]
            Kp = R.kkt_dense(d, dp, dd, per[b][1])[np.ix_(perm, perm)]
            L, D, Wm = _reference(("small", rname, b, tuple(perm[:8])), Kp)
            X0, X1, Bc = base[rname][b].T[perm], wide[rname][b].T[perm], rhs[b].T[perm]
            # K (x0 - x1) = r1 - r0 with both residuals inside their bounds: |K (x0 - x1)| <= bound(x0) + bound(x1)
            diff = np.abs(Kp.astype(R.LD) @ (X0.astype(R.LD) - X1.astype(R.LD)))
            bnd = R.LD((6 * len(perm) + 8) * R.EPS) * (Wm.astype(R.LD) @ (np.abs(X0) + np.abs(X1)).astype(R.LD) + 2 * np.abs(Bc).astype(R.LD))
            assert (diff <= bnd).all(), (lanes, rname, b, float((diff / bnd).max()))


@pytest.mark.parametrize("name,kb", [("coupled 1", 1), ("coupled 3", 3), ("circle 20", 0), ("circle 100", 3)])
def test_factor_bordered_band(hip, name, kb):
    """family 5: band + border; the sets with each coupling row in and out.  The pattern analysis takes circle(20) as a plain band of half
    width 19 (lane groups of 32, the LDS window): it stays as a case of that engine, and circle(100) -- the size of the reference's example --
    is the case with the two shared variables and the coupling row in the border."""
    fam = R.FAMILIES[name]
    inst = fam["make"](fam["B"])
    sb = _handle(hip, inst)
    print(f"  {name}: border {sb.border()}, bandwidth {sb.bandwidth()}, lanes {sb.lanes()}")
    assert sb.fronts() == 0 and sb.border() == kb
    if name == "circle 100":
        assert {0, 1} <= set(sb.ordering()[-kb:].tolist())      # the two shared variables sit in the border
    factor_family(hip, name, sb=sb, inst=inst)


@pytest.mark.parametrize("name", ["dense rows", "grid 12", "grid 30"])
def test_factor_general_ldl(hip, monkeypatch, name):
    """families 6 and 7: one front of more than 64 rows through the front buffer; several fronts.  (The 12 x 12 grid fits a band of half
    width below 64, which the pattern analysis prefers, and so does the 30 x 30 one: LCQP_SPARSE_GENERAL=1 sends them to the general LDL'.)"""
    if name.startswith("grid"):
        monkeypatch.setenv("LCQP_SPARSE_GENERAL", "1")
    fam = R.FAMILIES[name]
    inst = fam["make"](fam["B"])
    sb = _handle(hip, inst)
    assert sb.lanes() == 64 and sb.border() == 0 and (sb.fronts() >= 1 if name == "dense rows" else sb.fronts() > 1)
    print(f"  {name}: {sb.fronts()} fronts")
    factor_family(hip, name, sb=sb, inst=inst)


def test_factor_general_ldl_on_the_banded_pattern(hip, monkeypatch):
    """family 8: LCQP_SPARSE_GENERAL=1 on (64, 32, 8)"""
    monkeypatch.setenv("LCQP_SPARSE_GENERAL", "1")
    inst = R.FAMILIES["small general"]["make"](R.FAMILIES["small general"]["B"])
    sb = _handle(hip, inst)
    assert sb.fronts() >= 1 and sb.lanes() == 64
    factor_family(hip, "small general", sb=sb, inst=inst)


# ---- FACTOR mode: what must hold to the bit ------------------------------------------------------------------------------------------------
def _probe_args(hip, name, inst, rname):
    opt = hip.default_options()
    per = dict(R.plan(name, inst))[rname]
    m = inst[0]["E"].shape[0]
    regs = [R.regularisations(opt, R.scale_of(d), m)[rname] for d in inst]
    return dict(dprim=np.array([r[0] for r in regs]), ddual=np.stack([r[1] for r in regs]), use=np.stack([u for _, u in per]))


@pytest.mark.parametrize("name,env", [("small", None), ("small span 18", None), ("coupled 3", None), ("small general", "LCQP_SPARSE_GENERAL")])
def test_factor_bits_do_not_depend_on_the_batch_or_the_call(hip, monkeypatch, name, env):
    """instance b of a batch with mixed sets = the same instance in a batch of one; nrhs = 8 = eight calls with nrhs = 1; the second of two
    FACTOR calls with different sets = the same call on a fresh handle (nothing of the first factor or window survives)"""
    if env:
        monkeypatch.setenv(env, "1")
    fam = R.FAMILIES[name]
    inst = fam["make"](fam["B"])
    B, N = len(inst), inst[0]["nV"] + inst[0]["E"].shape[0]
    rhs, _ = _rhs(N, B, unit=False)
    rhs = np.ascontiguousarray(rhs[:, :8])
    a_admm, a_safe = _probe_args(hip, name, inst, "admm"), _probe_args(hip, name, inst, "safe")
    sb = _handle(hip, inst)
    first = sb.kkt_probe(rhs, **a_admm)
    second = sb.kkt_probe(rhs, **a_safe)
    singles = np.concatenate([sb.kkt_probe(np.ascontiguousarray(rhs[:, k:k + 1]), **a_safe) for k in range(8)], axis=1)
    assert np.array_equal(singles, second)
    sb.close()
    fresh = _handle(hip, inst)
    assert np.array_equal(fresh.kkt_probe(rhs, **a_safe), second) and not np.array_equal(first, second)
    fresh.close()
    for b in (0, B // 2, B - 1):
        one = _handle(hip, inst[b:b + 1])
        sol = one.kkt_probe(rhs[b:b + 1], **{k: v[b:b + 1] for k, v in a_admm.items()})
        assert np.array_equal(sol[0], first[b]), (name, b)
        one.close()


@pytest.mark.parametrize("name", ["small", "small span 10"])
def test_factor_bit_set_or_flags_give_the_same_bits(hip, monkeypatch, name):
    """LCQP_SPARSE_NOBITS=1: the working set read from memory instead of the bit set in LDS (G = 8 and 16)"""
    fam = R.FAMILIES[name]
    inst = fam["make"](fam["B"])
    N = inst[0]["nV"] + inst[0]["E"].shape[0]
    rhs, _ = _rhs(N, len(inst), unit=False)
    args = _probe_args(hip, name, inst, "admm")
    sb = _handle(hip, inst)
    bits = sb.kkt_probe(rhs, **args)
    sb.close()
    monkeypatch.setenv("LCQP_SPARSE_NOBITS", "1")
    sb = _handle(hip, inst)
    assert np.array_equal(sb.kkt_probe(rhs, **args), bits)
    sb.close()


def test_factor_mode_invalidates_the_stored_solution(hip):
    """a FACTOR call overwrites the polish factor: sensitivity then answers LCQP_LCQPOBJECT_NOT_SETUP, a warm resolve starts every instance
    cold (the bits and iterate counts of the first run), and the next STORED call on the polish slot is served again"""
    name = "small"
    inst = R.FAMILIES[name]["make"](R.FAMILIES[name]["B"])
    sb = _handle(hip, inst)
    x0, y0, st0 = sb.solution()
    N = sb.nV + sb.m
    rhs, _ = _rhs(N, len(inst), unit=False)
    v = np.ones((len(inst), sb.nV))
    sb.sensitivity(v)
    sb.kkt_probe(rhs, **_probe_args(hip, name, inst, "admm"))
    with pytest.raises(RuntimeError, match="code 300"):
        sb.sensitivity(v)
    with pytest.raises(RuntimeError, match="code 300"):
        sb.kkt_probe(rhs, which=0)
    sb.resolve(warm=True)
    x1, y1, st1 = sb.solution()
    assert np.array_equal(x1, x0) and np.array_equal(y1, y0)
    assert [s["iterTotal"] for s in st1] == [s["iterTotal"] for s in st0]
    assert sb.launch_counts() == (1, 2)
    sb.sensitivity(v)
    sb.kkt_probe(rhs, which=0)
    sb.close()


# ---- STORED mode: the factors a run leaves -----------------------------------------------------------------------------------------------------
def _admm_weights(opt, d, lbA, ubA):
    """1 / rho_r as k_sparse_setup forms it: rho = admmRho scale; a free row 1e-6 rho, an equality rho rhoEqMult, anything else rho"""
    m = d["E"].shape[0]; nC = d["nC"]
    lo = np.concatenate([lbA, np.zeros(m - nC)]); hi = np.concatenate([ubA, np.full(m - nC, np.inf)])
    rho = opt.admmRho * R.scale_of(d)
    rv = np.where(np.isinf(lo) & np.isinf(hi), 1e-6 * rho, np.where(lo == hi, rho * opt.rhoEqMult, rho))
    return 1.0 / rv


@pytest.mark.parametrize("name", ["small", "mid", "coupled 3", "circle 100", "grid 12", "grid 30"])
def test_stored_factors_after_a_run(hip, monkeypatch, name):
    """families 1, 5, 7 after run(): the polish factor is the factor of its record (the set equals side != 0 of sensitivity(), the pair is one
    of the instance's two levels), the ADMM factor that of [Q + sigma I, E'; E, -diag(1 / rhov)]; then an update that turns inequality rows
    of SOME instances into equalities and a cold resolve: the ADMM factor of every instance -- those k_sparse_refresh refactorised and those
    it left in place -- is the factor of the new weights (a stale factor fails here)"""
    if name.startswith("grid"):
        monkeypatch.setenv("LCQP_SPARSE_GENERAL", "1")
    fam = R.FAMILIES[name]
    inst = fam["make"](fam["B"])
    sb = _handle(hip, inst)
    assert (sb.fronts() > 1) == fam["general"]
    opt = hip.default_options()
    B, N, m, n = len(inst), sb.nV + sb.m, sb.m, sb.nV
    perm = sb.ordering()
    _, _, st = sb.solution()
    rhs, cols = _rhs(N, B, unit=(name != "mid"))
    _, _, side, info = sb.sensitivity(np.ones((B, n)))
    sol, rec = sb.kkt_probe(rhs, which=0)
    worst = 0.0
    for b, d in enumerate(inst):
        if st[b]["returnValue"] != 0:
            continue
        sc = R.scale_of(d)
        assert np.array_equal(rec["use"][b], (side[b] != 0).astype(np.int32)), (name, b)
        levels = [(opt.proxBig * sc, 1e-9 / sc), (opt.proxSmall * sc, 1e-14 / sc)]
        assert (rec["dprim"][b], rec["ddual"][b][0]) in levels and (rec["ddual"][b] == rec["ddual"][b][0]).all(), (name, b, rec["dprim"][b], levels)
        K = R.kkt_dense(d, rec["dprim"][b], rec["ddual"][b], rec["use"][b])
        w, gr = check_solves(f"{name} / stored polish / instance {b}", K, perm, sol[b], cols[b], kb=sb.border())
        print(f"      growth {gr:.2e}, {int(rec['use'][b].sum())} rows, level {levels.index((rec['dprim'][b], rec['ddual'][b][0]))}")
        worst = max(worst, w)
    assert st[0]["returnValue"] == 0
    lbA = np.stack([d["lbA"] for d in inst]); ubA = np.stack([d["ubA"] for d in inst])

    def admm_slot(tag, lbA, ubA):
        nonlocal worst
        sol, rec = sb.kkt_probe(rhs, which=1)
        for b, d in enumerate(inst):
            dd = _admm_weights(opt, d, lbA[b], ubA[b])
            assert rec["dprim"][b] == opt.admmSigma * R.scale_of(d) and np.array_equal(rec["ddual"][b], dd) and rec["use"][b].all(), (name, tag, b)
            K = R.kkt_dense(d, rec["dprim"][b], dd, np.ones(m, dtype=np.int32))
            w, _ = check_solves(f"{name} / stored ADMM {tag} / instance {b}", K, perm, sol[b], cols[b], kb=sb.border())
            worst = max(worst, w)
    admm_slot("after run", lbA, ubA)
    # rows of some instances become equalities; the others keep their data
    changed = [b for b in range(B) if b % 2 == 0]
    lb2, ub2 = lbA.copy(), ubA.copy()
    for b in changed:
        rows = np.flatnonzero(np.isfinite(lbA[b]) & np.isfinite(ubA[b]) & (lbA[b] < ubA[b]))[b % 3::5]
        if rows.size == 0:      # (the circle example has equality rows only: nothing to turn)
            continue
        mid = 0.5 * (lbA[b][rows] + ubA[b][rows])
        lb2[b][rows] = mid; ub2[b][rows] = mid
        kw = dict(x0=inst[b]["x0"][None]) if "x0" in inst[b] else {}
        assert sb.update(b, 1, inst[b]["g"][None], lbA=lb2[b][None], ubA=ub2[b][None], **kw) == 0
    if len(changed) < B and not np.array_equal(lb2, lbA):
        sb.resolve(warm=False)
        sb.synchronize()
        assert sb.launch_counts() == (1, 2)
        admm_slot("after update and resolve", lb2, ub2)
    print(f"  {name}: worst error / bound of the stored factors = {worst:.3e}")
    sb.close()
