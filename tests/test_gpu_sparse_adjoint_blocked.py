"""Panels with gradients on y and the dual rows of the solution Jacobian on the sparse arm (lcqp_hip_sparse_adjoint_blocked,
lcqp_hip_sparse_jacobian_duals, SparseBatchLCQPLayer.jacobian_full; DESIGN.md section 3a'''', "The sparse arm: panels with gradients on y").

Convention (include/lcqp_hip.h): K0 [d; mu] = [v_x; -v_y|_W], K0 = [[Q, E_W'], [E_W, 0]], dg = -d, db_W = mu; y as solution() returns it.

1  against numpy on the device's own working set (kkt_adjoint_reference: float64 LU refined with long-double residuals); the bound of
   tests/test_gpu_sparse_adjoint.py::bound_1, b1 = 1e-12 (nV + |W|) cond_2(K0) max(|v_x|_inf, |v_y|_inf); E_r dg = v_y[r] on every row r of W to
   b1 |E_r|_1; db exactly 0.0 outside W.
2  against the loop of vector adjoint(vx_k, vy_k) calls: b1; bit equality printed, asserted on the fallback.
3  VY = None: the bits of sensitivity_blocked(VX); VX = None: the bits of an explicit zero VX.
4  column independence, bit for bit: sub-calls of widths 1, 3, P, P + 1, a permutation, a repeated call, exact zeros for the zero pair.
5  entries of vy outside W replaced by NaN and by 1e300: the same bits.
6  jacobian_duals: rows of W against the blocks (K0^-1)_{lambda x} and -(K0^-1)_{lambda lambda} of a float64 inverse, the bound of check 4 of
   tests/test_gpu_sparse_sensitivity_blocked.py (b1 with |v| = 1); rows outside W exactly zero; Jyg[r][j] against jacobian()'s Jb[j][r]; the
   rows equal adjoint_blocked(None, unit VY) (to the bit on the band engines); four chunkings give the same bits.
7  central differences of l = v_x.x + v_y.y, h = 1e-6, through warm re-solves in g and in the bounds two active rows of A sit on; the bound
   of tests/test_gpu_adjoint.py::fd_bounds (the construction tests/test_gpu_adjoint_blocked.py uses for its y part), x part + y part, from
   the stationarity tolerance.  v_y is zero outside W: those duals are not functions of the data on the branch.
8  the calls change nothing.      9  state errors and a failed instance.      10  torch.

One solve per case (solved_case); every figure is printed before it is asserted.  The 44 x 44 grid serves checks 1 and 6 only, its dual
Jacobian for one instance."""
import ctypes
import functools

import numpy as np
import pytest

from batch_helpers import LD, assert_same_bits, environment, handle, result, update_all
from problems import MID, OPT, SMALL, instances, moved
from test_gpu_sparse_sensitivity import CASES as VECTOR_CASES, instances_of

pytestmark = pytest.mark.gpu

H_FD = 1e-6
NOT_SETUP, INVALID_ARGUMENT = 300, 100
FALLBACK, GENERAL_PANEL, GRID = "small, general ldl", "small, general ldl, panel", "grid, general ldl"
#        case of tests/test_gpu_sparse_sensitivity.py, set_general_panel
CASES = {"small": ("small", False), "lanes 32": ("lanes 32", False), "pools of 4": ("pools of 4", False),
         "bordered circle": ("bordered circle", False), "mid": ("mid", False),
         FALLBACK: ("small, general ldl", False), GENERAL_PANEL: ("small, general ldl", True), GRID: ("grid, general ldl", True)}
KEYS = [k for k in CASES if k != GRID]      # the cases of every check; GRID: checks 1 and 6


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def kkt_adjoint_reference(Q, EW, VX, VYW):
    """dg [k][n], mu [k][|W|] of K [d; mu] = [vx; -vy_W] for the k pairs in the rows of VX, VYW: float64 LU, refined three times with
    long-double residuals; cond_2(K) and the plain float64 inverse of K with them"""
    n, m = Q.shape[0], EW.shape[0]
    K = np.zeros((n + m, n + m)); K[:n, :n] = Q; K[:n, n:] = EW.T; K[n:, :n] = EW
    rhs = np.concatenate([VX.T, -VYW.T])
    Kinv = np.linalg.solve(K, np.eye(n + m))
    sol = np.linalg.solve(K, rhs)
    KL, rl, sl = K.astype(LD), rhs.astype(LD), sol.astype(LD)
    for _ in range(3):
        sl = sl + np.linalg.solve(K, (rl - KL @ sl).astype(np.float64)).astype(LD)
    sol = sl.astype(np.float64)
    ev = np.abs(np.linalg.eigvalsh(K))
    return -sol[:n].T, sol[n:].T, float(ev.max() / ev.min()), Kinv


def fd_bounds(tol, Q, EW, vx, vyW):
    """tests/test_gpu_adjoint.py::fd_bounds: the error of a central difference of x* resp. y* whose solves stop at the stationarity tolerance"""
    ev = np.linalg.eigvalsh(Q)
    bx = tol * np.abs(vx).sum() / (H_FD * ev[0])
    by = 0.0
    if len(EW):
        by = tol * np.sqrt(len(vx) * ev[-1] / ev[0]) * np.abs(vyW).sum() / (H_FD * np.linalg.svd(EW, compute_uv=False)[-1])
    return bx, by


def unit_vy(side):
    """VY [B][m][m]: pair r of instance b is e_r (every instance gets every row; outside its W the pair is a zero pair by definition)"""
    B, m = side.shape
    return np.ascontiguousarray(np.broadcast_to(np.eye(m), (B, m, m)))


@functools.lru_cache(maxsize=None)
def solved_case(key):
    import lcqpow_amd as hip
    base, switch = CASES[key]
    ds = instances_of(base)
    B, n = len(ds), ds[0]["nV"]
    with environment(VECTOR_CASES[base][1]):
        sb = handle(hip, ds, hip.default_options(**OPT))
    if switch:
        sb.set_general_panel(True)
    P, m = sb.sens_panel(), sb.m
    c = dict(ds=ds, engine=dict(lanes=sb.lanes(), fronts=sb.fronts(), border=sb.border(), panel=P), P=P)
    sb.run()
    c["x"], c["y"], c["st"] = sb.solution()
    nrhs = 2 * P + 3 if P else 5
    rng = np.random.default_rng(79)
    VX, VY = rng.standard_normal((B, nrhs, n)), rng.standard_normal((B, nrhs, m))
    VY[:, 0] = 0.0; VX[:, 1] = 0.0          # a pair without vy, a pair without vx
    VX[:, 2] = 0.0; VY[:, 2] = 0.0          # a zero pair
    c.update(VX=VX, VY=VY)
    counts = sb.launch_counts()
    c["blk"] = sb.adjoint_blocked(VX, VY)
    c["ms"] = sb.sensitivity_kernel_ms()
    side = c["blk"][2]
    grid = key == GRID
    # the dual Jacobian: unchunked (the grid: one instance), a sub-range, one item per launch, a cap that leaves a partial last chunk
    cnt = 1 if grid else B
    c["jd"] = sb.jacobian_duals(count=cnt)
    c["jd_ms"] = sb.sensitivity_kernel_ms()
    c["jac"] = sb.jacobian(count=cnt)
    if not grid:
        c["vec"] = [sb.adjoint(np.ascontiguousarray(VX[:, k]), np.ascontiguousarray(VY[:, k]), matrices=()) for k in range(nrhs)]
        c["novy"] = sb.adjoint_blocked(VX, None); c["sens"] = sb.sensitivity_blocked(VX)
        c["novx"] = sb.adjoint_blocked(None, VY); c["zerovx"] = sb.adjoint_blocked(np.zeros_like(VX), VY)
        widths = sorted({1, 3, max(P, 1), max(P, 1) + 1} & set(range(1, nrhs)))
        c["sub"] = {w: sb.adjoint_blocked(np.ascontiguousarray(VX[:, 1:1 + w]), np.ascontiguousarray(VY[:, 1:1 + w])) for w in widths}
        c["perm"] = rng.permutation(nrhs)
        c["permuted"] = sb.adjoint_blocked(np.ascontiguousarray(VX[:, c["perm"]]), np.ascontiguousarray(VY[:, c["perm"]]))
        c["again"] = sb.adjoint_blocked(VX, VY)
        outside = np.broadcast_to((side == 0)[:, None, :], VY.shape)
        c["nan"] = sb.adjoint_blocked(VX, np.where(outside, np.nan, VY))
        c["huge"] = sb.adjoint_blocked(VX, np.where(outside, 1e300, VY))
        c["units"] = sb.adjoint_blocked(None, unit_vy(side))
        c["jd_nobounds"] = sb.jacobian_duals(bounds=False)
        c["jd_range"] = sb.jacobian_duals(first=1, count=min(2, B - 1))
        c["jd_one"] = sb.jacobian_duals(_staging_bytes=1)
        items = B * (-(-m // P)) if P else int(np.count_nonzero(side.any(axis=0)))
        item_bytes = 8 * (P * (n + m) + P * (n + m + 64 + 2 * n + m)) + 4 * P if P else 8 * B * 2 * (n + m)      # an upper estimate of one item's staging
        per_chunk = max(2, (items + 2) // 3 + 1)
        c["partial"] = (items, per_chunk)
        c["jd_partial"] = sb.jacobian_duals(_staging_bytes=item_bytes * per_chunk)
    assert sb.launch_counts() == counts
    sb.close()
    return c


@functools.lru_cache(maxsize=None)
def reference_of(key):
    c = solved_case(key)
    out, seen = [], {}
    for b, d in enumerate(c["ds"]):
        W = np.flatnonzero(c["blk"][2][b])
        ident = (id(d["Q"]), id(d["E"]), W.tobytes())      # the instances of the grid are one problem: one factorisation
        if ident not in seen:
            seen[ident] = d["E"].toarray()
        E = seen[ident]
        dg, mu, cond, Kinv = kkt_adjoint_reference(d["Q"].toarray(), E[W], c["VX"][b], c["VY"][b][:, W])
        out.append(dict(E=E, W=W, dg=dg, mu=mu, cond=cond, Kinv=Kinv))
    return out


def bound_1(c, r, b, vinf=None):
    vinf = max(np.abs(c["VX"][b]).max(), np.abs(c["VY"][b]).max()) if vinf is None else vinf
    return 1e-12 * (c["ds"][b]["nV"] + len(r["W"])) * r["cond"] * vinf


def test_the_cases_reach_the_engines(hip):
    eng = {k: solved_case(k)["engine"] for k in CASES}
    print(" ", eng)
    assert eng["small"]["lanes"] == 8 and eng["lanes 32"]["lanes"] == 32 and eng["bordered circle"]["border"] > 0
    assert all(eng[k]["panel"] in (4, 8) for k in CASES if k != FALLBACK)
    assert eng[FALLBACK]["fronts"] > 0 and eng[FALLBACK]["panel"] == 0 and eng[GENERAL_PANEL]["fronts"] > 0
    assert eng[GRID]["fronts"] > 4 and eng[GRID]["lanes"] == 64


# ---- 1: against numpy on the device's own working set ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_against_numpy_on_the_working_set(hip, key):
    c, refs = solved_case(key), reference_of(key)
    dg, db, side, info = c["blk"]
    nrhs, m = c["VX"].shape[1], side.shape[1]
    print(f"  {key}: {nrhs} pairs per instance, kernel time {c['ms']:.3f} ms")
    worst = 0.0
    for b, r in enumerate(refs):
        W = r["W"]
        assert c["st"][b]["returnValue"] == 0 and not (info[b] & 1)
        b1 = bound_1(c, r, b)
        dbr = np.zeros((nrhs, m)); dbr[:, W] = r["mu"]
        e_g, e_b = np.abs(dg[b] - r["dg"]).max(), np.abs(db[b] - dbr).max()
        rows = np.abs(dg[b] @ r["E"][W].T - c["VY"][b][:, W]) / np.abs(r["E"][W]).sum(axis=1)      # |E_r dg - vy_r| / |E_r|_1, [nrhs][|W|]
        e_r = rows.max(initial=0.0)
        worst = max(worst, max(e_g, e_b, e_r) / b1)
        print(f"  {key} instance {b}: |W| = {len(W)}, cond(K0) = {r['cond']:.3g}, err dg {e_g:.3g}, err db {e_b:.3g}, "
              f"worst row of E_W dg = vy_W {e_r:.3g}, bound {b1:.3g}, info {info[b]}")
        assert e_g <= b1 and e_b <= b1 and e_r <= b1
        outside = np.ones(m, dtype=bool); outside[W] = False
        assert np.all(db[b][:, outside] == 0.0) and np.any(db[b][:, W] != 0.0)
        assert (info[b] & ~4) == 0 if key == "bordered circle" else info[b] == 0
    print(f"  {key}: worst error / bound = {worst:.3g}")


# ---- 2: against the loop of vector calls -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_against_the_vector_adjoint(hip, key):
    c, refs = solved_case(key), reference_of(key)
    dg, db, side, info = c["blk"]
    vdg = np.stack([v["dg"] for v in c["vec"]], axis=1); vdb = np.stack([v["db"] for v in c["vec"]], axis=1)
    for b, r in enumerate(refs):
        b1 = bound_1(c, r, b)
        e_g, e_b = np.abs(dg[b] - vdg[b]).max(), np.abs(db[b] - vdb[b]).max()
        print(f"  {key} instance {b}: max|blocked - vector| dg {e_g:.3g} db {e_b:.3g} (bound {b1:.3g})")
        assert e_g <= b1 and e_b <= b1
    assert all(np.array_equal(v["side"], side) for v in c["vec"])
    equal = np.array_equal(dg, vdg) and np.array_equal(db, vdb)
    print(f"  {key}: the bits of the blocked call equal the vector kernel's: {equal}")
    if key == FALLBACK:
        assert equal


# ---- 3: absent blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_absent_blocks(hip, key):
    c = solved_case(key)
    a, z = same(c["novy"], c["sens"]), same(c["novx"], c["zerovx"])
    print(f"  {key}: VY = None gives the bits of sensitivity_blocked: {a}; VX = None gives the bits of a zero VX: {z}")
    assert a and z and np.any(c["novx"][0] != 0.0)


# ---- 4: column independence, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_column_independence(hip, key):
    c = solved_case(key)
    dg, db, side, info = c["blk"]
    print(f"  {key}: panel {c['P']}, widths {sorted(c['sub'])}")
    for w, got in c["sub"].items():
        assert np.array_equal(got[0], dg[:, 1:1 + w]) and np.array_equal(got[1], db[:, 1:1 + w]), w
        assert np.array_equal(got[2], side) and np.array_equal(got[3], info)
    assert np.array_equal(c["permuted"][0], dg[:, c["perm"]]) and np.array_equal(c["permuted"][1], db[:, c["perm"]])
    assert np.all(dg[:, 2] == 0.0) and np.all(db[:, 2] == 0.0) and np.any(dg[:, 1] != 0.0) and np.any(dg[:, 0] != 0.0)
    assert same(c["again"], c["blk"])


# ---- 5: entries of vy outside W ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_entries_outside_the_working_set_are_dropped(hip, key):
    c = solved_case(key)
    nout = int(np.count_nonzero(c["blk"][2] == 0))
    a, h = same(c["nan"], c["blk"]), same(c["huge"], c["blk"])
    print(f"  {key}: {nout} rows outside W over the batch; NaN there: the same bits {a}; 1e300 there: the same bits {h}")
    assert nout > 0 and a and h


# ---- 6: the dual rows of the Jacobian ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_jacobian_duals(hip, key):
    c, refs = solved_case(key), reference_of(key)
    Jyg, Jyb, side, info = c["jd"]
    Jg, Jb = c["jac"][:2]
    cnt, m, n = Jyg.shape
    assert Jyb.shape == (cnt, m, m) and np.array_equal(side, c["blk"][2][:cnt]) and np.array_equal(info, c["blk"][3][:cnt])
    print(f"  {key}: {cnt} instances, kernel time {c['jd_ms']:.3f} ms")
    assert c["jd_ms"] > 0.0
    for b, r in enumerate(refs[:cnt]):
        W, Kinv = r["W"], r["Kinv"]
        bound = bound_1(c, r, b, 1.0)
        outside = np.ones(m, dtype=bool); outside[W] = False
        e_g = np.abs(Jyg[b][W] - Kinv[n:, :n]).max()
        e_b = np.abs(Jyb[b][np.ix_(W, W)] + Kinv[n:, n:]).max()
        e_x = np.abs(Jyg[b] - Jb[b].T).max()
        print(f"  {key} instance {b}: |W| = {len(W)}, err Jyg {e_g:.3g}, err Jyb {e_b:.3g}, |Jyg - Jb'| {e_x:.3g}, bound {bound:.3g}")
        assert e_g <= bound and e_b <= bound and e_x <= bound
        assert np.all(Jyg[b][outside] == 0.0) and np.all(Jyb[b][outside] == 0.0) and np.all(Jyb[b][:, outside] == 0.0)
        assert np.any(Jyg[b][W] != 0.0)
    if key == GRID:
        return
    B = len(refs)
    udg, udb = c["units"][:2]
    bits = np.array_equal(Jyg, udg) and np.array_equal(Jyb, udb)
    print(f"  {key}: the rows equal adjoint_blocked(None, unit VY) to the bit: {bits}")
    for b, r in enumerate(refs):
        bound = bound_1(c, r, b, 1.0)
        assert np.abs(Jyg[b] - udg[b]).max() <= bound and np.abs(Jyb[b] - udb[b]).max() <= bound
    if c["engine"]["fronts"] == 0 or key == FALLBACK:      # the band engines (and the vector kernel against itself)
        assert bits
    assert c["jd_nobounds"][1] is None and np.array_equal(c["jd_nobounds"][0], Jyg)
    k = min(2, B - 1)
    assert same(c["jd_range"], (Jyg[1:1 + k], Jyb[1:1 + k], side[1:1 + k], info[1:1 + k]))
    print(f"  {key}: {c['partial'][0]} work items; chunks of 1 and of at most {c['partial'][1]}")
    assert same(c["jd_one"], c["jd"]) and same(c["jd_partial"], c["jd"])


# ---- 7: central differences through warm re-solves -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", [(SMALL, 4), (MID, 2)])
def test_central_differences_through_warm_resolves(hip, shape, B):
    n, nC, nK = shape
    m = nC + 2 * nK
    opt = hip.default_options(**OPT)
    ds = instances(shape, B)
    sb = handle(hip, ds, opt)
    sb.run()
    assert all(s["returnValue"] == 0 for s in sb.solution()[2])
    rng = np.random.default_rng(6)
    VX, VY = rng.standard_normal((B, 1, n)), rng.standard_normal((B, 1, m))
    Z = rng.standard_normal((B, n)); ZB = rng.standard_normal((B, 2))
    side = sb.sensitivity(VX[:, 0])[2]
    VY[:, 0][side == 0] = 0.0
    dg, db, side, info = sb.adjoint_blocked(VX, VY)
    dg, db = dg[:, 0], db[:, 0]
    assert np.all(info == 0)
    bound = np.zeros(B)
    for b, d in enumerate(ds):
        W = np.flatnonzero(side[b])
        bound[b] = sum(fd_bounds(opt.stationarityTolerance, d["Q"].toarray(), d["E"].toarray()[W], VX[b, 0], VY[b, 0][W]))

    def resolved(ds2):
        update_all(sb, ds2)
        sb.resolve(warm=True)
        x, y, st = sb.solution()
        side2 = sb.sensitivity(VX[:, 0])[2]
        val = np.einsum("bi,bi->b", VX[:, 0], x) + np.einsum("bi,bi->b", VY[:, 0], y)
        return val, np.array([st[b]["returnValue"] == 0 and np.array_equal(side2[b], side[b]) for b in range(B)])

    def compare(name, plus, minus, predicted):
        vp, kp = resolved(plus); vm, km = resolved(minus)
        fd = (vp - vm) / (2 * H_FD)
        err = np.abs(fd - predicted)
        for b in range(B):
            print(f"  {shape} {name} instance {b}: fd {fd[b]:+.9e} predicted {predicted[b]:+.9e} err {err[b]:.3g} "
                  f"(rel {err[b] / max(abs(predicted[b]), 1e-300):.3g}) bound {bound[b]:.3g} W kept {bool(kp[b] and km[b])}")
        assert np.all(kp & km)                     # every instance keeps W at both offsets
        assert np.all(err <= bound) and np.any(predicted != 0.0)

    compare("g", [dict(d, g=d["g"] + H_FD * Z[b]) for b, d in enumerate(ds)], [dict(d, g=d["g"] - H_FD * Z[b]) for b, d in enumerate(ds)],
            np.einsum("bi,bi->b", dg, Z))
    rows = [np.flatnonzero(side[b, :nC])[:2] for b in range(B)]      # the bound two active rows of A sit on moves (an equality row: both bounds)
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


# ---- 8: no side effects ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "bordered circle"])
@pytest.mark.parametrize("warm", [True, False])
def test_the_calls_change_nothing(hip, case, warm):
    ds = instances_of(case)
    if case == "bordered circle":
        ds2 = [dict(d, g=d["g"] * (1.0 + 0.02 * np.random.default_rng(300 + b).standard_normal(d["nV"]))) for b, d in enumerate(ds)]
    else:
        ds2 = [moved(d, 300 + b) for b, d in enumerate(ds)]
    opt = hip.default_options(**OPT)
    rng = np.random.default_rng(1)
    B, n, m = len(ds), ds[0]["nV"], ds[0]["nC"] + 2 * ds[0]["nComp"]
    VX, VY = rng.standard_normal((B, 11, n)), rng.standard_normal((B, 11, m))
    out = []
    for with_calls in (True, False):
        with environment(VECTOR_CASES[case][1]):
            sb = handle(hip, ds, opt)
        sb.run()
        first = result(sb)
        if with_calls:
            counts = sb.launch_counts()
            before = sb.adjoint(VX[:, 0], VY[:, 0], matrices=())
            assert np.any(sb.jacobian_duals()[0] != 0.0)
            assert np.any(sb.adjoint_blocked(VX, VY)[0] != 0.0)
            after = sb.adjoint(VX[:, 0], VY[:, 0], matrices=())      # the pools the vector kernel borrows were not disturbed
            assert all(np.array_equal(before[k], after[k]) for k in before)
            assert sb.launch_counts() == counts
            assert_same_bits(first, result(sb))
        update_all(sb, ds2)
        sb.resolve(warm=warm)
        out.append(result(sb))
        assert sb.launch_counts() == (1, 2)
        sb.close()
    assert_same_bits(out[0], out[1])


# ---- 9: state errors and a failed instance ---------------------------------------------------------------------------------------------
def test_state_errors(hip):
    L = hip.lib()
    ds = instances(SMALL, 2)
    n, m = SMALL[0], SMALL[1] + 2 * SMALL[2]
    dp = ctypes.POINTER(ctypes.c_double)
    P = lambda a: a.ctypes.data_as(dp)
    vx, vy = np.ones((2, 1, n)), np.ones((2, 1, m))
    dg = np.full((2, 1, n), 7.0); Jyg = np.full((2, m, n), 7.0)
    d = ds[0]
    sb = hip.SparseBatchLCQP(2, d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(**OPT))
    blocked = lambda: L.lcqp_hip_sparse_adjoint_blocked(sb.h, 1, P(vx), P(vy), P(dg), None, None, None)
    duals = lambda: L.lcqp_hip_sparse_jacobian_duals(sb.h, 0, 2, P(Jyg), None, None, None)
    load = lambda: sb.load(0, 2, np.stack([q["Q"].data for q in ds]), np.stack([q["g"] for q in ds]), np.stack([q["E"].data for q in ds]),
                           lbA=np.stack([q["lbA"] for q in ds]), ubA=np.stack([q["ubA"] for q in ds]))
    assert blocked() == NOT_SETUP and duals() == NOT_SETUP      # before anything
    assert load() == 0
    assert blocked() == NOT_SETUP and duals() == NOT_SETUP and np.all(dg == 7.0) and np.all(Jyg == 7.0)
    sb.run()
    assert L.lcqp_hip_sparse_adjoint_blocked(sb.h, 1, None, None, P(dg), None, None, None) == INVALID_ARGUMENT
    assert L.lcqp_hip_sparse_jacobian_duals(sb.h, 1, 2, P(Jyg), None, None, None) == INVALID_ARGUMENT      # first + count > B
    assert np.all(dg == 7.0) and np.all(Jyg == 7.0)
    assert blocked() == 0 and duals() == 0 and not np.any(dg == 7.0) and not np.any(Jyg == 7.0)
    assert load() == 0                                        # a load since the last solve
    assert blocked() == NOT_SETUP and duals() == NOT_SETUP
    with pytest.raises(RuntimeError, match="300"):
        sb.jacobian_duals()
    sb.close()


def test_flag_of_a_failed_instance(hip):
    """Instance 4 gets a NaN in g: its run ends with 203 (tests/test_gpu_sparse_sensitivity.py).  info & 1 and zero outputs for it, the bits
    of the clean batch for its neighbours."""
    c = solved_case("small")
    ds = list(c["ds"])
    bad = 4
    g = ds[bad]["g"].copy(); g[0] = np.nan
    ds[bad] = dict(ds[bad], g=g)
    sb = handle(hip, ds, hip.default_options(**OPT))
    sb.run()
    st = sb.solution()[2]
    Jyg, Jyb, side, info = sb.jacobian_duals()
    dg, db, side2, info2 = sb.adjoint_blocked(c["VX"], c["VY"])
    sb.close()
    print("  return values", [s["returnValue"] for s in st], "info", info, info2)
    assert st[bad]["returnValue"] == 203 and (info[bad] & 1) and (info2[bad] & 1)
    assert np.all(Jyg[bad] == 0.0) and np.all(Jyb[bad] == 0.0) and np.all(side[bad] == 0) and np.all(dg[bad] == 0.0) and np.all(db[bad] == 0.0)
    for b in range(len(ds)):
        if b != bad:
            assert st[b]["returnValue"] == 0 and info[b] == c["jd"][3][b]
            assert np.array_equal(Jyg[b], c["jd"][0][b]) and np.array_equal(Jyb[b], c["jd"][1][b]) and np.array_equal(side[b], c["jd"][2][b])
            assert np.array_equal(dg[b], c["blk"][0][b]) and np.array_equal(db[b], c["blk"][1][b])


# ---- 10: torch -------------------------------------------------------------------------------------------------------------------------
def test_torch_layer_jacobian_full(hip):
    import torch
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 3
    n, m = shape[0], shape[1] + 2 * shape[2]
    ds = instances(shape, B)
    stack = lambda k: np.stack([d[k] for d in ds])
    sb = handle(hip, ds, hip.default_options(**OPT))
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack("lbA"), ubA=stack("ubA")))
    g = torch.tensor(stack("g"), dtype=torch.float64)
    layer(g)
    J = layer.jacobian_full(serial=layer.solves)
    xg, xb, side, info = sb.jacobian()
    yg, yb, _, _ = sb.jacobian_duals()
    assert sorted(J) == ["info", "side", "xb", "xg", "yb", "yg"] and layer.last_path == "host"
    for k, want, shp in (("xg", xg, (B, n, n)), ("xb", xb, (B, n, m)), ("yg", yg, (B, m, n)), ("yb", yb, (B, m, m))):
        assert tuple(J[k].shape) == shp and J[k].dtype == torch.float64 and np.array_equal(J[k].numpy(), want), k
    assert np.array_equal(J["side"].numpy(), side) and np.array_equal(J["info"].numpy(), info) and np.array_equal(layer.info, info)
    assert torch.any(J["yg"] != 0.0)
    with torch.no_grad():
        layer(g * 1.01)
    with pytest.raises(RuntimeError, match="not the layer's last one"):
        layer.jacobian_full(serial=1)
    sb.close()
