"""The constant matrices of the dense setup chain (k_prepare, k_build_C, k_compress_C, k_factor, k_trsm / k_trsm_streamed, k_build_M) and
the inverse factor Ti of the working-set matrix (ti_bulk, ti_append, ti_delete), read back from the device and held to plain numpy
references built from the problem data -- never to the oracle's factorisations, which restate the same algorithm.

References are np.longdouble (80-bit) up to np = 512 and float64 beyond (its own error on these products, ~1e-15, is four orders below the
tolerance).  tol = 1e-12 n is the building-block tolerance of DESIGN.md section 2, applied componentwise against the magnitudes of the summed
terms (Higham's gamma_{n+1} |L||L'| form, valid for any summation order).  Every assertion goes through _chk(), which prints the worst
ratio error / bound (`python -m pytest tests/test_gpu_setup.py -m gpu -s`).  A ratio above 1e-2 has to be explained before it is accepted;
the bounds themselves do not move.  Worst ratios over the whole file on an MI355X (28 s of wall time, most of it long-double products):

    L L' - (Q + spv I)              3.0e-4        Et L' - E                         2.0e-5
    D1_J L_JJ - I                   1.4e-6        Et - E chol(Q + spv I)^-T         1.0e-4
    M - Et Et'                      4.1e-5        M - E (Q + spv I)^-1 E'           1.1e-4
    C - (L'R + R'L)                 5.3e-5        F1 padding diagonal               0 (exact)
    Ti'Ti S_W - I                   6.6e-5        (cond_2(S_W) <= 109 in every state checked)
    y_W - least-squares multipliers 5.1e-5        Qx + g - A_W'y_W                  4.4e-5   (both of Y_TOL = 1e-7)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
Y_TOL = 1e-7                # tests/test_gpu_parity.py


def _cond(Q):
    ev = np.linalg.eigvalsh(Q)
    return ev[-1] / ev[0]


def _chk(name, err, bound):
    """every entry of err within bound; the worst ratio is printed"""
    err = np.asarray(err, dtype=np.float64); bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    if err.size == 0:
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    worst = float(ratio.max())
    print(f"    {name}: worst error / bound = {worst:.3e}")
    assert (err <= bound).all(), f"{name}: worst error / bound = {worst:.3e}"


# ---- plain references ---------------------------------------------------------------------------------------------------------------
def tri_inv(D, dt):
    """inverse of a lower-triangular matrix by forward substitution, row by row, in dtype dt"""
    D = D.astype(dt); k = D.shape[0]
    X = np.zeros((k, k), dtype=dt)
    for i in range(k):
        row = -(D[i, :i] @ X[:i])
        row[i] = 1
        X[i] = row / D[i, i]
    return X


def chol_ref(A, dt):
    """lower Cholesky factor in dtype dt (right-looking, no pivoting); float64 goes to LAPACK"""
    if dt is np.float64:
        return np.linalg.cholesky(A)
    A = A.astype(dt).copy(); n = A.shape[0]
    for j in range(n):
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A)


def solve_lt_right(E, L, dt):
    """X with X L' = E for lower-triangular L, column by column, in dtype dt"""
    if dt is np.float64:
        import scipy.linalg
        return scipy.linalg.solve_triangular(L, E.T, lower=True).T
    E = E.astype(dt); n = L.shape[0]
    X = np.zeros(E.shape, dtype=dt)
    for j in range(n):
        X[:, j] = (E[:, j] - X[:, :j] @ L[j, :j]) / L[j, j]
    return X


def unpack_L(rs, dt):
    """L1 [np][np] from the read-back: the strict lower blocks from F1, the diagonal blocks by inverting D1 in long double"""
    npad, nblk = rs["np"], rs["nblk"]
    L = np.tril(rs["F1"]).astype(dt)
    for J in range(nblk):
        s = slice(64 * J, 64 * J + 64)
        L[s, s] = tri_inv(rs["D1"][J], LD).astype(dt)
    return L


def stacked_rows(d, lb=None, ub=None):
    """E = [A; L; R; box rows]: the box rows are rows of I for the variables with a finite bound, ascending (k_prepare)"""
    n = d["Q"].shape[0]
    rows = [d["A"].reshape(-1, n), d["L"].reshape(-1, n), d["R"].reshape(-1, n)]
    if lb is not None or ub is not None:
        lo = np.full(n, -np.inf) if lb is None else lb
        hi = np.full(n, np.inf) if ub is None else ub
        fin = np.flatnonzero(np.isfinite(lo) | np.isfinite(hi))
        rows.append(np.eye(n)[fin])
    return np.vstack(rows)


# ---- the setup chain of one instance ------------------------------------------------------------------------------------------------
def check_setup(rs, d, E, opt, direct=True, psd=False):
    """Everything the issue lists for one instance: rs = read_setup(b), d = the problem data, E = the stacked rows the device holds.

    Layout.  F1 is symmetric entry by entry (L1 below / L1' above outside the diagonal blocks, inv(L1_JJ) symmetric-filled inside: what
    wg_trsv streams in both directions); the lower triangle of a diagonal block of F1 is D1_J bit for bit and D1_J is zero above its
    diagonal (k_trsm and ti_bulk multiply by the whole 64 x 64 block).  Beyond n: rows and columns of C, Et and F1 are exact zeros, the
    padding diagonal of F1 holds inv(sqrt(1 + spv)) -- the factor of the unit diagonal k_prepare puts into Q, shifted like the rest; it is
    1 - spv / 2 and not 1.0, and padded variables stay 0 because their right-hand sides are 0 and the off-diagonal padding is 0.
    Beyond mE: rows of Et and the rows of the lower triangle of MM are exact zeros in a batch object that has been set up once (the row
    blocks k_trsm runs are products with zero rows of E, the others keep the zero fill of the allocation; k_build_M substitutes zeros for
    rows >= mE).  NO reader relies on it: k_build_M guards its loads by mE, ti_bulk and ti_append index M by rows of the working set, the
    sweeps over Et go through row lists -- so the assertion pins the state, not a contract another kernel needs.
    MM is read as M[max][min]: only the lower triangle is asserted.
    """
    n = d["Q"].shape[0]; npad, nblk, mE = rs["np"], rs["nblk"], rs["mE"]
    assert E.shape == (mE, n) and mE <= rs["mEcap"] <= rs["mMld"] and rs["setupFail"] == 0
    dt = LD if npad <= 512 else np.float64
    tol = 1e-12 * n
    F1, D1, Et, MM, C = rs["F1"], rs["D1"], rs["Et"], rs["MM"], rs["C"]
    spv, scale = rs["spv"], rs["scale"]
    # ---- layout invariants (exact)
    assert np.array_equal(F1, F1.T)
    for J in range(nblk):
        s = slice(64 * J, 64 * J + 64)
        assert np.array_equal(np.tril(F1[s, s]), D1[J]) and not np.triu(D1[J], 1).any()
    off = F1 - np.diag(np.diag(F1))
    assert not off[n:, :].any() and not off[:, n:].any()
    assert not C[n:, :].any() and not C[:, n:].any() and not Et[:, n:].any()
    assert not Et[mE:].any() and not np.tril(MM)[mE:].any()
    if npad > n:
        _chk("F1 padding diagonal = 1/sqrt(1+spv)", np.abs(np.diag(F1)[n:] * np.sqrt(1.0 + spv) - 1.0), 4 * np.finfo(float).eps)
    # ---- the shift
    assert scale == np.abs(np.diag(d["Q"])).max()
    assert spv == (opt.proxBig if psd else opt.proxSmall) * scale
    # ---- L1
    Lp = unpack_L(rs, dt)
    L = Lp[:n, :n]
    Qs = d["Q"].astype(dt) + dt(spv) * np.eye(n, dtype=dt)
    aL = np.abs(L)
    _chk("L L' - (Q + spv I)", np.abs(L @ L.T - Qs), tol * (aL @ aL.T))
    DL = [(D1[J].astype(LD), Lp[64 * J:64 * J + 64, 64 * J:64 * J + 64].astype(LD)) for J in range(nblk)]
    _chk("D1_J L_JJ - I", np.array([np.abs(DJ @ LJ - np.eye(64, dtype=LD)) for DJ, LJ in DL]),
         np.array([1e-12 * 64 * (np.abs(DJ) @ np.abs(LJ)) for DJ, LJ in DL]))
    # ---- Et
    Ett = Et[:mE, :n].astype(dt)
    _chk("Et L' - E", np.abs(Ett @ L.T - E.astype(dt)), tol * (np.abs(Ett) @ aL.T))
    Mdev = np.tril(MM[:mE, :mE])
    mmax = np.abs(Mdev).max()
    _chk("M - Et Et'", np.abs(np.tril(Ett @ Ett.T) - Mdev), tol * mmax)
    if direct:
        Lref = chol_ref(Qs, dt)
        X = solve_lt_right(E, Lref, dt)
        _chk("Et - E chol(Q + spv I)^-T", np.abs(Ett - X), tol)
        _chk("M - E (Q + spv I)^-1 E'", np.abs(np.tril(X @ X.T) - Mdev), tol * mmax)
    # ---- C and its compressed rows
    Lm, Rm = d["L"].astype(dt), d["R"].astype(dt)
    _chk("C - (L'R + R'L)", np.abs(C[:n, :n] - (Lm.T @ Rm + Rm.T @ Lm)), tol * (np.abs(Lm).T @ np.abs(Rm) + np.abs(Rm).T @ np.abs(Lm)) + 1e-300)
    nnz = int(np.count_nonzero(C))
    if d["L"].shape[0] == 0:
        assert rs["cNnz"] == -1 and nnz == 0       # no complementarity rows: the C branch of the setup does not run
    elif nnz > rs["capC"]:
        assert rs["cNnz"] == -1
    else:
        Cp, Ci, Cv = rs["Cp"], rs["Ci"], rs["Cv"]
        assert rs["cNnz"] == nnz == Cp[npad] and Cp[0] == 0 and (np.diff(Cp) >= 0).all()
        dense = np.zeros((npad, npad))
        for r in range(npad):
            cols = Ci[Cp[r]:Cp[r + 1]]
            assert (np.diff(cols) > 0).all() and (cols >= 0).all() and (cols < n).all()
            dense[r, cols] = Cv[Cp[r]:Cp[r + 1]]
        assert np.array_equal(dense, C)
    return nnz


def family(rng, n, nC, nComp, dense_LR=False):
    """Q = M'M / n + I (cond about 5), E Gaussian / sqrt(n); L, R rows of the identity (C has 2 nComp non-zeros) unless dense_LR"""
    M = rng.standard_normal((n, n))
    d = dict(Q=M.T @ M / n + np.eye(n), g=rng.standard_normal(n), A=rng.standard_normal((nC, n)) / np.sqrt(n))
    if dense_LR:
        d["L"] = rng.standard_normal((nComp, n)) / np.sqrt(n); d["R"] = rng.standard_normal((nComp, n)) / np.sqrt(n)
    else:
        p = rng.permutation(n)
        d["L"] = np.zeros((nComp, n)); d["R"] = np.zeros((nComp, n))
        for i in range(nComp):
            d["L"][i, p[(2 * i) % n]] = rng.uniform(0.5, 2.0); d["R"][i, p[(2 * i + 1) % n]] = rng.uniform(0.5, 2.0)
    return d


def run_setup_case(hip, n, nC, nComp, B=1, seed=0, overlapped=False, box=False, dense_LR=False, mutate=None, direct=True, psd=False):
    rng = np.random.default_rng(1000 + seed)
    opt = hip.default_options()
    bt = hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=opt)
    bt.set_overlapped(overlapped)
    data = []
    for b in range(B):
        d = family(rng, n, nC, nComp, dense_LR)
        lb = ub = None
        if box:      # partly infinite bounds: fewer box rows than the batch has room for (mE < mEcap)
            lb = np.where(rng.random(n) < 0.4, -1.0 - rng.random(n), -np.inf); ub = np.where(rng.random(n) < 0.3, 1.0 + rng.random(n), np.inf)
        if mutate:
            mutate(d, rng)
        assert bt.load(b, 1, d["Q"], d["g"], d["L"], d["R"], A=d["A"] if nC else None, lb=lb, ub=ub) == 0
        data.append((d, lb, ub))
    bt.setup()
    out = []
    for b, (d, lb, ub) in enumerate(data):
        back = bt.read_problem(b)
        for k in ("Q", "A", "L", "R"):
            assert np.array_equal(back[k], d[k])
        rs = bt.read_setup(b)
        E = stacked_rows(d, lb, ub)
        if direct and not psd:
            assert _cond(d["Q"]) < 1e2      # the direct comparisons are stated for the well-conditioned family
        if box:
            assert rs["mE"] < rs["mEcap"]
        out.append((rs, check_setup(rs, d, E, opt, direct=direct, psd=psd)))
    bt.close()
    return out


SIZES = [(2, 128), (33, 128), (64, 128), (65, 128), (127, 128), (128, 128), (129, 256), (200, 256), (256, 256), (300, 384), (512, 512),
         (513, 1024), (700, 1024), (1024, 1024), (1500, 2048), (3000, 4096)]


@pytest.mark.parametrize("n,npad", SIZES)
def test_setup_padded_sizes(hip, n, npad):
    """n off and on the block edges of every padded size (np >= 384 always runs the streamed k_trsm; n = 3000: float64 reference).
    Worst error / bound on an MI355X: see test_setup_ratios_are_small."""
    nComp = min(3, n // 2); nC = min(70, max(1, n // 2))
    (rs, _), = run_setup_case(hip, n, nC, nComp, seed=n)
    assert rs["np"] == npad and rs["cNnz"] == 2 * nComp


@pytest.mark.parametrize("mE", [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 640, 641, 897])
@pytest.mark.parametrize("overlapped", [False, True])
def test_setup_row_counts_at_tile_edges(hip, mE, overlapped):
    """n = 256, row counts at the edges of k_trsm's 64-row blocks and k_build_M's 128 x 64 tiles, in the resident and in the streamed
    form of k_trsm; mE = 64 and 640 have nC = 0 (rows of L and R only), mE = 1 has no complementarity row"""
    if mE in (64, 640):
        nC, nComp = 0, mE // 2
    else:
        nComp = min(8, mE // 2); nC = mE - 2 * nComp
    (rs, _), = run_setup_case(hip, 256, nC, nComp, seed=mE, overlapped=overlapped, dense_LR=(mE == 640))
    assert rs["mE"] == mE


@pytest.mark.parametrize("overlapped", [False, True])
def test_setup_box_rows(hip, overlapped):
    """a box-bounded batch: rows of I inside E, partly infinite bounds (mE < mEcap), different data per instance"""
    run_setup_case(hip, 200, 70, 5, B=2, seed=77, overlapped=overlapped, box=True)


@pytest.mark.parametrize("n", [128, 300])
def test_setup_three_different_neighbours(hip, n):
    """B = 3 with different data per instance: every instance's blocks are held to its own reference, nothing leaks between neighbours"""
    out = run_setup_case(hip, n, 90, 6, B=3, seed=3 + n)
    assert not np.array_equal(out[0][0]["F1"], out[1][0]["F1"]) and not np.array_equal(out[1][0]["Et"], out[2][0]["Et"])


def test_setup_large_batch_uses_the_four_per_cu_factor(hip):
    """B = 1040 > 3 x CU count at n = 128: the k_factor instantiation held to 128 registers (the other cases run the plain one).  Synthetic
    data generated on the device; a sample of instances -- the first, the last, one in each eighth of the batch (the ranges xcd_contiguous
    hands to the XCDs)"""
    B, n, nC, nComp = 1040, 128, 96, 32
    opt = hip.default_options()
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    bt.generate_synthetic(0)
    bt.setup()
    for b in sorted({0, B - 1} | {(k * B) // 8 + 5 for k in range(8)}):
        d = bt.read_problem(b)
        direct = _cond(d["Q"]) < 1e2
        print(f"  instance {b}: cond(Q) = {_cond(d['Q']):.3g}")
        check_setup(bt.read_setup(b), d, stacked_rows(d), opt, direct=direct)
    bt.close()


def test_setup_dense_C_and_degenerate_rows(hip):
    """non-synthetic structure: dense random L and R (C dense, not compressed), duplicated and zero rows in E"""
    def mutate(d, rng):
        d["A"][5] = d["A"][2]; d["A"][17] = d["A"][2]; d["A"][9] = 0.0; d["A"][-1] = 0.0
    (rs, nnz), = run_setup_case(hip, 200, 130, 40, seed=5, dense_LR=True, mutate=mutate)
    assert rs["cNnz"] == -1 and nnz > rs["capC"]


@pytest.mark.parametrize("extra", [0, 1])
def test_setup_compressed_C_at_its_capacity(hip, extra):
    """the number of non-zeros of C exactly at capC (compressed) and one pair above it (cNnz = -1); capC comes from the reader.
    L_r = e_r, R_r non-zero in columns beyond r: C holds every R value twice, at positions no other row touches."""
    n, nComp = 128, 16
    probe = hip.BatchLCQP(1, n, 1, nComp)
    probe.load(0, 1, np.eye(n), np.zeros(n), np.zeros((nComp, n)), np.zeros((nComp, n)), A=np.zeros((1, n)))
    probe.setup()
    capC = probe.read_setup(0)["capC"]
    probe.close()
    assert capC % (2 * nComp) == 0 and capC // (2 * nComp) + 1 + nComp <= n
    per = capC // (2 * nComp)

    def mutate(d, rng):
        d["L"][:] = 0.0; d["R"][:] = 0.0
        for r in range(nComp):
            k = per + (extra if r == 0 else 0)
            d["L"][r, r] = 1.0; d["R"][r, r + 1:r + 1 + k] = rng.uniform(0.5, 2.0, k)
    (rs, nnz), = run_setup_case(hip, n, 1, nComp, seed=8, mutate=mutate)
    assert rs["capC"] == capC and nnz == capC + 2 * extra
    assert rs["cNnz"] == (capC if extra == 0 else -1)


def test_setup_semidefinite_Q_takes_the_second_pass(hip):
    """Q of rank n / 2 (as in examples/OptimizeOnCircle.cpp): pass 1 of k_factor (shift proxSmall) meets a pivot below the threshold, pass 2
    factors Q + proxBig scale I.  The residual identities hold; the direct comparisons are left out (Et is about 1e4 in size)."""
    def mutate(d, rng):
        n = d["Q"].shape[0]
        V = rng.standard_normal((n // 2, n))
        d["Q"] = V.T @ V / n
    for n in (128, 200):
        run_setup_case(hip, n, 60, 4, seed=n, mutate=mutate, direct=False, psd=True)


def test_setup_indefinite_Q_is_reported(hip, oracle):
    """an indefinite Q: both passes of k_factor fail, setupFail = 3, and the run ends as the oracle's does"""
    import problems as P
    n, nC, nComp = 100, 20, 3
    rng = np.random.default_rng(4)
    d = family(rng, n, nC, nComp)
    d["Q"] = d["Q"] - 3.0 * np.eye(n)
    d.update(nV=n, nC=nC, nComp=nComp)
    opt = hip.default_options(perturbStep=0)
    bt = hip.BatchLCQP(1, n, nC, nComp, opt=opt)
    assert bt.load(0, 1, d["Q"], d["g"], d["L"], d["R"], A=d["A"]) == 0
    bt.setup()
    assert bt.read_setup(0)["setupFail"] == 3
    bt.run()
    _, _, st = bt.solution()
    assert bt.read_setup(0)["setupFail"] == 3
    bt.close()
    ro = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0))
    assert st[0]["returnValue"] == ro["ret"] != 0


# ---- the inverse factor -------------------------------------------------------------------------------------------------------------
def check_working_set(ws, rs, Q, E, dependent=False):
    """Structure of the inverse factor and the identity Ti'Ti S_W = I.  Returns the rows in slot order.

    Structure (lcqp_dev.hpp, "Inverse factor Ti"): slot_row and row_slot are inverse maps, no row twice, nT = occupied slots <= ns, crow
    on the occupied slots is a permutation of 0 .. nT-1, and column s of Ti is an exact zero in the rows above crow[s] -- in every row
    below nT for a free slot s < ns: ti_apply_fast and ti_delete do not load those entries, so a non-zero there is a wrong answer.
    dependent (the working set holds linearly dependent rows): a one-piece rebuild that flags k rows frees their slots but keeps their
    rows of Ti, cleared (ti_bulk: nT = na).  Then nT - k slots are occupied, crow maps them one-to-one into 0 .. nT-1 and every row of Ti
    no slot owns is an exact zero: such rows add nothing to Ti'Ti, and the identity below holds with them in place.
    Identity: S_W = E_W (Q + spv I)^-1 E_W' in long double from Q, E and the reported spv (not from the device's M);
    |Ti'Ti S_W - I|_max <= 1e-12 nT cond_2(S_W), and cond_2(S_W) <= 1e4 is asserted so that the bound means something.
    """
    capS, mE = rs["capS"], rs["mE"]
    nT, ns = ws["nT"], ws["ns"]
    slot_row, crow, row_slot, Ti = ws["slot_row"], ws["crow"], ws["row_slot"], ws["Ti"]
    assert 0 <= nT <= ns <= capS
    occ = np.flatnonzero(slot_row >= 0)
    assert (occ < ns).all() and (len(occ) <= nT if dependent else len(occ) == nT)
    W = slot_row[occ]
    assert (W < mE).all() and len(set(W.tolist())) == len(occ)
    assert np.array_equal(row_slot[W], occ) and np.count_nonzero(row_slot >= 0) == len(occ)
    owned = np.sort(crow[occ])
    assert (np.diff(owned) > 0).all() and (len(occ) == 0 or (owned[0] >= 0 and owned[-1] < nT))
    assert not np.delete(Ti[:nT, :ns], owned, axis=0).any()
    first = np.full(ns, nT)                      # free slots: zero in every row of the factor
    first[occ] = crow[occ]
    assert not (Ti[:nT, :ns] * (np.arange(nT)[:, None] < first[None, :])).any()
    if nT == 0:
        return W
    n = Q.shape[0]
    Lref = chol_ref(Q.astype(LD) + LD(rs["spv"]) * np.eye(n, dtype=LD), LD)
    X = solve_lt_right(E[W], Lref, LD)
    S = X @ X.T
    cond = np.linalg.cond(S.astype(np.float64))
    print(f"    nT = {nT}, occupied = {len(occ)}, ns = {ns}, cond(S_W) = {cond:.3g}")
    assert cond <= 1e4
    T = Ti[:nT][:, occ].astype(LD)
    _chk("Ti'Ti S_W - I", np.abs(T.T @ T @ S - np.eye(len(occ), dtype=LD)), 1e-12 * nT * cond)
    return W


def check_answer(W, Q, g, A, x, y, dup_ok=False):
    """the returned multipliers live on rows of the factor (or on exact copies of such rows when dup_ok), and y_W solves the
    working-set KKT system Q x + g = A_W' y_W of the returned x"""
    n = Q.shape[0]
    yA = y[n:]
    inW = np.zeros(len(yA), dtype=bool); inW[W] = True
    for r in np.flatnonzero((yA != 0) & ~inW):
        assert dup_ok and any(np.array_equal(A[r], A[w]) for w in W), f"row {r} carries a multiplier but is not in the factor"
    rhs = Q @ x + g
    if dup_ok:       # multipliers of a group of equal rows act through their sum
        yW = np.array([yA[[r for r in range(len(yA)) if np.array_equal(A[r], A[w])]].sum() for w in W])
    else:
        yW = yA[W]
    ystar = np.linalg.lstsq(A[W].T, rhs, rcond=None)[0] if len(W) else np.zeros(0)
    _chk("y_W - argmin |A_W'y - (Qx + g)|", np.abs(yW - ystar), Y_TOL)
    _chk("Qx + g - A_W'y_W", np.abs(rhs - A[W].T @ yW), Y_TOL)


def _qp_family(rng, n, m):
    M = rng.standard_normal((n, n)); Q = M.T @ M / n + np.eye(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n)
    return Q, A, rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("n,m,seed", [(96, 160, 11), (256, 640, 12)])
def test_inverse_factor_follows_every_kind_of_update(hip, n, m, seed):
    """Hot starts with changed bound values (inputs as in test_subsolver_hot_start_with_new_bound_values) drive the three update paths of
    qp_polish (lcqp_dev.hpp, `const bool bulk = ...`): a few rows enter (ti_append), a few rows leave (ti_delete), many rows enter
    (ti_bulk).  After every solve the factor is read back and held to check_working_set / check_answer, and the structure tells the paths
    apart:
      rebuild: ns == nT, crow[a] == a, slot_row ascending (ti_bulk numbers slots in ascending row order), after >= 16 rows entered;
      append : every row that stayed keeps its slot and its crow, the new rows own the crow values from the old nT upwards;
      delete : every row that stayed keeps its slot, crow closes up (values above the deleted one drop by one).
    Each kind, and a deletion from a slot that is not the last one, must be seen at least once: a seed that stops exercising a path
    fails here."""
    rng = np.random.default_rng(seed)
    Q, A, g, xs = _qp_family(rng, n, m)
    lbA = A @ xs - rng.uniform(2.0, 4.0, m); ubA = A @ xs + rng.uniform(2.0, 4.0, m)
    qh = hip.SubsolverHIP(n, m, Q, A)
    seen = dict(rebuild=0, append=0, delete=0, inner_delete=0)

    def solve(initial, lo, hi):
        rh = qh.solve(initial, g, lo, hi, np.zeros(n) if initial else None, None)
        assert (rh[0], rh[2]) == (0, 0), rh
        rs = qh.read_setup() if initial else solve.rs
        solve.rs = rs
        ws = qh.read_working_set()
        W = check_working_set(ws, rs, Q, A)
        x, y = qh.getSolution()
        check_answer(W, Q, g, A, x, y)
        assert (A @ x <= hi + 1e-8).all() and (A @ x >= lo - 1e-8).all()
        return ws, x

    def classify(old, new):
        so, sn = old["slot_row"], new["slot_row"]
        Wo = set(so[so >= 0].tolist()); Wn = set(sn[sn >= 0].tolist())
        ent, left, stay = Wn - Wo, Wo - Wn, sorted(Wo & Wn)
        stay = np.array(stay, dtype=int)
        keep = np.array_equal(old["row_slot"][stay], new["row_slot"][stay])
        occ = np.flatnonzero(sn >= 0)
        bulk_form = new["ns"] == new["nT"] and np.array_equal(new["crow"][:new["nT"]], np.arange(new["nT"])) and (np.diff(sn[occ]) > 0).all()
        print(f"    entered {len(ent)}, left {len(left)}, slots kept {keep}, rebuild form {bulk_form}, nT {old['nT']} -> {new['nT']}, ns {new['ns']}")
        if len(ent) >= 16 and not left and bulk_form:
            seen["rebuild"] += 1
        if 1 <= len(ent) <= 3 and not left and keep:
            ce = sorted(new["crow"][new["row_slot"][sorted(ent)]].tolist())
            if ce == list(range(old["nT"], new["nT"])) and np.array_equal(old["crow"][old["row_slot"][stay]], new["crow"][new["row_slot"][stay]]):
                seen["append"] += 1
        if 1 <= len(left) <= 3 and not ent and keep and len(left) < max(old["nT"] // 2, 8):
            gone = np.sort(old["crow"][old["row_slot"][sorted(left)]])
            co = old["crow"][old["row_slot"][stay]]
            if np.array_equal(co - np.searchsorted(gone, co), new["crow"][new["row_slot"][stay]]):
                seen["delete"] += 1
                if min(old["row_slot"][sorted(left)]) < old["ns"] - len(left):
                    seen["inner_delete"] += 1

    ws, x = solve(True, lbA, ubA)
    lo, hi = lbA.copy(), ubA.copy()

    def step(enter=(), release=()):
        """rows `enter` move 1e-3 past the current solution (they come in with small multipliers and little else moves); the bounds of
        rows `release` move 2e-3 to the other side of it, beyond the point the row came in from (back to the wide bounds the first
        correction would be a long step through many rows)"""
        nonlocal ws, x
        ax = A @ x
        for r in enter:
            hi[r] = ax[r] - 1e-3; lo[r] = min(lo[r], hi[r] - 1.0)
        for r in release:
            hi[r] = ax[r] + 2e-3
        old = ws
        ws, x = solve(False, lo, hi)
        classify(old, ws)

    def inactive(k):
        return [int(r) for r in rng.choice(np.setdiff1d(np.arange(m), ws["slot_row"][ws["slot_row"] >= 0]), k, replace=False)]

    for rnd in range(2):
        # a third of the rows cut the solution off by a wide margin: whatever path the trials take, the factor must come out right
        ax = A @ x
        sel = np.arange(rnd, m, 3)
        lo, hi = lbA.copy(), ubA.copy()
        hi[sel] = ax[sel] - 0.05 * (1 + rnd); lo[sel] = np.minimum(lo[sel], hi[sel] - 1.0)
        old = ws
        ws, x = solve(False, lo, hi)
        classify(old, ws)
        a, b, c = inactive(1), inactive(2), inactive(3)
        step(enter=a)                   # append
        step(enter=b)                   # append behind it
        step(release=a)                 # delete from a slot with two slots behind it
        step(enter=c)
        step(release=b)                 # delete
        step(release=c)
        for k in (16, 18, 20):
            many = inactive(k)
            step(enter=many)            # >= 16 rows enter: the rebuild
            step(release=many[:3])
            step(release=many[3:])
    qh.close()
    print("    seen:", seen)
    assert all(v >= 1 for v in seen.values()), seen


def test_inverse_factor_with_duplicated_rows(hip):
    """k exact copies of active rows: the factor holds one row of every group of equal rows, the identity holds on the rows it holds,
    the solve returns 0 and the multipliers of a group act through their sum"""
    n, m, k = 96, 160, 6
    rng = np.random.default_rng(21)
    Q, A, g, xs = _qp_family(rng, n, m)
    lbA = A @ xs - rng.uniform(0.1, 1.0, m); ubA = A @ xs + rng.uniform(0.1, 1.0, m)
    q0 = hip.SubsolverHIP(n, m, Q, A)
    assert q0.solve(True, g, lbA, ubA, np.zeros(n), None)[0] == 0
    act = q0.read_working_set()["slot_row"]; act = act[act >= 0]
    q0.close()
    assert len(act) >= k
    src = act[:k]
    A2 = np.vstack([A, A[src]]); lb2 = np.concatenate([lbA, lbA[src]]); ub2 = np.concatenate([ubA, ubA[src]])
    qh = hip.SubsolverHIP(n, m + k, Q, A2)
    rh = qh.solve(True, g, lb2, ub2, np.zeros(n), None)
    assert (rh[0], rh[2]) == (0, 0), rh
    ws = qh.read_working_set()
    W = check_working_set(ws, qh.read_setup(), Q, A2, dependent=True)
    x, y = qh.getSolution()
    check_answer(W, Q, g, A2, x, y, dup_ok=True)
    for j, r in enumerate(src):
        assert (r in W) + ((m + j) in W) == 1, (r, m + j)
    qh.close()


@pytest.mark.parametrize("n,m,neq", [(512, 600, 300), (96, 64, 64)])
def test_inverse_factor_at_the_capacity_edges(hip, n, m, neq):
    """more than 256 slots (the full-row path of ti_apply beyond TI_FAST_CHUNKS), and a factor that fills capS to the last row
    (64 equality rows in a batch whose capS is 64)"""
    rng = np.random.default_rng(31 + n)
    Q, A, g, xs = _qp_family(rng, n, m)
    lbA = A @ xs - rng.uniform(2.0, 4.0, m); ubA = A @ xs + rng.uniform(2.0, 4.0, m)
    lbA[:neq] = ubA[:neq] = (A @ xs)[:neq]
    qh = hip.SubsolverHIP(n, m, Q, A)
    rh = qh.solve(True, g, lbA, ubA, np.zeros(n), None)
    assert (rh[0], rh[2]) == (0, 0), rh
    rs = qh.read_setup(); ws = qh.read_working_set()
    W = check_working_set(ws, rs, Q, A)
    x, y = qh.getSolution()
    check_answer(W, Q, g, A, x, y)
    assert ws["nT"] >= neq and (ws["nT"] > 256 if neq > 256 else ws["nT"] >= rs["capS"] - 1)
    if ws["nT"] == neq:      # only the equality rows are active: one rebuild from the empty factor, slots in ascending row order
        assert ws["ns"] == neq and np.array_equal(ws["crow"][:neq], np.arange(neq)) and np.array_equal(ws["slot_row"][:neq], np.arange(neq))
    # one hot start on top: the factor is applied, not only built
    g2 = g + 0.1 * rng.standard_normal(n)
    rh = qh.solve(False, g2, lbA, ubA, None, None)
    assert (rh[0], rh[2]) == (0, 0), rh
    W = check_working_set(qh.read_working_set(), rs, Q, A)
    x, y = qh.getSolution()
    check_answer(W, Q, g2, A, x, y)
    qh.close()


@pytest.mark.parametrize("B,n,nC,nComp", [(5, 256, 512, 64), (3, 200, 330, 37)])
def test_inverse_factor_after_a_batched_run(hip, B, n, nC, nComp):
    """through BatchLCQP on the synthetic shapes: the factor every instance's last QP left.  (The returned y are the duals of the LCQP,
    src/LCQProblem.cpp:1485-1504, not the multipliers of that QP: the consistency check of the answer is the QP object's, above.)
    The setup matrices are checked after the run as well: the homotopy kernel must leave them as the setup wrote them."""
    opt = hip.default_options(perturbStep=0)
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=opt)
    bt.generate_synthetic(0)
    bt.run()
    _, _, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    for b in range(B):
        d = bt.read_problem(b)
        rs = bt.read_setup(b)
        E = stacked_rows(d)
        ws = bt.read_working_set(b)
        check_working_set(ws, rs, d["Q"], E)
        if b == 0:
            check_setup(rs, d, E, opt, direct=_cond(d["Q"]) < 1e2)
    bt.close()
