"""Parity tests proper: the HIP path (through the C ABI of include/lcqp_hip.h) against the CPU oracle on
identical inputs.  Tolerances: fp64 -- building blocks 1e-12 relative, QP/LCQP primal iterates 1e-9
absolute, duals 1e-7 absolute (north_star: "within a stated fp64 tolerance")."""
import os

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(P.GOLDEN, "oracle_golden.npz"))
X_TOL, Y_TOL = 1e-9, 1e-7


# ---- Utilities: the reference's known answers (test/RunUnitTests.cpp:33-246) through the HIP kernels ----
def test_kat_transposed_multiplication(hip):      # :60-78
    c = hip.util_gemv_t(np.array([[[1., 0, 2], [3, 1, 1]]]), np.array([[98., -10]]))
    assert list(c[0]) == [68, -10, 186]


def test_kat_matrix_multiplication(hip):          # :33-57, column by column (p = 1 kernels)
    A = np.array([[[1., 0, 2], [3, 1, 1]]]); B = np.array([[2., 0, 0, 2], [1, 0, 0, 1], [0, -1, -1, 0]])
    C = np.stack([hip.util_gemv(A, B[None, :, j])[0] for j in range(4)], axis=1)
    assert C.tolist() == [[2, -2, -2, 2], [7, -1, -1, 7]]


def test_kat_symmetrization(hip):                 # :81-104
    C = hip.util_symm_product(np.array([[[1., 0, 2], [3, 1, 1]]]), np.array([[[2., 0, 1], [0, 0, -1]]]))
    assert C[0].tolist() == [[4, 0, 2], [0, 0, -1], [2, -1, 2]]


def test_kat_affine_symmetric(hip):               # AffineLinearTransformation :107-129 restricted to symmetric A
    A = np.array([[[0., 1, 0], [1, 2, 1], [0, 1, 0]]]); b = np.array([[1., 2, 3]]); c = np.array([[-3., -3, -3]])
    d = hip.util_symv(2.0, A, b, c)
    assert list(d[0]) == [1, 13, 1]
    # QuadraticFormProduct KAT (:190-204): p'Qp = 24
    assert float(b[0] @ hip.util_symv(1.0, A, b, np.zeros((1, 3)))[0]) == 24


@pytest.mark.parametrize("n,m", [(3, 2), (100, 37), (256, 640), (300, 50), (512, 70), (700, 40), (1024, 130)])
def test_utilities_random(hip, oracle, n, m):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((2, n, n)); A = A + A.transpose(0, 2, 1)
    b = rng.standard_normal((2, n)); c = rng.standard_normal((2, n))
    d = hip.util_symv(2.0, A, b, c)
    E = rng.standard_normal((2, m, n)); x = rng.standard_normal((2, n)); y = rng.standard_normal((2, m))
    L = rng.standard_normal((2, m, n)); R = rng.standard_normal((2, m, n))
    ex = hip.util_gemv(E, x); ety = hip.util_gemv_t(E, y); Cm = hip.util_symm_product(L, R)
    for k in range(2):
        assert np.abs(d[k] - oracle.util_affine(2.0, A[k], b[k], c[k], n, n)).max() < 1e-12 * n
        assert np.abs(ex[k] - oracle.util_matmul(E[k], x[k], m, n, 1)).max() < 1e-12 * n
        assert np.abs(ety[k] - oracle.util_matmul_t(E[k], y[k], m, n, 1)).max() < 1e-12 * m
        assert np.abs(Cm[k] - oracle.util_symm_product(L[k], R[k], m, n).reshape(n, n)).max() < 1e-12 * m


@pytest.mark.parametrize("n", [5, 64, 100, 256, 300, 512, 896])
def test_factor_once_backsolve(hip, n):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((3, n, n)); K = np.einsum("bij,bkj->bik", M, M) / n + np.eye(n)
    b = rng.standard_normal((3, n))
    x, _ = hip.chol_solve(K, b, repeat=2)
    assert np.abs(np.einsum("bij,bj->bi", K, x) - b).max() < 1e-11


# ---- SubsolverBase semantics ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,seed", [(2, 2, 1), (20, 30, 2), (64, 100, 3), (128, 200, 7), (256, 400, 9)])
def test_subsolver_matches_oracle_and_kkt(hip, oracle, n, m, seed):
    r2 = np.random.default_rng(seed)
    M = r2.standard_normal((n, n)); Q = M.T @ M / n + np.eye(n)
    A = r2.standard_normal((m, n)) / np.sqrt(n); xs = r2.standard_normal(n)
    lbA = A @ xs - r2.uniform(0.1, 1, m); ubA = A @ xs + r2.uniform(0.1, 1, m)
    lbA[: m // 8] = ubA[: m // 8]
    ubA[m // 8: m // 4] = np.inf
    lb = xs - r2.uniform(0.1, 2, n); ub = xs + r2.uniform(0.1, 2, n)
    lb[::3] = -np.inf; ub[1::3] = np.inf
    g = r2.standard_normal(n)
    qo = oracle.QP(Q, A); qh = hip.SubsolverHIP(n, m, Q, A)
    ro = qo.solve(True, g, lbA, ubA, np.zeros(n), None, lb, ub)
    rh = qh.solve(True, g, lbA, ubA, np.zeros(n), None, lb, ub)
    # same return code / exit flag; the iteration count may differ by a trial when a KKT residual sits at
    # the acceptance tolerance (fp64 summation order differs between the scalar oracle and the wave kernels)
    assert (ro[0], ro[2]) == (rh[0], rh[2]) == (0, 0) and abs(ro[1] - rh[1]) <= max(8, 0.03 * ro[1])
    (xo, yo), (xh, yh) = qo.solution(), qh.getSolution()
    assert np.abs(xo - xh).max() < X_TOL and np.abs(yo - yh).max() < Y_TOL
    stat, pf, cs = P.kkt_residuals(Q, g, A, lbA, ubA, lb, ub, xh, yh)
    assert stat < 1e-10 and pf < 1e-8 and cs < 1e-8
    for k in range(3):   # hot starts: only g changes (src/LCQProblem.cpp:1118, src/SubsolverQPOASES.cpp:158)
        g = g + 0.2 * r2.standard_normal(n)
        ro = qo.solve(False, g, lbA, ubA, None, None, lb, ub)
        rh = qh.solve(False, g, lbA, ubA, None, None, lb, ub)
        assert (ro[0], ro[2]) == (rh[0], rh[2]) == (0, 0) and abs(ro[1] - rh[1]) <= max(8, 0.03 * ro[1])
        (xo, yo), (xh, yh) = qo.solution(), qh.getSolution()
        assert np.abs(xo - xh).max() < X_TOL and np.abs(yo - yh).max() < Y_TOL
        stat, pf, cs = P.kkt_residuals(Q, g, A, lbA, ubA, lb, ub, xh, yh)
        assert stat < 1e-10 and pf < 1e-8 and cs < 1e-8
    co, ch = qo.counters(), qh.counters()
    # work counters: equal up to the trials a failed polish round spends differently (this seed needs ADMM rounds, and the
    # all-in / all-out working-set updates of a failing round amplify rounding differences); the solutions above agree
    assert all(abs(co[k] - ch[k]) <= max(12, 0.2 * co[k]) for k in co), (co, ch)
    qh.close()


def test_subsolver_hot_start_with_new_bound_values(hip, oracle):
    """SubsolverBase::solve takes the bounds with every call (src/Subsolver.cpp:94-110): hot starts whose bound VALUES change (same
    finite / equality pattern) -- rows that were far inside their bounds become violated, so the safe margins of the row screening
    must not survive the call"""
    n, m = 96, 160
    r2 = np.random.default_rng(11)
    M = r2.standard_normal((n, n)); Q = M.T @ M / n + np.eye(n)
    A = r2.standard_normal((m, n)) / np.sqrt(n); xs = r2.standard_normal(n)
    lbA = A @ xs - r2.uniform(2.0, 4.0, m); ubA = A @ xs + r2.uniform(2.0, 4.0, m)      # wide: almost every row inactive and safe
    g = r2.standard_normal(n)
    qo = oracle.QP(Q, A); qh = hip.SubsolverHIP(n, m, Q, A)
    ro = qo.solve(True, g, lbA, ubA, np.zeros(n), None); rh = qh.solve(True, g, lbA, ubA, np.zeros(n), None)
    assert (ro[0], ro[2]) == (rh[0], rh[2]) == (0, 0)
    for k in range(4):
        # tighten a different third of the rows around the current solution so that they cut it off
        xh, _ = qh.getSolution()
        ax = A @ xh
        lb2, ub2 = lbA.copy(), ubA.copy()
        sel = np.arange(k, m, 3)
        ub2[sel] = ax[sel] - 0.05 * (1 + k)
        lb2[sel] = np.minimum(lb2[sel], ub2[sel] - 1.0)
        ro = qo.solve(False, g, lb2, ub2, None, None); rh = qh.solve(False, g, lb2, ub2, None, None)
        assert (ro[0], ro[2]) == (rh[0], rh[2]) == (0, 0), (k, ro, rh)
        (xo, yo), (xh, yh) = qo.solution(), qh.getSolution()
        assert np.abs(xo - xh).max() < X_TOL and np.abs(yo - yh).max() < Y_TOL
        assert (A @ xh <= ub2 + 1e-8).all() and (A @ xh >= lb2 - 1e-8).all()
    qh.close()


def test_subsolver_certificates(hip, oracle):
    """exit flags 4 (infeasible) and 5 (unbounded) from the ADMM iterates, same as the oracle"""
    inf, unb = P.certificate_qps()
    for d, flag in ((inf, 4), (unb, 5)):
        n = d["g"].size
        qh = hip.SubsolverHIP(n, d["A"].shape[0], d["Q"], d["A"])
        qo = oracle.QP(d["Q"], d["A"])
        rh = qh.solve(True, d["g"], d["lbA"], d["ubA"], np.zeros(n), None, None, None)
        ro = qo.solve(True, d["g"], d["lbA"], d["ubA"], np.zeros(n), None, None, None)
        assert (rh[0], rh[2]) == (ro[0], ro[2]) == (203, flag), (rh, ro)
        assert rh[1] < 1500
        qh.close()


def test_subsolver_infeasible_bounds(hip):
    """test/RunUnitTests.cpp:463-502 at the subsolver level: lbA > ubA => SUBPROBLEM_SOLVER_ERROR, flag != 0"""
    q = hip.SubsolverHIP(2, 1, 2 * np.eye(2), np.array([[1., 0.]]))
    ret, it, ef = q.solve(True, np.array([-2., -2.]), np.array([0.]), np.array([-1.]), np.zeros(2))
    assert ret == 203 and ef != 0
    q.close()


def test_subsolver_warm_start_duals(hip, oracle):
    """initial solve with a dual guess y0 in the reference layout (box duals first, include/LCQProblem.ipp:143-151)"""
    rng = np.random.default_rng(11)
    n, m = 30, 40
    M = rng.standard_normal((n, n)); Q = M.T @ M / n + np.eye(n)
    A = rng.standard_normal((m, n)); xs = rng.standard_normal(n)
    lbA = A @ xs - 0.5; ubA = A @ xs + 0.5; g = rng.standard_normal(n)
    q1 = hip.SubsolverHIP(n, m, Q, A); q1.solve(True, g, lbA, ubA, np.zeros(n)); x1, y1 = q1.getSolution()
    q2 = hip.SubsolverHIP(n, m, Q, A); r2 = q2.solve(True, g, lbA, ubA, x1, y1); x2, y2 = q2.getSolution()
    assert r2[0] == 0 and np.abs(x1 - x2).max() < X_TOL and np.abs(y1 - y2).max() < Y_TOL
    qo = oracle.QP(Q, A); ro = qo.solve(True, g, lbA, ubA, x1, y1)
    assert (ro[0], ro[2]) == (r2[0], r2[2]) and abs(ro[1] - r2[1]) <= 2
    q1.close(); q2.close()


def test_subsolver_clone_owns_its_batch(hip):
    """lcqp_hip_qp_clone copies the problem data, the options, the last solution and the counters, never the batch: a clone builds its own
    device state in its first solve, whether it was taken before or after the original's first solve, and outlives the original.  The same
    QP through two objects gives the same bits (no atomics in the kernels); a hot start is held to the QP's KKT conditions at the
    tolerances of test_subsolver_matches_oracle_and_kkt."""
    n, m = 24, 12
    r = np.random.default_rng(5)
    M = r.standard_normal((n, n)); Q = M.T @ M / n + np.eye(n)
    A = r.standard_normal((m, n)) / np.sqrt(n); xs = r.standard_normal(n)
    lbA = A @ xs - r.uniform(0.1, 1, m); ubA = A @ xs + r.uniform(0.1, 1, m)
    lbA[:2] = ubA[:2]                                                  # two equalities
    lb = np.full(n, -np.inf); ub = np.full(n, np.inf)
    lb[:4] = xs[:4] - r.uniform(0.1, 1, 4); ub[:4] = xs[:4] + r.uniform(0.1, 1, 4)      # box bounds on four variables
    g = r.standard_normal(n)
    # (a) clone before the first solve
    qa = hip.SubsolverHIP(n, m, Q, A); qb = qa.clone()
    ra = qa.solve(True, g, lbA, ubA, np.zeros(n), None, lb, ub); rb = qb.solve(True, g, lbA, ubA, np.zeros(n), None, lb, ub)
    assert ra == rb and (ra[0], ra[2]) == (0, 0), (ra, rb)
    (xa, ya), (xb, yb) = qa.getSolution(), qb.getSolution()
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
    qa.close(); qb.close()
    # (b) clone after a solve; the original goes first
    qa = hip.SubsolverHIP(n, m, Q, A)
    ra = qa.solve(True, g, lbA, ubA, np.zeros(n), None, lb, ub)
    assert (ra[0], ra[2]) == (0, 0)
    (xa, ya), ca = qa.getSolution(), qa.counters()
    qb = qa.clone()
    assert all(np.array_equal(u, v) for u, v in zip(qb.getSolution(), (xa, ya))) and qb.counters() == ca
    qa.close()
    rb = qb.solve(False, g, lbA, ubA, np.zeros(n), None, lb, ub)      # not an initial solve, but no batch yet: a fresh setup of its own
    assert rb == ra, (ra, rb)
    xb, yb = qb.getSolution()
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
    assert qb.counters() == {k: 2 * v for k, v in ca.items()}          # the counters it took over plus the same work once more
    g2 = g + 0.2 * r.standard_normal(n)
    rb = qb.solve(False, g2, lbA, ubA, None, None, lb, ub)              # the same bound pattern: a hot start
    assert (rb[0], rb[2]) == (0, 0), rb
    xb, yb = qb.getSolution()
    stat, pf, cs = P.kkt_residuals(Q, g2, A, lbA, ubA, lb, ub, xb, yb)
    print("hot start of the clone: stat %.3g pf %.3g cs %.3g" % (stat, pf, cs))
    assert stat < 1e-10 and pf < 1e-8 and cs < 1e-8
    qb.close()


@pytest.mark.parametrize("n", [100, 256, 300, 512, 700, 1024, 1500, 2048, 3000, 4096])
def test_row_list_sweep(hip, n):
    """wg_rows through a row list with row-indexed scalars (stage 1 / stage 2 of the subsolver's trials) on its own, every padded size
    np = 128 ... 1024: row products for the listed rows only (the others keep their values), the weighted row sum over the list.
    (Round 2 saw this routine return wrong residuals inside the np = 1024 instantiation of the homotopy kernel.)"""
    rng = np.random.default_rng(n)
    batch, m = 3, 157
    A = rng.standard_normal((batch, m, n)); x = rng.standard_normal((batch, n)); coef = rng.standard_normal((batch, m))
    for nlist in (1, 16, 17, 60, 157):
        lists = np.stack([np.sort(rng.choice(m, nlist, replace=False)) for _ in range(batch)]).astype(np.int32)
        d0 = rng.standard_normal((batch, m))
        dots, out = hip.util_rows_list(A, lists, x=x, coef=coef, dots0=d0)
        for b in range(batch):
            ref = d0[b].copy(); ref[lists[b]] = A[b, lists[b]] @ x[b]
            assert np.abs(dots[b] - ref).max() < 1e-12 * n
            assert np.abs(out[b] - coef[b, lists[b]] @ A[b, lists[b]]).max() < 1e-12 * n
        dots2, _ = hip.util_rows_list(A, lists, x=x, dots0=d0)            # products only
        _, out2 = hip.util_rows_list(A, lists, coef=coef)                 # row sum only
        assert np.array_equal(dots2, dots) and np.array_equal(out2, out)


# ---- LCQProblem::loadLCQP / runSolver on the device ----------------------------------------------------
def _cmp(ro, rh, xtol=X_TOL, ytol=Y_TOL, iters=True, status=True):
    assert rh["ret"] == ro["ret"]
    so, sh = ro["stats"], rh["stats"]
    if iters:
        for k in ("iterTotal", "iterOuter", "rhoOpt") + (("status",) if status else ()):
            assert so[k] == sh[k], (k, so, sh)
    if ro["ret"] == 0:
        assert np.abs(ro["x"] - rh["x"]).max() < xtol
        assert np.abs(ro["y"] - rh["y"]).max() < ytol


@pytest.mark.parametrize("name", ["warm_up_binary", "circle", "example_data"])
def test_lcqp_reference_problems(hip, oracle, name):
    """BASELINE config C2 (circle) and the reference's other fixtures: iterate counts, rho, status, x, y"""
    d = getattr(P, name)()
    ro = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0))
    rh = P.hip_solve(hip, d, hip.default_options(perturbStep=0))
    if name == "example_data":
        # box bounds duplicate complementarity rows in this fixture (lb = 0 on variables that L selects), so
        # the multipliers of the duplicated rows are not unique: compare x and the dual-dependent quantity
        # that is unique, the LCQP stationarity residual  Qx + g - A'y_A - L'y_L - R'y_R - y_box
        # (the stationarity TYPE, src/LCQProblem.cpp:1412-1453, is read off the signs of the multipliers of L and R; on biactive pairs whose
        # rows are duplicated by a box bound it depends on how the unique SUM is split between the duplicates -- S or W for the same point)
        _cmp(ro, rh, xtol=1e-7, ytol=np.inf, status=False)
        # Stationarity type (a parity output, row (a)13): each side reports what the reference's rule (src/LCQProblem.cpp:1412-1482) gives on ITS
        # multipliers.  Pair 25 has L_25 = -e_38 while variable 38 sits on its box bound lb = 0, two constraints that pin x_38 from both sides, so
        # only -y_L25 + y_box38 = -0.0538 is defined (equal on both sides, asserted below through `comb`) and any amount can be added to both
        # multipliers.  Until round 4 the oracle returned -5e-11 on the row (W: a negative multiplier on a biactive pair) and the device +0.029
        # (S); since the subsolver holds its active rows to their rounding floor (round 5) both sides return the same split and the same raw
        # type, S, which is also the committed golden value.  The rule applied to the most favourable admissible split
        # (problems.stationarity_type, merge_box) -- "there EXIST multipliers with these signs", the definition of the types -- gives S too.
        for r in (ro, rh):
            assert r["stats"]["status"] == P.stationarity_type(d, r["x"], r["y"], r["stats"]["rhoOpt"])
        assert ro["stats"]["status"] == rh["stats"]["status"] == int(GOLD["example_data_stats"][3]) == 4
        assert P.stationarity_type(d, ro["x"], ro["y"], ro["stats"]["rhoOpt"], merge_box=True) == \
               P.stationarity_type(d, rh["x"], rh["y"], rh["stats"]["rhoOpt"], merge_box=True) == 4
        n, nC, nComp = d["nV"], d["nC"], d["nComp"]
        for r in (ro, rh):
            yy = r["y"]
            stat = (d["Q"] @ r["x"] + d["g"] - d["A"].T @ yy[n:n + nC] - d["L"].T @ yy[n + nC:n + nC + nComp]
                    - d["R"].T @ yy[n + nC + nComp:] - yy[:n])
            # transformDuals (src/LCQProblem.cpp:1381-1409) does not shift by lbL/lbR, so with non-zero lower
            # complementarity bounds the identity holds up to rho * g_phi = -rho (R'lbL + L'lbR)  (:969-996)
            stat = stat - r["stats"]["rhoOpt"] * (d["R"].T @ d["lbL"] + d["L"].T @ d["lbR"])
            assert np.abs(stat).max() < 1e-8
        # the duals themselves, modulo the duplicated rows only: the multipliers of A, and per variable the sum of the multipliers of the
        # rows that coincide on it (its box bound and the one-hot rows of L and R)
        comb = lambda yy: d["L"].T @ yy[n + nC:n + nC + nComp] + d["R"].T @ yy[n + nC + nComp:] + yy[:n]
        assert np.abs(ro["y"][n:n + nC] - rh["y"][n:n + nC]).max() < 1e-5
        assert np.abs(comb(ro["y"]) - comb(rh["y"])).max() < 1e-5
    else:
        _cmp(ro, rh, xtol=1e-7 if name != "warm_up_binary" else X_TOL, ytol=1e-5)
    s = GOLD[name + "_stats"]
    nst = 3 if name == "example_data" else 4
    assert [rh["ret"], rh["stats"]["iterTotal"], rh["stats"]["iterOuter"], rh["stats"]["status"]][:nst] == list(s[:nst].astype(int))
    assert np.abs(rh["x"] - GOLD[name + "_x"]).max() < 1e-7
    if name == "circle":     # examples/OptimizeOnCircle.cpp:144
        assert np.abs(rh["x"][:2] - [0.1811, -0.9835]).max() < 1e-4


@pytest.mark.parametrize("name", ["circle", "warm_up_binary", "synthetic", "example_data"])
def test_lcqp_iterate_level_match(hip, oracle, name):
    """BASELINE config C2: per-iterate match against the CPU restatement (storeSteps tracking on the device):
    same number of iterates, same rho sequence, ||xk_gpu - xk_cpu||_inf, stationarity and complementarity per
    iterate.  (The step length alpha = -lk/qk is not compared: it is an ill-conditioned ratio once |pk| ~ 1e-8.)"""
    if name == "synthetic":
        d = oracle.synth_generate(1, 64, 96, 16)
    else:
        d = getattr(P, name)()
    ro = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0), trace=400)
    rh = P.hip_solve(hip, d, hip.default_options(perturbStep=0, storeSteps=1), trace=True)
    so, sh = ro["trace_scalars"], rh["trace_scalars"]
    assert len(so) == ro["stats"]["iterTotal"] and len(sh) == rh["stats"]["iterTotal"]
    if name == "synthetic":
        # The step-length test at the end of an inner loop is a coin flip at the rounding floor (oracle/lcqp_oracle.c, dot_lanes;
        # tests/test_oracle_solver.py::test_iterate_path_is_a_coin_flip_at_the_rounding_floor): the two sides walk the same path iterate
        # for iterate until one flip sends a penalty update one cycle of four iterates earlier or later; they meet again in the solution.
        k = min(len(so), len(sh))
        diff = np.nonzero(so[:k, 2] != sh[:k, 2])[0]
        k = int(diff[0]) if diff.size else k
        assert k >= 8 and (len(so) - len(sh)) % 4 == 0 and np.abs(ro["x"] - rh["x"]).max() < 1e-9
        ro = dict(ro, trace_x=ro["trace_x"][:k - 1]); rh = dict(rh, trace_x=rh["trace_x"][:k - 1])
        so, sh = so[:k - 1], sh[:k - 1]
    assert len(so) == len(sh)
    assert np.array_equal(so[:, 2], sh[:, 2])                                   # rho per iterate
    # Every iterate is a QP solution verified to resTol * (1 + |gk|_inf) = 1e-12 * (1 + rho |C xk| + ...) on both sides, so with
    # rho up to 1e3 on these problems two correct solvers may differ by 1e-9 in an intermediate xk (the final x is compared at
    # 1e-9 elsewhere: at convergence the complementarity pairs are exact zeros).  PSD Hessians (flat directions): 1e-7.
    # example_data: PSD Hessian AND duplicated rows, so the QPs as given have many minimisers; the subsolver returns the one the
    # proximal-point iteration from the previous iterate leads to (round 3: every step of it has a unique solution), the same on
    # both sides at every iterate.
    tol = 1e-7 if name in ("circle", "example_data") else 1e-8
    assert np.abs(ro["trace_x"] - rh["trace_x"]).max() < tol
    assert np.abs(so[:, 1] - sh[:, 1]).max() < 10 * tol                         # complementarity per iterate
    assert np.abs(so[:, 0] - sh[:, 0]).max() < 10 * tol                         # stationarity per iterate


def test_iterate_counts_against_the_oracle_are_unbiased(hip, oracle):
    """whether an inner loop ends at an iterate or one cycle of four iterates later is a coin flip at the rounding
    floor, so the two sides differ in the iterate count of about a third of the instances -- but with no bias (round 2 had +4 four times
    as often as -4; the whole-workload log is profiles/round3/full_parity_8192.log), by whole inner cycles, with identical return
    codes and the same solutions."""
    import os
    N = 512
    bt = hip.BatchLCQP(N, 256, 512, 64, opt=hip.default_options(perturbStep=0, printLevel=0))
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    ok, xo, yo, so = oracle.synth_batch_solve(0, N, 256, 512, 64, opt=oracle.default_options(perturbStep=0, printLevel=0),
                                              threads=len(os.sched_getaffinity(0)))
    assert ok == N and all(s["returnValue"] == 0 for s in st)
    assert np.abs(x - xo).max() < X_TOL and np.abs(y - yo).max() < Y_TOL
    d = np.array([s["iterTotal"] for s in st]) - np.array([s["iterTotal"] for s in so])
    assert (d % 4 == 0).mean() >= 0.99                       # whole inner cycles (a +-1 needs a flip in the very last iterate)
    assert abs(d.mean()) < 0.6, d.mean()                     # 5 sigma of the mean of 512 fair +-4 flips at rate 0.35
    # measured: 36.5 % of 8192 instances differ (profiles/round3/full_parity_8192.log); 512 draws at that rate stay below 0.45 at 4 sigma
    assert (d != 0).mean() < 0.45, (d != 0).mean()
    # everything that does not hinge on the coin is equal: return codes (above), and -- for the instances that took the same number of
    # iterates -- the number of penalty updates and the final penalty parameter
    same = d == 0
    assert all(st[i]["iterOuter"] == so[i]["iterOuter"] and st[i]["rhoOpt"] == so[i]["rhoOpt"] and st[i]["status"] == so[i]["status"] for i in np.nonzero(same)[0])
    # Parity does not hinge on the summation order the oracle shares with the device (oracle/lcqp_oracle.c: dot_lanes): the same 512 instances
    # against the PLAIN-order oracle (E x summed left to right), solutions only
    oracle.qp_set_sum_order(0)
    try:
        ok0, xo0, yo0, so0 = oracle.synth_batch_solve(0, N, 256, 512, 64, opt=oracle.default_options(perturbStep=0, printLevel=0),
                                                      threads=len(os.sched_getaffinity(0)))
    finally:
        oracle.qp_set_sum_order(1)
    assert ok0 == N and np.abs(x - xo0).max() < X_TOL and np.abs(y - yo0).max() < Y_TOL
    assert all(a["status"] == b_["status"] for a, b_ in zip(st, so0))
    bt.close()


def test_lcqp_run_warm_up(hip):
    """SolverTest.RunWarmUp (test/RunUnitTests.cpp:505-551) on the HIP path, 20 seeds"""
    d = P.warm_up()
    tol = 1e6 * 2.221e-16
    found = set()
    for i in range(20):
        r = P.hip_solve(hip, d, hip.default_options(perturbSeed=1000 + i))
        assert r["ret"] == 0
        x, y = r["x"], r["y"]
        s1 = abs(x[0] - 1) <= tol and abs(x[1]) <= tol
        s2 = abs(x[1] - 1) <= tol and abs(x[0]) <= tol
        assert s1 or s2
        found.add(1 if s1 else 2)
        assert abs(2 * x[0] - 2 - y[0] - y[2]) <= tol and abs(2 * x[1] - 2 - y[1] - y[3]) <= tol
    assert found == {1, 2}


def test_lcqp_error_codes(hip):
    """infeasible QP => SUBPROBLEM_SOLVER_ERROR with a non-zero flag (RunUnitTests.cpp:463-502);
    maxPenaltyParameter = 1 => MAX_PENALTY_REACHED (test/examples/test_max_penalty.cpp:49,75-79)"""
    r = P.hip_solve(hip, P.infeasible(), hip.default_options())
    assert r["ret"] == 203 and r["stats"]["qpSolverExitFlag"] != 0
    r = P.hip_solve(hip, P.warm_up_x0(), hip.default_options(maxPenaltyParameter=1.0, perturbStep=0))
    assert r["ret"] == 201
    r = P.hip_solve(hip, P.warm_up_w_A(), hip.default_options())
    assert r["ret"] == 0


def test_lcqp_load_argument_errors(hip):
    """NULL checks of loadLCQP: include/LCQProblem.ipp:44-45, src/LCQProblem.cpp:569-570,611-612,747-748"""
    d = P.warm_up()
    bt = hip.BatchLCQP(1, 2, 1, 1)
    assert bt.load(0, 1, d["Q"], None, d["L"], d["R"]) == 116
    assert bt.load(0, 1, d["Q"], d["g"], d["L"], d["R"]) == 117          # nC > 0 but A == NULL
    assert bt.load(0, 1, d["Q"], d["g"], None, d["R"], A=np.zeros((1, 2))) == 118
    assert bt.load(0, 1, d["Q"], d["g"], d["L"], d["R"], lbL=np.array([-np.inf]), A=np.zeros((1, 2))) == 120
    bt.close()


@pytest.mark.parametrize("B,n,nC,nComp", [(6, 64, 96, 16), (4, 256, 512, 64), (3, 130, 70, 20)])
def test_lcqp_synthetic_vs_oracle(hip, oracle, B, n, nC, nComp):
    """device-generated instances, read back, solved by both sides"""
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    oopt = oracle.default_options(perturbStep=0)
    same_path = 0
    for b in range(B):
        d = bt.read_problem(b)
        host = oracle.synth_generate(b, n, nC, nComp)
        for k in ("g", "A", "L", "R", "Q", "lbA", "ubA"):
            # counter-based generator, and the two reductions (M'M, A x*) summed in the host's order on the device:
            # the instance in HBM is bit-identical to the one the oracle generates
            assert np.array_equal(d[k], host[k]), k
        ro = oracle.lcqp_solve(d["Q"], d["g"], d["L"], d["R"], A=d["A"], lbA=d["lbA"], ubA=d["ubA"], opt=oopt)
        assert st[b]["returnValue"] == ro["ret"] == 0
        assert np.abs(ro["x"] - x[b]).max() < X_TOL and np.abs(ro["y"] - y[b]).max() < Y_TOL
        same_path += int(st[b]["iterTotal"] == ro["stats"]["iterTotal"] and st[b]["trials"] == ro["stats"]["trials"])
        xb = x[b]
        assert abs((d["L"] @ xb) @ (d["R"] @ xb)) < 1e3 * 2.221e-16          # complementarity tolerance
    assert same_path >= (B + 1) // 2     # iterate counts agree except for tolerance-borderline instances
    bt.close()


@pytest.mark.parametrize("B,n,nC,nComp", [(5, 256, 512, 64), (3, 200, 330, 37), (1040, 128, 96, 32), (800, 300, 96, 40)])
def test_setup_kernel_choices_give_the_same_bits(hip, B, n, nC, nComp):
    """lcqp_hip_batch_set_overlapped (the streamed form of Et = E inv(L1)' for a setup beside another batch's homotopy) and the instantiation of
    k_factor for batches of more than three workgroups per CU (B = 1040) are speed choices: every element is the same chain of operations.  So is
    the 256-register build of k_lcqp_run that batches of at most three workgroups per CU run (np <= 512): instances 0, 1 solved in a batch of 2
    and in the larger batch (B = 1040 and B = 800 are beyond three per CU on a 256-CU device) are the same bits"""
    res = []
    for overlapped in (False, True):
        bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
        bt.set_overlapped(overlapped)
        bt.generate_synthetic(0)
        bt.run()
        res.append(bt.solution())
        bt.close()
    small = hip.BatchLCQP(2, n, nC, nComp, opt=hip.default_options(perturbStep=0))      # instances 0, 1 through the kernels of a small batch
    small.generate_synthetic(0)
    small.run()
    xs, ys, sts = small.solution()
    small.close()
    (x0, y0, st0), (x1, y1, st1) = res
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
    assert [s["iterTotal"] for s in st0] == [s["iterTotal"] for s in st1]
    assert np.array_equal(x0[:2], xs) and np.array_equal(y0[:2], ys)
    assert all(s["returnValue"] == 0 for s in st0)


def test_lcqp_synthetic_golden(hip):
    bt = hip.BatchLCQP(4, 256, 512, 64, opt=hip.default_options(perturbStep=0))
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    for b in range(4):
        assert st[b]["returnValue"] == 0
        assert np.abs(x[b] - GOLD[f"synth_256_{b}_x"]).max() < 1e-8
    bt.close()


def test_lcqp_full_batch_properties(hip, oracle):
    """BASELINE config C3 at full size (B=1024, n=256, nC=512, nComp=64): size-independent properties --
    every instance terminates successfully, is complementary to the reference tolerance, primal feasible,
    and the returned (transformed) duals satisfy LCQP stationarity  Qx + g - A'y_A - L'y_L - R'y_R = 0."""
    B, n, nC, nComp = 1024, 256, 512, 64
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    assert all(s["status"] in (1, 2, 3, 4) for s in st)
    Lx = x[:, :nComp]; Rx = x[:, nComp:2 * nComp]          # one-hot selectors of the generator
    assert np.abs((Lx * Rx).sum(axis=1)).max() < 1e3 * 2.221e-16
    assert Lx.min() > -1e-9 and Rx.min() > -1e-9
    # The independent property check over the WHOLE batch (nothing here shares code with the homotopy): primal feasibility, LCQP stationarity
    # of the returned (transformed) duals, sign and complementary slackness of the row multipliers -- a few einsums per chunk of instances
    # read back from HBM (bit-identical to the host generator: test_lcqp_synthetic_vs_oracle).
    worst = dict(feas=0.0, stat=0.0, slack=0.0, sign=0.0)
    probs = {}
    for c0 in range(0, B, 128):
        ds = [bt.read_problem(b) for b in range(c0, c0 + 128)]
        for k_, b in enumerate(range(c0, c0 + 128)):
            if b % 16 == 0:
                probs[b] = ds[k_]                                             # the 64-instance sample of the branch-QP check below
        Qs = np.stack([d["Q"] for d in ds]); As = np.stack([d["A"] for d in ds]); gs = np.stack([d["g"] for d in ds])
        lo = np.stack([d["lbA"] for d in ds]); hi = np.stack([d["ubA"] for d in ds])
        xs, ys = x[c0:c0 + 128], y[c0:c0 + 128]
        Ax = np.einsum("brc,bc->br", As, xs)
        yA, yL, yR, ybox = ys[:, n:n + nC], ys[:, n + nC:n + nC + nComp], ys[:, n + nC + nComp:], ys[:, :n]
        stat = np.einsum("bij,bj->bi", Qs, xs) + gs - np.einsum("brc,br->bc", As, yA) - ybox
        stat[:, :nComp] -= yL; stat[:, nComp:2 * nComp] -= yR                 # L = [I 0 0], R = [0 I 0] (checked against the read-back below)
        assert all(np.array_equal(d["L"], np.eye(nComp, n)) and np.array_equal(d["R"], np.eye(nComp, n, nComp)) for d in ds[:4])
        worst["feas"] = max(worst["feas"], float(np.maximum(lo - Ax, Ax - hi).max()))
        worst["stat"] = max(worst["stat"], float(np.abs(stat).max()))
        # dual layout of SURVEY.md §8(b): y >= 0 on a row at its lower bound, <= 0 at its upper bound, zero strictly inside
        dlo, dhi = Ax - lo, hi - Ax
        worst["slack"] = max(worst["slack"], float((np.abs(yA) * np.minimum(dlo, dhi)).max()))
        worst["sign"] = max(worst["sign"], float(np.maximum(np.where(dlo > 1e-7, yA, 0.0).max(), np.where(dhi > 1e-7, -yA, 0.0).max())))
        assert np.abs(ybox).max() == 0.0                                      # no box bounds in this workload
    assert worst["feas"] < 1e-8 and worst["stat"] < 1e-8 and worst["slack"] < 1e-8 and worst["sign"] < 1e-8, worst
    # S-stationary points minimise the convex QP of their complementarity branch (biactive pairs as inequalities); the branch QP is solved
    # by the QP solver alone, no homotopy involved: every S-stationary instance of a 64-instance sample
    nS = 0
    for b, d in probs.items():
        if st[b]["status"] == 4:
            dd = dict(d); dd.update(nV=n, nC=nC, nComp=nComp)
            xb = P.branch_qp_solution(oracle, dd, x[b])
            assert xb is not None and np.abs(xb - x[b]).max() < 1e-7, b
            nS += 1
    assert nS >= 32
    # second run on the same handle reproduces the first bit for bit (determinism with perturbStep = 0)
    bt.run()
    x2, y2, st2 = bt.solution()
    assert np.array_equal(x, x2) and np.array_equal(y, y2)
    # byte accounting of bench.py's roofline: the C ABI's total is the documented formula applied to the work
    # counters and active-row sums the kernel keeps
    ws = bt.work_sums()
    m = nC + 2 * nComp
    bs = 8.0 * n * (n + 2)
    tot = lambda k: float(sum(s[k] for s in st2))
    # ws = (rows of Et read by the corrections, entries of the inverse factor read by the corrections, bytes moved by working-set updates, number of updates, rows of E read by
    #       the sweeps, triangular solves with L1)
    expect = (tot("reserved") * 8.0 * n * n + 8.0 * n * ws[4] + ws[5] * 0.5 * bs + 8.0 * ws[0] * n + 8.0 * (ws[1] + ws[0])
              + ws[2] + tot("admmIter") * (bs + 16.0 * m * n) + B * 16.0 * n * n + (tot("iterTotal") + B) * 12.0 * (2 * nComp))
    # (LCQP level: one sweep over Q and C per homotopy; C pk per iterate from the 2 nComp non-zeros of C = L'R + R'L for one-hot L, R)
    assert abs(bt.algorithmic_bytes() - expect) <= 1e-9 * expect
    assert tot("corrections") <= ws[5] <= 2 * tot("corrections")                  # one or two triangular solves per correction
    assert 64 < ws[0] / ws[5] < n and ws[1] >= (ws[0] / 2) ** 2 / tot("corrections") / 4
    assert ws[3] == tot("factorizations") and ws[2] > 0
    # one true-residual sweep per QP (plus the cold one); intermediate trials read only unscreened inactive rows
    assert tot("reserved") <= tot("qpSolves") * 1.25 + B
    assert ws[4] / tot("trials") < 0.6 * m
    bt.close()


@pytest.mark.parametrize("kw", [dict(admmFirst=20), dict(admmFirst=10, admmHot=5), dict(maxTrials=3)])
def test_lcqp_polish_after_admm(hip, oracle, kw):
    """the polish entered from ADMM iterates (admmFirst / admmHot > 0, or a trial budget so small that the fallback rounds run): ADMM
    writes its own E x and moves x without the polish knowing, so the polish must not trust margins or row values from before (cold
    entry: every row is read, margins rebuilt) -- same trials, same working sets, same solutions as the oracle, which screens nothing"""
    B, n, nC, nComp = 6, 64, 96, 16
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0, **kw))
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    for b in range(B):
        d = bt.read_problem(b)
        ro = oracle.lcqp_solve(d["Q"], d["g"], d["L"], d["R"], A=d["A"], lbA=d["lbA"], ubA=d["ubA"], opt=oracle.default_options(perturbStep=0, **kw))
        assert st[b]["returnValue"] == ro["ret"] == 0
        assert np.abs(ro["x"] - x[b]).max() < X_TOL and np.abs(ro["y"] - y[b]).max() < Y_TOL
        assert st[b]["admmIter"] == ro["stats"]["admmIter"] > 0
        assert abs(st[b]["trials"] - ro["stats"]["trials"]) <= 0.05 * ro["stats"]["trials"] + 4
    bt.close()


def test_lcqp_default_options_with_perturbation(hip, oracle):
    """reference defaults (perturbStep = true, src/Options.cpp:303) on the synthetic workload: the seeded
    perturbation stream is identical on both sides, so iterates still match the oracle"""
    B, n, nC, nComp = 16, 256, 512, 64
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options())
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    oopt = oracle.default_options()
    for b in (0, 7, 15):
        d = bt.read_problem(b)
        ro = oracle.lcqp_solve(d["Q"], d["g"], d["L"], d["R"], A=d["A"], lbA=d["lbA"], ubA=d["ubA"], opt=oopt)
        assert ro["ret"] == 0 and np.abs(ro["x"] - x[b]).max() < X_TOL
    bt.close()


def test_lcqp_node_sized_batch_on_one_gpu(hip):
    """BASELINE config C4's 8192 instances (8 x 1024) resident on ONE GPU (51 GB of the 288 GB): every
    instance solves; the shard [1024, 2048) equals what rank 1 of the sharded run computes."""
    n, nC, nComp = 256, 512, 64
    bt = hip.BatchLCQP(8192, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    assert all(s["returnValue"] == 0 for s in st)
    assert np.abs((x[:, :nComp] * x[:, nComp:2 * nComp]).sum(axis=1)).max() < 1e3 * 2.221e-16
    bt.close()
    b1 = hip.BatchLCQP(1024, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    b1.generate_synthetic(1024)          # rank 1's slice of instance ids
    b1.run()
    x1, _, _ = b1.solution()
    b1.close()
    assert np.array_equal(x1, x[1024:2048])


def test_csc_products_on_device(hip, oracle):
    """CSC Utilities on the device vs the oracle restatement: the reference's dense known
    answers through CSC, and random sparse matrices up to the BASELINE config-5 size n = 4096."""
    L = oracle._csc_setup()
    # known answers of test/RunUnitTests.cpp:33-78 through CSC
    A = np.array([[1., 0, 2], [3, 1, 1]])
    S = oracle.dns_to_csc(A); m, n, p, i, x = oracle.csc_arrays(S)
    M = hip.CSCMatrix(m, n, p, i, x)
    assert list(M.apply([98., -10], transposed=True)) == [68, -10, 186]
    assert list(M.apply([2., 0, 1])) == [4, 7]
    M.close()
    rng = np.random.default_rng(4)
    for (m, n, dens) in ((7, 5, 0.4), (640, 256, 0.05), (4096, 4096, 0.003)):
        A = np.where(rng.random((m, n)) < dens, rng.standard_normal((m, n)), 0.0)
        if m == n:
            A = A + A.T
        S = oracle.dns_to_csc(A); _, _, p, i, x = oracle.csc_arrays(S) if m < 1000 else (None, None, *_csc_np(A))
        M = hip.CSCMatrix(m, n, p, i, x)
        b = rng.standard_normal(n); bt = rng.standard_normal(m); c = rng.standard_normal(n)
        ref = np.zeros(m); L.orc_csc_matmul(S, oracle._p(b), oracle._p(ref))
        assert np.abs(M.apply(b) - ref).max() < 1e-12 * max(1, np.abs(ref).max())
        reft = np.zeros(n); L.orc_csc_matmul_t(S, oracle._p(bt), oracle._p(reft))
        assert np.abs(M.apply(bt, transposed=True) - reft).max() < 1e-12 * max(1, np.abs(reft).max())
        if m == n:      # AffineLinearTransformation / QuadraticFormProduct for symmetric S
            d = np.zeros(n); L.orc_csc_affine(2.0, S, oracle._p(b), oracle._p(c), oracle._p(d), n)
            dh = M.apply(b, transposed=True, alpha=2.0, c=c)
            assert np.abs(dh - d).max() < 1e-12 * max(1, np.abs(d).max())
            qf = L.orc_csc_quadform(S, oracle._p(b), n)
            assert abs(b @ M.apply(b, transposed=True) - qf) < 1e-10 * max(1, abs(qf))
        M.close()


def _csc_np(A):
    """CSC arrays of a dense matrix with numpy (column-major scan, as dns_to_csc does)"""
    cols, rows = np.nonzero(A.T)
    p = np.zeros(A.shape[1] + 1, dtype=np.int32)
    np.add.at(p, cols + 1, 1)
    return np.cumsum(p).astype(np.int32), rows.astype(np.int32), A.T[cols, rows]


@pytest.mark.parametrize("n,nC,nComp", [(512, 256, 128), (384, 700, 100), (100, 0, 50), (33, 17, 16), (256, 1500, 64),
                                        (2, 0, 1), (129, 64, 1), (64, 640, 8), (513, 0, 50), (600, 300, 100), (1024, 600, 256)])
def test_lcqp_shape_sweep(hip, oracle, n, nC, nComp):
    """every padded-size variant of the kernels (np = 128, 256, 384, 512 and, for 512 < nV <= 1024, 1024), nC = 0, more rows
    than the BASELINE shape"""
    B = 3 if n <= 512 else 2
    bt = hip.BatchLCQP(B, n, nC, nComp, opt=hip.default_options(perturbStep=0))
    bt.generate_synthetic(0)
    bt.run()
    x, y, st = bt.solution()
    for b in range(B):
        d = bt.read_problem(b)
        ro = oracle.lcqp_solve(d["Q"], d["g"], d["L"], d["R"], A=d["A"] if nC else None, lbA=d["lbA"] if nC else None,
                               ubA=d["ubA"] if nC else None, opt=oracle.default_options(perturbStep=0), nV=n, nC=nC, nComp=nComp)
        assert st[b]["returnValue"] == ro["ret"] == 0
        assert np.abs(ro["x"] - x[b]).max() < X_TOL and np.abs(ro["y"] - y[b]).max() < Y_TOL
    bt.close()


def test_mixed_shapes_and_bounds_in_one_call(hip):
    """The reference is one object per problem, any mix of sizes and of optional arguments (include/LCQProblem.hpp:56-60, 87-144).  One call of
    lcqpow_amd.solve_mixed (C++: LCQPow::MixedBatchLCQProblem) takes problems of three shapes, with and without lbL / lbR, box bounds, A and
    x0, in shuffled order: every instance returns the bits of its solo run.  (Until round 6 a batch refused to mix instances with and without
    lbL / lbR; an absent vector is the zero vector -- setComplementarityBounds :726-785 -- and the same arithmetic.)"""
    rng = np.random.default_rng(7)
    probs = []
    for n, nC, nComp in ((12, 5, 3), (40, 20, 8), (70, 0, 16)):
        for variant in range(4):
            M = rng.uniform(-1, 1, (n, n)); Q = M.T @ M / n + np.eye(n)
            g = rng.uniform(-1, 1, n)
            L = np.zeros((nComp, n)); R = np.zeros((nComp, n))
            for i in range(nComp):
                L[i, i] = 1.0; R[i, nComp + i] = 1.0
            xs = rng.uniform(0.2, 1, n); xs[nComp:2 * nComp] = 0.0
            d = dict(Q=Q, g=g, L=L, R=R, nV=n, nC=nC, nComp=nComp)
            if nC:
                A = rng.uniform(-1, 1, (nC, n)) / np.sqrt(n)
                d.update(A=A, lbA=A @ xs - rng.uniform(0.1, 1, nC), ubA=A @ xs + rng.uniform(0.1, 1, nC))
            if variant & 1:      # shifted complementarity bounds on some instances of a bucket only
                d.update(lbL=rng.uniform(-0.2, 0.0, nComp), lbR=rng.uniform(-0.2, 0.0, nComp))
            if variant & 2:      # box bounds: another bucket of the same (nV, nC, nComp)
                d.update(lb=xs - 2.0, ub=np.where(rng.random(n) < 0.5, xs + 2.0, np.inf))
            if variant == 3:
                d.update(x0=rng.uniform(-0.1, 0.1, n))
            probs.append(d)
    order = rng.permutation(len(probs))
    mixed = [probs[i] for i in order]
    opt = hip.default_options(perturbStep=0)
    res = hip.solve_mixed(mixed, opt=opt)
    assert len(res) == len(mixed)
    nbuckets = len({(d["nV"], d["nC"], d["nComp"], "lb" in d) for d in mixed})
    assert nbuckets == 6
    for d, r in zip(mixed, res):
        solo = P.hip_solve(hip, d, opt)
        assert r["ret"] == solo["ret"] == 0, (d["nV"], r["ret"], solo["ret"])
        assert np.array_equal(r["x"], solo["x"]) and np.array_equal(r["y"], solo["y"]) and r["stats"] == solo["stats"]
        if "lbL" not in d:      # (with shifted bounds the reference leaves rho g_phi out of g_tilde until the first penalty update, src/LCQProblem.cpp:966-967: reproduced, and not a stationary point of the shifted problem when the homotopy ends before one)
            stat, feas, compl, sign = P.lcqp_kkt_residuals(d, r["x"], r["y"], r["stats"]["rhoOpt"])
            assert stat < 1e-8 and feas < 1e-8 and compl < 1e-9, (stat, feas, compl)


def _fuzz_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpu_fuzz", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gpu_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def test_lcqp_structure_fuzz(hip, oracle):
    """tools/gpu_fuzz.py: random small LCQPs with the irregular structure the synthetic generator never produces (singular
    Hessians, dense / overlapping complementarity rows, equalities, duplicate and empty rows, finite upper complementarity
    bounds, box bounds, warm-start duals; about a quarter are infeasible or unbounded by construction).  HIP and oracle must
    end the same way: the SAME RETURN CODE on every problem and, on success, the same solution.  Until round 4 a few per cent
    differed (bound: 5 %) because the subsolver accepted active rows at 1e-12 while runSolver ends on phi < 1e3 eps
    (src/LCQProblem.cpp:511-534, src/Options.cpp:297); since the rows of the factor are held to their rounding floor (round 5) the five
    sets of tools/run_fuzz_sets.sh (1750 problems) show no differing return code and one other stationary point
    (profiles/round5/fuzz_*.log).  Asserted here on seed 5: no return code differs, at most 1 % other stationary points."""
    fz = _fuzz_module()
    count = 150
    cats, rets = fz.run(count, seed=5, verbose=False)
    assert cats["return codes differ"] == 0, (cats, rets)
    assert cats["other stationary point"] <= count // 100, (cats, rets)
    assert cats.get("branch minimiser checked", 0) >= count // 8 and cats.get("NOT a branch minimiser", 0) == 0, cats
    assert rets.get((0, 0), 0) >= count // 2, rets          # the generator is not mostly producing failures


@pytest.mark.parametrize("seed,ids", [(1, (542, 550, 555)), (3, (12, 70)), (11, (34, 277)), (15, (200,)), (22, (283,)), (8, (370,)), (9, (243,))])
def test_fuzz_regressions_end_the_same_way(hip, oracle, seed, ids):
    """The fuzz problems on which HIP and the oracle used to end differently (profiles/round4/fuzz_batched_seed1_600.log, fuzz_host.log,
    fuzz_diverge.log): seed 1 id 542 (oracle 0 / HIP 203: HIP stood at phi = 9e-13 above the 2.2e-13 tolerance and raised the penalty until a
    QP failed), ids 550 and seed 3 id 70 (201 / 203), seed 11 ids 34 and 277 and the oracle-vs-oracle cases seed 1 id 555, seed 3 id 12 (other
    stationary points after one side passed the termination test at its rounding floor).  Two causes, both removed in round 5: the subsolver
    accepted active rows at resTol (1 + |b|) = 1e-12 instead of their rounding floor, and the device carried C xk along the steps by linearity,
    forty roundings of eps |C xk| against a complementarity value that cancels to 1e3 eps (getPhi, src/LCQProblem.cpp:1172-1185).  The damped
    polish (one change of the working set per trial after three failed rounds) settles the LP-like QPs at rho ~ 1e7 of ids 550 and 70.
    Seed 15 id 200 and seed 22 id 283 (oracle MAX_ITERATIONS_REACHED, HIP 0; profiles/round5/fuzz_campaign_before_dependent_row_reset.log): two parallel
    equality rows whose multipliers drifted to 5e11 and -6e10 over the hot starts -- only their sum is determined -- until the cancellation error
    of A'y alone, 1.1e-7, kept the stationarity test from ever passing at a stationary point; a hot start now resets the multiplier of a row that
    is flagged dependent (qp_solve / orc_qp_solve).
    Round 6: seed 8 id 370 (oracle 0 / HIP 203 at the very FIRST QP): a QP whose solution lies far out along a flat direction of its Hessian
    (|g| = 2, |Qx| = |E'y| = 1e3, |x| = 4e5); the stationarity residual was tested against resTol (1 + |g|) = 3e-12, i.e. 3e-15 relative to the
    terms it is the sum of, and the refinement stagnated at 7e-12 with the right working set for forty rounds (profiles/round6/fuzz/case370_*.log).
    The tolerance now has the residual's own rounding floor under it, 64 eps max_i(|g_i| + |Qx|_i + |E'y|_i) (qp_polish, oracle and device);
    seed 9 id 243 (203 / 201 until then) ends with MAX_PENALTY_REACHED on both sides with it.
    Asserted: same return code, and on success the same solution and stationarity type (seed 1 id 542 passes the termination test two
    penalty updates later on the device, rho 10.24 against 2.56, at the same point)."""
    fz = _fuzz_module()
    oracle.lcqp_set_robust(1)
    rng = np.random.default_rng(seed)
    for k in range(max(ids) + 1):
        d = fz.make(rng)
        if k not in ids:
            continue
        ro = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0))
        rh = P.hip_solve(hip, d, hip.default_options(perturbStep=0))
        assert ro["ret"] == rh["ret"], (seed, k, ro["ret"], rh["ret"])
        if ro["ret"] == 0:
            assert np.abs(ro["x"] - rh["x"]).max() < 1e-6 * (1.0 + np.abs(ro["x"]).max()), (seed, k)
            assert ro["stats"]["status"] == rh["stats"]["status"], (seed, k)


@pytest.mark.parametrize("seed,k", [(2, 254), (17, 359), (27, 59), (29, 108)])
def test_fuzz_failing_homotopies_fail_on_both_sides(hip, oracle, seed, k):
    """The return-code differences of the 12 750 fuzz problems of round 6 (profiles/round6/fuzz/) that are NOT a success against a failure:
    MAX_PENALTY_REACHED (201) on one side, SUBPROBLEM_SOLVER_ERROR (203) on the other.  Both are the same event: a homotopy that has raised the
    penalty beyond 1e7, whose QPs are by then LP-like (|g| ~ rho |C x| ~ 1e7 ... 1e9 against curvatures of
    order one) and degenerate -- the damped polish cycles at a degenerate vertex for its 4 n + 32 trials on one side a penalty update or two
    before the other side reaches rho > 1e8.  The ORACLE differs from ITSELF in exactly this way when only its summation order changes
    (tools/oracle_selfcheck.py, profiles/round6/oracle_selfcheck_*.log: 5 such pairs in 13 200 problems, no other kind).  Asserted: both sides
    fail, both beyond rho = 1e6 after at least 50 iterates, neither reports a solution status; and the oracle against itself under the other
    summation order also ends in one of the two codes."""
    fz = _fuzz_module()
    oracle.lcqp_set_robust(1)
    rng = np.random.default_rng(seed)
    for i in range(k + 1):
        d = fz.make(rng)
    ro = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0))
    rh = P.hip_solve(hip, d, hip.default_options(perturbStep=0))
    oracle.qp_set_sum_order(0)
    try:
        rp = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0))
    finally:
        oracle.qp_set_sum_order(1)
    for r in (ro, rh, rp):
        assert r["ret"] in (201, 203), (seed, k, r["ret"])
        assert r["stats"]["rhoOpt"] >= 1e6 and r["stats"]["iterTotal"] >= 50 and r["stats"]["status"] == 0, (seed, k, r["stats"])


def test_fuzz_success_against_failure_is_the_stationarity_test_at_its_floor(hip, oracle):
    """The ONE problem of the 12 750 on which one side succeeds and the other fails: seed 8 id 46 (oracle SUCCESSFUL_RETURN after 27 iterates,
    device SUBPROBLEM_SOLVER_ERROR after ~140; profiles/round6/fuzz/case46_*.log).  The two homotopies agree iterate for iterate, to 3e-11 in x,
    through iterate 19, an inner loop at rho = 1.28 that converges slowly along the 19-dimensional null space of the Hessian: |stat| = 2.4e-9,
    4.7e-10, 3.4e-12 on the oracle, 5.6e-10, 2.3e-10 on the device at the same iterates -- the QP solutions differ by 1e-10 in flat directions
    (inside their residual tolerance) and stat = rho C p - r carries that difference times rho |C|.  The reference's test |stat| < 2.2e-10
    (src/LCQProblem.cpp:511, src/Options.cpp:298) passes on one side and misses by 5 % on the other; the side that passes raises the penalty one
    iterate earlier, and from there the two are different homotopies of a nonconvex problem: one finds a stationary point at rho = 5.12, the other
    climbs to rho > 1e5 where its LP-like QPs fail.  Asserted: exactly this -- the same path to 1e-8 while the penalty sequences agree, and at
    the iterate where they part both stationarity values within two decades of the tolerance, on opposite sides of it."""
    fz = _fuzz_module()
    oracle.lcqp_set_robust(1)
    rng = np.random.default_rng(8)
    for i in range(47):
        d = fz.make(rng)
    ev = np.linalg.eigvalsh(d["Q"])
    assert (ev < 1e-9 * ev.max()).sum() >= 10                                                # a large null space: QP solutions are loose along it
    ro = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0), trace=1200)
    rh = P.hip_solve(hip, d, hip.default_options(perturbStep=0, storeSteps=1), trace=True)
    so, sh, xo, xh = ro["trace_scalars"], rh["trace_scalars"], ro["trace_x"], rh["trace_x"]
    kk = min(len(so), len(sh))
    same_rho = so[:kk, 2] == sh[:kk, 2]
    split = int(np.argmin(same_rho)) if not same_rho.all() else kk       # first iterate with another penalty parameter
    if split == kk:
        assert ro["ret"] == rh["ret"]                                    # (the coin fell the same way on this box: nothing to explain)
        return
    assert split >= 2
    assert np.abs(xo[:split] - xh[:split]).max() < 1e-8 * (1.0 + np.abs(xo[:split]).max())
    stol = 1e6 * 2.221e-16
    a, b = so[split - 1, 0], sh[split - 1, 0]                            # |stat| at the iterate that decided: a penalty update on one side only
    assert min(a, b) < stol <= max(a, b), (a, b)
    assert max(a, b) < 100 * stol and min(a, b) > stol / 100.0, (a, b)
    assert 0 in (ro["ret"], rh["ret"])


@pytest.mark.parametrize("seed,k", [(11, 194), (24, 344), (33, 102)])
def test_fuzz_divergence_is_the_termination_test_at_its_rounding_floor(hip, oracle, seed, k):
    """The one problem of the five fuzz sets (1750 problems, profiles/round5/fuzz_*.log) on which HIP and the oracle still end at different
    stationary points: seed 11 id 194 (ids 34 and 277 of that seed did too until round 4 and agree since the subsolver holds its active rows to
    their rounding floor: test_fuzz_regressions_end_the_same_way).  Its iterates reach |x| ~ 1e2 ... 1e3 (objective -14939) along the 16-dimensional
    null space of its Hessian, and phi = phi_const + g_phi'x + 1/2 x'Cx (getPhi :1172-1185) is evaluated by both sides to eps |x|^2 |C| ~ 1e-12:
    the oracle reads -9.1e-13 at iterate 3 and ends, the device +9.0e-13 and goes on (profiles/round5/fuzz_diverge_11_194.log) -- the reference's
    own test `phi < 2.2e-13` applied to a number whose rounding error is four times the tolerance.  Root-caused in round 4 with
    `python tools/gpu.py fuzz_diverge 11 34 194 277` (profiles/round4/fuzz_diverge.log): the two
    homotopies agree iterate for iterate (to 1e-7) up to the iterate at which ONE side passes the termination test
    phi < complementarityTolerance = 2.2e-13 (src/LCQProblem.cpp:511-534) and the other does not.  At such an iterate the active side of
    every pair sits on its bound to the subsolver's residual tolerance (1e-12 relative, either sign), and with non-zero lbL / lbR -- all three
    problems have shifted bounds -- phi = phi_const + g_phi'x + 1/2 x'Cx (getPhi :1172-1185) is that residual times the O(1) ... O(100) value
    of the other side: a number of size 1e-12 and either sign, compared with 2.2e-13.  Which side of the tolerance it falls on is decided
    below the accuracy any QP solver is asked for: a coin flip of the reference's own test, like the step-length flip of DESIGN.md section 2.
    The side that continues takes a penalty update, and because all three Hessians are rank deficient (a face of QP minimisers) it settles
    on another point of that face.  Both ends are SUCCESSFUL_RETURN with the same stationarity type.  Asserted: exactly this mechanism."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpu_fuzz", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gpu_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    oracle.lcqp_set_robust(1)
    rng = np.random.default_rng(seed)
    ids = (k,)
    ctol = 1e3 * 2.221e-16
    for k in range(max(ids) + 1):
        d = fz.make(rng)
        if k not in ids:
            continue
        assert "lbL" in d and (np.any(d["lbL"]) or np.any(d["lbR"]))                        # shifted complementarity bounds
        ev = np.linalg.eigvalsh(d["Q"])
        if seed == 11:
            assert ev.min() < 1e-9 * ev.max()                                               # rank-deficient Hessian: a face of minimisers
        ro = P.oracle_solve(oracle, d, oracle.default_options(perturbStep=0), trace=1000)
        rh = P.hip_solve(hip, d, hip.default_options(perturbStep=0, storeSteps=1), trace=True)
        assert ro["ret"] == rh["ret"] == 0 and ro["stats"]["status"] == rh["stats"]["status"]
        so, sh, xo, xh = ro["trace_scalars"], rh["trace_scalars"], ro["trace_x"], rh["trace_x"]
        kk = min(len(so), len(sh))
        assert np.abs(xo[:kk] - xh[:kk]).max() < 1e-7 * (1.0 + np.abs(xo[:kk]).max())      # the same path while both run
        assert np.array_equal(so[:kk, 2], sh[:kk, 2])                                       # the same penalty parameter at every common iterate
        if len(so) != len(sh):
            short, long_ = (so, sh) if len(so) < len(sh) else (sh, so)
            last = len(short) - 1
            # the side that stopped passed both termination tests at its last iterate; the other side failed the complementarity test there by
            # an amount of the size of the subsolver's residual tolerance (resTol = 1e-12, relative to the terms phi is made of)
            assert short[last, 0] < 1e6 * 2.221e-16 and short[last, 1] < ctol
            assert long_[last, 0] < 1e6 * 2.221e-16 and long_[last, 1] >= ctol
            Lx = d["L"] @ xo[last]; Rx = d["R"] @ xo[last]
            terms = max(1.0, float(np.abs(d["lbL"] * d["lbR"]).sum()), float(np.abs(Lx * Rx).sum() + np.abs(Lx * d["lbR"]).sum() + np.abs(Rx * d["lbL"]).sum()))
            assert abs(long_[last, 1] - short[last, 1]) < 1e-11 * terms


@pytest.mark.parametrize("kw", [
    dict(solveZeroPenaltyFirst=0),                              # first QP already carries the penalty (src/LCQProblem.cpp:452-467)
    dict(nDynamicPenalty=0),                                    # no Leyffer test (:1275-1313)
    dict(nDynamicPenalty=1, etaDynamicPenalty=0.5),
    dict(nDynamicPenalty=12, etaDynamicPenalty=0.95),            # a window longer than the 8 of round 1
    dict(initialPenaltyParameter=1.0, penaltyUpdateFactor=10.0),
    dict(maxIterations=7),                                      # MAX_ITERATIONS_REACHED (:536-539)
    dict(maxPenaltyParameter=0.05),                             # MAX_PENALTY_REACHED (:541-543)
    dict(stationarityTolerance=1e-6, complementarityTolerance=1e-9),
    dict(perturbStep=1, perturbSeed=12345),
])
def test_lcqp_option_sweep(hip, oracle, kw):
    """every algorithm option of src/Options.cpp:296-333 that changes the control flow of runSolver, HIP batch vs oracle:
    same return code, same iterate counts (up to one inner cycle), same solution"""
    base = dict(perturbStep=0)
    base.update(kw)
    probs = [oracle.synth_generate(i, 64, 96, 16) for i in range(3)] + [P.circle(20), P.warm_up_binary()]
    for d in probs:
        d = dict(d)
        d.setdefault("nV", d["g"].size)
        d.setdefault("nComp", d["L"].shape[0] if d["L"].ndim == 2 else d["L"].size // d["nV"])
        d.setdefault("nC", 0 if d.get("A") is None else d["A"].size // d["nV"])
        ro = P.oracle_solve(oracle, d, oracle.default_options(**base))
        rh = P.hip_solve(hip, d, hip.default_options(**base))
        assert rh["ret"] == ro["ret"], (kw, rh["ret"], ro["ret"])
        so, sh = ro["stats"], rh["stats"]
        # one inner cycle more or less; a long Leyffer window compares more near-zero complementarity values
        slack = 4 * max(1, base.get("nDynamicPenalty", 3) // 3)
        assert abs(so["iterTotal"] - sh["iterTotal"]) <= slack and abs(so["iterOuter"] - sh["iterOuter"]) <= 1, (kw, so, sh)
        if ro["ret"] == 0:
            assert np.abs(ro["x"] - rh["x"]).max() < 1e-7, kw
            assert so["status"] == sh["status"]


def test_dense_problems_between_1024_and_4096_variables(hip, oracle):
    """Round 4 lifts the dense limit from nV = 1024 to 2048 (an np = 2048 instantiation: 96 KiB of LDS, one workgroup per CU, one row in flight
    per wave -- meant for single large problems).  (a) a random strictly convex QP with nV = 1300 through SubsolverHIP: the oracle's solution,
    KKT residuals; (b) the circle example at N = 700 (nV = 1402, nC = 701, nComp = 700) as a batch of one: the optimum the reference prints
    (examples/OptimizeOnCircle.cpp:144), complementarity, stationarity of the returned duals."""
    rng = np.random.default_rng(2048)
    n, m = 1300, 300
    Mx = rng.standard_normal((n, n)) / np.sqrt(n); Q = Mx.T @ Mx + np.eye(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n); xs = rng.standard_normal(n)
    lbA = A @ xs - rng.uniform(0.05, 0.5, m); ubA = A @ xs + rng.uniform(0.05, 0.5, m); g = rng.standard_normal(n)
    qh = hip.SubsolverHIP(n, m, Q, A)
    ret, it, flag = qh.solve(True, g, lbA, ubA, np.zeros(n))
    assert ret == 0 and flag == 0
    x, y = qh.getSolution()
    qh.close()
    res = P.kkt_residuals(Q, g, A, lbA, ubA, np.full(n, -np.inf), np.full(n, np.inf), x, y)
    assert max(res) < 1e-8, res
    qo = oracle.QP(Q, A); ro = qo.solve(True, g, lbA, ubA, np.zeros(n)); xo, yo = qo.solution()
    assert ro[0] == 0 and np.abs(x - xo).max() < X_TOL and np.abs(y - yo).max() < Y_TOL
    # (c) nV = 2500 on the np = 4096 instantiation (128 KiB of LDS: the four waves combine their partial sums in two copies instead of four)
    n, m = 2500, 200
    Mx = rng.standard_normal((n, n)) / np.sqrt(n); Q = Mx.T @ Mx + np.eye(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n); xs = rng.standard_normal(n)
    lbA = A @ xs - rng.uniform(0.05, 0.5, m); ubA = A @ xs + rng.uniform(0.05, 0.5, m); g = rng.standard_normal(n)
    qh = hip.SubsolverHIP(n, m, Q, A)
    ret, it, flag = qh.solve(True, g, lbA, ubA, np.zeros(n))
    assert ret == 0 and flag == 0
    x, y = qh.getSolution()
    qh.close()
    res = P.kkt_residuals(Q, g, A, lbA, ubA, np.full(n, -np.inf), np.full(n, np.inf), x, y)
    assert max(res) < 1e-8, res
    qo = oracle.QP(Q, A); ro = qo.solve(True, g, lbA, ubA, np.zeros(n)); xo, yo = qo.solution()
    assert ro[0] == 0 and np.abs(x - xo).max() < X_TOL and np.abs(y - yo).max() < Y_TOL
    d = P.circle(700)
    assert d["nV"] == 1402
    rh = P.hip_solve(hip, d, hip.default_options(perturbStep=0))
    # (the optimum moves with the discretisation: (0.1811, -0.9835) is what the reference prints for N = 100, a polygon with 700 corners gives
    #  (0.1798, -0.9837); both lie on the unit circle next to the unconstrained minimiser's direction)
    assert rh["ret"] == 0 and np.abs(rh["x"][:2] - [0.1811, -0.9835]).max() < 3e-3 and abs(np.hypot(*rh["x"][:2]) - 1.0) < 1e-3
    xx, yy, nV, nC, nK = rh["x"], rh["y"], d["nV"], d["nC"], d["nComp"]
    assert abs((d["L"] @ xx) @ (d["R"] @ xx)) < 1e3 * 2.221e-16
    stat = d["Q"] @ xx + d["g"] - d["A"].T @ yy[nV:nV + nC] - d["L"].T @ yy[nV + nC:nV + nC + nK] - d["R"].T @ yy[nV + nC + nK:] - yy[:nV]
    assert np.abs(stat).max() < 1e-7


def test_subsolver_active_row_capacity(hip, oracle):
    """more candidate active rows than the subsolver has room for (LCQP_MAX_ACTIVE = 896: the active-row triangular solves live in
    the LDS arena): 1000 copies of the row x_0 >= 1 at nV = 500.  The polish must give up cleanly, as the oracle does, instead of
    running past the arena; ADMM alone cannot verify a KKT point, so both sides report the same failure."""
    n, m = 500, 1000
    Q = np.eye(n); A = np.zeros((m, n)); A[:, 0] = 1.0
    g = np.zeros(n); lbA = np.ones(m); ubA = np.full(m, np.inf)
    opt_h = hip.default_options(maxRounds=4); opt_o = oracle.default_options(maxRounds=4)
    qh = hip.SubsolverHIP(n, m, Q, A, opt=opt_h); qo = oracle.QP(Q, A, opt_o)
    rh = qh.solve(True, g, lbA, ubA, np.zeros(n)); ro = qo.solve(True, g, lbA, ubA, np.zeros(n))
    assert (rh[0], rh[2]) == (ro[0], ro[2]), (rh, ro)
    assert rh[0] in (0, 203)
    qh.close()
    # the same rows within the capacity: solved, x_0 = 1
    m2 = 800
    qh = hip.SubsolverHIP(n, m2, Q, A[:m2]); qo = oracle.QP(Q, A[:m2])
    rh = qh.solve(True, g, lbA[:m2], ubA[:m2], np.zeros(n)); ro = qo.solve(True, g, lbA[:m2], ubA[:m2], np.zeros(n))
    assert (rh[0], rh[2]) == (ro[0], ro[2]) == (0, 0)
    x, y = qh.getSolution()
    assert abs(x[0] - 1.0) < 1e-9 and np.abs(x[1:]).max() < 1e-12 and abs(y[n:].sum() - 1.0) < 1e-8
    qh.close()


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_lcqp_objective_scaling(hip, oracle, scale):
    """scaling the objective (Q, g) together with the penalty parameters and the stationarity tolerance by a constant is the same
    homotopy in other units: same iterates, same solution, duals scaled.  It holds because the subsolver's own tolerances are
    relative to max|Q_ii| and |g| (the complementarity tolerance acts on x and stays)."""
    kw = dict(perturbStep=0, initialPenaltyParameter=0.01 * scale, maxPenaltyParameter=1e8 * scale, stationarityTolerance=1e6 * 2.221e-16 * scale)
    for d in [oracle.synth_generate(i, 64, 96, 16) for i in range(3)] + [P.circle(20)]:
        d = dict(d)
        base = P.hip_solve(hip, d, hip.default_options(perturbStep=0))
        ds = dict(d); ds["Q"] = scale * d["Q"]; ds["g"] = scale * d["g"]
        rs = P.hip_solve(hip, ds, hip.default_options(**kw))
        ro = P.oracle_solve(oracle, ds, oracle.default_options(**kw))
        assert base["ret"] == rs["ret"] == ro["ret"] == 0
        assert np.abs(rs["x"] - ro["x"]).max() < 1e-7
        assert np.abs(rs["x"] - base["x"]).max() < 1e-6 * (1 + np.abs(base["x"]).max())
        assert abs(rs["stats"]["iterTotal"] - base["stats"]["iterTotal"]) <= 4 and abs(rs["stats"]["rhoOpt"] / scale - base["stats"]["rhoOpt"]) < 1e-9
        n = d["nV"]
        assert np.abs(rs["y"][n:] / scale - base["y"][n:]).max() < 1e-5 * (1 + np.abs(base["y"]).max())


def test_lcqp_constraint_row_scaling(hip, oracle):
    """scaling rows of A together with their bounds by positive factors (0.01 ... 100) describes the same feasible set: same
    solution, row duals divided by the factors"""
    rng = np.random.default_rng(11)
    for d in [oracle.synth_generate(i, 64, 96, 16) for i in range(3)]:
        base = P.hip_solve(hip, d, hip.default_options(perturbStep=0))
        f = 10.0 ** rng.uniform(-2, 2, d["nC"])
        ds = dict(d); ds["A"] = d["A"] * f[:, None]; ds["lbA"] = d["lbA"] * f; ds["ubA"] = d["ubA"] * f
        rs = P.hip_solve(hip, ds, hip.default_options(perturbStep=0))
        ro = P.oracle_solve(oracle, ds, oracle.default_options(perturbStep=0))
        assert base["ret"] == rs["ret"] == ro["ret"] == 0
        assert np.abs(rs["x"] - ro["x"]).max() < 1e-7
        assert np.abs(rs["x"] - base["x"]).max() < 1e-6 * (1 + np.abs(base["x"]).max())
        n, nC = d["nV"], d["nC"]
        assert np.abs(rs["y"][n:n + nC] * f - base["y"][n:n + nC]).max() < 1e-5 * (1 + np.abs(base["y"]).max())
