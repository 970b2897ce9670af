// lcqp_sparse_solver.hpp -- the algorithm of the sparse arm, per instance: third layer of the sparse kernel unit (lcqp_sparse.hip has the
// map), the counterpart of lcqp_dev.hpp.
//
// Owns: the sparse products of an instance (sp_Ex, sp_Qx2, sp_ETy, sp_residual, sp_Cx2, sp_C_from_Ex, sp_maxabs), the ADMM iterations
// (sp_admm), the polish and the homotopy as phase routines (sp_polish_*, sp_ph_*, sp_qp_begin, sp_finish: each returns the phase the
// instance enters next), and the two pieces of the setup the kernels share (sp_prepare_vectors, sp_admm_factor).  Who runs a phase for
// which instance, and when, is the scheduler's business (lcqp_sparse.hip).
// May include: lcqp_sparse_factor.hpp (and through it the lane layer).  Device code only, in the anonymous namespace.
#pragma once
#include "lcqp_sparse_factor.hpp"

#include <cstring>

namespace {

// ---- the sparse products of an instance: sp_ell (lcqp_sparse_lane.hpp) over the slabs of Q, E and E' ------------------------------------
struct NoPre { };

template <int G> __device__ __forceinline__ void sp_Ex(SpCtx<G>& c, GD x, GD out)
{
    SPROF(c, SP_VECTORS);
    sp_ell<G, false>(c.db->ellE, c.gl, c.Ex(), [&](int j) { return D2{x[j], 0.0}; }, [](int) { return NoPre{}; }, [&](int r, double s, double, NoPre) { out[r] = s; });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
// two vectors through one pass over Q: o0 = Q x0, o1 = Q x1
template <int G> __device__ __forceinline__ void sp_Qx2(SpCtx<G>& c, GD x0, GD x1, GD o0, GD o1)
{
    SPROF(c, SP_VECTORS);
    sp_ell<G, false>(c.db->ellQ, c.gl, c.Qx(), [&](int j) { return D2{x0[j], x1[j]}; }, [](int) { return NoPre{}; },
              [&](int i, double s0, double s1, NoPre) { o0[i] = s0; o1[i] = s1; });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
// out[i] = base(pre(i)) - (E'y)[i]   (column gather over the CSC of E); returns max |out| over the group
template <int G, class Pre, class Base> __device__ __forceinline__ double sp_ETy(SpCtx<G>& c, GD y, GD out, Pre pre, Base base)
{
    SPROF(c, SP_VECTORS);
    double mx = 0.0;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(), [&](int r) { return D2{y[r], 0.0}; }, pre,
              [&](int i, double s, double, typename val_of<decltype(pre(0))>::type pv) { const double v = base(pv) - s; out[i] = v; mx = nmax(mx, fabs(v)); });
    g_sync();
    SPROF(c, SP_PRODUCTS);
    return g_max<G>(mx);
}
// the residual of the stationarity condition in one pass over Q and E' (both indexed by the variable):
// r1[i] = (-g[i] - (Q x)[i]) - (E'y)[i]; returns max |r1|
// r1 = -g - Q x - E'y; returns |r1|_inf and, in `scale`, max_i(|g_i| + |Q x|_i + |E'y|_i): the residual's own rounding floor is 64 eps of that (round 6, as on
// the dense path: qp_polish in lcqp_dev.hpp)
template <int G> __device__ __forceinline__ double sp_residual(SpCtx<G>& c, GD g, GD x, GD y, GD r1, GD qx, double& scale)
{
    SPROF(c, SP_VECTORS);
    sp_ell<G, false>(c.db->ellQ, c.gl, c.Qx(), [&](int j) { return D2{x[j], 0.0}; }, [](int) { return NoPre{}; }, [&](int i, double s, double, NoPre) { qx[i] = s; });
    g_sync();
    double mx = 0.0, sc = 0.0;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(), [&](int r) { return D2{y[r], 0.0}; }, [&](int i) { return D2{g[i], qx[i]}; },
              [&](int i, double s, double, D2 pv) { const double v = (-pv.a - pv.b) - s; r1[i] = v; mx = nmax(mx, fabs(v)); sc = fmax(sc, fabs(pv.a) + fabs(pv.b) + fabs(s)); });
    g_sync();
    SPROF(c, SP_PRODUCTS);
    scale = g_max<G>(sc);
    return g_max<G>(mx);
}
// C v = L'(R v) + R'(L v) for two vectors: lx = E v (rows of L: nC .. nC+nComp, of R: nC+nComp ..), then a column gather with
// swapped coefficients
template <int G> __device__ __forceinline__ void sp_Cx2(SpCtx<G>& c, GD v0, GD v1, GD o0, GD o1)
{
    SPROF(c, SP_VECTORS);
    GD lx0 = c.M(MV_LX), lx1 = c.M(MV_LX2);
    sp_ell<G, false>(c.db->ellE, c.gl, c.Ex(), [&](int j) { return D2{v0[j], v1[j]}; }, [](int) { return NoPre{}; },
              [&](int r, double s0, double s1, NoPre) { lx0[r] = s0; lx1[r] = s1; });
    g_sync();
    const int nC = c.db->nC, nK = c.db->nComp;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(),
              [&](int r) { const int rr = r >= nC + nK ? r - nK : (r >= nC ? r + nK : -1);      // R'(L v) + L'(R v)
                           return rr >= 0 ? D2{lx0[rr], lx1[rr]} : D2{0.0, 0.0}; },
              [](int) { return NoPre{}; }, [&](int i, double s0, double s1, NoPre) { o0[i] = s0; o1[i] = s1; });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
// C v from lx = E v that somebody else has computed (the polish leaves E x of its solution), for one vector or two:
// out(i, (C v0)[i], (C v1)[i], pre(i))
template <int G, bool TWO, class Pre, class Out> __device__ __forceinline__ void sp_C_from_Ex(SpCtx<G>& c, GD lx0, GD lx1, Pre pre, Out out)
{
    SPROF(c, SP_VECTORS);
    const int nC = c.db->nC, nK = c.db->nComp;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(),
              [&](int r) { const int rr = r >= nC + nK ? r - nK : (r >= nC ? r + nK : -1);
                           return rr >= 0 ? D2{lx0[rr], TWO ? (double)lx1[rr] : 0.0} : D2{0.0, 0.0}; },
              pre, [&](int i, double s0, double s1, typename val_of<decltype(pre(0))>::type pv) { out(i, s0, s1, pv); });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
template <int G> __device__ __forceinline__ double sp_maxabs(const SpCtx<G>& c, GD a, int n)
{
    double s = 0.0;
    const int gl = here(c.gl);
#pragma unroll 8
    for (int i = gl; i < n; i += G) s = fmax(s, fabs(a[i]));
    return g_max<G>(s);
}

// ---- ADMM iterations (OSQP, KKT form; oracle: sqp_admm) ----------------------------------------------------------------------
template <int G>
__device__ __forceinline__ void sp_admm(SpCtx<G>& c, GD g, int n_it)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    const double alpha = db.opt.admmAlpha, sigma = c.info->sigma;
    GD xa = c.V(NV_XA), ya = c.M(MV_YA), za = c.M(MV_ZA), b = c.Nv();
    GD l = c.M(MV_L), u = c.M(MV_U), rhov = c.M(MV_RHOV);
    for (int it = 0; it < n_it; it++) {
        for (int i = t; i < n; i += G) b[db.iperm[i]] = sigma * xa[i] - g[i];
        for (int r = t; r < m; r += G) b[db.iperm[n + r]] = za[r] - ya[r] / rhov[r];
        g_sync();
        sp_solve<G>(c, true, b);
        for (int r = t; r < m; r += G) {
            const double rv = rhov[r];
            const double zt = za[r] + (b[db.iperm[n + r]] - ya[r]) / rv;
            const double zr = alpha * zt + (1.0 - alpha) * za[r];
            if (isinf(l[r]) && isinf(u[r])) { za[r] = zr; ya[r] = 0.0; continue; }
            const double zn = fmin(fmax(zr + ya[r] / rv, l[r]), u[r]);
            ya[r] += rv * (zr - zn);
            za[r] = zn;
        }
        for (int i = t; i < n; i += G) xa[i] = alpha * b[db.iperm[i]] + (1.0 - alpha) * xa[i];
        g_sync();
        c.cAdmm++;
    }
}

// ---- the phases of an instance's homotopy (k_sparse_sched runs them) -----------------------------------------------------------------------
// Every routine below is called by the G lanes of one instance with that instance's context and state record (all values uniform inside the
// group) and returns the phase the instance enters next (PH_NUM: finished).  Together they are runSolver (src/LCQProblem.cpp:444-560), the
// subsolver call (oracle: sqp_solve) and the polish (oracle: sqp_polish) of round 3, cut at the points where instances of one wavefront used
// to part: before a trial, before a factorisation, before a correction, at the end of a QP.
struct StRow { int s; double e, lo, hi, y; };
struct I2 { int a, b; };
struct I2D { int a, b; double y; };
struct ID4 { int p, s; double lo, hi, e; };
struct ID2 { int s; double v, y; };
struct ID3 { int s; double lo, hi, z, y; };

// the polish starts (oracle: sqp_polish, entry): tolerances scale with 1 + |g|_inf
template <int G>
__device__ __forceinline__ int sp_polish_begin(SpCtx<G>& c, SpState& S, GD g, int reuse)
{
    const lcqp_options_t& o = c.db->opt;
    S.gs = 1.0 + ((reuse && S.gmaxNext >= 0.0) ? S.gmaxNext : sp_maxabs<G>(c, g, c.db->n));      // (the LCQP level knows max|g| of the vector it has just formed)
    S.ytol = o.feasTol * S.gs;
    S.fact_valid = 0; S.borderTodo = 0;
    // (S.dpUsed / S.d2Used stay: they are the regularisation of the factorisation IN MEMORY, written by sp_ph_factor.  A hot start whose
    // working set matches the factor's corrects with that factor, whichever of the two levels it holds.)
    S.trial = 0; S.reuse = reuse; S.nrefine = 0; S.xinf = 0.0;
    return PH_TRIAL;
}

// the instance is finished: statistics and solution go out
template <int G>
__device__ __forceinline__ int sp_finish(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl), n = db.n, m = db.m;
    GD xk = c.V(NV_XK), yk = c.M(MV_YK);
    S.st.status = S.algoStat; S.st.returnValue = S.rc;
    S.st.admmIter = c.cAdmm; S.st.trials = c.cTrials; S.st.factorizations = c.cFact; S.st.corrections = c.cCorr; S.st.reserved = c.cSweeps;
    for (int i = t; i < n; i += G) db.xout[(size_t)c.b * n + i] = xk[i];
    for (int r = t; r < m; r += G) db.yout[(size_t)c.b * m + r] = yk[r];
    if (t == 0) { db.stats[c.b] = S.st; c.info->bytes += c.bytes; }
    c.bytes = 0.0;
    return PH_NUM;
}

// a polish that did not settle (oracle: the tail of the round loop of sqp_solve): twice as many ADMM iterations, or the QP has failed
template <int G>
__device__ __forceinline__ int sp_polish_failed(SpCtx<G>& c, SpState& S)
{
    const lcqp_options_t& o = c.db->opt;
    S.n_admm = 2 * S.n_admm;
    if (S.n_admm < 10) S.n_admm = 10;
    if (S.n_admm > 400) S.n_admm = 400;
    S.round++;
    if (S.round < o.maxRounds) return PH_ROUND;
    S.qpIter = (c.cTrials - S.trials0) + (c.cAdmm - S.admm0);
    S.st.subproblemIter += S.qpIter; S.st.qpSolverExitFlag = 1; S.st.qpSolves++;
    S.rc = LCQP_SUBPROBLEM_SOLVER_ERROR;
    return sp_finish<G>(c, S);
}

// PH_TRIAL: the head of one trial of the polish -- E x, the status test, the true residual when the working set did not change, acceptance;
// else the leaving rows, and whether the factorisation still matches the working set
template <int G>
__device__ __forceinline__ int sp_ph_trial(SpCtx<G>& c, SpState& S, GD g)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n, m = db.m, trial = S.trial;
    GD x = c.V(NV_XT), r1 = c.V(NV_R1), qx = c.V(NV_TMP), yt = c.M(MV_YT), ex = c.M(MV_EX);
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI st = c.I(MI_STT), stf = c.I(MI_STF), newst = c.I(MI_NEW);
    const double gs = S.gs, ytol = S.ytol;
    c.cTrials++;
    // Two stages, as on the dense path (oracle: sqp_polish).  Stage 1 is what every trial needs: E x, for the status test.  Stage 2 -- the
    // true residual, one pass over Q and one over E' -- runs only when stage 1 changed nothing: after a correction the residual is zero on
    // the old working set up to rounding and regularisation, so when the set changes the next right-hand side is known without it (the
    // multipliers of the leaving rows, below); the trial that accepts always has the true residual.
    double res_stat = 0.0;
    int have_r1 = 0;
    double res_eq = 0.0, bmax = 0.0;
    int chg = 0, act = 0, loose = 0;
    // active rows are held to the rounding floor of a computed E_r x, 16 eps (|b_r| + |E_r|_1 |x|_inf), before a point is accepted (round 5;
    // oracle: sqp_polish; dense twin: qp_polish in lcqp_dev.hpp): runSolver ends on phi < 1e3 eps, a sum of products of such residuals
    const double exScale = c.info->e1max * S.xinf;
    auto status = [&](int r, StRow v) {
        int ns = v.s;
        if (v.s == ST_INACT) {
            const double ftol = o.feasTol * (1.0 + fabs(v.e));
            if (v.e < v.lo - ftol) ns = ST_LOWER;
            else if (v.e > v.hi + ftol) ns = ST_UPPER;
        } else {
            const double bb = (v.s == ST_UPPER) ? v.hi : v.lo;
            const bool above = !(fabs(bb - v.e) <= 16.0 * 2.221e-16 * (fabs(bb) + exScale));      // (a NaN counts) a row at the rounding floor of its computed E_r x is not a residual (round 6)
            if (above) res_eq = nmax(res_eq, fabs(bb - v.e));
            bmax = fmax(bmax, fabs(bb));
            loose |= above;
            if (v.s == ST_LOWER && v.y > ytol) ns = ST_INACT;
            if (v.s == ST_UPPER && v.y < -ytol) ns = ST_INACT;
        }
        newst[r] = ns;
        chg += (ns != v.s);
        act += (ns != ST_INACT);
    };
    if (trial == 0 && S.reuse) {
        // hot start with an unchanged (x, y): r1 = r1_last + (g_last - g) and E x are in place -- the residual and E x of the accepted
        // trial stay where they are, and the LCQP level adds (g_last - g) to r1 in the pass that forms the new g (sp_ph_qpend)
        have_r1 = 1;
        g_map<G, 4>(m, t, [&](int r) { return StRow{st[r], ex[r], l[r], u[r], yt[r]}; }, status);
    } else {
        // E x and the status test in ONE pass (round 5): the row's state rides along as the product's `pre`, the sum goes straight into the
        // test and into ex (the right-hand side of the correction needs it) -- no second pass over st, ex, l, u, y
        SPROF(c, SP_VECTORS);
        sp_ell<G, false>(db.ellE, c.gl, c.Ex(), [&](int j) { return D2{x[j], 0.0}; },
                  [&](int r) { return StRow{st[r], 0.0, l[r], u[r], yt[r]}; },
                  [&](int r, double s0, double, StRow v) { ex[r] = s0; v.e = s0; status(r, v); });
        g_sync();
        SPROF(c, SP_PRODUCTS);
        c.bytes += db.by[BY_EX];
    }
    const int changed = g_sum_i<G>(chg), nact = g_sum_i<G>(act);
    res_eq = g_max<G>(res_eq);
    bmax = g_max<G>(bmax);
    SPROF(c, SP_ASSEMBLE);      // (profile builds: the status test on its own)
    double rscale = 0.0;
    if (!have_r1 && (trial == 0 || !changed)) {
        res_stat = sp_residual<G>(c, g, x, yt, r1, qx, rscale);
        c.cSweeps++;
        c.bytes += db.by[BY_SWEEP];
        have_r1 = 1;
    }
    if (trial > 0 && !changed && res_stat <= fmax(o.resTol * gs, 64.0 * 2.221e-16 * rscale) && res_eq <= o.resTol * (1.0 + bmax)) {
        if (!(g_any<G>(loose) && S.nrefine < 2 && trial + 1 < o.maxTrials)) return PH_QPEND;      // a verified KKT point
        S.nrefine++;      // ... whose active rows can be held more exactly: one more correction
    }
    if (changed && trial > 0) {
        if (trial >= 2 && nact > n && changed > max(n / 2, 32)) return sp_polish_failed<G>(c, S);       // overshooting cold start: hand over to ADMM
        // leaving rows: their multipliers leave the residual (r1 += E_r' y_r), then the new working set takes over
        GD ytmp = c.M(MV_LX);
        g_sync();
        g_map<G, 8>(m, t, [&](int r) { return I2D{newst[r], st[r], yt[r]}; },
                    [&](int r, I2D v) { const bool leaves = (v.a == ST_INACT && v.b != ST_INACT); ytmp[r] = leaves ? -v.y : 0.0; st[r] = v.a; if (leaves && v.y != 0.0) yt[r] = 0.0; });
        g_sync();
        // r1 - E'(-y_leaving) = r1 + E'y_leaving; without a true residual r1 is the predicted one: nothing was left on the old working set
        if (have_r1) sp_ETy<G>(c, ytmp, r1, [&](int i) { return r1[i]; }, [](double v) { return v; });
        else sp_ETy<G>(c, ytmp, r1, [](int) { return NoPre{}; }, [](NoPre) { return 0.0; });
        S.fact_valid = 0;
    }
    if (!S.fact_valid) {
        int diff = (c.info->stfValid == 0);
#pragma unroll 8
        for (int r = t; r < m; r += G) diff |= ((stf[r] != ST_INACT) != (st[r] != ST_INACT));
        if (g_any<G>(diff)) return PH_FACTOR;
        S.fact_valid = 1;
    }
    return PH_CORRECT;
}

// PH_FACTOR: the band LDL' of [Q + delta I, Ea'; Ea, -delta2 I] for the working set in MI_STT
template <int G>
__device__ __forceinline__ int sp_ph_factor(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    GI st = c.I(MI_STT), stf = c.I(MI_STF);
    // Two levels of regularisation, as on the dense path (proxSmall / proxBig).  A correction with the safe level leaves
    // delta dx and delta2 dy (1e-8, 1e-9 relative) in the true residuals: every QP paid one refinement trial -- a sweep, a band
    // solve, the vector passes -- for the regularisation alone.  The light level (1e-12, 1e-14) is accepted at once.  The band
    // LDL' is not pivoted, so the light level needs an ordering in which every row follows one of its variables (lightOK, chosen
    // by the host when every Hessian of the batch is safely definite) and is only kept when every pivot has the sign its node
    // prescribes and a safe size; a variable's pivot failing makes the safe level permanent for the instance.
    int level = (db.lightOK && !c.info->bigReg) ? 0 : 1;
    // the working set as a bit set in LDS: the factorisation asks for the membership of the row behind every entry of E it meets (up to
    // 2 w per band row) -- from memory these were gathers of 4-byte flags, 8 instances apart in one wavefront
    unsigned* bits = nullptr;
    if (G <= 16 && db.bitWords > 0) {
        bits = reinterpret_cast<unsigned*>(sp_dyn_lds) + (size_t)((int)threadIdx.x / G) * db.bitWords;
        for (int w = t; w < db.bitWords; w += G) {
            unsigned word = 0u;
#pragma unroll 8
            for (int k = 0; k < 32; k++) { const int r = w * 32 + k; if (r < m && st[r] != ST_INACT) word |= 1u << k; }
            bits[w] = word;
        }
        wave_sync();
    }
    for (;;) {
        S.dpUsed = level ? c.info->delta : c.info->deltaS;
        S.d2Used = level ? c.info->delta2 : c.info->delta2S;
        const double d2 = S.d2Used;
        if (bits) sp_factor_band<G>(c, c.KF(false), c.KD(false), S.dpUsed, [=](int) { return d2; }, [=](int r) { return ((bits[r >> 5] >> (r & 31)) & 1u) != 0u; });
        else sp_factor_band<G>(c, c.KF(false), c.KD(false), S.dpUsed, [=](int) { return d2; }, [=](int r) { return st[r] != ST_INACT; });
        if (level == 1) break;
        int badVar = 0, badRow = 0;
        GD Kd = c.KD(false);
        const double sc = c.info->scale, vmax = 1.0 / (1e-8 * sc), rmax = sc / 1e-8;
        const int Nb = db.N - db.kb;
#pragma unroll 4
        for (int p = t; p < Nb; p += G) {
            const double kd = Kd[p];            // 1 / D
            const int node = db.pnode[p];
            if (node < n) badVar |= !(kd > 0.0 && kd < vmax);
            else if (st[node - n] != ST_INACT) badRow |= !(kd < 0.0 && kd > -rmax);
        }
        const bool bv = g_any<G>(badVar), br = g_any<G>(badRow);
        if (!bv && !br) break;
        if (bv && t == 0) c.info->bigReg = 1;
        level = 1;
    }
    if (db.kb > 0) { sp_border_prepare<G>(c, false, [=](int r) { return st[r] != ST_INACT; }); S.borderTodo = db.kb; }
    g_map<G, 8>(m, t, [&](int r) { return st[r]; }, [&](int r, int v) { stf[r] = v; });
    if (t == 0) c.info->stfValid = 1;
    g_sync();
    S.fact_valid = 1;
    return PH_CORRECT;
}

// PH_CORRECT: [Q + delta I, Ea'; Ea, -delta2 I][dx; dy] = [r1; ba - Ea x], x += dx, y += dy; then the next trial (or the polish has run out of trials)
template <int G>
__device__ __forceinline__ int sp_ph_correct(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    GD x = c.V(NV_XT), r1 = c.V(NV_R1), yt = c.M(MV_YT), ex = c.M(MV_EX), b = c.Nv();
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI st = c.I(MI_STT);
    const int* iperm = db.iperm;
    SPROF(c, SP_VECTORS);
    // (deep tiles: the band's lane groups are 8 lanes wide, a pass over n is n / (8 U) round trips)
    g_map<G, 16>(n, t, [&](int i) { return ID{iperm[i], r1[i]}; }, [&](int, ID v) { b[v.i] = v.a; });
    g_map<G, 6>(m, t, [&](int r) { return ID4{iperm[n + r], st[r], l[r], u[r], ex[r]}; },
                [&](int, ID4 v) { b[v.p] = (v.s != ST_INACT) ? ((v.s == ST_UPPER) ? v.hi : v.lo) - v.e : 0.0; });
    g_sync();
    SPROF(c, SP_RHS);
    // one call site of the band solve: first the columns of W = U inv(Bd) a fresh factorisation owes (none for a plain band), then b
    const int borderTodo = S.borderTodo;
    for (int jb = 0; jb <= borderTodo; jb++) {
        GD vec = b;
        if (jb < borderTodo) vec = sp_border_column<G>(c, false, jb);
        else if (borderTodo > 0) { const double d2 = S.d2Used; sp_border_schur<G>(c, false, S.dpUsed, [=](int) { return d2; }, [=](int r) { return st[r] != ST_INACT; }); }
        sp_solve_band<G>(c, false, vec);
    }
    S.borderTodo = 0;
    if (db.kb > 0) sp_border_solve<G>(c, false, b);
    double xm = 0.0;
    g_map<G, 12>(n, t, [&](int i) { return D2{b[iperm[i]], x[i]}; }, [&](int i, D2 v) { const double xn = v.b + v.a; x[i] = xn; xm = fmax(xm, fabs(xn)); });
    S.xinf = g_max<G>(xm);
    g_map<G, 10>(m, t, [&](int r) { return ID2{st[r], b[iperm[n + r]], yt[r]}; }, [&](int r, ID2 v) { if (v.s != ST_INACT) yt[r] = v.y + v.v; });
    g_sync();
    c.cCorr++;
    S.trial++;
    if (S.trial >= c.db->opt.maxTrials) return sp_polish_failed<G>(c, S);
    return PH_TRIAL;
}

// the subsolver call starts (oracle: sqp_solve, entry): SubsolverBase::solve on the OSQP arm.  A hot start from the stored solution goes
// straight to the polish; everything else takes the round preamble (PH_ROUND).
// warmFirst (sp_ph_start of a warm re-solve, k_sparse_refresh): the first QP of the homotopy is a hot start on the stored point and working
// set -- but the stored residual and E x belong to the g and the bounds of the run before, so the polish takes its cold entry there.
template <int G>
__device__ __forceinline__ int sp_qp_begin(SpCtx<G>& c, SpState& S, GD g, bool warmFirst = false)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n, m = db.m, initial = S.initial && !warmFirst;
    GD xq = c.V(NV_XQ), xa = c.V(NV_XA), xt = c.V(NV_XT);
    GD yq = c.M(MV_YQ), ya = c.M(MV_YA), yt = c.M(MV_YT);
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI st = c.I(MI_ST), stt = c.I(MI_STT);
    S.trials0 = c.cTrials; S.admm0 = c.cAdmm; S.qpIter = 0;
    S.n_admm = initial ? o.admmFirst : o.admmHot;
    S.use_stored = (!initial && c.info->haveSolution && S.n_admm == 0);
    // The ADMM iterate (xa, ya) starts as a copy of the stored solution.  A hot start hands the stored solution to the polish directly and
    // the copy is made only if the polish fails and an ADMM round follows (one QP in a thousand on the synthetic workload).
    S.backup_pending = 0;
    if (initial) {
        GD x0 = c.V(NV_X0), y0 = c.M(MV_Y0);
        const int hasY0 = c.info->hasY0;
        g_map<G, 8>(n, t, [&](int i) { return x0[i]; }, [&](int i, double v) { xq[i] = v; xa[i] = v; });
        g_map<G, 8>(m, t, [&](int r) { return y0[r]; }, [&](int r, double v) { const double yv = hasY0 ? -v : 0.0; yq[r] = yv; ya[r] = yv; });
    } else if (S.use_stored) {
        S.backup_pending = 1;
    } else {
        g_map<G, 8>(n, t, [&](int i) { return xq[i]; }, [&](int i, double v) { xa[i] = v; });
        g_map<G, 8>(m, t, [&](int r) { return yq[r]; }, [&](int r, double v) { ya[r] = v; });
    }
    g_sync();
    S.admm_ready = 0; S.round = 0;
    if (!S.use_stored) return PH_ROUND;
    g_map<G, 4>(m, t, [&](int r) { return ID3{st[r], l[r], u[r], 0.0, yq[r]}; },
                [&](int r, ID3 v) { const int s = (v.lo == v.hi) ? ST_EQ : v.s; stt[r] = s; yt[r] = (s != ST_INACT) ? v.y : 0.0; });
    // (xt is xq already: the stored solution is the accepted trial vector of the QP before, copied from xt in sp_ph_qpend, and nothing has
    // written xt since -- use_stored is only set behind that copy)
    g_sync();
    return sp_polish_begin<G>(c, S, g, warmFirst ? 0 : 1);
}

// PH_ROUND: the preamble of a round that does not start from the stored solution -- the first QP of a homotopy, and every round after a
// polish that failed: ADMM iterations from (xa, ya), the working set they propose, the polish from there
template <int G>
__device__ __forceinline__ int sp_ph_round(SpCtx<G>& c, SpState& S, GD g)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    GD xq = c.V(NV_XQ), xa = c.V(NV_XA), xt = c.V(NV_XT);
    GD yq = c.M(MV_YQ), ya = c.M(MV_YA), za = c.M(MV_ZA), yt = c.M(MV_YT);
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI stt = c.I(MI_STT);
    if (S.backup_pending && S.round > 0) {
        g_map<G, 8>(n, t, [&](int i) { return xq[i]; }, [&](int i, double v) { xa[i] = v; });
        g_map<G, 8>(m, t, [&](int r) { return yq[r]; }, [&](int r, double v) { ya[r] = v; });
        g_sync();
        S.backup_pending = 0;
    }
    if (!S.admm_ready) {
        sp_Ex<G>(c, xa, za);
        g_map<G, 8>(m, t, [&](int r) { return D3{za[r], l[r], u[r]}; },
                    [&](int r, D3 v) { za[r] = fmin(fmax(v.a, v.b), v.c); if (isinf(v.b) && isinf(v.c)) ya[r] = 0.0; });
        g_sync();
        S.admm_ready = 1;
    }
    if (S.n_admm > 0) sp_admm<G>(c, g, S.n_admm);
    g_map<G, 4>(m, t, [&](int r) { return ID3{0, l[r], u[r], za[r], ya[r]}; },
                [&](int r, ID3 v) {
                    int s = ST_INACT;
                    if (isfinite(v.lo) && (v.z - v.lo < -v.y)) s = ST_LOWER;
                    if (isfinite(v.hi) && (v.hi - v.z < v.y)) s = ST_UPPER;
                    if (v.lo == v.hi) s = ST_EQ;
                    stt[r] = s;
                    yt[r] = (s != ST_INACT) ? v.y : 0.0;
                });
    g_map<G, 8>(n, t, [&](int i) { return xa[i]; }, [&](int i, double v) { xt[i] = v; });
    g_sync();
    return sp_polish_begin<G>(c, S, g, 0);
}
// ---- LCQProblem::runSolver, OSQP_SPARSE arm (oracle: orc_sparse_lcqp_solve) ----------------------------------------------------
// PH_START: everything in front of the first QP
template <int G>
__device__ __forceinline__ int sp_ph_start(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n;
    GD g = c.V(NV_G), gtil = c.V(NV_GTIL), xk = c.V(NV_XK), gk = c.V(NV_GK);
    GD Qx = c.V(NV_QX), Cx = c.V(NV_CX), Qp = c.V(NV_QP), Cp = c.V(NV_CP);
    memset(&S.st, 0, sizeof(S.st));
    S.rc = 0; S.qpIter = 0; S.histLen = 0; S.algoStat = 0; S.totalIter = 0;
    // warm (k_sparse_refresh): the pass that follows is still the first of the homotopy -- no step length, no perturbation, rhoOpt = rho --
    // but it starts at the last solution (NV_XK still holds it) and at the penalty rho0, without the zero-penalty QP, and its QP is a hot
    // start on the stored point and working set (sp_qp_begin)
    const int warm = c.info->warm;
    S.alphak = 1.0; S.rho = warm ? c.info->rho0 : o.initialPenaltyParameter;
    S.perturbCounter = 0;
    if (db.traceCap > 0 && t == 0) db.traceLen[c.b] = 0;     // a run that records nothing leaves an empty trace
    if (warm) {
        const double rho = S.rho;
        if (db.hasLbL || db.hasLbR) { GD gphi = c.V(NV_GPHI); g_map<G, 8>(n, t, [&](int i) { return D2{g[i], gphi[i]}; }, [&](int i, D2 v) { gtil[i] = v.a + rho * v.b; }); }
        else g_map<G, 8>(n, t, [&](int i) { return g[i]; }, [&](int i, double v) { gtil[i] = v; });
    } else {
        GD x0 = c.V(NV_X0);
        g_map<G, 8>(n, t, [&](int i) { return D2{x0[i], g[i]}; }, [&](int i, D2 v) { xk[i] = v.a; gtil[i] = v.b; });
    }
    g_sync();
    // Q x0 and C x0 once; from here on both follow the steps (sp_ph_qpend)
    sp_Qx2<G>(c, xk, xk, Qx, Qp); sp_Cx2<G>(c, xk, xk, Cx, Cp);
    c.bytes += db.by[BY_START];
    if (o.solveZeroPenaltyFirst && !warm) { for (int i = t; i < n; i += G) gk[i] = g[i]; g_sync(); }
    else { const double rho = S.rho; for (int i = t; i < n; i += G) gk[i] = rho * Cx[i] + gtil[i]; g_sync(); }
    S.initial = 1;
    S.gmaxNext = -1.0;      // max |gk| of the next QP when this level has formed it (-1: the subsolver looks)
    return sp_qp_begin<G>(c, S, gk, warm != 0);
}

// PH_QPEND: the subsolver has a verified solution (oracle: the exit of sqp_solve), then one iterate of runSolver's loop up to the next QP
template <int G>
__device__ __forceinline__ int sp_ph_qpend(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n, m = db.m, nC = db.nC, nK = db.nComp;
    GD g = c.V(NV_G), gtil = c.V(NV_GTIL), gphi = c.V(NV_GPHI), xk = c.V(NV_XK), pk = c.V(NV_PK), xnew = c.V(NV_XNEW), gk = c.V(NV_GK);
    GD Qx = c.V(NV_QX), Cx = c.V(NV_CX), Qp = c.V(NV_QP), Cp = c.V(NV_CP);
    GD yk = c.M(MV_YK), lx = c.M(MV_LX);
    const bool hasPhi = db.hasLbL || db.hasLbR;
    const double phiConst = c.info->phiConst;
    double* hist = c.info->hist;
    {   // the solution becomes the stored one (sqp_solve's exit)
        GD xq = c.V(NV_XQ), xt = c.V(NV_XT), yq = c.M(MV_YQ), yt = c.M(MV_YT);
        GI st = c.I(MI_ST), stt = c.I(MI_STT);
        S.qpIter = (c.cTrials - S.trials0) + (c.cAdmm - S.admm0);
        // (x: in the pass below that forms pk)
        g_map<G, 8>(m, t, [&](int r) { return ID{stt[r], yt[r]}; }, [&](int r, ID v) { yq[r] = v.a; st[r] = v.i; });
        if (t == 0) c.info->haveSolution = 1;
        g_sync();
    }
    SPROF(c, SP_VECTORS);
    S.st.subproblemIter += S.qpIter; S.st.qpSolverExitFlag = 0; S.st.qpSolves++;
    double rho = S.rho, alphak = S.alphak;
    auto updatePenalty = [&]() {
        if (o.nDynamicPenalty > 0) S.histLen = 0;
        rho *= o.penaltyUpdateFactor;
        S.st.rhoOpt = rho;
        if (hasPhi) { for (int i = t; i < n; i += G) gtil[i] = g[i] + rho * gphi[i]; g_sync(); }
    };
    // What the subsolver's accepted trial leaves behind makes every product of this level but one unnecessary (the dense kernel does
    // the same, lcqp_dev.hpp: lcqp_run): Q xq is in NV_TMP (sp_residual), E xq in MV_EX, and its residual r1 = -gk - Q xq - E'yq (NV_R1, gk still the vector of that QP)
    // gives E'yq.  So pk = xq - xk, Q pk = Q xq - Q xk with Q xk kept up to date below, C xq = L'(R xq) + R'(L xq) is one column
    // gather over E with the entries of E xq, C pk = C xq - C xk, and the stationarity needs no pass over E' of its own.
    // (round 2: one pass over Q, one over E, two over E' per iterate.)
    GD qxs = c.V(NV_TMP), exs = c.M(MV_EX), r1s = c.V(NV_R1), gs0 = gk;
    {
        GD xq = c.V(NV_XQ), xt = c.V(NV_XT), yq = c.M(MV_YQ);
        g_map<G, 8>(n, t, [&](int i) { return D4{xt[i], xk[i], qxs[i], Qx[i]}; }, [&](int i, D4 v) { xq[i] = v.a; xnew[i] = v.a; pk[i] = v.a - v.b; Qp[i] = v.c - v.d; });
        g_map<G, 8>(m, t, [&](int r) { return yq[r]; }, [&](int r, double v) { yk[r] = -v; });     // src/SubsolverOSQP.cpp:196-199
        g_sync();
    }
    const int initial = S.initial;
    bool perturbed = false;
    if (initial) S.st.rhoOpt = rho;
    else if (o.perturbStep) {
        perturbed = true;
        const uint64_t pc = S.perturbCounter;
        for (int i = t; i < n; i += G) {
            uint64_t z = o.perturbSeed + (pc + (uint64_t)i + 1ULL) * opaque_u64(0x9E3779B97F4A7C15ULL);
            z = (z ^ (z >> 30)) * opaque_u64(0xBF58476D1CE4E5B9ULL); z = (z ^ (z >> 27)) * opaque_u64(0x94D049BB133111EBULL); z = z ^ (z >> 31);
            xk[i] += ((int)(z % 3ULL) - 1) * 2.221e-16;
        }
        S.perturbCounter += (uint64_t)n;
        g_sync();
    }
    double sq = 0.0, sl = 0.0;      // pk'(Q + rho C) pk and pk'((Q + rho C) xk + g~)
    if (perturbed) {
        // the perturbation has to reach the penalty gradient rho C xk -- it is there to break the symmetry of problems like warm_up
        // (perturbStep :1353-1362) -- so C xk is formed from the perturbed xk and C pk from pk itself (pk = xq - xk is the unperturbed
        // difference: C xq - C xk would not be C pk), both in one pass over E and one column gather, as the dense kernel does.
        // (Q xk is not re-formed: 2.2e-16 per component is below its rounding; the dense kernel does the same.)
        sp_Cx2<G>(c, pk, xk, Cp, Cx);
        c.bytes += 3.0 * db.by[BY_E];
    } else {
        // C pk and, in the same pass, the two sums of the step length (round 5: they were a pass of their own over pk, Qp, Cp, Qx, Cx, gtil)
        struct D5 { double cx, pk, qp, qx, gt; };
        sp_C_from_Ex<G, false>(c, exs, exs, [&](int i) { return D5{Cx[i], pk[i], Qp[i], Qx[i], gtil[i]}; },
                               [&](int i, double cxq, double, D5 v) {
                                   const double cp = cxq - v.cx;
                                   Cp[i] = cp;
                                   sq += v.pk * (v.qp + rho * cp); sl += v.pk * ((v.qx + rho * v.cx) + v.gt);
                               });
        c.bytes += db.by[BY_E];
    }
    if (!initial) {
        if (perturbed) {
#pragma unroll 4
            for (int i = t; i < n; i += G) { sq += pk[i] * (Qp[i] + rho * Cp[i]); sl += pk[i] * ((Qx[i] + rho * Cx[i]) + gtil[i]); }
        }
        const double qk = g_sum<G>(sq), lk = g_sum<G>(sl);
        alphak = 1.0;
        if (qk > 0 && lk < 0) alphak = fmin(-lk / qk, 1.0);
    }
    S.initial = 0;
    // the step, the products that follow it, and updateStationarity without a box term: statk = Qk xk + g_tilde - E'yk with
    // E'yk = -E'yq = gs0 + Q xq + r1s
    double statMax = 0.0, phiSum = 0.0;
    { struct D10 { double a, b, c, d, e, f, g0, q, r, gt, gp; };
      g_map<G, 3>(n, t, [&](int i) { return D10{xk[i], pk[i], Qx[i], Qp[i], Cx[i], Cp[i], gs0[i], qxs[i], r1s[i], gtil[i], hasPhi ? (double)gphi[i] : 0.0}; },
                  [&](int i, D10 v) {
                      const double qn = v.c + alphak * v.d, cn = v.e + alphak * v.f, xn = v.a + alphak * v.b;
                      xk[i] = xn; Qx[i] = qn; Cx[i] = cn;
                      statMax = nmax(statMax, fabs(((qn + rho * cn) + v.gt) - ((v.g0 + v.q) + v.r)));
                      phiSum += (hasPhi ? v.gp * xn : 0.0) + 0.5 * xn * cn;      // getPhi of the new iterate, in its order of summation
                  }); }
    g_sync();
    const double statInf = g_max<G>(statMax);
    const double phiStep = phiConst + g_sum<G>(phiSum);      // (xk and C xk do not change again in this iterate: every getPhi below is this value)
    int totalIter = S.totalIter;
    if (db.traceCap > 0 && totalIter < db.traceCap) {   // storeSteps :488-490, printIteration :1528-1576 (the host rebuilds both from this)
        const double phiNow = phiStep;
        double so = 0.0, sm = 0.0, pm = 0.0;
        for (int i = t; i < n; i += G) { const double xv = xk[i]; so += g[i] * xv + 0.5 * xv * Qx[i]; sm += 0.5 * rho * xv * Cx[i]; pm = fmax(pm, fabs(pk[i])); }
        const double objNow = g_sum<G>(so), meritNow = objNow + g_sum<G>(sm), stepNow = g_max<G>(pm);
        double* ts = db.traceS + ((size_t)c.b * db.traceCap + totalIter) * 8;
        double* tx = db.traceX + ((size_t)c.b * db.traceCap + totalIter) * n;
        if (t == 0) {
            ts[0] = statInf; ts[1] = phiNow; ts[2] = rho; ts[3] = alphak; ts[4] = objNow; ts[5] = meritNow; ts[6] = stepNow; ts[7] = (double)S.qpIter;
            db.traceLen[c.b] = totalIter + 1;
        }
        for (int i = t; i < n; i += G) tx[i] = xk[i];
    }
    totalIter++; S.totalIter = totalIter; S.st.iterTotal++;
    bool leyffer = false;
    const int nd = o.nDynamicPenalty;
    if (nd > 0) {
        const double cur = phiStep;
        if (S.histLen < nd) { if (t == 0) hist[S.histLen] = cur; S.histLen++; g_sync(); }
        else {
            if (!(cur < o.complementarityTolerance)) {
                leyffer = true;
                for (int i = 0; i < nd; i++) if (cur < o.etaDynamicPenalty * hist[i]) { leyffer = false; break; }
            }
            g_sync();
            if (t == 0) { for (int i = 0; i + 1 < nd; i++) hist[i] = hist[i + 1]; hist[nd - 1] = cur; }
            g_sync();
        }
    }
    if (leyffer) { updatePenalty(); S.st.iterOuter++; }
    bool done = false;
    if (statInf < o.stationarityTolerance) {
        if (phiStep < o.complementarityTolerance) {
            sp_Ex<G>(c, xk, lx);
            int sflag = 1, mflag = 1, wflag = 0;
            const double ctol = o.complementarityTolerance;
            for (int i = 0; i < nK; i++) {
                const double Lx = lx[nC + i], Rx = lx[nC + nK + i];
                if (!(Lx <= ctol && Rx <= ctol)) continue;
                const double a = yk[nC + i], bq = yk[nC + nK + i];
                const double dualProd = a * bq, dualMin = fmin(a, bq);
                if (dualMin < 0) sflag = 0;
                if (fabs(dualProd) >= ctol && dualMin <= 0) { if (dualProd <= ctol) { wflag = 1; break; } mflag = 0; }
            }
            S.algoStat = wflag ? 1 : (sflag ? 4 : (mflag ? 3 : 2));
            g_sync();
            for (int i = t; i < nK; i += G) { const double Lx = lx[nC + i], Rx = lx[nC + nK + i]; yk[nC + i] -= rho * Rx; yk[nC + nK + i] -= rho * Lx; }
            g_sync();
            S.rc = 0;
            done = true;
        } else {
            updatePenalty(); S.st.iterOuter++;
        }
    }
    if (!done && totalIter > o.maxIterations) { S.rc = LCQP_MAX_ITERATIONS_REACHED; done = true; }
    if (!done && rho > o.maxPenaltyParameter) { S.rc = LCQP_MAX_PENALTY_REACHED; done = true; }
    S.rho = rho; S.alphak = alphak;
    if (done) return sp_finish<G>(c, S);
    // the next QP's linear term; its hot start needs r1 = r1_last + (g_last - g): the residual of the accepted trial is still in NV_R1
    { GD r1 = c.V(NV_R1);
      double gm = 0.0;
      g_map<G, 8>(n, t, [&](int i) { return D4{Cx[i], gtil[i], gk[i], r1[i]}; },
                  [&](int i, D4 v) { const double gn = rho * v.a + v.b; gk[i] = gn; r1[i] = v.d + (v.c - gn); gm = fmax(gm, fabs(gn)); });
      S.gmaxNext = g_max<G>(gm); }
    g_sync();
    SPROF(c, SP_LCQP);
    return sp_qp_begin<G>(c, S, gk);
}

// The vector half of the setup, shared by k_sparse_setup and k_sparse_refresh: the ADMM weights of the rows from l and u (a free row
// 1e-6 rho, an equality rho rhoEqMult, anything else rho), g_phi and phi_const from lbL / lbR (src/LCQProblem.cpp:969-996).  Returns
// phi_const.  DETECT: `changed` says whether a weight of this lane's rows differs from the one in place, i.e. from the one inside the ADMM
// KKT factor.
template <int G, bool DETECT>
__device__ __forceinline__ double sp_prepare_vectors(SpCtx<G>& c, double scale, int& changed)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m, nC = db.nC, nK = db.nComp;
    const double rho = db.opt.admmRho * scale;
    GD l = c.M(MV_L), u = c.M(MV_U), rhov = c.M(MV_RHOV);
    changed = 0;
    for (int r = t; r < m; r += G) {
        double rv = rho;
        if (isinf(l[r]) && isinf(u[r])) rv = 1e-6 * rho;
        else if (l[r] == u[r]) rv = rho * db.opt.rhoEqMult;
        if (DETECT) changed |= (rhov[r] != rv);
        rhov[r] = rv;
    }
    // phi expressions (src/LCQProblem.cpp:969-996)
    double phiConst = 0.0;
    GD gphi = c.V(NV_GPHI);
    if (db.hasLbL || db.hasLbR) {
        GD lbL = c.arr(db.lbL, nK), lbR = c.arr(db.lbR, nK);
        double s = 0.0;
        for (int i = t; i < nK; i += G) s += lbL[i] * lbR[i];
        phiConst = g_sum<G>(s);
        GD coef = c.M(MV_LX);
        for (int r = t; r < m; r += G) coef[r] = (r >= nC + nK) ? lbL[r - nC - nK] : ((r >= nC) ? lbR[r - nC] : 0.0);     // R'lbL + L'lbR
        g_sync();
        sp_ETy<G>(c, coef, gphi, [](int) { return 0.0; }, [](double v) { return v; });
    } else {
        for (int i = t; i < n; i += G) gphi[i] = 0.0;
    }
    return phiConst;
}

// the ADMM KKT matrix [Q + sigma I, E'; E, -diag(1 / rhov)] factorised, with its border when the pattern has one
template <int G>
__device__ __forceinline__ void sp_admm_factor(SpCtx<G>& c, double scale)
{
    const SpBatch& db = *c.db;
    GD rhov = c.M(MV_RHOV);
    sp_factor_band<G>(c, c.KF(true), c.KD(true), db.opt.admmSigma * scale, [=](int r) { return 1.0 / rhov[r]; }, [](int) { return true; });
    if (db.kb > 0) {
        sp_border_prepare<G>(c, true, [](int) { return true; });
        for (int jb = 0; jb < db.kb; jb++) { GD vec = sp_border_column<G>(c, true, jb); sp_solve_band<G>(c, true, vec); }
        sp_border_schur<G>(c, true, db.opt.admmSigma * scale, [=](int r) { return 1.0 / rhov[r]; }, [](int) { return true; });
    }
}

}  // namespace
