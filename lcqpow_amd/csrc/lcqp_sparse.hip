// lcqp_sparse.hip -- the SPARSE arm of the hot path on gfx950: B independent LCQPs that share one sparsity pattern, behind
// lcqp_hip_sparse_* (include/lcqp_hip.h).  G lanes of a wavefront per instance (G = 8, 16, 32 or 64: the smallest power of two
// above the half bandwidth of the KKT band), 64 / G instances per wavefront, one wavefront per workgroup (k_sparse_sched).
//
// Restates, with the conventions of the reference's OSQP_SPARSE arm (src/LCQProblem.cpp:929-960: no box constraints, nC + 2 nComp
// duals, no box term in the stationarity :1246-1272, dual sign of src/SubsolverOSQP.cpp:196-199):
//   * runSolver (src/LCQProblem.cpp:444-560) with the CSC Utilities products (src/Utilities.cpp:49-59,75-82,189-199) done as CSR
//     row gathers (Q x, E x) and CSC column gathers (E'y) -- deterministic, no atomics; C x = L'(R x) + R'(L x), C never formed;
//   * the subsolver behind SubsolverOSQP (src/SubsolverOSQP.cpp:124-200; OSQP itself is an absent submodule -- its published
//     algorithm is what is built): ADMM on the quasi-definite KKT matrix [Q + sigma I, E'; E, -1/rho], factorised ONCE per LCQP,
//     and an active-set polish on [Q + delta I, Ea'; Ea, -delta2 I] in iterative-refinement form, refactorised only when the
//     working set changes.  oracle/lcqp_oracle_sparse.c is the same algorithm in scalar C.
// The KKT matrices are factorised as BAND matrices in a reverse Cuthill-McKee ordering computed once per pattern on the host
// (lcqp_sparse_pattern.hpp; all instances of a batch share it): LDL' with a sliding G x G window in registers (G <= 16) or LDS (half bandwidth w <= G - 1 <= 63), triangular
// solves that keep the G pending rows of an instance in its G lanes (axpy form both ways, no reductions in the chain; the finished
// entry is broadcast inside the lane group by DPP).  A group of lanes behaves like a small workgroup of its own: every branch
// condition is uniform inside a group, groups of one wavefront diverge through the execution mask, there are no workgroup barriers.
// Patterns whose KKT band is wider take a bordered band (a few dense nodes behind the band, e.g. the arrow-shaped circle example) or the
// general sparse LDL' (lcqp_sparse_general.hpp); what neither holds is refused here, and the host layer runs it on the dense kernels behind
// the same OSQP_SPARSE surface.
//
// Kernels only: the host side of lcqp_hip_sparse_* is lcqp_sparse_host.hip, and lcqp_sparse_launch.hpp is the seam between the two (the
// batch struct the kernels take, the launch table instantiated at the end of this file).  One translation unit per lane-group width:
// compile with -DLCQP_TU_G=G.
//
// The kernel unit in layers, cut like the dense arm, each on the one before it:
//   lcqp_sparse_lane.hpp     the lane-group model: addressing, SpCtx, collectives, g_map, g_ell       (dense: lcqp_wg.hpp)
//   lcqp_sparse_factor.hpp   assembly, the three factorisation engines, sweeps, border, sp_solve
//   lcqp_sparse_solver.hpp   products, ADMM, polish, the phases of the homotopy, the setup's pieces  (dense: lcqp_dev.hpp)
//   lcqp_sparse.hip          this file: the setup / refresh / sensitivity (vector and panel) / probe kernels, the queue scheduler, the launches and their table
//                                                                                                    (dense: lcqp_kernels.hpp / lcqp_nch.hip)
#include "lcqp_sparse_solver.hpp"

#include <algorithm>

#ifndef LCQP_TU_G
#error "compile lcqp_sparse.hip with -DLCQP_TU_G=8|16|32|64"
#endif

namespace {

constexpr int SCHED_WAVES_PER_SIMD = 2;   // register budget of k_sparse_sched at G <= 8: 512 / SCHED_WAVES_PER_SIMD per lane

// ---- the pieces of the three setup kernels (k_sparse_setup, k_sparse_refresh, k_sparse_setup_warm) -------------------------------------
// The matrix half: everything a setup derives from the values of Q and E alone -- scale from the diagonal of Q, e1max, sigma and the four
// regularisations, and at G <= 16 the assembled band rows K0 through the bsrc / bdiag of the ordering in place.  Returns scale.
template <int G>
__device__ __forceinline__ double sp_setup_matrices(SpCtx<G>& c)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    double dmax = 0.0;
    for (int i = t; i < n; i += G)
        for (int k = db.Qp[i]; k < db.Qp[i + 1]; k++) if (db.Qi[k] == i) dmax = fmax(dmax, fabs(c.Qx()[k]));
    double scale = g_max<G>(dmax);
    if (!(scale > 1e-300)) scale = 1.0;
    double e1 = 0.0;
    {
        GD Ev = c.Ex();
        for (int r = t; r < m; r += G) { double s1 = 0.0; for (int k = db.Ep[r]; k < db.Ep[r + 1]; k++) s1 += fabs(Ev[k]); e1 = fmax(e1, s1); }
        e1 = g_max<G>(e1);
    }
    if (t == 0) {
        c.info->e1max = e1;
        c.info->scale = scale; c.info->sigma = db.opt.admmSigma * scale; c.info->delta = db.opt.proxBig * scale; c.info->delta2 = 1e-9 / scale;
        c.info->deltaS = db.opt.proxSmall * scale; c.info->delta2S = 1e-14 / scale;
    }
    if constexpr (G <= 16) {
        // the assembled band rows every factorisation of this instance streams (sp_factor_reg): the one gather from the values of Q and E
        GD K0 = c.K0(), Qv = c.Qx(), Ev = c.Ex();
        const int nnzQ = db.nnzQ;
#pragma unroll 2
        for (int r = t; r < db.N; r += G) {      // upper form: entry k of row r is K[r + k][r] (sp_factor_reg), the diagonal in entry 0
#pragma unroll
            for (int k = 1; k < G; k++) {
                const int code = db.bsrc[r * G + k];
                K0[r * G + k] = (code >= nnzQ) ? (double)Ev[code - nnzQ] : ((code >= 0) ? (double)Qv[code] : 0.0);
            }
            const int bd = db.bdiag[r];
            K0[r * G] = (bd >= 0) ? (double)Qv[bd] : 0.0;
        }
    }
    return scale;
}

// what an instance that starts cold reports when its first QP fails: sp_finish hands out MV_YK, which the first QP end writes -- zeros, as
// on a fresh handle, not the duals of the run before
template <int G>
__device__ __forceinline__ void sp_cold_duals(SpCtx<G>& c)
{
    GD yk = c.M(MV_YK);
    for (int r = c.gl; r < c.db->m; r += G) yk[r] = 0.0;
}

// the SpInfo fields of a fresh setup that do not come from the values: no solution, no polish factor, no verdict on the pivots, a cold start
template <int G>
__device__ __forceinline__ void sp_setup_marks(SpCtx<G>& c, double phiConst)
{
    sp_cold_duals<G>(c);
    if (c.gl != 0) return;
    c.info->phiConst = phiConst; c.info->haveSolution = 0; c.info->stfValid = 0; c.info->bytes = 0.0;
    c.info->bigReg = 0; c.info->warm = 0;
}

// mode 1 and a last run that returned 0: the instance starts warm (read before anything of the hand-over is written)
template <int G>
__device__ __forceinline__ int sp_warm_condition(const SpCtx<G>& c, int mode)
{
    return mode == 1 && c.info->haveSolution != 0 && c.db->stats[c.b].returnValue == 0;
}
// ... at rho0[b], else at its last rhoOpt, else at the option; a cold instance at the option
template <int G>
__device__ __forceinline__ double sp_warm_penalty(const SpCtx<G>& c, int warm, const double* rho0)
{
    const SpBatch& db = *c.db;
    if (!warm) return db.opt.initialPenaltyParameter;
    const double last = db.stats[c.b].rhoOpt;
    return rho0 ? rho0[c.b] : (last > 0.0 ? last : db.opt.initialPenaltyParameter);
}

// The hand-over between two runs.  A warm instance: the stored statuses in line with the new bounds -- equal bounds make an equality; an
// equality whose bounds differ, or a row held at a side that is infinite now, leaves with a zero multiplier (the trial's comparison of the
// factor's set with the working set then asks for a factorisation) --, SpInfo::warm and the starting penalty.  KEEP_FACTOR: the polish
// factor in memory and the verdict on its pivots (bigReg) belong to the matrices in place and stay; without it both go, as in a cold
// instance, and the first trial asks for a factorisation (sp_ph_trial: stfValid == 0).  A cold instance gets the marks of a setup.
template <int G, bool KEEP_FACTOR>
__device__ __forceinline__ void sp_warm_handover(SpCtx<G>& c, int warm, double rhoStart, double phiConst)
{
    const int t = c.gl, m = c.db->m;
    if (warm) {
        GD l = c.M(MV_L), u = c.M(MV_U), yq = c.M(MV_YQ);
        GI st = c.I(MI_ST);
        for (int r = t; r < m; r += G) {
            const double lo = l[r], hi = u[r];
            int s = st[r];
            if (lo == hi) s = ST_EQ;
            else if (s == ST_EQ || (s == ST_LOWER && isinf(lo)) || (s == ST_UPPER && isinf(hi))) s = ST_INACT;
            if (s == ST_INACT) yq[r] = 0.0;
            st[r] = s;
        }
    } else sp_cold_duals<G>(c);
    if (t == 0) {
        c.info->phiConst = phiConst; c.info->bytes = 0.0;
        c.info->warm = warm; c.info->rho0 = rhoStart;
        if (!warm) c.info->haveSolution = 0;
        if (!warm || !KEEP_FACTOR) { c.info->stfValid = 0; c.info->bigReg = 0; }
    }
}

// ---- setup: scales, rho vector, phi expressions, the ONE factorisation of the ADMM KKT matrix ----------------------------------
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_setup(SpBatch db)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl;
#ifdef LCQP_PROFILE
    if (t == 0) for (int k = 0; k < SP_NPHASE; k++) c.info->prof[k] = 0.0;
#endif
    const double scale = sp_setup_matrices<G>(c);
    int unused;
    const double phiConst = sp_prepare_vectors<G, false>(c, scale, unused);
    sp_setup_marks<G>(c, phiConst);
    g_sync();
    sp_admm_factor<G>(c, scale);
    if (t == 0) c.info->bytes = c.bytes;
}

// ---- refresh: new vectors on the setup in place, and the hand-over between two runs (lcqp_hip_sparse_resolve) ----------------------------
// Stands where k_sparse_setup stands in a run.  The matrices, hence scale, sigma, the regularisations, e1max and K0, are the ones in memory;
// what depends on the bounds and on lbL / lbR is formed again exactly as the setup forms it.  The ADMM KKT factor contains 1 / rhov: it is
// rebuilt for an instance in which the class of a row changed (free, equality, other) and left in place otherwise -- the same weights give
// the same factor bit for bit.  (Lane groups of one wavefront may part here: the factorisation and the border routines keep everything
// per group -- collectives inside the group, the group's own piece of LDS, no workgroup barrier -- as k_sparse_sched relies on when a
// step holds fewer instances than the wavefront has groups.)
// mode 0: every instance starts cold, as the setup leaves it.  mode 1: an instance whose last run returned 0 starts warm (SpInfo::warm):
// at its last x and at rho0[b] (else its last rhoOpt), its first QP a hot start on the stored point, working set and polish factor
// (sp_warm_handover).
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_refresh(SpBatch db, int mode, const double* rho0)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl;
    const double scale = c.info->scale;
    const int warm = sp_warm_condition<G>(c, mode);
    const double rhoStart = sp_warm_penalty<G>(c, warm, rho0);
    int changed;
    const double phiConst = sp_prepare_vectors<G, true>(c, scale, changed);
    sp_warm_handover<G, true>(c, warm, rhoStart, phiConst);
    g_sync();
    if (g_any<G>(changed)) sp_admm_factor<G>(c, scale);
    if (t == 0) c.info->bytes = c.bytes;
}

// ---- setup around a kept point: new VALUES of Q and E under the point of the last run (lcqp_hip_sparse_update_values, then a warm
// lcqp_hip_sparse_resolve) ----------------------------------------------------------------------------------------------------------------
// Stands where k_sparse_setup stands in a run, and is that kernel's matrix half -- scale, e1max, sigma, the regularisations, K0 in the
// ordering the host has just chosen, the vector half, the ADMM factor of EVERY instance: the one in memory holds the old Q, E and sigma --
// followed by the warm hand-over of k_sparse_refresh.  Nothing stored in permuted order outlives it unread: both factors, the border
// arrays and K0 are rebuilt before their first use, and NV_XK, NV_XQ, MV_YQ, MI_ST are in natural order, so the host may have changed the
// ordering in between.  The polish factor belongs to the old matrices: a warm instance keeps its point, statuses, multipliers and penalty
// but neither stfValid nor bigReg (sp_warm_handover<G, false>), and its first trial asks for a factorisation.  An instance that is not
// warm (no solve, or a last return value other than 0) gets exactly the marks of k_sparse_setup.  Lane groups of a wavefront part on
// `warm` as in k_sparse_refresh.
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_setup_warm(SpBatch db, const double* rho0)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl;
#ifdef LCQP_PROFILE
    if (t == 0) for (int k = 0; k < SP_NPHASE; k++) c.info->prof[k] = 0.0;
#endif
    const int warm = sp_warm_condition<G>(c, 1);
    const double rhoStart = sp_warm_penalty<G>(c, warm, rho0);
    const double scale = sp_setup_matrices<G>(c);
    int unused;
    const double phiConst = sp_prepare_vectors<G, false>(c, scale, unused);
    sp_warm_handover<G, false>(c, warm, rhoStart, phiConst);
    g_sync();
    sp_admm_factor<G>(c, scale);
    if (t == 0) c.info->bytes = c.bytes;
}

// the side codes of an instance's rows (0 outside W, -1 at lower, +1 at upper, 2 equality) into sd [m], and its flags 4 and 8 as the return
// value (include/lcqp_hip.h) -- shared by k_sparse_sensitivity and k_sparse_sensitivity_blk, as sens_marks is on the dense side.
// Flags, as on the dense path (k_sensitivity): a row of L or R at its lower bound is a side of its pair; the active side of a pair that
// is not biactive is an equality of the branch and needs no multiplier.
template <int G>
__device__ __forceinline__ int sp_sens_marks(const SpBatch& db, GI st, GD yq, int t, int* sd)
{
    const int m = db.m, nC = db.nC, nK = db.nComp;
    double ym = 0.0;
    for (int r = t; r < m; r += G) ym = fmax(ym, fabs(yq[r]));
    const double ytol = 1e-9 * (1.0 + g_max<G>(ym));
    auto sideIn = [&](int r) { const int s = st[r]; return s != ST_INACT && s != ST_UPPER; };
    int weak = 0, open = 0;
    for (int r = t; r < m; r += G) {
        const int s = st[r];
        sd[r] = (s == ST_INACT) ? 0 : ((s == ST_EQ) ? 2 : (s == ST_UPPER ? 1 : -1));
        if (s == ST_INACT) continue;
        bool ineq = s != ST_EQ;
        if (ineq && r >= nC && s != ST_UPPER) ineq = sideIn(r < nC + nK ? r + nK : r - nK);
        if (ineq && fabs(yq[r]) <= ytol) weak = 1;
    }
    for (int i = t; i < nK; i += G) if (!sideIn(nC + i) && !sideIn(nC + nK + i)) open = 1;
    weak = g_any<G>(weak) ? 1 : 0;
    open = g_any<G>(open) ? 1 : 0;
    return (weak ? 4 : 0) | (open ? 8 : 0);
}

// ---- k_sparse_sensitivity: adjoint derivatives of the returned x in g and in the bounds of the stored working set (DESIGN.md 3a'') ----------
// At the point the last run returned, x is the minimiser of 1/2 x'Qx + g'x on E_W x = b_W, W the stored working set (MI_ST).  For an upstream
// gradient v:  K0 [d; lambda] = [v; 0],  K0 = [Q, E_W'; E_W, 0];  dl/dg = -d,  dl/db_W = lambda.  The polish factor in memory is the LDL' of
// [Q + delta I, E_W'; E_W, -delta2 I] for exactly this set: an instance leaves its last QP through a trial that changed nothing behind a
// correction whose factor matched MI_STT (sp_ph_trial / sp_ph_factor), sp_ph_qpend copies MI_STT to MI_ST, and nothing factorises after it.
// Which of the two regularisation levels it holds does not matter here: it only preconditions the refinement against the UNREGULARISED
// K0 -- residual [v - Q d - E_W'lambda; -E_W d] from the ELL products, correction through the same factor -- that runs until the residual
// is under its own rounding floor, 64 eps max_i(sum of |terms|_i), at most SENS_REFINE_MAX times (contraction delta |K0^-1| per step).
// G lanes per instance, as k_sparse_refresh; per instance a loop over the nrhs vectors.  The kernel READS the state of the instance; it
// writes its outputs and four buffers that every phase of a run overwrites before it reads them: the solve vector (SpBatch::Nv), NV_PK (d),
// NV_QP (Q d) and MV_LX (lambda).
//   v, dg [B][nrhs][n];  dbo [B][nrhs][m];  side [B][m]: 0 outside W, -1 at lower, +1 at upper, 2 equality;  sinfo [B]: flag bits
//   (include/lcqp_hip.h), 0 = differentiable.
// DUAL (DESIGN.md section 3a'''', lcqp_hip_sparse_adjoint): an upstream gradient vy [B][nrhs][m] on the returned duals joins the right-hand
// side, K0 [d; lambda] = [v; -vy_W], so that E_W d = -vy_W.  The refinement carries it in its second block -- residual
// [v - Q d - E_W'lambda; -vy_W - E_W d] -- and in the scale of the rounding floor (|vy_r| on the rows of W).  Entries of vy outside W are
// loaded and dropped: whatever they hold, the bits are the same.  Without DUAL vy is not read at all, and the code is the one above.
constexpr int SENS_REFINE_MAX = 4;
template <int G, bool DUAL>
__global__ __launch_bounds__(WGS) void k_sparse_sensitivity(SpBatch db, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo, const double* vy)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl, n = db.n, m = db.m, nC = db.nC, nK = db.nComp;
    int* sd = side + (size_t)b * m;
    const int solved = c.info->haveSolution != 0 && db.stats[b].returnValue == 0;
    if (!solved) {      // (uniform inside the group) nothing to differentiate: zero outputs
        for (int r = t; r < m; r += G) sd[r] = 0;
        for (int k = 0; k < nrhs; k++) {
            double* og = dg + ((size_t)b * nrhs + k) * n;
            double* ob = dbo + ((size_t)b * nrhs + k) * m;
            for (int i = t; i < n; i += G) og[i] = 0.0;
            for (int r = t; r < m; r += G) ob[r] = 0.0;
        }
        if (t == 0) sinfo[b] = 1;
        return;
    }
    GI st = c.I(MI_ST);
    GD yq = c.M(MV_YQ);
    const int* iperm = db.iperm;
    const int marks = sp_sens_marks<G>(db, st, yq, t, sd);
    GD d = c.V(NV_PK), qd = c.V(NV_QP), lam = c.M(MV_LX), bv = c.Nv();
    const double e1 = c.info->e1max;
    int stalled = 0;
    for (int k = 0; k < nrhs; k++) {
        const double* vk = v + ((size_t)b * nrhs + k) * n;
        double* og = dg + ((size_t)b * nrhs + k) * n;
        double* ob = dbo + ((size_t)b * nrhs + k) * m;
        auto write_out = [&]() {      // dl/dg = -d, dl/db_W = lambda
            g_map<G, 8>(n, t, [&](int i) { return (double)d[i]; }, [&](int i, double w) { og[i] = -w; });
            g_map<G, 8>(m, t, [&](int r) { return (double)lam[r]; }, [&](int r, double w) { ob[r] = w; });
        };
        g_map<G, 8>(n, t, [&](int i) { return ID{iperm[i], vk[i]}; }, [&](int i, ID w) { bv[w.i] = w.a; d[i] = 0.0; });
        const double* vyk = DUAL ? vy + ((size_t)b * nrhs + k) * m : nullptr;
        if constexpr (DUAL)
            g_map<G, 8>(m, t, [&](int r) { return I2D{st[r], iperm[n + r], vyk[r]}; }, [&](int r, I2D w) { bv[w.b] = (w.a != ST_INACT) ? -w.y : 0.0; lam[r] = 0.0; });
        else
            g_map<G, 8>(m, t, [&](int r) { return iperm[n + r]; }, [&](int r, int p) { bv[p] = 0.0; lam[r] = 0.0; });
        g_sync();
        for (int it = 0;; it++) {
            sp_solve<G>(c, false, bv);
            double dm = 0.0;
            g_map<G, 8>(n, t, [&](int i) { return D2{bv[iperm[i]], d[i]}; }, [&](int i, D2 w) { const double dn = w.b + w.a; d[i] = dn; dm = fmax(dm, fabs(dn)); });
            g_map<G, 8>(m, t, [&](int r) { return ID2{st[r], bv[iperm[n + r]], lam[r]}; }, [&](int r, ID2 w) { lam[r] = (w.s != ST_INACT) ? w.y + w.v : 0.0; });
            g_sync();
            if (it == 0) write_out();      // the answer of the regularised system: what stays when the refinement does not reach its floor
            // the residual against K0, straight into the solve vector: [v - Q d - E_W'lambda; -E_W d]
            SPROF(c, SP_VECTORS);
            sp_ell<G, false>(db.ellQ, c.gl, c.Qx(), [&](int j) { return D2{d[j], 0.0}; }, [](int) { return NoPre{}; }, [&](int i, double s, double, NoPre) { qd[i] = s; });
            g_sync();
            double mx = 0.0, sc = 0.0;
            sp_ell<G, true>(db.ellT, c.gl, c.Ex(), [&](int r) { return D2{(st[r] != ST_INACT) ? (double)lam[r] : 0.0, 0.0}; },
                            [&](int i) { return ID2{iperm[i], vk[i], qd[i]}; },
                            [&](int, double s, double, ID2 w) { const double rv = (w.v - w.y) - s; bv[w.s] = rv; mx = nmax(mx, fabs(rv)); sc = fmax(sc, fabs(w.v) + fabs(w.y) + fabs(s)); });
            if constexpr (DUAL)
                sp_ell<G, false>(db.ellE, c.gl, c.Ex(), [&](int j) { return D2{d[j], 0.0}; }, [&](int r) { return I2D{st[r], iperm[n + r], vyk[r]}; },
                                 [&](int, double s, double, I2D w) {
                                     const bool in = w.a != ST_INACT;
                                     const double rv = in ? -w.y - s : 0.0;
                                     bv[w.b] = rv; mx = nmax(mx, fabs(rv));
                                     if (in) sc = fmax(sc, fabs(w.y) + fabs(s));
                                 });
            else
                sp_ell<G, false>(db.ellE, c.gl, c.Ex(), [&](int j) { return D2{d[j], 0.0}; }, [&](int r) { return I2{st[r], iperm[n + r]}; },
                                 [&](int, double s, double, I2 w) { const double rv = (w.a != ST_INACT) ? -s : 0.0; bv[w.b] = rv; mx = nmax(mx, fabs(rv)); });
            g_sync();
            SPROF(c, SP_PRODUCTS);
            const double res = g_max<G>(mx), scale = fmax(g_max<G>(sc), e1 * g_max<G>(dm));
            const bool conv = res <= 64.0 * 2.221e-16 * scale;      // (a NaN does not pass)
            if (conv || it == SENS_REFINE_MAX) {
                if (!conv) stalled = 1;
                if (conv && it > 0) write_out();
                break;
            }
        }
        g_sync();
    }
    if (t == 0) sinfo[b] = (stalled ? 2 : 0) | marks;
}

// ---- k_sparse_sensitivity_blk: k_sparse_sensitivity for many vectors, in panels of P columns (DESIGN.md section 3a''', "The sparse arm") ------
// One lane group per (instance, panel) WORK ITEM, not per instance: a Jacobian of one instance fills the device.  Per item the loop of
// k_sparse_sensitivity on P columns at once: scatter [v; 0] through iperm, panel solve (sp_solve_panel: the factor is streamed once per
// panel, P independent chains per lane), accumulate into [d; lambda], residual against the unregularised K0 by the ELL products with P
// vectors per pass over the matrix values, per column the stopping rule of the vector kernel with the same per-column scale, at most
// SENS_REFINE_MAX corrections.
// Column independence: every quantity is formed per column by the sequence of operations the vector kernel applies to that vector.  A column
// that has converged is written out at that iteration and FROZEN: its slice of the panel is zeroed (the solves then carry exact zeros
// there) and its d, lambda are not touched again.  The padding columns of a ragged last panel are zero columns, frozen from the start.  So
// the result of a column depends on nothing but that column -- not on its place in the panel, not on its neighbours -- bit for bit.
// The kernel READS the batch (pools, MI_ST, MV_YQ, SpInfo, the polish factor, the border) and WRITES only its own buffers: the staged
// outputs, side, info and the item's workspace (SpSensBlkArgs).  It uses none of SpBatch::Nv, NV_PK, NV_QP, MV_LX: two items of one
// instance run at the same time and would collide there.
// side is written by the item of panel 0; the flags are OR-ed into info (integer atomicOr: the order does not matter) -- 2 by any item with
// a stalled column, 4 and 8 by the item of panel 0, 1 by every item of an unsolved instance, whose outputs are zero.
// unit: column j of the call is e_j, written into the solve panel by the kernel itself; v is not read.
// Band engines (plain and bordered); the general LDL' has the same body under k_sparse_sensitivity_blk_general below.
constexpr int sens_panel_width(int G) { return LCQP_SPARSE_SENS_PANEL; }      // per lane width; 4 where 8 would need scratch
constexpr int general_panel_width() { return LCQP_SPARSE_SENS_PANEL; }        // the general LDL' (sp_general_front_panel): all three front classes

// g_ell's sums for the P columns of a panel behind one pass over the matrix values: per column the W slab entries in order (an absent one
// adds 0 * 0), then the tail of a long row.  xv(j, k): entry j of column k of the gathered panel; out(i, s): the P sums of row i.
template <int G, int P, bool MAP, class Xv, class Out>
__device__ __forceinline__ void sp_ell_panel(const EllMat& E, int gl, GD vals, Xv xv, Out out)
{
    const int rows = E.rows, W = E.W;
    gl = here(gl);
    for (int i = gl; i < rows; i += G) {
        double s[P];
#pragma unroll
        for (int k = 0; k < P; k++) s[k] = 0.0;
        const int p0 = E.ptr[i], p1 = E.ptr[i + 1];
#pragma unroll 4
        for (int q = 0; q < W; q++) {
            const int pos = MAP ? E.epos[q * rows + i] : ((p0 + q < p1) ? p0 + q : -1);
            const bool ok = pos >= 0;
            const int j = ok ? E.eidx[q * rows + i] : 0;
            const double av = vals[ok ? pos : 0];
            const double a = ok ? av : 0.0;
#pragma unroll
            for (int k = 0; k < P; k++) { const double x = xv(j, k); s[k] += a * (ok ? x : 0.0); }
        }
        if (E.tails)
            for (int e = p0 + W; e < p1; e++) {
                const double av = vals[E.cmap ? E.cmap[e] : e]; const int j = E.cidx[e];
#pragma unroll
                for (int k = 0; k < P; k++) s[k] += av * xv(j, k);
            }
        out(i, s);
    }
}

// GENERAL (G = 64 only): the solve is the general LDL's panel form, sp_general_solve_panel; everything else is the same code.
// DUAL (DESIGN.md section 3a'''', "The sparse arm: panels with gradients on y"; lcqp_hip_sparse_adjoint_blocked / _jacobian_duals): the
// right-hand side of k_sparse_sensitivity<G, true> for a panel, K0 [d; lambda] = [v; -vy_W] per column.  Position iperm[n + r] of column k
// holds -vy[k][r] on the rows of W and 0 elsewhere; a.v == NULL: the first block is a zero panel.  The refinement carries the second block
// -- residual [v - Q d - E_W'lambda; -vy_W - E_W d], |vy_r| + |E_r d| in the column's scale on the rows of W -- per column as the vector
// kernel does per vector.  vy is read from memory where it is used, under a select on the row's status: entries outside W never reach the
// arithmetic, whatever they hold.  Stopping, freezing and padding are those above, so a column's result depends on that column alone.
// a.dunit (the dual rows of the Jacobian): ncols = m, column j of an instance is [0; -e_r(j)], r(j) the j-th row of W in row order, found by
// a prefix count over MI_ST inside the lane group and written to rowpos[item][k] (-1: a column past |W|); nothing is uploaded.  The columns
// past |W| are padding columns; an item whose first column lies past |W| writes its -1s and returns without a solve.
// Without DUAL vy, dunit and rowpos are not read, and the code is the one above.
template <int G, bool GENERAL, bool DUAL>
__device__ __forceinline__ void sp_sensitivity_blk(const SpBatch& db, const SpSensBlkArgs& a)
{
    static_assert(!GENERAL || G == 64, "the general LDL' runs one wavefront per instance");
    constexpr int P = GENERAL ? general_panel_width() : sens_panel_width(G), IPW = 64 / G;
    const int li = blockIdx.x * IPW + threadIdx.x / G;      // item of this launch
    if (li >= a.nItems) return;
    const int item = a.item0 + li, ir = item / a.npan, pan = item - ir * a.npan, b = a.first + ir;
    const int w0 = a.first + (a.item0 + (int)blockIdx.x * IPW) / a.npan;      // the instance of the wave's first item (uniform): b >= w0
    SpCtx<G> c = sp_ctx<G>(db, b, w0, (int)threadIdx.x);
    const int t = c.gl, n = db.n, m = db.m, Np = db.Np;
    const int c0 = pan * P;
    int nc = min(P, a.ncols - c0);
    double* og = a.dg + (size_t)li * P * n;
    double* ob = a.dbo + (size_t)li * P * m;
    int* sd = a.side + (size_t)ir * m;
    const int solved = c.info->haveSolution != 0 && db.stats[b].returnValue == 0;
    if (!solved) {      // (uniform inside the group) nothing to differentiate: zero outputs
        if (pan == 0) for (int r = t; r < m; r += G) sd[r] = 0;
        for (int i = t; i < nc * n; i += G) og[i] = 0.0;
        for (int r = t; r < nc * m; r += G) ob[r] = 0.0;
        if (t == 0) atomicOr(a.info + ir, 1);
        if constexpr (DUAL) { if (a.dunit) for (int k = t; k < P; k += G) a.rowpos[(size_t)li * P + k] = -1; }
        return;
    }
    GI st = c.I(MI_ST);
    const int* iperm = db.iperm;
    if (pan == 0) {
        const int marks = sp_sens_marks<G>(db, st, c.M(MV_YQ), t, sd);
        if (t == 0 && marks) atomicOr(a.info + ir, marks);
    }
    int rk[DUAL ? P : 1];      // (DUAL, dunit) the row of W behind column k of this panel, -1 past |W|
    if constexpr (DUAL) {
        if (a.dunit) {
            int* rp = a.rowpos + (size_t)li * P;
            for (int k = t; k < P; k += G) rp[k] = -1;
            g_sync();
            int before = 0;      // rows of W in front of this tile of G rows (uniform inside the group)
            for (int r0 = 0; r0 < m; r0 += G) {
                const int r = r0 + t;
                const int in = (r < m && (int)st[r < m ? r : 0] != ST_INACT) ? 1 : 0;
                const unsigned long long mk = (__ballot(in) >> (threadIdx.x & ~(G - 1) & 63)) & (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull));
                const int rank = before + __popcll(mk & ((1ull << t) - 1ull));
                if (in && rank >= c0 && rank < c0 + nc) rp[rank - c0] = r;
                before += __popcll(mk);
            }
            g_sync();
#pragma unroll
            for (int k = 0; k < P; k++) rk[k] = rp[k];
            nc = max(0, min(nc, before - c0));      // the columns past |W| are padding columns
            if (nc == 0) return;
        }
    }
    // the item's workspace: the base of the wave's first item (uniform) + this group's offset
    const size_t wsItem = sens_blk_ws_doubles(db, P);
    double* wbase = a.ws + (size_t)blockIdx.x * IPW * wsItem;
    const unsigned woff = (unsigned)(threadIdx.x / G) * (unsigned)wsItem * 8u;
    GD bv{wbase, woff}, d{wbase + (size_t)P * Np, woff}, qd{wbase + (size_t)P * (Np + n), woff}, lam{wbase + (size_t)P * (Np + 2 * n), woff};
    const double* vi = (DUAL ? a.v == nullptr : a.unit != 0) ? nullptr : a.v + ((size_t)ir * a.ncols + c0) * n;
    auto vin = [&](int i, int k) -> double {      // entry i of column k of the panel (a padding column: zero)
        if (k >= nc) return 0.0;
        if constexpr (DUAL) return vi ? vi[(size_t)k * n + i] : 0.0;
        else return a.unit ? ((i == c0 + k) ? 1.0 : 0.0) : vi[(size_t)k * n + i];
    };
    const double* vyi = (DUAL && !a.dunit) ? a.vy + ((size_t)ir * a.ncols + c0) * m : nullptr;
    auto vyin = [&](int r, int k) -> double {      // (DUAL) entry r of column k's upstream gradient on y (a padding column: zero)
        if (k >= nc) return 0.0;
        return vyi ? vyi[(size_t)k * m + r] : ((r == rk[k]) ? 1.0 : 0.0);
    };
    for (int p = t; p < Np * P; p += G) bv[p] = 0.0;
    g_sync();
    for (int i = t; i < n; i += G) {
        const int pi = iperm[i];
#pragma unroll
        for (int k = 0; k < P; k++) { bv[pi * P + k] = vin(i, k); d[i * P + k] = 0.0; }
    }
    if constexpr (DUAL)
        for (int r = t; r < m; r += G) {
            const int pr = iperm[n + r]; const bool in = st[r] != ST_INACT;
#pragma unroll
            for (int k = 0; k < P; k++) { const double y = vyin(r, k); bv[pr * P + k] = (in && k < nc) ? -y : 0.0; }
        }
    for (int r = t; r < m * P; r += G) lam[r] = 0.0;
    g_sync();
    const double e1 = c.info->e1max;
    unsigned act = (1u << nc) - 1u;      // columns still refined (uniform inside the group)
    int stalled = 0;
    auto write_out = [&](unsigned cols) {      // dl/dg = -d, dl/db_W = lambda
#pragma unroll
        for (int k = 0; k < P; k++)
            if ((cols >> k) & 1u) {
                for (int i = t; i < n; i += G) og[(size_t)k * n + i] = -(double)d[i * P + k];
                for (int r = t; r < m; r += G) ob[(size_t)k * m + r] = (double)lam[r * P + k];
            }
    };
    for (int it = 0; act; it++) {
        if constexpr (GENERAL) sp_general_solve_panel<P>(c, bv);
        else sp_solve_panel<G, P>(c, bv);
        double dm[P], mx[P], sc[P];
#pragma unroll
        for (int k = 0; k < P; k++) dm[k] = mx[k] = sc[k] = 0.0;
        for (int i = t; i < n; i += G) {
            const int pi = iperm[i];
#pragma unroll
            for (int k = 0; k < P; k++)
                if ((act >> k) & 1u) { const double dn = (double)d[i * P + k] + (double)bv[pi * P + k]; d[i * P + k] = dn; dm[k] = fmax(dm[k], fabs(dn)); }
        }
        for (int r = t; r < m; r += G) {
            const int pr = iperm[n + r]; const bool in = st[r] != ST_INACT;
#pragma unroll
            for (int k = 0; k < P; k++)
                if ((act >> k) & 1u) lam[r * P + k] = in ? (double)lam[r * P + k] + (double)bv[pr * P + k] : 0.0;
        }
        g_sync();
        if (it == 0) write_out(act);      // the answer of the regularised system: what stays when the refinement does not reach its floor
        // the residual against K0, straight into the solve panel: [v - Q d - E_W'lambda; -E_W d]; a frozen column keeps its zeros
        sp_ell_panel<G, P, false>(db.ellQ, t, c.Qx(), [&](int j, int k) { return (double)d[j * P + k]; },
                                  [&](int i, double (&s)[P]) {
#pragma unroll
                                      for (int k = 0; k < P; k++) qd[i * P + k] = s[k];
                                  });
        g_sync();
        sp_ell_panel<G, P, true>(db.ellT, t, c.Ex(), [&](int r, int k) { return (st[r] != ST_INACT) ? (double)lam[r * P + k] : 0.0; },
                                 [&](int i, double (&s)[P]) {
                                     const int pi = iperm[i];
#pragma unroll
                                     for (int k = 0; k < P; k++) {
                                         if (!((act >> k) & 1u)) continue;
                                         const double vv = vin(i, k), y = qd[i * P + k];
                                         const double rv = (vv - y) - s[k];
                                         bv[pi * P + k] = rv; mx[k] = nmax(mx[k], fabs(rv)); sc[k] = fmax(sc[k], fabs(vv) + fabs(y) + fabs(s[k]));
                                     }
                                 });
        sp_ell_panel<G, P, false>(db.ellE, t, c.Ex(), [&](int j, int k) { return (double)d[j * P + k]; },
                                  [&](int r, double (&s)[P]) {
                                      const int pr = iperm[n + r]; const bool in = st[r] != ST_INACT;
#pragma unroll
                                      for (int k = 0; k < P; k++) {
                                          if (!((act >> k) & 1u)) continue;
                                          if constexpr (DUAL) {      // the second block carries -vy_W, and |vy_r| + |E_r d| joins the column's scale
                                              const double y = vyin(r, k);
                                              const double rv = in ? -y - s[k] : 0.0;
                                              bv[pr * P + k] = rv; mx[k] = nmax(mx[k], fabs(rv));
                                              if (in) sc[k] = fmax(sc[k], fabs(y) + fabs(s[k]));
                                          } else {
                                              const double rv = in ? -s[k] : 0.0;
                                              bv[pr * P + k] = rv; mx[k] = nmax(mx[k], fabs(rv));
                                          }
                                      }
                                  });
        g_sync();
        unsigned done = 0u, conv = 0u;
#pragma unroll
        for (int k = 0; k < P; k++) {
            const double res = g_max<G>(mx[k]), scale = fmax(g_max<G>(sc[k]), e1 * g_max<G>(dm[k]));
            const bool cv = res <= 64.0 * 2.221e-16 * scale;      // (a NaN does not pass)
            if (((act >> k) & 1u) && (cv || it == SENS_REFINE_MAX)) { done |= 1u << k; if (cv) conv |= 1u << k; else stalled = 1; }
        }
        if (done) {
            if (it > 0 && conv) write_out(conv);
            act &= ~done;
            if (act) {      // freeze: the finished columns leave the panel
                for (int p = t; p < Np; p += G) {
#pragma unroll
                    for (int k = 0; k < P; k++) if ((done >> k) & 1u) bv[p * P + k] = 0.0;
                }
                g_sync();
            }
        }
    }
    if (t == 0 && stalled) atomicOr(a.info + ir, 2);
}

template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_sensitivity_blk(SpBatch db, SpSensBlkArgs a)
{
    sp_sensitivity_blk<G, false, false>(db, a);
}

// k_sparse_sensitivity_blk with upstream gradients on y, or on the unit columns of the working set: the DUAL body above
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_sensitivity_blk_dual(SpBatch db, SpSensBlkArgs a)
{
    sp_sensitivity_blk<G, false, true>(db, a);
}

// k_sparse_sensitivity_blk on the general LDL' (DESIGN.md section 3a''', "The general engine"): one wavefront per (instance, panel) work
// item, the same body with sp_general_solve_panel as its solve.  The panel sweeps hold their right-hand sides in registers: no LDS.
// Launched only for a handle that switched the panel form on (lcqp_hip_sparse_set_general_panel).  Compiled into the unit of G = 64 alone.
#if LCQP_TU_G == 64
__global__ __launch_bounds__(WGS) void k_sparse_sensitivity_blk_general(SpBatch db, SpSensBlkArgs a)
{
    sp_sensitivity_blk<64, true, false>(db, a);
}
__global__ __launch_bounds__(WGS) void k_sparse_sensitivity_blk_general_dual(SpBatch db, SpSensBlkArgs a)
{
    sp_sensitivity_blk<64, true, true>(db, a);
}
#endif

// ---- k_sparse_kkt_probe: test and diagnostic kernel (lcqp_hip_sparse_kkt_probe) -- the factorisation engines and sp_solve held to a plain
// reference, one solve per right-hand side, no refinement (tests/test_gpu_sparse_factor.py) ------------------------------------------------
// rhs, sol [B][nrhs][N] in NODE order (variables, then the rows of E); the solve vector is filled through iperm as sp_ph_correct fills it,
// its padding positions are zero.
// mode 0 (FACTOR): [Q + dprim[b] I, E_use'; E_use, -diag(ddual[b])] (use [B][m], 0 / 1; a row outside: diagonal -1, no entries) is factorised
// into the POLISH slot by the pieces sp_ph_factor / sp_ph_correct compose -- the working set as a bit set in LDS (G <= 16, bitWords > 0),
// sp_factor_band, sp_border_prepare, the kb columns of W through sp_solve_band, sp_border_schur.  The stored polish factor is gone after it:
// haveSolution, stfValid and fact_valid are cleared (a warm re-solve starts this instance cold; the host clears its own mark).
// mode 1 (STORED): no factorisation; the factor of slot `which` (0 polish, 1 ADMM) as the last run left it, and the record of the matrix it
// is the factor of: recP [B], recD [B][m], recU [B][m] -- polish: S.dpUsed, S.d2Used on every row, MI_STF != ST_INACT; ADMM: sigma,
// 1 / rhov[r], ones.  Writes its outputs and the solve vector only.
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_kkt_probe(SpBatch db, int mode, int which, int nrhs, const double* dprim, const double* ddual, const int* use,
                                                          const double* rhs, double* sol, double* recP, double* recD, int* recU)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl, m = db.m, N = db.N;
    const int* iperm = db.iperm;
    const bool admm = mode == 1 && which == 1;
    if (mode == 0) {
        const double dp = dprim[b];
        const double* dd = ddual + (size_t)b * m;
        const int* us = use + (size_t)b * m;
        // the working set as a bit set in LDS, as sp_ph_factor builds it
        unsigned* bits = nullptr;
        if (G <= 16 && db.bitWords > 0) {
            bits = reinterpret_cast<unsigned*>(sp_dyn_lds) + (size_t)((int)threadIdx.x / G) * db.bitWords;
            for (int w = t; w < db.bitWords; w += G) {
                unsigned word = 0u;
#pragma unroll 8
                for (int k = 0; k < 32; k++) { const int r = w * 32 + k; if (r < m && us[r] != 0) word |= 1u << k; }
                bits[w] = word;
            }
            wave_sync();
        }
        if (bits) sp_factor_band<G>(c, c.KF(false), c.KD(false), dp, [=](int r) { return dd[r]; }, [=](int r) { return ((bits[r >> 5] >> (r & 31)) & 1u) != 0u; });
        else sp_factor_band<G>(c, c.KF(false), c.KD(false), dp, [=](int r) { return dd[r]; }, [=](int r) { return us[r] != 0; });
        if (db.kb > 0) {
            sp_border_prepare<G>(c, false, [=](int r) { return us[r] != 0; });
            for (int jb = 0; jb < db.kb; jb++) { GD vec = sp_border_column<G>(c, false, jb); sp_solve_band<G>(c, false, vec); }
            sp_border_schur<G>(c, false, dp, [=](int r) { return dd[r]; }, [=](int r) { return us[r] != 0; });
        }
        if (t == 0) { c.info->haveSolution = 0; c.info->stfValid = 0; db.state[b].fact_valid = 0; }
    } else if (admm) {
        GD rhov = c.M(MV_RHOV);
        for (int r = t; r < m; r += G) { recD[(size_t)b * m + r] = 1.0 / rhov[r]; recU[(size_t)b * m + r] = 1; }
        if (t == 0) recP[b] = c.info->sigma;
    } else {
        GI stf = c.I(MI_STF);
        const double d2 = db.state[b].d2Used;
        for (int r = t; r < m; r += G) { recD[(size_t)b * m + r] = d2; recU[(size_t)b * m + r] = (stf[r] != ST_INACT) ? 1 : 0; }
        if (t == 0) recP[b] = db.state[b].dpUsed;
    }
    GD bv = c.Nv();
    for (int p = N + t; p < db.Np; p += G) bv[p] = 0.0;
    for (int k = 0; k < nrhs; k++) {
        const double* bk = rhs + ((size_t)b * nrhs + k) * N;
        double* xk = sol + ((size_t)b * nrhs + k) * N;
        g_map<G, 8>(N, t, [&](int i) { return ID{iperm[i], bk[i]}; }, [&](int, ID w) { bv[w.i] = w.a; });
        g_sync();
        sp_solve<G>(c, admm, bv);
        g_map<G, 8>(N, t, [&](int i) { return (double)bv[iperm[i]]; }, [&](int i, double w) { xk[i] = w; });
        g_sync();
    }
}

// ---- k_sparse_product_probe: test and diagnostic kernel (lcqp_hip_sparse_product_probe) -- the sparse products of lcqp_sparse_solver.hpp
// themselves applied to vectors the caller supplies, so that every branch of g_ell (slab width 4 / 8, scalar tail, position map, ragged last
// tile) can be held to a plain reference (tests/test_gpu_sparse_products.py) ---------------------------------------------------------------
// Layouts: lcqp_sparse_launch.hpp (PPN_*, PPM_*, PPO_*, PPS_*).  Reads the values of Q and E and the caller's inputs; writes the caller's
// outputs and MV_LX / MV_LX2 (sp_Cx2's own scratch, which every phase of a run writes before it reads).  GL lanes per instance.
// The kernel is launched WITHOUT dynamic LDS (the products use none): c.win of the context below points at nothing and must not be touched.
template <int GL>
__device__ __forceinline__ void sp_product_probe(const SpBatch& db, const SpProductProbeArgs& a, int b, int w0, int lane)
{
    SpCtx<GL> c = sp_ctx<GL>(db, b, w0, lane);
    const int t = c.gl, n = db.n, m = db.m;
    auto vn = [&](int k) { return c.arr(a.vn, (size_t)PPN_NUM * n, (unsigned)k * n); };
    auto vm = [&](int k) { return c.arr(a.vm, (size_t)PPM_NUM * m, (unsigned)k * m); };
    auto on = [&](int k) { return c.arr(a.on, (size_t)PPO_NUM * n, (unsigned)k * n); };
    double* os = a.os + (size_t)b * PPS_NUM;
    sp_Ex<GL>(c, vn(PPN_X), c.arr(a.om, (size_t)m));
    sp_Qx2<GL>(c, vn(PPN_Q0), vn(PPN_Q1), on(PPO_QX0), on(PPO_QX1));
    {
        GD base = vn(PPN_BASE);
        const double mx = sp_ETy<GL>(c, vm(PPM_Y), on(PPO_ETY), [&](int i) { return base[i]; }, [](double v) { return v; });
        if (t == 0) os[PPS_ETY_MAX] = mx;
    }
    {
        double scale = 0.0;
        const double mx = sp_residual<GL>(c, vn(PPN_G), vn(PPN_XR), vm(PPM_YR), on(PPO_R1), on(PPO_QXR), scale);
        if (t == 0) { os[PPS_RES_MAX] = mx; os[PPS_RES_SCALE] = scale; }
    }
    sp_Cx2<GL>(c, vn(PPN_C0), vn(PPN_C1), on(PPO_CX0), on(PPO_CX1));
    {
        GD o0 = on(PPO_CE0), o1 = on(PPO_CE1);
        sp_C_from_Ex<GL, true>(c, vm(PPM_LX0), vm(PPM_LX1), [](int) { return NoPre{}; }, [&](int i, double s0, double s1, NoPre) { o0[i] = s0; o1[i] = s1; });
    }
    {
        GD o0 = on(PPO_CE), o1 = on(PPO_CEZ);
        sp_C_from_Ex<GL, false>(c, vm(PPM_LX0), vm(PPM_LX1), [](int) { return NoPre{}; }, [&](int i, double s0, double s1, NoPre) { o0[i] = s0; o1[i] = s1; });
    }
}
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_product_probe(SpBatch db, int wide, SpProductProbeArgs a)
{
    if (wide) { sp_product_probe<64>(db, a, blockIdx.x, blockIdx.x, (int)threadIdx.x); return; }      // grid = B
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    sp_product_probe<G>(db, a, b, blockIdx.x * (64 / G), (int)threadIdx.x);
}

// ---- the scheduler: persistent wavefronts that serve the phase queues of their pool -------------------------------------------------------
// Queue discipline (per pool and phase): push = take a position (atomicAdd on tail), wait until its slot's sequence says "free for this
// position" (at once, unless the ring has been lapped), store (position + 1, instance id) into it, atomicAdd on count; pop = claim entries of
// count (compare-and-swap), take as many positions (atomicAdd on head), wait for each slot's sequence to say "holds this position" (its pusher
// writes it a few instructions after taking the position), acquire fence, hand the slot on (store (position + poolSize, -)).  An instance is in at most one queue, so a ring of poolSize entries never overflows.
// Everything an instance's phase wrote to memory is released by the fence in front of its push and acquired by the fence behind the pop of
// whichever wavefront runs its next phase.
// agent scope: a pool is served by wavefronts of several XCDs, whose L2s are not coherent with each other -- the release writes the L2 back, the
// acquire invalidates L1 and L2 (workgroup-scope fences in their place: stale vectors, more iterates, 15 - 25 % SLOWER; profiles/round4)
#define SP_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#define SP_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent")
__device__ __forceinline__ int q_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long q_load64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void q_store64(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long q_slot(int seq, int id) { return ((unsigned long long)(unsigned)seq << 32) | (unsigned)id; }

// Lanes per instance depend on the phase (round 4, second step): the band phases (PH_FACTOR, PH_CORRECT, PH_ROUND with its ADMM band solves) need
// the G lanes the folded band layout is made for and take 64 / G instances per wavefront; the STREAMING phases (PH_START, PH_TRIAL, PH_QPEND:
// sparse products and element-wise loops, 60 % of the time) take ONE instance with all 64 lanes -- a wavefront instruction then reads 512
// contiguous bytes of one instance instead of eight 64-byte pieces of eight instances, the access pattern this part streams best
// (tools/micro/stream_pattern.py: 2.4 TB/s for eight far-apart pieces per wavefront, 5.8 TB/s for one stream).
constexpr int WIDE_BATCH_MAX = 16;      // instances of a streaming step at most (one per lane)
// G: the band's lane group; GL: the lanes this phase runs with (G, or all 64 in a streaming phase)
template <int G, int GL>
__device__ __forceinline__ int sp_run_phase(const SpBatch& db, int ph, int b, int w0, int lane)
{
    SpCtx<GL> c = sp_ctx<GL>(db, b, w0, lane);
    // INVARIANT (lock step): the record lives in global memory and EVERY lane of the instance's group reads and writes it -- the same
    // values, in the same instruction (S.trial++, S.round++, S.nrefine++ ...: a load and a store the group issues together).  That is
    // well defined only because (1) every branch that leads to an access of S is uniform inside the group (conditions are group
    // reductions or values read from S itself), (2) the group's lanes are lanes of ONE wavefront (G <= 64), so a load and the store
    // behind it are not separated by another lane's store, and (3) no other group touches this record while the instance is in a phase
    // (an instance is in at most one queue; the hand-over is ordered by the queue's fences).  A phase routine that accesses S under a
    // condition that differs between the lanes of a group breaks this.  (A private copy in registers, written back by lane 0, would
    // cost 50 VGPRs of the 249 the kernel has: the band factorisation's register window takes the rest.)
    SpState& S = db.state[b];
    c.cAdmm = S.cAdmm; c.cTrials = S.cTrials; c.cFact = S.cFact; c.cCorr = S.cCorr; c.cSweeps = S.cSweeps; c.bytes = S.bytes;
    GD gk = c.V(NV_GK);
    int next;
    if constexpr (GL == G) {
        // every phase can run with the band's lane group (the streaming ones do at G == 64)
        switch (ph) {
            case PH_START:   c.cAdmm = c.cTrials = c.cFact = c.cCorr = c.cSweeps = 0; c.bytes = 0.0; next = sp_ph_start<GL>(c, S); break;
            case PH_ROUND:   next = sp_ph_round<GL>(c, S, gk); break;
            case PH_TRIAL:   next = sp_ph_trial<GL>(c, S, gk); break;
            case PH_FACTOR:  next = sp_ph_factor<GL>(c, S); break;
            case PH_CORRECT: next = sp_ph_correct<GL>(c, S); break;
            default:         next = sp_ph_qpend<GL>(c, S); break;
        }
    } else {
        switch (ph) {
            case PH_START:   c.cAdmm = c.cTrials = c.cFact = c.cCorr = c.cSweeps = 0; c.bytes = 0.0; next = sp_ph_start<GL>(c, S); break;
            case PH_TRIAL:   next = sp_ph_trial<GL>(c, S, gk); break;
            default:         next = sp_ph_qpend<GL>(c, S); break;
        }
    }
    S.cAdmm = c.cAdmm; S.cTrials = c.cTrials; S.cFact = c.cFact; S.cCorr = c.cCorr; S.cSweeps = c.cSweeps; S.bytes = c.bytes;
#ifdef LCQP_PROFILE
    SPROF(c, SP_VECTORS);
    if (c.gl == 0) for (int k = 0; k < SP_NPHASE; k++) c.info->prof[k] += (double)c.prof[k];
#endif
    return next;
}

template <int G>
__global__ __launch_bounds__(WGS, (G <= 8 ? SCHED_WAVES_PER_SIMD : 1)) void k_sparse_sched(SpBatch db)
{
    constexpr int IPW = 64 / G;
    constexpr int GW = 64;      // lanes per instance of the streaming phases
    constexpr int IPWW = 64 / GW;
    __shared__ int s_id[WGS], s_next[WGS], s_ctl[2];      // the step's instances, where each goes next; [0] how many they are, [1] polls without work in a row
    // the pool's queues, derived afresh in front of the pop and in front of the push: nothing of the scheduler is alive across a phase
    struct Q { int w0, mask; unsigned long long* ring; int* ctl; int* remaining; };
    auto queues = [&]() {
        int pool = blockIdx.x % db.nPools;
        asm volatile("" : "+s"(pool));
        Q q;
        q.w0 = pool * db.poolSize; q.mask = db.poolSize - 1;
        q.ring = db.qring + (size_t)pool * PH_NUM * db.poolSize;
        q.ctl = db.qctl + (size_t)pool * (PH_NUM + 1) * QCTL;
        q.remaining = q.ctl + PH_NUM * QCTL;
        return q;
    };
    if (threadIdx.x == 0) s_ctl[1] = 0;
    for (;;) {
        const int lane = here((int)threadIdx.x);      // per step: nothing derived from the lane number is carried around the loop (it would be hoisted and spilled)
        const Q q0 = queues();
        const int w0 = q0.w0, mask = q0.mask;
        unsigned long long* ring = q0.ring;
        int* ctl = q0.ctl;
        int* remaining = q0.remaining;
        // ---- pop: one phase for the whole wavefront (lane 0 decides).  A band phase with a full wavefront's worth of instances first (the long
        // steps run at full width), else the fullest streaming queue, else whatever a band queue holds.
        int ph = -1, take = 0, base = 0;
        if (lane == 0) {
            int cnt[PH_NUM];
            for (int k = 0; k < PH_NUM; k++) cnt[k] = q_load(&ctl[k * QCTL + 2]);
            auto isWide = [](int k) { return GW != G && (k == PH_START || k == PH_TRIAL || k == PH_QPEND); };
            int best = 0;
            for (int k = 0; k < PH_NUM; k++) if (!isWide(k) && cnt[k] >= IPW && cnt[k] > best) { best = cnt[k]; ph = k; }
            if (ph < 0) for (int k = 0; k < PH_NUM; k++) if (isWide(k) && cnt[k] > best) { best = cnt[k]; ph = k; }
            if (ph < 0) for (int k = 0; k < PH_NUM; k++) if (cnt[k] > best) { best = cnt[k]; ph = k; }
            if (ph >= 0) {
                // instances of a streaming step: they run one after the other on this wavefront, so a long step makes the last of them wait
                // for the others while wavefronts elsewhere poll -- P = unfinished instances per SIMD of the machine up to 4, P / 2 beyond,
                // at most WIDE_BATCH_MAX (the fences of a step are paid once for all of them: full steps for batches that fill the
                // machine).  profiles/round5/sparse_wide_batch_rule.log: against 16 per step +20 % at B = 1024, +15 % at 2048, +11 % at
                // 4096, +7 % at 8192, the same from 16 384 on
                int wb = WIDE_BATCH_MAX;
                if (isWide(ph)) { const int P = q_load(remaining) / db.wideDiv; wb = max(1, min(WIDE_BATCH_MAX, P <= 4 ? P : max(4, P >> 1))); }
                take = min(best, isWide(ph) ? IPWW * wb : IPW);
                if (atomicCAS(&ctl[ph * QCTL + 2], best, best - take) == best) base = atomicAdd(&ctl[ph * QCTL + 1], take);
                else { ph = -1; take = 0; }      // somebody else moved the counter: look again
            }
        }
        ph = __builtin_amdgcn_readfirstlane(ph); take = __builtin_amdgcn_readfirstlane(take); base = __builtin_amdgcn_readfirstlane(base);
#ifdef LCQP_SCHED_PROFILE
        const unsigned long long tq0 = __builtin_amdgcn_s_memtime();
#endif
        if (take == 0) {
            if (q_load(remaining) <= 0) break;
            const int idle = s_ctl[1] + 1;
            if (lane == 0) s_ctl[1] = idle;
            // back off: a wavefront that finds nothing polls again later and later (each poll reads the pool's counters through the L2 all
            // wavefronts of the pool share; with s_sleep(32) per poll a quarter of idle wavefronts halved the rate of the working ones:
            // profiles/round5/sparse_waves.log) -- 2^min(idle, 7) / 8 sleeps of 127 x 64 clocks, at most ~ 60 us
            if (idle > 2) { const int reps = (1 << min(idle, 7)) >> 3; for (int k = 0; k < max(reps, 1); k++) __builtin_amdgcn_s_sleep(127); }
#ifdef LCQP_SCHED_PROFILE
            if (lane == 0) { atomicAdd(&db.qprof[PH_NUM * 3 + 0], __builtin_amdgcn_s_memtime() - tq0); atomicAdd(&db.qprof[PH_NUM * 3 + 1], 1ull); }
#endif
            continue;
        }
        if (lane == 0) { s_ctl[1] = 0; s_ctl[0] = take; }
        int myid = -1;
        const size_t qoff = (size_t)ph * db.poolSize;
        if (lane < take) {
            const int pos = base + lane;
            unsigned long long e;
            while ((int)((e = q_load64(&ring[qoff + (pos & mask)])) >> 32) != pos + 1) __builtin_amdgcn_s_sleep(1);
            myid = (int)(unsigned)e;
        }
        SP_ACQUIRE();                                                                    // (also orders the slot's read in front of handing it on)
        if (lane < take) {
            const int pos = base + lane;
            q_store64(&ring[qoff + (pos & mask)], q_slot(pos + db.poolSize, -1));
        }
        const bool wide = GW != G && (ph == PH_START || ph == PH_TRIAL || ph == PH_QPEND);
        // ---- run the phase for the instances popped (lane groups without one idle through it).  The instances of the step and where each goes
        // next are kept in LDS, one per lane: no register of the scheduler is alive across a phase.
        s_id[lane] = myid;
        __builtin_amdgcn_wave_barrier();
        if (wide) {
            // streaming phases: the instances popped (up to WIDE_BATCH_MAX) one after the other, GW lanes each, so that the fences of the step
            // -- the release writes back the whole XCD's L2 -- are paid once for all of them.  A streaming phase that leads to another one
            // (an accepted trial -> the end of its QP -> the first trial of the next) stays here: same lanes, same instance, its own stores in
            // program order -- no queue, no fences.
            for (int j = 0; j < take; j += IPWW) {
                const int ln = here(lane), bj = s_id[j + ln / GW];
                int nj = -1;
                if (bj >= 0)
                    for (int p = ph;; p = nj) {
                        nj = sp_run_phase<G, GW>(db, p, bj, w0, ln);
                        if (!(nj == PH_TRIAL || nj == PH_QPEND)) break;
                    }
                if ((ln & (GW - 1)) == 0) s_next[j + ln / GW] = nj;
            }
        } else {
            // band phases: 64 / G instances side by side, one such pass per step
            for (int j = 0; j < take; j += IPW) {
                const int l0 = here(lane), bj = s_id[j + l0 / G];
                int nj = -1;
                if (bj >= 0)
                    for (int p = ph;; p = nj) {      // (a factorisation is always followed by its correction: same lanes, same instances)
                        nj = sp_run_phase<G, G>(db, p, here(bj), w0, here(l0));      // (re-laundered per pass: nothing of the instance's addressing is carried around the loop)
                        if (!(p == PH_FACTOR && nj == PH_CORRECT)) break;
                    }
                if ((l0 & (G - 1)) == 0) s_next[j + l0 / G] = nj;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- push: what this wavefront wrote is released, then every instance goes to the queue of its next phase
        SP_RELEASE();
        if (here((int)threadIdx.x) < s_ctl[0]) {
            const Q q1 = queues();
            const int b = s_id[threadIdx.x], next = s_next[threadIdx.x];
            if (next == PH_NUM) atomicSub(q1.remaining, 1);
            else {
                const int pos = atomicAdd(&q1.ctl[next * QCTL + 0], 1), sl = pos & q1.mask;
                const size_t noff = (size_t)next * db.poolSize;
                while ((int)(q_load64(&q1.ring[noff + sl]) >> 32) != pos) __builtin_amdgcn_s_sleep(1);      // (waits only when the ring has been lapped onto a slot that is still being read)
                q_store64(&q1.ring[noff + sl], q_slot(pos + 1, b));
                atomicAdd(&q1.ctl[next * QCTL + 2], 1);
            }
        }
#ifdef LCQP_SCHED_PROFILE
        if (lane == 0) { atomicAdd(&db.qprof[ph * 3 + 0], __builtin_amdgcn_s_memtime() - tq0); atomicAdd(&db.qprof[ph * 3 + 1], 1ull); atomicAdd(&db.qprof[ph * 3 + 2], (unsigned long long)take); }
#endif
    }
}

// fills the queues of a run: every instance of every pool into PH_START
__global__ void k_sparse_sched_init(SpBatch db)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = db.nPools * (PH_NUM + 1) * QCTL;
    if (b < nq) {
        const int pool = b / ((PH_NUM + 1) * QCTL), k = (b / QCTL) % (PH_NUM + 1), f = b % QCTL;
        const int inPool = max(0, min(db.poolSize, db.B - pool * db.poolSize));
        int v = 0;
        if (k == PH_NUM) v = (f == 0) ? inPool : 0;                        // remaining
        else if (k == PH_START) v = (f == 0 || f == 2) ? inPool : 0;       // tail = count = instances of the pool, head = 0
        db.qctl[b] = v;
    }
    if (b < db.nPools * db.poolSize) {
        const int pool = b / db.poolSize, i = b % db.poolSize;
        for (int k = 0; k < PH_NUM; k++) {
            const bool filled = (k == PH_START && pool * db.poolSize + i < db.B);      // position i of the start queue holds instance i of the pool
            db.qring[((size_t)pool * PH_NUM + k) * db.poolSize + i] = filled ? q_slot(i + 1, pool * db.poolSize + i) : q_slot(i, -1);
        }
    }
}

// first: the kernel in front of the homotopy -- k_sparse_setup<G>, k_sparse_refresh<G>(mode, rho0) or k_sparse_setup_warm<G>(rho0) (lcqp_hip_sparse_resolve)
template <int G>
static void sp_launch(const SpBatch& db, int cus, hipStream_t stream, hipEvent_t mid, SpFirst first, int mode, const double* rho0)
{
    const int ipw = 64 / G, grid = (db.B + ipw - 1) / ipw;
    // LDS: the working sets' bit sets of sp_ph_factor (G <= 16), the window of sp_factor_lds (per group G x G and 16 staged rows) otherwise
    const size_t ldsBytes = G <= 16 ? sizeof(unsigned) * (size_t)ipw * db.bitWords : sizeof(double) * (size_t)ipw * group_lds_doubles(G);
    switch (first) {
    case SpFirst::REFRESH: hipLaunchKernelGGL(k_sparse_refresh<G>, dim3(grid), dim3(WGS), ldsBytes, stream, db, mode, rho0); break;
    case SpFirst::SETUP_WARM: hipLaunchKernelGGL(k_sparse_setup_warm<G>, dim3(grid), dim3(WGS), ldsBytes, stream, db, rho0); break;
    case SpFirst::SETUP: hipLaunchKernelGGL(k_sparse_setup<G>, dim3(grid), dim3(WGS), ldsBytes, stream, db); break;
    }
    (void)hipEventRecord(mid, stream);
    const int ninit = std::max(db.nPools * db.poolSize, db.nPools * (PH_NUM + 1) * QCTL);
    hipLaunchKernelGGL(k_sparse_sched_init, dim3((ninit + 255) / 256), dim3(256), 0, stream, db);
    // persistent wavefronts: as many as the batch has work for, at most what the device (cus compute units) holds at once (they leave when
    // their pool is done); a multiple of the number of pools so that every pool is served
    // More wavefronts than one per 64 / G instances for batches that do not fill the machine (round 5, profiles/round5/sparse_waves_small_batches.log):
    // a streaming phase runs ONE instance on a wavefront's 64 lanes, so a wavefront that holds eight instances serialises their trial heads and
    // QP ends; with a wavefront per instance (up to 256) or per four instances B = 64 gains 52 %, 256: 44 %, 512: 39 %, 1024: 23 %, 2048: 12 %,
    // 8192: 4 % (4096: +-0); idle wavefronts back off exponentially, so the surplus costs nothing.
    int waves = std::max(grid, std::max(std::min(db.B, 256), db.B / 4));
    waves = std::min(waves, cus * 4 * (G <= 8 ? SCHED_WAVES_PER_SIMD : 1));      // resident at once (k_sparse_sched's launch bounds)
    waves = ((waves + db.nPools - 1) / db.nPools) * db.nPools;
    hipLaunchKernelGGL(k_sparse_sched<G>, dim3(waves), dim3(WGS), ldsBytes, stream, db);
}

// one launch of k_sparse_sensitivity<G, DUAL> (DESIGN.md sections 3a'', 3a'''') on device buffers
template <int G, bool DUAL>
static void sp_launch_sens(const SpBatch& db, hipStream_t stream, int nrhs, const double* v, const double* vy, double* dg, double* dbo, int* side, int* sinfo)
{
    const int ipw = 64 / G, grid = (db.B + ipw - 1) / ipw;
    const size_t ldsBytes = (G == 64 && db.general) ? sizeof(double) * (size_t)ipw * group_lds_doubles(G) : 0;      // the window of the general solve
    hipLaunchKernelGGL((k_sparse_sensitivity<G, DUAL>), dim3(grid), dim3(WGS), ldsBytes, stream, db, nrhs, v, dg, dbo, side, sinfo, vy);
}
template <int G>
static void sp_launch_sensitivity(const SpBatch& db, hipStream_t stream, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo)
{
    sp_launch_sens<G, false>(db, stream, nrhs, v, nullptr, dg, dbo, side, sinfo);
}
template <int G>
static void sp_launch_sensitivity_dual(const SpBatch& db, hipStream_t stream, int nrhs, const double* v, const double* vy, double* dg, double* dbo, int* side, int* sinfo)
{
    sp_launch_sens<G, true>(db, stream, nrhs, v, vy, dg, dbo, side, sinfo);
}

// one launch of k_sparse_sensitivity_blk<G> (lcqp_sparse_launch.hpp: SpSensBlkArgs): a lane group per work item, no LDS (band engines only)
template <int G>
static void sp_launch_sensitivity_blk(const SpBatch& db, hipStream_t stream, const SpSensBlkArgs& a)
{
    const int ipw = 64 / G, grid = (a.nItems + ipw - 1) / ipw;
    hipLaunchKernelGGL(k_sparse_sensitivity_blk<G>, dim3(grid), dim3(WGS), 0, stream, db, a);
}

// one launch of k_sparse_sensitivity_blk_general: a wavefront per work item, no LDS
static void sp_launch_sensitivity_blk_general(const SpBatch& db, hipStream_t stream, const SpSensBlkArgs& a)
{
#if LCQP_TU_G == 64
    hipLaunchKernelGGL(k_sparse_sensitivity_blk_general, dim3(a.nItems), dim3(WGS), 0, stream, db, a);
#endif
}

// the same two launches on the DUAL kernels (k_sparse_sensitivity_blk_dual<G>, k_sparse_sensitivity_blk_general_dual)
template <int G>
static void sp_launch_sensitivity_blk_dual(const SpBatch& db, hipStream_t stream, const SpSensBlkArgs& a)
{
    const int ipw = 64 / G, grid = (a.nItems + ipw - 1) / ipw;
    hipLaunchKernelGGL(k_sparse_sensitivity_blk_dual<G>, dim3(grid), dim3(WGS), 0, stream, db, a);
}
static void sp_launch_sensitivity_blk_general_dual(const SpBatch& db, hipStream_t stream, const SpSensBlkArgs& a)
{
#if LCQP_TU_G == 64
    hipLaunchKernelGGL(k_sparse_sensitivity_blk_general_dual, dim3(a.nItems), dim3(WGS), 0, stream, db, a);
#endif
}

// one launch of k_sparse_kkt_probe<G> on device buffers; the LDS of a factorisation (sp_launch), which covers the window of the general solve
template <int G>
static void sp_launch_kkt_probe(const SpBatch& db, hipStream_t stream, int mode, int which, int nrhs, const double* dprim, const double* ddual, const int* use,
                                const double* rhs, double* sol, double* recP, double* recD, int* recU)
{
    const int ipw = 64 / G, grid = (db.B + ipw - 1) / ipw;
    const size_t ldsBytes = G <= 16 ? sizeof(unsigned) * (size_t)ipw * db.bitWords : sizeof(double) * (size_t)ipw * group_lds_doubles(G);
    hipLaunchKernelGGL(k_sparse_kkt_probe<G>, dim3(grid), dim3(WGS), ldsBytes, stream, db, mode, which, nrhs, dprim, ddual, use, rhs, sol, recP, recD, recU);
}

// one launch of k_sparse_product_probe<G> on device buffers: a lane group per instance, or with `wide` a wavefront; the products use no LDS
template <int G>
static void sp_launch_product_probe(const SpBatch& db, hipStream_t stream, int wide, const SpProductProbeArgs& a)
{
    const int ipw = 64 / G, grid = wide ? db.B : (db.B + ipw - 1) / ipw;
    hipLaunchKernelGGL(k_sparse_product_probe<G>, dim3(grid), dim3(WGS), 0, stream, db, wide, a);
}

}  // namespace

// the launch table of this unit's width (lcqp_sparse_launch.hpp)
namespace lcqp_sparse {
template <int G>
const SpKernels& sparse_kernels()
{
    static const SpKernels k = {G, sp_launch<G>, sp_launch_sensitivity<G>, sp_launch_sensitivity_dual<G>, sp_launch_kkt_probe<G>,
                                sp_launch_sensitivity_blk<G>, sens_panel_width(G),
                                G == 64 ? sp_launch_sensitivity_blk_general : nullptr, G == 64 ? general_panel_width() : 0,
                                sp_launch_product_probe<G>,
                                sp_launch_sensitivity_blk_dual<G>, G == 64 ? sp_launch_sensitivity_blk_general_dual : nullptr};
    return k;
}
}
template const lcqp_sparse::SpKernels& lcqp_sparse::sparse_kernels<LCQP_TU_G>();
