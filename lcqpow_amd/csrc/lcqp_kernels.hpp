// lcqp_kernels.hpp -- the kernels that are instantiated once per padded size np = 128*NCH, and their launch tables (lcqp_launch.hpp).
// Each instantiation is its own translation unit (lcqp_nch.hip compiled with -DLCQP_TU_NCH=1,2,3,4,8,16,32, and for NCH <= 4 a second
// time with -DLCQP_TU_FEW for the two persistent kernels alone): the eleven builds run in parallel, and the register allocation of one
// size cannot perturb another's (cdna_hip_programming.md §5.4 rule 19).
#pragma once
#include "lcqp_dev.hpp"
#include "lcqp_launch.hpp"
#include "../../include/lcqp_synth.h"

using namespace lcqp;


// ---- the vector half of the setup: bounds of the box rows, ADMM rho vector, phi expressions (k_prepare, k_refresh, k_prepare_warm) ------
// Returns phi_const (uniform); writes M_L / M_U of the box rows, M_RHOV and V_GPHI.
template <int NCH>
__device__ __forceinline__ double prepare_vectors(const DevBatch& db, Ctx<NCH>& c, Lds lds, double scale)
{
    constexpr int np = 128 * NCH;
    const int b = c.b, t = threadIdx.x;
    const int mA = db.mA, nC = db.nC, nComp = db.nComp;
    const int nfin = c.info->nfin;
    const int mE = mA + nfin;
    double *l = c.M(M_L), *u = c.M(M_U), *rhov = c.M(M_RHOV);
    for (int k = t; k < nfin; k += WG) {
        const int bi = c.boxidx[k];
        l[mA + k] = c.V(V_LB)[bi]; u[mA + k] = c.V(V_UB)[bi];
    }
    __syncthreads();
    const double rho = db.opt.admmRho * scale;
    for (int r = t; r < mE; r += WG) {
        const double lo = l[r], hi = u[r];
        double rv = rho;
        if (isinf(lo) && isinf(hi)) rv = 0.0;
        else if (lo == hi) rv = rho * db.opt.rhoEqMult;
        rhov[r] = rv;
    }
    // phi expressions, src/LCQProblem.cpp:969-996
    double phiConst = 0.0;
    double* gphi = c.V(V_GPHI);
    if (db.hasLbL || db.hasLbR) {
        const double* lbL = db.lbL + (size_t)b * nComp;
        const double* lbR = db.lbR + (size_t)b * nComp;
        double s = 0.0;
        for (int i = t; i < nComp; i += WG) s += lbL[i] * lbR[i];
        phiConst = block_sum(s, lds);
        double* coef = c.M(M_COEF);
        for (int r = t; r < mA; r += WG) {
            double v = 0.0;
            if (r >= nC && r < nC + nComp) v = lbR[r - nC];          // L' * lbR
            else if (r >= nC + nComp) v = lbL[r - nC - nComp];       // R' * lbL
            coef[r] = v;
        }
        __syncthreads();
        wg_rows<NCH>(c.E, nullptr, mA, nullptr, nullptr, coef, lds, [&](int i, double sum) { gphi[i] = -sum; });
    } else {
        wg_fill(gphi, 0.0, np);
    }
    return phiConst;
}

// the subsolver of an instance starts cold: no dependent-row flags or promotions survive (qp_polish), the inverse factor of the
// working-set matrix is empty, no stored solution, a homotopy from x0 at the initial penalty
template <int NCH>
__device__ __forceinline__ void prepare_cold(const DevBatch& db, Ctx<NCH>& c)
{
    const int t = threadIdx.x;
    int *dep = c.I(I_DEP), *prio = c.I(I_PRIO), *rslot = c.I(I_SLOT);
    for (int r = t; r < db.mEcap; r += WG) { dep[r] = 0; prio[r] = 0; rslot[r] = -1; }
    for (int a = t; a < db.capS; a += WG) c.idx[a] = -1;
    if (t == 0) {
        c.info->prioCtr = 0;
        c.info->ndep = 0;
        c.info->haveSolution = 0;
        c.info->nT = 0; c.info->ns = 0;
        c.info->warm = 0; c.info->rho0 = db.opt.initialPenaltyParameter;
    }
}

// the matrix half of k_prepare / k_prepare_warm: the scale of Q (returned, uniform), the unit diagonal of its padding, the box rows of E
template <int NCH>
__device__ __forceinline__ double prepare_matrices(const DevBatch& db, Ctx<NCH>& c, Lds lds)
{
    constexpr int np = 128 * NCH;
    const int t = threadIdx.x;
    const int n = db.n, mA = db.mA;
    double dmax = 0.0;
    for (int i = t; i < n; i += WG) dmax = fmax(dmax, fabs(c.Q[(size_t)i * np + i]));
    double scale = block_max(dmax, lds);
    if (!(scale > 1e-300)) scale = 1.0;
    for (int i = n + t; i < np; i += WG) c.Q[(size_t)i * np + i] = 1.0;
    const int nfin = c.info->nfin;
    for (int k = 0; k < nfin; k++) {
        double* row = c.E + (size_t)(mA + k) * np;
        const int bi = c.boxidx[k];
        for (int i = t; i < np; i += WG) row[i] = (i == bi) ? 1.0 : 0.0;
    }
    return scale;
}

// the marks of a fresh setup (thread 0 of k_prepare / k_prepare_warm)
template <int NCH>
__device__ __forceinline__ void prepare_marks(const DevBatch& db, Ctx<NCH>& c, double scale, double phiConst)
{
    c.info->mE = db.mA + c.info->nfin;
    c.info->scale = scale;
    c.info->sigma = db.opt.admmSigma * scale;
    c.info->rhoAdmm = db.opt.admmRho * scale;
    c.info->phiConst = phiConst;
    c.info->cNnz = -1;
    c.info->setupFail = 0;
    c.info->isSetup = 1;
}

// ---- k_prepare: scales, padding, box rows, ADMM rho vector, phi expressions ----------------------
template <int NCH>
__global__ __launch_bounds__(WG) void k_prepare(DevBatch db)
{
    LCQP_LDS_N(NCH)
    const int b = blockIdx.x, t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const double scale = prepare_matrices<NCH>(db, c, lds);
    const double phiConst = prepare_vectors<NCH>(db, c, lds, scale);
    prepare_cold<NCH>(db, c);
    if (t == 0) prepare_marks<NCH>(db, c, scale, phiConst);
}

// ---- k_refresh: new vectors on the setup in place, and the hand-over between two runs (lcqp_hip_batch_resolve) ----------------------
// Stands where the five setup kernels stand in a run: the matrices, hence scale, sigma, spv, C and its compressed rows, L1, Et and M, are
// the ones in HBM; what depends on g, the bounds and lbL / lbR is formed again exactly as k_prepare forms it, and L_K (which contains
// E' diag(rho) E) is left to the rare instance that needs ADMM.  mode 0: every instance starts cold -- the bits of a run after a fresh load.
// mode 1: an instance whose last run returned 0 starts warm (InstInfo::warm): from its last x, at rho0[b] (else its last rhoOpt), and its
// first QP is a hot start on the stored point, working set and inverse factor.  The stored statuses are brought in line with the new bounds
// (a row with equal bounds is an equality; an equality whose bounds differ, or a row held at a side that is infinite now, leaves with a zero
// multiplier -- the polish rotates it out of the factor), a row flagged dependent hands its multiplier back as in qp_solve, and the stored
// residual is marked void (haveSolution = 2): the polish takes its cold entry, which also forms E x, the margins and the status of every row
// anew -- nothing of the last run's row state survives a moved bound.
// an instance starts warm when the caller asks for it and its last run returned 0 on a setup that did not fail (uniform)
template <int NCH>
__device__ __forceinline__ int warm_start(const DevBatch& db, const Ctx<NCH>& c, int mode)
{
    return mode == 1 && c.info->haveSolution != 0 && db.stats[c.b].returnValue == 0 && c.info->setupFail == 0;
}

// the penalty a warm instance starts at: rho0[b] when given, else its last rhoOpt; a cold one starts at the initial penalty
template <int NCH>
__device__ __forceinline__ double warm_penalty(const DevBatch& db, const Ctx<NCH>& c, int warm, const double* rho0)
{
    if (!warm) return db.opt.initialPenaltyParameter;
    const double last = db.stats[c.b].rhoOpt;
    return rho0 ? rho0[c.b] : (last > 0.0 ? last : db.opt.initialPenaltyParameter);
}

// the hand-over of a warm instance (the comment of k_refresh): statuses in line with the bounds in M_L / M_U, multipliers of dependent rows
// handed back, no flags or promotions, the stored residual void.  EMPTY (k_prepare_warm): the matrices changed too -- the inverse factor
// is emptied as prepare_cold empties it, and the polish's cold entry builds it in one piece from the stored working set (ti_bulk)
template <int NCH, bool EMPTY>
__device__ __forceinline__ void prepare_warm(const DevBatch& db, Ctx<NCH>& c, double rhoStart)
{
    const int t = threadIdx.x;
    const int mE = c.mE;
    const double *l = c.M(M_L), *u = c.M(M_U);
    double* yq = c.M(M_YQ);
    int *st = c.I(I_ST), *dep = c.I(I_DEP), *prio = c.I(I_PRIO);
    for (int r = t; r < mE; r += WG) {
        const double lo = l[r], hi = u[r];
        int s = st[r];
        if (lo == hi) s = ST_EQ;
        else if (s == ST_EQ || (s == ST_LOWER && isinf(lo)) || (s == ST_UPPER && isinf(hi))) s = ST_INACT;
        if (s == ST_INACT || dep[r]) yq[r] = 0.0;
        st[r] = s;
        dep[r] = 0; prio[r] = 0;
    }
    if constexpr (EMPTY) {
        int* rslot = c.I(I_SLOT);
        for (int r = t; r < db.mEcap; r += WG) rslot[r] = -1;
        for (int a = t; a < db.capS; a += WG) c.idx[a] = -1;
    }
    if (t == 0) {
        c.info->prioCtr = 0; c.info->ndep = 0; c.info->haveSolution = 2; c.info->warm = 1; c.info->rho0 = rhoStart;
        if constexpr (EMPTY) { c.info->nT = 0; c.info->ns = 0; }
    }
}

template <int NCH>
__global__ __launch_bounds__(WG) void k_refresh(DevBatch db, int mode, const double* rho0)
{
    LCQP_LDS_N(NCH)
    const int b = blockIdx.x, t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const double scale = c.info->scale;
    const int warm = warm_start<NCH>(db, c, mode);
    const double rhoStart = warm_penalty<NCH>(db, c, warm, rho0);
    __syncthreads();      // every thread has read the marks thread 0 rewrites below
    const double phiConst = prepare_vectors<NCH>(db, c, lds, scale);
    if (warm) prepare_warm<NCH, false>(db, c, rhoStart);
    else prepare_cold<NCH>(db, c);
    if (t == 0) {
        c.info->rhoAdmm = db.opt.admmRho * scale;
        c.info->phiConst = phiConst;
        c.info->kReady = 0;
    }
}

// ---- k_prepare_warm: k_prepare for a batch whose matrices changed under a stored point (lcqp_hip_batch_update_matrices + _resolve) -------
// Stands where k_prepare stands in the setup: everything that depends on the matrices is formed again by it and the four kernels behind
// it.  An instance whose last run returned 0 keeps its x (V_XK), its multipliers and statuses and its penalty, exactly as k_refresh hands
// them over in mode 1, and starts warm at rho0[b] (else its last rhoOpt) -- but Et and M are new, so no row of the old inverse factor may
// survive: the factor is emptied.  Every other instance starts cold.
template <int NCH>
__global__ __launch_bounds__(WG) void k_prepare_warm(DevBatch db, const double* rho0)
{
    LCQP_LDS_N(NCH)
    const int b = blockIdx.x, t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const int warm = warm_start<NCH>(db, c, 1);
    const double rhoStart = warm_penalty<NCH>(db, c, warm, rho0);
    __syncthreads();      // every thread has read the marks thread 0 rewrites below
    const double scale = prepare_matrices<NCH>(db, c, lds);
    const double phiConst = prepare_vectors<NCH>(db, c, lds, scale);
    if (warm) prepare_warm<NCH, true>(db, c, rhoStart);
    else prepare_cold<NCH>(db, c);
    if (t == 0) prepare_marks<NCH>(db, c, scale, phiConst);
}

// ---- the setup of a batch that holds ONE set of matrices (lcqp_hip_batch_create_shared; DESIGN.md section 3a, "One set of matrices") -------
// The setup chain runs on a grid of one matrix instance, instance 0, whose blocks are the batch's: k_prepare_shared stands where k_prepare
// stands and is its matrix half alone -- no vector, status, point or working set of instance 0 is touched --, then k_build_C, k_compress_C,
// k_factor, k_trsm and k_build_M as they are.  k_share_setup, over all B instances, then hands every instance the marks the chain left in
// InstInfo 0 and forms the vector half exactly as k_prepare / k_prepare_warm form it.
// src: the instance whose list of box-bounded variables is the batch's (the lowest one that holds a problem; the set is one for the batch).
template <int NCH>
__global__ __launch_bounds__(WG) void k_prepare_shared(DevBatch db, int src)
{
    LCQP_LDS_N(NCH)
    const int t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, 0, lds);
    const int nfin = uniform_i(db.info[src].nfin), prevFail = uniform_i(c.info->setupFail);
    __syncthreads();      // every thread has read the marks thread 0 rewrites below
    c.boxidx = db.boxidx + (size_t)src * (128 * NCH);
    if (t == 0) c.info->nfin = nfin;      // (prepare_matrices and prepare_marks read it; src == 0, or instance 0 holds no problem)
    __syncthreads();
    const double scale = prepare_matrices<NCH>(db, c, lds);
    if (t == 0) {
        c.info->prevFail = prevFail;
        c.info->mE = db.mA + nfin;
        c.info->scale = scale;
        c.info->sigma = db.opt.admmSigma * scale;
        c.info->cNnz = -1;
        c.info->setupFail = 0;
        c.info->isSetup = 1;
    }
}

// mode 0: every instance starts cold (k_prepare); mode 1: the matrices changed under a stored point and an instance whose last run
// returned 0 starts warm with an emptied inverse factor (k_prepare_warm).  rho0 [B] or null, as k_refresh takes it.
template <int NCH>
__global__ __launch_bounds__(WG) void k_share_setup(DevBatch db, int mode, const double* rho0)
{
    LCQP_LDS_N(NCH)
    const int b = blockIdx.x, t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const InstInfo* m = db.info;      // the matrix instance's marks; its own workgroup rewrites none of the fields read here
    const int mE = uniform_i(m->mE), cNnz = uniform_i(m->cNnz), fail = uniform_i(m->setupFail), prevFail = uniform_i(m->prevFail);
    const double scale = m->scale, sigma = m->sigma, spv = m->spv;
    c.mE = mE;
    const int warm = mode == 1 && c.info->haveSolution != 0 && db.stats[b].returnValue == 0 && prevFail == 0;      // warm_start, with the setup before this one
    const double rhoStart = warm_penalty<NCH>(db, c, warm, rho0);
    __syncthreads();      // every thread has read the marks thread 0 rewrites below
    const double phiConst = prepare_vectors<NCH>(db, c, lds, scale);
    if (warm) prepare_warm<NCH, true>(db, c, rhoStart);
    else prepare_cold<NCH>(db, c);
    if (t == 0) {
        if (b != 0) {
            c.info->mE = mE; c.info->scale = scale; c.info->sigma = sigma; c.info->spv = spv;
            c.info->cNnz = cNnz; c.info->setupFail = fail; c.info->isSetup = 1;
            c.info->kReady = 0; c.info->rnReady = 0;      // as k_factor leaves them
        }
        c.info->rhoAdmm = db.opt.admmRho * scale;
        c.info->phiConst = phiConst;
    }
}

// ---- the marks of a sensitivity call: `side` of every row in the working set and the flag bits of the instance (include/lcqp_hip.h) -----
// One function for k_sensitivity and k_sensitivity_blk, so that the two kernels cannot disagree about a flag.  sd [nd]: zero on entry (every
// thread's fill may still be in flight: the barrier inside block_max orders it before the marks); sflag: the instance's entry of `info`.
template <int NCH>
__device__ __forceinline__ void sens_marks(const DevBatch& db, Ctx<NCH>& c, Lds lds, int* sd, int* sflag)
{
    const int t = threadIdx.x;
    const int n = db.n, nC = db.nC, nComp = db.nComp, mA = db.mA, mE = c.mE;
    const int *st = c.I(I_ST), *rslot = c.I(I_SLOT), *boxidx = c.boxidx;
    const double* yq = c.M(M_YQ);
    auto pos = [&](int r) { return r < mA ? n + r : boxidx[r - mA]; };      // row of E -> entry of the reference's dual vector
    double ym = 0.0;
    for (int r = t; r < mE; r += WG) ym = fmax(ym, fabs(yq[r]));
    const double ytol = 1e-9 * (1.0 + block_max(ym, lds));      // (the barrier inside also orders the zero fill of `side` before the marks below)
    // a row of L or R at its LOWER bound is a side of its pair; the active side of a pair that is not biactive is an equality of the branch
    auto sideIn = [&](int r) { return rslot[r] >= 0 && st[r] != ST_UPPER; };
    int weak = 0, open = 0;
    for (int r = t; r < mE; r += WG) {
        if (rslot[r] < 0) continue;
        const int s = st[r];
        sd[pos(r)] = (s == ST_EQ) ? 2 : (s == ST_UPPER ? 1 : -1);
        bool ineq = s != ST_EQ;
        if (ineq && r >= nC && r < mA && s != ST_UPPER) ineq = sideIn(r < nC + nComp ? r + nComp : r - nComp);
        if (ineq && fabs(yq[r]) <= ytol) weak = 1;
    }
    for (int i = t; i < nComp; i += WG) if (!sideIn(nC + i) && !sideIn(nC + nComp + i)) open = 1;
    weak = block_or(weak, lds);
    open = block_or(open, lds);
    if (t == 0) *sflag = (uniform_i(c.info->ndep) > 0 ? 2 : 0) | (weak ? 4 : 0) | (open ? 8 : 0);
}

// ---- k_sensitivity: adjoint derivatives of the returned x in g and in the bounds of the working set (DESIGN.md section 3a') -------------
// At the point the last run (or QP solve) returned, x is the minimiser of 1/2 x'Hx + g'x on E_W x = b_W, H = Q + sigma_p I = L1 L1', W the
// rows in the inverse factor.  For an upstream gradient v:  c = L1^-1 v;  lambda = Ti'Ti (Et_W c);  d = L1^-T (c - Et_W' lambda);
// dl/dg = -d, dl/db_W = lambda: one full correction of qp_polish with r1 = v, r2 = 0, from the same routines with the same load policy
// (plain first pass over Et_W, streamed second pass, the triangle of Ti).  The kernel READS the state of the instance and writes only its
// outputs -- no vector pool, InstInfo, status or factor changes, so that a warm re-solve after it returns what it returns without it.
//   v [B][nrhs][n];  dg [B][nrhs][np] (the work vector of the solves; -d on return, zero on the padding);
//   dbo [B][nrhs][nd + capS]: nd derivatives in the reference's dual layout (box first), then capS slot-space scratch (lambda);
//   side [B][nd]: 0 outside W, -1 at lower, +1 at upper, 2 equality;  sinfo [B]: flag bits (include/lcqp_hip.h), 0 = differentiable.
// DUAL (DESIGN.md section 3a'''', lcqp_hip_batch_adjoint): an upstream gradient vy [B][nrhs][nd] on the returned duals, in their layout,
// joins the right-hand side: lambda = Ti'Ti (Et_W c + vy_W), so that E_W d = -vy_W.  Entries of vy outside W are not read.  Without DUAL vy
// is not read at all.
template <int NCH, bool DUAL>
__global__ __launch_bounds__(WG) void k_sensitivity(DevBatch db, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo, const double* vy)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int b = blockIdx.x, t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const int n = db.n, mA = db.mA, nd = db.nd;
    const int ldb = nd + db.capS;
    const int solved = c.info->haveSolution != 0 && c.info->setupFail == 0 && db.stats[b].returnValue == 0;
    int* sd = side + (size_t)b * nd;
    for (int i = t; i < nd; i += WG) sd[i] = 0;
    if (!solved) {      // (uniform) nothing to differentiate: zero outputs
        for (int k = 0; k < nrhs; k++) {
            wg_fill(dg + ((size_t)b * nrhs + k) * np, 0.0, np);
            wg_fill(dbo + ((size_t)b * nrhs + k) * ldb, 0.0, ldb);
        }
        if (t == 0) sinfo[b] = 1;
        return;
    }
    const int nT = uniform_i(c.info->nT), ns = uniform_i(c.info->ns);
    const int nsp = 64 * ((ns + 63) >> 6);
    const int *idx = c.idx, *boxidx = c.boxidx;
    auto pos = [&](int r) { return r < mA ? n + r : boxidx[r - mA]; };      // row of E -> entry of the reference's dual vector
    sens_marks<NCH>(db, c, lds, sd, sinfo + b);
    for (int k = 0; k < nrhs; k++) {
        const double* vk = v + ((size_t)b * nrhs + k) * n;
        double* w = dg + ((size_t)b * nrhs + k) * np;
        double* out = dbo + ((size_t)b * nrhs + k) * ldb;
        double* lam = out + nd;
        for (int i = t; i < np; i += WG) w[i] = (i < n) ? vk[i] : 0.0;
        for (int i = t; i < nd; i += WG) out[i] = 0.0;
        __syncthreads();
        wg_trsv<wg_ncopy(NCH) == 2>(c.F1, np, c.nblk, w, true, lds);
        if (nT > 0) {
            wg_rows<NCH, false, true>(c.Et, idx, ns, w, lam, nullptr, lds, [](int, double) {});
            if constexpr (DUAL) {
                const double* vyk = vy + ((size_t)b * nrhs + k) * nd;
                for (int a = t; a < nsp; a += WG) lam[a] = (a < ns && idx[a] >= 0) ? lam[a] + vyk[pos(idx[a])] : 0.0;
            } else {
                for (int a = t; a < nsp; a += WG) lam[a] = (a < ns && idx[a] >= 0) ? lam[a] : 0.0;
            }
            __syncthreads();
            ti_apply<NCH>(c, lam, lam, nT, ns);
            wg_rows<NCH>(c.Et, idx, ns, nullptr, nullptr, lam, lds, [&](int i, double s) { w[i] = w[i] - s; });
        }
        wg_trsv<wg_ncopy(NCH) == 2>(c.F1, np, c.nblk, w, false, lds);
        for (int i = t; i < np; i += WG) w[i] = (i < n) ? -w[i] : 0.0;
        for (int a = t; a < ns; a += WG) { const int r = idx[a]; if (r >= 0) out[pos(r)] = lam[a]; }
        __syncthreads();
    }
}

// ---- k_sensitivity_blk: the correction of k_sensitivity for SENS_PANEL upstream gradients at once (DESIGN.md section 3a''') ------------
// The vectors of an instance are taken in panels of SENS_PANEL columns (the last one padded with zero columns); the panel X (np x SENS_PANEL)
// lives in LDS from its load to its store, and every product is a chain of v_mfma_f64_16x16x4_f64 on a 64 x 64 block of the matrix, staged in
// LDS, times 64 rows of a panel:
//   C = L1^-1 X        left-looking block forward substitution  C_I = D_II (X_I - sum_{J<I} L_IJ C_J): the blocks below the diagonal of F1, and
//                      the lower triangle of the symmetric-filled inverted diagonal block;
//   S = Et_W C         rows of Et gathered through idx (a free slot or a slot beyond ns is a zero row);
//   U = Ti S, Lambda = Ti' U     the entries (j, s) of Ti with j < nT, s < ns, idx[s] >= 0 and j >= crow[s] -- exactly what ti_apply_fast reads,
//                      one layout whatever ns is (ti_apply's two passes for ns > 256 read the same matrix);
//   C <- C - Et_W' Lambda;   D = L1^-T C   block backward substitution with the blocks above the diagonal (L_JI' as stored) and the upper triangle
//                      of the diagonal block;   dg = -D, db_W = Lambda scattered as k_sensitivity scatters them.
// A column of the result depends on its own column of X only, through the same instructions wherever it stands in a panel: permuting the
// vectors of a call permutes its outputs bit for bit, and a zero column returns zeros.
// Per panel each block of F1 is read once (forward: below the diagonal, backward: above it -- the symmetric fill holds both), each entry of Ti
// and each active row of Et twice (S and U have to be complete before Lambda and the correction can start; the second read follows the first
// within microseconds and is expected to be served by L2 -- that has not been measured).  The slot-space panels S / Lambda and U (at most capS x SENS_PANEL each) stay out of LDS: they live in the slot-space
// scratch behind each vector's row of dbo -- 8 KB per staged block against the 32 KB block of the matrix it multiplies.
// SENS_PANEL = 16, the N of the fp64 MFMA: one accumulator per wave and 64-row block.  LDS: the panel 16 np doubles (64 KB at np = 512), a
// 64 x 66 block of the matrix (33 KB; pitch 66: the plain A-operand reads of a half-wave fall into 64 distinct banks; the transposed reads of
// Lambda = Ti' U and of the correction are 2-way conflicted at this pitch, and the panel load writes X at a stride of 16 doubles once per
// panel -- neither has been measured) and 64 rows of a slot-space panel (8 KB): 57 / 73 / 89 / 105 KB for NCH = 1 .. 4.  174 - 184 VGPRs and 8
// AGPRs (at most 192 unified registers: two waves per SIMD): two workgroups per CU up to np = 256, one above, where LDS is the bound.  The
// product loop is unrolled by four, not fully: sixteen operand pairs in flight cost 278 registers and the second workgroup.  32 columns would
// double the panel and leave np = 512 without room for the matrix block.  (The kernel never runs beside k_lcqp_run.)
//   v [count][nrhs][n], or null: vector k of every instance is the unit vector e_k (the rows of the Jacobian; the block rows of the forward
//   substitution above the panel's first unit entry are zero and are skipped);  dg [count][nrhs][np];  dbo [count][nrhs][nd + 2 capS]: nd
//   derivatives, then S / Lambda and U;  side [count][nd];  sinfo [count].  Workgroup o works on instance first + o and writes row o of the outputs.
constexpr int SENS_PANEL = 16;
constexpr int SENS_PA = 66;

//
// DUAL (DESIGN.md section 3a'''', "Panels with gradients on y"; lcqp_hip_batch_adjoint_blocked / _jacobian_duals): the slot-space right-hand
// side of k_sensitivity<NCH, true> for a panel.  Without DUAL vy, unit and rowpos are not read, and the code is the one above.
//   unit == 0: S <- Et_W C + V_y,W with V_y,W(a, j) = vy[j][pos(idx[a])] on the occupied slots a < ns and zero elsewhere, added where S is
//     stored to the slot-space scratch, before U = Ti S.  vy [count][nrhs][nd] or null.  v == null is a ZERO panel here (not unit vectors):
//     the forward substitution and S = Et_W C are not run at all, S = V_y,W.
//   unit == 1: column j of the call is the unit vector of the j-th occupied slot (idx[s] >= 0, s < ns, in slot order), written straight into
//     S; v and vy are not read, nothing is substituted forward.  The call has min(nrhs, occupied slots) columns (nrhs <= capS staged rows per
//     instance); rowpos [count][capS] receives pos(idx[s(j)]) for every staged row j and -1 behind them: where the row belongs in y.  An
//     instance without a solution gets -1 throughout and no rows.
// A column depends on its own columns of X and V_y only, through the same instructions wherever it stands (the sums over slots and rows run
// in the order of the kernel above whatever the other columns hold).
// Registers: the figures above (174 - 184 VGPRs + 8 AGPRs, at most 192 unified) are those of DUAL = false.  The DUAL build takes 188 / 189 /
// 178 / 185 VGPRs + 8 AGPRs for NCH = 1 .. 4, i.e. 196 / 197 / 186 / 193 unified registers: above 192 at three sizes, without scratch.  That
// costs nothing at run time -- a workgroup is one wave per SIMD, the occupancy steps of two and one workgroups per CU lie at 256 and 512
// registers, and LDS bounds np >= 384 to one workgroup anyway -- but it leaves no headroom: a change that adds registers here should be
// looked at with csrc/resusage.sh.  (The V_y,W pass is a loop of its own and the ranks come from mbcnt for this reason.)
// The body of both kernels (k_sensitivity_blk: DUAL = false; k_sensitivity_blk_dual: DUAL = true, below it).
template <int NCH, bool DUAL>
__device__ __forceinline__ void sensitivity_blk(const DevBatch& db, int first, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo,
                                                const double* vy, int unit, int* rowpos)
{
    constexpr int np = 128 * NCH, P = SENS_PANEL, PA = SENS_PA;
    static_assert(P == 16, "one 16-column MFMA block per wave and row block");
    __shared__ double Xs[np * P];
    __shared__ double As[64 * PA];
    __shared__ double Bs[64 * P];
    __shared__ double sh_red[16];
    __shared__ int sh_ired[16];
    Lds lds{As, sh_red, sh_ired};
    const int o = blockIdx.x, b = first + o, t = tid_here(), lane = t & 63, w = t >> 6, il = lane & 15, kl = lane >> 4;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const int n = db.n, mA = db.mA, nd = db.nd, capS = db.capS, nblk = c.nblk;
    const int ldb = nd + 2 * capS;
    const int solved = c.info->haveSolution != 0 && c.info->setupFail == 0 && db.stats[b].returnValue == 0;
    int* sd = side + (size_t)o * nd;
    for (int i = t; i < nd; i += WG) sd[i] = 0;
    if (!solved) {      // (uniform) nothing to differentiate: zero outputs
        const bool rowsOnly = DUAL && unit;      // (the staged rows of a dual Jacobian are read through rowpos only)
        for (int k = 0; k < nrhs && !rowsOnly; k++) {
            wg_fill(dg + ((size_t)o * nrhs + k) * np, 0.0, np);
            wg_fill(dbo + ((size_t)o * nrhs + k) * ldb, 0.0, ldb);
        }
        if constexpr (DUAL) { if (unit) for (int j = t; j < capS; j += WG) rowpos[(size_t)o * capS + j] = -1; }
        if (t == 0) sinfo[o] = 1;
        return;
    }
    const int nT = uniform_i(c.info->nT), ns = uniform_i(c.info->ns);
    const int nsb = (ns + 63) >> 6, njb = (nT + 63) >> 6;      // 64 nsb, 64 njb <= capS: ns, nT <= capS, a multiple of 64
    const int *idx = c.idx, *boxidx = c.boxidx, *crow = c.crow;
    const double *F1 = c.F1, *Et = c.Et, *Ti = c.S;
    auto pos = [&](int r) { return r < mA ? n + r : boxidx[r - mA]; };
    sens_marks<NCH>(db, c, lds, sd, sinfo + o);
    // (DUAL, unit) the occupied slots in slot order: wave 0 calls f(a, rank) for the rank-th occupied slot a; every wave returns their number
    auto occupied = [&](auto f) {
        int cnt = 0;
        for (int a0 = 0; a0 < ns; a0 += 64) {
            const int a = a0 + lane;
            const bool occ = a < ns && idx[a] >= 0;
            const unsigned long long m = __ballot(occ);
            // (mbcnt: the occupied lanes below this one, without a lane mask that would stay in registers over the product loops)
            if (occ && w == 0) f(a, cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)));
            cnt += __popcll(m);
        }
        return cnt;
    };
    int ncols = nrhs;
    if constexpr (DUAL) {
        if (unit) {
            int* rp = rowpos + (size_t)o * capS;
            const int nocc = occupied([&](int a, int rank) { rp[rank] = rank < nrhs ? pos(idx[a]) : -1; });
            ncols = min(nrhs, nocc);
            for (int j = nocc + t; j < capS; j += WG) rp[j] = -1;
        }
    }

    // a 64 x 64 block of a matrix on its way into As: thread t carries the column pair 2 (t & 31) of the rows (t >> 5) + 8 i
    const int ar = t >> 5, ac = (t & 31) * 2;
    double2 ra[8];
    double rb[4];
    // rowp(r): where row r of the block starts (its 64 columns), or null for a zero row; keep(r, col): whether an entry takes part
    auto loadA = [&](auto rowp, auto keep) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int r = ar + 8 * i;
            const double* p = rowp(r);
            double2 x{0.0, 0.0};
            if (p) x = *reinterpret_cast<const double2*>(p + ac);
            if (!keep(r, ac)) x.x = 0.0;
            if (!keep(r, ac + 1)) x.y = 0.0;
            ra[i] = x;
        }
    };
    auto storeA = [&]() {
#pragma unroll
        for (int i = 0; i < 8; i++) *reinterpret_cast<double2*>(As + (ar + 8 * i) * PA + ac) = ra[i];
    };
    auto all = [](int, int) { return true; };
    // acc += (As or its transpose)[rows 16 w .. 16 w + 15] * Bp (64 x P, pitch P)
    auto mm = [&](d4_t& acc, const double* Bp, bool tr) {
#pragma unroll 4
        for (int k4 = 0; k4 < 16; k4++) {
            const int k = 4 * k4 + kl;
            const double av = tr ? As[k * PA + 16 * w + il] : As[(16 * w + il) * PA + k];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bp[k * P + il], acc, 0, 0, 0);
        }
    };

    #pragma nounroll
    for (int k0 = 0; k0 < ncols; k0 += P) {
        const int pv = min(P, ncols - k0);      // columns of this panel that are vectors of the call
        const size_t row0 = (size_t)o * nrhs + k0;
        // entry (a, j) of the slot-space panels: S, then Lambda, at offset nd of vector j's row of dbo; U at nd + capS
        auto slotp = [&](int which, int a, int j) -> double* { return dbo + (row0 + j) * ldb + nd + which * capS + a; };
        // 64 rows of a slot-space panel on their way into Bs: rb[m] is entry (a0 + (e & 63), e >> 6) for e = t + 256 m; padded columns are zero
        auto loadB = [&](int which, int a0) {
#pragma unroll
            for (int m = 0; m < 4; m++) { const int e = t + WG * m, j = e >> 6; rb[m] = (j < pv) ? *slotp(which, a0 + (e & 63), j) : 0.0; }
        };
        auto storeB = [&]() {
#pragma unroll
            for (int m = 0; m < 4; m++) { const int e = t + WG * m; Bs[(e & 63) * P + (e >> 6)] = rb[m]; }
        };
        // accumulator register q of a wave is row 16 w + kl + 4 q of the block, column il
        auto storeSlot = [&](int which, int a0, const d4_t& acc) {
            if (il < pv) {
#pragma unroll
                for (int q = 0; q < 4; q++) *slotp(which, a0 + 16 * w + kl + 4 * q, il) = acc[q];
            }
        };
        const int skip = (DUAL || v) ? 0 : (k0 >> 6);      // unit vectors: the block rows above the first unit entry stay zero in the forward substitution
        for (int e = t; e < np * P; e += WG) {
            const int j = e / np, i = e - j * np;
            double x = 0.0;
            if constexpr (DUAL) { if (v && i < n && j < pv) x = v[(row0 + j) * n + i]; }
            else if (i < n && j < pv) x = v ? v[(row0 + j) * n + i] : (i == k0 + j ? 1.0 : 0.0);
            Xs[i * P + j] = x;
        }
        for (int j = 0; j < pv; j++) wg_fill(dbo + (row0 + j) * ldb, 0.0, nd);
        __syncthreads();

        // X <- L1^-1 X (forward) or L1^-T X (backward): block (I, J) of the symmetric-filled F1 is L_IJ below the diagonal and L_JI' above it
        auto trisolve = [&](bool fwd) {
            #pragma nounroll
            for (int s = (fwd ? skip : 0); s < nblk; s++) {
                const int I = fwd ? s : nblk - 1 - s;
                const int J0 = fwd ? skip : I + 1, J1 = fwd ? I : nblk;
                auto blk = [&](int J) { return [=](int r) { return F1 + (size_t)(64 * I + r) * np + 64 * J; }; };
                d4_t acc{0.0, 0.0, 0.0, 0.0};
                if (J1 > J0) loadA(blk(J0), all);
                #pragma nounroll
                for (int J = J0; J < J1; J++) {
                    storeA();
                    __syncthreads();
                    if (J + 1 < J1) loadA(blk(J + 1), all);
                    mm(acc, Xs + 64 * J * P, false);
                    __syncthreads();
                }
                // the diagonal block holds D = inv(L_II) below and D' above: forward applies D (entries c <= r), backward D' (c >= r)
                if (fwd) loadA(blk(I), [](int r, int cc) { return cc <= r; });
                else loadA(blk(I), [](int r, int cc) { return cc >= r; });
#pragma unroll
                for (int q = 0; q < 4; q++) Xs[(64 * I + 16 * w + kl + 4 * q) * P + il] -= acc[q];
                storeA();
                __syncthreads();
                d4_t y{0.0, 0.0, 0.0, 0.0};
                mm(y, Xs + 64 * I * P, false);
                __syncthreads();      // every wave has read X_I
#pragma unroll
                for (int q = 0; q < 4; q++) Xs[(64 * I + 16 * w + kl + 4 * q) * P + il] = y[q];
                __syncthreads();
            }
        };
        if (!DUAL || v) trisolve(true);      // (DUAL without X: C = 0, nothing to substitute)
        if (nT > 0) {
            // rows of Et held by the slots 64 sb .. 64 sb + 63, columns 64 J .. 64 J + 63
            auto etBlk = [&](int sb, int J) {
                return [=](int r) -> const double* {
                    const int a = 64 * sb + r;
                    const int row = (a < ns) ? idx[a] : -1;
                    return row >= 0 ? Et + (size_t)row * np + 64 * J : nullptr;
                };
            };
            // rows 64 jb .. of Ti, slots 64 sb ..: column s is zero above crow[s], and everywhere on a free slot
            auto tiBlk = [&](int jb, int sb) { return [=](int r) -> const double* { return (64 * jb + r < nT) ? Ti + (size_t)(64 * jb + r) * capS + 64 * sb : nullptr; }; };
            auto tiKeep = [&](int jb, int sb) {
                return [=](int r, int cc) { const int s = 64 * sb + cc; return s < ns && idx[s] >= 0 && 64 * jb + r >= crow[s]; };
            };
            // S = Et_W C
            #pragma nounroll
            for (int sb = 0; sb < ((!DUAL || v) ? nsb : 0); sb++) {
                d4_t acc{0.0, 0.0, 0.0, 0.0};
                loadA(etBlk(sb, 0), all);
                #pragma nounroll
                for (int J = 0; J < nblk; J++) {
                    storeA();
                    __syncthreads();
                    if (J + 1 < nblk) loadA(etBlk(sb, J + 1), all);
                    mm(acc, Xs + 64 * J * P, false);
                    __syncthreads();
                }
                storeSlot(0, 64 * sb, acc);
            }
            if constexpr (DUAL) {
                // S <- S + V_y,W in the scratch, before U = Ti S reads it (a pass of its own over at most capS x 16 entries: the addresses of vy
                // stay out of the product loops' registers).  No X: S is V_y,W itself, or the unit vectors of the occupied slots k0 .. k0 + pv - 1.
                if (!v || vy) {
                    if (v) __syncthreads();
                    const int rows = 64 * nsb;
                    for (int e = t; e < rows * pv; e += WG) {
                        const int j = e / rows, a = e - j * rows;
                        const int r = (!unit && vy && a < ns) ? idx[a] : -1;
                        double s = v ? *slotp(0, a, j) : 0.0;
                        if (r >= 0) s += vy[(row0 + j) * nd + pos(r)];
                        *slotp(0, a, j) = s;
                    }
                    if (unit) {
                        __syncthreads();
                        occupied([&](int a, int rank) { if (rank >= k0 && rank < k0 + pv) *slotp(0, a, rank - k0) = 1.0; });
                    }
                }
            }
            __syncthreads();
            // U = Ti S
            #pragma nounroll
            for (int jb = 0; jb < njb; jb++) {
                d4_t acc{0.0, 0.0, 0.0, 0.0};
                loadA(tiBlk(jb, 0), tiKeep(jb, 0));
                loadB(0, 0);
                #pragma nounroll
                for (int sb = 0; sb < nsb; sb++) {
                    storeA();
                    storeB();
                    __syncthreads();
                    if (sb + 1 < nsb) { loadA(tiBlk(jb, sb + 1), tiKeep(jb, sb + 1)); loadB(0, 64 * (sb + 1)); }
                    mm(acc, Bs, false);
                    __syncthreads();
                }
                storeSlot(1, 64 * jb, acc);
            }
            __syncthreads();
            // Lambda = Ti' U, in the place of S
            #pragma nounroll
            for (int sb = 0; sb < nsb; sb++) {
                d4_t acc{0.0, 0.0, 0.0, 0.0};
                loadA(tiBlk(0, sb), tiKeep(0, sb));
                loadB(1, 0);
                #pragma nounroll
                for (int jb = 0; jb < njb; jb++) {
                    storeA();
                    storeB();
                    __syncthreads();
                    if (jb + 1 < njb) { loadA(tiBlk(jb + 1, sb), tiKeep(jb + 1, sb)); loadB(1, 64 * (jb + 1)); }
                    mm(acc, Bs, true);
                    __syncthreads();
                }
                storeSlot(0, 64 * sb, acc);
            }
            __syncthreads();
            // C <- C - Et_W' Lambda
            #pragma nounroll
            for (int J = 0; J < nblk; J++) {
                d4_t acc{0.0, 0.0, 0.0, 0.0};
                loadA(etBlk(0, J), all);
                loadB(0, 0);
                #pragma nounroll
                for (int sb = 0; sb < nsb; sb++) {
                    storeA();
                    storeB();
                    __syncthreads();
                    if (sb + 1 < nsb) { loadA(etBlk(sb + 1, J), all); loadB(0, 64 * (sb + 1)); }
                    mm(acc, Bs, true);
                    __syncthreads();
                }
#pragma unroll
                for (int q = 0; q < 4; q++) Xs[(64 * J + 16 * w + kl + 4 * q) * P + il] -= acc[q];
            }
            __syncthreads();
        }
        trisolve(false);
        for (int e = t; e < np * pv; e += WG) {
            const int j = e / np, i = e - j * np;
            dg[(row0 + j) * np + i] = (i < n) ? -Xs[i * P + j] : 0.0;
        }
        if (nT > 0)
            for (int e = t; e < ns * pv; e += WG) {
                const int j = e / ns, a = e - j * ns;
                const int r = idx[a];
                if (r >= 0) dbo[(row0 + j) * ldb + pos(r)] = *slotp(0, a, j);
            }
        __syncthreads();
    }
}

template <int NCH>
__global__ __launch_bounds__(WG) void k_sensitivity_blk(DevBatch db, int first, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo)
{
    sensitivity_blk<NCH, false>(db, first, nrhs, v, dg, dbo, side, sinfo, nullptr, 0, nullptr);
}

template <int NCH>
__global__ __launch_bounds__(WG) void k_sensitivity_blk_dual(DevBatch db, int first, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo,
                            const double* vy, int unit, int* rowpos)
{
    sensitivity_blk<NCH, true>(db, first, nrhs, v, dg, dbo, side, sinfo, vy, unit, rowpos);
}

// ---- k_build_C: C = L'R + R'L (Utilities::MatrixSymmetrizationProduct, src/Utilities.cpp:104-116) ----
// One 64 x 64 tile of the lower triangle per workgroup.  Both products advance in the same loop (four panels of 16 rows of L and R per step:
// half the steps, barriers and exposed loads of two products one after the other), and the mirrored tile goes through LDS so that its rows
// are stored contiguously (rounds 1 - 5: every lane its own 8 bytes at a stride of a row).  Each sum is the same chain as before.
template <int NCH>
__global__ __launch_bounds__(WG, 4) void k_build_C(DevBatch db)      // 128 registers: a workgroup fits where one instance of k_lcqp_run has finished
{
    constexpr int np = 128 * NCH, PL = TILE_PL;
    __shared__ double sP[4 * 16 * PL];      // panels of L_I, R_I, L_J, R_J; afterwards the tile for the mirrored store (64 x 65)
    static_assert(4 * 16 * PL >= 64 * 65, "the tile must fit where the panels were");
    const int ntile = db.nblk * (db.nblk + 1) / 2;
    const int bid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int b = bid / ntile, tIdx = bid % ntile;
    int I, J;
    tri_tile(tIdx, I, J);
    const double* Lm = db.E + (size_t)b * db.mEcap * np + (size_t)db.nC * np;
    const double* Rm = Lm + (size_t)db.nComp * np;
    double* C = db.C + (size_t)b * np * np;
    const int nrows = db.nComp;
    const int t = tid_here(), kk = t >> 4, c4 = (t & 15) * 4;
    double a1[4][4], a2[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) a1[i][j] = a2[i][j] = 0.0;
    double2 p[4][2];
    auto fetch = [&](int r) {
        const double2 z{0.0, 0.0};
#pragma unroll
        for (int m = 0; m < 4; m++) p[m][0] = p[m][1] = z;
        if (r < nrows) {
            const double* src[4] = {Lm + (size_t)r * np + 64 * I + c4, Rm + (size_t)r * np + 64 * I + c4,
                                    Lm + (size_t)r * np + 64 * J + c4, Rm + (size_t)r * np + 64 * J + c4};
#pragma unroll
            for (int m = 0; m < 4; m++) { p[m][0] = *reinterpret_cast<const double2*>(src[m]); p[m][1] = *reinterpret_cast<const double2*>(src[m] + 2); }
        }
    };
    fetch(kk);
    for (int k0 = 0; k0 < nrows; k0 += 16) {
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; m++) {
            *reinterpret_cast<double2*>(sP + m * 16 * PL + kk * PL + c4) = p[m][0];
            *reinterpret_cast<double2*>(sP + m * 16 * PL + kk * PL + c4 + 2) = p[m][1];
        }
        __syncthreads();
        if (k0 + 16 < nrows) fetch(k0 + 16 + kk);
        tile_panel(a1, sP, sP + 3 * 16 * PL);                    // L_I' R_J
        tile_panel(a2, sP + 16 * PL, sP + 2 * 16 * PL);          // R_I' L_J
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int li = tile_li(i, j), lj = tile_lj(i, j);
            const double v = a1[i][j] + a2[i][j];
            C[(size_t)(64 * I + li) * np + 64 * J + lj] = v;
            if (I != J) sP[li * 65 + lj] = v;
        }
    if (I == J) return;      // the tile on the diagonal is its own mirror image, entry by entry
    __syncthreads();
    for (int e = t; e < 64 * 64; e += WG) {
        const int r = e >> 6, cidx = e & 63;
        C[(size_t)(64 * J + r) * np + 64 * I + cidx] = sP[cidx * 65 + r];
    }
}

// ---- k_compress_C: C in compressed rows when it is sparse (one-hot L, R give 2 nComp non-zeros) ------------------------------------
// The homotopy applies C to one vector per iterate; from compressed rows that costs 12 bytes per non-zero instead of a sweep over
// np x np doubles.  More than capC non-zeros: cNnz = -1 and C stays a dense sweep.
template <int NCH>
__global__ __launch_bounds__(WG) void k_compress_C(DevBatch db)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int b = blockIdx.x, t = threadIdx.x, l = lane_id(), w = wave_id();
    const double* C = db.C + (size_t)b * np * np;
    int* cp = db.Cp + (size_t)b * (np + 1);
    int* ci = db.Ci + (size_t)b * db.capC;
    double* cv = db.Cv + (size_t)b * db.capC;
    int* cnt = reinterpret_cast<int*>(lds.arena);        // np row counts, then row starts
    const int n = db.n;
    // (up to eight loads of a row, and two rows per wave, are in flight together: a wave that waited for every load by itself made this kernel
    // 0.49 ms of dependent round trips at B = 1024; np is a multiple of 2 NWAVE)
    constexpr int NC = (np / 64 < 8) ? np / 64 : 8;
    for (int r = w; r < np; r += 2 * NWAVE) {
        const int r2 = r + NWAVE;
        int k1 = 0, k2 = 0;
        for (int c0 = 0; c0 < np; c0 += 64 * NC) {
            double v1[NC], v2[NC];
#pragma unroll
            for (int q = 0; q < NC; q++) {
                v1[q] = (r < n) ? C[(size_t)r * np + c0 + 64 * q + l] : 0.0;
                v2[q] = (r2 < n) ? C[(size_t)r2 * np + c0 + 64 * q + l] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < NC; q++) { k1 += __popcll(__ballot(v1[q] != 0.0)); k2 += __popcll(__ballot(v2[q] != 0.0)); }
        }
        if (l == 0) { cnt[r] = k1; cnt[r2] = k2; }
    }
    __syncthreads();
    {   // exclusive scan of the np counts: each thread a contiguous chunk
        constexpr int per = (np + WG - 1) / WG;
        const int r0 = t * per;
        int loc = 0;
        for (int q = 0; q < per; q++) if (r0 + q < np) loc += cnt[r0 + q];
        int incl = loc;
#pragma unroll
        for (int ofs = 1; ofs < 64; ofs <<= 1) { const int v = __shfl_up(incl, ofs, 64); if (l >= ofs) incl += v; }
        if (l == 63) lds.ired[8 + w] = incl;
        __syncthreads();
        int run = incl - loc;
        for (int ww = 0; ww < w; ww++) run += lds.ired[8 + ww];
        const int total = lds.ired[8] + lds.ired[9] + lds.ired[10] + lds.ired[11];
        __syncthreads();
        for (int q = 0; q < per; q++) if (r0 + q < np) { const int k = cnt[r0 + q]; cnt[r0 + q] = run; run += k; }
        __syncthreads();
        if (total > db.capC) { if (t == 0) db.info[b].cNnz = -1; return; }
        if (t == 0) { db.info[b].cNnz = total; cp[np] = total; }
    }
    for (int r = w; r < np; r += 2 * NWAVE) {
        const int r2 = r + NWAVE;
        int pos1 = cnt[r], pos2 = cnt[r2];
        if (l == 0) { cp[r] = pos1; cp[r2] = pos2; }
        for (int c0 = 0; c0 < np; c0 += 64 * NC) {
            double v1[NC], v2[NC];
#pragma unroll
            for (int q = 0; q < NC; q++) {
                v1[q] = (r < n) ? C[(size_t)r * np + c0 + 64 * q + l] : 0.0;
                v2[q] = (r2 < n) ? C[(size_t)r2 * np + c0 + 64 * q + l] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < NC; q++) {
                const unsigned long long m1 = __ballot(v1[q] != 0.0), m2 = __ballot(v2[q] != 0.0), below = (1ULL << l) - 1ULL;
                if (v1[q] != 0.0) { const int o = pos1 + __popcll(m1 & below); ci[o] = c0 + 64 * q + l; cv[o] = v1[q]; }
                if (v2[q] != 0.0) { const int o = pos2 + __popcll(m2 & below); ci[o] = c0 + 64 * q + l; cv[o] = v2[q]; }
                pos1 += __popcll(m1); pos2 += __popcll(m2);
            }
        }
    }
}

// ---- k_factor: the constant factorisation L1 of Q + sp I (L_K of the ADMM fallback is built on demand, qp_build_K) ----
// One workgroup per instance; its life is chains (16 x 16 sub-block factorisations, dependent tiles): ~0.35 ms alone, ~0.7 ms with four per CU.
// Round 6: profiles/round6/factor_phases*.log -- with 138 registers only three workgroups per CU were resident and the default batch took two
// rounds (a quarter of the workgroups started 0.6 ms late); the copy F1 = Q + sp I in front of the factorisation was 15 % of a workgroup's life.
// MINW = 4 holds the kernel to 128 registers: four workgroups per CU, a batch of more than three workgroups per CU in one residency round
// (-0.12 ms at B = 1024); MINW = 1 (138 registers) is 0.09 ms faster for one workgroup alone -- the launcher picks by the size of the batch.
template <int NCH, int MINW>
__global__ __launch_bounds__(WG, MINW) void k_factor(DevBatch db)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int b = blockIdx.x, t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const double scale = c.info->scale;
    __shared__ int sfail;
    int failed = 0;
    double spv = 0.0;
#ifdef LCQP_FACTOR_PROFILE
    unsigned long long fpv[16];
    for (int k = 0; k < 16; k++) fpv[k] = 0;
    fpv[15] = fpv[14] = clock64();
    fpv[13] = wall_clock64();
    unsigned long long* fp = fpv;
#else
    unsigned long long* fp = nullptr;
#endif
    for (int pass = 0; pass < 2; pass++) {
        spv = (pass == 0 ? db.opt.proxSmall : db.opt.proxBig) * scale;
        if (t == 0) sfail = 0;
        __syncthreads();
        FPROF(7);
        // D1 keeps every inverted diagonal block (dense lower) for the TRSM that forms Et
        double minpiv = INFINITY;
        {
            // factor block column by block column so each D block lands in its own slot of D1
            minpiv = wg_chol(c.F1, np, c.nblk, c.n, 0.0, c.D1, nullptr, &sfail, lds, 4096, fp, c.Q, spv);      // F1 = chol(Q + spv I), Q read in place
        }
        __syncthreads();
        failed = sfail;
        __syncthreads();   // every thread has read the flag before thread 0 of the retry pass clears it
        if (!failed && (pass == 1 || minpiv >= db.opt.pivotThreshold * scale)) break;
        if (pass == 1) break;
    }
    if (t == 0) {
        c.info->spv = spv;
        c.info->kReady = 0;          // L_K (ADMM fallback) is built by the first instance that needs it: qp_build_K
        c.info->rnReady = 0;         // row norms of E for the row screening of the residual sweeps: first sweep
        if (failed) c.info->setupFail = 3;
#ifdef LCQP_FACTOR_PROFILE
        fpv[8] = clock64() - fpv[14];      // the whole kernel as this workgroup saw it
        for (int k = 0; k < 9; k++) db.prof[(size_t)b * 16 + k] = fpv[k];
        db.prof[(size_t)b * 16 + 9] = wall_clock64();      // 100 MHz, the same counter on every XCD: when did this workgroup end
        db.prof[(size_t)b * 16 + 10] = fpv[13];            // and start
#endif
    }
}

// ---- k_trsm: Et = E L1^-T, 64 rows of E per workgroup ----------------------------------------------
// Block column J of the result is  Et_J = (E_J - sum_{K<J} Et_K L_JK') D_J'  (D_J: the inverted diagonal block of L1 from k_factor).
//
// trsm_rows_resident (np <= 256): the sums of ALL block columns still to come live in registers (wave w: rows 16w..16w+15, 16 doubles per lane
// and block column), and the block column just finished is the A operand of the products out of a wave-private LDS region -- so E is read
// once, Et written once, and only the blocks of L1 / D1 stream through the workgroup (two 16-deep panels in LDS, one barrier per panel).
// Before (rounds 1 - 5, still the form of the larger sizes below): block column J re-read Et_0..J-1 from memory and wrote Et_J twice:
// 10 GB of traffic per launch of the default workload for 3.2 GB of operands (pmc_fetch_size / pmc_write_size), 1.69 ms at 6 TB/s.
// Every element is the same chain of v_mfma_f64_16x16x4 (k ascending, four per instruction, from zero), so the bits are the same.
template <int NCH>
__device__ __forceinline__ void trsm_rows_resident(const DevBatch& db)
{
    constexpr int np = 128 * NCH, NB = 2 * NCH, PL = TILE_PL;
    __shared__ double sA[NWAVE * 1024];      // per wave: 64 k x 16 rows, entry (k, r) at 16 k + (r ^ swz(k)): conflict-free C-layout writes and A-operand reads
    __shared__ double sB[2][16 * PL];
    const int nrb = (db.mEcap + 63) / 64;
    const int bid = xcd_contiguous(blockIdx.x, gridDim.x);      // the row blocks of an instance share L1 and D1: one L2
    const int b = bid / nrb, rb = bid % nrb;
    if (64 * rb >= db.info[b].mE) return;
    const double* E = db.E + (size_t)b * db.mEcap * np + (size_t)(64 * rb) * np;
    double* Et = db.Et + (size_t)b * db.mEcap * np + (size_t)(64 * rb) * np;
    const double* F1 = db.F1 + (size_t)b * np * np;
    const double* D1 = db.D1 + (size_t)b * db.nblk * 4096;
    const int rows = min(64, db.mEcap - 64 * rb);
    const int t = tid_here(), lane = t & 63, w = t >> 6, il = lane & 15, kl = lane >> 4;
    double* A = sA + 1024 * w;
    auto swz = [](int k) { return ((k >> 1) & 7) << 1; };
    const int lr = t >> 2, kq = (t & 3) * 4;      // loader of the B panels: row lr of the block, four consecutive k
    // panel q (16 k) of block `blk` of column J: blk 0 is D_J, blk i > 0 is L_{J+i, J}
    auto src = [&](int J, int blk, int q) -> const double* {
        return blk == 0 ? D1 + (size_t)J * 4096 + lr * 64 + 16 * q + kq
                        : F1 + (size_t)(64 * (J + blk) + lr) * np + 64 * J + 16 * q + kq;
    };
    double2 r0, r1;
    auto fetch = [&](const double* p) { r0 = *reinterpret_cast<const double2*>(p); r1 = *reinterpret_cast<const double2*>(p + 2); };
    auto commit = [&](int buf) {
        double* Bs = sB[buf];
        Bs[(kq + 0) * PL + lr] = r0.x; Bs[(kq + 1) * PL + lr] = r0.y; Bs[(kq + 2) * PL + lr] = r1.x; Bs[(kq + 3) * PL + lr] = r1.y;
    };
    // C layout of this wave's 16 x 64 block: x[a][q] is row (lane >> 4) + 4 q, column 16 a + (lane & 15)
    auto loadE = [&](d4_t (&x)[4], int J) {
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int li = 16 * w + kl + 4 * q;
                x[a][q] = (li < rows) ? E[(size_t)li * np + 64 * J + 16 * a + il] : 0.0;
            }
    };
    auto toA = [&](const d4_t (&x)[4]) {
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int q = 0; q < 4; q++) { const int k = 16 * a + il, r = kl + 4 * q; A[16 * k + (r ^ swz(k))] = x[a][q]; }
    };
    d4_t acc[NB][4];      // acc[I]: sum_{K<J} Et_K L_IK' of the block columns I > J still to come
#pragma unroll
    for (int I = 0; I < NB; I++)
#pragma unroll
        for (int a = 0; a < 4; a++) acc[I][a] = d4_t{0.0, 0.0, 0.0, 0.0};
    d4_t cur[4];
    fetch(src(0, 0, 0));
    loadE(cur, 0);
    commit(0);
    fetch(src(0, 0, 1));
    toA(cur);
    __syncthreads();
    int pc = 0;
#pragma unroll
    for (int J = 0; J < NB; J++) {
#pragma unroll
        for (int blk = 0; blk < NB - J; blk++) {
            if (blk == 0) {
#pragma unroll
                for (int a = 0; a < 4; a++) cur[a] = d4_t{0.0, 0.0, 0.0, 0.0};
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double* Bs = sB[pc & 1];
#pragma unroll
                for (int k4 = 0; k4 < 4; k4++) {
                    const int k = 16 * q + 4 * k4 + kl;
                    const double av = A[16 * k + (il ^ swz(k))];
#pragma unroll
                    for (int a = 0; a < 4; a++) {
                        const double bv = Bs[(4 * k4 + kl) * PL + 16 * a + il];
                        if (blk == 0) cur[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, cur[a], 0, 0, 0);
                        else acc[J + blk][a] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[J + blk][a], 0, 0, 0);
                    }
                }
                // the successors of this panel in the order of the loops
                int J1 = J, b1 = blk, q1 = q + 1;
                if (q1 == 4) { q1 = 0; b1++; if (b1 == NB - J1) { b1 = 0; J1++; } }
                if (J1 < NB) {
                    commit((pc + 1) & 1);
                    int J2 = J1, b2 = b1, q2 = q1 + 1;
                    if (q2 == 4) { q2 = 0; b2++; if (b2 == NB - J2) { b2 = 0; J2++; } }
                    if (J2 < NB) fetch(src(J2, b2, q2));
                }
                __syncthreads();
                pc++;
            }
            if (blk == 0) {
                // cur = Et_J: to memory, and in place of E_J - sum as the A operand of the products with the blocks of L1 below D_J
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int li = 16 * w + kl + 4 * q;
                        if (li < rows) Et[(size_t)li * np + 64 * J + 16 * a + il] = cur[a][q];
                    }
                toA(cur);
                if (J + 1 < NB) loadE(cur, J + 1);      // on its way while the products of this block column run
            }
        }
        if (J + 1 < NB) {
#pragma unroll
            for (int a = 0; a < 4; a++) cur[a] = cur[a] - acc[J + 1][a];
            toA(cur);
        }
    }
}

template <int NCH>
__device__ __forceinline__ void trsm_rows_streamed(const DevBatch& db)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int nrb = (db.mEcap + 63) / 64;
    const int bid = xcd_contiguous(blockIdx.x, gridDim.x);      // the row blocks of an instance share L1 and D1: one L2
    const int b = bid / nrb, rb = bid % nrb;
    const InstInfo* info = db.info + b;
    if (64 * rb >= info->mE) return;
    const double* E = db.E + (size_t)b * db.mEcap * np + (size_t)(64 * rb) * np;
    double* Et = db.Et + (size_t)b * db.mEcap * np + (size_t)(64 * rb) * np;
    const double* F1 = db.F1 + (size_t)b * np * np;
    const double* D1 = db.D1 + (size_t)b * db.nblk * 4096;
    const int rows = min(64, db.mEcap - 64 * rb);
    auto rowok = [=](int r) { return (long)(r < rows ? r : -1); };
    auto ident = [](int r) { return (long)r; };
    for (int J = 0; J < db.nblk; J++) {
        double acc[4][4];
        if (J > 0) wg_tile_nt(acc, Et, np, rowok, F1 + (size_t)(64 * J) * np, np, ident, 64 * J, lds);
        else {
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int li = tile_li(i, j), gj = 64 * J + tile_lj(i, j);
                if (li < rows) Et[(size_t)li * np + gj] = E[(size_t)li * np + gj] - acc[i][j];
            }
        __syncthreads();
        double acc2[4][4];
        wg_tile_nt(acc2, Et + 64 * J, np, rowok, D1 + (size_t)J * 4096, 64, ident, 64, lds);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int li = tile_li(i, j), gj = 64 * J + tile_lj(i, j);
                if (li < rows) Et[(size_t)li * np + gj] = acc2[i][j];
            }
        __syncthreads();
    }
}

// 207 registers, two waves per SIMD (held to 168 -- three waves -- the kernel spills 32 registers and the setup is 0.17 ms slower)
template <int NCH>
__global__ __launch_bounds__(WG) void k_trsm(DevBatch db)
{
    if constexpr (NCH <= 2) trsm_rows_resident<NCH>(db);
    else trsm_rows_streamed<NCH>(db);
}

// the streamed form for every size: 52 registers and 36 KB of LDS, a workgroup fits where ONE instance of k_lcqp_run has finished
// (lcqp_hip_batch_set_overlapped)
template <int NCH>
__global__ __launch_bounds__(WG) void k_trsm_streamed(DevBatch db) { trsm_rows_streamed<NCH>(db); }

// ---- k_build_M: M = Et Et', every entry of every working-set matrix S_W = Et_W Et_W' (lower triangle; readers take M[max][min]) ----
// fp64 MFMA.  Tiles of 128 rows x 64 columns (round 6; rounds 3 - 5: 128 x 128 with a 64 x 64 quadrant per wave -- 128 accumulator registers of
// 226, two waves per SIMD, the matrix pipe busy 62 % of the time): the four waves own 64 x 32 blocks as 4 x 2 blocks of v_mfma_f64_16x16x4_f64,
// 64 accumulator registers, so that three to four workgroups share a CU and another wave has products to issue while one waits at a barrier.  One
// 16-deep panel pair in LDS (k-major, pitches 144 / 80 doubles: conflict-free operand reads); the panels of step k + 16 are fetched into registers
// while the products of step k run.  Column blocks inside the row block (the tiles on the diagonal) take their operand from the row panel.
// Every element is the same chain of instructions as before (k ascending, four per instruction, from zero): the bits are the same.
// Tile t of an instance: row block I (128 rows), column block J (64 columns), J <= 2 I + 1; tiles are numbered row block by row block.
template <int NCH>
__global__ __launch_bounds__(WG, 4) void k_build_M(DevBatch db)
{
    constexpr int np = 128 * NCH;
    constexpr int PA = 144, PB = 80;
    __shared__ double As[16 * PA], Bs[16 * PB];
    const int nb = (db.mMld + 127) / 128, ntile = nb * (nb + 1);
    const int bid = xcd_contiguous(blockIdx.x, gridDim.x);      // the tiles of an instance read the same Et (1.3 MB): one L2
    const int b = bid / ntile, tIdx = bid % ntile;
    int I = 0;
    while ((I + 1) * (I + 2) <= tIdx) I++;
    const int J = tIdx - I * (I + 1);
    const int mE = db.info[b].mE, ld = db.mMld;
    if (128 * (J >> 1) >= mE || 64 * J >= ld) return;       // a block of 128 columns beyond the rows in use (then the rows are too)
    const double* Et = db.Et + (size_t)b * db.mEcap * np;
    double* M = db.MM + (size_t)b * ld * ld;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wy = w >> 1, wx = w & 1;
    const int lr = t >> 1, kh = (t & 1) * 8;      // loader of the row panel: row lr of the tile, eight consecutive k
    const int lc = t >> 2, kq = (t & 3) * 4;      // loader of the column panel: row lc of the column block, four consecutive k
    const bool inside = (J >> 1) == I;            // the column block is part of the row block
    const double* ap = (128 * I + lr < mE) ? Et + (size_t)(128 * I + lr) * np + kh : nullptr;
    const double* bp = (!inside && 64 * J + lc < mE) ? Et + (size_t)(64 * J + lc) * np + kq : nullptr;
    d4_t acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    double2 ra[4], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; q++) ra[q] = ap ? *reinterpret_cast<const double2*>(ap + k0 + 2 * q) : double2{0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 2; q++) rb[q] = bp ? *reinterpret_cast<const double2*>(bp + k0 + 2 * q) : double2{0.0, 0.0};
    };
    fetch(0);
    const double* Bsrc = inside ? As + 64 * (J & 1) : Bs;
    const int PBs = inside ? PA : PB;
    for (int k0 = 0; k0 < np; k0 += 16) {
        __syncthreads();      // the panels of the last step are consumed
#pragma unroll
        for (int q = 0; q < 4; q++) { As[(kh + 2 * q) * PA + lr] = ra[q].x; As[(kh + 2 * q + 1) * PA + lr] = ra[q].y; }
        if (!inside) {
#pragma unroll
            for (int q = 0; q < 2; q++) { Bs[(kq + 2 * q) * PB + lc] = rb[q].x; Bs[(kq + 2 * q + 1) * PB + lc] = rb[q].y; }
        }
        __syncthreads();
        if (k0 + 16 < np) fetch(k0 + 16);
#pragma unroll
        for (int k4 = 0; k4 < 4; k4++) {
            const int kk = 4 * k4 + (lane >> 4), il = lane & 15;
            double av[4], bv[2];
#pragma unroll
            for (int i = 0; i < 4; i++) av[i] = As[kk * PA + 64 * wy + 16 * i + il];
#pragma unroll
            for (int j = 0; j < 2; j++) bv[j] = Bsrc[kk * PBs + 32 * wx + 16 * j + il];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    // block (i, j), accumulator register q: row 16 i + (lane >> 4) + 4 q, column 16 j + (lane & 15)   (C/D layout of the f64 MFMA)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int gi = 128 * I + 64 * wy + 16 * i + (lane >> 4) + 4 * q;
            if (gi >= ld) continue;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int gj = 64 * J + 32 * wx + 16 * j + (lane & 15);
                if (gj < ld) M[(size_t)gi * ld + gj] = acc[i][j][q];
            }
        }
}

// ---- the homotopy megakernel: one persistent workgroup per LCQP -----------------------------------
#ifndef LCQP_MINWAVES
#define LCQP_MINWAVES 4      // waves per SIMD the register allocation is held to (4 workgroups per CU)
#endif
// A second build of the two persistent kernels for batches of at most three workgroups per CU, np <= 512 (lcqp_nch.hip with -DLCQP_TU_FEW: LCQP_VARIANT 1,
// LCQP_MINWAVES 2): 256 registers instead of 128 -- 8.0 -> 7.3 ms for one LCQP alone, 11.3 -> 10.3 at B = 16, 13.5 -> 12.3 at B = 128,
// 14.4 -> 13.2 at B = 256, 21.7 -> 20.7 at B = 768 (two workgroups per CU resident, the rest behind them), the same bits; from B = 896 on four
// resident workgroups per CU win (28.6 against 31.9 ms at B = 1024).  profiles/round6/latency/.  (Eight rows in flight per wave instead of
// four would take another 1 - 4 % off the small batches, but the compiler then contracts the dot products of the sweeps into other fused
// multiply-adds: 1e-16 of difference and other iterate counts -- an instance must not depend on the size of the batch it is solved in.)
// V gives the instantiations of the builds different names: 0 the standard one, 1 the second one; 2 and 3 are the same two builds of
// k_lcqp_run for a batch that holds one set of matrices (lcqp_nch.hip with -DLCQP_TU_SHARED), where every matrix block is instance 0's.
#ifndef LCQP_VARIANT
#define LCQP_VARIANT 0
#endif
// LR: the row state of the subsolver lives in LDS (np <= 256 and at most LDS_ROWS_MAX rows of E; lcqp_wg.hpp)
template <int NCH, bool LR, int V>
__global__ __launch_bounds__(WG, LCQP_MINWAVES) void k_lcqp_run(DevBatch db)
{
    LCQP_LDS_N(NCH)
    constexpr int MI = V >= 2 ? MI_FIRST : MI_OWN;
    Ctx<NCH> c = make_ctx<NCH, MI>(db, blockIdx.x, lds);
    // the dependent-row rules are part of the subsolver here too (round 2 measured them behind a switch at 73.0 vs 72.0 ms, profiles/round2:
    // since the factor is updated instead of rebuilt they cost nothing), so the batched loop and the per-QP path are ONE algorithm
    lcqp_run<NCH, LR, MI>(c);
}

// ---- one QP per workgroup with the SubsolverBase semantics ----------------------------------------
template <int NCH, int V>
__global__ __launch_bounds__(WG, LCQP_MINWAVES) void k_qp_solve(DevBatch db, int initial)
{
    LCQP_LDS_N(NCH)
    Ctx<NCH> c = make_ctx<NCH, MI_OWN>(db, blockIdx.x, lds);      // the QP object's batch of one is never a shared one
    const double* y0 = (initial && c.info->hasY0) ? db.y0 + (size_t)c.b * db.nd : nullptr;
    int iters = 0;
    const int ef = qp_solve<NCH>(c, initial, c.V(V_GK), y0, &iters);   // single-QP path: dependent-row rules and rho adaptation
    if (ef == 0) qp_export<NCH>(c, db.xout + (size_t)c.b * db.n, db.n, db.yout + (size_t)c.b * db.nd);
    if (threadIdx.x == 0) {
        lcqp_stats_t s;
        memset(&s, 0, sizeof(s));
        s.subproblemIter = iters;
        s.qpSolverExitFlag = ef;
        s.returnValue = ef ? LCQP_SUBPROBLEM_SOLVER_ERROR : 0;
        s.admmIter = c.cAdmm; s.trials = c.cTrials; s.factorizations = c.cFact; s.corrections = c.cCorr; s.qpSolves = 1; s.reserved = c.cSweeps;
        db.stats[c.b] = s;
    }
}

// ---- synthetic instances directly in HBM (include/lcqp_synth.h) ---------------------
template <int NCH>
__global__ __launch_bounds__(WG) void k_synth_fill(DevBatch db, uint64_t seed0, uint64_t first)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int b = blockIdx.x, t = threadIdx.x;
    Ctx<NCH> c = make_ctx<NCH>(db, b, lds);
    const int n = db.n, nC = db.nC, nComp = db.nComp, mA = db.mA;
    const uint64_t st = lcqp_synth_state(seed0, first + (uint64_t)b);
    double* Mm = c.F1;   // scratch: M, consumed by k_synth_Q
    for (int e = t; e < np * np; e += WG) {
        const int i = e / np, j = e - i * np;
        Mm[e] = (i < n && j < n) ? lcqp_synth_M(st, n, i, j) : 0.0;
    }
    double* xs = c.V(V_TMP);
    for (int i = t; i < np; i += WG) {
        c.V(V_G)[i] = (i < n) ? lcqp_synth_g(st, n, nC, nComp, i) : 0.0;
        xs[i] = (i < n) ? lcqp_synth_xstar(st, n, nC, nComp, i) : 0.0;
        c.V(V_X0)[i] = 0.0;
        c.V(V_LB)[i] = -INFINITY;
        c.V(V_UB)[i] = INFINITY;
    }
    const double sn = sqrt((double)n);
    for (int r = 0; r < mA; r++) {
        double* row = c.E + (size_t)r * np;
        for (int j = t; j < np; j += WG) {
            double v = 0.0;
            if (j < n) {
                if (r < nC) v = lcqp_synth_Araw(st, n, nC, nComp, r, j) / sn;
                else if (r < nC + nComp) v = (j == r - nC) ? 1.0 : 0.0;
                else v = (j == nComp + (r - nC - nComp)) ? 1.0 : 0.0;
            }
            row[j] = v;
        }
    }
    __syncthreads();
    double *l = c.M(M_L), *u = c.M(M_U);
    for (int r = t; r < mA; r += WG) {
        if (r < nC) {
            // A x* summed left to right with separately rounded products, as the host generator does
            const double* row = c.E + (size_t)r * np;
            double ax = 0.0;
            for (int j = 0; j < n; j++) {
#pragma clang fp contract(off)
                const double pr = row[j] * xs[j];
                ax = ax + pr;
            }
            l[r] = ax - lcqp_synth_slo(st, n, nC, nComp, r);
            u[r] = ax + lcqp_synth_shi(st, n, nC, nComp, r);
        } else { l[r] = 0.0; u[r] = INFINITY; }
    }
    if (t == 0) { c.info->nfin = 0; c.info->hasY0 = 0; c.info->isSetup = 0; }
}

// Q = M'M/n + I in exactly the arithmetic of the host generator (oracle: orc_synth_generate): every element is the sum over
// k ascending of separately rounded products (no FMA contraction), then one division and one addition -- so the instances
// generated in HBM are bit-identical to the ones the CPU oracle generates.  One 64x64 tile of the lower triangle per
// workgroup, a 4x4 block per thread; the generator runs before the timed region of bench.py.
template <int NCH>
__global__ __launch_bounds__(WG) void k_synth_Q(DevBatch db)
{
    constexpr int np = 128 * NCH;
    const int ntile = db.nblk * (db.nblk + 1) / 2;
    const int b = blockIdx.x / ntile, tIdx = blockIdx.x % ntile, t = threadIdx.x;
    int I, J;
    tri_tile(tIdx, I, J);
    const double* Mm = db.F1 + (size_t)b * np * np;
    double* Q = db.Q + (size_t)b * np * np;
    const int gi0 = 64 * I + 4 * (t >> 4), gj0 = 64 * J + 4 * (t & 15);
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    for (int k = 0; k < db.n; k++) {
#pragma clang fp contract(off)      // separately rounded product and sum (plain operators: the pragma does not reach into __dmul_rn)
        const double* mk = Mm + (size_t)k * np;
        double mi[4], mj[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { mi[i] = mk[gi0 + i]; mj[i] = mk[gj0 + i]; }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) { const double pr = mi[i] * mj[j]; acc[i][j] = acc[i][j] + pr; }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int gi = gi0 + i, gj = gj0 + j;
            double v = 0.0;
            if (gi < db.n && gj < db.n) v = acc[i][j] / (double)db.n + (gi == gj ? 1.0 : 0.0);   // a quotient plus 0 or 1: nothing to fuse
            Q[(size_t)gi * np + gj] = v;
            Q[(size_t)gj * np + gi] = v;
        }
}

// ---- building-block kernels for tests / micro-benchmarks ------------------------------------------
template <int NCH>
__global__ __launch_bounds__(WG) void k_util_symv(int n, double alpha, const double* A, const double* bv, const double* cv, double* d)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int b = blockIdx.x;
    double* out = d + (size_t)b * np;
    wg_symv<NCH>(A + (size_t)b * np * np, nullptr, n, bv + (size_t)b * np, nullptr, out, nullptr, nullptr, nullptr, lds);
    for (int i = threadIdx.x; i < np; i += WG) out[i] = alpha * out[i] + cv[(size_t)b * np + i];
}

template <int NCH>
__global__ __launch_bounds__(WG) void k_util_rows(int m, const double* A, const double* x, double* dots, const double* coef, double* outT)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int b = blockIdx.x;
    double* o = outT ? outT + (size_t)b * np : nullptr;
    wg_rows<NCH>(A + (size_t)b * m * np, nullptr, m, x ? x + (size_t)b * np : nullptr, dots ? dots + (size_t)b * m : nullptr,
                 coef ? coef + (size_t)b * m : nullptr, lds, [&](int i, double s) { if (o) o[i] = s; });
}

// the row sweep through a row list with row-indexed scalars (wg_rows<NCH, true>: stage 1 / stage 2 of the subsolver's trials), on its own
template <int NCH>
__global__ __launch_bounds__(WG) void k_util_rows_list(int m, int nlist, const double* A, const int* list, const double* x, double* dots, const double* coef, double* outT)
{
    LCQP_LDS_N(NCH)
    constexpr int np = 128 * NCH;
    const int b = blockIdx.x;
    double* o = outT ? outT + (size_t)b * np : nullptr;
    wg_rows<NCH, true>(A + (size_t)b * m * np, list + (size_t)b * nlist, nlist, x ? x + (size_t)b * np : nullptr, dots ? dots + (size_t)b * m : nullptr,
                       coef ? coef + (size_t)b * m : nullptr, lds, [&](int i, double s) { if (o) o[i] = s; });
}

// ---- the launch tables of this translation unit's instantiation (declared in lcqp_launch.hpp) -------------------------------------
template <int NCH>
static void launch_run(const DevBatch& db, int grid, hipStream_t s)
{
    if constexpr (NCH <= 2) {
        // the row state sits behind the routines' scratch (arena[0, LDS_ROWS_OFF)): the sweeps need 6 np doubles there, the triangular solves
        // 5 np, the widest pass over the inverse factor 4 capS, the rotations 3 capS
        static_assert(6 * 128 * NCH <= LDS_ROWS_OFF, "k_lcqp_run<NCH, true>: the sweeps' scratch must end below the row state");
        if (db.mEcap <= LDS_ROWS_MAX && 4 * db.capS <= LDS_ROWS_OFF) { hipLaunchKernelGGL((k_lcqp_run<NCH, true, LCQP_VARIANT>), dim3(grid), dim3(WG), 0, s, db); return; }
    }
    hipLaunchKernelGGL((k_lcqp_run<NCH, false, LCQP_VARIANT>), dim3(grid), dim3(WG), 0, s, db);
}

template <int NCH>
static void launch_qp_solve(const DevBatch& db, int grid, hipStream_t s, int initial)
{
    hipLaunchKernelGGL((k_qp_solve<NCH, LCQP_VARIANT>), dim3(grid), dim3(WG), 0, s, db, initial);
}

namespace lcqp {
#ifdef LCQP_TU_SHARED
// the translation units of a shared batch's builds hold k_lcqp_run only
template <int NCH, int V>
BatchKernel shared_run_kernel()
{
    static_assert(V == LCQP_VARIANT && V >= 2, "compile with -DLCQP_VARIANT=2 (standard) or 3 (second build)");
    return launch_run<NCH>;
}
#elif defined(LCQP_TU_FEW)
// the translation unit of the second build holds the two persistent kernels only
template <int NCH>
const RunKernels& few_kernels()
{
    static const RunKernels k = {launch_run<NCH>, launch_qp_solve<NCH>};      // as this unit builds them: LCQP_VARIANT, LCQP_MINWAVES
    return k;
}
#else
template <int NCH>
const SizeKernels& size_kernels()
{
    static const SizeKernels k = [] {
        SizeKernels t{};
        t.nch = NCH;
        if constexpr (NCH <= 4) t.few = &few_kernels<NCH>();
        t.prepare = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_prepare<NCH>), dim3(grid), dim3(WG), 0, s, db); };
        t.refresh = [](const DevBatch& db, int grid, hipStream_t s, int mode, const double* rho0) { hipLaunchKernelGGL((k_refresh<NCH>), dim3(grid), dim3(WG), 0, s, db, mode, rho0); };
        t.prepare_warm = [](const DevBatch& db, int grid, hipStream_t s, const double* rho0) { hipLaunchKernelGGL((k_prepare_warm<NCH>), dim3(grid), dim3(WG), 0, s, db, rho0); };
        t.prepare_shared = [](const DevBatch& db, hipStream_t s, int src) { hipLaunchKernelGGL((k_prepare_shared<NCH>), dim3(1), dim3(WG), 0, s, db, src); };
        t.share_setup = [](const DevBatch& db, int grid, hipStream_t s, int mode, const double* rho0) { hipLaunchKernelGGL((k_share_setup<NCH>), dim3(grid), dim3(WG), 0, s, db, mode, rho0); };
        if constexpr (NCH <= 4)      // np <= 512 only: a panel of np >= 1024 does not fit LDS
        {
            t.sensitivity_blk = [](const DevBatch& db, int grid, hipStream_t s, int first, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo) {
                hipLaunchKernelGGL((k_sensitivity_blk<NCH>), dim3(grid), dim3(WG), 0, s, db, first, nrhs, v, dg, dbo, side, sinfo);
            };
            t.sensitivity_blk_dual = [](const DevBatch& db, int grid, hipStream_t s, int first, int nrhs, const double* v, const double* vy, int unit,
                                        double* dg, double* dbo, int* side, int* sinfo, int* rowpos) {
                hipLaunchKernelGGL((k_sensitivity_blk_dual<NCH>), dim3(grid), dim3(WG), 0, s, db, first, nrhs, v, dg, dbo, side, sinfo, vy, unit, rowpos);
            };
        }
        t.sensitivity = [](const DevBatch& db, int grid, hipStream_t s, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo) {
            hipLaunchKernelGGL((k_sensitivity<NCH, false>), dim3(grid), dim3(WG), 0, s, db, nrhs, v, dg, dbo, side, sinfo, nullptr);
        };
        t.sensitivity_dual = [](const DevBatch& db, int grid, hipStream_t s, int nrhs, const double* v, const double* vy, double* dg, double* dbo, int* side, int* sinfo) {
            hipLaunchKernelGGL((k_sensitivity<NCH, true>), dim3(grid), dim3(WG), 0, s, db, nrhs, v, dg, dbo, side, sinfo, vy);
        };
        t.build_C = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_build_C<NCH>), dim3(grid), dim3(WG), 0, s, db); };
        t.compress_C = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_compress_C<NCH>), dim3(grid), dim3(WG), 0, s, db); };
        t.factor = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_factor<NCH, 1>), dim3(grid), dim3(WG), 0, s, db); };
        t.factor_full = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_factor<NCH, NCH <= 2 ? 4 : 1>), dim3(grid), dim3(WG), 0, s, db); };
        t.trsm = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_trsm<NCH>), dim3(grid), dim3(WG), 0, s, db); };
        t.trsm_streamed = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_trsm_streamed<NCH>), dim3(grid), dim3(WG), 0, s, db); };
        t.build_M = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_build_M<NCH>), dim3(grid), dim3(WG), 0, s, db); };
        t.run = {launch_run<NCH>, launch_qp_solve<NCH>};
        t.shared_run = shared_run_kernel<NCH, 2>();
        if constexpr (NCH <= 4) t.shared_run_few = shared_run_kernel<NCH, 3>();
        t.synth_fill = [](const DevBatch& db, int grid, hipStream_t s, uint64_t seed0, uint64_t first) { hipLaunchKernelGGL((k_synth_fill<NCH>), dim3(grid), dim3(WG), 0, s, db, seed0, first); };
        t.synth_Q = [](const DevBatch& db, int grid, hipStream_t s) { hipLaunchKernelGGL((k_synth_Q<NCH>), dim3(grid), dim3(WG), 0, s, db); };
        t.util_symv = [](int grid, hipStream_t s, int n, double alpha, const double* A, const double* b, const double* c, double* d) {
            hipLaunchKernelGGL((k_util_symv<NCH>), dim3(grid), dim3(WG), 0, s, n, alpha, A, b, c, d);
        };
        t.util_rows = [](int grid, hipStream_t s, int m, const double* A, const double* x, double* dots, const double* coef, double* outT) {
            hipLaunchKernelGGL((k_util_rows<NCH>), dim3(grid), dim3(WG), 0, s, m, A, x, dots, coef, outT);
        };
        t.util_rows_list = [](int grid, hipStream_t s, int m, int nlist, const double* A, const int* list, const double* x, double* dots, const double* coef, double* outT) {
            hipLaunchKernelGGL((k_util_rows_list<NCH>), dim3(grid), dim3(WG), 0, s, m, nlist, A, list, x, dots, coef, outT);
        };
        return t;
    }();
    return k;
}
#endif
}  // namespace lcqp
