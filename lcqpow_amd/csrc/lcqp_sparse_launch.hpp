// lcqp_sparse_launch.hpp -- the seam between the host translation unit of the sparse arm (lcqp_sparse_host.hip: the C ABI lcqp_hip_sparse_*)
// and its kernel translation units (lcqp_sparse.hip, one per lane-group width G in {8,16,32,64}): the batch as the kernels see it, the
// constants both sides index it with, and the table of launch functions of a width.  Plain structs and declarations only: no device code
// lives here.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/lcqp_hip.h"

namespace lcqp_sparse {
// nothing of the seam enters the dynamic symbol table of the library: not the launch functions, and not what the host runtime's templates
// (lcqp_host_rt.hpp) become when they are instantiated over these structs
#pragma GCC visibility push(hidden)

enum { NV_G, NV_GTIL, NV_GPHI, NV_XK, NV_PK, NV_XNEW, NV_GK, NV_QX, NV_CX, NV_QP, NV_CP, NV_TMP, NV_XQ, NV_XA, NV_XT, NV_R1,
       NV_X0, NV_NUM };
enum { MV_L, MV_U, MV_RHOV, MV_YQ, MV_YA, MV_ZA, MV_YT, MV_EX, MV_YK, MV_Y0, MV_LX, MV_LX2, MV_NUM };
enum { MI_ST, MI_STT, MI_STF, MI_NEW, MI_NUM };

struct SpInfo {
    int haveSolution, stfValid, hasY0, bigReg;     // bigReg: this instance needs the safe regularisation of the polish (a Hessian that is only semidefinite)
    int warm, pad0;                                // warm (k_sparse_refresh, k_sparse_setup_warm): sp_ph_start begins at the last solution, at the penalty rho0, without the zero-penalty QP
    double rho0;
    double scale, sigma, delta, delta2, phiConst;
    double deltaS, delta2S;                        // the light level tried first (sp_polish)
    double e1max;                                  // largest row 1-norm of E: with |x|_inf the scale of the rounding of a computed E_r x (the active-row test of the polish)
    double hist[64];
    double bytes;        // algorithmic bytes counted by the kernel
    double prof[8];      // -DLCQP_PROFILE: clock ticks per phase (SP_* below)
};
enum { SP_PRODUCTS, SP_ASSEMBLE, SP_FACTOR, SP_FORWARD, SP_BACKWARD, SP_VECTORS, SP_LCQP, SP_RHS, SP_NPHASE };

// ---- the homotopy as a phase machine (round 4) ----------------------------------------------------------------------------------------
// Round 3 ran the whole homotopy of an instance inside one persistent lane group: the 64 / G instances of a wavefront moved in lock step, an
// instance was active in 74 % of its wavefront's trials and refactorised in 26 % of them while its wavefront did in 83 %.  Now an instance is
// a record in memory (SpState + its vectors) that moves through QUEUES, one per phase; a wavefront pops up to 64 / G instances that are in
// the SAME phase, runs that phase for them, and pushes each to the queue of its next phase (k_sparse_sched).  A wavefront therefore only
// ever holds instances doing the same thing; nobody waits for a neighbour's factorisation or for the slowest polish of eight.
enum { PH_START, PH_ROUND, PH_TRIAL, PH_FACTOR, PH_CORRECT, PH_QPEND, PH_NUM };
enum { BY_ASSEMBLE, BY_FACTOR_LDS, BY_FACTOR, BY_SOLVE, BY_BORDER_PREPARE, BY_BORDER_SOLVE, BY_EX, BY_SWEEP, BY_START, BY_E, BY_NUM };
struct SpState {
    // LCQProblem::runSolver (src/LCQProblem.cpp:444-560)
    int initial, histLen, algoStat, totalIter, rc, qpIter;
    double alphak, rho, gmaxNext;
    unsigned long long perturbCounter;
    lcqp_stats_t st;
    // the subsolver call (oracle: sqp_solve)
    int round, n_admm, use_stored, backup_pending, admm_ready, trials0, admm0;
    // the polish (oracle: sqp_polish)
    int trial, reuse, fact_valid, borderTodo, nrefine;      // nrefine: refinement corrections taken for the active rows alone
    double gs, ytol, dpUsed, d2Used, xinf;                  // xinf: |x|_inf behind the last correction
    // work counters
    int cAdmm, cTrials, cFact, cCorr, cSweeps;
    double bytes;
};
// Queues: the batch is cut into pools of `poolSize` consecutive instances (a power of two; the byte offset of an instance inside its pool fits
// 32 bits for every per-instance array: the saddr + 32-bit offset addressing of SpCtx::arr); wavefront w serves pool w % nPools.  Per pool
// and phase a ring of poolSize entries (an instance is in at most one queue) and three counters: tail (next position to write), head (next
// position to read), count (entries published); every ring slot carries a SEQUENCE number beside the instance id (a bounded multi-producer /
// multi-consumer queue after Vyukov; sequence and id share one 64-bit word, written by one store): slot p & mask is free for position p when
// its sequence is p, holds position p's entry when it is p + 1, and is handed on to position p + poolSize by its consumer -- a producer that laps the ring onto a slot whose entry has been claimed but not
// read yet waits instead of overwriting it.  ctl[pool][PH_NUM] = instances of the pool not finished yet.
constexpr int QCTL = 4;      // ints per (pool, phase): tail, head, count, pad

struct EllMat { const int *eidx, *epos, *ptr, *cidx, *cmap; int rows, W, tails; };   // see g_ell

struct SpBatch {
    int B, n, m, nC, nComp, N, Np, w, ld, nnzQ, nnzE, G;  // Np: N rounded up to a multiple of 64 (padding rows: zero coefficients)
    int hasLbL, hasLbR;
    lcqp_options_t opt;
    const int *Qp, *Qi, *Ep, *Ei, *ETp, *ETi, *ETmap, *iperm, *bandQ, *bandE;
    const int *bsrc, *pnode, *qdiag, *Erow;   // band entry -> value it comes from (sp_factor_reg), node of a band position, Q_ii, row of an E entry
    const int *bgate, *bdiag;                 // band entry -> the row of E whose membership in the working set gates it (-1: none); band position -> its diagonal (sp_factor_reg)
    EllMat ellQ, ellE, ellT; // rows of Q, rows of E, columns of E in ELL slabs
    double *Qx, *Ex;         // [B][nnzQ], [B][nnzE] (CSR order)
    double *Kb;              // [B][N*ld] assembled band rows (input of a factorisation): Kb[i*ld + k] = K[i][i-w+k]
    double *KaF, *KaD;       // ADMM KKT factor in the folded layout of band_sweep [B][Np*G], 1/D [B][Np]
    double *KpF, *KpD;       // polish KKT factor
    double* K0;              // [Np][G] per instance: the band rows of [Q, E'; E, .] with every row of E in, diagonal slot Q_ii (variables) -- what sp_factor_reg streams
    int bitWords;            // 32-bit words of a working set's bit set in LDS (sp_ph_factor), 0: it does not fit, the flags are read from memory
    double *nv, *mv, *Nv;    // [B][NV_NUM][n], [B][MV_NUM][m], [B][2][Np]
    // Bordered band (round 3): the last kb positions of the ordering are border nodes -- rows or variables too dense for any band (the
    // coupling constraint and the two shared variables of examples/OptimizeOnCircle.cpp).  K = [Bd U'; U C]: the band engine factorises
    // Bd with the border positions as isolated unit pivots; the border is carried by W = U inv(Bd) (kb band solves per factorisation) and
    // the Schur complement S = C - W U' (kb x kb, dense LDL').  U: per border node the entries it shares with band nodes (Upos: band
    // position, Usrc: entry of Q (k < nnzQ) or of E (nnzQ + k, CSR order), Ugate: the row of E whose membership in the working set gates
    // the entry, -1 none); C: the entries among border nodes, lower triangle (Cb2: the other border node).
    int kb, nU, nCb;
    int lightOK;     // the ordering puts every row behind one of its variables and every Hessian of the batch is safely definite: the polish tries its light regularisation first
    const int *bnode, *Uptr, *Upos, *Usrc, *Ugate, *Cptr, *Cb2, *Csrc, *Cgate;
    double *bW, *bUv, *bS;   // [B][2][kb][Np] W rows, [B][2][nU] gated values of U, [B][2][kb][kb] factor of S   (index 0: polish, 1: ADMM)
    double *lbL, *lbR;       // [B][nComp]
    int* mi;                 // [B][MI_NUM][m]
    SpInfo* info;
    lcqp_stats_t* stats;
    double *xout, *yout;     // [B][n], [B][m]
    // per-iterate tracking (options.storeSteps, src/LCQProblem.cpp:1365-1378), as on the dense path: [B][traceCap][8] = (|statk|inf, phi, rho,
    // alphak, obj, merit, |pk|inf, QP iterations), [B][traceCap][n] = xk, traceLen[B]; traceCap == 0: not allocated
    double *traceS, *traceX;
    int* traceLen;
    int traceCap;
    // phase machine
    SpState* state;          // [B]
    unsigned long long* qring;  // [nPools][PH_NUM][poolSize] ring slots: (sequence number << 32) | instance id, one 64-bit word so that a slot changes hands in one store
    int* qctl;                  // [nPools][PH_NUM + 1][QCTL]
    int poolSize, nPools;
    int wideDiv;                // SIMDs of the device per pool (lcqp_hip_sparse_create): unfinished instances of the pool / wideDiv = instances of a streaming step
    // General sparse LDL' (round 6; lcqp_sparse_general.hpp): patterns that are neither banded nor bordered -- multifrontal over a nested-
    // dissection tree with dense fronts, one wavefront per instance (G = 64).  general != 0: KaF / KpF hold the panels of the fronts
    // (gLsize doubles per instance instead of Np * G), KaD / KpD 1 / D per position as for the band; kb = 0, lightOK = 0.
    int general, gnF, gMaxFront;
    unsigned gLsize, gStackSize;
    const int *gPiv0, *gNp, *gNb, *gRowPtr, *gRows, *gChildPtr, *gChild, *gRel, *gAsmPtr, *gAsmSrc, *gAsmGate, *gAsmPos;
    const unsigned *gLoff, *gCBoff;
    const int *gMeta, *gChildInfo;   // [gnF][GEN_META] np, nb, piv0, rowPtr, asmPtr, asmEnd, childPtr, childEnd, Loff, CBoff: one load per front; [children][4] nb, CBoff, rowPtr of the child
    double *gStack, *gFront;     // [B][gStackSize] update blocks of the fronts, [B][gMaxFront^2] a front too large for LDS
    size_t kfStride;             // doubles per instance of KaF / KpF
    // algorithmic bytes of one event of each kind (filled by the host: formed in the kernel they are loop invariants the compiler keeps in
    // registers across every phase)
    double by[BY_NUM];
    unsigned long long* qprof;   // [PH_NUM + 1][3] (-DLCQP_SCHED_PROFILE): clock ticks, wavefront steps, instances served per phase; row PH_NUM: ticks / polls without work
};

constexpr int GEN_META = 12;      // ints per front of SpBatch::gMeta

// Per lane-group width one table of launch functions, as lcqp_launch.hpp has one per padded size.
// SpFirst: the kernel in front of the homotopy -- SETUP: k_sparse_setup<G> (a run); REFRESH: k_sparse_refresh<G>(mode, rho0), new vectors on
// the setup in place; SETUP_WARM: k_sparse_setup_warm<G>(rho0), new values of the matrices under the point of the last run.
// SpRunFn: the launches of a run on `stream` -- the kernel `first` names, `mid` recorded behind it, then the homotopy (k_sparse_sched_init,
// k_sparse_sched<G>).  cus: compute units of the device the batch lives on (the persistent wavefronts of k_sparse_sched are at most what
// it holds at once).
// SpSensitivityFn: one launch of k_sparse_sensitivity<G, false> on `stream` over device buffers (layouts at the kernel).
// SpSensitivityDualFn: k_sparse_sensitivity<G, true>, which adds the upstream gradients on the duals vy [B][nrhs][m] (lcqp_hip_sparse_adjoint).
enum class SpFirst { SETUP, REFRESH, SETUP_WARM };
using SpRunFn = void(const SpBatch& db, int cus, hipStream_t stream, hipEvent_t mid, SpFirst first, int mode, const double* rho0);
using SpSensitivityFn = void(const SpBatch& db, hipStream_t stream, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo);
using SpSensitivityDualFn = void(const SpBatch& db, hipStream_t stream, int nrhs, const double* v, const double* vy, double* dg, double* dbo, int* side, int* sinfo);
// SpKktProbeFn: one launch of k_sparse_kkt_probe<G> on `stream` over device buffers (layouts and modes at the kernel).
using SpKktProbeFn = void(const SpBatch& db, hipStream_t stream, int mode, int which, int nrhs, const double* dprim, const double* ddual, const int* use,
                          const double* rhs, double* sol, double* recP, double* recD, int* recU);
// SpProductProbeFn: one launch of k_sparse_product_probe<G> on `stream` over device buffers: the sparse products of lcqp_sparse_solver.hpp
// applied to the caller's vectors.  vn [B][PPN_NUM][n] and vm [B][PPM_NUM][m] are the inputs, on [B][PPO_NUM][n], om [B][m] (E x) and os
// [B][PPS_NUM] the outputs.  wide: one instance per wavefront with all 64 lanes, as the streaming phases of k_sparse_sched run the products.
enum { PPN_X, PPN_Q0, PPN_Q1, PPN_BASE, PPN_G, PPN_XR, PPN_C0, PPN_C1, PPN_NUM };      // sp_Ex | sp_Qx2 | base of sp_ETy | g, x of sp_residual | sp_Cx2
enum { PPM_Y, PPM_YR, PPM_LX0, PPM_LX1, PPM_NUM };                                     // y of sp_ETy | y of sp_residual | lx0, lx1 of sp_C_from_Ex
enum { PPO_QX0, PPO_QX1, PPO_ETY, PPO_R1, PPO_QXR, PPO_CX0, PPO_CX1, PPO_CE0, PPO_CE1, PPO_CE, PPO_CEZ, PPO_NUM };   // CE0, CE1: TWO; CE, CEZ (zeros): one vector
enum { PPS_ETY_MAX, PPS_RES_MAX, PPS_RES_SCALE, PPS_NUM };
struct SpProductProbeArgs { double *vn, *vm, *on, *om, *os; };
using SpProductProbeFn = void(const SpBatch& db, hipStream_t stream, int wide, const SpProductProbeArgs& a);
// SpSensitivityBlkFn: one launch of k_sparse_sensitivity_blk<G> on `stream` (DESIGN.md section 3a''', "The sparse arm"): the work items
// [item0, item0 + nItems) of a call whose items are numbered (instance - first) * npan + panel; column c of panel q is column q * panel + c of
// the call, ncols columns per instance.  unit != 0: column j is the unit vector e_j and v is not read; else v [count][ncols][n].  The outputs
// of item item0 + i are staged at dg + i * panel * n and dbo + i * panel * m, one contiguous vector per column; side [count][m] (written by
// the item of panel 0), info [count] (OR-ed into: zeroed by the host in front of the call's first launch); ws: the items' workspaces,
// sens_blk_ws_doubles(db, panel) doubles each.
// The DUAL kernels (k_sparse_sensitivity_blk_dual<G>, k_sparse_sensitivity_blk_general_dual; DESIGN.md section 3a'''', "The sparse arm: panels with
// gradients on y") read three more members, which the kernels above ignore: vy [count][ncols][m], the upstream gradients on the duals (v may
// then be NULL: a zero panel; unit is 0); dunit != 0: ncols = m, column j is [0; -e_r(j)] on the j-th row of W, v and vy are not read, and
// rowpos [nItems][panel] receives r(j) per staged column (-1: a column past |W|, whose staged outputs are not written).
struct SpSensBlkArgs {
    int first, npan, ncols, unit, item0, nItems;
    const double* v;
    double *dg, *dbo;
    int *side, *info;
    double* ws;
    const double* vy;
    int dunit;
    int* rowpos;
};
using SpSensitivityBlkFn = void(const SpBatch& db, hipStream_t stream, const SpSensBlkArgs& a);
// doubles of workspace per work item: the solve panel [Np], d and Q d [n], lambda [m], interleaved by column
__host__ __device__ inline size_t sens_blk_ws_doubles(const SpBatch& db, int panel) { return (size_t)panel * ((size_t)db.Np + 2 * (size_t)db.n + db.m); }
// panel: the panel width of this lane width's k_sparse_sensitivity_blk (0: the width is routed to the vector kernel)
// sensitivity_blk_general, panel_general: k_sparse_sensitivity_blk_general and its panel width -- the unit of G = 64 alone, null / 0 elsewhere
// sensitivity_blk_dual, sensitivity_blk_general_dual: the DUAL kernels of the two, with the same panel widths
struct SpKernels { int G; SpRunFn* run; SpSensitivityFn* sensitivity; SpSensitivityDualFn* sensitivity_dual; SpKktProbeFn* kkt_probe;
                   SpSensitivityBlkFn* sensitivity_blk; int panel; SpSensitivityBlkFn* sensitivity_blk_general; int panel_general;
                   SpProductProbeFn* product_probe;
                   SpSensitivityBlkFn* sensitivity_blk_dual; SpSensitivityBlkFn* sensitivity_blk_general_dual; };
// defined in lcqp_sparse.hip and instantiated there for G = LCQP_TU_G
template <int G> const SpKernels& sparse_kernels();
#pragma GCC visibility pop

}  // namespace lcqp_sparse
