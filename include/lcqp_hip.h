/*
 * lcqp_hip.h -- C ABI of the MI355X-native LCQPow hot path (liblcqpow_hip.so).
 *
 * This is the drop-in boundary of SURVEY.md §8(b): plain C types, caller-owned buffers, integer
 * return codes, no exceptions.  Each entry point cites the reference interface it replaces
 * (file:line under the LCQPow tree).  A reference-side binding (a SubsolverHIP class derived from
 * SubsolverBase) is shown in INTEGRATION.md.
 *
 * Two groups:
 *   lcqp_hip_qp_*     one convex QP object with the SubsolverBase semantics
 *                     (include/SubsolverBase.hpp:37,52-56; src/SubsolverQPOASES.cpp:32-46,134-181).
 *   lcqp_hip_batch_*  B independent LCQPs solved by the penalty homotopy entirely on the device
 *                     (LCQProblem::loadLCQP + runSolver, src/LCQProblem.cpp:87-144,444-560), one
 *                     persistent workgroup per instance.  The reference has no batched API; this is
 *                     the throughput path that BASELINE.json's metric is measured on.
 *
 * All matrices are dense row-major doubles exactly as the reference takes them
 * (src/Utilities.cpp:43).  Infinite bounds are IEEE +-INFINITY (src/LCQProblem.cpp:596,607).
 */
#ifndef LCQP_HIP_H
#define LCQP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ReturnValue subset used across the boundary: include/Utilities.hpp:37-87 */
#define LCQP_SUCCESSFUL_RETURN 0
#define LCQP_INVALID_ARGUMENT 100
#define LCQP_INVALID_OBJECTIVE_LINEAR_TERM 116
#define LCQP_INVALID_CONSTRAINT_MATRIX 117
#define LCQP_INVALID_COMPLEMENTARITY_MATRIX 118
#define LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND 120
#define LCQP_MAX_ITERATIONS_REACHED 200
#define LCQP_MAX_PENALTY_REACHED 201
#define LCQP_SUBPROBLEM_SOLVER_ERROR 203
#define LCQP_LCQPOBJECT_NOT_SETUP 300
/* backend errors (new) */
#define LCQP_HIP_ERROR 900          /* a HIP runtime call failed; see lcqp_hip_last_error() */
#define LCQP_HIP_UNSUPPORTED 901    /* dimensions outside what the kernels are built for */

/* Options: the 13 algorithm options of include/Options.hpp with the defaults of
 * src/Options.cpp:296-333, followed by the subsolver knobs that take the place of
 * qpOASES::Options (src/Options.cpp:320-321). */
typedef struct {
    double complementarityTolerance; /* 1e3*EPS */
    double stationarityTolerance;    /* 1e6*EPS */
    double initialPenaltyParameter;  /* 0.01 */
    double penaltyUpdateFactor;      /* 2 */
    double maxPenaltyParameter;      /* 1e8 */
    double etaDynamicPenalty;        /* 0.9 */
    int    solveZeroPenaltyFirst;    /* 1 */
    int    perturbStep;              /* 1 */
    int    maxIterations;            /* 1000 */
    int    nDynamicPenalty;          /* 3 */
    int    printLevel;               /* 2; the device path never prints */
    int    storeSteps;               /* 0 */
    uint64_t perturbSeed;            /* deterministic stand-in for srand(time(NULL)), src/LCQProblem.cpp:1016 */
    double admmRho, admmSigma, admmAlpha, rhoEqMult;
    double proxSmall, proxBig, pivotThreshold, depTau, feasTol, resTol;
    int    admmFirst, admmHot, maxTrials, maxRounds;
} lcqp_options_t;

/* OutputStatistics counters (src/OutputStatistics.cpp:81-128) + work counters of the subsolver. */
typedef struct {
    int    iterTotal, iterOuter, subproblemIter, status, qpSolverExitFlag, returnValue;
    double rhoOpt;
    int    admmIter, trials, factorizations, corrections, qpSolves, reserved;
} lcqp_stats_t;

void lcqp_hip_options_default(lcqp_options_t* opt);               /* Options::setToDefault, src/Options.cpp:296 */
const char* lcqp_hip_last_error(void);
int  lcqp_hip_device_count(void);
/* Ask the HIP runtime for n hardware queues (sets GPU_MAX_HW_QUEUES unless the environment already holds a value).  Opt-in, for the
 * PROGRAM to call before the first HIP call of the process -- the runtime reads the variable once; the library never changes the
 * environment by itself.  A BatchPipeline with more batch objects alive than its own wants this.
 * Returns 0 (set), 1 (already set by the caller's environment: left alone) or LCQP_HIP_ERROR (n outside 1..64). */
int  lcqp_hip_request_hw_queues(int n);

/* ------------------------------------------------------------------------------------------------
 * QP object == SubsolverBase implementation state.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lcqp_hip_qp lcqp_hip_qp_t;

/* SubsolverQPOASES(int nV,int nC,double* Q,double* A): src/SubsolverQPOASES.cpp:32-46 (deep copy of Q, A).
 * nC is the number of stacked rows (nC + 2*nComp).  Host pointers.  Returns NULL on failure. */
lcqp_hip_qp_t* lcqp_hip_qp_create(int nV, int nC, const double* Q, const double* A,
                                  const lcqp_options_t* opt, int device);
/* copy-ctor / operator= of the reference (src/SubsolverQPOASES.cpp:184-230): the clone carries the host copies
 * of Q, A and the options; its device state is built by its own first (initial) solve -- the reference only
 * copies subsolvers before their first use (src/Subsolver.cpp:125-136, src/LCQProblem.cpp:906-907). */
lcqp_hip_qp_t* lcqp_hip_qp_clone(const lcqp_hip_qp_t* src);
void lcqp_hip_qp_destroy(lcqp_hip_qp_t* qp);
/* SubsolverQPOASES::setOptions, src/SubsolverQPOASES.cpp:120-131 (takes effect at the next initial solve) */
int  lcqp_hip_qp_set_options(lcqp_hip_qp_t* qp, const lcqp_options_t* opt);
/* SubsolverBase::solve, include/SubsolverBase.hpp:52-56 / src/SubsolverQPOASES.cpp:134-169.
 * Returns LCQP_SUCCESSFUL_RETURN or LCQP_SUBPROBLEM_SOLVER_ERROR; *exit_flag != 0 on failure (the reference stores
 * qpOASES' raw status there, src/LCQProblem.cpp:1122, and its tests only require "non-zero on failure"):
 *   1 the subsolver gave up after maxRounds rounds, 2 lbA > ubA or lb > ub, 3 the setup factorisations failed,
 *   4 certified primal infeasible, 5 certified unbounded (OSQP's certificates on the ADMM iterates), -1 HIP error.
 * lbA/ubA/lb/ub/x0/y0 may be NULL as in the reference. */
int  lcqp_hip_qp_solve(lcqp_hip_qp_t* qp, int initialSolve, int* iterations, int* exit_flag,
                       const double* g, const double* lbA, const double* ubA,
                       const double* x0, const double* y0, const double* lb, const double* ub);
/* SubsolverBase::getSolution, include/SubsolverBase.hpp:37 / src/SubsolverQPOASES.cpp:172-181:
 * x[nV], y[nV + nC]: box duals first, then one dual per stacked row; Qx + g - A'y_A - y_box = 0. */
void lcqp_hip_qp_get_solution(lcqp_hip_qp_t* qp, double* x, double* y);
void lcqp_hip_qp_get_counters(lcqp_hip_qp_t* qp, int* admm, int* trials, int* factorizations, int* corrections);
/* lcqp_hip_batch_sensitivity (below) for the batch of one this object holds: the derivatives of the solution of the convex QP last solved,
 * dg [nrhs][nV], db and side [.][nV + nC], info [1].  LCQP_LCQPOBJECT_NOT_SETUP before the first successful solve and after set_options. */
int  lcqp_hip_qp_sensitivity(lcqp_hip_qp_t* qp, int nrhs, const double* v, double* dg, double* db, int* side, int* info);
/* lcqp_hip_batch_sensitivity_blocked and lcqp_hip_batch_jacobian (below) for the batch of one: dg [nrhs][nV], db [nrhs][nV + nC];
 * Jg [nV][nV], Jb [nV][nV + nC] (or NULL), side [nV + nC], info [1].  nV > 512: the vector kernel, the bits of lcqp_hip_qp_sensitivity. */
int  lcqp_hip_qp_sensitivity_blocked(lcqp_hip_qp_t* qp, int nrhs, const double* v, double* dg, double* db, int* side, int* info);
int  lcqp_hip_qp_jacobian(lcqp_hip_qp_t* qp, double* Jg, double* Jb, int* side, int* info);
/* lcqp_hip_batch_adjoint (below) for the batch of one: vx, dg [nV]; vy (or NULL), db, side [nV + nC]; info [1]; dQ [nV][nV] and dA [nC][nV]
 * (A = the stacked rows) may be NULL.  LCQP_INVALID_ARGUMENT: NULL object, vx or dg; LCQP_LCQPOBJECT_NOT_SETUP as lcqp_hip_qp_sensitivity. */
int  lcqp_hip_qp_adjoint(lcqp_hip_qp_t* qp, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                         double* dQ, double* dA);
/* test and diagnostic entry points: lcqp_hip_batch_read_setup / lcqp_hip_batch_read_working_set / lcqp_hip_batch_read_admm (below) for the
 * batch of one this object holds; LCQP_LCQPOBJECT_NOT_SETUP before its first solve */
int  lcqp_hip_qp_read_setup(lcqp_hip_qp_t* qp, int dims[9], double scal[2], double* C, double* F1, double* D1, double* Et, double* MM,
                            int* Cp, int* Ci, double* Cv);
int  lcqp_hip_qp_read_working_set(lcqp_hip_qp_t* qp, int dims[2], int* slot_row, int* crow, int* row_slot, double* Ti);
int  lcqp_hip_qp_read_admm(lcqp_hip_qp_t* qp, int dims[6], double scal[3], double* FK, double* rhov, double* l, double* u,
                           double* xa, double* ya, double* za, double* dy, double* dx);
/* lcqp_hip_batch_read_polish (below) for the batch of one; k_qp_solve keeps the row state in its global arrays (dims[9] says what the
 * homotopy kernel of that shape would do and does not concern this object) */
int  lcqp_hip_qp_read_polish(lcqp_hip_qp_t* qp, int dims[12], double scal[7], double* V, double* M, int* I);

/* ------------------------------------------------------------------------------------------------
 * Batch of B independent dense LCQPs of one shape (nV, nC, nComp).
 * ---------------------------------------------------------------------------------------------- */
typedef struct lcqp_hip_batch lcqp_hip_batch_t;

/* LCQProblem(nV,nC,nComp) x B: src/LCQProblem.cpp:43-79.  withBox != 0 reserves rows for lb/ub. */
lcqp_hip_batch_t* lcqp_hip_batch_create(int batch, int nV, int nC, int nComp, int withBox, int device);
/* A batch that holds ONE Q, A, L, R for all its instances (parametric MPC, parameter sweeps, multi-start; DESIGN.md section 3a, "One set
 * of matrices"): the blocks that depend on the matrices, the box pattern and the options alone -- Q, C, E, Et, L1, its inverted diagonal
 * blocks, M and the compressed rows of C -- are stored once and set up once, on a grid of one matrix instance; what an instance writes
 * during a solve stays per instance.  The handle is an lcqp_hip_batch_t that every lcqp_hip_batch_* call accepts, and an instance returns
 * the same BITS (x, y, statistics, trace, every derivative) as the same problem in an ordinary batch of the same shape.  What differs:
 *   lcqp_hip_batch_load / _load_device   Q, L, R, A are ONE [rows][nV] array each.  A non-NULL matrix replaces the batch's matrix whatever
 *       the range; NULL keeps the one in place (the host call too), and before a matrix is in place its missing-matrix code is returned.
 *       The device twin wants the `shared` bit of every matrix it is given, else LCQP_INVALID_ARGUMENT, nothing written.  Vectors are
 *       [count][..] as ever.  The set of variables with a finite lb or ub is ONE for the batch (they are rows of the one E): the first
 *       load defines it, from its first instance, and so does a load that brings a matrix while no instance outside its range holds a
 *       problem; any other load whose set differs gets LCQP_INVALID_ARGUMENT, the lowest (instance, variable) in lcqp_hip_last_error(),
 *       nothing written -- the rule lcqp_hip_batch_update has on every batch.
 *   lcqp_hip_batch_update_matrices / _device   first == 0 and count == batch, arrays [rows][nV], the `shared` bits as above; anything else
 *       LCQP_INVALID_ARGUMENT, nothing written.
 *   lcqp_hip_batch_generate_synthetic   LCQP_INVALID_ARGUMENT: the generator draws matrices per instance.
 * A factorisation that fails, fails every instance (setupFail on all of them, LCQP_SUBPROBLEM_SOLVER_ERROR from the run). */
lcqp_hip_batch_t* lcqp_hip_batch_create_shared(int batch, int nV, int nC, int nComp, int withBox, int device);
/* out[0]: bytes of device memory in the pools lcqp_hip_batch_create(_shared) allocated; out[1]: the part of them held once for the batch
 * (0 on an ordinary batch).  Host arithmetic; NULL handle: LCQP_LCQPOBJECT_NOT_SETUP, NULL out: LCQP_INVALID_ARGUMENT. */
int  lcqp_hip_batch_device_bytes(lcqp_hip_batch_t* b, size_t out[2]);
void lcqp_hip_batch_destroy(lcqp_hip_batch_t* b);
/* LCQProblem::setOptions, include/LCQProblem.ipp:160-163 */
int  lcqp_hip_batch_set_options(lcqp_hip_batch_t* b, const lcqp_options_t* opt);
/* LCQProblem::loadLCQP (dense), src/LCQProblem.cpp:87-144, for instances [first, first+count):
 * arrays are host pointers, packed instance after instance ([count][...]); NULL as in the reference.
 * The host load and update are the device path (lcqp_hip_batch_load_device / _update_device below) behind an upload: after the argument
 * and value checks, which run on the host over the whole range, the arrays go to the device as they are, in chunks of whole instances
 * through two pinned slots into a device staging of two chunks, and the pack kernels of the device path build the pools from each chunk.
 * A chunk holds at most 16 MiB and at most half the staging cap of lcqp_hip_batch_set_jacobian_staging (one instance always fits); the
 * pools do not depend on the chunking.  Synchronous: the arrays are free on return.  A failing load, like a failing update, leaves the
 * range untouched: nothing is written, and no host state changes. */
int  lcqp_hip_batch_load(lcqp_hip_batch_t* b, int first, int count,
                         const double* Q, const double* g, const double* L, const double* R,
                         const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                         const double* A, const double* lbA, const double* ubA,
                         const double* lb, const double* ub, const double* x0, const double* y0);
/* Fill instances [0,B) with the synthetic generator of include/lcqp_synth.h directly in HBM
 * (instance id = firstInstance + b). */
int  lcqp_hip_batch_generate_synthetic(lcqp_hip_batch_t* b, uint64_t seed0, uint64_t firstInstance);
/* read one instance's problem data back (any pointer may be NULL) -- used by parity tests / cpu_baseline */
int  lcqp_hip_batch_read_problem(lcqp_hip_batch_t* b, int instance, double* Q, double* g, double* L, double* R,
                                 double* A, double* lbA, double* ubA);
/* Test and diagnostic entry points: the raw, padded device blocks of one instance after lcqp_hip_batch_setup / lcqp_hip_batch_run
 * (both streams of the batch are synchronised first; any pointer may be NULL -- call once with buffers NULL to learn the sizes).
 * dims[9] = np, nblk, mEcap, mMld, capS, capC, the instance's mE, cNnz (-1: C is not compressed), setupFail; scal[2] = spv (the shift
 * sigma_p of L1 = chol(Q + spv I)), scale (max |Q_ii|).  C [np][np]; F1 [np][np]: the symmetric-filled factor (L1 below and L1' above
 * outside the diagonal 64 x 64 blocks, inv(L1_JJ) symmetric-filled inside them); D1 [nblk][64][64]: inv(L1_JJ), dense lower;
 * Et [mEcap][np] = E L1^-T; MM [mMld][mMld]: M = Et Et', lower triangle; Cp [np + 1], Ci [capC], Cv [capC]: the compressed rows of C. */
int  lcqp_hip_batch_read_setup(lcqp_hip_batch_t* b, int instance, int dims[9], double scal[2], double* C, double* F1, double* D1,
                               double* Et, double* MM, int* Cp, int* Ci, double* Cv);
/* The inverse factor Ti of the working-set matrix as the last lcqp_hip_batch_run left it (Ti'Ti = inv(Et_W Et_W')):
 * dims[2] = nT (rows of Ti), ns (slots in use, free ones inside included); slot_row [capS] (row of E held by a slot, -1: free),
 * crow [capS] (the row of Ti appended together with the slot), row_slot [mE] (-1: not in the factor), Ti [capS][capS]. */
int  lcqp_hip_batch_read_working_set(lcqp_hip_batch_t* b, int instance, int dims[2], int* slot_row, int* crow, int* row_slot, double* Ti);
/* The state of the ADMM fallback of the dense subsolver (qp_build_K, qp_admm, qp_adapt_rho) as the last QP that ran it left it; the polish
 * writes none of it.  Both streams are synchronised, nothing is launched, any pointer may be NULL (buffers NULL: the sizes).
 * dims[6] = np, nblk, mEcap, the instance's mE, kReady (FK holds the factor of the rho vector in place), setupFail; scal[3] = sigma,
 * rhoAdmm, scale.  FK [np][np]: L_K, the factor of K = Q + sigma I + E' diag(rhov) E, symmetric-filled, its diagonal 64 x 64 blocks
 * holding their inverses (as F1).  rhov, l, u (the bounds of the stacked rows), ya, za, dy (the change of ya in the last iteration)
 * [mEcap]; xa, dx (the change of xa in the last iteration) [np].  LCQP_INVALID_ARGUMENT: NULL handle, instance out of range;
 * LCQP_LCQPOBJECT_NOT_SETUP: no setup belongs to the data in place (before lcqp_hip_batch_setup / lcqp_hip_batch_run). */
int  lcqp_hip_batch_read_admm(lcqp_hip_batch_t* b, int instance, int dims[6], double scal[3], double* FK, double* rhov, double* l, double* u,
                              double* xa, double* ya, double* za, double* dy, double* dx);
/* The state of the active-set polish (qp_polish / qp_solve in lcqp_dev.hpp) as the last solve left it, accepted or given up.  Both streams
 * are synchronised, nothing is launched, any pointer may be NULL (buffers NULL: the sizes).
 * dims[12] = np, mEcap, the instance's mE, nT, ns, ndep, rnReady, nHot, haveSolution, rowsInLds, nV, capS; scal[7] = spv (sigma_p), then the six work sums of the instance
 * (lcqp_hip_batch_work_sums; [4]: rows of E read by the residual sweeps).
 * V [8][np]: V_XT (the polish's x), V_XS (x of the last residual sweep: the margins belong to it), V_XREF, V_R1S, V_GS, V_ATY, V_QXN, V_XQ.
 * M [10][mEcap]: M_YT, M_EX, M_EXS, M_MG (screening margins), M_RN, M_HOTV, M_YLV, M_L, M_U, M_YQ.  I [5][mEcap]: I_STT, I_ST, I_DEP,
 * I_SLOT, I_HOTC.  rowsInLds = 1: the homotopy kernel of this shape (np <= 256, mEcap <= 640, 4 capS <= 2048) keeps yt, ex, mg and st
 * in LDS for the whole launch, and M_YT, M_EX, M_MG, I_STT are STALE after lcqp_hip_batch_run / _resolve (they hold what the last
 * one-piece rebuild of a factor saved); every other array is current.  LCQP_INVALID_ARGUMENT / LCQP_LCQPOBJECT_NOT_SETUP as
 * lcqp_hip_batch_read_admm. */
int  lcqp_hip_batch_read_polish(lcqp_hip_batch_t* b, int instance, int dims[12], double scal[7], double* V, double* M, int* I);
/* Constant-matrix setup: C = L'R + R'L (src/LCQProblem.cpp:622-623), phi expressions (:969-996) and the
 * two factorisations the subsolver reuses across every iterate (replaces qp.init's setup,
 * src/SubsolverQPOASES.cpp:152).  Asynchronous on the batch stream. */
int  lcqp_hip_batch_setup(lcqp_hip_batch_t* b);
/* LCQProblem::runSolver for all instances, src/LCQProblem.cpp:444-560.  Asynchronous on the batch
 * stream; includes setup if it has not run since the last load. */
int  lcqp_hip_batch_run(lcqp_hip_batch_t* b);
/* Re-solves: the matrices stay, the vectors change (receding horizon, parameter sweeps).
 * lcqp_hip_batch_update replaces every vector of instances [first, first+count) and nothing else: the arguments of lcqp_hip_batch_load
 * without Q, L, R, A -- the same packing, the same meaning of NULL (g is required).  The batch must hold problems (load or
 * generate_synthetic; else LCQP_LCQPOBJECT_NOT_SETUP).  The set of variables with a finite lb or ub must be the one the instance was
 * loaded with (box bounds are rows of the factored matrices): otherwise LCQP_INVALID_ARGUMENT with a message, and nothing is written.
 * Values, and finite against infinite on lbA / ubA / ubL / ubR, may change freely; lbL / lbR of -inf are refused as in load. */
int  lcqp_hip_batch_update(lcqp_hip_batch_t* b, int first, int count, const double* g,
                           const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                           const double* lbA, const double* ubA, const double* lb, const double* ub,
                           const double* x0, const double* y0);
/* Solve every instance again on the setup that is in place: ONE kernel (k_refresh) stands where the setup kernels of lcqp_hip_batch_run
 * stand, then the homotopy launch.  Asynchronous on the batch stream.  When no setup belongs to the matrices and options in place (none
 * yet, or a load / generate_synthetic / set_options since) this is lcqp_hip_batch_run.
 * mode 0 (cold): every instance starts as after a fresh load -- the result is the bits of a new batch object given the same data by
 *   lcqp_hip_batch_load and solved by lcqp_hip_batch_run.
 * mode 1 (warm): an instance whose last run returned LCQP_SUCCESSFUL_RETURN starts at its last x with the penalty rho0[i] (host array [B],
 *   every entry finite and > 0, else LCQP_INVALID_ARGUMENT) or, with rho0 == NULL, its last rhoOpt; it skips the zero-penalty QP, and its first QP is a hot start from the stored
 *   point, working set and inverse factor.  Its x0 / y0 are not read.  In the reference's terms: runSolver with x0, y0 = the last
 *   solution, solveZeroPenaltyFirst = false, initialPenaltyParameter = that penalty.  Every other instance runs cold as in mode 0.
 * lcqp_hip_batch_last_timing reports k_refresh as setup_ms.
 * After lcqp_hip_batch_update_matrices (below), mode 1 is the same warm start around new matrices: the five setup kernels run, with
 * k_prepare_warm in front, and lcqp_hip_batch_last_timing reports them as setup_ms. */
int  lcqp_hip_batch_resolve(lcqp_hip_batch_t* b, int mode, const double* rho0);
/* Re-solves after a change of the matrices (an outer SQP loop that re-linearises, a layer whose Q / A are trained).
 * lcqp_hip_batch_update_matrices replaces the named matrices of instances [first, first+count) and nothing else: Q, L, R, A as
 * lcqp_hip_batch_load takes them (host arrays [count][rows][nV]), NULL: the matrix stays.  No vector, status, multiplier, stored point or
 * statistic is touched.  Checked before any device call, in this order, and nothing is written when a check fails: every matrix NULL
 * (LCQP_INVALID_ARGUMENT), NULL handle (LCQP_LCQPOBJECT_NOT_SETUP), a range outside the batch (LCQP_INVALID_ARGUMENT), an instance of the
 * range that holds no problem (LCQP_LCQPOBJECT_NOT_SETUP), only matrices the batch has no rows of (LCQP_INVALID_ARGUMENT).
 * Afterwards no setup and no solve belong to the data in place: the sensitivity, Jacobian and adjoint calls answer
 * LCQP_LCQPOBJECT_NOT_SETUP until the next solve.  What the last solve stored on the device is kept, and the next
 * lcqp_hip_batch_resolve(mode 1) starts from it: a full setup on the new matrices in which an instance whose last run returned
 * LCQP_SUCCESSFUL_RETURN keeps its x, multipliers, statuses and penalty (rho0 as above), with an EMPTY inverse factor -- its first QP
 * rebuilds the factor in one piece from the stored working set and the new matrices.  In the reference's terms: runSolver on the new data
 * with x0, y0 = the last solution, solveZeroPenaltyFirst = false, initialPenaltyParameter = that penalty.  Every other instance, and every
 * instance of a mode 0 resolve or a run, starts cold: the bits of a new batch object given the same data by lcqp_hip_batch_load.
 * lcqp_hip_batch_update and lcqp_hip_batch_update_matrices may precede the resolve in either order; a load, generate_synthetic or
 * set_options in between makes it a cold run. */
int  lcqp_hip_batch_update_matrices(lcqp_hip_batch_t* b, int first, int count, const double* Q, const double* L, const double* R, const double* A);
/* Solution sensitivities (DESIGN.md section 3a'): adjoint derivatives of the x the last run / resolve returned with respect to g and to
 * the bounds its working set W sits on.  For instance i and right-hand side k, v[i][k] = dl/dx is an upstream gradient ([B][nrhs][nV], host);
 *   dg[i][k]   [nV]                 = dl/dg
 *   db[i][k]   [nV + nC + 2 nComp]  entry r = dl/d(the bound row r sits on), zero for rows outside W; the reference's dual layout
 *                                    (box rows first, then A, L, R)
 *   side[i]    [nV + nC + 2 nComp]  0 outside W, -1 at the lower bound, +1 at the upper bound, 2 equality (both bounds move the row)
 *   info[i]    0 when x is locally a smooth function of (g, b_W) given by the equality-constrained QP on W; else a sum of
 *              1  the last run did not return 0, or nothing was solved yet: the outputs of the instance are zero
 *              2  active rows flagged linearly dependent are not in W: the derivative is the one with those rows dropped
 *              4  an inequality-type row of W (both rows of a biactive complementarity pair included) has |y_r| <= 1e-9 (1 + |y|_inf)
 *              8  a complementarity pair has neither side in W
 * db, side, info may be NULL.  One launch of k_sensitivity on the batch stream behind whatever is queued there; synchronous on return.  The
 * call reads the state of the batch and changes none of it: a warm resolve after it returns the bits it returns without it.
 * LCQP_INVALID_ARGUMENT: NULL handle, v or dg, or nrhs < 1.  LCQP_LCQPOBJECT_NOT_SETUP: no run / resolve on this object yet, or a load /
 * generate_synthetic / set_options since the last one.  LCQP_HIP_ERROR: a HIP call failed (no device). */
int  lcqp_hip_batch_sensitivity(lcqp_hip_batch_t* b, int nrhs, const double* v, double* dg, double* db, int* side, int* info);
/* kernel time of the last lcqp_hip_batch_sensitivity / _sensitivity_blocked / _jacobian / _adjoint_blocked / _jacobian_duals call of this
 * object or of their device twins, ms (HIP events around k_sensitivity, k_sensitivity_blk or k_sensitivity_blk_dual, the copies excluded; a Jacobian that went in chunks: the sum over its launches) */
int  lcqp_hip_batch_sensitivity_timing(lcqp_hip_batch_t* b, float* kernel_ms);
/* lcqp_hip_batch_sensitivity for many vectors (DESIGN.md section 3a'''): the same arguments, layouts, flags and return codes, checked in the
 * same order before any device call.  The vectors of an instance go through k_sensitivity_blk in panels of 16 (LCQP_SENS_PANEL; the last
 * panel padded with zero columns): the correction as block x panel products on the fp64 matrix cores, each 64 x 64 block of the factor
 * read once per panel instead of once per vector.  The results equal lcqp_hip_batch_sensitivity's to rounding (the bound of DESIGN.md
 * section 2), NOT to the bit: the sums are formed in another order.  Within this entry point a vector's result does not depend on the
 * other vectors of the call or on its place among them, bit for bit.  side and info are those of lcqp_hip_batch_sensitivity.
 * Padded sizes above 512 (nV > 512: np = 1024 / 2048 / 4096) have no room for a panel in LDS: there this entry point launches
 * k_sensitivity and returns the bits of lcqp_hip_batch_sensitivity.  With one or a few vectors the vector kernel is the faster one (a
 * panel is then mostly zero columns). */
#define LCQP_SENS_PANEL 16
int  lcqp_hip_batch_sensitivity_blocked(lcqp_hip_batch_t* b, int nrhs, const double* v, double* dg, double* db, int* side, int* info);
/* The full solution Jacobians of the instances [first, first + count): the blocked kernel on the unit vectors, which it generates on the
 * device (nothing is uploaded).
 *   Jg[i][k][j]  [count][nV][nV]   d x*_k / d g_j of instance first + i
 *   Jb[i][k][r]  [count][nV][nd]   d x*_k / d (the bound row r of the dual layout sits on), zero outside W; may be NULL
 *   side [count][nd], info [count]  as lcqp_hip_batch_sensitivity; may be NULL
 * The staging on the device is bounded: the call loops over chunks of instances whose staging stays below
 * LCQP_JACOBIAN_STAGING_BYTES (at least one instance per chunk), one launch and one download per chunk; the results do not depend on the
 * chunking.  nV > 512: k_sensitivity on an uploaded identity, in chunks of unit vectors under the same cap; a sub-range then costs the
 * launches of the whole batch (the vector kernel has no instance offset).
 * LCQP_INVALID_ARGUMENT: NULL handle or Jg, first < 0, count < 1, first + count > B.  LCQP_LCQPOBJECT_NOT_SETUP as lcqp_hip_batch_sensitivity. */
#define LCQP_JACOBIAN_STAGING_BYTES (1ull << 30)
int  lcqp_hip_batch_jacobian(lcqp_hip_batch_t* b, int first, int count, double* Jg, double* Jb, int* side, int* info);
/* another staging cap for this object's Jacobian and adjoint calls and for the two chunks of staging of a host load / update (0: the
 * default); for tests of the chunking and for small devices */
int  lcqp_hip_batch_set_jacobian_staging(lcqp_hip_batch_t* b, size_t bytes);
/* The full adjoint (DESIGN.md section 3a''''): lcqp_hip_batch_sensitivity with nrhs = 1, extended by upstream gradients on the returned duals
 * and by the gradients in the matrices.  At the returned point x, y_W solve  H x + g - E_W' y_W = 0,  E_W x = b_W  (H = Q + sigma_p I; y in the
 * reference's layout, box rows first; the returned y is the multiplier of this penalty-free system).  For a loss l with vx = dl/dx [B][nV] and
 * vy = dl/dy [B][nd] (host; vy may be NULL = zero; its entries outside W are ignored: those duals are identically zero on the branch):
 *   d, mu with  H d + E_W' mu = vx,  E_W d = -vy_W;     dg = dl/dg = -d,   db_W = dl/db_W = mu   (dg, db, side, info as lcqp_hip_batch_sensitivity)
 *   dQ = 1/2 (dg x' + x dg')                             the symmetric derivative; symmetric to the bit
 *   row r of dA / dL / dR = -(db_r x + y_r dg)           for the rows with side != 0, exactly zero elsewhere; box rows have no matrix
 * reduce = 0: dQ [B][nV][nV], dA [B][nC][nV], dL and dR [B][nComp][nV], computed in chunks of instances whose staging stays below the cap of
 * lcqp_hip_batch_set_jacobian_staging (the results do not depend on the chunking).  reduce = 1: [nV][nV], [nC][nV], [nComp][nV]: the sums over
 * the batch (one matrix shared by the instances), formed on the device in the order of the batch -- the same bits on every call; an instance
 * with info & 1 contributes zeros, every other flagged instance what the kernels computed.  Each of dQ, dA, dL, dR may be NULL.
 * With vy == NULL and no matrix output the call is lcqp_hip_batch_sensitivity with nrhs = 1, to the bit.  It reads the batch and changes none
 * of it.  lcqp_hip_batch_sensitivity_timing then reports the sum of its kernels.
 * LCQP_INVALID_ARGUMENT: NULL handle, vx or dg, or reduce outside 0 / 1.  LCQP_LCQPOBJECT_NOT_SETUP as lcqp_hip_batch_sensitivity.  Both are
 * decided before any device call. */
int  lcqp_hip_batch_adjoint(lcqp_hip_batch_t* b, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                            int reduce, double* dQ, double* dA, double* dL, double* dR);
/* The blocked adjoint (DESIGN.md section 3a'''', "Panels with gradients on y"): lcqp_hip_batch_sensitivity_blocked with upstream gradients on
 * the duals.  vx [B][nrhs][nV], vy [B][nrhs][nd] (host; either may be NULL = zero, not both; entries of vy outside W are not read);
 * dg [B][nrhs][nV], db [B][nrhs][nd], side [B][nd], info [B] as lcqp_hip_batch_adjoint gives them for one pair.  The pairs of an instance
 * go through k_sensitivity_blk_dual in panels of LCQP_SENS_PANEL; with vx == NULL the forward substitution is not run.  A pair's
 * result does not depend on the other pairs of the call or on its place among them, bit for bit.  With vy == NULL the call is
 * lcqp_hip_batch_sensitivity_blocked, to the bit.  nV > 512: k_sensitivity<NCH, true> and its bits (a NULL vx is a zero panel there).
 * LCQP_INVALID_ARGUMENT: NULL handle or dg, vx and vy both NULL, nrhs < 1.  LCQP_LCQPOBJECT_NOT_SETUP as lcqp_hip_batch_sensitivity. */
int  lcqp_hip_batch_adjoint_blocked(lcqp_hip_batch_t* b, int nrhs, const double* vx, const double* vy, double* dg, double* db, int* side, int* info);
/* The dual rows of the solution Jacobian for the instances [first, first + count): D y* / D (g, b_W), the blocked kernel on the unit
 * vectors of the slot space, which it generates on the device (nothing is uploaded, no forward substitution).
 *   Jyg[i][r][j]  [count][nd][nV]   d y*_r / d g_j of instance first + i
 *   Jyb[i][r][s]  [count][nd][nd]   d y*_r / d (the bound row s of the dual layout sits on); may be NULL
 *   side [count][nd], info [count]  as lcqp_hip_batch_sensitivity; may be NULL
 * Rows (and, in Jyb, columns) outside W are zero.  Jyg[i][r][j] is Jb[i][j][r] of lcqp_hip_batch_jacobian to rounding: both are the block
 * (K^-1)_{x lambda}.  The staging on the device holds one row per slot of the working set (at most capS per instance, not nd) and is
 * chunked over instances under the cap of lcqp_hip_batch_set_jacobian_staging; the results do not depend on the chunking.  nV > 512:
 * k_sensitivity<NCH, true> on uploaded unit vectors of the rows in W, in chunks of vectors under the same cap, on the whole batch.
 * LCQP_INVALID_ARGUMENT: NULL handle or Jyg, first < 0, count < 1, first + count > B.  LCQP_LCQPOBJECT_NOT_SETUP as lcqp_hip_batch_sensitivity. */
int  lcqp_hip_batch_jacobian_duals(lcqp_hip_batch_t* b, int first, int count, double* Jyg, double* Jyb, int* side, int* info);
/* out[0] = full setups, out[1] = homotopy launches this object has issued (host counters) */
int  lcqp_hip_batch_launch_counts(lcqp_hip_batch_t* b, int out[2]);
/* Hint of a caller that keeps several batch objects in flight (BatchPipeline): the setup of this object will run beside the homotopy
 * kernel of another one.  The library then launches the setup kernels that fit into the registers and LDS ONE finished instance frees on
 * a compute unit (the streamed form of Et = E L1^-T instead of the register-resident one), so that the setup starts in the gaps of the
 * other launch instead of behind it (+10 % through a two-deep pipeline at B = 1024, profiles/round6/setup/pipelined_variants.log).  The
 * results are the same bits either way; the default (0) is the faster setup of a batch that runs alone. */
int  lcqp_hip_batch_set_overlapped(lcqp_hip_batch_t* b, int overlapped);
int  lcqp_hip_batch_synchronize(lcqp_hip_batch_t* b);
/* time of the last run measured with HIP events on the batch stream, ms: setup_ms = the setup kernels, solve_ms = the homotopy launch */
int  lcqp_hip_batch_last_timing(lcqp_hip_batch_t* b, float* setup_ms, float* solve_ms);
/* getPrimalSolution / getDualSolution / getOutputStatistics, src/LCQProblem.cpp:1485-1504,1519:
 * x[B][nV], y[B][nV+nC+2nComp], stats[B]; returnValue of runSolver is stats[i].returnValue. */
int  lcqp_hip_batch_get_solution(lcqp_hip_batch_t* b, double* x, double* y, lcqp_stats_t* stats);

/* ---- Device-pointer entry points of the dense batch (DESIGN.md section 3a'''''): the twins of lcqp_hip_batch_load / _update / _get_solution /
 * _sensitivity(_blocked) / _adjoint whose data pointers are DEVICE pointers.  Layouts, defaults for absent vectors, return codes and the order
 * of the checks are the host twins'; the pools, the solution and every gradient hold the bits the host twins leave.  The differences:
 *   pointers  every non-NULL data pointer is plain device memory (hipMalloc) of the handle's device that holds the bytes the call moves; pinned or
 *             managed host memory, another device's memory and pageable memory are refused with LCQP_INVALID_ARGUMENT and a message, before
 *             anything is enqueued.  dQ, dA, dL, dR must be 16-byte aligned (the adjoint kernels store pairs of doubles).
 *   stream    the caller's hipStream_t (NULL: the legacy default stream).  The handle's stream waits for an event recorded on it, the work is
 *             enqueued on the handle's stream, and the caller's stream waits for an event recorded behind it: inputs are read after their
 *             producers, outputs are visible to what the caller enqueues next, and no call waits on the host -- except load_device and
 *             update_device, which read one status word (and, for a load with box bounds, the flags of the bounded variables) back.
 *   shared    (load) bits 1, 2, 4, 8 for Q, A, L, R: the pointer holds ONE matrix for all `count` instances (broadcast by the pack kernel).
 *   NULL matrix (load) leaves that block of each instance as the pool holds it; every instance of the range must then already hold a problem,
 *             else the host twin's code for the missing matrix is returned.  g stays mandatory.
 *   validation the value checks (-inf in lbL / lbR: LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND; update: the set of box-bounded variables stays,
 *             LCQP_INVALID_ARGUMENT) run in one kernel over the whole range before anything is written; on a failure nothing is written, and
 *             the message names the lowest (instance, variable), as the host twin's does.
 *   NULL handle: LCQP_LCQPOBJECT_NOT_SETUP from all five.
 * The two paths mix on one handle: the host state (which instances hold problems, the box flags, the lbL / lbR flags) is kept in step.
 * sensitivity_device: blocked != 0 is lcqp_hip_batch_sensitivity_blocked.  v [B][nrhs][nV], vx [B][nV], vy [B][nd] are read where they lie;
 * stats of get_solution_device is a device array of B lcqp_stats_t.  The kernel time of sensitivity_device / adjoint_device is formed when
 * lcqp_hip_batch_sensitivity_timing asks for it (that call then waits for the kernels). */
int  lcqp_hip_batch_load_device(lcqp_hip_batch_t* b, int first, int count, int shared,
                                const double* Q, const double* g, const double* L, const double* R,
                                const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                                const double* A, const double* lbA, const double* ubA,
                                const double* lb, const double* ub, const double* x0, const double* y0, void* stream);
int  lcqp_hip_batch_update_device(lcqp_hip_batch_t* b, int first, int count, const double* g,
                                  const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                                  const double* lbA, const double* ubA, const double* lb, const double* ub,
                                  const double* x0, const double* y0, void* stream);
/* lcqp_hip_batch_update_matrices on device arrays, under the rules above: shared as in load_device, a NULL matrix stays, the checks and
 * their order are the host twin's (a bit of shared outside 1 | 2 | 4 | 8: LCQP_INVALID_ARGUMENT), nothing waits on the host. */
int  lcqp_hip_batch_update_matrices_device(lcqp_hip_batch_t* b, int first, int count, int shared, const double* Q, const double* L,
                                           const double* R, const double* A, void* stream);
int  lcqp_hip_batch_get_solution_device(lcqp_hip_batch_t* b, double* x, double* y, lcqp_stats_t* stats, void* stream);
int  lcqp_hip_batch_sensitivity_device(lcqp_hip_batch_t* b, int blocked, int nrhs, const double* v,
                                       double* dg, double* db, int* side, int* info, void* stream);
int  lcqp_hip_batch_adjoint_device(lcqp_hip_batch_t* b, const double* vx, const double* vy,
                                   double* dg, double* db, int* side, int* info,
                                   int reduce, double* dQ, double* dA, double* dL, double* dR, void* stream);
/* The twins of lcqp_hip_batch_adjoint_blocked, _jacobian and _jacobian_duals under the same rules: device arrays in and out, the bits of the
 * host twins, NULL handle: LCQP_LCQPOBJECT_NOT_SETUP.  The Jacobians go in the host twins' chunks of instances; a small kernel
 * (k_pack_dual_rows) moves the staged rows of the dual Jacobian to their rows of Jyg / Jyb, which are zero-filled on the device before it.
 * lcqp_hip_batch_sensitivity_timing reports the sum over the chunks' kernels, as after the host twins (a call with more than one chunk
 * waits on the host for each chunk's kernel but the last: the next chunk reuses the staging and the events).  nV > 512 (no blocked kernel): the Jacobians are formed by the host
 * twins and copied to the device; those two calls then wait on the host. */
int  lcqp_hip_batch_adjoint_blocked_device(lcqp_hip_batch_t* b, int nrhs, const double* vx, const double* vy,
                                           double* dg, double* db, int* side, int* info, void* stream);
int  lcqp_hip_batch_jacobian_device(lcqp_hip_batch_t* b, int first, int count, double* Jg, double* Jb, int* side, int* info, void* stream);
int  lcqp_hip_batch_jacobian_duals_device(lcqp_hip_batch_t* b, int first, int count, double* Jyg, double* Jyb, int* side, int* info, void* stream);

/* per-iterate tracking of one instance when options.storeSteps != 0 (LCQProblem::storeSteps,
 * src/LCQProblem.cpp:1365-1378; OutputStatistics tracking vectors, src/OutputStatistics.cpp:131-164): scalars[len][8] =
 * (|statk|_inf, phi, rho, alphak, objective, merit, |pk|_inf, iterations of the last QP), x[len][nV] = xk at the top of
 * every pass of the loop; at most cap rows are copied. */
int  lcqp_hip_batch_get_trace(lcqp_hip_batch_t* b, int instance, int cap, double* scalars, double* x, int* len);
/* per-instance cycle counters of the homotopy kernel's phases, out[B][16]; all zero unless the library was
 * built with -DLCQP_PROFILE (tools/gpu.py phase_profile) */
int  lcqp_hip_batch_read_profile(lcqp_hip_batch_t* b, unsigned long long* out);
/* raw HIP stream (hipStream_t) the batch launches on, for event timing by the caller */
void* lcqp_hip_batch_stream(lcqp_hip_batch_t* b);
/* algorithmic HBM bytes of the last run, from the work counters the kernels keep */
double lcqp_hip_batch_algorithmic_bytes(lcqp_hip_batch_t* b);
/* the work sums that enter it, summed over the batch (counted by the kernel): out[0] = rows of Et read by the corrections (twice the
 * rows of the factor for a full correction, once plus the rows that left for a predicted one), out[1] = entries of the inverse factor read by
 * the corrections (its triangle, n_T (n_T + 1) / 2 per pass; full rows beyond 256 slots), out[2] = bytes moved by the working-set updates (and the entries of M a predicted correction
 * reads), out[3] = number of working-set updates, out[4] = rows of E read by the residual sweeps (stage 1: unscreened inactive rows;
 * stage 2: active rows), out[5] = triangular solves with L1 (two per full correction, one per predicted correction) */
int    lcqp_hip_batch_work_sums(lcqp_hip_batch_t* b, double out[6]);

/* ------------------------------------------------------------------------------------------------
 * Building blocks exposed for parity tests and micro-benchmarks (each is one kernel launch over a
 * batch of independent instances; host pointers, synchronous).  Three more test and diagnostic entry points sit with the objects they
 * read: lcqp_hip_batch_read_setup / lcqp_hip_batch_read_working_set (and lcqp_hip_qp_read_setup / lcqp_hip_qp_read_working_set) copy the
 * constant matrices of the setup kernels and the inverse factor of the working-set matrix back as they lie on the device
 * (tests/test_gpu_setup.py); lcqp_hip_batch_read_admm (and lcqp_hip_qp_read_admm) does the same for the factor L_K, the rho vector and
 * the iterates of the ADMM fallback (tests/test_gpu_admm.py).  They launch nothing.
 * ---------------------------------------------------------------------------------------------- */
/* Utilities::AffineLinearTransformation for symmetric A, src/Utilities.cpp:176-186: d = alpha*A*b + c */
int lcqp_hip_util_symv(int batch, int n, double alpha, const double* A, const double* b, const double* c, double* d);
/* Utilities::TransponsedMatrixMultiplication with p = 1, src/Utilities.cpp:62-72: c = A' * b (A is m x n) */
int lcqp_hip_util_gemv_t(int batch, int m, int n, const double* A, const double* b, double* c);
/* Utilities::MatrixMultiplication with p = 1, src/Utilities.cpp:38-47: c = A * b */
int lcqp_hip_util_gemv(int batch, int m, int n, const double* A, const double* b, double* c);
/* the row sweep of the subsolver's trials on its own (wg_rows through a row list, scalars indexed by row): for the nlist rows r = list[b][k]
 * of every instance, dots[b][r] = A_r . x (other entries of dots stay) and outT[b] = sum_k coef[b][r] A_r; x, coef, dots, outT may be NULL */
int lcqp_hip_util_rows_list(int batch, int m, int n, const double* A, const int* list, int nlist, const double* x, const double* coef,
                            double* dots, double* outT);
/* Utilities::MatrixSymmetrizationProduct, src/Utilities.cpp:104-116: C = A'B + B'A (A, B are m x n) */
int lcqp_hip_util_symm_product(int batch, int m, int n, const double* A, const double* B, double* C);
/* ---- CSC utilities on the device (host pointers, synchronous) ----
 * Handle on one CSC matrix (fields of the reference's `csc`, src/Utilities.cpp:469-484) and its transpose. */
typedef struct lcqp_hip_csc lcqp_hip_csc_t;
lcqp_hip_csc_t* lcqp_hip_csc_create(int m, int n, int nnz, const int* p, const int* i, const double* x, int device);
void lcqp_hip_csc_destroy(lcqp_hip_csc_t* M);
/* d = alpha * op(A) b + c (c may be NULL).  transposed == 0: Utilities::MatrixMultiplication(csc) src/Utilities.cpp:49-59;
 * transposed != 0: TransponsedMatrixMultiplication(csc) :75-82 and, for symmetric S, AffineLinearTransformation(csc)
 * :189-199 (QuadraticFormProduct :228-241 is b'd).  repeat > 1 re-launches for timing, *ms = time per launch. */
int lcqp_hip_csc_apply(lcqp_hip_csc_t* M, int transposed, double alpha, const double* b, const double* c, double* d,
                       int repeat, float* ms);
/* micro-benchmark of the row sweep on device-resident random data (batch matrices of m x n):
 * mode 1 = A x (dots), 2 = A'y (axpy), 3 = both in one sweep; *ms = time per launch */
int lcqp_hip_bench_rows(int batch, int m, int n, int mode, int repeat, float* ms);
/* Cholesky factorisation + nrhs back-solves of an SPD n x n matrix: x = K^-1 b (the factor-once /
 * back-solve-many kernel pair).  repeat > 1 re-runs the back-solve for timing; *ms gets the
 * per-back-solve kernel time. */
int lcqp_hip_chol_solve(int batch, int n, const double* K, const double* b, double* x, int repeat, float* ms);


/* ------------------------------------------------------------------------------------------------
 * Batch of B independent SPARSE LCQPs that share one sparsity pattern: the OSQP_SPARSE arm of the reference
 * (src/LCQProblem.cpp:929-960: no box constraints, nC + 2 nComp duals) on the device -- ADMM on the quasi-definite KKT
 * matrix + active-set polish (the role of SubsolverOSQP, src/SubsolverOSQP.cpp:124-200), CSR/CSC products, band LDL' in a
 * reverse Cuthill-McKee ordering computed here once per pattern.  Pattern arrays are the CSC arrays the reference holds
 * (Q_sparse and the stacked A_sparse = [A; L; R], src/LCQProblem.cpp:629-723; Q full symmetric).  Three factorisation engines, chosen
 * here per pattern: a band of half width <= 63; such a band plus at most 16 dense border nodes (rows or variables that touch many
 * others: the arrow of examples/OptimizeOnCircle.cpp); and, for any other pattern -- as the reference's OSQP arm takes any
 * (src/SubsolverOSQP.cpp:136-152) --, a general sparse LDL' (dense fronts, one wavefront per instance: lcqp_sparse_general.hpp; a 2-D
 * grid with 16 384 variables is one).  Its ordering is nested dissection; where that would need a front of more than 576 rows or a factor
 * of 2^28 entries -- KKT graphs of small diameter: hundreds of small blocks coupled through a few dozen shared variables --, or where it
 * lowers the largest front by a size class of the kernels and the flops with it, a minimum-degree ordering takes its place, provided it
 * needs no more fronts (lcqp_hip_sparse_general_ordering says which one runs).  Returns NULL only when the ordering left by these rules
 * still exceeds 576 rows in a front or 2^28 entries in the factor or the stack of update blocks -- many dense rows over many variables --
 * (lcqp_hip_sparse_last_error() says so): the host layer runs such a problem on the dense kernels, which take nV <= 4096.
 *
 * Re-solves on the matrices in place (the sparse twin of lcqp_hip_batch_update / _resolve / _launch_counts):
 *   lcqp_hip_sparse_update   new g, bounds, x0, y0 for instances [first, first + count): the argument list of lcqp_hip_sparse_load without
 *                            Qx and Ax, same packing, NULL as there.  The stored solution, working set and factors of the instances stay.
 *                            Refused before anything is written: a range outside the batch (LCQP_INVALID_ARGUMENT), an instance never loaded
 *                            (LCQP_LCQPOBJECT_NOT_SETUP), g == NULL (LCQP_INVALID_OBJECTIVE_LINEAR_TERM), -inf in lbL / lbR
 *                            (LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND).
 *   lcqp_hip_sparse_resolve  solves again (asynchronous, like run).  While the setup on the device belongs to the matrices and options in
 *                            place (run and resolve set the mark, load and set_options clear it) ONE kernel stands where the setup kernel
 *                            of a run stands: it forms what depends on the bounds and rebuilds the ADMM KKT factor only for instances in
 *                            which a row changed its class (free, equality, other); last_timing reports it as setup_ms.  Otherwise the
 *                            call is lcqp_hip_sparse_run.  mode 0 (cold): the bits of a fresh handle given the same data by load and solved
 *                            by run.  mode 1 (warm): an instance whose last run returned 0 starts at its last solution, working set, polish
 *                            factor and penalty -- rho0 [B] (host; every entry finite and > 0, else LCQP_INVALID_ARGUMENT) or NULL for its
 *                            last rhoOpt -- without the zero-penalty QP: runSolver with x0, y0 = the last solution,
 *                            solveZeroPenaltyFirst = false, initialPenaltyParameter = rho.  Every other instance runs cold.
 *   lcqp_hip_sparse_update_values   new values of the matrices on the pattern of the handle, for instances [first, first + count) of a batch
 *                            that holds problems (the sparse twin of lcqp_hip_batch_update_matrices): Qx [count][nnzQ], Ax [count][nnzA]
 *                            as lcqp_hip_sparse_load takes them, NULL: the array stays.  Only those values are written: no vector, no
 *                            status, multiplier, point, statistic or factor.  Checked before any device call, in this order: neither array
 *                            (LCQP_INVALID_ARGUMENT), NULL handle (LCQP_LCQPOBJECT_NOT_SETUP), the range (LCQP_INVALID_ARGUMENT), an instance
 *                            never loaded (LCQP_LCQPOBJECT_NOT_SETUP); a refused call changes nothing.  The setup and the solve no longer
 *                            belong to the data in place: the sensitivity, panel, Jacobian, adjoint and probe calls answer
 *                            LCQP_LCQPOBJECT_NOT_SETUP until the next solve.  With Qx the ordering is chosen again from the new diagonals.
 *                            A cold lcqp_hip_sparse_resolve behind it is lcqp_hip_sparse_run.  A WARM one (mode 1) launches ONE kernel where
 *                            the setup kernel of a run stands (one setup and one launch in launch_counts, setup_ms in last_timing): the
 *                            whole setup on the new values -- scales, regularisations, the ADMM KKT factor of every instance -- around the
 *                            stored point: an instance whose last run returned 0 keeps its x, multipliers, working set and penalty (rho0 as
 *                            above) but not its polish factor, which belongs to the old values; every other instance runs cold.
 *                            lcqp_hip_sparse_update and _update_values may precede the resolve in either order; a load or set_options in
 *                            between makes the resolve a run.
 *   lcqp_hip_sparse_launch_counts   out[0] full setups, out[1] homotopy launches this handle has issued.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lcqp_hip_sparse lcqp_hip_sparse_t;
lcqp_hip_sparse_t* lcqp_hip_sparse_create(int batch, int nV, int nC, int nComp, const int* Qp, const int* Qi,
                                          const int* Ap, const int* Ai, int device);
void lcqp_hip_sparse_destroy(lcqp_hip_sparse_t* s);
const char* lcqp_hip_sparse_last_error(void);
/* diagnostic (-DLCQP_SCHED_PROFILE builds, zeros otherwise): per phase of the scheduler (start, round, trial, factor, correct, QP end, idle polls)
 * clock ticks, wavefront steps, instances served: 21 values */
int  lcqp_hip_sparse_sched_profile(lcqp_hip_sparse_t* s, unsigned long long* out21);
int  lcqp_hip_sparse_bandwidth(const lcqp_hip_sparse_t* s);              /* half bandwidth of the KKT band */
int  lcqp_hip_sparse_lanes(const lcqp_hip_sparse_t* s);                  /* lanes of a wavefront per instance: 8, 16, 32 or 64 */
int  lcqp_hip_sparse_fronts(const lcqp_hip_sparse_t* s);                 /* fronts of the general sparse LDL' (a pattern that is neither banded nor bordered: nested dissection, dense fronts, a wavefront per instance); 0: a band engine */
/* the ordering of the general sparse LDL' of this handle: 0 a band engine (no general LDL'), 1 nested dissection, 2 minimum degree (the rule:
 * lcqp_hip_sparse_create above; the test hook LCQP_SPARSE_ORDERING=nd|md, read by create, forces one of the two on a pattern the general
 * engine takes and sends no band pattern there); -1: NULL handle */
int  lcqp_hip_sparse_general_ordering(const lcqp_hip_sparse_t* s);
int  lcqp_hip_sparse_border(const lcqp_hip_sparse_t* s);                 /* border nodes of the bordered band: the last positions of the ordering (0: plain band) */
/* perm[nV + nC + 2 nComp]: position -> node.  Two orderings of the band are prepared (the second, for Hessians that are safely definite by
 * their diagonals, puts every row behind one of its variables); this is the one the instances loaded so far select (before any load: the first) */
int  lcqp_hip_sparse_get_ordering(const lcqp_hip_sparse_t* s, int* perm);
int  lcqp_hip_sparse_set_options(lcqp_hip_sparse_t* s, const lcqp_options_t* opt);
/* loadLCQP, sparse overload (src/LCQProblem.cpp:390-441), values only: Qx [count][nnzQ], Ax [count][nnzA] in the CSC order of
 * the pattern; y0 [count][nC + 2 nComp]; NULL as in the reference.  load and update are the device path (lcqp_hip_sparse_load_device /
 * _update_device below) behind an upload, as lcqp_hip_batch_load: checks on the host over the whole range, then chunks of instances
 * (at most 16 MiB, at most half the cap of lcqp_hip_sparse_set_adjoint_staging) through two pinned slots to the pack kernels, in stream
 * order behind a run in flight, one synchronisation at the end.  A failing load or update leaves the range and the host state untouched. */
int  lcqp_hip_sparse_load(lcqp_hip_sparse_t* s, int first, int count, const double* Qx, const double* g, const double* Ax,
                          const double* lbA, const double* ubA, const double* lbL, const double* ubL, const double* lbR,
                          const double* ubR, const double* x0, const double* y0);
int  lcqp_hip_sparse_run(lcqp_hip_sparse_t* s);                          /* runSolver for every instance (asynchronous) */
int  lcqp_hip_sparse_update(lcqp_hip_sparse_t* s, int first, int count, const double* g,
                            const double* lbA, const double* ubA, const double* lbL, const double* ubL,
                            const double* lbR, const double* ubR, const double* x0, const double* y0);
int  lcqp_hip_sparse_update_values(lcqp_hip_sparse_t* s, int first, int count, const double* Qx, const double* Ax);
int  lcqp_hip_sparse_resolve(lcqp_hip_sparse_t* s, int mode, const double* rho0);
int  lcqp_hip_sparse_launch_counts(lcqp_hip_sparse_t* s, int out[2]);   /* full setups, homotopy launches */
/* Solution sensitivities of the sparse batch (DESIGN.md section 3a''; the twin of lcqp_hip_batch_sensitivity in this arm's conventions: no
 * box rows, m = nC + 2 nComp rows [A; L; R]): adjoint derivatives of the x the last run / resolve returned with respect to g and to the
 * bounds its stored working set W sits on.  For instance i and right-hand side k, v[i][k] = dl/dx is an upstream gradient
 * ([B][nrhs][nV], host);
 *   dg[i][k]   [nV]   = dl/dg
 *   db[i][k]   [m]    entry r = dl/d(the bound row r sits on), zero for rows outside W -- the derivative with respect to the bound as
 *                     the caller hands it to load / update, whatever the sign of this arm's duals
 *   side[i]    [m]    0 outside W, -1 at the lower bound, +1 at the upper bound, 2 equality (both bounds move the row)
 *   info[i]    0 when x is locally a smooth function of (g, b_W) given by the equality-constrained QP on W; else a sum of
 *              1  the last run did not return 0, or nothing was solved yet: the outputs of the instance are zero
 *              2  the refinement against [Q, E_W'; E_W, 0] did not reach its rounding floor: that matrix is singular or too ill-conditioned
 *                 (dependent rows in W, or a semidefinite Q with a null direction on W); the outputs are those of the regularised system
 *              4  an inequality-type row of W (both rows of a biactive complementarity pair included) has |y_r| <= 1e-9 (1 + |y|_inf)
 *              8  a complementarity pair has neither side in W
 * db, side, info may be NULL.  One launch of k_sparse_sensitivity on the handle's stream behind whatever is queued there; synchronous on
 * return.  The call reads the state of the batch: a cold or warm resolve after it returns the bits it returns without it.
 * LCQP_INVALID_ARGUMENT: NULL handle, v or dg, or nrhs < 1.  LCQP_LCQPOBJECT_NOT_SETUP: no run / resolve on this handle yet, or a load /
 * set_options since the last one (the mark of lcqp_hip_sparse_resolve).  LCQP_HIP_ERROR: a HIP call failed. */
int  lcqp_hip_sparse_sensitivity(lcqp_hip_sparse_t* s, int nrhs, const double* v, double* dg, double* db, int* side, int* info);
/* kernel time of the last lcqp_hip_sparse_sensitivity / _sensitivity_blocked / _jacobian / _adjoint_blocked / _jacobian_duals call of this handle, ms (HIP events around
 * k_sparse_sensitivity or k_sparse_sensitivity_blk, the copies excluded; a call that went in chunks: the sum over its launches) */
int  lcqp_hip_sparse_sensitivity_timing(lcqp_hip_sparse_t* s, float* kernel_ms);
/* lcqp_hip_sparse_sensitivity for many vectors (DESIGN.md section 3a''', "The sparse arm"): the same arguments, layouts, flags and return
 * codes, checked in the same order before any device call.  The vectors of an instance go through k_sparse_sensitivity_blk in panels of
 * lcqp_hip_sparse_sens_panel(s) columns (LCQP_SPARSE_SENS_PANEL by default; the last panel padded with zero columns): one lane group per
 * (instance, panel) pair, the band factor streamed once per panel instead of once per vector, the panel's columns as independent chains
 * of one sweep.  Per column the arithmetic is the sequence of k_sparse_sensitivity, so the results equal lcqp_hip_sparse_sensitivity's to
 * rounding (the bound of DESIGN.md section 2), NOT to the bit (the two kernels are compiled apart and contract differently; measured: the
 * last bits differ); within this entry point a vector's result does not depend on the other vectors of the call or on its place among
 * them, bit for bit.  side and info are those of lcqp_hip_sparse_sensitivity.  The staging
 * on the device is bounded as for lcqp_hip_sparse_jacobian.
 * The general sparse LDL' (lcqp_hip_sparse_fronts(s) > 0) has a panel kernel of its own, k_sparse_sensitivity_blk_general, behind a switch
 * of the handle that is OFF by default (lcqp_hip_sparse_set_general_panel): without it lcqp_hip_sparse_sens_panel returns 0 there, and this
 * entry point launches k_sparse_sensitivity and returns the bits of lcqp_hip_sparse_sensitivity. */
#define LCQP_SPARSE_SENS_PANEL 8
/* the panel width this handle's engine uses; 0 where the two entry points fall back to the vector kernel -- the general sparse LDL' of a
 * handle that has not switched its panel form on (NULL handle: 0) */
int  lcqp_hip_sparse_sens_panel(const lcqp_hip_sparse_t* s);
/* The panel form of the general sparse LDL' (DESIGN.md section 3a''', "The general engine"), per handle, off by default.  on = 1: on a
 * handle of the general engine lcqp_hip_sparse_sens_panel returns the panel width, and lcqp_hip_sparse_sensitivity_blocked and
 * lcqp_hip_sparse_jacobian go through the (instance, panel) work items of the band engines -- chunks under the staging cap, unit vectors
 * generated on the device, a sub-range at the cost of its own items -- with a panel sweep over the fronts as the solve.  Per column the
 * results equal the vector kernel's to rounding, not to the bit; within the panel form a column's result depends on nothing but that
 * column, bit for bit.  on = 0: the vector kernel again, and its bits.  A handle of a band engine accepts the call, and nothing changes.
 * The call makes no device call and touches neither the setup, nor the mark of the last solve, nor the stored solution.
 * LCQP_INVALID_ARGUMENT: NULL handle, or on outside 0 / 1. */
int  lcqp_hip_sparse_set_general_panel(lcqp_hip_sparse_t* s, int on);
/* the largest front (pivots + update rows) of the handle's general sparse LDL': which classes of the sweeps run (<= 64, <= 256, larger);
 * 0: a band engine (NULL handle: -1) */
int  lcqp_hip_sparse_max_front(const lcqp_hip_sparse_t* s);
int  lcqp_hip_sparse_sensitivity_blocked(lcqp_hip_sparse_t* s, int nrhs, const double* v, double* dg, double* db, int* side, int* info);
/* The full solution Jacobians of the instances [first, first + count): the panel kernel on the unit vectors, which it writes into its solve
 * panels on the device (nothing is uploaded).
 *   Jg[i][k][j]  [count][nV][nV]   d x*_k / d g_j of instance first + i
 *   Jb[i][k][r]  [count][nV][m]    d x*_k / d (the bound row r sits on), m = nC + 2 nComp, rows A, L, R; zero outside W; may be NULL
 *   side [count][m], info [count]  as lcqp_hip_sparse_sensitivity; may be NULL
 * Row k of Jg[i] and of Jb[i] is what lcqp_hip_sparse_sensitivity_blocked returns for v = e_k, to the bit.
 * The staging on the device (outputs and workspaces of the work items in flight) is bounded by the cap of
 * lcqp_hip_sparse_set_adjoint_staging, which governs the adjoint's chunks and these: the call loops over chunks of whole (instance, panel)
 * items, at least one per chunk -- a chunk may split an instance by columns --, one launch and one download per chunk; the results do not
 * depend on the chunking, bit for bit.  General sparse LDL' without lcqp_hip_sparse_set_general_panel: k_sparse_sensitivity on uploaded unit vectors, in chunks of columns under the
 * same cap; a sub-range then costs the launches of the whole batch (the vector kernel has no instance offset).
 * Both calls are synchronous on return, change nothing a run / resolve reads and leave lcqp_hip_sparse_launch_counts alone.
 * LCQP_INVALID_ARGUMENT: NULL handle or Jg, first < 0, count < 1, first + count > B.  Then LCQP_LCQPOBJECT_NOT_SETUP as
 * lcqp_hip_sparse_sensitivity.  Both are decided before any device call. */
int  lcqp_hip_sparse_jacobian(lcqp_hip_sparse_t* s, int first, int count, double* Jg, double* Jb, int* side, int* info);
/* The full adjoint of the sparse batch (DESIGN.md section 3a''''; the twin of lcqp_hip_batch_adjoint): lcqp_hip_sparse_sensitivity with
 * nrhs = 1, extended by upstream gradients on the returned duals and by the gradients on the stored entries of Q and of E = [A; L; R].  At the
 * returned point x, y_W solve  Q x + g - E_W' y_W = 0,  E_W x = b_W  (y as lcqp_hip_sparse_get_solution returns it, [m], m = nC + 2 nComp, rows
 * A, L, R: the multiplier of this penalty-free system).  For a loss l with vx = dl/dx [B][nV] and vy = dl/dy [B][m] (host; vy may be NULL =
 * zero; its entries outside W are ignored: those duals are identically zero on the branch):
 *   d, mu with  Q d + E_W' mu = vx,  E_W d = -vy_W;     dg = dl/dg = -d,   db_W = dl/db_W = mu   (dg, db, side, info as lcqp_hip_sparse_sensitivity)
 *   dQx[k] = 1/2 (dg_i x_j + x_i dg_j)                   stored entry k = (i, j) of Q: the symmetric derivative.  Q is given as the full
 *                                                        symmetric pattern; entries (i, j) and (j, i) are equal to the bit, and for a
 *                                                        symmetric perturbation Z on the pattern  dl = sum_k dQx[k] Z[k]
 *   dAx[k] = -(db_r x_j + y_r dg_j)                      stored entry k = (r, j) of the stacked pattern given to lcqp_hip_sparse_create, for
 *                                                        the rows with side != 0; exactly zero elsewhere
 * Both are in the order of Qx / Ax of lcqp_hip_sparse_load (the caller's CSC order).  reduce = 0: dQx [B][nnzQ], dAx [B][nnzA], computed in
 * chunks of instances whose staging stays below the cap of lcqp_hip_sparse_set_adjoint_staging (the results do not depend on the chunking).
 * reduce = 1: [nnzQ], [nnzA]: the sums over the batch (one value array shared by the instances), formed on the device in the order of the
 * batch -- the same bits on every call; an instance with info & 1 contributes zeros, every other flagged instance what the kernels computed.
 * db, side, info, dQx, dAx may be NULL.
 * With vy == NULL and no matrix output the call is lcqp_hip_sparse_sensitivity with nrhs = 1, to the bit.  It reads the batch and changes none
 * of it.  lcqp_hip_sparse_sensitivity_timing then reports the sum of its kernels.
 * LCQP_INVALID_ARGUMENT: NULL handle, vx or dg, or reduce outside 0 / 1.  Then LCQP_LCQPOBJECT_NOT_SETUP as lcqp_hip_sparse_sensitivity.  Both
 * are decided before any device call. */
int  lcqp_hip_sparse_adjoint(lcqp_hip_sparse_t* s, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                             int reduce, double* dQx, double* dAx);
/* lcqp_hip_sparse_adjoint without matrices for many pairs per instance, and the dual rows of the solution Jacobian (DESIGN.md section 3a'''',
 * "The sparse arm: panels with gradients on y"; the twins of lcqp_hip_batch_adjoint_blocked / _jacobian_duals in this arm's conventions: no box
 * rows, m = nC + 2 nComp rows [A; L; R], y as lcqp_hip_sparse_get_solution returns it).
 * adjoint_blocked: vx [B][nrhs][nV] or NULL (zero), vy [B][nrhs][m] or NULL (zero), not both NULL; per pair
 *     Q d + E_W' mu = vx,  E_W d = -vy_W;     dg = -d [B][nrhs][nV],   db_W = mu [B][nrhs][m] (exactly 0.0 outside W);
 * side, info and the layouts are those of lcqp_hip_sparse_sensitivity_blocked.  Entries of vy outside W are dropped: whatever they hold (a NaN
 * included), the bits are the same.  The pairs go through k_sparse_sensitivity_blk_dual (the general LDL' with its panel form on:
 * k_sparse_sensitivity_blk_general_dual) in panels of lcqp_hip_sparse_sens_panel(s) columns, as work items in chunks under the staging cap; the
 * refinement carries the second block, residual [vx - Q d - E_W' mu; -vy_W - E_W d].  A pair's result depends on nothing but that pair -- not
 * on its place in the call, its neighbours or the chunking --, bit for bit, and equals lcqp_hip_sparse_adjoint's to rounding.  vy == NULL: the
 * call is lcqp_hip_sparse_sensitivity_blocked, to the bit; vx == NULL: the bits of an explicit zero vx.
 * jacobian_duals, for the instances [first, first + count):
 *   Jyg[i][r][j]  [count][m][nV]   d y*_r / d g_j of instance first + i
 *   Jyb[i][r][s]  [count][m][m]    d y*_r / d (the bound row s sits on); may be NULL
 *   side [count][m], info [count]  as lcqp_hip_sparse_sensitivity; may be NULL
 * Rows (and columns of Jyb) outside W are exactly 0.0.  Row r of W is what adjoint_blocked returns for vx = 0, vy = e_r (band engines: to the
 * bit).  The unit columns of W are written by the kernel, nothing is uploaded; the call is sized for m columns per instance, goes in chunks of
 * (instance, panel) work items under the cap of lcqp_hip_sparse_set_adjoint_staging, and an instance's rows do not depend on the chunking.
 * With lcqp_hip_sparse_jacobian the two give the whole map D(x*, y*) / D(g, b_W).
 * On a handle whose lcqp_hip_sparse_sens_panel is 0 (the general LDL' without lcqp_hip_sparse_set_general_panel) both run the vector kernel
 * k_sparse_sensitivity with vy and return its bits -- adjoint_blocked on the nrhs pairs, jacobian_duals on uploaded unit vy in chunks of
 * columns under the same cap (a sub-range then costs the launches of the whole batch).
 * Both are synchronous on return, change nothing a run / resolve reads and leave lcqp_hip_sparse_launch_counts alone;
 * lcqp_hip_sparse_sensitivity_timing reports the sum of their launches.
 * LCQP_INVALID_ARGUMENT: NULL handle; adjoint_blocked: nrhs < 1, vx and vy both NULL, NULL dg; jacobian_duals: NULL Jyg, first < 0, count < 1,
 * first + count > B.  Then LCQP_LCQPOBJECT_NOT_SETUP as lcqp_hip_sparse_sensitivity.  Both are decided before any device call. */
int  lcqp_hip_sparse_adjoint_blocked(lcqp_hip_sparse_t* s, int nrhs, const double* vx, const double* vy,
                                     double* dg, double* db, int* side, int* info);
int  lcqp_hip_sparse_jacobian_duals(lcqp_hip_sparse_t* s, int first, int count,
                                    double* Jyg, double* Jyb, int* side, int* info);
/* another staging cap for this handle's adjoint, blocked-sensitivity and Jacobian calls and for the two chunks of staging of a host load /
 * update (0: the default, LCQP_JACOBIAN_STAGING_BYTES); for tests of the chunking and for small devices */
int  lcqp_hip_sparse_set_adjoint_staging(lcqp_hip_sparse_t* s, size_t bytes);
/* ---- Device-pointer entry points of the sparse batch (DESIGN.md section 3a''''', "The sparse arm"): the twins of lcqp_hip_sparse_load / _update /
 * _get_solution / _sensitivity / _adjoint whose data pointers are DEVICE pointers, under the rules of the dense device calls above.  Layouts,
 * defaults for absent vectors and return codes are the host twins'; the pools, the solution and every gradient hold the bits the host twins
 * leave, and the handle chooses the ordering and the light regularisation a host load of the same data chooses.  The differences:
 *   pointers  every non-NULL data pointer is plain device memory (hipMalloc) of the handle's device that holds the bytes the call moves; host,
 *             pinned and managed memory and another device's memory are refused with LCQP_INVALID_ARGUMENT and a message, on the host, before
 *             anything is enqueued.  dQx must be 16-byte aligned (the Q segment of the gradient kernels stores pairs of doubles), dAx 8-byte.
 *   stream    the caller's hipStream_t (NULL: the legacy default stream).  The handle's stream waits for an event recorded on it, the work is
 *             enqueued on the handle's stream, and the caller's stream waits for an event recorded behind it.  run and resolve stay on the
 *             handle's stream: update_device -> resolve -> get_solution_device needs no host wait, and update_device does not drain the
 *             stream first -- stream order replaces that.  load_device and update_device wait for ONE status
 *             read each (the check below; for a load with Qx also two numbers per instance from the diagonal of its Hessian, from which the
 *             host forms the ratio that selects the ordering); a call also waits when a buffer of the handle grows.  Nothing else waits.
 *   shared    (load) bit 1: Qx is ONE [nnzQ] array for all `count` instances, bit 2: the same for Ax (broadcast by the pack kernel; the
 *             setting reduce = 1 of the adjoint is meant for).  Other bits: LCQP_INVALID_ARGUMENT.
 *   NULL Qx / Ax (load) leaves those values as the batch holds them; every instance of the range must then already hold a problem, else
 *             LCQP_INVALID_ARGUMENT (the host twin's code for a missing matrix).  g stays mandatory: LCQP_INVALID_OBJECTIVE_LINEAR_TERM.
 *   validation -inf in lbL / lbR is looked for by one kernel over the whole range before anything is written; on a failure nothing is
 *             written, NO host state changes, and the code is LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND, as with lcqp_hip_sparse_load.
 *   NULL handle: LCQP_LCQPOBJECT_NOT_SETUP from all five.
 * The two paths mix on one handle: the host state (which instances hold problems, the lbL / lbR flags, the diagonal ratios, the setup mark)
 * is kept in step.  sensitivity_device / adjoint_device make the state checks of their host twins (LCQP_INVALID_ARGUMENT for NULL v / vx / dg,
 * nrhs < 1, reduce outside 0 / 1; then LCQP_LCQPOBJECT_NOT_SETUP without a finished solve); v [B][nrhs][nV], vx [B][nV], vy [B][m] are read
 * where they lie; dQx / dAx ([B][nnz], or [nnz] with reduce = 1) are written by ONE launch, without staging or chunks, with the terms -- hence
 * the bits -- of the host call.  stats of get_solution_device is a device array of B lcqp_stats_t.  The kernel time of the two is formed when
 * lcqp_hip_sparse_sensitivity_timing asks for it (that call then waits for the kernels). */
int  lcqp_hip_sparse_load_device(lcqp_hip_sparse_t* s, int first, int count, int shared,
                                 const double* Qx, const double* g, const double* Ax,
                                 const double* lbA, const double* ubA, const double* lbL, const double* ubL,
                                 const double* lbR, const double* ubR, const double* x0, const double* y0, void* stream);
int  lcqp_hip_sparse_update_device(lcqp_hip_sparse_t* s, int first, int count, const double* g,
                                   const double* lbA, const double* ubA, const double* lbL, const double* ubL,
                                   const double* lbR, const double* ubR, const double* x0, const double* y0, void* stream);
/* lcqp_hip_sparse_update_values on device arrays, under the rules above: shared as in load_device, a NULL array stays; the checks of the
 * host twin in its order, then shared & ~3 (LCQP_INVALID_ARGUMENT), then the pointers.  With Qx one small kernel forms the diagonal pairs
 * of the new Hessians and the call waits for them (the one host synchronisation, as in load_device). */
int  lcqp_hip_sparse_update_values_device(lcqp_hip_sparse_t* s, int first, int count, int shared,
                                          const double* Qx, const double* Ax, void* stream);
int  lcqp_hip_sparse_get_solution_device(lcqp_hip_sparse_t* s, double* x, double* y, lcqp_stats_t* stats, void* stream);
int  lcqp_hip_sparse_sensitivity_device(lcqp_hip_sparse_t* s, int nrhs, const double* v,
                                        double* dg, double* db, int* side, int* info, void* stream);
int  lcqp_hip_sparse_adjoint_device(lcqp_hip_sparse_t* s, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                                    int reduce, double* dQx, double* dAx, void* stream);
/* The device-pointer twins of the four panel calls -- lcqp_hip_sparse_sensitivity_blocked, _adjoint_blocked, _jacobian and _jacobian_duals --
 * under the rules above (DESIGN.md section 3a''''', "The sparse arm: panels and Jacobians into device arrays"): layouts, results and codes are
 * the host twins', every array is a device array, and the results hold the host twins' bits, whatever the chunking.
 *   checks    NULL handle: LCQP_LCQPOBJECT_NOT_SETUP.  Then the host twin's argument checks in its order (LCQP_INVALID_ARGUMENT), then
 *             LCQP_LCQPOBJECT_NOT_SETUP without a finished solve, then the pointers: every non-NULL data pointer plain device memory of the
 *             handle's device, 8-byte aligned (side, info: 4), with the bytes the call moves behind it -- else LCQP_INVALID_ARGUMENT and a
 *             message that names the argument.  All of it on the host, before anything is enqueued.
 *   inputs    v, vx [B][nrhs][nV] and vy [B][nrhs][m] are read where they lie.
 *   work      on the handle's stream between the two events of the hand-over: the host twin's chunks of (instance, panel) work items under
 *             the cap of lcqp_hip_sparse_set_adjoint_staging, each chunk's panel launch followed by ONE launch of k_sparse_scatter_panels,
 *             which takes the staged columns to the rows of the caller's arrays the host twin's copies take them to (the padding columns of
 *             a ragged last panel nowhere; jacobian_duals: column k to the row the panel kernel recorded for it, and Jyg / Jyb are
 *             zero-filled on the stream first: rows outside W are exact zeros); side and info go device to device.
 *   waits     none on the host, but for a buffer of the handle that grows, and for a call of more than one chunk: it waits for the kernel
 *             of every chunk but the last, whose events it is about to reuse.  lcqp_hip_sparse_sensitivity_timing reports the sum over the
 *             chunks' panel kernels, as after the host twins (and waits for the last one).
 *   no panel form (lcqp_hip_sparse_sens_panel(s) == 0): the two blocked calls run the vector kernel on the caller's arrays, as
 *             lcqp_hip_sparse_sensitivity_device does (an absent vx: a zero array on the device) -- the host twins' bits.  The two Jacobian
 *             calls form their result through the host twins and copy it to the device: THOSE TWO THEN WAIT ON THE HOST.
 * The calls change nothing a run / resolve reads, leave lcqp_hip_sparse_launch_counts alone and share the handle's staging with the host
 * twins: host and device calls may alternate on one handle. */
int  lcqp_hip_sparse_sensitivity_blocked_device(lcqp_hip_sparse_t* s, int nrhs, const double* v,
                                                double* dg, double* db, int* side, int* info, void* stream);
int  lcqp_hip_sparse_adjoint_blocked_device(lcqp_hip_sparse_t* s, int nrhs, const double* vx, const double* vy,
                                            double* dg, double* db, int* side, int* info, void* stream);
int  lcqp_hip_sparse_jacobian_device(lcqp_hip_sparse_t* s, int first, int count,
                                     double* Jg, double* Jb, int* side, int* info, void* stream);
int  lcqp_hip_sparse_jacobian_duals_device(lcqp_hip_sparse_t* s, int first, int count,
                                           double* Jyg, double* Jyb, int* side, int* info, void* stream);
/* Test and diagnostic entry point: the problem of one instance as the pools hold it, so that a load or an update can be held bit for bit and
 * not only through solutions.  Host buffers, synchronous, launches nothing; any output may be NULL.  Qx [nnzQ]; Ax [nnzA] in the caller's CSC
 * order (through the inverse of the value map); g, x0 [nV]; lE, uE [m]: the stacked row bounds as stored, m = nC + 2 nComp; lbL, lbR [nComp];
 * y0 [m]; hasY0 [1].  LCQP_INVALID_ARGUMENT: NULL handle, or an instance outside the batch. */
int  lcqp_hip_sparse_read_problem(lcqp_hip_sparse_t* s, int instance, double* Qx, double* Ax, double* g,
                                  double* lE, double* uE, double* lbL, double* lbR, double* x0, double* y0, int* hasY0);
/* Test and diagnostic entry point (as lcqp_hip_batch_read_admm on the dense arm): the state of the ADMM rounds of one instance as it lies on
 * the device, so that tests/test_gpu_sparse_admm.py can hold the weights and the iterates to a plain reference.  Host buffers, synchronous,
 * launches nothing and changes nothing; any output may be NULL.  dims [2]: nV, m = nC + 2 nComp; scal [3]: sigma = admmSigma scale, rho =
 * admmRho scale, scale = max |Q_ii|; rhov, l, u, ya, za [m] in the row order of [A; L; R]; xa [nV].  The polish writes none of xa, ya, za:
 * they are those of the last QP that ran ADMM iterations (ya = -y0 at the start of a solve that is given y0).
 * LCQP_INVALID_ARGUMENT: NULL handle, or an instance outside the batch.  LCQP_LCQPOBJECT_NOT_SETUP: no run / resolve on this handle yet, or a
 * load / set_options since. */
int  lcqp_hip_sparse_read_admm(lcqp_hip_sparse_t* s, int instance, int dims[2], double scal[3], double* rhov, double* l, double* u,
                               double* xa, double* ya, double* za);
/* Test and diagnostic entry point (as lcqp_hip_batch_read_polish on the dense arm): the state of the active-set polish of one instance as
 * the last run / resolve left it on the device, so that tests/test_gpu_sparse_polish_audit.py can hold every trial to a plain reference.  Host
 * buffers, synchronous, launches nothing and changes nothing; any of dims, scal, V, M, I may be NULL.
 *   dims [15]  0 nV, 1 m = nC + 2 nComp | the polish record: 2 trial, 3 reuse, 4 fact_valid, 5 nrefine, 6 round, 7 rc | the instance:
 *              8 stfValid, 9 bigReg, 10 haveSolution | the handle: 11 lightOK, 12 border nodes, 13 general LDL', 14 lanes per instance
 *   scal [11]  0 gs = 1 + |g|_inf, 1 ytol, 2 dpUsed, 3 d2Used (the regularisation pair of the factor in memory), 4 xinf = |x|_inf behind the
 *              last correction | 5 delta, 6 deltaS, 7 delta2, 8 delta2S (the safe pair delta / delta2, the light pair deltaS / delta2S),
 *              9 e1max = the largest row 1-norm of E, 10 scale = max |Q_ii|
 *   V [5][nV]  the trial point xt, the right-hand side / residual r1, Q x of the last sweep, the linear term gk of the QP, the stored xq
 *   M [5][m]   the trial multipliers yt, E x of the last trial, the stacked bounds l, u, the stored yq     (row order of [A; L; R])
 *   I [4][m]   row states (0 inactive, 1 lower, 2 upper, 3 equality): the stored set st, the trial's set stt, the set of the factor in memory
 *              stf, the set the last status test proposed
 * LCQP_INVALID_ARGUMENT: NULL handle, or an instance outside the batch.  LCQP_LCQPOBJECT_NOT_SETUP: no run / resolve on this handle yet, or a
 * load / set_options since. */
int  lcqp_hip_sparse_read_polish(lcqp_hip_sparse_t* s, int instance, int dims[15], double scal[11], double* V, double* M, int* I);
/* Test and diagnostic entry point: the sparse products of the solver (sp_Ex, sp_Qx2, sp_ETy, sp_residual, sp_Cx2, sp_C_from_Ex in
 * lcqp_sparse_solver.hpp) themselves, applied for every instance of a loaded batch to vectors the caller supplies, so that
 * tests/test_gpu_sparse_products.py can hold every branch of the ELL-slab gather to a plain reference.  One launch of k_sparse_product_probe
 * on the handle's stream; the handle is synchronised first, the call is synchronous.  Writes only scratch a run rewrites before it reads it.
 *   wide  0: the lane group of the handle per instance (lcqp_hip_sparse_lanes); 1: a wavefront per instance, as the streaming phases of a run
 *   vn    [B][8][nV]  inputs: x of E x | x0, x1 of Q x0, Q x1 | base of base - E'y | g, x of the residual | v0, v1 of C v0, C v1
 *   vm    [B][4][m]   inputs: y of base - E'y | y of the residual | lx0, lx1 of the two C-from-E-x forms (entries of E v; rows of A unused)
 *   on    [B][11][nV] outputs: Q x0, Q x1 | base - E'y | r1 = -g - Q x - E'y, Q x | C v0, C v1 | L'R + R'L gathers of (lx0, lx1) |
 *                     the one-vector form of lx0 and its second sum (zeros)
 *   om    [B][m]      E x
 *   os    [B][3]      max |base - E'y|, max |r1|, max_i (|g_i| + |Q x|_i + |E'y|_i) as the routines return them
 *   ell   [6] or NULL slab width (4 / 8) and tail flag of the row slab of Q, the row slab of E and the column slab of E
 * LCQP_INVALID_ARGUMENT: NULL handle or buffer, wide outside 0 / 1.  LCQP_LCQPOBJECT_NOT_SETUP: nothing loaded yet. */
int  lcqp_hip_sparse_product_probe(lcqp_hip_sparse_t* s, int wide, const double* vn, const double* vm, double* on, double* om, double* os, int ell[6]);
/* Test and diagnostic entry point (as lcqp_hip_batch_read_setup / _read_working_set on the dense arm): the KKT factorisations and solves
 * of the sparse arm -- the register band, the LDS-window band, the bordered band, the general LDL' -- run for every instance of the batch
 * on matrices the caller names, one solve per right-hand side and NO refinement, so that tests/test_gpu_sparse_factor.py can hold each engine
 * to a plain reference.  One launch of k_sparse_kkt_probe on the handle's stream; the handle is synchronised first, the call is synchronous.
 *   rhs, sol   [B][nrhs][nV + nC + 2 nComp] (host) in NODE order: the variables, then the rows of E = [A; L; R]
 * mode LCQP_KKT_PROBE_FACTOR: dprim [B], ddual [B][m], use [B][m] (0 / 1), m = nC + 2 nComp.  [Q + dprim I, E_use'; E_use, -diag(ddual)] is
 *   factorised into the polish slot -- a row outside `use` gets the diagonal -1 and no entries -- by exactly the pieces a run composes, then
 *   solved with.  `which` and the record buffers are ignored.  THE STORED POLISH FACTOR IS OVERWRITTEN: afterwards
 *   lcqp_hip_sparse_sensitivity answers LCQP_LCQPOBJECT_NOT_SETUP and a warm lcqp_hip_sparse_resolve starts every instance cold, until the next
 *   run / resolve.
 * mode LCQP_KKT_PROBE_STORED: no factorisation; the solves run with the factor of slot `which` (0: the polish slot, 1: the ADMM slot) as the
 *   last run / resolve left it, and the record of the matrix that factor is the factor of comes back in the layout of the FACTOR inputs:
 *   rec_dprim [B], rec_ddual [B][m], rec_use [B][m] -- polish: the regularisation pair of the last factorisation and its working set; ADMM:
 *   sigma, 1 / rho_r, all ones.  dprim, ddual, use are ignored.  Changes nothing a run reads.
 * LCQP_INVALID_ARGUMENT: nrhs < 1, NULL rhs or sol, a mode other than the two, FACTOR with a NULL input, STORED with `which` outside 0 / 1 or a
 * NULL record buffer.  Then LCQP_LCQPOBJECT_NOT_SETUP: NULL handle, no run / resolve on this handle yet or a load / set_options since (the band
 * rows the register engine streams exist only behind one), STORED on the polish slot behind a FACTOR call.  LCQP_HIP_ERROR: a HIP call failed. */
#define LCQP_KKT_PROBE_FACTOR 0
#define LCQP_KKT_PROBE_STORED 1
int  lcqp_hip_sparse_kkt_probe(lcqp_hip_sparse_t* s, int mode, int which, int nrhs, const double* dprim, const double* ddual, const int* use,
                               const double* rhs, double* sol, double* rec_dprim, double* rec_ddual, int* rec_use);
int  lcqp_hip_sparse_synchronize(lcqp_hip_sparse_t* s);
int  lcqp_hip_sparse_last_timing(lcqp_hip_sparse_t* s, float* setup_ms, float* solve_ms);
int  lcqp_hip_sparse_get_solution(lcqp_hip_sparse_t* s, double* x, double* y, lcqp_stats_t* stats);   /* y: [B][nC + 2 nComp] */
double lcqp_hip_sparse_algorithmic_bytes(lcqp_hip_sparse_t* s);
/* per-iterate trace of one instance of the last run (options.storeSteps), same layout as lcqp_hip_batch_get_trace
 * (src/LCQProblem.cpp:1365-1378, 1528-1576: the host LCQProblem rebuilds the tracking vectors and the iteration table from it) */
int  lcqp_hip_sparse_get_trace(lcqp_hip_sparse_t* s, int instance, int cap, double* scalars, double* x, int* len);
/* mean clock ticks per instance in 8 phases of the last run; LCQP_HIP_UNSUPPORTED unless the library was built with -DLCQP_PROFILE */
int  lcqp_hip_sparse_read_profile(lcqp_hip_sparse_t* s, double* out);

#ifdef __cplusplus
}
#endif
#endif /* LCQP_HIP_H */
