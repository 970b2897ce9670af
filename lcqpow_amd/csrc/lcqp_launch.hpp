// lcqp_launch.hpp -- the seam between the host translation units (lcqp_hip.hip, lcqp_hip_qp.hip, lcqp_hip_util.hip) and the per-size kernel translation units
// (lcqp_nch.hip, one per NCH in {1,2,3,4,8,16,32} and a second one of the two persistent kernels for NCH <= 4): per padded size one table
// of launch functions, each with the arguments its kernel takes.  `grid` is the number of workgroups; every launch is asynchronous on
// `s`.  Declarations only: no device code lives here.
#pragma once
#include "lcqp_dev.hpp"

namespace lcqp {
// nothing of the seam enters the dynamic symbol table of the library
#pragma GCC visibility push(hidden)

using BatchKernel = void (*)(const DevBatch& db, int grid, hipStream_t s);

// the two persistent kernels: the standard unit and the second (256-register) build each define a pair
struct RunKernels {
    void (*lcqp_run)(const DevBatch& db, int grid, hipStream_t s);
    void (*qp_solve)(const DevBatch& db, int grid, hipStream_t s, int initial);
};


struct SizeKernels {
    int nch;                    // np = 128 * nch
    RunKernels run;
    const RunKernels* few;      // the second build of the persistent kernels (np <= 512, at most three workgroups per CU), null for NCH > 4
    BatchKernel shared_run, shared_run_few;      // k_lcqp_run of a batch that holds one set of matrices: the standard and the second build (null for NCH > 4)
    BatchKernel prepare;
    // mode 0: every instance cold, 1: warm where the last run succeeded; rho0 [B]: starting penalties of the warm instances (device), or null
    void (*refresh)(const DevBatch& db, int grid, hipStream_t s, int mode, const double* rho0);
    // k_prepare where the matrices changed under a stored point: warm where the last run succeeded, with an empty inverse factor; rho0 as above
    void (*prepare_warm)(const DevBatch& db, int grid, hipStream_t s, const double* rho0);
    // a batch that holds one set of matrices: k_prepare_shared on a grid of one (src: the instance whose box list is the batch's), and
    // k_share_setup over the batch behind the setup chain (mode 0: cold, 1: warm with an emptied factor; rho0 as above)
    void (*prepare_shared)(const DevBatch& db, hipStream_t s, int src);
    void (*share_setup)(const DevBatch& db, int grid, hipStream_t s, int mode, const double* rho0);
    BatchKernel build_C, compress_C;
    BatchKernel factor, factor_full;      // factor_full: held to 128 registers for np <= 256, so that four workgroups per CU are resident
    BatchKernel trsm, trsm_streamed, build_M;
    void (*synth_fill)(const DevBatch& db, int grid, hipStream_t s, uint64_t seed0, uint64_t first);
    BatchKernel synth_Q;
    // device buffers, layouts at the kernels.  sensitivity: the whole batch.  sensitivity_blk: workgroup o works on instance first + o,
    // v null: unit vectors; null for NCH > 4 (a panel of np >= 1024 does not fit LDS).  sensitivity_dual: k_sensitivity<NCH, true>, which adds
    // the upstream gradients vy [B][nrhs][nd] on the duals to the right-hand side
    void (*sensitivity)(const DevBatch& db, int grid, hipStream_t s, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo);
    void (*sensitivity_dual)(const DevBatch& db, int grid, hipStream_t s, int nrhs, const double* v, const double* vy, double* dg, double* dbo, int* side, int* sinfo);
    void (*sensitivity_blk)(const DevBatch& db, int grid, hipStream_t s, int first, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo);
    // k_sensitivity_blk_dual<NCH> (null for NCH > 4).  unit 0: panels of pairs, v [count][nrhs][n] or null (a zero panel: no forward
    // substitution), vy [count][nrhs][nd] or null.  unit 1: the unit vectors of the slot space, nrhs <= capS staged rows per instance, and
    // rowpos [count][capS]: the dual position of every staged row, -1 behind the last occupied slot
    void (*sensitivity_blk_dual)(const DevBatch& db, int grid, hipStream_t s, int first, int nrhs, const double* v, const double* vy, int unit,
                                 double* dg, double* dbo, int* side, int* sinfo, int* rowpos);
    // building-block kernels
    void (*util_symv)(int grid, hipStream_t s, int n, double alpha, const double* A, const double* b, const double* c, double* d);
    void (*util_rows)(int grid, hipStream_t s, int m, const double* A, const double* x, double* dots, const double* coef, double* outT);
    void (*util_rows_list)(int grid, hipStream_t s, int m, int nlist, const double* A, const int* list, const double* x, double* dots, const double* coef, double* outT);
};

// defined in lcqp_kernels.hpp and instantiated by lcqp_nch.hip for NCH = LCQP_TU_NCH: size_kernels by the standard unit, few_kernels by
// the unit compiled with -DLCQP_TU_FEW
template <int NCH> const SizeKernels& size_kernels();
template <int NCH> const RunKernels& few_kernels();
// the units compiled with -DLCQP_TU_SHARED -DLCQP_VARIANT=V: V = 2 the standard build, 3 the second one (with -DLCQP_MINWAVES=2)
template <int NCH, int V> BatchKernel shared_run_kernel();

#pragma GCC visibility pop
}  // namespace lcqp
