// lcqp_nch.hip -- one instantiation of the per-size kernels and of their launch table: compile with -DLCQP_TU_NCH=k, k in {1,2,3,4,8,16,32}.
#include "lcqp_kernels.hpp"

#ifndef LCQP_TU_NCH
#error "compile lcqp_nch.hip with -DLCQP_TU_NCH=1|2|3|4|8|16|32"
#endif

#ifdef LCQP_TU_SHARED   // k_lcqp_run for a batch that holds one set of matrices: -DLCQP_VARIANT=2, or the second build with -DLCQP_VARIANT=3 -DLCQP_MINWAVES=2
template lcqp::BatchKernel lcqp::shared_run_kernel<LCQP_TU_NCH, LCQP_VARIANT>();
#elif defined(LCQP_TU_FEW)      // the second build of the persistent kernels (batches of at most three workgroups per CU; lcqp_kernels.hpp): with
                        // -DLCQP_VARIANT=1 -DLCQP_MINWAVES=2
template const lcqp::RunKernels& lcqp::few_kernels<LCQP_TU_NCH>();
#else
template const lcqp::SizeKernels& lcqp::size_kernels<LCQP_TU_NCH>();
#endif
