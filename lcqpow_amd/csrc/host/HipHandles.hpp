// Owners of the C ABI's handles (include/lcqp_hip.h): a handle a host class or function creates is held in one of these from the line
// it is created on and released by the owner alone, on whichever path the scope is left.
#ifndef LCQPOW_AMD_HIPHANDLES_HPP
#define LCQPOW_AMD_HIPHANDLES_HPP

#include <memory>

#include "lcqp_hip.h"

namespace LCQPow {

struct HipHandleDeleter {
    void operator()(lcqp_hip_batch_t* h) const { lcqp_hip_batch_destroy(h); }
    void operator()(lcqp_hip_sparse_t* h) const { lcqp_hip_sparse_destroy(h); }
    void operator()(lcqp_hip_qp_t* h) const { lcqp_hip_qp_destroy(h); }
};
using BatchHandle = std::unique_ptr<lcqp_hip_batch_t, HipHandleDeleter>;
using SparseHandle = std::unique_ptr<lcqp_hip_sparse_t, HipHandleDeleter>;
using QpHandle = std::unique_ptr<lcqp_hip_qp_t, HipHandleDeleter>;

}  // namespace LCQPow
#endif
