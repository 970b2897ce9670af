// A stand-in for liblcqpow_hip.so in host_owner_test: exactly the lcqp_hip_* functions the host layer (lcqpow_amd/csrc/host) and the inline
// members of BatchLCQProblem.hpp that the test uses refer to.  It hands out dummy handles, counts what is created, cloned and destroyed per
// handle kind, lets a scenario make a named call fail, and computes nothing: every solution is zero.  No GPU, no HIP.
#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "lcqp_hip.h"

struct lcqp_hip_batch { int B, nV, nd; };
struct lcqp_hip_sparse { int B, nV, nd; };
struct lcqp_hip_qp { int nV, nd; };

namespace fake {

struct Counts { int created, cloned, destroyed; };
Counts batch, sparse, qp;
int strayDestroys = 0;                                  // a destroy of something that is not a live handle (a second destroy, a wild pointer)
static std::set<const void*> liveSet;
static std::map<std::string, std::pair<int, int> > failures;      // name -> (calls left until the failing one, code it returns)

int live() { return (int)liveSet.size(); }
void reset() { batch = sparse = qp = Counts(); strayDestroys = 0; failures.clear(); }      // (live handles stay counted: a leak of one scenario shows in the next)
// the nth call of `name` from now fails, once: a create or clone returns NULL, every other call returns `code`
void fail(const char* name, int nth = 1, int code = LCQP_HIP_ERROR) { failures[name] = std::make_pair(nth, code); }

static int failing(const char* name)
{
    std::map<std::string, std::pair<int, int> >::iterator f = failures.find(name);
    if (f == failures.end() || --f->second.first > 0) return 0;
    const int code = f->second.second;
    failures.erase(f);
    return code;
}

template <typename H> static H* made(H* h, int& counter) { liveSet.insert(h); counter++; return h; }
template <typename H> static void gone(H* h, Counts& c)
{
    if (!liveSet.erase(h)) { strayDestroys++; return; }
    c.destroyed++;
    delete h;
}

static void solved(int B, lcqp_stats_t* st)
{
    for (int i = 0; st && i < B; i++) { std::memset(&st[i], 0, sizeof(st[i])); st[i].iterTotal = 1; st[i].status = 4; st[i].rhoOpt = 1.0; }
}
static int trace(int nV, int cap, double* scalars, double* x, int* len)
{
    *len = std::min(cap, 1);
    if (*len) { std::fill(scalars, scalars + 8, 0.0); std::fill(x, x + nV, 0.0); }
    return 0;
}

}  // namespace fake

using namespace fake;
#define FAILS(name) if (const int code_ = failing(#name)) return code_
#define FAILS_NULL(name) if (failing(#name)) return nullptr

extern "C" {

void lcqp_hip_options_default(lcqp_options_t* o)
{
    std::memset(o, 0, sizeof(*o));
    o->complementarityTolerance = 1e3 * 2.221e-16; o->stationarityTolerance = 1e6 * 2.221e-16; o->initialPenaltyParameter = 0.01;
    o->penaltyUpdateFactor = 2; o->maxPenaltyParameter = 1e8; o->etaDynamicPenalty = 0.9; o->solveZeroPenaltyFirst = 1; o->perturbStep = 1;
    o->maxIterations = 1000; o->nDynamicPenalty = 3; o->printLevel = 2;
}

lcqp_hip_qp_t* lcqp_hip_qp_create(int nV, int nC, const double*, const double*, const lcqp_options_t*, int)
{
    FAILS_NULL(lcqp_hip_qp_create);
    return made(new lcqp_hip_qp{nV, nV + nC}, qp.created);
}
lcqp_hip_qp_t* lcqp_hip_qp_clone(const lcqp_hip_qp_t* src)
{
    FAILS_NULL(lcqp_hip_qp_clone);
    return made(new lcqp_hip_qp(*src), qp.cloned);
}
void lcqp_hip_qp_destroy(lcqp_hip_qp_t* h) { gone(h, qp); }
int lcqp_hip_qp_set_options(lcqp_hip_qp_t*, const lcqp_options_t*) { FAILS(lcqp_hip_qp_set_options); return 0; }
int lcqp_hip_qp_solve(lcqp_hip_qp_t*, int, int* iterations, int* exit_flag, const double*, const double*, const double*, const double*, const double*,
                      const double*, const double*)
{
    FAILS(lcqp_hip_qp_solve);
    *iterations = 1; *exit_flag = 0;
    return 0;
}
void lcqp_hip_qp_get_solution(lcqp_hip_qp_t* h, double* x, double* y) { std::fill(x, x + h->nV, 0.0); std::fill(y, y + h->nd, 0.0); }
int lcqp_hip_qp_sensitivity(lcqp_hip_qp_t*, int, const double*, double*, double*, int*, int*) { return LCQP_HIP_UNSUPPORTED; }
int lcqp_hip_qp_sensitivity_blocked(lcqp_hip_qp_t*, int, const double*, double*, double*, int*, int*) { return LCQP_HIP_UNSUPPORTED; }
int lcqp_hip_qp_jacobian(lcqp_hip_qp_t*, double*, double*, int*, int*) { return LCQP_HIP_UNSUPPORTED; }
int lcqp_hip_qp_adjoint(lcqp_hip_qp_t*, const double*, const double*, double*, double*, int*, int*, double*, double*) { return LCQP_HIP_UNSUPPORTED; }

lcqp_hip_batch_t* lcqp_hip_batch_create(int B, int nV, int nC, int nComp, int, int)
{
    FAILS_NULL(lcqp_hip_batch_create);
    return made(new lcqp_hip_batch{B, nV, nV + nC + 2 * nComp}, batch.created);
}
void lcqp_hip_batch_destroy(lcqp_hip_batch_t* h) { gone(h, batch); }
int lcqp_hip_batch_set_options(lcqp_hip_batch_t*, const lcqp_options_t*) { FAILS(lcqp_hip_batch_set_options); return 0; }
int lcqp_hip_batch_set_overlapped(lcqp_hip_batch_t*, int) { FAILS(lcqp_hip_batch_set_overlapped); return 0; }
int lcqp_hip_batch_load(lcqp_hip_batch_t*, int, int, const double*, const double*, const double*, const double*, const double*, const double*,
                        const double*, const double*, const double*, const double*, const double*, const double*, const double*, const double*,
                        const double*)
{
    FAILS(lcqp_hip_batch_load);
    return 0;
}
int lcqp_hip_batch_run(lcqp_hip_batch_t*) { FAILS(lcqp_hip_batch_run); return 0; }
int lcqp_hip_batch_get_solution(lcqp_hip_batch_t* h, double* x, double* y, lcqp_stats_t* st)
{
    FAILS(lcqp_hip_batch_get_solution);
    std::fill(x, x + (size_t)h->B * h->nV, 0.0); std::fill(y, y + (size_t)h->B * h->nd, 0.0);
    solved(h->B, st);
    return 0;
}
int lcqp_hip_batch_get_trace(lcqp_hip_batch_t* h, int, int cap, double* scalars, double* x, int* len)
{
    FAILS(lcqp_hip_batch_get_trace);
    return trace(h->nV, cap, scalars, x, len);
}

lcqp_hip_sparse_t* lcqp_hip_sparse_create(int B, int nV, int nC, int nComp, const int*, const int*, const int*, const int*, int)
{
    FAILS_NULL(lcqp_hip_sparse_create);
    return made(new lcqp_hip_sparse{B, nV, nC + 2 * nComp}, sparse.created);
}
void lcqp_hip_sparse_destroy(lcqp_hip_sparse_t* h) { gone(h, sparse); }
int lcqp_hip_sparse_set_options(lcqp_hip_sparse_t*, const lcqp_options_t*) { FAILS(lcqp_hip_sparse_set_options); return 0; }
int lcqp_hip_sparse_load(lcqp_hip_sparse_t*, int, int, const double*, const double*, const double*, const double*, const double*, const double*,
                         const double*, const double*, const double*, const double*, const double*)
{
    FAILS(lcqp_hip_sparse_load);
    return 0;
}
int lcqp_hip_sparse_run(lcqp_hip_sparse_t*) { FAILS(lcqp_hip_sparse_run); return 0; }
int lcqp_hip_sparse_get_solution(lcqp_hip_sparse_t* h, double* x, double* y, lcqp_stats_t* st)
{
    FAILS(lcqp_hip_sparse_get_solution);
    std::fill(x, x + (size_t)h->B * h->nV, 0.0); std::fill(y, y + (size_t)h->B * h->nd, 0.0);
    solved(h->B, st);
    return 0;
}
int lcqp_hip_sparse_get_trace(lcqp_hip_sparse_t* h, int, int cap, double* scalars, double* x, int* len)
{
    FAILS(lcqp_hip_sparse_get_trace);
    return trace(h->nV, cap, scalars, x, len);
}

}  // extern "C"
