// lcqp_hip_qp.hip -- the QP object of the dense arm, lcqp_hip_qp_* (include/lcqp_hip.h; the subsolver of the host loop, SubsolverHIP).  It
// reaches its batch through lcqp_hip_batch.hpp and the public entry points lcqp_hip_batch_create / load / set_options / destroy.
#include "lcqp_hip_batch.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

using namespace lcqp;
using namespace lcqp_rt;

// =================================================================================================
// QP object (SubsolverBase semantics): a batch of one with nComp = 0 whose rows are the nC stacked rows
// =================================================================================================
struct BatchDeleter { void operator()(lcqp_hip_batch* h) const { lcqp_hip_batch_destroy(h); } };

struct lcqp_hip_qp {
    std::unique_ptr<lcqp_hip_batch, BatchDeleter> hb;      // built by the first solve
    int nV = 0, nC = 0;
    std::vector<double> Q, A;          // host copies (deep copy, src/SubsolverQPOASES.cpp:41-45)
    std::vector<double> lbA, ubA, lb, ub;
    bool haveBounds = false, withBox = false;
    lcqp_options_t opt{};
    int device = 0;
    std::vector<double> xsol, ysol;
    int cAdmm = 0, cTrials = 0, cFact = 0, cCorr = 0;
    bool solved = false;               // the last solve returned a solution on the options in place (lcqp_hip_qp_sensitivity)
    lcqp_hip_qp() = default;
    lcqp_hip_qp(const lcqp_hip_qp&) = delete;      // a copy would alias the batch: lcqp_hip_qp_clone copies the data fields
    lcqp_hip_qp& operator=(const lcqp_hip_qp&) = delete;
};

extern "C" lcqp_hip_qp_t* lcqp_hip_qp_create(int nV, int nC, const double* Q, const double* A, const lcqp_options_t* opt, int device)
{ return guarded(dense_err(), [&]() -> lcqp_hip_qp_t* {
    if (nV <= 0 || nC < 0 || !Q || (nC > 0 && !A)) { dense_err() = "invalid arguments"; return nullptr; }
    std::unique_ptr<lcqp_hip_qp> q(new lcqp_hip_qp());
    q->nV = nV; q->nC = nC; q->device = device;
    q->Q.assign(Q, Q + (size_t)nV * nV);
    if (nC) q->A.assign(A, A + (size_t)nC * nV);
    if (opt) q->opt = *opt; else lcqp_hip_options_default(&q->opt);
    q->xsol.assign(nV, 0.0); q->ysol.assign((size_t)nV + nC, 0.0);
    return q.release();
}, nullptr); }

extern "C" lcqp_hip_qp_t* lcqp_hip_qp_clone(const lcqp_hip_qp_t* s)
{ return guarded(dense_err(), [&]() -> lcqp_hip_qp_t* {
    if (!s) return nullptr;
    // The reference copies subsolvers only before their first use (src/Subsolver.cpp:125-136,
    // src/LCQProblem.cpp:906-907): the clone carries the problem data and options; device state is
    // rebuilt by its own first solve.  The bounds of the last solve and withBox are not carried: with no batch and haveBounds false
    // that first solve is a fresh one, which assigns all of them before it reads any.
    std::unique_ptr<lcqp_hip_qp> q(new lcqp_hip_qp());
    q->nV = s->nV; q->nC = s->nC; q->device = s->device;
    q->Q = s->Q; q->A = s->A; q->opt = s->opt;
    q->xsol = s->xsol; q->ysol = s->ysol;
    q->cAdmm = s->cAdmm; q->cTrials = s->cTrials; q->cFact = s->cFact; q->cCorr = s->cCorr;
    return q.release();
}, nullptr); }

extern "C" void lcqp_hip_qp_destroy(lcqp_hip_qp_t* q)
{
    guarded(dense_err(), [&] { delete q; });      // the batch, if one was built, through lcqp_hip_batch_destroy
}

extern "C" int lcqp_hip_qp_set_options(lcqp_hip_qp_t* q, const lcqp_options_t* opt)
{ return guarded(dense_err(), [&] {
    if (!q || !opt) return LCQP_INVALID_ARGUMENT;
    q->opt = *opt;
    q->haveBounds = false;   // forces a fresh setup (rho / sigma / prox weights enter the factorisations)
    q->solved = false;
    return 0;
}); }

static bool same_pattern(const std::vector<double>& a0, const std::vector<double>& b0, const double* a1, const double* b1, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        const double lo1 = a1 ? a1[i] : -INFINITY, hi1 = b1 ? b1[i] : INFINITY;
        const bool fin0 = std::isfinite(a0[i]) || std::isfinite(b0[i]), fin1 = std::isfinite(lo1) || std::isfinite(hi1);
        const bool eq0 = a0[i] == b0[i], eq1 = lo1 == hi1;
        if (fin0 != fin1 || eq0 != eq1) return false;
    }
    return true;
}

// The one failure path of lcqp_hip_qp_solve; QPCHK takes it with "<call>: <HIP reason>" in the error slot, as HIPCHK does.
static int qp_fail(int* exit_flag) { *exit_flag = -1; return LCQP_SUBPROBLEM_SOLVER_ERROR; }
#define QPCHK(call)                                                                             \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) { hip_fail(dense_err(), #call, e_); return qp_fail(exit_flag); }  \
    } while (0)

extern "C" int lcqp_hip_qp_solve(lcqp_hip_qp_t* q, int initialSolve, int* iterations, int* exit_flag,
                                 const double* g, const double* lbA, const double* ubA,
                                 const double* x0, const double* y0, const double* lb, const double* ub)
{ return guarded(dense_err(), [&] {
    if (!q || !g || !iterations || !exit_flag) return LCQP_INVALID_ARGUMENT;
    const int n = q->nV, nC = q->nC;
    *iterations = 0; *exit_flag = 0;
    q->solved = false;
    const bool needBox = (lb != nullptr) || (ub != nullptr);
    bool fresh = initialSolve || !q->hb || !q->haveBounds;
    if (!fresh) {
        if (needBox && !q->withBox) fresh = true;
        else if (!same_pattern(q->lbA, q->ubA, lbA, ubA, nC) || !same_pattern(q->lb, q->ub, lb, ub, n)) fresh = true;
    }
    if (q->hb && (fresh && (needBox && !q->withBox))) q->hb.reset();
    if (!q->hb) {
        q->hb.reset(lcqp_hip_batch_create(1, n, nC, 0, needBox ? 1 : 0, q->device));
        if (!q->hb) return qp_fail(exit_flag);
        q->withBox = needBox;
        fresh = true;
    }
    lcqp_hip_batch* h = q->hb.get();
    DevBatch& d = h->db;
    QPCHK(hipSetDevice(h->device));
    q->lbA.assign(nC, -INFINITY); q->ubA.assign(nC, INFINITY); q->lb.assign(n, -INFINITY); q->ub.assign(n, INFINITY);
    for (int i = 0; i < nC; i++) { if (lbA) q->lbA[i] = lbA[i]; if (ubA) q->ubA[i] = ubA[i]; }
    for (int i = 0; i < n; i++) { if (lb) q->lb[i] = lb[i]; if (ub) q->ub[i] = ub[i]; }
    q->haveBounds = true;
    int rc;
    if (fresh) {
        // the return is not looked at: options with nDynamicPenalty > 64 are refused and not stored, and the solve goes on with the options
        // the batch holds (those of its creation, or the last ones it accepted)
        lcqp_hip_batch_set_options(h, &q->opt);
        // batch of one, nComp = 0: the "A" block carries all stacked rows; L/R are empty
        double dummy = 0.0;
        rc = lcqp_hip_batch_load(h, 0, 1, q->Q.data(), g, &dummy, &dummy, nullptr, nullptr, nullptr, nullptr,
                                 nC ? q->A.data() : nullptr, q->lbA.data(), q->ubA.data(),
                                 q->withBox ? q->lb.data() : nullptr, q->withBox ? q->ub.data() : nullptr, x0, y0);
        if (rc) return qp_fail(exit_flag);
        rc = launch_setup(h);
        if (rc) return qp_fail(exit_flag);
        initialSolve = 1;
    } else {
        // same pattern: refresh bound values (finite/equality pattern unchanged, factorisations stay valid)
        std::vector<double> l(d.mEcap, 0.0), u(d.mEcap, 0.0);
        for (int r = 0; r < nC; r++) { l[r] = q->lbA[r]; u[r] = q->ubA[r]; }
        int k = 0;
        for (int i = 0; i < n; i++)
            if (std::isfinite(q->lb[i]) || std::isfinite(q->ub[i])) { l[nC + k] = q->lb[i]; u[nC + k] = q->ub[i]; k++; }
        QPCHK(hipMemcpyAsync(d.mv + (size_t)M_L * d.mEcap, l.data(), sizeof(double) * d.mEcap, hipMemcpyHostToDevice, h->stream));
        QPCHK(hipMemcpyAsync(d.mv + (size_t)M_U * d.mEcap, u.data(), sizeof(double) * d.mEcap, hipMemcpyHostToDevice, h->stream));
        // new bound values: the safe margins of the row screening (M_MG, relative to the old bounds) are void -- NaN margins make
        // the next residual sweep read every row
        QPCHK(hipMemsetAsync(d.mv + (size_t)M_MG * d.mEcap, 0xFF, sizeof(double) * d.mEcap, h->stream));
        QPCHK(hipStreamSynchronize(h->stream));
    }
    // linear term of this call
    std::vector<double> gp(d.np, 0.0);
    memcpy(gp.data(), g, sizeof(double) * n);
    QPCHK(hipMemcpyAsync(d.nv + (size_t)V_GK * d.np, gp.data(), sizeof(double) * d.np, hipMemcpyHostToDevice, h->stream));
    run_kernels(h).qp_solve(d, 1, h->stream, initialSolve ? 1 : 0);
    QPCHK(hipGetLastError());
    lcqp_stats_t st;
    QPCHK(hipStreamSynchronize(h->stream));
    QPCHK(hipMemcpy(&st, d.stats, sizeof(st), hipMemcpyDeviceToHost));
    *iterations = st.subproblemIter;
    *exit_flag = st.qpSolverExitFlag;
    q->cAdmm += st.admmIter; q->cTrials += st.trials; q->cFact += st.factorizations; q->cCorr += st.corrections;
    if (st.qpSolverExitFlag != 0) return LCQP_SUBPROBLEM_SOLVER_ERROR;
    QPCHK(hipMemcpy(q->xsol.data(), d.xout, sizeof(double) * n, hipMemcpyDeviceToHost));
    QPCHK(hipMemcpy(q->ysol.data(), d.yout, sizeof(double) * ((size_t)n + nC), hipMemcpyDeviceToHost));
    q->solved = true;
    return LCQP_SUCCESSFUL_RETURN;
}); }

extern "C" void lcqp_hip_qp_get_solution(lcqp_hip_qp_t* q, double* x, double* y)
{ guarded(dense_err(), [&] {
    if (!q) return;
    if (x) memcpy(x, q->xsol.data(), sizeof(double) * q->nV);
    if (y) memcpy(y, q->ysol.data(), sizeof(double) * ((size_t)q->nV + q->nC));
}); }

extern "C" void lcqp_hip_qp_get_counters(lcqp_hip_qp_t* q, int* admm, int* trials, int* factorizations, int* corrections)
{ guarded(dense_err(), [&] {
    if (!q) return;
    if (admm) *admm = q->cAdmm;
    if (trials) *trials = q->cTrials;
    if (factorizations) *factorizations = q->cFact;
    if (corrections) *corrections = q->cCorr;
}); }

// the QP object is a batch of one: the same three readers through its batch (LCQP_LCQPOBJECT_NOT_SETUP before the first solve built it)
extern "C" int lcqp_hip_qp_read_setup(lcqp_hip_qp_t* q, int dims[9], double scal[2], double* Cm, double* F1, double* D1, double* Et,
                                      double* MM, int* Cp, int* Ci, double* Cv)
{
    if (!q) return LCQP_INVALID_ARGUMENT;
    if (!q->hb) return LCQP_LCQPOBJECT_NOT_SETUP;
    return lcqp_hip_batch_read_setup(q->hb.get(), 0, dims, scal, Cm, F1, D1, Et, MM, Cp, Ci, Cv);
}

extern "C" int lcqp_hip_qp_read_working_set(lcqp_hip_qp_t* q, int dims[2], int* slot_row, int* crow, int* row_slot, double* Ti)
{
    if (!q) return LCQP_INVALID_ARGUMENT;
    if (!q->hb) return LCQP_LCQPOBJECT_NOT_SETUP;
    return lcqp_hip_batch_read_working_set(q->hb.get(), 0, dims, slot_row, crow, row_slot, Ti);
}

extern "C" int lcqp_hip_qp_read_admm(lcqp_hip_qp_t* q, int dims[6], double scal[3], double* FK, double* rhov, double* l, double* u,
                                     double* xa, double* ya, double* za, double* dy, double* dx)
{
    if (!q) return LCQP_INVALID_ARGUMENT;
    if (!q->hb) return LCQP_LCQPOBJECT_NOT_SETUP;
    return lcqp_hip_batch_read_admm(q->hb.get(), 0, dims, scal, FK, rhov, l, u, xa, ya, za, dy, dx);
}

extern "C" int lcqp_hip_qp_read_polish(lcqp_hip_qp_t* q, int dims[12], double scal[7], double* V, double* M, int* I)
{
    if (!q) return LCQP_INVALID_ARGUMENT;
    if (!q->hb) return LCQP_LCQPOBJECT_NOT_SETUP;
    return lcqp_hip_batch_read_polish(q->hb.get(), 0, dims, scal, V, M, I);
}

// the derivatives of the convex QP last solved: k_sensitivity on the batch of one (dg [nrhs][nV], db / side [.][nV + nC], info [1])
extern "C" int lcqp_hip_qp_sensitivity(lcqp_hip_qp_t* q, int nrhs, const double* v, double* dg, double* db, int* side, int* info)
{ return guarded(dense_err(), [&] {
    if (!q || nrhs < 1 || !v || !dg) return LCQP_INVALID_ARGUMENT;
    if (!q->hb || !q->solved) return LCQP_LCQPOBJECT_NOT_SETUP;
    return batch_sensitivity(q->hb.get(), false, nrhs, v, dg, db, side, info);
}); }

// the full adjoint on the batch of one (lcqp_hip_batch_adjoint): vy, db, side [nV + nC]; dQ [nV][nV], dA [nC][nV] (the stacked rows) may be NULL
extern "C" int lcqp_hip_qp_adjoint(lcqp_hip_qp_t* q, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                                   double* dQ, double* dA)
{ return guarded(dense_err(), [&] {
    if (!q || !vx || !dg) return LCQP_INVALID_ARGUMENT;
    if (!q->hb || !q->solved) return LCQP_LCQPOBJECT_NOT_SETUP;
    return batch_adjoint(q->hb.get(), vx, vy, dg, db, side, info, 0, dQ, dA, nullptr, nullptr);
}); }

// the blocked twins on the batch of one (lcqp_hip_batch_sensitivity_blocked, lcqp_hip_batch_jacobian)
extern "C" int lcqp_hip_qp_sensitivity_blocked(lcqp_hip_qp_t* q, int nrhs, const double* v, double* dg, double* db, int* side, int* info)
{ return guarded(dense_err(), [&] {
    if (!q || nrhs < 1 || !v || !dg) return LCQP_INVALID_ARGUMENT;
    if (!q->hb || !q->solved) return LCQP_LCQPOBJECT_NOT_SETUP;
    return batch_sensitivity(q->hb.get(), true, nrhs, v, dg, db, side, info);
}); }

extern "C" int lcqp_hip_qp_jacobian(lcqp_hip_qp_t* q, double* Jg, double* Jb, int* side, int* info)
{ return guarded(dense_err(), [&] {
    if (!q || !Jg) return LCQP_INVALID_ARGUMENT;
    if (!q->hb || !q->solved) return LCQP_LCQPOBJECT_NOT_SETUP;
    return dense_jacobian(q->hb.get(), 0, 1, Jg, Jb, side, info, false);
}); }
