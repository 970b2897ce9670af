// Who owns what in the host layer (lcqpow_amd/csrc/host): CSC matrices, the C ABI's handles, batch objects.  Built from the host sources with
// AddressSanitizer and UBSan against fake_lcqp_hip.cpp in place of liblcqpow_hip.so, so it needs no GPU: the fake hands out dummy handles, counts
// creates, clones and destroys, and fails a named call on request.  Every scenario ends with no live handle; what leaks on the host, is released
// with the wrong function or is read after its release stops the program through the sanitizers.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "BatchLCQProblem.hpp"
#include "LCQProblem.hpp"

using namespace LCQPow;

namespace fake {      // fake_lcqp_hip.cpp
struct Counts { int created, cloned, destroyed; };
extern Counts batch, sparse, qp;
extern int strayDestroys;
int live();
void reset();
void fail(const char* name, int nth = 1, int code = LCQP_HIP_ERROR);
}

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// the end of every scenario: nothing alive, every handle released once, by its own destroy
static void check_all_released()
{
    CHECK(fake::live() == 0 && fake::strayDestroys == 0);
    CHECK(fake::batch.created + fake::batch.cloned == fake::batch.destroyed);
    CHECK(fake::sparse.created + fake::sparse.cloned == fake::sparse.destroyed);
    CHECK(fake::qp.created + fake::qp.cloned == fake::qp.destroyed);
}

// min x'x  s.t.  0 <= x1 _|_ x2 >= 0: the fake's all-zero answers are its solution, so the host loop ends after one iterate
static const double Q2[4] = {2, 0, 0, 2}, g0[2] = {0, 0}, L2[2] = {1, 0}, R2[2] = {0, 1}, Rzero[2] = {0, 0};

static Options quiet(QPSolver arm)
{
    Options o;
    o.setPrintLevel(NONE); o.setQPSolver(arm);
    return o;
}

struct Csc2 {      // the 2-variable problem in compressed columns, R as given (the loader copies what it is handed)
    csc *Q, *L, *R;
    explicit Csc2(const double* r) : Q(Utilities::dns_to_csc(Q2, 2, 2)), L(Utilities::dns_to_csc(L2, 1, 2)), R(Utilities::dns_to_csc(r, 1, 2)) {}
    ~Csc2() { Utilities::ClearSparseMat(&Q); Utilities::ClearSparseMat(&L); Utilities::ClearSparseMat(&R); }
    ReturnValue load(LCQProblem& p) const { return p.loadLCQP(Q, g0, L, R); }
};

static void scenario_a_empty_C()
{   // no row of L and R is non-zero in both: C = L'R + R'L has no entry, and its storage is ClearSparseMat's to release
    fake::reset();
    const Csc2 m(Rzero);
    {
        LCQProblem p(2, 0, 1);
        CHECK(m.load(p) == SUCCESSFUL_RETURN);
    }
    {
        LCQProblem p(2, 0, 1);
        CHECK(m.load(p) == SUCCESSFUL_RETURN);
        CHECK(m.load(p) == SUCCESSFUL_RETURN);
        CHECK(p.switchToDenseMode() == SUCCESSFUL_RETURN);      // reads the empty C
    }
    check_all_released();
}

static void scenario_b_mode_switches()
{
    fake::reset();
    {
        LCQProblem p(2, 0, 1);
        CHECK(p.loadLCQP(Q2, g0, L2, R2) == SUCCESSFUL_RETURN);
        CHECK(p.switchToSparseMode() == SUCCESSFUL_RETURN);
        CHECK(p.switchToDenseMode() == SUCCESSFUL_RETURN);
        CHECK(p.switchToSparseMode() == SUCCESSFUL_RETURN);
        CHECK(p.loadLCQP(Q2, g0, L2, R2) == SUCCESSFUL_RETURN);
    }
    check_all_released();
}

static void scenario_c_dense_device()
{   // HIP_DENSE: a batch of one, released on every way out of runOnDevice
    fake::reset();
    {
        LCQProblem p(2, 0, 1);
        Options o = quiet(HIP_DENSE); o.setStoreSteps(true);
        p.setOptions(o);
        CHECK(p.loadLCQP(Q2, g0, L2, R2) == SUCCESSFUL_RETURN);
        CHECK(p.runSolver() == SUCCESSFUL_RETURN && p.getLastEngine() == LCQProblem::ENGINE_DENSE_DEVICE);
        OutputStatistics st; p.getOutputStatistics(st);
        CHECK(st.getIterTotal() == 1 && st.getSolutionStatus() == S_STATIONARY_SOLUTION && st.getxStepsStdVec().size() == 1);      // the fake's one-row trace
        CHECK(fake::batch.created == 1 && fake::live() == 0);
        fake::fail("lcqp_hip_batch_load");
        CHECK(p.runSolver() == SUBPROBLEM_SOLVER_ERROR && fake::live() == 0);
        fake::fail("lcqp_hip_batch_run");
        CHECK(p.runSolver() == SUBPROBLEM_SOLVER_ERROR && fake::live() == 0);
        CHECK(fake::batch.created == 3 && fake::qp.created == 0);
    }
    check_all_released();
}

static void scenario_d_sparse_device()
{   // OSQP_SPARSE with CSC data: the sparse engine, or the host loop when the engine does not take the problem
    fake::reset();
    const Csc2 m(R2);
    {
        LCQProblem p(2, 0, 1);
        p.setOptions(quiet(OSQP_SPARSE));
        CHECK(m.load(p) == SUCCESSFUL_RETURN);
        fake::fail("lcqp_hip_sparse_create");
        CHECK(p.runSolver() == SUCCESSFUL_RETURN && p.getLastEngine() == LCQProblem::ENGINE_HOST_LOOP);
        CHECK(fake::sparse.created == 0 && fake::qp.created == 1);

        CHECK(m.load(p) == SUCCESSFUL_RETURN);
        fake::fail("lcqp_hip_sparse_set_options");
        CHECK(p.runSolver() == SUCCESSFUL_RETURN && p.getLastEngine() == LCQProblem::ENGINE_HOST_LOOP);
        CHECK(fake::sparse.created == 1 && fake::sparse.destroyed == 1 && fake::qp.created == 2);

        CHECK(m.load(p) == SUCCESSFUL_RETURN);
        fake::fail("lcqp_hip_sparse_load", 1, INVALID_LOWER_COMPLEMENTARITY_BOUND);
        CHECK(p.runSolver() == INVALID_LOWER_COMPLEMENTARITY_BOUND && p.getLastEngine() == LCQProblem::ENGINE_SPARSE_DEVICE);
        CHECK(fake::sparse.created == 2 && fake::sparse.destroyed == 2);

        CHECK(m.load(p) == SUCCESSFUL_RETURN);
        CHECK(p.runSolver() == SUCCESSFUL_RETURN && p.getLastEngine() == LCQProblem::ENGINE_SPARSE_DEVICE);
        CHECK(fake::sparse.created == 3 && fake::sparse.destroyed == 3 && fake::qp.created == 2);
        double x[2] = {7, 7}, y[2] = {7, 7};
        CHECK(p.getPrimalSolution(x) == S_STATIONARY_SOLUTION && x[0] == 0 && x[1] == 0);
        CHECK(p.getNumberOfDuals() == 2 && p.getDualSolution(y) == S_STATIONARY_SOLUTION && y[0] == 0 && y[1] == 0);
    }
    check_all_released();
}

static void scenario_e_host_loop()
{   // one QP object per initializeSolver, handed on by moves; a copy of a Subsolver is a clone, a move is nothing
    fake::reset();
    {
        LCQProblem p(2, 0, 1);
        p.setOptions(quiet(HIP_DENSE)); p.setHostLoop(true);
        CHECK(p.loadLCQP(Q2, g0, L2, R2) == SUCCESSFUL_RETURN);
        for (int run = 1; run <= 3; run++) {
            CHECK(p.runSolver() == SUCCESSFUL_RETURN && p.getLastEngine() == LCQProblem::ENGINE_HOST_LOOP);
            CHECK(fake::qp.created == run && fake::qp.cloned == 0 && fake::live() == 1);      // the object of the last run lives in the problem
        }
        CHECK(fake::batch.created == 0);
    }
    check_all_released();
    fake::reset();
    {
        const double A3[6] = {1, 0, 0, 1, 1, 1};
        Subsolver a(2, 3, Q2, A3);
        CHECK(fake::qp.created == 1 && fake::qp.cloned == 0);
        Subsolver b(a);
        CHECK(fake::qp.created == 1 && fake::qp.cloned == 1);
        Subsolver c(std::move(a));
        CHECK(fake::qp.created == 1 && fake::qp.cloned == 1 && fake::live() == 2);
        c = std::move(b);
        CHECK(fake::qp.created == 1 && fake::qp.cloned == 1 && fake::live() == 1);
        Subsolver d;
        d = c;
        CHECK(fake::qp.created == 1 && fake::qp.cloned == 2 && fake::live() == 2);
    }
    check_all_released();
}

static void check_unsolved(const MixedBatchLCQProblem& mixed, int i)
{
    double x[2] = {7, 7}, y[4] = {7, 7, 7, 7};
    CHECK(mixed.getReturnValue(i) == LCQPOBJECT_NOT_SETUP);
    CHECK(mixed.getPrimalSolution(i, x) == PROBLEM_NOT_SOLVED && x[0] == 7 && x[1] == 7);
    CHECK(mixed.getDualSolution(i, y) == PROBLEM_NOT_SOLVED && y[0] == 7 && y[1] == 7 && y[2] == 7 && y[3] == 7);
    const lcqp_stats_t& st = mixed.getStats(i);
    CHECK(st.iterTotal == 0 && st.iterOuter == 0 && st.subproblemIter == 0 && st.status == 0 && st.qpSolverExitFlag == 0 && st.returnValue == 0 && st.rhoOpt == 0.0);
}

static void scenario_f_mixed_batch()
{   // two buckets, the second one's batch object cannot be created: its members have no batch behind them
    fake::reset();
    {
        const double A1[2] = {1, 1}, lbA[1] = {-1}, ubA[1] = {1};
        MixedBatchLCQProblem mixed;
        mixed.setOptions(quiet(HIP_DENSE));
        check_unsolved(mixed, -1); check_unsolved(mixed, 0);      // nothing added
        CHECK(mixed.addProblem(2, 0, 1, Q2, g0, L2, R2) == 0);
        CHECK(mixed.addProblem(2, 1, 1, Q2, g0, L2, R2, 0, 0, 0, 0, A1, lbA, ubA) == 1);
        CHECK(mixed.addProblem(2, 0, 1, Q2, g0, L2, R2) == 2);
        check_unsolved(mixed, -1); check_unsolved(mixed, 1); check_unsolved(mixed, 3);      // before any runSolver
        fake::fail("lcqp_hip_batch_create", 2);
        CHECK(mixed.runSolver() == LCQPOBJECT_NOT_SETUP && mixed.numberOfBuckets() == 2);
        CHECK(fake::batch.created == 1 && fake::live() == 1);
        check_unsolved(mixed, 1); check_unsolved(mixed, -1); check_unsolved(mixed, 3);
        double x[2] = {7, 7};
        CHECK(mixed.getReturnValue(2) == SUCCESSFUL_RETURN && mixed.getPrimalSolution(2, x) == S_STATIONARY_SOLUTION && x[0] == 0 && x[1] == 0);
        CHECK(mixed.getStats(0).iterTotal == 1);
        CHECK(mixed.runSolver() == SUCCESSFUL_RETURN);              // again, both buckets this time: the first run's batch objects go
        CHECK(fake::batch.created == 3 && fake::live() == 2 && mixed.getReturnValue(1) == SUCCESSFUL_RETURN);
    }
    check_all_released();
}

static void scenario_g_pipeline()
{
    fake::reset();
    {
        BatchPipeline pipe(3, 4, 2, 0, 1);
        CHECK(pipe.ok() && pipe.depth() == 3 && fake::batch.created == 3);
        BatchLCQProblem& b = pipe.acquire();
        CHECK(pipe.launch(b) == SUCCESSFUL_RETURN && !pipe.hasResults());
    }
    CHECK(fake::batch.destroyed == 3);
    check_all_released();
}

int main(int argc, char** argv)
{   // host_owner_test [letters]: the scenarios named, e.g. `host_owner_test cd`; all of them without an argument
    const char* which = argc > 1 ? argv[1] : "abcdefg";
    void (*const scenarios[7])() = {scenario_a_empty_C, scenario_b_mode_switches, scenario_c_dense_device, scenario_d_sparse_device,
                                    scenario_e_host_loop, scenario_f_mixed_batch, scenario_g_pipeline};
    for (const char* c = which; *c; c++)
        if (*c >= 'a' && *c <= 'g') scenarios[*c - 'a']();
    std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED%.0d\n", failures);
    return failures ? 1 : 0;
}
