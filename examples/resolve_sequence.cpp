// Load once, then K steps of new vectors + warm re-solve: a batch of controllers that solve the same LCQP matrices
// again and again with a new linear term and new bounds.
//   resolve_sequence [B=256] [steps=5]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "BatchLCQProblem.hpp"

using namespace LCQPow;

int main(int argc, char** argv)
{
    const int B = argc > 1 ? std::atoi(argv[1]) : 256, steps = argc > 2 ? std::atoi(argv[2]) : 5;
    const int nV = 256, nC = 512, nComp = 64;
    BatchLCQProblem batch(B, nV, nC, nComp);
    if (!batch.ok()) { std::printf("could not create the batch: %s\n", lcqp_hip_last_error()); return 1; }
    Options options;
    options.setPrintLevel(NONE);
    batch.setOptions(options);
    batch.generateSynthetic(0x4C43515000000001ULL, 0);      // stands for loadLCQP: the matrices go to the device once
    if (batch.runSolver() != SUCCESSFUL_RETURN) { std::printf("runSolver failed: %s\n", lcqp_hip_last_error()); return 1; }
    std::vector<double> g((size_t)B * nV), lbA((size_t)B * nC), ubA((size_t)B * nC);
    for (int i = 0; i < B; i++)
        if (lcqp_hip_batch_read_problem(batch.handle(), i, 0, &g[(size_t)i * nV], 0, 0, 0, &lbA[(size_t)i * nC], &ubA[(size_t)i * nC])) return 1;
    std::mt19937_64 rng(0);
    std::normal_distribution<double> z(0.0, 1.0);
    for (int step = 1; step <= steps; step++) {
        for (size_t k = 0; k < g.size(); k++) g[k] *= 1.0 + 0.02 * z(rng);
        for (size_t k = 0; k < lbA.size(); k++) { const double s = 0.02 * (ubA[k] - lbA[k]) * z(rng); lbA[k] += s; ubA[k] += s; }
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < B; i++)
            if (batch.updateLCQP(i, &g[(size_t)i * nV], 0, 0, 0, 0, &lbA[(size_t)i * nC], &ubA[(size_t)i * nC]) != SUCCESSFUL_RETURN) {
                std::printf("updateLCQP failed: %s\n", lcqp_hip_last_error()); return 1;
            }
        if (batch.resolve(/*warm=*/true) != SUCCESSFUL_RETURN) { std::printf("resolve failed: %s\n", lcqp_hip_last_error()); return 1; }
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        float refresh = 0.f, solve = 0.f;
        lcqp_hip_batch_last_timing(batch.handle(), &refresh, &solve);
        int ok = 0, itMax = 0;
        long iters = 0;
        for (int i = 0; i < B; i++) {
            ok += batch.getReturnValue(i) == SUCCESSFUL_RETURN; iters += batch.getStats(i).iterTotal;
            if (batch.getStats(i).iterTotal > itMax) itMax = batch.getStats(i).iterTotal;
        }
        std::printf("step %d: %d/%d solved, iterates mean %.1f max %d, refresh %.3f ms + homotopy %.2f ms, %.1f ms with update and read-back\n",
                    step, ok, B, (double)iters / B, itMax, refresh, solve, wall * 1e3);
        if (ok != B) return 1;
    }
    int setups = 0, launches = 0;
    batch.getLaunchCounts(setups, launches);
    std::printf("%d full setup(s), %d homotopy launches\n", setups, launches);
    return setups == 1 ? 0 : 1;
}
