// C++ test of the blocked sensitivities and Jacobians of the host layer: BatchLCQProblem::getJacobian, SubsolverHIP::getJacobian and the
// `blocked` argument of both getSensitivity (lcqp_hip_batch_sensitivity_blocked / lcqp_hip_batch_jacobian and the lcqp_hip_qp_* twins).
//   jacobian_test      runs on GPU 0; prints "ALL PASSED" and returns 0 when every check holds
// The tolerances: the blocked kernel equals the vector kernel to rounding; on these well-conditioned problems (Q = M'M/n + I) 1e-9 relative to
// the largest entry is five orders above what either kernel's rounding explains and far below any wrong entry.
#include <cmath>
#include <cstdio>
#include <vector>

#include "BatchLCQProblem.hpp"
#include "SubsolverHIP.hpp"

using namespace LCQPow;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static double maxabs(const std::vector<double>& a) { double m = 0; for (double v : a) m = std::fmax(m, std::fabs(v)); return m; }
static double maxdiff(const double* a, const double* b, size_t k) { double m = 0; for (size_t i = 0; i < k; i++) m = std::fmax(m, std::fabs(a[i] - b[i])); return m; }

static void test_batch()
{
    const int B = 4, n = 64, nC = 96, nComp = 16, nd = n + nC + 2 * nComp;
    BatchLCQProblem bt(B, n, nC, nComp);
    CHECK(bt.ok());
    Options options; options.setPrintLevel(NONE); options.setPerturbStep(false);
    CHECK(bt.setOptions(options) == SUCCESSFUL_RETURN);
    CHECK(bt.generateSynthetic(0x4C43515000000001ULL, 0) == SUCCESSFUL_RETURN);
    std::vector<double> Jg((size_t)B * n * n, 7.0), Jb((size_t)B * n * nd, 7.0);
    std::vector<int> side((size_t)B * nd, 7), info(B, 7);
    CHECK((int)bt.getJacobian(0, B, Jg.data(), Jb.data(), side.data(), info.data()) == 300);      // before the first run
    CHECK(bt.runSolver() == SUCCESSFUL_RETURN);
    const int bad[][2] = {{-1, 1}, {0, 0}, {0, -2}, {0, B + 1}, {1, B}, {B, 1}};
    for (const auto& fc : bad) CHECK((int)bt.getJacobian(fc[0], fc[1], Jg.data(), Jb.data(), side.data(), info.data()) == 100);
    CHECK((int)bt.getJacobian(0, B, 0) == 100);
    CHECK(Jg[0] == 7.0 && Jb[0] == 7.0 && side[0] == 7 && info[0] == 7);      // the refusals wrote nothing
    CHECK(bt.getJacobian(0, B, Jg.data(), Jb.data(), side.data(), info.data()) == SUCCESSFUL_RETURN);
    // the unit vectors through both kernels
    std::vector<double> eye((size_t)B * n * n, 0.0), dgv(eye.size()), dbv(Jb.size()), dgb(eye.size()), dbb(Jb.size());
    for (int b = 0; b < B; b++) for (int k = 0; k < n; k++) eye[((size_t)b * n + k) * n + k] = 1.0;
    std::vector<int> sv(side.size()), iv(B), sb(side.size()), ib(B);
    CHECK(bt.getSensitivity(n, eye.data(), dgv.data(), dbv.data(), sv.data(), iv.data()) == SUCCESSFUL_RETURN);
    CHECK(bt.getSensitivity(n, eye.data(), dgb.data(), dbb.data(), sb.data(), ib.data(), true) == SUCCESSFUL_RETURN);
    CHECK(sv == side && sb == side && iv == info && ib == info);
    const double tg = 1e-9 * maxabs(dgv), tb = 1e-9 * std::fmax(maxabs(dbv), 1.0);
    CHECK(maxabs(dgv) > 0.0);
    const double e1 = maxdiff(Jg.data(), dgv.data(), Jg.size()), e2 = maxdiff(dgb.data(), dgv.data(), Jg.size());
    const double e3 = maxdiff(Jb.data(), dbv.data(), Jb.size()), e4 = maxdiff(dbb.data(), dbv.data(), Jb.size());
    double sym = 0;
    for (int b = 0; b < B; b++) for (int k = 0; k < n; k++) for (int j = 0; j < k; j++)
        sym = std::fmax(sym, std::fabs(Jg[((size_t)b * n + k) * n + j] - Jg[((size_t)b * n + j) * n + k]));
    std::printf("batch: |Jg - vector| %.3g, |blocked - vector| %.3g (tol %.3g); Jb %.3g, %.3g (tol %.3g); |Jg - Jg'| %.3g\n", e1, e2, tg, e3, e4, tb, sym);
    CHECK(e1 <= tg && e2 <= tg && e3 <= tb && e4 <= tb && sym <= 2 * tg);
    // a sub-range returns the rows of the full call, bit for bit; Jb, side and info may be absent
    std::vector<double> part((size_t)2 * n * n);
    CHECK(bt.getJacobian(1, 2, part.data()) == SUCCESSFUL_RETURN);
    CHECK(maxdiff(part.data(), Jg.data() + (size_t)n * n, part.size()) == 0.0);
}

static void test_qp()
{
    const int n = 8, m = 4;
    std::vector<double> Q((size_t)n * n, 0.0), A((size_t)m * n, 0.0), g(n), lbA(m), ubA(m), x0(n, 0.0);
    for (int i = 0; i < n; i++) { Q[(size_t)i * n + i] = 2.0 + 0.1 * i; g[i] = (i % 2 ? 1.0 : -1.0) * (1.0 + i); }
    for (int i = 0; i + 1 < n; i++) Q[(size_t)i * n + i + 1] = Q[(size_t)(i + 1) * n + i] = 0.3;
    for (int r = 0; r < m; r++) { A[(size_t)r * n + r] = 1.0; A[(size_t)r * n + r + 4] = 0.5; lbA[r] = -0.2; ubA[r] = 0.2; }
    SubsolverHIP qp(n, m, Q.data(), A.data());
    std::vector<double> Jg((size_t)n * n, 7.0), Jb((size_t)n * (n + m), 7.0), eye((size_t)n * n, 0.0), dgv(Jg.size()), dbv(Jb.size()), dgb(Jg.size()), dbb(Jb.size());
    std::vector<int> side(n + m, 7), sv(n + m), sb(n + m);
    int info = 7, iv = 7, ib = 7;
    CHECK((int)qp.getJacobian(Jg.data()) == 300 && Jg[0] == 7.0);      // before the first solve
    CHECK((int)qp.getSensitivity(1, eye.data(), dgb.data(), 0, 0, 0, true) == 300);
    int it = 0, flag = 0;
    CHECK(qp.solve(true, it, flag, g.data(), lbA.data(), ubA.data(), x0.data()) == SUCCESSFUL_RETURN && flag == 0);
    for (int k = 0; k < n; k++) eye[(size_t)k * n + k] = 1.0;
    CHECK((int)qp.getJacobian(0) == 100);
    CHECK(qp.getJacobian(Jg.data(), Jb.data(), side.data(), &info) == SUCCESSFUL_RETURN);
    CHECK(qp.getSensitivity(n, eye.data(), dgv.data(), dbv.data(), sv.data(), &iv) == SUCCESSFUL_RETURN);
    CHECK(qp.getSensitivity(n, eye.data(), dgb.data(), dbb.data(), sb.data(), &ib, true) == SUCCESSFUL_RETURN);
    CHECK(sv == side && sb == side && iv == info && ib == info && info == 0);
    int active = 0; for (int s : side) active += s != 0;
    CHECK(active > 0);
    const double tg = 1e-9 * maxabs(dgv), tb = 1e-9 * std::fmax(maxabs(dbv), 1.0);
    const double e1 = maxdiff(Jg.data(), dgv.data(), Jg.size()), e2 = maxdiff(dgb.data(), dgv.data(), Jg.size());
    const double e3 = maxdiff(Jb.data(), dbv.data(), Jb.size()), e4 = maxdiff(dbb.data(), dbv.data(), Jb.size());
    std::printf("qp: %d active rows; |Jg - vector| %.3g, |blocked - vector| %.3g (tol %.3g); Jb %.3g, %.3g (tol %.3g)\n", active, e1, e2, tg, e3, e4, tb);
    CHECK(maxabs(dgv) > 0.0 && e1 <= tg && e2 <= tg && e3 <= tb && e4 <= tb);
}

int main()
{
    test_batch();
    test_qp();
    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("ALL PASSED\n");
    return 0;
}
