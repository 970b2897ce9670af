// CPU check of the minimum-degree ordering of the general sparse LDL' (lcqpow_amd/csrc/lcqp_sparse_general.hpp: md_front_tree, build_symbolic,
// symbolic_violation) and of the choice between it and nested dissection (lcqp_sparse_pattern.hpp: order_kkt).  Reads a pattern, runs the whole
// analysis, and prints what tests/test_sparse_min_degree.py asserts: engine, ordering, sizes, the validity of the Symbolic (the kernels'
// assumptions, an explicit set-based elimination whose every entry must lie in some front), equality with a direct call of analyze(...)
// where nested dissection is kept, determinism, and a numeric factorisation and solve by a scalar restatement of the device's loops
// (as tests/cpp/general_ldl_test.cpp) held to the componentwise bound of tests/sparse_kkt_ref.py, with |L| |D| |L'| taken from a reference
// factor of the same matrix in the same ordering (long double, on the structure of the explicit elimination), not from the factor under test.
// usage: min_degree_test CASE_FILE [auto|nd|md] [fill] [numeric]      (no GPU)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../lcqpow_amd/csrc/lcqp_sparse_pattern.hpp"

using lcqp_general::Symbolic;
using lcqp_pattern::Pattern;

struct Factor { std::vector<double> L, Dinv, stack, F; };

// numeric factorisation: K = [Q + dprim I, Ea'; Ea, -ddual I] in the ordering S.perm; rows with use[r] == 0 are decoupled (diagonal -1)
static void factor(const Symbolic& S, int n, const double* Qx, const double* Ex, int nnzQ, double dprim, double ddual, const std::vector<int>& use, Factor& W)
{
    W.L.assign(S.Lsize, 0.0); W.Dinv.assign(S.N, 0.0); W.stack.assign(S.stackSize ? S.stackSize : 1, 0.0); W.F.assign((size_t)S.maxFront * S.maxFront, 0.0);
    for (int f = 0; f < S.nF; f++) {
        const int np = S.np[f], nb = S.nb[f], ff = np + nb;
        double* F = W.F.data();
        for (int e = 0; e < ff * ff; e++) F[e] = 0.0;
        for (int e = S.asmPtr[f]; e < S.asmPtr[f + 1]; e++) {
            const int src = S.asmSrc[e], gate = S.asmGate[e];
            F[S.asmPos[e]] = (gate >= 0 && !use[gate]) ? 0.0 : (src >= nnzQ ? Ex[src - nnzQ] : Qx[src]);      // by assignment, as the device
        }
        for (int j = 0; j < np; j++) {
            const int node = S.perm[S.piv0[f] + j];
            if (node < n) F[j + ff * j] += dprim;
            else F[j + ff * j] = use[node - n] ? -ddual : -1.0;
        }
        for (int ci = S.childPtr[f]; ci < S.childPtr[f + 1]; ci++) {
            const int c = S.child[ci], nbc = S.nb[c];
            const double* CB = W.stack.data() + S.CBoff[c];
            const int* rel = S.rel.data() + S.rowPtr[c];
            for (int b = 0; b < nbc; b++) for (int a = b; a < nbc; a++) F[rel[a] + ff * rel[b]] += CB[a + nbc * b];
        }
        for (int j = 0; j < np; j++) {
            const double dinv = 1.0 / F[j + ff * j];
            W.Dinv[S.piv0[f] + j] = dinv;
            for (int k = j + 1; k < ff; k++) {
                const double fkj = F[k + ff * j];
                if (fkj == 0.0) continue;
                for (int i = k; i < ff; i++) F[i + ff * k] -= (F[i + ff * j] * dinv) * fkj;
            }
            for (int i = j + 1; i < ff; i++) F[i + ff * j] *= dinv;
        }
        double* Lp = W.L.data() + S.Loff[f];
        for (int j = 0; j < np; j++) for (int i = j + 1; i < ff; i++) Lp[i + ff * j] = F[i + ff * j];
        double* CB = W.stack.data() + S.CBoff[f];      // (written after the children's blocks were read: the stack discipline)
        for (int b = 0; b < nb; b++) for (int a = b; a < nb; a++) CB[a + nb * b] = F[(np + a) + ff * (np + b)];
    }
}

static int pos_of(const Symbolic& S, int f, int i) { return i < S.np[f] ? S.piv0[f] + i : S.rows[S.rowPtr[f] + i - S.np[f]]; }

static void solve(const Symbolic& S, const Factor& W, std::vector<double>& b)
{
    std::vector<double> bl(S.maxFront);
    for (int f = 0; f < S.nF; f++) {
        const int np = S.np[f], ff = np + S.nb[f];
        const double* Lp = W.L.data() + S.Loff[f];
        for (int i = 0; i < ff; i++) bl[i] = b[pos_of(S, f, i)];
        for (int j = 0; j < np; j++) { const double yj = bl[j]; for (int i = j + 1; i < ff; i++) bl[i] -= Lp[i + ff * j] * yj; }
        for (int i = 0; i < ff; i++) b[pos_of(S, f, i)] = bl[i];
    }
    for (int p = 0; p < S.N; p++) b[p] *= W.Dinv[p];
    for (int f = S.nF - 1; f >= 0; f--) {
        const int np = S.np[f], ff = np + S.nb[f];
        const double* Lp = W.L.data() + S.Loff[f];
        for (int i = 0; i < ff; i++) bl[i] = b[pos_of(S, f, i)];
        for (int j = np - 1; j >= 0; j--) { double s = bl[j]; for (int i = j + 1; i < ff; i++) s -= Lp[i + ff * j] * bl[i]; bl[j] = s; }
        for (int j = 0; j < np; j++) b[S.piv0[f] + j] = bl[j];
    }
}

// The reference factor of the bound: a right-looking LDL' without pivoting in long double on the filled structure of the explicit
// elimination (rows[p]: the positions below the diagonal of column p, ascending; it shares nothing with the fronts, their assembly lists or
// the loops above).  K in position order: diag[p], and val[p][k] the entry (rows[p][k], p).  On return val holds L, diag holds D.
static void reference_ldl(const std::vector<std::vector<int>>& rows, std::vector<std::vector<long double>>& val, std::vector<long double>& diag)
{
    const int N = (int)rows.size();
    for (int p = 0; p < N; p++) {
        const std::vector<int>& r = rows[p];
        const long double d = diag[p];
        for (size_t a = 0; a < r.size(); a++) {
            const long double la = val[p][a] / d;
            if (val[p][a] != 0.0L) {
                diag[r[a]] -= la * val[p][a];
                const std::vector<int>& ra = rows[r[a]];
                size_t k = 0;
                for (size_t b = a + 1; b < r.size(); b++) {      // (r[b] is a row of column r[a]: the fill of eliminating p; both lists ascend)
                    while (ra[k] != r[b]) k++;
                    val[r[a]][k] -= la * val[p][b];
                }
            }
        }
        for (size_t a = 0; a < r.size(); a++) val[p][a] /= d;
    }
}

// Wm |x| with Wm = |L| |D| |L'| (tests/sparse_kkt_ref.py) of the reference factor; x in position order
static std::vector<long double> growth_vector(const std::vector<std::vector<int>>& rows, const std::vector<std::vector<long double>>& L, const std::vector<long double>& D,
                                              const std::vector<double>& x)
{
    const int N = (int)rows.size();
    std::vector<long double> y(N), w(N, 0.0L);
    for (int p = 0; p < N; p++) {
        long double s = std::fabs(x[p]);
        for (size_t a = 0; a < rows[p].size(); a++) s += std::fabs(L[p][a]) * std::fabs(x[rows[p][a]]);
        y[p] = s * std::fabs(D[p]);
    }
    for (int p = 0; p < N; p++) {
        w[p] += y[p];
        for (size_t a = 0; a < rows[p].size(); a++) w[rows[p][a]] += std::fabs(L[p][a]) * y[p];
    }
    return w;
}

static bool same(const Symbolic& a, const Symbolic& b)
{
    return a.N == b.N && a.nF == b.nF && a.perm == b.perm && a.iperm == b.iperm && a.piv0 == b.piv0 && a.np == b.np && a.nb == b.nb && a.parent == b.parent &&
           a.rowPtr == b.rowPtr && a.rows == b.rows && a.childPtr == b.childPtr && a.child == b.child && a.rel == b.rel && a.Loff == b.Loff && a.CBoff == b.CBoff &&
           a.asmPtr == b.asmPtr && a.asmSrc == b.asmSrc && a.asmGate == b.asmGate && a.asmPos == b.asmPos && a.Lsize == b.Lsize && a.stackSize == b.stackSize &&
           a.maxFront == b.maxFront && a.flops == b.flops && a.nnzL == b.nnzL;
}

int main(int argc, char** argv)
{
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: min_degree_test CASE_FILE [auto|nd|md] [fill] [numeric]\n"); return 2; }
    int nV, nC, nComp, nnzQ, nnzA, general = 0;
    lcqp_pattern::Hooks hooks;
    bool fill = false, numeric = false;
    for (int a = 2; a < argc; a++) {
        if (!strcmp(argv[a], "nd")) hooks.ordering = lcqp_pattern::ORDER_ND;
        else if (!strcmp(argv[a], "md")) hooks.ordering = lcqp_pattern::ORDER_MD;
        else if (!strcmp(argv[a], "fill")) fill = true;
        else if (!strcmp(argv[a], "numeric")) numeric = true;
    }
    if (fscanf(f, "%d %d %d %d %d", &nV, &nC, &nComp, &general, &hooks.lanes) != 5) return 2;
    hooks.general = general == 1;
    auto rd = [&](std::vector<int>& v, int cnt) { v.resize(cnt); for (int& x : v) if (fscanf(f, "%d", &x) != 1) exit(2); };
    std::vector<int> Qp, Qi, Ap, Ai;
    rd(Qp, nV + 1); if (fscanf(f, "%d", &nnzQ) != 1) return 2; rd(Qi, nnzQ);
    rd(Ap, nV + 1); if (fscanf(f, "%d", &nnzA) != 1) return 2; rd(Ai, nnzA);
    fclose(f);

    Pattern P, P2;
    std::string err;
    if (!lcqp_pattern::analyse_pattern(nV, nC, nComp, Qp.data(), Qi.data(), Ap.data(), Ai.data(), hooks, P, err)) { printf("error %s\nnote %s\n", err.c_str(), P.note.c_str()); return 0; }
    printf("ok\ngeneral %d\nordering %d\nkb %d\nw %d\n", P.general ? 1 : 0, P.ordering, P.kb, P.general ? 0 : P.w);
    if (!P.general) return 0;
    const Symbolic& S = P.sym;
    const int n = P.n, m = P.m, N = P.N;
    printf("N %d\nnF %d\nmaxFront %d\nLsize %lld\nflops %lld\nnnzL %lld\nstackSize %lld\n", N, S.nF, S.maxFront, S.Lsize, S.flops, S.nnzL, S.stackSize);
    {
        const std::string bad = lcqp_general::symbolic_violation(S);
        printf("violation %s\n", bad.empty() ? "none" : bad.c_str());
    }
    // determinism: a second analysis of the same pattern
    if (!lcqp_pattern::analyse_pattern(nV, nC, nComp, Qp.data(), Qi.data(), Ap.data(), Ai.data(), hooks, P2, err)) { printf("error second analysis: %s\n", err.c_str()); return 0; }
    printf("deterministic %d\n", same(S, P2.sym) && P.ord[0].perm == P2.ord[0].perm ? 1 : 0);
    // nested dissection by a direct call of analyze(...) with the arguments order_kkt gives it
    const std::vector<std::vector<int>> adj = lcqp_pattern::kkt_graph(n, m, Qp.data(), Qi.data(), P.Ep, P.Ei);
    const Symbolic nd = lcqp_general::analyze(n, m, adj, Qp.data(), Qi.data(), P.Ep.data(), P.Ei.data(), 32);
    printf("nd_nF %d\nnd_maxFront %d\nnd_Lsize %lld\nnd_flops %lld\nsame_as_analyze %d\n", nd.nF, nd.maxFront, nd.Lsize, nd.flops, same(S, nd) ? 1 : 0);

    std::vector<int> frontOf(N);
    for (int q = 0; q < S.nF; q++) for (int j = 0; j < S.np[q]; j++) frontOf[S.piv0[q] + j] = q;
    std::vector<std::vector<int>> filled(N);      // of the explicit elimination: the rows below the diagonal of every column, ascending
    if (fill || numeric) {
        // explicit elimination on sets of positions: eliminating p joins its later neighbours pairwise; every entry (a, p), a > p, of the filled
        // matrix must be a row of the front that holds the pivot p
        std::vector<std::set<int>> later(N);
        for (int v = 0; v < N; v++) for (int u : adj[v]) { const int pv = S.iperm[v], pu = S.iperm[u]; if (pu > pv) later[pv].insert(pu); }
        long long entries = 0, lost = 0;
        for (int p = 0; p < N; p++) {
            const int q = frontOf[p];
            const int* b0 = S.rows.data() + S.rowPtr[q]; const int* b1 = S.rows.data() + S.rowPtr[q + 1];
            for (auto a = later[p].begin(); a != later[p].end(); ++a) {
                entries++;
                const bool inside = (*a < S.piv0[q] + S.np[q]) || std::binary_search(b0, b1, *a);
                if (!inside) lost++;
                auto b = a;
                for (++b; b != later[p].end(); ++b) later[*a].insert(*b);
            }
        }
        for (int p = 0; p < N; p++) filled[p].assign(later[p].begin(), later[p].end());
        printf("fill_entries %lld\nfill_lost %lld\n", entries, lost);
    }
    if (numeric) {
        // values: a diagonally dominant Q (symmetric by construction: the value of a pair depends on the pair), rows of E over three decades
        unsigned long long st = 0x9E3779B97F4A7C15ULL;
        auto rnd = [&]() { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((st >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 53); };
        auto pairval = [](int a, int b) { unsigned long long h = (unsigned long long)std::min(a, b) * 1000003ULL + (unsigned long long)std::max(a, b) * 7919ULL + 12345ULL; h ^= h >> 13; h *= 0x9E3779B97F4A7C15ULL; h ^= h >> 29; return -0.2 - 0.8 * (double)(h % 100000ULL) / 100000.0; };
        std::vector<double> Qx(nnzQ), Ex(P.nnzE);
        for (int c = 0; c < n; c++) {
            double off = 0.0; int dk = -1;
            for (int k = Qp[c]; k < Qp[c + 1]; k++) { if (Qi[k] == c) dk = k; else { Qx[k] = pairval(c, Qi[k]); off += std::fabs(Qx[k]); } }
            if (dk >= 0) Qx[dk] = off + 0.5 + (double)(c % 7) * 0.25;
        }
        for (int r = 0; r < m; r++) { const double s = std::pow(10.0, 3.0 * rnd() - 1.5); for (int k = P.Ep[r]; k < P.Ep[r + 1]; k++) Ex[k] = s * (rnd() < 0.5 ? -1.0 : 1.0) * (0.5 + rnd()); }
        double worst = 0.0, worstGrowth = 0.0;
        for (int pass = 0; pass < 3; pass++) {
            std::vector<int> use(m, 1);
            if (pass == 1) for (int r = 0; r < m; r += 3) use[r] = 0;
            if (pass == 2) use.assign(m, 0);
            const double dprim = pass == 1 ? 1e-6 : 1e-8, ddual = pass == 1 ? 1e-3 : 1e-9;      // the polish pair, and a pair of the ADMM factor's size
            Factor W;
            factor(S, n, Qx.data(), Ex.data(), nnzQ, dprim, ddual, use, W);
            std::vector<double> rhs(N), b(N), x(N);
            for (int v = 0; v < N; v++) rhs[v] = 2.0 * rnd() - 1.0;
            for (int p = 0; p < N; p++) b[p] = rhs[S.perm[p]];
            solve(S, W, b);
            for (int p = 0; p < N; p++) x[S.perm[p]] = b[p];
            // residual in long double, in node order, sparse
            std::vector<long double> res(N), kx(N, 0.0L);
            for (int v = 0; v < N; v++) res[v] = rhs[v];
            for (int i = 0; i < n; i++) { for (int k = Qp[i]; k < Qp[i + 1]; k++) { res[Qi[k]] -= (long double)Qx[k] * x[i]; kx[Qi[k]] += std::fabs((long double)Qx[k] * x[i]); } res[i] -= (long double)dprim * x[i]; }
            for (int r = 0; r < m; r++) {
                if (!use[r]) { res[n + r] += x[n + r]; kx[n + r] += std::fabs(x[n + r]); continue; }
                res[n + r] += (long double)ddual * x[n + r];
                for (int k = P.Ep[r]; k < P.Ep[r + 1]; k++) { res[n + r] -= (long double)Ex[k] * x[P.Ei[k]]; res[P.Ei[k]] -= (long double)Ex[k] * x[n + r]; kx[n + r] += std::fabs((long double)Ex[k] * x[P.Ei[k]]); kx[P.Ei[k]] += std::fabs((long double)Ex[k] * x[n + r]); }
            }
            // the reference factor of the same matrix in the same ordering, and the bound from it
            std::vector<std::vector<long double>> rv(N);
            std::vector<long double> rd(N, 0.0L);
            for (int p = 0; p < N; p++) rv[p].assign(filled[p].size(), 0.0L);
            auto entry = [&](int pa, int pb, long double v) {
                if (pa == pb) { rd[pa] += v; return; }
                const int lo = std::min(pa, pb), hi = std::max(pa, pb);
                rv[lo][std::lower_bound(filled[lo].begin(), filled[lo].end(), hi) - filled[lo].begin()] += v;
            };
            for (int i = 0; i < n; i++) { for (int k = Qp[i]; k < Qp[i + 1]; k++) if (Qi[k] <= i) entry(S.iperm[i], S.iperm[Qi[k]], Qx[k]); entry(S.iperm[i], S.iperm[i], dprim); }
            for (int r = 0; r < m; r++) {
                entry(S.iperm[n + r], S.iperm[n + r], use[r] ? -(long double)ddual : -1.0L);
                if (use[r]) for (int k = P.Ep[r]; k < P.Ep[r + 1]; k++) entry(S.iperm[n + r], S.iperm[P.Ei[k]], Ex[k]);
            }
            reference_ldl(filled, rv, rd);
            const std::vector<long double> wm = growth_vector(filled, rv, rd, b);
            const long double c = (6.0L * N + 8.0L) * 2.220446049250313e-16L;
            long double gmax = 0.0L, kmax = 0.0L;
            for (int p = 0; p < N; p++) {
                const int v = S.perm[p];
                const long double bound = c * (wm[p] + std::fabs((long double)rhs[v]));
                worst = std::fmax(worst, (double)(std::fabs(res[v]) / bound));
                gmax = std::fmax(gmax, wm[p]); kmax = std::fmax(kmax, kx[v]);
            }
            worstGrowth = std::fmax(worstGrowth, (double)(gmax / kmax));
        }
        printf("bound_ratio %.3e\ngrowth %.3e\n", worst, worstGrowth);
    }
    return 0;
}
