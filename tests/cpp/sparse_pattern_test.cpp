// CPU check of the sparse arm's pattern analysis (lcqpow_amd/csrc/lcqp_sparse_pattern.hpp).  usage: sparse_pattern_test CASE_FILE
// (no GPU; run by tests/test_sparse_pattern.py, which writes the case files).  Prints what the golden records -- w as lcqp_hip_sparse_bandwidth
// reports it, G, kb, general, nF, hasB, every ordering with its rowsFollow -- or the analysis' error, then the invariants that need no golden:
// perm is a permutation; every entry of Q and E the maps place in the band sits in row max(p_i, p_j) at an offset of at most w, and bsrc / bgate
// point back to it; every entry that touches a border node is listed once in U or C; the ELL slabs reproduce the compressed rows.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../lcqpow_amd/csrc/lcqp_sparse_pattern.hpp"

using lcqp_pattern::Pattern;

static int failures = 0;
#define CHECK(cond, ...)                                                                       \
    do { if (!(cond)) { if (failures++ < 10) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_ell(const char* name, const lcqp_pattern::Ell& e, int rows, const int* ptr, const int* idx, const int* map)
{
    int mx = 0;
    for (int i = 0; i < rows; i++) mx = std::max(mx, ptr[i + 1] - ptr[i]);
    CHECK((e.W == 4 || e.W == 8) && e.tails == (mx > e.W ? 1 : 0), "%s: W %d tails %d longest row %d", name, e.W, e.tails, mx);
    CHECK(e.eidx.size() == (size_t)e.W * rows && e.epos.size() == (map ? e.eidx.size() : 0), "%s: slab sizes", name);
    if (e.eidx.size() != (size_t)e.W * rows || e.epos.size() != (map ? e.eidx.size() : 0)) return;
    for (int i = 0; i < rows; i++)
        for (int q = 0; q < e.W; q++) {
            const size_t s = (size_t)q * rows + i;
            const bool in = ptr[i] + q < ptr[i + 1];
            CHECK(e.eidx[s] == (in ? idx[ptr[i] + q] : 0), "%s: row %d entry %d", name, i, q);
            if (map) CHECK(e.epos[s] == (in ? map[ptr[i] + q] : -1), "%s: row %d position %d", name, i, q);
        }
}

static void check_ordering(const Pattern& P, const int* Qp, const int* Qi, const lcqp_pattern::Ordering& O, char which)
{
    const int n = P.n, N = P.N, nnzQ = P.nnzQ, ld = P.G, Nband = N - P.kb;
    std::vector<int> seen(N, 0);
    bool isPerm = (int)O.perm.size() == N && (int)O.iperm.size() == N;
    for (int p = 0; isPerm && p < N; p++) isPerm = O.perm[p] >= 0 && O.perm[p] < N && !seen[O.perm[p]]++ && O.iperm[O.perm[p]] == p;
    CHECK(isPerm, "perm%c is not a permutation with its inverse", which);
    if (!isPerm) return;
    for (int p = Nband; p < N; p++) CHECK(O.perm[p] == P.border[p - Nband], "perm%c: border node %d behind the band", which, p - Nband);
    if (P.general) {
        for (int b : O.bandQ) CHECK(b == -1, "perm%c: general, Q entry in a band", which);
        for (int b : O.bandE) CHECK(b == -1, "perm%c: general, E entry in a band", which);
        return;
    }
    // band slot of an entry between positions hi >= lo, and the slot of bsrc / bgate that describes it (upper form when G <= 16)
    auto src_slot = [&](int hi, int lo) { return ld <= 16 ? (size_t)lo * ld + (hi - lo) : (size_t)hi * ld + (ld - 1) - (hi - lo); };
    size_t placed = 0;
    for (int i = 0; i < n; i++)
        for (int k = Qp[i]; k < Qp[i + 1]; k++) {
            const int pi = O.iperm[i], pj = O.iperm[Qi[k]];
            if (!(pj <= pi && pi < Nband)) { CHECK(O.bandQ[k] == -1, "perm%c: Q entry %d outside the lower band placed", which, k); continue; }
            CHECK(O.bandQ[k] / ld == pi && (ld - 1) - O.bandQ[k] % ld == pi - pj && pi - pj <= P.w, "perm%c: Q entry %d at slot %d", which, k, O.bandQ[k]);
            if (Qi[k] == i) { CHECK(O.bdiag[pi] == k, "perm%c: diagonal of position %d", which, pi); continue; }
            placed++;
            CHECK(O.bsrc[src_slot(pi, pj)] == k && O.bgate[src_slot(pi, pj)] == -1, "perm%c: source of Q entry %d", which, k);
        }
    for (int r = 0; r < P.m; r++)
        for (int k = P.Ep[r]; k < P.Ep[r + 1]; k++) {
            const int pr = O.iperm[n + r], pc = O.iperm[P.Ei[k]], hi = std::max(pr, pc), lo = std::min(pr, pc);
            if (hi >= Nband) { CHECK(O.bandE[k] == -1, "perm%c: E entry %d at the border placed", which, k); continue; }
            placed++;
            CHECK(O.bandE[k] / ld == hi && (ld - 1) - O.bandE[k] % ld == hi - lo && hi - lo <= P.w, "perm%c: E entry %d at slot %d", which, k, O.bandE[k]);
            CHECK(O.bsrc[src_slot(hi, lo)] == nnzQ + k && O.bgate[src_slot(hi, lo)] == r, "perm%c: source of E entry %d", which, k);
        }
    size_t sources = 0;
    for (int s : O.bsrc) sources += s >= 0;
    CHECK(sources == placed, "perm%c: %zu band sources for %zu off-diagonal entries", which, sources, placed);
    for (int p = 0; p < N; p++) {
        const int v = O.perm[p];
        CHECK(O.bdiag[p] == (p >= Nband ? INT_MIN : v < n ? P.qdiag[v] : -2 - (v - n)), "perm%c: bdiag of position %d", which, p);
    }
}

// the two nodes of the entry src (k < nnzQ: entry k of Q in column col; else entry src - nnzQ of E in CSR order)
static void ends(const Pattern& P, const int* Qi, int col, int src, int& a, int& b)
{
    if (src < P.nnzQ) { a = col; b = Qi[src]; }
    else { a = P.n + P.Erow[src - P.nnzQ]; b = P.Ei[src - P.nnzQ]; }
}

static void check_border(const Pattern& P, const int* Qp, const int* Qi)
{
    const int n = P.n, kb = P.kb;
    std::vector<int> bidx(P.N, -1), qcol(P.nnzQ), cntQ(P.nnzQ, 0), cntE(P.nnzE, 0);
    for (int b = 0; b < kb; b++) bidx[P.border[b]] = b;
    for (int i = 0; i < n; i++) for (int k = Qp[i]; k < Qp[i + 1]; k++) qcol[k] = i;
    CHECK(P.Uptr.size() == (size_t)kb + 1 && P.Uptr[kb] == (int)P.Usrc.size() && P.Cptr[kb] == (int)P.Csrc.size(), "border list sizes");
    for (int b = 0; b < kb; b++) {
        const int v = P.border[b];
        for (int e = P.Uptr[b]; e < P.Uptr[b + 1]; e++) {
            const int src = P.Usrc[e];
            int x, y; ends(P, Qi, src < P.nnzQ ? qcol[src] : 0, src, x, y);
            const int other = x == v ? y : x;
            CHECK((x == v || y == v) && bidx[other] < 0, "U entry %d of border node %d", e, b);
            CHECK(P.Ugate[e] == (src < P.nnzQ ? -1 : P.Erow[src - P.nnzQ]), "gate of U entry %d", e);
            for (int k = 0; k < (P.hasB ? 2 : 1); k++) CHECK(P.ord[k].Upos[e] == P.ord[k].iperm[other], "Upos of U entry %d", e);
            (src < P.nnzQ ? cntQ[src] : cntE[src - P.nnzQ])++;
        }
        for (int e = P.Cptr[b]; e < P.Cptr[b + 1]; e++) {
            const int src = P.Csrc[e];
            int x, y; ends(P, Qi, src < P.nnzQ ? qcol[src] : 0, src, x, y);
            const int other = x == v ? y : x;
            CHECK((x == v || y == v) && P.Cb2[e] >= 0 && P.Cb2[e] < b && P.border[P.Cb2[e]] == other, "C entry %d of border node %d", e, b);
            CHECK(P.Cgate[e] == (src < P.nnzQ ? -1 : P.Erow[src - P.nnzQ]), "gate of C entry %d", e);
            (src < P.nnzQ ? cntQ[src] : cntE[src - P.nnzQ])++;
        }
    }
    for (int i = 0; i < n; i++)
        for (int k = Qp[i]; k < Qp[i + 1]; k++) {
            const int j = Qi[k];
            if (j == i) { CHECK(cntQ[k] == 0, "diagonal Q entry %d in a border list", k); continue; }
            const int mirror = (int)(std::lower_bound(Qi + Qp[j], Qi + Qp[j + 1], i) - Qi);
            CHECK(cntQ[k] + cntQ[mirror] == (bidx[i] >= 0 || bidx[j] >= 0 ? 1 : 0), "Q entry %d (%d, %d) listed %d times", k, i, j, cntQ[k] + cntQ[mirror]);
        }
    for (int k = 0; k < P.nnzE; k++)
        CHECK(cntE[k] == (bidx[n + P.Erow[k]] >= 0 || bidx[P.Ei[k]] >= 0 ? 1 : 0), "E entry %d listed %d times", k, cntE[k]);
}

static void check_csr(const Pattern& P, const int* Qp, const int* Qi, const int* Ap, const int* Ai)
{
    for (int r = 0; r < P.m; r++)
        for (int d = P.Ep[r]; d < P.Ep[r + 1]; d++) {
            const int k = P.csr2csc[d];
            CHECK(Ai[k] == r && Ap[P.Ei[d]] <= k && k < Ap[P.Ei[d] + 1] && P.ETmap[k] == d && P.Erow[d] == r, "CSR entry %d of row %d", d, r);
            CHECK(d == P.Ep[r] || P.Ei[d] > P.Ei[d - 1], "columns of CSR row %d ascend", r);
        }
    for (int i = 0; i < P.n; i++) CHECK(P.qdiag[i] < 0 ? !std::binary_search(Qi + Qp[i], Qi + Qp[i + 1], i) : Qi[P.qdiag[i]] == i, "qdiag of %d", i);
}

int main(int argc, char** argv)
{
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: sparse_pattern_test CASE_FILE\n"); return 2; }
    int nV, nC, nComp, nnzQ, nnzA;
    lcqp_pattern::Hooks hooks;
    int general = 0;
    if (fscanf(f, "%d %d %d %d %d", &nV, &nC, &nComp, &general, &hooks.lanes) != 5) return 2;
    hooks.general = general == 1;
    auto rd = [&](std::vector<int>& v, int cnt) { v.resize(cnt); for (int& x : v) if (fscanf(f, "%d", &x) != 1) exit(2); };
    std::vector<int> Qp, Qi, Ap, Ai;
    rd(Qp, nV + 1); if (fscanf(f, "%d", &nnzQ) != 1) return 2; rd(Qi, nnzQ);
    rd(Ap, nV + 1); if (fscanf(f, "%d", &nnzA) != 1) return 2; rd(Ai, nnzA);
    fclose(f);

    Pattern P;
    std::string err;
    if (!lcqp_pattern::analyse_pattern(nV, nC, nComp, Qp.data(), Qi.data(), Ap.data(), Ai.data(), hooks, P, err)) { printf("error %s\n", err.c_str()); return 0; }
    printf("ok\nw %d\nG %d\nkb %d\ngeneral %d\nnF %d\nhasB %d\n", P.general ? 0 : P.w, P.G, P.kb, P.general ? 1 : 0, P.general ? P.sym.nF : 0, P.hasB ? 1 : 0);
    for (int k = 0; k < (P.hasB ? 2 : 1); k++) {
        printf("perm%c", k ? 'B' : 'A');
        for (int v : P.ord[k].perm) printf(" %d", v);
        printf("\nrowsFollow%c %d\n", k ? 'B' : 'A', P.ord[k].rowsFollow ? 1 : 0);
    }

    check_csr(P, Qp.data(), Qi.data(), Ap.data(), Ai.data());
    for (int k = 0; k < (P.hasB ? 2 : 1); k++) check_ordering(P, Qp.data(), Qi.data(), P.ord[k], k ? 'B' : 'A');
    check_border(P, Qp.data(), Qi.data());
    check_ell("ellQ", P.ellQ, P.n, Qp.data(), Qi.data(), nullptr);
    check_ell("ellE", P.ellE, P.m, P.Ep.data(), P.Ei.data(), nullptr);
    check_ell("ellT", P.ellT, P.n, P.ETp.data(), P.ETi.data(), P.ETmap.data());
    printf("invariant failures %d\n", failures);
    return 0;
}
