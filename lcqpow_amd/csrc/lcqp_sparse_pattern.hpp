// lcqp_sparse_pattern.hpp -- the pattern analysis of the sparse arm: everything lcqp_hip_sparse_create (lcqp_sparse_host.hip) derives from the CSC
// patterns of Q and of the stacked [A; L; R] before it touches a device -- checks, CSR form, the orderings of the KKT matrix and the choice
// between band, bordered band and general LDL', the band maps of each ordering, the border lists, the ELL slabs of the gathers.  Host only,
// once per pattern; no HIP in this file (CPU checks: tests/cpp/sparse_pattern_test.cpp).
#pragma once
#include "lcqp_sparse_general.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <queue>
#include <string>
#include <utility>
#include <vector>

namespace lcqp_pattern {

constexpr int SP_WMAX = 63;
constexpr int SP_KBMAX = 16;             // border nodes of the bordered band (rows / variables too dense for a band)
constexpr int GEN_MAX_FRONT = 576;       // panel of the largest front: 576 x 8 doubles beside nothing else in the 40 KB of a wavefront

// runtime test hooks that change the analysis, read from the environment by lcqp_hip_sparse_create: LCQP_SPARSE_GENERAL=1 (the general LDL'
// on a pattern the band engine would take), LCQP_SPARSE_LANES (16, 32 or 64 lanes per instance when that is more than the band needs),
// LCQP_SPARSE_ORDERING=nd|md (the ordering of the general LDL' whatever the choice rule says; it sends no band pattern to the general engine)
enum { ORDER_BAND = 0, ORDER_ND = 1, ORDER_MD = 2 };      // Pattern::ordering, lcqp_hip_sparse_general_ordering
struct Hooks { bool general = false; int lanes = 0; int ordering = 0; };

// the size class of a front in the kernels (the QR = 1, 4, 9 rows per lane of lcqp_sparse_factor.hpp); 3: beyond what they take
inline int front_class(int ff) { return ff <= 64 ? 0 : (ff <= 256 ? 1 : (ff <= GEN_MAX_FRONT ? 2 : 3)); }

// what depends on the ordering: perm[position] = node and its inverse, band slot of every entry of Q and E (-1: not in the band -- an
// upper-triangle entry of Q, or an entry of the border), where every off-diagonal band entry comes from (assembly inside the factorisation:
// -1 nothing, k < nnzQ the entry k of Q, nnzQ + k the entry k of E in CSR order) and the row of E that gates it, the diagonal of every
// position, the band positions of U; rowsFollow: every row of the band comes behind one of its variables (the light regularisation, sp_polish)
struct Ordering { std::vector<int> perm, iperm, bandQ, bandE, bsrc, bgate, bdiag, Upos; bool rowsFollow = false; };

// host arrays of the ELL slab of one gather (g_ell): entry q of row i at [q * rows + i]; no position slab (epos) without a value map
struct Ell { int W = 0, tails = 0; std::vector<int> eidx, epos; };

struct Pattern {
    int n = 0, m = 0, N = 0, nnzQ = 0, nnzE = 0;
    int w = 0, G = 0, kb = 0;     // half bandwidth (at least 1; the general LDL' has no band), lanes per instance, border nodes
    bool general = false, hasB = false;
    int ordering = ORDER_BAND;    // of the general LDL': ORDER_ND or ORDER_MD
    std::vector<int> Ep, Ei, csr2csc, ETp, ETi, ETmap;      // E in CSR (csr2csc: its value order in the caller's CSC) and in CSC (ETmap: CSC -> CSR)
    std::vector<int> qdiag, Erow;                           // entry of Q_ii (-1: none), row of every CSR entry of E
    Ordering ord[2];                                        // [0] reverse Cuthill-McKee, [1] its rows-follow variant (hasB)
    std::vector<int> border, Uptr, Usrc, Ugate, Cptr, Cb2, Csrc, Cgate;
    Ell ellQ, ellE, ellT;                                   // rows of Q, rows of E, columns of E
    lcqp_general::Symbolic sym;                             // the general LDL' (general only)
    std::string note;                                       // of a refused pattern: what the message does not say (a minimum-degree ordering that fits but is not taken)
};

// The pattern is taken at its word below, so it is checked first: column pointers start at 0 and never decrease; row indices inside a
// column strictly increase (sorted, no duplicates: a duplicate would share one band slot and lose a value); Q structurally symmetric
// (both triangles given, as the reference hands Q to OSQP's P -- only entries with a mirror image reach the band)
inline bool check_pattern(int n, int m, const int* Qp, const int* Qi, const int* Ap, const int* Ai, std::string& err)
{
    for (int pass = 0; pass < 2; pass++) {
        const int* P = pass ? Ap : Qp; const int* I = pass ? Ai : Qi; const int rows = pass ? m : n;
        if (P[0] != 0) { err = "column pointers must start at 0"; return false; }
        for (int c = 0; c < n; c++) {
            if (P[c + 1] < P[c]) { err = "column pointers must not decrease"; return false; }
            for (int k = P[c]; k < P[c + 1]; k++) {
                if (I[k] < 0 || I[k] >= rows) { err = pass ? "row index out of bounds" : "Q index out of bounds"; return false; }
                if (k > P[c] && I[k] <= I[k - 1]) { err = "row indices of a column must be sorted and free of duplicates"; return false; }
            }
        }
    }
    for (int c = 0; c < n; c++)
        for (int k = Qp[c]; k < Qp[c + 1]; k++) {
            const int r = Qi[k];
            if (r == c) continue;
            if (!std::binary_search(Qi + Qp[r], Qi + Qp[r + 1], c)) { err = "Q must be structurally symmetric (both triangles given)"; return false; }
        }
    return true;
}

// CSC of the stacked matrix -> CSR (pattern and the value permutation)
inline void csc_to_csr(int n, int m, const int* Ap, const int* Ai, Pattern& P)
{
    const int nnzA = Ap[n];
    P.Ep.assign(m + 1, 0); P.Ei.resize(nnzA); P.csr2csc.resize(nnzA); P.ETp.assign(Ap, Ap + n + 1); P.ETi.assign(Ai, Ai + nnzA); P.ETmap.resize(nnzA);
    for (int k = 0; k < nnzA; k++) P.Ep[Ai[k] + 1]++;
    for (int r = 0; r < m; r++) P.Ep[r + 1] += P.Ep[r];
    std::vector<int> cur(P.Ep.begin(), P.Ep.end() - 1);
    for (int c = 0; c < n; c++) for (int k = Ap[c]; k < Ap[c + 1]; k++) { const int d = cur[Ai[k]]++; P.Ei[d] = c; P.csr2csc[d] = k; P.ETmap[k] = d; }
    P.Erow.resize(nnzA);
    for (int r = 0; r < m; r++) for (int k = P.Ep[r]; k < P.Ep[r + 1]; k++) P.Erow[k] = r;
}

// KKT graph: nodes 0..n-1 variables, n..n+m-1 rows; sorted adjacency lists without self loops
inline std::vector<std::vector<int>> kkt_graph(int n, int m, const int* Qp, const int* Qi, const std::vector<int>& Ep, const std::vector<int>& Ei)
{
    std::vector<std::vector<int>> adj(n + m);
    for (int i = 0; i < n; i++) for (int k = Qp[i]; k < Qp[i + 1]; k++) { const int j = Qi[k]; if (j != i) adj[i].push_back(j); }
    for (int r = 0; r < m; r++) for (int k = Ep[r]; k < Ep[r + 1]; k++) { adj[n + r].push_back(Ei[k]); adj[Ei[k]].push_back(n + r); }
    for (auto& a : adj) { std::sort(a.begin(), a.end()); a.erase(std::unique(a.begin(), a.end()), a.end()); }
    return adj;
}

// reverse Cuthill-McKee ordering of a graph
inline void rcm_order(int N, const std::vector<std::vector<int>>& adj, std::vector<int>& perm)
{
    std::vector<int> deg(N), order; std::vector<char> seen(N, 0);
    for (int i = 0; i < N; i++) deg[i] = (int)adj[i].size();
    order.reserve(N);
    auto bfs = [&](int start, std::vector<int>& out, std::vector<char>& mark) {
        std::queue<int> q; q.push(start); mark[start] = 1;
        while (!q.empty()) {
            const int v = q.front(); q.pop(); out.push_back(v);
            std::vector<int> nb;
            for (int u : adj[v]) if (!mark[u]) { mark[u] = 1; nb.push_back(u); }
            std::sort(nb.begin(), nb.end(), [&](int a, int b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; });
            for (int u : nb) q.push(u);
        }
    };
    for (int s0 = 0; s0 < N; s0++) {
        if (seen[s0]) continue;
        // pseudo-peripheral start: the last node of a BFS from the minimum-degree node of the component, twice
        int start = s0;
        for (int pass = 0; pass < 2; pass++) {
            std::vector<int> tmp; std::vector<char> mk(seen.begin(), seen.end());
            bfs(start, tmp, mk);
            if (pass == 0) { int best = tmp[0]; for (int v : tmp) if (deg[v] < deg[best]) best = v; start = best; }
            else start = tmp.back();
        }
        bfs(start, order, seen);
    }
    perm.assign(order.rbegin(), order.rend());
}

// half bandwidth of the graph `sub` of the band nodes (border nodes have no edges in it) in the ordering pm
inline int half_bandwidth(const std::vector<int>& pm, const std::vector<std::vector<int>>& sub)
{
    const int N = (int)pm.size();
    std::vector<int> ip(N);
    for (int p = 0; p < N; p++) ip[pm[p]] = p;
    int wv = 0;
    for (int v = 0; v < N; v++) for (int u : sub[v]) wv = std::max(wv, std::abs(ip[v] - ip[u]));
    return wv;
}

// Ordering: reverse Cuthill-McKee; while the half bandwidth exceeds what a lane group covers, the node of highest degree moves to the
// border (at most SP_KBMAX nodes), the positions behind the band.  Arrow-shaped KKT matrices (a coupling row, a shared variable:
// examples/OptimizeOnCircle.cpp:44) become a narrow band plus a few border nodes.  Neither a banded nor a bordered problem: the general sparse
// LDL' (round 6; until then such a pattern was refused here and ran densified).  Sets P.ord[0].perm, P.border, P.general, P.ordering, P.sym;
// sub = the graph of the band nodes, wA = the half bandwidth of the ordering.
// The ordering of the general LDL': nested dissection, as before there was a choice.  Minimum degree (lcqp_sparse_general.hpp) takes its
// place ONLY where nested dissection is refused -- a front beyond GEN_MAX_FRONT rows or storage beyond the 32-bit offsets --, or where the
// largest front of minimum degree lies in a strictly lower size class of the kernels (front_class) AND its flops are lower; a tie keeps
// nested dissection.  In both cases minimum degree must not need MORE FRONTS than nested dissection: a front costs its fixed time whatever
// its size (lcqp_sparse_general.hpp), and the patterns on which minimum degree pays with fronts are those with dense rows -- forty or sixty
// rows over every variable: each variable becomes a front of its own under all of those rows, its update block on the stack beside
// those of the others -- which are dense in earnest: they keep the single large front of nested dissection, or stay refused and run on
// the dense kernels.  No tuned threshold: the class boundaries are where the kernels change their code.  What neither ordering fits is
// refused; where both exceed the limits the message names both largest fronts.
inline bool order_kkt(const int* Qp, const int* Qi, const std::vector<std::vector<int>>& adj, const Hooks& hooks, Pattern& P,
                      std::vector<std::vector<int>>& sub, int& wA, std::string& err)
{
    const bool forceGeneral = hooks.general;
    const int n = P.n, m = P.m, N = P.N;
    std::vector<int>& permA = P.ord[0].perm;
    std::vector<int>& border = P.border;
    bool general = forceGeneral;
    std::vector<char> isBorder(N, 0);
    sub.assign(N, std::vector<int>());
    wA = 0;
    for (; !general;) {
        for (int v = 0; v < N; v++) { sub[v].clear(); if (!isBorder[v]) for (int u : adj[v]) if (!isBorder[u]) sub[v].push_back(u); }
        std::vector<int> full;
        rcm_order(N, sub, full);
        permA.clear();
        for (int v : full) if (!isBorder[v]) permA.push_back(v);
        for (int v : border) permA.push_back(v);
        wA = half_bandwidth(permA, sub);
        if (wA <= SP_WMAX) break;
        if ((int)border.size() >= SP_KBMAX) { general = true; break; }
        int best = -1; size_t deg = 0;
        for (int v = 0; v < N; v++) if (!isBorder[v] && sub[v].size() > deg) { deg = sub[v].size(); best = v; }
        if (best < 0) { err = "ordering failed"; return false; }
        isBorder[best] = 1; border.push_back(best);
    }
    if (general) {
        using lcqp_general::Symbolic;
        auto refused = [](const Symbolic& s) { return s.maxFront > GEN_MAX_FRONT || s.Lsize >= (1LL << 28) || s.stackSize >= (1LL << 28); };
        Symbolic nd, md;
        if (hooks.ordering != ORDER_MD) nd = lcqp_general::analyze(n, m, adj, Qp, Qi, P.Ep.data(), P.Ei.data(), 32);
        // (minimum degree cannot win the class rule against a nested dissection whose fronts are all of the lowest class: not computed then)
        const bool tryMd = hooks.ordering == ORDER_MD || (hooks.ordering != ORDER_ND && (refused(nd) || front_class(nd.maxFront) > 0));
        if (tryMd) {
            md = lcqp_general::analyze_md(n, m, adj, Qp, Qi, P.Ep.data(), P.Ei.data());
            const std::string bad = lcqp_general::symbolic_violation(md);
            if (!bad.empty()) { err = "minimum-degree analysis: " + bad; return false; }
        }
        const bool takeMd = hooks.ordering == ORDER_MD ||
                            (tryMd && !refused(md) && md.nF <= nd.nF && (refused(nd) || (front_class(md.maxFront) < front_class(nd.maxFront) && md.flops < nd.flops)));
        P.ordering = takeMd ? ORDER_MD : ORDER_ND;
        if (refused(takeMd ? md : nd)) {
            const Symbolic& s = takeMd ? md : nd;
            const bool both = hooks.ordering == 0 && tryMd && refused(md);
            err = "general sparse LDL' of this pattern: largest front " + std::to_string(s.maxFront) +
                  (both ? " (nested dissection), " + std::to_string(md.maxFront) + " (minimum degree)" : std::string()) + " (limit " + std::to_string(GEN_MAX_FRONT) + "), " +
                  std::to_string((long long)s.Lsize) + " factor entries: too dense for the sparse engine (use the dense kernels)";
            // (the message of a pattern that nested dissection alone decides stays what it was; what follows goes beside it)
            if (hooks.ordering == 0 && tryMd && !refused(md) && md.nF > nd.nF)
                P.note = "; a minimum-degree ordering fits (largest front " + std::to_string(md.maxFront) + ") but needs " + std::to_string(md.nF) +
                         " fronts against " + std::to_string(nd.nF) + " and is not taken (LCQP_SPARSE_ORDERING=md runs it)";
            return false;
        }
        P.sym = takeMd ? std::move(md) : std::move(nd);
        const Symbolic& sym = P.sym;
        border.clear();
        permA = sym.perm; wA = 0;
        sub = adj;
    }
    P.general = general;
    return true;
}

// A second ordering of the same band nodes for batches whose Hessians are safely definite (chosen at run time, sp_choose_ordering): a
// constraint row eliminated before every variable it touches gets the bare dual regularisation as its pivot (the LDL' is not pivoted),
// which rules out the light regularisation of the polish (sp_polish).  Here such rows move to just behind their first variable, so that
// every row pivot is -(delta2 + e D^-1 e').  With a Hessian that is nearly flat in that variable the same move is harmful (two active
// rows that hinge on it cancel), hence the choice by the data.
// Reverse Cuthill-McKee happens to put most multiplier nodes in front of their variables, and a band is as wide backwards: the second
// ordering is the first one reversed, and what rows are still in front of all their variables move behind the first of them.
inline std::vector<int> rows_follow_order(int n, int Nband, const std::vector<int>& permA, const std::vector<std::vector<int>>& sub)
{
    const int N = (int)permA.size();
    std::vector<int> permB(permA);
    std::reverse(permB.begin(), permB.begin() + Nband);
    std::vector<int> pos(N, -1), base(permB);
    for (int p = 0; p < Nband; p++) pos[base[p]] = p;
    std::vector<std::pair<double, int>> key(Nband);
    for (int p = 0; p < Nband; p++) {
        const int v = base[p];
        double k = p;
        if (v >= n) {
            int first = 1 << 30;
            for (int u : sub[v]) if (u < n && pos[u] >= 0) first = std::min(first, pos[u]);
            if (first != (1 << 30) && first > p) k = first + 0.5;
        }
        key[p] = {k, v};
    }
    std::stable_sort(key.begin(), key.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
    for (int p = 0; p < Nband; p++) permB[p] = key[p].second;
    return permB;
}

// lanes per instance: the smallest of 8, 16, 32, 64 above the half bandwidth
inline int lanes_for(int wv) { return wv < 8 ? 8 : (wv < 16 ? 16 : (wv < 32 ? 32 : 64)); }

// The border: per border node its entries with band nodes (U) and with border nodes of lower index (C); the enumeration order does not
// depend on the ordering of the band.  Returns the band node of every entry of U.
inline std::vector<int> border_lists(const int* Qp, const int* Qi, Pattern& P)
{
    const int n = P.n, kb = P.kb, nnzQ = P.nnzQ;
    std::vector<int> Uother, bidx(P.N, -1);
    P.Uptr.assign(kb + 1, 0); P.Cptr.assign(kb + 1, 0);
    for (int b = 0; b < kb; b++) bidx[P.border[b]] = b;
    for (int b = 0; b < kb; b++) {
        const int v = P.border[b];
        auto put = [&](int other, int src, int gate) {
            if (bidx[other] < 0) { Uother.push_back(other); P.Usrc.push_back(src); P.Ugate.push_back(gate); }
            else if (bidx[other] < b) { P.Cb2.push_back(bidx[other]); P.Csrc.push_back(src); P.Cgate.push_back(gate); }
        };
        if (v < n) {
            for (int k = Qp[v]; k < Qp[v + 1]; k++) if (Qi[k] != v) put(Qi[k], k, -1);                                  // Q is symmetric: row v = column v
            for (int kc = P.ETp[v]; kc < P.ETp[v + 1]; kc++) put(n + P.ETi[kc], nnzQ + P.ETmap[kc], P.ETi[kc]);       // column v of E
        } else {
            const int r = v - n;
            for (int k = P.Ep[r]; k < P.Ep[r + 1]; k++) put(P.Ei[k], nnzQ + k, r);
        }
        P.Uptr[b + 1] = (int)Uother.size(); P.Cptr[b + 1] = (int)P.Cb2.size();
    }
    return Uother;
}

// the maps of the ordering pm (struct Ordering); band rows are stored G wide: entry k of row i is K[i][i - (G-1) + k] (zero outside the true band)
inline Ordering ordering_maps(const int* Qp, const int* Qi, const Pattern& P, const std::vector<int>& pm, const std::vector<int>& Uother)
{
    const int n = P.n, m = P.m, N = P.N, nnzQ = P.nnzQ, nnzA = P.nnzE, Nband = N - P.kb, ld = P.G, wS = P.G - 1;
    const std::vector<int>& Ep = P.Ep;
    const std::vector<int>& Ei = P.Ei;
    Ordering M;
    M.perm = pm; M.iperm.assign(N, 0);
    for (int p = 0; p < N; p++) M.iperm[pm[p]] = p;
    M.rowsFollow = true;
    for (int r = 0; r < m; r++) {
        if (M.iperm[n + r] >= Nband) continue;
        bool follows = false;
        for (int e = Ep[r]; e < Ep[r + 1]; e++) follows = follows || M.iperm[Ei[e]] < M.iperm[n + r];
        M.rowsFollow = M.rowsFollow && follows;
    }
    if (P.general) {      // no band: the maps of the band engines stay empty (sp_assemble / sp_factor_reg are never entered)
        M.bandQ.assign(nnzQ, -1); M.bandE.assign(nnzA, -1); M.bsrc.assign(1, -1); M.bgate.assign(1, -1); M.bdiag.assign(N, -1); M.Upos.assign(1, 0);
        return M;
    }
    M.bandQ.assign(nnzQ, -1); M.bandE.assign(nnzA, -1); M.bsrc.assign((size_t)N * ld, -1);
    for (int i = 0; i < n; i++) for (int k = Qp[i]; k < Qp[i + 1]; k++) { const int pi = M.iperm[i], pj = M.iperm[Qi[k]]; if (pj <= pi && pi < Nband) M.bandQ[k] = pi * ld + wS - (pi - pj); }
    for (int r = 0; r < m; r++) for (int k = Ep[r]; k < Ep[r + 1]; k++) { const int pr = M.iperm[n + r], pc = M.iperm[Ei[k]]; const int hi = std::max(pr, pc), lo = std::min(pr, pc); if (hi < Nband) M.bandE[k] = hi * ld + wS - (hi - lo); }
    for (int i = 0; i < n; i++) for (int k = Qp[i]; k < Qp[i + 1]; k++) if (Qi[k] != i && M.bandQ[k] >= 0) M.bsrc[M.bandQ[k]] = k;
    for (int r = 0; r < m; r++) for (int k = Ep[r]; k < Ep[r + 1]; k++) if (M.bandE[k] >= 0) M.bsrc[M.bandE[k]] = nnzQ + k;
    // the same information one level of indirection shorter (sp_factor_reg: load_row): the gating row of every band entry, the diagonal of every position
    M.bgate.assign((size_t)N * ld, -1);
    for (int r = 0; r < m; r++) for (int k = Ep[r]; k < Ep[r + 1]; k++) if (M.bandE[k] >= 0) M.bgate[M.bandE[k]] = r;
    if (P.G <= 16) {
        // sp_factor_reg keeps a row in UPPER form relative to its diagonal: entry k of row r is K[r + k][r] = the lower-form entry
        // (r + k, ld - 1 - k); the diagonal slot (k = 0) is described by bdiag
        std::vector<int> su((size_t)N * ld, -1), gu((size_t)N * ld, -1);
        for (int r = 0; r < N; r++)
            for (int k = 1; k < ld && r + k < N; k++) { su[(size_t)r * ld + k] = M.bsrc[(size_t)(r + k) * ld + (ld - 1 - k)]; gu[(size_t)r * ld + k] = M.bgate[(size_t)(r + k) * ld + (ld - 1 - k)]; }
        M.bsrc.swap(su); M.bgate.swap(gu);
    }
    M.bdiag.assign(N, -1);
    for (int p_ = 0; p_ < N; p_++) {
        const int node = pm[p_];
        if (p_ >= Nband) M.bdiag[p_] = INT_MIN;
        else if (node < n) M.bdiag[p_] = P.qdiag[node];
        else M.bdiag[p_] = -2 - (node - n);
    }
    M.Upos.resize(Uother.size());
    for (size_t e = 0; e < Uother.size(); e++) M.Upos[e] = M.iperm[Uother[e]];
    return M;
}

// ELL slab of a gather over `rows` rows of a compressed matrix (ptr, idx; map: value position of every entry, nullptr for the identity)
inline Ell ell_slab(int rows, const int* ptr, const int* idx, const int* map)
{
    int mx = 0;
    for (int i = 0; i < rows; i++) mx = std::max(mx, ptr[i + 1] - ptr[i]);
    Ell e;
    e.W = mx <= 4 ? 4 : 8;
    e.tails = mx > e.W ? 1 : 0;
    e.eidx.assign((size_t)e.W * rows, 0);
    std::vector<int> ep((size_t)e.W * rows, -1);
    for (int i = 0; i < rows; i++)
        for (int q = 0; q < e.W && ptr[i] + q < ptr[i + 1]; q++) { const int k = ptr[i] + q; e.eidx[(size_t)q * rows + i] = idx[k]; ep[(size_t)q * rows + i] = map ? map[k] : k; }
    if (map) e.epos.swap(ep);      // without a map the position of entry q of row i is ptr[i] + q (g_ell): no position slab
    return e;
}

// the whole analysis of a pattern: Q (nV x nV, both triangles) and the stacked [A; L; R] ((nC + 2 nComp) x nV), both CSC; false and a
// message when the pattern is malformed or too dense for the sparse engine
inline bool analyse_pattern(int nV, int nC, int nComp, const int* Qp, const int* Qi, const int* Ap, const int* Ai, const Hooks& hooks, Pattern& out,
                            std::string& err)
{
    Pattern& P = out;
    const int n = nV, m = nC + 2 * nComp, N = n + m;
    if (!check_pattern(n, m, Qp, Qi, Ap, Ai, err)) return false;
    P.n = n; P.m = m; P.N = N; P.nnzQ = Qp[n]; P.nnzE = Ap[n];
    csc_to_csr(n, m, Ap, Ai, P);
    P.qdiag.assign(n, -1);
    for (int i = 0; i < n; i++) for (int k = Qp[i]; k < Qp[i + 1]; k++) if (Qi[k] == i) P.qdiag[i] = k;
    std::vector<std::vector<int>> sub;
    int wA = 0;
    if (!order_kkt(Qp, Qi, kkt_graph(n, m, Qp, Qi, P.Ep, P.Ei), hooks, P, sub, wA, err)) return false;
    P.kb = (int)P.border.size();
    std::vector<int> permB;
    int wB = 0;
    if (!P.general) {
        permB = rows_follow_order(n, N - P.kb, P.ord[0].perm, sub);
        wB = half_bandwidth(permB, sub);
    }
    P.hasB = !P.general && wB <= SP_WMAX && lanes_for(wB) == lanes_for(wA);      // not at the price of a wider lane group
    P.w = std::max(P.hasB ? std::max(wA, wB) : wA, 1);
    // LCQP_SPARSE_LANES raises G (test hook); the general LDL' takes a wavefront
    P.G = P.general ? 64 : lanes_for(P.w);
    if ((hooks.lanes == 16 || hooks.lanes == 32 || hooks.lanes == 64) && hooks.lanes > P.G) P.G = hooks.lanes;
    const std::vector<int> Uother = border_lists(Qp, Qi, P);
    P.ord[0] = ordering_maps(Qp, Qi, P, P.ord[0].perm, Uother);
    if (P.hasB) P.ord[1] = ordering_maps(Qp, Qi, P, permB, Uother);
    P.ellQ = ell_slab(n, Qp, Qi, nullptr);
    P.ellE = ell_slab(m, P.Ep.data(), P.Ei.data(), nullptr);
    P.ellT = ell_slab(n, P.ETp.data(), P.ETi.data(), P.ETmap.data());
    return true;
}

}  // namespace lcqp_pattern
