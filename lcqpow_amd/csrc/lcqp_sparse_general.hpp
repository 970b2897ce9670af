// lcqp_sparse_general.hpp -- symbolic analysis of the GENERAL sparse LDL' of the sparse arm (round 6): KKT patterns that are neither banded nor
// bordered (a 2-D grid, an unstructured mesh) -- what the reference's OSQP arm factorises with QDLDL whatever the pattern
// (src/SubsolverOSQP.cpp:136-152, osqp_setup; src/LCQProblem.cpp:390-441, 629-723).  Host only, once per pattern; no HIP in this file.
//
// Method: multifrontal LDL' over a front tree with DENSE fronts.  Two orderings make a front tree (nd_front_tree, md_front_tree below; the choice
// between them is order_kkt's, lcqp_sparse_pattern.hpp); one builder turns either into the Symbolic the kernels run (build_symbolic).
//   * Ordering, by default: nested dissection by breadth-first level structures (George 1973): a region larger than `leaf` nodes is cut by the level of
//     a breadth-first search from a pseudo-peripheral node that balances the two sides; both sides are ordered first, the separator last;
//     a region of at most `leaf` nodes is one leaf.  Disconnected regions are handled component by component.
//   * Fronts: every leaf and every separator is ONE front: its nodes are the pivots (contiguous positions of the ordering), its update rows
//     are the boundary of the region it closes -- the later nodes adjacent to the region --, taken as dense (the fill of eliminating a connected
//     region IS the clique on its boundary; a few explicit zeros stand where a separator node does not touch every boundary node).  The
//     front tree is the dissection tree; fronts are numbered in postorder, children before parents.
//   * Numeric (device: sp_general_factor / sp_general_solve in lcqp_sparse_factor.hpp; CPU restatement of the same loops for the tests:
//     tests/cpp/general_ldl_test.cpp): a front F (ff x ff, ff = np + nb) is zeroed, takes the entries of K whose column is one of its pivots
//     (asm lists below; entries of E are gated by the working set by VALUE, the pattern never changes), takes the update blocks of its
//     children (extend-add through `rel`), eliminates its np pivots (right-looking, no pivoting: the matrix is quasi-definite for
//     delta, delta2 > 0 and any symmetric permutation of a quasi-definite matrix factorises), stores the panel L (ff x np, column-major) and
//     1/D, and leaves its update block (nb x nb) on a stack whose offsets are fixed here.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <queue>
#include <string>
#include <utility>
#include <vector>

namespace lcqp_general {

struct Symbolic {
    int N = 0, nF = 0;
    std::vector<int> perm, iperm;             // perm[position] = node, iperm[node] = position
    // per front (postorder)
    std::vector<int> piv0, np, nb, parent;    // first pivot position, pivots, boundary rows, parent front (-1: a root)
    std::vector<int> rowPtr, rows;            // boundary rows of front f: positions rows[rowPtr[f] .. rowPtr[f+1]), ascending, all behind its pivots
    std::vector<int> childPtr, child;         // children of front f
    std::vector<int> rel;                     // rel[rowPtr[f] + a]: local index of boundary row a of front f in its PARENT's front (pivots 0 .. np-1, then boundary)
    std::vector<long long> Loff, CBoff;       // panel of front f in the factor storage (ff x np doubles, column-major, ld = ff); its update block on the stack (nb x nb, ld = nb)
    // assembly: the entries of K whose column (the earlier of the two positions) is a pivot of front f
    std::vector<int> asmPtr, asmSrc, asmGate, asmPos;   // src: k < nnzQ entry k of Q, else nnzQ + k entry k of E (CSR order); gate: row of E or -1; pos: i + ff * j (local row, local column)
    long long Lsize = 0, stackSize = 0;
    int maxFront = 0;
    long long flops = 0, nnzL = 0;
};

// What an ordering hands to build_symbolic: the ordering and the fronts in postorder (children before parents, the fronts of a subtree
// contiguous), every front a run of consecutive positions, the children of a front ascending.
struct FrontTree {
    std::vector<int> perm, piv0, np, parent;
    std::vector<std::vector<int>> children;
};

// boundaries, bottom-up (postorder = index order): later neighbours of the pivots and what the children hand up
inline std::vector<std::vector<int>> front_boundaries(const std::vector<int>& perm, const std::vector<int>& piv0, const std::vector<int>& np,
                                                      const std::vector<std::vector<int>>& children, const std::vector<std::vector<int>>& adj, const std::vector<int>& iperm)
{
    const int nF = (int)np.size();
    std::vector<std::vector<int>> bnd(nF);
    for (int f = 0; f < nF; f++) {
        const int last = piv0[f] + np[f];
        std::vector<int>& b = bnd[f];
        for (int j = 0; j < np[f]; j++) for (int u : adj[perm[piv0[f] + j]]) { const int pu = iperm[u]; if (pu >= last) b.push_back(pu); }
        for (int c : children[f]) for (int pu : bnd[c]) if (pu >= last) b.push_back(pu);
        std::sort(b.begin(), b.end()); b.erase(std::unique(b.begin(), b.end()), b.end());
    }
    return bnd;
}

// Nested dissection (the header comment): the ordering and the dissection tree.
// mergeFront: a front absorbs its LAST child (whose pivots lie right in front of its own) while the merged front stays within this many rows --
// the small separators at the bottom of the dissection tree then ride in their parents' fronts instead of costing a front of their own
// (a front costs a fixed ~20 us in a factorisation and ~5 us per sweep whatever its size; 0: no merging)
inline FrontTree nd_front_tree(int N, const std::vector<std::vector<int>>& adj, int leaf, int mergeFront)
{
    FrontTree S;
    S.perm.reserve(N);
    std::vector<int> mark(N, -1), level(N, 0), queue;      // mark[v] = id of the region v currently belongs to
    queue.reserve(N);
    int regionId = 0, nF = 0;
    std::vector<std::vector<int>>& frontChildren = S.children;

    // breadth-first search inside the nodes marked `id`, from `start`; fills `queue` (visit order) and level[]; the visited nodes are re-marked `newId`
    auto bfs = [&](int start, int id, int newId) {
        queue.clear();
        queue.push_back(start); mark[start] = newId; level[start] = 0;
        for (size_t h = 0; h < queue.size(); h++) {
            const int v = queue[h];
            for (int u : adj[v]) if (mark[u] == id) { mark[u] = newId; level[u] = level[v] + 1; queue.push_back(u); }
        }
    };
    auto new_front = [&](const std::vector<int>& pivots, const std::vector<int>& children) {
        const int f = nF++;
        S.piv0.push_back((int)S.perm.size()); S.np.push_back((int)pivots.size()); S.parent.push_back(-1);
        for (int v : pivots) S.perm.push_back(v);
        frontChildren.push_back(children);
        for (int c : children) S.parent[c] = f;
        return f;
    };
    // recursion over (node set) -> top fronts; the depth is logarithmic for every separator this routine produces (the balanced level)
    std::vector<int> rootTops;
    struct Rec {
        static void run(const std::vector<std::vector<int>>& adj, std::vector<int>& mark, std::vector<int>& level, std::vector<int>& queue,
                        int& regionId, int leaf, std::vector<int>& nodes, std::vector<int>& tops,
                        const std::function<void(int, int, int)>& bfs, const std::function<int(const std::vector<int>&, const std::vector<int>&)>& new_front)
        {
            const int id = regionId++;
            for (int v : nodes) mark[v] = id;
            for (size_t s = 0; s < nodes.size(); s++) {
                if (mark[nodes[s]] != id) continue;                   // already taken by a component found earlier
                const int compId = regionId++;
                bfs(nodes[s], id, compId);
                std::vector<int> comp(queue);
                if ((int)comp.size() <= leaf) { tops.push_back(new_front(comp, {})); continue; }
                // pseudo-peripheral start: the last node of the first search
                const int tmpId = regionId++;
                bfs(comp.back(), compId, tmpId);
                comp = queue;
                const int depth = level[comp.back()];
                if (depth < 2) { tops.push_back(new_front(comp, {})); continue; }      // clique-like: no separator to be had
                // the level that balances the two sides (not the first, not the last)
                std::vector<int> cnt(depth + 1, 0);
                for (int v : comp) cnt[level[v]]++;
                int best = 1; long long bestCost = -1, below = cnt[0];
                for (int l = 1; l < depth; l++) {
                    const long long above = (long long)comp.size() - below - cnt[l];
                    const long long cost = std::max(below, above) + 2LL * cnt[l];     // balance, with a price on the separator's size
                    if (bestCost < 0 || cost < bestCost) { bestCost = cost; best = l; }
                    below += cnt[l];
                }
                std::vector<int> A, B, sep;
                for (int v : comp) (level[v] < best ? A : (level[v] > best ? B : sep)).push_back(v);
                std::vector<int> ch;
                run(adj, mark, level, queue, regionId, leaf, A, ch, bfs, new_front);
                run(adj, mark, level, queue, regionId, leaf, B, ch, bfs, new_front);
                tops.push_back(new_front(sep, ch));
            }
        }
    };
    {
        std::vector<int> all(N);
        for (int v = 0; v < N; v++) all[v] = v;
        std::function<void(int, int, int)> bfsF = bfs;
        std::function<int(const std::vector<int>&, const std::vector<int>&)> nfF = new_front;
        Rec::run(adj, mark, level, queue, regionId, leaf, all, rootTops, bfsF, nfF);
    }
    if (mergeFront > 0) {
        std::vector<int> iperm(N);
        for (int p = 0; p < N; p++) iperm[S.perm[p]] = p;
        const std::vector<std::vector<int>> bnd = front_boundaries(S.perm, S.piv0, S.np, S.children, adj, iperm);      // (a merged front keeps the boundary of the front that absorbs)
        std::vector<char> dead(nF, 0);
        for (int f = 0; f < nF; f++) {
            while (!frontChildren[f].empty()) {
                const int c = frontChildren[f].back();
                if (S.piv0[c] + S.np[c] != S.piv0[f]) break;                                   // (the last child in postorder: always adjacent)
                if (S.np[c] + S.np[f] + (int)bnd[f].size() > mergeFront) break;
                S.piv0[f] = S.piv0[c]; S.np[f] += S.np[c];
                frontChildren[f].pop_back();
                for (int ch : frontChildren[c]) { frontChildren[f].push_back(ch); S.parent[ch] = f; }      // (indices between the other children's and c: still ascending)
                dead[c] = 1;
            }
        }
        std::vector<int> newId(nF, -1);
        int live = 0;
        for (int f = 0; f < nF; f++) if (!dead[f]) newId[f] = live++;
        std::vector<int> piv0(live), npv(live), par(live);
        std::vector<std::vector<int>> fc(live);
        for (int f = 0; f < nF; f++) {
            if (dead[f]) continue;
            const int g = newId[f];
            piv0[g] = S.piv0[f]; npv[g] = S.np[f]; par[g] = S.parent[f] >= 0 ? newId[S.parent[f]] : -1;
            for (int ch : frontChildren[f]) fc[g].push_back(newId[ch]);
        }
        S.piv0.swap(piv0); S.np.swap(npv); S.parent.swap(par); frontChildren.swap(fc);
    }
    return S;
}

// Minimum degree (for KKT graphs of small diameter -- many small blocks coupled through a few dozen shared variables --, where a
// breadth-first level holds a node of nearly every block and nested dissection has no small separator to find).
//   * Ordering: elimination on the quotient graph (George & Liu): an eliminated node becomes an ELEMENT that lists the uneliminated nodes it
//     reaches; the elements a pivot touches are absorbed into the pivot's element, so the structure of the pivot's column is known exactly
//     (its entries below the diagonal = the members of its element) without any fill being stored.  The degrees are the approximate external
//     degrees of Amestoy, Davis & Duff (1996), an upper bound that one pass over the element lists of the pivot's members gives.
//     Deterministic: of the nodes of lowest degree the one of lowest index goes first.
//   * Elimination tree: the parent of a pivot is the pivot its element is absorbed by (the first of its members to go).
//   * Fundamental supernodes: a pivot joins its only child when the child's column is the pivot plus the pivot's column (no explicit zero).
//   * Relaxed amalgamation: a supernode, taken in elimination order, absorbs children -- ANY child, lowest first -- while the merged front
//     (the pivots of both and the parent's boundary) stays within mergeFront rows: explicit zeros bought for fewer fronts.
//   * Numbering: the fronts in postorder of the amalgamated tree (roots and children in elimination order), the pivots of a front
//     contiguous, an absorbed child's in front of its parent's.
inline FrontTree md_front_tree(int N, const std::vector<std::vector<int>>& adj, int mergeFront)
{
    std::vector<std::vector<int>> A(adj), E(N), Le(N);      // uneliminated neighbours, adjacent elements, members of an element
    std::vector<int> deg(N), order, pos(N, -1), parent(N, -1), count(N, 0), mark(N, -1), w(N, 0), wmark(N, -1);
    std::vector<char> elim(N, 0), dead(N, 0);
    typedef std::pair<int, int> DegNode;
    std::priority_queue<DegNode, std::vector<DegNode>, std::greater<DegNode>> heap;      // (degree, node): stale entries are skipped
    for (int v = 0; v < N; v++) { deg[v] = (int)A[v].size(); heap.push(DegNode(deg[v], v)); }
    order.reserve(N);
    std::vector<int> Lp;
    while ((int)order.size() < N) {
        const DegNode top = heap.top(); heap.pop();
        const int p = top.second;
        if (elim[p] || top.first != deg[p]) continue;
        const int k = (int)order.size();
        pos[p] = k; order.push_back(p); elim[p] = 1; mark[p] = k;
        Lp.clear();
        for (int v : A[p]) if (!elim[v] && mark[v] != k) { mark[v] = k; Lp.push_back(v); }
        for (int e : E[p]) {
            if (dead[e]) continue;
            for (int v : Le[e]) if (mark[v] != k) { mark[v] = k; Lp.push_back(v); }      // (a live element has no eliminated member but p)
            dead[e] = 1; parent[e] = p;
            std::vector<int>().swap(Le[e]);
        }
        std::vector<int>().swap(A[p]); std::vector<int>().swap(E[p]);
        std::sort(Lp.begin(), Lp.end());
        count[p] = (int)Lp.size();
        const int left = N - k - 1, lp = (int)Lp.size();
        for (int i : Lp) {      // the lists of the members: absorbed elements out, p in; neighbours that p's element now covers out
            std::vector<int>& Ei = E[i];
            size_t o = 0;
            for (int e : Ei) if (!dead[e]) Ei[o++] = e;
            Ei.resize(o);
            for (int e : Ei) { if (wmark[e] != k) { wmark[e] = k; w[e] = (int)Le[e].size(); } w[e]--; }      // w[e] -> |Le \ Lp|
            Ei.push_back(p);
            std::vector<int>& Ai = A[i];
            o = 0;
            for (int v : Ai) if (!elim[v] && mark[v] != k) Ai[o++] = v;
            Ai.resize(o);
        }
        for (int i : Lp) {
            long long d = (long long)A[i].size() + (lp - 1);
            for (int e : E[i]) if (e != p) d += w[e];
            d = std::min<long long>(d, std::min<long long>(left - 1, (long long)deg[i] + (lp - 1)));
            deg[i] = (int)std::max<long long>(d, 0);
            heap.push(DegNode(deg[i], i));
        }
        Le[p] = Lp;
    }
    // supernodes: a group is named by its last pivot; piv: its pivots in elimination order, kids: its child groups
    std::vector<std::vector<int>> piv(N), kids(N);
    std::vector<int> gpar(parent);
    std::vector<char> gone(N, 0);
    for (int v = 0; v < N; v++) piv[v].assign(1, v);
    for (int k = 0; k < N; k++) { const int v = order[k]; if (parent[v] >= 0) kids[parent[v]].push_back(v); }      // ascending in elimination order
    auto absorb = [&](int f, int c) {      // the pivots of c in front of those of f, the children of c in the place of c
        std::vector<int> pv(piv[c]);
        pv.insert(pv.end(), piv[f].begin(), piv[f].end());
        piv[f].swap(pv); std::vector<int>().swap(piv[c]);
        std::vector<int> kd;
        for (int x : kids[f]) if (x != c) kd.push_back(x);
        for (int x : kids[c]) { kd.push_back(x); gpar[x] = f; }
        std::sort(kd.begin(), kd.end(), [&](int a, int b) { return pos[a] < pos[b]; });
        kids[f].swap(kd); std::vector<int>().swap(kids[c]);
        gone[c] = 1;
    };
    for (int k = 0; k < N; k++) {      // fundamental supernodes
        const int v = order[k];
        if (kids[v].size() == 1 && count[kids[v][0]] == count[v] + 1) absorb(v, kids[v][0]);
    }
    for (int k = 0; k < N && mergeFront > 0; k++) {      // relaxed amalgamation
        const int f = order[k];
        if (gone[f]) continue;
        for (bool again = true; again;) {
            again = false;
            for (int c : kids[f])
                if ((int)piv[c].size() + (int)piv[f].size() + count[f] <= mergeFront) { absorb(f, c); again = true; break; }
        }
    }
    // postorder of the groups
    FrontTree T;
    T.perm.reserve(N);
    std::vector<int> frontOfGroup(N, -1), stack, next(N, 0);
    for (int k = 0; k < N; k++) {
        const int r = order[k];
        if (gone[r] || gpar[r] >= 0) continue;
        stack.assign(1, r);
        while (!stack.empty()) {
            const int g = stack.back();
            if (next[g] < (int)kids[g].size()) { stack.push_back(kids[g][next[g]++]); continue; }
            stack.pop_back();
            const int f = (int)T.np.size();
            frontOfGroup[g] = f;
            T.piv0.push_back((int)T.perm.size()); T.np.push_back((int)piv[g].size()); T.parent.push_back(-1);
            T.perm.insert(T.perm.end(), piv[g].begin(), piv[g].end());
            T.children.push_back(std::vector<int>());
            for (int c : kids[g]) { T.children[f].push_back(frontOfGroup[c]); T.parent[frontOfGroup[c]] = f; }
        }
    }
    return T;
}

// A front tree -> Symbolic: boundaries, rel, assembly lists, the panels' and the update blocks' places, the counts.
// Q given as both triangles (CSC = CSR), E in CSR.
inline Symbolic build_symbolic(int n, int m, const std::vector<std::vector<int>>& adj, const int* Qp, const int* Qi, const int* Ep, const int* Ei, FrontTree&& T)
{
    const int N = n + m;
    Symbolic S;
    S.N = N; S.nF = (int)T.np.size();
    S.perm.swap(T.perm); S.piv0.swap(T.piv0); S.np.swap(T.np); S.parent.swap(T.parent);
    std::vector<std::vector<int>>& frontChildren = T.children;
    S.iperm.assign(N, 0);
    for (int p = 0; p < N; p++) S.iperm[S.perm[p]] = p;
    const int nF = S.nF;
    S.childPtr.assign(nF + 1, 0);
    for (int f = 0; f < nF; f++) S.childPtr[f + 1] = S.childPtr[f] + (int)frontChildren[f].size();
    S.child.reserve(S.childPtr[nF]);
    for (int f = 0; f < nF; f++) for (int c : frontChildren[f]) S.child.push_back(c);
    const std::vector<std::vector<int>> bnd = front_boundaries(S.perm, S.piv0, S.np, frontChildren, adj, S.iperm);
    std::vector<int> frontOf(N);
    for (int f = 0; f < nF; f++) for (int j = 0; j < S.np[f]; j++) frontOf[S.piv0[f] + j] = f;
    S.nb.resize(S.nF); S.rowPtr.assign(S.nF + 1, 0);
    for (int f = 0; f < S.nF; f++) { S.nb[f] = (int)bnd[f].size(); S.rowPtr[f + 1] = S.rowPtr[f] + S.nb[f]; }
    S.rows.reserve(S.rowPtr[S.nF]);
    for (int f = 0; f < S.nF; f++) for (int p : bnd[f]) S.rows.push_back(p);
    // local index of a position in front f
    auto local = [&](int f, int pos) {
        if (pos >= S.piv0[f] && pos < S.piv0[f] + S.np[f]) return pos - S.piv0[f];
        const int* b0 = S.rows.data() + S.rowPtr[f]; const int* b1 = S.rows.data() + S.rowPtr[f + 1];
        const int* it = std::lower_bound(b0, b1, pos);
        return (it != b1 && *it == pos) ? S.np[f] + (int)(it - b0) : -1;
    };
    S.rel.assign(S.rows.size(), -1);
    for (int f = 0; f < S.nF; f++) {
        const int p = S.parent[f];
        if (p < 0) continue;      // (a root has no boundary: nothing comes after the last region)
        for (int a = 0; a < S.nb[f]; a++) S.rel[S.rowPtr[f] + a] = local(p, S.rows[S.rowPtr[f] + a]);
    }
    // assembly lists
    const int nnzQ = Qp[n];
    std::vector<std::vector<int>> aS(S.nF), aG(S.nF), aP(S.nF);
    auto put = [&](int pa, int pb, int src, int gate) {
        const int lo = std::min(pa, pb), hi = std::max(pa, pb), f = frontOf[lo], ff = S.np[f] + S.nb[f];
        const int j = lo - S.piv0[f], i = local(f, hi);
        aS[f].push_back(src); aG[f].push_back(gate); aP[f].push_back(i + ff * j);      // (i >= 0: hi is a later neighbour of a pivot of f)
    };
    for (int i = 0; i < n; i++) for (int k = Qp[i]; k < Qp[i + 1]; k++) { const int pi = S.iperm[i], pj = S.iperm[Qi[k]]; if (pj <= pi) put(pi, pj, k, -1); }     // one of each symmetric pair
    for (int r = 0; r < m; r++) for (int k = Ep[r]; k < Ep[r + 1]; k++) put(S.iperm[n + r], S.iperm[Ei[k]], nnzQ + k, r);
    S.asmPtr.assign(S.nF + 1, 0);
    for (int f = 0; f < S.nF; f++) S.asmPtr[f + 1] = S.asmPtr[f] + (int)aS[f].size();
    for (int f = 0; f < S.nF; f++) { S.asmSrc.insert(S.asmSrc.end(), aS[f].begin(), aS[f].end()); S.asmGate.insert(S.asmGate.end(), aG[f].begin(), aG[f].end()); S.asmPos.insert(S.asmPos.end(), aP[f].begin(), aP[f].end()); }
    // storage: panels one after the other; the stack of update blocks (a front's block takes the place its children's blocks had)
    S.Loff.resize(S.nF); S.CBoff.resize(S.nF);
    long long sp = 0;
    for (int f = 0; f < S.nF; f++) {
        const long long ff = S.np[f] + S.nb[f];
        S.Loff[f] = S.Lsize; S.Lsize += ff * S.np[f];
        S.maxFront = std::max(S.maxFront, (int)ff);
        if (!frontChildren[f].empty()) sp = S.CBoff[frontChildren[f][0]];
        S.CBoff[f] = sp;
        sp += (long long)S.nb[f] * S.nb[f];
        S.stackSize = std::max(S.stackSize, sp);
        for (int j = 0; j < S.np[f]; j++) { const long long r = ff - j - 1; S.flops += r * (r + 3); S.nnzL += r; }
    }
    return S;
}

// What sp_general_factor, sp_general_solve and sp_general_solve_panel (lcqp_sparse_factor.hpp) take for granted of a Symbolic beyond the
// comments of its fields.  They put no limit on the number of fronts, on the children of a front or on the depth of the tree (plain loops
// over gMeta and gChildInfo, no table of fixed size), but:
//   * the update blocks are a STACK: when front f is reached, the blocks on top of the stack are exactly those of its children, lowest
//     first, and f writes its own block where the first of them lay (or on top) after it has read them all -- so the fronts must be in
//     postorder with the fronts of a subtree contiguous, and a front's children ascending;
//   * extend-add writes F[rel[a] + ff * rel[b]] for a >= b into the LOWER triangle of the parent: rel must be present for every boundary
//     row of a front with a parent and strictly ascending; a root has no boundary;
//   * the sweeps read the rows behind a front's pivots from fronts that come later: boundary rows ascending and behind the pivots;
//   * a front takes every entry of K exactly once by assignment, before its children: asmPos inside the ff x np panel, no position twice;
//   * offsets are 32-bit on the device: the panels and the stack below 2^28 doubles, asmPos = i + ff * j below 2^31.
// Empty string: all hold.  Nested dissection meets them by construction; an ordering that feeds build_symbolic is held to them here.
inline std::string symbolic_violation(const Symbolic& S)
{
    auto at = [](const char* what, int f) { return std::string(what) + " (front " + std::to_string(f) + ")"; };
    if ((int)S.perm.size() != S.N || (int)S.iperm.size() != S.N) return "perm has the wrong length";
    { std::vector<char> seen(S.N, 0); for (int v : S.perm) { if (v < 0 || v >= S.N || seen[v]) return "perm is no permutation"; seen[v] = 1; } }
    std::vector<int> stack;
    long long sp = 0, Lsize = 0;
    int nextPiv = 0;
    for (int f = 0; f < S.nF; f++) {
        const int np = S.np[f], nb = S.nb[f], ff = np + nb, nch = S.childPtr[f + 1] - S.childPtr[f];
        if (np < 1 || S.piv0[f] != nextPiv) return at("the pivots of the fronts are not consecutive", f);
        nextPiv += np;
        if (S.parent[f] >= 0 ? S.parent[f] <= f || S.parent[f] >= S.nF : nb != 0) return at("a parent in front of its child, or a root with a boundary", f);
        if (S.rowPtr[f + 1] - S.rowPtr[f] != nb) return at("rowPtr", f);
        for (int a = 0; a < nb; a++) {
            const int r = S.rows[S.rowPtr[f] + a], rl = S.rel[S.rowPtr[f] + a], p = S.parent[f];
            if (r < S.piv0[f] + np || r >= S.N || (a && r <= S.rows[S.rowPtr[f] + a - 1])) return at("boundary rows not ascending behind the pivots", f);
            if (rl < 0 || rl >= S.np[p] + S.nb[p] || (a && rl <= S.rel[S.rowPtr[f] + a - 1])) return at("rel not ascending inside the parent's front", f);
            if ((rl < S.np[p] ? S.piv0[p] + rl : S.rows[S.rowPtr[p] + rl - S.np[p]]) != r) return at("rel names another row of the parent", f);
        }
        // the stack: the children are its top, lowest first
        if ((int)stack.size() < nch) return at("children missing from the stack", f);
        for (int k = 0; k < nch; k++) {
            const int c = S.child[S.childPtr[f] + k];
            if (stack[stack.size() - nch + k] != c || S.parent[c] != f) return at("the top of the stack is not the children, lowest first", f);
        }
        for (int k = 0; k < nch; k++) { const int c = stack.back(); stack.pop_back(); sp -= (long long)S.nb[c] * S.nb[c]; }
        if (S.CBoff[f] != sp) return at("update block not on top of the stack", f);
        sp += (long long)nb * nb;
        if (sp > S.stackSize) return at("stack overflow", f);
        stack.push_back(f);
        if (S.Loff[f] != Lsize) return at("Loff", f);
        Lsize += (long long)ff * np;
        if ((long long)ff * ff >= (1LL << 31)) return at("front too large for 32-bit positions", f);
        std::vector<int> posn(S.asmPos.begin() + S.asmPtr[f], S.asmPos.begin() + S.asmPtr[f + 1]);
        std::sort(posn.begin(), posn.end());
        for (size_t e = 0; e < posn.size(); e++)
            if (posn[e] < 0 || posn[e] >= ff * np || posn[e] % ff < posn[e] / ff || (e && posn[e] == posn[e - 1])) return at("assembly position outside the panel's lower part, or taken twice", f);
    }
    if (nextPiv != S.N) return "the fronts do not cover every position";
    for (int f : stack) if (S.parent[f] >= 0) return at("a block left on the stack", f);
    if (Lsize != S.Lsize) return "Lsize";
    return std::string();
}

// adj: adjacency lists of the KKT graph on N = n + m nodes (sorted, no self loops).  Q given as both triangles (CSC = CSR), E in CSR.
// leaf, mergeFront: nd_front_tree
inline Symbolic analyze(int n, int m, const std::vector<std::vector<int>>& adj, const int* Qp, const int* Qi, const int* Ep, const int* Ei, int leaf = 32, int mergeFront = 64)
{
    return build_symbolic(n, m, adj, Qp, Qi, Ep, Ei, nd_front_tree(n + m, adj, leaf, mergeFront));
}

// the same through the minimum-degree ordering
inline Symbolic analyze_md(int n, int m, const std::vector<std::vector<int>>& adj, const int* Qp, const int* Qi, const int* Ep, const int* Ei, int mergeFront = 64)
{
    return build_symbolic(n, m, adj, Qp, Qi, Ep, Ei, md_front_tree(n + m, adj, mergeFront));
}

}  // namespace lcqp_general
