// lcqp_sparse_factor.hpp -- the factorisations of an instance's KKT matrix and the solves with them, second layer of the sparse kernel unit
// (lcqp_sparse.hip has the map).
//
// Owns: the assembly of the band array (sp_assemble), the three engines -- the band with its rows in registers (sp_factor_reg, G <= 16), the
// band with a sliding window in LDS (sp_factor_lds), the general multifrontal LDL' (sp_general_*, G = 64; symbolic side:
// lcqp_sparse_general.hpp) --, the band sweeps and their folded layouts (band_sweep, sp_solve_band), the border (sp_border_*), and the two
// entry points the solver layer calls: sp_factor_band and sp_solve.  Nothing here knows what the matrix is for: the regularisations and the
// working set arrive as arguments (dprim, ddual, use).
// May include: lcqp_sparse_lane.hpp, and lcqp_sparse_pattern.hpp for GEN_MAX_FRONT.  Device code only, in the anonymous namespace.
#pragma once
#include "lcqp_sparse_lane.hpp"
#include "lcqp_sparse_pattern.hpp"      // GEN_MAX_FRONT

#include <climits>

namespace {

// ---- KKT assembly into band storage: Kb[i*ld + k] = K[i][i-w+k] in the ordering iperm ----------------------------------------
// variables: Q + dprim I; row r: -(use ? ddual(r) : 1) on the diagonal, its entries of E only when used
template <int G, class Dd, class Use>
__device__ __forceinline__ void sp_assemble(SpCtx<G>& c, double dprim, Dd ddual, Use use)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, ld = db.ld, w = db.ld - 1, n = db.n, m = db.m;
    GD Kb = c.Kb();
    SPROF(c, SP_VECTORS);
    for (int e = t; e < db.N * ld; e += G) Kb[e] = 0.0;
    g_sync();
    for (int k = t; k < db.nnzQ; k += G) { const int o = db.bandQ[k]; if (o >= 0) Kb[o] = c.Qx()[k]; }
    for (int r = t; r < m; r += G) {
        const bool on = use(r);
        if (on) for (int k = db.Ep[r]; k < db.Ep[r + 1]; k++) { const int o = db.bandE[k]; if (o >= 0) Kb[o] = c.Ex()[k]; }      // (-1: an entry of the border)
        Kb[(size_t)db.iperm[n + r] * ld + w] = on ? -ddual(r) : -1.0;
    }
    g_sync();
    for (int i = t; i < n; i += G) Kb[(size_t)db.iperm[i] * ld + w] += dprim;
    g_sync();
    for (int b = t; b < db.kb; b += G) Kb[(size_t)(db.N - db.kb + b) * ld + w] = 1.0;      // border positions: isolated unit pivots of the band
    g_sync();
    c.bytes += db.by[BY_ASSEMBLE];
    SPROF(c, SP_ASSEMBLE);
}

// ---- band LDL' with a sliding G x G window in LDS ---------------------------------------------------------------------------------
// The elimination is a chain of N column steps with O(w^2) work each, run by the G lanes of the instance without barriers; the rows
// that enter the window are fetched 16 columns ahead.  Window slot of K[r][c]: win[(r % G) * G + (c % G)].
// in: Kb assembled band rows; out: the unit lower factor L in the folded layout the sweeps stream (band_sweep), Kd = 1/D:
//     KF[((j / G) * G + r % G) * G + j % G] = L[r][j]          (forward: columns finish in ascending order)
template <int G>
__device__ __forceinline__ void sp_factor_lds(SpCtx<G>& c, GD KF, GD Kd)
{
    constexpr int GM = G - 1;
    const int N = c.db->N, Np = c.db->Np, w = G - 1, ld = G, l = c.gl;
    GD Kb = c.Kb();
    double* win = c.win;                  // G * G
    double* stage = win + G * G;          // 16 rows x G
    for (int r = 0; r <= w && r < N; r++) {
        const int cc = r - w + l;
        if (l <= w && cc >= 0) win[(r & GM) * G + (cc & GM)] = Kb[(size_t)r * ld + l];
    }
    double pre[16];                        // rows j0 + w + 1 .. j0 + w + 16 of the NEXT block of columns, one band entry per lane and row
#pragma unroll
    for (int q = 0; q < 16; q++) { const int rn = w + 1 + q; pre[q] = (l <= w && rn < N) ? Kb[(size_t)rn * ld + l] : 0.0; }
    for (int j0 = 0; j0 < N; j0 += 16) {
#pragma unroll
        for (int q = 0; q < 16; q++) stage[q * G + l] = pre[q];
#pragma unroll
        for (int q = 0; q < 16; q++) { const int rn = j0 + 16 + w + 1 + q; pre[q] = (l <= w && rn < N) ? Kb[(size_t)rn * ld + l] : 0.0; }
        wave_sync();
        const int j1 = min(N, j0 + 16);
        for (int j = j0; j < j1; j++) {
            const int jm = j & GM, r = j + l + 1;
            const double d = win[jm * G + jm];
            const bool mine = (l < w) && (r < N);
            double la = 0.0;
            if (mine) {
                la = win[(r & GM) * G + jm] / d;
                KF[((size_t)(j & ~GM) + (r & GM)) * G + jm] = la;
            }
            if (l == 0) Kd[j] = 1.0 / d;
            const double lad = la * d;
#pragma unroll
            for (int bb = 1; bb < G; bb++) {
                const double lb = g_bcast<G>(la, bb - 1);          // L[j + bb][j]
                if (mine && bb <= l + 1) win[(r & GM) * G + ((j + bb) & GM)] -= lad * lb;
            }
            wave_sync();
            const int rn = j + w + 1;
            if (l <= w && rn < N) win[(rn & GM) * G + ((j + 1 + l) & GM)] = stage[(j - j0) * G + l];
            wave_sync();
        }
    }
    c.bytes += c.db->by[BY_FACTOR_LDS];
    c.cFact++;
    SPROF(c, SP_FACTOR);
}

// ---- band LDL' with the rows in registers and the pivot row through LDS (G <= 16) ---------------------------------------------------
// Round 5.  Lane l of the group holds ONE row r (r % G == l) of the part of the band that is still to be eliminated, in UPPER form
// relative to its own diagonal: wr[k] = K[r][r + k], k = 0 .. G-1 (by symmetry the entries of column r below the diagonal).  At step j
// the lane of row j puts its row into the group's LDS buffer; every other lane -- row i = j + a, a = 1 .. G-1 -- reads the part of the
// pivot row that reaches its own columns, p[k] = K[j][i + k] = buf[a + k] (one LDS read per entry at a lane-dependent address; behind the
// G entries of the buffer lie G zeros, so what is outside the band needs no predicate), forms its multiplier L[i][j] = p[0] / d_j as
// p[0] * (1 / d_j) and subtracts L[i][j] * p[k] from its row.  The lane whose row is finished takes over row j + G (gathered three
// blocks ahead from the instance's assembled rows).  Per step: 4 LDS writes, G + 1 LDS reads, one division, G fused multiply-adds.
// (Round 4 kept row r in LOWER form with the entry of column c in register slot c % G, so that every access had a static index, and
// moved the pivot and the G-1 multipliers of a step through the lane group by DPP: six moves and selects per double, two divisions,
// about a hundred instructions and 780 clocks per step for G = 8 -- the factorisation was the longest chain of an instance,
// profiles/round5/sparse_sched_profile_small_batches.log.)  The oracle's band_factor does the same arithmetic in the same order.
// Rows >= N are identity rows.  What depends on the working set is applied while a row is loaded: bgate (shared by the batch) names the
// row of E whose membership gates an entry (-1: none), bdiag what the diagonal is (>= -1 a variable: Q_ii, in K0, + dprim; -2 - rr the
// constraint row rr; INT_MIN a border position).  K0 / bgate are in the same upper form: entry k of row r is K[r + k][r].
__shared__ double sp_piv_lds[2 * WGS];      // per lane group: the pivot row (G doubles) and G zeros behind it
template <int G, class Dd, class Use>
__device__ __forceinline__ void sp_factor_reg(SpCtx<G>& c, GD KF, GD Kd, double dprim, Dd ddual, Use use)
{
    constexpr int GM = G - 1;
    const int N = c.db->N, Np = c.db->Np, l = here(c.gl);
    GD K0 = c.K0();
    const int NG = (N + GM) & ~GM;
    const int* __restrict__ bgate = c.db->bgate;
    const int* __restrict__ bdiag = c.db->bdiag;
    double* buf = sp_piv_lds + (size_t)(here((int)threadIdx.x) / G) * (2 * G);
    // A row is fetched in two halves: row_issue starts the loads (the instance's assembled row, the gates and the diagonal code: 9 x 16
    // bytes) and row_finish, one block of G steps later, applies what depends on the working set.  (Until round 5 both sat at the top of a
    // block: the gating consumed the loads it had just issued, one memory round trip per block of G steps -- most of a factorisation's
    // time.)
    struct RawRow { double val[G]; int gate[G]; int bd; };
    auto row_issue = [&](RawRow& rw, int r) {
        const int rr = (r < N) ? r : 0;      // (rows >= N are identity rows: the loads are harmless, row_finish ignores them)
#pragma unroll
        for (int k = 0; k < G; k += 4) { const int4 g4 = *reinterpret_cast<const int4*>(bgate + (size_t)rr * G + k); rw.gate[k] = g4.x; rw.gate[k + 1] = g4.y; rw.gate[k + 2] = g4.z; rw.gate[k + 3] = g4.w; }
        rw.bd = bdiag[rr];
#pragma unroll
        for (int k = 0; k < G; k += 2) { const dv2 v = K0.ld2(rr * G + k); rw.val[k] = v.x; rw.val[k + 1] = v.y; }
    };
    auto row_finish = [&](double* dst, const RawRow& rw, int r) {
        if (r < N) {
#pragma unroll
            for (int k = 1; k < G; k++) dst[k] = (rw.gate[k] < 0 || use(rw.gate[k])) ? rw.val[k] : 0.0;
            const int bd = rw.bd;
            if (bd == INT_MIN) dst[0] = 1.0;                           // a border position: an isolated unit pivot of the band
            else if (bd >= -1) dst[0] = rw.val[0] + dprim;
            else { const int rr = -2 - bd; dst[0] = use(rr) ? -ddual(rr) : -1.0; }
        } else {
#pragma unroll
            for (int k = 0; k < G; k++) dst[k] = (k == 0) ? 1.0 : 0.0;
        }
    };
    // G = 8: the lane's row of the next block is held gated (nx) and the rows of the two blocks behind it are in flight (ra, rb): a row is
    // requested FOUR blocks before it is the pivot row's neighbour and gated two blocks after the request -- under load a round trip to
    // memory is longer than the ~2.3 us a block of eight steps takes, and with one block between request and use the chain waited for it at every
    // block (the factorisation steps of a full machine took 1.7 x the time of a lone instance).  The block loop is unrolled by two so that
    // each buffer is named statically (a copy from one to the other would wait for the load).  G = 16 has registers for one gated row
    // ahead and one in flight only (DEEP: with a second one in flight scratch).
    constexpr bool DEEP = (G == 8);
    double wr[G], nx[G], kf[DEEP ? G : 1];
    RawRow ra, rb;
    row_issue(ra, l); row_finish(wr, ra, l);
    row_issue(ra, G + l); row_finish(nx, ra, G + l);
    row_issue(ra, 2 * G + l);
    if (DEEP) row_issue(rb, 3 * G + l);
    buf[G + l] = 0.0;                                // the zeros behind the pivot row
    double rinv = 1.0;
    auto block = [&](int j0, RawRow& raw) {
#pragma unroll
        for (int u = 0; u < G; u++) {
            const int ag = (l - u) & GM;                               // this lane holds row j + ag, j = j0 + u (ag == 0: the pivot row)
            if (ag == 0) {
#pragma unroll
                for (int k = 0; k < G; k += 2) { dv2 v; v.x = wr[k]; v.y = wr[k + 1]; *reinterpret_cast<dv2*>(buf + k) = v; }
            }
            asm volatile("" ::: "memory");      // (LDS traffic of one wavefront is in order: the reads below see the pivot lane's stores)
            const double ri = 1.0 / buf[0];
            double p[G];
#pragma unroll
            for (int k = 0; k < G; k++) p[k] = buf[ag + k];              // K[j][j + ag + k]: zero beyond the band (the padding)
            asm volatile("" ::: "memory");
            const double la = (ag != 0) ? p[0] * ri : 0.0;                // L[j + ag][j]
            if (DEEP) kf[u] = la;
            else KF[(j0 + l) * G + u] = la;                                 // (G = 16: no registers for a block of the factor; one 8-byte store per step)
            if (ag == 0) {                                               // row j is finished: row j + G enters this lane
                rinv = ri;
#pragma unroll
                for (int k = 0; k < G; k++) wr[k] = nx[k];
            } else {
#pragma unroll
                for (int k = 0; k < G; k++) wr[k] -= la * p[k];
            }
        }
        // forward layout: row (j0 + l) of the block holds L[.][j0 + u] in column u (zero on and above this lane's own step)
        if (DEEP) {
#pragma unroll
            for (int k = 0; k < G; k += 2) { dv2 v; v.x = kf[k]; v.y = kf[k + 1]; *reinterpret_cast<dv2*>(reinterpret_cast<char*>(KF.base) + (size_t)(KF.off + (unsigned)((j0 + l) * G + k) * 8u)) = v; }
        }
        if (j0 + l < Np) Kd[j0 + l] = rinv;
        row_finish(nx, raw, j0 + 2 * G + l);          // requested two blocks ago (G = 16: one)
        row_issue(raw, j0 + (DEEP ? 4 : 3) * G + l);
    };
    if (DEEP) {
        for (int j0 = 0; j0 < NG; j0 += 2 * G) {
            block(j0, ra);
            if (j0 + G < NG) block(j0 + G, rb);
        }
    } else {
        for (int j0 = 0; j0 < NG; j0 += G) block(j0, ra);
    }
    c.bytes += c.db->by[BY_FACTOR];      // matrix entries read, factor and 1/D written
    c.cFact++;
    SPROF(c, SP_FACTOR);
}
// the band part of the KKT matrix [Q + dprim I, E_use'; E_use, -diag(ddual)] factorised: assembled on the fly (G <= 16) or through the band array
// ---- general sparse LDL' (round 6): multifrontal over the dissection tree, one wavefront per instance ------------------------------------
// Symbolic side: lcqp_sparse_general.hpp (fronts in postorder: pivots = a leaf region or a separator, update rows = the boundary of the
// region the front closes; assembly lists; positions of a child's update rows in its parent's front; storage offsets).  CPU restatement of
// the loops below, checked against a dense solve: tests/cpp/general_ldl_test.cpp.  The reference's OSQP arm factorises the same matrix
// with QDLDL whatever the pattern (src/SubsolverOSQP.cpp:136-152).
// A front F (ff x ff, column-major, lower triangle used) lives in LDS when ff <= 64, else in the instance's front buffer; its pivots go
// in blocks of GEN_JB: the block's columns (the panel, rows below included) are staged in LDS, eliminated there, stored scaled into the
// factor's panel storage, and applied to the rest of the front as ONE rank-GEN_JB update -- GEN_JB fused multiply-adds per entry read and
// written.  No pivoting: K is quasi-definite for delta, delta2 > 0, and every symmetric permutation of a quasi-definite matrix factorises.
constexpr int GEN_JB = 8;
constexpr int GEN_LDS_FRONT = 64;        // fronts up to this size are factorised inside LDS
using lcqp_pattern::GEN_MAX_FRONT;       // the panel of the largest front (lcqp_sparse_pattern.hpp refuses larger ones)

constexpr int GEN_BITS_OFF = GEN_MAX_FRONT * GEN_JB + 16;        // doubles: the working set as a bit set behind the panel and 1 / D of a block
constexpr int GEN_BITS_WORDS = (GEN_LDS_FRONT * GEN_LDS_FRONT + 16 * 64 - GEN_BITS_OFF) * 2;      // 32-bit words that fit the rest of the window

// `in(r)`: is row r of E in the working set -- a bit in LDS (sp_general_factor builds the set once per factorisation: the gate of an entry and
// the diagonal of a row node are then no round trip to memory)
template <bool LDSF, class FA, class Dd, class In>
__device__ __forceinline__ void sp_general_front(SpCtx<64>& c, int f, FA F, double* P, GD Lst, GD Kd, GD stack, double dprim, Dd ddual, In in)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl), n = db.n, nnzQ = db.nnzQ;
    // everything the front needs to know about itself in ONE load (the dependent chain of a front is what a factorisation costs: about
    // 33 us per front with a load per field, sixteen round trips; profiles/round6/general_ldl_timing.log)
    const int* mt = db.gMeta + (size_t)f * GEN_META;
    const int np = mt[0], nb = mt[1], piv0 = mt[2], asm0 = mt[4], asm1 = mt[5], ch0 = mt[6], ch1 = mt[7];
    const unsigned Loff = (unsigned)mt[8], CBoff = (unsigned)mt[9];
    const int ff = np + nb;
    auto sync = [&]() { if (LDSF) wave_sync(); else g_sync(); };
    for (int e = t; e < ff * ff; e += 64) F[e] = 0.0;
    sync();
    {   // the entries of K whose column is a pivot of this front (one entry of Q or E each: distinct positions); rows of E gated by value
        GD Qv = c.Qx(), Ev = c.Ex();
        for (int e = asm0 + t; e < asm1; e += 64) {
            const int src = db.gAsmSrc[e], gate = db.gAsmGate[e], pos = db.gAsmPos[e];
            const double v = (src >= nnzQ ? (double)Ev[src - nnzQ] : (double)Qv[src]);
            F[pos] = (gate >= 0 && !in(gate)) ? 0.0 : v;
        }
    }
    sync();
    for (int j = t; j < np; j += 64) {      // diagonals: Q_ii + dprim; -ddual for an active row, -1 for a decoupled one
        const int node = db.pnode[piv0 + j];
        if (node < n) F[j + ff * j] += dprim;
        else F[j + ff * j] = in(node - n) ? -ddual(node - n) : -1.0;
    }
    sync();
    for (int ci = ch0; ci < ch1; ci++) {      // extend-add: the children's update blocks, one child after the other
        const int* cm = db.gChildInfo + (size_t)ci * 4;
        const int nbc = cm[0];
        GD CB = stack + cm[1];
        const int* rel = db.gRel + cm[2];
        for (int e = t; e < nbc * nbc; e += 64) {
            const int b = e / nbc, a = e - b * nbc;
            if (a >= b) F[rel[a] + ff * rel[b]] += (double)CB[a + nbc * b];
        }
        sync();
    }
    double* dv = c.win + GEN_MAX_FRONT * GEN_JB;      // 1 / D of the block's pivots (behind the largest panel either variant uses)
    GD Lp = Lst + (int)Loff;
    for (int j0 = 0; j0 < np; j0 += GEN_JB) {
        const int jb = min(GEN_JB, np - j0), h = ff - j0;
        if (h <= 256) {
            // The panel of the block in REGISTERS: lane t holds rows t, t + 64, t + 128, t + 192 of the panel, eight entries each.  The eight
            // pivots are eliminated with v_readlane broadcasts (the pivot rows are rows 0 .. 7: lanes 0 .. 7 of the first register set) --
            // a division and at most seven broadcast + fused multiply-add steps per pivot, ~100 clocks, where the version through LDS below paid a
            // dependent LDS round trip per step (~2000 clocks per pivot with one wavefront per SIMD: 23 % + 16 % of a factorisation's time).
            // Same operations on the same values: li = p[cc] / d, p[c2] -= li * P[c2][cc]; rows above the diagonal compute entries nobody reads.
            constexpr int QP = 4;
            double p[QP][GEN_JB];
#pragma unroll
            for (int q = 0; q < QP; q++)
#pragma unroll
                for (int cc = 0; cc < GEN_JB; cc++) { const int i = t + 64 * q; p[q][cc] = (i < h && cc < jb) ? (double)F[(j0 + i) + ff * (j0 + cc)] : 0.0; }
            double dvr[GEN_JB];
#pragma unroll
            for (int cc = 0; cc < GEN_JB; cc++) {
                dvr[cc] = 0.0;
                if (cc < jb) {
                    const double dinv = 1.0 / wave_bcast(p[0][cc], cc);
                    dvr[cc] = dinv;
                    if (t == 0) { dv[cc] = dinv; Kd[piv0 + j0 + cc] = dinv; }
#pragma unroll
                    for (int c2 = cc + 1; c2 < GEN_JB; c2++) {
                        if (c2 < jb) {
                            const double pc = wave_bcast(p[0][cc], c2);      // P[c2][cc], unscaled
#pragma unroll
                            for (int q = 0; q < QP; q++) p[q][c2] -= (p[q][cc] * dinv) * pc;
                        }
                    }
                }
            }
            // the scaled columns are the factor's panel; the unscaled ones go to LDS for the tiles below
#pragma unroll
            for (int q = 0; q < QP; q++) {
                const int i = t + 64 * q;
                if (i < h) {
#pragma unroll
                    for (int cc = 0; cc < GEN_JB; cc++) {
                        P[i * GEN_JB + cc] = p[q][cc];
                        if (cc < jb && i > cc) Lp[(j0 + i) + ff * (j0 + cc)] = p[q][cc] * dvr[cc];
                    }
                }
            }
            wave_sync();
        } else {
            // the panel of the block: rows j0 .. ff-1, columns j0 .. j0+jb-1 -> P[(i - j0) * JB + c]
            for (int e = t; e < h * GEN_JB; e += 64) { const int cc = e / h, i = e - cc * h; P[i * GEN_JB + cc] = (cc < jb) ? (double)F[(j0 + i) + ff * (j0 + cc)] : 0.0; }
            wave_sync();
            for (int cc = 0; cc < jb; cc++) {      // eliminate inside the panel (columns unscaled: column c holds l_ic d_c)
                const double dinv = 1.0 / P[cc * GEN_JB + cc];
                if (t == 0) { dv[cc] = dinv; Kd[piv0 + j0 + cc] = dinv; }
                for (int i = cc + 1 + t; i < h; i += 64) {
                    const double li = P[i * GEN_JB + cc] * dinv;
                    for (int c2 = cc + 1; c2 < jb; c2++) if (c2 <= i) P[i * GEN_JB + c2] -= li * P[c2 * GEN_JB + cc];
                }
                wave_sync();
            }
            // the scaled columns are the factor's panel (column-major, ld = ff)
            for (int e = t; e < h * jb; e += 64) { const int cc = e / h, i = e - cc * h; if (i > cc) Lp[(j0 + i) + ff * (j0 + cc)] = P[i * GEN_JB + cc] * dv[cc]; }
        }
        // rank-jb update of what lies behind the block, on the fp64 matrix cores: 16 x 16 tiles over the lower triangle of F[k0.., k0..],
        // each D = A B with A[i][c] = (l_ic d_c) / d_c ... = P[i][c] dv[c] and B[c][k] = P[k][c] (v_mfma_f64_16x16x4_f64, two per tile: c = 0..3, 4..7).
        // Operand lane map: A[i = lane & 15][c = lane >> 4], B[c = lane >> 4][k = lane & 15]; result register r of a lane: row (lane >> 4) + 4 r,
        // column lane & 15 (cdna_hip_programming.md).  A row or column outside the front feeds only results that are not written.
        // (The VALU version -- a lane per row, eight fused multiply-adds behind four 16-byte LDS reads per entry, half the lanes idle in a
        // triangle -- was 41 % of a factorisation: profiles/round6/README.md.)
        const int k0 = j0 + jb;
        {
            const int lr = t >> 4, lc = t & 15;
            const double dva = (lr < jb) ? dv[lr] : 0.0, dvb = (lr + 4 < jb) ? dv[lr + 4] : 0.0;
            const int nt = (ff - k0 + 15) >> 4;
            for (int ti = 0; ti < nt; ti++) {
                const int ia = k0 + 16 * ti + lc;
                const double a0 = (ia < ff && lr < jb) ? P[(ia - j0) * GEN_JB + lr] * dva : 0.0;
                const double a1 = (ia < ff && lr + 4 < jb) ? P[(ia - j0) * GEN_JB + lr + 4] * dvb : 0.0;
                for (int tk = 0; tk <= ti; tk++) {
                    const int kb = k0 + 16 * tk + lc;
                    const double b0 = (kb < ff && lr < jb) ? P[(kb - j0) * GEN_JB + lr] : 0.0;
                    const double b1 = (kb < ff && lr + 4 < jb) ? P[(kb - j0) * GEN_JB + lr + 4] : 0.0;
                    d4_t acc = {0.0, 0.0, 0.0, 0.0};
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
                    double fv[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) { const int i = k0 + 16 * ti + lr + 4 * r; fv[r] = (i < ff && kb < ff && i >= kb) ? (double)F[i + ff * kb] : 0.0; }
#pragma unroll
                    for (int r = 0; r < 4; r++) { const int i = k0 + 16 * ti + lr + 4 * r; if (i < ff && kb < ff && i >= kb) F[i + ff * kb] = fv[r] - acc[r]; }
                }
            }
        }
        sync();
    }
    {   // the update block goes onto the stack (its place was fixed by the host: where its children's blocks lay)
        GD CB = stack + (int)CBoff;
        for (int e = t; e < nb * nb; e += 64) { const int b = e / nb, a = e - b * nb; if (a >= b) CB[a + nb * b] = (double)F[(np + a) + ff * (np + b)]; }
    }
    g_sync();
}

template <class Dd, class Use>
__device__ __forceinline__ void sp_general_factor(SpCtx<64>& c, GD Lst, GD Kd, double dprim, Dd ddual, Use use)
{
    const SpBatch& db = *c.db;
    double* Fl = c.win;                                       // 64 x 64 front in LDS
    double* P = c.win + GEN_LDS_FRONT * GEN_LDS_FRONT;        // panel of a front in LDS (64 x 8) ...
    GD stack = c.GStack(), Fg = c.GFront();
    SPROF(c, SP_VECTORS);
    // the working set as a bit set in LDS (behind everything a front uses of the window)
    unsigned* bits = reinterpret_cast<unsigned*>(c.win + GEN_BITS_OFF);
    const int m = db.m, words = (m + 31) >> 5;
    const bool haveBits = words <= GEN_BITS_WORDS;
    if (haveBits) {
        for (int w = c.gl; w < words; w += 64) {
            unsigned word = 0u;
#pragma unroll 8
            for (int k = 0; k < 32; k++) { const int r = w * 32 + k; if (r < m && use(r)) word |= 1u << k; }
            bits[w] = word;
        }
        wave_sync();
    }
    for (int f = 0; f < db.gnF; f++) {
        const int* mt = db.gMeta + (size_t)f * GEN_META;
        const int ff = mt[0] + mt[1];
        if (haveBits) {
            auto in = [=](int r) { return ((bits[r >> 5] >> (r & 31)) & 1u) != 0u; };
            if (ff <= GEN_LDS_FRONT) sp_general_front<true>(c, f, Fl, P, Lst, Kd, stack, dprim, ddual, in);
            else sp_general_front<false>(c, f, Fg, c.win, Lst, Kd, stack, dprim, ddual, in);      // ... or of a front in memory (up to GEN_MAX_FRONT x 8: the whole window)
        } else {
            if (ff <= GEN_LDS_FRONT) sp_general_front<true>(c, f, Fl, P, Lst, Kd, stack, dprim, ddual, use);
            else sp_general_front<false>(c, f, Fg, c.win, Lst, Kd, stack, dprim, ddual, use);
        }
    }
    c.bytes += db.by[BY_FACTOR];
    SPROF(c, SP_FACTOR);
}

// K z = b in place (b in the ordering of the fronts): forward over the fronts in postorder, 1 / D, backward in reverse.  Per front the
// right-hand side's entries (pivots and update rows) are gathered into LDS, the panel is staged in LDS in chunks of columns (all lanes load,
// many loads in flight) and the columns are applied one after the other: an axpy per column forward, a dot product per column backward.
template <bool FWD>
__device__ __forceinline__ void sp_general_sweep(SpCtx<64>& c, GD Lst, GD b)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl);
    double* bl = c.win;                         // ff entries
    double* Pc = c.win + GEN_MAX_FRONT;         // a chunk of columns: (ff) x cw, column-major
    constexpr int CHUNK = GEN_LDS_FRONT * GEN_LDS_FRONT + 16 * 64 - GEN_MAX_FRONT;      // doubles left in the window
    for (int q = 0; q < db.gnF; q++) {
        const int f = FWD ? q : db.gnF - 1 - q;
        const int* mt = db.gMeta + (size_t)f * GEN_META;
        const int np = mt[0], nb = mt[1], ff = np + nb, piv0 = mt[2];
        const int* rows = db.gRows + mt[3];
        GD Lp = Lst + mt[8];
        if (ff <= 64) {
            // A front of at most 64 rows (every leaf, every merged separator: most of the pivots): lane t IS row t.  The right-hand side lives in
            // one register per lane, a pivot's value travels by v_readlane, the panel's column (forward) or row (backward) comes from LDS with an
            // address that does not depend on the chain -- a pivot step is a broadcast and a fused multiply-add, ~30 clocks, where the version
            // through LDS (below, kept for larger fronts) paid a read - modify - write round trip of the right-hand side per pivot, ~1000 clocks
            // with one wavefront per SIMD.  Backward in axpy form too (a finished x_i leaves every earlier row), so no reduction sits in the chain.
            wave_sync();
            // forward: lane t reads ITS entry of column j straight from the factor (coalesced; the addresses do not depend on the chain, so the
            // loads of all columns are in flight together) -- no staging in LDS
            double x = (t < ff) ? (double)b[t < np ? piv0 + t : rows[t - np]] : 0.0;
            wave_sync();
            if (FWD) {
                for (int j0 = 0; j0 < np; j0 += 8) {
                    double lv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) { const int j = j0 + u; lv[u] = (j < np && t > j && t < ff) ? (double)Lp[t + ff * j] : 0.0; }
#pragma unroll
                    for (int u = 0; u < 8; u++) { const int j = j0 + u; if (j < np) { const double yj = wave_bcast(x, j); x -= lv[u] * yj; } }
                }
                if (t < ff) b[t < np ? piv0 + t : rows[t - np]] = x;
            } else {
                // backward: lane t (a pivot) walks down ITS column of the panel, L[i][t] for i = ff-1 .. t+1 -- contiguous per lane (a cache line serves
                // eight steps), a stride of ff between the lanes; again no address depends on the chain, eight loads in flight
                for (int i0 = ff - 1; i0 >= 1; i0 -= 8) {
                    double lv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) { const int i = i0 - u; lv[u] = (i >= 1 && t < i && t < np) ? (double)Lp[i + ff * t] : 0.0; }
#pragma unroll
                    for (int u = 0; u < 8; u++) { const int i = i0 - u; if (i >= 1) { const double xi = wave_bcast(x, i); x -= lv[u] * xi; } }
                }
                if (t < np) b[piv0 + t] = x;
            }
            g_sync();
            continue;
        }
        if (ff <= 256) {
            // the same for a front of up to 256 rows: lane t holds rows t, t + 64, t + 128, t + 192 in four registers
            constexpr int QR = 4;
            double x[QR];
#pragma unroll
            for (int q = 0; q < QR; q++) { const int i = t + 64 * q; x[q] = (i < ff) ? (double)b[i < np ? piv0 + i : rows[i - np]] : 0.0; }
            auto bc = [&](int i) {      // value of row i: a broadcast from the register of lane i & 63 that holds chunk i >> 6 (uniform selection)
                const int qi = i >> 6, li = i & 63;
                double v = wave_bcast(x[0], li);
                if (qi == 1) v = wave_bcast(x[1], li);
                if (qi == 2) v = wave_bcast(x[2], li);
                if (qi == 3) v = wave_bcast(x[3], li);
                return v;
            };
            if (FWD) {
                for (int j0 = 0; j0 < np; j0 += 4) {
                    double lv[4][QR];
#pragma unroll
                    for (int u = 0; u < 4; u++)
#pragma unroll
                        for (int q = 0; q < QR; q++) { const int j = j0 + u, i = t + 64 * q; lv[u][q] = (j < np && i > j && i < ff) ? (double)Lp[i + ff * j] : 0.0; }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int j = j0 + u;
                        if (j < np) {
                            const double yj = bc(j);
#pragma unroll
                            for (int q = 0; q < QR; q++) x[q] -= lv[u][q] * yj;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < QR; q++) { const int i = t + 64 * q; if (i < ff) b[i < np ? piv0 + i : rows[i - np]] = x[q]; }
            } else {
                for (int i0 = ff - 1; i0 >= 1; i0 -= 4) {
                    double lv[4][QR];
#pragma unroll
                    for (int u = 0; u < 4; u++)
#pragma unroll
                        for (int q = 0; q < QR; q++) { const int i = i0 - u, j = t + 64 * q; lv[u][q] = (i >= 1 && j < i && j < np) ? (double)Lp[i + ff * j] : 0.0; }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int i = i0 - u;
                        if (i >= 1) {
                            const double xi = bc(i);
#pragma unroll
                            for (int q = 0; q < QR; q++) x[q] -= lv[u][q] * xi;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < QR; q++) { const int j = t + 64 * q; if (j < np) b[piv0 + j] = x[q]; }
            }
            g_sync();
            continue;
        }
        for (int i = t; i < ff; i += 64) bl[i] = (double)b[i < np ? piv0 + i : rows[i - np]];
        const int cw = max(1, min(np, CHUNK / ff));
        for (int c0 = FWD ? 0 : ((np - 1) / cw) * cw; FWD ? c0 < np : c0 >= 0; c0 += FWD ? cw : -cw) {
            const int c1 = min(np, c0 + cw), h = ff - c0;      // rows c0 .. ff-1 of the columns c0 .. c1-1
            wave_sync();
            for (int e = t; e < h * (c1 - c0); e += 64) { const int cc = e / h, i = e - cc * h; Pc[i + h * cc] = (i > cc) ? (double)Lp[(c0 + i) + ff * (c0 + cc)] : 0.0; }
            wave_sync();
            if (FWD) {
                for (int cc = 0; cc < c1 - c0; cc++) {
                    const double yj = bl[c0 + cc];
                    for (int i = cc + 1 + t; i < h; i += 64) bl[c0 + i] -= Pc[i + h * cc] * yj;
                    wave_sync();
                }
            } else {
                for (int cc = c1 - c0 - 1; cc >= 0; cc--) {
                    double sacc = 0.0;
                    for (int i = cc + 1 + t; i < h; i += 64) sacc += Pc[i + h * cc] * bl[c0 + i];
                    sacc = g_sum<64>(sacc);
                    if (t == 0) bl[c0 + cc] -= sacc;
                    wave_sync();
                }
            }
        }
        wave_sync();
        if (FWD) { for (int i = t; i < ff; i += 64) b[i < np ? piv0 + i : rows[i - np]] = bl[i]; }
        else { for (int i = t; i < np; i += 64) b[piv0 + i] = bl[i]; }
        g_sync();
    }
}

__device__ __forceinline__ void sp_general_solve(SpCtx<64>& c, bool admm, GD b)
{
    const SpBatch& db = *c.db;
    SPROF(c, SP_VECTORS);
    sp_general_sweep<true>(c, c.KF(admm), b);
    {
        GD Kd = c.KD(admm);
        g_map<64, 8>(db.N, c.gl, [&](int p) { return D2{b[p], Kd[p]}; }, [&](int p, D2 v) { b[p] = v.a * v.b; });
        g_sync();
    }
    SPROF(c, SP_FORWARD);
    sp_general_sweep<false>(c, c.KF(admm), b);
    SPROF(c, SP_BACKWARD);
    c.bytes += db.by[BY_SOLVE];
}

template <int G, class Dd, class Use>
__device__ __forceinline__ void sp_factor_band(SpCtx<G>& c, GD KF, GD Kd, double dprim, Dd ddual, Use use)
{
    if constexpr (G == 64) { if (c.db->general) { sp_general_factor(c, KF, Kd, dprim, ddual, use); return; } }
    if constexpr (G <= 16) sp_factor_reg<G>(c, KF, Kd, dprim, ddual, use);
    else { sp_assemble<G>(c, dprim, ddual, use); sp_factor_lds<G>(c, KF, Kd); }
}

// ---- band sweeps: L y = b, z = y / D (forward) and L' x = z (backward), in place ----------------------------------------------------
// Position p (0 .. Np-1 in processing order: row p forward, row Np-1-p backward) is pending in lane p % G of the group while steps
// p-G+1 .. p run; every step broadcasts the finished entry inside the group and every lane subtracts its multiple -- axpy form, no
// reduction in the chain.  The folded layouts put the coefficient lane u needs at step s of a block of G steps at K[(blk + u) * G + s]:
// one 8 G-byte row per lane and block, the rows of a group contiguous (G x G doubles per block), streamed RING chunks ahead of use.
// Right-hand sides and 1/D for the next 64 positions are loaded while the current 64 run.
template <int G, bool FWD>
__device__ __forceinline__ void band_sweep(GD K, GD Kd, GD b, int Np, int gl)
{
    // RING: coefficient chunks (CH steps each) in flight.  At G = 8 eight: seven chunks = 56 steps ahead of use, 8 800 / 5 600 clocks of the
    // forward / backward sweep, more than a round trip to memory on a busy machine (profiles/round5/sparse_sweep_ring8_ab.log)
    constexpr int CH = G < 16 ? G : 16, NCHUNK = 64 / CH, BPS = 64 / G, RING = (G == 8) ? 8 : 2;
    static_assert(RING >= 2 && NCHUNK % RING == 0, "the ring slots are assigned statically per 64 positions: RING has to divide 64 / CH (6 gave wrong coefficients and a run without end)");
    gl = here(gl);
    auto at = [&](int p) -> int { return FWD ? p : Np - 1 - p; };
    double cf[RING][CH];
    auto load_chunk = [&](double* dst, int sb, int ck) {
        const int s0 = ck * CH, bi = s0 / G, so = s0 % G;
        if (sb < Np) {
            if (FWD) {
                const int e0 = (sb + bi * G + gl) * G + so;
#pragma unroll
                for (int q = 0; q < CH / 2; q++) { const dv2 v = K.ld2(e0 + 2 * q); dst[2 * q] = v.x; dst[2 * q + 1] = v.y; }
            } else {
                // the same array read the other way: at step k of a block (row r = Np-1-(pb+k) finishes) the lane whose pending
                // row is i needs L[r][i] = K[((i / G) * G + r % G) * G + i % G]; i % G = G-1-gl, r % G = G-1-k, and i lies in the
                // row block of r for gl > k, in the one below for gl < k.  One double per lane and step, a group reads 8 G bytes
                // of one or two rows.
                const int pb = sb + bi * G;
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const int k = so + q;
                    const int iblk = Np - G - pb - (gl < k ? G : 0);
                    dst[q] = (iblk >= 0) ? K.ld((iblk + (G - 1 - k)) * G + (G - 1 - gl)) : 0.0;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < CH; q++) dst[q] = 0.0;
        }
    };
    // rh[q], dl[q]: right-hand side and 1/D of this lane's position in block q of the current 64 positions; a slot is refilled for
    // the next 64 as soon as it has been consumed
    double rh[BPS], dl[BPS];
#pragma unroll
    for (int q = 0; q < BPS; q++) { rh[q] = b[at(q * G + gl)]; dl[q] = FWD ? Kd.ld(q * G + gl) : 1.0; }
#pragma unroll
    for (int ck = 0; ck < RING - 1; ck++) load_chunk(cf[ck], 0, ck);
    double cur = rh[0];
    if (64 < Np) rh[0] = b[at(64 + gl)];
    for (int sb = 0; sb < Np; sb += 64) {
        const bool more = sb + 64 < Np, more2 = sb + 128 < Np;
        double res = 0.0;
#pragma unroll
        for (int ck = 0; ck < NCHUNK; ck++) {
            { const int nck = ck + RING - 1; load_chunk(cf[nck % RING], sb + 64 * (nck / NCHUNK), nck % NCHUNK); }
#pragma unroll
            for (int q = 0; q < CH; q++) {
                const int s = ck * CH + q, k = s % G, bi = s / G;
                const double yj = g_bcast<G>(cur, k);
                cur -= cf[ck % RING][q] * yj;
                if (gl == k) { res = yj; cur = rh[(bi + 1) % BPS]; }      // block bi+1 of these 64, or block 0 of the next 64 (already refilled)
                if (k == G - 1) {                                          // block bi is complete: store it, refill its slots
                    b[at(sb + bi * G + gl)] = FWD ? res * dl[bi] : res;
                    if (bi + 1 < BPS) { if (more) { rh[bi + 1] = b[at(sb + 64 + (bi + 1) * G + gl)]; } }
                    else if (more2) rh[0] = b[at(sb + 128 + gl)];
                    if (FWD && more) dl[bi] = Kd.ld(sb + 64 + bi * G + gl);
                }
            }
        }
    }
}

template <int G>
__device__ __forceinline__ void sp_solve_band(SpCtx<G>& c, bool admm, GD b)
{
    if constexpr (G == 64) { if (c.db->general) { sp_general_solve(c, admm, b); return; } }
    const int Np = c.db->Np;
    SPROF(c, SP_VECTORS);
    band_sweep<G, true>(c.KF(admm), c.KD(admm), b, Np, c.gl);
    g_sync();
    SPROF(c, SP_FORWARD);
    band_sweep<G, false>(c.KF(admm), c.KD(admm), b, Np, c.gl);
    g_sync();
    SPROF(c, SP_BACKWARD);
    c.bytes += c.db->by[BY_SOLVE];
}

// ---- the border (oracle: kkt_factor / kkt_solve) ---------------------------------------------------------------------------------
// After the band factorisation: the gated values of U (sp_border_prepare), W = U inv(Bd) -- one band solve per border node, run by the
// caller through ITS call site of the band solve (sp_border_column scatters column j; the kernel carries one copy of the sweeps per
// context) --, then S = C - W U' and its LDL' (sp_border_schur).
template <int G, class Use>
__device__ __forceinline__ void sp_border_prepare(SpCtx<G>& c, bool admm, Use use)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl), kb = db.kb, Np = db.Np, nnzQ = db.nnzQ, nU = db.nU;
    GD W = c.BW(admm), Uv = c.BUv(admm), Qv = c.Qx(), Ev = c.Ex();
    for (int e = t; e < nU; e += G) {
        const int src = db.Usrc[e], gate = db.Ugate[e];
        Uv[e] = (gate >= 0 && !use(gate)) ? 0.0 : (src >= nnzQ ? (double)Ev[src - nnzQ] : (double)Qv[src]);
    }
    for (int p = t; p < kb * Np; p += G) W[p] = 0.0;
    g_sync();
}
template <int G>
__device__ __forceinline__ GD sp_border_column(SpCtx<G>& c, bool admm, int b)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl);
    GD wb = c.BW(admm) + b * db.Np, Uv = c.BUv(admm);
    for (int e = db.Uptr[b] + t; e < db.Uptr[b + 1]; e += G) wb[db.Upos[e]] = Uv[e];
    g_sync();
    return wb;
}
template <int G, class Dd, class Use>
__device__ __forceinline__ void sp_border_schur(SpCtx<G>& c, bool admm, double dprim, Dd ddual, Use use)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl), kb = db.kb, Np = db.Np, nnzQ = db.nnzQ, nvar = db.n;
    GD W = c.BW(admm), Uv = c.BUv(admm), S = c.BS(admm), Qv = c.Qx(), Ev = c.Ex();
    // C: the border block itself (lane 0; a handful of entries), then S = C - W U'
    if (t == 0) {
        for (int e = 0; e < kb * kb; e++) S[e] = 0.0;
        for (int a = 0; a < kb; a++) {
            const int node = db.bnode[a];
            double dg;
            if (node < nvar) { const int qd = db.qdiag[node]; dg = (qd >= 0 ? (double)Qv[qd] : 0.0) + dprim; }
            else { const int rr = node - nvar; dg = use(rr) ? -ddual(rr) : -1.0; }
            S[a * kb + a] = dg;
            for (int e = db.Cptr[a]; e < db.Cptr[a + 1]; e++) {
                const int b2 = db.Cb2[e], src = db.Csrc[e], gate = db.Cgate[e];
                const double v = (gate >= 0 && !use(gate)) ? 0.0 : (src >= nnzQ ? (double)Ev[src - nnzQ] : (double)Qv[src]);
                S[a * kb + b2] += v; S[b2 * kb + a] += v;
            }
        }
    }
    g_sync();
    for (int a = 0; a < kb; a++)
        for (int b2 = 0; b2 < kb; b2++) {
            GD wb = W + b2 * Np;
            double sacc = 0.0;
            for (int e = db.Uptr[a] + t; e < db.Uptr[a + 1]; e += G) sacc += Uv[e] * wb[db.Upos[e]];
            sacc = g_sum<G>(sacc);
            if (t == 0) S[a * kb + b2] -= sacc;
        }
    g_sync();
    if (t == 0) {      // S = L D L' in place: L below the diagonal, D on it (quasi-definite: no pivoting)
        for (int j = 0; j < kb; j++) {
            double d = S[j * kb + j];
            for (int k = 0; k < j; k++) { const double ljk = S[j * kb + k]; d -= ljk * ljk * S[k * kb + k]; }
            S[j * kb + j] = d;
            for (int i = j + 1; i < kb; i++) {
                double v = S[i * kb + j];
                for (int k = 0; k < j; k++) v -= S[i * kb + k] * S[j * kb + k] * S[k * kb + k];
                S[i * kb + j] = v / d;
            }
        }
    }
    g_sync();
    c.bytes += db.by[BY_BORDER_PREPARE];
}
// After the band solve of b (the border positions pass through it untouched): the border unknowns from S, then the band part corrected
template <int G>
__device__ __forceinline__ void sp_border_solve(SpCtx<G>& c, bool admm, GD b)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl), kb = db.kb, Np = db.Np, Nb = db.N - db.kb;
    GD W = c.BW(admm), Uv = c.BUv(admm), S = c.BS(admm);
    for (int a = 0; a < kb; a++) {
        double sacc = 0.0;
        for (int e = db.Uptr[a] + t; e < db.Uptr[a + 1]; e += G) sacc += Uv[e] * b[db.Upos[e]];
        sacc = g_sum<G>(sacc);
        if (t == 0) b[Nb + a] -= sacc;
    }
    g_sync();
    if (t == 0) {
        for (int i = 0; i < kb; i++) { double v = b[Nb + i]; for (int k = 0; k < i; k++) v -= S[i * kb + k] * b[Nb + k]; b[Nb + i] = v; }
        for (int i = 0; i < kb; i++) b[Nb + i] = b[Nb + i] / S[i * kb + i];
        for (int i = kb - 1; i >= 0; i--) { double v = b[Nb + i]; for (int k = i + 1; k < kb; k++) v -= S[k * kb + i] * b[Nb + k]; b[Nb + i] = v; }
    }
    g_sync();
    for (int p = t; p < Nb; p += G) {
        double acc = 0.0;
        for (int a = 0; a < kb; a++) acc += W[a * Np + p] * b[Nb + a];
        b[p] -= acc;
    }
    g_sync();
    c.bytes += db.by[BY_BORDER_SOLVE];
}
// K x = b in place: the band solve, then the border
template <int G>
__device__ __forceinline__ void sp_solve(SpCtx<G>& c, bool admm, GD b)
{
    sp_solve_band<G>(c, admm, b);
    if (c.db->kb > 0) sp_border_solve<G>(c, admm, b);
}

// ---- the panel forms: P right-hand sides behind one pass over the factor (k_sparse_sensitivity_blk, DESIGN.md section 3a''') --------------
// The P vectors of a panel are stored INTERLEAVED: position p of column k is b[p * P + k], so that a lane fetches the P values of its position
// with wide loads and the store of a finished block is contiguous.  Per step one coefficient is loaded exactly as band_sweep loads it (the
// ring, the chunking and the folded layout are its own), P values are broadcast and P multiply-subtracts follow: P independent chains per
// lane for the coefficient traffic of one.  Per column the sequence of operations is the one of band_sweep, so a column's result depends on
// nothing but that column.  The scalar routines above are untouched: every kernel that had them keeps its code.
template <int G, int P, bool FWD>
__device__ __forceinline__ void band_sweep_panel(GD K, GD Kd, GD b, int Np, int gl)
{
    static_assert(P % 2 == 0, "the panel is moved in pairs of doubles");
    constexpr int CH = G < 16 ? G : 16, NCHUNK = 64 / CH, BPS = 64 / G, RING = (G == 8) ? 8 : 2;
    static_assert(RING >= 2 && NCHUNK % RING == 0, "RING has to divide 64 / CH (band_sweep)");
    gl = here(gl);
    auto at = [&](int p) -> int { return FWD ? p : Np - 1 - p; };
    double cf[RING][CH];
    auto load_chunk = [&](double* dst, int sb, int ck) {      // band_sweep's
        const int s0 = ck * CH, bi = s0 / G, so = s0 % G;
        if (sb < Np) {
            if (FWD) {
                const int e0 = (sb + bi * G + gl) * G + so;
#pragma unroll
                for (int q = 0; q < CH / 2; q++) { const dv2 v = K.ld2(e0 + 2 * q); dst[2 * q] = v.x; dst[2 * q + 1] = v.y; }
            } else {
                const int pb = sb + bi * G;
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const int k = so + q;
                    const int iblk = Np - G - pb - (gl < k ? G : 0);
                    dst[q] = (iblk >= 0) ? K.ld((iblk + (G - 1 - k)) * G + (G - 1 - gl)) : 0.0;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < CH; q++) dst[q] = 0.0;
        }
    };
    auto load_pos = [&](double* dst, int p) {
#pragma unroll
        for (int k = 0; k < P / 2; k++) { const dv2 v = b.ld2(p * P + 2 * k); dst[2 * k] = v.x; dst[2 * k + 1] = v.y; }
    };
    double rh[BPS][P], dl[BPS], cur[P], res[P];
#pragma unroll
    for (int q = 0; q < BPS; q++) { load_pos(rh[q], at(q * G + gl)); dl[q] = FWD ? Kd.ld(q * G + gl) : 1.0; }
#pragma unroll
    for (int ck = 0; ck < RING - 1; ck++) load_chunk(cf[ck], 0, ck);
#pragma unroll
    for (int c = 0; c < P; c++) { cur[c] = rh[0][c]; res[c] = 0.0; }
    if (64 < Np) load_pos(rh[0], at(64 + gl));
    for (int sb = 0; sb < Np; sb += 64) {
        const bool more = sb + 64 < Np, more2 = sb + 128 < Np;
#pragma unroll
        for (int ck = 0; ck < NCHUNK; ck++) {
            { const int nck = ck + RING - 1; load_chunk(cf[nck % RING], sb + 64 * (nck / NCHUNK), nck % NCHUNK); }
#pragma unroll
            for (int q = 0; q < CH; q++) {
                const int s = ck * CH + q, k = s % G, bi = s / G;
                double yj[P];
#pragma unroll
                for (int c = 0; c < P; c++) yj[c] = g_bcast<G>(cur[c], k);
#pragma unroll
                for (int c = 0; c < P; c++) cur[c] -= cf[ck % RING][q] * yj[c];
                if (gl == k) {
#pragma unroll
                    for (int c = 0; c < P; c++) { res[c] = yj[c]; cur[c] = rh[(bi + 1) % BPS][c]; }
                }
                if (k == G - 1) {                                          // block bi is complete: store it, refill its slots
                    const int p = at(sb + bi * G + gl);
#pragma unroll
                    for (int c = 0; c < P; c++) b[p * P + c] = FWD ? res[c] * dl[bi] : res[c];
                    if (bi + 1 < BPS) { if (more) load_pos(rh[bi + 1], at(sb + 64 + (bi + 1) * G + gl)); }
                    else if (more2) load_pos(rh[0], at(sb + 128 + gl));
                    if (FWD && more) dl[bi] = Kd.ld(sb + 64 + bi * G + gl);
                }
            }
        }
    }
}

// the polish factor on a panel, band engines (the general LDL' has its own panel form: sp_general_solve_panel below).  Reads the factor and
// the border; writes the panel alone -- no counter of the context, nothing of the instance.
template <int G, int P>
__device__ __forceinline__ void sp_solve_band_panel(SpCtx<G>& c, GD b)
{
    const int Np = c.db->Np;
    band_sweep_panel<G, P, true>(c.KF(false), c.KD(false), b, Np, c.gl);
    g_sync();
    band_sweep_panel<G, P, false>(c.KF(false), c.KD(false), b, Np, c.gl);
    g_sync();
}
// sp_border_solve per column: the kb border dot products and the W correction for the P columns; lane 0 solves with S once per column
template <int G, int P>
__device__ __forceinline__ void sp_border_solve_panel(SpCtx<G>& c, GD b)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl), kb = db.kb, Np = db.Np, Nb = db.N - db.kb;
    GD W = c.BW(false), Uv = c.BUv(false), S = c.BS(false);
    for (int a = 0; a < kb; a++) {
        double sacc[P];
#pragma unroll
        for (int k = 0; k < P; k++) sacc[k] = 0.0;
        for (int e = db.Uptr[a] + t; e < db.Uptr[a + 1]; e += G) {
            const double u = Uv[e]; const int pos = db.Upos[e];
#pragma unroll
            for (int k = 0; k < P; k++) sacc[k] += u * b[pos * P + k];
        }
#pragma unroll
        for (int k = 0; k < P; k++) { const double sa = g_sum<G>(sacc[k]); if (t == 0) b[(Nb + a) * P + k] -= sa; }
    }
    g_sync();
    if (t == 0) {
        for (int k = 0; k < P; k++) {
            for (int i = 0; i < kb; i++) { double v = b[(Nb + i) * P + k]; for (int j = 0; j < i; j++) v -= S[i * kb + j] * b[(Nb + j) * P + k]; b[(Nb + i) * P + k] = v; }
            for (int i = 0; i < kb; i++) b[(Nb + i) * P + k] = b[(Nb + i) * P + k] / S[i * kb + i];
            for (int i = kb - 1; i >= 0; i--) { double v = b[(Nb + i) * P + k]; for (int j = i + 1; j < kb; j++) v -= S[j * kb + i] * b[(Nb + j) * P + k]; b[(Nb + i) * P + k] = v; }
        }
    }
    g_sync();
    for (int p = t; p < Nb; p += G) {
        double acc[P];
#pragma unroll
        for (int k = 0; k < P; k++) acc[k] = 0.0;
        for (int a = 0; a < kb; a++) {
            const double w = W[a * Np + p];
#pragma unroll
            for (int k = 0; k < P; k++) acc[k] += w * b[(Nb + a) * P + k];
        }
#pragma unroll
        for (int k = 0; k < P; k++) b[p * P + k] -= acc[k];
    }
    g_sync();
}
template <int G, int P>
__device__ __forceinline__ void sp_solve_panel(SpCtx<G>& c, GD b)
{
    sp_solve_band_panel<G, P>(c, b);
    if (c.db->kb > 0) sp_border_solve_panel<G, P>(c, b);
}

// ---- the general LDL' on a panel (k_sparse_sensitivity_blk_general, DESIGN.md section 3a''', "The general engine") ------------------------
// One front of sp_general_sweep for P right-hand sides, interleaved as above.  Lane t holds rows t, t + 64, ... of the front, QR of them, the
// P values of a row in P registers: a pivot step is one coefficient per held row (read from the factor exactly as the vector sweep reads it,
// U pivots' worth in flight), P broadcasts and P fused multiply-adds per held row -- P independent chains behind every coefficient.  The
// front is walked by chunks of 64 rows with the chunk number a compile-time constant, so the register a pivot is broadcast from is fixed by
// the code, and the rows of the chunks a pivot cannot reach (above it forward, below it backward) are not touched.  All three front classes
// are this one routine: QR = 1 (ff <= 64), 4 (ff <= 256), 9 (ff <= GEN_MAX_FRONT); the right-hand sides of the largest class live in
// registers too (72 doubles per lane), so the routine uses no LDS.  Axpy form both ways, as the vector sweep.
// Per column the operations are: x_i -= l_ij y_j for the pivots j in ascending (forward) or the rows i in descending (backward) order --
// whatever the column's place in the panel, whatever its neighbours hold.  A zero column stays zero.
template <int P, int QR, int U, bool FWD>
__device__ __forceinline__ void sp_general_front_panel(GD Lp, GD b, const int* rows, int np, int ff, int piv0, int t)
{
    static_assert(P % 2 == 0, "the panel is moved in pairs of doubles");
    double x[QR][P];
#pragma unroll
    for (int q = 0; q < QR; q++) {
        const int i = t + 64 * q;
        if (i < ff) {
            const int pos = i < np ? piv0 + i : rows[i - np];
#pragma unroll
            for (int k = 0; k < P / 2; k++) { const dv2 v = b.ld2(pos * P + 2 * k); x[q][2 * k] = v.x; x[q][2 * k + 1] = v.y; }
        } else {
#pragma unroll
            for (int k = 0; k < P; k++) x[q][k] = 0.0;
        }
    }
    if (FWD) {
#pragma unroll
        for (int qp = 0; qp < QR; qp++) {      // the pivots of chunk qp: they live in x[qp], and reach the rows of the chunks qp .. QR-1
            const int je = min(np, 64 * qp + 64);
            for (int j0 = 64 * qp; j0 < je; j0 += U) {
                double lv[U][QR];
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int q = 0; q < QR; q++)
                        if (q >= qp) { const int j = j0 + u, i = t + 64 * q; lv[u][q] = (j < je && i > j && i < ff) ? (double)Lp[i + ff * j] : 0.0; }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int j = j0 + u;
                    if (j < je) {
                        double y[P];
#pragma unroll
                        for (int k = 0; k < P; k++) y[k] = wave_bcast(x[qp][k], j - 64 * qp);
#pragma unroll
                        for (int q = 0; q < QR; q++)
                            if (q >= qp) {
#pragma unroll
                                for (int k = 0; k < P; k++) x[q][k] -= lv[u][q] * y[k];
                            }
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int qq = 0; qq < QR; qq++) {      // the rows of chunk qi, last chunk first: they live in x[qi], and reach the pivots of the chunks 0 .. qi
            const int qi = QR - 1 - qq;
            const int ihi = min(ff - 1, 64 * qi + 63), ilo = max(1, 64 * qi);
            for (int i0 = ihi; i0 >= ilo; i0 -= U) {
                double lv[U][QR];
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int q = 0; q < QR; q++)
                        if (q <= qi) { const int i = i0 - u, j = t + 64 * q; lv[u][q] = (i >= ilo && j < i && j < np) ? (double)Lp[i + ff * j] : 0.0; }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int i = i0 - u;
                    if (i >= ilo) {
                        double y[P];
#pragma unroll
                        for (int k = 0; k < P; k++) y[k] = wave_bcast(x[qi][k], i - 64 * qi);
#pragma unroll
                        for (int q = 0; q < QR; q++)
                            if (q <= qi) {
#pragma unroll
                                for (int k = 0; k < P; k++) x[q][k] -= lv[u][q] * y[k];
                            }
                    }
                }
            }
        }
    }
    // forward: the pivots and the update rows go back; backward: the pivots alone (the rows behind them belong to the ancestors)
#pragma unroll
    for (int q = 0; q < QR; q++) {
        const int i = t + 64 * q;
        if (i < (FWD ? ff : np)) {
            const int pos = i < np ? piv0 + i : rows[i - np];
#pragma unroll
            for (int k = 0; k < P; k++) b[pos * P + k] = x[q][k];
        }
    }
}

// sp_general_sweep for a panel: the fronts in postorder (forward) or in reverse (backward), each by the class of its size
template <int P, bool FWD>
__device__ __forceinline__ void sp_general_sweep_panel(SpCtx<64>& c, GD Lst, GD b)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl);
    static_assert(GEN_MAX_FRONT <= 9 * 64, "the largest class holds nine rows per lane");
    for (int q = 0; q < db.gnF; q++) {
        const int f = FWD ? q : db.gnF - 1 - q;
        const int* mt = db.gMeta + (size_t)f * GEN_META;
        const int np = mt[0], nb = mt[1], ff = np + nb, piv0 = mt[2];
        const int* rows = db.gRows + mt[3];
        GD Lp = Lst + mt[8];
        if (ff <= 64) sp_general_front_panel<P, 1, 8, FWD>(Lp, b, rows, np, ff, piv0, t);
        else if (ff <= 256) sp_general_front_panel<P, 4, 4, FWD>(Lp, b, rows, np, ff, piv0, t);
        else sp_general_front_panel<P, 9, 2, FWD>(Lp, b, rows, np, ff, piv0, t);
        g_sync();      // the update rows a front wrote are read by other lanes in its parent
    }
}

// sp_general_solve on a panel, for the polish factor: forward, 1 / D per position for all P columns, backward.  Reads the factor, 1 / D,
// gMeta and gRows; writes the panel alone -- no counter of the context, nothing of the instance (no gStack, no gFront, no LDS).
template <int P>
__device__ __forceinline__ void sp_general_solve_panel(SpCtx<64>& c, GD b)
{
    const SpBatch& db = *c.db;
    sp_general_sweep_panel<P, true>(c, c.KF(false), b);
    {
        GD Kd = c.KD(false);
        const int t = here(c.gl);
        for (int p = t; p < db.N; p += 64) {
            const double dinv = Kd[p];
#pragma unroll
            for (int k = 0; k < P / 2; k++) { const dv2 v = b.ld2(p * P + 2 * k); b[p * P + 2 * k] = v.x * dinv; b[p * P + 2 * k + 1] = v.y * dinv; }
        }
        g_sync();
    }
    sp_general_sweep_panel<P, false>(c, c.KF(false), b);
}

}  // namespace
