// lcqp_hip_diff.hip -- differentiation of the dense arm's batch: the sensitivity, Jacobian and adjoint entry points of the C ABI
// lcqp_hip_batch_* (include/lcqp_hip.h) with their device-pointer twins, and the two adjoint kernels they launch.  A host call and its twin
// are one body with a flag `dev`: one guard per call shape, one chunk loop per Jacobian, one launch; the two differ in where the results go
// and in how the kernel time is kept.  The guards and the drivers around the kernels are lcqp_sens_rt.hpp's, which the sparse arm
// (lcqp_sparse_diff.hip) uses too; the batch's life cycle is lcqp_hip.hip, and lcqp_hip_batch.hpp is what the units share.
#include "lcqp_hip_batch.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace lcqp;
using namespace lcqp_rt;

// =================================================================================================
// device kernels: the per-size ones live in lcqp_kernels.hpp / lcqp_nch.hip; here only the two that are not templated and that the batch
// ABI launches (k_pack_dual_rows is in lcqp_hip_device.hip, four more in lcqp_hip_util.hip)
// =================================================================================================
// ---- the matrix gradients of an adjoint call (DESIGN.md section 3a'''', lcqp_hip_batch_adjoint) --------------------------------------
// With dg, db, side and info of k_sensitivity (nrhs = 1, still in its device buffers) and the returned x, y, row r of the stacked gradient
// [dQ; dA; dL; dR] ([nd][n]: r < n a row of Q, above it the entry of the dual layout the row of E belongs to) of instance b is
//   s_r (alpha_r x_b + beta_r dg_b),   r < n: alpha = dg_r, beta = x_r, s = 1/2 (the symmetric derivative);
//                                      r >= n: alpha = -db_r, beta = -y_r, s = 1 where side_r != 0, a zero row elsewhere;
// zero for an instance with info & 1.  The two products are rounded separately and then added (no contraction): entry (i, j) of dQ forms the
// products of entry (j, i) in the other order, so dQ is symmetric to the bit.  Both kernels read x, y and the four buffers, nothing else.
struct AdjointArgs {
    int B, n, np, nd, ldb;                 // ldb: pitch of db
    const double *x, *y, *dg, *db;         // xout [B][n], yout [B][nd], dg [B][np], db [B][ldb]
    const int *side, *info;                // [B][nd], [B]
};
// rows [r0, r0 + rows) of the stacked gradient go to out ([count][rows][n], or [rows][n] summed over the batch); null: not asked for
struct AdjointSeg { double* out; int r0, rows; };
struct AdjointSegs { AdjointSeg s[4]; };

__device__ __forceinline__ double adjoint_term(const AdjointArgs& a, int b, int r, int j)
{
#pragma clang fp contract(off)
    if (a.info[b] & 1) return 0.0;
    const double xj = a.x[(size_t)b * a.n + j], dj = a.dg[(size_t)b * a.np + j];
    if (r < a.n) return 0.5 * (a.dg[(size_t)b * a.np + r] * xj + a.x[(size_t)b * a.n + r] * dj);
    if (a.side[(size_t)b * a.nd + r] == 0) return 0.0;
    return -(a.db[(size_t)b * a.ldb + r] * xj + a.y[(size_t)b * a.nd + r] * dj);
}

// k_adjoint_outer: the gradients of the instances [first, first + count), one matrix per instance.  blockIdx.y: the segment; the threads
// walk its count * rows * n doubles as one array, two neighbours each (one 16-byte store; the buffers start on 16-byte boundaries).
__global__ __launch_bounds__(WG) void k_adjoint_outer(AdjointArgs a, AdjointSegs segs, int first, int count)
{
    const AdjointSeg sg = segs.s[blockIdx.y];
    if (!sg.out) return;
    const size_t per = (size_t)sg.rows * a.n, total = per * count;
    for (size_t p = ((size_t)blockIdx.x * WG + threadIdx.x) * 2; p < total; p += (size_t)gridDim.x * WG * 2) {
        double v[2] = {0.0, 0.0};
        for (int e = 0; e < 2; e++) {
            const size_t f = p + e;
            if (f >= total) break;
            const size_t o = f / per, rem = f - o * per;
            const int r = (int)(rem / a.n), j = (int)(rem - (size_t)r * a.n);
            v[e] = adjoint_term(a, first + (int)o, sg.r0 + r, j);
        }
        if (p + 1 < total) *reinterpret_cast<double2*>(sg.out + p) = double2{v[0], v[1]};
        else sg.out[p] = v[0];
    }
}

// k_adjoint_reduce: the same gradients summed over the batch (one Q / A / L / R shared by the instances).  A thread owns two neighbouring
// entries and adds the instances' terms -- the very values k_adjoint_outer writes -- in the order of the batch: no atomics, the same bits
// on every call, and the rounding error of a sum of B numbers, (B - 1) eps/2 sum_b |term_b|.  (A product [alpha' beta'] [X; DG] on the fp64
// matrix cores would round against the partial sums of alpha x and beta dg separately, which cancel inside a term: no bound in the terms.)
__global__ __launch_bounds__(WG) void k_adjoint_reduce(AdjointArgs a, AdjointSegs segs)
{
    const AdjointSeg sg = segs.s[blockIdx.y];
    if (!sg.out) return;
    const size_t total = (size_t)sg.rows * a.n;
    for (size_t p = ((size_t)blockIdx.x * WG + threadIdx.x) * 2; p < total; p += (size_t)gridDim.x * WG * 2) {
        const bool two = p + 1 < total;
        const int r0 = (int)(p / a.n), j0 = (int)(p - (size_t)r0 * a.n);
        const int r1 = two ? (int)((p + 1) / a.n) : r0, j1 = two ? (int)(p + 1 - (size_t)r1 * a.n) : j0;
        double s0 = 0.0, s1 = 0.0;
        for (int b = 0; b < a.B; b++) {
            s0 += adjoint_term(a, b, sg.r0 + r0, j0);
            s1 += adjoint_term(a, b, sg.r0 + r1, j1);
        }
        if (two) *reinterpret_cast<double2*>(sg.out + p) = double2{s0, s1};
        else sg.out[p] = s0;
    }
}

// =================================================================================================
// host side
// =================================================================================================
#define g_err dense_err()      // the error slot of the dense arm (thread_local, lcqp_hip.hip)

// ---- solution sensitivities (DESIGN.md sections 3a' and 3a'''): k_sensitivity on the whole batch, k_sensitivity_blk (np <= 512) on a range ----
// One launch through sensitivity_call (lcqp_sens_rt.hpp: host or device arrays in and out, the kernel time added to ms or left in the
// events).  blk: k_sensitivity_blk on the instances [first, first + count), on buffers of its own (the two kernels fix different pitches of
// db); v == nullptr: unit vectors, nothing uploaded.  Otherwise k_sensitivity -- with vy its DUAL instantiation --, which has no instance
// offset: first = 0, count = B.
static int dense_sensitivity(lcqp_hip_batch* h, bool blk, int first, int count, int nrhs, const double* v, const double* vy, bool dev,
                             double* dg, double* db, int* side, int* info, float& ms)
{
    DevBatch& d = h->db;
    // (ldV is the same for a Jacobian and a blocked call so that the rows reserved by one serve the other: a Jacobian's rows carry an unused v)
    const SensPitch p = {(size_t)d.n, (size_t)d.np, (size_t)d.nd + (blk ? 2 : 1) * (size_t)d.capS, (size_t)d.nd};
    return sensitivity_call(g_err, h, blk ? h->sensBlk : h->sn.sens, p, count, nrhs, v, vy, dev, blk ? 2 : 1, dg, db, side, info, ms,
                            [&](const double* dv, const double* dvy, SensBuffers& sb) {
        if (blk) h->k->sensitivity_blk(d, count, h->stream, first, nrhs, dv, sb.dg, sb.db, sb.side, sb.info);
        else if (vy) h->k->sensitivity_dual(d, count, h->stream, nrhs, dv, dvy, sb.dg, sb.db, sb.side, sb.info);
        else h->k->sensitivity(d, count, h->stream, nrhs, dv, sb.dg, sb.db, sb.side, sb.info);
    });
}

// blk: the blocked kernel where the padded size has one, the vector kernel and its bits above
int batch_sensitivity(lcqp_hip_batch* h, bool blk, int nrhs, const double* v, double* dg, double* db, int* side, int* info, bool dev, void* stream)
{
    return sens_body(g_err, h, dev, stream, [&](float& ms) {
        return dense_sensitivity(h, blk && h->k->sensitivity_blk, 0, h->db.B, nrhs, v, nullptr, dev, dg, db, side, info, ms);
    });
}

static int sensitivity_entry(lcqp_hip_batch* h, bool blk, int nrhs, const double* v, double* dg, double* db, int* side, int* info, bool dev, void* stream)
{ return guarded(g_err, [&] {
    if (int rc = guard_vectors(g_err, h, dev, nrhs, v, dg, db, side, info)) return rc;
    return batch_sensitivity(h, blk, nrhs, v, dg, db, side, info, dev, stream);
}); }

extern "C" int lcqp_hip_batch_sensitivity(lcqp_hip_batch_t* h, int nrhs, const double* v, double* dg, double* db, int* side, int* info)
{ return sensitivity_entry(h, false, nrhs, v, dg, db, side, info, false, nullptr); }

extern "C" int lcqp_hip_batch_sensitivity_blocked(lcqp_hip_batch_t* h, int nrhs, const double* v, double* dg, double* db, int* side, int* info)
{ return sensitivity_entry(h, true, nrhs, v, dg, db, side, info, false, nullptr); }

extern "C" int lcqp_hip_batch_sensitivity_device(lcqp_hip_batch_t* h, int blocked, int nrhs, const double* v, double* dg, double* db,
                                                 int* side, int* info, void* stream)
{ return sensitivity_entry(h, blocked != 0, nrhs, v, dg, db, side, info, true, stream); }

extern "C" int lcqp_hip_batch_set_jacobian_staging(lcqp_hip_batch_t* h, size_t bytes)
{
    return guarded(g_err, [&] { return set_staging(h, bytes); });
}

extern "C" int lcqp_hip_batch_sensitivity_timing(lcqp_hip_batch_t* h, float* kernel_ms)
{
    return guarded(g_err, [&] { return sensitivity_timing(g_err, h, kernel_ms, h ? &h->sensBlk : nullptr, h ? &h->sensDual : nullptr); });
}

// ---- full Jacobians (DESIGN.md section 3a'''): Jg [count][n][n], Jb [count][n][nd] (or NULL), side [count][nd], info [count] of the
// instances [first, first + count) ----
// k_sensitivity_blk on unit vectors, in chunks of instances whose staging (n rows of v, dg and db each) stays below the cap: one launch per
// chunk, its results copied to their place in the caller's arrays.  Host call: host arrays, a download per chunk, the kernel times summed
// into rs.sensMs.  dev (the device-pointer twin): device arrays and copies on the handle's stream; only a call of several chunks waits on
// the host, for the kernel time of each chunk but the last (chunk_time; the events are reused), whose own stays in the events.
// No blocked kernel (np >= 1024): k_sensitivity on an uploaded identity (these sizes are the single-large-problem ones, B small), for the
// twin copied to the device from the host call's arrays.
int dense_jacobian(lcqp_hip_batch* h, int first, int count, double* Jg, double* Jb, int* side, int* info, bool dev)
{
    DevBatch& d = h->db;
    const size_t n = d.n, nd = d.nd;
    if (!h->k->sensitivity_blk) {
        auto host = [&](double* G, double* Bd, int* sd, int* in) {
            return jacobian_by_vectors(h, sizeof(double) * (size_t)d.B * (n + (size_t)d.np + nd + (size_t)d.capS), nd, first, count, G, Bd, sd, in,
                                       [&](int nc, const double* v, double* dg, double* db, int* s, int* i, float& ms) {
                return dense_sensitivity(h, false, 0, d.B, nc, v, nullptr, false, dg, db, s, i, ms);
            });
        };
        return dev ? jacobian_through_host(g_err, h, nd, count, n, Jg, Jb, side, info, host) : host(Jg, Jb, side, info);
    }
    const size_t chunk = staging_chunk(h->sn.staging, sizeof(double) * n * (n + (size_t)d.np + nd + 2 * (size_t)d.capS), count);
    float ms = 0.f;      // host: of every chunk; dev: of the chunks in front of the last one
    for (size_t c0 = 0; c0 < (size_t)count; c0 += chunk) {
        const size_t cb = std::min(chunk, (size_t)count - c0);
        if (dev && c0) if (int rc = chunk_time(g_err, h->sensBlk, ms)) return rc;
        if (int rc = dense_sensitivity(h, true, first + (int)c0, (int)cb, d.n, nullptr, nullptr, dev, Jg + c0 * n * n, Jb ? Jb + c0 * n * nd : nullptr,
                                       side ? side + c0 * nd : nullptr, info ? info + c0 : nullptr, ms)) return rc;
    }
    (dev ? h->sn.pendingMs : h->rs.sensMs) = ms;
    return 0;
}

// ---- the full adjoint (DESIGN.md section 3a''''): upstream gradients on x and y, gradients in g, the bounds and the matrices ----
// k_sensitivity (with vy: its DUAL instantiation) on the whole batch, its results to the host (the device twin: to the caller's device
// arrays); then, on the device buffers it left, the matrix gradients that were asked for.
// the four segments of the stacked gradient as the caller asked for them (a segment without rows is not asked for)
struct AdjointWanted { double* out[4]; int r0[4], rows[4]; };
static AdjointWanted adjoint_wanted(const DevBatch& d, double* dQ, double* dA, double* dL, double* dR)
{
    return {{dQ, d.nC ? dA : nullptr, d.nComp ? dL : nullptr, d.nComp ? dR : nullptr}, {0, d.n, d.n + d.nC, d.n + d.nC + d.nComp}, {d.n, d.nC, d.nComp, d.nComp}};
}
// k_adjoint_reduce, or k_adjoint_outer on the instances [first, first + count); most: the doubles of the largest segment
static void launch_adjoint(lcqp_hip_batch* h, const AdjointSegs& segs, size_t most, int reduce, int first, int count)
{
    const DevBatch& d = h->db;
    const SensBuffers& sb = h->sn.sens;
    const AdjointArgs a = {d.B, d.n, d.np, d.nd, (int)sb.ldDb, d.xout, d.yout, sb.dg, sb.db, sb.side, sb.info};
    const unsigned gx = (unsigned)std::min<size_t>((most + 2 * WG - 1) / (2 * WG), 65535);
    if (reduce) hipLaunchKernelGGL(k_adjoint_reduce, dim3(gx, 4), dim3(WG), 0, h->stream, a, segs);
    else hipLaunchKernelGGL(k_adjoint_outer, dim3(gx, 4), dim3(WG), 0, h->stream, a, segs, first, count);
}

// The host call: k_adjoint_reduce once, or k_adjoint_outer per chunk of instances under the Jacobian staging cap (adjoint_chunks).  dev:
// ONE launch of either kernel that writes the caller's arrays: no staging buffer, no chunks.
int batch_adjoint(lcqp_hip_batch* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                  int reduce, double* dQ, double* dA, double* dL, double* dR, bool dev, void* stream)
{
    return sens_body(g_err, h, dev, stream, [&](float& ms) -> int {
        DevBatch& d = h->db;
        if (int rc = dense_sensitivity(h, false, 0, d.B, 1, vx, vy, dev, dg, db, side, info, ms)) return rc;
        const size_t n = d.n;
        const AdjointWanted w = adjoint_wanted(d, dQ, dA, dL, dR);
        if (dev) {
            AdjointSegs segs{};
            size_t most = 0;
            for (int k = 0; k < 4; k++) {
                if (!w.out[k]) continue;
                segs.s[k] = {w.out[k], w.r0[k], w.rows[k]};
                most = std::max(most, (reduce ? (size_t)1 : (size_t)d.B) * w.rows[k] * n);
            }
            if (!most) return 0;
            return adjoint_device(g_err, h, [&] { launch_adjoint(h, segs, most, reduce, 0, d.B); });
        }
        size_t perInst = 0;      // doubles of one instance's gradients
        for (int k = 0; k < 4; k++) if (w.out[k]) perInst += (size_t)w.rows[k] * n;
        if (!perInst) return 0;
        return adjoint_chunks(g_err, h, perInst, 4, reduce, ms, [&](size_t c0, size_t cb, AdjCopy* cp) {      // (+ 4: every segment starts on an even offset)
            AdjointSegs segs{};
            size_t off = 0, most = 0;
            int ncp = 0;
            for (int k = 0; k < 4; k++) {
                if (!w.out[k]) continue;
                const size_t cnt = cb * w.rows[k] * n;
                segs.s[k] = {h->sn.adjOut + off, w.r0[k], w.rows[k]};
                cp[ncp++] = {w.out[k] + c0 * w.rows[k] * n, segs.s[k].out, cnt};
                off += cnt + (cnt & 1);
                most = std::max(most, cnt);
            }
            launch_adjoint(h, segs, most, reduce, (int)c0, (int)cb);
            return ncp;
        });
    });
}

static int adjoint_entry(lcqp_hip_batch* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                         int reduce, double* dQ, double* dA, double* dL, double* dR, bool dev, void* stream)
{ return guarded(g_err, [&] {
    if (int rc = guard_pairs(g_err, h, dev, 1, vx, vy, true, reduce, dg, db, side, info)) return rc;
    if (dev) {      // the matrix gradients: the kernels store pairs of doubles
        const DevBatch& d = h->db;
        const size_t lead = sizeof(double) * (reduce ? (size_t)1 : (size_t)d.B) * d.n;
        if (!device_pointer_ok(g_err, h, "dQ", dQ, lead * d.n, 16) || !device_pointer_ok(g_err, h, "dA", dA, lead * d.nC, 16) ||
            !device_pointer_ok(g_err, h, "dL", dL, lead * d.nComp, 16) || !device_pointer_ok(g_err, h, "dR", dR, lead * d.nComp, 16)) return LCQP_INVALID_ARGUMENT;
    }
    return batch_adjoint(h, vx, vy, dg, db, side, info, reduce, dQ, dA, dL, dR, dev, stream);
}); }

extern "C" int lcqp_hip_batch_adjoint(lcqp_hip_batch_t* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                                      int reduce, double* dQ, double* dA, double* dL, double* dR)
{ return adjoint_entry(h, vx, vy, dg, db, side, info, reduce, dQ, dA, dL, dR, false, nullptr); }

extern "C" int lcqp_hip_batch_adjoint_device(lcqp_hip_batch_t* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                                             int reduce, double* dQ, double* dA, double* dL, double* dR, void* stream)
{ return adjoint_entry(h, vx, vy, dg, db, side, info, reduce, dQ, dA, dL, dR, true, stream); }

// ---- panels with gradients on y, the dual rows of the Jacobian (DESIGN.md section 3a'''', "Panels with gradients on y") ----
// k_sensitivity_blk_dual on the whole batch through sensitivity_call, on the buffers and pitches of the blocked kernel.  vy == nullptr:
// the blocked sensitivity call itself.  No blocked kernel (np >= 1024): k_sensitivity<NCH, true>, an absent vx as a zero panel.
static int dense_adjoint_blocked(lcqp_hip_batch* h, int nrhs, const double* vx, const double* vy, bool dev,
                                 double* dg, double* db, int* side, int* info, float& ms)
{
    DevBatch& d = h->db;
    if (!vy) return dense_sensitivity(h, h->k->sensitivity_blk != nullptr, 0, d.B, nrhs, vx, nullptr, dev, dg, db, side, info, ms);
    const bool blk = h->k->sensitivity_blk_dual != nullptr;
    const SensPitch p = {(size_t)d.n, (size_t)d.np, (size_t)d.nd + (blk ? 2 : 1) * (size_t)d.capS, (size_t)d.nd};
    std::vector<double> zeros;
    if (!blk && !vx && !dev) { zeros.assign((size_t)d.B * nrhs * d.n, 0.0); vx = zeros.data(); }
    hipError_t filled = hipSuccess;
    if (int rc = sensitivity_call(g_err, h, blk ? h->sensBlk : h->sn.sens, p, d.B, nrhs, vx, vy, dev, blk ? 2 : 1, dg, db, side, info, ms,
                                  [&](const double* dv, const double* dvy, SensBuffers& sb) {
        if (blk) { h->k->sensitivity_blk_dual(d, d.B, h->stream, 0, nrhs, dv, dvy, 0, sb.dg, sb.db, sb.side, sb.info, nullptr); return; }
        if (!dv) { filled = hipMemsetAsync(sb.v, 0, sizeof(double) * sb.rows * d.n, h->stream); dv = sb.v; }      // (the device twin without vx)
        h->k->sensitivity_dual(d, d.B, h->stream, nrhs, dv, dvy, sb.dg, sb.db, sb.side, sb.info);
    })) return rc;
    HIPCHK(g_err, filled);
    return 0;
}

static int adjoint_blocked_entry(lcqp_hip_batch* h, int nrhs, const double* vx, const double* vy, double* dg, double* db, int* side, int* info, bool dev, void* stream)
{ return guarded(g_err, [&] {
    if (int rc = guard_pairs(g_err, h, dev, nrhs, vx, vy, false, 0, dg, db, side, info)) return rc;
    return sens_body(g_err, h, dev, stream, [&](float& ms) { return dense_adjoint_blocked(h, nrhs, vx, vy, dev, dg, db, side, info, ms); });
}); }

extern "C" int lcqp_hip_batch_adjoint_blocked(lcqp_hip_batch_t* h, int nrhs, const double* vx, const double* vy, double* dg, double* db, int* side, int* info)
{ return adjoint_blocked_entry(h, nrhs, vx, vy, dg, db, side, info, false, nullptr); }

extern "C" int lcqp_hip_batch_adjoint_blocked_device(lcqp_hip_batch_t* h, int nrhs, const double* vx, const double* vy,
                                                     double* dg, double* db, int* side, int* info, void* stream)
{ return adjoint_blocked_entry(h, nrhs, vx, vy, dg, db, side, info, true, stream); }

// One launch of k_sensitivity_blk_dual on the unit vectors of the slot space of the instances [first, first + count), on sensDual:
// capS staged rows per instance (row j: the j-th occupied slot), no v, and behind the `count` rows of `side` the map [count][capS] from
// staged row to dual position (-1: no such slot).  dual_rowpos: where that map lies.
static int* dual_rowpos(lcqp_hip_batch* h, int count) { return h->sensDual.side + (size_t)count * h->db.nd; }
static int dual_jacobian_launch(lcqp_hip_batch* h, int first, int count)
{
    DevBatch& d = h->db;
    SensBuffers& sb = h->sensDual;
    HIPCHK(g_err, hipSetDevice(h->device));
    if (int rc = sb.reserve(g_err, h->mem, h->stream, count, d.capS, 0, d.np, (size_t)d.nd + 2 * (size_t)d.capS, (size_t)d.nd + d.capS)) return rc;
    h->sn.sensPending = 0;
    h->sn.pendingMs = 0.f;
    return timed_launch(g_err, h->stream, sb.ev0, sb.ev1, [&] {
        h->k->sensitivity_blk_dual(d, count, h->stream, first, d.capS, nullptr, nullptr, 1, sb.dg, sb.db, sb.side, sb.info, dual_rowpos(h, count));
    });
}

// np >= 1024: k_sensitivity<NCH, true> with vx = 0 and vy = the unit vectors of the dual positions that are in W for some instance of the
// range, uploaded in chunks of vectors under the cap, on the whole batch (the vector kernel has no instance offset)
static int jacobian_duals_by_vectors(lcqp_hip_batch* h, int first, int count, double* Jyg, double* Jyb, int* side, int* info)
{
    DevBatch& d = h->db;
    const size_t B = d.B, n = d.n, nd = d.nd;
    std::vector<double> zero(B * n, 0.0);
    return lcqp_rt::jacobian_duals_by_vectors(h, sizeof(double) * B * (n + (size_t)d.np + 2 * nd + (size_t)d.capS), nd, first, count, Jyg, Jyb, side, info,
                                              [&](int nc, const double* VY, double* G, double* Bd, int* sd, int* in, float& ms) {
        if (!VY) return dense_sensitivity(h, false, 0, d.B, 1, zero.data(), nullptr, false, G, nullptr, sd, in, ms);
        return dense_adjoint_blocked(h, nc, nullptr, VY, false, G, Bd, sd, in, ms);
    });
}

// Jyg [count][nd][n], Jyb [count][nd][nd] (or NULL), side [count][nd], info [count] of the instances [first, first + count), in chunks of
// instances whose staging (dual_jacobian_launch, with the map: an int per staged row) stays below the cap: one launch per chunk, then staged
// row j of an instance to the row of its dual position rowpos; the rows that receive nothing (outside W) are zero.  Host call: a download per
// chunk, the rows scattered on the host, the kernel times summed into rs.sensMs.  dev: k_pack_dual_rows and copies on the handle's stream,
// the kernel time as dense_jacobian keeps it.  No blocked kernel: jacobian_duals_by_vectors, for the twin copied to the device.
static int dense_jacobian_duals(lcqp_hip_batch* h, int first, int count, double* Jyg, double* Jyb, int* side, int* info, bool dev)
{
    DevBatch& d = h->db;
    const size_t n = d.n, nd = d.nd, capS = d.capS;
    if (!h->k->sensitivity_blk_dual) {
        auto host = [&](double* G, double* Bd, int* sd, int* in) { return jacobian_duals_by_vectors(h, first, count, G, Bd, sd, in); };
        return dev ? jacobian_through_host(g_err, h, nd, count, nd, Jyg, Jyb, side, info, host) : host(Jyg, Jyb, side, info);
    }
    if (dev) {
        HIPCHK(g_err, hipMemsetAsync(Jyg, 0, sizeof(double) * (size_t)count * nd * n, h->stream));
        if (Jyb) HIPCHK(g_err, hipMemsetAsync(Jyb, 0, sizeof(double) * (size_t)count * nd * nd, h->stream));
    } else {
        std::memset(Jyg, 0, sizeof(double) * (size_t)count * nd * n);
        if (Jyb) std::memset(Jyb, 0, sizeof(double) * (size_t)count * nd * nd);
    }
    const size_t chunk = staging_chunk(h->sn.staging, sizeof(double) * capS * ((size_t)d.np + nd + 2 * capS) + sizeof(int) * capS, count);
    std::vector<double> G(dev ? 0 : chunk * capS * n), Bd(Jyb && !dev ? chunk * capS * nd : 0);
    std::vector<int> rp(dev ? 0 : chunk * capS);
    const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    SensBuffers& sb = h->sensDual;
    float ms = 0.f;      // host: of every chunk; dev: of the chunks in front of the last one
    for (size_t c0 = 0; c0 < (size_t)count; c0 += chunk) {
        const size_t cb = std::min(chunk, (size_t)count - c0);
        if (dev && c0) if (int rc = chunk_time(g_err, sb, ms)) return rc;
        if (int rc = dual_jacobian_launch(h, first + (int)c0, (int)cb)) return rc;
        double *const og = Jyg + c0 * nd * n, *const ob = Jyb ? Jyb + c0 * nd * nd : nullptr;
        if (dev) {
            launch_pack_dual_rows(d, h->stream, (int)cb, (int)sb.ldDb, sb.dg, sb.db, dual_rowpos(h, (int)cb), og, ob);
            HIPCHK(g_err, hipGetLastError());
        } else {
            HIPCHK(g_err, hipMemcpyAsync(rp.data(), dual_rowpos(h, (int)cb), sizeof(int) * cb * capS, hipMemcpyDeviceToHost, h->stream));
            if (int rc = sb.rows_out(g_err, G.data(), sb.dg, n, sb.ldDg)) return rc;
            if (Jyb) if (int rc = sb.rows_out(g_err, Bd.data(), sb.db, nd, sb.ldDb)) return rc;
        }
        if (side) HIPCHK(g_err, hipMemcpyAsync(side + c0 * nd, sb.side, sizeof(int) * cb * nd, out, h->stream));
        if (info) HIPCHK(g_err, hipMemcpyAsync(info + c0, sb.info, sizeof(int) * cb, out, h->stream));
        if (dev) continue;
        HIPCHK(g_err, hipStreamSynchronize(h->stream));
        float t = 0.f;
        HIPCHK(g_err, hipEventElapsedTime(&t, sb.ev0, sb.ev1));
        ms += t;
        for (size_t j = 0; j < cb * capS; j++) {      // (the row map of k_pack_dual_rows)
            const int r = rp[j];
            if (r < 0 || (size_t)r >= nd) continue;
            std::memcpy(og + ((j / capS) * nd + r) * n, G.data() + j * n, sizeof(double) * n);
            if (Jyb) std::memcpy(ob + ((j / capS) * nd + r) * nd, Bd.data() + j * nd, sizeof(double) * nd);
        }
    }
    if (dev) h->sn.sensPending = 3;
    (dev ? h->sn.pendingMs : h->rs.sensMs) = ms;
    return 0;
}

static int jacobian_entry(lcqp_hip_batch* h, bool duals, int first, int count, double* Jg, double* Jb, int* side, int* info, bool dev, void* stream)
{ return guarded(g_err, [&] {
    if (int rc = guard_range(g_err, h, dev, duals, first, count, Jg, Jb, side, info)) return rc;
    auto body = [&] { return duals ? dense_jacobian_duals(h, first, count, Jg, Jb, side, info, dev) : dense_jacobian(h, first, count, Jg, Jb, side, info, dev); };
    return dev ? device_call(g_err, h, stream, body) : body();
}); }

extern "C" int lcqp_hip_batch_jacobian(lcqp_hip_batch_t* h, int first, int count, double* Jg, double* Jb, int* side, int* info)
{ return jacobian_entry(h, false, first, count, Jg, Jb, side, info, false, nullptr); }

extern "C" int lcqp_hip_batch_jacobian_device(lcqp_hip_batch_t* h, int first, int count, double* Jg, double* Jb, int* side, int* info, void* stream)
{ return jacobian_entry(h, false, first, count, Jg, Jb, side, info, true, stream); }

extern "C" int lcqp_hip_batch_jacobian_duals(lcqp_hip_batch_t* h, int first, int count, double* Jyg, double* Jyb, int* side, int* info)
{ return jacobian_entry(h, true, first, count, Jyg, Jyb, side, info, false, nullptr); }

extern "C" int lcqp_hip_batch_jacobian_duals_device(lcqp_hip_batch_t* h, int first, int count, double* Jyg, double* Jyb, int* side, int* info, void* stream)
{ return jacobian_entry(h, true, first, count, Jyg, Jyb, side, info, true, stream); }
