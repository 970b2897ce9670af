// lcqp_sparse_diff.hip -- differentiation of the sparse arm: the sensitivity, panel, Jacobian and adjoint entry points of the C ABI
// lcqp_hip_sparse_* (include/lcqp_hip.h) with their device-pointer twins, and the two kernels that do not depend on the lane-group width --
// the matrix gradients of lcqp_hip_sparse_adjoint --, as k_adjoint_outer / k_adjoint_reduce stand in lcqp_hip_diff.hip.  A host call and its
// twin are one body with a flag `dev`.  The guards and the drivers around the kernels are lcqp_sens_rt.hpp's, which the dense arm uses too;
// the solver's kernels are in lcqp_sparse.hip, reached through the launch tables (sp_kernels); the handle's life cycle is
// lcqp_sparse_host.hip, and lcqp_sparse_batch.hpp is what the units share.
#include "lcqp_sparse_batch.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace lcqp_rt;
using namespace lcqp_sparse;

#define g_sp_err sparse_err()      // the error slot of the sparse arm (thread_local, lcqp_sparse_host.hip)

// ---- the gradients on the non-zeros of an adjoint call (DESIGN.md section 3a'''', lcqp_hip_sparse_adjoint) ----------------------------------
// With dg, db, side and info of k_sparse_sensitivity (nrhs = 1, still in its device buffers) and the returned x, y of instance b:
//   stored entry k = (i, j) of Q:                 1/2 (dg_i x_j + x_i dg_j)     (the symmetric derivative);
//   stored entry k = (r, j) of E = [A; L; R]:     -(db_r x_j + y_r dg_j)  where side_r != 0, exactly 0.0 elsewhere;
// zero for an instance with info & 1.  The two products are rounded separately and then added (contraction is switched off in the two term
// functions: __dmul_rn / __dadd_rn are plain operators to this compiler and would be fused): entry (j, i) of Q forms the products of entry
// (i, j) in the other order, so the two are equal to the bit.  k runs over the CSR arrays of the
// device (SpBatch::Qp / Qi, Erow / Ei); the outputs are in the caller's CSC order: for the symmetric pattern of Q that is the CSR order, for E
// entry k goes to position emap[k] (the device copy of csr2csc).  Both kernels read x, y, the four buffers and the index arrays, nothing else.
constexpr int SP_ADJ_WG = 256;
struct SpAdjointArgs {
    int B, n, m, nnzQ, nnzE;
    const double *x, *y, *dg, *db;         // xout [B][n], yout [B][m], dg [B][n], db [B][m]
    const int *side, *info;                // [B][m], [B]
    const int *Qp, *Qi, *Erow, *Ei;        // row pointers and columns of Q; row and column of every entry of E
    const int* emap;                       // [nnzE], null when outE is
    double *outQ, *outE;                   // [count][nnzQ], [count][nnzE], or [nnzQ], [nnzE] summed over the batch; null: not asked for
};

// the row of entry k of a CSR pattern: the largest i with ptr[i] <= k
__device__ __forceinline__ int sp_adjoint_row(const int* ptr, int rows, int k)
{
    int lo = 0, hi = rows;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ptr[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ double sp_adjoint_q(const SpAdjointArgs& a, int b, int i, int j)
{
#pragma clang fp contract(off)
    if (a.info[b] & 1) return 0.0;
    const double *x = a.x + (size_t)b * a.n, *g = a.dg + (size_t)b * a.n;
    const double p0 = g[i] * x[j], p1 = x[i] * g[j];
    return 0.5 * (p0 + p1);
}
__device__ __forceinline__ double sp_adjoint_e(const SpAdjointArgs& a, int b, int r, int j)
{
#pragma clang fp contract(off)
    if ((a.info[b] & 1) || a.side[(size_t)b * a.m + r] == 0) return 0.0;
    const double p0 = a.db[(size_t)b * a.m + r] * a.x[(size_t)b * a.n + j], p1 = a.y[(size_t)b * a.m + r] * a.dg[(size_t)b * a.n + j];
    return -(p0 + p1);
}

// k_sparse_adjoint_nnz: the gradients of the instances [first, first + count), one value array per instance.  blockIdx.y 0: Q -- the threads
// walk its count * nnzQ doubles as one array, two neighbours each (one 16-byte store; the segment starts on a 16-byte boundary); 1: E -- one
// entry per thread, read in CSR order (coalesced gathers of the indices) and stored through the map.
__global__ __launch_bounds__(SP_ADJ_WG) void k_sparse_adjoint_nnz(SpAdjointArgs a, int first, int count)
{
    const size_t tid = (size_t)blockIdx.x * SP_ADJ_WG + threadIdx.x, nth = (size_t)gridDim.x * SP_ADJ_WG;
    if (blockIdx.y == 0) {
        if (!a.outQ) return;
        const size_t per = a.nnzQ, total = per * count;
        for (size_t p = tid * 2; p < total; p += nth * 2) {
            double v[2] = {0.0, 0.0};
            for (int e = 0; e < 2; e++) {
                const size_t f = p + e;
                if (f >= total) break;
                const size_t o = f / per;
                const int k = (int)(f - o * per);
                v[e] = sp_adjoint_q(a, first + (int)o, sp_adjoint_row(a.Qp, a.n, k), a.Qi[k]);
            }
            if (p + 1 < total) *reinterpret_cast<double2*>(a.outQ + p) = double2{v[0], v[1]};
            else a.outQ[p] = v[0];
        }
    } else {
        if (!a.outE) return;
        const size_t per = a.nnzE, total = per * count;
        for (size_t f = tid; f < total; f += nth) {
            const size_t o = f / per;
            const int k = (int)(f - o * per);
            a.outE[o * per + a.emap[k]] = sp_adjoint_e(a, first + (int)o, a.Erow[k], a.Ei[k]);
        }
    }
}

// k_sparse_adjoint_reduce: the same terms summed over the batch (one Qx / Ax shared by the instances).  A thread owns its entries (two
// neighbours of Q, one of E) and adds the instances' terms -- the very values k_sparse_adjoint_nnz writes -- in the order of the batch: no
// atomics, the same bits on every call, and the rounding error of a sum of B numbers, (B - 1) eps/2 sum_b |term_b|.
__global__ __launch_bounds__(SP_ADJ_WG) void k_sparse_adjoint_reduce(SpAdjointArgs a)
{
    const size_t tid = (size_t)blockIdx.x * SP_ADJ_WG + threadIdx.x, nth = (size_t)gridDim.x * SP_ADJ_WG;
    if (blockIdx.y == 0) {
        if (!a.outQ) return;
        const size_t total = a.nnzQ;
        for (size_t p = tid * 2; p < total; p += nth * 2) {
            const bool two = p + 1 < total;
            const int k0 = (int)p, k1 = two ? k0 + 1 : k0;
            const int i0 = sp_adjoint_row(a.Qp, a.n, k0), j0 = a.Qi[k0], i1 = sp_adjoint_row(a.Qp, a.n, k1), j1 = a.Qi[k1];
            double s0 = 0.0, s1 = 0.0;
            for (int b = 0; b < a.B; b++) {
                s0 += sp_adjoint_q(a, b, i0, j0);
                s1 += sp_adjoint_q(a, b, i1, j1);
            }
            if (two) *reinterpret_cast<double2*>(a.outQ + p) = double2{s0, s1};
            else a.outQ[p] = s0;
        }
    } else {
        if (!a.outE) return;
        for (size_t f = tid; f < (size_t)a.nnzE; f += nth) {
            const int k = (int)f, r = a.Erow[k], j = a.Ei[k];
            double s = 0.0;
            for (int b = 0; b < a.B; b++) s += sp_adjoint_e(a, b, r, j);
            a.outE[a.emap[k]] = s;
        }
    }
}

// ---- solution sensitivities (DESIGN.md section 3a''): one launch of k_sparse_sensitivity -- with vy ([B][nrhs][m]) the DUAL instantiation of
// lcqp_hip_sparse_adjoint -- on the whole batch through sensitivity_call (lcqp_sens_rt.hpp: host or device arrays in and out, the kernel time
// added to ms or left in the events) ----
static int sp_sensitivity(lcqp_hip_sparse* h, int nrhs, const double* v, const double* vy, bool dev, double* dg, double* db, int* side, int* info, float& ms)
{
    SpBatch& d = h->db;
    const SensPitch p = {(size_t)d.n, (size_t)d.n, (size_t)d.m, (size_t)d.m};
    hipError_t filled = hipSuccess;
    if (int rc = sensitivity_call(g_sp_err, h, h->sn.sens, p, d.B, nrhs, v, vy, dev, 1, dg, db, side, info, ms, [&](const double* dv, const double* dvy, SensBuffers& sb) {
        if (vy && !dv) { filled = hipMemsetAsync(sb.v, 0, sizeof(double) * sb.rows * d.n, h->stream); dv = sb.v; }      // (a device twin without vx)
        if (vy) sp_kernels(d.G)->sensitivity_dual(d, h->stream, nrhs, dv, dvy, sb.dg, sb.db, sb.side, sb.info);
        else sp_kernels(d.G)->sensitivity(d, h->stream, nrhs, dv, sb.dg, sb.db, sb.side, sb.info);
    })) return rc;
    HIPCHK(g_sp_err, filled);
    return 0;
}

// ---- panels of vectors and full Jacobians (DESIGN.md section 3a''', "The sparse arm"): k_sparse_sensitivity_blk on the work items
// (instance, panel) of the call, in chunks under the staging cap ----
// the panel width of the handle's engine; 0: the general LDL' without its switch (lcqp_hip_sparse_set_general_panel), which both entry
// points then run on the vector kernel
static int sp_panel(const lcqp_hip_sparse* h)
{
    const SpKernels* k = sp_kernels(h->db.G);
    return h->db.general ? (h->generalPanel ? k->panel_general : 0) : k->panel;
}
extern "C" int lcqp_hip_sparse_sens_panel(const lcqp_hip_sparse_t* h) { return h ? sp_panel(h) : 0; }
// the switch is a member of the handle and nothing else: no device call, no mark of the setup or the solution is touched
extern "C" int lcqp_hip_sparse_set_general_panel(lcqp_hip_sparse_t* h, int on)
{
    if (!h || (on != 0 && on != 1)) return LCQP_INVALID_ARGUMENT;
    h->generalPanel = on == 1;
    return 0;
}
extern "C" int lcqp_hip_sparse_max_front(const lcqp_hip_sparse_t* h) { return h ? (h->db.general ? h->db.gMaxFront : 0) : -1; }

// Instances [first, first + count), ncols columns each: v [count][ncols][n] on the host, or NULL = the unit vectors (ncols = n).  dg
// [count][ncols][n], db [count][ncols][m], side [count][m], info [count] on the host.  One launch and one download per chunk of items; staged
// column k of an item goes to the row sp_panel_dest_row gives it, with one copy per column.  The kernel time of the call is the sum over
// its launches.
// vy [count][ncols][m] (host) or dunit: the DUAL kernels (DESIGN.md section 3a'''', "The sparse arm: panels with gradients on y").  vy is staged
// in sn.adjVy, as the vector adjoint stages its vy, and v may then be NULL (a zero panel).  dunit: ncols = m, the unit columns of the working
// set, written by the kernel; dg [count][m][n] and db [count][m][m] are zero-filled here and receive staged column k of an item at row
// rowpos[item][k] (the map lies behind the workspaces in sb.ws); rows outside W stay exactly zero.
// dev (the device-pointer twins, DESIGN.md section 3a''''', "The sparse arm: panels and Jacobians into device arrays"): every array is the
// caller's device array.  v and vy are read where they lie; behind each chunk's launch k_sparse_scatter_panels takes the staged columns to the
// rows the host loop takes them to (rowpos stays on the device); dg and db of dunit are zero-filled on the stream, side and info go device to
// device.  Nothing waits on the host but a call of several chunks, for the kernel time of each chunk but the last (chunk_time); the last
// one's stays in the events (sensPending).
static int sp_panel_run(lcqp_hip_sparse* h, int first, int count, int ncols, const double* v, double* dg, double* db, int* side, int* info,
                        const double* vy = nullptr, bool dunit = false, bool dev = false)
{
    SpBatch& d = h->db;
    SensBuffers& sb = h->sn.sens;
    const size_t P = sp_panel(h), n = d.n, m = d.m, npan = ((size_t)ncols + P - 1) / P, nItems = (size_t)count * npan;
    const size_t wsItem = sens_blk_ws_doubles(d, (int)P);      // (the general LDL': Np >= N = n + m positions in the ordering of the fronts)
    const bool dual = vy || dunit;
    const SpKernels* const k = sp_kernels(d.G);
    SpSensitivityBlkFn* const launch = dual ? (d.general ? k->sensitivity_blk_general_dual : k->sensitivity_blk_dual)
                                            : (d.general ? k->sensitivity_blk_general : k->sensitivity_blk);
    const size_t chunk = staging_chunk(h->sn.staging, sizeof(double) * (P * (n + m) + wsItem) + (dunit ? sizeof(int) * P : 0), nItems);
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    const size_t vrows = (v && !dev) ? (size_t)count * ncols : 0;
    if (int rc = sb.reserve_rows(g_sp_err, h->mem, h->stream, count, std::max(vrows, chunk * P), n, n, m, m)) return rc;
    if (int rc = sb.reserve_ws(g_sp_err, h->mem, h->stream, chunk * wsItem + (dunit ? (chunk * P + 1) / 2 : 0))) return rc;
    int* const rowpos = dunit ? reinterpret_cast<int*>(sb.ws + chunk * wsItem) : nullptr;
    h->sn.sensPending = 0;
    h->sn.pendingMs = 0.f;
    const double *dv = v, *dvy = vy;
    if (v && !dev) {
        HIPCHK(g_sp_err, hipMemcpyAsync(sb.v, v, sizeof(double) * vrows * n, hipMemcpyHostToDevice, h->stream));
        dv = sb.v;
    }
    if (vy && !dev) {
        const size_t nvy = (size_t)count * ncols * m;
        if (int rc = grow(g_sp_err, h, h->sn.adjVy, h->sn.adjVyCap, nvy)) return rc;
        HIPCHK(g_sp_err, hipMemcpyAsync(h->sn.adjVy, vy, sizeof(double) * nvy, hipMemcpyHostToDevice, h->stream));
        dvy = h->sn.adjVy;
    }
    if (dunit && dev) {
        HIPCHK(g_sp_err, hipMemsetAsync(dg, 0, sizeof(double) * (size_t)count * m * n, h->stream));
        if (db) HIPCHK(g_sp_err, hipMemsetAsync(db, 0, sizeof(double) * (size_t)count * m * m, h->stream));
    } else if (dunit) {
        std::memset(dg, 0, sizeof(double) * (size_t)count * m * n);
        if (db) std::memset(db, 0, sizeof(double) * (size_t)count * m * m);
    }
    std::vector<int> rp(dunit && !dev ? chunk * P : 0);
    HIPCHK(g_sp_err, hipMemsetAsync(sb.info, 0, sizeof(int) * (size_t)count, h->stream));
    std::vector<double> hg(dev ? 0 : chunk * P * n), hb(db && !dev ? chunk * P * m : 0);
    float ms = 0.f;
    for (size_t i0 = 0; i0 < nItems; i0 += chunk) {
        const size_t ni = std::min(chunk, nItems - i0);
        const SpSensBlkArgs a = {first, (int)npan, ncols, (v || dual) ? 0 : 1, (int)i0, (int)ni, dv, sb.dg, sb.db, sb.side, sb.info, sb.ws,
                                 dvy, dunit ? 1 : 0, rowpos};
        if (dev && i0) if (int rc = chunk_time(g_sp_err, sb, ms)) return rc;      // (the events are about to be recorded again)
        if (int rc = timed_launch(g_sp_err, h->stream, sb.ev0, sb.ev1, [&] { launch(d, h->stream, a); })) return rc;
        if (dev) {
            if (int rc = sparse_scatter_panels(h, SpScatterArgs{(int)npan, ncols, dunit ? 1 : 0, (int)P, d.n, d.m, (int)i0, (int)ni, sb.dg, sb.db, rowpos, dg, db})) return rc;
            continue;
        }
        if (dunit) HIPCHK(g_sp_err, hipMemcpyAsync(rp.data(), rowpos, sizeof(int) * ni * P, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(g_sp_err, hipMemcpyAsync(hg.data(), sb.dg, sizeof(double) * ni * P * n, hipMemcpyDeviceToHost, h->stream));
        if (db) HIPCHK(g_sp_err, hipMemcpyAsync(hb.data(), sb.db, sizeof(double) * ni * P * m, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(g_sp_err, hipStreamSynchronize(h->stream));
        float t = 0.f;
        HIPCHK(g_sp_err, hipEventElapsedTime(&t, sb.ev0, sb.ev1));
        ms += t;
        for (size_t c = 0; c < ni * P; c++) {
            const long long row = sp_panel_dest_row((unsigned)(i0 + c / P), (unsigned)(c % P), (unsigned)npan, (unsigned)P, (unsigned)ncols, dunit ? 1 : 0, dunit ? rp[c] : 0);
            if (row < 0) continue;
            std::memcpy(dg + (size_t)row * n, hg.data() + c * n, sizeof(double) * n);
            if (db) std::memcpy(db + (size_t)row * m, hb.data() + c * m, sizeof(double) * m);
        }
    }
    const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (side) HIPCHK(g_sp_err, hipMemcpyAsync(side, sb.side, sizeof(int) * (size_t)count * m, out, h->stream));
    if (info) HIPCHK(g_sp_err, hipMemcpyAsync(info, sb.info, sizeof(int) * (size_t)count, out, h->stream));
    if (dev) {
        h->sn.sensPending = 1;
        h->sn.pendingMs = ms;
        return 0;
    }
    HIPCHK(g_sp_err, hipStreamSynchronize(h->stream));
    h->rs.sensMs = ms;
    return 0;
}

// ---- the entry points: a host call and its device-pointer twin are one body with the flag dev ----
// the body behind a guard: as it stands, or between the two halves of the twin's hand-over
template <class F>
static int sp_call(lcqp_hip_sparse* h, bool dev, void* stream, F body) { return dev ? device_call(g_sp_err, h, stream, body) : body(); }

// nrhs vectors vx -- with vy ([B][nrhs][m]): pairs -- per instance on the whole batch: sp_panel_run where `blocked` asks for the panel kernel
// and the engine has a panel form, else k_sparse_sensitivity and its bits (its DUAL instantiation takes an absent vx as a zero array)
static int sp_vectors(lcqp_hip_sparse* h, bool blocked, int nrhs, const double* vx, const double* vy, double* dg, double* db, int* side, int* info, bool dev, void* stream)
{
    if (blocked && sp_panel(h)) return sp_call(h, dev, stream, [&] { return sp_panel_run(h, 0, h->db.B, nrhs, vx, dg, db, side, info, vy, false, dev); });
    std::vector<double> zeros;
    if (vy && !vx && !dev) { zeros.assign((size_t)h->db.B * nrhs * h->db.n, 0.0); vx = zeros.data(); }
    return sens_body(g_sp_err, h, dev, stream, [&](float& ms) { return sp_sensitivity(h, nrhs, vx, vy, dev, dg, db, side, info, ms); });
}

static int sensitivity_entry(lcqp_hip_sparse* h, bool blocked, int nrhs, const double* v, double* dg, double* db, int* side, int* info, bool dev, void* stream)
{ return guarded(g_sp_err, [&] {
    if (int rc = guard_vectors(g_sp_err, h, dev, nrhs, v, dg, db, side, info)) return rc;
    return sp_vectors(h, blocked, nrhs, v, nullptr, dg, db, side, info, dev, stream);
}); }

extern "C" int lcqp_hip_sparse_sensitivity(lcqp_hip_sparse_t* h, int nrhs, const double* v, double* dg, double* db, int* side, int* info)
{ return sensitivity_entry(h, false, nrhs, v, dg, db, side, info, false, nullptr); }

extern "C" int lcqp_hip_sparse_sensitivity_device(lcqp_hip_sparse_t* h, int nrhs, const double* v, double* dg, double* db, int* side, int* info, void* stream)
{ return sensitivity_entry(h, false, nrhs, v, dg, db, side, info, true, stream); }

extern "C" int lcqp_hip_sparse_sensitivity_blocked(lcqp_hip_sparse_t* h, int nrhs, const double* v, double* dg, double* db, int* side, int* info)
{ return sensitivity_entry(h, true, nrhs, v, dg, db, side, info, false, nullptr); }

extern "C" int lcqp_hip_sparse_sensitivity_blocked_device(lcqp_hip_sparse_t* h, int nrhs, const double* v, double* dg, double* db, int* side, int* info, void* stream)
{ return sensitivity_entry(h, true, nrhs, v, dg, db, side, info, true, stream); }

// ---- panels with gradients on y, the dual rows of the Jacobian (DESIGN.md section 3a'''', "The sparse arm: panels with gradients on y";
// the twins: section 3a''''', "The sparse arm: panels and Jacobians into device arrays") ----
// vy == NULL: the blocked sensitivity call itself, and its bits
static int adjoint_blocked_entry(lcqp_hip_sparse* h, int nrhs, const double* vx, const double* vy, double* dg, double* db, int* side, int* info, bool dev, void* stream)
{ return guarded(g_sp_err, [&] {
    if (int rc = guard_pairs(g_sp_err, h, dev, nrhs, vx, vy, false, 0, dg, db, side, info)) return rc;
    return sp_vectors(h, true, nrhs, vx, vy, dg, db, side, info, dev, stream);
}); }

extern "C" int lcqp_hip_sparse_adjoint_blocked(lcqp_hip_sparse_t* h, int nrhs, const double* vx, const double* vy, double* dg, double* db, int* side, int* info)
{ return adjoint_blocked_entry(h, nrhs, vx, vy, dg, db, side, info, false, nullptr); }

extern "C" int lcqp_hip_sparse_adjoint_blocked_device(lcqp_hip_sparse_t* h, int nrhs, const double* vx, const double* vy, double* dg, double* db,
                                                      int* side, int* info, void* stream)
{ return adjoint_blocked_entry(h, nrhs, vx, vy, dg, db, side, info, true, stream); }

// Jg [count][n][n], Jb [count][n][m] -- duals: Jyg [count][m][n], Jyb [count][m][m] -- (or NULL), side [count][m], info [count] of the
// instances [first, first + count): the panel kernel on the unit columns (duals: the DUAL one on the unit columns of the working set), in
// chunks of work items under the staging cap.  Without a panel form (the general LDL' before lcqp_hip_sparse_set_general_panel) the vector
// kernel on uploaded unit vectors in chunks of columns -- the staging of a column is v, dg and db (duals: v, vy, dg and db) of the whole
// batch --, for the twin copied to the device from host arrays (jacobian_through_host: it waits)
static int jacobian_entry(lcqp_hip_sparse* h, bool duals, int first, int count, double* Jg, double* Jb, int* side, int* info, bool dev, void* stream)
{ return guarded(g_sp_err, [&] {
    if (int rc = guard_range(g_sp_err, h, dev, duals, first, count, Jg, Jb, side, info)) return rc;
    const size_t B = h->db.B, n = h->db.n, m = h->db.m;
    auto by_vectors = [&](double* G, double* Bd, int* sd, int* in) {
        if (!duals)
            return jacobian_by_vectors(h, sizeof(double) * B * (2 * n + m), m, first, count, G, Bd, sd, in,
                                       [&](int nc, const double* v, double* dg, double* db, int* s, int* i, float& ms) {
                return sp_sensitivity(h, nc, v, nullptr, false, dg, db, s, i, ms);
            });
        std::vector<double> zeros;
        return jacobian_duals_by_vectors(h, sizeof(double) * B * 2 * (n + m), m, first, count, G, Bd, sd, in,
                                         [&](int nc, const double* VY, double* dg, double* db, int* s, int* i, float& ms) {
            zeros.assign(B * nc * n, 0.0);
            return sp_sensitivity(h, nc, zeros.data(), VY, false, dg, db, s, i, ms);
        });
    };
    return sp_call(h, dev, stream, [&] {
        if (sp_panel(h)) return sp_panel_run(h, first, count, duals ? h->db.m : h->db.n, nullptr, Jg, Jb, side, info, nullptr, duals, dev);
        return dev ? jacobian_through_host(g_sp_err, h, m, count, duals ? m : n, Jg, Jb, side, info, by_vectors) : by_vectors(Jg, Jb, side, info);
    });
}); }

extern "C" int lcqp_hip_sparse_jacobian(lcqp_hip_sparse_t* h, int first, int count, double* Jg, double* Jb, int* side, int* info)
{ return jacobian_entry(h, false, first, count, Jg, Jb, side, info, false, nullptr); }

extern "C" int lcqp_hip_sparse_jacobian_device(lcqp_hip_sparse_t* h, int first, int count, double* Jg, double* Jb, int* side, int* info, void* stream)
{ return jacobian_entry(h, false, first, count, Jg, Jb, side, info, true, stream); }

extern "C" int lcqp_hip_sparse_jacobian_duals(lcqp_hip_sparse_t* h, int first, int count, double* Jyg, double* Jyb, int* side, int* info)
{ return jacobian_entry(h, true, first, count, Jyg, Jyb, side, info, false, nullptr); }

extern "C" int lcqp_hip_sparse_jacobian_duals_device(lcqp_hip_sparse_t* h, int first, int count, double* Jyg, double* Jyb, int* side, int* info, void* stream)
{ return jacobian_entry(h, true, first, count, Jyg, Jyb, side, info, true, stream); }

// ---- the full adjoint (DESIGN.md section 3a''''): k_sparse_sensitivity (with vy: its DUAL instantiation) on the whole batch, its results to
// the host (the device twin: to the caller's device arrays); then, on the device buffers it left, the gradients on the non-zeros that were
// asked for ----
// k_sparse_adjoint_reduce, or k_sparse_adjoint_nnz on the instances [first, first + count), into outQ (cq doubles) and outE (ce doubles)
static void sp_launch_adjoint(lcqp_hip_sparse* h, double* outQ, size_t cq, double* outE, size_t ce, int reduce, int first, int count)
{
    const SpBatch& d = h->db;
    const SensBuffers& sb = h->sn.sens;
    const SpAdjointArgs a = {d.B, d.n, d.m, d.nnzQ, d.nnzE, d.xout, d.yout, sb.dg, sb.db, sb.side, sb.info, d.Qp, d.Qi, d.Erow, d.Ei, h->valMap, outQ, outE};
    // a thread of the Q segment owns two neighbouring entries, one of the E segment one entry
    const unsigned gx = (unsigned)std::min<size_t>((std::max((cq + 1) / 2, ce) + SP_ADJ_WG - 1) / SP_ADJ_WG, 65535);
    if (reduce) hipLaunchKernelGGL(k_sparse_adjoint_reduce, dim3(gx, 2), dim3(SP_ADJ_WG), 0, h->stream, a);
    else hipLaunchKernelGGL(k_sparse_adjoint_nnz, dim3(gx, 2), dim3(SP_ADJ_WG), 0, h->stream, a, first, count);
}

// The host call: k_sparse_adjoint_reduce once, or k_sparse_adjoint_nnz per chunk of instances under the staging cap (adjoint_chunks).  dev:
// ONE launch of either kernel over the whole batch that writes the caller's arrays: no staging buffer, no chunks.  The terms are those of
// sp_adjoint_q / sp_adjoint_e either way: the same bits.
static int adjoint_entry(lcqp_hip_sparse* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                         int reduce, double* dQx, double* dAx, bool dev, void* stream)
{ return guarded(g_sp_err, [&] {
    if (int rc = guard_pairs(g_sp_err, h, dev, 1, vx, vy, true, reduce, dg, db, side, info)) return rc;
    SpBatch& d = h->db;
    const size_t nq = dQx ? (size_t)d.nnzQ : 0, ne = dAx ? (size_t)d.nnzE : 0, lead = reduce ? (size_t)1 : (size_t)d.B;
    if (dev) {
        if (!device_pointer_ok(g_sp_err, h, "dQx", dQx, sizeof(double) * lead * nq, 16) || !device_pointer_ok(g_sp_err, h, "dAx", dAx, sizeof(double) * lead * ne)) return LCQP_INVALID_ARGUMENT;
        if (dAx) if (int rc = sp_value_map(h)) return rc;
    }
    return sens_body(g_sp_err, h, dev, stream, [&](float& ms) -> int {
        if (int rc = sp_sensitivity(h, 1, vx, vy, dev, dg, db, side, info, ms)) return rc;
        if (!(nq + ne)) return 0;
        if (dev) return adjoint_device(g_sp_err, h, [&] { sp_launch_adjoint(h, dQx, lead * nq, dAx, lead * ne, reduce, 0, d.B); });
        if (dAx) if (int rc = sp_value_map(h)) return rc;
        // (+ 2: both segments start on an even offset)
        return adjoint_chunks(g_sp_err, h, nq + ne, 2, reduce, ms, [&](size_t c0, size_t cb, AdjCopy* cp) {
            const size_t cq = cb * nq, ce = cb * ne;
            double *outQ = dQx ? h->sn.adjOut : nullptr, *outE = dAx ? h->sn.adjOut + cq + (cq & 1) : nullptr;
            int ncp = 0;
            if (dQx) cp[ncp++] = {dQx + c0 * nq, outQ, cq};
            if (dAx) cp[ncp++] = {dAx + c0 * ne, outE, ce};
            sp_launch_adjoint(h, outQ, cq, outE, ce, reduce, (int)c0, (int)cb);
            return ncp;
        });
    });
}); }

extern "C" int lcqp_hip_sparse_adjoint(lcqp_hip_sparse_t* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                                       int reduce, double* dQx, double* dAx)
{ return adjoint_entry(h, vx, vy, dg, db, side, info, reduce, dQx, dAx, false, nullptr); }

extern "C" int lcqp_hip_sparse_adjoint_device(lcqp_hip_sparse_t* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                                              int reduce, double* dQx, double* dAx, void* stream)
{ return adjoint_entry(h, vx, vy, dg, db, side, info, reduce, dQx, dAx, true, stream); }

extern "C" int lcqp_hip_sparse_set_adjoint_staging(lcqp_hip_sparse_t* h, size_t bytes)
{
    return guarded(g_sp_err, [&] { return set_staging(h, bytes); });
}
