// lcqp_sparse_device.hip -- the sparse batch's device-pointer entry points that fill and read the pools: lcqp_hip_sparse_load_device,
// _update_device and _get_solution_device (include/lcqp_hip.h, DESIGN.md section 3a'''''), with their three kernels, sparse_pack -- the pack step
// the host load / update of lcqp_sparse_host.hip run behind their upload: the pack kernels are the one definition of the pool layout --, the
// scatter kernel of the device-pointer panel calls (k_sparse_scatter_panels, launched by sp_panel_run of lcqp_sparse_diff.hip) and the diagnostic
// reader lcqp_hip_sparse_read_problem.  The twins of _sensitivity, _adjoint and the panel calls are one body with their host calls, in lcqp_sparse_diff.hip;
// lcqp_sparse_batch.hpp holds what the three units share, lcqp_host_rt.hpp the hand-over around every such call (device_call) and
// _get_solution_device, which are the dense arm's too.  The model is lcqp_hip_device.hip of the dense arm.
#include "lcqp_sparse_batch.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

using namespace lcqp_rt;
using namespace lcqp_sparse;

// =================================================================================================
// device kernels: size-independent streaming kernels, no LDS tiles
// =================================================================================================
constexpr int SP_DEV_WG = 256;
// (SpPackVectors, SpPackValues: the arrays of a load / an update as the caller holds them, lcqp_sparse_batch.hpp)
__device__ __forceinline__ double sp_vec_or(const double* p, size_t i, double dflt) { return p ? p[i] : dflt; }

// ---- k_sparse_check_vectors: the value checks of lcqp_hip_sparse_load / _update over the whole range, before anything is written ----
// One workgroup per instance.  words[0]: the lowest flat index k * nComp + i with -inf in lbL or lbR; it starts as all ones, and a minimum
// does not depend on the order of the atomics.  A load with Qx: the workgroups k < nq (count, or 1 for a shared array) also form the two
// numbers lcqp_hip_sparse_load takes from the diagonal of its Hessian, diag[k] = (min_i Q_ii, max_i |Q_ii|) over the diagonal entries
// qdiag[i] (a missing one counts as 0.0), with the host's comparisons: a NaN never replaces a number, and a minimum / maximum of a set of
// numbers does not depend on the order either (the sign of a zero minimum does, and the host's expression for the ratio does not read it).
__global__ __launch_bounds__(SP_DEV_WG) void k_sparse_check_vectors(SpBatch db, int count, SpPackVectors p, const double* Qx, size_t qStride, int nq,
                                                                    unsigned long long* words, double* diag)
{
    __shared__ double wmin[SP_DEV_WG / 64], wmax[SP_DEV_WG / 64];
    const int k = blockIdx.x, t = threadIdx.x, nComp = db.nComp;
    for (int i = t; i < nComp; i += SP_DEV_WG) {
        const size_t j = (size_t)k * nComp + i;
        if (sp_vec_or(p.lbL, j, 0.0) <= -INFINITY || sp_vec_or(p.lbR, j, 0.0) <= -INFINITY) atomicMin(&words[0], (unsigned long long)j);
    }
    if (!Qx || k >= nq) return;      // (uniform over the workgroup)
    const double* q = Qx + (size_t)k * qStride;
    double dmin = INFINITY, dmax = 0.0;
    for (int i = t; i < db.n; i += SP_DEV_WG) {
        const int e = db.qdiag[i];
        const double v = e >= 0 ? q[e] : 0.0, a = fabs(v);
        if (v < dmin) dmin = v;
        if (dmax < a) dmax = a;
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        const double vmin = __shfl_down(dmin, ofs, 64), vmax = __shfl_down(dmax, ofs, 64);
        if (vmin < dmin) dmin = vmin;
        if (dmax < vmax) dmax = vmax;
    }
    if ((t & 63) == 0) { wmin[t >> 6] = dmin; wmax[t >> 6] = dmax; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < SP_DEV_WG / 64; w++) {
            if (wmin[w] < dmin) dmin = wmin[w];
            if (dmax < wmax[w]) dmax = wmax[w];
        }
        diag[2 * (size_t)k] = dmin;
        diag[2 * (size_t)k + 1] = dmax;
    }
}

// ---- k_sparse_pack_values: the caller's value arrays into SpBatch::Qx / Ex, as lcqp_hip_sparse_load leaves them ----
// blockIdx.z: the segment -- 0: Q, a straight copy of [count][nnzQ] (a shared array: stride 0); 1: E, Ex[b][e] = Ax[k][emap[e]] with emap
// the device copy of csr2csc: the caller's CSC order into the CSR order of the device --, blockIdx.y: the instance, blockIdx.x and the
// threads: the entries.  Indexed by destination: the writes are coalesced, the reads of the E segment gather through the map.  A null
// source segment is skipped.
__global__ __launch_bounds__(SP_DEV_WG) void k_sparse_pack_values(SpBatch db, int first, int count, SpPackValues v, const int* emap)
{
    const int seg = blockIdx.z;
    const double* src = seg == 0 ? v.Qx : v.Ax;
    if (!src) return;
    const int nnz = seg == 0 ? db.nnzQ : db.nnzE;
    const size_t stride = seg == 0 ? v.qStride : v.aStride;
    double* pool = seg == 0 ? db.Qx : db.Ex;
    if ((int)(blockIdx.x * SP_DEV_WG) >= nnz) return;
    for (int o = blockIdx.y; o < count; o += gridDim.y) {
        double* dst = pool + ((size_t)first + o) * nnz;
        const double* s = src + (size_t)o * stride;
        for (int e = blockIdx.x * SP_DEV_WG + threadIdx.x; e < nnz; e += gridDim.x * SP_DEV_WG) dst[e] = seg == 0 ? s[e] : s[emap[e]];
    }
}

// ---- k_sparse_pack_vectors: the vector pools of one instance per workgroup, as lcqp_hip_sparse_load (update: as lcqp_hip_sparse_update) leaves them ----
// load: every vector of the nv and mv pools zero except NV_G, NV_X0 (absent: zeros), MV_L / MV_U (the rows of A, L, R by the rule of
// fill_row_bounds) and MV_Y0 when given; lbL, lbR; a zeroed SpInfo with hasY0.  update: NV_G, NV_X0, MV_L, MV_U, MV_Y0 only when given, lbL,
// lbR and hasY0.  No element is written twice, so the kernel needs no order among its stores.
static_assert(offsetof(SpInfo, hasY0) == 8 && sizeof(SpInfo) % 4 == 0, "k_sparse_pack_vectors writes SpInfo as ints: zeros, hasY0 at [2]");
__global__ __launch_bounds__(SP_DEV_WG) void k_sparse_pack_vectors(SpBatch db, int first, SpPackVectors p, int update)
{
    const int k = blockIdx.x, t = threadIdx.x;
    const int n = db.n, m = db.m, nC = db.nC, nComp = db.nComp;
    const size_t b = (size_t)first + k;
    double* nv = db.nv + b * NV_NUM * n;
    double* mv = db.mv + b * MV_NUM * m;
    if (!update) {
        for (int v = 0; v < NV_NUM; v++) {
            if (v == NV_G || v == NV_X0) continue;
            for (int i = t; i < n; i += SP_DEV_WG) nv[(size_t)v * n + i] = 0.0;
        }
        for (int v = 0; v < MV_NUM; v++) {
            if (v == MV_L || v == MV_U || (v == MV_Y0 && p.y0)) continue;
            for (int r = t; r < m; r += SP_DEV_WG) mv[(size_t)v * m + r] = 0.0;
        }
    }
    for (int i = t; i < n; i += SP_DEV_WG) {
        const size_t j = (size_t)k * n + i;
        nv[(size_t)NV_G * n + i] = p.g[j];
        nv[(size_t)NV_X0 * n + i] = sp_vec_or(p.x0, j, 0.0);
    }
    for (int r = t; r < m; r += SP_DEV_WG) {
        double lo, hi;
        if (r < nC) { lo = sp_vec_or(p.lbA, (size_t)k * nC + r, -INFINITY); hi = sp_vec_or(p.ubA, (size_t)k * nC + r, INFINITY); }
        else if (r < nC + nComp) { const size_t j = (size_t)k * nComp + (r - nC); lo = sp_vec_or(p.lbL, j, 0.0); hi = sp_vec_or(p.ubL, j, INFINITY); }
        else { const size_t j = (size_t)k * nComp + (r - nC - nComp); lo = sp_vec_or(p.lbR, j, 0.0); hi = sp_vec_or(p.ubR, j, INFINITY); }
        mv[(size_t)MV_L * m + r] = lo;
        mv[(size_t)MV_U * m + r] = hi;
        if (p.y0) mv[(size_t)MV_Y0 * m + r] = p.y0[(size_t)k * m + r];
    }
    for (int i = t; i < nComp; i += SP_DEV_WG) {
        const size_t j = (size_t)k * nComp + i;
        db.lbL[b * nComp + i] = sp_vec_or(p.lbL, j, 0.0);
        db.lbR[b * nComp + i] = sp_vec_or(p.lbR, j, 0.0);
    }
    if (update) {
        if (t == 0) db.info[b].hasY0 = p.y0 ? 1 : 0;
        return;
    }
    int* info = reinterpret_cast<int*>(db.info + b);
    for (int e = t; e < (int)(sizeof(SpInfo) / 4); e += SP_DEV_WG) info[e] = e == 2 ? (p.y0 ? 1 : 0) : 0;
}

// ---- k_sparse_scatter_panels: one chunk of staged work items of a panel call to the caller's device arrays (the device-pointer twins of
// lcqp_hip_sparse_sensitivity_blocked / _adjoint_blocked / _jacobian / _jacobian_duals; lcqp_sparse_batch.hpp: SpScatterArgs) ----
// What the host loop of sp_panel_run does with memcpy: staged column c = i * P + k goes to row sp_panel_dest_row(..) of dg and db, or nowhere.
// 1 << shift threads (16 .. SP_DEV_WG, chosen by the host from the longer row) take one staged column: its row of dg, then its row of db,
// each lane element t, t + 2^shift, ... -- neighbouring lanes load and store neighbouring doubles.  The workgroups stride over the columns.
// No two columns of a call have one destination row, so no element is written twice and the kernel needs no order among its stores.
__global__ __launch_bounds__(SP_DEV_WG) void k_sparse_scatter_panels(SpScatterArgs a, int shift)
{
    const unsigned tpc = 1u << shift, t = threadIdx.x & (tpc - 1), cpw = SP_DEV_WG >> shift;
    const unsigned total = (unsigned)a.nItems * a.P, P = a.P;
    const size_t n = a.n, m = a.m;
    for (unsigned c = blockIdx.x * cpw + (threadIdx.x >> shift); c < total; c += gridDim.x * cpw) {
        const unsigned i = c / P, k = c - i * P;
        const long long row = sp_panel_dest_row((unsigned)a.item0 + i, k, a.npan, P, a.ncols, a.dunit, a.dunit ? a.rowpos[c] : 0);
        if (row < 0) continue;
        const double* sg = a.sg + (size_t)c * n;
        double* dg = a.dg + (size_t)row * n;
        for (size_t e = t; e < n; e += tpc) dg[e] = sg[e];
        if (!a.db) continue;
        const double* sb = a.sb + (size_t)c * m;
        double* db = a.db + (size_t)row * m;
        for (size_t e = t; e < m; e += tpc) db[e] = sb[e];
    }
}

// =================================================================================================
// host side
// =================================================================================================
#define g_sp_err sparse_err()      // the error slot of the sparse arm (thread_local, lcqp_sparse_host.hip)

int sparse_scatter_panels(lcqp_hip_sparse* h, const SpScatterArgs& a)
{
    const size_t total = (size_t)a.nItems * a.P, longer = std::max(a.n, a.db ? a.m : 0);
    if (!total) return 0;
    if (total > 0xFFFFFFFFull) { g_sp_err = "scatter: more staged columns in one chunk than the kernel counts"; return LCQP_HIP_UNSUPPORTED; }
    int shift = 4;
    while ((1 << shift) < SP_DEV_WG && ((size_t)1 << shift) < longer) shift++;
    const size_t cpw = SP_DEV_WG >> shift;      // staged columns per workgroup and turn
    const unsigned gx = (unsigned)std::min<size_t>((total + cpw - 1) / cpw, (size_t)std::max(h->cus, 1) * 16);
    hipLaunchKernelGGL(k_sparse_scatter_panels, dim3(gx), dim3(SP_DEV_WG), 0, h->stream, a, shift);
    HIPCHK(g_sp_err, hipGetLastError());
    return 0;
}

int sparse_pack_values(lcqp_hip_sparse* h, int first, int count, const SpPackValues& m)
{
    const SpBatch& d = h->db;
    if (!m.Qx && !m.Ax) return 0;
    const int most = std::max(m.Qx ? d.nnzQ : 0, m.Ax ? d.nnzE : 0);
    const unsigned gx = (unsigned)std::min<size_t>(((size_t)most + 4 * SP_DEV_WG - 1) / (4 * SP_DEV_WG), 4096);      // four entries per thread
    hipLaunchKernelGGL(k_sparse_pack_values, dim3(std::max(gx, 1u), std::min(count, 65535), 2), dim3(SP_DEV_WG), 0, h->stream, d, first, count, m,
                       (const int*)h->valMap);
    HIPCHK(g_sp_err, hipGetLastError());
    return 0;
}

int sparse_pack(lcqp_hip_sparse* h, int first, int count, const SpPackVectors& v, const SpPackValues& m, bool update)
{
    const SpBatch& d = h->db;
    if (!update) if (int rc = sparse_pack_values(h, first, count, m)) return rc;
    hipLaunchKernelGGL(k_sparse_pack_vectors, dim3(count), dim3(SP_DEV_WG), 0, h->stream, d, first, v, update ? 1 : 0);
    HIPCHK(g_sp_err, hipGetLastError());
    return 0;
}

// the status word of k_sparse_check_vectors and the diagonal pairs of a load behind it: [2] words, then [B][2] doubles
static int sp_check_buffer(lcqp_hip_sparse* h)
{
    if (h->devChk) return 0;
    return h->mem.alloc(g_sp_err, h->devChk, 2 + 2 * (size_t)h->db.B) ? 0 : LCQP_HIP_ERROR;
}

static bool sp_vectors_ok(const lcqp_hip_sparse* h, size_t count, const SpPackVectors& p)
{
    const SpBatch& d = h->db;
    const size_t dbl = sizeof(double) * count;
    return device_pointer_ok(g_sp_err, h, "g", p.g, dbl * d.n) && device_pointer_ok(g_sp_err, h, "lbA", p.lbA, dbl * d.nC) &&
           device_pointer_ok(g_sp_err, h, "ubA", p.ubA, dbl * d.nC) && device_pointer_ok(g_sp_err, h, "lbL", p.lbL, dbl * d.nComp) &&
           device_pointer_ok(g_sp_err, h, "ubL", p.ubL, dbl * d.nComp) && device_pointer_ok(g_sp_err, h, "lbR", p.lbR, dbl * d.nComp) &&
           device_pointer_ok(g_sp_err, h, "ubR", p.ubR, dbl * d.nComp) && device_pointer_ok(g_sp_err, h, "x0", p.x0, dbl * d.n) &&
           device_pointer_ok(g_sp_err, h, "y0", p.y0, dbl * d.m);
}

// k_sparse_check_vectors on the range and its results back on the host: the one host synchronisation of a load / an update.  out: the word,
// a pad, then nq pairs (min Q_ii, max |Q_ii|) when Qx is given.  Returns 0 with out filled.
static int sp_check_vectors(lcqp_hip_sparse* h, int count, const SpPackVectors& p, const double* Qx, size_t qStride, int nq, std::vector<unsigned long long>& out)
{
    const SpBatch& d = h->db;
    if (int rc = sp_check_buffer(h)) return rc;
    out.assign(2 + 2 * (size_t)(Qx ? nq : 0), 0);
    HIPCHK(g_sp_err, hipMemsetAsync(h->devChk, 0xFF, 2 * sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_sparse_check_vectors, dim3(count), dim3(SP_DEV_WG), 0, h->stream, d, count, p, Qx, qStride, nq, h->devChk,
                       reinterpret_cast<double*>(h->devChk + 2));
    HIPCHK(g_sp_err, hipGetLastError());
    HIPCHK(g_sp_err, hipMemcpyAsync(out.data(), h->devChk, sizeof(unsigned long long) * out.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(g_sp_err, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int lcqp_hip_sparse_load_device(lcqp_hip_sparse_t* h, int first, int count, int shared,
                                           const double* Qx, const double* g, const double* Ax,
                                           const double* lbA, const double* ubA, const double* lbL, const double* ubL,
                                           const double* lbR, const double* ubR, const double* x0, const double* y0, void* stream)
{ return guarded(g_sp_err, [&] {
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    SpBatch& d = h->db;
    if (first < 0 || count <= 0 || first > d.B - count || (shared & ~3)) return LCQP_INVALID_ARGUMENT;
    // a value array that is not handed over stays as the pool holds it: every instance of the range must hold a problem then
    bool held = true;
    for (int k = 0; k < count; k++) held = held && h->rs.filled[(size_t)first + k];
    if ((!Qx || !Ax) && !held) return LCQP_INVALID_ARGUMENT;
    if (!g) return LCQP_INVALID_OBJECTIVE_LINEAR_TERM;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    const bool oneQ = shared & 1, oneA = shared & 2;
    const SpPackVectors pv = {g, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0};
    const SpPackValues pm = {Qx, Ax, oneQ ? 0 : (size_t)d.nnzQ, oneA ? 0 : (size_t)d.nnzE};
    if (!device_pointer_ok(g_sp_err, h, "Qx", Qx, sizeof(double) * (oneQ ? 1 : (size_t)count) * d.nnzQ) ||
        !device_pointer_ok(g_sp_err, h, "Ax", Ax, sizeof(double) * (oneA ? 1 : (size_t)count) * d.nnzE) || !sp_vectors_ok(h, count, pv)) return LCQP_INVALID_ARGUMENT;
    if (Ax) if (int rc = sp_value_map(h)) return rc;
    return device_call(g_sp_err, h, stream, [&] {
        const int nq = oneQ ? 1 : count;
        std::vector<unsigned long long> chk;
        if (int rc = sp_check_vectors(h, count, pv, Qx, pm.qStride, nq, chk)) return rc;
        if (chk[0] != ~0ull) return LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND;
        // the host state of lcqp_hip_sparse_load: the setup mark, the lbL / lbR flags, the diagonal ratios, the ordering
        h->rs.invalidate();
        load_bound_flags(d, h->loaded, first, lbL, lbR);
        for (int k = 0; k < count; k++) {
            h->rs.filled[(size_t)first + k] = 1;
            if (!Qx) continue;
            double pair[2];
            memcpy(pair, chk.data() + 2 + 2 * (size_t)(oneQ ? 0 : k), sizeof(pair));
            const double dmin = pair[0], dmax = pair[1];
            h->diagRatio[(size_t)first + k] = (dmax > 0.0 && dmin > 0.0) ? dmin / dmax : 0.0;
        }
        h->loaded = true;
        sp_choose_ordering(h);
        return sparse_pack(h, first, count, pv, pm, false);
    });
}); }

extern "C" int lcqp_hip_sparse_update_device(lcqp_hip_sparse_t* h, int first, int count, const double* g,
                                             const double* lbA, const double* ubA, const double* lbL, const double* ubL,
                                             const double* lbR, const double* ubR, const double* x0, const double* y0, void* stream)
{ return guarded(g_sp_err, [&] {
    if (int rc = check_update(g_sp_err, h, first, count, g)) return rc;      // (the values are checked on the device)
    SpBatch& d = h->db;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    const SpPackVectors pv = {g, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0};
    if (!sp_vectors_ok(h, count, pv)) return LCQP_INVALID_ARGUMENT;
    // no drain of the handle's stream: the kernels below are behind a run in flight on the same stream
    return device_call(g_sp_err, h, stream, [&] {
        std::vector<unsigned long long> chk;
        if (int rc = sp_check_vectors(h, count, pv, nullptr, 0, 0, chk)) return rc;
        if (chk[0] != ~0ull) return LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND;
        d.hasLbL |= lbL ? 1 : 0; d.hasLbR |= lbR ? 1 : 0;
        return sparse_pack(h, first, count, pv, SpPackValues{}, true);
    });
}); }

// New values of the matrices for instances [first, first + count) from device arrays of the caller: lcqp_hip_sparse_update_values behind
// the hand-over of the streams.  shared: the bits of lcqp_hip_sparse_load_device -- 1: one Qx for the range, 2: one Ax.  With Qx the
// diagonal pairs come from k_sparse_check_vectors over an empty set of vectors (its lbL / lbR half reads the zero default): the one host
// synchronisation of the call.
extern "C" int lcqp_hip_sparse_update_values_device(lcqp_hip_sparse_t* h, int first, int count, int shared, const double* Qx, const double* Ax,
                                                    void* stream)
{ return guarded(g_sp_err, [&] {
    if (int rc = check_update_values(h, first, count, Qx, Ax)) return rc;
    if (shared & ~3) return LCQP_INVALID_ARGUMENT;
    const SpBatch& d = h->db;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    const bool oneQ = shared & 1, oneA = shared & 2;
    const SpPackValues pm = {Qx, Ax, oneQ ? 0 : (size_t)d.nnzQ, oneA ? 0 : (size_t)d.nnzE};
    if (!device_pointer_ok(g_sp_err, h, "Qx", Qx, sizeof(double) * (oneQ ? 1 : (size_t)count) * d.nnzQ) ||
        !device_pointer_ok(g_sp_err, h, "Ax", Ax, sizeof(double) * (oneA ? 1 : (size_t)count) * d.nnzE)) return LCQP_INVALID_ARGUMENT;
    if (Ax) if (int rc = sp_value_map(h)) return rc;
    return device_call(g_sp_err, h, stream, [&] {
        std::vector<unsigned long long> chk;
        if (Qx) if (int rc = sp_check_vectors(h, count, SpPackVectors{}, Qx, pm.qStride, oneQ ? 1 : count, chk)) return rc;
        h->rs.matrices_changed();
        if (Qx)
            for (int k = 0; k < count; k++) {
                double pair[2];
                memcpy(pair, chk.data() + 2 + 2 * (size_t)(oneQ ? 0 : k), sizeof(pair));
                const double dmin = pair[0], dmax = pair[1];
                h->diagRatio[(size_t)first + k] = (dmax > 0.0 && dmin > 0.0) ? dmin / dmax : 0.0;
            }
        sp_choose_ordering(h);
        return sparse_pack_values(h, first, count, pm);
    });
}); }

extern "C" int lcqp_hip_sparse_get_solution_device(lcqp_hip_sparse_t* h, double* x, double* y, lcqp_stats_t* stats, void* stream)
{
    return guarded(g_sp_err, [&] { return get_solution_device(g_sp_err, h, h ? h->db.m : 0, x, y, stats, stream); });
}

// ---- test and diagnostic entry point: the problem of one instance as the pools hold it (host buffers, synchronous, launches nothing) ----
extern "C" int lcqp_hip_sparse_read_problem(lcqp_hip_sparse_t* h, int instance, double* Qx, double* Ax, double* g,
                                            double* lE, double* uE, double* lbL, double* lbR, double* x0, double* y0, int* hasY0)
{ return guarded(g_sp_err, [&] {
    if (!h || instance < 0 || instance >= h->db.B) return LCQP_INVALID_ARGUMENT;
    const SpBatch& d = h->db;
    if (int rc = synchronize(g_sp_err, h)) return rc;
    const size_t b = instance, n = d.n, m = d.m, nK = d.nComp;
    const double *nv = d.nv + b * NV_NUM * n, *mv = d.mv + b * MV_NUM * m;
    if (int rc = read_back(g_sp_err, Qx, d.Qx + b * d.nnzQ, d.nnzQ)) return rc;
    if (Ax) {      // Ex is in the CSR order of the device: entry e is entry csr2csc[e] of the caller's CSC array
        std::vector<double> ex(d.nnzE);
        if (int rc = read_back(g_sp_err, ex.data(), d.Ex + b * d.nnzE, d.nnzE)) return rc;
        for (int e = 0; e < d.nnzE; e++) Ax[h->csr2csc[e]] = ex[e];
    }
    if (int rc = read_back(g_sp_err, g, nv + (size_t)NV_G * n, n)) return rc;
    if (int rc = read_back(g_sp_err, x0, nv + (size_t)NV_X0 * n, n)) return rc;
    if (int rc = read_back(g_sp_err, lE, mv + (size_t)MV_L * m, m)) return rc;
    if (int rc = read_back(g_sp_err, uE, mv + (size_t)MV_U * m, m)) return rc;
    if (int rc = read_back(g_sp_err, y0, mv + (size_t)MV_Y0 * m, m)) return rc;
    if (int rc = read_back(g_sp_err, lbL, d.lbL + b * nK, nK)) return rc;
    if (int rc = read_back(g_sp_err, lbR, d.lbR + b * nK, nK)) return rc;
    if (int rc = read_back(g_sp_err, hasY0, &d.info[b].hasY0, 1)) return rc;
    return 0;
}); }

// ---- test and diagnostic entry point: the ADMM state of one instance as the pools hold it (host buffers, synchronous, launches nothing) ----
// The weights, the stacked bounds and the iterates (sp_prepare_vectors, sp_qp_begin, sp_ph_round, sp_admm in lcqp_sparse_solver.hpp).  The polish
// writes none of xa, ya, za, so they are those of the last QP that ran ADMM.
extern "C" int lcqp_hip_sparse_read_admm(lcqp_hip_sparse_t* h, int instance, int dims[2], double scal[3], double* rhov, double* l, double* u,
                                         double* xa, double* ya, double* za)
{ return guarded(g_sp_err, [&] {
    if (!h || instance < 0 || instance >= h->db.B) return LCQP_INVALID_ARGUMENT;
    if (!h->rs.setupValid) return LCQP_LCQPOBJECT_NOT_SETUP;
    const SpBatch& d = h->db;
    if (int rc = synchronize(g_sp_err, h)) return rc;
    const size_t b = instance, n = d.n, m = d.m;
    SpInfo info;
    HIPCHK(g_sp_err, hipMemcpy(&info, d.info + b, sizeof(SpInfo), hipMemcpyDeviceToHost));
    if (dims) { dims[0] = d.n; dims[1] = d.m; }
    if (scal) { scal[0] = info.sigma; scal[1] = d.opt.admmRho * info.scale; scal[2] = info.scale; }
    const double *nv = d.nv + b * NV_NUM * n, *mv = d.mv + b * MV_NUM * m;
    if (int rc = read_back(g_sp_err, rhov, mv + (size_t)MV_RHOV * m, m)) return rc;
    if (int rc = read_back(g_sp_err, l, mv + (size_t)MV_L * m, m)) return rc;
    if (int rc = read_back(g_sp_err, u, mv + (size_t)MV_U * m, m)) return rc;
    if (int rc = read_back(g_sp_err, xa, nv + (size_t)NV_XA * n, n)) return rc;
    if (int rc = read_back(g_sp_err, ya, mv + (size_t)MV_YA * m, m)) return rc;
    if (int rc = read_back(g_sp_err, za, mv + (size_t)MV_ZA * m, m)) return rc;
    return 0;
}); }

// ---- test and diagnostic entry point: the polish state of one instance as the pools hold it (host buffers, synchronous, launches nothing) ----
// The record of the phase machine (SpState), the instance's SpInfo and the vectors the trials of the polish read and write (sp_polish_begin,
// sp_ph_trial, sp_ph_factor, sp_ph_correct, sp_ph_qpend in lcqp_sparse_solver.hpp), as the last run / resolve left them.
extern "C" int lcqp_hip_sparse_read_polish(lcqp_hip_sparse_t* h, int instance, int dims[15], double scal[11], double* V, double* M, int* I)
{ return guarded(g_sp_err, [&] {
    if (!h || instance < 0 || instance >= h->db.B) return LCQP_INVALID_ARGUMENT;
    if (!h->rs.setupValid) return LCQP_LCQPOBJECT_NOT_SETUP;
    const SpBatch& d = h->db;
    if (int rc = synchronize(g_sp_err, h)) return rc;
    const size_t b = instance, n = d.n, m = d.m;
    SpInfo info;
    SpState S;
    HIPCHK(g_sp_err, hipMemcpy(&info, d.info + b, sizeof(SpInfo), hipMemcpyDeviceToHost));
    HIPCHK(g_sp_err, hipMemcpy(&S, d.state + b, sizeof(SpState), hipMemcpyDeviceToHost));
    if (dims) {
        const int v[15] = {d.n, d.m, S.trial, S.reuse, S.fact_valid, S.nrefine, S.round, S.rc, info.stfValid, info.bigReg, info.haveSolution,
                           d.lightOK, d.kb, d.general, d.G};
        memcpy(dims, v, sizeof(v));
    }
    if (scal) {
        const double v[11] = {S.gs, S.ytol, S.dpUsed, S.d2Used, S.xinf, info.delta, info.deltaS, info.delta2, info.delta2S, info.e1max, info.scale};
        memcpy(scal, v, sizeof(v));
    }
    const double *nv = d.nv + b * NV_NUM * n, *mv = d.mv + b * MV_NUM * m;
    const int* mi = d.mi + b * MI_NUM * m;
    static const int vsel[5] = {NV_XT, NV_R1, NV_TMP, NV_GK, NV_XQ}, msel[5] = {MV_YT, MV_EX, MV_L, MV_U, MV_YQ}, isel[4] = {MI_ST, MI_STT, MI_STF, MI_NEW};
    for (int k = 0; k < 5; k++) if (int rc = read_back(g_sp_err, V ? V + (size_t)k * n : nullptr, nv + (size_t)vsel[k] * n, n)) return rc;
    for (int k = 0; k < 5; k++) if (int rc = read_back(g_sp_err, M ? M + (size_t)k * m : nullptr, mv + (size_t)msel[k] * m, m)) return rc;
    for (int k = 0; k < 4; k++) if (int rc = read_back(g_sp_err, I ? I + (size_t)k * m : nullptr, mi + (size_t)isel[k] * m, m)) return rc;
    return 0;
}); }
