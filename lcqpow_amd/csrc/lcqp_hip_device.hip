// lcqp_hip_device.hip -- the dense batch's device-pointer entry points that fill and read the pools: lcqp_hip_batch_load_device,
// _update_device, _update_matrices_device and _get_solution_device (include/lcqp_hip.h, DESIGN.md section 3a'''''), with their three kernels, and dense_pack, the pack step
// the host load / update of lcqp_hip.hip run behind their upload: the pack kernels are the one definition of the pool layout.  The twins of
// the sensitivity, Jacobian and adjoint calls are one body with their host calls, in lcqp_hip_diff.hip (k_pack_dual_rows here is theirs); lcqp_hip_batch.hpp holds what the two units share, lcqp_host_rt.hpp the hand-over
// around every such call (device_call) and _get_solution_device, which are the sparse arm's too.
#include "lcqp_hip_batch.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

using namespace lcqp;
using namespace lcqp_rt;

// =================================================================================================
// device kernels: size-independent streaming kernels, no LDS tiles
// =================================================================================================
// (PackVectors, PackMatrices: the arrays of a load / an update as the caller holds them, lcqp_hip_batch.hpp)
__device__ __forceinline__ double vec_or(const double* p, size_t i, double dflt) { return p ? p[i] : dflt; }

// ---- k_check_vectors: the value checks of lcqp_hip_batch_load / _update over the whole range, before anything is written ----
// One workgroup per instance.  words[0]: the lowest flat index k * nComp + i with -inf in lbL or lbR; words[1] (update): the lowest
// (k * n + i) * 2 + (1: gains, 0: loses) of a variable whose box bound appears or disappears against the list the load left (boxidx,
// nfin: ascending, so a binary search); both start as all ones, and a minimum does not depend on the order of the atomics.  A load
// writes the box flags of its variables to flags [count][n] instead (the host keeps them for later host updates).
__global__ __launch_bounds__(WG) void k_check_vectors(DevBatch db, int first, int count, PackVectors p, int update, unsigned long long* words,
                                                      unsigned char* flags)
{
    const int k = blockIdx.x, t = threadIdx.x, n = db.n, nComp = db.nComp;
    const size_t b = (size_t)first + k;
    for (int i = t; i < nComp; i += WG) {
        const size_t j = (size_t)k * nComp + i;
        if (vec_or(p.lbL, j, 0.0) <= -INFINITY || vec_or(p.lbR, j, 0.0) <= -INFINITY) atomicMin(&words[0], (unsigned long long)j);
    }
    const int* boxidx = db.boxidx + b * db.np;
    const int nfin = update ? db.info[b].nfin : 0;
    for (int i = t; i < n; i += WG) {
        const size_t j = (size_t)k * n + i;
        const bool fin = isfinite(vec_or(p.lb, j, -INFINITY)) || isfinite(vec_or(p.ub, j, INFINITY));
        if (!update) { flags[j] = fin ? 1 : 0; continue; }
        int lo = 0, hi = nfin;      // the first entry of boxidx that is not below i
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (boxidx[mid] < i) lo = mid + 1; else hi = mid; }
        const bool was = lo < nfin && boxidx[lo] == i;
        if (fin != was) atomicMin(&words[1], (unsigned long long)j * 2 + (fin ? 1 : 0));
    }
}

// ---- k_pack_vectors: the vector pools of one instance per workgroup, as lcqp_hip_batch_load (update: as lcqp_hip_batch_update) leaves them ----
// load: every vector of the nv and mv pools zero, V_G / V_LB / V_UB / V_X0 (padding: 0 / -inf / +inf / 0), M_L / M_U of the rows of A, L, R
// (the box rows behind them follow on the device: k_prepare), lbL, lbR, y0 when given, the ascending list of the box-bounded variables and
// a zeroed InstInfo with mE, nfin, hasY0.  No element is written twice, so the kernel needs no order among its stores.
static_assert(offsetof(InstInfo, mE) == 0 && offsetof(InstInfo, nfin) == 4 && offsetof(InstInfo, hasY0) == 8 && sizeof(InstInfo) % 4 == 0,
              "k_pack_vectors writes InstInfo as ints: mE, nfin, hasY0, zeros");
__global__ __launch_bounds__(WG) void k_pack_vectors(DevBatch db, int first, int count, PackVectors p, int update)
{
    __shared__ int wsum[WG / 64];
    const int k = blockIdx.x, t = threadIdx.x;
    const int n = db.n, np = db.np, nC = db.nC, nComp = db.nComp, mA = db.mA, mE = db.mEcap, nd = db.nd;
    const size_t b = (size_t)first + k;
    double* nv = db.nv + b * V_NUM * np;
    double* mv = db.mv + b * M_NUM * mE;
    if (!update) {
        for (int v = 0; v < V_NUM; v++) {
            if (v == V_G || v == V_LB || v == V_UB || v == V_X0) continue;
            for (int i = t; i < np; i += WG) nv[(size_t)v * np + i] = 0.0;
        }
        for (int v = 0; v < M_NUM; v++) {
            if (v == M_L || v == M_U) continue;
            for (int r = t; r < mE; r += WG) mv[(size_t)v * mE + r] = 0.0;
        }
    }
    for (int i = t; i < np; i += WG) {
        const bool in = i < n;
        const size_t j = (size_t)k * n + i;
        nv[(size_t)V_G * np + i] = in ? p.g[j] : 0.0;
        nv[(size_t)V_LB * np + i] = in ? vec_or(p.lb, j, -INFINITY) : -INFINITY;
        nv[(size_t)V_UB * np + i] = in ? vec_or(p.ub, j, INFINITY) : INFINITY;
        nv[(size_t)V_X0 * np + i] = in ? vec_or(p.x0, j, 0.0) : 0.0;
    }
    for (int r = t; r < (update ? mA : mE); r += WG) {
        double lo = 0.0, hi = 0.0;
        if (r < nC) { lo = vec_or(p.lbA, (size_t)k * nC + r, -INFINITY); hi = vec_or(p.ubA, (size_t)k * nC + r, INFINITY); }
        else if (r < nC + nComp) { const size_t j = (size_t)k * nComp + (r - nC); lo = vec_or(p.lbL, j, 0.0); hi = vec_or(p.ubL, j, INFINITY); }
        else if (r < mA) { const size_t j = (size_t)k * nComp + (r - nC - nComp); lo = vec_or(p.lbR, j, 0.0); hi = vec_or(p.ubR, j, INFINITY); }
        mv[(size_t)M_L * mE + r] = lo;
        mv[(size_t)M_U * mE + r] = hi;
    }
    for (int i = t; i < nComp; i += WG) {
        const size_t j = (size_t)k * nComp + i;
        db.lbL[b * nComp + i] = vec_or(p.lbL, j, 0.0);
        db.lbR[b * nComp + i] = vec_or(p.lbR, j, 0.0);
    }
    if (p.y0) for (int i = t; i < nd; i += WG) db.y0[b * nd + i] = p.y0[(size_t)k * nd + i];
    if (update) {
        if (t == 0) db.info[b].hasY0 = p.y0 ? 1 : 0;
        return;
    }
    // the box-bounded variables in ascending order: thread t owns the variables [t * per, (t + 1) * per), an exclusive prefix sum of the
    // counts over the workgroup gives its place in the list
    const int per = (np + WG - 1) / WG, i0 = t * per, i1 = min(n, i0 + per);
    int mine = 0;
    for (int i = i0; i < i1; i++) {
        const size_t j = (size_t)k * n + i;
        mine += (isfinite(vec_or(p.lb, j, -INFINITY)) || isfinite(vec_or(p.ub, j, INFINITY))) ? 1 : 0;
    }
    int incl = mine;
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int ofs = 1; ofs < 64; ofs <<= 1) { const int v = __shfl_up(incl, ofs, 64); if (lane >= ofs) incl += v; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int at = incl - mine, nfin = 0;
    for (int w = 0; w < WG / 64; w++) { if (w < wave) at += wsum[w]; nfin += wsum[w]; }
    int* boxidx = db.boxidx + b * np;
    for (int i = i0; i < i1; i++) {
        const size_t j = (size_t)k * n + i;
        if (isfinite(vec_or(p.lb, j, -INFINITY)) || isfinite(vec_or(p.ub, j, INFINITY))) boxidx[at++] = i;
    }
    for (int e = nfin + t; e < np; e += WG) boxidx[e] = 0;
    int* info = reinterpret_cast<int*>(db.info + b);
    for (int e = t; e < (int)(sizeof(InstInfo) / 4); e += WG) info[e] = e == 0 ? mA + nfin : (e == 1 ? nfin : (e == 2 ? (p.y0 ? 1 : 0) : 0));
}

// ---- k_pack_matrices: caller rows [rows][n] into the padded pools, as lcqp_hip_batch_load leaves them ----
// blockIdx.z: the segment -- Q (np rows of the Q pool, zero behind column and row n), A, L, R (their rows of E = [A; L; R; box rows],
// zero behind column n) and the box rows of E up to mEcap (zero; k_prepare writes them) --, blockIdx.y: the instance, blockIdx.x and the
// threads: the segment's 16-byte pieces.  Indexed by destination: a thread owns an aligned pair of a padded row (np is even, the pools
// start on 256-byte boundaries) and reads its two source elements one by one -- rows of an odd n are not 16-byte aligned.
__global__ __launch_bounds__(WG) void k_pack_matrices(DevBatch db, int first, int count, PackMatrices m)
{
    const int seg = blockIdx.z, n = db.n, np = db.np, half = np / 2;
    const double* src = seg < 4 ? m.src[seg] : nullptr;
    if (seg < 4 && !src) return;
    const int rowOff = seg <= 1 ? 0 : (seg == 2 ? db.nC : (seg == 3 ? db.nC + db.nComp : db.mA));
    const int srcRows = seg == 0 ? n : (seg == 1 ? db.nC : (seg == 4 ? 0 : db.nComp));
    const int dstRows = seg == 0 ? np : (seg == 4 ? db.mEcap - db.mA : srcRows);
    const int pieces = dstRows * half;
    if ((int)(blockIdx.x * WG) >= pieces) return;
    for (int o = blockIdx.y; o < count; o += gridDim.y) {
        const size_t b = (size_t)first + o;
        double* dst = seg == 0 ? db.Q + b * np * np : db.E + (b * db.mEcap + rowOff) * np;
        const double* s = src ? src + (size_t)o * m.stride[seg] : nullptr;
        for (int pc = blockIdx.x * WG + threadIdx.x; pc < pieces; pc += gridDim.x * WG) {
            const int r = pc / half, j = 2 * (pc - r * half);
            double v0 = 0.0, v1 = 0.0;
            if (r < srcRows) {
                const double* row = s + (size_t)r * n;
                if (j < n) v0 = row[j];
                if (j + 1 < n) v1 = row[j + 1];
            }
            *reinterpret_cast<double2*>(dst + (size_t)r * np + j) = double2{v0, v1};
        }
    }
}

// ---- k_pack_dual_rows: the staged rows of a dual Jacobian to their rows of the caller's arrays (lcqp_hip_batch_jacobian_duals_device) ----
// blockIdx.x: the staged row j < capS, blockIdx.y (strided): the instance o of the chunk.  rowpos [count][capS]: the dual position r < nd of
// staged row j, or -1 -- no two staged rows of an instance share a position, so no element is written twice.  dg [count][capS][np] and
// db [count][capS][ldb] as k_sensitivity_blk left them; Jyg [count][nd][n], Jyb [count][nd][nd] or null.
__global__ __launch_bounds__(WG) void k_pack_dual_rows(int count, int capS, int n, int np, int nd, int ldb, const double* dg, const double* dbs,
                                                       const int* rowpos, double* Jyg, double* Jyb)
{
    const int j = blockIdx.x, t = threadIdx.x;
    for (int o = blockIdx.y; o < count; o += gridDim.y) {
        const size_t row = (size_t)o * capS + j;
        const int r = rowpos[row];
        if (r < 0 || r >= nd) continue;
        double* og = Jyg + ((size_t)o * nd + r) * n;
        for (int i = t; i < n; i += WG) og[i] = dg[row * np + i];
        if (!Jyb) continue;
        double* ob = Jyb + ((size_t)o * nd + r) * nd;
        for (int i = t; i < nd; i += WG) ob[i] = dbs[row * ldb + i];
    }
}

// =================================================================================================
// host side
// =================================================================================================
void launch_pack_dual_rows(const DevBatch& d, hipStream_t s, int count, int ldb, const double* dg, const double* db, const int* rowpos,
                           double* Jyg, double* Jyb)
{
    hipLaunchKernelGGL(k_pack_dual_rows, dim3(d.capS, std::min(count, 65535)), dim3(WG), 0, s, count, d.capS, d.n, d.np, d.nd, ldb, dg, db, rowpos, Jyg, Jyb);
}

#define g_err dense_err()      // the error slot of the dense arm (thread_local, lcqp_hip.hip)

// k_pack_matrices on the range.  boxRows: with the segment that zeroes the box rows of E, as a load leaves them before k_prepare writes
// them; a matrix-only update leaves that segment alone -- the rows k_prepare rewrites are rewritten anyway, the ones behind them are
// still the zeros of the load
int dense_pack_matrices(lcqp_hip_batch* h, int first, int count, const PackMatrices& m, bool boxRows)
{
    const DevBatch& d = h->db;
    const int half = d.np / 2, mostRows = std::max(d.np, std::max(d.nC, std::max(d.nComp, d.mEcap - d.mA)));
    const unsigned gx = (unsigned)std::min<size_t>(((size_t)mostRows * half + 4 * WG - 1) / (4 * WG), 4096);      // four pieces per thread
    hipLaunchKernelGGL(k_pack_matrices, dim3(gx, std::min(count, 65535), boxRows ? 5 : 4), dim3(WG), 0, h->stream, d, first, count, m);
    HIPCHK(g_err, hipGetLastError());
    return 0;
}

int dense_pack(lcqp_hip_batch* h, int first, int count, const PackVectors& v, const PackMatrices& m, bool update)
{
    const DevBatch& d = h->db;
    // (a batch that holds one set of matrices has one block per matrix pool: its loads pack instance 0 by themselves, never a range)
    if (!update && !d.shared) if (int rc = dense_pack_matrices(h, first, count, m, true)) return rc;
    hipLaunchKernelGGL(k_pack_vectors, dim3(count), dim3(WG), 0, h->stream, d, first, count, v, update ? 1 : 0);
    HIPCHK(g_err, hipGetLastError());
    return 0;
}

// lcqp_hip_batch_update_matrices and its device twin up to the first device call: the checks, in this order.  Nothing is written when
// one of them fails.
int check_update_matrices(lcqp_hip_batch* h, int first, int count, const double* Q, const double* L, const double* R, const double* A)
{
    if (!Q && !L && !R && !A) return LCQP_INVALID_ARGUMENT;
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (first < 0 || count <= 0 || first > h->db.B - count) return LCQP_INVALID_ARGUMENT;
    for (int k = 0; k < count; k++) if (!h->rs.filled[(size_t)first + k]) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (!Q && !(A && h->db.nC) && !((L || R) && h->db.nComp)) return LCQP_INVALID_ARGUMENT;      // only matrices this batch has no rows of
    if (h->db.shared && (first != 0 || count != h->db.B)) {
        dense_err() = "update_matrices: this batch holds one set of matrices; they change for the whole batch (first = 0, count = batch)";
        return LCQP_INVALID_ARGUMENT;
    }
    return 0;
}

// the status words (and, for a load, the box flags behind them) of k_check_vectors: [2] words, then [B][n] bytes
static int check_buffer(lcqp_hip_batch* h)
{
    if (h->devChk) return 0;
    const size_t words = 2 + ((size_t)h->db.B * h->db.n + 7) / 8;
    return h->mem.alloc(g_err, h->devChk, words) ? 0 : LCQP_HIP_ERROR;
}

static bool vectors_ok(const lcqp_hip_batch* h, size_t count, const PackVectors& p)
{
    const DevBatch& d = h->db;
    const size_t dbl = sizeof(double) * count;
    return device_pointer_ok(g_err, h, "g", p.g, dbl * d.n) && device_pointer_ok(g_err, h, "lbL", p.lbL, dbl * d.nComp) &&
           device_pointer_ok(g_err, h, "ubL", p.ubL, dbl * d.nComp) && device_pointer_ok(g_err, h, "lbR", p.lbR, dbl * d.nComp) &&
           device_pointer_ok(g_err, h, "ubR", p.ubR, dbl * d.nComp) && device_pointer_ok(g_err, h, "lbA", p.lbA, dbl * d.nC) &&
           device_pointer_ok(g_err, h, "ubA", p.ubA, dbl * d.nC) && device_pointer_ok(g_err, h, "lb", p.lb, dbl * d.n) &&
           device_pointer_ok(g_err, h, "ub", p.ub, dbl * d.n) && device_pointer_ok(g_err, h, "x0", p.x0, dbl * d.n) &&
           device_pointer_ok(g_err, h, "y0", p.y0, dbl * d.nd);
}

// k_check_vectors on the range and its words back on the host: the one host synchronisation of a load / an update.  flags: where a load
// wants the box flags of its variables ([count][n]), null for an update.  Returns 0 with words[] filled.
static int check_vectors(lcqp_hip_batch* h, int first, int count, const PackVectors& p, bool update, unsigned long long words[2], char* flags)
{
    const DevBatch& d = h->db;
    if (int rc = check_buffer(h)) return rc;
    unsigned char* dflags = reinterpret_cast<unsigned char*>(h->devChk + 2);
    HIPCHK(g_err, hipMemsetAsync(h->devChk, 0xFF, 2 * sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_check_vectors, dim3(count), dim3(WG), 0, h->stream, d, first, count, p, update ? 1 : 0, h->devChk, dflags);
    HIPCHK(g_err, hipGetLastError());
    HIPCHK(g_err, hipMemcpyAsync(words, h->devChk, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (flags) HIPCHK(g_err, hipMemcpyAsync(flags, dflags, (size_t)count * d.n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(g_err, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int lcqp_hip_batch_load_device(lcqp_hip_batch_t* h, int first, int count, int shared,
                                          const double* Q, const double* g, const double* L, const double* R,
                                          const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                                          const double* A, const double* lbA, const double* ubA,
                                          const double* lb, const double* ub, const double* x0, const double* y0, void* stream)
{ return guarded(g_err, [&] {
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    DevBatch& d = h->db;
    const int n = d.n, nC = d.nC, nComp = d.nComp;
    if (first < 0 || count <= 0 || first > d.B - count || (shared & ~15)) return LCQP_INVALID_ARGUMENT;
    // a matrix that is not handed over stays as the pool holds it: every instance of the range must hold a problem then
    bool held = true;
    for (int k = 0; k < count; k++) held = held && h->rs.filled[(size_t)first + k];
    const int given = given_matrices(Q, nC ? A : nullptr, nComp ? L : nullptr, nComp ? R : nullptr);
    if (d.shared) {      // one [rows][nV] array per matrix, for the batch: every given matrix carries its shared bit; NULL keeps the one in place
        if (given & ~shared) { g_err = "load_device: this batch holds one set of matrices; every matrix handed over needs its bit of `shared`"; return LCQP_INVALID_ARGUMENT; }
        const int rc = shared_matrices_present(h, given | (nComp ? 0 : 12));
        if (rc == LCQP_INVALID_ARGUMENT) return rc;
        if (!g) return LCQP_INVALID_OBJECTIVE_LINEAR_TERM;
        if (rc) return rc;
    } else {
    if (!Q && !held) return LCQP_INVALID_ARGUMENT;
    if (!g) return LCQP_INVALID_OBJECTIVE_LINEAR_TERM;
    if (!A && nC > 0 && !held) return LCQP_INVALID_CONSTRAINT_MATRIX;
    if ((!L || !R) && !held) return LCQP_INVALID_COMPLEMENTARITY_MATRIX;
    }
    if ((lb || ub) && d.boxcap == 0) { g_err = "batch was created without box-bound capacity"; return LCQP_INVALID_ARGUMENT; }
    HIPCHK(g_err, hipSetDevice(h->device));
    const PackVectors pv = {g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0};
    PackMatrices pm{};
    const double* mats[4] = {Q, nC ? A : nullptr, nComp ? L : nullptr, nComp ? R : nullptr};
    const char* names[4] = {"Q", "A", "L", "R"};
    const size_t rows[4] = {(size_t)n, (size_t)nC, (size_t)nComp, (size_t)nComp};
    for (int k = 0; k < 4; k++) {
        const bool one = (shared >> k) & 1;
        pm.src[k] = mats[k];
        pm.stride[k] = one ? 0 : rows[k] * n;
        if (!device_pointer_ok(g_err, h, names[k], mats[k], sizeof(double) * (one ? 1 : (size_t)count) * rows[k] * n)) return LCQP_INVALID_ARGUMENT;
    }
    if (!vectors_ok(h, count, pv)) return LCQP_INVALID_ARGUMENT;
    std::vector<char> flags((size_t)count * n);
    return device_call(g_err, h, stream, [&] {
        unsigned long long words[2];
        if (int rc = check_vectors(h, first, count, pv, false, words, (lb || ub) ? flags.data() : nullptr)) return rc;
        if (words[0] != ~0ull) return LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND;
        if (d.shared) {
            std::vector<char> set;
            if (int rc = shared_box_check(g_err, h, first, count, flags.data(), given, set)) return rc;
            h->boxSet = set; h->boxDefined = true; h->matsHeld |= given | (nComp ? 0 : 12);
            if (given) if (int rc = dense_pack_matrices(h, 0, 1, pm, true)) return rc;
        }
        // the host state of lcqp_hip_batch_load: the setup mark, the lbL / lbR flags, the box flags
        h->rs.invalidate();
        load_bound_flags(d, h->anyLoaded, first, lbL, lbR);
        for (int k = 0; k < count; k++) h->rs.filled[(size_t)first + k] = 1;
        memcpy(h->boxed.data() + (size_t)first * n, flags.data(), flags.size());
        h->anyLoaded = true;
        return dense_pack(h, first, count, pv, pm, false);
    });
}); }

extern "C" int lcqp_hip_batch_update_device(lcqp_hip_batch_t* h, int first, int count, const double* g,
                                            const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                                            const double* lbA, const double* ubA, const double* lb, const double* ub,
                                            const double* x0, const double* y0, void* stream)
{ return guarded(g_err, [&] {
    if (int rc = check_update(g_err, h, first, count, g)) return rc;      // (the values are checked on the device)
    DevBatch& d = h->db;
    HIPCHK(g_err, hipSetDevice(h->device));
    const PackVectors pv = {g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0};
    if (!vectors_ok(h, count, pv)) return LCQP_INVALID_ARGUMENT;
    return device_call(g_err, h, stream, [&] {
        unsigned long long words[2];
        if (int rc = check_vectors(h, first, count, pv, true, words, nullptr)) return rc;
        if (words[0] != ~0ull) return LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND;
        if (words[1] != ~0ull) {
            const unsigned long long j = words[1] >> 1;
            g_err = box_change_message((int)(j % d.n), first + (int)(j / d.n), words[1] & 1);
            return LCQP_INVALID_ARGUMENT;
        }
        d.hasLbL |= lbL ? 1 : 0; d.hasLbR |= lbR ? 1 : 0;
        return dense_pack(h, first, count, pv, PackMatrices{}, true);
    });
}); }

extern "C" int lcqp_hip_batch_get_solution_device(lcqp_hip_batch_t* h, double* x, double* y, lcqp_stats_t* stats, void* stream)
{
    return guarded(g_err, [&] { return get_solution_device(g_err, h, h ? h->db.nd : 0, x, y, stats, stream); });
}

// New matrices for instances [first, first + count) from device arrays of the caller: lcqp_hip_batch_update_matrices behind the hand-over
// of the streams.  shared: bit k set -- matrix k of (Q, A, L, R) is one [rows][nV] array for the whole range.
extern "C" int lcqp_hip_batch_update_matrices_device(lcqp_hip_batch_t* h, int first, int count, int shared, const double* Q, const double* L,
                                                     const double* R, const double* A, void* stream)
{ return guarded(g_err, [&] {
    if (int rc = check_update_matrices(h, first, count, Q, L, R, A)) return rc;
    if (shared & ~15) return LCQP_INVALID_ARGUMENT;
    const DevBatch& d = h->db;
    HIPCHK(g_err, hipSetDevice(h->device));
    PackMatrices pm{};
    const double* mats[4] = {Q, d.nC ? A : nullptr, d.nComp ? L : nullptr, d.nComp ? R : nullptr};
    const char* names[4] = {"Q", "A", "L", "R"};
    const size_t rows[4] = {(size_t)d.n, (size_t)d.nC, (size_t)d.nComp, (size_t)d.nComp};
    for (int k = 0; k < 4; k++) {
        const bool one = (shared >> k) & 1;
        pm.src[k] = mats[k];
        pm.stride[k] = one ? 0 : rows[k] * d.n;
        if (!device_pointer_ok(g_err, h, names[k], mats[k], sizeof(double) * (one ? 1 : (size_t)count) * rows[k] * d.n)) return LCQP_INVALID_ARGUMENT;
    }
    if (d.shared && (given_matrices(mats[0], mats[1], mats[2], mats[3]) & ~shared)) {
        g_err = "update_matrices_device: this batch holds one set of matrices; every matrix handed over needs its bit of `shared`";
        return LCQP_INVALID_ARGUMENT;
    }
    return device_call(g_err, h, stream, [&] {
        h->rs.matrices_changed();
        return d.shared ? dense_pack_matrices(h, 0, 1, pm, false) : dense_pack_matrices(h, first, count, pm, false);
    });
}); }
