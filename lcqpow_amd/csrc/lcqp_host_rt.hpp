// lcqp_host_rt.hpp -- host runtime shared by the C ABIs of the dense (lcqp_hip.hip, lcqp_hip_diff.hip, lcqp_hip_device.hip, lcqp_hip_qp.hip, lcqp_hip_util.hip) and sparse
// (lcqp_sparse_host.hip, lcqp_sparse_diff.hip, lcqp_sparse_device.hip) arms: error reporting, owners of streams, events and device memory, and the entry-point bodies both arms have
// in common -- solution, options, trace, re-solves, the buffers of a sensitivity launch, the hand-over of a device-pointer call, the upload of a host
// load / update.  What drives the sensitivity,
// Jacobian and adjoint kernels on top of these is lcqp_sens_rt.hpp.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/lcqp_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

namespace lcqp_rt {

// "<call>: <HIP reason>" into an arm's error slot (lcqp_hip_last_error / lcqp_hip_sparse_last_error).  The runtime also keeps the error
// as the thread's last one until it is asked for: it is taken here, or the hipGetLastError() behind the next launch of the thread --
// of any handle -- would report this call's failure as that launch's.
inline int hip_fail(std::string& slot, const char* call, hipError_t e)
{
    slot = std::string(call) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return LCQP_HIP_ERROR;
}
#define HIPCHK(slot, call)                                                 \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) return lcqp_rt::hip_fail(slot, #call, e_);   \
    } while (0)

// The body of an extern "C" entry point: nothing throws across the C boundary.  An exception (std::bad_alloc from a host container)
// leaves its message in the arm's slot and returns `fallback` -- LCQP_HIP_ERROR, or nullptr / 0.0 for the entry points that return a
// pointer / a double, nothing for the void ones.
template <class F, class R = int>
__attribute__((always_inline)) inline auto guarded(std::string& err, F body, R fallback = LCQP_HIP_ERROR) -> decltype(body())
{
    try { return body(); }
    catch (...) {
        err = "out of host memory";
        if constexpr (!std::is_void_v<decltype(body())>) return fallback;
    }
}

// a stream / an event, created by the constructor (its result in `status`) and destroyed by the destructor
struct Stream {
    hipStream_t s = nullptr;
    hipError_t status = hipStreamCreate(&s);
    Stream() = default;
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    hipError_t status;
    explicit Event(unsigned flags = hipEventDefault) : status(hipEventCreateWithFlags(&e, flags)) {}
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

// The device memory of a handle or of one call: `count` elements of T (at least one), copied from `init` or zero-filled on `zeroOn`
// (a handle's *_create synchronises that stream before it returns).  release() frees one allocation, the destructor all of them.
struct DevMem {
    hipStream_t zeroOn = nullptr;
    std::vector<void*> ptrs;
    DevMem() = default;
    explicit DevMem(hipStream_t s) : zeroOn(s) {}
    DevMem(const DevMem&) = delete; DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T>
    bool alloc(std::string& err, T*& p, size_t count, const std::remove_const_t<T>* init = nullptr)
    {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        void* q = nullptr;
        ptrs.reserve(ptrs.size() + 1);      // the push_back below cannot throw: nothing leaks
        if (hipError_t e = hipMalloc(&q, bytes)) { hip_fail(err, "hipMalloc", e); return false; }
        ptrs.push_back(q);
        p = static_cast<T*>(q);
        const hipError_t e = init ? hipMemcpy(q, init, sizeof(T) * count, hipMemcpyHostToDevice) : hipMemsetAsync(q, 0, bytes, zeroOn);
        if (e != hipSuccess) { hip_fail(err, init ? "hipMemcpy" : "hipMemsetAsync", e); return false; }
        return true;
    }
    void release(const void* p)
    {
        auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (it == ptrs.end()) return;
        (void)hipFree(*it);
        ptrs.erase(it);
    }
};

inline double bnd(const double* p, size_t i, double dflt) { return p ? p[i] : dflt; }

// ---- entry-point bodies of both arms: H is lcqp_hip_batch or lcqp_hip_sparse (device, stream, ev0 .. ev2, mem, ran and the batch
// struct db with the fields of the same names, DevBatch / SpBatch)

// *_synchronize: the device of the handle current, its stream drained
template <class H>
int synchronize(std::string& err, H* h)
{
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    HIPCHK(err, hipSetDevice(h->device));
    HIPCHK(err, hipStreamSynchronize(h->stream));
    return 0;
}

// *_set_options.  The per-iterate tracking buffers (options.storeSteps, src/OutputStatistics.cpp:131-164) hold the first `depth` iterates
// at most; they are kept at the largest trace the handle was asked for (a regrow frees the smaller ones), and the kernels record only
// while storeSteps is on: traceCap < 0 keeps the buffers of a handle whose tracking has been switched off again.
template <class H>
int set_options(std::string& err, H* h, const lcqp_options_t* opt, int depth)
{
    if (!h || !opt) return LCQP_INVALID_ARGUMENT;
    if (opt->nDynamicPenalty > 64) { err = "nDynamicPenalty > 64 unsupported"; return LCQP_HIP_UNSUPPORTED; }
    auto& d = h->db;
    const int want = opt->storeSteps ? std::min(std::max(opt->maxIterations + 1, 1), depth) : 0;
    const int have = d.traceCap < 0 ? -d.traceCap : d.traceCap;
    if (want > have) {
        if (int rc = synchronize(err, h)) return rc;
        h->mem.release(d.traceS); h->mem.release(d.traceX); h->mem.release(d.traceLen);
        d.traceS = d.traceX = nullptr; d.traceLen = nullptr; d.traceCap = 0;
        if (!h->mem.alloc(err, d.traceS, (size_t)d.B * want * 8) || !h->mem.alloc(err, d.traceX, (size_t)d.B * want * d.n) ||
            !h->mem.alloc(err, d.traceLen, (size_t)d.B)) {
            err = "out of device memory for the iterate trace: " + err;
            return LCQP_HIP_ERROR;
        }
        d.traceCap = want;
    } else d.traceCap = opt->storeSteps ? have : -have;
    d.opt = *opt;
    return 0;
}

// *_get_trace: the trace of one instance of the last run, at most `cap` iterates
template <class H>
int get_trace(std::string& err, H* h, int instance, int cap, double* scalars, double* x, int* len)
{
    if (!h || !len) return LCQP_INVALID_ARGUMENT;
    const auto& d = h->db;
    *len = 0;
    if (instance < 0 || instance >= d.B) return LCQP_INVALID_ARGUMENT;
    if (d.traceCap <= 0) return 0;      // no buffers, or tracking switched off: an empty trace
    if (int rc = synchronize(err, h)) return rc;
    int n = 0;
    HIPCHK(err, hipMemcpy(&n, d.traceLen + instance, sizeof(int), hipMemcpyDeviceToHost));
    n = std::min(n, std::min(cap, d.traceCap));
    if (n > 0 && scalars) HIPCHK(err, hipMemcpy(scalars, d.traceS + (size_t)instance * d.traceCap * 8, sizeof(double) * 8 * n, hipMemcpyDeviceToHost));
    if (n > 0 && x) HIPCHK(err, hipMemcpy(x, d.traceX + (size_t)instance * d.traceCap * d.n, sizeof(double) * (size_t)d.n * n, hipMemcpyDeviceToHost));
    *len = n;
    return 0;
}

// *_last_timing: setup (ev0 -> ev1) and solve (ev1 -> ev2) of the last run
template <class H>
int last_timing(std::string& err, H* h, float* setup_ms, float* solve_ms)
{
    if (!h || !h->ran) return LCQP_INVALID_ARGUMENT;
    HIPCHK(err, hipSetDevice(h->device));
    HIPCHK(err, hipEventSynchronize(h->ev2));
    if (setup_ms) HIPCHK(err, hipEventElapsedTime(setup_ms, h->ev0, h->ev1));
    if (solve_ms) HIPCHK(err, hipEventElapsedTime(solve_ms, h->ev1, h->ev2));
    return 0;
}

// *_get_solution: x [B][n], y [B][ndual], the statistics [B]
template <class H>
int get_solution(std::string& err, H* h, int ndual, double* x, double* y, lcqp_stats_t* stats)
{
    if (int rc = synchronize(err, h)) return rc;
    const auto& d = h->db;
    if (x) HIPCHK(err, hipMemcpy(x, d.xout, sizeof(double) * (size_t)d.B * d.n, hipMemcpyDeviceToHost));
    if (y) HIPCHK(err, hipMemcpy(y, d.yout, sizeof(double) * (size_t)d.B * ndual, hipMemcpyDeviceToHost));
    if (stats) HIPCHK(err, hipMemcpy(stats, d.stats, sizeof(lcqp_stats_t) * (size_t)d.B, hipMemcpyDeviceToHost));
    return 0;
}

// ---- re-solves (*_update / *_resolve / *_launch_counts) and sensitivities: the host state of a handle (member rs; lcqp_sens_rt.hpp: sn) and the
// entry-point bodies of both arms.  Nothing of it is a kernel argument, and none of it enters the dynamic symbol table of the library.
#pragma GCC visibility push(hidden)
struct ResolveState {
    // the setup on the device belongs to the matrices and options in place: set by run / setup / resolve, cleared by load /
    // generate_synthetic / set_options (invalidate)
    bool setupValid = false;
    // the stored point, working set and factors belong to a solve on the data in place (set by run / resolve, cleared with setupValid):
    // what *_sensitivity differentiates
    bool solved = false;
    // the matrices changed since the last solve (*_update_matrices, sparse arm: *_update_values), but its point, statuses and penalties
    // are still on the device: a warm *_resolve sets up again around them.  Cleared with setupValid by everything else that clears it
    bool pointKept = false;
    std::vector<char> filled;            // [B]: the instance holds a problem
    double* rhoStart = nullptr;           // [B] on the device: starting penalties of a warm re-solve
    int nSetups = 0, nLaunches = 0;       // full setups and homotopy launches issued
    // the kernel time of the last sensitivity call that returned its results, summed over its launches (ev0 -> ev1 of the SensBuffers each
    // ran on: a vector call is one launch, a Jacobian one per chunk); < 0 before the first
    float sensMs = -1.f;
    void invalidate() { setupValid = solved = pointKept = false; }
    // the host state of *_update_matrices / *_update_values once the range is about to be written: no setup and no solve belong to the
    // matrices in place any more, but what the last solve stored on the device is still there
    void matrices_changed()
    {
        const bool kept = solved || pointKept;
        invalidate();
        pointKept = kept;
    }
};

// the value check of a host load / update over its whole range ([count * nComp] each, null: absent): a lower complementarity bound of
// -inf is refused (the device-pointer twins make the same test in their check kernel)
inline int check_lower_bounds(size_t entries, const double* lbL, const double* lbR)
{
    for (size_t j = 0; j < entries; j++)
        if (bnd(lbL, j, 0.0) <= -INFINITY || bnd(lbR, j, 0.0) <= -INFINITY) return LCQP_INVALID_LOWER_COMPLEMENTARITY_BOUND;
    return 0;
}

// *_update and *_update_device: the checks both arms make that need no values, in this order; the host calls add the values' (lbL, lbR
// on the host).  Nothing has been written when one of them fails.
template <class H>
int check_update(std::string&, H* h, int first, int count, const double* g)
{
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (first < 0 || count <= 0 || first > h->db.B - count) return LCQP_INVALID_ARGUMENT;
    for (int k = 0; k < count; k++) if (!h->rs.filled[(size_t)first + k]) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (!g) return LCQP_INVALID_OBJECTIVE_LINEAR_TERM;
    return 0;
}
template <class H>
int check_update(std::string& err, H* h, int first, int count, const double* g, const double* lbL, const double* lbR)
{
    if (int rc = check_update(err, h, first, count, g)) return rc;
    return check_lower_bounds((size_t)count * h->db.nComp, lbL, lbR);
}

// The lbL / lbR flags of a batch at a load (host or device) of a range that starts at `first`.  A batch may mix instances with and without
// lbL / lbR: an absent bound vector is the zero vector, and the phi expressions of src/LCQProblem.cpp:969-996 with zeros are the arithmetic
// of an instance loaded without them, bit for bit.  The batch-wide flags only say whether ANY instance carries bounds, i.e. whether the
// kernels read the (zero-filled) arrays at all: the first load of the handle, or a load starting at instance 0, starts them over, every
// other load -- and every update -- adds to them.
template <class D>
void load_bound_flags(D& d, bool loaded, int first, const double* lbL, const double* lbR)
{
    const int hasL = lbL ? 1 : 0, hasR = lbR ? 1 : 0;
    if (!loaded || first == 0) { d.hasLbL = hasL; d.hasLbR = hasR; }
    else { d.hasLbL |= hasL; d.hasLbR |= hasR; }
}

// *_resolve up to the launches: an error code, RESOLVE_RUNS when no setup belongs to the matrices and options in place (the call is then
// *_run), 0 when the refresh kernel may stand where the setup stands.  rho0 [B]: every entry finite and positive.
enum { RESOLVE_RUNS = -1 };
template <class H>
int check_resolve(std::string& err, H* h, int mode, const double* rho0, bool loaded)
{
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (mode != 0 && mode != 1) { err = "resolve: mode is 0 (cold) or 1 (warm)"; return LCQP_INVALID_ARGUMENT; }
    if (rho0)
        for (int b = 0; b < h->db.B; b++)
            if (!(rho0[b] > 0.0) || !std::isfinite(rho0[b])) { err = "resolve: rho0[" + std::to_string(b) + "] is not a finite positive number"; return LCQP_INVALID_ARGUMENT; }
    if (!loaded) return LCQP_LCQPOBJECT_NOT_SETUP;
    return h->rs.setupValid ? 0 : RESOLVE_RUNS;
}

template <class H>
int launch_counts(H* h, int out[2])
{
    if (!h || !out) return LCQP_INVALID_ARGUMENT;
    out[0] = h->rs.nSetups; out[1] = h->rs.nLaunches;
    return 0;
}

// one block of a read-back entry point (tests, diagnostics): `count` values from the device to dst, or nothing when the caller passed NULL
template <class T>
int read_back(std::string& err, T* dst, const T* src, size_t count)
{
    if (dst) HIPCHK(err, hipMemcpy(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost));
    return 0;
}

// The device buffers of *_sensitivity (layouts at k_sensitivity / k_sensitivity_blk / k_sparse_sensitivity / k_sparse_sensitivity_blk), grown on demand, and the
// events around the last launch.  A call is reserve, upload, record(ev0), the arm's launch, record(ev1), download.
struct SensBuffers {
    double *v = nullptr, *dg = nullptr, *db = nullptr;
    int *side = nullptr, *info = nullptr;
    size_t capB = 0, capRows = 0;         // instances and rows the buffers have room for
    double* ws = nullptr;                 // k_sparse_sensitivity_blk: the workspaces of the work items of one chunk (reserve_ws)
    size_t capWs = 0;
    Event ev0, ev1;
    hipStream_t stream = nullptr;         // of the call in progress, with its sizes: rows = B * nrhs; leading dimensions in elements
    size_t B = 0, rows = 0, ldV = 0, ldDg = 0, ldDb = 0, nSide = 0;

    // room for nB instances and nB * nrhs rows, grown when either is exceeded (the blocked kernel's calls vary both: a Jacobian works on a
    // chunk of the batch, with one right-hand side per variable)
    int reserve(std::string& err, DevMem& mem, hipStream_t s, size_t nB, size_t nrhs, size_t ldv, size_t lddg, size_t lddb, size_t nside)
    {
        return reserve_rows(err, mem, s, nB, nB * nrhs, ldv, lddg, lddb, nside);
    }
    // the same with the rows given as such (the sparse panel kernel stages the rows of a chunk of work items, not of whole instances)
    int reserve_rows(std::string& err, DevMem& mem, hipStream_t s, size_t nB, size_t nRows, size_t ldv, size_t lddg, size_t lddb, size_t nside)
    {
        for (hipError_t e : {ev0.status, ev1.status}) if (e != hipSuccess) return hip_fail(err, "hipEventCreate", e);
        stream = s; B = nB; rows = nRows; ldV = ldv; ldDg = lddg; ldDb = lddb; nSide = nside;
        if (nB <= capB && rows <= capRows) return 0;
        HIPCHK(err, hipStreamSynchronize(s));
        for (const void* p : {(const void*)v, (const void*)dg, (const void*)db, (const void*)side, (const void*)info}) mem.release(p);
        v = dg = db = nullptr; side = info = nullptr;
        const size_t nb = nB > capB ? nB : capB, nr = rows > capRows ? rows : capRows;
        capB = capRows = 0;
        if (!mem.alloc(err, v, nr * ldV) || !mem.alloc(err, dg, nr * ldDg) || !mem.alloc(err, db, nr * ldDb) ||
            !mem.alloc(err, side, nb * nSide) || !mem.alloc(err, info, nb)) return LCQP_HIP_ERROR;
        capB = nb; capRows = nr;
        return 0;
    }
    int reserve_ws(std::string& err, DevMem& mem, hipStream_t s, size_t doubles)
    {
        if (doubles <= capWs) return 0;
        HIPCHK(err, hipStreamSynchronize(s));
        mem.release(ws);
        ws = nullptr; capWs = 0;
        if (!mem.alloc(err, ws, doubles)) return LCQP_HIP_ERROR;
        capWs = doubles;
        return 0;
    }
    int upload(std::string& err, const double* hv)
    {
        HIPCHK(err, hipMemcpyAsync(v, hv, sizeof(double) * rows * ldV, hipMemcpyHostToDevice, stream));
        return 0;
    }
    // rows of `width` doubles out of device rows of pitch `ld`: a pitched copy where the device rows are padded, a plain one otherwise
    int rows_out(std::string& err, double* dst, const double* src, size_t width, size_t ld)
    {
        if (ld > width) HIPCHK(err, hipMemcpy2DAsync(dst, sizeof(double) * width, src, sizeof(double) * ld, sizeof(double) * width, rows, hipMemcpyDeviceToHost, stream));
        else HIPCHK(err, hipMemcpyAsync(dst, src, sizeof(double) * rows * width, hipMemcpyDeviceToHost, stream));
        return 0;
    }
    // the results to device arrays of the caller (ddb, dside, dinfo may be NULL), on the stream; nothing waits
    int download_device(std::string& err, double* ddg, double* ddb, int* dside, int* dinfo, size_t wDg, size_t wDb)
    {
        HIPCHK(err, hipMemcpy2DAsync(ddg, sizeof(double) * wDg, dg, sizeof(double) * ldDg, sizeof(double) * wDg, rows, hipMemcpyDeviceToDevice, stream));
        if (ddb) HIPCHK(err, hipMemcpy2DAsync(ddb, sizeof(double) * wDb, db, sizeof(double) * ldDb, sizeof(double) * wDb, rows, hipMemcpyDeviceToDevice, stream));
        if (dside) HIPCHK(err, hipMemcpyAsync(dside, side, sizeof(int) * B * nSide, hipMemcpyDeviceToDevice, stream));
        if (dinfo) HIPCHK(err, hipMemcpyAsync(dinfo, info, sizeof(int) * B, hipMemcpyDeviceToDevice, stream));
        return 0;
    }
    // the results to the host (hdb, hside, hinfo may be NULL); synchronous on return
    int download(std::string& err, double* hdg, double* hdb, int* hside, int* hinfo, size_t wDg, size_t wDb)
    {
        if (int rc = rows_out(err, hdg, dg, wDg, ldDg)) return rc;
        if (hdb) if (int rc = rows_out(err, hdb, db, wDb, ldDb)) return rc;
        if (hside) HIPCHK(err, hipMemcpyAsync(hside, side, sizeof(int) * B * nSide, hipMemcpyDeviceToHost, stream));
        if (hinfo) HIPCHK(err, hipMemcpyAsync(hinfo, info, sizeof(int) * B, hipMemcpyDeviceToHost, stream));
        HIPCHK(err, hipStreamSynchronize(stream));
        return 0;
    }
};

// ---- the device-pointer entry points of both arms (lcqp_hip_diff.hip, lcqp_hip_device.hip; lcqp_sparse_diff.hip, lcqp_sparse_device.hip): H has
// device, stream and the two events evIn / evOut (hipEventDisableTiming) ----
// A data pointer of such a call: NULL, or plain device memory of the handle's device with `bytes` behind it (align: 8, or 16 where a kernel stores pairs of doubles).
// Anything else -- pageable, pinned or managed host memory, another device -- leaves a message and returns false; nothing is dereferenced.
template <class H>
bool device_pointer_ok(std::string& err, const H* h, const char* name, const void* p, size_t bytes, size_t align = 8)
{
    if (!p) return true;
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.isManaged) {
        err = std::string(name) + ": not a device pointer (the *_device entry points take plain device memory; host, pinned and managed memory go through the host entry points)";
        return false;
    }
    if (at.device != h->device) {
        err = std::string(name) + ": memory of device " + std::to_string(at.device) + ", the batch lives on device " + std::to_string(h->device);
        return false;
    }
    if ((size_t)(uintptr_t)p % align) {
        err = std::string(name) + ": not aligned to " + std::to_string(align) + " bytes";
        return false;
    }
    void* base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return true; }
    if ((const char*)p + bytes > (const char*)base + size) {
        err = std::string(name) + ": the allocation ends before the " + std::to_string(bytes) + " bytes the call moves";
        return false;
    }
    return true;
}

// The hand-over of a device-pointer call: the handle's stream waits for what the caller's stream holds so far (the constructor), the
// caller's stream for what the call enqueued on the handle's stream (done()).  Nothing waits on the host.
template <class H>
struct StreamHandOver {
    H* h;
    hipStream_t caller;
    hipError_t status = hipSuccess;
    StreamHandOver(H* h_, void* stream) : h(h_), caller((hipStream_t)stream)
    {
        if (caller == h->stream.s) return;
        status = hipEventRecord(h->evIn, caller);
        if (status == hipSuccess) status = hipStreamWaitEvent(h->stream, h->evIn, 0);
    }
    hipError_t done()
    {
        if (caller == h->stream.s) return hipSuccess;
        const hipError_t e = hipEventRecord(h->evOut, h->stream);
        return e != hipSuccess ? e : hipStreamWaitEvent(caller, h->evOut, 0);
    }
};

// What such a call enqueues, between the two halves of the hand-over: body() runs behind the caller's stream, and done() follows on every way
// out of it.  The code of the body where it fails (a failing done() behind it is not reported), else the status of done().
template <class H, class F>
int device_call(std::string& err, H* h, void* stream, F body)
{
    StreamHandOver<H> over(h, stream);
    HIPCHK(err, over.status);
    if (int rc = body()) {
        if (over.done() != hipSuccess) (void)hipGetLastError();
        return rc;
    }
    HIPCHK(err, over.done());
    return 0;
}

// *_get_solution_device: get_solution into device arrays of the caller, with copies on the handle's stream; nothing waits on the host
template <class H>
int get_solution_device(std::string& err, H* h, size_t ndual, double* x, double* y, lcqp_stats_t* stats, void* stream)
{
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    const auto& d = h->db;
    HIPCHK(err, hipSetDevice(h->device));
    const size_t B = d.B;
    if (!device_pointer_ok(err, h, "x", x, sizeof(double) * B * d.n) || !device_pointer_ok(err, h, "y", y, sizeof(double) * B * ndual) ||
        !device_pointer_ok(err, h, "stats", stats, sizeof(lcqp_stats_t) * B, 4)) return LCQP_INVALID_ARGUMENT;
    return device_call(err, h, stream, [&] {
        if (x) HIPCHK(err, hipMemcpyAsync(x, d.xout, sizeof(double) * B * d.n, hipMemcpyDeviceToDevice, h->stream));
        if (y) HIPCHK(err, hipMemcpyAsync(y, d.yout, sizeof(double) * B * ndual, hipMemcpyDeviceToDevice, h->stream));
        if (stats) HIPCHK(err, hipMemcpyAsync(stats, d.stats, sizeof(lcqp_stats_t) * B, hipMemcpyDeviceToDevice, h->stream));
        return 0;
    });
}

// a device buffer of the handle with room for `count` doubles (the stream is drained before a smaller one is freed)
template <class H>
int grow(std::string& err, H* h, double*& p, size_t& cap, size_t count)
{
    if (count <= cap) return 0;
    HIPCHK(err, hipStreamSynchronize(h->stream));
    h->mem.release(p);
    p = nullptr; cap = 0;
    if (!h->mem.alloc(err, p, count)) return LCQP_HIP_ERROR;
    cap = count;
    return 0;
}

// The chunks of a call with nItems work items of itemBytes of staging each under the cap: whole items, at least one per chunk.
inline size_t staging_chunk(size_t cap, size_t itemBytes, size_t nItems)
{
    size_t chunk = itemBytes ? cap / itemBytes : nItems;
    if (chunk < 1) chunk = 1;
    return chunk < nItems ? chunk : nItems;
}

// ---- the host load / update of both arms (lcqp_hip.hip, lcqp_sparse_host.hip) are transport only: the caller's raw arrays go to the device
// in chunks of instances, and the arm's pack step -- the kernels of its device-pointer load / update -- builds the pools from them.  H has
// stream, mem, the staging cap sn.staging and the member `up` ----
// a pinned staging slot and the event of the copy that last read it
struct StageSlot {
    void* buf = nullptr;
    Event done{hipEventDisableTiming};
    ~StageSlot() { if (buf) (void)hipHostFree(buf); }
};
// two pinned slots -- chunk k is gathered into slot k & 1 while the copy out of slot (k - 1) & 1 is in flight -- and the device staging
// of two chunks behind them (owned by the handle's DevMem)
struct UploadStage {
    StageSlot slot[2];
    size_t slotBytes = 0;
    double* dev = nullptr;
    size_t devCap = 0;
    // both pinned slots hold at least `bytes`
    int reserve(std::string& err, size_t bytes)
    {
        for (const StageSlot& st : slot) if (st.done.status != hipSuccess) return hip_fail(err, "hipEventCreate", st.done.status);
        if (slotBytes >= bytes) return 0;
        slotBytes = 0;
        for (StageSlot& st : slot) {
            HIPCHK(err, hipEventSynchronize(st.done));
            if (st.buf) (void)hipHostFree(st.buf);
            st.buf = nullptr;
            HIPCHK(err, hipHostMalloc(&st.buf, bytes, hipHostMallocDefault));
        }
        slotBytes = bytes;
        return 0;
    }
};

// one raw array of a host load / update: [count][per] doubles on the host; null or per = 0: absent
struct RawArray { const double* src; size_t per; };
// A chunk is whole instances, at least one, of at most UPLOAD_CHUNK_BYTES and at most half the handle's staging cap (the device staging
// holds two chunks).  Small chunks keep the pinned memory small and let the gather of one chunk hide behind the copy of the one before.
constexpr size_t UPLOAD_CHUNK_BYTES = (size_t)16 << 20;

// The arrays of `count` instances to the device and through pack(c0, cb, dev): for the chunk [c0, c0 + cb) of the range, dev[a] is array a
// of the chunk on the device ([cb][per]; null where the array is absent), and pack enqueues the pack step on h->stream.  Stream order
// keeps a chunk's staging until its pack kernels have read it; the one synchronisation is at the end, so the caller's arrays are free on
// return.  The value checks come before the call: nothing here depends on the values.
template <class H, size_t N, class P>
int upload_packed(std::string& err, H* h, int count, const RawArray (&arr)[N], P pack)
{
    size_t per = 0;
    for (const RawArray& a : arr) if (a.src) per += a.per;
    const size_t chunk = staging_chunk(std::min(h->sn.staging / 2, UPLOAD_CHUNK_BYTES), sizeof(double) * per, count);
    UploadStage& up = h->up;
    if (int rc = up.reserve(err, sizeof(double) * chunk * per)) return rc;
    if (int rc = grow(err, h, up.dev, up.devCap, 2 * chunk * per)) return rc;
    for (size_t c0 = 0, turn = 0; c0 < (size_t)count; c0 += chunk, turn ^= 1) {
        const size_t cb = std::min(chunk, (size_t)count - c0);
        StageSlot& slot = up.slot[turn];
        HIPCHK(err, hipEventSynchronize(slot.done));      // the copy that last read this slot is done
        double *pinned = static_cast<double*>(slot.buf), *staged = up.dev + turn * chunk * per;
        const double* dev[N];
        size_t at = 0;
        for (size_t a = 0; a < N; a++) {
            const bool there = arr[a].src && arr[a].per;
            dev[a] = there ? staged + at : nullptr;
            if (!there) continue;
            std::memcpy(pinned + at, arr[a].src + c0 * arr[a].per, sizeof(double) * cb * arr[a].per);
            at += cb * arr[a].per;
        }
        HIPCHK(err, hipMemcpyAsync(staged, pinned, sizeof(double) * at, hipMemcpyHostToDevice, h->stream));
        HIPCHK(err, hipEventRecord(slot.done, h->stream));
        if (int rc = pack((int)c0, (int)cb, dev)) return rc;
    }
    HIPCHK(err, hipStreamSynchronize(h->stream));
    return 0;
}

#pragma GCC visibility pop

}  // namespace lcqp_rt
