// lcqp_sens_rt.hpp -- the host code behind the sensitivity, Jacobian and adjoint entry points of both arms (lcqp_hip_diff.hip, lcqp_sparse_diff.hip):
// the state a handle keeps for them (member sn) and the one copy of what drives their kernels -- the staging cap (grow and staging_chunk
// are lcqp_host_rt.hpp's: the host load / update use them too), the timed launch, the call around a sensitivity kernel, the Jacobians through
// a vector kernel, the chunks of a host adjoint -- and of what every entry point opens and closes with: one guard per call shape (guard_vectors,
// guard_pairs, guard_range) and the body around a host call or its device-pointer twin (sens_body).  Templates on the handle H
// (lcqp_hip_batch / lcqp_hip_sparse: device, stream, mem, db, rs, sn, ndual()) like those of lcqp_host_rt.hpp; what differs between the arms -- the
// kernels, their pitches, the width of the dual vector -- comes in as arguments and callables.  Host code only.
#pragma once
#include "lcqp_host_rt.hpp"

#include <cstring>

namespace lcqp_rt {
#pragma GCC visibility push(hidden)

struct SensState {
    SensBuffers sens;                     // of k_sensitivity / k_sparse_sensitivity (and the sparse panel kernel)
    size_t staging = LCQP_JACOBIAN_STAGING_BYTES;      // device bytes a Jacobian / adjoint call may stage per chunk (*_set_jacobian_staging / *_set_adjoint_staging)
    // of *_adjoint, grown on demand: the upstream gradients on the duals [B][ndual]; the matrix gradients of one chunk of instances
    double *adjVy = nullptr, *adjOut = nullptr;
    size_t adjVyCap = 0, adjOutCap = 0;
    Event adjEv0, adjEv1;                 // around the last matrix-gradient launch
    // which events still hold the kernel time of the last sensitivity_device / adjoint_device call: 0: none, 1: sens, 2: the arm's second
    // SensBuffers (dense: sensBlk), 3: its third (dense: sensDual); + 4: adjEv0 / adjEv1 as well
    int sensPending = 0;
    // a device-pointer call that went in chunks: the kernel time of the chunks before the last one (their events are reused), added to
    // what the pending events hold
    float pendingMs = 0.f;
};

// *_set_jacobian_staging / *_set_adjoint_staging; 0: back to the default
template <class H>
int set_staging(H* h, size_t bytes)
{
    if (!h) return LCQP_INVALID_ARGUMENT;
    h->sn.staging = bytes ? bytes : (size_t)LCQP_JACOBIAN_STAGING_BYTES;
    return 0;
}

// one launch on stream s between two events, checked
template <class L>
int timed_launch(std::string& err, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, L launch)
{
    HIPCHK(err, hipEventRecord(ev0, s));
    launch();
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, hipEventRecord(ev1, s));
    return 0;
}

// The call around one launch of a sensitivity kernel on `count` instances with nrhs vectors each, on the handle's stream.  p: the row pitches of
// sb.v, sb.dg and sb.db in doubles and the width nd of the dual vector; v and dg go in and out n = p.ldV wide, vy, db and side nd wide.
// launch(dv, dvy, sb) starts the arm's kernel on the device vectors and the buffers of sb.
//   host call: v (NULL: the kernel makes unit vectors, nothing is uploaded) and vy (NULL: none) are uploaded, the results come back to host
//   arrays, synchronously, and the kernel time is added to ms.
//   dev (the device-pointer twins): v and vy are device arrays, read where they lie (they have the pitch the kernels expect); the results go
//   to the caller's device arrays with copies on the handle's stream, nothing waits on the host, and the kernel time stays in the events
//   of sb until *_sensitivity_timing asks for it: sensPending = pending.
struct SensPitch { size_t ldV, ldDg, ldDb, nd; };
template <class H, class L>
int sensitivity_call(std::string& err, H* h, SensBuffers& sb, const SensPitch& p, int count, int nrhs, const double* v, const double* vy, bool dev, int pending,
                     double* dg, double* db, int* side, int* info, float& ms, L launch)
{
    SensState& sn = h->sn;
    HIPCHK(err, hipSetDevice(h->device));
    if (int rc = sb.reserve(err, h->mem, h->stream, count, nrhs, p.ldV, p.ldDg, p.ldDb, p.nd)) return rc;
    sn.sensPending = 0;
    sn.pendingMs = 0.f;
    if (v && !dev) if (int rc = sb.upload(err, v)) return rc;
    const double *dv = dev ? v : (v ? sb.v : nullptr), *dvy = vy;
    if (vy && !dev) {      // (the DUAL instantiation of *_adjoint: vy [count][nrhs][nd] from the host)
        if (int rc = grow(err, h, sn.adjVy, sn.adjVyCap, sb.rows * p.nd)) return rc;
        HIPCHK(err, hipMemcpyAsync(sn.adjVy, vy, sizeof(double) * sb.rows * p.nd, hipMemcpyHostToDevice, h->stream));
        dvy = sn.adjVy;
    }
    if (int rc = timed_launch(err, h->stream, sb.ev0, sb.ev1, [&] { launch(dv, dvy, sb); })) return rc;
    if (dev) {
        if (int rc = sb.download_device(err, dg, db, side, info, p.ldV, p.nd)) return rc;
        sn.sensPending = pending;
        return 0;
    }
    if (int rc = sb.download(err, dg, db, side, info, p.ldV, p.nd)) return rc;
    float t = 0.f;
    HIPCHK(err, hipEventElapsedTime(&t, sb.ev0, sb.ev1));
    ms += t;
    return 0;
}

// The Jacobians of the instances [first, first + count) where the arm has only its vector kernel (dense: np >= 1024; sparse: the general LDL'):
// uploaded unit vectors in chunks of columns whose staging -- vecBytes per column, over the whole batch -- stays under the cap.  The vector
// kernel has no instance offset, so run(nc, v, dg, db, side, info, ms) takes nc columns through the whole batch of B (host arrays; ms: as
// sensitivity_call) and the range is copied out: a sub-range costs the launches of the full batch.  Jg [count][n][n], Jb [count][n][nd] or NULL.
template <class H, class R>
int jacobian_by_vectors(H* h, size_t vecBytes, size_t nd, int first, int count, double* Jg, double* Jb, int* side, int* info, R run)
{
    const size_t B = h->db.B, n = h->db.n, cc = staging_chunk(h->sn.staging, vecBytes, n);
    std::vector<double> V(B * cc * n), G(B * cc * n), Bd(Jb ? B * cc * nd : 0);
    std::vector<int> sd(B * nd), in(B);
    float ms = 0.f;
    for (size_t c0 = 0; c0 < n; c0 += cc) {
        const size_t nc = std::min(cc, n - c0);
        std::fill(V.begin(), V.end(), 0.0);
        for (size_t b = 0; b < B; b++) for (size_t k = 0; k < nc; k++) V[(b * nc + k) * n + c0 + k] = 1.0;
        if (int rc = run((int)nc, V.data(), G.data(), Jb ? Bd.data() : nullptr, sd.data(), in.data(), ms)) return rc;
        for (size_t i = 0; i < (size_t)count; i++) {
            std::memcpy(Jg + (i * n + c0) * n, G.data() + (first + i) * nc * n, sizeof(double) * nc * n);
            if (Jb) std::memcpy(Jb + (i * n + c0) * nd, Bd.data() + (first + i) * nc * nd, sizeof(double) * nc * nd);
        }
    }
    if (side) std::memcpy(side, sd.data() + (size_t)first * nd, sizeof(int) * (size_t)count * nd);
    if (info) std::memcpy(info, in.data() + first, sizeof(int) * (size_t)count);
    h->rs.sensMs = ms;
    return 0;
}

// The dual rows of the Jacobians of the instances [first, first + count) where the arm has only its vector kernel: vx = 0 and vy = the unit
// vectors of the dual positions that are in W for some instance of the range, uploaded in chunks of columns whose staging -- vecBytes per
// column, over the whole batch -- stays under the cap, on the whole batch (the vector kernel has no instance offset).
// run(nc, VY, G, Bd, sd, in, ms) takes nc pairs (0, VY [B][nc][nd]) through the batch (host arrays; sd, in may be NULL; ms: as
// sensitivity_call); its first call, with VY = NULL and nc = 1, is the plain sensitivity of a zero vector, for side and info.
// Jyg [count][nd][n], Jyb [count][nd][nd] or NULL, both zero-filled here: a row outside an instance's W stays exactly zero.
template <class H, class R>
int jacobian_duals_by_vectors(H* h, size_t vecBytes, size_t nd, int first, int count, double* Jyg, double* Jyb, int* side, int* info, R run)
{
    const size_t B = h->db.B, n = h->db.n;
    std::memset(Jyg, 0, sizeof(double) * (size_t)count * nd * n);
    if (Jyb) std::memset(Jyb, 0, sizeof(double) * (size_t)count * nd * nd);
    float ms = 0.f;
    std::vector<double> G(B * n);
    std::vector<int> sd(B * nd), in(B);
    if (int rc = run(1, nullptr, G.data(), nullptr, sd.data(), in.data(), ms)) return rc;
    std::vector<size_t> rows;
    for (size_t r = 0; r < nd; r++) {
        bool any = false;
        for (size_t i = 0; i < (size_t)count; i++) any = any || sd[(first + i) * nd + r] != 0;
        if (any) rows.push_back(r);
    }
    const size_t cc = staging_chunk(h->sn.staging, vecBytes, rows.size());
    std::vector<double> VY(B * cc * nd), Bd(B * cc * nd);
    G.resize(B * cc * n);
    for (size_t c0 = 0; c0 < rows.size(); c0 += cc) {
        const size_t nc = std::min(cc, rows.size() - c0);
        std::fill(VY.begin(), VY.end(), 0.0);
        for (size_t b = 0; b < B; b++) for (size_t k = 0; k < nc; k++) VY[(b * nc + k) * nd + rows[c0 + k]] = 1.0;
        if (int rc = run((int)nc, VY.data(), G.data(), Bd.data(), nullptr, nullptr, ms)) return rc;
        for (size_t i = 0; i < (size_t)count; i++)
            for (size_t k = 0; k < nc; k++) {
                const size_t r = rows[c0 + k], src = (first + i) * nc + k;
                if (sd[(first + i) * nd + r] == 0) continue;      // not in this instance's W: the row stays zero
                std::memcpy(Jyg + (i * nd + r) * n, G.data() + src * n, sizeof(double) * n);
                if (Jyb) std::memcpy(Jyb + (i * nd + r) * nd, Bd.data() + src * nd, sizeof(double) * nd);
            }
    }
    if (side) std::memcpy(side, sd.data() + (size_t)first * nd, sizeof(int) * (size_t)count * nd);
    if (info) std::memcpy(info, in.data() + first, sizeof(int) * (size_t)count);
    h->rs.sensMs = ms;
    return 0;
}

// ---- the matrix gradients of *_adjoint, on the buffers the sensitivity launch of the call left in sn.sens ----
// one launch of the arm's gradient kernel between adjEv0 and adjEv1
template <class H, class L>
int adjoint_launch(std::string& err, H* h, L launch)
{
    SensState& sn = h->sn;
    for (hipError_t e : {sn.adjEv0.status, sn.adjEv1.status}) if (e != hipSuccess) return hip_fail(err, "hipEventCreate", e);
    return timed_launch(err, h->stream, sn.adjEv0, sn.adjEv1, launch);
}

// the device-pointer twin: the one launch writes the caller's arrays, and its time stays in the events (sensPending)
template <class H, class L>
int adjoint_device(std::string& err, H* h, L launch)
{
    if (int rc = adjoint_launch(err, h, launch)) return rc;
    h->sn.sensPending |= 4;
    return 0;
}

// The host call: perInst doubles of gradients per instance, in chunks of instances whose staging in adjOut stays under the cap (reduce: the
// sums over the batch, one launch), `pad` spare doubles for the segments' alignment.  launch(c0, cb, cp) lays out the segments of the
// instances [c0, c0 + cb) in sn.adjOut, starts the arm's kernel on them, lists in cp what goes to the host and returns how many entries it
// listed (at most 4).  The kernel time of every chunk is added to ms.
struct AdjCopy { double* host; const double* dev; size_t doubles; };
template <class H, class L>
int adjoint_chunks(std::string& err, H* h, size_t perInst, size_t pad, int reduce, float& ms, L launch)
{
    SensState& sn = h->sn;
    const size_t N = reduce ? 1 : (size_t)h->db.B, chunk = staging_chunk(sn.staging, sizeof(double) * perInst, N);
    if (int rc = grow(err, h, sn.adjOut, sn.adjOutCap, chunk * perInst + pad)) return rc;
    for (size_t c0 = 0; c0 < N; c0 += chunk) {
        AdjCopy cp[4];
        int ncp = 0;
        if (int rc = adjoint_launch(err, h, [&] { ncp = launch(c0, std::min(chunk, N - c0), cp); })) return rc;
        for (int k = 0; k < ncp; k++) HIPCHK(err, hipMemcpyAsync(cp[k].host, cp[k].dev, sizeof(double) * cp[k].doubles, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(err, hipStreamSynchronize(h->stream));
        float t = 0.f;
        HIPCHK(err, hipEventElapsedTime(&t, sn.adjEv0, sn.adjEv1));
        ms += t;
    }
    return 0;
}

// Between two chunks of a device-pointer call: wait for the chunk's kernel and add its time to acc -- the next chunk reuses the events and
// the staging.  (Only a call whose staging exceeds the cap has more than one chunk; the last chunk's time stays in the events.)
inline int chunk_time(std::string& err, const SensBuffers& sb, float& acc)
{
    float t = 0.f;
    HIPCHK(err, hipEventSynchronize(sb.ev1));
    HIPCHK(err, hipEventElapsedTime(&t, sb.ev0, sb.ev1));
    acc += t;
    return 0;
}

// *_sensitivity_timing: the kernel time of the last sensitivity call (ResolveState::sensMs).  After a device-pointer call the time is still in
// the events: wait for them and form it.  second, third: the SensBuffers behind sensPending = 2 and 3 (the dense arm's sensBlk and sensDual).
template <class H>
int sensitivity_timing(std::string& err, H* h, float* kernel_ms, const SensBuffers* second = nullptr, const SensBuffers* third = nullptr)
{
    if (h && h->sn.sensPending) {
        SensState& sn = h->sn;
        HIPCHK(err, hipSetDevice(h->device));
        const SensBuffers& sb = (sn.sensPending & 3) == 3 ? *third : ((sn.sensPending & 3) == 2 ? *second : sn.sens);
        float t = 0.f, ta = 0.f;
        HIPCHK(err, hipEventSynchronize(sb.ev1));
        HIPCHK(err, hipEventElapsedTime(&t, sb.ev0, sb.ev1));
        if (sn.sensPending & 4) {
            HIPCHK(err, hipEventSynchronize(sn.adjEv1));
            HIPCHK(err, hipEventElapsedTime(&ta, sn.adjEv0, sn.adjEv1));
        }
        h->rs.sensMs = t + ta + sn.pendingMs;
        sn.sensPending = 0;
        sn.pendingMs = 0.f;
    }
    if (!h || !kernel_ms || h->rs.sensMs < 0.f) return LCQP_INVALID_ARGUMENT;
    *kernel_ms = h->rs.sensMs;
    return 0;
}

// ---- the guards of the entry points, one per call shape, for both arms and both twins of a pair (dev: the device-pointer twin).  A null
// handle is an invalid argument to a host call and an object that is not set up to its twin; then the arguments, then a finished solve; with
// dev the device is set and every array checked with the bytes the call moves.  H::ndual() is the width of the arm's dual vector. ----
inline int null_handle(bool dev) { return dev ? LCQP_LCQPOBJECT_NOT_SETUP : LCQP_INVALID_ARGUMENT; }

// what follows the argument checks of the vector and the pair shape, on `rows` vectors v (vname) and vy
template <class H>
int guard_rows(std::string& err, H* h, bool dev, size_t rows, const double* v, const char* vname, const double* vy, double* dg, double* db, int* side, int* info)
{
    if (!h->rs.solved) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (!dev) return 0;
    HIPCHK(err, hipSetDevice(h->device));
    const size_t B = h->db.B, n = h->db.n, nd = h->ndual();
    const bool ok = device_pointer_ok(err, h, vname, v, sizeof(double) * rows * n) && device_pointer_ok(err, h, "vy", vy, sizeof(double) * rows * nd) &&
                    device_pointer_ok(err, h, "dg", dg, sizeof(double) * rows * n) && device_pointer_ok(err, h, "db", db, sizeof(double) * rows * nd) &&
                    device_pointer_ok(err, h, "side", side, sizeof(int) * B * nd, 4) && device_pointer_ok(err, h, "info", info, sizeof(int) * B, 4);
    return ok ? 0 : LCQP_INVALID_ARGUMENT;
}

// the vector shape (*_sensitivity, *_sensitivity_blocked): nrhs vectors v per instance
template <class H>
int guard_vectors(std::string& err, H* h, bool dev, int nrhs, const double* v, double* dg, double* db, int* side, int* info)
{
    if (!h) return null_handle(dev);
    if (nrhs < 1 || !v || !dg) return LCQP_INVALID_ARGUMENT;
    return guard_rows(err, h, dev, (size_t)h->db.B * nrhs, v, "v", nullptr, dg, db, side, info);
}

// the pair shape: nrhs pairs (vx, vy) per instance, either of them (*_adjoint_blocked) or, with needVx, vx (*_adjoint: nrhs = 1, reduce 0 or 1)
template <class H>
int guard_pairs(std::string& err, H* h, bool dev, int nrhs, const double* vx, const double* vy, bool needVx, int reduce, double* dg, double* db, int* side, int* info)
{
    if (!h) return null_handle(dev);
    if (nrhs < 1 || !(vx || (vy && !needVx)) || !dg || (reduce != 0 && reduce != 1)) return LCQP_INVALID_ARGUMENT;
    return guard_rows(err, h, dev, (size_t)h->db.B * nrhs, vx, "vx", vy, dg, db, side, info);
}

// the range shape (*_jacobian; duals: *_jacobian_duals, whose blocks have ndual() rows per instance and are called Jyg, Jyb)
template <class H>
int guard_range(std::string& err, H* h, bool dev, bool duals, int first, int count, double* Jg, double* Jb, int* side, int* info)
{
    if (!h) return null_handle(dev);
    if (!Jg || first < 0 || count < 1 || first > h->db.B - count) return LCQP_INVALID_ARGUMENT;
    if (!h->rs.solved) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (!dev) return 0;
    HIPCHK(err, hipSetDevice(h->device));
    const size_t n = h->db.n, nd = h->ndual(), c = count, rows = duals ? nd : n;
    if (!device_pointer_ok(err, h, duals ? "Jyg" : "Jg", Jg, sizeof(double) * c * rows * n) || !device_pointer_ok(err, h, duals ? "Jyb" : "Jb", Jb, sizeof(double) * c * rows * nd) ||
        !device_pointer_ok(err, h, "side", side, sizeof(int) * c * nd, 4) || !device_pointer_ok(err, h, "info", info, sizeof(int) * c, 4)) return LCQP_INVALID_ARGUMENT;
    return 0;
}

// The body of a sensitivity entry point behind its guard.  A host call's body adds the kernel time of its launches to ms, and the sum becomes
// rs.sensMs.  The device-pointer twin runs the same body between the two halves of the hand-over (device_call); there the times stay in the
// events (sensPending, pendingMs) and ms is not read.
template <class H, class F>
int sens_body(std::string& err, H* h, bool dev, void* stream, F body)
{
    float ms = 0.f;
    if (dev) return device_call(err, h, stream, [&] { return body(ms); });
    if (int rc = body(ms)) return rc;
    h->rs.sensMs = ms;
    return 0;
}

// Where an arm has only its vector kernel for a Jacobian (dense: np >= 1024; sparse: the general LDL' without its panel form): the Jacobian
// formed by the host twin (run) and copied to the caller's device arrays; waits on the host
template <class H, class R>
int jacobian_through_host(std::string& err, H* h, size_t nd, size_t count, size_t rows, double* Jg, double* Jb, int* side, int* info, R run)
{
    const size_t n = h->db.n;
    std::vector<double> G(count * rows * n), Bd(Jb ? count * rows * nd : 0);
    std::vector<int> sd(count * nd), in(count);
    if (int rc = run(G.data(), Jb ? Bd.data() : nullptr, sd.data(), in.data())) return rc;
    HIPCHK(err, hipMemcpyAsync(Jg, G.data(), sizeof(double) * G.size(), hipMemcpyHostToDevice, h->stream));
    if (Jb) HIPCHK(err, hipMemcpyAsync(Jb, Bd.data(), sizeof(double) * Bd.size(), hipMemcpyHostToDevice, h->stream));
    if (side) HIPCHK(err, hipMemcpyAsync(side, sd.data(), sizeof(int) * sd.size(), hipMemcpyHostToDevice, h->stream));
    if (info) HIPCHK(err, hipMemcpyAsync(info, in.data(), sizeof(int) * in.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(err, hipStreamSynchronize(h->stream));
    return 0;
}

#pragma GCC visibility pop
}  // namespace lcqp_rt
