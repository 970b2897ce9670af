// lcqp_hip.hip -- the dense arm's batch: the process-wide entry points, the choice of launch table and build (dense_kernels, run_kernels)
// and the life cycle of the batch handle in the C ABI lcqp_hip_batch_* (gfx950 only; see include/lcqp_hip.h): create, load, setup, run,
// update, update_matrices, resolve and the readers.  Host code only, no kernel.  Differentiation -- the sensitivity, Jacobian and adjoint entry points, their
// device-pointer twins and the two adjoint kernels -- is lcqp_hip_diff.hip; the QP object is lcqp_hip_qp.hip, the building blocks and CSC
// utilities lcqp_hip_util.hip; lcqp_hip_batch.hpp is what the units share.
#include "lcqp_hip_batch.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace lcqp;
using namespace lcqp_rt;

// HIP maps the streams of a process onto a few hardware queues -- 4 unless GPU_MAX_HW_QUEUES says otherwise -- and every batch object has
// two streams: a process that keeps three batch objects alive can find both slots of a BatchPipeline on ONE queue, and its batches then
// run one after the other (tools/micro/pipeline_check.py: 35 200 LCQPs/s with two objects alive, 30 750 with an idle third one, 34 800
// again with eight queues).  The library does NOT touch the environment by itself (round 6; it used to, from a constructor: that changed
// the queue count of every GPU user of the host process).  A program that wants the queues asks for them explicitly, before the first
// HIP call of the process -- the runtime reads the variable once, when it initialises: bench.py and the examples do.
// Returns 0 when the variable was set, 1 when the caller's environment already holds a value (left alone), LCQP_HIP_ERROR on a bad count.
extern "C" int lcqp_hip_request_hw_queues(int n)
{
    if (n < 1 || n > 64) return LCQP_HIP_ERROR;
    if (getenv("GPU_MAX_HW_QUEUES")) return 1;
    char buf[16];
    snprintf(buf, sizeof buf, "%d", n);
    return setenv("GPU_MAX_HW_QUEUES", buf, /*overwrite=*/0) == 0 ? 0 : LCQP_HIP_ERROR;
}

static thread_local std::string g_err;      // the dense, QP, util and CSC entry points (lcqp_host_rt.hpp: HIPCHK(g_err, ...))
std::string& dense_err() { return g_err; }  // the slot for the other units of the arm

extern "C" const char* lcqp_hip_last_error(void) { return g_err.c_str(); }
extern "C" int lcqp_hip_device_count(void)
{ return guarded(g_err, [&] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}); }

extern "C" void lcqp_hip_options_default(lcqp_options_t* o)
{   // src/Options.cpp:296-333
    memset(o, 0, sizeof(*o));
    const double EPS = 2.221e-16;   // include/Utilities.hpp:350
    o->complementarityTolerance = 1.0e3 * EPS;
    o->stationarityTolerance = 1.0e6 * EPS;
    o->initialPenaltyParameter = 0.01;
    o->penaltyUpdateFactor = 2.0;
    o->maxPenaltyParameter = 1e8;
    o->etaDynamicPenalty = 0.9;
    o->solveZeroPenaltyFirst = 1;
    o->perturbStep = 1;
    o->maxIterations = 1000;
    o->nDynamicPenalty = 3;
    o->printLevel = 2;
    o->storeSteps = 0;
    o->perturbSeed = 0x5EEDULL;
    o->admmRho = 0.1; o->admmSigma = 1e-6; o->admmAlpha = 1.6; o->rhoEqMult = 1e3;
    o->proxSmall = 1e-12; o->proxBig = 1e-8; o->pivotThreshold = 1e-7; o->depTau = 1e-12;
    o->feasTol = 1e-9; o->resTol = 1e-12;
    o->admmFirst = 0; o->admmHot = 0; o->maxTrials = 16; o->maxRounds = 40;      // maxTrials: 12 until round 3 -- cold starts of the synthetic workload need up to 14 trials, and a polish that runs out of trials costs an ADMM round (the factor L_K, ten iterations, a second cold polish): those instances were the tail of the launch
}

// The launch table of a padded size (lcqp_launch.hpp), or null with a message: a size whose kernels this build does not link is an error,
// never another size's kernels (their buffers have another pitch).  -DLCQP_ONLY_NCH=k (the profile library, experiment builds: tools/gpu_ab.py)
// links the kernels of one padded size only.
const SizeKernels* dense_kernels(int nch)
{
#ifdef LCQP_ONLY_NCH
    static const SizeKernels* const sizes[] = {&size_kernels<LCQP_ONLY_NCH>()};
#else
    static const SizeKernels* const sizes[] = {&size_kernels<1>(), &size_kernels<2>(), &size_kernels<3>(), &size_kernels<4>(),
                                               &size_kernels<8>(), &size_kernels<16>(), &size_kernels<32>()};
#endif
    for (const SizeKernels* k : sizes) if (k->nch == nch) return k;
    g_err = "the dense kernels of the padded size " + std::to_string(128 * nch) + " are not part of this build of the library; it holds the padded sizes";
    for (const SizeKernels* k : sizes) g_err += " " + std::to_string(128 * k->nch);
    return nullptr;
}

// The build of the two persistent kernels a launch of the batch takes: the second one (256 registers) for np <= 512 (36 KB of LDS per
// workgroup) and at most three workgroups per CU, the standard one otherwise
const RunKernels& run_kernels(const lcqp_hip_batch* h)
{
    const bool few = h->nch <= 4 && h->db.B <= 3 * h->numCU && !h->overlapped && h->k->few;
    return few ? *h->k->few : h->k->run;
}

// k_lcqp_run on the whole batch: a batch that holds one set of matrices takes the builds that read instance 0's matrix blocks
static void launch_homotopy(lcqp_hip_batch* h)
{
    const RunKernels& rk = run_kernels(h);
    if (!h->db.shared) rk.lcqp_run(h->db, h->db.B, h->stream);
    else (&rk == &h->k->run ? h->k->shared_run : h->k->shared_run_few)(h->db, h->db.B, h->stream);
}

// shared: the batch holds ONE Q, A, L, R -- every pool of blocks that depend on the matrices, the box pattern and the options alone has one
// block, instance 0's (DevBatch::shared, matrix_instance); what an instance writes during a solve is [B] as ever
static lcqp_hip_batch_t* create_batch(int batch, int nV, int nC, int nComp, int withBox, int device, bool shared)
{ return guarded(g_err, [&]() -> lcqp_hip_batch_t* {
    if (batch <= 0 || nV <= 0 || nC < 0 || nComp < 0) { g_err = "invalid dimensions"; return nullptr; }
    if (nV > 4096) { g_err = "nV > 4096 is not supported by the dense kernels of this build (padded sizes 128 ... 4096; the sparse engine takes larger banded / bordered problems)"; return nullptr; }
    const SizeKernels* kernels = dense_kernels(padded_nch(nV));
    if (!kernels) return nullptr;
    if (hipError_t e = hipSetDevice(device)) { hip_fail(g_err, "hipSetDevice(device)", e); return nullptr; }
    std::unique_ptr<lcqp_hip_batch> h(new lcqp_hip_batch(device));
    for (hipError_t e : {h->stream.status, h->side.status, h->ev0.status, h->ev1.status, h->ev2.status, h->evFork.status, h->evJoin.status, h->evIn.status, h->evOut.status})
        if (e != hipSuccess) { hip_fail(g_err, "stream/event creation", e); return nullptr; }
    { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) h->numCU = cu; }
    DevBatch& d = h->db;
    d.shared = shared ? 1 : 0;
    d.B = batch; d.n = nV; d.nC = nC; d.nComp = nComp; d.mA = nC + 2 * nComp;
    h->k = kernels;
    h->nch = kernels->nch;        // 512 < nV <= 1024 runs the np = 1024 instantiation; 1024 < nV <= 2048: np = 2048 (96 KiB of LDS, one workgroup per CU, one row in flight per wave)
    d.np = 128 * h->nch;
    d.nblk = d.np / 64;
    d.boxcap = withBox ? nV : 0;
    d.mEcap = d.mA + d.boxcap;
    if (d.mEcap < 1) d.mEcap = 1;
    int capNa = 2 * nV > 64 ? 2 * nV : 64;      // active rows the Gram factor has room for (qp_polish)
    if (capNa > d.mEcap) capNa = d.mEcap;
    if (capNa > max_active(h->nch)) capNa = max_active(h->nch);
    d.capS = ((capNa + 63) / 64) * 64;
    if (d.capS < 64) d.capS = 64;
    d.nd = nV + d.mA;
    d.mMld = ((d.mEcap + 63) / 64) * 64;
    d.capC = 8 * d.np;                                     // C goes into compressed rows when it has at most 8 non-zeros per row on average
    lcqp_hip_options_default(&d.opt);
    const size_t B = batch, np = d.np, mE = d.mEcap, nLR = nComp ? nComp : 1;
    const size_t Bm = shared ? 1 : B;      // blocks of a matrix pool
    DevMem& m = h->mem;      // zero-filled on the batch's stream
    // every pool is counted where it is allocated (lcqp_hip_batch_device_bytes): `mat` a matrix pool -- Bm blocks, held once in a shared
    // batch --, `inst` a pool with one block per instance.  (The trace buffers of set_options, the staging of the loads and the sensitivity
    // buffers come and go with their calls and are not counted.)
    auto mat = [&](auto*& p, size_t per) {
        const size_t bytes = Bm * per * sizeof(*p);
        h->bytesAll += bytes; if (shared) h->bytesOnce += bytes;
        return m.alloc(g_err, p, Bm * per);
    };
    auto inst = [&](auto*& p, size_t per) {
        h->bytesAll += B * per * sizeof(*p);
        return m.alloc(g_err, p, B * per);
    };
    const size_t cS = d.capS, nd = d.nd;
    const bool ok = mat(d.Q, np * np) && mat(d.C, np * np) && mat(d.E, mE * np) &&
                    mat(d.Et, mE * np) && mat(d.F1, np * np) && inst(d.FK, np * np) &&
                    inst(d.S, cS * cS) && mat(d.MM, (size_t)d.mMld * d.mMld) && inst(d.crow, cS) &&
                    mat(d.Cp, np + 1) && mat(d.Ci, (size_t)d.capC) && mat(d.Cv, (size_t)d.capC) &&
                    inst(d.S2, cS * cS) && inst(d.DS, (cS / 64) * 4096) &&
                    mat(d.D1, (size_t)d.nblk * 4096) && inst(d.dscr, 4096) && inst(d.nv, V_NUM * np) &&
                    inst(d.mv, M_NUM * mE) && inst(d.sv, S_NUM * cS) && inst(d.mi, I_NUM * mE) &&
                    inst(d.idx, cS) && inst(d.boxidx, np) && inst(d.lbL, nLR) &&
                    inst(d.lbR, nLR) && inst(d.yk, nd) && inst(d.y0, nd) &&
                    inst(d.xout, (size_t)nV) && inst(d.yout, nd) && inst(d.stats, 1) &&
                    inst(d.info, 1) && inst(d.prof, 16);
    if (!ok || !inst(h->rs.rhoStart, 1)) return nullptr;
    h->rs.filled.assign(B, 0); h->boxed.assign(B * (size_t)nV, 0); h->boxSet.assign((size_t)nV, 0);
    if (hipError_t e = hipStreamSynchronize(h->stream)) { hip_fail(g_err, "hipStreamSynchronize(h->stream)", e); return nullptr; }
    return h.release();
}, nullptr); }

extern "C" lcqp_hip_batch_t* lcqp_hip_batch_create(int batch, int nV, int nC, int nComp, int withBox, int device)
{
    return create_batch(batch, nV, nC, nComp, withBox, device, false);
}

extern "C" lcqp_hip_batch_t* lcqp_hip_batch_create_shared(int batch, int nV, int nC, int nComp, int withBox, int device)
{
    return create_batch(batch, nV, nC, nComp, withBox, device, true);
}

extern "C" int lcqp_hip_batch_device_bytes(lcqp_hip_batch_t* h, size_t out[2])
{
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (!out) return LCQP_INVALID_ARGUMENT;
    out[0] = h->bytesAll; out[1] = h->bytesOnce;
    return 0;
}

extern "C" void lcqp_hip_batch_destroy(lcqp_hip_batch_t* h)
{
    guarded(g_err, [&] { delete h; });      // ~lcqp_hip_batch: set the device, synchronise, then the members
}

// storeSteps: the first 1024 iterates
extern "C" int lcqp_hip_batch_set_options(lcqp_hip_batch_t* h, const lcqp_options_t* opt)
{ return guarded(g_err, [&] {
    if (h) h->rs.invalidate();      // the scales of the ADMM weights and the proximal shifts of the factors come from the options
    return set_options(g_err, h, opt, 1024);
}); }

extern "C" int lcqp_hip_batch_get_trace(lcqp_hip_batch_t* h, int instance, int cap, double* scalars, double* x, int* len)
{
    return guarded(g_err, [&] { return get_trace(g_err, h, instance, cap, scalars, x, len); });
}

// diagnostic builds (-DLCQP_PROFILE): per-instance cycle counters of the megakernel's phases, [B][16]
extern "C" int lcqp_hip_batch_read_profile(lcqp_hip_batch_t* h, unsigned long long* out)
{ return guarded(g_err, [&] {
    if (!h || !out) return LCQP_INVALID_ARGUMENT;
    if (int rc = synchronize(g_err, h)) return rc;
    HIPCHK(g_err, hipMemcpy(out, h->db.prof, sizeof(unsigned long long) * (size_t)h->db.B * 16, hipMemcpyDeviceToHost));
    return 0;
}); }

extern "C" void* lcqp_hip_batch_stream(lcqp_hip_batch_t* h) { return h ? (void*)h->stream.s : nullptr; }

// The host load and update are the device path behind an upload: the caller's arrays (v, and for a load Q, A, L, R: host memory, [count][..]
// each, null: absent) go to the device in chunks of instances, and dense_pack -- the kernels of lcqp_hip_batch_load_device / _update_device --
// builds the pools of [first, first + count) from them.  Synchronous: the arrays are free on return.
static int dense_upload(lcqp_hip_batch* h, int first, int count, const PackVectors& v, const double* Q, const double* A, const double* L,
                        const double* R, bool update)
{
    const DevBatch& d = h->db;
    const size_t n = d.n, nC = d.nC, nComp = d.nComp, nd = d.nd;
    const RawArray raw[] = {{v.g, n}, {v.lbL, nComp}, {v.ubL, nComp}, {v.lbR, nComp}, {v.ubR, nComp}, {v.lbA, nC}, {v.ubA, nC}, {v.lb, n}, {v.ub, n},
                            {v.x0, n}, {v.y0, nd}, {Q, n * n}, {A, nC * n}, {L, nComp * n}, {R, nComp * n}};
    return upload_packed(g_err, h, count, raw, [&](int c0, int cb, const double* const* p) {
        return dense_pack(h, first + c0, cb, PackVectors{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10]},
                          PackMatrices{{p[11], p[12], p[13], p[14]}, {n * n, nC * n, nComp * n, nComp * n}}, update);
    });
}

// the one set of matrices of a shared batch from host arrays ([rows][nV] each, null: the block stays): the upload of one instance and
// k_pack_matrices on instance 0, whose blocks are the batch's.  boxRows: as dense_pack_matrices.
static int shared_upload_matrices(lcqp_hip_batch* h, const double* Q, const double* L, const double* R, const double* A, bool boxRows)
{
    const DevBatch& d = h->db;
    const size_t n = d.n, nC = d.nC, nComp = d.nComp;
    const RawArray raw[] = {{Q, n * n}, {A, nC * n}, {L, nComp * n}, {R, nComp * n}};
    return upload_packed(g_err, h, 1, raw, [&](int, int, const double* const* p) {
        return dense_pack_matrices(h, 0, 1, PackMatrices{{p[0], p[1], p[2], p[3]}, {n * n, nC * n, nComp * n, nComp * n}}, boxRows);
    });
}

extern "C" int lcqp_hip_batch_load(lcqp_hip_batch_t* h, int first, int count,
                                   const double* Q, const double* g, const double* L, const double* R,
                                   const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                                   const double* A, const double* lbA, const double* ubA,
                                   const double* lb, const double* ub, const double* x0, const double* y0)
{ return guarded(g_err, [&] {
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    DevBatch& d = h->db;
    const size_t n = d.n, nC = d.nC, nComp = d.nComp;
    if (first < 0 || count <= 0 || first > d.B - count) return LCQP_INVALID_ARGUMENT;
    // a batch that holds one set of matrices: Q, A, L, R are ONE [rows][nV] array each and replace the batch's, NULL keeps the one in place
    const int given = given_matrices(Q, nC ? A : nullptr, L, R);
    if (d.shared) {
        if (!g) return shared_matrices_present(h, given) == LCQP_INVALID_ARGUMENT ? LCQP_INVALID_ARGUMENT : LCQP_INVALID_OBJECTIVE_LINEAR_TERM;
        if (int rc = shared_matrices_present(h, given)) return rc;
    } else {
    if (!Q) return LCQP_INVALID_ARGUMENT;
    if (!g) return LCQP_INVALID_OBJECTIVE_LINEAR_TERM;               // include/LCQProblem.ipp:44-45
    if (!A && nC > 0) return LCQP_INVALID_CONSTRAINT_MATRIX;         // src/LCQProblem.cpp:569-570
    if (!L || !R) return LCQP_INVALID_COMPLEMENTARITY_MATRIX;        // :611-612
    }
    if ((lb || ub) && d.boxcap == 0) { g_err = "batch was created without box-bound capacity"; return LCQP_INVALID_ARGUMENT; }
    if (int rc = check_lower_bounds((size_t)count * nComp, lbL, lbR)) return rc;      // the last check: from here on the range is written
    std::vector<char> boxSet;
    if (d.shared) {      // (the last check of a shared batch: one set of box-bounded variables)
        std::vector<char> flags((size_t)count * n);
        for (size_t j = 0; j < flags.size(); j++) flags[j] = std::isfinite(bnd(lb, j, -INFINITY)) || std::isfinite(bnd(ub, j, INFINITY));
        if (int rc = shared_box_check(g_err, h, first, count, flags.data(), given, boxSet)) return rc;
    }
    HIPCHK(g_err, hipSetDevice(h->device));
    h->rs.invalidate();
    load_bound_flags(d, h->anyLoaded, first, lbL, lbR);
    for (size_t j = 0; j < (size_t)count * n; j++)      // setLB / setUB, include/LCQProblem.ipp:54-112
        h->boxed[(size_t)first * n + j] = std::isfinite(bnd(lb, j, -INFINITY)) || std::isfinite(bnd(ub, j, INFINITY));
    std::fill_n(h->rs.filled.begin() + first, count, 1);
    if (d.shared) {
        h->boxSet = boxSet; h->boxDefined = true; h->matsHeld |= given;
        if (given) if (int rc = shared_upload_matrices(h, Q, L, R, A, true)) return rc;
        if (int rc = dense_upload(h, first, count, PackVectors{g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0}, nullptr, nullptr, nullptr, nullptr, false)) return rc;
    }
    else if (int rc = dense_upload(h, first, count, PackVectors{g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0}, Q, A, L, R, false)) return rc;
    h->anyLoaded = true;
    return 0;
}); }

extern "C" int lcqp_hip_batch_generate_synthetic(lcqp_hip_batch_t* h, uint64_t seed0, uint64_t firstInstance)
{ return guarded(g_err, [&] {
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    HIPCHK(g_err, hipSetDevice(h->device));
    DevBatch& d = h->db;
    if (d.shared) { g_err = "generate_synthetic: the generator draws matrices per instance; this batch holds one set of matrices (lcqp_hip_batch_create_shared)"; return LCQP_INVALID_ARGUMENT; }
    if (d.nComp * 2 > d.n) { g_err = "synthetic generator needs 2*nComp <= nV"; return LCQP_INVALID_ARGUMENT; }
    d.hasLbL = d.hasLbR = 0; h->anyLoaded = true;
    h->rs.invalidate();
    std::fill(h->rs.filled.begin(), h->rs.filled.end(), 1); std::fill(h->boxed.begin(), h->boxed.end(), 0);      // no box bounds
    h->k->synth_fill(d, d.B, h->stream, seed0, firstInstance);
    h->k->synth_Q(d, d.B * (d.nblk * (d.nblk + 1) / 2), h->stream);
    HIPCHK(g_err, hipGetLastError());
    return 0;
}); }

extern "C" int lcqp_hip_batch_read_problem(lcqp_hip_batch_t* h, int b, double* Q, double* g, double* L, double* R,
                                           double* A, double* lbA, double* ubA)
{ return guarded(g_err, [&] {
    if (!h || b < 0 || b >= h->db.B) return LCQP_INVALID_ARGUMENT;
    if (int rc = synchronize(g_err, h)) return rc;
    DevBatch& d = h->db;
    const int n = d.n, nC = d.nC, nComp = d.nComp, np = d.np, mE = d.mEcap;
    std::vector<double> Qp((size_t)np * np), Ep((size_t)mE * np), nvb((size_t)V_NUM * np), mvb((size_t)M_NUM * mE);
    const size_t mb = matrix_instance(d, b);
    HIPCHK(g_err, hipMemcpy(Qp.data(), d.Q + mb * np * np, sizeof(double) * np * np, hipMemcpyDeviceToHost));
    HIPCHK(g_err, hipMemcpy(Ep.data(), d.E + mb * mE * np, sizeof(double) * mE * np, hipMemcpyDeviceToHost));
    HIPCHK(g_err, hipMemcpy(nvb.data(), d.nv + (size_t)b * V_NUM * np, sizeof(double) * V_NUM * np, hipMemcpyDeviceToHost));
    HIPCHK(g_err, hipMemcpy(mvb.data(), d.mv + (size_t)b * M_NUM * mE, sizeof(double) * M_NUM * mE, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        if (Q) memcpy(Q + (size_t)i * n, &Qp[(size_t)i * np], sizeof(double) * n);
        if (g) g[i] = nvb[(size_t)V_G * np + i];
    }
    for (int r = 0; r < nC; r++) {
        if (A) memcpy(A + (size_t)r * n, &Ep[(size_t)r * np], sizeof(double) * n);
        if (lbA) lbA[r] = mvb[(size_t)M_L * mE + r];
        if (ubA) ubA[r] = mvb[(size_t)M_U * mE + r];
    }
    for (int r = 0; r < nComp; r++) {
        if (L) memcpy(L + (size_t)r * n, &Ep[(size_t)(nC + r) * np], sizeof(double) * n);
        if (R) memcpy(R + (size_t)r * n, &Ep[(size_t)(nC + nComp + r) * np], sizeof(double) * n);
    }
    return 0;
}); }

// the setup kernels of the batch on its stream, the C branch on the side stream.  warm: k_prepare_warm stands where k_prepare stands --
// the matrices changed under a stored point (lcqp_hip_batch_update_matrices); rho0 [B] on the device, or null
int launch_setup(lcqp_hip_batch* h, bool warm, const double* rho0)
{
    const DevBatch& d = h->db;
    const SizeKernels& k = *h->k;
    hipStream_t on = h->stream;
    h->rs.invalidate();
    h->rs.nSetups++;
    const int ntile = d.nblk * (d.nblk + 1) / 2;
    const int nrb = (d.mEcap + 63) / 64, nb = (d.mMld + 127) / 128, nmt = nb * (nb + 1);      // k_build_M: 128 x 64 tiles of the lower triangle
    // a batch that holds one set of matrices: the chain below on a grid of ONE matrix instance (instance 0's blocks are the batch's), the
    // matrix half of k_prepare in front of it, and behind it k_share_setup over the batch -- the marks of the chain and the vector half
    const int nI = d.shared ? 1 : d.B;
    if (d.shared) {
        int src = 0;      // the lowest instance that holds a problem: its list of box-bounded variables is the batch's
        while (src < d.B - 1 && !h->rs.filled[src]) src++;
        if (!h->rs.filled[src]) src = 0;
        k.prepare_shared(d, on, src);
    }
    else if (warm) k.prepare_warm(d, d.B, on, rho0);
    else k.prepare(d, d.B, on);
    // C and its compressed rows depend on L and R only, the chain L1 -> Et -> M on Q and E: two branches.  The short one goes to the side
    // stream and runs in the gaps of k_factor (one workgroup per instance, a life of dependent chains).  Measured alternatives, round 6
    // (profiles/round6/README.md): the side branch beside k_trsm, or beside k_trsm and k_build_M -- both 0.2 ms slower.
    const bool fork = d.nComp > 0;
    if (fork) {
        HIPCHK(g_err, hipEventRecord(h->evFork, on));
        HIPCHK(g_err, hipStreamWaitEvent(h->side, h->evFork, 0));
        k.build_C(d, nI * ntile, h->side);
        k.compress_C(d, nI, h->side);
        HIPCHK(g_err, hipEventRecord(h->evJoin, h->side));
    }
    // more than three workgroups per CU (np <= 256: 36 KB of LDS each): the instantiation held to 128 registers, so that four are resident and
    // the batch needs one round
    const BatchKernel factor = (h->nch <= 2 && nI > 3 * h->numCU) ? k.factor_full : k.factor;
    const BatchKernel trsm = h->overlapped ? k.trsm_streamed : k.trsm;
    factor(d, nI, on);
    trsm(d, nI * nrb, on);
    // the join sits in front of the last setup kernel, not behind it: an event recorded right after a stream wait carried a late time stamp
    // (the homotopy kernel appeared 2 ms shorter than rocprofv3 and the wall clock say), and the side branch has long finished by then
    if (fork) HIPCHK(g_err, hipStreamWaitEvent(on, h->evJoin, 0));
    k.build_M(d, nI * nmt, on);
    if (d.shared) k.share_setup(d, d.B, on, warm ? 1 : 0, rho0);
    HIPCHK(g_err, hipGetLastError());
    h->rs.setupValid = true;
    return 0;
}

extern "C" int lcqp_hip_batch_set_overlapped(lcqp_hip_batch_t* h, int overlapped)
{
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    h->overlapped = overlapped != 0;
    return 0;
}

extern "C" int lcqp_hip_batch_setup(lcqp_hip_batch_t* h)
{ return guarded(g_err, [&] {
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    HIPCHK(g_err, hipSetDevice(h->device));
    return launch_setup(h);
}); }

// One launch for the whole batch.  (Round 5 measured the setup of one slice of the batch beside the homotopy of the slice before, as a
// switch of this call: slower at every split -- profiles/round5/run_chunks_ab.log: 30 200 LCQPs/s in one piece, 26 800 / 27 100 / 23 100 in
// two / three / four slices, the setup kernels crawl beside a homotopy launch that saturates HBM.  The switch is gone; overlap across
// BATCHES is the product's BatchPipeline.)
extern "C" int lcqp_hip_batch_run(lcqp_hip_batch_t* h)
{ return guarded(g_err, [&] {
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    HIPCHK(g_err, hipSetDevice(h->device));
    HIPCHK(g_err, hipEventRecord(h->ev0, h->stream));
    int rc = launch_setup(h);   // the factorisations are part of runSolver's cost (initializeSolver :885)
    if (rc) return rc;
    HIPCHK(g_err, hipEventRecord(h->ev1, h->stream));
    launch_homotopy(h);
    h->rs.nLaunches++;
    HIPCHK(g_err, hipGetLastError());
    HIPCHK(g_err, hipEventRecord(h->ev2, h->stream));
    h->ran = h->rs.solved = true;
    return 0;
}); }

// New vectors for instances [first, first + count) of a batch that holds problems: everything lcqp_hip_batch_load takes except the
// matrices.  The whole range is checked before anything is written.
extern "C" int lcqp_hip_batch_update(lcqp_hip_batch_t* h, int first, int count, const double* g,
                                     const double* lbL, const double* ubL, const double* lbR, const double* ubR,
                                     const double* lbA, const double* ubA, const double* lb, const double* ub,
                                     const double* x0, const double* y0)
{ return guarded(g_err, [&] {
    if (int rc = check_update(g_err, h, first, count, g, lbL, lbR)) return rc;
    DevBatch& d = h->db;
    const int n = d.n;
    for (int k = 0; k < count; k++)
        for (int i = 0; i < n; i++) {
            const size_t j = (size_t)k * n + i;
            const bool fin = std::isfinite(bnd(lb, j, -INFINITY)) || std::isfinite(bnd(ub, j, INFINITY));
            if (fin != (h->boxed[((size_t)first + k) * n + i] != 0)) {
                g_err = box_change_message(i, first + k, fin);
                return LCQP_INVALID_ARGUMENT;
            }
        }
    HIPCHK(g_err, hipSetDevice(h->device));
    d.hasLbL |= lbL ? 1 : 0; d.hasLbR |= lbR ? 1 : 0;      // switched on, never off: whatever the order of the calls (an absent vector is the zero vector)
    return dense_upload(h, first, count, PackVectors{g, lbL, ubL, lbR, ubR, lbA, ubA, lb, ub, x0, y0}, nullptr, nullptr, nullptr, nullptr, true);
}); }

// New matrices for instances [first, first + count) of a batch that holds problems: Q, L, R, A as lcqp_hip_batch_load takes them, NULL:
// the matrix stays.  Only their blocks of the pools are written (k_pack_matrices behind the chunked upload): no vector, no InstInfo, no
// status, multiplier, point or statistic.  The whole call is checked before anything is written.
extern "C" int lcqp_hip_batch_update_matrices(lcqp_hip_batch_t* h, int first, int count, const double* Q, const double* L, const double* R,
                                              const double* A)
{ return guarded(g_err, [&] {
    if (int rc = check_update_matrices(h, first, count, Q, L, R, A)) return rc;
    const DevBatch& d = h->db;
    const size_t n = d.n, nC = d.nC, nComp = d.nComp;
    HIPCHK(g_err, hipSetDevice(h->device));
    h->rs.matrices_changed();
    if (d.shared) return shared_upload_matrices(h, Q, L, R, A, false);
    const RawArray raw[] = {{Q, n * n}, {A, nC * n}, {L, nComp * n}, {R, nComp * n}};
    return upload_packed(g_err, h, count, raw, [&](int c0, int cb, const double* const* p) {
        return dense_pack_matrices(h, first + c0, cb, PackMatrices{{p[0], p[1], p[2], p[3]}, {n * n, nC * n, nComp * n, nComp * n}}, false);
    });
}); }

// Solve again on the setup in place: k_refresh instead of the five setup kernels, then the homotopy launch.  Without a setup that belongs
// to the matrices and options in place this is lcqp_hip_batch_run -- unless the call is warm and only the matrices changed since the last
// solve (lcqp_hip_batch_update_matrices): then the five setup kernels run with k_prepare_warm in front, which keeps the stored point.
extern "C" int lcqp_hip_batch_resolve(lcqp_hip_batch_t* h, int mode, const double* rho0)
{ return guarded(g_err, [&] {
    const int chk = check_resolve(g_err, h, mode, rho0, h && h->anyLoaded);
    const bool newMatrices = chk == RESOLVE_RUNS && mode == 1 && h->rs.pointKept;
    if (chk && !newMatrices) return chk == RESOLVE_RUNS ? lcqp_hip_batch_run(h) : chk;
    const int B = h->db.B;
    HIPCHK(g_err, hipSetDevice(h->device));
    const bool withRho = mode == 1 && rho0;
    if (withRho) {
        if (int rc = h->up.reserve(g_err, sizeof(double) * (size_t)B)) return rc;
        HIPCHK(g_err, hipEventSynchronize(h->up.slot[0].done));
        memcpy(h->up.slot[0].buf, rho0, sizeof(double) * (size_t)B);
        HIPCHK(g_err, hipMemcpyAsync(h->rs.rhoStart, h->up.slot[0].buf, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, h->stream));
        HIPCHK(g_err, hipEventRecord(h->up.slot[0].done, h->stream));
    }
    HIPCHK(g_err, hipEventRecord(h->ev0, h->stream));
    if (newMatrices) {
        if (int rc = launch_setup(h, true, withRho ? h->rs.rhoStart : nullptr)) return rc;
    } else {
        h->k->refresh(h->db, B, h->stream, mode, withRho ? h->rs.rhoStart : nullptr);
        HIPCHK(g_err, hipGetLastError());
    }
    HIPCHK(g_err, hipEventRecord(h->ev1, h->stream));
    launch_homotopy(h);
    h->rs.nLaunches++;
    HIPCHK(g_err, hipGetLastError());
    HIPCHK(g_err, hipEventRecord(h->ev2, h->stream));
    h->ran = h->rs.solved = true;
    return 0;
}); }

extern "C" int lcqp_hip_batch_launch_counts(lcqp_hip_batch_t* h, int out[2])
{
    return launch_counts(h, out);
}

extern "C" int lcqp_hip_batch_synchronize(lcqp_hip_batch_t* h)
{
    return guarded(g_err, [&] { return synchronize(g_err, h); });
}

extern "C" int lcqp_hip_batch_last_timing(lcqp_hip_batch_t* h, float* setup_ms, float* solve_ms)
{
    return guarded(g_err, [&] { return last_timing(g_err, h, setup_ms, solve_ms); });
}

extern "C" int lcqp_hip_batch_get_solution(lcqp_hip_batch_t* h, double* x, double* y, lcqp_stats_t* stats)
{
    return guarded(g_err, [&] { return get_solution(g_err, h, h ? h->db.nd : 0, x, y, stats); });
}

// Algorithmic HBM bytes of the last run, from the per-instance work counters:
//   residual evaluation (trial with sweeps, stats.reserved): Q + E once   8*(n*n + m*n)
//   correction                  : L1 fwd+bwd + 2 sweeps over the nT active rows of Et + one fused pass over the inverse factor Ti (nT x ns)
//   working-set update          : the bytes of Ti read and written by row appends and rotations, and the entries of M read (summed
//                                 exactly by the kernel, InstInfo::work[2])
//   ADMM iteration              : LK fwd+bwd + two sweeps over E
//   LCQP                        : one sweep over Q and C (Q x0, C x0); per iterate C pk from compressed rows (12 B per non-zero) or by a
//                                 sweep over C; Q pk comes from the subsolver's verified residual
extern "C" double lcqp_hip_batch_algorithmic_bytes(lcqp_hip_batch_t* h)
{ return guarded(g_err, [&] {
    if (!h) return 0.0;
    DevBatch& d = h->db;
    std::vector<lcqp_stats_t> st(d.B);
    if (hipSetDevice(h->device) != hipSuccess) return 0.0;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return 0.0;
    if (hipMemcpy(st.data(), d.stats, sizeof(lcqp_stats_t) * (size_t)d.B, hipMemcpyDeviceToHost) != hipSuccess) return 0.0;
    std::vector<InstInfo> info(d.B);
    if (hipMemcpy(info.data(), d.info, sizeof(InstInfo) * (size_t)d.B, hipMemcpyDeviceToHost) != hipSuccess) return 0.0;
    const double n = d.n, m = d.mA, N = d.n;
    const double bs = 8.0 * N * (N + 2.0);
    double total = 0.0;
    for (int b = 0; b < d.B; b++) {
        // the active rows of each correction and the bytes of each working-set update are summed by the kernel (InstInfo::work), not estimated
        const double rowsEt = info[b].work[0], tiC = info[b].work[1], updBytes = info[b].work[2], nTrsv = info[b].work[5];
        total += st[b].reserved * 8.0 * n * n + 8.0 * n * info[b].work[4];   // true-residual sweeps over Q; rows of E read by both stages of the trials (hot-start trials reuse the last residual)
        total += nTrsv * 0.5 * bs + 8.0 * rowsEt * n + 8.0 * (tiC + rowsEt);   // corrections: triangular solves with L1 (two per full, one per predicted correction), rows of Et, pass over Ti
        total += updBytes;
        total += st[b].admmIter * (bs + 2.0 * 8.0 * m * n);
        total += 2.0 * 8.0 * n * n;                                                   // Q x0, C x0: the one sweep over Q and C
        total += (st[b].iterTotal + 1) * (info[b].cNnz >= 0 ? 12.0 * info[b].cNnz : 8.0 * n * n);   // C pk per LCQP iterate: compressed rows or a sweep
    }
    return total;
}, 0.0); }

extern "C" int lcqp_hip_batch_work_sums(lcqp_hip_batch_t* h, double out[6])
{ return guarded(g_err, [&] {
    if (!h || !out) return LCQP_INVALID_ARGUMENT;
    DevBatch& d = h->db;
    if (int rc = synchronize(g_err, h)) return rc;
    std::vector<InstInfo> info(d.B);
    HIPCHK(g_err, hipMemcpy(info.data(), d.info, sizeof(InstInfo) * (size_t)d.B, hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; k++) out[k] = 0.0;
    for (int b = 0; b < d.B; b++) for (int k = 0; k < 6; k++) out[k] += info[b].work[k];
    return 0;
}); }

// ---- read-back of the constant matrices and of the working-set factor (tests, diagnostics): the raw padded blocks of one instance ----
extern "C" int lcqp_hip_batch_read_setup(lcqp_hip_batch_t* h, int b, int dims[9], double scal[2], double* Cm, double* F1, double* D1,
                                         double* Et, double* MM, int* Cp, int* Ci, double* Cv)
{ return guarded(g_err, [&] {
    if (!h || b < 0 || b >= h->db.B) return LCQP_INVALID_ARGUMENT;
    if (int rc = synchronize(g_err, h)) return rc;
    HIPCHK(g_err, hipStreamSynchronize(h->side));
    const DevBatch& d = h->db;
    const size_t np = d.np, mE = d.mEcap, ld = d.mMld;
    InstInfo info;
    HIPCHK(g_err, hipMemcpy(&info, d.info + b, sizeof(InstInfo), hipMemcpyDeviceToHost));
    const size_t ib = matrix_instance(d, b);      // every block below is a matrix block
    if (dims) {
        const int v[9] = {d.np, d.nblk, d.mEcap, d.mMld, d.capS, d.capC, info.mE, info.cNnz, info.setupFail};
        memcpy(dims, v, sizeof v);
    }
    if (scal) { scal[0] = info.spv; scal[1] = info.scale; }
    int rc = read_back(g_err, Cm, d.C + ib * np * np, np * np);
    if (!rc) rc = read_back(g_err, F1, d.F1 + ib * np * np, np * np);
    if (!rc) rc = read_back(g_err, D1, d.D1 + ib * d.nblk * 4096, (size_t)d.nblk * 4096);
    if (!rc) rc = read_back(g_err, Et, d.Et + ib * mE * np, mE * np);
    if (!rc) rc = read_back(g_err, MM, d.MM + ib * ld * ld, ld * ld);
    if (!rc) rc = read_back(g_err, Cp, d.Cp + ib * (np + 1), np + 1);
    if (!rc) rc = read_back(g_err, Ci, d.Ci + ib * d.capC, (size_t)d.capC);
    if (!rc) rc = read_back(g_err, Cv, d.Cv + ib * d.capC, (size_t)d.capC);
    return rc;
}); }

extern "C" int lcqp_hip_batch_read_working_set(lcqp_hip_batch_t* h, int b, int dims[2], int* slot_row, int* crow, int* row_slot, double* Ti)
{ return guarded(g_err, [&] {
    if (!h || b < 0 || b >= h->db.B) return LCQP_INVALID_ARGUMENT;
    if (int rc = synchronize(g_err, h)) return rc;
    const DevBatch& d = h->db;
    const size_t ib = b, capS = d.capS;
    InstInfo info;
    HIPCHK(g_err, hipMemcpy(&info, d.info + ib, sizeof(InstInfo), hipMemcpyDeviceToHost));
    if (dims) { dims[0] = info.nT; dims[1] = info.ns; }
    int rc = read_back(g_err, slot_row, d.idx + ib * capS, capS);
    if (!rc) rc = read_back(g_err, crow, d.crow + ib * capS, capS);
    if (!rc) rc = read_back(g_err, row_slot, d.mi + ib * I_NUM * d.mEcap + (size_t)I_SLOT * d.mEcap, (size_t)info.mE);
    if (!rc) rc = read_back(g_err, Ti, d.S + ib * capS * capS, capS * capS);
    return rc;
}); }
