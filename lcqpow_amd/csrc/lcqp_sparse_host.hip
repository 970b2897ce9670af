// lcqp_sparse_host.hip -- the life cycle of the sparse arm's handle in the C ABI lcqp_hip_sparse_* (include/lcqp_hip.h): the pattern
// analysis (lcqp_sparse_pattern.hpp) and the storage of a batch in create, load / update / run / resolve, the readers and probes, and the
// LCQP_SPARSE_* environment test hooks.  Host code only, no kernel: the kernels of the solver are in lcqp_sparse.hip, one translation unit per
// lane-group width G, reached through the launch tables of lcqp_sparse_launch.hpp (sp_kernels).  Differentiation -- sensitivities, panels,
// Jacobians, the full adjoint and their device-pointer twins -- is lcqp_sparse_diff.hip; the device-pointer load / update / solution and
// their kernels are lcqp_sparse_device.hip; lcqp_sparse_batch.hpp holds what the three units share.
#include "lcqp_sparse_batch.hpp"
#include "lcqp_sparse_pattern.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace lcqp_rt;
using namespace lcqp_sparse;

static thread_local std::string g_sp_err;
std::string& sparse_err() { return g_sp_err; }
extern "C" const char* lcqp_hip_sparse_last_error(void) { return g_sp_err.c_str(); }

// Ordering [1] and the light regularisation of the polish are for batches whose Hessians are safely definite, judged by their diagonals
// (min Q_ii >= 1e-6 max Q_ii in every loaded instance); the pivot check of sp_polish covers what the diagonals do not show.
void sp_choose_ordering(lcqp_hip_sparse* h)
{
    bool definite = h->loaded;      // nothing loaded yet: the plain ordering
    for (double r : h->diagRatio) definite = definite && (r >= 1e-6);
    const int k = (definite && h->hasB) ? 1 : 0;
    const lcqp_hip_sparse::Ord& o = h->ord[k];
    SpBatch& d = h->db;
    d.iperm = o.iperm; d.bandQ = o.bandQ; d.bandE = o.bandE; d.bsrc = o.bsrc; d.bgate = o.bgate; d.bdiag = o.bdiag; d.pnode = o.pnode; d.Upos = o.Upos;
    d.lightOK = (definite && o.rowsFollow) ? 1 : 0;
    h->useB = k;
}

// the launch table of a lane-group width, one per kernel translation unit; null for a width that has none (the pattern analysis gives 8,
// 16, 32 or 64, and create refuses anything else)
const SpKernels* sp_kernels(int G)
{
    static const SpKernels* const units[] = {&sparse_kernels<8>(), &sparse_kernels<16>(), &sparse_kernels<32>(), &sparse_kernels<64>()};
    for (const SpKernels* u : units) if (u->G == G) return u;
    return nullptr;
}

// the pattern analysis (lcqp_sparse_pattern.hpp), then the device copies of its arrays and the storage of the batch
extern "C" lcqp_hip_sparse_t* lcqp_hip_sparse_create(int batch, int nV, int nC, int nComp, const int* Qp, const int* Qi, const int* Ap, const int* Ai, int device)
{ return guarded(g_sp_err, [&]() -> lcqp_hip_sparse_t* {
    if (batch <= 0 || nV <= 0 || nC < 0 || nComp <= 0 || !Qp || !Qi || !Ap || !Ai) { g_sp_err = "invalid arguments"; return nullptr; }
    lcqp_pattern::Hooks hooks;
    if (const char* e = std::getenv("LCQP_SPARSE_GENERAL")) hooks.general = std::atoi(e) == 1;      // test hook: the general LDL' on a pattern the band engine would take
    if (const char* e = std::getenv("LCQP_SPARSE_LANES")) hooks.lanes = std::atoi(e);               // test hook: a wider lane group than the band needs
    if (const char* e = std::getenv("LCQP_SPARSE_ORDERING"))                                          // test hook: the ordering of the general LDL' (nd | md)
        hooks.ordering = !std::strcmp(e, "nd") ? lcqp_pattern::ORDER_ND : (!std::strcmp(e, "md") ? lcqp_pattern::ORDER_MD : 0);
    lcqp_pattern::Pattern P;
    if (!lcqp_pattern::analyse_pattern(nV, nC, nComp, Qp, Qi, Ap, Ai, hooks, P, g_sp_err)) { g_sp_err += P.note; return nullptr; }
    const int n = P.n, m = P.m, N = P.N, nnzQ = P.nnzQ, nnzA = P.nnzE, w = P.w, G = P.G, ld = G, kb = P.kb;
    const int nU = (int)P.Usrc.size(), nCb = (int)P.Csrc.size();
    const bool general = P.general;
    if (!sp_kernels(G)) { g_sp_err = "the pattern analysis chose a lane-group width that has no kernel unit"; return nullptr; }
    const lcqp_general::Symbolic& sym = P.sym;
    if (hipError_t e = hipSetDevice(device)) { hip_fail(g_sp_err, "hipSetDevice failed", e); return nullptr; }
    std::unique_ptr<lcqp_hip_sparse> h(new lcqp_hip_sparse(device));
    for (hipError_t e : {h->stream.status, h->ev0.status, h->ev1.status, h->ev2.status, h->evIn.status, h->evOut.status})
        if (e != hipSuccess) { hip_fail(g_sp_err, "stream/event creation", e); return nullptr; }
    if (hipError_t e = hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device)) { hip_fail(g_sp_err, "hipDeviceGetAttribute(multiprocessor count)", e); return nullptr; }
    h->csr2csc = P.csr2csc; h->hasB = P.hasB; h->generalOrdering = general ? P.ordering : 0; h->qdiagHost = P.qdiag; h->diagRatio.assign(batch, 1.0); h->rs.filled.assign(batch, 0);
    SpBatch& d = h->db;
    d.B = batch; d.n = n; d.m = m; d.nC = nC; d.nComp = nComp; d.N = N; d.Np = ((N + 63) / 64) * 64; d.w = w; d.ld = ld; d.nnzQ = nnzQ; d.nnzE = nnzA; d.G = G; d.kb = kb; d.nU = nU; d.nCb = nCb;
    d.general = general ? 1 : 0;
    d.kfStride = general ? (size_t)sym.Lsize : (size_t)d.Np * G;
    if (general) { d.gnF = sym.nF; d.gMaxFront = sym.maxFront; d.gLsize = (unsigned)sym.Lsize; d.gStackSize = (unsigned)std::max<long long>(sym.stackSize, 1); d.w = 0; }
    d.bitWords = (G <= 16 && (size_t)(64 / G) * ((m + 31) / 32) * sizeof(unsigned) <= 16384) ? (m + 31) / 32 : 0;      // at most 16 KB of LDS per wavefront
    if (const char* e = std::getenv("LCQP_SPARSE_NOBITS")) { if (std::atoi(e) == 1) d.bitWords = 0; }                    // test hook: the path of problems with more rows than that
    {   // algorithmic bytes per event (what each event has to read and write once: 8-byte values, 4-byte indices)
        const double dN = N, dq = nnzQ, de = nnzA, Nb = N - kb;
        d.by[BY_ASSEMBLE] = 8.0 * (dN * ld + dq + de) + 4.0 * (dq + de);
        d.by[BY_FACTOR_LDS] = 8.0 * (3.0 * dN * (w + 1));
        d.by[BY_FACTOR] = 12.0 * (dq + de) + 8.0 * dN * (w + 2);
        d.by[BY_SOLVE] = 8.0 * (2.0 * dN * w + 4.0 * dN);
        d.by[BY_BORDER_PREPARE] = 8.0 * (2.0 * (double)nU + (double)kb * d.Np);
        d.by[BY_BORDER_SOLVE] = 8.0 * ((double)kb * Nb + 2.0 * Nb + nU);
        d.by[BY_EX] = 12.0 * de + 8.0 * (n + m);
        d.by[BY_SWEEP] = 12.0 * (dq + de) + 8.0 * (3.0 * n + m);
        d.by[BY_START] = 12.0 * dq + 2.0 * 12.0 * de;
        d.by[BY_E] = 12.0 * de;
        if (general) {      // a factorisation reads every value of Q and E once and writes the panels and 1 / D; a solve reads the panels twice
            d.by[BY_FACTOR] = 12.0 * (dq + de) + 8.0 * ((double)sym.Lsize + dN);
            d.by[BY_SOLVE] = 8.0 * (2.0 * (double)sym.Lsize + 4.0 * dN);
        }
    }
    const size_t Np = d.Np;
    lcqp_hip_options_default(&d.opt);
    const size_t B = batch;
    DevMem& mm = h->mem;
    std::string& err = g_sp_err;
    bool ok = mm.alloc(err, d.Qp, n + 1, Qp) && mm.alloc(err, d.Qi, nnzQ, Qi) && mm.alloc(err, d.Ep, m + 1, P.Ep.data()) &&
         mm.alloc(err, d.Ei, nnzA, P.Ei.data()) && mm.alloc(err, d.ETp, n + 1, P.ETp.data()) && mm.alloc(err, d.ETi, nnzA, P.ETi.data()) &&
         mm.alloc(err, d.ETmap, nnzA, P.ETmap.data()) &&
         mm.alloc(err, d.qdiag, n, P.qdiag.data()) && mm.alloc(err, d.Erow, nnzA, P.Erow.data());
    for (int k = 0; k < (P.hasB ? 2 : 1); k++) {
        const lcqp_pattern::Ordering& M = P.ord[k];
        lcqp_hip_sparse::Ord& o = h->ord[k];
        ok = ok && mm.alloc(err, o.iperm, N, M.iperm.data()) && mm.alloc(err, o.bandQ, nnzQ, M.bandQ.data()) &&
             mm.alloc(err, o.bandE, nnzA, M.bandE.data()) && mm.alloc(err, o.bsrc, M.bsrc.size(), M.bsrc.data()) &&
             mm.alloc(err, o.bgate, M.bgate.size(), M.bgate.data()) && mm.alloc(err, o.bdiag, M.bdiag.size(), M.bdiag.data()) &&
             mm.alloc(err, o.pnode, N, M.perm.data()) && mm.alloc(err, o.Upos, nU, M.Upos.data());
        o.perm = M.perm; o.rowsFollow = M.rowsFollow;
    }
    if (ok) sp_choose_ordering(h.get());
    if (kb > 0)
        ok = ok && mm.alloc(err, d.bnode, kb, P.border.data()) && mm.alloc(err, d.Uptr, kb + 1, P.Uptr.data()) &&
             mm.alloc(err, d.Usrc, nU, P.Usrc.data()) && mm.alloc(err, d.Ugate, nU, P.Ugate.data()) && mm.alloc(err, d.Cptr, kb + 1, P.Cptr.data()) &&
             mm.alloc(err, d.Cb2, nCb, P.Cb2.data()) && mm.alloc(err, d.Csrc, nCb, P.Csrc.data()) && mm.alloc(err, d.Cgate, nCb, P.Cgate.data()) &&
             mm.alloc(err, d.bW, (size_t)batch * 2 * kb * d.Np) && mm.alloc(err, d.bUv, (size_t)batch * 2 * nU) &&
             mm.alloc(err, d.bS, (size_t)batch * 2 * kb * kb);
    // ELL slabs of the three gathers (g_ell): rows of Q, rows of E, columns of E
    auto ell = [&](EllMat& e, const lcqp_pattern::Ell& s, int rows, const int* dptr, const int* didx, const int* dmap) {
        e.rows = rows; e.W = s.W; e.tails = s.tails; e.ptr = dptr; e.cidx = didx; e.cmap = dmap; e.epos = nullptr;
        return mm.alloc(err, e.eidx, s.eidx.size(), s.eidx.data()) && (s.epos.empty() || mm.alloc(err, e.epos, s.epos.size(), s.epos.data()));
    };
    ok = ok && ell(d.ellQ, P.ellQ, n, d.Qp, d.Qi, nullptr) && ell(d.ellE, P.ellE, m, d.Ep, d.Ei, nullptr) && ell(d.ellT, P.ellT, n, d.ETp, d.ETi, d.ETmap);
    ok = ok && mm.alloc(err, d.Qx, B * nnzQ) && mm.alloc(err, d.Ex, B * nnzA) &&
         mm.alloc(err, d.Kb, (G > 16 && !general) ? B * N * ld : 0) &&      // the band array is only written by the LDS-window factorisation
         mm.alloc(err, d.KaF, B * d.kfStride) && mm.alloc(err, d.KaD, B * Np) &&
         mm.alloc(err, d.KpF, B * d.kfStride) && mm.alloc(err, d.KpD, B * Np) &&
         mm.alloc(err, d.K0, G <= 16 ? B * Np * G : 0) &&
         mm.alloc(err, d.nv, B * NV_NUM * n) && mm.alloc(err, d.mv, B * MV_NUM * m) && mm.alloc(err, d.Nv, B * 2 * Np) &&
         mm.alloc(err, d.lbL, B * nComp) && mm.alloc(err, d.lbR, B * nComp) && mm.alloc(err, d.mi, B * MI_NUM * m) &&
         mm.alloc(err, d.info, B) && mm.alloc(err, d.stats, B) && mm.alloc(err, d.xout, B * n) &&
         mm.alloc(err, d.yout, B * m);
    if (general) {
        std::vector<unsigned> lo(sym.Loff.begin(), sym.Loff.end()), co(sym.CBoff.begin(), sym.CBoff.end());
        std::vector<int> meta((size_t)sym.nF * GEN_META, 0), cinfo(std::max<size_t>(sym.child.size(), 1) * 4, 0);
        for (int f = 0; f < sym.nF; f++) {
            int* mt = meta.data() + (size_t)f * GEN_META;
            mt[0] = sym.np[f]; mt[1] = sym.nb[f]; mt[2] = sym.piv0[f]; mt[3] = sym.rowPtr[f]; mt[4] = sym.asmPtr[f]; mt[5] = sym.asmPtr[f + 1];
            mt[6] = sym.childPtr[f]; mt[7] = sym.childPtr[f + 1]; mt[8] = (int)sym.Loff[f]; mt[9] = (int)sym.CBoff[f];
        }
        for (size_t ci = 0; ci < sym.child.size(); ci++) { const int ch = sym.child[ci]; cinfo[4 * ci] = sym.nb[ch]; cinfo[4 * ci + 1] = (int)sym.CBoff[ch]; cinfo[4 * ci + 2] = sym.rowPtr[ch]; }
        ok = ok && mm.alloc(err, d.gPiv0, sym.piv0.size(), sym.piv0.data()) && mm.alloc(err, d.gNp, sym.np.size(), sym.np.data()) &&
             mm.alloc(err, d.gNb, sym.nb.size(), sym.nb.data()) && mm.alloc(err, d.gRowPtr, sym.rowPtr.size(), sym.rowPtr.data()) &&
             mm.alloc(err, d.gRows, std::max<size_t>(sym.rows.size(), 1), sym.rows.empty() ? nullptr : sym.rows.data()) &&
             mm.alloc(err, d.gChildPtr, sym.childPtr.size(), sym.childPtr.data()) &&
             mm.alloc(err, d.gChild, std::max<size_t>(sym.child.size(), 1), sym.child.empty() ? nullptr : sym.child.data()) &&
             mm.alloc(err, d.gRel, std::max<size_t>(sym.rel.size(), 1), sym.rel.empty() ? nullptr : sym.rel.data()) &&
             mm.alloc(err, d.gAsmPtr, sym.asmPtr.size(), sym.asmPtr.data()) && mm.alloc(err, d.gAsmSrc, sym.asmSrc.size(), sym.asmSrc.data()) &&
             mm.alloc(err, d.gAsmGate, sym.asmGate.size(), sym.asmGate.data()) && mm.alloc(err, d.gAsmPos, sym.asmPos.size(), sym.asmPos.data()) &&
             mm.alloc(err, d.gLoff, lo.size(), lo.data()) && mm.alloc(err, d.gCBoff, co.size(), co.data()) &&
             mm.alloc(err, d.gMeta, meta.size(), meta.data()) && mm.alloc(err, d.gChildInfo, cinfo.size(), cinfo.data()) &&
             mm.alloc(err, d.gStack, B * d.gStackSize) && mm.alloc(err, d.gFront, B * (size_t)d.gMaxFront * d.gMaxFront);
    }
    {
        // pools of the phase machine (k_sparse_sched): the largest power of two of instances whose per-instance arrays all stay below 4 GiB
        // (the 32-bit lane offsets of SpCtx::arr), at most the batch rounded up to a power of two
        size_t perInst = sizeof(double) * std::max<size_t>({(size_t)nnzQ, (size_t)nnzA, 2 * Np, (size_t)((G > 16 && !general) ? (size_t)N * ld : 0), d.kfStride,
                                                            general ? (size_t)d.gStackSize : 0, general ? (size_t)d.gMaxFront * d.gMaxFront : 0,
                                                            2 * (size_t)kb * Np, 2 * (size_t)nU, (size_t)NV_NUM * n, (size_t)MV_NUM * m, (size_t)nComp});
        perInst = std::max(perInst, sizeof(int) * (size_t)MI_NUM * m);
        int pool = 1;
        while ((size_t)(2 * pool) * perInst < ((size_t)1 << 32) && pool < batch) pool *= 2;
        if (const char* e = std::getenv("LCQP_SPARSE_POOL")) { const int v = std::atoi(e); if (v >= 1 && v < pool && (v & (v - 1)) == 0) pool = v; }      // test hook: several small pools
        d.poolSize = pool; d.nPools = (batch + pool - 1) / pool;
        d.wideDiv = std::max(1, h->cus * 4 / std::max(1, d.nPools));      // SIMDs of the device per pool
        ok = ok && mm.alloc(err, d.state, B) && mm.alloc(err, d.qring, (size_t)d.nPools * PH_NUM * pool) &&
             mm.alloc(err, d.qctl, (size_t)d.nPools * (PH_NUM + 1) * QCTL) && mm.alloc(err, d.qprof, (PH_NUM + 1) * 3);
    }
    if (!ok) { g_sp_err = "device allocation failed: " + g_sp_err; return nullptr; }
    if (hipError_t e = hipStreamSynchronize(h->stream)) { hip_fail(g_sp_err, "hipStreamSynchronize(h->stream)", e); return nullptr; }      // the zero-fills
    return h.release();
}, nullptr); }

extern "C" void lcqp_hip_sparse_destroy(lcqp_hip_sparse_t* h)
{
    guarded(g_sp_err, [&] { delete h; });      // ~lcqp_hip_sparse: set the device, synchronise, then the members
}

extern "C" int lcqp_hip_sparse_bandwidth(const lcqp_hip_sparse_t* h) { return h ? h->db.w : -1; }
extern "C" int lcqp_hip_sparse_lanes(const lcqp_hip_sparse_t* h) { return h ? h->db.G : -1; }
extern "C" int lcqp_hip_sparse_border(const lcqp_hip_sparse_t* h) { return h ? h->db.kb : -1; }
extern "C" int lcqp_hip_sparse_fronts(const lcqp_hip_sparse_t* h) { return h ? (h->db.general ? h->db.gnF : 0) : -1; }
extern "C" int lcqp_hip_sparse_general_ordering(const lcqp_hip_sparse_t* h) { return h ? h->generalOrdering : -1; }
extern "C" int lcqp_hip_sparse_get_ordering(const lcqp_hip_sparse_t* h, int* perm)
{
    if (!h || !perm) return LCQP_INVALID_ARGUMENT;
    const std::vector<int>& pm = h->ord[h->useB].perm;      // the ordering the loaded Hessians select (sp_choose_ordering)
    memcpy(perm, pm.data(), sizeof(int) * pm.size());
    return 0;
}

// storeSteps: the first 4096 iterates
extern "C" int lcqp_hip_sparse_set_options(lcqp_hip_sparse_t* h, const lcqp_options_t* opt)
{ return guarded(g_sp_err, [&] {
    if (h) h->rs.invalidate();      // the ADMM weights, sigma and the regularisations of the factors come from the options
    return set_options(g_sp_err, h, opt, 4096);
}); }

/* per-iterate trace of one instance of the last run (needs options.storeSteps), as lcqp_hip_batch_get_trace */
extern "C" int lcqp_hip_sparse_get_trace(lcqp_hip_sparse_t* h, int instance, int cap, double* scalars, double* x, int* len)
{
    return guarded(g_sp_err, [&] { return get_trace(g_sp_err, h, instance, cap, scalars, x, len); });
}

// The host load and update are the device path behind an upload: the caller's arrays (v, and for a load Qx and Ax: host memory, [count][..]
// each, null: absent) go to the device in chunks of instances, and sparse_pack -- the kernels of lcqp_hip_sparse_load_device /
// _update_device -- builds the pools of [first, first + count) from them.  Synchronous: the arrays are free on return.
static int sparse_upload(lcqp_hip_sparse* h, int first, int count, const SpPackVectors& v, const double* Qx, const double* Ax, bool update)
{
    const SpBatch& d = h->db;
    const size_t n = d.n, m = d.m, nC = d.nC, nK = d.nComp, nnzQ = d.nnzQ, nnzE = d.nnzE;
    const RawArray raw[] = {{v.g, n}, {v.lbA, nC}, {v.ubA, nC}, {v.lbL, nK}, {v.ubL, nK}, {v.lbR, nK}, {v.ubR, nK}, {v.x0, n}, {v.y0, m}, {Qx, nnzQ}, {Ax, nnzE}};
    return upload_packed(g_sp_err, h, count, raw, [&](int c0, int cb, const double* const* p) {
        return sparse_pack(h, first + c0, cb, SpPackVectors{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}, SpPackValues{p[9], p[10], nnzQ, nnzE}, update);
    });
}

// LCQProblem::loadLCQP (sparse overload, src/LCQProblem.cpp:390-441) for instances [first, first + count): values only -- the
// pattern was given to lcqp_hip_sparse_create.  Qx: [count][nnzQ]; Ax: [count][nnzA] in the CSC order of the stacked [A; L; R].
extern "C" int lcqp_hip_sparse_load(lcqp_hip_sparse_t* h, int first, int count, const double* Qx, const double* g, const double* Ax,
                                    const double* lbA, const double* ubA, const double* lbL, const double* ubL, const double* lbR,
                                    const double* ubR, const double* x0, const double* y0)
{ return guarded(g_sp_err, [&] {
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    SpBatch& d = h->db;
    const int n = d.n, nK = d.nComp;
    if (first < 0 || count <= 0 || first > d.B - count || !Qx || !Ax) return LCQP_INVALID_ARGUMENT;
    if (!g) return LCQP_INVALID_OBJECTIVE_LINEAR_TERM;
    if (int rc = check_lower_bounds((size_t)count * nK, lbL, lbR)) return rc;      // the last check: from here on the range is written
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    if (int rc = sp_value_map(h)) return rc;
    h->rs.invalidate();
    load_bound_flags(d, h->loaded, first, lbL, lbR);
    for (int k = 0; k < count; k++) {
        double dmin = INFINITY, dmax = 0.0;
        for (int i = 0; i < n; i++) { const double q = h->qdiagHost[i] >= 0 ? Qx[(size_t)k * d.nnzQ + h->qdiagHost[i]] : 0.0; dmin = std::min(dmin, q); dmax = std::max(dmax, std::fabs(q)); }
        h->diagRatio[(size_t)first + k] = (dmax > 0.0 && dmin > 0.0) ? dmin / dmax : 0.0;
        h->rs.filled[(size_t)first + k] = 1;
    }
    h->loaded = true;
    sp_choose_ordering(h);
    return sparse_upload(h, first, count, SpPackVectors{g, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0}, Qx, Ax, false);
}); }

/* -DLCQP_SCHED_PROFILE builds: per phase (rows 0 .. PH_NUM-1: start, round, trial, factor, correct, qp end; row PH_NUM: polls without work) the clock
 * ticks (100 MHz), wavefront steps and instances served, summed over the wavefronts of all runs since the handle was created: 3 (PH_NUM + 1) values */
extern "C" int lcqp_hip_sparse_sched_profile(lcqp_hip_sparse_t* h, unsigned long long* out)
{ return guarded(g_sp_err, [&] {
    if (!h || !out) return LCQP_INVALID_ARGUMENT;
    if (int rc = synchronize(g_sp_err, h)) return rc;
    HIPCHK(g_sp_err, hipMemcpy(out, h->db.qprof, sizeof(unsigned long long) * 3 * (PH_NUM + 1), hipMemcpyDeviceToHost));
    return 0;
}); }

// the launches of a run or a re-solve on the handle's stream: the setup (or the refresh, or the setup around the kept point) from ev0 to
// ev1, the homotopy from ev1 to ev2
static int sp_run(lcqp_hip_sparse* h, SpFirst first, int mode, const double* rho0)
{
    h->rs.invalidate();
    HIPCHK(g_sp_err, hipEventRecord(h->ev0, h->stream));
    sp_kernels(h->db.G)->run(h->db, h->cus, h->stream, h->ev1, first, mode, rho0);
    if (first != SpFirst::REFRESH) h->rs.nSetups++;
    h->rs.nLaunches++;
    HIPCHK(g_sp_err, hipGetLastError());
    HIPCHK(g_sp_err, hipEventRecord(h->ev2, h->stream));
    h->ran = h->rs.setupValid = h->rs.solved = true;
    return 0;
}

extern "C" int lcqp_hip_sparse_run(lcqp_hip_sparse_t* h)
{ return guarded(g_sp_err, [&] {
    if (!h || !h->loaded) return LCQP_LCQPOBJECT_NOT_SETUP;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    sp_choose_ordering(h);
    return sp_run(h, SpFirst::SETUP, 0, nullptr);
}); }

// New vectors for instances [first, first + count) of a batch that holds problems: the argument list of lcqp_hip_sparse_load without the
// values of the matrices, the same packing, the same meaning of NULL.  The whole range is checked before anything is written, and only
// NV_G, NV_X0, MV_L, MV_U, MV_Y0, lbL, lbR and hasY0 of those instances are written: the stored solution, the statuses and the factors stay.
extern "C" int lcqp_hip_sparse_update(lcqp_hip_sparse_t* h, int first, int count, const double* g,
                                      const double* lbA, const double* ubA, const double* lbL, const double* ubL,
                                      const double* lbR, const double* ubR, const double* x0, const double* y0)
{ return guarded(g_sp_err, [&] {
    if (int rc = check_update(g_sp_err, h, first, count, g, lbL, lbR)) return rc;
    SpBatch& d = h->db;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    d.hasLbL |= lbL ? 1 : 0; d.hasLbR |= lbR ? 1 : 0;      // switched on, never off (an absent vector is the zero vector)
    // (no drain of the stream: the copies and the pack kernel are behind a run in flight on it)
    return sparse_upload(h, first, count, SpPackVectors{g, lbA, ubA, lbL, ubL, lbR, ubR, x0, y0}, nullptr, nullptr, true);
}); }

// the range and value checks of lcqp_hip_sparse_update_values and its device twin up to the first device call, in the order of the dense
// check_update_matrices.  Nothing is written when one of them fails.
int check_update_values(lcqp_hip_sparse* h, int first, int count, const double* Qx, const double* Ax)
{
    if (!Qx && !Ax) return LCQP_INVALID_ARGUMENT;
    if (!h) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (first < 0 || count <= 0 || first > h->db.B - count) return LCQP_INVALID_ARGUMENT;
    for (int k = 0; k < count; k++) if (!h->rs.filled[(size_t)first + k]) return LCQP_LCQPOBJECT_NOT_SETUP;
    return 0;
}

// New values of the matrices for instances [first, first + count) of a batch that holds problems, on the pattern of the handle: Qx, Ax as
// lcqp_hip_sparse_load takes them, NULL: the array stays.  Only their segments of the value pools are written (k_sparse_pack_values behind
// the chunked upload): no vector, no SpInfo, no status, multiplier, point, statistic or factor.  The whole call is checked before anything
// is written.  New Hessians may move the batch across the definiteness line of sp_choose_ordering in either direction.
extern "C" int lcqp_hip_sparse_update_values(lcqp_hip_sparse_t* h, int first, int count, const double* Qx, const double* Ax)
{ return guarded(g_sp_err, [&] {
    if (int rc = check_update_values(h, first, count, Qx, Ax)) return rc;
    const SpBatch& d = h->db;
    const size_t nnzQ = d.nnzQ, nnzE = d.nnzE;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    if (Ax) if (int rc = sp_value_map(h)) return rc;
    h->rs.matrices_changed();
    if (Qx)
        for (int k = 0; k < count; k++) {
            double dmin = INFINITY, dmax = 0.0;
            for (int i = 0; i < d.n; i++) { const double q = h->qdiagHost[i] >= 0 ? Qx[(size_t)k * nnzQ + h->qdiagHost[i]] : 0.0; dmin = std::min(dmin, q); dmax = std::max(dmax, std::fabs(q)); }
            h->diagRatio[(size_t)first + k] = (dmax > 0.0 && dmin > 0.0) ? dmin / dmax : 0.0;
        }
    sp_choose_ordering(h);
    // (no drain of the stream: the copies and the pack kernel are behind a run in flight on it)
    const RawArray raw[] = {{Qx, nnzQ}, {Ax, nnzE}};
    return upload_packed(g_sp_err, h, count, raw, [&](int c0, int cb, const double* const* p) {
        return sparse_pack_values(h, first + c0, cb, SpPackValues{p[0], p[1], nnzQ, nnzE});
    });
}); }

// Solve again on the setup in place: k_sparse_refresh where a run has k_sparse_setup, then the homotopy launch.  Without a setup that
// belongs to the matrices and options in place this is lcqp_hip_sparse_run -- unless the call is warm and only the values of the matrices
// changed since the last solve (lcqp_hip_sparse_update_values): then k_sparse_setup_warm stands there, in the ordering the Hessians in
// place select, and keeps the stored point.
extern "C" int lcqp_hip_sparse_resolve(lcqp_hip_sparse_t* h, int mode, const double* rho0)
{ return guarded(g_sp_err, [&] {
    const int chk = check_resolve(g_sp_err, h, mode, rho0, h && h->loaded);
    const bool newValues = chk == RESOLVE_RUNS && mode == 1 && h->rs.pointKept;
    if (chk && !newValues) return chk == RESOLVE_RUNS ? lcqp_hip_sparse_run(h) : chk;
    const int B = h->db.B;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    const bool withRho = mode == 1 && rho0;
    if (withRho) {
        if (!h->rs.rhoStart && !h->mem.alloc(g_sp_err, h->rs.rhoStart, (size_t)B)) { g_sp_err = "device allocation failed: " + g_sp_err; return LCQP_HIP_ERROR; }
        HIPCHK(g_sp_err, hipStreamSynchronize(h->stream));      // the zero-fill of a fresh buffer, a run in flight that reads an older one
        HIPCHK(g_sp_err, hipMemcpy(h->rs.rhoStart, rho0, sizeof(double) * (size_t)B, hipMemcpyHostToDevice));
    }
    if (newValues) sp_choose_ordering(h);
    return sp_run(h, newValues ? SpFirst::SETUP_WARM : SpFirst::REFRESH, mode, withRho ? h->rs.rhoStart : nullptr);
}); }

extern "C" int lcqp_hip_sparse_launch_counts(lcqp_hip_sparse_t* h, int out[2])
{
    return launch_counts(h, out);
}

// the device copy of the one value map of the pattern (a permutation of the positions of the caller's Ax), uploaded once: entry k of the CSR
// arrays of E is entry valMap[k] of the caller's CSC array.  The adjoint scatters through it, a device load gathers through it.
int sp_value_map(lcqp_hip_sparse* h)
{
    if (h->valMap) return 0;
    const SpBatch& d = h->db;
    for (int k : h->csr2csc) if (k < 0 || k >= d.nnzE) { g_sp_err = "the value map of the pattern is out of range"; return LCQP_HIP_ERROR; }
    if ((int)h->csr2csc.size() != d.nnzE) { g_sp_err = "the value map of the pattern has the wrong length"; return LCQP_HIP_ERROR; }
    if (!h->mem.alloc(g_sp_err, h->valMap, h->csr2csc.size(), h->csr2csc.data())) return LCQP_HIP_ERROR;
    return 0;
}

// ---- test and diagnostic entry point: the KKT factorisations and solves of every instance held against a plain reference (k_sparse_kkt_probe) ----
extern "C" int lcqp_hip_sparse_kkt_probe(lcqp_hip_sparse_t* h, int mode, int which, int nrhs, const double* dprim, const double* ddual, const int* use,
                                         const double* rhs, double* sol, double* rec_dprim, double* rec_ddual, int* rec_use)
{ return guarded(g_sp_err, [&] {
    if (nrhs < 1 || !rhs || !sol) return LCQP_INVALID_ARGUMENT;
    if (mode != LCQP_KKT_PROBE_FACTOR && mode != LCQP_KKT_PROBE_STORED) { g_sp_err = "kkt_probe: mode is 0 (FACTOR) or 1 (STORED)"; return LCQP_INVALID_ARGUMENT; }
    if (mode == LCQP_KKT_PROBE_FACTOR && (!dprim || !ddual || !use)) return LCQP_INVALID_ARGUMENT;
    if (mode == LCQP_KKT_PROBE_STORED && ((which != 0 && which != 1) || !rec_dprim || !rec_ddual || !rec_use)) {
        g_sp_err = "kkt_probe: STORED takes which = 0 (polish slot) or 1 (ADMM slot) and the three record buffers";
        return LCQP_INVALID_ARGUMENT;
    }
    // K0 of the register engine and both factors exist behind a run or a resolve on the data in place; the stored polish factor and its record
    // only while no FACTOR probe has overwritten them
    if (!h || !h->rs.setupValid) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (mode == LCQP_KKT_PROBE_STORED && which == 0 && !h->rs.solved) return LCQP_LCQPOBJECT_NOT_SETUP;
    SpBatch& d = h->db;
    if (int rc = synchronize(g_sp_err, h)) return rc;
    const size_t B = d.B, m = d.m, nvec = B * (size_t)nrhs * d.N;
    DevMem tmp(h->stream);      // the buffers of this call; freed on every way out
    double *dP = nullptr, *dD = nullptr, *dRhs = nullptr, *dSol = nullptr, *rP = nullptr, *rD = nullptr;
    int *dU = nullptr, *rU = nullptr;
    bool ok = tmp.alloc(g_sp_err, dRhs, nvec, rhs) && tmp.alloc(g_sp_err, dSol, nvec);
    if (mode == LCQP_KKT_PROBE_FACTOR) ok = ok && tmp.alloc(g_sp_err, dP, B, dprim) && tmp.alloc(g_sp_err, dD, B * m, ddual) && tmp.alloc(g_sp_err, dU, B * m, use);
    else ok = ok && tmp.alloc(g_sp_err, rP, B) && tmp.alloc(g_sp_err, rD, B * m) && tmp.alloc(g_sp_err, rU, B * m);
    if (!ok) { g_sp_err = "device allocation failed: " + g_sp_err; return LCQP_HIP_ERROR; }
    if (mode == LCQP_KKT_PROBE_FACTOR) h->rs.solved = false;      // the polish factor of the last run is about to be overwritten
    sp_kernels(d.G)->kkt_probe(d, h->stream, mode, which, nrhs, dP, dD, dU, dRhs, dSol, rP, rD, rU);
    HIPCHK(g_sp_err, hipGetLastError());
    HIPCHK(g_sp_err, hipStreamSynchronize(h->stream));
    HIPCHK(g_sp_err, hipMemcpy(sol, dSol, sizeof(double) * nvec, hipMemcpyDeviceToHost));
    if (mode == LCQP_KKT_PROBE_STORED) {
        HIPCHK(g_sp_err, hipMemcpy(rec_dprim, rP, sizeof(double) * B, hipMemcpyDeviceToHost));
        HIPCHK(g_sp_err, hipMemcpy(rec_ddual, rD, sizeof(double) * B * m, hipMemcpyDeviceToHost));
        HIPCHK(g_sp_err, hipMemcpy(rec_use, rU, sizeof(int) * B * m, hipMemcpyDeviceToHost));
    }
    return 0;
}); }

// ---- test and diagnostic entry point: the sparse products of every instance applied to the caller's vectors (k_sparse_product_probe) ----
extern "C" int lcqp_hip_sparse_product_probe(lcqp_hip_sparse_t* h, int wide, const double* vn, const double* vm, double* on, double* om, double* os, int ell[6])
{ return guarded(g_sp_err, [&] {
    if (!h || !vn || !vm || !on || !om || !os || (wide != 0 && wide != 1)) return LCQP_INVALID_ARGUMENT;
    if (!h->loaded) return LCQP_LCQPOBJECT_NOT_SETUP;
    HIPCHK(g_sp_err, hipSetDevice(h->device));
    SpBatch& d = h->db;
    if (int rc = synchronize(g_sp_err, h)) return rc;
    if (ell) { const int v[6] = {d.ellQ.W, d.ellQ.tails, d.ellE.W, d.ellE.tails, d.ellT.W, d.ellT.tails}; memcpy(ell, v, sizeof v); }
    const size_t B = d.B, n = d.n, m = d.m;
    DevMem tmp(h->stream);      // the buffers of this call; freed on every way out
    SpProductProbeArgs a = {};
    if (!(tmp.alloc(g_sp_err, a.vn, B * PPN_NUM * n, vn) && tmp.alloc(g_sp_err, a.vm, B * PPM_NUM * m, vm) && tmp.alloc(g_sp_err, a.on, B * PPO_NUM * n) &&
          tmp.alloc(g_sp_err, a.om, B * m) && tmp.alloc(g_sp_err, a.os, B * PPS_NUM))) { g_sp_err = "device allocation failed: " + g_sp_err; return LCQP_HIP_ERROR; }
    sp_kernels(d.G)->product_probe(d, h->stream, wide, a);
    HIPCHK(g_sp_err, hipGetLastError());
    HIPCHK(g_sp_err, hipStreamSynchronize(h->stream));
    HIPCHK(g_sp_err, hipMemcpy(on, a.on, sizeof(double) * B * PPO_NUM * n, hipMemcpyDeviceToHost));
    HIPCHK(g_sp_err, hipMemcpy(om, a.om, sizeof(double) * B * m, hipMemcpyDeviceToHost));
    HIPCHK(g_sp_err, hipMemcpy(os, a.os, sizeof(double) * B * PPS_NUM, hipMemcpyDeviceToHost));
    return 0;
}); }

extern "C" int lcqp_hip_sparse_sensitivity_timing(lcqp_hip_sparse_t* h, float* kernel_ms)
{
    return guarded(g_sp_err, [&] { return sensitivity_timing(g_sp_err, h, kernel_ms); });
}

extern "C" int lcqp_hip_sparse_synchronize(lcqp_hip_sparse_t* h)
{
    return guarded(g_sp_err, [&] { return synchronize(g_sp_err, h); });
}

extern "C" int lcqp_hip_sparse_last_timing(lcqp_hip_sparse_t* h, float* setup_ms, float* solve_ms)
{
    return guarded(g_sp_err, [&] { return last_timing(g_sp_err, h, setup_ms, solve_ms); });
}

extern "C" int lcqp_hip_sparse_get_solution(lcqp_hip_sparse_t* h, double* x, double* y, lcqp_stats_t* stats)
{
    return guarded(g_sp_err, [&] { return get_solution(g_sp_err, h, h ? h->db.m : 0, x, y, stats); });
}

// -DLCQP_PROFILE builds (tools/gpu.py sparse_profile): mean clock ticks per instance and phase of the last run
// (products, assembly, factorisation, forward sweeps, backward sweeps, vector operations, LCQP level, -)
extern "C" int lcqp_hip_sparse_read_profile(lcqp_hip_sparse_t* h, double* out)
{ return guarded(g_sp_err, [&] {
#ifdef LCQP_PROFILE
    if (!h || !out) return LCQP_INVALID_ARGUMENT;
    SpBatch& d = h->db;
    if (int rc = synchronize(g_sp_err, h)) return rc;
    std::vector<SpInfo> info(d.B);
    HIPCHK(g_sp_err, hipMemcpy(info.data(), d.info, sizeof(SpInfo) * (size_t)d.B, hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; k++) { out[k] = 0.0; for (auto& i : info) out[k] += i.prof[k] / d.B; }
    return 0;
#else
    (void)h; (void)out;
    return LCQP_HIP_UNSUPPORTED;
#endif
}); }

// algorithmic bytes of the last run (setup + homotopy), counted by the kernels: CSR values and indices of every sparse product,
// band storage read and written by every assembly, factorisation and solve
extern "C" double lcqp_hip_sparse_algorithmic_bytes(lcqp_hip_sparse_t* h)
{ return guarded(g_sp_err, [&] {
    if (!h) return 0.0;
    SpBatch& d = h->db;
    if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return 0.0;
    std::vector<SpInfo> info(d.B);
    if (hipMemcpy(info.data(), d.info, sizeof(SpInfo) * (size_t)d.B, hipMemcpyDeviceToHost) != hipSuccess) return 0.0;
    double tot = 0.0;
    for (auto& i : info) tot += i.bytes;
    return tot;
}, 0.0); }
