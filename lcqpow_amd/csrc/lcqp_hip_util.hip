// lcqp_hip_util.hip -- building blocks of the dense arm for tests and micro-benchmarks (lcqp_hip_util_*, lcqp_hip_bench_rows,
// lcqp_hip_chol_solve) and the CSC utilities (lcqp_hip_csc_*), with their four kernels that are not templated (include/lcqp_hip.h).
#include "lcqp_hip_batch.hpp"
#include "../../include/lcqp_synth.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

using namespace lcqp;
using namespace lcqp_rt;

__global__ __launch_bounds__(WG) void k_chol(int np, int nblk, int n, double* F, double* dscr, int* fail)
{
    LCQP_LDS
    const int b = blockIdx.x;
    wg_chol(F + (size_t)b * np * np, np, nblk, n, 0.0, dscr + (size_t)b * 4096, nullptr, fail + b, lds, 0);
}

__global__ __launch_bounds__(WG, 4) void k_backsolve(int np, int nblk, const double* F, const double* rhs, double* x)
{
    LCQP_LDS
    const int b = blockIdx.x;
    double* xv = x + (size_t)b * np;
    for (int i = threadIdx.x; i < np; i += WG) xv[i] = rhs[(size_t)b * np + i];
    __syncthreads();
    wg_trsv(F + (size_t)b * np * np, np, nblk, xv, true, lds);
    wg_trsv(F + (size_t)b * np * np, np, nblk, xv, false, lds);
}

// =================================================================================================
// building blocks (tests, micro-benchmarks)
// =================================================================================================
// mean time of `repeat` launches (at least one) after one warm-up launch, all on the null stream
template <class Launch>
static int time_launches(int repeat, float* ms, Launch launch)
{
    Event e0, e1;      // destroyed on every return
    if (hipError_t e = e0.status ? e0.status : e1.status) return hip_fail(dense_err(), "hipEventCreate", e);
    if (repeat < 1) repeat = 1;
    launch();
    HIPCHK(dense_err(), hipEventRecord(e0, 0));
    for (int r = 0; r < repeat; r++) launch();
    HIPCHK(dense_err(), hipEventRecord(e1, 0));
    HIPCHK(dense_err(), hipEventSynchronize(e1));
    float t = 0.f;
    HIPCHK(dense_err(), hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / repeat;
    return 0;
}

static int upload_padded(double* dst, const double* src, int batch, int rows, int cols, int ld, int rowsPad)
{
    // src: [batch][rows][cols] -> dst: [batch][rowsPad][ld]
    std::vector<double> buf((size_t)rowsPad * ld);
    for (int b = 0; b < batch; b++) {
        std::fill(buf.begin(), buf.end(), 0.0);
        for (int r = 0; r < rows; r++) memcpy(&buf[(size_t)r * ld], src + ((size_t)b * rows + r) * cols, sizeof(double) * cols);
        HIPCHK(dense_err(), hipMemcpy(dst + (size_t)b * rowsPad * ld, buf.data(), sizeof(double) * rowsPad * ld, hipMemcpyHostToDevice));
    }
    return 0;
}
static int download_padded(double* dst, const double* src, int batch, int rows, int cols, int ld, int rowsPad)
{
    std::vector<double> buf((size_t)rowsPad * ld);
    for (int b = 0; b < batch; b++) {
        HIPCHK(dense_err(), hipMemcpy(buf.data(), src + (size_t)b * rowsPad * ld, sizeof(double) * rowsPad * ld, hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; r++) memcpy(dst + ((size_t)b * rows + r) * cols, &buf[(size_t)r * ld], sizeof(double) * cols);
    }
    return 0;
}

extern "C" int lcqp_hip_util_symv(int batch, int n, double alpha, const double* A, const double* bv, const double* cv, double* dv)
{ return guarded(dense_err(), [&] {
    if (n <= 0 || n > 4096 || batch <= 0) return LCQP_HIP_UNSUPPORTED;
    const SizeKernels* k = dense_kernels(padded_nch(n));
    if (!k) return LCQP_HIP_UNSUPPORTED;
    const int np = 128 * k->nch;
    DevMem tb;
    double *dA, *db_, *dc, *dd;
    if (!tb.alloc(dense_err(), dA, (size_t)batch * np * np) || !tb.alloc(dense_err(), db_, (size_t)batch * np) || !tb.alloc(dense_err(), dc, (size_t)batch * np) ||
        !tb.alloc(dense_err(), dd, (size_t)batch * np))
        return LCQP_HIP_ERROR;
    int rc = upload_padded(dA, A, batch, n, n, np, np); if (rc) return rc;
    rc = upload_padded(db_, bv, batch, 1, n, np, 1); if (rc) return rc;
    rc = upload_padded(dc, cv, batch, 1, n, np, 1); if (rc) return rc;
    k->util_symv(batch, 0, n, alpha, dA, db_, dc, dd);
    HIPCHK(dense_err(), hipDeviceSynchronize());
    return download_padded(dv, dd, batch, 1, n, np, 1);
}); }

static int util_rows(int batch, int m, int n, const double* A, const double* x, double* dots, const double* coef, double* outT)
{
    if (n <= 0 || n > 4096 || batch <= 0 || m <= 0) return LCQP_HIP_UNSUPPORTED;
    const SizeKernels* k = dense_kernels(padded_nch(n));
    if (!k) return LCQP_HIP_UNSUPPORTED;
    const int np = 128 * k->nch;
    DevMem tb;
    double *dA, *dx = nullptr, *dd = nullptr, *dcf = nullptr, *dout = nullptr;
    if (!tb.alloc(dense_err(), dA, (size_t)batch * m * np) || (x && !tb.alloc(dense_err(), dx, (size_t)batch * np)) || (dots && !tb.alloc(dense_err(), dd, (size_t)batch * m)) ||
        (coef && !tb.alloc(dense_err(), dcf, (size_t)batch * m, coef)) || (outT && !tb.alloc(dense_err(), dout, (size_t)batch * np)))
        return LCQP_HIP_ERROR;
    int rc = upload_padded(dA, A, batch, m, n, np, m); if (rc) return rc;
    if (x) { rc = upload_padded(dx, x, batch, 1, n, np, 1); if (rc) return rc; }
    k->util_rows(batch, 0, m, dA, dx, dd, dcf, dout);
    HIPCHK(dense_err(), hipDeviceSynchronize());
    if (dots) HIPCHK(dense_err(), hipMemcpy(dots, dd, sizeof(double) * (size_t)batch * m, hipMemcpyDeviceToHost));
    if (outT) return download_padded(outT, dout, batch, 1, n, np, 1);
    return 0;
}

extern "C" int lcqp_hip_util_rows_list(int batch, int m, int n, const double* A, const int* list, int nlist, const double* x, const double* coef,
                                       double* dots, double* outT)
{ return guarded(dense_err(), [&] {
    if (n <= 0 || n > 4096 || batch <= 0 || m <= 0 || nlist < 0 || nlist > m || !list) return LCQP_HIP_UNSUPPORTED;
    const SizeKernels* k = dense_kernels(padded_nch(n));
    if (!k) return LCQP_HIP_UNSUPPORTED;
    const int np = 128 * k->nch;
    DevMem tb;
    double *dA, *dx = nullptr, *dd = nullptr, *dcf = nullptr, *dout = nullptr;
    int* dl;
    if (!tb.alloc(dense_err(), dA, (size_t)batch * m * np) || (x && !tb.alloc(dense_err(), dx, (size_t)batch * np)) ||
        (dots && !tb.alloc(dense_err(), dd, (size_t)batch * m, dots)) ||      // rows outside the list keep the caller's values
        (coef && !tb.alloc(dense_err(), dcf, (size_t)batch * m, coef)) || (outT && !tb.alloc(dense_err(), dout, (size_t)batch * np)) ||
        !tb.alloc(dense_err(), dl, (size_t)batch * nlist, list))
        return LCQP_HIP_ERROR;
    int rc = upload_padded(dA, A, batch, m, n, np, m); if (rc) return rc;
    if (x) { rc = upload_padded(dx, x, batch, 1, n, np, 1); if (rc) return rc; }
    k->util_rows_list(batch, 0, m, nlist, dA, dl, dx, dd, dcf, dout);
    HIPCHK(dense_err(), hipDeviceSynchronize());
    if (dots) HIPCHK(dense_err(), hipMemcpy(dots, dd, sizeof(double) * (size_t)batch * m, hipMemcpyDeviceToHost));
    if (outT) return download_padded(outT, dout, batch, 1, n, np, 1);
    return 0;
}); }

extern "C" int lcqp_hip_util_gemv(int batch, int m, int n, const double* A, const double* b, double* c)
{
    return guarded(dense_err(), [&] { return util_rows(batch, m, n, A, b, c, nullptr, nullptr); });
}
extern "C" int lcqp_hip_util_gemv_t(int batch, int m, int n, const double* A, const double* b, double* c)
{
    return guarded(dense_err(), [&] { return util_rows(batch, m, n, A, nullptr, nullptr, b, c); });
}

extern "C" int lcqp_hip_util_symm_product(int batch, int m, int n, const double* A, const double* Bm, double* C)
{ return guarded(dense_err(), [&] {
    // goes through the batch object so that the production kernel k_build_C is what is tested
    lcqp_hip_batch* h = lcqp_hip_batch_create(batch, n, 0, m, 0, 0);
    if (!h) return LCQP_HIP_ERROR;
    DevBatch& d = h->db;
    int rc = upload_padded(d.E, A, batch, m, n, d.np, d.mEcap);
    if (!rc) {
        // second block (R) starts at row m of each instance
        std::vector<double> buf((size_t)d.mEcap * d.np);
        for (int b = 0; b < batch && !rc; b++) {
            if (hipMemcpy(buf.data(), d.E + (size_t)b * d.mEcap * d.np, sizeof(double) * buf.size(), hipMemcpyDeviceToHost) != hipSuccess) { rc = LCQP_HIP_ERROR; break; }
            for (int r = 0; r < m; r++) memcpy(&buf[(size_t)(m + r) * d.np], Bm + ((size_t)b * m + r) * n, sizeof(double) * n);
            if (hipMemcpy(d.E + (size_t)b * d.mEcap * d.np, buf.data(), sizeof(double) * buf.size(), hipMemcpyHostToDevice) != hipSuccess) rc = LCQP_HIP_ERROR;
        }
    }
    if (!rc) {
        h->k->build_C(d, d.B * (d.nblk * (d.nblk + 1) / 2), h->stream);
        if (hipStreamSynchronize(h->stream) != hipSuccess) rc = LCQP_HIP_ERROR;
    }
    if (!rc) rc = download_padded(C, d.C, batch, n, n, d.np, d.np);
    lcqp_hip_batch_destroy(h);
    return rc;
}); }

// =================================================================================================
// CSC utilities on the device: compressed-segment gather products.
// A CSC matrix is uploaded together with its transpose (the CSC of A' is the CSR of A), so both
// MatrixMultiplication (A b) and TransponsedMatrixMultiplication (A'b) are gathers over compressed segments --
// no atomics, deterministic, the same summation order as the reference's inner loops
// (src/Utilities.cpp:49-59,75-82,189-199,228-241).
// =================================================================================================
// out[s] = alpha * sum_{k in [ptr[s], ptr[s+1])} val[k] * v[idx[k]] + (add ? add[s] : 0); 16 lanes per segment
__global__ __launch_bounds__(256) void k_seg_gather(int nseg, const int* __restrict__ ptr, const int* __restrict__ idx,
                                                    const double* __restrict__ val, const double* __restrict__ v, double alpha,
                                                    const double* __restrict__ add, double* __restrict__ out)
{
    const int sub = threadIdx.x & 15;
    const int seg = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    double s = 0.0;
    if (seg < nseg) {
        const int k0 = ptr[seg], k1 = ptr[seg + 1];
        for (int k = k0 + sub; k < k1; k += 16) s += val[k] * v[idx[k]];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    if (seg < nseg && sub == 0) out[seg] = alpha * s + (add ? add[seg] : 0.0);
}

struct lcqp_hip_csc {
    int m, n, nnz, device;
    int *p, *i, *tp, *ti;        // CSC of A and CSC of A' (device)
    double *x, *tx;
    double *vin, *vout, *vadd;   // staging vectors of length max(m, n)
    DevMem mem;
    ~lcqp_hip_csc() { (void)hipSetDevice(device); }      // then the memory
};

extern "C" lcqp_hip_csc_t* lcqp_hip_csc_create(int m, int n, int nnz, const int* p, const int* i, const double* x, int device)
{ return guarded(dense_err(), [&]() -> lcqp_hip_csc_t* {
    if (m <= 0 || n <= 0 || nnz < 0 || !p || (nnz && (!i || !x))) { dense_err() = "invalid CSC arguments"; return nullptr; }
    if (hipError_t e = hipSetDevice(device)) { hip_fail(dense_err(), "hipSetDevice(device)", e); return nullptr; }
    // transpose on the host: counting sort by row index (stable, so columns stay ascending inside a row)
    std::vector<int> tp(m + 1, 0), ti(nnz ? nnz : 1);
    std::vector<double> tx(nnz ? nnz : 1);
    for (int k = 0; k < nnz; k++) { if (i[k] < 0 || i[k] >= m) { dense_err() = "CSC row index out of bounds"; return nullptr; } tp[i[k] + 1]++; }
    for (int r = 0; r < m; r++) tp[r + 1] += tp[r];
    std::vector<int> cur(tp.begin(), tp.end() - 1);
    for (int c = 0; c < n; c++)
        for (int k = p[c]; k < p[c + 1]; k++) { const int d = cur[i[k]]++; ti[d] = c; tx[d] = x[k]; }
    std::unique_ptr<lcqp_hip_csc> h(new lcqp_hip_csc());
    h->m = m; h->n = n; h->nnz = nnz; h->device = device;
    const size_t mx = (size_t)(m > n ? m : n);
    DevMem& dm = h->mem;
    const bool ok = dm.alloc(dense_err(), h->p, n + 1, p) && dm.alloc(dense_err(), h->i, nnz, i) && dm.alloc(dense_err(), h->x, nnz, x) &&
                    dm.alloc(dense_err(), h->tp, m + 1, tp.data()) && dm.alloc(dense_err(), h->ti, nnz, ti.data()) && dm.alloc(dense_err(), h->tx, nnz, tx.data()) &&
                    dm.alloc(dense_err(), h->vin, mx) && dm.alloc(dense_err(), h->vout, mx) && dm.alloc(dense_err(), h->vadd, mx);
    if (!ok) return nullptr;
    if (hipError_t e = hipStreamSynchronize(nullptr)) { hip_fail(dense_err(), "hipStreamSynchronize(nullptr)", e); return nullptr; }      // the zero-fills
    return h.release();
}, nullptr); }

extern "C" void lcqp_hip_csc_destroy(lcqp_hip_csc_t* h)
{
    guarded(dense_err(), [&] { delete h; });
}

// d = alpha * op(A) * b + (c ? c : 0);  transposed != 0: op(A) = A' (b has m entries, d has n), else op(A) = A.
// repeat > 1 re-launches the product for timing; *ms = time per launch.
extern "C" int lcqp_hip_csc_apply(lcqp_hip_csc_t* h, int transposed, double alpha, const double* b, const double* c, double* d,
                                  int repeat, float* ms)
{ return guarded(dense_err(), [&] {
    if (!h || !b || !d) return LCQP_INVALID_ARGUMENT;
    HIPCHK(dense_err(), hipSetDevice(h->device));
    const int nin = transposed ? h->m : h->n, nout = transposed ? h->n : h->m;
    HIPCHK(dense_err(), hipMemcpy(h->vin, b, sizeof(double) * nin, hipMemcpyHostToDevice));
    if (c) HIPCHK(dense_err(), hipMemcpy(h->vadd, c, sizeof(double) * nout, hipMemcpyHostToDevice));
    const int* ptr = transposed ? h->p : h->tp;     // A'b gathers over the columns of A, A b over the columns of A'
    const int* idx = transposed ? h->i : h->ti;
    const double* val = transposed ? h->x : h->tx;
    const int grid = (nout * 16 + 255) / 256;
    const int rc = time_launches(repeat, ms, [&] {
        hipLaunchKernelGGL(k_seg_gather, dim3(grid), dim3(256), 0, 0, nout, ptr, idx, val, h->vin, alpha, c ? h->vadd : nullptr, h->vout);
    });
    if (rc) return rc;
    HIPCHK(dense_err(), hipMemcpy(d, h->vout, sizeof(double) * nout, hipMemcpyDeviceToHost));
    return 0;
}); }

// micro-benchmark of the row sweep (wg_rows) on device-resident random data: mode 1 = dots only (A x),
// 2 = axpy only (A'y), 3 = both in one sweep; *ms = time per launch
__global__ void k_fill_random(double* p, size_t n, uint64_t seed)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] = 2.0 * lcqp_u01(seed, i) - 1.0;
}

extern "C" int lcqp_hip_bench_rows(int batch, int m, int n, int mode, int repeat, float* ms)
{ return guarded(dense_err(), [&] {
    if (n <= 0 || n > 4096 || batch <= 0 || m <= 0) return LCQP_HIP_UNSUPPORTED;
    const SizeKernels* k = dense_kernels(padded_nch(n));
    if (!k) return LCQP_HIP_UNSUPPORTED;
    const int np = 128 * k->nch;
    DevMem tb;
    double *dA, *dx, *dd, *dcf, *dout;
    if (!tb.alloc(dense_err(), dA, (size_t)batch * m * np) || !tb.alloc(dense_err(), dx, (size_t)batch * np) || !tb.alloc(dense_err(), dd, (size_t)batch * m) ||
        !tb.alloc(dense_err(), dcf, (size_t)batch * m) || !tb.alloc(dense_err(), dout, (size_t)batch * np))
        return LCQP_HIP_ERROR;
    hipLaunchKernelGGL(k_fill_random, dim3(2048), dim3(256), 0, 0, dA, (size_t)batch * m * np, 1ULL);
    hipLaunchKernelGGL(k_fill_random, dim3(256), dim3(256), 0, 0, dx, (size_t)batch * np, 2ULL);
    hipLaunchKernelGGL(k_fill_random, dim3(256), dim3(256), 0, 0, dcf, (size_t)batch * m, 3ULL);
    const bool dots = mode & 1, axpy = mode & 2;
    return time_launches(repeat, ms, [&] { k->util_rows(batch, 0, m, dA, dots ? dx : nullptr, dots ? dd : nullptr, axpy ? dcf : nullptr, axpy ? dout : nullptr); });
}); }

extern "C" int lcqp_hip_chol_solve(int batch, int n, const double* K, const double* b, double* x, int repeat, float* ms)
{ return guarded(dense_err(), [&] {
    if (n <= 0 || n > LCQP_MAX_ACTIVE || batch <= 0) return LCQP_HIP_UNSUPPORTED;   // k_chol / k_backsolve use the 35 KiB arena
    const int np = ((n + 63) / 64) * 64, nblk = np / 64;
    DevMem tb;
    double *dF, *dscr, *drhs, *dx;
    int* dfail;
    if (!tb.alloc(dense_err(), dF, (size_t)batch * np * np) || !tb.alloc(dense_err(), dscr, (size_t)batch * 4096) || !tb.alloc(dense_err(), drhs, (size_t)batch * np) ||
        !tb.alloc(dense_err(), dx, (size_t)batch * np) || !tb.alloc(dense_err(), dfail, batch))
        return LCQP_HIP_ERROR;
    // pad with a unit diagonal
    {
        std::vector<double> buf((size_t)np * np);
        for (int bb = 0; bb < batch; bb++) {
            std::fill(buf.begin(), buf.end(), 0.0);
            for (int i = 0; i < n; i++) memcpy(&buf[(size_t)i * np], K + ((size_t)bb * n + i) * n, sizeof(double) * n);
            for (int i = n; i < np; i++) buf[(size_t)i * np + i] = 1.0;
            HIPCHK(dense_err(), hipMemcpy(dF + (size_t)bb * np * np, buf.data(), sizeof(double) * np * np, hipMemcpyHostToDevice));
        }
    }
    int rc = upload_padded(drhs, b, batch, 1, n, np, 1); if (rc) return rc;
    hipLaunchKernelGGL(k_chol, dim3(batch), dim3(WG), 0, 0, np, nblk, n, dF, dscr, dfail);
    HIPCHK(dense_err(), hipDeviceSynchronize());
    std::vector<int> fail(batch);
    HIPCHK(dense_err(), hipMemcpy(fail.data(), dfail, sizeof(int) * batch, hipMemcpyDeviceToHost));
    for (int i = 0; i < batch; i++) if (fail[i]) { dense_err() = "matrix not positive definite"; return LCQP_SUBPROBLEM_SOLVER_ERROR; }
    rc = time_launches(repeat, ms, [&] { hipLaunchKernelGGL(k_backsolve, dim3(batch), dim3(WG), 0, 0, np, nblk, dF, drhs, dx); });
    return rc ? rc : download_padded(x, dx, batch, 1, n, np, 1);
}); }

// =================================================================================================
// read-back of the ADMM fallback (tests, diagnostics): the raw padded blocks of one instance, nothing is launched
// =================================================================================================
// L_K as it lies in FK, the rho vector, the bounds of the stacked rows and the iterates with their last change (qp_build_K, qp_admm,
// qp_adapt_rho in lcqp_dev.hpp).  The polish writes none of them, so they are those of the last QP that ran ADMM.  (The readers of the
// setup matrices and of the working set are in lcqp_hip.hip; this one stands here because that unit is one of the kernel sources the
// committed profiles are keyed to, and a reader is no reason to void them.)
extern "C" int lcqp_hip_batch_read_admm(lcqp_hip_batch_t* h, int b, int dims[6], double scal[3], double* FK, double* rhov, double* l, double* u,
                                        double* xa, double* ya, double* za, double* dy, double* dx)
{ return guarded(dense_err(), [&] {
    if (!h || b < 0 || b >= h->db.B) return LCQP_INVALID_ARGUMENT;
    if (!h->rs.setupValid) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (int rc = synchronize(dense_err(), h)) return rc;
    HIPCHK(dense_err(), hipStreamSynchronize(h->side));
    const DevBatch& d = h->db;
    const size_t ib = b, np = d.np, mE = d.mEcap;
    InstInfo info;
    HIPCHK(dense_err(), hipMemcpy(&info, d.info + ib, sizeof(InstInfo), hipMemcpyDeviceToHost));
    if (dims) {
        const int v[6] = {d.np, d.nblk, d.mEcap, info.mE, info.kReady, info.setupFail};
        memcpy(dims, v, sizeof v);
    }
    if (scal) { scal[0] = info.sigma; scal[1] = info.rhoAdmm; scal[2] = info.scale; }
    const double *nv = d.nv + ib * V_NUM * np, *mv = d.mv + ib * M_NUM * mE;
    int rc = read_back(dense_err(), FK, d.FK + ib * np * np, np * np);
    if (!rc) rc = read_back(dense_err(), rhov, mv + (size_t)M_RHOV * mE, mE);
    if (!rc) rc = read_back(dense_err(), l, mv + (size_t)M_L * mE, mE);
    if (!rc) rc = read_back(dense_err(), u, mv + (size_t)M_U * mE, mE);
    if (!rc) rc = read_back(dense_err(), xa, nv + (size_t)V_XA * np, np);
    if (!rc) rc = read_back(dense_err(), ya, mv + (size_t)M_YA * mE, mE);
    if (!rc) rc = read_back(dense_err(), za, mv + (size_t)M_ZA * mE, mE);
    if (!rc) rc = read_back(dense_err(), dy, mv + (size_t)M_DY * mE, mE);
    if (!rc) rc = read_back(dense_err(), dx, nv + (size_t)V_W * np, np);
    return rc;
}); }

// =================================================================================================
// read-back of the active-set polish (tests, diagnostics): the vectors qp_polish / qp_solve leave in the pools of one instance, nothing is launched
// =================================================================================================
// V [8][np]: V_XT, V_XS, V_XREF, V_R1S, V_GS, V_ATY, V_QXN, V_XQ;  M [10][mEcap]: M_YT, M_EX, M_EXS, M_MG, M_RN, M_HOTV, M_YLV, M_L, M_U, M_YQ;
// I [5][mEcap]: I_STT, I_ST, I_DEP, I_SLOT, I_HOTC -- in this order, as they lie on the device.  dims[9] (rowsInLds) is 1 when the
// homotopy kernel of this handle keeps the row state in LDS (launch_run in lcqp_kernels.hpp: np <= 256, mEcap <= LDS_ROWS_MAX,
// 4 capS <= LDS_ROWS_OFF): qp_polish then copies yt, ex, mg, st to their global arrays only around a one-piece rebuild of the factor, so
// M_YT, M_EX, M_MG and I_STT are STALE after lcqp_hip_batch_run / _resolve on such a handle (whatever the last rebuild left).  k_qp_solve
// (the QP object) always works on the global arrays.
extern "C" int lcqp_hip_batch_read_polish(lcqp_hip_batch_t* h, int b, int dims[12], double scal[7], double* V, double* M, int* I)
{ return guarded(dense_err(), [&] {
    if (!h || b < 0 || b >= h->db.B) return LCQP_INVALID_ARGUMENT;
    if (!h->rs.setupValid) return LCQP_LCQPOBJECT_NOT_SETUP;
    if (int rc = synchronize(dense_err(), h)) return rc;
    HIPCHK(dense_err(), hipStreamSynchronize(h->side));
    const DevBatch& d = h->db;
    const size_t ib = b, np = d.np, mE = d.mEcap;
    InstInfo info;
    HIPCHK(dense_err(), hipMemcpy(&info, d.info + ib, sizeof(InstInfo), hipMemcpyDeviceToHost));
    if (dims) {
        const int lr = d.np <= 256 && d.mEcap <= LDS_ROWS_MAX && 4 * d.capS <= LDS_ROWS_OFF;
        const int v[12] = {d.np, d.mEcap, info.mE, info.nT, info.ns, info.ndep, info.rnReady, info.nHot, info.haveSolution, lr, d.n, d.capS};
        memcpy(dims, v, sizeof v);
    }
    if (scal) { scal[0] = info.spv; for (int k = 0; k < 6; k++) scal[1 + k] = info.work[k]; }      // work: the exact work sums of InstInfo
    const double *nv = d.nv + ib * V_NUM * np, *mv = d.mv + ib * M_NUM * mE;
    const int* mi = d.mi + ib * I_NUM * mE;
    static const int vk[8] = {V_XT, V_XS, V_XREF, V_R1S, V_GS, V_ATY, V_QXN, V_XQ};
    static const int mk[10] = {M_YT, M_EX, M_EXS, M_MG, M_RN, M_HOTV, M_YLV, M_L, M_U, M_YQ};
    static const int ik[5] = {I_STT, I_ST, I_DEP, I_SLOT, I_HOTC};
    int rc = 0;
    for (int k = 0; k < 8 && !rc && V; k++) rc = read_back(dense_err(), V + k * np, nv + (size_t)vk[k] * np, np);
    for (int k = 0; k < 10 && !rc && M; k++) rc = read_back(dense_err(), M + k * mE, mv + (size_t)mk[k] * mE, mE);
    for (int k = 0; k < 5 && !rc && I; k++) rc = read_back(dense_err(), I + k * mE, mi + (size_t)ik[k] * mE, mE);
    return rc;
}); }
