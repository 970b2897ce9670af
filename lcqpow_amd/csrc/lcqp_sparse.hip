// lcqp_sparse.hip -- the SPARSE arm of the hot path on gfx950: B independent LCQPs that share one sparsity pattern, behind
// lcqp_hip_sparse_* (include/lcqp_hip.h).  G lanes of a wavefront per instance (G = 8, 16, 32 or 64: the smallest power of two
// above the half bandwidth of the KKT band), 64 / G instances per wavefront, one wavefront per workgroup (k_sparse_sched).
//
// Restates, with the conventions of the reference's OSQP_SPARSE arm (src/LCQProblem.cpp:929-960: no box constraints, nC + 2 nComp
// duals, no box term in the stationarity :1246-1272, dual sign of src/SubsolverOSQP.cpp:196-199):
//   * runSolver (src/LCQProblem.cpp:444-560) with the CSC Utilities products (src/Utilities.cpp:49-59,75-82,189-199) done as CSR
//     row gathers (Q x, E x) and CSC column gathers (E'y) -- deterministic, no atomics; C x = L'(R x) + R'(L x), C never formed;
//   * the subsolver behind SubsolverOSQP (src/SubsolverOSQP.cpp:124-200; OSQP itself is an absent submodule -- its published
//     algorithm is what is built): ADMM on the quasi-definite KKT matrix [Q + sigma I, E'; E, -1/rho], factorised ONCE per LCQP,
//     and an active-set polish on [Q + delta I, Ea'; Ea, -delta2 I] in iterative-refinement form, refactorised only when the
//     working set changes.  oracle/lcqp_oracle_sparse.c is the same algorithm in scalar C.
// The KKT matrices are factorised as BAND matrices in a reverse Cuthill-McKee ordering computed once per pattern on the host
// (lcqp_sparse_pattern.hpp; all instances of a batch share it): LDL' with a sliding G x G window in registers (G <= 16) or LDS (half bandwidth w <= G - 1 <= 63), triangular
// solves that keep the G pending rows of an instance in its G lanes (axpy form both ways, no reductions in the chain; the finished
// entry is broadcast inside the lane group by DPP).  A group of lanes behaves like a small workgroup of its own: every branch
// condition is uniform inside a group, groups of one wavefront diverge through the execution mask, there are no workgroup barriers.
// Patterns whose KKT band is wider take a bordered band (a few dense nodes behind the band, e.g. the arrow-shaped circle example) or the
// general sparse LDL' (lcqp_sparse_general.hpp); what neither holds is refused here, and the host layer runs it on the dense kernels behind
// the same OSQP_SPARSE surface.
//
// Kernels only: the host side of lcqp_hip_sparse_* is lcqp_sparse_host.hip, and lcqp_sparse_launch.hpp is the seam between the two (the
// batch struct the kernels take, the launch functions defined at the end of this file).  One translation unit per lane-group width:
// compile with -DLCQP_TU_G=G.
#include "lcqp_wg.hpp"
#include "lcqp_sparse_launch.hpp"
#include "lcqp_sparse_pattern.hpp"      // GEN_MAX_FRONT

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#ifndef LCQP_TU_G
#error "compile lcqp_sparse.hip with -DLCQP_TU_G=8|16|32|64"
#endif
#define LCQP_CAT2(a, b) a##b
#define LCQP_CAT(a, b) LCQP_CAT2(a, b)

using namespace lcqp;
using namespace lcqp_sparse;

namespace {

constexpr int WGS = 64;      // one wavefront per workgroup; 64 / G instances in it
constexpr int SCHED_WAVES_PER_SIMD = 2;   // register budget of k_sparse_sched at G <= 8: 512 / SCHED_WAVES_PER_SIMD per lane

// ---- addressing: uniform base pointer + 32-bit lane offset -------------------------------------------------------------------------
// Every per-instance array is reached as (base of the wave's first instance: uniform, SGPRs) + (byte offset of the lane's instance
// inside the wave's block + element offset: 32 bits, one VGPR) -- the global_load saddr form.  Per-lane 64-bit pointers would cost two
// VGPRs for each of the ~40 vectors of an instance (the compiler hoists them) and 64-bit VALU address arithmetic at every access.
typedef double dv2 __attribute__((ext_vector_type(2)));
template <class T> struct GRef {
    T* base; unsigned boff;
    __device__ __forceinline__ operator T() const { return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)boff); }
    __device__ __forceinline__ T operator=(T v) const { *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + (size_t)boff) = v; return v; }
    __device__ __forceinline__ T operator=(const GRef& o) const { return *this = (T)o; }
    __device__ __forceinline__ T operator+=(T v) const { return *this = (T)(*this) + v; }
    __device__ __forceinline__ T operator-=(T v) const { return *this = (T)(*this) - v; }
};
template <class T> struct GP {
    T* base; unsigned off;                       // uniform base; byte offset of this lane's data
    __device__ __forceinline__ GRef<T> operator[](int i) const { return GRef<T>{base, off + (unsigned)i * (unsigned)sizeof(T)}; }
    __device__ __forceinline__ T ld(int i) const { return (T)(*this)[i]; }
    __device__ __forceinline__ GP<T> operator+(int i) const { return GP<T>{base, off + (unsigned)i * (unsigned)sizeof(T)}; }
    __device__ __forceinline__ dv2 ld2(int i) const { return *reinterpret_cast<const dv2*>(reinterpret_cast<const char*>(base) + (size_t)(off + (unsigned)i * 8u)); }
};
typedef GP<double> GD;
typedef GP<int> GI;
// the value type behind what a load lambda returns (a lambda that returns x[i] returns the reference proxy, not the value)
template <class X> struct val_of { typedef X type; };
template <class T> struct val_of<GRef<T>> { typedef T type; };

extern __shared__ double sp_dyn_lds[];      // G <= 16: the working sets' bit sets (sp_ph_factor); G > 16: the windows of sp_factor_lds

template <int G>
struct SpCtx {
    const SpBatch* db;
    int b, gl;               // instance, lane inside the group
    unsigned gi;             // this instance's index relative to w0
    int w0;                  // first instance of the block of instances the wave addresses (uniform): its own 64 / G instances (k_sparse_setup) or its pool (k_sparse_sched)
    SpInfo* info;
    double* win;             // LDS of this group: G x G window + 16 staged rows
    int cAdmm, cTrials, cFact, cCorr, cSweeps;
    double bytes;
#ifdef LCQP_PROFILE
    unsigned long long tprev, prof[SP_NPHASE];
#endif
    // per-instance arrays: block of the wave's first instance (uniform) + this instance's offset inside it
    template <class T> __device__ __forceinline__ GP<T> arr(T* p, size_t perInst, unsigned extra = 0) const
    { return GP<T>{p + ((size_t)w0 * perInst + extra), gi * (unsigned)perInst * (unsigned)sizeof(T)}; }    // vectors differ in the (SGPR) base only
    __device__ __forceinline__ GD V(int k) const { return arr(db->nv, (size_t)NV_NUM * db->n, (unsigned)k * db->n); }
    __device__ __forceinline__ GD M(int k) const { return arr(db->mv, (size_t)MV_NUM * db->m, (unsigned)k * db->m); }
    __device__ __forceinline__ GI I(int k) const { return arr(db->mi, (size_t)MI_NUM * db->m, (unsigned)k * db->m); }
    __device__ __forceinline__ GD Qx() const { return arr(db->Qx, db->nnzQ); }
    __device__ __forceinline__ GD Ex() const { return arr(db->Ex, db->nnzE); }
    __device__ __forceinline__ GD Nv() const { return arr(db->Nv, (size_t)2 * db->Np); }
    __device__ __forceinline__ GD Kb() const { return arr(db->Kb, (size_t)db->N * db->ld); }
    __device__ __forceinline__ GD KF(bool admm) const { return arr(admm ? db->KaF : db->KpF, db->kfStride); }
    __device__ __forceinline__ GD GStack() const { return arr(db->gStack, db->gStackSize); }
    __device__ __forceinline__ GD GFront() const { return arr(db->gFront, (size_t)db->gMaxFront * db->gMaxFront); }
    __device__ __forceinline__ GD KD(bool admm) const { return arr(admm ? db->KaD : db->KpD, db->Np); }
    __device__ __forceinline__ GD K0() const { return arr(db->K0, (size_t)db->Np * G); }
    __device__ __forceinline__ GD BW(bool admm) const { return arr(db->bW, (size_t)2 * db->kb * db->Np, (unsigned)(admm ? db->kb * db->Np : 0)); }
    __device__ __forceinline__ GD BUv(bool admm) const { return arr(db->bUv, (size_t)2 * db->nU, (unsigned)(admm ? db->nU : 0)); }
    __device__ __forceinline__ GD BS(bool admm) const { return arr(db->bS, (size_t)2 * db->kb * db->kb, (unsigned)(admm ? db->kb * db->kb : 0)); }
};

#ifdef LCQP_PROFILE
#define SPROF(c, P) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); (c).prof[P] += t_ - (c).tprev; (c).tprev = t_; } while (0)
#else
#define SPROF(c, P) do { } while (0)
#endif

// Everything a lane computes from its lane number and uniform values is invariant in every loop of the kernel, and the compiler
// hoists it all to the top (hundreds of 64-bit addresses, spilled to scratch at once).  An empty volatile asm cannot be hoisted:
// what is derived from the laundered lane number stays inside the routine that uses it.
__device__ __forceinline__ int here(int lane) { asm volatile("" : "+v"(lane)); return lane; }

// ---- lane-group collectives (every lane of the group takes part; results are uniform inside the group) ------------------------
template <int CTRL> __device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int CTRL> __device__ __forceinline__ double dpp_d(double v)
{
    const int lo = dpp_i<CTRL>(__double2loint(v)), hi = dpp_i<CTRL>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// DPP controls: 0xB1 = quad_perm[1,0,3,2], 0x4E = quad_perm[2,3,0,1], 0x141 = row_half_mirror (lane j <- 7 - j of its 8), 0x140 = row_mirror
template <int G> __device__ __forceinline__ double g_sum(double v)
{
    v += dpp_d<0xB1>(v);
    v += dpp_d<0x4E>(v);
    v += dpp_d<0x141>(v);
    if (G >= 16) v += dpp_d<0x140>(v);
    if (G >= 32) v += __shfl_xor(v, 16, 64);
    if (G >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}
// maximum that keeps a NaN (fmax drops it): a residual with a NaN in it must not pass an acceptance test
__device__ __forceinline__ double nmax(double a, double b) { return (b > a || b != b) ? b : a; }
template <int G> __device__ __forceinline__ double g_max(double v)
{
    v = nmax(v, dpp_d<0xB1>(v));
    v = nmax(v, dpp_d<0x4E>(v));
    v = nmax(v, dpp_d<0x141>(v));
    if (G >= 16) v = nmax(v, dpp_d<0x140>(v));
    if (G >= 32) v = nmax(v, __shfl_xor(v, 16, 64));
    if (G >= 64) v = nmax(v, __shfl_xor(v, 32, 64));
    return v;
}
template <int G> __device__ __forceinline__ int g_sum_i(int v)
{
    v += dpp_i<0xB1>(v);
    v += dpp_i<0x4E>(v);
    v += dpp_i<0x141>(v);
    if (G >= 16) v += dpp_i<0x140>(v);
    if (G >= 32) v += __shfl_xor(v, 16, 64);
    if (G >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}
template <int G> __device__ __forceinline__ bool g_any(int v)
{
    const unsigned long long mk = __ballot(v != 0);
    if (G == 64) return mk != 0ull;
    const int sh = threadIdx.x & ~(G - 1);
    return ((mk >> sh) & ((1ull << (G & 63)) - 1ull)) != 0ull;
}
// value of lane k of the group (k is a compile-time constant after unrolling)
template <int G> __device__ __forceinline__ double g_bcast(double v, int k)
{
    if (G == 64) return wave_bcast(v, k);
    if (G == 8) {
        double t;
        switch (k & 3) {
            case 0: t = dpp_d<0x00>(v); break;
            case 1: t = dpp_d<0x55>(v); break;
            case 2: t = dpp_d<0xAA>(v); break;
            default: t = dpp_d<0xFF>(v); break;
        }
        const double u = dpp_d<0x141>(t);
        return ((((int)threadIdx.x >> 2) & 1) == (k >> 2)) ? t : u;
    }
    return __shfl(v, k, G);
}
// LDS traffic of one wave is in order; this keeps the compiler from moving LDS accesses across the point
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// global memory written by one lane of the group and read by another: wait for the stores (no barrier: the group is inside one wave)
__device__ __forceinline__ void g_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ---- loops over the entries of a vector, G lanes per instance ------------------------------------------------------------------
// One or two wavefronts per SIMD cannot hide a load behind other waves, so every loop is software-pipelined: the loads of the next
// tile of U*G elements (load(i) returns them by value) are issued before the stores of the current tile (store(i, v)).  Legal for
// element-wise loops only: store(i, .) must not write what load(j) reads for j != i.
template <int G, int U, class L, class S>
__device__ __forceinline__ void g_map(int n, int gl, L load, S store)
{
    using T = typename val_of<decltype(load(0))>::type;
    T v[U];
    gl = here(gl);
    // the first trip only loads (tile 0): keeping these loads inside the loop keeps their addresses from being hoisted to the top
    // of the kernel as loop invariants of the outer loops (one 64-bit address per vector and tile element, hundreds of registers)
    for (int i0 = gl - U * G; i0 < n; i0 += U * G) {
        T w[U];
        const int i1 = i0 + U * G;
        if (i1 - gl < n) {
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i1 + u * G; w[u] = load(i < n ? i : 0); }
        }
        if (i0 >= 0) {
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * G; if (i < n) store(i, v[u]); }
        }
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = w[u];
    }
}
struct D2 { double a, b; };
struct D3 { double a, b, c; };
struct D4 { double a, b, c, d; };
struct ID { int i; double a; };

// ---- sparse products: lane per row / per column of the pattern, in ELL form ----------------------------------------------------------
// The pattern is shared by the batch, so the host lays it out once as ELL slabs: eidx[q * rows + i] = index of the q-th entry of row
// i into the gathered vector, epos[q * rows + i] = its position in the instance's value array (-1: no such entry), q < W (4 or 8);
// longer rows finish in a scalar tail over the CSR/CSC arrays.  Per tile of U*G rows: the values and the gathered vector entries of
// the tile and the indices of the NEXT tile are in flight together.  xv(j) returns a D2 (two vectors share one pass over the
// matrix); pre(i) loads what the consumer needs beside the sums; out(i, s0, s1, pre) consumes.

template <int G, int U, int W, bool MAP, class Xv, class Pre, class Out>
__device__ __forceinline__ void g_ell(const EllMat& E, int gl, GD vals, Xv xv, Pre pre, Out out)
{
    const int rows = E.rows;
    gl = here(gl);
    // indices of a tile: the column slab and either the position slab (a value map: E^T over E's values) or the row's two pointers --
    // without a map the values of a row lie in row order, position of entry q = ptr[i] + q: two loads per row instead of W (round 5)
    constexpr int PW = MAP ? W : 2;
    constexpr bool mapped = MAP;
    constexpr bool PREF = !MAP;   // with a map the next tile's 2 W indices per row do not fit the register budget of the G = 8 scheduler kernel
    int ci[U][W], pa[U][PW];      // pa: positions (map) / pa[u][0], pa[u][1] = ptr[i], ptr[i + 1] (no map)
    auto load_idx = [&](int t0, int (&c)[U][W], int (&p)[U][PW]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = t0 + u * G; const bool ok = i < rows;
#pragma unroll
            for (int q = 0; q < W; q++) {
                c[u][q] = ok ? E.eidx[q * rows + i] : 0;
                if (mapped) p[u][q % PW] = ok ? E.epos[q * rows + i] : -1;
            }
            if (!mapped) { p[u][0] = ok ? E.ptr[i] : 0; p[u][1] = ok ? E.ptr[i + 1] : 0; }
        }
    };
    if (gl < rows) load_idx(gl, ci, pa);
    for (int i0 = gl; i0 < rows; i0 += U * G) {
        int ps[U][W];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int q = 0; q < W; q++)
                ps[u][q] = mapped ? pa[u][q % PW] : ((pa[u][0] + q < pa[u][1]) ? pa[u][0] + q : -1);
        double a[U][W]; D2 xs[U][W];
        typename val_of<decltype(pre(0))>::type pv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int q = 0; q < W; q++) {
                const bool ok = ps[u][q] >= 0;
                const double av = vals[ok ? ps[u][q] : 0];
                const D2 xv2 = xv(ok ? ci[u][q] : 0);
                a[u][q] = ok ? av : 0.0; xs[u][q].a = ok ? xv2.a : 0.0; xs[u][q].b = ok ? xv2.b : 0.0;
            }
            const int i = i0 + u * G;
            pv[u] = pre(i < rows ? i : 0);
        }
        // the indices of the NEXT tile go out behind this tile's values: one round trip per tile instead of two
        int cn[U][W], pn[U][PW];
        const bool more = i0 + U * G < rows;
        if (PREF && more) load_idx(i0 + U * G, cn, pn);
#pragma unroll
        for (int u = 0; u < U; u++) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int q = 0; q < W; q++) { s0 += a[u][q] * xs[u][q].a; s1 += a[u][q] * xs[u][q].b; }
            const int i = i0 + u * G;
            if (i < rows) {
                if (E.tails)
                    for (int k = E.ptr[i] + W; k < E.ptr[i + 1]; k++) {
                        const double av = vals[E.cmap ? E.cmap[k] : k]; const D2 xv2 = xv(E.cidx[k]);
                        s0 += av * xv2.a; s1 += av * xv2.b;
                    }
                out(i, s0, s1, pv[u]);
            }
        }
        if (PREF) {
            if (more) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int q = 0; q < W; q++) { ci[u][q] = cn[u][q]; pa[u][q % PW] = pn[u][q % PW]; }
            }
        } else if (more) load_idx(i0 + U * G, ci, pa);
    }
}
// dispatch on the slab width of the pattern (4 or 8)
template <int G, bool MAP, class Xv, class Pre, class Out>
__device__ __forceinline__ void sp_ell(const EllMat& E, int gl, GD vals, Xv xv, Pre pre, Out out)
{
    if (E.W == 4) g_ell<G, 4, 4, MAP>(E, gl, vals, xv, pre, out);
    else g_ell<G, 2, 8, MAP>(E, gl, vals, xv, pre, out);
}
struct NoPre { };

template <int G> __device__ __forceinline__ void sp_Ex(SpCtx<G>& c, GD x, GD out)
{
    SPROF(c, SP_VECTORS);
    sp_ell<G, false>(c.db->ellE, c.gl, c.Ex(), [&](int j) { return D2{x[j], 0.0}; }, [](int) { return NoPre{}; }, [&](int r, double s, double, NoPre) { out[r] = s; });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
// two vectors through one pass over Q: o0 = Q x0, o1 = Q x1
template <int G> __device__ __forceinline__ void sp_Qx2(SpCtx<G>& c, GD x0, GD x1, GD o0, GD o1)
{
    SPROF(c, SP_VECTORS);
    sp_ell<G, false>(c.db->ellQ, c.gl, c.Qx(), [&](int j) { return D2{x0[j], x1[j]}; }, [](int) { return NoPre{}; },
              [&](int i, double s0, double s1, NoPre) { o0[i] = s0; o1[i] = s1; });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
// out[i] = base(pre(i)) - (E'y)[i]   (column gather over the CSC of E); returns max |out| over the group
template <int G, class Pre, class Base> __device__ __forceinline__ double sp_ETy(SpCtx<G>& c, GD y, GD out, Pre pre, Base base)
{
    SPROF(c, SP_VECTORS);
    double mx = 0.0;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(), [&](int r) { return D2{y[r], 0.0}; }, pre,
              [&](int i, double s, double, typename val_of<decltype(pre(0))>::type pv) { const double v = base(pv) - s; out[i] = v; mx = nmax(mx, fabs(v)); });
    g_sync();
    SPROF(c, SP_PRODUCTS);
    return g_max<G>(mx);
}
// the residual of the stationarity condition in one pass over Q and E' (both indexed by the variable):
// r1[i] = (-g[i] - (Q x)[i]) - (E'y)[i]; returns max |r1|
// r1 = -g - Q x - E'y; returns |r1|_inf and, in `scale`, max_i(|g_i| + |Q x|_i + |E'y|_i): the residual's own rounding floor is 64 eps of that (round 6, as on
// the dense path: qp_polish in lcqp_dev.hpp)
template <int G> __device__ __forceinline__ double sp_residual(SpCtx<G>& c, GD g, GD x, GD y, GD r1, GD qx, double& scale)
{
    SPROF(c, SP_VECTORS);
    sp_ell<G, false>(c.db->ellQ, c.gl, c.Qx(), [&](int j) { return D2{x[j], 0.0}; }, [](int) { return NoPre{}; }, [&](int i, double s, double, NoPre) { qx[i] = s; });
    g_sync();
    double mx = 0.0, sc = 0.0;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(), [&](int r) { return D2{y[r], 0.0}; }, [&](int i) { return D2{g[i], qx[i]}; },
              [&](int i, double s, double, D2 pv) { const double v = (-pv.a - pv.b) - s; r1[i] = v; mx = nmax(mx, fabs(v)); sc = fmax(sc, fabs(pv.a) + fabs(pv.b) + fabs(s)); });
    g_sync();
    SPROF(c, SP_PRODUCTS);
    scale = g_max<G>(sc);
    return g_max<G>(mx);
}
// C v = L'(R v) + R'(L v) for two vectors: lx = E v (rows of L: nC .. nC+nComp, of R: nC+nComp ..), then a column gather with
// swapped coefficients
template <int G> __device__ __forceinline__ void sp_Cx2(SpCtx<G>& c, GD v0, GD v1, GD o0, GD o1)
{
    SPROF(c, SP_VECTORS);
    GD lx0 = c.M(MV_LX), lx1 = c.M(MV_LX2);
    sp_ell<G, false>(c.db->ellE, c.gl, c.Ex(), [&](int j) { return D2{v0[j], v1[j]}; }, [](int) { return NoPre{}; },
              [&](int r, double s0, double s1, NoPre) { lx0[r] = s0; lx1[r] = s1; });
    g_sync();
    const int nC = c.db->nC, nK = c.db->nComp;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(),
              [&](int r) { const int rr = r >= nC + nK ? r - nK : (r >= nC ? r + nK : -1);      // R'(L v) + L'(R v)
                           return rr >= 0 ? D2{lx0[rr], lx1[rr]} : D2{0.0, 0.0}; },
              [](int) { return NoPre{}; }, [&](int i, double s0, double s1, NoPre) { o0[i] = s0; o1[i] = s1; });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
// C v from lx = E v that somebody else has computed (the polish leaves E x of its solution), for one vector or two:
// out(i, (C v0)[i], (C v1)[i], pre(i))
template <int G, bool TWO, class Pre, class Out> __device__ __forceinline__ void sp_C_from_Ex(SpCtx<G>& c, GD lx0, GD lx1, Pre pre, Out out)
{
    SPROF(c, SP_VECTORS);
    const int nC = c.db->nC, nK = c.db->nComp;
    sp_ell<G, true>(c.db->ellT, c.gl, c.Ex(),
              [&](int r) { const int rr = r >= nC + nK ? r - nK : (r >= nC ? r + nK : -1);
                           return rr >= 0 ? D2{lx0[rr], TWO ? (double)lx1[rr] : 0.0} : D2{0.0, 0.0}; },
              pre, [&](int i, double s0, double s1, typename val_of<decltype(pre(0))>::type pv) { out(i, s0, s1, pv); });
    g_sync();
    SPROF(c, SP_PRODUCTS);
}
template <int G> __device__ __forceinline__ double sp_maxabs(const SpCtx<G>& c, GD a, int n)
{
    double s = 0.0;
    const int gl = here(c.gl);
#pragma unroll 8
    for (int i = gl; i < n; i += G) s = fmax(s, fabs(a[i]));
    return g_max<G>(s);
}

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

// ---- ADMM iterations (OSQP, KKT form; oracle: sqp_admm) ----------------------------------------------------------------------
template <int G>
__device__ __forceinline__ void sp_admm(SpCtx<G>& c, GD g, int n_it)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    const double alpha = db.opt.admmAlpha, sigma = c.info->sigma;
    GD xa = c.V(NV_XA), ya = c.M(MV_YA), za = c.M(MV_ZA), b = c.Nv();
    GD l = c.M(MV_L), u = c.M(MV_U), rhov = c.M(MV_RHOV);
    for (int it = 0; it < n_it; it++) {
        for (int i = t; i < n; i += G) b[db.iperm[i]] = sigma * xa[i] - g[i];
        for (int r = t; r < m; r += G) b[db.iperm[n + r]] = za[r] - ya[r] / rhov[r];
        g_sync();
        sp_solve<G>(c, true, b);
        for (int r = t; r < m; r += G) {
            const double rv = rhov[r];
            const double zt = za[r] + (b[db.iperm[n + r]] - ya[r]) / rv;
            const double zr = alpha * zt + (1.0 - alpha) * za[r];
            if (isinf(l[r]) && isinf(u[r])) { za[r] = zr; ya[r] = 0.0; continue; }
            const double zn = fmin(fmax(zr + ya[r] / rv, l[r]), u[r]);
            ya[r] += rv * (zr - zn);
            za[r] = zn;
        }
        for (int i = t; i < n; i += G) xa[i] = alpha * b[db.iperm[i]] + (1.0 - alpha) * xa[i];
        g_sync();
        c.cAdmm++;
    }
}

// ---- the phases of an instance's homotopy (k_sparse_sched runs them) -----------------------------------------------------------------------
// Every routine below is called by the G lanes of one instance with that instance's context and state record (all values uniform inside the
// group) and returns the phase the instance enters next (PH_NUM: finished).  Together they are runSolver (src/LCQProblem.cpp:444-560), the
// subsolver call (oracle: sqp_solve) and the polish (oracle: sqp_polish) of round 3, cut at the points where instances of one wavefront used
// to part: before a trial, before a factorisation, before a correction, at the end of a QP.
struct StRow { int s; double e, lo, hi, y; };
struct I2 { int a, b; };
struct I2D { int a, b; double y; };
struct ID4 { int p, s; double lo, hi, e; };
struct ID2 { int s; double v, y; };
struct ID3 { int s; double lo, hi, z, y; };

// the polish starts (oracle: sqp_polish, entry): tolerances scale with 1 + |g|_inf
template <int G>
__device__ __forceinline__ int sp_polish_begin(SpCtx<G>& c, SpState& S, GD g, int reuse)
{
    const lcqp_options_t& o = c.db->opt;
    S.gs = 1.0 + ((reuse && S.gmaxNext >= 0.0) ? S.gmaxNext : sp_maxabs<G>(c, g, c.db->n));      // (the LCQP level knows max|g| of the vector it has just formed)
    S.ytol = o.feasTol * S.gs;
    S.fact_valid = 0; S.borderTodo = 0;
    S.dpUsed = c.info->delta; S.d2Used = c.info->delta2;      // regularisation of the factorisation in use
    S.trial = 0; S.reuse = reuse; S.nrefine = 0; S.xinf = 0.0;
    return PH_TRIAL;
}

// the instance is finished: statistics and solution go out
template <int G>
__device__ __forceinline__ int sp_finish(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const int t = here(c.gl), n = db.n, m = db.m;
    GD xk = c.V(NV_XK), yk = c.M(MV_YK);
    S.st.status = S.algoStat; S.st.returnValue = S.rc;
    S.st.admmIter = c.cAdmm; S.st.trials = c.cTrials; S.st.factorizations = c.cFact; S.st.corrections = c.cCorr; S.st.reserved = c.cSweeps;
    for (int i = t; i < n; i += G) db.xout[(size_t)c.b * n + i] = xk[i];
    for (int r = t; r < m; r += G) db.yout[(size_t)c.b * m + r] = yk[r];
    if (t == 0) { db.stats[c.b] = S.st; c.info->bytes += c.bytes; }
    c.bytes = 0.0;
    return PH_NUM;
}

// a polish that did not settle (oracle: the tail of the round loop of sqp_solve): twice as many ADMM iterations, or the QP has failed
template <int G>
__device__ __forceinline__ int sp_polish_failed(SpCtx<G>& c, SpState& S)
{
    const lcqp_options_t& o = c.db->opt;
    S.n_admm = 2 * S.n_admm;
    if (S.n_admm < 10) S.n_admm = 10;
    if (S.n_admm > 400) S.n_admm = 400;
    S.round++;
    if (S.round < o.maxRounds) return PH_ROUND;
    S.qpIter = (c.cTrials - S.trials0) + (c.cAdmm - S.admm0);
    S.st.subproblemIter += S.qpIter; S.st.qpSolverExitFlag = 1; S.st.qpSolves++;
    S.rc = LCQP_SUBPROBLEM_SOLVER_ERROR;
    return sp_finish<G>(c, S);
}

// PH_TRIAL: the head of one trial of the polish -- E x, the status test, the true residual when the working set did not change, acceptance;
// else the leaving rows, and whether the factorisation still matches the working set
template <int G>
__device__ __forceinline__ int sp_ph_trial(SpCtx<G>& c, SpState& S, GD g)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n, m = db.m, trial = S.trial;
    GD x = c.V(NV_XT), r1 = c.V(NV_R1), qx = c.V(NV_TMP), yt = c.M(MV_YT), ex = c.M(MV_EX);
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI st = c.I(MI_STT), stf = c.I(MI_STF), newst = c.I(MI_NEW);
    const double gs = S.gs, ytol = S.ytol;
    c.cTrials++;
    // Two stages, as on the dense path (oracle: sqp_polish).  Stage 1 is what every trial needs: E x, for the status test.  Stage 2 -- the
    // true residual, one pass over Q and one over E' -- runs only when stage 1 changed nothing: after a correction the residual is zero on
    // the old working set up to rounding and regularisation, so when the set changes the next right-hand side is known without it (the
    // multipliers of the leaving rows, below); the trial that accepts always has the true residual.
    double res_stat = 0.0;
    int have_r1 = 0;
    double res_eq = 0.0, bmax = 0.0;
    int chg = 0, act = 0, loose = 0;
    // active rows are held to the rounding floor of a computed E_r x, 16 eps (|b_r| + |E_r|_1 |x|_inf), before a point is accepted (round 5;
    // oracle: sqp_polish; dense twin: qp_polish in lcqp_dev.hpp): runSolver ends on phi < 1e3 eps, a sum of products of such residuals
    const double exScale = c.info->e1max * S.xinf;
    auto status = [&](int r, StRow v) {
        int ns = v.s;
        if (v.s == ST_INACT) {
            const double ftol = o.feasTol * (1.0 + fabs(v.e));
            if (v.e < v.lo - ftol) ns = ST_LOWER;
            else if (v.e > v.hi + ftol) ns = ST_UPPER;
        } else {
            const double bb = (v.s == ST_UPPER) ? v.hi : v.lo;
            const bool above = !(fabs(bb - v.e) <= 16.0 * 2.221e-16 * (fabs(bb) + exScale));      // (a NaN counts) a row at the rounding floor of its computed E_r x is not a residual (round 6)
            if (above) res_eq = nmax(res_eq, fabs(bb - v.e));
            bmax = fmax(bmax, fabs(bb));
            loose |= above;
            if (v.s == ST_LOWER && v.y > ytol) ns = ST_INACT;
            if (v.s == ST_UPPER && v.y < -ytol) ns = ST_INACT;
        }
        newst[r] = ns;
        chg += (ns != v.s);
        act += (ns != ST_INACT);
    };
    if (trial == 0 && S.reuse) {
        // hot start with an unchanged (x, y): r1 = r1_last + (g_last - g) and E x are in place -- the residual and E x of the accepted
        // trial stay where they are, and the LCQP level adds (g_last - g) to r1 in the pass that forms the new g (sp_ph_qpend)
        have_r1 = 1;
        g_map<G, 4>(m, t, [&](int r) { return StRow{st[r], ex[r], l[r], u[r], yt[r]}; }, status);
    } else {
        // E x and the status test in ONE pass (round 5): the row's state rides along as the product's `pre`, the sum goes straight into the
        // test and into ex (the right-hand side of the correction needs it) -- no second pass over st, ex, l, u, y
        SPROF(c, SP_VECTORS);
        sp_ell<G, false>(db.ellE, c.gl, c.Ex(), [&](int j) { return D2{x[j], 0.0}; },
                  [&](int r) { return StRow{st[r], 0.0, l[r], u[r], yt[r]}; },
                  [&](int r, double s0, double, StRow v) { ex[r] = s0; v.e = s0; status(r, v); });
        g_sync();
        SPROF(c, SP_PRODUCTS);
        c.bytes += db.by[BY_EX];
    }
    const int changed = g_sum_i<G>(chg), nact = g_sum_i<G>(act);
    res_eq = g_max<G>(res_eq);
    bmax = g_max<G>(bmax);
    SPROF(c, SP_ASSEMBLE);      // (profile builds: the status test on its own)
    double rscale = 0.0;
    if (!have_r1 && (trial == 0 || !changed)) {
        res_stat = sp_residual<G>(c, g, x, yt, r1, qx, rscale);
        c.cSweeps++;
        c.bytes += db.by[BY_SWEEP];
        have_r1 = 1;
    }
    if (trial > 0 && !changed && res_stat <= fmax(o.resTol * gs, 64.0 * 2.221e-16 * rscale) && res_eq <= o.resTol * (1.0 + bmax)) {
        if (!(g_any<G>(loose) && S.nrefine < 2 && trial + 1 < o.maxTrials)) return PH_QPEND;      // a verified KKT point
        S.nrefine++;      // ... whose active rows can be held more exactly: one more correction
    }
    if (changed && trial > 0) {
        if (trial >= 2 && nact > n && changed > max(n / 2, 32)) return sp_polish_failed<G>(c, S);       // overshooting cold start: hand over to ADMM
        // leaving rows: their multipliers leave the residual (r1 += E_r' y_r), then the new working set takes over
        GD ytmp = c.M(MV_LX);
        g_sync();
        g_map<G, 8>(m, t, [&](int r) { return I2D{newst[r], st[r], yt[r]}; },
                    [&](int r, I2D v) { const bool leaves = (v.a == ST_INACT && v.b != ST_INACT); ytmp[r] = leaves ? -v.y : 0.0; st[r] = v.a; if (leaves && v.y != 0.0) yt[r] = 0.0; });
        g_sync();
        // r1 - E'(-y_leaving) = r1 + E'y_leaving; without a true residual r1 is the predicted one: nothing was left on the old working set
        if (have_r1) sp_ETy<G>(c, ytmp, r1, [&](int i) { return r1[i]; }, [](double v) { return v; });
        else sp_ETy<G>(c, ytmp, r1, [](int) { return NoPre{}; }, [](NoPre) { return 0.0; });
        S.fact_valid = 0;
    }
    if (!S.fact_valid) {
        int diff = (c.info->stfValid == 0);
#pragma unroll 8
        for (int r = t; r < m; r += G) diff |= ((stf[r] != ST_INACT) != (st[r] != ST_INACT));
        if (g_any<G>(diff)) return PH_FACTOR;
        S.fact_valid = 1;
    }
    return PH_CORRECT;
}

// PH_FACTOR: the band LDL' of [Q + delta I, Ea'; Ea, -delta2 I] for the working set in MI_STT
template <int G>
__device__ __forceinline__ int sp_ph_factor(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    GI st = c.I(MI_STT), stf = c.I(MI_STF);
    // Two levels of regularisation, as on the dense path (proxSmall / proxBig).  A correction with the safe level leaves
    // delta dx and delta2 dy (1e-8, 1e-9 relative) in the true residuals: every QP paid one refinement trial -- a sweep, a band
    // solve, the vector passes -- for the regularisation alone.  The light level (1e-12, 1e-14) is accepted at once.  The band
    // LDL' is not pivoted, so the light level needs an ordering in which every row follows one of its variables (lightOK, chosen
    // by the host when every Hessian of the batch is safely definite) and is only kept when every pivot has the sign its node
    // prescribes and a safe size; a variable's pivot failing makes the safe level permanent for the instance.
    int level = (db.lightOK && !c.info->bigReg) ? 0 : 1;
    // the working set as a bit set in LDS: the factorisation asks for the membership of the row behind every entry of E it meets (up to
    // 2 w per band row) -- from memory these were gathers of 4-byte flags, 8 instances apart in one wavefront
    unsigned* bits = nullptr;
    if (G <= 16 && db.bitWords > 0) {
        bits = reinterpret_cast<unsigned*>(sp_dyn_lds) + (size_t)((int)threadIdx.x / G) * db.bitWords;
        for (int w = t; w < db.bitWords; w += G) {
            unsigned word = 0u;
#pragma unroll 8
            for (int k = 0; k < 32; k++) { const int r = w * 32 + k; if (r < m && st[r] != ST_INACT) word |= 1u << k; }
            bits[w] = word;
        }
        wave_sync();
    }
    for (;;) {
        S.dpUsed = level ? c.info->delta : c.info->deltaS;
        S.d2Used = level ? c.info->delta2 : c.info->delta2S;
        const double d2 = S.d2Used;
        if (bits) sp_factor_band<G>(c, c.KF(false), c.KD(false), S.dpUsed, [=](int) { return d2; }, [=](int r) { return ((bits[r >> 5] >> (r & 31)) & 1u) != 0u; });
        else sp_factor_band<G>(c, c.KF(false), c.KD(false), S.dpUsed, [=](int) { return d2; }, [=](int r) { return st[r] != ST_INACT; });
        if (level == 1) break;
        int badVar = 0, badRow = 0;
        GD Kd = c.KD(false);
        const double sc = c.info->scale, vmax = 1.0 / (1e-8 * sc), rmax = sc / 1e-8;
        const int Nb = db.N - db.kb;
#pragma unroll 4
        for (int p = t; p < Nb; p += G) {
            const double kd = Kd[p];            // 1 / D
            const int node = db.pnode[p];
            if (node < n) badVar |= !(kd > 0.0 && kd < vmax);
            else if (st[node - n] != ST_INACT) badRow |= !(kd < 0.0 && kd > -rmax);
        }
        const bool bv = g_any<G>(badVar), br = g_any<G>(badRow);
        if (!bv && !br) break;
        if (bv && t == 0) c.info->bigReg = 1;
        level = 1;
    }
    if (db.kb > 0) { sp_border_prepare<G>(c, false, [=](int r) { return st[r] != ST_INACT; }); S.borderTodo = db.kb; }
    g_map<G, 8>(m, t, [&](int r) { return st[r]; }, [&](int r, int v) { stf[r] = v; });
    if (t == 0) c.info->stfValid = 1;
    g_sync();
    S.fact_valid = 1;
    return PH_CORRECT;
}

// PH_CORRECT: [Q + delta I, Ea'; Ea, -delta2 I][dx; dy] = [r1; ba - Ea x], x += dx, y += dy; then the next trial (or the polish has run out of trials)
template <int G>
__device__ __forceinline__ int sp_ph_correct(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    GD x = c.V(NV_XT), r1 = c.V(NV_R1), yt = c.M(MV_YT), ex = c.M(MV_EX), b = c.Nv();
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI st = c.I(MI_STT);
    const int* iperm = db.iperm;
    SPROF(c, SP_VECTORS);
    // (deep tiles: the band's lane groups are 8 lanes wide, a pass over n is n / (8 U) round trips)
    g_map<G, 16>(n, t, [&](int i) { return ID{iperm[i], r1[i]}; }, [&](int, ID v) { b[v.i] = v.a; });
    g_map<G, 6>(m, t, [&](int r) { return ID4{iperm[n + r], st[r], l[r], u[r], ex[r]}; },
                [&](int, ID4 v) { b[v.p] = (v.s != ST_INACT) ? ((v.s == ST_UPPER) ? v.hi : v.lo) - v.e : 0.0; });
    g_sync();
    SPROF(c, SP_RHS);
    // one call site of the band solve: first the columns of W = U inv(Bd) a fresh factorisation owes (none for a plain band), then b
    const int borderTodo = S.borderTodo;
    for (int jb = 0; jb <= borderTodo; jb++) {
        GD vec = b;
        if (jb < borderTodo) vec = sp_border_column<G>(c, false, jb);
        else if (borderTodo > 0) { const double d2 = S.d2Used; sp_border_schur<G>(c, false, S.dpUsed, [=](int) { return d2; }, [=](int r) { return st[r] != ST_INACT; }); }
        sp_solve_band<G>(c, false, vec);
    }
    S.borderTodo = 0;
    if (db.kb > 0) sp_border_solve<G>(c, false, b);
    double xm = 0.0;
    g_map<G, 12>(n, t, [&](int i) { return D2{b[iperm[i]], x[i]}; }, [&](int i, D2 v) { const double xn = v.b + v.a; x[i] = xn; xm = fmax(xm, fabs(xn)); });
    S.xinf = g_max<G>(xm);
    g_map<G, 10>(m, t, [&](int r) { return ID2{st[r], b[iperm[n + r]], yt[r]}; }, [&](int r, ID2 v) { if (v.s != ST_INACT) yt[r] = v.y + v.v; });
    g_sync();
    c.cCorr++;
    S.trial++;
    if (S.trial >= c.db->opt.maxTrials) return sp_polish_failed<G>(c, S);
    return PH_TRIAL;
}

// the subsolver call starts (oracle: sqp_solve, entry): SubsolverBase::solve on the OSQP arm.  A hot start from the stored solution goes
// straight to the polish; everything else takes the round preamble (PH_ROUND).
// warmFirst (sp_ph_start of a warm re-solve, k_sparse_refresh): the first QP of the homotopy is a hot start on the stored point and working
// set -- but the stored residual and E x belong to the g and the bounds of the run before, so the polish takes its cold entry there.
template <int G>
__device__ __forceinline__ int sp_qp_begin(SpCtx<G>& c, SpState& S, GD g, bool warmFirst = false)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n, m = db.m, initial = S.initial && !warmFirst;
    GD xq = c.V(NV_XQ), xa = c.V(NV_XA), xt = c.V(NV_XT);
    GD yq = c.M(MV_YQ), ya = c.M(MV_YA), yt = c.M(MV_YT);
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI st = c.I(MI_ST), stt = c.I(MI_STT);
    S.trials0 = c.cTrials; S.admm0 = c.cAdmm; S.qpIter = 0;
    S.n_admm = initial ? o.admmFirst : o.admmHot;
    S.use_stored = (!initial && c.info->haveSolution && S.n_admm == 0);
    // The ADMM iterate (xa, ya) starts as a copy of the stored solution.  A hot start hands the stored solution to the polish directly and
    // the copy is made only if the polish fails and an ADMM round follows (one QP in a thousand on the synthetic workload).
    S.backup_pending = 0;
    if (initial) {
        GD x0 = c.V(NV_X0), y0 = c.M(MV_Y0);
        const int hasY0 = c.info->hasY0;
        g_map<G, 8>(n, t, [&](int i) { return x0[i]; }, [&](int i, double v) { xq[i] = v; xa[i] = v; });
        g_map<G, 8>(m, t, [&](int r) { return y0[r]; }, [&](int r, double v) { const double yv = hasY0 ? -v : 0.0; yq[r] = yv; ya[r] = yv; });
    } else if (S.use_stored) {
        S.backup_pending = 1;
    } else {
        g_map<G, 8>(n, t, [&](int i) { return xq[i]; }, [&](int i, double v) { xa[i] = v; });
        g_map<G, 8>(m, t, [&](int r) { return yq[r]; }, [&](int r, double v) { ya[r] = v; });
    }
    g_sync();
    S.admm_ready = 0; S.round = 0;
    if (!S.use_stored) return PH_ROUND;
    g_map<G, 4>(m, t, [&](int r) { return ID3{st[r], l[r], u[r], 0.0, yq[r]}; },
                [&](int r, ID3 v) { const int s = (v.lo == v.hi) ? ST_EQ : v.s; stt[r] = s; yt[r] = (s != ST_INACT) ? v.y : 0.0; });
    // (xt is xq already: the stored solution is the accepted trial vector of the QP before, copied from xt in sp_ph_qpend, and nothing has
    // written xt since -- use_stored is only set behind that copy)
    g_sync();
    return sp_polish_begin<G>(c, S, g, warmFirst ? 0 : 1);
}

// PH_ROUND: the preamble of a round that does not start from the stored solution -- the first QP of a homotopy, and every round after a
// polish that failed: ADMM iterations from (xa, ya), the working set they propose, the polish from there
template <int G>
__device__ __forceinline__ int sp_ph_round(SpCtx<G>& c, SpState& S, GD g)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m;
    GD xq = c.V(NV_XQ), xa = c.V(NV_XA), xt = c.V(NV_XT);
    GD yq = c.M(MV_YQ), ya = c.M(MV_YA), za = c.M(MV_ZA), yt = c.M(MV_YT);
    GD l = c.M(MV_L), u = c.M(MV_U);
    GI stt = c.I(MI_STT);
    if (S.backup_pending && S.round > 0) {
        g_map<G, 8>(n, t, [&](int i) { return xq[i]; }, [&](int i, double v) { xa[i] = v; });
        g_map<G, 8>(m, t, [&](int r) { return yq[r]; }, [&](int r, double v) { ya[r] = v; });
        g_sync();
        S.backup_pending = 0;
    }
    if (!S.admm_ready) {
        sp_Ex<G>(c, xa, za);
        g_map<G, 8>(m, t, [&](int r) { return D3{za[r], l[r], u[r]}; },
                    [&](int r, D3 v) { za[r] = fmin(fmax(v.a, v.b), v.c); if (isinf(v.b) && isinf(v.c)) ya[r] = 0.0; });
        g_sync();
        S.admm_ready = 1;
    }
    if (S.n_admm > 0) sp_admm<G>(c, g, S.n_admm);
    g_map<G, 4>(m, t, [&](int r) { return ID3{0, l[r], u[r], za[r], ya[r]}; },
                [&](int r, ID3 v) {
                    int s = ST_INACT;
                    if (isfinite(v.lo) && (v.z - v.lo < -v.y)) s = ST_LOWER;
                    if (isfinite(v.hi) && (v.hi - v.z < v.y)) s = ST_UPPER;
                    if (v.lo == v.hi) s = ST_EQ;
                    stt[r] = s;
                    yt[r] = (s != ST_INACT) ? v.y : 0.0;
                });
    g_map<G, 8>(n, t, [&](int i) { return xa[i]; }, [&](int i, double v) { xt[i] = v; });
    g_sync();
    return sp_polish_begin<G>(c, S, g, 0);
}
// ---- LCQProblem::runSolver, OSQP_SPARSE arm (oracle: orc_sparse_lcqp_solve) ----------------------------------------------------
// PH_START: everything in front of the first QP
template <int G>
__device__ __forceinline__ int sp_ph_start(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n;
    GD g = c.V(NV_G), gtil = c.V(NV_GTIL), xk = c.V(NV_XK), gk = c.V(NV_GK);
    GD Qx = c.V(NV_QX), Cx = c.V(NV_CX), Qp = c.V(NV_QP), Cp = c.V(NV_CP);
    memset(&S.st, 0, sizeof(S.st));
    S.rc = 0; S.qpIter = 0; S.histLen = 0; S.algoStat = 0; S.totalIter = 0;
    // warm (k_sparse_refresh): the pass that follows is still the first of the homotopy -- no step length, no perturbation, rhoOpt = rho --
    // but it starts at the last solution (NV_XK still holds it) and at the penalty rho0, without the zero-penalty QP, and its QP is a hot
    // start on the stored point and working set (sp_qp_begin)
    const int warm = c.info->warm;
    S.alphak = 1.0; S.rho = warm ? c.info->rho0 : o.initialPenaltyParameter;
    S.perturbCounter = 0;
    if (db.traceCap > 0 && t == 0) db.traceLen[c.b] = 0;     // a run that records nothing leaves an empty trace
    if (warm) {
        const double rho = S.rho;
        if (db.hasLbL || db.hasLbR) { GD gphi = c.V(NV_GPHI); g_map<G, 8>(n, t, [&](int i) { return D2{g[i], gphi[i]}; }, [&](int i, D2 v) { gtil[i] = v.a + rho * v.b; }); }
        else g_map<G, 8>(n, t, [&](int i) { return g[i]; }, [&](int i, double v) { gtil[i] = v; });
    } else {
        GD x0 = c.V(NV_X0);
        g_map<G, 8>(n, t, [&](int i) { return D2{x0[i], g[i]}; }, [&](int i, D2 v) { xk[i] = v.a; gtil[i] = v.b; });
    }
    g_sync();
    // Q x0 and C x0 once; from here on both follow the steps (sp_ph_qpend)
    sp_Qx2<G>(c, xk, xk, Qx, Qp); sp_Cx2<G>(c, xk, xk, Cx, Cp);
    c.bytes += db.by[BY_START];
    if (o.solveZeroPenaltyFirst && !warm) { for (int i = t; i < n; i += G) gk[i] = g[i]; g_sync(); }
    else { const double rho = S.rho; for (int i = t; i < n; i += G) gk[i] = rho * Cx[i] + gtil[i]; g_sync(); }
    S.initial = 1;
    S.gmaxNext = -1.0;      // max |gk| of the next QP when this level has formed it (-1: the subsolver looks)
    return sp_qp_begin<G>(c, S, gk, warm != 0);
}

// PH_QPEND: the subsolver has a verified solution (oracle: the exit of sqp_solve), then one iterate of runSolver's loop up to the next QP
template <int G>
__device__ __forceinline__ int sp_ph_qpend(SpCtx<G>& c, SpState& S)
{
    const SpBatch& db = *c.db;
    const lcqp_options_t& o = db.opt;
    const int t = c.gl, n = db.n, m = db.m, nC = db.nC, nK = db.nComp;
    GD g = c.V(NV_G), gtil = c.V(NV_GTIL), gphi = c.V(NV_GPHI), xk = c.V(NV_XK), pk = c.V(NV_PK), xnew = c.V(NV_XNEW), gk = c.V(NV_GK);
    GD Qx = c.V(NV_QX), Cx = c.V(NV_CX), Qp = c.V(NV_QP), Cp = c.V(NV_CP);
    GD yk = c.M(MV_YK), lx = c.M(MV_LX);
    const bool hasPhi = db.hasLbL || db.hasLbR;
    const double phiConst = c.info->phiConst;
    double* hist = c.info->hist;
    {   // the solution becomes the stored one (sqp_solve's exit)
        GD xq = c.V(NV_XQ), xt = c.V(NV_XT), yq = c.M(MV_YQ), yt = c.M(MV_YT);
        GI st = c.I(MI_ST), stt = c.I(MI_STT);
        S.qpIter = (c.cTrials - S.trials0) + (c.cAdmm - S.admm0);
        // (x: in the pass below that forms pk)
        g_map<G, 8>(m, t, [&](int r) { return ID{stt[r], yt[r]}; }, [&](int r, ID v) { yq[r] = v.a; st[r] = v.i; });
        if (t == 0) c.info->haveSolution = 1;
        g_sync();
    }
    SPROF(c, SP_VECTORS);
    S.st.subproblemIter += S.qpIter; S.st.qpSolverExitFlag = 0; S.st.qpSolves++;
    double rho = S.rho, alphak = S.alphak;
    auto updatePenalty = [&]() {
        if (o.nDynamicPenalty > 0) S.histLen = 0;
        rho *= o.penaltyUpdateFactor;
        S.st.rhoOpt = rho;
        if (hasPhi) { for (int i = t; i < n; i += G) gtil[i] = g[i] + rho * gphi[i]; g_sync(); }
    };
    // What the subsolver's accepted trial leaves behind makes every product of this level but one unnecessary (the dense kernel does
    // the same, lcqp_dev.hpp: lcqp_run): Q xq is in NV_TMP (sp_residual), E xq in MV_EX, and its residual r1 = -gk - Q xq - E'yq (NV_R1, gk still the vector of that QP)
    // gives E'yq.  So pk = xq - xk, Q pk = Q xq - Q xk with Q xk kept up to date below, C xq = L'(R xq) + R'(L xq) is one column
    // gather over E with the entries of E xq, C pk = C xq - C xk, and the stationarity needs no pass over E' of its own.
    // (round 2: one pass over Q, one over E, two over E' per iterate.)
    GD qxs = c.V(NV_TMP), exs = c.M(MV_EX), r1s = c.V(NV_R1), gs0 = gk;
    {
        GD xq = c.V(NV_XQ), xt = c.V(NV_XT), yq = c.M(MV_YQ);
        g_map<G, 8>(n, t, [&](int i) { return D4{xt[i], xk[i], qxs[i], Qx[i]}; }, [&](int i, D4 v) { xq[i] = v.a; xnew[i] = v.a; pk[i] = v.a - v.b; Qp[i] = v.c - v.d; });
        g_map<G, 8>(m, t, [&](int r) { return yq[r]; }, [&](int r, double v) { yk[r] = -v; });     // src/SubsolverOSQP.cpp:196-199
        g_sync();
    }
    const int initial = S.initial;
    bool perturbed = false;
    if (initial) S.st.rhoOpt = rho;
    else if (o.perturbStep) {
        perturbed = true;
        const uint64_t pc = S.perturbCounter;
        for (int i = t; i < n; i += G) {
            uint64_t z = o.perturbSeed + (pc + (uint64_t)i + 1ULL) * opaque_u64(0x9E3779B97F4A7C15ULL);
            z = (z ^ (z >> 30)) * opaque_u64(0xBF58476D1CE4E5B9ULL); z = (z ^ (z >> 27)) * opaque_u64(0x94D049BB133111EBULL); z = z ^ (z >> 31);
            xk[i] += ((int)(z % 3ULL) - 1) * 2.221e-16;
        }
        S.perturbCounter += (uint64_t)n;
        g_sync();
    }
    double sq = 0.0, sl = 0.0;      // pk'(Q + rho C) pk and pk'((Q + rho C) xk + g~)
    if (perturbed) {
        // the perturbation has to reach the penalty gradient rho C xk -- it is there to break the symmetry of problems like warm_up
        // (perturbStep :1353-1362) -- so C xk is taken from the perturbed xk: one more pass over E, the column gather carries two
        // vectors.  (Q xk is not: 2.2e-16 per component is below its rounding; the dense kernel does the same.)
        sp_Ex<G>(c, xk, lx);
        sp_C_from_Ex<G, true>(c, exs, lx, [](int) { return NoPre{}; }, [&](int i, double cxq, double cxk, NoPre) { Cx[i] = cxk; Cp[i] = cxq - cxk; });
        c.bytes += 3.0 * db.by[BY_E];
    } else {
        // C pk and, in the same pass, the two sums of the step length (round 5: they were a pass of their own over pk, Qp, Cp, Qx, Cx, gtil)
        struct D5 { double cx, pk, qp, qx, gt; };
        sp_C_from_Ex<G, false>(c, exs, exs, [&](int i) { return D5{Cx[i], pk[i], Qp[i], Qx[i], gtil[i]}; },
                               [&](int i, double cxq, double, D5 v) {
                                   const double cp = cxq - v.cx;
                                   Cp[i] = cp;
                                   sq += v.pk * (v.qp + rho * cp); sl += v.pk * ((v.qx + rho * v.cx) + v.gt);
                               });
        c.bytes += db.by[BY_E];
    }
    if (!initial) {
        if (perturbed) {
#pragma unroll 4
            for (int i = t; i < n; i += G) { sq += pk[i] * (Qp[i] + rho * Cp[i]); sl += pk[i] * ((Qx[i] + rho * Cx[i]) + gtil[i]); }
        }
        const double qk = g_sum<G>(sq), lk = g_sum<G>(sl);
        alphak = 1.0;
        if (qk > 0 && lk < 0) alphak = fmin(-lk / qk, 1.0);
    }
    S.initial = 0;
    // the step, the products that follow it, and updateStationarity without a box term: statk = Qk xk + g_tilde - E'yk with
    // E'yk = -E'yq = gs0 + Q xq + r1s
    double statMax = 0.0, phiSum = 0.0;
    { struct D10 { double a, b, c, d, e, f, g0, q, r, gt, gp; };
      g_map<G, 3>(n, t, [&](int i) { return D10{xk[i], pk[i], Qx[i], Qp[i], Cx[i], Cp[i], gs0[i], qxs[i], r1s[i], gtil[i], hasPhi ? (double)gphi[i] : 0.0}; },
                  [&](int i, D10 v) {
                      const double qn = v.c + alphak * v.d, cn = v.e + alphak * v.f, xn = v.a + alphak * v.b;
                      xk[i] = xn; Qx[i] = qn; Cx[i] = cn;
                      statMax = nmax(statMax, fabs(((qn + rho * cn) + v.gt) - ((v.g0 + v.q) + v.r)));
                      phiSum += (hasPhi ? v.gp * xn : 0.0) + 0.5 * xn * cn;      // getPhi of the new iterate, in its order of summation
                  }); }
    g_sync();
    const double statInf = g_max<G>(statMax);
    const double phiStep = phiConst + g_sum<G>(phiSum);      // (xk and C xk do not change again in this iterate: every getPhi below is this value)
    int totalIter = S.totalIter;
    if (db.traceCap > 0 && totalIter < db.traceCap) {   // storeSteps :488-490, printIteration :1528-1576 (the host rebuilds both from this)
        const double phiNow = phiStep;
        double so = 0.0, sm = 0.0, pm = 0.0;
        for (int i = t; i < n; i += G) { const double xv = xk[i]; so += g[i] * xv + 0.5 * xv * Qx[i]; sm += 0.5 * rho * xv * Cx[i]; pm = fmax(pm, fabs(pk[i])); }
        const double objNow = g_sum<G>(so), meritNow = objNow + g_sum<G>(sm), stepNow = g_max<G>(pm);
        double* ts = db.traceS + ((size_t)c.b * db.traceCap + totalIter) * 8;
        double* tx = db.traceX + ((size_t)c.b * db.traceCap + totalIter) * n;
        if (t == 0) {
            ts[0] = statInf; ts[1] = phiNow; ts[2] = rho; ts[3] = alphak; ts[4] = objNow; ts[5] = meritNow; ts[6] = stepNow; ts[7] = (double)S.qpIter;
            db.traceLen[c.b] = totalIter + 1;
        }
        for (int i = t; i < n; i += G) tx[i] = xk[i];
    }
    totalIter++; S.totalIter = totalIter; S.st.iterTotal++;
    bool leyffer = false;
    const int nd = o.nDynamicPenalty;
    if (nd > 0) {
        const double cur = phiStep;
        if (S.histLen < nd) { if (t == 0) hist[S.histLen] = cur; S.histLen++; g_sync(); }
        else {
            if (!(cur < o.complementarityTolerance)) {
                leyffer = true;
                for (int i = 0; i < nd; i++) if (cur < o.etaDynamicPenalty * hist[i]) { leyffer = false; break; }
            }
            g_sync();
            if (t == 0) { for (int i = 0; i + 1 < nd; i++) hist[i] = hist[i + 1]; hist[nd - 1] = cur; }
            g_sync();
        }
    }
    if (leyffer) { updatePenalty(); S.st.iterOuter++; }
    bool done = false;
    if (statInf < o.stationarityTolerance) {
        if (phiStep < o.complementarityTolerance) {
            sp_Ex<G>(c, xk, lx);
            int sflag = 1, mflag = 1, wflag = 0;
            const double ctol = o.complementarityTolerance;
            for (int i = 0; i < nK; i++) {
                const double Lx = lx[nC + i], Rx = lx[nC + nK + i];
                if (!(Lx <= ctol && Rx <= ctol)) continue;
                const double a = yk[nC + i], bq = yk[nC + nK + i];
                const double dualProd = a * bq, dualMin = fmin(a, bq);
                if (dualMin < 0) sflag = 0;
                if (fabs(dualProd) >= ctol && dualMin <= 0) { if (dualProd <= ctol) { wflag = 1; break; } mflag = 0; }
            }
            S.algoStat = wflag ? 1 : (sflag ? 4 : (mflag ? 3 : 2));
            g_sync();
            for (int i = t; i < nK; i += G) { const double Lx = lx[nC + i], Rx = lx[nC + nK + i]; yk[nC + i] -= rho * Rx; yk[nC + nK + i] -= rho * Lx; }
            g_sync();
            S.rc = 0;
            done = true;
        } else {
            updatePenalty(); S.st.iterOuter++;
        }
    }
    if (!done && totalIter > o.maxIterations) { S.rc = LCQP_MAX_ITERATIONS_REACHED; done = true; }
    if (!done && rho > o.maxPenaltyParameter) { S.rc = LCQP_MAX_PENALTY_REACHED; done = true; }
    S.rho = rho; S.alphak = alphak;
    if (done) return sp_finish<G>(c, S);
    // the next QP's linear term; its hot start needs r1 = r1_last + (g_last - g): the residual of the accepted trial is still in NV_R1
    { GD r1 = c.V(NV_R1);
      double gm = 0.0;
      g_map<G, 8>(n, t, [&](int i) { return D4{Cx[i], gtil[i], gk[i], r1[i]}; },
                  [&](int i, D4 v) { const double gn = rho * v.a + v.b; gk[i] = gn; r1[i] = v.d + (v.c - gn); gm = fmax(gm, fabs(gn)); });
      S.gmaxNext = g_max<G>(gm); }
    g_sync();
    SPROF(c, SP_LCQP);
    return sp_qp_begin<G>(c, S, gk);
}


template <int G>
__device__ __forceinline__ SpCtx<G> sp_ctx(const SpBatch& db, int b, int w0, int lane)
{
    SpCtx<G> c;
    c.db = &db; c.b = b; c.gl = lane & (G - 1); c.gi = (unsigned)(b - w0); c.w0 = w0;
    c.info = db.info + b;
    c.win = sp_dyn_lds + (size_t)(lane / G) * (G * G + 16 * G);
    c.cAdmm = c.cTrials = c.cFact = c.cCorr = c.cSweeps = 0;
    c.bytes = 0.0;
#ifdef LCQP_PROFILE
    for (int k = 0; k < SP_NPHASE; k++) c.prof[k] = 0;
    c.tprev = __builtin_amdgcn_s_memtime();
#endif
    return c;
}

// ---- setup: scales, rho vector, phi expressions, the ONE factorisation of the ADMM KKT matrix ----------------------------------
// The vector half of the setup, shared by k_sparse_setup and k_sparse_refresh: the ADMM weights of the rows from l and u (a free row
// 1e-6 rho, an equality rho rhoEqMult, anything else rho), g_phi and phi_const from lbL / lbR (src/LCQProblem.cpp:969-996).  Returns
// phi_const.  DETECT: `changed` says whether a weight of this lane's rows differs from the one in place, i.e. from the one inside the ADMM
// KKT factor.
template <int G, bool DETECT>
__device__ __forceinline__ double sp_prepare_vectors(SpCtx<G>& c, double scale, int& changed)
{
    const SpBatch& db = *c.db;
    const int t = c.gl, n = db.n, m = db.m, nC = db.nC, nK = db.nComp;
    const double rho = db.opt.admmRho * scale;
    GD l = c.M(MV_L), u = c.M(MV_U), rhov = c.M(MV_RHOV);
    changed = 0;
    for (int r = t; r < m; r += G) {
        double rv = rho;
        if (isinf(l[r]) && isinf(u[r])) rv = 1e-6 * rho;
        else if (l[r] == u[r]) rv = rho * db.opt.rhoEqMult;
        if (DETECT) changed |= (rhov[r] != rv);
        rhov[r] = rv;
    }
    // phi expressions (src/LCQProblem.cpp:969-996)
    double phiConst = 0.0;
    GD gphi = c.V(NV_GPHI);
    if (db.hasLbL || db.hasLbR) {
        GD lbL = c.arr(db.lbL, nK), lbR = c.arr(db.lbR, nK);
        double s = 0.0;
        for (int i = t; i < nK; i += G) s += lbL[i] * lbR[i];
        phiConst = g_sum<G>(s);
        GD coef = c.M(MV_LX);
        for (int r = t; r < m; r += G) coef[r] = (r >= nC + nK) ? lbL[r - nC - nK] : ((r >= nC) ? lbR[r - nC] : 0.0);     // R'lbL + L'lbR
        g_sync();
        sp_ETy<G>(c, coef, gphi, [](int) { return 0.0; }, [](double v) { return v; });
    } else {
        for (int i = t; i < n; i += G) gphi[i] = 0.0;
    }
    return phiConst;
}

// the ADMM KKT matrix [Q + sigma I, E'; E, -diag(1 / rhov)] factorised, with its border when the pattern has one
template <int G>
__device__ __forceinline__ void sp_admm_factor(SpCtx<G>& c, double scale)
{
    const SpBatch& db = *c.db;
    GD rhov = c.M(MV_RHOV);
    sp_factor_band<G>(c, c.KF(true), c.KD(true), db.opt.admmSigma * scale, [=](int r) { return 1.0 / rhov[r]; }, [](int) { return true; });
    if (db.kb > 0) {
        sp_border_prepare<G>(c, true, [](int) { return true; });
        for (int jb = 0; jb < db.kb; jb++) { GD vec = sp_border_column<G>(c, true, jb); sp_solve_band<G>(c, true, vec); }
        sp_border_schur<G>(c, true, db.opt.admmSigma * scale, [=](int r) { return 1.0 / rhov[r]; }, [](int) { return true; });
    }
}

template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_setup(SpBatch db)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl, n = db.n, m = db.m;
#ifdef LCQP_PROFILE
    if (t == 0) for (int k = 0; k < SP_NPHASE; k++) c.info->prof[k] = 0.0;
#endif
    double dmax = 0.0;
    for (int i = t; i < n; i += G)
        for (int k = db.Qp[i]; k < db.Qp[i + 1]; k++) if (db.Qi[k] == i) dmax = fmax(dmax, fabs(c.Qx()[k]));
    double scale = g_max<G>(dmax);
    if (!(scale > 1e-300)) scale = 1.0;
    int unused;
    const double phiConst = sp_prepare_vectors<G, false>(c, scale, unused);
    double e1 = 0.0;
    {
        GD Ev = c.Ex();
        for (int r = t; r < m; r += G) { double s1 = 0.0; for (int k = db.Ep[r]; k < db.Ep[r + 1]; k++) s1 += fabs(Ev[k]); e1 = fmax(e1, s1); }
        e1 = g_max<G>(e1);
    }
    if (t == 0) {
        c.info->e1max = e1;
        c.info->scale = scale; c.info->sigma = db.opt.admmSigma * scale; c.info->delta = db.opt.proxBig * scale; c.info->delta2 = 1e-9 / scale;
        c.info->phiConst = phiConst; c.info->haveSolution = 0; c.info->stfValid = 0; c.info->bytes = 0.0;
        c.info->deltaS = db.opt.proxSmall * scale; c.info->delta2S = 1e-14 / scale; c.info->bigReg = 0;
        c.info->warm = 0;
    }
    g_sync();
    if constexpr (G <= 16) {
        // the assembled band rows every factorisation of this instance streams (sp_factor_reg): the one gather from the values of Q and E
        GD K0 = c.K0(), Qv = c.Qx(), Ev = c.Ex();
        const int nnzQ = db.nnzQ;
#pragma unroll 2
        for (int r = t; r < db.N; r += G) {      // upper form: entry k of row r is K[r + k][r] (sp_factor_reg), the diagonal in entry 0
#pragma unroll
            for (int k = 1; k < G; k++) {
                const int code = db.bsrc[r * G + k];
                K0[r * G + k] = (code >= nnzQ) ? (double)Ev[code - nnzQ] : ((code >= 0) ? (double)Qv[code] : 0.0);
            }
            const int bd = db.bdiag[r];
            K0[r * G] = (bd >= 0) ? (double)Qv[bd] : 0.0;
        }
        g_sync();
    }
    sp_admm_factor<G>(c, scale);
    if (t == 0) c.info->bytes = c.bytes;
}

// ---- refresh: new vectors on the setup in place, and the hand-over between two runs (lcqp_hip_sparse_resolve) ----------------------------
// Stands where k_sparse_setup stands in a run.  The matrices, hence scale, sigma, the regularisations, e1max and K0, are the ones in memory;
// what depends on the bounds and on lbL / lbR is formed again exactly as the setup forms it.  The ADMM KKT factor contains 1 / rhov: it is
// rebuilt for an instance in which the class of a row changed (free, equality, other) and left in place otherwise -- the same weights give
// the same factor bit for bit.  (Lane groups of one wavefront may part here: the factorisation and the border routines keep everything
// per group -- collectives inside the group, the group's own piece of LDS, no workgroup barrier -- as k_sparse_sched relies on when a
// step holds fewer instances than the wavefront has groups.)
// mode 0: every instance starts cold, as the setup leaves it.  mode 1: an instance whose last run returned 0 starts warm (SpInfo::warm):
// at its last x and at rho0[b] (else its last rhoOpt), its first QP a hot start on the stored point, working set and polish factor.  The
// stored statuses are brought in line with the new bounds: equal bounds make an equality; an equality whose bounds differ, or a row held
// at a side that is infinite now, leaves with a zero multiplier (the trial's comparison of the factor's set with the working set then
// asks for a factorisation).
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_refresh(SpBatch db, int mode, const double* rho0)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl, m = db.m;
    const double scale = c.info->scale;
    const int warm = mode == 1 && c.info->haveSolution != 0 && db.stats[b].returnValue == 0;
    double rhoStart = db.opt.initialPenaltyParameter;
    if (warm) {
        const double last = db.stats[b].rhoOpt;
        rhoStart = rho0 ? rho0[b] : (last > 0.0 ? last : db.opt.initialPenaltyParameter);
    }
    int changed;
    const double phiConst = sp_prepare_vectors<G, true>(c, scale, changed);
    if (warm) {
        GD l = c.M(MV_L), u = c.M(MV_U), yq = c.M(MV_YQ);
        GI st = c.I(MI_ST);
        for (int r = t; r < m; r += G) {
            const double lo = l[r], hi = u[r];
            int s = st[r];
            if (lo == hi) s = ST_EQ;
            else if (s == ST_EQ || (s == ST_LOWER && isinf(lo)) || (s == ST_UPPER && isinf(hi))) s = ST_INACT;
            if (s == ST_INACT) yq[r] = 0.0;
            st[r] = s;
        }
    }
    if (t == 0) {
        c.info->phiConst = phiConst; c.info->bytes = 0.0;
        c.info->warm = warm; c.info->rho0 = rhoStart;
        if (!warm) { c.info->haveSolution = 0; c.info->stfValid = 0; c.info->bigReg = 0; }
    }
    g_sync();
    if (g_any<G>(changed)) sp_admm_factor<G>(c, scale);
    if (t == 0) c.info->bytes = c.bytes;
}

// ---- k_sparse_sensitivity: adjoint derivatives of the returned x in g and in the bounds of the stored working set (DESIGN.md 3a'') ----------
// At the point the last run returned, x is the minimiser of 1/2 x'Qx + g'x on E_W x = b_W, W the stored working set (MI_ST).  For an upstream
// gradient v:  K0 [d; lambda] = [v; 0],  K0 = [Q, E_W'; E_W, 0];  dl/dg = -d,  dl/db_W = lambda.  The polish factor in memory is the LDL' of
// [Q + delta I, E_W'; E_W, -delta2 I] for exactly this set: an instance leaves its last QP through a trial that changed nothing behind a
// correction whose factor matched MI_STT (sp_ph_trial / sp_ph_factor), sp_ph_qpend copies MI_STT to MI_ST, and nothing factorises after it.
// Which of the two regularisation levels it holds does not matter here: it only preconditions the refinement against the UNREGULARISED
// K0 -- residual [v - Q d - E_W'lambda; -E_W d] from the ELL products, correction through the same factor -- that runs until the residual
// is under its own rounding floor, 64 eps max_i(sum of |terms|_i), at most SENS_REFINE_MAX times (contraction delta |K0^-1| per step).
// G lanes per instance, as k_sparse_refresh; per instance a loop over the nrhs vectors.  The kernel READS the state of the instance; it
// writes its outputs and four buffers that every phase of a run overwrites before it reads them: the solve vector (SpBatch::Nv), NV_PK (d),
// NV_QP (Q d) and MV_LX (lambda).
//   v, dg [B][nrhs][n];  dbo [B][nrhs][m];  side [B][m]: 0 outside W, -1 at lower, +1 at upper, 2 equality;  sinfo [B]: flag bits
//   (include/lcqp_hip.h), 0 = differentiable.
constexpr int SENS_REFINE_MAX = 4;
template <int G>
__global__ __launch_bounds__(WGS) void k_sparse_sensitivity(SpBatch db, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo)
{
    const int b = blockIdx.x * (64 / G) + threadIdx.x / G;
    if (b >= db.B) return;
    SpCtx<G> c = sp_ctx<G>(db, b, blockIdx.x * (64 / G), (int)threadIdx.x);
    const int t = c.gl, n = db.n, m = db.m, nC = db.nC, nK = db.nComp;
    int* sd = side + (size_t)b * m;
    const int solved = c.info->haveSolution != 0 && db.stats[b].returnValue == 0;
    if (!solved) {      // (uniform inside the group) nothing to differentiate: zero outputs
        for (int r = t; r < m; r += G) sd[r] = 0;
        for (int k = 0; k < nrhs; k++) {
            double* og = dg + ((size_t)b * nrhs + k) * n;
            double* ob = dbo + ((size_t)b * nrhs + k) * m;
            for (int i = t; i < n; i += G) og[i] = 0.0;
            for (int r = t; r < m; r += G) ob[r] = 0.0;
        }
        if (t == 0) sinfo[b] = 1;
        return;
    }
    GI st = c.I(MI_ST);
    GD yq = c.M(MV_YQ);
    const int* iperm = db.iperm;
    // flags, as on the dense path (k_sensitivity): a row of L or R at its lower bound is a side of its pair; the active side of a pair that
    // is not biactive is an equality of the branch and needs no multiplier
    double ym = 0.0;
    for (int r = t; r < m; r += G) ym = fmax(ym, fabs(yq[r]));
    const double ytol = 1e-9 * (1.0 + g_max<G>(ym));
    auto sideIn = [&](int r) { const int s = st[r]; return s != ST_INACT && s != ST_UPPER; };
    int weak = 0, open = 0;
    for (int r = t; r < m; r += G) {
        const int s = st[r];
        sd[r] = (s == ST_INACT) ? 0 : ((s == ST_EQ) ? 2 : (s == ST_UPPER ? 1 : -1));
        if (s == ST_INACT) continue;
        bool ineq = s != ST_EQ;
        if (ineq && r >= nC && s != ST_UPPER) ineq = sideIn(r < nC + nK ? r + nK : r - nK);
        if (ineq && fabs(yq[r]) <= ytol) weak = 1;
    }
    for (int i = t; i < nK; i += G) if (!sideIn(nC + i) && !sideIn(nC + nK + i)) open = 1;
    weak = g_any<G>(weak) ? 1 : 0;
    open = g_any<G>(open) ? 1 : 0;
    GD d = c.V(NV_PK), qd = c.V(NV_QP), lam = c.M(MV_LX), bv = c.Nv();
    const double e1 = c.info->e1max;
    int stalled = 0;
    for (int k = 0; k < nrhs; k++) {
        const double* vk = v + ((size_t)b * nrhs + k) * n;
        double* og = dg + ((size_t)b * nrhs + k) * n;
        double* ob = dbo + ((size_t)b * nrhs + k) * m;
        g_map<G, 8>(n, t, [&](int i) { return ID{iperm[i], vk[i]}; }, [&](int i, ID w) { bv[w.i] = w.a; d[i] = 0.0; });
        g_map<G, 8>(m, t, [&](int r) { return iperm[n + r]; }, [&](int r, int p) { bv[p] = 0.0; lam[r] = 0.0; });
        g_sync();
        for (int it = 0;; it++) {
            sp_solve<G>(c, false, bv);
            double dm = 0.0;
            g_map<G, 8>(n, t, [&](int i) { return D2{bv[iperm[i]], d[i]}; }, [&](int i, D2 w) { const double dn = w.b + w.a; d[i] = dn; dm = fmax(dm, fabs(dn)); });
            g_map<G, 8>(m, t, [&](int r) { return ID2{st[r], bv[iperm[n + r]], lam[r]}; }, [&](int r, ID2 w) { lam[r] = (w.s != ST_INACT) ? w.y + w.v : 0.0; });
            g_sync();
            if (it == 0) {      // the answer of the regularised system: what stays when the refinement does not reach its floor
                g_map<G, 8>(n, t, [&](int i) { return (double)d[i]; }, [&](int i, double w) { og[i] = -w; });
                g_map<G, 8>(m, t, [&](int r) { return (double)lam[r]; }, [&](int r, double w) { ob[r] = w; });
            }
            // the residual against K0, straight into the solve vector: [v - Q d - E_W'lambda; -E_W d]
            SPROF(c, SP_VECTORS);
            sp_ell<G, false>(db.ellQ, c.gl, c.Qx(), [&](int j) { return D2{d[j], 0.0}; }, [](int) { return NoPre{}; }, [&](int i, double s, double, NoPre) { qd[i] = s; });
            g_sync();
            double mx = 0.0, sc = 0.0;
            sp_ell<G, true>(db.ellT, c.gl, c.Ex(), [&](int r) { return D2{(st[r] != ST_INACT) ? (double)lam[r] : 0.0, 0.0}; },
                            [&](int i) { return ID2{iperm[i], vk[i], qd[i]}; },
                            [&](int, double s, double, ID2 w) { const double rv = (w.v - w.y) - s; bv[w.s] = rv; mx = nmax(mx, fabs(rv)); sc = fmax(sc, fabs(w.v) + fabs(w.y) + fabs(s)); });
            sp_ell<G, false>(db.ellE, c.gl, c.Ex(), [&](int j) { return D2{d[j], 0.0}; }, [&](int r) { return I2{st[r], iperm[n + r]}; },
                             [&](int, double s, double, I2 w) { const double rv = (w.a != ST_INACT) ? -s : 0.0; bv[w.b] = rv; mx = nmax(mx, fabs(rv)); });
            g_sync();
            SPROF(c, SP_PRODUCTS);
            const double res = g_max<G>(mx), scale = fmax(g_max<G>(sc), e1 * g_max<G>(dm));
            const bool conv = res <= 64.0 * 2.221e-16 * scale;      // (a NaN does not pass)
            if (conv || it == SENS_REFINE_MAX) {
                if (!conv) stalled = 1;
                if (conv && it > 0) {
                    g_map<G, 8>(n, t, [&](int i) { return (double)d[i]; }, [&](int i, double w) { og[i] = -w; });
                    g_map<G, 8>(m, t, [&](int r) { return (double)lam[r]; }, [&](int r, double w) { ob[r] = w; });
                }
                break;
            }
        }
        g_sync();
    }
    if (t == 0) sinfo[b] = (stalled ? 2 : 0) | (weak ? 4 : 0) | (open ? 8 : 0);
}

// ---- the scheduler: persistent wavefronts that serve the phase queues of their pool -------------------------------------------------------
// Queue discipline (per pool and phase): push = take a position (atomicAdd on tail), wait until its slot's sequence says "free for this
// position" (at once, unless the ring has been lapped), store (position + 1, instance id) into it, atomicAdd on count; pop = claim entries of
// count (compare-and-swap), take as many positions (atomicAdd on head), wait for each slot's sequence to say "holds this position" (its pusher
// writes it a few instructions after taking the position), acquire fence, hand the slot on (store (position + poolSize, -)).  An instance is in at most one queue, so a ring of poolSize entries never overflows.
// Everything an instance's phase wrote to memory is released by the fence in front of its push and acquired by the fence behind the pop of
// whichever wavefront runs its next phase.
// agent scope: a pool is served by wavefronts of several XCDs, whose L2s are not coherent with each other -- the release writes the L2 back, the
// acquire invalidates L1 and L2 (workgroup-scope fences in their place: stale vectors, more iterates, 15 - 25 % SLOWER; profiles/round4)
#define SP_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#define SP_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent")
__device__ __forceinline__ int q_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long q_load64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void q_store64(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long q_slot(int seq, int id) { return ((unsigned long long)(unsigned)seq << 32) | (unsigned)id; }

// Lanes per instance depend on the phase (round 4, second step): the band phases (PH_FACTOR, PH_CORRECT, PH_ROUND with its ADMM band solves) need
// the G lanes the folded band layout is made for and take 64 / G instances per wavefront; the STREAMING phases (PH_START, PH_TRIAL, PH_QPEND:
// sparse products and element-wise loops, 60 % of the time) take ONE instance with all 64 lanes -- a wavefront instruction then reads 512
// contiguous bytes of one instance instead of eight 64-byte pieces of eight instances, the access pattern this part streams best
// (tools/micro/stream_pattern.py: 2.4 TB/s for eight far-apart pieces per wavefront, 5.8 TB/s for one stream).
constexpr int WIDE_BATCH_MAX = 16;      // instances of a streaming step at most (one per lane)
template <int G, int GP>
__device__ __forceinline__ int sp_run_phase(const SpBatch& db, int ph, int b, int w0, int lane)
{
    SpCtx<GP> c = sp_ctx<GP>(db, b, w0, lane);
    // INVARIANT (lock step): the record lives in global memory and EVERY lane of the instance's group reads and writes it -- the same
    // values, in the same instruction (S.trial++, S.round++, S.nrefine++ ...: a load and a store the group issues together).  That is
    // well defined only because (1) every branch that leads to an access of S is uniform inside the group (conditions are group
    // reductions or values read from S itself), (2) the group's lanes are lanes of ONE wavefront (G <= 64), so a load and the store
    // behind it are not separated by another lane's store, and (3) no other group touches this record while the instance is in a phase
    // (an instance is in at most one queue; the hand-over is ordered by the queue's fences).  A phase routine that accesses S under a
    // condition that differs between the lanes of a group breaks this.  (A private copy in registers, written back by lane 0, would
    // cost 50 VGPRs of the 249 the kernel has: the band factorisation's register window takes the rest.)
    SpState& S = db.state[b];
    c.cAdmm = S.cAdmm; c.cTrials = S.cTrials; c.cFact = S.cFact; c.cCorr = S.cCorr; c.cSweeps = S.cSweeps; c.bytes = S.bytes;
    GD gk = c.V(NV_GK);
    int next;
    if constexpr (GP == G) {
        // every phase can run with the band's lane group (the streaming ones do at G == 64)
        switch (ph) {
            case PH_START:   c.cAdmm = c.cTrials = c.cFact = c.cCorr = c.cSweeps = 0; c.bytes = 0.0; next = sp_ph_start<GP>(c, S); break;
            case PH_ROUND:   next = sp_ph_round<GP>(c, S, gk); break;
            case PH_TRIAL:   next = sp_ph_trial<GP>(c, S, gk); break;
            case PH_FACTOR:  next = sp_ph_factor<GP>(c, S); break;
            case PH_CORRECT: next = sp_ph_correct<GP>(c, S); break;
            default:         next = sp_ph_qpend<GP>(c, S); break;
        }
    } else {
        switch (ph) {
            case PH_START:   c.cAdmm = c.cTrials = c.cFact = c.cCorr = c.cSweeps = 0; c.bytes = 0.0; next = sp_ph_start<GP>(c, S); break;
            case PH_TRIAL:   next = sp_ph_trial<GP>(c, S, gk); break;
            default:         next = sp_ph_qpend<GP>(c, S); break;
        }
    }
    S.cAdmm = c.cAdmm; S.cTrials = c.cTrials; S.cFact = c.cFact; S.cCorr = c.cCorr; S.cSweeps = c.cSweeps; S.bytes = c.bytes;
#ifdef LCQP_PROFILE
    SPROF(c, SP_VECTORS);
    if (c.gl == 0) for (int k = 0; k < SP_NPHASE; k++) c.info->prof[k] += (double)c.prof[k];
#endif
    return next;
}

template <int G>
__global__ __launch_bounds__(WGS, (G <= 8 ? SCHED_WAVES_PER_SIMD : 1)) void k_sparse_sched(SpBatch db)
{
    constexpr int IPW = 64 / G;
    constexpr int GW = 64;      // lanes per instance of the streaming phases
    constexpr int IPWW = 64 / GW;
    __shared__ int s_id[WGS], s_next[WGS], s_ctl[2];      // the step's instances, where each goes next; [0] how many they are, [1] polls without work in a row
    // the pool's queues, derived afresh in front of the pop and in front of the push: nothing of the scheduler is alive across a phase
    struct Q { int w0, mask; unsigned long long* ring; int* ctl; int* remaining; };
    auto queues = [&]() {
        int pool = blockIdx.x % db.nPools;
        asm volatile("" : "+s"(pool));
        Q q;
        q.w0 = pool * db.poolSize; q.mask = db.poolSize - 1;
        q.ring = db.qring + (size_t)pool * PH_NUM * db.poolSize;
        q.ctl = db.qctl + (size_t)pool * (PH_NUM + 1) * QCTL;
        q.remaining = q.ctl + PH_NUM * QCTL;
        return q;
    };
    if (threadIdx.x == 0) s_ctl[1] = 0;
    for (;;) {
        const int lane = here((int)threadIdx.x);      // per step: nothing derived from the lane number is carried around the loop (it would be hoisted and spilled)
        const Q q0 = queues();
        const int w0 = q0.w0, mask = q0.mask;
        unsigned long long* ring = q0.ring;
        int* ctl = q0.ctl;
        int* remaining = q0.remaining;
        // ---- pop: one phase for the whole wavefront (lane 0 decides).  A band phase with a full wavefront's worth of instances first (the long
        // steps run at full width), else the fullest streaming queue, else whatever a band queue holds.
        int ph = -1, take = 0, base = 0;
        if (lane == 0) {
            int cnt[PH_NUM];
            for (int k = 0; k < PH_NUM; k++) cnt[k] = q_load(&ctl[k * QCTL + 2]);
            auto isWide = [](int k) { return GW != G && (k == PH_START || k == PH_TRIAL || k == PH_QPEND); };
            int best = 0;
            for (int k = 0; k < PH_NUM; k++) if (!isWide(k) && cnt[k] >= IPW && cnt[k] > best) { best = cnt[k]; ph = k; }
            if (ph < 0) for (int k = 0; k < PH_NUM; k++) if (isWide(k) && cnt[k] > best) { best = cnt[k]; ph = k; }
            if (ph < 0) for (int k = 0; k < PH_NUM; k++) if (cnt[k] > best) { best = cnt[k]; ph = k; }
            if (ph >= 0) {
                // instances of a streaming step: they run one after the other on this wavefront, so a long step makes the last of them wait
                // for the others while wavefronts elsewhere poll -- P = unfinished instances per SIMD of the machine up to 4, P / 2 beyond,
                // at most WIDE_BATCH_MAX (the fences of a step are paid once for all of them: full steps for batches that fill the
                // machine).  profiles/round5/sparse_wide_batch_rule.log: against 16 per step +20 % at B = 1024, +15 % at 2048, +11 % at
                // 4096, +7 % at 8192, the same from 16 384 on
                int wb = WIDE_BATCH_MAX;
                if (isWide(ph)) { const int P = q_load(remaining) / db.wideDiv; wb = max(1, min(WIDE_BATCH_MAX, P <= 4 ? P : max(4, P >> 1))); }
                take = min(best, isWide(ph) ? IPWW * wb : IPW);
                if (atomicCAS(&ctl[ph * QCTL + 2], best, best - take) == best) base = atomicAdd(&ctl[ph * QCTL + 1], take);
                else { ph = -1; take = 0; }      // somebody else moved the counter: look again
            }
        }
        ph = __builtin_amdgcn_readfirstlane(ph); take = __builtin_amdgcn_readfirstlane(take); base = __builtin_amdgcn_readfirstlane(base);
#ifdef LCQP_SCHED_PROFILE
        const unsigned long long tq0 = __builtin_amdgcn_s_memtime();
#endif
        if (take == 0) {
            if (q_load(remaining) <= 0) break;
            const int idle = s_ctl[1] + 1;
            if (lane == 0) s_ctl[1] = idle;
            // back off: a wavefront that finds nothing polls again later and later (each poll reads the pool's counters through the L2 all
            // wavefronts of the pool share; with s_sleep(32) per poll a quarter of idle wavefronts halved the rate of the working ones:
            // profiles/round5/sparse_waves.log) -- 2^min(idle, 7) / 8 sleeps of 127 x 64 clocks, at most ~ 60 us
            if (idle > 2) { const int reps = (1 << min(idle, 7)) >> 3; for (int k = 0; k < max(reps, 1); k++) __builtin_amdgcn_s_sleep(127); }
#ifdef LCQP_SCHED_PROFILE
            if (lane == 0) { atomicAdd(&db.qprof[PH_NUM * 3 + 0], __builtin_amdgcn_s_memtime() - tq0); atomicAdd(&db.qprof[PH_NUM * 3 + 1], 1ull); }
#endif
            continue;
        }
        if (lane == 0) { s_ctl[1] = 0; s_ctl[0] = take; }
        int myid = -1;
        const size_t qoff = (size_t)ph * db.poolSize;
        if (lane < take) {
            const int pos = base + lane;
            unsigned long long e;
            while ((int)((e = q_load64(&ring[qoff + (pos & mask)])) >> 32) != pos + 1) __builtin_amdgcn_s_sleep(1);
            myid = (int)(unsigned)e;
        }
        SP_ACQUIRE();                                                                    // (also orders the slot's read in front of handing it on)
        if (lane < take) {
            const int pos = base + lane;
            q_store64(&ring[qoff + (pos & mask)], q_slot(pos + db.poolSize, -1));
        }
        const bool wide = GW != G && (ph == PH_START || ph == PH_TRIAL || ph == PH_QPEND);
        // ---- run the phase for the instances popped (lane groups without one idle through it).  The instances of the step and where each goes
        // next are kept in LDS, one per lane: no register of the scheduler is alive across a phase.
        s_id[lane] = myid;
        __builtin_amdgcn_wave_barrier();
        if (wide) {
            // streaming phases: the instances popped (up to WIDE_BATCH_MAX) one after the other, GW lanes each, so that the fences of the step
            // -- the release writes back the whole XCD's L2 -- are paid once for all of them.  A streaming phase that leads to another one
            // (an accepted trial -> the end of its QP -> the first trial of the next) stays here: same lanes, same instance, its own stores in
            // program order -- no queue, no fences.
            for (int j = 0; j < take; j += IPWW) {
                const int ln = here(lane), bj = s_id[j + ln / GW];
                int nj = -1;
                if (bj >= 0)
                    for (int p = ph;; p = nj) {
                        nj = sp_run_phase<G, GW>(db, p, bj, w0, ln);
                        if (!(nj == PH_TRIAL || nj == PH_QPEND)) break;
                    }
                if ((ln & (GW - 1)) == 0) s_next[j + ln / GW] = nj;
            }
        } else {
            // band phases: 64 / G instances side by side, one such pass per step
            for (int j = 0; j < take; j += IPW) {
                const int l0 = here(lane), bj = s_id[j + l0 / G];
                int nj = -1;
                if (bj >= 0)
                    for (int p = ph;; p = nj) {      // (a factorisation is always followed by its correction: same lanes, same instances)
                        nj = sp_run_phase<G, G>(db, p, here(bj), w0, here(l0));      // (re-laundered per pass: nothing of the instance's addressing is carried around the loop)
                        if (!(p == PH_FACTOR && nj == PH_CORRECT)) break;
                    }
                if ((l0 & (G - 1)) == 0) s_next[j + l0 / G] = nj;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- push: what this wavefront wrote is released, then every instance goes to the queue of its next phase
        SP_RELEASE();
        if (here((int)threadIdx.x) < s_ctl[0]) {
            const Q q1 = queues();
            const int b = s_id[threadIdx.x], next = s_next[threadIdx.x];
            if (next == PH_NUM) atomicSub(q1.remaining, 1);
            else {
                const int pos = atomicAdd(&q1.ctl[next * QCTL + 0], 1), sl = pos & q1.mask;
                const size_t noff = (size_t)next * db.poolSize;
                while ((int)(q_load64(&q1.ring[noff + sl]) >> 32) != pos) __builtin_amdgcn_s_sleep(1);      // (waits only when the ring has been lapped onto a slot that is still being read)
                q_store64(&q1.ring[noff + sl], q_slot(pos + 1, b));
                atomicAdd(&q1.ctl[next * QCTL + 2], 1);
            }
        }
#ifdef LCQP_SCHED_PROFILE
        if (lane == 0) { atomicAdd(&db.qprof[ph * 3 + 0], __builtin_amdgcn_s_memtime() - tq0); atomicAdd(&db.qprof[ph * 3 + 1], 1ull); atomicAdd(&db.qprof[ph * 3 + 2], (unsigned long long)take); }
#endif
    }
}

// fills the queues of a run: every instance of every pool into PH_START
__global__ void k_sparse_sched_init(SpBatch db)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = db.nPools * (PH_NUM + 1) * QCTL;
    if (b < nq) {
        const int pool = b / ((PH_NUM + 1) * QCTL), k = (b / QCTL) % (PH_NUM + 1), f = b % QCTL;
        const int inPool = max(0, min(db.poolSize, db.B - pool * db.poolSize));
        int v = 0;
        if (k == PH_NUM) v = (f == 0) ? inPool : 0;                        // remaining
        else if (k == PH_START) v = (f == 0 || f == 2) ? inPool : 0;       // tail = count = instances of the pool, head = 0
        db.qctl[b] = v;
    }
    if (b < db.nPools * db.poolSize) {
        const int pool = b / db.poolSize, i = b % db.poolSize;
        for (int k = 0; k < PH_NUM; k++) {
            const bool filled = (k == PH_START && pool * db.poolSize + i < db.B);      // position i of the start queue holds instance i of the pool
            db.qring[((size_t)pool * PH_NUM + k) * db.poolSize + i] = filled ? q_slot(i + 1, pool * db.poolSize + i) : q_slot(i, -1);
        }
    }
}

// refresh: k_sparse_refresh<G>(mode, rho0) stands where k_sparse_setup<G> stands (lcqp_hip_sparse_resolve)
template <int G>
static void sp_launch(const SpBatch& db, hipStream_t stream, hipEvent_t mid, bool refresh, int mode, const double* rho0)
{
    const int ipw = 64 / G, grid = (db.B + ipw - 1) / ipw;
    // LDS: the working sets' bit sets of sp_ph_factor (G <= 16), the window of sp_factor_lds (per group G x G and 16 staged rows) otherwise
    const size_t ldsBytes = G <= 16 ? sizeof(unsigned) * (size_t)ipw * db.bitWords : sizeof(double) * (size_t)ipw * (G * G + 16 * G);
    if (refresh) hipLaunchKernelGGL(k_sparse_refresh<G>, dim3(grid), dim3(WGS), ldsBytes, stream, db, mode, rho0);
    else hipLaunchKernelGGL(k_sparse_setup<G>, dim3(grid), dim3(WGS), ldsBytes, stream, db);
    (void)hipEventRecord(mid, stream);
    const int ninit = std::max(db.nPools * db.poolSize, db.nPools * (PH_NUM + 1) * QCTL);
    hipLaunchKernelGGL(k_sparse_sched_init, dim3((ninit + 255) / 256), dim3(256), 0, stream, db);
    // persistent wavefronts: as many as the batch has work for, at most what the device holds at once (they leave when their pool is done);
    // a multiple of the number of pools so that every pool is served
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    // More wavefronts than one per 64 / G instances for batches that do not fill the machine (round 5, profiles/round5/sparse_waves_small_batches.log):
    // a streaming phase runs ONE instance on a wavefront's 64 lanes, so a wavefront that holds eight instances serialises their trial heads and
    // QP ends; with a wavefront per instance (up to 256) or per four instances B = 64 gains 52 %, 256: 44 %, 512: 39 %, 1024: 23 %, 2048: 12 %,
    // 8192: 4 % (4096: +-0); idle wavefronts back off exponentially, so the surplus costs nothing.
    int waves = std::max(grid, std::max(std::min(db.B, 256), db.B / 4));
    waves = std::min(waves, cus * 4 * (G <= 8 ? SCHED_WAVES_PER_SIMD : 1));      // resident at once (k_sparse_sched's launch bounds)
    waves = ((waves + db.nPools - 1) / db.nPools) * db.nPools;
    SpBatch dbs = db;
    dbs.wideDiv = std::max(1, cus * 4 / std::max(1, db.nPools));
    hipLaunchKernelGGL(k_sparse_sched<G>, dim3(waves), dim3(WGS), ldsBytes, stream, dbs);
}

// one launch of k_sparse_sensitivity<G> (DESIGN.md section 3a'') on device buffers
template <int G>
static void sp_launch_sensitivity(const SpBatch& db, hipStream_t stream, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo)
{
    const int ipw = 64 / G, grid = (db.B + ipw - 1) / ipw;
    const size_t ldsBytes = (G == 64 && db.general) ? sizeof(double) * (size_t)(G * G + 16 * G) : 0;      // the window of the general solve
    hipLaunchKernelGGL(k_sparse_sensitivity<G>, dim3(grid), dim3(WGS), ldsBytes, stream, db, nrhs, v, dg, dbo, side, sinfo);
}

}  // namespace

// the two launch functions of this unit's width (lcqp_sparse_launch.hpp)
namespace lcqp_sparse {
void LCQP_CAT(lcqp_sparse_launch_, LCQP_TU_G)(const SpBatch& db, hipStream_t stream, hipEvent_t mid, bool refresh, int mode, const double* rho0)
{ sp_launch<LCQP_TU_G>(db, stream, mid, refresh, mode, rho0); }
void LCQP_CAT(lcqp_sparse_sensitivity_, LCQP_TU_G)(const SpBatch& db, hipStream_t stream, int nrhs, const double* v, double* dg, double* dbo, int* side, int* sinfo)
{ sp_launch_sensitivity<LCQP_TU_G>(db, stream, nrhs, v, dg, dbo, side, sinfo); }
}
