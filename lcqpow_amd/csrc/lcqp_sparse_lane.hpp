// lcqp_sparse_lane.hpp -- the lane-group model of the sparse arm: G lanes of a wavefront own one instance, 64 / G instances per wavefront.
// The sparse counterpart of lcqp_wg.hpp, first layer of the kernel unit (lcqp_sparse.hip has the map).
//
// Owns: the addressing of per-instance arrays (GRef / GP: uniform base + 32-bit lane offset), the context of an instance (SpCtx, sp_ctx) and
// the LDS a lane group owns, SPROF, `here`, the collectives inside a lane group (g_sum ... g_bcast, wave_sync, g_sync), the pipelined
// loops over a vector (g_map) and over the ELL slabs of a shared pattern (g_ell / sp_ell).  It knows the batch (SpBatch) only through
// SpCtx's accessors and the EllMat it is handed.
// May include: lcqp_wg.hpp (wave_bcast, opaque_u64, d4_t, the ST_* row states) and the seam lcqp_sparse_launch.hpp.  Device code only, all of
// it in the anonymous namespace of the translation unit.
#pragma once
#include "lcqp_wg.hpp"
#include "lcqp_sparse_launch.hpp"

#include <cmath>

using namespace lcqp;
using namespace lcqp_sparse;

namespace {

constexpr int WGS = 64;      // one wavefront per workgroup; 64 / G instances in it

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

// doubles of dynamic LDS a lane group owns (SpCtx::win): a G x G window and 16 staged rows.  The launches size the allocation with it.
constexpr int group_lds_doubles(int G) { return G * G + 16 * G; }

template <int G>
__device__ __forceinline__ SpCtx<G> sp_ctx(const SpBatch& db, int b, int w0, int lane)
{
    SpCtx<G> c;
    c.db = &db; c.b = b; c.gl = lane & (G - 1); c.gi = (unsigned)(b - w0); c.w0 = w0;
    c.info = db.info + b;
    c.win = sp_dyn_lds + (size_t)(lane / G) * group_lds_doubles(G);
    c.cAdmm = c.cTrials = c.cFact = c.cCorr = c.cSweeps = 0;
    c.bytes = 0.0;
#ifdef LCQP_PROFILE
    for (int k = 0; k < SP_NPHASE; k++) c.prof[k] = 0;
    c.tprev = __builtin_amdgcn_s_memtime();
#endif
    return c;
}

}  // namespace
