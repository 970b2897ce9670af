// lcqp_sparse_batch.hpp -- what the three host units of the sparse arm share: the handle behind lcqp_hip_sparse_t, the functions of
// lcqp_sparse_host.hip (the life cycle) that the differentiation unit (lcqp_sparse_diff.hip) and the device-pointer unit
// (lcqp_sparse_device.hip) call on it, what the latter gives the other two, and the arm's error slot.  The host code the handle
// shares with the dense arm's comes in with lcqp_host_rt.hpp and lcqp_sens_rt.hpp.  Internal: nothing of it enters the dynamic symbol table
// of the library.  Host code only.
#pragma once
#include "lcqp_sparse_launch.hpp"
#include "lcqp_sens_rt.hpp"

#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

// the error slot of the sparse arm (one thread_local string, defined in lcqp_sparse_host.hip): what lcqp_hip_sparse_last_error returns
std::string& sparse_err();

// The members are released in reverse order after the destructor's synchronisation: device memory, events, stream.
struct lcqp_hip_sparse {
    lcqp_sparse::SpBatch db;
    int device;
    int cus = 0;                   // compute units of `device` (create): bounds the persistent wavefronts of a run
    lcqp_rt::Stream stream;
    lcqp_rt::Event ev0, ev1, ev2;           // run: setup from ev0 to ev1, homotopy from ev1 to ev2
    lcqp_rt::UploadStage up;                // the staging of the host load / update (upload_packed)
    lcqp_rt::DevMem mem{stream};            // zero-fills on the handle's stream
    std::vector<int> csr2csc;      // value order: E (CSR) entry k comes from entry csr2csc[k] of the caller's CSC arrays
    // the two orderings of the band (lcqp_sparse_pattern.hpp: Pattern::ord): device copies of their maps, the permutation for get_ordering
    struct Ord { std::vector<int> perm; int *iperm, *bandQ, *bandE, *bsrc, *bgate, *bdiag, *pnode, *Upos; bool rowsFollow; } ord[2] = {};
    bool hasB = false;
    int generalOrdering = 0;       // lcqp_hip_sparse_general_ordering: 0 a band engine, 1 nested dissection, 2 minimum degree
    int useB = 0;                  // ordering of the last sp_choose_ordering
    std::vector<int> qdiagHost;    // entry of Q_ii in the value array
    std::vector<double> diagRatio; // per instance: min_i Q_ii / max_i Q_ii of the loaded Hessian (1: not loaded yet)
    bool loaded = false, ran = false;
    bool generalPanel = false;     // lcqp_hip_sparse_set_general_panel: many-vector derivatives of the general LDL' through its panel kernel
    // re-solves (lcqp_host_rt.hpp) and sensitivities (lcqp_sens_rt.hpp).  This arm has no setup without a solve: setupValid and solved go
    // together; rhoStart is allocated by the first resolve that carries penalties
    lcqp_rt::ResolveState rs;
    lcqp_rt::SensState sn;
    // the device copy of csr2csc (one per pattern, uploaded by sp_value_map for the first call that needs it): the adjoint stores dAx through
    // it, k_sparse_pack_values of a device load gathers Ax through it
    int* valMap = nullptr;
    // of the device-pointer entry points (lcqp_sparse_device.hip; the twins of the differentiation calls in lcqp_sparse_diff.hip): the events of
    // the hand-over between the caller's stream and `stream`; the status word of k_sparse_check_vectors followed by the diagonal pairs of a
    // load ([2] x 8 bytes, then [B][2] doubles)
    lcqp_rt::Event evIn{hipEventDisableTiming}, evOut{hipEventDisableTiming};
    unsigned long long* devChk = nullptr;
    explicit lcqp_hip_sparse(int dev) : db(), device(dev) {}
    size_t ndual() const { return (size_t)db.m; }      // the width of the dual vector (lcqp_sens_rt.hpp)
    ~lcqp_hip_sparse() { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); }
};

// lcqp_sparse_host.hip; the comments are at the definitions
void sp_choose_ordering(lcqp_hip_sparse* h);
int sp_value_map(lcqp_hip_sparse* h);
const lcqp_sparse::SpKernels* sp_kernels(int G);

// lcqp_sparse_device.hip: the pack step of a load / an update, the one definition of the pool layout.  Device pointers to the arrays as the
// caller holds them, of the `count` instances that go to [first, first + count):
// the vectors, [count][..] each, null = absent (the defaults of lcqp_hip_sparse_load)
struct SpPackVectors { const double *g, *lbA, *ubA, *lbL, *ubL, *lbR, *ubR, *x0, *y0; };
// the value arrays of a load: [count][nnz], or [nnz] with stride 0 (shared); null: the values of the pool stay
struct SpPackValues { const double *Qx, *Ax; size_t qStride, aStride; };
// k_sparse_pack_values (Ax needs sp_value_map first) and k_sparse_pack_vectors (update: k_sparse_pack_vectors alone, m is not read) on
// h->stream; nothing waits.  The checks and the host state are the caller's.
int sparse_pack(lcqp_hip_sparse* h, int first, int count, const SpPackVectors& v, const SpPackValues& m, bool update);
// lcqp_hip_sparse_update_values and its device twin: the checks in front of every device call (lcqp_sparse_host.hip; the host state of a
// range that is about to be written is ResolveState::matrices_changed), and k_sparse_pack_values alone
int check_update_values(lcqp_hip_sparse* h, int first, int count, const double* Qx, const double* Ax);
int sparse_pack_values(lcqp_hip_sparse* h, int first, int count, const SpPackValues& m);

// ---- from the staging of the panel kernels (lcqp_sparse_launch.hpp: SpSensBlkArgs) to the caller's arrays.  The one definition of where a
// staged column goes: the host loop of sp_panel_run (lcqp_sparse_diff.hip) and k_sparse_scatter_panels (lcqp_sparse_device.hip) both call it.
// Staged column k of work item `item` = (instance - first) * npan + panel of a call with ncols columns per instance in panels of P: the row
// of the caller's [count][ncols][..] arrays it is, or -1: nowhere.  Plain calls: column panel * P + k of its instance; the padding columns
// of a ragged last panel go nowhere.  dunit (the dual Jacobian, ncols = m): row rowpos -- what the kernel wrote for this column -- of its
// instance, nowhere when that is no row (-1: a column past |W|).
__host__ __device__ inline long long sp_panel_dest_row(unsigned item, unsigned k, unsigned npan, unsigned P, unsigned ncols, int dunit, int rowpos)
{
    const unsigned ir = item / npan;
    if (dunit) return (rowpos < 0 || (unsigned)rowpos >= ncols) ? -1 : (long long)ir * ncols + rowpos;
    const unsigned c = (item % npan) * P + k;
    return c >= ncols ? -1 : (long long)ir * ncols + c;
}
// one chunk of a call: the work items [item0, item0 + nItems), staged at sg [nItems][P][n] and sb [nItems][P][m] with rowpos [nItems][P]
// (dunit), to dg [count][ncols][n] and db [count][ncols][m] (null: not asked for) on the device
struct SpScatterArgs {
    int npan, ncols, dunit, P, n, m, item0, nItems;
    const double *sg, *sb;
    const int* rowpos;
    double *dg, *db;
};
// k_sparse_scatter_panels on h->stream; nothing waits
int sparse_scatter_panels(lcqp_hip_sparse* h, const SpScatterArgs& a);

#pragma GCC visibility pop
