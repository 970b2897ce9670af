// lcqp_hip_batch.hpp -- what the five host units of the dense arm share: the batch handle behind lcqp_hip_batch_t, the functions of
// lcqp_hip.hip (the batch's life cycle) and lcqp_hip_diff.hip (differentiation) that the QP object (lcqp_hip_qp.hip) and the building
// blocks (lcqp_hip_util.hip) call on it, what lcqp_hip_device.hip gives them, and the arm's error slot.  The
// host code the handle shares with the sparse arm's comes in with lcqp_host_rt.hpp and lcqp_sens_rt.hpp.
// Internal: nothing of it enters the dynamic symbol table of the library.  Host code only.
#pragma once
#include "lcqp_launch.hpp"
#include "lcqp_sens_rt.hpp"

#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

// the error slot of the dense arm (one thread_local string, defined in lcqp_hip.hip): what lcqp_hip_last_error returns for all five units
std::string& dense_err();

// The members are released in reverse order after the destructor's synchronisation: device memory, staging slots, events, streams.
struct lcqp_hip_batch {
    lcqp::DevBatch db;
    int device;
    // the setup has two independent branches (C = L'R + R'L and its compression; L1 -> Et -> M): the short one runs on `side`
    lcqp_rt::Stream stream, side;
    lcqp_rt::Event ev0, ev1, ev2;         // run: setup from ev0 to ev1, homotopy from ev1 to ev2
    lcqp_rt::Event evFork{hipEventDisableTiming}, evJoin{hipEventDisableTiming};
    lcqp_rt::UploadStage up;              // the staging of the host load / update (upload_packed); resolve sends rho0 through its first slot
    lcqp_rt::DevMem mem{stream};
    int numCU = 256;
    bool overlapped = false;      // lcqp_hip_batch_set_overlapped
    bool ran = false, anyLoaded = false;
    // re-solves (lcqp_host_rt.hpp) and sensitivities (lcqp_sens_rt.hpp).  boxed: which variables of an instance carry a finite box bound --
    // those are rows of E, hence of Et and M: an update must keep the set
    lcqp_rt::ResolveState rs;
    std::vector<char> boxed;              // [B][n]
    // a batch that holds one set of matrices (db.shared): which of Q, A, L, R are in place (bits as `shared` of the device loads), and
    // whether the set of box-bounded variables -- one for the batch, rows of the one E -- has been defined (it is boxed[] of every filled instance)
    int matsHeld = 0;
    bool boxDefined = false;
    std::vector<char> boxSet;             // [n]
    size_t bytesAll = 0, bytesOnce = 0;   // device memory lcqp_hip_batch_create(_shared) allocated, and the part of it held once for the batch
    lcqp_rt::SensState sn;                // sn.sens: of k_sensitivity
    lcqp_rt::SensBuffers sensBlk;         // of k_sensitivity_blk (another pitch of db, a varying number of instances)
    lcqp_rt::SensBuffers sensDual;        // of the dual Jacobian: capS staged rows per instance, no v, the row map behind `side`
    // of the device-pointer entry points (lcqp_hip_device.hip): the events of the hand-over between the caller's stream and `stream`; the
    // status words of k_check_vectors followed by the box flags of a load ([2] x 8 bytes, then [B][n] bytes)
    lcqp_rt::Event evIn{hipEventDisableTiming}, evOut{hipEventDisableTiming};
    unsigned long long* devChk = nullptr;
    int nch;
    const lcqp::SizeKernels* k = nullptr; // the launch table of the padded size (dense_kernels), set by lcqp_hip_batch_create
    explicit lcqp_hip_batch(int dev) : db(), device(dev) {}
    size_t ndual() const { return (size_t)db.nd; }      // the width of the dual vector (lcqp_sens_rt.hpp)
    ~lcqp_hip_batch() { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); }
};

// padded size of a problem with n variables in units of 128: 1, 2, 3, 4, then 8 (np = 1024), 16 (np = 2048) and 32 (np = 4096)
inline int padded_nch(int n) { const int k = (n + 127) / 128; return k > 16 ? 32 : (k > 8 ? 16 : (k > 4 ? 8 : k)); }

// lcqp_hip.hip; the comments are at the definitions
const lcqp::SizeKernels* dense_kernels(int nch);
const lcqp::RunKernels& run_kernels(const lcqp_hip_batch* h);
int launch_setup(lcqp_hip_batch* h, bool warm = false, const double* rho0 = nullptr);
// lcqp_hip_diff.hip: the bodies of the batch's sensitivity, Jacobian and adjoint entry points behind their guards, which the QP object
// calls on its batch of one (dev: the device-pointer twin, with the caller's stream)
int batch_sensitivity(lcqp_hip_batch* h, bool blk, int nrhs, const double* v, double* dg, double* db, int* side, int* info, bool dev = false, void* stream = nullptr);
int dense_jacobian(lcqp_hip_batch* h, int first, int count, double* Jg, double* Jb, int* side, int* info, bool dev);
int batch_adjoint(lcqp_hip_batch* h, const double* vx, const double* vy, double* dg, double* db, int* side, int* info,
                  int reduce, double* dQ, double* dA, double* dL, double* dR, bool dev = false, void* stream = nullptr);

// lcqp_hip_device.hip: k_pack_dual_rows on `count` instances -- staged row j of instance o (dg pitch np, db pitch ldb) goes to row
// rowpos[o][j] of Jyg [count][nd][n] and Jyb [count][nd][nd] (or null); rowpos < 0: the row is not part of the result
void launch_pack_dual_rows(const lcqp::DevBatch& d, hipStream_t s, int count, int ldb, const double* dg, const double* db, const int* rowpos,
                           double* Jyg, double* Jyb);

// lcqp_hip_device.hip: the pack step of a load / an update, the one definition of the pool layout.  Device pointers to the arrays as the caller
// holds them, of the `count` instances that go to [first, first + count):
// the vectors, [count][..] each, null = absent (the defaults of lcqp_hip_batch_load)
struct PackVectors { const double *g, *lbL, *ubL, *lbR, *ubR, *lbA, *ubA, *lb, *ub, *x0, *y0; };
// the matrices of a load: [count][rows][n], or [rows][n] with stride 0 (shared); null: the block of the pool stays
struct PackMatrices { const double* src[4]; size_t stride[4]; };      // Q, A, L, R
// k_pack_matrices and k_pack_vectors (update: k_pack_vectors alone, m is not read) on h->stream; nothing waits.  The checks and the host
// state are the caller's.
int dense_pack(lcqp_hip_batch* h, int first, int count, const PackVectors& v, const PackMatrices& m, bool update);
// lcqp_hip_batch_update_matrices and its device twin: the checks in front of every device call (the host state of a range that is about to
// be written is ResolveState::matrices_changed), and k_pack_matrices alone (boxRows: with the zero fill of the box rows of E, as a load)
int check_update_matrices(lcqp_hip_batch* h, int first, int count, const double* Q, const double* L, const double* R, const double* A);
int dense_pack_matrices(lcqp_hip_batch* h, int first, int count, const PackMatrices& m, bool boxRows);

// the message of lcqp_hip_batch_update and its device twin for a variable whose box bound appears or disappears
inline std::string box_change_message(int variable, int instance, bool gains)
{
    return "update: variable " + std::to_string(variable) + " of instance " + std::to_string(instance) + (gains ? " gains" : " loses") +
           " its box bound; the set of bounded variables is fixed by the load (they are rows of the factored matrices)";
}

// ---- a batch that holds one set of matrices (db.shared): the checks of its loads, host and device alike.  Nothing is written by them. ----
// the bits of the matrices a load brings, in the order of `shared` of the device loads: Q, A, L, R
inline int given_matrices(const double* Q, const double* A, const double* L, const double* R)
{
    return (Q ? 1 : 0) | (A ? 2 : 0) | (L ? 4 : 0) | (R ? 8 : 0);
}
// a matrix must be brought by the load or be in place: the missing-matrix codes of lcqp_hip_batch_load, in its order
inline int shared_matrices_present(const lcqp_hip_batch* h, int given)
{
    const int have = h->matsHeld | given;
    if (!(have & 1)) return LCQP_INVALID_ARGUMENT;
    if (!(have & 2) && h->db.nC > 0) return LCQP_INVALID_CONSTRAINT_MATRIX;
    if ((have & 12) != 12) return LCQP_INVALID_COMPLEMENTARITY_MATRIX;
    return 0;
}
// The set of box-bounded variables is one for the batch (they are rows of the one E).  flags [count][n]: the set of each instance of the
// load.  The load defines the set -- from its first instance -- when none is defined, or when it brings a matrix and no instance outside
// its range holds a problem; otherwise every instance must have the set in place.  set [n]: the set the load leaves (to be stored with
// boxDefined once the load goes ahead).  A difference: LCQP_INVALID_ARGUMENT and the lowest (instance, variable) in the message.
inline int shared_box_check(std::string& err, const lcqp_hip_batch* h, int first, int count, const char* flags, int given, std::vector<char>& set)
{
    const size_t n = (size_t)h->db.n;
    bool others = false;
    for (int b = 0; b < h->db.B; b++) others = others || (h->rs.filled[b] && (b < first || b >= first + count));
    const bool defines = !h->boxDefined || (given && !others);
    if (defines) set.assign(flags, flags + n); else set = h->boxSet;
    for (int k = 0; k < count; k++)
        for (size_t i = 0; i < n; i++)
            if ((flags[(size_t)k * n + i] != 0) != (set[i] != 0)) {
                err = "load: variable " + std::to_string(i) + " of instance " + std::to_string(first + k) + (flags[(size_t)k * n + i] ? " has" : " has not") +
                      " a box bound, against the set of the batch; a batch that holds one set of matrices has one set of bounded variables (they are rows of its E)";
                return LCQP_INVALID_ARGUMENT;
            }
    return 0;
}

// (device_pointer_ok, device_call and read_back, which the device-pointer entry points and the readers of the three units are built on, are
// templates in lcqp_host_rt.hpp: the sparse arm shares them)

#pragma GCC visibility pop
