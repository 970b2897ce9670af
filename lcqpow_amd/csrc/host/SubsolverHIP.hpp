// SubsolverHIP: the MI355X backend behind SubsolverBase.  Same constructor / copy / assignment /
// setOptions / solve / getSolution surface as SubsolverQPOASES (include/SubsolverQPOASES.hpp:36-110),
// implemented on the C ABI of include/lcqp_hip.h.
#ifndef LCQPOW_AMD_SUBSOLVERHIP_HPP
#define LCQPOW_AMD_SUBSOLVERHIP_HPP

#include "HipHandles.hpp"
#include "SubsolverBase.hpp"

namespace LCQPow {

class SubsolverHIP : public SubsolverBase {
  public:
    SubsolverHIP() = default;
    // nC = number of stacked rows nC + 2*nComp, Q (nV x nV) and A (nC x nV) row-major; deep copies
    SubsolverHIP(int nV, int nC, const double* Q, const double* A, int device = 0);
    // copies clone the QP object (the reference's surface, lcqp_hip_qp_clone); moves hand the one object on
    SubsolverHIP(const SubsolverHIP& rhs);
    SubsolverHIP& operator=(const SubsolverHIP& rhs);
    SubsolverHIP(SubsolverHIP&&) = default;
    SubsolverHIP& operator=(SubsolverHIP&&) = default;

    void setOptions(const lcqp_options_t& options);
    ReturnValue solve(bool initialSolve, int& iterations, int& exit_flag, const double* const g,
                      const double* const lbA, const double* const ubA, const double* const x0 = 0,
                      const double* const y0 = 0, const double* const lb = 0, const double* const ub = 0) override;
    void getSolution(double* x, double* y) override;
    // derivatives of the solution of the QP last solved (lcqp_hip_qp_sensitivity): v, dg [nrhs][nV]; db, side [.][nV + nC], info [1] may be 0
    ReturnValue getSensitivity(int nrhs, const double* v, double* dg, double* db = 0, int* side = 0, int* info = 0, bool blocked = false);
    // lcqp_hip_qp_jacobian: Jg [nV][nV], Jb [nV][nV + nC] (or 0), side [nV + nC], info [1]
    ReturnValue getJacobian(double* Jg, double* Jb = 0, int* side = 0, int* info = 0);
    // lcqp_hip_qp_adjoint: vx, dg [nV]; vy (or 0), db, side [nV + nC]; info [1]; dQ [nV][nV], dA [nC][nV] may be 0
    ReturnValue getAdjoint(const double* vx, const double* vy, double* dg, double* db = 0, int* side = 0, int* info = 0, double* dQ = 0, double* dA = 0);

  private:
    QpHandle qp;
};

}  // namespace LCQPow
#endif
