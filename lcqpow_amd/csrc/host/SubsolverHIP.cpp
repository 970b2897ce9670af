#include "SubsolverHIP.hpp"

namespace LCQPow {

SubsolverHIP::SubsolverHIP(int nV, int nC, const double* Q, const double* A, int device) : qp(lcqp_hip_qp_create(nV, nC, Q, A, nullptr, device)) {}

SubsolverHIP::SubsolverHIP(const SubsolverHIP& rhs) : qp(rhs.qp ? lcqp_hip_qp_clone(rhs.qp.get()) : nullptr) {}

SubsolverHIP& SubsolverHIP::operator=(const SubsolverHIP& rhs)
{
    if (this != &rhs) {
        qp.reset();      // the old object goes before its successor is built
        qp.reset(rhs.qp ? lcqp_hip_qp_clone(rhs.qp.get()) : nullptr);
    }
    return *this;
}

void SubsolverHIP::setOptions(const lcqp_options_t& options)
{
    if (qp) lcqp_hip_qp_set_options(qp.get(), &options);
}

ReturnValue SubsolverHIP::solve(bool initialSolve, int& iterations, int& exit_flag, const double* const g,
                                const double* const lbA, const double* const ubA, const double* const x0,
                                const double* const y0, const double* const lb, const double* const ub)
{
    if (!qp) { iterations = 0; exit_flag = -1; return SUBPROBLEM_SOLVER_ERROR; }
    const int rc = lcqp_hip_qp_solve(qp.get(), initialSolve ? 1 : 0, &iterations, &exit_flag, g, lbA, ubA, x0, y0, lb, ub);
    return rc == LCQP_SUCCESSFUL_RETURN ? SUCCESSFUL_RETURN : SUBPROBLEM_SOLVER_ERROR;
}

void SubsolverHIP::getSolution(double* x, double* y)
{
    if (qp) lcqp_hip_qp_get_solution(qp.get(), x, y);
}

ReturnValue SubsolverHIP::getSensitivity(int nrhs, const double* v, double* dg, double* db, int* side, int* info, bool blocked)
{
    return (ReturnValue)(blocked ? lcqp_hip_qp_sensitivity_blocked(qp.get(), nrhs, v, dg, db, side, info) : lcqp_hip_qp_sensitivity(qp.get(), nrhs, v, dg, db, side, info));
}

ReturnValue SubsolverHIP::getJacobian(double* Jg, double* Jb, int* side, int* info)
{
    return (ReturnValue)lcqp_hip_qp_jacobian(qp.get(), Jg, Jb, side, info);
}

ReturnValue SubsolverHIP::getAdjoint(const double* vx, const double* vy, double* dg, double* db, int* side, int* info, double* dQ, double* dA)
{
    return (ReturnValue)lcqp_hip_qp_adjoint(qp.get(), vx, vy, dg, db, side, info, dQ, dA);
}

}  // namespace LCQPow
