"""Fit the linear terms of 64 small LCQPs so that their solutions match targets: gradient steps through lcqpow_amd.diff.

Each step is one batched solve (update + warm re-solve after the first) and one lcqp_hip_batch_sensitivity call; the loss per step is
printed.  The targets are solutions of the same LCQPs for other linear terms, so a loss of zero is attainable.

    python examples/sensitivity.py
    python examples/sensitivity.py sparse      # the same fit on the sparse arm: 16 banded LCQPs (n = 64), lcqp_hip_sparse_sensitivity
    python examples/sensitivity.py jacobian    # the full Jacobians dx/dg of the 64 LCQPs (lcqp_hip_batch_jacobian): |Jg - Jg'| and the kernel time
    python examples/sensitivity.py duals       # the four blocks of D(x, y) / D(g, bounds) of one LCQP (lcqp_hip_batch_jacobian and _jacobian_duals)
    python examples/sensitivity.py sparse jacobian   # the full Jacobians of the 16 banded LCQPs (lcqp_hip_sparse_jacobian), panel kernel
    python examples/sensitivity.py sparse duals      # the four blocks of D(x, y) / D(g, bounds) of the 16 banded LCQPs (lcqp_hip_sparse_jacobian and _jacobian_duals)
    python examples/sensitivity.py adjoint     # learn ONE constraint matrix A shared by the 64 LCQPs from a loss on x and y (lcqp_hip_batch_adjoint)
    python examples/sensitivity.py sparse adjoint   # learn ONE value array of [A; L; R] shared by 16 banded LCQPs (lcqp_hip_sparse_adjoint)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402
from lcqpow_amd.diff import BatchLCQPLayer, SparseBatchLCQPLayer  # noqa: E402

B, n, nC, nComp = 64, 24, 12, 6


def problem(rng):
    M = rng.uniform(-1, 1, (n, n)); Q = M.T @ M / n + np.eye(n)
    L = np.zeros((nComp, n)); R = np.zeros((nComp, n))
    L[np.arange(nComp), np.arange(nComp)] = 1.0; R[np.arange(nComp), nComp + np.arange(nComp)] = 1.0
    xs = rng.uniform(0.2, 1, n); xs[nComp:2 * nComp] = 0.0
    A = rng.uniform(-1, 1, (nC, n)) / np.sqrt(n)
    return dict(Q=Q, L=L, R=R, A=A, lbA=A @ xs - rng.uniform(0.1, 1, nC), ubA=A @ xs + rng.uniform(0.1, 1, nC), g=rng.uniform(-1, 1, n))


def fit(layer, g0, rng, batch):
    with torch.no_grad():      # the targets: the solutions for a shifted linear term
        target = layer(torch.as_tensor(g0 + 0.3 * rng.standard_normal(g0.shape)))
    g = torch.tensor(g0, requires_grad=True)
    opt = torch.optim.SGD([g], lr=0.5)
    for step in range(12):
        opt.zero_grad()
        loss = 0.5 * ((layer(g) - target) ** 2).sum()      # a sum over independent instances: every instance takes its own step
        loss.backward()
        opt.step()
        print("step %2d  mean loss per LCQP %.6e  flagged instances %d" % (step, loss.item() / batch, int(np.count_nonzero(layer.info))))


def sparse_main(jacobian=False, duals=False):
    from lcqpow_amd import synth_sparse as S
    Bs, ns, nCs, nKs = 16, 64, 32, 8
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(ns, nCs, nKs)
    inst = [S.sparse_values(i, ns, nCs, nKs, orders=(qo, eo)) for i in range(Bs)]
    st = lambda k: np.stack([d[k] for d in inst])
    sb = la.SparseBatchLCQP(Bs, ns, nCs, nKs, Qpat, Apat, opt=la.default_options(perturbStep=0))
    assert sb.load(0, Bs, st("Qx"), st("g"), st("Ex"), lbA=st("lbA"), ubA=st("ubA")) == 0
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=st("lbA"), ubA=st("ubA")))
    if duals:
        with torch.no_grad():
            layer(torch.as_tensor(st("g")))
        J = layer.jacobian_full()      # the whole solution map D(x, y) / D(g, b_W): SparseBatchLCQP.jacobian and .jacobian_duals
        nW = np.count_nonzero(J["side"].numpy(), axis=1)
        print("xg %s xb %s yg %s yb %s; rows of W per instance %d to %d; max |xb - yg'| = %.3e, max |yb - yb'| = %.3e, kernel of the dual rows %.4f ms, "
              "flagged instances %d" % (tuple(J["xg"].shape), tuple(J["xb"].shape), tuple(J["yg"].shape), tuple(J["yb"].shape), nW.min(), nW.max(),
                                        (J["xb"] - J["yg"].transpose(1, 2)).abs().max().item(), (J["yb"] - J["yb"].transpose(1, 2)).abs().max().item(),
                                        sb.sensitivity_kernel_ms(), int(np.count_nonzero(layer.info))))
    elif jacobian:
        with torch.no_grad():
            layer(torch.as_tensor(st("g")))
        Jg = layer.jacobian()
        print("Jg %s (panels of %d columns): max |Jg - Jg'| = %.3e, kernel %.4f ms, flagged instances %d"
              % (tuple(Jg.shape), sb.sens_panel(), (Jg - Jg.transpose(1, 2)).abs().max().item(), sb.sensitivity_kernel_ms(), int(np.count_nonzero(layer.info))))
    else:
        fit(layer, st("g"), np.random.default_rng(0), Bs)
    sb.close()


def sparse_adjoint_main():
    """the OptNet setting on the sparse arm: the 16 LCQPs share the values of E = [A; L; R] on the pattern; targets (x, y) come from the true
    values, the fit starts from disturbed ones (the rows of A only: L and R stay the selectors they are)"""
    from lcqpow_amd import synth_sparse as S
    Bs, ns, nCs, nKs = 16, 64, 32, 8
    rng = np.random.default_rng(0)
    Qpat, Apat, qo, eo = S.sparse_pattern_arrays(ns, nCs, nKs)
    inst = [S.sparse_values(i, ns, nCs, nKs, orders=(qo, eo)) for i in range(Bs)]
    st = lambda k: np.stack([d[k] for d in inst])
    Ex_true = inst[0]["Ex"]
    in_A = np.asarray(Apat.indices) < nCs      # the entries of the stacked pattern that belong to rows of A
    sb = la.SparseBatchLCQP(Bs, ns, nCs, nKs, Qpat, Apat, opt=la.default_options(perturbStep=0))
    assert sb.load(0, Bs, st("Qx"), st("g"), np.stack([Ex_true] * Bs), lbA=st("lbA"), ubA=st("ubA")) == 0
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=st("lbA"), ubA=st("ubA")), values=dict(Qx=st("Qx"), Ax=Ex_true))
    g = torch.as_tensor(st("g"))
    with torch.no_grad():
        xt, yt = layer.solve(g, Ax=torch.as_tensor(Ex_true))
    Ax = torch.tensor(Ex_true + 0.02 * in_A * rng.standard_normal(Ex_true.shape), requires_grad=True)
    opt = torch.optim.SGD([Ax], lr=0.02)
    for step in range(12):
        opt.zero_grad()
        x, y = layer.solve(g, Ax=Ax)      # a shared [nnzA] tensor: load + run; Ax.grad is summed over the batch on the device
        loss = 0.5 * ((x - xt) ** 2).sum() + 0.5 * ((y - yt) ** 2).sum()
        loss.backward()
        Ax.grad *= torch.as_tensor(in_A, dtype=Ax.dtype)
        opt.step()
        print("step %2d  mean loss per LCQP %.6e  |Ax - Ax_true|_max %.3e  flagged instances %d"
              % (step, loss.item() / Bs, float(np.abs(Ax.detach().numpy() - Ex_true).max()), int(np.count_nonzero(layer.info))))
    sb.close()


def adjoint_main():
    """the OptNet setting: the 64 LCQPs share Q and A; targets (x, y) come from the true A, the fit starts from a disturbed one"""
    rng = np.random.default_rng(0)
    ds = [problem(rng) for _ in range(B)]
    st = lambda k: np.stack([d[k] for d in ds])
    Q, A_true = ds[0]["Q"], ds[0]["A"]
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options(perturbStep=0))
    assert bt.load(0, B, np.stack([Q] * B), st("g"), st("L"), st("R"), A=np.stack([A_true] * B), lbA=st("lbA"), ubA=st("ubA")) == 0
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=st("lbA"), ubA=st("ubA")))
    g = torch.as_tensor(st("g"))
    with torch.no_grad():
        xt, yt = layer.solve(g, A=torch.as_tensor(A_true))
    A = torch.tensor(A_true + 0.05 * rng.standard_normal(A_true.shape) / np.sqrt(n), requires_grad=True)
    opt = torch.optim.SGD([A], lr=0.02)
    for step in range(12):
        opt.zero_grad()
        x, y = layer.solve(g, A=A)      # a shared [nC][nV] tensor: load + run; A.grad is summed over the batch on the device
        loss = 0.5 * ((x - xt) ** 2).sum() + 0.5 * ((y - yt) ** 2).sum()
        loss.backward()
        opt.step()
        print("step %2d  mean loss per LCQP %.6e  |A - A_true|_max %.3e  flagged instances %d"
              % (step, loss.item() / B, float(np.abs(A.detach().numpy() - A_true).max()), int(np.count_nonzero(layer.info))))
    bt.close()


def main():
    if la.device_count() < 1:
        raise SystemExit("needs a GPU (the product path has no CPU fallback)")
    if sys.argv[1:] == ["sparse"]:
        return sparse_main()
    if sys.argv[1:] == ["sparse", "jacobian"]:
        return sparse_main(jacobian=True)
    if sys.argv[1:] == ["sparse", "duals"]:
        return sparse_main(duals=True)
    if sys.argv[1:] == ["sparse", "adjoint"]:
        return sparse_adjoint_main()
    if sys.argv[1:] == ["adjoint"]:
        return adjoint_main()
    rng = np.random.default_rng(0)
    ds = [problem(rng) for _ in range(B)]
    st = lambda k: np.stack([d[k] for d in ds])
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options(perturbStep=0))
    assert bt.load(0, B, st("Q"), st("g"), st("L"), st("R"), A=st("A"), lbA=st("lbA"), ubA=st("ubA")) == 0
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=st("lbA"), ubA=st("ubA")))
    if sys.argv[1:] == ["jacobian"]:
        with torch.no_grad():
            layer(torch.as_tensor(st("g")))
        Jg = layer.jacobian()
        print("Jg %s: max |Jg - Jg'| = %.3e, kernel %.4f ms, flagged instances %d"
              % (tuple(Jg.shape), (Jg - Jg.transpose(1, 2)).abs().max().item(), bt.sensitivity_kernel_ms(), int(np.count_nonzero(layer.info))))
    elif sys.argv[1:] == ["duals"]:
        with torch.no_grad():
            layer.solve(torch.as_tensor(st("g")))
        J = layer.jacobian(duals=True)      # the whole solution map D(x, y) / D(g, b_W): BatchLCQP.jacobian and .jacobian_duals
        W = torch.flatnonzero(J["side"][0])
        print("instance 0: %d rows in the working set, dual positions %s" % (len(W), W.tolist()))
        torch.set_printoptions(precision=4, linewidth=160)
        print("dx/dg  %s, first 4 x 4:\n%s" % (tuple(J["xg"].shape), J["xg"][0, :4, :4]))
        print("dx/db  %s, x rows 0 .. 3, columns of W:\n%s" % (tuple(J["xb"].shape), J["xb"][0, :4][:, W]))
        print("dy/dg  %s, rows of W, g columns 0 .. 3:\n%s" % (tuple(J["yg"].shape), J["yg"][0, W][:, :4]))
        print("dy/db  %s, W x W:\n%s" % (tuple(J["yb"].shape), J["yb"][0, W][:, W]))
        print("max |dy/dg - (dx/db)'| = %.3e, max |dy/db - (dy/db)'| = %.3e, flagged instances %d"
              % ((J["yg"] - J["xb"].transpose(1, 2)).abs().max().item(), (J["yb"] - J["yb"].transpose(1, 2)).abs().max().item(),
                 int(np.count_nonzero(layer.info))))
    else:
        fit(layer, st("g"), rng, B)
    bt.close()


if __name__ == "__main__":
    main()
