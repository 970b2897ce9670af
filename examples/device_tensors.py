"""A batch of LCQPs fed from torch tensors that live on the GPU (DESIGN.md section 3a'''''): load_device packs them into the solver's pools
with kernels, the solution and the gradients come back as tensors on the device, and the torch layer takes the same path by itself when
its inputs are on the device.  Nothing goes through the host but a status word.

    python examples/device_tensors.py            the dense batch
    python examples/device_tensors.py sparse     the sparse batch: value arrays of one pattern, shared or per instance"""
import os
import sys

import numpy as np
import torch      # before lcqpow_amd: the library and torch share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402
from lcqpow_amd.diff import BatchLCQPLayer, SparseBatchLCQPLayer  # noqa: E402


def sparse():
    """the same on the sparse arm: the banded synthetic workload, one Hessian for the batch, one E = [A; L; R] per instance"""
    from lcqpow_amd import synth_sparse as S
    B, n, nC, nK = 8, 64, 32, 8
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
    Qpat, Epat, qo, eo = S.sparse_pattern_arrays(n, nC, nK)
    inst = [S.sparse_values(i, n, nC, nK, orders=(qo, eo)) for i in range(B)]
    stack = lambda k: np.stack([d[k] for d in inst])
    Qx = t(inst[0]["Qx"])                           # ONE value array [nnzQ] for the batch: broadcast by the pack kernel
    Ax = t(stack("Ex"))                             # [B][nnzA]: one per instance, in the CSC order of the pattern
    g, lbA, ubA = t(stack("g")), t(stack("lbA")), t(stack("ubA"))
    sb = la.SparseBatchLCQP(B, n, nC, nK, Qpat, Epat, opt=la.default_options(printLevel=0))
    assert sb.load_device(0, B, Qx, g, Ax, lbA=lbA, ubA=ubA) == 0, sb._last_error()
    sb.run()
    x, y = sb.solution_device()
    print("x on", x.device, " lanes per instance:", sb.lanes())
    layer = SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack("lbA"), ubA=stack("ubA")), values=dict(Qx=inst[0]["Qx"], Ax=stack("Ex")))
    g.requires_grad_(True); Qx.requires_grad_(True); Ax.requires_grad_(True)
    x, y = layer.solve(g, Qx=Qx, Ax=Ax)
    (x.square().sum() + y.sum()).backward()
    print("path:", layer.last_path, " |dl/dg| %.3e  |dl/dQx| %.3e  |dl/dAx| %.3e" % (g.grad.norm(), Qx.grad.norm(), Ax.grad.norm()), " on", Qx.grad.device)
    print("solved:", sum(s["returnValue"] == 0 for s in layer.stats), "of", B)
    # the whole solution map D(x, y) / D(g, b_W) of that solve: with g on the device the panel kernels' staging goes to six device tensors
    # through k_sparse_scatter_panels (jacobian_device + jacobian_duals_device)
    J = layer.jacobian_full()
    print("jacobian_full path:", layer.last_path, " on", J["xg"].device, " blocks:", {k: tuple(v.shape) for k, v in J.items()},
          " |dx/dg| %.3e  |dy/dg| %.3e" % (J["xg"].norm(), J["yg"].norm()))
    sb.close()


if len(sys.argv) > 1 and sys.argv[1] == "sparse":
    sparse()
    sys.exit(0)

B, n, nC, nK = 8, 40, 20, 8
rng = np.random.default_rng(0)
dev = torch.device("cuda", 0)
t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)

M = rng.uniform(-1, 1, (n, n))
Q = t(M.T @ M / n + np.eye(n))                      # ONE Hessian for the batch: broadcast by the pack kernel
L = torch.zeros((nK, n), dtype=torch.float64, device=dev); R = torch.zeros_like(L)
L[range(nK), range(nK)] = 1.0; R[range(nK), range(nK, 2 * nK)] = 1.0
A = t(rng.uniform(-1, 1, (B, nC, n)) / np.sqrt(n))  # one constraint matrix per instance
g = t(rng.uniform(-1, 1, (B, n)))
lbA, ubA = t(-np.ones((B, nC))), t(np.ones((B, nC)))

bt = la.BatchLCQP(B, n, nC, nK, opt=la.default_options(printLevel=0))
assert bt.load_device(0, B, Q, g, L, R, A=A, lbA=lbA, ubA=ubA) == 0, la.capi.last_error()
bt.run()
x, y = bt.solution_device()
print("x on", x.device, " complementarity max:", float(((L @ x.T) * (R @ x.T)).abs().max()))

# the layer: g, Q and A are leaves on the device; every gradient is produced there
layer = BatchLCQPLayer(bt, bounds=dict(lbA=lbA.cpu().numpy(), ubA=ubA.cpu().numpy()))
g.requires_grad_(True); Q.requires_grad_(True); A.requires_grad_(True)
x, y = layer.solve(g, Q=Q, A=A)
(x.square().sum() + y.sum()).backward()
print("path:", layer.last_path, " |dl/dg| %.3e  |dl/dQ| %.3e  |dl/dA| %.3e" % (g.grad.norm(), Q.grad.norm(), A.grad.norm()), " on", Q.grad.device)
print("solved:", sum(s["returnValue"] == 0 for s in layer.stats), "of", B)
bt.close()
