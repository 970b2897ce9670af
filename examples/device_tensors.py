"""A batch of LCQPs fed from torch tensors that live on the GPU (DESIGN.md section 3a'''''): load_device packs them into the solver's pools
with kernels, the solution and the gradients come back as tensors on the device, and the torch layer takes the same path by itself when
its inputs are on the device.  Nothing goes through the host but a status word.

    python examples/device_tensors.py"""
import os
import sys

import numpy as np
import torch      # before lcqpow_amd: the library and torch share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402
from lcqpow_amd.diff import BatchLCQPLayer  # noqa: E402

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
