"""Differentiable batched LCQP solves for torch: x*(g, lbA, ubA) with gradients from lcqp_hip_batch_sensitivity (DESIGN.md section 3a') or,
for a SparseBatchLCQP behind a SparseBatchLCQPLayer, lcqp_hip_sparse_sensitivity (section 3a'').

The solve and its derivative run on the HIP path of :mod:`lcqpow_amd.capi`; there is no CPU fallback -- without the built library, or
without a device, using the layer raises.  Tensors are copied to the host and back around the C ABI (host pointers): plumbing, not a
hot path.

    bt = BatchLCQP(B, nV, nC, nComp, opt=...); bt.load(0, B, Q, g0, L, R, A=A, lbA=lbA, ubA=ubA)
    layer = BatchLCQPLayer(bt, bounds=dict(lbA=lbA, ubA=ubA))
    x = layer(g)                      # [B][nV], on g's device; update + run the first time, update + resolve(warm) afterwards
    loss(x).backward()                # g.grad = dl/dg through the working set the solve ended on

The full adjoint (lcqp_hip_batch_adjoint, DESIGN.md section 3a'''') also returns the duals and differentiates in the matrices:

    x, y = layer.solve(g, Q=Q, A=A)   # Q [nV][nV] shared by the batch (or [B][nV][nV] per instance), likewise A, L, R
    loss(x, y).backward()             # g.grad, Q.grad, A.grad

and on the sparse arm (lcqp_hip_sparse_adjoint) in the value arrays of the shared pattern:

    layer = SparseBatchLCQPLayer(sb, bounds=..., values=dict(Qx=Qx0, Ax=Ax0))      # the values the batch was loaded with
    x, y = layer.solve(g, Qx=Qx, Ax=Ax)   # Qx [nnzQ] shared by the batch (or [B][nnzQ] per instance), likewise Ax over [A; L; R]
    loss(x, y).backward()                 # g.grad, Qx.grad, Ax.grad
"""
import warnings

import numpy as np
import torch

from . import capi

BOUND_KEYS = ("lbL", "ubL", "lbR", "ubR", "lbA", "ubA", "lb", "ub")


def _host(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().to(torch.float64).numpy())


class LCQPSolveFunction(torch.autograd.Function):
    """forward(layer, g, lbA, ubA) -> x: lcqp_hip_batch_update with the layer's other vectors, then run (first call) or resolve(warm).
    backward: one lcqp_hip_batch_sensitivity call; gradients for g and, where they were given as tensors, lbA and ubA.

    The derivative is the one of the equality-constrained QP on the working set the solve ended on.  Instances the library flags
    (info != 0: a failed solve -- zero gradient --, dropped dependent rows, a vanishing multiplier, an open complementarity pair) still get
    what the kernel computed, together with ONE warning per backward call that counts them; nothing is zeroed silently.
    A row with lbA == ubA has one derivative for both bounds: when both are tensor inputs each receives half of it, so that bounds tied
    to one parameter (the only move that keeps the row an equality) sum to the value; a single tensor input receives all of it."""

    @staticmethod
    def forward(ctx, layer, g, lbA=None, ubA=None):
        bt = layer.bt
        kw = dict(layer.bounds)
        if lbA is not None: kw["lbA"] = _host(lbA)
        if ubA is not None: kw["ubA"] = _host(ubA)
        rc = bt.update(0, bt.B, _host(g), **kw)
        if rc != 0:
            raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
        if layer.solves == 0:
            bt.run()
        else:
            bt.resolve(warm=layer.warm)
        x, y, st = bt.solution()
        layer.solves += 1
        layer.y, layer.stats = y, st
        layer._like = (g.dtype, g.device)
        ctx.layer, ctx.serial = layer, layer.solves
        ctx.given = (lbA is not None, ubA is not None)
        return torch.as_tensor(x, dtype=g.dtype, device=g.device)

    @staticmethod
    def backward(ctx, grad_x):
        layer = ctx.layer
        if ctx.serial != layer.solves:
            raise RuntimeError("backward through a solve that is not the layer's last one: the batch object holds the state of one solve")
        bt = layer.bt
        dg, db, side, info = bt.sensitivity(_host(grad_x))
        layer.info = info
        bad = int(np.count_nonzero(info))
        if bad:
            warnings.warn(f"LCQPSolveFunction.backward: {bad} of {bt.B} instances are not differentiable by the library's criteria "
                          f"(info bits present: {int(np.bitwise_or.reduce(info))}); their gradients are the kernel's output as it is",
                          RuntimeWarning, stacklevel=2)
        out = lambda a: torch.as_tensor(a, dtype=grad_x.dtype, device=grad_x.device)
        parts = capi.split_bound_derivatives(db, side, bt.nV, bt.nC, bt.nComp, sparse=layer.sparse)
        a0 = 0 if layer.sparse else bt.nV      # first row of A in the layout of side
        eq = side[:, a0:a0 + bt.nC] == 2
        share = np.where(eq, 0.5, 1.0) if all(ctx.given) else 1.0
        glb = out(parts["dlbA"] * share) if ctx.given[0] else None
        gub = out(parts["dubA"] * share) if ctx.given[1] else None
        return None, out(dg), glb, gub


MATRIX_KEYS = ("Q", "A", "L", "R")


class LCQPFullSolveFunction(torch.autograd.Function):
    """forward(layer, g, Q, A, L, R, lbA, ubA) -> (x, y).  Without matrix tensors: update + run / resolve(warm), as LCQPSolveFunction.  With
    one: lcqp_hip_batch_load of the whole batch + run; a tensor of shape [B][..][nV] holds one matrix per instance, one of shape [..][nV] is
    shared by the batch (broadcast at the load); a matrix that is not given is the one the batch holds.
    backward: lcqp_hip_batch_adjoint with the upstream gradients on x and on y -- gradients for g, for lbA / ubA where they were tensors (the
    rules of LCQPSolveFunction), and for the matrix tensors: per instance (reduce = 0) or, for a shared tensor, summed over the batch on the
    device (reduce = 1).  Flagged instances: the one warning of LCQPSolveFunction."""

    @staticmethod
    def forward(ctx, layer, g, Q=None, A=None, L=None, R=None, lbA=None, ubA=None):
        bt = layer.bt
        kw = dict(layer.bounds)
        if lbA is not None: kw["lbA"] = _host(lbA)
        if ubA is not None: kw["ubA"] = _host(ubA)
        given = dict(zip(MATRIX_KEYS, (Q, A, L, R)))
        rows = dict(Q=bt.nV, A=bt.nC, L=bt.nComp, R=bt.nComp)
        shared = {}
        for k, t in given.items():
            if t is None:
                continue
            if tuple(t.shape) not in ((bt.B, rows[k], bt.nV), (rows[k], bt.nV)):
                raise ValueError(f"{k}: expected [{bt.B}][{rows[k]}][{bt.nV}] or [{rows[k]}][{bt.nV}], got {tuple(t.shape)}")
            shared[k] = t.dim() == 2
        if shared:
            held = layer._matrices()
            for k, t in given.items():
                if t is not None:
                    held[k] = np.ascontiguousarray(np.broadcast_to(_host(t), (bt.B, rows[k], bt.nV)))
            rc = bt.load(0, bt.B, held["Q"], _host(g), held["L"], held["R"], A=held["A"], **kw)
            if rc != 0:
                raise RuntimeError(f"load failed with code {rc}: {bt._last_error()}")
            bt.run()
        else:
            rc = bt.update(0, bt.B, _host(g), **kw)
            if rc != 0:
                raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
            if layer.solves == 0:
                bt.run()
            else:
                bt.resolve(warm=layer.warm)
        x, y, st = bt.solution()
        layer.solves += 1
        layer.y, layer.stats = y, st
        layer._like = (g.dtype, g.device)
        ctx.layer, ctx.serial = layer, layer.solves
        ctx.given = (lbA is not None, ubA is not None)
        ctx.shared = shared
        out = lambda a: torch.as_tensor(a, dtype=g.dtype, device=g.device)
        return out(x), out(y)

    @staticmethod
    def backward(ctx, grad_x, grad_y):
        layer = ctx.layer
        if ctx.serial != layer.solves:
            raise RuntimeError("backward through a solve that is not the layer's last one: the batch object holds the state of one solve")
        bt = layer.bt
        vx, vy = _host(grad_x), _host(grad_y)
        each = tuple(k for k, sh in ctx.shared.items() if not sh)
        summed = tuple(k for k, sh in ctx.shared.items() if sh)
        r = bt.adjoint(vx, vy, matrices=each, reduce=False)
        mats = {k: r[k] for k in each}
        if summed:
            rs = bt.adjoint(vx, vy, matrices=summed, reduce=True)
            mats.update({k: rs[k] for k in summed})
        dg, db, side, info = r["dg"], r["db"], r["side"], r["info"]
        layer.info = info
        bad = int(np.count_nonzero(info))
        if bad:
            warnings.warn(f"LCQPFullSolveFunction.backward: {bad} of {bt.B} instances are not differentiable by the library's criteria "
                          f"(info bits present: {int(np.bitwise_or.reduce(info))}); their gradients are the kernel's output as it is",
                          RuntimeWarning, stacklevel=2)
        out = lambda a: torch.as_tensor(a, dtype=grad_x.dtype, device=grad_x.device)
        parts = capi.split_bound_derivatives(db, side, bt.nV, bt.nC, bt.nComp)
        eq = side[:, bt.nV:bt.nV + bt.nC] == 2
        share = np.where(eq, 0.5, 1.0) if all(ctx.given) else 1.0
        glb = out(parts["dlbA"] * share) if ctx.given[0] else None
        gub = out(parts["dubA"] * share) if ctx.given[1] else None
        gm = [out(mats[k]) if k in mats else None for k in MATRIX_KEYS]
        return (None, out(dg), *gm, glb, gub)


SPARSE_VALUE_KEYS = ("Qx", "Ax")


class LCQPSparseFullSolveFunction(torch.autograd.Function):
    """forward(layer, g, Qx, Ax, lbA, ubA) -> (x, y): LCQPFullSolveFunction over lcqp_hip_sparse_*.  Without value tensors: update + run /
    resolve(warm).  With one: lcqp_hip_sparse_load of the whole batch + run; a tensor [B][nnz] holds one value array per instance, one of
    shape [nnz] is shared by the batch (broadcast at the load); an array that is not given is the one the layer holds (its `values`).
    backward: lcqp_hip_sparse_adjoint with the upstream gradients on x and on y -- one call for the per-instance tensors (reduce = 0), one
    for the shared ones (reduce = 1, the sum over the batch formed on the device).  Flagged instances: the one warning of LCQPSolveFunction."""

    @staticmethod
    def forward(ctx, layer, g, Qx=None, Ax=None, lbA=None, ubA=None):
        bt = layer.bt
        kw = dict(layer.bounds)
        if lbA is not None: kw["lbA"] = _host(lbA)
        if ubA is not None: kw["ubA"] = _host(ubA)
        given = dict(zip(SPARSE_VALUE_KEYS, (Qx, Ax)))
        nnz = dict(Qx=bt.nnzQ, Ax=bt.nnzA)
        shared = {}
        for k, t in given.items():
            if t is None:
                continue
            if tuple(t.shape) not in ((bt.B, nnz[k]), (nnz[k],)):
                raise ValueError(f"{k}: expected [{bt.B}][{nnz[k]}] or [{nnz[k]}], got {tuple(t.shape)}")
            shared[k] = t.dim() == 1
        if shared:
            held = layer.values
            for k, t in given.items():
                if t is not None:
                    held[k] = np.ascontiguousarray(np.broadcast_to(_host(t), (bt.B, nnz[k])))
            rc = bt.load(0, bt.B, held["Qx"], _host(g), held["Ax"], **kw)
            if rc != 0:
                raise RuntimeError(f"load failed with code {rc}: {bt._last_error()}")
            bt.run()
        else:
            rc = bt.update(0, bt.B, _host(g), **kw)
            if rc != 0:
                raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
            if layer.solves == 0:
                bt.run()
            else:
                bt.resolve(warm=layer.warm)
        x, y, st = bt.solution()
        layer.solves += 1
        layer.y, layer.stats = y, st
        layer._like = (g.dtype, g.device)
        ctx.layer, ctx.serial = layer, layer.solves
        ctx.given = (lbA is not None, ubA is not None)
        ctx.shared = shared
        out = lambda a: torch.as_tensor(a, dtype=g.dtype, device=g.device)
        return out(x), out(y)

    @staticmethod
    def backward(ctx, grad_x, grad_y):
        layer = ctx.layer
        if ctx.serial != layer.solves:
            raise RuntimeError("backward through a solve that is not the layer's last one: the batch object holds the state of one solve")
        bt = layer.bt
        vx, vy = _host(grad_x), _host(grad_y)
        name = dict(Qx="Q", Ax="A")      # the names of SparseBatchLCQP.adjoint
        each = tuple(name[k] for k, sh in ctx.shared.items() if not sh)
        summed = tuple(name[k] for k, sh in ctx.shared.items() if sh)
        r = bt.adjoint(vx, vy, matrices=each, reduce=False)
        mats = {k: r[k] for k in each}
        if summed:
            rs = bt.adjoint(vx, vy, matrices=summed, reduce=True)
            mats.update({k: rs[k] for k in summed})
        dg, db, side, info = r["dg"], r["db"], r["side"], r["info"]
        layer.info = info
        bad = int(np.count_nonzero(info))
        if bad:
            warnings.warn(f"LCQPSparseFullSolveFunction.backward: {bad} of {bt.B} instances are not differentiable by the library's criteria "
                          f"(info bits present: {int(np.bitwise_or.reduce(info))}); their gradients are the kernel's output as it is",
                          RuntimeWarning, stacklevel=2)
        out = lambda a: torch.as_tensor(a, dtype=grad_x.dtype, device=grad_x.device)
        parts = capi.split_bound_derivatives(db, side, bt.nV, bt.nC, bt.nComp, sparse=True)
        eq = side[:, :bt.nC] == 2
        share = np.where(eq, 0.5, 1.0) if all(ctx.given) else 1.0
        glb = out(parts["dlbA"] * share) if ctx.given[0] else None
        gub = out(parts["dubA"] * share) if ctx.given[1] else None
        gm = [out(mats[name[k]]) if name[k] in mats else None for k in SPARSE_VALUE_KEYS]
        return (None, out(dg), *gm, glb, gub)


class BatchLCQPLayer:
    """A loaded BatchLCQP as a torch layer.  bounds: the bound vectors the batch was loaded with ([B][...] arrays under the names of
    BatchLCQP.update: lbL, ubL, lbR, ubR, lbA, ubA, lb, ub) -- an update replaces EVERY vector, so the ones that are not inputs of the
    layer are handed over again with every solve.  warm: re-solves start from the last solution where it exists."""

    sparse = False
    bound_keys = BOUND_KEYS

    def __init__(self, batch, bounds=None, warm=True):
        capi.lib()      # raises when the HIP library is not built: no CPU fallback
        unknown = set(bounds or ()) - set(self.bound_keys)
        if unknown:
            raise ValueError(f"bounds: unknown keys {sorted(unknown)}")
        self.bt, self.warm, self.solves = batch, warm, 0
        self.bounds = {k: capi._arr(v) for k, v in (bounds or {}).items() if v is not None}
        self.y = self.stats = self.info = None
        self._held = None

    def __call__(self, g, lbA=None, ubA=None):
        return LCQPSolveFunction.apply(self, g, lbA, ubA)

    def solve(self, g, Q=None, A=None, L=None, R=None, lbA=None, ubA=None):
        """(x, y) of the batch for the linear terms g, both differentiable (LCQPFullSolveFunction): y [B][nV + nC + 2 nComp] in
        the reference's dual layout.  Q, A, L, R: tensors that replace the matrices of the batch for this and later solves -- [B][..][nV]
        one per instance, [..][nV] one shared by all instances (its gradient is the sum over the batch).  Without any, the solve is the
        update + resolve of __call__."""
        return LCQPFullSolveFunction.apply(self, g, Q, A, L, R, lbA, ubA)

    def _matrices(self):
        """the matrices the batch holds, [B][..][nV] each: read back once, then kept in step with the loads of solve"""
        if self._held is None:
            ps = [self.bt.read_problem(b) for b in range(self.bt.B)]
            self._held = {k: np.stack([p[k] for p in ps]) for k in MATRIX_KEYS}
        return self._held

    def jacobian(self, serial=None):
        """dx/dg of the layer's last solve, [B][nV][nV] ([b][k][j] = dx_k/dg_j), a tensor of the dtype and on the device of that
        solve's g (BatchLCQP.jacobian: the blocked kernel on the unit vectors; dense arm).  serial: the value of layer.solves right
        after the solve that is meant -- like backward, the call raises when that is not the last one.  layer.info holds the flags."""
        if self.solves == 0 or (serial is not None and serial != self.solves):
            raise RuntimeError("jacobian of a solve that is not the layer's last one: the batch object holds the state of one solve")
        if self.sparse:
            raise RuntimeError("jacobian: only the dense arm has the blocked kernel")
        Jg, _, _, info = self.bt.jacobian(bounds=False)
        self.info = info
        return torch.as_tensor(Jg, dtype=self._like[0], device=self._like[1])


class SparseBatchLCQPLayer(BatchLCQPLayer):
    """A loaded SparseBatchLCQP as a torch layer: the same function over lcqp_hip_sparse_update / _run / _resolve / _sensitivity.  bounds:
    the vectors of SparseBatchLCQP.update the batch was loaded with (lbA, ubA, lbL, ubL, lbR, ubR; the sparse arm has no box)."""
    sparse = True
    bound_keys = tuple(k for k in BOUND_KEYS if k not in ("lb", "ub"))

    def __init__(self, batch, bounds=None, warm=True, values=None):
        """values: dict(Qx=[B][nnzQ], Ax=[B][nnzA]) (or [nnz], shared) -- the value arrays the batch was loaded with.  The sparse handle cannot
        read its matrices back, so a layer whose solve() takes Qx or Ax needs them, the way it needs `bounds`: a load replaces BOTH arrays, and
        the one that is not an input of the solve is handed over again.  The layer keeps them in step with its own loads."""
        super().__init__(batch, bounds=bounds, warm=warm)
        self.values = None
        if values is not None:
            if set(values) != set(SPARSE_VALUE_KEYS):
                raise ValueError(f"values: expected the keys {list(SPARSE_VALUE_KEYS)}, got {sorted(values)}")
            nnz = dict(Qx=batch.nnzQ, Ax=batch.nnzA)
            self.values = {}
            for k in SPARSE_VALUE_KEYS:
                v = capi._arr(values[k])
                if v.shape not in ((batch.B, nnz[k]), (nnz[k],)):
                    raise ValueError(f"values[{k!r}]: expected [{batch.B}][{nnz[k]}] or [{nnz[k]}], got {v.shape}")
                self.values[k] = np.ascontiguousarray(np.broadcast_to(v, (batch.B, nnz[k])))

    def solve(self, g, Qx=None, Ax=None, lbA=None, ubA=None):
        """(x, y) of the batch for the linear terms g, both differentiable (LCQPSparseFullSolveFunction): y [B][nC + 2 nComp], rows A, L, R.
        Qx, Ax: tensors that replace the value arrays of the batch for this and later solves, in the order of SparseBatchLCQP.load --
        [B][nnz] one per instance, [nnz] one shared by all instances (its gradient is the sum over the batch).  Qx.grad is the symmetric
        derivative on the full pattern.  Without any, the solve is the update + resolve of __call__."""
        if (Qx is not None or Ax is not None) and self.values is None:
            raise ValueError("solve: a layer that takes Qx or Ax needs the value arrays the batch holds -- construct it with "
                             "values=dict(Qx=..., Ax=...) (the sparse handle cannot read its matrices back)")
        return LCQPSparseFullSolveFunction.apply(self, g, Qx, Ax, lbA, ubA)
