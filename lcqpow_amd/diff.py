"""Differentiable batched LCQP solves for torch: x*(g, lbA, ubA) with gradients from lcqp_hip_batch_sensitivity (DESIGN.md section 3a') or,
for a SparseBatchLCQP behind a SparseBatchLCQPLayer, lcqp_hip_sparse_sensitivity (section 3a'').

The solve and its derivative run on the HIP path of :mod:`lcqpow_amd.capi`; there is no CPU fallback -- without the built library, or
without a device, using the layer raises.  Both layers have two paths, chosen per call by where g lives (layer.last_path):
"device" when g is a tensor on the batch's GPU -- the device-pointer entry points (DESIGN.md section 3a'''''): tensors are packed into the
pools by kernels, x, y and every gradient are produced on the device, and nothing goes through the host but a status word and the count
of flagged instances -- and "host" otherwise: tensors are copied to the host and back around the host-pointer C ABI, exactly as a CPU
tensor always was.  Both paths return the same bits.

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


def _dev(t, device):
    """a tensor argument as the device-pointer entry points take it: float64, contiguous, on `device`, detached"""
    return None if t is None else t.detach().to(device=device, dtype=torch.float64).contiguous()


def _warn_flagged(who, info, B):
    """the one warning of a backward call on the device path: the count is the one scalar read of that call"""
    bad = int(torch.count_nonzero(info))
    if bad:
        bits = int(np.bitwise_or.reduce(info.cpu().numpy()))
        warnings.warn(f"{who}.backward: {bad} of {B} instances are not differentiable by the library's criteria "
                      f"(info bits present: {bits}); their gradients are the kernel's output as it is", RuntimeWarning, stacklevel=3)


def _bound_grads_device(bt, db, side, given, like, sparse=False):
    """the gradients of lbA / ubA on the device path: split_bound_derivatives and the equality rule of LCQPSolveFunction, on tensors"""
    parts = capi.split_bound_derivatives_torch(db, side, bt.nV, bt.nC, bt.nComp, sparse=sparse)
    a0 = 0 if sparse else bt.nV      # first row of A in the layout of side
    eq = side[:, a0:a0 + bt.nC] == 2
    one = db.new_ones(())
    share = torch.where(eq, 0.5 * one, one) if all(given) else one
    glb = (parts["dlbA"] * share).to(like) if given[0] else None
    gub = (parts["dubA"] * share).to(like) if given[1] else None
    return glb, gub


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
        ctx.device_path = layer._on_device(g)
        layer.last_path = "device" if ctx.device_path else "host"
        if ctx.device_path:
            kw = dict(layer._device_bounds(g.device))
            if lbA is not None: kw["lbA"] = _dev(lbA, g.device)
            if ubA is not None: kw["ubA"] = _dev(ubA, g.device)
            rc = bt.update_device(0, bt.B, _dev(g, g.device), **kw)
            if rc != 0:
                raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
            if layer.solves == 0:
                bt.run()
            else:
                bt.resolve(warm=layer.warm)
            x, y = bt.solution_device()
            layer.solves += 1
            layer.y, layer.stats = y, None      # (the statistics: through the host call, when layer.stats is read)
            layer._like = (g.dtype, g.device)
            ctx.layer, ctx.serial = layer, layer.solves
            ctx.given = (lbA is not None, ubA is not None)
            return x.to(g.dtype)
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
        if ctx.device_path:
            dg, db, side, info = bt.sensitivity_device(_dev(grad_x, grad_x.device))
            layer.info = info
            _warn_flagged("LCQPSolveFunction", info, bt.B)
            glb, gub = _bound_grads_device(bt, db, side, ctx.given, grad_x.dtype, sparse=layer.sparse)
            return None, dg.to(grad_x.dtype), glb, gub
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
        given = dict(zip(MATRIX_KEYS, (Q, A, L, R)))
        rows = dict(Q=bt.nV, A=bt.nC, L=bt.nComp, R=bt.nComp)
        shared = {}
        for k, t in given.items():
            if t is None:
                continue
            if tuple(t.shape) not in ((bt.B, rows[k], bt.nV), (rows[k], bt.nV)):
                raise ValueError(f"{k}: expected [{bt.B}][{rows[k]}][{bt.nV}] or [{rows[k]}][{bt.nV}], got {tuple(t.shape)}")
            shared[k] = t.dim() == 2
        ctx.device_path = layer._on_device(g)
        layer.last_path = "device" if ctx.device_path else "host"
        if ctx.device_path:
            kw = dict(layer._device_bounds(g.device))
            if lbA is not None: kw["lbA"] = _dev(lbA, g.device)
            if ubA is not None: kw["ubA"] = _dev(ubA, g.device)
            if shared:
                # a matrix that is not an input is not handed over: the batch keeps it (NULL), a shared one is broadcast by the pack kernel
                m = {k: _dev(t, g.device) for k, t in given.items()}
                rc = bt.load_device(0, bt.B, m["Q"], _dev(g, g.device), m["L"], m["R"], A=m["A"], **kw)
                if rc != 0:
                    raise RuntimeError(f"load failed with code {rc}: {bt._last_error()}")
                layer._held = None      # (the host path reads the matrices back again when it next needs them)
                bt.run()
            else:
                rc = bt.update_device(0, bt.B, _dev(g, g.device), **kw)
                if rc != 0:
                    raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
                if layer.solves == 0:
                    bt.run()
                else:
                    bt.resolve(warm=layer.warm)
            x, y = bt.solution_device()
            layer.solves += 1
            layer.y, layer.stats = y, None
            layer._like = (g.dtype, g.device)
            ctx.layer, ctx.serial = layer, layer.solves
            ctx.given = (lbA is not None, ubA is not None)
            ctx.shared = shared
            return x.to(g.dtype), y.to(g.dtype)
        kw = dict(layer.bounds)
        if lbA is not None: kw["lbA"] = _host(lbA)
        if ubA is not None: kw["ubA"] = _host(ubA)
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
        each = tuple(k for k, sh in ctx.shared.items() if not sh)
        summed = tuple(k for k, sh in ctx.shared.items() if sh)
        if ctx.device_path:
            vx, vy = _dev(grad_x, grad_x.device), _dev(grad_y, grad_x.device)
            r = bt.adjoint_device(vx, vy, matrices=each, reduce=False)
            mats = {k: r[k] for k in each}
            if summed:
                rs = bt.adjoint_device(vx, vy, matrices=summed, reduce=True)
                mats.update({k: rs[k] for k in summed})
            layer.info = r["info"]
            _warn_flagged("LCQPFullSolveFunction", r["info"], bt.B)
            glb, gub = _bound_grads_device(bt, r["db"], r["side"], ctx.given, grad_x.dtype)
            gm = [mats[k].to(grad_x.dtype) if k in mats else None for k in MATRIX_KEYS]
            return (None, r["dg"].to(grad_x.dtype), *gm, glb, gub)
        vx, vy = _host(grad_x), _host(grad_y)
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
    for the shared ones (reduce = 1, the sum over the batch formed on the device).  Flagged instances: the one warning of LCQPSolveFunction.
    With g on the GPU of the batch the calls are the device-pointer twins (lcqp_hip_sparse_load_device and so on): an array that is not given
    is not handed over, the batch keeps it; a shared one is broadcast by the pack kernel."""

    @staticmethod
    def forward(ctx, layer, g, Qx=None, Ax=None, lbA=None, ubA=None):
        bt = layer.bt
        given = dict(zip(SPARSE_VALUE_KEYS, (Qx, Ax)))
        nnz = dict(Qx=bt.nnzQ, Ax=bt.nnzA)
        shared = {}
        for k, t in given.items():
            if t is None:
                continue
            if tuple(t.shape) not in ((bt.B, nnz[k]), (nnz[k],)):
                raise ValueError(f"{k}: expected [{bt.B}][{nnz[k]}] or [{nnz[k]}], got {tuple(t.shape)}")
            shared[k] = t.dim() == 1
        ctx.device_path = layer._on_device(g)
        layer.last_path = "device" if ctx.device_path else "host"
        if ctx.device_path:
            kw = dict(layer._device_bounds(g.device))
            if lbA is not None: kw["lbA"] = _dev(lbA, g.device)
            if ubA is not None: kw["ubA"] = _dev(ubA, g.device)
            if shared:
                rc = bt.load_device(0, bt.B, _dev(Qx, g.device), _dev(g, g.device), _dev(Ax, g.device), **kw)
                if rc != 0:
                    raise RuntimeError(f"load failed with code {rc}: {bt._last_error()}")
                layer._values_stale = True      # (the host path reads the value arrays back when it next needs them)
                bt.run()
            else:
                rc = bt.update_device(0, bt.B, _dev(g, g.device), **kw)
                if rc != 0:
                    raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
                if layer.solves == 0:
                    bt.run()
                else:
                    bt.resolve(warm=layer.warm)
            x, y = bt.solution_device()
            layer.solves += 1
            layer.y, layer.stats = y, None
            layer._like = (g.dtype, g.device)
            ctx.layer, ctx.serial = layer, layer.solves
            ctx.given = (lbA is not None, ubA is not None)
            ctx.shared = shared
            return x.to(g.dtype), y.to(g.dtype)
        kw = dict(layer.bounds)
        if lbA is not None: kw["lbA"] = _host(lbA)
        if ubA is not None: kw["ubA"] = _host(ubA)
        if shared:
            held = layer._values()
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
        name = dict(Qx="Q", Ax="A")      # the names of SparseBatchLCQP.adjoint
        each = tuple(name[k] for k, sh in ctx.shared.items() if not sh)
        summed = tuple(name[k] for k, sh in ctx.shared.items() if sh)
        if ctx.device_path:
            vx, vy = _dev(grad_x, grad_x.device), _dev(grad_y, grad_x.device)
            r = bt.adjoint_device(vx, vy, matrices=each, reduce=False)
            mats = {k: r[k] for k in each}
            if summed:
                rs = bt.adjoint_device(vx, vy, matrices=summed, reduce=True)
                mats.update({k: rs[k] for k in summed})
            layer.info = r["info"]
            _warn_flagged("LCQPSparseFullSolveFunction", r["info"], bt.B)
            glb, gub = _bound_grads_device(bt, r["db"], r["side"], ctx.given, grad_x.dtype, sparse=True)
            gm = [mats[name[k]].to(grad_x.dtype) if name[k] in mats else None for k in SPARSE_VALUE_KEYS]
            return (None, r["dg"].to(grad_x.dtype), *gm, glb, gub)
        vx, vy = _host(grad_x), _host(grad_y)
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
        self.last_path = None      # "device" or "host": the path of the last solve
        self._bounds_dev = None

    def __call__(self, g, lbA=None, ubA=None):
        return LCQPSolveFunction.apply(self, g, lbA, ubA)

    @property
    def stats(self):
        """the statistics of the last solve, a list of dicts; after a solve on the device path they are fetched through the host call
        (BatchLCQP.solution) when first asked for"""
        if self._stats is None and self.solves and self.last_path == "device":
            self._stats = self.bt.solution()[2]
        return self._stats

    @stats.setter
    def stats(self, st):
        self._stats = st

    def _on_device(self, g):
        """the device path: g a tensor on the GPU of the batch"""
        return g.is_cuda and g.device.index == getattr(self.bt, "device", None)

    def _device_bounds(self, device):
        """the layer's bound vectors as float64 tensors on the device, uploaded once"""
        if self._bounds_dev is None:
            self._bounds_dev = {k: torch.as_tensor(v, dtype=torch.float64, device=device).contiguous() for k, v in self.bounds.items()}
        return self._bounds_dev

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

    def jacobian(self, serial=None, duals=False):
        """dx/dg of the layer's last solve, [B][nV][nV] ([b][k][j] = dx_k/dg_j), a tensor of the dtype and on the device of that
        solve's g (BatchLCQP.jacobian / SparseBatchLCQP.jacobian: the arm's blocked kernel on the unit vectors).  serial: the value of layer.solves right
        after the solve that is meant -- like backward, the call raises when that is not the last one.  layer.info holds the flags.
        duals=True (dense batch): the whole solution map D(x, y) / D(g, b_W) as a dict of the four blocks -- xg [B][nV][nV], xb [B][nV][nd],
        yg [B][nd][nV], yb [B][nd][nd] (BatchLCQP.jacobian and .jacobian_duals) -- and side [B][nd]; with the last solve's g on the GPU of the
        batch the device-pointer twins write device tensors (layer.last_path = "device"), else the host calls run ("host")."""
        if self.solves == 0 or (serial is not None and serial != self.solves):
            raise RuntimeError("jacobian of a solve that is not the layer's last one: the batch object holds the state of one solve")
        if duals:
            dtype, device = self._like
            on_device = device.type == "cuda" and device.index == getattr(self.bt, "device", None)
            self.last_path = "device" if on_device else "host"
            if on_device:
                xg, xb, side, info = self.bt.jacobian_device()
                yg, yb, _, _ = self.bt.jacobian_duals_device()
            else:
                xg, xb, side, info = self.bt.jacobian()
                yg, yb, _, _ = self.bt.jacobian_duals()
            self.info = info if not on_device else info.cpu().numpy()
            out = {k: torch.as_tensor(v, device=device).to(dtype) for k, v in dict(xg=xg, xb=xb, yg=yg, yb=yb).items()}
            out["side"] = torch.as_tensor(side, device=device)
            return out
        Jg, _, _, info = self.bt.jacobian(bounds=False)
        self.info = info
        return torch.as_tensor(Jg, dtype=self._like[0], device=self._like[1])


class SparseBatchLCQPLayer(BatchLCQPLayer):
    """A loaded SparseBatchLCQP as a torch layer: the same function over lcqp_hip_sparse_update / _run / _resolve / _sensitivity (with g on the
    GPU of the batch: over their device-pointer twins; layer.last_path says which path ran).  bounds:
    the vectors of SparseBatchLCQP.update the batch was loaded with (lbA, ubA, lbL, ubL, lbR, ubR; the sparse arm has no box)."""
    sparse = True
    bound_keys = tuple(k for k in BOUND_KEYS if k not in ("lb", "ub"))

    def __init__(self, batch, bounds=None, warm=True, values=None, general_panel=None):
        """general_panel: True / False is handed to batch.set_general_panel -- jacobian() of a batch on the general sparse LDL' through that
        engine's panel kernel (None: the handle's setting stays).
        values: dict(Qx=[B][nnzQ], Ax=[B][nnzA]) (or [nnz], shared) -- the value arrays the batch was loaded with.  A layer whose solve()
        takes Qx or Ax needs them, the way it needs `bounds`: a host load replaces BOTH arrays, and the one that is not an input of the solve
        is handed over again.  The layer keeps them in step with its own loads (after a load on the device path: read back through
        SparseBatchLCQP.read_problem when the host path next needs them)."""
        super().__init__(batch, bounds=bounds, warm=warm)
        if general_panel is not None:
            batch.set_general_panel(bool(general_panel))
        self.values = None
        self._values_stale = False
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

    def jacobian(self, serial=None):
        """BatchLCQPLayer.jacobian without the dual blocks: the sparse arm has no panel call for them"""
        return super().jacobian(serial)

    def _values(self):
        """the value arrays the batch holds, [B][nnz] each, for a load on the host path"""
        if self._values_stale:
            ps = [self.bt.read_problem(b) for b in range(self.bt.B)]
            self.values = {k: np.stack([p[k] for p in ps]) for k in SPARSE_VALUE_KEYS}
            self._values_stale = False
        return self.values

    def solve(self, g, Qx=None, Ax=None, lbA=None, ubA=None):
        """(x, y) of the batch for the linear terms g, both differentiable (LCQPSparseFullSolveFunction): y [B][nC + 2 nComp], rows A, L, R.
        Qx, Ax: tensors that replace the value arrays of the batch for this and later solves, in the order of SparseBatchLCQP.load --
        [B][nnz] one per instance, [nnz] one shared by all instances (its gradient is the sum over the batch).  Qx.grad is the symmetric
        derivative on the full pattern.  Without any, the solve is the update + resolve of __call__."""
        if (Qx is not None or Ax is not None) and self.values is None:
            raise ValueError("solve: a layer that takes Qx or Ax needs the value arrays the batch holds -- construct it with "
                             "values=dict(Qx=..., Ax=...) (the sparse handle cannot read its matrices back)")
        return LCQPSparseFullSolveFunction.apply(self, g, Qx, Ax, lbA, ubA)
