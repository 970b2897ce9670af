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

The three autograd functions share one solve and one backward routine (_solve, _backward).  What the two paths do differently is in
_HostPath / _DevicePath, what the two arms do differently is on the layer classes.
"""
import warnings

import numpy as np
import torch

from . import capi

BOUND_KEYS = ("lbL", "ubL", "lbR", "ubR", "lbA", "ubA", "lb", "ub")
MATRIX_KEYS = ("Q", "A", "L", "R")
SPARSE_VALUE_KEYS = ("Qx", "Ax")


def _host(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().to(torch.float64).numpy())


def _dev(t, device):
    """a tensor argument as the device-pointer entry points take it: float64, contiguous, on `device`, detached"""
    return None if t is None else t.detach().to(device=device, dtype=torch.float64).contiguous()


class _HostPath:
    """the host-pointer calls around a solve: tensors become numpy arrays, results become tensors like `ref` (the g or the upstream
    gradient of the call)"""
    name, suffix = "host", ""

    @staticmethod
    def conv(t, ref):
        return _host(t)

    @staticmethod
    def out(a, ref):
        return torch.as_tensor(a, dtype=ref.dtype, device=ref.device)

    @staticmethod
    def bounds(layer, ref):
        return layer.bounds

    @staticmethod
    def load_arrays(layer, replaced, ref):
        """a host load replaces every array: the ones the layer holds, with the inputs broadcast over the batch in their place (and kept)"""
        held = layer._held_arrays()
        for k, t in replaced.items():
            if t is not None:
                held[k] = np.ascontiguousarray(np.broadcast_to(_host(t), (layer.bt.B,) + layer._trailing(k)))
        return held

    @staticmethod
    def loaded(layer):
        pass

    @staticmethod
    def update_matrices(layer, given, ref):
        """the given matrices alone, broadcast over the batch; the copies the layer holds are kept in step"""
        full = {k: np.ascontiguousarray(np.broadcast_to(_host(t), (layer.bt.B,) + layer._trailing(k))) for k, t in given.items()}
        layer._keep_sent(full)
        return layer._update_matrices("", full)


class _DevicePath:
    """the device-pointer twins (capi: *_device): tensors stay where they are, float64; results are converted to ref's dtype"""
    name, suffix = "device", "_device"

    @staticmethod
    def conv(t, ref):
        return _dev(t, ref.device)

    @staticmethod
    def out(a, ref):
        return a.to(ref.dtype)

    @staticmethod
    def bounds(layer, ref):
        return layer._device_bounds(ref.device)

    @staticmethod
    def load_arrays(layer, replaced, ref):
        """an array that is not an input is not handed over: the batch keeps it (NULL), a shared one is broadcast by the pack kernel"""
        return {k: _dev(t, ref.device) for k, t in replaced.items()}

    @staticmethod
    def loaded(layer):
        layer._mark_stale()      # (the host path reads the arrays back again when it next needs them)

    @staticmethod
    def update_matrices(layer, given, ref):
        """the given matrices alone, from where they lie; a shared one is broadcast by the pack kernel"""
        layer._mark_stale()
        return layer._update_matrices("_device", {k: _dev(t, ref.device) for k, t in given.items()})


def _solve(ctx, layer, g, lbA, ubA, replaced):
    """The forward of all three functions, on either path.  replaced: the matrix or value tensors of the call by name (None: not given).
    Without one: update + run (first solve) / resolve(warm); with one: a load of the whole batch + run.  Returns (path, x, y), x and y
    as the batch object returned them."""
    bt = layer.bt
    shared = {}
    for k, t in replaced.items():
        if t is None:
            continue
        trail = layer._trailing(k)
        if tuple(t.shape) not in ((bt.B,) + trail, trail):
            dims = "".join(f"[{d}]" for d in trail)
            raise ValueError(f"{k}: expected [{bt.B}]{dims} or {dims}, got {tuple(t.shape)}")
        shared[k] = t.dim() == len(trail)
    path = ctx.path = _DevicePath if layer._on_device(g) else _HostPath
    layer.last_path = path.name
    kw = dict(path.bounds(layer, g))
    if lbA is not None: kw["lbA"] = path.conv(lbA, g)
    if ubA is not None: kw["ubA"] = path.conv(ubA, g)
    if shared and layer.solves > 0 and layer.warm_matrices:
        # the batch holds a solved point: only the given matrices are sent, and the solve starts from that point (update_matrices / update_values)
        given = {k: t for k, t in replaced.items() if t is not None}
        rc = path.update_matrices(layer, given, g)
        if rc == 0:
            rc = getattr(bt, "update" + path.suffix)(0, bt.B, path.conv(g, g), **kw)
        if rc != 0:
            raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
        bt.resolve(warm=True)
    elif shared:
        rc = layer._load(getattr(bt, "load" + path.suffix), path.load_arrays(layer, replaced, g), path.conv(g, g), kw)
        if rc != 0:
            raise RuntimeError(f"load failed with code {rc}: {bt._last_error()}")
        path.loaded(layer)
        bt.run()
    else:
        rc = getattr(bt, "update" + path.suffix)(0, bt.B, path.conv(g, g), **kw)
        if rc != 0:
            raise RuntimeError(f"update failed with code {rc}: {bt._last_error()}")
        if layer.solves == 0:
            bt.run()
        else:
            bt.resolve(warm=layer.warm)
    x, y, *st = getattr(bt, "solution" + path.suffix)()
    layer.solves += 1
    layer.y, layer.stats = y, (st[0] if st else None)      # (device path: the statistics through the host call, when layer.stats is read)
    layer._like = (g.dtype, g.device)
    ctx.layer, ctx.serial = layer, layer.solves
    ctx.given = (lbA is not None, ubA is not None)
    ctx.shared = shared
    return path, x, y


def _warn_flagged(who, info, B):
    """the one warning of a backward call; info: numpy or a tensor on the device, where the count is the one scalar read of that call"""
    bad = int(torch.count_nonzero(info)) if torch.is_tensor(info) else int(np.count_nonzero(info))
    if bad:
        bits = int(np.bitwise_or.reduce(info.cpu().numpy() if torch.is_tensor(info) else info))
        warnings.warn(f"{who}.backward: {bad} of {B} instances are not differentiable by the library's criteria "
                      f"(info bits present: {bits}); their gradients are the kernel's output as it is", RuntimeWarning, stacklevel=4)


def _bound_grads(layer, db, side, given, out):
    """the gradients of lbA / ubA, db and side numpy or tensors: split_bound_derivatives and the equality rule of LCQPSolveFunction"""
    bt = layer.bt
    on_device = torch.is_tensor(db)
    split = capi.split_bound_derivatives_torch if on_device else capi.split_bound_derivatives
    parts = split(db, side, bt.nV, bt.nC, bt.nComp, sparse=layer.sparse)
    a0 = 0 if layer.sparse else bt.nV      # first row of A in the layout of side
    eq = side[:, a0:a0 + bt.nC] == 2
    if on_device:
        one = db.new_ones(())
        share = torch.where(eq, 0.5 * one, one) if all(given) else one
    else:
        share = np.where(eq, 0.5, 1.0) if all(given) else 1.0
    glb = out(parts["dlbA"] * share) if given[0] else None
    gub = out(parts["dubA"] * share) if given[1] else None
    return glb, gub


def _backward(who, ctx, grad_x, grad_y=None, adjoint=False):
    """The backward of all three functions, on the path of the solve.  adjoint=False: one sensitivity call; True: the adjoint call for
    the per-instance inputs (reduce = 0) and, where there are shared ones, a second for those (reduce = 1).  Returns the gradients of
    (layer, g, *the layer's input keys when adjoint, lbA, ubA)."""
    layer = ctx.layer
    if ctx.serial != layer.solves:
        raise RuntimeError("backward through a solve that is not the layer's last one: the batch object holds the state of one solve")
    bt, path = layer.bt, ctx.path
    out = lambda a: path.out(a, grad_x)
    mats = {}
    if adjoint:
        name = layer.adjoint_names
        each = tuple(name[k] for k, sh in ctx.shared.items() if not sh)
        summed = tuple(name[k] for k, sh in ctx.shared.items() if sh)
        call = getattr(bt, "adjoint" + path.suffix)
        vx, vy = path.conv(grad_x, grad_x), path.conv(grad_y, grad_x)
        r = call(vx, vy, matrices=each, reduce=False)
        mats.update({k: r[k] for k in each})
        if summed:
            rs = call(vx, vy, matrices=summed, reduce=True)
            mats.update({k: rs[k] for k in summed})
        dg, db, side, info = r["dg"], r["db"], r["side"], r["info"]
        gm = [out(mats[name[k]]) if name[k] in mats else None for k in layer.input_keys]
    else:
        dg, db, side, info = getattr(bt, "sensitivity" + path.suffix)(path.conv(grad_x, grad_x))
        gm = []
    layer.info = info
    _warn_flagged(who, info, bt.B)
    glb, gub = _bound_grads(layer, db, side, ctx.given, out)
    return (None, out(dg), *gm, glb, gub)


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
        path, x, _ = _solve(ctx, layer, g, lbA, ubA, {})
        return path.out(x, g)

    @staticmethod
    def backward(ctx, grad_x):
        return _backward("LCQPSolveFunction", ctx, grad_x)


class LCQPFullSolveFunction(torch.autograd.Function):
    """forward(layer, g, Q, A, L, R, lbA, ubA) -> (x, y).  Without matrix tensors: update + run / resolve(warm), as LCQPSolveFunction.  With
    one: lcqp_hip_batch_load of the whole batch + run; a tensor of shape [B][..][nV] holds one matrix per instance, one of shape [..][nV] is
    shared by the batch (broadcast at the load); a matrix that is not given is the one the batch holds.
    backward: lcqp_hip_batch_adjoint with the upstream gradients on x and on y -- gradients for g, for lbA / ubA where they were tensors (the
    rules of LCQPSolveFunction), and for the matrix tensors: per instance (reduce = 0) or, for a shared tensor, summed over the batch on the
    device (reduce = 1).  Flagged instances: the one warning of LCQPSolveFunction."""

    @staticmethod
    def forward(ctx, layer, g, Q=None, A=None, L=None, R=None, lbA=None, ubA=None):
        path, x, y = _solve(ctx, layer, g, lbA, ubA, dict(zip(MATRIX_KEYS, (Q, A, L, R))))
        return path.out(x, g), path.out(y, g)

    @staticmethod
    def backward(ctx, grad_x, grad_y):
        return _backward("LCQPFullSolveFunction", ctx, grad_x, grad_y, adjoint=True)


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
        path, x, y = _solve(ctx, layer, g, lbA, ubA, dict(zip(SPARSE_VALUE_KEYS, (Qx, Ax))))
        return path.out(x, g), path.out(y, g)

    @staticmethod
    def backward(ctx, grad_x, grad_y):
        return _backward("LCQPSparseFullSolveFunction", ctx, grad_x, grad_y, adjoint=True)


class BatchLCQPLayer:
    """A loaded BatchLCQP as a torch layer.  bounds: the bound vectors the batch was loaded with ([B][...] arrays under the names of
    BatchLCQP.update: lbL, ubL, lbR, ubR, lbA, ubA, lb, ub) -- an update replaces EVERY vector, so the ones that are not inputs of the
    layer are handed over again with every solve.  warm: re-solves start from the last solution where it exists."""

    # what the arms differ in (_solve and _backward read these): the layout of side, the bound vectors, the matrix inputs of solve in
    # their order and the name each has in adjoint(matrices=...) -- and _trailing, _held_arrays, _mark_stale, _load below
    sparse = False
    bound_keys = BOUND_KEYS
    input_keys = MATRIX_KEYS
    adjoint_names = dict(zip(MATRIX_KEYS, MATRIX_KEYS))

    def __init__(self, batch, bounds=None, warm=True, warm_matrices=False):
        capi.lib()      # raises when the HIP library is not built: no CPU fallback
        self.warm_matrices = bool(warm_matrices)      # solve() with matrices: update_matrices (sparse: update_values) + resolve(warm)
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
        update + resolve of __call__.  With one, on a layer constructed with warm_matrices=True that has solved before: the matrices go
        through BatchLCQP.update_matrices instead of a load, and the solve is a resolve(warm=True) from the last solution and working set
        on the new matrices ("New matrices"); the default is the load + cold run.  (The switch is the layer's, not
        an argument: the parameter list of solve is part of this class's tested surface.)"""
        return LCQPFullSolveFunction.apply(self, g, Q, A, L, R, lbA, ubA)

    def _trailing(self, k):
        """the shape of one instance's matrix k"""
        bt = self.bt
        return (dict(Q=bt.nV, A=bt.nC, L=bt.nComp, R=bt.nComp)[k], bt.nV)

    def _held_arrays(self):
        """the matrices the batch holds, [B][..][nV] each: read back once, then kept in step with the loads of solve"""
        if self._held is None:
            ps = [self.bt.read_problem(b) for b in range(self.bt.B)]
            self._held = {k: np.stack([p[k] for p in ps]) for k in MATRIX_KEYS}
        return self._held

    def _mark_stale(self):
        """after a load on the device path: the host copies of the matrices are read back when they are next needed"""
        self._held = None

    def _load(self, load, m, g, kw):
        """load: BatchLCQP.load or .load_device; m: the four matrices by name"""
        return load(0, self.bt.B, m["Q"], g, m["L"], m["R"], A=m["A"], **kw)

    def _keep_sent(self, full):
        """after update_matrices on the host path: the copies the layer holds take the arrays that were sent"""
        if self._held is not None:
            self._held.update(full)

    def _update_matrices(self, suffix, arrays):
        """the given matrices alone to the whole batch: BatchLCQP.update_matrices or (suffix "_device") its device-pointer twin"""
        return getattr(self.bt, "update_matrices" + suffix)(0, self.bt.B, **arrays)

    def _last_solve(self, serial):
        if self.solves == 0 or (serial is not None and serial != self.solves):
            raise RuntimeError("jacobian of a solve that is not the layer's last one: the batch object holds the state of one solve")

    def _jacobian_blocks(self, device_twins):
        """the four blocks of D(x, y) / D(g, b_W) of the last solve and side as tensors of the dtype and on the device of that solve's g: jacobian + jacobian_duals of the batch, or -- device_twins, with that g on the GPU of
        the batch -- their device-pointer twins"""
        dtype, device = self._like
        on_device = device_twins and device.type == "cuda" and device.index == getattr(self.bt, "device", None)
        self.last_path = "device" if on_device else "host"
        if on_device:
            xg, xb, side, info = self.bt.jacobian_device()
            yg, yb, _, _ = self.bt.jacobian_duals_device()
        else:
            xg, xb, side, info = self.bt.jacobian()
            yg, yb, _, _ = self.bt.jacobian_duals()
        self.info = info if not on_device else info.cpu().numpy()
        self._info_as_returned = info      # (on the device path: the tensor, for a caller that wants it there)
        out = {k: torch.as_tensor(v, device=device).to(dtype) for k, v in dict(xg=xg, xb=xb, yg=yg, yb=yb).items()}
        out["side"] = torch.as_tensor(side, device=device)
        return out

    def jacobian(self, serial=None, duals=False):
        """dx/dg of the layer's last solve, [B][nV][nV] ([b][k][j] = dx_k/dg_j), a tensor of the dtype and on the device of that
        solve's g (BatchLCQP.jacobian / SparseBatchLCQP.jacobian: the arm's blocked kernel on the unit vectors).  serial: the value of layer.solves right
        after the solve that is meant -- like backward, the call raises when that is not the last one.  layer.info holds the flags.
        duals=True (dense batch): the whole solution map D(x, y) / D(g, b_W) as a dict of the four blocks -- xg [B][nV][nV], xb [B][nV][nd],
        yg [B][nd][nV], yb [B][nd][nd] (BatchLCQP.jacobian and .jacobian_duals) -- and side [B][nd]; with the last solve's g on the GPU of the
        batch the device-pointer twins write device tensors (layer.last_path = "device"), else the host calls run ("host")."""
        self._last_solve(serial)
        if duals:
            return self._jacobian_blocks(device_twins=True)
        Jg, _, _, info = self.bt.jacobian(bounds=False)
        self.info = info
        return torch.as_tensor(Jg, dtype=self._like[0], device=self._like[1])


class SparseBatchLCQPLayer(BatchLCQPLayer):
    """A loaded SparseBatchLCQP as a torch layer: the same function over lcqp_hip_sparse_update / _run / _resolve / _sensitivity (with g on the
    GPU of the batch: over their device-pointer twins; layer.last_path says which path ran).  bounds:
    the vectors of SparseBatchLCQP.update the batch was loaded with (lbA, ubA, lbL, ubL, lbR, ubR; the sparse arm has no box)."""
    sparse = True
    bound_keys = tuple(k for k in BOUND_KEYS if k not in ("lb", "ub"))
    input_keys = SPARSE_VALUE_KEYS
    adjoint_names = dict(Qx="Q", Ax="A")      # the names of SparseBatchLCQP.adjoint

    def __init__(self, batch, bounds=None, warm=True, values=None, general_panel=None, warm_matrices=False):
        """warm_matrices: solve() with Qx or Ax on a layer that has solved before sends the given arrays alone through
        SparseBatchLCQP.update_values and solves by resolve(warm=True) from the last solution and working set ("New
        matrices: the sparse arm"); such a solve needs no `values`.  The default is the load + cold run.
        general_panel: True / False is handed to batch.set_general_panel -- jacobian() of a batch on the general sparse LDL' through that
        engine's panel kernel (None: the handle's setting stays).
        values: dict(Qx=[B][nnzQ], Ax=[B][nnzA]) (or [nnz], shared) -- the value arrays the batch was loaded with.  A layer whose solve()
        takes Qx or Ax needs them, the way it needs `bounds`: a host load replaces BOTH arrays, and the one that is not an input of the solve
        is handed over again.  The layer keeps them in step with its own loads (after a load on the device path: read back through
        SparseBatchLCQP.read_problem when the host path next needs them)."""
        super().__init__(batch, bounds=bounds, warm=warm, warm_matrices=warm_matrices)
        if general_panel is not None:
            batch.set_general_panel(bool(general_panel))
        self.values = None
        self._values_stale = False
        if values is not None:
            if set(values) != set(SPARSE_VALUE_KEYS):
                raise ValueError(f"values: expected the keys {list(SPARSE_VALUE_KEYS)}, got {sorted(values)}")
            self.values = {}
            for k in SPARSE_VALUE_KEYS:
                v = capi._arr(values[k])
                nnz, = self._trailing(k)
                if v.shape not in ((batch.B, nnz), (nnz,)):
                    raise ValueError(f"values[{k!r}]: expected [{batch.B}][{nnz}] or [{nnz}], got {v.shape}")
                self.values[k] = np.ascontiguousarray(np.broadcast_to(v, (batch.B, nnz)))

    def jacobian(self, serial=None):
        """BatchLCQPLayer.jacobian without the dual blocks (its signature is part of this class's tested surface): jacobian_full has them"""
        return super().jacobian(serial)

    def jacobian_full(self, serial=None):
        """The whole solution map D(x, y) / D(g, b_W) of the layer's last solve, the dict BatchLCQPLayer.jacobian(duals=True) returns: xg
        [B][nV][nV], xb [B][nV][m], yg [B][m][nV], yb [B][m][m] (SparseBatchLCQP.jacobian and .jacobian_duals: the arm's panel kernels on the
        unit vectors, DESIGN.md section 3a''''), side [B][m], and info [B], as tensors of the dtype and on the device of that solve's g.  With
        that g on the GPU of the batch the device-pointer twins run (SparseBatchLCQP.jacobian_device and .jacobian_duals_device: the staged
        panels go to the six device tensors on the device, nothing passes through the host; layer.last_path = "device"), else the host calls
        ("host").  serial: as jacobian."""
        self._last_solve(serial)
        out = self._jacobian_blocks(device_twins=True)
        out["info"] = torch.as_tensor(self._info_as_returned, device=self._like[1])
        return out

    def _trailing(self, k):
        """the shape of one instance's value array k"""
        return (dict(Qx=self.bt.nnzQ, Ax=self.bt.nnzA)[k],)

    def _held_arrays(self):
        """the value arrays the batch holds, [B][nnz] each, for a load on the host path"""
        if self._values_stale:
            ps = [self.bt.read_problem(b) for b in range(self.bt.B)]
            self.values = {k: np.stack([p[k] for p in ps]) for k in SPARSE_VALUE_KEYS}
            self._values_stale = False
        return self.values

    def _mark_stale(self):
        self._values_stale = True

    def _load(self, load, m, g, kw):
        """load: SparseBatchLCQP.load or .load_device; m: the two value arrays by name"""
        return load(0, self.bt.B, m["Qx"], g, m["Ax"], **kw)

    def _keep_sent(self, full):
        """after update_values on the host path: the layer's `values` take the arrays that were sent (a stale copy is read back whole)"""
        if self.values is not None and not self._values_stale:
            self.values.update(full)

    def _update_matrices(self, suffix, arrays):
        """the given value arrays alone to the whole batch: SparseBatchLCQP.update_values or (suffix "_device") its device-pointer twin"""
        return getattr(self.bt, "update_values" + suffix)(0, self.bt.B, **arrays)

    def solve(self, g, Qx=None, Ax=None, lbA=None, ubA=None):
        """(x, y) of the batch for the linear terms g, both differentiable (LCQPSparseFullSolveFunction): y [B][nC + 2 nComp], rows A, L, R.
        Qx, Ax: tensors that replace the value arrays of the batch for this and later solves, in the order of SparseBatchLCQP.load --
        [B][nnz] one per instance, [nnz] one shared by all instances (its gradient is the sum over the batch).  Qx.grad is the symmetric
        derivative on the full pattern.  Without any, the solve is the update + resolve of __call__."""
        if (Qx is not None or Ax is not None) and self.values is None and not (self.warm_matrices and self.solves > 0):
            raise ValueError("solve: a layer that takes Qx or Ax needs the value arrays the batch holds -- construct it with "
                             "values=dict(Qx=..., Ax=...) (the sparse handle cannot read its matrices back)")
        return LCQPSparseFullSolveFunction.apply(self, g, Qx, Ax, lbA, ubA)
