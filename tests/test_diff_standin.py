"""The host path of the three autograd functions of lcqpow_amd.diff, held to what they ask of the batch object: driven through duck-typed
stand-ins (one dense, one sparse) that log every call and answer with fixed arrays.  No device is needed -- the built library only
because BatchLCQPLayer.__init__ calls capi.lib().  What is pinned: the calls of a first and a second solve and of a solve with matrix or
value tensors, the split of a backward into its adjoint calls, the gradients (the equality-row rule of lbA / ubA among them), the one
warning about flagged instances, the errors and their messages, and the layer's attributes.  (That an input which was not given gets
None is held by torch itself: autograd raises when backward returns a gradient for an input that was no tensor, so every backward below
that runs through autograd with some inputs left out checks it.)"""
import warnings

import numpy as np
import pytest
import torch

from lcqpow_amd import diff

B, NV, NC, NK = 3, 4, 2, 1
NNZQ, NNZA = 6, 5
STALE = "backward through a solve that is not the layer's last one: the batch object holds the state of one solve"


class _StandIn:
    """the methods the layers call on a batch object; log: (name, args, kwargs) of every call"""
    B, nV, nC, nComp, device = B, NV, NC, NK, None

    def __init__(self, info=(0, 0, 0)):
        nd = self.ndual
        self.log, self.rc = [], 0
        rng = np.random.default_rng(5)
        self.X, self.Y = rng.standard_normal((B, NV)), rng.standard_normal((B, nd))
        self.stats = [dict(returnValue=0, iterTotal=b) for b in range(B)]
        self.DG = rng.standard_normal((B, NV))
        self.DB = np.arange(1.0, B * nd + 1).reshape(B, nd)
        # the rows of A: instance 0 (equality, lower), 1 (equality, upper), 2 (lower, outside); every other row sits on a bound, so that
        # a wrong offset into the layout shows
        self.side = np.ones((B, nd), dtype=np.int32)
        self.side[:, self.a0:self.a0 + NC] = ((2, -1), (2, 1), (-1, 0))
        self.info = np.array(info, dtype=np.int32)
        self.J = rng.standard_normal((B, NV, NV))

    def _note(self, name, *a, **kw):
        self.log.append((name, a, kw))

    def names(self):
        return [e[0] for e in self.log]

    def _last_error(self):
        return "stand-in error"

    def update(self, *a, **kw):
        self._note("update", *a, **kw)
        return self.rc

    def load(self, *a, **kw):
        self._note("load", *a, **kw)
        return self.rc

    def run(self, *a, **kw):
        self._note("run", *a, **kw)

    def resolve(self, *a, **kw):
        self._note("resolve", *a, **kw)

    def solution(self):
        self._note("solution")
        return self.X, self.Y, self.stats

    def sensitivity(self, *a, **kw):
        self._note("sensitivity", *a, **kw)
        return self.DG, self.DB, self.side, self.info

    def adjoint(self, vx, vy=None, matrices=(), reduce=False):
        self._note("adjoint", vx, vy, matrices=matrices, reduce=reduce)
        r = dict(dg=self.DG, db=self.DB, side=self.side, info=self.info)
        for k in matrices:
            r[k] = self.grad_of(k, reduce)
        return r

    def grad_of(self, k, reduce):
        shp = (() if reduce else (B,)) + self.shapes[k]
        return (3.0 if reduce else 1.0) * (1 + sorted(self.shapes).index(k)) + np.arange(float(np.prod(shp))).reshape(shp)

    def jacobian(self, *a, **kw):
        self._note("jacobian", *a, **kw)
        return self.J, (None if kw.get("bounds") is False else np.zeros((B, NV, self.ndual))), self.side, self.info


class DenseStandIn(_StandIn):
    nd = ndual = NV + NC + 2 * NK
    a0 = NV
    shapes = dict(Q=(NV, NV), A=(NC, NV), L=(NK, NV), R=(NK, NV))

    def read_problem(self, b):
        self._note("read_problem", b)
        return {k: np.full(shp, 10.0 * (b + 1) + i) for i, (k, shp) in enumerate(self.shapes.items())}

    def jacobian_duals(self, *a, **kw):
        self._note("jacobian_duals", *a, **kw)
        return np.ones((B, self.nd, NV)), np.ones((B, self.nd, self.nd)), self.side, self.info


class SparseStandIn(_StandIn):
    m = ndual = NC + 2 * NK
    a0 = 0
    nnzQ, nnzA = NNZQ, NNZA
    shapes = dict(Q=(NNZQ,), A=(NNZA,))

    def read_problem(self, b):
        self._note("read_problem", b)
        return dict(Qx=np.full(NNZQ, 10.0 * (b + 1)), Ax=np.full(NNZA, 10.0 * (b + 1) + 1))


def f64(*shape, seed=0, grad=False):
    t = torch.as_tensor(np.random.default_rng(seed).standard_normal(shape), dtype=torch.float64)
    return t.requires_grad_(grad)


BOUNDS = dict(lbL=np.zeros((B, NK)), ubR=np.full((B, NK), 9.0), lbA=np.full((B, NC), -1.0), ubA=np.full((B, NC), 1.0))
VALUES = dict(Qx=np.arange(1.0, NNZQ + 1), Ax=np.arange(1.0, B * NNZA + 1).reshape(B, NNZA))


def make(arm, info=(0, 0, 0), **kw):
    if arm == "dense":
        bt = DenseStandIn(info)
        return bt, diff.BatchLCQPLayer(bt, bounds=BOUNDS, **kw)
    bt = SparseStandIn(info)
    return bt, diff.SparseBatchLCQPLayer(bt, bounds=BOUNDS, values=VALUES, **kw)


# the four ways into the three functions: (arm, how the layer is called, the function's name, whether y comes back)
DRIVERS = [("dense", "call", "LCQPSolveFunction"), ("sparse", "call", "LCQPSolveFunction"),
           ("dense", "solve", "LCQPFullSolveFunction"), ("sparse", "solve", "LCQPSparseFullSolveFunction")]
FULL = [d for d in DRIVERS if d[1] == "solve"]


def solve(layer, how, g, **kw):
    """(x, y or None) through __call__ or solve"""
    if how == "call":
        return layer(g, **kw), None
    return layer.solve(g, **kw)


def loss_of(x, y, wx, wy):
    return (x * wx).sum() + (0 if y is None else (y * wy).sum())


def same(a, b):
    return isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == np.shape(b) and np.array_equal(a, b)


@pytest.mark.parametrize("arm,how,name", DRIVERS)
@pytest.mark.parametrize("warm", (True, False))
def test_first_and_second_solve_update_then_run_then_resolve(arm, how, name, warm):
    bt, layer = make(arm, warm=warm)
    assert layer.last_path is None and layer.solves == 0
    g, lbA = f64(B, NV, seed=1), f64(B, NC, seed=2)
    for k in (1, 2):
        x, y = solve(layer, how, g * k, lbA=lbA)
        assert torch.equal(x, torch.as_tensor(bt.X)) and x.dtype == torch.float64
        if how == "solve":
            assert torch.equal(y, torch.as_tensor(bt.Y))
        assert layer.solves == k and layer.last_path == "host" and layer.y is bt.Y and layer.stats is bt.stats
    assert bt.names() == ["update", "run", "solution", "update", "resolve", "solution"]
    for k, e in ((1, bt.log[0]), (2, bt.log[3])):
        first, count, gh = e[1]
        assert (first, count) == (0, B) and same(gh, (g * k).numpy())
        assert set(e[2]) == set(BOUNDS)      # exactly the layer's bound keys: lbA is among them and is replaced by the tensor
        assert same(e[2]["lbA"], lbA.numpy())
        for key in ("lbL", "ubR", "ubA"):
            assert same(e[2][key], BOUNDS[key])
    assert bt.log[1][1:] == ((), {}) and bt.log[4][1:] == ((), dict(warm=warm))


@pytest.mark.parametrize("arm,how,name", DRIVERS)
def test_a_bound_the_layer_does_not_hold_is_added_and_float32_comes_back_as_float32(arm, how, name):
    bt = DenseStandIn() if arm == "dense" else SparseStandIn()
    layer = (diff.BatchLCQPLayer if arm == "dense" else diff.SparseBatchLCQPLayer)(bt, bounds=dict(lbL=BOUNDS["lbL"]))
    g, ubA = f64(B, NV, seed=1).to(torch.float32), f64(B, NC, seed=2).to(torch.float32)
    x, y = solve(layer, how, g, ubA=ubA)
    assert x.dtype == torch.float32 and torch.equal(x, torch.as_tensor(bt.X).to(torch.float32))
    if how == "solve":
        assert y.dtype == torch.float32 and torch.equal(y, torch.as_tensor(bt.Y).to(torch.float32))
    e = bt.log[0]
    assert e[0] == "update" and set(e[2]) == {"lbL", "ubA"}
    assert same(e[1][2], g.to(torch.float64).numpy()) and same(e[2]["ubA"], ubA.to(torch.float64).numpy())


def test_dense_solve_with_matrices_loads_the_whole_batch():
    bt, layer = make("dense")
    g, Q, A = f64(B, NV, seed=1), f64(NV, NV, seed=2), f64(B, NC, NV, seed=3)
    held = [DenseStandIn.read_problem(bt, b) for b in range(B)]
    bt.log.clear()
    x, y = layer.solve(g, Q=Q, A=A, ubA=f64(B, NC, seed=4))
    assert bt.names() == ["read_problem"] * B + ["load", "run", "solution"]
    assert [e[1] for e in bt.log[:B]] == [(b,) for b in range(B)]
    args, kw = bt.log[B][1:]
    assert args[:2] == (0, B) and len(args) == 6 and set(kw) == set(BOUNDS) | {"A"}
    assert same(args[2], np.broadcast_to(Q.numpy(), (B, NV, NV))) and same(args[3], g.numpy())
    assert same(args[4], np.stack([p["L"] for p in held])) and same(args[5], np.stack([p["R"] for p in held]))
    assert same(kw["A"], A.numpy()) and same(kw["ubA"], f64(B, NC, seed=4).numpy()) and same(kw["lbA"], BOUNDS["lbA"])
    assert layer.solves == 1 and layer.last_path == "host" and layer.y is bt.Y and layer.stats is bt.stats
    # again with another matrix: a load again (never a resolve), the matrices are not read back again, the earlier Q and A are kept
    bt.log.clear()
    L = f64(NK, NV, seed=5)
    layer.solve(g, L=L)
    assert bt.names() == ["load", "run", "solution"]
    args, kw = bt.log[0][1:]
    assert same(args[2], np.broadcast_to(Q.numpy(), (B, NV, NV))) and same(args[4], np.broadcast_to(L.numpy(), (B, NK, NV)))
    assert same(kw["A"], A.numpy())
    # and without one: update + resolve
    bt.log.clear()
    layer.solve(g)
    assert bt.names() == ["update", "resolve", "solution"] and layer.solves == 3


def test_sparse_solve_with_values_loads_the_whole_batch():
    bt, layer = make("sparse")
    g, Qx = f64(B, NV, seed=1), f64(NNZQ, seed=2)
    layer.solve(g, Qx=Qx, lbA=f64(B, NC, seed=4))
    assert bt.names() == ["load", "run", "solution"]
    args, kw = bt.log[0][1:]
    assert args[:2] == (0, B) and len(args) == 5 and set(kw) == set(BOUNDS)
    assert same(args[2], np.broadcast_to(Qx.numpy(), (B, NNZQ))) and same(args[3], g.numpy()) and same(args[4], VALUES["Ax"])
    assert same(kw["lbA"], f64(B, NC, seed=4).numpy())
    assert layer.solves == 1 and layer.last_path == "host" and layer.y is bt.Y and layer.stats is bt.stats
    bt.log.clear()
    Ax = f64(B, NNZA, seed=3)
    layer.solve(g, Ax=Ax)
    args = bt.log[0][1]
    assert bt.names() == ["load", "run", "solution"]
    assert same(args[2], np.broadcast_to(Qx.numpy(), (B, NNZQ))) and same(args[4], Ax.numpy())
    bt.log.clear()
    layer.solve(g)
    assert bt.names() == ["update", "resolve", "solution"]


def expected_bound_grads(bt, both):
    """the rule, written out: a row at its lower bound gives db to lbA, at its upper bound to ubA, an equality row to both -- half each
    when both are inputs"""
    sd = bt.side[:, bt.a0:bt.a0 + NC]; db = bt.DB[:, bt.a0:bt.a0 + NC]
    share = np.where(sd == 2, 0.5, 1.0) if both else 1.0
    lo = np.where((sd == -1) | (sd == 2), db, 0.0) * share
    hi = np.where((sd == 1) | (sd == 2), db, 0.0) * share
    return torch.as_tensor(lo), torch.as_tensor(hi)


@pytest.mark.parametrize("arm,how,name", DRIVERS)
@pytest.mark.parametrize("given", ((True, True), (True, False), (False, True), (False, False)))
def test_gradients_of_g_and_the_bounds(arm, how, name, given):
    bt, layer = make(arm)
    g = f64(B, NV, seed=1, grad=True)
    kw = {}
    if given[0]: kw["lbA"] = f64(B, NC, seed=2, grad=True)
    if given[1]: kw["ubA"] = f64(B, NC, seed=3, grad=True)
    wx, wy = f64(B, NV, seed=6), f64(B, bt.ndual, seed=7)
    x, y = solve(layer, how, g, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # info is zero: no warning
        loss_of(x, y, wx, wy).backward()
    assert torch.equal(g.grad, torch.as_tensor(bt.DG))      # dg as the batch object returned it
    lo, hi = expected_bound_grads(bt, all(given))
    if given[0]: assert torch.equal(kw["lbA"].grad, lo)
    if given[1]: assert torch.equal(kw["ubA"].grad, hi)
    assert layer.info is bt.info
    e = bt.log[-1]
    if how == "call":
        assert e[0] == "sensitivity" and len(e[1]) == 1 and e[2] == {} and same(e[1][0], wx.numpy())
    else:
        assert e[0] == "adjoint" and same(e[1][0], wx.numpy()) and same(e[1][1], wy.numpy()) and e[2] == dict(matrices=(), reduce=False)
        assert bt.names().count("adjoint") == 1


def test_float32_gradients_are_converted_last():
    bt, layer = make("dense")
    g = f64(B, NV, seed=1).to(torch.float32).requires_grad_(True)
    lbA, ubA = (f64(B, NC, seed=s).to(torch.float32).requires_grad_(True) for s in (2, 3))
    layer(g, lbA=lbA, ubA=ubA).sum().backward()
    lo, hi = expected_bound_grads(bt, True)
    assert g.grad.dtype == torch.float32 and torch.equal(g.grad, torch.as_tensor(bt.DG).to(torch.float32))
    assert torch.equal(lbA.grad, lo.to(torch.float32)) and torch.equal(ubA.grad, hi.to(torch.float32))


@pytest.mark.parametrize("arm,how,name", FULL)
@pytest.mark.parametrize("case", ("shared and per instance", "per instance only", "shared only"))
def test_backward_splits_the_matrices_into_each_and_summed(arm, how, name, case):
    bt, layer = make(arm)
    keys, trail = (("Q", "A"), ((NV, NV), (NC, NV))) if arm == "dense" else (("Qx", "Ax"), ((NNZQ,), (NNZA,)))
    lead = dict([("shared and per instance", ((), (B,))), ("per instance only", ((B,), (B,))), ("shared only", ((), ()))])[case]
    g = f64(B, NV, seed=1, grad=True)
    m = {k: f64(*(ld + tr), seed=10 + i, grad=True) for i, (k, ld, tr) in enumerate(zip(keys, lead, trail))}
    wx, wy = f64(B, NV, seed=6), f64(B, bt.ndual, seed=7)
    x, y = layer.solve(g, **m)
    loss_of(x, y, wx, wy).backward()
    calls = [e for e in bt.log if e[0] == "adjoint"]
    each = tuple(n for n, ld in zip(("Q", "A"), lead) if ld)
    summed = tuple(n for n, ld in zip(("Q", "A"), lead) if not ld)
    assert calls[0][2] == dict(matrices=each, reduce=False)
    assert len(calls) == (2 if summed else 1)
    if summed:
        assert calls[1][2] == dict(matrices=summed, reduce=True)
    for c in calls:
        assert same(c[1][0], wx.numpy()) and same(c[1][1], wy.numpy())
    for k, n, ld in zip(keys, ("Q", "A"), lead):
        assert torch.equal(m[k].grad, torch.as_tensor(bt.grad_of(n, not ld)))
    assert torch.equal(g.grad, torch.as_tensor(bt.DG)) and layer.info is bt.info


@pytest.mark.parametrize("arm,how,name", DRIVERS)
def test_one_warning_per_backward_with_flagged_instances(arm, how, name):
    bt, layer = make(arm, info=(0, 4, 2))
    g = f64(B, NV, seed=1, grad=True)
    x, y = solve(layer, how, g, lbA=f64(B, NC, seed=2, grad=True))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        loss_of(x, y, 1.0, 1.0).backward()
    assert len(w) == 1 and w[0].category is RuntimeWarning
    assert str(w[0].message) == (f"{name}.backward: 2 of {B} instances are not differentiable by the library's criteria "
                                 "(info bits present: 6); their gradients are the kernel's output as it is")
    assert torch.equal(g.grad, torch.as_tensor(bt.DG)) and layer.info is bt.info      # the gradients are the kernel's output as it is


@pytest.mark.parametrize("arm,how,name", DRIVERS)
def test_a_refused_update_and_a_stale_backward_raise(arm, how, name):
    bt, layer = make(arm)
    g = f64(B, NV, seed=1, grad=True)
    bt.rc = 7
    with pytest.raises(RuntimeError) as e:
        solve(layer, how, g)
    assert str(e.value) == "update failed with code 7: stand-in error"
    assert layer.solves == 0 and bt.names() == ["update"]
    bt.rc = 0
    x1, y1 = solve(layer, how, g)
    solve(layer, how, g)
    with pytest.raises(RuntimeError) as e:
        loss_of(x1, y1, 1.0, 1.0).backward()
    assert str(e.value) == STALE
    assert "sensitivity" not in bt.names() and "adjoint" not in bt.names()


@pytest.mark.parametrize("arm,how,name", FULL)
def test_a_refused_load_raises(arm, how, name):
    bt, layer = make(arm)
    bt.rc = 116
    m = dict(Q=f64(NV, NV)) if arm == "dense" else dict(Qx=f64(NNZQ))
    with pytest.raises(RuntimeError) as e:
        layer.solve(f64(B, NV, seed=1), **m)
    assert str(e.value) == "load failed with code 116: stand-in error"
    assert layer.solves == 0 and bt.names()[-1] == "load"


def test_wrongly_shaped_matrix_and_value_tensors_are_refused_before_any_call():
    bt, layer = make("dense")
    g = f64(B, NV, seed=1)
    for k, t, msg in (("Q", f64(NV + 1, NV), f"Q: expected [{B}][{NV}][{NV}] or [{NV}][{NV}], got ({NV + 1}, {NV})"),
                      ("A", f64(B + 1, NC, NV), f"A: expected [{B}][{NC}][{NV}] or [{NC}][{NV}], got ({B + 1}, {NC}, {NV})"),
                      ("R", f64(NV), f"R: expected [{B}][{NK}][{NV}] or [{NK}][{NV}], got ({NV},)")):
        with pytest.raises(ValueError) as e:
            layer.solve(g, **{k: t})
        assert str(e.value) == msg
    sb, slayer = make("sparse")
    for k, t, msg in (("Qx", f64(NNZQ + 1), f"Qx: expected [{B}][{NNZQ}] or [{NNZQ}], got ({NNZQ + 1},)"),
                      ("Ax", f64(B, NNZA, 1), f"Ax: expected [{B}][{NNZA}] or [{NNZA}], got ({B}, {NNZA}, 1)")):
        with pytest.raises(ValueError) as e:
            slayer.solve(g, **{k: t})
        assert str(e.value) == msg
    assert bt.log == [] and sb.log == [] and layer.solves == 0 and slayer.solves == 0


@pytest.mark.parametrize("arm", ("dense", "sparse"))
def test_layer_jacobian_on_the_host_path(arm):
    bt, layer = make(arm)
    with pytest.raises(RuntimeError, match="jacobian of a solve that is not the layer's last one"):
        layer.jacobian()
    layer(f64(B, NV, seed=1).to(torch.float32))
    bt.log.clear()
    J = layer.jacobian(serial=1)
    assert bt.log == [("jacobian", (), dict(bounds=False))] and layer.info is bt.info
    assert J.dtype == torch.float32 and torch.equal(J, torch.as_tensor(bt.J).to(torch.float32))
    with pytest.raises(RuntimeError, match="jacobian of a solve that is not the layer's last one"):
        layer.jacobian(serial=2)
    if arm == "dense":
        bt.log.clear()
        d = layer.jacobian(duals=True)
        assert bt.log == [("jacobian", (), {}), ("jacobian_duals", (), {})] and layer.last_path == "host"
        assert sorted(d) == ["side", "xb", "xg", "yb", "yg"] and torch.equal(d["xg"], torch.as_tensor(bt.J).to(torch.float32))
