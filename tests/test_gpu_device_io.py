"""The device-pointer entry points of the dense batch (lcqp_hip_batch_load_device / _update_device / _get_solution_device /
_sensitivity_device / _adjoint_device, DESIGN.md section 3a''''') against their oracle, the host entry points: every comparison is bit for
bit, so there is no tolerance anywhere in this file."""
import warnings

import numpy as np
import pytest
import torch      # noqa: F401 -- before the library is first loaded: the library and torch must share one HIP runtime (lcqpow_amd.capi.lib)

from batch_helpers import assert_same_bits, load_all, result, stack, update_all, vectors
from problems import perturbed, random_lcqp

pytestmark = pytest.mark.gpu

# (nV, nC, nComp, B, box, shifted, with x0 and y0): np = 128 twice (one with an odd row length), 256, 1024 (the other launch table), no rows of A
SHAPES = ((40, 20, 8, 5, False, False, False), (33, 7, 5, 3, True, True, True), (200, 330, 37, 3, True, False, False),
          (600, 200, 50, 2, True, True, False), (12, 0, 3, 2, False, False, False))
IDS = ["%dx%dx%d" % s[:3] for s in SHAPES]
MATS = ("Q", "A", "L", "R")
_cache = {}


def data(shape):
    """the instances of a shape and their perturbed twins, made once"""
    if shape not in _cache:
        n, nC, nComp, B, box, shifted, start = shape
        rng = np.random.default_rng(7 * n + B)
        ds = [random_lcqp(rng, n, nC, nComp, box, shifted) for _ in range(B)]
        if start:
            ds = [dict(d, x0=rng.uniform(-0.1, 0.1, n), y0=rng.uniform(-0.1, 0.1, n + nC + 2 * nComp)) for d in ds]
        _cache[shape] = (ds, [perturbed(d, 100 + b) for b, d in enumerate(ds)])
    return _cache[shape]


def make(hip, shape, trace=False):
    n, nC, nComp, B, box = shape[:5]
    return hip.BatchLCQP(B, n, nC, nComp, with_box=box, opt=hip.default_options(perturbStep=0, printLevel=0, storeSteps=1 if trace else 0))


def dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def load_device_all(bt, ds, first=0, only=MATS, shared=()):
    m = {k: (dev(ds[0][k]) if k in shared else dev(stack(ds, k))) if k in only else None for k in MATS}
    rc = bt.load_device(first, len(ds), m["Q"], dev(stack(ds, "g")), m["L"], m["R"], A=m["A"], **{k: dev(v) for k, v in vectors(bt.load, ds).items()})
    assert rc == 0, (rc, bt._last_error())


def update_device_all(bt, ds, first=0):
    rc = bt.update_device(first, len(ds), dev(stack(ds, "g")), **{k: dev(v) for k, v in vectors(bt.update, ds).items()})
    assert rc == 0, (rc, bt._last_error())


def same_problem_and_setup(a, b):
    for i in range(a.B):
        pa, pb = a.read_problem(i), b.read_problem(i)
        for k in pa:
            assert np.array_equal(pa[k], pb[k]), (i, k)
        sa, sb = a.read_setup(i), b.read_setup(i)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (i, k)


def solved_pair(hip, shape):
    """two handles with the same data, the first loaded from the host, the second from the device; both solved"""
    ds, _ = data(shape)
    a, b = make(hip, shape), make(hip, shape)
    load_all(a, ds); load_device_all(b, ds)
    a.run(); b.run()
    return a, b


# ---- 1: load_device leaves what load leaves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_load_device_equals_load(hip, shape):
    ds, _ = data(shape)
    a, b = make(hip, shape, trace=True), make(hip, shape, trace=True)
    load_all(a, ds); load_device_all(b, ds)
    a.run(); b.run()
    ra, rb = result(a, trace=True), result(b, trace=True)
    assert_same_bits(ra, rb)
    assert np.array_equal(ra["work"], rb["work"])
    same_problem_and_setup(a, b)
    a.close(); b.close()


# ---- 2, 3, 4: shared matrices, NULL matrices, a sub-range -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", (SHAPES[1], SHAPES[2]), ids=(IDS[1], IDS[2]))
def test_shared_matrices_are_broadcast(hip, shape):
    ds, _ = data(shape)
    ds = [dict(d, Q=ds[0]["Q"], A=ds[0]["A"]) for d in ds]
    a, b = make(hip, shape), make(hip, shape)
    load_all(a, ds); load_device_all(b, ds, shared=("Q", "A"))
    a.run(); b.run()
    assert_same_bits(result(a), result(b))
    same_problem_and_setup(a, b)
    a.close(); b.close()


@pytest.mark.parametrize("shape", (SHAPES[1], SHAPES[3]), ids=(IDS[1], IDS[3]))
def test_null_matrix_keeps_what_the_batch_holds(hip, shape):
    ds, _ = data(shape)
    ds2 = [dict(d, Q=d["Q"] + 0.25 * np.eye(d["nV"])) for d in ds]
    a, b = make(hip, shape), make(hip, shape)
    load_all(a, ds2)
    load_all(b, ds); b.run()                      # (a solved batch: its pools hold what a setup and a run leave)
    load_device_all(b, ds2, only=("Q",))
    a.run(); b.run()
    assert_same_bits(result(a), result(b))
    same_problem_and_setup(a, b)
    a.close(); b.close()
    c = make(hip, shape)                           # nothing to keep: the host twin's code for the missing matrix
    g = dev(stack(ds, "g"))
    assert c.load_device(0, c.B, None, g, dev(stack(ds, "L")), dev(stack(ds, "R")), A=dev(stack(ds, "A"))) == 100
    assert c.load_device(0, c.B, dev(stack(ds, "Q")), g, None, dev(stack(ds, "R")), A=dev(stack(ds, "A"))) == 118
    assert c.load_device(0, c.B, dev(stack(ds, "Q")), g, dev(stack(ds, "L")), dev(stack(ds, "R"))) == 117
    assert c.load_device(0, c.B, dev(stack(ds, "Q")), None, dev(stack(ds, "L")), dev(stack(ds, "R")), A=dev(stack(ds, "A"))) == 116
    c.close()


@pytest.mark.parametrize("shape", (SHAPES[0], SHAPES[1]), ids=(IDS[0], IDS[1]))
def test_sub_range_after_a_host_load(hip, shape):
    ds, _ = data(shape)
    a, b = make(hip, shape), make(hip, shape)
    load_all(a, ds)
    assert b.load(0, 1, *[stack(ds[:1], k) for k in ("Q", "g", "L", "R")], A=stack(ds[:1], "A"), **vectors(b.load, ds[:1])) == 0
    load_device_all(b, ds[1:], first=1)
    a.run(); b.run()
    assert_same_bits(result(a), result(b))
    same_problem_and_setup(a, b)
    a.close(); b.close()


# ---- 5, 6: update_device, and the two paths mixed on one handle ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_update_device_equals_update(hip, shape):
    ds, ds2 = data(shape)
    a, b = solved_pair(hip, shape)
    for warm in (False, True):
        update_all(a, ds2); update_device_all(b, ds2)
        a.resolve(warm=warm); b.resolve(warm=warm)
        assert_same_bits(result(a), result(b))
        assert a.launch_counts() == b.launch_counts()
        ds2 = ds                                   # (the warm re-solve goes back to the first vectors)
    a.close(); b.close()


@pytest.mark.parametrize("shape", (SHAPES[1], SHAPES[2]), ids=(IDS[1], IDS[2]))
def test_host_and_device_calls_mix(hip, shape):
    ds, ds2 = data(shape)
    a, b, c = make(hip, shape), make(hip, shape), make(hip, shape)
    load_all(a, ds); load_device_all(b, ds); load_all(c, ds)
    for bt in (a, b, c):
        bt.run()
    update_all(a, ds2); update_all(b, ds2); update_device_all(c, ds2)
    for bt in (a, b, c):
        bt.resolve(warm=True)
    ra = result(a)
    assert_same_bits(ra, result(b)); assert_same_bits(ra, result(c))
    assert a.launch_counts() == b.launch_counts() == c.launch_counts()
    for bt in (a, b, c):
        bt.close()


# ---- 7: refusals: the code, and a warm re-solve that returns what it returns without the refused call ------------------------------------
def test_refusals_change_nothing(hip):
    import torch
    shape = SHAPES[1]
    n, nC, nComp, B = shape[:4]
    # every second variable without an upper bound loses its lower one as well: free variables
    ds = [dict(d, lb=np.where(np.isfinite(d["ub"]) | (np.arange(n) % 2 == 0), d["lb"], -np.inf)) for d in data(shape)[0]]
    ds2 = [perturbed(d, 100 + b) for b, d in enumerate(ds)]
    a, b, never = make(hip, shape), make(hip, shape), make(hip, shape)
    load_all(a, ds); load_device_all(b, ds); load_device_all(never, ds)
    a.run(); b.run()
    assert_same_bits(result(a), result(b))
    g = dev(stack(ds2, "g"))
    kw = {k: dev(v) for k, v in vectors(b.update, ds2).items()}

    bad = stack(ds2, "lbL").copy(); bad[1, 2] = -np.inf
    assert b.update_device(0, B, g, **dict(kw, lbL=dev(bad))) == 120
    assert b.load_device(0, B, None, g, None, None, **dict(kw, lbL=dev(bad))) == 120

    lb, ub = stack(ds2, "lb"), stack(ds2, "ub").copy()
    hit = None
    for k in (2, 1):                               # two offenders: the message names the lowest (instance, variable), as the host's
        free = [i for i in range(n) if not np.isfinite(lb[k, i]) and not np.isfinite(ub[k, i])]
        assert len(free) > 1
        ub[k, free[-1]] = 1.0; hit = (k, free[-1])
    assert b.update_device(0, B, g, **dict(kw, ub=dev(ub))) == 100
    msg = b._last_error()
    assert a.update(0, B, stack(ds2, "g"), **dict(vectors(a.update, ds2), ub=ub)) == 100
    assert msg == a._last_error() and "variable %d of instance %d gains" % (hit[1], hit[0]) in msg

    pinned = torch.empty((B, n), dtype=torch.float64).pin_memory()
    raw = hip.lib().lcqp_hip_batch_update_device
    assert raw(b.h, 0, B, pinned.data_ptr(), *[None] * 10, None) == 100 and "g: not a device pointer" in b._last_error()
    assert raw(b.h, 0, B, np.zeros((B, n)).ctypes.data, *[None] * 10, None) == 100 and "g: not a device pointer" in b._last_error()

    vx = dev(np.ones((B, n)))
    buf = torch.zeros(B * n * n + 1, dtype=torch.float64, device="cuda:0")
    with pytest.raises(RuntimeError, match="dQ: not aligned to 16 bytes"):
        b.adjoint_device(vx, matrices=("Q",), out=dict(Q=buf[1:].view(B, n, n)))
    with pytest.raises(RuntimeError, match="code 300"):
        never.sensitivity_device(vx)
    with pytest.raises(RuntimeError, match="code 300"):
        never.adjoint_device(vx)

    a.resolve(warm=True); b.resolve(warm=True)
    assert_same_bits(result(a), result(b))
    assert a.launch_counts() == b.launch_counts()
    for bt in (a, b, never):
        bt.close()


# ---- 8, 9, 10: the solution and the derivatives, read and written where they lie ---------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_solution_sensitivity_and_adjoint_device(hip, shape):
    import ctypes
    n, nC, nComp, B = shape[:4]
    nd = n + nC + 2 * nComp
    ds, _ = data(shape)
    bt = make(hip, shape)
    load_device_all(bt, ds)
    bt.run()
    x, y, st = bt.solution()
    xd, yd, sd = bt.solution_device(stats=True)
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(yd.cpu().numpy(), y)
    raw = sd.cpu().numpy()
    assert [hip.capi.Stats.from_buffer_copy(raw[b].tobytes()).asdict() for b in range(B)] == st
    assert raw.shape[1] == ctypes.sizeof(hip.capi.Stats)

    rng = np.random.default_rng(n)
    V = rng.standard_normal((B, 3, n))
    for v in (V[:, 0], V[:, :1], V):
        for blocked in (False, True):
            want = bt.sensitivity(v, blocked=blocked)
            got = bt.sensitivity_device(dev(v), blocked=blocked)
            for w, g_ in zip(want, got):
                assert g_.is_cuda and np.array_equal(g_.cpu().numpy(), w)
            ms = bt.sensitivity_kernel_ms()
            assert ms > 0
    vx, vy = V[:, 0], rng.standard_normal((B, nd))
    for matrices in (MATS, ("A",), ()):
        for uy in (vy, None):
            for reduce in (False, True):
                want = bt.adjoint(vx, uy, matrices=matrices, reduce=reduce)
                small = bt.adjoint(vx, uy, matrices=matrices, reduce=reduce, _staging_bytes=1)
                got = bt.adjoint_device(dev(vx), dev(uy), matrices=matrices, reduce=reduce)
                assert set(got) == set(want)
                for k in want:
                    assert got[k].is_cuda and np.array_equal(got[k].cpu().numpy(), want[k]) and np.array_equal(small[k], want[k]), (k, matrices, reduce)
        assert bt.sensitivity_kernel_ms() > 0
    bt.close()


# ---- 11: stream order: nothing between the producer of g, the library and the consumer of x but the streams ------------------------------
def test_stream_order(hip):
    import torch
    shape = SHAPES[2]
    n, nC, nComp, B = shape[:4]
    ds, ds2 = data(shape)
    a, b = solved_pair(hip, shape)
    kw = {k: dev(v) for k, v in vectors(b.update, ds2).items()}
    g2 = dev(stack(ds2, "g"))
    big = torch.ones((4096, 4096), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        one = (big @ big)[0, 0] / 4096.0           # 1.0, behind a matrix product that takes the device a while
        g = g2 * one.to(torch.float64)
        assert b.update_device(0, B, g, **kw) == 0
        b.resolve(warm=True)
        x, y = b.solution_device()
        total = x.sum(dim=1)
    s.synchronize()
    update_all(a, ds2)
    a.resolve(warm=True)
    xa, ya, _ = a.solution()
    assert np.array_equal(x.cpu().numpy(), xa) and np.array_equal(y.cpu().numpy(), ya)
    assert np.array_equal(total.cpu().numpy(), dev(xa).sum(dim=1).cpu().numpy())      # (the same reduction kernel on the same bits)
    assert_same_bits(result(a), result(b))
    a.close(); b.close()


# ---- 12: the torch layer: the same bits from tensors on the device and from CPU tensors ----------------------------------------------------
def test_layer_device_path(hip):
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    shape = SHAPES[2]
    n, nC, nComp, B = shape[:4]
    ds, ds2 = data(shape)
    a, b = make(hip, shape), make(hip, shape)
    load_all(a, ds); load_all(b, ds)
    bounds = {k: v for k, v in vectors(a.update, ds).items() if v is not None and k not in ("x0", "y0")}
    la, lb_ = BatchLCQPLayer(a, bounds=bounds), BatchLCQPLayer(b, bounds=bounds)
    rng = np.random.default_rng(3)
    wx, wy = rng.standard_normal((B, n)), rng.standard_normal((B, n + nC + 2 * nComp))

    def leaves(where, **arrays):
        return {k: torch.tensor(v, dtype=torch.float64, device=where, requires_grad=True) for k, v in arrays.items()}

    def run(layer, where):
        out = []
        t = leaves(where, g=stack(ds, "g"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            x = layer(t["g"])
            (x * torch.as_tensor(wx, device=where)).sum().backward()
            out += [x, t["g"].grad]
            t = leaves(where, g=stack(ds2, "g"), Q=ds[0]["Q"] + 0.1 * np.eye(n), A=stack(ds2, "A") * 1.01, lbA=stack(ds2, "lbA"))
            x, y = layer.solve(t["g"], Q=t["Q"], A=t["A"], lbA=t["lbA"])
            ((x * torch.as_tensor(wx, device=where)).sum() + (y * torch.as_tensor(wy, device=where)).sum()).backward()
            out += [x, y] + [t[k].grad for k in ("g", "Q", "A", "lbA")]
        return out

    host = run(la, "cpu")
    device = run(lb_, "cuda:0")
    assert la.last_path == "host" and lb_.last_path == "device"
    assert len(host) == len(device) == 8
    for h, d in zip(host, device):
        assert d.is_cuda and d.shape == h.shape and np.array_equal(d.detach().cpu().numpy(), h.detach().numpy())
    assert lb_.y.is_cuda and lb_.info.is_cuda
    assert lb_.stats == la.stats
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        xh = lb_(torch.tensor(stack(ds, "g")))
    assert lb_.last_path == "host" and not xh.is_cuda
    a.close(); b.close()


def test_layer_device_path_equality_rows_and_flagged_instances(hip):
    """both bounds of an equality row as inputs (each gets half of the row's derivative) and the one warning about flagged instances,
    through layer(g, lbA, ubA) and through layer.solve(g, lbA=, ubA=): the same bits and the same warning from both paths"""
    import torch
    from lcqpow_amd.diff import BatchLCQPLayer
    shape = SHAPES[0]
    n, nC, nComp, B = shape[:4]
    ds, _ = data(shape)
    a, b = make(hip, shape), make(hip, shape)
    load_all(a, ds); load_all(b, ds)
    lo, hi = stack(ds, "lbA").copy(), stack(ds, "ubA").copy()
    lo[:, 0] = hi[:, 0] = 0.5 * (lo[:, 0] + hi[:, 0])      # row 0 of every instance: an equality inside the old range
    lo[1, 1] = hi[1, 1] + 1.0                               # instance 1: nothing satisfies its row 1, the solve fails
    la, lb_ = BatchLCQPLayer(a), BatchLCQPLayer(b)
    rng = np.random.default_rng(4)
    wx, wy = rng.standard_normal((B, n)), rng.standard_normal((B, n + nC + 2 * nComp))

    def run(layer, where):
        out, messages = [], []
        for full in (False, True):
            t = {k: torch.tensor(v, dtype=torch.float64, device=where, requires_grad=True) for k, v in dict(g=stack(ds, "g"), lbA=lo, ubA=hi).items()}
            if full:
                x, y = layer.solve(t["g"], lbA=t["lbA"], ubA=t["ubA"])
                loss = (x * torch.as_tensor(wx, device=where)).sum() + (y * torch.as_tensor(wy, device=where)).sum()
            else:
                x = y = layer(t["g"], t["lbA"], t["ubA"])
                loss = (x * torch.as_tensor(wx, device=where)).sum()
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                loss.backward()
            messages += [(w.category, str(w.message)) for w in rec]
            out += [x, y, t["g"].grad, t["lbA"].grad, t["ubA"].grad, torch.as_tensor(layer.info)]
        return out, messages

    host, said = run(la, "cpu")
    device, said_d = run(lb_, "cuda:0")
    assert la.last_path == "host" and lb_.last_path == "device"
    assert len(host) == len(device) == 12
    for h, d in zip(host, device):
        assert d.is_cuda and torch.equal(d.detach().cpu(), h.detach())
    assert said == said_d and len(said) == 2 and all(c is RuntimeWarning for c, _ in said)      # one per backward
    assert said[0][1].startswith(f"LCQPSolveFunction.backward: 1 of {B} instances") and said[1][1].startswith(f"LCQPFullSolveFunction.backward: 1 of {B} instances")
    for x, y, dg, dlo, dhi, info in (host[:6], host[6:]):
        ok = info == 0
        assert ok.tolist() == [True, False, True, True, True] and info[1] & 1
        assert torch.equal(dlo[:, 0], dhi[:, 0]) and torch.all(dlo[ok, 0] != 0)      # the equality row: half to each bound
        assert not torch.any((dlo[:, 1:] != 0) & (dhi[:, 1:] != 0))                # every other row sits on one bound at the most
    a.close(); b.close()
