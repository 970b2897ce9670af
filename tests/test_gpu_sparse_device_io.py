"""The device-pointer entry points of the sparse batch (lcqp_hip_sparse_load_device / _update_device / _get_solution_device /
_sensitivity_device / _adjoint_device, DESIGN.md section 3a''''') against their oracle, the host entry points: every comparison is bit for
bit, so there is no tolerance anywhere in this file.  lcqp_hip_sparse_read_problem holds the pools themselves, not only the solutions."""
import torch      # noqa: F401 -- before the library is first loaded: the library and torch must share one HIP runtime (lcqpow_amd.capi.lib)

import warnings

import numpy as np
import pytest

import problems as P
from batch_helpers import environment, stack, vectors
from problems import MID, OPT, SMALL, circle_instances, instances, moved

pytestmark = pytest.mark.gpu

ODD = (63, 31, 7)      # nnzQ = 187: the instances of the flat [B][nnzQ] array start on odd offsets
#        instances              environment
CASES = {"small": (("synth", SMALL, 6), {}),
         "lanes 32": (("synth", SMALL, 6), {"LCQP_SPARSE_LANES": "32"}),
         "pools of 4": (("synth", SMALL, 6), {"LCQP_SPARSE_POOL": "4"}),      # a ragged last pool
         "general ldl": (("synth", SMALL, 6), {"LCQP_SPARSE_GENERAL": "1"}),
         "mid": (("synth", MID, 2), {}),
         "bordered circle": (("circle", 100, 2), {}),                        # x0 given; every Hessian has min Q_ii / max Q_ii = 5e-12 / 17
         "odd, x0, y0, shifted": (("start", ODD, 3), {}),
         "no rows of A": (("synth", (64, 0, 8), 3), {}),
         "weak diagonal": (("weak", SMALL, 3), {})}                           # one instance of three below the 1e-6 of sp_choose_ordering
_cache = {}


def instances_of(key):
    """the instances of a case and their moved twins, made once"""
    if key not in _cache:
        (kind, shape, B), _ = CASES[key]
        if kind == "circle":
            ds = circle_instances(B)
            ds2 = [dict(d, g=d["g"] * (1.0 + 0.02 * np.random.default_rng(300 + b).standard_normal(d["nV"]))) for b, d in enumerate(ds)]
        else:
            ds = instances(shape, B)
            n, nC, nK = shape
            if kind == "start":
                rng = np.random.default_rng(11)
                ds = [dict(d, x0=rng.uniform(-0.1, 0.1, n), y0=rng.uniform(-0.1, 0.1, nC + 2 * nK), lbL=rng.uniform(-0.2, 0.0, nK),
                           lbR=rng.uniform(-0.2, 0.0, nK), ubL=rng.uniform(5.0, 6.0, nK)) for d in ds]
            if kind == "weak":      # variable 5 of instance 1 leaves the Hessian but for a tiny diagonal: a principal submatrix stays definite
                Q = ds[1]["Q"].copy()      # (the zeros stay stored: one pattern for the batch)
                col = np.repeat(np.arange(n), np.diff(Q.indptr))
                Q.data[(Q.indices == 5) | (col == 5)] = 0.0
                Q.data[(Q.indices == 5) & (col == 5)] = 1e-8
                ds[1] = dict(ds[1], Q=Q)
            ds2 = [moved(d, 300 + b) for b, d in enumerate(ds)]
        _cache[key] = (ds, ds2)
    return _cache[key]


def make(hip, key, B=None, trace=False):
    ds, _ = instances_of(key)
    d = ds[0]
    with environment(CASES[key][1]):
        return hip.SparseBatchLCQP(B or len(ds), d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(storeSteps=1 if trace else 0, **OPT))


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def values(ds):
    return np.stack([d["Q"].data for d in ds]), np.stack([d["E"].data for d in ds])


def load_host(sb, ds, first=0, **over):
    Qx, Ax = values(ds)
    rc = sb.load(first, len(ds), Qx, stack(ds, "g"), Ax, **dict(vectors(sb.load, ds), **over))
    assert rc == 0, (rc, sb._last_error())


def load_dev(sb, ds, first=0, only=("Qx", "Ax"), shared=(), **over):
    Qx, Ax = values(ds)
    v = dict(Qx=Qx[0] if "Qx" in shared else Qx, Ax=Ax[0] if "Ax" in shared else Ax)
    kw = dict(vectors(sb.load, ds), **over)
    rc = sb.load_device(first, len(ds), dev(v["Qx"]) if "Qx" in only else None, dev(stack(ds, "g")), dev(v["Ax"]) if "Ax" in only else None,
                        **{k: dev(a) for k, a in kw.items()})
    assert rc == 0, (rc, sb._last_error())


def update_host(sb, ds, first=0):
    rc = sb.update(first, len(ds), stack(ds, "g"), **vectors(sb.update, ds))
    assert rc == 0, (rc, sb._last_error())


def update_dev(sb, ds, first=0):
    rc = sb.update_device(first, len(ds), dev(stack(ds, "g")), **{k: dev(a) for k, a in vectors(sb.update, ds).items()})
    assert rc == 0, (rc, sb._last_error())


def bits(a, b):
    """the same shape and the same bytes (NaNs and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def problem(sb):
    return [sb.read_problem(b) for b in range(sb.B)]


def same_problem(pa, pb):
    assert len(pa) == len(pb)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert set(a) == set(b)
        for k in a:
            assert (a[k] == b[k]) if k == "hasY0" else bits(a[k], b[k]), (i, k)


def result(sb, trace=False):
    x, y, st = sb.solution()
    out = dict(x=x, y=y, st=st)
    if trace:
        out["trace"] = [sb.trace(b) for b in range(sb.B)]
    return out


def same_stats(sa, sb):
    """two lists of statistics dicts, field by field (a NaN equals itself here)"""
    key = lambda st: [(k, np.float64(v).tobytes()) for s in st for k, v in s.items()]
    return key(sa) == key(sb)


def same_result(a, b):
    assert bits(a["x"], b["x"]) and bits(a["y"], b["y"])
    assert same_stats(a["st"], b["st"]), (a["st"], b["st"])
    if "trace" in a:
        for (sa, xa), (sb_, xb) in zip(a["trace"], b["trace"]):
            assert bits(sa, sb_) and bits(xa, xb)
        assert all(len(t[0]) == s["iterTotal"] for t, s in zip(a["trace"], a["st"]))


def solved_pair(hip, key):
    """two handles with the same data, the first loaded from the host, the second from the device; both solved"""
    ds, _ = instances_of(key)
    a, b = make(hip, key), make(hip, key)
    load_host(a, ds); load_dev(b, ds)
    a.run(); b.run()
    return a, b


# ---- the cases: every engine, the ragged sizes, an odd nnzQ, a diagonal that flips the ordering --------------------------------------------
def test_the_cases_cover_the_ground(hip):
    odd = [k for k, ((_, _, B), _) in CASES.items() if instances_of(k)[0][0]["Q"].nnz % 2 == 1 and B >= 2]
    assert odd, "no case has an odd nnzQ with B >= 2"
    ratios = {}
    for key in ("weak diagonal", "bordered circle", "small"):
        dg = [d["Q"].diagonal() for d in instances_of(key)[0]]
        ratios[key] = [float(q.min() / np.abs(q).max()) if q.min() > 0 else 0.0 for q in dg]
    print("  odd nnzQ:", odd, " diagonal ratios:", ratios)
    assert min(ratios["weak diagonal"]) < 1e-6 <= max(ratios["weak diagonal"])      # some instance, not all
    assert max(ratios["bordered circle"]) < 1e-6 and min(ratios["small"]) >= 1e-6
    eng = {}
    for key in CASES:
        ds, _ = instances_of(key)
        a, b = make(hip, key), make(hip, key)
        before = a.ordering()
        load_host(a, ds); load_dev(b, ds)
        eng[key] = dict(lanes=a.lanes(), fronts=a.fronts(), border=a.border(), flipped=not np.array_equal(before, a.ordering()))
        # the ratio computed on the device selects the ordering (and with it the light regularisation) the host's selects
        assert np.array_equal(a.ordering(), b.ordering()) and a.lanes() == b.lanes(), key
        a.close(); b.close()
    print(" ", eng)
    assert eng["small"]["lanes"] == 8 and eng["lanes 32"]["lanes"] == 32
    assert eng["general ldl"]["fronts"] > 0 and eng["bordered circle"]["border"] > 0
    # a batch of definite Hessians moves to the second ordering at its load; one weak diagonal in the batch keeps the first
    assert eng["small"]["flipped"] and not eng["weak diagonal"]["flipped"]


# ---- 1: load_device leaves what load leaves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_load_device_equals_load(hip, key):
    ds, _ = instances_of(key)
    a, b = make(hip, key, trace=True), make(hip, key, trace=True)
    load_host(a, ds); load_dev(b, ds)
    same_problem(problem(a), problem(b))
    a.run(); b.run()
    same_result(result(a, trace=True), result(b, trace=True))
    assert a.algorithmic_bytes() == b.algorithmic_bytes() > 0
    assert np.array_equal(a.ordering(), b.ordering())
    same_problem(problem(a), problem(b))
    a.close(); b.close()


# ---- 2, 3, 4: shared arrays, NULL arrays, a sub-range ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ("small", "odd, x0, y0, shifted"))
@pytest.mark.parametrize("shared", (("Qx", "Ax"), ("Qx",), ("Ax",)))
def test_shared_values_are_broadcast(hip, key, shared):
    ds, _ = instances_of(key)
    ds = [dict(d, **{m: ds[0][m] for m, v in (("Q", "Qx"), ("E", "Ax")) if v in shared}) for d in ds]
    a, b = make(hip, key), make(hip, key)
    load_host(a, ds); load_dev(b, ds, shared=shared)
    same_problem(problem(a), problem(b))
    a.run(); b.run()
    same_result(result(a), result(b))
    assert np.array_equal(a.ordering(), b.ordering())
    a.close(); b.close()


@pytest.mark.parametrize("key", ("small", "odd, x0, y0, shifted"))
def test_null_values_keep_what_the_batch_holds(hip, key):
    ds, _ = instances_of(key)

    def scaled(d, m, f):
        M = d[m].copy(); M.data = M.data * f
        return dict(d, **{m: M})
    for m, only, f in (("Q", ("Qx",), 1.25), ("E", ("Ax",), 1.01)):
        ds2 = [scaled(d, m, f) for d in ds]
        a, b = make(hip, key), make(hip, key)
        load_host(a, ds2)
        load_host(b, ds); b.run()                 # (a solved batch: its pools hold what a run leaves)
        load_dev(b, ds2, only=only)
        same_problem(problem(a), problem(b))
        a.run(); b.run()
        same_result(result(a), result(b))
        assert a.launch_counts()[0] + 1 == b.launch_counts()[0] == 2      # the load cleared the setup mark
        a.close(); b.close()
    c = make(hip, key)                            # nothing to keep: the host twin's code for a missing matrix
    Qx, Ax = (dev(v) for v in values(ds))
    g = dev(stack(ds, "g"))
    assert c.load_device(0, c.B, None, g, Ax) == 100
    assert c.load_device(0, c.B, Qx, g, None) == 100
    assert c.load_device(0, c.B, Qx, None, Ax) == 116
    assert c.load_device(0, c.B, Qx, g, Ax) == 0
    assert c.load_device(0, c.B, None, g, None) == 0
    c.close()


@pytest.mark.parametrize("key", ("small", "odd, x0, y0, shifted"))
def test_sub_range_after_a_host_load(hip, key):
    ds, _ = instances_of(key)
    a, b = make(hip, key), make(hip, key)
    load_host(a, ds)
    load_host(b, ds[:1]); load_dev(b, ds[1:], first=1)
    same_problem(problem(a), problem(b))
    a.run(); b.run()
    same_result(result(a), result(b))
    a.close(); b.close()


@pytest.mark.parametrize("second", ("adds lbL", "starts over"))
def test_lbl_flags_follow_the_rule_of_the_host(hip, second):
    """lbL / lbR given to only one of two loads: a later load behind instance 0 adds to the batch-wide flags, one at instance 0 starts them over"""
    key = "odd, x0, y0, shifted"
    ds, _ = instances_of(key)
    a, b = make(hip, key), make(hip, key)
    if second == "adds lbL":
        for sb, again in ((a, load_host), (b, load_dev)):
            load_host(sb, ds, lbL=None, lbR=None)
            again(sb, ds[1:], first=1)
    else:
        for sb, again in ((a, load_host), (b, load_dev)):
            load_host(sb, ds)
            again(sb, ds[:1], first=0, lbL=None, lbR=None)
    same_problem(problem(a), problem(b))
    a.run(); b.run()
    same_result(result(a), result(b))
    a.close(); b.close()


# ---- 5: update_device, and the two paths mixed on one handle --------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_update_device_equals_update(hip, key):
    ds, ds2 = instances_of(key)
    a, b = solved_pair(hip, key)
    same_result(result(a), result(b))
    #            vectors, warm, how b is updated: host and device updates alternate on one handle
    for step, (vs, warm, upd) in enumerate(((ds2, False, update_dev), (ds, True, update_host), (ds2, True, update_dev))):
        update_host(a, vs); upd(b, vs)
        same_problem(problem(a), problem(b))
        a.resolve(warm=warm); b.resolve(warm=warm)
        same_result(result(a), result(b))
        assert a.launch_counts() == b.launch_counts() == (1, 2 + step)
    a.close(); b.close()


# ---- 6: refusals: the code, and pools and a warm re-solve that are what they are without the refused calls ----------------------------------
def test_refusals_change_nothing(hip):
    key = "odd, x0, y0, shifted"
    ds, ds2 = instances_of(key)
    B, n, nK = len(ds), ds[0]["nV"], ds[0]["nComp"]
    nnzQ = ds[0]["Q"].nnz
    a, b = solved_pair(hip, key)
    never = make(hip, key); load_dev(never, ds[:1])      # instances 1 and 2 never loaded, nothing solved
    before = problem(b)
    ordering = b.ordering()
    L = hip.lib()
    g = dev(stack(ds2, "g"))
    Qx, Ax = (dev(v) for v in values(ds2))
    kw = {k: dev(v) for k, v in vectors(b.update, ds2).items()}
    none = [None]

    # host memory: a CPU tensor's address, and pinned memory
    cpu = torch.zeros((B, n), dtype=torch.float64)
    pinned = torch.zeros((B, n), dtype=torch.float64).pin_memory()
    for t in (cpu, pinned):
        assert L.lcqp_hip_sparse_update_device(b.h, 0, B, t.data_ptr(), *none * 8, None) == 100 and "g: not a device pointer" in b._last_error()
        assert L.lcqp_hip_sparse_load_device(b.h, 0, B, 0, None, t.data_ptr(), None, *none * 8, None) == 100 and "g: not a device pointer" in b._last_error()
    cpuQ = torch.zeros((B, nnzQ), dtype=torch.float64)
    assert L.lcqp_hip_sparse_load_device(b.h, 0, B, 0, cpuQ.data_ptr(), g.data_ptr(), None, *none * 8, None) == 100 and "Qx: not a device pointer" in b._last_error()
    # bits outside 1 | 2 in shared; ranges outside the batch
    assert L.lcqp_hip_sparse_load_device(b.h, 0, B, 4, Qx.data_ptr(), g.data_ptr(), Ax.data_ptr(), *none * 8, None) == 100
    assert L.lcqp_hip_sparse_load_device(b.h, 1, B, 0, Qx.data_ptr(), g.data_ptr(), Ax.data_ptr(), *none * 8, None) == 100
    assert L.lcqp_hip_sparse_load_device(b.h, -1, 1, 0, Qx.data_ptr(), g.data_ptr(), Ax.data_ptr(), *none * 8, None) == 100
    assert L.lcqp_hip_sparse_update_device(b.h, 1, B, g.data_ptr(), *none * 8, None) == 100
    assert L.lcqp_hip_sparse_update_device(b.h, 0, 0, g.data_ptr(), *none * 8, None) == 100
    # an instance never loaded
    assert never.update_device(0, B, g, **kw) == 300
    assert never.load_device(0, B, None, g, None, **kw) == 100
    # -inf in lbL: found on the device before anything is written, and no host state changes -- the setup mark stays
    bad = stack(ds2, "lbL").copy(); bad[B - 1, nK - 1] = -np.inf
    assert b.update_device(0, B, g, **dict(kw, lbL=dev(bad))) == 120
    assert b.load_device(0, B, Qx, g, Ax, **dict(kw, lbL=dev(bad))) == 120
    assert b.load_device(0, B, Qx, g, Ax, **dict(kw, lbR=dev(bad))) == 120
    # a misaligned dQx (a view offset by one double); calls before a solve
    vx = dev(np.ones((B, n)))
    buf = torch.zeros(B * nnzQ + 1, dtype=torch.float64, device="cuda:0")
    with pytest.raises(RuntimeError, match="dQx: not aligned to 16 bytes"):
        b.adjoint_device(vx, matrices=("Q",), out=dict(Q=buf[1:].view(B, nnzQ)))
    assert torch.all(buf == 0.0)
    with pytest.raises(RuntimeError, match="code 300"):
        never.sensitivity_device(vx)
    with pytest.raises(RuntimeError, match="code 300"):
        never.adjoint_device(vx)
    dg = torch.zeros((B, n), dtype=torch.float64, device="cuda:0")
    assert L.lcqp_hip_sparse_adjoint_device(b.h, vx.data_ptr(), None, dg.data_ptr(), None, None, None, 2, None, None, None) == 100
    assert L.lcqp_hip_sparse_sensitivity_device(b.h, 0, vx.data_ptr(), dg.data_ptr(), None, None, None, None) == 100
    assert torch.all(dg == 0.0)

    same_problem(before, problem(b))
    assert np.array_equal(ordering, b.ordering())
    a.resolve(warm=True); b.resolve(warm=True)
    same_result(result(a), result(b))
    assert a.launch_counts() == b.launch_counts() == (1, 2)
    for sb in (a, b, never):
        sb.close()


# ---- 7: the solution and the derivatives, read and written where they lie -------------------------------------------------------------------
def compare_derivatives(hip, sb, V, vy):
    import ctypes
    B = sb.B
    x, y, st = sb.solution()
    xd, yd, sd = sb.solution_device(stats=True)
    assert bits(xd.cpu().numpy(), x) and bits(yd.cpu().numpy(), y)
    raw = sd.cpu().numpy()
    assert raw.shape[1] == ctypes.sizeof(hip.capi.Stats)
    assert same_stats([hip.capi.Stats.from_buffer_copy(raw[b].tobytes()).asdict() for b in range(B)], st)
    x2, y2 = sb.solution_device()
    assert torch.equal(x2, xd) and torch.equal(y2, yd)
    for v in (V[:, 0], V[:, :1], V):      # nrhs = 1 (both shapes) and 3
        want = sb.sensitivity(v)
        got = sb.sensitivity_device(dev(v))
        for w, g_ in zip(want, got):
            assert g_.is_cuda and bits(g_.cpu().numpy(), w)
        assert sb.sensitivity_kernel_ms() > 0
    one = 8 * (sb.nnzQ + sb.nnzA)          # the host side staged at one instance per chunk: its chunking does not change the bits
    out = {}
    for matrices in (("Q", "A"), ("A",), ("Q",), ()):
        for uy in (vy, None):
            for reduce in (False, True):
                want = sb.adjoint(V[:, 0], uy, matrices=matrices, reduce=reduce)
                got = sb.adjoint_device(dev(V[:, 0]), dev(uy), matrices=matrices, reduce=reduce)
                assert set(got) == set(want)
                for k in want:
                    assert got[k].is_cuda and bits(got[k].cpu().numpy(), want[k]), (k, matrices, reduce, uy is None)
                if matrices == ("Q", "A") and uy is not None:
                    small = sb.adjoint(V[:, 0], uy, matrices=matrices, reduce=reduce, _staging_bytes=one)
                    for k in want:
                        assert bits(small[k], want[k]), (k, reduce)
                    out[reduce] = want
        assert sb.sensitivity_kernel_ms() > 0
    return out


@pytest.mark.parametrize("key", list(CASES))
def test_solution_sensitivity_and_adjoint_device(hip, key):
    ds, ds2 = instances_of(key)
    B, n, m = len(ds), ds[0]["nV"], ds[0]["nC"] + 2 * ds[0]["nComp"]
    rng = np.random.default_rng(n)
    V, vy = rng.standard_normal((B, 3, n)), rng.standard_normal((B, m))
    a, b = solved_pair(hip, key)           # a: solved and left alone
    out = compare_derivatives(hip, b, V, vy)
    assert np.any(out[False]["Q"] != 0.0) and np.any(out[True]["A"] != 0.0)
    # a warm re-solve after the calls returns the bits it returns without them
    update_host(a, ds2); update_dev(b, ds2)
    a.resolve(warm=True); b.resolve(warm=True)
    same_result(result(a), result(b))
    assert a.launch_counts() == b.launch_counts()
    a.close(); b.close()


def test_a_failed_instance_contributes_zeros(hip):
    key = "small"
    ds = list(instances_of(key)[0])
    bad = 4
    g = ds[bad]["g"].copy(); g[0] = np.nan      # no trial of this instance's polish is accepted: its run fails (tests/test_gpu_sparse_sensitivity.py)
    ds[bad] = dict(ds[bad], g=g)
    B, n, m = len(ds), ds[0]["nV"], ds[0]["nC"] + 2 * ds[0]["nComp"]
    sb = make(hip, key)
    load_dev(sb, ds)
    sb.run()
    st = sb.solution()[2]
    assert st[bad]["returnValue"] != 0 and all(st[b]["returnValue"] == 0 for b in range(B) if b != bad)
    rng = np.random.default_rng(n)
    V, vy = rng.standard_normal((B, 3, n)), rng.standard_normal((B, m))
    out = compare_derivatives(hip, sb, V, vy)
    r = sb.adjoint_device(dev(V[:, 0]), dev(vy))
    assert int(r["info"][bad]) & 1
    for k in ("dg", "db", "side", "Q", "A"):
        assert not torch.any(r[k][bad] != 0) and torch.any(r[k][bad - 1] != 0), k
    # the sums over the batch are the sums without the failed instance: its terms are exact zeros
    others = [b for b in range(B) if b != bad]
    for k in ("Q", "A"):
        s = np.zeros_like(out[False][k][0])
        for b in range(B):
            s = s + out[False][k][b]
        assert bits(s, out[True][k]) and np.all(out[False][k][bad] == 0.0) and np.any(out[False][k][others] != 0.0), k
    sb.close()


# ---- 8: stream order: nothing between the producer of g, the library and the consumer of x but the streams -----------------------------------
def test_stream_order(hip):
    key = "mid"
    ds, ds2 = instances_of(key)
    B = len(ds)
    a, b = solved_pair(hip, key)
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
    update_host(a, ds2)
    a.resolve(warm=True)
    xa, ya, _ = a.solution()
    assert bits(x.cpu().numpy(), xa) and bits(y.cpu().numpy(), ya)
    assert bits(total.cpu().numpy(), dev(xa).sum(dim=1).cpu().numpy())      # (the same reduction kernel on the same bits)
    same_result(result(a), result(b))
    a.close(); b.close()


# ---- 9: the torch layer: the same bits from tensors on the device and from CPU tensors -------------------------------------------------------
def test_layer_device_path(hip):
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    key = "odd, x0, y0, shifted"
    ds, ds2 = instances_of(key)
    ds = [{k: v for k, v in d.items() if k not in ("x0", "y0")} for d in ds]
    B, n, nC, nK = len(ds), ds[0]["nV"], ds[0]["nC"], ds[0]["nComp"]
    m = nC + 2 * nK
    Qx, Ax = values(ds)
    a, b = make(hip, key), make(hip, key)
    load_host(a, ds); load_host(b, ds)
    bounds = {k: v for k, v in vectors(a.update, ds).items() if v is not None}
    la, lb_ = (SparseBatchLCQPLayer(sb, bounds=bounds, values=dict(Qx=Qx, Ax=Ax)) for sb in (a, b))
    rng = np.random.default_rng(3)
    wx, wy = rng.standard_normal((B, n)), rng.standard_normal((B, m))

    def leaves(where, **arrays):
        return {k: torch.tensor(v, dtype=torch.float64, device=where, requires_grad=True) for k, v in arrays.items()}

    def loss(x, y, where):
        return (x * torch.as_tensor(wx, device=where)).sum() + (y * torch.as_tensor(wy, device=where)).sum()

    def run(layer, where):
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            t = leaves(where, g=stack(ds, "g"), lbA=stack(ds, "lbA"))
            x = layer(t["g"], t["lbA"])
            (x * torch.as_tensor(wx, device=where)).sum().backward()
            out += [x, t["g"].grad, t["lbA"].grad]
            # a shared Qx (its gradient: the sum over the batch, formed on the device), one Ax per instance
            t = leaves(where, g=stack(ds2, "g"), Qx=Qx[0] * 1.1, Ax=Ax * 1.01, lbA=stack(ds2, "lbA"))
            x, y = layer.solve(t["g"], Qx=t["Qx"], Ax=t["Ax"], lbA=t["lbA"])
            loss(x, y, where).backward()
            out += [x, y] + [t[k].grad for k in ("g", "Qx", "Ax", "lbA")]
            t = leaves(where, g=stack(ds, "g"))      # the matrices of the load above stay: update + warm resolve
            x, y = layer.solve(t["g"])
            loss(x, y, where).backward()
            out += [x, y, t["g"].grad]
        return out

    host = run(la, "cpu")
    assert la.last_path == "host"
    device = run(lb_, "cuda:0")
    assert lb_.last_path == "device"
    assert len(host) == len(device) == 12
    for i, (h, d) in enumerate(zip(host, device)):
        assert d.is_cuda and d.shape == h.shape and bits(d.detach().cpu().numpy(), h.detach().numpy()), i
    assert lb_.y.is_cuda and lb_.info.is_cuda
    assert same_stats(lb_.stats, la.stats)
    assert a.launch_counts() == b.launch_counts()
    # CPU tensors on the layer that ran on the device: the host path, with the value arrays read back from the batch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        outs = []
        for layer in (la, lb_):
            t = leaves("cpu", g=stack(ds2, "g"), Ax=Ax * 0.99)
            x, y = layer.solve(t["g"], Ax=t["Ax"])
            loss(x, y, "cpu").backward()
            outs.append([x, y, t["g"].grad, t["Ax"].grad])
    assert lb_.last_path == "host" and not outs[1][0].is_cuda
    for h, d in zip(*outs):
        assert bits(d.detach().numpy(), h.detach().numpy())
    a.close(); b.close()


def test_layer_device_path_equality_rows_and_flagged_instances(hip):
    """both bounds of an equality row as inputs (each gets half of the row's derivative) and the one warning about flagged instances,
    through layer(g, lbA, ubA) and through layer.solve(g, lbA=, ubA=): the same bits and the same warning from both paths"""
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    key = "small"
    ds, _ = instances_of(key)
    B, n, nC, nK = len(ds), ds[0]["nV"], ds[0]["nC"], ds[0]["nComp"]
    a, b = make(hip, key), make(hip, key)
    load_host(a, ds); load_host(b, ds)
    lo, hi = stack(ds, "lbA").copy(), stack(ds, "ubA").copy()
    lo[:, 0] = hi[:, 0] = 0.5 * (lo[:, 0] + hi[:, 0])      # row 0 of every instance: an equality inside the old range
    gs = stack(ds, "g").copy(); gs[1, 0] = np.nan           # instance 1: no trial of its polish is accepted, the solve fails
    la, lb_ = SparseBatchLCQPLayer(a), SparseBatchLCQPLayer(b)
    rng = np.random.default_rng(4)
    wx, wy = rng.standard_normal((B, n)), rng.standard_normal((B, nC + 2 * nK))

    def run(layer, where):
        out, messages = [], []
        for full in (False, True):
            t = {k: torch.tensor(v, dtype=torch.float64, device=where, requires_grad=True) for k, v in dict(g=gs, lbA=lo, ubA=hi).items()}
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
    for i, (h, d) in enumerate(zip(host, device)):      # (bits, not torch.equal: what the failed instance returns may hold NaNs)
        assert d.is_cuda and bits(d.detach().cpu().numpy(), h.detach().numpy()), i
    assert said == said_d and len(said) == 2 and all(c is RuntimeWarning for c, _ in said)      # one per backward
    assert said[0][1].startswith(f"LCQPSolveFunction.backward: 1 of {B} instances")
    assert said[1][1].startswith(f"LCQPSparseFullSolveFunction.backward: 1 of {B} instances")
    for x, y, dg, dlo, dhi, info in (host[:6], host[6:]):
        ok = info == 0
        assert ok.tolist() == [i != 1 for i in range(B)] and info[1] & 1
        assert torch.equal(dlo[:, 0], dhi[:, 0]) and torch.all(dlo[ok, 0] != 0)      # the equality row: half to each bound
        assert not torch.any((dlo[:, 1:] != 0) & (dhi[:, 1:] != 0))                # every other row sits on one bound at the most
    a.close(); b.close()
