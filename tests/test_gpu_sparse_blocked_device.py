"""The device-pointer twins of the sparse arm's four panel calls (lcqp_hip_sparse_sensitivity_blocked_device, _adjoint_blocked_device,
_jacobian_device, _jacobian_duals_device; DESIGN.md section 3a''''', "The sparse arm: panels and Jacobians into device arrays") against their
oracle, the host twins: every comparison is bit for bit, so there is no tolerance anywhere in this file.

1  the blocked calls       2  the Jacobians: the whole batch, a sub-range, bounds=False, three staging caps       3  guard rows around the
Jacobians, exact zeros outside W       4  host, device, host on one handle       5  cold and warm re-solves after the calls
6  stream order            7  refusals       8  a failed instance       9  the kernel time       10  the torch layer

One solve per case (solved_case) serves checks 1 - 4 and 9.  The shapes are the smallest at which k_sparse_scatter_panels can go wrong: a
ragged last panel in the blocked calls of every case (nrhs = 2 P + 3) and in both Jacobians of the circle (nV = 202: 2 columns, m = 301: 5
columns), more than one pool, every lane width's panel kernel, the general LDL' with its panel form and without (the fallback)."""
import torch      # noqa: F401 -- before the library is first loaded: the library and torch must share one HIP runtime (lcqpow_amd.capi.lib)

import functools

import numpy as np
import pytest

from batch_helpers import assert_same_bits, environment, handle, result, update_all
from problems import OPT, SMALL, instances, moved
from test_gpu_sparse_sensitivity import CASES as VECTOR_CASES, instances_of

pytestmark = pytest.mark.gpu

NOT_SETUP, INVALID_ARGUMENT = 300, 100
NRHS = 19                  # 2 P + 3 with the panel width P = 8 of every engine: two full panels and a ragged one
SENTINEL = -1234.5
FALLBACK, GENERAL_PANEL = "small, general ldl", "small, general ldl, panel"
#        case of tests/test_gpu_sparse_sensitivity.py, set_general_panel
CASES = {"small": ("small", False), "pools of 4": ("pools of 4", False), "lanes 32": ("lanes 32", False),
         "bordered circle": ("bordered circle", False), GENERAL_PANEL: ("small, general ldl", True), FALLBACK: ("small, general ldl", False)}
JAC = ("jacobian", "jacobian_duals")


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def host(t):
    """the tensors of a device twin's result on the host (None stays None)"""
    return tuple(None if x is None else x.cpu().numpy() for x in t)


def bits(a, b):
    """two results, entry by entry: the same shape, type and bytes (NaNs and signed zeros included); None equals None"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x is None or y is None:
            if x is not y:
                return False
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return True


def make(hip, key, ds=None):
    base, switch = CASES[key]
    with environment(VECTOR_CASES[base][1]):
        sb = handle(hip, ds or instances_of(base), hip.default_options(**OPT))
    if switch:
        sb.set_general_panel(True)
    return sb


def inputs(B, n, m):
    rng = np.random.default_rng(83)
    V, VY = rng.standard_normal((B, NRHS, n)), rng.standard_normal((B, NRHS, m))
    V[:, 5] = 0.0; VY[:, 5] = 0.0      # a zero column
    return V, VY


def item_bytes(P, n, m, dunit):
    """the staging of one (instance, panel) work item: its outputs, its workspace (sens_blk_ws_doubles) and, for the dual Jacobian, its row map"""
    Np = (n + m + 63) // 64 * 64
    return 8 * (P * (n + m) + P * (Np + 2 * n + m)) + (4 * P if dunit else 0)


def caps(P, n, m, count, dunit):
    """the three staging caps of check 2 with the chunks they give: the default (one chunk), one work item per launch, a partial last chunk"""
    if not P:
        return {"default": None, "one": 1, "partial": 8 * 6 * 2 * (n + m) * 5}      # the fallback goes in chunks of columns
    items = count * (-(-(m if dunit else n) // P))
    per = max(2, (items + 2) // 3 + 1)
    assert per < items and items % per != 0, (items, per)      # more than one chunk, the last one partial
    return {"default": None, "one": 1, "partial": item_bytes(P, n, m, dunit) * per}


@functools.lru_cache(maxsize=None)
def solved_case(key):
    """one solve per case: every host call and its device twin that checks 1 - 4 and 9 compare, as numpy"""
    import lcqpow_amd as hip
    sb = make(hip, key)
    B, n, m, P = sb.B, sb.nV, sb.m, sb.sens_panel()
    c = dict(B=B, n=n, m=m, P=P, engine=dict(lanes=sb.lanes(), fronts=sb.fronts(), border=sb.border(), pools=VECTOR_CASES[CASES[key][0]][1]))
    sb.run()
    c["st"] = sb.solution()[2]
    counts = sb.launch_counts()
    V, VY = inputs(B, n, m)
    ms = {}
    # 1: the blocked calls
    c["sens"] = (sb.sensitivity_blocked(V), host(sb.sensitivity_blocked_device(dev(V))))
    ms["sensitivity_blocked_device"] = sb.sensitivity_kernel_ms()
    c["adj"] = {}
    for name, vx, vy in (("VX, VY", V, VY), ("VX, None", V, None), ("None, VY", None, VY)):
        c["adj"][name] = (sb.adjoint_blocked(vx, vy), host(sb.adjoint_blocked_device(dev(vx), dev(vy))))
        ms["adjoint_blocked_device " + name] = sb.sensitivity_kernel_ms()
    # 2: the Jacobians
    sub = (1, 2) if B >= 3 else (1, 1)
    for name in JAC:
        hostcall, twin = getattr(sb, name), getattr(sb, name + "_device")
        r = c[name] = {}
        r["whole"] = (hostcall(), host(twin()))
        ms[name + "_device"] = sb.sensitivity_kernel_ms()
        r["range"] = (hostcall(first=sub[0], count=sub[1]), host(twin(first=sub[0], count=sub[1])))
        r["nobounds"] = (hostcall(bounds=False), host(twin(bounds=False)))
        for cap, nbytes in caps(P, n, m, B, name == "jacobian_duals").items():
            with sb._staging(nbytes):
                got = host(twin())
                ms[name + "_device, cap " + cap] = sb.sensitivity_kernel_ms()
            r["cap " + cap] = (hostcall(_staging_bytes=nbytes), got)
        # 4: host, device, host
        r["again"] = hostcall()
    c["ms"] = ms
    assert sb.launch_counts() == counts
    sb.close()
    return c


def test_the_cases_reach_every_engine(hip):
    eng = {k: dict(solved_case(k)["engine"], P=solved_case(k)["P"], n=solved_case(k)["n"], m=solved_case(k)["m"]) for k in CASES}
    print(" ", eng)
    assert eng["small"]["lanes"] == 8 and eng["lanes 32"]["lanes"] == 32 and eng["bordered circle"]["border"] > 0
    assert eng[GENERAL_PANEL]["fronts"] > 0 and eng[GENERAL_PANEL]["P"] == 8 and eng[FALLBACK]["fronts"] > 0 and eng[FALLBACK]["P"] == 0
    assert all(e["P"] == 8 for k, e in eng.items() if k != FALLBACK)      # NRHS = 2 P + 3
    c = eng["bordered circle"]
    assert (c["n"], c["m"], c["n"] % 8, c["m"] % 8) == (202, 301, 2, 5)      # both Jacobians end in a ragged panel


# ---- 1: the blocked calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_blocked_calls_equal_the_host_twins(hip, key):
    c = solved_case(key)
    want, got = c["sens"]
    assert bits(want, got) and np.any(want[0] != 0.0) and np.all(want[0][:, 5] == 0.0)
    for name, (want, got) in c["adj"].items():
        assert bits(want, got), name
        assert np.any(want[0] != 0.0), name
    assert bits(c["adj"]["VX, None"][1], c["sens"][1])      # vy == NULL: the blocked sensitivity call itself


# ---- 2: the Jacobians -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", JAC)
@pytest.mark.parametrize("key", list(CASES))
def test_jacobians_equal_the_host_twins(hip, key, name):
    c = solved_case(key)
    r = c[name]
    for what in ("whole", "range", "nobounds", "cap default", "cap one", "cap partial"):
        want, got = r[what]
        assert bits(want, got), what
    assert r["nobounds"][1][1] is None
    whole = r["whole"][1]
    assert np.any(whole[0] != 0.0) and np.any(whole[1] != 0.0)
    for what in ("cap default", "cap one", "cap partial"):      # the chunking does not change the bits
        assert bits(r[what][1], whole), what
    lo, cnt = (1, 2) if c["B"] >= 3 else (1, 1)
    assert bits(r["range"][1], tuple(a[lo:lo + cnt] for a in whole))
    if name == "jacobian_duals" and key == "small":
        # a working set that is not a prefix of the rows: a row map of k in place of rowpos cannot pass
        W = [np.flatnonzero(s) for s in whole[2]]
        print("  |W| per instance:", [len(w) for w in W])
        assert any(len(w) and not np.array_equal(w, np.arange(len(w))) for w in W)


# ---- 3: guard rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_guard_rows_keep_their_bits(hip, key):
    """the two Jacobian twins through the C ABI, into the middle of tensors filled with a sentinel: a guard of 2 P rows of the widest row
    length in front of and behind each block holds its bits, and the rows of Jyg / Jyb outside W are exact zeros"""
    c = solved_case(key)
    B, n, m = c["B"], c["n"], c["m"]
    sb = make(hip, key)
    sb.run()
    L = hip.lib()
    guard = 2 * 8 * max(n, m)      # doubles
    stream = torch.cuda.current_stream(0).cuda_stream
    for name, rows in (("jacobian", n), ("jacobian_duals", m)):
        bufs = [torch.full((guard + B * rows * w + guard,), SENTINEL, dtype=torch.float64, device="cuda:0") for w in (n, m)]
        side = torch.full((B, m), 77, dtype=torch.int32, device="cuda:0"); info = torch.full((B,), 77, dtype=torch.int32, device="cuda:0")
        rc = getattr(L, "lcqp_hip_sparse_" + name + "_device")(sb.h, 0, B, bufs[0].data_ptr() + 8 * guard, bufs[1].data_ptr() + 8 * guard,
                                                               side.data_ptr(), info.data_ptr(), stream)
        assert rc == 0, (rc, sb._last_error())
        torch.cuda.synchronize()
        want = c[name]["whole"][0]
        for buf, w, ref in zip(bufs, (n, m), want[:2]):
            h = buf.cpu().numpy()
            front, inner, back = h[:guard], h[guard:guard + B * rows * w].reshape(B, rows, w), h[guard + B * rows * w:]
            bad = int(np.count_nonzero(front != SENTINEL)), int(np.count_nonzero(back != SENTINEL))
            print(f"  {key} {name} width {w}: guard doubles overwritten in front {bad[0]}, behind {bad[1]}")
            assert bad == (0, 0)
            assert bits((inner,), (ref,)) and not np.any(inner == SENTINEL)
            if name == "jacobian_duals":
                outside = want[2] == 0
                assert outside.any() and np.all(inner[outside] == 0.0) and not np.any(np.signbit(inner[outside]))
        assert bits((side.cpu().numpy(), info.cpu().numpy()), want[2:])
    sb.close()


# ---- 4: host, device, host on one handle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_host_and_device_calls_alternate(hip, key):
    c = solved_case(key)
    for name in JAC:      # (solved_case: whole on the host, the twins under every cap, then the host call again)
        assert bits(c[name]["whole"][0], c[name]["again"]), name
    sb = make(hip, key)
    sb.run()
    V, VY = inputs(c["B"], c["n"], c["m"])
    first = sb.adjoint_blocked(V, VY)
    assert bits(host(sb.adjoint_blocked_device(dev(V), dev(VY))), first)
    assert bits(sb.adjoint_blocked(V, VY), first) and bits(first, c["adj"]["VX, VY"][0])
    assert bits(host(sb.jacobian_duals_device()), c["jacobian_duals"]["whole"][0])
    assert bits(sb.sensitivity_blocked(V), c["sens"][0])
    sb.close()


# ---- 5: the calls change nothing a re-solve reads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["small", "bordered circle"])
def test_resolves_after_the_calls(hip, key):
    ds = instances_of(CASES[key][0])
    if key == "bordered circle":
        ds2 = [dict(d, g=d["g"] * (1.0 + 0.02 * np.random.default_rng(300 + b).standard_normal(d["nV"]))) for b, d in enumerate(ds)]
    else:
        ds2 = [moved(d, 300 + b) for b, d in enumerate(ds)]
    out = []
    for with_calls in (True, False):
        sb = make(hip, key)
        sb.run()
        first = result(sb)
        if with_calls:
            counts = sb.launch_counts()
            V, VY = inputs(sb.B, sb.nV, sb.m)
            assert torch.any(sb.sensitivity_blocked_device(dev(V))[0] != 0.0) and torch.any(sb.adjoint_blocked_device(dev(V), dev(VY))[0] != 0.0)
            assert torch.any(sb.jacobian_device()[0] != 0.0) and torch.any(sb.jacobian_duals_device()[0] != 0.0)
            assert sb.launch_counts() == counts
            assert_same_bits(first, result(sb))
        update_all(sb, ds2)
        sb.resolve(warm=False)
        cold = result(sb)
        update_all(sb, ds)
        sb.resolve(warm=True)
        out.append((cold, result(sb), sb.launch_counts()))
        sb.close()
    assert_same_bits(out[0][0], out[1][0]); assert_same_bits(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] == (1, 3)


# ---- 6: stream order ------------------------------------------------------------------------------------------------------------------------
def test_stream_order(hip):
    """inputs produced, the twin called and its outputs consumed on a side stream, with nothing between the three but the stream"""
    c = solved_case("small")
    sb = make(hip, "small")
    sb.run()
    V, VY = inputs(c["B"], c["n"], c["m"])
    Vd, VYd = dev(V), dev(VY)
    big = torch.ones((4096, 4096), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        one = ((big @ big)[0, 0] / 4096.0).to(torch.float64)      # 1.0, behind a matrix product that takes the device a while
        vx, vy = Vd * one, VYd * one
        sens = sb.sensitivity_blocked_device(vx)
        adj = sb.adjoint_blocked_device(vx, vy)
        jac = sb.jacobian_device()
        jd = sb.jacobian_duals_device()
        sums = [t[0].sum(dim=-1) + t[1].sum(dim=-1) for t in (sens, adj, jac, jd)]
    s.synchronize()
    for got, want, total in zip((sens, adj, jac, jd), (c["sens"][0], c["adj"]["VX, VY"][0], c["jacobian"]["whole"][0], c["jacobian_duals"]["whole"][0]), sums):
        assert bits(host(got), want)
        assert bits((total.cpu().numpy(),), ((dev(want[0]).sum(dim=-1) + dev(want[1]).sum(dim=-1)).cpu().numpy(),))      # (the same kernels on the same bits)
    sb.close()


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    L = hip.lib()
    ds = instances(SMALL, 2)
    B, n, m = 2, SMALL[0], SMALL[1] + 2 * SMALL[2]
    d = ds[0]
    sb = hip.SparseBatchLCQP(B, d["nV"], d["nC"], d["nComp"], d["Q"], d["E"], opt=hip.default_options(**OPT))
    load = lambda: sb.load(0, B, np.stack([q["Q"].data for q in ds]), np.stack([q["g"] for q in ds]), np.stack([q["E"].data for q in ds]),
                           lbA=np.stack([q["lbA"] for q in ds]), ubA=np.stack([q["ubA"] for q in ds]))
    fill = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda:0")
    # (every array one double per row longer than the call needs: a pointer 4 bytes in still has the bytes behind it, so it is refused for its alignment)
    vx, vy = dev(np.ones((B, 2, n))), dev(np.ones((B, 2, m)))
    out = dict(dg=fill(B, 2, n + 1), db=fill(B, 2, m + 1), Jg=fill(B, n, n + 1), Jb=fill(B, n, m + 1), Jyg=fill(B, m, n + 1), Jyb=fill(B, m, m + 1))
    side = torch.full((B, m), 77, dtype=torch.int32, device="cuda:0"); info = torch.full((B,), 77, dtype=torch.int32, device="cuda:0")
    p = {k: t.data_ptr() for k, t in out.items()}
    p.update(vx=vx.data_ptr(), vy=vy.data_ptr(), side=side.data_ptr(), info=info.data_ptr())
    # each call as a function of its data pointers, by the names of include/lcqp_hip.h
    calls = {
        "sensitivity_blocked": (("v", "dg", "db"), lambda q, nrhs=2: L.lcqp_hip_sparse_sensitivity_blocked_device(sb.h, nrhs, q["v"], q["dg"], q["db"], p["side"], p["info"], None)),
        "adjoint_blocked": (("vx", "vy", "dg", "db"), lambda q, nrhs=2: L.lcqp_hip_sparse_adjoint_blocked_device(sb.h, nrhs, q["vx"], q["vy"], q["dg"], q["db"], p["side"], p["info"], None)),
        "jacobian": (("Jg", "Jb"), lambda q, first=0, count=B: L.lcqp_hip_sparse_jacobian_device(sb.h, first, count, q["Jg"], q["Jb"], p["side"], p["info"], None)),
        "jacobian_duals": (("Jyg", "Jyb"), lambda q, first=0, count=B: L.lcqp_hip_sparse_jacobian_duals_device(sb.h, first, count, q["Jyg"], q["Jyb"], p["side"], p["info"], None)),
    }
    good = dict(p, v=p["vx"])
    untouched = lambda: all(bool(torch.all(t == SENTINEL)) for t in out.values()) and bool(torch.all(side == 77)) and bool(torch.all(info == 77))

    assert all(call(good) == NOT_SETUP for _, call in calls.values())      # before anything
    assert load() == 0
    assert all(call(good) == NOT_SETUP for _, call in calls.values()) and untouched()      # loaded, not solved
    sb.run()
    pageable = np.full(B * max(n, m) * (max(n, m) + 1), 1.0)
    pinned = torch.ones(B * max(n, m) * (max(n, m) + 1), dtype=torch.float64).pin_memory()
    for name, (args, call) in calls.items():
        for arg in args:
            for what, ptr, says in (("pageable", pageable.ctypes.data, "not a device pointer"), ("pinned", pinned.data_ptr(), "not a device pointer"),
                                    ("off by 4 bytes", good[arg] + 4, "not aligned to 8 bytes")):
                assert call(dict(good, **{arg: ptr})) == INVALID_ARGUMENT, (name, arg, what)
                assert sb._last_error().startswith(arg + ": ") and says in sb._last_error(), (name, arg, what, sb._last_error())
    assert calls["sensitivity_blocked"][1](good, nrhs=0) == INVALID_ARGUMENT and calls["adjoint_blocked"][1](good, nrhs=0) == INVALID_ARGUMENT
    assert calls["sensitivity_blocked"][1](dict(good, v=None)) == INVALID_ARGUMENT and calls["sensitivity_blocked"][1](dict(good, dg=None)) == INVALID_ARGUMENT
    assert calls["adjoint_blocked"][1](dict(good, vx=None, vy=None)) == INVALID_ARGUMENT and calls["adjoint_blocked"][1](dict(good, dg=None)) == INVALID_ARGUMENT
    for name, first in (("jacobian", "Jg"), ("jacobian_duals", "Jyg")):
        call = calls[name][1]
        assert call(good, first=-1, count=1) == INVALID_ARGUMENT and call(good, count=0) == INVALID_ARGUMENT and call(good, count=-2) == INVALID_ARGUMENT
        assert call(good, first=1, count=B) == INVALID_ARGUMENT and call(good, first=2 ** 31 - 1, count=2 ** 31 - 1) == INVALID_ARGUMENT
        assert call(dict(good, **{first: None})) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert untouched()
    # the Python methods: host arrays and the wrong device type are refused before the C call
    with pytest.raises(ValueError, match="expected a torch tensor"):
        sb.sensitivity_blocked_device(np.ones((B, 2, n)))
    with pytest.raises(ValueError, match="expected a torch tensor"):
        sb.adjoint_blocked_device(None, np.ones((B, 2, m)))
    with pytest.raises(ValueError, match="cuda:0"):
        sb.adjoint_blocked_device(torch.ones((B, 2, n), dtype=torch.float64))
    with pytest.raises(ValueError, match="outside the batch"):
        sb.jacobian_device(first=1, count=B)
    # after all the refusals the calls work
    assert all(bool(torch.any(t[0] != 0.0)) for t in (sb.sensitivity_blocked_device(vx), sb.adjoint_blocked_device(None, vy), sb.jacobian_device(), sb.jacobian_duals_device()))
    assert load() == 0                                        # a load since the last solve
    assert all(call(good) == NOT_SETUP for _, call in calls.values())
    with pytest.raises(RuntimeError, match="300"):
        sb.jacobian_duals_device()
    torch.cuda.synchronize()
    assert untouched()
    sb.close()


# ---- 8: a failed instance -------------------------------------------------------------------------------------------------------------------
def test_a_failed_instance_has_zero_rows(hip):
    """Instance 4 gets a NaN in g: its run ends with 203 (tests/test_gpu_sparse_sensitivity.py).  info & 1 and zero rows for it in all four
    outputs, the bits of the clean batch for its neighbours."""
    c = solved_case("small")
    ds = list(instances_of("small"))
    bad = 4
    g = ds[bad]["g"].copy(); g[0] = np.nan
    ds[bad] = dict(ds[bad], g=g)
    sb = make(hip, "small", ds)
    sb.run()
    st = sb.solution()[2]
    V, VY = inputs(c["B"], c["n"], c["m"])
    got = dict(sens=host(sb.sensitivity_blocked_device(dev(V))), adj=host(sb.adjoint_blocked_device(dev(V), dev(VY))),
               jacobian=host(sb.jacobian_device()), jacobian_duals=host(sb.jacobian_duals_device()))
    hosts = dict(sens=sb.sensitivity_blocked(V), adj=sb.adjoint_blocked(V, VY), jacobian=sb.jacobian(), jacobian_duals=sb.jacobian_duals())
    sb.close()
    clean = dict(sens=c["sens"][0], adj=c["adj"]["VX, VY"][0], jacobian=c["jacobian"]["whole"][0], jacobian_duals=c["jacobian_duals"]["whole"][0])
    print("  return values", [s["returnValue"] for s in st], "info", {k: r[3].tolist() for k, r in got.items()})
    assert st[bad]["returnValue"] == 203
    for k, r in got.items():
        assert bits(r, hosts[k]), k
        assert r[3][bad] & 1 and all(np.all(a[bad] == 0) for a in r[:3]), k
        for b in range(len(ds)):
            if b != bad:
                assert st[b]["returnValue"] == 0 and bits(tuple(a[b] for a in r), tuple(a[b] for a in clean[k])), (k, b)


# ---- 9: the kernel time ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_kernel_time(hip, key):
    """> 0 after every twin; after a chunked Jacobian it is the sum over the chunks' panel kernels: printed beside the unchunked figure"""
    ms = solved_case(key)["ms"]
    for k, v in ms.items():
        print(f"  {key}: {k}: {v:.4f} ms")
    assert all(v > 0 for v in ms.values())


# ---- 10: the torch layer --------------------------------------------------------------------------------------------------------------------
def test_torch_layer_jacobian_full_on_the_device(hip):
    from lcqpow_amd.diff import SparseBatchLCQPLayer
    shape, B = SMALL, 3
    n, m = shape[0], shape[1] + 2 * shape[2]
    ds = instances(shape, B)
    stack = lambda k: np.stack([d[k] for d in ds])
    a, b = (handle(hip, ds, hip.default_options(**OPT)) for _ in range(2))
    la, lb_ = (SparseBatchLCQPLayer(sb, bounds=dict(lbA=stack("lbA"), ubA=stack("ubA"))) for sb in (a, b))
    g = torch.tensor(stack("g"), dtype=torch.float64)
    la(g); lb_(g.to("cuda:0"))
    H = la.jacobian_full(serial=la.solves)
    assert la.last_path == "host" and not any(t.is_cuda for t in H.values())
    D = lb_.jacobian_full(serial=lb_.solves)
    assert lb_.last_path == "device" and sorted(D) == sorted(H) == ["info", "side", "xb", "xg", "yb", "yg"]
    for k, shp in (("xg", (B, n, n)), ("xb", (B, n, m)), ("yg", (B, m, n)), ("yb", (B, m, m)), ("side", (B, m)), ("info", (B,))):
        assert D[k].is_cuda and tuple(D[k].shape) == shp and D[k].dtype == H[k].dtype, k
        assert bits((D[k].cpu().numpy(),), (H[k].numpy(),)), k
    assert torch.any(D["yg"] != 0.0) and np.array_equal(np.asarray(lb_.info), np.asarray(la.info))
    assert torch.equal(lb_.jacobian(), D["xg"])      # jacobian() stays: the host call, a tensor like g
    # the same layer with g on the host: the host calls
    with torch.no_grad():
        lb_(g * 1.01)
    assert not lb_.jacobian_full()["yg"].is_cuda and lb_.last_path == "host"
    a.close(); b.close()
