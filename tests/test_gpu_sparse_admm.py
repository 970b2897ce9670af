"""The ADMM rounds of the sparse arm (sp_prepare_vectors, the start of a round in sp_ph_round, sp_admm, the refresh decision of
k_sparse_refresh) read back from the device (lcqp_hip_sparse_read_admm: it launches nothing) and held to tests/sparse_admm_ref.py, a
long-double numpy reference in the reduced form K = Q + sigma I + E' diag(rho) E -- never to the oracle.  A round only proposes a working
set and the polish accepts a point on its true residual, so a wrong relaxation step, a wrong weight or a stale ADMM factor costs rounds and
never shows in x or y.

The polish writes none of xa, ya, za (NV_XA, MV_YA, MV_ZA appear only in sp_admm, sp_qp_begin and sp_ph_round), and with admmFirst = k,
admmHot = 0 and solveZeroPenaltyFirst = 1 the first QP runs k iterations on g itself from the x0, y0 given (ya = -y0) while every later QP
is a hot start on the stored point and runs none.  A polish that fails would be followed by a further round of iterations (on the bordered
circle no polish of the first QP settles: thousands of iterations), so every case but C runs with maxRounds = 1: a failed polish then ends
the solve and the state stays that of the k iterations.  Every case asserts stats.admmIter (k, or k + max(10, 2 k) behind one failed polish).

  A  rhov, sigma, rho, scale and the stacked l, u: bit for bit
  B  xa, ya, za after k = 1, 5, 20 iterations, from zero and from a given x0, y0:
     1e-12 n cond_2(K) k max(1, |xa|, |za|, |ya| / min rho) (rows of ya: times rho_r; the minimum over the rows that carry a multiplier)
  C  the state behind one failed polish (maxTrials = 1, maxRounds = 2): k + max(10, 2 k) iterations without a new start
  D  update() that moves rows between two-sided / equality / free, then a cold resolve(): rhov bit for bit at the new classes, the iterates
     against the reference at the NEW weights (a stale ADMM factor fails here); an update that changes no class: no second
     setup launch (launch_counts; whether k_sparse_refresh refactorises an instance is its own decision, which no counter shows), the
     iterates still hold
  E  a read-back changes nothing: the run behind it returns the bits of a run without it; NOT_SETUP before the first run

tests/test_admm_ref.py holds a float64 run of the device's form (KKT matrix, LDL' without pivoting, no refinement) to 1e-2 of the bounds
of B for every case here.  `python -m pytest tests/test_gpu_sparse_admm.py -m gpu -s` prints every ratio.

Worst error / bound (23 tests, 6 s on an MI355X):
    float64 run of the device's form on the CPU     xa 1.4e-6 (circle; 1.4e-8 elsewhere)   ya 9.7e-8   za 5.6e-8
    MI355X                                          xa 8.6e-7   ya 2.0e-6 (circle)   za 2.1e-8;   A: 0 (exact)
cond_2(K) is 1.0e2 ... 2.1e2 on the synthetic cases and 1.0e5 ... 1.7e5 on the circle, so the bound is 1e-7 ... 4e-5 absolute (7e-4 at the
most: circle, k = 20) against iterates of size 1: a relaxation step with the wrong alpha or a weight that is off by a percent exceeds it by
orders of magnitude.  The small ratios come from the fixed 1e-12 n k against eps = 2e-16, not from the conditioning.

Mutants of the sparse kernel units (scratch builds, loaded through LCQPOW_HIP_LIBRARY; failing tests of this file and of
tests/test_gpu_sparse_products.py, 41 together / of the eight sparse GPU files before them, 282 tests):

    1  alpha applied to xa but not to za in sp_admm            22 (every iterate check: xa, ya, za) / 0
    2  rhoEqMult dropped in sp_prepare_vectors                 22 (rhov, bit for bit) / 6 (the stored ADMM factor against the reference's weights)
    3  DETECT forced to "unchanged" in k_sparse_refresh        4 (the iterates behind update() + resolve() at the new weights, every engine) / 6
    4  the tail loop of g_ell starting at ptr[i] + W + 1       13 (9 of the products file on P3; 4 of this file at span 10 and 18) / 12
    5  sp_Cx2 without the swap of the L and R rows             14 (C v0, C v1 on every pattern, lane group and wavefront) / 13
"""
import functools

import numpy as np
import pytest

import admm_ref as A
import sparse_admm_ref as SR

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _chk(name, err, bound):
    err = np.asarray(err, dtype=LD); bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    worst = float(ratio.max()) if err.size else 0.0
    print(f"    {name}: worst error / bound = {worst:.3e}")
    assert np.isfinite(err).all() and (err <= bound).all(), f"{name}: worst error / bound = {worst:.3e}"
    return worst


@functools.lru_cache(maxsize=None)
def _inst(name):
    return SR.CASES[name][0]()


class Ref:
    """the reference of one instance at given A bounds: weights, cond_2(K) and the states after the kept iteration counts, per start"""

    def __init__(self, d, opt, lbA=None, ubA=None, keep=SR.KS):
        self.d, self.n = d, d["nV"]
        self.Q, self.E = SR.dense(d)
        self.l, self.u = SR.stacked(d, lbA, ubA)
        self.scale = float(np.abs(np.diag(self.Q)).max())
        self.sigma = opt.admmSigma * self.scale
        self.rho = opt.admmRho * self.scale
        self.rhov = SR.rho_vector(opt, self.scale, self.l, self.u)
        self.alpha = opt.admmAlpha
        self.condK = A.cond2(A.K(self.Q, self.E, self.sigma, self.rhov, np.float64))
        self.keep = tuple(keep)
        self._states = {}

    def states(self, given):
        if given not in self._states:
            m = len(self.l)
            x0, y0 = (self.d["x0"], -self.d["y0"]) if given else (np.zeros(self.n), np.zeros(m))
            self._states[given] = SR.admm(self.Q, self.E, self.d["g"], self.l, self.u, self.rhov, self.sigma, self.alpha, x0, y0, max(self.keep), LD, self.keep)
        return self._states[given]


@functools.lru_cache(maxsize=None)
def _refs(name, keep=SR.KS):
    import lcqpow_amd as la
    return [Ref(d, la.default_options(), keep=keep) for d in _inst(name)]


def _handle(hip, monkeypatch, name, given=False, **okw):
    inst = _inst(name)
    for k, v in SR.CASES[name][1].items():
        monkeypatch.setenv(k, v)
    d0 = inst[0]
    opt = hip.default_options(**dict(dict(perturbStep=0, printLevel=0, admmHot=0, solveZeroPenaltyFirst=1, maxRounds=1), **okw))
    sb = hip.SparseBatchLCQP(len(inst), d0["nV"], d0["nC"], d0["nComp"], d0["Q"], d0["E"], opt=opt)
    kw = dict(lbA=np.stack([d["lbA"] for d in inst]), ubA=np.stack([d["ubA"] for d in inst]))
    if given:
        kw.update(x0=np.stack([d["x0"] for d in inst]), y0=np.stack([d["y0"] for d in inst]))
    assert sb.load(0, len(inst), np.stack([d["Q"].data for d in inst]), np.stack([d["g"] for d in inst]), np.stack([d["E"].data for d in inst]), **kw) == 0
    return sb


def check_vectors(ra, ref):
    """A"""
    assert (ra["n"], ra["m"]) == (ref.n, len(ref.l))
    assert ra["scale"] == ref.scale and ra["sigma"] == ref.sigma and ra["rho"] == ref.rho, "scale, sigma, rho"
    assert np.array_equal(ra["l"], ref.l) and np.array_equal(ra["u"], ref.u), "stacked l, u"
    assert np.array_equal(ra["rhov"], ref.rhov), "rhov"


def check_iterates(ra, ref, k, state, tag):
    """B"""
    b, by = SR.iterate_bounds(ref.n, ref.condK, k, *state, ref.rhov, ref.l, ref.u)
    free = SR.free_rows(ref.l, ref.u)
    assert not ra["ya"][free].any()
    return {nm: _chk(f"{tag}k = {k}: {nm}", err, bd) for nm, err, bd in SR.iterate_errors((ra["xa"], ra["ya"], ra["za"]), state, b, by)}


# the engine behind sp_solve, from what the handle reports (the host chooses it by these very numbers): the register band at G = 8 / 16, the
# LDS window at G > 16 on a plain band (as tests/test_gpu_sparse_factor.py tells them apart), the bordered band, the general LDL'
ENGINE = {"small": "reg 8", "small pool 4": "reg 8", "small span 10": "reg 16", "small span 18": "lds", "circle 100": "border",
          "small general": "general", "mid": "reg 8"}


def engine_of(sb):
    if sb.fronts() > 0:
        return "general"
    if sb.border() > 0:
        return "border"
    assert sb.bandwidth() < sb.lanes()
    return "reg %d" % sb.lanes() if sb.lanes() <= 16 else "lds"


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("name", list(SR.CASES))
def test_iterates_after_k_iterations(hip, monkeypatch, name, given):
    """A and B for every engine behind sp_admm: one handle, the batch loaded and run once per k"""
    refs = _refs(name)
    sb = _handle(hip, monkeypatch, name, given)
    assert engine_of(sb) == ENGINE[name], (name, sb.lanes(), sb.bandwidth(), sb.border(), sb.fronts())
    if name == "circle 100":
        assert sb.border() == 3
    with pytest.raises(RuntimeError, match="code 300"):
        sb.read_admm(0)
    for k in SR.KS:
        sb.set_options(hip.default_options(perturbStep=0, printLevel=0, admmHot=0, solveZeroPenaltyFirst=1, maxRounds=1, admmFirst=k))
        sb.run()
        _, _, st = sb.solution()
        for b, ref in enumerate(refs):
            assert st[b]["admmIter"] == k, (name, b, k, st[b])
            ra = sb.read_admm(b)
            check_vectors(ra, ref)
            check_iterates(ra, ref, k, ref.states(given)[k], f"{name} / instance {b} / {'x0, y0' if given else 'zero'} / ")
    sb.close()


@pytest.mark.parametrize("name,k", [("small", 5), ("small span 18", 1), ("circle 100", 5)])
def test_state_behind_one_failed_polish(hip, monkeypatch, name, k):
    """C: maxTrials = 1 ends every polish, maxRounds = 2 allows one more round: k + max(10, 2 k) iterations on the first QP's g, the second
    round continuing from the state of the first (no clip of za, no copy of the start)"""
    total = k + max(10, 2 * k)
    refs = _refs(name, keep=(total,))
    sb = _handle(hip, monkeypatch, name, True, admmFirst=k, maxTrials=1, maxRounds=2)
    sb.run()
    _, _, st = sb.solution()
    for b, ref in enumerate(refs):
        assert st[b]["admmIter"] == total and st[b]["returnValue"] != 0, (name, b, st[b])
        ra = sb.read_admm(b)
        check_vectors(ra, ref)
        check_iterates(ra, ref, total, ref.states(True)[total], f"{name} / instance {b} / two rounds / ")
    sb.close()


@pytest.mark.parametrize("name", ["small", "small span 18", "circle 100", "small general"])
def test_update_that_moves_rows_between_classes(hip, monkeypatch, name):
    """D: the weights and the ADMM factor follow the new classes -- in the instances that were updated and in those that were not"""
    k = 5
    inst = _inst(name)
    old = _refs(name)
    sb = _handle(hip, monkeypatch, name, True, admmFirst=k)
    sb.run()
    sb.synchronize()
    new = []
    for b, d in enumerate(inst):
        if b % 2 == 0:
            lo, hi = SR.move_classes(d, 70 + b)
            assert sb.update(b, 1, d["g"][None], lbA=lo[None], ubA=hi[None], x0=d["x0"][None], y0=d["y0"][None]) == 0
            new.append(Ref(d, hip.default_options(), lo, hi, keep=(k,)))
            assert not np.array_equal(new[-1].rhov, old[b].rhov)
        else:
            new.append(old[b])
    sb.resolve(warm=False)
    _, _, st = sb.solution()
    assert sb.launch_counts() == (1, 2)
    for b, ref in enumerate(new):
        assert st[b]["admmIter"] == k, (name, b, st[b])
        ra = sb.read_admm(b)
        check_vectors(ra, ref)
        check_iterates(ra, ref, k, ref.states(True)[k], f"{name} / instance {b} / {'moved' if b % 2 == 0 else 'kept'} / ")
    sb.close()


def test_update_that_changes_no_class(hip, monkeypatch):
    """D: shifted bounds, every row in its class: no second setup launch (one setup, two launches) and the iterates hold at the old
    weights and the new bounds"""
    name, k = "small", 5
    inst = _inst(name)
    sb = _handle(hip, monkeypatch, name, True, admmFirst=k)
    sb.run()
    sb.synchronize()
    new = []
    for b, d in enumerate(inst):
        lo, hi = SR.same_classes(d, 90 + b)
        assert sb.update(b, 1, d["g"][None], lbA=lo[None], ubA=hi[None], x0=d["x0"][None], y0=d["y0"][None]) == 0
        new.append(Ref(d, hip.default_options(), lo, hi, keep=(k,)))
        assert np.array_equal(new[-1].rhov, _refs(name)[b].rhov)
    sb.resolve(warm=False)
    _, _, st = sb.solution()
    assert sb.launch_counts() == (1, 2)
    for b, ref in enumerate(new):
        assert st[b]["admmIter"] == k
        ra = sb.read_admm(b)
        check_vectors(ra, ref)
        check_iterates(ra, ref, k, ref.states(True)[k], f"{name} / instance {b} / same classes / ")
    sb.close()


def test_read_back_changes_nothing(hip, monkeypatch):
    """E: run, read every instance back, run again = run twice without the read-back, to the bit (solutions, statistics, ADMM state)"""
    name = "small"
    out = []
    for read in (False, True):
        sb = _handle(hip, monkeypatch, name, True, admmFirst=5)
        sb.run()
        if read:
            first = [sb.read_admm(b) for b in range(sb.B)]
            again = [sb.read_admm(b) for b in range(sb.B)]
            for f, a in zip(first, again):
                assert all(np.array_equal(f[k], a[k]) for k in ("rhov", "l", "u", "xa", "ya", "za"))
        else:
            sb.synchronize()
        sb.run()
        x, y, st = sb.solution()
        out.append((x, y, [(s["iterTotal"], s["admmIter"], s["trials"]) for s in st], [sb.read_admm(b) for b in range(sb.B)]))
        sb.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    for f, a in zip(out[0][3], out[1][3]):
        assert all(np.array_equal(f[k], a[k]) for k in ("xa", "ya", "za", "rhov"))
