"""The dense cases of tests/test_gpu_host_io.py and the sequence of host calls whose solutions tools/make_host_io_golden.py records as
tests/golden/host_io_bits.npz: one definition for the recorder and the test.

Shapes (nV, nC, nComp), the smallest where packing can go wrong: (5, 0, 2) has an odd row length (rows that are not 16-byte aligned) and no
A, (7, 3, 0) no complementarity rows (the pools of lbL / lbR hold one spare element), (129, 2, 3) crosses a padded size (np = 256).  B = 5
each, a box on a strict subset of the variables.  Every optional vector is present in the "full" variant of a shape; its other variant
keeps only the lower ("lb only") or only the upper ("ub only") box bounds, so each vector is also absent in some case."""
import numpy as np

from batch_helpers import stack, vectors
from problems import random_lcqp

B = 5
CASES = (((5, 0, 2), "full"), ((5, 0, 2), "lb only"), ((7, 3, 0), "full"), ((7, 3, 0), "ub only"), ((129, 2, 3), "full"), ((129, 2, 3), "lb only"))
IDS = ["%dx%dx%d, %s" % (s + (v,)) for s, v in CASES]
STAGES = ("load", "range", "update")      # a load of the batch; a load of [2, 4) onto it; an update of the batch and a warm re-solve
RANGE = (2, 2)                            # first, count of the second load
OPTIONAL = ("lbL", "ubL", "lbR", "ubR", "lbA", "ubA", "lb", "ub", "x0", "y0")
_cache = {}


def instance(rng, shape, variant):
    n, nC, nK = shape
    d = random_lcqp(rng, n, nC, nK, box=True, shifted=True)
    boxed = np.arange(n) % 3 != 0
    lo = np.where(boxed, d["lb"], -np.inf)                                   # random_lcqp: lb = xs - 2 on every variable
    d.update(lb=lo, ub=np.where(boxed & (np.arange(n) % 2 == 1), lo + 4.0, np.inf),
             ubL=rng.uniform(5.0, 6.0, nK), ubR=rng.uniform(5.0, 6.0, nK), x0=rng.uniform(-0.1, 0.1, n), y0=rng.uniform(-0.1, 0.1, n + nC + 2 * nK))
    if variant != "full":
        if variant == "ub only":
            d["ub"] = np.where(boxed, lo + 4.0, np.inf)
        keep = variant[:2]
        for k in OPTIONAL:
            if k != keep:
                d[k] = None
    return d


def moved(d, seed):
    """new values for every vector an update takes that the instance carries; the set of box-bounded variables stays"""
    rng = np.random.default_rng(seed)
    e = dict(d, g=d["g"] * (1.0 + 0.02 * rng.standard_normal(d["nV"])))
    for k in OPTIONAL:
        if d[k] is not None:
            e[k] = d[k] + 0.02 * rng.uniform(-1.0, 1.0, d[k].shape) * (0.1 if k in ("lbL", "lbR") else 1.0)      # (inf stays inf)
    return e


def data(case):
    """the instances of the three stages, made once: B for the load, RANGE[1] for the second load, B moved ones for the update"""
    if case not in _cache:
        shape, variant = case
        rng = np.random.default_rng(1000 * shape[0] + len(variant))
        ds = [instance(rng, shape, variant) for _ in range(B)]
        ds2 = [instance(rng, shape, variant) for _ in range(RANGE[1])]
        held = ds[:RANGE[0]] + ds2 + ds[RANGE[0] + RANGE[1]:]
        _cache[case] = (ds, ds2, [moved(d, 50 + b) for b, d in enumerate(held)])
    return _cache[case]


def cap_for(arrays, count, chunk):
    """the staging cap under which a host call that moves `arrays` ([count][..] each, or None) goes in chunks of `chunk` instances: two
    chunks of device staging, half the cap each (include/lcqp_hip.h, lcqp_hip_batch_load)"""
    per = 8 * sum(a.size // count for a in arrays if a is not None)
    return 2 * chunk * per + 8


def stats_array(st):
    return np.array([[float(v) for v in s.values()] for s in st])


def run_stages(hip, case, chunked=False):
    """the three stages on one handle.  Returns (bits, pools): bits[stage + "_x" / "_y" / "_st"] of the solve behind each stage, pools[stage]
    = read_problem of every instance right after the stage's load / update.  chunked: every host call under a staging cap that makes a
    call on 5 instances go in chunks of 2, 2, 1 and one on 2 instances in chunks of 1, 1."""
    (n, nC, nK), _ = case
    ds, ds2, ds3 = data(case)
    bt = hip.BatchLCQP(B, n, nC, nK, with_box=True, opt=hip.default_options(perturbStep=0, printLevel=0))
    bits, pools = {}, {}

    def call(f, first, xs, mats):
        args = [stack(xs, k) for k in mats]
        kw = vectors(f, xs)
        if f == bt.load:
            kw["A"] = stack(xs, "A")
        cap = cap_for(args + list(kw.values()), len(xs), 2 if len(xs) == B else 1) if chunked else None
        with bt._staging(cap):
            rc = f(first, len(xs), *args, **kw)
        assert rc == 0, (rc, bt._last_error())

    def record(stage):
        pools[stage] = [bt.read_problem(b) for b in range(B)]
        x, y, st = bt.solution()
        bits.update({stage + "_x": x, stage + "_y": y, stage + "_st": stats_array(st)})

    call(bt.load, 0, ds, ("Q", "g", "L", "R"))
    bt.run(); record("load")
    call(bt.load, RANGE[0], ds2, ("Q", "g", "L", "R"))
    bt.run(); record("range")
    call(bt.update, 0, ds3, ("g",))
    bt.resolve(warm=True); record("update")
    bt.close()
    return bits, pools
