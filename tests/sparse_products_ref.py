"""Patterns, inputs, long-double references and bounds for the sparse products of the sparse arm (sp_Ex, sp_Qx2, sp_ETy, sp_residual, sp_Cx2,
sp_C_from_Ex over g_ell; tests/test_gpu_sparse_products.py holds lcqp_hip_sparse_product_probe to them, tests/test_sparse_products_ref.py
shows on the CPU that a float64 evaluation of the same sums stays inside the bounds).  Everything is formed from dense copies of the CSC
matrices; nothing comes from oracle/.

Bounds (eps = 2^-52; a dot product of len terms in any order, fused or not, errs by at most len eps / 2 of the sum of magnitudes):
    plain products   |out_i - ref_i| <= (len_i + 2) eps (|M| |x| + |base|)_i      len_i the row or column length
    r1               the same with len_i = len_i(Q) + len_i(E') and the magnitudes |g| + |Q| |x| + |E|' |y|
    C v              (len_col_i + max len_row + 3) eps (|E|' P |E| |v|)_i,  P the swap of the L and R rows (zero on the rows of A)
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
B = 5


def _values(rng, k):
    """mixed signs, magnitudes over six decades"""
    return rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-3, 3, k)


def _instances(n, nC, nK, Qmask, Emask, seed):
    """B instances on one pattern: Q symmetric in values, E = [A; L; R]"""
    out = []
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        Qd = np.zeros((n, n)); iu = np.triu_indices(n)
        Qd[iu] = _values(rng, len(iu[0])); Qd = np.where(Qmask, np.triu(Qd) + np.triu(Qd, 1).T, 0.0)
        Ed = np.where(Emask, _values(rng, Emask.size).reshape(Emask.shape), 0.0)
        Q = sp.csc_matrix(Qd); E = sp.csc_matrix(Ed)
        Q.sort_indices(); E.sort_indices()
        assert Q.nnz == int(Qmask.sum()) and E.nnz == int(Emask.sum())
        out.append(dict(nV=n, nC=nC, nComp=nK, Q=Q, E=E, Qd=Qd, Ed=Ed, g=np.zeros(n), lbA=np.full(nC, -1.0), ubA=np.full(nC, 1.0)))
    return out


def p1():
    """tridiagonal Q, rows of A with four consecutive variables (overlapping by one), L and R on single variables: no row of Q or E and no
    column of E longer than 4; n = 70 is no multiple of a tile (4 x 8 rows at width 4), m = 36 neither"""
    n, nC, nK = 70, 20, 8
    Qm = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 1
    Em = np.zeros((nC + 2 * nK, n), dtype=bool)
    for r in range(nC):
        Em[r, 3 * r:3 * r + 4] = True
    for i in range(nK):
        Em[nC + i, 4 * i + 1] = True; Em[nC + nK + i, 4 * i + 2] = True
    return _instances(n, nC, nK, Qm, Em, 100)


def p2():
    """the pattern of the synthetic (64, 32, 8) at span = 6, with values of mixed size"""
    import sparse_kkt_ref as S
    d = S.synthetic((64, 32, 8), 1)[0]
    Qm = np.asarray(d["Q"].todense()) != 0; Em = np.asarray(d["E"].todense()) != 0
    return _instances(64, 32, 8, Qm | Qm.T, Em, 200)


def p3():
    """the coupling-row pattern (sparse_kkt_ref.coupled at extra = 3) widened: three rows of E over (nearly) every variable, variable 5 in
    nine further rows, row and column 0 of Q with twelve further entries, and the last variable in no row of E"""
    import sparse_kkt_ref as S
    d = S.coupled((128, 64, 16), 1, 3)[0]
    n, nC, nK = d["nV"], d["nC"], d["nComp"]
    Qm = np.asarray(d["Q"].todense()) != 0; Qm = Qm | Qm.T
    Qm[0, 1:13] = True; Qm[1:13, 0] = True
    Em = np.asarray(d["E"].todense()) != 0
    Em[10:19, 5] = True
    lone = [j for j in range(n) if not Em[nC:, j].any()][-1]      # (not a variable of a complementarity pair: those rows would be empty)
    Em[:, lone] = False
    assert Em.any(axis=1).all()
    return _instances(n, nC, nK, Qm, Em, 300)


PATTERNS = {"P1": p1, "P2": p2, "P3": p3}


def slab(lengths):
    """(W, tails) of the ELL slab of a gather with these row lengths: width 4 if no row is longer than 4, else 8; a tail if one is longer
    than the width (lcqp_sparse_pattern.hpp: ell_slab)"""
    mx = int(np.max(lengths))
    W = 4 if mx <= 4 else 8
    return W, int(mx > W)


def slabs(d):
    Qm, Em = d["Qd"] != 0, d["Ed"] != 0
    return dict(Q=slab(Qm.sum(axis=1)), E=slab(Em.sum(axis=1)), T=slab(Em.sum(axis=0)))


def inputs(inst, seed):
    """vn [B][8][n], vm [B][4][m] of mixed signs and sizes"""
    rng = np.random.default_rng(seed)
    n, m = inst[0]["nV"], inst[0]["Ed"].shape[0]
    return _values(rng, B * 8 * n).reshape(B, 8, n), _values(rng, B * 4 * m).reshape(B, 4, m)


def swap(d, v):
    """P v: the entries of the L rows and the R rows exchanged, zero on the rows of A"""
    nC, nK = d["nC"], d["nComp"]
    out = np.zeros_like(v)
    out[nC:nC + nK] = v[nC + nK:]; out[nC + nK:] = v[nC:nC + nK]
    return out


N_IN = ("x", "q0", "q1", "base", "g", "xr", "c0", "c1")
M_IN = ("y", "yr", "lx0", "lx1")


def evaluate(d, vn, vm, dt):
    """every output of the probe for one instance in dtype dt, by dense products"""
    Q, E = d["Qd"].astype(dt), d["Ed"].astype(dt)
    a = {k: vn[i].astype(dt) for i, k in enumerate(N_IN)}; a.update({k: vm[i].astype(dt) for i, k in enumerate(M_IN)})
    ety = E.T @ a["yr"]; qxr = Q @ a["xr"]
    r = dict(Ex=E @ a["x"], Qx0=Q @ a["q0"], Qx1=Q @ a["q1"], ETy=a["base"] - E.T @ a["y"], r1=(-a["g"] - qxr) - ety, Qxr=qxr,
             Cx0=E.T @ swap(d, E @ a["c0"]), Cx1=E.T @ swap(d, E @ a["c1"]), CE0=E.T @ swap(d, a["lx0"]), CE1=E.T @ swap(d, a["lx1"]),
             CE=E.T @ swap(d, a["lx0"]), CEzero=np.zeros(len(a["g"]), dtype=dt))
    r["r1_scale"] = (np.abs(a["g"]) + np.abs(qxr) + np.abs(ety)).max()
    return r


def bounds(d, vn, vm):
    """the bound of every output (long double), and the relative one of r1_scale"""
    aQ, aE = np.abs(d["Qd"]).astype(LD), np.abs(d["Ed"]).astype(LD)
    a = {k: np.abs(vn[i]).astype(LD) for i, k in enumerate(N_IN)}; a.update({k: np.abs(vm[i]).astype(LD) for i, k in enumerate(M_IN)})
    lq = (d["Qd"] != 0).sum(axis=1); le = (d["Ed"] != 0).sum(axis=1); lt = (d["Ed"] != 0).sum(axis=0)
    e = LD(EPS)
    c = (lt + le.max() + 3) * e
    r = dict(Ex=(le + 2) * e * (aE @ a["x"]), Qx0=(lq + 2) * e * (aQ @ a["q0"]), Qx1=(lq + 2) * e * (aQ @ a["q1"]),
             ETy=(lt + 2) * e * (aE.T @ a["y"] + a["base"]), r1=(lq + lt + 2) * e * (a["g"] + aQ @ a["xr"] + aE.T @ a["yr"]), Qxr=(lq + 2) * e * (aQ @ a["xr"]),
             Cx0=c * (aE.T @ swap(d, aE @ a["c0"])), Cx1=c * (aE.T @ swap(d, aE @ a["c1"])),
             CE0=(lt + 2) * e * (aE.T @ swap(d, a["lx0"])), CE1=(lt + 2) * e * (aE.T @ swap(d, a["lx1"])),
             CE=(lt + 2) * e * (aE.T @ swap(d, a["lx0"])), CEzero=np.zeros(len(lq), dtype=LD))
    r["r1_scale"] = float((lq + lt).max() + 3) * EPS
    return r


OUTPUTS = ("Ex", "Qx0", "Qx1", "ETy", "r1", "Qxr", "Cx0", "Cx1", "CE0", "CE1", "CE", "CEzero")


def ratios(got, d, vn, vm):
    """name -> worst |got - ref| / bound over the entries (0 / 0 = 0; anything / 0 = inf)"""
    ref = evaluate(d, vn, vm, LD); bd = bounds(d, vn, vm)
    out = {}
    for k in OUTPUTS:
        err = np.abs(np.asarray(got[k], dtype=LD) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = float(np.where(err > 0, err / bd[k], 0.0).max())
    out["r1_scale"] = abs(float(got["r1_scale"]) / float(ref["r1_scale"]) - 1.0) / bd["r1_scale"]
    return out
