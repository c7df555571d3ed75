"""Reference of descriptools_amd.routing in integers, written from the definition in that module's docstring on the
graphs tests/_mfd_ref.py (graph, split) and tests/_dinf_ref.py (receivers, share) build; the levels are Kahn's, as
in their accumulate.

The definition, restated.  The graph, nodata, q = rint(w * 2^s), the split and the -100 on or below a cycle are the
accumulations'.  A complete cell with load T = q + arrivals passes on O = f(T, p) and keeps R = T - O; the receivers
get the accumulation's split of O.  p is float64:
    decay    D = rint(ldexp(p, 30)), p in [0, 1]:  O = floor(T * D / 2^30)
    retain   C = min(rint(ldexp(p, s)), 2^53):     O = T - C if T > C else 0
    limit    the same C:                           O = min(T, C)
A parameter outside its contract (NaN, negative, a decay above 1) acts as the identity, O = T (the device tier; the
host tier refuses it).  Outputs: inflow = T - q, load = T, outflow = O, retained = R, each ldexp(., -s) as float64, -100
where the cell never completes or is nodata."""
import numpy as np

import _dinf_ref as D
import _mfd_ref as M

CAP_MAX = 1 << 53
OUTPUTS = ("inflow", "load", "outflow", "retained")


def quantise_param(transfer, param, frac_bits):
    """-> (int64 D or C per cell, flat; bad bool per cell): a bad cell holds the identity"""
    p = np.asarray(param, np.float64).reshape(-1)
    if transfer == "decay":
        bad = ~((p >= 0) & (p <= 1))
        return np.rint(np.ldexp(np.where(bad, 1.0, p), 30)).astype(np.int64), bad
    bad = ~(p >= 0)
    ident = 0.0 if transfer == "retain" else np.inf
    with np.errstate(over="ignore"):
        c = np.rint(np.ldexp(np.where(bad, ident, p), frac_bits))
    big = c >= float(CAP_MAX)
    return np.where(big, CAP_MAX, np.where(big, 0.0, c).astype(np.int64)), bad


def transfer_of(transfer, T, Q):
    """O of the loads T (int64) under the quantised parameters Q"""
    T = np.asarray(T, np.int64)
    if transfer == "decay":
        return (T >> 30) * Q + (((T & ((1 << 30) - 1)) * Q) >> 30)
    if transfer == "retain":
        return np.where(T > Q, T - Q, 0)
    if transfer == "limit":
        return np.minimum(T, Q)
    raise ValueError(transfer)


def transfer_exact(transfer, T, Q):
    """the same on Python integers of any size, one cell"""
    T, Q = int(T), int(Q)
    if transfer == "decay":
        return T * Q >> 30
    return max(T - Q, 0) if transfer == "retain" else min(T, Q)


def route(flow, param, transfer, weights=None, frac_bits=None, full=False):
    """flow: uint16[H, W, 8] shares or float32[H, W] angles -> dict of the four float64 rasters; full=True:
    (that, dict(T, O, q, done, left, nodata, bad)) with `left` what left the domain: the O of cells without an edge
    plus the parts of a split that point off the raster or into nodata, a Python integer"""
    f = np.asarray(flow)
    mfd = f.ndim == 3
    H, W = f.shape[:2]
    n = H * W
    if frac_bits is None:
        wmax = 1.0 if weights is None else (float(np.max(weights)) if n else 0.0)
        frac_bits = D.default_frac_bits(n, wmax) if n else 0
    q = D.quantise(weights, (H, W), frac_bits)
    Q, bad = quantise_param(transfer, param, frac_bits)
    if mfd:
        P, nod, recv, edge, gone = M.graph(f)
        pending = np.bincount(recv[edge], minlength=n)
    else:
        r0, r1, p2, gone0, gone1 = D.receivers(f)
        nod = (f == np.float32(-100)).reshape(-1)
        pending = np.bincount(r0[r0 >= 0], minlength=n) + np.bincount(r1[r1 >= 0], minlength=n)
    T = q.copy()
    O = np.zeros(n, np.int64)
    done = np.zeros(n, bool)
    left = 0
    front = np.flatnonzero((pending == 0) & ~nod)
    while front.size:
        done[front] = True
        o = transfer_of(transfer, T[front], Q[front])
        O[front] = o
        if mfd:
            m = M.split(o, P[front])
            e, r = edge[front], recv[front]
            np.add.at(T, r[e], m[e])
            left += int(m[gone[front]].sum()) + int(o[~(P[front] > 0).any(axis=1)].sum())
            cand = r[e]
        else:
            m2 = D.share(o, p2[front])
            m1 = o - m2
            f0, f1 = r0[front], r1[front]
            e0, e1 = f0 >= 0, f1 >= 0
            np.add.at(T, f0[e0], m1[e0])
            np.add.at(T, f1[e1], m2[e1])
            g0, g1 = gone0[front], gone1[front]
            none = ~(e0 | g0)  # no receiver at all: m1 = O leaves
            left += int(m1[g0 | none].sum()) + int(m2[g1].sum())
            cand = np.concatenate((f0[e0], f1[e1]))
        np.subtract.at(pending, cand, 1)
        front = np.unique(cand[pending[cand] == 0])

    def scaled(v):
        return np.where(done, np.ldexp(v.astype(np.float64), -frac_bits), -100.0).reshape(H, W)

    out = {"inflow": scaled(T - q), "load": scaled(T), "outflow": scaled(O), "retained": scaled(T - O)}
    if full:
        return out, dict(T=T, O=O, q=q, done=done, left=left, nodata=nod, bad=bad, frac_bits=frac_bits)
    return out
