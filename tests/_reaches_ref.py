"""Pure-numpy reference of descriptools_amd.reaches, independent of the kernels: searchsorted for ranks and bins,
bincount with the quantised values as weights (exact: every partial sum is an integer below 2^53), cumsum along k.

Shared by tests/test_reaches_host.py (which checks it on hand-built cases whose tables are written out by hand) and
tests/test_gpu_reaches.py (which holds the GPU to it entry for entry).  network() gives the inputs of a terrain case:
link from tests/_streams_ref.py and the river index and HAND from oracle.flowhand, never from the code under test."""
import numpy as np

import _streams_ref as S

E, SE, S_, SW, W_, NW, N, NE = S.E, S.SE, S.S, S.SW, S.W_, S.NW, S.N, S.NE


def network(dem, fdr, river):
    """(link int64, idx int64, hand in the DEM's dtype) of a terrain case: the river index of the oracle's flowhand
    walk, HAND = dem - dem[idx] with negatives -> 0 (flowhand.hand_calculator), -100 where there is no river cell"""
    import oracle
    _, _, link = S.reference(fdr, river)
    idx, _, _ = oracle.flowhand_fast(fdr, river)
    dem = np.asarray(dem)
    ok = idx >= 0
    d = dem.reshape(-1)
    diff = dem - d[np.where(ok, idx, 0)]
    hand = np.where(ok, np.maximum(diff, 0), -100).astype(dem.dtype)
    return link, idx, hand


def terrain(H, W, seed, threshold, px=10.0):
    """(dem, slope, fdr, fac, river) of synthetic terrain, all from the oracle"""
    import oracle
    dem = oracle.synth_dem(seed, H, W)
    slope, fdr = oracle.slope_d8(dem, px)
    fac = oracle.flowacc(fdr)
    return dem, slope, fdr, fac, (fac > threshold).astype(np.int8)


def catchments(link, idx):
    """(reach int32, catch int32, heads int64)"""
    link = np.asarray(link, np.int64)
    shape = link.shape
    l = link.reshape(-1)
    n = l.size
    heads = np.flatnonzero(l == np.arange(n, dtype=np.int64)).astype(np.int64)
    reach = np.full(n, -100, np.int32)
    m = np.flatnonzero(l >= 0)
    if heads.size:
        pos = np.searchsorted(heads, l[m])
        ok = (pos < heads.size) & (heads[np.minimum(pos, heads.size - 1)] == l[m])
        reach[m] = np.where(ok, pos, -100)
    i = np.asarray(idx, np.int64).reshape(-1)
    v = (i >= 0) & (i < n)
    cat = np.full(n, -100, np.int32)
    cat[v] = reach[i[v]]
    return reach.reshape(shape), cat.reshape(shape), heads


def channels(fdr, reach, px, R):
    """(end, down, n_cells, n_card, n_diag: int64[R]; length float64[R])"""
    fdr = np.asarray(fdr, np.uint8)
    H, W = fdr.shape
    r = np.asarray(reach).reshape(-1).astype(np.int64)
    net, succ = S.network_edges(fdr, (r >= 0).reshape(H, W))
    c = np.flatnonzero(net)
    has = succ[c] >= 0
    d = succ[c]
    y, x = np.divmod(c, max(W, 1))
    dy, dx = np.divmod(np.where(has, d, c), max(W, 1))
    diag = has & (dy != y) & (dx != x)
    card = has & ~diag
    n_cells = np.bincount(r[c], minlength=R).astype(np.int64)
    n_card = np.bincount(r[c[card]], minlength=R).astype(np.int64)
    n_diag = np.bincount(r[c[diag]], minlength=R).astype(np.int64)
    rd = np.where(has, r[np.where(has, d, c)], -1)
    last = ~has | (rd != r[c])
    end = np.full(R, -1, np.int64)
    down = np.full(R, -1, np.int64)
    end[r[c[last]]] = np.where(has, d, c)[last]
    down[r[c[last]]] = rd[last]
    length = n_card.astype(np.float64) * px + n_diag.astype(np.float64) * (px * np.sqrt(2.0))
    return end, down, n_cells, n_card, n_diag, length


def heights(hand):
    """hand as the Python layer hands it to the library: float32 and float64 as they are, anything else as float64"""
    h = np.asarray(hand)
    return h if h.dtype in (np.float32, np.float64) else h.astype(np.float64)


def bed_weights(slope, shape):
    """sqrt(1 + t * t) in float64, t = slope / 100 where slope is finite and > 0, else 0"""
    if slope is None:
        return np.ones(shape, np.float64)
    sl = np.asarray(slope, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(sl) & (sl > 0)
    t = np.where(ok, sl.astype(np.float64) / 100.0, 0.0)
    with np.errstate(over="ignore"):
        return np.sqrt(1.0 + t * t)


def default_frac_bits(n, stages, slope=None):
    """s = 51 - ceil(log2 n) - e with 2^e <= max(stages[-1], wmax) < 2^(e+1), flowacc's rule for weights up to that
    maximum; the contract n * rint(max * 2^s) <= 2^52 is asserted"""
    top = max(float(stages[-1]), float(bed_weights(slope, np.shape(slope)).max()) if slope is not None else 1.0)
    e = int(np.floor(np.log2(top)))
    assert 2.0 ** e <= top < 2.0 ** (e + 1)
    s = 51 - int(np.ceil(np.log2(n))) - e
    assert n * int(np.rint(np.ldexp(top, s))) <= 2 ** 52
    return s


def tables(catch, hand, stages, R, s, slope=None):
    """(cells, Hq, Bq: int64[R, K]) and the count of taking-part cells"""
    st = np.asarray(stages, np.float64)
    K = st.size
    c = np.asarray(catch).reshape(-1).astype(np.int64)
    h = heights(hand).reshape(-1).astype(np.float64)  # float32 -> float64 is exact
    w = bed_weights(slope, np.shape(catch)).reshape(-1)
    with np.errstate(invalid="ignore"):
        take = (c >= 0) & (c < R) & (h >= 0) & (h <= st[-1])
    k = np.searchsorted(st, h[take], side="left")
    key = c[take] * K + k
    hq = np.rint(np.ldexp(h[take], s))
    wq = np.rint(np.ldexp(w[take], s))
    assert hq.sum() < 2 ** 53 and wq.sum() < 2 ** 53
    cells = np.bincount(key, minlength=R * K).astype(np.int64).reshape(R, K).cumsum(axis=1)
    Hq = np.bincount(key, weights=hq, minlength=R * K).astype(np.int64).reshape(R, K).cumsum(axis=1)
    Bq = np.bincount(key, weights=wq, minlength=R * K).astype(np.int64).reshape(R, K).cumsum(axis=1)
    return cells, Hq, Bq, int(take.sum())


def derive(stages, cells, Hq, Bq, px, s):
    """(area, volume, bed_area) float64[R, K]"""
    st = np.asarray(stages, np.float64)
    a = px * px
    fc = cells.astype(np.float64)
    area = fc * a
    volume = np.maximum(st[None, :] * fc - np.ldexp(Hq.astype(np.float64), -s), 0.0) * a
    bed = np.ldexp(Bq.astype(np.float64), -s) * a
    return area, volume, bed


def inundate(catch, hand, stage):
    """depth float32"""
    c = np.asarray(catch).astype(np.int64)
    h = heights(hand).astype(np.float64)
    sg = np.asarray(stage, np.float64)
    R = sg.size
    inr = (c >= 0) & (c < R)
    st = np.where(inr, sg[np.where(inr, c, 0)] if R else np.nan, np.nan)
    with np.errstate(invalid="ignore"):
        wet = inr & np.isfinite(st) & (h >= 0) & (h <= st)
        depth = np.where(wet, (st - h).astype(np.float32), np.float32(0))
    depth = np.where(h == -100, np.float32(-100), depth)
    return depth.astype(np.float32)


_ = -100


def hand_cases():
    """name -> dict of inputs and of every expected output, written out by hand"""
    c = {}
    r2 = np.sqrt(2.0)
    # two one-cell links (0,0) and (0,2) meet at the confluence (1,1); the link below runs (1,1) -> (2,1) and off the
    # raster.  HAND is a V across the lower link.
    c["confluence"] = dict(
        fdr=[[SE, S_, SW], [E, S_, W_], [E, S_, W_]],
        river=[[1, 0, 1], [0, 1, 0], [0, 1, 0]],
        link=[[0, _, 2], [_, 4, _], [_, 4, _]],
        idx=[[0, 4, 2], [4, 4, 4], [7, 7, 7]],
        reach=[[0, _, 1], [_, 2, _], [_, 2, _]],
        catch=[[0, 2, 1], [2, 2, 2], [2, 2, 2]],
        heads=[0, 2, 4],
        px=2.0,
        end=[4, 4, 7], down=[2, 2, -1], n_cells=[1, 1, 2], n_card=[0, 0, 1], n_diag=[1, 1, 0],
        length=[0.0 * 2.0 + 1.0 * (2.0 * r2), 0.0 * 2.0 + 1.0 * (2.0 * r2), 2.0],
        hand=np.array([[0, 1.5, 0], [2.0, 0, 2.5], [1.0, 0, 3.0]], np.float32),
        slope=None, stages=[0.0, 1.0, 2.0, 3.0], s=2,
        cells=[[1, 1, 1, 1], [1, 1, 1, 1], [2, 3, 5, 7]],
        Hq=[[0, 0, 0, 0], [0, 0, 0, 0], [0, 4, 18, 40]],
        Bq=[[4, 4, 4, 4], [4, 4, 4, 4], [8, 12, 20, 28]],
        area=[[4.0] * 4, [4.0] * 4, [8.0, 12.0, 20.0, 28.0]],
        volume=[[0.0, 4.0, 8.0, 12.0], [0.0, 4.0, 8.0, 12.0], [0.0, 8.0, 22.0, 44.0]],
        bed_area=[[4.0] * 4, [4.0] * 4, [8.0, 12.0, 20.0, 28.0]],
        stage=[0.5, np.nan, 2.0],
        depth=[[0.5, 0.5, 0], [0, 2, 0], [1, 2, 0]])
    # a one-cell link without an edge, (0,0), beside a two-cell link; a slope raster with a 75 % cell (bed weight 1.25),
    # a NaN and a negative (weight 1)
    c["one_cell_link"] = dict(
        fdr=[[E, E, E, 0]],
        river=[[1, 0, 1, 1]],
        link=[[0, _, 2, 2]],
        idx=[[0, 2, 2, 3]],
        reach=[[0, _, 1, 1]],
        catch=[[0, 1, 1, 1]],
        heads=[0, 2],
        px=1.0,
        end=[0, 3], down=[-1, -1], n_cells=[1, 2], n_card=[0, 1], n_diag=[0, 0], length=[0.0, 1.0],
        hand=np.array([[0, 0.75, 0, 0]], np.float64),
        slope=np.array([[0, 75.0, np.nan, -5.0]], np.float32), stages=[0.5, 1.0], s=3,
        cells=[[1, 1], [2, 3]],
        Hq=[[0, 0], [0, 6]],
        Bq=[[8, 8], [16, 26]],
        area=[[1.0, 1.0], [2.0, 3.0]],
        volume=[[0.5, 1.0], [1.0, 2.25]],
        bed_area=[[1.0, 1.0], [2.0, 3.25]],
        stage=[np.inf, 0.75],
        depth=[[0, 0, 0.75, 0.75]])
    # a network cycle (0,0) -> (0,1) -> (1,1) -> (1,0) with the tributary (2,2) as the only link: (1,2) drains to a
    # cell of the cycle and so has no catchment; the link's code points at the cycle, which is no edge
    c["cycle"] = dict(
        fdr=[[E, S_, 0], [N, W_, 0], [0, 0, NW]],
        river=[[1, 1, 0], [1, 1, 0], [0, 0, 1]],
        link=[[_, _, _], [_, _, _], [_, _, 8]],
        idx=[[0, 1, _], [3, 4, 4], [_, 8, 8]],
        reach=[[_, _, _], [_, _, _], [_, _, 0]],
        catch=[[_, _, _], [_, _, _], [_, 0, 0]],
        heads=[8],
        px=3.0,
        end=[8], down=[-1], n_cells=[1], n_card=[0], n_diag=[0], length=[0.0],
        hand=np.array([[0, 0, 5], [0, 0, 1], [-100, 2, 0]], np.int16),
        slope=None, stages=[1.0], s=0,
        cells=[[1]], Hq=[[0]], Bq=[[1]],
        area=[[9.0]], volume=[[9.0]], bed_area=[[9.0]],
        stage=[1.0],
        depth=[[0, 0, 0], [0, 0, 0], [-100, 0, 1]])
    for d in c.values():
        d["fdr"] = np.array(d["fdr"], np.uint8)
        d["river"] = np.array(d["river"], np.int8)
        for k in ("link", "idx", "heads", "end", "down", "n_cells", "n_card", "n_diag", "cells", "Hq", "Bq"):
            d[k] = np.array(d[k], np.int64)
        for k in ("reach", "catch"):
            d[k] = np.array(d[k], np.int32)
        for k in ("length", "area", "volume", "bed_area", "stages", "stage"):
            d[k] = np.array(d[k], np.float64)
        d["depth"] = np.array(d["depth"], np.float32)
    return c
