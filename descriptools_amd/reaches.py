"""Reach catchments, per-reach stage tables, rating curves and HAND inundation (net-new), on the GPU: the HAND
synthetic-rating-curve method (Zheng et al. 2018) on the rasters the chain already computes.

Definitions (the kernels in csrc/dt_reaches.hip, the C header and the tests hold to them).  Rasters are H x W,
row-major, flat index y * W + x, N = H * W < 2^31.

* Reaches.  link (int64) as streams.stream_network writes it: the flat index of the head of the cell's link on network
  cells, -100 elsewhere.  A cell c is a head when link[c] == c; R = the number of heads.  The reach id of a head is its
  rank among the heads in ascending flat index, 0-based; heads[r] is that flat index.  reach[c] (int32) = the id of
  link[c] on cells with link[c] >= 0, -100 elsewhere.
* Catchments.  indices: the river index of flowhand.flow_hand_index (the flat index of the river cell the cell drains
  to, the cell itself on river cells, -100 where there is none).  catchment[c] (int32) = reach[indices[c]] when
  0 <= indices[c] < N, else -100 (so -100 too where indices[c] names a cell off the network or on a network cycle).
* Channels (per reach, from fdr and reach).  The network graph is streams' own: a cell c with reach[c] >= 0 has the
  edge c -> d when its code is one of the eight D8 codes and d is in the raster with reach[d] >= 0.  For reach r over
  its cells: n_cells[r]; n_card[r], n_diag[r] = the cardinal / diagonal edges leaving its cells (the move out of the
  link's last cell into the next link counts for r); end[r] = the flat index where the link's last move lands (the
  last cell itself when it has no edge); down[r] = reach[end[r]] when the last cell has an edge, else -1.  All int64,
  exact.  length[r] = float64(n_card) * px + float64(n_diag) * (px * sqrt(2.0)), watershed's formula and association.
* Stage tables.  stages: float64[K], 1 <= K <= 1024, finite, stages[0] >= 0, strictly increasing.  A cell takes part
  when catchment[c] = r with 0 <= r < R and 0 <= hand[c] <= stages[K-1] (comparisons on the exact value; false for NaN
  and for -100).  Its bin is the smallest k with hand[c] <= stages[k].  Its quantised height is
  hq = rint(hand * 2^s), its quantised bed weight wq = rint(sqrt(1 + t*t) * 2^s) with t = slope[c] / 100 (slope in
  percent, as slope.sloper gives it) when slope[c] is finite and > 0, else t = 0 (and t = 0 everywhere without a slope
  raster); all in float64, round half to even, as flowacc.accumulate_weighted quantises.  For every reach r and stage
  k, over the cells of r with bin <= k: cells[r,k] = their number, Hq[r,k] = the sum of hq, Bq[r,k] = the sum of wq
  (int64, from the library).  Derived on the host in float64, in exactly this association:

      area     = float64(cells) * (px * px)
      volume   = max(stages[k] * float64(cells) - ldexp(float64(Hq), -s), 0.0) * (px * px)
      bed_area = ldexp(float64(Bq), -s) * (px * px)

  Contract on s = frac_bits: N * rint(max(stages[K-1], wmax) * 2^s) <= 2^52, wmax the largest bed weight (1 without a
  slope raster); every sum then converts to float64 exactly.  The default is the finest such s.
* Inundation.  depth[c] (float32) = -100 where hand[c] == -100; else float32(stage[r] - float64(hand[c])) when
  catchment[c] = r in range, stage[r] is finite and 0 <= hand[c] <= stage[r]; else 0.
* Connected inundation.  A cell is wet exactly when it gets the value of inundation's third clause (catchment in range,
  stage finite, 0 <= hand <= stage: a cell with hand == stage is wet with depth 0).  The seeds are the wet cells with
  river == 1 (river as int8, as flowhand.flow_hand_index takes it).  depth[c] is inundation's value, except that a wet
  cell whose wet region (regions.py, connectivity 8 or 4) holds no seed gets 0; cells with hand == -100 keep -100.
* Rating curves (numpy on the R x K tables).  With channel length L, bed slope S0 and Manning's n per reach (scalars
  broadcast): A = volume / L, Rh = volume / bed_area, Q = A * Rh**(2/3) * sqrt(S0) / n; 0 where cells == 0; NaN where
  L == 0, S0 is not > 0 or n is not > 0.

hand may be float32 or float64; any other real or integer dtype (the int16 HAND of an int16 DEM) is converted to
float64.  Bad arguments raise ValueError before any library call.  Users of a resident chain call the dt_dev_reach_*
entries on chain.p("idx"), chain.p("hand") and dt_dev_stream_order's link."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_i8p, c_i32p, c_i64p, c_u8p, check, ptr

Catchments = namedtuple("Catchments", ["reach", "catchment", "heads"])
Channels = namedtuple("Channels", ["end", "down", "n_cells", "n_card", "n_diag", "length"])
HydraulicTables = namedtuple("HydraulicTables", ["stages", "cells", "area", "volume", "bed_area", "frac_bits"])

_MAX_STAGES = 1024
_HEADS_CAP = 1 << 20  # heads asked for in the first call; a network with more links takes a second, lighter call


def _ids(a, what, shape=None, other=None):
    """an id / index raster (reach, catchment, link, indices) as int64 or int32 without wrapping"""
    r = _args.raster(a, what, shape, other, kinds="iu")
    if r.dtype.kind == "u" and r.size and int(r.max()) > np.iinfo(np.int64).max:
        raise ValueError("%s holds values beyond int64" % what)
    return r


def _ids32(a, what, shape=None, other=None):
    r = _ids(a, what, shape, other)
    if r.dtype != np.int32 and r.size and (int(r.max()) >= 2 ** 31 or int(r.min()) < -2 ** 31):
        raise ValueError("%s holds values that do not fit int32" % what)
    return np.ascontiguousarray(r, np.int32)


def _hand(hand, shape):
    """(array, element size): float32 and float64 as they are, anything else real or integer as float64"""
    h = _args.raster(hand, "hand", shape, "the catchment raster", kinds="biuf")
    if h.dtype == np.float32:
        return np.ascontiguousarray(h), 4
    return np.ascontiguousarray(h, np.float64), 8


def _stage(stage):
    """the stage per reach as C-contiguous float64[R]"""
    try:
        sg = np.ascontiguousarray(stage, np.float64)
    except (TypeError, ValueError):
        raise ValueError("stage must be a 1-D array of numbers") from None
    if sg.ndim != 1 or sg.size >= 2 ** 31:
        raise ValueError("stage must be a 1-D array with one value per reach, not of shape %s" % (sg.shape,))
    return sg


def _stages(stages):
    try:
        st = np.ascontiguousarray(stages, np.float64)
    except (TypeError, ValueError):
        raise ValueError("stages must be a 1-D array of numbers") from None
    if st.ndim != 1 or not 1 <= st.size <= _MAX_STAGES:
        raise ValueError("stages must be a 1-D array of 1 to %d values, not of shape %s" % (_MAX_STAGES, st.shape))
    if not np.isfinite(st).all():
        raise ValueError("stages must be finite")
    if st[0] < 0:
        raise ValueError("stages must be >= 0 (the first is %r)" % float(st[0]))
    if not (np.diff(st) > 0).all():
        raise ValueError("stages must be strictly increasing")
    return st


def bed_weight_max(slope):
    """the largest bed weight sqrt(1 + (slope / 100)^2) of a slope raster in percent; cells that are not finite and > 0
    weigh 1"""
    s = np.asarray(slope)
    ok = np.isfinite(s) & (s > 0)
    if not ok.any():
        return 1.0
    t = float(s[ok].max()) / 100.0
    return math.sqrt(1.0 + t * t)


def catchments(link, indices):
    """Catchments(reach, catchment, heads) of the link raster of streams.stream_network and the river index of
    flowhand.flow_hand_index: reach and catchment int32 rasters, heads int64[R] (see the module docstring)."""
    lk = _ids(link, "link")
    ix = _ids(indices, "indices", lk.shape, "the link raster")
    lk = np.ascontiguousarray(lk, np.int64)
    ix = np.ascontiguousarray(ix, np.int64)
    H, W = lk.shape
    n = H * W
    reach = np.empty((H, W), np.int32)
    cat = np.empty((H, W), np.int32)
    cap = min(n, _HEADS_CAP)
    heads = np.empty(cap, np.int64)
    r = C.c_int64(0)
    L = _lib.lib()
    check(L.dt_reach_catchments(ptr(lk, c_i64p), ptr(ix, c_i64p), H, W, ptr(reach, c_i32p), ptr(cat, c_i32p),
                                ptr(heads, c_i64p), cap, C.byref(r)))
    R = int(r.value)
    if R > cap:  # heads alone, at their size
        heads = np.empty(R, np.int64)
        check(L.dt_reach_catchments(ptr(lk, c_i64p), None, H, W, None, None, ptr(heads, c_i64p), R, C.byref(r)))
    return Catchments(reach, cat, heads[:R].copy() if R < heads.size else heads)


def channels(fdr, reach, px, n_reaches):
    """Channels(end, down, n_cells, n_card, n_diag, length) of every reach: int64[R] each, length float64[R] (see the
    module docstring)."""
    f = _args.raster(fdr, "fdr", dtype=np.uint8)
    rc = _ids32(reach, "reach", f.shape, "the direction raster")
    p = _args.pixel_size(px)
    R = _args.integer(n_reaches, "n_reaches", 0, 2 ** 31 - 1)
    H, W = f.shape
    out = [np.empty(R, np.int64) for _ in range(5)]
    check(_lib.lib().dt_reach_channels(ptr(f, c_u8p), ptr(rc, c_i32p), H, W, R, *[ptr(o, c_i64p) for o in out]))
    end, down, n_cells, n_card, n_diag = out
    length = n_card.astype(np.float64) * p + n_diag.astype(np.float64) * (p * math.sqrt(2.0))
    return Channels(end, down, n_cells, n_card, n_diag, length)


def hydraulic_tables(catchment, hand, px, stages, n_reaches, slope=None, frac_bits=None):
    """HydraulicTables(stages, cells, area, volume, bed_area, frac_bits): for every reach and stage the number of
    cells at or below the stage (int64[R, K]) and their area, the volume between them and the stage and their wetted
    bed area (float64[R, K]); see the module docstring.  slope: float32 percent (slope.sloper), optional."""
    cat = _ids32(catchment, "catchment")
    h, hb = _hand(hand, cat.shape)
    p = _args.pixel_size(px)
    st = _stages(stages)
    R = _args.integer(n_reaches, "n_reaches", 0, 2 ** 31 - 1)
    sl = None
    wmax = 1.0
    if slope is not None:
        sl = _args.raster(slope, "slope", cat.shape, "the catchment raster", kinds="biuf", dtype=np.float32)
        wmax = bed_weight_max(sl)
    H, W = cat.shape
    n = H * W
    s = _args.frac_bits(n, max(float(st[-1]), wmax), frac_bits,
                        ": N * rint(max(stages[K-1], wmax) * 2^frac_bits)", "the default is")
    K = st.size
    cells = np.zeros((R, K), np.int64)
    hq = np.zeros((R, K), np.int64)
    bq = np.zeros((R, K), np.int64)
    check(_lib.lib().dt_reach_tables(ptr(cat, c_i32p), h.ctypes.data_as(C.c_void_p), hb, ptr(sl, c_f32p), H, W,
                                     ptr(st, c_f64p), K, R, s, ptr(cells, c_i64p), ptr(hq, c_i64p),
                                     ptr(bq, c_i64p)))
    return tables_from_sums(st, cells, hq, bq, p, s)


def tables_from_sums(stages, cells, hq, bq, px, frac_bits):
    """HydraulicTables from the integer tables of dt_reach_tables / dt_dev_reach_tables (host arithmetic on R x K
    numbers, in the association of the module docstring)."""
    st = np.asarray(stages, np.float64)
    a = px * px
    fc = cells.astype(np.float64)
    area = fc * a
    volume = np.maximum(st[None, :] * fc - np.ldexp(hq.astype(np.float64), -frac_bits), 0.0) * a
    bed = np.ldexp(bq.astype(np.float64), -frac_bits) * a
    return HydraulicTables(st, cells, area, volume, bed, frac_bits)


def rating_curves(tables, length, bed_slope, manning_n):
    """Discharge Q (float64[R, K]) of every reach at every stage by Manning's equation on the tables: A = volume / L,
    Rh = volume / bed_area, Q = A * Rh**(2/3) * sqrt(S0) / n; 0 where cells == 0; NaN where L == 0, S0 is not > 0 or n
    is not > 0.  length, bed_slope, manning_n: per reach, scalars broadcast."""
    R, K = tables.cells.shape
    try:
        L = np.broadcast_to(np.asarray(length, np.float64), (R,))
        S0 = np.broadcast_to(np.asarray(bed_slope, np.float64), (R,))
        n = np.broadcast_to(np.asarray(manning_n, np.float64), (R,))
    except ValueError:
        raise ValueError("length, bed_slope and manning_n must be scalars or arrays of %d values" % R) from None
    bad = (L == 0) | ~(S0 > 0) | ~(n > 0)
    wet = tables.cells > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        A = tables.volume / L[:, None]
        Rh = tables.volume / tables.bed_area
        Q = A * Rh ** (2.0 / 3.0) * np.sqrt(S0)[:, None] / n[:, None]
    Q = np.where(wet, Q, 0.0)
    Q[bad] = np.nan
    return Q


def stage_for_discharge(stages, Q, q):
    """The stage (float64[R]) at which each reach carries q[r]: linear interpolation of stages over
    np.maximum.accumulate(Q[r]); NaN where q[r] is NaN, negative, above the table's last value, or the reach's curve
    is NaN."""
    st = _stages(stages)
    Q = np.asarray(Q, np.float64)
    if Q.ndim != 2 or Q.shape[1] != st.size:
        raise ValueError("Q must be of shape (R, %d), not %s" % (st.size, Q.shape))
    try:
        qq = np.broadcast_to(np.asarray(q, np.float64), (Q.shape[0],))
    except ValueError:
        raise ValueError("q must be a scalar or an array of %d values" % Q.shape[0]) from None
    out = np.full(Q.shape[0], np.nan)
    for r in range(Q.shape[0]):
        if np.isnan(Q[r]).any() or not qq[r] >= 0:
            continue
        curve = np.maximum.accumulate(Q[r])
        if qq[r] > curve[-1]:
            continue
        out[r] = np.interp(qq[r], curve, st)
    return out


def inundate(catchment, hand, stage):
    """Inundation depth (float32 raster) for a stage per reach (float64[R]); see the module docstring."""
    cat = _ids32(catchment, "catchment")
    h, hb = _hand(hand, cat.shape)
    sg = _stage(stage)
    H, W = cat.shape
    depth = np.empty((H, W), np.float32)
    check(_lib.lib().dt_inundate(ptr(cat, c_i32p), h.ctypes.data_as(C.c_void_p), hb, ptr(sg, c_f64p), H, W, sg.size,
                                 ptr(depth, c_f32p)))
    return depth


def inundate_connected(catchment, hand, stage, river, connectivity=8):
    """inundate kept to the wet regions that hold a river cell: the depth (float32 raster) of inundate, 0 on the wet
    cells without a wet path (under `connectivity`, 8 or 4) to a wet cell with river == 1; see the module docstring."""
    cat = _ids32(catchment, "catchment")
    h, hb = _hand(hand, cat.shape)
    sg = _stage(stage)
    rv = _args.raster(river, "river", cat.shape, "the catchment raster", kinds="biu", dtype=np.int8)
    cn = _args.connectivity(connectivity)
    H, W = cat.shape
    depth = np.empty((H, W), np.float32)
    check(_lib.lib().dt_inundate_connected(ptr(cat, c_i32p), h.ctypes.data_as(C.c_void_p), hb, ptr(sg, c_f64p),
                                           ptr(rv, c_i8p), H, W, sg.size, cn, ptr(depth, c_f32p)))
    return depth
