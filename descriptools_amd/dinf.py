"""D-infinity flow direction, contributing area and distance down to the stream (net-new; Tarboton 1997, TauDEM's
DinfFlowDir / AreaDinf / DinfDistDown): a flow angle on eight triangular facets, the flow of a cell split between the
two neighbours that bracket its angle.

Angle convention.  Radians, counter-clockwise from east; rows grow to the south.  Octant k (0..7) is the neighbour at
angle k pi / 4: E, NE, N, NW, W, SW, S, SE -- the D8 codes 1, 128, 64, 32, 16, 8, 4, 2.  A height is valid when it is
finite and > -100; <= -100 is nodata, as everywhere in the package; NaN and +inf are not nodata but take part in no
facet.

flow_direction.  For a valid centre e0 the facets (e1 cardinal, e2 diagonal, ac, af)

    1 (E, NE, 0, +1)  2 (N, NE, 1, -1)  3 (N, NW, 1, +1)  4 (W, NW, 2, -1)
    5 (W, SW, 2, +1)  6 (S, SW, 3, -1)  7 (S, SE, 3, +1)  8 (E, SE, 4, -1)

are tried in this order, a facet only when both neighbours lie in the raster and are valid, in float64:
s1 = (e0 - e1) / px, s2 = (e1 - e2) / px; if s2 < 0: r = 0, s = s1; else if s2 > s1: r = pi / 4,
s = (e0 - e2) / (px * sqrt(2.0)); else r = atan2(s2, s1), s = sqrt(s1 * s1 + s2 * s2).  The facet with the largest s
wins (strict >, so the first of equals), and s must be > 0.  angle64 = af * r + ac * (pi / 2), less 2 pi when it is
>= 2 pi; angle = float32(angle64), 0 when that is >= float32(2 pi); slope = float32(s): drop over distance (TauDEM's
`slp`), not percent.  A valid centre without a winning facet (a pit, a flat, an edge cell without a complete facet)
takes, when `fdr` is given, holds one of the eight D8 codes there and that neighbour lies in the raster and is valid,
angle = float32(k pi / 4) of the code's octant with slope 0; otherwise angle = -1 (no flow), slope = 0.  A NaN or +inf
centre: angle -1, slope 0.  A nodata centre: angle -100, slope -100.  A decision: -inf satisfies <= -100, so a -inf
centre is nodata (-100 / -100) like everywhere else in the package (_lib.nodata_mask, the D8 kernels), not a
non-finite centre; as a neighbour it takes part in no facet either way.  Every receiver with a non-zero share is
strictly lower than the centre.

accumulate.  An angle a >= 0 is decoded as t = float64(a) * 1.2732395447351628 (the float64 nearest 4 / pi): when
|t - rint(t)| <= 2^-20 the cell has one receiver, octant rint(t) mod 8 (float32(k pi / 4) does not land on k exactly);
otherwise k = floor(t), P2 = rint((t - k) * 2^30) and the receivers are octant k mod 8 with share 2^30 - P2 and octant
(k + 1) mod 8 with share P2.  a = -1: no receiver; a = -100: nodata; anything else (NaN, other negatives, beyond
float32(2 pi)) is refused.  c -> d is an edge for each receiver d that lies in the raster and is not nodata; a share
that points off the raster or into nodata leaves the domain; a cell with angle -1 still receives.  The sums are int64
fixed point as in flowacc.accumulate_weighted: q(c) = rint(w(c) * 2^s), T(c) = q(c) + the shares received; a complete
c sends m2 = floor(T * P2 / 2^30) (the 82-bit product taken exactly) to octant k + 1 and m1 = T - m2 to octant k, so
mass is conserved and no T exceeds the sum of q <= 2^52.  result(c) = ldexp(T(c) - q(c), -s): self excluded, as in
flowacc.accumulate; -100 on nodata and on every cell on or downstream of a cycle (its inflow never completes).  The
result does not depend on order or run.  On angles float32(k pi / 4) made from a D8 raster it is
flowacc.accumulate(fdr) exactly (frac_bits=0).

distance_down / hand.  The distance from every cell down the D-infinity flow field to the stream, as TauDEM's
DinfDistDown computes it; TauDEM itself was not at hand when this was written, so what follows is our reading of it
and, with the numpy reference of the test suite, the definition.  Inputs: `angle` under accumulate's contract and
decoding; `river`, taken as int8: a TARGET is a cell with river == 1 whose angle is not -100; `px` finite and > 0;
`dem`, optional float32 heights, taken as given (nodata is decided by `angle` alone).  Three measures: horizontal h,
vertical v, surface s.  For a hop c -> d at octant k: L = px when k is even, else px * 1.4142135623730951 (one float64
product); dz = float64(dem[c]) - float64(dem[d]); S = sqrt(L * L + dz * dz).  Every cell is in one of three states,
reaches / dead / unsettled.  Targets reach, with h = v = s = 0.  A non-target, non-nodata cell without any edge (angle
-1, or every share pointing off the raster or into nodata) is dead.  Any other cell settles once EVERY receiver it has
an edge to is settled: with check_edges=True it reaches iff no share of it leaves the domain and every receiver reaches
(TauDEM's edge-contamination rule), with check_edges=False iff at least one receiver reaches; otherwise it is dead.  A
cell that never settles (on a cycle, or with a receiver that never settles) stays unsettled in either mode.  For a
reaching cell the terms t_j = m(d_j) + hop_m(c -> d_j) are taken over its reaching receivers in the order j = 0, 1
(octant k, octant k + 1).  One term: the value is that term.  Two terms: ave = (float64(w0) * t0 + float64(w1) * t1) *
2^-30 with w0 = 2^30 - P2, w1 = P2; min = t1 if t1 < t0 else t0; max = t1 if t1 > t0 else t0; the statistic is applied
to each measure on its own.  All outputs are float64; nodata and every cell that does not reach hold -100; h >= 0 where
a cell reaches, so h == -100 is the mask.  All arithmetic is IEEE float64 in exactly this association, and a value is a
pure function of its receivers' final values: the result is unique, independent of schedule, rounds and run, and equal
to the numpy reference bit for bit.  A non-finite height on a reaching path gives IEEE's inf / NaN in v and s there; h
is not affected."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_i8p, c_i64p, c_u8p, check, ptr
from .flowacc import _countdown_accumulate, _specific_area

F2PI = np.float32(2.0 * math.pi)


class DinfDistance(tuple):
    """(horizontal, vertical, surface) of distance_down, float64; vertical and surface are None without heights"""
    __slots__ = ()

    def __new__(cls, horizontal, vertical, surface):
        return tuple.__new__(cls, (horizontal, vertical, surface))

    horizontal = property(lambda self: self[0])
    vertical = property(lambda self: self[1])
    surface = property(lambda self: self[2])


class DinfDirection(tuple):
    """(angle, slope) of flow_direction, both float32"""
    __slots__ = ()

    def __new__(cls, angle, slope):
        return tuple.__new__(cls, (angle, slope))

    angle = property(lambda self: self[0])
    slope = property(lambda self: self[1])


def flow_direction(dem, px, fdr=None):
    """D-infinity angle and slope of `dem` (float32-exact heights; a DEM that float32 cannot hold raises ValueError, as
    flowdir.d8 does by default) -> DinfDirection(angle float32, slope float32); the module docstring holds the
    definition.  `fdr` (optional, D8 codes) routes the cells that have no downslope facet.

    With flowdir.d8_conditioned pass the FILLED surface (return_filled=True) together with its fdr: then every flow is
    to a lower cell or along the conditioned D8 codes, and the drainage graph has no cycle."""
    d = _args.raster(dem, "dem")
    p = _args.pixel_size(px)
    f = None if fdr is None else _args.raster(fdr, "fdr", d.shape, "the DEM", dtype=np.uint8)
    d = _lib.dem_f32(d)
    H, W = d.shape
    angle = np.empty((H, W), np.float32)
    slope = np.empty((H, W), np.float32)
    check(_lib.lib().dt_dinf_direction(ptr(d, c_f32p), ptr(f, c_u8p), H, W, p, ptr(angle, c_f32p), ptr(slope, c_f32p)))
    return DinfDirection(angle, slope)


def _angles_f32(angle):
    a = _args.raster(angle, "angle", kinds="iuf", dtype=np.float32)
    ok = (a == np.float32(-1)) | (a == np.float32(-100)) | ((a >= 0) & (a <= F2PI))
    if not ok.all():
        k = int(np.argmin(ok.reshape(-1)))
        raise ValueError("angle %r at flat index %d is neither -1 (no flow), -100 (nodata) nor in [0, float32(2 pi)]"
                         % (a.reshape(-1)[k].item(), k))
    return a


def _accumulate(angle, weights, frac_bits):
    """-> (acc, w or None, s, info): info = {rounds, queue_high, queued, two_receiver_cells}"""
    a = _angles_f32(angle)
    return _countdown_accumulate("dt_dinf_accumulate", a, c_f32p, a.shape, weights, frac_bits, "two_receiver_cells")


def accumulate(angle, weights=None, frac_bits=None):
    """D-infinity contributing area of an angle raster (flow_direction's, or a TauDEM `ang` grid), self excluded, as
    float64: the number of upslope cells by share (weights None), or the sum of their weights; the module docstring
    holds the definition.  weights and frac_bits follow flowacc.accumulate_weighted (finite, >= 0; the default
    frac_bits is flowacc.weight_frac_bits's rule; one with N * rint(max(weights) * 2^frac_bits) > 2^52 is refused).
    Bad arguments raise ValueError before any library call."""
    return _accumulate(angle, weights, frac_bits)[0]


def specific_catchment_area(angle, px, weights=None, frac_bits=None):
    """(accumulate(angle, weights, frac_bits) + the cell's own (quantised) weight) * px: contributing area per unit
    contour length with the cell itself included, TauDEM's `sca` for unit weights; -100 where accumulate gives -100."""
    p = _args.pixel_size(px)
    acc, w, s, _ = _accumulate(angle, weights, frac_bits)
    return _specific_area(acc, w, s, p)


_STATS = {"ave": 0, "min": 1, "max": 2}


def _distance_down(angle, river, px, dem, stat, check_edges, visit_limit):
    """-> (DinfDistance, info): info = {rounds, reach, dead, unsettled}"""
    a = _angles_f32(angle)
    p = _args.pixel_size(px)
    if not isinstance(stat, str) or stat not in _STATS:
        raise ValueError("stat must be 'ave', 'min' or 'max', not %r" % (stat,))
    limit = _args.integer(visit_limit, "_visit_limit", 0, 2 ** 31 - 1)
    r = _args.raster(river, "river", a.shape, "the angle raster", dtype=np.int8)
    d = None if dem is None else _lib.dem_f32(_args.raster(dem, "dem", a.shape, "the angle raster"))
    H, W = a.shape
    h = np.empty((H, W), np.float64)
    v = None if d is None else np.empty((H, W), np.float64)
    s = None if d is None else np.empty((H, W), np.float64)
    info = np.zeros(4, np.int64)
    check(_lib.lib().dt_dinf_distance_down(ptr(a, c_f32p), ptr(r, c_i8p), ptr(d, c_f32p), H, W, p, _STATS[stat],
                                           1 if check_edges else 0, limit, ptr(h, c_f64p), ptr(v, c_f64p),
                                           ptr(s, c_f64p), ptr(info, c_i64p)))
    return DinfDistance(h, v, s), dict(zip(("rounds", "reach", "dead", "unsettled"), (int(x) for x in info)))


def distance_down(angle, river, px, dem=None, stat="ave", check_edges=True, _visit_limit=0):
    """Distance from every cell down the D-infinity flow field of `angle` to the targets (river == 1 and not nodata)
    -> DinfDistance(horizontal, vertical, surface), float64, -100 where a cell does not reach a target and on nodata;
    vertical and surface are None without `dem` (float32-exact heights, as flow_direction).  stat: 'ave' (weighted by
    the flow shares), 'min' or 'max' over the two receivers; check_edges=True: a cell any of whose flow leaves the
    domain or ends without reaching a target does not reach.  The module docstring holds the definition.  Bad
    arguments raise ValueError before any library call."""
    return _distance_down(angle, river, px, dem, stat, check_edges, _visit_limit)[0]


def hand(angle, river, dem, px, stat="ave", check_edges=True, _visit_limit=0):
    """D-infinity height above the nearest drainage: distance_down's vertical raster (float64, -100 where a cell does
    not reach the stream and on nodata) -- what reaches.hydraulic_tables and reaches.inundate take as `hand`."""
    if dem is None:
        raise ValueError("hand needs the heights (dem)")
    return _distance_down(angle, river, px, dem, stat, check_edges, _visit_limit)[0].vertical
