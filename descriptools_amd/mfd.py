"""Multiple-flow-direction (MFD) flow shares and contributing area (net-new; Quinn et al. 1991, Freeman 1991, Holmgren
1994): the flow of a cell spread over every lower neighbour in proportion to a power of the slope.

Share raster.  uint16[H, W, 8], C-contiguous; the last axis is the octant in dinf's convention, the neighbour at angle
k pi / 4 counter-clockwise from east with rows growing to the south: E, NE, N, NW, W, SW, S, SE -- the D8 codes 1, 128,
64, 32, 16, 8, 4, 2.  A share is stored in units of 2^-15 (a single receiver holds 32768, which fits a uint16 without
an escape value).  A cell whose eight slots are all 0xFFFF is nodata.  In any other cell every slot is <= 32768 and
the slots sum to 32768, or to 0 when the cell has no receiver.

flow_shares.  A height is valid when it is finite and > -100; <= -100 is nodata, which includes -inf, as everywhere in
the package.  A nodata centre stores 0xFFFF in all eight slots; a NaN or +inf centre stores eight zeros.  The receivers
of a valid centre z0 are the neighbours that lie in the raster, are valid and are strictly lower.  All arithmetic is
float64 on the float32 heights.  For each receiver, in octant order k = 0..7: d_k = z0 - z_k; g_k = d_k for even k and
d_k / 1.4142135623730951 for odd k; u_k = g_k / gmax with gmax the largest g, so u is in (0, 1] and nothing overflows;
f_k = u_k^p, taken by repeated multiplication when `exponent` is integer-valued (f = 1.0, then f = f * u, p times:
IEEE-exact, so the GPU and numpy agree bit for bit) and as pow(u, p) otherwise (the GPU's pow and libm's may round
differently: a share may then differ by one unit in a handful of cells of a raster); with `contour` f_k is multiplied
by 0.5 for even k and by 0.35355339059327373 for odd k (Quinn's contour lengths).  F = the sum of the f_k from left to
right in octant order (a neighbour that is no receiver adds 0.0), r_k = f_k / F.  The main receiver is the one with the
largest f (strict >, so the first of equals in octant order).  Every other receiver stores P_k = floor(ldexp(r_k, 15)),
and is dropped when that is 0; the main receiver stores 32768 less the sum of the others.  The pixel size appears
nowhere: with square cells it cancels out of every share, so flow_shares takes no `px`.  A valid centre without a
lower neighbour (a pit, a flat, a cell with a complete rim) takes, when `fdr` is given, holds one of the eight D8
codes there and that neighbour lies in the raster and is valid, 32768 in the code's octant; otherwise eight zeros.

accumulate.  The result is a function of the share raster alone.  c -> d is an edge for each octant k with P_k > 0
whose neighbour d lies in the raster and is not nodata; a share that points off the raster or into nodata leaves the
domain; a cell without a receiver still receives.  The main receiver of a cell is the slot with the largest P, the
first of equals in octant order.  The sums are int64 fixed point as in flowacc.accumulate_weighted:
q(c) = rint(w(c) * 2^s), T(c) = q(c) + the shares received; a complete c sends m_k = floor(T * P_k / 2^15) to every
receiver k but the main one and T less the sum of those m_k to the main one, so mass is conserved and no T exceeds
the sum of q <= 2^52.  result(c) = ldexp(T(c) - q(c), -s): self excluded, as in flowacc.accumulate; -100 on nodata and
on every cell on or downstream of a cycle (its inflow never completes).  The result does not depend on order or run.
On d8_shares(fdr) with frac_bits=0 it is flowacc.accumulate(fdr) exactly."""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_u8p, c_u16p, check, ptr
from .flowacc import _countdown_accumulate, _specific_area

UNIT = 32768
NODATA_SLOT = 0xFFFF
OCTANT_CODES = (1, 128, 64, 32, 16, 8, 4, 2)


def _exponent(exponent):
    try:
        p = math.nan if isinstance(exponent, (bool, np.bool_)) else float(exponent)
    except (TypeError, ValueError):
        p = math.nan
    if not (math.isfinite(p) and 0.0 <= p <= 64.0):
        raise ValueError("exponent must be a finite number in [0, 64], not %r" % (exponent,))
    return p


def flow_shares(dem, exponent=1.1, contour=False, fdr=None):
    """MFD share raster of `dem` (float32-exact heights; a DEM that float32 cannot hold raises ValueError, as
    dinf.flow_direction does) -> uint16[H, W, 8]; the module docstring holds the definition.  exponent: finite, in
    [0, 64] (1.1: Freeman; 1: Quinn; larger values concentrate the flow on the steepest neighbours); contour=True
    weights the shares by Quinn's contour lengths; `fdr` (optional, D8 codes) routes the cells that have no lower
    neighbour.  There is no `px`: with square cells the pixel size cancels out of every share.

    With flowdir.d8_conditioned pass the FILLED surface (return_filled=True) together with its fdr: then every flow is
    to a lower cell or along the conditioned D8 codes, and the drainage graph has no cycle."""
    d = _args.raster(dem, "dem")
    p = _exponent(exponent)
    if not isinstance(contour, (bool, np.bool_)):
        raise ValueError("contour must be a bool, not %r" % (contour,))
    f = None if fdr is None else _args.raster(fdr, "fdr", d.shape, "the DEM", dtype=np.uint8)
    d = _lib.dem_f32(d)
    H, W = d.shape
    shares = np.empty((H, W, 8), np.uint16)
    check(_lib.lib().dt_mfd_shares(ptr(d, c_f32p), ptr(f, c_u8p), H, W, p, 1 if contour else 0, ptr(shares, c_u16p)))
    return shares


def d8_shares(fdr):
    """The share raster that sends everything along the D8 codes of `fdr`: 32768 in the code's octant, 0 elsewhere;
    a cell without one of the eight codes has no receiver.  Host-side numpy."""
    f = _args.raster(fdr, "fdr", kinds="biu")
    shares = np.zeros(f.shape + (8,), np.uint16)
    for k, code in enumerate(OCTANT_CODES):
        shares[..., k][f == code] = UNIT
    return shares


def _shares_u16(shares):
    s = np.asarray(shares)
    if s.ndim != 3 or s.shape[2] != 8:
        raise ValueError("shares must be a raster of shape (H, W, 8), not %s" % (s.shape,))
    if s.shape[0] * s.shape[1] >= _args.MAX_CELLS:
        raise ValueError("shares has %d cells; a raster must have fewer than 2^31" % (s.shape[0] * s.shape[1]))
    if s.dtype != np.uint16:
        raise ValueError("shares must be of dtype uint16, not %s" % s.dtype)
    s = np.ascontiguousarray(s)
    nodata = (s == NODATA_SLOT).all(axis=2)
    total = s.sum(axis=2, dtype=np.int64)
    ok = nodata | ((s <= UNIT).all(axis=2) & ((total == 0) | (total == UNIT)))
    if not ok.all():
        k = int(np.argmin(ok.reshape(-1)))
        raise ValueError("the shares %r at flat index %d are neither eight 0xFFFF (nodata) nor eight values <= 32768 "
                         "that sum to 0 or to 32768" % (s.reshape(-1, 8)[k].tolist(), k))
    return s


def _accumulate(shares, weights, frac_bits):
    """-> (acc, w or None, s, info): info = {rounds, queue_high, queued, multi_receiver_cells}"""
    sh = _shares_u16(shares)
    return _countdown_accumulate("dt_mfd_accumulate", sh, c_u16p, sh.shape[:2], weights, frac_bits,
                                 "multi_receiver_cells")


def accumulate(shares, weights=None, frac_bits=None):
    """MFD contributing area of a share raster (flow_shares', d8_shares', or a caller's own under the contract of the
    module docstring), self excluded, as float64: the number of upslope cells by share (weights None), or the sum of
    their weights.  weights and frac_bits follow flowacc.accumulate_weighted (finite, >= 0; the default frac_bits is
    flowacc.weight_frac_bits's rule; one with N * rint(max(weights) * 2^frac_bits) > 2^52 is refused).  Bad arguments
    raise ValueError before any library call."""
    return _accumulate(shares, weights, frac_bits)[0]


def specific_catchment_area(shares, px, weights=None, frac_bits=None):
    """(accumulate(shares, weights, frac_bits) + the cell's own (quantised) weight) * px: contributing area per unit
    contour length with the cell itself included; -100 where accumulate gives -100.  The topographic wetness index is
    np.log(sca / np.tan(slope_radians)) on it."""
    p = _args.pixel_size(px)
    acc, w, s, _ = _accumulate(shares, weights, frac_bits)
    return _specific_area(acc, w, s, p)
