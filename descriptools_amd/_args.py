"""The argument checks the op modules share.  Every one raises ValueError and touches no library, so an op that runs
them first refuses a bad argument before any library call.  The op modules call them as _args.<name>(...): importing
the names would export them through the descriptools/ alias modules.

What stays with the op modules is what a value means to them: != 0 for masks and rivers, the int32 range of ids, the
weights contract of flowacc._weights_f64, the angle contract of dinf."""
import math

import numpy as np

MAX_CELLS = 2 ** 31
# every partial sum of quantised weights stays <= 2^52: the countdown's sum field holds it and float64 converts it
# without rounding
_SUM_BITS = 52
# frac_bits is bounded as the C ABI bounds it (dt_dev_flowacc_weighted)
_FRAC_BITS_MAX = 2200

_KINDS = {"iu": "an integer", "biu": "a bool or integer", "iuf": "a real", "biuf": "a real or integer"}


def raster(a, what, shape=None, other=None, cap=True, kinds=None, dtype=None):
    """a as a 2-D array, C-contiguous and of `dtype` when one is given.  ValueError, in this order, for another rank,
    for a shape other than `shape` (the shape of the raster that `other` names in words: "the direction raster"), with
    `cap` for 2^31 cells or more, and for a dtype whose kind is not in `kinds` (a key of _KINDS)"""
    r = np.asarray(a)
    if r.ndim != 2:
        raise ValueError("%s must be a 2-D raster, not of shape %s" % (what, r.shape))
    if shape is not None and r.shape != shape:
        raise ValueError("%s has shape %s, %s %s" % (what, r.shape, other, shape))
    if cap and r.size >= MAX_CELLS:
        raise ValueError("%s has %d cells; a raster must have fewer than 2^31" % (what, r.size))
    if kinds is not None and r.dtype.kind not in kinds:
        raise ValueError("%s must be of %s dtype, not %s" % (what, _KINDS[kinds], r.dtype))
    return r if dtype is None else np.ascontiguousarray(r, dtype)


def pixel_size(px):
    """px as a float; ValueError unless it is a number (not a bool), finite and > 0"""
    try:
        p = math.nan if isinstance(px, (bool, np.bool_)) else float(px)
    except (TypeError, ValueError):
        p = math.nan
    if not (math.isfinite(p) and p > 0):
        raise ValueError("px must be a finite number > 0, not %r" % (px,))
    return p


def positive(v, what):
    """v as a float; ValueError unless it is a number (not a bool), finite and > 0"""
    try:
        p = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
    except (TypeError, ValueError):
        p = math.nan
    if not (math.isfinite(p) and p > 0):
        raise ValueError("%s must be a finite number > 0, not %r" % (what, v))
    return p


def at_least(v, what, lo, strict=False):
    """v as a float; ValueError unless it is a number (not a bool), finite and >= lo (`strict`: > lo)"""
    try:
        p = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
    except (TypeError, ValueError):
        p = math.nan
    if not (math.isfinite(p) and (p > lo if strict else p >= lo)):
        raise ValueError("%s must be a finite number %s %g, not %r" % (what, ">" if strict else ">=", lo, v))
    return p


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def integer(v, what, lo, hi=None):
    """v as an int; ValueError unless it is an integer (not a bool) with lo <= v, and v <= hi when there is a hi"""
    if not _is_int(v) or int(v) < lo or (hi is not None and int(v) > hi):
        bound = ">= %d" % lo if hi is None else "in [%d, %d]" % (lo, hi)
        raise ValueError("%s must be an integer %s, not %r" % (what, bound, v))
    return int(v)


def connectivity(c):
    """4 or 8 as an int; ValueError for anything else"""
    if not _is_int(c) or int(c) not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, not %r" % (c,))
    return int(c)


def _default_frac_bits(n, wmax):
    """s = 51 - ceil(log2 n) - e with 2^e <= wmax < 2^(e+1); 0 when every weight is 0"""
    if wmax == 0:
        return 0
    e = math.frexp(wmax)[1] - 1
    return _SUM_BITS - 1 - (n - 1).bit_length() - e


def frac_bits(n, top, frac_bits, bound_text, default_text):
    """The fixed-point scale s of a sum over n cells whose largest term is `top`: the default (the finest s with
    n * rint(top * 2^s) <= 2^52) for frac_bits None, else frac_bits itself; ValueError unless that is an integer (not
    a bool) within +-_FRAC_BITS_MAX that keeps the bound.  The last message reads "frac_bits=<s> is too fine<bound_text>
    exceeds 2^52 (<default_text> <the default>)"."""
    if frac_bits is None:
        return _default_frac_bits(n, top) if n else 0
    if not _is_int(frac_bits):
        raise ValueError("frac_bits must be an integer, not %r" % (frac_bits,))
    s = int(frac_bits)
    if not -_FRAC_BITS_MAX <= s <= _FRAC_BITS_MAX:
        raise ValueError("frac_bits must lie in [%d, %d], not %d" % (-_FRAC_BITS_MAX, _FRAC_BITS_MAX, s))
    with np.errstate(over="ignore"):
        qmax = np.rint(np.ldexp(top, s))
    if not np.isfinite(qmax) or n * int(qmax) > 2 ** _SUM_BITS:
        raise ValueError("frac_bits=%d is too fine%s exceeds 2^52 (%s %d)"
                         % (s, bound_text, default_text, _default_frac_bits(n, top)))
    return s
