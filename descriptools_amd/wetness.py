"""The SAGA wetness index (net-new; Boehner & Selige 2006, SAGA's "SAGA Wetness Index" module): the topographic wetness
index on a MODIFIED catchment area.  Every other wetness-style descriptor here (TI / MTI, TWI on dinf or mfd specific
catchment area) leaves the contributing area on the cells the flow algorithm routes through -- on a flat valley floor
a one-cell thread or a narrow braid, and hillslope values a few cells beside the channel.  Here each cell's area is
raised to what its largest neighbour can pass on through a slope-dependent "suction" factor, until nothing changes: on
flat ground the factor is close to 1 and the channel's area spreads over the floor, on a slope it is close to 0 and
nothing spreads.

The parameter names follow SAGA's module.  SAGA's source was not consulted: THIS definition, not SAGA's code, is the
contract, and tests/_wetness_ref.py is its reference.

Inputs.  `area`: a 2-D real raster, taken as float64, in any area unit that is > 0 on valid cells.  `suction`: a
float32 raster in [0, 1].  `slope`: float32 radians.

Suction.  s = suction(slope, t=10.0, slope_weight=1.0, slope_offset=radians(0.1), slope_min=0.0), in float64 with one
rounding per operation:
    b = max(float64(slope) + slope_offset, slope_min)
    e = slope_weight * b
    L = log(t), taken once on the host and passed to the kernel, so the library and the reference use the same bits
    s = exp(-((e * exp(exp(e * L))) * L)), that is (1/t)^(e exp(t^e)): the paper's (1/15)^(beta exp(15^beta)) with
        SAGA's default t = 10
rounded to float32; anything below the smallest normal float32 becomes 0.  Cells whose slope is NaN or not in
[0, pi/2) hold -100.

Valid cell.  0 < area < +inf and 0 <= suction <= 1 (NaN fails both).  Every other cell is nodata: it is nobody's
neighbour and holds -100 in every output.

Modified area.  M is the least solution of M(v) = max(A(v), fl(float64(s(v)) * max over the valid 8-neighbours u of
M(u))).  The product is monotone in M(u) and never exceeds it (s <= 1), so taking the maximum first and multiplying once
equals the maximum of the products, the solution is unique, and any relaxation that starts at M = A reaches it, in any
order and any tiling (csrc/dt_wetness.hip relaxes tile by tile); a max-heap Dijkstra returns it too.  The result is held
bit for bit against that Dijkstra; it does not depend on schedule or run.

Index.  swi = float32(log(M / tan(b))), b as above; -100 where the cell is not valid or b >= pi/2.  slope_offset +
slope_min > 0 is required, so tan b > 0.

Refused with ValueError before any library call: a raster that is not 2-D, shapes that differ, 2^31 cells or more, a t
that is not finite and > 1, a slope_weight that is not finite and > 0, a slope_offset or slope_min that is negative or
not finite, both of them 0 for the index.

Recipes.  area from the multiple-flow-direction accumulation or from D8 counts:
    area = mfd.specific_catchment_area(mfd.flow_shares(dem), px)        # or (flowacc + 1) * px
The slope in radians from the percent slope of slope.sloper:
    slope = np.arctan(sloper / 100)
SAGA's other slope type, the catchment slope, is the mean slope of a cell's catchment:
    slope = flowacc.accumulate_weighted(fdr, slope) / count
The index is large where it is wet, so it calibrates against a flood map as
    evaluation.calibration(swi, flood_map, 'over')"""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_i64p, check, ptr
from .device import host_empty

SLOPE_OFFSET = math.radians(0.1)  # SAGA's 0.1 degrees


class ModifiedArea(np.ndarray):
    """the float64 raster of modified_catchment_area.  `info`: the call's counts, {"rounds": rounds of tile visits that
    raised something, "raised": cells with M > A, "tile_visits": visits of 64 x 64 tiles}"""
    info = None

    def __array_finalize__(self, obj):
        self.info = getattr(obj, "info", None)


def _with_info(m, info4):
    out = m.view(ModifiedArea)
    out.info = {"rounds": int(info4[0]), "raised": int(info4[1]), "tile_visits": int(info4[2])}
    return out


def _parameters(t, slope_weight, slope_offset, slope_min, index=False):
    t = _args.at_least(t, "t", 1.0, strict=True)
    w = _args.positive(slope_weight, "slope_weight")
    o = _args.at_least(slope_offset, "slope_offset", 0.0)
    m = _args.at_least(slope_min, "slope_min", 0.0)
    if index and not o + m > 0:
        raise ValueError("slope_offset and slope_min must not both be 0: the index divides by tan(b)")
    return t, w, o, m


def _f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(a, np.float32)


def _f64(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(a, np.float64)


def suction(slope, t=10.0, slope_weight=1.0, slope_offset=SLOPE_OFFSET, slope_min=0.0):
    """The suction factor of a slope raster in radians -> float32 in [0, 1], -100 where the slope is NaN or not in
    [0, pi/2); the module docstring holds the definition."""
    sl = _args.raster(slope, "slope", kinds="biuf")
    t, w, o, m = _parameters(t, slope_weight, slope_offset, slope_min)
    sl = _f32(sl)
    H, W = sl.shape
    out = host_empty((H, W), np.float32)
    check(_lib.lib().dt_wetness_suction(ptr(sl, c_f32p), H, W, t, w, o, m, ptr(out, c_f32p)))
    return out


def modified_catchment_area(area, suction, _visit_limit=0):
    """The modified catchment area of `area` under `suction` -> ModifiedArea (float64, -100 on nodata) with `.info`; the
    module docstring holds the definition.  `_visit_limit` (tests) caps the sweeps a workgroup makes per tile visit;
    the output does not depend on it."""
    a = _args.raster(area, "area", kinds="biuf")
    s = _args.raster(suction, "suction", shape=a.shape, other="area", kinds="biuf")
    limit = _args.integer(_visit_limit, "_visit_limit", 0, 2 ** 31 - 1)
    a, s = _f64(a), _f32(s)
    H, W = a.shape
    out = host_empty((H, W), np.float64)
    info = np.zeros(4, np.int64)
    check(_lib.lib().dt_wetness_modified_area(ptr(a, c_f64p), ptr(s, c_f32p), H, W, limit, ptr(out, c_f64p),
                                              ptr(info, c_i64p)))
    return _with_info(out, info)


def saga_wetness_index(area, slope, t=10.0, slope_weight=1.0, slope_offset=SLOPE_OFFSET, slope_min=0.0,
                       modified=False, _visit_limit=0):
    """The SAGA wetness index of `area` and `slope` (radians) -> float32, -100 on nodata; with `modified=True`
    (swi, ModifiedArea).  The suction, the modified area and the index are one library call: nothing comes back to the
    host between them.  The module docstring holds the definition."""
    a = _args.raster(area, "area", kinds="biuf")
    sl = _args.raster(slope, "slope", shape=a.shape, other="area", kinds="biuf")
    t, w, o, m = _parameters(t, slope_weight, slope_offset, slope_min, index=True)
    limit = _args.integer(_visit_limit, "_visit_limit", 0, 2 ** 31 - 1)
    a, sl = _f64(a), _f32(sl)
    H, W = a.shape
    swi = host_empty((H, W), np.float32)
    mod = host_empty((H, W), np.float64) if modified else None
    info = np.zeros(4, np.int64)
    check(_lib.lib().dt_wetness_saga(ptr(a, c_f64p), ptr(sl, c_f32p), H, W, t, w, o, m, limit, ptr(swi, c_f32p),
                                     ptr(mod, c_f64p), None, ptr(info, c_i64p)))
    return (swi, _with_info(mod, info)) if modified else swi
