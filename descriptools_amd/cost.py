"""Cost distance, cost allocation and back-links over a friction raster (net-new; the GIS "cost distance / cost
allocation / cost back link", GRASS r.cost, WhiteboxTools CostDistance): the least accumulated cost from every cell to a
river cell, going round barriers and slowing on rough ground -- the fourth distance beside the D8 flow path
(flowhand.flow_hand_index), the D-infinity flow field (dinf.distance_down) and the straight line
(proximity.nearest_river).

Inputs.  `friction`: a 2-D real raster, taken as float32.  `sources`: a raster of the same shape, taken as int8.  `px`:
finite and > 0.  `connectivity`: 8 (default) or 4.

Passable cells.  A cell is passable iff 0 < friction < +inf: zero, negatives (the -100 sentinel included), NaN and +inf
are barriers.  A diagonal move between two barrier cells is allowed, as in the GIS tools.

Sources.  A source is a passable cell with sources == 1 (the river rule of proximity and flow_hand_index).

Edge cost.  For adjacent passable cells u and v, in float64 with one rounding per operation,
w(u, v) = step * ((f(u) + f(v)) * 0.5), step = px for a cardinal move and px * 1.4142135623730951 for a diagonal one
(connectivity 4: cardinal moves only).  w is symmetric.

Cost.  A is the greatest solution of A(s) = 0 at every source s and A(v) = min over neighbours u of fl(A(u) + w(u, v))
elsewhere.  fl(a + w) is monotone in a and w >= 0, so the solution is unique: Dijkstra returns it, and so does any
relaxation that starts at +inf, in any order and any tiling (csrc/dt_cost.hip relaxes tile by tile).  The result is held
bit for bit against a heap Dijkstra; it does not depend on order or run.

Back-link.  backlink(v) is the ESRI D8 code (1 E, 2 SE, 4 S, 8 SW, 16 W, 32 NW, 64 N, 128 NE) of one neighbour u with
A(u) < A(v) and fl(A(u) + w(u, v)) == A(v); among several, the first in the scan order NW, N, NE, W, E, SW, S, SE.
Sources, barriers and unreached cells hold 0.  A strictly falls along the links, so they form a forest rooted at the
sources.

Allocation.  indices(v) is the flat index of the source at the root of v's back-link tree; a source's is itself.

Degenerate case.  A reached non-source cell has no such neighbour only when rounding absorbs a whole edge cost
(friction [[1, 1e30, 1e-30, 1e-30]] with the first cell as source leaves the last cell without a link).  The call counts
these cells and the functions here raise RuntimeError naming the count; the device tier raises DT_STATUS_NO_BACKLINK
(256) on the context.

Outputs.  cost float64, indices int64, backlink uint8; barriers and unreached cells hold -100, -100 and 0.

Refused with ValueError before any library call: a raster that is not 2-D, shapes that differ, 2^31 cells or more, a px
that is not finite and > 0, a connectivity other than 4 or 8.

Recipes.  indices feeds flowhand.hand_calculator, gfi.gfi_calculator, gfi.river_accumulation, reaches.catchments and
reaches.inundate unchanged, as proximity's do.  backlink is a valid D8 raster for watershed, flowacc and streams:
watershed.basins(backlink) reproduces indices on the reached cells.  The attenuated "bathtub" inundation, whose water
level falls with the path travelled over land, is one line on top:
    depth = np.where(cost >= 0, np.maximum(level - attenuation * cost - dem, 0), 0)"""
import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_i8p, c_i64p, c_u8p, check, ptr
from .device import host_empty
from .flowhand import hand_calculator


class CostDistance(tuple):
    """(cost float64, indices int64, backlink uint8 or None) of cost_distance.  `info`: the call's counts, {"rounds":
    rounds of tile visits that lowered something, "reached": reached cells, "tile_visits": visits of 64 x 64 tiles}"""

    def __new__(cls, cost, indices, backlink, info=None):
        self = tuple.__new__(cls, (cost, indices, backlink))
        self.info = info
        return self

    cost = property(lambda self: self[0])
    indices = property(lambda self: self[1])
    backlink = property(lambda self: self[2])


def cost_distance(friction, sources, px, connectivity=8, backlink=False, _visit_limit=0):
    """Least accumulated cost to, and flat index of, the source a cell is reached from over `friction`
    -> CostDistance(cost float64, indices int64, backlink uint8 or None); the module docstring holds the definition.
    `backlink=True` returns the back-link raster too.  `_visit_limit` (tests) caps the sweeps a workgroup makes per tile
    visit; the outputs do not depend on it."""
    f = _args.raster(friction, "friction", kinds="biuf")
    s = _args.raster(sources, "sources", shape=f.shape, other="friction")
    p = _args.pixel_size(px)
    conn = _args.connectivity(connectivity)
    limit = _args.integer(_visit_limit, "_visit_limit", 0, 2 ** 31 - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.ascontiguousarray(f, np.float32)
        s = np.ascontiguousarray(s, np.int8)
    H, W = f.shape
    cost = host_empty((H, W), np.float64)
    indices = host_empty((H, W), np.int64)
    link = host_empty((H, W), np.uint8) if backlink else None
    info = np.zeros(4, np.int64)
    check(_lib.lib().dt_cost_distance(ptr(f, c_f32p), ptr(s, c_i8p), H, W, p, conn, limit, ptr(cost, c_f64p),
                                      ptr(indices, c_i64p), ptr(link, c_u8p), ptr(info, c_i64p)))
    if info[2]:
        raise RuntimeError("cost_distance: %d reached cell(s) without a back-link: rounding absorbed a whole edge cost "
                           "(the friction spans more orders of magnitude than float64 resolves)" % int(info[2]))
    return CostDistance(cost, indices, link,
                        {"rounds": int(info[0]), "reached": int(info[1]), "tile_visits": int(info[3])})


def cost_hand(dem, river, px, friction=None, connectivity=8):
    """The least-cost twin of proximity.euclidean_hand -> (cost float64, indices int64, hand in the DEM's dtype), the
    same -100 conventions: hand is the height above the river cell that is nearest by cost.  Cells that
    _lib.nodata_mask(dem) calls nodata are barriers; friction=None means 1 on every valid cell: the geodesic distance
    that stays on the data."""
    d = _args.raster(dem, "dem")
    nod = _lib.nodata_mask(d, d.shape) != 0
    if friction is None:
        f = np.where(nod, np.float32(0), np.float32(1))
    else:
        f = _args.raster(friction, "friction", shape=d.shape, other="dem", kinds="biuf")
        with np.errstate(over="ignore", invalid="ignore"):
            f = np.where(nod, np.float32(0), np.asarray(f, np.float32))
    cost, indices, _ = cost_distance(f, river, px, connectivity)
    return cost, indices, hand_calculator(dem, indices)
