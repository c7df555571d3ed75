"""Connected regions of a mask on the GPU (net-new): labels, sizes, and the selection of regions by seed and by size --
what turns a cell-by-cell flood map (evaluation.binary_map, reaches.inundate) into the extent that has a wet path to the
channel, and what a sieve filter does.

Definitions (the kernels in csrc/dt_regions.hip, the C header and the tests hold to them).  Rasters are H x W,
row-major, flat index y * W + x, N = H * W < 2^31.

* Foreground.  mask is a 2-D raster of bool or integer dtype; a cell is foreground when mask != 0.  seeds follows the
  same rule.  The library is handed uint8(mask != 0).  Float rasters are refused: write river == 1 or depth > 0.
* Adjacency.  connectivity=8 (the default) uses the eight neighbours, connectivity=4 the four cardinal ones.  Two
  foreground cells are in the same region when a chain of adjacent foreground cells joins them.
* Label.  label[c] (int64) = the smallest flat index among the cells of c's region; -100 on background.
* Size.  size[c] (int64) = the number of cells of c's region; 0 on background.
* Selection.  A region is seeded when one of its own cells has seeds != 0; a seed on a background cell seeds nothing.
  keep[c] (uint8) = 1 when c is foreground, no seeds were given or c's region is seeded, and size[c] >= min_cells;
  else 0.

All of these are functions of the inputs alone: no choice of schedule, tile size or run shows in a single bit.  The work
is a fixed number of launches whatever the mask holds (a union-find over TILE x TILE tiles, then over their seams, whose
root is the region's smallest cell -- the label itself).  reaches.inundate_connected applies the selection to HAND
inundation.  Bad arguments raise ValueError before any library call; there is no CPU path.  Users of a resident chain
call dt_dev_regions_label / dt_dev_regions_select on device rasters."""
from collections import namedtuple

import numpy as np

from . import _args, _lib
from ._lib import c_i64p, c_u8p, check, ptr
from .device import host_empty

Regions = namedtuple("Regions", ["label", "size"])

TILE = 64  # DT_REGIONS_TILE: the edge of the tiles the kernels solve in LDS (tests place cells on their seams)


def _mask(a, what, shape=None):
    """a as uint8(a != 0), C-contiguous; ValueError unless it is a 2-D bool / integer raster of fewer than 2^31 cells
    (and of `shape`).  A float raster is refused: compare first, river == 1 or depth > 0"""
    return np.ascontiguousarray(_args.raster(a, what, shape, "the mask", kinds="biu") != 0, np.uint8)


def _min_cells(min_cells):
    # no region has 2^31 cells: every larger bound keeps nothing either
    return min(_args.integer(min_cells, "min_cells", 1), _args.MAX_CELLS)


def label(mask, connectivity=8, sizes=False):
    """The int64 label raster of mask != 0 (the smallest flat index of the cell's region, -100 on background), or with
    sizes=True Regions(label, size); see the module docstring."""
    m = _mask(mask, "mask")
    cn = _args.connectivity(connectivity)
    H, W = m.shape
    lab = host_empty((H, W), np.int64)
    size = host_empty((H, W), np.int64) if sizes else None
    check(_lib.lib().dt_regions_label(ptr(m, c_u8p), H, W, cn, ptr(lab, c_i64p), ptr(size, c_i64p)))
    return Regions(lab, size) if sizes else lab


def _select(m, s, cn, mc):
    H, W = m.shape
    keep = host_empty((H, W), np.uint8)
    check(_lib.lib().dt_regions_select(ptr(m, c_u8p), ptr(s, c_u8p), H, W, cn, mc, ptr(keep, c_u8p)))
    return keep


def connected(mask, seeds, connectivity=8, min_cells=1):
    """uint8 raster: 1 on the foreground cells whose region holds a cell with seeds != 0 and has at least min_cells
    cells, 0 elsewhere; see the module docstring."""
    m = _mask(mask, "mask")
    s = _mask(seeds, "seeds", m.shape)
    return _select(m, s, _args.connectivity(connectivity), _min_cells(min_cells))


def sieve(mask, min_cells, connectivity=8):
    """uint8 raster: 1 on the foreground cells whose region has at least min_cells cells, 0 elsewhere."""
    m = _mask(mask, "mask")
    return _select(m, None, _args.connectivity(connectivity), _min_cells(min_cells))
