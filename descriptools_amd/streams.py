"""Stream order of a D8 channel network (net-new): Strahler order, Shreve magnitude and stream links, on the GPU.

The network is given as a river mask, typically river = fac > threshold from the chain.  Definition (the kernels
in csrc/dt_streams.hip and the tests hold to it):

* Network graph.  The nodes are the cells with river != 0.  A network cell c has the edge c -> d when its code is
  one of the eight ESRI D8 codes (1 E, 2 SE, 4 S, 8 SW, 16 W, 32 NW, 64 N, 128 NE) and points at an in-raster cell d
  that is also in the network.  Otherwise c is a network outlet: its code is 0 or not a D8 code, or it points off the
  raster or at a cell outside the network.  A cell's children are the network cells with an edge into it.
* Cycles.  A network cell that in-degree peeling on this graph never removes lies on a D8 cycle of network cells.
  It gets -100 in every output.
* Strahler (int8).  0 off the network.  A network cell with no children gets 1.  Otherwise, with m the largest
  order among its children, it gets m + 1 if at least two children have order m, and m if only one does.
* Shreve (int64).  0 off the network.  A cell with no children gets 1; any other cell the sum of its children's
  magnitudes.
* Link (int64).  -100 off the network and on cycles.  For a network cell, the flat index y * W + x of the head of its
  link.  A cell is its own head if its number of children is not exactly 1 (a source or a confluence); otherwise it
  takes the head of its only child.  Strahler and Shreve are constant along a link.

All three are integers: results are exact and do not depend on order, tiling or run.  Nodata reaches this op only
through river (the chain's river is 0 wherever fac is -100).

Users of a resident chain call dt_dev_stream_order on chain.p("fdr") / chain.p("river")."""
from collections import namedtuple

import numpy as np

from . import _args, _lib
from ._lib import c_i8p, c_i64p, c_u8p, check, ptr

StreamNetwork = namedtuple("StreamNetwork", ["strahler", "shreve", "link"])


def _checked(fdr, river):
    """(fdr as C-contiguous uint8, river as C-contiguous int8 0/1); ValueError before any library call.  No cap on
    the cells here: the size limit is the library's (dt_check_so)"""
    f = _args.raster(fdr, "fdr", cap=False, dtype=np.uint8)
    r = _args.raster(river, "river", f.shape, "the direction raster", cap=False, kinds="biu")
    return f, np.ascontiguousarray(r != 0, np.int8)


def stream_network(fdr, river):
    """Strahler order (int8), Shreve magnitude (int64) and link head (int64 flat index) of every cell of the network
    river != 0 on the D8 raster fdr, as StreamNetwork(strahler, shreve, link).  See the module docstring for the
    definition: 0 / 0 / -100 off the network, -100 / -100 / -100 on D8 cycles of network cells."""
    f, r = _checked(fdr, river)
    H, W = f.shape
    so = np.empty((H, W), np.int8)
    sh = np.empty((H, W), np.int64)
    lk = np.empty((H, W), np.int64)
    check(_lib.lib().dt_stream_order(ptr(f, c_u8p), ptr(r, c_i8p), H, W, ptr(so, c_i8p), ptr(sh, c_i64p),
                                     ptr(lk, c_i64p)))
    return StreamNetwork(so, sh, lk)


def strahler(fdr, river):
    """Strahler order (int8) of the network river != 0 on fdr: 0 off the network, -100 on D8 cycles"""
    f, r = _checked(fdr, river)
    H, W = f.shape
    so = np.empty((H, W), np.int8)
    check(_lib.lib().dt_stream_order(ptr(f, c_u8p), ptr(r, c_i8p), H, W, ptr(so, c_i8p), None, None))
    return so


def shreve(fdr, river):
    """Shreve magnitude (int64) of the network river != 0 on fdr: 0 off the network, -100 on D8 cycles"""
    return stream_network(fdr, river).shreve
