"""Decayed, retention-limited and transport-limited accumulation (net-new; TauDEM's DinfDecayAccum, DinfTransLimAccum
and retention-limited flow, and fill-and-spill of depressions along the flow graph): an accumulation in which a cell
passes on only a function of what it holds.

Definition.  The graph, the edges, nodata, the main receiver, q(c) = rint(w(c) * 2^s), the split rule and the -100 on
or below a cycle are exactly those of mfd.accumulate (on a share raster) and of dinf.accumulate (on an angle raster);
the only change is what a complete cell sends.

    T(c) = q(c) + arrivals      the load
    O(c) = f(T(c), p(c))        the outflow
    R(c) = T(c) - O(c)          retained

The receivers get the existing split applied to O instead of T: MFD sends floor(O * P_k / 2^15) to every receiver but
the main one and the rest of O to the main one; D-infinity sends m2 = floor(O * P2 / 2^30) to octant k + 1 and O - m2
to octant k.  p is a float64 raster, read and quantised when the cell completes.  The three transfer functions:

    transfer   parameter                        quantised                          O
    "decay"    fraction passed on, in [0, 1]    D = rint(ldexp(p, 30))             floor(T * D / 2^30)
    "retain"   capacity >= 0, +inf allowed      C = min(rint(ldexp(p, s)), 2^53)   T - C if T > C, else 0
    "limit"    capacity >= 0, +inf allowed      the same C                         min(T, C)

The decay product is taken as (T >> 30) * D + (((T & (2^30 - 1)) * D) >> 30), exact in 64 bits.  The parameter 1 for
decay, 0 for retain and +inf for limit are identities: O = T.  A parameter outside its contract (NaN, negative, a
decay above 1) is refused here before any library call; on the device tier it acts as the identity and raises
DT_STATUS_BAD_PARAM (512).  A cell without receivers still has its O and R; its O leaves the domain, as does the part
of a share that points off the raster or into nodata.  O <= T for all three, so no sum exceeds the accumulations' bound
(the sum of q <= 2^52).

Four outputs, all float64, all ldexp(., -s), all -100 where accumulate gives -100:

    inflow     T - q   what accumulate returns when the transfer is an identity
    load       T
    outflow    O
    retained   R

The sums are integers: the result is exact and does not depend on order, rounds or run."""
import numpy as np

from . import _args, _lib, mfd, watershed
from ._lib import c_f32p, c_f64p, c_i64p, c_u16p, check, ptr
from .dinf import _angles_f32
from .flowacc import _weights_f64

TRANSFERS = {"decay": 1, "retain": 2, "limit": 3}
OUTPUTS = ("inflow", "load", "outflow", "retained")


class Routed(dict):
    """{name: float64[H, W]} in the order asked for; .info = {rounds, queue_high, queued, and multi_receiver_cells
    (shares, D8 codes) or two_receiver_cells (angles)}, as mfd._accumulate and dinf._accumulate give it"""
    info = None


def _outputs(outputs):
    if isinstance(outputs, str) or not hasattr(outputs, "__iter__"):
        raise ValueError("outputs must be a sequence of names from %s, not %r" % (OUTPUTS, outputs))
    names = tuple(outputs)
    if not names:
        raise ValueError("outputs is empty; name at least one of %s" % (OUTPUTS,))
    for n in names:
        if not isinstance(n, str) or n not in OUTPUTS:
            raise ValueError("output %r is not one of %s" % (n, OUTPUTS))
    if len(set(names)) != len(names):
        raise ValueError("outputs names an output twice: %r" % (names,))
    return names


def _flow(flow):
    """-> (entry, raster, ctypes pointer type, (H, W), the name of info's fourth count)"""
    f = np.asarray(flow)
    if f.ndim == 3:
        s = mfd._shares_u16(f)
        return "dt_mfd_route", s, c_u16p, s.shape[:2], "multi_receiver_cells"
    if f.ndim == 2 and f.dtype == np.uint8:
        s = mfd.d8_shares(_args.raster(f, "flow"))
        return "dt_mfd_route", s, c_u16p, s.shape[:2], "multi_receiver_cells"
    if f.ndim == 2 and f.dtype == np.float32:
        a = _angles_f32(f)
        return "dt_dinf_route", a, c_f32p, a.shape, "two_receiver_cells"
    raise ValueError("flow must be a uint16 share raster of shape (H, W, 8), a float32 D-infinity angle raster or a "
                     "uint8 D8 code raster, not %s of shape %s" % (f.dtype, f.shape))


def _param_f64(param, transfer, shape, what="param"):
    """the parameter raster of `transfer` -> C-contiguous float64; ValueError outside the contract"""
    a = np.asarray(param)
    if a.shape != shape:
        raise ValueError("%s has shape %s, the flow raster %s" % (what, a.shape, shape))
    if a.dtype.kind not in "biuf":
        raise ValueError("%s must be of a real or integer dtype, not %s" % (what, a.dtype))
    p = np.ascontiguousarray(a, dtype=np.float64)
    ok = (p >= 0) & (p <= 1) if transfer == "decay" else p >= 0  # NaN fails both
    if not ok.all():
        k = int(np.argmin(ok.reshape(-1)))
        raise ValueError("%s holds %r at flat index %d: %s" % (what, p.reshape(-1)[k].item(), k, (
            "a decay is the fraction passed on, in [0, 1]" if transfer == "decay"
            else "a capacity is >= 0 (+inf: no limit)")))
    return p


def route(flow, param, transfer, weights=None, frac_bits=None, outputs=("outflow",)):
    """Route the weights down `flow` under the transfer function `transfer` ('decay', 'retain' or 'limit') with the
    per-cell parameter raster `param` -> Routed {name: float64[H, W]} of the `outputs` asked for (any of 'inflow',
    'load', 'outflow', 'retained', each once), with .info; the module docstring holds the definition.

    flow: a uint16 [H, W, 8] share raster (mfd's contract), a float32 [H, W] D-infinity angle raster (dinf's
    contract) or a uint8 [H, W] D8 code raster (taken through mfd.d8_shares).  weights and frac_bits follow
    flowacc.accumulate_weighted (finite, >= 0, None: 1 everywhere; the default frac_bits is flowacc.weight_frac_bits's
    rule; one with N * rint(max(weights) * 2^frac_bits) > 2^52 is refused).  Bad arguments raise ValueError before any
    library call."""
    if not isinstance(transfer, str) or transfer not in TRANSFERS:
        raise ValueError("transfer must be one of %s, not %r" % (tuple(TRANSFERS), transfer))
    names = _outputs(outputs)
    entry, raster, raster_type, (H, W), fourth = _flow(flow)
    p = _param_f64(param, transfer, (H, W))
    n = H * W
    w = None if weights is None else _weights_f64(weights, (H, W))
    wmax = 1.0 if w is None else (float(w.max()) if n else 0.0)
    s = _args.frac_bits(n, wmax, frac_bits, " for these weights: N * rint(max(weights) * 2^frac_bits)",
                        "the default is")
    out = Routed((name, np.empty((H, W), np.float64)) for name in names)
    info = np.zeros(4, np.int64)
    check(getattr(_lib.lib(), entry)(ptr(raster, raster_type), ptr(w, c_f64p), ptr(p, c_f64p), H, W, s,
                                     TRANSFERS[transfer], *(ptr(out.get(name), c_f64p) for name in OUTPUTS),
                                     ptr(info, c_i64p)))
    out.info = dict(zip(("rounds", "queue_high", "queued", fourth), (int(v) for v in info)))
    return out


def decayed_accumulation(flow, decay, weights=None, frac_bits=None):
    """The load of route(flow, decay, 'decay'): every cell's own weight plus what reaches it when each cell passes on
    the fraction decay(c) of its load (first-order loss along the path; TauDEM's DecayAccum, the cell included)."""
    return route(flow, decay, "decay", weights, frac_bits, ("load",))["load"]


def retention_limited(flow, capacity, weights=None, frac_bits=None):
    """(outflow, retained) of route(flow, capacity, 'retain'): a cell keeps its load up to capacity(c) and passes on
    the excess -- infiltration and run-on losses with a capacity everywhere, fill and spill of depressions with
    sink_capacity's."""
    r = route(flow, capacity, "retain", weights, frac_bits, ("outflow", "retained"))
    return r["outflow"], r["retained"]


def transport_limited(flow, supply, capacity, frac_bits=None):
    """(transport, deposition) of route(flow, capacity, 'limit', weights=supply): a cell passes on its supply plus
    what arrives up to its transport capacity and deposits the rest (TauDEM's tla and tdep)."""
    r = route(flow, capacity, "limit", supply, frac_bits, ("outflow", "retained"))
    return r["outflow"], r["retained"]


def sink_capacity(dem, filled, fdr, px, frac_bits=None):
    """The volume of every depression of `dem` below its `filled` surface, placed on the depression's exit cell, as
    float64 (0 elsewhere): the capacity raster of the pluvial recipe, retention_limited(fdr, sink_capacity(...),
    rain * px * px).  Host-side numpy on watershed.drainage.

    A lake cell has filled > dem.  Its exit is the first cell on its D8 path, itself included, that is a lake cell
    whose receiver is not a lake cell (the receiver may be off the raster, nodata, or the cell may hold no code).
    capacity[e] = the exact integer sum of rint(ldexp((filled - dem) * px * px, s)) over the lake cells with exit e,
    scaled back by 2^-s; the differences and products are float64.  s = frac_bits, by default the finest scale at
    which the sum over the whole raster stays <= 2^52 (flowacc.weight_frac_bits's rule on the volumes).  A lake cell
    whose path does not reach an exit (a D8 cycle) adds nothing."""
    z = _args.raster(dem, "dem", kinds="biuf")
    zf = _args.raster(filled, "filled", z.shape, "the DEM", kinds="biuf")
    f = _args.raster(fdr, "fdr", z.shape, "the DEM", dtype=np.uint8)
    p = _args.pixel_size(px)
    H, W = z.shape
    n = H * W
    z64, f64 = np.asarray(z, np.float64), np.asarray(zf, np.float64)
    lake = f64 > z64
    vol = np.where(lake, (f64 - z64) * p * p, 0.0)
    if not np.isfinite(vol).all():
        raise ValueError("a depression depth (filled - dem) * px * px is not finite (flat index %d)"
                         % int(np.argmin(np.isfinite(vol).reshape(-1))))
    s = _args.frac_bits(n, float(vol.max()) if n else 0.0, frac_bits,
                        " for these volumes: N * rint(max((filled - dem) * px * px) * 2^frac_bits)", "the default is")
    cap = np.zeros((H, W), np.float64)
    if not lake.any():
        return cap
    yy, xx = np.mgrid[0:H, 0:W]
    to_lake = np.zeros((H, W), bool)  # the receiver exists and is a lake cell
    for k, code in enumerate(mfd.OCTANT_CODES):
        dy, dx = (0, -1, -1, -1, 0, 1, 1, 1)[k], (1, 1, 0, -1, -1, -1, 0, 1)[k]
        ny, nx = yy + dy, xx + dx
        inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        to_lake |= (f == code) & inside & lake[np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)]
    exits = lake & ~to_lake
    target = watershed.drainage(f, 1.0, None, exits.astype(np.int64)).target
    member = lake & (target >= 0)
    q = np.rint(np.ldexp(vol[member], s)).astype(np.int64)
    total = np.zeros(n, np.int64)
    np.add.at(total, target[member], q)
    return np.ldexp(total.astype(np.float64), -s).reshape(H, W)
