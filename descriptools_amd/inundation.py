"""Local-inertial 2-D flood inundation (net-new): the simplified shallow-water scheme of Bates, Horritt & Fewtrell
(2010), the one behind LISFLOOD-FP -- the dynamic primitive beside the static descriptors.  It turns a rain depth, an
inflow hydrograph or a HAND stage map into routed water, so that the package can make the benchmark flood map its
descriptors are calibrated against, and let water pond behind what flowdir.d8_carved cuts through.

Inputs.  `dem`: a 2-D real raster, taken as float32 and widened to float64; a cell is valid iff _lib.nodata_mask == 0
and its height is finite, every other cell is a wall.  `manning`: a scalar (float64), or a raster taken as float32,
finite and > 0 on valid cells.  `depth`: the water depth the run starts from, float64, finite and >= 0 on valid cells
(None: dry).  `rain`: a scalar or a raster taken as float32, m/s, finite and >= 0, constant over the call.  `inflow`:
(cells int64[K] flat indices of valid cells without duplicates, K <= 4096; times float64[T] ascending strictly;
discharge float64[K, T] in m^3/s, finite and >= 0): linear in time, the end values outside the table, evaluated at the
start of each step.  `boundary`: "closed" (the raster's edge is a wall) or "open" (water leaves over every side of a
valid cell that faces the raster's edge, at normal depth for `boundary_slope`); nodata is a wall in both.

State.  h[H, W] the depth; qx[i, j] the unit-width discharge (m^2/s) over the face between (i, j) and (i, j + 1),
positive eastwards; qy[i, j] over the face to (i + 1, j), positive southwards; float64.  Faces to a wall and faces beyond
the raster hold 0.  g = 9.80665.

A step, in this association (the contract: csrc/dt_inundation.hip and the numpy restatement the tests keep evaluate
exactly these expressions, float64, one rounding per operation, no fused multiply-add):
 1. hmax = the largest h (exact, whatever the order).  dt = dt_max if hmax <= 0 else min(dt_max, (alpha * px) /
    sqrt(g * hmax)); rem = t_end - t; the step is the last when dt >= rem, and then dt = rem.
 2. On a face between valid cells a (west / north) and b: ea = za + ha, eb = zb + hb, hf = max(ea, eb) - max(za, zb).
    If hf > dry: num = q - ((g * hf) * dt) * ((eb - ea) / px); nf = 0.5 * (na + nb);
    den = 1 + (((g * dt) * (nf * nf)) * |q|) / ((hf * hf) * cbrt3(hf)); q* = num / den.  Otherwise q* = 0.
 3. Open boundary: a valid cell with h > dry and s > 0 sides on the raster's edge loses eo = s * ((((h * c) * c) *
    sqrt(boundary_slope)) / n) with c = cbrt3(h); otherwise eo = 0.
 4. Limiter: out = (((max(-q*N, 0) + max(-q*W, 0)) + max(q*E, 0)) + max(q*S, 0)) + eo; r = (h * px) / (dt * out) if
    dt * out > h * px, else 1.  It keeps depths non-negative and the volume conserved.
 5. Every q* is multiplied by the r of the cell it leaves (the west / north cell when q* > 0, the east / south cell
    otherwise): the new qx, qy.
 6. h' = max(0, h + dt * (((((qN - qS) + (qW - qE)) - eo * r) / px) + rain)); then each inflow cell gains
    (Q(t) * dt) / (px * px); then max_depth = max(max_depth, h') and arrival = the new time where it is still NaN and
    h' > arrival_depth; then t = t_end on the last step, t + dt otherwise.  The hmax of the next step sees the inflow.
cbrt3(x), x > 0: x = m * 2^(3k) exactly with m in [0.5, 4) (frexp, ldexp); y = (0.6 + 0.35 * m) - 0.03 * (m * m); four
times y = ((2 * y) + m / (y * y)) / 3; the result is y * 2^k exactly.  The seed is within 8.2 % and a step squares the
relative error (6.6e-3, 4.3e-5, 1.9e-9, 3.5e-18), so four steps end within 1 ulp of the cube root and a fifth would
change nothing but the cost (two divisions).  Not the device library's cbrt or pow, which do not round like libm.

What a call holds.  The state, max_depth, arrival, t and the step count are the numpy restatement's bit for bit, on
every run, in both tiers and whatever `sync_every` is.  h >= 0.  A lake at rest stays at rest exactly (heights whose
sums with the depth are exact: every flux is exactly 0).  The volume changes by rain, inflow and the open boundary's
loss only, to rounding (about 5 * steps * 2^-53 relative).

Refused with ValueError before any library call: rasters that are not 2-D, shapes that differ, 2^31 cells or more, a px,
t_end, alpha, dt_max or boundary_slope that is not finite and > 0, alpha > 1, a negative dry or arrival_depth, a
boundary other than "closed" / "open", unknown outputs, a bad inflow table, manning, rain or depth values outside their
ranges on valid cells, a sync_every outside 1..1024, a negative max_steps, a state of another shape.

Recipes.
    res = inundation.simulate(dem, px, 6 * 3600, rain=50e-3 / 3600, outputs=("depth", "max_depth"))
    evaluation.calibration(hand, res.max_depth > 0.1, under=True)         # a benchmark map from a model of our own
    res = inundation.simulate(dem, px, 3600, depth=reaches.inundate(...))  # a HAND stage map routed onward
    more = inundation.simulate(dem, px, 7200, rain=0.0, state=res.state)   # the same run, on with another rain"""
import math

import numpy as np

from . import _args, _lib
from ._lib import c_f32p, c_f64p, c_i64p, check, ptr

G = 9.80665
INFO_WORDS = 8  # DT_INUNDATION_INFO_WORDS
INFLOW_MAX = 4096  # DT_INUNDATION_INFLOW_MAX
OUTPUTS = ("depth", "max_depth", "arrival")
BOUNDARIES = ("closed", "open")


class Inundation(tuple):
    """the requested outputs in their order, with `.depth`, `.max_depth`, `.arrival` (None when not asked for),
    `.state` ({"depth", "qx", "qy", "t", "steps"} and, when asked for, "max_depth", "arrival": what state= takes) and
    `.info`: {"t", "steps": in all, "finished": t >= t_end, "dt_min", "dt_last", "hmax", "volume": math.fsum(depth *
    px^2) over valid cells, "limited_steps": the steps of this call in which the limiter acted}"""

    def __new__(cls, names, fields, state=None, info=None):
        self = tuple.__new__(cls, tuple(fields[n] for n in names))
        self._fields_by_name = {n: fields[n] for n in names}
        self.state = state
        self.info = info
        return self

    depth = property(lambda self: self._fields_by_name.get("depth"))
    max_depth = property(lambda self: self._fields_by_name.get("max_depth"))
    arrival = property(lambda self: self._fields_by_name.get("arrival"))


def _number(v, what, positive=False):
    """v as a float; ValueError unless it is a number (not a bool), finite and >= 0 (positive: > 0)"""
    try:
        p = math.nan if isinstance(v, (bool, np.bool_)) else float(v)
    except (TypeError, ValueError):
        p = math.nan
    if not (math.isfinite(p) and (p > 0 if positive else p >= 0)):
        raise ValueError("%s must be a finite number %s 0, not %r" % (what, ">" if positive else ">=", v))
    return p


def _field(v, what, shape, valid, positive):
    """a scalar -> (None, float); a raster -> (float32 array, 0.0); its values on valid cells finite and >= 0 (> 0)"""
    if np.ndim(v) == 0:
        return None, _number(v, what, positive)
    r = _args.raster(v, what, shape=shape, other="dem", kinds="biuf")
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.ascontiguousarray(r, np.float32)
    on = r[valid]
    if not (np.isfinite(on).all() and ((on > 0).all() if positive else (on >= 0).all())):
        raise ValueError("%s must be finite and %s 0 on valid cells" % (what, ">" if positive else ">="))
    return r, 0.0


def _depth(v, what, shape, valid):
    """a depth raster as float64: finite and >= 0 on valid cells, +0 on walls"""
    r = _args.raster(v, what, shape=shape, other="dem", kinds="biuf")
    r = np.asarray(r, np.float64)
    on = r[valid]
    if not (np.isfinite(on).all() and (on >= 0).all()):
        raise ValueError("%s must be finite and >= 0 on valid cells" % what)
    return np.ascontiguousarray(np.where(valid, r + 0.0, 0.0))


def _flux(v, what, shape):
    r = _args.raster(v, what, shape=shape, other="dem", kinds="f")
    if not np.isfinite(r).all():
        raise ValueError("%s must be finite" % what)
    return np.array(r, np.float64, order="C")


def _inflow(inflow, valid):
    """(cells int64[K], times float64[T], discharge float64[K, T]) checked, or (None, None, None)"""
    if inflow is None:
        return None, None, None
    try:
        cells, times, q = inflow
    except (TypeError, ValueError):
        raise ValueError("inflow must be the triple (cells, times, discharge)")
    cells, times, q = np.asarray(cells), np.asarray(times), np.asarray(q)
    if cells.ndim != 1 or cells.dtype.kind not in "iu":
        raise ValueError("inflow cells must be a 1-D integer array")
    if cells.size > INFLOW_MAX:
        raise ValueError("inflow has %d cells, at most %d can be taken" % (cells.size, INFLOW_MAX))
    if times.ndim != 1 or times.dtype.kind not in "iuf" or q.dtype.kind not in "iuf":
        raise ValueError("inflow times must be a 1-D real array and the discharge real")
    if q.shape != (cells.size, times.size):
        raise ValueError("inflow discharge has shape %s, not (cells, times) = %s" % (q.shape, (cells.size, times.size)))
    if cells.size == 0:
        return None, None, None
    if times.size == 0 or times.size > 1 << 20:
        raise ValueError("inflow times must number 1 to 2^20")
    cells = np.ascontiguousarray(cells, np.int64)
    times = np.ascontiguousarray(times, np.float64)
    q = np.ascontiguousarray(q, np.float64)
    if not (np.isfinite(times).all() and (np.diff(times) > 0).all()):
        raise ValueError("inflow times must be finite and strictly ascending")
    if not (np.isfinite(q).all() and (q >= 0).all()):
        raise ValueError("inflow discharge must be finite and >= 0")
    if cells.min() < 0 or cells.max() >= valid.size or np.unique(cells).size != cells.size:
        raise ValueError("inflow cells must be flat indices into the raster without duplicates")
    if not valid.reshape(-1)[cells].all():
        raise ValueError("inflow cells must be valid cells of the dem")
    return cells, times, q


def simulate(dem, px, t_end, manning=0.05, depth=None, rain=None, inflow=None, boundary="closed", boundary_slope=1e-3,
             alpha=0.7, dt_max=60.0, dry=1e-3, outputs=("depth",), arrival_depth=0.05, state=None, max_steps=None,
             sync_every=64):
    """Route water over `dem` (pixel size px, m) until t_end (s) -> Inundation: the requested `outputs` ("depth",
    "max_depth", "arrival": float64; -100 on invalid cells in the depths, NaN in arrival and where the water never got
    deeper than arrival_depth) with `.state` and `.info`.  The module docstring holds the scheme.  `state`: the
    `.state` of an earlier call to go on from (its time and fluxes; `depth` is then not taken); `max_steps`: end the
    call after that many steps (info["finished"] says whether t_end was reached); `sync_every` (1..1024): how many
    guarded steps are enqueued between two read-backs of the control block -- the result does not depend on it."""
    d = _args.raster(dem, "dem", kinds="iuf")
    p = _args.pixel_size(px)
    te = _args.positive(t_end, "t_end")
    al = _args.positive(alpha, "alpha")
    if al > 1:
        raise ValueError("alpha must be <= 1, not %r" % (alpha,))
    dm = _args.positive(dt_max, "dt_max")
    bs = _args.positive(boundary_slope, "boundary_slope")
    dr = _number(dry, "dry")
    ad = _number(arrival_depth, "arrival_depth")
    if not isinstance(boundary, str) or boundary not in BOUNDARIES:
        raise ValueError("boundary must be one of %s, not %r" % (BOUNDARIES, boundary))
    if isinstance(outputs, str):
        outputs = (outputs,)
    names = tuple(outputs)
    if not names or any(not isinstance(n, str) or n not in OUTPUTS for n in names) or len(set(names)) != len(names):
        raise ValueError("outputs must be distinct names out of %s, not %r" % (OUTPUTS, outputs))
    ms = -1 if max_steps is None else _args.integer(max_steps, "max_steps", 0)
    se = _args.integer(sync_every, "sync_every", 1, 1024)
    H, W = d.shape
    with np.errstate(over="ignore", invalid="ignore"):
        z = np.ascontiguousarray(d, np.float32)
    valid = (_lib.nodata_mask(d, d.shape) == 0) & np.isfinite(z)
    z = np.where(valid, z, np.float32(np.nan))
    nr, ns = _field(manning, "manning", d.shape, valid, True)
    rr, rs = _field(0.0 if rain is None else rain, "rain", d.shape, valid, False)
    cells, times, q = _inflow(inflow, valid)
    want_md, want_ar = "max_depth" in names, "arrival" in names
    md = ar = None
    if state is not None:
        try:
            h = _depth(state["depth"], "state depth", d.shape, valid)
            qx, qy = _flux(state["qx"], "state qx", d.shape), _flux(state["qy"], "state qy", d.shape)
            t0, steps0 = _number(state["t"], "state t"), _args.integer(state["steps"], "state steps", 0)
            if want_md and state.get("max_depth") is not None:
                md = _depth(state["max_depth"], "state max_depth", d.shape, valid)
            if want_ar and state.get("arrival") is not None:
                ar = np.array(_args.raster(state["arrival"], "state arrival", shape=d.shape, other="dem", kinds="f"),
                              np.float64, order="C")
        except (KeyError, TypeError, AttributeError):
            raise ValueError("state must be the .state of an earlier call")
    else:
        h = np.zeros(d.shape) if depth is None else _depth(depth, "depth", d.shape, valid)
        qx, qy, t0, steps0 = np.zeros(d.shape), np.zeros(d.shape), 0.0, 0
    if want_md and md is None:
        md = h.copy()
    if want_ar and ar is None:
        ar = np.where(valid & (h > ad), t0, np.nan)
    par = np.array([p, t0, te, ns, rs, al, dm, dr, bs, ad], np.float64)
    info = np.zeros(INFO_WORDS, np.int64)
    check(_lib.lib().dt_inundation(ptr(z, c_f32p), ptr(nr, c_f32p), ptr(rr, c_f32p), H, W, ptr(par, c_f64p),
                                   BOUNDARIES.index(boundary), ptr(cells, c_i64p), ptr(times, c_f64p), ptr(q, c_f64p),
                                   0 if cells is None else cells.size, 0 if cells is None else times.size, steps0, ms,
                                   se, ptr(h, c_f64p), ptr(qx, c_f64p), ptr(qy, c_f64p), ptr(md, c_f64p),
                                   ptr(ar, c_f64p), ptr(info, c_i64p)))
    f = info[2:6].view(np.float64)
    if d.size:
        t, steps, finished = float(f[0]), int(info[0]), bool(info[7])
    else:  # no cell to step: the call is at its end
        t, steps, finished = max(t0, te), steps0, True
    st = {"depth": h, "qx": qx, "qy": qy, "t": t, "steps": steps}
    fields = {"depth": np.where(valid, h, -100.0)}
    if want_md:
        st["max_depth"] = md
        fields["max_depth"] = np.where(valid, md, -100.0)
    if want_ar:
        st["arrival"] = ar
        fields["arrival"] = ar
    out = {"t": t, "steps": steps, "finished": finished, "dt_min": float(f[1]), "dt_last": float(f[2]),
           "hmax": float(f[3]), "volume": math.fsum((h[valid] * (p * p)).tolist()), "limited_steps": int(info[6])}
    return Inundation(names, fields, st, out)
