"""The numpy reference of descriptools_amd.inundation (its module docstring holds the scheme): the six steps in exactly
that association, vectorised, float64 throughout.  Every expression is parenthesised the way the kernel evaluates it, so
that the device result can be held to these bits.  No library is touched."""
import math

import numpy as np

G = 9.80665


def cbrt3(x):
    """the cube root of x > 0 by the stated sequence: x = m * 2^(3k) with m in [0.5, 4) exactly, the seed
    (0.6 + 0.35 m) - 0.03 (m m), four steps y = (2 y + m / (y y)) / 3, the result y * 2^k exactly"""
    x = np.asarray(x, np.float64)
    f, e = np.frexp(x)
    k = np.floor_divide(e, 3)
    m = np.ldexp(f, e - 3 * k)
    y = (0.6 + 0.35 * m) - 0.03 * (m * m)
    for _ in range(4):
        y = ((2.0 * y) + m / (y * y)) / 3.0
    return np.ldexp(y, k)


def discharge(times, q, t):
    """Q(t) of every inflow cell: linear between the table's times, its end values outside"""
    T = len(times)
    i = int(np.searchsorted(times, t, side="right"))
    if i == 0:
        return q[:, 0].copy()
    if i == T:
        return q[:, T - 1].copy()
    ta, tb = times[i - 1], times[i]
    return q[:, i - 1] + (q[:, i] - q[:, i - 1]) * ((t - ta) / (tb - ta))


def _face(q, za, zb, ha, hb, na, nb, ok, dt, px, dry):
    """the candidate flux on faces between cells a (west / north) and b; ok: both valid"""
    ea, eb = za + ha, zb + hb
    hf = np.maximum(ea, eb) - np.maximum(za, zb)
    wet = ok & (hf > dry)
    hs = np.where(wet, hf, 1.0)
    num = q - ((G * hs) * dt) * ((eb - ea) / px)
    nf = 0.5 * (na + nb)
    den = 1.0 + (((G * dt) * (nf * nf)) * np.abs(q)) / ((hs * hs) * cbrt3(hs))
    return np.where(wet, num / den, 0.0)


def simulate(z, valid, px, t_end, manning=0.05, depth=None, rain=0.0, inflow=None, boundary="closed",
             boundary_slope=1e-3, alpha=0.7, dt_max=60.0, dry=1e-3, arrival_depth=0.05, state=None, max_steps=None,
             track=False):
    """-> dict(depth, qx, qy, max_depth, arrival, t, steps, dt_min, dt_last, hmax, limited_steps, finished[, volumes]);
    z: heights (float64; anything on invalid cells), valid: bool; manning, rain: scalars or float64 rasters; inflow:
    (cells, times, discharge[K, T]); state: a dict of an earlier result to go on from; track: keep the volume after
    every step.  Invalid cells hold 0 in depth and max_depth, NaN in arrival."""
    valid = np.asarray(valid, bool)
    H, W = valid.shape
    z = np.where(valid, np.asarray(z, np.float64), 0.0)
    n = np.broadcast_to(np.asarray(manning, np.float64), (H, W))
    n = np.where(valid, n, 1.0)
    rn = np.where(valid, np.broadcast_to(np.asarray(rain, np.float64), (H, W)), 0.0)
    if state is not None:
        h = np.where(valid, state["depth"], 0.0)
        qx, qy = state["qx"].copy(), state["qy"].copy()
        t, steps = float(state["t"]), int(state["steps"])
    else:
        h = np.zeros((H, W)) if depth is None else np.where(valid, np.asarray(depth, np.float64), 0.0)
        qx, qy = np.zeros((H, W)), np.zeros((H, W))
        t, steps = 0.0, 0
    if state is not None and state.get("max_depth") is not None:
        md = np.where(valid, state["max_depth"], 0.0)
    else:
        md = h.copy()
    if state is not None and state.get("arrival") is not None:
        arr = state["arrival"].copy()
    else:
        arr = np.where(valid & (h > arrival_depth), t, np.nan)
    okx = valid[:, :-1] & valid[:, 1:]
    oky = valid[:-1, :] & valid[1:, :]
    sides = np.zeros((H, W))
    if boundary == "open" and H and W:
        sides[0, :] += 1.0
        sides[-1, :] += 1.0
        sides[:, 0] += 1.0
        sides[:, -1] += 1.0
    sqrt_s = math.sqrt(boundary_slope)
    if inflow is not None:
        cells, times, qtab = (np.asarray(inflow[0], np.int64), np.asarray(inflow[1], np.float64),
                              np.asarray(inflow[2], np.float64).reshape(len(inflow[0]), -1))
    k, dt_min, dt_last, limited, vols = 0, math.inf, 0.0, 0, []
    hmax = float(h.max()) if h.size else 0.0
    while t < t_end and (max_steps is None or k < max_steps):
        dt = dt_max if hmax <= 0 else min(dt_max, (alpha * px) / math.sqrt(G * hmax))
        rem = t_end - t
        last = dt >= rem
        if last:
            dt = rem
        t_new = t_end if last else t + dt
        sx = np.zeros((H, W))
        sy = np.zeros((H, W))
        sx[:, :-1] = _face(qx[:, :-1], z[:, :-1], z[:, 1:], h[:, :-1], h[:, 1:], n[:, :-1], n[:, 1:], okx, dt, px, dry)
        sy[:-1, :] = _face(qy[:-1, :], z[:-1, :], z[1:, :], h[:-1, :], h[1:, :], n[:-1, :], n[1:, :], oky, dt, px, dry)
        eo = np.zeros((H, W))
        ob = valid & (h > dry) & (sides > 0)
        if ob.any():
            hb = h[ob]
            c = cbrt3(hb)
            eo[ob] = sides[ob] * ((((hb * c) * c) * sqrt_s) / n[ob])
        sN = np.zeros((H, W))
        sN[1:, :] = sy[:-1, :]
        sW = np.zeros((H, W))
        sW[:, 1:] = sx[:, :-1]
        out = (((np.maximum(-sN, 0.0) + np.maximum(-sW, 0.0)) + np.maximum(sx, 0.0)) + np.maximum(sy, 0.0)) + eo
        lim = (dt * out) > (h * px)
        r = np.where(lim, (h * px) / np.where(lim, dt * out, 1.0), 1.0)
        limited += bool((lim & valid).any())
        rE = np.ones((H, W))
        rE[:, :-1] = r[:, 1:]
        rS = np.ones((H, W))
        rS[:-1, :] = r[1:, :]
        qx = sx * np.where(sx > 0, r, rE)
        qy = sy * np.where(sy > 0, r, rS)
        qN = np.zeros((H, W))
        qN[1:, :] = qy[:-1, :]
        qW = np.zeros((H, W))
        qW[:, 1:] = qx[:, :-1]
        h = np.where(valid, np.maximum(0.0, h + dt * (((((qN - qy) + (qW - qx)) - eo * r) / px) + rn)), 0.0)
        if inflow is not None:
            Q = discharge(times, qtab, t)
            h.reshape(-1)[cells] += (Q * dt) / (px * px)
        md = np.maximum(md, h)
        arr = np.where(np.isnan(arr) & valid & (h > arrival_depth), t_new, arr)
        t = t_new
        steps += 1
        k += 1
        dt_min, dt_last = min(dt_min, dt), dt
        hmax = float(h.max())
        if track:
            vols.append(math.fsum((h * (px * px)).reshape(-1).tolist()))
    res = {"depth": h, "qx": qx, "qy": qy, "max_depth": md, "arrival": arr, "t": t, "steps": steps,
           "dt_min": dt_min if k else 0.0, "dt_last": dt_last, "hmax": hmax, "limited_steps": limited,
           "finished": t >= t_end}
    if track:
        res["volumes"] = vols
    return res


# ---- the cases the host and the device tests share --------------------------------------------------------------------
def lake(level, islands):
    """heights that are multiples of 1/64 with a nodata wall, a lake at `level` -> (dem float32, valid, depth)"""
    rng = np.random.default_rng(3)
    H, W = 37, 70
    top = 3.5 if islands else 1.9
    dem = (rng.integers(0, int(top * 64), (H, W)) / 64.0).astype(np.float32)
    dem[5:30, 40] = -100.0  # the wall
    dem[20, 10:20] = -100.0
    valid = dem > -100
    depth = np.where(valid, np.maximum(level - dem.astype(np.float64), 0.0), 0.0)
    return dem, valid, depth


def rough_terrain():
    """rough tilted 70 x 131 terrain with a few nodata cells -> (dem float32, valid)"""
    rng = np.random.default_rng(7)
    H, W = 70, 131
    y, x = np.mgrid[0:H, 0:W]
    dem = (0.02 * x + 0.01 * y + 0.3 * rng.random((H, W))).astype(np.float32)
    dem[30:34, 60:66] = -100.0
    return dem, dem > -100


def dam_break():
    """a 3 m column of water behind a dam at the top of a 10 % slope, 40 x 90 -> (dem float32, valid, depth)"""
    H, W = 40, 90
    dem = np.broadcast_to((0.1 * 10.0 * (W - 1 - np.arange(W))).astype(np.float32), (H, W)).copy()
    depth = np.zeros((H, W))
    depth[:, :12] = 3.0
    return dem, np.ones((H, W), bool), depth


def hunter(px=25.0, cells=200, n=0.03, u=1.0, t_end=3600.0):
    """Hunter et al. (2005): the inflow table whose wave over a flat bed has a closed form -> (inflow, analytic h)"""
    times = np.arange(0.0, t_end + 1.0, 10.0)
    h0 = (7.0 / 3.0 * n * n * u ** 3 * times) ** (3.0 / 7.0)
    inflow = (np.array([0], np.int64), times, (u * h0 * px)[None, :])
    x = (np.arange(cells) + 0.5) * px
    ana = np.where(x < u * t_end, (7.0 / 3.0 * n * n * u * u * np.maximum(u * t_end - x, 0.0)) ** (3.0 / 7.0), 0.0)
    return inflow, ana
