"""GPU (-m gpu): D-infinity flow direction and contributing area (descriptools_amd.dinf, dt_dinf_direction,
dt_dinf_accumulate and the device tier; k_dinf / k_di_* in dt_dinf.hip) against the numpy reference
(tests/_dinf_ref.py).  Direction: slope and the nodata / no-flow masks bit for bit, the angle equal or one float32
spacing away (the GPU's atan2 may differ from libm's by an ulp of float64, which flips a float32 rounding about once
in 2^27 cells: at most 10 cells per million may differ at all -- a float32 atan2 would differ on most cells).
Accumulation: bit for bit, on the reference's angles."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import golden
from descriptools_amd import dinf

import _dinf_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = 10.0


def _bits_equal(name, g, r):
    assert g.dtype == r.dtype and g.shape == r.shape, name
    gb, rb = g.view(np.int32 if g.itemsize == 4 else np.int64), r.view(np.int32 if r.itemsize == 4 else np.int64)
    if not np.array_equal(gb, rb):
        bad = np.argwhere(gb != rb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r" % (name, len(bad), i, g[i], r[i]))


def check_direction(dem, px, fdr=None):
    """GPU direction of `dem` against the reference; returns the reference's (angle, slope)"""
    got = dinf.flow_direction(dem, px, fdr)
    ra, rs = R.flow_direction(dem, px, fdr)
    assert got.angle.dtype == np.float32 and got.slope.dtype == np.float32
    _bits_equal("slope", got.slope, rs)
    for v in (-1.0, -100.0):
        assert np.array_equal(got.angle == np.float32(v), ra == np.float32(v)), "mask of angle == %g differs" % v
    diff = got.angle != ra
    n_diff = int(diff.sum())
    print("direction %s: %d of %d angles differ from the reference" % (dem.shape, n_diff, dem.size))
    assert (np.abs(got.angle[diff].astype(np.float64) - ra[diff].astype(np.float64)) <= np.spacing(ra[diff])).all()
    assert n_diff * 1_000_000 <= 10 * dem.size, "%d of %d angles differ" % (n_diff, dem.size)
    return ra, rs


def _plane(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (1000 - 3 * yy - xx).astype(np.float32)


@functools.lru_cache(maxsize=None)
def terrain(H, W, nodata_pct):
    dem = oracle.synth_dem(11, H, W, nodata_pct=nodata_pct)
    dem.setflags(write=False)
    return dem


@functools.lru_cache(maxsize=None)
def ref_angles(H, W, nodata_pct):
    """the reference's angles of a terrain (H > 0) or of the plane (nodata_pct = -1), read-only"""
    dem = _plane(H, W) if nodata_pct < 0 else terrain(H, W, nodata_pct)
    a, _ = R.flow_direction(dem, PX)
    a.setflags(write=False)
    return a


def check_accumulate(angle, weights=None, frac_bits=None):
    got = dinf.accumulate(angle, weights, frac_bits)
    ref = R.accumulate(angle, weights, frac_bits)
    assert got.dtype == np.float64
    _bits_equal("accumulation", got, ref)
    return ref


# ---- direction -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,nodata_pct", [(200, 333, 0), (200, 333, 2), (600, 1000, 0), (600, 1000, 2)])
def test_direction_terrain(H, W, nodata_pct):
    ra, rs = check_direction(terrain(H, W, nodata_pct), PX)
    assert (rs > 0).mean() > 0.9 and ((ra == -100).any() == (nodata_pct > 0))


def test_direction_plane_and_pixel_sizes():
    check_direction(_plane(300, 500), 1.0)
    check_direction(_plane(40, 50), 30.87)
    check_direction(terrain(200, 333, 2), 0.1)


def _pitted():
    """terrain with planted pits and a flat shelf"""
    dem = oracle.synth_dem(5, 150, 210, nodata_pct=1).copy()
    rng = np.random.default_rng(8)
    for _ in range(40):
        y, x = int(rng.integers(3, 147)), int(rng.integers(3, 207))
        if (dem[y - 2:y + 3, x - 2:x + 3] > -100).all():
            dem[y - 1:y + 2, x - 1:x + 2] -= 25
            dem[y, x] -= 10
    shelf = dem[60:90, 40:120]
    shelf[shelf > -100] = np.float32(np.median(shelf[shelf > -100]))
    return dem


def test_direction_fallback_on_conditioned_surface():
    dem = _pitted()
    fdr, filled = oracle.condition_d8(dem, PX)  # arrays only: the codes and the filled surface
    for surface in (dem, filled):
        a0, _ = check_direction(surface, PX)
        a1, s1 = check_direction(surface, PX, fdr)
        fell = (a0 == -1) & (a1 != -1)
        assert (s1[fell] == 0).all()
        octants = np.array([R.octant_angle(k) for k in range(8)], np.float32)
        assert np.isin(a1[fell].view(np.int32), octants.view(np.int32)).all()
        same = ~fell
        _bits_equal("cells with a facet", a1[same], a0[same])
    a0, _ = R.flow_direction(filled, PX)
    a1, _ = R.flow_direction(filled, PX, fdr)
    assert ((a0 == -1) & (a1 != -1)).sum() > 500, "the shelf and the filled pits take the D8 codes"
    # with the filled surface and its codes the graph has no cycle: everything completes
    acc = dinf.accumulate(a1)
    assert np.array_equal(acc == -100, a1 == -100)


@pytest.mark.parametrize("name", ["nonfinite", "nonfinite_f64"])
def test_direction_non_finite_heights(name):
    g = golden(name)
    dem = g["dem"].astype(np.float32)  # NaN, +inf, -inf and below-sentinel heights
    assert np.isnan(dem).any() and np.isinf(dem).any() and (dem < -100).any()
    px = float(g["px"])
    ra, rs = check_direction(dem, px)
    check_direction(dem, px, g["fdr"])
    odd = ~np.isfinite(dem) & ~(dem <= -100)
    assert (ra[odd] == -1).all() and (rs[odd] == 0).all()
    assert (ra[dem <= -100] == -100).all() and (rs[dem <= -100] == -100).all()


@pytest.mark.parametrize("shape", [(1, 37), (41, 1), (2, 2), (65, 1), (1, 1), (3, 130), (9, 129)])
def test_direction_odd_shapes(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    dem = rng.integers(0, 50, shape).astype(np.float32)
    dem[0, 0] = -100
    fdr = np.full(shape, 4, np.uint8)
    ra, rs = check_direction(dem, PX)
    check_direction(dem, PX, fdr)
    if min(shape) == 1:  # no complete facet anywhere
        assert np.isin(ra, (-1, -100)).all() and np.isin(rs, (0, -100)).all()
    flat = np.full(shape, 7, np.float32)
    flat[-1, -1] = -100
    ra, _ = check_direction(flat, PX)
    assert np.isin(ra, (-1, -100)).all()
    check_accumulate(ra)


# ---- accumulation on the reference's angles ----------------------------------------------------------------------
@pytest.mark.parametrize("H,W,nodata_pct", [(200, 333, 0), (200, 333, 2), (600, 1000, 0), (600, 1000, 2)])
def test_accumulate_terrain_unit_weights(H, W, nodata_pct):
    ref = check_accumulate(ref_angles(H, W, nodata_pct))
    assert ref.max() > 1000


def test_accumulate_float_weights():
    a = ref_angles(600, 1000, 2)
    w = np.random.default_rng(1).uniform(0, 10, a.shape)
    check_accumulate(a, w)
    check_accumulate(ref_angles(200, 333, 2), w[:200, :333].astype(np.float32))


def test_accumulate_integer_weights_frac_bits_0():
    a = ref_angles(600, 1000, 2)
    w = np.random.default_rng(2).integers(0, 1000, a.shape)
    ref = check_accumulate(a, w, 0)
    assert (ref[ref != -100] == np.rint(ref[ref != -100])).all()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from descriptools_amd import dinf
acc, _, _, info = dinf._accumulate(np.load(sys.argv[1]), None, None)
np.save(sys.argv[2], acc)
print("INFO", info["rounds"], info["queued"], info["queue_high"])
"""


def test_accumulate_plane_and_forced_spill(tmp_path):
    """every cell has two donors and two receivers; a fresh process with DT_DBG_DINF_STACK=1 runs the spill queue
    and several rounds, and gives the same bytes"""
    a = ref_angles(300, 500, -1)
    ref = check_accumulate(a)
    np.save(tmp_path / "a.npy", a)
    env = dict(os.environ, DT_DBG_DINF_STACK="1")
    out = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(tmp_path / "a.npy"), str(tmp_path / "acc.npy")],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rounds, queued, high = (int(v) for v in out.stdout.split("INFO")[1].split())
    print("forced spill: %d rounds, %d cells queued, largest round %d" % (rounds, queued, high))
    assert queued > 0 and rounds >= 2, "the spill path did not run"
    _bits_equal("forced spill", np.load(tmp_path / "acc.npy"), ref)


def test_accumulate_cone():
    """fully divergent: flow spreads from the summit"""
    yy, xx = np.mgrid[0:211, 0:190]
    dem = (5000 - 7 * np.sqrt((yy - 100.0) ** 2 + (xx - 93.0) ** 2)).astype(np.float32)
    a, _ = check_direction(dem, PX)
    kind, _, _ = R.decode(a)
    assert (kind == 2).mean() > 0.9
    ref = check_accumulate(a)
    assert (ref != -100).all()


def test_accumulate_serpentine_depth():
    """one chain of cardinal angles through every cell of 257 x 256 (65,791 moves): nothing depends on path depth"""
    H, W = 257, 256
    a = np.empty((H, W), np.float32)
    a[0::2, :] = R.octant_angle(0)
    a[1::2, :] = R.octant_angle(4)
    a[0::2, -1] = R.octant_angle(6)
    a[1::2, 0] = R.octant_angle(6)
    a[-1, -1] = -1
    order = np.arange(H * W).reshape(H, W)
    order[1::2] = order[1::2, ::-1]
    got = dinf.accumulate(a)
    _bits_equal("serpentine", got, order.astype(np.float64))
    w = np.random.default_rng(4).integers(0, 9, (H, W))
    got = dinf.accumulate(a, w, 0)
    flat = np.empty(H * W, np.int64)
    flat[order.reshape(-1)] = w.reshape(-1)
    want = np.empty(H * W, np.float64)
    want[order.reshape(-1)] = np.cumsum(flat) - flat
    _bits_equal("weighted serpentine", got, want.reshape(H, W))


def test_accumulate_d8_angles_equal_flowacc():
    from descriptools_amd import flowacc, flowdir
    dem = oracle.synth_dem(3, 600, 1001)
    fdr = flowdir.d8(dem, PX)
    got = dinf.accumulate(R.d8_angles(fdr), frac_bits=0)
    acc = flowacc.accumulate(fdr)
    assert (acc != -100).all()
    _bits_equal("D8 angles", got, acc.astype(np.float64))


# ---- cycles and bad values -----------------------------------------------------------------------------------------
def _with_cycles():
    a = ref_angles(200, 333, 2).copy()
    E, N, W_, S = (R.octant_angle(k) for k in (0, 2, 4, 6))
    for y, x in ((10, 10), (63, 63), (150, 300), (198, 127)):  # 2 x 2 cycles, two of them across tile borders
        a[y, x], a[y, x + 1], a[y + 1, x + 1], a[y + 1, x] = E, S, W_, N
        a[y, x + 1] = np.float32(3 * np.pi / 2 + 0.3)  # part of it leaves the cycle to the south-east: cells below it
    return a


def test_cycles_give_minus_100_on_and_below_them():
    a = _with_cycles()
    base = R.accumulate(ref_angles(200, 333, 2))
    ref = check_accumulate(a)
    for y, x in ((10, 10), (63, 63), (150, 300), (198, 127)):
        assert (ref[y:y + 2, x:x + 2] == -100).all()
    lost = (ref == -100) & (base != -100)
    kept = (ref != -100) & (ref == base)
    assert lost.sum() > 16 and kept.sum() > 0.5 * a.size, "cells elsewhere keep their values"
    # a ring of 150 x 90 cells across many tiles, fed from outside and from inside
    H, W = 200, 300
    ring = np.full((H, W), R.octant_angle(0), np.float32)  # everything flows east, except the ring (clockwise)
    ring[20:170, 119] = R.octant_angle(6)
    ring[169, 30:120] = R.octant_angle(4)
    ring[20:170, 30] = R.octant_angle(2)
    ring[20, 30] = R.octant_angle(0)
    ref = check_accumulate(ring)
    on_ring = np.zeros((H, W), bool)
    on_ring[20, 30:120] = on_ring[169, 30:120] = on_ring[20:170, 30] = on_ring[20:170, 119] = True
    assert np.array_equal(ref == -100, on_ring), "the ring sends nothing out of itself: every other cell completes"
    assert ref[50, 29] == 29 and ref[50, 118] == 87 and ref[50, 299] == 179


def test_bad_angle_on_the_device_tier():
    from descriptools_amd import _lib, device
    H, W = 70, 90
    a = ref_angles(200, 333, 2)[:H, :W].copy()
    ctx = device.Context()
    L = _lib.lib()
    out = ctx.empty((H, W), np.float64)
    try:
        for bad in (np.nan, -3.0, 7.0):
            b = a.copy()
            b[33, 44] = bad
            d = ctx.to_device(b)
            _lib.check(L.dt_dev_dinf_accumulate(ctx.h, d.ptr, None, H, W, 10, 64, out.ptr))
            assert ctx.status() & 16, "DT_STATUS_BAD_ANGLE"
            got = out.to_host()
            d.free()
            b[33, 44] = -1  # counted as no flow
            _bits_equal("bad angle as -1", got, R.accumulate(b, None, 10))
        d = ctx.to_device(a)
        _lib.check(L.dt_dev_dinf_accumulate(ctx.h, d.ptr, None, H, W, 10, 64, out.ptr))
        assert ctx.status() == 0
        d.free()
        assert L.dt_dev_dinf_accumulate(ctx.h, None, None, 0, 0, 0, 1, None) == 0
        assert L.dt_dev_dinf_accumulate(ctx.h, out.ptr, None, H, W, 10, 0, out.ptr) != 0      # rounds 0
        assert L.dt_dev_dinf_direction(ctx.h, out.ptr, None, H, W, 0.0, out.ptr, None) != 0   # px
    finally:
        out.free()
        ctx.close()


# ---- end to end and the device tier ------------------------------------------------------------------------------
def test_end_to_end_and_repeated_runs():
    dem = terrain(600, 1000, 2)
    runs = [dinf.flow_direction(dem, PX) for _ in range(2)]
    _bits_equal("angle, repeated", runs[1].angle, runs[0].angle)
    _bits_equal("slope, repeated", runs[1].slope, runs[0].slope)
    accs = [dinf.accumulate(runs[0].angle) for _ in range(3)]
    for a in accs[1:]:
        _bits_equal("accumulation, repeated", a, accs[0])
    _bits_equal("the GPU's own angles", accs[0], R.accumulate(runs[0].angle))
    sca = dinf.specific_catchment_area(runs[0].angle, PX)
    _bits_equal("sca", sca, np.where(accs[0] == -100, -100.0, (accs[0] + 1.0) * PX))
    # with weights the cell's own quantised weight takes the place of the 1
    w = np.random.default_rng(6).uniform(0, 3, dem.shape)
    s = R.default_frac_bits(dem.size, float(w.max()))
    accw = R.accumulate(runs[0].angle, w, s)
    own = np.ldexp(np.rint(np.ldexp(w, s)), -s)
    _bits_equal("weighted sca", dinf.specific_catchment_area(runs[0].angle, PX, w),
                np.where(accw == -100, -100.0, (accw + own) * PX))


def test_device_tier_on_a_chain():
    """dt_dev_dinf_direction on a conditioning Chain's filled surface and codes, dt_dev_dinf_accumulate on its angles:
    equal to the host tier"""
    from descriptools_amd import _lib, chain, device
    H, W = 320, 448
    dem = _pitted_large(H, W)
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=PX, overlap=False, tune_placement=False, river_threshold=200, condition=True,
                     condition_rounds=500)
    d = ctx.to_device(dem)
    ang, slp, acc = ctx.empty((H, W), np.float32), ctx.empty((H, W), np.float32), ctx.empty((H, W), np.float64)
    L = _lib.lib()
    try:
        ch.run(d.ptr)
        _lib.check(L.dt_dev_dinf_direction(ctx.h, ch.p("filled"), ch.p("fdr"), H, W, PX, ang.ptr, slp.ptr))
        _lib.check(L.dt_dev_dinf_accumulate(ctx.h, ang.ptr, None, H, W, 20, 256, acc.ptr))
        assert ctx.status() == 0
        info = np.zeros(4, np.int64)
        _lib.check(L.dt_dev_dinf_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
        g_ang, g_slp, g_acc = ang.to_host(), slp.to_host(), acc.to_host()
        assert info[3] == (R.decode(g_ang)[0] == 2).sum() and info[2] >= info[1] >= 0 and info[0] < 256
        _lib.check(L.dt_dev_dinf_direction(ctx.h, ch.p("filled"), ch.p("fdr"), H, W, PX, ang.ptr, None))  # slope NULL
        ctx.sync()
        _bits_equal("slope NULL", ang.to_host(), g_ang)
        filled, fdr = ch.buf["filled"].to_host(), ch.buf["fdr"].to_host()
    finally:
        for b in (d, ang, slp, acc):
            b.free()
        ch.free()
        ctx.close()
    host = dinf.flow_direction(filled, PX, fdr)
    _bits_equal("angle", g_ang, host.angle)
    _bits_equal("slope", g_slp, host.slope)
    _bits_equal("accumulation", g_acc, dinf.accumulate(host.angle, frac_bits=20))
    assert np.array_equal(g_acc == -100, g_ang == -100), "conditioned: no cycle"


def _pitted_large(H, W):
    dem = oracle.synth_dem(9, H, W, nodata_pct=1).copy()
    dem[100:140, 200:260][dem[100:140, 200:260] > -100] -= 30
    return np.ascontiguousarray(dem, np.float32)


def test_device_tier_budget_of_rounds():
    """rounds = 1 with a lane capped at one cell (no stack) leaves queued work on the plane: DT_STATUS_NOT_CONVERGED; calls
    with a negative budget continue and finish it"""
    from descriptools_amd import _lib, device
    H, W = 300, 500
    a = ref_angles(H, W, -1)
    ref = R.accumulate(a, None, 30)
    ctx = device.Context()
    L = _lib.lib()
    d = ctx.to_device(a)
    out = ctx.empty((H, W), np.float64)
    DT_DBG_DINF_STACK = 11
    try:
        _lib.check(L.dt_debug_set(DT_DBG_DINF_STACK, 1))
        _lib.check(L.dt_dev_dinf_accumulate(ctx.h, d.ptr, None, H, W, 30, 1, out.ptr))
        assert ctx.status() & 2, "DT_STATUS_NOT_CONVERGED"
        part = out.to_host()
        assert (part == -100).any() and ((part == ref) | (part == -100)).all()
        calls = 0
        while True:
            _lib.check(L.dt_dev_dinf_accumulate(ctx.h, d.ptr, None, H, W, 30, -32, out.ptr))
            calls += 1
            if not ctx.status() & 2:
                break
            assert calls < 2000
        print("finished after %d further calls of 32 rounds" % calls)
        # a continuation names what it was started with
        assert L.dt_dev_dinf_accumulate(ctx.h, d.ptr, None, H, W, 29, -1, out.ptr) != 0
        assert L.dt_dev_dinf_accumulate(ctx.h, out.ptr, None, H, W, 30, -1, out.ptr) != 0
        assert L.dt_dev_dinf_accumulate(ctx.h, d.ptr, out.ptr, H, W, 30, -1, out.ptr) != 0
        assert L.dt_dev_dinf_accumulate(ctx.h, d.ptr, None, W, H, 30, -1, out.ptr) != 0
        _bits_equal("continued", out.to_host(), ref)
        # another call on the context takes the scratch: nothing to continue
        other = ctx.to_device(np.ones((H, W), np.uint8))
        up = ctx.empty((H, W), np.float64)
        _lib.check(L.dt_dev_upslope_length(ctx.h, other.ptr, None, H, W, PX, up.ptr))
        assert L.dt_dev_dinf_accumulate(ctx.h, d.ptr, None, H, W, 30, -1, out.ptr) != 0
        other.free()
        up.free()
    finally:
        L.dt_debug_set(DT_DBG_DINF_STACK, 0)
        d.free()
        out.free()
        ctx.close()
