"""GPU (-m gpu): the line-of-sight attributes (descriptools_amd.horizon, dt_horizon, dt_dev_horizon; k_horizon in
dt_horizon.hip) against the numpy reference (tests/_horizon_ref.py).  landform, pattern and sky_view: bit for bit,
dtypes and contiguity included.  positive and negative hold eight atan each, and the GPU's and numpy's need not round
alike: the same -100 cells, every other cell within one float32 spacing, and at most 16 cells of a raster that differ
at all -- the rule and the reasoning of tests/test_gpu_terrain.py for aspect: a few-ulp float64 error moves a float32
rounding in far fewer than 10^-3 of the cells of these rasters, so the cap is a condition, not a measurement.

Duality and ties.  Turning a surface upside down negates every tangent exactly (the heights of that test are multiples
of 1/256 below 64), so tmax and tmin change places and signs.  The digit rule then swaps +1 and -1 -- except at a tie
|tmax| == |tmin| > T, which rule 2 sends to -1 on both surfaces (a direction with a single sample is one;
tests/test_horizon_host.py).  test_duality holds every cell and direction to exactly that: swapped wherever the
reference's extremes do not tie, -1 on both sides where they do, and the dual landform on every cell without a tie."""
import functools
import importlib
import json
import math
import os

import numpy as np
import pytest

import oracle
from conftest import golden
from descriptools_amd import horizon

import _horizon_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = horizon.OUTPUTS
EXACT = ("landform", "pattern", "sky_view")
DTYPES = {"landform": np.uint8, "pattern": np.uint16, "positive": np.float32, "negative": np.float32,
          "sky_view": np.float32}
NONE = {"landform": 0, "pattern": 65535, "positive": -100, "negative": -100, "sky_view": -100}
T1 = R.flat_tangent(1.0)


def _bits_equal(name, g, r):
    assert g.dtype == r.dtype and g.shape == r.shape, name
    gi, ri = (a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) for a in (g, r))
    if not np.array_equal(gi, ri):
        bad = np.argwhere(gi != ri)
        i = tuple(bad[0])
        raise AssertionError("%s: %d values differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i], r[i]))


def _openness_close(name, g, r):
    assert g.dtype == r.dtype == np.float32 and g.shape == r.shape, name
    assert np.array_equal(g == -100, r == -100), name + ": cells without a value differ"
    live = r != -100
    g64, r64 = g[live].astype(np.float64), r[live].astype(np.float64)
    assert ((g64 > 0) & (g64 < math.pi)).all(), name
    tol = np.spacing(np.maximum(g[live], r[live])).astype(np.float64)
    cells = int((g64 != r64).sum())
    print("%s: %d of %d values differ from the reference" % (name, cells, live.sum()))
    d = np.abs(g64 - r64)
    assert (d <= tol).all(), "%s: a value is off by %r" % (name, float((d - tol).max()))
    assert cells <= 16, name


def check(name, got, ref, outputs=ALL):
    assert tuple(got) == tuple(outputs), name
    for k in outputs:
        assert got[k].dtype == DTYPES[k] and got[k].flags.c_contiguous, (name, k)
        (_bits_equal if k in EXACT else _openness_close)("%s, %s" % (name, k), got[k], ref[k])


@functools.lru_cache(maxsize=None)
def synth(H, W, nodata_pct):
    dem = oracle.synth_dem(11, H, W, nodata_pct=nodata_pct)
    dem.setflags(write=False)
    return dem


@functools.lru_cache(maxsize=None)
def synth_ref(H, W, nodata_pct, px, radius, skip=0, flat=1.0):
    """the reference's five outputs on a synthetic terrain, computed once and read-only"""
    ref = R.attributes(synth(H, W, nodata_pct), px, R.flat_tangent(flat), ALL, radius, skip)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _valued(ref):
    return float((ref["landform"] != 0).mean())


CASES = [(H, W, nod, r) for (H, W, nod) in ((200, 333, 0), (200, 333, 2), (600, 1000, 2)) for r in (1, 3)]


@pytest.mark.parametrize("H,W,nodata_pct,radius", CASES)
def test_against_the_reference_on_terrain(H, W, nodata_pct, radius):
    dem = synth(H, W, nodata_pct)
    for px in (10.0, 7.3):
        ref = synth_ref(H, W, nodata_pct, px, radius)
        print("%dx%d nodata %d%% radius %d: %.1f%% of the cells have a value, %d landforms"
              % (H, W, nodata_pct, radius, 100.0 * _valued(ref), len(np.unique(ref["landform"]))))
        assert _valued(ref) >= 0.5
        check("horizon px %r" % px, horizon.attributes(dem, px, ALL, radius), ref)


@pytest.mark.parametrize("radius", [4, 5, 16, 17, 32, 33, 64])
def test_radii_on_both_sides_of_a_tile_geometry(radius):
    """the launcher picks the tile and its staged block by radius: <= 4, <= 16, <= 32, <= 64; the last radius of one
    geometry and the first of the next, all five outputs and the instance with the digits alone"""
    dem = synth(200, 333, 2)
    ref = synth_ref(200, 333, 2, 7.3, radius)
    print("radius %d: %.1f%% of the cells have a value" % (radius, 100.0 * _valued(ref)))
    assert _valued(ref) >= 0.5
    check("radius %d" % radius, horizon.attributes(dem, 7.3, ALL, radius), ref)
    check("radius %d, digits" % radius, horizon.attributes(dem, 7.3, ("pattern", "landform"), radius), ref,
          ("pattern", "landform"))


def test_radius_64_on_a_raster_smaller_than_one_haloed_tile():
    dem = synth(150, 200, 2)
    ref = synth_ref(150, 200, 2, 10.0, 64)
    assert _valued(ref) >= 0.5
    check("150 x 200, radius 64", horizon.attributes(dem, 10.0, ALL, 64), ref)


def _random_dem(shape, seed):
    return np.random.default_rng(seed).uniform(10, 400, shape).astype(np.float32)


@pytest.mark.parametrize("radius", [1, 8])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (1, 37), (41, 1), (5, 130), (9, 129)])
def test_odd_shapes(shape, radius):
    """most cells have no value; everything is compared"""
    dem = _random_dem(shape, shape[0] * 1000 + shape[1])
    ref = R.attributes(dem, 7.3, T1, ALL, radius)
    assert (ref["landform"] != 0).sum() == max(shape[0] - 2, 0) * max(shape[1] - 2, 0)
    for k in ALL:
        assert ((ref[k] != NONE[k]) == (ref["landform"] != 0)).all()
    check("shape %s radius %d" % (shape, radius), horizon.attributes(dem, 7.3, ALL, radius), ref)


@pytest.mark.parametrize("radius,skip", [(1, 0), (3, 0), (3, 1), (3, 2), (8, 1), (8, 7), (20, 1), (20, 19), (40, 39)])
def test_skip(radius, skip):
    dem = synth(200, 333, 2)
    ref = synth_ref(200, 333, 2, 7.3, radius, skip)
    assert _valued(ref) >= (0.5 if skip < 16 else 0.2)
    check("radius %d skip %d" % (radius, skip), horizon.attributes(dem, 7.3, ALL, radius, skip), ref)
    if skip:  # the cells skipped matter: another answer than skip = 0
        assert not np.array_equal(ref["pattern"], synth_ref(200, 333, 2, 7.3, radius)["pattern"])


@pytest.mark.parametrize("flat", [0, 1, 30])
def test_flat(flat):
    dem = synth(200, 333, 2)
    seen = []
    for radius in (3, 12):
        ref = synth_ref(200, 333, 2, 10.0, radius, 0, float(flat))
        got = horizon.attributes(dem, 10.0, ALL, radius, 0, flat)
        check("flat %r radius %d" % (flat, radius), got, ref)
        seen.append(np.unique(got["landform"]))
    if flat == 0:  # a zero digit needs tmax == tmin == 0: the synthetic terrain has next to no flat cell
        assert (R.decode(got["pattern"])[:, got["landform"] != 0] == 0).mean() < 0.05
    if flat == 30:  # nothing on this terrain is that steep: all flat
        assert set(seen[0]) <= {0, 1}


def test_output_selection():
    """every single-output call and mixed subsets hold the bytes of the all-outputs call: the subset kernels are other
    template instances (digits / openness / sky view, any combination)"""
    dem = synth(200, 333, 2)
    for radius in (3, 12):
        full = horizon.attributes(dem, 7.3, ALL, radius)
        check("all five", full, synth_ref(200, 333, 2, 7.3, radius))
        asked = [(k,) for k in ALL] + [("sky_view", "landform"), ("negative", "pattern"), ("positive", "sky_view"),
                                       ("positive", "negative"), ALL[::-1]]
        for names in asked:
            got = horizon.attributes(dem, 7.3, names, radius)
            assert tuple(got) == tuple(names)
            for k in names:
                _bits_equal("%s of %s" % (k, names), got[k], full[k])
        _bits_equal("geomorphons()", horizon.geomorphons(dem, 7.3, radius), full["landform"])
        _bits_equal("openness()", horizon.openness(dem, 7.3, radius), full["positive"])
        _bits_equal("openness(negative)", horizon.openness(dem, 7.3, radius, "negative"), full["negative"])
        _bits_equal("sky_view()", horizon.sky_view(dem, 7.3, radius), full["sky_view"])
    d = horizon.attributes(dem, 7.3)
    assert tuple(d) == ("landform",)
    _bits_equal("defaults", d["landform"], synth_ref(200, 333, 2, 7.3, 10)["landform"])


@pytest.mark.parametrize("radius", [1, 4, 12])
def test_duality(radius):
    """attributes(c - dem): digits swapped except at ties (the module docstring above), the dual landform, positive
    and negative exchanged to one float32 spacing"""
    dem = synth(200, 333, 0)  # multiples of 1 / 256 below 64: c - dem is exact in float32
    assert R.valid(dem).all() and dem.max() < 64 and np.array_equal(dem * 256, np.round(dem * 256))
    down = (np.float32(64) - dem).astype(np.float32)
    assert np.array_equal(down.astype(np.float64), 64.0 - dem.astype(np.float64))
    a = horizon.attributes(dem, 7.3, ALL, radius)
    b = horizon.attributes(down, 7.3, ALL, radius)
    check("up", a, R.attributes(dem, 7.3, T1, ALL, radius))
    check("down", b, R.attributes(down, 7.3, T1, ALL, radius))
    has = a["landform"] != 0
    assert np.array_equal(has, b["landform"] != 0) and has.mean() > 0.9
    tmax, tmin = R.extremes(dem, 7.3, radius)
    with np.errstate(invalid="ignore"):
        tie = (np.abs(tmax) == np.abs(tmin)) & (np.abs(tmin) > T1)
    da, db = R.decode(a["pattern"]), R.decode(b["pattern"])
    free = has[None] & ~tie
    assert np.array_equal(db[free], -da[free])
    assert (da[has[None] & tie] == -1).all() and (db[has[None] & tie] == -1).all()
    clean = has & ~tie.any(axis=0)
    print("radius %d: %d of %d valued cells have a tie in some direction" % (radius, (has & ~clean).sum(), has.sum()))
    if radius > 1:  # at radius 1 every direction is a single sample
        assert clean.sum() > 0.8 * has.sum()
        assert len(np.unique(a["landform"][clean])) >= 6
    assert np.array_equal(b["landform"][clean], R.DUAL[a["landform"][clean]])
    for x, y in ((a["positive"], b["negative"]), (a["negative"], b["positive"])):
        assert np.array_equal(x == -100, y == -100)
        d = np.abs(x[has].astype(np.float64) - y[has].astype(np.float64))
        assert (d <= np.spacing(np.maximum(x[has], y[has])).astype(np.float64)).all()


@pytest.mark.parametrize("radius", [1, 3, 8])
def test_non_finite_heights(radius):
    dem = golden("nonfinite")["dem"].astype(np.float32)  # NaN, +inf, -inf and below-sentinel heights
    assert np.isnan(dem).any() and np.isinf(dem).any() and (dem < -100).any()
    ref = R.attributes(dem, 10.0, T1, ALL, radius)
    assert (ref["landform"] != 0).mean() > 0.5 and (ref["landform"][~R.valid(dem)] == 0).all()
    check("nonfinite", horizon.attributes(dem, 10.0, ALL, radius), ref)


def test_nodata_in_a_line_of_sight_is_skipped_across_a_tile_seam():
    """a wall of nodata two cells wide next to a tile seam (column 64): the cells west of it still see the terrain
    east of it, so they keep a value, and the values are the reference's"""
    dem = synth(70, 200, 0).copy()
    dem[:, 64:66] = -100
    dem[20, 30] = np.nan
    ref = R.attributes(dem, 7.3, T1, ALL, 5)
    assert (ref["landform"][8:-8, 60:64] != 0).all() and (ref["landform"][:, 64:66] == 0).all()
    check("wall", horizon.attributes(dem, 7.3, ALL, 5), ref)
    # at radius 2 nothing lies beyond the wall for column 63: no value there
    ref = R.attributes(dem, 7.3, T1, ALL, 2)
    assert (ref["landform"][:, 63] == 0).all() and (ref["landform"][8:-8, 62] != 0).all()
    check("wall, radius 2", horizon.attributes(dem, 7.3, ALL, 2), ref)


def test_analytic_surfaces():
    """the host test's surfaces through the kernel: a level plane, a pit and a peak, a valley and a ridge"""
    level = horizon.attributes(np.full((20, 70), 250, np.float32), 10.0, ALL, 5)
    has = level["landform"] != 0
    assert has.sum() == 18 * 68 and (level["landform"][has] == 1).all() and (level["pattern"][has] == 3280).all()
    assert (level["sky_view"][has] == 1).all() and (level["positive"][has] == np.float32(math.pi / 2)).all()
    assert (level["negative"][has] == np.float32(math.pi / 2)).all()
    cone = R.cone(29, rise=0.7, curl=0.01)
    assert horizon.geomorphons(cone, 10.0, 12)[14, 14] == 2
    assert horizon.geomorphons((np.float32(200) - cone).astype(np.float32), 10.0, 12)[14, 14] == 10
    valley = R.valley_ns(31, 29, rise=0.7, curl=0.01)
    assert (horizon.geomorphons(valley, 10.0, 12)[2:-2, 14] == 9).all()
    assert (horizon.geomorphons((np.float32(300) - valley).astype(np.float32), 10.0, 12)[2:-2, 14] == 3).all()
    slope = horizon.geomorphons(R.plane_east(33, 35, rise=0.7, curl=0.01), 10.0, 12)
    assert (slope[2:-2, 2:-2] == 6).all()


def test_two_runs_give_identical_bytes():
    dem = synth(600, 1000, 2)
    for radius in (3, 20):
        a, b = (horizon.attributes(dem, 7.3, ALL, radius) for _ in range(2))
        for k in ALL:
            _bits_equal("%s, repeated" % k, b[k], a[k])


# ---- the device tier ---------------------------------------------------------------------------------------------
GUARD = 1 << 16  # bytes on either side of every raster


def test_device_tier_on_a_torch_stream_with_guard_bands():
    """dt_dev_horizon on torch tensors, on a context bound to a torch stream: the host tier's bytes, also between two
    calls that take the context's scratch (it uses none); every output raster sits between guard bands of a known
    pattern inside one allocation and the bands come back untouched; an output whose pointer is NULL is left
    untouched; its refusals; an empty raster"""
    import torch
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    L = _lib.lib()
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    H, W = 150, 203  # more than one tile each way in every geometry but the largest, ragged last tiles
    dem = synth(H, W, 2)
    sizes = {k: H * W * np.dtype(DTYPES[k]).itemsize for k in ALL}
    offs, total = {}, GUARD
    for k, nb in sizes.items():
        offs[k] = total
        total += (nb + 255) // 256 * 256 + GUARD
    inside = np.zeros(total, bool)
    for k, nb in sizes.items():
        inside[offs[k]:offs[k] + nb] = True
    try:
        with torch.cuda.stream(st):
            d = torch.from_numpy(dem.copy()).to("cuda")
            fdr = torch.ones((H, W), dtype=torch.uint8, device="cuda")
            up = torch.empty((H, W), dtype=torch.float64, device="cuda")
            for radius, skip, names in ((3, 0, ALL), (5, 1, ("landform", "sky_view")), (17, 0, ("negative",)),
                                        (40, 2, ("pattern", "positive")), (64, 0, ALL)):
                arena = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
                base = arena.data_ptr()
                assert base % 256 == 0
                ptrs = [base + offs[k] if k in names else None for k in ALL]
                _lib.check(L.dt_dev_upslope_length(ctx.h, fdr.data_ptr(), None, H, W, 7.3, up.data_ptr()))
                _lib.check(L.dt_dev_horizon(ctx.h, d.data_ptr(), H, W, 7.3, radius, skip, T1, *ptrs))
                _lib.check(L.dt_dev_upslope_length(ctx.h, fdr.data_ptr(), None, H, W, 7.3, up.data_ptr()))
                ctx.sync()
                assert ctx.status() == 0
                raw = arena.cpu().numpy()
                bad = np.flatnonzero(~inside & (raw != 0xA5))
                assert bad.size == 0, "radius %d: %d guard bytes overwritten, first at %d" % (radius, bad.size, bad[0])
                host = horizon.attributes(dem, 7.3, names, radius, skip)
                for k in ALL:
                    got = raw[offs[k]:offs[k] + sizes[k]]
                    if k in names:
                        _bits_equal("device tier, radius %d, %s" % (radius, k),
                                    got.view(DTYPES[k]).reshape(H, W), host[k])
                    else:
                        assert (got == 0xA5).all(), "radius %d: %s was not asked for and was written" % (radius, k)
                del arena
            arena = torch.empty((total,), dtype=torch.uint8, device="cuda")
            ptrs = [arena.data_ptr() + offs[k] for k in ALL]
            dp = d.data_ptr()
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 0, 0, T1, *ptrs) != 0
            assert b"radius" in L.dt_last_error()
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 65, 0, T1, *ptrs) != 0
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 4, 4, T1, *ptrs) != 0
            assert b"skip" in L.dt_last_error()
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 4, -1, T1, *ptrs) != 0
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 4, 0, float("nan"), *ptrs) != 0
            assert b"flat_tan" in L.dt_last_error()
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 4, 0, -0.5, *ptrs) != 0
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 4, 0, float("inf"), *ptrs) != 0
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 4, 0, T1, *[None] * 5) != 0
            assert b"output" in L.dt_last_error()
            assert L.dt_dev_horizon(ctx.h, None, H, W, 7.3, 4, 0, T1, *ptrs) != 0
            assert b"NULL" in L.dt_last_error()
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 0.0, 4, 0, T1, *ptrs) != 0
            assert L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 0, 0, T1, *[None] * 5) != 0  # the ranges come before the outputs
            assert b"radius" in L.dt_last_error()
            assert L.dt_dev_horizon(ctx.h, None, 0, 0, 7.3, 4, 0, T1, *[None] * 5) == 0
            assert L.dt_dev_horizon(ctx.h, dp, 0, W, 7.3, 4, 0, T1, *ptrs) == 0
            _lib.check(L.dt_dev_horizon(ctx.h, dp, H, W, 7.3, 4, 0, 0.0, *ptrs))  # and the context still works
            ctx.sync()
            assert ctx.status() == 0
    finally:
        ctx.close()
        torch.cuda.empty_cache()
    empty = horizon.attributes(np.zeros((0, 5), np.float32), 10.0, ("pattern", "negative"))
    assert tuple(empty) == ("pattern", "negative") and empty["pattern"].shape == (0, 5)
    assert empty["pattern"].dtype == np.uint16


# ---- the bench tool ----------------------------------------------------------------------------------------------
def test_bench_tool_prints_one_json_line(tmp_path, capsys, monkeypatch):
    """tools/horizon_bench.py under the contract of the op tools (tests/test_gpu_bench_tools.py)"""
    from test_gpu_bench_tools import _times
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    out = tmp_path / "horizon_bench.json"
    importlib.import_module("horizon_bench").main(["--size", "512", "--steps", "2", "--warmup", "1", "--out", str(out)])
    line = capsys.readouterr().out.strip()
    res = json.loads(line)
    assert out.read_text() == line + "\n"
    assert res["tool"] == "horizon_bench" and res["size"] == [512, 512] and res["steps"] == 2 and res["warmup"] == 1
    assert isinstance(res["timing"], str) and res["timing"]
    times = list(_times(res))
    assert len(times) >= 6
    for v in times:
        assert isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0, (v, res)
    assert set(res["ms"]) == {"terrain_r1_all", "r3_landform", "r3_all", "r10_all", "r32_all", "r64_all"}
    assert res["status"] == 0 and 0.5 < res["cells_with_a_value_last_call"] <= 1
