"""GPU (-m gpu): the local terrain attributes (descriptools_amd.terrain, dt_terrain, dt_dev_terrain; k_terrain1 /
k_terrain in dt_terrain.hip) against the numpy reference (tests/_terrain_ref.py).  Every output but aspect: bit for bit.
Aspect has one atan2, and the GPU's and numpy's need not round alike: the same -100 and -1 cells, every other cell
within one float32 spacing (circular across 0 / 360), and at most 16 cells of a raster that differ at all -- the rule
and the reasoning of tests/test_gpu_mfd.py for pow: a few-ulp float64 error moves a float32 rounding in far fewer than
10^-3 of the cells of these rasters."""
import functools
import importlib
import itertools
import json
import math
import os

import numpy as np
import pytest

import oracle
from conftest import golden
from descriptools_amd import terrain

import _terrain_ref as R
from _terrain_ref import paraboloid, plane, sphere_cap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = terrain.OUTPUTS
FIRST = ("gradient", "aspect", "hillshade")
CURV = ("profile", "plan", "tangential", "mean", "laplacian")


def _bits_equal(name, g, r):
    assert g.dtype == r.dtype and g.shape == r.shape, name
    gi, ri = g.view(np.int32), r.view(np.int32)
    if not np.array_equal(gi, ri):
        bad = np.argwhere(gi != ri)
        i = tuple(bad[0])
        raise AssertionError("%s: %d values differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i], r[i]))


def _aspect_close(name, g, r):
    assert g.dtype == r.dtype == np.float32 and g.shape == r.shape, name
    assert np.array_equal(g == -100, r == -100), name + ": cells without a value differ"
    assert np.array_equal(g == -1, r == -1), name + ": flat cells differ"
    live = r >= 0
    assert ((g[live] >= 0) & (g[live] < 360)).all(), name
    g64, r64 = g[live].astype(np.float64), r[live].astype(np.float64)
    d = np.abs(g64 - r64)
    d = np.minimum(d, 360.0 - d)
    tol = np.spacing(np.maximum(g[live], r[live])).astype(np.float64)
    cells = int((g64 != r64).sum())
    print("%s: %d of %d aspects differ from the reference" % (name, cells, live.sum()))
    assert (d <= tol).all(), "%s: an aspect is off by %r" % (name, float((d - tol).max()))
    assert cells <= 16, name


def check(name, got, ref, outputs=ALL):
    assert tuple(got) == tuple(outputs), name
    for k in outputs:
        assert got[k].dtype == np.float32 and got[k].flags.c_contiguous
        (_aspect_close if k == "aspect" else _bits_equal)("%s, %s" % (name, k), got[k], ref[k])


@functools.lru_cache(maxsize=None)
def synth(H, W, nodata_pct):
    dem = oracle.synth_dem(11, H, W, nodata_pct=nodata_pct)
    dem.setflags(write=False)
    return dem


@functools.lru_cache(maxsize=None)
def synth_ref(H, W, nodata_pct, px, radius):
    """the reference's eight outputs on a synthetic terrain, computed once and read-only"""
    ref = R.attributes(synth(H, W, nodata_pct), px, ALL, radius)
    for v in ref.values():
        v.setflags(write=False)
    return ref


CASES = [(H, W, nod, r) for (H, W, nod) in ((200, 333, 0), (200, 333, 2), (600, 1000, 2)) for r in (1, 2, 5)]
CASES.append((200, 333, 2, 16))


@pytest.mark.parametrize("H,W,nodata_pct,radius", CASES)
def test_bit_for_bit_on_terrain(H, W, nodata_pct, radius):
    dem = synth(H, W, nodata_pct)
    for px in (10.0, 7.3):
        ref = synth_ref(H, W, nodata_pct, px, radius)
        has = ref["gradient"] != -100
        print("%dx%d nodata %d%% radius %d: %.1f%% of the cells have a value"
              % (H, W, nodata_pct, radius, 100.0 * has.mean()))
        assert has.mean() >= 0.5
        check("terrain px %r" % px, terrain.attributes(dem, px, ALL, radius), ref)


@pytest.mark.parametrize("radius", [4, 5, 12, 13, 20, 21])
def test_radii_on_both_sides_of_a_tile_geometry(radius):
    """the launcher picks the tile and its LDS planes by radius: <= 4, <= 12, <= 20, <= 32; the last radius of one
    geometry and the first of the next, all eight outputs and the variant without second moments"""
    dem = synth(200, 333, 2)
    ref = synth_ref(200, 333, 2, 7.3, radius)
    assert (ref["gradient"] != -100).mean() > 0.5
    check("radius %d" % radius, terrain.attributes(dem, 7.3, ALL, radius), ref)
    check("radius %d, first derivatives" % radius, terrain.attributes(dem, 7.3, FIRST, radius), ref, FIRST)


def _random_dem(shape, seed):
    return np.random.default_rng(seed).uniform(10, 400, shape).astype(np.float32)


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (1, 37), (41, 1), (3, 130), (9, 129)])
def test_odd_shapes_radius_1(shape):
    dem = _random_dem(shape, shape[0] * 1000 + shape[1])
    ref = R.attributes(dem, 7.3, ALL, 1)
    assert (ref["gradient"] != -100).sum() == max(shape[0] - 2, 0) * max(shape[1] - 2, 0)
    check("shape %s" % (shape,), terrain.attributes(dem, 7.3, ALL, 1), ref)
    check("shape %s, first derivatives" % (shape,), terrain.attributes(dem, 7.3, FIRST, 1), ref, FIRST)


@pytest.mark.parametrize("radius", [2, 7, 32])
def test_odd_shapes_larger_radii(radius):
    r = radius
    for shape, valued in (((2 * r + 1, 2 * r + 1), 1), ((2 * r, 2 * r + 40), 0), ((2 * r + 9, 2 * r + 129), 9 * 129)):
        dem = _random_dem(shape, r * 100 + shape[1])
        ref = R.attributes(dem, 7.3, ALL, r)
        has = ref["gradient"] != -100
        assert has.sum() == valued
        if valued > 1:  # values on both sides of a 128-column tile seam
            assert has[:, :128].any() and has[:, 128:].any()
        check("radius %d shape %s" % (r, shape), terrain.attributes(dem, 7.3, ALL, r), ref)
        check("radius %d shape %s, first derivatives" % (r, shape), terrain.attributes(dem, 7.3, FIRST, r), ref, FIRST)


@pytest.mark.parametrize("radius", [1, 3, 8])
def test_tile_seams_and_the_window_rule(radius):
    """a single nodata cell on a tile's last row, a NaN on a tile's first column and a +inf inside a tile (rows 31 and
    columns 128 end and begin a tile of every kernel: 128 x 8 at radius 1, 64 x 16 above): exactly the (2 r + 1)^2
    cells around it lose their value, every other cell keeps its bytes"""
    r = radius
    H, W = 70, 300
    base = synth(H, W, 0)
    assert R.valid(base).all()
    clean = terrain.attributes(base, 7.3, ALL, r)
    check("clean", clean, R.attributes(base, 7.3, ALL, r))
    for value, y, x in ((np.float32(-100), 31, 100), (np.float32("nan"), 40, 128), (np.float32("inf"), 50, 200)):
        assert r <= y < H - r and r <= x < W - r
        dem = base.copy()
        dem[y, x] = value
        got = terrain.attributes(dem, 7.3, ALL, r)
        lost = np.zeros((H, W), bool)
        lost[y - r:y + r + 1, x - r:x + r + 1] = True
        assert lost.sum() == (2 * r + 1) ** 2
        for k in ALL:
            assert (got[k][lost] == -100).all(), (k, value)
            assert (clean[k][lost] != -100).all(), k
            _bits_equal("%s beside a planted %r" % (k, value), got[k][~lost], clean[k][~lost])


@pytest.mark.parametrize("radius", [1, 2])
def test_non_finite_heights(radius):
    dem = golden("nonfinite")["dem"].astype(np.float32)  # NaN, +inf, -inf and below-sentinel heights
    assert np.isnan(dem).any() and np.isinf(dem).any() and (dem < -100).any()
    ref = R.attributes(dem, 10.0, ALL, radius)
    assert (ref["gradient"] != -100).any() and (ref["gradient"][~R.valid(dem)] == -100).all()
    check("nonfinite", terrain.attributes(dem, 10.0, ALL, radius), ref)


@pytest.mark.parametrize("radius", [1, 3])
def test_output_selection(radius):
    """a single output, and each pair of a first-derivative and a curvature output, hold the bytes of the all-eight
    call; so does the first-derivative-only call, which runs the variant without second moments"""
    dem = synth(200, 333, 2)
    full = terrain.attributes(dem, 7.3, ALL, radius, 200.0, 30.0)
    check("all eight", full, R.attributes(dem, 7.3, ALL, radius, 200.0, 30.0))
    asked = [(k,) for k in ALL] + list(itertools.product(FIRST, CURV)) + [FIRST, ("hillshade", "aspect", "gradient"),
                                                                          CURV[::-1]]
    for names in asked:
        got = terrain.attributes(dem, 7.3, names, radius, 200.0, 30.0)
        assert tuple(got) == tuple(names)
        for k in names:
            _bits_equal("%s of %s" % (k, names), got[k], full[k])
    _bits_equal("gradient()", terrain.gradient(dem, 7.3, radius), full["gradient"])
    _bits_equal("aspect()", terrain.aspect(dem, 7.3, radius), full["aspect"])
    _bits_equal("hillshade()", terrain.hillshade(dem, 7.3, 200.0, 30.0, radius), full["hillshade"])
    for kind in CURV:
        _bits_equal("curvature(%s)" % kind, terrain.curvature(dem, 7.3, kind, radius), full[kind])


@pytest.mark.parametrize("radius", [1, 3, 8])
def test_analytic_plane_and_paraboloid(radius):
    dem = plane(40, 50, 3, -4)
    out = terrain.attributes(dem, 1.0, ALL, radius)
    check("plane", out, R.attributes(dem, 1.0, ALL, radius))
    has = out["gradient"] != -100
    assert has.sum() == (40 - 2 * radius) * (50 - 2 * radius)
    for k in CURV:
        assert (out[k][has] == 0).all(), k
    assert (out["gradient"][has] == 5).all()
    dem = paraboloid(41, 41)
    out = terrain.attributes(dem, 1.0, ALL, radius)
    check("paraboloid", out, R.attributes(dem, 1.0, ALL, radius))
    has = out["gradient"] != -100
    assert has.sum() == (41 - 2 * radius) ** 2 and (out["laplacian"][has] == 4).all()
    assert out["gradient"][20, 20] == 0 and out["aspect"][20, 20] == -1 and out["profile"][20, 20] == 0


def test_analytic_aspect_and_hillshade():
    for (a, b), want in (((0, -1), 0.0), ((-1, 0), 90.0), ((0, 1), 180.0), ((1, 0), 270.0)):
        got = terrain.aspect(plane(9, 140, a, b), 2.0)
        assert (got[1:-1, 1:-1] == np.float32(want)).all(), (a, b)
    for alt in (45.0, 30.0, 90.0):
        hs = terrain.hillshade(np.full((7, 8), 120, np.float32), 10.0, altitude=alt)
        assert (hs[1:-1, 1:-1] == np.float32(math.sin(math.radians(alt)))).all() and (hs[0] == -100).all()


@pytest.mark.parametrize("radius", [1, 4])
def test_analytic_sphere_cap(radius):
    """On float32 heights: the reference bit for bit, and convex is positive.  That the reference gives +1 / R within
    1e-6 is the host test's, on float64 heights: the rounding of a float32 height of size R is far above 1e-6 of a
    second difference."""
    R_, px = 500.0, 5.0
    dem = sphere_cap(61, 61, R_, px).astype(np.float32)
    out = terrain.attributes(dem, px, ALL, radius)
    check("sphere", out, R.attributes(dem, px, ALL, radius))
    sel = (out["gradient"] != -100) & (out["gradient"] > 0.05)
    assert sel.sum() > 1000
    for k in ("profile", "plan", "tangential", "mean"):
        assert (out[k][sel] > 0).all(), k
    assert (out["laplacian"][sel] < 0).all()


def test_two_runs_give_identical_bytes():
    dem = synth(600, 1000, 2)
    for radius in (1, 5):
        a, b = (terrain.attributes(dem, 7.3, ALL, radius) for _ in range(2))
        for k in ALL:
            _bits_equal("%s, repeated" % k, b[k], a[k])


# ---- the device tier ---------------------------------------------------------------------------------------------
def test_device_tier():
    """dt_dev_terrain on a context and a device DEM equals the host tier, also between two calls that take the
    context's scratch (it uses none); its refusals; an empty raster"""
    from descriptools_amd import _lib, device
    H, W = 200, 333
    dem = synth(H, W, 2)
    sun = terrain.sun_vector(200.0, 30.0)
    ctx = device.Context()
    L = _lib.lib()
    d = ctx.to_device(dem)
    outs = [ctx.empty((H, W), np.float32) for _ in ALL]
    fdr = ctx.to_device(np.ones((H, W), np.uint8))
    up = ctx.empty((H, W), np.float64)
    try:
        for radius in (1, 5):
            host = terrain.attributes(dem, 7.3, ALL, radius, 200.0, 30.0)
            _lib.check(L.dt_dev_upslope_length(ctx.h, fdr.ptr, None, H, W, 7.3, up.ptr))
            _lib.check(L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, radius, *sun, *[o.ptr for o in outs]))
            _lib.check(L.dt_dev_upslope_length(ctx.h, fdr.ptr, None, H, W, 7.3, up.ptr))
            assert ctx.status() == 0
            for k, o in zip(ALL, outs):
                _bits_equal("device tier, radius %d, %s" % (radius, k), o.to_host(), host[k])
            # two outputs only: the others keep their bytes
            keep = outs[2].to_host()
            ptrs = [outs[0].ptr, None, None, None, None, None, None, outs[7].ptr]
            _lib.check(L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, radius, *sun, *ptrs))
            _bits_equal("gradient alone", outs[0].to_host(), host["gradient"])
            _bits_equal("hillshade alone", outs[7].to_host(), host["hillshade"])
            _bits_equal("profile untouched", outs[2].to_host(), keep)
        ptrs = [o.ptr for o in outs]
        assert L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, 0, *sun, *ptrs) != 0
        assert b"radius" in L.dt_last_error()
        assert L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, 33, *sun, *ptrs) != 0
        assert L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, 1, float("nan"), sun[1], sun[2], *ptrs) != 0
        assert b"sun" in L.dt_last_error()
        assert L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, 1, sun[0], sun[1], float("inf"), *ptrs) != 0
        assert L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, 1, *sun, *[None] * 8) != 0
        assert b"output" in L.dt_last_error()
        assert L.dt_dev_terrain(ctx.h, d.ptr, H, W, 0.0, 1, *sun, *ptrs) != 0
        assert L.dt_dev_terrain(ctx.h, None, 0, 0, 7.3, 1, *sun, *[None] * 8) == 0
        assert L.dt_dev_terrain(ctx.h, d.ptr, 0, W, 7.3, 1, *sun, *ptrs) == 0
        _lib.check(L.dt_dev_terrain(ctx.h, d.ptr, H, W, 7.3, 1, *sun, *ptrs))  # and the context still works
        assert ctx.status() == 0
    finally:
        for b in [d, fdr, up] + outs:
            b.free()
        ctx.close()
    empty = terrain.attributes(np.zeros((0, 5), np.float32), 10.0)
    assert tuple(empty) == ("gradient", "aspect") and empty["aspect"].shape == (0, 5)


# ---- the bench tool ----------------------------------------------------------------------------------------------
def test_bench_tool_prints_one_json_line(tmp_path, capsys, monkeypatch):
    """tools/terrain_bench.py under the contract of the op tools (tests/test_gpu_bench_tools.py)"""
    from test_gpu_bench_tools import _times
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    out = tmp_path / "terrain_bench.json"
    importlib.import_module("terrain_bench").main(["--size", "512", "--steps", "2", "--warmup", "1", "--out", str(out)])
    line = capsys.readouterr().out.strip()
    res = json.loads(line)
    assert out.read_text() == line + "\n"
    assert res["tool"] == "terrain_bench" and res["size"] == [512, 512] and res["steps"] == 2 and res["warmup"] == 1
    assert isinstance(res["timing"], str) and res["timing"]
    times = list(_times(res))
    assert len(times) >= 3
    for v in times:
        assert isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0, (v, res)
    assert set(res["ms"]) == {"dinf_direction", "r1_gradient_aspect", "r1_all", "r4_all", "r16_all"}
    assert res["status"] == 0 and 0.5 < res["cells_with_a_value_last_call"] <= 1
