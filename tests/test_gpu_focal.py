"""GPU (-m gpu): descriptools_amd.focal against the numpy reference of tests/_focal_ref.py, bit for bit.

Float outputs are compared as their uint32 views and their NaN positions as masks.  The shapes are the smallest at which
a scan can go wrong: they straddle 64 and 128 (wave seams) and 1024 and 2048 on each axis separately and on both.  The
kernels' own constants are not all among those: k_fc_scan walks a row in chunks of 256 columns (FC_CHUNK, and the 256
columns of a k_fc_band_sums block) and cuts the rows into bands of 8 (FC_BH), so widths 255, 256, 257 and heights 7, 8, 9
are added -- (8, 256) also takes the 16-byte path, as (1100, 1300) does, the odd widths the scalar one."""
import ctypes as C
import math

import numpy as np
import pytest

import _focal_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (3, 3), (67, 131), (130, 2051), (2051, 67), (1100, 1300),
          (7, 255), (8, 256), (9, 257)]
_CACHE = {}


def _dem(shape):
    if shape not in _CACHE:
        d = R.terrain(shape[0], shape[1], seed=shape[0] * 7 + shape[1], holes=shape[0] * shape[1] >= 64)
        d.setflags(write=False)
        _CACHE[shape] = d
    return _CACHE[shape]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), "%s: NaN positions differ at %d cells" % (what, int((gn != wn).sum()))
        got, want = np.where(gn, np.float32(0), got), np.where(wn, np.float32(0), want)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), "%s: %d cells differ, first at %s: %r, reference %r" % (
        what, int(diff.sum()), tuple(np.argwhere(diff)[0]), got[diff][0], want[diff][0])


@pytest.mark.parametrize("radius", [1, 2, 7, 64, "whole"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_statistics_equal_the_reference_bit_for_bit(shape, radius):
    from descriptools_amd import focal
    dem = _dem(shape)
    r = max(shape) if radius == "whole" else radius
    origin, s = R.default_origin(dem), focal.default_frac_bits(dem, r)
    got = focal.statistics(dem, r, focal.OUTPUTS)
    want = R.statistics(dem, r, origin, s)
    assert list(got) == list(focal.OUTPUTS)
    if shape[0] * shape[1] >= 64:
        assert np.isnan(want["tpi"]).any() and (want["mean"] == -100).any()
    for k in focal.OUTPUTS:
        _assert_same(got[k], want[k], "%s at radius %d" % (k, r))


def test_exact_where_the_table_wraps():
    from descriptools_amd import focal
    dem = R.wrap_case()
    ok, q = R.quantise(dem, R.WRAP["origin"], R.WRAP["frac_bits"])
    assert sum(int(v) ** 2 for v in q.reshape(-1)) > 2 ** 64
    got = focal.statistics(dem, R.WRAP["radius"], focal.OUTPUTS, R.WRAP["frac_bits"], R.WRAP["origin"])
    want = R.statistics(dem, **R.WRAP)
    for k in focal.OUTPUTS:
        _assert_same(got[k], want[k], k)


@pytest.mark.parametrize("shape", [(130, 300), (1100, 1300)], ids=lambda s: "%dx%d" % s)
def test_dev_max_equals_the_reference_bit_for_bit(shape):
    from descriptools_amd import focal
    dem = _dem(shape) if shape in SHAPES else R.terrain(shape[0], shape[1], seed=5)
    radii = (1, 3, 10, 40)
    origin, s = R.default_origin(dem), focal.default_frac_bits(dem, radii[-1])
    dev, scale = focal.dev_max(dem, radii)
    wdev, wscale = R.dev_max(dem, radii, origin, s)
    assert len(np.unique(wscale)) == 5  # every radius is taken somewhere, and 0
    _assert_same(dev, wdev, "dev")
    _assert_same(scale, wscale, "scale")


def test_dev_max_tie_keeps_the_smaller_radius():
    from descriptools_amd import focal
    dev, scale = focal.dev_max(np.full((40, 50), 123, np.float32), (1, 3, 10))
    assert dev.dtype == np.float32 and scale.dtype == np.uint16
    assert (dev == 0).all() and (scale == 1).all()


def test_dev_max_of_one_radius_is_dev():
    from descriptools_amd import focal
    dem = _dem((67, 131))
    ok = R.valid(dem)
    dev, scale = focal.dev_max(dem, (6,))
    _assert_same(dev, focal.dev(dem, 6), "dev")
    assert (scale[ok] == 6).all() and (scale[~ok] == 0).all() and np.isnan(dev[~ok]).all()


# ---- analytic cases at frac_bits = 0, integer heights ------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 3, 6])
def test_plane(radius):
    from descriptools_amd import focal
    H, W = 20, 30
    y, x = np.mgrid[0:H, 0:W]
    out = focal.statistics((3 * x + 2 * y).astype(np.float32), radius, ("tpi", "std", "count"), frac_bits=0, origin=0.0)
    inner = (slice(radius, H - radius), slice(radius, W - radius))
    assert (out["count"][inner] == (2 * radius + 1) ** 2).all()
    assert (out["tpi"][inner] == 0).all()
    assert (out["std"][inner] == np.float32(math.sqrt(13 * radius * (radius + 1) / 3))).all()


def test_constant_raster():
    from descriptools_amd import focal
    H, W, r = 11, 17, 4
    out = focal.statistics(np.full((H, W), 57, np.float32), r, focal.OUTPUTS, frac_bits=0, origin=0.0)
    assert (out["std"] == 0).all() and (out["dev"] == 0).all() and (out["mean"] == 57).all() and (out["tpi"] == 0).all()
    y, x = np.mgrid[0:H, 0:W]
    area = (np.minimum(y + r, H - 1) - np.maximum(y - r, 0) + 1) * (np.minimum(x + r, W - 1) - np.maximum(x - r, 0) + 1)
    assert np.array_equal(out["count"], area.astype(np.int32))
    assert out["count"][0, 0] == 25 and out["count"][5, 8] == 81


@pytest.mark.parametrize("at,n", [((10, 12), 49), ((0, 0), 16), ((20, 5), 28)])
def test_single_spike(at, n):
    from descriptools_amd import focal
    h = 980.0  # h / n is exact for 49, 16 and 28
    dem = np.zeros((21, 25), np.float32)
    dem[at] = h
    out = focal.statistics(dem, 3, ("tpi", "count"), frac_bits=0, origin=0.0)
    assert out["count"][at] == n
    assert out["tpi"][at] == np.float32(h - h / n)


# ---- the two tiers ---------------------------------------------------------------------------------------------------
GUARD = 1 << 12  # bytes on either side of every raster
NAMES = ("count", "mean", "std", "tpi", "dev", "scale")


def _radii(rs):
    return (C.c_int32 * len(rs))(*rs)


def _dev_call(ctx, dem_dev, H, W, origin, s, radii, ask):
    """dt_dev_focal into an arena of guarded rasters -> (arena bytes on the host, offsets, sizes)"""
    from descriptools_amd import _lib
    sizes = {n: H * W * (2 if n == "scale" else 4) for n in NAMES}
    offs, total = {}, GUARD
    for n in NAMES:
        offs[n] = total
        total += (sizes[n] + 255) // 256 * 256 + GUARD
    arena = ctx.to_device(np.full(total, 0xA5, np.uint8))
    try:
        base = arena.ptr.value
        assert base % 256 == 0
        _lib.check(_lib.lib().dt_dev_focal(ctx.h, dem_dev.ptr, H, W, origin, s, _radii(radii), len(radii),
                                           *[base + offs[n] if n in ask else None for n in NAMES]))
        ctx.sync()
        return arena.to_host(), offs, sizes
    finally:
        arena.free()


@pytest.mark.parametrize("ask,radii", [(("tpi",), (5,)), (("count", "std"), (5,)), (("mean", "dev", "scale"), (5,)),
                                       (NAMES, (300,)), (("dev",), (2, 9)), (("scale",), (2, 9)),
                                       (("dev", "scale"), (1, 3, 10, 40))])
def test_only_requested_outputs_are_written(ask, radii):
    from descriptools_amd import focal
    from descriptools_amd.device import Context
    dem = _dem((67, 131))
    H, W = dem.shape
    origin, s = R.default_origin(dem), focal.default_frac_bits(dem, radii[-1])
    ctx = Context()
    try:
        d = ctx.to_device(dem)
        host, offs, sizes = _dev_call(ctx, d, H, W, origin, s, radii, ask)
        assert ctx.status() == 0
        d.free()
    finally:
        ctx.close()
    inside = np.zeros(host.size, bool)
    for n in ask:
        inside[offs[n]:offs[n] + sizes[n]] = True
    bad = np.flatnonzero(~inside & (host != 0xA5))
    assert bad.size == 0, "%d bytes outside the requested rasters were written, first at %d (rasters at %s)" % (
        bad.size, int(bad[0]), offs)
    # and what was asked for is the host tier's, byte for byte
    if len(radii) == 1:
        want = dict(focal.statistics(dem, radii[0], focal.OUTPUTS))
        want["scale"] = np.where(R.valid(dem), np.uint16(radii[0]), np.uint16(0)).astype(np.uint16)
    else:
        want = dict(zip(("dev", "scale"), focal.dev_max(dem, radii)))
    for n in ask:
        assert host[offs[n]:offs[n] + sizes[n]].tobytes() == want[n].tobytes(), n


def test_two_runs_agree_byte_for_byte():
    from descriptools_amd import focal
    dem = _dem((130, 2051))
    a = focal.statistics(dem, 33, focal.OUTPUTS)
    b = focal.statistics(dem, 33, focal.OUTPUTS)
    for k in focal.OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
    m1, m2 = focal.dev_max(dem, (2, 33, 500)), focal.dev_max(dem, (2, 33, 500))
    assert m1[0].tobytes() == m2[0].tobytes() and m1[1].tobytes() == m2[1].tobytes()


def test_device_tier_refusals():
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    L = _lib.lib()
    ctx = Context()
    try:
        d = ctx.to_device(np.zeros((4, 5), np.float32))
        o = ctx.empty((4, 5), np.float32)
        call = lambda origin=0.0, s=0, radii=(1,), n=None, outs=(None, None, None, o.ptr, None, None), dem=d.ptr, H=4: \
            L.dt_dev_focal(ctx.h, dem, H, 5, origin, s, _radii(radii) if radii else None,
                           len(radii) if n is None else n, *outs)
        for kw, msg in ((dict(radii=(0,)), b"[1, 4096]"), (dict(radii=(4097,)), b"[1, 4096]"),
                        (dict(radii=(2, 2)), b"strictly increasing"), (dict(radii=(1,), n=0), b"1..32 radii"),
                        (dict(radii=tuple(range(1, 34))), b"1..32 radii"), (dict(radii=None, n=1), b"1..32 radii"),
                        (dict(s=-1), b"frac_bits"), (dict(s=25), b"frac_bits"),
                        (dict(origin=float("nan")), b"origin"), (dict(origin=float("inf")), b"origin"),
                        (dict(radii=(1, 2)), b"only dev and scale"), (dict(outs=(None,) * 6), b"no output raster"),
                        (dict(dem=None), b"NULL raster"), (dict(H=-1), b"negative raster shape")):
            assert call(**kw) == -1, kw
            assert msg in L.dt_last_error(), (kw, L.dt_last_error())
        assert call(H=0) == 0 and call() == 0
        assert ctx.status() == 0
        d.free()
        o.free()
    finally:
        ctx.close()


def test_height_outside_the_contract_is_an_error_in_both_tiers():
    """an origin above a valid height: the kernels count that cell as q = 0 and raise DT_STATUS_BAD_HEIGHT; nothing is
    read or written out of bounds, and the next call on the context is clean"""
    from descriptools_amd import _lib, focal
    from descriptools_amd.device import Context
    from descriptools_amd._lib import c_f32p, c_i32p, ptr
    L = _lib.lib()
    dem = _dem((67, 131))
    H, W = dem.shape
    origin = R.default_origin(dem)
    ctx = Context()
    try:
        d = ctx.to_device(dem)
        host, offs, sizes = _dev_call(ctx, d, H, W, origin + 50.0, 4, (5,), ("tpi", "count"))
        with pytest.raises(ValueError, match="DT_STATUS_BAD_HEIGHT"):
            ctx.raise_on_status()
        assert ctx.status() == 0  # reading clears it
        # over the bound: frac_bits 24 at radius 4096
        _dev_call(ctx, d, H, W, origin, 24, (4096,), ("dev",))
        assert ctx.status() == 64
        host, offs, sizes = _dev_call(ctx, d, H, W, origin, 4, (5,), ("tpi",))
        assert ctx.status() == 0
        assert host[offs["tpi"]:offs["tpi"] + sizes["tpi"]].tobytes() == \
            focal.statistics(dem, 5, ("tpi",), 4, origin)["tpi"].tobytes()
        d.free()
    finally:
        ctx.close()
    out = np.empty((H, W), np.float32)
    rs = np.array([5], np.int32)
    rc = L.dt_focal(ptr(dem, c_f32p), H, W, origin + 50.0, 4, ptr(rs, c_i32p), 1, None, None, None, ptr(out, c_f32p),
                    None, None)
    msg = L.dt_last_error().decode()
    assert rc == -1
    assert "origin=%d" % (origin + 50) in msg and "frac_bits=4" in msg and str(R.qmax(5)) in msg, msg


# ---- the bench tool ----------------------------------------------------------------------------------------------
def test_bench_tool_prints_one_json_line(tmp_path, capsys, monkeypatch):
    """tools/focal_bench.py under the contract of the op tools (tests/test_gpu_bench_tools.py)"""
    import importlib
    import json
    import os
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    out = tmp_path / "focal_bench.json"
    importlib.import_module("focal_bench").main(["--size", "512", "--steps", "2", "--warmup", "1", "--out", str(out)])
    line = capsys.readouterr().out.strip()
    res = json.loads(line)
    assert out.read_text() == line + "\n"
    assert res["tool"] == "focal_bench" and res["size"] == [512, 512] and res["steps"] == 2 and res["warmup"] == 1
    assert isinstance(res["timing"], str) and res["timing"]
    assert set(res["ms"]) == {"copy_28B_per_cell", "r4_tpi", "r4_all", "r64_tpi", "r64_all", "r1024_tpi", "r1024_all",
                              "dev_max_8", "dev_max_32", "terrain_r32_gradient"}
    for k, v in res["ms"].items():
        assert math.isfinite(v) and v > 0, (k, v)
        assert 0 < res["ms_min_max"][k][0] <= res["ms_min_max"][k][1]
    assert set(res["dev_max_ms_per_radius"]) == {"8", "32"} and min(res["dev_max_ms_per_radius"].values()) > 0
    assert res["status"] == 0 and 20 <= res["scratch_bytes_per_cell"] <= 24
