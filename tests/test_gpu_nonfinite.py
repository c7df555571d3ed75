"""GPU (-m gpu): NaN, +inf, -inf and finite heights below the -100 sentinel on every GPU path.  A float GeoTIFF whose
nodata value is NaN reaches the chain with NaN cells (rasterio_lite.read_masked maps only < -1e30 and a finite nodata
value to -100).  The oracle is pinned to the reference's own run on such a DEM (tests/golden/nonfinite*.npz,
tests/test_oracle_golden.py); here every kernel path is held to that oracle, with the special values placed on the
seams where the kernels change behaviour: stencil tiles (x = 0, 255 mod 256; y = 0, 15 mod 16), 64 x 64 flow tiles,
raster borders and corners, rank borders and halos."""
import numpy as np
import pytest

import oracle
from conftest import assert_float_close, golden

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)
SPECIAL = (NAN, INF, -INF, np.float32(-250), NAN, np.float32(-9999), INF, NAN)
ALL = ("slope", "fdr", "fac", "river", "fdist", "idx", "hand", "a_river", "slope_rad", "ti", "mti", "gfi", "lnhlh",
       "down")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def seam_dem(seed, H, W, nod=4, extra=()):
    """synthetic float32 DEM with the special values on tile seams, borders, corners and in touching pairs"""
    dem = oracle.synth_dem(seed, 4096, 4096, 200, 300, H, W, nod)
    ys = sorted({y for y in (0, 1, 15, 16, 31, 32, 47, 63, 64, 65, 79, 127, 128, H - 2, H - 1) if 0 <= y < H})
    xs = sorted({x for x in (0, 1, 63, 64, 127, 128, 255, 256, 257, 511, 512, 767, 768, 1000, W - 2, W - 1)
                 if 0 <= x < W})
    k = seed
    for y in ys:
        for x in xs:
            if (y * 7 + x * 3 + seed) % 3 == 0:
                dem[y, x] = SPECIAL[k % len(SPECIAL)]
                k += 1
    for y, x, v in extra:
        dem[y % H, x % W] = v
    # pairs of touching special values, and specials next to -100
    for j, (y, x) in enumerate(((H // 2, W // 3), (H // 3, W // 2), (H - 3, 2), (2, W - 3))):
        dem[y, x] = SPECIAL[j % len(SPECIAL)]
        dem[y, x + 1] = SPECIAL[(j + 1) % len(SPECIAL)]
        dem[y + 1, x] = SPECIAL[(j + 2) % len(SPECIAL)]
    ny, nx = np.nonzero(dem == -100)
    for i in range(0, len(ny), max(1, len(ny) // 6)):
        y, x = ny[i], nx[i]
        if x + 1 < W and dem[y, x + 1] != -100:
            dem[y, x + 1] = NAN
    for corner in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        if dem[corner] > -100 and np.isfinite(dem[corner]):
            dem[corner] = NAN
    return dem


def oracle_chain(dem, px, thr, dz=5.0):
    """every output of the resident chain from the (fixture-pinned) oracle; slope_rad is compared apart"""
    sl, fdr = oracle.slope_d8(dem, px)
    acc = oracle.flowacc(fdr, dem)
    river = (acc > thr).astype(np.int8)
    fd, idx, hand = oracle.flowhand(dem, fdr, river, px)
    flat = acc.reshape(-1)
    a_river = np.where(idx != -100, flat[np.where(idx != -100, idx, 0)], -100)
    return {"slope": sl, "fdr": fdr, "fac": acc, "river": river, "fdist": fd, "idx": idx, "hand": hand,
            "a_river": a_river, "gfi": oracle.gfi(hand, acc, idx, 0.4, 0.1, px),
            "lnhlh": oracle.lnhlh(hand, acc, 0.4, 0.1, px), "down": oracle.downslope(dem, fdr, px, dz)}


def check_chain(out, dem, px, thr, what):
    ref = oracle_chain(dem, px, thr)
    for k in ("slope", "fdr", "fac", "river", "fdist", "idx", "hand", "a_river", "down"):
        got = np.asarray(out[k])
        assert same(got, ref[k].astype(got.dtype)), "%s %s: %d cells differ" % (
            what, k, int((~((got == ref[k]) | (np.isnan(got) & np.isnan(ref[k].astype(np.float64))))).sum()))
    slr = np.where(dem == -100, -100, np.arctan(ref["slope"].astype(np.float32) / 100)).astype(np.float32)
    fin = np.isfinite(slr)
    assert np.array_equal(np.isnan(out["slope_rad"]), np.isnan(slr)), what + " slope_rad NaN"
    assert np.max(np.abs(out["slope_rad"][fin].astype(np.float64) - slr[fin])) <= 2.4e-7, what + " slope_rad"
    ti_o, mti_o = oracle.twi(ref["fac"], out["slope_rad"], px, 0.1)
    assert_float_close(out["ti"], ti_o, rtol=1e-5, what=what + " ti")
    assert_float_close(out["mti"], mti_o, rtol=1e-5, atol=1e-6, what=what + " mti")
    assert_float_close(out["gfi"], ref["gfi"], rtol=1e-5, atol=1e-6, what=what + " gfi")
    assert_float_close(out["lnhlh"], ref["lnhlh"], rtol=1e-5, atol=1e-6, what=what + " lnhlh")
    return ref


def chain_once(dem, px, thr, heights="float32", overlap=False, **kw):
    from descriptools_amd import chain, device
    H, W = dem.shape
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=px, overlap=overlap, tune_placement=False, heights=heights,
                     river_threshold=thr, **kw)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float64 if heights == "float64" else np.float32))
    try:
        ch.run(d.ptr)
        ctx.sync()
        ch.check_status()
        ch.finish_long_walks()
        ctx.sync()
        out = {k: ch.buf[k].to_host() for k, _ in ch.outputs}
    finally:
        d.free()
        ch.free()
        ctx.close()
    return out


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heights", ["float32", "float64"])
def test_drop_in_functions_on_the_reference_fixture(heights):
    """tests/golden/nonfinite.npz through the drop-in functions, on both height tiers"""
    from descriptools_amd import downslope, flowacc, flowdir, flowhand, gfi, slope, topoindexes
    g = golden("nonfinite")
    dem, px, fdr_g = g["dem"], float(g["px"]), g["fdr"]
    fdr, sl = flowdir.d8(dem, px, return_slope=True, heights=heights)
    assert np.array_equal(fdr, fdr_g), "D8: %d cells differ" % int((fdr != fdr_g).sum())
    assert np.array_equal(sl, g["slope"])
    assert np.array_equal(np.asarray(slope.sloper(dem, px), np.float32), g["slope"])
    assert np.array_equal(flowacc.accumulate(fdr_g, dem), g["fac"])
    fd, idx, hand = flowhand.flow_hand_index(dem, fdr_g, g["river"], px)
    assert np.array_equal(idx, g["idx"]) and np.array_equal(fd, g["fdist"])
    assert same(np.asarray(hand, np.float32), g["hand"])
    ti, mti = topoindexes.topographic_index(g["fac"], g["slope_rad"], px, float(g["n_top"]))
    assert_float_close(ti, g["ti"], rtol=1e-5, what="ti")
    assert_float_close(mti, g["mti"], rtol=1e-5, atol=1e-6, what="mti")
    assert_float_close(gfi.gfi_calculator(g["hand"], g["fac"], g["idx"], 0.4, 0.1, px), g["gfi"], rtol=1e-5,
                       atol=1e-6, what="gfi")
    assert_float_close(gfi.ln_hl_H_calculator(g["hand"], g["fac"], 0.4, 0.1, px), g["lnhlh"], rtol=1e-5, atol=1e-6,
                       what="lnhlh")
    want = oracle.downslope(dem, fdr_g, px, 5.0)   # the reference's downslope with its pits at 0 (oracle-pinned)
    assert same(downslope.downsloper(dem, fdr_g, px, 5), want)
    assert np.isnan(want[np.isnan(dem) | np.isposinf(dem)]).all()
    # the repair form: the -50 cells of a given raster are filled in, everything else kept
    given = downslope.downslope_cpu(dem, fdr_g, px, 5)
    fixed = downslope.downslope_sequential_jit(dem, fdr_g, px, 5, downslope=given.copy())
    assert same(np.asarray(fixed, np.float32), want)


def test_drop_in_functions_on_the_float64_fixture():
    from descriptools_amd import downslope, flowhand, gfi, slope
    g = golden("nonfinite_f64")
    dem, px = g["dem"], float(g["px"])
    assert np.array_equal(np.asarray(slope.sloper(dem, px), np.float32), g["slope"])
    fd, idx, hand = flowhand.flow_hand_index(dem, g["fdr"], g["river"], px)
    assert np.array_equal(idx, g["idx"]) and np.array_equal(fd, g["fdist"])
    assert hand.dtype == np.float64 and same(hand, g["hand"])
    assert same(downslope.downsloper(dem, g["fdr"], px, 5), oracle.downslope_f64(dem, g["fdr"], px, 5.0))
    assert_float_close(gfi.gfi_calculator(g["hand"], g["fac"], g["idx"], 0.4, 0.1, px), g["gfi"], rtol=1e-5,
                       atol=1e-6, what="gfi")


def test_d8_nodata_mask_is_exactly_the_sentinel_test():
    """dt_dev_slope_d8_m: the mask bit is dem <= -100 and nothing else (not NaN, not +inf); the _m and the DEM-reading
    accumulation passes agree and equal the oracle"""
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    L = _lib.lib()
    ctx = Context()
    for H, W, nod, seed in ((130, 1024, 4, 1), (96, 1000, 3, 2), (80, 1001, 2, 3), (64, 64, 0, 4), (257, 515, 6, 5)):
        dem = seam_dem(seed, H, W, nod)
        d = ctx.to_device(dem)
        fdr = ctx.empty((H, W), np.uint8)
        nb = int(L.dt_nodata_mask_bytes(H, W))
        ldw = int(L.dt_nodata_mask_bytes(4, W)) // 2
        mask = ctx.empty((nb,), np.uint8)
        _lib.check(L.dt_dev_slope_d8_m(ctx.h, d.ptr, H, W, 10.0, fdr.ptr, mask.ptr))
        ctx.sync()
        m = mask.to_host().view(np.uint16).reshape((H + 3) // 4, ldw)
        bits = np.zeros((4 * m.shape[0], 4 * ldw), bool)
        for j in range(4):
            for k in range(4):
                bits[j::4, k::4] = (m >> (4 * j + k)) & 1
        assert np.array_equal(bits[:H, :W], dem <= -100), (H, W, int((bits[:H, :W] != (dem <= -100)).sum()))
        fdr_o = oracle.slope_d8(dem, 10.0)[1]
        got = fdr.to_host()
        assert np.array_equal(got, fdr_o), (H, W, int((got != fdr_o).sum()))
        outs = []
        for use_mask in (False, True):
            fac, river = ctx.empty((H, W), np.int32), ctx.empty((H, W), np.int8)
            if use_mask:
                _lib.check(L.dt_dev_flowacc_river_flowhand_local_m(ctx.h, fdr.ptr, d.ptr, mask.ptr, H, W, 50, fac.ptr,
                                                                   river.ptr))
            else:
                _lib.check(L.dt_dev_flowacc_river_flowhand_local(ctx.h, fdr.ptr, d.ptr, H, W, 50, fac.ptr, river.ptr))
            ctx.sync()
            outs.append((fac.to_host(), river.to_host()))
            fac.free()
            river.free()
        acc_o = oracle.flowacc(fdr_o, dem)
        for f, r in outs:
            assert np.array_equal(f, acc_o), (H, W, int((f != acc_o).sum()))
            assert np.array_equal(r, (acc_o > 50).astype(np.int8))
        for b in (d, fdr, mask):
            b.free()
    ctx.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_resident_chain_on_every_width_form(overlap):
    """W = 1024 (fused D8 + accumulation), 1000 (unfused), 1001 (odd: scalar staging): every output equals the oracle,
    so the cropped rasters agree with one another as well"""
    px, H = 10.0, 130
    base = seam_dem(7, H, 1024, 4, extra=((40, 999, NAN), (41, 1000, INF), (70, 1000, NAN), (90, 999, -INF)))
    for W in (1024, 1000, 1001):
        dem = np.ascontiguousarray(base[:, :W])
        thr = 40
        out = chain_once(dem, px, thr, overlap=overlap)
        check_chain(out, dem, px, thr, "W=%d overlap=%s" % (W, overlap))


def test_float64_chain_and_run_host():
    """Chain(heights="float64") on the float64 copy and run_host on both tiers: the float32 chain's rasters"""
    from descriptools_amd import chain
    px, H, W, thr = 10.0, 130, 1024, 40
    dem = seam_dem(9, H, W, 4)
    out = chain_once(dem, px, thr)
    ref = check_chain(out, dem, px, thr, "float32")
    out64 = chain_once(dem.astype(np.float64), px, thr, heights="float64")
    for k in ("slope", "fdr", "fac", "river", "fdist", "idx", "a_river", "down", "slope_rad", "ti", "mti", "gfi",
              "lnhlh"):
        assert same(out64[k], out[k]), "float64 chain " + k
    assert out64["hand"].dtype == np.float64 and same(out64["hand"].astype(np.float32), ref["hand"])
    for heights in ("float32", "float64"):
        h = chain.run_host(dem if heights == "float32" else dem.astype(np.float64), px, river_threshold=thr,
                           heights=heights)
        for k in ALL:
            assert same(np.asarray(h[k]).astype(np.asarray(out[k]).dtype), out[k]), "run_host %s %s" % (heights, k)


@pytest.mark.parametrize("long_walks", [True, "auto"])
def test_long_walks_with_special_values_on_the_walks(long_walks):
    """gentle east-falling rows (5 m over 1280 cells: walks of ~1300 moves, beyond the windowed kernel's reach) with
    NaN / +inf / -inf / -250 cells on and beside the walks: skip tables and the window kernel agree with the oracle"""
    px, H, W, thr = 10.0, 64, 2048, 10 ** 9
    xx = np.arange(W, dtype=np.float32)
    dem = np.tile(np.float32(600) - xx / np.float32(256), (H, 1))
    dem += (np.arange(H, dtype=np.float32) % 3)[:, None] / np.float32(256)
    rng = np.random.default_rng(3)
    for v in SPECIAL:
        for _ in range(12):
            dem[rng.integers(0, H), rng.integers(0, W)] = v
    dem[10, 300:310] = NAN
    dem[20, 700] = INF
    dem[30, 1500] = -INF
    dem[40, 900] = np.float32(-250)
    out = chain_once(dem, px, thr, long_walks=long_walks)
    plain = chain_once(dem, px, thr)
    ref = oracle_chain(dem, px, thr)
    assert np.array_equal(out["fdr"], ref["fdr"])
    assert same(out["down"], ref["down"]), int((~((out["down"] == ref["down"]) |
                                                  (np.isnan(out["down"]) & np.isnan(ref["down"])))).sum())
    assert same(plain["down"], ref["down"])
    assert (ref["down"] > 0).sum() > H * W // 2


def _rank_tiles(layout, dem, heights, marker):
    from descriptools_amd import tiling
    h = tiling.HALO
    pad = np.full((layout.Hg + 2 * h, layout.Wg + 2 * h), marker, np.float64)  # a finite height: must never be read
    pad[h:h + layout.Hg, h:h + layout.Wg] = dem
    thr = (layout.Hg * layout.Wg) // 512
    tiles = []
    for r in range(layout.size):
        t = tiling.RankTile(layout, r, device=0, px=10.0, river_threshold=thr, tune_placement=False, heights=heights)
        y0, x0 = layout.origin(r)
        t.set_dem_ext(np.ascontiguousarray(pad[y0:y0 + t.He, x0:x0 + t.We], np.float32 if heights == "float32"
                                           else np.float64))
        tiles.append(t)
    return tiles, thr


@pytest.mark.parametrize("heights", ["float32", "float64"])
def test_rank_tiles_2x2_with_special_values_on_rank_borders(heights):
    import torch
    from descriptools_amd import chain, tiling
    layout = tiling.Layout([192, 130], [256, 200])
    Hg, Wg, h = layout.Hg, layout.Wg, tiling.HALO
    extra = []
    for k, y in enumerate((191, 192, 191 - h + 1, 192 + h - 1, 0, Hg - 1)):
        for j, x in enumerate((255, 256, 255 - h + 1, 256 + h - 1, 100, 0, Wg - 1)):
            extra.append((y, x, SPECIAL[(k + j) % len(SPECIAL)]))
    for y in range(0, Hg, 9):
        extra += [(y, 255, SPECIAL[y % 5]), (y, 256 + (y % 3), SPECIAL[(y + 2) % 5])]
    for x in range(0, Wg, 11):
        extra += [(191, x, SPECIAL[x % 7]), (192 + (x % 2), x, SPECIAL[(x + 3) % 7])]
    dem = seam_dem(10, Hg, Wg, 3, extra=extra)
    dem_in = dem if heights == "float32" else dem.astype(np.float64)
    tiles, thr = _rank_tiles(layout, dem_in, heights, marker=31000.0)
    ref = chain.run_host(dem_in, 10.0, river_threshold=thr, heights=heights)
    check_chain(chain.run_host(dem, 10.0, river_threshold=thr), dem, 10.0, thr, "untiled")
    try:
        tiling.simulate_dev(tiles, layout)
        for t in tiles:
            assert t.unresolved_downslope() == 0
            y0, x0 = layout.origin(t.rank)
            sl = (slice(y0, y0 + t.H), slice(x0, x0 + t.W))
            for name in ("fdr", "fac", "river", "fdist", "idx", "hand", "slope", "ti", "mti", "gfi", "lnhlh", "down"):
                got, want = t.host(name), ref[name][sl]
                assert same(got, want.astype(got.dtype)), "rank %d %s" % (t.rank, name)
    finally:
        for t in tiles:
            t.free()
        torch.cuda.empty_cache()


def test_conditioning_with_below_sentinel_heights():
    """flowdir.d8_conditioned against oracle.condition_d8 with -250, -9999 and -inf cells inside the raster (heights to
    the fill, which raises them to their spill level).  On an outlet -- the raster border or next to -100 -- such a cell
    keeps its height, gets no code, and both refuse the raster.  NaN and +inf are out of scope for conditioning
    (the fill surface uses +inf as "not yet reached")."""
    from descriptools_amd import flowdir
    px = 10.0
    for H, W, seed in ((130, 1000, 1), (64, 64, 2), (97, 300, 3)):
        dem = oracle.synth_dem(seed, 2048, 2048, 50, 70, H, W, 3)
        nod = dem == -100
        outlet = np.ones_like(nod)
        inner = np.zeros_like(nod)
        inner[1:-1, 1:-1] = True
        near = nod.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near |= np.roll(np.roll(nod, dy, 0), dx, 1)
        outlet = ~inner | near
        rng = np.random.default_rng(seed)
        cand = np.argwhere(~outlet)
        for j, v in enumerate((-INF, np.float32(-250), np.float32(-9999)) * 15):
            y, x = cand[rng.integers(0, len(cand))]
            dem[y, x] = v
        fdr, filled = flowdir.d8_conditioned(dem, px, return_filled=True)
        fdr_o, filled_o = oracle.condition_d8(dem, px)
        assert same(filled, filled_o), int((filled != filled_o).sum())
        assert np.array_equal(fdr, fdr_o), int((fdr != fdr_o).sum())
        bad = dem.copy()
        bad[0, W // 2] = np.float32(-250)
        with pytest.raises(RuntimeError, match="could not be routed"):
            flowdir.d8_conditioned(bad, px)


def test_weighted_accumulation_with_unit_weights_is_the_count():
    from descriptools_amd import flowacc
    for H, W, seed in ((130, 1024, 11), (80, 1001, 12)):
        dem = seam_dem(seed, H, W, 3)
        fdr = oracle.slope_d8(dem, 10.0)[1]
        cnt = flowacc.accumulate(fdr, dem)
        assert np.array_equal(cnt, oracle.flowacc(fdr, dem))
        got = flowacc.accumulate_weighted(fdr, np.ones(fdr.shape), dem)
        assert np.array_equal(got, cnt.astype(np.float64))
