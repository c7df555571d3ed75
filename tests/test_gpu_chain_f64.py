"""The resident chain and D8 on float64 heights (Chain(heights="float64"), run_host / flowdir.d8 heights=): the
reference's fixture on a genuinely float64 DEM, the float64 oracle on larger rasters (W = 420: the unfused,
non-64-wide path; 1024 x 1024), and the float32 chain bit for bit on heights both tiers hold exactly."""
import numpy as np
import pytest

import oracle
from conftest import assert_float_close, golden, load_example

# scan order NW, N, NE, W, E, SW, S, SE and the ESRI codes (flowhand.py:801-824)
SCAN = ((-1, -1, 32), (-1, 0, 64), (-1, 1, 128), (0, -1, 16), (0, 1, 1), (1, -1, 8), (1, 0, 4), (1, 1, 2))


def d8_f64_np(dem, px):
    """The D8 definition restated in numpy, differences in float64: the first strict maximum of (z - z_nb) / d in scan
    order (aux starts at 0), neighbours outside the raster or equal to -100 skipped, nodata z <= -100 -> 0, and a
    border cell with no lower neighbour drains out (bottom row S, top row N, left column W, right column E)."""
    dem = np.asarray(dem, np.float64)
    H, W = dem.shape
    pad = np.full((H + 2, W + 2), -100.0)
    pad[1:-1, 1:-1] = dem
    aux = np.zeros((H, W))
    code = np.zeros((H, W), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy, dx, c in SCAN:
            nb = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            v = (dem - nb) / (px if dy == 0 or dx == 0 else px * np.sqrt(2.0))
            up = (nb != -100.0) & (aux < v)
            aux = np.where(up, v, aux)
            code = np.where(up, np.uint8(c), code)
    nod = dem <= -100.0
    free = (code == 0) & ~nod
    yy, xx = np.mgrid[0:H, 0:W]
    edge = np.zeros((H, W), np.uint8)  # the rule's priority: the last assignment wins
    edge[xx == W - 1] = 1
    edge[xx == 0] = 16
    edge[yy == 0] = 64
    edge[yy == H - 1] = 4
    code = np.where(free, edge, code)
    return np.where(nod, 0, code).astype(np.uint8)


def wide_dems(H, W):
    """the two DEMs of test_dem_dtype.test_wide_dems_against_the_float64_oracle: float64 heights with sub-float32
    structure and nodata, and int32 millimetres beyond 2^24 (with their dz)"""
    d32 = oracle.synth_dem(8, max(1024, 2 * H), max(1024, 2 * W), 100, 200, H, W, 3)
    yy, xx = np.mgrid[0:H, 0:W]
    d64 = np.where(d32 == -100, -100.0, d32.astype(np.float64) + 1e-3 * np.sin(0.3 * yy + 0.2 * xx) + 1e-7 * xx)
    mm = np.where(d32 == -100, -100, np.round(d32.astype(np.float64) * 1000.0) + 2 ** 25).astype(np.int32)
    assert (d64.astype(np.float32).astype(np.float64) != d64).any()
    assert (mm.astype(np.float32).astype(np.int64) != mm).any()
    return d64, mm


def chain_once(dem, px, heights, fdr=None, **kw):
    """one step of a Chain on one stream (no graph), outputs to the host; fdr given -> external_fdr"""
    from descriptools_amd import chain, device
    H, W = dem.shape
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=px, overlap=False, tune_placement=False, heights=heights,
                     external_fdr=fdr is not None, **kw)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float64 if heights == "float64" else np.float32))
    try:
        if fdr is not None:
            ch.buf["fdr"].copy_from(fdr)
        ch.run(d.ptr)
        ctx.sync()
        out = {k: ch.buf[k].to_host() for k, _ in ch.outputs}
    finally:
        d.free()
        ch.free()
        ctx.close()
    return out


@pytest.mark.gpu
def test_reference_fixture_through_the_float64_chain():
    """tests/golden/f64.npz (the reference's run on a float64 DEM) with its D8 raster: slope, downslope, flow
    distance, river index and HAND (float64) bit for bit; GFI / ln(hl/H) within the drop-in functions' tolerance"""
    g = golden("f64")
    dem, px = g["dem"], float(g["px"])
    out = chain_once(dem, px, "float64", fdr=g["fdr"], river_threshold=25, n_top=0.1, n_gfi=0.4, b=0.1, dz=5.0)
    assert np.array_equal(out["fac"], g["fac"]) and np.array_equal(out["river"], g["river"])
    assert np.array_equal(out["slope"], g["slope"])
    assert np.array_equal(out["down"], np.where(np.isnan(g["down"]), 0, g["down"]))
    assert np.array_equal(out["fdist"], g["fdist"]) and np.array_equal(out["idx"], g["idx"])
    assert out["hand"].dtype == np.float64 and np.array_equal(out["hand"], g["hand"])
    for k in ("gfi", "lnhlh"):
        assert np.array_equal(out[k] == -100, g[k] == -100), k
        assert np.allclose(out[k], g[k], rtol=1e-5, atol=1e-6), k


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(300, 420), (1024, 1024)])
@pytest.mark.parametrize("kind", ["float64", "int32_mm"])
def test_float64_chain_against_the_float64_oracle(shape, kind):
    from descriptools_amd import chain
    H, W = shape
    px, thr = 10.0, 40
    d64, mm = wide_dems(H, W)
    dem, dz, heights = (d64, 5.0, "float64") if kind == "float64" else (mm, 5000.0, "auto")
    dd = dem.astype(np.float64)
    out = chain.run_host(dem, px, heights=heights, river_threshold=thr, dz=dz)
    fdr = d8_f64_np(dd, px)
    assert np.array_equal(out["fdr"], fdr), "%d codes differ" % int((out["fdr"] != fdr).sum())
    assert np.array_equal(out["slope"], oracle.slope_f64(dd, px))
    fac = oracle.flowacc(fdr, np.where(dd <= -100, -100, 0).astype(np.float32))
    assert np.array_equal(out["fac"], fac)
    river = (fac > thr).astype(np.int8)
    assert np.array_equal(out["river"], river)
    idx, nc, nd = oracle.flowhand_fast(fdr, river)
    assert np.array_equal(out["idx"], idx)
    ok = idx != -100
    assert np.array_equal(out["fdist"], np.where(ok, px * nc + (px * np.sqrt(2.0)) * nd, -100.0).astype(np.float32))
    hand = oracle.hand_f64(dd, idx)
    assert out["hand"].dtype == np.float64 and np.array_equal(out["hand"], hand)
    assert np.array_equal(out["down"], oracle.downslope_f64(dd, fdr, px, dz))
    slr = np.where(dd == -100, -100, np.arctan(out["slope"] / 100)).astype(np.float32)
    assert np.max(np.abs(out["slope_rad"].astype(np.float64) - slr)) <= 2.4e-7
    ti, mti = oracle.twi(fac, out["slope_rad"], px, 0.1)
    assert_float_close(out["ti"], ti, rtol=1e-5, what="ti")
    assert_float_close(out["mti"], mti, rtol=1e-5, atol=1e-6, what="mti")
    assert_float_close(out["gfi"], oracle.gfi_f64h(hand, fac, idx, 0.4, 0.1, px), rtol=1e-5, atol=1e-6, what="gfi")
    assert_float_close(out["lnhlh"], oracle.lnhlh_f64h(hand, fac, 0.4, 0.1, px), rtol=1e-5, atol=1e-6, what="lnhlh")


SAME = ("slope", "fdr", "fac", "river", "fdist", "idx", "down", "slope_rad", "ti", "mti")


def _same_as_float32(a, b, keys=SAME):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s: %d cells differ" % (k, int((a[k] != b[k]).sum()))
    assert a["hand"].dtype == np.float64 and np.array_equal(a["hand"], b["hand"].astype(np.float64))
    for k in ("gfi", "lnhlh"):
        assert_float_close(a[k], b[k], rtol=1e-5, atol=1e-6, what=k)


@pytest.mark.gpu
def test_integer_heights_agree_with_the_float32_chain_at_4096():
    """integer heights below 2^24: float32 and float64 differences are the same numbers, so the two tiers must agree
    bit for bit (HAND after the cast; GFI / ln(hl/H) are evaluated from a float64 HAND: within 1e-5)"""
    from descriptools_amd import chain
    dem = np.round(oracle.synth_dem(1, 4096, 4096, 0, 0, 4096, 4096, 2))  # nodata stays -100
    assert (dem == -100).any()
    _same_as_float32(chain.run_host(dem, 10.0, heights="float64"), chain.run_host(dem, 10.0))


@pytest.mark.gpu
def test_example_through_the_float64_chain():
    """the bundled Example with its GIS D8 raster: the float64 chain equals the float32 one; and the float64 HAND pass
    (dt_dev_hand_gfi_f64) on the Example's own river index (its GIS accumulation > 128000, which the chain's
    accumulation from the codes does not reproduce) gives Example/output/hand_class.tif (the reference's known answer)"""
    from descriptools_amd import _lib, device, evaluation, flowhand
    dem, fdr, fac, river, flood, klass = load_example()
    kw = dict(river_threshold=128000, long_walks=False)
    a = chain_once(dem, 12.5, "float64", fdr=fdr, **kw)
    b = chain_once(dem, 12.5, "float32", fdr=fdr, **kw)
    _same_as_float32(a, b, [k for k in SAME if k != "fdr"])
    _, idx, _ = flowhand.flow_hand_index(dem, fdr, river, 12.5)
    H, W = dem.shape
    ctx = device.Context()
    bufs = [ctx.to_device(dem.astype(np.float64)), ctx.to_device(idx.astype(np.int32)),
            ctx.to_device(np.clip(fac, -100, 2 ** 31 - 1).astype(np.int32)), ctx.empty((H, W), np.float64)]
    try:
        _lib.check(_lib.lib().dt_dev_hand_gfi_f64(ctx.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, H, W, 12.5, 0.4, 0.1,
                                                  bufs[3].ptr, None, None))
        hand = bufs[3].to_host()
    finally:
        for x in bufs:
            x.free()
        ctx.close()
    assert hand.dtype == np.float64
    el = np.unique(hand)
    mn, mx = el[1], el[-1]
    assert (mn, mx) == (0, 259)
    desc = evaluation.minMaxScale(hand, mn, mx, -100)
    th = evaluation.calibration(desc, flood, 'under')
    assert th == 0.012
    c, f, cm = evaluation.avaliacao(evaluation.binary_map(desc, th, 'under'), flood)
    assert int((cm.astype(np.uint8) != klass).sum()) == 0


@pytest.mark.gpu
def test_flowdir_d8_float64():
    from descriptools_amd import flowdir
    g = golden("f64")
    d64, mm = wide_dems(300, 420)
    for dem, px in ((g["dem"], float(g["px"])), (d64, 10.0), (mm.astype(np.float64), 10.0)):
        fdr, sl = flowdir.d8(dem, px, return_slope=True, heights="float64")
        assert np.array_equal(fdr, d8_f64_np(dem, px))
        assert np.array_equal(sl, oracle.slope_f64(dem, px))
    assert np.array_equal(flowdir.d8(mm, 10.0, heights="auto"), d8_f64_np(mm, 10.0))
    # float32 values: "auto" takes the float32 kernels, which give the same codes
    d32 = oracle.synth_dem(3, 256, 256, 0, 0, 200, 260, 2)
    assert np.array_equal(flowdir.d8(d32.astype(np.float64), 10.0, heights="auto"), oracle.slope_d8(d32, 10.0)[1])
    assert np.array_equal(flowdir.d8(d32, 10.0, heights="float64"), oracle.slope_d8(d32, 10.0)[1])


@pytest.mark.gpu
def test_float64_chain_ties_in_scan_order():
    """exact ties between neighbours (equal differences, and a cardinal / diagonal pair whose float64 quotients are
    equal) take the first neighbour in scan order, as the literal loop does"""
    from descriptools_amd import flowdir
    rng = np.random.default_rng(7)
    dem = np.round(rng.random((67, 131)) * 4.0) * 0.25 + 1000.0  # many equal differences
    dem[5:9, 5:9] = -100.0
    dem[20, 30] = np.nan
    fdr, sl = flowdir.d8(dem, 1.0, return_slope=True, heights="float64")
    assert np.array_equal(fdr, d8_f64_np(dem, 1.0))
    assert np.array_equal(sl, oracle.slope_f64(dem, 1.0))
