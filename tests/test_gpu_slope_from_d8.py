"""The float32 chain without a slope + TI + MTI pass: slope out of the D8 kernel (k_d8_slope), TI / MTI out of flow
accumulation's last tile pass (k_fa3fh1_twi), the exact recomputation of the marked cells (k_slope_twi_fix) -- against the
three calls the step made before (dt_dev_slope_d8_m, dt_dev_flowacc_river_flowhand_local_m, dt_dev_slope_twi), every
raster bit for bit (floats compared as int32, so that NaN payloads count).

The DEMs are chosen so that every class of cell the fast paths reject occurs: a slope on a float32 rounding boundary,
|TI| < 0.25, tan(slope) > 2.5, and a rough field where a large share of the cells is marked.  That they do produce those
classes is checked on the CPU with the oracle (test_dems_produce_the_rejected_classes, no GPU needed); on the GPU the
marks must contain those cells, so the fix path cannot be dead without anyone noticing."""
import numpy as np
import pytest

import oracle
from conftest import golden, load_example

gpu = pytest.mark.gpu
RASTERS = ("fdr", "fac", "river", "slope", "ti", "mti")
N_TOP = 0.1


# ---- the DEMs ------------------------------------------------------------------------------------------------------
def dem_boundary():
    """px 10: cells whose only drop is 1 + 2^-22 to a cardinal neighbour.  slope = 10 (1 + 2^-22) = 10 + 5 2^-21, an odd
    multiple of 2^-21: exactly half way between two float32 values of [8, 16) (ulp 2^-20)."""
    rng = np.random.default_rng(3)
    dem = (100.0 + rng.integers(0, 4, size=(128, 256))).astype(np.float32)
    cells = [(8, 8), (40, 200), (77, 131), (127, 64)]
    # the centre must stand 1 + 2^-22 above its west neighbour and below everything else
    for y, x in cells:
        dem[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 50.0
        dem[y, x - 1] = 0.0
        dem[y, x] = np.float32(1.0 + 2.0 ** -22)
    return dem, 10.0, cells


def dem_small_ti():
    """px 1: a plane falling 1 per cell to the south with a little noise -- slope 100 %, accumulation 0, 1, 2 ... down
    each column: TI = ln(max(fac, 1)) - ln tan(pi / 4 + 0.01) is -0.02 on the two top rows"""
    rng = np.random.default_rng(5)
    H, W = 192, 320
    dem = (np.arange(H, 0, -1, dtype=np.float32)[:, None] + np.zeros((1, W), np.float32))
    dem[:, ::7] += (rng.integers(0, 3, size=(H, len(range(0, W, 7)))) * 0.125).astype(np.float32)
    return dem, 1.0


def dem_rough(H=256, W=512, seed=11):
    """px 10, heights uniform in [0, 40) m with 40 m pits and a nodata block: slopes beyond 250 % on a large share"""
    rng = np.random.default_rng(seed)
    dem = (rng.random((H, W)) * 40.0).astype(np.float32)
    dem[rng.random((H, W)) < 0.05] -= 40.0
    dem[dem <= -100.0] = -99.0
    dem[60:90, 100:180] = -100.0
    return dem, 10.0


def dem_nonfinite(name, pad):
    """tests/golden/nonfinite*.npz (NaN, +-inf and below-sentinel heights), as it is (80 x 100: the stencil's path) or
    set into a 128 x 128 field (the new kernels' path)"""
    g = golden(name)
    with np.errstate(over="ignore"):
        dem = g["dem"].astype(np.float32)
    if pad:
        dem = np.pad(dem, ((24, 24), (14, 14)), mode="reflect")
    return dem, float(g["px"])


def dem_example(crop):
    dem = load_example()[0].astype(np.float32)
    if crop:
        dem = np.ascontiguousarray(dem[:, :dem.shape[1] // 64 * 64])
    return dem, 10.0


# ---- the classes on the CPU -----------------------------------------------------------------------------------------
def cpu_classes(dem, px):
    """(near_mid, small_ti, steep): the cells of each rejected class, from the oracle's slope / accumulation / TI and the
    float64 product form of the slope (max of the class maxima times 100 / px, 100 / (px sqrt 2)); nodata excluded"""
    dem = np.ascontiguousarray(dem, np.float32)
    H, W = dem.shape
    slope, fdr = oracle.slope_d8(dem, px)
    fac = oracle.flowacc(fdr, dem)
    with np.errstate(all="ignore"):
        srad = np.arctan(slope / np.float32(100.0)).astype(np.float32)
        ti, mti = oracle.twi(fac, srad, px, N_TOP)
        z = np.where(dem == -100.0, np.nan, dem).astype(np.float32)
        p = np.pad(z, 1, constant_values=np.nan)
        c = p[1:-1, 1:-1]
        cb = np.zeros((H, W), np.float32)
        db = np.zeros((H, W), np.float32)
        for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
            cb = np.fmax(cb, c - p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        for dy, dx in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
            db = np.fmax(db, c - p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        q = np.fmax(cb.astype(np.float64) * (100.0 / px), db.astype(np.float64) * (100.0 / (px * np.sqrt(2.0))))
    ok = (dem > -100.0) & np.isfinite(q)
    lo = q.view(np.uint64) & np.uint64(0x1FFFFFFF)
    near_mid = ok & (lo == np.uint64(0x10000000)) & (q > 0)
    live = ok & (fac > -100)
    small_ti = live & (np.abs(ti) < 0.2) & (slope <= 200.0)
    steep = live & (slope > 260.0) & np.isfinite(slope)
    return near_mid, small_ti, steep


def test_dems_produce_the_rejected_classes():
    dem, px, cells = dem_boundary()
    near_mid = cpu_classes(dem, px)[0]
    assert all(near_mid[y, x] for y, x in cells)
    dem, px = dem_small_ti()
    small = cpu_classes(dem, px)[1]
    assert small[:2, 3::7].all() and not small[100].any()  # (columns away from the noise)
    dem, px = dem_rough()
    steep = cpu_classes(dem, px)[2]
    assert steep.mean() > 0.10


# ---- the two forms of the step on the GPU ---------------------------------------------------------------------------
def three_calls(dem, px, thr):
    """the step's calls before this change, on one context"""
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    L, (H, W) = _lib.lib(), dem.shape
    ctx = Context()
    try:
        d = ctx.to_device(np.ascontiguousarray(dem, np.float32))
        b = {k: ctx.empty((H, W), dt) for k, dt in (("fdr", np.uint8), ("fac", np.int32), ("river", np.int8),
                                                     ("slope", np.float32), ("ti", np.float32), ("mti", np.float32))}
        m4 = ctx.empty((int(L.dt_nodata_mask_bytes(H, W)),), np.uint8)
        _lib.check(L.dt_dev_slope_d8_m(ctx.h, d.ptr, H, W, px, b["fdr"].ptr, m4.ptr))
        _lib.check(L.dt_dev_flowacc_river_flowhand_local_m(ctx.h, b["fdr"].ptr, d.ptr, m4.ptr, H, W, thr, b["fac"].ptr,
                                                           b["river"].ptr))
        _lib.check(L.dt_dev_slope_twi(ctx.h, d.ptr, b["fac"].ptr, H, W, px, N_TOP, b["slope"].ptr, None, b["ti"].ptr,
                                      b["mti"].ptr))
        ctx.sync()
        out = {k: v.to_host() for k, v in b.items()}
        for v in list(b.values()) + [d, m4]:
            v.free()
    finally:
        ctx.close()
    return out


def marked_cells(raw, H, W):
    """the marks workspace as a boolean raster: a byte per 256 x 16 tile, then 16 bits per lane of every tile
    (bit 4 j + k = cell (j, k) of the lane's 4 x 4 patch; every lane's word is written on this path)"""
    tx, ty = (W + 255) // 256, (H + 15) // 16
    nt = tx * ty
    off = (nt + 255) // 256 * 256
    tile_mark = raw[:nt].reshape(ty, tx)
    lanes = raw[off:off + nt * 512].view(np.uint16).reshape(ty, tx, 4, 64)
    y, x = np.mgrid[0:H, 0:W]
    w16 = lanes[y >> 4, x >> 8, (y & 15) >> 2, (x & 255) >> 2]
    m = ((w16 >> (4 * (y & 3) + (x & 3)).astype(np.uint16)) & 1).astype(bool)
    assert not (m & ~tile_mark[y >> 4, x >> 8].astype(bool)).any(), "a marked cell in a tile that is not marked"
    return m


def chain_step(dem, px, thr, overlap):
    """the chain's step as Chain.run enqueues it; also whether it took the new calls, and the marked cells"""
    from descriptools_amd import chain
    from descriptools_amd.device import Context
    H, W = dem.shape
    ctx = Context()
    try:
        d = ctx.to_device(np.ascontiguousarray(dem, np.float32))
        ch = chain.Chain(H, W, ctx=ctx, px=px, n_top=N_TOP, river_threshold=thr, want_slope_rad=False,
                         tune_placement=False, overlap=overlap)
        new = ch._from_d8()
        ch.run(d.ptr, want_a_river=False)
        ctx.sync()
        ch.check_status()
        out = {k: ch.buf[k].to_host() for k in RASTERS}
        marks = marked_cells(ch._marks.to_host(), H, W) if new else None
        assert [n for n, _, _ in ch.ops(d.ptr)] == [o[0] for o in chain.OPS]
        ch.free()
        d.free()
    finally:
        ctx.close()
    return out, new, marks


def same_bits(a, b):
    if a.dtype == np.float32:
        a, b = a.view(np.int32), b.view(np.int32)
    return np.array_equal(a, b)


def check(dem, px, expect_new, must_mark=None, overlap=True):
    H, W = dem.shape
    thr = max(H * W // 512, 8)
    ref = three_calls(dem, px, thr)
    got, new, marks = chain_step(dem, px, thr, overlap)
    assert new == expect_new
    for k in RASTERS:
        assert same_bits(got[k], ref[k]), (k, int((got[k].view(np.int32) != ref[k].view(np.int32)).sum())
                                           if got[k].dtype.itemsize == 4 else k)
    if new:
        assert marks.any(), "nothing marked: the fix path would be dead"
        if must_mark is not None:
            assert must_mark.any() and marks[must_mark].all(), int((must_mark & ~marks).sum())
    return marks


@gpu
@pytest.mark.parametrize("nodata_pct", [0, 2])
def test_synthetic_1024(nodata_pct):
    dem = oracle.synth_dem(21 + nodata_pct, 4096, 4096, 512, 1024, 1024, 1024, nodata_pct)
    dem = dem.copy()  # two cells at 1000 m: slopes beyond 250 % around them, so that smooth terrain has marked cells too
    dem[500, 500], dem[500, 499] = np.float32(1000.0), np.float32(1000.0) - np.float32(1.0 + 2.0 ** -22)
    check(dem, 10.0, True)


@gpu
@pytest.mark.parametrize("shape,expect_new", [((1000, 832), True), ((500, 700), False), ((70, 64), True)])
def test_ragged_shapes(shape, expect_new):
    """rows that are no multiple of 16 or 64, columns that are no multiple of 256 (ragged stencil tiles); a width that is
    no multiple of 64 keeps the stencil pass"""
    H, W = shape
    dem, px = dem_rough(H, W, seed=H)
    check(dem, px, expect_new)


@gpu
@pytest.mark.parametrize("overlap", [True, False])
def test_slope_on_a_rounding_boundary(overlap):
    dem, px, cells = dem_boundary()
    near_mid = cpu_classes(dem, px)[0]
    assert all(near_mid[y, x] for y, x in cells)
    check(dem, px, True, must_mark=near_mid, overlap=overlap)


@gpu
def test_ti_near_zero():
    dem, px = dem_small_ti()
    small = cpu_classes(dem, px)[1]
    assert small[:2, 3::7].all()
    check(dem, px, True, must_mark=small)


@gpu
def test_rough_dem_marks_a_large_share():
    dem, px = dem_rough()
    steep = cpu_classes(dem, px)[2]
    assert steep.mean() > 0.10
    marks = check(dem, px, True, must_mark=steep)
    assert marks.mean() > 0.10


@gpu
@pytest.mark.parametrize("crop", [True, False])
def test_bundled_example(crop):
    dem, px = dem_example(crop)
    check(dem, px, crop)


@gpu
@pytest.mark.parametrize("name", ["nonfinite", "nonfinite_f64"])
@pytest.mark.parametrize("pad", [True, False])
def test_nonfinite_heights(name, pad):
    dem, px = dem_nonfinite(name, pad)
    check(dem, px, pad)
