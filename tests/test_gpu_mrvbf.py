"""GPU (-m gpu): descriptools_amd.mrvbf against the numpy reference of tests/_mrvbf_ref.py.

Shapes.  Smaller than a window and a block: (1, 1), (1, 70), (70, 1), (3, 3), (13, 14); every residue of the width and
the height modulo 3 and 9: (67, 131), (130, 200), (243, 300); and the kernels' own tile sizes with one cell less and one
more on both axes: k_percentile and k_mrvbf work on tiles of 64 x 16 cells (MV_TX, MV_TY; a lane takes 4 rows of a
column, MV_RB) -> (15, 63), (16, 64), (17, 65); k_coarsen on tiles of 16 x 8 coarse = 48 x 24 fine cells (CO_CX, CO_CY)
-> (23, 47), (24, 48), (25, 49).  (243, 300) is 11 x 7 of the latter and 16 x 5 of the former.  Rasters of 64 cells or
more carry nodata blobs (-100 and -9999) and a NaN, a +inf, a -inf and a -150 cell.

elevation_percentile and coarsen have no transcendental function on the device: bit for bit.

indices takes one pow per level and output with a non-integer exponent, and the GPU's pow is not the reference's.  The
measure of what that may cost is the reference's own sensitivity to pow: with pow(q, p) replaced by exp(p log q), on the
(130, 200) and the (67, 131) terrain of this file at px = 30 with 10 levels, both outputs, 0 of 23,904 and 0 of 8,145
valid cells move and no NaN appears (tests/test_mrvbf_host.py::test_pow_as_exp_log_moves_no_cell asserts it).  The
bound is that worst movement plus one float32 spacing, because the GPU's pow is a third implementation: every value
within ONE float32 spacing of the reference, and the -100 positions identical.  The test prints how many cells differ at all
before it asserts."""
import numpy as np
import pytest

import _focal_ref
import _mrvbf_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (3, 3), (13, 14), (67, 131), (130, 200), (243, 300),
          (15, 63), (16, 64), (17, 65), (23, 47), (24, 48), (25, 49)]
PX = 30.0
BOUND = 1  # float32 spacings
_sid = lambda s: "%dx%d" % s
_DEMS, _COUNTS, _INDICES = {}, {}, {}


def _dem(shape):
    if shape not in _DEMS:
        d = R.terrain(shape[0], shape[1], seed=shape[0] * 7 + shape[1], holes=shape[0] * shape[1] >= 64)
        d.setflags(write=False)
        _DEMS[shape] = d
    return _DEMS[shape]


def _reference_indices(shape, levels):
    key = (shape, levels)
    if key not in _INDICES:
        r = R.indices(_dem(shape), PX, ("mrvbf", "mrrtf"), levels=levels)
        for a in r.values():
            a.setflags(write=False)
        _INDICES[key] = r
    return _INDICES[key]


def _assert_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    assert not np.isnan(got).any(), what
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), "%s: %d cells differ, first at %s: %r, reference %r" % (
        what, int(diff.sum()), tuple(np.argwhere(diff)[0]), got[diff][0], want[diff][0])


def _spacings(got, want):
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("radius", [1, 3, 6, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_elevation_percentile_equals_the_reference_bit_for_bit(shape, radius):
    from descriptools_amd import mrvbf
    dem = _dem(shape)
    if (shape, radius) not in _COUNTS:
        _COUNTS[shape, radius] = R.percentile64(dem, radius)
    ok, lo, hi = _COUNTS[shape, radius]
    for kind, p in (("lower", lo), ("higher", hi)):
        want = np.where(ok, p.astype(np.float32), np.float32(-100))
        if shape[0] * shape[1] >= 64:
            assert (want == -100).any() and len(np.unique(want)) > 4
        _assert_bits(mrvbf.elevation_percentile(dem, radius, kind), want, "%s at radius %d" % (kind, radius))


@pytest.mark.parametrize("px", [30.0, 7.3])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_coarsen_equals_the_reference_bit_for_bit(shape, px):
    from descriptools_amd import mrvbf
    dem = _dem(shape)
    dem3, slope3 = mrvbf.coarsen(dem, px)
    want3, wslope3 = R.coarsen(dem, px)
    assert dem3.shape == (-(-shape[0] // 3), -(-shape[1] // 3))
    _assert_bits(dem3, want3, "dem3")
    _assert_bits(slope3, wslope3, "slope3")


@pytest.mark.parametrize("shape", [(67, 131), (243, 300), (25, 49)], ids=_sid)
def test_coarsen_twice_equals_the_reference_twice(shape):
    from descriptools_amd import mrvbf
    dem = _dem(shape)
    a, _ = mrvbf.coarsen(dem, 7.3)
    b, sb = mrvbf.coarsen(a, 7.3 * 3.0)
    ra, _ = R.coarsen(dem, 7.3)
    rb, rsb = R.coarsen(ra, 7.3 * 3.0)
    if shape[0] * shape[1] >= 64 * 81:
        assert (ra == -100).any()  # a block of nine nodata cells: the second step meets -100
    _assert_bits(b, rb, "dem9")
    _assert_bits(sb, rsb, "slope9")


@pytest.mark.parametrize("levels", [None, 2, 10])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_indices_within_the_bound_of_the_reference(shape, levels):
    from descriptools_amd import mrvbf
    dem = _dem(shape)
    want = _reference_indices(shape, levels)
    got = mrvbf.indices(dem, PX, ("mrvbf", "mrrtf"), levels=levels)
    assert list(got) == ["mrvbf", "mrrtf"]
    ok = R.valid(dem)
    for n in ("mrvbf", "mrrtf"):
        assert got[n].dtype == np.float32 and not np.isnan(got[n]).any()
        assert np.array_equal(got[n] == -100, ~ok) and np.array_equal(want[n] == -100, ~ok), n
        d = _spacings(got[n], want[n])
        print("%s levels=%s %s: %d of %d valid cells differ, by at most %d float32 spacings"
              % (_sid(shape), levels, n, int((d != 0).sum()), int(ok.sum()), int(d.max())))
        assert d.max() <= BOUND, "%s: %d cells beyond the bound, the worst by %d spacings at %s: %r, reference %r" % (
            n, int((d > BOUND).sum()), int(d.max()), tuple(np.argwhere(d == d.max())[0]),
            got[n][d == d.max()][0], want[n][d == d.max()][0])


@pytest.mark.parametrize("shape", [(130, 200), (67, 131)], ids=_sid)
def test_the_reference_spreads_over_the_classes(shape):
    """otherwise the comparison above shows little: at least 2 % of the valid cells in each class, both outputs"""
    want = _reference_indices(shape, None)
    ok = R.valid(_dem(shape))
    for n in ("mrvbf", "mrrtf"):
        v = want[n][ok]
        for lo, hi in ((0, 0.5), (0.5, 1.5), (1.5, 2.5), (2.5, np.inf)):
            share = float(((v >= lo) & (v < hi)).mean())
            assert share >= 0.02, (n, lo, hi, share)


# ---- exact identities on the GPU alone -------------------------------------------------------------------------------
def _integer_dem(shape, seed):
    d = np.rint(_focal_ref.terrain(shape[0], shape[1], seed, lo=0.0, hi=40.0))
    return np.where(_focal_ref.valid(d), d, np.float32(-100)).astype(np.float32)


@pytest.mark.parametrize("levels", [None, 10])
def test_mrvbf_of_the_negated_dem_is_mrrtf(levels):
    from descriptools_amd import mrvbf
    d = _focal_ref.terrain(130, 200, 3, lo=-50.0, hi=50.0)
    dem = np.where(_focal_ref.valid(d), d, np.float32("nan")).astype(np.float32)  # NaN: not valid under either sign
    assert (dem < 0).any() and (dem > 0).any() and np.isnan(dem).any()
    a = mrvbf.mrvbf(-dem, PX, levels=levels, pctl_valley=0.37)
    b = mrvbf.mrrtf(dem, PX, levels=levels, pctl_ridge=0.37)
    assert len(np.unique(b)) > 1000
    _assert_bits(a, b, "mrvbf(-dem) against mrrtf(dem)")


def test_level_two_ignores_an_offset_and_follows_a_flip():
    from descriptools_amd import mrvbf
    dem = _integer_dem((67, 131), 4)
    ok = dem != -100
    base = mrvbf.indices(dem, PX, ("mrvbf", "mrrtf"), levels=2)
    up = mrvbf.indices(np.where(ok, dem + 64, dem).astype(np.float32), PX, ("mrvbf", "mrrtf"), levels=2)
    flip = mrvbf.indices(np.ascontiguousarray(dem[:, ::-1]), PX, ("mrvbf", "mrrtf"), levels=2)
    for n in base:
        assert len(np.unique(base[n])) > 100
        _assert_bits(up[n], base[n], n + " of dem + 64")
        _assert_bits(np.ascontiguousarray(flip[n][:, ::-1]), base[n], n + " of the flipped dem")


def test_outputs_come_in_the_order_asked_for_with_the_bits_of_separate_calls():
    from descriptools_amd import mrvbf
    dem = _dem((130, 200))
    both = mrvbf.indices(dem, PX, ("mrrtf", "mrvbf"))
    assert list(both) == ["mrrtf", "mrvbf"]
    _assert_bits(both["mrvbf"], mrvbf.mrvbf(dem, PX), "mrvbf")
    _assert_bits(both["mrrtf"], mrvbf.mrrtf(dem, PX), "mrrtf")
    assert list(mrvbf.indices(dem, PX)) == ["mrvbf"]


def test_a_raster_without_a_valid_cell_and_an_empty_one():
    from descriptools_amd import mrvbf
    dem = np.full((40, 70), -100, np.float32)
    dem[3, 4], dem[5, 6], dem[7, 8], dem[9, 9] = np.nan, np.inf, -np.inf, -9999
    for levels in (None, 2, 10):
        r = mrvbf.indices(dem, PX, ("mrvbf", "mrrtf"), levels=levels)
        assert (r["mrvbf"] == -100).all() and (r["mrrtf"] == -100).all()
    assert (mrvbf.elevation_percentile(dem, 6) == -100).all()
    z3, s3 = mrvbf.coarsen(dem, PX)
    assert (z3 == -100).all() and (s3 == -100).all()
    e = mrvbf.indices(np.zeros((0, 5), np.float32), PX, ("mrrtf", "mrvbf"))
    assert list(e) == ["mrrtf", "mrvbf"] and e["mrvbf"].shape == (0, 5)
    assert mrvbf.coarsen(np.zeros((0, 5), np.float32), PX)[0].shape == (0, 2)


# ---- the device tier -------------------------------------------------------------------------------------------------
def test_device_tier_on_torch_tensors_equals_the_host_tier_and_reuses_its_scratch():
    """dt_dev_mrvbf, dt_dev_percentile and dt_dev_coarsen on torch tensors, on a context bound to a torch stream: the
    host tier's bytes.  dt_dev_mrvbf runs twice on the context with a larger raster's call in between, so the second
    run builds its pyramid in scratch that holds another pyramid's rasters."""
    import ctypes as C
    import torch
    from descriptools_amd import _lib, mrvbf
    from descriptools_amd.device import Context
    L = _lib.lib()
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    dem, big = _dem((130, 200)), _dem((243, 300))
    H, W = dem.shape
    levels = 6
    p = (C.c_double * (levels - 1))(*mrvbf._exponents(levels))
    g = (C.c_double * 6)(*mrvbf._gauss_weights())
    t = mrvbf.slope_threshold(PX)
    host = mrvbf.indices(dem, PX, ("mrvbf", "mrrtf"), levels=levels)
    try:
        with torch.cuda.stream(st):
            d, db = torch.from_numpy(dem.copy()).to("cuda"), torch.from_numpy(big.copy()).to("cuda")
            out = torch.full((4, H, W), 7.0, dtype=torch.float32, device="cuda")
            outb = torch.empty(big.shape, dtype=torch.float32, device="cuda")

            def run(v, r):
                _lib.check(L.dt_dev_mrvbf(ctx.h, d.data_ptr(), H, W, PX, t, levels, 0.4, 0.35, p,
                                          out[v].data_ptr() if v is not None else None,
                                          out[r].data_ptr() if r is not None else None))
            run(0, 1)
            assert L.dt_ctx_scratch_bytes(ctx.h) >= 16 * (44 * 67 + 15 * 23 + 5 * 8 + 2 * 3)
            _lib.check(L.dt_dev_mrvbf(ctx.h, db.data_ptr(), big.shape[0], big.shape[1], PX, t, 10, 0.4, 0.35,
                                      (C.c_double * 9)(*mrvbf._exponents(10)), outb.data_ptr(), None))
            run(2, None)
            run(None, 3)
            ctx.sync()
            assert ctx.status() == 0
            got = out.cpu().numpy()
            _assert_bits(got[0], host["mrvbf"], "device tier, first run, mrvbf")
            _assert_bits(got[1], host["mrrtf"], "device tier, first run, mrrtf")
            _assert_bits(got[2], host["mrvbf"], "device tier, second run, mrvbf alone")
            _assert_bits(got[3], host["mrrtf"], "device tier, second run, mrrtf alone")
            _assert_bits(outb.cpu().numpy(), mrvbf.mrvbf(big, PX, levels=10), "the larger raster in between")
            lo = torch.empty((H, W), dtype=torch.float32, device="cuda")
            _lib.check(L.dt_dev_percentile(ctx.h, d.data_ptr(), H, W, 6, lo.data_ptr(), None))
            Hc, Wc = -(-H // 3), -(-W // 3)
            z3 = torch.empty((2, Hc, Wc), dtype=torch.float32, device="cuda")
            _lib.check(L.dt_dev_coarsen(ctx.h, d.data_ptr(), H, W, PX, g, z3[0].data_ptr(), z3[1].data_ptr()))
            ctx.sync()
            _assert_bits(lo.cpu().numpy(), mrvbf.elevation_percentile(dem, 6), "dt_dev_percentile")
            hz3, hs3 = mrvbf.coarsen(dem, PX)
            _assert_bits(z3[0].cpu().numpy(), hz3, "dt_dev_coarsen dem3")
            _assert_bits(z3[1].cpu().numpy(), hs3, "dt_dev_coarsen slope3")
            # refusals: every one before a launch
            dp, op = d.data_ptr(), out[0].data_ptr()
            for args, msg in (((dp, H, W, PX, t, 1, 0.4, 0.35, p, op, None), b"levels"),
                              ((dp, H, W, PX, t, 11, 0.4, 0.35, p, op, None), b"levels"),
                              ((dp, H, W, 0.0, t, levels, 0.4, 0.35, p, op, None), b"px"),
                              ((dp, H, W, PX, 0.0, levels, 0.4, 0.35, p, op, None), b"slope_threshold"),
                              ((dp, H, W, PX, t, levels, 0.0, 0.35, p, op, None), b"pctl"),
                              ((dp, H, W, PX, t, levels, 0.4, 1.5, p, op, None), b"pctl"),
                              ((dp, H, W, PX, t, levels, 0.4, 0.35, None, op, None), b"exponent"),
                              ((dp, H, W, PX, t, levels, 0.4, 0.35, p, None, None), b"no output raster"),
                              ((None, H, W, PX, t, levels, 0.4, 0.35, p, op, None), b"NULL raster")):
                assert L.dt_dev_mrvbf(ctx.h, *args) == -1, msg
                assert msg in L.dt_last_error(), (msg, L.dt_last_error())
            assert L.dt_dev_percentile(ctx.h, dp, H, W, 17, op, None) == -1 and b"[1, 16]" in L.dt_last_error()
            assert L.dt_dev_percentile(ctx.h, dp, H, W, 3, None, None) == -1
            assert L.dt_dev_coarsen(ctx.h, dp, H, W, PX, None, op, op) == -1 and b"Gaussian" in L.dt_last_error()
            assert L.dt_dev_mrvbf(ctx.h, dp, 0, W, PX, t, levels, 0.4, 0.35, p, op, None) == 0
            ctx.sync()
            assert ctx.status() == 0
    finally:
        ctx.close()
        torch.cuda.empty_cache()
