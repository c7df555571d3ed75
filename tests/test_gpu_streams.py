"""GPU (-m gpu): stream order (streams.stream_network, dt_stream_order, dt_dev_stream_order; k_so_* in
dt_streams.hip) against the pure-numpy in-degree-peeling reference (tests/_streams_ref.py), cell for cell, for
Strahler, Shreve and link: hand-built networks, a comb with thousands of junctions on one serial chain, a serpentine
link across many tiles, random south-draining fields with planted cycles, degenerate shapes, the bundled Example and a
4096^2 synthetic network.  The device tier on a Chain's own buffers equals the host tier; NULL outputs are left
untouched; runs are bit-identical."""
import ctypes

import numpy as np
import pytest

import oracle
from conftest import load_example

import _streams_ref as R

pytestmark = pytest.mark.gpu


def check(fdr, river):
    from descriptools_amd import streams
    got = streams.stream_network(fdr, river)
    ref = R.reference(fdr, river)
    for name, g, r in zip(("strahler", "shreve", "link"), got, ref):
        assert g.dtype == r.dtype, name
        if not np.array_equal(g, r):
            bad = np.argwhere(g != r)
            i = tuple(bad[0])
            raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r"
                                 % (name, len(bad), i, g[i], r[i]))
    return got


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_built(name):
    fdr, river, so, sh, lk = R.hand_cases()[name]
    got = check(fdr, river)
    np.testing.assert_array_equal(got.strahler, so)
    np.testing.assert_array_equal(got.shreve, sh)
    np.testing.assert_array_equal(got.link, lk)


def test_comb():
    """a main stem of 8200 cells along row 1 takes a side source from row 0 at every other cell: 4100 junctions in one
    serial countdown chain"""
    W = 8200
    fdr = np.zeros((2, W), np.uint8)
    fdr[1, :] = R.E
    fdr[0, ::2] = R.S
    river = np.zeros((2, W), np.int8)
    river[1, :] = 1
    river[0, ::2] = 1
    so, sh, lk = check(fdr, river)
    assert so.max() == 2 and sh[1, -1] == W // 2
    assert len(np.unique(lk[1])) > 4000


def test_comb_rising_orders():
    """side branches that are themselves Ys keep raising the stem's Shreve magnitude; orders up to 3"""
    W = 6000
    fdr = np.zeros((4, W), np.uint8)
    fdr[3, :] = R.E
    fdr[2, 1::4] = R.S                       # the Y's stem
    fdr[1, 0::4] = R.SE                      # its two sources
    fdr[1, 2::4] = R.SW
    fdr[2, 3::4] = R.S                       # single side sources
    river = (fdr != 0).astype(np.int8)
    river[3, :] = 1
    so, sh, lk = check(fdr, river)
    assert so.max() == 3


def test_serpentine_link():
    """one link of 256 x 256 cells snaking row by row across sixteen 64 x 64 tiles: one head, the first cell"""
    n = 256
    fdr = np.zeros((n, n), np.uint8)
    fdr[0::2, :] = R.E
    fdr[1::2, :] = R.W_
    fdr[0::2, -1] = R.S
    fdr[1::2, 0] = R.S
    fdr[-1, 0] = 0
    river = np.ones((n, n), np.int8)
    so, sh, lk = check(fdr, river)
    assert (so == 1).all() and (sh == 1).all() and (lk == 0).all()


def _south_field(H, W, seed, cycles):
    rng = np.random.default_rng(seed)
    fdr = rng.choice(np.array([R.SW, R.S, R.SE], np.uint8), size=(H, W))
    fdr[rng.random((H, W)) < 0.01] = 0
    fdr[rng.random((H, W)) < 0.005] = 3      # not a D8 code
    river = (rng.random((H, W)) < 0.8).astype(np.int8)
    for _ in range(cycles):                  # 2 x 2 cycles, all in the network
        y, x = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
        fdr[y, x], fdr[y, x + 1], fdr[y + 1, x + 1], fdr[y + 1, x] = R.E, R.S, R.W_, R.N
        river[y:y + 2, x:x + 2] = 1
    return fdr, river


@pytest.mark.parametrize("W", [1024, 1000])
def test_random_south_draining_with_cycles(W):
    fdr, river = _south_field(600, W, W, cycles=40)
    so, sh, lk = check(fdr, river)
    assert (so == -100).any() and so.max() >= 3


@pytest.mark.parametrize("shape", [(1, 5000), (5000, 1), (0, 0), (0, 7), (7, 0), (1, 1)])
def test_degenerate_shapes(shape):
    H, W = shape
    rng = np.random.default_rng(H + 3 * W)
    fdr = np.full(shape, R.E if H == 1 else R.S, np.uint8)
    river = (rng.random(shape) < 0.9).astype(np.int8)
    so, sh, lk = check(fdr, river)
    assert so.shape == shape


def test_example():
    """the bundled Example's GIS D8 raster: fac > 128000 reaches order 2, fac > 1000 order 6 over 29,959 cells"""
    _, fdr, fac, _, _, _ = load_example()
    so, _, _ = check(fdr, fac > 128000)
    assert so.max() == 2
    river = fac > 1000
    assert int(river.sum()) == 29959
    so, _, _ = check(fdr, river)
    assert so.max() == 6


def test_synthetic_4096():
    from descriptools_amd import flowacc, flowdir
    n = 4096
    dem = oracle.synth_dem(5, n, n)
    fdr = flowdir.d8(dem, 10.0)
    fac = flowacc.accumulate(fdr)
    river = fac > 100
    so, sh, _ = check(fdr, river)
    assert so.max() >= 4 and river.sum() > 100000


def _dev(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a))


def test_device_tier_on_chain_buffers():
    """dt_dev_stream_order on a Chain's own fdr / river equals the host tier on their host copies"""
    from descriptools_amd import _lib, chain, device, streams
    H, W = 512, 640
    dem = oracle.synth_dem(7, H, W)
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=10.0, overlap=False, tune_placement=False, river_threshold=200)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float32))
    so_d = ctx.empty((H, W), np.int8)
    sh_d = ctx.empty((H, W), np.int64)
    lk_d = ctx.empty((H, W), np.int64)
    try:
        ch.run(d.ptr)
        _lib.check(_lib.lib().dt_dev_stream_order(ctx.h, ch.p("fdr"), ch.p("river"), H, W, so_d.ptr, sh_d.ptr,
                                                  lk_d.ptr))
        ctx.sync()
        fdr, river = ch.buf["fdr"].to_host(), ch.buf["river"].to_host()
        got = (so_d.to_host(), sh_d.to_host(), lk_d.to_host())
    finally:
        for b in (d, so_d, sh_d, lk_d):
            b.free()
        ch.free()
        ctx.close()
    assert river.sum() > 100
    host = streams.stream_network(fdr, river)
    for g, h in zip(got, host):
        np.testing.assert_array_equal(g, h)
    ref = R.reference(fdr, river)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)


def test_null_outputs_untouched_and_runs_identical():
    from descriptools_amd import _lib, device
    fdr, river = _south_field(300, 1000, 11, cycles=10)
    H, W = fdr.shape
    ref = R.reference(fdr, river)
    ctx = device.Context()
    f_d, r_d = _dev(ctx, fdr), _dev(ctx, river)
    so_d = ctx.empty((H, W), np.int8)
    sh_d = _dev(ctx, np.full((H, W), 12345, np.int64))
    lk_d = _dev(ctx, np.full((H, W), -777, np.int64))
    L = _lib.lib()
    try:
        _lib.check(L.dt_dev_stream_order(ctx.h, f_d.ptr, r_d.ptr, H, W, so_d.ptr, None, None))
        ctx.sync()
        np.testing.assert_array_equal(so_d.to_host(), ref[0])
        assert (sh_d.to_host() == 12345).all() and (lk_d.to_host() == -777).all()
        runs = []
        for _ in range(3):
            _lib.check(L.dt_dev_stream_order(ctx.h, f_d.ptr, r_d.ptr, H, W, so_d.ptr, sh_d.ptr, lk_d.ptr))
            ctx.sync()
            runs.append((so_d.to_host(), sh_d.to_host(), lk_d.to_host()))
        for run in runs:
            for g, r in zip(run, ref):
                np.testing.assert_array_equal(g, r)
        # strahler is required; an empty raster is fine with NULL rasters
        assert L.dt_dev_stream_order(ctx.h, f_d.ptr, r_d.ptr, H, W, None, None, None) != 0
        assert L.dt_dev_stream_order(ctx.h, None, None, 0, 0, None, None, None) == 0
    finally:
        for b in (f_d, r_d, so_d, sh_d, lk_d):
            b.free()
        ctx.close()


def test_unaligned_outputs():
    """output pointers off the 16-byte grid take the scalar store path and give the same bits"""
    from descriptools_amd import _lib, device
    fdr, river = _south_field(64, 333, 5, cycles=3)
    H, W = fdr.shape
    n = H * W
    ref = R.reference(fdr, river)
    ctx = device.Context()
    f_d, r_d = _dev(ctx, fdr), _dev(ctx, river)
    so_d = ctx.empty((n + 16,), np.int8)
    sh_d = ctx.empty((n + 2,), np.int64)
    lk_d = ctx.empty((n + 2,), np.int64)
    try:
        _lib.check(_lib.lib().dt_dev_stream_order(ctx.h, f_d.ptr, r_d.ptr, H, W, so_d.ptr.value + 1, sh_d.ptr.value + 8,
                                                  lk_d.ptr.value + 8))
        ctx.sync()
        so = so_d.to_host()[1:n + 1].reshape(H, W)
        sh = sh_d.to_host()[1:n + 1].reshape(H, W)
        lk = lk_d.to_host()[1:n + 1].reshape(H, W)
    finally:
        for b in (f_d, r_d, so_d, sh_d, lk_d):
            b.free()
        ctx.close()
    for g, r in zip((so, sh, lk), ref):
        np.testing.assert_array_equal(g, r)
