"""GPU (-m gpu): flow accumulation's perimeter graph in the gather form -- pass 3 sums an entry cell's inflow from its
feeders' resolved words, and the countdown combines the first hops of a wave's source exits by parent (k_fa_reduce,
fa_gather in dt_tiles.hip) -- against the oracle and against the scatter form it replaced (debug key
DT_DBG_FA_SCATTER = 9), bit for bit.  Each field runs on a width that takes the fused last pass (W % 64 == 0,
k_fa3fh1) and on one that does not (k_fa_tile3)."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

DBG_FA_SCATTER = 9
E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128


def _run_single(fdr, dem, scatter):
    """dt_dev_flowacc_river_flowhand_local (the chain's op) and dt_flowacc_u8 under one setting of the key"""
    from descriptools_amd import _lib, flowacc
    from descriptools_amd.device import Context
    L = _lib.lib()
    H, W = fdr.shape
    _lib.check(L.dt_debug_set(DBG_FA_SCATTER, scatter))
    ctx = Context()
    try:
        f, d = ctx.to_device(np.ascontiguousarray(fdr, np.uint8)), ctx.to_device(np.ascontiguousarray(dem, np.float32))
        fac, river = ctx.empty((H, W), np.int32), ctx.empty((H, W), np.int8)
        _lib.check(L.dt_dev_flowacc_river_flowhand_local(ctx.h, f.ptr, d.ptr, H, W, 50, fac.ptr, river.ptr))
        ctx.sync()
        a = fac.to_host().astype(np.int64)
        for b in (f, d, fac, river):
            b.free()
        b2 = flowacc.accumulate(fdr, dem)
    finally:
        _lib.check(L.dt_debug_set(DBG_FA_SCATTER, 0))
        ctx.close()
    return a, b2


def _check_single(fdr, dem=None):
    if dem is None:
        dem = np.zeros(fdr.shape, np.float32)
    ref = oracle.flowacc(fdr, dem)
    for scatter in (0, 1):
        for got in _run_single(fdr, dem, scatter):
            assert np.array_equal(got, ref), (scatter, int((got != ref).sum()))
    return ref


def _south(rng, H, W):
    fdr = np.full((H, W), S, np.uint8)
    fdr[rng.random((H, W)) < 0.2] = SE
    fdr[rng.random((H, W)) < 0.2] = SW
    return fdr


@pytest.mark.parametrize("W", [192, 200])
def test_cycles_across_two_and_four_tiles(W):
    """A 4-cycle around the corner where four tiles meet, a long rectangular cycle through two tiles, and south-flowing
    terrain draining into both (and through the tiles below them): the cycles' cells are -100, what only feeds them is
    counted, and nothing downstream of a pending exit is resolved."""
    H = 192
    fdr = _south(np.random.default_rng(W), H, W)
    fdr[63, 63], fdr[63, 64], fdr[64, 64], fdr[64, 63] = E, S, W_, N      # four tiles
    fdr[20, 40:90] = E                                                   # tiles (0, 0) and (0, 1)
    fdr[20:30, 90] = S
    fdr[30, 41:91] = W_
    fdr[21:31, 40] = N
    ref = _check_single(fdr)
    assert (ref == -100).sum() >= 4 + 2 * 50 + 2 * 10 - 4


@pytest.mark.parametrize("W", [192, 200])
def test_exit_with_most_feeders(W):
    """Every cell around tile (1, 1) steps into it and the tile drains through one exit: 259 source exits with one
    parent, spread over several waves (their first hops combine within a wave; the lane whose returned count equals its
    wave's share retires the exit).  The corner entry (64, 64) has all five outside neighbours as feeders."""
    H = 192
    fdr = np.full((H, W), S, np.uint8)
    fdr[63, 64:128] = S
    fdr[63, 63], fdr[63, 128] = SE, SW
    fdr[64:128, 63] = E
    fdr[64:128, 128] = W_
    fdr[128, 64:128] = N
    fdr[128, 63], fdr[128, 128] = NE, NW
    fdr[63, 65], fdr[65, 63] = SW, NE                                     # corner entry: five feeders
    fdr[64:127, 64:128] = S                                               # the tile drains to its bottom row ...
    fdr[127, 64:96] = E
    fdr[127, 97:128] = W_
    fdr[127, 96] = S                                                      # ... and leaves through (127, 96)
    fdr[128, 96] = S
    ref = _check_single(fdr)
    assert ref[128, 96] >= 64 * 64 + 259


@pytest.mark.parametrize("W", [256, 264])
def test_every_exit_a_source(W):
    """Even tile columns flow east into odd ones, which flow south onto a row of sinks: every exit of the raster is a
    source, and no entry path leads to another exit (nothing for the countdown, everything for the gather)."""
    H = 192
    fdr = np.full((H, W), E, np.uint8)
    x = np.arange(W)
    odd = (x // 64) % 2 == 1
    fdr[:, odd] = S
    for ty in range(H // 64):
        fdr[64 * ty + 63, odd] = 0
    _check_single(fdr)


@pytest.mark.parametrize("W", [192, 200])
def test_random_fields_both_forms(W):
    """arbitrary codes (cycles inside and across tiles, dead ends) and a nodata blob"""
    rng = np.random.default_rng(7 + W)
    codes = np.array([E, SE, S, SW, W_, NW, N, NE], np.uint8)
    fdr = codes[rng.integers(0, 8, size=(256, W))]
    dem = np.zeros(fdr.shape, np.float32)
    dem[100:120, 30:70] = -100.0
    _check_single(fdr, dem)


def _rank_run(acc64, fdr, ext, scatter):
    import torch
    from descriptools_amd import _lib, tiling
    L = _lib.lib()
    layout = tiling.Layout([192], [192, fdr.shape[1]])
    _lib.check(L.dt_debug_set(DBG_FA_SCATTER, scatter))
    try:
        t = tiling.RankTile(layout, 1, device=0, river_threshold=2 ** 20, acc64=acc64)
        h = t.halo
        t.t["fdr"].fill_(E)
        t.t["fdr"][h:h + t.H, h:h + t.W] = torch.as_tensor(fdr, device=t.t["fdr"].device)
        t.t["dem"].fill_(1.0)
        torch.cuda.synchronize()
        t.fa_local()
        t.fa_finish(ext)
        t.check_status()
        fac = t.host("fac").astype(np.int64)
        t.free()
    finally:
        _lib.check(L.dt_debug_set(DBG_FA_SCATTER, 0))
    return fac


@pytest.mark.parametrize("acc64", [False, True])
@pytest.mark.parametrize("W", [192, 200])
def test_rank_step_with_injected_inflow(acc64, W):
    """A rank whose west ring receives inflow from the rank before it -- beyond 2^31 on the int64 path, where the last
    pass carries it in two limbs -- on an east-flowing field with a cycle across two tiles and one across four, so that
    k_fa_propagate's ext and the gathered inflow meet at the same entries.  Gather form == scatter form, and the
    cycle-free rows equal their closed form."""
    from descriptools_amd import tiling
    H = 192
    fdr = np.full((H, W), E, np.uint8)
    fdr[63, 63], fdr[63, 64], fdr[64, 64], fdr[64, 63] = E, S, W_, N
    fdr[100, 60:70], fdr[100, 70], fdr[101, 61:71], fdr[101, 60] = E, S, W_, N
    fdr[140, 10:190] = SE if W > 192 else E
    ys, xs = tiling.ring_coords(H, W)
    ext = np.zeros(len(ys), np.uint64)
    big = 2 ** 33 + 7 if acc64 else 2 ** 24 + 3
    ext[(ys == 5) & (xs == 0)] = big
    ext[(ys == 63) & (xs == 0)] = 11                                      # runs into the four-tile cycle
    ext[(ys == 150) & (xs == 0)] = 5
    got = [_rank_run(acc64, fdr, ext, s) for s in (0, 1)]
    assert np.array_equal(got[0], got[1]), int((got[0] != got[1]).sum())
    x = np.arange(W, dtype=np.int64)
    assert np.array_equal(got[0][5], x + big)
    assert np.array_equal(got[0][150], x + 5)
    assert got[0][63, 63] == -100 and got[0][100, 65] == -100
