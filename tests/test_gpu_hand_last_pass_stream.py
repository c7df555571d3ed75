"""GPU (-m gpu): the stream of HAND's solving last pass (k_fh_tile3_solve).  A cell goes from the word the tile solve
left in LDS straight to its rasters on one path: the exit-slot look-up is made for every cell and selected, GFI's
n ln(A_river) is taken once per exit slot, and the arm for paths that end on a river cell of the cell's own tile is
compiled only into the code that tiles with river bytes run.  Direction fields built for those decisions, driven through
Chain(external_fdr=True) as test_gpu_hand_last_pass_solve.py does (the river is the chain's own: accumulation >
threshold), with and without the A_river raster, and held to

  * the oracle at test_gpu_hand_fields.py's bars (river index, HAND and A_river equal, flow distance rtol 1e-6, GFI and
    ln(hl/H) rtol 1e-5 / atol 1e-6),
  * the cached kernels' rasters bit for bit (a 1 x 1 RankTile on the same rasters),
  * dt_dev_gfi_lnhlh on the step's own hand, A_river and accumulation bit for bit (what bench.py's verify_step
    compares at 16384^2).

Every field asserts on the CPU, before anything runs on the GPU, that it contains the case it is named for.

A river cell without a height cannot come out of the chain's own river mask (a nodata cell's accumulation is -100, below
any threshold that leaves a non-river cell): the special-values field runs the fused accumulation pass on heights without
nodata and the last pass on a second DEM with the nodata cells planted, which is all the last pass reads heights for."""
import collections
import functools

import numpy as np
import pytest

import oracle
from conftest import assert_float_close

import _hand_fields as F
from test_gpu_hand_last_pass_solve import _rank_tile, fed_mask, intile_path

pytestmark = pytest.mark.gpu

PX, N_GFI, B_GFI = F.PX, 0.4, 0.1
T = F.TILE
E, SE, S, SW, W, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128

# dem: what the fused accumulation pass reads; dem_last: what the last pass reads (None: the same)
Case = collections.namedtuple("Case", "dem fdr thr checks dem_last")


def _dem(shape, seed):
    return (np.random.default_rng(seed).random(shape) * 50.0 + 1.0).astype(np.float32)


def _tile(a, ty, tx):
    return a[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]


def _flat(shape, y, x):
    return y * shape[1] + x


@functools.lru_cache(maxsize=None)
def answer(name):
    c = CASES[name]()
    last = c.dem if c.dem_last is None else c.dem_last
    fac = oracle.flowacc(c.fdr, c.dem)
    river = (fac > c.thr).astype(np.int8)
    fd, idx, hand = oracle.flowhand(last, c.fdr, river, PX)
    e = F.expected(last, c.fdr, river, PX, fac=fac)
    assert np.array_equal(idx, e["idx"]) and np.array_equal(hand, e["hand"])
    assert np.allclose(fd, e["fdist"], rtol=1e-6, atol=0)
    e.update(river=river, fd_oracle=fd, gfi=oracle.gfi(hand, fac, idx, N_GFI, B_GFI, PX),
             lnhlh=oracle.lnhlh(hand, fac, N_GFI, B_GFI, PX))
    c.checks(c, e)
    for a in e.values():
        a.setflags(write=False)
    return c, e


# ---------------------------------------------------------------------------------------------------------
# the fields
# ---------------------------------------------------------------------------------------------------------
def mixed_arms():
    """128 x 128, rows flowing east, river where the accumulation passes 80: T00 and T10 are river-free and sit beside
    T01 and T11, which hold river cells -- both arms of the stream in one launch.  Planted: a block of T01 that flows
    south into T11 (paths of a river tile that end on another tile's river); row 19 of T01 dead, so that T00's row 19
    leaves through exits whose node is dead; (20, 127), a river cell on T01's perimeter with code 0, fed from (19, 127);
    (64, 75), a river cell on T11's perimeter whose code leaves the tile, fed from (65, 75)."""
    shape = (128, 128)
    fdr = np.full(shape, E, np.uint8)
    fdr[40:64, 64:71] = S
    fdr[19, 64:127] = 0
    fdr[19, 127] = S
    fdr[20, 127] = 0
    fdr[64, 75] = N
    fdr[65, 75] = N
    dem = _dem(shape, 31)

    def checks(c, e):
        river, idx = e["river"], e["idx"]
        assert _tile(river, 0, 0).sum() == 0 and _tile(river, 1, 0).sum() == 0, "T00 / T10 are not river-free"
        assert _tile(river, 0, 1).any() and _tile(river, 1, 1).any()
        assert (_tile(idx, 0, 0)[:19] != -100).all(), "the river-free tile resolves nothing"
        # ends on a river cell of the own tile, reached inside the tile
        assert river[5, 81] == 1 and idx[5, 70] == _flat(shape, 5, 81) and intile_path(c.fdr, river, 5, 70)[-1] == (5, 81)
        # leaves the river tile T01 and ends on T11's river
        assert river[50, 66] == 0 and idx[50, 66] != -100 and idx[50, 66] // 128 >= 64 and (idx[50, 66] % 128) >= 64
        assert intile_path(c.fdr, river, 50, 66)[-1][0] == 64
        # dead exit nodes, no river downstream
        assert fed_mask(c.fdr)[19, 64] and c.fdr[19, 64] == 0 and (idx[19, :64] == -100).all()
        # a perimeter river cell with code 0: arriving on it is a dead end
        assert river[20, 127] == 1 and c.fdr[20, 127] == 0 and river[19, 127] == 0 and idx[19, 127] == -100
        # a river cell that is itself a perimeter exit
        assert river[64, 75] == 1 and c.fdr[64, 75] == N and river[65, 75] == 0 and idx[65, 75] == _flat(shape, 64, 75)
        assert not F.wide_tiles(c.fdr, river).any()
    return Case(dem, fdr, 80, checks, None)


def cap_across_exit():
    """192 x 128: one serpentine of full rows, the river 20001 moves from its head.  The head's exit slot resolves
    (the exit cell of its tile is within the cap), the head's own in-tile moves added to it pass 20000: the head is dead,
    the cell after it resolves with exactly 20000 moves -- both behind the same valid slot."""
    cells = []
    for y in range(160):
        xs = range(128) if y % 2 == 0 else range(127, -1, -1)
        cells += [(y, x) for x in xs]
    fdr = F.from_path((192, 128), cells, 0)
    dem = F._path_dem((192, 128), cells)

    def checks(c, e):
        (y0, x0), (y1, x1) = cells[0], cells[1]
        assert e["idx"][y0, x0] == -100 and e["idx"][y1, x1] != -100 and e["nc"][y1, x1] + e["nd"][y1, x1] == 20000
        assert e["river"][cells[20001]] == 1 and e["river"][cells[20000]] == 0
        path = intile_path(c.fdr, e["river"], y0, x0)
        ye, xe = path[-2]  # the exit cell of the head's tile: same tile, on the perimeter, resolving
        assert (ye // T, xe // T) == (y0 // T, x0 // T) and path[-1][1] // T != x0 // T and e["idx"][ye, xe] != -100
        assert len(path) - 2 >= 2 and not F.wide_tiles(c.fdr, e["river"]).any()
    return Case(dem, fdr, 20000, checks, None)


def _corners(diag):
    """192 x 128: a 31-cell feeder along the row into each of the four corner positions of a tile -- T10's top-right and
    bottom-right, T11's top-left and bottom-left -- which leaves diagonally (or cardinally) and reaches a river cell
    three moves on (that one flows on: a river cell with code 0 would be a dead end); everything else is code 0."""
    def make():
        shape = (192, 128)
        fdr = np.zeros(shape, np.uint8)
        plan = []  # (corner cell, first cell outside, direction of the tail)
        for y, up in ((64, True), (127, False)):
            for x, left in ((63, False), (64, True)):
                dy = -1 if up else 1
                dx = (-1 if left else 1) if diag else 0
                feeder = [(y, x + k * (1 if left else -1)) for k in range(30, -1, -1)]
                out = (y + dy, x + dx)
                tail = [(out[0] + k * dy, out[1]) for k in range(4)]
                F.put_path(fdr, feeder + tail + [(tail[-1][0] + dy, tail[-1][1])], 0)
                plan.append(((y, x), out, tail[-1]))
        dem = _dem(shape, 33 + int(diag))

        def checks(c, e):
            river, idx = e["river"], e["idx"]
            assert river.sum() == 8
            local = set()
            for (y, x), out, end in plan:
                assert river[end] == 1 and idx[y, x] == _flat(shape, *end)
                assert (out[0] // T, out[1] // T) != (y // T, x // T)
                assert ((out[0] != y) and (out[1] != x)) == diag
                head = (y, x + (30 if x == 64 else -30))
                assert idx[head] == _flat(shape, *end) and intile_path(c.fdr, river, *head)[-2] == (y, x)
                local.add((y % T, x % T))
            assert local == {(0, 0), (0, T - 1), (T - 1, 0), (T - 1, T - 1)}
        return Case(dem, fdr, 33, checks, None)
    return make


def narrow_gives_up():
    """128 x 128: a serpentine over six rows of T00 (383 cardinal moves in one tile: the narrow solve gives the tile up,
    the marked kernels produce it) that leaves east into T01 and reaches the river 40 moves on"""
    cells = []
    for y in range(6):
        xs = range(63, -1, -1) if y % 2 == 0 else range(64)
        cells += [(y, x) for x in xs]
    cells += [(5, x) for x in range(64, 128)]
    fdr = F.from_path((128, 128), cells, 0)
    dem = F._path_dem((128, 128), cells)

    def checks(c, e):
        river, wide = e["river"], F.wide_tiles(c.fdr, e["river"])
        nc, _ = F.intile_counts(c.fdr, river)
        assert nc[:64, :64].max() > 255 and wide.tolist() == [[True, False], [False, False]]
        assert not river[:64, :64].any() and river[5, 104] and not river[5, 103]
        assert e["nc"][0, 63] == 383 + 41 and (e["idx"][:6, :64] != -100).all()
    return Case(dem, fdr, 383 + 40, checks, None)


def threshold_zero():
    """64 x 64, threshold 0: every cell with an inflow is a river cell, so the heads of the rows (accumulation 0) step
    onto a river cell whose accumulation is 1 -- ln(A_river) = 0 exactly"""
    shape = (64, 64)
    fdr = np.zeros(shape, np.uint8)
    fdr[:, :10] = E
    fdr[::2, 9] = 0
    dem = _dem(shape, 35)

    def checks(c, e):
        river = e["river"]
        assert (e["fac"][:, 0] == 0).all() and (river[:, 0] == 0).all() and (river[:, 1] == 1).all()
        assert (e["a_river"][:, 0] == 1).all() and (e["idx"][:, 0] != -100).all()
        assert (e["hand"][:, 0] != -100).all()
    return Case(dem, fdr, 0, checks, None)


def special_values():
    """128 x 128, rows flowing east, river where the accumulation passes 80 (T01 / T11), the last pass on a second DEM:
    row 3 and row 70 as high as their river cells (HAND exactly 0, in a river-free tile and in a river tile), row 5 below
    its river cell (clipped to 0), nodata cells on the resolving paths of rows 7 and 72, and the river cells of rows 9 and
    74 without a height.  Every row starts with accumulation 0 beside accumulation >= 1."""
    shape = (128, 128)
    fdr = np.full(shape, E, np.uint8)
    dem = _dem(shape, 36)
    last = dem.copy()
    last[3, :] = last[3, 81]
    last[70, :] = last[70, 81]
    last[5, :81] = last[5, 81] - 2.0
    last[7, 20:24] = -100.0
    last[72, 66:70] = -100.0
    last[9, 81] = -100.0
    last[74, 81] = -100.0

    def checks(c, e):
        river, hand, idx = e["river"], e["hand"], e["idx"]
        assert (e["fac"] >= 0).all() and (e["fac"][:, 0] == 0).all() and (e["fac"][:, 1] == 1).all()
        assert (river[:, :81] == 0).all() and (river[:, 81] == 1).all() and (idx[:, :81] != -100).all()
        assert (hand[3, :82] == 0).all() and (hand[70, :82] == 0).all() and (hand[5, :82] == 0).all()
        assert (hand[7, 20:24] == -100).all() and (hand[7, :20] != -100).all() and (idx[7, 20:24] != -100).all()
        assert (hand[72, 66:70] == -100).all() and (hand[72, 70:81] != -100).all()
        for y in (9, 74):
            assert c.dem_last[y, 81] == -100 and (idx[y, :81] == _flat(shape, y, 81)).all()
            assert (hand[y, :81] == c.dem_last[y, :81] + np.float32(100)).all() and hand[y, 81] == -100
    return Case(dem, fdr, 80, checks, last)


CASES = {"mixed_arms-128x128": mixed_arms, "cap_across_exit-192x128": cap_across_exit,
         "corners_diagonal-192x128": _corners(True), "corners_cardinal-192x128": _corners(False),
         "narrow_gives_up-128x128": narrow_gives_up, "threshold_zero-64x64": threshold_zero,
         "special_values-128x128": special_values}


# ---------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------
RASTERS = ("fac", "river", "idx", "fdist", "hand", "gfi", "lnhlh")


def _chain(c, want_a_river):
    """Chain(external_fdr=True): walks in the fused pass, the solve in the last pass (which reads c.dem_last when the
    case has one); then GFI and ln(hl/H) again from the step's own hand, A_river and accumulation, unfused"""
    import ctypes as C
    from descriptools_amd import _lib, chain, device
    H, W = c.fdr.shape
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=PX, n_gfi=N_GFI, b=B_GFI, overlap=False, tune_placement=False,
                     external_fdr=True, river_threshold=c.thr)
    d = ctx.to_device(c.dem)
    d2 = d if c.dem_last is None else ctx.to_device(c.dem_last)
    bufs = [d] + ([d2] if d2 is not d else [])
    try:
        ch.buf["fdr"].copy_from(c.fdr)
        last = {name: call for name, _, call in ch.ops(d2.ptr, want_a_river)}["flowhand_gfi_finish"]
        for name, _, call in ch.ops(d.ptr, want_a_river):
            _lib.check(last() if name == "flowhand_gfi_finish" else call())
        ctx.sync()
        ch.check_status()
        out = {k: ch.buf[k].to_host() for k in RASTERS}
        if want_a_river:
            out["a_river"] = ch.buf["a_river"].to_host()
            ar = out["a_river"]
        else:
            ok = out["idx"] >= 0
            ar = np.where(ok, out["fac"].ravel()[np.where(ok, out["idx"], 0)], -100).astype(np.int32)
        hand_d, ar_d, fac_d = ctx.to_device(out["hand"]), ctx.to_device(ar), ctx.to_device(out["fac"].astype(np.int32))
        g_d, l_d = ctx.empty((H, W), np.float32), ctx.empty((H, W), np.float32)
        bufs += [hand_d, ar_d, fac_d, g_d, l_d]
        _lib.check(_lib.lib().dt_dev_gfi_lnhlh(ctx.h, hand_d.ptr, ar_d.ptr, fac_d.ptr, H * W, N_GFI, B_GFI, PX,
                                              g_d.ptr, l_d.ptr))
        ctx.sync()
        out["gfi_unfused"], out["lnhlh_unfused"] = g_d.to_host(), l_d.to_host()
        return out
    finally:
        for b in bufs:
            b.free()
        ch.free()
        ctx.close()


@pytest.mark.parametrize("name", list(CASES))
def test_last_pass_stream(name):
    c, e = answer(name)
    out = _chain(c, True)
    assert np.array_equal(out["fac"], e["fac"]), "fac"
    assert np.array_equal(out["river"], e["river"]), "river"
    assert np.array_equal(out["idx"], e["idx"]), "%d river indices differ" % int((out["idx"] != e["idx"]).sum())
    assert np.array_equal(out["hand"], e["hand"]), "%d HAND cells differ" % int((out["hand"] != e["hand"]).sum())
    assert np.array_equal(out["fdist"] == -100, e["fd_oracle"] == -100)
    assert np.allclose(out["fdist"], e["fd_oracle"], rtol=1e-6, atol=0), "flow distance"
    assert np.array_equal(out["a_river"], e["a_river"]), "A_river"
    dead = e["idx"] == -100
    for k in ("gfi", "lnhlh"):
        assert (out[k][dead] == -100).all(), "%s: not -100 where no river is found" % k
        assert out[k].tobytes() == out[k + "_unfused"].tobytes(), "%s: not the unfused kernel's bits (%d cells)" % (
            k, int((out[k].view(np.uint32) != out[k + "_unfused"].view(np.uint32)).sum()))
        assert_float_close(out[k], e[k], rtol=1e-5, atol=1e-6, what=k)
    # the cached kernels on the same rasters (they read the last pass's DEM only)
    old = _rank_tile(c._replace(dem=c.dem if c.dem_last is None else c.dem_last), e)
    for k in ("idx", "fdist", "hand", "a_river"):
        assert out[k].dtype == old[k].dtype and out[k].tobytes() == old[k].tobytes(), "%s: not the cached path's bits" % k
    # without the A_river raster: every other raster byte for byte the same
    out2 = _chain(c, False)
    for k in RASTERS + ("gfi_unfused", "lnhlh_unfused"):
        assert out[k].dtype == out2[k].dtype and out[k].tobytes() == out2[k].tobytes(), "%s changes with want_a_river" % k
