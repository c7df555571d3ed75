"""GPU (-m gpu): HAND with the tile solve in the LAST pass.  On a single raster the fused accumulation + HAND pass only
walks the fed perimeter entries (k_fa3fh1w*: fh_walk_body) and k_fh_tile3_solve solves every tile; a tile whose narrow
solve overflows goes through k_fh_tile1_marked / k_fh_tile3_marked.  Direction fields built for that split, driven
through Chain(external_fdr=True) (the river is the chain's own: accumulation > threshold) and held to
oracle.flowhand / oracle.gfi / oracle.lnhlh with test_gpu_hand_fields.py's bars -- river index and HAND equal, flow
distance within rtol 1e-6, GFI and ln(hl/H) within rtol 1e-5 / atol 1e-6 -- and, bit for bit, to the same rasters out of
the cached kernels, which a 1 x 1 RankTile still takes.

Every field asserts on the CPU that it contains the case it is named for (checks(): which perimeter cells are fed, which
directions cross tile borders, which tiles the narrow solve gives up), so a field that stops exercising its case fails."""
import collections
import functools

import numpy as np
import pytest

import oracle
from conftest import assert_float_close

import _hand_fields as F

pytestmark = pytest.mark.gpu

PX, N_GFI, B_GFI = F.PX, 0.4, 0.1
T = F.TILE
E, SE, S, SW, W, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
MIRROR = np.arange(256, dtype=np.uint8)  # the code of the same move in the raster flipped left to right
for _a, _b in ((E, W), (SE, SW), (NE, NW)):
    MIRROR[_a], MIRROR[_b] = _b, _a

Case = collections.namedtuple("Case", "dem fdr thr checks")


# ---------------------------------------------------------------------------------------------------------
# what a field contains, restated on the CPU
# ---------------------------------------------------------------------------------------------------------
def crossings(fdr):
    """(y, x, ny, nx) of every step that lands in another tile of the raster"""
    ok, _, _, ny, nx = F._successor(np.asarray(fdr, np.uint8))
    yy, xx = np.mgrid[0:fdr.shape[0], 0:fdr.shape[1]]
    m = ok & ((ny // T != yy // T) | (nx // T != xx // T))
    return yy[m], xx[m], ny[m], nx[m]


def fed_mask(fdr):
    """cells some other tile's cell steps onto: the entries pass 1 walks"""
    fed = np.zeros(fdr.shape, bool)
    _, _, ny, nx = crossings(fdr)
    fed[ny, nx] = True
    return fed


def intile_path(fdr, river, y, x):
    """the cells of the in-tile walk from (y, x), as fh_walk_body makes it (an in-tile cycle: until it closes)"""
    ok, _, _, ny, nx = F._successor(np.asarray(fdr, np.uint8))
    cells = [(y, x)]
    while ok[y, x] and river[y, x] != 1 and fdr[y, x] != 0:
        y2, x2 = int(ny[y, x]), int(nx[y, x])
        if (y2 // T, x2 // T) != (y // T, x // T) or (y2, x2) in cells:
            cells.append((y2, x2))
            break
        y, x = y2, x2
        cells.append((y, x))
    return cells


@functools.lru_cache(maxsize=None)
def answer(name):
    c = CASES[name]()
    fac = oracle.flowacc(c.fdr, c.dem)
    river = (fac > c.thr).astype(np.int8)
    fd, idx, hand = oracle.flowhand(c.dem, c.fdr, river, PX)
    e = F.expected(c.dem, c.fdr, river, PX, fac=fac)
    # the closed-form answer of _hand_fields and the oracle's walk agree on what is compared by equality
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
def _dem(shape, seed):
    return (np.random.default_rng(seed).random(shape) * 50.0 + 1.0).astype(np.float32)


def one_tile():
    """64 x 64: one tile, no other tile to feed it -- every node word is the unfed one, the last pass solves alone"""
    f = F.descending((64, 64))[0]

    def checks(c, e):
        assert not fed_mask(c.fdr).any() and e["river"].any() and (e["idx"] != -100).sum() > 1000
        assert not F.wide_tiles(c.fdr, e["river"]).any()
    return Case(f.dem, f.fdr, 40, checks)


def _ring(H):
    """T00 flows south, T10 east, T11 north, T01 east and off the raster; the border rows and columns cross with all
    three moves of their side in turn, so every cell of T10's top row (but the one at the corner), T11's left column and
    T01's bottom row is fed.
    With 192 rows the third tile row flows north into the second.  Planted on entries of T10's top row: code 0, a first
    move that leaves the tile again, a nodata stretch; the row's accumulation makes most of its entries river cells."""
    fdr = np.zeros((H, 128), np.uint8)
    fdr[:64, :64] = S
    fdr[64:128, :64] = E
    fdr[64:128, 64:] = N
    fdr[:64, 64:] = E
    fdr[63, :64] = np.array([SW, S, SE], np.uint8)[np.arange(64) % 3]   # onto (64, x - 1 | x | x + 1)
    fdr[63, 0], fdr[63, 62] = S, S
    fdr[63, 63] = SE  # T00 -> T11 through the corner of four tiles (so (64, 63) alone has no feeder)
    fdr[64:128, 63] = np.array([NE, E, SE], np.uint8)[np.arange(64) % 3]  # onto (y - 1 | y | y + 1, 64)
    fdr[64, 63] = E
    fdr[64, 64:] = np.array([NW, N, NE], np.uint8)[np.arange(64) % 3]   # onto (63, x - 1 | x | x + 1)
    fdr[64, 64] = N  # (NW would step back into T00 and close a cycle)
    if H > 128:
        fdr[128:, :] = N
        fdr[128, :] = np.array([NW, N, NE], np.uint8)[np.arange(128) % 3]
        fdr[128, 0], fdr[128, 127] = N, N
    fdr[64, 5] = 0       # a fed entry with code 0
    fdr[64, 10] = NE     # a fed entry whose first move leaves the tile again: (63, 11), which steps back to (64, 11)
    dem = _dem((H, 128), 21)
    dem[64, 20:24] = -100.0  # nodata on the path of the entries west of it

    def checks(c, e):
        fed, river = fed_mask(c.fdr), e["river"]
        assert fed[64, :63].all() and fed[64:128, 64].all() and fed[63, 64:].all()
        y, x, ny, nx = crossings(c.fdr)
        moves = set(zip((ny - y).tolist(), (nx - x).tolist()))
        assert moves >= {(1, 0), (1, 1), (1, -1), (0, 1), (-1, 1), (-1, 0), (-1, -1)}
        assert ((ny // T != y // T) & (nx // T != x // T)).any(), "no diagonal step through a tile corner"
        assert fed[64, 5] and c.fdr[64, 5] == 0
        assert fed[64, 10] and intile_path(c.fdr, river, 64, 10)[1] == (63, 11)
        assert fed[64, 12] and (64, 21) in intile_path(c.fdr, river, 64, 12) and e["fac"][64, 21] == -100
        riv_entries = fed & (river == 1)
        assert riv_entries[64, 30:63].all() and not river[64, :5].any()
        assert not F.wide_tiles(c.fdr, river).any() and (e["idx"] != -100).sum() > 4000
    return Case(dem, fdr, 1000, checks)


def _mirrored(make):
    """the same field flipped left to right: the crossings that went east, north-east and south-east go west"""
    def flipped():
        c = make()

        def checks(c2, e):
            y, x, ny, nx = crossings(c2.fdr)
            assert set(zip((ny - y).tolist(), (nx - x).tolist())) >= {(0, -1), (-1, -1), (1, -1)}
        return Case(np.ascontiguousarray(c.dem[:, ::-1]), np.ascontiguousarray(MIRROR[c.fdr][:, ::-1]), c.thr, checks)
    return flipped


def river_free_beside_all_river():
    """128 x 128, every valid cell a river cell (threshold -1): T00 is nodata throughout (accumulation -100: river-free)
    and flows east into T01, all river"""
    fdr = np.full((128, 128), E, np.uint8)
    fdr[64:, :] = N
    dem = _dem((128, 128), 22)
    dem[:64, :64] = -100.0

    def checks(c, e):
        river = e["river"]
        assert river[:64, :64].sum() == 0 and river[:64, 64:].all() and fed_mask(c.fdr)[:64, 64].all()
        assert (e["idx"][:64, :64] != -100).all() and (e["hand"][:64, :64] == -100).all()
    return Case(dem, fdr, -1, checks)


def cycles():
    """128 x 128: a row of T00 enters T01 and runs into a cycle inside it; a rectangle cycle lies across the T10 / T11
    border, with a feeder from T10; a long row with a river keeps the rasters from being empty"""
    fdr = np.zeros((128, 128), np.uint8)
    F.put_path(fdr, [(10, x) for x in range(40, 71)], E)  # (10, 70) -> (10, 71): onto the cycle
    F.put_path(fdr, F._rect_cycle(10, 71, 6, 9), 0)
    cyc = F._rect_cycle(10, 71, 6, 9)
    d = (cyc[0][0] - cyc[-1][0], cyc[0][1] - cyc[-1][1])
    fdr[cyc[-1]] = F.CODE_OF[d]
    two = [(100, x) for x in range(62, 66)] + [(101, x) for x in range(65, 61, -1)]
    F.put_path(fdr, two + [two[0]], 0)
    fdr[100, 62] = E
    F.put_path(fdr, [(100, x) for x in range(30, 62)], E)
    F.put_path(fdr, [(120, x) for x in range(0, 128)], 0)
    dem = _dem((128, 128), 23)

    def checks(c, e):
        fed, river = fed_mask(c.fdr), e["river"]
        assert fed[10, 64] and len(set(p := intile_path(c.fdr, river, 10, 64))) < len(p), "no in-tile cycle from the entry"
        assert fed[100, 64] and fed[101, 63] and e["fac"][100, 64] == -100  # the cycle spanning two tiles
        assert (e["idx"][10, 40:71] == -100).all() and (e["idx"][100, 30:66] == -100).all()
        assert river[120, 101:].all() and fed[120, 64] and (e["idx"][120, :100] != -100).all()
    return Case(dem, fdr, 100, checks)


def serpentine():
    """128 x 128: T00 is one serpentine of 4096 cells (4032 cardinal moves in one tile: the narrow solve gives it up,
    the marked-tile redo produces it) that leaves east into T01 and reaches the river there after 40 more moves; a
    column of T10 feeds the serpentine's last row from the south"""
    cells = []
    for y in range(64):
        xs = range(63, -1, -1) if y % 2 == 0 else range(64)
        cells += [(y, x) for x in xs]
    cells += [(63, x) for x in range(64, 128)]
    fdr = F.from_path((128, 128), cells, 0)
    F.put_path(fdr, [(y, 5) for y in range(100, 62, -1)], fdr[63, 5])
    dem = F._path_dem((128, 128), cells)

    def checks(c, e):
        river, wide = e["river"], F.wide_tiles(c.fdr, e["river"])
        nc, nd = F.intile_counts(c.fdr, river)
        assert nc[:64, :64].max() > 255 and wide.tolist() == [[True, False], [False, False]]
        assert fed_mask(c.fdr)[63, 5] and not river[:64, :64].any() and river[63, 104] and not river[63, 103]
        assert e["nc"][0, 63] == 4095 + 41 and (e["idx"][:64, :64] != -100).all()
    return Case(dem, fdr, 4095 + 37 + 40, checks)


def cap():
    """192 x 128: a serpentine of full rows, a tile border every 64 moves and no tile the narrow solve gives up; the
    river starts 20001 moves from the head -- the head is dead, the cell after it resolves with exactly 20000 moves"""
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
        assert not F.wide_tiles(c.fdr, e["river"]).any() and len(F.tile_crossings(c.fdr)) >= 7
    return Case(dem, fdr, 20000, checks)


CASES = {"one_tile-64x64": one_tile, "ring-128x128": lambda: _ring(128), "ring-192x128": lambda: _ring(192),
         "ring_mirrored-128x128": _mirrored(lambda: _ring(128)), "river_free_beside_all_river-128x128":
         river_free_beside_all_river, "cycles-128x128": cycles, "serpentine-128x128": serpentine, "cap-192x128": cap}


# ---------------------------------------------------------------------------------------------------------
# the two paths on the GPU
# ---------------------------------------------------------------------------------------------------------
def _chain(c):
    """Chain(external_fdr=True): walks in the fused pass, the solve in the last pass"""
    from descriptools_amd import chain, device
    H, W = c.fdr.shape
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=PX, n_gfi=N_GFI, b=B_GFI, overlap=False, tune_placement=False,
                     external_fdr=True, river_threshold=c.thr)
    d = ctx.to_device(c.dem)
    try:
        ch.buf["fdr"].copy_from(c.fdr)
        ch.run(d.ptr)
        ctx.sync()
        ch.check_status()
        return {k: ch.buf[k].to_host() for k in ("fac", "river", "idx", "fdist", "hand", "a_river", "gfi", "lnhlh")}
    finally:
        d.free()
        ch.free()
        ctx.close()


def _rank_tile(c, e):
    """the cached kernels (k_fh_tile1n, k_fh_tile3 on the word cache): a 1 x 1 RankTile on the same rasters"""
    import torch
    from descriptools_amd import tiling
    H, W = c.fdr.shape
    h = tiling.HALO
    t = tiling.RankTile(tiling.Layout([H], [W]), 0, device=0, px=PX, river_threshold=10, tune_placement=False)
    try:
        for k, a, fill in (("fdr", c.fdr, 0), ("river", e["river"], 0), ("dem", c.dem, 1.0),
                           ("fac", e["fac"].astype(np.int32), 0)):
            p = np.full((H + 2 * h, W + 2 * h), fill, a.dtype)
            p[h:h + H, h:h + W] = a
            t.t[k].copy_(torch.as_tensor(p))
        torch.cuda.synchronize()
        t.fill_ring_codes()
        t.fh_local(sync=False)
        t.ctx.sync()
        rows = t.fh_row.clone()
        torch.cuda.synchronize()
        t.fh_solve_finish(rows)
        return {k: t.host(k) for k in ("idx", "fdist", "hand", "a_river")}
    finally:
        t.free()


@pytest.mark.parametrize("name", list(CASES))
def test_last_pass_solve(name):
    c, e = answer(name)
    out = _chain(c)
    assert np.array_equal(out["fac"], e["fac"]), "fac"
    assert np.array_equal(out["river"], e["river"]), "river"
    assert np.array_equal(out["idx"], e["idx"]), "%d river indices differ" % int((out["idx"] != e["idx"]).sum())
    assert np.array_equal(out["hand"], e["hand"]), "%d HAND cells differ" % int((out["hand"] != e["hand"]).sum())
    assert np.array_equal(out["fdist"] == -100, e["fd_oracle"] == -100)
    assert np.allclose(out["fdist"], e["fd_oracle"], rtol=1e-6, atol=0), "flow distance"
    assert np.array_equal(out["a_river"], e["a_river"]), "A_river"
    if (e["fac"] >= 0).all():  # (test_gpu_hand_fields.py: GFI is compared on fields without -100 accumulation)
        assert_float_close(out["gfi"], e["gfi"], rtol=1e-5, atol=1e-6, what="gfi")
        assert_float_close(out["lnhlh"], e["lnhlh"], rtol=1e-5, atol=1e-6, what="lnhlh")
    old = _rank_tile(c, e)
    for k in ("idx", "fdist", "hand", "a_river"):
        assert out[k].dtype == old[k].dtype and out[k].tobytes() == old[k].tobytes(), "%s: not the cached path's bits" % k
