"""Adversarial direction fields for HAND (flow distance, river index, height above drainage) and the answer the
kernels are held to on them -- test infrastructure shared by test_hand_fields_host.py and test_gpu_hand_fields.py.

Every field is generated from a seed or a formula.  A family is a function returning a list of Field(name, dem, fdr,
river); `intile_counts` restates the tile pass's in-tile walk so that the tests can assert WHICH tile solve a field
reaches (the narrow 32-bit one or the 64-bit fallback) instead of hoping for it."""
import collections
import functools

import numpy as np

import oracle

TILE = 64
# ESRI codes: E=1, SE=2, S=4, SW=8, W=16, NW=32, N=64, NE=128
DELTA = {1: (0, 1), 2: (1, 1), 4: (1, 0), 8: (1, -1), 16: (0, -1), 32: (-1, -1), 64: (-1, 0), 128: (-1, 1)}
CODE_OF = {d: c for c, d in DELTA.items()}
D8 = np.array(sorted(DELTA), np.uint8)
NON_D8 = np.array([0, 3, 255], np.uint8)
_DY = np.zeros(256, np.int64)
_DX = np.zeros(256, np.int64)
_VALID = np.zeros(256, bool)
for _c, (_dy, _dx) in DELTA.items():
    _DY[_c], _DX[_c], _VALID[_c] = _dy, _dx, True

Field = collections.namedtuple("Field", "name dem fdr river")


# ---------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------
def from_path(shape, cells, last_code):
    """the codes that lead along a list of 8-connected cells (the last one gets `last_code`); every other cell 0"""
    fdr = np.zeros(shape, np.uint8)
    put_path(fdr, cells, last_code)
    return fdr


def put_path(fdr, cells, last_code):
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    assert c[:, 0].min() >= 0 and c[:, 1].min() >= 0 and c[:, 0].max() < fdr.shape[0] and c[:, 1].max() < fdr.shape[1]
    d = np.diff(c, axis=0)
    assert np.abs(d).max(initial=0) <= 1 and (np.abs(d).sum(axis=1) > 0).all(), "cells are not 8-connected"
    lut = np.zeros((3, 3), np.uint8)
    for (dy, dx), code in CODE_OF.items():
        lut[dy + 1, dx + 1] = code
    fdr[c[:-1, 0], c[:-1, 1]] = lut[d[:, 0] + 1, d[:, 1] + 1]
    fdr[c[-1, 0], c[-1, 1]] = last_code


def _successor(fdr):
    """(moves, flat index of the successor, diagonal?) of every cell: moves is False for a code that is no D8 code
    and for a step off the raster"""
    H, W = fdr.shape
    yy, xx = np.mgrid[0:H, 0:W]
    ny, nx = yy + _DY[fdr], xx + _DX[fdr]
    ok = _VALID[fdr] & (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
    return ok, np.where(ok, ny * W + nx, yy * W + xx), (_DY[fdr] != 0) & (_DX[fdr] != 0), ny, nx


def intile_counts(fdr, river):
    """The tile pass's in-tile walk restated: from every cell follow the codes until the path ends (code 0 or no D8
    code, a river cell, a step off the raster) or would leave its 64 x 64 tile.  Returns the (cardinal, diagonal) move
    counts per cell, the walk capped at 4096 iterations (a cell on or above an in-tile cycle reaches the cap)."""
    fdr = np.asarray(fdr, np.uint8)
    H, W = fdr.shape
    ok, nxt, diag, ny, nx = _successor(fdr)
    yy, xx = np.mgrid[0:H, 0:W]
    moves = ok & (np.asarray(river) != 1) & (ny // TILE == yy // TILE) & (nx // TILE == xx // TILE)
    moves, nxt, diag = moves.ravel(), nxt.ravel(), diag.ravel()
    nc = np.zeros(H * W, np.int32)
    nd = np.zeros(H * W, np.int32)
    cell = np.flatnonzero(moves)  # cells still walking, and where they are
    pos = cell.copy()
    for _ in range(4096):
        if cell.size == 0:
            break
        d = diag[pos]
        nd[cell[d]] += 1
        nc[cell[~d]] += 1
        pos = nxt[pos]
        keep = moves[pos]
        cell, pos = cell[keep], pos[keep]
    return nc.reshape(H, W), nd.reshape(H, W)


def wide_tiles(fdr, river):
    """per tile: does the narrow tile solve give it up (some in-tile count above 255)?"""
    nc, nd = intile_counts(fdr, river)
    H, W = nc.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    m = np.zeros((ty * TILE, tx * TILE), np.int32)
    m[:H, :W] = np.maximum(nc, nd)
    return m.reshape(ty, TILE, tx, TILE).max(axis=(1, 3)) > 255


def tile_crossings(fdr):
    """set of (from tile, to tile) pairs that some cell's step connects, tiles as (ty, tx)"""
    H, W = fdr.shape
    ok, _, _, ny, nx = _successor(np.asarray(fdr, np.uint8))
    yy, xx = np.mgrid[0:H, 0:W]
    m = ok & ((ny // TILE != yy // TILE) | (nx // TILE != xx // TILE))
    return set(zip(zip((yy[m] // TILE).tolist(), (xx[m] // TILE).tolist()),
                   zip((ny[m] // TILE).tolist(), (nx[m] // TILE).tolist())))


# ---------------------------------------------------------------------------------------------------------
# the expected answer
# ---------------------------------------------------------------------------------------------------------
def expected(dem, fdr, river, px, fac=None):
    """dict(idx, nc, nd, fdist, hand, a_river, fac): river index and move counts from the oracle's O(N) solve, the
    flow distance in closed form (one rounding), HAND as flowhand.py:414-442 takes it (float32 difference, negatives
    other than exactly -100 clipped to 0), A_river = fac[idx]"""
    dem = np.ascontiguousarray(dem, np.float32)
    fdr = np.ascontiguousarray(fdr, np.uint8)
    river = np.ascontiguousarray(river, np.int8)
    idx, nc, nd = oracle.flowhand_fast(fdr, river)
    ok = idx != -100
    fdist = np.where(ok, px * nc.astype(np.float64) + (px * np.sqrt(2.0)) * nd.astype(np.float64), -100.0)
    fdist = fdist.astype(np.float32)
    safe = np.where(ok, idx, 0)
    hand = np.full(dem.shape, -100.0, np.float32)
    m = (dem != np.float32(-100)) & ok
    h = (dem - dem.ravel()[safe]).astype(np.float32)
    h = np.where((h < 0) & (h != np.float32(-100)), np.float32(0), h)
    hand[m] = h[m]
    if fac is None:
        fac = oracle.flowacc(fdr, dem)
    a_river = np.where(ok, fac.ravel()[safe], -100)
    return dict(idx=idx, nc=nc, nd=nd, fdist=fdist, hand=hand, a_river=a_river, fac=fac)


def one_kind(e):
    """cells of an expected() answer whose path is made of one kind of move (or none): their flow distance is one
    product, exact whatever the order of the kernel's arithmetic"""
    return (e["nc"] == 0) | (e["nd"] == 0) | (e["idx"] == -100)


# ---------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------
def _dem_random(shape, seed):
    return (np.random.default_rng(1000 + seed).random(shape) * 50.0 + 1.0).astype(np.float32)


def _river_from_acc(fdr, thr):
    return (oracle.flowacc(fdr) > thr).astype(np.int8)


def uniform(shape, seed=0):
    """every cell carries the same code, one field per D8 code.  Rivers: one cell per tile, the raster's four corners
    and the four corners of an interior tile -- every perimeter slot exits in every direction"""
    H, W = shape
    river = np.zeros(shape, np.int8)
    river[31::TILE, 17::TILE] = 1
    river[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 1
    if H >= 2 * TILE and W >= 2 * TILE:
        river[[TILE, TILE, 2 * TILE - 1, 2 * TILE - 1], [TILE, 2 * TILE - 1, TILE, 2 * TILE - 1]] = 1
    dem = _dem_random(shape, seed)
    return [Field("uniform%d" % c, dem, np.full(shape, c, np.uint8), river) for c in D8.tolist()]


def _descending(shape, seed, tilt=0.5):
    """(dem, fdr): each cell points to a uniformly chosen neighbour that is lower on rng.random() - tilt * (y + x / 2),
    or gets code 0 if none is.  Acyclic by construction, all 8 directions in use."""
    H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = rng.random(shape) - tilt * (yy + 0.5 * xx)
    pad = np.full((H + 2, W + 2), np.inf)
    pad[1:-1, 1:-1] = z
    key = np.empty((8, H, W))
    for k, c in enumerate(D8.tolist()):
        dy, dx = DELTA[c]
        lower = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] < z
        key[k] = np.where(lower, rng.random(shape), -1.0)
    best = key.argmax(axis=0)
    fdr = np.where(key.max(axis=0) >= 0, D8[best], 0).astype(np.uint8)
    # the heights as a DEM: shifted above the nodata sentinel (z goes far below -100)
    return (z + tilt * 1.5 * (H + W) + 10.0).astype(np.float32), fdr


def descending(shape, seed=1):
    dem, fdr = _descending(shape, seed)
    thr = 300 if min(shape) > 1 else 3
    return [Field("descending", dem, fdr, _river_from_acc(fdr, thr))]


def _rect_cycle(y0, x0, h, w):
    """the 2 (h + w) - 4 cells of a rectangle's outline, clockwise from its top-left corner, closed on itself"""
    top = [(y0, x) for x in range(x0, x0 + w)]
    right = [(y, x0 + w - 1) for y in range(y0 + 1, y0 + h)]
    bottom = [(y0 + h - 1, x) for x in range(x0 + w - 2, x0 - 1, -1)]
    left = [(y, x0) for y in range(y0 + h - 2, y0, -1)]
    return top + right + bottom + left


def planted(shape, seed=2):
    """a descending field with planted defects: a 2-cycle, a 4-cycle around the four-tile corner (64, 64), a 40-cell
    cycle inside tile (1, 2), a 300-cell rectangular cycle through the four tiles around (192, 256), 1 % non-D8 codes"""
    H, W = shape
    assert H >= 230 and W >= 300
    dem, fdr = _descending(shape, seed)
    rng = np.random.default_rng(seed + 77)
    bad = rng.random(shape) < 0.01
    fdr[bad] = NON_D8[rng.integers(0, 3, size=int(bad.sum()))]
    fdr[10, 10], fdr[10, 11] = 1, 16
    fdr[63, 63], fdr[63, 64], fdr[64, 64], fdr[64, 63] = 1, 4, 16, 64
    for cyc in (_rect_cycle(84, 148, 11, 11), _rect_cycle(157, 215, 70, 82)):
        put_path(fdr, cyc + [cyc[0]], 0)
        y, x = cyc[0]
        fdr[y, x] = 1
    assert len(_rect_cycle(84, 148, 11, 11)) == 40 and len(_rect_cycle(157, 215, 70, 82)) == 300
    return [Field("planted", dem, fdr, _river_from_acc(fdr, 300))]


def random_codes(shape, seed=3):
    """each cell draws uniformly from the 8 codes plus 0, 3 and 255: in-tile cycles everywhere, the 64-bit tile
    solve's family"""
    rng = np.random.default_rng(seed)
    fdr = np.concatenate([D8, NON_D8])[rng.integers(0, 11, size=shape)]
    river = (rng.random(shape) < 0.02).astype(np.int8)
    return [Field("random_codes", _dem_random(shape, seed), fdr, river)]


def _rev_tile_path(nc, nd):
    """Cells of a path inside a 64 x 64 tile (local coordinates, columns 4..63 only) given BACKWARDS from its end
    (0, 63): first `nd` diagonal moves as zigzags along row pairs -- NE/SE towards the east, NW/SW towards the west,
    alternating, joined by single N steps -- then cardinal moves as a boustrophedon, so that the whole path has
    exactly `nc` cardinal moves (the joins included) and `nd` diagonal ones."""
    lo, hi = 4, TILE - 1
    cells = [(0, hi)]
    y, x, d, r, c, g = 0, hi, -1, 0, 0, 0  # r: upper row of the current pair; c / g: cardinal / diagonal moves made
    while g < nd:
        if lo <= x + d <= hi:
            y, x = (r + 1 if y == r else r), x + d
            g += 1
        else:  # at the wall, on the pair's lower row: up into the next pair
            assert y == r + 1
            r += 2
            y, d = r, -d
            c += 1
        cells.append((y, x))
    assert c <= nc
    if nc > c:
        if nd:  # leave the zigzag's row pair
            while y < r + 2 and c < nc:
                y += 1
                c += 1
                cells.append((y, x))
            d = -1 if x > (lo + hi) // 2 else 1
        while c < nc:
            if lo <= x + d <= hi:
                x += d
            else:
                y, d = y + 1, -d
            c += 1
            cells.append((y, x))
    assert y < TILE and len(set(cells)) == len(cells)
    return cells


COUNT_EDGES = ((255, 0), (256, 0), (4, 255), (4, 256), (200, 200))


def count_edges(shape, seed=0):
    """One tile-local path per tile with exactly the in-tile counts of COUNT_EDGES (cardinal, diagonal) at its head:
    255 and 256 moves of either kind and 200 + 200.  (A diagonal run changes row pairs by one cardinal step, so the
    diagonal paths carry 4 cardinal moves as well.)  One set ends on a river cell of its tile, a second set leaves
    its tile eastwards from (0, 63) with the river 3 moves on.  seed 0 gives the interior tiles to the paths that
    leave, seed 1 to those that end in their tile."""
    H, W = shape
    fdr = np.zeros(shape, np.uint8)
    river = np.zeros(shape, np.int8)
    ty, tx = -(-H // TILE), -(-W // TILE)
    full = [(a, b) for a in range(H // TILE) for b in range(W // TILE)]
    interior = lambda t: 0 < t[0] < ty - 1 and 0 < t[1] < tx - 1
    can_exit = [t for t in full if (t[1] + 1) * TILE + 3 <= W]
    take_first = sorted(can_exit, key=lambda t: (not interior(t), t))[:len(COUNT_EDGES)] if seed % 2 == 0 else None
    if take_first is None:
        stay = sorted(full, key=lambda t: (not interior(t), t))[:len(COUNT_EDGES)]
        leave = [t for t in can_exit if t not in stay][:len(COUNT_EDGES)]
    else:
        leave = take_first
        stay = sorted([t for t in full if t not in leave], key=lambda t: (not interior(t), t))[:len(COUNT_EDGES)]
    assert len(leave) == len(stay) == len(COUNT_EDGES)
    plan = {}
    for tiles, leaves in ((leave, True), (stay, False)):
        for (a, b), (nc, nd) in zip(tiles, COUNT_EDGES):
            y0, x0 = a * TILE, b * TILE
            cells = [(y0 + y, x0 + x) for y, x in reversed(_rev_tile_path(nc, nd))]
            if leaves:
                cells += [(y0, x0 + TILE), (y0, x0 + TILE + 1), (y0, x0 + TILE + 2)]
            put_path(fdr, cells, 1)
            river[cells[-1]] = 1
            plan[(a, b)] = (nc, nd, leaves, cells[0])
    f = Field("count_edges%d" % (seed % 2), _dem_random(shape, seed), fdr, river)
    return [f], plan


# hop_dense: every move (members a, c, d) or every other move (b) crosses a tile border, so the perimeter-node chain
# is as long as the path.  The rasters are the smallest that hold a 20000-hop chain.
HOP_SHAPE = (128, 20224)


def _zigzag(x0, n):
    """n diagonal moves eastwards over the border between rows 63 and 64, from (63, x0)"""
    k = np.arange(n + 1)
    return list(zip((63 + (k & 1)).tolist(), (x0 + k).tolist()))


def _path_dem(shape, cells, step=6.0):
    """heights that fall by `step` along a path (1.0 elsewhere): exact in float32, and any walk that needs a drop
    finds it in one move"""
    dem = np.ones(shape, np.float32)
    c = np.asarray(cells)
    dem[c[:, 0], c[:, 1]] = 1.0 + step * np.arange(len(cells) - 1, -1, -1)
    return dem


def _orient(f, flip_axis, transpose):
    """the member in its second orientation (the flow reversed relative to the tile order) and / or transposed"""
    dem, fdr, river = f.dem, f.fdr, f.river
    lut = np.arange(256, dtype=np.uint8)
    if flip_axis is not None:
        dem, fdr, river = (np.flip(a, axis=flip_axis) for a in (dem, fdr, river))
        for c, (dy, dx) in DELTA.items():
            lut[c] = CODE_OF[(-dy, dx) if flip_axis == 0 else (dy, -dx)]
        fdr = lut[fdr]
    if transpose:
        lut = np.arange(256, dtype=np.uint8)
        for c, (dy, dx) in DELTA.items():
            lut[c] = CODE_OF[(dx, dy)]
        dem, fdr, river = dem.T, lut[fdr.T], river.T
    return Field(f.name, np.ascontiguousarray(dem), np.ascontiguousarray(fdr), np.ascontiguousarray(river))


def hop_a(moves=20100, flipped=False, river=True):
    """(a) a diagonal zigzag of `moves` moves over the border between rows 63 and 64 of a 128 x 20224 raster, river on
    its last cell (river=False: no river at all -- the chain test derives one from the accumulation)"""
    cells = _zigzag(50, moves)
    fdr = from_path(HOP_SHAPE, cells, 1)
    riv = np.zeros(HOP_SHAPE, np.int8)
    if river:
        riv[cells[-1]] = 1
    f = Field("hop_a%d%s" % (moves, "_w" if flipped else "_e"), _path_dem(HOP_SHAPE, cells), fdr, riv)
    return _orient(f, 1 if flipped else None, False)


def hop_b(moves=20100, flipped=False):
    """(b) the cardinal analogue over the border between columns 63 and 64 of a 20224 x 128 raster: E, S, W, S, ...;
    every other move is a hop"""
    k = np.arange(moves + 1)
    # cell k: row 50 + k // 2; column 63, 64, 64, 63, 63, 64, ... (period 4: E, S, W, S)
    ys, xs = 50 + k // 2, 63 + np.array([0, 1, 1, 0])[k % 4]
    cells = list(zip(ys.tolist(), xs.tolist()))
    shape = (HOP_SHAPE[1], HOP_SHAPE[0])
    fdr = from_path(shape, cells, 4)
    riv = np.zeros(shape, np.int8)
    riv[cells[-1]] = 1
    f = Field("hop_b%s" % ("_n" if flipped else "_s"), _path_dem(shape, cells), fdr, riv)
    return _orient(f, 0 if flipped else None, False)


def _closed_zigzag(x0, m):
    """a cycle of 2 m + 2 moves (m odd), every one across the border between rows 63 and 64: m diagonal moves
    eastwards from (63, x0), one step north, m diagonal moves westwards on the cells the way out left free, one step
    north"""
    assert m % 2 == 1
    out = _zigzag(x0, m)                                   # ends on (64, x0 + m)
    k = np.arange(m + 1)
    back = list(zip((63 + (k & 1)).tolist(), (x0 + m - k).tolist()))  # (63, x0 + m) ... (64, x0)
    return out + back


def hop_c(flipped=False):
    """(c) two cycles across tiles made of the same zigzag closed on itself, of 15000 and of 25000 moves, each with
    a tributary: all of it -100.  A short path to a river cell elsewhere keeps the answer from being one constant."""
    fdr = np.zeros(HOP_SHAPE, np.uint8)
    for x0, total in ((8, 15000), (7600, 25000)):
        cyc = _closed_zigzag(x0, (total - 2) // 2)
        assert len(cyc) == total
        put_path(fdr, cyc + [cyc[0]], 0)
        fdr[cyc[0]] = 2
        put_path(fdr, [(57, x0 + 400), (58, x0 + 400), (59, x0 + 401), (60, x0 + 401), (61, x0 + 400),
                       (62, x0 + 400), (63, x0 + 400)], fdr[63, x0 + 400])
    put_path(fdr, [(10, x) for x in range(100, 140)], 1)
    riv = np.zeros(HOP_SHAPE, np.int8)
    riv[10, 139] = 1
    f = Field("hop_c%s" % ("_w" if flipped else "_e"), _dem_random(HOP_SHAPE, 5), fdr, riv)
    return _orient(f, 1 if flipped else None, False)


def hop_d(moves, flipped=False):
    """(d) member (a) with `moves` moves and a 250-cell cardinal feeder inside one tile that joins it 100 moves below
    its head: the cells of the feeder lie 19891 + ... moves from the river, so the cap falls inside the feeder, where
    the last tile pass adds the in-tile part to the node's."""
    cells = _zigzag(50, moves)
    fdr = from_path(HOP_SHAPE, cells, 1)
    jy, jx = cells[100]
    assert jy == 63
    tx0 = jx // TILE * TILE
    feeder, y, x, d = [], 62, jx, -1
    while len(feeder) < 250:  # backwards from (62, jx): a boustrophedon up the tile
        feeder.append((y, x))
        if tx0 <= x + d < tx0 + TILE:
            x += d
        else:
            y, d = y - 1, -d
    put_path(fdr, feeder[::-1] + [(jy, jx)], fdr[jy, jx])
    riv = np.zeros(HOP_SHAPE, np.int8)
    riv[cells[-1]] = 1
    dem = _path_dem(HOP_SHAPE, cells)
    f = Field("hop_d%d%s" % (moves, "_w" if flipped else "_e"), dem, fdr, riv)
    return _orient(f, 1 if flipped else None, False)


def hop_dense():
    """all members in both flow orientations (the node doubling is in place: the launch order relative to the flow
    matters)"""
    out = []
    for fl in (False, True):
        out += [hop_a(flipped=fl), hop_b(flipped=fl), hop_c(flipped=fl), hop_d(19990, fl), hop_d(20010, fl)]
    return out


def cap_mixed(shape=(512, 512), seed=4):
    """one snake through the raster whose moves alternate E, SE, E, NE (W, SW, W, NW on the way back), bands three
    rows apart joined by two S steps; a river cell every 20403 moves, so that cells at 19999, 20000 and 20001 moves
    exist several times over, at different places in their tiles"""
    H, W = shape
    cells = []
    for band in range((H - 1) // 3):
        r = 3 * band
        o = np.arange(W)
        rows = r + ((o // 2) & 1)
        cols = W - 1 - o if band % 2 else o
        cells += list(zip(rows.tolist(), cols.tolist()))
        cells.append((r + 2, int(cols[-1])))
    fdr = from_path(shape, cells, 1)
    river = np.zeros(shape, np.int8)
    for i in list(range(20403, len(cells), 20403)) + [len(cells) - 1]:
        river[cells[i]] = 1
    return [Field("cap_mixed", _dem_random(shape, seed), fdr, river)]


def river_quirks(shape, seed=6):
    """a descending field and the river mask's quirks: mask values 2, -1 and 127 (not river), river cells with code 0
    (dead: arriving on one kills the path) on tile-perimeter and tile-corner cells that other tiles drain into, river
    on the raster's four corners only, an all-river mask, an all-zero mask"""
    H, W = shape
    dem, fdr = _descending(shape, seed)
    base = _river_from_acc(fdr, 300)
    rng = np.random.default_rng(seed + 5)
    odd = base.copy()
    pick = np.flatnonzero(base.ravel() == 1)
    pick = pick[rng.random(pick.size) < 0.4]
    odd.ravel()[pick] = np.array([2, -1, 127], np.int8)[rng.integers(0, 3, size=pick.size)]
    # cells that a step from another tile lands on
    ok, nxt, _, ny, nx = _successor(fdr)
    yy, xx = np.mgrid[0:H, 0:W]
    cross = ok & ((ny // TILE != yy // TILE) | (nx // TILE != xx // TILE))
    entered = np.unique(nxt[cross])
    ey, ex = np.divmod(entered, W)
    corner = ((ey % TILE == 0) | (ey % TILE == TILE - 1)) & ((ex % TILE == 0) | (ex % TILE == TILE - 1))
    chosen = np.concatenate([entered[corner], entered[~corner][rng.random(int((~corner).sum())) < 0.1]])
    dead_f, dead_r = fdr.copy(), base.copy()
    dead_f.ravel()[chosen] = 0
    dead_r.ravel()[chosen] = 1
    corners = np.zeros(shape, np.int8)
    corners[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 1
    return [Field("quirk_values", dem, fdr, odd), Field("quirk_dead_river", dem, dead_f, dead_r),
            Field("quirk_corners", dem, fdr, corners), Field("quirk_all_river", dem, fdr, np.ones(shape, np.int8)),
            Field("quirk_no_river", dem, fdr, np.zeros(shape, np.int8))]


# ---------------------------------------------------------------------------------------------------------
# the cases the two test files share, built once per process
# ---------------------------------------------------------------------------------------------------------
BIG = ((256, 320), (250, 300))   # four interior tiles; ragged last tile row and column
THIN = ((1, 300), (300, 1))
PX = 10.0


@functools.lru_cache(maxsize=None)
def small_fields():
    """name -> Field for every family at its small shapes (hop_dense is separate: hop_fields)"""
    out = {}

    def add(fields, shape):
        for f in fields:
            out["%s-%dx%d" % (f.name, shape[0], shape[1])] = f
    for shape in BIG + THIN:
        add(uniform(shape), shape)
        add(descending(shape), shape)
    for shape in BIG:
        add(planted(shape), shape)
        add(random_codes(shape), shape)
        add(count_edges(shape, 0)[0], shape)
        add(count_edges(shape, 1)[0], shape)
        add(river_quirks(shape), shape)
    add(cap_mixed(), (512, 512))
    return out


def small_names(families=None, shapes=BIG + THIN + ((512, 512),)):
    """the names small_fields() gives, without building anything (for parametrize); optionally only the fields whose
    name starts with one of `families` and / or of the given shapes"""
    out = []
    for shape in BIG + THIN:
        out += ["uniform%d" % c for c in D8.tolist()] + ["descending"]
        if shape in BIG:
            out += ["planted", "random_codes", "count_edges0", "count_edges1", "quirk_values", "quirk_dead_river",
                    "quirk_corners", "quirk_all_river", "quirk_no_river"]
        out = [n if "-" in n else "%s-%dx%d" % (n, shape[0], shape[1]) for n in out]
    out.append("cap_mixed-512x512")
    keep = ["-%dx%d" % s for s in shapes]
    return [n for n in out if n.endswith(tuple(keep)) and (families is None or n.startswith(tuple(families)))]


@functools.lru_cache(maxsize=None)
def hop_fields():
    return {f.name: f for f in hop_dense()}


HOP_NAMES = ["hop_a20100_e", "hop_b_s", "hop_c_e", "hop_d19990_e", "hop_d20010_e",
             "hop_a20100_w", "hop_b_n", "hop_c_w", "hop_d19990_w", "hop_d20010_w"]


def field(name):
    return hop_fields()[name] if name.startswith("hop_") else small_fields()[name]


@functools.lru_cache(maxsize=None)
def answer(name):
    """expected() of a named field, computed once and shared (read-only) by the tests"""
    f = field(name)
    e = expected(f.dem, f.fdr, f.river, PX)
    for a in e.values():
        a.setflags(write=False)
    return e
