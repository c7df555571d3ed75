"""Every pixel-size-dependent GPU path at pixel sizes whose products are not exact.

The rest of the suite runs at px = 10, 12.5 and 1 (3 in one watershed test) and at the default exponents, where
px * k, 100 / px and the sequential sum of k cardinal moves are exact in float64: there the rounding arguments of the
fast paths (the count form of a downslope walk's length in ds_quotient, the product form of the slope in
sd_slope_fast, the |result| >= 0.25 switch of the logarithms) never have to be right.  This module runs them at
px = 30, 0.1, 1/3, 30.922080775909325 and 2500 and at three parameter sets beside the default one (PARAM_SETS), on
inputs that NEED the exact paths.  That they need them is proven on the CPU with numpy and the oracle alone
(the tests of this module without the gpu mark); the GPU tests then hold every path to the oracle on the same inputs.

THE CONTRAST THAT IS THE POINT OF THE MODULE.  dem_long_walks() gives walks of 1000 - 5000 moves whose drops keep
all 24 bits of a float32 (heights inside (-8, 8) m).  At px = 10 the reference's move-by-move sum of n cardinal moves
is px * n exactly, and float32(drop / count form) differs from the reference on NO cell of the cardinal-only lanes;
at px = 0.1 and 1/3 the two path lengths drift hundreds of float64 ulps apart and the count form rounds to another
float32 on hundreds of cells (below), all of them walks of 2^j or 3 * 2^j moves, where drop / (px * n) lies next to a
float32 rounding midpoint.  A kernel that kept the count form there would pass everything else in the suite.

Measured on the CPU (the conditions the non-GPU tests of this module assert):

  long-walk raster, 38 x 5120 (194560 cells), dz = 5: path cells of the lanes whose count-form float32 is not the oracle's
      px 0.1: 287    px 1/3: 147    (all of them on cardinal-only lanes)    px 10, 30, 30.92..., 2500: 0
      59539 walks of 1000 - 4900 moves, 20796 with more than 300 diagonal moves, 200 walks that end at the cap of 5000
      moves, every lane ends on the raster's edge or (lanes that would fall below -7.9 m, and one flat lane) on nodata
  slope, product form against the literal fl(fl(d / dist) * 100) over every float32 drop of one binade (2^23 values;
  both forms scale exactly with 2^k, so one binade stands for every normal drop -- the bounded offline scan):
      px 30 cardinal: 34952 drops differ, each an exact tie of the product form; px 30 diagonal: none
      px 0.1, 1/3, 30.92..., 2500, cardinal and diagonal: none -- NOTHING FOUND there, px 30 carries that class.
      params_scan.npz keeps per pixel size and class the eight drops that agree but lie nearest a rounding midpoint
      (float64 ulps from it: 0 = ties at px 30, 0.1, 1/3 cardinal; 22 at px 30.92 cardinal; 88 / 24 / 9 / 66 / 1
      diagonal at px 30 / 0.1 / 1/3 / 30.92 / 2500): planted too
  planted raster (128 x 256): 12 cells where product form and oracle differ at px 30 (cardinal neighbour), the same 12
      drops to a diagonal neighbour (they cannot differ, see above), 32 near-miss cells, and for dz = 5, 0.3, 0.1 and
      0.7 a walk whose drop is the smallest float32 >= dz (1 move) and one whose drop is the float32 below it (2 moves;
      for 0.7 that is float32(dz) itself, which only the double comparison sends on);
      cells inside the kernel's midpoint window: 52 (px 30), 16 (0.1), 18 (1/3), 0 (30.92...), 2 (2500)
  steep variant of the planted raster at px 1/3 (test_ti_next_to_the_pole): 618 cells of 6000 - 14000 % slope, 40 of
      them with a finite TI (beyond 10000 % the tangent is negative and TI is NaN), on which one float32 ulp of the
      angle moves TI by up to 4.8e-4
  index raster (448 x 640, relief scaled with px), values with |v| < 0.25 / >= 0.25 over TI, MTI, GFI and ln(hl/H)
  together, then the values inside per index (INDEX_CASES; nodata excluded):
      px 0.1  default    52168 / 1041334    ti 10065   mti  8877   gfi 29885   lnhlh  3341
      px 1/3  unit_n     72978 / 1020524    ti 29056   mti 29056   gfi  9646   lnhlh  5220
      px 0.1  big_b      54714 / 1038788    ti 10065   mti  8877   gfi   961   lnhlh 34811
      px 1/3  dz_0.1    129237 /  964265    ti 29056   mti 72769   gfi 25345   lnhlh  2067
      px 30   unit_n     20948 / 1072554    ti     0   mti     0   gfi     0   lnhlh 20948
  (at px >= 30 TI = ln(fac px^2 / tan) >= ln 900 on any terrain; every index has >= 1000 values inside in some case.)

The non-GPU tests of the module take 18 s (the oracle walks the long-walk raster once per pixel size, 3 s each); its 50
GPU tests took 22 s on an MI355X, 12.6 s of them the first 2 x 2 rank case (which also loads torch)."""
import functools
import threading

import numpy as np
import pytest

import oracle
from conftest import assert_float_close, golden

gpu = pytest.mark.gpu

S2 = float(np.sqrt(2.0))
PX_ODD = 30.922080775909325
PXS = (30.0, 0.1, 1.0 / 3.0, PX_ODD, 2500.0)
# (n_top, n_gfi, b, dz): the reference's example, exponents of one, a scale factor >= 1 with a dz float32 cannot hold,
# and another such dz with exponents of their own
PARAM_SETS = {"default": (0.1, 0.4, 0.1, 5.0), "unit_n": (1.0, 1.0, 0.1, 5.0), "big_b": (0.1, 0.4, 1.5, 0.3),
              "dz_0.1": (0.5, 0.25, 0.1, 0.1)}
# every pixel size at the defaults, every other set at two pixel sizes
CASES = [(px, "default") for px in PXS] + [(0.1, "unit_n"), (PX_ODD, "unit_n"), (1.0 / 3.0, "big_b"),
                                            (2500.0, "big_b"), (0.1, "dz_0.1"), (30.0, "dz_0.1")]
INDEX_CASES = [(0.1, "default"), (1.0 / 3.0, "unit_n"), (0.1, "big_b"), (1.0 / 3.0, "dz_0.1"), (30.0, "unit_n")]
# (0.7: its float32 lies BELOW it, so a drop of float32(dz) has to go on -- a float32 comparison would stop there)
DZS = (5.0, 0.3, 0.1, 0.7)
E, SE, NE = 1, 2, 128
# float32 drops (bit patterns in [1, 2)) whose product form d * fl(100 / 30) is an exact float32 tie while the literal
# fl(fl(d / 30) * 100) is not, so that the two round to different float32 values: found by the exhaustive scan of the
# binade (oracle/gen_golden.py params); 0x3EF00015 = 0.46875062584877014 is the first of them times 2^-2
SLOPE_30_BITS = (0x3FF00015, 0x3FF00027, 0x3FF00051, 0x3FF00063)
SLOPE_30_SCALES = (-2, 0, 3)


def case_id(c):
    return "px%.4g-%s" % c


# ---- the DEMs ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dem_long_walks(W=5120, seed=7):
    """-> (dem, lanes).  Lanes that fall eastwards between walls a metre higher, the mean fall per move chosen so that
    dz = 5 is reached after about the given number of moves (+- a few: the steps vary by 20 %): cardinal-only lanes
    (one row, every code E) and lanes that switch between two rows at random (a third of the moves SE / NE).  Two
    "flat" lanes fall 2.4 m in 5000 moves and run into the move cap; the second one ends on nodata.  A lane that would
    fall below -7.9 m ends on nodata too: the heights are multiples of 2^-21 m inside (-8, 8), so the drops of 5 - 8 m
    use all 24 bits of a float32 (only such drops make drop / (px n) land next to float32 midpoints) and are exact,
    whether the difference is taken in float32 or in float64.  The walls' own cells walk into a lane (one S, N or
    diagonal move) and along it.
    lanes: ((r0, r1 or None), y[x] = row of the path in column x, "card" | "zig")."""
    rng = np.random.default_rng(seed)
    card_n = [1024, 1536, 1536, 2048, 3072, 4096, 4096, 1000, 2500, 4900]
    zig_n = [1536, 2900, 4096, 4800]
    spec = sorted([("card", n) for n in card_n] + [("zig", n) for n in zig_n], key=lambda s: s[1])
    spec += [("card", 0), ("zig", 0)]  # sorted: neighbouring lanes stay close in height, so the walls stay low
    rows, path_h, path_y, r = [], [], [], 1
    for kind, n in spec:
        g = 5.0 / (n - 0.5) if n else 2.0 ** -11
        steps = g * (0.8 + 0.4 * rng.random(W))
        h = 7.9 - np.concatenate([[0.0], np.cumsum(steps[:-1])])
        h = np.round(h * 2.0 ** 21) / 2.0 ** 21   # every drop below 8 m is then exact in float32 and in float64
        path_h.append(np.where(h > -7.9, h, -100.0).astype(np.float32))
        if kind == "card":
            rows.append((r, None))
            path_y.append(np.full(W, r))
            r += 2
        else:
            sw = rng.random(W) < 1.0 / 3.0
            sw[0] = False
            path_y.append(r + (np.cumsum(sw) & 1))
            rows.append((r, r + 1))
            r += 3
    H, x, one = r, np.arange(W), np.float32(1.0)
    dem = np.zeros((H, W), np.float32)
    lane_rows = set()
    for k, (r0, r1) in enumerate(rows):
        lane_rows.update([r0] if r1 is None else [r0, r1])
        if r1 is not None:  # the cells of the lane's two rows that are not on the path: a metre above it
            dem[r0] = dem[r1] = np.where(path_h[k] == -100.0, path_h[k], path_h[k] + one)
        dem[path_y[k], x] = path_h[k]
    for y in range(H):  # walls: a metre above the highest cell beside them; nodata where both sides are
        if y in lane_rows:
            continue
        nb = np.full(W, -100.0, np.float32)
        for yy in (y - 1, y + 1):
            if 0 <= yy < H:
                p = np.pad(dem[yy], 1, mode="edge")
                nb = np.maximum(nb, np.maximum(p[1:-1], np.maximum(p[:-2], p[2:])))
        dem[y] = np.where(nb == -100.0, nb, nb + one)
    r0, r1 = rows[-1]
    dem[r0:r1 + 1, W - 40:] = -100.0
    dem.setflags(write=False)
    return dem, tuple((rows[k], path_y[k], spec[k][0]) for k in range(len(spec)))


@functools.lru_cache(maxsize=None)
def dem_ranks():
    """the long-walk raster between two planes that fall southwards (short walks), 128 rows: 2 x 2 ranks of 64 x 2560
    cut through the lanes in both directions"""
    dem, _ = dem_long_walks()
    H, W = dem.shape
    top, bottom = (128 - H) // 2, 128 - H - (128 - H) // 2
    up = 20.0 + 1.5 * np.arange(top, 0, -1, dtype=np.float32)[:, None] + np.zeros((1, W), np.float32)
    down = -20.0 - 1.5 * np.arange(1, bottom + 1, dtype=np.float32)[:, None] + np.zeros((1, W), np.float32)
    out = np.vstack([up, dem, down]).astype(np.float32)
    assert out.shape == (128, W) and out[out != -100.0].min() > -100.0
    out.setflags(write=False)
    return out


def host_walk(dem, fdr, dz, y0, x0):
    """the reference's walk of one cell, move by move (downslope.py:435-532 as dt_oracle.c restates it)
    -> (moves, diagonal moves, float32 drop)"""
    H, W = dem.shape
    step = {1: (0, 1), 2: (1, 1), 4: (1, 0), 8: (1, -1), 16: (0, -1), 32: (-1, -1), 64: (-1, 0), 128: (-1, 1)}
    z0, y, x, n, nd = dem[y0, x0], y0, x0, 0, 0
    for _ in range(5000):
        if not float(np.float32(z0 - dem[y, x])) < dz:
            break
        d = step.get(int(fdr[y, x]))
        if d is None:
            continue
        yy, xx = y + d[0], x + d[1]
        if not (0 <= yy < H and 0 <= xx < W) or dem[yy, xx] == -100.0:
            break
        y, x, n, nd = yy, xx, n + 1, nd + int(d[0] != 0 and d[1] != 0)
    return n, nd, np.float32(z0 - dem[y, x])


def lane_walks(dem, fdr, lanes, dz):
    """The host walk of every PATH cell, lane by lane: the D8 codes must follow the lane (asserted), the heights fall
    along it, so the walk of column x ends at the first column whose float32 drop is >= dz, at the lane's last valid
    column or after 5000 moves.  -> rasters moves, diagonal moves (-1 off the paths) and float32 drop."""
    H, W = dem.shape
    n_r, nd_r = np.full((H, W), -1, np.int64), np.full((H, W), -1, np.int64)
    drop_r = np.zeros((H, W), np.float32)
    for (r0, r1), py, kind in lanes:
        h = dem[py, np.arange(W)]
        last = int(np.flatnonzero(h != -100.0)[-1])
        h, xs = h[:last + 1], np.arange(last + 1)
        diag = (py[1:last + 1] != py[:last]).astype(np.int64)
        code = np.where(diag == 0, E, np.where(py[1:last + 1] > py[:last], SE, NE))
        assert np.array_equal(fdr[py[:last], xs[:last]], code), "the D8 codes must follow the lane"
        assert (np.diff(h) < 0).all()
        cd = np.concatenate([[0], np.cumsum(diag)])
        h64 = -h.astype(np.float64)
        end = np.empty(last + 1, np.int64)
        for x0 in range(last + 1):
            lo = max(int(np.searchsorted(h64, h64[x0] + dz - 1e-3)) - 1, x0)   # a little early, then the float32 test
            while lo < last and float(np.float32(h[x0] - h[lo])) < dz:
                lo += 1
            end[x0] = min(lo, x0 + 5000)
        n_r[py[:last + 1], xs] = end - xs
        nd_r[py[:last + 1], xs] = cd[end] - cd[xs]
        drop_r[py[:last + 1], xs] = h[xs] - h[end]
    return n_r, nd_r, drop_r


def count_form(drop, n, nd, px):
    """float32(drop / (px nc + px sqrt2 nd)): what the fast path computes before its margin test"""
    dist = px * (n - nd).astype(np.float64) + (px * S2) * nd.astype(np.float64)
    with np.errstate(all="ignore"):
        return (drop.astype(np.float64) / dist).astype(np.float32)


def near_miss_drops(px):
    """(cardinal, diagonal): float32 drops in [1, 2) whose product-form slope lies nearest a float32 rounding midpoint,
    from the exhaustive scan stored in tests/golden/params_scan.npz"""
    g = golden("params_scan")
    k = int(np.flatnonzero(g["scan_px"] == px)[0])
    return g["scan_card_bits"][k].view(np.float32), g["scan_diag_bits"][k].view(np.float32)


@functools.lru_cache(maxsize=None)
def dem_planted(px, steep=False):
    """-> (dem 128 x 256, plants): noise 50 m or more above 3 x 5 blocks of one level, in each a cell whose ONLY descent is
    the planted drop.  plants: {"slope30_card" / "slope30_diag": cells whose drop is one of SLOPE_30_BITS * 2^k, to the
    W / SW neighbour; "near_card" / "near_diag": this pixel size's near-miss drops; ("dz", dz, "at" | "below"): start
    cells of a walk E over a cell dz_f32 (or the float32 below it) lower, then one as much lower again (exact drops)}.
    steep: blocks of 50 m under noise of 100 m and the drops unscaled at every px -- at px < 1 hundreds of cells with
    slopes of 6000 - 14000 % (test_ti_next_to_the_pole, px 1/3)."""
    rng = np.random.default_rng(3)
    # The blocks' level: above every planted drop (< 16 m), and at px < 1 so far above that no slope falls between
    # 6000 % and 14000 %: there slope + 0.01 rad comes within a few float32 ulps' reach of pi / 2 and TI hangs on
    # the last bit of the arctangent (beyond, the tangent is negative and TI is NaN for the reference and the build).
    level = np.float32(50.0 if px >= 1.0 or steep else 16.0 + 210.0 * px)
    above = np.float32(50.0 if px >= 1.0 or steep else max(50.0, np.ceil(250.0 * px)))
    dem = (level + above + rng.integers(0, 4, size=(128, 256))).astype(np.float32)
    spots = iter([(y, x) for y in range(4, 124, 6) for x in range(4, 250, 8)])
    plants = {}

    def block():
        y, x = next(spots)
        dem[y - 1:y + 2, x - 2:x + 3] = level
        return y, x
    # (powers of two keep a drop's place between the rounding boundaries; at px < 1 they keep the planted slopes low)
    shift = 0 if steep else min(int(np.floor(np.log2(px))), 0)
    drops30 = [np.ldexp(np.uint32(b).view(np.float32), k + shift) for b in SLOPE_30_BITS for k in SLOPE_30_SCALES]
    nc, nd = (np.ldexp(v, shift) for v in near_miss_drops(px))
    for name, drops, (dy, dx) in (("slope30_card", drops30, (0, -1)), ("slope30_diag", drops30, (1, -1)),
                                  ("near_card", list(nc) + [d * 4 for d in nc], (0, -1)),
                                  ("near_diag", list(nd) + [d * 0.5 for d in nd], (1, -1))):
        for d in drops:
            y, x = block()
            if dy:  # room for the diagonal neighbour inside the block's level
                dem[y + 1:y + 3, x - 2:x + 3] = level
            dem[y, x], dem[y + dy, x + dx] = np.float32(d), 0.0
            plants.setdefault(name, []).append((y, x))
    for dz in DZS:
        dzf = np.float32(dz)
        if float(dzf) < dz:
            dzf = np.nextafter(dzf, np.float32(np.inf))  # the smallest float32 that is not below dz
        for tag, z0 in (("at", dzf), ("below", np.nextafter(dzf, np.float32(0.0)))):
            y, x = block()
            dem[y, x - 1], dem[y, x], dem[y, x + 1] = z0, 0.0, -z0
            plants[("dz", dz, tag)] = (y, x - 1)
    dem.setflags(write=False)
    return dem, plants


@functools.lru_cache(maxsize=None)
def dem_indices(px):
    """448 x 640 of the synthetic terrain (nodata blobs), its relief scaled with the pixel size so that the slopes are
    the same 17 - 96 % at every px: what moves with px is the area term px^2 of the four indices"""
    base = oracle.synth_dem(31, 2048, 2048, 300, 200, 448, 640, 2)
    scale = np.float32(px * 0.8)
    dem = np.where(base == -100.0, base, (base - np.float32(300.0)) * scale).astype(np.float32)
    assert dem[base != -100.0].min() > -100.0
    dem.setflags(write=False)
    return dem


def exact_descents(dem):
    """the cells whose height differences to lower neighbours are exact in float32 (a rise never sets the slope)"""
    H, W = dem.shape
    p = np.pad(dem, 1, mode="edge")
    ok = np.ones((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            nb = p[dy:dy + H, dx:dx + W]
            d64 = dem.astype(np.float64) - nb.astype(np.float64)
            ok &= (d64 <= 0) | ((dem - nb).astype(np.float64) == d64)
    return ok


def product_form(dem, px):
    """-> (q float64, near_mid): the slope as sd_slope_fast forms it (class maxima times 100 / px, 100 / (px sqrt 2)) and
    the cells whose q lies within the kernel's window of 16 float64 ulps around a float32 rounding midpoint"""
    H, W = dem.shape
    with np.errstate(all="ignore"):
        z = np.where(dem == -100.0, np.nan, dem).astype(np.float32)
        p = np.pad(z, 1, constant_values=np.nan)
        c = p[1:-1, 1:-1]
        cb, db = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
        for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
            cb = np.fmax(cb, c - p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        for dy, dx in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
            db = np.fmax(db, c - p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        q = np.fmax(cb.astype(np.float64) * (100.0 / px), db.astype(np.float64) * (100.0 / (px * S2)))
    lo = (q.view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64) - 0x10000000
    return q, (np.abs(lo) <= 16) & (q > 0) & (dem > -100.0)


# ---- the oracle's rasters, computed once per input ------------------------------------------------------------------
def slope_rad(slope):
    """the example's radians: float32 arctangent of the float32 percent / 100, nodata kept (Example/example.py:62-63)"""
    with np.errstate(all="ignore"):
        return np.where(slope == -100.0, np.float32(-100.0), np.arctan(slope / np.float32(100.0)).astype(np.float32))


RAGGED = 6   # columns taken off a raster for the width that is no multiple of 64 (no planted block reaches them)


@functools.lru_cache(maxsize=None)
def oracle_d8(kind, px):
    """(dem, slope, fdr) of the raster `kind`; "<kind>_r": the raster without its last RAGGED columns"""
    if kind.endswith("_r"):
        dem = np.ascontiguousarray(oracle_d8(kind[:-2], px)[0][:, :-RAGGED])
    else:
        dem = {"long": lambda: dem_long_walks()[0], "planted": lambda: dem_planted(px)[0],
               "steep": lambda: dem_planted(px, steep=True)[0],
               "indices": lambda: dem_indices(px), "ranks": dem_ranks}[kind]()
    slope, fdr = oracle.slope_d8(dem, px)
    return dem, slope, fdr


@functools.lru_cache(maxsize=None)
def oracle_down(kind, px, dz):
    dem, _, fdr = oracle_d8(kind, px)
    return oracle.downslope(dem, fdr, px, dz)


@functools.lru_cache(maxsize=8)
def oracle_chain(kind, px, sname, thr=None):
    """every raster of the chain from the oracle; the river threshold is the chain's default N // 512"""
    n_top, n_gfi, b, dz = PARAM_SETS[sname]
    dem, slope, fdr = oracle_d8(kind, px)
    fac = oracle.flowacc(fdr, dem)
    river = (fac > (dem.size // 512 if thr is None else thr)).astype(np.int8)
    fdist, idx, hand = oracle.flowhand(dem, fdr, river, px)
    ti, mti = oracle.twi(fac, slope_rad(slope), px, n_top)
    with np.errstate(all="ignore"):
        out = {"dem": dem, "slope": slope, "fdr": fdr, "fac": fac, "river": river, "fdist": fdist, "idx": idx,
               "hand": hand, "ti": ti, "mti": mti, "gfi": oracle.gfi(hand, fac, idx, n_gfi, b, px),
               "lnhlh": oracle.lnhlh(hand, fac, n_gfi, b, px), "down": oracle_down(kind, px, dz)}
    return out


def index_counts(o):
    """{index: (cells with |value| < 0.25, cells with |value| >= 0.25)}; nodata and non-finite values in neither"""
    res = {}
    for k in ("ti", "mti", "gfi", "lnhlh"):
        v = o[k][(o[k] != -100.0) & np.isfinite(o[k])]
        res[k] = (int((np.abs(v) < 0.25).sum()), int((np.abs(v) >= 0.25).sum()))
    return res


# ---- the CPU proof --------------------------------------------------------------------------------------------------
def divergent_lane_cells(px, dz=5.0):
    """-> (divergent, cardinal rows, n, nd): the path cells of the long-walk raster whose count-form float32 is not the
    oracle's"""
    dem, lanes = dem_long_walks()
    _, _, fdr = oracle_d8("long", px)
    n, nd, drop = lane_walks(dem, fdr, lanes, dz)
    on = n > 0
    bad = on & (count_form(drop, np.maximum(n, 1), np.maximum(nd, 0), px) != oracle_down("long", px, dz))
    card = np.zeros(dem.shape, bool)
    for (r0, r1), _, kind in lanes:
        card[r0] = kind == "card"
    return bad, card, n, nd


def test_long_walks_need_the_sequential_sum():
    dem, lanes = dem_long_walks()
    assert 150_000 < dem.size < 500_000
    for px in (0.1, 1.0 / 3.0):
        bad, card, n, nd = divergent_lane_cells(px)
        print("px %r: %d lane cells where the count form rounds differently (%d on cardinal lanes)"
              % (px, int(bad.sum()), int((bad & card).sum())))
        assert int(bad.sum()) >= 16
        # lane_walks is the host walk: move by move on a few of the cells, the divergent ones first
        _, _, fdr = oracle_d8("long", px)
        ys, xs = np.nonzero(bad)
        drop = lane_walks(dem, fdr, lanes, 5.0)[2]
        for y, x in list(zip(ys[:3], xs[:3])) + [(int(lanes[-1][1][100]), 100), (int(lanes[3][1][4000]), 4000)]:
            assert host_walk(dem, fdr, 5.0, y, x) == (n[y, x], nd[y, x], drop[y, x])
    # the lengths asked for: walks of 1000 - 4900 moves that reach dz, diagonal moves among them, the cap, nodata
    on = n > 0
    assert ((n >= 1000) & (n <= 4900)).sum() > 20_000 and (nd[on] > 300).sum() > 5_000
    assert (n == 5000).sum() >= 100
    ends = [int(np.flatnonzero(dem[py, np.arange(dem.shape[1])] != -100.0)[-1]) for _, py, _ in lanes]
    assert sum(e < dem.shape[1] - 1 for e in ends) >= 1 and ends[-1] == dem.shape[1] - 41
    # THE CONTRAST: at px = 10 the sequential sum of cardinal moves is px * n, and the count form is the reference
    bad, card, _, _ = divergent_lane_cells(10.0)
    assert card.any() and not (bad & card).any()


def test_planted_slopes_need_the_exact_division():
    px = 30.0
    dem, plants = dem_planted(px)
    _, slope, fdr = oracle_d8("planted", px)
    q, near = product_form(dem, px)
    for name, code in (("slope30_card", 16), ("slope30_diag", 8)):
        for y, x in plants[name]:
            assert fdr[y, x] == code, "the planted drop must be the cell's only descent"
    cells = plants["slope30_card"]
    assert len(cells) == len(SLOPE_30_BITS) * len(SLOPE_30_SCALES)
    assert dem[cells[0]] == np.float32(0.46875062584877014)
    for y, x in cells:
        assert np.float32(q[y, x]) != slope[y, x] and near[y, x]
    # the same drops to a diagonal neighbour: no float32 drop makes the two forms differ there (exhaustive scan of
    # the binade, recorded in the golden file), so these only have to agree
    for y, x in plants["slope30_diag"]:
        assert np.float32(q[y, x]) == slope[y, x]
    g = golden("params_scan")
    k30 = int(np.flatnonzero(g["scan_px"] == 30.0)[0])
    assert g["scan_card_mismatches"][k30] > 30000 and g["scan_diag_mismatches"][k30] == 0
    others = np.arange(len(g["scan_px"])) != k30
    assert not g["scan_card_mismatches"][others].any() and not g["scan_diag_mismatches"].any()


@pytest.mark.parametrize("px", PXS)
def test_planted_near_misses_and_dz_boundaries(px):
    dem, plants = dem_planted(px)
    _, slope, fdr = oracle_d8("planted", px)
    q, near = product_form(dem, px)
    valid = dem > -100.0
    assert np.array_equal(q.astype(np.float32)[valid & ~near], slope[valid & ~near])
    assert not ((slope > 6000.0) & (slope < 14000.0)).any(), "TI would hang on the last bit of the arctangent"
    for name, code in (("near_card", 16), ("near_diag", 8)):
        cells = plants[name]
        assert len(cells) == 16 and all(fdr[y, x] == code for y, x in cells)
        # the nearest any drop of this class comes to a midpoint at this px: inside the window or just outside it
        lo = np.array([int(q[y, x].view(np.uint64) & np.uint64(0x1FFFFFFF)) - 0x10000000 for y, x in cells])
        print("px %r %s: distance of the product form from the midpoint, float64 ulps: %s" % (px, name, lo.tolist()))
        assert all(np.float32(q[y, x]) == slope[y, x] for y, x in cells) or px == 30.0
    for dz in DZS:
        dzf = np.float32(dz) if float(np.float32(dz)) >= dz else np.nextafter(np.float32(dz), np.float32(np.inf))
        below = np.nextafter(dzf, np.float32(0.0))
        down = oracle_down("planted", px, dz)
        y, x = plants[("dz", dz, "at")]
        assert host_walk(dem, fdr, dz, y, x) == (1, 0, dzf)          # dz_f32 < dz is false in float64: one move
        assert down[y, x] == np.float32(float(dzf) / px)
        y, x = plants[("dz", dz, "below")]
        assert host_walk(dem, fdr, dz, y, x) == (2, 0, below + below)   # below < dz: the walk goes on
        assert down[y, x] == np.float32(float(below + below) / (px + px))


@pytest.mark.parametrize("case", INDEX_CASES, ids=case_id)
def test_indices_lie_on_both_sides_of_the_switch(case):
    px, sname = case
    c = index_counts(oracle_chain("indices", px, sname))
    inside, outside = sum(v[0] for v in c.values()), sum(v[1] for v in c.values())
    print("px %r %s: %d inside 0.25, %d outside; inside per index %s"
          % (px, sname, inside, outside, {k: v[0] for k, v in c.items()}))
    assert inside >= 1000 and outside >= 1000
    if px < 1.0:   # (TI cannot come near zero at px >= 30: fac px^2 / tan >= 900 / tan)
        assert c["ti"][0] >= 1000 and c["ti"][1] >= 1000
    assert c["gfi"][0] + c["lnhlh"][0] >= 1000


HALF_PI = float(np.pi / 2)


def ti_near_the_pole(kind, px, n_top):
    """TI / MTI where slope + 0.01 rad lies next to pi / 2, and how far a float32 ulp of the angle may move them.

    The reference forms y = float32(arctan(float32 slope / 100)) and TI = ln A - ln tan(y + 0.01).  d/dy ln tan(y + 0.01) =
    1 / (sin cos)(y + 0.01) grows like 1 / (pi/2 - y - 0.01): at 9333 % slope one float32 ulp of y (2^-23) moves TI by
    1.7e-4, seventeen times the 1e-5 contract.  numpy's float32 arctangent is itself only good to a few ulps, differently
    from one CPU to the next, so here the reference angle is the correctly rounded one (the float64 arctangent rounded
    to float32), and the build's angle is allowed ONE float32 ulp u around it (dt_atanf_pos ends in a float64
    multiply-add that is rounded once).  By the mean value theorem the logarithm then moves by at most
    u * max 1 / |sin cos| over [y + 0.01 - u, y + 0.01 + u], which is the value at the end nearer pi / 2.  That is added
    to the contract's 1e-5 |ref| + 1e-6; nothing else is.  Cells within 4 u of the pole, where one ulp decides between a
    huge TI and NaN, are left out (`dropped`; the steep rasters have none).
    -> (ti, mti, tol, band, dropped): reference rasters, the tolerance raster, the cells of 6000 - 14000 % slope"""
    dem, slope, fdr = oracle_d8(kind, px)
    fac = oracle.flowacc(fdr, dem)
    with np.errstate(all="ignore"):
        q = (slope / np.float32(100.0)).astype(np.float64)
        y = np.where(slope == -100.0, np.float32(-100.0), np.arctan(q).astype(np.float32))
        ti, mti = oracle.twi(fac, y, px, n_top)
        u = np.spacing(np.abs(y)).astype(np.float64)
        th = y.astype(np.float64) + 0.01
        near = np.where(th < HALF_PI, th + u, th - u)   # the end of the interval nearer the pole
        move = u / np.abs(np.sin(near) * np.cos(near))
    band = (slope > 6000.0) & (slope < 14000.0)
    dropped = (slope != -100.0) & (np.abs(HALF_PI - th) <= 4 * u)
    tol = {"ti": 1e-5 * np.abs(ti) + 1e-6 + move, "mti": 1e-5 * np.abs(mti) + 1e-6 + move}
    return ti, mti, tol, band, dropped


@pytest.mark.parametrize("px", [1.0 / 3.0])
def test_steep_raster_lies_next_to_the_pole(px):
    ti, mti, tol, band, dropped = ti_near_the_pole("steep", px, 0.1)
    finite = band & np.isfinite(ti)
    print("px %r: %d cells of 6000 - 14000 %% slope, %d with a finite TI, largest allowance for the angle's ulp %.1e"
          % (px, int(band.sum()), int(finite.sum()), float((tol["ti"] - 1e-5 * np.abs(ti) - 1e-6)[finite].max())))
    assert band.sum() >= 100 and finite.sum() >= 30 and not dropped.any()
    # the allowance matters: on some of these cells it is larger than the plain contract
    assert ((tol["ti"] > 2 * (1e-5 * np.abs(ti) + 1e-6)) & finite).sum() >= 4


def test_every_index_is_near_zero_somewhere():
    best = {k: 0 for k in ("ti", "mti", "gfi", "lnhlh")}
    for px, sname in INDEX_CASES:
        for k, v in index_counts(oracle_chain("indices", px, sname)).items():
            best[k] = max(best[k], v[0])
    assert all(v >= 1000 for v in best.values()), best


# ---- the GPU paths against the oracle -------------------------------------------------------------------------------
INT_RASTERS = ("fdr", "fac", "river", "idx")
BIT_RASTERS = ("slope", "hand", "down")
LOG_RASTERS = ("ti", "mti", "gfi", "lnhlh")
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def hold_to_oracle(got, o, what, rasters=INT_RASTERS + BIT_RASTERS + LOG_RASTERS + ("fdist",)):
    """fdr, fac, river, idx, slope, hand and down bit for bit (floats as int32), fdist to 1e-6, the logarithms through
    the project's assert_float_close(1e-5, 1e-6)"""
    for k in rasters:
        g, r = np.asarray(got[k]), o[k]
        if k in INT_RASTERS:
            assert np.array_equal(g.astype(np.int64), r.astype(np.int64)), \
                "%s %s: %d cells differ" % (what, k, int((g.astype(np.int64) != r).sum()))
        elif k in BIT_RASTERS:
            if not same_bits(g, r):
                bad = np.argwhere(np.asarray(g, np.float32).view(np.int32) != r.view(np.int32))
                i = tuple(bad[0])
                raise AssertionError("%s %s: %d cells differ, first at %s: got %r, oracle %r"
                                     % (what, k, len(bad), i, g[i], r[i]))
        elif k == "fdist":
            assert_float_close(g, r, rtol=1e-6, what=what + " fdist")
        else:
            assert_float_close(g, r, rtol=1e-5, atol=1e-6, what="%s %s" % (what, k))


def ragged(kind):
    return kind + "_r"


def run_chain(dem, px, sname, overlap=True, heights="float32", long_walks=False):
    """the chain's step as Chain.run enqueues it (no slope_rad: the plain float32 chain then takes the slope from the D8
    kernel where the width allows it) -> (rasters, whether it did, the cells it marked for the exact recomputation)"""
    from descriptools_amd import chain
    from descriptools_amd.device import Context
    from test_gpu_slope_from_d8 import marked_cells
    n_top, n_gfi, b, dz = PARAM_SETS[sname]
    H, W = dem.shape
    ctx = Context()
    try:
        d = ctx.to_device(np.ascontiguousarray(dem, np.float64 if heights == "float64" else np.float32))
        ch = chain.Chain(H, W, ctx=ctx, px=px, n_top=n_top, n_gfi=n_gfi, b=b, dz=dz, want_slope_rad=False,
                         tune_placement=False, overlap=overlap, heights=heights, long_walks=long_walks)
        new = ch._from_d8()
        ch.run(d.ptr, want_a_river=False)
        ctx.sync()
        ch.check_status()
        out = {k: ch.buf[k].to_host() for k in INT_RASTERS + BIT_RASTERS + LOG_RASTERS + ("fdist",)}
        marks = marked_cells(ch._marks.to_host(), H, W) if new else None
        ch.free()
        d.free()
    finally:
        ctx.close()
    return out, new, marks


def equal_runs(a, b, what):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            x, y = x.astype(np.float32).view(np.int32), y.astype(np.float32).view(np.int32)
        assert np.array_equal(x, y), "%s: %s differs on %d cells" % (what, k, int((x != y).sum()))


def chain_on(kind, px, sname, aligned, must_mark=None):
    """the float32 chain on one raster at one width: overlap on and off, float64 heights on the same values, the host
    convenience -- all equal, and equal to the oracle"""
    from descriptools_amd import chain
    k = kind if aligned else ragged(kind)
    o = oracle_chain(k, px, sname)
    dem = o["dem"]
    assert (dem.shape[1] % 64 == 0) == aligned
    what = "%s px %r %s" % (k, px, sname)
    got, new, marks = run_chain(dem, px, sname, overlap=True)
    assert new == aligned, "slope from the D8 kernel exactly on rows of whole 64-cell tiles"
    hold_to_oracle(got, o, what)
    if aligned and must_mark is not None:
        assert must_mark.any() and marks[must_mark].all(), int((must_mark & ~marks).sum())
    serial, new2, _ = run_chain(dem, px, sname, overlap=False)
    assert new2 == aligned
    equal_runs(got, serial, what + " overlap=False")
    # float64 heights on the same values: the same rasters wherever float32 takes the height differences exactly (else
    # the two tiers differ by design: the float64 one does not round them) -- the codes and what follows from them, and
    # the slope of the cells whose descents are exact, the planted ones among them
    if kind == "planted":
        wide, _, _ = run_chain(dem, px, sname, heights="float64")
        equal_runs({k: got[k] for k in INT_RASTERS + ("fdist",)}, {k: wide[k] for k in INT_RASTERS + ("fdist",)},
                   what + " heights=float64")
        ex = exact_descents(dem)
        assert ex.mean() > 0.8 and same_bits(wide["slope"][ex], got["slope"][ex])
        got["down_f64"] = wide["down"]
    n_top, n_gfi, b, dz = PARAM_SETS[sname]
    host = chain.run_host(dem, px, n_top=n_top, n_gfi=n_gfi, b=b, dz=dz)   # (with slope_rad: the stencil pass)
    hold_to_oracle(host, o, what + " run_host")
    return got


@gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["w64", "ragged"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_chain_on_the_planted_raster(case, aligned):
    px, sname = case
    dem, plants = dem_planted(px)
    must = None
    if aligned:
        # what the product form cannot prove must be in the marks: the window of the rounding test, on the CPU
        must = product_form(dem, px)[1]
        if px == 30.0:
            assert all(must[y, x] for y, x in plants["slope30_card"])
        if not must.any():
            must = None
    got = chain_on("planted", px, sname, aligned, must)
    dz = PARAM_SETS[sname][3]
    o = oracle_down("planted" if aligned else ragged("planted"), px, dz)
    for tag in ("at", "below"):   # (exact drops: the float64 tier must give the same float32 there)
        y, x = plants[("dz", dz, tag)]
        assert got["down"][y, x] == o[y, x] and o[y, x] > 0 and got["down_f64"][y, x] == o[y, x]


@gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["w64", "ragged"])
@pytest.mark.parametrize("px", [1.0 / 3.0], ids=["px1/3"])
def test_ti_next_to_the_pole(px, aligned):
    """The case that failed when this module was first run: slopes of 6000 - 14000 %, where TI / MTI follow the last
    bit of the float32 angle (four cells were 5e-5 off at px 1/3 against a reference angle from numpy's float32
    arctangent).  Kept as it was found, with the bound derived in ti_near_the_pole: the build may be one float32 ulp
    of the angle away from the correctly rounded one, and no further.  Both forms of the step (TI from the
    accumulation pass + fix-up, and the stencil), the host convenience and the drop-in function; everything else on
    the raster by the usual rules."""
    from descriptools_amd import chain, topoindexes
    kind = "steep" if aligned else ragged("steep")
    n_top = PARAM_SETS["default"][0]
    ti, mti, tol, band, dropped = ti_near_the_pole(kind, px, n_top)
    assert band.sum() >= 100 and not dropped.any()
    o = oracle_chain(kind, px, "default")
    dem = o["dem"]
    got, new, _ = run_chain(dem, px, "default")
    assert new == aligned
    host = chain.run_host(dem, px)
    # the device's radians: within one float32 ulp of the correctly rounded arctangent
    with np.errstate(all="ignore"):
        y = np.arctan((o["slope"] / np.float32(100.0)).astype(np.float64)).astype(np.float32)
    valid = o["slope"] != -100.0
    d = np.abs(host["slope_rad"][valid].astype(np.float64) - y[valid])
    print("angle: largest |device - correctly rounded| = %.3g float32 ulps" % float((d / np.spacing(y[valid])).max()))
    assert (d <= np.spacing(y[valid])).all()
    drop_in = dict(zip(("ti", "mti"), topoindexes.topographic_index(o["fac"], y, px, n_top)))
    rest = tuple(k for k in INT_RASTERS + BIT_RASTERS + ("gfi", "lnhlh", "fdist"))
    for what, res in (("chain", got), ("run_host", host), ("topographic_index", drop_in)):
        if what != "topographic_index":
            hold_to_oracle(res, o, "%s %s px %r" % (what, kind, px), rasters=rest)
        for k, ref in (("ti", ti), ("mti", mti)):
            g = np.asarray(res[k], np.float64)
            assert np.array_equal(g == -100.0, ref == -100.0), k
            err = np.abs(g - ref)
            # (the drop-in function is GIVEN the reference angle: the plain contract, no allowance for the angle)
            bound = 1e-5 * np.abs(ref) + 1e-6 if what == "topographic_index" else tol[k]
            ok = (np.isnan(g) & np.isnan(ref)) | (ref == -100.0) | (g == ref) | (err <= bound)
            with np.errstate(all="ignore"):
                worst = float(np.nanmax(np.where(band & np.isfinite(ref), err / bound, 0.0)))
            print("%s %s: largest error / bound in the band %.3f" % (what, k, worst))
            assert ok.all(), "%s %s: %d cells beyond the bound, first %s" % (what, k, int((~ok).sum()),
                                                                            np.argwhere(~ok)[0])


@gpu
@pytest.mark.parametrize("case,aligned", [(c, True) for c in INDEX_CASES] + [(INDEX_CASES[0], False),
                                                                               (INDEX_CASES[3], False)],
                         ids=lambda v: case_id(v) if isinstance(v, tuple) else ("w64" if v else "ragged"))
def test_chain_on_the_index_raster(case, aligned):
    px, sname = case
    chain_on("indices", px, sname, aligned)


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_drop_in_functions(case):
    """the reference's own entry points, one by one, each on the oracle's inputs"""
    from descriptools_amd import downslope, flowdir, flowhand, gfi, slope, topoindexes
    px, sname = case
    n_top, n_gfi, b, dz = PARAM_SETS[sname]
    for kind in ("planted", "indices") if case in INDEX_CASES else ("planted",):
        o = oracle_chain(kind, px, sname)
        dem, what = o["dem"], "%s px %r %s" % (kind, px, sname)
        got = {"slope": slope.sloper(dem, px)}
        fdr, sl = flowdir.d8(dem, px, return_slope=True)
        assert same_bits(sl, o["slope"]), what + ": slope of flowdir.d8"
        got["fdr"] = fdr
        got["fdist"], got["idx"], got["hand"] = flowhand.flow_hand_index(dem, o["fdr"], o["river"], px)
        got["down"] = downslope.downsloper(dem, o["fdr"], px, dz)
        if kind == "planted":   # a dz whose float32 lies below it: float32(dz) has to walk on
            assert same_bits(downslope.downsloper(dem, o["fdr"], px, 0.7), oracle_down(kind, px, 0.7))
        got["ti"], got["mti"] = topoindexes.topographic_index(o["fac"], slope_rad(o["slope"]), px, n_top)
        got["gfi"] = gfi.gfi_calculator(o["hand"], o["fac"], o["idx"], n_gfi, b, px)
        got["lnhlh"] = gfi.ln_hl_H_calculator(o["hand"], o["fac"], n_gfi, b, px)
        hold_to_oracle(got, o, what, rasters=tuple(got))


@gpu
@pytest.mark.parametrize("case", [(PX_ODD, "dz_0.1"), (1.0 / 3.0, "unit_n")], ids=case_id)
def test_float64_dem(case):
    """heights float32 cannot hold (the index raster plus a ripple below its float32 ulp) at inexact pixel sizes: every
    height difference in float64, against the oracle's *_f64 functions"""
    from descriptools_amd import chain
    from test_gpu_chain_f64 import d8_f64_np
    px, sname = case
    n_top, n_gfi, b, dz = PARAM_SETS[sname]
    dem32 = dem_indices(px)
    yy, xx = np.mgrid[0:dem32.shape[0], 0:dem32.shape[1]]
    ripple = px * (1e-4 * np.sin(0.37 * yy + 0.11 * xx) + 1e-7 * np.cos(1.3 * xx))
    dem = np.where(dem32 == -100.0, -100.0, dem32.astype(np.float64) + ripple)
    assert (dem.astype(np.float32).astype(np.float64) != dem).mean() > 0.8
    out = chain.run_host(dem, px, heights="float64", n_top=n_top, n_gfi=n_gfi, b=b, dz=dz)
    fdr = d8_f64_np(dem, px)   # the D8 rule on float64 differences, restated in numpy
    assert np.array_equal(out["fdr"], fdr), "%d codes differ" % int((out["fdr"] != fdr).sum())
    fac = oracle.flowacc(fdr, dem.astype(np.float32))
    assert np.array_equal(out["fac"], fac)
    river = (fac > dem.size // 512).astype(np.int8)
    fdist, idx, _ = oracle.flowhand(dem.astype(np.float32), fdr, river, px)
    assert np.array_equal(out["idx"], idx)
    assert_float_close(out["fdist"], fdist, rtol=1e-6, what="fdist")
    slope = oracle.slope_f64(dem, px)
    assert same_bits(out["slope"], slope)
    hand = oracle.hand_f64(dem, idx)
    assert out["hand"].dtype == np.float64 and np.array_equal(out["hand"], hand)
    assert same_bits(out["down"], oracle.downslope_f64(dem, fdr, px, dz))
    ti, mti = oracle.twi(fac, slope_rad(slope), px, n_top)
    assert_float_close(out["ti"], ti, rtol=1e-5, atol=1e-6, what="ti")
    assert_float_close(out["mti"], mti, rtol=1e-5, atol=1e-6, what="mti")
    assert_float_close(out["gfi"], oracle.gfi_f64h(hand, fac, idx, n_gfi, b, px), rtol=1e-5, atol=1e-6, what="gfi")
    assert_float_close(out["lnhlh"], oracle.lnhlh_f64h(hand, fac, n_gfi, b, px), rtol=1e-5, atol=1e-6, what="lnhlh")


@gpu
@pytest.mark.parametrize("px", [0.1, 1.0 / 3.0], ids=["px0.1", "px1/3"])
def test_long_walks(px):
    """the walks that need the reference's own sum, through every downslope kernel: the window kernel with its
    continuation, the queue + skip tables of long_walks=True, "auto" (run_host), the drop-in function, and the kernels
    on float64 heights, which sum move by move"""
    from descriptools_amd import chain, downslope
    dem, _ = dem_long_walks()
    bad = divergent_lane_cells(px)[0]
    assert int(bad.sum()) >= 16
    _, slope, fdr = oracle_d8("long", px)
    want = oracle_down("long", px, 5.0)
    for long_walks in (False, True):
        got, new, _ = run_chain(dem, px, "default", long_walks=long_walks)
        assert new
        what = "long walks px %r long_walks=%r" % (px, long_walks)
        hold_to_oracle(got, {"fdr": fdr, "slope": slope, "down": want}, what, rasters=("fdr", "slope", "down"))
    host = chain.run_host(dem, px)
    hold_to_oracle(host, {"fdr": fdr, "slope": slope, "down": want}, "run_host", rasters=("fdr", "slope", "down"))
    assert same_bits(downslope.downsloper(dem, fdr, px, 5.0), want)
    wide, _, _ = run_chain(dem, px, "default", heights="float64")
    assert same_bits(wide["down"], want) and same_bits(wide["slope"], slope)
    # another dz on the same raster: shorter walks, other drops
    got, _, _ = run_chain(dem[:, :-RAGGED], px, "big_b", long_walks=True)
    d = np.ascontiguousarray(dem[:, :-RAGGED])
    assert same_bits(got["down"], oracle.downslope(d, oracle.slope_d8(d, px)[1], px, 0.3))


@gpu
@pytest.mark.parametrize("long_walks", [False, True])
def test_long_walks_across_rank_borders(long_walks):
    """2 x 2 ranks of 64 x 2560 over the long-walk raster (dem_ranks) at px 0.1: the lanes cross the border between the
    columns of ranks, so the walks go on as walker records (counts, and the reference's sequential sum for those that
    fail the rounding test); the result is the untiled chain's and the oracle's"""
    import torch
    from descriptools_amd import chain, tiling
    px = 0.1
    dem = dem_ranks()
    Hg, Wg = dem.shape
    assert int(divergent_lane_cells(px)[0][:, :Wg // 2].sum()) >= 16, "divergent walks must start left of the border"
    layout = tiling.Layout([Hg // 2, Hg // 2], [Wg // 2, Wg // 2])
    thr = Hg * Wg // 512
    ref = chain.run_host(dem, px, river_threshold=thr)
    want = oracle_down("ranks", px, 5.0)
    assert same_bits(ref["down"], want)
    h = tiling.HALO
    pad = np.full((Hg + 2 * h, Wg + 2 * h), -100.0, np.float32)
    pad[h:h + Hg, h:h + Wg] = dem
    tiles = []
    for r in range(layout.size):
        tl = tiling.RankTile(layout, r, device=0, px=px, dz=5.0, river_threshold=thr, long_walks=long_walks)
        y0, x0 = layout.origin(r)
        tl.set_dem_ext(pad[y0:y0 + tl.He, x0:x0 + tl.We])
        tiles.append(tl)
    tiling.simulate(tiles, layout)
    marked = sum(tl.unresolved_downslope() for tl in tiles)
    assert marked > 1000, "the lanes are meant to send their walks across the border"
    comms = tiling.LocalComm.create(layout.size)
    done, errors = [None] * layout.size, []

    def work(r):
        try:
            done[r] = tiling.finish_downslope(tiles[r], comms[r])
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append(e)
            comms[r].sh.barrier.abort()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(layout.size)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert all(d == marked for d in done), "every marked walk travels as a walker and comes home"
    for tl in tiles:
        y0, x0 = layout.origin(tl.rank)
        sl = (slice(y0, y0 + tl.H), slice(x0, x0 + tl.W))
        assert tl.unresolved_downslope() == 0
        for name in ("fdr", "fac", "river", "fdist", "hand", "slope", "ti", "mti", "gfi", "lnhlh", "down"):
            g, w = tl.host(name), ref[name][sl]
            assert np.array_equal(g, w.astype(g.dtype), equal_nan=True), \
                "rank %d %s: %d cells differ" % (tl.rank, name, int((g != w).sum()))
        assert np.array_equal(tl.host("idx"), ref["idx"][sl])
        assert same_bits(tl.host("down"), want[sl])
        tl.free()
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("px", [PX_ODD, 1.0 / 3.0], ids=["px30.92", "px1/3"])
def test_watershed_and_reaches(px):
    """the px * count lengths of drainage / upslope_length and of the reaches' channels, and the px^2 areas of the
    stage tables, against their numpy references"""
    from test_gpu_reaches import check_network
    from test_gpu_watershed import check as check_watershed
    dem = np.ascontiguousarray(dem_indices(px)[100:292, 200:520])
    slope, fdr = oracle.slope_d8(dem, px)
    check_watershed(fdr, px, dem)
    fac = oracle.flowacc(fdr, dem)
    river = (fac > 150).astype(np.int8)
    stages = np.arange(1, 9) * (0.4 * px)
    assert check_network(fdr, river, dem, px, stages, slope=slope) > 4
