"""The label rasters of the polygonisation tests (tests/test_polygonize_host.py, tests/test_gpu_polygonize.py).  They are
70 x 130 unless stated, so that nothing is a multiple of 64 and the 64-cell steps of the west walk and the 256- and
1024-item blocks of the scans are crossed.  Negative values are background."""
import functools

import numpy as np

SHAPE = (70, 130)


def _block(a, r0, r1, c0, c1, v):
    a[r0:r1, c0:c1] = v
    return a


def spiral(H, W):
    """a one-cell-wide spiral of 1 on -1, walked inwards from the top left corner: one 4-connected region, one ring"""
    a = np.full((H, W), -1, np.int32)
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    i = j = d = 0
    a[0, 0] = 1
    while True:
        for _ in range(2):
            di, dj = step[d]
            ni, nj, ai, aj = i + di, j + dj, i + 2 * di, j + 2 * dj
            if 0 <= ni < H and 0 <= nj < W and a[ni, nj] < 0 and not (0 <= ai < H and 0 <= aj < W and a[ai, aj] == 1):
                i, j = ni, nj
                a[i, j] = 1
                break
            d = (d + 1) % 4
        else:
            return a


@functools.lru_cache(maxsize=None)
def cases():
    """{name: label raster}; the arrays are shared and read-only"""
    H, W = SHAPE
    rng = np.random.default_rng(5)
    out = {}
    out["1x1"] = np.array([[5]], np.int32)
    out["1x200"] = rng.integers(0, 3, (1, 200)).astype(np.int32)
    out["200x1"] = rng.integers(-1, 2, (200, 1)).astype(np.int64)
    out["all background"] = np.full(SHAPE, -1, np.int32)
    out["one label"] = np.full(SHAPE, 7, np.int16)
    yy, xx = np.mgrid[0:H, 0:W]
    out["checkerboard"] = ((yy + xx) % 2 + 1).astype(np.uint8)
    out["diagonal pair"] = np.array([[3, -1], [-1, 3]], np.int32)
    out["diagonal pair of two labels"] = np.array([[3, 4], [4, 3]], np.int32)
    # a region whose ring passes one vertex twice: 3 x 3 without its corner and without its centre
    out["pinched"] = np.array([[-1, 1, 1], [1, -1, 1], [1, 1, 1]], np.int32)
    # an island in a hole in an island in a hole; the innermost island carries another label
    a = np.full(SHAPE, -1, np.int32)
    _block(a, 3, 67, 5, 125, 1)
    _block(a, 10, 60, 15, 115, -1)
    _block(a, 17, 53, 25, 105, 1)
    _block(a, 24, 46, 35, 95, -1)
    _block(a, 30, 40, 45, 85, 2)
    out["nested"] = a
    # holes side by side whose tops descend from west to east: the walk from each meets the one before it and inherits
    a = np.full(SHAPE, 1, np.int32)
    _block(a, 20, 40, 20, 30, -1)
    _block(a, 30, 40, 40, 50, -1)
    _block(a, 35, 40, 60, 70, 4)
    _block(a, 38, 40, 100, 129, -1)
    _block(a, 39, 40, 90, 95, -1)      # two holes inherit through the third
    out["holes in a row"] = a
    # walks of more than 64 and more than 128 cells, to the border, to another label and to an earlier hole
    a = np.full((40, 300), 1, np.int32)
    _block(a, 5, 8, 200, 204, -1)      # 200 cells to the border
    _block(a, 12, 15, 100, 104, -1)    # 100 cells to the border
    _block(a, 20, 23, 250, 254, -1)    # 239 cells to the label-2 bar below
    _block(a, 17, 23, 10, 11, 2)
    _block(a, 30, 33, 280, 284, -1)    # 129 cells to the hole below
    _block(a, 25, 33, 150, 151, -1)
    out["long walks"] = a
    # a hole of label 1 filled by label 2: the hole and the shell of label 2 start at one vertex
    a = np.full(SHAPE, -1, np.int32)
    _block(a, 5, 60, 5, 120, 1)
    _block(a, 20, 40, 30, 90, 2)
    _block(a, 25, 30, 40, 50, 1)       # and label 1 again inside label 2
    out["tie"] = a
    out["spiral 65x67"] = spiral(65, 67)
    # a one-cell-wide diagonal staircase: a ring that turns at every edge
    a = np.full(SHAPE, -1, np.int32)
    k = np.arange(69)
    a[k, k + 20] = 6
    a[k + 1, k + 20] = 6
    out["staircase"] = a
    a = rng.integers(0, 3, SHAPE).astype(np.int64)
    a[a == 1] = 2 ** 30
    a[10:20, 30:60] = -7
    a[40:45, :] = -(2 ** 40)
    a[50:, 100:] = 0
    out["extreme labels"] = a
    out["noise of 8 labels"] = rng.integers(0, 8, SHAPE).astype(np.int32)
    out["noise with background"] = rng.integers(-2, 3, SHAPE).astype(np.int8)
    out["1x5000 strip"] = (np.arange(5000) % 2).astype(np.int32).reshape(1, 5000)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def terrain():
    """600 x 900, smooth and realistic: oracle.synth_dem thresholded against its own 31 x 31 mean into four classes of
    local relief, the lowest one background -- valley floors, slopes and ridges, about 1,900 rings of which 400 are holes.
    (The DEM itself is one long slope: its height classes are three bands without a hole.)"""
    import oracle
    dem = np.asarray(oracle.synth_dem(3, 600, 900), np.float64)
    k = 15
    c = np.pad(np.cumsum(np.cumsum(np.pad(dem, k, mode="edge"), 0), 1), ((1, 0), (1, 0)))
    n = 2 * k + 1
    relief = dem - (c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]) / (n * n)
    lab = (np.searchsorted(np.quantile(relief, [0.25, 0.5, 0.75]), relief) - 1).astype(np.int32)
    lab.setflags(write=False)
    return lab


def masks():
    """(name, raster, background): masks, where 0 is background by request"""
    H, W = SHAPE
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (yy - 35) ** 2 + (xx - 60) ** 2 < 900
    ring = disc & ~((yy - 35) ** 2 + (xx - 60) ** 2 < 200)
    return [("bool ring", ring, 0), ("uint8 disc", disc.astype(np.uint8), 0),
            ("label 3 as background", cases()["noise of 8 labels"], 3)]
