"""The geometry cases that tests/test_gpu_vector.py rasterises and tests/test_vector_host.py counts: name -> (kind,
coords float64[N, 2], parts int64[P + 1], ids int32[P], shape).  Built once (functools.lru_cache) and read-only."""
import functools

import numpy as np

SHAPE = (70, 130)   # more than one wave of columns, rows that differ, clipped and unclipped spans


def geom(kind, runs, ids, shape=SHAPE):
    """arrays from a list of vertex lists"""
    coords = np.array([v for r in runs for v in r], np.float64).reshape(-1, 2)
    parts = np.cumsum([0] + [len(r) for r in runs]).astype(np.int64)
    out = (kind, coords, parts, np.array(ids, np.int32), shape)
    for a in out[1:4]:
        a.setflags(write=False)
    return out


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


TRIANGLE = [(10.3, 5.2), (100.7, 20.1), (40.2, 60.9)]
CONCAVE = [(8.2, 6.1), (120.4, 9.3), (118.9, 62.2), (90.1, 30.7), (64.6, 66.3), (40.2, 25.5), (12.8, 64.4)]


def tessellation(seed=3):
    """60 triangles that tile the rectangle [7.3, 121.6) x [4.2, 64.7): a 7 x 6 lattice of points, the interior ones
    jittered, the ones on the rim moved along it, each quad cut by a random diagonal.  -> (rings, rectangle)"""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = 7.3, 4.2, 121.6, 64.7
    nx, ny = 7, 6
    gx, gy = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
    jx, jy = rng.uniform(-0.2, 0.2, gx.shape) * (x1 - x0) / (nx - 1), rng.uniform(-0.2, 0.2, gy.shape) * (y1 - y0) / (ny - 1)
    jx[:, 0] = jx[:, -1] = 0.0
    jy[0, :] = jy[-1, :] = 0.0
    px, py = gx + jx, gy + jy
    rings = []
    for i in range(ny - 1):
        for j in range(nx - 1):
            a, b, c, d = (px[i, j], py[i, j]), (px[i, j + 1], py[i, j + 1]), (px[i + 1, j + 1], py[i + 1, j + 1]), (px[i + 1, j], py[i + 1, j])
            if rng.random() < 0.5:
                rings += [[a, b, c], [a, c, d]]
            else:
                rings += [[a, b, d], [b, c, d]]
    assert len(rings) == 60
    return rings, (x0, y0, x1, y1)


def comb(teeth, shape):
    """`teeth` rectangles of one id, each narrower than a cell, side by side across the raster's width and taller than
    the raster: every row's centre line is crossed 2 * teeth times, and most spans are empty"""
    H, W = shape
    pitch = W / teeth
    return [rect(k * pitch + 0.1 * pitch, -1.5, k * pitch + 0.6 * pitch, H + 1.5) for k in range(teeth)]


def star(n, cx, cy, r_in, r_out):
    a = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    r = np.where(np.arange(n) % 2 == 0, r_out, r_in) * (1.0 + 0.05 * np.sin(7.0 * a))
    return list(zip(cx + r * np.cos(a), cy + r * np.sin(a)))


@functools.lru_cache(maxsize=None)
def polygon_cases():
    rng = np.random.default_rng(11)
    c = {}
    for shape in ((1, 1), (1, 200), (200, 1)):
        c["trivial %dx%d" % shape] = geom("polygon", [[(-3.2, -2.1), (260.4, -1.3), (150.2, 240.9), (0.2, 0.9)]], [5], shape)
    c["triangle"] = geom("polygon", [TRIANGLE], [0])
    c["concave"] = geom("polygon", [CONCAVE], [2])
    c["two holes"] = geom("polygon", [rect(5.2, 4.4, 125.7, 66.3), rect(20.3, 10.2, 50.9, 30.8),
                                      [(70.1, 40.2), (110.6, 35.3), (95.4, 60.7)]], [3, 3, 3])
    c["overlapping multipolygon"] = geom("polygon", [rect(10.2, 8.3, 80.6, 50.4), rect(50.1, 30.2, 120.8, 65.9)], [4, 4])
    c["bow-tie"] = geom("polygon", [[(10.2, 10.4), (100.7, 60.3), (100.2, 10.9), (10.6, 60.8)]], [1])
    c["on centres"] = geom("polygon", [[(10.5, 10.5), (50.5, 10.5), (50.5, 40.5), (30.5, 20.5), (10.5, 40.5)],
                                       rect(60.0, 20.5, 100.5, 50.0)], [6, 7])
    c["zero area"] = geom("polygon", [[(10.2, 10.3), (60.7, 50.1), (10.2, 10.3)], [(5.0, 60.0), (45.0, 40.0), (85.0, 20.0)]], [1, 2])
    c["two overlapping"] = geom("polygon", [rect(10.2, 8.3, 80.6, 50.4), rect(50.1, 30.2, 120.8, 65.9)], [9, 4])
    c["five overlapping"] = geom("polygon", [rect(5.3 + 9 * k, 3.1 + 5 * k, 70.2 + 11 * k, 40.6 + 6 * k) for k in range(5)],
                                 [3, 0, 4, 1, 2])
    c["ids to 2^30"] = geom("polygon", [rect(5.3 + 20 * k, 3.1 + 9 * k, 45.2 + 20 * k, 40.6 + 6 * k) for k in range(5)],
                            [2 ** 30, 0, 77777, 2 ** 30 - 1, 123456789])
    rings, _ = tessellation()
    c["tessellation"] = geom("polygon", rings, list(rng.permutation(60)))
    c["outside left"] = geom("polygon", [[(x - 300.0, y) for x, y in TRIANGLE]], [1])
    c["outside right"] = geom("polygon", [[(x + 300.0, y) for x, y in TRIANGLE]], [1])
    c["outside above"] = geom("polygon", [[(x, y - 300.0) for x, y in TRIANGLE]], [1])
    c["outside below"] = geom("polygon", [[(x, y + 300.0) for x, y in TRIANGLE]], [1])
    c["partly outside"] = geom("polygon", [[(x * 1.7 - 40.0, y * 1.9 - 30.0) for x, y in CONCAVE]], [8])
    c["far vertices"] = geom("polygon", [[(-1e12, -1e12 + 7.0), (1e12, -3e11), (40.3, 1e12), (-2e11, 20.7)],
                                         [(-1e12, 30.2), (60.4, -1e12), (1e12, 35.8), (70.6, 1e12)]], [2, 5])
    c["empty"] = geom("polygon", [], [])
    return c


@functools.lru_cache(maxsize=None)
def comb_case(teeth=10000, shape=(40, 130)):
    return geom("polygon", comb(teeth, shape), [7] * teeth, shape)


@functools.lru_cache(maxsize=None)
def large_case():
    """3,000 random small polygons and one 20,000-vertex star on 1500 x 2300: many rows, long spans beside short ones,
    every kernel's tail"""
    H, W = 1500, 2300
    rng = np.random.default_rng(23)
    rings = []
    for _ in range(3000):
        n = int(rng.integers(3, 9))
        cx, cy = rng.uniform(-20.0, W + 20.0), rng.uniform(-20.0, H + 20.0)
        a = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
        r = rng.uniform(2.0, 40.0, n)
        rings.append(list(zip(cx + r * np.cos(a), cy + r * np.sin(a))))
    rings.append(star(20000, W / 2 + 0.37, H / 2 - 0.21, 300.0, 720.0))
    return geom("polygon", rings, list(rng.permutation(3000) + 1) + [0], (H, W))


def _octants():
    """segments in all eight octants and both orientations, axis-parallel ones, endpoints inside cells, on cell corners
    and on cell edges, and zero-length ones"""
    out = []
    for x0, y0 in ((40.3, 30.6), (40.0, 30.0), (40.0, 30.4), (40.7, 30.0)):
        for dx, dy in ((25.4, 9.7), (9.7, 25.4), (-9.7, 25.4), (-25.4, 9.7), (-25.4, -9.7), (-9.7, -25.4), (9.7, -25.4),
                       (25.4, -9.7), (20.0, 0.0), (0.0, 20.0), (-20.0, 0.0), (0.0, -20.0), (15.0, 15.0), (-15.0, 15.0),
                       (12.0, 5.0), (0.0, 0.0), (0.3, 0.2)):
            out.append([(x0, y0), (x0 + dx, y0 + dy)])
            out.append([(x0 + dx, y0 + dy), (x0, y0)])
    return out


@functools.lru_cache(maxsize=None)
def line_cases():
    rng = np.random.default_rng(5)
    c = {}
    segs = _octants()
    c["octants"] = geom("line", segs, list(rng.permutation(len(segs))))
    c["one vertex"] = geom("line", [[(12.3, 7.9)], [(0.0, 0.0)], [(130.0, 5.0)], [(-0.5, 3.0)]], [1, 2, 3, 4])
    c["far segment"] = geom("line", [[(-1e12, -1e12), (1e12, 1e12)], [(-1e12, 4e11), (1e12, -3.9e11)],
                                     [(64.6, -1e12), (65.2, 1e12)]], [1, 2, 3])
    walk = np.cumsum(rng.uniform(-1.5, 1.5, (5000, 2)), axis=0) + (65.0, 35.0)
    c["random walk"] = geom("line", [[tuple(v) for v in walk]], [12])
    c["levee ring"] = geom("line", [[(20.4, 15.3), (100.2, 22.8), (90.7, 60.1), (30.3, 50.6), (20.4, 15.3)]], [0])
    c["empty"] = geom("line", [], [])
    return c


@functools.lru_cache(maxsize=None)
def point_cases():
    c = {}
    c["points"] = geom("point", [[(0.0, 0.0), (1.0, 1.0), (129.999, 69.999), (130.0, 5.0), (5.0, 70.0), (-0.0001, 3.0),
                                  (3.0, -0.0001), (64.5, 35.5), (1e12, 3.0), (-1e12, -1e12)],
                                 [(64.5, 35.5), (12.25, 8.75)], []], [3, 9, 4])
    c["empty"] = geom("point", [], [])
    return c
