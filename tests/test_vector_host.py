"""CPU (not gpu): descriptools_amd/vector.py without a device.  Every refusal of the module docstring raises ValueError
before any library call; to_pixel inverts the convention of resample.compose; from_geojson reads every listed type;
dt_rasterize_count (host arithmetic) equals the reference's count on the cases the GPU tests rasterise; and the numpy
reference itself, tests/_vector_ref.py, is held against independent truths: rectangles, an exact fractions.Fraction
even-odd test at every cell centre, a 60-triangle tessellation, and the connectivity of every line."""
from collections import deque
from fractions import Fraction

import numpy as np
import pytest

import _vector_cases as K
import _vector_ref as R


def _G(case):
    from descriptools_amd import vector
    return vector.Geometry(*case[:4])


# ---- refusals -----------------------------------------------------------------------------------------------------------
SQUARE = [(1.0, 1.0), (5.0, 1.0), (5.0, 5.0), (1.0, 5.0)]


@pytest.mark.parametrize("kind, coords, parts, ids", [
    ("polygon", [(1.0, 1.0), (np.nan, 1.0), (5.0, 5.0)], [0, 3], [1]),
    ("line", [(1.0, 1.0), (np.inf, 1.0)], [0, 2], [1]),
    ("point", [(1.0, -np.inf)], [0, 1], [1]),
    ("polygon", SQUARE, [1, 4], [1]),                      # parts does not start at 0
    ("polygon", SQUARE, [0, 3], [1]),                      # ... does not end at N
    ("line", SQUARE, [0, 3, 2, 4], [1, 2, 3]),             # ... decreases
    ("polygon", SQUARE, [0, 4], [-1]),                     # id below the range
    ("polygon", SQUARE, [0, 4], [2 ** 30 + 1]),            # id above the range
    ("polygon", SQUARE, [0, 4], [1, 2]),                   # one id per part
    ("polygon", SQUARE, [0, 2, 4], [1, 2]),                # rings of 2 vertices
    ("line", SQUARE, [0, 4, 4], [1, 2]),                   # a line part without a vertex
    ("polygon", [1.0, 2.0, 3.0], [0, 3], [1]),             # coords not (N, 2)
    ("surface", SQUARE, [0, 4], [1]),
    ("polygon", SQUARE, [0.0, 4.0], [1]),                  # offsets must be integers
])
def test_bad_geometry_is_refused(kind, coords, parts, ids):
    from descriptools_amd import vector
    with pytest.raises(ValueError):
        vector.rasterize(vector.Geometry(kind, coords, parts, ids), (8, 8))


def test_bad_calls_are_refused_before_the_library(monkeypatch):
    from descriptools_amd import _lib, vector
    g = vector.Geometry("polygon", SQUARE, [0, 4], [1])

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_lib, "lib", no_library)
    for shape in ((0, 8), (8,), (8, 8, 8), (-1, 8), (2 ** 16, 2 ** 15), (8.0, 8), None, (True, 8)):
        for call in (vector.rasterize, vector.mask, vector.count_crossings):
            with pytest.raises(ValueError):
                call(g, shape)
        with pytest.raises(ValueError):
            vector.burn(g, shape, np.zeros(2), 0.0)
    for conn in (0, 6, 4.0, "8", None, True):
        with pytest.raises(ValueError):
            vector.rasterize(g, (8, 8), connectivity=conn)
        with pytest.raises(ValueError):
            vector.mask(g, (8, 8), conn)
    with pytest.raises(ValueError):
        vector.rasterize(g, (8, 8), all_touched=1)
    with pytest.raises(ValueError):
        vector.rasterize(("polygon", SQUARE, [0, 4], [1]), (8, 8))
    # a geometry whose arrays went bad after it was made
    g.coords[0, 0] = np.nan
    with pytest.raises(ValueError):
        vector.rasterize(g, (8, 8))


def test_empty_geometry_is_valid():
    from descriptools_amd import vector
    for kind in vector.KINDS:
        g = vector.Geometry(kind, np.zeros((0, 2)), [0], [])
        assert g.coords.shape == (0, 2) and g.parts.tolist() == [0] and g.ids.size == 0
        assert vector.count_crossings(g, (5, 7)) == (0, 0)
    assert vector.Geometry("point", [], [0, 0], [4]).ids.tolist() == [4]    # a run of no points


# ---- to_pixel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [(500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0), (-12.5, 0.25, 0.0, 40.0, 0.0, 0.5),
                               (500000.0, 25.98, -15.0, 4100000.0, -15.0, -25.98), (3.0, 0.0, 2.0, -1.0, 4.0, 0.0)])
def test_to_pixel_inverts_the_geotransform(t):
    from descriptools_amd import resample, vector
    rng = np.random.default_rng(1)
    px = rng.uniform(-50.0, 400.0, (200, 2))
    x0, dx, rx, y0, ry, dy = t
    world = np.stack((x0 + dx * px[:, 0] + rx * px[:, 1], y0 + ry * px[:, 0] + dy * px[:, 1]), axis=-1)
    back = vector.to_pixel(world, t)
    assert back.dtype == np.float64 and back.shape == px.shape
    assert np.allclose(back, px, rtol=0, atol=1e-6)
    # compose(t, identity) is the matrix that takes world coordinates to t's pixel coordinates
    a0, a1, a2, b0, b1, b2 = resample.compose(t, (0.0, 1.0, 0.0, 0.0, 0.0, 1.0))
    assert np.allclose(back[:, 0], a0 + a1 * world[:, 0] + a2 * world[:, 1], rtol=0, atol=1e-6)
    assert np.allclose(back[:, 1], b0 + b1 * world[:, 0] + b2 * world[:, 1], rtol=0, atol=1e-6)
    # the origin and the unit steps, exactly
    assert vector.to_pixel((x0, y0), t).tolist() == [0.0, 0.0]
    assert vector.to_pixel([[[x0, y0]]], t).shape == (1, 1, 2)


def test_to_pixel_refuses_bad_transforms():
    from descriptools_amd import vector
    for t in ((0, 1, 0, 0, 0), (0, 1, 2, 0, 2, 4), (0, np.nan, 0, 0, 0, 1), (0, 0, 0, 0, 0, 0), "transform", None,
              (0, True, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            vector.to_pixel([(1.0, 2.0)], t)
    with pytest.raises(ValueError):
        vector.to_pixel([1.0, 2.0, 3.0], (0, 1, 0, 0, 0, 1))


# ---- from_geojson -------------------------------------------------------------------------------------------------------
COLLECTION = {"type": "FeatureCollection", "features": [
    {"type": "Feature", "properties": {"name": "gauge"}, "geometry": {"type": "Point", "coordinates": [3.5, 4.5]}},
    {"type": "Feature", "properties": {"name": "marks"},
     "geometry": {"type": "MultiPoint", "coordinates": [[1.0, 2.0], [3.0, 4.0, 99.0]]}},
    {"type": "Feature", "properties": {"name": "river"},
     "geometry": {"type": "LineString", "coordinates": [[0.0, 0.0], [5.0, 5.0], [9.0, 5.0]]}},
    {"type": "Feature", "properties": {"name": "levees"},
     "geometry": {"type": "MultiLineString", "coordinates": [[[0.0, 1.0], [4.0, 1.0]], [[6.0, 1.0], [9.0, 2.0]]]}},
    {"type": "Feature", "properties": {"name": "lake"},
     "geometry": {"type": "Polygon", "coordinates": [[[1, 1], [9, 1], [9, 9], [1, 9], [1, 1]],
                                                      [[3, 3], [5, 3], [5, 5], [3, 5], [3, 3]]]}},
    {"type": "Feature", "properties": {"name": "islands"},
     "geometry": {"type": "MultiPolygon", "coordinates": [[[[0, 0], [2, 0], [2, 2], [0, 0]]],
                                                           [[[6, 6], [8, 6], [8, 8], [6, 8], [6, 6]],
                                                            [[6.5, 6.5], [7.5, 6.5], [7.5, 7.5], [6.5, 6.5]]]]}},
    {"type": "Feature", "properties": None, "geometry": None},
]}


def test_from_geojson_reads_every_type(tmp_path):
    import json
    from descriptools_amd import vector
    g = vector.from_geojson(COLLECTION)
    assert [p and p["name"] for p in g["properties"]] == ["gauge", "marks", "river", "levees", "lake", "islands", None]
    pt, ln, pg = g["point"], g["line"], g["polygon"]
    assert pt.kind == "point" and pt.parts.tolist() == [0, 1, 3] and pt.ids.tolist() == [0, 1]
    assert pt.coords.tolist() == [[3.5, 4.5], [1.0, 2.0], [3.0, 4.0]]
    assert ln.kind == "line" and ln.parts.tolist() == [0, 3, 5, 7] and ln.ids.tolist() == [2, 3, 3]
    # rings lose GeoJSON's repeated first vertex; a hole is one more ring of the same id
    assert pg.kind == "polygon" and pg.parts.tolist() == [0, 4, 8, 11, 15, 18] and pg.ids.tolist() == [4, 4, 5, 5, 5]
    assert pg.coords[4:8].tolist() == [[3, 3], [5, 3], [5, 5], [3, 5]]
    for a, dt in ((pg.coords, np.float64), (pg.parts, np.int64), (pg.ids, np.int32)):
        assert a.dtype == dt and a.flags.c_contiguous
    # the lake with its hole and the islands with theirs, through the reference: ids are feature positions
    lab = R.rasterize(pg.kind, pg.coords, pg.parts, pg.ids, (10, 10))
    assert lab[2, 2] == 4 and lab[3, 3] == -1 and lab[4, 4] == -1 and lab[5, 5] == 4 and lab[0, 1] == 5
    # the islands' hole has a vertex on the centre of cell (6, 6): half-open, that cell is in the hole
    assert lab[6, 6] == 4 and lab[6, 7] == 5 and lab[7, 6] == 5 and lab[7, 7] == 5 and lab[9, 9] == -1
    # a bare geometry, a single feature, a file, a transform
    one = vector.from_geojson(COLLECTION["features"][2]["geometry"])
    assert one["polygon"] is None and one["point"] is None and one["line"].ids.tolist() == [0] and one["properties"] == [None]
    assert vector.from_geojson(COLLECTION["features"][4])["polygon"].ids.tolist() == [0, 0]
    path = tmp_path / "c.geojson"
    path.write_text(json.dumps(COLLECTION))
    t = (100.0, 2.0, 0.0, 50.0, 0.0, -2.0)
    h = vector.from_geojson(str(path), t)
    assert np.array_equal(h["line"].coords, vector.to_pixel(ln.coords, t)) and h["line"].parts.tolist() == ln.parts.tolist()
    with pytest.raises(ValueError):
        vector.from_geojson({"type": "Feature", "properties": {}, "geometry": {"type": "Curve", "coordinates": []}})
    with pytest.raises(ValueError):
        vector.from_geojson({"type": "Polygon", "coordinates": [[[0, 0], [1, 1]]]})


# ---- the count ----------------------------------------------------------------------------------------------------------
def _all_cases():
    cases = {"polygon: " + k: v for k, v in K.polygon_cases().items()}
    cases["polygon: comb"] = K.comb_case()
    cases["polygon: large"] = K.large_case()
    cases.update({"line: " + k: v for k, v in K.line_cases().items()})
    cases.update({"point: " + k: v for k, v in K.point_cases().items()})
    return cases


def test_count_equals_the_reference_without_a_device():
    from descriptools_amd import vector
    seen = 0
    for name, case in _all_cases().items():
        want = R.count(*case)
        assert vector.count_crossings(_G(case), case[4]) == want, name
        seen += want[0] > 0
    assert seen >= 18
    assert R.count(*K.comb_case()) == (40 * 20000, 20000)
    assert R.count(*K.polygon_cases()["far vertices"])[0] > 0


def test_count_entry_refuses_bad_arguments():
    import ctypes as C
    from descriptools_amd import _lib
    L = _lib.lib()
    xy = (C.c_double * 6)(1, 1, 5, 1, 5, 5)
    tot, big = C.c_int64(7), C.c_int64(7)
    ok = (C.c_int64 * 2)(0, 3)
    assert L.dt_rasterize_count(0, xy, ok, 1, 8, 8, C.byref(tot), C.byref(big)) == 0 and (tot.value, big.value) == (8, 2)
    for kind, parts, P, H, W in ((3, ok, 1, 8, 8), (0, (C.c_int64 * 2)(1, 3), 1, 8, 8), (0, (C.c_int64 * 3)(0, 3, 2), 2, 8, 8),
                                 (0, ok, 1, 0, 8), (0, ok, 1, 2 ** 16, 2 ** 15), (0, None, 1, 8, 8), (0, ok, -1, 8, 8)):
        assert L.dt_rasterize_count(kind, xy, parts, P, H, W, C.byref(tot), C.byref(big)) == -1, (kind, P, H, W)
        assert L.dt_last_error().startswith(b"invalid argument")
    assert L.dt_rasterize_count(0, xy, ok, 1, 8, 8, None, None) == -1


# ---- the reference against independent truths ---------------------------------------------------------------------------------
def test_reference_rectangles_hold_the_cells_whose_centres_they_contain():
    rng = np.random.default_rng(2)
    H, W = K.SHAPE
    yc, xc = np.mgrid[0:H, 0:W] + 0.5
    for k in range(40):
        x0, x1 = np.sort(rng.uniform(-20.0, W + 20.0, 2))
        y0, y1 = np.sort(rng.uniform(-20.0, H + 20.0, 2))
        if k % 4 == 0:   # edges exactly on centre lines: half-open, [x0, x1) x [y0, y1)
            x0, x1, y0, y1 = np.floor(x0) + 0.5, np.floor(x1) + 0.5, np.floor(y0) + 0.5, np.floor(y1) + 0.5
        ring = K.rect(x0, y0, x1, y1) if k % 2 else K.rect(x0, y0, x1, y1)[::-1]
        got = R.rasterize(*K.geom("polygon", [ring], [k]))
        want = np.where((xc >= x0) & (xc < x1) & (yc >= y0) & (yc < y1), k, -1).astype(np.int32)
        R.same("rectangle %d" % k, got, want)


def _lattice_polygon(rng, n, H, W):
    """n (even) vertices on the lattice k/4 + 1/8, in eighths: x = 1 mod 4, y alternately 1 and 3 mod 4.  Consecutive
    vertices then differ by a multiple of 4 in x and by 2 mod 4 in y, while a cell centre (4 mod 8) differs from a vertex
    by odd numbers: the cross product of an edge with a centre is a sum of terms of different 2-adic order and cannot
    vanish, so no centre lies on an edge's line"""
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
    r = rng.uniform(0.2, 0.48, n)
    x8 = np.rint(((0.5 + r * np.cos(a)) * W * 8 - 1) / 4).astype(int) * 4 + 1
    y8 = np.rint(((0.5 + r * np.sin(a)) * H * 8 - 1) / 4).astype(int) * 4 + 1 + 2 * (np.arange(n) % 2)
    return [(Fraction(int(x), 8), Fraction(int(y), 8)) for x, y in zip(x8, y8)]


def _dist2_to_segment(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    t = ((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy)
    t = max(Fraction(0), min(Fraction(1), t))
    ex, ey = ax + t * dx - px, ay + t * dy - py
    return ex * ex + ey * ey


@pytest.mark.parametrize("seed, n", [(1, 6), (2, 10), (3, 14)])
def test_reference_against_exact_even_odd(seed, n):
    H, W = 30, 40
    rng = np.random.default_rng(seed)
    rings = [_lattice_polygon(rng, n, H, W), _lattice_polygon(rng, 4, H, W)]   # one id: even-odd over both rings
    edges = [(r[k], r[(k + 1) % len(r)]) for r in rings for k in range(len(r))]
    assert all(a != b for a, b in edges)
    want = np.full((H, W), -1, np.int32)
    tol2, excluded = Fraction(1, 10 ** 18), 0
    for i in range(H):
        py = Fraction(2 * i + 1, 2)
        for j in range(W):
            px = Fraction(2 * j + 1, 2)
            crossings = 0
            for (ax, ay), (bx, by) in edges:
                if _dist2_to_segment(px, py, ax, ay, bx, by) <= tol2:
                    excluded += 1
                if (ay <= py) != (by <= py):
                    crossings += ax + (py - ay) * (bx - ax) / (by - ay) > px
            if crossings % 2:
                want[i, j] = 9
    assert excluded == 0, "a centre within 1e-9 of an edge: rounding could decide it"
    assert 50 < (want == 9).sum() < H * W - 50
    got = R.rasterize(*K.geom("polygon", [[(float(x), float(y)) for x, y in r] for r in rings], [9, 9], (H, W)))
    R.same("even-odd", got, want)


def test_reference_tessellation_covers_every_cell_once():
    rings, (x0, y0, x1, y1) = K.tessellation()
    H, W = K.SHAPE
    cover = np.zeros((H, W), np.int64)
    for k, ring in enumerate(rings):
        m = R.rasterize(*K.geom("polygon", [ring], [k])) >= 0
        assert m.any(), k
        cover += m
    yc, xc = np.mgrid[0:H, 0:W] + 0.5
    inside = (xc >= x0) & (xc < x1) & (yc >= y0) & (yc < y1)
    assert np.array_equal(cover, inside.astype(np.int64)), "masks are pairwise disjoint and cover the hull exactly once"
    case = K.polygon_cases()["tessellation"]
    lab = R.rasterize(*case)
    assert np.array_equal(lab >= 0, inside)
    for k, ring in enumerate(rings):   # every cell of triangle k holds the id of triangle k
        m = R.rasterize(*K.geom("polygon", [ring], [0])) >= 0
        assert (lab[m] == case[3][k]).all()


def _connected(cells, connectivity):
    cells = set(cells)
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    start = next(iter(cells))
    seen, todo = {start}, deque([start])
    while todo:
        i, j = todo.popleft()
        for di, dj in steps:
            q = (i + di, j + dj)
            if q in cells and q not in seen:
                seen.add(q)
                todo.append(q)
    return seen == cells


@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_lines_are_connected(connectivity):
    H, W = K.SHAPE
    for seg in K._octants():
        lab = R.rasterize(*K.geom("line", [seg], [1]), connectivity=connectivity)
        cells = [tuple(c) for c in np.argwhere(lab == 1)]
        (xa, ya), (xb, yb) = seg
        for x, y in seg:   # both endpoint cells are burnt
            assert (int(np.floor(y)), int(np.floor(x))) in cells, seg
        assert _connected(cells, connectivity), (seg, connectivity)
        # no cell further than one cell from the segment's bounding box, and no more cells than a thin line needs
        ii, jj = np.array(cells).T
        assert ii.min() >= np.floor(min(ya, yb)) and ii.max() <= np.floor(max(ya, yb))
        assert jj.min() >= np.floor(min(xa, xb)) and jj.max() <= np.floor(max(xa, xb))
        if connectivity == 8:
            assert len(cells) <= max(abs(np.floor(xb) - np.floor(xa)), abs(np.floor(yb) - np.floor(ya))) + 3
    # the thin line of a diagonal is NOT 4-connected: the two settings differ where it matters
    diag = R.rasterize(*K.geom("line", [[(10.3, 10.6), (40.8, 38.2)]], [1]), connectivity=8)
    assert not _connected([tuple(c) for c in np.argwhere(diag == 1)], 4)


def test_reference_points_and_all_touched():
    H, W = K.SHAPE
    lab = R.rasterize(*K.point_cases()["points"])
    assert lab[0, 0] == 3 and lab[1, 1] == 3 and lab[69, 129] == 3 and lab[35, 64] == 9 and lab[8, 12] == 9
    assert (lab >= 0).sum() == 5
    case = K.polygon_cases()["concave"]
    inner = R.rasterize(*case)
    closed = K.geom("line", [list(map(tuple, case[1])) + [tuple(case[1][0])]], [2])
    both = R.rasterize(*case, all_touched=True)
    R.same("all_touched", both, np.maximum(inner, R.rasterize(*closed, connectivity=4)))
    assert (both >= 0).sum() > (inner >= 0).sum()
