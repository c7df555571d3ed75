"""CPU (not gpu): vector.polygonize's reference and the host-side companions, without a device.  The reference
(tests/_polygonize_ref.py) is held against the definition's invariants on every case of tests/_polygonize_cases.py:
closed rings of integer vertices that alternate between horizontal and vertical runs without collinear triples, the
start vertex smallest, the parts strictly ascending in (start vertex, hole), per-id shoelace areas equal to the cell
counts, one shell per 4-connected region, `shell` by labelling equal to `shell` by the west walk restated here in numpy,
and tests/_vector_ref.rasterize of the rings giving the labels back.  Then the refusals, from_pixel, to_geojson and the
declaration of the new symbols."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import _polygonize_cases as K
import _polygonize_ref as P
import _vector_ref as R


@functools.lru_cache(maxsize=None)
def ref(name):
    lab = K.terrain() if name == "terrain" else K.cases()[name]
    out = P.polygonize(lab)
    for a in out[:4]:
        a.setflags(write=False)
    return out


NAMES = list(K.cases()) + ["terrain"]


def _labels(name):
    return P.normalise(K.terrain() if name == "terrain" else K.cases()[name])


def west_walk_shell(lab, coords, parts, ids):
    """`shell` by the rule of the definition: the vertical edge west of the cell above a hole's start vertex"""
    H, W = lab.shape
    n = len(ids)
    north = np.full((H, W + 1), -1, np.int64)      # the ring of the north-going edge on the left of cell (i, j)
    for p in range(n):
        ring = coords[parts[p]:parts[p + 1]].astype(np.int64)
        for (xa, ya), (xb, yb) in zip(ring, np.roll(ring, -1, axis=0)):
            if xa == xb and yb < ya:
                assert (north[yb:ya, xa] == -1).all()
                north[yb:ya, xa] = p
    first = coords[parts[:-1]].astype(np.int64)
    hole = coords[parts[:-1] + 1, 0] == coords[parts[:-1], 0] if n else np.zeros(0, bool)
    link = np.arange(n)
    for p in np.flatnonzero(hole):
        x, y = first[p]
        assert y >= 1 and lab[y - 1, x] == ids[p]
        j = x
        while j >= 0 and lab[y - 1, j] == ids[p]:
            j -= 1
        link[p] = north[y - 1, j + 1]
        assert link[p] >= 0 and ids[link[p]] == ids[p]
        if hole[link[p]]:
            assert tuple(first[link[p]][::-1]) < (y, x), "a hole inherits from a hole with a smaller start vertex"
    shell = link.copy()
    for p in range(n):      # ascending start vertex: the links of earlier holes are resolved
        shell[p] = shell[link[p]]
    return shell.astype(np.int32)


@pytest.mark.parametrize("name", NAMES)
def test_reference_satisfies_the_definition(name):
    lab = _labels(name)
    H, W = lab.shape
    coords, parts, ids, shell, info = ref(name)
    n = len(ids)
    assert coords.dtype == np.float64 and parts.dtype == np.int64 and ids.dtype == np.int32 and shell.dtype == np.int32
    assert coords.shape == (parts[-1], 2) and parts[0] == 0 and shell.shape == (n,)
    assert np.array_equal(coords, np.rint(coords)) and coords.min(initial=0) >= 0
    assert (coords[:, 0] <= W).all() and (coords[:, 1] <= H).all()
    keys = []
    area = {}
    for p in range(n):
        ring = coords[parts[p]:parts[p + 1]]
        m = len(ring)
        assert m >= 4 and m % 2 == 0
        step = np.roll(ring, -1, axis=0) - ring      # closed: the last vertex is joined to the first
        horizontal = step[:, 1] == 0
        assert ((step[:, 0] == 0) != horizontal).all(), "every run is horizontal or vertical and has a length"
        assert (horizontal != np.roll(horizontal, -1)).all(), "runs alternate: no collinear triple"
        yx = [tuple(v) for v in ring[:, ::-1]]
        assert min(yx) == yx[0] and yx.count(yx[0]) == 1
        a = P.shoelace(ring)
        hole = not horizontal[0]
        assert (step[0, 0] > 0 and a > 0) if not hole else (step[0, 1] > 0 and a < 0)
        assert (shell[p] == p) == (not hole)
        keys.append((int(ring[0, 1]) * (W + 1) + int(ring[0, 0]), int(hole)))
        area[int(ids[p])] = area.get(int(ids[p]), 0.0) + a
    assert keys == sorted(keys) and len(set(keys)) == n, "strictly ascending in (start vertex, hole)"
    values, counts = np.unique(lab[lab >= 0], return_counts=True)
    assert area == {int(v): float(c) for v, c in zip(values, counts)}
    # one shell per 4-connected region, and every ring's shell is a shell of its id
    comp = P.components(lab)
    assert int((shell == np.arange(n)).sum()) == int(comp.max()) + 1
    assert (shell[shell] == shell).all() and (ids[shell] == ids).all()
    assert np.array_equal(shell, west_walk_shell(lab, coords, parts, ids))
    assert info["edges"] >= info["vertices"] and info["vertices"] == parts[-1] and info["rings"] == n
    assert info["holes"] == int((shell != np.arange(n)).sum()) and info["rings"] <= info["vertices"] // 4
    assert 1 <= info["rounds"] <= max(1, int(np.ceil(np.log2(max(info["edges"], 1)))) + 1)


@pytest.mark.parametrize("name", NAMES)
def test_reference_rings_rasterise_back_to_the_labels(name):
    lab = _labels(name)
    coords, parts, ids, _, _ = ref(name)
    R.same(name, R.rasterize("polygon", coords, parts, ids, lab.shape), lab.astype(np.int32))


def test_cases_reach_what_they_are_for():
    info = {name: ref(name)[4] for name in NAMES}
    assert info["all background"] == {"edges": 0, "vertices": 0, "rings": 0, "holes": 0, "rounds": 1}
    assert ref("all background")[1].tolist() == [0]
    assert (info["one label"]["vertices"], info["one label"]["rings"], info["one label"]["edges"]) == (4, 1, 400)
    assert info["checkerboard"]["rings"] == 70 * 130 and info["checkerboard"]["vertices"] == 4 * 70 * 130
    assert info["diagonal pair"]["rings"] == 2 and info["pinched"]["rings"] == 1 and info["pinched"]["vertices"] == 10
    assert [tuple(v) for v in ref("pinched")[0]].count((1.0, 1.0)) == 2, "the ring passes the pinch twice"
    assert info["spiral 65x67"]["rings"] == 1 and info["spiral 65x67"]["edges"] > 4000
    assert info["spiral 65x67"]["rounds"] >= 12
    assert info["staircase"]["rings"] == 1 and info["staircase"]["vertices"] == info["staircase"]["edges"] - 2
    coords, parts, ids, shell, _ = ref("holes in a row")
    assert sorted(np.bincount(shell).tolist())[-1] == 6, "five holes resolve to the one shell of label 1"
    coords, parts, ids, shell, _ = ref("tie")
    first = [tuple(v) for v in coords[parts[:-1]]]
    assert len(set(first)) == len(first) - 2, "two vertices start a shell and a hole"
    assert info["terrain"]["edges"] > 20000 and info["terrain"]["holes"] > 10


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_before_the_library(monkeypatch):
    from descriptools_amd import _lib, vector

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_lib, "lib", no_library)
    ok = np.zeros((4, 5), np.int32)
    for bad in (ok.astype(np.float32), ok.astype(np.float64), np.zeros((2, 3, 4), np.int32), np.zeros(7, np.int32),
                np.full((4, 5), 2 ** 30 + 1, np.int64), np.full((4, 5), 2 ** 40, np.uint64), "labels", None):
        with pytest.raises(ValueError):
            vector.polygonize(bad)
    for background in (0.0, "0", True, (0,), np.float32(1)):
        with pytest.raises(ValueError):
            vector.polygonize(ok, background=background)
    # the value named as background may be anything, and only what remains is checked
    assert vector._labels(np.full((2, 2), 2 ** 40, np.int64), 2 ** 40).tolist() == [[-1, -1], [-1, -1]]
    assert vector._labels(np.array([[True, False]]), 0).tolist() == [[1, -1]]
    assert vector._labels(np.array([[-5, 2 ** 30]], np.int64), None).tolist() == [[-1, 2 ** 30]]
    assert vector._labels(np.array([[200, 3]], np.uint8), 3).dtype == np.int32


def test_c_entries_refuse_bad_arguments_without_a_device():
    from descriptools_amd import _lib
    L = _lib.lib()
    lab = np.zeros((4, 5), np.int32)
    lp = _lib.ptr(lab, _lib.c_i32p)
    xy, parts, ids, shell = np.zeros((8, 2)), np.zeros(3, np.int64), np.zeros(2, np.int32), np.zeros(2, np.int32)
    info = np.zeros(8, np.int64)
    out = (_lib.ptr(xy, _lib.c_f64p), _lib.ptr(parts, _lib.c_i64p), _lib.ptr(ids, _lib.c_i32p),
           _lib.ptr(shell, _lib.c_i32p), _lib.ptr(info, _lib.c_i64p))
    for args, message in (((lp, 0, 5, 8, 2) + out, b"invalid argument: empty raster shape"),
                          ((lp, 2 ** 16, 2 ** 15, 8, 2) + out, b"invalid argument: raster of 2^31 cells or more"),
                          ((lp, 4, 5, -1, 2) + out, b"invalid argument: cap_vertices must be in [0, 2^31) vertices"),
                          ((lp, 4, 5, 8, -1) + out, b"invalid argument: cap_rings must be in [0, 2^31) rings"),
                          ((lp, 4, 5, 8, 2 ** 31) + out, b"invalid argument: cap_rings must be in [0, 2^31) rings"),
                          ((None, 4, 5, 8, 2) + out, b"invalid argument: NULL labels"),
                          ((lp, 4, 5, 8, 2, None) + out[1:], b"invalid argument: NULL coords, parts, ids, shell or info"),
                          ((lp, 4, 5, 8, 2) + out[:4] + (None,), b"invalid argument: NULL coords, parts, ids, shell or info")):
        assert L.dt_polygonize(*args) == -1
        assert L.dt_last_error() == message
    two = (C.c_int64 * 2)()
    assert L.dt_polygonize_count(lp, 4, 0, two) == -1 and L.dt_last_error() == b"invalid argument: empty raster shape"
    assert L.dt_polygonize_count(None, 4, 5, two) == -1 and L.dt_last_error() == b"invalid argument: NULL labels or info"
    assert L.dt_polygonize_count(lp, 4, 5, None) == -1


# ---- from_pixel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [(500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0), (-12.5, 0.25, 0.0, 40.0, 0.0, 0.5),
                               (500000.0, 25.98, -15.0, 4100000.0, -15.0, -25.98)])
def test_from_pixel_inverts_to_pixel(t):
    """Both directions are a handful of float64 operations on numbers no larger than M, the largest world coordinate,
    for these transforms of condition number 1: the subtraction of the origin, two products, a difference and a
    quotient one way; two products and two sums the other.  Each rounds by at most 2^-53 of its result, which is at most
    M in world units: 32 * 2^-53 * M bounds the round trip with room for the rotated transform's second terms."""
    from descriptools_amd import vector
    rng = np.random.default_rng(4)
    px = rng.uniform(-50.0, 4000.0, (500, 2))
    world = vector.from_pixel(px, t)
    assert world.dtype == np.float64 and world.shape == px.shape
    x0, dx, rx, y0, ry, dy = t
    assert np.array_equal(world[:, 0], (x0 + dx * px[:, 0]) + rx * px[:, 1])
    assert np.array_equal(world[:, 1], (y0 + ry * px[:, 0]) + dy * px[:, 1])
    again = vector.from_pixel(vector.to_pixel(world, t), t)
    bound = 32 * 2.0 ** -53 * np.abs(world).max()
    assert np.abs(again - world).max() <= bound
    assert vector.from_pixel((0.0, 0.0), t).tolist() == [x0, y0]
    assert vector.from_pixel([[[1.0, 2.0]]], t).shape == (1, 1, 2)


def test_from_pixel_is_exact_for_north_up_power_of_two_pixels():
    from descriptools_amd import vector
    t = (4096.0, 0.25, 0.0, 8192.0, 0.0, -0.25)
    rng = np.random.default_rng(6)
    px = rng.integers(-800, 80000, (400, 2)) / 8.0
    world = vector.from_pixel(px, t)
    assert np.array_equal(vector.to_pixel(world, t), px)
    assert np.array_equal(vector.from_pixel(vector.to_pixel(world, t), t), world)
    for bad in ((0, 1, 0, 0, 0), (0, 1, 2, 0, 2, 4), (0, np.nan, 0, 0, 0, 1), None, (0, True, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            vector.from_pixel([(1.0, 2.0)], bad)
    with pytest.raises(ValueError):
        vector.from_pixel([1.0, 2.0, 3.0], t)


# ---- to_geojson ---------------------------------------------------------------------------------------------------------
def _polygons(name):
    from descriptools_amd import vector
    coords, parts, ids, shell, _ = ref(name)
    return vector.Polygons(vector.Geometry("polygon", coords, parts, ids), shell)


@pytest.mark.parametrize("name", ["nested", "holes in a row", "tie", "noise of 8 labels", "all background"])
def test_geojson_round_trip_reproduces_rings_and_grouping(name, tmp_path):
    from descriptools_amd import vector
    pg = _polygons(name)
    g, shell = pg.geometry, pg.shell
    path = tmp_path / "out.geojson"
    doc = vector.to_geojson(pg, path=str(path))
    assert json.loads(path.read_text()) == json.loads(json.dumps(doc)) and doc["type"] == "FeatureCollection"
    values = sorted(set(g.ids.tolist()))
    assert [f["properties"] for f in doc["features"]] == [{"id": v} for v in values]
    rings = [g.coords[g.parts[p]:g.parts[p + 1]].tolist() for p in range(g.ids.size)]
    want_rings, want_ids = [], []
    for k, (f, v) in enumerate(zip(doc["features"], values)):
        shells = [p for p in range(g.ids.size) if g.ids[p] == v and shell[p] == p]
        groups = [[s] + [p for p in range(g.ids.size) if shell[p] == s and p != s] for s in shells]
        geom = f["geometry"]
        assert geom["type"] == ("Polygon" if len(groups) == 1 else "MultiPolygon")
        polys = [geom["coordinates"]] if geom["type"] == "Polygon" else geom["coordinates"]
        assert len(polys) == len(groups)
        for poly, group in zip(polys, groups):
            assert len(poly) == len(group)
            for ring, p in zip(poly, group):
                assert ring[0] == ring[-1] and ring[:-1] == rings[p], "closed, and the shell first"
                want_rings.append(rings[p])
                want_ids.append(k)
    back = vector.from_geojson(json.loads(json.dumps(doc)))["polygon"]
    if not want_ids:
        assert back is None and doc["features"] == []
        return
    assert back.ids.tolist() == want_ids
    assert [back.coords[back.parts[p]:back.parts[p + 1]].tolist() for p in range(back.ids.size)] == want_rings
    # the same cells: ids are feature positions now
    lab = _labels(name)
    rank = np.searchsorted(values, np.where(lab >= 0, lab, values[0]))
    R.same(name, R.rasterize("polygon", back.coords, back.parts, back.ids, lab.shape),
           np.where(lab >= 0, rank, -1).astype(np.int32))


def test_geojson_transform_properties_lines_and_points():
    from descriptools_amd import vector
    pg = _polygons("tie")
    t = (500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0)
    doc = vector.to_geojson(pg, t, properties={1: {"name": "outer"}})
    assert [f["properties"] for f in doc["features"]] == [{"name": "outer"}, {"id": 2}]
    first = doc["features"][0]["geometry"]
    ring = np.array((first["coordinates"] if first["type"] == "Polygon" else first["coordinates"][0])[0])
    assert np.array_equal(ring[:-1], vector.from_pixel(pg.geometry.coords[:len(ring) - 1], t))
    assert P.shoelace(ring[:-1]) < 0 < P.shoelace(pg.geometry.coords[:len(ring) - 1]), "counter-clockwise with y up"
    assert vector.to_geojson(pg, properties=["a", "b", "c"])["features"][1]["properties"] == "c"
    line = vector.Geometry("line", [(0, 0), (5, 5), (9, 5), (1, 1), (2, 2), (7, 7), (8, 8)], [0, 3, 5, 7], [4, 2, 4])
    doc = vector.to_geojson(line)
    assert [(f["properties"]["id"], f["geometry"]["type"]) for f in doc["features"]] == [(2, "LineString"),
                                                                                       (4, "MultiLineString")]
    assert doc["features"][0]["geometry"]["coordinates"] == [[1.0, 1.0], [2.0, 2.0]]
    assert doc["features"][1]["geometry"]["coordinates"] == [[[0.0, 0.0], [5.0, 5.0], [9.0, 5.0]], [[7.0, 7.0], [8.0, 8.0]]]
    point = vector.Geometry("point", [(3.5, 4.5), (1, 2), (3, 4)], [0, 1, 3], [9, 1])
    doc = vector.to_geojson(point)
    assert [(f["properties"]["id"], f["geometry"]) for f in doc["features"]] == [
        (1, {"type": "MultiPoint", "coordinates": [[1.0, 2.0], [3.0, 4.0]]}), (9, {"type": "Point", "coordinates": [3.5, 4.5]})]
    back = vector.from_geojson(json.loads(json.dumps(vector.to_geojson(line))))["line"]
    assert back.parts.tolist() == [0, 2, 5, 7] and back.ids.tolist() == [0, 1, 1]


def test_geojson_refuses_polygons_without_shell():
    from descriptools_amd import vector
    pg = _polygons("nested")
    with pytest.raises(ValueError, match="polygonize"):
        vector.to_geojson(pg.geometry)
    with pytest.raises(ValueError):
        vector.to_geojson(vector.Polygons(pg.geometry, pg.shell[:-1]))
    with pytest.raises(ValueError):
        vector.to_geojson(vector.Polygons(pg.geometry, np.zeros(pg.shell.size, np.int32)))
    with pytest.raises(ValueError):
        vector.to_geojson("geometry")


# ---- declared, exported, bound --------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import os
    import re
    from descriptools_amd import _lib, vector
    import descriptools.vector as alias
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "descriptools_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("dt_polygonize", "dt_polygonize_count", "dt_dev_polygonize", "dt_dev_polygonize_timed"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in _lib.exported_symbols(), name
    for name in ("polygonize", "Polygons", "from_pixel", "to_geojson"):
        assert getattr(alias, name) is getattr(vector, name) and name in alias.__all__
    assert vector.Polygons._fields == ("geometry", "shell")
