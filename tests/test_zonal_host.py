"""CPU (not gpu): the numpy reference of the zonal statistics (tests/_zonal_ref.py) against explicit per-zone Python
loops on small rasters, every ValueError path of descriptools_amd.zonal (each raised before any library call, so none
needs a device), the host-side float stage and quantiles, the alias module and the binding table."""
import math

import numpy as np
import pytest

import _zonal_ref as Z

from descriptools_amd import zonal


def _case(seed, H=37, W=29, nz=7, dtype=np.float32):
    rng = np.random.default_rng(seed)
    zones = rng.integers(-2, nz, (H, W)).astype(np.int32)
    zones[zones == -2] = -100
    v = (rng.random((H, W)) * 50 - 10).astype(dtype)
    v[rng.random((H, W)) < 0.05] = np.nan
    v[rng.random((H, W)) < 0.03] = np.inf
    v[rng.random((H, W)) < 0.03] = -np.inf
    v[rng.random((H, W)) < 0.05] = -100.0
    v[0, 0], v[0, 1] = -0.0, 0.0
    zones[0, 0] = zones[0, 1] = nz - 1
    return zones, v, nz


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nodata", [-100.0, None])
def test_reference_tables_against_loops(dtype, nodata):
    zones, v, nz = _case(1, dtype=dtype)
    o, s = Z.default_scale(zones, v, nz, nodata)
    t = Z.tables(zones, v, nz, o, s, nodata)
    assert t["out"] == 0
    for k in range(nz):
        vals = []
        for y in range(zones.shape[0]):
            for x in range(zones.shape[1]):
                val = v[y, x]
                if zones[y, x] != k or not math.isfinite(val) or (nodata is not None and float(val) == nodata):
                    continue
                vals.append(val)
        qs = [int(np.rint((np.float64(val) - o) * 2.0 ** s)) for val in vals]
        assert t["count"][k] == len(vals)
        assert t["s1"][k] == sum(qs)
        assert t["s2"][k] == sum(q * q for q in qs)
        assert int(t["s2_hi"][k]) * 2 ** 32 + int(t["s2_lo"][k]) == sum(q * q for q in qs)
        assert t["vmin"].dtype == dtype and t["vmax"].dtype == dtype
        if vals:
            assert t["vmin"][k] == min(vals) and t["vmax"][k] == max(vals)
        else:
            assert np.isnan(t["vmin"][k]) and np.isnan(t["vmax"][k])
    assert not np.signbit(t["vmin"][nz - 1]) or t["vmin"][nz - 1] != 0   # -0.0 came in as +0.0
    st = Z.statistics(t, o, s)
    for k in range(nz):
        n = int(t["count"][k])
        if n:
            m = np.float64(int(t["s1"][k])) / np.float64(n)
            assert st["mean"][k] == o + m * 2.0 ** -s
            assert abs(st["sum"][k] - sum(float(x) for x in v[(zones == k) & Z.taking_part(zones, v, nz, nodata)])) < 1e-3 * n


def test_reference_empty_zone_and_minus_zero():
    zones = np.array([[0, 0, 2, -100]], np.int32)
    v = np.array([[-0.0, 0.0, 5.0, 1.0]], np.float32)
    t = Z.tables(zones, v, 3, 0.0, 4)
    assert t["count"].tolist() == [2, 0, 1]
    assert t["vmin"][0] == 0 and not np.signbit(t["vmin"][0]) and not np.signbit(t["vmax"][0])
    st = Z.statistics(t, 0.0, 4)
    assert st["count"].tolist() == [2, 0, 1] and st["sum"].tolist() == [0.0, 0.0, 5.0]
    for name in ("mean", "std", "min", "max", "range"):
        assert np.isnan(st[name][1]), name
    assert st["std"][2] == 0.0 and st["range"][2] == 0.0 and st["mean"][2] == 5.0


def test_reference_compact_histogram_crosstab_paint_against_loops():
    rng = np.random.default_rng(3)
    labels = rng.choice([-100, -1, 0, 31, 32, 63, 64, 500, 1199, 1200, 5000], (30, 40)).astype(np.int64)
    zones, labels_of = Z.compact(labels)
    want = sorted({int(l) for l in labels.ravel() if 0 <= l < labels.size})
    assert labels_of.tolist() == want and zones.dtype == np.int32 and labels_of.dtype == np.int64
    for l, z in zip(labels.ravel(), zones.ravel()):
        assert z == (want.index(int(l)) if 0 <= l < labels.size else -100)
    zones, v, nz = _case(4, H=40, W=40)
    edges = np.array([-10.0, 0.0, 0.5, 7.0, 40.0])
    v[1, :5] = edges
    h = Z.histogram(zones, v, nz, edges)
    for k in range(nz):
        row = [0] * 4
        for z, val in zip(zones.ravel(), v.ravel()):
            if z != k or not math.isfinite(val) or val == -100.0:
                continue
            for b in range(4):
                if edges[b] <= val < edges[b + 1] or (b == 3 and val == edges[4]):
                    row[b] += 1
        assert h[k].tolist() == row
    b = rng.integers(-1, 3, zones.shape).astype(np.int32)
    ct = Z.crosstab(zones, b, nz, 2)
    for i in range(nz):
        for j in range(2):
            assert ct[i, j] == int(((zones == i) & (b == j)).sum())
    table = np.arange(nz, dtype=np.float64) * 1.5
    p = Z.paint(table, zones, np.nan)
    for z, o in zip(zones.ravel(), p.ravel()):
        assert (o == table[z]) if 0 <= z < nz else np.isnan(o)


def test_float_stage_matches_reference_and_quantiles():
    zones, v, nz = _case(5, dtype=np.float64)
    o, s = Z.default_scale(zones, v, nz)
    r = Z.tables(zones, v, nz, o, s)
    t = zonal.ZoneTables(r["count"], r["s1"], r["s2_lo"], r["s2_hi"], r["vmin"], r["vmax"], o, s)
    got = zonal.statistics_from_tables(t, zonal.OUTPUTS)
    ref = Z.statistics(r, o, s)
    assert list(got) == list(zonal.OUTPUTS)
    for name in zonal.OUTPUTS:
        assert got[name].dtype == ref[name].dtype and got[name].tobytes() == ref[name].tobytes(), name
    with pytest.raises(ValueError, match="needs the accumulator"):
        zonal.statistics_from_tables(t._replace(s2_lo=None, s2_hi=None), ("std",))
    edges = np.linspace(-10, 40, 11)
    h = Z.histogram(zones, v, nz, edges)
    h[2] = 0
    q = zonal.quantiles(h, edges, [0.0, 0.25, 0.5, 1.0])
    assert q.shape == (nz, 4) and np.isnan(q[2]).all()
    for k in range(nz):
        for i, p in enumerate([0.0, 0.25, 0.5, 1.0]):
            e = Z.quantile_loop(h[k], edges, p)
            assert (np.isnan(e) and np.isnan(q[k, i])) or q[k, i] == e
    assert zonal.quantiles(h, edges, 0.5).tobytes() == q[:, 2].tobytes()
    one = zonal.quantiles(np.array([[0, 4, 0]]), [0.0, 1.0, 2.0, 3.0], [0.0, 0.5, 1.0])
    assert one.tolist() == [[1.0, 1.5, 2.0]]
    for bad in (2.0, -0.1, [[0.5]], "x"):
        with pytest.raises(ValueError):
            zonal.quantiles(h, edges, bad)
    with pytest.raises(ValueError, match="hist"):
        zonal.quantiles(h[:, :3], edges, 0.5)


Z4 = np.zeros((4, 4), np.int32)
V4 = np.ones((4, 4), np.float32)


@pytest.mark.parametrize("call, match", [
    # shapes and dtypes
    (lambda: zonal.compact(np.zeros(4, np.int32)), "2-D"),
    (lambda: zonal.compact(np.zeros((4, 4), np.float32)), "integer dtype"),
    (lambda: zonal.tables(np.zeros(4, np.int32), V4, 1), "2-D"),
    (lambda: zonal.tables(Z4, np.ones((4, 5), np.float32), 1), "shape"),
    (lambda: zonal.tables(Z4.astype(np.float32), V4, 1), "integer dtype"),
    (lambda: zonal.tables(Z4, V4.astype(complex), 1), "dtype"),
    (lambda: zonal.tables(Z4.astype(np.int64) + 2 ** 31, V4, 1), "int32"),
    (lambda: zonal.histogram(Z4, np.ones((5, 4)), 1, [0, 1]), "shape"),
    (lambda: zonal.crosstab(Z4, np.zeros((4, 5), np.int32), 1, 1), "shape"),
    (lambda: zonal.crosstab(Z4, V4, 1, 1), "integer dtype"),
    (lambda: zonal.paint(np.zeros((2, 2)), Z4, 0.0), "1-D"),
    (lambda: zonal.paint(np.zeros(2, np.int16), Z4, 0), "float32, float64, int32 or int64"),
    (lambda: zonal.paint(np.zeros(2), V4, 0.0), "integer dtype"),
    (lambda: zonal.paint(np.zeros(2, np.int32), Z4, np.nan), "fill"),
    (lambda: zonal.paint(np.zeros(2, np.int32), Z4, 2 ** 31), "fill"),
    (lambda: zonal.paint(np.zeros(2), Z4, "x"), "fill"),
    # n_zones, limit
    (lambda: zonal.tables(Z4, V4, -1), "n_zones"),
    (lambda: zonal.tables(Z4, V4, 1.0), "n_zones"),
    (lambda: zonal.tables(Z4, V4, True), "n_zones"),
    (lambda: zonal.tables(Z4, V4, 2 ** 31), "n_zones"),
    (lambda: zonal.compact(Z4, limit=0), "limit"),
    (lambda: zonal.compact(Z4, limit=2 ** 31), "limit"),
    (lambda: zonal.compact(Z4, limit=3.0), "limit"),
    (lambda: zonal.crosstab(Z4, Z4, 1, 0), "n_b"),
    (lambda: zonal.crosstab(Z4, Z4, 1, 1025), "n_b"),
    (lambda: zonal.crosstab(Z4, Z4, -1, 1), "n_a"),
    # a zone >= n_zones
    (lambda: zonal.tables(Z4 + 3, V4, 3), "holds the id 3, n_zones is 3"),
    (lambda: zonal.histogram(Z4 + 3, V4, 3, [0, 1]), "holds the id 3"),
    (lambda: zonal.crosstab(Z4 + 1, Z4, 1, 1), "a holds the id 1, n_a is 1"),
    (lambda: zonal.crosstab(Z4, Z4 + 2, 1, 2), "b holds the id 2, n_b is 2"),
    # K and edges
    (lambda: zonal.histogram(Z4, V4, 1, [0.0]), "edges"),
    (lambda: zonal.histogram(Z4, V4, 1, np.arange(1026.0)), "edges"),
    (lambda: zonal.histogram(Z4, V4, 1, [[0.0, 1.0]]), "edges"),
    (lambda: zonal.histogram(Z4, V4, 1, [0.0, 1.0, 1.0]), "strictly increasing"),
    (lambda: zonal.histogram(Z4, V4, 1, [0.0, 2.0, 1.0]), "strictly increasing"),
    (lambda: zonal.histogram(Z4, V4, 1, [0.0, np.nan]), "finite"),
    (lambda: zonal.histogram(Z4, V4, 1, [0.0, np.inf]), "finite"),
    (lambda: zonal.histogram(Z4, V4, 1, ["a", "b"]), "edges"),
    # the 2 GiB cap
    (lambda: zonal.histogram(Z4, V4, 2 ** 18 + 1, np.arange(1025.0)), "2 GiB"),
    (lambda: zonal.crosstab(Z4, Z4, 2 ** 18 + 1, 1024), "2 GiB"),
    # frac_bits, origin, nodata, a value outside the contract
    (lambda: zonal.tables(Z4, V4, 1, frac_bits=25), "frac_bits"),
    (lambda: zonal.tables(Z4, V4, 1, frac_bits=-1), "frac_bits"),
    (lambda: zonal.tables(Z4, V4, 1, frac_bits=1.5), "frac_bits"),
    (lambda: zonal.tables(Z4, V4, 1, origin=np.nan), "origin"),
    (lambda: zonal.tables(Z4, V4, 1, origin="a"), "origin"),
    (lambda: zonal.tables(Z4, V4, 1, nodata=np.inf), "nodata"),
    (lambda: zonal.tables(Z4, V4 * 2 ** 20, 1, frac_bits=16, origin=0.0), "too fine"),
    (lambda: zonal.tables(Z4, V4, 1, frac_bits=0, origin=2.0 ** 31 + 1), "too fine"),
    (lambda: zonal.tables(Z4, V4.astype(np.float64) * 1e300, 1, origin=0.0), "do not fit"),
    (lambda: zonal.statistics(Z4, V4 * 2 ** 20, 1, frac_bits=16, origin=0.0), "too fine"),
    # want / outputs unknown, repeated or empty
    (lambda: zonal.tables(Z4, V4, 1, want=()), "empty"),
    (lambda: zonal.tables(Z4, V4, 1, want=("count", "count")), "twice"),
    (lambda: zonal.tables(Z4, V4, 1, want=("median",)), "not one of"),
    (lambda: zonal.tables(Z4, V4, 1, want="count"), "sequence"),
    (lambda: zonal.statistics(Z4, V4, 1, outputs=()), "empty"),
    (lambda: zonal.statistics(Z4, V4, 1, outputs=("mean", "mean")), "twice"),
    (lambda: zonal.statistics(Z4, V4, 1, outputs=("median",)), "not one of"),
    (lambda: zonal.statistics(Z4, V4, 1, outputs="mean"), "sequence"),
    (lambda: zonal.statistics(Z4, V4, 1, outputs=(1,)), "not one of"),
])
def test_bad_arguments_raise_before_any_library_call(call, match, monkeypatch):
    from descriptools_amd import _lib

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match=match):
        call()


def test_default_scale():
    z = np.zeros((1, 3), np.int32)
    assert zonal._scale((3.7, 120.2), None, None) == (3.0, 16)
    assert zonal._scale((3.7, 40000.0), None, None) == (3.0, 15)       # 39997 * 2^16 > 2^31 - 1
    assert zonal._scale(None, None, None) == (0.0, 16)
    assert zonal._scale((-5.5, 1.0), 3, 10.0) == (10.0, 3)              # negative q is within the contract
    v = np.array([[3.7, 120.2, -100.0]], np.float32)
    assert zonal._range(z, v, -100.0) == (float(np.float32(3.7)), float(np.float32(120.2)))
    assert zonal._range(z, v, None)[0] == -100.0
    assert zonal._range(z - 1, v, None) is None
    assert Z.default_scale(z, v, 1) == (3.0, 16)
    # exactly on the bound, and one over it
    assert zonal._scale((0.0, float(2 ** 31 - 1)), 0, 0.0) == (0.0, 0)
    with pytest.raises(ValueError, match="too fine"):
        zonal._scale((0.0, float(2 ** 31)), 0, 0.0)


def test_alias_module_and_bindings():
    import descriptools.zonal as alias
    from descriptools_amd import _lib
    for name in ("compact", "tables", "statistics", "statistics_from_tables", "histogram", "crosstab", "quantiles",
                 "paint", "Compact", "ZoneTables", "OUTPUTS", "ACCUMULATORS"):
        assert getattr(alias, name) is getattr(zonal, name), name
        assert name in alias.__all__
    for name in ("dt_zonal_compact", "dt_zonal_tables", "dt_zonal_counts", "dt_zonal_paint"):
        assert name in _lib._SIGS and name.replace("dt_", "dt_dev_", 1) in _lib._SIGS, name
        assert len(_lib._SIGS[name.replace("dt_", "dt_dev_", 1)][1]) == len(_lib._SIGS[name][1]) + 1
    assert zonal._ZONES_CAP == 1 << 20
