"""CPU (not gpu): descriptools_amd.proximity refuses bad arguments with ValueError before any library call and has no
CPU fallback; dt_proximity is declared, exported, bound and built; the alias module serves the same functions; and the
two forms of the numpy reference the GPU tests compare against (tests/_proximity_ref.py) agree with each other, ties
included."""
import ctypes
import os
import re

import numpy as np
import pytest

from descriptools_amd import proximity

import _proximity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference's two forms ------------------------------------------------------------------------------------
def _cases(shape, rng):
    H, W = shape
    z = np.zeros(shape, np.int8)
    yield "none", z
    yield "all", z + 1
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        c = z.copy()
        c[y, x] = 1
        yield "corner %d,%d" % (y, x), c
    c = z.copy()
    c[H // 3, ::3] = 1
    yield "one row", c
    c = z.copy()
    c[::5, (2 * W) // 3] = 1
    yield "one column", c
    yield "sparse", (rng.random(shape) < 0.002).astype(np.int8)
    yield "dense", (rng.random(shape) < 0.3).astype(np.int8)
    c = z.copy()
    c[::8, ::8] = 1
    yield "lattice", c
    yield "other values", rng.integers(-1, 3, shape).astype(np.int8)


@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (23, 1), (48, 48), (64, 64), (65, 63)], ids=lambda s: "%dx%d" % s)
def test_brute_equals_sweep(shape):
    rng = np.random.default_rng(5)
    for name, river in _cases(shape, rng):
        for nodata in (None, rng.random(shape) < 0.1):
            b, s = R.brute(river, nodata, 12.3), R.sweep(river, nodata, 12.3)
            for what, x, y in zip(("indices", "distance", "d2"), b, s):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, what)
            idx, dist, d2 = b
            src = R.sources(river, nodata)
            off = (idx == -100)
            assert np.array_equal(off, (dist == -100)) and np.array_equal(off, d2 == -100)
            if src.any():
                assert np.array_equal(off, np.zeros(shape, bool) if nodata is None else nodata)
                assert src.reshape(-1)[idx[~off]].all()  # every index names a source
                live = src if nodata is None else src & ~nodata
                assert np.array_equal(idx[live], np.flatnonzero(live.reshape(-1)))  # a source's index is itself
            else:
                assert off.all()


def test_reference_tie_rule_by_hand():
    river = np.zeros((3, 3), np.int8)
    river[0, 1] = river[1, 0] = river[1, 2] = river[2, 1] = 1  # the centre is 1 away from all four
    for form in (R.brute, R.sweep):
        idx, dist, d2 = form(river, None, 2.5)
        assert idx[1, 1] == 1 and d2[1, 1] == 1 and dist[1, 1] == np.float32(2.5)
        assert idx[0, 0] == 1 and idx[2, 2] == 5 and idx[0, 2] == 1 and idx[2, 0] == 3  # corners: two at d2 = 1
        assert dist.dtype == np.float32 and idx.dtype == np.int64


# ---- argument checks ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    from descriptools_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def test_value_errors_before_any_library_call(no_library):
    river = np.zeros((5, 6), np.int8)
    dem = np.zeros((5, 6), np.float32)
    for bad in (river.reshape(-1), river.reshape(5, 6, 1), np.int8(1)):
        with pytest.raises(ValueError, match="2-D"):
            proximity.nearest_river(bad, 10.0)
        with pytest.raises(ValueError, match="2-D"):
            proximity.euclidean_hand(dem, bad, 10.0)
    for other in (np.zeros((6, 5), np.float32), np.zeros((5, 7), np.float64), np.zeros(30, np.float32)):
        with pytest.raises(ValueError, match="shape"):
            proximity.nearest_river(river, 10.0, dem=other)
        with pytest.raises(ValueError, match="shape"):
            proximity.euclidean_hand(other, river, 10.0)
    for px in (0.0, -1.0, float("nan"), float("inf"), "wide", None, True, "a"):
        with pytest.raises(ValueError, match="px"):
            proximity.nearest_river(river, px)
        with pytest.raises(ValueError, match="px"):
            proximity.euclidean_hand(dem, river, px)


def test_2_31_cells_refused(no_library):
    big = np.broadcast_to(np.int8(0), (1 << 16, 1 << 15))  # 2^31 cells, 1 byte of memory
    with pytest.raises(ValueError, match="2\\^31"):
        proximity.nearest_river(big, 10.0)
    with pytest.raises(ValueError, match="2\\^31"):
        proximity.euclidean_hand(np.broadcast_to(np.float32(0), big.shape), big, 10.0)


# ---- the entry and its plumbing -------------------------------------------------------------------------------------
def test_entry_is_declared_exported_bound_and_built():
    from descriptools_amd import _lib, build
    assert "dt_proximity.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "dt_proximity.hip"))
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+dt_proximity\s*\(\s*const\s+int8_t\s*\*", header)
    assert not re.search(r"\bdt_dev_proximity", header), "the device-tier form is a follow-up"
    res, args = _lib._SIGS["dt_proximity"]
    assert res is ctypes.c_int
    assert args == [_lib.c_i8p, _lib.c_f32p, _lib.i64, _lib.i64, _lib.f64, _lib.c_f32p, _lib.c_i64p]
    assert hasattr(ctypes.CDLL(build.build()), "dt_proximity")
    assert hasattr(_lib.lib(), "dt_proximity")


def test_alias_module():
    import descriptools.proximity
    assert descriptools.proximity.nearest_river is proximity.nearest_river
    assert descriptools.proximity.euclidean_hand is proximity.euclidean_hand
    assert descriptools.proximity.Proximity is proximity.Proximity
    p = proximity.Proximity(1, 2)
    assert isinstance(p, tuple) and p.distance == 1 and p.indices == 2 and tuple(p) == (1, 2)


def test_no_cpu_fallback_without_gpu():
    from descriptools_amd import _lib
    if _lib.lib().dt_device_count() > 0:
        pytest.skip("a GPU is visible")
    river = np.zeros((8, 8), np.int8)
    river[3, 3] = 1
    with pytest.raises(RuntimeError):
        proximity.nearest_river(river, 10.0)
    with pytest.raises(RuntimeError):
        proximity.euclidean_hand(np.zeros((8, 8), np.float32), river, 10.0)
