"""CPU (not gpu): descriptools_amd.wetness refuses bad arguments with ValueError before any library call; the reference
of its GPU tests (tests/_wetness_ref.py) is the unique solution the definition claims -- a max-heap Dijkstra, plain
Jacobi sweeps and a randomly ordered tile relaxation agree to the bit; a single row gives the sequential products; the
entries are declared, exported, bound and built; the alias module imports."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _wetness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7


# ---- argument checks ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    from descriptools_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def test_value_errors_before_any_library_call(no_library):
    from descriptools_amd import wetness
    a = np.ones((5, 6), np.float64)
    s = np.ones((5, 6), np.float32)
    for bad in (a.reshape(-1), a.reshape(5, 6, 1), np.float64(1)):
        with pytest.raises(ValueError, match="2-D"):
            wetness.modified_catchment_area(bad, s)
        with pytest.raises(ValueError, match="2-D"):
            wetness.modified_catchment_area(a, bad)
        with pytest.raises(ValueError, match="2-D"):
            wetness.saga_wetness_index(bad, s)
        with pytest.raises(ValueError, match="2-D"):
            wetness.saga_wetness_index(a, bad)
        with pytest.raises(ValueError, match="2-D"):
            wetness.suction(bad)
    for other in (np.ones((6, 5), np.float32), np.ones((5, 7), np.float32)):
        with pytest.raises(ValueError, match="shape"):
            wetness.modified_catchment_area(a, other)
        with pytest.raises(ValueError, match="shape"):
            wetness.saga_wetness_index(a, other)
    with pytest.raises(ValueError, match="dtype"):
        wetness.modified_catchment_area(a.astype(complex), s)
    for t in (1.0, 0.5, 0.0, -10.0, float("nan"), float("inf"), None, True, "a"):
        with pytest.raises(ValueError, match=r"\bt must"):
            wetness.suction(s, t=t)
        with pytest.raises(ValueError, match=r"\bt must"):
            wetness.saga_wetness_index(a, s, t=t)
    for w in (0.0, -1.0, float("nan"), float("inf"), None, True):
        with pytest.raises(ValueError, match="slope_weight"):
            wetness.suction(s, slope_weight=w)
        with pytest.raises(ValueError, match="slope_weight"):
            wetness.saga_wetness_index(a, s, slope_weight=w)
    for v in (-1e-9, float("nan"), float("inf"), None, True):
        with pytest.raises(ValueError, match="slope_offset"):
            wetness.suction(s, slope_offset=v)
        with pytest.raises(ValueError, match="slope_offset"):
            wetness.saga_wetness_index(a, s, slope_offset=v)
        with pytest.raises(ValueError, match="slope_min"):
            wetness.suction(s, slope_min=v)
        with pytest.raises(ValueError, match="slope_min"):
            wetness.saga_wetness_index(a, s, slope_min=v)
    with pytest.raises(ValueError, match="both be 0"):
        wetness.saga_wetness_index(a, s, slope_offset=0.0, slope_min=0.0)
    for limit in (-1, 1.0, None, True):
        with pytest.raises(ValueError, match="_visit_limit"):
            wetness.modified_catchment_area(a, s, _visit_limit=limit)


def test_2_31_cells_refused(no_library):
    from descriptools_amd import wetness
    big = np.broadcast_to(np.float32(1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
    with pytest.raises(ValueError, match="2\\^31"):
        wetness.suction(big)
    with pytest.raises(ValueError, match="2\\^31"):
        wetness.modified_catchment_area(big, big)
    with pytest.raises(ValueError, match="2\\^31"):
        wetness.saga_wetness_index(big, big)


# ---- the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", [(65, 63), (130, 257)], ids=lambda s: "%dx%d" % s)
def test_dijkstra_jacobi_and_a_randomly_ordered_tile_relaxation_agree(shape, kind):
    """the uniqueness claim: the least solution does not depend on the order or the tiling"""
    a, s = R.random_case(shape, kind, SEED)
    ok = R.valid(a, s)
    assert ok.mean() >= 0.85
    D = R.dijkstra(a, s)
    assert D.dtype == np.float64 and (D[~ok] == -100).all()
    assert R.raised(a, s, D) >= 0.5 * ok.sum(), "the case raises too few cells to test anything: change the seed"
    J, sweeps = R.jacobi(a, s)
    assert sweeps >= 5
    assert np.array_equal(D.view(np.int64), J.view(np.int64))
    T = R.tile_relaxation(a, s, 64, 4)
    assert np.array_equal(D.view(np.int64), T.view(np.int64))


def test_every_kind_of_nodata_is_in_the_cases():
    a, s = R.random_case((65, 63), "uniform", SEED)
    assert np.isnan(a).any() and (a == -100).any() and np.isinf(a).any() and (a == 0).any() and (a == -1).any()
    assert np.isnan(s).any() and (s > 1).any() and ((s < 0) & (s > -1)).any() and (s == -100).any()
    a, s = R.random_case((65, 63), "plateau", SEED)
    assert (s == 1).mean() > 0.2 and (a[R.valid(a, s)] == np.floor(a[R.valid(a, s)])).all()
    a, s = R.random_case((65, 63), "steep", SEED)
    assert (s == 0).mean() > 0.05


def test_single_row_gives_the_sequential_products():
    sv = np.float32(0.9)
    a = np.ones((1, 120), np.float64)
    a[0, 0] = 12345.678
    M = R.dijkstra(a, np.full(a.shape, sv, np.float32))
    want, m = [], a[0, 0]
    for k in range(120):
        want.append(max(m, 1.0))
        m = float(sv) * m
    assert M[0].tolist() == want
    assert M[0, 1] == float(sv) * a[0, 0] and M[0, 119] == 1.0 and M[0, 80] > 1.0 and M[0, 2] == float(sv) * (float(sv) * a[0, 0])


def test_lone_cell_with_zero_suction_among_nodata_keeps_its_area():
    a = np.full((3, 3), -100.0)
    a[1, 1] = 5.0
    s = np.zeros((3, 3), np.float32)
    for M in (R.dijkstra(a, s), R.jacobi(a, s)[0], R.tile_relaxation(a, s, 64, 1)):
        assert M[1, 1] == 5.0 and (np.delete(M.reshape(-1), 4) == -100).all()


def test_suction_and_index_by_hand():
    s = R.suction(np.array([[0.0, 1.0, math.pi / 2, -100.0, np.nan, -1e-9]], np.float32))
    assert s.dtype == np.float32
    e = math.radians(0.1)
    assert abs(float(s[0, 0]) - 10.0 ** -(e * math.exp(10.0 ** e))) <= float(np.spacing(s[0, 0]))
    assert s[0, 1] == 0 and list(s[0, 2:]) == [-100] * 4
    assert R.suction(np.zeros((1, 1), np.float32), slope_offset=0.0)[0, 0] == 1.0
    w = R.swi(np.array([[100.0, -100.0, 100.0, np.inf]]), np.array([[0.5, 0.5, 1.5706, 0.5]], np.float32))
    assert abs(float(w[0, 0]) - math.log(100.0 / math.tan(float(np.float32(0.5)) + e))) <= float(np.spacing(w[0, 0]))
    assert list(w[0, 1:]) == [-100] * 3  # nodata; b >= pi/2; M not finite


def test_serpentine_reference():
    a, s = R.serpentine(s=1.0)
    ok = R.valid(a, s)
    assert int(ok.sum()) == 25154 and (R.dijkstra(a, s)[ok] == 1e6).all()
    a, s = R.serpentine(s=np.float32(0.999))
    M = R.dijkstra(a, s)
    assert len(np.unique(M[ok])) == 8386 and abs(M[ok].min() - 227.33468672097197) < 1e-9
    assert R.raised(a, s, M) == 25154 - 1
    assert R.serpentine_tile_entries() == 135


# ---- the entries and their plumbing ---------------------------------------------------------------------------------
def test_entries_are_declared_exported_bound_and_built():
    from descriptools_amd import _lib, build
    assert "dt_wetness.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "dt_wetness.hip"))
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = ("dt_wetness_suction", "dt_wetness_modified_area", "dt_wetness_saga", "dt_dev_wetness_suction",
             "dt_dev_wetness_modified_area", "dt_dev_wetness_index")
    so = ctypes.CDLL(build.build())
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._SIGS and _lib._SIGS[name][0] is ctypes.c_int, name
        assert hasattr(so, name), name
    assert _lib._SIGS["dt_wetness_saga"][1] == [_lib.c_f64p, _lib.c_f32p, _lib.i64, _lib.i64, _lib.f64, _lib.f64,
                                               _lib.f64, _lib.f64, _lib.ci, _lib.c_f32p, _lib.c_f64p, _lib.c_f32p,
                                               _lib.c_i64p]
    assert _lib._SIGS["dt_wetness_modified_area"][1] == [_lib.c_f64p, _lib.c_f32p, _lib.i64, _lib.i64, _lib.ci,
                                                        _lib.c_f64p, _lib.c_i64p]
    L = _lib.lib()
    assert L.dt_dev_wetness_modified_area(None, None, None, 4, 4, 0, 1, None) == -1
    assert L.dt_last_error() == b"invalid argument: ctx is NULL"


def test_raise_on_status_names_the_modified_area():
    from descriptools_amd import device

    class Ctx(device.Context):
        def __init__(self, st):
            self._st = st

        def status(self):
            return self._st

    with pytest.raises(RuntimeError, match="dt_dev_wetness_modified_area"):
        Ctx(2).raise_on_status()
    Ctx(0).raise_on_status()


def test_alias_module():
    import descriptools.wetness as alias
    from descriptools_amd import wetness
    assert alias.suction is wetness.suction
    assert alias.modified_catchment_area is wetness.modified_catchment_area
    assert alias.saga_wetness_index is wetness.saga_wetness_index
    assert alias.ModifiedArea is wetness.ModifiedArea
    assert "saga_wetness_index" in alias.__all__
    assert wetness.SLOPE_OFFSET == math.radians(0.1)
