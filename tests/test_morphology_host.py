"""CPU (not gpu): descriptools_amd.morphology refuses bad arguments with ValueError before any library call; the
references of its GPU tests (tests/_morphology_ref.py) agree with each other -- the max-heap Dijkstra and plain Jacobi
sweeps to the bit, the fill with a sequential priority flood, the regional extrema through the definition with a
brute-force plateau labelling; the reconstruction is idempotent and lies between its start and the mask; the entries
are declared, exported, bound and built; the alias module imports."""
import ctypes
import os
import re

import numpy as np
import pytest

import _morphology_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
KINDS = ("dilation", "erosion")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- argument checks ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    from descriptools_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def test_value_errors_before_any_library_call(no_library):
    from descriptools_amd import morphology as M
    z = np.ones((5, 6), np.float32)
    one = (lambda d, **k: M.fill(d, **k), lambda d, **k: M.hminima(d, 1.0, **k), lambda d, **k: M.hmaxima(d, 1.0, **k),
           M.regional_minima, M.regional_maxima, lambda d, **k: M.opening_by_reconstruction(d, 2, **k),
           lambda d, **k: M.closing_by_reconstruction(d, 2, **k), lambda d, **k: M.reconstruct(d, z, **k),
           lambda d, **k: M.reconstruct(z, d, **k))
    for f in one:
        for bad in (z.reshape(-1), z.reshape(5, 6, 1), np.float32(1)):
            with pytest.raises(ValueError, match="2-D"):
                f(bad)
        for cn in (6, 0, 8.0, None, True, "8"):
            with pytest.raises(ValueError, match="connectivity"):
                f(z, connectivity=cn)
    for other in (np.ones((6, 5), np.float32), np.ones((5, 7), np.float32)):
        with pytest.raises(ValueError, match="shape"):
            M.reconstruct(other, z)
        with pytest.raises(ValueError, match="shape"):
            M.fill(z, outlets=other.astype(bool))
    with pytest.raises(ValueError, match="dtype"):
        M.reconstruct(z.astype(complex), z)
    with pytest.raises(ValueError, match="dtype"):
        M.fill(z, outlets=z)  # a float raster as a mask: compare first
    for kind in ("open", None, 0, b"erosion"):
        with pytest.raises(ValueError, match="kind"):
            M.reconstruct(z, z, kind=kind)
    for limit in (-1, 1.0, None, True):
        with pytest.raises(ValueError, match="_visit_limit"):
            M.reconstruct(z, z, _visit_limit=limit)
    for h in (0.0, -1.0, float("nan"), float("inf"), None, True, "a"):
        with pytest.raises(ValueError, match=r"\bh must"):
            M.hminima(z, h)
        with pytest.raises(ValueError, match=r"\bh must"):
            M.hmaxima(z, h)
    for r in (0, -1, 4097, 2.0, None, True):
        with pytest.raises(ValueError, match="radius"):
            M.opening_by_reconstruction(z, r)
        with pytest.raises(ValueError, match="radius"):
            M.closing_by_reconstruction(z, r)
    # a DEM that float32 cannot hold
    inexact = np.full((5, 6), 0.1, np.float64)
    for f in one[:-2]:
        with pytest.raises(ValueError, match="float32"):
            f(inexact)
    with pytest.raises(ValueError, match="float32"):
        M.reconstruct(z, inexact)


def test_2_31_cells_refused(no_library):
    from descriptools_amd import morphology as M
    big = np.broadcast_to(np.float32(1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
    for f in (M.fill, lambda d: M.hminima(d, 1.0), lambda d: M.hmaxima(d, 1.0), M.regional_minima, M.regional_maxima,
              lambda d: M.opening_by_reconstruction(d, 1), lambda d: M.closing_by_reconstruction(d, 1),
              lambda d: M.reconstruct(d, d)):
        with pytest.raises(ValueError, match="2\\^31"):
            f(big)


# ---- the references -------------------------------------------------------------------------------------------------
def test_key_is_order_preserving_and_leaves_zero_free():
    v = np.array([-np.inf, -3e38, -100.0, -1.5, -1e-45, -0.0, 0.0, 1e-45, 2.5, 3e38, np.inf], np.float32)
    k = R.key(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert _bits(R.unkey(k)).tolist() == _bits(v).tolist()
    assert (k != 0).all() and (~k != 0).all()
    # the float32 values whose key or complemented key is 0 or 1 are NaNs
    for kk in (0, 1, 0xFFFFFFFF, 0xFFFFFFFE):
        assert np.isnan(R.unkey(np.array([kk], np.uint32))[0])
    assert _bits(R.FLOOR) == 0xC2C7FFFF and R.FLOOR > np.float32(-100)


@pytest.mark.parametrize("cn", (8, 4))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", R.FIELDS)
def test_dijkstra_and_jacobi_agree_and_the_result_is_a_reconstruction(field, kind, cn):
    marker, mask = R.random_case((41, 67), field, SEED)
    e = kind == "erosion"
    ref = R.reconstruct(marker, mask, kind, cn)
    jac, sweeps = R.jacobi(marker, mask, kind, cn)
    assert sweeps >= 2
    assert _bits(ref).tolist() == _bits(jac).tolist()
    F, G, ok = R.start_keys(marker, mask, e)
    F0 = R.from_keys(F, e)
    # -100 exactly on the invalid cells and on the valid cells nothing reaches
    assert (ref[~ok] == -100).all()
    reach = ok & (ref != -100)
    assert reach.any()
    # between the start and the mask, and one of the input's bit patterns
    if e:
        assert (ref[reach] >= mask[reach]).all() and (ref[reach] <= np.where(F != 0, F0, np.inf)[reach]).all()
    else:
        assert (ref[reach] <= mask[reach]).all() and (ref[reach] >= np.where(F != 0, F0, -np.inf)[reach]).all()
    pool = set(_bits(mask[ok]).tolist()) | set(_bits(marker[R.given(marker)]).tolist())
    assert set(_bits(ref[reach]).tolist()) <= pool
    # idempotent: the result as the marker gives the result
    again = R.reconstruct(ref, mask, kind, cn)
    assert _bits(again).tolist() == _bits(ref).tolist()
    assert R.changed(marker, mask, kind, ref) >= 0.1 * ok.sum()


def test_every_kind_of_nodata_is_in_the_case():
    marker, mask = R.random_case((130, 257), "nodata", SEED)
    assert np.isnan(mask).any() and (mask == np.inf).any() and (mask == -np.inf).any()
    assert (mask == -100).any() and (mask < -100).any()
    ok = R.valid(mask)
    assert (np.isnan(marker) & ok).any() and ((marker == np.inf) & ok).any() and ((marker <= -100) & ok).any()


@pytest.mark.parametrize("cn", (8, 4))
def test_fill_is_the_priority_flood(cn):
    dem = R.dem_with_voids((60, 90), SEED)
    f = R.fill(dem, cn=cn)
    assert _bits(f).tolist() == _bits(R.priority_flood(dem, cn=cn)).tolist()
    ok = R.valid(dem)
    assert (f[ok] >= dem[ok]).all() and (f[ok] > dem[ok]).mean() >= 0.10
    # seeded: one outlet in a corner; a basin walled off by invalid cells reaches nothing
    dem = dem.copy()
    dem[20:31, 20] = dem[20:31, 30] = dem[20, 20:31] = dem[30, 20:31] = -100.0
    seeds = np.zeros(dem.shape, bool)
    seeds[0, 0] = True
    f = R.fill(dem, seeds, cn)
    assert _bits(f).tolist() == _bits(R.priority_flood(dem, seeds, cn)).tolist()
    assert (f[21:30, 21:30] == -100).all() and f[0, 0] == dem[0, 0] and (f[R.valid(dem)] != -100).sum() > 1000


@pytest.mark.parametrize("cn", (8, 4))
@pytest.mark.parametrize("maxima", (False, True))
def test_regional_extrema_by_reconstruction_are_the_labelled_plateaus(maxima, cn):
    _, dem = R.random_case((41, 67), "nodata", SEED)
    a = R.regional(dem, maxima, cn)
    assert a.tolist() == R.regional_by_reconstruction(dem, maxima, cn).tolist()
    assert 0 < a.sum() < R.valid(dem).sum() and not a[~R.valid(dem)].any()


def test_h_extrema_by_hand():
    z = np.full((7, 9), 10.0, np.float32)
    z[2, 2] = 9.0   # a pit of depth 1
    z[4, 6] = 7.0   # a pit of depth 3
    r = R.h_extrema(z, 2.0, False)
    assert r[2, 2] == 10.0 and r[4, 6] == 9.0 and (np.delete(r.ravel(), [2 * 9 + 2, 4 * 9 + 6]) == 10.0).all()
    r = R.h_extrema(-z, 2.0, True)
    assert r[2, 2] == -10.0 and r[4, 6] == -9.0
    # the floor of the h-maxima marker
    low = np.full((3, 3), -99.5, np.float32)
    assert (R.h_marker(low, 2.0, True) == R.FLOOR).all()
    assert (R.h_extrema(low, 2.0, True) == R.FLOOR).all()


def test_serpentine_and_spiral_are_long_paths():
    marker, mask = R.serpentine(48)
    ref, sweeps = R.jacobi(marker, mask)
    assert sweeps >= 24 * 47 and (ref[mask == 10] == 10).all() and (ref[mask == 1] == 1).all()
    marker, mask = R.spiral(32)
    ref, sweeps = R.jacobi(marker, mask)
    assert sweeps >= 32 * 32 // 2 - 64 and (ref[mask == 10] == 10).all()
    assert (mask == 10).sum() >= 32 * 32 // 2 - 64


# ---- the entries and their plumbing ---------------------------------------------------------------------------------
def test_entries_are_declared_exported_bound_and_built():
    from descriptools_amd import _lib, build
    assert "dt_morphology.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "dt_morphology.hip"))
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    modes = dict(re.findall(r"#define (DT_MORPH_[A-Z]+) (\d+)", header))
    assert modes == {"DT_MORPH_MARKER": "0", "DT_MORPH_SHIFT": "1", "DT_MORPH_STEP": "2", "DT_MORPH_OUTLETS": "3",
                     "DT_MORPH_WINDOW": "4"}
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    so = ctypes.CDLL(build.build())
    for name in ("dt_morph_reconstruct", "dt_dev_morph_reconstruct"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._SIGS and _lib._SIGS[name][0] is ctypes.c_int, name
        assert hasattr(so, name), name
    L = _lib.lib()
    assert L.dt_dev_morph_reconstruct(None, 0, 0, 8, None, None, None, 0.0, 0, 4, 4, 0, 1, None, None) == -1
    assert L.dt_last_error() == b"invalid argument: ctx is NULL"


def test_raise_on_status_names_the_reconstruction():
    from descriptools_amd import device

    class Ctx(device.Context):
        def __init__(self, st):
            self._st = st

        def status(self):
            return self._st

    with pytest.raises(RuntimeError, match="dt_dev_morph_reconstruct"):
        Ctx(2).raise_on_status()


def test_alias_module():
    import descriptools.morphology as alias
    from descriptools_amd import morphology
    for name in ("reconstruct", "fill", "hminima", "hmaxima", "regional_minima", "regional_maxima",
                 "opening_by_reconstruction", "closing_by_reconstruction", "Reconstruction"):
        assert getattr(alias, name) is getattr(morphology, name), name
        assert name in alias.__all__
