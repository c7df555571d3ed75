"""CPU (not gpu): watershed.drainage / basins / watersheds / upslope_length refuse bad arguments with ValueError before
any library call, call the bound dt_drainage / dt_upslope_length, and the entry points are declared and bound.  The
pure-numpy reference that the GPU tests hold the kernels to (tests/_watershed_ref.py) is checked here on hand-built
cases."""
import os
import re

import numpy as np
import pytest

from descriptools_amd import _lib, watershed

import _watershed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(watershed._lib, "lib", boom)


FDR = np.full((5, 7), R.E, np.uint8)


class _Huge:
    """a 2-D array-like of 2^31 cells that holds no memory"""
    ndim = 2
    shape = (1 << 16, 1 << 15)
    size = 1 << 31

    def __array__(self, dtype=None, copy=None):
        return np.broadcast_to(np.uint8(1), self.shape)


@pytest.mark.parametrize("kw, what", [
    (dict(fdr=np.ones(7, np.uint8)), "2-D"),
    (dict(fdr=np.ones((2, 3, 4), np.uint8)), "2-D"),
    (dict(dem=np.ones((5, 6), np.float32)), "shape"),
    (dict(pour_points=np.ones((7, 5), np.int64)), "shape"),
    (dict(pour_points=np.ones((5, 7), np.float64)), "integer"),
    (dict(pour_points=np.ones((5, 7), bool)), "integer"),
    (dict(pour_points=np.full((5, 7), -1, np.int32)), ">= 0"),
    (dict(pour_points=np.full((5, 7), 2 ** 63, np.uint64)), "int64"),
    (dict(px=0.0), "px"),
    (dict(px=-1.0), "px"),
    (dict(px=float("nan")), "px"),
    (dict(px=float("inf")), "px"),
    (dict(px="a"), "px"),
    (dict(px=True), "px"),
])
def test_drainage_refuses_before_the_library(no_library, kw, what):
    args = dict(fdr=FDR, px=1.0, dem=None, pour_points=None)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        watershed.drainage(**args)


def test_other_entry_points_refuse_before_the_library(no_library):
    with pytest.raises(ValueError, match="2-D"):
        watershed.basins(np.ones(3, np.uint8))
    with pytest.raises(ValueError, match="shape"):
        watershed.basins(FDR, dem=np.ones((2, 2)))
    with pytest.raises(ValueError, match="integer"):
        watershed.watersheds(FDR, np.ones((5, 7), np.float32))
    with pytest.raises(ValueError, match=">= 0"):
        watershed.watersheds(FDR, np.full((5, 7), -3, np.int64))
    with pytest.raises(ValueError, match="px"):
        watershed.upslope_length(FDR, px=0)
    with pytest.raises(ValueError, match="shape"):
        watershed.upslope_length(FDR, dem=np.ones((5, 8)))
    with pytest.raises(ValueError, match="2\\^31"):
        watershed.upslope_length(_Huge())
    with pytest.raises(ValueError, match="2\\^31"):
        watershed.drainage(_Huge())


class _FakeLib:
    """records calls and fills the outputs it is given"""

    def __init__(self):
        self.calls = []

    def dt_drainage(self, f, d, p, H, W, px, tg, ln, lb):
        self.calls.append(("drainage", H, W, px, d is not None, p is not None, tg is not None, ln is not None,
                           lb is not None))
        n = H * W
        if p:
            pour = np.ctypeslib.as_array(p, (n,))
            assert pour.dtype == np.int64
        if tg:
            np.ctypeslib.as_array(tg, (n,))[:] = 5
        if ln:
            np.ctypeslib.as_array(ln, (n,))[:] = 1.5
        if lb:
            np.ctypeslib.as_array(lb, (n,))[:] = 6
        return 0

    def dt_upslope_length(self, f, d, H, W, px, out):
        self.calls.append(("upslope", H, W, px, d is not None))
        np.ctypeslib.as_array(out, (H * W,))[:] = 2.5
        return 0


def test_entry_points_call_the_bound_symbols(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(watershed._lib, "lib", lambda: fake)
    dem = np.zeros((5, 7), np.float64)
    pour = np.zeros((5, 7), np.uint8)
    dr = watershed.drainage(FDR, 3.0, dem, pour)
    assert isinstance(dr, watershed.Drainage) and dr._fields == ("target", "length")
    assert dr.target.dtype == np.int64 and dr.length.dtype == np.float64
    assert (dr.target == 5).all() and (dr.length == 1.5).all()
    b = watershed.basins(FDR)
    assert b.dtype == np.int64 and b.shape == (5, 7) and (b == 5).all()
    w = watershed.watersheds(FDR, pour.astype(np.int16))
    assert w.dtype == np.int64 and (w == 6).all()
    u = watershed.upslope_length(FDR, 2, dem)
    assert u.dtype == np.float64 and (u == 2.5).all()
    assert fake.calls == [("drainage", 5, 7, 3.0, True, True, True, True, False),
                          ("drainage", 5, 7, 1.0, False, False, True, False, False),
                          ("drainage", 5, 7, 1.0, False, True, False, False, True),
                          ("upslope", 5, 7, 2.0, True)]


def test_dem_mask_is_taken_in_the_dems_dtype(monkeypatch):
    """dem <= -100 is nodata in the DEM's own dtype; NaN is not nodata"""
    seen = {}

    class Fake(_FakeLib):
        def dt_upslope_length(self, f, d, H, W, px, out):
            seen["mask"] = np.ctypeslib.as_array(d, (H * W,)).copy()
            return 0

    monkeypatch.setattr(watershed._lib, "lib", lambda: Fake())
    dem = np.array([[np.nan, -100.0, -np.inf, np.inf, -99.99999999, -100.00000001]], np.float64)
    watershed.upslope_length(np.zeros((1, 6), np.uint8), dem=dem)
    assert list(seen["mask"]) == [0, -100, -100, 0, 0, -100]


def test_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    for name in ("dt_drainage", "dt_upslope_length", "dt_dev_drainage", "dt_dev_upslope_length"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib._SIGS, name
    from descriptools_amd import build
    assert "dt_watershed.hip" in build.SOURCES


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_reference_on_hand_built_cases(name):
    fdr, dem, pour, px, tg, ln, lb, up = R.hand_cases()[name]
    t, l, b = R.drainage(fdr, px, dem, pour)
    assert t.dtype == np.int64 and l.dtype == np.float64
    np.testing.assert_array_equal(t, tg)
    np.testing.assert_array_equal(l, np.asarray(ln, np.float64))
    if lb is not None:
        assert b.dtype == np.int64
        np.testing.assert_array_equal(b, lb)
    np.testing.assert_array_equal(R.upslope_length(fdr, px, dem), np.asarray(up, np.float64))


def test_reference_exact_pair_order():
    """two distinct count pairs never tie; the order is that of n_card + n_diag * sqrt(2)"""
    assert R.pair_greater(3, 0, 0, 2)                 # 3 > 2.83
    assert not R.pair_greater(1, 0, 0, 1)             # 1 < 1.41
    assert not R.pair_greater(0, 70, 99, 0)           # 70 sqrt 2 = 98.995 < 99
    assert R.pair_greater(0, 99, 140, 0)              # 99 sqrt 2 = 140.007 > 140
    a, b = 2 ** 31 - 2, 0
    c, d = 0, int((2 ** 31 - 2) / np.sqrt(2.0))
    assert R.pair_greater(a, b, c, d) != R.pair_greater(c, d, a, b)


def test_reference_basins_partition_the_valid_cells():
    rng = np.random.default_rng(4)
    fdr = rng.choice(np.array([R.E, R.SE, R.S, R.SW, 0], np.uint8), size=(30, 40))
    dem = rng.random((30, 40)).astype(np.float32)
    dem[rng.random((30, 40)) < 0.05] = -100
    t, l, _ = R.drainage(fdr, 1.0, dem)
    valid = dem > -100
    assert (t[valid] >= 0).all() and (t[~valid] == -100).all()
    sizes = np.bincount(t[valid])
    assert sizes.sum() == valid.sum()
    up = R.upslope_length(fdr, 1.0, dem)
    # the upslope length at each outlet is the largest length in its basin
    for o in np.unique(t[valid]):
        assert up.reshape(-1)[o] == l[t == o].max()
