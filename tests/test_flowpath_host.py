"""CPU (not gpu): flowpath.upslope_extreme / downstream_extreme and flowdir.d8_carved refuse bad arguments with
ValueError before any library call, call the bound dt_flowpath_* / dt_carve with what they should, and the entry points
are declared, exported and bound.  The pure-numpy reference that the GPU tests hold the kernels to
(tests/_flowpath_ref.py) is checked here on hand-built cases with literal expected arrays and against a plain walk per
cell on a small random field with cycles."""
import ctypes
import os
import re

import numpy as np
import pytest

from descriptools_amd import _lib, flowdir, flowpath

import _flowpath_ref as R
from _watershed_ref import E, N, S, SE, SW, W_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dt_flowpath_upslope", "dt_flowpath_downstream", "dt_carve", "dt_dev_flowpath_upslope",
           "dt_dev_flowpath_downstream", "dt_dev_carve_blend")


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


FDR = np.full((5, 7), E, np.uint8)
VAL = np.ones((5, 7), np.float32)


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
    (dict(fdr=_Huge()), "2\\^31"),
    (dict(values=np.ones((5, 6), np.float32)), "shape"),
    (dict(values=np.ones(35, np.float32)), "2-D"),
    (dict(dem=np.ones((7, 5), np.float32)), "shape"),
    (dict(kind="mean"), "kind"),
    (dict(kind=0), "kind"),
    (dict(kind=None), "kind"),
    (dict(values=np.full((5, 7), 0.1, np.float64)), "float32"),
    (dict(values=np.full((5, 7), 2 ** 24 + 1, np.int32)), "float32"),
    (dict(values=np.full((5, 7), 2 ** 63 + 1, np.uint64)), "float32"),
    (dict(values=np.full((5, 7), 1j, np.complex64)), "real"),
])
def test_both_refuse_before_the_library(no_library, kw, what):
    args = dict(fdr=FDR, values=VAL, kind="max", dem=None)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        flowpath.upslope_extreme(**args)
    with pytest.raises(ValueError, match=what):
        flowpath.downstream_extreme(**args)


@pytest.mark.parametrize("stop, what", [
    (np.ones((5, 7), np.float32), "integer"),
    (np.ones((5, 7), np.float64), "integer"),
    (np.ones((7, 5), np.int8), "shape"),
    (np.ones(35, bool), "2-D"),
])
def test_downstream_refuses_a_bad_stop(no_library, stop, what):
    with pytest.raises(ValueError, match=what):
        flowpath.downstream_extreme(FDR, VAL, "min", stop=stop)


@pytest.mark.parametrize("kw, what", [
    (dict(max_cut=-1.0), "max_cut"),
    (dict(max_cut=float("nan")), "max_cut"),
    (dict(max_cut=-np.inf), "max_cut"),
    (dict(max_cut="deep"), "max_cut"),
    (dict(max_cut=True), "max_cut"),
    (dict(px=0.0), "px"),
    (dict(px=float("inf")), "px"),
    (dict(dem=np.ones(9, np.float32)), "2-D"),
    (dict(dem=np.full((4, 4), 0.1, np.float64)), "float32"),
    (dict(dem=np.array([[1.0, np.nan], [2.0, 3.0]], np.float32)), "NaN"),
    (dict(dem=np.array([[1.0, np.inf], [2.0, 3.0]], np.float32)), "inf"),
])
def test_carved_refuses_before_the_library(no_library, kw, what):
    args = dict(dem=np.ones((4, 4), np.float32), px=10.0, max_cut=None)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        flowdir.d8_carved(**args)
    assert "heights" not in flowdir.d8_carved.__code__.co_varnames  # the float32 tier only


class _FakeLib:
    """records calls and fills the outputs it is given"""

    def __init__(self):
        self.calls = []
        self.seen = {}

    def _fill(self, H, W, value, where):
        if value:
            np.ctypeslib.as_array(value, (H * W,))[:] = 2.5
        if where:
            np.ctypeslib.as_array(where, (H * W,))[:] = 7

    def dt_flowpath_upslope(self, f, d, v, H, W, kind, value, where):
        self.calls.append(("up", H, W, kind, d is not None, bool(value), bool(where)))
        self.seen["values"] = np.ctypeslib.as_array(v, (H * W,)).copy()
        self._fill(H, W, value, where)
        return 0

    def dt_flowpath_downstream(self, f, d, v, s, H, W, kind, value, where):
        self.calls.append(("down", H, W, kind, d is not None, s is not None, bool(value), bool(where)))
        if s:
            self.seen["stop"] = np.ctypeslib.as_array(s, (H * W,)).copy()
        if d:
            self.seen["mask"] = np.ctypeslib.as_array(d, (H * W,)).copy()
        self._fill(H, W, value, where)
        return 0

    def dt_carve(self, dem, H, W, px, cut, fdr, carved, filled, info):
        self.calls.append(("carve", H, W, px, cut, bool(filled)))
        np.ctypeslib.as_array(fdr, (H * W,))[:] = 4
        np.ctypeslib.as_array(carved, (H * W,))[:] = 1.5
        if filled:
            np.ctypeslib.as_array(filled, (H * W,))[:] = 3.5
        return 0


def test_entry_points_call_the_bound_symbols(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    dem = np.zeros((5, 7), np.float64)
    dem[0, :3] = (-100.0, -99.99999999, np.nan)
    vals = np.arange(35, dtype=np.int64).reshape(5, 7)  # exact in float32: accepted
    u = flowpath.upslope_extreme(FDR, vals, "min", dem)
    assert isinstance(u, flowpath.Extreme) and u._fields == ("value", "where")
    assert u.value.dtype == np.float32 and u.value.shape == (5, 7) and (u.value == 2.5).all() and u.where is None
    assert fake.seen["values"].dtype == np.float32 and (fake.seen["values"] == np.arange(35)).all()
    u = flowpath.upslope_extreme(FDR, VAL, where=True)
    assert u.where.dtype == np.int64 and (u.where == 7).all()
    stop = np.zeros((5, 7), np.int64)
    stop[1, 1], stop[2, 2] = 5, -3  # nonzero means stop
    d = flowpath.downstream_extreme(FDR, VAL.astype(np.float64), "max", dem, stop, where=True)
    assert d.value.dtype == np.float32 and d.where.dtype == np.int64
    assert fake.seen["stop"].dtype == np.uint8 and fake.seen["stop"].sum() == 2
    assert list(fake.seen["mask"][:3]) == [-100, 0, 0]  # dem <= -100 in the DEM's own dtype; NaN is not nodata
    flowpath.downstream_extreme(FDR, VAL, "min", stop=np.ones((5, 7), bool))
    flowpath.downstream_extreme(FDR, VAL)
    assert fake.calls == [("up", 5, 7, 1, True, True, False), ("up", 5, 7, 0, False, True, True),
                          ("down", 5, 7, 0, True, True, True, True), ("down", 5, 7, 1, False, True, True, False),
                          ("down", 5, 7, 0, False, False, True, False)]
    fake.calls.clear()
    heights = np.ones((4, 6), np.int16)
    fdr, carved = flowdir.d8_carved(heights, 10)
    assert fdr.dtype == np.uint8 and (fdr == 4).all() and carved.dtype == np.float32 and (carved == 1.5).all()
    fdr, carved, filled = flowdir.d8_carved(heights, 2.0, max_cut=0.5, return_filled=True)
    assert filled.dtype == np.float32 and (filled == 3.5).all()
    flowdir.d8_carved(heights, 2.0, max_cut=np.inf)
    flowdir.d8_carved(heights, 2.0, max_cut=0)
    assert fake.calls == [("carve", 4, 6, 10.0, np.inf, False), ("carve", 4, 6, 2.0, 0.5, True),
                          ("carve", 4, 6, 2.0, np.inf, False), ("carve", 4, 6, 2.0, 0.0, False)]


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    from descriptools_amd import build
    assert "dt_flowpath.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    # the device entries name their shape rows, cols
    for name in SYMBOLS[3:]:
        proto = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert "int64_t rows" in proto and "int64_t cols" in proto and not re.search(r"\bH\b", proto), name


def test_alias_module():
    import descriptools.flowpath as alias
    assert alias.upslope_extreme is flowpath.upslope_extreme
    assert alias.downstream_extreme is flowpath.downstream_extreme and alias.Extreme is flowpath.Extreme


def _same(name, got, want):
    for g, w, part in zip(got, want, ("value", "where")):
        assert g.dtype == w.dtype, (name, part)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (name, part))
    z = got[0] == 0
    assert not np.signbit(got[0][z]).any(), name  # -0.0 comes back as +0.0


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_reference_on_hand_built_cases(name):
    c = R.hand_cases()[name]
    _same(name + " up", R.upslope(c["fdr"], c["values"], c["kind"], c["dem"]), c["up"])
    _same(name + " down", R.downstream(c["fdr"], c["values"], c["kind"], c["dem"], c["stop"]), c["dn"])
    up, dn = R.walk(c["fdr"], c["values"], c["kind"], c["dem"], c["stop"])
    _same(name + " walk up", up, c["up"])
    _same(name + " walk down", dn, c["dn"])


def small_field(seed=5):
    """12 x 17 random codes with two planted cycles, a nodata corner, quantised values with NaN and a stop mask"""
    rng = np.random.default_rng(seed)
    fdr = rng.choice(np.array([E, SE, S, SW, W_, N, 0, 3], np.uint8), size=(12, 17))
    fdr[2, 3], fdr[2, 4], fdr[3, 4], fdr[3, 3] = E, S, W_, N
    fdr[7, 9:13] = E
    fdr[7, 13], fdr[8, 13] = S, W_
    fdr[8, 10:13] = W_
    fdr[8, 9] = N
    dem = np.ones((12, 17), np.float32)
    dem[9:, :4] = -100
    values = rng.integers(0, 5, (12, 17)).astype(np.float32)
    values[rng.random((12, 17)) < 0.1] = np.nan
    stop = (rng.random((12, 17)) < 0.06).astype(np.int8)
    stop[8, 11] = 1  # on the long cycle
    stop[10, 1] = 1  # on nodata
    return fdr, dem, values, stop


@pytest.mark.parametrize("kind", ["max", "min"])
@pytest.mark.parametrize("with_stop", [False, True])
def test_reference_against_a_plain_walk(kind, with_stop):
    fdr, dem, values, stop = small_field()
    st = stop if with_stop else None
    up, dn = R.walk(fdr, values, kind, dem, st)
    _same("up", R.upslope(fdr, values, kind, dem), up)
    _same("down", R.downstream(fdr, values, kind, dem, st), dn)
    assert np.isnan(dn[0]).any() and (dn[1] >= 0).any()
