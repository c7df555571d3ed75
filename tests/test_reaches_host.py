"""CPU (not gpu): reaches.catchments / channels / hydraulic_tables / inundate refuse bad arguments with ValueError before
any library call and call the bound symbols with what they should; the entry points are declared and bound; the
pure-numpy reference that the GPU tests hold the kernels to (tests/_reaches_ref.py) gives the tables written out by
hand on hand-built rasters; rating_curves gives the closed form of a rectangular channel and stage_for_discharge
interpolates at, between, below and above table points."""
import ctypes
import os
import re

import numpy as np
import pytest

from descriptools_amd import _lib, reaches

import _reaches_ref as R
import _streams_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(reaches._lib, "lib", boom)


class _Huge:
    """a 2-D array-like of 2^31 cells that holds no memory"""
    ndim = 2
    shape = (1 << 16, 1 << 15)
    size = 1 << 31

    def __array__(self, dtype=None, copy=None):
        return np.broadcast_to(np.int32(1), self.shape)


LINK = np.full((5, 7), -100, np.int64)
CAT = np.zeros((5, 7), np.int32)
HAND = np.zeros((5, 7), np.float32)
FDR = np.ones((5, 7), np.uint8)


@pytest.mark.parametrize("kw, what", [
    (dict(link=np.zeros(7, np.int64)), "2-D"),
    (dict(link=np.zeros((5, 7), np.float64)), "integer"),
    (dict(indices=np.zeros((7, 5), np.int64)), "shape"),
    (dict(indices=np.zeros((5, 7), np.float32)), "integer"),
    (dict(link=_Huge(), indices=_Huge()), "2\\^31"),
])
def test_catchments_refuses_before_the_library(no_library, kw, what):
    args = dict(link=LINK, indices=LINK)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        reaches.catchments(**args)


@pytest.mark.parametrize("kw, what", [
    (dict(fdr=np.ones(7, np.uint8)), "2-D"),
    (dict(reach=np.zeros((5, 6), np.int32)), "shape"),
    (dict(reach=np.zeros((5, 7), np.float32)), "integer"),
    (dict(reach=np.full((5, 7), 2 ** 31, np.int64)), "int32"),
    (dict(px=0), "px"),
    (dict(px=float("nan")), "px"),
    (dict(px=True), "px"),
    (dict(px="a"), "px"),
    (dict(n_reaches=-1), "n_reaches"),
    (dict(n_reaches=2 ** 31), "n_reaches"),
    (dict(n_reaches=1.5), "n_reaches"),
    (dict(n_reaches=True), "n_reaches"),
])
def test_channels_refuses_before_the_library(no_library, kw, what):
    args = dict(fdr=FDR, reach=CAT, px=1.0, n_reaches=3)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        reaches.channels(**args)


@pytest.mark.parametrize("kw, what", [
    (dict(catchment=np.zeros(7, np.int32)), "2-D"),
    (dict(catchment=np.zeros((5, 7), np.float32)), "integer"),
    (dict(catchment=_Huge()), "2\\^31"),
    (dict(hand=np.zeros((5, 6), np.float32)), "shape"),
    (dict(hand=np.zeros((5, 7), np.complex64)), "real"),
    (dict(px=-1.0), "px"),
    (dict(px=float("inf")), "px"),
    (dict(stages=[]), "stages"),
    (dict(stages=np.zeros(1025)), "stages"),
    (dict(stages=np.zeros((2, 2))), "stages"),
    (dict(stages=[0.0, np.nan]), "finite"),
    (dict(stages=[0.0, np.inf]), "finite"),
    (dict(stages=[-0.5, 1.0]), ">= 0"),
    (dict(stages=[0.0, 1.0, 1.0]), "increasing"),
    (dict(stages=[0.0, 2.0, 1.0]), "increasing"),
    (dict(stages="abc"), "stages"),
    (dict(n_reaches=-3), "n_reaches"),
    (dict(n_reaches=None), "n_reaches"),
    (dict(slope=np.zeros((7, 5), np.float32)), "shape"),
    (dict(frac_bits=1.5), "frac_bits"),
    (dict(frac_bits=True), "frac_bits"),
    (dict(frac_bits=5000), "frac_bits"),
    (dict(frac_bits=50), "too fine"),                                    # 35 * rint(3 * 2^50) > 2^52
    (dict(frac_bits=46, slope=np.full((5, 7), 1e4, np.float32)), "too fine"),   # bed weight ~100
])
def test_hydraulic_tables_refuses_before_the_library(no_library, kw, what):
    args = dict(catchment=CAT, hand=HAND, px=10.0, stages=[0.0, 1.0, 3.0], n_reaches=2, slope=None, frac_bits=None)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        reaches.hydraulic_tables(**args)


@pytest.mark.parametrize("kw, what", [
    (dict(catchment=np.zeros((5, 7, 1), np.int32)), "2-D"),
    (dict(hand=np.zeros((4, 7), np.float32)), "shape"),
    (dict(stage=np.zeros((2, 2))), "stage"),
    (dict(stage="x"), "stage"),
])
def test_inundate_refuses_before_the_library(no_library, kw, what):
    args = dict(catchment=CAT, hand=HAND, stage=np.zeros(2))
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        reaches.inundate(**args)


class _FakeLib:
    """records what each entry point is called with and fills the outputs it is given"""

    def __init__(self, n_heads=3):
        self.calls = []
        self.n_heads = n_heads

    def dt_reach_catchments(self, link, idx, H, W, reach, cat, heads, cap, r):
        self.calls.append(("catchments", H, W, bool(idx), bool(reach), bool(cat), bool(heads), cap))
        n = H * W
        assert np.ctypeslib.as_array(link, (n,)).dtype == np.int64
        if idx:
            assert np.ctypeslib.as_array(idx, (n,)).dtype == np.int64
        if reach:
            np.ctypeslib.as_array(reach, (n,))[:] = 1
        if cat:
            np.ctypeslib.as_array(cat, (n,))[:] = 2
        if heads:
            h = np.ctypeslib.as_array(heads, (cap,))
            h[:] = -1
            k = min(cap, self.n_heads)
            h[:k] = 10 * np.arange(k)
        ctypes.cast(r, ctypes.POINTER(ctypes.c_int64))[0] = self.n_heads
        return 0

    def dt_reach_channels(self, f, reach, H, W, R, end, down, nc, ncard, ndiag):
        self.calls.append(("channels", H, W, R))
        assert np.ctypeslib.as_array(reach, (H * W,)).dtype == np.int32
        for k, a in enumerate((end, down, nc, ncard, ndiag)):
            np.ctypeslib.as_array(a, (R,))[:] = k + 1
        return 0

    def dt_reach_tables(self, cat, hand, hb, slope, H, W, st, K, R, s, cells, hq, bq):
        self.calls.append(("tables", hb, bool(slope), H, W, list(np.ctypeslib.as_array(st, (K,))), K, R, s))
        np.ctypeslib.as_array(cells, (R * K,))[:] = 2
        np.ctypeslib.as_array(hq, (R * K,))[:] = 1 << s
        np.ctypeslib.as_array(bq, (R * K,))[:] = 3 << s
        return 0

    def dt_inundate(self, cat, hand, hb, stage, H, W, R, depth):
        self.calls.append(("inundate", hb, H, W, R, list(np.ctypeslib.as_array(stage, (R,)))))
        np.ctypeslib.as_array(depth, (H * W,))[:] = 0.25
        return 0


def test_entry_points_call_the_bound_symbols(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(reaches._lib, "lib", lambda: fake)
    c = reaches.catchments(LINK.astype(np.int32), LINK)
    assert isinstance(c, reaches.Catchments) and c._fields == ("reach", "catchment", "heads")
    assert c.reach.dtype == np.int32 and c.catchment.dtype == np.int32 and c.heads.dtype == np.int64
    assert (c.reach == 1).all() and (c.catchment == 2).all() and list(c.heads) == [0, 10, 20]
    ch = reaches.channels(FDR, CAT.astype(np.int64), 2.0, 4)
    assert ch._fields == ("end", "down", "n_cells", "n_card", "n_diag", "length")
    assert all(getattr(ch, f).dtype == np.int64 and getattr(ch, f).shape == (4,) for f in ch._fields[:5])
    assert (ch.end == 1).all() and (ch.n_diag == 5).all()
    np.testing.assert_array_equal(ch.length, np.full(4, 4.0 * 2.0 + 5.0 * (2.0 * np.sqrt(2.0))))
    t = reaches.hydraulic_tables(CAT, HAND, 10.0, [0.0, 1.0, 3.0], 2)
    s = t.frac_bits
    assert s == 51 - 6 - 1          # 35 cells, stages up to 3
    assert t._fields == ("stages", "cells", "area", "volume", "bed_area", "frac_bits")
    assert t.cells.dtype == np.int64 and t.cells.shape == (2, 3) and (t.cells == 2).all()
    np.testing.assert_array_equal(t.area, np.full((2, 3), 200.0))
    np.testing.assert_array_equal(t.volume, np.array([[0.0, 100.0, 500.0]] * 2))   # max(stage * 2 - 1, 0) * 100
    np.testing.assert_array_equal(t.bed_area, np.full((2, 3), 300.0))
    # an int16 HAND travels as float64; a slope raster is passed on and bounds the default frac_bits
    reaches.hydraulic_tables(CAT, HAND.astype(np.int16), 1.0, [2.0], 1, slope=np.full((5, 7), 300.0), frac_bits=4)
    d = reaches.inundate(CAT.astype(np.int8), HAND.astype(np.float64), [1.0, 2.0])
    assert d.dtype == np.float32 and d.shape == (5, 7) and (d == 0.25).all()
    assert fake.calls == [("catchments", 5, 7, True, True, True, True, 35),
                          ("channels", 5, 7, 4),
                          ("tables", 4, False, 5, 7, [0.0, 1.0, 3.0], 3, 2, s),
                          ("tables", 8, True, 5, 7, [2.0], 1, 1, 4),
                          ("inundate", 8, 5, 7, 2, [1.0, 2.0])]


def test_heads_beyond_the_first_capacity_take_a_second_call(monkeypatch):
    fake = _FakeLib(n_heads=5)
    monkeypatch.setattr(reaches._lib, "lib", lambda: fake)
    monkeypatch.setattr(reaches, "_HEADS_CAP", 2)
    c = reaches.catchments(LINK, LINK)
    assert list(c.heads) == [0, 10, 20, 30, 40]
    assert fake.calls == [("catchments", 5, 7, True, True, True, True, 2),
                          ("catchments", 5, 7, False, False, False, True, 5)]


def test_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    for name in ("dt_reach_catchments", "dt_reach_channels", "dt_reach_tables", "dt_inundate",
                 "dt_dev_reach_catchments", "dt_dev_reach_channels", "dt_dev_reach_tables", "dt_dev_inundate"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib._SIGS, name
    assert re.search(r"#define\s+DT_STATUS_REACH_RANGE\s+8\b", hdr)
    from descriptools_amd import build
    assert "dt_reaches.hip" in build.SOURCES


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_reference_on_hand_built_cases(name):
    c = R.hand_cases()[name]
    _, _, link = S.reference(c["fdr"], c["river"])
    np.testing.assert_array_equal(link, c["link"])
    reach, cat, heads = R.catchments(link, c["idx"])
    assert reach.dtype == np.int32 and cat.dtype == np.int32 and heads.dtype == np.int64
    np.testing.assert_array_equal(reach, c["reach"])
    np.testing.assert_array_equal(cat, c["catch"])
    np.testing.assert_array_equal(heads, c["heads"])
    nr = heads.size
    ch = R.channels(c["fdr"], reach, c["px"], nr)
    for got, k in zip(ch, ("end", "down", "n_cells", "n_card", "n_diag", "length")):
        assert got.dtype == c[k].dtype, k
        np.testing.assert_array_equal(got, c[k], k)
    cells, hq, bq, took = R.tables(cat, c["hand"], c["stages"], nr, c["s"], c["slope"])
    np.testing.assert_array_equal(cells, c["cells"])
    np.testing.assert_array_equal(hq, c["Hq"])
    np.testing.assert_array_equal(bq, c["Bq"])
    assert took == cells[:, -1].sum()
    area, vol, bed = R.derive(c["stages"], cells, hq, bq, c["px"], c["s"])
    np.testing.assert_array_equal(area, c["area"])
    np.testing.assert_array_equal(vol, c["volume"])
    np.testing.assert_array_equal(bed, c["bed_area"])
    np.testing.assert_array_equal(R.inundate(cat, c["hand"], c["stage"]), c["depth"])
    # the package's host arithmetic is the reference's
    t = reaches.tables_from_sums(c["stages"], cells, hq, bq, c["px"], c["s"])
    np.testing.assert_array_equal(t.area, c["area"])
    np.testing.assert_array_equal(t.volume, c["volume"])
    np.testing.assert_array_equal(t.bed_area, c["bed_area"])


def test_reference_bins_and_participation():
    """a height equal to a stage to the bit falls in that stage's bin; NaN, inf, -100, negatives and heights above the
    last stage take no part"""
    st = np.array([0.1, 0.30000000000000004, 0.9])
    hand = np.array([[0.1, np.nextafter(0.1, 1), 0.30000000000000004, 0.3, 0.9, np.nextafter(0.9, 1),
                      np.nan, np.inf, -np.inf, -100.0, -1e-300, 0.0, -0.0]])
    cat = np.zeros(hand.shape, np.int32)
    cells, _, _, took = R.tables(cat, hand, st, 1, 10)
    np.testing.assert_array_equal(cells, [[3, 6, 7]])   # bin 0: 0.1, 0, -0; bin 1: next(0.1), 0.3.., 0.3; bin 2: 0.9
    assert took == 7


def _rect_tables(width, length, px, stages, s=20):
    """the tables of a rectangular channel: width x length cells, all at HAND 0, flat bed"""
    n = width * length
    cells = np.full((1, len(stages)), n, np.int64)
    hq = np.zeros_like(cells)
    bq = cells << s
    return reaches.tables_from_sums(stages, cells, hq, bq, px, s)


def test_rating_curve_of_a_rectangular_channel():
    """b = 3 cells x 10 m wide, L = 50 cells x 10 m long, depth h: A = b h, wetted bed b (the tables carry no walls),
    so Q = b h * h^(2/3) * sqrt(S0) / n"""
    px, stages = 10.0, np.array([0.0, 0.5, 1.0, 2.0, 4.0])
    t = _rect_tables(3, 50, px, stages)
    L, S0, n = 500.0, 0.001, 0.05
    Q = reaches.rating_curves(t, L, S0, n)
    assert Q.shape == (1, 5) and Q[0, 0] == 0.0
    np.testing.assert_allclose(Q[0], 30.0 * stages * stages ** (2.0 / 3.0) * np.sqrt(S0) / n, rtol=1e-14)
    # per-reach arrays, and the refusals of the definition
    t2 = reaches.HydraulicTables(stages, np.vstack([t.cells, t.cells, t.cells, 0 * t.cells]),
                                 np.vstack([t.area] * 4), np.vstack([t.volume] * 3 + [0 * t.volume]),
                                 np.vstack([t.bed_area] * 3 + [0 * t.bed_area]), 20)
    Q2 = reaches.rating_curves(t2, [500.0, 0.0, 500.0, 500.0], [0.001, 0.001, -1.0, 0.001], 0.05)
    np.testing.assert_array_equal(Q2[0], Q[0])
    assert np.isnan(Q2[1]).all() and np.isnan(Q2[2]).all()
    np.testing.assert_array_equal(Q2[3], np.zeros(5))           # no cells: 0
    assert np.isnan(reaches.rating_curves(t, L, S0, 0.0)).all()
    assert np.isnan(reaches.rating_curves(t, L, np.nan, n)).all()
    with pytest.raises(ValueError):
        reaches.rating_curves(t, [1.0, 2.0], S0, n)


def test_stage_for_discharge():
    stages = np.array([0.0, 1.0, 2.0, 4.0])
    Q = np.array([[0.0, 10.0, 30.0, 90.0],
                  [0.0, 10.0, 5.0, 20.0],           # not monotone: the running maximum is interpolated
                  [np.nan, 1.0, 2.0, 3.0],
                  [2.0, 4.0, 8.0, 16.0]])
    g = reaches.stage_for_discharge(stages, Q, [10.0, 15.0, 1.0, 1.0])
    np.testing.assert_array_equal(g[:2], [1.0, 3.0])           # at a table point; between (10 at 2 and 20 at 4)
    assert np.isnan(g[2])                                       # a NaN curve
    assert g[3] == 0.0                                          # below the first point: the first stage
    g = reaches.stage_for_discharge(stages, Q, [20.0, 20.0, 2.0, 16.0])
    np.testing.assert_array_equal(g[[0, 1, 3]], [1.5, 4.0, 4.0])
    g = reaches.stage_for_discharge(stages, Q, [90.000001, -1.0, 1.0, np.nan])
    assert np.isnan(g).all()                                    # above the table, negative, NaN curve, NaN
    np.testing.assert_array_equal(reaches.stage_for_discharge(stages, Q[:1], 60.0), [3.0])
    with pytest.raises(ValueError):
        reaches.stage_for_discharge(stages, Q[:, :3], 1.0)
    with pytest.raises(ValueError):
        reaches.stage_for_discharge(stages, Q, [1.0, 2.0])
