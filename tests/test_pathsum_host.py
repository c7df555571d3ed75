"""CPU (not gpu): flowpath.downstream_sum / upslope_longest / travel_time / time_of_concentration refuse bad arguments
with ValueError before any library call, call the bound dt_flowpath_downstream_sum / dt_flowpath_upslope_longest with
what they should, and the entry points are declared, exported and bound; step_length and path_frac_bits.  The reference
that the GPU tests hold the kernels to (tests/_pathsum_ref.py) is checked here on hand-built cases with literal expected
arrays, and the identities the kernels rest on are checked on it in exact integers: U = M - T, T defined exactly where
drainage has a target, max T <= 2^52, and sum T = sum q * (defined cells whose path leaves through the cell)."""
import os
import re

import numpy as np
import pytest

import oracle
from descriptools_amd import _lib, flowacc, flowpath

import _pathsum_ref as R
import _watershed_ref as WR
from _watershed_ref import E, N, S, SE, SW, W_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dt_flowpath_downstream_sum", "dt_flowpath_upslope_longest", "dt_dev_flowpath_downstream_sum",
           "dt_dev_flowpath_upslope_longest")


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_reference_on_hand_cases(name):
    c = R.hand_cases()[name]
    dn = R.downstream_sum(c["fdr"], c["weights"], c["dem"], c["stop"], c["frac_bits"])
    up = R.upslope_longest(c["fdr"], c["weights"], c["dem"], c["frac_bits"])
    assert dn.dtype == up.dtype == np.float64
    np.testing.assert_array_equal(dn, c["dn"])
    np.testing.assert_array_equal(up, c["up"])


@pytest.fixture(scope="module")
def planted():
    """90 x 140 with planted cycles, noise codes and a nodata block"""
    H, W = 90, 140
    fdr, _ = R.field(H, W, 41, cycles=5, ring=(60, 30))
    dem = np.ones((H, W), np.float32)
    dem[70:82, 100:125] = -100
    rng = np.random.default_rng(9)
    w = rng.random((H, W)) * 30.0
    s = R.default_frac_bits(w)
    stop = rng.random((H, W)) < 0.01
    stop[75, 110] = True                                 # on nodata: ignored
    stop[H // 3, W // 4 + 7] = True                      # on the long cycle
    return fdr, dem, R.quantise(w, s), stop


def test_longest_is_upslope_max_minus_sum(planted):
    fdr, dem, q, _ = planted
    T = R.sums(fdr, q, dem)
    U = R.longest(fdr, q, dem)
    ok = T >= 0
    assert ok.any() and (~ok & (dem.reshape(-1) > -100)).any()
    M = np.where(ok, T, -1)
    for cells, src, _, _ in R.walk_paths(fdr, q, dem, None, R.sources(fdr, dem, ok)):
        np.maximum.at(M, cells, T[src])
    np.testing.assert_array_equal(U[ok], (M - T)[ok])
    np.testing.assert_array_equal(U[~ok], -1)
    assert (U[ok] >= 0).all() and U.max() > 0


@pytest.mark.parametrize("stopped", [False, True])
def test_sum_is_defined_where_drainage_has_a_target(planted, stopped):
    fdr, dem, q, stop = planted
    st = stop if stopped else None
    T = R.sums(fdr, q, dem, st).reshape(fdr.shape)
    target = WR.drainage(fdr, 1.0, dem, None if st is None else st.astype(np.int64))[0]
    np.testing.assert_array_equal(T >= 0, target >= 0)
    assert (T >= 0).any() and (T < 0).any()
    assert int(T.max()) <= 2 ** 52
    if stopped:
        assert (T[stop & (dem > -100)] == 0).all()
        ring = T[fdr.shape[0] // 3, fdr.shape[1] // 4:fdr.shape[1] // 4 + 60]
        assert (ring >= 0).all()                         # the stop cell on the long cycle defines its cells


@pytest.mark.parametrize("stopped", [False, True])
def test_sum_of_sums_counts_every_move_once_per_path(planted, stopped):
    fdr, dem, q, stop = planted
    st = stop if stopped else None
    T = R.sums(fdr, q, dem, st)
    ok = T >= 0
    through = np.zeros(fdr.size, np.int64)               # defined cells whose path leaves through the cell
    for cells, _, _, go in R.walk_paths(fdr, q, dem, st, np.flatnonzero(ok)):
        np.add.at(through, cells[go], 1)
    total = sum(int(a) * int(b) for a, b in zip(q.reshape(-1)[through > 0], through[through > 0]))
    assert sum(int(t) for t in T[ok]) == total and total > 0


def test_sum_of_sums_on_an_acyclic_field_is_the_weighted_accumulation():
    rng = np.random.default_rng(2)
    fdr = rng.choice(np.array([E, S, SE, SW], np.uint8), size=(70, 90))
    q = rng.integers(0, 1000, fdr.shape)
    T = R.sums(fdr, q)
    assert (T >= 0).all()
    acc = oracle.flowacc(fdr)
    moving = WR.graph(fdr)[1].reshape(fdr.shape) >= 0
    assert int(T.sum()) == int((q * (acc + 1))[moving].sum())


def test_step_length():
    r2 = np.sqrt(2.0)
    fdr = np.array([[E, SE, S, 0], [SW, W_, 3, 128], [N, 32, 64, 255]], np.uint8)
    want = np.array([[2.0, 2 * r2, 2.0, 0], [0, 2.0, 0, 0], [2.0, 2 * r2, 2.0, 0]])
    got = flowpath.step_length(fdr, 2.0)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    dem = np.ones((3, 4), np.float32)
    dem[1, 1] = -100
    dem[1, 0] = -250
    want_d = want.copy()
    want_d[1, 1] = want_d[1, 0] = 0                      # nodata cells
    want_d[2, 0] = want_d[2, 1] = 0                      # N and NW into nodata
    np.testing.assert_array_equal(flowpath.step_length(fdr, 2.0, dem), want_d)
    fdr_r, dem_r = R.field(60, 80, 3, cycles=3, nodata=True, ring=(30, 20))
    for d in (None, dem_r):
        np.testing.assert_array_equal(flowpath.step_length(fdr_r, 7.5, d), R.step_length(fdr_r, 7.5, d))
    assert flowpath.step_length(np.zeros((0, 5), np.uint8), 1.0).shape == (0, 5)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "wide"):
        with pytest.raises(ValueError, match="px"):
            flowpath.step_length(fdr, bad)
    with pytest.raises(ValueError, match="2-D"):
        flowpath.step_length(np.ones(5, np.uint8), 1.0)
    with pytest.raises(ValueError, match="shape"):
        flowpath.step_length(fdr, 1.0, np.ones((4, 3), np.float32))


def test_path_frac_bits():
    rng = np.random.default_rng(1)
    for shape, scale in (((5, 7), 1.0), ((128, 192), 37.5), ((100, 3), 1e9), ((9, 9), 2.0 ** -30), ((4, 4), 1.0)):
        w = rng.random(shape) * scale
        if shape == (4, 4):
            w[:] = 1.0                                   # a power of two on the nose
        s = flowpath.path_frac_bits(w)
        assert s == flowacc.weight_frac_bits(w) == R.default_frac_bits(w)
        n, top = w.size, float(w.max())
        # within the bound, and at most two bits coarser than the finest scale within it
        assert n * int(np.rint(np.ldexp(top, s))) <= 2 ** 52 < n * int(np.rint(np.ldexp(top, s + 2)))
    assert flowpath.path_frac_bits(np.zeros((3, 3))) == 0
    assert flowpath.path_frac_bits(np.zeros((0, 3))) == 0
    assert flowpath.path_frac_bits(np.ones((2, 2), np.int16)) == 49
    for bad, what in ((np.array([[1.0, -1.0]]), ">= 0"), (np.array([[np.nan, 1.0]]), "finite"),
                      (np.array([[1j]]), "real")):
        with pytest.raises(ValueError, match=what):
            flowpath.path_frac_bits(bad)


FDR = np.full((5, 7), E, np.uint8)
ONE = np.ones((5, 7), np.float64)


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
    (dict(weights=np.ones((5, 6))), "shape"),
    (dict(weights=np.ones(35)), "shape"),
    (dict(weights=np.full((5, 7), -1.0)), ">= 0"),
    (dict(weights=np.full((5, 7), -1, np.int32)), ">= 0"),
    (dict(weights=np.full((5, 7), np.nan)), "finite"),
    (dict(weights=np.full((5, 7), np.inf)), "finite"),
    (dict(weights=np.full((5, 7), 1j)), "real"),
    (dict(weights=np.full((5, 7), "a")), "real"),
    (dict(dem=np.ones((7, 5), np.float32)), "shape"),
    (dict(frac_bits=1.0), "frac_bits must be an integer"),
    (dict(frac_bits=True), "frac_bits must be an integer"),
    (dict(frac_bits="fine"), "frac_bits must be an integer"),
    (dict(frac_bits=2201), "frac_bits must lie"),
    (dict(frac_bits=-2201), "frac_bits must lie"),
    (dict(frac_bits=48), "too fine"),                    # 35 * 2^48 > 2^52
])
def test_both_refuse_before_the_library(no_library, kw, what):
    args = dict(fdr=FDR, weights=ONE, dem=None, frac_bits=None)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        flowpath.downstream_sum(**args)
    with pytest.raises(ValueError, match=what):
        flowpath.upslope_longest(**args)


@pytest.mark.parametrize("stop, what", [
    (np.ones((5, 7), np.float32), "integer"),
    (np.ones((5, 7), np.float64), "integer"),
    (np.ones((7, 5), np.int8), "shape"),
    (np.ones(35, bool), "2-D"),
])
def test_a_bad_stop_is_refused(no_library, stop, what):
    with pytest.raises(ValueError, match=what):
        flowpath.downstream_sum(FDR, ONE, stop=stop)
    with pytest.raises(ValueError, match=what):
        flowpath.travel_time(FDR, 10.0, ONE, stop=stop)


def test_times_refuse_before_the_library(no_library):
    fdr = np.array([[E, E, 0], [E, E, E]], np.uint8)
    dem = np.array([[1, 1, 1], [-100, 1, 1]], np.float32)
    good = np.array([[1.0, 2.0, np.nan], [-5.0, 3.0, 0.0]])   # NaN on a terminal, -5 on nodata, 0 on an edge terminal
    for fn in (flowpath.travel_time, flowpath.time_of_concentration):
        for bad, at in ((0.0, 1), (-1.0, 1), (np.nan, 0), (np.inf, 4)):
            v = good.copy()
            v.reshape(-1)[at] = bad
            with pytest.raises(ValueError, match="speed must be finite and > 0.*flat index %d" % at):
                fn(fdr, 10.0, v, dem)
        v = good.copy()
        v[0, 0] = v[0, 1] = 0.0
        with pytest.raises(ValueError, match="flat index 0"):  # the first offender
            fn(fdr, 10.0, v, dem)
        with pytest.raises(ValueError, match="shape"):
            fn(fdr, 10.0, np.ones((3, 2)), dem)
        with pytest.raises(ValueError, match="real"):
            fn(fdr, 10.0, np.full((2, 3), 1j), dem)
        with pytest.raises(ValueError, match="px"):
            fn(fdr, 0.0, good, dem)
        with pytest.raises(ValueError, match="frac_bits"):
            fn(fdr, 10.0, good, dem, frac_bits=0.5)


class _FakeLib:
    """records calls and fills the output it is given"""

    def __init__(self):
        self.calls = []

    def dt_flowpath_downstream_sum(self, f, d, w, s, H, W, frac_bits, out):
        self.calls.append(("dn", H, W, frac_bits, d is not None, s is not None,
                           np.ctypeslib.as_array(w, (H * W,)).copy(),
                           None if s is None else np.ctypeslib.as_array(s, (H * W,)).copy()))
        np.ctypeslib.as_array(out, (H * W,))[:] = 1.5
        return 0

    def dt_flowpath_upslope_longest(self, f, d, w, H, W, frac_bits, out):
        self.calls.append(("up", H, W, frac_bits, d is not None, False, np.ctypeslib.as_array(w, (H * W,)).copy(), None))
        np.ctypeslib.as_array(out, (H * W,))[:] = 2.5
        return 0


def test_calls_into_the_library(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    fdr = np.array([[E, SE, 0], [E, E, E]], np.uint8)
    dem = np.array([[1, 1, 1], [-100, 1, 1]], np.float32)
    w = np.array([[1, 2, 3], [4, 5, 6]], np.int16)
    out = flowpath.downstream_sum(fdr, w, dem, stop=np.array([[0, 2, 0], [0, 0, -1]]), frac_bits=3)
    assert out.dtype == np.float64 and (out == 1.5).all()
    out = flowpath.upslope_longest(fdr[:, ::-1], w[:, ::-1])          # not contiguous
    assert out.dtype == np.float64 and (out == 2.5).all()
    speed = np.array([[2.0, 4.0, np.nan], [0.0, 5.0, -1.0]])
    flowpath.travel_time(fdr, 10.0, speed, dem)
    flowpath.time_of_concentration(fdr, 10.0, speed, dem, frac_bits=4)
    (k0, H, W, s0, d0, st0, w0, stop0), (k1, _, _, s1, d1, _, w1, _), c2, c3 = fake.calls
    assert (k0, H, W, s0, d0, st0) == ("dn", 2, 3, 3, True, True)
    np.testing.assert_array_equal(w0, [1, 2, 3, 4, 5, 6])
    np.testing.assert_array_equal(stop0, [0, 1, 0, 0, 0, 1])
    assert (k1, s1, d1) == ("up", 51 - 3 - 2, False)                  # N = 6, max 6: s = 51 - ceil(log2 6) - 2
    np.testing.assert_array_equal(w1, [3, 2, 1, 6, 5, 4])
    tw = np.array([10.0 / 2.0, 10.0 * np.sqrt(2.0) / 4.0, 0, 0, 10.0 / 5.0, 0])
    assert c2[0] == "dn" and c2[3] == flowpath.path_frac_bits(tw) and not c2[5]
    np.testing.assert_array_equal(c2[6], tw)
    assert c3[0] == "up" and c3[3] == 4
    np.testing.assert_array_equal(c3[6], tw)


def test_declared_exported_and_bound():
    import descriptools.flowpath as alias
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib._SIGS
        assert getattr(L, name) is not None
    for name in ("downstream_sum", "upslope_longest", "path_frac_bits", "step_length", "travel_time",
                 "time_of_concentration"):
        assert getattr(alias, name) is getattr(flowpath, name)
    assert "wider than" in flowpath.__doc__ and "upslope_length" in flowpath.upslope_longest.__doc__
