"""CPU (not gpu): descriptools_amd.mfd refuses bad arguments with ValueError before any library call, d8_shares does
what it says, and the numpy reference the GPU tests compare against (tests/_mfd_ref.py) gives the shares and sums
worked out by hand from the definition: a 3 x 3 cone, a plane tilted to the east, a plane tilted along a diagonal."""
import numpy as np
import pytest

import oracle
from descriptools_amd import _lib, mfd

import _mfd_ref as R

U = 32768


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", refuse)


def _sh(shape=(5, 6)):
    return np.zeros(shape + (8,), np.uint16)


# ---- argument checks ----------------------------------------------------------------------------------------------
def test_flow_shares_value_errors(no_library):
    dem = np.arange(30, dtype=np.float32).reshape(5, 6)
    with pytest.raises(ValueError, match="2-D"):
        mfd.flow_shares(dem.reshape(-1))
    with pytest.raises(ValueError, match="2-D"):
        mfd.flow_shares(dem.reshape(5, 6, 1))
    with pytest.raises(ValueError, match="shape"):
        mfd.flow_shares(dem, fdr=np.ones((5, 7), np.uint8))
    with pytest.raises(ValueError, match="2-D"):
        mfd.flow_shares(dem, fdr=np.ones(30, np.uint8))
    for p in (True, False, float("nan"), float("inf"), -0.5, -1, 64.5, 100, "steep", None, np.bool_(True)):
        with pytest.raises(ValueError, match="exponent"):
            mfd.flow_shares(dem, exponent=p)
    for c in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="contour"):
            mfd.flow_shares(dem, contour=c)
    with pytest.raises(ValueError, match="float32"):
        mfd.flow_shares(dem.astype(np.float64) + 1e-9)
    big = np.broadcast_to(np.float32(1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
    with pytest.raises(ValueError, match="2\\^31"):
        mfd.flow_shares(big)


@pytest.mark.parametrize("call", [mfd.accumulate, lambda s, **k: mfd.specific_catchment_area(s, 10.0, **k)])
def test_accumulate_value_errors(no_library, call):
    with pytest.raises(ValueError, match=r"\(H, W, 8\)"):
        call(np.zeros((5, 6), np.uint16))
    with pytest.raises(ValueError, match=r"\(H, W, 8\)"):
        call(np.zeros((5, 6, 4), np.uint16))
    with pytest.raises(ValueError, match=r"\(H, W, 8\)"):
        call(np.zeros((5, 6, 8, 1), np.uint16))
    for dt in (np.int16, np.uint8, np.int32, np.float32):
        with pytest.raises(ValueError, match="uint16"):
            call(np.zeros((5, 6, 8), dt))
    s = _sh()
    s[2, 3, 4] = U + 1  # a slot above 32768
    with pytest.raises(ValueError, match="flat index 15"):
        call(s)
    s = _sh()
    s[2, 3, 0], s[2, 3, 5] = 20000, 12767  # a sum that is neither 0 nor 32768
    with pytest.raises(ValueError, match="flat index 15"):
        call(s)
    s = _sh()
    s[2, 3, 0] = s[2, 3, 1] = U  # twice the whole
    with pytest.raises(ValueError, match="flat index 15"):
        call(s)
    s = _sh()
    s[4, 5, :7] = 0xFFFF  # a partial nodata word
    with pytest.raises(ValueError, match="flat index 29"):
        call(s)
    with pytest.raises(ValueError):
        R.accumulate(s)
    big = np.broadcast_to(np.uint16(0), (1 << 16, 1 << 15, 8))
    with pytest.raises(ValueError, match="2\\^31"):
        call(big)
    # the weights and frac_bits refusals of flowacc.accumulate_weighted
    s = _sh()
    with pytest.raises(ValueError, match="shape"):
        call(s, weights=np.ones((6, 5)))
    for w in (np.full((5, 6), -1.0), np.full((5, 6), np.nan), np.full((5, 6), np.inf),
              np.full((5, 6), "x", dtype=object)):
        with pytest.raises(ValueError, match="weights"):
            call(s, weights=w)
    for fb in (1.5, True, "3", 5000):
        with pytest.raises(ValueError, match="frac_bits"):
            call(s, frac_bits=fb)
    with pytest.raises(ValueError, match="too fine"):
        call(s, frac_bits=50)  # 30 cells * 2^50 > 2^52
    with pytest.raises(ValueError, match="too fine"):
        call(s, weights=np.full((5, 6), 1000.0), frac_bits=45)


def test_specific_catchment_area_px(no_library):
    for px in (0.0, -1.0, float("nan"), float("inf"), "wide", True):
        with pytest.raises(ValueError, match="px"):
            mfd.specific_catchment_area(_sh(), px)


def test_alias_module():
    import descriptools.mfd
    for name in ("flow_shares", "accumulate", "specific_catchment_area", "d8_shares"):
        assert getattr(descriptools.mfd, name) is getattr(mfd, name)
        assert name in descriptools.mfd.__all__


def test_d8_shares(no_library):
    fdr = np.array([[1, 128, 64, 32], [16, 8, 4, 2], [0, 3, 255, 1]], np.uint8)
    s = mfd.d8_shares(fdr)
    assert s.dtype == np.uint16 and s.shape == (3, 4, 8) and s.flags.c_contiguous
    want = np.zeros((3, 4, 8), np.uint16)
    for (y, x), k in {(0, 0): 0, (0, 1): 1, (0, 2): 2, (0, 3): 3, (1, 0): 4, (1, 1): 5, (1, 2): 6, (1, 3): 7,
                      (2, 3): 0}.items():
        want[y, x, k] = U
    np.testing.assert_array_equal(s, want)  # 0, 3 and 255 are no code: no receiver
    np.testing.assert_array_equal(R.d8_shares(fdr), want)
    with pytest.raises(ValueError, match="2-D"):
        mfd.d8_shares(fdr.reshape(-1))


# ---- the reference against cases worked by hand ---------------------------------------------------------------------
def _cone():
    return np.array([[7, 8, 7], [8, 10, 8], [7, 8, 7]], np.float32)


def test_cone_by_hand():
    # exponent 0: eight receivers with f = 1, F = 8, r = 1 / 8: 4096 each; the main one (E, the first of equals) keeps
    # 32768 - 7 * 4096 = 4096
    s = R.flow_shares(_cone(), 0)
    assert s[1, 1].tolist() == [4096] * 8
    # exponent 0 with contour: f = 0.5 (even k), 0.35355339 (odd k); F = 2 + 1.41421356 = 3.41421356;
    # r = 0.14644661 -> floor(4798.76) and 0.10355339 -> floor(3393.24); main E: 32768 - 3 * 4798 - 4 * 3393 = 4802
    s = R.flow_shares(_cone(), 0, contour=True)
    assert s[1, 1].tolist() == [4802, 3393, 4798, 3393, 4798, 3393, 4798, 3393]
    # exponent 1: g = 2 (cardinal), 3 / 1.41421356 = 2.12132034 (diagonal, the largest); u = 0.94280904, 1;
    # F = 4 * 0.94280904 + 4 = 7.77123617; r = 0.12132034 -> floor(3975.42), 0.12867966 -> floor(4216.57);
    # main NE (the first diagonal): 32768 - 4 * 3975 - 3 * 4216 = 4220
    s = R.flow_shares(_cone(), 1)
    assert s[1, 1].tolist() == [3975, 4220, 3975, 4216, 3975, 4216, 3975, 4216]
    # the corners are lowest: no receiver; the edge cells send everything to their two corners
    assert s[0, 0].tolist() == [0] * 8 and s[2, 2].tolist() == [0] * 8
    assert s[0, 1].tolist() == [U // 2, 0, 0, 0, U // 2, 0, 0, 0]
    assert (s.sum(axis=2, dtype=np.int64) % U == 0).all()
    # nodata, NaN and +inf centres, and a pit with and without a D8 code
    dem = _cone()
    dem[0, 0], dem[0, 2], dem[2, 0], dem[1, 1] = -100, np.nan, np.inf, 1
    s = R.flow_shares(dem, 1.1)
    assert s[0, 0].tolist() == [0xFFFF] * 8 and s[0, 2].tolist() == [0] * 8 and s[2, 0].tolist() == [0] * 8
    assert s[1, 1].tolist() == [0] * 8
    fdr = np.zeros((3, 3), np.uint8)
    fdr[1, 1] = 4  # S
    assert R.flow_shares(dem, 1.1, fdr=fdr)[1, 1].tolist() == [0, 0, 0, 0, 0, 0, U, 0]
    for code in (32, 128, 8):  # NW is nodata, NE is NaN, SW is +inf: no fallback
        fdr[1, 1] = code
        assert R.flow_shares(dem, 1.1, fdr=fdr)[1, 1].tolist() == [0] * 8
    dem[0, 1] = -np.inf  # -inf is nodata
    assert R.flow_shares(dem, 1.1)[0, 1].tolist() == [0xFFFF] * 8


def test_plane_tilted_east_by_hand():
    yy, xx = np.mgrid[0:5, 0:6]
    dem = (100 - xx).astype(np.float32)
    # interior: E (g = 1), NE and SE (g = 0.70710678); u = 1, 0.70710678; F = 2.41421356; r = 0.41421356, 0.29289322
    # -> floor(9597.53) = 9597 to each diagonal, 32768 - 2 * 9597 = 13574 to E
    for px_free in (1, 1.0):
        s = R.flow_shares(dem, px_free)
        assert (s[1:-1, 1:-1] == np.array([13574, 9597, 0, 0, 0, 0, 0, 9597], np.uint16)).all()
    # top row: no NE: E 1 / 1.70710678 = 0.58578644 -> main, SE floor(0.41421356 * 32768) = 13572
    assert s[0, 2].tolist() == [U - 13572, 0, 0, 0, 0, 0, 0, 13572]
    assert (s[:, -1] == 0).all(), "the last column has no lower neighbour"
    res, x = R.accumulate(s, frac_bits=0, full=True)
    assert x["done"].all() and res[:, 0].tolist() == [0] * 5
    assert int(x["q"].sum()) == int(x["T"].reshape(5, 6)[:, -1].sum()), "everything arrives in the last column"


def test_plane_tilted_along_a_diagonal_by_hand():
    yy, xx = np.mgrid[0:5, 0:5]
    dem = (100 - xx - yy).astype(np.float32)
    # interior: E and S (g = 1), SE (g = 2 / 1.41421356 = 1.41421356, the largest); u = 0.70710678 twice and 1:
    # the two equal side receivers get floor(0.29289322 * 32768) = 9597 each, SE keeps 13574
    s = R.flow_shares(dem, 1)
    assert (s[1:-1, 1:-1] == np.array([9597, 0, 0, 0, 0, 0, 9597, 13574], np.uint16)).all()
    # exponent 0: three equal f; the first of equals in octant order (E) is the main receiver and keeps the
    # remainder of the two floors: floor(32768 / 3) = 10922 to S and SE, 10924 to E
    s = R.flow_shares(dem, 0)
    assert (s[1:-1, 1:-1] == np.array([10924, 0, 0, 0, 0, 0, 10922, 10922], np.uint16)).all()


def test_accumulate_by_hand():
    # A -> E 10924 (main, the first of the largest), S 10922, SE 10922;  B -> S;  C -> E;  D holds
    s = np.zeros((2, 2, 8), np.uint16)
    s[0, 0, 0], s[0, 0, 6], s[0, 0, 7] = 10924, 10922, 10922
    s[0, 1, 6] = U
    s[1, 0, 0] = U
    # frac_bits 0: A's total 1 splits as floor(10922 / 32768) = 0 twice, the main receiver takes the 1
    np.testing.assert_array_equal(R.accumulate(s, frac_bits=0), [[0, 1], [0, 3]])
    # frac_bits 15: q = 32768; A sends 10924 to B, 10922 to C and to D
    np.testing.assert_array_equal(R.accumulate(s, frac_bits=15), [[0, 10924 / U], [10922 / U, 3]])
    # equal largest shares: the first in octant order is the main receiver and takes the odd unit
    s[0, 0] = 0
    s[0, 0, 0] = s[0, 0, 6] = U // 2
    np.testing.assert_array_equal(R.accumulate(s, frac_bits=0), [[0, 1], [0, 3]])
    np.testing.assert_array_equal(R.accumulate(s, np.full((2, 2), 3), 0), [[0, 2], [1, 9]])
    # a share into nodata or off the raster leaves the domain; a cycle gives -100 on and below it
    s[1, 1] = 0xFFFF
    res, x = R.accumulate(s, frac_bits=0, full=True)
    np.testing.assert_array_equal(res, [[0, 1], [0, -100]])
    assert x["left"] == 0 and int(x["T"][1]) == 2 and int(x["T"][2]) == 1, "B and C have no edge: they hold"
    s = np.zeros((1, 4, 8), np.uint16)
    s[0, 0, 0] = s[0, 1, 0] = s[0, 3, 4] = U
    s[0, 2, 4], s[0, 2, 0] = U // 2, U // 2
    np.testing.assert_array_equal(R.accumulate(s, frac_bits=0), [[0, -100, -100, -100]])


def test_d8_equivalence_with_oracle_flowacc():
    dem = oracle.synth_dem(2, 70, 67)
    _, fdr = oracle.slope_d8(dem, 10.0)
    ref = oracle.flowacc(fdr)
    got = R.accumulate(R.d8_shares(fdr), frac_bits=0)
    cyc = ref == -100
    np.testing.assert_array_equal(got[~cyc], ref[~cyc].astype(np.float64))
    assert (got[cyc] == -100).all()


@pytest.mark.parametrize("exponent,contour", [(1, False), (1.1, False), (4, True), (0, False)])
def test_share_invariants_and_mass_conservation(exponent, contour):
    dem = oracle.synth_dem(7, 90, 120, nodata_pct=2)
    fdr, filled = oracle.condition_d8(dem, 10.0)
    s = R.flow_shares(filled, exponent, contour, fdr)
    nod = (s == 0xFFFF).all(axis=2)
    np.testing.assert_array_equal(nod, filled <= -100)
    tot = s.sum(axis=2, dtype=np.int64)
    assert np.isin(tot[~nod], (0, U)).all() and (s[~nod] <= U).all()
    assert (s[~nod].max(axis=1)[tot[~nod] == U] >= 4096).all(), "the main share is at least an eighth"
    res, x = R.accumulate(s, full=True)
    assert (x["done"] | x["nodata"]).all(), "a conditioned surface has no cycle"
    sink = x["done"] & ~x["edge"].any(axis=1)
    assert int(x["q"][~x["nodata"]].sum()) == int(x["T"][sink].sum()) + x["left"]
