"""CPU (not gpu): the numpy reference of the focal statistics (tests/_focal_ref.py) is pinned here against a brute-force
sum in Python integers -- on a raster with nodata, NaN, +-inf and a below-sentinel height, and on a raster whose q^2
table wraps 2^64 -- and so are qmax, default_frac_bits and the argument checks of descriptools_amd.focal, which run
before any library call."""
import math

import numpy as np
import pytest

import _focal_ref as R
from descriptools_amd import focal


def _assert_brute(dem, radius, origin, frac_bits):
    ok, _, n, A, B = R.nab(dem, radius, origin, frac_bits)
    rows = R.brute(dem, radius, origin, frac_bits)
    assert len(rows) == int(ok.sum()) > 0
    for y, x, bn, bA, bB in rows:
        assert (int(n[y, x]), int(A[y, x]), int(B[y, x])) == (bn, bA, bB), (y, x)
        assert 0 <= bB < 2 ** 63 and abs(bA) < 2 ** 63


@pytest.mark.parametrize("radius", [1, 5, 50])
def test_reference_integers_equal_brute_force(radius):
    dem = R.terrain(37, 45, seed=11)
    ok = R.valid(dem)
    assert 0.03 < 1 - ok.mean() < 0.2
    assert np.isnan(dem).sum() == 1 and np.isinf(dem).sum() == 2 and (dem == -150).sum() == 1
    assert radius != 50 or radius >= max(dem.shape)
    _assert_brute(dem, radius, R.default_origin(dem), 8)


def test_reference_is_exact_where_the_table_wraps():
    dem = R.wrap_case()
    ok, q = R.quantise(dem, R.WRAP["origin"], R.WRAP["frac_bits"])
    assert ok.all()
    total = sum(int(v) ** 2 for v in q.reshape(-1))
    assert total > 2 ** 64, total / 2 ** 64
    assert int(q.max()) <= R.qmax(R.WRAP["radius"]) and 121 * int(q.max()) ** 2 < 2 ** 63
    P2 = R.planes(ok, q)[2]
    assert int(P2[-1, -1]) == total % 2 ** 64 != total
    _assert_brute(dem, **R.WRAP)


def test_qmax():
    assert focal.qmax(1) == R.qmax(1) == 1012333499      # 2^31.5 / 3 = 1012333499.99
    assert focal.qmax(4096) == R.qmax(4096) == 370682    # 2^31.5 / 8193 = 370682.35
    for r in (1, 2, 7, 64, 1000, 4096):
        m, q = (2 * r + 1) ** 2, focal.qmax(r)
        assert m * q * q < 2 ** 63 <= m * (q + 1) ** 2


def _two(lo, hi):
    return np.array([[lo, hi]], np.float32)


def test_default_frac_bits_on_both_sides_of_a_bound():
    # radius 4096: qmax = 370682.  370682 / 16 is a float32: at s = 4 the top height quantises to the bound itself
    assert focal.default_frac_bits(_two(0, 370682 / 16), 4096) == 4
    assert focal.default_frac_bits(_two(0, 370683 / 16), 4096) == 3   # rint(185341.5) = 185342 fits, 370683 does not
    assert focal.default_frac_bits(_two(0, 370682), 4096) == 0
    with pytest.raises(ValueError, match="370683.*4096|4096.*370683"):
        focal.default_frac_bits(_two(0, 370683), 4096)
    # 2^-16 m is the ceiling
    assert focal.default_frac_bits(_two(0, 1), 1) == 16
    assert focal.default_frac_bits(_two(0, 15446), 1) == 16          # 15446 * 65536 = 1012269056 <= 1012333499
    assert focal.default_frac_bits(_two(0, 15448), 1) == 15          # 15448 * 65536 = 1012400128 is over
    # origin = floor(min valid height): only the range above it counts
    assert focal.default_frac_bits(_two(1000.5, 1000 + 370682 / 16), 4096) == 4     # from 0 it would be 3
    assert focal.default_frac_bits(_two(1000.5, 1000 + 370682 / 16), 4096, origin=0.0) == 3
    assert focal.default_frac_bits(np.full((3, 3), -100, np.float32), 4096) == 16  # no valid cell
    assert focal.default_frac_bits(_two(0, 370683), 4096, origin=1.0) == 0


def test_alias_module_and_constants():
    import descriptools.focal
    assert descriptools.focal.statistics is focal.statistics and descriptools.focal.dev_max is focal.dev_max
    assert descriptools.focal.OUTPUTS == focal.OUTPUTS == R.OUTPUTS == ("count", "mean", "std", "tpi", "dev")
    assert (focal.RADIUS_MAX, focal.RADII_MAX, focal.FRAC_BITS_MAX) == (4096, 32, 24)
    for name in ("mean", "std", "tpi", "dev", "default_frac_bits", "qmax"):
        assert callable(getattr(descriptools.focal, name))


def test_docstring_carries_the_formulas():
    doc = " ".join(focal.__doc__.split())
    for piece in ("rint((float64(z) - origin) * 2^s)", "A = S1 - n q_c", "B = S2 - 2 q_c S1 + n q_c^2",
                  "(2 R + 1)^2 qmax^2 < 2^63", "a = float64(A) / nf", "var = b - a a", "origin + (float64(q_c) + a) u",
                  "(-a) / sd", "a tie keeps the smaller radius", "modulo 2^64"):
        assert piece in doc, piece


def test_source_is_in_the_build():
    from descriptools_amd import build
    assert "dt_focal.hip" in build.SOURCES


DEM = np.zeros((6, 7), np.float32)
HILL = np.array([[0, 250, 1000]], np.float32)


@pytest.mark.parametrize("call", [
    lambda: focal.statistics(np.zeros(5, np.float32), 2),                           # not 2-D
    lambda: focal.statistics(np.zeros((2, 3, 4), np.float32), 2),
    lambda: focal.dev_max(np.zeros(5, np.float32), (1, 2)),
    lambda: focal.statistics(np.array([[0.1, 0.2]], np.float64), 2),                # float32 cannot hold it
    lambda: focal.dev_max(np.array([[0.1, 0.2]], np.float64), (1, 2)),
    lambda: focal.default_frac_bits(np.array([[0.1, 0.2]], np.float64), 2),
    lambda: focal.statistics(DEM, 0),
    lambda: focal.statistics(DEM, 4097),
    lambda: focal.statistics(DEM, 1.5),
    lambda: focal.statistics(DEM, True),
    lambda: focal.statistics(DEM, None),
    lambda: focal.tpi(DEM, 0),
    lambda: focal.dev(DEM, 4097),
    lambda: focal.mean(DEM, 1.5),
    lambda: focal.std(DEM, None),
    lambda: focal.default_frac_bits(DEM, 0),
    lambda: focal.dev_max(DEM, ()),
    lambda: focal.dev_max(DEM, tuple(range(1, 34))),                                # 33 radii
    lambda: focal.dev_max(DEM, (3, 2)),
    lambda: focal.dev_max(DEM, (2, 3, 3)),
    lambda: focal.dev_max(DEM, (0, 3)),
    lambda: focal.dev_max(DEM, (3, 4097)),
    lambda: focal.dev_max(DEM, (1, 2.0)),
    lambda: focal.dev_max(DEM, 3),
    lambda: focal.dev_max(DEM, None),
    lambda: focal.statistics(DEM, 2, outputs=()),
    lambda: focal.statistics(DEM, 2, outputs="tpi"),
    lambda: focal.statistics(DEM, 2, outputs=None),
    lambda: focal.statistics(DEM, 2, outputs=("tpi", "tpi")),
    lambda: focal.statistics(DEM, 2, outputs=("tpi", "range")),
    lambda: focal.statistics(DEM, 2, outputs=("dev", 3)),
    lambda: focal.statistics(DEM, 2, frac_bits=-1),
    lambda: focal.statistics(DEM, 2, frac_bits=25),
    lambda: focal.statistics(DEM, 2, frac_bits=1.0),
    lambda: focal.statistics(DEM, 2, frac_bits=True),
    lambda: focal.dev_max(DEM, (1, 2), frac_bits=25),
    lambda: focal.statistics(DEM, 2, origin=float("nan")),
    lambda: focal.statistics(DEM, 2, origin=float("inf")),
    lambda: focal.statistics(DEM, 2, origin="sea"),
    lambda: focal.dev_max(DEM, (1, 2), origin=float("-inf")),
    lambda: focal.statistics(DEM, 2, origin=1.0),                                   # above the smallest height
    lambda: focal.dev_max(HILL, (1, 2), origin=0.5),
    lambda: focal.statistics(HILL, 4096, frac_bits=16),                             # 1000 * 2^16 > qmax(4096)
    lambda: focal.statistics(HILL, 4096, frac_bits=9),                              # 512000 > 370682
    lambda: focal.dev_max(HILL, (1, 4096), frac_bits=9),
    lambda: focal.statistics(HILL, 4096, origin=-400000.0),                         # no frac_bits fits
])
def test_bad_arguments_raise_value_error(call, monkeypatch):
    from descriptools_amd import _lib

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError):
        call()


def test_contract_holds_on_the_edge_without_a_library_call(monkeypatch):
    """the same checks let a call through that sits on the bound: it reaches the library"""
    from descriptools_amd import _lib

    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "lib", reached)
    with pytest.raises(Reached):
        focal.statistics(HILL, 4096, frac_bits=8)    # 256000 <= 370682
    with pytest.raises(Reached):
        focal.statistics(HILL, 4096, origin=0.0)
    with pytest.raises(Reached):
        focal.dev_max(HILL, (1, 4096))


def test_too_many_cells_is_refused():
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 16, 2 ** 15), (0, 0))
    with pytest.raises(ValueError, match="2\\^31"):
        focal.statistics(big, 3)
    with pytest.raises(ValueError, match="2\\^31"):
        focal.dev_max(big, (1, 2))
