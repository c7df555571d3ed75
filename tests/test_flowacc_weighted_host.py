"""CPU (not gpu): flowacc.accumulate_weighted and flowacc.accumulate refuse bad arguments with ValueError before any
library call, flowacc.weight_frac_bits follows its documented rule, and the weighted entry points are declared,
exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

from descriptools_amd import _lib, flowacc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any call into the HIP library fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(flowacc._lib, "lib", boom)


FDR = np.full((5, 7), 1, np.uint8)


@pytest.mark.parametrize("weights, what", [
    (np.ones((5, 6)), "shape"),
    (np.ones((7, 5)), "shape"),
    (np.ones((5, 7), np.complex128), "dtype"),
    (np.array([["a"] * 7] * 5), "dtype"),
    (np.full((5, 7), -1.0), ">= 0"),
    (np.full((5, 7), -1, np.int32), ">= 0"),
    (np.where(np.eye(5, 7) > 0, np.nan, 1.0), "finite"),
    (np.where(np.eye(5, 7) > 0, np.inf, 1.0), "finite"),
    (np.full((5, 7), 2 ** 53 + 1, np.int64), "2^53"),
    (np.full((5, 7), 2 ** 63, np.uint64), "2^53"),
])
def test_bad_weights_refused_before_the_library(no_library, weights, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        flowacc.accumulate_weighted(FDR, weights)


def test_negative_zero_and_one_negative_cell(no_library):
    w = np.ones((5, 7))
    w[3, 4] = -1e-300
    with pytest.raises(ValueError, match=">= 0"):
        flowacc.accumulate_weighted(FDR, w)
    with pytest.raises(ValueError, match=">= 0"):
        flowacc.weight_frac_bits(w)


def test_bad_shapes_and_frac_bits_refused_before_the_library(no_library):
    w = np.ones((5, 7))
    with pytest.raises(ValueError, match="2-D"):
        flowacc.accumulate_weighted(np.ones(7, np.uint8), np.ones(7))
    with pytest.raises(ValueError, match="dem has shape"):
        flowacc.accumulate_weighted(FDR, w, dem=np.zeros((5, 6), np.float32))
    for fb in (1.5, "3", True, None.__class__):
        with pytest.raises(ValueError, match="integer"):
            flowacc.accumulate_weighted(FDR, w, frac_bits=fb)
    with pytest.raises(ValueError, match="lie in"):
        flowacc.accumulate_weighted(FDR, w, frac_bits=5000)
    # N * rint(max w * 2^s) > 2^52: 35 cells of weight 1 allow s <= 46 (35 * 2^46 < 2^52 < 35 * 2^47)
    with pytest.raises(ValueError, match="too fine"):
        flowacc.accumulate_weighted(FDR, w, frac_bits=47)
    # integer weights whose sum can exceed 2^52 even at frac_bits=0
    with pytest.raises(ValueError, match="too fine"):
        flowacc.accumulate_weighted(FDR, np.full((5, 7), 2 ** 50, np.int64), frac_bits=0)
    # overflow of the scaled maximum itself
    with pytest.raises(ValueError, match="too fine"):
        flowacc.accumulate_weighted(FDR, np.full((5, 7), 1e300), frac_bits=2000)


def test_accumulate_refuses_bad_shapes_before_the_library(no_library):
    # a smaller dem would have the library read H * W float32 cells past the end of its mask
    with pytest.raises(ValueError, match=re.escape("dem has shape (4, 7), the direction raster (5, 7)")):
        flowacc.accumulate(FDR, np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="dem has shape"):
        flowacc.accumulate(FDR, np.zeros(35, np.float32))
    with pytest.raises(ValueError, match=re.escape("fdr must be a 2-D raster, not of shape (2, 5, 7)")):
        flowacc.accumulate(np.ones((2, 5, 7), np.uint8))
    with pytest.raises(ValueError, match="2-D"):
        flowacc.accumulate(np.ones(7, np.uint8))


def test_frac_bits_at_the_bound_passes_validation(monkeypatch):
    """the largest accepted frac_bits reaches the library (which the fixture replaces by a recorder)"""
    seen = {}

    class Rec:
        def dt_flowacc_weighted(self, *a):
            seen["s"] = a[5]
            return 0
    monkeypatch.setattr(flowacc._lib, "lib", lambda: Rec())
    flowacc.accumulate_weighted(FDR, np.ones((5, 7)), frac_bits=46)
    assert seen["s"] == 46
    flowacc.accumulate_weighted(FDR, np.ones((5, 7)))
    assert seen["s"] == flowacc.weight_frac_bits(np.ones((5, 7))) == 51 - 6 - 0
    flowacc.accumulate_weighted(FDR, np.full((5, 7), 2 ** 46, np.int64), frac_bits=0)  # 35 * 2^46 < 2^52
    assert seen["s"] == 0


def _rule(n, wmax):
    e = int(np.floor(np.log2(wmax)))
    return 51 - int(np.ceil(np.log2(n))) - e


def test_weight_frac_bits_rule(no_library):
    rng = np.random.default_rng(3)
    for shape in [(1, 1), (1, 2), (3, 3), (64, 64), (65, 64), (1000, 1)]:
        w = rng.random(shape) * 7.3 + 0.01
        n = int(np.prod(shape))
        assert flowacc.weight_frac_bits(w) == _rule(n, float(w.max()))
    # the bound holds at the default scale, and one bit more would break it for a maximum just below a power of two
    w = np.full((9, 9), np.nextafter(4.0, 0.0))
    s = flowacc.weight_frac_bits(w)
    assert 81 * int(np.rint(np.ldexp(w.max(), s))) <= 2 ** 52 < 81 * int(np.rint(np.ldexp(w.max(), s + 1)))


def test_weight_frac_bits_edge_cases(no_library):
    assert flowacc.weight_frac_bits(np.zeros((4, 5))) == 0            # all zeros: s = 0
    assert flowacc.weight_frac_bits(np.zeros((0, 5))) == 0            # no cells
    assert flowacc.weight_frac_bits(np.array([[1.0]])) == 51           # single cell: ceil(log2 1) = 0
    assert flowacc.weight_frac_bits(np.array([[5.0]])) == 49
    assert flowacc.weight_frac_bits(np.full((2, 2), 8.0)) == 51 - 2 - 3  # max an exact power of two: e = 3
    assert flowacc.weight_frac_bits(np.full((2, 2), 0.25)) == 51 - 2 + 2
    assert flowacc.weight_frac_bits(np.array([[5e-324, 0.0]])) == 51 - 1 + 1074  # subnormal maximum
    assert flowacc.weight_frac_bits(np.ones((4, 4), np.int32)) == 47
    assert flowacc.weight_frac_bits(np.ones((4, 4), np.bool_)) == 47
    assert flowacc.weight_frac_bits(np.full((3, 3), 2.0 ** 60)) == 51 - 4 - 60  # negative scales are fine
    assert flowacc.weight_frac_bits([[1, 2], [3, 4]]) == 51 - 2 - 2  # lists


def test_weighted_symbols_declared_exported_and_bound():
    from descriptools_amd import build
    txt = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in ("dt_flowacc_weighted", "dt_dev_flowacc_weighted"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in _lib.exported_symbols(), name
    assert re.search(r"#define\s+DT_STATUS_BAD_WEIGHT\s+4\b", txt)
    res, args = _lib._SIGS["dt_flowacc_weighted"]
    assert args == [_lib.c_u8p, _lib.c_f32p, _lib.c_f64p, _lib.i64, _lib.i64, _lib.ci, _lib.c_f64p]
    assert len(_lib._SIGS["dt_dev_flowacc_weighted"][1]) == 8
    import inspect
    assert list(inspect.signature(flowacc.accumulate_weighted).parameters) == ["fdr", "weights", "dem", "frac_bits"]
    assert list(inspect.signature(flowacc.accumulate).parameters) == ["fdr", "dem"]
