"""CPU (not gpu): harmonic interpolation without a device -- the numpy reference of tests/_harmonic_ref.py against
literal tables and against its own residual; every ValueError of descriptools_amd.harmonic, raised before the library is
loaded; the void selection of fill_voids on a literal mask; the new entries in the header, the binding table and the
build (what the C entries refuse is in tests/test_gpu_harmonic.py, where a device lets them run); the alias module."""
import os

import numpy as np
import pytest

import _harmonic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference -----------------------------------------------------------------------------------------------
def test_reference_strip():
    v = np.array([[0.0, 9, 9, 9, 1.0]])
    fixed = np.array([[1, 0, 0, 0, 1]], bool)
    dom = np.ones((1, 5), bool)
    u = R.direct(v, fixed, dom)
    assert np.allclose(u, [[0, 0.25, 0.5, 0.75, 1]], rtol=0, atol=1e-15)
    assert np.array_equal(u[fixed], v[fixed])
    # the expected hitting time of the ends of a path of n free cells from cell i (1-based) is i (n + 1 - i)
    assert np.allclose(R.hitting_time(fixed, dom), [[0, 3, 4, 3, 0]], rtol=0, atol=1e-12)
    assert R.residual(u, fixed, dom).max() <= 1e-15


def test_reference_constant():
    v = np.zeros((3, 3))
    v[0, 0] = 37.5
    fixed = v != 0
    u = R.direct(v, fixed, np.ones((3, 3), bool))
    assert np.allclose(u, 37.5, rtol=0, atol=1e-12)


def test_reference_residual_is_in_the_stated_association():
    # N, W, E, S from the left: (1e16 + 1) + -1e16 + 1 is 1 in that order (1e16 + 1 rounds to 1e16), 2 in another
    u = np.array([[0, 1e16, 0], [1.0, 0.25, -1e16], [0, 1.0, 0]])
    dom = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    fixed = dom.copy()
    fixed[1, 1] = False
    avg, k = R.average(u, dom)
    assert k[1, 1] == 4 and avg[1, 1] == 0.25
    assert R.residual(u, fixed, dom)[1, 1] == 0.0
    # k counts the neighbours in the domain only, the raster's edge is no neighbour
    dom[0, 1] = False
    avg, k = R.average(u, dom)
    assert k[1, 1] == 3 and avg[1, 1] == ((1.0 + -1e16) + 1.0) / 3
    assert k[0, 0] == 1 and k[2, 2] == 2


@pytest.mark.parametrize("seed", range(4))
def test_reference_direct_has_no_residual(seed):
    rng = np.random.default_rng(seed)
    H, W = 23, 31
    dom = rng.random((H, W)) > 0.15
    fixed = dom & (rng.random((H, W)) < 0.05)
    v = np.where(fixed, rng.normal(0, 100, (H, W)).astype(np.float32), np.nan)
    u = R.direct(v, fixed, dom)
    reach = R.reachable(fixed, dom)
    assert np.array_equal(np.isnan(u), ~reach | (reach & ~fixed & (R.average(u, dom)[1] == 0)))
    assert not np.isnan(u[reach]).any()
    assert R.residual(np.where(reach, u, 0.0), fixed, reach).max() <= 1e-12
    t = R.hitting_time(fixed, dom)
    assert (t[reach & ~fixed] >= 1.0 - 1e-9).all() and (t[~reach | fixed] == 0).all()


def test_reference_rooms():
    dom = np.ones((5, 9), bool)
    dom[:, 4] = False  # a wall: the right room has no fixed cell
    fixed = np.zeros((5, 9), bool)
    fixed[2, 1] = True
    reach = R.reachable(fixed, dom)
    assert reach[:, :4].all() and not reach[:, 4:].any()
    u = R.direct(np.where(fixed, 12.25, 0.0), fixed, dom)
    assert np.allclose(u[:, :4], 12.25, rtol=0, atol=1e-12) and np.isnan(u[:, 4:]).all()


def test_reference_labels():
    m = np.array([[1, 0, 0, 1],
                  [0, 1, 0, 0],
                  [0, 0, 0, 1]])
    lab, size = R.label(m, 8)
    assert np.array_equal(lab, [[0, -100, -100, 3], [-100, 0, -100, -100], [-100, -100, -100, 11]])
    assert np.array_equal(size, [[2, 0, 0, 1], [0, 2, 0, 0], [0, 0, 0, 1]])
    lab4, size4 = R.label(m, 4)
    assert lab4[1, 1] == 5 and size4[0, 0] == 1


# ---- the argument checks: before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from descriptools_amd import _lib

    def refuse():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_value_errors(no_library):
    from descriptools_amd import harmonic
    z = np.zeros((4, 5), np.float32)
    f = np.zeros((4, 5), np.int8)
    for call in (lambda: harmonic.interpolate(np.zeros(5), np.zeros(5)),
                 lambda: harmonic.interpolate(np.zeros((2, 2, 2)), np.zeros((2, 2, 2))),
                 lambda: harmonic.interpolate(z, np.zeros((5, 4), np.int8)),
                 lambda: harmonic.interpolate(z, f, domain=np.zeros((4, 4), np.int8)),
                 lambda: harmonic.interpolate(z.astype(complex), f),
                 lambda: harmonic.fill_voids(np.zeros(7)),
                 lambda: harmonic.base_level(z, np.zeros((3, 5), np.int8)),
                 lambda: harmonic.base_level(np.zeros(3), np.zeros(3)),
                 lambda: harmonic.vdcn(z, np.zeros((4, 6), np.int8)),
                 lambda: harmonic.fill_voids(z, max_cells=-1),
                 lambda: harmonic.fill_voids(z, max_cells=2.5),
                 lambda: harmonic.fill_voids(z, max_cells=True)):
        with pytest.raises(ValueError):
            call()
    for tol in (0, -1e-5, float("nan"), float("inf"), None, "x", True):
        for call in (lambda: harmonic.interpolate(z, f, tol=tol), lambda: harmonic.base_level(z, f, tol=tol),
                     lambda: harmonic.vdcn(z, f, tol=tol), lambda: harmonic.fill_voids(z, tol=tol)):
            with pytest.raises(ValueError, match="tol"):
                call()
    for n in (0, -1, 4097, 1.5, True, None):
        with pytest.raises(ValueError, match="max_rounds"):
            harmonic.interpolate(z, f, max_rounds=n)
    big = np.broadcast_to(np.float32(1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
    src = np.broadcast_to(np.int8(0), big.shape)
    for call in (lambda: harmonic.interpolate(big, src), lambda: harmonic.fill_voids(big),
                 lambda: harmonic.base_level(big, src), lambda: harmonic.vdcn(big, src)):
        with pytest.raises(ValueError, match="2\\^31"):
            call()


# ---- the void selection ---------------------------------------------------------------------------------------------
def test_select_voids():
    from descriptools_amd import harmonic
    m = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                  [0, 1, 1, 0, 0, 0, 1, 0],
                  [0, 1, 0, 0, 1, 0, 0, 1],   # (1, 6) and (2, 7) touch by a corner: one void, on the border
                  [0, 0, 0, 0, 0, 0, 0, 0],
                  [0, 0, 1, 0, 0, 0, 0, 0],
                  [0, 0, 1, 0, 0, 0, 0, 0]])  # reaches the last row
    lab, size = R.label(m, 8)
    three = np.zeros(m.shape, bool)
    three[1, 1:3] = three[2, 1] = True
    one = np.zeros(m.shape, bool)
    one[2, 4] = True
    assert np.array_equal(harmonic.select_voids(lab, size), three | one)
    assert np.array_equal(harmonic.select_voids(lab, size, max_cells=2), one)
    assert np.array_equal(harmonic.select_voids(lab, size, max_cells=3), three | one)
    assert not harmonic.select_voids(lab, size, max_cells=0).any()
    assert np.array_equal(harmonic.select_voids(lab, size, edges=True), m != 0)
    assert np.array_equal(harmonic.select_voids(lab, size, max_cells=2, edges=True), (m != 0) & ~three)
    e = np.full((0, 4), -100, np.int64)
    assert harmonic.select_voids(e, e).shape == (0, 4)


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_built():
    from descriptools_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    for name in ("dt_harmonic", "dt_dev_harmonic"):
        assert "int %s(" % name in header
        assert name in _lib._SIGS
    assert "dt_harmonic.hip" in build.SOURCES


def test_alias_module():
    import descriptools.harmonic as alias
    from descriptools_amd import harmonic
    for name in ("interpolate", "fill_voids", "base_level", "vdcn", "select_voids", "Harmonic"):
        assert getattr(alias, name) is getattr(harmonic, name)
        assert name in alias.__all__
