"""CPU (not gpu): the numpy reference of the terrain attributes (tests/_terrain_ref.py) is pinned here -- against a
least-squares fit of the six-term quadratic, against Evans' written-out 3 x 3 formulas and on surfaces whose derivatives
are known -- and so are the argument checks of descriptools_amd.terrain, which run before any library call."""
import math

import numpy as np
import pytest

import _terrain_ref as R
from _terrain_ref import paraboloid, plane, sphere_cap
from descriptools_amd import terrain


def _centre(a, radius):
    return a[radius, radius]


# ---- the closed forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 5, 16])
def test_derivatives_equal_a_least_squares_fit(radius):
    """p, q, r, s, t against np.linalg.lstsq of z = a x^2 + b y^2 + c x y + d x + e y + f on random windows (x east,
    y north, in cells; the pixel size scales the coefficients afterwards).  rtol 1e-9: two float64 evaluations of one
    well-conditioned fit."""
    px = 7.3
    n = 2 * radius + 1
    jj, ii = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    x, y = ii.astype(np.float64).ravel(), (-jj).astype(np.float64).ravel()
    A = np.stack([x * x, y * y, x * y, x, y, np.ones_like(x)], axis=1)
    rng = np.random.default_rng(100 + radius)
    for _ in range(8):
        win = rng.uniform(0, 100, (n, n)).astype(np.float32)
        a, b, c, d, e, _f = np.linalg.lstsq(A, win.astype(np.float64).ravel(), rcond=None)[0]
        want = (d / px, e / px, 2 * a / px ** 2, c / px ** 2, 2 * b / px ** 2)
        p, q, r, s, t, has = R.derivatives(win, px, radius)
        assert has.sum() == 1 and has[radius, radius]
        got = tuple(_centre(v, radius) for v in (p, q, r, s, t))
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)


def test_radius_1_is_evans_3x3():
    rng = np.random.default_rng(7)
    h = 7.3
    for _ in range(20):
        win = rng.uniform(-50, 900, (3, 3)).astype(np.float32)
        z1, z2, z3, z4, z5, z6, z7, z8, z9 = (float(v) for v in win.ravel())  # rows from the north, columns from the west
        want = ((z3 + z6 + z9 - z1 - z4 - z7) / (6 * h),
                (z1 + z2 + z3 - z7 - z8 - z9) / (6 * h),
                (z1 + z3 + z4 + z6 + z7 + z9 - 2 * (z2 + z5 + z8)) / (3 * h * h),
                (z3 + z7 - z1 - z9) / (4 * h * h),
                (z1 + z2 + z3 + z7 + z8 + z9 - 2 * (z4 + z5 + z6)) / (3 * h * h))
        got = tuple(_centre(v, 1) for v in R.derivatives(win, h, 1)[:5])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("radius", [1, 3, 8])
def test_integer_plane_is_exact(radius):
    dem = plane(40, 50, 3, -4)
    out = R.attributes(dem, 1.0, radius=radius)
    has = out["gradient"] != -100
    assert has.sum() == (40 - 2 * radius) * (50 - 2 * radius)
    for k in ("profile", "plan", "tangential", "mean", "laplacian"):
        assert (out[k][has] == 0).all(), k
    assert (out["gradient"][has] == np.float32(5.0)).all()
    p, q = R.derivatives(dem, 1.0, radius)[:2]
    assert (p[has] == 3.0).all() and (q[has] == -4.0).all()


@pytest.mark.parametrize("radius", [1, 3, 8])
def test_integer_paraboloid_is_exact(radius):
    dem = paraboloid(41, 41)
    p, q, r, s, t, has = R.derivatives(dem, 1.0, radius)
    assert has.sum() == (41 - 2 * radius) ** 2
    assert (r[has] == 2.0).all() and (t[has] == 2.0).all() and (s[has] == 0.0).all()
    assert (R.attributes(dem, 1.0, ("laplacian",), radius)["laplacian"][has] == 4).all()
    assert p[20, 20] == 0 and q[20, 20] == 0


@pytest.mark.parametrize("radius", [1, 4])
def test_sphere_cap_has_curvature_one_over_R(radius):
    """Positive is convex: profile, tangential and mean curvature of a cap of radius R are +1 / R, within 1e-6
    relative.  The heights are float64 (float32 heights of size R carry a rounding of 3e-5, far above 1e-6 of a second
    difference h^2 / R); the pixel size is small against R because the cap is not a quadratic: the fit over a window of
    half-width radius * px is off by the order of (radius * px / R)^2 = 1.6e-7 at radius 4.  Cells within five cells
    of the apex are left out: the three divide by w = p p + q q, which is 0 there."""
    R_, px = 500.0, 0.05
    dem = sphere_cap(61, 61, R_, px)
    assert dem.dtype == np.float64
    out = R.attributes(dem, px, ("profile", "tangential", "mean", "plan", "gradient"), radius)
    sel = (out["gradient"] != -100) & (out["gradient"] > 5 * px / R_)
    assert sel.sum() > 2000
    for k in ("profile", "tangential", "mean"):
        np.testing.assert_allclose(out[k][sel].astype(np.float64), 1 / R_, rtol=1e-6, err_msg=k)
    assert (out["plan"][sel] > 0).all()


def test_sphere_cap_float32_heights_are_convex():
    """on float32 heights (what the package takes) the cap is convex in every curvature"""
    R_, px = 500.0, 5.0
    dem = sphere_cap(61, 61, R_, px).astype(np.float32)
    out = R.attributes(dem, px, R.OUTPUTS, radius=4)
    sel = (out["gradient"] != -100) & (out["gradient"] > 0.05)
    assert sel.sum() > 1000
    for k in ("profile", "plan", "tangential", "mean"):
        assert (out[k][sel] > 0).all(), k
    assert (out["laplacian"][sel] < 0).all(), "z_xx + z_yy of a dome is negative: the Laplacian is not sign-flipped"


def test_aspect_of_the_four_cardinal_tilts():
    for (a, b), want in (((0, -1), 0.0), ((-1, 0), 90.0), ((0, 1), 180.0), ((1, 0), 270.0)):
        # z = a x + b y falls towards -(a, b): b = -1 rises to the south, so it faces north
        out = R.attributes(plane(9, 9, a, b), 2.0, ("aspect", "gradient"), radius=1)
        has = out["gradient"] != -100
        assert has.sum() == 49
        assert (out["aspect"][has] == np.float32(want)).all(), (a, b, out["aspect"][4, 4])
    flat = R.attributes(np.full((5, 5), 3, np.float32), 2.0, ("aspect",), radius=1)["aspect"]
    assert (flat[1:-1, 1:-1] == -1).all() and (flat[0] == -100).all()


def test_hillshade_of_a_flat_raster_is_sin_altitude():
    for alt in (45.0, 30.0, 90.0, 12.5):
        hs = R.attributes(np.full((7, 8), 120, np.float32), 10.0, ("hillshade",), 1, 315.0, alt)["hillshade"]
        assert (hs[1:-1, 1:-1] == np.float32(math.sin(math.radians(alt)))).all()
        assert terrain.sun_vector(315.0, alt) == R.sun_vector(315.0, alt)
    # a slope facing away from a low sun is dark
    out = R.attributes(plane(9, 9, 2, 0), 1.0, ("hillshade",), 1, 90.0, 20.0)["hillshade"]
    assert (out[1:-1, 1:-1] == 0).all()


def test_window_rule():
    dem = np.arange(12 * 15, dtype=np.float32).reshape(12, 15)
    dem[5, 6] = -100
    dem[9, 12] = np.nan
    dem[2, 2] = np.inf
    for radius in (1, 2):
        has = R.attributes(dem, 1.0, ("gradient",), radius)["gradient"] != -100
        want = np.zeros_like(has)
        want[radius:12 - radius, radius:15 - radius] = True
        for y, x in ((5, 6), (9, 12), (2, 2)):
            want[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = False
        assert np.array_equal(has, want)


# ---- the public interface ------------------------------------------------------------------------------------------
def test_alias_module():
    import descriptools.terrain
    assert descriptools.terrain.attributes is terrain.attributes
    assert descriptools.terrain.OUTPUTS == terrain.OUTPUTS == R.OUTPUTS
    assert terrain.OUTPUTS == ("gradient", "aspect", "profile", "plan", "tangential", "mean", "laplacian",
                               "hillshade")


DEM = np.zeros((6, 7), np.float32)


@pytest.mark.parametrize("call", [
    lambda: terrain.attributes(np.zeros(5, np.float32), 10.0),                       # not 2-D
    lambda: terrain.attributes(np.zeros((2, 3, 4), np.float32), 10.0),
    lambda: terrain.attributes(np.array([[0.1, 0.2]], np.float64), 10.0),            # float32 cannot hold it
    lambda: terrain.attributes(np.array([[2 ** 24 + 1]], np.int64), 10.0),
    lambda: terrain.attributes(DEM, 0.0),
    lambda: terrain.attributes(DEM, -1.0),
    lambda: terrain.attributes(DEM, float("nan")),
    lambda: terrain.attributes(DEM, float("inf")),
    lambda: terrain.attributes(DEM, True),
    lambda: terrain.attributes(DEM, "ten"),
    lambda: terrain.attributes(DEM, 10.0, radius=0),
    lambda: terrain.attributes(DEM, 10.0, radius=33),
    lambda: terrain.attributes(DEM, 10.0, radius=-1),
    lambda: terrain.attributes(DEM, 10.0, radius=2.0),
    lambda: terrain.attributes(DEM, 10.0, radius=True),
    lambda: terrain.attributes(DEM, 10.0, radius=None),
    lambda: terrain.attributes(DEM, 10.0, outputs=()),
    lambda: terrain.attributes(DEM, 10.0, outputs=[]),
    lambda: terrain.attributes(DEM, 10.0, outputs="gradient"),
    lambda: terrain.attributes(DEM, 10.0, outputs=None),
    lambda: terrain.attributes(DEM, 10.0, outputs=("gradient", "slope")),
    lambda: terrain.attributes(DEM, 10.0, outputs=("gradient", 3)),
    lambda: terrain.attributes(DEM, 10.0, outputs=("aspect", "gradient", "aspect")),
    lambda: terrain.attributes(DEM, 10.0, azimuth=float("nan")),
    lambda: terrain.attributes(DEM, 10.0, azimuth=float("inf")),
    lambda: terrain.attributes(DEM, 10.0, azimuth="north"),
    lambda: terrain.attributes(DEM, 10.0, altitude=0.0),
    lambda: terrain.attributes(DEM, 10.0, altitude=-5.0),
    lambda: terrain.attributes(DEM, 10.0, altitude=90.5),
    lambda: terrain.attributes(DEM, 10.0, altitude=float("nan")),
    lambda: terrain.gradient(DEM, 10.0, radius=40),
    lambda: terrain.aspect(DEM, 0.0),
    lambda: terrain.curvature(DEM, 10.0, kind="gaussian"),
    lambda: terrain.curvature(DEM, 10.0, kind="gradient"),
    lambda: terrain.curvature(DEM, 10.0, kind=None),
    lambda: terrain.curvature(DEM, 10.0, "profile", 0),
    lambda: terrain.hillshade(DEM, 10.0, altitude=0.0),
    lambda: terrain.hillshade(DEM, 10.0, azimuth=float("-inf")),
    lambda: terrain.hillshade(DEM, 10.0, 315.0, 45.0, 33),
])
def test_bad_arguments_raise_value_error(call):
    with pytest.raises(ValueError):
        call()


def test_too_many_cells_is_refused():
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 16, 2 ** 15), (0, 0))
    with pytest.raises(ValueError, match="2\\^31"):
        terrain.attributes(big, 10.0)
