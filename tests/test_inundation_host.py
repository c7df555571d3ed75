"""CPU (not gpu): flood inundation without a device -- the numpy reference of tests/_inundation_ref.py against what the
scheme must hold (cbrt3 against np.cbrt, a lake at rest, conservation and non-negativity, the open boundary's decay,
Hunter's analytic wave, resuming); every ValueError of descriptools_amd.inundation, raised before the library is
loaded; the new entries in the header, the binding table and the build (what the C entries refuse is in
tests/test_gpu_inundation.py, where a device lets them run); the alias module."""
import math
import os

import numpy as np
import pytest

import _inundation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the RMSE of the reference against Hunter's analytic profile at px = 25 (cell centres), as DESIGN.md 4.25 records it
HUNTER_RMSE = 0.03563


def _volume(depth, px):
    return math.fsum((depth * (px * px)).reshape(-1).tolist())


# ---- the reference ----------------------------------------------------------------------------------------------------
def test_cbrt3_is_within_2_ulp():
    x = np.exp(np.random.default_rng(0).uniform(math.log(1e-6), math.log(1e4), 100000))
    got, ref = R.cbrt3(x), np.cbrt(x)
    ulp = np.abs(got - ref) / np.spacing(ref)
    print("largest distance to np.cbrt: %.2f ulp" % ulp.max())
    assert ulp.max() <= 2.0
    # exact where the root is a float64: the scaling is exact and Newton's fixed point is the root
    cubes = np.array([1.0, 8.0, 27.0, 0.125, 1e-6 ** 3, 4096.0, 2.0 ** -300, 2.0 ** 300])
    assert (np.abs(R.cbrt3(cubes) - np.cbrt(cubes)) <= np.spacing(np.cbrt(cubes))).all()
    assert R.cbrt3(np.float64(5e-324)) > 0  # the smallest subnormal has an exponent to split, too


@pytest.mark.parametrize("level,islands", [(5.0, False), (2.0, True)])
def test_lake_at_rest(level, islands):
    dem, valid, depth = R.lake(level, islands)
    assert ((depth[valid] == 0).sum() > 100) == islands
    r = R.simulate(dem, valid, 10.0, 600.0, depth=depth)
    assert r["finished"] and r["t"] == 600.0 and r["steps"] > 100
    assert np.array_equal(r["depth"].view(np.int64), depth.view(np.int64))
    assert not r["qx"].any() and not r["qy"].any()


def _rain_and_inflow():
    dem, valid = R.rough_terrain()
    cell = 35 * dem.shape[1] + 3
    rain = 50e-3 / 3600.0
    r = R.simulate(dem, valid, 10.0, 1800.0, rain=rain, inflow=(np.array([cell]), np.array([0.0]), np.array([[20.0]])))
    return r, (rain * valid.sum() * 100.0 + 20.0) * 1800.0


def test_conservation_and_non_negativity_rain_and_inflow():
    r, v_in = _rain_and_inflow()
    v = _volume(r["depth"], 10.0)
    print("steps %d, volume %.6f of %.6f, limited steps %d" % (r["steps"], v, v_in, r["limited_steps"]))
    assert r["finished"] and r["limited_steps"] > 0
    assert not np.isnan(r["depth"]).any() and r["depth"].min() >= 0
    assert abs(v - v_in) <= 1e-9 * v_in
    assert np.array_equal(np.isnan(r["arrival"]), ~(r["max_depth"] > 0.05))


def test_conservation_and_non_negativity_dam_break():
    dem, valid, depth = R.dam_break()
    r = R.simulate(dem, valid, 10.0, 900.0, manning=0.01, depth=depth)
    v, v_in = _volume(r["depth"], 10.0), _volume(depth, 10.0)
    print("steps %d, volume %.6f of %.6f, limited steps %d" % (r["steps"], v, v_in, r["limited_steps"]))
    assert not np.isnan(r["depth"]).any() and r["depth"].min() >= 0
    assert abs(v - v_in) <= 1e-9 * v_in
    assert r["depth"][:, -1].max() > 0.1, "the wave reached the foot of the slope"


def test_open_boundary_decay():
    dem, valid, depth = R.dam_break()
    r = R.simulate(dem, valid, 10.0, 3600.0, manning=0.01, depth=depth, boundary="open", track=True)
    v = np.array([_volume(depth, 10.0)] + r["volumes"])
    print("%.3f %% of the volume is left" % (100 * v[-1] / v[0]))
    assert (np.diff(v) <= 0).all()
    assert v[-1] < 0.05 * v[0]
    assert r["depth"].min() >= 0


def test_hunter_wave():
    inflow, ana = R.hunter()
    r = R.simulate(np.zeros((1, 200)), np.ones((1, 200), bool), 25.0, 3600.0, manning=0.03, inflow=inflow)
    h = r["depth"][0]
    rmse = float(np.sqrt(np.mean((h - ana) ** 2)))
    front = (int(np.nonzero(h > 0.01)[0][-1]) + 1) * 25.0
    print("RMSE %.5f m (recorded %.5f), upstream depth %.3f m, front at %.0f m" % (rmse, HUNTER_RMSE, ana[0], front))
    assert rmse <= 1.5 * HUNTER_RMSE
    assert rmse <= 0.05 * 2.38
    assert abs(front - 3600.0) <= 360.0


def test_resume_equals_the_uncut_run():
    dem, valid = R.rough_terrain()
    kw = dict(rain=20e-3 / 3600.0, inflow=(np.array([40 * 131 + 5]), np.array([0.0, 300.0]), np.array([[0.0, 30.0]])),
              boundary="open")
    whole = R.simulate(dem, valid, 10.0, 400.0, **kw)
    part = R.simulate(dem, valid, 10.0, 400.0, max_steps=37, **kw)
    assert part["steps"] == 37 and not part["finished"]
    rest = R.simulate(dem, valid, 10.0, 400.0, state=part, **kw)
    assert rest["steps"] == whole["steps"] and rest["t"] == whole["t"] == 400.0
    for name in ("depth", "qx", "qy", "max_depth", "arrival"):
        assert np.array_equal(rest[name].view(np.int64), whole[name].view(np.int64)), name


# ---- the argument checks: before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from descriptools_amd import _lib

    def refuse():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_value_errors(no_library):
    from descriptools_amd import inundation
    z = np.zeros((4, 5), np.float32)
    sim = inundation.simulate
    good = (np.array([3]), np.array([0.0, 10.0]), np.array([[1.0, 2.0]]))
    state = {"depth": np.zeros((4, 5)), "qx": np.zeros((4, 5)), "qy": np.zeros((4, 5)), "t": 0.0, "steps": 0}
    nod = z.copy()
    nod[0, 3] = -100
    for call in (lambda: sim(np.zeros(5), 10.0, 60.0),
                 lambda: sim(np.zeros((2, 2, 2)), 10.0, 60.0),
                 lambda: sim(z.astype(complex), 10.0, 60.0),
                 lambda: sim(z, 10.0, 60.0, manning=np.full((5, 4), 0.05)),
                 lambda: sim(z, 10.0, 60.0, rain=np.zeros((4, 4))),
                 lambda: sim(z, 10.0, 60.0, depth=np.zeros((3, 5))),
                 lambda: sim(z, 10.0, 60.0, depth=np.full((4, 5), -1.0)),
                 lambda: sim(z, 10.0, 60.0, depth=np.full((4, 5), np.nan)),
                 lambda: sim(z, 10.0, 60.0, manning=0.0),
                 lambda: sim(z, 10.0, 60.0, manning=float("nan")),
                 lambda: sim(z, 10.0, 60.0, manning=np.zeros((4, 5))),
                 lambda: sim(z, 10.0, 60.0, rain=-1e-6),
                 lambda: sim(z, 10.0, 60.0, rain=np.full((4, 5), np.inf)),
                 lambda: sim(z, 10.0, 60.0, alpha=1.5),
                 lambda: sim(z, 10.0, 60.0, dry=-1e-3),
                 lambda: sim(z, 10.0, 60.0, dry=float("nan")),
                 lambda: sim(z, 10.0, 60.0, arrival_depth=-1.0),
                 lambda: sim(z, 10.0, 60.0, boundary="periodic"),
                 lambda: sim(z, 10.0, 60.0, boundary=1),
                 lambda: sim(z, 10.0, 60.0, outputs=("depth", "speed")),
                 lambda: sim(z, 10.0, 60.0, outputs=()),
                 lambda: sim(z, 10.0, 60.0, outputs=("depth", "depth")),
                 lambda: sim(z, 10.0, 60.0, max_steps=-1),
                 lambda: sim(z, 10.0, 60.0, max_steps=2.5),
                 lambda: sim(z, 10.0, 60.0, sync_every=0),
                 lambda: sim(z, 10.0, 60.0, sync_every=1025),
                 lambda: sim(z, 10.0, 60.0, sync_every=True),
                 lambda: sim(z, 10.0, 60.0, state=dict(state, depth=np.zeros((5, 4)))),
                 lambda: sim(z, 10.0, 60.0, state=dict(state, qx=np.zeros((4, 6)))),
                 lambda: sim(z, 10.0, 60.0, state={"depth": np.zeros((4, 5))}),
                 lambda: sim(z, 10.0, 60.0, state=7),
                 lambda: sim(z, 10.0, 60.0, inflow=(np.array([3]), np.array([0.0, 10.0]))),
                 lambda: sim(z, 10.0, 60.0, inflow=(np.array([3.0]), good[1], good[2])),
                 lambda: sim(z, 10.0, 60.0, inflow=(np.array([20]), good[1], good[2])),
                 lambda: sim(z, 10.0, 60.0, inflow=(np.array([-1]), good[1], good[2])),
                 lambda: sim(z, 10.0, 60.0, inflow=(np.array([3, 3]), good[1], np.ones((2, 2)))),
                 lambda: sim(z, 10.0, 60.0, inflow=(good[0], np.array([0.0, 0.0]), good[2])),
                 lambda: sim(z, 10.0, 60.0, inflow=(good[0], np.array([10.0, 0.0]), good[2])),
                 lambda: sim(z, 10.0, 60.0, inflow=(good[0], good[1], np.array([[1.0, np.nan]]))),
                 lambda: sim(z, 10.0, 60.0, inflow=(good[0], good[1], np.array([[1.0, -2.0]]))),
                 lambda: sim(z, 10.0, 60.0, inflow=(good[0], good[1], np.ones((1, 3)))),
                 lambda: sim(z, 10.0, 60.0, inflow=(good[0], np.zeros(0), np.ones((1, 0)))),
                 lambda: sim(nod, 10.0, 60.0, inflow=good),
                 lambda: sim(z, 10.0, 60.0, inflow=(np.arange(4097), np.array([0.0]), np.ones((4097, 1))))):
        with pytest.raises(ValueError):
            call()
    for bad in (0, -1.0, float("nan"), float("inf"), None, "x", True):
        for name in ("px", "t_end", "alpha", "dt_max", "boundary_slope"):
            kw = {"px": 10.0, "t_end": 60.0}
            kw[name] = bad
            with pytest.raises(ValueError, match=name):
                sim(z, kw.pop("px"), kw.pop("t_end"), **kw)
    big = np.broadcast_to(np.float32(1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
    with pytest.raises(ValueError, match="2\\^31"):
        sim(big, 10.0, 60.0)


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_built():
    from descriptools_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    for name in ("dt_inundation", "dt_dev_inundation"):
        assert "int %s(" % name in header
        assert name in _lib._SIGS
    assert "dt_inundation.hip" in build.SOURCES
    kernels = open(os.path.join(ROOT, "descriptools_amd", "csrc", "dt_kernels.h")).read()
    assert "dt_launch_inundation_steps(" in kernels


def test_alias_module():
    import descriptools.inundation as alias
    from descriptools_amd import inundation
    for name in ("simulate", "Inundation"):
        assert getattr(alias, name) is getattr(inundation, name)
        assert name in alias.__all__
