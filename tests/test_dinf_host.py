"""CPU (not gpu): descriptools_amd.dinf refuses bad arguments with ValueError before any library call, and the numpy
reference the GPU tests compare against (tests/_dinf_ref.py) has the properties the definition promises: on D8 angles
it is the oracle's flow accumulation exactly, it conserves mass, every cell of a tilted plane completes, and the eight
float32 multiples of pi / 4 decode to one receiver each."""
import numpy as np
import pytest

import oracle
from descriptools_amd import dinf

import _dinf_ref as R


# ---- argument checks ----------------------------------------------------------------------------------------------
def _ang(shape=(5, 6)):
    return np.full(shape, -1, np.float32)


def test_value_errors_before_any_library_call():
    dem = np.arange(30, dtype=np.float32).reshape(5, 6)
    with pytest.raises(ValueError, match="2-D"):
        dinf.flow_direction(dem.reshape(-1), 10.0)
    with pytest.raises(ValueError, match="2-D"):
        dinf.accumulate(_ang().reshape(-1))
    with pytest.raises(ValueError, match="2-D"):
        dinf.specific_catchment_area(_ang().reshape(5, 6, 1), 10.0)
    with pytest.raises(ValueError, match="shape"):
        dinf.flow_direction(dem, 10.0, fdr=np.ones((5, 7), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        dinf.accumulate(_ang(), weights=np.ones((6, 5)))
    for px in (0.0, -1.0, float("nan"), float("inf"), "wide", True, "a"):
        with pytest.raises(ValueError, match="px"):
            dinf.flow_direction(dem, px)
        with pytest.raises(ValueError, match="px"):
            dinf.specific_catchment_area(_ang(), px)
    with pytest.raises(ValueError, match="float32"):
        dinf.flow_direction(dem.astype(np.float64) + 1e-9, 10.0)


@pytest.mark.parametrize("bad", [np.nan, -2.0, -0.5, -99.0, 6.2831860, np.inf, -np.inf])
def test_bad_angles(bad):
    a = _ang()
    a[2, 3] = bad
    with pytest.raises(ValueError, match="angle"):
        dinf.accumulate(a)
    with pytest.raises(ValueError):
        R.decode(a)


def test_bad_weights_and_frac_bits():
    a = _ang()
    for w in (np.full(a.shape, -1.0), np.full(a.shape, np.nan), np.full(a.shape, np.inf),
              np.full(a.shape, "x", dtype=object)):
        with pytest.raises(ValueError, match="weights"):
            dinf.accumulate(a, weights=w)
    for fb in (1.5, True, "3", 5000):
        with pytest.raises(ValueError, match="frac_bits"):
            dinf.accumulate(a, frac_bits=fb)
    with pytest.raises(ValueError, match="too fine"):
        dinf.accumulate(a, frac_bits=50)  # 30 cells * 2^50 > 2^52
    with pytest.raises(ValueError, match="too fine"):
        dinf.accumulate(a, weights=np.full(a.shape, 1000.0), frac_bits=45)


def test_2_31_cells_refused():
    big = np.broadcast_to(np.float32(-1), (1 << 16, 1 << 15))  # 2^31 cells, 4 bytes of memory
    with pytest.raises(ValueError, match="2\\^31"):
        dinf.accumulate(big)
    with pytest.raises(ValueError, match="2\\^31"):
        dinf.flow_direction(big, 10.0)


def test_alias_module():
    import descriptools.dinf
    assert descriptools.dinf.flow_direction is dinf.flow_direction
    assert descriptools.dinf.accumulate is dinf.accumulate
    assert descriptools.dinf.specific_catchment_area is dinf.specific_catchment_area


# ---- the reference's own properties --------------------------------------------------------------------------------
def test_eight_float32_multiples_snap():
    a = np.array([[np.float32(k * np.pi / 4) for k in range(9)]], np.float32)
    assert a[0, 8] == R.F2PI
    kind, k, p2 = R.decode(a)
    assert (kind == 1).all() and (p2 == 0).all()
    assert k[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    c = a[:, 1:8] + np.float32(1e-5)
    kind, kk, p2 = R.decode(c)
    assert (kind == 2).all() and (p2 > 0).all() and kk[0].tolist() == [1, 2, 3, 4, 5, 6, 7]


def test_share_is_exact():
    rng = np.random.default_rng(3)
    T = rng.integers(0, 1 << 52, 2000, dtype=np.int64)
    p2 = rng.integers(0, (1 << 30) + 1, 2000, dtype=np.int64)
    want = np.array([(int(t) * int(p)) >> 30 for t, p in zip(T, p2)], np.int64)
    np.testing.assert_array_equal(R.share(T, p2), want)


def test_d8_equivalence_with_oracle_flowacc():
    dem = oracle.synth_dem(2, 70, 67)
    _, fdr = oracle.slope_d8(dem, 10.0)
    ref = oracle.flowacc(fdr)
    a = R.d8_angles(fdr)
    got = R.accumulate(a, frac_bits=0)
    cyc = ref == -100
    np.testing.assert_array_equal(got[~cyc], ref[~cyc].astype(np.float64))
    assert (got[cyc] == -100).all()


@pytest.mark.parametrize("case", ["terrain", "terrain_nodata", "plane", "weights"])
def test_mass_conservation(case):
    rng = np.random.default_rng(5)
    w = None
    if case == "plane":
        yy, xx = np.mgrid[0:40, 0:50]
        dem = (1000 - 3 * yy - xx).astype(np.float32)
    else:
        dem = oracle.synth_dem(7, 90, 120, nodata_pct=2 if case == "terrain_nodata" else 0)
        if case == "weights":
            w = rng.uniform(0, 10, dem.shape)
    fdr, filled = oracle.condition_d8(dem, 10.0)
    a, _ = R.flow_direction(filled, 10.0, fdr)
    res, x = R.accumulate(a, w, full=True)
    assert (x["done"] | x["nodata"]).all(), "a conditioned surface has no cycle"
    sink = x["done"] & (x["r0"] < 0) & (x["r1"] < 0)
    live = ~x["nodata"]
    assert int(x["q"][live].sum()) == int(x["T"][sink].sum()) + x["left"]
    assert (res[x["nodata"].reshape(res.shape)] == -100).all() and (res[live.reshape(res.shape)] >= 0).all()


def test_plane_every_cell_completes_with_two_donors_and_receivers():
    yy, xx = np.mgrid[0:40, 0:50]
    dem = (1000 - 3 * yy - xx).astype(np.float32)
    a, s = R.flow_direction(dem, 1.0)
    # interior: facet 7 (S, SE), r = atan2(1, 3), s = sqrt(10)
    assert (s[1:-1, 1:-1] == np.float32(np.sqrt(10.0))).all()
    want = np.float32(3 * np.pi / 2 + np.arctan2(1.0, 3.0))
    assert (np.abs(a[1:-1, 1:-1] - want) <= np.spacing(want)).all()
    res, x = R.accumulate(a, full=True)
    assert x["done"].all()
    r0, r1 = x["r0"].reshape(40, 50), x["r1"].reshape(40, 50)
    assert (r0[1:-1, 1:-1] >= 0).all() and (r1[1:-1, 1:-1] >= 0).all()
    pend = np.bincount(x["r0"][x["r0"] >= 0], minlength=2000) + np.bincount(x["r1"][x["r1"] >= 0], minlength=2000)
    assert (pend.reshape(40, 50)[2:-1, 1:-1] == 2).all()


def test_direction_rules_on_small_cases():
    # a pit, a flat and nodata / non-finite centres
    dem = np.full((5, 5), 10, np.float32)
    dem[2, 2] = 5          # pit
    dem[0, 0] = -100       # nodata
    dem[4, 4] = np.nan
    dem[0, 4] = np.inf
    a, s = R.flow_direction(dem, 2.0)
    assert a[2, 2] == -1 and s[2, 2] == 0
    assert a[0, 0] == -100 and s[0, 0] == -100
    assert a[4, 4] == -1 and s[4, 4] == 0 and a[0, 4] == -1 and s[0, 4] == 0
    assert a[1, 2] == np.float32(3 * np.pi / 2) and s[1, 2] == np.float32(2.5)  # straight south into the pit
    assert a[1, 1] == np.float32(7 * np.pi / 4)                                  # diagonal into the pit
    assert s[1, 1] == np.float32(5 / (2.0 * np.sqrt(2.0)))
    fdr = np.zeros((5, 5), np.uint8)
    fdr[2, 2] = 1      # pit -> E (valid)
    fdr[3, 4] = 2      # flat cell -> SE, which is NaN: no fallback
    fdr[0, 1] = 16     # -> W, which is nodata: no fallback
    fdr[4, 0] = 4      # -> S, off the raster
    fdr[3, 0] = 64     # flat -> N
    a2, s2 = R.flow_direction(dem, 2.0, fdr)
    assert a2[2, 2] == np.float32(0) and s2[2, 2] == 0
    assert a2[3, 4] == -1 and a2[0, 1] == -1 and a2[4, 0] == -1
    assert a2[3, 0] == np.float32(np.pi / 2)
    won = s > 0
    np.testing.assert_array_equal(a2[won], a[won])
