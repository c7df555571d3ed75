"""CPU (not gpu): the numpy reference of the threshold curves (tests/_curve_ref.py) pinned against _evaluation_ref
threshold by threshold, its integer AUC against a brute-force pair count, the input on which the four-stage search misses
the best threshold of its own lattice, and every ValueError the Python layer raises before it touches the library."""
import numpy as np
import pytest

import _curve_ref as CR
import _evaluation_ref as R

SIDES = ("under", "over")


def _descriptor(dtype, first, n=600, seed=0):
    """values k / 64 in 0..1 with cells on thresholds, +-0.0, +-inf, NaN and many cells equal to the first"""
    rng = np.random.default_rng(seed)
    d = (np.floor(rng.random(n) * 65) / 64).astype(np.float64)
    d[5:9] = (0.0, -0.0, np.inf, -np.inf)
    d[9:12] = np.nan
    d[0] = {"nan": np.nan, "valid": 0.25, "outside": -1.0}[first]
    d[12:20] = d[0]
    if np.dtype(dtype).kind != "f":
        d = np.where(np.isfinite(d), np.floor(np.nan_to_num(d, posinf=0, neginf=0) * 64), -100)
    return d.astype(dtype)


def _bench(n, seed, extra=False):
    rng = np.random.default_rng(seed + 100)
    b = rng.choice(np.array([0, 1, -100], np.int8), n)
    if extra:
        b[::7] = 3
    return b


THRESHOLDS = np.array([-np.inf, -1.0, -0.0, 0.0, 0.0, 0.1, 0.25, 0.25, 0.3, 0.5, 33 / 64, 0.75, 1.0, 1.5, np.inf])


@pytest.mark.parametrize("under", SIDES)
@pytest.mark.parametrize("first", ["nan", "valid", "outside"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64, np.int16])
def test_reference_counts_equal_binary_map_and_class_map(dtype, first, under):
    d, b = _descriptor(dtype, first), _bench(600, 1)
    th = THRESHOLDS * (64 if np.dtype(dtype).kind != "f" else 1)
    live = R._live(d)
    assert np.isnan(live).sum() > 8 and (np.asarray(live, np.float64)[:, None] == CR.compared(d, th)[None, :]).any()
    h = CR.hist(d, b, th, under)
    assert h[-1] == 0 and h.sum() == d.size
    counts = CR.counts_of(h, len(th), under)
    for k, t in enumerate(th):
        assert np.array_equal(counts[k], R.class_map(R.binary_map(d, float(t), under), b)[1]), (k, t)


@pytest.mark.parametrize("under", SIDES)
def test_reference_reports_unknown_benchmark_values(under):
    d, b = _descriptor(np.float64, "nan"), _bench(600, 2, extra=True)
    h = CR.hist(d, b, THRESHOLDS, under)
    assert h[-1] == np.count_nonzero(b == 3) > 0 and h.sum() == d.size


@pytest.mark.parametrize("under", SIDES)
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_auc_equals_pair_count(seed, under):
    """with a threshold between every two distinct values, one below the smallest and one above the largest, no two
    values share a bin and the dead cells have one of their own, so the binned area is the exact Mann-Whitney statistic"""
    n = 1500
    rng = np.random.default_rng(seed)
    d = np.floor(rng.random(n) * 200) / 256
    d[3:40] = np.nan
    d[0] = d[50]
    b = np.where(rng.random(n) < 0.2 + 0.6 * np.nan_to_num(d if under == "over" else 1 - d), 1, 0).astype(np.int8)
    b[rng.random(n) < 0.1] = -100
    live = R._live(d)
    u = np.unique(live[~np.isnan(live)])
    th = np.concatenate([[u[0] - 1], (u[:-1] + u[1:]) / 2, [u[-1] + 1]])
    assert np.isnan(live).sum() > 37 and not np.isin(th, u).any()
    assert len(np.unique(CR.bins(d, th, under))) == len(u) + 1
    c = CR.curve(d, b, under, thresholds=th)
    assert c.auc == CR.auc_pairs(d, b, under)
    assert 0.5 < c.auc < 1.0


def _motivating(seed, mirrored):
    u = np.random.default_rng(seed).random(4096)
    d = np.floor(u * 4096) / 4096
    d[0] = -1
    b = (((d >= 0) & (d < 0.03)) | ((d > 0.8) & (d < 0.97))).astype(np.int8)
    return (1 - d, b, "over") if mirrored else (d, b, "under")


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("seed", range(5))
def test_four_stage_search_misses_the_best_lattice_threshold(seed, mirrored):
    d, b, under = _motivating(seed, mirrored)
    fit_at = R.fit_of(d, b, under)
    searched, best = R.calibrate(d, b, under), CR.exhaustive(d, b, under)
    assert abs(best - searched) > 0.25  # out of the search's reach
    assert fit_at(best) > fit_at(searched)
    assert fit_at(best) == np.nanmax(CR.curve(d, b, under).fit)


@pytest.mark.parametrize("objective", ["fit", "tss", "kappa"])
def test_reference_exhaustive_is_first_argmax(objective):
    d, b, under = _motivating(0, False)
    score = getattr(CR.curve(d, b, under, steps=100), objective)
    k = round(CR.exhaustive(d, b, under, steps=100, objective=objective) * 100)
    assert score[k] == np.nanmax(score) and not (score[:k] == score[k]).any()


def test_value_errors_before_the_library(monkeypatch):
    from descriptools_amd import _lib, evaluation

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    d, b = np.linspace(0, 1, 12).reshape(3, 4), np.zeros((3, 4), np.int8)
    bad = [([0.5, 0.25], "sorted"), ([0.1, np.nan, 0.3], "NaN"), ([np.nan], "NaN"), ([], "thresholds"),
           (np.zeros(65536), "thresholds")]
    for th, what in bad:
        with pytest.raises(ValueError, match=what):
            evaluation.threshold_counts(d, b, th, "under")
        with pytest.raises(ValueError, match=what):
            evaluation.curve(d, b, "over", thresholds=th)
        with pytest.raises(ValueError, match=what):
            evaluation.curve_resident(None, None, None, 12, th, "under", 0.0)
    # a float32 descriptor rounds the thresholds first: these two become equal, which is sorted
    with pytest.raises(AssertionError, match="touched"):
        evaluation.threshold_counts(d.astype(np.float32), b, [0.5 + 1e-12, 0.5], "under")
    with pytest.raises(ValueError, match="sorted"):
        evaluation.threshold_counts(d, b, [0.5 + 1e-12, 0.5], "under")
    for shape in ((4, 3), (12,), (3, 5)):
        with pytest.raises(ValueError, match="shape"):
            evaluation.threshold_counts(d, np.zeros(shape, np.int8), [0.5], "under")
        with pytest.raises(ValueError, match="shape"):
            evaluation.calibration_exhaustive(d, np.zeros(shape, np.int8), "under")
    for value in (2, 300):  # what the kernel could not tell from a flooded cell: a raw 2, a value that wraps in int8
        with pytest.raises(ValueError, match="other than -100, 0 and 1"):
            evaluation.threshold_counts(d, np.full((3, 4), value, np.int16), [0.5], "under")
    with pytest.raises(ValueError, match="objective"):
        evaluation.calibration_exhaustive(d, b, "under", objective="auc")
    with pytest.raises(ValueError, match="steps"):
        evaluation.calibration_exhaustive(d, b, "under", steps=0)
    with pytest.raises(ValueError, match="thresholds"):
        evaluation.calibration_exhaustive(d, b, "under", steps=65535)


def test_curve_names_reach_the_alias_package():
    import descriptools.evaluation as alias
    from descriptools_amd import evaluation
    for name in ("threshold_counts", "curve", "calibration_exhaustive", "curve_resident", "Curve"):
        assert getattr(alias, name) is getattr(evaluation, name)
