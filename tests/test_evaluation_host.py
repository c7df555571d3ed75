"""CPU: the numpy reference of the evaluation layer (tests/_evaluation_ref.py) is pinned against the reference
implementation's recorded results (tests/golden/eval.npz, eval_edge.npz), and the host-only parts of
descriptools_amd.evaluation -- the grid search, the combination of per-rank extremes, the dtype table -- against it.
Everything here is exact: integer counts, IEEE comparisons, one or two correctly rounded operations."""
import operator
import warnings

import numpy as np
import pytest

from conftest import golden
from descriptools_amd import evaluation

import _evaluation_ref as R


def _cases():
    g = golden("eval")
    for k in range(3):
        yield "eval.e%d" % k, {n: g["e%d_%s" % (k, n)] for n in ("flood", "under", "mn", "mx", "desc", "th", "binary",
                                                                 "c", "f", "class", "flood_after")} | {"raw": g["e%d_hand" % k]}
    g = golden("eval_edge")
    for name in g["names"]:
        yield "edge." + str(name), {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(str(name) + "_")}


CASES = dict(_cases())


def test_edge_golden_holds_the_cases_it_is_for():
    e = {k[5:]: v for k, v in CASES.items() if k.startswith("edge.")}
    assert {c["raw"].dtype for c in e.values()} >= {np.dtype(t) for t in (np.float16, np.float32, np.float64, np.int16)}
    assert e["f16"]["desc"].dtype == np.float16 and e["f32"]["desc"].dtype == np.float32
    assert {int(c["coarse"]) for c in e.values() if "coarse" in c} == {25, 50, 75}
    assert str(e["over"]["under"]) == "over" and (e["over"]["raw"] < 0).sum() > 100
    river = e["river"]
    assert river["desc"][0, 0] == 0.0 and (river["desc"] == 0.0).sum() > 1000 and river["binary"][river["desc"] == 0.0].sum() == 0
    assert (e["quant"]["desc"] == float(e["quant"]["th"])).sum() > 10
    assert float(e["tie"]["th"]) >= 0.6 and int(e["tie"]["coarse"]) == 50
    assert str(e["drynan"]["error"]) == "UnboundLocalError" and "error" not in e["dry"]
    assert (e["dry"]["flood"] == 1).sum() == 0 and np.isnan(e["dry"]["c"]) and float(e["dry"]["f"]) == 0.0
    for c in e.values():
        assert c["raw"].shape[0] <= 64 and c["raw"].shape[1] <= 96


@pytest.mark.parametrize("name", list(CASES))
def test_reference_reproduces_golden(name):
    c = CASES[name]
    under, flood = str(c["under"]), c["flood"]
    desc = R.scale(c["raw"], c["mn"][()], c["mx"][()], -100)
    assert R.same(desc, c["desc"])
    if "error" in c:
        with pytest.raises(UnboundLocalError) as err:
            R.calibrate(desc, flood, under)
        assert type(err.value).__name__ == str(c["error"])
        return
    th = R.calibrate(desc, flood, under)
    assert th == float(c["th"])
    binary = R.binary_map(desc, th, under)
    assert binary.dtype == np.int64 and np.array_equal(binary, c["binary"])
    klass, counts = R.class_map(binary, flood)
    assert np.array_equal(klass, c["class"]) and np.array_equal(R.remap(flood), c["flood_after"])
    assert np.array_equal(counts, np.bincount(c["class"].reshape(-1).astype(np.int64), minlength=4))
    if "counts" in c:
        assert np.array_equal(counts, c["counts"])
    cor, fit = R.indexes(counts)
    assert np.array_equal([cor, fit], [float(c["c"]), float(c["f"])], equal_nan=True)


# ---- the grid search on fit functions given as tables ------------------------------------------------------------
KEY0, NKEY = -200, 10600   # thresholds the search can ask for, in 1/10000: -0.011 .. 1.011


def _table(family, seed):
    rng = np.random.default_rng(1000 * family + seed)
    k = np.arange(NKEY) + KEY0
    q = [4, 8, 16, 1000][seed % 4]   # coarse quantisation: many equal fits
    if family == 0:      # monotone, rising or falling
        f = k / 10000.0 if seed % 2 else 1.0 - k / 10000.0
    elif family == 1:    # one peak anywhere, also outside the coarse candidates' reach
        f = 1.0 / (1.0 + ((k - rng.integers(-100, 10100)) / rng.integers(50, 4000)) ** 2)
    elif family == 2:    # plateau: equal fits over a range, lower outside
        a = rng.integers(0, 9000)
        f = np.where((k >= a) & (k <= a + rng.integers(100, 4000)), 0.75, 0.25 + 0.1 * np.sin(k / 700.0))
    elif family == 3:    # NaN everywhere
        return np.full(NKEY, np.nan)
    else:                # a peak with NaN stretches
        f = 1.0 / (1.0 + ((k - rng.integers(0, 10000)) / rng.integers(300, 4000)) ** 2)
        for _ in range(rng.integers(1, 6)):
            a = rng.integers(KEY0, KEY0 + NKEY)
            f[max(a - KEY0, 0):a - KEY0 + rng.integers(30, 3000)] = np.nan
        return np.floor(f * q) / q
    return np.floor(f * q) / q


def _lookup(table, asked):
    def at(th):
        key = int(round(th * 10000))
        assert abs(key / 10000 - th) < 1e-12
        asked.append(key)
        return float(table[key - KEY0])
    return at


def _outcome(fn):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn()
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return type(e)


def test_grid_search_equals_reference_search_on_tables():
    strict_first = ((100, 20, 10, operator.gt),) + R.STAGES[1:]
    seen, tie_decided, raised = set(), 0, 0
    for family in range(5):
        for seed in range(40):
            table = _table(family, seed)
            a_ref, a_got = [], []
            at = _lookup(table, a_got)
            want = _outcome(lambda: R.search(_lookup(table, a_ref)))
            got = _outcome(lambda: evaluation._grid_search(lambda ths: [at(t) for t in ths]))
            assert got == want, (family, seed, got, want)
            assert a_got == a_ref, "same thresholds asked for, in the same order"
            if isinstance(want, type):
                assert want is UnboundLocalError
                raised += 1
                continue
            seen.add(a_ref[3] // 100 + 20)   # centre of the first stage
            tie_decided += _outcome(lambda: R.search(_lookup(table, []), strict_first)) != want
    assert seen == {25, 50, 75} and raised >= 40 and tie_decided >= 5, (seen, raised, tie_decided)


# ---- per-rank extremes combined ------------------------------------------------------------------------------
def _split(x, cuts):
    return np.split(np.asarray(x, np.float32), cuts)


RANKS = {
    "one rank": _split([3, 1, 2, np.nan, 1], []),
    "all-equal ranks": _split([5, 5, 5, 5, 7, 7], [2, 4]),
    "every rank the same constant": _split([5, 5, 5, 5], [2]),
    "all-NaN rank among others": _split([np.nan, np.nan, 4, -2, 9], [2]),
    "only all-NaN ranks": _split([np.nan] * 5, [2]),
    "minimum on several ranks, more than once": _split([-100, 3, -100, -100, 0, 7, -100, 2], [2, 5]),
    "second is another rank's minimum": _split([-100, 50, 60, 1, 2, 3], [3]),
    "infinite second and largest": _split([1, np.inf, 1, 1], [2]),
    "-inf minimum": _split([-np.inf, 0, 5, -np.inf], [2]),
    "both zeros": _split([-0.0, 3, 0.0, 2], [2]),
    "empty rank": _split([4, 2, 8], [0, 2]),
}


@pytest.mark.parametrize("name", list(RANKS))
def test_combine_extremes_equals_extremes_of_the_whole(name):
    ranks = RANKS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # an all-NaN rank is ordinary input: no RuntimeWarning
        got = evaluation.combine_extremes([R.extremes(r) for r in ranks])
    assert R.same(got, R.extremes(np.concatenate(ranks))), (got, R.extremes(np.concatenate(ranks)))


def test_combine_extremes_random_splits():
    rng = np.random.default_rng(5)
    for _ in range(200):
        x = rng.integers(-3, 4, size=rng.integers(1, 12)).astype(np.float32)
        x[rng.random(x.size) < 0.3] = np.nan
        ranks = np.split(x, np.sort(rng.integers(0, x.size + 1, size=rng.integers(0, 4))))
        assert R.same(evaluation.combine_extremes([R.extremes(r) for r in ranks]), R.extremes(x)), ranks


# ---- the dtype table ------------------------------------------------------------------------------------------
DTYPES = [np.float16, np.float32, np.float64, np.int16, np.int32, np.uint8, np.bool_]
SCALARS = {"python float": (0.5, 7.25), "python int": (0, 7), "np.float32": (np.float32(0.5), np.float32(7.25)),
           "np.float64": (np.float64(0.5), np.float64(7.25)), "np.int16": (np.int16(0), np.int16(7))}


@pytest.mark.parametrize("kind", list(SCALARS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_float_view_follows_numpy(dtype, kind):
    a = np.array([[1, 0, 1], [0, 1, 1]], dtype)
    mn, mx = SCALARS[kind]
    want = R.scale(a, mn, mx, -100 if np.dtype(dtype).kind in "fi" else 0).dtype
    x, rt = evaluation._float_view(a, mn, mx)
    assert rt == want and x.dtype == want and x.flags.c_contiguous and np.array_equal(x, a.astype(want))
    # binary_map's comparison: the first-cell rule writes NaN into the raster, the threshold joins by its own rule
    holed = np.where(a == a[0, 0], np.nan, a)
    assert evaluation._float_view(a, mx)[1] == np.result_type(holed, mx)
