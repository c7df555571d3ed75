"""CPU: bench.py's CPU baseline on a checkout it cannot write (built earlier by another user): the oracle's timed
build is made in a temporary directory instead of oracle/_build, and the baseline runs."""
import importlib
import os

bench = importlib.import_module("bench")


def test_baseline_library_outside_a_read_only_tree(monkeypatch, tmp_path):
    import oracle
    so = str(tmp_path / "ro" / "_build" / "libdt_oracle_bench.so")  # missing, in a directory we may not write
    monkeypatch.setattr(oracle, "_SO_BENCH", so)
    monkeypatch.setattr(bench.os, "access", lambda p, mode: False)
    tmp = bench.baseline_library(oracle)
    try:
        assert tmp is not None and os.path.isdir(tmp)
        assert oracle._SO_BENCH == os.path.join(tmp, "_build", "libdt_oracle_bench.so")
        assert os.path.exists(oracle._SO_BENCH) and not os.path.exists(so)
        oracle.use_bench_build(1)
        dem = oracle.synth_dem(1, 64, 64)
        sl, fdr = oracle.slope_d8(dem, 10.0)
        assert sl.shape == (64, 64)
    finally:
        oracle.use_bench_build(None)
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


def test_cpu_baseline_restores_the_oracle_and_cleans_up(monkeypatch, tmp_path):
    import oracle
    so = str(tmp_path / "ro" / "_build" / "libdt_oracle_bench.so")
    monkeypatch.setattr(oracle, "_SO_BENCH", so)
    monkeypatch.setattr(bench.os, "access", lambda p, mode: False)
    r = bench.cpu_baseline(128)
    assert r["value"] > 0 and r["all_cores"]["value"] > 0
    assert oracle._SO_BENCH == so and not os.path.exists(so)
