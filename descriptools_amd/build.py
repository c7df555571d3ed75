"""Build libdescriptools_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libdescriptools_hip.so")
SOURCES = ["dt_kernels.hip", "dt_stencil.hip", "dt_tiles.hip", "dt_hydro.hip", "dt_wide.hip", "dt_streams.hip",
           "dt_watershed.hip", "dt_reaches.hip", "dt_countdown.hip", "dt_dinf.hip", "dt_dinf_dist.hip", "dt_mfd.hip",
           "dt_terrain.hip", "dt_horizon.hip", "dt_proximity.hip", "dt_regions.hip", "dt_curve.hip",
           "dt_focal.hip", "dt_mrvbf.hip", "dt_zonal.hip", "dt_cost.hip", "dt_wetness.hip", "dt_morphology.hip",
           "dt_flowpath.hip", "dt_harmonic.hip", "dt_inundation.hip", "dt_filters.hip", "dt_resample.hip",
           "dt_vector.hip", "dt_polygonize.hip", "dt_capi.hip"]
HEADERS = ["dt_common.h", "dt_kernels.h", "dt_countdown.h", "dt_dinf_common.h", "dt_tile_rounds.h", "dt_path_tiles.h",
           "dt_math.h", "dt_math_coeffs.h", "dt_reach_wet.h", "dt_d8_kernel.inc", "dt_fa3fh1_kernel.inc",
           os.path.join("..", "..", "include", "descriptools_hip.h")]
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-function"]


def _stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not _stale():
        return SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        cmd = [hipcc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
