"""The byte size of every workspace, against a recorded table.

Each workspace in csrc/ has one layout function, and its size is what that function returns when it is given no
memory ("Workspaces").  These sizes are part of what a caller sees: dt_ctx_scratch_bytes after a device-tier
call, and the size-only exports a caller allocates by.  The tables below are recorded, not computed: `python
tests/test_gpu_scratch_layout.py` prints them from the library it finds, and they are its output on the commit named
above each table, the last one with hand-written size formulas.  A context's scratch only grows, so every reading opens
a context of its own."""
import ctypes as C

import numpy as np
import pytest

SHAPES = [(1, 1), (64, 64), (65, 63), (130, 257), (1000, 1001)]  # one cell; one tile; ragged both ways; ...

# recorded on 59e6e22 (size-only exports: no device needed); the slope_marks column on the child of 63a8c81, which
# sizes the marks for the one 256 x 16 tile geometry instead of the largest of three
EXPORTS = {
    (1, 1): {
        "downslope_lift_w": 2304, "slope_marks": 768, "downslope_lift": 1536, "downslope_queue": 512,
        "downslope_tables": 1024, "hand_f64_table": 1024,
    },
    (64, 64): {
        "downslope_lift_w": 153856, "slope_marks": 2304, "downslope_lift": 135424, "downslope_queue": 33024,
        "downslope_tables": 102400, "hand_f64_table": 131072,
    },
    (65, 63): {
        "downslope_lift_w": 153856, "slope_marks": 2816, "downslope_lift": 135424, "downslope_queue": 33024,
        "downslope_tables": 102400, "hand_f64_table": 131072,
    },
    (130, 257): {
        "downslope_lift_w": 1152768, "slope_marks": 9472, "downslope_lift": 1103872, "downslope_queue": 267776,
        "downslope_tables": 836096, "hand_f64_table": 2097152,
    },
    (1000, 1001): {
        "downslope_lift_w": 33309440, "slope_marks": 129280, "downslope_lift": 33034240, "downslope_queue": 8008448,
        "downslope_tables": 25025792, "hand_f64_table": 33554432,
    },
}

# recorded on 59e6e22, on an MI355X
DEVICE = {
    (1, 1): {
        "flowacc": 17920, "flowacc_weighted": 38144, "flowhand": 35584, "condition": 5632, "stream_order": 13312,
        "drainage": 8704, "upslope_length": 8704, "dinf_accumulate": 1024, "reach_catchments": 1536,
        "reach_catchments_own_reach": 1792, "reach_tables_k1": 512, "reach_tables_k1024": 8448,
    },
    (64, 64): {
        "flowacc": 17920, "flowacc_weighted": 38144, "flowhand": 37632, "condition": 25600, "stream_order": 124672,
        "drainage": 8704, "upslope_length": 8704, "dinf_accumulate": 49664, "reach_catchments": 1536,
        "reach_catchments_own_reach": 17920, "reach_tables_k1": 512, "reach_tables_k1024": 8448,
    },
    (65, 63): {
        "flowacc": 35328, "flowacc_weighted": 76032, "flowhand": 72448, "condition": 25600, "stream_order": 124672,
        "drainage": 16896, "upslope_length": 16896, "dinf_accumulate": 49664, "reach_catchments": 1536,
        "reach_catchments_own_reach": 17920, "reach_tables_k1": 512, "reach_tables_k1024": 8448,
    },
    (130, 257): {
        "flowacc": 260864, "flowacc_weighted": 568064, "flowhand": 528896, "condition": 172544,
        "stream_order": 1012224, "drainage": 123392, "upslope_length": 123392, "dinf_accumulate": 401920,
        "reach_catchments": 1536, "reach_catchments_own_reach": 135424, "reach_tables_k1": 512,
        "reach_tables_k1024": 8448,
    },
    (1000, 1001): {
        "flowacc": 4420096, "flowacc_weighted": 9679104, "flowhand": 8937472, "condition": 5010432,
        "stream_order": 30040576, "drainage": 2097664, "upslope_length": 2097664, "dinf_accumulate": 12012800,
        "reach_catchments": 7168, "reach_catchments_own_reach": 4011264, "reach_tables_k1": 512,
        "reach_tables_k1024": 8448,
    },
}


def export_sizes(L, H, W):
    from descriptools_amd._lib import Window
    # the same shape as one rank's core inside a larger raster: a halo of 2 cells, a row stride with 3 spare cells
    win = Window(H, W, W + 2 * 2 + 3, 5, 7, H + 20, W + 30, 2)
    return {
        "downslope_lift_w": int(L.dt_downslope_lift_workspace_w(C.byref(win))),
        "slope_marks": int(L.dt_slope_marks_bytes(H, W)),
        "downslope_lift": int(L.dt_downslope_lift_workspace(H, W)),
        "downslope_queue": int(L.dt_downslope_queue_workspace(H, W)),
        "downslope_tables": int(L.dt_downslope_tables_workspace(H, W)),
        "hand_f64_table": int(L.dt_hand_f64_table_bytes(H * W)),
    }


def device_sizes(L, H, W):
    """dt_ctx_scratch_bytes of a fresh context after one device-tier entry, per entry"""
    from descriptools_amd._lib import check
    from descriptools_amd.device import Context
    n = H * W
    host = {
        "fdr": np.full((H, W), 1, np.uint8),  # every cell flows east
        "dem": np.zeros((H, W), np.float32),
        "river": np.zeros((H, W), np.int8),
        "wt": np.ones((H, W), np.float64),
        "angle": np.zeros((H, W), np.float32),
        "link": np.full((H, W), -100, np.int64),
        "idx": np.full((H, W), -100, np.int64),
        "cat": np.full((H, W), -100, np.int32),
    }
    stages = {K: np.arange(1, K + 1, dtype=np.float64) for K in (1, 1024)}

    def st(K):
        return stages[K].ctypes.data_as(C.POINTER(C.c_double))

    entries = {
        "flowacc": lambda c, d, o: L.dt_dev_flowacc(c.h, d["fdr"], d["dem"], H, W, o(4)),
        "flowacc_weighted": lambda c, d, o: L.dt_dev_flowacc_weighted(c.h, d["fdr"], d["dem"], d["wt"], H, W, 10, o(8)),
        "flowhand": lambda c, d, o: L.dt_dev_flowhand(c.h, d["dem"], d["fdr"], d["river"], None, H, W, 10.0, o(4), o(4),
                                                      o(4), None),
        "condition": lambda c, d, o: L.dt_dev_condition_d8_async(c.h, d["dem"], H, W, 10.0, o(4), o(1), 4),
        "stream_order": lambda c, d, o: L.dt_dev_stream_order(c.h, d["fdr"], d["river"], H, W, o(1), o(8), o(8)),
        "drainage": lambda c, d, o: L.dt_dev_drainage(c.h, d["fdr"], d["dem"], None, H, W, 10.0, o(8), o(8), None),
        "upslope_length": lambda c, d, o: L.dt_dev_upslope_length(c.h, d["fdr"], d["dem"], H, W, 10.0, o(8)),
        "dinf_accumulate": lambda c, d, o: L.dt_dev_dinf_accumulate(c.h, d["angle"], None, H, W, 10, 2, o(8)),
        "reach_catchments": lambda c, d, o: L.dt_dev_reach_catchments(c.h, d["link"], d["idx"], 8, H, W, o(4), o(4),
                                                                      None, 0, None),
        "reach_catchments_own_reach": lambda c, d, o: L.dt_dev_reach_catchments(c.h, d["link"], d["idx"], 8, H, W, None,
                                                                                o(4), None, 0, None),
        "reach_tables_k1": lambda c, d, o: L.dt_dev_reach_tables(c.h, d["cat"], d["dem"], 4, None, H, W, st(1), 1, 1, 0,
                                                                 o(8, 1), o(8, 1), o(8, 1)),
        "reach_tables_k1024": lambda c, d, o: L.dt_dev_reach_tables(c.h, d["cat"], d["dem"], 4, None, H, W, st(1024),
                                                                    1024, 1, 0, o(8, 1024), o(8, 1024), o(8, 1024)),
    }
    sizes = {}
    for name, call in entries.items():
        ctx = Context()
        held = []
        try:
            assert int(L.dt_ctx_scratch_bytes(ctx.h)) == 0

            def out(itemsize, count=n):
                held.append(ctx.empty((count * itemsize,), np.uint8))
                return held[-1].ptr

            dev = {}
            for k, a in host.items():
                held.append(ctx.to_device(a))
                dev[k] = held[-1].ptr
            check(call(ctx, dev, out))
            ctx.sync()
            sizes[name] = int(L.dt_ctx_scratch_bytes(ctx.h))
        finally:
            for a in held:
                a.free()
            ctx.close()
    return sizes


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_size_only_exports(shape):
    from descriptools_amd import _lib
    assert export_sizes(_lib.lib(), *shape) == EXPORTS[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_context_scratch_after_each_entry(shape):
    from descriptools_amd import _lib
    assert device_sizes(_lib.lib(), *shape) == DEVICE[shape]


if __name__ == "__main__":
    import os
    import pprint
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from descriptools_amd import _lib
    lib = _lib.lib()
    print("EXPORTS =")
    pprint.pprint({s: export_sizes(lib, *s) for s in SHAPES}, width=110, sort_dicts=False)
    if lib.dt_device_count() >= 1:
        print("DEVICE =")
        pprint.pprint({s: device_sizes(lib, *s) for s in SHAPES}, width=110, sort_dicts=False)
