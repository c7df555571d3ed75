/*
 * descriptools_hip.h -- C ABI of libdescriptools_hip.so (MI355X / gfx950 terrain-descriptor engine)
 *
 * Drop-in boundary for the descriptools hot path.  Each entry point replaces one host<->device
 * shim (`*_cpu`) + Numba-CUDA kernel (`*_gpu`) pair of the reference (citations are
 * file:line relative to /root/reference/descriptools/).  Plain pointers and sizes only.
 *
 * Conventions:
 *   - rasters are row-major C-contiguous, H rows x W columns; nodata sentinel is -100;
 *   - DEM / HAND are float32 (int16 rasters are converted exactly by the caller);
 *   - D8 codes are ESRI: 1=E 2=SE 4=S 8=SW 16=W 32=NW 64=N 128=NE, 0 = nodata / undefined;
 *   - every function returns 0 on success and a negative DT_E* code on failure;
 *     dt_last_error() gives the message (thread-local).  Nothing falls back to the CPU.
 *
 * Two tiers:
 *   dt_<op>(...)      host pointers in / host pointers out (what the reference's *_cpu do);
 *   dt_dev_<op>(ctx,) device pointers, asynchronous on the context's stream -- the resident
 *                     chained / multi-GPU path.  Device buffers are caller-owned (hipMalloc,
 *                     torch tensors, ...); scratch is owned by the context.
 */
#ifndef DESCRIPTOOLS_HIP_H
#define DESCRIPTOOLS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DT_OK 0
#define DT_EINVAL (-1) /* bad shape / null pointer / unsupported size */
#define DT_EHIP (-2)   /* HIP runtime error (message in dt_last_error) */
#define DT_ENOMEM (-3) /* device allocation failed */
#define DT_ENODEV (-4) /* no usable GPU */

typedef struct dt_ctx dt_ctx;

/* One rank's CORE window (H x W cells) of a global Hg x Wg raster, at global offset (gy0, gx0).
 * Every raster pointer passed with a window addresses the core origin with row stride ld; `halo`
 * cells beyond the core exist in memory on every side (>= 1 when the global raster is larger).
 * Single GPU: ld = W, gy0 = gx0 = 0, Hg = H, Wg = W, halo = 0. */
typedef struct dt_window {
  int64_t H, W, ld, gy0, gx0, Hg, Wg, halo;
} dt_window;

/* ---- runtime ------------------------------------------------------------------------- */
const char *dt_last_error(void);
int dt_device_count(void);
const char *dt_version(void);
/* A/B knob: 1 = first-generation global kernels for flow accumulation / HAND / downslope (raster-wide
 * countdown, raster-wide pointer doubling, one thread per cell walking global memory), 2 = tile-hierarchical /
 * windowed (default; also selectable with the environment variable DT_FLOW_IMPL=v1).  Same results: bench.py
 * cross-checks the timed step against impl 1. */
int dt_set_flow_impl(int impl);
/* Test knobs, all 0 by default.  key 0 (DT_DBG_TWI_FLAG_ALL): the fused slope + TI + MTI stencil sends every
 * cell through its exact (cold) path as well as the fast one; keys 8-11: see csrc/dt_common.h.  Keys 1-7 selected
 * kernel variants of finished A/B runs and were retired with them: setting one is an error (DT_EINVAL) and changes
 * nothing.  key 12 (DT_DBG_POISON): 0x100 | b fills every workspace the library hands out with byte b before the
 * op that asked for it starts -- the context scratch at every reset, the host tier's device blocks (scratch, inputs
 * before their upload, outputs), the side buffers and dt_dev_malloc's blocks -- with hipMemsetAsync on the call's
 * stream; read at call time.  No result may depend on it.  Do not set it around dt_graph_begin / dt_graph_end: the
 * memsets would be recorded into the graph. */
int dt_debug_set(int key, int value);

/* Context = one device + one stream + grow-only scratch.  `stream` may be NULL (the context
 * creates its own non-blocking stream) or an existing hipStream_t (e.g. torch's). */
int dt_ctx_create(int device, void *stream, dt_ctx **out);
int dt_ctx_destroy(dt_ctx *ctx);
int dt_ctx_set_stream(dt_ctx *ctx, void *stream);
void *dt_ctx_stream(dt_ctx *ctx);
/* Two contexts of one device as concurrent branches of a pipeline: after dt_ctx_fork the child's stream waits
 * for everything enqueued so far on the parent's; after dt_ctx_join the parent's waits for the child's.
 * Device-side ordering only (events), the host never blocks.  The chain uses it to run downslope beside the
 * flow-accumulation / HAND kernels, whose latency chains leave most of the GPU idle. */
/* Re-create the context's own stream with a scheduling priority: -1 high, 0 normal, +1 low (clamped to the device's
 * range).  DT_EINVAL for a context that runs on a caller's stream. */
int dt_ctx_set_priority(dt_ctx *ctx, int priority);
int dt_ctx_fork(dt_ctx *parent, dt_ctx *child);
int dt_ctx_join(dt_ctx *parent, dt_ctx *child);
int dt_ctx_sync(dt_ctx *ctx);
/* HIP graphs.  Everything enqueued on the context's stream between dt_ctx_capture_begin and dt_ctx_capture_end
 * (dt_dev_* calls on this context, and on contexts forked from it and joined again) is recorded instead of run;
 * dt_graph_launch replays it with ONE launch on a context of the same device.  Capture a step whose buffers and
 * workspaces already exist (run it once first): allocation and synchronisation inside a capture fail.  The
 * pointers the calls were given are baked in.  No reference counterpart (the reference launches kernel by
 * kernel, descriptools/slope.py:190-200).  It frees the host (one call per step instead of ~45), it does not
 * shorten the step: the launches are asynchronous and already keep ahead of the GPU at every raster size tried. */
typedef struct dt_graph dt_graph;
int dt_ctx_capture_begin(dt_ctx *ctx);
int dt_ctx_capture_end(dt_ctx *ctx, dt_graph **out);
int dt_graph_launch(dt_graph *graph, dt_ctx *ctx);
int dt_graph_destroy(dt_graph *graph);
/* Sticky status bits raised by kernels since the last call (synchronises the context's stream, clears them).
 * DT_STATUS_ACC_OVERFLOW: a flow accumulation value of a multi-rank raster may have reached 2^31 cells while the step
 * ran with int32 accumulation rasters (the `_w` entry points; a device tile is < 2^31 cells), so its results are
 * not valid: rasters of more than 2^31 cells go through the `_w_a64` entry points (int64 rasters), which never raise it. */
#define DT_STATUS_ACC_OVERFLOW 1
/* DT_STATUS_NOT_CONVERGED: dt_dev_condition_d8_async's budget of rounds ran out before the fixed point (or a flat
 * cell was left without a code): the conditioned rasters of that step are not valid.  The other calls that take a
 * budget of rounds raise it the same way -- dt_dev_dinf_accumulate, dt_dev_mfd_accumulate, dt_dev_dinf_route,
 * dt_dev_mfd_route, dt_dev_cost_distance,
 * dt_dev_harmonic, dt_dev_wetness_modified_area (its last round still raised a cell: `modified` is not the least
 * solution yet; call again with a larger budget) and dt_dev_morph_reconstruct (the same: the output is not the
 * reconstruction yet). */
#define DT_STATUS_NOT_CONVERGED 2
/* DT_STATUS_BAD_WEIGHT: dt_dev_flowacc_weighted met a weight outside its contract (negative, NaN, infinite, or one whose
 * rint(w * 2^frac_bits) exceeds 2^52 / (H * W)): the weighted accumulation of that call is not valid. */
#define DT_STATUS_BAD_WEIGHT 4
/* DT_STATUS_REACH_RANGE: dt_dev_reach_tables met a catchment id >= the number of reaches it was given; that cell was
 * left out of the tables. */
#define DT_STATUS_REACH_RANGE 8
/* DT_STATUS_BAD_ANGLE: dt_dev_dinf_accumulate met an angle that is neither -1, -100 nor in [0, float32(2 pi)] (NaN
 * included); that cell was taken as -1 (no receiver). */
#define DT_STATUS_BAD_ANGLE 16
/* DT_STATUS_BAD_SHARES: dt_dev_mfd_accumulate met a share word outside its contract (not eight 0xFFFF, and a slot above
 * 32768 or slots that sum to neither 0 nor 32768); that cell was taken as having no receiver. */
#define DT_STATUS_BAD_SHARES 32
/* DT_STATUS_BAD_HEIGHT: dt_dev_focal met a valid height whose quantised value rint((z - origin) * 2^frac_bits) is
 * negative or over the bound of the call's largest radius; that cell counted as 0 and the rasters of that call are not
 * valid.  dt_dev_zonal_tables raises it for a participating value whose |rint((v - origin) * 2^frac_bits)| exceeds
 * 2^31 - 1; that cell was left out of the tables. */
#define DT_STATUS_BAD_HEIGHT 64
/* DT_STATUS_ZONE_RANGE: dt_dev_zonal_tables or dt_dev_zonal_counts met a zone id >= the number of zones it was given
 * (or a cross-tabulation column >= the number of columns); that cell was left out of the tables. */
#define DT_STATUS_ZONE_RANGE 128
/* DT_STATUS_NO_BACKLINK: dt_dev_cost_distance left a reached non-source cell without a back-link (rounding absorbed a
 * whole edge cost): backlink is 0 there, and indices is -100 there and on every cell whose links lead to it. */
#define DT_STATUS_NO_BACKLINK 256
/* DT_STATUS_BAD_PARAM: dt_dev_mfd_route or dt_dev_dinf_route met a parameter outside its mode's contract (NaN, negative,
 * a decay fraction above 1) on a cell that is not nodata; that cell passed its whole load on (the identity). */
#define DT_STATUS_BAD_PARAM 512
int dt_ctx_status(dt_ctx *ctx, int32_t *out);
int64_t dt_ctx_scratch_bytes(dt_ctx *ctx);
/* the base of that scratch (NULL before the first call that takes some): a device pointer that the next call which
 * needs more may free.  For tests that put guard bytes around what an entry carves out of it. */
void *dt_ctx_scratch_ptr(dt_ctx *ctx);

/* ---- host-pointer tier (drop-in for the reference's *_cpu shims) -----------------------
 * Device blocks behind these calls are cached per process (dt_host_trim frees the idle ones); dt_host_alloc /
 * dt_host_free give page-locked host memory for rasters that should cross PCIe at the full rate. */
int dt_host_trim(void);
int dt_host_alloc(int64_t bytes, void **out);
int dt_host_free(void *p);
/* dst[i] = (double)src[i] on the host with a few threads (float64 containers of float32 rasters, as the reference
 * returns them). */
int dt_host_f32_to_f64(const float *src, double *dst, int64_t n);


/* slope.slope_cpu + slope_gpu (slope.py:152-259): steepest-descent slope in percent.  The
 * -100 ring the reference pads on (slope.py:175-182) is implicit: neighbours outside the raster
 * are skipped like nodata neighbours. */
int dt_slope_f32(const float *dem, int64_t H, int64_t W, double px, float *slope);

/* Net-new N1 (no reference function; encoding pinned by flowhand.py:801-824): D8 code of the
 * neighbour that sets slope_gpu's maximum, first in its scan order.  `slope` may be NULL. */
int dt_d8_f32(const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *slope);

/* Net-new: D8 on a hydrologically conditioned surface, for DEMs with pits and flats (the reference
 * reads such an `fdr` from a GIS tool, Example/example.py:36).  Depressions are filled (priority-flood surface:
 * outlets = raster edge and cells next to nodata), D8 is taken on the filled surface, and the cells left without a
 * lower neighbour are routed over their flat to the nearest cell that has a code (hop distance through cells of
 * the same filled height; among the neighbours one hop closer the first of N,W,E,S, else of NW,NE,SW,SE); a
 * code-less cell next to nodata drains into its first nodata neighbour.  Every valid cell gets a code and the codes
 * contain no cycle.  filled (may be NULL) receives the filled surface; info3 (may be NULL) = {cells left without a
 * code (0), fill rounds, flat rounds}. */
int dt_d8_conditioned_f32(const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *filled,
                          int32_t *info3);
/* dt_d8_conditioned_f32's definition with the heights compared in float64 (a DEM that float32 cannot hold:
 * flowdir.d8_conditioned(heights="float64")); filled (may be NULL) receives the float64 filled surface. */
int dt_d8_conditioned_f64(const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr, double *filled,
                          int32_t *info3);

/* Net-new N2: flow accumulation = number of upstream cells excluding self; `dem` may be NULL,
 * otherwise cells with dem <= -100 are set to -100.  Cells on a D8 cycle get -100. */
int dt_flowacc_u8(const uint8_t *fdr, const float *dem, int64_t H, int64_t W, int64_t *acc);
/* Net-new: weighted flow accumulation, acc[c] = 2^-s * sum over the cells u strictly upstream of c of rint(w[u] * 2^s),
 * s = frac_bits, summed in int64 fixed point (exact and independent of order and tiling), on dt_flowacc_u8's D8 tree;
 * acc = -100 where dt_flowacc_u8 gives -100.  Nodata cells still pass their weight and inflow downstream, as they
 * pass their count (a caller who wants them out gives them weight 0).  Every weight must be finite and >= 0 with
 * H * W * rint(w * 2^frac_bits) <= 2^52 (flowacc.weight_frac_bits picks the largest such frac_bits for a raster);
 * otherwise the call fails and acc is not valid. */
int dt_flowacc_weighted(const uint8_t *fdr, const float *dem, const double *w, int64_t H, int64_t W, int frac_bits,
                        double *acc);
/* Net-new: stream order of the channel network `river` (nonzero = network cell) on the D8 raster `fdr`.  A network
 * cell c has the edge c -> d when its code is one of the eight D8 codes and points at an in-raster network cell d;
 * otherwise c is a network outlet.  Its children are the network cells with an edge into it.
 *   strahler (int8): 0 off the network; 1 with no children; else m + 1 when two or more children have the largest
 *                    child order m, m when one has.
 *   shreve (int64):  0 off the network; 1 with no children; else the sum of the children's magnitudes.
 *   link (int64):    -100 off the network; the flat index y * W + x of the head of the cell's link, where a cell is
 *                    its own head unless it has exactly one child, whose head it then takes.
 * Network cells that in-degree peeling never removes (on a D8 cycle of network cells) get -100 in all three.  Results
 * are exact integers.  shreve and link may be NULL (not written); a network of 2^31 cells or more is refused. */
int dt_stream_order(const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W, int8_t *strahler, int64_t *shreve,
                    int64_t *link);
/* Net-new: drainage on the D8 raster `fdr`.  c -> d is an edge when c's code is one of the eight D8 codes, d lies in
 * the raster and, when `dem` is given, neither c nor d is nodata (dem <= -100).  A valid cell with no edge is a
 * terminal.  `pour` (may be NULL): pour[i] > 0 is a pour point, anything else none.
 *   target (int64): the flat index y * W + x where c's path stops: the first cell on it (c included) with pour > 0
 *                   when pour is given, else its terminal.
 *   length (float64): from c to target, float64(n_card) * px + float64(n_diag) * (px * sqrt(2.0)) on the path's
 *                   exact move counts; 0 when c is its own target.
 *   label (int64, requires pour): pour[target]; 0 where the path reaches a terminal without meeting a pour point.
 * target and length are -100 on nodata, where the path enters a D8 cycle before it stops and (with pour) where it
 * ends at a terminal without meeting a pour point; label is -100 in the first two cases.  Any output may be NULL
 * (not written).  Rasters of 2^31 cells or more and a px that is not finite and > 0 are refused. */
int dt_drainage(const uint8_t *fdr, const float *dem, const int64_t *pour, int64_t H, int64_t W, double px,
                int64_t *target, double *length, int64_t *label);
/* Net-new: upslope (longest) flow length on dt_drainage's graph without pour points: for every cell c the length of
 * the longest path that ends at c (0 at a source), longest on the exact order of n_card + n_diag * sqrt(2), as
 * float64(n_card) * px + float64(n_diag) * (px * sqrt(2.0)).  -100 on nodata and on cells of a D8 cycle; cells that
 * drain into a cycle get their value.  Same refusals as dt_drainage. */
int dt_upslope_length(const uint8_t *fdr, const float *dem, int64_t H, int64_t W, double px, double *length);
/* Net-new: flow-path extremes of the float32 raster `values` on dt_drainage's graph.  kind 0: the maximum, 1: the
 * minimum (anything else: DT_EINVAL).  A NaN is no value and is skipped, -0.0 counts as +0.0 (and comes back as +0.0),
 * +-inf are ordinary values; between equal values the cell with the smallest flat index holds the extreme.
 *   dt_flowpath_upslope:    the extreme of values[s] over every valid cell s whose path contains c, s = c included.
 *                           Cells on a D8 cycle get the extreme over everything that reaches the cycle, the cycle
 *                           included.
 *   dt_flowpath_downstream: the extreme over the cells of c's path, from c to where it stops, both included.  Without
 *                           `stop` the path stops at its terminal; when it enters a D8 cycle the extreme is over its
 *                           tail and the whole cycle.  With `stop` (stop[i] != 0: a stop cell; on nodata: ignored) it
 *                           stops at the first stop cell, c included, and a cell whose path ends at a terminal or runs
 *                           round a cycle without meeting one has no value (where dt_drainage with these pour points
 *                           gives -100).
 *   value (float32): the extreme, NaN on nodata and where there is no value.
 *   where (int64):   the flat index y * W + x of the cell that holds it, -100 where value is NaN.
 * dem and stop may be NULL, so may value or where (not computed).  Exact: no arithmetic touches a value.  Rasters of
 * 2^31 cells or more are refused. */
int dt_flowpath_upslope(const uint8_t *fdr, const float *dem, const float *values, int64_t H, int64_t W, int kind,
                        float *value, int64_t *where);
int dt_flowpath_downstream(const uint8_t *fdr, const float *dem, const float *values, const uint8_t *stop, int64_t H,
                           int64_t W, int kind, float *value, int64_t *where);
/* Net-new: weighted flow-path sums on dt_drainage's graph (travel time with w = step length / velocity).  The weights
 * (float64, finite, >= 0) are quantised as dt_flowacc_weighted quantises them, q(c) = rint(w(c) * 2^frac_bits), round
 * half to even, under the same bound H * W * rint(max w * 2^frac_bits) <= 2^52 (a path has fewer than H * W moves, so
 * every sum converts to float64 exactly), and summed in unsigned 64-bit integers: exact, and independent of order,
 * tiling and run.  q(c) is the cost of the move out of c; the weight of the cell where a path stops is never counted.
 *   dt_flowpath_downstream_sum: T(target) = 0, T(c) = q(c) + T(succ(c)); the target is the path's terminal or, with
 *                               `stop` (stop[i] != 0; on nodata: ignored), the first stop cell on the path, c included.
 *                               out = T * 2^-frac_bits, and -100 exactly where dt_drainage (with stop as its pour
 *                               points) gives target -100: on nodata, where the path enters a D8 cycle before it
 *                               stops, and (with stop) where it reaches a terminal without meeting a stop cell.
 *   dt_flowpath_upslope_longest: U(c) = the largest sum of q over the cells of s's path from s up to, not including,
 *                               c, over every cell s whose path contains c (s = c: 0, so a source has 0); it equals
 *                               M(c) - T(c), M the largest stop-less T upslope of c.  out = U * 2^-frac_bits, and -100
 *                               wherever the stop-less T(c) is -100 -- wider than dt_upslope_length, which keeps the
 *                               cells that drain into a cycle.
 * dem and stop may be NULL; out NULL: nothing runs.  A frac_bits outside [-2200, 2200], a weight outside the contract
 * and rasters of 2^31 cells or more are refused. */
int dt_flowpath_downstream_sum(const uint8_t *fdr, const float *dem, const double *weights, const uint8_t *stop,
                               int64_t H, int64_t W, int frac_bits, double *out);
int dt_flowpath_upslope_longest(const uint8_t *fdr, const float *dem, const double *weights, int64_t H, int64_t W,
                                int frac_bits, double *out);
/* Net-new: depression carving (Soille 2004; the complete form of breaching).  fdr and filled as dt_d8_conditioned_f32
 * gives them for dem; lowest = dt_flowpath_upslope(fdr, dem, dem, kind 1): the lowest height above or at each cell on
 * the conditioned D8 tree, which is non-increasing along every edge and <= dem.  carved = lowest when max_cut is +inf,
 * else max(lowest, filled - float32(max_cut)), subtraction and maximum in float32: at most max_cut is cut and the rest
 * filled; max_cut 0 gives filled.  Nodata cells (dem <= -100) keep their dem value.  filled may be NULL; info3 as in
 * dt_d8_conditioned_f32.  A negative or NaN max_cut is refused, and what dt_drainage refuses.  NaN and +inf heights
 * are outside the contract, as they are for the conditioning. */
int dt_carve(const float *dem, int64_t H, int64_t W, double px, double max_cut, uint8_t *fdr, float *carved,
             float *filled, int32_t *info3);
/* Net-new: D-infinity (Tarboton 1997) flow direction.  angle (float32): radians counter-clockwise from east, rows
 * growing to the south, so octant k = 0..7 (the neighbour at k pi / 4) is E, NE, N, NW, W, SW, S, SE (D8 codes 1, 128,
 * 64, 32, 16, 8, 4, 2).  A height is valid when it is finite and > -100.  For a valid centre e0 the eight facets
 * (e1, e2, ac, af) = (E, NE, 0, +1), (N, NE, 1, -1), (N, NW, 1, +1), (W, NW, 2, -1), (W, SW, 2, +1), (S, SW, 3, -1),
 * (S, SE, 3, +1), (E, SE, 4, -1) are tried in this order, those with both neighbours in the raster and valid, in
 * float64: s1 = (e0 - e1) / px, s2 = (e1 - e2) / px; s2 < 0: r = 0, s = s1; else s2 > s1: r = pi / 4, s = (e0 - e2) /
 * (px * sqrt(2.0)); else r = atan2(s2, s1), s = sqrt(s1 * s1 + s2 * s2).  The largest s > 0 wins (strict >: the first
 * of equals); angle64 = af * r + ac * (pi / 2), less 2 pi when >= 2 pi; angle = float32(angle64), 0 when that is >=
 * float32(2 pi); slope = float32(s), drop over distance.  A valid centre without a winning facet: when fdr (may be
 * NULL) holds a D8 code there whose neighbour is in the raster and valid, angle = float32(k pi / 4) of that octant,
 * else -1 (no flow); slope 0.  A centre that is NaN or +inf: -1 and 0.  A nodata centre (<= -100): -100 and -100;
 * -inf is <= -100 and therefore nodata, as in every other entry of this library, not a non-finite centre.
 * slope may be NULL.  Rasters of 2^31 cells or more and a px that is not finite and > 0 are refused. */
int dt_dinf_direction(const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px, float *angle,
                      float *slope);
/* Net-new: D-infinity contributing area of an angle raster (dt_dinf_direction's, or a TauDEM `ang` grid).  An angle
 * a >= 0 is decoded as t = float64(a) * 1.2732395447351628: when |t - rint(t)| <= 2^-20 the cell has one receiver,
 * octant rint(t) mod 8; else k = floor(t), P2 = rint((t - k) * 2^30), and its receivers are octant k mod 8 with share
 * 2^30 - P2 and octant (k + 1) mod 8 with share P2.  -1: no receiver; -100: nodata; anything else fails the call.
 * c -> d is an edge for each receiver d in the raster that is not nodata (other shares leave the domain).  With
 * q(c) = rint(w(c) * 2^s), s = frac_bits (w NULL: 1 everywhere; the rules of dt_flowacc_weighted), T(c) = q(c) + what
 * c receives; a complete c sends m2 = floor(T * P2 / 2^30) to octant k + 1 and T - m2 to octant k.
 * acc = ldexp(T - q, -s) (self excluded), -100 on nodata and on every cell on or below a cycle.  Exact integer sums:
 * the result does not depend on order or run.  info4 (may be NULL) = {queue rounds that found work, the largest
 * number of cells one round drained, cells queued in all, two-receiver cells}. */
int dt_dinf_accumulate(const float *angle, const double *w, int64_t H, int64_t W, int frac_bits, double *acc,
                       int64_t *info4);
/* Net-new: D-infinity distance down to the stream (TauDEM's DinfDistDown as we read it; descriptools_amd/dinf.py and
 * the test suite's numpy reference are the definition).  angle is decoded as in dt_dinf_accumulate (an angle outside
 * the contract raises DT_STATUS_BAD_ANGLE and fails the call); a target is a cell with river == 1 whose angle is not
 * -100; dem (may be NULL) holds float32 heights taken as given.  Measures: horizontal h, vertical v, surface s.  A hop
 * c -> d at octant k has L = px (k even) or px * 1.4142135623730951, dz = (double)dem[c] - (double)dem[d],
 * S = sqrt(L * L + dz * dz).  Targets reach with h = v = s = 0; a non-target, non-nodata cell without any edge is dead;
 * any other cell settles once every receiver it has an edge to is settled: with check_edges = 1 it reaches iff no share
 * leaves the domain and every receiver reaches, with check_edges = 0 iff at least one receiver reaches; else it is
 * dead; a cell on a cycle, or above one, never settles.  A reaching cell takes the terms t_j = m(d_j) + hop_m(c -> d_j)
 * over its reaching receivers in the order j = 0, 1: one term is the value; two give, per measure, stat 0 (ave)
 * ((double)w0 * t0 + (double)w1 * t1) * 2^-30 with w0 = 2^30 - P2, w1 = P2, stat 1 (min) t1 < t0 ? t1 : t0, stat 2 (max)
 * t1 > t0 ? t1 : t0.  h, v, s are float64 with -100 on nodata and wherever a cell does not reach; IEEE float64 in this
 * association, a pure function of the receivers' final values: independent of schedule, rounds and run.  dem, v, s and
 * info4 may be NULL; v or s without dem is DT_EINVAL.  visit_limit: 0, or n >= 1 caps the sweeps a workgroup makes over
 * its tile per visit (tests: it forces many rounds on small rasters; the outputs do not depend on it).  info4 = {rounds
 * that settled something, cells that reach, dead cells, unsettled non-nodata cells}.  The call ends when a round
 * settles nothing: a cycle costs one empty round.  Rasters of 2^31 cells or more and a px that is not finite and > 0
 * are refused. */
int dt_dinf_distance_down(const float *angle, const int8_t *river, const float *dem, int64_t H, int64_t W, double px,
                          int stat, int check_edges, int visit_limit, double *h, double *v, double *s,
                          int64_t *info4);
/* Net-new: multiple-flow-direction (MFD; Quinn et al. 1991, Freeman 1991, Holmgren 1994) flow shares of a DEM
 * (descriptools_amd/mfd.py holds the full definition).  shares is uint16[H][W][8], 16-byte aligned; the last axis is
 * the octant as in dt_dinf_direction (E, NE, N, NW, W, SW, S, SE), the unit 2^-15.  A height is valid when it is finite
 * and > -100.  A nodata centre (<= -100, -inf included) stores eight 0xFFFF, a NaN or +inf centre eight zeros.  The
 * receivers of a valid centre z0 are the neighbours in the raster that are valid and strictly lower; in float64, in
 * octant order: d = z0 - z_k, g = d (k even) or d / 1.4142135623730951 (k odd), u = g / max g, f = u^p (p integer-valued:
 * p successive products from 1.0; otherwise pow(u, p)), with contour != 0 times 0.5 (k even) or 0.35355339059327373
 * (k odd); F = the sum of the f in octant order, r = f / F.  The main receiver has the largest f (the first of equals);
 * every other stores floor(ldexp(r, 15)) and the main one 32768 less their sum, so a cell's shares sum to 32768.  A
 * valid centre without a lower neighbour: when fdr (may be NULL) holds a D8 code there whose neighbour is in the raster
 * and valid, 32768 in that octant; else eight zeros.  The pixel size cancels out of every share.  exponent must be
 * finite and in [0, 64]; rasters of 2^31 cells or more are refused. */
int dt_mfd_shares(const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double exponent, int contour,
                  uint16_t *shares);
/* Net-new: MFD contributing area of a share raster (dt_mfd_shares', or any raster under its contract: a word of eight
 * 0xFFFF is nodata; in any other every slot is <= 32768 and the slots sum to 0 or 32768; anything else fails the call).
 * c -> d is an edge for each octant k with P_k > 0 whose neighbour d is in the raster and not nodata (other shares leave
 * the domain); the main receiver is the slot with the largest P, the first of equals.  With q(c) = rint(w(c) * 2^s),
 * s = frac_bits (w NULL: 1 everywhere; the rules of dt_flowacc_weighted), T(c) = q(c) + what c receives; a complete c
 * sends m_k = floor(T * P_k / 2^15) to every other receiver k and T less their sum to the main one.
 * acc = ldexp(T - q, -s) (self excluded), -100 on nodata and on every cell on or below a cycle.  Exact integer sums: the
 * result does not depend on order or run.  info4 (may be NULL) = {queue rounds that found work, the largest number of
 * cells one round drained, cells queued in all, cells with two or more receivers}. */
int dt_mfd_accumulate(const uint16_t *shares, const double *w, int64_t H, int64_t W, int frac_bits, double *acc,
                      int64_t *info4);
/* Net-new: decayed, retention-limited and transport-limited accumulation (descriptools_amd/routing.py holds the
 * definition).  The graph, nodata, q(c) = rint(w(c) * 2^s), the split and the -100 on or below a cycle are those of
 * dt_mfd_accumulate (share raster) and dt_dinf_accumulate (angle raster); what changes is what a complete cell sends.
 * With the load T(c) = q(c) + what c receives, the outflow is O(c) = f(T(c), param(c)) and R(c) = T(c) - O(c) stays in
 * the cell; the receivers get the accumulation's split applied to O instead of T (MFD: floor(O * P_k / 2^15) to every
 * receiver but the main one, the rest to the main one; D-infinity: floor(O * P2 / 2^30) and O less that).  param is a
 * float64 raster, never NULL; by mode
 *   DT_ROUTE_DECAY   the fraction passed on, in [0, 1]: D = rint(ldexp(p, 30)), O = floor(T * D / 2^30), the product taken
 *                    as (T >> 30) * D + (((T & (2^30 - 1)) * D) >> 30);
 *   DT_ROUTE_RETAIN  a capacity >= 0 (+inf allowed): C = min(rint(ldexp(p, s)), 2^53), O = T - C when T > C, else 0;
 *   DT_ROUTE_LIMIT   the same C: O = min(T, C).
 * 1, 0 and +inf are the identities of the three modes (O = T).  A cell without receivers still has its O and R; its O
 * leaves the domain, as does the part of a share that points off the raster or into nodata.  O <= T, so no sum exceeds
 * the accumulation's bound.  The outputs, float64, each may be NULL but not all four: inflow = ldexp(T - q, -s) (what the
 * accumulation returns when the parameter is the identity), load = ldexp(T, -s), outflow = ldexp(O, -s), retained =
 * ldexp(R, -s); -100 where the accumulation gives -100.  Exact integer sums: independent of order, rounds and run.  A
 * parameter that is NaN, negative or (decay) above 1 on a cell that is not nodata fails the call; a bad angle, share
 * word or weight as in the accumulations.  info4 as theirs. */
#define DT_ROUTE_DECAY 1
#define DT_ROUTE_RETAIN 2
#define DT_ROUTE_LIMIT 3
int dt_mfd_route(const uint16_t *shares, const double *w, const double *param, int64_t H, int64_t W, int frac_bits,
                 int mode, double *inflow, double *load, double *outflow, double *retained, int64_t *info4);
int dt_dinf_route(const float *angle, const double *w, const double *param, int64_t H, int64_t W, int frac_bits,
                  int mode, double *inflow, double *load, double *outflow, double *retained, int64_t *info4);
/* Net-new: local terrain attributes of the quadratic fitted by least squares over the (2 radius + 1)^2 window of
 * every cell (Evans 1980, Wood 1996; descriptools_amd/terrain.py holds the full definition).  A height is valid when
 * it is finite and > -100; a cell has a value when all n^2 heights of its window (n = 2 radius + 1) lie in the raster
 * and are valid, and holds -100 in every output otherwise.  All arithmetic is IEEE float64, sums from their first term
 * in ascending offset (i: columns, east positive; j: rows, south positive; -radius .. radius), the integer factor
 * converted and multiplied before each addition: C0 = sum_j z, C1 = sum_j (-j) z, C2 = sum_j (j j) z down a column,
 * then M00 = sum_i C0, M10 = sum_i i C0, M20 = sum_i (i i) C0, M01 = sum_i C1, M11 = sum_i i C1, M02 = sum_i C2 along
 * the row.  With S2 = r(r+1)(2r+1)/3, S4 = r(r+1)(2r+1)(3r^2+3r-1)/15, D = n S4 - S2^2, h = px: den1 = (double)(n S2) h,
 * den2 = (double)(S2^2) (h h), den3 = (double)(n D) (h h); p = M10 / den1, q = M01 / den1 (x east, y north),
 * s = M11 / den2, r = 2 ((n M20 - S2 M00) / den3), t = 2 ((n M02 - S2 M00) / den3).  w = p p + q q, g1 = 1 + w,
 * pq2 = 2 (p q); each output is (float) of: gradient sqrt(w) (rise over run); aspect, degrees clockwise from north of
 * the downslope direction: a = atan2(-p, -q) 57.29577951308232, + 360 when a < 0, 0 when (float)a >= 360, -1 when
 * w == 0; profile -(((p p) r + pq2 s) + (q q) t) / (w (g1 sqrt(g1))); plan -(((q q) r - pq2 s) + (p p) t) / (w sqrt(w));
 * tangential the same numerator over w sqrt(g1) (the three are 0 when w == 0); mean -(((1 + q q) r - pq2 s) +
 * (1 + p p) t) / (2 (g1 sqrt(g1))); laplacian r + t; hillshade ((sz - p sx) - q sy) / sqrt(g1), 0 when that is not > 0,
 * (sx, sy, sz) the unit vector to the sun (east, north, up).  Positive curvature is convex.  Every output but aspect is
 * a pure function of the heights in this association: bit for bit the numpy reference of the test suite.  Each output
 * may be NULL (it is then neither computed nor stored) but not all of them.  radius must lie in [1, 32], the sun
 * vector must be finite; rasters of 2^31 cells or more and a px that is not finite and > 0 are refused. */
int dt_terrain(const float *dem, int64_t H, int64_t W, double px, int radius, double sx, double sy, double sz,
               float *gradient, float *aspect, float *profile, float *plan, float *tangential, float *mean,
               float *laplacian, float *hillshade);
/* Net-new: what a cell sees along eight lines of sight -- geomorphon landforms and patterns (Jasiewicz & Stepinski
 * 2013), positive and negative topographic openness (Yokoyama et al. 2002), the sky-view factor (Zaksek et al. 2011);
 * descriptools_amd/horizon.py holds the full definition.  A height is valid when it is finite and > -100.  Directions
 * d = 0..7 = N, NE, E, SE, S, SW, W, NW with row / column steps (-1,0) (-1,1) (0,1) (1,1) (1,0) (1,-1) (0,-1) (-1,-1).
 * For a valid centre z0 the samples of direction d are the cells k = skip + 1 .. radius steps away that lie in the
 * raster and are valid; cells that are not are skipped, the line of sight goes on past them.  IEEE float64 on the
 * float32 heights: step[0] = px, step[1] = px * 1.4142135623730951 (diagonals), inv[c][k] = 1.0 / ((double)k *
 * step[c]) (tabulated on the host by the entry), t = ((double)z_k - (double)z0) * inv[c][k] -- a multiplication by the
 * tabulated reciprocal, by definition; tmax_d / tmin_d = the largest / smallest t of direction d.  A cell has a value
 * iff its centre is valid and every direction has a sample; any other cell holds 0 in landform, 65535 in pattern and
 * -100 in the float outputs.  Digit of a direction against flat_tan = tan(flatness angle): +1 if |tmax| > |tmin| and
 * |tmax| > flat_tan; else -1 if |tmin| > flat_tan and |tmax| <= |tmin|; else 0.  pattern = sum_d (digit_d + 1) 3^d
 * (0..6560).  landform = 1 flat, 2 peak, 3 ridge, 4 shoulder, 5 spur, 6 slope, 7 hollow, 8 footslope, 9 valley,
 * 10 pit, from the numbers m of -1 digits and p of +1 digits by the table of horizon.py (rows m = 0..8, columns
 * p = 0..8-m: 1 1 1 8 8 9 9 9 10 / 1 1 8 8 8 9 9 9 / 1 4 6 6 7 7 9 / 4 4 6 6 6 7 / 4 4 5 6 6 / 3 3 5 5 / 3 3 3 /
 * 3 3 / 2).  positive = (float)((sum_d (pi/2 - atan(tmax_d))) / 8.0), negative = (float)((sum_d (pi/2 + atan(tmin_d)))
 * / 8.0), radians, summed over d = 0..7 in order; sky_view = (float)(1.0 - (sum_d s_d) / 8.0) with s_d = tmax_d /
 * sqrt(1.0 + tmax_d tmax_d) when tmax_d > 0, else 0.  landform, pattern and sky_view are pure functions of the heights
 * in this association: bit for bit the numpy reference of the test suite; the two openness rasters hold eight atan
 * each and are within one float32 spacing of it.  Each output may be NULL (it is then neither computed nor stored)
 * but not all of them.  radius must lie in [1, 64], skip in [0, radius - 1], flat_tan must be finite and >= 0;
 * rasters of 2^31 cells or more and a px that is not finite and > 0 are refused. */
int dt_horizon(const float *dem, int64_t H, int64_t W, double px, int radius, int skip, double flat_tan,
               uint8_t *landform, uint16_t *pattern, float *positive, float *negative, float *sky_view);
/* Net-new: focal statistics at any radius -- count, mean and standard deviation of the heights in the (2 R + 1)^2 window
 * of every cell, the topographic position index TPI (Weiss 2001), the deviation from mean elevation DEV (De Reu et al.
 * 2013) and the multi-scale DEVmax with its scale (Lindsay et al. 2015); descriptools_amd/focal.py holds the full
 * definition.  A height is valid when it is finite and > -100.  Quantisation: q = (int64)rint(((double)z - origin) *
 * 2^frac_bits), rint to even, of a valid cell; the window of radius R is the square clipped to the raster, invalid
 * cells in it are skipped, and a cell has a value iff its own height is valid.  With q_c the centre's q, over the valid
 * cells i of the window: n the count, A = sum (q_i - q_c), B = sum (q_i - q_c)^2, exact integers.  They come from the
 * inclusive two-dimensional prefix sums of [valid], q and q^2, the latter two uint64 with wrap-around: a window sum is
 * the four-corner difference modulo 2^64, A = S1 - n q_c, B = S2 - 2 q_c S1 + n q_c^2 modulo 2^64, read as int64.
 * Contract: 0 <= q <= qmax(R_max), the largest integer with (2 R_max + 1)^2 qmax^2 < 2^63, R_max the call's largest
 * radius; a valid height outside it raises DT_STATUS_BAD_HEIGHT, counts as q = 0 and fails the call.  Float stage,
 * IEEE float64 in this association: nf = (double)n, a = (double)A / nf, b = (double)B / nf, var = b - a a (0 when
 * negative), sd = sqrt(var), u = 2^-frac_bits.  count = n (int32; 0 without a value), mean = (float)(origin +
 * ((double)q_c + a) u) and std = (float)(sd u) (population; -100 without a value), tpi = (float)((-a) u) and dev =
 * (float)((-a) / sd), 0.0 when sd == 0 (NaN without a value).  radii is a strictly increasing table of n_radii radii
 * (1..32, each in [1, 4096]) in host memory.  n_radii == 1: each of count, mean, std, tpi, dev, scale may be NULL, not
 * all; scale = the radius (uint16; 0 without a value).  n_radii > 1 (DEVmax): only dev and scale may be given; per
 * cell d_k = (-a_k) / sd_k (0 when sd_k == 0) in float64 for every radius, the one of largest |d_k| is kept, a tie
 * keeps the smaller radius; dev = (float)d_k, scale = that radius.  frac_bits must lie in [0, 24], origin must be
 * finite; rasters of 2^31 cells or more are refused.  Every output is the numpy reference's bit for bit. */
int dt_focal(const float *dem, int64_t H, int64_t W, double origin, int frac_bits, const int32_t *radii, int n_radii,
             int32_t *count, float *mean, float *std, float *tpi, float *dev, uint16_t *scale);
/* Net-new: DEM filters; descriptools_amd/filters.py holds the full definition.  A height is valid when it is finite and
 * > -100; the window of radius R is the (2 R + 1)^2 square clipped to the raster, invalid cells in it are skipped, and a
 * cell has a value iff its own height is valid (-100 otherwise).  Heights are ordered by the order-preserving integer
 * key of their float32 bits (u ^ 0x80000000 for a clear sign bit, ~u otherwise: the order of the reals, -0.0 below
 * +0.0), so every extreme and every rank is the bit pattern of one of the window's heights.
 * dt_filter_extremes: minimum and maximum of the window's valid heights, range = (float)((double)maximum -
 * (double)minimum), opening = the maximum over the window of the minimum raster and closing = the minimum over the
 * window of the maximum raster (the no-value cells of the first raster are invalid in the second pass; they are the
 * invalid cells of the input).  Each output may be NULL (then neither computed nor stored), not all.  radius in
 * [1, 4096]; the cost per cell does not depend on it.
 * dt_filter_rank: the element of index table[n] of the window's n valid heights sorted ascending.  table holds
 * n_table = (2 radius + 1)^2 + 1 entries in host memory, table[n] < max(n, 1); radius in [1, 16].
 * dt_filter_denoise: feature-preserving denoising (Sun et al. 2007), float64 arithmetic (+, -, *, /, sqrt) on the
 * float32 heights in the association filters.py states: unit normals of the 3 x 3 Sobel gradient (a missing neighbour
 * is 2 z_c - z_opposite, or z_c), held as float32; over the valid cells i of the window, row-major, c = n_c . n_i and,
 * where c > cos_threshold, w = (c - cos_threshold)^2 and m += w n_i; m / |m| held as float32; then `iterations` Jacobi
 * steps: over the valid neighbours E, SE, S, SW, W, NW, N, NE whose smoothed normal passes the same test, sw += w and
 * sz += w (z_i + (a_i dx px + b_i dy px) / c_i); (float)(sz / sw) replaces the height iff it is within max_change of
 * the input height.  Invalid cells keep their bits.  radius in [1, 16], cos_threshold in (0, 1), iterations in
 * [1, 32], max_change finite and > 0, px finite and > 0; out must not be dem.
 * Rasters of 2^31 cells or more are refused.  Every output is the numpy reference's bit for bit. */
int dt_filter_extremes(const float *dem, int64_t H, int64_t W, int radius, float *minimum, float *maximum, float *range,
                       float *opening, float *closing);
int dt_filter_rank(const float *dem, int64_t H, int64_t W, int radius, const uint16_t *table, int n_table, float *out);
int dt_filter_denoise(const float *dem, int64_t H, int64_t W, double px, int radius, double cos_threshold,
                      int iterations, double max_change, float *out);
/* Net-new: the multi-resolution valley bottom flatness MRVBF and ridge top flatness MRRTF (Gallant & Dowling 2003) and
 * their two building blocks; descriptools_amd/mrvbf.py holds the full definition.  A height is valid when it is finite
 * and > -100; all arithmetic is IEEE float64 on the float32 heights, the rasters of a pyramid level are float32.
 * dt_percentile: over the disc dx^2 + dy^2 <= radius^2 clipped to the raster, centre included, n valid cells, l of them
 * strictly lower and h strictly higher than the centre (compared as float32): lower = (float)((double)l / n), higher =
 * (float)((double)h / n), -100 where the centre is not valid.  Each may be NULL, not both; radius in [1, 16].
 * dt_coarsen: one generalisation step of a raster of cell size px.  g6[k] = exp(-k^2 / 18), k = 0..5 (host memory).
 * Row sums of g z over the valid cells of the 11 taps, k ascending -5..5, then column sums of those, again ascending;
 * the same of g [valid]; the smoothed height of a valid cell is their quotient, its slope (percent) takes central
 * differences over 2 px where both neighbours are valid, one-sided ones over px where one is, 0 where none is, S = 100
 * sqrt(p p + q q).  dem3 / slope3[I][J] = the mean of the smoothed height / of the slope over the valid cells of rows
 * 3I..3I+2 and columns 3J..3J+2 (clipped, row-major sum over count), -100 where the block has none; both are rasters of
 * ceil(H / 3) x ceil(W / 3) cells.  Both ops equal the numpy reference of the tests bit for bit.
 * dt_mrvbf: the index over `levels` levels (2..10; levels 1 and 2 are the base raster, level L >= 3 the raster
 * coarsened L - 2 times) with the first slope threshold slope_threshold (percent, finite and > 0), the percentile
 * thresholds pctl_valley and pctl_ridge in (0, 1] and the exponents p[L - 2] of the levels L = 2..levels (host memory;
 * log10((L - 0.5) / 0.1) / log10(1.5)).  mrvbf and mrrtf may each be NULL (then neither computed nor stored), not
 * both; -100 where the height is not valid.  One pow per level and output: the tests hold it to one float32 spacing of
 * the reference.  Rasters of 2^31 cells or more and a px that is not finite and > 0 are refused. */
int dt_mrvbf(const float *dem, int64_t H, int64_t W, double px, double slope_threshold, int levels, double pctl_valley,
             double pctl_ridge, const double *p, float *mrvbf, float *mrrtf);
int dt_percentile(const float *dem, int64_t H, int64_t W, int radius, float *lower, float *higher);
int dt_coarsen(const float *dem, int64_t H, int64_t W, double px, const double *g6, float *dem3, float *slope3);
/* Net-new: exact Euclidean proximity to the river network.  A source is a cell with river == 1 that is not nodata;
 * nodata is a cell with nod <= -100, where nod (may be NULL: no nodata) is any float32 raster of the shape: a float32
 * DEM, or for heights float32 cannot hold the -100 / 0 mask of the DEM's own comparison (descriptools_amd._lib.
 * nodata_mask).  For a cell c = (y, x) and a source s = (ys, xs), d2 = (y - ys)^2 + (x - xs)^2 in int64; nearest(c) is
 * the source of smallest d2, among equals the one of smallest flat index ys * W + xs.  indices = that flat index,
 * distance = float32(px * sqrt(float64(d2))), both operations in float64.  Both are -100 on nodata (which is no
 * barrier: distances are straight lines over it) and when the raster has no source.  The result is exact and does not
 * depend on order or run; the work is O(H W log H) whatever the sources.  Rasters of 2^31 cells or more and a px that
 * is not finite and > 0 are refused.  HAND above the nearest source: dt_hand_f32 / dt_hand_f64 on indices. */
int dt_proximity(const int8_t *river, const float *nod, int64_t H, int64_t W, double px, float *distance,
                 int64_t *indices);
/* Net-new: cost distance, cost allocation and back-links over a friction raster (the GIS cost distance / allocation /
 * back link, GRASS r.cost; descriptools_amd/cost.py and the test suite's Dijkstra are the definition).  A cell is
 * passable iff 0 < friction < +inf (zero, negatives, NaN and +inf are barriers; a diagonal move between two barriers
 * is allowed); a source is a passable cell with sources == 1.  Adjacent passable cells u, v (connectivity 8, or 4:
 * cardinal moves only) are joined by w(u, v) = step * ((f(u) + f(v)) * 0.5) in float64, one rounding per operation,
 * step = px (cardinal) or px * 1.4142135623730951 (diagonal).  cost = A, the greatest solution of A(s) = 0 at the
 * sources and A(v) = min over neighbours u of fl(A(u) + w(u, v)) elsewhere: what Dijkstra returns, to the bit, whatever
 * the schedule.  backlink(v) = the ESRI D8 code (1 E, 2 SE, 4 S, 8 SW, 16 W, 32 NW, 64 N, 128 NE) of the first
 * neighbour u in the order NW, N, NE, W, E, SW, S, SE with A(u) < A(v) and fl(A(u) + w(u, v)) == A(v); 0 on sources.
 * indices(v) = the flat index of the source at the root of v's back-link tree (a source: itself).  Barriers and
 * unreached cells hold cost -100, indices -100, backlink 0.  A reached non-source cell without such a neighbour (rounding
 * absorbed a whole edge cost) is counted: backlink 0, indices -100 there and on the cells whose links lead to it.
 * cost is float64, indices int64, backlink uint8; indices, backlink and info4 may be NULL.  visit_limit: 0, or n >= 1
 * caps the sweeps a workgroup makes over its tile per visit (tests: the outputs do not depend on it).  info4 = {rounds
 * that lowered something, reached cells, reached non-source cells without a back-link, tile visits}.  The call ends
 * when a round lowers nothing.  Rasters of 2^31 cells or more and a px that is not finite and > 0 are refused. */
int dt_cost_distance(const float *friction, const int8_t *sources, int64_t H, int64_t W, double px, int connectivity,
                     int visit_limit, double *cost, int64_t *indices, uint8_t *backlink, int64_t *info4);
/* Net-new: the SAGA wetness index (Boehner & Selige 2006; descriptools_amd/wetness.py and the test suite's reference
 * are the definition, not SAGA's code).  area float64, slope float32 radians, suction float32, H x W with fewer than
 * 2^31 cells.
 * dt_wetness_suction: in float64 with one rounding per operation, b = max(slope + slope_offset, slope_min), e =
 * slope_weight * b, L = log(t) taken once on the host, s = exp(-((e * exp(exp(e * L))) * L)) = (1/t)^(e exp(t^e)),
 * rounded to float32, 0 below the smallest normal float32; -100 where the slope is NaN or not in [0, pi/2).
 * dt_wetness_modified_area: a cell is valid iff 0 < area < +inf and 0 <= suction <= 1; every other cell is nodata, is
 * nobody's neighbour and holds -100.  modified = M, the least solution of M(v) = max(A(v), fl(float64(s(v)) * max over
 * the valid 8-neighbours u of M(u))): what a max-heap Dijkstra returns, to the bit, whatever the schedule.
 * visit_limit: 0, or n >= 1 caps the sweeps a workgroup makes over its tile per visit (tests: the outputs do not depend
 * on it).  info4 (may be NULL) = {rounds of tile visits that raised something, raised cells (M > A), tile visits, 0}.
 * dt_wetness_saga: the suction of `slope`, the modified area of `area` under it and swi = float32(log(M / tan(b))),
 * -100 where the cell is not valid or b >= pi/2, in one call on the device; modified and suction may be NULL.
 * Refused: t not finite or <= 1, slope_weight not finite or <= 0, a negative or non-finite slope_offset or slope_min,
 * both of them 0 for dt_wetness_saga, a negative visit_limit, 2^31 cells or more. */
int dt_wetness_suction(const float *slope, int64_t H, int64_t W, double t, double slope_weight, double slope_offset,
                       double slope_min, float *suction);
int dt_wetness_modified_area(const double *area, const float *suction, int64_t H, int64_t W, int visit_limit,
                             double *modified, int64_t *info4);
int dt_wetness_saga(const double *area, const float *slope, int64_t H, int64_t W, double t, double slope_weight,
                    double slope_offset, double slope_min, int visit_limit, float *swi, double *modified,
                    float *suction, int64_t *info4);
/* Net-new: raster resampling (descriptools_amd/resample.py holds the definition, the test suite's numpy reference
 * matches it bit for bit): src (Hs x Ws) read onto a destination grid (Hd x Wd).  matrix = (a0, a1, a2, b0, b1, b2)
 * maps destination to source pixel-corner coordinates, u = (a0 + a1 x) + a2 y, v = (b0 + b1 x) + b2 y, column first.
 * method: 0 nearest, 1 bilinear, 2 cubic (Keys, a = -0.5; bilinear where the 4 x 4 window is not whole), 3 average,
 * 4 sum, 5 min, 6 max, 7 mode.  dtype: the element size in bytes (1, 2, 4, 8) for nearest, which copies bits; 1
 * (uint8) for mode; 32 (float32) or 64 (float64) for the others, which compute in float64, treat a cell as valid iff
 * it is finite and > -100, never let a value reach a destination cell whose containing source cell is invalid, and
 * write -100 where there is no value.  fill_bits: the element (in the low bytes) that nearest and mode write where
 * there is nothing to take.  nodata: -1, or the uint8 value that mode does not count.  Methods 3-7 are footprint
 * reductions over the source cells that destination cell (i, j) = [a0 + a1 j, a0 + a1 (j + 1)) x [b0 + b2 i, b0 + b2
 * (i + 1)) overlaps, weighted by the overlap.  Refused: an empty shape, 2^31 cells or more on either side, a matrix
 * that is not six finite numbers or is singular, a method / dtype pair outside these lists, for methods 3-7 a matrix
 * with a2 != 0, b1 != 0, a1 <= 0 or b2 <= 0, or with a1 > 256 or b2 > 256 (chain two calls). */
int dt_resample(const void *src, int dtype, int64_t Hs, int64_t Ws, const double *matrix, int method, int64_t nodata,
                uint64_t fill_bits, void *dst, int64_t Hd, int64_t Wd);
/* Net-new: vector rasterisation (descriptools_amd/vector.py holds the definition, the test suite's numpy reference
 * matches it bit for bit): one kind of geometry burnt onto an H x W int32 label raster, -1 where nothing burns, the
 * largest id where several parts do.  kind: 0 polygon (even-odd over all rings of an id, a cell is inside when its
 * centre is), 1 line, 2 point.  coords: float64[N][2], (x, y) in pixel-corner coordinates; parts: int64[P + 1], the
 * offsets of the parts (rings, linestrings, runs of points), non-decreasing from 0 to N; ids: int32[P] in [0, 2^30].
 * connectivity (4 or 8): how a line is drawn; all_touched (0 or 1): a polygon's rings are burnt on top of its interior
 * as connectivity-4 lines.  info4 (may be NULL): crossings of ring edges with row centre lines, the most on one row,
 * the rows sorted in global memory because they do not fit LDS, the overflow flag (always 0 here).  Refused: a kind,
 * connectivity or all_touched outside these lists, an empty shape or 2^31 cells or more, parts that do not start at 0
 * or decrease, 2^31 vertices, parts or crossings or more.  The caller vouches for finite coordinates and ids in range
 * (vector.py checks both). */
int dt_rasterize(int kind, const double *coords, const int64_t *parts, const int32_t *ids, int64_t P, int64_t H,
                 int64_t W, int connectivity, int all_touched, int32_t *label, int64_t *info4);
/* The exact work count of dt_rasterize in host arithmetic, no device needed: *total = the crossings of a polygon
 * geometry's edges with the centre lines of the H rows (8 bytes of scratch each), *largest_row = the most on one row.
 * Both 0 for lines and points. */
int dt_rasterize_count(int kind, const double *coords, const int64_t *parts, int64_t P, int64_t H, int64_t W,
                       int64_t *total, int64_t *largest_row);
/* Net-new: polygonisation, the inverse of dt_rasterize (descriptools_amd/vector.py holds the definition, the test
 * suite's reference matches it byte for byte): the regions of an H x W int32 label raster traced into rings.  A
 * negative label is background, and so is everything outside the raster.  A unit edge of the cell lattice between two
 * different labels carries one directed edge for each side that is not background, its own cell on the right of the
 * travel (x to the right, y down); at its head an edge goes on into the edge of its label that leaves there, turning
 * right where two do; every cycle is a ring.  coords: float64[cap_vertices][2], the vertices (x, y) where a ring turns,
 * from the ring's smallest (y, x) vertex on in the direction of travel; parts: int64[cap_rings + 1], the rings' offsets,
 * the rings in ascending start vertex y * (W + 1) + x, at one vertex the shell before the hole; ids: int32[cap_rings],
 * the rings' labels; shell: int32[cap_rings], the position of the outer ring of the ring's 4-connected region (its own
 * for an outer ring).  info8 (required): edges, vertices, rings, holes, rounds of the leader doubling up to and with
 * the quiet one, the overflow flags (1: edges -- never here --, 2: more vertices than cap_vertices, 4: more rings than
 * cap_rings), rounds of the rank doubling, rounds of the shell links.  A call that overflows leaves coords, parts, ids
 * and shell untouched and still counts edges, vertices and rings (holes are counted by a call that fits).  rings <=
 * vertices / 4 always.  Refused: NULL arrays, an empty shape or 2^31 cells or more, a negative capacity or one of 2^31
 * or more, a raster of 2^31 directed edges or more. */
int dt_polygonize(const int32_t *labels, int64_t H, int64_t W, int64_t cap_vertices, int64_t cap_rings, double *coords,
                  int64_t *parts, int32_t *ids, int32_t *shell, int64_t *info8);
/* The count phase of dt_polygonize alone, on the device: info2 = {directed edges, vertices}.  Sizes the call: cap_vertices
 * = info2[1], cap_rings = info2[1] / 4. */
int dt_polygonize_count(const int32_t *labels, int64_t H, int64_t W, int64_t *info2);
/* Net-new: greyscale geodesic reconstruction (Vincent 1993; descriptools_amd/morphology.py holds the definition): a
 * marker spreads under `mask` until it stops.  mask, marker and out float32, seeds and out8 uint8, H x W with fewer than
 * 2^31 cells.  A cell is valid iff its mask height is finite and > -100; every other cell is nobody's neighbour, holds
 * -100 in out and 0 in out8.  Heights are compared by the order-preserving uint32 key of their float32 bits (-0.0 below
 * +0.0).  erosion 0: reconstruction by dilation, the least R >= F0 with R(v) = min(mask(v), max(R(v), max over the
 * valid neighbours of R)), F0 = min(marker, mask) where the marker is given and none elsewhere; erosion 1: the dual
 * (min and max swapped, none above everything).  A valid cell that no marker reaches holds -100.  connectivity 4 or 8.
 * mode says what the marker is:
 *   DT_MORPH_MARKER   the raster `marker`: given on a cell iff it is not NaN and > -100 (+inf is given).
 *   DT_MORPH_SHIFT    the h-extrema transforms: float32(float64(mask) + h) for erosion, max(float32(float64(mask) - h),
 *                     the float32 next above -100) for dilation, given on every valid cell; h finite and > 0.
 *   DT_MORPH_STEP     the regional extrema: the key of the mask + 1 for erosion, - 1 for dilation.
 *   DT_MORPH_OUTLETS  the seeded fill: the mask itself on the outlet cells, none elsewhere.  seeds given: the valid
 *                     cells with seeds != 0; seeds NULL: the valid cells on the raster's edge or with an invalid
 *                     8-neighbour (the rule of dt_condition_d8).
 *   DT_MORPH_WINDOW   opening / closing by reconstruction: the window minimum (dilation) or maximum (erosion) of the
 *                     mask at `radius` in [1, 4096], as dt_filter_extremes computes it, without leaving the device.
 * Arguments a mode does not use are ignored.  Exactly one of out and out8 is given: out is the reconstruction, out8 is 1
 * where the reconstruction differs from the mask (valid cells only) and 0 elsewhere.  visit_limit: 0, or n >= 1 caps the
 * rounds of sweeps a workgroup makes over its tile per visit (tests: the outputs do not depend on it).  info4 (may be
 * NULL) = {rounds of tile visits that stored something, valid cells whose result is not F0, tile visits, 0}.  The result
 * does not depend on schedule, tiling or run: it equals a max-heap Dijkstra (widest path) on the keys bit for bit. */
#define DT_MORPH_MARKER 0
#define DT_MORPH_SHIFT 1
#define DT_MORPH_STEP 2
#define DT_MORPH_OUTLETS 3
#define DT_MORPH_WINDOW 4
int dt_morph_reconstruct(int mode, int erosion, int connectivity, const float *mask, const float *marker,
                         const uint8_t *seeds, double h, int radius, int64_t H, int64_t W, int visit_limit, float *out,
                         uint8_t *out8, int64_t *info4);
/* Net-new: harmonic interpolation on a masked raster (descriptools_amd/harmonic.py holds the definition; void filling,
 * the channel network base level and the vertical distance to channel network are built on it).  values float32, fixed
 * and domain int8, H x W with fewer than 2^31 cells; domain may be NULL (everywhere).  A cell is fixed iff fixed == 1
 * and its value is finite; a fixed cell is in the domain, a cell with fixed == 1 and a non-finite value is outside it,
 * every other cell is in the domain iff domain != 0.  The values of free cells are never read.  On every free cell v of
 * the domain with k >= 1 of its four edge neighbours (N, W, E, S) in the domain: s = the sum of those neighbours' u in
 * that order, one rounding per addition, avg = s / k in float64, r(v) = |avg - u(v)|.  out (float64) holds the fixed
 * values exactly, NaN outside the domain, and max r <= tol over those cells -- the same bits on every run; which iterate
 * passes the test depends on the schedule (tiles of 64 x 64, 4 over-relaxed red-black sweeps per visit, a pyramid by
 * 2), so equality with another solver is not part of the contract.  PRECONDITION: every free cell of the domain is joined to a fixed
 * cell by a 4-connected path through the domain; without it such cells hold an unspecified constant (the call still
 * ends).  tol is finite and > 0; max_rounds (1..4096) is the budget of rounds of tile visits per level of the pyramid.
 * info (int64[DT_HARMONIC_INFO_WORDS], may be NULL): 0 the levels, 1 the rounds on the finest level, 2 the rounds on
 * all levels, 3 the tile visits, 4 the last residual of the finest level as a double's bits, 5 whether it is <= tol,
 * 6-7 zero, 8 + l the rounds on level l (0 the finest).  The call returns DT_OK when the budget ran out on the finest
 * level: info[5] says so (a NULL info hides it). */
#define DT_HARMONIC_INFO_WORDS 40
int dt_harmonic(const float *values, const int8_t *fixed, const int8_t *domain, int64_t H, int64_t W, double tol,
                int max_rounds, double *out, int64_t *info);
/* Net-new: local-inertial 2-D flood inundation (Bates, Horritt & Fewtrell 2010; descriptools_amd/inundation.py holds
 * the scheme and its association, which is the contract: the state is a numpy restatement's bit for bit).  Rasters are
 * H x W with fewer than 2^31 cells.  z: float32 heights, NaN on a wall (nodata).  manning, rain: float32 rasters, or
 * NULL for the scalars in par.  par (double[DT_INUNDATION_PAR], host memory in both tiers): 0 px, 1 the time the call
 * starts at, 2 t_end, 3 Manning's n, 4 the rain rate (m/s), 5 alpha, 6 dt_max, 7 the dry depth, 8 the slope of the open
 * boundary, 9 the arrival depth.  boundary: 0 closed, 1 open.  The inflow table: cells int64[K] (flat indices of valid
 * cells, no duplicates, K <= DT_INUNDATION_INFLOW_MAX, may be 0), times double[T] ascending strictly, discharge
 * double[K * T] in m^3/s, finite and >= 0.  h, qx, qy (float64) are the state, read and written in place: h >= 0 on
 * valid cells (what walls hold is ignored and comes back 0), qx / qy the unit-width discharge over the east / south
 * face.  max_depth and arrival (float64, may each be NULL) are updated in place.  steps0: the steps taken before this
 * call; max_steps: the steps of this call at most, -1 for no limit; sync_every (1..1024): the guarded steps enqueued
 * between two read-backs of the control block -- the result does not depend on it.  info
 * (int64[DT_INUNDATION_INFO_WORDS], may be NULL): 0 the steps in all, 1 the steps of this call, 2 t, 3 the smallest
 * dt, 4 the last dt, 5 the largest depth (2-5: a double's bits), 6 the steps in which the limiter acted, 7 whether
 * t >= t_end. */
#define DT_INUNDATION_PAR 10
#define DT_INUNDATION_INFO_WORDS 8
#define DT_INUNDATION_INFLOW_MAX 4096
#define DT_INUNDATION_DEV_STEPS_MAX (1 << 20)
int dt_inundation(const float *z, const float *manning, const float *rain, int64_t H, int64_t W, const double *par,
                  int boundary, const int64_t *cells, const double *times, const double *discharge, int K, int T,
                  int64_t steps0, int64_t max_steps, int sync_every, double *h, double *qx, double *qy,
                  double *max_depth, double *arrival, int64_t *info);
/* Net-new: reaches (the HAND synthetic-rating-curve method).  Rasters are H x W with fewer than 2^31 cells, flat index
 * y * W + x; results are exact integers (and depth one float32 rounding), independent of order and run.
 *
 * dt_reach_catchments.  `link` as dt_stream_order writes it.  A cell c is a head when link[c] == c; R = the number of
 * heads; the id of a head is its rank among the heads in ascending flat index, heads[id] that flat index.
 *   reach (int32): the id of link[c] where link[c] >= 0 (and names a head), -100 elsewhere.
 *   catch (int32): reach[idx[c]] where 0 <= idx[c] < H * W (idx: the river index dt_flowhand writes), -100 elsewhere.
 *   heads (int64[cap]): ids >= cap are not written; entries from R on are -1.  *n_reaches = R, whatever cap is, so a
 *                  caller whose capacity was too small calls again with reach = catch = idx = NULL and cap = R.
 * reach, catch (then idx too) and heads may be NULL. */
int dt_reach_catchments(const int64_t *link, const int64_t *idx, int64_t H, int64_t W, int32_t *reach, int32_t *catch_,
                        int64_t *heads, int64_t cap, int64_t *n_reaches);
/* dt_reach_channels.  On dt_stream_order's network graph restricted to reach >= 0 (c -> d when c's code is a D8 code
 * and d is in the raster with reach[d] >= 0), for every reach r < R over its cells, all int64[R]:
 *   n_cells; n_card / n_diag: the cardinal / diagonal edges leaving its cells (the move out of the link's last cell
 *   counts for r); end: the flat index where the link's last move lands (the last cell itself when it has no edge);
 *   down: reach[end] when the last cell has an edge, else -1. */
int dt_reach_channels(const uint8_t *fdr, const int32_t *reach, int64_t H, int64_t W, int64_t R, int64_t *end,
                      int64_t *down, int64_t *n_cells, int64_t *n_card, int64_t *n_diag);
/* dt_reach_tables.  hand is float32 (hand_bytes 4) or float64 (8); slope (float32, percent) may be NULL; stages is
 * float64[K], 1 <= K <= 1024, finite, stages[0] >= 0, strictly increasing.  A cell takes part when catch[c] = r with
 * 0 <= r < R and 0 <= hand[c] <= stages[K - 1] (false for NaN and -100); its bin is the smallest k with hand[c] <=
 * stages[k]; hq = rint(hand * 2^s) and wq = rint(sqrt(1 + t * t) * 2^s), t = slope[c] / 100 where slope[c] is finite
 * and > 0, else 0 (everywhere without slope), in float64, round half to even, s = frac_bits.  For every reach r and
 * stage k, over the cells of r with bin <= k (int64[R * K], row r):
 *   cells = their number, Hq = the sum of hq, Bq = the sum of wq.
 * H * W * rint(max(stages[K - 1], 1) * 2^s) must be <= 2^52 (refused otherwise).  A bed weight whose wq exceeds
 * 2^52 / (H * W), or a catch value >= R, fails the call and the tables are not valid. */
int dt_reach_tables(const int32_t *catch_, const void *hand, int hand_bytes, const float *slope, int64_t H, int64_t W,
                    const double *stages, int K, int64_t R, int frac_bits, int64_t *cells, int64_t *Hq, int64_t *Bq);
/* dt_inundate.  depth (float32) = -100 where hand[c] == -100; else float32(stage[r] - float64(hand[c])) when
 * catch[c] = r with 0 <= r < R, stage[r] (float64[R]) is finite and 0 <= hand[c] <= stage[r]; else 0. */
int dt_inundate(const int32_t *catch_, const void *hand, int hand_bytes, const double *stage, int64_t H, int64_t W,
                int64_t R, float *depth);
/* Net-new: connected regions of a mask.  mask (and seeds) are uint8 rasters, foreground = non-zero; connectivity is 8
 * (the eight neighbours) or 4 (the cardinal ones); two foreground cells are in one region when a chain of adjacent
 * foreground cells joins them.  H * W < 2^31.
 *   label (int64): the smallest flat index y * W + x among the cells of the cell's region; -100 on background.
 *   size  (int64, may be NULL): the number of cells of the cell's region; 0 on background.
 *   keep  (uint8): 1 when the cell is foreground, seeds is NULL or one of its region's own cells has seeds != 0 (a seed
 *          on background seeds nothing), and size >= min_cells (>= 1); else 0.
 * All are functions of the inputs alone, identical in every bit from run to run.  The kernels work on tiles of
 * DT_REGIONS_TILE x DT_REGIONS_TILE cells.  A connectivity other than 4 or 8 and min_cells < 1 are DT_EINVAL. */
#define DT_REGIONS_TILE 64
int dt_regions_label(const uint8_t *mask, int64_t H, int64_t W, int connectivity, int64_t *label, int64_t *size);
int dt_regions_select(const uint8_t *mask, const uint8_t *seeds, int64_t H, int64_t W, int connectivity,
                      int64_t min_cells, uint8_t *keep);
/* dt_inundate kept to the wet regions that touch the channel.  A cell is wet exactly when dt_inundate gives it the value
 * of its third clause (catch in range, stage finite, 0 <= hand <= stage: a cell with hand == stage is wet at depth 0);
 * the seeds are the wet cells with river == 1.  depth = dt_inundate's value, except 0 on a wet cell whose wet region
 * (under `connectivity`) holds no seed; cells with hand == -100 keep -100. */
int dt_inundate_connected(const int32_t *catch_, const void *hand, int hand_bytes, const double *stage,
                          const int8_t *river, int64_t H, int64_t W, int64_t R, int connectivity, float *depth);
/* Net-new: zonal statistics -- label compaction, per-zone integer tables, per-zone histograms / cross-tabulation and
 * painting a table back onto its zones (descriptools_amd/zonal.py holds the definitions in full).  Rasters are H x W,
 * row-major, H * W < 2^31.
 * dt_zonal_compact.  labels is int32 (label_bytes 4) or int64 (8); a label is valid when 0 <= l < limit, 1 <= limit <=
 * 2^31 - 1.  *n_zones = the number of distinct valid labels; labels_of[r] (int64, the first `cap` of them; may be NULL
 * with cap 0) = the r-th smallest; zones (int32, may be NULL) = the rank of the cell's label, -100 where it is not valid.
 * dt_zonal_tables.  zones is int32: a cell has a zone when 0 <= z < n_zones, negative values have none, z >= n_zones
 * fails the call.  values is float32 (value_bytes 4) or float64 (8).  A cell takes part when it has a zone, its value is
 * finite and (with has_nodata) not equal to nodata as float64; -0.0 counts as +0.0.  q = rint((float64(v) - origin) *
 * 2^frac_bits), round to even, 0 <= frac_bits <= 24, origin finite; |q| <= 2^31 - 1, a value beyond fails the call.
 * Per zone, over its participating cells, each table [n_zones] and NULL when not wanted (at least one is): count =
 * their number; s1 = sum q (int64); s2_lo = sum (q^2 mod 2^32) and s2_hi = sum (q^2 div 2^32) (uint64, wanted
 * together: sum q^2 = s2_hi 2^32 + s2_lo); vmin / vmax = the smallest / largest value in the dtype of values, NaN on
 * a zone without a participating cell.
 * dt_zonal_counts.  counts is int64[n_zones][K], 1 <= K <= 1024, n_zones * K * 8 <= 2^31.  value_bytes 4 / 8: values
 * is a float32 / float64 raster and edges float64[K + 1], finite and strictly increasing; a participating cell (as
 * above) counts in bin k when edges[k] <= v < edges[k + 1], the last bin also takes v == edges[K] (compared as
 * float64).  value_bytes 0: values is a second int32 zone raster and the column is its cell, 0 <= b < K (edges unused;
 * negative b counts nowhere, b >= K fails the call like z >= n_zones).
 * dt_zonal_paint.  out[c] = table[zones[c]] where 0 <= zones[c] < n_table, else *fill; table, fill and out are words
 * of elem_bytes (4 or 8) bytes, moved as they are. */
int dt_zonal_compact(const void *labels, int label_bytes, int64_t H, int64_t W, int64_t limit, int32_t *zones,
                     int64_t *labels_of, int64_t cap, int64_t *n_zones);
int dt_zonal_tables(const int32_t *zones, const void *values, int value_bytes, int64_t H, int64_t W, int64_t n_zones,
                    double origin, int frac_bits, int has_nodata, double nodata, int64_t *count, int64_t *s1,
                    uint64_t *s2_lo, uint64_t *s2_hi, void *vmin, void *vmax);
int dt_zonal_counts(const int32_t *zones, const void *values, int value_bytes, int64_t H, int64_t W, int64_t n_zones,
                    const double *edges, int K, int has_nodata, double nodata, int64_t *counts);
int dt_zonal_paint(const void *table, int elem_bytes, int64_t n_table, const int32_t *zones, int64_t H, int64_t W,
                   const void *fill, void *out);

/* flowhand.flow_distance_index_cpu + flow_distance_index_gpu (flowhand.py:476-846, untiled
 * call: out = 0, row_start = col_start = 0, matrix_columns = W) and flowhand.hand_calculator
 * (flowhand.py:414-442).  `dem`/`hand` may both be NULL to skip HAND. */
int dt_flowhand(const float *dem, const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W,
                double px, float *fdist, int64_t *idx, float *hand);

/* flowhand.hand_calculator alone (flowhand.py:414-442): dem - dem[idx], negatives -> 0. */
int dt_hand_f32(const float *dem, const int64_t *idx, int64_t N, float *hand);

/* topoindexes.topographic_index_cpu + both kernels (topoindexes.py:170-295); slope in radians. */
int dt_twi(const int64_t *fac, const float *slope_rad, int64_t N, double px, double n_top,
           float *ti, float *mti);

/* gfi.river_accumulation (gfi.py:119-147): out[i] = fac[idx[i]] where idx != -100 else fac[0]. */
int dt_river_accumulation(const int64_t *fac, const int64_t *idx, int64_t N, int64_t *out);

/* gfi.geomorphic_flood_index_cpu/_gpu (gfi.py:210-294; zero_guard = 0) and gfi.ln_hl_H_cpu/_gpu
 * (gfi.py:349-440; zero_guard = 1: area == 0 -> 1) on an explicit per-cell area raster. */
int dt_gfi_area(const float *hand, const int64_t *area, int64_t N, double n_gfi, double scale_factor,
                double size, int zero_guard, float *out);

/* gfi.river_accumulation + geomorphic_flood_index_cpu/_gpu (gfi.py:119-147, 210-294). */
int dt_gfi(const float *hand, const int64_t *fac, const int64_t *idx, int64_t N, double n_gfi,
           double scale_factor, double size, float *gfi);

/* gfi.ln_hl_H_cpu/_gpu (gfi.py:349-440). */
int dt_lnhlh(const float *hand, const int64_t *fac, int64_t N, double n_gfi, double scale_factor,
             double size, float *out);

/* downslope.downslope_cpu + downslope_gpu + the -50 repair of downslope_sequential_jit
 * (downslope.py:379-532, 161-314), untiled.
 * raw != 0 reproduces downslope_cpu alone: failed walks are left as the marker -50. */
int dt_downslope(const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                 double elevation_difference, int raw, float *out);

/* ---- heights in float64: a DEM (or HAND) that float32 cannot hold --------------------------------------------
 * The reference takes height differences in the raster's OWN dtype (slope.py:244-258 under Numba typing,
 * flowhand.py:436-438 `dem - dem[indices]`, downslope.py:468) and adds 0.01 to the HAND it is given in float64
 * (gfi.py:289-294, :429-440).  The float32 entry points above are that arithmetic exactly when every height is a
 * float32 value; for the rest -- a genuinely float64 DEM, integer heights beyond 2^24 (exact in float64 up to 2^53)
 * -- these take the heights as float64 and evaluate the literal expressions (one thread per cell on global memory:
 * the capability, not the tuned path).  descriptools_amd/_lib.py picks the tier per raster. */
/* slope.py:152-259 */
int dt_slope_f64(const double *dem, int64_t H, int64_t W, double px, float *slope);
/* flowhand.hand_calculator, flowhand.py:414-442 (flow distance / river index do not read heights: dt_flowhand with
 * dem = hand = NULL) */
int dt_hand_f64(const double *dem, const int64_t *idx, int64_t N, double *hand);
/* downslope.py:379-532 + the repair :161-314; raw as in dt_downslope */
int dt_downslope_f64(const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                     double elevation_difference, int raw, float *out);
/* gfi.py:119-147 + :210-294 (own_area = 0: area of the river cell idx points at, no zero guard; idx required),
 * gfi.py:349-440 (own_area = 1: the cell's own accumulation, 0 -> 1; idx ignored) and geomorphic_flood_index_cpu on
 * an explicit per-cell area raster passed as `fac` (own_area = 2: no zero guard), on a float64 HAND */
int dt_gfi_f64h(const double *hand, const int64_t *fac, const int64_t *idx, int64_t N, double n_gfi,
                double scale_factor, double size, int own_area, float *out);

/* D8 (flowdir.d8's definition, N1) with the differences taken in float64: codes of the first strict maximum of
 * (z - z_nb) / d in scan order NW, N, NE, W, E, SW, S, SE, the raster-border rule, nodata z <= -100; slope (may be
 * NULL) as dt_slope_f64 */
int dt_d8_f64(const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *slope);

/* evaluation.binary_map + avaliacao for `nth` thresholds in one pass (evaluation.py:90-171):
 * counts4[t*4 + v] = #cells with binary(desc, th[t]) + remapped(flood) == v, v = 0..3.
 * Cells equal to `nodata_value` (the caller passes desc[0,0], evaluation.py:111) or NaN
 * classify 0; flood is remapped 1 -> 2, -100 -> 0 on the fly (evaluation.py:149-150). */
int dt_confusion_multi(const double *desc, const int8_t *flood, int64_t N, double nodata_value,
                       const double *th, int nth, int under, int64_t *counts4);

/* The same counts at every threshold of a sorted table from ONE pass: the histogram of the bin at which
 * a cell's classification changes.  th: K thresholds, 1 <= K <= 65535, ascending by `<=` (equal neighbours, -0.0 beside
 * +0.0 and +-inf are fine), none NaN -- checked here.  hist = int64[2 (K + 1) + 1]:
 *   under != 0: a cell's bin j = #{k : th[k] <  v}, it floods at every k >= j; nodata / NaN cells get j = K
 *   under == 0:             j = #{k : th[k] <= v}, it floods at every k <  j; nodata / NaN cells get j = 0
 *   hist[j] counts the cells whose remapped benchmark value is 0, hist[K + 1 + j] those where it is 2, hist[2K + 2] the
 *   cells with any other benchmark value (which dt_confusion_multi counts by their sum; here they are only reported).
 * Cell semantics (nodata_value, NaN, the remap of flood) as dt_confusion_multi.  With c0 / c2 the inclusive prefix sums
 * of the two histograms and T0 / T2 their totals, counts4[k] = {T0 - f0, f0, T2 - f2, f2} where f = c[k] (under) or
 * T - c[k] (otherwise). */
int dt_threshold_hist(const double *desc, const int8_t *flood, int64_t N, double nodata_value,
                      const double *th, int K, int under, int64_t *hist);

/* evaluation.minMaxScale (evaluation.py:5-9): out = NaN where x == nodata or x is NaN, else (x - mn) / (mx - mn),
 * in float32 for a float32 raster (is_f32) and float64 otherwise -- numpy's arithmetic for those dtypes. */
int dt_minmax_scale(const void *x, int is_f32, int64_t N, double mn, double mx, double nodata, void *out);
/* the same with the denominator den = mx - mn given, in the raster's own float type (cell_bytes 2 / 4 / 8: float16 /
 * float32 / float64 in and out): numpy subtracts the two scalars from each other before they meet the raster, so the
 * denominator is not T(mx) - T(mn) in general.  A float16 raster is scaled as numpy scales it: the difference and the
 * quotient are each rounded to float16. */
int dt_minmax_scale_den(const void *x, int cell_bytes, int64_t N, double mn, double den, double nodata, void *out);
/* evaluation.binary_map (evaluation.py:90-123): binary = 1 where desc <= threshold ('under') or >= threshold,
 * 0 elsewhere, where desc is NaN and where desc == nodata_value (the caller passes desc[0, 0], :111). */
int dt_binary_map(const void *desc, int is_f32, int64_t N, double nodata_value, double threshold, int under,
                  uint8_t *binary);
/* evaluation.avaliacao (evaluation.py:126-171): flood is remapped IN PLACE (1 -> 2, -100 -> 0, :149-150),
 * klass (may be NULL) = binary + flood, counts4[v] = cells of class v = 0..3. */
int dt_avaliacao(const int32_t *binary, int8_t *flood, int64_t N, int32_t *klass, int64_t *counts4);

/* Synthetic "tilted integer fBm" DEM window, bit-identical to the oracle's. */
int dt_synth_dem(uint32_t seed, int64_t Hg, int64_t Wg, int64_t y0, int64_t x0, int64_t h,
                 int64_t w, int nodata_pct, float *out);

/* ---- device-pointer tier (resident chain; all asynchronous on ctx's stream) ------------- */
/* plain device memory for callers without their own allocator (numpy-only hosts) */
int dt_dev_malloc(dt_ctx *ctx, int64_t bytes, void **out);
int dt_dev_free(dt_ctx *ctx, void *p);
int dt_dev_h2d(dt_ctx *ctx, void *dst_dev, const void *src_host, int64_t bytes); /* synchronous */
int dt_dev_d2h(dt_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes); /* synchronous */
/* enqueue only: dt_ctx_sync before the host reads dst_host (page-locked memory: dt_host_alloc) */
int dt_dev_d2h_async(dt_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes);
int dt_dev_synth_dem(dt_ctx *ctx, uint32_t seed, int64_t Hg, int64_t Wg, int64_t y0, int64_t x0,
                     int64_t h, int64_t w, int nodata_pct, float *out);
/* slope (may be NULL), fdr (may be NULL), slope_rad (may be NULL): fused 3x3 stencil.
 * slope_rad = float32(atan(slope/100)), -100 where dem == -100 (Example/example.py:63-64). */
int dt_dev_slope_d8(dt_ctx *ctx, const float *dem, int64_t H, int64_t W, double px, float *slope,
                    uint8_t *fdr, float *slope_rad);
/* The north_star's fused "slope+TWI" stencil: one pass over dem (+ acc32) producing slope %
 * (may be NULL), slope in radians (may be NULL), TI and MTI -- the slope raster never has to be
 * re-read (topoindexes.py:234-295 on top of slope.py:210-259). */
int dt_dev_slope_twi(dt_ctx *ctx, const float *dem, const int32_t *acc32, int64_t H, int64_t W,
                     double px, double n_top, float *slope, float *slope_rad, float *ti, float *mti);
/* dt_d8_conditioned_f32 on device rasters; synchronous (the fixed-point iterations read a flag back). */
int dt_dev_condition_d8(dt_ctx *ctx, const float *dem, int64_t H, int64_t W, double px, float *filled, uint8_t *fdr,
                        int32_t *info3);
/* The same without any host synchronisation (the resident chain's form, chain.Chain(condition=True)): `rounds`
 * fill rounds and `rounds` flat rounds are enqueued (1..500), a round that follows a quiet one returns at once, and
 * DT_STATUS_NOT_CONVERGED is raised on the context (dt_ctx_status) when the budget did not reach the fixed point. */
int dt_dev_condition_d8_async(dt_ctx *ctx, const float *dem, int64_t H, int64_t W, double px, float *filled,
                              uint8_t *fdr, int rounds);
/* The float64 forms of the two: dt_d8_conditioned_f32's definition with the heights compared in float64; dem and
 * filled are H x W double rasters on the device, every other argument as in the float32 form (the async form takes
 * 1..500 rounds and raises DT_STATUS_NOT_CONVERGED when they run out).  The resident float64 chain takes such codes
 * as external ones: Chain(heights="float64", external_fdr=True), dt_dev_condition_d8_f64_async into its fdr raster
 * on its context, then run(). */
int dt_dev_condition_d8_f64(dt_ctx *ctx, const double *dem, int64_t H, int64_t W, double px, double *filled,
                            uint8_t *fdr, int32_t *info3);
int dt_dev_condition_d8_f64_async(dt_ctx *ctx, const double *dem, int64_t H, int64_t W, double px, double *filled,
                                  uint8_t *fdr, int rounds);
/* acc32: int32 accumulation (H*W < 2^31); dem may be NULL. */
int dt_dev_flowacc(dt_ctx *ctx, const uint8_t *fdr, const float *dem, int64_t H, int64_t W,
                   int32_t *acc32);
/* dt_flowacc_weighted on device rasters (H * W < 2^31, dem may be NULL).  A weight outside the contract raises
 * DT_STATUS_BAD_WEIGHT on the context (dt_ctx_status) and counts as 0. */
int dt_dev_flowacc_weighted(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const double *w, int64_t H, int64_t W,
                            int frac_bits, double *acc);
/* dt_stream_order on device rasters, on the context's stream: it does not synchronise (except on rasters of 2^31
 * cells or more, where it reads the network's size back to refuse 2^31 network cells).  shreve and link may be NULL. */
int dt_dev_stream_order(dt_ctx *ctx, const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W, int8_t *strahler,
                        int64_t *shreve, int64_t *link);
/* dt_drainage and dt_upslope_length on device rasters, on the context's stream: they do not synchronise.  dem and
 * pour may be NULL, so may any output (label requires pour). */
int dt_dev_drainage(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const int64_t *pour, int64_t H, int64_t W,
                    double px, int64_t *target, double *length, int64_t *label);
int dt_dev_upslope_length(dt_ctx *ctx, const uint8_t *fdr, const float *dem, int64_t H, int64_t W, double px,
                          double *length);
/* dt_flowpath_upslope and dt_flowpath_downstream on device rasters (rows x cols), on the context's stream: they do
 * not synchronise and take their scratch from the context.  dem and stop may be NULL; a NULL output is not computed.
 * dt_dev_carve_blend: carved = max(lowest, filled - float32(max_cut)) in float32, the dem value on nodata cells -- the
 * last step of dt_carve for a finite max_cut >= 0 (anything else: DT_EINVAL); carved may alias lowest.  On a resident
 * chain: lowest = dt_dev_flowpath_upslope(fdr, dem, dem, kind 1) on the chain's own codes. */
int dt_dev_flowpath_upslope(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const float *values, int64_t rows,
                            int64_t cols, int kind, float *value, int64_t *where);
int dt_dev_flowpath_downstream(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const float *values,
                               const uint8_t *stop, int64_t rows, int64_t cols, int kind, float *value,
                               int64_t *where);
int dt_dev_carve_blend(dt_ctx *ctx, const float *dem, const float *filled, const float *lowest, int64_t rows,
                       int64_t cols, double max_cut, float *carved);
/* dt_flowpath_downstream_sum and dt_flowpath_upslope_longest on device rasters (rows x cols), on the context's stream:
 * they do not synchronise and take their scratch from the context (32 B per perimeter node of the 64 x 64 tiles, and
 * 8 B per cell more for the longest fold).  dem and stop may be NULL; out NULL: nothing runs.  A weight outside the
 * contract counts as 0 and raises DT_STATUS_BAD_WEIGHT (dt_ctx_status). */
int dt_dev_flowpath_downstream_sum(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const double *weights,
                                   const uint8_t *stop, int64_t rows, int64_t cols, int frac_bits, double *out);
int dt_dev_flowpath_upslope_longest(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const double *weights,
                                    int64_t rows, int64_t cols, int frac_bits, double *out);
/* dt_dinf_direction and dt_dinf_accumulate on device rasters, on the context's stream: neither synchronises.  fdr,
 * slope and w may be NULL.  dt_dev_dinf_accumulate enqueues round 0 (from the cells without donors) and rounds - 1
 * rounds that drain the queue of cells handed on (1 <= rounds <= 4096; a round that finds the queue empty returns at
 * once), then writes acc; when queued work is left it raises DT_STATUS_NOT_CONVERGED (dt_ctx_status) and the cells
 * not reached hold -100.  A start (a source, a queued cell) completes at most 128 cells in a round before it hands
 * on, so a raster needs at least its longest flow path / 128 rounds: dt_dev_dinf_accumulate_info says how many found
 * work.  A call with -4096 <= rounds <= -1 continues that accumulation with -rounds further rounds and writes acc
 * again; it must name the same angle raster, weight raster, shape and frac_bits (DT_EINVAL otherwise, and when
 * another call has used the context's scratch since; the rasters' contents must not have changed, which is not
 * checked).  An angle outside the contract raises DT_STATUS_BAD_ANGLE and counts as -1, a bad weight
 * DT_STATUS_BAD_WEIGHT and 0. */
int dt_dev_dinf_direction(dt_ctx *ctx, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                          float *angle, float *slope);
int dt_dev_dinf_accumulate(dt_ctx *ctx, const float *angle, const double *w, int64_t H, int64_t W, int frac_bits,
                           int rounds, double *acc);
/* dt_dinf_accumulate's info4 for the accumulation last enqueued on this context (synchronises): what a caller sizes
 * its budget of rounds with.  DT_EINVAL when another call has used the context's scratch since. */
int dt_dev_dinf_accumulate_info(dt_ctx *ctx, int64_t *info4);
/* dt_mfd_shares and dt_mfd_accumulate on device rasters (rows x cols = H x W), on the context's stream: neither
 * synchronises.  fdr and w may be NULL; the share raster is 16-byte aligned.  dt_dev_mfd_accumulate takes its budget of
 * rounds as
 * dt_dev_dinf_accumulate does: round 0 and rounds - 1 queue rounds (1 <= rounds <= 4096), DT_STATUS_NOT_CONVERGED when
 * queued work is left, and -4096 <= rounds <= -1 continues with -rounds further rounds on the same share raster,
 * weight raster, shape and frac_bits (DT_EINVAL otherwise, and when another call has used the context's scratch
 * since).  A share word outside the contract raises DT_STATUS_BAD_SHARES and counts as no receiver, a bad weight
 * DT_STATUS_BAD_WEIGHT and 0.  dt_dev_mfd_accumulate_info: dt_mfd_accumulate's info4 for the accumulation last enqueued
 * on this context (synchronises). */
int dt_dev_mfd_shares(dt_ctx *ctx, const float *dem, const uint8_t *fdr, int64_t rows, int64_t cols, double exponent,
                      int contour, uint16_t *shares);
int dt_dev_mfd_accumulate(dt_ctx *ctx, const uint16_t *shares, const double *w, int64_t rows, int64_t cols,
                          int frac_bits, int rounds, double *acc);
int dt_dev_mfd_accumulate_info(dt_ctx *ctx, int64_t *info4);
/* dt_mfd_route and dt_dinf_route on device rasters, on the context's stream: neither synchronises.  They are the
 * accumulations with a transfer function, on the accumulations' own state: the budget of rounds means what it means to
 * dt_dev_mfd_accumulate / dt_dev_dinf_accumulate (1 <= rounds <= 4096 starts, DT_STATUS_NOT_CONVERGED when queued work is
 * left, -4096 <= rounds <= -1 continues and must name the same flow raster, weight raster, parameter raster, mode,
 * shape and frac_bits), and dt_dev_mfd_accumulate_info / dt_dev_dinf_accumulate_info report a routing run as they
 * report an accumulation.  w may be NULL; each output may be NULL.  DT_EINVAL for a mode that is not one of DT_ROUTE_*,
 * and on a raster with cells for a NULL param, for four NULL outputs, for an output that is one of the inputs and for
 * two outputs that are the same raster.  A parameter outside its contract raises DT_STATUS_BAD_PARAM and acts as the
 * identity; angles, share words and weights as in the accumulations. */
int dt_dev_mfd_route(dt_ctx *ctx, const uint16_t *shares, const double *w, const double *param, int64_t rows,
                     int64_t cols, int frac_bits, int mode, int rounds, double *inflow, double *load,
                     double *outflow, double *retained);
int dt_dev_dinf_route(dt_ctx *ctx, const float *angle, const double *w, const double *param, int64_t rows,
                      int64_t cols, int frac_bits, int mode, int rounds, double *inflow, double *load,
                      double *outflow, double *retained);
/* dt_terrain on device rasters (rows x cols = H x W), on the context's stream: one launch, no synchronisation, and
 * none of the context's scratch (a two-phase op started on the context stays continuable).  Output pointers may be
 * NULL, not all of them; a radius outside [1, 32] and a sun vector that is not finite are DT_EINVAL; H * W == 0 is
 * DT_OK.  16-byte aligned rasters with cols % 4 == 0 are read and written 16 bytes at a time at radius 1. */
int dt_dev_terrain(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, double px, int radius, double sx,
                   double sy, double sz, float *gradient, float *aspect, float *profile, float *plan,
                   float *tangential, float *mean, float *laplacian, float *hillshade);
/* dt_horizon on device rasters (rows x cols = H x W), on the context's stream: one launch, no device allocation, no
 * copy (the 2 x 64 reciprocal table travels as a kernel argument), no synchronisation, and none of the context's
 * scratch, so it may stand anywhere on a context's stream.  Checked in this order: the context, shape and px, radius /
 * skip / flat_tan (DT_EINVAL outside [1, 64], [0, radius - 1], finite and >= 0); H * W == 0 is DT_OK; then at least
 * one output, a non-NULL dem. */
int dt_dev_horizon(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, double px, int radius, int skip,
                   double flat_tan, uint8_t *landform, uint16_t *pattern, float *positive, float *negative,
                   float *sky_view);
/* dt_focal on device rasters (rows x cols = H x W; radii in host memory, it travels as a kernel argument), on the
 * context's stream: four launches whatever the rasters hold, no synchronisation.  The tables (22.5 bytes per cell: a
 * uint32 and two uint64 planes, and the column sums of every band of 8 rows) are the context's scratch; nothing is kept
 * between calls.  Checked in this order: the context and shape, the radius table, frac_bits, origin, the outputs that
 * go with n_radii, at least one output; rows * cols == 0 is DT_OK; then a non-NULL dem.  A valid height outside the
 * contract raises DT_STATUS_BAD_HEIGHT on the context (dt_ctx_status) and counts as q = 0: the rasters of that call
 * are not valid. */
int dt_dev_focal(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, double origin, int frac_bits,
                 const int32_t *radii, int n_radii, int32_t *count, float *mean, float *std, float *tpi, float *dev,
                 uint16_t *scale);
/* dt_filter_extremes, dt_filter_rank and dt_filter_denoise on device rasters (rows x cols = H x W; table in host
 * memory, it travels as a kernel argument), on the context's stream, no synchronisation.  dt_dev_filter_extremes: three
 * launches per window pass (one pass per minimum and maximum, one more per opening and closing), its running extremes
 * and the intermediate rasters (24 bytes per cell) in the context's scratch.  dt_dev_filter_rank: one launch, no
 * scratch.  dt_dev_filter_denoise: 2 + iterations launches, the normals, the smoothed normals and one height buffer
 * (28 bytes per cell) in the context's scratch.  Nothing is kept between calls.  Checked in this order: the context and
 * shape (and px), the op's own arguments; rows * cols == 0 is DT_OK; then the outputs and a non-NULL dem. */
int dt_dev_filter_extremes(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, int radius, float *minimum,
                           float *maximum, float *range, float *opening, float *closing);
int dt_dev_filter_rank(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, int radius, const uint16_t *table,
                       int n_table, float *out);
int dt_dev_filter_denoise(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, double px, int radius,
                          double cos_threshold, int iterations, double max_change, float *out);
/* dt_mrvbf, dt_percentile and dt_coarsen on device rasters (rows x cols = H x W; p and g6 in host memory, they travel
 * as kernel arguments), on the context's stream, no synchronisation.  dt_dev_mrvbf keeps the pyramid of the levels >= 3
 * (float32 height, slope, lower and higher percentile: 16 bytes per coarse cell, about 2 bytes per base cell over all
 * levels) in the context's scratch: two launches per level >= 3 build it, one launch at base resolution writes the
 * outputs; nothing is kept between calls.  dt_dev_percentile and dt_dev_coarsen are one launch each and take no
 * scratch; dem3 and slope3 hold ceil(rows / 3) x ceil(cols / 3) cells.  Checked in this order: the context and shape
 * (and px), the op's own arguments; rows * cols == 0 is DT_OK; then the outputs and a non-NULL dem. */
int dt_dev_mrvbf(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, double px, double slope_threshold,
                 int levels, double pctl_valley, double pctl_ridge, const double *p, float *mrvbf, float *mrrtf);
int dt_dev_percentile(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, int radius, float *lower,
                      float *higher);
int dt_dev_coarsen(dt_ctx *ctx, const float *dem, int64_t rows, int64_t cols, double px, const double *g6,
                   float *dem3, float *slope3);
/* The reach calls on device rasters, on the context's stream: none synchronises.  idx is int32 (idx_bytes 4, the
 * resident chain's raster) or int64 (8); n_reaches (may be NULL) is one int64 on the device; heads entries from R on
 * are left as they were.  dt_dev_reach_tables takes `stages` from the host (they travel as kernel arguments) and the
 * tables on the device; a bed weight over the bound raises DT_STATUS_BAD_WEIGHT and counts as 0, a catch value >= R
 * raises DT_STATUS_REACH_RANGE and is left out (dt_ctx_status).  stage is float64[R] on the device. */
int dt_dev_reach_catchments(dt_ctx *ctx, const int64_t *link, const void *idx, int idx_bytes, int64_t H, int64_t W,
                            int32_t *reach, int32_t *catch_, int64_t *heads, int64_t cap, int64_t *n_reaches);
int dt_dev_reach_channels(dt_ctx *ctx, const uint8_t *fdr, const int32_t *reach, int64_t H, int64_t W, int64_t R,
                          int64_t *end, int64_t *down, int64_t *n_cells, int64_t *n_card, int64_t *n_diag);
int dt_dev_reach_tables(dt_ctx *ctx, const int32_t *catch_, const void *hand, int hand_bytes, const float *slope,
                        int64_t H, int64_t W, const double *stages, int K, int64_t R, int frac_bits, int64_t *cells,
                        int64_t *Hq, int64_t *Bq);
int dt_dev_inundate(dt_ctx *ctx, const int32_t *catch_, const void *hand, int hand_bytes, const double *stage,
                    int64_t H, int64_t W, int64_t R, float *depth);
/* The zonal calls on device rasters (rows x cols = H x W), on the context's stream: none synchronises.  n_zones of
 * dt_dev_zonal_compact (may be NULL) is one int64 on the device; labels_of entries from n_zones on are left as they
 * were; its workspace (the bitmap, the word ranks and the block counts: limit / 4 bytes) is the context's scratch.
 * The tables are on the device; the entry zeroes them.  A value outside the bound of frac_bits raises
 * DT_STATUS_BAD_HEIGHT, a zone id (or column) out of range DT_STATUS_ZONE_RANGE; either cell is left out
 * (dt_ctx_status).  edges and fill are read on the host (they travel as kernel arguments). */
int dt_dev_zonal_compact(dt_ctx *ctx, const void *labels, int label_bytes, int64_t rows, int64_t cols, int64_t limit,
                         int32_t *zones, int64_t *labels_of, int64_t cap, int64_t *n_zones);
int dt_dev_zonal_tables(dt_ctx *ctx, const int32_t *zones, const void *values, int value_bytes, int64_t rows,
                        int64_t cols, int64_t n_zones, double origin, int frac_bits, int has_nodata, double nodata,
                        int64_t *count, int64_t *s1, uint64_t *s2_lo, uint64_t *s2_hi, void *vmin, void *vmax);
int dt_dev_zonal_counts(dt_ctx *ctx, const int32_t *zones, const void *values, int value_bytes, int64_t rows,
                        int64_t cols, int64_t n_zones, const double *edges, int K, int has_nodata, double nodata,
                        int64_t *counts);
int dt_dev_zonal_paint(dt_ctx *ctx, const void *table, int elem_bytes, int64_t n_table, const int32_t *zones,
                       int64_t rows, int64_t cols, const void *fill, void *out);
/* dt_cost_distance on device rasters (rows x cols = H x W), on the context's stream, without a host synchronisation:
 * the initialisation, `rounds` (1..4096) rounds of tile visits -- a round that follows a quiet one returns at once --
 * then the back-links, the fills and the allocation.  When the last round still lowered something the budget was too
 * small: DT_STATUS_NOT_CONVERGED is raised on the context (dt_ctx_status) and the three rasters are not valid; call
 * again with a larger budget.  DT_STATUS_NO_BACKLINK says that a reached cell has no back-link.  The
 * workspace (4 bytes per cell when indices is given, a few bytes per tile of 64 x 64) is the context's scratch; nothing
 * is kept between calls.  indices and backlink may be NULL. */
int dt_dev_cost_distance(dt_ctx *ctx, const float *friction, const int8_t *sources, int64_t rows, int64_t cols,
                         double px, int connectivity, int visit_limit, int rounds, double *cost, int64_t *indices,
                         uint8_t *backlink);
/* The three stages of dt_wetness_saga on device rasters (rows x cols = H x W), on the context's stream, without a host
 * synchronisation.  dt_dev_wetness_modified_area: the initialisation, `rounds` (1..4096) rounds of tile visits -- a
 * round that follows a quiet one returns at once -- then the fills.  When the last round still raised something the
 * budget was too small: DT_STATUS_NOT_CONVERGED is raised on the context (dt_ctx_status) and `modified` is not valid;
 * call again with a larger budget.  Its workspace (a few bytes per tile of 64 x 64) is the context's scratch; nothing is
 * kept between calls.  dt_dev_wetness_index takes any modified area and -100 where it is not in (0, +inf), the slope is
 * NaN or not in [0, pi/2), or b >= pi/2. */
int dt_dev_wetness_suction(dt_ctx *ctx, const float *slope, int64_t rows, int64_t cols, double t, double slope_weight,
                           double slope_offset, double slope_min, float *suction);
int dt_dev_wetness_modified_area(dt_ctx *ctx, const double *area, const float *suction, int64_t rows, int64_t cols,
                                 int visit_limit, int rounds, double *modified);
int dt_dev_wetness_index(dt_ctx *ctx, const double *modified, const float *slope, int64_t rows, int64_t cols,
                         double slope_offset, double slope_min, float *swi);
/* dt_resample on device rasters, on the context's stream, without a host synchronisation: one kernel launch, the
 * matrix (a host pointer, read before the call returns) travels in its arguments, no scratch and no allocation.  dst
 * must not overlap src. */
int dt_dev_resample(dt_ctx *ctx, const void *src, int dtype, int64_t Hs, int64_t Ws, const double *matrix, int method,
                    int64_t nodata, uint64_t fill_bits, void *dst, int64_t Hd, int64_t Wd);
/* dt_rasterize on device arrays (N = parts[P] vertices), on the context's stream, without a host synchronisation.
 * The raster is rows x cols = H x W.  Scratch is the context's: 4 H + 8 capacity bytes.  capacity: the crossing slots the caller vouches for
 * (dt_rasterize_count gives the exact number); the kernels never write past it, and a geometry with more crossings
 * leaves label all -1 and says so in info.  info: int64[4] on the device, required: crossings found, the most on one
 * row, rows sorted in global memory, overflow flag. */
int dt_dev_rasterize(dt_ctx *ctx, int kind, const double *coords, const int64_t *parts, const int32_t *ids, int64_t P,
                     int64_t N, int64_t rows, int64_t cols, int connectivity, int all_touched, int64_t capacity,
                     int32_t *label, int64_t *info);
/* dt_dev_rasterize between events, followed by a synchronisation: phase_ms (host, double[7]) = the device time of the
 * clear, count, scan, emit, sort, fill and line / point phases.  A measuring tool's entry. */
int dt_dev_rasterize_timed(dt_ctx *ctx, int kind, const double *coords, const int64_t *parts, const int32_t *ids,
                           int64_t P, int64_t N, int64_t rows, int64_t cols, int connectivity, int all_touched,
                           int64_t capacity, int32_t *label, int64_t *info, double *phase_ms);
/* dt_polygonize on device arrays, on the context's stream, without a host synchronisation: a fixed list of launches
 * whatever the raster holds -- each of the two pointer doublings issues ceil(log2 cap_edges) + 1 rounds, the shell links
 * ceil(log2 cap_rings) + 1, and a round behind a quiet one returns at once.  The raster is rows x cols = H x W.
 * cap_edges, cap_vertices, cap_rings: the directed edges, vertices and rings the caller vouches for (each in [0, 2^31);
 * edges <= 4 H W, vertices <= edges, rings <= vertices / 4); no kernel writes at or past one, and a raster that needs
 * more leaves coords (float64[cap_vertices][2]), parts (int64[cap_rings + 1]), ids and shell (int32[cap_rings])
 * untouched and says so in info.  info: int64[8] on the device, required, as dt_polygonize's info8; when the edges
 * overflow, rings and holes read -1.  Scratch is the context's: 768 bytes of round flags, 8 bytes per 1024 lattice
 * vertices (H (W + 1)) of block sums, 4 bytes per cell, and 20 bytes per edge of cap_edges (two 8-byte doubling words
 * and the 4-byte leader), each array rounded up to 256; nothing is kept between calls. */
int dt_dev_polygonize(dt_ctx *ctx, const int32_t *labels, int64_t rows, int64_t cols, int64_t cap_edges,
                      int64_t cap_vertices, int64_t cap_rings, double *coords, int64_t *parts, int32_t *ids,
                      int32_t *shell, int64_t *info);
/* dt_dev_polygonize between events, followed by a synchronisation: phase_ms (host, double[7]) = the device time of the
 * count, link, leaders, ranks, rings, emit and shells phases.  A measuring tool's entry. */
int dt_dev_polygonize_timed(dt_ctx *ctx, const int32_t *labels, int64_t rows, int64_t cols, int64_t cap_edges,
                            int64_t cap_vertices, int64_t cap_rings, double *coords, int64_t *parts, int32_t *ids,
                            int32_t *shell, int64_t *info, double *phase_ms);
/* dt_morph_reconstruct on device rasters (rows x cols = H x W), on the context's stream, without a host
 * synchronisation: the start keys, `rounds` (1..4096) rounds of tile visits -- a round that follows a quiet one returns
 * at once -- then the output.  When the last round still stored something the budget was too small:
 * DT_STATUS_NOT_CONVERGED is raised on the context (dt_ctx_status) and the output is not valid; call again with a larger
 * budget.  out must be neither mask nor marker.  The workspace is the context's scratch (a few bytes per tile of
 * 64 x 64; 4 bytes per cell more for out8, 28 more for DT_MORPH_WINDOW); nothing is kept between calls. */
int dt_dev_morph_reconstruct(dt_ctx *ctx, int mode, int erosion, int connectivity, const float *mask,
                             const float *marker, const uint8_t *seeds, double h, int radius, int64_t rows,
                             int64_t cols, int visit_limit, int rounds, float *out, uint8_t *out8);
/* dt_harmonic on device rasters (rows x cols = H x W), on the context's stream, without a host synchronisation: the
 * pyramid, then on every level from the coarsest to the finest max_rounds rounds of tile visits, each with its
 * residual -- the launches behind a round that met tol return at once -- and the injection into the next level.  When
 * the finest level's last residual exceeds tol the budget was too small: DT_STATUS_NOT_CONVERGED is raised on the
 * context (dt_ctx_status) and `out` holds the last iterate; call again with a larger budget.  info (int64[
 * DT_HARMONIC_INFO_WORDS] ON THE DEVICE, may be NULL) is written by the last launch.  The workspace (about 4 bytes per
 * cell and 8 bytes per level and round) is the context's scratch; nothing is kept between calls.  domain may be NULL. */
int dt_dev_harmonic(dt_ctx *ctx, const float *values, const int8_t *fixed, const int8_t *domain, int64_t rows,
                    int64_t cols, double tol, int max_rounds, double *out, int64_t *info);
/* dt_inundation on device rasters (rows x cols = H x W; the inflow table on the device too, par in host memory), on
 * the context's stream, without a host synchronisation: exactly max_steps (0..DT_INUNDATION_DEV_STEPS_MAX) guarded
 * steps are enqueued, two launches each, and those that come after t_end return at once -- info[7] says whether t_end
 * was reached; call again with steps0 = info[0] and par[1] = t to go on.  info (int64[DT_INUNDATION_INFO_WORDS] ON
 * THE DEVICE, may be NULL) is written by the last launch.  The workspace (24 bytes per cell: the second copy of the
 * state) is the context's scratch; nothing is kept between calls. */
int dt_dev_inundation(dt_ctx *ctx, const float *z, const float *manning, const float *rain, int64_t rows, int64_t cols,
                      const double *par, int boundary, const int64_t *cells, const double *times,
                      const double *discharge, int K, int T, int64_t steps0, int64_t max_steps, double *h, double *qx,
                      double *qy, double *max_depth, double *arrival, int64_t *info);
/* dt_regions_label, dt_regions_select and dt_inundate_connected on device rasters (rows x cols = H x W), on the
 * context's stream: three to five launches whatever the rasters hold, none synchronises.  The workspace (12 bytes per
 * cell, 14 for the inundation) is the context's scratch; nothing is kept between calls.  size and seeds may be NULL. */
int dt_dev_regions_label(dt_ctx *ctx, const uint8_t *mask, int64_t rows, int64_t cols, int connectivity,
                         int64_t *label, int64_t *size);
int dt_dev_regions_select(dt_ctx *ctx, const uint8_t *mask, const uint8_t *seeds, int64_t rows, int64_t cols,
                          int connectivity, int64_t min_cells, uint8_t *keep);
int dt_dev_inundate_connected(dt_ctx *ctx, const int32_t *catch_, const void *hand, int hand_bytes,
                              const double *stage, const int8_t *river, int64_t rows, int64_t cols, int64_t R,
                              int connectivity, float *depth);
/* flow accumulation with the river mask (acc > threshold, Example/example.py:52) written by the
 * same final pass */
int dt_dev_flowacc_river(dt_ctx *ctx, const uint8_t *fdr, const float *dem, int64_t H, int64_t W,
                         int64_t threshold, int32_t *acc32, int8_t *river);
/* the same and the first phase of HAND (tile solve, perimeter node doubling) in one call: the single-raster form
 * of dt_dev_flowacc_finish_flowhand_local_w.  dt_dev_flowhand_finish_w / dt_dev_flowhand_gfi_finish_w with the whole
 * raster as the window (ld = W, halo 0) follow on the same context. */
int dt_dev_flowacc_river_flowhand_local(dt_ctx *ctx, const uint8_t *fdr, const float *dem, int64_t H, int64_t W,
                                        int64_t threshold, int32_t *acc32, int8_t *river);
/* The same with the nodata mask the D8 kernel can write on its way: dt_dev_slope_d8_m = dt_dev_slope_d8 (codes only)
 * that also fills `nodata4` -- one 16-bit word per 4 x 4 patch of cells, bit 4 j + k = cell (4 r + j, 4 i + k) holds the
 * sentinel (z <= -100); dt_nodata_mask_bytes(4, W) bytes per row of patches, dt_nodata_mask_bytes(H, W) in all -- and
 * dt_dev_flowacc_river_flowhand_local_m reads that mask instead of the DEM where it only needs "is this cell nodata"
 * (0.125 instead of 4 bytes per cell; the resident chain's form).  Heights that are NaN or +inf are outside the
 * contract of the mask (the D8 kernel treats them as nodata -- code 0, mask bit set --, `dem <= -100` does not). */
int64_t dt_nodata_mask_bytes(int64_t H, int64_t W);
int dt_dev_slope_d8_m(dt_ctx *ctx, const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr, uint8_t *nodata4);
int dt_dev_flowacc_river_flowhand_local_m(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const uint8_t *nodata4,
                                          int64_t H, int64_t W, int64_t threshold, int32_t *acc32, int8_t *river);
/* Slope out of the D8 kernel and TI / MTI out of the last accumulation tile pass (the float32 resident chain's form: no
 * slope + TI + MTI pass over the raster).  dt_dev_slope_d8_ms = dt_dev_slope_d8_m that also writes `slope` (NULL: it IS
 * dt_dev_slope_d8_m) and records the cells whose float32 slope is not proven in `marks` (dt_slope_marks_bytes(H, W) bytes
 * of device memory, 16-byte aligned); dt_dev_flowacc_river_flowhand_local_ms reads that slope raster, writes ti / mti
 * beside acc32 and adds the cells whose TI / MTI fast path fails to `marks`; dt_dev_slope_twi_fix then recomputes slope,
 * ti and mti of the marked cells exactly.  The three calls give bit for bit what dt_dev_slope_twi gives.  Only where
 * dt_slope_from_d8_ok(H, W) != 0 (rows of whole 64-cell tiles) and the rasters are 16-byte aligned; otherwise
 * dt_dev_flowacc_river_flowhand_local_ms fails with DT_EINVAL and dt_dev_slope_twi is the way. */
int dt_slope_from_d8_ok(int64_t H, int64_t W);
int64_t dt_slope_marks_bytes(int64_t H, int64_t W);
int dt_dev_slope_d8_ms(dt_ctx *ctx, const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr, uint8_t *nodata4,
                       float *slope, void *marks);
int dt_dev_flowacc_river_flowhand_local_ms(dt_ctx *ctx, const uint8_t *fdr, const float *dem, const uint8_t *nodata4,
                                           int64_t H, int64_t W, int64_t threshold, int32_t *acc32, int8_t *river,
                                           double px, double n_top, const float *slope, float *ti, float *mti,
                                           void *marks);
int dt_dev_slope_twi_fix(dt_ctx *ctx, const float *dem, const int32_t *acc32, int64_t H, int64_t W, double px,
                         double n_top, float *slope, float *ti, float *mti, const void *marks);
/* The resident chain on float64 heights (descriptools_amd.chain.Chain(heights="float64")); `dem` is an H x W double
 * raster on the device.  Conditioning has its own float64 entry points (dt_dev_condition_d8_f64*), ranks their
 * windowed ones (dt_*_f64_w below: tiling.RankTile(heights="float64")).  Out of scope on float64 heights: the
 * long-walk skip tables, conditioning over ranks (dt_dev_condition_stage*_w), evaluation of a float64 raster.
 * dt_dev_slope_d8_f64: D8 codes as dt_d8_f64 (fdr may be NULL), and the float32 nodata proxy (may be NULL): -100 where
 * z <= -100, otherwise (float)z kept above -100 -- what the flow-accumulation / HAND-index entry points
 * (dt_dev_flowacc_river_flowhand_local, dt_dev_flowhand_finish_w with dem = hand = NULL) need of the DEM.
 * dt_dev_slope_twi_f64: dt_dev_slope_twi with the slope (slope.py:244-259) taken from float64 differences.
 * dt_dev_downslope_f64: dt_downslope_f64 on device rasters, staged through LDS windows.
 * dt_dev_hand_gfi_f64: HAND in float64 (flowhand.py:436-438) from the int32 river index, GFI (A = acc32[idx]) and
 * ln(hl/H) (the cell's own acc32, 0 -> 1) from it; gfi / lnhlh may be NULL; size = px. */
int dt_dev_slope_d8_f64(dt_ctx *ctx, const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *proxy);
int dt_dev_slope_twi_f64(dt_ctx *ctx, const double *dem, const int32_t *acc32, int64_t H, int64_t W, double px,
                         double n_top, float *slope, float *slope_rad, float *ti, float *mti);
int dt_dev_downslope_f64(dt_ctx *ctx, const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                         double elevation_difference, int raw, float *out);
int dt_dev_hand_gfi_f64(dt_ctx *ctx, const double *dem, const int32_t *idx32, const int32_t *acc32, int64_t H,
                        int64_t W, double px, double n_gfi, double scale_factor, double *hand, float *gfi,
                        float *lnhlh);
int dt_dev_river_mask(dt_ctx *ctx, const int32_t *acc32, int64_t N, int64_t threshold,
                      int8_t *river);
/* idx32: local flat index of the drained-to river cell (int32), -100 = none; a_river (may be
 * NULL, needs acc32) = acc32[idx] carried as payload (removes gfi.river_accumulation's gather;
 * -100 where there is no river cell, i.e. where hand is -100 and GFI is -100 whatever the area) */
int dt_dev_flowhand(dt_ctx *ctx, const float *dem, const uint8_t *fdr, const int8_t *river,
                    const int32_t *acc32, int64_t H, int64_t W, double px, float *fdist,
                    int32_t *idx32, float *hand, int32_t *a_river);
/* the same plus GFI and ln(hl/H) (gfi.py:268-294, :404-440; size = px as in example.py:81-91) evaluated in the
 * last tile pass from the HAND / river accumulation it holds in registers: one pass over the rasters less than
 * dt_dev_flowhand + dt_dev_gfi_lnhlh.  a_river may be NULL. */
int dt_dev_flowhand_gfi(dt_ctx *ctx, const float *dem, const uint8_t *fdr, const int8_t *river,
                        const int32_t *acc32, int64_t H, int64_t W, double px, double n_gfi, double b,
                        float *fdist, int32_t *idx32, float *hand, int32_t *a_river, float *gfi, float *lnhlh);
int dt_dev_twi(dt_ctx *ctx, const int32_t *acc32, const float *slope_rad, int64_t N, double px,
               double n_top, float *ti, float *mti);
/* a_river[i] = fac[idx[i]] (or anything where hand <= -100) */
int dt_dev_gfi(dt_ctx *ctx, const float *hand, const int32_t *a_river, int64_t N, double n_gfi,
               double scale_factor, double size, float *gfi);
int dt_dev_lnhlh(dt_ctx *ctx, const float *hand, const int32_t *acc32, int64_t N, double n_gfi,
                 double scale_factor, double size, float *out);
/* GFI and ln(hl/H) fused: one read of hand, ln(hand + 0.01) evaluated once */
int dt_dev_gfi_lnhlh(dt_ctx *ctx, const float *hand, const int32_t *a_river, const int32_t *acc32,
                     int64_t N, double n_gfi, double scale_factor, double size, float *gfi, float *lnhlh);
int dt_dev_downslope(dt_ctx *ctx, const float *dem, const uint8_t *fdr, int64_t H, int64_t W,
                     double px, double elevation_difference, int raw, float *out);
/* The same with the long-walk acceleration: walks that leave the kernel's window and are still short of the elevation
 * difference after 32 further moves are queued and finished with skip tables (8 moves per skip for every cell, 16 / 32 /
 * 64 for the queued cells, built on the device when at least 256 walks were queued) -- on real, conditioned terrain,
 * where flats and valley floors make walks thousands of moves long, an order of magnitude faster; same results.
 * `work`: dt_downslope_lift_workspace(H, W) bytes of device memory (33 bytes per cell), the library's for the duration
 * of the call's kernels. */
int64_t dt_downslope_lift_workspace(int64_t H, int64_t W);
int dt_dev_downslope_lift(dt_ctx *ctx, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                          double dz, int raw, float *out, void *work, int64_t work_bytes);
/* The same in two steps, for callers that may synchronise in between and want the tables' 25 bytes per cell only for
 * rasters that need them: dt_dev_downslope_queue runs the window kernel and queues the long walks (qwork:
 * dt_downslope_queue_workspace bytes, 8 per cell); dt_dev_downslope_queued waits for it and returns their number;
 * dt_dev_downslope_finish finishes them -- with skip tables when twork (dt_downslope_tables_workspace bytes) is given
 * and at least dt_downslope_tables_threshold walks are queued, move by move otherwise (twork may be NULL). */
int64_t dt_downslope_queue_workspace(int64_t H, int64_t W);
int64_t dt_downslope_tables_workspace(int64_t H, int64_t W);
int64_t dt_downslope_tables_threshold(int64_t H, int64_t W);
int dt_dev_downslope_queue(dt_ctx *ctx, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                           double dz, int raw, float *out, void *qwork, int64_t qbytes);
int dt_dev_downslope_queued(dt_ctx *ctx, const void *qwork, int64_t *count);
int dt_dev_downslope_finish(dt_ctx *ctx, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                            double dz, int raw, float *out, void *qwork, int64_t qbytes, void *twork, int64_t tbytes);
/* counts4_dev: device int64[nth*4], zeroed by the call */
int dt_dev_confusion_multi(dt_ctx *ctx, const double *desc, const int8_t *flood, int64_t N,
                           double nodata_value, const double *th_host, int nth, int under,
                           int64_t *counts4_dev);
/* dt_threshold_hist on resident rasters: th_dev = device float64[K], hist_dev = device int64[2 (K + 1) + 1], zeroed by
 * the call.  PRECONDITIONS, not checked: th_dev is ascending by `<=` and holds no NaN (the search counts a prefix of the
 * table; on an unsorted table the bins are meaningless, though every access stays inside the arrays).  N <= 2^39.  One
 * memset and one launch on the context's stream while K + 1 <= 18432 bins fit the workgroup's LDS, one launch per 18432
 * bins above; no scratch. */
int dt_dev_threshold_hist(dt_ctx *ctx, const double *desc, const int8_t *flood, int64_t N, double nodata_value,
                          const double *th_dev, int K, int under, int64_t *hist_dev);
/* ---- windowed device tier: the same kernels on one rank's window of a larger raster (multi-GPU).
 * Flow accumulation and HAND are split in two phases so the ranks can exchange one summary row per
 * cell of their core ring in between (descriptools_amd/tiling.py).  Ring order: top row, bottom row,
 * left column, right column (dt_perim_cells(H, W) rows). ------------------------------------------ */
int64_t dt_perim_cells(int64_t H, int64_t W);
/* hydrological conditioning on one rank's window (SURVEY.md 8f-4 tiled over ranks): the fixed points of
 * dt_dev_condition_d8 are iterated per rank, with a halo exchange of the filled surface / the flat distances and an
 * all-reduce of the "changed" flag in between (descriptools_amd/tiling.py: condition_ranks).  stage 0: init of the
 * surface (outlets: edge of the GLOBAL raster, cells next to nodata); 1: `rounds` fill rounds over the core, reading
 * the halo; 2: init of the flat distances (after D8 on the surface, dt_dev_slope_d8_w); 3: `rounds` flat rounds;
 * 4: the flat cells' codes.  *flag_dev (device int32, zeroed by the caller): raised by stages 1 / 3 when a cell changed,
 * number of cells left without a code after stage 4.  dist: uint32 raster laid out like the others. */
int dt_dev_condition_stage_w(dt_ctx *ctx, const dt_window *win, int stage, int rounds, const float *dem, float *filled,
                             uint8_t *fdr, uint32_t *dist, int32_t *flag_dev);
/* The same with a byte raster `nsame` (laid out like the others; the library's between stage 2 and stage 4): stage 2
 * leaves one byte per cell there -- which neighbours have another filled height -- and stages 3 / 4 work from it instead
 * of from the surface (less traffic and LDS per tile visit; same results). */
int dt_dev_condition_stage_m_w(dt_ctx *ctx, const dt_window *win, int stage, int rounds, const float *dem, float *filled,
                               uint8_t *fdr, uint32_t *dist, int32_t *flag_dev, uint8_t *nsame);
int dt_dev_slope_d8_w(dt_ctx *ctx, const dt_window *win, const float *dem, double px, float *slope,
                      uint8_t *fdr, float *slope_rad);
int dt_dev_slope_twi_w(dt_ctx *ctx, const dt_window *win, const float *dem, const int32_t *acc32, double px,
                       double n_top, float *slope, float *slope_rad, float *ti, float *mti);
/* n_unresolved_dev (device int32, may be NULL): walks that left this rank's halo (marked -50) */
int dt_dev_downslope_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr, double px,
                       double elevation_difference, int raw, float *out, int32_t *n_unresolved_dev);
/* The same with the long-walk workspace (dt_dev_downslope_lift, for a rank): `work` = dt_downslope_lift_workspace_w(win)
 * bytes (8 per core cell for the queue, 24 per cell of the rank's memory -- core + halo -- for the skip tables).  On
 * real terrain (flats, valley floors) the walks of thousands of moves that stay in the rank's memory are finished in
 * skips of 64 moves instead of one dependent load per move (four ranks of the Example tiled 4 x 4: 69 -> see DESIGN.md
 * ms); the ones that leave it are marked and counted exactly as by dt_dev_downslope_w.  Same results bit for bit. */
int64_t dt_downslope_lift_workspace_w(const dt_window *win);
int dt_dev_downslope_lift_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr, double px,
                            double elevation_difference, int raw, float *out, int32_t *n_unresolved_dev, void *work,
                            int64_t work_bytes);
/* Downslope walks that leave a rank's memory (real terrain: walks of thousands of moves along valley floors cross rank
 * borders).  dt_dev_downslope_emit_w = dt_dev_downslope_w (work NULL) / dt_dev_downslope_lift_w (work = the long-walk
 * workspace) that additionally EMITS every such walk, where it leaves, as a 48-byte walker record into `walkers`
 * (bytes 0-3: number of walks emitted, possibly more than fit; records from byte 256):
 *   words 0-3  start cell (global row, column), cell the walk stands on (global row, column)
 *   words 4-7  moves made, diagonal moves, float bits of the start height, flags (1 = carries the reference's
 *              sequential float64 path length instead of counts, 2 = finished)
 *   words 8-11 that float64 sum (two words), float bits of the result (finished walkers), 0
 * dt_dev_downslope_walk_w advances, in place, the n records that stand in this rank's memory until they finish or
 * reach the end of it again (the host sends them on: descriptools_amd/tiling.finish_downslope uses an all-to-all of
 * device buffers; the reference's analogue is the CPU repair downslope.py:373-374).  dt_dev_downslope_walk_seed_w
 * writes records of walkers at their start cells (core coordinates) for cells that are marked -50 without one. */
int dt_dev_downslope_emit_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr, double px,
                            double elevation_difference, int raw, float *out, int32_t *n_unresolved_dev, void *work,
                            int64_t work_bytes, void *walkers, int64_t walkers_bytes);
int dt_dev_downslope_walk_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr, double px,
                            double elevation_difference, int64_t n, void *records, void *work, int64_t work_bytes);
/* One iteration of the walkers' journey prepared on the device: records that arrived finished (flag 2) are home -- their
 * value is written into `out` (this rank's downslope raster, core origin) and they are marked (flag 4) -- the others
 * advance like dt_dev_downslope_walk_w; every record still wanted somewhere is then copied into `send` grouped by
 * destination rank (a walker that has just finished: the owner of its start cell; otherwise the owner of the cell it
 * stands on), counts[d] = records for rank d and counts[ty * tx] = how many of them are still on their way.  The host
 * reads `counts` (its one synchronisation), exchanges them and the groups (all-to-all), and calls again with what it
 * received until no rank sends anything.  row_starts[ty + 1] / col_starts[tx + 1]: first global row / column of every
 * rank row / column and the raster's end (device arrays; rank = rank row * tx + rank column, at most 1024 ranks);
 * counts: int32[ty * tx + 1]; scratch: int32[n + ty * tx]; send: room for n records. */
int dt_dev_downslope_walk_route_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr, double px,
                                  double elevation_difference, int64_t n, void *records, void *work, int64_t work_bytes,
                                  float *out, const int32_t *row_starts, int32_t ty, const int32_t *col_starts,
                                  int32_t tx, void *send, int32_t *counts, int32_t *scratch);
int dt_dev_downslope_walk_seed_w(dt_ctx *ctx, const dt_window *win, const float *dem, int64_t n, const int32_t *ys,
                                 const int32_t *xs, void *records);
/* phase 1: in-rank accumulation; per ring cell: A = cells of this rank draining OUT through it (0 unless
 * its D8 step leaves the core), code = that step's D8 code, xr = ring index of the rank exit reached by
 * a path ENTERING at this cell (-1 none, -2 cycle inside the rank).  acc32 is not touched by this phase (the raster
 * is written by dt_dev_flowacc_finish_w / _w_a64) and may be NULL. */
int dt_dev_flowacc_local_w(dt_ctx *ctx, const dt_window *win, const uint8_t *fdr, int32_t *acc32,
                           int64_t *A_perim, int32_t *xr_perim, uint8_t *code_perim);
/* phase 2: ext_perim[i] = inflow arriving at ring cell i from other ranks (bit 63: fed by a D8 cycle
 * spanning ranks); NULL = none.  Must directly follow phase 1 on the same context. */
int dt_dev_flowacc_finish_w(dt_ctx *ctx, const dt_window *win, const uint8_t *fdr, const float *dem,
                            const uint64_t *ext_perim, int64_t threshold, int32_t *acc32, int8_t *river);
/* phase 2 of flow accumulation and phase 1 of HAND in one call: the last accumulation tile pass and HAND's first
 * stage the same 64 x 64 tiles of direction codes, and HAND's river mask is what the accumulation pass has just
 * computed, so in the common form (int32 accumulation, core width a multiple of 64, 16-byte aligned rasters) they are
 * ONE kernel; otherwise the separate kernels run back to back.  Results and the state left in the context are those
 * of dt_dev_flowacc_finish_w followed by dt_dev_flowhand_local_w (whose summary outputs kind ... ar these are). */
int dt_dev_flowacc_finish_flowhand_local_w(dt_ctx *ctx, const dt_window *win, const uint8_t *fdr, const float *dem,
                                           const uint64_t *ext_perim, int64_t threshold, int32_t *acc32, int8_t *river,
                                           uint8_t *kind, int32_t *ref, int32_t *nc, int32_t *nd, float *zr,
                                           int64_t *ar);
/* phase 1: per ring cell, the path ENTERING the rank there: kind 1 = ends on river cell `ref` (core-local
 * flat index; zr / ar = its height / accumulation), 2 = dead, 4 = leaves the rank again through ring
 * cell `ref`; nc / nd = cardinal / diagonal moves (kind 4: including the step out of the rank).  Everything that
 * crosses ranks carries accumulations as int64 (ar here, rem_ar below), whatever the rasters' width. */
int dt_dev_flowhand_local_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr,
                            const int8_t *river, const int32_t *acc32, uint8_t *kind, int32_t *ref,
                            int32_t *nc, int32_t *nd, float *zr, int64_t *ar);
/* phase 2: for every ring cell whose step leaves the rank: res_ok != 0 -> that path ends on a river
 * cell after res_nc / res_nd further moves, global flat index rem_gidx, height rem_zr, accumulation
 * rem_ar (all NULL = no other ranks).  idx64 (may be NULL) receives GLOBAL flat indices; so does idx32 (may be NULL)
 * whenever the rank tables or idx64 are given -- meaningful while the global raster has <= 2^31 cells, and half
 * the bytes -- and the core-local flat index otherwise (a single raster: the same thing). */
int dt_dev_flowhand_finish_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr,
                             const int8_t *river, const int32_t *acc32, double px, const uint8_t *res_ok,
                             const int32_t *res_nc, const int32_t *res_nd, const int64_t *rem_gidx,
                             const float *rem_zr, const int64_t *rem_ar, float *fdist, int32_t *idx32,
                             int64_t *idx64, float *hand, int32_t *a_river);
int dt_dev_flowhand_gfi_finish_w(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr,
                                 const int8_t *river, const int32_t *acc32, double px, double n_gfi, double b,
                                 const uint8_t *res_ok, const int32_t *res_nc, const int32_t *res_nd,
                                 const int64_t *rem_gidx, const float *rem_zr, const int64_t *rem_ar,
                                 float *fdist, int32_t *idx32, int64_t *idx64, float *hand, int32_t *a_river,
                                 float *gfi, float *lnhlh);

/* ---- one rank's step on float64 heights (tiling.RankTile(heights="float64")): windowed forms of the float64 chain's
 * entry points above, with the window semantics of the float32 _w entries (core + halo in the rank's memory, -100 only
 * outside the GLOBAL raster, no D8 code on the last ring of that memory).  The flow-accumulation / HAND-index entries
 * (dt_dev_flowacc_*_w, dt_dev_flowhand_*_w with dem = the float32 nodata proxy, hand = NULL) are shared.
 * dt_dev_slope_d8_f64_w: D8 codes (may be NULL) and the nodata proxy (may be NULL) over the window -- for RankTile.d8
 *   the core plus the halo minus its outer ring, as dt_dev_slope_d8_w.
 * dt_dev_slope_twi_f64_w (_a64): dt_dev_slope_twi_w with the slope from float64 differences.
 * dt_dev_downslope_f64_w: as dt_dev_downslope_w (walks that leave the rank's memory: -50 and *n_unresolved_dev).
 * dt_dev_downslope_walk_seed_f64_w / dt_dev_downslope_walk_route_f64_w: the walker entries for such walks on float64
 *   heights.  Records are 48 bytes as above, always flag 1 (words 8-9: the reference's sequential float64 path
 *   length); the start height is a double: low word in word 6, high word in word 11.
 * dt_dev_flowhand_zr64_w: after the HAND summary (dt_dev_flowhand_local_w or the fused phase), zr64[i] = the float64
 *   height of the river cell summary entry i ends on (kind 1), -100 otherwise: the eighth field of the float64 HAND row.
 * dt_dev_rank_solve_flowhand_f64: dt_dev_rank_solve_flowhand on rows with that eighth field (field_offsets8[7], 8-byte
 *   aligned); rem_zr64 = the float64 height of the river cell each rank exit's path ends on.
 * dt_dev_hand_gfi_f64_w (_a64): HAND in float64 from the GLOBAL river index (idx32 or idx64), GFI with A = a_river (the
 *   river-accumulation payload of dt_dev_flowhand_finish_w) and ln(hl/H) with the cell's own accumulation; the river
 *   height comes from the rank's memory, or for a river cell on another rank from (rem_gidx, rem_zr64) of the n_remote
 *   ring cells (res_ok) through `table` (dt_hand_f64_table_bytes(n_remote) bytes of device memory); size = px. */
int dt_dev_slope_d8_f64_w(dt_ctx *ctx, const dt_window *win, const double *dem, double px, uint8_t *fdr, float *proxy);
int dt_dev_slope_twi_f64_w(dt_ctx *ctx, const dt_window *win, const double *dem, const int32_t *acc32, double px,
                           double n_top, float *slope, float *slope_rad, float *ti, float *mti);
int dt_dev_slope_twi_f64_w_a64(dt_ctx *ctx, const dt_window *win, const double *dem, const int64_t *acc64, double px,
                               double n_top, float *slope, float *slope_rad, float *ti, float *mti);
int dt_dev_downslope_f64_w(dt_ctx *ctx, const dt_window *win, const double *dem, const uint8_t *fdr, double px,
                           double elevation_difference, int raw, float *out, int32_t *n_unresolved_dev);
int dt_dev_downslope_walk_seed_f64_w(dt_ctx *ctx, const dt_window *win, const double *dem, int64_t n, const int32_t *ys,
                                     const int32_t *xs, void *records);
int dt_dev_downslope_walk_route_f64_w(dt_ctx *ctx, const dt_window *win, const double *dem, const uint8_t *fdr,
                                      double px, double elevation_difference, int64_t n, void *records, float *out,
                                      const int32_t *row_starts, int32_t ty, const int32_t *col_starts, int32_t tx,
                                      void *send, int32_t *counts, int32_t *scratch);
int dt_dev_flowhand_zr64_w(dt_ctx *ctx, const dt_window *win, const double *dem, int64_t n, const uint8_t *kind,
                           const int32_t *ref, double *zr64);
int dt_dev_rank_solve_flowhand_f64(dt_ctx *ctx, int ty, int tx, const int64_t *heights, const int64_t *widths,
                                   int64_t Pmax, const void *rows_dev, int64_t rowbytes,
                                   const int64_t *field_offsets8, int rank, int64_t P_rank, uint8_t *res_ok,
                                   int32_t *res_nc, int32_t *res_nd, int64_t *rem_gidx, float *rem_zr,
                                   int64_t *rem_ar, double *rem_zr64);
int64_t dt_hand_f64_table_bytes(int64_t n_remote);
int dt_dev_hand_gfi_f64_w(dt_ctx *ctx, const dt_window *win, const double *dem, const int32_t *idx32,
                          const int64_t *idx64, const int32_t *acc32, const int32_t *a_river32, int64_t n_remote,
                          const uint8_t *res_ok, const int64_t *rem_gidx, const double *rem_zr64, void *table,
                          int64_t table_bytes, double px, double n_gfi, double scale_factor, double *hand, float *gfi,
                          float *lnhlh);
int dt_dev_hand_gfi_f64_w_a64(dt_ctx *ctx, const dt_window *win, const double *dem, const int32_t *idx32,
                              const int64_t *idx64, const int64_t *acc64, const int64_t *a_river64, int64_t n_remote,
                              const uint8_t *res_ok, const int64_t *rem_gidx, const double *rem_zr64, void *table,
                              int64_t table_bytes, double px, double n_gfi, double scale_factor, double *hand,
                              float *gfi, float *lnhlh);

/* ---- the same steps on int64 accumulation rasters (`_a64`).  The reference's flow accumulation is int64 end to
 * end (Example/example.py:39 reads it as int64; topoindexes.py:252-261, gfi.py:141-143 and :432-440 consume it).  On
 * the device a raster of up to 2^31 cells keeps it as int32 (half the bytes; exact, an accumulation being at most
 * cells - 1); a larger raster split
 * over ranks -- BASELINE.json configs[4], 65536^2 -- can hold basins beyond 32 bits, and its ranks run these entry
 * points instead: accumulation, river accumulation payload and every consumer (TI / MTI, HAND's river payload, GFI,
 * ln(hl/H)) in 64 bits; DT_STATUS_ACC_OVERFLOW is never raised.  dt_dev_flowacc_local_w, the rank-level solves and
 * dt_dev_downslope_w do not touch the accumulation raster and are shared. */
int dt_dev_flowacc_finish_w_a64(dt_ctx *ctx, const dt_window *win, const uint8_t *fdr, const float *dem,
                                const uint64_t *ext_perim, int64_t threshold, int64_t *acc64, int8_t *river);
int dt_dev_flowacc_finish_flowhand_local_w_a64(dt_ctx *ctx, const dt_window *win, const uint8_t *fdr, const float *dem,
                                               const uint64_t *ext_perim, int64_t threshold, int64_t *acc64,
                                               int8_t *river, uint8_t *kind, int32_t *ref, int32_t *nc, int32_t *nd,
                                               float *zr, int64_t *ar);
int dt_dev_slope_twi_w_a64(dt_ctx *ctx, const dt_window *win, const float *dem, const int64_t *acc64, double px,
                           double n_top, float *slope, float *slope_rad, float *ti, float *mti);
int dt_dev_flowhand_local_w_a64(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr,
                                const int8_t *river, const int64_t *acc64, uint8_t *kind, int32_t *ref,
                                int32_t *nc, int32_t *nd, float *zr, int64_t *ar);
int dt_dev_flowhand_finish_w_a64(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr,
                                 const int8_t *river, const int64_t *acc64, double px, const uint8_t *res_ok,
                                 const int32_t *res_nc, const int32_t *res_nd, const int64_t *rem_gidx,
                                 const float *rem_zr, const int64_t *rem_ar, float *fdist, int32_t *idx32,
                                 int64_t *idx64, float *hand, int64_t *a_river64);
int dt_dev_flowhand_gfi_finish_w_a64(dt_ctx *ctx, const dt_window *win, const float *dem, const uint8_t *fdr,
                                     const int8_t *river, const int64_t *acc64, double px, double n_gfi, double b,
                                     const uint8_t *res_ok, const int32_t *res_nc, const int32_t *res_nd,
                                     const int64_t *rem_gidx, const float *rem_zr, const int64_t *rem_ar,
                                     float *fdist, int32_t *idx32, int64_t *idx64, float *hand,
                                     int64_t *a_river64, float *gfi, float *lnhlh);
int dt_dev_gfi_lnhlh_a64(dt_ctx *ctx, const float *hand, const int64_t *a_river64, const int64_t *acc64, int64_t N,
                         double n_gfi, double scale_factor, double size, float *gfi, float *lnhlh);

/* evaluation on resident rasters.  out3_dev (device float[3]) = smallest,
 * second-smallest distinct and largest value of x, i.e. np.unique(x)[0], [1], [-1] as
 * Example/example.py:113-115 uses them (NaN when absent). */
int dt_dev_unique_extremes_f32(dt_ctx *ctx, const float *x, int64_t N, float *out3_dev);
/* evaluation.minMaxScale (evaluation.py:5-9) of a float32 raster: float32 arithmetic like numpy,
 * NaN where x == nodata, written as the float64 raster dt_dev_confusion_multi reads. */
int dt_dev_minmax_scale_f32(dt_ctx *ctx, const float *x, int64_t N, float mn, float mx, float nodata,
                            double *desc);

/* the same for an integer-valued raster kept as float32 on the device (the example's int16 HAND): float64
 * arithmetic, as numpy scales integer rasters */
int dt_dev_minmax_scale_f32_f64(dt_ctx *ctx, const float *x, int64_t N, double mn, double mx, double nodata,
                                double *desc);
/* binary_map + avaliacao at one threshold on resident rasters (Example/example.py:139-147): binary (may be NULL),
 * klass = binary + remapped flood (may be NULL), counts4_dev[v] = cells of class v; remap_flood != 0 rewrites the
 * benchmark map in place (1 -> 2, -100 -> 0) as avaliacao does. */
int dt_dev_classify(dt_ctx *ctx, const double *desc, int8_t *flood, int64_t N, double nodata_value, double threshold,
                    int under, int remap_flood, uint8_t *binary, int32_t *klass, int64_t *counts4_dev);

/* Device-to-device copy of N floats, the practical HBM ceiling the roofline fractions are put beside:
 * blocks > 0: float4 grid-stride copy with that many workgroups; blocks < 0: the buffer walked as rows of 16384
 * floats in 1024 x 4 patches, one per workgroup (N a multiple of 65536) -- the faster of the two forms on
 * MI355X (6.1 vs 5.4 TB/s), bench.py reports the better one */
int dt_dev_membench_copy(dt_ctx *ctx, const float *a, float *b, int64_t N, int blocks);
/* The same patches with n_reads (0-2) read streams summed into n_writes (1-3) write streams, optionally with
 * non-temporal loads / stores: the rate the memory system gives a read / write MIX with no arithmetic in the way.
 * The fused slope + TI + MTI stencil is 2 reads + 3 writes (60 % of its bytes are written). */
int dt_dev_membench_mix(dt_ctx *ctx, const float *r0, const float *r1, float *w0, float *w1, float *w2, int64_t N,
                        int n_reads, int n_writes, int nontemporal);
/* `reps` launches of dt_dev_membench_mix bracketed by HIP events on the context's stream (after one untimed launch):
 * *ms = mean duration of one launch.  Synchronises.  What descriptools_amd/placement.py labels blocks with. */
int dt_dev_membench_mix_timed(dt_ctx *ctx, const float *r0, const float *r1, float *w0, float *w1, float *w2, int64_t N,
                              int n_reads, int n_writes, int nontemporal, int reps, double *ms);
/* free / total bytes of the context's device (hipMemGetInfo) */
int dt_dev_mem_info(dt_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);

/* Rank-level solves on the GPU (multi-GPU): `rows_dev` holds one all-gathered byte row per rank
 * (rowbytes apart); field k of rank r starts at rows_dev + r * rowbytes + field_offsets[k] and has Pmax
 * entries.  heights / widths (host) describe the ty x tx rank grid.
 *   flow accumulation fields: {A int64, xr int32, code uint8} (the outputs of dt_dev_flowacc_local_w)
 *     -> ext_out_dev[P_rank] for dt_dev_flowacc_finish_w
 *   HAND fields: {ref int32, nc int32, nd int32, zr float, ar int64, kind uint8, ring D8 code uint8}
 *     -> the res_* / rem_* arrays [P_rank] for dt_dev_flowhand_finish_w */
int dt_dev_rank_solve_flowacc(dt_ctx *ctx, int ty, int tx, const int64_t *heights, const int64_t *widths,
                              int64_t Pmax, const void *rows_dev, int64_t rowbytes,
                              const int64_t *field_offsets3, int rank, int64_t P_rank, uint64_t *ext_out_dev);
int dt_dev_rank_solve_flowhand(dt_ctx *ctx, int ty, int tx, const int64_t *heights, const int64_t *widths,
                               int64_t Pmax, const void *rows_dev, int64_t rowbytes,
                               const int64_t *field_offsets7, int rank, int64_t P_rank, uint8_t *res_ok,
                               int32_t *res_nc, int32_t *res_nd, int64_t *rem_gidx, float *rem_zr,
                               int64_t *rem_ar);

/* widen / narrow helpers for the int64 API dtypes */
int dt_dev_i32_to_i64(dt_ctx *ctx, const int32_t *src, int64_t N, int64_t *dst);
int dt_dev_i64_to_i32(dt_ctx *ctx, const int64_t *src, int64_t N, int32_t *dst);

#ifdef __cplusplus
}
#endif
#endif /* DESCRIPTOOLS_HIP_H */
