// dt_capi.hip -- extern "C" boundary of libdescriptools_hip.so (see include/descriptools_hip.h).
#include <cmath>
#include <stdarg.h>
#include <stdlib.h>

#include <sys/mman.h>
#include <atomic>
#include <chrono>
#include <mutex>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "dt_common.h"
#include "dt_kernels.h"

// ---- errors -----------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void dt_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char *dt_last_error(void) { return g_err; }
extern "C" const char *dt_version(void) { return "descriptools_hip 0.1 (gfx950)"; }

static int g_debug[DT_DBG_COUNT] = {0};
int dt_debug_get(int key) { return (key >= 0 && key < DT_DBG_COUNT) ? g_debug[key] : 0; }
extern "C" int dt_debug_set(int key, int value) {
  DT_REQUIRE(key >= 0 && key < DT_DBG_COUNT, "unknown debug key");
  DT_REQUIRE(key < DT_DBG_RETIRED_FIRST || key > DT_DBG_RETIRED_LAST,
             "this debug key was retired together with the kernel variants it selected (keys 1-7)");
  g_debug[key] = value;
  return DT_OK;
}

extern "C" int dt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---- context ----------------------------------------------------------------------------------
// live contexts (a graph remembers the context it was captured on and must know whether that still exists)
static std::mutex g_ctx_mu;
static std::vector<dt_ctx *> g_live_ctx;
static bool dt_ctx_alive(dt_ctx *c) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  for (dt_ctx *p : g_live_ctx)
    if (p == c) return true;
  return false;
}

extern "C" int dt_ctx_create(int device, void *stream, dt_ctx **out) {
  DT_REQUIRE(out != nullptr, "out is NULL");
  int n = dt_device_count();
  if (n <= 0) {
    dt_set_error("no HIP device visible");
    return DT_ENODEV;
  }
  DT_REQUIRE(device >= 0 && device < n, "device index out of range");
  DT_HIP(hipSetDevice(device));
  dt_ctx *c = new dt_ctx();
  c->device = device;
  c->scratch = nullptr;
  c->scratch_bytes = 0;
  c->scratch_used = 0;
  c->claim = DtScratchClaim{};
  c->scratch2 = nullptr;
  c->scratch2_bytes = 0;
  c->ev = nullptr;
  c->aux = nullptr;
  c->aux_bytes = 0;
  c->ws_gen = 0;
  c->status = nullptr;
  if (hipMalloc((void **)&c->status, 64) != hipSuccess || hipMemset(c->status, 0, 64) != hipSuccess) {
    dt_set_error("cannot allocate the context's status word");
    delete c;
    return DT_ENOMEM;
  }
  if (stream) {
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      dt_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
      delete c;
      return DT_EHIP;
    }
    c->own_stream = true;
  }
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    g_live_ctx.push_back(c);
  }
  *out = c;
  return DT_OK;
}

extern "C" int dt_ctx_destroy(dt_ctx *c) {
  if (!c) return DT_OK;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (size_t i = 0; i < g_live_ctx.size(); i++)
      if (g_live_ctx[i] == c) {
        g_live_ctx.erase(g_live_ctx.begin() + (long)i);
        break;
      }
  }
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->scratch2) (void)hipFree(c->scratch2);
  if (c->aux) (void)hipFree(c->aux);
  if (c->status) (void)hipFree(c->status);
  if (c->ev) (void)hipEventDestroy(c->ev);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return DT_OK;
}

extern "C" int dt_ctx_set_stream(dt_ctx *c, void *stream) {
  DT_REQUIRE(c != nullptr, "ctx is NULL");
  DT_HIP(hipStreamSynchronize(c->stream));
  if (c->own_stream) DT_HIP(hipStreamDestroy(c->stream));
  if (stream) {
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
  } else {
    DT_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return DT_OK;
}
extern "C" void *dt_ctx_stream(dt_ctx *c) { return c ? (void *)c->stream : nullptr; }

// The context's own stream re-created with a scheduling priority: -1 high, 0 normal, +1 low (clamped to what the
// device offers).  A side branch of a pipeline on a LOW-priority stream fills the slots the main branch leaves
// idle instead of competing with it for every freed slot.
extern "C" int dt_ctx_set_priority(dt_ctx *c, int priority) {
  DT_REQUIRE(c != nullptr, "ctx is NULL");
  DT_REQUIRE(c->own_stream, "the context runs on a caller's stream: create that stream with the priority wanted");
  DT_HIP(hipSetDevice(c->device));
  int least = 0, greatest = 0;  // numerically: least priority = largest value
  DT_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  int pr = priority < greatest ? greatest : (priority > least ? least : priority);
  hipStream_t ns = nullptr;
  DT_HIP(hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, pr));
  DT_HIP(hipStreamSynchronize(c->stream));
  DT_HIP(hipStreamDestroy(c->stream));
  c->stream = ns;
  return DT_OK;
}

// `waiter`'s stream waits for everything enqueued so far on `signaller`'s stream (no host synchronisation)
static int dt_ctx_order(dt_ctx *signaller, dt_ctx *waiter) {
  DT_REQUIRE(signaller != nullptr && waiter != nullptr, "ctx is NULL");
  DT_REQUIRE(signaller->device == waiter->device, "contexts on different devices");
  if (signaller->stream == waiter->stream) return DT_OK;
  DT_HIP(hipSetDevice(signaller->device));
  if (!signaller->ev) DT_HIP(hipEventCreateWithFlags(&signaller->ev, hipEventDisableTiming));
  DT_HIP(hipEventRecord(signaller->ev, signaller->stream));
  DT_HIP(hipStreamWaitEvent(waiter->stream, signaller->ev, 0));
  return DT_OK;
}
extern "C" int dt_ctx_fork(dt_ctx *parent, dt_ctx *child) { return dt_ctx_order(parent, child); }
extern "C" int dt_ctx_join(dt_ctx *parent, dt_ctx *child) { return dt_ctx_order(child, parent); }
extern "C" int dt_ctx_sync(dt_ctx *c) {
  DT_REQUIRE(c != nullptr, "ctx is NULL");
  DT_HIP(hipStreamSynchronize(c->stream));
  return DT_OK;
}
// ---- HIP graphs: record what is enqueued on a context's stream once, replay it with one launch ----------------
// (the chain is ~45 launches per step: one host call per step instead; the step itself is no shorter, see
// chain.Chain.capture)
struct dt_graph {
  hipGraph_t graph;
  hipGraphExec_t exec;
  int device;
  dt_ctx *owner;       // the context it was captured on: the kernels' workspace pointers are that context's
  uint64_t owner_gen;  // its workspace generation at capture time
};
extern "C" int dt_ctx_capture_begin(dt_ctx *c) {
  DT_REQUIRE(c != nullptr, "ctx is NULL");
  DT_HIP(hipSetDevice(c->device));
  DT_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
  return DT_OK;
}
extern "C" int dt_ctx_capture_end(dt_ctx *c, dt_graph **out) {
  DT_REQUIRE(c != nullptr && out != nullptr, "NULL argument");
  *out = nullptr;
  DT_HIP(hipSetDevice(c->device));
  hipGraph_t g = nullptr;
  DT_HIP(hipStreamEndCapture(c->stream, &g));
  DT_REQUIRE(g != nullptr, "nothing was captured");
  hipGraphExec_t e = nullptr;
  hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
  if (err != hipSuccess) {
    (void)hipGraphDestroy(g);
    DT_HIP(err);
  }
  *out = new dt_graph{g, e, c->device, c, c->ws_gen};
  return DT_OK;
}
extern "C" int dt_graph_launch(dt_graph *g, dt_ctx *c) {
  DT_REQUIRE(g != nullptr && c != nullptr, "NULL argument");
  DT_REQUIRE(g->device == c->device, "graph and context on different devices");
  // The captured kernels hold the raw addresses of the capturing context's grow-only workspaces.  A later call
  // that needed a larger one (a bigger raster, dt_dev_condition_d8, a rank-level solve) has freed the old block,
  // and so has destroying that context: replaying would write into freed memory.
  DT_REQUIRE(dt_ctx_alive(g->owner), "the context this graph was captured on has been destroyed: capture again");
  DT_REQUIRE(g->owner->ws_gen == g->owner_gen,
             "a workspace of the capturing context was reallocated after the capture (a call needed more scratch): "
             "the graph's pointers are stale, capture the step again");
  DT_HIP(hipSetDevice(c->device));
  DT_HIP(hipGraphLaunch(g->exec, c->stream));
  return DT_OK;
}
extern "C" int dt_graph_destroy(dt_graph *g) {
  if (!g) return DT_OK;
  (void)hipGraphExecDestroy(g->exec);
  (void)hipGraphDestroy(g->graph);
  delete g;
  return DT_OK;
}
// sticky status bits raised by kernels since the last call (synchronises the stream); bit 0: a flow accumulation
// value of a multi-rank raster may have reached 2^31 and does not fit the int32 accumulation rasters
extern "C" int dt_ctx_status(dt_ctx *c, int32_t *out) {
  DT_REQUIRE(c != nullptr && out != nullptr, "NULL argument");
  DT_HIP(hipSetDevice(c->device));
  DT_HIP(hipMemcpyAsync(out, c->status, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  DT_HIP(hipMemsetAsync(c->status, 0, sizeof(int32_t), c->stream));
  DT_HIP(hipStreamSynchronize(c->stream));
  return DT_OK;
}
extern "C" int64_t dt_ctx_scratch_bytes(dt_ctx *c) { return c ? (int64_t)c->scratch_bytes : 0; }
extern "C" void *dt_ctx_scratch_ptr(dt_ctx *c) { return c ? (void *)c->scratch : nullptr; }

// DT_DBG_POISON (tests): 0x100 | b fills the first `bytes` of a workspace with byte b, on the stream of the call that is
// about to use it, so the fill is ordered before the op's first kernel and before any upload into the block.  Off (0):
// this one integer test, nothing enqueued.
static int dt_poison(hipStream_t s, void *p, size_t bytes) {
  const int v = dt_debug_get(DT_DBG_POISON);
  if (!(v & 0x100) || !p || bytes == 0) return DT_OK;
  DT_HIP(hipMemsetAsync(p, v & 0xFF, bytes, s));
  return DT_OK;
}

int dt_scratch_reset(dt_ctx *c, size_t total) {
  total = dt_align256(total) + 256;
  if (total > c->scratch_bytes) {
    // earlier work on the stream may still use the old block
    DT_HIP(hipStreamSynchronize(c->stream));
    if (c->scratch) DT_HIP(hipFree(c->scratch));
    c->scratch = nullptr;
    c->scratch_bytes = 0;
    c->ws_gen++;
    DT_HIP(hipMalloc((void **)&c->scratch, total));
    c->scratch_bytes = total;
  }
  c->scratch_used = 0;
  c->claim = DtScratchClaim{};  // whatever two-phase state was here is about to be overwritten
  return dt_poison(c->stream, c->scratch, total);  // what this call asked for, not the whole grown block
}
void *dt_scratch_take(dt_ctx *c, size_t bytes) {
  size_t off = c->scratch_used;
  c->scratch_used += dt_align256(bytes);
  if (c->scratch_used > c->scratch_bytes) return nullptr;
  return c->scratch + off;
}

// grow-only side buffers (scratch2: rank-level solves; aux: stencil marks).  Neither carries state from one call to
// the next: every entry that reserves aux launches the hot kernel that writes the marks and the fix-up that reads them
// in the same call, and every rank solve rebuilds its sums and tables from the rows it is given.  So DT_DBG_POISON
// fills the bytes asked for at every reservation, not only when the block is allocated.
static int dt_side_reserve(dt_ctx *c, char **buf, size_t *have, size_t bytes) {
  if (bytes > *have) {
    DT_HIP(hipStreamSynchronize(c->stream));
    if (*buf) DT_HIP(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
    c->ws_gen++;
    DT_HIP(hipMalloc((void **)buf, bytes));
    *have = bytes;
  }
  return dt_poison(c->stream, *buf, bytes);
}

#define DT_CTX(c)                            \
  DT_REQUIRE((c) != nullptr, "ctx is NULL"); \
  DT_HIP(hipSetDevice((c)->device))

// DT_FLOW_IMPL=v1 selects the first-generation global kernels for flow accumulation / HAND
static int g_flow_impl = -1;
int dt_flow_impl() {
  if (g_flow_impl < 0) {
    const char *e = getenv("DT_FLOW_IMPL");
    g_flow_impl = (e && strcmp(e, "v1") == 0) ? 1 : 2;
  }
  return g_flow_impl;
}
extern "C" int dt_set_flow_impl(int impl) {
  DT_REQUIRE(impl == 1 || impl == 2, "impl must be 1 (global kernels) or 2 (tile-hierarchical)");
  g_flow_impl = impl;
  return DT_OK;
}

static int dt_convert_window(const dt_window *in, DtWin *out) {
  DT_REQUIRE(in != nullptr, "window is NULL");
  DT_REQUIRE(in->H >= 0 && in->W >= 0 && in->H * in->W < (1ll << 31), "bad core shape");
  DT_REQUIRE(in->ld >= in->W, "ld < W");
  DT_REQUIRE(in->Hg < (1ll << 31) && in->Wg < (1ll << 31) && in->gy0 >= 0 && in->gx0 >= 0 &&
                 in->gy0 + in->H <= in->Hg && in->gx0 + in->W <= in->Wg, "core window outside the global raster");
  DT_REQUIRE(in->halo >= 0, "negative halo");
  bool touches_all = in->gy0 == 0 && in->gx0 == 0 && in->gy0 + in->H == in->Hg && in->gx0 + in->W == in->Wg;
  DT_REQUIRE(touches_all || in->halo >= 1, "a window inside a larger raster needs a halo of >= 1 cell");
  out->H = (int)in->H; out->W = (int)in->W; out->ld = in->ld; out->gy0 = (int)in->gy0; out->gx0 = (int)in->gx0;
  out->Hg = (int)in->Hg; out->Wg = (int)in->Wg; out->halo = (int)in->halo;
  return DT_OK;
}

// the shape rules of the entries that take (H, W)
static int dt_check_hw(int64_t H, int64_t W) {
  DT_REQUIRE(H >= 0 && W >= 0, "negative raster shape");
  DT_REQUIRE(H * W < (1ll << 31), "rasters of >= 2^31 cells must be tiled (one tile per GPU)");
  return DT_OK;
}
// stream order: flat indices are int64, so the raster may exceed 2^31 cells (the network may not)
static int dt_check_so(int64_t H, int64_t W) {
  DT_REQUIRE(H >= 0 && W >= 0, "negative raster shape");
  DT_REQUIRE(W == 0 || H <= (1ll << 42) / W, "raster too large");
  return DT_OK;
}
// drainage / upslope length / D-infinity: flat indices travel in 31 or 32 bits and the kernels' coordinates in int, so
// the raster has fewer than 2^31 cells
static int dt_check_ws(int64_t H, int64_t W, double px) {
  DT_REQUIRE(H >= 0 && W >= 0, "negative raster shape");
  DT_REQUIRE(W == 0 || H < ((1ll << 31) + W - 1) / W, "raster of 2^31 cells or more");
  DT_REQUIRE(std::isfinite(px) && px > 0.0, "px must be finite and > 0");
  return DT_OK;
}

// ---- two-phase scratch: who owns it ------------------------------------------------------------------------------
// The first phase of a multi-call op claims the scratch it leaves its state in, a later phase asks for the claim back:
// dt_scratch_reset drops it, so any scratch-using call in between makes the later phase fail instead of reading
// another op's bytes.  p2: a second region reserved beside the first (HAND's, beside flow accumulation's); in0 / in1 /
// frac_bits: what a D-infinity continuation must name again.
static void dt_scratch_claim(dt_ctx *c, DtScratchOwner owner, int64_t H, int64_t W, void *p, void *p2 = nullptr,
                             const void *in0 = nullptr, const void *in1 = nullptr, int frac_bits = 0,
                             const void *param = nullptr, int mode = 0) {
  c->claim = DtScratchClaim{owner, H, W, (char *)p, (char *)p2, {in0, in1}, frac_bits, param, mode};
}
// the claim of `owner` on a raster of w's core shape (w NULL: of any shape), with both regions when `two`; fails with
// the entry's own message
static int dt_scratch_claimed(dt_ctx *c, DtScratchOwner owner, const DtWin *w, bool two, const char *msg,
                              const DtScratchClaim **out) {
  const DtScratchClaim &k = c->claim;
  DT_REQUIRE(c->scratch && k.owner == owner && (!w || (k.h == w->H && k.w == w->W)) && (!two || k.ptr2), msg);
  *out = &k;
  return DT_OK;
}

// after a launch: what the launcher returned, then what the runtime says about the launch
static int dt_launched(int rc) {
  DT_TRY(rc);
  DT_HIP(hipGetLastError());
  return DT_OK;
}

// ---- device tier ------------------------------------------------------------------------------
// One device-tier call.  It opens on a context alone, on a context and a raster shape (checked by dt_check_hw, by
// another rule of that signature, or by dt_check_ws when a pixel size is given; w = the full window), or on a context
// and a dt_window (w = the converted window).  rc keeps the first failure: an entry opens the call with DT_DEV, which
// returns it, and checks it again after scratch().  done() closes the call after the last launch.  No state beyond
// these three members, so an entry on the scaffold runs what it ran written out by hand.
namespace {
struct DevCall {
  dt_ctx *c;
  DtWin w;
  int rc;
  explicit DevCall(dt_ctx *ctx) : c(ctx), w(), rc(open()) {}
  DevCall(dt_ctx *ctx, int64_t H, int64_t W, int (*rule)(int64_t, int64_t) = dt_check_hw) : DevCall(ctx) {
    if (rc == DT_OK) rc = rule(H, W);
    if (rc == DT_OK) w = dt_full_window(H, W);
  }
  DevCall(dt_ctx *ctx, int64_t H, int64_t W, double px) : DevCall(ctx) {
    if (rc == DT_OK) rc = dt_check_ws(H, W, px);
    if (rc == DT_OK) w = dt_full_window(H, W);
  }
  DevCall(dt_ctx *ctx, const dt_window *win) : DevCall(ctx) {
    if (rc == DT_OK) rc = dt_convert_window(win, &w);
  }
  // the context's scratch, reset (which drops any claim) and taken once; `reserve` > bytes asks for a larger block
  void *scratch(size_t bytes, size_t reserve = 0) {
    if (rc == DT_OK) rc = dt_scratch_reset(c, reserve > bytes ? reserve : bytes);
    return rc == DT_OK ? dt_scratch_take(c, bytes) : nullptr;
  }
  // two regions side by side in one reservation
  void scratch(size_t bytes, size_t bytes2, void **p, void **p2) {
    *p = scratch(bytes, bytes + bytes2 + 512);
    *p2 = rc == DT_OK ? dt_scratch_take(c, bytes2) : nullptr;
    if (rc == DT_OK && !(*p && *p2)) {
      dt_set_error("invalid argument: %s", "scratch reservation failed");
      rc = DT_EINVAL;
    }
  }
  // after the last launch (`launched`: what it returned)
  int done(int launched = DT_OK) const { return dt_launched(launched); }

 private:
  int open() const {
    DT_CTX(c);
    return DT_OK;
  }
};
}  // namespace
// opens the call `d` of an entry; its failure is the entry's
#define DT_DEV(d, ...)    \
  DevCall d(__VA_ARGS__); \
  DT_TRY(d.rc)

// Not on the scaffold, because they enqueue no kernel and would get no shorter: dt_dev_malloc, dt_dev_free, the copies,
// dt_dev_downslope_queued, the two *_accumulate_info entries (dev_countdown_info), dt_dev_membench_mix_timed and
// dt_dev_mem_info.
extern "C" int dt_dev_malloc(dt_ctx *c, int64_t bytes, void **out) {
  DT_CTX(c);
  DT_REQUIRE(out && bytes >= 0, "bad arguments");
  *out = nullptr;
  const size_t n = bytes > 0 ? (size_t)bytes : 16;
  if (hipMalloc(out, n) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    dt_host_trim();  // the host tier's cached device blocks are the only memory this library holds on to
    const hipError_t e = hipMalloc(out, n);
    if (e != hipSuccess) {
      // the runtime keeps the last error until it is read: left in place, the hipGetLastError() behind the next
      // kernel launch of ANY entry point would report this out-of-memory (placement.assign uses a full device as
      // control flow)
      (void)hipGetLastError();
      *out = nullptr;
      dt_set_error("hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? DT_ENOMEM : DT_EHIP;
    }
  }
  return dt_poison(c->stream, *out, n);
}
extern "C" int dt_dev_free(dt_ctx *c, void *p) {
  DT_CTX(c);
  if (!p) return DT_OK;
  DT_HIP(hipStreamSynchronize(c->stream));
  DT_HIP(hipFree(p));
  return DT_OK;
}
// sync: the host may read dst (or reuse src) on return; otherwise enqueue only (dt_ctx_sync before the host reads dst;
// dst should be page-locked: dt_host_alloc)
static int dev_copy(dt_ctx *c, void *dst, const void *src, int64_t bytes, hipMemcpyKind kind, bool sync) {
  DT_CTX(c);
  if (bytes <= 0) return DT_OK;
  DT_REQUIRE(dst && src, "NULL pointer");
  DT_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, kind, c->stream));
  if (sync) DT_HIP(hipStreamSynchronize(c->stream));
  return DT_OK;
}
extern "C" int dt_dev_h2d(dt_ctx *c, void *dst, const void *src, int64_t bytes) {
  return dev_copy(c, dst, src, bytes, hipMemcpyHostToDevice, true);
}
extern "C" int dt_dev_d2h(dt_ctx *c, void *dst, const void *src, int64_t bytes) {
  return dev_copy(c, dst, src, bytes, hipMemcpyDeviceToHost, true);
}
extern "C" int dt_dev_d2h_async(dt_ctx *c, void *dst, const void *src, int64_t bytes) {
  return dev_copy(c, dst, src, bytes, hipMemcpyDeviceToHost, false);
}

extern "C" int dt_dev_slope_twi(dt_ctx *c, const float *dem, const int32_t *acc32, int64_t H, int64_t W,
                                double px, double n_top, float *slope, float *slope_rad, float *ti,
                                float *mti) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && acc32 && ti && mti) || H * W == 0, "NULL raster");
  DT_TRY(dt_side_reserve(c, &c->aux, &c->aux_bytes, dt_stencil_aux_bytes(H, W)));
  return d.done(dt_launch_stencil(c->stream, d.w, dem, px, slope, nullptr, slope_rad, acc32, 0, n_top, ti, mti, c->aux));
}

static int synth_octaves(int64_t Hg, int64_t Wg) {
  int64_t m = Hg < Wg ? Hg : Wg;
  int lg = 0;
  while ((m >> (lg + 1)) > 0) lg++;
  int O = lg - 2;
  if (O < 5) O = 5;
  if (O > 14) O = 14;
  return O;
}

extern "C" int dt_dev_synth_dem(dt_ctx *c, uint32_t seed, int64_t Hg, int64_t Wg, int64_t y0,
                                int64_t x0, int64_t h, int64_t w, int nodata_pct, float *out) {
  DT_DEV(d, c);
  DT_REQUIRE(out || h * w == 0, "out is NULL");
  DT_REQUIRE(Hg > 0 && Wg > 0 && h >= 0 && w >= 0, "bad shape");
  return d.done(dt_launch_synth_dem(c->stream, seed, synth_octaves(Hg, Wg), Hg, y0, x0, h, w, nodata_pct, out));
}

extern "C" int dt_dev_slope_d8(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px,
                               float *slope, uint8_t *fdr, float *slope_rad) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE(dem || H * W == 0, "dem is NULL");
  DT_REQUIRE(slope || fdr || slope_rad, "no output requested");
  DT_TRY(dt_side_reserve(c, &c->aux, &c->aux_bytes, dt_stencil_aux_bytes(H, W)));
  return d.done(dt_launch_stencil(c->stream, d.w, dem, px, slope, fdr, slope_rad, nullptr, 0, 0.0, nullptr, nullptr,
                                  c->aux));
}

// Conditioned D8: fill depressions, D8 on the filled surface, resolve flats.  `filled` (device,
// H*W heights) receives the filled surface; info3 (host, may be NULL) = {flat cells left without a code (0), fill
// rounds, flat rounds}.  Synchronous: the fixed-point iterations read a flag back per batch of rounds.  T: float32
// heights, or a float64 DEM and filled surface, with the launcher for them.
template <typename T, typename Launch>
static int dev_condition_d8(dt_ctx *c, const T *dem, int64_t H, int64_t W, double px, T *filled, uint8_t *fdr,
                            int32_t *info3, Launch launch) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && filled) || H * W == 0, "NULL raster");
  void *scr = d.scratch(dt_hydro_scratch(H, W));
  DT_TRY(d.rc);
  int unresolved = 0, rounds[2] = {0, 0};
  DT_TRY(d.done(launch(c->stream, dem, H, W, px, filled, fdr, scr, &unresolved, rounds)));
  if (info3) {
    info3[0] = unresolved;
    info3[1] = rounds[0];
    info3[2] = rounds[1];
  }
  return DT_OK;
}
template <typename T, typename Launch>
static int dev_condition_d8_async(dt_ctx *c, const T *dem, int64_t H, int64_t W, double px, T *filled, uint8_t *fdr,
                                  int rounds, Launch launch) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && filled && fdr) || H * W == 0, "NULL raster");
  void *scr = d.scratch(dt_hydro_scratch(H, W));
  DT_TRY(d.rc);
  return d.done(launch(c->stream, dem, H, W, px, filled, fdr, scr, rounds, c->status));
}
extern "C" int dt_dev_condition_d8(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, float *filled,
                                   uint8_t *fdr, int32_t *info3) {
  return dev_condition_d8(c, dem, H, W, px, filled, fdr, info3, dt_launch_condition);
}
extern "C" int dt_dev_condition_d8_async(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, float *filled,
                                         uint8_t *fdr, int rounds) {
  return dev_condition_d8_async(c, dem, H, W, px, filled, fdr, rounds, dt_launch_condition_async);
}
extern "C" int dt_dev_condition_d8_f64(dt_ctx *c, const double *dem, int64_t H, int64_t W, double px, double *filled,
                                       uint8_t *fdr, int32_t *info3) {
  return dev_condition_d8(c, dem, H, W, px, filled, fdr, info3, dt_launch_condition_f64);
}
extern "C" int dt_dev_condition_d8_f64_async(dt_ctx *c, const double *dem, int64_t H, int64_t W, double px,
                                             double *filled, uint8_t *fdr, int rounds) {
  return dev_condition_d8_async(c, dem, H, W, px, filled, fdr, rounds, dt_launch_condition_async_f64);
}

// ... stage by stage on one rank's window.  With a byte raster `nsame` (laid out like the others, the library's between
// stage 2 and stage 4) the flat stages work from one byte per cell instead of the surface -- less traffic and LDS per
// tile visit
extern "C" int dt_dev_condition_stage_w(dt_ctx *c, const dt_window *win, int stage, int rounds, const float *dem,
                                        float *filled, uint8_t *fdr, uint32_t *dist, int32_t *flag_dev) {
  DT_DEV(d, c, win);
  return d.done(dt_launch_condition_stage(c->stream, d.w, stage, rounds, dem, filled, fdr, dist, (int *)flag_dev));
}
extern "C" int dt_dev_condition_stage_m_w(dt_ctx *c, const dt_window *win, int stage, int rounds, const float *dem,
                                          float *filled, uint8_t *fdr, uint32_t *dist, int32_t *flag_dev,
                                          uint8_t *nsame) {
  DT_DEV(d, c, win);
  DT_REQUIRE(nsame != nullptr || stage < 2, "the byte raster is missing");
  return d.done(dt_launch_condition_stage(c->stream, d.w, stage, rounds, dem, filled, fdr, dist, (int *)flag_dev, nsame));
}

// tiled flow accumulation over the call's full window, all phases (threshold / river: the river mask out of the last
// pass, 0 / NULL without)
static int dev_flowacc_tiled(DevCall &d, const uint8_t *fdr, const float *dem, int64_t threshold, int32_t *acc32,
                             int8_t *river) {
  const size_t need = dt_flowacc_tiled_scratch(d.w.H, d.w.W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  DT_TRY(dt_launch_fa_local(d.c->stream, d.w, fdr, scr, need, acc32, 0));
  return d.done(dt_launch_fa_finish(d.c->stream, d.w, fdr, dem, scr, nullptr, threshold, acc32, 0, river));
}

extern "C" int dt_dev_flowacc(dt_ctx *c, const uint8_t *fdr, const float *dem, int64_t H, int64_t W,
                              int32_t *acc32) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((fdr && acc32) || H * W == 0, "NULL raster");
  if (dt_flow_impl() != 1) return dev_flowacc_tiled(d, fdr, dem, 0, acc32, nullptr);
  // v1: one global countdown (kept for A/B runs: DT_FLOW_IMPL=v1)
  unsigned long long *state = (unsigned long long *)d.scratch((size_t)H * W * 8);
  DT_TRY(d.rc);
  return d.done(dt_launch_flowacc(c->stream, fdr, dem, H, W, state, acc32));
}

// frac_bits is bounded so that 2^frac_bits and 2^-frac_bits stay finite for every weight that can pass the bound
#define DT_FRAC_BITS_MAX 2200
extern "C" int dt_dev_flowacc_weighted(dt_ctx *c, const uint8_t *fdr, const float *dem, const double *w, int64_t H,
                                       int64_t W, int frac_bits, double *acc) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((fdr && w && acc) || H * W == 0, "NULL raster");
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  if (H * W == 0) return DT_OK;
  const size_t need = dt_flowacc_weighted_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_flowacc_weighted(c->stream, d.w, fdr, dem, w, frac_bits, scr, need, acc, c->status));
}

extern "C" int dt_dev_stream_order(dt_ctx *c, const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W,
                                   int8_t *strahler, int64_t *shreve, int64_t *link) {
  DT_DEV(d, c, H, W, dt_check_so);
  DT_REQUIRE((fdr && river && strahler) || H * W == 0, "NULL raster");
  if (H * W == 0) return DT_OK;
  const size_t need = dt_stream_order_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  int64_t m = 0;
  return d.done(dt_launch_stream_order(c->stream, fdr, river, H, W, scr, need, strahler, shreve, link,
                                       H * W >= (1ll << 31) ? &m : nullptr));
}

extern "C" int dt_dev_drainage(dt_ctx *c, const uint8_t *fdr, const float *dem, const int64_t *pour, int64_t H,
                               int64_t W, double px, int64_t *target, double *length, int64_t *label) {
  DT_DEV(d, c, H, W, px);
  DT_REQUIRE(fdr || H * W == 0, "NULL raster");
  DT_REQUIRE(!label || pour, "label requires pour");
  if (H * W == 0) return DT_OK;
  const size_t need = dt_drainage_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_drainage(c->stream, fdr, dem, pour, H, W, px, scr, need, target, length, label));
}

extern "C" int dt_dev_upslope_length(dt_ctx *c, const uint8_t *fdr, const float *dem, int64_t H, int64_t W, double px,
                                     double *length) {
  DT_DEV(d, c, H, W, px);
  DT_REQUIRE(fdr || H * W == 0, "NULL raster");
  if (H * W == 0 || !length) return DT_OK;
  const size_t need = dt_upslope_length_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_upslope_length(c->stream, fdr, dem, H, W, px, scr, need, length));
}

// flow-path extremes and the carving blend: dt_check_ws's shape rule (they take no pixel size)
static int dt_check_fp(int64_t rows, int64_t cols) { return dt_check_ws(rows, cols, 1.0); }
#define DT_FP_KIND(kind) DT_REQUIRE((kind) == 0 || (kind) == 1, "kind must be 0 (max) or 1 (min)")

extern "C" int dt_dev_flowpath_upslope(dt_ctx *c, const uint8_t *fdr, const float *dem, const float *values,
                                       int64_t rows, int64_t cols, int kind, float *value, int64_t *where) {
  DT_DEV(d, c, rows, cols, dt_check_fp);
  DT_FP_KIND(kind);
  DT_REQUIRE((fdr && values) || rows * cols == 0, "NULL raster");
  if (rows * cols == 0 || (!value && !where)) return DT_OK;
  const size_t need = dt_flowpath_scratch(rows, cols, 1);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_flowpath_upslope(c->stream, fdr, dem, values, rows, cols, kind, scr, need, value, where));
}

extern "C" int dt_dev_flowpath_downstream(dt_ctx *c, const uint8_t *fdr, const float *dem, const float *values,
                                          const uint8_t *stop, int64_t rows, int64_t cols, int kind, float *value,
                                          int64_t *where) {
  DT_DEV(d, c, rows, cols, dt_check_fp);
  DT_FP_KIND(kind);
  DT_REQUIRE((fdr && values) || rows * cols == 0, "NULL raster");
  if (rows * cols == 0 || (!value && !where)) return DT_OK;
  const size_t need = dt_flowpath_scratch(rows, cols, 0);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_flowpath_downstream(c->stream, fdr, dem, values, stop, rows, cols, kind, scr, need, value,
                                              where));
}

extern "C" int dt_dev_carve_blend(dt_ctx *c, const float *dem, const float *filled, const float *lowest, int64_t rows,
                                  int64_t cols, double max_cut, float *carved) {
  DT_DEV(d, c, rows, cols, dt_check_fp);
  DT_REQUIRE(std::isfinite(max_cut) && max_cut >= 0.0, "max_cut must be finite and >= 0");
  DT_REQUIRE((dem && filled && lowest) || rows * cols == 0, "NULL raster");
  if (rows * cols == 0 || !carved) return DT_OK;
  return d.done(dt_launch_carve_blend(c->stream, dem, filled, lowest, rows * cols, (float)max_cut, carved));
}

// weighted flow-path sums: the weights' contract and frac_bits are dt_dev_flowacc_weighted's
extern "C" int dt_dev_flowpath_downstream_sum(dt_ctx *c, const uint8_t *fdr, const float *dem, const double *w,
                                              const uint8_t *stop, int64_t rows, int64_t cols, int frac_bits,
                                              double *out) {
  DT_DEV(d, c, rows, cols, dt_check_fp);
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  DT_REQUIRE((fdr && w) || rows * cols == 0, "NULL raster");
  if (rows * cols == 0 || !out) return DT_OK;
  const size_t need = dt_pathsum_scratch(rows, cols, 0);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_pathsum_downstream(c->stream, fdr, dem, w, stop, rows, cols, frac_bits, scr, need, out,
                                             c->status));
}

extern "C" int dt_dev_flowpath_upslope_longest(dt_ctx *c, const uint8_t *fdr, const float *dem, const double *w,
                                               int64_t rows, int64_t cols, int frac_bits, double *out) {
  DT_DEV(d, c, rows, cols, dt_check_fp);
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  DT_REQUIRE((fdr && w) || rows * cols == 0, "NULL raster");
  if (rows * cols == 0 || !out) return DT_OK;
  const size_t need = dt_pathsum_scratch(rows, cols, 1);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_pathsum_longest(c->stream, fdr, dem, w, rows, cols, frac_bits, scr, need, out, c->status));
}

extern "C" int dt_dev_dinf_direction(dt_ctx *c, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                                     float *angle, float *slope) {
  DT_DEV(d, c, H, W, px);
  DT_REQUIRE((dem && angle) || H * W == 0, "NULL raster");
  if (H * W == 0) return DT_OK;
  return d.done(dt_launch_dinf_direction(c->stream, dem, fdr, H, W, px, angle, slope));
}

// ---- countdown accumulations (D-infinity, MFD; dt_countdown.h) ----
// A stack-cap knob (the launchers' stack_cap): dt_debug_set(KEY, n) when the knob has a key (KEY >= 0) and it is set,
// else the environment variable `name`, read once
template <int KEY>
static int dt_stack_cap(const char *name) {
  const int v = KEY >= 0 ? dt_debug_get(KEY) : 0;
  if (v != 0) return v;
  static int env = -1;
  if (env < 0) {
    const char *e = getenv(name);
    env = e ? atoi(e) : 0;
    if (env < 0) env = 0;
  }
  return env;
}
static int dt_dinf_stack_cap() { return dt_stack_cap<DT_DBG_DINF_STACK>("DT_DBG_DINF_STACK"); }
static int dt_mfd_stack_cap() { return dt_stack_cap<-1>("DT_DBG_MFD_STACK"); }
// info4 of the control words: queue rounds that found work, the largest window, queued, cells with >= 2 receivers
static void dt_countdown_info4(const uint32_t *ctl, int64_t *info4) {
  info4[0] = ctl[3];
  info4[1] = ctl[4];
  info4[2] = ctl[0];
  info4[3] = ctl[5];
}

// Start (rounds > 0: round 0 and rounds - 1 queue rounds) or continue (rounds < 0: -rounds queue rounds) an
// accumulation on the rasters `in` (an `raster` raster, in the messages of `entry`) and w, each time with the out step.
// launch(start, rounds, scr, need) is the op's launcher on them, `scratch` its size function.  acc: the output (of a
// routing run: any of those it writes).  param, mode: the parameter raster and the mode of a routing run, NULL and 0
// for an accumulation; a continuation names them again, so neither continues the other.
#define DT_DINF_ROUNDS_MAX 4096
template <typename Launch>
static int dev_countdown(dt_ctx *c, DtScratchOwner owner, const char *entry, const char *raster, const void *in,
                         const double *w, int64_t H, int64_t W, int frac_bits, int rounds, double *acc,
                         size_t (*scratch)(int64_t, int64_t), Launch launch, const double *param = nullptr,
                         int mode = 0) {
  DT_DEV(d, c, H, W, 1.0);
  DT_REQUIRE((in && acc) || H * W == 0, "NULL raster");
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  DT_REQUIRE(rounds != 0 && rounds >= -DT_DINF_ROUNDS_MAX && rounds <= DT_DINF_ROUNDS_MAX,
             "rounds must lie in [1, 4096] (or [-4096, -1] to continue)");
  if (H * W == 0) return DT_OK;
  const size_t need = scratch(H, W);
  if (rounds > 0) {
    void *scr = d.scratch(need);
    DT_TRY(d.rc);
    DT_TRY(launch(1, rounds - 1, scr, need));
    dt_scratch_claim(c, owner, H, W, scr, nullptr, in, w, frac_bits, param, mode);
    return d.done();
  }
  char msg[256];
  const DtScratchClaim *k;
  snprintf(msg, sizeof(msg), "%s cannot continue: no accumulation of this shape was started on this context (or "
           "another call has used the context's scratch in between)", entry);
  DT_TRY(dt_scratch_claimed(c, owner, &d.w, false, msg, &k));
  snprintf(msg, sizeof(msg), "%s continues with another %s raster, weight raster or frac_bits than it was started with",
           entry, raster);
  DT_REQUIRE(k->in[0] == in && k->in[1] == w && k->frac_bits == frac_bits, msg);
  snprintf(msg, sizeof(msg), "%s continues with another parameter raster or mode than it was started with (a routing "
           "run and an accumulation do not continue each other)", entry);
  DT_REQUIRE(k->param == param && k->mode == mode, msg);
  return d.done(launch(0, -rounds, k->ptr, need));
}
// info4 of the `name` accumulation last enqueued on the context, from its control words (synchronises)
static int dev_countdown_info(dt_ctx *c, DtScratchOwner owner, const char *name,
                              const uint32_t *(*ctl_of)(void *, int64_t, int64_t), int64_t *info4) {
  DT_CTX(c);
  DT_REQUIRE(info4 != nullptr, "info4 is NULL");
  char msg[128];
  const DtScratchClaim *k;
  snprintf(msg, sizeof(msg), "no %s accumulation on this context (or another call has used the context's scratch "
           "since)", name);
  DT_TRY(dt_scratch_claimed(c, owner, nullptr, false, msg, &k));
  uint32_t ctl[8];
  DT_HIP(hipMemcpyAsync(ctl, ctl_of(k->ptr, k->h, k->w), sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
  DT_HIP(hipStreamSynchronize(c->stream));
  dt_countdown_info4(ctl, info4);
  return DT_OK;
}

extern "C" int dt_dev_dinf_accumulate(dt_ctx *c, const float *angle, const double *w, int64_t H, int64_t W,
                                      int frac_bits, int rounds, double *acc) {
  return dev_countdown(c, DT_OWNER_DINF, "dt_dev_dinf_accumulate", "angle", angle, w, H, W, frac_bits, rounds, acc,
                       dt_dinf_accumulate_scratch, [&](int start, int n, void *scr, size_t need) {
                         return dt_launch_dinf_accumulate(c->stream, angle, w, H, W, frac_bits, start, n, 1,
                                                          dt_dinf_stack_cap(), scr, need, acc, c->status);
                       });
}
// What the two routing entries refuse before dev_countdown takes over: a mode that is none, and on a raster with cells
// a NULL parameter raster, no output at all, an output that is an input or that is named twice.  *any: an output.
static int dt_check_route(int64_t H, int64_t W, const void *in, const double *w, const double *param, int mode,
                          double *const (&out)[4], double **any) {
  DT_REQUIRE(mode == DT_ROUTE_DECAY || mode == DT_ROUTE_RETAIN || mode == DT_ROUTE_LIMIT,
             "mode must be DT_ROUTE_DECAY, DT_ROUTE_RETAIN or DT_ROUTE_LIMIT");
  *any = nullptr;
  if (H <= 0 || W <= 0) return DT_OK;  // dev_countdown's checks say the rest
  DT_REQUIRE(param != nullptr, "param is NULL");
  for (int i = 0; i < 4; i++) {
    if (!out[i]) continue;
    *any = out[i];
    DT_REQUIRE((const void *)out[i] != in && out[i] != w && out[i] != param, "an output raster is one of the inputs");
    for (int j = 0; j < i; j++) DT_REQUIRE(out[j] != out[i], "two outputs are the same raster");
  }
  DT_REQUIRE(*any != nullptr, "all four outputs are NULL");
  return DT_OK;
}
extern "C" int dt_dev_dinf_route(dt_ctx *c, const float *angle, const double *w, const double *param, int64_t H,
                                 int64_t W, int frac_bits, int mode, int rounds, double *inflow, double *load,
                                 double *outflow, double *retained) {
  DT_CTX(c);
  double *const out[4] = {inflow, load, outflow, retained};
  double *any;
  DT_TRY(dt_check_route(H, W, angle, w, param, mode, out, &any));
  return dev_countdown(c, DT_OWNER_DINF, "dt_dev_dinf_route", "angle", angle, w, H, W, frac_bits, rounds, any,
                       dt_dinf_accumulate_scratch, [&](int start, int n, void *scr, size_t need) {
                         return dt_launch_dinf_route(c->stream, angle, w, param, H, W, frac_bits, mode, start, n, 1,
                                                     dt_dinf_stack_cap(), scr, need, inflow, load, outflow, retained,
                                                     c->status);
                       }, param, mode);
}
extern "C" int dt_dev_dinf_accumulate_info(dt_ctx *c, int64_t *info4) {
  return dev_countdown_info(c, DT_OWNER_DINF, "D-infinity", dt_dinf_accumulate_ctl, info4);
}

extern "C" int dt_dev_cost_distance(dt_ctx *c, const float *friction, const int8_t *sources, int64_t H, int64_t W,
                                    double px, int connectivity, int visit_limit, int rounds, double *cost,
                                    int64_t *indices, uint8_t *backlink) {
  DT_DEV(d, c, H, W, px);
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity is 4 or 8");
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  DT_REQUIRE(rounds >= 1 && rounds <= DT_TILE_ROUNDS_MAX, "rounds must lie in [1, 4096]");
  DT_REQUIRE((friction && sources && cost) || H * W == 0, "NULL raster");
  if (H * W == 0) return DT_OK;
  const size_t need = dt_cost_distance_scratch(H, W, indices != nullptr);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_cost_distance(c->stream, friction, sources, H, W, px, connectivity, visit_limit, 1, rounds, 1,
                                        scr, need, cost, indices, backlink, c->status));
}

// SAGA wetness index: what both tiers require of the suction's parameters; `index`: the offset and the minimum must
// not both be zero (tan b > 0)
static int dt_check_wetness(double t, double weight, double offset, double minimum, bool suction, bool index) {
  if (suction) {
    DT_REQUIRE(std::isfinite(t) && t > 1.0, "t must be finite and > 1");
    DT_REQUIRE(std::isfinite(weight) && weight > 0.0, "slope_weight must be finite and > 0");
  }
  DT_REQUIRE(std::isfinite(offset) && offset >= 0.0, "slope_offset must be finite and >= 0");
  DT_REQUIRE(std::isfinite(minimum) && minimum >= 0.0, "slope_min must be finite and >= 0");
  DT_REQUIRE(!index || offset + minimum > 0.0, "slope_offset and slope_min must not both be 0");
  return DT_OK;
}

extern "C" int dt_dev_wetness_suction(dt_ctx *c, const float *slope, int64_t H, int64_t W, double t, double weight,
                                      double offset, double minimum, float *suction) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_wetness(t, weight, offset, minimum, true, false));
  DT_REQUIRE((slope && suction) || H * W == 0, "NULL raster");
  return d.done(dt_launch_wetness_suction(c->stream, slope, H * W, std::log(t), weight, offset, minimum, suction));
}

extern "C" int dt_dev_wetness_modified_area(dt_ctx *c, const double *area, const float *suction, int64_t H, int64_t W,
                                            int visit_limit, int rounds, double *modified) {
  DT_DEV(d, c, H, W, 1.0);
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  DT_REQUIRE(rounds >= 1 && rounds <= DT_TILE_ROUNDS_MAX, "rounds must lie in [1, 4096]");
  DT_REQUIRE((area && suction && modified) || H * W == 0, "NULL raster");
  if (H * W == 0) return DT_OK;
  const size_t need = dt_wetness_scratch(H, W, 0, 0);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_wetness_area(c->stream, area, suction, H, W, visit_limit, 1, rounds, 1, scr, need, modified,
                                       c->status));
}

extern "C" int dt_dev_wetness_index(dt_ctx *c, const double *modified, const float *slope, int64_t H, int64_t W,
                                    double offset, double minimum, float *swi) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_wetness(0.0, 0.0, offset, minimum, false, true));
  DT_REQUIRE((modified && slope && swi) || H * W == 0, "NULL raster");
  return d.done(dt_launch_wetness_index(c->stream, modified, slope, H * W, offset, minimum, swi));
}

// resampling: the two rasters have shapes of their own, so the call opens on the context alone and
// dt_check_resample holds the shape rules
extern "C" int dt_dev_resample(dt_ctx *c, const void *src, int dtype, int64_t Hs, int64_t Ws, const double *matrix,
                               int method, int64_t nodata, uint64_t fill_bits, void *dst, int64_t Hd, int64_t Wd) {
  DT_DEV(d, c);
  DT_TRY(dt_check_resample(dtype, Hs, Ws, matrix, method, nodata, Hd, Wd));
  DT_REQUIRE(src && dst, "NULL raster");
  return d.done(dt_launch_resample(c->stream, src, dtype, Hs, Ws, matrix, method, nodata, fill_bits, dst, Hd, Wd));
}

// vector rasterisation: the geometry has a length of its own, so the call opens on the context alone and
// dt_check_rasterize holds the rules; `capacity` crossing slots of scratch, which the kernels never write past
static int dev_rasterize(dt_ctx *c, int kind, const double *coords, const int64_t *parts, const int32_t *ids, int64_t P,
                         int64_t N, int64_t H, int64_t W, int connectivity, int all_touched, int64_t capacity,
                         int32_t *label, int64_t *info, hipEvent_t *ev) {
  DT_DEV(d, c);
  DT_TRY(dt_check_rasterize(kind, P, N, H, W, connectivity, all_touched, capacity));
  DT_REQUIRE(label && info, "NULL label or info");
  DT_REQUIRE((coords && parts && ids) || P == 0 || N == 0, "NULL geometry");
  const size_t need = dt_rasterize_scratch(H, capacity);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  DT_REQUIRE(scr, "scratch reservation failed");
  return d.done(dt_launch_rasterize(c->stream, kind, coords, parts, ids, P, N, H, W, connectivity, all_touched, capacity,
                                    scr, need, label, info, ev));
}
extern "C" int dt_dev_rasterize(dt_ctx *c, int kind, const double *coords, const int64_t *parts, const int32_t *ids,
                                int64_t P, int64_t N, int64_t H, int64_t W, int connectivity, int all_touched,
                                int64_t capacity, int32_t *label, int64_t *info) {
  return dev_rasterize(c, kind, coords, parts, ids, P, N, H, W, connectivity, all_touched, capacity, label, info,
                       nullptr);
}
// the same call between events, then a synchronisation: phase_ms[7] = the device time of clear, count, scan, emit,
// sort, fill and lines / points, written only when the call succeeds (tools/vector_bench.py)
extern "C" int dt_dev_rasterize_timed(dt_ctx *c, int kind, const double *coords, const int64_t *parts,
                                      const int32_t *ids, int64_t P, int64_t N, int64_t H, int64_t W, int connectivity,
                                      int all_touched, int64_t capacity, int32_t *label, int64_t *info,
                                      double *phase_ms) {
  DT_CTX(c);
  DT_REQUIRE(phase_ms, "phase_ms is NULL");
  hipEvent_t ev[8] = {};
  int rc = DT_OK;
  for (int k = 0; k < 8 && rc == DT_OK; k++)
    if (hipEventCreate(&ev[k]) != hipSuccess) {
      dt_set_error("hipEventCreate failed: %s", hipGetErrorString(hipGetLastError()));
      rc = DT_EHIP;
    }
  if (rc == DT_OK)
    rc = dev_rasterize(c, kind, coords, parts, ids, P, N, H, W, connectivity, all_touched, capacity, label, info, ev);
  float t[7] = {};
  if (rc == DT_OK) {
    if (hipEventSynchronize(ev[7]) != hipSuccess) rc = DT_EHIP;
    for (int k = 0; k < 7 && rc == DT_OK; k++)
      if (hipEventElapsedTime(&t[k], ev[k], ev[k + 1]) != hipSuccess) rc = DT_EHIP;
    if (rc != DT_OK) dt_set_error("event timing failed: %s", hipGetErrorString(hipGetLastError()));
  }
  for (int k = 0; k < 8; k++)
    if (ev[k]) (void)hipEventDestroy(ev[k]);
  if (rc == DT_OK)
    for (int k = 0; k < 7; k++) phase_ms[k] = (double)t[k];
  return rc;
}

// polygonisation: the rings have lengths of their own, so the call opens on the context alone and dt_check_polygonize
// holds the rules; the scratch is sized by cap_edges, which the kernels never write past.  count_only: the count phase
// alone, info[0] = edges and info[1] = corners (the host entries size their calls with it)
static int dev_polygonize(dt_ctx *c, const int32_t *labels, int64_t H, int64_t W, int64_t cap_edges,
                          int64_t cap_vertices, int64_t cap_rings, int count_only, double *coords, int64_t *parts,
                          int32_t *ids, int32_t *shell, int64_t *info, hipEvent_t *ev) {
  DT_DEV(d, c);
  DT_TRY(dt_check_polygonize(H, W, cap_edges, cap_vertices, cap_rings));
  DT_REQUIRE(labels, "NULL labels");
  DT_REQUIRE(info && (count_only || (coords && parts && ids && shell)), "NULL coords, parts, ids, shell or info");
  const size_t need = dt_polygonize_scratch(H, W, cap_edges, count_only);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  DT_REQUIRE(scr, "scratch reservation failed");
  return d.done(dt_launch_polygonize(c->stream, labels, H, W, cap_edges, cap_vertices, cap_rings, count_only, scr, need,
                                     coords, parts, ids, shell, info, ev));
}
extern "C" int dt_dev_polygonize(dt_ctx *c, const int32_t *labels, int64_t H, int64_t W, int64_t cap_edges,
                                 int64_t cap_vertices, int64_t cap_rings, double *coords, int64_t *parts, int32_t *ids,
                                 int32_t *shell, int64_t *info) {
  return dev_polygonize(c, labels, H, W, cap_edges, cap_vertices, cap_rings, 0, coords, parts, ids, shell, info, nullptr);
}
// the same call between events, then a synchronisation: phase_ms[7] = the device time of count, link, leaders, ranks,
// rings, emit and shells, written only when the call succeeds (tools/vector_bench.py)
extern "C" int dt_dev_polygonize_timed(dt_ctx *c, const int32_t *labels, int64_t H, int64_t W, int64_t cap_edges,
                                       int64_t cap_vertices, int64_t cap_rings, double *coords, int64_t *parts,
                                       int32_t *ids, int32_t *shell, int64_t *info, double *phase_ms) {
  DT_CTX(c);
  DT_REQUIRE(phase_ms, "phase_ms is NULL");
  hipEvent_t ev[8] = {};
  int rc = DT_OK;
  for (int k = 0; k < 8 && rc == DT_OK; k++)
    if (hipEventCreate(&ev[k]) != hipSuccess) {
      dt_set_error("hipEventCreate failed: %s", hipGetErrorString(hipGetLastError()));
      rc = DT_EHIP;
    }
  if (rc == DT_OK)
    rc = dev_polygonize(c, labels, H, W, cap_edges, cap_vertices, cap_rings, 0, coords, parts, ids, shell, info, ev);
  float t[7] = {};
  if (rc == DT_OK) {
    if (hipEventSynchronize(ev[7]) != hipSuccess) rc = DT_EHIP;
    for (int k = 0; k < 7 && rc == DT_OK; k++)
      if (hipEventElapsedTime(&t[k], ev[k], ev[k + 1]) != hipSuccess) rc = DT_EHIP;
    if (rc != DT_OK) dt_set_error("event timing failed: %s", hipGetErrorString(hipGetLastError()));
  }
  for (int k = 0; k < 8; k++)
    if (ev[k]) (void)hipEventDestroy(ev[k]);
  if (rc == DT_OK)
    for (int k = 0; k < 7; k++) phase_ms[k] = (double)t[k];
  return rc;
}

// geodesic reconstruction: what both tiers require of the marker mode and its parameters
static int dt_check_morph(int mode, int erosion, int connectivity, double h, int radius, int visit_limit) {
  DT_REQUIRE(mode >= DT_MORPH_MARKER && mode <= DT_MORPH_WINDOW, "mode must be one of DT_MORPH_*");
  DT_REQUIRE(erosion == 0 || erosion == 1, "erosion is 0 or 1");
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
  DT_REQUIRE(mode != DT_MORPH_SHIFT || (std::isfinite(h) && h > 0.0), "h must be finite and > 0");
  DT_REQUIRE(mode != DT_MORPH_WINDOW || (radius >= 1 && radius <= DT_FILTER_RADIUS_MAX), "radius must lie in [1, 4096]");
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  return DT_OK;
}
// ... and of the rasters of a call with cells
static int dt_check_morph_rasters(int mode, const float *mask, const float *marker, const float *out,
                                  const uint8_t *out8) {
  DT_REQUIRE((out != nullptr) != (out8 != nullptr), "exactly one of out and out8 is given");
  DT_REQUIRE(mask && (mode != DT_MORPH_MARKER || marker), "NULL raster");
  DT_REQUIRE(!out || (out != mask && out != marker), "out must be neither mask nor marker");
  return DT_OK;
}

extern "C" int dt_dev_morph_reconstruct(dt_ctx *c, int mode, int erosion, int connectivity, const float *mask,
                                        const float *marker, const uint8_t *seeds, double h, int radius, int64_t H,
                                        int64_t W, int visit_limit, int rounds, float *out, uint8_t *out8) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_morph(mode, erosion, connectivity, h, radius, visit_limit));
  DT_REQUIRE(rounds >= 1 && rounds <= DT_TILE_ROUNDS_MAX, "rounds must lie in [1, 4096]");
  if (H * W == 0) return DT_OK;
  DT_TRY(dt_check_morph_rasters(mode, mask, marker, out, out8));
  const size_t need = dt_morph_scratch(H, W, mode, out8 != nullptr);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_morph(c->stream, mode, erosion, connectivity, mask, marker, seeds, h, radius, H, W,
                                visit_limit, 1, rounds, 1, scr, need, out, out8, c->status));
}

// harmonic interpolation: the shape rule of dt_check_ws, and what both tiers require of tol and the budget
static int dt_check_harmonic(double tol, int max_rounds) {
  DT_REQUIRE(std::isfinite(tol) && tol > 0.0, "tol must be finite and > 0");
  DT_REQUIRE(max_rounds >= 1 && max_rounds <= DT_TILE_ROUNDS_MAX, "max_rounds must lie in [1, 4096]");
  return DT_OK;
}
// DT_DBG_HARMONIC_LEVELS=n (n >= 1): the pyramid has n levels at most (benchmarks; 0: as many as the raster needs)
static int dt_harmonic_level_cap() {
  const char *e = getenv("DT_DBG_HARMONIC_LEVELS");
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : 0;
}
extern "C" int dt_dev_harmonic(dt_ctx *c, const float *values, const int8_t *fixed, const int8_t *domain, int64_t rows,
                               int64_t cols, double tol, int max_rounds, double *out, int64_t *info) {
  DT_DEV(d, c, rows, cols, dt_check_fp);
  DT_TRY(dt_check_harmonic(tol, max_rounds));
  DT_REQUIRE((values && fixed && out) || rows * cols == 0, "NULL raster");
  if (rows * cols == 0) return DT_OK;
  const int cap = dt_harmonic_level_cap();
  const size_t need = dt_harmonic_scratch(rows, cols, max_rounds, cap);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  DT_TRY(dt_launch_harmonic_setup(c->stream, values, fixed, domain, rows, cols, max_rounds, cap, scr, need, out));
  for (int l = dt_harmonic_levels(rows, cols, cap) - 1; l >= 0; l--) {
    DT_TRY(dt_launch_harmonic_rounds(c->stream, rows, cols, max_rounds, cap, l, 0, max_rounds, tol, scr, need, out));
    if (l) DT_TRY(dt_launch_harmonic_prolong(c->stream, rows, cols, max_rounds, cap, l, scr, need, out));
  }
  return d.done(dt_launch_harmonic_finish(c->stream, rows, cols, max_rounds, cap, tol, scr, need, info, c->status));
}

// flood inundation: what both tiers require of the scalars (the shape rule is dt_check_ws's, with px), and the call's
// description for the launchers
static int dt_check_inundation(const double *par, const float *manning, const float *rain, int boundary, int K, int T,
                               int64_t steps0) {
  DT_REQUIRE(par, "NULL parameters");
  const double *p = par;
  DT_REQUIRE(std::isfinite(p[1]) && p[1] >= 0.0, "t0 must be finite and >= 0");
  DT_REQUIRE(std::isfinite(p[2]) && p[2] > 0.0, "t_end must be finite and > 0");
  DT_REQUIRE(manning || (std::isfinite(p[3]) && p[3] > 0.0), "manning must be finite and > 0");
  DT_REQUIRE(rain || (std::isfinite(p[4]) && p[4] >= 0.0), "rain must be finite and >= 0");
  DT_REQUIRE(std::isfinite(p[5]) && p[5] > 0.0 && p[5] <= 1.0, "alpha must lie in (0, 1]");
  DT_REQUIRE(std::isfinite(p[6]) && p[6] > 0.0, "dt_max must be finite and > 0");
  DT_REQUIRE(std::isfinite(p[7]) && p[7] >= 0.0, "dry must be finite and >= 0");
  DT_REQUIRE(std::isfinite(p[8]) && p[8] > 0.0, "boundary_slope must be finite and > 0");
  DT_REQUIRE(std::isfinite(p[9]) && p[9] >= 0.0, "arrival_depth must be finite and >= 0");
  DT_REQUIRE(boundary == 0 || boundary == 1, "boundary is 0 (closed) or 1 (open)");
  DT_REQUIRE(K >= 0 && K <= DT_INUNDATION_INFLOW_MAX, "inflow cells must number 0 to 4096");
  DT_REQUIRE(K == 0 || (T >= 1 && T <= (1 << 20)), "inflow times must number 1 to 2^20");
  DT_REQUIRE(steps0 >= 0, "steps0 is negative");
  return DT_OK;
}
static DtInundation dt_inundation_call(const float *z, const float *manning, const float *rain, int64_t H, int64_t W,
                                       const double *p, int boundary, const int64_t *cells, const double *times,
                                       const double *discharge, int K, int T, int64_t max_steps, double *h, double *qx,
                                       double *qy, double *max_depth, double *arrival) {
  DtInundation d;
  d.z = z; d.manning = manning; d.rain = rain;
  d.H = H; d.W = W;
  d.px = p[0]; d.t_end = p[2]; d.n = p[3]; d.rain_s = p[4]; d.alpha = p[5]; d.dt_max = p[6]; d.dry = p[7];
  d.slope = p[8]; d.arrival_depth = p[9];
  d.open = boundary;
  d.cells = cells; d.times = times; d.discharge = discharge;
  d.K = K; d.T = K ? T : 0;
  d.max_steps = max_steps;
  d.h = h; d.qx = qx; d.qy = qy; d.max_depth = max_depth; d.arrival = arrival;
  return d;
}
extern "C" int dt_dev_inundation(dt_ctx *c, const float *z, const float *manning, const float *rain, int64_t rows,
                                 int64_t cols, const double *par, int boundary, const int64_t *cells,
                                 const double *times, const double *discharge, int K, int T, int64_t steps0,
                                 int64_t max_steps, double *h, double *qx, double *qy, double *max_depth,
                                 double *arrival, int64_t *info) {
  DT_DEV(d, c, rows, cols, par ? par[0] : 0.0);
  DT_TRY(dt_check_inundation(par, manning, rain, boundary, K, T, steps0));
  DT_REQUIRE(max_steps >= 0 && max_steps <= DT_INUNDATION_DEV_STEPS_MAX, "max_steps must lie in [0, 2^20]");
  DT_REQUIRE((z && h && qx && qy) || rows * cols == 0, "NULL raster");
  DT_REQUIRE(K == 0 || (cells && times && discharge), "NULL inflow table");
  if (rows * cols == 0) return DT_OK;
  const size_t need = dt_inundation_scratch(rows, cols);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  const DtInundation call = dt_inundation_call(z, manning, rain, rows, cols, par, boundary, cells, times, discharge, K,
                                               T, max_steps, h, qx, qy, max_depth, arrival);
  DT_TRY(dt_launch_inundation_begin(c->stream, call, par[1], steps0, scr, need));
  DT_TRY(dt_launch_inundation_steps(c->stream, call, (int)max_steps, scr, need));
  return d.done(dt_launch_inundation_finish(c->stream, call, scr, need, info));
}

static int dt_check_mfd_exponent(double exponent) {
  DT_REQUIRE(std::isfinite(exponent) && exponent >= 0.0 && exponent <= 64.0, "exponent must be finite and in [0, 64]");
  return DT_OK;
}
extern "C" int dt_dev_mfd_shares(dt_ctx *c, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double exponent,
                                 int contour, uint16_t *shares) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_mfd_exponent(exponent));
  DT_REQUIRE((dem && shares) || H * W == 0, "NULL raster");
  if (H * W == 0) return DT_OK;
  return d.done(dt_launch_mfd_shares(c->stream, dem, fdr, H, W, exponent, contour, shares));
}

extern "C" int dt_dev_mfd_accumulate(dt_ctx *c, const uint16_t *shares, const double *w, int64_t H, int64_t W,
                                     int frac_bits, int rounds, double *acc) {
  return dev_countdown(c, DT_OWNER_MFD, "dt_dev_mfd_accumulate", "share", shares, w, H, W, frac_bits, rounds, acc,
                       dt_mfd_accumulate_scratch, [&](int start, int n, void *scr, size_t need) {
                         return dt_launch_mfd_accumulate(c->stream, shares, w, H, W, frac_bits, start, n, 1,
                                                         dt_mfd_stack_cap(), scr, need, acc, c->status);
                       });
}
extern "C" int dt_dev_mfd_route(dt_ctx *c, const uint16_t *shares, const double *w, const double *param, int64_t H,
                                int64_t W, int frac_bits, int mode, int rounds, double *inflow, double *load,
                                double *outflow, double *retained) {
  DT_CTX(c);
  double *const out[4] = {inflow, load, outflow, retained};
  double *any;
  DT_TRY(dt_check_route(H, W, shares, w, param, mode, out, &any));
  return dev_countdown(c, DT_OWNER_MFD, "dt_dev_mfd_route", "share", shares, w, H, W, frac_bits, rounds, any,
                       dt_mfd_accumulate_scratch, [&](int start, int n, void *scr, size_t need) {
                         return dt_launch_mfd_route(c->stream, shares, w, param, H, W, frac_bits, mode, start, n, 1,
                                                    dt_mfd_stack_cap(), scr, need, inflow, load, outflow, retained,
                                                    c->status);
                       }, param, mode);
}
extern "C" int dt_dev_mfd_accumulate_info(dt_ctx *c, int64_t *info4) {
  return dev_countdown_info(c, DT_OWNER_MFD, "MFD", dt_mfd_accumulate_ctl, info4);
}

static int dt_check_terrain(int radius, double sx, double sy, double sz) {
  DT_REQUIRE(radius >= 1 && radius <= DT_TERRAIN_RADIUS_MAX, "radius must lie in [1, 32]");
  DT_REQUIRE(std::isfinite(sx) && std::isfinite(sy) && std::isfinite(sz), "the sun vector must be finite");
  return DT_OK;
}
extern "C" int dt_dev_terrain(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, int radius, double sx,
                              double sy, double sz, float *gradient, float *aspect, float *profile, float *plan,
                              float *tangential, float *mean, float *laplacian, float *hillshade) {
  DT_DEV(d, c, H, W, px);
  DT_TRY(dt_check_terrain(radius, sx, sy, sz));
  if (H * W == 0) return DT_OK;
  float *const out[DT_TERRAIN_OUTPUTS] = {gradient, aspect, profile, plan, tangential, mean, laplacian, hillshade};
  bool any = false;
  for (float *o : out) any = any || o != nullptr;
  DT_REQUIRE(any, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  return d.done(dt_launch_terrain(c->stream, dem, H, W, px, radius, sx, sy, sz, out));
}

// focal statistics (dt_focal.hip): the radius table, frac_bits, origin, and which outputs go with how many radii
static int dt_check_focal(double origin, int frac_bits, const int32_t *radii, int n_radii, bool stats, bool any) {
  DT_REQUIRE(n_radii >= 1 && n_radii <= DT_FOCAL_RADII_MAX && radii, "1..32 radii per call");
  for (int k = 0; k < n_radii; k++) {
    DT_REQUIRE(radii[k] >= 1 && radii[k] <= DT_FOCAL_RADIUS_MAX, "a radius must lie in [1, 4096]");
    DT_REQUIRE(k == 0 || radii[k] > radii[k - 1], "radii must be strictly increasing");
  }
  DT_REQUIRE(frac_bits >= 0 && frac_bits <= DT_FOCAL_FRAC_BITS_MAX, "frac_bits must lie in [0, 24]");
  DT_REQUIRE(std::isfinite(origin), "origin must be finite");
  DT_REQUIRE(n_radii == 1 || !stats, "with more than one radius only dev and scale are defined");
  DT_REQUIRE(any, "no output raster");
  return DT_OK;
}
extern "C" int dt_dev_focal(dt_ctx *c, const float *dem, int64_t H, int64_t W, double origin, int frac_bits,
                            const int32_t *radii, int n_radii, int32_t *count, float *mean, float *std_, float *tpi,
                            float *dev, uint16_t *scale) {
  DT_DEV(d, c, H, W, 1.0);
  const bool stats = count || mean || std_ || tpi;
  DT_TRY(dt_check_focal(origin, frac_bits, radii, n_radii, stats, stats || dev || scale));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(dem, "NULL raster");
  const size_t need = dt_focal_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_focal(c->stream, dem, H, W, origin, frac_bits, radii, n_radii, scr, need, count, mean, std_,
                                tpi, dev, scale, c->status));
}

// DEM filters (dt_filters.hip): the radius of the extremes; the radius and the rank table of the rank filter; the
// radius, threshold cosine, iterations and largest change of the denoising
static int dt_check_filter_extremes(int radius) {
  DT_REQUIRE(radius >= 1 && radius <= DT_FILTER_RADIUS_MAX, "radius must lie in [1, 4096]");
  return DT_OK;
}
static int dt_check_filter_rank(int radius, const uint16_t *table, int n_table) {
  DT_REQUIRE(radius >= 1 && radius <= DT_FILTER_RANK_RADIUS_MAX, "radius must lie in [1, 16]");
  const int cells = (2 * radius + 1) * (2 * radius + 1);
  DT_REQUIRE(table && n_table == cells + 1, "the rank table must hold (2 radius + 1)^2 + 1 entries");
  for (int n = 0; n <= cells; n++) DT_REQUIRE((int)table[n] < (n > 1 ? n : 1), "rank table: k[n] must be below n");
  return DT_OK;
}
static int dt_check_filter_denoise(int radius, double cos_threshold, int iterations, double max_change) {
  DT_REQUIRE(radius >= 1 && radius <= DT_FILTER_DENOISE_RADIUS_MAX, "radius must lie in [1, 16]");
  DT_REQUIRE(cos_threshold > 0.0 && cos_threshold < 1.0, "cos_threshold must lie in (0, 1)");
  DT_REQUIRE(iterations >= 1 && iterations <= DT_FILTER_DENOISE_ITERATIONS_MAX, "iterations must lie in [1, 32]");
  DT_REQUIRE(std::isfinite(max_change) && max_change > 0.0, "max_change must be finite and > 0");
  return DT_OK;
}
extern "C" int dt_dev_filter_extremes(dt_ctx *c, const float *dem, int64_t H, int64_t W, int radius, float *minimum,
                                      float *maximum, float *range, float *opening, float *closing) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_filter_extremes(radius));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(minimum || maximum || range || opening || closing, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const size_t need = dt_filter_extremes_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_filter_extremes(c->stream, dem, H, W, radius, scr, need, minimum, maximum, range, opening,
                                          closing));
}
extern "C" int dt_dev_filter_rank(dt_ctx *c, const float *dem, int64_t H, int64_t W, int radius, const uint16_t *table,
                                  int n_table, float *out) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_filter_rank(radius, table, n_table));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(out, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  return d.done(dt_launch_filter_rank(c->stream, dem, H, W, radius, table, n_table, out));
}
extern "C" int dt_dev_filter_denoise(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, int radius,
                                     double cos_threshold, int iterations, double max_change, float *out) {
  DT_DEV(d, c, H, W, px);
  DT_TRY(dt_check_filter_denoise(radius, cos_threshold, iterations, max_change));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(out, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  DT_REQUIRE(out != dem, "out must not be dem");
  const size_t need = dt_filter_denoise_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_filter_denoise(c->stream, dem, H, W, px, radius, cos_threshold, iterations, max_change, scr,
                                         need, out));
}

// lines of sight (dt_horizon.hip): the ranges of radius, skip and the flatness tangent
static int dt_check_horizon(int radius, int skip, double flat_tan) {
  DT_REQUIRE(radius >= 1 && radius <= DT_HORIZON_RADIUS_MAX, "radius must lie in [1, 64]");
  DT_REQUIRE(skip >= 0 && skip < radius, "skip must lie in [0, radius - 1]");
  DT_REQUIRE(std::isfinite(flat_tan) && flat_tan >= 0.0, "flat_tan must be finite and >= 0");
  return DT_OK;
}
extern "C" int dt_dev_horizon(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, int radius, int skip,
                              double flat_tan, uint8_t *landform, uint16_t *pattern, float *positive, float *negative,
                              float *sky_view) {
  DT_DEV(d, c, H, W, px);
  DT_TRY(dt_check_horizon(radius, skip, flat_tan));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(landform || pattern || positive || negative || sky_view, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  return d.done(dt_launch_horizon(c->stream, dem, H, W, px, radius, skip, flat_tan, landform, pattern, positive,
                                  negative, sky_view));
}

// valley bottom / ridge top flatness (dt_mrvbf.hip): the ranges of the thresholds, the levels and the exponent table
static int dt_check_mrvbf(double slope_threshold, int levels, double pctl_valley, double pctl_ridge, const double *p) {
  DT_REQUIRE(std::isfinite(slope_threshold) && slope_threshold > 0.0, "slope_threshold must be finite and > 0");
  DT_REQUIRE(levels >= 2 && levels <= DT_MRVBF_LEVELS_MAX, "levels must lie in [2, 10]");
  DT_REQUIRE(pctl_valley > 0.0 && pctl_valley <= 1.0 && pctl_ridge > 0.0 && pctl_ridge <= 1.0,
             "pctl_valley and pctl_ridge must lie in (0, 1]");
  DT_REQUIRE(p, "the exponent table is NULL");
  for (int k = 0; k < levels - 1; k++) {
    DT_REQUIRE(std::isfinite(p[k]) && p[k] > 0.0, "an exponent must be finite and > 0");
  }
  return DT_OK;
}
extern "C" int dt_dev_mrvbf(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, double slope_threshold,
                            int levels, double pctl_valley, double pctl_ridge, const double *p, float *mrvbf,
                            float *mrrtf) {
  DT_DEV(d, c, H, W, px);
  DT_TRY(dt_check_mrvbf(slope_threshold, levels, pctl_valley, pctl_ridge, p));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(mrvbf || mrrtf, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const size_t need = dt_mrvbf_scratch(H, W, levels);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_mrvbf(c->stream, dem, H, W, px, slope_threshold, levels, pctl_valley, pctl_ridge, p, scr,
                                need, mrvbf, mrrtf));
}
static int dt_check_percentile(int radius) {
  DT_REQUIRE(radius >= 1 && radius <= DT_PERCENTILE_RADIUS_MAX, "radius must lie in [1, 16]");
  return DT_OK;
}
extern "C" int dt_dev_percentile(dt_ctx *c, const float *dem, int64_t H, int64_t W, int radius, float *lower,
                                 float *higher) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_percentile(radius));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(lower || higher, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  return d.done(dt_launch_percentile(c->stream, dem, H, W, radius, lower, higher));
}
static int dt_check_coarsen(const double *g6) {
  DT_REQUIRE(g6, "the Gaussian weights are NULL");
  for (int k = 0; k < 6; k++) {
    DT_REQUIRE(std::isfinite(g6[k]) && g6[k] > 0.0, "a Gaussian weight must be finite and > 0");
  }
  return DT_OK;
}
extern "C" int dt_dev_coarsen(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, const double *g6,
                              float *dem3, float *slope3) {
  DT_DEV(d, c, H, W, px);
  DT_TRY(dt_check_coarsen(g6));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(dem && dem3 && slope3, "NULL raster");
  return d.done(dt_launch_coarsen(c->stream, dem, H, W, px, g6, dem3, slope3));
}

// reaches: reach ids and flat indices travel in 31 bits
static int dt_check_reach_count(int64_t R) {
  DT_REQUIRE(R >= 0 && R < (1ll << 31), "the number of reaches must lie in [0, 2^31)");
  return DT_OK;
}

extern "C" int dt_dev_reach_catchments(dt_ctx *c, const int64_t *link, const void *idx, int idx_bytes, int64_t H,
                                       int64_t W, int32_t *reach, int32_t *catch_, int64_t *heads, int64_t cap,
                                       int64_t *n_reaches) {
  DT_DEV(d, c, H, W);
  const int64_t N = H * W;
  DT_REQUIRE(link || N == 0, "NULL raster");
  DT_REQUIRE(!catch_ || N == 0 || (idx && (idx_bytes == 4 || idx_bytes == 8)),
             "catch needs idx with an element size of 4 or 8");
  DT_REQUIRE(cap >= 0, "negative capacity");
  const size_t need = dt_reach_catchments_scratch(N, reach == nullptr);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_reach_catchments(c->stream, link, idx, idx_bytes, N, scr, need, reach, catch_, heads, cap,
                                           n_reaches));
}

extern "C" int dt_dev_reach_channels(dt_ctx *c, const uint8_t *fdr, const int32_t *reach, int64_t H, int64_t W,
                                     int64_t R, int64_t *end, int64_t *down, int64_t *n_cells, int64_t *n_card,
                                     int64_t *n_diag) {
  DT_DEV(d, c, H, W);
  DT_TRY(dt_check_reach_count(R));
  if (R == 0) return DT_OK;
  DT_REQUIRE((fdr && reach) || H * W == 0, "NULL raster");
  DT_REQUIRE(end && down && n_cells && n_card && n_diag, "NULL output");
  return d.done(dt_launch_reach_channels(c->stream, fdr, reach, H, W, R, end, down, n_cells, n_card, n_diag));
}

// the stages' contract and the bound of frac_bits: N * rint(max(stages[K - 1], 1) * 2^frac_bits) <= 2^52
static int dt_check_stages(const double *stages, int K, int frac_bits, int64_t N) {
  DT_REQUIRE(K >= 1 && K <= 1024 && stages, "1..1024 stages per call");
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  DT_REQUIRE(std::isfinite(stages[0]) && stages[0] >= 0.0, "stages must be finite and >= 0");
  for (int k = 1; k < K; k++)
    DT_REQUIRE(std::isfinite(stages[k]) && stages[k] > stages[k - 1], "stages must be finite and strictly increasing");
  const double top = stages[K - 1] > 1.0 ? stages[K - 1] : 1.0;
  const double q = rint(ldexp(top, frac_bits));
  DT_REQUIRE(N == 0 || q <= (double)((1ull << 52) / (unsigned long long)N),
             "frac_bits is too fine: N * rint(max(stages[K - 1], 1) * 2^frac_bits) exceeds 2^52");
  return DT_OK;
}

extern "C" int dt_dev_reach_tables(dt_ctx *c, const int32_t *catch_, const void *hand, int hand_bytes,
                                   const float *slope, int64_t H, int64_t W, const double *stages, int K, int64_t R,
                                   int frac_bits, int64_t *cells, int64_t *Hq, int64_t *Bq) {
  DT_DEV(d, c, H, W);
  DT_TRY(dt_check_reach_count(R));
  DT_TRY(dt_check_stages(stages, K, frac_bits, H * W));
  DT_REQUIRE(hand_bytes == 4 || hand_bytes == 8, "hand's element size must be 4 or 8");
  if (R == 0) return DT_OK;
  DT_REQUIRE((catch_ && hand) || H * W == 0, "NULL raster");
  DT_REQUIRE(cells && Hq && Bq, "NULL table");
  const size_t need = dt_reach_tables_scratch(K);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_reach_tables(c->stream, catch_, hand, hand_bytes, slope, H, W, stages, K, R, frac_bits, scr,
                                       need, cells, Hq, Bq, c->status, dt_debug_get(DT_DBG_RC_SLOTS)));
}

extern "C" int dt_dev_inundate(dt_ctx *c, const int32_t *catch_, const void *hand, int hand_bytes, const double *stage,
                               int64_t H, int64_t W, int64_t R, float *depth) {
  DT_DEV(d, c, H, W);
  DT_TRY(dt_check_reach_count(R));
  DT_REQUIRE(hand_bytes == 4 || hand_bytes == 8, "hand's element size must be 4 or 8");
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(catch_ && hand && depth && (stage || R == 0), "NULL raster");
  return d.done(dt_launch_inundate(c->stream, catch_, hand, hand_bytes, stage, H * W, R, depth));
}

// zonal statistics: zone ids and labels travel in 31 bits
static int dt_check_zone_count(int64_t n_zones) {
  DT_REQUIRE(n_zones >= 0 && n_zones < (1ll << 31), "the number of zones must lie in [0, 2^31)");
  return DT_OK;
}
static int dt_check_zonal_compact(int label_bytes, int64_t limit, int64_t cap) {
  DT_REQUIRE(label_bytes == 4 || label_bytes == 8, "the labels' element size must be 4 or 8");
  DT_REQUIRE(limit >= 1 && limit < (1ll << 31), "limit must lie in [1, 2^31)");
  DT_REQUIRE(cap >= 0, "negative capacity");
  return DT_OK;
}
static int dt_check_zonal_tables(int64_t n_zones, int value_bytes, double origin, int frac_bits, const void *s2_lo,
                                 const void *s2_hi) {
  DT_TRY(dt_check_zone_count(n_zones));
  DT_REQUIRE(value_bytes == 4 || value_bytes == 8, "the values' element size must be 4 or 8");
  DT_REQUIRE(frac_bits >= 0 && frac_bits <= 24, "frac_bits must lie in [0, 24]");
  DT_REQUIRE(std::isfinite(origin), "origin must be finite");
  DT_REQUIRE((s2_lo == nullptr) == (s2_hi == nullptr), "s2_lo and s2_hi go together");
  return DT_OK;
}
static int dt_check_zonal_counts(int64_t n_zones, int value_bytes, const double *edges, int K) {
  DT_TRY(dt_check_zone_count(n_zones));
  DT_REQUIRE(value_bytes == 0 || value_bytes == 4 || value_bytes == 8, "the values' element size must be 0, 4 or 8");
  DT_REQUIRE(K >= 1 && K <= 1024, "1..1024 columns per call");
  DT_REQUIRE(n_zones * (int64_t)K * 8 <= (1ll << 31), "the table n_zones * K * 8 bytes exceeds 2 GiB");
  if (value_bytes != 0) {
    DT_REQUIRE(edges, "NULL edges");
    for (int k = 0; k <= K; k++)
      DT_REQUIRE(std::isfinite(edges[k]) && (k == 0 || edges[k] > edges[k - 1]),
                 "edges must be finite and strictly increasing");
  }
  return DT_OK;
}

extern "C" int dt_dev_zonal_compact(dt_ctx *c, const void *labels, int label_bytes, int64_t H, int64_t W,
                                    int64_t limit, int32_t *zones, int64_t *labels_of, int64_t cap, int64_t *n_zones) {
  DT_DEV(d, c, H, W);
  DT_TRY(dt_check_zonal_compact(label_bytes, limit, cap));
  const int64_t N = H * W;
  DT_REQUIRE(labels || N == 0, "NULL raster");
  DT_REQUIRE(labels_of || cap == 0, "a capacity without labels_of");
  const size_t need = dt_zonal_compact_scratch(limit);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_zonal_compact(c->stream, labels, label_bytes, N, limit, scr, need, zones,
                                        cap ? labels_of : nullptr, cap, n_zones));
}

extern "C" int dt_dev_zonal_tables(dt_ctx *c, const int32_t *zones, const void *values, int value_bytes, int64_t H,
                                   int64_t W, int64_t n_zones, double origin, int frac_bits, int has_nodata,
                                   double nodata, int64_t *count, int64_t *s1, uint64_t *s2_lo, uint64_t *s2_hi,
                                   void *vmin, void *vmax) {
  DT_DEV(d, c, H, W);
  DT_TRY(dt_check_zonal_tables(n_zones, value_bytes, origin, frac_bits, s2_lo, s2_hi));
  if (n_zones == 0) return DT_OK;
  DT_REQUIRE((zones && values) || H * W == 0, "NULL raster");
  DT_REQUIRE(count || s1 || s2_lo || vmin || vmax, "no table");
  return d.done(dt_launch_zonal_tables(c->stream, zones, values, value_bytes, H, W, n_zones, origin, frac_bits,
                                       has_nodata != 0, nodata, count, s1, s2_lo, s2_hi, vmin, vmax, c->status,
                                       dt_debug_get(DT_DBG_RC_SLOTS)));
}

extern "C" int dt_dev_zonal_counts(dt_ctx *c, const int32_t *zones, const void *values, int value_bytes, int64_t H,
                                   int64_t W, int64_t n_zones, const double *edges, int K, int has_nodata,
                                   double nodata, int64_t *counts) {
  DT_DEV(d, c, H, W);
  DT_TRY(dt_check_zonal_counts(n_zones, value_bytes, edges, K));
  if (n_zones == 0) return DT_OK;
  DT_REQUIRE((zones && values) || H * W == 0, "NULL raster");
  DT_REQUIRE(counts, "NULL table");
  const size_t need = dt_zonal_counts_scratch(K);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_zonal_counts(c->stream, zones, values, value_bytes, H, W, n_zones, edges, K, has_nodata != 0,
                                       nodata, scr, need, counts, c->status, dt_debug_get(DT_DBG_RC_SLOTS)));
}

extern "C" int dt_dev_zonal_paint(dt_ctx *c, const void *table, int elem_bytes, int64_t n_table, const int32_t *zones,
                                  int64_t H, int64_t W, const void *fill, void *out) {
  DT_DEV(d, c, H, W);
  DT_TRY(dt_check_zone_count(n_table));
  DT_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "the table's element size must be 4 or 8");
  DT_REQUIRE(fill, "NULL fill");
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(zones && out && (table || n_table == 0), "NULL raster");
  uint64_t bits = 0;
  memcpy(&bits, fill, (size_t)elem_bytes);
  return d.done(dt_launch_zonal_paint(c->stream, table, elem_bytes, n_table, zones, H * W, bits, out));
}

// connected regions: flat indices travel in int32
static int dt_check_regions(int connectivity, int64_t min_cells) {
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
  DT_REQUIRE(min_cells >= 1, "min_cells must be >= 1");
  return DT_OK;
}

extern "C" int dt_dev_regions_label(dt_ctx *c, const uint8_t *mask, int64_t H, int64_t W, int connectivity,
                                    int64_t *label, int64_t *size) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_regions(connectivity, 1));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(mask && label, "NULL raster");
  const size_t need = dt_regions_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_regions(c->stream, mask, nullptr, H, W, connectivity, 1, scr, need, label, size, nullptr));
}

extern "C" int dt_dev_regions_select(dt_ctx *c, const uint8_t *mask, const uint8_t *seeds, int64_t H, int64_t W,
                                     int connectivity, int64_t min_cells, uint8_t *keep) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_regions(connectivity, min_cells));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(mask && keep, "NULL raster");
  const size_t need = dt_regions_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_regions(c->stream, mask, seeds, H, W, connectivity, min_cells, scr, need, nullptr, nullptr,
                                  keep));
}

extern "C" int dt_dev_inundate_connected(dt_ctx *c, const int32_t *catch_, const void *hand, int hand_bytes,
                                         const double *stage, const int8_t *river, int64_t H, int64_t W, int64_t R,
                                         int connectivity, float *depth) {
  DT_DEV(d, c, H, W, 1.0);
  DT_TRY(dt_check_reach_count(R));
  DT_REQUIRE(hand_bytes == 4 || hand_bytes == 8, "hand's element size must be 4 or 8");
  DT_TRY(dt_check_regions(connectivity, 1));
  if (H * W == 0) return DT_OK;
  DT_REQUIRE(catch_ && hand && river && depth && (stage || R == 0), "NULL raster");
  const size_t need = dt_inundate_connected_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  return d.done(dt_launch_inundate_connected(c->stream, catch_, hand, hand_bytes, stage, river, H, W, R, connectivity,
                                             scr, need, depth));
}

extern "C" int dt_dev_river_mask(dt_ctx *c, const int32_t *acc32, int64_t N, int64_t threshold,
                                 int8_t *river) {
  DT_DEV(d, c);
  DT_REQUIRE((acc32 && river) || N == 0, "NULL raster");
  return d.done(dt_launch_river_mask(c->stream, acc32, N, threshold, river));
}

// dt_dev_flowhand, and with `fused` dt_dev_flowhand_gfi: the last tile pass also evaluates gfi.py:268-294 and :404-440
// from the values it holds in registers
static int dev_flowhand(dt_ctx *c, const float *dem, const uint8_t *fdr, const int8_t *river, const int32_t *acc32,
                        int64_t H, int64_t W, double px, double n_gfi, double b, double size, float *fdist,
                        int32_t *idx32, float *hand, int32_t *a_river, float *gfi, float *lnhlh, bool fused) {
  DT_DEV(d, c, H, W);
  if (fused) {
    DT_REQUIRE((dem && fdr && river && acc32 && gfi && lnhlh) || H * W == 0, "NULL raster");
  } else {
    DT_REQUIRE((fdr && river) || H * W == 0, "NULL raster");
    DT_REQUIRE(!hand || dem, "hand needs dem");
    DT_REQUIRE(!a_river || acc32, "a_river needs acc32");
    if (dt_flow_impl() == 1) {
      unsigned long long *state = (unsigned long long *)d.scratch((size_t)H * W * 8);
      DT_TRY(d.rc);
      return d.done(dt_launch_flowhand(c->stream, dem, fdr, river, acc32, H, W, px, state, fdist, idx32, hand, a_river));
    }
  }
  const size_t need = dt_flowhand_tiled_scratch(H, W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  DT_TRY(dt_launch_fh_local(c->stream, d.w, fdr, river, scr, need));
  return d.done(dt_launch_fh_finish(c->stream, d.w, dem, fdr, river, acc32, 0, px, scr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, fdist, idx32, nullptr, hand, a_river, gfi, lnhlh, n_gfi, b, size));
}
extern "C" int dt_dev_flowhand(dt_ctx *c, const float *dem, const uint8_t *fdr, const int8_t *river,
                               const int32_t *acc32, int64_t H, int64_t W, double px, float *fdist,
                               int32_t *idx32, float *hand, int32_t *a_river) {
  return dev_flowhand(c, dem, fdr, river, acc32, H, W, px, 0.0, 1.0, 1.0, fdist, idx32, hand, a_river, nullptr, nullptr,
                      false);
}
// HAND + GFI + ln(hl/H) in one go.  a_river may be NULL (it is only an intermediate).
extern "C" int dt_dev_flowhand_gfi(dt_ctx *c, const float *dem, const uint8_t *fdr, const int8_t *river,
                                   const int32_t *acc32, int64_t H, int64_t W, double px, double n_gfi,
                                   double b, float *fdist, int32_t *idx32, float *hand, int32_t *a_river,
                                   float *gfi, float *lnhlh) {
  return dev_flowhand(c, dem, fdr, river, acc32, H, W, px, n_gfi, b, px, fdist, idx32, hand, a_river, gfi, lnhlh, true);
}

extern "C" int dt_dev_twi(dt_ctx *c, const int32_t *acc32, const float *slope_rad, int64_t N, double px,
                          double n_top, float *ti, float *mti) {
  DT_DEV(d, c);
  DT_REQUIRE((acc32 && slope_rad && ti && mti) || N == 0, "NULL raster");
  return d.done(dt_launch_twi(c->stream, acc32, slope_rad, N, px, n_top, ti, mti));
}

extern "C" int dt_dev_gfi(dt_ctx *c, const float *hand, const int32_t *a_river, int64_t N, double n_gfi,
                          double b, double size, float *gfi) {
  DT_DEV(d, c);
  DT_REQUIRE((hand && a_river && gfi) || N == 0, "NULL raster");
  return d.done(dt_launch_gfi(c->stream, hand, a_river, N, n_gfi, b, size, gfi, 0));
}

extern "C" int dt_dev_lnhlh(dt_ctx *c, const float *hand, const int32_t *acc32, int64_t N, double n_gfi,
                            double b, double size, float *out) {
  DT_DEV(d, c);
  DT_REQUIRE((hand && acc32 && out) || N == 0, "NULL raster");
  return d.done(dt_launch_gfi(c->stream, hand, acc32, N, n_gfi, b, size, out, 1));
}

static int dev_gfi_lnhlh(dt_ctx *c, const float *hand, const void *a_river, const void *acc, int acc64, int64_t N,
                         double n_gfi, double b, double size, float *gfi, float *lnhlh) {
  DT_DEV(d, c);
  DT_REQUIRE((hand && a_river && acc && gfi && lnhlh) || N == 0, "NULL raster");
  return d.done(dt_launch_gfi_both(c->stream, hand, a_river, acc, acc64, N, n_gfi, b, size, gfi, lnhlh));
}
extern "C" int dt_dev_gfi_lnhlh(dt_ctx *c, const float *hand, const int32_t *a_river, const int32_t *acc32,
                                int64_t N, double n_gfi, double b, double size, float *gfi, float *lnhlh) {
  return dev_gfi_lnhlh(c, hand, a_river, acc32, 0, N, n_gfi, b, size, gfi, lnhlh);
}
extern "C" int dt_dev_gfi_lnhlh_a64(dt_ctx *c, const float *hand, const int64_t *a_river, const int64_t *acc64,
                                    int64_t N, double n_gfi, double b, double size, float *gfi, float *lnhlh) {
  return dev_gfi_lnhlh(c, hand, a_river, acc64, 1, N, n_gfi, b, size, gfi, lnhlh);
}

extern "C" int dt_dev_flowacc_river(dt_ctx *c, const uint8_t *fdr, const float *dem, int64_t H, int64_t W,
                                    int64_t threshold, int32_t *acc32, int8_t *river) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((fdr && acc32 && river) || H * W == 0, "NULL raster");
  if (dt_flow_impl() != 1) return dev_flowacc_tiled(d, fdr, dem, threshold, acc32, river);
  DT_TRY(dt_dev_flowacc(c, fdr, dem, H, W, acc32));
  return dt_dev_river_mask(c, acc32, H * W, threshold, river);
}

extern "C" int dt_dev_downslope(dt_ctx *c, const float *dem, const uint8_t *fdr, int64_t H, int64_t W,
                                double px, double dz, int raw, float *out) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && fdr && out) || H * W == 0, "NULL raster");
  // v1: one thread per cell walking global memory (kept for A/B and verification runs)
  if (dt_flow_impl() == 1) return d.done(dt_launch_downslope_v1(c->stream, dem, fdr, H, W, px, dz, raw, out));
  return d.done(dt_launch_downslope(c->stream, d.w, dem, fdr, px, dz, raw, out, nullptr));
}

extern "C" int64_t dt_downslope_lift_workspace(int64_t H, int64_t W) {
  return (H <= 0 || W <= 0) ? 0 : (int64_t)dt_downslope_lift_bytes(H, W);
}
extern "C" int64_t dt_downslope_queue_workspace(int64_t H, int64_t W) {
  return (H <= 0 || W <= 0) ? 0 : (int64_t)dt_downslope_queue_bytes(H, W);
}
extern "C" int64_t dt_downslope_tables_workspace(int64_t H, int64_t W) {
  return (H <= 0 || W <= 0) ? 0 : (int64_t)dt_downslope_tables_bytes(H, W);
}
extern "C" int64_t dt_downslope_tables_threshold(int64_t H, int64_t W) {
  return (H <= 0 || W <= 0) ? 0 : (int64_t)dt_downslope_lift_min(H, W);
}
// dt_dev_downslope with the long-walk acceleration (dt_kernels.hip, DsQueue), by the launcher's phase.  0: everything
// in one call, qwork = dt_downslope_lift_workspace bytes of device memory (queue | tables), the caller's for the
// duration of the call's kernels.  1 and 2: the same in two steps, for callers that may synchronise in between and want
// the 48 bytes per cell of the tables only for rasters that need them: dt_dev_downslope_queue runs the window kernel and
// queues the long walks (qwork: dt_downslope_queue_workspace bytes), dt_dev_downslope_queued waits and says how many
// there are, dt_dev_downslope_finish finishes them -- with skip tables when twork (dt_downslope_tables_workspace bytes)
// is given and at least dt_downslope_tables_threshold walks are queued, move by move otherwise.
static int dev_downslope_phase(dt_ctx *c, int phase, const float *dem, const uint8_t *fdr, int64_t H, int64_t W,
                               double px, double dz, int raw, float *out, void *qwork, int64_t qbytes, void *twork,
                               int64_t tbytes) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && fdr && out) || H * W == 0, "NULL raster");
  if (phase == 0) {
    DT_REQUIRE(qwork != nullptr && qbytes >= dt_downslope_lift_workspace(H, W), "downslope workspace missing or too small");
    const DtDsLift L = dt_downslope_lift_layout(d.w, qwork);
    qwork = L.qcount;
    twork = L.tab[0];
  } else {
    DT_REQUIRE(qwork != nullptr && qbytes >= dt_downslope_queue_workspace(H, W), "queue workspace missing or too small");
    DT_REQUIRE(twork == nullptr || tbytes >= dt_downslope_tables_workspace(H, W), "tables workspace too small");
  }
  return d.done(dt_launch_downslope(c->stream, d.w, dem, fdr, px, dz, raw, out, nullptr, qwork, twork, phase));
}
extern "C" int dt_dev_downslope_lift(dt_ctx *c, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                                     double dz, int raw, float *out, void *work, int64_t work_bytes) {
  return dev_downslope_phase(c, 0, dem, fdr, H, W, px, dz, raw, out, work, work_bytes, nullptr, 0);
}
extern "C" int dt_dev_downslope_queue(dt_ctx *c, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                                      double dz, int raw, float *out, void *qwork, int64_t qbytes) {
  return dev_downslope_phase(c, 1, dem, fdr, H, W, px, dz, raw, out, qwork, qbytes, nullptr, 0);
}
extern "C" int dt_dev_downslope_queued(dt_ctx *c, const void *qwork, int64_t *count) {
  DT_CTX(c);
  DT_REQUIRE(qwork && count, "NULL pointer");
  uint32_t n = 0;
  DT_HIP(hipMemcpyAsync(&n, qwork, sizeof(n), hipMemcpyDeviceToHost, c->stream));
  DT_HIP(hipStreamSynchronize(c->stream));
  *count = (int64_t)n;
  return DT_OK;
}
extern "C" int dt_dev_downslope_finish(dt_ctx *c, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                                       double dz, int raw, float *out, void *qwork, int64_t qbytes, void *twork,
                                       int64_t tbytes) {
  return dev_downslope_phase(c, 2, dem, fdr, H, W, px, dz, raw, out, qwork, qbytes, twork, tbytes);
}

extern "C" int dt_dev_confusion_multi(dt_ctx *c, const double *desc, const int8_t *flood, int64_t N,
                                      double nodata_value, const double *th_host, int nth, int under,
                                      int64_t *counts4_dev) {
  DT_DEV(d, c);
  DT_REQUIRE(th_host && counts4_dev, "NULL thresholds / counts");
  DT_REQUIRE((desc && flood) || N == 0, "NULL raster");
  return d.done(dt_launch_confusion(c->stream, desc, flood, N, nodata_value, th_host, nth, under,
                                    (unsigned long long *)counts4_dev));
}

extern "C" int dt_dev_threshold_hist(dt_ctx *c, const double *desc, const int8_t *flood, int64_t N,
                                     double nodata_value, const double *th_dev, int K, int under, int64_t *hist_dev) {
  DT_DEV(d, c);
  DT_REQUIRE(th_dev && hist_dev, "NULL thresholds / histogram");
  DT_REQUIRE((desc && flood) || N == 0, "NULL raster");
  return d.done(dt_launch_threshold_hist(c->stream, desc, flood, N, nodata_value, th_dev, K, under,
                                         (unsigned long long *)hist_dev));
}

// out3 = {smallest, second-smallest distinct, largest} value of x: np.unique(x)[0], [1], [-1] with one documented
// difference, the NaN rule.  np.unique sorts NaN last, so one NaN cell would make the largest value NaN and the raster
// impossible to scale; here NaN cells are skipped (a HAND with NaN cells still calibrates).  A slot that has no value
// is NaN: the second when all values are equal or N == 1, all three when N == 0 or every cell is NaN.  -inf and +inf
// are values.  -0.0 and +0.0 are one value, as for np.unique; which zero is returned for it is not specified.
extern "C" int dt_dev_unique_extremes_f32(dt_ctx *c, const float *x, int64_t N, float *out3_dev) {
  DT_DEV(d, c);
  DT_REQUIRE(x && out3_dev && N >= 0, "bad arguments");
  uint32_t *work = (uint32_t *)d.scratch(64, 256);
  DT_TRY(d.rc);
  return d.done(dt_launch_unique_extremes(c->stream, x, N, work, out3_dev));
}

extern "C" int dt_dev_minmax_scale_f32(dt_ctx *c, const float *x, int64_t N, float mn, float mx, float nodata,
                                       double *desc) {
  DT_DEV(d, c);
  DT_REQUIRE((x && desc) || N == 0, "NULL raster");
  return d.done(dt_launch_minmax_scale(c->stream, x, N, mn, mx, nodata, desc));
}

extern "C" int dt_dev_minmax_scale_f32_f64(dt_ctx *c, const float *x, int64_t N, double mn, double mx, double nodata,
                                           double *desc) {
  DT_DEV(d, c);
  DT_REQUIRE((x && desc) || N == 0, "NULL raster");
  return d.done(dt_launch_minmax_scale_f32f64(c->stream, x, N, mn, mx, nodata, desc));
}

extern "C" int dt_dev_classify(dt_ctx *c, const double *desc, int8_t *flood, int64_t N, double nodata_value,
                               double threshold, int under, int remap_flood, uint8_t *binary, int32_t *klass,
                               int64_t *counts4_dev) {
  DT_DEV(d, c);
  DT_REQUIRE(counts4_dev != nullptr, "counts4 is NULL");
  DT_REQUIRE((desc && flood) || N == 0, "NULL raster");
  return d.done(dt_launch_classify_f64(c->stream, desc, nullptr, flood, N, nodata_value, threshold, under, remap_flood,
                                       binary, klass, (unsigned long long *)counts4_dev));
}

extern "C" int dt_dev_membench_copy(dt_ctx *c, const float *a, float *b, int64_t N, int blocks) {
  DT_DEV(d, c);
  DT_REQUIRE(a && b && N >= 0 && blocks != 0, "bad arguments");
  return d.done(dt_launch_membench_copy(c->stream, a, b, N, blocks));
}

extern "C" int dt_dev_membench_mix(dt_ctx *c, const float *r0, const float *r1, float *w0, float *w1, float *w2,
                                   int64_t N, int n_reads, int n_writes, int nontemporal) {
  DT_DEV(d, c);
  DT_REQUIRE((n_reads < 1 || r0) && (n_reads < 2 || r1) && w0 && (n_writes < 2 || w1) && (n_writes < 3 || w2),
             "NULL stream");
  return d.done(dt_launch_membench_mix(c->stream, r0, r1, w0, w1, w2, N, n_reads, n_writes, nontemporal));
}

// *ms is written only when the call succeeds
extern "C" int dt_dev_membench_mix_timed(dt_ctx *c, const float *r0, const float *r1, float *w0, float *w1, float *w2,
                                         int64_t N, int n_reads, int n_writes, int nontemporal, int reps, double *ms) {
  DT_CTX(c);
  DT_REQUIRE(ms && reps >= 1, "bad arguments");
  DT_TRY(dt_dev_membench_mix(c, r0, r1, w0, w1, w2, N, n_reads, n_writes, nontemporal));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  DT_HIP(hipEventCreate(&e0));
  const hipError_t created = hipEventCreate(&e1);
  if (created != hipSuccess) {
    (void)hipEventDestroy(e0);
    DT_HIP(created);
  }
  int rc = DT_OK;
  float t = 0.0f;
  if (hipEventRecord(e0, c->stream) != hipSuccess) rc = DT_EHIP;
  for (int r = 0; r < reps && rc == DT_OK; r++)
    rc = dt_dev_membench_mix(c, r0, r1, w0, w1, w2, N, n_reads, n_writes, nontemporal);
  if (rc == DT_OK && (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                      hipEventElapsedTime(&t, e0, e1) != hipSuccess)) {
    dt_set_error("event timing failed: %s", hipGetErrorString(hipGetLastError()));
    rc = DT_EHIP;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc == DT_OK) *ms = (double)t / reps;
  return rc;
}
extern "C" int dt_dev_mem_info(dt_ctx *c, int64_t *free_bytes, int64_t *total_bytes) {
  DT_CTX(c);
  size_t f = 0, t = 0;
  DT_HIP(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  return DT_OK;
}

extern "C" int dt_dev_i32_to_i64(dt_ctx *c, const int32_t *src, int64_t N, int64_t *dst) {
  DT_DEV(d, c);
  return d.done(dt_launch_i32_to_i64(c->stream, src, N, dst));
}
extern "C" int dt_dev_i64_to_i32(dt_ctx *c, const int64_t *src, int64_t N, int32_t *dst) {
  DT_DEV(d, c);
  return d.done(dt_launch_i64_to_i32(c->stream, src, N, dst));
}

// ---- windowed device tier (one rank's core window of a larger raster; multi-GPU) ------------------
extern "C" int64_t dt_perim_cells(int64_t H, int64_t W) { return dt_perim_count((int)H, (int)W); }

extern "C" int dt_dev_slope_d8_w(dt_ctx *c, const dt_window *win, const float *dem, double px, float *slope,
                                 uint8_t *fdr, float *slope_rad) {
  DT_DEV(d, c, win);
  DT_REQUIRE(dem && (slope || fdr || slope_rad), "NULL raster");
  DT_TRY(dt_side_reserve(c, &c->aux, &c->aux_bytes, dt_stencil_aux_bytes(d.w.H, d.w.W)));
  return d.done(dt_launch_stencil(c->stream, d.w, dem, px, slope, fdr, slope_rad, nullptr, 0, 0.0, nullptr, nullptr,
                                  c->aux));
}

static int dev_slope_twi_w(dt_ctx *c, const dt_window *win, const float *dem, const void *acc, int acc64, double px,
                           double n_top, float *slope, float *slope_rad, float *ti, float *mti) {
  DT_DEV(d, c, win);
  DT_REQUIRE(dem && acc && ti && mti, "NULL raster");
  DT_TRY(dt_side_reserve(c, &c->aux, &c->aux_bytes, dt_stencil_aux_bytes(d.w.H, d.w.W)));
  return d.done(dt_launch_stencil(c->stream, d.w, dem, px, slope, nullptr, slope_rad, acc, acc64, n_top, ti, mti,
                                  c->aux));
}
extern "C" int dt_dev_slope_twi_w(dt_ctx *c, const dt_window *win, const float *dem, const int32_t *acc32,
                                  double px, double n_top, float *slope, float *slope_rad, float *ti,
                                  float *mti) {
  return dev_slope_twi_w(c, win, dem, acc32, 0, px, n_top, slope, slope_rad, ti, mti);
}
extern "C" int dt_dev_slope_twi_w_a64(dt_ctx *c, const dt_window *win, const float *dem, const int64_t *acc64,
                                      double px, double n_top, float *slope, float *slope_rad, float *ti,
                                      float *mti) {
  return dev_slope_twi_w(c, win, dem, acc64, 1, px, n_top, slope, slope_rad, ti, mti);
}

// dt_dev_downslope_w in its three forms.  DS_LIFT, with the long-walk workspace `work`: the long walks that stay in the
// rank's memory (core + halo) are queued and finished with skip tables over that memory; the ones that leave it are
// marked and counted as ever.  DS_EMIT (work = NULL or the long-walk workspace) also EMITS the walks leaving the rank's
// memory as walker records: walkers = [count u32, pad to 256 bytes | 48-byte records], see DsWalkOut in dt_kernels.hip.
// More walks than records fit: the count says so, the cells are marked -50 all the same.
extern "C" int64_t dt_downslope_lift_workspace_w(const dt_window *win) {
  DtWin w;
  if (dt_convert_window(win, &w) != DT_OK) return -1;
  return (int64_t)dt_downslope_lift_bytes_w(w);
}
enum DsForm { DS_PLAIN, DS_LIFT, DS_EMIT };
static int dev_downslope_w(dt_ctx *c, DsForm form, const dt_window *win, const float *dem, const uint8_t *fdr, double px,
                           double dz, int raw, float *out, int32_t *n_unresolved_dev, void *work, int64_t work_bytes,
                           void *walkers, int64_t walkers_bytes) {
  DT_DEV(d, c, win);
  DT_REQUIRE(dem && fdr && out, "NULL raster");
  if (form == DS_LIFT)
    DT_REQUIRE(work != nullptr && work_bytes >= (int64_t)dt_downslope_lift_bytes_w(d.w),
               "downslope workspace missing or too small");
  if (form == DS_EMIT) {
    DT_REQUIRE(work == nullptr || work_bytes >= (int64_t)dt_downslope_lift_bytes_w(d.w), "downslope workspace too small");
    DT_REQUIRE(walkers != nullptr && walkers_bytes >= 256 + 48, "walker buffer missing or too small");
  }
  if (n_unresolved_dev) DT_HIP(hipMemsetAsync(n_unresolved_dev, 0, sizeof(int32_t), c->stream));
  const DtDsLift L = work ? dt_downslope_lift_layout(d.w, work) : DtDsLift{};  // all null without work
  return d.done(dt_launch_downslope(c->stream, d.w, dem, fdr, px, dz, raw, out, (int *)n_unresolved_dev, L.qcount,
                                    L.tab[0], 0, walkers, (size_t)walkers_bytes));
}
extern "C" int dt_dev_downslope_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                  double px, double dz, int raw, float *out, int32_t *n_unresolved_dev) {
  return dev_downslope_w(c, DS_PLAIN, win, dem, fdr, px, dz, raw, out, n_unresolved_dev, nullptr, 0, nullptr, 0);
}
extern "C" int dt_dev_downslope_lift_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                       double px, double dz, int raw, float *out, int32_t *n_unresolved_dev,
                                       void *work, int64_t work_bytes) {
  return dev_downslope_w(c, DS_LIFT, win, dem, fdr, px, dz, raw, out, n_unresolved_dev, work, work_bytes, nullptr, 0);
}
extern "C" int dt_dev_downslope_emit_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                       double px, double dz, int raw, float *out, int32_t *n_unresolved_dev,
                                       void *work, int64_t work_bytes, void *walkers, int64_t walkers_bytes) {
  return dev_downslope_w(c, DS_EMIT, win, dem, fdr, px, dz, raw, out, n_unresolved_dev, work, work_bytes, walkers,
                         walkers_bytes);
}

// The walkers standing in this rank's memory advanced in place (k_ds_walk): rec = n records of 48 bytes; work
// (optional) = the rank's long-walk workspace as the downslope call of this step left it (its skip tables carry
// counting walkers across the rank 64 moves at a time).
extern "C" int dt_dev_downslope_walk_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr, double px,
                                       double dz, int64_t n, void *rec, void *work, int64_t work_bytes) {
  DT_DEV(d, c, win);
  DT_REQUIRE(n >= 0, "negative count");
  DT_REQUIRE(n == 0 || (dem && fdr && rec), "NULL pointer");
  DT_REQUIRE(work == nullptr || work_bytes >= (int64_t)dt_downslope_lift_bytes_w(d.w), "downslope workspace too small");
  return d.done(dt_launch_ds_walk(c->stream, d.w, dem, fdr, px, dz, n, rec, work));
}
// One iteration of the walkers' journey, prepared on the device (tiling.finish_downslope): the records that arrived
// finished are home -- their value goes into `out` (this rank's downslope raster, core origin) -- the others advance like
// dt_dev_downslope_walk_w; then every record that is still wanted somewhere is copied into `send`, grouped by destination
// rank (a walker that has just finished: the owner of its start cell; the others: the owner of the cell they stand on),
// and counts[d] = records for rank d, counts[n_ranks] = how many of them are still on their way.  row_starts /
// col_starts: device arrays of ty + 1 / tx + 1 global rows / columns (the layout's bands and the raster's end);
// counts: int32[ty * tx + 1]; scratch: int32[n + ty * tx]; send: room for n records.
extern "C" int dt_dev_downslope_walk_route_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                             double px, double dz, int64_t n, void *rec, void *work, int64_t work_bytes,
                                             float *out, const int32_t *row_starts, int32_t ty,
                                             const int32_t *col_starts, int32_t tx, void *send, int32_t *counts,
                                             int32_t *scratch) {
  DT_DEV(d, c, win);
  DT_REQUIRE(n >= 0, "negative count");
  DT_REQUIRE(ty >= 1 && tx >= 1 && row_starts && col_starts && counts, "layout / counts missing");
  DT_REQUIRE(n == 0 || (dem && fdr && rec && out && send && scratch), "NULL pointer");
  DT_REQUIRE(work == nullptr || work_bytes >= (int64_t)dt_downslope_lift_bytes_w(d.w), "downslope workspace too small");
  DT_TRY(dt_launch_ds_walk(c->stream, d.w, dem, fdr, px, dz, n, rec, work, out));
  return d.done(dt_launch_ds_route(c->stream, n, rec, row_starts, ty, col_starts, tx, send, counts, scratch));
}
// records of walkers at their start cells (core coordinates ys / xs of n cells), no move made: for cells that are
// marked -50 without a record (emission buffer too small, or a tile without one)
template <typename T, typename Launch>
static int dev_downslope_walk_seed_w(dt_ctx *c, const dt_window *win, const T *dem, int64_t n, const int32_t *ys,
                                     const int32_t *xs, void *rec, Launch launch) {
  DT_DEV(d, c, win);
  DT_REQUIRE(n >= 0, "negative count");
  DT_REQUIRE(n == 0 || (dem && ys && xs && rec), "NULL pointer");
  return d.done(launch(c->stream, d.w, dem, n, ys, xs, rec));
}
extern "C" int dt_dev_downslope_walk_seed_w(dt_ctx *c, const dt_window *win, const float *dem, int64_t n,
                                            const int32_t *ys, const int32_t *xs, void *rec) {
  return dev_downslope_walk_seed_w(c, win, dem, n, ys, xs, rec, dt_launch_ds_walk_seed);
}

extern "C" int dt_dev_flowacc_local_w(dt_ctx *c, const dt_window *win, const uint8_t *fdr, int32_t *acc32,
                                      int64_t *A_perim, int32_t *xr_perim, uint8_t *code_perim) {
  DT_DEV(d, c, win);
  DT_REQUIRE(fdr && A_perim && xr_perim && code_perim, "NULL pointer");  // acc32 is not touched by phase 1
  // HAND's workspace is reserved beside flow accumulation's, so that phase 2 can run fused with HAND's phase 1
  // (dt_dev_flowacc_finish_flowhand_local_w) without disturbing the state this call leaves
  const size_t need = dt_flowacc_tiled_scratch(d.w.H, d.w.W);
  void *scr, *scr2;
  d.scratch(need, dt_flowhand_tiled_scratch(d.w.H, d.w.W), &scr, &scr2);
  DT_TRY(d.rc);
  DT_TRY(dt_launch_fa_local(c->stream, d.w, fdr, scr, need, acc32, 1));
  DT_TRY(d.done(dt_launch_fa_summary(c->stream, d.w, scr, A_perim, xr_perim, code_perim)));
  dt_scratch_claim(c, DT_OWNER_FLOWACC, d.w.H, d.w.W, scr, scr2);
  return DT_OK;
}

// must follow dt_dev_flowacc_local_w on the same context with no other scratch-using call in between
static int dev_flowacc_finish_w(dt_ctx *c, const dt_window *win, const uint8_t *fdr, const float *dem,
                                const uint64_t *ext_perim, int64_t threshold, void *acc, int acc64, int8_t *river) {
  DT_DEV(d, c, win);
  DT_REQUIRE(fdr && acc, "NULL raster");
  const DtScratchClaim *k;
  DT_TRY(dt_scratch_claimed(c, DT_OWNER_FLOWACC, &d.w, false,
                            "dt_dev_flowacc_finish_w without a matching dt_dev_flowacc_local_w on this context (another "
                            "call has used the context's scratch in between)", &k));
  return d.done(dt_launch_fa_finish(c->stream, d.w, fdr, dem, k->ptr, (const unsigned long long *)ext_perim, threshold,
                                    acc, acc64, river, c->status));
}
extern "C" int dt_dev_flowacc_finish_w(dt_ctx *c, const dt_window *win, const uint8_t *fdr, const float *dem,
                                       const uint64_t *ext_perim, int64_t threshold, int32_t *acc32,
                                       int8_t *river) {
  return dev_flowacc_finish_w(c, win, fdr, dem, ext_perim, threshold, acc32, 0, river);
}
extern "C" int dt_dev_flowacc_finish_w_a64(dt_ctx *c, const dt_window *win, const uint8_t *fdr, const float *dem,
                                           const uint64_t *ext_perim, int64_t threshold, int64_t *acc64,
                                           int8_t *river) {
  return dev_flowacc_finish_w(c, win, fdr, dem, ext_perim, threshold, acc64, 1, river);
}

// phase 2 of flow accumulation and phase 1 of HAND in one call (the last accumulation tile pass and HAND's first
// share the tile's codes and the river mask: one kernel in the common form, dt_launch_fa_finish_fh_local); leaves the
// context in the state dt_dev_flowhand_local_w leaves it in
static int dev_flowacc_finish_fh_local_w(dt_ctx *c, const dt_window *win, const uint8_t *fdr, const float *dem,
                                         const uint64_t *ext_perim, int64_t threshold, void *acc, int acc64,
                                         int8_t *river, uint8_t *kind, int32_t *ref, int32_t *nc, int32_t *nd,
                                         float *zr, int64_t *ar) {
  DT_DEV(d, c, win);
  DT_REQUIRE(fdr && acc && river && kind && ref && nc && nd && zr && ar, "NULL pointer");
  const DtScratchClaim *k;
  DT_TRY(dt_scratch_claimed(c, DT_OWNER_FLOWACC, &d.w, true,
                            "dt_dev_flowacc_finish_flowhand_local_w without a matching dt_dev_flowacc_local_w on this "
                            "context (another call has used the context's scratch in between)", &k));
  char *fh = k->ptr2;
  DT_TRY(dt_launch_fa_finish_fh_local(c->stream, d.w, fdr, dem, k->ptr, fh, dt_flowhand_tiled_scratch(d.w.H, d.w.W),
                                      (const unsigned long long *)ext_perim, threshold, acc, acc64, river, c->status));
  DT_TRY(d.done(dt_launch_fh_summary(c->stream, d.w, fh, dem, acc, acc64, kind, ref, nc, nd, zr, (long long *)ar)));
  dt_scratch_claim(c, DT_OWNER_HAND, d.w.H, d.w.W, fh);  // flow accumulation's second region becomes HAND's
  return DT_OK;
}
extern "C" int dt_dev_flowacc_finish_flowhand_local_w(dt_ctx *c, const dt_window *win, const uint8_t *fdr,
                                                      const float *dem, const uint64_t *ext_perim, int64_t threshold,
                                                      int32_t *acc32, int8_t *river, uint8_t *kind, int32_t *ref,
                                                      int32_t *nc, int32_t *nd, float *zr, int64_t *ar) {
  return dev_flowacc_finish_fh_local_w(c, win, fdr, dem, ext_perim, threshold, acc32, 0, river, kind, ref, nc, nd, zr, ar);
}
extern "C" int dt_dev_flowacc_finish_flowhand_local_w_a64(dt_ctx *c, const dt_window *win, const uint8_t *fdr,
                                                          const float *dem, const uint64_t *ext_perim,
                                                          int64_t threshold, int64_t *acc64, int8_t *river,
                                                          uint8_t *kind, int32_t *ref, int32_t *nc, int32_t *nd,
                                                          float *zr, int64_t *ar) {
  return dev_flowacc_finish_fh_local_w(c, win, fdr, dem, ext_perim, threshold, acc64, 1, river, kind, ref, nc, nd, zr, ar);
}

// single raster: flow accumulation (all phases), river mask and HAND's phase 1; dt_dev_flowhand_finish_w /
// dt_dev_flowhand_gfi_finish_w with the whole raster as the window follow
static int dev_flowacc_river_flowhand_local(dt_ctx *c, const uint8_t *fdr, const float *dem, const uint8_t *nod4,
                                           int64_t H, int64_t W, int64_t threshold, int32_t *acc32, int8_t *river,
                                           const DtTwiEpilogue *twi = nullptr) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((fdr && acc32 && river) || H * W == 0, "NULL raster");
  DT_REQUIRE(!twi || H * W == 0 || dt_twi_epilogue_ok(d.w, acc32, river, twi),
             "this raster does not take the TI / MTI epilogue (dt_slope_from_d8_ok): use dt_dev_slope_twi");
  const size_t need = dt_flowacc_tiled_scratch(H, W), need2 = dt_flowhand_tiled_scratch(H, W);
  void *scr, *scr2;
  d.scratch(need, need2, &scr, &scr2);
  DT_TRY(d.rc);
  DT_TRY(dt_launch_fa_local(c->stream, d.w, fdr, scr, need, acc32, 0));
  int walked = 0;  // the launcher's choice of HAND's pass 1 (the walk form where the fused tile pass applies)
  DT_TRY(d.done(dt_launch_fa_finish_fh_local(c->stream, d.w, fdr, dem, scr, scr2, need2, nullptr, threshold, acc32, 0,
                                             river, c->status, nod4, dt_nodata4_ld(W), twi, &walked)));
  dt_scratch_claim(c, walked ? DT_OWNER_HAND_WALK : DT_OWNER_HAND, H, W, scr2);
  return DT_OK;
}
extern "C" int dt_dev_flowacc_river_flowhand_local(dt_ctx *c, const uint8_t *fdr, const float *dem, int64_t H, int64_t W,
                                                   int64_t threshold, int32_t *acc32, int8_t *river) {
  return dev_flowacc_river_flowhand_local(c, fdr, dem, nullptr, H, W, threshold, acc32, river);
}
// ... with the nodata mask the D8 kernel wrote (dt_dev_slope_d8_m): the pass reads 0.125 instead of 4 bytes per cell to
// learn which cells are nodata.  `dem` is still required (it serves the raster shapes the fused kernel does not take).
extern "C" int dt_dev_flowacc_river_flowhand_local_m(dt_ctx *c, const uint8_t *fdr, const float *dem,
                                                     const uint8_t *nodata4, int64_t H, int64_t W, int64_t threshold,
                                                     int32_t *acc32, int8_t *river) {
  DT_REQUIRE((dem && nodata4) || H * W == 0, "dem and the nodata mask are both required");
  return dev_flowacc_river_flowhand_local(c, fdr, dem, nodata4, H, W, threshold, acc32, river);
}
// ... and with TI / MTI out of the last accumulation tile pass: `slope` is the raster dt_dev_slope_d8_ms wrote, `marks`
// the workspace it was given (the cells whose TI / MTI fast path fails are added to it); dt_dev_slope_twi_fix follows.
// Only for the shapes dt_slope_from_d8_ok accepts.
extern "C" int dt_dev_flowacc_river_flowhand_local_ms(dt_ctx *c, const uint8_t *fdr, const float *dem,
                                                      const uint8_t *nodata4, int64_t H, int64_t W, int64_t threshold,
                                                      int32_t *acc32, int8_t *river, double px, double n_top,
                                                      const float *slope, float *ti, float *mti, void *marks) {
  DT_REQUIRE((dem && nodata4 && slope && ti && mti && marks) || H * W == 0, "NULL raster");
  const DtTwiEpilogue twi{slope, ti, mti, px, n_top, marks};
  return dev_flowacc_river_flowhand_local(c, fdr, dem, nodata4, H, W, threshold, acc32, river, &twi);
}
// the shapes on which the D8 kernel's slope and the accumulation pass's TI / MTI replace the slope + TI + MTI stencil
// (rows of whole 64-cell tiles; the rasters and the marks 16-byte aligned), and the bytes of the marks
extern "C" int dt_slope_from_d8_ok(int64_t H, int64_t W) {
  return H > 0 && W > 0 && W % 64 == 0;
}
extern "C" int64_t dt_slope_marks_bytes(int64_t H, int64_t W) {
  return (H < 0 || W < 0) ? -1 : (int64_t)dt_stencil_aux_bytes(H, W);
}
// the exact recomputation (k_slope_twi_fix) of slope, TI and MTI on the cells marked by dt_dev_slope_d8_ms and
// dt_dev_flowacc_river_flowhand_local_ms: microseconds when few are
extern "C" int dt_dev_slope_twi_fix(dt_ctx *c, const float *dem, const int32_t *acc32, int64_t H, int64_t W, double px,
                                    double n_top, float *slope, float *ti, float *mti, const void *marks) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && acc32 && slope && ti && mti && marks) || H * W == 0, "NULL raster");
  return d.done(dt_launch_slope_twi_fix(c->stream, d.w, dem, px, slope, acc32, n_top, ti, mti, (void *)marks));
}
extern "C" int64_t dt_nodata_mask_bytes(int64_t H, int64_t W) {
  return (H < 0 || W < 0) ? -1 : (int64_t)dt_nodata4_bytes(H, W);
}
// D8 codes (the hot / cold kernel pair) and, on the way, the nodata mask: one 16-bit word per 4 x 4 patch of cells
// (bit 4 j + k = cell (4 r + j, 4 i + k) holds the sentinel, z <= -100)
extern "C" int dt_dev_slope_d8_m(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr,
                                 uint8_t *nodata4) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && fdr && nodata4) || H * W == 0, "NULL raster");
  DT_TRY(dt_side_reserve(c, &c->aux, &c->aux_bytes, dt_stencil_aux_bytes(H, W)));
  return d.done(dt_launch_stencil(c->stream, d.w, dem, px, nullptr, fdr, nullptr, nullptr, 0, 0.0, nullptr, nullptr,
                                  c->aux, nodata4, dt_nodata4_ld(W)));
}
// ... and the slope raster (NULL: dt_dev_slope_d8_m), with the cells whose float32 slope is not proven in `marks`
// (dt_slope_marks_bytes; dt_dev_flowacc_river_flowhand_local_ms and dt_dev_slope_twi_fix take them from there)
extern "C" int dt_dev_slope_d8_ms(dt_ctx *c, const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr,
                                  uint8_t *nodata4, float *slope, void *marks) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && fdr && nodata4 && (marks || !slope)) || H * W == 0, "NULL raster");
  DT_TRY(dt_side_reserve(c, &c->aux, &c->aux_bytes, dt_stencil_aux_bytes(H, W)));
  return d.done(dt_launch_d8_slope(c->stream, d.w, dem, px, fdr, slope, c->aux, nodata4, dt_nodata4_ld(W), marks));
}
// ---- the resident chain on float64 heights ------------------------------------------------------------------------
extern "C" int dt_dev_slope_d8_f64(dt_ctx *c, const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr,
                                   float *proxy) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE(dem || H * W == 0, "NULL raster");
  return d.done(dt_launch_d8_f64(c->stream, dem, H, W, px, fdr, nullptr, proxy));
}
extern "C" int dt_dev_slope_twi_f64(dt_ctx *c, const double *dem, const int32_t *acc32, int64_t H, int64_t W,
                                    double px, double n_top, float *slope, float *slope_rad, float *ti, float *mti) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && acc32 && ti && mti) || H * W == 0, "NULL raster");
  return d.done(dt_launch_slope_twi_f64(c->stream, dem, acc32, H, W, px, n_top, slope, slope_rad, ti, mti));
}
extern "C" int dt_dev_downslope_f64(dt_ctx *c, const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                                    double dz, int raw, float *out) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && fdr && out) || H * W == 0, "NULL raster");
  return d.done(dt_launch_downslope_win_f64(c->stream, dem, fdr, H, W, px, dz, raw, out));
}
extern "C" int dt_dev_hand_gfi_f64(dt_ctx *c, const double *dem, const int32_t *idx32, const int32_t *acc32, int64_t H,
                                   int64_t W, double px, double n_gfi, double b, double *hand, float *gfi,
                                   float *lnhlh) {
  DT_DEV(d, c, H, W);
  DT_REQUIRE((dem && idx32 && acc32 && hand) || H * W == 0, "NULL raster");
  return d.done(dt_launch_hand_gfi_f64(c->stream, dem, idx32, acc32, H * W, n_gfi, b, px, hand, gfi, lnhlh));
}

static int dev_flowhand_local_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                const int8_t *river, const void *acc, int acc64, uint8_t *kind, int32_t *ref,
                                int32_t *nc, int32_t *nd, float *zr, int64_t *ar) {
  DT_DEV(d, c, win);
  DT_REQUIRE(fdr && river && kind && ref && nc && nd && zr && ar, "NULL pointer");
  const size_t need = dt_flowhand_tiled_scratch(d.w.H, d.w.W);
  void *scr = d.scratch(need);
  DT_TRY(d.rc);
  DT_TRY(dt_launch_fh_local(c->stream, d.w, fdr, river, scr, need));
  DT_TRY(d.done(dt_launch_fh_summary(c->stream, d.w, scr, dem, acc, acc64, kind, ref, nc, nd, zr, (long long *)ar)));
  dt_scratch_claim(c, DT_OWNER_HAND, d.w.H, d.w.W, scr);
  return DT_OK;
}
extern "C" int dt_dev_flowhand_local_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                       const int8_t *river, const int32_t *acc32, uint8_t *kind, int32_t *ref,
                                       int32_t *nc, int32_t *nd, float *zr, int64_t *ar) {
  return dev_flowhand_local_w(c, win, dem, fdr, river, acc32, 0, kind, ref, nc, nd, zr, ar);
}
extern "C" int dt_dev_flowhand_local_w_a64(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                           const int8_t *river, const int64_t *acc64, uint8_t *kind, int32_t *ref,
                                           int32_t *nc, int32_t *nd, float *zr, int64_t *ar) {
  return dev_flowhand_local_w(c, win, dem, fdr, river, acc64, 1, kind, ref, nc, nd, zr, ar);
}

// must follow dt_dev_flowhand_local_w on the same context with no other scratch-using call in between; `fused`: with
// the GFI / ln(hl/H) epilogue (see dt_dev_flowhand_gfi)
static int dev_flowhand_finish_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                 const int8_t *river, const void *acc, int acc64, double px, double n_gfi, double b,
                                 const uint8_t *res_ok, const int32_t *res_nc, const int32_t *res_nd,
                                 const int64_t *rem_gidx, const float *rem_zr, const int64_t *rem_ar, float *fdist,
                                 int32_t *idx32, int64_t *idx64, float *hand, void *a_river, float *gfi,
                                 float *lnhlh, bool fused) {
  DT_DEV(d, c, win);
  DT_REQUIRE(fdr && river, "NULL raster");
  DT_REQUIRE(!hand || dem, "hand needs dem");
  DT_REQUIRE(!a_river || acc, "a_river needs the accumulation raster");
  DT_REQUIRE(!fused || (dem && acc && gfi && lnhlh), "NULL raster");
  DT_REQUIRE(!res_ok || (res_nc && res_nd && rem_gidx && rem_zr && rem_ar), "incomplete rank-exit results");
  const DtScratchClaim *k;
  // the claim says which form pass 1 took: the walk form's is the single raster's, whole
  const bool walked = c->claim.owner == DT_OWNER_HAND_WALK && d.w.halo == 0 && d.w.gy0 == 0 && d.w.gx0 == 0 &&
                      d.w.H == d.w.Hg && d.w.W == d.w.Wg;
  DT_TRY(dt_scratch_claimed(c, walked ? DT_OWNER_HAND_WALK : DT_OWNER_HAND, &d.w, false,
                            "flowhand finish without a matching dt_dev_flowhand_local_w on this context (another call "
                            "has used the context's scratch in between)", &k));
  return d.done(dt_launch_fh_finish(c->stream, d.w, dem, fdr, river, acc, acc64, px, k->ptr, res_ok, res_nc, res_nd,
                                    (const long long *)rem_gidx, rem_zr, (const long long *)rem_ar, fdist, idx32,
                                    (long long *)idx64, hand, a_river, fused ? gfi : nullptr, fused ? lnhlh : nullptr,
                                    n_gfi, b, px, walked ? 1 : 0));
}
extern "C" int dt_dev_flowhand_finish_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                        const int8_t *river, const int32_t *acc32, double px,
                                        const uint8_t *res_ok, const int32_t *res_nc, const int32_t *res_nd,
                                        const int64_t *rem_gidx, const float *rem_zr, const int64_t *rem_ar,
                                        float *fdist, int32_t *idx32, int64_t *idx64, float *hand,
                                        int32_t *a_river) {
  return dev_flowhand_finish_w(c, win, dem, fdr, river, acc32, 0, px, 0.0, 1.0, res_ok, res_nc, res_nd, rem_gidx, rem_zr,
                               rem_ar, fdist, idx32, idx64, hand, a_river, nullptr, nullptr, false);
}
extern "C" int dt_dev_flowhand_finish_w_a64(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                            const int8_t *river, const int64_t *acc64, double px,
                                            const uint8_t *res_ok, const int32_t *res_nc, const int32_t *res_nd,
                                            const int64_t *rem_gidx, const float *rem_zr, const int64_t *rem_ar,
                                            float *fdist, int32_t *idx32, int64_t *idx64, float *hand,
                                            int64_t *a_river64) {
  return dev_flowhand_finish_w(c, win, dem, fdr, river, acc64, 1, px, 0.0, 1.0, res_ok, res_nc, res_nd, rem_gidx, rem_zr,
                               rem_ar, fdist, idx32, idx64, hand, a_river64, nullptr, nullptr, false);
}
extern "C" int dt_dev_flowhand_gfi_finish_w(dt_ctx *c, const dt_window *win, const float *dem, const uint8_t *fdr,
                                            const int8_t *river, const int32_t *acc32, double px, double n_gfi,
                                            double b, const uint8_t *res_ok, const int32_t *res_nc,
                                            const int32_t *res_nd, const int64_t *rem_gidx, const float *rem_zr,
                                            const int64_t *rem_ar, float *fdist, int32_t *idx32, int64_t *idx64,
                                            float *hand, int32_t *a_river, float *gfi, float *lnhlh) {
  return dev_flowhand_finish_w(c, win, dem, fdr, river, acc32, 0, px, n_gfi, b, res_ok, res_nc, res_nd, rem_gidx, rem_zr,
                               rem_ar, fdist, idx32, idx64, hand, a_river, gfi, lnhlh, true);
}
extern "C" int dt_dev_flowhand_gfi_finish_w_a64(dt_ctx *c, const dt_window *win, const float *dem,
                                                const uint8_t *fdr, const int8_t *river, const int64_t *acc64,
                                                double px, double n_gfi, double b, const uint8_t *res_ok,
                                                const int32_t *res_nc, const int32_t *res_nd,
                                                const int64_t *rem_gidx, const float *rem_zr, const int64_t *rem_ar,
                                                float *fdist, int32_t *idx32, int64_t *idx64, float *hand,
                                                int64_t *a_river64, float *gfi, float *lnhlh) {
  return dev_flowhand_finish_w(c, win, dem, fdr, river, acc64, 1, px, n_gfi, b, res_ok, res_nc, res_nd, rem_gidx, rem_zr,
                               rem_ar, fdist, idx32, idx64, hand, a_river64, gfi, lnhlh, true);
}

// the rank-level solves: their workspace is scratch2 (they run between the two phases of the tile kernels)
static int dt_scratch2_reserve(dt_ctx *c, size_t bytes) {
  return dt_side_reserve(c, &c->scratch2, &c->scratch2_bytes, bytes);
}

extern "C" int dt_dev_rank_solve_flowacc(dt_ctx *c, int ty, int tx, const int64_t *heights, const int64_t *widths,
                                         int64_t Pmax, const void *rows_dev, int64_t rowbytes,
                                         const int64_t *field_offsets3, int rank, int64_t P_rank,
                                         uint64_t *ext_out_dev) {
  DT_DEV(d, c);
  DT_REQUIRE(heights && widths && rows_dev && field_offsets3 && ext_out_dev, "NULL pointer");
  DT_REQUIRE(rank >= 0 && rank < ty * tx && P_rank >= 0 && P_rank <= Pmax, "bad rank / ring size");
  DT_TRY(dt_scratch2_reserve(c, dt_rank_solve_scratch(ty * tx, Pmax)));
  return d.done(dt_launch_rank_solve_flowacc(c->stream, ty, tx, heights, widths, Pmax, rows_dev, rowbytes,
                                             field_offsets3, rank, P_rank, c->scratch2,
                                             (unsigned long long *)ext_out_dev));
}

extern "C" int dt_dev_rank_solve_flowhand(dt_ctx *c, int ty, int tx, const int64_t *heights, const int64_t *widths,
                                          int64_t Pmax, const void *rows_dev, int64_t rowbytes,
                                          const int64_t *field_offsets7, int rank, int64_t P_rank,
                                          uint8_t *res_ok, int32_t *res_nc, int32_t *res_nd, int64_t *rem_gidx,
                                          float *rem_zr, int64_t *rem_ar) {
  DT_DEV(d, c);
  DT_REQUIRE(heights && widths && rows_dev && field_offsets7 && res_ok && res_nc && res_nd && rem_gidx && rem_zr &&
                 rem_ar, "NULL pointer");
  DT_REQUIRE(rank >= 0 && rank < ty * tx && P_rank >= 0 && P_rank <= Pmax, "bad rank / ring size");
  DT_TRY(dt_scratch2_reserve(c, dt_rank_solve_scratch(ty * tx, Pmax)));
  return d.done(dt_launch_rank_solve_flowhand(c->stream, ty, tx, heights, widths, Pmax, rows_dev, rowbytes,
                                              field_offsets7, rank, P_rank, c->scratch2, res_ok, res_nc, res_nd,
                                              (long long *)rem_gidx, rem_zr, (long long *)rem_ar));
}

// ---- float64 heights on one rank's window (tiling.RankTile(heights="float64")) ------------------------------------
extern "C" int dt_dev_slope_d8_f64_w(dt_ctx *c, const dt_window *win, const double *dem, double px, uint8_t *fdr,
                                     float *proxy) {
  DT_DEV(d, c, win);
  DT_REQUIRE(dem && (fdr || proxy), "NULL raster");
  return d.done(dt_launch_d8_f64_w(c->stream, d.w, dem, px, fdr, proxy));
}
static int dev_slope_twi_f64_w(dt_ctx *c, const dt_window *win, const double *dem, const void *acc, int acc64,
                               double px, double n_top, float *slope, float *slope_rad, float *ti, float *mti) {
  DT_DEV(d, c, win);
  DT_REQUIRE(dem && acc && ti && mti, "NULL raster");
  return d.done(dt_launch_slope_twi_f64_w(c->stream, d.w, dem, acc, acc64, px, n_top, slope, slope_rad, ti, mti));
}
extern "C" int dt_dev_slope_twi_f64_w(dt_ctx *c, const dt_window *win, const double *dem, const int32_t *acc32,
                                      double px, double n_top, float *slope, float *slope_rad, float *ti, float *mti) {
  return dev_slope_twi_f64_w(c, win, dem, acc32, 0, px, n_top, slope, slope_rad, ti, mti);
}
extern "C" int dt_dev_slope_twi_f64_w_a64(dt_ctx *c, const dt_window *win, const double *dem, const int64_t *acc64,
                                          double px, double n_top, float *slope, float *slope_rad, float *ti,
                                          float *mti) {
  return dev_slope_twi_f64_w(c, win, dem, acc64, 1, px, n_top, slope, slope_rad, ti, mti);
}
extern "C" int dt_dev_downslope_f64_w(dt_ctx *c, const dt_window *win, const double *dem, const uint8_t *fdr,
                                      double px, double dz, int raw, float *out, int32_t *n_unresolved_dev) {
  DT_DEV(d, c, win);
  DT_REQUIRE(dem && fdr && out, "NULL raster");
  if (n_unresolved_dev) DT_HIP(hipMemsetAsync(n_unresolved_dev, 0, sizeof(int32_t), c->stream));
  return d.done(dt_launch_downslope_win_f64_w(c->stream, d.w, dem, fdr, px, dz, raw, out, (int *)n_unresolved_dev));
}
extern "C" int dt_dev_downslope_walk_seed_f64_w(dt_ctx *c, const dt_window *win, const double *dem, int64_t n,
                                                const int32_t *ys, const int32_t *xs, void *rec) {
  return dev_downslope_walk_seed_w(c, win, dem, n, ys, xs, rec, dt_launch_ds_walk_seed_f64);
}
extern "C" int dt_dev_downslope_walk_route_f64_w(dt_ctx *c, const dt_window *win, const double *dem,
                                                 const uint8_t *fdr, double px, double dz, int64_t n, void *rec,
                                                 float *out, const int32_t *row_starts, int32_t ty,
                                                 const int32_t *col_starts, int32_t tx, void *send, int32_t *counts,
                                                 int32_t *scratch) {
  DT_DEV(d, c, win);
  DT_REQUIRE(n >= 0, "negative count");
  DT_REQUIRE(ty >= 1 && tx >= 1 && row_starts && col_starts && counts, "layout / counts missing");
  DT_REQUIRE(n == 0 || (dem && fdr && rec && out && send && scratch), "NULL pointer");
  DT_TRY(dt_launch_ds_walk_f64(c->stream, d.w, dem, fdr, px, dz, n, rec, out));
  return d.done(dt_launch_ds_route(c->stream, n, rec, row_starts, ty, col_starts, tx, send, counts, scratch));
}
extern "C" int dt_dev_flowhand_zr64_w(dt_ctx *c, const dt_window *win, const double *dem, int64_t n,
                                      const uint8_t *kind, const int32_t *ref, double *zr64) {
  DT_DEV(d, c, win);
  DT_REQUIRE(n >= 0 && n <= dt_perim_count(d.w.H, d.w.W), "bad ring size");
  DT_REQUIRE(n == 0 || (dem && kind && ref && zr64), "NULL pointer");
  return d.done(dt_launch_fh_zr64_w(c->stream, d.w, dem, n, kind, ref, zr64));
}
extern "C" int dt_dev_rank_solve_flowhand_f64(dt_ctx *c, int ty, int tx, const int64_t *heights, const int64_t *widths,
                                              int64_t Pmax, const void *rows_dev, int64_t rowbytes,
                                              const int64_t *field_offsets8, int rank, int64_t P_rank,
                                              uint8_t *res_ok, int32_t *res_nc, int32_t *res_nd, int64_t *rem_gidx,
                                              float *rem_zr, int64_t *rem_ar, double *rem_zr64) {
  DT_DEV(d, c);
  DT_REQUIRE(heights && widths && rows_dev && field_offsets8 && res_ok && res_nc && res_nd && rem_gidx && rem_zr &&
                 rem_ar && rem_zr64, "NULL pointer");
  DT_REQUIRE(rank >= 0 && rank < ty * tx && P_rank >= 0 && P_rank <= Pmax, "bad rank / ring size");
  DT_REQUIRE(field_offsets8[7] % 8 == 0 && rowbytes % 8 == 0, "the float64 field must be 8-byte aligned");
  DT_TRY(dt_scratch2_reserve(c, dt_rank_solve_scratch(ty * tx, Pmax)));
  return d.done(dt_launch_rank_solve_flowhand_f64(c->stream, ty, tx, heights, widths, Pmax, rows_dev, rowbytes,
                                                  field_offsets8, rank, P_rank, c->scratch2, res_ok, res_nc, res_nd,
                                                  (long long *)rem_gidx, rem_zr, (long long *)rem_ar, rem_zr64));
}
extern "C" int64_t dt_hand_f64_table_bytes(int64_t n_remote) {
  return n_remote < 0 ? -1 : dt_hand_f64_table_slots(n_remote) * 16;
}
static int dev_hand_gfi_f64_w(dt_ctx *c, const dt_window *win, const double *dem, const int32_t *idx32,
                              const int64_t *idx64, const void *acc, const void *a_river, int acc64, int64_t n_remote,
                              const uint8_t *res_ok, const int64_t *rem_gidx, const double *rem_zr64, void *table,
                              int64_t table_bytes, double px, double n_gfi, double b, double *hand, float *gfi,
                              float *lnhlh) {
  DT_DEV(d, c, win);
  DT_REQUIRE(dem && (idx32 || idx64) && acc && a_river && hand, "NULL raster");
  DT_REQUIRE(n_remote >= 0 && (n_remote == 0 || !res_ok || (rem_gidx && rem_zr64)), "incomplete rank-exit results");
  DT_REQUIRE(table && table_bytes >= dt_hand_f64_table_bytes(n_remote), "river-height table missing or too small");
  return d.done(dt_launch_hand_gfi_f64_w(c->stream, d.w, dem, idx64 ? nullptr : idx32, idx64, acc, a_river, acc64,
                                         n_remote, res_ok, rem_gidx, rem_zr64, table, n_gfi, b, px, hand, gfi, lnhlh));
}
extern "C" int dt_dev_hand_gfi_f64_w(dt_ctx *c, const dt_window *win, const double *dem, const int32_t *idx32,
                                     const int64_t *idx64, const int32_t *acc32, const int32_t *a_river32,
                                     int64_t n_remote, const uint8_t *res_ok, const int64_t *rem_gidx,
                                     const double *rem_zr64, void *table, int64_t table_bytes, double px,
                                     double n_gfi, double b, double *hand, float *gfi, float *lnhlh) {
  return dev_hand_gfi_f64_w(c, win, dem, idx32, idx64, acc32, a_river32, 0, n_remote, res_ok, rem_gidx, rem_zr64,
                            table, table_bytes, px, n_gfi, b, hand, gfi, lnhlh);
}
extern "C" int dt_dev_hand_gfi_f64_w_a64(dt_ctx *c, const dt_window *win, const double *dem, const int32_t *idx32,
                                         const int64_t *idx64, const int64_t *acc64, const int64_t *a_river64,
                                         int64_t n_remote, const uint8_t *res_ok, const int64_t *rem_gidx,
                                         const double *rem_zr64, void *table, int64_t table_bytes, double px,
                                         double n_gfi, double b, double *hand, float *gfi, float *lnhlh) {
  return dev_hand_gfi_f64_w(c, win, dem, idx32, idx64, acc64, a_river64, 1, n_remote, res_ok, rem_gidx, rem_zr64,
                            table, table_bytes, px, n_gfi, b, hand, gfi, lnhlh);
}

// ---- host tier: upload, kernels, download on a process-wide default context ----------------------------
static dt_ctx *g_host_ctx = nullptr;
static std::mutex g_host_mu;  // whole-call granularity, as SURVEY.md 8b (threading) allows

static int host_ctx(dt_ctx **out) {
  if (!g_host_ctx) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    DT_TRY(dt_ctx_create(dev, nullptr, &g_host_ctx));
  }
  *out = g_host_ctx;
  return hipSetDevice(g_host_ctx->device) == hipSuccess ? DT_OK : DT_EHIP;
}

// Device blocks of the host tier, cached per process: a drop-in caller makes one dt_<op> call per descriptor and
// raster-sized hipMalloc / hipFree pairs cost more than the kernels.  Blocks are handed out best-fit (within 25 %
// of the request) and kept when released; dt_host_trim() frees the idle ones.  Guarded by g_host_mu.
struct HostBlock {
  void *p;
  size_t bytes;
  bool busy;
};
static std::vector<HostBlock> g_blocks;
static void host_blocks_drop_idle(size_t keep_bytes) {
  // largest idle blocks go first; the host tier's stream is idle whenever a block is released (a HostCall waits for
  // it before it releases its blocks)
  for (;;) {
    size_t idle = 0;
    int big = -1;
    for (size_t i = 0; i < g_blocks.size(); i++)
      if (!g_blocks[i].busy) {
        idle += g_blocks[i].bytes;
        if (big < 0 || g_blocks[i].bytes > g_blocks[(size_t)big].bytes) big = (int)i;
      }
    if (idle <= keep_bytes || big < 0) return;
    (void)hipFree(g_blocks[(size_t)big].p);
    g_blocks.erase(g_blocks.begin() + big);
  }
}
static void *host_block_take(size_t bytes) {
  int best = -1;
  for (size_t i = 0; i < g_blocks.size(); i++)
    if (!g_blocks[i].busy && g_blocks[i].bytes >= bytes && g_blocks[i].bytes <= bytes + bytes / 4 + 4096 &&
        (best < 0 || g_blocks[i].bytes < g_blocks[(size_t)best].bytes))
      best = (int)i;
  if (best >= 0) {
    g_blocks[(size_t)best].busy = true;
    return g_blocks[(size_t)best].p;
  }
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    host_blocks_drop_idle(0);  // out of memory: drop every idle block and try once more
    (void)hipGetLastError();
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  }
  g_blocks.push_back(HostBlock{p, bytes, true});
  return p;
}
// idle blocks kept beyond this many bytes are freed on release (DT_HOST_CACHE_MB, default 4096; 0 = keep nothing)
static size_t host_cache_budget() {
  static long long mb = -1;
  if (mb < 0) {
    const char *e = getenv("DT_HOST_CACHE_MB");
    mb = e ? atoll(e) : 4096;
    if (mb < 0) mb = 0;
  }
  return (size_t)mb << 20;
}
static void host_block_release(void *p) {
  for (auto &b : g_blocks)
    if (b.p == p) b.busy = false;
  host_blocks_drop_idle(host_cache_budget());
}
// One host-tier call: it holds g_host_mu and the host context throughout and owns the call's device blocks.  in()
// uploads a host array into a new block, out() gives a block that finish() downloads, scratch() one that stays on the
// device: each returns the typed device pointer, NULL for a NULL host pointer.  rc keeps the first failure (opening
// the context included) and nothing is enqueued after it: an entry checks it on entry and before its first launch.
// finish() enqueues the downloads in the order they were asked for and synchronises; an entry that returns before it
// still waits for its stream (dt_last_error() keeps its message), so nothing enqueued outlives the call or its blocks.
struct HostCall {
  std::lock_guard<std::mutex> lk{g_host_mu};  // first member: the blocks are released while it is held
  dt_ctx *c = nullptr;
  int rc = host_ctx(&c);
  ~HostCall() {
    if (!synced && c) (void)hipStreamSynchronize(c->stream);
    for (void *p : blocks) host_block_release(p);
  }
  // a block the call can do without: NULL when none is to be had, and no failure recorded
  void *workspace(size_t bytes) {
    void *p = host_block_take(bytes ? bytes : 16);
    if (p) blocks.push_back(p);
    // cached or new, over the bytes asked for: scratch<T>, in() before its copy, out()
    if (p && c && dt_poison(c->stream, p, bytes) != DT_OK && rc == DT_OK) rc = DT_EHIP;
    return p;
  }
  template <typename T>
  T *scratch(size_t count) {
    T *d = rc == DT_OK ? (T *)workspace(count * sizeof(T)) : nullptr;
    if (!d && rc == DT_OK) {
      dt_set_error("hipMalloc of %zu bytes failed", count ? count * sizeof(T) : 16);
      rc = DT_ENOMEM;
    }
    return d;
  }
  template <typename T>
  T *in(const T *src, size_t count) {
    T *d = src ? scratch<T>(count) : nullptr;
    if (d) copy(d, src, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <typename T>
  T *out(T *dst, size_t count) {
    T *d = dst ? scratch<T>(count) : nullptr;
    if (d) downloads.push_back({dst, d, count * sizeof(T)});
    return d;
  }
  // a download enqueued now, not at finish()
  template <typename T>
  int download(T *dst, const T *src, size_t count) {
    copy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost);
    return rc;
  }
  int finish() {
    for (const Copy &d : downloads) copy(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost);
    if (rc != DT_OK) return rc;
    synced = true;
    return dt_ctx_sync(c);
  }

 private:
  struct Copy {
    void *dst;
    const void *src;
    size_t bytes;
  };
  std::vector<void *> blocks;
  std::vector<Copy> downloads;
  bool synced = false;
  void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (rc != DT_OK || bytes == 0) return;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    if (e != hipSuccess) {
      dt_set_error("hipMemcpyAsync of %zu bytes failed: %s", bytes, hipGetErrorString(e));
      rc = e == hipErrorOutOfMemory ? DT_ENOMEM : DT_EHIP;
    }
  }
};
extern "C" int dt_host_trim(void) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  if (g_host_ctx) DT_HIP(hipStreamSynchronize(g_host_ctx->stream));
  for (size_t i = 0; i < g_blocks.size();) {
    if (!g_blocks[i].busy) {
      DT_HIP(hipFree(g_blocks[i].p));
      g_blocks.erase(g_blocks.begin() + (long)i);
    } else {
      i++;
    }
  }
  return DT_OK;
}
// page-locked host memory for rasters that cross PCIe at full rate (the Python package keeps a pool of these
// behind the arrays chain.run_host returns)
// Page-locked host memory for rasters.  Large blocks are anonymous mappings on transparent huge pages, first touched
// by a few threads, then registered with the runtime: 9-15 ms per GiB on the MI355X host against 125 ms for
// hipHostMalloc (which faults and pins 4 KiB pages one thread at a time), the same 57 GB/s device-to-host
// (tools/micro/host_alloc.cpp, profiles/r3/host_alloc.txt).  Falls back to hipHostMalloc when the mapping or the
// registration is refused.
struct HostMap {
  void *map;
  size_t map_bytes;
};
static std::mutex g_hostmap_mu;
static std::vector<std::pair<void *, HostMap>> g_hostmaps;  // registered blocks by their aligned address
static const size_t DT_HUGE = (size_t)2 << 20;
// Huge pages are asked for until one such block takes longer to map and touch than plain pages would (a host whose
// memory is fragmented compacts it inside the page faults: seconds per GiB have been seen); 4 KiB pages from then on.
static std::atomic<bool> g_host_thp{true};

extern "C" int dt_host_alloc(int64_t bytes, void **out) {
  DT_REQUIRE(out && bytes >= 0, "bad arguments");
  *out = nullptr;
  if ((size_t)bytes >= 16 * DT_HUGE) {
    const size_t n = ((size_t)bytes + DT_HUGE - 1) & ~(DT_HUGE - 1);
    void *m = mmap(nullptr, n + DT_HUGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m != MAP_FAILED) {
      char *a = (char *)(((uintptr_t)m + DT_HUGE - 1) & ~(uintptr_t)(DT_HUGE - 1));
      const bool thp = g_host_thp.load();
      if (thp) (void)madvise(a, n, MADV_HUGEPAGE);
      const auto t_touch = std::chrono::steady_clock::now();
      unsigned hc = std::thread::hardware_concurrency();
      const int threads = (int)(hc == 0 ? 1 : (hc > 8 ? 8 : hc));
      const size_t per = ((n / (size_t)threads) + DT_HUGE - 1) & ~(DT_HUGE - 1);
      std::vector<std::thread> th;
      auto touch = [=](int t) {
        for (size_t o = per * (size_t)t; o < n && o < per * (size_t)(t + 1); o += 4096) a[o] = 0;
      };
      for (int t = 0; t < threads; t++) {
        try {
          th.emplace_back(touch, t);
        } catch (const std::system_error &) {  // no thread to be had: this one does the work (nothing may be thrown
          touch(t);                             // through extern "C")
        }
      }
      for (auto &t : th) t.join();
      const double touch_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_touch).count();
      if (thp && touch_s > 0.1 * ((double)n / (double)(1ull << 30)) + 0.02) g_host_thp.store(false);
      if (hipHostRegister(a, n, hipHostRegisterPortable) == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_hostmap_mu);
        g_hostmaps.push_back({(void *)a, HostMap{m, n + DT_HUGE}});
        *out = a;
        return DT_OK;
      }
      (void)hipGetLastError();
      munmap(m, n + DT_HUGE);
    }
  }
  DT_HIP(hipHostMalloc(out, bytes > 0 ? (size_t)bytes : 16, hipHostMallocDefault));
  return DT_OK;
}
extern "C" int dt_host_free(void *p) {
  if (!p) return DT_OK;
  HostMap hm{nullptr, 0};
  {
    std::lock_guard<std::mutex> lk(g_hostmap_mu);
    for (size_t i = 0; i < g_hostmaps.size(); i++)
      if (g_hostmaps[i].first == p) {
        hm = g_hostmaps[i].second;
        g_hostmaps.erase(g_hostmaps.begin() + (long)i);
        break;
      }
  }
  if (hm.map) {
    DT_HIP(hipHostUnregister(p));
    munmap(hm.map, hm.map_bytes);
    return DT_OK;
  }
  DT_HIP(hipHostFree(p));
  return DT_OK;
}
// float32 -> float64 on the host with a few threads (the reference's containers are float64 rasters holding float32
// values: numpy's single-threaded astype over a 16384^2 raster costs more than the kernel and both copies together)
extern "C" int dt_host_f32_to_f64(const float *src, double *dst, int64_t n) {
  DT_REQUIRE((src && dst) || n == 0, "NULL pointer");
  DT_REQUIRE(n >= 0, "negative size");
  unsigned hc = std::thread::hardware_concurrency();
  int threads = (int)(hc == 0 ? 1 : (hc > 8 ? 8 : hc));
  if (n < (int64_t)1 << 22) threads = 1;
  const int64_t per = (n + threads - 1) / threads;
  auto work = [=](int t) {
    const int64_t a = per * t, b = a + per < n ? a + per : n;
    for (int64_t i = a; i < b; i++) dst[i] = (double)src[i];
  };
  if (threads == 1) {
    work(0);
    return DT_OK;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++) {
    try {
      th.emplace_back(work, t);
    } catch (const std::system_error &) {  // no thread to be had: this one does the work
      work(t);
    }
  }
  for (auto &t : th) t.join();
  return DT_OK;
}
extern "C" int dt_synth_dem(uint32_t seed, int64_t Hg, int64_t Wg, int64_t y0, int64_t x0, int64_t h,
                            int64_t w, int nodata_pct, float *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  float *d = hc.out(out, (size_t)h * w);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_synth_dem(hc.c, seed, Hg, Wg, y0, x0, h, w, nodata_pct, d));
  return hc.finish();
}

static int host_slope_d8(const float *dem, int64_t H, int64_t W, double px, float *slope, uint8_t *fdr) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_REQUIRE(dem || H * W == 0, "dem is NULL");
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  const float *d_dem = hc.in(dem, n);
  float *d_sl = hc.out(slope, n);
  uint8_t *d_f = hc.out(fdr, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_slope_d8(hc.c, d_dem, H, W, px, d_sl, d_f, nullptr));
  return hc.finish();
}

extern "C" int dt_slope_f32(const float *dem, int64_t H, int64_t W, double px, float *slope) {
  DT_REQUIRE(slope || H * W == 0, "slope is NULL");
  return host_slope_d8(dem, H, W, px, slope, nullptr);
}
extern "C" int dt_d8_f32(const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *slope) {
  DT_REQUIRE(fdr || H * W == 0, "fdr is NULL");
  return host_slope_d8(dem, H, W, px, slope, fdr);
}

extern "C" int dt_flowacc_u8(const uint8_t *fdr, const float *dem, int64_t H, int64_t W, int64_t *acc) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(fdr && acc, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const float *d_dem = hc.in(dem, n);
  int32_t *d_a32 = hc.scratch<int32_t>(n);
  int64_t *d_a64 = hc.out(acc, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_flowacc(hc.c, d_f, d_dem, H, W, d_a32));
  DT_TRY(dt_dev_i32_to_i64(hc.c, d_a32, (int64_t)n, d_a64));
  return hc.finish();
}

extern "C" int dt_flowacc_weighted(const uint8_t *fdr, const float *dem, const double *w, int64_t H, int64_t W,
                                   int frac_bits, double *acc) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(fdr && w && acc, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const double *d_w = hc.in(w, n);
  const float *d_dem = hc.in(dem, n);
  double *d_a = hc.out(acc, n);
  DT_TRY(hc.rc);
  int32_t st = 0;
  DT_TRY(dt_ctx_status(hc.c, &st));  // this call's status only
  DT_TRY(dt_dev_flowacc_weighted(hc.c, d_f, d_dem, d_w, H, W, frac_bits, d_a));
  DT_TRY(dt_ctx_status(hc.c, &st));
  DT_REQUIRE(!(st & DT_STATUS_BAD_WEIGHT), "a weight is negative, not finite, or over the bound of frac_bits");
  return hc.finish();
}

extern "C" int dt_stream_order(const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W, int8_t *strahler,
                               int64_t *shreve, int64_t *link) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_so(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(fdr && river && strahler, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const int8_t *d_r = hc.in(river, n);
  int8_t *d_o = hc.out(strahler, n);
  int64_t *d_s = hc.out(shreve, n);
  int64_t *d_l = hc.out(link, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_stream_order(hc.c, d_f, d_r, H, W, d_o, d_s, d_l));
  return hc.finish();
}

extern "C" int dt_drainage(const uint8_t *fdr, const float *dem, const int64_t *pour, int64_t H, int64_t W,
                           double px, int64_t *target, double *length, int64_t *label) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_REQUIRE(!label || pour, "label requires pour");
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(fdr, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const float *d_dem = hc.in(dem, n);
  const int64_t *d_p = hc.in(pour, n);
  int64_t *d_t = hc.out(target, n);
  double *d_l = hc.out(length, n);
  int64_t *d_b = hc.out(label, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_drainage(hc.c, d_f, d_dem, d_p, H, W, px, d_t, d_l, d_b));
  return hc.finish();
}

extern "C" int dt_upslope_length(const uint8_t *fdr, const float *dem, int64_t H, int64_t W, double px,
                                 double *length) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  const size_t n = (size_t)H * W;
  if (n == 0 || !length) return DT_OK;
  DT_REQUIRE(fdr, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  double *d_l = hc.out(length, n);
  const float *d_dem = hc.in(dem, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_upslope_length(hc.c, d_f, d_dem, H, W, px, d_l));
  return hc.finish();
}

extern "C" int dt_dinf_direction(const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px, float *angle,
                                 float *slope) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && angle, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  const uint8_t *d_f = hc.in(fdr, n);
  float *d_a = hc.out(angle, n);
  float *d_s = hc.out(slope, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_dinf_direction(hc.c, d_dem, d_f, H, W, px, d_a, d_s));
  return hc.finish();
}

// The rounds of a countdown accumulation on the host tier: round 0, then batches of DT_DINF_BATCH queue rounds until a
// look at the control words (d_ctl) finds everything queued drained, then the out step.  launch(start, rounds, finish)
// is the op's launcher on the call's rasters.  *st: the status bits this call raised; info4: dt_countdown_info4's.
#define DT_DINF_BATCH 32
template <typename Launch>
static int host_countdown(HostCall &hc, const uint32_t *d_ctl, int32_t *st, int64_t *info4, Launch launch) {
  DT_TRY(dt_ctx_status(hc.c, st));  // this call's status only
  uint32_t ctl[8] = {0};
  for (int start = 1;; start = 0) {
    DT_TRY(launch(start, DT_DINF_BATCH, 0));
    DT_TRY(hc.download(ctl, d_ctl, 8));
    DT_HIP(hipStreamSynchronize(hc.c->stream));
    if (ctl[0] == ctl[2]) break;  // everything queued has been drained
  }
  DT_TRY(dt_launched(launch(0, 0, 1)));
  DT_TRY(dt_ctx_status(hc.c, st));
  dt_countdown_info4(ctl, info4);
  return DT_OK;
}

extern "C" int dt_dinf_accumulate(const float *angle, const double *w, int64_t H, int64_t W, int frac_bits,
                                  double *acc, int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(angle && acc, "NULL raster");
  const float *d_a = hc.in(angle, n);
  const double *d_w = hc.in(w, n);
  double *d_o = hc.out(acc, n);
  const size_t need = dt_dinf_accumulate_scratch(H, W);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  int32_t st = 0;
  int64_t got[4];
  const int cap = dt_dinf_stack_cap();
  DT_TRY(host_countdown(hc, dt_dinf_accumulate_ctl(scr, H, W), &st, got, [&](int start, int rounds, int finish) {
    return dt_launch_dinf_accumulate(hc.c->stream, d_a, d_w, H, W, frac_bits, start, rounds, finish, cap, scr, need,
                                     d_o, hc.c->status);
  }));
  DT_REQUIRE(!(st & DT_STATUS_BAD_ANGLE), "an angle is neither -1, -100 nor in [0, float32(2 pi)]");
  DT_REQUIRE(!(st & DT_STATUS_BAD_WEIGHT), "a weight is negative, not finite, or over the bound of frac_bits");
  if (info4) memcpy(info4, got, sizeof(got));
  return hc.finish();
}

// The host tier of a routing run, after the flow raster: the weights, the parameter and the outputs on the device, the
// rounds (host_countdown) and the status.  launch(d_w, d_p, d_out, start, rounds, finish) is the op's launcher.
template <typename Launch>
static int host_route(HostCall &hc, const double *w, const double *param, size_t n, double *const (&host)[4],
                      const uint32_t *d_ctl, int bad_flow_bit, const char *bad_flow_msg, int64_t *info4,
                      Launch launch) {
  const double *d_w = hc.in(w, n);
  const double *d_p = hc.in(param, n);
  double *d_o[4];
  for (int i = 0; i < 4; i++) d_o[i] = hc.out(host[i], n);
  DT_TRY(hc.rc);
  int32_t st = 0;
  int64_t got[4];
  DT_TRY(host_countdown(hc, d_ctl, &st, got, [&](int start, int rounds, int finish) {
    return launch(d_w, d_p, d_o, start, rounds, finish);
  }));
  DT_REQUIRE(!(st & bad_flow_bit), bad_flow_msg);
  DT_REQUIRE(!(st & DT_STATUS_BAD_WEIGHT), "a weight is negative, not finite, or over the bound of frac_bits");
  DT_REQUIRE(!(st & DT_STATUS_BAD_PARAM), "a parameter is NaN, negative or (decay) above 1");
  if (info4) memcpy(info4, got, sizeof(got));
  return hc.finish();
}
// what both host entries check first
static int dt_check_route_host(int64_t H, int64_t W, int frac_bits, int mode, int64_t *info4) {
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  DT_REQUIRE(mode == DT_ROUTE_DECAY || mode == DT_ROUTE_RETAIN || mode == DT_ROUTE_LIMIT,
             "mode must be DT_ROUTE_DECAY, DT_ROUTE_RETAIN or DT_ROUTE_LIMIT");
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  return DT_OK;
}

extern "C" int dt_dinf_route(const float *angle, const double *w, const double *param, int64_t H, int64_t W,
                             int frac_bits, int mode, double *inflow, double *load, double *outflow, double *retained,
                             int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_route_host(H, W, frac_bits, mode, info4));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(angle && param, "NULL raster");
  DT_REQUIRE(inflow || load || outflow || retained, "all four outputs are NULL");
  double *const host[4] = {inflow, load, outflow, retained};
  const float *d_a = hc.in(angle, n);
  const size_t need = dt_dinf_accumulate_scratch(H, W);
  char *scr = hc.scratch<char>(need);
  const int cap = dt_dinf_stack_cap();
  return host_route(hc, w, param, n, host, dt_dinf_accumulate_ctl(scr, H, W), DT_STATUS_BAD_ANGLE,
                    "an angle is neither -1, -100 nor in [0, float32(2 pi)]", info4,
                    [&](const double *d_w, const double *d_p, double *const *d_o, int start, int rounds, int finish) {
                      return dt_launch_dinf_route(hc.c->stream, d_a, d_w, d_p, H, W, frac_bits, mode, start, rounds,
                                                  finish, cap, scr, need, d_o[0], d_o[1], d_o[2], d_o[3],
                                                  hc.c->status);
                    });
}

extern "C" int dt_mfd_route(const uint16_t *shares, const double *w, const double *param, int64_t H, int64_t W,
                            int frac_bits, int mode, double *inflow, double *load, double *outflow, double *retained,
                            int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_route_host(H, W, frac_bits, mode, info4));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(shares && param, "NULL raster");
  DT_REQUIRE(inflow || load || outflow || retained, "all four outputs are NULL");
  double *const host[4] = {inflow, load, outflow, retained};
  const uint16_t *d_s = hc.in(shares, n * 8);
  const size_t need = dt_mfd_accumulate_scratch(H, W);
  char *scr = hc.scratch<char>(need);
  const int cap = dt_mfd_stack_cap();
  return host_route(hc, w, param, n, host, dt_mfd_accumulate_ctl(scr, H, W), DT_STATUS_BAD_SHARES,
                    "a share word is not eight 0xFFFF and has a slot above 32768 or a sum that is neither 0 nor 32768",
                    info4,
                    [&](const double *d_w, const double *d_p, double *const *d_o, int start, int rounds, int finish) {
                      return dt_launch_mfd_route(hc.c->stream, d_s, d_w, d_p, H, W, frac_bits, mode, start, rounds,
                                                 finish, cap, scr, need, d_o[0], d_o[1], d_o[2], d_o[3],
                                                 hc.c->status);
                    });
}

extern "C" int dt_mfd_shares(const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double exponent, int contour,
                             uint16_t *shares) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_TRY(dt_check_mfd_exponent(exponent));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && shares, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  const uint8_t *d_f = hc.in(fdr, n);
  uint16_t *d_s = hc.out(shares, n * 8);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_mfd_shares(hc.c, d_dem, d_f, H, W, exponent, contour, d_s));
  return hc.finish();
}

extern "C" int dt_mfd_accumulate(const uint16_t *shares, const double *w, int64_t H, int64_t W, int frac_bits,
                                 double *acc, int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(shares && acc, "NULL raster");
  const uint16_t *d_s = hc.in(shares, n * 8);
  const double *d_w = hc.in(w, n);
  double *d_o = hc.out(acc, n);
  const size_t need = dt_mfd_accumulate_scratch(H, W);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  int32_t st = 0;
  int64_t got[4];
  const int cap = dt_mfd_stack_cap();
  DT_TRY(host_countdown(hc, dt_mfd_accumulate_ctl(scr, H, W), &st, got, [&](int start, int rounds, int finish) {
    return dt_launch_mfd_accumulate(hc.c->stream, d_s, d_w, H, W, frac_bits, start, rounds, finish, cap, scr, need, d_o,
                                    hc.c->status);
  }));
  DT_REQUIRE(!(st & DT_STATUS_BAD_SHARES),
             "a share word is not eight 0xFFFF and has a slot above 32768 or a sum that is neither 0 nor 32768");
  DT_REQUIRE(!(st & DT_STATUS_BAD_WEIGHT), "a weight is negative, not finite, or over the bound of frac_bits");
  if (info4) memcpy(info4, got, sizeof(got));
  return hc.finish();
}

extern "C" int dt_terrain(const float *dem, int64_t H, int64_t W, double px, int radius, double sx, double sy,
                          double sz, float *gradient, float *aspect, float *profile, float *plan, float *tangential,
                          float *mean, float *laplacian, float *hillshade) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_TRY(dt_check_terrain(radius, sx, sy, sz));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  float *const host[DT_TERRAIN_OUTPUTS] = {gradient, aspect, profile, plan, tangential, mean, laplacian, hillshade};
  bool any = false;
  for (float *o : host) any = any || o != nullptr;
  DT_REQUIRE(any, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  float *d[DT_TERRAIN_OUTPUTS];
  for (int o = 0; o < DT_TERRAIN_OUTPUTS; o++) d[o] = hc.out(host[o], n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_terrain(hc.c, d_dem, H, W, px, radius, sx, sy, sz, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]));
  return hc.finish();
}

extern "C" int dt_focal(const float *dem, int64_t H, int64_t W, double origin, int frac_bits, const int32_t *radii,
                        int n_radii, int32_t *count, float *mean, float *std_, float *tpi, float *dev,
                        uint16_t *scale) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  const bool stats = count || mean || std_ || tpi;
  DT_TRY(dt_check_focal(origin, frac_bits, radii, n_radii, stats, stats || dev || scale));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  int32_t *d_count = hc.out(count, n);
  float *d_mean = hc.out(mean, n), *d_std = hc.out(std_, n), *d_tpi = hc.out(tpi, n), *d_dev = hc.out(dev, n);
  uint16_t *d_scale = hc.out(scale, n);
  DT_TRY(hc.rc);
  int32_t st = 0;
  DT_TRY(dt_ctx_status(hc.c, &st));  // this call's status only
  DT_TRY(dt_dev_focal(hc.c, d_dem, H, W, origin, frac_bits, radii, n_radii, d_count, d_mean, d_std, d_tpi, d_dev,
                      d_scale));
  DT_TRY(dt_ctx_status(hc.c, &st));
  if (st & DT_STATUS_BAD_HEIGHT) {
    dt_set_error("invalid argument: a valid height is outside the contract of origin=%.17g, frac_bits=%d: "
                 "0 <= rint((z - origin) * 2^frac_bits) <= %lld (the bound of radius %d)",
                 origin, frac_bits, (long long)dt_focal_qmax(radii[n_radii - 1]), (int)radii[n_radii - 1]);
    return DT_EINVAL;
  }
  return hc.finish();
}

extern "C" int dt_filter_extremes(const float *dem, int64_t H, int64_t W, int radius, float *minimum, float *maximum,
                                  float *range, float *opening, float *closing) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_TRY(dt_check_filter_extremes(radius));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(minimum || maximum || range || opening || closing, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  float *d_min = hc.out(minimum, n), *d_max = hc.out(maximum, n), *d_range = hc.out(range, n);
  float *d_open = hc.out(opening, n), *d_close = hc.out(closing, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_filter_extremes(hc.c, d_dem, H, W, radius, d_min, d_max, d_range, d_open, d_close));
  return hc.finish();
}

extern "C" int dt_filter_rank(const float *dem, int64_t H, int64_t W, int radius, const uint16_t *table, int n_table,
                              float *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_TRY(dt_check_filter_rank(radius, table, n_table));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(out, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  float *d_out = hc.out(out, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_filter_rank(hc.c, d_dem, H, W, radius, table, n_table, d_out));
  return hc.finish();
}

extern "C" int dt_filter_denoise(const float *dem, int64_t H, int64_t W, double px, int radius, double cos_threshold,
                                 int iterations, double max_change, float *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_TRY(dt_check_filter_denoise(radius, cos_threshold, iterations, max_change));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(out, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  float *d_out = hc.out(out, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_filter_denoise(hc.c, d_dem, H, W, px, radius, cos_threshold, iterations, max_change, d_out));
  return hc.finish();
}

extern "C" int dt_horizon(const float *dem, int64_t H, int64_t W, double px, int radius, int skip, double flat_tan,
                          uint8_t *landform, uint16_t *pattern, float *positive, float *negative, float *sky_view) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_TRY(dt_check_horizon(radius, skip, flat_tan));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(landform || pattern || positive || negative || sky_view, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  uint8_t *d_form = hc.out(landform, n);
  uint16_t *d_pat = hc.out(pattern, n);
  float *d_pos = hc.out(positive, n), *d_neg = hc.out(negative, n), *d_sky = hc.out(sky_view, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_horizon(hc.c, d_dem, H, W, px, radius, skip, flat_tan, d_form, d_pat, d_pos, d_neg, d_sky));
  return hc.finish();
}

extern "C" int dt_mrvbf(const float *dem, int64_t H, int64_t W, double px, double slope_threshold, int levels,
                        double pctl_valley, double pctl_ridge, const double *p, float *mrvbf, float *mrrtf) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_TRY(dt_check_mrvbf(slope_threshold, levels, pctl_valley, pctl_ridge, p));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(mrvbf || mrrtf, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  float *d_v = hc.out(mrvbf, n), *d_r = hc.out(mrrtf, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_mrvbf(hc.c, d_dem, H, W, px, slope_threshold, levels, pctl_valley, pctl_ridge, p, d_v, d_r));
  return hc.finish();
}

extern "C" int dt_percentile(const float *dem, int64_t H, int64_t W, int radius, float *lower, float *higher) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_TRY(dt_check_percentile(radius));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(lower || higher, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  float *d_lo = hc.out(lower, n), *d_hi = hc.out(higher, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_percentile(hc.c, d_dem, H, W, radius, d_lo, d_hi));
  return hc.finish();
}

extern "C" int dt_coarsen(const float *dem, int64_t H, int64_t W, double px, const double *g6, float *dem3,
                          float *slope3) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_TRY(dt_check_coarsen(g6));
  const size_t n = (size_t)H * W, nc = (size_t)((H + 2) / 3) * (size_t)((W + 2) / 3);
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && dem3 && slope3, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  float *d_z = hc.out(dem3, nc), *d_s = hc.out(slope3, nc);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_coarsen(hc.c, d_dem, H, W, px, g6, d_z, d_s));
  return hc.finish();
}

// Batches of tile rounds (dt_tile_rounds.h) until a quiet one: launch(start, batch) enqueues `batch` rounds, round r of
// them raising the device word d_flags[r]; 8, 16, 32, then 64 rounds between two looks at the flags (a round that
// follows a quiet one costs a few microseconds; a path that winds through many tiles wants few host round trips per
// round).  *rounds counts the rounds that did something, also while the batches run (launch may look).  Synchronises.
template <typename Launch>
static int host_tile_rounds(HostCall &hc, const uint32_t *d_flags, int64_t *rounds, Launch launch) {
  uint32_t flags[DT_TILE_ROUNDS_BATCH_MAX];
  *rounds = 0;
  int batch = DT_TILE_ROUNDS_BATCH0;
  for (int start = 1;; start = 0) {
    DT_TRY(launch(start, batch));
    DT_TRY(hc.download(flags, d_flags, (size_t)batch));
    DT_HIP(hipStreamSynchronize(hc.c->stream));
    int used = 0;
    while (used < batch && flags[used]) used++;
    *rounds += used;
    if (used < batch) return DT_OK;  // a quiet round: nothing is left to do
    if (batch < DT_TILE_ROUNDS_BATCH_MAX) batch *= 2;
  }
}
// A private diagnostic, not part of the C ABI (not in descriptools_hip.h, not bound by _lib): the tile visits of the
// last dt_dinf_distance_down call that THIS THREAD made and that succeeded -- per thread, so that another thread's
// call cannot land between a call and the question.  tools/dinf_distance_bench.py asks it by name.
static thread_local int64_t t_dinf_distance_visits = 0;
extern "C" int64_t dt_dinf_distance_visits_(void) { return t_dinf_distance_visits; }
extern "C" int dt_dinf_distance_down(const float *angle, const int8_t *river, const float *dem, int64_t H, int64_t W,
                                     double px, int stat, int check_edges, int visit_limit, double *h, double *v,
                                     double *s, int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_REQUIRE(stat >= 0 && stat <= 2, "stat is 0 (ave), 1 (min) or 2 (max)");
  DT_REQUIRE(check_edges == 0 || check_edges == 1, "check_edges is 0 or 1");
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  DT_REQUIRE(dem || (!v && !s), "the vertical and the surface distance need heights");
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(angle && river && h, "NULL raster");
  const bool z = dem && (v || s);
  const float *d_a = hc.in(angle, n);
  const int8_t *d_r = hc.in(river, n);
  const float *d_z = z ? hc.in(dem, n) : nullptr;
  double *d_h = hc.out(h, n);
  double *d_v = !z ? nullptr : (v ? hc.out(v, n) : hc.scratch<double>(n));  // the kernel computes both or neither
  double *d_s = !z ? nullptr : (s ? hc.out(s, n) : hc.scratch<double>(n));
  const size_t need = dt_dinf_distance_scratch(H, W);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  int32_t st = 0;
  DT_TRY(dt_ctx_status(hc.c, &st));  // this call's status only
  int64_t rounds;
  DT_TRY(host_tile_rounds(hc, dt_dinf_distance_ctl(scr, H, W), &rounds, [&](int start, int batch) -> int {
    DT_REQUIRE(rounds <= (int64_t)n, "more rounds than cells (a defect: every round but the last settles a cell)");
    return dt_launch_dinf_distance(hc.c->stream, d_a, d_r, d_z, H, W, px, stat, check_edges, visit_limit, start, batch,
                                   0, scr, need, d_h, d_v, d_s, hc.c->status);
  }));
  DT_TRY(dt_launched(dt_launch_dinf_distance(hc.c->stream, d_a, d_r, d_z, H, W, px, stat, check_edges, visit_limit, 0,
                                             0, 1, scr, need, d_h, d_v, d_s, hc.c->status)));
  uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
  DT_TRY(hc.download(cnt, dt_dinf_distance_ctl(scr, H, W) + DT_TILE_ROUNDS_BATCH_MAX, 6));
  DT_TRY(dt_ctx_status(hc.c, &st));  // (synchronises)
  DT_REQUIRE(!(st & DT_STATUS_BAD_ANGLE), "an angle is neither -1, -100 nor in [0, float32(2 pi)]");
  if (info4) {
    info4[0] = rounds;
    info4[1] = cnt[0];
    info4[2] = cnt[1];
    info4[3] = cnt[2];
  }
  t_dinf_distance_visits = (int64_t)cnt[4] | (int64_t)cnt[5] << 32;
  return hc.finish();
}

extern "C" int dt_cost_distance(const float *friction, const int8_t *sources, int64_t H, int64_t W, double px,
                                int connectivity, int visit_limit, double *cost, int64_t *indices, uint8_t *backlink,
                                int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity is 4 or 8");
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(friction && sources && cost, "NULL raster");
  const float *d_f = hc.in(friction, n);
  const int8_t *d_s = hc.in(sources, n);
  double *d_c = hc.out(cost, n);
  int64_t *d_i = hc.out(indices, n);
  uint8_t *d_b = hc.out(backlink, n);
  const int alloc = indices != nullptr;
  const size_t need = dt_cost_distance_scratch(H, W, alloc);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  const uint32_t *ctl = dt_cost_distance_ctl(scr, H, W, alloc);
  int64_t rounds;
  DT_TRY(host_tile_rounds(hc, ctl, &rounds, [&](int start, int batch) {
    return dt_launch_cost_distance(hc.c->stream, d_f, d_s, H, W, px, connectivity, visit_limit, start, batch, 0, scr,
                                   need, d_c, d_i, d_b, nullptr);
  }));
  DT_TRY(dt_launched(dt_launch_cost_distance(hc.c->stream, d_f, d_s, H, W, px, connectivity, visit_limit, 0, 0, 1, scr,
                                             need, d_c, d_i, d_b, nullptr)));
  uint32_t cnt[4] = {0, 0, 0, 0};
  DT_TRY(hc.download(cnt, ctl + DT_COST_CTL_COUNTS, 4));
  DT_TRY(hc.finish());  // (synchronises: cnt is here)
  if (info4) {
    info4[0] = rounds;
    info4[1] = cnt[0];
    info4[2] = cnt[1];
    info4[3] = (int64_t)cnt[2] | (int64_t)cnt[3] << 32;
  }
  return DT_OK;
}

// The modified area of device rasters within a host call: batches of rounds until a quiet one, then the fills and the
// counts -> cnt4 = {rounds that raised something, raised cells, tile visits, 0}.  Synchronises.
static int host_wetness_area(HostCall &hc, const double *d_a, const float *d_s, int64_t H, int64_t W, int visit_limit,
                             char *scr, size_t need, double *d_m, int64_t *cnt4) {
  const uint32_t *ctl = dt_wetness_ctl(scr, H, W);
  int64_t rounds;
  DT_TRY(host_tile_rounds(hc, ctl, &rounds, [&](int start, int batch) {
    return dt_launch_wetness_area(hc.c->stream, d_a, d_s, H, W, visit_limit, start, batch, 0, scr, need, d_m, nullptr);
  }));
  DT_TRY(dt_launched(dt_launch_wetness_area(hc.c->stream, d_a, d_s, H, W, visit_limit, 0, 0, 1, scr, need, d_m,
                                            nullptr)));
  uint32_t cnt[4] = {0, 0, 0, 0};
  DT_TRY(hc.download(cnt, ctl + DT_WETNESS_CTL_COUNTS, 4));
  DT_HIP(hipStreamSynchronize(hc.c->stream));
  cnt4[0] = rounds;
  cnt4[1] = cnt[0];
  cnt4[2] = (int64_t)cnt[2] | (int64_t)cnt[3] << 32;
  cnt4[3] = 0;
  return DT_OK;
}

extern "C" int dt_wetness_suction(const float *slope, int64_t H, int64_t W, double t, double weight, double offset,
                                  double minimum, float *suction) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_TRY(dt_check_wetness(t, weight, offset, minimum, true, false));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(slope && suction, "NULL raster");
  const float *d_sl = hc.in(slope, n);
  float *d_s = hc.out(suction, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_wetness_suction(hc.c->stream, d_sl, (int64_t)n, std::log(t), weight, offset, minimum,
                                               d_s)));
  return hc.finish();
}

extern "C" int dt_wetness_modified_area(const double *area, const float *suction, int64_t H, int64_t W,
                                        int visit_limit, double *modified, int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(area && suction && modified, "NULL raster");
  const double *d_a = hc.in(area, n);
  const float *d_s = hc.in(suction, n);
  double *d_m = hc.out(modified, n);
  const size_t need = dt_wetness_scratch(H, W, 0, 0);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  int64_t cnt4[4];
  DT_TRY(host_wetness_area(hc, d_a, d_s, H, W, visit_limit, scr, need, d_m, cnt4));
  DT_TRY(hc.finish());
  if (info4) memcpy(info4, cnt4, sizeof(cnt4));
  return DT_OK;
}

extern "C" int dt_wetness_saga(const double *area, const float *slope, int64_t H, int64_t W, double t, double weight,
                               double offset, double minimum, int visit_limit, float *swi, double *modified,
                               float *suction, int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_TRY(dt_check_wetness(t, weight, offset, minimum, true, true));
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(area && slope && swi, "NULL raster");
  const double *d_a = hc.in(area, n);
  const float *d_sl = hc.in(slope, n);
  float *d_w = hc.out(swi, n);
  // the planes the caller does not ask for live in the scratch; nothing crosses PCIe between the three stages
  double *d_m = hc.out(modified, n);
  float *d_s = hc.out(suction, n);
  const int own_s = d_s == nullptr, own_m = d_m == nullptr;
  const size_t need = dt_wetness_scratch(H, W, own_s, own_m);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  if (own_s) d_s = dt_wetness_suction_plane(scr, H, W);
  if (own_m) d_m = dt_wetness_m_plane(scr, H, W, own_s);
  DT_TRY(dt_launched(dt_launch_wetness_suction(hc.c->stream, d_sl, (int64_t)n, std::log(t), weight, offset, minimum,
                                               d_s)));
  int64_t cnt4[4];
  DT_TRY(host_wetness_area(hc, d_a, d_s, H, W, visit_limit, scr, need, d_m, cnt4));
  DT_TRY(dt_launched(dt_launch_wetness_index(hc.c->stream, d_m, d_sl, (int64_t)n, offset, minimum, d_w)));
  DT_TRY(hc.finish());
  if (info4) memcpy(info4, cnt4, sizeof(cnt4));
  return DT_OK;
}

// resampling: a bad argument is refused before the device is asked for
extern "C" int dt_resample(const void *src, int dtype, int64_t Hs, int64_t Ws, const double *matrix, int method,
                           int64_t nodata, uint64_t fill_bits, void *dst, int64_t Hd, int64_t Wd) {
  DT_TRY(dt_check_resample(dtype, Hs, Ws, matrix, method, nodata, Hd, Wd));
  DT_REQUIRE(src && dst, "NULL raster");
  HostCall hc;
  DT_TRY(hc.rc);
  const size_t es = dtype == 32 ? 4 : dtype == 64 ? 8 : (size_t)dtype;
  const unsigned char *d_src = hc.in((const unsigned char *)src, (size_t)Hs * Ws * es);
  unsigned char *d_dst = hc.out((unsigned char *)dst, (size_t)Hd * Wd * es);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_resample(hc.c->stream, d_src, dtype, Hs, Ws, matrix, method, nodata, fill_bits, d_dst,
                                        Hd, Wd)));
  return hc.finish();
}

// vector rasterisation: what the host entries require of the geometry's host arrays before they read them
static int dt_check_parts(const double *coords, const int64_t *parts, int64_t P, int64_t *N) {
  DT_REQUIRE(P >= 0 && P < (1ll << 31), "P must be in [0, 2^31)");
  *N = 0;
  if (P == 0) return DT_OK;
  DT_REQUIRE(parts, "parts is NULL");
  DT_REQUIRE(parts[0] == 0, "parts must start at 0");
  for (int64_t p = 0; p < P; p++) DT_REQUIRE(parts[p] <= parts[p + 1], "parts must not decrease");
  DT_REQUIRE(parts[P] < (1ll << 31), "2^31 vertices or more");
  DT_REQUIRE(coords || parts[P] == 0, "coords is NULL");
  *N = parts[P];
  return DT_OK;
}
// the exact work count of a geometry: pure host arithmetic, no device is asked for
extern "C" int dt_rasterize_count(int kind, const double *coords, const int64_t *parts, int64_t P, int64_t H, int64_t W,
                                  int64_t *total, int64_t *largest_row) {
  int64_t N = 0;
  DT_TRY(dt_check_parts(coords, parts, P, &N));
  DT_TRY(dt_check_rasterize(kind, P, N, H, W, 8, 0, 0));
  DT_REQUIRE(total && largest_row, "NULL result");
  *total = *largest_row = 0;
  if (kind == 0 && N > 0) dt_rasterize_count_host(coords, parts, P, H, total, largest_row);
  return DT_OK;
}
// a bad argument is refused before the device is asked for; the scratch is sized from the exact count
extern "C" int dt_rasterize(int kind, const double *coords, const int64_t *parts, const int32_t *ids, int64_t P,
                            int64_t H, int64_t W, int connectivity, int all_touched, int32_t *label, int64_t *info4) {
  int64_t N = 0, total = 0, largest = 0;
  DT_TRY(dt_check_parts(coords, parts, P, &N));
  DT_TRY(dt_check_rasterize(kind, P, N, H, W, connectivity, all_touched, 0));
  DT_REQUIRE(label && (ids || P == 0), "NULL label or ids");
  if (kind == 0 && N > 0) dt_rasterize_count_host(coords, parts, P, H, &total, &largest);
  DT_REQUIRE(total < (1ll << 31), "the geometry crosses the rows' centre lines 2^31 times or more");
  HostCall hc;
  DT_TRY(hc.rc);
  const double *d_c = hc.in(coords, (size_t)N * 2);
  const int64_t *d_p = hc.in(parts, (size_t)P + 1);
  const int32_t *d_i = hc.in(ids, (size_t)P);
  int32_t *d_l = hc.out(label, (size_t)H * W);
  int64_t scratch4[4];
  int64_t *d_info = hc.out(info4 ? info4 : scratch4, 4);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_rasterize(hc.c, kind, d_c, d_p, d_i, P, N, H, W, connectivity, all_touched, total, d_l, d_info));
  return hc.finish();
}

// polygonisation: the count phase on the device, info2 = {edges, corners}
static int host_polygonize_count(HostCall &hc, const int32_t *d_lab, int64_t H, int64_t W, int64_t *info8) {
  int64_t *d_info = hc.scratch<int64_t>(8);
  DT_TRY(hc.rc);
  DT_TRY(dev_polygonize(hc.c, d_lab, H, W, 0, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, d_info, nullptr));
  DT_TRY(hc.download(info8, d_info, 8));
  return dt_ctx_sync(hc.c);
}
extern "C" int dt_polygonize_count(const int32_t *labels, int64_t H, int64_t W, int64_t *info2) {
  DT_TRY(dt_check_polygonize(H, W, 0, 0, 0));
  DT_REQUIRE(labels && info2, "NULL labels or info");
  HostCall hc;
  DT_TRY(hc.rc);
  const int32_t *d_lab = hc.in(labels, (size_t)H * W);
  int64_t info8[8];
  DT_TRY(host_polygonize_count(hc, d_lab, H, W, info8));
  info2[0] = info8[0];
  info2[1] = info8[1];
  return hc.finish();
}
// a bad argument is refused before the device is asked for; the edge scratch is sized from the count phase.  The rings
// come back only when they fit: an overflow leaves the outputs untouched and says so in info8[5]
extern "C" int dt_polygonize(const int32_t *labels, int64_t H, int64_t W, int64_t cap_vertices, int64_t cap_rings,
                             double *coords, int64_t *parts, int32_t *ids, int32_t *shell, int64_t *info8) {
  DT_TRY(dt_check_polygonize(H, W, 0, cap_vertices, cap_rings));
  DT_REQUIRE(labels, "NULL labels");
  DT_REQUIRE(coords && parts && ids && shell && info8, "NULL coords, parts, ids, shell or info");
  HostCall hc;
  DT_TRY(hc.rc);
  const int32_t *d_lab = hc.in(labels, (size_t)H * W);
  int64_t cnt[8];
  DT_TRY(host_polygonize_count(hc, d_lab, H, W, cnt));
  DT_REQUIRE(cnt[0] < (1ll << 31), "the raster has 2^31 directed boundary edges or more");
  double *d_c = hc.scratch<double>((size_t)cap_vertices * 2);
  int64_t *d_p = hc.scratch<int64_t>((size_t)cap_rings + 1);
  int32_t *d_i = hc.scratch<int32_t>((size_t)cap_rings);
  int32_t *d_s = hc.scratch<int32_t>((size_t)cap_rings);
  int64_t *d_info = hc.scratch<int64_t>(8);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_polygonize(hc.c, d_lab, H, W, cnt[0], cap_vertices, cap_rings, d_c, d_p, d_i, d_s, d_info));
  DT_TRY(hc.download(info8, d_info, 8));
  DT_TRY(dt_ctx_sync(hc.c));
  if (info8[5] == 0) {
    const size_t V = (size_t)info8[1], P = (size_t)info8[2];
    DT_TRY(hc.download(coords, d_c, V * 2));
    DT_TRY(hc.download(parts, d_p, P + 1));
    DT_TRY(hc.download(ids, d_i, P));
    DT_TRY(hc.download(shell, d_s, P));
  }
  return hc.finish();
}

// geodesic reconstruction: batches of rounds until a quiet one, then the output and the counts
extern "C" int dt_morph_reconstruct(int mode, int erosion, int connectivity, const float *mask, const float *marker,
                                    const uint8_t *seeds, double h, int radius, int64_t H, int64_t W, int visit_limit,
                                    float *out, uint8_t *out8, int64_t *info4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_TRY(dt_check_morph(mode, erosion, connectivity, h, radius, visit_limit));
  if (info4) info4[0] = info4[1] = info4[2] = info4[3] = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_TRY(dt_check_morph_rasters(mode, mask, marker, out, out8));
  const float *d_mask = hc.in(mask, n);
  const float *d_marker = mode == DT_MORPH_MARKER ? hc.in(marker, n) : nullptr;
  const uint8_t *d_seeds = mode == DT_MORPH_OUTLETS ? hc.in(seeds, n) : nullptr;
  float *d_out = hc.out(out, n);
  uint8_t *d_out8 = hc.out(out8, n);
  const size_t need = dt_morph_scratch(H, W, mode, out8 != nullptr);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  const uint32_t *ctl = dt_morph_ctl(scr, H, W);
  int64_t rounds;
  DT_TRY(host_tile_rounds(hc, ctl, &rounds, [&](int start, int batch) {
    return dt_launch_morph(hc.c->stream, mode, erosion, connectivity, d_mask, d_marker, d_seeds, h, radius, H, W,
                           visit_limit, start, batch, 0, scr, need, d_out, d_out8, nullptr);
  }));
  DT_TRY(dt_launched(dt_launch_morph(hc.c->stream, mode, erosion, connectivity, d_mask, d_marker, d_seeds, h, radius, H,
                                     W, visit_limit, 0, 0, 1, scr, need, d_out, d_out8, nullptr)));
  uint32_t cnt[4] = {0, 0, 0, 0};
  DT_TRY(hc.download(cnt, ctl + DT_MORPH_CTL_COUNTS, 4));
  DT_TRY(hc.finish());
  if (info4) {
    info4[0] = rounds;
    info4[1] = cnt[0];
    info4[2] = (int64_t)cnt[2] | (int64_t)cnt[3] << 32;
  }
  return DT_OK;
}

// (the batches of host_tile_rounds per level of the pyramid, on residual keys and within the budget of rounds)
extern "C" int dt_harmonic(const float *values, const int8_t *fixed, const int8_t *domain, int64_t H, int64_t W,
                           double tol, int max_rounds, double *out, int64_t *info) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_TRY(dt_check_harmonic(tol, max_rounds));
  if (info) memset(info, 0, sizeof(int64_t) * DT_HARMONIC_INFO);
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(values && fixed && out, "NULL raster");
  const float *d_v = hc.in(values, n);
  const int8_t *d_f = hc.in(fixed, n);
  const int8_t *d_d = hc.in(domain, n);
  double *d_o = hc.out(out, n);
  const int cap = dt_harmonic_level_cap();
  const size_t need = dt_harmonic_scratch(H, W, max_rounds, cap);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  hipStream_t s = hc.c->stream;
  DT_TRY(dt_launch_harmonic_setup(s, d_v, d_f, d_d, H, W, max_rounds, cap, scr, need, d_o));
  unsigned long long keys[DT_TILE_ROUNDS_BATCH_MAX];
  unsigned long long tol_key;
  memcpy(&tol_key, &tol, sizeof(tol_key));
  for (int l = dt_harmonic_levels(H, W, cap) - 1; l >= 0; l--) {
    const unsigned long long *d_keys = dt_harmonic_keys(scr, H, W, max_rounds, cap, l);
    int batch = DT_TILE_ROUNDS_BATCH0;
    for (int first = 0; first < max_rounds;) {
      const int b = batch < max_rounds - first ? batch : max_rounds - first;
      DT_TRY(dt_launch_harmonic_rounds(s, H, W, max_rounds, cap, l, first, b, tol, scr, need, d_o));
      DT_TRY(hc.download(keys, d_keys + first, (size_t)b));
      DT_HIP(hipStreamSynchronize(s));
      if (keys[b - 1] <= tol_key) break;  // (a round behind one that met tol hands its key on)
      first += b;
      if (batch < DT_TILE_ROUNDS_BATCH_MAX) batch *= 2;
    }
    if (l) DT_TRY(dt_launch_harmonic_prolong(s, H, W, max_rounds, cap, l, scr, need, d_o));
  }
  DT_TRY(dt_launched(dt_launch_harmonic_finish(s, H, W, max_rounds, cap, tol, scr, need, nullptr, nullptr)));
  int64_t got[DT_HARMONIC_INFO];
  DT_TRY(hc.download(got, dt_harmonic_info(scr, H, W, max_rounds, cap), (size_t)DT_HARMONIC_INFO));
  DT_TRY(hc.finish());  // (synchronises: got is here)
  if (info) memcpy(info, got, sizeof(got));
  return DT_OK;
}

// (batches of sync_every guarded steps; the control block's "no step is left" word is read back after each)
extern "C" int dt_inundation(const float *z, const float *manning, const float *rain, int64_t H, int64_t W,
                             const double *par, int boundary, const int64_t *cells, const double *times,
                             const double *discharge, int K, int T, int64_t steps0, int64_t max_steps, int sync_every,
                             double *h, double *qx, double *qy, double *max_depth, double *arrival, int64_t *info) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, par ? par[0] : 0.0));
  DT_TRY(dt_check_inundation(par, manning, rain, boundary, K, T, steps0));
  DT_REQUIRE(max_steps >= -1, "max_steps must be >= 0, or -1 for no limit");
  DT_REQUIRE(sync_every >= 1 && sync_every <= 1024, "sync_every must lie in [1, 1024]");
  if (info) memset(info, 0, sizeof(int64_t) * DT_INUNDATION_INFO_WORDS);
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(z && h && qx && qy, "NULL raster");
  DT_REQUIRE(K == 0 || (cells && times && discharge), "NULL inflow table");
  for (int j = 0; j < K; j++) DT_REQUIRE(cells[j] >= 0 && (size_t)cells[j] < n, "inflow cell outside the raster");
  for (int j = 1; j < (K ? T : 0); j++) DT_REQUIRE(times[j] > times[j - 1], "inflow times must ascend strictly");
  for (size_t j = 0; j < (size_t)K * (size_t)T; j++)
    DT_REQUIRE(std::isfinite(discharge[j]) && discharge[j] >= 0.0, "discharge must be finite and >= 0");
  const float *d_z = hc.in(z, n), *d_m = hc.in(manning, n), *d_r = hc.in(rain, n);
  double *d_h = hc.in(h, n), *d_qx = hc.in(qx, n), *d_qy = hc.in(qy, n);
  double *d_md = hc.in(max_depth, n), *d_ar = hc.in(arrival, n);
  const int64_t *d_c = K ? hc.in(cells, (size_t)K) : nullptr;
  const double *d_t = K ? hc.in(times, (size_t)T) : nullptr;
  const double *d_q = K ? hc.in(discharge, (size_t)K * (size_t)T) : nullptr;
  int64_t *d_info = hc.scratch<int64_t>(DT_INUNDATION_INFO_WORDS);
  const size_t need = dt_inundation_scratch(H, W);
  char *scr = hc.scratch<char>(need);
  DT_TRY(hc.rc);
  hipStream_t s = hc.c->stream;
  const DtInundation call = dt_inundation_call(d_z, d_m, d_r, H, W, par, boundary, d_c, d_t, d_q, K, T, max_steps, d_h,
                                               d_qx, d_qy, d_md, d_ar);
  DT_TRY(dt_launch_inundation_begin(s, call, par[1], steps0, scr, need));
  const unsigned long long *d_ctl = dt_inundation_ctl(scr, H, W);
  unsigned long long ctl[DT_IN_CTL];
  for (;;) {
    DT_TRY(hc.download(ctl, d_ctl, (size_t)DT_IN_CTL));
    DT_HIP(hipStreamSynchronize(s));
    if (ctl[3]) break;  // no step is left
    DT_TRY(dt_launched(dt_launch_inundation_steps(s, call, sync_every, scr, need)));
  }
  DT_TRY(dt_launched(dt_launch_inundation_finish(s, call, scr, need, d_info)));
  int64_t got[DT_INUNDATION_INFO_WORDS];
  DT_TRY(hc.download(got, (const int64_t *)d_info, (size_t)DT_INUNDATION_INFO_WORDS));
  DT_TRY(hc.download(h, (const double *)d_h, n));
  DT_TRY(hc.download(qx, (const double *)d_qx, n));
  DT_TRY(hc.download(qy, (const double *)d_qy, n));
  if (max_depth) DT_TRY(hc.download(max_depth, (const double *)d_md, n));
  if (arrival) DT_TRY(hc.download(arrival, (const double *)d_ar, n));
  DT_TRY(hc.finish());  // (synchronises: got is here)
  if (info) memcpy(info, got, sizeof(got));
  return DT_OK;
}

extern "C" int dt_proximity(const int8_t *river, const float *nod, int64_t H, int64_t W, double px, float *distance,
                            int64_t *indices) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(river && distance && indices, "NULL raster");
  const int8_t *d_r = hc.in(river, n);
  const float *d_n = hc.in(nod, n);
  float *d_d = hc.out(distance, n);
  int64_t *d_i = hc.out(indices, n);
  DT_TRY(hc.rc);
  const size_t need = dt_proximity_scratch(H, W);
  DT_TRY(dt_scratch_reset(hc.c, need));
  void *scr = dt_scratch_take(hc.c, need);
  DT_REQUIRE(scr, "scratch reservation failed");
  DT_TRY(dt_launched(dt_launch_proximity(hc.c->stream, d_r, d_n, H, W, px, scr, need, d_d, d_i)));
  return hc.finish();
}

extern "C" int dt_reach_catchments(const int64_t *link, const int64_t *idx, int64_t H, int64_t W, int32_t *reach,
                                   int32_t *catch_, int64_t *heads, int64_t cap, int64_t *n_reaches) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_REQUIRE(n_reaches && cap >= 0 && (heads || cap == 0), "bad arguments");
  *n_reaches = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(link && (idx || !catch_), "NULL raster");
  if ((size_t)cap > n) cap = (int64_t)n;
  const int64_t *d_l = hc.in(link, n);
  const int64_t *d_i = catch_ ? hc.in(idx, n) : nullptr;
  int32_t *d_r = hc.out(reach, n);
  int32_t *d_c = hc.out(catch_, n);
  int64_t *d_h = cap ? hc.out(heads, (size_t)cap) : nullptr;
  int64_t *d_n = hc.scratch<int64_t>(1);
  DT_TRY(hc.rc);
  if (d_h) DT_HIP(hipMemsetAsync(d_h, 0xFF, (size_t)cap * 8, hc.c->stream));  // -1 beyond the last head
  DT_TRY(dt_dev_reach_catchments(hc.c, d_l, d_i, 8, H, W, d_r, d_c, d_h, cap, d_n));
  DT_TRY(hc.download(n_reaches, (const int64_t *)d_n, 1));
  return hc.finish();
}

extern "C" int dt_reach_channels(const uint8_t *fdr, const int32_t *reach, int64_t H, int64_t W, int64_t R,
                                 int64_t *end, int64_t *down, int64_t *n_cells, int64_t *n_card, int64_t *n_diag) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_TRY(dt_check_reach_count(R));
  if (R == 0) return DT_OK;
  DT_REQUIRE(end && down && n_cells && n_card && n_diag, "NULL output");
  const size_t n = (size_t)H * W;
  DT_REQUIRE((fdr && reach) || n == 0, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const int32_t *d_r = hc.in(reach, n);
  int64_t *d_e = hc.out(end, (size_t)R), *d_d = hc.out(down, (size_t)R), *d_n = hc.out(n_cells, (size_t)R);
  int64_t *d_nc = hc.out(n_card, (size_t)R), *d_nd = hc.out(n_diag, (size_t)R);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_reach_channels(hc.c, d_f, d_r, H, W, R, d_e, d_d, d_n, d_nc, d_nd));
  return hc.finish();
}

extern "C" int dt_reach_tables(const int32_t *catch_, const void *hand, int hand_bytes, const float *slope, int64_t H,
                               int64_t W, const double *stages, int K, int64_t R, int frac_bits, int64_t *cells,
                               int64_t *Hq, int64_t *Bq) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_TRY(dt_check_reach_count(R));
  DT_TRY(dt_check_stages(stages, K, frac_bits, H * W));
  DT_REQUIRE(hand_bytes == 4 || hand_bytes == 8, "hand's element size must be 4 or 8");
  if (R == 0) return DT_OK;
  DT_REQUIRE(cells && Hq && Bq, "NULL table");
  const size_t n = (size_t)H * W, rk = (size_t)R * (size_t)K;
  DT_REQUIRE((catch_ && hand) || n == 0, "NULL raster");
  const int32_t *d_c = hc.in(catch_, n);
  const unsigned char *d_h = hc.in((const unsigned char *)hand, n * (size_t)hand_bytes);
  const float *d_s = hc.in(slope, n);
  int64_t *d_n = hc.out(cells, rk), *d_hq = hc.out(Hq, rk), *d_bq = hc.out(Bq, rk);
  DT_TRY(hc.rc);
  int32_t st = 0;
  DT_TRY(dt_ctx_status(hc.c, &st));  // this call's status only
  DT_TRY(dt_dev_reach_tables(hc.c, d_c, d_h, hand_bytes, d_s, H, W, stages, K, R, frac_bits, d_n, d_hq, d_bq));
  DT_TRY(dt_ctx_status(hc.c, &st));
  DT_REQUIRE(!(st & DT_STATUS_BAD_WEIGHT), "a bed weight sqrt(1 + (slope / 100)^2) is over the bound of frac_bits");
  DT_REQUIRE(!(st & DT_STATUS_REACH_RANGE), "a catchment id is >= the number of reaches");
  return hc.finish();
}

extern "C" int dt_inundate(const int32_t *catch_, const void *hand, int hand_bytes, const double *stage, int64_t H,
                           int64_t W, int64_t R, float *depth) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_TRY(dt_check_reach_count(R));
  DT_REQUIRE(hand_bytes == 4 || hand_bytes == 8, "hand's element size must be 4 or 8");
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(catch_ && hand && depth && (stage || R == 0), "NULL raster");
  const int32_t *d_c = hc.in(catch_, n);
  const unsigned char *d_h = hc.in((const unsigned char *)hand, n * (size_t)hand_bytes);
  const double *d_s = hc.in(stage, (size_t)R);
  float *d_d = hc.out(depth, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_inundate(hc.c, d_c, d_h, hand_bytes, d_s, H, W, R, d_d));
  return hc.finish();
}

extern "C" int dt_zonal_compact(const void *labels, int label_bytes, int64_t H, int64_t W, int64_t limit,
                                int32_t *zones, int64_t *labels_of, int64_t cap, int64_t *n_zones) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_TRY(dt_check_zonal_compact(label_bytes, limit, cap));
  DT_REQUIRE(n_zones && (labels_of || cap == 0), "bad arguments");
  *n_zones = 0;
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(labels, "NULL raster");
  if (cap > limit) cap = limit;
  const unsigned char *d_l = hc.in((const unsigned char *)labels, n * (size_t)label_bytes);
  int32_t *d_z = hc.out(zones, n);
  int64_t *d_o = cap ? hc.out(labels_of, (size_t)cap) : nullptr;
  int64_t *d_n = hc.scratch<int64_t>(1);
  DT_TRY(hc.rc);
  if (d_o) DT_HIP(hipMemsetAsync(d_o, 0xFF, (size_t)cap * 8, hc.c->stream));  // -1 beyond the last zone
  DT_TRY(dt_dev_zonal_compact(hc.c, d_l, label_bytes, H, W, limit, d_z, d_o, cap, d_n));
  DT_TRY(hc.download(n_zones, (const int64_t *)d_n, 1));
  return hc.finish();
}

extern "C" int dt_zonal_tables(const int32_t *zones, const void *values, int value_bytes, int64_t H, int64_t W,
                               int64_t n_zones, double origin, int frac_bits, int has_nodata, double nodata,
                               int64_t *count, int64_t *s1, uint64_t *s2_lo, uint64_t *s2_hi, void *vmin, void *vmax) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_TRY(dt_check_zonal_tables(n_zones, value_bytes, origin, frac_bits, s2_lo, s2_hi));
  if (n_zones == 0) return DT_OK;
  DT_REQUIRE(count || s1 || s2_lo || vmin || vmax, "no table");
  const size_t n = (size_t)H * W, z = (size_t)n_zones;
  DT_REQUIRE((zones && values) || n == 0, "NULL raster");
  const int32_t *d_z = hc.in(zones, n);
  const unsigned char *d_v = hc.in((const unsigned char *)values, n * (size_t)value_bytes);
  int64_t *d_c = hc.out(count, z), *d_s1 = hc.out(s1, z);
  uint64_t *d_lo = hc.out(s2_lo, z), *d_hi = hc.out(s2_hi, z);
  unsigned char *d_mn = hc.out((unsigned char *)vmin, z * (size_t)value_bytes);
  unsigned char *d_mx = hc.out((unsigned char *)vmax, z * (size_t)value_bytes);
  DT_TRY(hc.rc);
  int32_t st = 0;
  DT_TRY(dt_ctx_status(hc.c, &st));  // this call's status only
  DT_TRY(dt_dev_zonal_tables(hc.c, d_z, d_v, value_bytes, H, W, n_zones, origin, frac_bits, has_nodata, nodata, d_c,
                             d_s1, d_lo, d_hi, d_mn, d_mx));
  DT_TRY(dt_ctx_status(hc.c, &st));
  DT_REQUIRE(!(st & DT_STATUS_BAD_HEIGHT), "a value's |rint((v - origin) * 2^frac_bits)| exceeds 2^31 - 1");
  DT_REQUIRE(!(st & DT_STATUS_ZONE_RANGE), "a zone id is >= the number of zones");
  return hc.finish();
}

extern "C" int dt_zonal_counts(const int32_t *zones, const void *values, int value_bytes, int64_t H, int64_t W,
                               int64_t n_zones, const double *edges, int K, int has_nodata, double nodata,
                               int64_t *counts) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_TRY(dt_check_zonal_counts(n_zones, value_bytes, edges, K));
  if (n_zones == 0) return DT_OK;
  DT_REQUIRE(counts, "NULL table");
  const size_t n = (size_t)H * W;
  DT_REQUIRE((zones && values) || n == 0, "NULL raster");
  const int32_t *d_z = hc.in(zones, n);
  const unsigned char *d_v = hc.in((const unsigned char *)values, n * (size_t)(value_bytes ? value_bytes : 4));
  int64_t *d_c = hc.out(counts, (size_t)n_zones * (size_t)K);
  DT_TRY(hc.rc);
  int32_t st = 0;
  DT_TRY(dt_ctx_status(hc.c, &st));  // this call's status only
  DT_TRY(dt_dev_zonal_counts(hc.c, d_z, d_v, value_bytes, H, W, n_zones, edges, K, has_nodata, nodata, d_c));
  DT_TRY(dt_ctx_status(hc.c, &st));
  DT_REQUIRE(!(st & DT_STATUS_ZONE_RANGE), "a zone id is >= the number of zones (or a column >= K)");
  return hc.finish();
}

extern "C" int dt_zonal_paint(const void *table, int elem_bytes, int64_t n_table, const int32_t *zones, int64_t H,
                              int64_t W, const void *fill, void *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  DT_TRY(dt_check_zone_count(n_table));
  DT_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "the table's element size must be 4 or 8");
  DT_REQUIRE(fill, "NULL fill");
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(zones && out && (table || n_table == 0), "NULL raster");
  const unsigned char *d_t = hc.in((const unsigned char *)table, (size_t)n_table * (size_t)elem_bytes);
  const int32_t *d_z = hc.in(zones, n);
  unsigned char *d_o = hc.out((unsigned char *)out, n * (size_t)elem_bytes);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_zonal_paint(hc.c, d_t, elem_bytes, n_table, d_z, H, W, fill, d_o));
  return hc.finish();
}

extern "C" int dt_regions_label(const uint8_t *mask, int64_t H, int64_t W, int connectivity, int64_t *label,
                                int64_t *size) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_TRY(dt_check_regions(connectivity, 1));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(mask && label, "NULL raster");
  const uint8_t *d_m = hc.in(mask, n);
  int64_t *d_l = hc.out(label, n);
  int64_t *d_s = hc.out(size, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_regions_label(hc.c, d_m, H, W, connectivity, d_l, d_s));
  return hc.finish();
}

extern "C" int dt_regions_select(const uint8_t *mask, const uint8_t *seeds, int64_t H, int64_t W, int connectivity,
                                 int64_t min_cells, uint8_t *keep) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_TRY(dt_check_regions(connectivity, min_cells));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(mask && keep, "NULL raster");
  const uint8_t *d_m = hc.in(mask, n);
  const uint8_t *d_s = hc.in(seeds, n);
  uint8_t *d_k = hc.out(keep, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_regions_select(hc.c, d_m, d_s, H, W, connectivity, min_cells, d_k));
  return hc.finish();
}

extern "C" int dt_inundate_connected(const int32_t *catch_, const void *hand, int hand_bytes, const double *stage,
                                     const int8_t *river, int64_t H, int64_t W, int64_t R, int connectivity,
                                     float *depth) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, 1.0));
  DT_TRY(dt_check_reach_count(R));
  DT_REQUIRE(hand_bytes == 4 || hand_bytes == 8, "hand's element size must be 4 or 8");
  DT_TRY(dt_check_regions(connectivity, 1));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(catch_ && hand && river && depth && (stage || R == 0), "NULL raster");
  const int32_t *d_c = hc.in(catch_, n);
  const unsigned char *d_h = hc.in((const unsigned char *)hand, n * (size_t)hand_bytes);
  const double *d_s = hc.in(stage, (size_t)R);
  const int8_t *d_r = hc.in(river, n);
  float *d_d = hc.out(depth, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_inundate_connected(hc.c, d_c, d_h, hand_bytes, d_s, d_r, H, W, R, connectivity, d_d));
  return hc.finish();
}

extern "C" int dt_flowhand(const float *dem, const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W,
                           double px, float *fdist, int64_t *idx, float *hand) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(fdr && river, "NULL raster");
  DT_REQUIRE(!hand || dem, "hand needs dem");
  const uint8_t *d_f = hc.in(fdr, n);
  const int8_t *d_r = hc.in(river, n);
  const float *d_dem = hand ? hc.in(dem, n) : nullptr;
  int32_t *d_i32 = idx ? hc.scratch<int32_t>(n) : nullptr;
  int64_t *d_i64 = hc.out(idx, n);
  float *d_fd = hc.out(fdist, n);
  float *d_h = hc.out(hand, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_flowhand(hc.c, d_dem, d_f, d_r, nullptr, H, W, px, d_fd, d_i32, d_h, nullptr));
  if (idx) DT_TRY(dt_dev_i32_to_i64(hc.c, d_i32, (int64_t)n, d_i64));
  return hc.finish();
}

extern "C" int dt_twi(const int64_t *fac, const float *slope_rad, int64_t N, double px, double n_top,
                      float *ti, float *mti) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0, "negative size");
  if (N == 0) return DT_OK;
  DT_REQUIRE(fac && slope_rad && ti && mti, "NULL raster");
  const int64_t *d_f = hc.in(fac, N);
  const float *d_s = hc.in(slope_rad, N);
  float *d_t = hc.out(ti, N);
  float *d_m = hc.out(mti, N);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_twi_i64(hc.c->stream, d_f, d_s, N, px, n_top, d_t, d_m)));
  return hc.finish();
}

extern "C" int dt_river_accumulation(const int64_t *fac, const int64_t *idx, int64_t N, int64_t *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0, "negative size");
  if (N == 0) return DT_OK;
  DT_REQUIRE(fac && idx && out, "NULL raster");
  const int64_t *d_f = hc.in(fac, N);
  const int64_t *d_i = hc.in(idx, N);
  int64_t *d_a = hc.out(out, N);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_river_acc_i64(hc.c->stream, d_f, d_i, N, d_a)));
  return hc.finish();
}

static int host_gfi(const float *hand, const int64_t *fac, const int64_t *idx, int64_t N, double n_gfi,
                    double b, double size, float *out, int own_cell) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0, "negative size");
  if (N == 0) return DT_OK;
  DT_REQUIRE(hand && fac && out, "NULL raster");
  const float *d_h = hc.in(hand, N);
  const int64_t *d_f = hc.in(fac, N);
  float *d_o = hc.out(out, N);
  const int64_t *d_i = hc.in(idx, N);
  int64_t *d_a = idx ? hc.scratch<int64_t>(N) : nullptr;
  DT_TRY(hc.rc);
  if (idx) DT_TRY(dt_launch_river_acc_i64(hc.c->stream, d_f, d_i, N, d_a));
  DT_TRY(dt_launched(dt_launch_gfi_i64(hc.c->stream, d_h, idx ? d_a : d_f, N, n_gfi, b, size, d_o, own_cell)));
  return hc.finish();
}
extern "C" int dt_gfi(const float *hand, const int64_t *fac, const int64_t *idx, int64_t N, double n_gfi,
                      double b, double size, float *gfi) {
  DT_REQUIRE(idx || N == 0, "idx is NULL");
  return host_gfi(hand, fac, idx, N, n_gfi, b, size, gfi, 0);
}
extern "C" int dt_lnhlh(const float *hand, const int64_t *fac, int64_t N, double n_gfi, double b, double size,
                        float *out) {
  return host_gfi(hand, fac, nullptr, N, n_gfi, b, size, out, 1);
}
extern "C" int dt_gfi_area(const float *hand, const int64_t *area, int64_t N, double n_gfi, double b,
                           double size, int zero_guard, float *out) {
  return host_gfi(hand, area, nullptr, N, n_gfi, b, size, out, zero_guard ? 1 : 0);
}

// HAND on the host tier, float32 or float64 heights
template <typename T>
static int host_hand(const T *dem, const int64_t *idx, int64_t N, T *hand,
                     int (*launch)(hipStream_t, const T *, const int64_t *, int64_t, T *)) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0, "negative size");
  if (N == 0) return DT_OK;
  DT_REQUIRE(dem && idx && hand, "NULL raster");
  const T *d_d = hc.in(dem, N);
  const int64_t *d_i = hc.in(idx, N);
  T *d_h = hc.out(hand, N);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(launch(hc.c->stream, d_d, d_i, N, d_h)));
  return hc.finish();
}
extern "C" int dt_hand_f32(const float *dem, const int64_t *idx, int64_t N, float *hand) {
  return host_hand(dem, idx, N, hand, dt_launch_hand_i64);
}

// ---- heights in float64 (dt_wide.hip): see include/descriptools_hip.h --------------------------------------------
extern "C" int dt_slope_f64(const double *dem, int64_t H, int64_t W, double px, float *slope) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && slope, "NULL raster");
  const double *d_d = hc.in(dem, n);
  float *d_s = hc.out(slope, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_slope_f64(hc.c->stream, d_d, H, W, px, d_s)));
  return hc.finish();
}
extern "C" int dt_d8_f64(const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *slope) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && fdr, "NULL raster");
  const double *d_d = hc.in(dem, n);
  uint8_t *d_f = hc.out(fdr, n);
  float *d_s = hc.out(slope, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_d8_f64(hc.c->stream, d_d, H, W, px, d_f, d_s, nullptr)));
  return hc.finish();
}
extern "C" int dt_hand_f64(const double *dem, const int64_t *idx, int64_t N, double *hand) {
  return host_hand(dem, idx, N, hand, dt_launch_hand_f64);
}
extern "C" int dt_downslope_f64(const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px, double dz,
                                int raw, float *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && fdr && out, "NULL raster");
  const double *d_d = hc.in(dem, n);
  const uint8_t *d_f = hc.in(fdr, n);
  float *d_o = hc.out(out, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_downslope_f64(hc.c->stream, d_d, d_f, H, W, px, dz, raw, d_o)));
  return hc.finish();
}
extern "C" int dt_gfi_f64h(const double *hand, const int64_t *fac, const int64_t *idx, int64_t N, double n_gfi,
                           double b, double size, int own_area, float *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0, "negative size");
  if (N == 0) return DT_OK;
  DT_REQUIRE(hand && fac && out && (own_area || idx), "NULL raster");
  const double *d_h = hc.in(hand, N);
  const int64_t *d_f = hc.in(fac, N);
  float *d_o = hc.out(out, N);
  const int64_t *d_i = own_area ? nullptr : hc.in(idx, N);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_gfi_f64h(hc.c->stream, d_h, d_f, d_i, N, n_gfi, b, size, own_area, d_o)));
  return hc.finish();
}

extern "C" int dt_downslope(const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px, double dz,
                            int raw, float *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && fdr && out, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  const uint8_t *d_f = hc.in(fdr, n);
  float *d_o = hc.out(out, n);
  DT_TRY(hc.rc);
  // Long walks (real, conditioned rasters walk thousands of moves through flats and along valley floors) are queued;
  // this call is synchronous anyway, so it looks at the queue and allocates the skip tables only for a raster that
  // has enough of them.  The plain kernel when the device has no room for the queue.
  const size_t qb = dt_flow_impl() == 1 ? 0 : (size_t)dt_downslope_queue_workspace(H, W);
  void *d_w = qb ? hc.workspace(qb) : nullptr;
  if (d_w) {
    DT_TRY(dt_dev_downslope_queue(hc.c, d_dem, d_f, H, W, px, dz, raw, d_o, d_w, (int64_t)qb));
    int64_t queued = 0;
    DT_TRY(dt_dev_downslope_queued(hc.c, d_w, &queued));
    if (queued > 0) {
      const size_t tb = (size_t)dt_downslope_tables_workspace(H, W);
      void *d_t = queued >= dt_downslope_tables_threshold(H, W) ? hc.workspace(tb) : nullptr;
      DT_TRY(dt_dev_downslope_finish(hc.c, d_dem, d_f, H, W, px, dz, raw, d_o, d_w, (int64_t)qb, d_t,
                                     d_t ? (int64_t)tb : 0));
    }
  } else {
    DT_TRY(dt_dev_downslope(hc.c, d_dem, d_f, H, W, px, dz, raw, d_o));
  }
  return hc.finish();
}

extern "C" int dt_confusion_multi(const double *desc, const int8_t *flood, int64_t N, double nodata_value,
                                  const double *th, int nth, int under, int64_t *counts4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0 && th && counts4 && nth >= 1, "bad arguments");
  const double *d_d = hc.in(desc, N);
  const int8_t *d_f = hc.in(flood, N);
  int64_t *d_c = hc.scratch<int64_t>(4 * 24);
  DT_TRY(hc.rc);
  // more than 24 thresholds: several passes over the resident rasters
  for (int t0 = 0; t0 < nth; t0 += 24) {
    int k = nth - t0 < 24 ? nth - t0 : 24;
    DT_TRY(dt_dev_confusion_multi(hc.c, d_d, d_f, N, nodata_value, th + t0, k, under, d_c));
    DT_TRY(hc.download(counts4 + (size_t)t0 * 4, d_c, (size_t)k * 4));
  }
  return hc.finish();
}

extern "C" int dt_threshold_hist(const double *desc, const int8_t *flood, int64_t N, double nodata_value,
                                 const double *th, int K, int under, int64_t *hist) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0 && th && hist && K >= 1 && K <= 65535, "bad arguments");
  DT_REQUIRE((desc && flood) || N == 0, "NULL raster");
  // what the device entry takes as a precondition: t[k] <= t[k + 1] is false for a descending pair and for a NaN
  DT_REQUIRE(th[0] == th[0], "a threshold is NaN");
  for (int k = 0; k + 1 < K; k++) DT_REQUIRE(th[k] <= th[k + 1], "thresholds are not sorted ascending (or one is NaN)");
  const double *d_d = hc.in(desc, N);
  const int8_t *d_f = hc.in(flood, N);
  const double *d_t = hc.in(th, K);
  int64_t *d_h = hc.out(hist, 2 * ((size_t)K + 1) + 1);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_threshold_hist(hc.c, d_d, d_f, N, nodata_value, d_t, K, under, d_h));
  return hc.finish();
}

// ---- evaluation.minMaxScale / binary_map / avaliacao, host tier --------------------------------------
// minMaxScale with the denominator mx - mn given (numpy subtracts the scalars from each other before they meet the
// raster); cell_bytes 2 / 4 / 8: a float16 / float32 / float64 raster in and out, computed in that type
extern "C" int dt_minmax_scale_den(const void *x, int cell_bytes, int64_t N, double mn, double den, double nodata,
                                   void *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0, "negative size");
  DT_REQUIRE(cell_bytes == 2 || cell_bytes == 4 || cell_bytes == 8, "cell_bytes is 2, 4 or 8");
  if (N == 0) return DT_OK;
  DT_REQUIRE(x && out, "NULL raster");
  const size_t bytes = (size_t)N * cell_bytes;
  const uint8_t *d_x = hc.in((const uint8_t *)x, bytes);
  uint8_t *d_o = hc.out((uint8_t *)out, bytes);
  DT_TRY(hc.rc);
  hipStream_t s = hc.c->stream;
  DT_TRY(dt_launched(
      cell_bytes == 2   ? dt_launch_minmax_scale_f16(s, d_x, N, (float)mn, (float)den, (float)nodata, d_o)
      : cell_bytes == 4 ? dt_launch_minmax_scale_den_f32(s, (const float *)d_x, N, (float)mn, (float)den, (float)nodata,
                                                         (float *)d_o)
                        : dt_launch_minmax_scale_den_f64(s, (const double *)d_x, N, mn, den, nodata, (double *)d_o)));
  return hc.finish();
}

// mn and mx given in the raster's own type: the denominator is T(mx) - T(mn)
extern "C" int dt_minmax_scale(const void *x, int is_f32, int64_t N, double mn, double mx, double nodata, void *out) {
  if (is_f32) return dt_minmax_scale_den(x, 4, N, (float)mn, (double)((float)mx - (float)mn), nodata, out);
  return dt_minmax_scale_den(x, 8, N, mn, mx - mn, nodata, out);
}

extern "C" int dt_binary_map(const void *desc, int is_f32, int64_t N, double nodata_value, double threshold, int under,
                             uint8_t *binary) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0, "negative size");
  if (N == 0) return DT_OK;
  DT_REQUIRE(desc && binary, "NULL raster");
  const float *d_d32 = is_f32 ? hc.in((const float *)desc, N) : nullptr;
  const double *d_d64 = is_f32 ? nullptr : hc.in((const double *)desc, N);
  int8_t *d_f = hc.scratch<int8_t>(N);
  uint8_t *d_b = hc.out(binary, N);
  unsigned long long *d_c = hc.scratch<unsigned long long>(4);
  DT_TRY(hc.rc);
  DT_HIP(hipMemsetAsync(d_f, 0, N, hc.c->stream));
  DT_TRY(dt_launched(is_f32 ? dt_launch_classify_f32(hc.c->stream, d_d32, nullptr, d_f, N, (float)nodata_value,
                                                     (float)threshold, under, 0, d_b, nullptr, d_c)
                            : dt_launch_classify_f64(hc.c->stream, d_d64, nullptr, d_f, N, nodata_value, threshold,
                                                     under, 0, d_b, nullptr, d_c)));
  return hc.finish();
}

extern "C" int dt_avaliacao(const int32_t *binary, int8_t *flood, int64_t N, int32_t *klass, int64_t *counts4) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_REQUIRE(N >= 0 && counts4, "bad arguments");
  DT_REQUIRE((binary && flood) || N == 0, "NULL raster");
  const int32_t *d_b = hc.in(binary, N);
  int8_t *d_f = hc.in(flood, N);
  int32_t *d_k = hc.scratch<int32_t>(N);
  int64_t *d_c = hc.out(counts4, 4);
  DT_TRY(hc.rc);
  DT_TRY(dt_launched(dt_launch_classify_f64(hc.c->stream, nullptr, d_b, d_f, N, 0.0, 0.0, 0, 1, nullptr,
                                            klass ? d_k : nullptr, (unsigned long long *)d_c)));
  DT_TRY(hc.download(flood, d_f, N));  // the benchmark map comes back remapped (evaluation.py:149-150 mutates it)
  if (klass) DT_TRY(hc.download(klass, d_k, N));
  return hc.finish();
}

// conditioned D8, host tier: dem in, D8 codes (flats resolved on the filled surface) and optionally the filled
// surface out; the float64 twin compares the heights in float64
template <typename T>
static int host_d8_conditioned(const T *dem, int64_t H, int64_t W, double px, uint8_t *fdr, T *filled, int32_t *info3,
                               int (*condition)(dt_ctx *, const T *, int64_t, int64_t, double, T *, uint8_t *,
                                                int32_t *)) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_hw(H, W));
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && fdr, "NULL raster");
  const T *d_dem = hc.in(dem, n);
  uint8_t *d_f = hc.out(fdr, n);
  T *d_w = filled ? hc.out(filled, n) : hc.scratch<T>(n);
  DT_TRY(hc.rc);
  DT_TRY(condition(hc.c, d_dem, H, W, px, d_w, d_f, info3));
  return hc.finish();
}
extern "C" int dt_d8_conditioned_f32(const float *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *filled,
                                     int32_t *info3) {
  return host_d8_conditioned(dem, H, W, px, fdr, filled, info3, dt_dev_condition_d8);
}
extern "C" int dt_d8_conditioned_f64(const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr, double *filled,
                                     int32_t *info3) {
  return host_d8_conditioned(dem, H, W, px, fdr, filled, info3, dt_dev_condition_d8_f64);
}

// flow-path extremes, host tier
extern "C" int dt_flowpath_upslope(const uint8_t *fdr, const float *dem, const float *values, int64_t H, int64_t W,
                                   int kind, float *value, int64_t *where) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_FP_KIND(kind);
  const size_t n = (size_t)H * W;
  if (n == 0 || (!value && !where)) return DT_OK;
  DT_REQUIRE(fdr && values, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const float *d_dem = hc.in(dem, n);
  const float *d_v = hc.in(values, n);
  float *d_o = hc.out(value, n);
  int64_t *d_w = hc.out(where, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_flowpath_upslope(hc.c, d_f, d_dem, d_v, H, W, kind, d_o, d_w));
  return hc.finish();
}

extern "C" int dt_flowpath_downstream(const uint8_t *fdr, const float *dem, const float *values, const uint8_t *stop,
                                      int64_t H, int64_t W, int kind, float *value, int64_t *where) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_FP_KIND(kind);
  const size_t n = (size_t)H * W;
  if (n == 0 || (!value && !where)) return DT_OK;
  DT_REQUIRE(fdr && values, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const float *d_dem = hc.in(dem, n);
  const float *d_v = hc.in(values, n);
  const uint8_t *d_s = hc.in(stop, n);
  float *d_o = hc.out(value, n);
  int64_t *d_w = hc.out(where, n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_flowpath_downstream(hc.c, d_f, d_dem, d_v, d_s, H, W, kind, d_o, d_w));
  return hc.finish();
}

// weighted flow-path sums, host tier (stop NULL and longest: dt_flowpath_upslope_longest)
static int host_pathsum(const uint8_t *fdr, const float *dem, const double *w, const uint8_t *stop, int64_t H,
                        int64_t W, int frac_bits, bool longest, double *out) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_fp(H, W));
  DT_REQUIRE(frac_bits >= -DT_FRAC_BITS_MAX && frac_bits <= DT_FRAC_BITS_MAX, "frac_bits out of range");
  const size_t n = (size_t)H * W;
  if (n == 0 || !out) return DT_OK;
  DT_REQUIRE(fdr && w, "NULL raster");
  const uint8_t *d_f = hc.in(fdr, n);
  const float *d_dem = hc.in(dem, n);
  const double *d_w = hc.in(w, n);
  const uint8_t *d_s = hc.in(stop, n);
  double *d_o = hc.out(out, n);
  DT_TRY(hc.rc);
  int32_t st = 0;
  DT_TRY(dt_ctx_status(hc.c, &st));  // this call's status only
  if (longest) DT_TRY(dt_dev_flowpath_upslope_longest(hc.c, d_f, d_dem, d_w, H, W, frac_bits, d_o));
  else DT_TRY(dt_dev_flowpath_downstream_sum(hc.c, d_f, d_dem, d_w, d_s, H, W, frac_bits, d_o));
  DT_TRY(dt_ctx_status(hc.c, &st));
  DT_REQUIRE(!(st & DT_STATUS_BAD_WEIGHT), "a weight is negative, not finite, or over the bound of frac_bits");
  return hc.finish();
}
extern "C" int dt_flowpath_downstream_sum(const uint8_t *fdr, const float *dem, const double *w, const uint8_t *stop,
                                          int64_t H, int64_t W, int frac_bits, double *out) {
  return host_pathsum(fdr, dem, w, stop, H, W, frac_bits, false, out);
}
extern "C" int dt_flowpath_upslope_longest(const uint8_t *fdr, const float *dem, const double *w, int64_t H, int64_t W,
                                           int frac_bits, double *out) {
  return host_pathsum(fdr, dem, w, nullptr, H, W, frac_bits, true, out);
}

// depression carving, host tier: conditioned D8, the upslope minimum of the DEM over its tree, and the blend with the
// filled surface when the cut is limited (max_cut +inf: no limit)
extern "C" int dt_carve(const float *dem, int64_t H, int64_t W, double px, double max_cut, uint8_t *fdr, float *carved,
                        float *filled, int32_t *info3) {
  HostCall hc;
  DT_TRY(hc.rc);
  DT_TRY(dt_check_ws(H, W, px));
  DT_REQUIRE(max_cut >= 0.0, "max_cut must be >= 0 (+inf: no limit)");
  const size_t n = (size_t)H * W;
  if (n == 0) return DT_OK;
  DT_REQUIRE(dem && fdr && carved, "NULL raster");
  const float *d_dem = hc.in(dem, n);
  uint8_t *d_f = hc.out(fdr, n);
  float *d_c = hc.out(carved, n);
  float *d_w = filled ? hc.out(filled, n) : hc.scratch<float>(n);
  DT_TRY(hc.rc);
  DT_TRY(dt_dev_condition_d8(hc.c, d_dem, H, W, px, d_w, d_f, info3));
  DT_TRY(dt_dev_flowpath_upslope(hc.c, d_f, d_dem, d_dem, H, W, 1, d_c, nullptr));
  DT_TRY(dt_launched(dt_launch_carve_blend(hc.c->stream, d_dem, std::isinf(max_cut) ? nullptr : d_w, d_c, (int64_t)n,
                                           (float)max_cut, d_c)));
  return hc.finish();
}
