// dt_common.h -- shared host/device helpers of libdescriptools_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/descriptools_hip.h"

#define DT_NODATA (-100.0f)

// ---- error plumbing ---------------------------------------------------------------------
void dt_set_error(const char *fmt, ...);

#define DT_HIP(call)                                                                   \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess) {                                                           \
      dt_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,   \
                   __LINE__);                                                          \
      return e__ == hipErrorOutOfMemory ? DT_ENOMEM : DT_EHIP;                         \
    }                                                                                  \
  } while (0)

#define DT_REQUIRE(cond, msg)                      \
  do {                                             \
    if (!(cond)) {                                 \
      dt_set_error("invalid argument: %s", msg);   \
      return DT_EINVAL;                            \
    }                                              \
  } while (0)

#define DT_TRY(expr)          \
  do {                        \
    int rc__ = (expr);        \
    if (rc__ != DT_OK) return rc__; \
  } while (0)

// ---- test / experiment knobs (dt_debug_set in the C ABI; all 0 by default) -------------------------
// Keys 1-7 (DT_DBG_TWI_PLAIN, DT_DBG_TWI_WX, DT_DBG_TWI_MAP, DT_DBG_DS_MARGIN, DT_DBG_NO_FUSED_FA_FH,
// DT_DBG_HY_FILL_SWEEPS, DT_DBG_HY_FLAT_SWEEPS) selected kernel variants and sweep counts whose A/B runs are settled
// (DESIGN.md 4.1, 4.4 and the conditioning section; profiles/ names them); the variants are gone, and dt_debug_set
// answers those numbers with an error.  The numbers stay unused: tests and tools address the keys by number, and a
// stale caller must fail instead of switching something else.
enum {
  DT_DBG_TWI_FLAG_ALL = 0,  /* the fused slope + TI + MTI stencil sends every cell through its exact path as well (tests) */
  DT_DBG_RETIRED_FIRST = 1, DT_DBG_RETIRED_LAST = 7,
  DT_DBG_HY_COLOUR_MIN = 8, /* tiles from which the conditioning rounds are coloured (0: the default; tests) */
  DT_DBG_FA_SCATTER = 9,    /* flow accumulation: the scatter form of the perimeter graph (A/B) */
  DT_DBG_RC_SLOTS = 10,     /* reach tables: n > 0 caps the LDS table at n slots (tests), -1 = no LDS table, one global
                               atomic per cell (A/B) */
  DT_DBG_DINF_STACK = 11,   /* D-infinity accumulation: n > 0: a lane holds at most n complete cells, the one it carries on
                               with included (1: no stack), so that the spill queue and its rounds run (tests); the
                               environment variable DT_DBG_DINF_STACK sets it too */
  DT_DBG_POISON = 12,       /* 0x100 | b: every workspace the library hands out is filled with byte b on the call's stream
                               before the op's first kernel (dt_poison in dt_capi.hip; tests).  Read at call time; not
                               to be set around a graph capture, which would record the memsets */
  DT_DBG_COUNT = 13
};
int dt_debug_get(int key);

// ---- context ------------------------------------------------------------------------------
// Which multi-call op's state lives in the context's `scratch`, and where.  The op's first phase claims it (*_local_w,
// the first rounds of dt_dev_dinf_accumulate), every dt_scratch_reset drops the claim, the later phases (*_finish_w, a
// continuation) require it -- dt_scratch_claim / dt_scratch_claimed in dt_capi.hip are the only code that touches it.
// DT_OWNER_HAND_WALK: HAND's state as the walk form of pass 1 leaves it (node words of the fed entries, no word cache: the
// last pass solves the tiles) -- the first phase that launched that form claims it, so the last pass cannot be told wrong.
enum DtScratchOwner { DT_OWNER_NONE = 0, DT_OWNER_FLOWACC, DT_OWNER_HAND, DT_OWNER_DINF, DT_OWNER_MFD, DT_OWNER_HAND_WALK };
struct DtScratchClaim {
  DtScratchOwner owner;
  int64_t h, w;       // the core shape of the raster the state belongs to
  char *ptr;          // where in `scratch` that state starts
  char *ptr2;         // flow accumulation only: HAND's region reserved beside it, for when phase 2 of the one and phase 1
                      // of the other are fused (the region then becomes HAND's `ptr`)
  const void *in[2];  // D-infinity, MFD: the angle (share) and weight rasters the accumulation was started on,
  int frac_bits;      // and its frac_bits: a continuation must name the same
  const void *param;  // a routing run on that state: its parameter raster and its mode (NULL and 0: an accumulation)
  int mode;
};
struct dt_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  char *scratch;
  size_t scratch_bytes;
  size_t scratch_used;  // bump pointer, reset at the start of every entry point
  DtScratchClaim claim;  // the two-phase state in `scratch`, if any
  char *scratch2;       // rank-level solves (must not disturb the two-phase tile scratch)
  size_t scratch2_bytes;
  hipEvent_t ev;        // fork / join with another context's stream (created on first use)
  int *status;          // device word of sticky DT_STATUS_* bits raised by kernels (dt_ctx_status reads and clears)
  char *aux;            // workspace of the fused slope + TI + MTI stencil (it runs between the two phases of
  size_t aux_bytes;     // the tile kernels in a multi-GPU step, so it must not touch `scratch`)
  uint64_t ws_gen;      // bumped whenever scratch / scratch2 / aux is reallocated or freed: a captured graph holds
                        // their raw addresses and must not be replayed across such a change (dt_graph_launch checks)
};

// grow-only scratch, bump-allocated per entry point (256-B aligned)
int dt_scratch_reset(dt_ctx *ctx, size_t total_bytes);
void *dt_scratch_take(dt_ctx *ctx, size_t bytes);
static inline size_t dt_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- workspaces ---------------------------------------------------------------------------------
// A workspace has one layout function: it carves its arrays out of `scratch` with a DtCarver, in order, and records
// bytes().  Given no memory (nullptr) the same function only sizes, so the size and the pointers cannot disagree.
struct DtCarver {
  char *base;  // may be null: sizing only, every pointer handed out is null
  size_t off = 0;
  explicit DtCarver(void *p) : base((char *)p) {}
  void *raw(size_t nbytes) {  // a counter header, a flag block, a pad: rounded up to 256 bytes like every array
    char *q = base ? base + off : nullptr;
    off += dt_align256(nbytes);
    return q;
  }
  template <typename T> T *take(size_t count) { return (T *)raw(count * sizeof(T)); }
  size_t bytes() const { return off; }
};
// ceil(log2 N) + 1: the rounds pointer doubling needs on chains of at most N cells
static inline int dt_doubling_rounds(int64_t N) {
  int r = 0;
  while (r < 62 && (1ll << r) < N) r++;
  return r + 1;
}
// blocks of 256 threads that cover n items at one item per thread, at most `cap` (the kernel strides beyond)
static inline unsigned dt_capped_grid(int64_t n, int64_t cap) {
  const int64_t want = (n + 255) / 256;
  return (unsigned)(want < cap ? want : cap);
}

// exclusive block scan of one 32-bit value per thread (256 threads, s_w: 4 words of LDS); *total = the block's sum
__device__ __forceinline__ uint32_t dt_block_scan_256(uint32_t v, uint32_t *s_w, uint32_t *total) {
  const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)x, o);
    if (lane >= o) x += t;
  }
  if (lane == 63) s_w[wv] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t t = s_w[k];
    before += k < wv ? t : 0u;
    all += t;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

// The fixed-point weight of the integer sums (weighted flow accumulation, the countdowns, the path sums): q = rint(v *
// 2^sbits), exact scaling and round half to even.  A weight that is negative, not finite or over qmax is `bad` and
// counts as 0.
__device__ __forceinline__ unsigned long long dt_quant_weight(double v, int sbits, unsigned long long qmax, bool &bad) {
  if (!(v >= 0.0)) {  // negative or NaN
    bad = true;
    return 0ull;
  }
  const double q = rint(ldexp(v, sbits));
  if (!(q <= (double)qmax)) {  // inf, or over the bound
    bad = true;
    return 0ull;
  }
  return (unsigned long long)q;
}

// four consecutive values of a float32 / float64 raster, 16-byte loads (f a multiple of 4, the raster 16-byte aligned)
template <typename HT>
__device__ __forceinline__ void dt_load4(const HT *__restrict__ src, int64_t f, HT (&hh)[4]) {
  if (sizeof(HT) == 4) {
    const float4 q = *reinterpret_cast<const float4 *>(src + f);
    hh[0] = (HT)q.x; hh[1] = (HT)q.y; hh[2] = (HT)q.z; hh[3] = (HT)q.w;
  } else {
    const double2 q0 = *reinterpret_cast<const double2 *>(src + f);
    const double2 q1 = *reinterpret_cast<const double2 *>(src + f + 2);
    hh[0] = (HT)q0.x; hh[1] = (HT)q0.y; hh[2] = (HT)q1.x; hh[3] = (HT)q1.y;
  }
}

// The slot of id r in a workgroup's LDS table of S slots (the reach and the zonal tables), -1 when every slot belongs
// to another id: linear probing from r mod S.  A key goes from empty (-1) to an id once and stays, so a slot found, or
// found wanting, is final.
__device__ __forceinline__ int dt_claim_slot(int *s_key, int S, int r) {
  int j = S > 0 ? (int)((uint32_t)r % (uint32_t)S) : 0;
  for (int i = 0; i < S; i++) {
    int k = s_key[j];
    if (k == -1) {
      k = atomicCAS(&s_key[j], -1, r);
      if (k == -1) return j;
    }
    if (k == r) return j;
    if (++j == S) j = 0;
  }
  return -1;
}

// ---- D8 decoding (flowhand.py:801-824 / downslope.py:490-513) -------------------------------
// code -> bit index: 1=E 2=SE 4=S 8=SW 16=W 32=NW 64=N 128=NE
__device__ __forceinline__ bool dt_d8_valid(uint32_t code) {
  return code != 0u && (code & (code - 1u)) == 0u;
}
// dx/dy for bit index i, packed 2 bits each as (d + 1)
//   i :  0  1  2  3  4  5  6  7
//   dx:  1  1  0 -1 -1 -1  0  1
//   dy:  0  1  1  1  0 -1 -1 -1
#define DT_PK8(a, b, c, d, e, f, g, h)                                                 \
  ((uint32_t)((a) + 1) | (uint32_t)((b) + 1) << 2 | (uint32_t)((c) + 1) << 4 |          \
   (uint32_t)((d) + 1) << 6 | (uint32_t)((e) + 1) << 8 | (uint32_t)((f) + 1) << 10 |    \
   (uint32_t)((g) + 1) << 12 | (uint32_t)((h) + 1) << 14)
#define DT_DX_PACK DT_PK8(1, 1, 0, -1, -1, -1, 0, 1)
#define DT_DY_PACK DT_PK8(0, 1, 1, 1, 0, -1, -1, -1)
// the step to neighbour i (the bit index of its code)
__device__ __forceinline__ void dt_nb_delta(int i, int &dy, int &dx) {
  dx = (int)((DT_DX_PACK >> (2 * i)) & 3u) - 1;
  dy = (int)((DT_DY_PACK >> (2 * i)) & 3u) - 1;
}
// the code with which neighbour i points back at the centre: the opposite step, E<->W, SE<->NW, S<->N, SW<->NE
__device__ __forceinline__ uint32_t dt_nb_back_code(int i) { return 1u << ((i + 4) & 7); }
__device__ __forceinline__ void dt_d8_delta(uint32_t code, int &dy, int &dx) {
  dt_nb_delta(__ffs((int)code) - 1, dy, dx);
}

// ---- raster window -------------------------------------------------------------------------------
// A core window of H x W cells inside rasters of row stride ld, placed at (gy0, gx0) of a global
// Hg x Wg raster.  Raster pointers are relative to the core origin: cell (y, x) is p[y * ld + x].
// `halo` cells beyond the core are present in memory on every side (0 for a single-GPU raster, where
// the core IS the global raster: ld = W, gy0 = gx0 = 0, Hg = H, Wg = W).
struct DtWin {
  int H, W;
  long long ld;
  int gy0, gx0, Hg, Wg;
  int halo;
};
// the window of a single raster
static inline DtWin dt_full_window(int64_t H, int64_t W) {
  DtWin w;
  w.H = (int)H; w.W = (int)W; w.ld = W; w.gy0 = 0; w.gx0 = 0; w.Hg = (int)H; w.Wg = (int)W; w.halo = 0;
  return w;
}
__host__ __device__ __forceinline__ bool dt_in_core(const DtWin &w, int y, int x) {
  return y >= 0 && y < w.H && x >= 0 && x < w.W;
}
// inside the global raster AND present in memory
__host__ __device__ __forceinline__ bool dt_readable(const DtWin &w, int y, int x) {
  int gy = w.gy0 + y, gx = w.gx0 + x;
  return gy >= 0 && gy < w.Hg && gx >= 0 && gx < w.Wg && y >= -w.halo && y < w.H + w.halo && x >= -w.halo &&
         x < w.W + w.halo;
}
// readable AND its D8 code is in memory: a rank computes the codes of its core and of its halo minus the outermost
// ring (a code needs the cell's eight neighbours), so a cell on the ring of the rank's memory has a height but no code
// -- unless that ring is the edge of the global raster, where the border rule gave it one
__host__ __device__ __forceinline__ bool dt_has_code(const DtWin &w, int y, int x) {
  if (!dt_readable(w, y, x)) return false;
  const int gy = w.gy0 + y, gx = w.gx0 + x;
  return (y > -w.halo || gy == 0) && (y < w.H + w.halo - 1 || gy == w.Hg - 1) && (x > -w.halo || gx == 0) &&
         (x < w.W + w.halo - 1 || gx == w.Wg - 1);
}
__host__ __device__ __forceinline__ bool dt_in_global(const DtWin &w, int y, int x) {
  int gy = w.gy0 + y, gx = w.gx0 + x;
  return gy >= 0 && gy < w.Hg && gx >= 0 && gx < w.Wg;
}
// ring of the core window ("rank perimeter"), P cells: top row, bottom row, left column, right column
__host__ __device__ __forceinline__ long long dt_perim_count(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  if (H == 1) return W;
  if (W == 1) return H;
  return 2ll * W + 2ll * (H - 2);
}
__host__ __device__ __forceinline__ long long dt_perim_index(int H, int W, int y, int x) {
  if (H == 1) return x;
  if (W == 1) return y;
  if (y == 0) return x;
  if (y == H - 1) return (long long)W + x;
  if (x == 0) return 2ll * W + (y - 1);
  if (x == W - 1) return 2ll * W + (H - 2) + (y - 1);
  return -1;
}
__host__ __device__ __forceinline__ void dt_perim_cell(int H, int W, long long i, int &y, int &x) {
  if (H == 1) { y = 0; x = (int)i; return; }
  if (W == 1) { y = (int)i; x = 0; return; }
  if (i < W) { y = 0; x = (int)i; }
  else if (i < 2ll * W) { y = H - 1; x = (int)(i - W); }
  else if (i < 2ll * W + (H - 2)) { y = (int)(i - 2ll * W) + 1; x = 0; }
  else { y = (int)(i - 2ll * W - (H - 2)) + 1; x = W - 1; }
}
