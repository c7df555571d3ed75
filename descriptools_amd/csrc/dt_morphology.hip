// dt_morphology.hip -- greyscale geodesic reconstruction (Vincent 1993): a marker raster spreads under a mask raster
// until it stops (net-new; descriptools_amd/morphology.py holds the definition).  The seeded fill, the h-minima and
// h-maxima transforms, the regional extrema and opening / closing by reconstruction are this one operator with
// different markers.
//
// Heights are compared by the order-preserving uint32 key of their float32 bits (dt_filters.hip's).  No valid or
// infinite float has key 0, nor does the complement of its key, so 0 stands for "none" and for "not a cell".
// Reconstruction by dilation is the least R >= F0 with R(v) = min(G(v), max(R(v), max over the neighbours u of R(u)))
// on keys, G the mask's key on valid cells and 0 elsewhere: an invalid cell is clamped to 0, so it holds none and is
// nobody's neighbour without any test.  Reconstruction by erosion is the same on complemented keys (`flip` = ~0).  The
// operator is monotone and only selects among the keys it is given, so any relaxation that starts at F0 reaches the one
// solution, in any order and any tiling: the (max, min) member beside the (min, +) of dt_cost.hip and the (max, x) of
// dt_wetness.hip, on the schedule of dt_tile_rounds.h.
// k_mo_init    the start keys F0 = min(marker key, G) from the marker mode (MoStart), 0 on invalid cells, into the
//              uint32 plane: the float output itself where there is one, a scratch plane for the uint8 output.
// k_mo_round   one workgroup per tile of 64 x 64 cells: R of tile and halo (0 beyond the raster) and G of the tile go
//              to LDS (17.3 + 16.3 KB), every global load issued before the first LDS store, whole tiles 16 bytes at a
//              time.  Then k_fill_relax's relaxation (dt_hydro.hip): four concurrent in-place directional sweeps, a
//              wave each, the line a sweep comes from in registers and its neighbours' lanes by DPP, odd row strides.
//              A step is integer max / min; the store is the LDS atomic max, so a concurrent sweep never loses a larger
//              value and no fresh re-read is needed.  Rounds of four sweeps repeat until one stores nothing or
//              `visit_limit` is reached (the tile then stays HY_OPEN); a visit that stored something writes the tile back.
// k_mo_finish  keys back to float32 (-100 for none), or the uint8 plane R != G; counts the valid cells with R != F0
//              and sums the tile visits.
#include <cmath>

#include "dt_kernels.h"
#include "dt_tile_rounds.h"

#define MO_T 64
#define MO_LD (MO_T + 2)
// LDS row strides: odd, so the column sweeps (a lane per row) fall on all banks (dt_hydro.hip measured it)
#define MO_LS (MO_LD + 1) /* 67 */
#define MO_GS (MO_T + 1)  /* 65 */
#define MO_CPT (MO_T * MO_T / 256)
#define MO_RING (2 * MO_LD + 2 * MO_T)

// control words of one call
enum {
  MO_C_FLAGS = 0,  // DT_TILE_ROUNDS_MAX of them: round r raises word r when it stored something
  MO_C_CHANGED = DT_MORPH_CTL_COUNTS,
  MO_C_VISITS = MO_C_CHANGED + 2,  // 64 bits (8-byte aligned: MO_C_CHANGED is even)
  MO_C_WORDS = MO_C_CHANGED + 8
};

typedef uint32_t mo_v4u_a4 __attribute__((ext_vector_type(4), aligned(4)));  // (rows are 4-byte aligned at any width)

__device__ __forceinline__ bool mo_valid(float z) { return z > -100.0f && z < INFINITY; }
__device__ __forceinline__ uint32_t mo_key(float z) {
  const uint32_t u = __float_as_uint(z);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float mo_unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
// the clamp key G of a mask height: 0 on an invalid cell
__device__ __forceinline__ uint32_t mo_clamp(float z, uint32_t flip) { return mo_valid(z) ? mo_key(z) ^ flip : 0u; }
__device__ __forceinline__ uint32_t mo_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t mo_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t mo_max3(uint32_t a, uint32_t b, uint32_t c) { return mo_max(mo_max(a, b), c); }

// what the start keys are made from
struct MoStart {
  int mode;       // DT_MORPH_*
  uint32_t flip;  // ~0 for erosion
  const float *mask, *marker;
  const uint8_t *seeds;
  double h;
  int H, W;
};
// F0 of cell c, whose clamp key is g != 0
__device__ __forceinline__ uint32_t mo_start(const MoStart &a, long long c, uint32_t g) {
  switch (a.mode) {
    case DT_MORPH_SHIFT: {
      const double z = (double)a.mask[c];
      // (erosion: z + h, given whatever it is; dilation: z - h, kept a valid height: the float32 next above -100)
      const float m = a.flip ? (float)(z + a.h) : fmaxf((float)(z - a.h), __uint_as_float(0xC2C7FFFFu));
      return mo_min(mo_key(m) ^ a.flip, g);
    }
    case DT_MORPH_STEP:
      return g - 1u;  // key + 1 for erosion (its complement is one less), key - 1 for dilation
    case DT_MORPH_OUTLETS: {
      if (a.seeds) return a.seeds[c] ? g : 0u;
      const int y = (int)(c / a.W), x = (int)(c - (long long)y * a.W);
      bool outlet = y == 0 || x == 0 || y == a.H - 1 || x == a.W - 1;
      if (!outlet) {
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
          for (int dx = -1; dx <= 1; dx++)
            if ((dy || dx) && !mo_valid(a.mask[c + (long long)dy * a.W + dx])) outlet = true;
      }
      return outlet ? g : 0u;
    }
    default: {  // DT_MORPH_MARKER, DT_MORPH_WINDOW: a raster; given iff not NaN and > -100 (+inf is)
      const float m = a.marker[c];
      return m > -100.0f ? mo_min(mo_key(m) ^ a.flip, g) : 0u;
    }
  }
}

__global__ __launch_bounds__(256) void k_mo_init(const MoStart a, long long N, uint32_t *__restrict__ rk) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const uint32_t g = mo_clamp(a.mask[c], a.flip);
  rk[c] = g ? mo_start(a, c, g) : 0u;
}

// v of the lane before / after mine; `edge` for lane 0 / 63 (wave_shr:1 / wave_shl:1 keep the old value there)
__device__ __forceinline__ uint32_t mo_from_prev_lane(uint32_t edge, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t mo_from_next_lane(uint32_t edge, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x130, 0xF, 0xF, false);
}
__device__ __forceinline__ void mo_ring_cell(int j, int &r, int &c) {  // 66 above, 66 below, 64 left, 64 right
  if (j < MO_LD) { r = 0; c = j; }
  else if (j < 2 * MO_LD) { r = MO_LD - 1; c = j - MO_LD; }
  else if (j < 2 * MO_LD + MO_T) { r = j - 2 * MO_LD + 1; c = 0; }
  else { r = j - 2 * MO_LD - MO_T + 1; c = MO_LD - 1; }
}

// One directional in-place sweep over the tile in LDS, hy_fill_sweep's walk on keys: BY_ROWS: a lane per column, the
// sweep walks rows; DIR: +1 from the first line to the last, -1 back.  The cell the lane stands on and the line ahead
// were fetched a step earlier and may be stale -- only ever too small, which costs a store that changes nothing.
// Returns bit 0: the sweep stored something; bit 1: on the tile's outer ring.
template <bool BY_ROWS, int DIR, int CONN>
__device__ __forceinline__ int mo_sweep(uint32_t *__restrict__ s_r, const uint32_t *__restrict__ s_g, int lane) {
  constexpr int SA = BY_ROWS ? DIR * MO_LS : DIR;  // one step along the sweep
  constexpr int SC = BY_ROWS ? 1 : MO_LS;          // one lane across it
  constexpr int GA = BY_ROWS ? DIR * MO_GS : DIR;
  constexpr int K0 = DIR < 0 ? MO_T - 1 : 0;
  int p = BY_ROWS ? (K0 + 1) * MO_LS + lane + 1 : (lane + 1) * MO_LS + K0 + 1;
  int gi = BY_ROWS ? K0 * MO_GS + lane : lane * MO_GS + K0;
  uint32_t up = s_r[p - SA];                              // the line before the tile (halo: nobody writes it)
  uint32_t hl = s_r[p - SA - SC], hr = s_r[p - SA + SC];  // its cells beside lanes 0 / 63
  uint32_t cur = s_r[p], lf = s_r[p - SC], rt = s_r[p + SC];
  const bool on_side = lane == 0 || lane == MO_T - 1;
  int ch = 0;
#pragma unroll 4
  for (int step = 0; step < MO_T; step++) {
    const uint32_t d0 = s_r[p + SA - SC], d1 = s_r[p + SA], d2 = s_r[p + SA + SC];
    const uint32_t g = s_g[gi];
    uint32_t m;
    if (CONN == 8) {
      const uint32_t upm = mo_from_prev_lane(hl, up), upp = mo_from_next_lane(hr, up);
      m = mo_max3(mo_max3(upm, up, upp), mo_max(lf, rt), mo_max3(d0, d1, d2));
    } else {
      m = mo_max(mo_max(up, d1), mo_max(lf, rt));
    }
    const uint32_t nw = mo_min(g, m);  // (g = 0 on an invalid cell: it never stores)
    if (nw > cur) {
      atomicMax(&s_r[p], nw);
      ch |= (on_side || step == 0 || step == MO_T - 1) ? 3 : 1;
    }
    up = mo_max(cur, nw);  // what this lane leaves behind
    hl = lf;               // the next step's line before is this line: beside lanes 0 / 63 lie its halo cells
    hr = rt;
    cur = d1;
    lf = d0;
    rt = d2;
    p += SA;
    gi += GA;
  }
  return ch;
}

template <int CONN>
__global__ __launch_bounds__(256) void k_mo_round(const float *__restrict__ mask, uint32_t *__restrict__ rk, int H,
                                                  int W, uint32_t flip, int visit_limit, const HyRound rnd) {
  __shared__ uint32_t s_r[MO_LD * MO_LS];
  __shared__ uint32_t s_g[MO_T * MO_GS];  // the clamp keys of the tile's own cells (0 beyond the raster)
  int ty, tx;
  if (!hy_round_enter(rnd, ty, tx)) return;
  const int tile = ty * rnd.tiles_x + tx;
  const int y0 = ty * MO_T, x0 = tx * MO_T;
  // block-uniform: a whole tile -- keys and heights in, keys out go 16 bytes at a time
  const bool whole = y0 + MO_T <= H && x0 + MO_T <= W;
  // every load of the visit before the first LDS store: the ring of R (0 beyond the raster) ...
  uint32_t ring_v[2] = {0u, 0u};
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int j = (int)threadIdx.x + 256 * k;
    if (j < MO_RING) {
      int r, c;
      mo_ring_cell(j, r, c);
      const int gy = y0 - 1 + r, gx = x0 - 1 + c;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) ring_v[k] = rk[(long long)gy * W + gx];
    }
  }
  // ... then R and the heights of the core
  if (whole) {
    mo_v4u_a4 r4[4], z4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = (int)threadIdx.x + 256 * k;  // 16 groups of four cells per row
      const long long o = (long long)(y0 + (i >> 4)) * W + x0 + (i & 15) * 4;
      r4[k] = *reinterpret_cast<const mo_v4u_a4 *>(rk + o);
      z4[k] = *reinterpret_cast<const mo_v4u_a4 *>(mask + o);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = (int)threadIdx.x + 256 * k;
      uint32_t *dr = s_r + ((i >> 4) + 1) * MO_LS + 1 + (i & 15) * 4, *dg = s_g + (i >> 4) * MO_GS + (i & 15) * 4;
      dr[0] = r4[k].x;
      dr[1] = r4[k].y;
      dr[2] = r4[k].z;
      dr[3] = r4[k].w;
      dg[0] = mo_clamp(__uint_as_float(z4[k].x), flip);
      dg[1] = mo_clamp(__uint_as_float(z4[k].y), flip);
      dg[2] = mo_clamp(__uint_as_float(z4[k].z), flip);
      dg[3] = mo_clamp(__uint_as_float(z4[k].w), flip);
    }
  } else {
    uint32_t r1[MO_CPT], g1[MO_CPT];
#pragma unroll
    for (int j = 0; j < MO_CPT; j++) {
      const int c = (int)threadIdx.x + 256 * j;
      const int y = y0 + c / MO_T, x = x0 + c % MO_T;
      r1[j] = g1[j] = 0u;
      if (y < H && x < W) {
        r1[j] = rk[(long long)y * W + x];
        g1[j] = mo_clamp(mask[(long long)y * W + x], flip);
      }
    }
#pragma unroll
    for (int j = 0; j < MO_CPT; j++) {
      const int c = (int)threadIdx.x + 256 * j;
      s_r[(c / MO_T + 1) * MO_LS + c % MO_T + 1] = r1[j];
      s_g[(c / MO_T) * MO_GS + c % MO_T] = g1[j];
    }
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int j = (int)threadIdx.x + 256 * k;
    if (j < MO_RING) {
      int r, c;
      mo_ring_cell(j, r, c);
      s_r[r * MO_LS + c] = ring_v[k];
    }
  }
  __syncthreads();
  // Rounds of four concurrent sweeps until one stores nothing: the image did not change during that round, every read
  // of it was fresh and no cell could rise -- the tile's fixed point under this halo.
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int limit = visit_limit > 0 ? visit_limit : 0x7fffffff;
  int any = 0, open = 0, ring = 0;
  for (int it = 0; it < limit; it++) {
    int ch;
    if (wave == 0) ch = mo_sweep<true, 1, CONN>(s_r, s_g, lane);         // top to bottom
    else if (wave == 1) ch = mo_sweep<true, -1, CONN>(s_r, s_g, lane);   // bottom to top
    else if (wave == 2) ch = mo_sweep<false, 1, CONN>(s_r, s_g, lane);   // left to right (a lane per row)
    else ch = mo_sweep<false, -1, CONN>(s_r, s_g, lane);                 // right to left
    open = __syncthreads_or(ch);
    if (!open) break;
    any = 1;
    ring |= __syncthreads_or(ch & 2);
  }
  if (any) {
    if (whole) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int i = (int)threadIdx.x + 256 * k;
        const uint32_t *sr = s_r + ((i >> 4) + 1) * MO_LS + 1 + (i & 15) * 4;
        mo_v4u_a4 v;
        v.x = sr[0];
        v.y = sr[1];
        v.z = sr[2];
        v.w = sr[3];
        *reinterpret_cast<mo_v4u_a4 *>(rk + (long long)(y0 + (i >> 4)) * W + x0 + (i & 15) * 4) = v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < MO_CPT; j++) {
        const int c = (int)threadIdx.x + 256 * j;
        const int y = y0 + c / MO_T, x = x0 + c % MO_T;
        if (y < H && x < W) rk[(long long)y * W + x] = s_r[(c / MO_T + 1) * MO_LS + c % MO_T + 1];
      }
    }
  }
  // open: the limit ended the visit while a round of sweeps still stored something
  hy_round_leave(rnd, tile, (ring ? HY_CHANGED : 0) | (open ? HY_OPEN : 0), any);
}

// rk and out may be the same memory (the float output holds the keys until now); out8: the uint8 form, R != G.
// last_flag: the flag word of the last round enqueued before this kernel (NULL: the caller looked at the flags itself)
__global__ __launch_bounds__(256) void k_mo_finish(const MoStart a, long long N, const uint32_t *rk, float *out,
                                                   uint8_t *__restrict__ out8, const uint32_t *__restrict__ visits,
                                                   int tiles, const int *__restrict__ last_flag,
                                                   uint32_t *__restrict__ ctl, int *__restrict__ status) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (c < N) {
    const uint32_t g = mo_clamp(a.mask[c], a.flip), r = rk[c];
    changed = g && r != mo_start(a, c, g);
    if (out8) out8[c] = (g && r != g) ? 1 : 0;
    else out[c] = r ? mo_unkey(r ^ a.flip) : DT_NODATA;
  }
  const int nc = __syncthreads_count(changed);
  hy_visits_sum(visits, tiles, &ctl[MO_C_VISITS]);
  if (threadIdx.x == 0) {
    if (nc) atomicAdd(&ctl[MO_C_CHANGED], (uint32_t)nc);
    if (status && blockIdx.x == 0 && last_flag && *last_flag) atomicOr(status, DT_STATUS_NOT_CONVERGED);
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
struct MoLayout {
  HyRoundsScratch r;
  uint32_t *plane;  // the keys of a call whose output is uint8
  float *window;    // DT_MORPH_WINDOW: the window minimum / maximum, and behind it the window pass's own scratch
  void *fx;
  size_t fx_bytes, bytes;
};
static MoLayout mo_layout(int64_t H, int64_t W, int mode, bool to_u8, void *scratch) {
  MoLayout L = {};
  DtCarver c(scratch);
  L.r = hy_rounds_take(c, H, W, MO_T, MO_C_WORDS);
  L.plane = to_u8 ? c.take<uint32_t>((size_t)(H * W)) : nullptr;
  if (mode == DT_MORPH_WINDOW) {
    L.window = c.take<float>((size_t)(H * W));
    L.fx_bytes = dt_filter_extremes_scratch(H, W);
    L.fx = c.raw(L.fx_bytes);
  }
  L.bytes = c.bytes();
  return L;
}
size_t dt_morph_scratch(int64_t H, int64_t W, int mode, int to_u8) {
  return mo_layout(H, W, mode, to_u8 != 0, nullptr).bytes;
}
const uint32_t *dt_morph_ctl(void *scratch, int64_t H, int64_t W) {
  return mo_layout(H, W, DT_MORPH_MARKER, false, scratch).r.ctl;
}

int dt_launch_morph(hipStream_t s, int mode, int erosion, int connectivity, const float *mask, const float *marker,
                    const uint8_t *seeds, double h, int radius, int64_t H, int64_t W, int visit_limit, int start,
                    int rounds, int finish, void *scratch, size_t scratch_bytes, float *out, uint8_t *out8,
                    int *status) {
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(mode >= DT_MORPH_MARKER && mode <= DT_MORPH_WINDOW, "bad marker mode");
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  DT_REQUIRE(rounds >= 0 && rounds <= DT_TILE_ROUNDS_MAX, "bad number of rounds");
  DT_REQUIRE((out != nullptr) != (out8 != nullptr), "one output raster, float32 or uint8");
  const int64_t N = H * W;
  const MoLayout L = mo_layout(H, W, mode, out8 != nullptr, scratch);
  DT_REQUIRE(scratch && scratch_bytes >= L.bytes, "scratch too small");
  const dim3 b(256);
  const dim3 cells((unsigned)((N + 255) / 256));
  uint32_t *ctl = L.r.ctl;
  uint32_t *rk = out8 ? L.plane : reinterpret_cast<uint32_t *>(out);
  const uint32_t flip = erosion ? 0xFFFFFFFFu : 0u;
  const MoStart a = {mode, flip, mask, mode == DT_MORPH_WINDOW ? L.window : marker, seeds, h, (int)H, (int)W};
  if (start) {
    // opening: the window minimum spreads under the heights; closing: the window maximum, by erosion
    if (mode == DT_MORPH_WINDOW)
      DT_TRY(dt_launch_filter_extremes(s, mask, H, W, radius, L.fx, L.fx_bytes, erosion ? nullptr : L.window,
                                       erosion ? L.window : nullptr, nullptr, nullptr, nullptr));
    hipLaunchKernelGGL(k_mo_init, cells, b, 0, s, a, (long long)N, rk);
  }
  DT_TRY(hy_launch_rounds(s, L.r, ctl + MO_C_FLAGS, start, rounds, [&](dim3 blocks, const HyRound &rnd) {
    if (connectivity == 8)
      hipLaunchKernelGGL(k_mo_round<8>, blocks, b, 0, s, mask, rk, (int)H, (int)W, flip, visit_limit, rnd);
    else
      hipLaunchKernelGGL(k_mo_round<4>, blocks, b, 0, s, mask, rk, (int)H, (int)W, flip, visit_limit, rnd);
  }));
  if (finish) {
    DT_HIP(hipMemsetAsync(ctl + MO_C_CHANGED, 0, sizeof(uint32_t) * (MO_C_WORDS - MO_C_CHANGED), s));
    // (finish with rounds: the device tier, which says so when its last round still stored something)
    const int *last = rounds ? (const int *)ctl + MO_C_FLAGS + rounds - 1 : nullptr;
    hipLaunchKernelGGL(k_mo_finish, cells, b, 0, s, a, (long long)N, (const uint32_t *)rk, out, out8,
                       (const uint32_t *)L.r.visits, (int)L.r.tiles(), last, ctl, status);
  }
  return DT_OK;
}
