// dt_filters.hip -- DEM filters: window minimum / maximum / range with morphological opening and closing at any radius,
// the window percentile (median) and feature-preserving denoising (Sun et al. 2007; net-new, descriptools_amd/filters.py
// holds the definition).  A height is valid iff it is finite and > -100.
//
// Extremes.  Everything is an unsigned minimum of the order-preserving key of the float (FT_NONE where there is no valid
// height; the maximum runs on the complemented key), so the result is a selection and exact.  The window minimum is
// separable, and each axis is the van Herk / Gil-Werman scheme over segments of L = 2 R + 1 cells: g = the running
// minimum from the segment's first cell, h = the running minimum from its last, and the window [a, b] is
// min(h[a], g[b]) -- three comparisons per cell and axis whatever the radius.  Three launches per plane:
// k_fx_rows   a wave takes 64 rows of a span of whole segments, 64 columns at a time: the tile goes through LDS so that
//             the heights are read and g / h written along the rows while lane r walks row r (stride 65: no conflict).
//             blockIdx.y = 0 walks east and writes g, 1 walks west and writes h.
// k_fx_cols   a thread takes a column of a span of whole segments: per row the row window min(h[a], g[b]) (a, b and
//             which of the two count depend on the column only), and the running minimum down (g2) or up (h2).
// k_fx_final  per cell min(h2[ya], g2[yb]), decoded; -100 where the cell's own height is not valid.
// Opening is the maximum of the minimum raster, closing the minimum of the maximum raster: the same three launches on
// the first result, whose -100 cells are the invalid cells of the input.
//
// k_fr_rank   the height at a rank: a 64 x 16 tile with a halo of R cells as keys in LDS, a lane takes four cells of a
//             column.  One sweep of the window for n, min and max; k = table[n] (the host's table, staged in LDS); then
//             the largest v with #{key < v} <= k, built bit by bit below the highest bit in which min and max differ
//             (one window sweep per bit): that v is the k-th smallest key.
// k_fr_rank_net  radius 1 and 2: the window's 9 / 25 keys in registers, a bitonic sorting network over 16 / 32, and a
//             chain of selects for the element of index k (DESIGN.md 4.27 holds what each form measured).
//
// Denoising, all float64 arithmetic on float32 planes, no contraction (+, -, *, /, sqrt only):
// k_fd_normals  3 x 3 Sobel normal of every valid cell from a 64 x 16 tile with a halo of one cell in LDS.
// k_fd_smooth   the thresholded, weighted sum of the unit normals over the window: a 32 x 32 tile with a halo of R cells
//               as three float32 planes in dynamic LDS, (32 + 2 R)^2 * 12 bytes: 21 KiB at R = 5 (7 workgroups of 4 waves
//               on a CU's 160 KiB), 48 KiB at R = 16 (3 workgroups).
// k_fd_update   one Jacobi step of the heights towards the facets of the eight neighbours: a 3 x 3 stencil over 16 bytes
//               per cell, straight from global memory.
#include <cmath>

#include "dt_common.h"
#include "dt_kernels.h"

#define FT_NONE 0xFFFFFFFFu  // the key of no height: above every valid key, and above every complemented one

__device__ __forceinline__ bool ft_valid(float z) { return z > -100.0f && z < INFINITY; }
// the order-preserving key of a float: a < b as floats <=> key(a) < key(b) as uint32 (-0.0 sorts below +0.0)
__device__ __forceinline__ uint32_t ft_key(float z) {
  const uint32_t u = __float_as_uint(z);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ft_unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ uint32_t ft_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// ---- extremes -----------------------------------------------------------------------------------------------------------
#define FX_T 64          // rows and columns of a k_fx_rows tile
#define FX_ROW_SPAN 1024 // columns a k_fx_rows wave walks, rounded down to whole segments (at least one)
#define FX_COL_SPAN 128  // rows a k_fx_cols thread walks, likewise

struct FxLayout {
  uint32_t *g, *h, *g2, *h2;  // the running minima of the row pass and of the column pass
  float *lo, *hi;             // the minimum and the maximum raster where the caller gave none
  size_t bytes;
};
static FxLayout fx_layout(int64_t H, int64_t W, void *scratch) {
  FxLayout L = {};
  DtCarver c(scratch);
  const size_t n = (size_t)(H * W);
  L.g = c.take<uint32_t>(n);
  L.h = c.take<uint32_t>(n);
  L.g2 = c.take<uint32_t>(n);
  L.h2 = c.take<uint32_t>(n);
  L.lo = c.take<float>(n);
  L.hi = c.take<float>(n);
  L.bytes = c.bytes();
  return L;
}
size_t dt_filter_extremes_scratch(int64_t H, int64_t W) { return fx_layout(H, W, nullptr).bytes; }

// the window [a, b] of cell x on an axis of n cells cut into segments of L: which of h[a] and g[b] make it up.  Both,
// unless a and b lie in one segment: then a is the segment's first cell (g[b] alone) or the window is clipped at n - 1
// (h[a] alone, it runs to the end of the axis)
__device__ __forceinline__ void fx_window(int x, int n, int R, int L, int &a, int &b, bool &use_h, bool &use_g) {
  a = x > R ? x - R : 0;
  b = n - 1 - x > R ? x + R : n - 1;
  const bool same = a / L == b / L, first = a % L == 0;
  use_h = !(same && first);
  use_g = !(same && !first);
}

template <bool MAXP>
__global__ __launch_bounds__(64) void k_fx_rows(const float *__restrict__ src, int H, int W, int L, int span,
                                                int spans_x, uint32_t *__restrict__ g, uint32_t *__restrict__ h) {
  __shared__ uint32_t s[FX_T][FX_T + 1];
  const int band = (int)(blockIdx.x / (unsigned)spans_x), sp = (int)(blockIdx.x - (unsigned)band * (unsigned)spans_x);
  const bool back = blockIdx.y == 1;
  const long long y0 = (long long)band * FX_T, xa = (long long)sp * span;
  const long long xb = xa + span < W ? xa + span : W;  // the span is [xa, xb)
  uint32_t *__restrict__ dst = back ? h : g;
  const int lane = (int)threadIdx.x;
  const int chunks = (int)((xb - xa + FX_T - 1) / FX_T);
  uint32_t run = FT_NONE;
  // the place in its segment of the next cell the walk meets (xa is a segment's first cell)
  int pos = back ? (int)(((long long)chunks * FX_T - 1) % L) : 0;
  for (int c = 0; c < chunks; c++) {
    const long long cx = xa + (long long)(back ? chunks - 1 - c : c) * FX_T;
    const long long x = cx + lane;
#pragma unroll
    for (int r0 = 0; r0 < FX_T; r0 += 16) {
      float z[16];
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const long long y = y0 + r0 + i;
        z[i] = y < H && x < xb ? src[y * W + x] : DT_NODATA;
      }
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint32_t k = ft_key(z[i]);
        s[r0 + i][lane] = ft_valid(z[i]) ? (MAXP ? ~k : k) : FT_NONE;
      }
    }
    __syncthreads();
    if (!back) {
      for (int j = 0; j < FX_T; j++) {
        if (pos == 0) run = FT_NONE;
        run = ft_min(run, s[lane][j]);
        s[lane][j] = run;
        pos = pos + 1 == L ? 0 : pos + 1;
      }
    } else {
      for (int j = FX_T - 1; j >= 0; j--) {
        if (pos == L - 1) run = FT_NONE;
        run = ft_min(run, s[lane][j]);
        s[lane][j] = run;
        pos = pos == 0 ? L - 1 : pos - 1;
      }
    }
    __syncthreads();
    if (x < xb) {
#pragma unroll 16
      for (int i = 0; i < FX_T; i++) {
        const long long y = y0 + i;
        if (y < H) dst[y * W + x] = s[i][lane];
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_fx_cols(const uint32_t *__restrict__ g, const uint32_t *__restrict__ h, int H,
                                                 int W, int R, int L, int span, int col_blocks,
                                                 uint32_t *__restrict__ g2, uint32_t *__restrict__ h2) {
  const int sp = (int)(blockIdx.x / (unsigned)col_blocks), cb = (int)(blockIdx.x - (unsigned)sp * (unsigned)col_blocks);
  const long long xl = (long long)cb * 256 + (int)threadIdx.x;
  if (xl >= W) return;
  const int x = (int)xl;
  int a, b;
  bool use_h, use_g;
  fx_window(x, W, R, L, a, b, use_h, use_g);
  const bool back = blockIdx.y == 1;
  const long long ya = (long long)sp * span, yb = ya + span < H ? ya + span : H;  // rows [ya, yb), ya a segment's first
  uint32_t *__restrict__ dst = back ? h2 : g2;
  uint32_t run = FT_NONE;
  if (!back) {
    int pos = 0;
    for (long long y0 = ya; y0 < yb; y0 += 8) {
      uint32_t v[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const long long y = y0 + i;
        const uint32_t vh = use_h && y < yb ? h[y * W + a] : FT_NONE, vg = use_g && y < yb ? g[y * W + b] : FT_NONE;
        v[i] = ft_min(vh, vg);
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const long long y = y0 + i;
        if (y >= yb) break;
        if (pos == 0) run = FT_NONE;
        run = ft_min(run, v[i]);
        dst[y * W + x] = run;
        pos = pos + 1 == L ? 0 : pos + 1;
      }
    }
  } else {
    int pos = (int)((yb - 1 - ya) % L);
    for (long long y0 = yb - 1; y0 >= ya; y0 -= 8) {
      uint32_t v[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const long long y = y0 - i;
        const uint32_t vh = use_h && y >= ya ? h[y * W + a] : FT_NONE, vg = use_g && y >= ya ? g[y * W + b] : FT_NONE;
        v[i] = ft_min(vh, vg);
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const long long y = y0 - i;
        if (y < ya) break;
        if (pos == L - 1) run = FT_NONE;
        run = ft_min(run, v[i]);
        dst[y * W + x] = run;
        pos = pos == 0 ? L - 1 : pos - 1;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_fx_final(const float *__restrict__ src, const uint32_t *__restrict__ g2,
                                                  const uint32_t *__restrict__ h2, int H, int W, int R, int L, int maxp,
                                                  float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= (long long)H * W) return;
  if (!ft_valid(src[i])) {
    out[i] = DT_NODATA;
    return;
  }
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  int a, b;
  bool use_h, use_g;
  fx_window(y, H, R, L, a, b, use_h, use_g);
  const uint32_t vh = use_h ? h2[(long long)a * W + x] : FT_NONE, vg = use_g ? g2[(long long)b * W + x] : FT_NONE;
  const uint32_t k = ft_min(vh, vg);
  out[i] = ft_unkey(maxp ? ~k : k);
}

__global__ __launch_bounds__(256) void k_fx_range(const float *__restrict__ lo, const float *__restrict__ hi,
                                                  long long n, float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const float a = lo[i];  // a valid height is > -100: -100 is the marker alone
  out[i] = a == DT_NODATA ? DT_NODATA : (float)((double)hi[i] - (double)a);
}

// the window minimum (maxp = 0) or maximum (1) of `src` into `out`
static void fx_plane(hipStream_t s, const float *src, int64_t H, int64_t W, int R, int maxp, const FxLayout &Y,
                     float *out) {
  const int L = 2 * R + 1;
  const int span_x = (FX_ROW_SPAN / L > 1 ? FX_ROW_SPAN / L : 1) * L, span_y = (FX_COL_SPAN / L > 1 ? FX_COL_SPAN / L : 1) * L;
  const int64_t spans_x = (W + span_x - 1) / span_x, bands = (H + FX_T - 1) / FX_T;
  const int64_t spans_y = (H + span_y - 1) / span_y, col_blocks = (W + 255) / 256;
  if (maxp)
    hipLaunchKernelGGL(k_fx_rows<true>, dim3((unsigned)(bands * spans_x), 2), dim3(64), 0, s, src, (int)H, (int)W, L,
                       span_x, (int)spans_x, Y.g, Y.h);
  else
    hipLaunchKernelGGL(k_fx_rows<false>, dim3((unsigned)(bands * spans_x), 2), dim3(64), 0, s, src, (int)H, (int)W, L,
                       span_x, (int)spans_x, Y.g, Y.h);
  hipLaunchKernelGGL(k_fx_cols, dim3((unsigned)(spans_y * col_blocks), 2), dim3(256), 0, s, Y.g, Y.h, (int)H, (int)W, R,
                     L, span_y, (int)col_blocks, Y.g2, Y.h2);
  hipLaunchKernelGGL(k_fx_final, dim3((unsigned)((H * W + 255) / 256)), dim3(256), 0, s, src, Y.g2, Y.h2, (int)H,
                     (int)W, R, L, maxp, out);
}

int dt_launch_filter_extremes(hipStream_t s, const float *dem, int64_t H, int64_t W, int radius, void *scratch,
                              size_t scratch_bytes, float *minimum, float *maximum, float *range, float *opening,
                              float *closing) {
  DT_REQUIRE(radius >= 1 && radius <= DT_FILTER_RADIUS_MAX, "radius must lie in [1, 4096]");
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(minimum || maximum || range || opening || closing, "no output raster");
  const FxLayout Y = fx_layout(H, W, scratch);
  DT_REQUIRE(scratch && scratch_bytes >= Y.bytes, "scratch too small");
  float *lo = minimum ? minimum : Y.lo, *hi = maximum ? maximum : Y.hi;
  if (minimum || range || opening) fx_plane(s, dem, H, W, radius, 0, Y, lo);
  if (maximum || range || closing) fx_plane(s, dem, H, W, radius, 1, Y, hi);
  if (range)
    hipLaunchKernelGGL(k_fx_range, dim3((unsigned)((H * W + 255) / 256)), dim3(256), 0, s, lo, hi, (long long)(H * W),
                       range);
  if (opening) fx_plane(s, lo, H, W, radius, 1, Y, opening);
  if (closing) fx_plane(s, hi, H, W, radius, 0, Y, closing);
  return DT_OK;
}

// ---- the height at a rank ------------------------------------------------------------------------------------------------
#define FR_TX 64   // a wave takes 64 consecutive cells of one row: stride-1 LDS reads
#define FR_TY 16
#define FR_RB 4    // cells of a column that a lane takes
#define FR_NT 256  // FR_TX * FR_TY / FR_RB
#define FR_RMAX DT_FILTER_RANK_RADIUS_MAX
#define FR_TABLE ((2 * FR_RMAX + 1) * (2 * FR_RMAX + 1) + 1)

struct FrTable {
  uint16_t k[FR_TABLE];  // k[n]: the index of the output among the n valid heights of a window, sorted ascending
};

// per cell b of the lane's four, the count of the window's keys below t[b]: every staged row is read once
__device__ __forceinline__ void fr_count(const uint32_t *hc, int wt, int r, const uint32_t (&t)[FR_RB], int (&cnt)[FR_RB]) {
#pragma unroll
  for (int b = 0; b < FR_RB; b++) cnt[b] = 0;
  for (int j = -r; j < FR_RB + r; j++) {
    uint32_t te[FR_RB];  // nothing is below 0: a row outside the window of cell b counts nothing
#pragma unroll
    for (int b = 0; b < FR_RB; b++) te[b] = j - b >= -r && j - b <= r ? t[b] : 0u;
    const uint32_t *row = hc + j * wt;
    for (int dx = -r; dx <= r; dx++) {
      const uint32_t v = row[dx];
#pragma unroll
      for (int b = 0; b < FR_RB; b++) cnt[b] += v < te[b];
    }
  }
}

// the FR_TX x FR_TY tile at (x0, y0) with a halo of r cells as keys, and the rank table; eight global reads of a thread
// are issued before their first LDS store
__device__ __forceinline__ void fr_stage(uint32_t *s, uint16_t *s_k, const float *__restrict__ dem, int H, int W, int x0,
                                         int y0, int r, const FrTable &T) {
  const int wt = FR_TX + 2 * r, ht = FR_TY + 2 * r;
  for (int i0 = (int)threadIdx.x; i0 < ht * wt; i0 += 8 * FR_NT) {
    float z[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = i0 + u * FR_NT;
      const int row = i / wt, col = i - row * wt;
      const int gy = y0 - r + row, gx = x0 - r + col;
      z[u] = i < ht * wt && gy >= 0 && gy < H && gx >= 0 && gx < W ? dem[(long long)gy * W + gx] : DT_NODATA;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = i0 + u * FR_NT;
      if (i < ht * wt) s[i] = ft_valid(z[u]) ? ft_key(z[u]) : FT_NONE;
    }
  }
  const int cells = (2 * r + 1) * (2 * r + 1);
  for (int i = (int)threadIdx.x; i <= cells; i += FR_NT) s_k[i] = T.k[i];
}

// bitonic sorting network over N registers (a power of two), ascending: every index is a compile-time constant
template <int N>
__device__ __forceinline__ void fr_sort(uint32_t (&v)[N]) {
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < N; i++) {
        const int l = i ^ j;
        if (l > i) {
          const uint32_t a = v[i], b = v[l];
          const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
          const bool up = (i & k) == 0;
          v[i] = up ? lo : hi;
          v[l] = up ? hi : lo;
        }
      }
    }
  }
}

// radius 1 and 2: the window's 9 / 25 keys in registers, padded with FT_NONE to 16 / 32, sorted by the network (the
// keys of no height sort last), and the element of index table[n] picked by a chain of selects
template <int R>
__global__ __launch_bounds__(FR_NT) void k_fr_rank_net(const float *__restrict__ dem, int H, int W, int tiles_x,
                                                       FrTable T, float *__restrict__ out) {
  constexpr int L = 2 * R + 1, CELLS = L * L, NP = CELLS <= 16 ? 16 : 32, WT = FR_TX + 2 * R;
  __shared__ uint32_t s[(FR_TY + 2 * R) * WT];
  __shared__ uint16_t s_k[CELLS + 1];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * FR_TX, y0 = tyi * FR_TY;
  fr_stage(s, s_k, dem, H, W, x0, y0, R, T);
  __syncthreads();
  const int lx = (int)threadIdx.x & (FR_TX - 1), ly0 = ((int)threadIdx.x / FR_TX) * FR_RB;
  const int gx = x0 + lx;
#pragma unroll 1
  for (int b = 0; b < FR_RB; b++) {
    const int gy = y0 + ly0 + b;
    if (gy >= H || gx >= W) continue;
    const uint32_t *c = &s[(ly0 + b + R) * WT + lx + R];
    uint32_t v[NP];
    int n = 0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
      v[i] = i < CELLS ? c[(i / L - R) * WT + (i % L - R)] : FT_NONE;
      n += v[i] != FT_NONE;
    }
    const uint32_t centre = v[R * L + R];
    fr_sort<NP>(v);
    const int k = s_k[n];
    uint32_t pick = v[0];
#pragma unroll
    for (int i = 1; i < CELLS; i++) pick = k == i ? v[i] : pick;
    out[(long long)gy * W + gx] = centre != FT_NONE ? ft_unkey(pick) : DT_NODATA;
  }
}

__global__ __launch_bounds__(FR_NT) void k_fr_rank(const float *__restrict__ dem, int H, int W, int tiles_x, int r,
                                                   FrTable T, float *__restrict__ out) {
  __shared__ uint32_t s[(FR_TY + 2 * FR_RMAX) * (FR_TX + 2 * FR_RMAX)];
  __shared__ uint16_t s_k[FR_TABLE];
  const int wt = FR_TX + 2 * r;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * FR_TX, y0 = tyi * FR_TY;
  fr_stage(s, s_k, dem, H, W, x0, y0, r, T);
  __syncthreads();
  const int lx = (int)threadIdx.x & (FR_TX - 1);
  const int ly0 = __builtin_amdgcn_readfirstlane((int)threadIdx.x / FR_TX) * FR_RB;  // a wave is one row of lanes
  const uint32_t *hc = &s[(ly0 + r) * wt + lx + r];

  // n, the smallest and the largest key of every window
  int n[FR_RB];
  uint32_t lo[FR_RB], hi[FR_RB];
#pragma unroll
  for (int b = 0; b < FR_RB; b++) {
    n[b] = 0;
    lo[b] = FT_NONE;
    hi[b] = 0;
  }
  for (int j = -r; j < FR_RB + r; j++) {
    bool in[FR_RB];
#pragma unroll
    for (int b = 0; b < FR_RB; b++) in[b] = j - b >= -r && j - b <= r;
    const uint32_t *row = hc + j * wt;
    for (int dx = -r; dx <= r; dx++) {
      const uint32_t v = row[dx];
      if (v == FT_NONE) continue;
#pragma unroll
      for (int b = 0; b < FR_RB; b++) {
        if (in[b]) {
          n[b]++;
          lo[b] = v < lo[b] ? v : lo[b];
          hi[b] = v > hi[b] ? v : hi[b];
        }
      }
    }
  }
  // the search starts from what min and max have in common above their highest differing bit; a bit above that of a
  // cell's own changes nothing for it (v | bit is v, or is above max and counts n > k), so the four cells share a loop
  int k[FR_RB], top = -1;
  uint32_t v[FR_RB];
#pragma unroll
  for (int b = 0; b < FR_RB; b++) {
    k[b] = s_k[n[b]];
    const uint32_t d = n[b] ? lo[b] ^ hi[b] : 0u;
    const int hb = d ? 31 - __clz((int)d) : -1;
    v[b] = hb >= 31 ? 0u : lo[b] & ~((2u << (hb < 0 ? 0 : hb)) - 1u);
    if (hb < 0) v[b] = lo[b];
    if (k[b] == 0) v[b] = lo[b];  // the minimum and the maximum need no search
    else if (k[b] == n[b] - 1) v[b] = hi[b];
    else top = hb > top ? hb : top;
  }
  for (int bit = top; bit >= 0; bit--) {
    uint32_t t[FR_RB];
    int cnt[FR_RB];
#pragma unroll
    for (int b = 0; b < FR_RB; b++) t[b] = v[b] | (1u << bit);
    fr_count(hc, wt, r, t, cnt);
#pragma unroll
    for (int b = 0; b < FR_RB; b++)
      if (cnt[b] <= k[b]) v[b] = t[b];
  }
  const int gx = x0 + lx;
#pragma unroll
  for (int b = 0; b < FR_RB; b++) {
    const int gy = y0 + ly0 + b;
    if (gy >= H || gx >= W) continue;
    out[(long long)gy * W + gx] = hc[b * wt] != FT_NONE ? ft_unkey(v[b]) : DT_NODATA;
  }
}

int dt_launch_filter_rank(hipStream_t s, const float *dem, int64_t H, int64_t W, int radius, const uint16_t *table,
                          int n_table, float *out) {
  DT_REQUIRE(radius >= 1 && radius <= DT_FILTER_RANK_RADIUS_MAX, "radius must lie in [1, 16]");
  const int cells = (2 * radius + 1) * (2 * radius + 1);
  DT_REQUIRE(table && n_table == cells + 1, "the rank table must hold (2 radius + 1)^2 + 1 entries");
  for (int n = 0; n <= cells; n++)
    DT_REQUIRE((int)table[n] < (n > 1 ? n : 1), "rank table: k[n] must be below n");
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(out, "no output raster");
  FrTable T = {};
  for (int n = 0; n <= cells; n++) T.k[n] = table[n];
  const int tiles_x = (int)((W + FR_TX - 1) / FR_TX);
  const unsigned nt = (unsigned)(((H + FR_TY - 1) / FR_TY) * tiles_x);
  if (radius == 1)
    hipLaunchKernelGGL(k_fr_rank_net<1>, dim3(nt), dim3(FR_NT), 0, s, dem, (int)H, (int)W, tiles_x, T, out);
  else if (radius == 2)
    hipLaunchKernelGGL(k_fr_rank_net<2>, dim3(nt), dim3(FR_NT), 0, s, dem, (int)H, (int)W, tiles_x, T, out);
  else
    hipLaunchKernelGGL(k_fr_rank, dim3(nt), dim3(FR_NT), 0, s, dem, (int)H, (int)W, tiles_x, radius, T, out);
  return DT_OK;
}

// ---- feature-preserving denoising ------------------------------------------------------------------------------------------
#define FD_NX 64  // the tile of k_fd_normals
#define FD_NY 16
#define FD_T 32   // the tile edge of k_fd_smooth
#define FD_RB 4   // cells a thread of either takes

struct FdLayout {
  float *n[3], *m[3];  // the unit normals and the smoothed unit normals; [0] is NaN where the height is not valid
  float *z;            // the second height buffer of the Jacobi steps (the output raster is the first)
  size_t bytes;
};
static FdLayout fd_layout(int64_t H, int64_t W, void *scratch) {
  FdLayout L = {};
  DtCarver c(scratch);
  const size_t n = (size_t)(H * W);
  for (int k = 0; k < 3; k++) L.n[k] = c.take<float>(n);
  for (int k = 0; k < 3; k++) L.m[k] = c.take<float>(n);
  L.z = c.take<float>(n);
  L.bytes = c.bytes();
  return L;
}
size_t dt_filter_denoise_scratch(int64_t H, int64_t W) { return fd_layout(H, W, nullptr).bytes; }

__global__ __launch_bounds__(256) void k_fd_normals(const float *__restrict__ dem, int H, int W, int tiles_x, double px,
                                                    float *__restrict__ nx, float *__restrict__ ny,
                                                    float *__restrict__ nz) {
  constexpr int WT = FD_NX + 2, HT = FD_NY + 2, ROUNDS = (WT * HT + 255) / 256;
  __shared__ float s[HT * WT];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * FD_NX, y0 = tyi * FD_NY;
  float zz[ROUNDS];
#pragma unroll
  for (int u = 0; u < ROUNDS; u++) {
    const int i = (int)threadIdx.x + 256 * u;
    const int row = i / WT, col = i - row * WT;
    const int gy = y0 - 1 + row, gx = x0 - 1 + col;
    zz[u] = i < HT * WT && gy >= 0 && gy < H && gx >= 0 && gx < W ? dem[(long long)gy * W + gx] : DT_NODATA;
  }
#pragma unroll
  for (int u = 0; u < ROUNDS; u++) {
    const int i = (int)threadIdx.x + 256 * u;
    if (i < HT * WT) s[i] = ft_valid(zz[u]) ? zz[u] : NAN;
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & (FD_NX - 1), ly0 = (int)threadIdx.x / FD_NX;
  const int gx = x0 + lx;
#pragma unroll
  for (int b = 0; b < FD_RB; b++) {
    const int ly = ly0 + b * (FD_NY / FD_RB), gy = y0 + ly;
    if (gy >= H || gx >= W) continue;
    const long long o = (long long)gy * W + gx;
    const float *c = &s[(ly + 1) * WT + lx + 1];
    const float zf = c[0];
    if (!(zf == zf)) {
      nx[o] = NAN;
      ny[o] = 0.0f;
      nz[o] = 0.0f;
      continue;
    }
    const double zc = (double)zf;
    double q[8];  // E, SE, S, SW, W, NW, N, NE
#pragma unroll
    for (int i = 0; i < 8; i++) {
      int dy, dx;
      dt_nb_delta(i, dy, dx);
      const float v = c[dy * WT + dx], opp = c[-dy * WT - dx];
      q[i] = v == v ? (double)v : opp == opp ? 2.0 * zc - (double)opp : zc;
    }
    const double gxs = ((q[7] + 2.0 * q[0]) + q[1]) - ((q[5] + 2.0 * q[4]) + q[3]);
    const double gys = ((q[3] + 2.0 * q[2]) + q[1]) - ((q[5] + 2.0 * q[6]) + q[7]);
    const double a = -gxs, bb = -gys, cc = 8.0 * px;
    const double len = sqrt((a * a + bb * bb) + cc * cc);
    nx[o] = (float)(a / len);
    ny[o] = (float)(bb / len);
    nz[o] = (float)(cc / len);
  }
}

__global__ __launch_bounds__(256) void k_fd_smooth(const float *__restrict__ nx, const float *__restrict__ ny,
                                                   const float *__restrict__ nz, int H, int W, int tiles_x, int r,
                                                   double t, float *__restrict__ mx, float *__restrict__ my,
                                                   float *__restrict__ mz) {
  extern __shared__ float fd_lds[];
  const int wt = FD_T + 2 * r, cells = wt * wt;
  float *sx = fd_lds, *sy = fd_lds + cells, *sz = fd_lds + 2 * cells;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * FD_T, y0 = tyi * FD_T;
  // every global read of a batch is issued before its first LDS store
  for (int i0 = (int)threadIdx.x; i0 < cells; i0 += 4 * 256) {
    float vx[4], vy[4], vz[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + u * 256;
      const int row = i / wt, col = i - row * wt;
      const int gy = y0 - r + row, gx = x0 - r + col;
      const bool in = i < cells && gy >= 0 && gy < H && gx >= 0 && gx < W;
      const long long o = (long long)gy * W + gx;
      vx[u] = in ? nx[o] : NAN;
      vy[u] = in ? ny[o] : 0.0f;
      vz[u] = in ? nz[o] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + u * 256;
      if (i < cells) {
        sx[i] = vx[u];
        sy[i] = vy[u];
        sz[i] = vz[u];
      }
    }
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & (FD_T - 1), ly0 = (int)threadIdx.x / FD_T;
  const int gx = x0 + lx;
  for (int b = 0; b < FD_RB; b++) {
    const int ly = ly0 + b * (FD_T / FD_RB), gy = y0 + ly;
    if (gy >= H || gx >= W) continue;
    const long long o = (long long)gy * W + gx;
    const int c0 = (ly + r) * wt + lx + r;
    const float cxf = sx[c0];
    if (!(cxf == cxf)) {
      mx[o] = NAN;
      my[o] = 0.0f;
      mz[o] = 0.0f;
      continue;
    }
    const double cx = (double)cxf, cy = (double)sy[c0], cz = (double)sz[c0];
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int dy = -r; dy <= r; dy++) {
      const int rb = c0 + dy * wt;
      for (int dx = -r; dx <= r; dx++) {
        const float fx = sx[rb + dx];
        if (!(fx == fx)) continue;
        const double ux = (double)fx, uy = (double)sy[rb + dx], uz = (double)sz[rb + dx];
        const double c = (cx * ux + cy * uy) + cz * uz;
        if (c > t) {
          const double w = (c - t) * (c - t);
          ax = ax + w * ux;
          ay = ay + w * uy;
          az = az + w * uz;
        }
      }
    }
    const double len = sqrt((ax * ax + ay * ay) + az * az);
    mx[o] = (float)(ax / len);
    my[o] = (float)(ay / len);
    mz[o] = (float)(az / len);
  }
}

__global__ __launch_bounds__(256) void k_fd_update(const float *__restrict__ z0, const float *__restrict__ zp,
                                                   const float *__restrict__ mx, const float *__restrict__ my,
                                                   const float *__restrict__ mz, int H, int W, double px, double t,
                                                   double max_change, float *__restrict__ zn) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= (long long)H * W) return;
  const float a0 = mx[i];
  if (!(a0 == a0)) {  // not a valid height: the input's bits
    reinterpret_cast<uint32_t *>(zn)[i] = reinterpret_cast<const uint32_t *>(z0)[i];
    return;
  }
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const double ac = (double)a0, bc = (double)my[i], cc = (double)mz[i];
  // the eight neighbours' reads first: E, SE, S, SW, W, NW, N, NE
  float za[8], ma[8], mb[8], mc[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    int dy, dx;
    dt_nb_delta(k, dy, dx);
    const int yy = y + dy, xx = x + dx;
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const long long o = (long long)yy * W + xx;
    ma[k] = in ? mx[o] : NAN;
    mb[k] = in ? my[o] : 0.0f;
    mc[k] = in ? mz[o] : 0.0f;
    za[k] = in ? zp[o] : 0.0f;
  }
  double sw = 0.0, sz = 0.0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (!(ma[k] == ma[k])) continue;
    int dy, dx;
    dt_nb_delta(k, dy, dx);
    const double ai = (double)ma[k], bi = (double)mb[k], ci = (double)mc[k];
    const double c = (ac * ai + bc * bi) + cc * ci;
    if (c > t) {
      const double w = (c - t) * (c - t);
      const double e = (double)za[k] + (ai * ((double)dx * px) + bi * ((double)dy * px)) / ci;
      sw = sw + w;
      sz = sz + w * e;
    }
  }
  const float prev = zp[i];
  float res = prev;
  if (sw > 0.0) {
    const float zh = (float)(sz / sw);
    if (fabs((double)zh - (double)z0[i]) <= max_change) res = zh;
  }
  zn[i] = res;
}

int dt_launch_filter_denoise(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, int radius,
                             double cos_threshold, int iterations, double max_change, void *scratch,
                             size_t scratch_bytes, float *out) {
  DT_REQUIRE(radius >= 1 && radius <= DT_FILTER_DENOISE_RADIUS_MAX, "radius must lie in [1, 16]");
  DT_REQUIRE(cos_threshold > 0.0 && cos_threshold < 1.0, "cos_threshold must lie in (0, 1)");
  DT_REQUIRE(iterations >= 1 && iterations <= DT_FILTER_DENOISE_ITERATIONS_MAX, "iterations must lie in [1, 32]");
  DT_REQUIRE(std::isfinite(max_change) && max_change > 0.0, "max_change must be finite and > 0");
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(out, "no output raster");
  const FdLayout Y = fd_layout(H, W, scratch);
  DT_REQUIRE(scratch && scratch_bytes >= Y.bytes, "scratch too small");
  {
    const int tiles_x = (int)((W + FD_NX - 1) / FD_NX);
    const unsigned nt = (unsigned)(((H + FD_NY - 1) / FD_NY) * tiles_x);
    hipLaunchKernelGGL(k_fd_normals, dim3(nt), dim3(256), 0, s, dem, (int)H, (int)W, tiles_x, px, Y.n[0], Y.n[1],
                       Y.n[2]);
  }
  {
    const int tiles_x = (int)((W + FD_T - 1) / FD_T), wt = FD_T + 2 * radius;
    const unsigned nt = (unsigned)(((H + FD_T - 1) / FD_T) * tiles_x);
    hipLaunchKernelGGL(k_fd_smooth, dim3(nt), dim3(256), (size_t)wt * wt * 3 * sizeof(float), s, Y.n[0], Y.n[1], Y.n[2],
                       (int)H, (int)W, tiles_x, radius, cos_threshold, Y.m[0], Y.m[1], Y.m[2]);
  }
  // Jacobi steps between `out` and the scratch buffer, so that the last one writes `out`
  const float *prev = dem;
  const unsigned blocks = (unsigned)((H * W + 255) / 256);
  for (int it = 1; it <= iterations; it++) {
    float *next = (iterations - it) % 2 == 0 ? out : Y.z;
    hipLaunchKernelGGL(k_fd_update, dim3(blocks), dim3(256), 0, s, dem, prev, Y.m[0], Y.m[1], Y.m[2], (int)H, (int)W,
                       px, cos_threshold, max_change, next);
    prev = next;
  }
  return DT_OK;
}
