// dt_wetness.hip -- the SAGA wetness index (Boehner & Selige 2006): the suction factor of a slope raster, the modified
// catchment area and the index on it (net-new; descriptools_amd/wetness.py holds the definition).
//
// The modified area M is the least solution of M(v) = max(A(v), fl(s(v) * max over the valid neighbours u of M(u))),
// s in [0, 1] in float32, the product in float64.  The product is monotone in M(u) and never exceeds it, so any
// relaxation that starts at M = A reaches that solution, in any order and any tiling: the (max, x) twin of the cost
// distance's (min, +) relaxation (dt_cost.hip), on the schedule of dt_tile_rounds.h.
// k_wet_suction  s = float32(exp(-((e * exp(exp(e * L))) * L))), e = weight * max(slope + offset, minimum), L = ln t
//                taken once on the host; -100 where the slope is NaN or not in [0, pi/2).
// k_wet_init     M = A on valid cells (0 < A < +inf and 0 <= s <= 1), -inf elsewhere.  M lives in the output raster.
// k_wet_round    one workgroup per tile of 64 x 64 cells with a one-cell halo: M of tile and halo goes to LDS (35 KB; -inf
//                beyond the raster and on nodata, which the initialisation left in M itself, so the halo needs no second
//                raster).  A lane owns 16 consecutive cells of one column and keeps their s in registers (negative: never
//                updates) -- a neighbour's s is never needed, so s does not go to LDS.  A sweep is two steps with a
//                barrier between them: every lane walks down its column with the maxima of three rows of three cells in
//                registers (54 LDS reads for 16 cells), then the lanes that found a larger value write it -- no lane
//                reads what another is writing, no atomics.  Sweeps repeat until one raises nothing or `visit_limit` is
//                reached; the raised cells go back to the raster.  Activity bytes, colours, flag words: dt_tile_rounds.h.
// k_wet_finish   -100 on nodata cells; counts the raised cells (M > A) and sums the tile visits.
// k_wet_index    swi = float32(log(M / tan(b))), b = max(slope + offset, minimum); -100 on nodata and where b >= pi/2.
#include <cfloat>
#include <cmath>

#include "dt_kernels.h"
#include "dt_tile_rounds.h"

#define WT_T 64
#define WT_LD (WT_T + 2)
#define WT_LS (WT_LD + 1)  // LDS row stride in cells
#define WT_CELLS (WT_LD * WT_LS)
#define WT_CPT (WT_T * WT_T / 256)            // cells per lane: rows WT_CPT * (lane / 64) ... of column lane % 64
#define WT_STAGE ((WT_LD * WT_LD + 255) / 256)  // staging loads per lane

#define WT_HALF_PI 1.5707963267948966

// control words of one call
enum {
  WT_C_FLAGS = 0,  // DT_TILE_ROUNDS_MAX of them: round r raises word r when it raised something
  WT_C_RAISED = DT_WETNESS_CTL_COUNTS,
  WT_C_VISITS = WT_C_RAISED + 2,  // 64 bits (8-byte aligned: WT_C_RAISED is even)
  WT_C_WORDS = WT_C_RAISED + 8
};

__device__ __forceinline__ bool wt_valid(double a, float s) {
  return a > 0.0 && a < (double)INFINITY && s >= 0.0f && s <= 1.0f;
}
__device__ __forceinline__ bool wt_slope_ok(float sl) { return (double)sl >= 0.0 && (double)sl < WT_HALF_PI; }
// max(slope + offset, minimum) for a slope that wt_slope_ok
__device__ __forceinline__ double wt_beta(float sl, double offset, double minimum) {
  const double b = (double)sl + offset;
  return b > minimum ? b : minimum;
}

__global__ __launch_bounds__(256) void k_wet_suction(const float *__restrict__ slope, long long N, double L,
                                                     double weight, double offset, double minimum,
                                                     float *__restrict__ suction) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const float sl = slope[c];
  float out = DT_NODATA;
  if (wt_slope_ok(sl)) {
    // float64, one rounding per operation (the library is built without contraction)
    const double e = weight * wt_beta(sl, offset, minimum);
    const double s = exp(-((e * exp(exp(e * L))) * L));
    out = s < (double)FLT_MIN ? 0.0f : (float)s;
  }
  suction[c] = out;
}

__global__ __launch_bounds__(256) void k_wet_init(const double *__restrict__ area, const float *__restrict__ suction,
                                                  long long N, double *__restrict__ m) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const double a = area[c];
  m[c] = wt_valid(a, suction[c]) ? a : -(double)INFINITY;
}

__global__ __launch_bounds__(256) void k_wet_round(const float *__restrict__ suction, double *__restrict__ m, int H,
                                                   int W, int visit_limit, const HyRound rnd) {
  __shared__ double s_m[WT_CELLS];
  int ty, tx;
  if (!hy_round_enter(rnd, ty, tx)) return;
  const int tile = ty * rnd.tiles_x + tx;
  const int y0 = ty * WT_T, x0 = tx * WT_T;
  // this lane's cells: column lx, rows ly0 ... ly0 + WT_CPT - 1
  const int lx = (int)threadIdx.x & (WT_T - 1), ly0 = ((int)threadIdx.x >> 6) * WT_CPT;
  // every load of the visit before the first use: M of tile and halo (-inf beyond the raster), s of the lane's cells
  double stage[WT_STAGE];
#pragma unroll
  for (int k = 0; k < WT_STAGE; k++) {
    const int i = (int)threadIdx.x + 256 * k;
    const int r = i / WT_LD, c = i - r * WT_LD;
    const int gy = y0 - 1 + r, gx = x0 - 1 + c;
    stage[k] = -(double)INFINITY;
    if (i < WT_LD * WT_LD && gy >= 0 && gy < H && gx >= 0 && gx < W) stage[k] = m[(long long)gy * W + gx];
  }
  float sc[WT_CPT];
#pragma unroll
  for (int j = 0; j < WT_CPT; j++) {
    const int gy = y0 + ly0 + j, gx = x0 + lx;
    sc[j] = (gy < H && gx < W) ? suction[(long long)gy * W + gx] : -1.0f;
  }
#pragma unroll
  for (int k = 0; k < WT_STAGE; k++) {
    const int i = (int)threadIdx.x + 256 * k;
    const int r = i / WT_LD, c = i - r * WT_LD;
    if (i < WT_LD * WT_LD) s_m[r * WT_LS + c] = stage[k];
  }
  __syncthreads();
  const int p0 = (ly0 + 1) * WT_LS + lx + 1;
  // a cell that is nodata holds -inf and never updates, whatever its s (NaN, beyond [0, 1])
#pragma unroll
  for (int j = 0; j < WT_CPT; j++)
    if (!(s_m[p0 + j * WT_LS] > -(double)INFINITY) || !(sc[j] >= 0.0f)) sc[j] = -1.0f;
  const int sweeps_max = visit_limit > 0 ? visit_limit : 0x7fffffff;
  uint32_t dirty = 0u;  // bit j: cell j was raised during this visit
  int open = 0;
  for (int sweep = 0; sweep < sweeps_max; sweep++) {
    double na[WT_CPT];
    uint32_t up = 0u;
    // rows ly0 - 1 ... ly0 + WT_CPT of the columns lx - 1, lx, lx + 1: `all` the maximum of a row's three cells, `side`
    // that of its outer two, `mid` the cell of the lane's own column
    double all_prev, all_cur, side_cur, mid_cur;
    {
      const int q = p0 - WT_LS;
      all_prev = fmax(fmax(s_m[q - 1], s_m[q]), s_m[q + 1]);
      const double l = s_m[p0 - 1], r = s_m[p0 + 1];
      mid_cur = s_m[p0];
      side_cur = fmax(l, r);
      all_cur = fmax(side_cur, mid_cur);
    }
#pragma unroll
    for (int j = 0; j < WT_CPT; j++) {
      const int q = p0 + (j + 1) * WT_LS;
      const double l = s_m[q - 1], mid_next = s_m[q], r = s_m[q + 1];
      const double side_next = fmax(l, r), all_next = fmax(side_next, mid_next);
      // one multiplication on the maximum: the product is monotone, so this is the maximum of the products.  A cell
      // with s = 0 among nodata gives 0 * -inf = NaN, which never compares greater
      const double cand = (double)sc[j] * fmax(fmax(all_prev, side_cur), all_next);
      na[j] = cand;
      if (sc[j] >= 0.0f && cand > mid_cur) up |= 1u << j;
      all_prev = all_cur;
      all_cur = all_next;
      side_cur = side_next;
      mid_cur = mid_next;
    }
    __syncthreads();  // every lane has read what it needs of this sweep's LDS
#pragma unroll
    for (int j = 0; j < WT_CPT; j++)
      if (up & (1u << j)) s_m[p0 + j * WT_LS] = na[j];
    dirty |= up;
    open = __syncthreads_or(up != 0u);
    if (!open) break;
  }
  // the raised cells go back to the raster (all of them lie in the raster: beyond it sc is negative)
  int ring = 0;
#pragma unroll
  for (int j = 0; j < WT_CPT; j++) {
    if (!(dirty & (1u << j))) continue;
    const int ly = ly0 + j;
    m[(long long)(y0 + ly) * W + (x0 + lx)] = s_m[p0 + j * WT_LS];
    ring |= (ly == 0 || ly == WT_T - 1 || lx == 0 || lx == WT_T - 1) ? 1 : 0;
  }
  const int any = __syncthreads_or(dirty != 0u);
  ring = __syncthreads_or(ring);
  // open: the limit ended the visit while a sweep still raised something
  hy_round_leave(rnd, tile, (ring ? HY_CHANGED : 0) | (open ? HY_OPEN : 0), any);
}

// last_flag: the flag word of the last round enqueued before this kernel (NULL: the caller looked at the flags itself)
__global__ __launch_bounds__(256) void k_wet_finish(const double *__restrict__ area, double *__restrict__ m,
                                                    long long N, const uint32_t *__restrict__ visits, int tiles,
                                                    const int *__restrict__ last_flag, uint32_t *__restrict__ ctl,
                                                    int *__restrict__ status) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  bool raised = false;
  if (c < N) {
    const double v = m[c];
    if (v > -(double)INFINITY) raised = v > area[c];
    else m[c] = -100.0;
  }
  const int nr = __syncthreads_count(raised);
  hy_visits_sum(visits, tiles, &ctl[WT_C_VISITS]);
  if (threadIdx.x == 0) {
    if (nr) atomicAdd(&ctl[WT_C_RAISED], (uint32_t)nr);
    if (status && blockIdx.x == 0 && last_flag && *last_flag) atomicOr(status, DT_STATUS_NOT_CONVERGED);
  }
}

__global__ __launch_bounds__(256) void k_wet_index(const double *__restrict__ m, const float *__restrict__ slope,
                                                   long long N, double offset, double minimum,
                                                   float *__restrict__ swi) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const double v = m[c];
  const float sl = slope[c];
  float out = DT_NODATA;
  if (v > 0.0 && v < (double)INFINITY && wt_slope_ok(sl)) {
    const double b = wt_beta(sl, offset, minimum);
    if (b < WT_HALF_PI) out = (float)log(v / tan(b));
  }
  swi[c] = out;
}

// ---- launchers -----------------------------------------------------------------------------------------------------
struct WtLayout {
  HyRoundsScratch r;
  float *suction;  // the composite call's planes
  double *m;
  size_t bytes;
};
static WtLayout wt_layout(int64_t H, int64_t W, bool suction_plane, bool m_plane, void *scratch) {
  WtLayout L = {};
  DtCarver c(scratch);
  L.r = hy_rounds_take(c, H, W, WT_T, WT_C_WORDS);
  L.suction = suction_plane ? c.take<float>((size_t)(H * W)) : nullptr;
  L.m = m_plane ? c.take<double>((size_t)(H * W)) : nullptr;
  L.bytes = c.bytes();
  return L;
}
size_t dt_wetness_scratch(int64_t H, int64_t W, int suction_plane, int m_plane) {
  return wt_layout(H, W, suction_plane != 0, m_plane != 0, nullptr).bytes;
}
const uint32_t *dt_wetness_ctl(void *scratch, int64_t H, int64_t W) { return wt_layout(H, W, false, false, scratch).r.ctl; }
float *dt_wetness_suction_plane(void *scratch, int64_t H, int64_t W) {
  return wt_layout(H, W, true, false, scratch).suction;
}
double *dt_wetness_m_plane(void *scratch, int64_t H, int64_t W, int suction_plane) {
  return wt_layout(H, W, suction_plane != 0, true, scratch).m;
}

int dt_launch_wetness_suction(hipStream_t s, const float *slope, int64_t N, double log_t, double weight, double offset,
                              double minimum, float *suction) {
  if (N == 0) return DT_OK;
  hipLaunchKernelGGL(k_wet_suction, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, slope, (long long)N, log_t,
                     weight, offset, minimum, suction);
  return DT_OK;
}

int dt_launch_wetness_index(hipStream_t s, const double *modified, const float *slope, int64_t N, double offset,
                            double minimum, float *swi) {
  if (N == 0) return DT_OK;
  hipLaunchKernelGGL(k_wet_index, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, modified, slope, (long long)N,
                     offset, minimum, swi);
  return DT_OK;
}

int dt_launch_wetness_area(hipStream_t s, const double *area, const float *suction, int64_t H, int64_t W,
                           int visit_limit, int start, int rounds, int finish, void *scratch, size_t scratch_bytes,
                           double *modified, int *status) {
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  DT_REQUIRE(rounds >= 0 && rounds <= DT_TILE_ROUNDS_MAX, "bad number of rounds");
  const int64_t N = H * W;
  const WtLayout L = wt_layout(H, W, false, false, scratch);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const dim3 b(256);
  const dim3 cells((unsigned)((N + 255) / 256));
  uint32_t *ctl = L.r.ctl;
  if (start) hipLaunchKernelGGL(k_wet_init, cells, b, 0, s, area, suction, (long long)N, modified);
  DT_TRY(hy_launch_rounds(s, L.r, ctl + WT_C_FLAGS, start, rounds, [&](dim3 blocks, const HyRound &rnd) {
    hipLaunchKernelGGL(k_wet_round, blocks, b, 0, s, suction, modified, (int)H, (int)W, visit_limit, rnd);
  }));
  if (finish) {
    DT_HIP(hipMemsetAsync(ctl + WT_C_RAISED, 0, sizeof(uint32_t) * (WT_C_WORDS - WT_C_RAISED), s));
    // (finish with rounds: the device tier, which says so when its last round still raised something)
    const int *last = rounds ? (const int *)ctl + WT_C_FLAGS + rounds - 1 : nullptr;
    hipLaunchKernelGGL(k_wet_finish, cells, b, 0, s, area, modified, (long long)N, (const uint32_t *)L.r.visits,
                       (int)L.r.tiles(), last, ctl, status);
  }
  return DT_OK;
}
