// dt_curve.hip -- confusion counts at every threshold of a sorted table from one pass over the raster.
//
// A cell's classification changes once along a sorted threshold table, so the counts at all K thresholds are a prefix sum
// over a histogram of that change point, the cell's bin:
//   under:      j = #{k : t_k <  v}, the cell floods at every k >= j; a dead cell (nodata or NaN) gets j = K
//   otherwise:  j = #{k : t_k <= v}, the cell floods at every k <  j; a dead cell gets j = 0
// hist[j] counts the cells of benchmark class 0 (flood 0 or -100), hist[K + 1 + j] those of class 2 (flood 1),
// hist[2K + 2] the cells with any other benchmark value.  The cell semantics are k_confusion's (dt_kernels.hip).
//
// The bin is found with the comparisons the definition names, on the table itself: a branchless count over a coarse
// index in LDS (every S-th threshold, S a power of two) and then over the S - 1 thresholds between two index entries,
// read from the table in global memory (L2).  The two histograms of a workgroup are uint32 counters in LDS.
#include "dt_common.h"
#include "dt_kernels.h"

#define DT_CURVE_THREADS 1024      // one workgroup; with the histogram of a large K in LDS only one fits a CU
#define DT_CURVE_UNROLL 4          // cells per thread and trip
#define DT_CURVE_TILE (DT_CURVE_THREADS * DT_CURVE_UNROLL)
#define DT_CURVE_GRID_MAX 256      // workgroups; the kernel strides beyond
#define DT_CURVE_K_MAX 65535
#define DT_CURVE_LDS_BYTES 163840  // what one workgroup may declare on gfx950
#define DT_CURVE_COARSE_MAX 2048   // entries of the coarse index in LDS (16 KiB); S = 1 up to this K
// bins per class that the rest of the LDS holds: above DT_CURVE_BINS_MAX - 1 thresholds the raster is read once per
// range of DT_CURVE_BINS_MAX bins
#define DT_CURVE_BINS_MAX ((DT_CURVE_LDS_BYTES - DT_CURVE_COARSE_MAX * 8) / 8)
static_assert(DT_CURVE_BINS_MAX == 18432, "the tests mirror this capacity");
static_assert(((DT_CURVE_K_MAX + 31) >> 5) <= DT_CURVE_COARSE_MAX, "S = 32 covers the largest table");

struct CurveArgs {
  int K;        // thresholds
  int s_log2;   // log2 S
  int M;        // coarse entries: ceil(K / S)
  int top;      // the largest power of two <= M
  int bin0;     // this launch counts the bins bin0 .. bin0 + nb - 1
  int nb;
  int first;    // the launch that counts the dead cells and the unknown benchmark values
};

// #{k : p(t_k)} for p(t) = UNDER ? t < v : t <= v, which is true on a prefix of the sorted table
template <bool UNDER>
__device__ __forceinline__ int curve_bin(double v, const double *__restrict__ s_coarse,
                                         const double *__restrict__ th, const CurveArgs &a) {
  int cm = 0;
  for (int s = a.top; s > 0; s >>= 1) {
    const int m = cm + s;
    if (m <= a.M) {
      const double t = s_coarse[m - 1];
      if (UNDER ? (t < v) : (t <= v)) cm = m;
    }
  }
  if (a.s_log2 == 0 || cm == 0) return cm;
  // t[(cm - 1) S] passes and t[cm S] (if there is one) does not: count the thresholds in between
  const int base = ((cm - 1) << a.s_log2) + 1;
  const int end = min(cm << a.s_log2, a.K);
  const int len = end - base;
  int c = 0;
  for (int s = 1 << (a.s_log2 - 1); s > 0; s >>= 1) {
    const int m = c + s;
    if (m <= len) {
      const double t = th[base + m - 1];
      if (UNDER ? (t < v) : (t <= v)) c = m;
    }
  }
  return base + c;
}

// one trip's cells of a lane, DT_CURVE_THREADS apart (neighbouring lanes read neighbouring cells); `first` = the lane's
// first cell (>= 0).  A cell beyond the raster reads the last cell instead (n >= 1) and is dropped by its index later:
// loads under a branch would keep the compiler from counting how many are in flight
__device__ __forceinline__ void curve_load(const double *__restrict__ desc, const int8_t *__restrict__ flood, int64_t n,
                                           int64_t first, double *v, int *g) {
#pragma unroll
  for (int u = 0; u < DT_CURVE_UNROLL; u++) {
    const int64_t i = first + u * DT_CURVE_THREADS;
    const int64_t at = i < n ? i : n - 1;
    v[u] = desc[at];
    g[u] = (int)flood[at];
  }
}

template <bool UNDER>
__global__ __launch_bounds__(DT_CURVE_THREADS) void k_threshold_hist(const double *__restrict__ desc,
                                                                     const int8_t *__restrict__ flood, int64_t n,
                                                                     double nodata, const double *__restrict__ th,
                                                                     CurveArgs a, unsigned long long *__restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  double *s_coarse = reinterpret_cast<double *>(s_raw);
  uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_coarse + a.M);  // [0, nb): class 0, [nb, 2 nb): class 2
  const int tid = (int)threadIdx.x, lane = tid & 63;
  for (int i = tid; i < a.M; i += DT_CURVE_THREADS) s_coarse[i] = th[(int64_t)i << a.s_log2];
  for (int i = tid; i < 2 * a.nb; i += DT_CURVE_THREADS) s_hist[i] = 0u;
  __syncthreads();

  uint32_t dead0 = 0u, dead2 = 0u, other = 0u;  // per lane: at most n / (DT_CURVE_GRID_MAX * DT_CURVE_THREADS) + 4 cells
  const int64_t stride = (int64_t)gridDim.x * DT_CURVE_TILE;
  double v[DT_CURVE_UNROLL], v_next[DT_CURVE_UNROLL];
  int g[DT_CURVE_UNROLL], g_next[DT_CURVE_UNROLL];
  curve_load(desc, flood, n, (int64_t)blockIdx.x * DT_CURVE_TILE + tid, v, g);
  for (int64_t t0 = (int64_t)blockIdx.x * DT_CURVE_TILE; t0 < n; t0 += stride) {
    // the next trip's cells are on their way while this trip's are searched and counted
    curve_load(desc, flood, n, t0 + stride + tid, v_next, g_next);
#pragma unroll
    for (int u = 0; u < DT_CURVE_UNROLL; u++) {
      const bool cell = t0 + u * DT_CURVE_THREADS + tid < n;
      int gg = g[u];
      if (gg == 1) gg = 2;            // evaluation.py:149
      else if (gg == -100) gg = 0;    // evaluation.py:150
      const double x = v[u];
      const bool isn = (x == nodata) || (x != x);  // evaluation.py:111-121
      const bool known = cell && (gg == 0 || gg == 2);
      // every lane searches (the trip counts are uniform); a lane without a live cell drops the result
      const int j = curve_bin<UNDER>(x, s_coarse, th, a);
      int idx = -1;
      if (known && !isn) {
        const int jj = j - a.bin0;
        if ((unsigned)jj < (unsigned)a.nb) idx = (gg == 2 ? a.nb : 0) + jj;
      }
      dead0 += (known && isn && gg == 0) ? 1u : 0u;
      dead2 += (known && isn && gg == 2) ? 1u : 0u;
      other += (cell && !known) ? 1u : 0u;
      // neighbouring lanes hold neighbouring cells: a run of equal bins is added once, by its first lane
      const int prev = __shfl_up(idx, 1);
      const bool head = lane == 0 || idx != prev;
      const unsigned long long heads = __ballot(head);
      const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
      const int run = above ? __ffsll((long long)above) : 64 - lane;
      if (head && idx >= 0) atomicAdd(&s_hist[idx], (uint32_t)run);
    }
#pragma unroll
    for (int u = 0; u < DT_CURVE_UNROLL; u++) {
      v[u] = v_next[u];
      g[u] = g_next[u];
    }
  }
  __syncthreads();
  // one 64-bit atomic per non-empty bin and workgroup
  for (int i = tid; i < 2 * a.nb; i += DT_CURVE_THREADS) {
    const uint32_t c = s_hist[i];
    if (c) {
      const int64_t at = i < a.nb ? (int64_t)a.bin0 + i : (int64_t)a.K + 1 + a.bin0 + (i - a.nb);
      atomicAdd(&hist[at], (unsigned long long)c);
    }
  }
  if (a.first) {
    // the dead cells and the unknown benchmark values were counted in registers: one atomic per wave and counter
    unsigned long long d0 = dead0, d2 = dead2, ot = other;
    for (int off = 32; off > 0; off >>= 1) {
      d0 += __shfl_down(d0, off);
      d2 += __shfl_down(d2, off);
      ot += __shfl_down(ot, off);
    }
    if (lane == 0) {
      const int64_t dead_bin = UNDER ? a.K : 0;
      if (d0) atomicAdd(&hist[dead_bin], d0);
      if (d2) atomicAdd(&hist[(int64_t)a.K + 1 + dead_bin], d2);
      if (ot) atomicAdd(&hist[2 * ((int64_t)a.K + 1)], ot);
    }
  }
}

int dt_launch_threshold_hist(hipStream_t s, const double *desc, const int8_t *flood, int64_t n, double nodata,
                             const double *th_dev, int K, int under, unsigned long long *hist) {
  DT_REQUIRE(K >= 1 && K <= DT_CURVE_K_MAX, "1..65535 thresholds");
  // a workgroup counts in 32 bits and sees at most n / DT_CURVE_GRID_MAX + DT_CURVE_TILE cells: below 2^32 up to here
  DT_REQUIRE(n >= 0 && n <= (1ll << 39), "0..2^39 cells per call");
  DT_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * (2 * ((size_t)K + 1) + 1), s));
  if (n == 0) return DT_OK;
  CurveArgs a;
  a.K = K;
  a.s_log2 = 0;
  while (((K + (1 << a.s_log2) - 1) >> a.s_log2) > DT_CURVE_COARSE_MAX) a.s_log2++;
  a.M = (K + (1 << a.s_log2) - 1) >> a.s_log2;
  a.top = 1;
  while (a.top * 2 <= a.M) a.top *= 2;
  const int64_t tiles = (n + DT_CURVE_TILE - 1) / DT_CURVE_TILE;
  const unsigned grid = (unsigned)(tiles < DT_CURVE_GRID_MAX ? tiles : DT_CURVE_GRID_MAX);
  auto kernel = under ? k_threshold_hist<true> : k_threshold_hist<false>;
  const int bins = K + 1;
  // more bins than the LDS holds: one launch per range of bins, each reading the raster again
  for (a.bin0 = 0; a.bin0 < bins; a.bin0 += DT_CURVE_BINS_MAX) {
    a.nb = bins - a.bin0 < DT_CURVE_BINS_MAX ? bins - a.bin0 : DT_CURVE_BINS_MAX;
    a.first = a.bin0 == 0;
    const size_t lds = (size_t)a.M * sizeof(double) + 2 * (size_t)a.nb * sizeof(uint32_t);
    DT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(DT_CURVE_THREADS), lds, s, desc, flood, n, nodata, th_dev, a, hist);
  }
  return DT_OK;
}
