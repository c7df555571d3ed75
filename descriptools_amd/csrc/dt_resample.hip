// dt_resample.hip -- raster resampling: a raster on one grid read onto another (resample.py holds the definition,
// tests/_resample_ref.py is its reference).  The matrix (a0, a1, a2, b0, b1, b2) maps destination pixel coordinates to
// source pixel coordinates, u = (a0 + a1 x) + a2 y, v = (b0 + b1 x) + b2 y, and travels by value in the kernel
// arguments.  All arithmetic is float64, one rounding per operation (the library is built with -ffp-contract=off), in
// the association the definition states.  One launch per call, no scratch, no global atomics.
//
// Point methods (nearest, bilinear, cubic): k_rs_point.  A wave owns 64 * K consecutive destination columns of one
// row, a lane K = 16 / sizeof(element) of them, written with one 16-byte store where the run is whole and aligned.
// (u, v) are compared against [0, Ws) x [0, Hs) as doubles BEFORE any conversion to an integer: a destination grid may
// lie 10^12 cells (or 10^300) beside the source, and a float -> int overflow there would become an address.
//
// Area methods (average, sum, min, max): k_rs_area.  A workgroup owns `tw` destination columns of one destination
// row.  The source rows of its footprint go through LDS in stages of `rs` rows, each stage loaded with 16-byte loads
// that are all issued before the first is waited for; then one thread per (destination column, staged row) takes the
// row's partial sums left to right, and one thread per destination column combines the rows top to bottom.  tw shrinks
// as a1 grows so that a stage fits (dt_launch_resample sizes it): at a1 = 256 a row of 31 float32 destination cells is
// 31 KiB already.
//
// mode (uint8): at a footprint of at most RS_MODE_SMALL cells one thread per destination cell copies its footprint to
// LDS and counts each value against the ones after it (k_rs_mode_small); beyond, one wave per destination cell fills a
// 256-bin LDS histogram (LDS adds, no global atomic) and takes its first maximum (k_rs_mode_wave).  256 x 256 cells do
// not fit a 16-bit counter: the bins are 32-bit.
#include <cmath>

#include "dt_common.h"
#include "dt_kernels.h"

namespace {

struct RsMatrix {
  double a0, a1, a2, b0, b1, b2;
};

enum { RS_NEAREST = 0, RS_BILINEAR = 1, RS_CUBIC = 2, RS_AVERAGE = 3, RS_SUM = 4, RS_MIN = 5, RS_MAX = 6, RS_MODE = 7 };

constexpr int RS_STAGE_BYTES = 32768;   // one stage of source rows in LDS: 256 threads x 8 loads of 16 bytes
constexpr int RS_STAGE_LOADS = 8;
constexpr int RS_PARTIALS = 1024;       // (destination column, staged row) pairs of a stage
constexpr int RS_MIN_TILES = 1024;      // an area call is cut into at least this many tiles where it has the cells
constexpr int RS_MODE_SMALL = 36;       // cells of the largest footprint that mode's thread-per-cell path takes

__device__ __forceinline__ bool rs_valid(double z) { return z > -100.0 && z < INFINITY; }  // NaN fails the first

// Keys' kernel, a = -0.5, in Horner form: the two inner taps at distance t in [0, 1], the two outer at t in [1, 2]
__device__ __forceinline__ double rs_keys_near(double t) { return ((1.5 * t - 2.5) * t) * t + 1.0; }
__device__ __forceinline__ double rs_keys_far(double t) { return ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0; }

// the value of a float raster at (u, v), a point known to lie inside it; false: no value
template <typename T, int METHOD>
__device__ __forceinline__ bool rs_interpolate(const T *__restrict__ src, int Hs, int Ws, double u, double v, double *out) {
  const int c = (int)floor(u), r = (int)floor(v);
  if (!rs_valid((double)src[(int64_t)r * Ws + c])) return false;
  const double up = u - 0.5, vp = v - 0.5;
  const double fc = floor(up), fr = floor(vp);
  const int c0 = (int)fc, r0 = (int)fr;  // in [-1, Ws - 1] and [-1, Hs - 1]
  const double fx = up - fc, fy = vp - fr;
  if (METHOD == RS_CUBIC && c0 >= 1 && r0 >= 1 && c0 + 2 < Ws && r0 + 2 < Hs) {
    const double wx[4] = {rs_keys_far(1.0 + fx), rs_keys_near(fx), rs_keys_near(1.0 - fx), rs_keys_far(2.0 - fx)};
    const double wy[4] = {rs_keys_far(1.0 + fy), rs_keys_near(fy), rs_keys_near(1.0 - fy), rs_keys_far(2.0 - fy)};
    double acc = 0.0;
    bool whole = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const T *row = src + (int64_t)(r0 - 1 + k) * Ws + (c0 - 1);
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const double z = (double)row[m];
        whole = whole && rs_valid(z);
        s = s + wx[m] * z;
      }
      acc = acc + wy[k] * s;
    }
    if (whole) {
      *out = acc;
      return true;
    }
  }
  const double wxs[2] = {1.0 - fx, fx}, wys[2] = {1.0 - fy, fy};
  double S = 0.0, D = 0.0;
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const double w = wys[k] * wxs[m];
      const int rr = r0 + k, cc = c0 + m;
      if (w != 0.0 && rr >= 0 && rr < Hs && cc >= 0 && cc < Ws) {
        const double z = (double)src[(int64_t)rr * Ws + cc];
        if (rs_valid(z)) {
          S = S + w * z;
          D = D + w;
        }
      }
    }
  *out = S / D;  // the containing cell counted with w >= 0.25
  return true;
}

// T: the element as bits (nearest) or as a float type; K cells per lane
template <typename T, int METHOD>
__global__ __launch_bounds__(256) void k_rs_point(const T *__restrict__ src, int Hs, int Ws, RsMatrix m, T fill,
                                                  T *__restrict__ dst, int Hd, int Wd, unsigned nbx) {
  constexpr int K = 16 / (int)sizeof(T);
  const unsigned bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const int64_t i = (int64_t)by * 4 + (threadIdx.x >> 6);
  const int64_t j0 = ((int64_t)bx * 64 + (threadIdx.x & 63u)) * K;
  if (i >= Hd || j0 >= Wd) return;
  const double y = (double)i + 0.5, ws = (double)Ws, hs = (double)Hs;
  T val[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const double x = (double)(j0 + k) + 0.5;
    const double u = (m.a0 + m.a1 * x) + m.a2 * y, v = (m.b0 + m.b1 * x) + m.b2 * y;
    T o = fill;
    if (j0 + k < Wd && u >= 0.0 && u < ws && v >= 0.0 && v < hs) {  // as doubles: NaN and any distance fail here
      if (METHOD == RS_NEAREST) {
        o = src[(int64_t)floor(v) * Ws + (int64_t)floor(u)];
      } else {
        double z;
        if (rs_interpolate<T, METHOD>(src, Hs, Ws, u, v, &z)) o = (T)z;
      }
    }
    val[k] = o;
  }
  T *p = dst + i * Wd + j0;
  if (j0 + K <= Wd && ((uintptr_t)p & 15u) == 0) {
    uint4 q;
    __builtin_memcpy(&q, val, 16);
    *reinterpret_cast<uint4 *>(p) = q;
  } else {
#pragma unroll
    for (int k = 0; k < K; k++)
      if (j0 + k < Wd) p[k] = val[k];
  }
}

// the source cells [lo, hi) that the interval [e0, e1) takes of n cells; false when it takes none.  Decided on the
// doubles: e0 and e1 may be anywhere
__device__ __forceinline__ bool rs_span(double e0, double e1, int n, int *lo, int *hi) {
  const double dn = (double)n;
  if (!(e0 < dn && e1 > 0.0 && e1 > e0)) return false;
  *lo = (int)floor(fmax(e0, 0.0));
  *hi = (int)ceil(fmin(e1, dn));
  return *hi > *lo;
}

// MODE: RS_AVERAGE, RS_SUM, RS_MIN or RS_MAX.  Dynamic LDS: rs * fwp elements of T, then 2 * rs * tw doubles.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_rs_area(const T *__restrict__ src, int Hs, int Ws, RsMatrix m,
                                                 T *__restrict__ dst, int Hd, int Wd, int tw, int rs, int fwp,
                                                 unsigned nbx, int vec) {
  constexpr int V = 16 / (int)sizeof(T);
  extern __shared__ uint4 s_raw[];
  T *s_row = reinterpret_cast<T *>(s_raw);
  double *s_ps = reinterpret_cast<double *>(s_raw + ((size_t)rs * fwp * sizeof(T) + 15) / 16);
  double *s_pd = s_ps + rs * tw;
  const int tid = (int)threadIdx.x;
  const int i = (int)(blockIdx.x / nbx);
  const int j0 = (int)(blockIdx.x % nbx) * tw;
  const int ntw = min(tw, Wd - j0);
  const int64_t N = (int64_t)Hs * Ws;

  // this thread's destination column and its source columns
  const int j = j0 + tid;
  const double u0 = m.a0 + m.a1 * (double)j, u1 = m.a0 + m.a1 * (double)(j + 1);
  int cb = 0, ce = 0;
  const bool mine = tid < ntw && rs_span(u0, u1, Ws, &cb, &ce);
  // the tile's: the edges grow with j (a1 > 0, and rounding is monotone), so the span of [the first column's left
  // edge, the last column's right edge) holds every column's span
  int tb = 0, te = 0;
  const bool any = rs_span(m.a0 + m.a1 * (double)j0, m.a0 + m.a1 * (double)(j0 + ntw), Ws, &tb, &te);
  const double v0 = m.b0 + m.b2 * (double)i, v1 = m.b0 + m.b2 * (double)(i + 1);
  int rb = 0, re = 0;
  if (!any || !rs_span(v0, v1, Hs, &rb, &re)) re = rb = 0;
  // Unreachable as dt_launch_resample sizes fwp (te - tb <= ceil(a1 * tw) + 2 <= fwp - V - 2); it stands so that a
  // stage stays inside its LDS whatever a later change of the sizing does.
  if (te - tb > fwp - V) te = tb + (fwp - V);

  double S = 0.0, D = 0.0;  // of destination column tid; min / max: the extreme and whether there is one
  for (int r0 = rb; r0 < re; r0 += rs) {
    const int nr = min(rs, re - r0);
    // ---- stage: rows r0 .. r0 + nr, columns tb .. te, each row from the 16-byte boundary at or before its first cell
    const int vpr = fwp / V;
    const int nvec = nr * vpr;
    uint4 q[RS_STAGE_LOADS];
#pragma unroll
    for (int k = 0; k < RS_STAGE_LOADS; k++) {
      const int idx = tid + k * 256;
      q[k] = make_uint4(0u, 0u, 0u, 0u);
      if (idx < nvec) {
        const int rr = idx / vpr, qv = idx - rr * vpr;
        const int64_t first = (int64_t)(r0 + rr) * Ws + tb;
        const int64_t e = (first & ~(int64_t)(V - 1)) + (int64_t)qv * V;
        if (e < first + (te - tb)) {
          if (vec && e + V <= N) {
            q[k] = *reinterpret_cast<const uint4 *>(src + e);
          } else {
            T t[V];
#pragma unroll
            for (int z = 0; z < V; z++) t[z] = e + z < N ? src[e + z] : (T)0;
            __builtin_memcpy(&q[k], t, 16);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RS_STAGE_LOADS; k++) {
      const int idx = tid + k * 256;
      if (idx < nvec) reinterpret_cast<uint4 *>(s_row)[idx] = q[k];
    }
    __syncthreads();
    // ---- one (destination column, staged row) per thread: the row's sums, left to right
    for (int p = tid; p < ntw * nr; p += 256) {
      const int rr = p / ntw, jj = p - rr * ntw;
      const double e0 = m.a0 + m.a1 * (double)(j0 + jj), e1 = m.a0 + m.a1 * (double)(j0 + jj + 1);
      int lo, hi;
      double s = 0.0, d = 0.0;
      if (rs_span(e0, e1, Ws, &lo, &hi)) {
        lo = max(lo, tb);
        hi = min(hi, te);
        const int64_t first = (int64_t)(r0 + rr) * Ws + tb;
        const T *row = s_row + (size_t)rr * fwp + (int)(first & (int64_t)(V - 1)) - tb;
        for (int c = lo; c < hi; c++) {
          const double wx = fmin(e1, (double)(c + 1)) - fmax(e0, (double)c);
          const double z = (double)row[c];
          if (wx > 0.0 && rs_valid(z)) {
            if (MODE == RS_MIN) {  // strict: of equal values (-0.0 and 0.0) the first stays
              s = d > 0.0 && !(z < s) ? s : z;
              d = 1.0;
            } else if (MODE == RS_MAX) {
              s = d > 0.0 && !(z > s) ? s : z;
              d = 1.0;
            } else {
              s = s + wx * z;
              d = d + wx;
            }
          }
        }
      }
      s_ps[p] = s;
      s_pd[p] = d;
    }
    __syncthreads();
    // ---- one destination column per thread: the rows, top to bottom
    if (mine) {
      for (int rr = 0; rr < nr; rr++) {
        const int r = r0 + rr;
        const double wy = fmin(v1, (double)(r + 1)) - fmax(v0, (double)r);
        const double s = s_ps[rr * ntw + tid], d = s_pd[rr * ntw + tid];
        if (!(wy > 0.0)) continue;
        if (MODE == RS_MIN) {
          if (d > 0.0) S = D > 0.0 && !(s < S) ? S : s, D = 1.0;
        } else if (MODE == RS_MAX) {
          if (d > 0.0) S = D > 0.0 && !(s > S) ? S : s, D = 1.0;
        } else {
          S = S + wy * s;
          D = D + wy * d;
        }
      }
    }
    __syncthreads();  // the next stage overwrites the rows and the partial sums
  }
  if (tid < ntw) {
    double o = -100.0;
    if (mine && D > 0.0) o = MODE == RS_AVERAGE ? S / D : S;
    dst[(int64_t)i * Wd + j] = (T)o;
  }
}

// the better of two (count, value) pairs: the larger count, the smaller value on a tie; packed count << 8 | 255 - value
__device__ __forceinline__ uint32_t rs_mode_key(uint32_t count, uint32_t value) { return count << 8 | (255u - value); }

__global__ __launch_bounds__(256) void k_rs_mode_small(const uint8_t *__restrict__ src, int Hs, int Ws, RsMatrix m,
                                                       int nodata, uint8_t fill, uint8_t *__restrict__ dst, int Hd,
                                                       int Wd) {
  // a thread's footprint, read once: 36 bytes apart, so the threads of a wave read different banks
  __shared__ uint8_t s_val[256 * RS_MODE_SMALL];
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (int64_t)Hd * Wd) return;
  const int i = (int)(cell / Wd), j = (int)(cell - (int64_t)i * Wd);
  int cb, ce, rb, re;
  uint32_t best = 0;
  if (rs_span(m.a0 + m.a1 * (double)j, m.a0 + m.a1 * (double)(j + 1), Ws, &cb, &ce) &&
      rs_span(m.b0 + m.b2 * (double)i, m.b0 + m.b2 * (double)(i + 1), Hs, &rb, &re)) {
    const int n = (re - rb) * (ce - cb);
    if (n <= RS_MODE_SMALL) {
      uint8_t *own = s_val + threadIdx.x * RS_MODE_SMALL;
      int k = 0;
      for (int r = rb; r < re; r++)
        for (int c = cb; c < ce; c++) own[k++] = src[(int64_t)r * Ws + c];
      // a value's first occurrence counts itself and every later one: its whole count
      for (int p = 0; p < n; p++) {
        const int v = own[p];
        if (v == nodata) continue;
        uint32_t cnt = 1;
        for (int q = p + 1; q < n; q++) cnt += own[q] == v ? 1u : 0u;
        best = max(best, rs_mode_key(cnt, (uint32_t)v));
      }
    } else {  // the rounding of the edges gave the footprint one cell more than ceil(a1) + 1: count in place
      for (int r = rb; r < re; r++)
        for (int c = cb; c < ce; c++) {
          const int v = src[(int64_t)r * Ws + c];
          if (v == nodata) continue;
          uint32_t cnt = 0;
          for (int r2 = rb; r2 < re; r2++)
            for (int c2 = cb; c2 < ce; c2++) cnt += src[(int64_t)r2 * Ws + c2] == v ? 1u : 0u;
          best = max(best, rs_mode_key(cnt, (uint32_t)v));
        }
    }
  }
  dst[cell] = best ? (uint8_t)(255u - (best & 255u)) : fill;
}

__global__ __launch_bounds__(256) void k_rs_mode_wave(const uint8_t *__restrict__ src, int Hs, int Ws, RsMatrix m,
                                                      int nodata, uint8_t fill, uint8_t *__restrict__ dst, int Hd,
                                                      int Wd) {
  __shared__ uint32_t s_hist[4][256];
  const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
  const int64_t cell = (int64_t)blockIdx.x * 4 + wv;
  const bool live = cell < (int64_t)Hd * Wd;
  const int i = live ? (int)(cell / Wd) : 0, j = live ? (int)(cell - (int64_t)i * Wd) : 0;
#pragma unroll
  for (int k = 0; k < 4; k++) s_hist[wv][lane * 4 + k] = 0u;
  __syncthreads();
  int cb, ce, rb, re;
  if (live && rs_span(m.a0 + m.a1 * (double)j, m.a0 + m.a1 * (double)(j + 1), Ws, &cb, &ce) &&
      rs_span(m.b0 + m.b2 * (double)i, m.b0 + m.b2 * (double)(i + 1), Hs, &rb, &re)) {
    // a lane per column, the wave down the rows: consecutive bytes per load
    for (int r = rb; r < re; r++)
      for (int c = cb + lane; c < ce; c += 64) {
        const int v = src[(int64_t)r * Ws + c];
        if (v != nodata) atomicAdd(&s_hist[wv][v], 1u);
      }
  }
  __syncthreads();
  uint32_t best = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t n = s_hist[wv][lane * 4 + k];
    if (n) best = max(best, rs_mode_key(n, (uint32_t)(lane * 4 + k)));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o));
  if (live && lane == 0) dst[cell] = best ? (uint8_t)(255u - (best & 255u)) : fill;
}

template <typename T>
int rs_launch_nearest(hipStream_t s, const void *src, int Hs, int Ws, const RsMatrix &m, uint64_t fill_bits,
                      void *dst, int Hd, int Wd) {
  constexpr int K = 16 / (int)sizeof(T);
  const unsigned nbx = (unsigned)(((int64_t)Wd + 64 * K - 1) / (64 * K)), nby = (unsigned)(((int64_t)Hd + 3) / 4);
  hipLaunchKernelGGL((k_rs_point<T, RS_NEAREST>), dim3(nbx * nby), dim3(256), 0, s, (const T *)src, Hs, Ws, m,
                     (T)fill_bits, (T *)dst, Hd, Wd, nbx);
  return DT_OK;
}

template <typename T>
int rs_launch_float(hipStream_t s, const void *src, int Hs, int Ws, const RsMatrix &m, int method, void *dst, int Hd,
                    int Wd) {
  constexpr int K = 16 / (int)sizeof(T), V = K;
  if (method == RS_BILINEAR || method == RS_CUBIC) {
    const unsigned nbx = (unsigned)(((int64_t)Wd + 64 * K - 1) / (64 * K)), nby = (unsigned)(((int64_t)Hd + 3) / 4);
    const dim3 g(nbx * nby), b(256);
    if (method == RS_BILINEAR)
      hipLaunchKernelGGL((k_rs_point<T, RS_BILINEAR>), g, b, 0, s, (const T *)src, Hs, Ws, m, (T)-100, (T *)dst, Hd, Wd, nbx);
    else
      hipLaunchKernelGGL((k_rs_point<T, RS_CUBIC>), g, b, 0, s, (const T *)src, Hs, Ws, m, (T)-100, (T *)dst, Hd, Wd, nbx);
    return DT_OK;
  }
  // the widest tile whose footprint row, with the slack of the 16-byte boundary and of the rounding, fits a stage
  const int cap = RS_STAGE_BYTES / (int)sizeof(T);
  int tw = (int)fmin(256.0, floor((double)(cap - 4 - 2 * V) / m.a1));
  // a small destination: narrower tiles, so that there are workgroups enough to hide each other's latency (a stage of
  // wide footprints keeps few threads busy: one per kilobyte of LDS at a1 = 256)
  const int64_t spread = ((int64_t)Hd * Wd + RS_MIN_TILES - 1) / RS_MIN_TILES;
  if (tw > spread) tw = (int)spread;
  if (tw > Wd) tw = Wd;
  if (tw < 1) tw = 1;
  int fwp = (int)ceil(m.a1 * (double)tw) + 4 + 2 * V;
  fwp = (fwp + V - 1) / V * V;
  if (fwp > cap) fwp = cap / V * V;
  int rs = (int)ceil(m.b2) + 1;
  if (rs > cap / fwp) rs = cap / fwp;
  if (rs > RS_PARTIALS / tw) rs = RS_PARTIALS / tw;
  if (rs < 1) rs = 1;
  const size_t lds = ((size_t)rs * fwp * sizeof(T) + 15) / 16 * 16 + (size_t)2 * rs * tw * sizeof(double);
  const unsigned nbx = (unsigned)((Wd + tw - 1) / tw);
  const dim3 g(nbx * (unsigned)Hd), b(256);
  const int vec = ((uintptr_t)src & 15u) == 0;
#define RS_AREA(MODE) \
  hipLaunchKernelGGL((k_rs_area<T, MODE>), g, b, lds, s, (const T *)src, Hs, Ws, m, (T *)dst, Hd, Wd, tw, rs, fwp, nbx, vec)
  switch (method) {
    case RS_AVERAGE: RS_AREA(RS_AVERAGE); break;
    case RS_SUM: RS_AREA(RS_SUM); break;
    case RS_MIN: RS_AREA(RS_MIN); break;
    default: RS_AREA(RS_MAX); break;
  }
#undef RS_AREA
  return DT_OK;
}

}  // namespace

// What both tiers require of a resampling call (the contract is in include/descriptools_hip.h).
int dt_check_resample(int dtype, int64_t Hs, int64_t Ws, const double *matrix, int method, int64_t nodata, int64_t Hd,
                      int64_t Wd) {
  DT_REQUIRE(Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1, "empty raster shape");
  DT_REQUIRE(Hs < (1ll << 31) && Ws < (1ll << 31) && Hs * Ws < (1ll << 31), "source raster of 2^31 cells or more");
  DT_REQUIRE(Hd < (1ll << 31) && Wd < (1ll << 31) && Hd * Wd < (1ll << 31), "destination raster of 2^31 cells or more");
  DT_REQUIRE(matrix != nullptr, "matrix is NULL");
  for (int k = 0; k < 6; k++) DT_REQUIRE(std::isfinite(matrix[k]), "the matrix must hold six finite numbers");
  const double det = matrix[1] * matrix[5] - matrix[2] * matrix[4];
  DT_REQUIRE(std::isfinite(det) && det != 0.0, "the matrix is singular");
  DT_REQUIRE(method >= RS_NEAREST && method <= RS_MODE, "unknown method");
  if (method == RS_NEAREST)
    DT_REQUIRE(dtype == 1 || dtype == 2 || dtype == 4 || dtype == 8, "nearest takes elements of 1, 2, 4 or 8 bytes");
  else if (method == RS_MODE)
    DT_REQUIRE(dtype == 1, "mode takes uint8 (dtype 1) only");
  else
    DT_REQUIRE(dtype == 32 || dtype == 64, "the interpolating and area methods take float32 (32) or float64 (64)");
  if (method >= RS_AVERAGE) {
    DT_REQUIRE(matrix[2] == 0.0 && matrix[4] == 0.0 && matrix[1] > 0.0 && matrix[5] > 0.0,
               "an area method takes an axis-aligned matrix: a2 == b1 == 0, a1 > 0, b2 > 0");
    DT_REQUIRE(matrix[1] <= 256.0 && matrix[5] <= 256.0,
               "an area method takes at most 256 source cells per destination cell and axis: chain two calls");
  }
  DT_REQUIRE(nodata >= -1 && nodata <= 255, "nodata must be -1 (none) or a uint8 value");
  return DT_OK;
}

int dt_launch_resample(hipStream_t s, const void *src, int dtype, int64_t Hs, int64_t Ws, const double *matrix,
                       int method, int64_t nodata, uint64_t fill_bits, void *dst, int64_t Hd, int64_t Wd) {
  // the arguments have passed dt_check_resample: each entry runs it once, before anything else
  const RsMatrix m{matrix[0], matrix[1], matrix[2], matrix[3], matrix[4], matrix[5]};
  const int hs = (int)Hs, ws = (int)Ws, hd = (int)Hd, wd = (int)Wd;
  if (method == RS_NEAREST) {
    switch (dtype) {
      case 1: return rs_launch_nearest<uint8_t>(s, src, hs, ws, m, fill_bits, dst, hd, wd);
      case 2: return rs_launch_nearest<uint16_t>(s, src, hs, ws, m, fill_bits, dst, hd, wd);
      case 4: return rs_launch_nearest<uint32_t>(s, src, hs, ws, m, fill_bits, dst, hd, wd);
      default: return rs_launch_nearest<uint64_t>(s, src, hs, ws, m, fill_bits, dst, hd, wd);
    }
  }
  if (method == RS_MODE) {
    const int64_t cells = Hd * Wd;
    const bool small = (ceil(m.a1) + 1.0) * (ceil(m.b2) + 1.0) <= (double)RS_MODE_SMALL;
    if (small)
      hipLaunchKernelGGL(k_rs_mode_small, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const uint8_t *)src,
                         hs, ws, m, (int)nodata, (uint8_t)fill_bits, (uint8_t *)dst, hd, wd);
    else
      hipLaunchKernelGGL(k_rs_mode_wave, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, s, (const uint8_t *)src, hs,
                         ws, m, (int)nodata, (uint8_t)fill_bits, (uint8_t *)dst, hd, wd);
    return DT_OK;
  }
  if (dtype == 32) return rs_launch_float<float>(s, src, hs, ws, m, method, dst, hd, wd);
  return rs_launch_float<double>(s, src, hs, ws, m, method, dst, hd, wd);
}
