// dt_focal.hip -- focal statistics at any radius: count, mean, standard deviation, TPI, DEV and the multi-scale DEVmax
// of the (2 radius + 1)^2 window of every cell (Weiss 2001; De Reu et al. 2013; Lindsay et al. 2015; net-new,
// descriptools_amd/focal.py holds the definition).
//
// The window sums come from summed-area tables: the inclusive two-dimensional prefix sums of [valid], q and q^2, q the
// height quantised to 2^-frac_bits units above `origin`.  The q and q^2 planes are uint64 and wrap: a window sum that
// fits 63 bits comes out of the four-corner difference exactly whatever the table did, so the planes are the same bits
// however the scan is cut, and every output is the numpy reference's bit for bit.
//
// The scan, three launches whatever the raster holds; a band is FC_BH rows:
// k_fc_band_sums  per band and column the sums of [valid], q, q^2 over the band's rows, from the heights (4 B / cell
//                 read); raises DT_STATUS_BAD_HEIGHT for a valid height outside 0 <= q <= qmax, which counts as q = 0.
// k_fc_band_scan  per column the exclusive scan of those sums down the bands, in place: the column sums above a band.
// k_fc_scan       one wave per band walks the band's rows left to right, 256 columns at a time.  A lane holds four
//                 adjacent columns and their running column sums C(y, x) = sum of rows 0 .. y, which start at the band's
//                 carry; P(y, x) = sum over x' <= x of C(y, x') is a prefix along the row: four terms in the lane, a
//                 wave64 shuffle scan of the lanes' totals, and the row's carry from the chunks before.  The heights are
//                 read a second time and the planes written once: 28 B / cell with the first launch.
// No atomics on the planes, no host synchronisation, nothing depends on the rasters' content.
//
// k_fc_eval       one thread per cell: per radius the clipped corners, four loads per plane, the modular differences
//                 and the float64 stage; MULTI is the DEVmax form over a table of up to 32 radii in kernel arguments.
#include <cmath>

#include "dt_common.h"
#include "dt_kernels.h"

#define FC_BH 8     // rows of a band
#define FC_CPL 4    // columns a lane holds
#define FC_CHUNK (64 * FC_CPL)

struct FcQuant {
  double origin, scale, qmax;  // q = rint((z - origin) * scale), scale = 2^frac_bits, 0 <= q <= qmax
};

// the quantised height of a cell: false for a height that is not valid (q = 0); a valid height outside the contract
// sets `bad` and counts as q = 0, so nothing downstream sees a value the bounds were not made for
__device__ __forceinline__ bool fc_quant(float z, const FcQuant &Q, uint32_t &q, bool &bad) {
  q = 0;
  if (!(z > -100.0f && z < INFINITY)) return false;
  const double t = rint(((double)z - Q.origin) * Q.scale);
  if (t >= 0.0 && t <= Q.qmax)
    q = (uint32_t)t;  // qmax < 2^30
  else
    bad = true;
  return true;
}

struct FcLayout {
  uint32_t *Pn;        // per cell: the prefix count
  uint64_t *P1, *P2;   // per cell: the prefix sums of q and q^2, modulo 2^64
  uint32_t *cn;        // per band and column: the count of the rows above the band
  uint64_t *c1, *c2;   // ... and their sums of q and q^2
  int64_t bands;
  size_t bytes;
};
static FcLayout fc_layout(int64_t H, int64_t W, void *scratch) {
  FcLayout L = {};
  DtCarver c(scratch);
  const size_t n = (size_t)(H * W);
  L.bands = (H + FC_BH - 1) / FC_BH;
  const size_t nc = (size_t)(L.bands * W);
  L.Pn = c.take<uint32_t>(n);
  L.P1 = c.take<uint64_t>(n);
  L.P2 = c.take<uint64_t>(n);
  L.cn = c.take<uint32_t>(nc);
  L.c1 = c.take<uint64_t>(nc);
  L.c2 = c.take<uint64_t>(nc);
  L.bytes = c.bytes();
  return L;
}
size_t dt_focal_scratch(int64_t H, int64_t W) { return fc_layout(H, W, nullptr).bytes; }

// ---- the scan --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fc_band_sums(const float *__restrict__ dem, int H, int W, int col_blocks,
                                                      FcQuant Q, uint32_t *__restrict__ cn, uint64_t *__restrict__ c1,
                                                      uint64_t *__restrict__ c2, int *status) {
  const int b = (int)(blockIdx.x / (unsigned)col_blocks), cb = (int)(blockIdx.x - (unsigned)b * (unsigned)col_blocks);
  const long long x = (long long)cb * 256 + (int)threadIdx.x;
  if (x >= W) return;
  const long long y0 = (long long)b * FC_BH;
  uint32_t n = 0;
  uint64_t s1 = 0, s2 = 0;
  bool bad = false;
#pragma unroll
  for (int r = 0; r < FC_BH; r++) {
    const long long y = y0 + r;
    if (y >= H) break;
    uint32_t q;
    if (fc_quant(dem[y * W + x], Q, q, bad)) {
      n++;
      s1 += q;
      s2 += (uint64_t)q * q;
    }
  }
  const long long o = (long long)b * W + x;
  cn[o] = n;
  c1[o] = s1;
  c2[o] = s2;
  if (bad && status) atomicOr(status, DT_STATUS_BAD_HEIGHT);
}

// one wave per workgroup, so that a raster of 16,384 columns has a wave on every CU; unrolled, so that a lane has the
// loads of eight bands in flight and only the additions wait for each other
__global__ __launch_bounds__(64) void k_fc_band_scan(int W, int bands, uint32_t *__restrict__ cn,
                                                     uint64_t *__restrict__ c1, uint64_t *__restrict__ c2) {
  const long long x = (long long)blockIdx.x * 64 + (int)threadIdx.x;
  if (x >= W) return;
  uint32_t n = 0;
  uint64_t s1 = 0, s2 = 0;
  for (int b0 = 0; b0 < bands; b0 += 8) {
    uint32_t tn[8];
    uint64_t t1[8], t2[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const bool in = b0 + k < bands;
      const long long o = (long long)(b0 + k) * W + x;
      tn[k] = in ? cn[o] : 0u;
      t1[k] = in ? c1[o] : 0ull;
      t2[k] = in ? c2[o] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (b0 + k < bands) {
        const long long o = (long long)(b0 + k) * W + x;
        cn[o] = n;
        c1[o] = s1;
        c2[o] = s2;
      }
      n += tn[k];
      s1 += t1[k];
      s2 += t2[k];
    }
  }
}

// inclusive scan of one value per lane over the wave's 64 lanes
template <typename T>
__device__ __forceinline__ T fc_wave_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, (unsigned)o);
    if (lane >= o) v += t;
  }
  return v;
}

// vec: the heights and the planes may be read and written 16 bytes at a time (W % 4 == 0, aligned bases)
__global__ __launch_bounds__(64) void k_fc_scan(const float *__restrict__ dem, int H, int W, FcQuant Q,
                                                const uint32_t *__restrict__ cn, const uint64_t *__restrict__ c1,
                                                const uint64_t *__restrict__ c2, int vec, uint32_t *__restrict__ Pn,
                                                uint64_t *__restrict__ P1, uint64_t *__restrict__ P2) {
  const int lane = (int)threadIdx.x;
  const long long b = blockIdx.x, y0 = b * FC_BH;
  uint32_t rn[FC_BH];  // the rows' carries: P at the last column of the chunks before
  uint64_t r1[FC_BH], r2[FC_BH];
#pragma unroll
  for (int r = 0; r < FC_BH; r++) {
    rn[r] = 0;
    r1[r] = 0;
    r2[r] = 0;
  }
  for (long long xc = 0; xc < W; xc += FC_CHUNK) {
    const long long x = xc + FC_CPL * lane;
    const bool full = x + FC_CPL <= W;
    uint32_t an[FC_CPL];  // the running column sums of the lane's columns
    uint64_t a1[FC_CPL], a2[FC_CPL];
#pragma unroll
    for (int j = 0; j < FC_CPL; j++) {
      const bool in = x + j < W;
      const long long o = b * W + x + j;
      an[j] = in ? cn[o] : 0u;
      a1[j] = in ? c1[o] : 0ull;
      a2[j] = in ? c2[o] : 0ull;
    }
#pragma unroll
    for (int r = 0; r < FC_BH; r++) {
      const long long y = y0 + r;
      if (y >= H) break;  // the same for every lane
      const long long o = y * W + x;
      float z[FC_CPL];
      if (vec && full) {
        const float4 v = *reinterpret_cast<const float4 *>(dem + o);
        z[0] = v.x;
        z[1] = v.y;
        z[2] = v.z;
        z[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < FC_CPL; j++) z[j] = x + j < W ? dem[o + j] : DT_NODATA;
      }
      uint32_t pn[FC_CPL];
      uint64_t p1[FC_CPL], p2[FC_CPL];
      bool bad = false;
#pragma unroll
      for (int j = 0; j < FC_CPL; j++) {
        uint32_t q;
        if (fc_quant(z[j], Q, q, bad)) {
          an[j]++;
          a1[j] += q;
          a2[j] += (uint64_t)q * q;
        }
        pn[j] = an[j] + (j ? pn[j - 1] : 0u);
        p1[j] = a1[j] + (j ? p1[j - 1] : 0ull);
        p2[j] = a2[j] + (j ? p2[j - 1] : 0ull);
      }
      const uint32_t in_n = fc_wave_scan(pn[FC_CPL - 1], lane);
      const uint64_t in_1 = fc_wave_scan((unsigned long long)p1[FC_CPL - 1], lane);
      const uint64_t in_2 = fc_wave_scan((unsigned long long)p2[FC_CPL - 1], lane);
      const uint32_t bn = rn[r] + (in_n - pn[FC_CPL - 1]);
      const uint64_t b1 = r1[r] + (in_1 - p1[FC_CPL - 1]), b2 = r2[r] + (in_2 - p2[FC_CPL - 1]);
      if (vec && full) {
        *reinterpret_cast<uint4 *>(Pn + o) = make_uint4(bn + pn[0], bn + pn[1], bn + pn[2], bn + pn[3]);
        *reinterpret_cast<ulonglong2 *>(P1 + o) = make_ulonglong2(b1 + p1[0], b1 + p1[1]);
        *reinterpret_cast<ulonglong2 *>(P1 + o + 2) = make_ulonglong2(b1 + p1[2], b1 + p1[3]);
        *reinterpret_cast<ulonglong2 *>(P2 + o) = make_ulonglong2(b2 + p2[0], b2 + p2[1]);
        *reinterpret_cast<ulonglong2 *>(P2 + o + 2) = make_ulonglong2(b2 + p2[2], b2 + p2[3]);
      } else {
#pragma unroll
        for (int j = 0; j < FC_CPL; j++) {
          if (x + j < W) {
            Pn[o + j] = bn + pn[j];
            P1[o + j] = b1 + p1[j];
            P2[o + j] = b2 + p2[j];
          }
        }
      }
      rn[r] += __shfl(in_n, 63);
      r1[r] += (uint64_t)__shfl((unsigned long long)in_1, 63);
      r2[r] += (uint64_t)__shfl((unsigned long long)in_2, 63);
    }
  }
}

// ---- evaluation --------------------------------------------------------------------------------------------------------
struct FcEval {
  int n;                             // radii
  int radius[DT_FOCAL_RADII_MAX];
  double origin, u;                  // u = 2^-frac_bits
  int32_t *count;
  float *mean, *std_, *tpi, *dev;
  uint16_t *scale;
};

// the window of radius R around (y, x): n, A = sum (q_i - q_c), B = sum (q_i - q_c)^2 from the planes
__device__ __forceinline__ void fc_window(const uint32_t *__restrict__ Pn, const uint64_t *__restrict__ P1,
                                          const uint64_t *__restrict__ P2, int H, int W, int y, int x, int R,
                                          uint64_t qc, uint32_t &n, int64_t &A, int64_t &B) {
  const int ya = (y > R ? y - R : 0) - 1, yb = y + (R < H - 1 - y ? R : H - 1 - y);
  const int xa = (x > R ? x - R : 0) - 1, xb = x + (R < W - 1 - x ? R : W - 1 - x);
  const long long o11 = (long long)yb * W + xb, o01 = (long long)ya * W + xb, o10 = (long long)yb * W + xa,
                  o00 = (long long)ya * W + xa;
  n = Pn[o11];
  uint64_t s1 = P1[o11], s2 = P2[o11];
  if (ya >= 0) {
    n -= Pn[o01];
    s1 -= P1[o01];
    s2 -= P2[o01];
  }
  if (xa >= 0) {
    n -= Pn[o10];
    s1 -= P1[o10];
    s2 -= P2[o10];
  }
  if (ya >= 0 && xa >= 0) {
    n += Pn[o00];
    s1 += P1[o00];
    s2 += P2[o00];
  }
  const uint64_t nn = n;
  A = (int64_t)(s1 - nn * qc);
  B = (int64_t)(s2 - 2ull * qc * s1 + nn * qc * qc);
}
// the float64 stage: a = A / n and sd = sqrt(max(B / n - a a, 0))
__device__ __forceinline__ void fc_moments(uint32_t n, int64_t A, int64_t B, double &a, double &sd) {
  const double nf = (double)n;
  a = (double)A / nf;
  const double b = (double)B / nf;
  double var = b - a * a;
  if (var < 0.0) var = 0.0;
  sd = sqrt(var);
}

template <bool MULTI>
__global__ __launch_bounds__(256) void k_fc_eval(const float *__restrict__ dem, int H, int W, FcQuant Q,
                                                 const uint32_t *__restrict__ Pn, const uint64_t *__restrict__ P1,
                                                 const uint64_t *__restrict__ P2, FcEval E) {
  const long long i = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= (long long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  uint32_t qc;
  bool bad = false;
  if (!fc_quant(dem[i], Q, qc, bad)) {
    if (MULTI) {
      if (E.dev) E.dev[i] = NAN;
      if (E.scale) E.scale[i] = 0;
    } else {
      if (E.count) E.count[i] = 0;
      if (E.mean) E.mean[i] = DT_NODATA;
      if (E.std_) E.std_[i] = DT_NODATA;
      if (E.tpi) E.tpi[i] = NAN;
      if (E.dev) E.dev[i] = NAN;
      if (E.scale) E.scale[i] = 0;
    }
    return;
  }
  uint32_t n;
  int64_t A, B;
  double a, sd;
  if (MULTI) {
    double best = 0.0;
    int at = 0;
    for (int k = 0; k < E.n; k++) {
      fc_window(Pn, P1, P2, H, W, y, x, E.radius[k], qc, n, A, B);
      fc_moments(n, A, B, a, sd);
      const double d = sd == 0.0 ? 0.0 : (-a) / sd;
      if (k == 0 || fabs(d) > fabs(best)) {  // a tie keeps the smaller radius
        best = d;
        at = E.radius[k];
      }
    }
    if (E.dev) E.dev[i] = (float)best;
    if (E.scale) E.scale[i] = (uint16_t)at;
  } else {
    fc_window(Pn, P1, P2, H, W, y, x, E.radius[0], qc, n, A, B);
    fc_moments(n, A, B, a, sd);
    if (E.count) E.count[i] = (int32_t)n;
    if (E.mean) E.mean[i] = (float)(E.origin + ((double)qc + a) * E.u);
    if (E.std_) E.std_[i] = (float)(sd * E.u);
    if (E.tpi) E.tpi[i] = (float)((-a) * E.u);
    if (E.dev) E.dev[i] = sd == 0.0 ? 0.0f : (float)((-a) / sd);
    if (E.scale) E.scale[i] = (uint16_t)E.radius[0];
  }
}

// the largest integer q with (2 radius + 1)^2 q^2 < 2^63
int64_t dt_focal_qmax(int radius) {
  const uint64_t m = (uint64_t)(2 * radius + 1) * (uint64_t)(2 * radius + 1);
  const uint64_t t = ((1ull << 63) - 1) / m;  // q^2 <= t
  uint64_t q = (uint64_t)sqrt((double)t);
  while (q * q > t) q--;
  while ((q + 1) * (q + 1) <= t) q++;
  return (int64_t)q;
}

int dt_launch_focal(hipStream_t s, const float *dem, int64_t H, int64_t W, double origin, int frac_bits,
                    const int32_t *radii, int n_radii, void *scratch, size_t scratch_bytes, int32_t *count,
                    float *mean, float *std_, float *tpi, float *dev, uint16_t *scale, int *status) {
  DT_REQUIRE(n_radii >= 1 && n_radii <= DT_FOCAL_RADII_MAX && radii, "1..32 radii per call");
  for (int k = 0; k < n_radii; k++) {
    DT_REQUIRE(radii[k] >= 1 && radii[k] <= DT_FOCAL_RADIUS_MAX, "a radius must lie in [1, 4096]");
    DT_REQUIRE(k == 0 || radii[k] > radii[k - 1], "radii must be strictly increasing");
  }
  DT_REQUIRE(frac_bits >= 0 && frac_bits <= DT_FOCAL_FRAC_BITS_MAX, "frac_bits must lie in [0, 24]");
  DT_REQUIRE(std::isfinite(origin), "origin must be finite");
  if (H == 0 || W == 0) return DT_OK;
  const FcLayout L = fc_layout(H, W, scratch);
  DT_REQUIRE(scratch && scratch_bytes >= L.bytes, "scratch too small");
  FcQuant Q;
  Q.origin = origin;
  Q.scale = ldexp(1.0, frac_bits);
  Q.qmax = (double)dt_focal_qmax(radii[n_radii - 1]);
  const int64_t col_blocks = (W + 255) / 256;
  const int vec = W % 4 == 0 && ((uintptr_t)dem & 15) == 0;  // the planes are 256-byte aligned
  hipLaunchKernelGGL(k_fc_band_sums, dim3((unsigned)(L.bands * col_blocks)), dim3(256), 0, s, dem, (int)H, (int)W,
                     (int)col_blocks, Q, L.cn, L.c1, L.c2, status);
  hipLaunchKernelGGL(k_fc_band_scan, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, s, (int)W, (int)L.bands, L.cn, L.c1,
                     L.c2);
  hipLaunchKernelGGL(k_fc_scan, dim3((unsigned)L.bands), dim3(64), 0, s, dem, (int)H, (int)W, Q, L.cn, L.c1, L.c2,
                     vec, L.Pn, L.P1, L.P2);
  FcEval E = {};
  E.n = n_radii;
  for (int k = 0; k < n_radii; k++) E.radius[k] = radii[k];
  E.origin = origin;
  E.u = ldexp(1.0, -frac_bits);
  E.count = count;
  E.mean = mean;
  E.std_ = std_;
  E.tpi = tpi;
  E.dev = dev;
  E.scale = scale;
  const unsigned blocks = (unsigned)((H * W + 255) / 256);
  if (n_radii > 1)
    hipLaunchKernelGGL(k_fc_eval<true>, dim3(blocks), dim3(256), 0, s, dem, (int)H, (int)W, Q, L.Pn, L.P1, L.P2, E);
  else
    hipLaunchKernelGGL(k_fc_eval<false>, dim3(blocks), dim3(256), 0, s, dem, (int)H, (int)W, Q, L.Pn, L.P1, L.P2, E);
  return DT_OK;
}
