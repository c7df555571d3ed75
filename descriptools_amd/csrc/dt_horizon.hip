// dt_horizon.hip -- what a cell sees along eight lines of sight: geomorphon landforms and their ternary patterns
// (Jasiewicz & Stepinski 2013), positive and negative topographic openness (Yokoyama et al. 2002) and the sky-view
// factor (Zaksek et al. 2011); net-new, descriptools_amd/horizon.py holds the definition.
//
// All of them derive from one pair per direction: the largest and the smallest tangent of the elevation angle to the
// samples k = skip + 1 .. radius of that direction, t = (z_k - z0) * inv[c][k] in float64 on the float32 heights, with
// inv the tabulated reciprocal of the distance (the launcher builds it on the host; the kernel divides nowhere in its
// inner loop).  The extremes start as NaN and grow by fmax / fmin, which return the operand that is not NaN: a height
// that is not valid, or lies outside the raster, is staged as NaN and so drops out of the extremes without a test, and
// a direction without a sample is a maximum that is still NaN -- no count is kept.
//
// k_horizon   one launch: a workgroup stages the heights of its TX x TY tile with a halo of `radius` cells as float32
//             in LDS (TX = 64: a wave takes 64 consecutive cells of one row, so the k-th sample of any direction is a
//             stride-1 LDS read across the wave and no bank conflict arises).  A lane finishes one direction -- its
//             digit, its two openness terms, its sky-view term -- before the next, so the eight pairs never live in
//             registers together.  DIG / OPEN / SKY are the three families of outputs: an instance without OPEN has no
//             atan, one without SKY no square root and no division.
#include <cmath>

#include "dt_dinf_common.h"

#define HZ_HALF_PI 1.5707963267948966

struct HzArgs {
  double inv[2][DT_HORIZON_RADIUS_MAX];  // inv[c][k - 1] = 1 / (k step[c]); c = 0 cardinal, 1 diagonal
  double flat_tan;
  uint8_t *landform;
  uint16_t *pattern;
  float *positive, *negative, *sky_view;
  int r, skip;
};

// landform of (m, p) = the numbers of -1 and +1 digits; m + p > 8 does not occur
__constant__ uint8_t HZ_FORM[9][9] = {{1, 1, 1, 8, 8, 9, 9, 9, 10}, {1, 1, 8, 8, 8, 9, 9, 9, 0}, {1, 4, 6, 6, 7, 7, 9, 0, 0},
                                      {4, 4, 6, 6, 6, 7, 0, 0, 0},  {4, 4, 5, 6, 6, 0, 0, 0, 0}, {3, 3, 5, 5, 0, 0, 0, 0, 0},
                                      {3, 3, 3, 0, 0, 0, 0, 0, 0},  {3, 3, 0, 0, 0, 0, 0, 0, 0}, {2, 0, 0, 0, 0, 0, 0, 0, 0}};

// the row / column step of direction d = N, NE, E, SE, S, SW, W, NW: two bits of (step + 1) per direction
__device__ __forceinline__ int hz_dy(int d) { return (int)((0x1A90u >> (2 * d)) & 3u) - 1; }  // -1 -1 0 1 1 1 0 -1
__device__ __forceinline__ int hz_dx(int d) { return (int)((0x01A9u >> (2 * d)) & 3u) - 1; }  // 0 1 1 1 0 -1 -1 -1

// The tile is TX x TY cells, RMAX the largest radius the instantiation has LDS for, NT its threads; wt = TX + 2 r is
// the run-time width of the staged block, TY + 2 r its rows.
template <int TX, int TY, int RMAX, int NT, bool DIG, bool OPEN, bool SKY>
__global__ __launch_bounds__(NT) void k_horizon(const float *__restrict__ dem, int H, int W, int tiles_x, HzArgs A) {
  __shared__ float h[(TY + 2 * RMAX) * (TX + 2 * RMAX)];
  const int r = A.r;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * TX, y0 = tyi * TY;
  const int wt = TX + 2 * r, ht = TY + 2 * r;
  for (int i = (int)threadIdx.x; i < ht * wt; i += NT) {
    const int row = i / wt, col = i - row * wt;
    const int gy = y0 - r + row, gx = x0 - r + col;
    float v = NAN;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      v = dem[(long long)gy * W + gx];
      if (!di_valid(v)) v = NAN;
    }
    h[i] = v;
  }
  __syncthreads();
  for (int i = (int)threadIdx.x; i < TX * TY; i += NT) {
    const int ly = i / TX, lx = i - ly * TX;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const float *hc = &h[(ly + r) * wt + lx + r];
    const float c32 = *hc;
    const double z0 = (double)c32;
    bool has = c32 == c32;
    unsigned pat = 0, pw = 1;
    int m = 0, p = 0;
    double pos = 0.0, neg = 0.0, sky = 0.0;  // 0.0 + the d = 0 term is that term
    if (has) {
#pragma unroll 1
      for (int d = 0; d < 8; d++) {
        const int off = hz_dy(d) * wt + hz_dx(d);
        const double *inv = A.inv[d & 1];
        const float *q = hc + A.skip * off;
        double tmax = NAN, tmin = NAN;
#pragma unroll 4
        for (int k = A.skip; k < r; k++) {  // the sample at distance k + 1
          q += off;
          const double t = ((double)*q - z0) * inv[k];
          tmax = fmax(tmax, t);
          if (DIG || OPEN) tmin = fmin(tmin, t);
        }
        // no sample in this direction: no value.  The other directions still run (their results are dropped), which
        // keeps d and the table's row uniform across the wave: scalar loads of the reciprocals.
        has = has && tmax == tmax;
        if (DIG) {
          const double a = fabs(tmax), b = fabs(tmin);
          const unsigned dg = (a > b && a > A.flat_tan) ? 2u : ((b > A.flat_tan && a <= b) ? 0u : 1u);  // digit + 1
          pat += dg * pw;
          pw *= 3u;
          m += dg == 0u;
          p += dg == 2u;
        }
        if (OPEN) {
          if (A.positive) pos += HZ_HALF_PI - atan(tmax);
          if (A.negative) neg += HZ_HALF_PI + atan(tmin);
        }
        if (SKY) sky += tmax > 0.0 ? tmax / sqrt(1.0 + tmax * tmax) : 0.0;
      }
    }
    const long long o = (long long)gy * W + gx;
    if (DIG) {
      if (A.landform) A.landform[o] = has ? HZ_FORM[m][p] : (uint8_t)0;
      if (A.pattern) A.pattern[o] = has ? (uint16_t)pat : (uint16_t)65535;
    }
    if (OPEN) {
      if (A.positive) A.positive[o] = has ? (float)(pos / 8.0) : DT_NODATA;
      if (A.negative) A.negative[o] = has ? (float)(neg / 8.0) : DT_NODATA;
    }
    if (SKY) A.sky_view[o] = has ? (float)(1.0 - sky / 8.0) : DT_NODATA;
  }
}

template <int TX, int TY, int RMAX, int NT>
static void hz_launch(hipStream_t s, int what, const float *dem, int64_t H, int64_t W, const HzArgs &A) {
  static_assert(sizeof(float) * (TY + 2 * RMAX) * (TX + 2 * RMAX) <= 160 * 1024, "the LDS of a compute unit");
  static_assert(TX == 64 && (TX * TY) % NT == 0, "a wave is one row of 64 cells");
  const int tiles_x = (int)((W + TX - 1) / TX);
  const unsigned nt = (unsigned)(((H + TY - 1) / TY) * tiles_x);
  void (*k)(const float *, int, int, int, HzArgs) = nullptr;
  switch (what) {  // bit 0: digits, bit 1: openness, bit 2: sky view
    case 1: k = k_horizon<TX, TY, RMAX, NT, true, false, false>; break;
    case 2: k = k_horizon<TX, TY, RMAX, NT, false, true, false>; break;
    case 3: k = k_horizon<TX, TY, RMAX, NT, true, true, false>; break;
    case 4: k = k_horizon<TX, TY, RMAX, NT, false, false, true>; break;
    case 5: k = k_horizon<TX, TY, RMAX, NT, true, false, true>; break;
    case 6: k = k_horizon<TX, TY, RMAX, NT, false, true, true>; break;
    default: k = k_horizon<TX, TY, RMAX, NT, true, true, true>; break;
  }
  hipLaunchKernelGGL(k, dim3(nt), dim3(NT), 0, s, dem, (int)H, (int)W, tiles_x, A);
}

int dt_launch_horizon(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, int radius, int skip,
                      double flat_tan, uint8_t *landform, uint16_t *pattern, float *positive, float *negative,
                      float *sky_view) {
  DT_REQUIRE(radius >= 1 && radius <= DT_HORIZON_RADIUS_MAX, "radius must lie in [1, 64]");
  DT_REQUIRE(skip >= 0 && skip < radius, "skip must lie in [0, radius - 1]");
  DT_REQUIRE(std::isfinite(flat_tan) && flat_tan >= 0.0, "flat_tan must be finite and >= 0");
  if (H == 0 || W == 0) return DT_OK;
  const int what = ((landform || pattern) ? 1 : 0) | ((positive || negative) ? 2 : 0) | (sky_view ? 4 : 0);
  DT_REQUIRE(what, "no output raster");
  HzArgs A;
  const double step[2] = {px, px * 1.4142135623730951};
  for (int c = 0; c < 2; c++)
    for (int k = 1; k <= DT_HORIZON_RADIUS_MAX; k++) A.inv[c][k - 1] = 1.0 / ((double)k * step[c]);
  A.flat_tan = flat_tan;
  A.landform = landform;
  A.pattern = pattern;
  A.positive = positive;
  A.negative = negative;
  A.sky_view = sky_view;
  A.r = radius;
  A.skip = skip;
  if (radius <= 4) {
    hz_launch<64, 16, 4, 256>(s, what, dem, H, W, A);
  } else if (radius <= 16) {
    hz_launch<64, 32, 16, 256>(s, what, dem, H, W, A);
  } else if (radius <= 32) {
    hz_launch<64, 64, 32, 1024>(s, what, dem, H, W, A);
  } else {
    hz_launch<64, 64, 64, 1024>(s, what, dem, H, W, A);
  }
  return DT_OK;
}
