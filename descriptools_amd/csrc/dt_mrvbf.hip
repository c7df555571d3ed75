// dt_mrvbf.hip -- multi-resolution valley bottom flatness MRVBF and ridge top flatness MRRTF (Gallant & Dowling 2003),
// with the two building blocks that are ops of their own: the elevation percentile of a disc (Lindsay's EP) and one
// generalisation step (Gaussian smoothing, slope, coarsening by 3); net-new, descriptools_amd/mrvbf.py holds the
// definition.
//
// k_percentile  a workgroup stages the heights of its 64 x 16 tile with a halo of `radius` cells as float32 in LDS, NaN
//               for a height that is not valid or lies outside the raster.  A lane takes MV_RB cells of one column and
//               walks the staged rows of their discs once: a value read from LDS is compared with every one of the
//               lane's centres whose disc holds it (which ones is the same for the whole wave: scalar branches).
//               Integer counts n, l, h, then one float64 division.  The op itself and every pyramid level.
// k_coarsen     a workgroup makes 16 x 8 coarse cells: the 48 x 24 fine cells with a halo of 6 in LDS, the row sums of
//               the 11-tap Gaussian (numerator and denominator, float64), their column sums on the fine tile and one
//               ring around it, the slope of that smoothed surface, and the 3 x 3 block means of both.
// k_mrvbf       ONE launch at base resolution: the tile with a halo of 6, the base slope, the radius-3 and radius-6
//               counts in one walk (the inner disc's cells are counted apart and added), then the levels in registers:
//               the level's small slope and percentile rasters are interpolated from the pyramid, whose pointers,
//               shapes, thresholds and exponents are the kernel argument.
// The pyramid (float32 DEM, slope, lower and higher percentile per level >= 3) lives in `scratch`; 2 (levels - 2)
// launches build it.  No atomics, no host synchronisation.
#include <cmath>

#include "dt_common.h"
#include "dt_kernels.h"

#define MV_TX 64   // a wave takes 64 consecutive cells of one row: stride-1 LDS reads
#define MV_TY 16
#define MV_RB 4    // cells of a column that a lane takes
#define MV_NT 256  // MV_TX * MV_TY / MV_RB
#define MV_R2 6    // the radius of level 2 and of every pyramid level
#define MV_R1 3    // the radius of level 1

__device__ __forceinline__ bool mv_valid(float z) { return z > -100.0f && z < INFINITY; }

// half widths of the disc dx^2 + dy^2 <= r^2 by |dy|
struct MvDisc {
  int r;
  int hw[DT_PERCENTILE_RADIUS_MAX + 1];
};
static MvDisc mv_disc(int r) {
  MvDisc D = {};
  D.r = r;
  for (int dy = 0; dy <= r; dy++) {
    int w = 0;
    while ((w + 1) * (w + 1) + dy * dy <= r * r) w++;
    D.hw[dy] = w;
  }
  return D;
}

// the MV_TX x MV_TY tile at (x0, y0) with a halo of r cells, NaN where there is no valid height
__device__ __forceinline__ void mv_stage(float *h, const float *__restrict__ dem, int H, int W, int x0, int y0, int r) {
  const int wt = MV_TX + 2 * r, ht = MV_TY + 2 * r;
  for (int i = (int)threadIdx.x; i < ht * wt; i += MV_NT) {
    const int row = i / wt, col = i - row * wt;
    const int gy = y0 - r + row, gx = x0 - r + col;
    float v = NAN;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      v = dem[(long long)gy * W + gx];
      if (!mv_valid(v)) v = NAN;
    }
    h[i] = v;
  }
}

struct MvCount {
  int n[MV_RB], l[MV_RB], h[MV_RB];
};
__device__ __forceinline__ void mv_zero(MvCount &c) {
#pragma unroll
  for (int b = 0; b < MV_RB; b++) c.n[b] = c.l[b] = c.h[b] = 0;
}
__device__ __forceinline__ void mv_tally(MvCount &c, int b, float v, float zc) {
  c.n[b] += v == v;
  c.l[b] += v < zc;
  c.h[b] += v > zc;
}

// The counts of the discs D of the lane's MV_RB cells hc[0], hc[wt], ...: the staged rows j = -r .. MV_RB - 1 + r
// relative to the first cell, each read once.  INNER: the cells of the smaller disc Din go to `in` and are added to
// `out` at the end.  Everything but hc and zc is the same across the wave.
template <bool INNER>
__device__ __forceinline__ void mv_counts(const float *hc, int wt, const MvDisc &D, const MvDisc &Din,
                                          const float (&zc)[MV_RB], MvCount &out, MvCount &in) {
  mv_zero(out);
  if (INNER) mv_zero(in);
  const int r = D.r;
  for (int j = -r; j < MV_RB + r; j++) {
    int w[MV_RB], wi[MV_RB], wmax = -1;
#pragma unroll
    for (int b = 0; b < MV_RB; b++) {
      const int ady = j >= b ? j - b : b - j;
      w[b] = ady <= r ? D.hw[ady] : -1;
      wi[b] = INNER && ady <= Din.r ? Din.hw[ady] : -1;
      wmax = w[b] > wmax ? w[b] : wmax;
    }
    const float *row = hc + j * wt;
    for (int dx = -wmax; dx <= wmax; dx++) {
      const float v = row[dx];
      const int adx = dx < 0 ? -dx : dx;
#pragma unroll
      for (int b = 0; b < MV_RB; b++) {
        if (INNER && adx <= wi[b])
          mv_tally(in, b, v, zc[b]);
        else if (adx <= w[b])
          mv_tally(out, b, v, zc[b]);
      }
    }
  }
  if (INNER) {
#pragma unroll
    for (int b = 0; b < MV_RB; b++) {
      out.n[b] += in.n[b];
      out.l[b] += in.l[b];
      out.h[b] += in.h[b];
    }
  }
}

// ---- elevation percentile ------------------------------------------------------------------------------------------
struct PcArgs {
  MvDisc D;
  float *lower, *higher;
};

__global__ __launch_bounds__(MV_NT) void k_percentile(const float *__restrict__ dem, int H, int W, int tiles_x,
                                                      PcArgs A) {
  __shared__ float h[(MV_TY + 2 * DT_PERCENTILE_RADIUS_MAX) * (MV_TX + 2 * DT_PERCENTILE_RADIUS_MAX)];
  const int r = A.D.r, wt = MV_TX + 2 * r;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * MV_TX, y0 = tyi * MV_TY;
  mv_stage(h, dem, H, W, x0, y0, r);
  __syncthreads();
  const int lx = (int)threadIdx.x & (MV_TX - 1);
  const int ly0 = __builtin_amdgcn_readfirstlane((int)threadIdx.x / MV_TX) * MV_RB;  // a wave is one row of lanes
  const float *hc = &h[(ly0 + r) * wt + lx + r];
  float zc[MV_RB];
#pragma unroll
  for (int b = 0; b < MV_RB; b++) zc[b] = hc[b * wt];
  MvCount c, unused;
  mv_counts<false>(hc, wt, A.D, A.D, zc, c, unused);
  const int gx = x0 + lx;
#pragma unroll
  for (int b = 0; b < MV_RB; b++) {
    const int gy = y0 + ly0 + b;
    if (gy >= H || gx >= W) continue;
    const long long o = (long long)gy * W + gx;
    const bool has = zc[b] == zc[b];
    const double nf = (double)c.n[b];
    if (A.lower) A.lower[o] = has ? (float)((double)c.l[b] / nf) : DT_NODATA;
    if (A.higher) A.higher[o] = has ? (float)((double)c.h[b] / nf) : DT_NODATA;
  }
}

int dt_launch_percentile(hipStream_t s, const float *dem, int64_t H, int64_t W, int radius, float *lower,
                         float *higher) {
  DT_REQUIRE(radius >= 1 && radius <= DT_PERCENTILE_RADIUS_MAX, "radius must lie in [1, 16]");
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(lower || higher, "no output raster");
  PcArgs A;
  A.D = mv_disc(radius);
  A.lower = lower;
  A.higher = higher;
  const int tiles_x = (int)((W + MV_TX - 1) / MV_TX);
  const unsigned nt = (unsigned)(((H + MV_TY - 1) / MV_TY) * tiles_x);
  hipLaunchKernelGGL(k_percentile, dim3(nt), dim3(MV_NT), 0, s, dem, (int)H, (int)W, tiles_x, A);
  return DT_OK;
}

// ---- slope of a float64 surface, NaN where it has no value ---------------------------------------------------------
__device__ __forceinline__ double mv_gradient(double zm, double z, double zp, double c) {
  const bool okm = zm == zm, okp = zp == zp;
  if (okp && okm) return (zp - zm) / (2.0 * c);
  if (okp) return (zp - z) / c;
  if (okm) return (z - zm) / c;
  return 0.0;
}
__device__ __forceinline__ double mv_slope(double west, double east, double north, double south, double z, double c) {
  const double p = mv_gradient(west, z, east, c), q = mv_gradient(north, z, south, c);
  return 100.0 * sqrt(p * p + q * q);
}

// ---- one generalisation step ---------------------------------------------------------------------------------------
#define CO_CX 16             // coarse cells of a tile
#define CO_CY 8
#define CO_FW (3 * CO_CX)    // its fine cells
#define CO_FH (3 * CO_CY)
#define CO_ZW (CO_FW + 12)   // the staged heights: a halo of 6
#define CO_ZH (CO_FH + 12)
#define CO_RW (CO_FW + 2)    // the smoothed surface: a ring of 1 for the slope; the row sums have these columns
#define CO_SH (CO_FH + 2)
static_assert(CO_CX * CO_CY <= 256, "a lane per coarse cell");

struct CoArgs {
  double g[6];  // exp(-k^2 / 18)
  double c;     // the cell size of the fine raster
};

__global__ __launch_bounds__(256) void k_coarsen(const float *__restrict__ dem, int H, int W, int Hc, int Wc,
                                                 int tiles_x, CoArgs A, float *__restrict__ dem3,
                                                 float *__restrict__ slope3) {
  __shared__ float z[CO_ZH * CO_ZW];
  __shared__ double rn[CO_ZH * CO_RW], rd[CO_ZH * CO_RW];
  __shared__ double sm[CO_SH * CO_RW];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int fx0 = txi * CO_FW, fy0 = tyi * CO_FH;
  for (int i = (int)threadIdx.x; i < CO_ZH * CO_ZW; i += 256) {
    const int row = i / CO_ZW, col = i - row * CO_ZW;
    const int gy = fy0 - 6 + row, gx = fx0 - 6 + col;
    float v = NAN;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      v = dem[(long long)gy * W + gx];
      if (!mv_valid(v)) v = NAN;
    }
    z[i] = v;
  }
  __syncthreads();
  // row sums at the staged rows and the fine columns fx0 - 1 .. fx0 + CO_FW: column `col` is staged column col + 5
  for (int i = (int)threadIdx.x; i < CO_ZH * CO_RW; i += 256) {
    const int row = i / CO_RW, col = i - row * CO_RW;
    const float *zr = &z[row * CO_ZW + col + 5];
    double n = 0.0, d = 0.0;
#pragma unroll
    for (int k = -5; k <= 5; k++) {
      const float v = zr[k];
      const double g = A.g[k < 0 ? -k : k];
      if (v == v) {
        n = n + g * (double)v;
        d = d + g;
      }
    }
    rn[i] = n;
    rd[i] = d;
  }
  __syncthreads();
  // column sums at the fine rows fy0 - 1 .. fy0 + CO_FH: row `row` is staged row row + 5
  for (int i = (int)threadIdx.x; i < CO_SH * CO_RW; i += 256) {
    const int row = i / CO_RW, col = i - row * CO_RW;
    const float zc = z[(row + 5) * CO_ZW + col + 5];
    double v = NAN;
    if (zc == zc) {
      double n = 0.0, d = 0.0;
#pragma unroll
      for (int k = -5; k <= 5; k++) {
        const double g = A.g[k < 0 ? -k : k];
        n = n + g * rn[(row + 5 + k) * CO_RW + col];
        d = d + g * rd[(row + 5 + k) * CO_RW + col];
      }
      v = n / d;
    }
    sm[i] = v;
  }
  __syncthreads();
  const int ci = (int)threadIdx.x % CO_CX, cj = (int)threadIdx.x / CO_CX;
  const int I = tyi * CO_CY + cj, J = txi * CO_CX + ci;
  if (cj >= CO_CY || I >= Hc || J >= Wc) return;
  double sum_z = 0.0, sum_s = 0.0;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < 3; j++) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double *p = &sm[(1 + 3 * cj + j) * CO_RW + 1 + 3 * ci + i];
      const double v = *p;
      if (v == v) {
        sum_z = sum_z + v;
        sum_s = sum_s + mv_slope(p[-1], p[1], p[-CO_RW], p[CO_RW], v, A.c);
        cnt++;
      }
    }
  }
  const long long o = (long long)I * Wc + J;
  dem3[o] = cnt ? (float)(sum_z / (double)cnt) : DT_NODATA;
  slope3[o] = cnt ? (float)(sum_s / (double)cnt) : DT_NODATA;
}

int dt_launch_coarsen(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, const double *g6, float *dem3,
                      float *slope3) {
  DT_REQUIRE(g6, "the Gaussian weights are NULL");
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(dem && dem3 && slope3, "NULL raster");
  CoArgs A;
  for (int k = 0; k < 6; k++) A.g[k] = g6[k];
  A.c = px;
  const int64_t Hc = (H + 2) / 3, Wc = (W + 2) / 3;
  const int tiles_x = (int)((Wc + CO_CX - 1) / CO_CX);
  const unsigned nt = (unsigned)(((Hc + CO_CY - 1) / CO_CY) * tiles_x);
  hipLaunchKernelGGL(k_coarsen, dim3(nt), dim3(256), 0, s, dem, (int)H, (int)W, (int)Hc, (int)Wc, tiles_x, A, dem3,
                     slope3);
  return DT_OK;
}

// ---- the index -----------------------------------------------------------------------------------------------------
struct MvLevel {
  const float *slope, *lower, *higher;
  int h, w, s;  // the level's shape and 3^(L - 2)
  double t, p;  // t_L and p_L
};
struct MvArgs {
  MvDisc D2, D1;
  int levels;
  double c, t1, t2, p2, T[2];  // T: pctl_valley, pctl_ridge
  float *out[2];               // mrvbf, mrrtf
  MvLevel lev[DT_MRVBF_LEVELS_MAX - 2];
};

__device__ __forceinline__ double mv_n3(double x, double t) {
  const double q = x / t;
  return 1.0 / (1.0 + q * q * q);
}
__device__ __forceinline__ double mv_n4(double x, double t) {
  const double q = x / t, q2 = q * q;
  return 1.0 / (1.0 + q2 * q2);
}
__device__ __forceinline__ double mv_np(double x, double t, double p) { return 1.0 / (1.0 + pow(x / t, p)); }

// where base coordinate y falls on a level axis of n cells of s base cells each
struct MvAt {
  int i0, i1;
  double f;
};
__device__ __forceinline__ MvAt mv_at(int y, int n, int s) {
  // a = 2 y + 1 - s > -2 s: floor(a / (2 s)) of a negative a is -1, which is clamped; otherwise a fits 32 bits
  const unsigned u = 2u * (unsigned)y + 1u, s2 = 2u * (unsigned)s;
  MvAt at;
  at.i0 = 0;
  at.f = 0.0;
  if (u >= (unsigned)s) {
    const unsigned a = u - (unsigned)s, q = a / s2;
    if (q + 1u < (unsigned)n) {
      at.i0 = (int)q;
      at.f = (double)(a - q * s2) / (double)s2;
    } else {
      at.i0 = n - 1;
    }
  }
  at.i1 = at.i0 + 1 < n ? at.i0 + 1 : n - 1;
  return at;
}
__device__ __forceinline__ void mv_corner(const float *__restrict__ c, long long o, double w, double &acc, double &ws) {
  const float v = c[o];
  if (v != DT_NODATA) {
    acc = acc + w * (double)v;
    ws = ws + w;
  }
}
// (y, x) and s find the level's own cell, for a cell whose corners hold no value
__device__ __forceinline__ double mv_interp(const float *__restrict__ c, int wc, const MvAt &ay, const MvAt &ax, int y,
                                            int x, int s) {
  const double wy0 = 1.0 - ay.f, wx0 = 1.0 - ax.f;
  const long long r0 = (long long)ay.i0 * wc, r1 = (long long)ay.i1 * wc;
  double acc = 0.0, ws = 0.0;
  mv_corner(c, r0 + ax.i0, wy0 * wx0, acc, ws);
  mv_corner(c, r0 + ax.i1, wy0 * ax.f, acc, ws);
  mv_corner(c, r1 + ax.i0, ay.f * wx0, acc, ws);
  mv_corner(c, r1 + ax.i1, ay.f * ax.f, acc, ws);
  return ws == 0.0 ? (double)c[(long long)(y / s) * wc + x / s] : acc / ws;
}

__global__ __launch_bounds__(MV_NT) void k_mrvbf(const float *__restrict__ dem, int H, int W, int tiles_x, MvArgs A) {
  __shared__ float h[(MV_TY + 2 * MV_R2) * (MV_TX + 2 * MV_R2)];
  __shared__ uint2 cnt[MV_TY * MV_TX];
  constexpr int r = MV_R2, wt = MV_TX + 2 * r;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * MV_TX, y0 = tyi * MV_TY;
  mv_stage(h, dem, H, W, x0, y0, r);
  __syncthreads();
  const int lx = (int)threadIdx.x & (MV_TX - 1);
  const int ly0 = __builtin_amdgcn_readfirstlane((int)threadIdx.x / MV_TX) * MV_RB;
  const float *hc = &h[(ly0 + r) * wt + lx + r];
  float zc[MV_RB];
#pragma unroll
  for (int b = 0; b < MV_RB; b++) zc[b] = hc[b * wt];
  MvCount c2, c1;
  mv_counts<true>(hc, wt, A.D2, A.D1, zc, c2, c1);
  // the lane's counts go through LDS (three bytes per disc: at most 113 cells), so that the walk over the levels below
  // is one loop body with a run-time b and not MV_RB copies of it
#pragma unroll
  for (int b = 0; b < MV_RB; b++)
    cnt[(ly0 + b) * MV_TX + lx] = make_uint2((unsigned)(c1.n[b] | c1.l[b] << 8 | c1.h[b] << 16),
                                             (unsigned)(c2.n[b] | c2.l[b] << 8 | c2.h[b] << 16));
  const int gx = x0 + lx;
  if (gx >= W) return;
#pragma unroll 1
  for (int b = 0; b < MV_RB; b++) {
    const int gy = y0 + ly0 + b;
    if (gy >= H) break;
    const long long o = (long long)gy * W + gx;
    const float *q = hc + b * wt;
    const float z0 = *q;
    if (!(z0 == z0)) {
      if (A.out[0]) A.out[0][o] = DT_NODATA;
      if (A.out[1]) A.out[1][o] = DT_NODATA;
      continue;
    }
    const double S1 = mv_slope((double)q[-1], (double)q[1], (double)q[-wt], (double)q[wt], (double)z0, A.c);
    const double F1 = mv_n4(S1, A.t1);
    double cf = mv_n4(S1, A.t2);
    const uint2 pk = cnt[(ly0 + b) * MV_TX + lx];  // the lane's own store
    const double n1 = (double)(pk.x & 255u), n2 = (double)(pk.y & 255u);
    const unsigned cl1 = pk.x >> 8 & 255u, ch1 = pk.x >> 16, cl2 = pk.y >> 8 & 255u, ch2 = pk.y >> 16;
    double M[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (!A.out[k]) continue;
      const double P1 = (double)(k ? ch1 : cl1) / n1, P2 = (double)(k ? ch2 : cl2) / n2;
      const double VF1 = 1.0 - mv_n4(F1 * mv_n3(P1, A.T[k]), 0.3);
      const double VF2 = 1.0 - mv_n4(cf * mv_n3(P2, A.T[k]), 0.3);
      const double W2 = 1.0 - mv_np(VF2, 0.4, A.p2);
      M[k] = W2 * (1.0 + VF2) + (1.0 - W2) * VF1;
    }
    for (int L = 3; L <= A.levels; L++) {
      const MvLevel &V = A.lev[L - 3];
      const MvAt ay = mv_at(gy, V.h, V.s), ax = mv_at(gx, V.w, V.s);
      cf = cf * mv_n4(mv_interp(V.slope, V.w, ay, ax, gy, gx, V.s), V.t);
#pragma unroll
      for (int k = 0; k < 2; k++) {
        if (!A.out[k]) continue;
        const double P = mv_interp(k ? V.higher : V.lower, V.w, ay, ax, gy, gx, V.s);
        const double VF = 1.0 - mv_n4(cf * mv_n3(P, A.T[k]), 0.3);
        const double Wl = 1.0 - mv_np(VF, 0.4, V.p);
        M[k] = Wl * ((double)(L - 1) + VF) + (1.0 - Wl) * M[k];
      }
    }
    if (A.out[0]) A.out[0][o] = (float)M[0];
    if (A.out[1]) A.out[1][o] = (float)M[1];
  }
}

// the pyramid in scratch: per level 3 .. levels the float32 DEM, slope, lower and higher percentile
struct MvPyramid {
  float *dem[DT_MRVBF_LEVELS_MAX - 2], *slope[DT_MRVBF_LEVELS_MAX - 2], *lower[DT_MRVBF_LEVELS_MAX - 2],
      *higher[DT_MRVBF_LEVELS_MAX - 2];
  int64_t h[DT_MRVBF_LEVELS_MAX - 2], w[DT_MRVBF_LEVELS_MAX - 2];
  size_t bytes;
};
static MvPyramid mv_pyramid(int64_t H, int64_t W, int levels, void *scratch) {
  MvPyramid P = {};
  DtCarver c(scratch);
  for (int L = 3; L <= levels && L <= DT_MRVBF_LEVELS_MAX; L++) {
    H = (H + 2) / 3;
    W = (W + 2) / 3;
    const size_t n = (size_t)(H * W);
    P.h[L - 3] = H;
    P.w[L - 3] = W;
    P.dem[L - 3] = c.take<float>(n);
    P.slope[L - 3] = c.take<float>(n);
    P.lower[L - 3] = c.take<float>(n);
    P.higher[L - 3] = c.take<float>(n);
  }
  P.bytes = c.bytes();
  return P;
}
size_t dt_mrvbf_scratch(int64_t H, int64_t W, int levels) { return mv_pyramid(H, W, levels, nullptr).bytes; }

int dt_launch_mrvbf(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, double slope_threshold,
                    int levels, double pctl_valley, double pctl_ridge, const double *p, void *scratch,
                    size_t scratch_bytes, float *mrvbf, float *mrrtf) {
  DT_REQUIRE(levels >= 2 && levels <= DT_MRVBF_LEVELS_MAX, "levels must lie in [2, 10]");
  DT_REQUIRE(p, "the exponent table is NULL");
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(mrvbf || mrrtf, "no output raster");
  DT_REQUIRE(dem, "NULL raster");
  const MvPyramid P = mv_pyramid(H, W, levels, scratch);
  DT_REQUIRE(P.bytes == 0 || (scratch && scratch_bytes >= P.bytes), "scratch too small");
  double g[6];
  for (int k = 0; k < 6; k++) g[k] = exp(-(double)(k * k) / 18.0);
  MvArgs A = {};
  A.D2 = mv_disc(MV_R2);
  A.D1 = mv_disc(MV_R1);
  A.levels = levels;
  A.c = px;
  A.t1 = slope_threshold;
  A.t2 = slope_threshold / 2.0;
  A.p2 = p[0];
  A.T[0] = pctl_valley;
  A.T[1] = pctl_ridge;
  A.out[0] = mrvbf;
  A.out[1] = mrrtf;
  const float *fine = dem;
  int64_t fh = H, fw = W;
  double c = px;
  int s3 = 1;
  for (int L = 3; L <= levels; L++) {
    const int i = L - 3;
    DT_TRY(dt_launch_coarsen(s, fine, fh, fw, c, g, P.dem[i], P.slope[i]));
    DT_TRY(dt_launch_percentile(s, P.dem[i], P.h[i], P.w[i], MV_R2, mrvbf ? P.lower[i] : nullptr,
                                mrrtf ? P.higher[i] : nullptr));
    c = c * 3.0;
    s3 *= 3;
    fine = P.dem[i];
    fh = P.h[i];
    fw = P.w[i];
    MvLevel &V = A.lev[i];
    V.slope = P.slope[i];
    V.lower = P.lower[i];
    V.higher = P.higher[i];
    V.h = (int)fh;
    V.w = (int)fw;
    V.s = s3;
    V.t = slope_threshold / (double)(1 << (L - 1));
    V.p = p[L - 2];
  }
  const int tiles_x = (int)((W + MV_TX - 1) / MV_TX);
  const unsigned nt = (unsigned)(((H + MV_TY - 1) / MV_TY) * tiles_x);
  hipLaunchKernelGGL(k_mrvbf, dim3(nt), dim3(MV_NT), 0, s, dem, (int)H, (int)W, tiles_x, A);
  return DT_OK;
}
