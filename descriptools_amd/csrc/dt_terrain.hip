// dt_terrain.hip -- local terrain attributes: gradient, aspect, five curvatures and hillshade of the quadratic fitted by
// least squares over a (2 radius + 1)^2 window (Evans 1980; Wood 1996; net-new, descriptools_amd/terrain.py holds the
// definition).
//
// The fit is separable: a column pass sums the float32 heights of a window column into three float64 moments (C0, C1,
// C2), a row pass sums those along the row into six (M00, M10, M20, M01, M11, M02), and the five derivatives of the
// quadratic at the centre are quotients of them.  Every sum runs from its first term in ascending offset, one
// multiplication by the offset's integer factor before each addition, so a value is the numpy reference's bit for bit
// (the library is built with -ffp-contract=off -fno-fast-math); a sliding update would be O(1) per cell and another
// association.  Window completeness travels with the sums: a height that is not valid, or lies outside the raster, is
// staged as NaN, and M00 is NaN exactly when the window is not complete (valid float32 heights cannot overflow a
// float64 sum of 4,225 terms).
//
// k_terrain1  radius 1, on D-infinity's 128 x 8 staging tile with its one-cell halo: a lane takes four cells, computes
//             the column moments of its six staged columns once and stores 16 bytes per output where di_vec_ok allows.
// k_terrain   radius >= 2, one fused launch: a workgroup stages the heights of its TX x TY tile with a halo of `radius`
//             cells as float32, leaves the column moments of the tile's rows (TX + 2 radius columns) in LDS as float64,
//             and takes the row pass from there.  Nothing goes through global memory between the passes; the price is
//             the column pass of the 2 radius halo columns, done again by the neighbouring tile.
// CURV = false is the variant for calls without a curvature output: no C2, M20, M11, M02.
#include <cmath>

#include "dt_dinf_common.h"

enum { TR_GRADIENT, TR_ASPECT, TR_PROFILE, TR_PLAN, TR_TANGENTIAL, TR_MEAN, TR_LAPLACIAN, TR_HILLSHADE };

struct TrArgs {
  double den1, den2, den3;  // n S2 h, S2^2 h^2, n D h^2
  double nf, s2f;           // n and S2 as float64
  double sx, sy, sz;        // the unit vector to the sun
  float *out[DT_TERRAIN_OUTPUTS];
};

// a staged height as a term of the sums: NaN unless it is valid
__device__ __forceinline__ float tr_height(float v) { return di_valid(v) ? v : NAN; }

// the term of row offset j of a column's moments
template <bool CURV, bool FIRST>
__device__ __forceinline__ void tr_col_term(double z, int j, double (&C)[3]) {
  const double t1 = (double)(-j) * z;
  if (FIRST) {
    C[0] = z;
    C[1] = t1;
  } else {
    C[0] += z;
    C[1] += t1;
  }
  if (CURV) {
    const double t2 = (double)(j * j) * z;
    if (FIRST)
      C[2] = t2;
    else
      C[2] += t2;
  }
}
// the term of column offset i of a cell's moments M00, M10, M01, M20, M11, M02 from that column's C0, C1, C2
template <bool CURV, bool FIRST>
__device__ __forceinline__ void tr_row_term(double c0, double c1, double c2, int i, double (&M)[6]) {
  const double fi = (double)i;
  const double t10 = fi * c0;
  if (FIRST) {
    M[0] = c0;
    M[1] = t10;
    M[2] = c1;
  } else {
    M[0] += c0;
    M[1] += t10;
    M[2] += c1;
  }
  if (CURV) {
    const double t20 = (double)(i * i) * c0, t11 = fi * c1;
    if (FIRST) {
      M[3] = t20;
      M[4] = t11;
      M[5] = c2;
    } else {
      M[3] += t20;
      M[4] += t11;
      M[5] += c2;
    }
  }
}

// one cell from its moments: v[o] for every output asked for (the others are left alone)
template <bool CURV>
__device__ __forceinline__ void tr_cell(const TrArgs &A, const double (&M)[6], float (&v)[DT_TERRAIN_OUTPUTS]) {
  if (M[0] != M[0]) {  // the window is not complete
#pragma unroll
    for (int o = 0; o < DT_TERRAIN_OUTPUTS; o++) v[o] = DT_NODATA;
    return;
  }
  const double p = M[1] / A.den1, q = M[2] / A.den1;
  const double pp = p * p, qq = q * q;
  const double w = pp + qq, g1 = 1.0 + w;
  const bool flat = w == 0.0;
  if (A.out[TR_GRADIENT]) v[TR_GRADIENT] = (float)sqrt(w);
  if (A.out[TR_ASPECT]) {
    float a32 = -1.0f;
    if (!flat) {
      double a = atan2(-p, -q) * 57.29577951308232;
      if (a < 0.0) a += 360.0;
      a32 = (float)a;
      if (a32 >= 360.0f) a32 = 0.0f;
    }
    v[TR_ASPECT] = a32;
  }
  if (A.out[TR_HILLSHADE]) {
    const double hs = ((A.sz - p * A.sx) - q * A.sy) / sqrt(g1);
    v[TR_HILLSHADE] = hs > 0.0 ? (float)hs : 0.0f;
  }
  if (CURV) {
    const double s = M[4] / A.den2;
    const double r = 2.0 * ((A.nf * M[3] - A.s2f * M[0]) / A.den3);
    const double t = 2.0 * ((A.nf * M[5] - A.s2f * M[0]) / A.den3);
    const double pq2 = 2.0 * (p * q);
    const double sg1 = sqrt(g1);
    if (A.out[TR_PROFILE])
      v[TR_PROFILE] = flat ? 0.0f : (float)(-((pp * r + pq2 * s) + qq * t) / (w * (g1 * sg1)));
    if (A.out[TR_PLAN] || A.out[TR_TANGENTIAL]) {
      const double num = -((qq * r - pq2 * s) + pp * t);
      if (A.out[TR_PLAN]) v[TR_PLAN] = flat ? 0.0f : (float)(num / (w * sqrt(w)));
      if (A.out[TR_TANGENTIAL]) v[TR_TANGENTIAL] = flat ? 0.0f : (float)(num / (w * sg1));
    }
    if (A.out[TR_MEAN])
      v[TR_MEAN] = (float)(-(((1.0 + qq) * r - pq2 * s) + (1.0 + pp) * t) / (2.0 * (g1 * sg1)));
    if (A.out[TR_LAPLACIAN]) v[TR_LAPLACIAN] = (float)(r + t);
  }
}

// ---- radius 1 ------------------------------------------------------------------------------------------------------
template <bool CURV>
__global__ __launch_bounds__(256) void k_terrain1(const float *__restrict__ dem, int H, int W, int tiles_x, int vec_ok,
                                                  TrArgs A) {
  __shared__ __attribute__((aligned(16))) float t[(DI_TY + 2) * DI_LDW];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * DI_TX, y0 = tyi * DI_TY;
  di_stage(t, dem, H, W, x0, y0, vec_ok, NAN);
  __syncthreads();
  const int cx = ((int)threadIdx.x & 31) * 4, ly = (int)threadIdx.x >> 5;
  const int gy = y0 + ly, gx = x0 + cx;
  if (gy >= H || gx >= W) return;
  float a[6], b[6], c[6];
  di_load_row(t, ly, cx, a);
  di_load_row(t, ly + 1, cx, b);
  di_load_row(t, ly + 2, cx, c);
  double C[6][3];  // the column moments of the six staged columns, shared by the lane's four cells
#pragma unroll
  for (int m = 0; m < 6; m++) {
    tr_col_term<CURV, true>((double)tr_height(a[m]), -1, C[m]);
    tr_col_term<CURV, false>((double)tr_height(b[m]), 0, C[m]);
    tr_col_term<CURV, false>((double)tr_height(c[m]), 1, C[m]);
  }
  float v[4][DT_TERRAIN_OUTPUTS];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double M[6];
    tr_row_term<CURV, true>(C[k][0], C[k][1], C[k][2], -1, M);
    tr_row_term<CURV, false>(C[k + 1][0], C[k + 1][1], C[k + 1][2], 0, M);
    tr_row_term<CURV, false>(C[k + 2][0], C[k + 2][1], C[k + 2][2], 1, M);
    tr_cell<CURV>(A, M, v[k]);
  }
  const long long o = (long long)gy * W + gx;
  const bool full = vec_ok && gx + 3 < W;
#pragma unroll
  for (int n = 0; n < DT_TERRAIN_OUTPUTS; n++) {
    if (!CURV && n >= TR_PROFILE && n <= TR_LAPLACIAN) continue;
    float *dst = A.out[n];
    if (!dst) continue;
    if (full) {
      *reinterpret_cast<float4 *>(dst + o) = make_float4(v[0][n], v[1][n], v[2][n], v[3][n]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (gx + k < W) dst[o + k] = v[k][n];
    }
  }
}

// ---- radius >= 2 ---------------------------------------------------------------------------------------------------
// The tile is TX x TY cells, RMAX the largest radius the instantiation has LDS for.  wt = TX + 2 r is the width of
// both LDS planes: the heights hold TY + 2 r rows of it, each moment plane TY.
template <int TX, int TY, int RMAX, bool CURV>
__global__ __launch_bounds__(256) void k_terrain(const float *__restrict__ dem, int H, int W, int tiles_x, int r,
                                                 TrArgs A) {
  constexpr int NM = CURV ? 3 : 2;
  constexpr int WMAX = TX + 2 * RMAX;
  __shared__ float h[(TY + 2 * RMAX) * WMAX];
  __shared__ double cm[NM * TY * WMAX];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * TX, y0 = tyi * TY;
  const int wt = TX + 2 * r, ht = TY + 2 * r;
  for (int i = (int)threadIdx.x; i < ht * wt; i += 256) {
    const int row = i / wt, col = i - row * wt;
    const int gy = y0 - r + row, gx = x0 - r + col;
    float v = NAN;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = tr_height(dem[(long long)gy * W + gx]);
    h[i] = v;
  }
  __syncthreads();
  // column pass: the moments of column `col` over the rows ly - r .. ly + r of the tile's row ly
  for (int i = (int)threadIdx.x; i < TY * wt; i += 256) {
    const float *hp = &h[i];  // row ly of the staged block is the window's first row
    double C[3];
    tr_col_term<CURV, true>((double)hp[0], -r, C);
    for (int j = 1 - r; j <= r; j++) tr_col_term<CURV, false>((double)hp[(j + r) * wt], j, C);
    cm[i] = C[0];
    cm[TY * wt + i] = C[1];
    if (CURV) cm[2 * TY * wt + i] = C[2];
  }
  __syncthreads();
  // row pass: the moments of cell (ly, lx) over the columns lx .. lx + 2 r of the moment planes
  for (int i = (int)threadIdx.x; i < TX * TY; i += 256) {
    const int ly = i / TX, lx = i - ly * TX;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const double *c0 = &cm[ly * wt + lx], *c1 = c0 + TY * wt, *c2 = c0 + (CURV ? 2 * TY * wt : 0);
    double M[6];
    tr_row_term<CURV, true>(c0[0], c1[0], c2[0], -r, M);
    for (int k = 1; k <= 2 * r; k++) tr_row_term<CURV, false>(c0[k], c1[k], c2[k], k - r, M);
    float v[DT_TERRAIN_OUTPUTS];
    tr_cell<CURV>(A, M, v);
    const long long o = (long long)gy * W + gx;
#pragma unroll
    for (int n = 0; n < DT_TERRAIN_OUTPUTS; n++) {
      if (!CURV && n >= TR_PROFILE && n <= TR_LAPLACIAN) continue;
      if (A.out[n]) A.out[n][o] = v[n];
    }
  }
}

template <int TX, int TY, int RMAX>
static void tr_launch(hipStream_t s, bool curv, const float *dem, int64_t H, int64_t W, int r, const TrArgs &A) {
  static_assert(sizeof(float) * (TY + 2 * RMAX) * (TX + 2 * RMAX) + sizeof(double) * 3 * TY * (TX + 2 * RMAX) <= 65536,
                "static LDS of a workgroup");
  const int tiles_x = (int)((W + TX - 1) / TX);
  const unsigned nt = (unsigned)(((H + TY - 1) / TY) * tiles_x);
  auto *k = curv ? k_terrain<TX, TY, RMAX, true> : k_terrain<TX, TY, RMAX, false>;
  hipLaunchKernelGGL(k, dim3(nt), dim3(256), 0, s, dem, (int)H, (int)W, tiles_x, r, A);
}

int dt_launch_terrain(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, int radius, double sx,
                      double sy, double sz, float *const out[DT_TERRAIN_OUTPUTS]) {
  DT_REQUIRE(radius >= 1 && radius <= DT_TERRAIN_RADIUS_MAX, "radius must lie in [1, 32]");
  if (H == 0 || W == 0) return DT_OK;
  // S2 = sum of i^2, S4 = sum of i^4 over -r .. r; D = n S4 - S2^2: integers, exact in float64 for r <= 32
  const int64_t r = radius, n = 2 * r + 1;
  const int64_t S2 = r * (r + 1) * (2 * r + 1) / 3;
  const int64_t S4 = r * (r + 1) * (2 * r + 1) * (3 * r * r + 3 * r - 1) / 15;
  const int64_t D = n * S4 - S2 * S2;
  TrArgs A;
  A.den1 = (double)(n * S2) * px;
  A.den2 = (double)(S2 * S2) * (px * px);
  A.den3 = (double)(n * D) * (px * px);
  A.nf = (double)n;
  A.s2f = (double)S2;
  A.sx = sx;
  A.sy = sy;
  A.sz = sz;
  bool curv = false, any = false;
  int vec_ok = di_vec_ok(dem, W);
  for (int o = 0; o < DT_TERRAIN_OUTPUTS; o++) {
    A.out[o] = out[o];
    if (!out[o]) continue;
    any = true;
    curv = curv || (o >= TR_PROFILE && o <= TR_LAPLACIAN);
    vec_ok = vec_ok && di_vec_ok(out[o], W);
  }
  DT_REQUIRE(any, "no output raster");
  if (radius == 1) {
    int tiles_x;
    const unsigned nt = di_tiles(H, W, tiles_x);
    auto *k = curv ? k_terrain1<true> : k_terrain1<false>;
    hipLaunchKernelGGL(k, dim3(nt), dim3(256), 0, s, dem, (int)H, (int)W, tiles_x, vec_ok, A);
  } else if (radius <= 4) {
    tr_launch<64, 16, 4>(s, curv, dem, H, W, radius, A);
  } else if (radius <= 12) {
    tr_launch<64, 16, 12>(s, curv, dem, H, W, radius, A);
  } else if (radius <= 20) {
    tr_launch<64, 16, 20>(s, curv, dem, H, W, radius, A);
  } else {
    tr_launch<64, 8, 32>(s, curv, dem, H, W, radius, A);
  }
  return DT_OK;
}
