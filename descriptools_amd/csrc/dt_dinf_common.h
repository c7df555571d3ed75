// dt_dinf_common.h -- what the kernels on D-infinity's tile geometry share (dt_dinf.hip: direction and contributing
// area; dt_dinf_dist.hip: distance to the stream; dt_mfd.hip: MFD shares and contributing area; dt_terrain.hip: the
// radius-1 terrain attributes): the 128 x 8 staging
// tile with its one-cell halo and its launch geometry, the octant steps, the validity of a height, the D8 codes of a
// lane's four cells and the decoding of an angle into receivers (descriptools_amd/dinf.py holds the definition).
#pragma once
#include <cmath>

#include "dt_kernels.h"

#define DI_TX 128
#define DI_TY 8
#define DI_LDW (DI_TX + 8)  // LDS row stride in floats; the interior starts at column 4
#define DI_PI 3.141592653589793
#define DI_4_OVER_PI 1.2732395447351628  // the float64 nearest 4 / pi
#define DI_F2PI 6.2831854820251465f      // float32(2 pi)

// dy / dx of octant k (angle k pi / 4 counter-clockwise from east, rows grow to the south), packed as DT_PK8 packs
#define DI_DX_PACK DT_PK8(1, 1, 0, -1, -1, -1, 0, 1)
#define DI_DY_PACK DT_PK8(0, -1, -1, -1, 0, 1, 1, 1)

// finite and > -100 (false for NaN)
__device__ __forceinline__ bool di_valid(float v) { return v > -100.0f && v < INFINITY; }

// the tiles of an H x W raster: one workgroup each
static inline unsigned di_tiles(int64_t H, int64_t W, int &tiles_x) {
  tiles_x = (int)((W + DI_TX - 1) / DI_TX);
  return (unsigned)(((H + DI_TY - 1) / DI_TY) * tiles_x);
}
// a float raster of width W at p may be read and written four cells (16 bytes) at a time
static inline int di_vec_ok(const void *p, int64_t W) { return W % 4 == 0 && ((uintptr_t)p & 15u) == 0; }

// the D8 codes of the lane's four cells from gx on (flat index o), one per byte; 0 without `fdr` and beyond the row.
// full: the four lie in the row and fdr + o is 4-byte aligned
__device__ __forceinline__ uint32_t di_load_codes(const uint8_t *__restrict__ fdr, long long o, int gx, int W,
                                                  bool full) {
  uint32_t codes = 0u;
  if (fdr) {
    if (full) {
      codes = *reinterpret_cast<const uint32_t *>(fdr + o);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (gx + k < W) codes |= (uint32_t)fdr[o + k] << (8 * k);
    }
  }
  return codes;
}

// stage (DI_TY + 2) x (DI_TX + 2) cells of src around the tile at (y0, x0); `fill` outside the raster.  The caller
// synchronises.
__device__ __forceinline__ void di_stage(float *t, const float *__restrict__ src, int H, int W, int x0, int y0,
                                         int vec_ok, float fill) {
#pragma unroll
  for (int u = 0; u < 2; u++) {
    const int i = (int)threadIdx.x + 256 * u;
    if (i < (DI_TY + 2) * (DI_TX / 4)) {
      const int r = i / (DI_TX / 4), c4 = i - r * (DI_TX / 4);
      const int gy = y0 - 1 + r, gx = x0 + c4 * 4;
      float4 v = make_float4(fill, fill, fill, fill);
      if (gy >= 0 && gy < H) {
        const float *p = src + (long long)gy * W + gx;
        if (vec_ok && gx + 3 < W) {
          v = *reinterpret_cast<const float4 *>(p);
        } else {
          if (gx < W) v.x = p[0];
          if (gx + 1 < W) v.y = p[1];
          if (gx + 2 < W) v.z = p[2];
          if (gx + 3 < W) v.w = p[3];
        }
      }
      *reinterpret_cast<float4 *>(&t[r * DI_LDW + 4 + c4 * 4]) = v;
    }
  }
  if (threadIdx.x < (DI_TY + 2) * 2) {
    const int r = (int)threadIdx.x >> 1, side = (int)threadIdx.x & 1;
    const int gy = y0 - 1 + r, gx = side ? x0 + DI_TX : x0 - 1;
    float v = fill;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = src[(long long)gy * W + gx];
    t[r * DI_LDW + (side ? 4 + DI_TX : 3)] = v;
  }
}

// the eight neighbours of the lane's cell k (0..3) by octant, from its three rows of six staged values
__device__ __forceinline__ void di_octants(const float (&a)[6], const float (&b)[6], const float (&c)[6], int k,
                                           float (&n)[8]) {
  n[0] = b[k + 2];
  n[1] = a[k + 2];
  n[2] = a[k + 1];
  n[3] = a[k];
  n[4] = b[k];
  n[5] = c[k];
  n[6] = c[k + 1];
  n[7] = c[k + 2];
}

__device__ __forceinline__ void di_load_row(const float *t, int lr, int cx, float (&dst)[6]) {
  const float *row = &t[lr * DI_LDW];
  const float4 m = *reinterpret_cast<const float4 *>(row + 4 + cx);
  dst[0] = row[3 + cx];
  dst[1] = m.x;
  dst[2] = m.y;
  dst[3] = m.z;
  dst[4] = m.w;
  dst[5] = row[8 + cx];
}

// an angle as receivers: kind 0 none (-1, nodata, or a value outside the contract: bad), 1 one receiver (octant k),
// 2 two (octant k with share 2^30 - p2, octant k + 1 with share p2)
struct DiDec {
  int kind, k;
  uint32_t p2;
};
__device__ __forceinline__ DiDec di_decode(float a, bool &bad) {
  DiDec d = {0, 0, 0u};
  if (a == -1.0f || a == DT_NODATA) return d;
  if (!(a >= 0.0f && a <= DI_F2PI)) {  // NaN, another negative, beyond float32(2 pi)
    bad = true;
    return d;
  }
  const double t = (double)a * DI_4_OVER_PI;
  const double rt = rint(t);
  if (fabs(t - rt) <= 0x1p-20) {
    d.kind = 1;
    d.k = (int)rt & 7;
  } else {
    const double fl = floor(t);
    d.kind = 2;
    d.k = (int)fl & 7;
    d.p2 = (uint32_t)rint((t - fl) * 0x1p30);
  }
  return d;
}
