// dt_stencil.hip -- 3x3 stencil kernels: slope (S3), D8 (N1), radians, fused slope + TI + MTI (T2, T3).
// Reference citations are file:line relative to /root/reference/descriptools/.
#include <math.h>

#include "dt_common.h"
#include "dt_kernels.h"
#include "dt_math.h"

// ===========================================================================================
// 3x3 stencil: slope (S3, slope.py:210-259) + D8 (N1) + radians + optional fused TI/MTI.
//
// Tile = 256 columns x 16 rows per 256-thread workgroup, staged (with a 1-cell halo) through
// LDS by coalesced 16-byte row loads; thread (tx, ty) then owns a 4-wide x 4-tall patch and
// reads its 6 x 6 neighbourhood as one ds_read_b128 + two ds_read_b32 per row.  Stores are
// float4 / uchar4 per row (1 KiB / 256 B contiguous per wave).  Workgroup ids are remapped so
// that each XCD (ids congruent mod 8 share one) sweeps its own horizontal band of the raster
// top to bottom: the halo rows shared by vertically adjacent tiles are then re-read from that
// XCD's L2 instead of HBM.
//
// Exactness: the reference compares float64 quotients (z_c - z_nb)/d in scan order
// NW,N,NE,W,E,SW,S,SE with strict '<'.  Division by a positive constant is monotone and
// injective on float32 differences, so the maximum over the 4 cardinal (4 diagonal)
// neighbours is taken on the float32 differences and only the two class maxima are divided
// in float64 -- bit-identical results with 2 instead of 8 float64 divisions per cell.
// ===========================================================================================
#define SD_TX 256
#define SD_TY 16
#define SD_LDW (SD_TX + 8)  // LDS row stride in floats; interior starts at column 4

struct SlopeCell {
  float slope;
  uint8_t code;
};

// scan positions: NW0 N1 NE2 W3 E4 SW5 S6 SE7.  NEED_CODE = false (slope only): the D8 bookkeeping
// (which neighbour, scan position for ties) is skipped -- the slope value does not depend on it.
// scan position (NW 0, N 1, NE 2, W 3, E 4, SW 5, S 6, SE 7; 8 = none) of a D8 code
__device__ __forceinline__ int dt_scan_pos(uint32_t code) {
  if (code == 0u) return 8;
  // bit index of the code 0..7 = E SE S SW W NW N NE -> position 4 7 6 5 3 0 1 2
  return (int)((0x21035674u >> (4 * (__ffs((int)code) - 1))) & 0xFu);
}

// Neighbour heights arrive with nodata (== -100) replaced by a NaN of a fixed payload (sd_nod, done once per cell
// when the tile is staged): c - NaN = NaN never beats a candidate, which is the reference's "neighbour == -100
// skipped" (slope.py:247) without a test per neighbour; a real NaN or +inf neighbour drops out the same way, as it
// does in the reference.  `c` is the centre's original value.
template <bool NEED_CODE, bool NEED_SLOPE>
__device__ __forceinline__ SlopeCell dt_slope_cell(float c, float nw, float n, float ne, float w,
                                                  float e, float sw, float s, float se,
                                                  double inv_card, double inv_diag, double dcard,
                                                  double ddiag) {
  SlopeCell r;
  if (c <= DT_NODATA) {  // slope.py:231
    r.slope = DT_NODATA;
    r.code = 0;
    return r;
  }
  // cardinals in scan order N, W, E, S, then the diagonals NW, NE, SW, SE; strict > keeps the first maximum
  float cb = 0.0f, db = 0.0f;
  uint32_t ccode = 0, dcode = 0;
  if (NEED_CODE) {
#define DT_CAND(nb, best, bcode, code_) \
  {                                     \
    float d_ = c - (nb);                \
    if (d_ > best) {                    \
      best = d_;                        \
      bcode = code_;                    \
    }                                   \
  }
    DT_CAND(n, cb, ccode, 64u)
    DT_CAND(w, cb, ccode, 16u)
    DT_CAND(e, cb, ccode, 1u)
    DT_CAND(s, cb, ccode, 4u)
    DT_CAND(nw, db, dcode, 32u)
    DT_CAND(ne, db, dcode, 128u)
    DT_CAND(sw, db, dcode, 8u)
    DT_CAND(se, db, dcode, 2u)
#undef DT_CAND
  } else {
    cb = fmaxf(fmaxf(fmaxf(c - n, c - w), fmaxf(c - e, c - s)), 0.0f);
    db = fmaxf(fmaxf(fmaxf(c - nw, c - ne), fmaxf(c - sw, c - se)), 0.0f);
  }
  // Exact float64 divisions are ~15 instructions each.  Fast path: multiply by the (correctly rounded)
  // reciprocals -- within 3 float64 ulp of the reference's quotient -- and accept the result only if
  // neither the cardinal / diagonal comparison nor (when the slope is wanted) the final float32 rounding
  // can be affected by those ulps; otherwise divide.  Results are bit-identical either way.
  double vc = (double)cb * inv_card, vd = (double)db * inv_diag;
  const double EPS = 8.9e-16;  // 4 ulp, relative
  double vmax = vc > vd ? vc : vd;
  bool ambiguous = (vc != vd) && fabs(vc - vd) <= EPS * vmax;
  if (NEED_SLOPE) {
    float f_lo = (float)(vmax * (100.0 * (1.0 - EPS))), f_hi = (float)(vmax * (100.0 * (1.0 + EPS)));
    ambiguous = ambiguous || (f_lo != f_hi);
  }
  if (ambiguous) {
    vc = cb > 0.0f ? (double)cb / dcard : 0.0;
    vd = db > 0.0f ? (double)db / ddiag : 0.0;
  }
  double v;
  uint32_t code;
  // equal quotients: the candidate met first in scan order wins (positions looked up only then)
  if (vc > vd || (vc == vd && dt_scan_pos(ccode) < dt_scan_pos(dcode))) {
    v = vc;
    code = ccode;
  } else {
    v = vd;
    code = dcode;
  }
  r.slope = (float)(v * 100.0);  // slope.py:259
  r.code = (uint8_t)code;
  return r;
}

// XCD-aware tile mapping: workgroup id b runs on XCD group (b % 8); give each group a band of tile rows
// and walk it row-major -- each group starting an eighth of a band further in than the previous one (and
// wrapping), so that the eight write fronts are not exactly one band apart in memory: 1-1.5 % on the fused
// stencil on every placement tried (tools/placement_probe5.py; identity and row-interleaved maps: slower).
__device__ __forceinline__ int sd_tile_of_block(int b, int ntiles) {
  int xcd = b & 7, j = b >> 3;
  int q = ntiles >> 3, rem = ntiles & 7;
  int base = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
  int n = q + (xcd < rem ? 1 : 0);  // tiles of this band (j < n)
  int k = j + xcd * (n >> 3);
  return base + (k >= n ? k - n : k);
}

__device__ __forceinline__ void sd_tile_origin(int b, int tiles_x, int tiles_y, int &x0, int &y0) {
  int tile = sd_tile_of_block(b, tiles_x * tiles_y);
  int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  x0 = txi * SD_TX;
  y0 = tyi * SD_TY;
}

// The staged stand-in for nodata: a quiet NaN with a payload no arithmetic produces (hardware NaNs are 0x7FC00000),
// told apart from a real NaN or +inf height by its bits -- so that a NaN centre keeps the reference's answer (slope
// 0, the border out-code) and a +inf centre its own (slope inf and a code) instead of passing for nodata.
#define SD_NOD_BITS 0x7FC0D0DAu
__device__ __forceinline__ float sd_nod() { return __uint_as_float(SD_NOD_BITS); }
__device__ __forceinline__ float sd_stage_val(float v) { return v == DT_NODATA ? sd_nod() : v; }
// the centre's own value (-100 for staged nodata)
__device__ __forceinline__ float sd_centre(float v) { return __float_as_uint(v) == SD_NOD_BITS ? DT_NODATA : v; }

// stage (SD_TY + 2) x (SD_TX + 2) cells; outside the GLOBAL raster = -100 ring (slope.py:175); cells outside
// the core but inside the global raster come from the halo of the window.  nodata (and everything outside
// the raster) is staged as sd_nod(): see dt_slope_cell.  The caller synchronises.
__device__ __forceinline__ void sd_stage(float *t, const float *__restrict__ dem, const DtWin &w, int x0, int y0,
                                         int vec_ok) {
  const int H = w.H, W = w.W;
  const int ylo = -(w.gy0 > 0 ? 1 : 0), yhi = H + (w.gy0 + H < w.Hg ? 1 : 0);  // readable rows [ylo, yhi)
  const int xlo = -(w.gx0 > 0 ? 1 : 0), xhi = W + (w.gx0 + W < w.Wg ? 1 : 0);
  // Block-uniform fast form for tiles whose whole 18 x 258 window is readable: every load of a thread is issued
  // before the first use (five 16-byte loads and one halo value in flight per thread).  The guarded loop below
  // waits for each load before the next: five dependent memory round trips per workgroup, which made every
  // stencil kernel latency-bound (the D8-only kernel took as long as the 8 B/cell slope kernel).
  if (vec_ok && y0 - 1 >= ylo && y0 + SD_TY + 1 <= yhi && x0 - 1 >= xlo && x0 + SD_TX + 1 <= xhi) {
    constexpr int NV = ((SD_TY + 2) * (SD_TX / 4) + 255) / 256;  // 5
    float4 v[NV];
    const float *base = dem + (long long)(y0 - 1) * w.ld + x0;
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int i = threadIdx.x + 256 * u;
      if (i < (SD_TY + 2) * (SD_TX / 4)) {
        const int r = i / (SD_TX / 4), c4 = i - r * (SD_TX / 4);
        v[u] = *reinterpret_cast<const float4 *>(base + (long long)r * w.ld + c4 * 4);
      }
    }
    float hv = 0.0f;
    const int hr = threadIdx.x >> 1, hside = threadIdx.x & 1;
    if (threadIdx.x < (SD_TY + 2) * 2) hv = base[(long long)hr * w.ld + (hside ? SD_TX : -1)];
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int i = threadIdx.x + 256 * u;
      if (i < (SD_TY + 2) * (SD_TX / 4)) {
        const int r = i / (SD_TX / 4), c4 = i - r * (SD_TX / 4);
        float4 q = v[u];
        q.x = sd_stage_val(q.x);
        q.y = sd_stage_val(q.y);
        q.z = sd_stage_val(q.z);
        q.w = sd_stage_val(q.w);
        *reinterpret_cast<float4 *>(&t[r * SD_LDW + 4 + c4 * 4]) = q;
      }
    }
    if (threadIdx.x < (SD_TY + 2) * 2) t[hr * SD_LDW + (hside ? 4 + SD_TX : 3)] = sd_stage_val(hv);
    return;
  }
  for (int i = threadIdx.x; i < (SD_TY + 2) * (SD_TX / 4); i += 256) {
    int r = i / (SD_TX / 4), c4 = i - r * (SD_TX / 4);
    int gy = y0 - 1 + r, gx = x0 + c4 * 4;
    float4 v = make_float4(DT_NODATA, DT_NODATA, DT_NODATA, DT_NODATA);
    if (gy >= ylo && gy < yhi) {
      const float *p = dem + (long long)gy * w.ld + gx;
      if (vec_ok && gx + 3 < xhi) {
        v = *reinterpret_cast<const float4 *>(p);
      } else {
        if (gx < xhi) v.x = p[0];
        if (gx + 1 < xhi) v.y = p[1];
        if (gx + 2 < xhi) v.z = p[2];
        if (gx + 3 < xhi) v.w = p[3];
      }
    }
    v.x = sd_stage_val(v.x);
    v.y = sd_stage_val(v.y);
    v.z = sd_stage_val(v.z);
    v.w = sd_stage_val(v.w);
    *reinterpret_cast<float4 *>(&t[r * SD_LDW + 4 + c4 * 4]) = v;
  }
  for (int i = threadIdx.x; i < (SD_TY + 2) * 2; i += 256) {
    int r = i >> 1, side = i & 1;
    int gy = y0 - 1 + r, gx = side ? x0 + SD_TX : x0 - 1;
    float v = DT_NODATA;
    if (gy >= ylo && gy < yhi && gx >= xlo && gx < xhi) v = dem[(long long)gy * w.ld + gx];
    t[r * SD_LDW + (side ? 4 + SD_TX : 3)] = sd_stage_val(v);
  }
}

template <bool W_SLOPE, bool W_FDR, bool W_RAD>
__global__ __launch_bounds__(256, 6) void k_stencil(const float *__restrict__ dem, DtWin w,
                                                double px, float *__restrict__ slope,
                                                uint8_t *__restrict__ fdr,
                                                float *__restrict__ slope_rad, int tiles_x, int tiles_y,
                                                int vec_ok) {
  __shared__ __attribute__((aligned(16))) float t[(SD_TY + 2) * SD_LDW];

  int x0, y0;
  sd_tile_origin(blockIdx.x, tiles_x, tiles_y, x0, y0);
  const int H = w.H, W = w.W;
  sd_stage(t, dem, w, x0, y0, vec_ok);
  __syncthreads();

  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int cx = tx * 4;  // tile column of the patch
  const int ry = ty * 4;  // tile row of the patch
  const int gx = x0 + cx;
  if (gx >= W) return;
  const double dcard = px, ddiag = px * sqrt(2.0);
  const double inv_card = 1.0 / dcard, inv_diag = 1.0 / ddiag;

  // rolling 3-row window of 6 values (cols cx-1 .. cx+4)
  float a[6], bb[6], cc[6];
  auto load_row = [&](int lr, float *dst) {
    const float *p = &t[lr * SD_LDW + 4 + cx];
    float4 m = *reinterpret_cast<const float4 *>(p);
    dst[0] = p[-1];
    dst[1] = m.x;
    dst[2] = m.y;
    dst[3] = m.z;
    dst[4] = m.w;
    dst[5] = p[4];
  };
  load_row(ry, a);       // row above the first output row (tile row ry == raster row y0-1+ry)
  load_row(ry + 1, bb);  // first output row
#pragma unroll
  for (int j = 0; j < 4; j++) {
    int gy = y0 + ry + j;
    load_row(ry + 2 + j, cc);
    if (gy < H) {
      float so[4], ro[4];
      uint32_t codes = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float cz = sd_centre(bb[k + 1]);  // the centre's own value
        SlopeCell sc = dt_slope_cell<W_FDR, (W_SLOPE || W_RAD)>(cz, a[k], a[k + 1], a[k + 2], bb[k],
                                                                       bb[k + 2], cc[k], cc[k + 1], cc[k + 2],
                                                                       inv_card, inv_diag, dcard, ddiag);
        so[k] = sc.slope;
        uint32_t code = sc.code;
        if (W_FDR) {
          // N1 border rule: a border cell with no lower neighbour drains out of the raster
          int gyy = w.gy0 + gy, gxx = w.gx0 + gx + k;  // global position
          if (code == 0u && !(cz <= DT_NODATA)) {  // (a NaN centre drains out as well)
            if (gyy == w.Hg - 1) code = 4u;
            else if (gyy == 0) code = 64u;
            else if (gxx == 0) code = 16u;
            else if (gxx == w.Wg - 1) code = 1u;
          }
          codes |= code << (8 * k);
        }
        if (W_RAD) ro[k] = dt_slope_rad(sc.slope, cz);
      }
      long long o = (long long)gy * w.ld + gx;
      bool full = vec_ok && gx + 3 < W;
      if (full) {
        if (W_SLOPE) *reinterpret_cast<float4 *>(slope + o) = make_float4(so[0], so[1], so[2], so[3]);
        if (W_RAD) *reinterpret_cast<float4 *>(slope_rad + o) = make_float4(ro[0], ro[1], ro[2], ro[3]);
        if (W_FDR) *reinterpret_cast<uint32_t *>(fdr + o) = codes;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (gx + k < W) {
            if (W_SLOPE) slope[o + k] = so[k];
            if (W_RAD) slope_rad[o + k] = ro[k];
            if (W_FDR) fdr[o + k] = (uint8_t)(codes >> (8 * k));
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
      a[q] = bb[q];
      bb[q] = cc[q];
    }
  }
}

// ===========================================================================================
// Fused slope + TI + MTI (+ radians), hot / cold split -- the north_star's "slope+TWI stencil".
//
// k_slope_twi is branch-free: every cell takes the product form of the slope and the float32 fast path
// of the logarithms (dt_math.h), and a cell whose result cannot be PROVEN identical to the literal
// float64 expression is only flagged (one bit per cell, 16 per lane):
//   slope   q = max(cb * kc, db * kd), kc = 100 / px, kd = 100 / (px sqrt 2), is within 2^-51 (relative) of
//           the reference's fl(fl(d / dist) * 100) whichever of the two classes wins, so float32(q) is the
//           reference's float32 unless q lies within SD_MID ulps of a float32 rounding boundary (bits 0-28
//           of the mantissa = 2^28), is not a normal float32, or the quotient / arctangent leave their
//           fast domain;
//   TI/MTI  fast-path domain and |result| >= DT_FAST_MIN, exactly the conditions of dt_twi_cell.
// A workgroup with a flagged cell marks its tile and writes the lanes' masks; k_slope_twi_fix, a few
// workgroups striding over the tile marks afterwards, recomputes those cells with the exact per-cell
// functions (dt_slope_cell / dt_slope_rad / dt_twi_cell: true float64 divisions, table logarithms,
// library fall-backs) and overwrites them.  ~1e-7 of the cells of a terrain raster are flagged.  The hot
// kernel has no slow-path code, no scratch, <= 64 VGPRs (8 waves per SIMD) and 19 KiB of LDS.
//
// The columns left and right of a lane's 4-wide patch are its neighbours' own registers: a lane's row is
// one ds_read_b128 plus two DPP wave shifts (lane 0 / 63 take the tile's halo columns from a
// wave-uniform LDS address), instead of two bank-conflicting ds_read_b32.
// ===========================================================================================
#define SD_MID 16u /* flag |low 29 mantissa bits - 2^28| <= SD_MID */
// The fix-up kernels read the tile marks 256 at a time; SD_FIX_SPLIT workgroups share the marked tiles of one such
// chunk.  (With one workgroup per chunk a raster whose tiles are ALL marked -- slopes beyond 250 %, TI / MTI near 0 on
// many cells: 15 % of the cells of a rough synthetic DEM with 40 m pits at 10 m pixels -- ran on one workgroup per CU.)
#define SD_FIX_SPLIT 8

// value of `v` in the previous / next lane of the wave; lane 0 / lane 63 keep `edge`
__device__ __forceinline__ float sd_from_prev_lane(float edge, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138 /* wave_shr:1 */,
                                                    0xF, 0xF, false));
}
__device__ __forceinline__ float sd_from_next_lane(float edge, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130 /* wave_shl:1 */,
                                                    0xF, 0xF, false));
}

// slope.py:210-259 in product form; returns true when the cell must be redone exactly
__device__ __forceinline__ bool sd_slope_fast(float c, float nw, float n, float ne, float w, float e, float sw,
                                              float s, float se, double kc, double kd, float &slope) {
  float cb = fmaxf(fmaxf(fmaxf(c - n, c - w), fmaxf(c - e, c - s)), 0.0f);
  float db = fmaxf(fmaxf(fmaxf(c - nw, c - ne), fmaxf(c - sw, c - se)), 0.0f);
  double qc = (double)cb * kc, qd = (double)db * kd;
  double q = qc > qd ? qc : qd;
  unsigned long long bits = (unsigned long long)__double_as_longlong(q);
  uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
  bool near_mid = ((lo & 0x1FFFFFFFu) - (0x10000000u - SD_MID)) <= 2u * SD_MID;
  bool odd = ((hi >> 20) - 897u) > 253u && bits != 0ull;  // not a normal float32 (and not 0): inf, NaN, tiny
  slope = (float)q;
  return near_mid || odd;
}

// (sd_twi_fast, the float32 fast path of TI / MTI from q = slope % / 100, lives in dt_math.h: flow accumulation's last
// tile pass evaluates it too, dt_tiles.hip k_fa3fh1_twi)
typedef float sd_v4f __attribute__((ext_vector_type(4)));
typedef int sd_v4i __attribute__((ext_vector_type(4)));
typedef long long sd_v2l __attribute__((ext_vector_type(2)));
// The fused stencil's streams are non-temporal, the loads of the accumulation raster and the stores of the outputs:
// each byte is touched once (0.86 instead of 0.92 ms at 16384^2).
__device__ __forceinline__ void sd_store4(float *p, float a, float b, float c, float d) {
  sd_v4f v = {a, b, c, d};
  __builtin_nontemporal_store(v, reinterpret_cast<sd_v4f *>(p));
}

// The tile is 256 x 16 cells: one 4 x 4 patch per lane, a wave = 256 columns x 4 rows.  AccT = width of the
// accumulation raster.
template <bool W_SLOPE, bool W_RAD, typename AccT>
__global__ __launch_bounds__(256, 8) void k_slope_twi(const float *__restrict__ dem, DtWin w, double kc, double kd,
                                                     float *__restrict__ slope, float *__restrict__ slope_rad,
                                                     const AccT *__restrict__ acc32, double n_top, double lnpx2,
                                                     float *__restrict__ ti, float *__restrict__ mti, int tiles_x,
                                                     int tiles_y, int vec_ok, uint8_t *__restrict__ tile_mark,
                                                     uint16_t *__restrict__ lane_mask, uint32_t flag_all) {
  __shared__ __attribute__((aligned(16))) float t[(SD_TY + 2) * SD_LDW];
  const double nlnpx2 = n_top * lnpx2;
  // (tried: identity and row-interleaved block -> tile maps instead of one band per XCD: 2 % slower)
  const int tile = sd_tile_of_block(blockIdx.x, tiles_x * tiles_y);
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int x0 = txi * SD_TX, y0 = tyi * SD_TY;
  const int H = w.H, W = w.W;
  sd_stage(t, dem, w, x0, y0, vec_ok);
  __syncthreads();

  const int tx = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cx = tx * 4, ry = wv * 4;  // tile column / row of the lane's 4 x 4 patch
  const int gx = x0 + cx;
  // every lane stays active to the end (its neighbours' DPP reads need it); stores are guarded
  auto load_row = [&](int lr, float *dst) {
    const float *row = &t[lr * SD_LDW];
    float4 m = *reinterpret_cast<const float4 *>(row + 4 + cx);
    float lh = row[3], rh = row[4 + SD_TX];  // columns beside the wave: wave-uniform address (broadcast)
    dst[0] = sd_from_prev_lane(lh, m.w);
    dst[1] = m.x;
    dst[2] = m.y;
    dst[3] = m.z;
    dst[4] = m.w;
    dst[5] = sd_from_next_lane(rh, m.x);
  };
  const bool full = vec_ok && gx + 3 < W;
  float a[6], bb[6], cc[6];
  load_row(ry, a);
  load_row(ry + 1, bb);
  uint32_t mask = flag_all;  // test knob: 0xFFFF sends every cell through the exact path as well
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int gy = y0 + ry + j;
    const long long o = (long long)gy * w.ld + gx;
    AccT fv[4] = {(AccT)-100, (AccT)-100, (AccT)-100, (AccT)-100};
    if (gy < H) {
      const AccT *pf = acc32 + o;
      if (full && sizeof(AccT) == 8) {
        const sd_v2l *p2 = reinterpret_cast<const sd_v2l *>(pf);
        sd_v2l a2 = __builtin_nontemporal_load(p2), b2 = __builtin_nontemporal_load(p2 + 1);
        fv[0] = (AccT)a2.x; fv[1] = (AccT)a2.y; fv[2] = (AccT)b2.x; fv[3] = (AccT)b2.y;
      } else if (full) {
        sd_v4i f4 = __builtin_nontemporal_load(reinterpret_cast<const sd_v4i *>(pf));
        fv[0] = (AccT)f4.x; fv[1] = (AccT)f4.y; fv[2] = (AccT)f4.z; fv[3] = (AccT)f4.w;
      } else {
        if (gx < W) fv[0] = pf[0];
        if (gx + 1 < W) fv[1] = pf[1];
        if (gx + 2 < W) fv[2] = pf[2];
        if (gx + 3 < W) fv[3] = pf[3];
      }
    }
    load_row(ry + 2 + j, cc);
    float so[4], ro[4], tio[4], mtio[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float c = bb[k + 1];
      const float cz = sd_centre(c);  // the centre's own value
      float sl, rad = 0.0f, tv, mv;
      bool flag = sd_slope_fast(c, a[k], a[k + 1], a[k + 2], bb[k], bb[k + 2], cc[k], cc[k + 1], cc[k + 2], kc, kd, sl);
      const bool snod = cz <= DT_NODATA;  // slope.py:231
      sl = snod ? DT_NODATA : sl;
      flag = flag && !snod;
      const float q = dt_pct_to_tan(sl);
      if (W_RAD) {  // dt_slope_rad: -100 where dem == -100, else the arctangent (q outside its domain: flagged)
        const bool rnod = cz == DT_NODATA;
        rad = rnod ? DT_NODATA : (float)dt_atanf_pos(q);
        flag = flag || (!rnod && !(q >= 0.0f && q < 1e30f));
      }
      const AccT f = fv[k];
      const bool tnod = f <= (AccT)-100;  // topoindexes.py:252
      flag = (sd_twi_fast(f, q, n_top, lnpx2, nlnpx2, tv, mv) && !tnod) || flag;
      so[k] = sl;
      ro[k] = rad;
      tio[k] = tnod ? DT_NODATA : tv;
      mtio[k] = tnod ? DT_NODATA : mv;
      mask |= (flag ? 1u : 0u) << (4 * j + k);
    }
    if (gy < H) {
      if (full) {
        if (W_SLOPE) sd_store4(slope + o, so[0], so[1], so[2], so[3]);
        if (W_RAD) sd_store4(slope_rad + o, ro[0], ro[1], ro[2], ro[3]);
        sd_store4(ti + o, tio[0], tio[1], tio[2], tio[3]);
        sd_store4(mti + o, mtio[0], mtio[1], mtio[2], mtio[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (gx + k < W) {
            if (W_SLOPE) slope[o + k] = so[k];
            if (W_RAD) slope_rad[o + k] = ro[k];
            ti[o + k] = tio[k];
            mti[o + k] = mtio[k];
          } else {
            mask &= ~(1u << (4 * j + k));
          }
        }
      }
    } else {
      mask &= ~(0xFu << (4 * j));
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
      a[q] = bb[q];
      bb[q] = cc[q];
    }
  }
  const int any = __syncthreads_or(mask != 0u);
  if (threadIdx.x == 0) tile_mark[tile] = (uint8_t)(any != 0);
  if (any) lane_mask[(size_t)tile * 256 + threadIdx.x] = (uint16_t)mask;
}

// the cold half: exact recomputation of the flagged cells (a handful per raster)
template <typename AccT>
__global__ __launch_bounds__(256) void k_slope_twi_fix(const float *__restrict__ dem, DtWin w, double px,
                                                      float *__restrict__ slope, float *__restrict__ slope_rad,
                                                      const AccT *__restrict__ acc32, double n_top, double lnpx2,
                                                      float *__restrict__ ti, float *__restrict__ mti, int tiles_x,
                                                      int tiles_y, int vec_ok, const uint8_t *__restrict__ tile_mark,
                                                      const uint16_t *__restrict__ lane_mask,
                                                      const DtLogEntry *__restrict__ g_tab) {
  __shared__ __attribute__((aligned(16))) float t[(SD_TY + 2) * SD_LDW];
  const int ntiles = tiles_x * tiles_y;
  const double dcard = px, ddiag = px * sqrt(2.0);
  const double inv_card = 1.0 / dcard, inv_diag = 1.0 / ddiag;
  // 256 tile marks per step, one per lane: an unmarked raster costs ceil(ntiles / 256) independent byte loads
  __shared__ uint8_t s_mark[256];
  for (int chunk = blockIdx.x / SD_FIX_SPLIT; chunk * 256 < ntiles; chunk += gridDim.x / SD_FIX_SPLIT) {
    const int mine = chunk * 256 + (int)threadIdx.x;
    const uint8_t m = mine < ntiles ? tile_mark[mine] : (uint8_t)0;
    __syncthreads();  // the previous chunk's readers are done with s_mark
    s_mark[threadIdx.x] = m;
    if (!__syncthreads_or(m)) continue;
    for (int i = blockIdx.x % SD_FIX_SPLIT; i < 256; i += SD_FIX_SPLIT) {
      if (!s_mark[i]) continue;  // block-uniform
      const int tile = chunk * 256 + i;
      const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
      const int x0 = txi * SD_TX, y0 = tyi * SD_TY;
      __syncthreads();  // the previous tile's readers are done with t
      sd_stage(t, dem, w, x0, y0, vec_ok);
      __syncthreads();
      uint32_t mask = lane_mask[(size_t)tile * 256 + threadIdx.x];
      const int cx = (threadIdx.x & 63) * 4, ry = (threadIdx.x >> 6) * 4;
      while (mask) {
        const int bit = __ffs((int)mask) - 1;
        mask &= mask - 1u;
        const int j = bit >> 2, k = bit & 3;
        const int gy = y0 + ry + j, gx = x0 + cx + k;
        if (gy >= w.H || gx >= w.W) continue;
        const float *p = &t[(ry + j + 1) * SD_LDW + 4 + cx + k];  // the centre in the staged tile
        const float cz = sd_centre(p[0]);
        SlopeCell sc = dt_slope_cell<false, true>(cz, p[-SD_LDW - 1], p[-SD_LDW], p[-SD_LDW + 1], p[-1], p[1],
                                                  p[SD_LDW - 1], p[SD_LDW], p[SD_LDW + 1], inv_card, inv_diag, dcard,
                                                  ddiag);
        const long long o = (long long)gy * w.ld + gx;
        const float rad = dt_slope_rad(sc.slope, cz);
        float tv, mv;
        dt_twi_cell((int64_t)acc32[o], rad, lnpx2, n_top, tv, mv, g_tab);
        if (slope) slope[o] = sc.slope;
        if (slope_rad) slope_rad[o] = rad;
        ti[o] = tv;
        mti[o] = mv;
      }
    }
  }
}

// ===========================================================================================
// D8 alone (N1), hot / cold like k_slope_twi: the chain's first kernel writes only the direction codes.
// Within a class the first strict maximum of the float32 differences wins (scan order N, W, E, S / NW, NE, SW, SE);
// between the classes the reference compares cb / px with db / (px sqrt 2), i.e. cb with db / sqrt 2: decided in
// float32 whenever the two differ by more than 2^-21 relative (the float32 product is within 2^-23 of db / sqrt 2),
// flagged for the exact float64 path of dt_slope_cell otherwise (~1e-6 of the cells; equality is impossible for
// non-zero differences, the ratio being irrational).
// ===========================================================================================
__device__ __forceinline__ bool sd_d8_fast(float c, float nw, float n, float ne, float w, float e, float sw, float s,
                                           float se, uint32_t &code) {
  float cb = 0.0f, db = 0.0f;
  uint32_t ccode = 0, dcode = 0;
#define SD_CAND(nb, best, bcode, code_) \
  {                                     \
    const float d_ = c - (nb);          \
    const bool up_ = d_ > best;         \
    best = up_ ? d_ : best;             \
    bcode = up_ ? code_ : bcode;        \
  }
  SD_CAND(n, cb, ccode, 64u)
  SD_CAND(w, cb, ccode, 16u)
  SD_CAND(e, cb, ccode, 1u)
  SD_CAND(s, cb, ccode, 4u)
  SD_CAND(nw, db, dcode, 32u)
  SD_CAND(ne, db, dcode, 128u)
  SD_CAND(sw, db, dcode, 8u)
  SD_CAND(se, db, dcode, 2u)
#undef SD_CAND
  const float t = db * 0.70710678118654752f;
  const float hi = fmaxf(cb, t);
  code = cb > t ? ccode : dcode;  // both zero: dcode == 0
  // not finite / tiny differences go to the exact path as well (inf - finite = inf would compare equal)
  return hi != 0.0f && (fabsf(cb - t) <= hi * 4.76837158e-7f || !(hi < 3.0e38f) || hi < 1.0e-30f);
}

// nod4 (may be NULL): the nodata mask, one 16-bit word per 4 x 4 patch of cells -- bit 4 j + k = cell (4 r + j, 4 i + k)
// holds the nodata sentinel (z <= -100 and nothing else: NaN and +inf are heights, as in the reference) -- what the flow-accumulation
// pass needs of the DEM (-100 on nodata cells), so that it reads 0.125 instead of 4 bytes per cell (dt_dev_slope_d8_m /
// dt_dev_flowacc_river_flowhand_local_m).  A patch is what one thread of this kernel owns: ONE store per thread (four
// byte stores, a row each, cost this issue-bound kernel 12 %).  ldm = words per row of patches.  Only for a single
// raster (window origin on the 4-cell grid).
#define SD_D8_SLOPE 0
#include "dt_d8_kernel.inc"
#undef SD_D8_SLOPE
#define SD_D8_SLOPE 1
#include "dt_d8_kernel.inc"
#undef SD_D8_SLOPE

__global__ __launch_bounds__(256) void k_d8_fix(const float *__restrict__ dem, DtWin w, double px,
                                               uint8_t *__restrict__ fdr, int tiles_x, int tiles_y, int vec_ok,
                                               const uint8_t *__restrict__ tile_mark,
                                               const uint16_t *__restrict__ lane_mask) {
  __shared__ __attribute__((aligned(16))) float t[(SD_TY + 2) * SD_LDW];
  __shared__ uint8_t s_mark[256];
  const int ntiles = tiles_x * tiles_y;
  const double dcard = px, ddiag = px * sqrt(2.0);
  const double inv_card = 1.0 / dcard, inv_diag = 1.0 / ddiag;
  for (int chunk = blockIdx.x / SD_FIX_SPLIT; chunk * 256 < ntiles; chunk += gridDim.x / SD_FIX_SPLIT) {
    const int mine = chunk * 256 + (int)threadIdx.x;
    const uint8_t m = mine < ntiles ? tile_mark[mine] : (uint8_t)0;
    __syncthreads();
    s_mark[threadIdx.x] = m;
    if (!__syncthreads_or(m)) continue;
    for (int i = blockIdx.x % SD_FIX_SPLIT; i < 256; i += SD_FIX_SPLIT) {
      if (!s_mark[i]) continue;  // block-uniform
      const int tile = chunk * 256 + i;
      const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
      const int x0 = txi * SD_TX, y0 = tyi * SD_TY;
      __syncthreads();
      sd_stage(t, dem, w, x0, y0, vec_ok);
      __syncthreads();
      uint32_t mask = lane_mask[(size_t)tile * 256 + threadIdx.x];
      const int cx = (threadIdx.x & 63) * 4, ry = (threadIdx.x >> 6) * 4;
      while (mask) {
        const int bit = __ffs((int)mask) - 1;
        mask &= mask - 1u;
        const int j = bit >> 2, k = bit & 3;
        const int gy = y0 + ry + j, gx = x0 + cx + k;
        if (gy >= w.H || gx >= w.W) continue;
        const float *p = &t[(ry + j + 1) * SD_LDW + 4 + cx + k];
        const float cz = sd_centre(p[0]);
        SlopeCell sc = dt_slope_cell<true, false>(cz, p[-SD_LDW - 1], p[-SD_LDW], p[-SD_LDW + 1], p[-1], p[1],
                                                  p[SD_LDW - 1], p[SD_LDW], p[SD_LDW + 1], inv_card, inv_diag, dcard,
                                                  ddiag);
        uint32_t code = sc.code;
        const int gyy = w.gy0 + gy, gxx = w.gx0 + gx;
        if (code == 0u && !(cz <= DT_NODATA)) {
          if (gyy == w.Hg - 1) code = 4u;
          else if (gyy == 0) code = 64u;
          else if (gxx == 0) code = 16u;
          else if (gxx == w.Wg - 1) code = 1u;
        }
        fdr[(long long)gy * w.ld + gx] = (uint8_t)code;
      }
    }
  }
}

// bytes of the mark / mask workspace for an H x W window: DtStencilAux at its count of 256 x 16 tiles
static int64_t sd_aux_tiles(int64_t H, int64_t W) { return ((W + SD_TX - 1) / SD_TX) * ((H + SD_TY - 1) / SD_TY); }
size_t dt_stencil_aux_bytes(int64_t H, int64_t W) { return dt_stencil_aux_layout(sd_aux_tiles(H, W), nullptr).bytes; }

// the fused slope + TI + MTI pair (hot kernel + fix-up of the flagged cells) for one accumulation width
template <typename AccT>
static int launch_slope_twi(hipStream_t s, const DtWin &w, const float *dem, double px, float *slope, float *slope_rad,
                            const AccT *acc, double n_top, float *ti, float *mti, void *aux, int vec_ok) {
  const int tiles_x = (int)((w.W + SD_TX - 1) / SD_TX), tiles_y = (int)((w.H + SD_TY - 1) / SD_TY);
  const int64_t ntiles = (int64_t)tiles_x * tiles_y;
  DT_REQUIRE(ntiles < (1ll << 31), "raster too large for one launch");
  DT_REQUIRE(aux != nullptr, "fused TWI needs its mark / mask workspace");
  dim3 g((unsigned)ntiles), b(256);
  const bool ws = slope != nullptr, wr = slope_rad != nullptr;
  const DtStencilAux A = dt_stencil_aux_layout(ntiles, aux);
  uint8_t *mark = A.mark;
  uint16_t *lmask = A.lmask;
  const double kc = 100.0 / px, kd = 100.0 / (px * sqrt(2.0)), lnpx2 = log(px * px);
  const DtLogEntry *g_tab = dt_math_device_table(s);
#define DT_HOT(S, R)                                                                                               \
  hipLaunchKernelGGL((k_slope_twi<S, R, AccT>), g, b, 0, s, dem, w, kc, kd, slope, slope_rad, acc, n_top, lnpx2, ti, \
                     mti, tiles_x, tiles_y, vec_ok, mark, lmask, dt_debug_get(DT_DBG_TWI_FLAG_ALL) ? 0xFFFFu : 0u)
  if (ws && wr) DT_HOT(true, true);
  else if (ws) DT_HOT(true, false);
  else if (wr) DT_HOT(false, true);
  else DT_HOT(false, false);
#undef DT_HOT
  unsigned fix_blocks = SD_FIX_SPLIT * dt_capped_grid(ntiles, 1024);
  hipLaunchKernelGGL((k_slope_twi_fix<AccT>), dim3(fix_blocks), b, 0, s, dem, w, px, slope, slope_rad, acc, n_top,
                     lnpx2, ti, mti, tiles_x, tiles_y, vec_ok, mark, lmask, g_tab);
  return DT_OK;
}

// The float32 chain's first kernel and its fix-up: D8 codes, the nodata mask and -- slope != NULL -- the slope raster
// with its flags in `smarks` (dt_stencil_aux_bytes: the marks of dt_launch_fa_finish_fh_local's TI / MTI epilogue and
// of dt_launch_slope_twi_fix).  `aux` holds the D8 marks, as in dt_launch_stencil.  A single raster (full window).
int dt_launch_d8_slope(hipStream_t s, const DtWin &w, const float *dem, double px, uint8_t *fdr, float *slope,
                       void *aux, uint8_t *nod4, int ldm, void *smarks) {
  if (w.H == 0 || w.W == 0) return DT_OK;
  if (!slope) return dt_launch_stencil(s, w, dem, px, nullptr, fdr, nullptr, nullptr, 0, 0.0, nullptr, nullptr, aux, nod4, ldm);
  DT_REQUIRE(aux && smarks && nod4 && fdr, "D8 + slope needs both mark workspaces, the codes and the nodata mask");
  const int tiles_x = (int)((w.W + SD_TX - 1) / SD_TX), tiles_y = (int)((w.H + SD_TY - 1) / SD_TY);
  const int64_t ntiles = (int64_t)tiles_x * tiles_y;
  DT_REQUIRE(ntiles < (1ll << 31), "raster too large for one launch");
  const int vec_ok = (w.W % 4 == 0) && (w.ld % 4 == 0) && (((uintptr_t)dem | (uintptr_t)slope) & 15) == 0 &&
                     ((uintptr_t)fdr & 3) == 0;
  dim3 g((unsigned)ntiles), b(256);
  const DtStencilAux A = dt_stencil_aux_layout(ntiles, aux), S = dt_stencil_aux_layout(ntiles, smarks);
  const double kc = 100.0 / px, kd = 100.0 / (px * sqrt(2.0));
  hipLaunchKernelGGL(k_d8_slope, g, b, 0, s, dem, w, fdr, tiles_x, tiles_y, vec_ok, A.mark, A.lmask, nod4, ldm, kc, kd,
                     slope, S.mark, S.lmask, dt_debug_get(DT_DBG_TWI_FLAG_ALL) ? 0xFFFFu : 0u);
  unsigned fix_blocks = SD_FIX_SPLIT * dt_capped_grid(ntiles, 1024);
  hipLaunchKernelGGL(k_d8_fix, dim3(fix_blocks), b, 0, s, dem, w, px, fdr, tiles_x, tiles_y, vec_ok, A.mark, A.lmask);
  return DT_OK;
}

// k_slope_twi_fix alone over the marks k_d8_slope and k_fa3fh1_twi left in `smarks`: slope, TI and MTI of every marked
// cell from the DEM and the accumulation with the exact functions (256 x 16 tiles, int32 accumulation)
int dt_launch_slope_twi_fix(hipStream_t s, const DtWin &w, const float *dem, double px, float *slope,
                            const int32_t *acc, double n_top, float *ti, float *mti, void *smarks) {
  if (w.H == 0 || w.W == 0) return DT_OK;
  DT_REQUIRE(smarks && dem && slope && acc && ti && mti, "NULL pointer");
  const int tiles_x = (int)((w.W + SD_TX - 1) / SD_TX), tiles_y = (int)((w.H + SD_TY - 1) / SD_TY);
  const int64_t ntiles = (int64_t)tiles_x * tiles_y;
  DT_REQUIRE(ntiles < (1ll << 31), "raster too large for one launch");
  const int vec_ok = (w.W % 4 == 0) && (w.ld % 4 == 0) && ((uintptr_t)dem & 15) == 0;  // (the staging's loads)
  const DtStencilAux S = dt_stencil_aux_layout(ntiles, smarks);
  unsigned fix_blocks = SD_FIX_SPLIT * dt_capped_grid(ntiles, 1024);
  hipLaunchKernelGGL((k_slope_twi_fix<int32_t>), dim3(fix_blocks), dim3(256), 0, s, dem, w, px, slope, (float *)nullptr,
                     acc, n_top, log(px * px), ti, mti, tiles_x, tiles_y, vec_ok, (const uint8_t *)S.mark,
                     (const uint16_t *)S.lmask, dt_math_device_table(s));
  return DT_OK;
}

// `acc` (fused TI / MTI only): int32_t* raster, or int64_t* with acc64 != 0
int dt_launch_stencil(hipStream_t s, const DtWin &w, const float *dem, double px, float *slope,
                      uint8_t *fdr, float *slope_rad, const void *acc, int acc64, double n_top, float *ti,
                      float *mti, void *aux, uint8_t *nod4, int ldm) {
  const int64_t H = w.H, W = w.W;
  if (H == 0 || W == 0) return DT_OK;
  int tiles_x = (int)((W + SD_TX - 1) / SD_TX), tiles_y = (int)((H + SD_TY - 1) / SD_TY);
  int64_t ntiles = (int64_t)tiles_x * tiles_y;
  DT_REQUIRE(ntiles < (1ll << 31), "raster too large for one launch");
  // 16-byte vector path needs W % 4 == 0 and 16-byte aligned bases
  int vec_ok = (W % 4 == 0) && (w.ld % 4 == 0) && (((uintptr_t)dem & 15) == 0) && (!slope || ((uintptr_t)slope & 15) == 0) &&
               (!slope_rad || ((uintptr_t)slope_rad & 15) == 0) && (!ti || ((uintptr_t)ti & 15) == 0) &&
               (!mti || ((uintptr_t)mti & 15) == 0) && (!fdr || ((uintptr_t)fdr & 3) == 0) &&
               (!acc || ((uintptr_t)acc & 15) == 0);
  dim3 g((unsigned)ntiles), b(256);
  bool ws = slope != nullptr, wf = fdr != nullptr, wr = slope_rad != nullptr, wt = ti != nullptr;
  DT_REQUIRE(!nod4 || (wf && aux && !ws && !wr && !wt),
             "the nodata mask comes from the D8-only kernel (fdr and a workspace, no other output)");
#define DT_GO(S, F, R) \
  hipLaunchKernelGGL((k_stencil<S, F, R>), g, b, 0, s, dem, w, px, slope, fdr, slope_rad, tiles_x, tiles_y, vec_ok)
  if (wt) {
    DT_REQUIRE(acc && mti, "fused TWI needs the accumulation raster, ti and mti");
    if (acc64)
      return launch_slope_twi(s, w, dem, px, slope, slope_rad, (const long long *)acc, n_top, ti, mti, aux, vec_ok);
    return launch_slope_twi(s, w, dem, px, slope, slope_rad, (const int32_t *)acc, n_top, ti, mti, aux, vec_ok);
  } else if (ws && wf && wr) DT_GO(true, true, true);
  else if (ws && wf) DT_GO(true, true, false);
  else if (ws && wr) DT_GO(true, false, true);
  else if (wf && wr) DT_GO(false, true, true);
  else if (ws) DT_GO(true, false, false);
  else if (wf && aux) {  // D8 alone with a workspace: the hot / cold pair
    const DtStencilAux A = dt_stencil_aux_layout(ntiles, aux);
    hipLaunchKernelGGL(k_d8<false>, g, b, 0, s, dem, w, fdr, tiles_x, tiles_y, vec_ok, A.mark, A.lmask, nod4, ldm);
    unsigned fix_blocks = SD_FIX_SPLIT * dt_capped_grid(ntiles, 1024);
    hipLaunchKernelGGL(k_d8_fix, dim3(fix_blocks), b, 0, s, dem, w, px, fdr, tiles_x, tiles_y, vec_ok, A.mark, A.lmask);
  } else if (wf) DT_GO(false, true, false);
  else if (wr) DT_GO(false, false, true);
#undef DT_GO
  return DT_OK;
}

// ===========================================================================================
// The same stencils on float64 heights (the resident chain's heights="float64" tier; dt_capi.hip dt_dev_*_f64).
//
// Tile = 64 columns x 16 rows per 256-thread workgroup, staged with its 1-cell halo through LDS as doubles (18 x 66
// x 8 B = 9.3 KiB: the LDS is not what limits occupancy); every load of a thread is issued before the first LDS
// store.  Lane tx owns column tx of the tile, wave ty rows 4 ty .. 4 ty + 3 (a wave's row of stores is 64 cells:
// 256 B of float32, 64 B of codes).  Cells outside the raster are staged as -100, the reference's ring (slope.py:175),
// so the neighbour rule "nb == -100: skipped" (slope.py:247) covers them.  Heights are the DEM's own values: only
// z <= -100 is nodata (no NaN / inf sentinel handling).
// ===========================================================================================
#define SW_TX 64
#define SW_TY 16
#define SW_LDW (SW_TX + 2)

__device__ __forceinline__ void sw_stage(double *t, const double *__restrict__ dem, int H, int W, int x0, int y0) {
  constexpr int N = (SW_TY + 2) * SW_LDW, NV = (N + 255) / 256;
  double v[NV];
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 256 * u;
    const int r = i / SW_LDW, c = i - r * SW_LDW;
    const int gy = y0 - 1 + r, gx = x0 - 1 + c;
    v[u] = -100.0;
    if (i < N && gy >= 0 && gy < H && gx >= 0 && gx < W) v[u] = dem[(long long)gy * W + gx];
  }
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 256 * u;
    if (i < N) t[i] = v[u];
  }
}

// the eight neighbours of tile cell (r, c) in scan order NW, N, NE, W, E, SW, S, SE
__device__ __forceinline__ void sw_nbrs(const double *t, int r, int c, double (&nb)[8]) {
  const double *p = &t[(r + 1) * SW_LDW + c + 1];
  nb[0] = p[-SW_LDW - 1];
  nb[1] = p[-SW_LDW];
  nb[2] = p[-SW_LDW + 1];
  nb[3] = p[-1];
  nb[4] = p[1];
  nb[5] = p[SW_LDW - 1];
  nb[6] = p[SW_LDW];
  nb[7] = p[SW_LDW + 1];
}
__device__ __forceinline__ bool sw_diag(int k) { return k == 0 || k == 2 || k == 5 || k == 7; }

// Largest cardinal and largest diagonal difference c - nb over the neighbours that count (nb != -100); 0 when none is
// positive.  A strict `>` skips NaN as the reference's `aux < v` does.  Division by a positive constant is monotone, so
// the largest quotient of a class is its largest difference divided once.
__device__ __forceinline__ void sw_class_max(double c, const double (&nb)[8], double &dc, double &dd) {
  dc = 0.0;
  dd = 0.0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double d = c - nb[k];
    const bool ok = nb[k] != -100.0;
    if (sw_diag(k)) dd = (ok && d > dd) ? d : dd;
    else dc = (ok && d > dc) ? d : dc;
  }
}

// D8 code of the literal definition (flowdir.d8, N1, with float64 differences): the first neighbour in
// scan order whose quotient equals the maximum v > 0.  The quotient is not injective (two differences may round to
// the same value), so a neighbour other than its class's largest difference can still be the first to reach v: it is
// divided whenever its difference lies within 1e-15 (relative) of the class maximum -- equal float64 quotients of
// one divisor are within 2^-52 of each other -- which on real terrain is essentially never.
__device__ __forceinline__ uint32_t sw_d8_code(double c, const double (&nb)[8], double dc, double dd, double qc,
                                               double qd, double dcard, double ddiag) {
  const uint8_t CODE[8] = {32, 64, 128, 16, 1, 8, 4, 2};
  const double v = qc > qd ? qc : qd;
  uint32_t code = 0u;
  if (!(v > 0.0)) return 0u;
#pragma unroll
  for (int k = 7; k >= 0; k--) {  // backwards: the last assignment is the first match in scan order
    const bool dg = sw_diag(k);
    const double best = dg ? dd : dc, q = dg ? qd : qc, d = c - nb[k];
    if (nb[k] == -100.0 || !(d > 0.0) || q != v) continue;
    bool hit = d == best;
    if (!hit && (best == __builtin_inf() || d >= best * (1.0 - 1e-15))) hit = d / (dg ? ddiag : dcard) == v;
    code = hit ? (uint32_t)CODE[k] : code;
  }
  return code;
}

// D8 (fdr, may be NULL), the exact slope % (may be NULL) and the float32 nodata proxy (may be NULL): -100 where
// z <= -100, otherwise (float)z kept above -100 (NaN stays NaN).  What the flow-accumulation kernels need of the DEM
// is exactly that nodata test, so they run unchanged on the proxy.
__global__ __launch_bounds__(256) void k_d8_f64(const double *__restrict__ dem, int H, int W, double px,
                                                uint8_t *__restrict__ fdr, float *__restrict__ slope,
                                                float *__restrict__ proxy) {
  __shared__ double t[(SW_TY + 2) * SW_LDW];
  const int x0 = (int)blockIdx.x * SW_TX, y0 = (int)blockIdx.y * SW_TY;
  sw_stage(t, dem, H, W, x0, y0);
  __syncthreads();
  const int tx = (int)threadIdx.x & 63, ty = (int)threadIdx.x >> 6;
  const int gx = x0 + tx;
  if (gx >= W) return;
  const double dcard = px, ddiag = px * sqrt(2.0);
  const float above = -99.99999237060547f;  // the float32 value next to -100 towards 0
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = ty * 4 + j, gy = y0 + r;
    if (gy >= H) break;
    const double c = t[(r + 1) * SW_LDW + tx + 1];
    const long long o = (long long)gy * W + gx;
    const bool nod = c <= -100.0;  // slope.py:231
    double nb[8];
    sw_nbrs(t, r, tx, nb);
    double dc, dd;
    sw_class_max(c, nb, dc, dd);
    const double qc = dc > 0.0 ? dc / dcard : 0.0, qd = dd > 0.0 ? dd / ddiag : 0.0;
    if (fdr) {
      uint32_t code = nod ? 0u : sw_d8_code(c, nb, dc, dd, qc, qd, dcard, ddiag);
      if (code == 0u && !nod)  // N1 border rule
        code = gy == H - 1 ? 4u : (gy == 0 ? 64u : (gx == 0 ? 16u : (gx == W - 1 ? 1u : 0u)));
      fdr[o] = (uint8_t)code;
    }
    if (slope) slope[o] = nod ? DT_NODATA : (float)((qc > qd ? qc : qd) * 100.0);  // slope.py:259
    if (proxy) {
      const float f = (float)c;
      proxy[o] = nod ? DT_NODATA : (f <= DT_NODATA ? above : f);
    }
  }
}

// slope + TI + MTI (+ radians) on float64 heights: the float32 kernel's per-cell math (k_slope_twi) from the class
// maxima of the float64 differences -- the same product-form slope and its rounding test (sd_slope_fast), the same
// sd_twi_fast and its flags -- and the cold path of k_slope_twi_fix (exact divisions, dt_slope_rad, dt_twi_cell) for
// the flagged cells, in place: they are a handful per raster.  On heights that are float32 values the class maxima are
// the float32 kernel's, so every cell takes the same path there and comes out bit for bit the same.
template <bool W_RAD>
__global__ __launch_bounds__(256) void k_slope_twi_f64(const double *__restrict__ dem, int H, int W, double px,
                                                       double kc, double kd, const int32_t *__restrict__ acc32,
                                                       double n_top, double lnpx2, float *__restrict__ slope,
                                                       float *__restrict__ slope_rad, float *__restrict__ ti,
                                                       float *__restrict__ mti, const DtLogEntry *__restrict__ g_tab) {
  __shared__ double t[(SW_TY + 2) * SW_LDW];
  const int x0 = (int)blockIdx.x * SW_TX, y0 = (int)blockIdx.y * SW_TY;
  sw_stage(t, dem, H, W, x0, y0);
  __syncthreads();
  const int tx = (int)threadIdx.x & 63, ty = (int)threadIdx.x >> 6;
  const int gx = x0 + tx;
  if (gx >= W) return;
  const double nlnpx2 = n_top * lnpx2;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = ty * 4 + j, gy = y0 + r;
    if (gy >= H) break;
    const long long o = (long long)gy * W + gx;
    const int32_t f = acc32[o];
    const double c = t[(r + 1) * SW_LDW + tx + 1];
    double nb[8];
    sw_nbrs(t, r, tx, nb);
    double dc, dd;
    sw_class_max(c, nb, dc, dd);
    // sd_slope_fast on the class maxima
    const double qp = dc * kc > dd * kd ? dc * kc : dd * kd;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(qp);
    const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    const bool near_mid = ((lo & 0x1FFFFFFFu) - (0x10000000u - SD_MID)) <= 2u * SD_MID;
    const bool odd = ((hi >> 20) - 897u) > 253u && bits != 0ull;
    bool flag = near_mid || odd;
    float sl = (float)qp, rad = 0.0f, tv, mv;
    const bool snod = c <= -100.0;  // slope.py:231
    sl = snod ? DT_NODATA : sl;
    flag = flag && !snod;
    const float q = dt_pct_to_tan(sl);
    const bool rnod = c == -100.0;
    if (W_RAD) {
      rad = rnod ? DT_NODATA : (float)dt_atanf_pos(q);
      flag = flag || (!rnod && !(q >= 0.0f && q < 1e30f));
    }
    const bool tnod = f <= -100;  // topoindexes.py:252
    flag = (sd_twi_fast(f, q, n_top, lnpx2, nlnpx2, tv, mv) && !tnod) || flag;
    tv = tnod ? DT_NODATA : tv;
    mv = tnod ? DT_NODATA : mv;
    if (flag) {  // k_slope_twi_fix's exact path
      const double dcard = px, ddiag = px * sqrt(2.0);
      const double qc = dc > 0.0 ? dc / dcard : 0.0, qd = dd > 0.0 ? dd / ddiag : 0.0;
      sl = snod ? DT_NODATA : (float)((qc > qd ? qc : qd) * 100.0);
      rad = dt_slope_rad(sl, rnod ? DT_NODATA : 0.0f);
      dt_twi_cell((int64_t)f, rad, lnpx2, n_top, tv, mv, g_tab);
    }
    if (slope) slope[o] = sl;
    if (W_RAD) slope_rad[o] = rad;
    ti[o] = tv;
    mti[o] = mv;
  }
}

int dt_launch_d8_f64(hipStream_t s, const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *slope,
                     float *proxy) {
  if (H == 0 || W == 0) return DT_OK;
  const dim3 g((unsigned)((W + SW_TX - 1) / SW_TX), (unsigned)((H + SW_TY - 1) / SW_TY));
  DT_REQUIRE(g.y < 65536u, "raster too tall for one launch");
  hipLaunchKernelGGL(k_d8_f64, g, dim3(256), 0, s, dem, (int)H, (int)W, px, fdr, slope, proxy);
  return DT_OK;
}

int dt_launch_slope_twi_f64(hipStream_t s, const double *dem, const int32_t *acc32, int64_t H, int64_t W, double px,
                            double n_top, float *slope, float *slope_rad, float *ti, float *mti) {
  if (H == 0 || W == 0) return DT_OK;
  const dim3 g((unsigned)((W + SW_TX - 1) / SW_TX), (unsigned)((H + SW_TY - 1) / SW_TY));
  DT_REQUIRE(g.y < 65536u, "raster too tall for one launch");
  // the float32 kernel's constants, computed the same way (launch_slope_twi)
  const double kc = 100.0 / px, kd = 100.0 / (px * sqrt(2.0)), lnpx2 = log(px * px);
  const DtLogEntry *g_tab = dt_math_device_table(s);
  if (slope_rad)
    hipLaunchKernelGGL(k_slope_twi_f64<true>, g, dim3(256), 0, s, dem, (int)H, (int)W, px, kc, kd, acc32, n_top, lnpx2,
                       slope, slope_rad, ti, mti, g_tab);
  else
    hipLaunchKernelGGL(k_slope_twi_f64<false>, g, dim3(256), 0, s, dem, (int)H, (int)W, px, kc, kd, acc32, n_top,
                       lnpx2, slope, slope_rad, ti, mti, g_tab);
  return DT_OK;
}

// ---- the same two stencils on one rank's window of a larger raster (tiling.RankTile(heights="float64")) ----------------
// The tile is staged from the rank's memory (core + halo, row stride w.ld; pointers at the core origin); a cell outside
// the GLOBAL raster is staged as -100, the reference's ring, so the result at every cell is the single raster's.  The
// border rule of D8 looks at the global raster's edges.
__device__ __forceinline__ void sw_stage_w(double *t, const double *__restrict__ dem, const DtWin &w, int x0, int y0) {
  constexpr int N = (SW_TY + 2) * SW_LDW, NV = (N + 255) / 256;
  double v[NV];
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 256 * u;
    const int r = i / SW_LDW, c = i - r * SW_LDW;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    v[u] = -100.0;
    if (i < N && dt_readable(w, y, x)) v[u] = dem[(long long)y * w.ld + x];
  }
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 256 * u;
    if (i < N) t[i] = v[u];
  }
}

// k_d8_f64 on a window (fdr and proxy may each be NULL)
__global__ __launch_bounds__(256) void k_d8_f64_w(const double *__restrict__ dem, DtWin w, double px,
                                                  uint8_t *__restrict__ fdr, float *__restrict__ proxy) {
  __shared__ double t[(SW_TY + 2) * SW_LDW];
  const int x0 = (int)blockIdx.x * SW_TX, y0 = (int)blockIdx.y * SW_TY;
  sw_stage_w(t, dem, w, x0, y0);
  __syncthreads();
  const int tx = (int)threadIdx.x & 63, ty = (int)threadIdx.x >> 6;
  const int x = x0 + tx;
  if (x >= w.W) return;
  const double dcard = px, ddiag = px * sqrt(2.0);
  const float above = -99.99999237060547f;  // the float32 value next to -100 towards 0
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = ty * 4 + j, y = y0 + r;
    if (y >= w.H) break;
    const double c = t[(r + 1) * SW_LDW + tx + 1];
    const long long o = (long long)y * w.ld + x;
    const bool nod = c <= -100.0;  // slope.py:231
    if (fdr) {
      double nb[8];
      sw_nbrs(t, r, tx, nb);
      double dc, dd;
      sw_class_max(c, nb, dc, dd);
      const double qc = dc > 0.0 ? dc / dcard : 0.0, qd = dd > 0.0 ? dd / ddiag : 0.0;
      uint32_t code = nod ? 0u : sw_d8_code(c, nb, dc, dd, qc, qd, dcard, ddiag);
      if (code == 0u && !nod) {  // N1 border rule, on the global raster's edges
        const int gy = w.gy0 + y, gx = w.gx0 + x;
        code = gy == w.Hg - 1 ? 4u : (gy == 0 ? 64u : (gx == 0 ? 16u : (gx == w.Wg - 1 ? 1u : 0u)));
      }
      fdr[o] = (uint8_t)code;
    }
    if (proxy) {
      const float f = (float)c;
      proxy[o] = nod ? DT_NODATA : (f <= DT_NODATA ? above : f);
    }
  }
}

// k_slope_twi_f64 on a window, on an int32 or int64 accumulation raster (AccT)
template <bool W_RAD, typename AccT>
__global__ __launch_bounds__(256) void k_slope_twi_f64_w(const double *__restrict__ dem, DtWin w, double px, double kc,
                                                         double kd, const AccT *__restrict__ acc, double n_top,
                                                         double lnpx2, float *__restrict__ slope,
                                                         float *__restrict__ slope_rad, float *__restrict__ ti,
                                                         float *__restrict__ mti, const DtLogEntry *__restrict__ g_tab) {
  __shared__ double t[(SW_TY + 2) * SW_LDW];
  const int x0 = (int)blockIdx.x * SW_TX, y0 = (int)blockIdx.y * SW_TY;
  sw_stage_w(t, dem, w, x0, y0);
  __syncthreads();
  const int tx = (int)threadIdx.x & 63, ty = (int)threadIdx.x >> 6;
  const int x = x0 + tx;
  if (x >= w.W) return;
  const double nlnpx2 = n_top * lnpx2;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = ty * 4 + j, y = y0 + r;
    if (y >= w.H) break;
    const long long o = (long long)y * w.ld + x;
    const AccT f = acc[o];
    const double c = t[(r + 1) * SW_LDW + tx + 1];
    double nb[8];
    sw_nbrs(t, r, tx, nb);
    double dc, dd;
    sw_class_max(c, nb, dc, dd);
    const double qp = dc * kc > dd * kd ? dc * kc : dd * kd;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(qp);
    const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    const bool near_mid = ((lo & 0x1FFFFFFFu) - (0x10000000u - SD_MID)) <= 2u * SD_MID;
    const bool odd = ((hi >> 20) - 897u) > 253u && bits != 0ull;
    bool flag = near_mid || odd;
    float sl = (float)qp, rad = 0.0f, tv, mv;
    const bool snod = c <= -100.0;  // slope.py:231
    sl = snod ? DT_NODATA : sl;
    flag = flag && !snod;
    const float q = dt_pct_to_tan(sl);
    const bool rnod = c == -100.0;
    if (W_RAD) {
      rad = rnod ? DT_NODATA : (float)dt_atanf_pos(q);
      flag = flag || (!rnod && !(q >= 0.0f && q < 1e30f));
    }
    const bool tnod = f <= -100;  // topoindexes.py:252
    flag = (sd_twi_fast(f, q, n_top, lnpx2, nlnpx2, tv, mv) && !tnod) || flag;
    tv = tnod ? DT_NODATA : tv;
    mv = tnod ? DT_NODATA : mv;
    if (flag) {  // k_slope_twi_fix's exact path
      const double dcard = px, ddiag = px * sqrt(2.0);
      const double qc = dc > 0.0 ? dc / dcard : 0.0, qd = dd > 0.0 ? dd / ddiag : 0.0;
      sl = snod ? DT_NODATA : (float)((qc > qd ? qc : qd) * 100.0);
      rad = dt_slope_rad(sl, rnod ? DT_NODATA : 0.0f);
      dt_twi_cell((int64_t)f, rad, lnpx2, n_top, tv, mv, g_tab);
    }
    if (slope) slope[o] = sl;
    if (W_RAD) slope_rad[o] = rad;
    ti[o] = tv;
    mti[o] = mv;
  }
}

int dt_launch_d8_f64_w(hipStream_t s, const DtWin &w, const double *dem, double px, uint8_t *fdr, float *proxy) {
  if (w.H == 0 || w.W == 0) return DT_OK;
  const dim3 g((unsigned)((w.W + SW_TX - 1) / SW_TX), (unsigned)((w.H + SW_TY - 1) / SW_TY));
  DT_REQUIRE(g.y < 65536u, "window too tall for one launch");
  hipLaunchKernelGGL(k_d8_f64_w, g, dim3(256), 0, s, dem, w, px, fdr, proxy);
  return DT_OK;
}

int dt_launch_slope_twi_f64_w(hipStream_t s, const DtWin &w, const double *dem, const void *acc, int acc64, double px,
                              double n_top, float *slope, float *slope_rad, float *ti, float *mti) {
  if (w.H == 0 || w.W == 0) return DT_OK;
  const dim3 g((unsigned)((w.W + SW_TX - 1) / SW_TX), (unsigned)((w.H + SW_TY - 1) / SW_TY));
  DT_REQUIRE(g.y < 65536u, "window too tall for one launch");
  const double kc = 100.0 / px, kd = 100.0 / (px * sqrt(2.0)), lnpx2 = log(px * px);
  const DtLogEntry *g_tab = dt_math_device_table(s);
#define DT_STW64(R, T) \
  hipLaunchKernelGGL((k_slope_twi_f64_w<R, T>), g, dim3(256), 0, s, dem, w, px, kc, kd, (const T *)acc, n_top, lnpx2, \
                     slope, slope_rad, ti, mti, g_tab)
  if (acc64) {
    if (slope_rad) DT_STW64(true, int64_t);
    else DT_STW64(false, int64_t);
  } else {
    if (slope_rad) DT_STW64(true, int32_t);
    else DT_STW64(false, int32_t);
  }
#undef DT_STW64
  return DT_OK;
}
