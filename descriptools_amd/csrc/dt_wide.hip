// dt_wide.hip -- the descriptors that read HEIGHTS, on a DEM (or HAND) that float32 cannot hold.
//
// The reference takes every height difference in the raster's OWN dtype: slope.py:244-258 under Numba typing
// (float64 - float64 for a float64 DEM, int64 - int64 for an integer one), flowhand.py:436-438 `dem - dem[indices]`,
// downslope.py:468 `dem[i] - dem[pos]`; and gfi.py:289-294 / :429-440 add 0.01 to whatever HAND they are given, in
// float64.  The resident chain and every hot kernel of this library keep heights as float32 -- the same arithmetic
// exactly when the heights ARE float32 values, which is what descriptools_amd/_lib.py checks at the boundary.  A
// raster that fails that check (a genuinely float64 DEM; integer heights beyond 2^24, which float64 holds exactly up
// to 2^53) takes the kernels below instead: one thread per cell on global memory, heights as float64, the literal
// expressions.  They are the capability, not the benchmark: a float64 raster moves twice the bytes and these kernels
// make no attempt at the LDS staging of the float32 path (slope: 9 L2-served reads per cell; downslope: the plain
// per-cell walk).  Pinned by tests/golden/f64.npz, the reference's own run on such a raster.
#include <math.h>

#include "dt_common.h"
#include "dt_kernels.h"

// S3 slope (%), slope.py:210-259 with float64 heights
__global__ __launch_bounds__(256) void k_slope_f64(const double *__restrict__ dem, int H, int W, double px,
                                                  float *__restrict__ slope) {
  const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
  const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
  if (x >= W || y >= H) return;
  const long long i = (long long)y * W + x;
  const double c = dem[i];
  if (c <= -100.0) {  // slope.py:231
    slope[i] = DT_NODATA;
    return;
  }
  const double dcard = px, ddiag = px * sqrt(2.0);
  double aux = 0.0;
  // scan order NW, N, NE, W, E, SW, S, SE with strict `<` (slope.py:244-258); only the maximum reaches the output
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int dy = k < 3 ? -1 : (k < 5 ? 0 : 1);
    const int dx = (k == 0 || k == 3 || k == 5) ? -1 : ((k == 1 || k == 6) ? 0 : 1);
    const int yy = y + dy, xx = x + dx;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;  // the -100 ring (slope.py:175-182)
    const double nb = dem[(long long)yy * W + xx];
    if (nb == -100.0) continue;  // slope.py:247
    const double v = (c - nb) / ((dy == 0 || dx == 0) ? dcard : ddiag);
    if (aux < v) aux = v;
  }
  slope[i] = (float)(aux * 100.0);
}

// F4 HAND, flowhand.py:414-442, in float64
__global__ __launch_bounds__(256) void k_hand_f64(const double *__restrict__ dem, const int64_t *__restrict__ idx,
                                                 int64_t n, double *__restrict__ hand) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double z = dem[i];
  double h = -100.0;
  int64_t k = idx[i];
  if (z != -100.0 && k != -100) {
    if (k < 0) k += n;  // numpy negative indexing, as the reference's dem[indices]
    if (k >= 0 && k < n) {
      h = z - dem[k];
      if (h < 0.0 && h != -100.0) h = 0.0;
    }
  }
  hand[i] = h;
}

// D2 + D3 downslope, downslope.py:435-532 + :161-314, heights in float64 (the walk of k_downslope in dt_kernels.hip)
__device__ __forceinline__ int64_t dw_step(int64_t pos, uint32_t code, int H, int W, bool &diag) {
  if (!dt_d8_valid(code)) return -1;
  int dy, dx;
  dt_d8_delta(code, dy, dx);
  const int y = (int)(pos / W), x = (int)(pos - (int64_t)y * W);
  const int ny = y + dy, nx = x + dx;
  if (ny < 0 || ny >= H || nx < 0 || nx >= W) return -2;
  diag = dy != 0 && dx != 0;
  return (int64_t)ny * W + nx;
}
__global__ __launch_bounds__(256) void k_downslope_f64(const double *__restrict__ dem, const uint8_t *__restrict__ fdr,
                                                      int H, int W, double px, double dz, int raw,
                                                      float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const double z0 = dem[i];
  if (!(z0 > -100.0 && z0 < __builtin_inf())) {  // downslope.py:460; NaN / +inf: NaN (DS_NONFINITE, dt_kernels.hip)
    out[i] = z0 <= -100.0 ? DT_NODATA : __builtin_nanf("");
    return;
  }
  const double dcard = px, ddiag = px * sqrt(2.0);
  int64_t pos = i;
  double dist = 0.0, drop = 0.0;
  int loop = 0;
  bool failed = false;
  while (drop < dz) {
    bool diag = false;
    const int64_t t = dw_step(pos, fdr[pos], H, W, diag);
    if (t == -2) { failed = true; break; }  // raster-edge exit: stop (downslope.py:209-228)
    if (t >= 0) {
      const double zt = dem[t];
      if (zt == -100.0) { failed = true; break; }  // nodata ahead: stop without moving (:231-281)
      pos = t;
      dist += diag ? ddiag : dcard;
      drop = z0 - zt;  // downslope.py:468, the DEM's own dtype
    }
    if (++loop == 5000) { failed = true; break; }  // :303-304 / :518-521
  }
  if (raw && failed) out[i] = -50.0f;
  else out[i] = dist == 0.0 ? 0.0f : (float)(drop / dist);
}

// G2 / G3 with a float64 HAND: ln(b * (A * size^2)^n / (hand + 0.01)), gfi.py:268-294 (A = fac[idx], no zero guard)
// and :404-440 (A = the cell's own fac, 0 -> 1)
__global__ __launch_bounds__(256) void k_gfi_f64h(const double *__restrict__ hand, const int64_t *__restrict__ fac,
                                                 const int64_t *__restrict__ idx, int64_t n, double expo, double b,
                                                 double size, int own_area, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double h = hand[i];
  if (h <= -100.0) {
    out[i] = DT_NODATA;
    return;
  }
  double a;
  if (own_area) {  // 1: the cell's own area with the zero guard of gfi.py:432; 2: an explicit area raster, no guard
    const int64_t f = fac[i];
    a = (f == 0 && own_area == 1) ? 1.0 * (size * size) : (double)f * (size * size);
  } else {
    int64_t k = idx[i];
    if (k == -100) k = 0;  // gfi.py:141-143: fac.flat[0]
    if (k < 0) k += n;     // numpy negative indexing
    a = (double)((k >= 0 && k < n) ? fac[k] : fac[0]) * (size * size);
  }
  out[i] = (float)log(b * pow(a, expo) / (h + 0.01));
}

// ---- the resident chain's float64 tier (chain.Chain(heights="float64")) ------------------------------------------
// D2 + D3 downslope staged like k_downslope_win: a workgroup owns a DWC x DWC core and stages heights (8 B) and codes
// (1 B) of the core plus a DWM-cell margin into LDS -- 88 x 88 x 9 B = 68 KiB, two workgroups per CU (160 KiB).  The
// float32 kernel's 24-cell margin (112 x 112) would take 98 KiB of doubles and leave one.  Each walk is the
// reference's literal loop (downslope.py:435-532 on float64 heights): the drop tested before each move, the float64 path length summed
// move by move -- no count form, so nothing needs a rounding test -- and a cell outside the window read from global
// memory instead of LDS, so walks that leave the window simply go on there.  A non-D8 code never moves again: the
// reference spins to its 5000-move cap with the same outcome, here the walk stops at once as failed.
#define DWC 64
#define DWM 12
#define DWS (DWC + 2 * DWM)
__global__ __launch_bounds__(1024) void k_downslope_win_f64(const double *__restrict__ dem,
                                                            const uint8_t *__restrict__ fdr, int H, int W, double px,
                                                            double dz, int raw, float *__restrict__ out) {
  __shared__ double sz[DWS * DWS];
  __shared__ uint8_t sc[DWS * DWS];
  const int cy0 = (int)blockIdx.y * DWC, cx0 = (int)blockIdx.x * DWC;
  const int wy0 = cy0 - DWM, wx0 = cx0 - DWM;
  // every load of a thread in flight before the first LDS store
  constexpr int NV = (DWS * DWS + 1023) / 1024;
  double vz[NV];
  uint32_t vc[NV];
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 1024 * u;
    const int r = i / DWS, c = i - r * DWS, gy = wy0 + r, gx = wx0 + c;
    const bool in = i < DWS * DWS && gy >= 0 && gy < H && gx >= 0 && gx < W;
    const long long g = (long long)gy * W + gx;
    vz[u] = in ? dem[g] : -100.0;
    vc[u] = in ? (uint32_t)fdr[g] : 0u;
  }
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 1024 * u;
    if (i < DWS * DWS) {
      sz[i] = vz[u];
      sc[i] = (uint8_t)vc[u];
    }
  }
  __syncthreads();
  const double dcard = px, ddiag = px * sqrt(2.0);
  for (int k = (int)threadIdx.x; k < DWC * DWC; k += 1024) {
    const int y0 = cy0 + k / DWC, x0 = cx0 + k % DWC;
    if (y0 >= H || x0 >= W) continue;
    const double z0 = sz[(y0 - wy0) * DWS + (x0 - wx0)];
    float res;
    if (z0 <= -100.0) {  // downslope.py:460
      res = DT_NODATA;
    } else if (!(z0 < __builtin_inf())) {  // NaN / +inf start: NaN (DS_NONFINITE, dt_kernels.hip)
      res = __builtin_nanf("");
    } else {
      int y = y0, x = x0, loop = 0;
      double dist = 0.0, drop = z0 - z0;
      bool failed = false;
      while (drop < dz) {
        const int ly = y - wy0, lx = x - wx0;
        const bool lds = ly >= 0 && ly < DWS && lx >= 0 && lx < DWS;
        const uint32_t code = lds ? sc[ly * DWS + lx] : fdr[(long long)y * W + x];
        if (!dt_d8_valid(code)) { failed = true; break; }  // spins to the cap in the reference
        int dy, dx;
        dt_d8_delta(code, dy, dx);
        const int ny = y + dy, nx = x + dx;
        if (ny < 0 || ny >= H || nx < 0 || nx >= W) { failed = true; break; }  // raster-edge exit (downslope.py:209-228)
        const int my = ny - wy0, mx = nx - wx0;
        const double zt = (my >= 0 && my < DWS && mx >= 0 && mx < DWS) ? sz[my * DWS + mx] : dem[(long long)ny * W + nx];
        if (zt == -100.0) { failed = true; break; }  // nodata ahead: stop without moving (:231-281)
        y = ny;
        x = nx;
        dist += (dy != 0 && dx != 0) ? ddiag : dcard;
        drop = z0 - zt;  // downslope.py:468, in the DEM's own dtype
        if (++loop == 5000) { failed = true; break; }  // :303-304 / :518-521
      }
      res = (raw && failed) ? -50.0f : (dist == 0.0 ? 0.0f : (float)(drop / dist));
    }
    out[(long long)y0 * W + x0] = res;
  }
}

// F4 HAND in float64 from the chain's int32 river index, and G2 / G3 (gfi.py:268-294 with A = fac[idx]; :404-440 with
// the cell's own fac, 0 -> 1) from that HAND: one pass, 16 B read + 16 B written per cell (the gather dem[idx] and
// fac[idx] hits the few river cells)
__global__ __launch_bounds__(256) void k_hand_gfi_f64(const double *__restrict__ dem, const int32_t *__restrict__ idx,
                                                     const int32_t *__restrict__ fac, int64_t n, double expo, double b,
                                                     double size, double *__restrict__ hand, float *__restrict__ gfi,
                                                     float *__restrict__ lnhlh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double z = dem[i];
  const int64_t k = idx[i];
  double h = -100.0;
  if (z != -100.0 && k != -100 && k >= 0 && k < n) {  // flowhand.py:436
    h = z - dem[k];
    if (h < 0.0 && h != -100.0) h = 0.0;  // :438
  }
  hand[i] = h;
  float g = DT_NODATA, l = DT_NODATA;
  if (!(h <= -100.0)) {
    const double s2 = size * size, a_r = (double)fac[k] * s2;
    const int32_t f = fac[i];
    const double a_o = f == 0 ? 1.0 * s2 : (double)f * s2;
    g = (float)log(b * pow(a_r, expo) / (h + 0.01));
    l = (float)log((b * pow(a_o, expo)) / (h + 0.01));
  }
  if (gfi) gfi[i] = g;
  if (lnhlh) lnhlh[i] = l;
}

int dt_launch_downslope_win_f64(hipStream_t s, const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                                double dz, int raw, float *out) {
  if (H == 0 || W == 0) return DT_OK;
  const dim3 g((unsigned)((W + DWC - 1) / DWC), (unsigned)((H + DWC - 1) / DWC));
  DT_REQUIRE(g.y < 65536u, "raster too tall for one launch");
  hipLaunchKernelGGL(k_downslope_win_f64, g, dim3(1024), 0, s, dem, fdr, (int)H, (int)W, px, dz, raw, out);
  return DT_OK;
}
int dt_launch_hand_gfi_f64(hipStream_t s, const double *dem, const int32_t *idx32, const int32_t *acc32, int64_t n,
                           double expo, double b, double size, double *hand, float *gfi, float *lnhlh) {
  if (n) hipLaunchKernelGGL(k_hand_gfi_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dem, idx32, acc32, n, expo,
                            b, size, hand, gfi, lnhlh);
  return DT_OK;
}

int dt_launch_slope_f64(hipStream_t s, const double *dem, int64_t H, int64_t W, double px, float *slope) {
  if (H * W == 0) return DT_OK;
  hipLaunchKernelGGL(k_slope_f64, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), dim3(256), 0, s, dem, (int)H,
                     (int)W, px, slope);
  return DT_OK;
}
int dt_launch_hand_f64(hipStream_t s, const double *dem, const int64_t *idx, int64_t n, double *hand) {
  if (n) hipLaunchKernelGGL(k_hand_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dem, idx, n, hand);
  return DT_OK;
}
int dt_launch_downslope_f64(hipStream_t s, const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                            double dz, int raw, float *out) {
  const int64_t n = H * W;
  if (n) hipLaunchKernelGGL(k_downslope_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dem, fdr, (int)H, (int)W,
                            px, dz, raw, out);
  return DT_OK;
}
int dt_launch_gfi_f64h(hipStream_t s, const double *hand, const int64_t *fac, const int64_t *idx, int64_t n,
                       double expo, double b, double size, int own_area, float *out) {
  if (n) hipLaunchKernelGGL(k_gfi_f64h, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, hand, fac, idx, n, expo, b,
                            size, own_area, out);
  return DT_OK;
}

// ---- the same on one rank's window of a larger raster (tiling.RankTile(heights="float64")) ------------------------
// Downslope on a window: k_downslope_win_f64's walk over the rank's memory (core + halo, row stride w.ld; pointers at
// the core origin).  The window semantics are dt_dev_downslope_w's: a walk that stands on a cell without a D8 code in
// this memory (its last ring; dt_has_code) or steps to a cell outside it is another rank's to finish -- marked -50 and
// counted in *n_unresolved (tiling.finish_downslope walks it on); only the GLOBAL raster's edge ends a walk as failed.
__global__ __launch_bounds__(1024) void k_downslope_win_f64_w(const double *__restrict__ dem,
                                                              const uint8_t *__restrict__ fdr, DtWin w, double px,
                                                              double dz, int raw, float *__restrict__ out,
                                                              int *__restrict__ n_unresolved) {
  __shared__ double sz[DWS * DWS];
  __shared__ uint8_t sc[DWS * DWS];
  const int cy0 = (int)blockIdx.y * DWC, cx0 = (int)blockIdx.x * DWC;
  const int wy0 = cy0 - DWM, wx0 = cx0 - DWM;
  constexpr int NV = (DWS * DWS + 1023) / 1024;
  double vz[NV];
  uint32_t vc[NV];
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 1024 * u;
    const int r = i / DWS, c = i - r * DWS, y = wy0 + r, x = wx0 + c;
    const bool in = i < DWS * DWS && dt_readable(w, y, x);
    const long long g = (long long)y * w.ld + x;
    vz[u] = in ? dem[g] : -100.0;
    vc[u] = (in && dt_has_code(w, y, x)) ? (uint32_t)fdr[g] : 0u;
  }
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = (int)threadIdx.x + 1024 * u;
    if (i < DWS * DWS) {
      sz[i] = vz[u];
      sc[i] = (uint8_t)vc[u];
    }
  }
  __syncthreads();
  const double dcard = px, ddiag = px * sqrt(2.0);
  uint32_t unres = 0u;
  for (int k = (int)threadIdx.x; k < DWC * DWC; k += 1024) {
    const int y0 = cy0 + k / DWC, x0 = cx0 + k % DWC;
    if (y0 >= w.H || x0 >= w.W) continue;
    const double z0 = sz[(y0 - wy0) * DWS + (x0 - wx0)];
    float res;
    if (z0 <= -100.0) {  // downslope.py:460
      res = DT_NODATA;
    } else if (!(z0 < __builtin_inf())) {  // NaN / +inf start: NaN (DS_NONFINITE, dt_kernels.hip)
      res = __builtin_nanf("");
    } else {
      int y = y0, x = x0, loop = 0;
      double dist = 0.0, drop = z0 - z0;
      bool failed = false, unresolved = false;
      while (drop < dz) {
        if (!dt_has_code(w, y, x)) { unresolved = true; break; }  // the end of this rank's memory
        const int ly = y - wy0, lx = x - wx0;
        const bool lds = ly >= 0 && ly < DWS && lx >= 0 && lx < DWS;
        const uint32_t code = lds ? sc[ly * DWS + lx] : fdr[(long long)y * w.ld + x];
        if (!dt_d8_valid(code)) { failed = true; break; }  // spins to the cap in the reference
        int dy, dx;
        dt_d8_delta(code, dy, dx);
        const int ny = y + dy, nx = x + dx;
        if (!dt_in_global(w, ny, nx)) { failed = true; break; }  // raster-edge exit (downslope.py:209-228)
        if (!dt_readable(w, ny, nx)) { unresolved = true; break; }
        const int my = ny - wy0, mx = nx - wx0;
        const double zt = (my >= 0 && my < DWS && mx >= 0 && mx < DWS) ? sz[my * DWS + mx]
                                                                         : dem[(long long)ny * w.ld + nx];
        if (zt == -100.0) { failed = true; break; }  // nodata ahead: stop without moving (:231-281)
        y = ny;
        x = nx;
        dist += (dy != 0 && dx != 0) ? ddiag : dcard;
        drop = z0 - zt;  // downslope.py:468, in the DEM's own dtype
        if (++loop == 5000) { failed = true; break; }  // :303-304 / :518-521
      }
      if (unresolved) {
        res = -50.0f;
        unres++;
      } else {
        res = (raw && failed) ? -50.0f : (dist == 0.0 ? 0.0f : (float)(drop / dist));
      }
    }
    out[(long long)y0 * w.ld + x0] = res;
  }
  for (int o = 32; o; o >>= 1) unres += (uint32_t)__shfl_xor((int)unres, o);
  if ((threadIdx.x & 63u) == 0u && unres && n_unresolved) atomicAdd(n_unresolved, (int)unres);
}

// The float64 river height of every HAND summary entry that ends on a river cell of this rank (kind 1, ref = core-local
// flat index), -100 otherwise: the field the rank-level solve hands to the ranks whose paths end there
__global__ __launch_bounds__(256) void k_fh_zr64_w(const double *__restrict__ dem, DtWin w, int64_t n,
                                                  const uint8_t *__restrict__ kind, const int32_t *__restrict__ ref,
                                                  double *__restrict__ zr64) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double z = -100.0;
  if (kind[i] == 1u) {
    const int r = ref[i];
    if (r >= 0 && r < w.H * w.W) z = dem[(long long)(r / w.W) * w.ld + r % w.W];
  }
  zr64[i] = z;
}

// River cells on other ranks: an open-addressing table (global flat index -> float64 height) built from the rank-level
// solve's results -- at most one entry per ring cell, a power of two of at least twice as many slots, so every probe
// sequence ends on an empty slot
#define RT_EMPTY 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ uint32_t rt_slot(unsigned long long k, uint32_t mask) {
  return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}
__global__ __launch_bounds__(256) void k_rt_build(int64_t n, const uint8_t *__restrict__ res_ok,
                                                 const int64_t *__restrict__ gidx, const double *__restrict__ zr64,
                                                 uint32_t mask, unsigned long long *__restrict__ keys,
                                                 double *__restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !res_ok[i] || gidx[i] < 0) return;
  const unsigned long long k = (unsigned long long)gidx[i];
  uint32_t s = rt_slot(k, mask);
  for (uint32_t p = 0; p <= mask; p++) {
    const unsigned long long prev = atomicCAS(&keys[s], RT_EMPTY, k);
    if (prev == RT_EMPTY || prev == k) {
      vals[s] = zr64[i];  // every entry of one river cell carries the same height
      return;
    }
    s = (s + 1u) & mask;
  }
}
__device__ __forceinline__ double rt_find(const unsigned long long *__restrict__ keys, const double *__restrict__ vals,
                                          uint32_t mask, unsigned long long k) {
  uint32_t s = rt_slot(k, mask);
  for (uint32_t p = 0; p <= mask; p++) {
    const unsigned long long e = keys[s];
    if (e == k) return vals[s];
    if (e == RT_EMPTY) break;
    s = (s + 1u) & mask;
  }
  return __builtin_nan("");  // (no such path: every remote river index came through the table)
}

// k_hand_gfi_f64 on a window: idx holds GLOBAL flat indices (int32 or int64); the river cell's height is read from the
// rank's memory when it lies there, from the table otherwise; GFI's area is the river-accumulation payload a_river
// (the river cell's accumulation, carried across ranks by the HAND summaries), the cell's own accumulation ln(hl/H)'s
__device__ __forceinline__ int64_t hg_idx(const int32_t *i32, const int64_t *i64, long long o) {
  return i64 ? i64[o] : (int64_t)i32[o];
}
template <typename AccT>
__global__ __launch_bounds__(256) void k_hand_gfi_f64_w(const double *__restrict__ dem, DtWin w,
                                                       const int32_t *__restrict__ idx32,
                                                       const int64_t *__restrict__ idx64, const AccT *__restrict__ fac,
                                                       const AccT *__restrict__ a_river,
                                                       const unsigned long long *__restrict__ keys,
                                                       const double *__restrict__ vals, uint32_t mask, double expo,
                                                       double b, double size, double *__restrict__ hand,
                                                       float *__restrict__ gfi, float *__restrict__ lnhlh) {
  const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
  const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
  if (x >= w.W || y >= w.H) return;
  const long long o = (long long)y * w.ld + x;
  const int64_t n = (int64_t)w.Hg * w.Wg;
  const double z = dem[o];
  const int64_t k = hg_idx(idx32, idx64, o);
  double h = -100.0;
  if (z != -100.0 && k != -100 && k >= 0 && k < n) {  // flowhand.py:436
    const int gy = (int)(k / w.Wg), gx = (int)(k - (int64_t)gy * w.Wg);
    const int ly = gy - w.gy0, lx = gx - w.gx0;
    const double zr = dt_readable(w, ly, lx) ? dem[(long long)ly * w.ld + lx] : rt_find(keys, vals, mask, (unsigned long long)k);
    h = z - zr;
    if (h < 0.0 && h != -100.0) h = 0.0;  // :438
  }
  hand[o] = h;
  float g = DT_NODATA, l = DT_NODATA;
  if (!(h <= -100.0)) {
    const double s2 = size * size, a_r = (double)a_river[o] * s2;
    const AccT f = fac[o];
    const double a_o = f == 0 ? 1.0 * s2 : (double)f * s2;
    g = (float)log(b * pow(a_r, expo) / (h + 0.01));
    l = (float)log((b * pow(a_o, expo)) / (h + 0.01));
  }
  if (gfi) gfi[o] = g;
  if (lnhlh) lnhlh[o] = l;
}

int dt_launch_downslope_win_f64_w(hipStream_t s, const DtWin &w, const double *dem, const uint8_t *fdr, double px,
                                  double dz, int raw, float *out, int *n_unresolved) {
  if (w.H == 0 || w.W == 0) return DT_OK;
  const dim3 g((unsigned)((w.W + DWC - 1) / DWC), (unsigned)((w.H + DWC - 1) / DWC));
  DT_REQUIRE(g.y < 65536u, "window too tall for one launch");
  hipLaunchKernelGGL(k_downslope_win_f64_w, g, dim3(1024), 0, s, dem, fdr, w, px, dz, raw, out, n_unresolved);
  return DT_OK;
}
int dt_launch_fh_zr64_w(hipStream_t s, const DtWin &w, const double *dem, int64_t n, const uint8_t *kind,
                        const int32_t *ref, double *zr64) {
  if (n > 0)
    hipLaunchKernelGGL(k_fh_zr64_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dem, w, n, kind, ref, zr64);
  return DT_OK;
}
int64_t dt_hand_f64_table_slots(int64_t n_remote) {
  int64_t c = 64;
  while (c < 2 * n_remote) c <<= 1;
  return c;
}
int dt_launch_hand_gfi_f64_w(hipStream_t s, const DtWin &w, const double *dem, const int32_t *idx32,
                             const int64_t *idx64, const void *fac, const void *a_river, int acc64, int64_t n_remote,
                             const uint8_t *res_ok, const int64_t *rem_gidx, const double *rem_zr64, void *table,
                             double expo, double b, double size, double *hand, float *gfi, float *lnhlh) {
  const int64_t slots = dt_hand_f64_table_slots(n_remote);
  unsigned long long *keys = (unsigned long long *)table;
  double *vals = (double *)(keys + slots);
  const uint32_t mask = (uint32_t)(slots - 1);
  DT_HIP(hipMemsetAsync(keys, 0xFF, (size_t)slots * 8, s));
  if (n_remote > 0 && res_ok)
    hipLaunchKernelGGL(k_rt_build, dim3((unsigned)((n_remote + 255) / 256)), dim3(256), 0, s, n_remote, res_ok,
                       rem_gidx, rem_zr64, mask, keys, vals);
  if (w.H == 0 || w.W == 0) return DT_OK;
  const dim3 g((unsigned)((w.W + 63) / 64), (unsigned)((w.H + 3) / 4));
  DT_REQUIRE(g.y < 65536u, "window too tall for one launch");
  if (acc64)
    hipLaunchKernelGGL(k_hand_gfi_f64_w<int64_t>, g, dim3(256), 0, s, dem, w, idx32, idx64, (const int64_t *)fac,
                       (const int64_t *)a_river, keys, vals, mask, expo, b, size, hand, gfi, lnhlh);
  else
    hipLaunchKernelGGL(k_hand_gfi_f64_w<int32_t>, g, dim3(256), 0, s, dem, w, idx32, idx64, (const int32_t *)fac,
                       (const int32_t *)a_river, keys, vals, mask, expo, b, size, hand, gfi, lnhlh);
  return DT_OK;
}
