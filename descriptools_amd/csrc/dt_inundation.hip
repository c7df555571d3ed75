// dt_inundation.hip -- local-inertial 2-D flood inundation (Bates, Horritt & Fewtrell 2010) on float64 state.
// descriptools_amd/inundation.py holds the scheme and its association; every expression here is written in that
// association and the library is built with -ffp-contract=off, so the state is the numpy reference's bit for bit.
//
// One step is two launches.  k_in_step: one pass over the state in tiles of 64 x 16 cells with a two-cell halo in LDS
// (the limiter makes a cell's update depend on depths two cells away): depths, heights and roughness into LDS, the
// candidate flux of every face of the tile and its first halo ring, the limiter ratio r of every cell of the tile and
// that ring, then the final fluxes and the new depth of the tile's own cells into the OTHER copy of the state
// (neighbours read the old one).  k_in_close: one workgroup that adds the inflow hydrograph's cells, closes the step's
// book-keeping and computes the next step's dt.
//
// The control block (DT_IN_CTL words of 8 bytes on the device).  k_in_step only READS words 0-5 and only ACCUMULATES
// (integer atomic max / or, never reading them) into words 10-11; k_in_close, a single workgroup, is the only writer of
// words 0-9 and 12 and the only reader of 10-11, which it zeroes.  So no workgroup reads a word that another
// workgroup writes in the same launch, and a launch boundary is the only cross-workgroup ordering there is.  Which
// copy of the state is current is word 4's parity (the steps taken in this call): a step enqueued after the end
// returns at once and moves nothing, so the host may enqueue any number of them.
#include "dt_common.h"
#include "dt_kernels.h"

#include <math.h>

namespace {

constexpr int IN_TX = 64, IN_TY = 16;
constexpr int IN_LW = IN_TX + 4, IN_LH = IN_TY + 4, IN_LN = IN_LW * IN_LH;
constexpr double IN_G = 9.80665;
typedef unsigned long long u64;

enum { C_T = 0, C_DT, C_TNEW, C_DONE, C_K, C_STEPS, C_DTMIN, C_DTLAST, C_LIMITED, C_HMAX, C_ACC_HMAX, C_ACC_LIM,
       C_FINISHED };

struct InArgs {
  const float *z, *nr, *rr;
  double *h[2], *qx[2], *qy[2];
  double *md, *arr;
  u64 *ctl;
  int H, W;
  double px, n, rain, dry, sqrt_s, ad;
  int open;
};
struct InClose {
  double t_end, dt_max, alpha;
  long long max_steps;
  const int64_t *cells;
  const double *times, *q;
  int K, T;
};

struct InWs {
  double *h, *qx, *qy;
  u64 *ctl;
  size_t bytes;
};
InWs in_layout(void *scratch, int64_t n) {
  DtCarver c(scratch);
  InWs w;
  w.h = c.take<double>((size_t)n);
  w.qx = c.take<double>((size_t)n);
  w.qy = c.take<double>((size_t)n);
  w.ctl = c.take<u64>(DT_IN_CTL);
  w.bytes = c.bytes();
  return w;
}

__device__ __forceinline__ double in_f(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 in_b(double v) { return (u64)__double_as_longlong(v); }

// the cube root of x > 0 by the stated sequence (inundation.py): only exact scalings and float64 + - * /
__device__ __forceinline__ double in_cbrt3(double x) {
  int e;
  const double f = frexp(x, &e);
  int k = e / 3;
  if (e - 3 * k < 0) k--;  // floor
  const double m = ldexp(f, e - 3 * k);
  double y = (0.6 + 0.35 * m) - 0.03 * (m * m);
#pragma unroll
  for (int i = 0; i < 4; i++) y = ((2.0 * y) + m / (y * y)) / 3.0;
  return ldexp(y, k);
}

// step 2: the candidate flux on the face between valid cells a (west / north) and b
__device__ __forceinline__ double in_face(double q, double za, double zb, double ha, double hb, double na, double nb,
                                          double dt, double px, double dry) {
  const double ea = za + ha, eb = zb + hb;
  const double hf = fmax(ea, eb) - fmax(za, zb);
  if (!(hf > dry)) return 0.0;
  const double num = q - ((IN_G * hf) * dt) * ((eb - ea) / px);
  const double nf = 0.5 * (na + nb);
  const double den = 1.0 + (((IN_G * dt) * (nf * nf)) * fabs(q)) / ((hf * hf) * in_cbrt3(hf));
  return num / den;
}

// step 3: what leaves a valid cell over the raster's edge at normal depth
__device__ __forceinline__ double in_edge_loss(const InArgs &a, double h, double n, int gy, int gx) {
  if (!a.open || !(h > a.dry)) return 0.0;
  const int s = (gy == 0) + (gy == a.H - 1) + (gx == 0) + (gx == a.W - 1);
  if (s == 0) return 0.0;
  const double c = in_cbrt3(h);
  return (double)s * ((((h * c) * c) * a.sqrt_s) / n);
}

// the largest of one value per thread (bit patterns of non-negative doubles), valid in thread 0
__device__ __forceinline__ u64 in_block_max(u64 v, u64 *s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = (u64)__shfl_xor((long long)v, o);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63u) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < 4; k++) v = s_red[k] > v ? s_red[k] : v;
  return v;
}

// the largest depth of the state the call starts from
__global__ __launch_bounds__(256) void k_in_hmax(InArgs a, int64_t n) {
  __shared__ u64 s_red[4];
  u64 v = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float z = a.z[i];
    if (z == z) {
      const u64 b = in_b(a.h[0][i]);
      v = b > v ? b : v;
    }
  }
  v = in_block_max(v, s_red);
  if (threadIdx.x == 0 && v) atomicMax(&a.ctl[C_ACC_HMAX], v);
}

constexpr int IN_ROUNDS = (IN_LN + 255) / 256;  // LDS cells per thread
constexpr int IN_OWN = IN_TX * IN_TY / 256;     // tile cells per thread
constexpr int IN_NX = (IN_LH - 2) * (IN_LW - 1), IN_NY = (IN_LH - 1) * (IN_LW - 2);  // faces with a candidate
constexpr int IN_FACE_ROUNDS = (IN_NX + IN_NY + 255) / 256;

// NRAS: Manning's n is a raster (and then sits in LDS beside the heights)
template <bool NRAS>
__global__ __launch_bounds__(256) void k_in_step(InArgs a, int tiles_x) {
  // s_hr: the depth until the candidate fluxes are in, the limiter ratio from then on (a thread keeps the depth of its
  // own cells in registers); s_qx / s_qy: the old flux, then the candidate in its place
  __shared__ double s_hr[IN_LN], s_qx[IN_LN], s_qy[IN_LN];
  __shared__ float s_z[IN_LN], s_n[NRAS ? IN_LN : 1];
  __shared__ u64 s_red[4];
  const u64 *ctl = a.ctl;
  if (ctl[C_DONE]) return;
  const double dt = in_f(ctl[C_DT]), tnew = in_f(ctl[C_TNEW]);
  const int p = (int)(ctl[C_K] & 1ull);
  const double *__restrict__ h0 = a.h[p], *__restrict__ qx0 = a.qx[p], *__restrict__ qy0 = a.qy[p];
  double *__restrict__ h1 = a.h[1 - p], *__restrict__ qx1 = a.qx[1 - p], *__restrict__ qy1 = a.qy[1 - p];
  const int H = a.H, W = a.W;
  const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * IN_TY, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * IN_TX;
  const int tid = (int)threadIdx.x;

  // Every global read of the step, issued before the first wait: the tile and two rings around it.  A cell outside
  // the raster or without a height is a wall (z = NaN, h = 0).  The old fluxes are read where a candidate is wanted:
  // the east faces of rows 1 .. LH-2 and the south faces of columns 1 .. LW-2 (what the limiter of the tile and its
  // first ring reads).
#pragma unroll
  for (int k = 0; k < IN_ROUNDS; k++) {
    const int i = tid + 256 * k;
    if (i >= IN_LN) break;
    const int ly = i / IN_LW, lx = i - ly * IN_LW;
    const int gy = ty0 - 2 + ly, gx = tx0 - 2 + lx;
    float z = __int_as_float(0x7fc00000), n = 1.0f;
    double h = 0.0, qx = 0.0, qy = 0.0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int64_t g = (int64_t)gy * W + gx;
      z = a.z[g];
      h = h0[g];
      if (lx + 1 < IN_LW && ly >= 1 && ly <= IN_LH - 2) qx = qx0[g];
      if (ly + 1 < IN_LH && lx >= 1 && lx <= IN_LW - 2) qy = qy0[g];
      if (NRAS) n = a.nr[g];
      if (!(z == z)) h = 0.0;
    }
    s_z[i] = z;
    s_hr[i] = h;
    s_qx[i] = qx;
    s_qy[i] = qy;
    if (NRAS) s_n[i] = n;
  }
  __syncthreads();

  // candidate fluxes, in place of the old ones; a face to a wall holds 0.  One face per thread and round: the east
  // faces of rows 1 .. LH-2 first, then the south faces of columns 1 .. LW-2
#pragma unroll
  for (int k = 0; k < IN_FACE_ROUNDS; k++) {
    const int t = tid + 256 * k;
    if (t >= IN_NX + IN_NY) break;
    const bool east = t < IN_NX;
    const int u = east ? t : t - IN_NX, per = east ? IN_LW - 1 : IN_LW - 2;
    const int row = u / per, col = u - row * per;
    const int i = east ? (row + 1) * IN_LW + col : row * IN_LW + col + 1;
    const int j = east ? i + 1 : i + IN_LW;
    double *sq = east ? s_qx : s_qy;
    const float za = s_z[i], zb = s_z[j];
    double f = 0.0;
    if (za == za && zb == zb)
      f = in_face(sq[i], (double)za, (double)zb, s_hr[i], s_hr[j], NRAS ? (double)s_n[i] : a.n,
                  NRAS ? (double)s_n[j] : a.n, dt, a.px, a.dry);
    sq[i] = f;  // (a slot is read and written by its own thread only)
  }
  double own[IN_OWN];  // the depth of the thread's own cells, before the ratios take its place
#pragma unroll
  for (int j = 0; j < IN_OWN; j++) {
    const int c = tid + 256 * j;
    own[j] = s_hr[(c / IN_TX + 2) * IN_LW + (c % IN_TX) + 2];
  }
  __syncthreads();

  // the limiter ratio of the tile's cells and of the first ring, in place of the depth
  int limited = 0;
#pragma unroll
  for (int k = 0; k < IN_ROUNDS; k++) {
    const int i = tid + 256 * k;
    if (i >= IN_LN) break;
    const int ly = i / IN_LW, lx = i - ly * IN_LW;
    if (ly < 1 || ly > IN_LH - 2 || lx < 1 || lx > IN_LW - 2) continue;
    double r = 1.0;
    if (s_z[i] == s_z[i]) {
      const double h = s_hr[i];
      const double eo = in_edge_loss(a, h, NRAS ? (double)s_n[i] : a.n, ty0 - 2 + ly, tx0 - 2 + lx);
      const double out =
          (((fmax(-s_qy[i - IN_LW], 0.0) + fmax(-s_qx[i - 1], 0.0)) + fmax(s_qx[i], 0.0)) + fmax(s_qy[i], 0.0)) + eo;
      if (dt * out > h * a.px) {
        r = (h * a.px) / (dt * out);
        limited |= (ly >= 2 && ly < IN_LH - 2 && lx >= 2 && lx < IN_LW - 2);
      }
    }
    s_hr[i] = r;
  }
  limited = __syncthreads_or(limited);

  // final fluxes and the new depth of the tile's own cells
  u64 top = 0;
#pragma unroll
  for (int j = 0; j < IN_OWN; j++) {
    const int c = tid + 256 * j;
    const int cy = c / IN_TX, cx = c - cy * IN_TX;
    const int gy = ty0 + cy, gx = tx0 + cx;
    if (gy >= H || gx >= W) continue;
    const int i = (cy + 2) * IN_LW + cx + 2;
    const int64_t g = (int64_t)gy * W + gx;
    double hn = 0.0, qe = 0.0, qs = 0.0;
    const bool valid = s_z[i] == s_z[i];
    if (valid) {
      const double h = own[j], r = s_hr[i];
      const double se = s_qx[i], ss = s_qy[i], sw = s_qx[i - 1], sn = s_qy[i - IN_LW];
      qe = se * (se > 0.0 ? r : s_hr[i + 1]);
      qs = ss * (ss > 0.0 ? r : s_hr[i + IN_LW]);
      const double qw = sw * (sw > 0.0 ? s_hr[i - 1] : r);
      const double qn = sn * (sn > 0.0 ? s_hr[i - IN_LW] : r);
      const double eo = in_edge_loss(a, h, NRAS ? (double)s_n[i] : a.n, gy, gx);
      const double rain = a.rr ? (double)a.rr[g] : a.rain;
      hn = fmax(0.0, h + dt * (((((qn - qs) + (qw - qe)) - eo * r) / a.px) + rain));
    }
    h1[g] = hn;
    qx1[g] = qe;
    qy1[g] = qs;
    if (valid) {
      if (a.md) {
        const double m = a.md[g];
        if (hn > m) a.md[g] = hn;
      }
      if (a.arr && hn > a.ad) {
        const double t = a.arr[g];
        if (t != t) a.arr[g] = tnew;
      }
      const u64 b = in_b(hn);
      top = b > top ? b : top;
    }
  }
  top = in_block_max(top, s_red);
  if (tid == 0) {
    if (top) atomicMax(&a.ctl[C_ACC_HMAX], top);
    if (limited) atomicOr(&a.ctl[C_ACC_LIM], 1ull);
  }
}

// One workgroup.  first: opens the call (t0, steps0; the accumulated word holds the start state's largest depth).
// Otherwise closes the step just taken: the inflow cells gain (Q(t) dt) / (px px) with Q linear in the table at the
// step's start time, the counters move on, and the next step's dt is set.
__global__ __launch_bounds__(256) void k_in_close(InArgs a, InClose c, int first, double t0, long long steps0) {
  __shared__ u64 s_red[4];
  u64 *ctl = a.ctl;
  const u64 done = ctl[C_DONE];
  if (!first && done) return;
  double t = first ? t0 : in_f(ctl[C_T]);
  const double dt = in_f(ctl[C_DT]), tnew = in_f(ctl[C_TNEW]);
  const u64 k0 = first ? 0ull : ctl[C_K];
  u64 top = 0;
  if (!first && c.K > 0) {
    double *h1 = a.h[1 - (int)(k0 & 1ull)];
    int seg = 0;  // the number of table times <= t
    {
      int lo = 0, hi = c.T;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c.times[mid] <= t) lo = mid + 1; else hi = mid;
      }
      seg = lo;
    }
    for (int j = (int)threadIdx.x; j < c.K; j += 256) {
      const double *q = c.q + (size_t)j * c.T;
      double Q;
      if (seg == 0) Q = q[0];
      else if (seg == c.T) Q = q[c.T - 1];
      else {
        const double ta = c.times[seg - 1], tb = c.times[seg];
        Q = q[seg - 1] + (q[seg] - q[seg - 1]) * ((t - ta) / (tb - ta));
      }
      const int64_t g = c.cells[j];
      if (g < 0 || g >= (int64_t)a.H * a.W) continue;
      const double h = h1[g] + (Q * dt) / (a.px * a.px);
      h1[g] = h;
      if (a.md && h > a.md[g]) a.md[g] = h;
      if (a.arr && h > a.ad) {
        const double ta = a.arr[g];
        if (ta != ta) a.arr[g] = tnew;
      }
      const u64 b = in_b(h);
      top = b > top ? b : top;
    }
  }
  top = in_block_max(top, s_red);
  if (threadIdx.x != 0) return;
  u64 k = k0, steps = first ? (u64)steps0 : ctl[C_STEPS], limited = first ? 0ull : ctl[C_LIMITED];
  double dt_min = first ? 0.0 : in_f(ctl[C_DTMIN]), dt_last = first ? 0.0 : in_f(ctl[C_DTLAST]);
  const u64 acc = ctl[C_ACC_HMAX];
  if (!first) {
    dt_min = k == 0 ? dt : fmin(dt_min, dt);
    dt_last = dt;
    limited += ctl[C_ACC_LIM] ? 1ull : 0ull;
    k++;
    steps++;
    t = tnew;
  }
  const double hmax = in_f(acc > top ? acc : top);
  const bool finished = !(t < c.t_end);
  const bool stop = finished || (c.max_steps >= 0 && (long long)k >= c.max_steps);
  double dn = 0.0, tn = t;
  if (!stop) {
    // step 1
    dn = hmax <= 0.0 ? c.dt_max : fmin(c.dt_max, (c.alpha * a.px) / sqrt(IN_G * hmax));
    const double rem = c.t_end - t;
    const bool last = dn >= rem;
    if (last) dn = rem;
    tn = last ? c.t_end : t + dn;
  }
  ctl[C_T] = in_b(t);
  ctl[C_DT] = in_b(dn);
  ctl[C_TNEW] = in_b(tn);
  ctl[C_DONE] = stop ? 1ull : 0ull;
  ctl[C_K] = k;
  ctl[C_STEPS] = steps;
  ctl[C_DTMIN] = in_b(dt_min);
  ctl[C_DTLAST] = in_b(dt_last);
  ctl[C_LIMITED] = limited;
  ctl[C_HMAX] = in_b(hmax);
  ctl[C_ACC_HMAX] = 0ull;
  ctl[C_ACC_LIM] = 0ull;
  ctl[C_FINISHED] = finished ? 1ull : 0ull;
}

// the state back into the caller's rasters when an odd number of steps left it in the second copy; the info words
__global__ __launch_bounds__(256) void k_in_finish(InArgs a, int64_t n, int64_t *info) {
  const u64 *ctl = a.ctl;
  if (ctl[C_K] & 1ull) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      a.h[0][i] = a.h[1][i];
      a.qx[0][i] = a.qx[1][i];
      a.qy[0][i] = a.qy[1][i];
    }
  }
  if (info && blockIdx.x == 0 && threadIdx.x == 0) {
    info[0] = (int64_t)ctl[C_STEPS];
    info[1] = (int64_t)ctl[C_K];
    info[2] = (int64_t)ctl[C_T];
    info[3] = (int64_t)ctl[C_DTMIN];
    info[4] = (int64_t)ctl[C_DTLAST];
    info[5] = (int64_t)ctl[C_HMAX];
    info[6] = (int64_t)ctl[C_LIMITED];
    info[7] = (int64_t)ctl[C_FINISHED];
  }
}

InArgs in_args(const DtInundation &d, const InWs &w) {
  InArgs a;
  a.z = d.z; a.nr = d.manning; a.rr = d.rain;
  a.h[0] = d.h; a.h[1] = w.h;
  a.qx[0] = d.qx; a.qx[1] = w.qx;
  a.qy[0] = d.qy; a.qy[1] = w.qy;
  a.md = d.max_depth; a.arr = d.arrival;
  a.ctl = w.ctl;
  a.H = (int)d.H; a.W = (int)d.W;
  a.px = d.px; a.n = d.n; a.rain = d.rain_s; a.dry = d.dry; a.sqrt_s = sqrt(d.slope); a.ad = d.arrival_depth;
  a.open = d.open;
  return a;
}
InClose in_close(const DtInundation &d) {
  InClose c;
  c.t_end = d.t_end; c.dt_max = d.dt_max; c.alpha = d.alpha; c.max_steps = d.max_steps;
  c.cells = d.cells; c.times = d.times; c.q = d.discharge;
  c.K = d.K; c.T = d.T;
  return c;
}
int in_ws(const DtInundation &d, void *scratch, size_t scratch_bytes, InWs *w) {
  DT_REQUIRE(d.H > 0 && d.W > 0 && d.H * d.W < (1ll << 31), "raster of no cells, or of 2^31 or more");
  *w = in_layout(scratch, d.H * d.W);
  DT_REQUIRE(scratch && scratch_bytes >= w->bytes, "scratch too small");
  return DT_OK;
}

}  // namespace

size_t dt_inundation_scratch(int64_t H, int64_t W) { return in_layout(nullptr, H * W).bytes; }
const unsigned long long *dt_inundation_ctl(void *scratch, int64_t H, int64_t W) {
  return in_layout(scratch, H * W).ctl;
}

int dt_launch_inundation_begin(hipStream_t s, const DtInundation &d, double t0, int64_t steps0, void *scratch,
                               size_t scratch_bytes) {
  InWs w;
  DT_TRY(in_ws(d, scratch, scratch_bytes, &w));
  const InArgs a = in_args(d, w);
  const int64_t n = d.H * d.W;
  DT_HIP(hipMemsetAsync(w.ctl, 0, sizeof(u64) * DT_IN_CTL, s));
  hipLaunchKernelGGL(k_in_hmax, dim3(dt_capped_grid(n, 4096)), dim3(256), 0, s, a, n);
  hipLaunchKernelGGL(k_in_close, dim3(1), dim3(256), 0, s, a, in_close(d), 1, t0, (long long)steps0);
  return DT_OK;
}

int dt_launch_inundation_steps(hipStream_t s, const DtInundation &d, int steps, void *scratch, size_t scratch_bytes) {
  InWs w;
  DT_TRY(in_ws(d, scratch, scratch_bytes, &w));
  const InArgs a = in_args(d, w);
  const InClose c = in_close(d);
  const int64_t tx = (d.W + IN_TX - 1) / IN_TX, ty = (d.H + IN_TY - 1) / IN_TY;
  for (int i = 0; i < steps; i++) {
    if (a.nr) hipLaunchKernelGGL(k_in_step<true>, dim3((unsigned)(tx * ty)), dim3(256), 0, s, a, (int)tx);
    else hipLaunchKernelGGL(k_in_step<false>, dim3((unsigned)(tx * ty)), dim3(256), 0, s, a, (int)tx);
    hipLaunchKernelGGL(k_in_close, dim3(1), dim3(256), 0, s, a, c, 0, 0.0, 0ll);
  }
  return DT_OK;
}

int dt_launch_inundation_finish(hipStream_t s, const DtInundation &d, void *scratch, size_t scratch_bytes,
                                int64_t *info) {
  InWs w;
  DT_TRY(in_ws(d, scratch, scratch_bytes, &w));
  const int64_t n = d.H * d.W;
  hipLaunchKernelGGL(k_in_finish, dim3(dt_capped_grid(n, 8192)), dim3(256), 0, s, in_args(d, w), n, info);
  return DT_OK;
}
