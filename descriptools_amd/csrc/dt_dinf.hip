// dt_dinf.hip -- D-infinity flow direction and contributing area (Tarboton 1997; net-new, descriptools_amd/dinf.py
// holds the definition).
//
// Direction (k_dinf): a 3 x 3 stencil on an LDS tile of 128 x 8 cells with a one-cell halo, four cells per lane.  The
// eight triangular facets are evaluated in float64 on the float32 heights; the facet of steepest descent is chosen on
// its slope alone (strict >, the first facet wins a tie), so the one atan2 of a cell is taken after the choice, on the
// winning facet.  A neighbour takes part when it is finite and > -100; everything outside the raster is staged as
// -100.  A valid centre without a winning facet takes the caller's D8 code (when that neighbour is valid) or -1.
//
// Accumulation: the in-degree countdown of dt_countdown.h (the protocol is written out there) on a DAG of out-degree
// <= 2.  The word's own flags: 61, 62 the edge to the first / second receiver exists (the receiver lies in the raster
// and is not nodata).
// k_di_init   gathers each cell's in-degree from the eight neighbours' angles (LDS tile of angles, no atomics).
// k_di_flow   a complete cell sends m2 = floor(T * P2 / 2^30) to the second receiver and T - m2 to the first.  A lane
//             that completes both receivers keeps one and puts the other on a STACK of DI_STACK cells in LDS (last in,
//             first out: it follows one branch to its end), and when that is full on the queue.  A start walks at most
//             DI_MOVES = 128 cells in a round: while one lane follows a channel of tens of thousands of cells
//             everything queued behind it would wait (measured: DESIGN.md 4.11).  The receivers' angles are asked for
//             beside the atomics.
// k_di_out    nodata is read from the angle raster.
// The three are templates on dt_countdown.h's transfer mode: CD_T_NONE is the accumulation (no parameter raster is
// read), the others are routing.py's decay / retain / limit, which split O = cd_transfer(T) and write up to four rasters.
#include <cmath>

#include "dt_countdown.h"
#include "dt_dinf_common.h"

#define DI_F_E0 (1ull << 61)
#define DI_F_E1 (1ull << 62)
#define DI_MOVES 128  // cells one start (a source, a queue entry) may complete in a round before it hands on

// ---- direction -----------------------------------------------------------------------------------------------------
// one cell: e0 and its neighbours by octant; code = the caller's D8 code (0 without one)
__device__ __forceinline__ void di_cell(float c, const float (&n)[8], double px, double pxd, uint32_t code,
                                        float &angle, float &slope) {
  if (c <= DT_NODATA) {
    angle = DT_NODATA;
    slope = DT_NODATA;
    return;
  }
  angle = -1.0f;
  slope = 0.0f;
  if (!di_valid(c)) return;  // NaN, +inf: no flow
  const double e0 = (double)c;
  double best = 0.0, bs1 = 0.0, bs2 = 0.0;
  int bf = -1, bmode = 0;
#pragma unroll
  for (int f = 0; f < 8; f++) {
    const int o1 = ((f + 1) >> 1 << 1) & 7;  // E N N W W S S E
    const int o2 = f | 1;                    // NE NE NW NW SW SW SE SE
    if (!(di_valid(n[o1]) && di_valid(n[o2]))) continue;
    const double e1 = (double)n[o1], e2 = (double)n[o2];
    const double s1 = (e0 - e1) / px, s2 = (e1 - e2) / px;
    double s;
    int mode;
    if (s2 < 0.0) {
      s = s1;
      mode = 0;
    } else if (s2 > s1) {
      s = (e0 - e2) / pxd;
      mode = 1;
    } else {
      s = sqrt(s1 * s1 + s2 * s2);
      mode = 2;
    }
    if (s > best) {
      best = s;
      bf = f;
      bs1 = s1;
      bs2 = s2;
      bmode = mode;
    }
  }
  if (bf >= 0) {
    const double r = bmode == 0 ? 0.0 : (bmode == 1 ? DI_PI / 4 : atan2(bs2, bs1));
    const double af = (bf & 1) ? -1.0 : 1.0, ac = (double)((bf + 1) >> 1);
    double a64 = af * r + ac * (DI_PI / 2);
    if (a64 >= 2 * DI_PI) a64 -= 2 * DI_PI;
    float a32 = (float)a64;
    if (a32 >= DI_F2PI) a32 = 0.0f;
    angle = a32;
    slope = (float)best;
    return;
  }
  if (dt_d8_valid(code)) {  // a pit, a flat or an edge cell: the caller's D8 code, when it points at a valid cell
    const int k = (8 - (__ffs((int)code) - 1)) & 7;
    if (di_valid(n[k])) angle = (float)((double)k * (DI_PI / 4));
  }
}

__global__ __launch_bounds__(256) void k_dinf(const float *__restrict__ dem, const uint8_t *__restrict__ fdr, int H,
                                              int W, int tiles_x, int vec_ok, double px, double pxd,
                                              float *__restrict__ angle, float *__restrict__ slope) {
  __shared__ __attribute__((aligned(16))) float t[(DI_TY + 2) * DI_LDW];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * DI_TX, y0 = tyi * DI_TY;
  di_stage(t, dem, H, W, x0, y0, vec_ok, DT_NODATA);
  __syncthreads();
  const int cx = ((int)threadIdx.x & 31) * 4, ly = (int)threadIdx.x >> 5;
  const int gy = y0 + ly, gx = x0 + cx;
  if (gy >= H || gx >= W) return;
  float a[6], b[6], c[6];
  di_load_row(t, ly, cx, a);
  di_load_row(t, ly + 1, cx, b);
  di_load_row(t, ly + 2, cx, c);
  const long long o = (long long)gy * W + gx;
  const bool full = vec_ok && gx + 3 < W;
  const uint32_t codes = di_load_codes(fdr, o, gx, W, full);
  float ao[4], so[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float n[8];
    di_octants(a, b, c, k, n);
    di_cell(b[k + 1], n, px, pxd, (codes >> (8 * k)) & 0xFFu, ao[k], so[k]);
  }
  if (full) {
    *reinterpret_cast<float4 *>(angle + o) = make_float4(ao[0], ao[1], ao[2], ao[3]);
    if (slope) *reinterpret_cast<float4 *>(slope + o) = make_float4(so[0], so[1], so[2], so[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (gx + k < W) {
        angle[o + k] = ao[k];
        if (slope) slope[o + k] = so[k];
      }
    }
  }
}

// ---- accumulation --------------------------------------------------------------------------------------------------
// MODE: dt_countdown.h's transfer mode; a routing run (MODE != CD_T_NONE) checks its parameter raster here
template <int MODE>
__global__ __launch_bounds__(256) void k_di_init(const float *__restrict__ angle, const double *__restrict__ wt,
                                                 const double *__restrict__ param, int H, int W, int tiles_x,
                                                 int vec_ok, int sbits, unsigned long long qmax,
                                                 unsigned long long *__restrict__ word, uint32_t *__restrict__ ctl,
                                                 int *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) float t[(DI_TY + 2) * DI_LDW];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * DI_TX, y0 = tyi * DI_TY;
  di_stage(t, angle, H, W, x0, y0, vec_ok, DT_NODATA);
  __syncthreads();
  const int cx = ((int)threadIdx.x & 31) * 4, ly = (int)threadIdx.x >> 5;
  const int gy = y0 + ly, gx = x0 + cx;
  bool bad_a = false, bad_w = false, bad_p = false;
  uint32_t two = 0u;
  if (gy < H && gx < W) {
    float a[6], b[6], c[6];
    di_load_row(t, ly, cx, a);
    di_load_row(t, ly + 1, cx, b);
    di_load_row(t, ly + 2, cx, c);
    const long long o = (long long)gy * W + gx;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (gx + k >= W) continue;
      float n[8];
      di_octants(a, b, c, k, n);
      const float me = b[k + 1];
      unsigned long long wv = 0ull;
      if (me != DT_NODATA) {
        bool ignore = false;  // a neighbour's bad angle is reported where it is the centre
        uint32_t pending = 0u;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const DiDec d = di_decode(n[j], ignore);
          const int back = (j + 4) & 7;  // this cell as the neighbour sees it
          pending += (d.kind >= 1 && d.k == back) || (d.kind == 2 && ((d.k + 1) & 7) == back) ? 1u : 0u;
        }
        const DiDec d = di_decode(me, bad_a);
        wv = cd_quant(wt, o + k, sbits, qmax, bad_w) | ((unsigned long long)pending << 56);
        if (pending == 0u) wv |= CD_F_SRC;
        if (d.kind >= 1 && n[d.k] != DT_NODATA) wv |= DI_F_E0;
        if (d.kind == 2 && n[(d.k + 1) & 7] != DT_NODATA) wv |= DI_F_E1;
        two += d.kind == 2 ? 1u : 0u;
        if (MODE != CD_T_NONE) (void)cd_transfer(MODE, 0ull, param, o + k, sbits, bad_p);
      }
      word[o + k] = wv;
    }
  }
  if (status && (bad_a || bad_w || bad_p))
    atomicOr(status, (bad_a ? DT_STATUS_BAD_ANGLE : 0) | (bad_w ? DT_STATUS_BAD_WEIGHT : 0) |
                         (bad_p ? DT_STATUS_BAD_PARAM : 0));
  if (two) atomicAdd(&ctl[CD_C_MULTI], two);
}

// floor(T * p2 / 2^30), T < 2^56, p2 < 2^30: the 86-bit product held exactly in two words
__device__ __forceinline__ unsigned long long di_share(unsigned long long T, uint32_t p2) {
  const unsigned long long lo = T * (unsigned long long)p2, hi = __umul64hi(T, (unsigned long long)p2);
  return (hi << 34) | (lo >> 30);
}

// MODE != CD_T_NONE: the cell splits O = cd_transfer(T) instead of T; a cell's parameter travels with its angle (asked
// for wherever the angle is: at a start, beside the atomics for the receivers, at a pop)
template <bool SCAN, int MODE>
__global__ __launch_bounds__(256) void k_di_flow(const float *__restrict__ angle, const double *__restrict__ param,
                                                 int sbits, unsigned long long *word, int H, int W, uint32_t *queue,
                                                 uint32_t *ctl, int cap, int moves_max) {
  __shared__ uint32_t s_stack[DI_STACK * 256];
  const uint32_t lo = SCAN ? 0u : ctl[CD_C_LO], hi = SCAN ? (uint32_t)((long long)H * W) : ctl[CD_C_HI];
  for (unsigned long long i = (unsigned long long)lo + (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < hi;
       i += (unsigned long long)gridDim.x * 256ull) {
    uint32_t c;
    unsigned long long wv;
    if (SCAN) {
      c = (uint32_t)i;
      wv = word[c];  // a source's word receives nothing; the flag bits of any word never change
      if (!(wv & CD_F_SRC)) continue;
    } else {
      c = queue[i];
      wv = __hip_atomic_load(&word[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float ac = angle[c];
    double pc = MODE != CD_T_NONE ? param[c] : 0.0;
    int sp = 0;
    for (int moves = 0;;) {  // c is complete, wv is its word, ac its angle and pc its parameter
      uint32_t next = CD_NONE;
      unsigned long long nextw = 0ull;
      float nexta = 0.0f;
      double nextp = 0.0;
      if (wv & (DI_F_E0 | DI_F_E1)) {
        bool ignore = false;
        const unsigned long long T = cd_transfer_value(MODE, wv & CD_SUM_MASK, pc, sbits, ignore);
        const DiDec d = di_decode(ac, ignore);
        const unsigned long long m2 = d.kind == 2 ? di_share(T, d.p2) : 0ull;
        const unsigned long long m1 = T - m2;
        // the receivers' angles are asked for beside the atomics, not after the one that completes a receiver: a
        // move then costs one memory round trip, not two in a row
        uint32_t rr[2];
        float ra[2];
        double rp[2] = {0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int k = (d.k + e) & 7;
          const int dx = (int)((DI_DX_PACK >> (2 * k)) & 3u) - 1, dy = (int)((DI_DY_PACK >> (2 * k)) & 3u) - 1;
          rr[e] = (uint32_t)((long long)c + (long long)dy * W + dx);
          ra[e] = (wv & (e ? DI_F_E1 : DI_F_E0)) ? angle[rr[e]] : 0.0f;
          if (MODE != CD_T_NONE) rp[e] = (wv & (e ? DI_F_E1 : DI_F_E0)) ? param[rr[e]] : 0.0;
        }
        // both atomics are in flight before either answer is looked at
        unsigned long long add[2], old[2] = {0ull, 0ull};
#pragma unroll
        for (int e = 0; e < 2; e++) {
          add[e] = (e ? m2 : m1) - CD_ONE_PEND;
          if (wv & (e ? DI_F_E1 : DI_F_E0)) old[e] = atomicAdd(&word[rr[e]], add[e]);
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
          if (cd_pending(old[e]) != 1ull) continue;  // no edge, or donors of the receiver are still to come
          const uint32_t r = rr[e];
          if (next == CD_NONE) {
            next = r;
            nextw = old[e] + add[e];
            nexta = ra[e];
            nextp = rp[e];
          } else if (sp < cap) {
            s_stack[sp++ * 256 + threadIdx.x] = r;
          } else {
            queue[atomicAdd(&ctl[CD_C_TAIL], 1u)] = r;
          }
        }
      }
      if (++moves >= moves_max) {  // this entry's share of the round is used up: the next round carries on
        if (next != CD_NONE) queue[atomicAdd(&ctl[CD_C_TAIL], 1u)] = next;
        while (sp > 0) queue[atomicAdd(&ctl[CD_C_TAIL], 1u)] = s_stack[--sp * 256 + threadIdx.x];
        break;
      }
      if (next != CD_NONE) {
        c = next;
        wv = nextw;
        ac = nexta;
        pc = nextp;
      } else if (sp > 0) {
        c = s_stack[--sp * 256 + threadIdx.x];
        wv = __hip_atomic_load(&word[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ac = angle[c];
        if (MODE != CD_T_NONE) pc = param[c];
      } else {
        break;
      }
    }
  }
}

// MODE == CD_T_NONE writes the accumulation (o.inflow alone, never NULL); a routing run any subset of the four
template <int MODE>
__global__ __launch_bounds__(256) void k_di_out(const float *__restrict__ angle, const double *__restrict__ wt,
                                                const double *__restrict__ param,
                                                const unsigned long long *__restrict__ word, long long N, int sbits,
                                                unsigned long long qmax, const uint32_t *__restrict__ ctl,
                                                CdRouteOut o, int *__restrict__ status) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  cd_not_converged(c == 0, ctl, status);
  if (c >= N) return;
  const unsigned long long wv = word[c];
  const bool complete = angle[c] != DT_NODATA && cd_pending(wv) == 0ull;
  bool ignore = false;
  if (MODE == CD_T_NONE) {
    o.inflow[c] = complete ? cd_result(wv, cd_quant(wt, c, sbits, qmax, ignore), sbits) : -100.0;
    return;
  }
  cd_route_store(MODE, o, c, complete, wv, complete ? cd_quant(wt, c, sbits, qmax, ignore) : 0ull, param, sbits);
}

// ---- launchers -----------------------------------------------------------------------------------------------------
size_t dt_dinf_accumulate_scratch(int64_t H, int64_t W) { return cd_layout(H * W, nullptr, false).bytes; }
// the control words of the accumulation in `scratch` (device pointer to CD_C_WORDS uint32)
const uint32_t *dt_dinf_accumulate_ctl(void *scratch, int64_t H, int64_t W) {
  return cd_layout(H * W, scratch, false).ctl;
}

int dt_launch_dinf_direction(hipStream_t s, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                             float *angle, float *slope) {
  if (H == 0 || W == 0) return DT_OK;
  int tiles_x;
  const unsigned nt = di_tiles(H, W, tiles_x);
  const int vec_ok = di_vec_ok(dem, W) && di_vec_ok(angle, W) && (!slope || di_vec_ok(slope, W)) &&
                     (!fdr || ((uintptr_t)fdr & 3u) == 0);
  hipLaunchKernelGGL(k_dinf, dim3(nt), dim3(256), 0, s, dem, fdr, (int)H, (int)W, tiles_x, vec_ok, px,
                     px * std::sqrt(2.0), angle, slope);
  return DT_OK;
}

// one countdown run of the mode: start, rounds and finish are cd_run's
template <int MODE>
static int di_run(hipStream_t s, const float *angle, const double *wt, const double *param, int64_t H, int64_t W,
                  int frac_bits, int start, int rounds, int finish, int stack_cap, void *scratch, size_t scratch_bytes,
                  CdRouteOut o, int *status) {
  const int64_t N = H * W;
  const CdLayout L = cd_layout(N, scratch, false);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const unsigned long long qmax = cd_qmax(N);
  const int cap = cd_stack_cap(stack_cap, DI_STACK);
  const dim3 b(256);
  return cd_run(
      s, N, L.ctl, start, rounds, finish,
      [&] {
        int tiles_x;
        const unsigned nt = di_tiles(H, W, tiles_x);
        hipLaunchKernelGGL(k_di_init<MODE>, dim3(nt), b, 0, s, angle, wt, param, (int)H, (int)W, tiles_x,
                           di_vec_ok(angle, W), frac_bits, qmax, L.word, L.ctl, status);
      },
      [&](bool scan, dim3 g) {
        auto *flow = scan ? k_di_flow<true, MODE> : k_di_flow<false, MODE>;
        hipLaunchKernelGGL(flow, g, b, 0, s, angle, param, frac_bits, L.word, (int)H, (int)W, L.queue, L.ctl, cap,
                           DI_MOVES);
      },
      [&](dim3 g) {
        hipLaunchKernelGGL(k_di_out<MODE>, g, b, 0, s, angle, wt, param, L.word, (long long)N, frac_bits, qmax, L.ctl,
                           o, status);
      });
}

int dt_launch_dinf_accumulate(hipStream_t s, const float *angle, const double *wt, int64_t H, int64_t W, int frac_bits,
                              int start, int rounds, int finish, int stack_cap, void *scratch, size_t scratch_bytes,
                              double *out, int *status) {
  if (H == 0 || W == 0) return DT_OK;
  return di_run<CD_T_NONE>(s, angle, wt, nullptr, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                           scratch_bytes, CdRouteOut{out, nullptr, nullptr, nullptr}, status);
}

int dt_launch_dinf_route(hipStream_t s, const float *angle, const double *wt, const double *param, int64_t H,
                         int64_t W, int frac_bits, int mode, int start, int rounds, int finish, int stack_cap,
                         void *scratch, size_t scratch_bytes, double *inflow, double *load, double *outflow,
                         double *retained, int *status) {
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(param != nullptr, "NULL parameter raster");
  const CdRouteOut o = {inflow, load, outflow, retained};
  switch (mode) {
    case CD_T_DECAY:
      return di_run<CD_T_DECAY>(s, angle, wt, param, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                                scratch_bytes, o, status);
    case CD_T_RETAIN:
      return di_run<CD_T_RETAIN>(s, angle, wt, param, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                                 scratch_bytes, o, status);
    case CD_T_LIMIT:
      return di_run<CD_T_LIMIT>(s, angle, wt, param, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                                scratch_bytes, o, status);
  }
  DT_REQUIRE(false, "mode must be DT_ROUTE_DECAY, DT_ROUTE_RETAIN or DT_ROUTE_LIMIT");
  return DT_EINVAL;
}
