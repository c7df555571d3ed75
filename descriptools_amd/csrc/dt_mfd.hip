// dt_mfd.hip -- multiple-flow-direction shares and contributing area (Quinn et al. 1991, Freeman 1991, Holmgren 1994;
// net-new, descriptools_amd/mfd.py holds the definition).
//
// Shares (k_mfd_shares): k_dinf's geometry, a 3 x 3 stencil on an LDS tile of 128 x 8 cells with a one-cell halo, four
// cells per lane, everything outside the raster staged as -100.  A valid centre spreads its flow over every valid,
// strictly lower neighbour in proportion to (slope / steepest slope)^p, in float64 on the float32 heights, and stores
// the shares in units of 2^-15 as eight uint16 by octant: one 16-byte store per cell.  The integer exponents (repeated
// multiplication, IEEE-exact) and the others (pow) are two template instances.
//
// Accumulation: the in-degree countdown of dt_countdown.h (the protocol is written out there) on a DAG of out-degree
// <= 8.  The word's own flag: 61 nodata.  One byte per cell beside it: bit k = the edge to the receiver in octant k
// exists (the share is > 0, the receiver lies in the raster and is not nodata).
// k_mf_init   classifies the share words of a 128 x 8 tile and its halo into LDS (receiver mask, nodata, bad), then
//             every cell gathers its in-degree from slot (k + 4) & 7 of neighbour k (no atomics), works out its own
//             edges, quantises its weight and writes word and edge byte.  A word outside the contract raises
//             DT_STATUS_BAD_SHARES and counts as no receiver.
// k_mf_flow   a complete cell sends m_k = floor(T * P_k / 2^15) to every receiver but the main one and the rest to the
//             main one; all of a cell's atomics are issued before any answer is looked at.  The complete cells a lane
//             holds wait in a RING of MF_STACK cells in LDS and are taken in the order they completed (a lane that
//             holds nothing else carries straight on with the receiver it completed); a full ring spills to the
//             queue.  First in, first out and not a stack: a cell completes only after ALL its donors, so the critical
//             path runs through cells that a lane following one branch to its end would leave waiting.  A start
//             completes at most MF_MOVES = 32 cells in a round (both measured: DESIGN.md 4.15).
// k_mf_out    nodata is read from the word.
// The three are templates on dt_countdown.h's transfer mode: CD_T_NONE is the accumulation (no parameter raster is
// read), the others are routing.py's decay / retain / limit, which split O = cd_transfer(T) and write up to four rasters.
#include <cmath>

#include "dt_countdown.h"
#include "dt_dinf_common.h"

#define MF_F_NODATA (1ull << 61)
#define MF_MOVES 32  // cells one start (a source, a queue entry) may complete in a round before it hands on
#define MF_STACK 8   // complete cells a lane holds in its ring in LDS (a power of two)
#define MF_UNIT 32768u
// a share word as k_mf_init classifies it: bits 0-7 the octants with a share > 0
#define MF_CL_NODATA 0x100u
#define MF_CL_BAD 0x200u

__device__ __forceinline__ void mf_unpack(const uint4 w, uint32_t (&P)[8]) {
  P[0] = w.x & 0xFFFFu;
  P[1] = w.x >> 16;
  P[2] = w.y & 0xFFFFu;
  P[3] = w.y >> 16;
  P[4] = w.z & 0xFFFFu;
  P[5] = w.z >> 16;
  P[6] = w.w & 0xFFFFu;
  P[7] = w.w >> 16;
}
__device__ __forceinline__ uint4 mf_pack(const uint32_t (&P)[8]) {
  return make_uint4(P[0] | P[1] << 16, P[2] | P[3] << 16, P[4] | P[5] << 16, P[6] | P[7] << 16);
}

// ---- shares ------------------------------------------------------------------------------------------------------
// one cell: the centre and its neighbours by octant; ce / co = the contour weight of the even / odd octants (1 without
// `contour`: an exact product); code = the caller's D8 code (0 without one)
template <bool INT_P>
__device__ __forceinline__ uint4 mf_cell(float c, const float (&n)[8], double p, int ip, double ce, double co,
                                         uint32_t code) {
  if (c <= DT_NODATA) return make_uint4(~0u, ~0u, ~0u, ~0u);
  uint32_t P[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (!di_valid(c)) return mf_pack(P);  // NaN, +inf: no receiver
  const double z0 = (double)c;
  double g[8], gmax = 0.0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const bool rec = di_valid(n[k]) && n[k] < c;
    const double d = z0 - (double)n[k];
    g[k] = rec ? ((k & 1) ? d / 1.4142135623730951 : d) : 0.0;  // > 0 for every receiver
    gmax = g[k] > gmax ? g[k] : gmax;
  }
  if (gmax > 0.0) {
    double u[8], f[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      u[k] = g[k] / gmax;
      f[k] = 1.0;
    }
    if (INT_P) {
      for (int i = 0; i < ip; i++) {
#pragma unroll
        for (int k = 0; k < 8; k++) f[k] = f[k] * u[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) f[k] = pow(u[k], p);
    }
    double F = 0.0, fbest = 0.0;
    int mk = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      f[k] = g[k] > 0.0 ? f[k] * ((k & 1) ? co : ce) : 0.0;
      F = F + f[k];
      if (f[k] > fbest) {
        fbest = f[k];
        mk = k;
      }
    }
    uint32_t others = 0u;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      P[k] = (uint32_t)floor(ldexp(f[k] / F, 15));
      others += k == mk ? 0u : P[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (k == mk) P[k] = MF_UNIT - others;
    return mf_pack(P);
  }
  if (dt_d8_valid(code)) {  // a pit, a flat or a cell with a complete rim: the caller's D8 code, when it points at a
    const int k = (8 - (__ffs((int)code) - 1)) & 7;  // valid cell
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (j == k && di_valid(n[j])) P[j] = MF_UNIT;
  }
  return mf_pack(P);
}

template <bool INT_P>
__global__ __launch_bounds__(256) void k_mfd_shares(const float *__restrict__ dem, const uint8_t *__restrict__ fdr,
                                                    int H, int W, int tiles_x, int vec_ok, double p, int ip, double ce,
                                                    double co, uint4 *__restrict__ shares) {
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
  const uint32_t codes = di_load_codes(fdr, o, gx, W, vec_ok && gx + 3 < W);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (gx + k >= W) continue;
    float n[8];
    di_octants(a, b, c, k, n);
    shares[o + k] = mf_cell<INT_P>(b[k + 1], n, p, ip, ce, co, (codes >> (8 * k)) & 0xFFu);
  }
}

// ---- accumulation --------------------------------------------------------------------------------------------------
// receiver mask | MF_CL_NODATA | MF_CL_BAD of one share word: nodata is eight 0xFFFF; otherwise every slot is <= 2^15
// and the slots sum to 0 or 2^15, anything else is bad and has no receiver
__device__ __forceinline__ uint32_t mf_classify(const uint4 w) {
  if ((w.x & w.y & w.z & w.w) == 0xFFFFFFFFu) return MF_CL_NODATA;
  uint32_t P[8];
  mf_unpack(w, P);
  uint32_t sum = 0u, over = 0u, mask = 0u;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    sum += P[k];
    over |= P[k] > MF_UNIT ? 1u : 0u;
    mask |= P[k] ? 1u << k : 0u;
  }
  if (over || (sum != 0u && sum != MF_UNIT)) return MF_CL_BAD;
  return mask;
}

#define MF_TW (DI_TX + 2)  // the classified tile: (DI_TY + 2) rows of DI_TX + 2 cells
// MODE: dt_countdown.h's transfer mode; a routing run (MODE != CD_T_NONE) checks its parameter raster here
template <int MODE>
__global__ __launch_bounds__(256) void k_mf_init(const uint4 *__restrict__ shares, const double *__restrict__ wt,
                                                 const double *__restrict__ param, int H, int W, int tiles_x,
                                                 int sbits, unsigned long long qmax,
                                                 unsigned long long *__restrict__ word, uint8_t *__restrict__ edges,
                                                 uint32_t *__restrict__ ctl, int *__restrict__ status) {
  __shared__ uint16_t t[(DI_TY + 2) * MF_TW];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * DI_TX, y0 = tyi * DI_TY;
  for (int i = (int)threadIdx.x; i < (DI_TY + 2) * MF_TW; i += 256) {
    const int r = i / MF_TW, cc = i - r * MF_TW;
    const int gy = y0 - 1 + r, gx = x0 - 1 + cc;
    uint32_t cl = MF_CL_NODATA;  // outside the raster: no donor, no receiver
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) cl = mf_classify(shares[(long long)gy * W + gx]);
    t[i] = (uint16_t)cl;
  }
  __syncthreads();
  bool bad_s = false, bad_w = false, bad_p = false;
  uint32_t multi = 0u;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int j = (int)threadIdx.x + 256 * v;
    const int ly = j / DI_TX, lx = j - ly * DI_TX;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const long long o = (long long)gy * W + gx;
    const uint32_t me = t[(ly + 1) * MF_TW + lx + 1];
    unsigned long long wv = MF_F_NODATA;
    uint32_t emask = 0u;
    if (!(me & MF_CL_NODATA)) {
      uint32_t pending = 0u;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int dx = (int)((DI_DX_PACK >> (2 * k)) & 3u) - 1, dy = (int)((DI_DY_PACK >> (2 * k)) & 3u) - 1;
        const uint32_t nb = t[(ly + 1 + dy) * MF_TW + lx + 1 + dx];
        pending += (nb >> ((k + 4) & 7)) & 1u;  // this cell as neighbour k sees it; the bit is 0 on nodata and bad
        emask |= (nb & MF_CL_NODATA) ? 0u : me & (1u << k);
      }
      bad_s |= (me & MF_CL_BAD) != 0u;
      multi += __popc(me & 0xFFu) >= 2 ? 1u : 0u;
      wv = cd_quant(wt, o, sbits, qmax, bad_w) | ((unsigned long long)pending << 56);
      if (pending == 0u) wv |= CD_F_SRC;
      if (MODE != CD_T_NONE) (void)cd_transfer(MODE, 0ull, param, o, sbits, bad_p);
    }
    word[o] = wv;
    edges[o] = (uint8_t)emask;
  }
  if (status && (bad_s || bad_w || bad_p))
    atomicOr(status, (bad_s ? DT_STATUS_BAD_SHARES : 0) | (bad_w ? DT_STATUS_BAD_WEIGHT : 0) |
                         (bad_p ? DT_STATUS_BAD_PARAM : 0));
  if (multi) atomicAdd(&ctl[CD_C_MULTI], multi);
}

// floor(T * P / 2^15), T < 2^56, P <= 2^15, in 64 bits
__device__ __forceinline__ unsigned long long mf_share(unsigned long long T, uint32_t P) {
  return (T >> 15) * P + (((T & 32767ull) * P) >> 15);
}

// a complete cell that this lane cannot keep goes on the queue; n = its slots (a cell is queued once, so the guard
// never refuses: it keeps a mistake elsewhere from becoming a store out of bounds)
__device__ __forceinline__ void mf_enqueue(uint32_t *queue, uint32_t *ctl, uint32_t n, uint32_t c) {
  const uint32_t i = atomicAdd(&ctl[CD_C_TAIL], 1u);
  if (i < n) queue[i] = c;
}

// MODE != CD_T_NONE: the cell splits O = cd_transfer(T) instead of T; its parameter is asked for beside its shares
template <bool SCAN, int MODE>
__global__ __launch_bounds__(256) void k_mf_flow(const uint4 *__restrict__ shares, const uint8_t *__restrict__ edges,
                                                 const double *__restrict__ param, int sbits,
                                                 unsigned long long *word, int W, uint32_t n, uint32_t *queue,
                                                 uint32_t *ctl, int cap, int moves_max) {
  __shared__ uint32_t s_ring[MF_STACK * 256];
  const uint32_t lo = SCAN ? 0u : ctl[CD_C_LO], hi = SCAN ? n : min(ctl[CD_C_HI], n);
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
    int held = 0, head = 0;  // the ring: `held` cells from slot `head` on
    for (int moves = 0;;) {  // c is complete and wv is its word
      uint32_t next = CD_NONE;
      unsigned long long nextw = 0ull;
      const uint32_t em = edges[c];
      if (em) {
        unsigned long long T = wv & CD_SUM_MASK;
        const uint4 sw = shares[c];
        if (MODE != CD_T_NONE) {
          bool ignore = false;
          T = cd_transfer(MODE, T, param, c, sbits, ignore);
        }
        uint32_t P[8];
        mf_unpack(sw, P);
        int mk = 0;
        uint32_t pbest = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          if (P[k] > pbest) {
            pbest = P[k];
            mk = k;
          }
        }
        unsigned long long m[8], others = 0ull;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          m[k] = k == mk ? 0ull : mf_share(T, P[k]);
          others += m[k];
        }
        // every atomic of the cell is in flight before any answer is looked at
        unsigned long long add[8], old[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int dx = (int)((DI_DX_PACK >> (2 * k)) & 3u) - 1, dy = (int)((DI_DY_PACK >> (2 * k)) & 3u) - 1;
          add[k] = (k == mk ? T - others : m[k]) - CD_ONE_PEND;
          old[k] = 0ull;
          if (em & (1u << k)) old[k] = atomicAdd(&word[(long long)c + (long long)dy * W + dx], add[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
          if (cd_pending(old[k]) != 1ull) continue;  // no edge, or donors of the receiver are still to come
          const int dx = (int)((DI_DX_PACK >> (2 * k)) & 3u) - 1, dy = (int)((DI_DY_PACK >> (2 * k)) & 3u) - 1;
          const uint32_t r = (uint32_t)((long long)c + (long long)dy * W + dx);
          if (next == CD_NONE) {
            next = r;
            nextw = old[k] + add[k];
          } else if (held < cap) {
            s_ring[((head + held++) & (MF_STACK - 1)) * 256 + threadIdx.x] = r;
          } else {
            mf_enqueue(queue, ctl, n, r);
          }
        }
      }
      if (++moves >= moves_max) {  // this entry's share of the round is used up: the next round carries on
        if (next != CD_NONE) mf_enqueue(queue, ctl, n, next);
        while (held > 0) mf_enqueue(queue, ctl, n, s_ring[((head + --held) & (MF_STACK - 1)) * 256 + threadIdx.x]);
        break;
      }
      if (next != CD_NONE && held > 0) {  // cells wait in the ring: this one goes behind them
        if (held < cap)
          s_ring[((head + held++) & (MF_STACK - 1)) * 256 + threadIdx.x] = next;
        else
          mf_enqueue(queue, ctl, n, next);
        next = CD_NONE;
      }
      if (next != CD_NONE) {
        c = next;
        wv = nextw;
      } else if (held > 0) {
        c = s_ring[(head++ & (MF_STACK - 1)) * 256 + threadIdx.x];
        held--;
        wv = __hip_atomic_load(&word[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        break;
      }
    }
  }
}

// MODE == CD_T_NONE writes the accumulation (o.inflow alone, never NULL); a routing run any subset of the four
template <int MODE>
__global__ __launch_bounds__(256) void k_mf_out(const double *__restrict__ wt, const double *__restrict__ param,
                                                const unsigned long long *__restrict__ word, long long N, int sbits,
                                                unsigned long long qmax, const uint32_t *__restrict__ ctl,
                                                CdRouteOut o, int *__restrict__ status) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  cd_not_converged(c == 0, ctl, status);
  if (c >= N) return;
  const unsigned long long wv = word[c];
  const bool complete = !(wv & MF_F_NODATA) && cd_pending(wv) == 0ull;
  bool ignore = false;
  if (MODE == CD_T_NONE) {
    o.inflow[c] = complete ? cd_result(wv, cd_quant(wt, c, sbits, qmax, ignore), sbits) : -100.0;
    return;
  }
  cd_route_store(MODE, o, c, complete, wv, complete ? cd_quant(wt, c, sbits, qmax, ignore) : 0ull, param, sbits);
}

// ---- launchers -----------------------------------------------------------------------------------------------------
size_t dt_mfd_accumulate_scratch(int64_t H, int64_t W) { return cd_layout(H * W, nullptr, true).bytes; }
// the control words of the accumulation in `scratch` (device pointer to CD_C_WORDS uint32)
const uint32_t *dt_mfd_accumulate_ctl(void *scratch, int64_t H, int64_t W) {
  return cd_layout(H * W, scratch, true).ctl;
}

int dt_launch_mfd_shares(hipStream_t s, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double exponent,
                         int contour, uint16_t *shares) {
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(exponent >= 0.0 && exponent <= 64.0, "exponent must lie in [0, 64]");
  DT_REQUIRE(((uintptr_t)shares & 15u) == 0, "the share raster must be 16-byte aligned");
  int tiles_x;
  const unsigned nt = di_tiles(H, W, tiles_x);
  const int vec_ok = W % 4 == 0 && ((uintptr_t)dem & 15u) == 0 && (!fdr || ((uintptr_t)fdr & 3u) == 0);
  const double ce = contour ? 0.5 : 1.0, co = contour ? 0.35355339059327373 : 1.0;
  const bool int_p = exponent == std::floor(exponent);
  if (int_p)
    hipLaunchKernelGGL(k_mfd_shares<true>, dim3(nt), dim3(256), 0, s, dem, fdr, (int)H, (int)W, tiles_x, vec_ok,
                       exponent, (int)exponent, ce, co, (uint4 *)shares);
  else
    hipLaunchKernelGGL(k_mfd_shares<false>, dim3(nt), dim3(256), 0, s, dem, fdr, (int)H, (int)W, tiles_x, vec_ok,
                       exponent, 0, ce, co, (uint4 *)shares);
  return DT_OK;
}

// one countdown run of the mode: start, rounds and finish are cd_run's
template <int MODE>
static int mf_run(hipStream_t s, const uint16_t *shares, const double *wt, const double *param, int64_t H, int64_t W,
                  int frac_bits, int start, int rounds, int finish, int stack_cap, void *scratch, size_t scratch_bytes,
                  CdRouteOut o, int *status) {
  const int64_t N = H * W;
  const CdLayout L = cd_layout(N, scratch, true);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  DT_REQUIRE(((uintptr_t)shares & 15u) == 0, "the share raster must be 16-byte aligned");
  const unsigned long long qmax = cd_qmax(N);
  const int cap = cd_stack_cap(stack_cap, MF_STACK);
  const uint4 *sh = (const uint4 *)shares;
  const dim3 b(256);
  return cd_run(
      s, N, L.ctl, start, rounds, finish,
      [&] {
        int tiles_x;
        const unsigned nt = di_tiles(H, W, tiles_x);
        hipLaunchKernelGGL(k_mf_init<MODE>, dim3(nt), b, 0, s, sh, wt, param, (int)H, (int)W, tiles_x, frac_bits, qmax,
                           L.word, L.edges, L.ctl, status);
      },
      [&](bool scan, dim3 g) {
        auto *flow = scan ? k_mf_flow<true, MODE> : k_mf_flow<false, MODE>;
        hipLaunchKernelGGL(flow, g, b, 0, s, sh, L.edges, param, frac_bits, L.word, (int)W, (uint32_t)N, L.queue,
                           L.ctl, cap, MF_MOVES);
      },
      [&](dim3 g) {
        hipLaunchKernelGGL(k_mf_out<MODE>, g, b, 0, s, wt, param, L.word, (long long)N, frac_bits, qmax, L.ctl, o,
                           status);
      });
}

int dt_launch_mfd_accumulate(hipStream_t s, const uint16_t *shares, const double *wt, int64_t H, int64_t W,
                             int frac_bits, int start, int rounds, int finish, int stack_cap, void *scratch,
                             size_t scratch_bytes, double *out, int *status) {
  if (H == 0 || W == 0) return DT_OK;
  return mf_run<CD_T_NONE>(s, shares, wt, nullptr, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                           scratch_bytes, CdRouteOut{out, nullptr, nullptr, nullptr}, status);
}

int dt_launch_mfd_route(hipStream_t s, const uint16_t *shares, const double *wt, const double *param, int64_t H,
                        int64_t W, int frac_bits, int mode, int start, int rounds, int finish, int stack_cap,
                        void *scratch, size_t scratch_bytes, double *inflow, double *load, double *outflow,
                        double *retained, int *status) {
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(param != nullptr, "NULL parameter raster");
  const CdRouteOut o = {inflow, load, outflow, retained};
  switch (mode) {
    case CD_T_DECAY:
      return mf_run<CD_T_DECAY>(s, shares, wt, param, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                                scratch_bytes, o, status);
    case CD_T_RETAIN:
      return mf_run<CD_T_RETAIN>(s, shares, wt, param, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                                 scratch_bytes, o, status);
    case CD_T_LIMIT:
      return mf_run<CD_T_LIMIT>(s, shares, wt, param, H, W, frac_bits, start, rounds, finish, stack_cap, scratch,
                                scratch_bytes, o, status);
  }
  DT_REQUIRE(false, "mode must be DT_ROUTE_DECAY, DT_ROUTE_RETAIN or DT_ROUTE_LIMIT");
  return DT_EINVAL;
}
