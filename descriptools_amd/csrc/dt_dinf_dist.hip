// dt_dinf_dist.hip -- D-infinity distance down to the stream: horizontal, vertical (the D-infinity HAND) and surface
// distance along the D-infinity flow field, as the average / minimum / maximum over the two receivers (net-new;
// descriptools_amd/dinf.py holds the definition; TauDEM's DinfDistDown as we read it).
//
// The drainage graph is a DAG of out-degree <= 2 and a cell's value is a function of its receivers' final values:
// values are PULLED up the graph from the targets (dt_dinf.hip pushes mass down it).  The chain of dependencies is a
// hillslope flow path to the nearest stream cell, a few hundred cells, so the schedule is that of dt_tile_rounds.h (the
// conditioning rounds' one), not a countdown:
// k_dd_init   decodes every angle once (the 128 x 8 tile of dt_dinf_common.h) and writes one state byte per cell,
//               bits 0-1 DD_UNSET / DD_REACH / DD_DEAD / DD_NODATA | 2, 3 the edge to the first / second receiver exists
//               | 4 a share leaves the domain
//             targets (river == 1, not nodata) reach with 0 in every measure, cells without an edge are dead.
// k_dd_round  one workgroup per tile of 32 x 32 cells with a one-cell halo: state bytes, heights and the settled
//             values of tile and halo go to LDS, each lane keeps its four cells' decoded angles in registers.  A sweep
//             is two steps with a barrier between them: every unsettled cell whose receivers are ALL settled works out
//             its state and values from LDS into registers, then the lanes write them to LDS -- no lane reads a value
//             another one is writing, and a sweep moves every chain of the tile one cell on.  Sweeps repeat until one
//             settles nothing (at most 32 * 32 + 1 of them: each but the last settles a cell) or `visit_limit` is
//             reached.  The newly settled cells go to the state raster and the output rasters, which double as the
//             store of settled values: settling is write-once.  The tile leaves an activity byte (dt_tile_rounds.h):
//             HY_CHANGED when it settled something (anywhere in the tile, not only on its outer ring), HY_OPEN when the
//             limit stopped it; the round raises its flag word when it settled anything.
// k_dd_final  -100 on everything that does not reach; counts the reaching, dead and unsettled cells.
// No data passes between workgroups inside a launch, nothing waits for another workgroup, no float atomics: every
// value is computed once, by one lane, from final values, in the association the definition gives -- the result does
// not depend on the schedule, the number of rounds or visit_limit.  A cycle never settles: it costs one quiet round.
#include <cmath>

#include "dt_dinf_common.h"
#include "dt_tile_rounds.h"

#define DD_T 32
#define DD_LD (DD_T + 2)
#define DD_LS (DD_LD + 1)  // LDS row stride in cells
#define DD_CELLS (DD_LD * DD_LS)
#define DD_CPT (DD_T * DD_T / 256)

#define DD_UNSET 0u
#define DD_REACH 1u
#define DD_DEAD 2u
#define DD_NODATA 3u
#define DD_STATE 3u
#define DD_E0 4u
#define DD_E1 8u
#define DD_LEAVE 16u

// control words of one call: the flags of a batch of rounds, then the final kernel's counts
// (and, as one 64-bit word, the tile visits of the call)
enum {
  DD_C_FLAGS = 0,  // DT_TILE_ROUNDS_BATCH_MAX of them
  DD_C_REACH = DT_TILE_ROUNDS_BATCH_MAX,
  DD_C_DEAD,
  DD_C_UNSET,
  DD_C_VISITS = DD_C_REACH + 4,  // 8-byte aligned
  DD_C_WORDS = DD_C_REACH + 8
};

__global__ __launch_bounds__(256) void k_dd_init(const float *__restrict__ angle, const int8_t *__restrict__ river,
                                                 int H, int W, int tiles_x, int vec_ok, uint8_t *__restrict__ st,
                                                 double *__restrict__ oh, double *__restrict__ ov,
                                                 double *__restrict__ os, int *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) float t[(DI_TY + 2) * DI_LDW];
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * DI_TX, y0 = tyi * DI_TY;
  di_stage(t, angle, H, W, x0, y0, vec_ok, DT_NODATA);
  __syncthreads();
  const int cx = ((int)threadIdx.x & 31) * 4, ly = (int)threadIdx.x >> 5;
  const int gy = y0 + ly, gx = x0 + cx;
  bool bad = false;
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
      uint32_t sv = DD_NODATA;
      if (me != DT_NODATA) {
        const DiDec d = di_decode(me, bad);
        const bool e0 = d.kind >= 1 && n[d.k] != DT_NODATA;
        const bool e1 = d.kind == 2 && n[(d.k + 1) & 7] != DT_NODATA;
        const bool leave = (d.kind >= 1 && !e0) || (d.kind == 2 && !e1);
        if (river[o + k] == 1) {
          sv = DD_REACH;
          oh[o + k] = 0.0;
          if (ov) ov[o + k] = 0.0;
          if (os) os[o + k] = 0.0;
        } else if (!(e0 || e1)) {
          sv = DD_DEAD;
        } else {
          sv = DD_UNSET | (e0 ? DD_E0 : 0u) | (e1 ? DD_E1 : 0u) | (leave ? DD_LEAVE : 0u);
        }
      }
      st[o + k] = (uint8_t)sv;
    }
  }
  if (status && bad) atomicOr(status, DT_STATUS_BAD_ANGLE);
}

// the term of one measure over the reaching receivers (n of them, in the order j = 0, 1)
__device__ __forceinline__ double dd_stat(int stat, int n, double t0, double t1, double w0, double w1) {
  if (n == 1) return t0;
  if (stat == 0) return (w0 * t0 + w1 * t1) * 0x1p-30;
  if (stat == 1) return t1 < t0 ? t1 : t0;
  return t1 > t0 ? t1 : t0;
}

// Z: heights are given and the vertical and the surface measure are computed beside the horizontal one
template <bool Z>
__global__ __launch_bounds__(256) void k_dd_round(const float *__restrict__ angle, const float *__restrict__ dem,
                                                  uint8_t *__restrict__ st, double *__restrict__ oh,
                                                  double *__restrict__ ov, double *__restrict__ os, int H, int W,
                                                  double px, double pxd, int stat, int check_edges, int visit_limit,
                                                  const HyRound rnd) {
  __shared__ double s_h[DD_CELLS];
  __shared__ double s_v[Z ? DD_CELLS : 1];
  __shared__ double s_s[Z ? DD_CELLS : 1];
  __shared__ float s_z[Z ? DD_CELLS : 1];
  __shared__ uint8_t s_st[DD_CELLS];
  int ty, tx;
  if (!hy_round_enter(rnd, ty, tx)) return;
  const int tile = ty * rnd.tiles_x + tx;
  const int y0 = ty * DD_T, x0 = tx * DD_T;
  // tile and halo: the state of every cell (nodata beyond the raster) and the values of the cells that reach
  for (int i = threadIdx.x; i < DD_LD * DD_LD; i += 256) {
    const int r = i / DD_LD, c = i - r * DD_LD;
    const int gy = y0 - 1 + r, gx = x0 - 1 + c;
    const int p = r * DD_LS + c;
    uint32_t sv = DD_NODATA;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const long long g = (long long)gy * W + gx;
      sv = st[g];
      if (Z) s_z[p] = dem[g];
      if ((sv & DD_STATE) == DD_REACH) {
        s_h[p] = oh[g];
        if (Z) {
          s_v[p] = ov[g];
          s_s[p] = os[g];
        }
      }
    }
    s_st[p] = (uint8_t)sv;
  }
  // this lane's cells: where they and their receivers lie in LDS, the second receiver's share
  int pc[DD_CPT], pr0[DD_CPT], pr1[DD_CPT];
  uint32_t sv0[DD_CPT], cur[DD_CPT], p2[DD_CPT];
#pragma unroll
  for (int j = 0; j < DD_CPT; j++) {
    const int c = (int)threadIdx.x + 256 * j;
    const int ly = c / DD_T, lx = c - ly * DD_T;
    const int gy = y0 + ly, gx = x0 + lx;
    pc[j] = (ly + 1) * DD_LS + lx + 1;
    pr0[j] = pr1[j] = pc[j];
    p2[j] = 0u;
    sv0[j] = DD_NODATA;
    if (gy < H && gx < W) {
      const long long g = (long long)gy * W + gx;
      sv0[j] = st[g];
      if ((sv0[j] & DD_STATE) == DD_UNSET) {
        bool ignore = false;  // k_dd_init reported it
        const DiDec d = di_decode(angle[g], ignore);
        const int k0 = d.k, k1 = (d.k + 1) & 7;
        pr0[j] = pc[j] + ((int)((DI_DY_PACK >> (2 * k0)) & 3u) - 1) * DD_LS + (int)((DI_DX_PACK >> (2 * k0)) & 3u) - 1;
        pr1[j] = pc[j] + ((int)((DI_DY_PACK >> (2 * k1)) & 3u) - 1) * DD_LS + (int)((DI_DX_PACK >> (2 * k1)) & 3u) - 1;
        p2[j] = d.p2;
        sv0[j] |= (uint32_t)k0 << 8;  // the first receiver's octant: the second one's is the next
      }
    }
    cur[j] = sv0[j];
  }
  __syncthreads();
  // each sweep but the last settles at least one of the tile's cells
  const int sweeps_max = visit_limit > 0 ? visit_limit : DD_T * DD_T + 1;
  int settled = 0, open = 0;
  for (int sweep = 0; sweep < sweeps_max; sweep++) {
    uint32_t ns[DD_CPT];
    double nh[DD_CPT], nv[DD_CPT], nsf[DD_CPT];
    int any = 0;
#pragma unroll
    for (int j = 0; j < DD_CPT; j++) {
      ns[j] = DD_UNSET;
      nh[j] = nv[j] = nsf[j] = 0.0;
      if ((cur[j] & DD_STATE) != DD_UNSET) continue;
      const bool e0 = (cur[j] & DD_E0) != 0u, e1 = (cur[j] & DD_E1) != 0u;
      const uint32_t s0 = e0 ? (uint32_t)s_st[pr0[j]] & DD_STATE : DD_DEAD;
      const uint32_t s1 = e1 ? (uint32_t)s_st[pr1[j]] & DD_STATE : DD_DEAD;
      if (s0 == DD_UNSET || s1 == DD_UNSET) continue;  // a receiver it has an edge to is not settled yet
      const bool r0 = e0 && s0 == DD_REACH, r1 = e1 && s1 == DD_REACH;
      const bool reach = check_edges ? (!(cur[j] & DD_LEAVE) && (!e0 || r0) && (!e1 || r1)) : (r0 || r1);
      any = 1;
      if (!reach) {
        ns[j] = DD_DEAD;
        continue;
      }
      ns[j] = DD_REACH;
      const int k0 = (int)(cur[j] >> 8) & 7;
      // the terms of the two receivers (octant k0 + 1 has the other parity); the first reaching one comes first
      double ah[2] = {0.0, 0.0}, av[2] = {0.0, 0.0}, as[2] = {0.0, 0.0};
#pragma unroll
      for (int e = 0; e < 2; e++) {
        if (!(e ? r1 : r0)) continue;
        const int pr = e ? pr1[j] : pr0[j];
        const double L = ((k0 + e) & 1) ? pxd : px;
        ah[e] = s_h[pr] + L;
        if (Z) {
          const double dz = (double)s_z[pc[j]] - (double)s_z[pr];
          av[e] = s_v[pr] + dz;
          as[e] = s_s[pr] + sqrt(L * L + dz * dz);
        }
      }
      const int n = (r0 ? 1 : 0) + (r1 ? 1 : 0);
      const double w1 = (double)p2[j], w0 = (double)((1u << 30) - p2[j]);
      nh[j] = dd_stat(stat, n, r0 ? ah[0] : ah[1], ah[1], w0, w1);
      if (Z) {
        nv[j] = dd_stat(stat, n, r0 ? av[0] : av[1], av[1], w0, w1);
        nsf[j] = dd_stat(stat, n, r0 ? as[0] : as[1], as[1], w0, w1);
      }
    }
    __syncthreads();  // every lane has read what it needs of this sweep's LDS
#pragma unroll
    for (int j = 0; j < DD_CPT; j++) {
      if (ns[j] == DD_UNSET) continue;
      cur[j] = (cur[j] & ~DD_STATE) | ns[j];
      s_st[pc[j]] = (uint8_t)cur[j];
      if (ns[j] == DD_REACH) {
        s_h[pc[j]] = nh[j];
        if (Z) {
          s_v[pc[j]] = nv[j];
          s_s[pc[j]] = nsf[j];
        }
      }
    }
    open = __syncthreads_or(any);
    if (!open) break;
    settled = 1;
  }
  // the newly settled cells: the state raster and, where they reach, the outputs
#pragma unroll
  for (int j = 0; j < DD_CPT; j++) {
    if ((sv0[j] & DD_STATE) != DD_UNSET || (cur[j] & DD_STATE) == DD_UNSET) continue;
    const int c = (int)threadIdx.x + 256 * j;
    const int ly = c / DD_T, lx = c - ly * DD_T;
    const long long g = (long long)(y0 + ly) * W + (x0 + lx);
    st[g] = (uint8_t)cur[j];
    if ((cur[j] & DD_STATE) == DD_REACH) {
      oh[g] = s_h[pc[j]];
      if (Z) {
        ov[g] = s_v[pc[j]];
        os[g] = s_s[pc[j]];
      }
    }
  }
  // open: the limit ended the visit while a sweep still settled something
  hy_round_leave(rnd, tile, settled ? HY_CHANGED | (open ? HY_OPEN : 0) : 0, settled);
}

__global__ __launch_bounds__(256) void k_dd_final(const uint8_t *__restrict__ st, long long N, double *__restrict__ oh,
                                                  double *__restrict__ ov, double *__restrict__ os,
                                                  const uint32_t *__restrict__ visits, int tiles,
                                                  uint32_t *__restrict__ ctl) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  uint32_t sv = DD_NODATA;
  if (c < N) {
    sv = st[c] & DD_STATE;
    if (sv != DD_REACH) {
      oh[c] = -100.0;
      if (ov) ov[c] = -100.0;
      if (os) os[c] = -100.0;
    }
  }
  const int nr = __syncthreads_count(sv == DD_REACH), nd = __syncthreads_count(sv == DD_DEAD),
            nu = __syncthreads_count(sv == DD_UNSET);
  hy_visits_sum(visits, tiles, &ctl[DD_C_VISITS]);
  if (threadIdx.x == 0) {
    if (nr) atomicAdd(&ctl[DD_C_REACH], (uint32_t)nr);
    if (nd) atomicAdd(&ctl[DD_C_DEAD], (uint32_t)nd);
    if (nu) atomicAdd(&ctl[DD_C_UNSET], (uint32_t)nu);
  }
}

// ---- launcher ------------------------------------------------------------------------------------------------------
struct DdLayout {
  HyRoundsScratch r;
  uint8_t *st;  // the state byte of every cell
  size_t bytes;
};
static DdLayout dd_layout(int64_t H, int64_t W, void *scratch) {
  DdLayout L = {};
  DtCarver c(scratch);
  L.r = hy_rounds_take(c, H, W, DD_T, DD_C_WORDS, &L.st);
  L.bytes = c.bytes();
  return L;
}
size_t dt_dinf_distance_scratch(int64_t H, int64_t W) { return dd_layout(H, W, nullptr).bytes; }
const uint32_t *dt_dinf_distance_ctl(void *scratch, int64_t H, int64_t W) { return dd_layout(H, W, scratch).r.ctl; }

// start != 0: k_dd_init first, and the first of the rounds visits every tile; `rounds` (<= 64) rounds, round r raising
// control word r when it settled something; finish != 0: k_dd_final, its counts in control words 64-66 and the tile
// visits of the call as a 64-bit count in words 68-69
int dt_launch_dinf_distance(hipStream_t s, const float *angle, const int8_t *river, const float *dem, int64_t H,
                            int64_t W, double px, int stat, int check_edges, int visit_limit, int start, int rounds,
                            int finish, void *scratch, size_t scratch_bytes, double *h, double *v, double *sf,
                            int *status) {
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(stat >= 0 && stat <= 2 && (check_edges == 0 || check_edges == 1) && visit_limit >= 0, "bad stat, check_edges or visit_limit");
  DT_REQUIRE(rounds >= 0 && rounds <= DT_TILE_ROUNDS_BATCH_MAX, "bad number of rounds");
  DT_REQUIRE(dem ? (v && sf) : (!v && !sf), "heights go with both the vertical and the surface raster");
  const int64_t N = H * W;
  const DdLayout L = dd_layout(H, W, scratch);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const dim3 b(256);
  if (start) {
    int tiles_x;
    const unsigned nt = di_tiles(H, W, tiles_x);
    hipLaunchKernelGGL(k_dd_init, dim3(nt), b, 0, s, angle, river, (int)H, (int)W, tiles_x, di_vec_ok(angle, W), L.st,
                       h, v, sf, status);
  }
  const double pxd = px * 1.4142135623730951;
  DT_TRY(hy_launch_rounds(s, L.r, L.r.ctl + DD_C_FLAGS, start, rounds, [&](dim3 blocks, const HyRound &rnd) {
    if (dem)
      hipLaunchKernelGGL(k_dd_round<true>, blocks, b, 0, s, angle, dem, L.st, h, v, sf, (int)H, (int)W, px, pxd, stat,
                         check_edges, visit_limit, rnd);
    else
      hipLaunchKernelGGL(k_dd_round<false>, blocks, b, 0, s, angle, dem, L.st, h, v, sf, (int)H, (int)W, px, pxd, stat,
                         check_edges, visit_limit, rnd);
  }));
  if (finish) {
    DT_HIP(hipMemsetAsync(L.r.ctl + DD_C_REACH, 0, sizeof(uint32_t) * (DD_C_WORDS - DD_C_REACH), s));
    hipLaunchKernelGGL(k_dd_final, dim3((unsigned)((N + 255) / 256)), b, 0, s, (const uint8_t *)L.st, (long long)N, h, v,
                       sf, (const uint32_t *)L.r.visits, (int)L.r.tiles(), L.r.ctl);
  }
  return DT_OK;
}
