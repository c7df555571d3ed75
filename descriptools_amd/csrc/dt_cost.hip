// dt_cost.hip -- cost distance, cost allocation and back-links over a friction raster: the least accumulated cost from
// every cell to a source, the source it is reached from and the D8 code of the first step towards it (net-new;
// descriptools_amd/cost.py holds the definition; the GIS "cost distance / allocation / back link", GRASS r.cost).
//
// The cost A is the greatest solution of A(s) = 0 at the sources and A(v) = min over the passable neighbours u of
// fl(A(u) + w(u, v)) elsewhere, w(u, v) = step * ((f(u) + f(v)) * 0.5) in float64, one rounding per operation.  fl(a + w)
// is monotone in a and w >= 0, so any relaxation that starts at +inf reaches that solution, in any order and any tiling:
// the schedule is dt_tile_rounds.h's, the value of a cell is lowered many times instead of settled once (the D-infinity
// distance, dt_dinf_dist.hip, settles each cell once on the same schedule).
// k_cost_init   A = 0 at the sources (passable and sources == 1), +inf everywhere else.  A lives in the cost raster.
// k_cost_round  one workgroup per tile of 64 x 64 cells with a one-cell halo: A (float64) and the friction (float32, 0
//               on barriers and beyond the raster) of tile and halo go to LDS, 53 KB.  A sweep is two steps with a
//               barrier between them: every lane pulls the minimum over the neighbours of its 16 cells from LDS into
//               registers, then the lanes that found a lower value write it -- no lane reads what another is writing, no
//               atomics.  Sweeps repeat until one lowers nothing or `visit_limit` is reached; the cells that were
//               lowered go back to the cost raster.  The tile leaves an activity byte (dt_tile_rounds.h): HY_CHANGED
//               when a cell of its outer ring was lowered (what its neighbours read), HY_OPEN when the limit stopped
//               it; the round raises its flag word when it lowered anything.
// k_cost_link   from the final A: backlink = the ESRI code of the first neighbour u, in the order NW, N, NE, W, E, SW,
//               S, SE, with A(u) < A(v) and fl(A(u) + w(u, v)) == A(v) -- the same expression the rounds evaluated, so
//               tightness is a comparison of bits; that neighbour's flat index goes to the parent plane (a source is
//               its own parent, -1 for everything without one).  It counts the reached and the linkless cells, sums
//               the tile visits and raises the status bits.
// k_cost_fill   -100 on barriers and unreached cells (after k_cost_link, which reads the neighbours' A).
// k_cost_jump   pointer doubling on the parent plane, in place: A falls strictly along the links, so they form a forest
//               and every value a lane can read is an ancestor.  At most 31 passes (chains are shorter than 2^31); a
//               pass that moved nothing makes the passes after it return at once.
// k_cost_index  indices = the root as int64, -100 without one.
#include <cmath>

#include "dt_kernels.h"
#include "dt_tile_rounds.h"

#define CD_T 64
#define CD_LD (CD_T + 2)
#define CD_LS (CD_LD + 1)  // LDS row stride in cells
#define CD_CELLS (CD_LD * CD_LS)
#define CD_CPT (CD_T * CD_T / 256)
#define CD_JUMPS 31

// control words of one call
enum {
  CD_C_FLAGS = 0,  // DT_TILE_ROUNDS_MAX of them: round r raises word r when it lowered something
  CD_C_JUMP = DT_TILE_ROUNDS_MAX,  // CD_JUMPS + 1 of them: pass p raises word p when it moved a pointer
  CD_C_REACH = DT_COST_CTL_COUNTS,  // (CD_C_JUMP + 32)
  CD_C_NOLINK,
  CD_C_VISITS,  // 64 bits (8-byte aligned: CD_C_REACH is even)
  CD_C_WORDS = CD_C_REACH + 8
};

__device__ __forceinline__ bool cd_passable(float f) { return f > 0.0f && f < INFINITY; }
__device__ __forceinline__ bool cd_reached(double a) { return a >= 0.0 && a < (double)INFINITY; }
// the edge cost: float64, one rounding per operation (the library is built without contraction)
__device__ __forceinline__ double cd_edge(double step, float fu, float fv) {
  return step * (((double)fu + (double)fv) * 0.5);
}

__global__ __launch_bounds__(256) void k_cost_init(const float *__restrict__ friction,
                                                   const int8_t *__restrict__ sources, long long N,
                                                   double *__restrict__ cost) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  cost[c] = (sources[c] == 1 && cd_passable(friction[c])) ? 0.0 : (double)INFINITY;
}

// DIAG: connectivity 8
template <bool DIAG>
__global__ __launch_bounds__(256) void k_cost_round(const float *__restrict__ friction, double *__restrict__ cost,
                                                    int H, int W, double px, double pxd, int visit_limit,
                                                    const HyRound rnd) {
  __shared__ double s_a[CD_CELLS];
  __shared__ float s_f[CD_CELLS];
  int ty, tx;
  if (!hy_round_enter(rnd, ty, tx)) return;
  const int tile = ty * rnd.tiles_x + tx;
  const int y0 = ty * CD_T, x0 = tx * CD_T;
  // tile and halo: friction 0 (a barrier) beyond the raster and on every cell that is not passable
  for (int i = threadIdx.x; i < CD_LD * CD_LD; i += 256) {
    const int r = i / CD_LD, c = i - r * CD_LD;
    const int gy = y0 - 1 + r, gx = x0 - 1 + c;
    float f = 0.0f;
    double a = (double)INFINITY;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const long long g = (long long)gy * W + gx;
      f = friction[g];
      if (cd_passable(f)) a = cost[g];
      else f = 0.0f;
    }
    s_f[r * CD_LS + c] = f;
    s_a[r * CD_LS + c] = a;
  }
  __syncthreads();
  // this lane's cells: column lx, rows ly0 + 4 j
  const int lx = (int)threadIdx.x & (CD_T - 1), ly0 = (int)threadIdx.x >> 6;
  const int p0 = (ly0 + 1) * CD_LS + lx + 1;
  float fc[CD_CPT];
#pragma unroll
  for (int j = 0; j < CD_CPT; j++) fc[j] = s_f[p0 + 4 * j * CD_LS];
  const int sweeps_max = visit_limit > 0 ? visit_limit : 0x7fffffff;
  uint32_t dirty = 0u;  // bit j: cell j was lowered during this visit
  int open = 0;
  for (int sweep = 0; sweep < sweeps_max; sweep++) {
    double na[CD_CPT];
    uint32_t low = 0u;
#pragma unroll
    for (int j = 0; j < CD_CPT; j++) {
      na[j] = 0.0;
      if (!(fc[j] > 0.0f)) continue;
      const int p = p0 + 4 * j * CD_LS;
      const double old = s_a[p];
      double best = old;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int dy = k < 3 ? -1 : (k < 5 ? 0 : 1);
        const int dx = k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6));
        const bool diag = dy != 0 && dx != 0;
        if (diag && !DIAG) continue;
        const int q = p + dy * CD_LS + dx;
        const float fn = s_f[q];
        if (!(fn > 0.0f)) continue;
        const double cand = s_a[q] + cd_edge(diag ? pxd : px, fn, fc[j]);
        if (cand < best) best = cand;
      }
      if (best < old) {
        na[j] = best;
        low |= 1u << j;
      }
    }
    __syncthreads();  // every lane has read what it needs of this sweep's LDS
#pragma unroll
    for (int j = 0; j < CD_CPT; j++)
      if (low & (1u << j)) s_a[p0 + 4 * j * CD_LS] = na[j];
    dirty |= low;
    open = __syncthreads_or(low != 0u);
    if (!open) break;
  }
  // the lowered cells go back to the cost raster (all of them lie in the raster: beyond it fc is 0)
  int ring = 0;
#pragma unroll
  for (int j = 0; j < CD_CPT; j++) {
    if (!(dirty & (1u << j))) continue;
    const int ly = ly0 + 4 * j;
    cost[(long long)(y0 + ly) * W + (x0 + lx)] = s_a[p0 + 4 * j * CD_LS];
    ring |= (ly == 0 || ly == CD_T - 1 || lx == 0 || lx == CD_T - 1) ? 1 : 0;
  }
  const int any = __syncthreads_or(dirty != 0u);
  ring = __syncthreads_or(ring);
  // open: the limit ended the visit while a sweep still lowered something
  hy_round_leave(rnd, tile, (ring ? HY_CHANGED : 0) | (open ? HY_OPEN : 0), any);
}

// last_flag: the flag word of the last round enqueued before this kernel (NULL: the caller looked at the flags itself)
template <bool DIAG>
__global__ __launch_bounds__(256) void k_cost_link(const float *__restrict__ friction,
                                                   const int8_t *__restrict__ sources,
                                                   const double *__restrict__ cost, int H, int W, double px, double pxd,
                                                   uint8_t *__restrict__ backlink, int32_t *__restrict__ parent,
                                                   const uint32_t *__restrict__ visits, int tiles,
                                                   const int *__restrict__ last_flag, uint32_t *__restrict__ ctl,
                                                   int *__restrict__ status) {
  const long long N = (long long)H * W;
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  bool reached = false, nolink = false;
  if (c < N) {
    const int y = (int)(c / W), x = (int)(c - (long long)y * W);
    const float f = friction[c];
    const double a = cost[c];
    uint32_t code = 0u;
    int32_t par = -1;
    if (cd_passable(f) && cd_reached(a)) {
      reached = true;
      if (sources[c] == 1) {
        par = (int32_t)c;
      } else {
        // NW, N, NE, W, E, SW, S, SE
        const uint32_t codes = 32u | 64u << 8 | 128u << 16 | 16u << 24;
        const uint32_t codes2 = 1u | 8u << 8 | 4u << 16 | 2u << 24;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int dy = k < 3 ? -1 : (k < 5 ? 0 : 1);
          const int dx = k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6));
          const bool diag = dy != 0 && dx != 0;
          if (diag && !DIAG) continue;
          const int ny = y + dy, nx = x + dx;
          if (code != 0u || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
          const long long g = (long long)ny * W + nx;
          const float fn = friction[g];
          if (!cd_passable(fn)) continue;
          const double an = cost[g];
          if (!(an < a)) continue;
          if (an + cd_edge(diag ? pxd : px, fn, f) == a) {
            code = ((k < 4 ? codes : codes2) >> (8 * (k & 3))) & 255u;
            par = (int32_t)g;
          }
        }
        nolink = code == 0u;
      }
    }
    if (backlink) backlink[c] = (uint8_t)code;
    if (parent) parent[c] = par;
  }
  const int nr = __syncthreads_count(reached), nl = __syncthreads_count(nolink);
  hy_visits_sum(visits, tiles, &ctl[CD_C_VISITS]);
  if (threadIdx.x == 0) {
    if (nr) atomicAdd(&ctl[CD_C_REACH], (uint32_t)nr);
    if (nl) atomicAdd(&ctl[CD_C_NOLINK], (uint32_t)nl);
    if (status && nl) atomicOr(status, DT_STATUS_NO_BACKLINK);
    if (status && blockIdx.x == 0 && last_flag && *last_flag) atomicOr(status, DT_STATUS_NOT_CONVERGED);
  }
}

__global__ __launch_bounds__(256) void k_cost_fill(const float *__restrict__ friction, long long N,
                                                   double *__restrict__ cost) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  if (!(cd_passable(friction[c]) && cd_reached(cost[c]))) cost[c] = -100.0;
}

// One pass of pointer doubling, in place.  Another lane may be moving parent[u] while this one reads it: both the old
// and the new value are ancestors of u (32-bit words are read and written whole), so the pointer only moves rootwards.
__global__ __launch_bounds__(256) void k_cost_jump(int32_t *__restrict__ parent, long long N, int *__restrict__ moved,
                                                   const int *__restrict__ prev) {
  if (prev && *prev == 0) return;
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  int m = 0;
  if (c < N) {
    const int32_t u = parent[c];
    if (u >= 0 && u != (int32_t)c) {
      const int32_t g = ((volatile int32_t *)parent)[u];
      if (g != u) {  // u is no root: its parent, or -1 when the chain ends in a cell without a link
        ((volatile int32_t *)parent)[c] = g;
        m = 1;
      }
    }
  }
  if (__syncthreads_or(m) && threadIdx.x == 0) *moved = 1;
}

__global__ __launch_bounds__(256) void k_cost_index(const int32_t *__restrict__ parent, long long N,
                                                    int64_t *__restrict__ indices) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int32_t r = parent[c];
  indices[c] = r >= 0 ? (int64_t)r : (int64_t)-100;
}

// ---- launcher ------------------------------------------------------------------------------------------------------
struct CdLayout {
  HyRoundsScratch r;
  int32_t *parent;  // with `alloc` only
  size_t bytes;
};
static CdLayout cd_layout(int64_t H, int64_t W, bool alloc, void *scratch) {
  CdLayout L = {};
  DtCarver c(scratch);
  L.r = hy_rounds_take(c, H, W, CD_T, CD_C_WORDS);
  L.parent = alloc ? c.take<int32_t>((size_t)(H * W)) : nullptr;
  L.bytes = c.bytes();
  return L;
}
size_t dt_cost_distance_scratch(int64_t H, int64_t W, int alloc) { return cd_layout(H, W, alloc != 0, nullptr).bytes; }
const uint32_t *dt_cost_distance_ctl(void *scratch, int64_t H, int64_t W, int alloc) {
  return cd_layout(H, W, alloc != 0, scratch).r.ctl;
}

int dt_launch_cost_distance(hipStream_t s, const float *friction, const int8_t *sources, int64_t H, int64_t W,
                            double px, int connectivity, int visit_limit, int start, int rounds, int finish,
                            void *scratch, size_t scratch_bytes, double *cost, int64_t *indices, uint8_t *backlink,
                            int *status) {
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity is 4 or 8");
  DT_REQUIRE(visit_limit >= 0, "visit_limit is negative");
  DT_REQUIRE(rounds >= 0 && rounds <= DT_TILE_ROUNDS_MAX, "bad number of rounds");
  const int64_t N = H * W;
  const CdLayout L = cd_layout(H, W, indices != nullptr, scratch);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const dim3 b(256);
  const dim3 cells((unsigned)((N + 255) / 256));
  const bool diag = connectivity == 8;
  const double pxd = px * 1.4142135623730951;
  uint32_t *ctl = L.r.ctl;
  if (start) hipLaunchKernelGGL(k_cost_init, cells, b, 0, s, friction, sources, (long long)N, cost);
  DT_TRY(hy_launch_rounds(s, L.r, ctl + CD_C_FLAGS, start, rounds, [&](dim3 blocks, const HyRound &rnd) {
    if (diag)
      hipLaunchKernelGGL(k_cost_round<true>, blocks, b, 0, s, friction, cost, (int)H, (int)W, px, pxd, visit_limit, rnd);
    else
      hipLaunchKernelGGL(k_cost_round<false>, blocks, b, 0, s, friction, cost, (int)H, (int)W, px, pxd, visit_limit, rnd);
  }));
  if (finish) {
    DT_HIP(hipMemsetAsync(ctl + CD_C_JUMP, 0, sizeof(uint32_t) * (CD_C_WORDS - CD_C_JUMP), s));
    // (finish with rounds: the device tier, which says so when its last round still lowered something)
    const int *last = rounds ? (const int *)ctl + CD_C_FLAGS + rounds - 1 : nullptr;
    if (diag)
      hipLaunchKernelGGL(k_cost_link<true>, cells, b, 0, s, friction, sources, (const double *)cost, (int)H, (int)W, px,
                         pxd, backlink, L.parent, (const uint32_t *)L.r.visits, (int)L.r.tiles(), last, ctl, status);
    else
      hipLaunchKernelGGL(k_cost_link<false>, cells, b, 0, s, friction, sources, (const double *)cost, (int)H, (int)W,
                         px, pxd, backlink, L.parent, (const uint32_t *)L.r.visits, (int)L.r.tiles(), last, ctl, status);
    hipLaunchKernelGGL(k_cost_fill, cells, b, 0, s, friction, (long long)N, cost);
    if (indices) {
      for (int p = 0; p < CD_JUMPS; p++) {
        int *moved = (int *)ctl + CD_C_JUMP + p;
        hipLaunchKernelGGL(k_cost_jump, cells, b, 0, s, L.parent, (long long)N, moved, p ? moved - 1 : nullptr);
      }
      hipLaunchKernelGGL(k_cost_index, cells, b, 0, s, (const int32_t *)L.parent, (long long)N, indices);
    }
  }
  return DT_OK;
}
