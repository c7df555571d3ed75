// dt_harmonic.hip -- harmonic interpolation on a masked raster: the discrete harmonic function with some cells held
// fixed and zero flux at nodata and at the raster's edge (net-new; descriptools_amd/harmonic.py holds the definition;
// void filling, SAGA's "channel network base level" and the vertical distance to channel network are built on it).
//
// Definition.  values float32 (widened to float64), fixed int8, domain int8 or NULL (everywhere).  A cell is FIXED iff
// fixed == 1 and its value is finite; a fixed cell is in the domain, a cell with fixed == 1 and a non-finite value is
// outside it, every other cell is in the domain iff domain != 0.  The values of free cells are never read.  On every
// free cell v of the domain that has k >= 1 of its four edge neighbours (N, W, E, S) in the domain: s = the sum of those
// neighbours' u in that order, left to right, one rounding per addition; avg = s / k in float64, one division; r(v) =
// |avg - u(v)|.  u solves r = 0, fixed cells hold their value.  Connectivity is 4.
// Precondition: every free cell of the domain is joined to a fixed cell by a 4-connected path through the domain
// (harmonic.py removes the others with regions.connected).  Without it such cells settle on an unspecified constant;
// every loop here is bounded by the sweep count or the budget of rounds, so the call still ends.
// What a call leaves: fixed cells carry their value exactly, NaN outside the domain, and max r <= tol over the solved
// cells, with r evaluated by exactly the expression above -- or the last residual says that the budget ran out.  The same
// bits on every run: coloured rounds, red-black sweeps with a barrier between the half-sweeps, no float atomics.  WHICH
// iterate passes the residual test depends on the schedule below, so equality with another solver is no part of the
// contract.
//
// The solver is nested iteration (cascadic multigrid): a pyramid by 2 down to a raster of at most one tile, the coarsest
// level solved from its fixed values spread outwards, every level handing its result up by injection.
// k_hm_init      level 0: the mask byte (HM_DOM, HM_FIX) of every cell; u = the value on fixed cells, NaN outside the
//                domain, 0 on free cells (injection overwrites it).  u of level 0 is the output raster.
// k_hm_restrict  one launch per level, no atomics: a coarse cell (Y, X) has the children (2Y, 2X), (2Y, 2X + 1),
//                (2Y + 1, 2X), (2Y + 1, 2X + 1) that lie in the finer raster (ceil on odd sizes); it is in the domain if
//                any child is, fixed if any child is fixed, with the mean of its fixed children summed in that order.
//                A path to a fixed cell survives coarsening, so the precondition holds on every level.
// k_hm_flood     the coarsest level (at most one tile) starts from its fixed values spread outwards: one workgroup, the
//                level in LDS; in every step each free cell without a value takes that of its first neighbour, in the
//                order N, W, E, S, that had one before the step (pull, barrier, commit), until a step sets nothing --
//                at most as many steps as the level has cells.  So a part of the domain that stays closed off on every
//                level starts from its own fixed values only: with a single one it IS that constant, exactly, and
//                stays so (sums of 2, 3 and 4 copies of a float32 value and their quotients are exact).  A wall
//                thinner than the coarsest cell does not survive coarsening (a coarse cell merges both sides of it);
//                behind such a wall the start is only as good as that.
// k_hm_start     level_cap only (benchmarks), when the coarsest level is larger than a tile: its free cells start from
//                the least fixed value (0 without a fixed cell).
// k_hm_prolong   a free child takes its parent's value.
// k_hm_round     the smoother: one workgroup per tile of 64 x 64 cells with a one-cell halo; u (float64) and the mask
//                byte of tile and halo go to LDS, 39.1 KB.  HM_SWEEPS (4; 64 on a level of one tile) red-black
//                sweeps run from LDS, colour = (y + x) & 1, a barrier after each half-sweep: a cell reads only cells
//                of the other colour, so no lane reads what another is writing.  The update is over-relaxed and
//                clamped, u <- min(max(u + HM_OMEGA * (avg - u), lo), hi) with HM_OMEGA = 1.95 and [lo, hi] the range of
//                the fixed values (k_hm_init: two atomics on order-preserving keys): the solution lies in that range,
//                so the clamp does not move the fixed point (avg == u stays put, whatever the factor) and every
//                iterate on every level stays within [lo, hi] -- the coarse fixed values are means of input values (for
//                float32 inputs k * max is a float64: rounding cannot carry a mean past it), the start copies them.
//                Each single update lowers the energy of the symmetric positive definite system for any factor in
//                (0, 2) and any order of the cells, so the rounds converge whatever the tiling.  A tile in which no
//                solved cell has three neighbours never divides.  Changed cells go back to global memory.
//                The schedule is dt_tile_rounds.h's, with the residual key of the round before in place of its flag
//                word: a tile rests while neither it (HY_OPEN: its last sweep still changed a bit) nor its halo
//                (HY_CHANGED: a neighbour's outer ring changed) moved.  HM_DIRTY says that the visit wrote anything at
//                all (the residual's reuse rule).
// k_hm_residual  after each round: the maximum of r over the level's solved cells, one workgroup per tile, one 64-bit
//                integer atomic maximum per workgroup on the bits of r (r >= 0: its bits order as it does) into the
//                round's key word, skipped when the word already holds as much.  A tile whose cells and halo did not
//                change since its last evaluation reuses that value.  The level ends when the key is <= tol's: the
//                launches of every later round see that in the key word before theirs and return at once, the residual
//                kernel handing the key on, so the word of the last round enqueued holds the level's last residual.
//                A coarse level whose budget runs out hands on what it has; only level 0's residual is the contract's.
// k_hm_finish    rounds per level, their sum, the tile visits and the last residual into the info block;
//                DT_STATUS_NOT_CONVERGED when level 0's last residual exceeds tol.
// No kernel waits on another workgroup.
#include <cmath>

#include "dt_kernels.h"
#include "dt_tile_rounds.h"

#define HM_T 64
#define HM_LD (HM_T + 2)
#define HM_LS (HM_LD + 1)  // LDS row stride in cells
#define HM_CELLS (HM_LD * HM_LS)
#define HM_CPT (HM_T * HM_T / 256)  // cells per lane: 8 of each colour
#define HM_SWEEPS 4                 // red-black sweeps per tile visit
#define HM_SWEEPS_ONE 64            // on a level that is a single tile
#define HM_OMEGA 1.95               // the relaxation factor: u += HM_OMEGA * (avg - u)
#define HM_DOM 1
#define HM_FIX 2
#define HM_DIRTY 4  // activity byte, beside HY_CHANGED and HY_OPEN: the visit wrote a cell
// a cell's code in the smoother: which neighbours are in the domain, and whether the cell is solved
#define HM_N 1
#define HM_W 2
#define HM_E 4
#define HM_S 8
#define HM_SOLVED 16

typedef unsigned long long hm_key_t;
static_assert(DT_HARMONIC_INFO == DT_HARMONIC_INFO_WORDS, "the info block of the header");

// the bits of a residual (>= 0, never NaN: every u is finite): they order as the doubles do
__device__ __forceinline__ hm_key_t hm_res_key(double r) { return (hm_key_t)__double_as_longlong(r); }
// order-preserving key of any double but NaN
__device__ __forceinline__ hm_key_t hm_order_key(double v) {
  const hm_key_t b = (hm_key_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double hm_order_value(hm_key_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
// avg of the definition.  A neighbour outside the domain is handed in as 0: x + 0 is x, so the plain sum in the order N,
// W, E, S is the sum of the definition, one rounding per addition of a neighbour that counts; then the one division.
// DIV3 false: for a caller that knows k != 3 -- the product with 1, 0.5 or 0.25 is the same correctly rounded quotient,
// and a float64 division is some thirty instructions.
template <bool DIV3>
__device__ __forceinline__ double hm_average(uint32_t code, double n, double w, double e, double s) {
  const double sum = ((n + w) + e) + s;
  const int k = __popc(code & 15u);
  if (DIV3) return sum / (double)k;
  return sum * (k == 4 ? 0.25 : (k == 2 ? 0.5 : 1.0));
}

// range (before: all ones, 0): the order keys of the least and the greatest fixed value, two integer atomics per
// workgroup at most, skipped when the word already holds as much
__global__ __launch_bounds__(256) void k_hm_init(const float *__restrict__ values, const int8_t *__restrict__ fixed,
                                                 const int8_t *__restrict__ domain, long long N,
                                                 double *__restrict__ u, uint8_t *__restrict__ m,
                                                 hm_key_t *__restrict__ range) {
  __shared__ hm_key_t s_lo, s_hi;
  if (threadIdx.x == 0) {
    s_lo = ~0ull;
    s_hi = 0ull;
  }
  __syncthreads();
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c < N) {
    const bool fx = fixed[c] == 1;
    const float v = fx ? values[c] : 0.0f;
    const bool fin = fabsf(v) < INFINITY;  // (false for NaN)
    const bool dom = fx ? fin : (domain ? domain[c] != 0 : true);
    m[c] = (uint8_t)((dom ? HM_DOM : 0) | (fx && fin ? HM_FIX : 0));
    u[c] = (fx && fin) ? (double)v : (dom ? 0.0 : (double)NAN);
    if (fx && fin) {
      const hm_key_t k = hm_order_key((double)v);
      atomicMin(&s_lo, k);
      atomicMax(&s_hi, k);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_lo != ~0ull) {
    if (s_lo < *(volatile hm_key_t *)&range[0]) atomicMin(&range[0], s_lo);
    if (s_hi > *(volatile hm_key_t *)&range[1]) atomicMax(&range[1], s_hi);
  }
}

__global__ __launch_bounds__(256) void k_hm_restrict(const double *__restrict__ uf, const uint8_t *__restrict__ mf,
                                                     int Hf, int Wf, double *__restrict__ uc,
                                                     uint8_t *__restrict__ mc, int Hc, int Wc) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= (long long)Hc * Wc) return;
  const int Y = (int)(c / Wc), X = (int)(c - (long long)Y * Wc);
  uint32_t any = 0u;
  int nfix = 0;
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int y = 2 * Y + (k >> 1), x = 2 * X + (k & 1);
    if (y >= Hf || x >= Wf) continue;
    const long long g = (long long)y * Wf + x;
    const uint32_t mm = mf[g];
    any |= mm;
    if (mm & HM_FIX) {
      sum += uf[g];
      nfix++;
    }
  }
  mc[c] = (uint8_t)(any & (HM_DOM | HM_FIX));
  uc[c] = nfix ? sum / (double)nfix : 0.0;
}

// level_cap only: the free cells of a coarsest level of more than one tile start from the least fixed value
__global__ __launch_bounds__(256) void k_hm_start(double *__restrict__ u, const uint8_t *__restrict__ m, long long N,
                                                  const hm_key_t *__restrict__ range) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const hm_key_t k = range[0];
  if ((m[c] & (HM_DOM | HM_FIX)) == HM_DOM) u[c] = k == ~0ull ? 0.0 : hm_order_value(k);
}

// One workgroup; H, W <= HM_T.
__global__ __launch_bounds__(256) void k_hm_flood(double *__restrict__ u, const uint8_t *__restrict__ m, int H, int W) {
  __shared__ double s_u[HM_LD * HM_LS];
  __shared__ uint8_t s_set[HM_LD * HM_LS];  // 1: the cell has a value (halo and cells beyond the level: never)
  for (int i = threadIdx.x; i < HM_LD * HM_LS; i += 256) {
    s_set[i] = 0;
    s_u[i] = 0.0;
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & (HM_T - 1), ly0 = (int)threadIdx.x >> 6;
  const int p0 = (ly0 + 1) * HM_LS + lx + 1;
  uint32_t want = 0u;  // bit j: cell j is a free cell of the domain without a value
#pragma unroll
  for (int j = 0; j < HM_CPT; j++) {
    const int y = ly0 + 4 * j;
    if (y >= H || lx >= W) continue;
    const uint32_t mm = m[y * W + lx];
    if (mm & HM_FIX) {
      s_set[p0 + 4 * j * HM_LS] = 1;
      s_u[p0 + 4 * j * HM_LS] = u[y * W + lx];
    } else if (mm & HM_DOM) {
      want |= 1u << j;
    }
  }
  __syncthreads();
  for (int step = 0; step < H * W; step++) {
    double nv[HM_CPT];
    uint32_t got = 0u;
#pragma unroll
    for (int j = 0; j < HM_CPT; j++) {
      nv[j] = 0.0;
      if (!(want & (1u << j))) continue;
      const int p = p0 + 4 * j * HM_LS;
      const int q = s_set[p - HM_LS] ? p - HM_LS
                                     : (s_set[p - 1] ? p - 1 : (s_set[p + 1] ? p + 1 : (s_set[p + HM_LS] ? p + HM_LS : -1)));
      if (q >= 0) {
        nv[j] = s_u[q];
        got |= 1u << j;
      }
    }
    __syncthreads();  // every lane has read what it needs of this step's LDS
#pragma unroll
    for (int j = 0; j < HM_CPT; j++)
      if (got & (1u << j)) {
        s_u[p0 + 4 * j * HM_LS] = nv[j];
        s_set[p0 + 4 * j * HM_LS] = 1;
      }
    want &= ~got;
    if (!__syncthreads_or(got != 0u)) break;
  }
#pragma unroll
  for (int j = 0; j < HM_CPT; j++) {
    const int y = ly0 + 4 * j;
    if (y >= H || lx >= W) continue;
    if ((m[y * W + lx] & (HM_DOM | HM_FIX)) == HM_DOM) u[y * W + lx] = s_u[p0 + 4 * j * HM_LS];  // (0 without a value)
  }
}

__global__ __launch_bounds__(256) void k_hm_prolong(const double *__restrict__ uc, int Wc, double *__restrict__ uf,
                                                    const uint8_t *__restrict__ mf, int Hf, int Wf) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= (long long)Hf * Wf) return;
  if ((mf[c] & (HM_DOM | HM_FIX)) != HM_DOM) return;
  const int y = (int)(c / Wf), x = (int)(c - (long long)y * Wf);
  uf[c] = uc[(long long)(y >> 1) * Wc + (x >> 1)];
}

// The sweeps of one tile visit, from LDS; -> whether the last sweep still changed a bit.  Every lane of the workgroup
// calls it with the same DIV3 and the same `sweeps`.
template <bool DIV3>
__device__ __forceinline__ int hm_sweeps(double *s_u, const uint32_t (&codes)[2][2], int lr, int lc, int sweeps,
                                         double lo, double hi, uint32_t &dirty) {
  int open = 0;
  for (int sweep = 0; sweep < sweeps; sweep++) {
    int ch = 0;
#pragma unroll
    for (int col = 0; col < 2; col++) {
#pragma unroll
      for (int j = 0; j < HM_CPT / 2; j++) {
        // without a branch: a cell that is not solved is written back as it is (nobody reads this colour now)
        const uint32_t code = (codes[col][j >> 2] >> (8 * (j & 3))) & 255u;
        const int ly = lr + 8 * j, lx = 2 * lc + ((ly + col) & 1);
        const int p = (ly + 1) * HM_LS + lx + 1;
        const double old = s_u[p];
        const double avg = hm_average<DIV3>(code, s_u[p - HM_LS], s_u[p - 1], s_u[p + 1], s_u[p + HM_LS]);
        const double now = (code & HM_SOLVED) ? fmin(fmax(old + HM_OMEGA * (avg - old), lo), hi) : old;
        s_u[p] = now;
        const uint32_t moved = now != old ? 1u : 0u;
        dirty |= moved << (8 * col + j);
        ch |= (int)moved;
      }
      if (col == 0) __syncthreads();
    }
    open = __syncthreads_or(ch);  // (the barrier after the second half-sweep)
    if (!open) break;
  }
  return open;
}

// prev_key: the key word of the round before this one (NULL: the level's first round); rnd: without flag words
__global__ __launch_bounds__(256) void k_hm_round(double *__restrict__ u, const uint8_t *__restrict__ m, int H, int W,
                                                  const hm_key_t *__restrict__ prev_key, hm_key_t tol_key,
                                                  const hm_key_t *__restrict__ range, int sweeps, const HyRound rnd) {
  __shared__ double s_u[HM_CELLS];
  __shared__ uint8_t s_m[HM_CELLS];
  // (the previous round's key was completed by the previous kernels: a plain load sees it)
  if (prev_key && *prev_key <= tol_key) return;
  int ty, tx;
  if (!hy_round_tile(rnd, ty, tx)) return;
  const int tile = ty * rnd.tiles_x + tx;
  const int y0 = ty * HM_T, x0 = tx * HM_T;
  // tile and halo: beyond the raster nothing is in the domain
  for (int i = threadIdx.x; i < HM_LD * HM_LD; i += 256) {
    const int r = i / HM_LD, c = i - r * HM_LD;
    const int gy = y0 - 1 + r, gx = x0 - 1 + c;
    uint8_t mm = 0;
    double a = 0.0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const long long g = (long long)gy * W + gx;
      mm = m[g];
      if (mm & HM_DOM) a = u[g];
    }
    s_m[r * HM_LS + c] = mm;
    s_u[r * HM_LS + c] = a;
  }
  __syncthreads();
  // this lane's cells: rows lr + 8 j, j = 0..7; in each the cell of columns 2 lc, 2 lc + 1 whose colour is the
  // half-sweep's (the tile's origin is even in both coordinates: the local parity is the raster's)
  const int lc = (int)threadIdx.x & 31, lr = (int)threadIdx.x >> 5;
  uint32_t codes[2][2] = {{0u, 0u}, {0u, 0u}};  // [colour][j >> 2], a byte per cell
  int three = 0;
#pragma unroll
  for (int col = 0; col < 2; col++)
#pragma unroll
    for (int j = 0; j < HM_CPT / 2; j++) {
      const int ly = lr + 8 * j, lx = 2 * lc + ((ly + col) & 1);
      const int p = (ly + 1) * HM_LS + lx + 1;
      uint32_t code = 0u;
      if (s_m[p - HM_LS] & HM_DOM) code |= HM_N;
      if (s_m[p - 1] & HM_DOM) code |= HM_W;
      if (s_m[p + 1] & HM_DOM) code |= HM_E;
      if (s_m[p + HM_LS] & HM_DOM) code |= HM_S;
      if ((s_m[p] & (HM_DOM | HM_FIX)) == HM_DOM && code) code |= HM_SOLVED;
      three |= ((code & HM_SOLVED) && __popc(code & 15u) == 3) ? 1 : 0;
      codes[col][j >> 2] |= code << (8 * (j & 3));
    }
  // (a tile without a solved cell of three neighbours -- all of them, away from nodata and the raster's edge -- never
  // divides)
  uint32_t dirty = 0u;  // bit 8 col + j: the cell was written during this visit
  const hm_key_t klo = range[0], khi = range[1];
  const double lo = klo == ~0ull ? -(double)INFINITY : hm_order_value(klo);  // (no fixed cell: no bounds)
  const double hi = klo == ~0ull ? (double)INFINITY : hm_order_value(khi);
  const int open = __syncthreads_or(three) ? hm_sweeps<true>(s_u, codes, lr, lc, sweeps, lo, hi, dirty)
                                           : hm_sweeps<false>(s_u, codes, lr, lc, sweeps, lo, hi, dirty);
  // the written cells go back (all of them lie in the raster: beyond it nothing is solved)
  int ring = 0;
#pragma unroll
  for (int col = 0; col < 2; col++)
#pragma unroll
    for (int j = 0; j < HM_CPT / 2; j++) {
      if (!(dirty & (1u << (8 * col + j)))) continue;
      const int ly = lr + 8 * j, lx = 2 * lc + ((ly + col) & 1);
      u[(long long)(y0 + ly) * W + (x0 + lx)] = s_u[(ly + 1) * HM_LS + lx + 1];
      ring |= (ly == 0 || ly == HM_T - 1 || lx == 0 || lx == HM_T - 1) ? 1 : 0;
    }
  const int any = __syncthreads_or(dirty != 0u);
  ring = __syncthreads_or(ring);
  hy_round_leave(rnd, tile, (ring ? HY_CHANGED : 0) | (open ? HY_OPEN : 0) | (any ? HM_DIRTY : 0), 0);
}

// One workgroup per tile.  first: the level's first round (no tile has a stored value yet).
__global__ __launch_bounds__(256) void k_hm_residual(const double *__restrict__ u, const uint8_t *__restrict__ m, int H,
                                                     int W, int tiles_x, int tiles_y, const uint8_t *__restrict__ act,
                                                     int first, hm_key_t *__restrict__ tile_key,
                                                     const hm_key_t *__restrict__ prev_key, hm_key_t tol_key,
                                                     hm_key_t *__restrict__ key) {
  __shared__ hm_key_t s_k;
  if (prev_key && *prev_key <= tol_key) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *key = *prev_key;  // (no other workgroup writes the word in this launch)
    return;
  }
  const int tile = (int)blockIdx.x;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  if (threadIdx.x == 0) s_k = 0ull;
  // evaluate again when the tile's last visit wrote a cell or a neighbour's wrote its outer ring (act is never NULL:
  // the test ends on the barrier that s_k needs)
  const bool again = hy_tile_active(act, ty, tx, tiles_x, tiles_y, HM_DIRTY) || first;
  if (again) {
    const int lx = (int)threadIdx.x & (HM_T - 1), x = tx * HM_T + lx;
    hm_key_t k = 0ull;
    for (int ly = (int)threadIdx.x >> 6; ly < HM_T; ly += 4) {
      const int y = ty * HM_T + ly;
      if (y >= H || x >= W) continue;
      const long long g = (long long)y * W + x;
      if ((m[g] & (HM_DOM | HM_FIX)) != HM_DOM) continue;
      uint32_t code = 0u;
      double n = 0.0, w = 0.0, e = 0.0, s = 0.0;
      if (y > 0 && (m[g - W] & HM_DOM)) { code |= HM_N; n = u[g - W]; }
      if (x > 0 && (m[g - 1] & HM_DOM)) { code |= HM_W; w = u[g - 1]; }
      if (x < W - 1 && (m[g + 1] & HM_DOM)) { code |= HM_E; e = u[g + 1]; }
      if (y < H - 1 && (m[g + W] & HM_DOM)) { code |= HM_S; s = u[g + W]; }
      if (!code) continue;
      const hm_key_t q = hm_res_key(fabs(hm_average<true>(code, n, w, e, s) - u[g]));
      k = q > k ? q : k;
    }
    if (k) atomicMax(&s_k, k);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const hm_key_t k = again ? s_k : tile_key[tile];
    if (again) tile_key[tile] = k;
    if (k > *(volatile hm_key_t *)key) atomicMax(key, k);
  }
}

// One workgroup.  keys: `levels` rows of `stride` key words, one per round of the budget.
__global__ __launch_bounds__(256) void k_hm_finish(const hm_key_t *__restrict__ keys, int levels, int stride,
                                                   hm_key_t tol_key,
                                                   const uint32_t *__restrict__ visits, long long tiles_all,
                                                   int64_t *__restrict__ info, int *__restrict__ status) {
  __shared__ unsigned long long s_visits;
  __shared__ int s_rounds[DT_HARMONIC_LEVELS_MAX];
  if (threadIdx.x == 0) s_visits = 0ull;
  if (threadIdx.x < DT_HARMONIC_LEVELS_MAX) s_rounds[threadIdx.x] = 0;
  __syncthreads();
  // round r of a level ran when it is the first or the round before it left a residual above tol (a round that was
  // never enqueued left 0)
  for (int l = 0; l < levels; l++) {
    int n = 0;
    for (int r = threadIdx.x; r < stride; r += 256)
      if (r == 0 || keys[(size_t)l * stride + r - 1] > tol_key) n++;
    if (n) atomicAdd(&s_rounds[l], n);
  }
  unsigned long long v = 0ull;
  for (long long t = threadIdx.x; t < tiles_all; t += 256) v += visits[t];
  if (v) atomicAdd(&s_visits, v);
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t all = 0;
    for (int l = 0; l < levels; l++) {
      all += s_rounds[l];
      info[DT_HARMONIC_INFO_LEVEL0 + l] = s_rounds[l];
    }
    for (int l = levels; l < DT_HARMONIC_LEVELS_MAX; l++) info[DT_HARMONIC_INFO_LEVEL0 + l] = 0;
    const hm_key_t last = keys[s_rounds[0] - 1];  // (level 0's row is the first; it ran at least one round)
    info[0] = levels;
    info[1] = s_rounds[0];
    info[2] = all;
    info[3] = (int64_t)s_visits;
    info[4] = (int64_t)last;
    info[5] = last <= tol_key ? 1 : 0;
    info[6] = info[7] = 0;
    if (status && last > tol_key) atomicOr(status, DT_STATUS_NOT_CONVERGED);
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
struct HmLevel {
  int H, W, tiles_x, tiles_y;
  double *u;  // level 0: the output raster
  uint8_t *m;
  uint8_t *act;
  uint32_t *visits;
  hm_key_t *tile_key;
  hm_key_t *keys;  // max_rounds words: the residual after each round
};
struct HmLayout {
  int levels;
  HmLevel lv[DT_HARMONIC_LEVELS_MAX];
  hm_key_t *keys;     // levels x max_rounds
  hm_key_t *range;    // the order keys of the least and the greatest fixed value
  int64_t *info;      // DT_HARMONIC_INFO words
  uint32_t *visits;   // every level's, level 0 first
  size_t tiles_all;
  size_t bytes;
};
static HmLayout hm_layout(int64_t H, int64_t W, int max_rounds, int level_cap, void *scratch, double *out) {
  HmLayout L = {};
  int64_t h = H, w = W;
  L.levels = 0;
  for (;;) {
    HmLevel &v = L.lv[L.levels++];
    v.H = (int)h;
    v.W = (int)w;
    v.tiles_x = (int)((w + HM_T - 1) / HM_T);
    v.tiles_y = (int)((h + HM_T - 1) / HM_T);
    L.tiles_all += (size_t)v.tiles_x * (size_t)v.tiles_y;
    if ((h <= HM_T && w <= HM_T) || L.levels == DT_HARMONIC_LEVELS_MAX || (level_cap > 0 && L.levels == level_cap))
      break;
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  DtCarver c(scratch);
  L.keys = c.take<hm_key_t>((size_t)L.levels * (size_t)max_rounds);
  L.range = c.take<hm_key_t>(2);
  L.info = c.take<int64_t>(DT_HARMONIC_INFO);
  L.visits = c.take<uint32_t>(L.tiles_all);
  size_t t0 = 0;
  for (int l = 0; l < L.levels; l++) {
    HmLevel &v = L.lv[l];
    const size_t cells = (size_t)v.H * (size_t)v.W, tiles = (size_t)v.tiles_x * (size_t)v.tiles_y;
    v.u = l ? c.take<double>(cells) : out;
    v.m = c.take<uint8_t>(cells);
    v.act = c.take<uint8_t>(tiles);
    v.tile_key = c.take<hm_key_t>(tiles);
    v.visits = L.visits ? L.visits + t0 : nullptr;
    v.keys = L.keys ? L.keys + (size_t)l * (size_t)max_rounds : nullptr;
    t0 += tiles;
  }
  L.bytes = c.bytes();
  return L;
}
static int hm_check(int64_t H, int64_t W, int max_rounds, int level_cap) {
  DT_REQUIRE(H > 0 && W > 0 && H * W < (1ll << 31), "bad raster shape");
  DT_REQUIRE(max_rounds >= 1 && max_rounds <= DT_TILE_ROUNDS_MAX, "max_rounds must lie in [1, 4096]");
  DT_REQUIRE(level_cap >= 0, "level_cap is negative");
  return DT_OK;
}
static hm_key_t hm_host_key(double tol) {
  hm_key_t k;
  memcpy(&k, &tol, sizeof(k));
  return k;
}

size_t dt_harmonic_scratch(int64_t H, int64_t W, int max_rounds, int level_cap) {
  return hm_layout(H, W, max_rounds, level_cap, nullptr, nullptr).bytes;
}
int dt_harmonic_levels(int64_t H, int64_t W, int level_cap) {
  return hm_layout(H, W, 1, level_cap, nullptr, nullptr).levels;
}
const unsigned long long *dt_harmonic_keys(void *scratch, int64_t H, int64_t W, int max_rounds, int level_cap,
                                           int level) {
  return hm_layout(H, W, max_rounds, level_cap, scratch, nullptr).lv[level].keys;
}
const int64_t *dt_harmonic_info(void *scratch, int64_t H, int64_t W, int max_rounds, int level_cap) {
  return hm_layout(H, W, max_rounds, level_cap, scratch, nullptr).info;
}

static unsigned hm_blocks(size_t cells) { return (unsigned)((cells + 255) / 256); }

int dt_launch_harmonic_setup(hipStream_t s, const float *values, const int8_t *fixed, const int8_t *domain, int64_t H,
                             int64_t W, int max_rounds, int level_cap, void *scratch, size_t scratch_bytes,
                             double *out) {
  DT_TRY(hm_check(H, W, max_rounds, level_cap));
  const HmLayout L = hm_layout(H, W, max_rounds, level_cap, scratch, out);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const dim3 b(256);
  DT_HIP(hipMemsetAsync(L.keys, 0, sizeof(hm_key_t) * (size_t)L.levels * (size_t)max_rounds, s));
  DT_HIP(hipMemsetAsync(L.range, 0xff, sizeof(hm_key_t), s));
  DT_HIP(hipMemsetAsync(L.range + 1, 0, sizeof(hm_key_t), s));
  DT_HIP(hipMemsetAsync(L.visits, 0, sizeof(uint32_t) * L.tiles_all, s));
  hipLaunchKernelGGL(k_hm_init, dim3(hm_blocks((size_t)(H * W))), b, 0, s, values, fixed, domain, (long long)(H * W),
                     L.lv[0].u, L.lv[0].m, L.range);
  for (int l = 1; l < L.levels; l++) {
    const HmLevel &f = L.lv[l - 1], &c = L.lv[l];
    hipLaunchKernelGGL(k_hm_restrict, dim3(hm_blocks((size_t)c.H * (size_t)c.W)), b, 0, s, (const double *)f.u,
                       (const uint8_t *)f.m, f.H, f.W, c.u, c.m, c.H, c.W);
  }
  const HmLevel &c = L.lv[L.levels - 1];
  if (c.H <= HM_T && c.W <= HM_T) {
    hipLaunchKernelGGL(k_hm_flood, dim3(1), b, 0, s, c.u, (const uint8_t *)c.m, c.H, c.W);
  } else {  // (level_cap cut the pyramid short)
    const long long n = (long long)c.H * c.W;
    hipLaunchKernelGGL(k_hm_start, dim3(hm_blocks((size_t)n)), b, 0, s, c.u, (const uint8_t *)c.m, n,
                       (const hm_key_t *)L.range);
  }
  return DT_OK;
}

int dt_launch_harmonic_rounds(hipStream_t s, int64_t H, int64_t W, int max_rounds, int level_cap, int level,
                              int first_round, int rounds, double tol, void *scratch, size_t scratch_bytes,
                              double *out) {
  DT_TRY(hm_check(H, W, max_rounds, level_cap));
  DT_REQUIRE(tol > 0.0 && tol < (double)INFINITY, "tol must be finite and > 0");
  const HmLayout L = hm_layout(H, W, max_rounds, level_cap, scratch, out);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  DT_REQUIRE(level >= 0 && level < L.levels, "no such level");
  DT_REQUIRE(first_round >= 0 && rounds >= 0 && first_round + rounds <= max_rounds, "rounds beyond the budget");
  const HmLevel &v = L.lv[level];
  const hm_key_t tol_key = hm_host_key(tol);
  const dim3 b(256);
  // (a level of one tile has no halo that could change under a visit: longer visits, fewer rounds)
  const int sweeps = v.tiles_x * v.tiles_y == 1 ? HM_SWEEPS_ONE : HM_SWEEPS;
  for (int r = first_round; r < first_round + rounds; r++) {
    const hm_key_t *prev = r ? v.keys + r - 1 : nullptr;
    // (the level's first round visits every tile)
    hy_launch_colours(HyRound{nullptr, nullptr, r ? v.act : nullptr, v.act, v.visits, v.tiles_x, v.tiles_y, 0},
                      [&](dim3 blocks, const HyRound &rnd) {
                        hipLaunchKernelGGL(k_hm_round, blocks, b, 0, s, v.u, (const uint8_t *)v.m, v.H, v.W, prev,
                                           tol_key, (const hm_key_t *)L.range, sweeps, rnd);
                      });
    hipLaunchKernelGGL(k_hm_residual, dim3((unsigned)(v.tiles_x * v.tiles_y)), b, 0, s, (const double *)v.u,
                       (const uint8_t *)v.m, v.H, v.W, v.tiles_x, v.tiles_y, (const uint8_t *)v.act, r == 0 ? 1 : 0,
                       v.tile_key, prev, tol_key, v.keys + r);
  }
  return DT_OK;
}

int dt_launch_harmonic_prolong(hipStream_t s, int64_t H, int64_t W, int max_rounds, int level_cap, int level,
                               void *scratch, size_t scratch_bytes, double *out) {
  DT_TRY(hm_check(H, W, max_rounds, level_cap));
  const HmLayout L = hm_layout(H, W, max_rounds, level_cap, scratch, out);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  DT_REQUIRE(level >= 1 && level < L.levels, "no such level");
  const HmLevel &c = L.lv[level], &f = L.lv[level - 1];
  hipLaunchKernelGGL(k_hm_prolong, dim3(hm_blocks((size_t)f.H * (size_t)f.W)), dim3(256), 0, s, (const double *)c.u,
                     c.W, f.u, (const uint8_t *)f.m, f.H, f.W);
  return DT_OK;
}

int dt_launch_harmonic_finish(hipStream_t s, int64_t H, int64_t W, int max_rounds, int level_cap, double tol,
                              void *scratch, size_t scratch_bytes, int64_t *info, int *status) {
  DT_TRY(hm_check(H, W, max_rounds, level_cap));
  const HmLayout L = hm_layout(H, W, max_rounds, level_cap, scratch, nullptr);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  hipLaunchKernelGGL(k_hm_finish, dim3(1), dim3(256), 0, s, (const hm_key_t *)L.keys, L.levels, max_rounds,
                     hm_host_key(tol), (const uint32_t *)L.visits, (long long)L.tiles_all, info ? info : L.info, status);
  return DT_OK;
}
