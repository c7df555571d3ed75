// dt_regions.hip -- connected regions of a mask: labels, sizes, seeded / sieved selection, and HAND inundation kept to
// the wet regions that hold a river cell (net-new; descriptools_amd/regions.py holds the definition).
//
// Foreground = mask != 0.  Two foreground cells are in one region when a chain of adjacent foreground cells joins them
// (connectivity 4: N, S, E, W; 8: the diagonals too).  label = the smallest flat index of the cell's region, size = the
// number of its cells; both are functions of the mask alone.
//
// Union-find on one int32 plane P.  On foreground P[x] <= x always, and a root has P[r] == r: every find walks strictly
// downward and ends, and the root of a finished set is its smallest member -- which IS the label, so no tie rule
// exists.  Background holds RG_BG and is never walked.  uniting(a, b): find both roots, hang the larger under the
// smaller with one atomicMin, go on from the value it returns when another thread got there first (each retry starts
// lower, so it ends).
//
// Which pairs are united.  Every pair of orthogonally adjacent foreground cells ends up in one set: (c, W) always; (c, N)
// directly unless W and NW are foreground too (then W ~ NW by the same rule one cell to the left, c ~ W and NW ~ N).
// Under 8-connectivity a diagonal pair is united directly only when the two cells that touch both are background
// (otherwise it follows from the orthogonal pairs).
//
//   k_rg_local   one workgroup per 64 x 64 tile, a wave per row (one ballot = the row's mask): the tile's own regions
//                in LDS -- a cell starts under the first cell of its row run, the rules above unite the runs across
//                rows with LDS atomics, outside the tile counts as background.  P = the flat index of the smallest cell
//                of the cell's tile-local region.  With `aux` it also writes the plane A: on the smallest cell of a
//                tile-local region its cell count (31 bits) and, in bit 31, whether it holds a seed; 0 elsewhere.
//   k_rg_seam    one thread per cell of every tile's first row (pairs N, NW, NE) and first column (pairs W, NW, SW):
//                the same rules across the seams, on P in global memory.  What other workgroups write is read with
//                relaxed agent-scope atomic loads.  No thread waits for another.
//   k_rg_flat    root = find(P, c) (P is final: plain loads), written as the int64 label and / or as an int32 root
//                plane; with `aux` the smallest cell of every tile-local region adds its count and its seed bit to A at
//                the root -- one atomic per tile-local region, not per cell.
//   k_rg_out     size / keep gathered from A at the root.
// Connected inundation: k_rg_wet in front (the wet mask by dt_reach_wet.h's predicate, seeds = wet and river == 1),
// k_rg_depth behind (dt_inundate's value, 0 on a wet cell whose region holds no seed).
// 3 or 4 launches (5 for the inundation) whatever the mask holds; the launcher never synchronises.
#include "dt_kernels.h"
#include "dt_reach_wet.h"

#define RG_T DT_REGIONS_TILE  // 64: a row of a tile is one wave
#define RG_BG (-1)
#define RG_SEEDED 0x80000000u

struct RgLayout {
  int32_t *P;     // per cell: the parent (a flat index <= the cell's own), RG_BG on background
  uint32_t *A;    // per cell: count | seeded << 31 of the (tile-local, then whole) region whose smallest cell this is
  int32_t *root;  // per cell: the root, where no int64 label is written
  uint8_t *wet, *seed;  // connected inundation only
  size_t bytes;
};
static RgLayout rg_layout(int64_t H, int64_t W, void *scratch, bool masks) {
  RgLayout L = {};
  DtCarver c(scratch);
  const size_t n = (size_t)(H * W);
  L.P = c.take<int32_t>(n);
  L.A = c.take<uint32_t>(n);
  L.root = c.take<int32_t>(n);
  if (masks) {
    L.wet = c.take<uint8_t>(n);
    L.seed = c.take<uint8_t>(n);
  }
  L.bytes = c.bytes();
  return L;
}
size_t dt_regions_scratch(int64_t H, int64_t W) { return rg_layout(H, W, nullptr, false).bytes; }
size_t dt_inundate_connected_scratch(int64_t H, int64_t W) { return rg_layout(H, W, nullptr, true).bytes; }

// ---- union-find in LDS (local ids ly * 64 + lx) ------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rg_lfind(uint32_t *par, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void rg_lunite(uint32_t *par, uint32_t a, uint32_t b) {
  for (;;) {
    a = rg_lfind(par, a);
    b = rg_lfind(par, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(&par[a], b);  // a > b
    if (old == a) return;                        // a was still a root
    a = old;                                     // it had been hung under old < a meanwhile: unite that with b
  }
}
// ---- union-find on P ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t rg_find(int32_t *P, int32_t x) {
  for (;;) {
    const int32_t p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void rg_unite(int32_t *P, int32_t a, int32_t b) {
  for (;;) {
    a = rg_find(P, a);
    b = rg_find(P, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicMin(&P[a], b);
    if (old == a) return;
    a = old;
  }
}

// bit l of a row mask, false outside 0..63
__device__ __forceinline__ bool rg_bit(unsigned long long m, int l) { return l >= 0 && l < 64 && ((m >> l) & 1ull); }

template <bool CONN8>
__global__ __launch_bounds__(256) void k_rg_local(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ seeds,
                                                  int H, int W, int xtiles, int aux, int32_t *__restrict__ P,
                                                  uint32_t *__restrict__ A) {
  __shared__ uint32_t s_par[RG_T * RG_T], s_cnt[RG_T * RG_T];
  __shared__ unsigned long long s_fg[RG_T], s_sd[RG_T];
  const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
  const int ty = (int)(blockIdx.x / (unsigned)xtiles), tx = (int)(blockIdx.x - (unsigned)ty * xtiles);
  const int y0 = ty * RG_T, x0 = tx * RG_T, x = x0 + lane;
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes left of this one
  // the rows' masks; every cell under the first cell of its run
#pragma unroll 4
  for (int k = 0; k < 16; k++) {
    const int ly = wv * 16 + k, y = y0 + ly;
    const bool in = y < H && x < W;
    const int64_t i = (int64_t)y * W + x;
    const bool fg = in && mask[i] != 0;
    const unsigned long long m = __ballot(fg);
    const unsigned long long sd = __ballot(fg && seeds && seeds[i] != 0);
    const unsigned long long gap = ~m & below;  // background left of the lane
    const int start = gap ? 64 - (int)__builtin_clzll(gap) : 0;
    s_par[ly * RG_T + lane] = (uint32_t)(ly * RG_T + start);
    s_cnt[ly * RG_T + lane] = 0u;
    if (lane == 0) {
      s_fg[ly] = m;
      s_sd[ly] = sd;
    }
  }
  __syncthreads();
  // the runs united across rows
  for (int k = 0; k < 16; k++) {
    const int ly = wv * 16 + k;
    if (ly == 0) continue;  // wave-uniform
    const unsigned long long m = s_fg[ly], up = s_fg[ly - 1];
    if (!rg_bit(m, lane)) continue;
    const bool w = rg_bit(m, lane - 1), e = rg_bit(m, lane + 1);
    const bool n = rg_bit(up, lane), nw = rg_bit(up, lane - 1), ne = rg_bit(up, lane + 1);
    const uint32_t c = (uint32_t)(ly * RG_T + lane);
    if (n && !(w && nw)) rg_lunite(s_par, c, c - RG_T);
    if (CONN8) {
      if (nw && !n && !w) rg_lunite(s_par, c, c - RG_T - 1);
      if (ne && !n && !e) rg_lunite(s_par, c, c - RG_T + 1);
    }
  }
  __syncthreads();
  // the roots (one find per run, by its first lane), the counts and seed bits on them
  uint32_t root[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int ly = wv * 16 + k;
    const unsigned long long m = s_fg[ly];
    const bool fg = rg_bit(m, lane);
    const unsigned long long gap = ~m & below;
    const int start = gap ? 64 - (int)__builtin_clzll(gap) : 0;
    uint32_t r = 0;
    if (fg && start == lane) {
      r = rg_lfind(s_par, (uint32_t)(ly * RG_T + lane));
      if (aux) {
        const unsigned long long rest = ~(m >> lane);  // bit j: lane + j is background (or past the row)
        const int len = rest ? (int)__builtin_ctzll(rest) : 64;
        const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
        atomicAdd(&s_cnt[r], (uint32_t)len);
        if (s_sd[ly] & run) atomicOr(&s_cnt[r], RG_SEEDED);
      }
    }
    root[k] = (uint32_t)__shfl((int)r, start);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int ly = wv * 16 + k, y = y0 + ly;
    if (y >= H || x >= W) continue;
    const int64_t i = (int64_t)y * W + x;
    const bool fg = rg_bit(s_fg[ly], lane);
    const uint32_t r = root[k];
    P[i] = fg ? (int32_t)((int64_t)(y0 + (int)(r >> 6)) * W + x0 + (int)(r & 63u)) : RG_BG;
    if (aux) A[i] = (fg && r == (uint32_t)(ly * RG_T + lane)) ? s_cnt[r] : 0u;
  }
}

// items: first the cells of the rows y = 64 k (k >= 1), then those of the columns x = 64 j (j >= 1)
template <bool CONN8>
__global__ __launch_bounds__(256) void k_rg_seam(int H, int W, int64_t row_items, int64_t items, int32_t *P) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= items) return;
  // foreground-ness never changes, so a plain load tells it
  if (t < row_items) {
    const int y = (int)(t / W + 1) * RG_T, x = (int)(t % W);
    const int64_t i = (int64_t)y * W + x;
    if (P[i] < 0) return;
    const int32_t *up = P + i - W;
    const bool hw = x > 0, he = x + 1 < W;
    const bool n = up[0] >= 0, w = hw && P[i - 1] >= 0, nw = hw && up[-1] >= 0;
    if (n && !(w && nw)) rg_unite(P, (int32_t)i, (int32_t)(i - W));
    if (CONN8) {
      const bool e = he && P[i + 1] >= 0, ne = he && up[1] >= 0;
      if (nw && !n && !w) rg_unite(P, (int32_t)i, (int32_t)(i - W - 1));
      if (ne && !n && !e) rg_unite(P, (int32_t)i, (int32_t)(i - W + 1));
    }
  } else {
    const int64_t u = t - row_items;
    const int x = (int)(u / H + 1) * RG_T, y = (int)(u % H);
    const int64_t i = (int64_t)y * W + x;
    if (P[i] < 0) return;
    const bool w = P[i - 1] >= 0;
    if (w) rg_unite(P, (int32_t)i, (int32_t)(i - 1));
    if (CONN8 && !w) {
      const bool hn = y > 0, hs = y + 1 < H;
      if (hn && P[i - W - 1] >= 0 && !(P[i - W] >= 0)) rg_unite(P, (int32_t)i, (int32_t)(i - W - 1));
      if (hs && P[i + W - 1] >= 0 && !(P[i + W] >= 0)) rg_unite(P, (int32_t)i, (int32_t)(i + W - 1));
    }
  }
}

__global__ __launch_bounds__(256) void k_rg_flat(const int32_t *__restrict__ P, int64_t N, int aux,
                                                 uint32_t *A, int64_t *__restrict__ label,
                                                 int32_t *__restrict__ root) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int32_t r = P[i];
  if (r >= 0) {
    for (int32_t q = P[r]; q != r; q = P[r]) r = q;
    if (aux && r != (int32_t)i) {
      // a is non-zero on the smallest cell of a tile-local region only; nobody adds to such a cell unless it is a root,
      // which r != i excludes
      const uint32_t a = A[i];
      if (a & ~RG_SEEDED) atomicAdd(&A[r], a & ~RG_SEEDED);
      if (a & RG_SEEDED) atomicOr(&A[r], RG_SEEDED);
    }
  }
  if (label) label[i] = r >= 0 ? (int64_t)r : -100ll;
  if (root) root[i] = r;
}

// the root of cell i from the label (int64, -100 on background) or from the root plane
__device__ __forceinline__ int32_t rg_root_of(const int64_t *__restrict__ label, const int32_t *__restrict__ root,
                                              int64_t i) {
  if (label) {
    const int64_t l = label[i];
    return l < 0 ? RG_BG : (int32_t)l;
  }
  return root[i];
}

__global__ __launch_bounds__(256) void k_rg_out(const int64_t *__restrict__ label, const int32_t *__restrict__ root,
                                                const uint32_t *__restrict__ A, int64_t N, int seeded,
                                                int64_t min_cells, int64_t *__restrict__ size,
                                                uint8_t *__restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int32_t r = rg_root_of(label, root, i);
  const uint32_t a = r >= 0 ? A[r] : 0u;
  const int64_t n = (int64_t)(a & ~RG_SEEDED);
  if (size) size[i] = n;
  if (keep) keep[i] = (r >= 0 && (!seeded || (a & RG_SEEDED)) && n >= min_cells) ? 1 : 0;
}

template <typename HT>
__global__ __launch_bounds__(256) void k_rg_wet(const int32_t *__restrict__ catch_, const HT *__restrict__ hand,
                                                const double *__restrict__ stage, const int8_t *__restrict__ river,
                                                int64_t N, int64_t R, uint8_t *__restrict__ wet,
                                                uint8_t *__restrict__ seed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  bool w;
  (void)dt_rc_depth(catch_[i], hand[i], stage, R, w);
  wet[i] = w ? 1 : 0;
  seed[i] = (w && river[i] == 1) ? 1 : 0;
}

template <typename HT>
__global__ __launch_bounds__(256) void k_rg_depth(const int32_t *__restrict__ catch_, const HT *__restrict__ hand,
                                                  const double *__restrict__ stage, const int32_t *__restrict__ root,
                                                  const uint32_t *__restrict__ A, int64_t N, int64_t R,
                                                  float *__restrict__ depth) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  bool w;
  float d = dt_rc_depth(catch_[i], hand[i], stage, R, w);
  if (w && !(A[root[i]] & RG_SEEDED)) d = 0.f;  // a wet cell is foreground of k_rg_wet's mask: its root is a cell
  depth[i] = d;
}

// local, seam, flat on the workspace L: afterwards the roots are in `label` and / or L.root and, with aux, A is final
static void rg_solve(hipStream_t s, const RgLayout &L, const uint8_t *mask, const uint8_t *seeds, int64_t H, int64_t W,
                     int connectivity, int aux, int64_t *label, int32_t *root) {
  const int64_t N = H * W;
  const int xt = (int)((W + RG_T - 1) / RG_T), yt = (int)((H + RG_T - 1) / RG_T);
  const int64_t row_items = (int64_t)(yt - 1) * W, items = row_items + (int64_t)(xt - 1) * H;
  const dim3 gt((unsigned)(xt * yt)), gs((unsigned)((items + 255) / 256)), gn((unsigned)((N + 255) / 256)), b(256);
  if (connectivity == 8) {
    hipLaunchKernelGGL(k_rg_local<true>, gt, b, 0, s, mask, seeds, (int)H, (int)W, xt, aux, L.P, L.A);
    if (items) hipLaunchKernelGGL(k_rg_seam<true>, gs, b, 0, s, (int)H, (int)W, row_items, items, L.P);
  } else {
    hipLaunchKernelGGL(k_rg_local<false>, gt, b, 0, s, mask, seeds, (int)H, (int)W, xt, aux, L.P, L.A);
    if (items) hipLaunchKernelGGL(k_rg_seam<false>, gs, b, 0, s, (int)H, (int)W, row_items, items, L.P);
  }
  hipLaunchKernelGGL(k_rg_flat, gn, b, 0, s, L.P, N, aux, L.A, label, root);
}

int dt_launch_regions(hipStream_t s, const uint8_t *mask, const uint8_t *seeds, int64_t H, int64_t W, int connectivity,
                      int64_t min_cells, void *scratch, size_t scratch_bytes, int64_t *label, int64_t *size,
                      uint8_t *keep) {
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
  DT_REQUIRE(!keep || min_cells >= 1, "min_cells must be >= 1");
  if (H == 0 || W == 0) return DT_OK;
  const RgLayout L = rg_layout(H, W, scratch, false);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const int aux = size || keep;
  rg_solve(s, L, mask, keep ? seeds : nullptr, H, W, connectivity, aux, label, label ? nullptr : L.root);
  if (aux) {
    const int64_t N = H * W;
    hipLaunchKernelGGL(k_rg_out, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, label, L.root, L.A, N,
                       seeds != nullptr, min_cells, size, keep);
  }
  return DT_OK;
}

int dt_launch_inundate_connected(hipStream_t s, const int32_t *catch_, const void *hand, int hand_bytes,
                                 const double *stage, const int8_t *river, int64_t H, int64_t W, int64_t R,
                                 int connectivity, void *scratch, size_t scratch_bytes, float *depth) {
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
  if (H == 0 || W == 0) return DT_OK;
  const RgLayout L = rg_layout(H, W, scratch, true);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const int64_t N = H * W;
  const dim3 g((unsigned)((N + 255) / 256)), b(256);
  const float *h4 = (const float *)hand;
  const double *h8 = (const double *)hand;
  if (hand_bytes == 4) hipLaunchKernelGGL(k_rg_wet<float>, g, b, 0, s, catch_, h4, stage, river, N, R, L.wet, L.seed);
  else hipLaunchKernelGGL(k_rg_wet<double>, g, b, 0, s, catch_, h8, stage, river, N, R, L.wet, L.seed);
  rg_solve(s, L, L.wet, L.seed, H, W, connectivity, 1, nullptr, L.root);
  if (hand_bytes == 4) hipLaunchKernelGGL(k_rg_depth<float>, g, b, 0, s, catch_, h4, stage, L.root, L.A, N, R, depth);
  else hipLaunchKernelGGL(k_rg_depth<double>, g, b, 0, s, catch_, h8, stage, L.root, L.A, N, R, depth);
  return DT_OK;
}
