// dt_watershed.hip -- drainage targets / flow lengths, pour-point watersheds and upslope (longest) flow length
// (net-new; descriptools_amd/watershed.py holds the definition).
//
// dt_path_tiles.h holds the drainage graph, the tiles, the perimeter nodes, the node rounds and the host sequence.
// Every length is a pair of exact move counts (n_card, n_diag), turned into float64 once, as n_card * px + n_diag *
// (px * sqrt(2)).  A tile is resolved in LDS by pointer doubling on one 64-bit word per cell (ws_resolve):
//   bits 0-11 local pointer | 16-31 n_card | 32-47 n_diag | 48-50 kind
// A jump is one addition (target word + my counts: counts stay <= 4096 per field, no carry); the pointer of a cell
// still PTR after 12 rounds is its 4096th successor, a cell of an in-tile cycle.
//
// Drainage (k_dr_tile1, k_dr_node x R, k_dr_tile3): record rounds on {p, tag, n_card, n_diag}.  p < 2^31: another
// node further down the path; p = 2^31 | flat index: resolved to that stop cell; p = PT_FAILP: resolved to no target
// (n_diag 0: nodata or a cycle; 1: a terminal that is no pour point).  An open record spans >= 2^(r+1) moves after
// round r; at >= N moves its path has repeated a cell, so it is resolved as a cycle.  k_dr_tile3 resolves the tile
// again, stages its perimeter records (and their pour labels) in LDS and writes target / length / label.
//
// Upslope length (k_ul_tile1, k_ul_node x R, k_ul_tile3): U(c) = the longest path that ends at c, a max-fold up
// the tree on the exact order of n_card + n_diag * sqrt(2).  Values are pairs (n_card | n_diag << 32); WS_CYC (all
// ones) is a walk of >= N moves, which only a cycle cell can end.  In a tile, every round of the doubling also sends
// value(c) + counts(c -> ptr) to ptr with a compare-and-swap max (pointer doubling with scatter: a max is
// idempotent and monotone, so the values are updated in place); a final send delivers every resolved cell to its end.
// The node rounds are scatter rounds with a weight: S(n) + w(n) goes to ptr(n) by CAS max and (ptr, w) doubles.
// k_ul_tile3 gathers each entry's inflow S(f) + 1 move from its feeders f in other tiles, folds the tile once more
// from those values and writes U; cells on an in-tile cycle (the images of the 4096th-successor pointers) or holding
// WS_CYC get -100.
#include "dt_path_tiles.h"

#define WS_KIND_SH 48
#define WS_CNT_MASK 0x0000FFFFFFFF0000ull
#define WS_CYC 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ uint32_t ws_ptr(uint64_t w) { return (uint32_t)w & 0xFFFu; }
__device__ __forceinline__ uint64_t ws_kind(uint64_t w) { return w >> WS_KIND_SH; }
__device__ __forceinline__ uint64_t ws_word(uint32_t ptr, uint32_t card, uint32_t diag, uint64_t kind) {
  return (uint64_t)ptr | ((uint64_t)card << 16) | ((uint64_t)diag << 32) | (kind << WS_KIND_SH);
}
// the counts of a word as a value pair
__device__ __forceinline__ uint64_t ws_cnt_pair(uint64_t w) {
  return ((w >> 16) & 0xFFFFull) | (((w >> 32) & 0xFFFFull) << 32);
}

// pair arithmetic: a + b, WS_CYC once the walk reaches N moves (inputs below N moves each: no overflow)
__device__ __forceinline__ uint64_t ws_add(uint64_t a, uint64_t b, int64_t N) {
  if (a == WS_CYC || b == WS_CYC) return WS_CYC;
  const uint64_t c = (a & 0xFFFFFFFFull) + (b & 0xFFFFFFFFull), d = (a >> 32) + (b >> 32);
  return c + d >= (uint64_t)N ? WS_CYC : (c | (d << 32));
}
// exact order of n_card + n_diag * sqrt(2): the sign of da + db * sqrt(2) from da^2 against 2 db^2 (|d| < 2^31)
__device__ __forceinline__ bool ws_greater(uint64_t a, uint64_t b) {
  if (a == b) return false;
  if (a == WS_CYC) return true;
  if (b == WS_CYC) return false;
  const int64_t da = (int64_t)(a & 0xFFFFFFFFull) - (int64_t)(b & 0xFFFFFFFFull);
  const int64_t db = (int64_t)(a >> 32) - (int64_t)(b >> 32);
  if (da >= 0 && db >= 0) return true;  // not both 0: a != b
  if (da <= 0 && db <= 0) return false;
  const uint64_t a2 = (uint64_t)(da < 0 ? -da : da) * (uint64_t)(da < 0 ? -da : da);
  const uint64_t b2 = 2ull * (uint64_t)(db < 0 ? -db : db) * (uint64_t)(db < 0 ? -db : db);
  return da > 0 ? a2 > b2 : b2 > a2;
}
// max-fold v into *p on the exact order (the first guess is a relaxed load; every failed CAS returns the word there)
template <int SCOPE>
__device__ __forceinline__ void ws_casmax(unsigned long long *p, uint64_t v) {
  unsigned long long cur = __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
  while (ws_greater(v, cur)) {
    const unsigned long long seen = atomicCAS(p, cur, (unsigned long long)v);
    if (seen == cur) return;
    cur = seen;
  }
}

__device__ __forceinline__ double ws_length(uint64_t card, uint64_t diag, double px, double pxd) {
  return (double)card * px + (double)diag * pxd;
}

// the starting word of local cell l of the tile at (y0, x0): pt_classify's result packed with the counts of its move
__device__ __forceinline__ uint64_t ws_init(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                            const int64_t *__restrict__ pour, int64_t H, int64_t W, int64_t y0,
                                            int64_t x0, int l) {
  return pt_classify(fdr, dem, pour, H, W, y0, x0, l, [](uint32_t kind, uint32_t ptr, bool diag) {
    if (kind != PT_K_PTR) return ws_word(ptr, 0u, 0u, kind);
    return ws_word(ptr, diag ? 0u : 1u, diag ? 1u : 0u, kind);
  });
}

// Pointer doubling of the tile's words (s_w holds w[] on entry, after a barrier).  SEND: pointer doubling with
// scatter of the value pairs s_v (initialised, after a barrier), with a final send from every resolved cell to its
// end.  On return (after a barrier) w[] / s_w hold the resolved words; a word still PTR is on or drains into an
// in-tile cycle.
template <bool SEND>
__device__ __forceinline__ void ws_resolve(uint64_t *s_w, unsigned long long *s_v, uint64_t (&w)[PT_CPT], int64_t N) {
  const int t = (int)threadIdx.x;
  for (int r = 0; r < PT_ROUNDS; r++) {
    if (SEND) {
#pragma unroll
      for (int k = 0; k < PT_CPT; k++) {
        const int l = k * 256 + t;
        const uint64_t kd = ws_kind(w[k]);
        if (kd != PT_K_FAIL && ws_ptr(w[k]) != (uint32_t)l) {
          const uint64_t v = __hip_atomic_load(&s_v[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          ws_casmax<__HIP_MEMORY_SCOPE_WORKGROUP>(&s_v[ws_ptr(w[k])], ws_add(v, ws_cnt_pair(w[k]), N));
        }
      }
    }
    uint64_t tg[PT_CPT];
#pragma unroll
    for (int k = 0; k < PT_CPT; k++) tg[k] = ws_kind(w[k]) == PT_K_PTR ? s_w[ws_ptr(w[k])] : 0ull;
    __syncthreads();
    int pend = 0;
#pragma unroll
    for (int k = 0; k < PT_CPT; k++) {
      if (ws_kind(w[k]) == PT_K_PTR) {
        w[k] = tg[k] + (w[k] & WS_CNT_MASK);
        s_w[k * 256 + t] = w[k];
        pend |= ws_kind(w[k]) == PT_K_PTR;
      }
    }
    if (!__syncthreads_or(pend)) break;
  }
  if (SEND) {
#pragma unroll
    for (int k = 0; k < PT_CPT; k++) {
      const int l = k * 256 + t;
      const uint64_t kd = ws_kind(w[k]);
      if (kd != PT_K_FAIL && kd != PT_K_PTR && ws_ptr(w[k]) != (uint32_t)l) {
        const uint64_t v = __hip_atomic_load(&s_v[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ws_casmax<__HIP_MEMORY_SCOPE_WORKGROUP>(&s_v[ws_ptr(w[k])], ws_add(v, ws_cnt_pair(w[k]), N));
      }
    }
    __syncthreads();
  }
}

// ---- drainage ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dr_tile1(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                  const int64_t *__restrict__ pour, int64_t H, int64_t W, int64_t TX,
                                                  uint4 *__restrict__ rec) {
  __shared__ uint64_t s_w[PT_T * PT_T];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint64_t w[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    w[k] = ws_init(fdr, dem, pour, H, W, T.y0, T.x0, k * 256 + t);
    s_w[k * 256 + t] = w[k];
  }
  __syncthreads();
  ws_resolve<false>(s_w, nullptr, w, H * W);
  uint4 o = make_uint4(PT_FAILP, 0xFFFFFFFFu, 0u, 0u);
  int l;
  int64_t y, x;
  if (pt_lane_cell(T, H, W, l, y, x)) {
    const uint64_t v = s_w[l];
    const uint64_t kd = ws_kind(v);
    const uint32_t p = ws_ptr(v);
    if (kd == PT_K_EXIT && p == (uint32_t)l) {
      bool dg;
      const uint32_t node = pt_exit_successor(fdr[y * W + x], TX, y, x, dg);
      o = make_uint4(node, 0u, dg ? 0u : 1u, dg ? 1u : 0u);
    } else if (kd == PT_K_EXIT) {
      o = make_uint4(pt_exit_own(p), 0u, (uint32_t)((v >> 16) & 0xFFFFu), (uint32_t)((v >> 32) & 0xFFFFu));
    } else if (kd == PT_K_STOP) {
      o = make_uint4(PT_RES | (uint32_t)((T.y0 + (p >> 6)) * W + T.x0 + (p & 63)), 0xFFFFFFFFu,
                     (uint32_t)((v >> 16) & 0xFFFFu), (uint32_t)((v >> 32) & 0xFFFFu));
    } else if (kd == PT_K_NOEND) {
      o = make_uint4(PT_FAILP, 0xFFFFFFFFu, 0u, 1u);
    }
  }
  rec[(int64_t)blockIdx.x * PT_SLOTS + t] = o;
}

// One record round src -> dst (dt_path_tiles.h; dt_flowpath.hip's fp_dn_round is its other form): the move counts add,
// and a record closes on a target, on no target, or -- at N moves -- as a cycle.
__global__ __launch_bounds__(256) void k_dr_node(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t NN,
                                                 int64_t N, uint32_t *flags, int r) {
  if (r >= 2 && flags[r - 1] == 0u) return;
  bool pend = false;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < NN; n += (int64_t)gridDim.x * 256) {
    const uint4 s = src[n];
    if (s.x & PT_RES) {
      if ((int32_t)s.y > r - 2) dst[n] = s;
      continue;
    }
    const uint4 q = src[s.x];
    uint4 o;
    if (q.x == PT_FAILP) {
      o = make_uint4(PT_FAILP, (uint32_t)r, 0u, q.w);
    } else {
      const uint64_t c = (uint64_t)s.z + q.z, d = (uint64_t)s.w + q.w;
      if (q.x & PT_RES) {
        o = make_uint4(q.x, (uint32_t)r, (uint32_t)c, (uint32_t)d);
      } else if (c + d >= (uint64_t)N) {
        o = make_uint4(PT_FAILP, (uint32_t)r, 0u, 0u);  // the path repeated a cell: a cycle
      } else {
        o = make_uint4(q.x, 0xFFFFFFFFu, (uint32_t)c, (uint32_t)d);
        pend = true;
      }
    }
    dst[n] = o;
  }
  if (__ballot(pend) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(&flags[r + 1], 1u);
}

__global__ __launch_bounds__(256) void k_dr_tile3(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                  const int64_t *__restrict__ pour, int64_t H, int64_t W, int64_t TX,
                                                  double px, double pxd, const uint4 *__restrict__ rec,
                                                  int64_t *__restrict__ target, double *__restrict__ length,
                                                  int64_t *__restrict__ label) {
  __shared__ uint64_t s_w[PT_T * PT_T];
  __shared__ uint4 s_x[PT_SLOTS];
  __shared__ int64_t s_lab[PT_SLOTS];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint64_t w[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    w[k] = ws_init(fdr, dem, pour, H, W, T.y0, T.x0, k * 256 + t);
    s_w[k * 256 + t] = w[k];
  }
  {
    const uint4 q = rec[(int64_t)blockIdx.x * PT_SLOTS + t];
    s_x[t] = q;
    if (label) s_lab[t] = (q.x & PT_RES) && q.x != PT_FAILP ? pour[q.x & ~PT_RES] : (q.x == PT_FAILP && q.w == 1u ? 0 : -100);
  }
  __syncthreads();
  ws_resolve<false>(s_w, nullptr, w, H * W);
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    const int64_t y = T.y0 + (l >> 6), x = T.x0 + (l & 63);
    if (y >= H || x >= W) continue;
    const uint64_t v = w[k];
    const uint64_t kd = ws_kind(v);
    const uint32_t p = ws_ptr(v);
    int64_t tg = -100, lb = -100;
    double ln = -100.0;
    uint64_t card = (v >> 16) & 0xFFFFull, diag = (v >> 32) & 0xFFFFull;
    if (kd == PT_K_STOP) {
      tg = (T.y0 + (p >> 6)) * W + T.x0 + (p & 63);
      ln = ws_length(card, diag, px, pxd);
      if (label) lb = pour[tg];
    } else if (kd == PT_K_EXIT) {
      const int j = pt_slot((int)(p >> 6), (int)(p & 63));
      const uint4 q = s_x[j];
      if ((q.x & PT_RES) && q.x != PT_FAILP) {
        tg = q.x & ~PT_RES;
        ln = ws_length(card + q.z, diag + q.w, px, pxd);
      }
      if (label) lb = s_lab[j];
    } else if (kd == PT_K_NOEND) {
      lb = 0;
    }
    const int64_t c = y * W + x;
    if (target) target[c] = tg;
    if (length) length[c] = ln;
    if (label) label[c] = lb;
  }
}

// ---- upslope length ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ul_tile1(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                  int64_t H, int64_t W, int64_t TX, uint32_t *__restrict__ uptr,
                                                  unsigned long long *__restrict__ uw,
                                                  unsigned long long *__restrict__ S) {
  __shared__ uint64_t s_w[PT_T * PT_T];
  __shared__ unsigned long long s_v[PT_T * PT_T];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  const int64_t N = H * W;
  uint64_t w[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    w[k] = ws_init(fdr, dem, nullptr, H, W, T.y0, T.x0, k * 256 + t);
    s_w[k * 256 + t] = w[k];
    s_v[k * 256 + t] = 0ull;
  }
  __syncthreads();
  ws_resolve<true>(s_w, s_v, w, N);
  uint32_t p_out = PT_NONE;
  unsigned long long w_out = 0ull, s_out = 0ull;
  int l;
  int64_t y, x;
  if (pt_lane_cell(T, H, W, l, y, x)) {
    const uint64_t v = s_w[l];
    s_out = s_v[l];
    const uint32_t p = ws_ptr(v);
    if (ws_kind(v) == PT_K_EXIT && p == (uint32_t)l) {
      bool dg;
      p_out = pt_exit_successor(fdr[y * W + x], TX, y, x, dg);
      w_out = dg ? (1ull << 32) : 1ull;
    } else if (ws_kind(v) == PT_K_EXIT) {
      p_out = pt_exit_own(p);
      w_out = ws_cnt_pair(v);
    }
  }
  const int64_t n = (int64_t)blockIdx.x * PT_SLOTS + t;
  uptr[n] = p_out;
  uw[n] = w_out;
  S[n] = s_out;
}

// the scatter round of upslope length: S(n) + w goes up by CAS max on the exact order, and the weights add
struct UlFold {
  int64_t N;
  __device__ __forceinline__ void send(unsigned long long *to, unsigned long long sv, unsigned long long w) const {
    ws_casmax<__HIP_MEMORY_SCOPE_AGENT>(to, ws_add(sv, w, N));
  }
  __device__ __forceinline__ unsigned long long join(unsigned long long a, unsigned long long b) const {
    return ws_add(a, b, N);
  }
};
__global__ __launch_bounds__(256) void k_ul_node(const uint32_t *__restrict__ psrc, uint32_t *__restrict__ pdst,
                                                 const unsigned long long *__restrict__ wsrc,
                                                 unsigned long long *__restrict__ wdst, unsigned long long *S,
                                                 int64_t NN, int64_t N, uint32_t *flags, int r) {
  pt_scatter_round<true>(psrc, pdst, wsrc, wdst, S, NN, flags, r, UlFold{N});
}

__global__ __launch_bounds__(256) void k_ul_tile3(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                  int64_t H, int64_t W, int64_t TX, double px, double pxd,
                                                  const unsigned long long *__restrict__ S,
                                                  double *__restrict__ length) {
  __shared__ uint64_t s_w[PT_T * PT_T];
  __shared__ unsigned long long s_v[PT_T * PT_T];
  __shared__ uint8_t s_onc[PT_T * PT_T];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  const int64_t N = H * W;
  uint64_t w[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    w[k] = ws_init(fdr, dem, nullptr, H, W, T.y0, T.x0, k * 256 + t);
    s_w[k * 256 + t] = w[k];
    s_v[k * 256 + t] = 0ull;
    s_onc[k * 256 + t] = 0;
  }
  __syncthreads();
  // entry inflow: S(f) + one move from each feeder f in another tile (an exit of its tile, so a perimeter node)
  if (t < 252) {
    const int l = pt_slot_cell(t);
    const int64_t y = T.y0 + (l >> 6), x = T.x0 + (l & 63);
    if (y < H && x < W && !(dem && dem[y * W + x] <= -100.0f)) {
      unsigned long long ext = 0ull;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        int dy, dx;
        dt_nb_delta(i, dy, dx);
        const int64_t fy = y + dy, fx = x + dx;
        if (fy < 0 || fy >= H || fx < 0 || fx >= W) continue;
        if ((fy >> 6) == T.ty && (fx >> 6) == T.tx) continue;
        const int64_t f = fy * W + fx;
        if (fdr[f] != (uint8_t)dt_nb_back_code(i)) continue;  // f's code points back at this cell
        if (dem && dem[f] <= -100.0f) continue;
        const uint64_t v = ws_add(S[pt_node(fy, fx, TX)], (dy != 0 && dx != 0) ? (1ull << 32) : 1ull, N);
        if (ws_greater(v, ext)) ext = v;
      }
      s_v[l] = ext;
    }
  }
  __syncthreads();
  ws_resolve<true>(s_w, s_v, w, N);
#pragma unroll
  for (int k = 0; k < PT_CPT; k++)
    if (ws_kind(w[k]) == PT_K_PTR) s_onc[ws_ptr(w[k])] = 1;
  __syncthreads();
  double out[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    const uint64_t v = s_v[l];
    out[k] = (ws_kind(w[k]) == PT_K_FAIL || s_onc[l] || v == WS_CYC)
                 ? -100.0
                 : ws_length(v & 0xFFFFFFFFull, v >> 32, px, pxd);
  }
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    const int64_t y = T.y0 + (l >> 6), x = T.x0 + (l & 63);
    if (y < H && x < W) length[y * W + x] = out[k];
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------
static PtLayout ws_layout(int64_t H, int64_t W, bool upslope, void *scratch) {
  DtCarver c(scratch);
  return pt_layout(c, H, W, upslope ? PT_BUF_PTR_WEIGHT : PT_BUF_REC);
}

size_t dt_drainage_scratch(int64_t H, int64_t W) { return ws_layout(H, W, false, nullptr).bytes; }
size_t dt_upslope_length_scratch(int64_t H, int64_t W) { return ws_layout(H, W, true, nullptr).bytes; }

int dt_launch_drainage(hipStream_t s, const uint8_t *fdr, const float *dem, const int64_t *pour, int64_t H, int64_t W,
                       double px, void *scratch, size_t scratch_bytes, int64_t *target, double *length,
                       int64_t *label) {
  const PtLayout L = ws_layout(H, W, false, scratch);
  int R;
  DT_TRY(pt_begin(s, L, H, W, scratch_bytes, R));
  if (!R) return DT_OK;
  const int64_t N = H * W;
  const double pxd = px * std::sqrt(2.0);
  pt_launch_passes(
      L, R, [&](dim3 g, dim3 b) { hipLaunchKernelGGL(k_dr_tile1, g, b, 0, s, fdr, dem, pour, H, W, L.TX, L.rec[0]); },
      [&](dim3 g, dim3 b, int r, int src, int dst) {
        hipLaunchKernelGGL(k_dr_node, g, b, 0, s, L.rec[src], L.rec[dst], L.NN, N, L.flags, r);
      },
      [&](dim3 g, dim3 b, int last) {
        hipLaunchKernelGGL(k_dr_tile3, g, b, 0, s, fdr, dem, pour, H, W, L.TX, px, pxd, L.rec[last], target, length,
                           label);
      });
  return DT_OK;
}

int dt_launch_upslope_length(hipStream_t s, const uint8_t *fdr, const float *dem, int64_t H, int64_t W, double px,
                             void *scratch, size_t scratch_bytes, double *length) {
  const PtLayout L = ws_layout(H, W, true, scratch);
  int R;
  DT_TRY(pt_begin(s, L, H, W, scratch_bytes, R));
  if (!R) return DT_OK;
  const int64_t N = H * W;
  const double pxd = px * std::sqrt(2.0);
  pt_launch_passes(
      L, R,
      [&](dim3 g, dim3 b) {
        hipLaunchKernelGGL(k_ul_tile1, g, b, 0, s, fdr, dem, H, W, L.TX, L.uptr[0], L.uw[0], L.S);
      },
      [&](dim3 g, dim3 b, int r, int src, int dst) {
        hipLaunchKernelGGL(k_ul_node, g, b, 0, s, L.uptr[src], L.uptr[dst], L.uw[src], L.uw[dst], L.S, L.NN, N, L.flags,
                           r);
      },
      [&](dim3 g, dim3 b, int) {
        hipLaunchKernelGGL(k_ul_tile3, g, b, 0, s, fdr, dem, H, W, L.TX, px, pxd, L.S, length);
      });
  return DT_OK;
}
