// dt_flowpath.hip -- flow-path extremes: the max / min of a value raster over everything upslope of a cell, or along
// its path downstream, the pointwise blend of depression carving, and the weighted sums along a path: travel time
// and time of concentration (net-new; descriptools_amd/flowpath.py and flowdir.d8_carved hold the definitions).
//
// dt_path_tiles.h holds the drainage graph, the tiles, the perimeter nodes, the node rounds and the host sequence.
//
// Key.  A cell's value travels as one 64-bit word: the order-preserving uint32 key of the float (dt_zonal.hip's,
// complemented for a minimum) in the high half, 0xFFFFFFFF - flat index in the low half.  The larger word is the
// better value and, between equal values, the smaller flat index, for both kinds; NaN has no word (0: "no value";
// a real word is never 0 because the flat index stays below 2^31).  -0.0 is keyed as +0.0.  Every fold is therefore
// an unsigned 64-bit max: one native LDS / global atomic per send upslope, a plain compare downstream.
//
// Words.  A tile's paths are resolved in LDS by pointer doubling on one 32-bit word per cell: bits 0-11 a local
// pointer, bits 12-14 the kind.
//
// Upslope fold (k_fp_up_tile1, k_fp_up_node x R, k_fp_up_tile3): U(c) = the max word over every cell whose path
// contains c.  Pointer doubling with scatter: in round r every PTR cell sends its word to its pointer with an atomic
// max, then doubles the pointer.  By induction the word of d holds, after round r, every cell at most 2^(r+1) - 1
// moves above d (the cell 2^r moves above d is PTR with pointer d, and held everything < 2^r moves above itself); a
// max is idempotent and monotone, so the words are updated in place and a word read early or late only carries more
// of what belongs there.  A resolved cell stops sending and delivers its word to its path's end once, after the
// rounds.  A cycle is no special case: its cells stay PTR and send in all 12 rounds, which cover the < 4096 moves
// between any two cells of one tile.  The node rounds are scatter rounds without a weight; on a cycle the pointers
// never run out, all R rounds run, and that is enough: a node path that repeats no node is shorter than N <= 2^(R-1).
// Entries and exits of a path are all on its node path, so S at an exit cell is complete; a perimeter cell that a path
// merely passes is not, which is why k_fp_up_tile3 takes each perimeter cell's inflow from its feeders in other tiles
// (exits of theirs), folds the tile once more and writes the decoded value and its cell.
//
// Downstream fold (k_fp_dn_tile1, k_fp_dn_node x R, k_fp_dn_tile3): D(c) = the max word over c's path up to where it
// stops.  A gather without atomics: v(c) = max(v(c), v(ptr(c))), ptr(c) = ptr(ptr(c)), both read before a barrier and
// written after it, so every round reads the state of the round before.  After round r, v(c) covers the 2^(r+1) cells
// from c on (or the path to its end, end included); a cell on or draining into an in-tile cycle has its whole tail and
// the cycle after 12 rounds.  The node rounds are record rounds on {pointer, tag, word}: PT_RES the path has stopped
// and the word is final, PT_FAILP it ended without a stop cell.  Without a stop raster a record still open after R
// rounds lies on or drains into a cycle and its word is complete (R rounds cover N node-moves); with one, such a path
// met no stop cell and gets no value.
//
// Path sums (k_ps_dn_tile1, k_ps_dn_node x R, k_ps_dn_tile3; the upslope kernels above with a raw key): T(c) = the sum
// of q = rint(w * 2^s) over the moves of c's path down to where it stops, and U(c) = the longest such sum that ends at
// c.  The downstream sum is the downstream fold with an unsigned 64-bit add in place of the max: v(c) += v(ptr(c)),
// where v(c) is the cost of the moves from c up to, not including, its pointer (an end carries 0, and an exit cell's
// own move travels in its perimeter record, so nothing is added twice).  A sum, unlike a max, is not idempotent: a
// path that never stops (a D8 cycle) doubles its sum every round, the wrap is that of unsigned arithmetic, and the
// value is discarded -- such a cell has no target and gets -100, as watershed.drainage gives it, with or without a
// stop raster.  U rests on T(s) = D(s -> c) + T(c) for every s above c: U(c) = M(c) - T(c), M the upslope max of T,
// which is the upslope fold on the raw key T + 1 (0: no value), so cycles need no special case there either and no
// sum can exceed the largest T.  Sums stay <= 2^52 under the caller's bound N * rint(max w * 2^s) <= 2^52.
#include "dt_path_tiles.h"

#define FP_OPEN 0xFFFFFFFEu  // tag of a record that is still a pointer

typedef unsigned long long fp_u64;

__device__ __forceinline__ uint32_t fp_ptr(uint32_t w) { return w & 0xFFFu; }
__device__ __forceinline__ uint32_t fp_kind(uint32_t w) { return w >> 12; }
__device__ __forceinline__ uint32_t fp_word(uint32_t ptr, uint32_t kind) { return ptr | (kind << 12); }

// the word of value v at flat index c (0: NaN), and back.  MIN: the order of the float key is reversed
template <bool MIN>
__device__ __forceinline__ fp_u64 fp_key(float v, int64_t c) {
  if (v != v) return 0ull;
  const uint32_t b = v == 0.0f ? 0u : __float_as_uint(v);
  uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if (MIN) k = ~k;
  return ((fp_u64)k << 32) | (fp_u64)(0xFFFFFFFFu - (uint32_t)c);
}
template <bool MIN>
__device__ __forceinline__ float fp_value(fp_u64 key) {
  uint32_t k = (uint32_t)(key >> 32);
  if (MIN) k = ~k;
  return key == 0ull ? __uint_as_float(0x7FC00000u)
                     : __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ int64_t fp_where(fp_u64 key) {
  return key == 0ull ? -100 : (int64_t)(0xFFFFFFFFu - (uint32_t)key);
}

// the starting word of local cell l of the tile at (y0, x0): pt_classify's result packed; stop may be NULL
__device__ __forceinline__ uint32_t fp_init(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                            const uint8_t *__restrict__ stop, int64_t H, int64_t W, int64_t y0,
                                            int64_t x0, int l) {
  return pt_classify(fdr, dem, stop, H, W, y0, x0, l,
                     [](uint32_t kind, uint32_t ptr, bool) { return fp_word(ptr, kind); });
}

// the value word of local cell l with word w, for a fold of `values`
template <bool MIN>
__device__ __forceinline__ fp_u64 fp_cell_key(const float *__restrict__ values, uint32_t w, int64_t H, int64_t W,
                                              int64_t y0, int64_t x0, int l) {
  if (fp_kind(w) == PT_K_FAIL) return 0ull;  // outside the raster, or nodata
  const int64_t c = (y0 + (l >> 6)) * W + x0 + (l & 63);
  return fp_key<MIN>(values[c], c);
}

// What an upslope fold folds: key(c) the word of cell c (0: no value), put(c, v) the outputs of cell c from the fold's
// word v.  FpExtreme: a float raster's max / min and the cell that holds it.
template <bool MIN>
struct FpExtreme {
  const float *__restrict__ values;
  float *__restrict__ value;
  int64_t *__restrict__ where;
  __device__ __forceinline__ fp_u64 key(int64_t c) const { return fp_key<MIN>(values[c], c); }
  __device__ __forceinline__ void put(int64_t c, fp_u64 v) const {
    if (value) value[c] = fp_value<MIN>(v);
    if (where) where[c] = fp_where(v);
  }
};
// PsLongest: the raw key T + 1 of a downstream-sum plane (T < 0: no value); out = (M - T) * 2^-s, -100 without a T
struct PsLongest {
  const int64_t *__restrict__ T;
  double *__restrict__ out;
  int sbits;
  __device__ __forceinline__ fp_u64 key(int64_t c) const { return (fp_u64)(T[c] + 1); }
  __device__ __forceinline__ void put(int64_t c, fp_u64 m) const {
    const int64_t t = T[c];
    out[c] = (t < 0 || m == 0ull) ? -100.0 : ldexp((double)(int64_t)(m - 1ull - (fp_u64)t), -sbits);
  }
};
template <class P>
__device__ __forceinline__ fp_u64 fp_cell_key(const P &p, uint32_t w, int64_t W, int64_t y0, int64_t x0, int l) {
  if (fp_kind(w) == PT_K_FAIL) return 0ull;  // outside the raster, or nodata
  return p.key((y0 + (l >> 6)) * W + x0 + (l & 63));
}

// Upslope: pointer doubling with scatter.  s_w holds w[], s_v the cells' own words (and, in pass 3, the inflow of the
// entries), after a barrier.  On return (after a barrier) s_v[l] is the max over everything above l inside the tile.
__device__ __forceinline__ void fp_fold_up(uint32_t *s_w, fp_u64 *s_v, uint32_t (&w)[PT_CPT]) {
  const int t = (int)threadIdx.x;
  for (int r = 0; r < PT_ROUNDS; r++) {
    uint32_t tg[PT_CPT];
#pragma unroll
    for (int k = 0; k < PT_CPT; k++) {
      const int l = k * 256 + t;
      tg[k] = 0u;
      if (fp_kind(w[k]) == PT_K_PTR) {
        const uint32_t p = fp_ptr(w[k]);
        if (p != (uint32_t)l) {
          const fp_u64 v = __hip_atomic_load(&s_v[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (v) atomicMax(&s_v[p], v);
        }
        tg[k] = s_w[p];
      }
    }
    __syncthreads();
    int pend = 0;
#pragma unroll
    for (int k = 0; k < PT_CPT; k++) {
      if (fp_kind(w[k]) == PT_K_PTR) {
        w[k] = tg[k];
        s_w[k * 256 + t] = w[k];
        pend |= fp_kind(w[k]) == PT_K_PTR;
      }
    }
    if (!__syncthreads_or(pend)) break;
  }
  // every resolved cell delivers to its path's end, once
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    const uint32_t kd = fp_kind(w[k]), p = fp_ptr(w[k]);
    if (kd != PT_K_FAIL && kd != PT_K_PTR && p != (uint32_t)l) {
      const fp_u64 v = __hip_atomic_load(&s_v[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (v) atomicMax(&s_v[p], v);
    }
  }
  __syncthreads();
}

// Downstream: pointer doubling with gather.  s_w holds w[], s_v holds v[], after a barrier.  On return (after a
// barrier) v[] / s_v hold the max over each cell's in-tile path, its end included (SUM: the sum, modulo 2^64).
template <bool SUM = false>
__device__ __forceinline__ void fp_fold_down(uint32_t *s_w, fp_u64 *s_v, uint32_t (&w)[PT_CPT], fp_u64 (&v)[PT_CPT]) {
  const int t = (int)threadIdx.x;
  for (int r = 0; r < PT_ROUNDS; r++) {
    uint32_t tg[PT_CPT];
    fp_u64 tv[PT_CPT];
#pragma unroll
    for (int k = 0; k < PT_CPT; k++) {
      const bool open = fp_kind(w[k]) == PT_K_PTR;
      tg[k] = open ? s_w[fp_ptr(w[k])] : 0u;
      tv[k] = open ? s_v[fp_ptr(w[k])] : 0ull;
    }
    __syncthreads();
    int pend = 0;
#pragma unroll
    for (int k = 0; k < PT_CPT; k++) {
      if (fp_kind(w[k]) == PT_K_PTR) {
        w[k] = tg[k];
        v[k] = SUM ? v[k] + tv[k] : (tv[k] > v[k] ? tv[k] : v[k]);
        s_w[k * 256 + t] = w[k];
        s_v[k * 256 + t] = v[k];
        pend |= fp_kind(w[k]) == PT_K_PTR;
      }
    }
    if (!__syncthreads_or(pend)) break;
  }
}

// ---- upslope -----------------------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void k_fp_up_tile1(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                     const P fold, int64_t H, int64_t W, int64_t TX,
                                                     uint32_t *__restrict__ uptr, fp_u64 *__restrict__ S) {
  __shared__ uint32_t s_w[PT_T * PT_T];
  __shared__ fp_u64 s_v[PT_T * PT_T];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint32_t w[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    w[k] = fp_init(fdr, dem, nullptr, H, W, T.y0, T.x0, l);
    s_w[l] = w[k];
    s_v[l] = fp_cell_key(fold, w[k], W, T.y0, T.x0, l);
  }
  __syncthreads();
  fp_fold_up(s_w, s_v, w);
  uint32_t p_out = PT_NONE;
  fp_u64 s_out = 0ull;
  int l;
  int64_t y, x;
  if (pt_lane_cell(T, H, W, l, y, x)) {
    const uint32_t v = s_w[l];
    s_out = s_v[l];
    const uint32_t p = fp_ptr(v);
    bool diag;
    if (fp_kind(v) == PT_K_EXIT && p == (uint32_t)l) p_out = pt_exit_successor(fdr[y * W + x], TX, y, x, diag);
    else if (fp_kind(v) == PT_K_EXIT) p_out = pt_exit_own(p);
  }
  const int64_t n = (int64_t)blockIdx.x * PT_SLOTS + t;
  uptr[n] = p_out;
  S[n] = s_out;
}

// the scatter round of the upslope fold: a native max, no weight.  Most sends of the later rounds bring nothing new: a
// load tells, and only a word that raises S(p) is sent
struct FpUpFold {
  __device__ __forceinline__ void send(fp_u64 *to, fp_u64 sv, fp_u64) const {
    if (sv > __hip_atomic_load(to, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(to, sv);
  }
};
__global__ __launch_bounds__(256) void k_fp_up_node(const uint32_t *__restrict__ psrc, uint32_t *__restrict__ pdst,
                                                    fp_u64 *S, int64_t NN, uint32_t *flags, int r) {
  pt_scatter_round<false>(psrc, pdst, nullptr, nullptr, S, NN, flags, r, FpUpFold{});
}

template <class P>
__global__ __launch_bounds__(256) void k_fp_up_tile3(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                     const P fold, int64_t H, int64_t W, int64_t TX,
                                                     const fp_u64 *__restrict__ S) {
  __shared__ uint32_t s_w[PT_T * PT_T];
  __shared__ fp_u64 s_v[PT_T * PT_T];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint32_t w[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    w[k] = fp_init(fdr, dem, nullptr, H, W, T.y0, T.x0, l);
    s_w[l] = w[k];
    s_v[l] = fp_cell_key(fold, w[k], W, T.y0, T.x0, l);
  }
  __syncthreads();
  // entry inflow: S(f) of each feeder f in another tile (an exit of its tile, so a perimeter node whose S is complete)
  if (t < 252) {
    const int l = pt_slot_cell(t);
    const int64_t y = T.y0 + (l >> 6), x = T.x0 + (l & 63);
    if (y < H && x < W && !(dem && dem[y * W + x] <= -100.0f)) {
      fp_u64 ext = s_v[l];
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
        const fp_u64 v = S[pt_node(fy, fx, TX)];
        ext = v > ext ? v : ext;
      }
      s_v[l] = ext;
    }
  }
  __syncthreads();
  fp_fold_up(s_w, s_v, w);
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    const int64_t y = T.y0 + (l >> 6), x = T.x0 + (l & 63);
    if (y >= H || x >= W) continue;
    fold.put(y * W + x, s_v[l]);
  }
}

// ---- downstream --------------------------------------------------------------------------------------------------
template <bool MIN>
__global__ __launch_bounds__(256) void k_fp_dn_tile1(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                     const float *__restrict__ values,
                                                     const uint8_t *__restrict__ stop, int64_t H, int64_t W, int64_t TX,
                                                     uint4 *__restrict__ rec) {
  __shared__ uint32_t s_w[PT_T * PT_T];
  __shared__ fp_u64 s_v[PT_T * PT_T];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint32_t w[PT_CPT];
  fp_u64 v[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    w[k] = fp_init(fdr, dem, stop, H, W, T.y0, T.x0, l);
    v[k] = fp_cell_key<MIN>(values, w[k], H, W, T.y0, T.x0, l);
    s_w[l] = w[k];
    s_v[l] = v[k];
  }
  __syncthreads();
  fp_fold_down(s_w, s_v, w, v);
  uint4 o = make_uint4(PT_FAILP, 0xFFFFFFFFu, 0u, 0u);
  int l;
  int64_t y, x;
  if (pt_lane_cell(T, H, W, l, y, x)) {
    const uint32_t q = s_w[l];
    const uint32_t kd = fp_kind(q), p = fp_ptr(q);
    const fp_u64 key = s_v[l];
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    bool diag;
    if (kd == PT_K_EXIT && p == (uint32_t)l) {
      o = make_uint4(pt_exit_successor(fdr[y * W + x], TX, y, x, diag), FP_OPEN, lo, hi);
    } else if (kd == PT_K_EXIT) {
      o = make_uint4(pt_exit_own(p), FP_OPEN, lo, hi);
    } else if (kd == PT_K_STOP || (kd == PT_K_PTR && !stop)) {
      o = make_uint4(PT_RES, 0xFFFFFFFFu, lo, hi);  // stopped; or an in-tile cycle of a call without stop cells
    }
  }
  rec[(int64_t)blockIdx.x * PT_SLOTS + t] = o;
}

// One record round src -> dst (dt_path_tiles.h; k_dr_node is its other form): the words take the max, SUM: the sum
// modulo 2^64, and a record closes when the one it points at has.
template <bool SUM>
__device__ __forceinline__ void fp_dn_round(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t NN,
                                            uint32_t *flags, int r) {
  if (r >= 2 && flags[r - 1] == 0u) return;
  bool pend = false;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < NN; n += (int64_t)gridDim.x * 256) {
    const uint4 s = src[n];
    if (s.x & PT_RES) {
      if ((int32_t)s.y > r - 2) dst[n] = s;
      continue;
    }
    const uint4 q = src[s.x];
    const fp_u64 a = (fp_u64)s.z | ((fp_u64)s.w << 32), b = (fp_u64)q.z | ((fp_u64)q.w << 32);
    const fp_u64 m = SUM ? a + b : (a > b ? a : b);
    uint4 o;
    if (q.x == PT_FAILP) {
      o = make_uint4(PT_FAILP, (uint32_t)r, 0u, 0u);
    } else if (q.x & PT_RES) {
      o = make_uint4(PT_RES, (uint32_t)r, (uint32_t)m, (uint32_t)(m >> 32));
    } else {
      o = make_uint4(q.x, FP_OPEN, (uint32_t)m, (uint32_t)(m >> 32));
      pend = true;
    }
    dst[n] = o;
  }
  if (__ballot(pend) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(&flags[r + 1], 1u);
}
__global__ __launch_bounds__(256) void k_fp_dn_node(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t NN,
                                                    uint32_t *flags, int r) {
  fp_dn_round<false>(src, dst, NN, flags, r);
}
__global__ __launch_bounds__(256) void k_ps_dn_node(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t NN,
                                                    uint32_t *flags, int r) {
  fp_dn_round<true>(src, dst, NN, flags, r);
}

template <bool MIN>
__global__ __launch_bounds__(256) void k_fp_dn_tile3(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                     const float *__restrict__ values,
                                                     const uint8_t *__restrict__ stop, int64_t H, int64_t W, int64_t TX,
                                                     const uint4 *__restrict__ rec, float *__restrict__ value,
                                                     int64_t *__restrict__ where) {
  __shared__ uint32_t s_w[PT_T * PT_T];
  __shared__ fp_u64 s_v[PT_T * PT_T];
  __shared__ uint4 s_x[PT_SLOTS];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint32_t w[PT_CPT];
  fp_u64 v[PT_CPT];
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    w[k] = fp_init(fdr, dem, stop, H, W, T.y0, T.x0, l);
    v[k] = fp_cell_key<MIN>(values, w[k], H, W, T.y0, T.x0, l);
    s_w[l] = w[k];
    s_v[l] = v[k];
  }
  s_x[t] = rec[(int64_t)blockIdx.x * PT_SLOTS + t];
  __syncthreads();
  fp_fold_down(s_w, s_v, w, v);
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    const int64_t y = T.y0 + (l >> 6), x = T.x0 + (l & 63);
    if (y >= H || x >= W) continue;
    const uint32_t kd = fp_kind(w[k]), p = fp_ptr(w[k]);
    fp_u64 out = 0ull;
    if (kd == PT_K_STOP || (kd == PT_K_PTR && !stop)) {
      out = v[k];
    } else if (kd == PT_K_EXIT) {
      // the exit's record: everything from the exit cell on, and whether that path stopped
      const uint4 q = s_x[pt_slot((int)(p >> 6), (int)(p & 63))];
      const fp_u64 b = (fp_u64)q.z | ((fp_u64)q.w << 32);
      if (stop ? q.x == PT_RES : q.x != PT_FAILP) out = b > v[k] ? b : v[k];
    }
    if (value) value[y * W + x] = fp_value<MIN>(out);
    if (where) where[y * W + x] = fp_where(out);
  }
}

// ---- downstream sum ----------------------------------------------------------------------------------------------
// the starting sum of local cell l with word w: the cost of its move when that move stays in the tile, else 0 (an exit
// cell's move is its record's).  Every weight inside the raster is looked at, so a bad one is found wherever it lies.
__device__ __forceinline__ fp_u64 ps_cell_cost(const double *__restrict__ wt, uint32_t w, int64_t H, int64_t W,
                                               int64_t y0, int64_t x0, int l, int sbits, fp_u64 qmax, bool &bad) {
  const int64_t y = y0 + (l >> 6), x = x0 + (l & 63);
  if (y >= H || x >= W) return 0ull;
  const fp_u64 q = dt_quant_weight(wt[y * W + x], sbits, qmax, bad);
  return fp_kind(w) == PT_K_PTR ? q : 0ull;
}
// what a cell with the sum T gets (ok: its path stopped): T * 2^-s as float64 and -100, or T itself and -1
__device__ __forceinline__ void ps_put(double *__restrict__ out, int64_t c, bool ok, fp_u64 T, int sbits) {
  out[c] = ok ? ldexp((double)(int64_t)T, -sbits) : -100.0;
}
__device__ __forceinline__ void ps_put(int64_t *__restrict__ out, int64_t c, bool ok, fp_u64 T, int) {
  out[c] = ok ? (int64_t)T : -1;
}

__global__ __launch_bounds__(256) void k_ps_dn_tile1(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                     const double *__restrict__ wt, const uint8_t *__restrict__ stop,
                                                     int64_t H, int64_t W, int64_t TX, int sbits, fp_u64 qmax,
                                                     uint4 *__restrict__ rec, int *__restrict__ status) {
  __shared__ uint32_t s_w[PT_T * PT_T];
  __shared__ fp_u64 s_v[PT_T * PT_T];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint32_t w[PT_CPT];
  fp_u64 v[PT_CPT];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    w[k] = fp_init(fdr, dem, stop, H, W, T.y0, T.x0, l);
    v[k] = ps_cell_cost(wt, w[k], H, W, T.y0, T.x0, l, sbits, qmax, bad);
    s_w[l] = w[k];
    s_v[l] = v[k];
  }
  if (bad && status) atomicOr(status, DT_STATUS_BAD_WEIGHT);
  __syncthreads();
  fp_fold_down<true>(s_w, s_v, w, v);
  // the sum from the cell up to, not including, the node its record points at
  uint4 o = make_uint4(PT_FAILP, 0xFFFFFFFFu, 0u, 0u);
  int l;
  int64_t y, x;
  if (pt_lane_cell(T, H, W, l, y, x)) {
    const uint32_t q = s_w[l];
    const uint32_t kd = fp_kind(q), p = fp_ptr(q);
    const fp_u64 sum = s_v[l];
    if (kd == PT_K_EXIT && p == (uint32_t)l) {
      const int64_t c = y * W + x;
      int dy, dx;
      dt_d8_delta(fdr[c], dy, dx);
      bool again = false;
      const fp_u64 own = dt_quant_weight(wt[c], sbits, qmax, again);  // the move out of the tile
      o = make_uint4(pt_node(y + dy, x + dx, TX), FP_OPEN, (uint32_t)own, (uint32_t)(own >> 32));
    } else if (kd == PT_K_EXIT) {
      o = make_uint4(pt_exit_own(p), FP_OPEN, (uint32_t)sum, (uint32_t)(sum >> 32));
    } else if (kd == PT_K_STOP) {
      o = make_uint4(PT_RES, 0xFFFFFFFFu, (uint32_t)sum, (uint32_t)(sum >> 32));
    }  // still a pointer: on or into an in-tile cycle, which never stops
  }
  rec[(int64_t)blockIdx.x * PT_SLOTS + t] = o;
}

// OUT double: T * 2^-s and -100; OUT int64_t: the plane of the longest fold, T and -1
template <typename OUT>
__global__ __launch_bounds__(256) void k_ps_dn_tile3(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
                                                     const double *__restrict__ wt, const uint8_t *__restrict__ stop,
                                                     int64_t H, int64_t W, int64_t TX, int sbits, fp_u64 qmax,
                                                     const uint4 *__restrict__ rec, OUT *__restrict__ out) {
  __shared__ uint32_t s_w[PT_T * PT_T];
  __shared__ fp_u64 s_v[PT_T * PT_T];
  __shared__ uint4 s_x[PT_SLOTS];
  const PtTile T = pt_tile(TX);
  const int t = (int)threadIdx.x;
  uint32_t w[PT_CPT];
  fp_u64 v[PT_CPT];
  bool bad = false;  // pass 1 has reported it
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    w[k] = fp_init(fdr, dem, stop, H, W, T.y0, T.x0, l);
    v[k] = ps_cell_cost(wt, w[k], H, W, T.y0, T.x0, l, sbits, qmax, bad);
    s_w[l] = w[k];
    s_v[l] = v[k];
  }
  s_x[t] = rec[(int64_t)blockIdx.x * PT_SLOTS + t];
  __syncthreads();
  fp_fold_down<true>(s_w, s_v, w, v);
#pragma unroll
  for (int k = 0; k < PT_CPT; k++) {
    const int l = k * 256 + t;
    const int64_t y = T.y0 + (l >> 6), x = T.x0 + (l & 63);
    if (y >= H || x >= W) continue;
    const uint32_t kd = fp_kind(w[k]), p = fp_ptr(w[k]);
    bool ok = kd == PT_K_STOP;
    fp_u64 sum = v[k];
    if (kd == PT_K_EXIT) {
      // the exit's record: its own move and everything after it, when that path stopped
      const uint4 q = s_x[pt_slot((int)(p >> 6), (int)(p & 63))];
      ok = q.x == PT_RES;
      sum += (fp_u64)q.z | ((fp_u64)q.w << 32);
    }
    ps_put(out, y * W + x, ok, sum, sbits);
  }
}

// ---- carving: carved =max(lowest, filled - cut) in float32, the DEM's own value on nodata -------------------------
// filled NULL: no limit on the cut (carved = lowest).  carved may alias lowest.
__global__ __launch_bounds__(256) void k_carve_blend(const float *__restrict__ dem, const float *__restrict__ filled,
                                                     const float *lowest, int64_t N, float cut, float *carved) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < N; c += (int64_t)gridDim.x * 256) {
    const float d = dem[c];
    float o = d;
    if (!(d <= -100.0f)) {
      o = lowest[c];
      if (filled) {
        const float floor_ = filled[c] - cut;
        o = floor_ > o ? floor_ : o;
      }
    }
    carved[c] = o;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------
static PtLayout fp_layout(int64_t H, int64_t W, bool upslope, void *scratch) {
  DtCarver c(scratch);
  return pt_layout(c, H, W, upslope ? PT_BUF_PTR : PT_BUF_REC);
}

size_t dt_flowpath_scratch(int64_t H, int64_t W, int upslope) { return fp_layout(H, W, upslope != 0, nullptr).bytes; }

// the upslope fold of `fold` (FpExtreme, PsLongest) on L's pointer pair, S and flags (zeroed)
template <class P>
static void fp_launch_up(hipStream_t s, const PtLayout &L, const uint8_t *fdr, const float *dem, const P &fold,
                         int64_t H, int64_t W, int R) {
  pt_launch_passes(
      L, R,
      [&](dim3 g, dim3 b) {
        hipLaunchKernelGGL(k_fp_up_tile1<P>, g, b, 0, s, fdr, dem, fold, H, W, L.TX, L.uptr[0], L.S);
      },
      [&](dim3 g, dim3 b, int r, int src, int dst) {
        hipLaunchKernelGGL(k_fp_up_node, g, b, 0, s, L.uptr[src], L.uptr[dst], L.S, L.NN, L.flags, r);
      },
      [&](dim3 g, dim3 b, int) { hipLaunchKernelGGL(k_fp_up_tile3<P>, g, b, 0, s, fdr, dem, fold, H, W, L.TX, L.S); });
}

template <bool MIN>
static void fp_launch_down(hipStream_t s, const PtLayout &L, const uint8_t *fdr, const float *dem, const float *values,
                           const uint8_t *stop, int64_t H, int64_t W, int R, float *value, int64_t *where) {
  pt_launch_passes(
      L, R,
      [&](dim3 g, dim3 b) {
        hipLaunchKernelGGL(k_fp_dn_tile1<MIN>, g, b, 0, s, fdr, dem, values, stop, H, W, L.TX, L.rec[0]);
      },
      [&](dim3 g, dim3 b, int r, int src, int dst) {
        hipLaunchKernelGGL(k_fp_dn_node, g, b, 0, s, L.rec[src], L.rec[dst], L.NN, L.flags, r);
      },
      [&](dim3 g, dim3 b, int last) {
        hipLaunchKernelGGL(k_fp_dn_tile3<MIN>, g, b, 0, s, fdr, dem, values, stop, H, W, L.TX, L.rec[last], value,
                           where);
      });
}

int dt_launch_flowpath_upslope(hipStream_t s, const uint8_t *fdr, const float *dem, const float *values, int64_t H,
                               int64_t W, int kind, void *scratch, size_t scratch_bytes, float *value,
                               int64_t *where) {
  DT_REQUIRE(kind == 0 || kind == 1, "kind must be 0 (max) or 1 (min)");
  if (!value && !where) return DT_OK;
  const PtLayout L = fp_layout(H, W, true, scratch);
  int R;
  DT_TRY(pt_begin(s, L, H, W, scratch_bytes, R));
  if (!R) return DT_OK;
  if (kind == 1) fp_launch_up(s, L, fdr, dem, FpExtreme<true>{values, value, where}, H, W, R);
  else fp_launch_up(s, L, fdr, dem, FpExtreme<false>{values, value, where}, H, W, R);
  return DT_OK;
}

int dt_launch_flowpath_downstream(hipStream_t s, const uint8_t *fdr, const float *dem, const float *values,
                                  const uint8_t *stop, int64_t H, int64_t W, int kind, void *scratch,
                                  size_t scratch_bytes, float *value, int64_t *where) {
  DT_REQUIRE(kind == 0 || kind == 1, "kind must be 0 (max) or 1 (min)");
  if (!value && !where) return DT_OK;
  const PtLayout L = fp_layout(H, W, false, scratch);
  int R;
  DT_TRY(pt_begin(s, L, H, W, scratch_bytes, R));
  if (!R) return DT_OK;
  if (kind == 1) fp_launch_down<true>(s, L, fdr, dem, values, stop, H, W, R, value, where);
  else fp_launch_down<false>(s, L, fdr, dem, values, stop, H, W, R, value, where);
  return DT_OK;
}

// Path sums: the records of the downstream sum (flags [0, 64)) and, for the longest fold, the int64 plane of T behind
// them.  The upslope fold (flags [64, 128)) runs after the sum has been written out, so its 16 bytes per node lie over
// the first record buffer: `up` is that view.
struct PsLayout {
  PtLayout dn, up;
  int64_t *plane;
};
static PsLayout ps_layout(int64_t H, int64_t W, bool longest, void *scratch) {
  DtCarver c(scratch);
  PsLayout L = {pt_layout(c, H, W, PT_BUF_REC, 128), {}, nullptr};
  if (longest) L.plane = c.take<int64_t>((size_t)(H * W));
  L.dn.bytes = c.bytes();
  L.up = L.dn;
  if (longest && scratch) {
    L.up.flags = L.dn.flags + 64;
    L.up.uptr[0] = (uint32_t *)L.dn.rec[0];
    L.up.uptr[1] = L.up.uptr[0] + L.dn.NN;
    L.up.S = (fp_u64 *)L.dn.rec[0] + L.dn.NN;
  }
  return L;
}

size_t dt_pathsum_scratch(int64_t H, int64_t W, int longest) { return ps_layout(H, W, longest != 0, nullptr).dn.bytes; }

template <typename OUT>
static void ps_launch_down(hipStream_t s, const PtLayout &L, const uint8_t *fdr, const float *dem, const double *wt,
                           const uint8_t *stop, int64_t H, int64_t W, int frac_bits, int R, OUT *out, int *status) {
  const fp_u64 qmax = (1ull << 52) / (fp_u64)(H * W);
  pt_launch_passes(
      L, R,
      [&](dim3 g, dim3 b) {
        hipLaunchKernelGGL(k_ps_dn_tile1, g, b, 0, s, fdr, dem, wt, stop, H, W, L.TX, frac_bits, qmax, L.rec[0],
                           status);
      },
      [&](dim3 g, dim3 b, int r, int src, int dst) {
        hipLaunchKernelGGL(k_ps_dn_node, g, b, 0, s, L.rec[src], L.rec[dst], L.NN, L.flags, r);
      },
      [&](dim3 g, dim3 b, int last) {
        hipLaunchKernelGGL(k_ps_dn_tile3<OUT>, g, b, 0, s, fdr, dem, wt, stop, H, W, L.TX, frac_bits, qmax, L.rec[last],
                           out);
      });
}

int dt_launch_pathsum_downstream(hipStream_t s, const uint8_t *fdr, const float *dem, const double *wt,
                                 const uint8_t *stop, int64_t H, int64_t W, int frac_bits, void *scratch,
                                 size_t scratch_bytes, double *out, int *status) {
  if (!out) return DT_OK;
  const PsLayout L = ps_layout(H, W, false, scratch);
  int R;
  DT_TRY(pt_begin(s, L.dn, H, W, scratch_bytes, R));
  if (!R) return DT_OK;
  ps_launch_down(s, L.dn, fdr, dem, wt, stop, H, W, frac_bits, R, out, status);
  return DT_OK;
}

int dt_launch_pathsum_longest(hipStream_t s, const uint8_t *fdr, const float *dem, const double *wt, int64_t H,
                              int64_t W, int frac_bits, void *scratch, size_t scratch_bytes, double *out,
                              int *status) {
  if (!out) return DT_OK;
  const PsLayout L = ps_layout(H, W, true, scratch);
  int R;
  DT_TRY(pt_begin(s, L.dn, H, W, scratch_bytes, R));
  if (!R) return DT_OK;
  ps_launch_down(s, L.dn, fdr, dem, wt, nullptr, H, W, frac_bits, R, L.plane, status);
  fp_launch_up(s, L.up, fdr, dem, PsLongest{L.plane, out, frac_bits}, H, W, R);
  return DT_OK;
}

int dt_launch_carve_blend(hipStream_t s, const float *dem, const float *filled, const float *lowest, int64_t N,
                          float cut, float *carved) {
  if (N == 0) return DT_OK;
  hipLaunchKernelGGL(k_carve_blend, dim3(dt_capped_grid(N, 8192)), dim3(256), 0, s, dem, filled, lowest, N, cut,
                     carved);
  return DT_OK;
}
