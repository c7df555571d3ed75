// dt_reaches.hip -- reach catchments, per-reach stage tables and HAND inundation (net-new).
//
// The definitions are in descriptools_amd/reaches.py and include/descriptools_hip.h.  Every launch is asynchronous on
// the caller's stream and every sum is an integer sum, so no result depends on order, tiling or run.
//
//   catchments  rc_count     heads (link[c] == c) per block of 2048 cells
//               dt_launch_count_scan   the three scan launches of dt_streams.hip on those block counts: heads
//                            before each block, R
//               rc_rank      the rank of every head (block scan again): reach[head], heads[rank]
//               rc_fill      reach of the other network cells and catch, both through the head's rank
//   channels    rc_channels  one thread per cell, work only where reach >= 0: 64-bit integer atomics per reach
//   tables      rc_stages    the stages into device memory, 128 per launch, as kernel arguments (no host copy)
//               rc_tables    a workgroup per 64 x 64 tile.  A table of S slots x K bins x {count, Hq, Bq} in LDS; a
//                            slot is claimed per distinct reach id met in the tile (compare-and-swap on its key).  A
//                            thread merges the consecutive cells that share an entry in registers, adds the run with
//                            LDS integer atomics, and the workgroup flushes its non-zero entries with 64-bit global
//                            atomics into the bin (not cumulative) tables.  Cells whose reach finds no free slot add
//                            straight to global memory.
//               rc_prefix    a wave per reach: running sums along k, in place
//   inundate    rc_inundate  pointwise, 4 cells per thread, 16-B loads and stores
#include <cmath>

#include "dt_kernels.h"
#include "dt_reach_wet.h"

#define RC_TW 64
#define RC_TH 64
#define RC_SLOTS_MAX 16
#define RC_LDS_TABLE_BYTES 32768  // the LDS table's budget: S = min(16, budget / bytes per slot), at least 1
#define RC_STAGE_CHUNK 128
#define RC_NONE (-100)

// ---- catchments ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rc_count(const int64_t *__restrict__ link, int64_t N,
                                                  uint32_t *__restrict__ bcount) {
  __shared__ uint32_t s_w[4];
  const int64_t f0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) v += (f0 + k < N && link[f0 + k] == f0 + k) ? 1u : 0u;
  uint32_t total;
  dt_block_scan_256(v, s_w, &total);
  if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_rc_rank(const int64_t *__restrict__ link, int64_t N,
                                                 const int64_t *__restrict__ offsets, int32_t *__restrict__ reach,
                                                 int64_t *__restrict__ heads, int64_t cap) {
  __shared__ uint32_t s_w[4];
  const int64_t f0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  uint32_t flags = 0;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) flags |= (f0 + k < N && link[f0 + k] == f0 + k) ? 1u << k : 0u;
  uint32_t total;
  const uint32_t ex = dt_block_scan_256((uint32_t)__popc(flags), s_w, &total);
  int64_t id = offsets[blockIdx.x] + ex;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    if (flags & (1u << k)) {
      reach[f0 + k] = (int32_t)id;
      if (heads && id < cap) heads[id] = f0 + k;
      id++;
    }
  }
}

// the rank of the head `l` names, -100 when l is no head; only head cells of `reach` are read, and k_rc_fill writes
// only the others
__device__ __forceinline__ int32_t rc_rank_of(const int64_t *__restrict__ link, const int32_t *reach, int64_t N,
                                              int64_t l) {
  return (l >= 0 && l < N && link[l] == l) ? reach[l] : RC_NONE;
}

template <typename IDX, bool WRITE_REACH>
__global__ __launch_bounds__(256) void k_rc_fill(const int64_t *__restrict__ link, const IDX *__restrict__ idx,
                                                 int64_t N, int32_t *reach, int32_t *__restrict__ catch_) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  if (WRITE_REACH) {
    const int64_t l = link[c];
    if (l != c) reach[c] = rc_rank_of(link, reach, N, l);
  }
  if (catch_) {
    const int64_t i = (int64_t)idx[c];
    catch_[c] = (i >= 0 && i < N) ? rc_rank_of(link, reach, N, link[i]) : RC_NONE;
  }
}

struct RcCatchLayout {
  DtCountScan scan;
  int32_t *reach;  // the head ranks, when the caller asks for no reach raster
  size_t bytes;
};

static RcCatchLayout rc_catch_layout(int64_t N, bool own_reach, void *scratch) {
  RcCatchLayout L;
  DtCarver c(scratch);
  L.scan = dt_count_scan_carve(c, N, c.take<int64_t>(2));
  L.reach = own_reach ? c.take<int32_t>((size_t)N) : nullptr;
  L.bytes = c.bytes();
  return L;
}

size_t dt_reach_catchments_scratch(int64_t N, int own_reach) { return rc_catch_layout(N, own_reach != 0, nullptr).bytes; }

int dt_launch_reach_catchments(hipStream_t s, const int64_t *link, const void *idx, int idx_bytes, int64_t N,
                               void *scratch, size_t scratch_bytes, int32_t *reach, int32_t *catch_, int64_t *heads,
                               int64_t cap, int64_t *n_reaches_dev) {
  if (N == 0) {
    if (n_reaches_dev) DT_HIP(hipMemsetAsync(n_reaches_dev, 0, sizeof(int64_t), s));
    return DT_OK;
  }
  RcCatchLayout L = rc_catch_layout(N, reach == nullptr, scratch);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const DtCountScan &cs = L.scan;
  dim3 b(256), gr((unsigned)cs.nblk), gc((unsigned)((N + 255) / 256));
  hipLaunchKernelGGL(k_rc_count, gr, b, 0, s, link, N, cs.bcount);
  DT_TRY(dt_launch_count_scan(s, cs, cs.nblk));
  if (n_reaches_dev) DT_HIP(hipMemcpyAsync(n_reaches_dev, cs.meta, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (!reach && !catch_ && !heads) return DT_OK;
  int32_t *rk = reach ? reach : L.reach;
  hipLaunchKernelGGL(k_rc_rank, gr, b, 0, s, link, N, (const int64_t *)cs.offsets, rk, heads, cap);
  if (!reach && !catch_) return DT_OK;
  if (idx_bytes == 4) {
    if (reach) hipLaunchKernelGGL((k_rc_fill<int32_t, true>), gc, b, 0, s, link, (const int32_t *)idx, N, rk, catch_);
    else hipLaunchKernelGGL((k_rc_fill<int32_t, false>), gc, b, 0, s, link, (const int32_t *)idx, N, rk, catch_);
  } else {
    if (reach) hipLaunchKernelGGL((k_rc_fill<int64_t, true>), gc, b, 0, s, link, (const int64_t *)idx, N, rk, catch_);
    else hipLaunchKernelGGL((k_rc_fill<int64_t, false>), gc, b, 0, s, link, (const int64_t *)idx, N, rk, catch_);
  }
  return DT_OK;
}

// ---- channels --------------------------------------------------------------------------------------------------------
// end / down arrive as -1 (the launcher's memset), the three counts as 0.  A link has one last cell: the one without
// an edge, or whose edge leaves the link.
__global__ __launch_bounds__(256) void k_rc_channels(const uint8_t *__restrict__ fdr, const int32_t *__restrict__ reach,
                                                     int64_t H, int64_t W, int64_t R, int64_t *__restrict__ end,
                                                     int64_t *__restrict__ down,
                                                     unsigned long long *__restrict__ n_cells,
                                                     unsigned long long *__restrict__ n_card,
                                                     unsigned long long *__restrict__ n_diag) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= H * W) return;
  const int32_t r = reach[c];
  if (r < 0 || r >= R) return;
  atomicAdd(&n_cells[r], 1ull);
  const uint32_t code = fdr[c];
  int64_t d = -1;
  int32_t rd = -1;
  if (dt_d8_valid(code)) {
    int dy, dx;
    dt_d8_delta(code, dy, dx);
    const int64_t y = c / W, x = c - y * W;
    if (y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W) {
      const int64_t g = c + dy * W + dx;
      const int32_t rg = reach[g];
      if (rg >= 0) {
        d = g;
        rd = rg;
        atomicAdd((dy != 0 && dx != 0) ? &n_diag[r] : &n_card[r], 1ull);
      }
    }
  }
  if (d < 0) {
    end[r] = c;
    down[r] = -1;
  } else if (rd != r) {
    end[r] = d;
    down[r] = rd;
  }
}

int dt_launch_reach_channels(hipStream_t s, const uint8_t *fdr, const int32_t *reach, int64_t H, int64_t W, int64_t R,
                             int64_t *end, int64_t *down, int64_t *n_cells, int64_t *n_card, int64_t *n_diag) {
  if (R == 0) return DT_OK;
  const size_t rb = (size_t)R * 8;
  DT_HIP(hipMemsetAsync(end, 0xFF, rb, s));
  DT_HIP(hipMemsetAsync(down, 0xFF, rb, s));
  DT_HIP(hipMemsetAsync(n_cells, 0, rb, s));
  DT_HIP(hipMemsetAsync(n_card, 0, rb, s));
  DT_HIP(hipMemsetAsync(n_diag, 0, rb, s));
  if (H * W == 0) return DT_OK;
  hipLaunchKernelGGL(k_rc_channels, dim3((unsigned)((H * W + 255) / 256)), dim3(256), 0, s, fdr, reach, H, W, R, end,
                     down, (unsigned long long *)n_cells, (unsigned long long *)n_card, (unsigned long long *)n_diag);
  return DT_OK;
}

// ---- stage tables ----------------------------------------------------------------------------------------------------
struct RcStageChunk {
  double v[RC_STAGE_CHUNK];
};
__global__ void k_rc_stages(RcStageChunk ch, int n, double *__restrict__ dst) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = ch.v[threadIdx.x];
}

void dt_launch_host_doubles(hipStream_t s, const double *src_host, int n, double *dst) {
  for (int base = 0; base < n; base += RC_STAGE_CHUNK) {
    RcStageChunk ch;
    const int m = n - base < RC_STAGE_CHUNK ? n - base : RC_STAGE_CHUNK;
    for (int i = 0; i < RC_STAGE_CHUNK; i++) ch.v[i] = i < m ? src_host[base + i] : 0.0;
    hipLaunchKernelGGL(k_rc_stages, dim3(1), dim3(RC_STAGE_CHUNK), 0, s, ch, m, dst + base);
  }
}

struct RcTablesArgs {
  int64_t H, W, R;
  int K, S, sbits, uniform;
  double s0, inv_d;           // the uniform guess: ceil((h - s0) * inv_d)
  unsigned long long qmax;    // floor(2^52 / N)
};

// the smallest k with h <= st[k], for 0 <= h <= st[K - 1].  The uniform guess is taken only when the two neighbouring
// stages confirm it, so the result is the search's whatever the stages are.
__device__ __forceinline__ int rc_bin(const double *st, const RcTablesArgs &a, double h) {
  if (a.uniform) {
    const double g = ceil((h - a.s0) * a.inv_d);
    const int k = g < 0.0 ? 0 : (g > (double)(a.K - 1) ? a.K - 1 : (int)g);
#pragma unroll
    for (int o = 0; o < 3; o++) {
      const int j = k + (o == 0 ? 0 : (o == 1 ? -1 : 1));
      if (j >= 0 && j < a.K && h <= st[j] && (j == 0 || h > st[j - 1])) return j;
    }
  }
  int lo = 0, hi = a.K - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (h <= st[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// a thread's run of consecutive cells that share a table entry: key >= 0 names an LDS entry (slot * K + bin), key < 0
// the global entry ~key (reach * K + bin) of a reach without a slot
struct RcRun {
  long long key;
  uint32_t cnt;
  unsigned long long h, b;
};

template <bool SLOPE>
__device__ __forceinline__ void rc_flush_run(const RcRun &run, uint32_t *s_c, unsigned long long *s_h,
                                             unsigned long long *s_b, unsigned long long *cells,
                                             unsigned long long *Hq, unsigned long long *Bq) {
  if (run.cnt == 0u) return;
  if (run.key >= 0) {
    atomicAdd(&s_c[run.key], run.cnt);
    if (run.h) atomicAdd(&s_h[run.key], run.h);
    if (SLOPE && run.b) atomicAdd(&s_b[run.key], run.b);
  } else {
    const long long g = ~run.key;
    atomicAdd(&cells[g], (unsigned long long)run.cnt);
    if (run.h) atomicAdd(&Hq[g], run.h);
    if (SLOPE && run.b) atomicAdd(&Bq[g], run.b);
  }
}

template <typename HT, bool SLOPE, bool VEC>
__global__ __launch_bounds__(256) void k_rc_tables(const int32_t *__restrict__ catch_, const HT *__restrict__ hand,
                                                   const float *__restrict__ slope,
                                                   const double *__restrict__ stages, RcTablesArgs a,
                                                   unsigned long long *cells, unsigned long long *Hq,
                                                   unsigned long long *Bq, int *status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int SK = a.S * a.K;
  double *s_st = reinterpret_cast<double *>(s_raw);
  unsigned long long *s_h = reinterpret_cast<unsigned long long *>(s_st + a.K);
  unsigned long long *s_b = s_h + (SLOPE ? SK : 0);
  uint32_t *s_c = reinterpret_cast<uint32_t *>(s_b + SK);
  int *s_key = reinterpret_cast<int *>(s_c + SK);
  for (int i = threadIdx.x; i < a.K; i += 256) s_st[i] = stages[i];
  for (int i = threadIdx.x; i < SK; i += 256) {
    s_h[i] = 0ull;
    if (SLOPE) s_b[i] = 0ull;
    s_c[i] = 0u;
  }
  if ((int)threadIdx.x < a.S) s_key[threadIdx.x] = -1;
  __syncthreads();

  const int tiles_x = (int)((a.W + RC_TW - 1) / RC_TW);
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int64_t x = (int64_t)tx * RC_TW + (int64_t)(threadIdx.x & 15u) * 4;
  const int64_t yb = (int64_t)ty * RC_TH + (int64_t)(threadIdx.x >> 4);
  const double smax = s_st[a.K - 1];
  RcRun run = {0, 0u, 0ull, 0ull};
  int last_r = -1, last_slot = -1;
  bool bad_w = false, bad_r = false;
#pragma unroll
  for (int j = 0; j < RC_TH / 16; j++) {
    const int64_t y = yb + 16 * j;
    if (y >= a.H || x >= a.W) continue;
    const int64_t f = y * a.W + x;
    int32_t rr[4];
    HT hh[4];
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {  // W is a multiple of 4 and the rasters are 16-B aligned
      const int4 v = *reinterpret_cast<const int4 *>(catch_ + f);
      rr[0] = v.x; rr[1] = v.y; rr[2] = v.z; rr[3] = v.w;
      dt_load4(hand, f, hh);
      if (SLOPE) {
        const float4 q = *reinterpret_cast<const float4 *>(slope + f);
        ss[0] = q.x; ss[1] = q.y; ss[2] = q.z; ss[3] = q.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const bool in = x + i < a.W;
        rr[i] = in ? catch_[f + i] : RC_NONE;
        hh[i] = in ? hand[f + i] : (HT)0;
        if (SLOPE) ss[i] = in ? slope[f + i] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = rr[i];
      if (r < 0) continue;
      if (r >= a.R) {
        bad_r = true;
        continue;
      }
      const double h = (double)hh[i];
      if (!(h >= 0.0 && h <= smax)) continue;
      const int k = rc_bin(s_st, a, h);
      const unsigned long long hq = (unsigned long long)rint(ldexp(h, a.sbits));
      unsigned long long wq = 0ull;
      if (SLOPE) {
        const float sl = ss[i];
        const double t = (sl > 0.f && sl <= 3.402823466e+38f) ? (double)sl / 100.0 : 0.0;
        const double q = rint(ldexp(sqrt(1.0 + t * t), a.sbits));
        if (q <= (double)a.qmax) wq = (unsigned long long)q;
        else bad_w = true;
      }
      if (r != last_r) {
        last_r = r;
        last_slot = dt_claim_slot(s_key, a.S, r);
      }
      const long long key = last_slot >= 0 ? (long long)last_slot * a.K + k : ~((long long)r * a.K + k);
      if (key != run.key) {
        rc_flush_run<SLOPE>(run, s_c, s_h, s_b, cells, Hq, Bq);
        run.key = key;
        run.cnt = 0u;
        run.h = run.b = 0ull;
      }
      run.cnt++;
      run.h += hq;
      run.b += wq;
    }
  }
  rc_flush_run<SLOPE>(run, s_c, s_h, s_b, cells, Hq, Bq);
  if (bad_w) atomicOr(status, DT_STATUS_BAD_WEIGHT);
  if (bad_r) atomicOr(status, DT_STATUS_REACH_RANGE);
  __syncthreads();
  for (int e = threadIdx.x; e < SK; e += 256) {
    const uint32_t c = s_c[e];
    if (c == 0u) continue;
    const int slot = e / a.K;
    const long long g = (long long)s_key[slot] * a.K + (e - slot * a.K);
    atomicAdd(&cells[g], (unsigned long long)c);
    const unsigned long long h = s_h[e];
    if (h) atomicAdd(&Hq[g], h);
    if (SLOPE) {
      const unsigned long long b = s_b[e];
      if (b) atomicAdd(&Bq[g], b);
    }
  }
}

// running sums along k, a wave per reach; without a slope raster every bed weight is wq1, so Bq = cells * wq1
template <bool SLOPE>
__global__ __launch_bounds__(256) void k_rc_prefix(unsigned long long *cells, unsigned long long *Hq,
                                                   unsigned long long *Bq, int64_t R, int K, unsigned long long wq1) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long carry[3] = {0ull, 0ull, 0ull};
  unsigned long long *const tab[3] = {cells, Hq, Bq};
  for (int base = 0; base < K; base += 64) {
    const int k = base + lane;
    unsigned long long cum0 = 0ull;
#pragma unroll
    for (int t = 0; t < 3; t++) {
      if (t == 2 && !SLOPE) {
        if (k < K) Bq[r * K + k] = cum0 * wq1;
        continue;
      }
      unsigned long long x = k < K ? tab[t][r * K + k] : 0ull;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = (unsigned long long)__shfl_up((long long)x, o);
        if (lane >= o) x += u;
      }
      x += carry[t];
      if (k < K) tab[t][r * K + k] = x;
      carry[t] = (unsigned long long)__shfl((long long)x, 63);
      if (t == 0) cum0 = x;
    }
  }
}

static int rc_slots(int K, bool slope) {
  const int per = K * (slope ? 20 : 12);
  int S = RC_LDS_TABLE_BYTES / per;
  return S > RC_SLOTS_MAX ? RC_SLOTS_MAX : (S < 1 ? 1 : S);
}

size_t dt_reach_tables_scratch(int K) { return dt_align256((size_t)K * sizeof(double)); }

template <typename HT>
static void rc_launch_tables(hipStream_t s, dim3 grid, size_t lds, bool with_slope, bool vec, const int32_t *catch_,
                             const HT *hand, const float *slope, const double *stages, const RcTablesArgs &a,
                             unsigned long long *cells, unsigned long long *Hq, unsigned long long *Bq, int *status) {
  dim3 b(256);
  if (with_slope) {
    if (vec) hipLaunchKernelGGL((k_rc_tables<HT, true, true>), grid, b, lds, s, catch_, hand, slope, stages, a, cells, Hq, Bq, status);
    else hipLaunchKernelGGL((k_rc_tables<HT, true, false>), grid, b, lds, s, catch_, hand, slope, stages, a, cells, Hq, Bq, status);
  } else {
    if (vec) hipLaunchKernelGGL((k_rc_tables<HT, false, true>), grid, b, lds, s, catch_, hand, slope, stages, a, cells, Hq, Bq, status);
    else hipLaunchKernelGGL((k_rc_tables<HT, false, false>), grid, b, lds, s, catch_, hand, slope, stages, a, cells, Hq, Bq, status);
  }
}

int dt_launch_reach_tables(hipStream_t s, const int32_t *catch_, const void *hand, int hand_bytes, const float *slope,
                           int64_t H, int64_t W, const double *stages_host, int K, int64_t R, int frac_bits,
                           void *scratch, size_t scratch_bytes, int64_t *cells, int64_t *Hq, int64_t *Bq, int *status,
                           int slots) {
  const int64_t N = H * W;
  if (R == 0) return DT_OK;
  const size_t tb = (size_t)R * (size_t)K * 8;
  DT_HIP(hipMemsetAsync(cells, 0, tb, s));
  DT_HIP(hipMemsetAsync(Hq, 0, tb, s));
  DT_HIP(hipMemsetAsync(Bq, 0, tb, s));
  if (N == 0) return DT_OK;
  DT_REQUIRE(scratch_bytes >= dt_reach_tables_scratch(K), "scratch too small");
  double *d_st = (double *)scratch;
  dt_launch_host_doubles(s, stages_host, K, d_st);
  RcTablesArgs a;
  a.H = H; a.W = W; a.R = R; a.K = K; a.sbits = frac_bits;
  a.S = rc_slots(K, slope != nullptr);
  if (slots < 0) a.S = 0;  // no LDS table: every cell adds straight to global memory (A/B runs)
  else if (slots >= 1 && slots < a.S) a.S = slots;
  a.qmax = (1ull << 52) / (unsigned long long)N;
  a.uniform = 0; a.s0 = stages_host[0]; a.inv_d = 0.0;
  if (K >= 2) {
    const double d = (stages_host[K - 1] - stages_host[0]) / (double)(K - 1);
    bool uni = d > 0.0 && std::isfinite(1.0 / d);
    for (int k = 0; uni && k < K; k++) uni = fabs(stages_host[k] - (stages_host[0] + k * d)) <= 0.25 * d;
    a.uniform = uni ? 1 : 0;
    a.inv_d = uni ? 1.0 / d : 0.0;
  }
  const size_t SK = (size_t)a.S * K;
  const size_t lds = (size_t)K * 8 + SK * (slope ? 20 : 12) + (size_t)a.S * 4;
  const int64_t tiles = ((H + RC_TH - 1) / RC_TH) * ((W + RC_TW - 1) / RC_TW);
  const bool vec = (W & 3) == 0 && ((uintptr_t)catch_ & 15u) == 0 && ((uintptr_t)hand & 15u) == 0 &&
                   ((uintptr_t)slope & 15u) == 0;
  unsigned long long *c = (unsigned long long *)cells, *h = (unsigned long long *)Hq, *bq = (unsigned long long *)Bq;
  if (hand_bytes == 4)
    rc_launch_tables<float>(s, dim3((unsigned)tiles), lds, slope != nullptr, vec, catch_, (const float *)hand, slope, d_st, a, c, h, bq, status);
  else
    rc_launch_tables<double>(s, dim3((unsigned)tiles), lds, slope != nullptr, vec, catch_, (const double *)hand, slope, d_st, a, c, h, bq, status);
  const unsigned long long wq1 = (unsigned long long)rint(ldexp(1.0, frac_bits));
  dim3 gp((unsigned)((R + 3) / 4));
  if (slope) hipLaunchKernelGGL(k_rc_prefix<true>, gp, dim3(256), 0, s, c, h, bq, R, K, wq1);
  else hipLaunchKernelGGL(k_rc_prefix<false>, gp, dim3(256), 0, s, c, h, bq, R, K, wq1);
  return DT_OK;
}

// ---- inundation ------------------------------------------------------------------------------------------------------
// (the predicate and the depth: dt_reach_wet.h, shared with connected inundation in dt_regions.hip)
template <typename HT>
__device__ __forceinline__ float rc_depth(int32_t r, HT hv, const double *__restrict__ stage, int64_t R) {
  bool wet;
  return dt_rc_depth(r, hv, stage, R, wet);
}

template <typename HT, bool VEC>
__global__ __launch_bounds__(256) void k_rc_inundate(const int32_t *__restrict__ catch_, const HT *__restrict__ hand,
                                                     const double *__restrict__ stage, int64_t N, int64_t R,
                                                     float *__restrict__ depth) {
  const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (f >= N) return;
  if (VEC && f + 4 <= N) {
    const int4 v = *reinterpret_cast<const int4 *>(catch_ + f);
    HT hh[4];
    dt_load4(hand, f, hh);
    *reinterpret_cast<float4 *>(depth + f) = make_float4(rc_depth(v.x, hh[0], stage, R), rc_depth(v.y, hh[1], stage, R),
                                                         rc_depth(v.z, hh[2], stage, R), rc_depth(v.w, hh[3], stage, R));
    return;
  }
  for (int i = 0; i < 4 && f + i < N; i++) depth[f + i] = rc_depth(catch_[f + i], hand[f + i], stage, R);
}

int dt_launch_inundate(hipStream_t s, const int32_t *catch_, const void *hand, int hand_bytes, const double *stage,
                       int64_t N, int64_t R, float *depth) {
  if (N == 0) return DT_OK;
  const bool vec = ((uintptr_t)catch_ & 15u) == 0 && ((uintptr_t)hand & 15u) == 0 && ((uintptr_t)depth & 15u) == 0;
  dim3 g((unsigned)((N + 1023) / 1024)), b(256);
  if (hand_bytes == 4) {
    if (vec) hipLaunchKernelGGL((k_rc_inundate<float, true>), g, b, 0, s, catch_, (const float *)hand, stage, N, R, depth);
    else hipLaunchKernelGGL((k_rc_inundate<float, false>), g, b, 0, s, catch_, (const float *)hand, stage, N, R, depth);
  } else {
    if (vec) hipLaunchKernelGGL((k_rc_inundate<double, true>), g, b, 0, s, catch_, (const double *)hand, stage, N, R, depth);
    else hipLaunchKernelGGL((k_rc_inundate<double, false>), g, b, 0, s, catch_, (const double *)hand, stage, N, R, depth);
  }
  return DT_OK;
}
