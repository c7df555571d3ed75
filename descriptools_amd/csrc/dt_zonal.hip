// dt_zonal.hip -- zonal statistics: label compaction, per-zone tables, per-zone histograms and cross-tabulation, and
// painting a table back onto its zones (net-new).
//
// The definitions are in descriptools_amd/zonal.py and include/descriptools_hip.h.  Every launch is asynchronous on the
// caller's stream and every sum is an integer sum, so no result depends on order, tiling or run.
//
//   compact   zn_mark      a presence bitmap of `limit` bits: 32-bit atomic OR, skipped where the bit is seen set
//             zn_wcount    set bits per block of DT_SCAN_CHUNK bitmap words
//             dt_launch_count_scan   the three scan launches of dt_streams.hip on those block counts: n_zones
//             zn_rank      the rank of every word's first bit (block scan again) and labels_of[rank]
//             zn_relabel   zones[c] = the word's rank + the set bits below the label's own
//   tables    zn_tables    a workgroup per 64 x 64 tile, a lane 4 x 4 cells as in k_rc_tables.  A lane merges its
//                          consecutive cells of one zone in registers, adds the run to a per-workgroup table in LDS and
//                          the workgroup flushes the non-empty entries with 64-bit global atomics, min / max with
//                          atomic min / max on the order-preserving key of the float.  The LDS table is direct (slot =
//                          zone, in up to ZN_COPIES copies) for up to ZN_DIRECT_MAX zones, else ZN_SLOTS slots claimed
//                          by compare-and-swap; a zone without a slot adds its runs straight to global memory.
//             zn_keys      min / max keys back to floats, NaN on empty zones
//   counts    zn_counts    the same tile walk on (zone, column) entries: the column is the bin of the value among the
//                          edges (binary search on the exact float64) or the cell of a second zone raster
//   paint     zn_paint     pointwise gather of 4- or 8-byte words, 4 cells per lane, 16-B loads and stores
#include <cmath>
#include <type_traits>

#include "dt_kernels.h"

#define ZN_TW 64
#define ZN_TH 64
#define ZN_NONE (-100)
#define ZN_DIRECT_MAX 256         // zones at most for slot = zone: 256 x 48 B = 12 KiB of LDS on float64 values
#define ZN_SLOTS 64               // claimed slots per workgroup otherwise: 3.3 KiB
#define ZN_COPIES 16              // copies of a direct table at most
#define ZN_DIRECT_GRID 2048u      // workgroups of a launch with a direct table: 8 per CU
#define ZN_COUNTS_TABLE_BYTES 16384  // the counts table's LDS budget (beside the edges, 8 KiB at most)
#define ZN_COUNTS_SLOTS_MAX 16
enum { ZN_COUNT = 1, ZN_S1 = 2, ZN_S2 = 4, ZN_MIN = 8, ZN_MAX = 16 };

typedef unsigned long long zn_u64;

// the order-preserving unsigned key of a float: a < b (as reals, -0 = +0 aside) exactly when key(a) < key(b)
template <typename VT> struct ZnKey;
template <> struct ZnKey<float> {
  typedef uint32_t T;
  static __device__ __forceinline__ T of(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  static __device__ __forceinline__ T bits(T k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }  // the float's
  static __device__ __forceinline__ T nan_bits() { return 0x7FC00000u; }
};
template <> struct ZnKey<double> {
  typedef zn_u64 T;
  static __device__ __forceinline__ T of(double v) {
    const zn_u64 b = (zn_u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
  }
  static __device__ __forceinline__ T bits(T k) { return (k >> 63) ? (k & ~(1ull << 63)) : ~k; }
  static __device__ __forceinline__ T nan_bits() { return 0x7FF8000000000000ull; }
};

// four consecutive cells of a value raster (float32 / float64) or of a second zone raster (int32), 16-byte loads
template <typename VT>
__device__ __forceinline__ void zn_load4(const VT *__restrict__ src, int64_t f, VT (&vv)[4]) {
  dt_load4(src, f, vv);
}
template <>
__device__ __forceinline__ void zn_load4<int32_t>(const int32_t *__restrict__ src, int64_t f, int32_t (&vv)[4]) {
  const int4 v = *reinterpret_cast<const int4 *>(src + f);
  vv[0] = v.x; vv[1] = v.y; vv[2] = v.z; vv[3] = v.w;
}

// ---- compact ---------------------------------------------------------------------------------------------------------
template <typename LT>
__global__ __launch_bounds__(256) void k_zn_mark(const LT *__restrict__ labels, int64_t N, int64_t limit,
                                                 uint32_t *bm) {
  const int64_t c0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int64_t c = c0 + 256 * i;
    if (c >= N) break;
    const int64_t l = (int64_t)labels[c];
    if (l < 0 || l >= limit) continue;
    const uint32_t bit = 1u << (l & 31);
    uint32_t *w = &bm[l >> 5];
    // labels come in patches: most cells find their bit set and add no atomic
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
  }
}

__global__ __launch_bounds__(256) void k_zn_wcount(const uint32_t *__restrict__ bm, int64_t nwords,
                                                   uint32_t *__restrict__ bcount) {
  __shared__ uint32_t s_w[4];
  const int64_t w0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) v += w0 + k < nwords ? (uint32_t)__popc(bm[w0 + k]) : 0u;
  uint32_t total;
  dt_block_scan_256(v, s_w, &total);
  if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_zn_rank(const uint32_t *__restrict__ bm, int64_t nwords,
                                                 const int64_t *__restrict__ offsets, uint32_t *__restrict__ wrank,
                                                 int64_t *__restrict__ labels_of, int64_t cap) {
  __shared__ uint32_t s_w[4];
  const int64_t w0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  uint32_t bits[DT_SCAN_CPT];
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    bits[k] = w0 + k < nwords ? bm[w0 + k] : 0u;
    v += (uint32_t)__popc(bits[k]);
  }
  uint32_t total;
  const uint32_t ex = dt_block_scan_256(v, s_w, &total);
  int64_t id = offsets[blockIdx.x] + ex;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    if (w0 + k >= nwords) break;
    wrank[w0 + k] = (uint32_t)id;
    uint32_t b = bits[k];
    while (b) {
      const int j = __ffs((int)b) - 1;
      b &= b - 1u;
      if (labels_of && id < cap) labels_of[id] = (w0 + k) * 32 + j;
      id++;
    }
  }
}

template <typename LT>
__global__ __launch_bounds__(256) void k_zn_relabel(const LT *__restrict__ labels, int64_t N, int64_t limit,
                                                    const uint32_t *__restrict__ bm,
                                                    const uint32_t *__restrict__ wrank, int32_t *__restrict__ zones) {
  const int64_t c0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int64_t c = c0 + 256 * i;
    if (c >= N) break;
    const int64_t l = (int64_t)labels[c];
    int32_t z = ZN_NONE;
    if (l >= 0 && l < limit) z = (int32_t)(wrank[l >> 5] + (uint32_t)__popc(bm[l >> 5] & ((1u << (l & 31)) - 1u)));
    zones[c] = z;
  }
}

struct ZnCompactLayout {
  DtCountScan scan;
  int64_t nwords;
  uint32_t *bm, *wrank;
  size_t bytes;
};

static ZnCompactLayout zn_compact_layout(int64_t limit, void *scratch) {
  ZnCompactLayout L;
  DtCarver c(scratch);
  L.nwords = (limit + 31) / 32;
  L.scan = dt_count_scan_carve(c, L.nwords, c.take<int64_t>(2));
  L.bm = c.take<uint32_t>((size_t)L.nwords);
  L.wrank = c.take<uint32_t>((size_t)L.nwords);
  L.bytes = c.bytes();
  return L;
}

size_t dt_zonal_compact_scratch(int64_t limit) { return zn_compact_layout(limit, nullptr).bytes; }

int dt_launch_zonal_compact(hipStream_t s, const void *labels, int label_bytes, int64_t N, int64_t limit,
                            void *scratch, size_t scratch_bytes, int32_t *zones, int64_t *labels_of, int64_t cap,
                            int64_t *n_zones_dev) {
  if (N == 0) {
    if (n_zones_dev) DT_HIP(hipMemsetAsync(n_zones_dev, 0, sizeof(int64_t), s));
    return DT_OK;
  }
  ZnCompactLayout L = zn_compact_layout(limit, scratch);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const DtCountScan &cs = L.scan;
  DT_HIP(hipMemsetAsync(L.bm, 0, (size_t)L.nwords * sizeof(uint32_t), s));
  dim3 b(256), gw((unsigned)cs.nblk), gc((unsigned)((N + 1023) / 1024));
  if (label_bytes == 4) hipLaunchKernelGGL(k_zn_mark<int32_t>, gc, b, 0, s, (const int32_t *)labels, N, limit, L.bm);
  else hipLaunchKernelGGL(k_zn_mark<int64_t>, gc, b, 0, s, (const int64_t *)labels, N, limit, L.bm);
  hipLaunchKernelGGL(k_zn_wcount, gw, b, 0, s, (const uint32_t *)L.bm, L.nwords, cs.bcount);
  DT_TRY(dt_launch_count_scan(s, cs, cs.nblk));
  if (n_zones_dev) DT_HIP(hipMemcpyAsync(n_zones_dev, cs.meta, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (!zones && !labels_of) return DT_OK;
  hipLaunchKernelGGL(k_zn_rank, gw, b, 0, s, (const uint32_t *)L.bm, L.nwords, (const int64_t *)cs.offsets, L.wrank,
                     labels_of, cap);
  if (!zones) return DT_OK;
  if (label_bytes == 4)
    hipLaunchKernelGGL(k_zn_relabel<int32_t>, gc, b, 0, s, (const int32_t *)labels, N, limit, (const uint32_t *)L.bm,
                       (const uint32_t *)L.wrank, zones);
  else
    hipLaunchKernelGGL(k_zn_relabel<int64_t>, gc, b, 0, s, (const int64_t *)labels, N, limit, (const uint32_t *)L.bm,
                       (const uint32_t *)L.wrank, zones);
  return DT_OK;
}

// ---- tables ----------------------------------------------------------------------------------------------------------
struct ZnTablesArgs {
  int64_t H, W, Z;
  unsigned tiles;
  int S, direct, rep, sbits, want, has_nodata;  // direct: S = Z * rep, a lane adds to copy threadIdx.x % rep
  double origin, nodata;
};

// a lane's run of consecutive cells of one zone: key >= 0 names an LDS slot, key < 0 the zone ~key without one
template <typename KT>
struct ZnRun {
  int key;
  uint32_t cnt;
  zn_u64 s1, lo, hi;  // s1 wraps: the sum of signed q modulo 2^64
  KT mn, mx;
};

template <typename KT>
struct ZnTables {
  zn_u64 *cnt, *s1, *lo, *hi;
  KT *mn, *mx;
};

template <typename KT>
__device__ __forceinline__ void zn_flush_run(const ZnRun<KT> &run, int want, uint32_t *s_c, zn_u64 *s_s1, zn_u64 *s_lo,
                                             zn_u64 *s_hi, KT *s_mn, KT *s_mx, const ZnTables<KT> &g) {
  if (run.cnt == 0u) return;
  if (run.key >= 0) {
    const int k = run.key;
    atomicAdd(&s_c[k], run.cnt);
    if ((want & ZN_S1) && run.s1) atomicAdd(&s_s1[k], run.s1);
    if (want & ZN_S2) {
      if (run.lo) atomicAdd(&s_lo[k], run.lo);
      if (run.hi) atomicAdd(&s_hi[k], run.hi);
    }
    if (want & ZN_MIN) atomicMin(&s_mn[k], run.mn);
    if (want & ZN_MAX) atomicMax(&s_mx[k], run.mx);
  } else {
    const int64_t z = (int64_t)~run.key;
    if (want & ZN_COUNT) atomicAdd(&g.cnt[z], (zn_u64)run.cnt);
    if ((want & ZN_S1) && run.s1) atomicAdd(&g.s1[z], run.s1);
    if (want & ZN_S2) {
      if (run.lo) atomicAdd(&g.lo[z], run.lo);
      if (run.hi) atomicAdd(&g.hi[z], run.hi);
    }
    if (want & ZN_MIN) atomicMin(&g.mn[z], run.mn);
    if (want & ZN_MAX) atomicMax(&g.mx[z], run.mx);
  }
}

template <typename VT, bool VEC>
__global__ __launch_bounds__(256) void k_zn_tables(const int32_t *__restrict__ zones, const VT *__restrict__ values,
                                                   ZnTablesArgs a, ZnTables<typename ZnKey<VT>::T> g, int *status) {
  typedef typename ZnKey<VT>::T KT;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int S = a.S;
  zn_u64 *s_s1 = reinterpret_cast<zn_u64 *>(s_raw);
  zn_u64 *s_lo = s_s1 + S;
  zn_u64 *s_hi = s_lo + S;
  KT *s_mn = reinterpret_cast<KT *>(s_hi + S);
  KT *s_mx = s_mn + S;
  uint32_t *s_c = reinterpret_cast<uint32_t *>(s_mx + S);
  int *s_key = reinterpret_cast<int *>(s_c + S);
  for (int i = threadIdx.x; i < S; i += 256) {
    s_s1[i] = s_lo[i] = s_hi[i] = 0ull;
    s_mn[i] = ~(KT)0;
    s_mx[i] = (KT)0;
    s_c[i] = 0u;
    s_key[i] = -1;
  }
  __syncthreads();

  const unsigned tiles_x = (unsigned)((a.W + ZN_TW - 1) / ZN_TW);
  ZnRun<KT> run = {0, 0u, 0ull, 0ull, 0ull, ~(KT)0, (KT)0};
  const int copy0 = a.direct ? (int)(threadIdx.x % (unsigned)a.rep) * (int)a.Z : 0;
  int last_z = -1, last_slot = -1;
  bool bad_z = false, bad_q = false;
  // a claimed table belongs to one tile (the grid covers the tiles); a direct one serves tile after tile
  for (unsigned tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const unsigned ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int64_t x = (int64_t)tx * ZN_TW + (int64_t)(threadIdx.x & 15u) * 4;
    const int64_t yb = (int64_t)ty * ZN_TH + (int64_t)(threadIdx.x >> 4);
#pragma unroll
    for (int j = 0; j < ZN_TH / 16; j++) {
      const int64_t y = yb + 16 * j;
      if (y >= a.H || x >= a.W) continue;
      const int64_t f = y * a.W + x;
      int32_t zz[4];
      VT vv[4];
      if (VEC) {  // W is a multiple of 4 and the rasters are 16-B aligned
        zn_load4(zones, f, zz);
        zn_load4(values, f, vv);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const bool in = x + i < a.W;
          zz[i] = in ? zones[f + i] : ZN_NONE;
          vv[i] = in ? values[f + i] : (VT)0;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int z = zz[i];
        if (z < 0) continue;
        if (z >= a.Z) {
          bad_z = true;
          continue;
        }
        VT v = vv[i];
        const double d = (double)v;
        if (!(fabs(d) < INFINITY)) continue;  // NaN, +-inf
        if (a.has_nodata && d == a.nodata) continue;
        if (v == (VT)0) v = (VT)0;  // -0.0 counts as +0.0
        const double qd = rint(ldexp(d - a.origin, a.sbits));
        if (!(fabs(qd) <= 2147483647.0)) {
          bad_q = true;
          continue;
        }
        const long long q = (long long)qd;
        const zn_u64 q2 = (zn_u64)(q * q);
        if (z != last_z) {
          last_z = z;
          last_slot = a.direct ? copy0 + z : dt_claim_slot(s_key, S, z);
        }
        const int key = last_slot >= 0 ? last_slot : ~z;
        if (key != run.key) {
          zn_flush_run(run, a.want, s_c, s_s1, s_lo, s_hi, s_mn, s_mx, g);
          run.key = key;
          run.cnt = 0u;
          run.s1 = run.lo = run.hi = 0ull;
          run.mn = ~(KT)0;
          run.mx = (KT)0;
        }
        const KT k = ZnKey<VT>::of(v);
        run.cnt++;
        run.s1 += (zn_u64)q;
        run.lo += q2 & 0xFFFFFFFFull;
        run.hi += q2 >> 32;
        run.mn = k < run.mn ? k : run.mn;
        run.mx = k > run.mx ? k : run.mx;
      }
    }
  }
  zn_flush_run(run, a.want, s_c, s_s1, s_lo, s_hi, s_mn, s_mx, g);
  if (bad_q) atomicOr(status, DT_STATUS_BAD_HEIGHT);
  if (bad_z) atomicOr(status, DT_STATUS_ZONE_RANGE);
  __syncthreads();
  // one global add per entry: the copies of a direct table are summed here
  const int entries = a.direct ? (int)a.Z : S, copies = a.direct ? a.rep : 1;
  for (int e = threadIdx.x; e < entries; e += 256) {
    uint32_t c = 0u;
    zn_u64 t = 0ull, lo = 0ull, hi = 0ull;
    KT mn = ~(KT)0, mx = (KT)0;
    for (int r = 0; r < copies; r++) {
      const int i = e + r * entries;
      c += s_c[i];
      t += s_s1[i];
      lo += s_lo[i];
      hi += s_hi[i];
      mn = s_mn[i] < mn ? s_mn[i] : mn;
      mx = s_mx[i] > mx ? s_mx[i] : mx;
    }
    if (c == 0u) continue;
    const int64_t z = a.direct ? e : s_key[e];
    if (a.want & ZN_COUNT) atomicAdd(&g.cnt[z], (zn_u64)c);
    if ((a.want & ZN_S1) && t) atomicAdd(&g.s1[z], t);
    if (a.want & ZN_S2) {
      if (lo) atomicAdd(&g.lo[z], lo);
      if (hi) atomicAdd(&g.hi[z], hi);
    }
    if (a.want & ZN_MIN) atomicMin(&g.mn[z], mn);
    if (a.want & ZN_MAX) atomicMax(&g.mx[z], mx);
  }
}

// min / max keys back to the bits of their values, in place (the key and the value have one size); an untouched key
// is an empty zone: NaN
template <typename VT>
__global__ __launch_bounds__(256) void k_zn_keys(typename ZnKey<VT>::T *mn, typename ZnKey<VT>::T *mx, int64_t Z) {
  typedef typename ZnKey<VT>::T KT;
  const int64_t z = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (z >= Z) return;
  if (mn) {
    const KT k = mn[z];
    mn[z] = k == ~(KT)0 ? ZnKey<VT>::nan_bits() : ZnKey<VT>::bits(k);
  }
  if (mx) {
    const KT k = mx[z];
    mx[z] = k == (KT)0 ? ZnKey<VT>::nan_bits() : ZnKey<VT>::bits(k);
  }
}

// The LDS table of a launch: direct for few zones, claimed slots otherwise; `slots` is DT_DBG_RC_SLOTS.  A direct
// table of few zones is kept in up to ZN_COPIES copies, a lane adding to copy lane % copies: with ten zones every lane
// of the workgroup would otherwise queue on ten words.
static void zn_table_mode(int64_t Z, int direct_max, int claimed, int slots, int *S, int *direct, int *rep) {
  *rep = 1;
  *direct = 0;
  if (slots < 0) {
    *S = 0;
    return;
  }
  const int cap = slots > 0 ? slots : 0x7FFFFFFF;
  if (Z <= direct_max && Z <= cap) {
    const int room = (direct_max < cap ? direct_max : cap) / (int)Z;
    *rep = room > ZN_COPIES ? ZN_COPIES : room;
    *S = (int)Z * *rep;
    *direct = 1;
    return;
  }
  *S = claimed < cap ? claimed : cap;
}

// a workgroup per tile; with a direct table at most ZN_DIRECT_GRID workgroups, each taking tile after tile, so that a
// zone's global word is added to ZN_DIRECT_GRID times and not once per tile (ten zones, 65536 tiles: the flush alone
// took as long as two copies of the rasters)
static unsigned zn_grid(unsigned tiles, int direct) {
  return direct && tiles > ZN_DIRECT_GRID ? ZN_DIRECT_GRID : tiles;
}

template <typename VT>
static void zn_launch_tables(hipStream_t s, const int32_t *zones, const VT *values, const ZnTablesArgs &a, bool vec,
                             int64_t *count, int64_t *s1, uint64_t *s2_lo, uint64_t *s2_hi, void *vmin, void *vmax,
                             int *status) {
  typedef typename ZnKey<VT>::T KT;
  ZnTables<KT> g = {(zn_u64 *)count, (zn_u64 *)s1, (zn_u64 *)s2_lo, (zn_u64 *)s2_hi, (KT *)vmin, (KT *)vmax};
  const size_t lds = (size_t)a.S * (24 + 2 * sizeof(KT) + 8);
  const int64_t tiles = a.tiles;
  dim3 grid(zn_grid(a.tiles, a.direct)), b(256);
  if (tiles == 0) {
    // no cell takes part: the keys still become NaN below
  } else if (vec) {
    hipLaunchKernelGGL((k_zn_tables<VT, true>), grid, b, lds, s, zones, values, a, g, status);
  } else {
    hipLaunchKernelGGL((k_zn_tables<VT, false>), grid, b, lds, s, zones, values, a, g, status);
  }
  if (vmin || vmax)
    hipLaunchKernelGGL(k_zn_keys<VT>, dim3((unsigned)((a.Z + 255) / 256)), b, 0, s, (KT *)vmin, (KT *)vmax, a.Z);
}

int dt_launch_zonal_tables(hipStream_t s, const int32_t *zones, const void *values, int value_bytes, int64_t H,
                           int64_t W, int64_t n_zones, double origin, int frac_bits, int has_nodata, double nodata,
                           int64_t *count, int64_t *s1, uint64_t *s2_lo, uint64_t *s2_hi, void *vmin, void *vmax,
                           int *status, int slots) {
  if (n_zones == 0) return DT_OK;
  const size_t zb = (size_t)n_zones * 8, kb = (size_t)n_zones * (size_t)value_bytes;
  if (count) DT_HIP(hipMemsetAsync(count, 0, zb, s));
  if (s1) DT_HIP(hipMemsetAsync(s1, 0, zb, s));
  if (s2_lo) DT_HIP(hipMemsetAsync(s2_lo, 0, zb, s));
  if (s2_hi) DT_HIP(hipMemsetAsync(s2_hi, 0, zb, s));
  if (vmin) DT_HIP(hipMemsetAsync(vmin, 0xFF, kb, s));
  if (vmax) DT_HIP(hipMemsetAsync(vmax, 0, kb, s));
  ZnTablesArgs a;
  a.H = H; a.W = W; a.Z = n_zones; a.sbits = frac_bits; a.has_nodata = has_nodata; a.origin = origin;
  a.nodata = nodata;
  a.want = (count ? ZN_COUNT : 0) | (s1 ? ZN_S1 : 0) | (s2_lo ? ZN_S2 : 0) | (vmin ? ZN_MIN : 0) | (vmax ? ZN_MAX : 0);
  zn_table_mode(n_zones, ZN_DIRECT_MAX, ZN_SLOTS, slots, &a.S, &a.direct, &a.rep);
  a.tiles = (unsigned)(((H + ZN_TH - 1) / ZN_TH) * ((W + ZN_TW - 1) / ZN_TW));
  const bool vec = (W & 3) == 0 && ((uintptr_t)zones & 15u) == 0 && ((uintptr_t)values & 15u) == 0;
  if (value_bytes == 4)
    zn_launch_tables<float>(s, zones, (const float *)values, a, vec, count, s1, s2_lo, s2_hi, vmin, vmax, status);
  else
    zn_launch_tables<double>(s, zones, (const double *)values, a, vec, count, s1, s2_lo, s2_hi, vmin, vmax, status);
  return DT_OK;
}

// ---- counts: per-zone histogram (VT float / double) and cross-tabulation (VT int32_t) ------------------------------------
struct ZnCountsArgs {
  int64_t H, W, Z;
  unsigned tiles;
  int K, S, direct, rep, has_nodata;
  double nodata;
};

__device__ __forceinline__ void zn_flush_count(long long key, uint32_t cnt, uint32_t *s_c, zn_u64 *counts) {
  if (cnt == 0u) return;
  if (key >= 0) atomicAdd(&s_c[key], cnt);
  else atomicAdd(&counts[~key], (zn_u64)cnt);
}

template <typename VT, bool VEC>
__global__ __launch_bounds__(256) void k_zn_counts(const int32_t *__restrict__ zones, const VT *__restrict__ values,
                                                   const double *__restrict__ edges, ZnCountsArgs a, zn_u64 *counts,
                                                   int *status) {
  constexpr bool XT = std::is_same<VT, int32_t>::value;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int K = a.K, SK = a.S * a.K, NE = XT ? 0 : K + 1;
  double *s_e = reinterpret_cast<double *>(s_raw);
  uint32_t *s_c = reinterpret_cast<uint32_t *>(s_e + NE);
  int *s_key = reinterpret_cast<int *>(s_c + SK);
  for (int i = threadIdx.x; i < NE; i += 256) s_e[i] = edges[i];
  for (int i = threadIdx.x; i < SK; i += 256) s_c[i] = 0u;
  for (int i = threadIdx.x; i < a.S; i += 256) s_key[i] = -1;
  __syncthreads();

  const unsigned tiles_x = (unsigned)((a.W + ZN_TW - 1) / ZN_TW);
  long long run_key = 0;
  uint32_t run_cnt = 0u;
  const int copy0 = a.direct ? (int)(threadIdx.x % (unsigned)a.rep) * (int)a.Z : 0;
  int last_z = -1, last_slot = -1;
  bool bad_z = false;
  for (unsigned tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // as in k_zn_tables
    const unsigned ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int64_t x = (int64_t)tx * ZN_TW + (int64_t)(threadIdx.x & 15u) * 4;
    const int64_t yb = (int64_t)ty * ZN_TH + (int64_t)(threadIdx.x >> 4);
#pragma unroll
    for (int j = 0; j < ZN_TH / 16; j++) {
      const int64_t y = yb + 16 * j;
      if (y >= a.H || x >= a.W) continue;
      const int64_t f = y * a.W + x;
      int32_t zz[4];
      VT vv[4];
      if (VEC) {
        zn_load4(zones, f, zz);
        zn_load4(values, f, vv);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const bool in = x + i < a.W;
          zz[i] = in ? zones[f + i] : ZN_NONE;
          vv[i] = in ? values[f + i] : (VT)0;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int z = zz[i];
        if (z < 0) continue;
        if (z >= a.Z) {
          bad_z = true;
          continue;
        }
        int col;
        if (XT) {
          col = (int)vv[i];
          if (col < 0) continue;
          if (col >= K) {
            bad_z = true;
            continue;
          }
        } else {
          const double d = (double)vv[i];
          if (!(fabs(d) < INFINITY)) continue;
          if (a.has_nodata && d == a.nodata) continue;
          if (d < s_e[0] || d > s_e[K]) continue;
          int lo = 0, hi = K;  // the largest k with edges[k] <= d; the last edge closes the last bin
          while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_e[mid] <= d) lo = mid;
            else hi = mid - 1;
          }
          col = lo < K ? lo : K - 1;
        }
        if (z != last_z) {
          last_z = z;
          last_slot = a.direct ? copy0 + z : dt_claim_slot(s_key, a.S, z);
        }
        const long long key = last_slot >= 0 ? (long long)last_slot * K + col : ~((long long)z * K + col);
        if (key != run_key) {
          zn_flush_count(run_key, run_cnt, s_c, counts);
          run_key = key;
          run_cnt = 0u;
        }
        run_cnt++;
      }
    }
  }
  zn_flush_count(run_key, run_cnt, s_c, counts);
  if (bad_z) atomicOr(status, DT_STATUS_ZONE_RANGE);
  __syncthreads();
  const int entries = a.direct ? (int)a.Z * K : SK, copies = a.direct ? a.rep : 1;
  for (int e = threadIdx.x; e < entries; e += 256) {
    uint32_t c = 0u;
    for (int r = 0; r < copies; r++) c += s_c[e + r * entries];
    if (c == 0u) continue;
    const int slot = e / K;
    const long long z = a.direct ? slot : s_key[slot];
    atomicAdd(&counts[z * K + (e - slot * K)], (zn_u64)c);
  }
}

size_t dt_zonal_counts_scratch(int K) { return dt_align256((size_t)(K + 1) * sizeof(double)); }

template <typename VT>
static void zn_launch_counts(hipStream_t s, const int32_t *zones, const VT *values, const double *edges,
                             const ZnCountsArgs &a, bool vec, int64_t *counts, int *status) {
  const bool xt = std::is_same<VT, int32_t>::value;
  const size_t lds = (xt ? 0 : (size_t)(a.K + 1) * 8) + (size_t)a.S * a.K * 4 + (size_t)a.S * 4;
  dim3 grid(zn_grid(a.tiles, a.direct)), b(256);
  if (vec) hipLaunchKernelGGL((k_zn_counts<VT, true>), grid, b, lds, s, zones, values, edges, a, (zn_u64 *)counts, status);
  else hipLaunchKernelGGL((k_zn_counts<VT, false>), grid, b, lds, s, zones, values, edges, a, (zn_u64 *)counts, status);
}

int dt_launch_zonal_counts(hipStream_t s, const int32_t *zones, const void *values, int value_bytes, int64_t H,
                           int64_t W, int64_t n_zones, const double *edges_host, int K, int has_nodata, double nodata,
                           void *scratch, size_t scratch_bytes, int64_t *counts, int *status, int slots) {
  if (n_zones == 0) return DT_OK;
  DT_HIP(hipMemsetAsync(counts, 0, (size_t)n_zones * (size_t)K * 8, s));
  if (H * W == 0) return DT_OK;
  double *d_e = nullptr;
  if (value_bytes != 0) {
    DT_REQUIRE(scratch_bytes >= dt_zonal_counts_scratch(K), "scratch too small");
    d_e = (double *)scratch;
    dt_launch_host_doubles(s, edges_host, K + 1, d_e);
  }
  ZnCountsArgs a;
  a.H = H; a.W = W; a.Z = n_zones; a.K = K; a.has_nodata = has_nodata; a.nodata = nodata;
  int claimed = ZN_COUNTS_TABLE_BYTES / (4 * K);
  claimed = claimed > ZN_COUNTS_SLOTS_MAX ? ZN_COUNTS_SLOTS_MAX : (claimed < 1 ? 1 : claimed);
  zn_table_mode(n_zones, ZN_COUNTS_TABLE_BYTES / (4 * K), claimed, slots, &a.S, &a.direct, &a.rep);
  a.tiles = (unsigned)(((H + ZN_TH - 1) / ZN_TH) * ((W + ZN_TW - 1) / ZN_TW));
  const bool vec = (W & 3) == 0 && ((uintptr_t)zones & 15u) == 0 && ((uintptr_t)values & 15u) == 0;
  if (value_bytes == 0) zn_launch_counts<int32_t>(s, zones, (const int32_t *)values, d_e, a, vec, counts, status);
  else if (value_bytes == 4) zn_launch_counts<float>(s, zones, (const float *)values, d_e, a, vec, counts, status);
  else zn_launch_counts<double>(s, zones, (const double *)values, d_e, a, vec, counts, status);
  return DT_OK;
}

// ---- paint -----------------------------------------------------------------------------------------------------------
template <typename WT>
__device__ __forceinline__ WT zn_pick(const WT *__restrict__ table, int64_t T, int32_t z, WT fill) {
  return (z >= 0 && z < T) ? table[z] : fill;
}

template <typename WT, bool VEC>
__global__ __launch_bounds__(256) void k_zn_paint(const WT *__restrict__ table, int64_t T,
                                                  const int32_t *__restrict__ zones, int64_t N, WT fill,
                                                  WT *__restrict__ out) {
  const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (f >= N) return;
  if (VEC && f + 4 <= N) {
    const int4 z = *reinterpret_cast<const int4 *>(zones + f);
    const WT o0 = zn_pick(table, T, z.x, fill), o1 = zn_pick(table, T, z.y, fill);
    const WT o2 = zn_pick(table, T, z.z, fill), o3 = zn_pick(table, T, z.w, fill);
    if (sizeof(WT) == 4) {
      *reinterpret_cast<uint4 *>(out + f) = make_uint4((uint32_t)o0, (uint32_t)o1, (uint32_t)o2, (uint32_t)o3);
    } else {
      *reinterpret_cast<ulonglong2 *>(out + f) = make_ulonglong2((zn_u64)o0, (zn_u64)o1);
      *reinterpret_cast<ulonglong2 *>(out + f + 2) = make_ulonglong2((zn_u64)o2, (zn_u64)o3);
    }
    return;
  }
  for (int i = 0; i < 4 && f + i < N; i++) out[f + i] = zn_pick(table, T, zones[f + i], fill);
}

int dt_launch_zonal_paint(hipStream_t s, const void *table, int elem_bytes, int64_t n_table, const int32_t *zones,
                          int64_t N, uint64_t fill_bits, void *out) {
  if (N == 0) return DT_OK;
  const bool vec = ((uintptr_t)zones & 15u) == 0 && ((uintptr_t)out & 15u) == 0;
  dim3 g((unsigned)((N + 1023) / 1024)), b(256);
  if (elem_bytes == 4) {
    const uint32_t fill = (uint32_t)fill_bits;
    if (vec) hipLaunchKernelGGL((k_zn_paint<uint32_t, true>), g, b, 0, s, (const uint32_t *)table, n_table, zones, N, fill, (uint32_t *)out);
    else hipLaunchKernelGGL((k_zn_paint<uint32_t, false>), g, b, 0, s, (const uint32_t *)table, n_table, zones, N, fill, (uint32_t *)out);
  } else {
    const zn_u64 fill = (zn_u64)fill_bits;
    if (vec) hipLaunchKernelGGL((k_zn_paint<zn_u64, true>), g, b, 0, s, (const zn_u64 *)table, n_table, zones, N, fill, (zn_u64 *)out);
    else hipLaunchKernelGGL((k_zn_paint<zn_u64, false>), g, b, 0, s, (const zn_u64 *)table, n_table, zones, N, fill, (zn_u64 *)out);
  }
  return DT_OK;
}
