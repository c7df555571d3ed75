// dt_streams.hip -- Strahler order, Shreve magnitude and stream links of a D8 channel network (net-new).
//
// The network is the set of cells with river != 0; c -> d is an edge when c's D8 code points at an in-raster network
// cell d.  The op works on a compacted list of the network cells (a few percent of the raster at the chain's
// threshold), in ten launches plus the pointer-doubling rounds:
//   so_info     full raster, 2048 cells per block: child count and single-child direction per cell (info byte) from
//               fdr / river rows staged in LDS with a one-cell halo; network cells per block
//   so_scan     three launches (dt_launch_count_scan, shared with dt_reaches.hip): exclusive scan of the block
//               counts -> compact id of each block's first network cell, M
//   so_compact  full raster: compact id of each network cell (block scan again); pos, map, cinfo
//   so_links    compact: down pointer (flagged when it enters a confluence), link pointer J (the single child, or
//               ~self at a head), countdown word initialised
//   so_jump     compact, ceil(log2 N) + 1 rounds: in-place pointer doubling of J to ~head; a round whose
//               predecessor left nothing unresolved returns at once
//   so_tails    compact: the tail of each link names its parent junction (jpar[head])
//   so_count    compact, from every source: the junction countdown on one 64-bit word per junction
//   so_scatter  full raster: strahler / shreve / link through each cell's head, 8 cells per thread, 16-B stores
//
// Countdown word (one per compact cell, meaningful at heads):
//   bits 0-31 Shreve sum | 32-37 largest child order m | 38 tie (two children of order m) | 40-43 pending children
// A junction starts at (pending = child count); each arrival folds (order, magnitude) into it with a compare-and-swap
// whose expected value is the previous return, so every arrival sees and extends the whole state in one word.  The
// arrival that takes pending from 1 to 0 holds the full fold in the value its CAS wrote: order = m + tie, magnitude =
// the sum, and it carries them to the junction below.  It reads nothing else that another workgroup writes in this
// launch (jpar is written by so_tails), so no fence is needed (cdna_hip_programming.md Guideline 16; the same
// hand-off as k_faw_reduce).  A source's word is written final by so_links (m = 1, sum = 1, pending 0).  A junction
// on a D8 cycle never reaches pending 0: its link's cells come out as -100.
#include "dt_kernels.h"

#define SO_SEG (DT_SCAN_CHUNK + 2)  // a staged row segment: the chunk's cells and one halo cell on each side
#define SO_NET 0x80u                // info byte: network cell | child count (bits 0-3) | single child's dir (4-6)
#define SO_TAIL_J 0x80000000u       // down word: the downstream cell is a confluence (its link ends here)
#define SO_NONE 0xFFFFFFFFu         // down word: network outlet
#define SO_PEND_SH 40
#define SO_M_SH 32
#define SO_TIE (1ull << 38)
#define SO_SUM_MASK 0xFFFFFFFFull

__device__ __forceinline__ uint32_t so_net_count(uint2 v) {
  return (uint32_t)__popc(v.x & 0x80808080u) + (uint32_t)__popc(v.y & 0x80808080u);
}

// ---- so_info ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_so_info(const uint8_t *__restrict__ fdr, const int8_t *__restrict__ river,
                                                 int64_t H, int64_t W, uint8_t *__restrict__ info,
                                                 uint32_t *__restrict__ bcount) {
  __shared__ uint8_t s_f[3][SO_SEG + 2];
  __shared__ uint8_t s_r[3][SO_SEG + 2];
  __shared__ uint32_t s_w[4];
  const int64_t N = H * W;
  const int64_t base = (int64_t)blockIdx.x * DT_SCAN_CHUNK;
  for (int r = 0; r < 3; r++) {
    const int64_t st = base + (int64_t)(r - 1) * W - 1;
    for (int i = threadIdx.x; i < SO_SEG; i += 256) {
      const int64_t g = st + i;
      const bool in = g >= 0 && g < N;
      s_f[r][i] = in ? fdr[g] : (uint8_t)0;
      s_r[r][i] = in ? (uint8_t)(river[g] != 0) : (uint8_t)0;
    }
  }
  __syncthreads();
  const int l0 = (int)threadIdx.x * DT_SCAN_CPT;
  const int64_t f0 = base + l0;
  int64_t x = f0 % W;
  uint32_t word[2] = {0u, 0u}, cnt_net = 0;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    const int li = l0 + k + 1;
    uint32_t b = 0;
    if (f0 + k < N && s_r[1][li]) {
      uint32_t cnt = 0, dir = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        int dy, dx;
        dt_nb_delta(i, dy, dx);
        const bool xin = x + dx >= 0 && x + dx < W;
        if (xin && s_r[dy + 1][li + dx] && s_f[dy + 1][li + dx] == dt_nb_back_code(i)) {
          cnt++;
          dir = (uint32_t)i;
        }
      }
      b = SO_NET | cnt | (cnt == 1u ? dir << 4 : 0u);
      cnt_net++;
    }
    word[k >> 2] |= b << (8 * (k & 3));
    if (++x == W) x = 0;
  }
  *reinterpret_cast<uint2 *>(info + f0) = make_uint2(word[0], word[1]);
  uint32_t total;
  dt_block_scan_256(cnt_net, s_w, &total);
  if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

// ---- so_scan ---------------------------------------------------------------------------------------------------------
// Exclusive scan of the per-block counts in three steps (dt_launch_count_scan): so_gsum sums groups of DT_SCAN_CHUNK
// counts, so_gscan (one block) scans the group sums, so_expand scans each group again from its group's offset.
// offsets[b] = the counts before block b (here: network cells); meta[0] = the total (M).
__global__ __launch_bounds__(256) void k_so_gsum(const uint32_t *__restrict__ bcount, int64_t nblk,
                                                 uint32_t *__restrict__ gsum) {
  __shared__ uint32_t s_w[4];
  const int64_t b0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) v += b0 + k < nblk ? bcount[b0 + k] : 0u;
  uint32_t total;
  dt_block_scan_256(v, s_w, &total);
  if (threadIdx.x == 0) gsum[blockIdx.x] = total;
}

// one block; thread t owns a run of ceil(ng / 256) consecutive group sums (one each below 2^30 cells)
__global__ __launch_bounds__(256) void k_so_gscan(const uint32_t *__restrict__ gsum, int64_t ng,
                                                  int64_t *__restrict__ goff, int64_t *__restrict__ meta) {
  __shared__ int64_t s_t[256];
  const int64_t per = (ng + 255) / 256;
  const int64_t g0 = (int64_t)threadIdx.x * per;
  const int64_t g1 = g0 + per < ng ? g0 + per : ng;
  int64_t mine = 0;
  for (int64_t g = g0; g < g1; g++) mine += gsum[g];
  s_t[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // inclusive Hillis-Steele scan
    const int64_t t = threadIdx.x >= (unsigned)o ? s_t[threadIdx.x - o] : 0;
    __syncthreads();
    s_t[threadIdx.x] += t;
    __syncthreads();
  }
  int64_t run = s_t[threadIdx.x] - mine;
  for (int64_t g = g0; g < g1; g++) {
    goff[g] = run;
    run += gsum[g];
  }
  if (threadIdx.x == 255) meta[0] = s_t[255];
}

__global__ __launch_bounds__(256) void k_so_expand(const uint32_t *__restrict__ bcount, int64_t nblk,
                                                   const int64_t *__restrict__ goff, int64_t *__restrict__ offsets) {
  __shared__ uint32_t s_w[4];
  const int64_t b0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  uint32_t c[DT_SCAN_CPT], v = 0;
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    c[k] = b0 + k < nblk ? bcount[b0 + k] : 0u;
    v += c[k];
  }
  uint32_t total;
  int64_t run = goff[blockIdx.x] + dt_block_scan_256(v, s_w, &total);
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    if (b0 + k < nblk) offsets[b0 + k] = run;
    run += c[k];
  }
}

// ---- so_compact ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_so_compact(const uint8_t *__restrict__ info, const int64_t *__restrict__ offsets,
                                                    int64_t *__restrict__ pos, int32_t *__restrict__ map,
                                                    uint8_t *__restrict__ cinfo) {
  __shared__ uint32_t s_w[4];
  const int64_t f0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  const uint2 v = *reinterpret_cast<const uint2 *>(info + f0);
  uint32_t total;
  const uint32_t ex = dt_block_scan_256(so_net_count(v), s_w, &total);
  int64_t cid = offsets[blockIdx.x] + ex;
  const uint32_t w2[2] = {v.x, v.y};
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    const uint32_t b = (w2[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    if (b & SO_NET) {
      pos[cid] = f0 + k;
      map[f0 + k] = (int32_t)cid;
      cinfo[cid] = (uint8_t)b;
      cid++;
    }
  }
}

// ---- so_links --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_so_links(const uint8_t *__restrict__ fdr, int64_t H, int64_t W,
                                                  const uint8_t *__restrict__ info, const int32_t *__restrict__ map,
                                                  const int64_t *__restrict__ meta, const int64_t *__restrict__ pos,
                                                  const uint8_t *__restrict__ cinfo, uint32_t *__restrict__ down,
                                                  int32_t *__restrict__ J, unsigned long long *__restrict__ st) {
  const int64_t M = meta[0];
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < M; c += (int64_t)gridDim.x * 256) {
    const int64_t f = pos[c];
    const int64_t y = f / W, x = f - y * W;
    const uint32_t ci = cinfo[c];
    const uint32_t cnt = ci & 15u;
    const uint32_t code = fdr[f];
    uint32_t dn = SO_NONE;
    if (dt_d8_valid(code)) {
      int dy, dx;
      dt_d8_delta(code, dy, dx);
      if (y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W) {
        const int64_t g = f + dy * W + dx;
        const uint32_t gi = info[g];
        if (gi & SO_NET) dn = (uint32_t)map[g] | ((gi & 15u) != 1u ? SO_TAIL_J : 0u);
      }
    }
    down[c] = dn;
    int32_t j = ~(int32_t)c;
    if (cnt == 1u) {
      int dy, dx;
      dt_nb_delta((int)((ci >> 4) & 7u), dy, dx);
      j = map[f + dy * W + dx];
    }
    J[c] = j;
    // a source is final at once: order 1 (m = 1, no tie), magnitude 1; a junction waits for its children
    st[c] = cnt == 0u ? ((1ull << SO_M_SH) | 1ull) : ((unsigned long long)cnt << SO_PEND_SH);
  }
}

// ---- so_jump ---------------------------------------------------------------------------------------------------------
// J[c] >= 0: a cell further up c's link; J[c] < 0: ~head.  In place: a value read from a neighbour that has already
// jumped this round is still a cell of the same link, only further up.  flags[r + 1] = 1 when this round left a
// cell unresolved (round 0 always runs).
__global__ __launch_bounds__(256) void k_so_jump(const int64_t *__restrict__ meta, int32_t *J, uint32_t *flags, int r) {
  if (r > 0 && flags[r] == 0u) return;
  const int64_t M = meta[0];
  bool pend = false;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < M; c += (int64_t)gridDim.x * 256) {
    const int32_t j = J[c];
    if (j >= 0) {
      const int32_t j2 = J[j];
      J[c] = j2;
      pend |= j2 >= 0;
    }
  }
  if (__ballot(pend) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(&flags[r + 1], 1u);
}

// ---- so_tails --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_so_tails(const int64_t *__restrict__ meta, const int32_t *__restrict__ J,
                                                  const uint32_t *__restrict__ down, int32_t *__restrict__ jpar) {
  const int64_t M = meta[0];
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < M; c += (int64_t)gridDim.x * 256) {
    const int32_t j = J[c];
    const uint32_t dn = down[c];
    if (j < 0 && (dn == SO_NONE || (dn & SO_TAIL_J))) jpar[~j] = dn == SO_NONE ? -1 : (int32_t)(dn & ~SO_TAIL_J);
  }
}

// ---- so_count --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long so_fold(unsigned long long w, uint32_t o, uint32_t s) {
  const uint32_t m = (uint32_t)(w >> SO_M_SH) & 63u;
  unsigned long long r = (w & SO_SUM_MASK) + s;
  if (o > m) r |= (unsigned long long)o << SO_M_SH;
  else r |= (w & ((63ull << SO_M_SH) | SO_TIE)) | (o == m ? SO_TIE : 0ull);
  return r | ((((w >> SO_PEND_SH) & 15ull) - 1ull) << SO_PEND_SH);
}

__global__ __launch_bounds__(256) void k_so_count(const int64_t *__restrict__ meta, const uint8_t *__restrict__ cinfo,
                                                  const int32_t *__restrict__ jpar, unsigned long long *st) {
  const int64_t M = meta[0];
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < M; c += (int64_t)gridDim.x * 256) {
    if ((cinfo[c] & 15u) != 0u) continue;
    uint32_t o = 1u, s = 1u;
    int32_t p = jpar[c];
    for (int64_t it = 0; it < M && p >= 0 && p < M; it++) {
      // the first guess is the junction's initial word; every failed CAS returns the word that is there
      unsigned long long cur = (unsigned long long)(cinfo[p] & 15u) << SO_PEND_SH, nw = 0ull;
      bool done = false;
      for (int a = 0; a < 9 && !done; a++) {  // at most (children - 1) other arrivals can intervene
        nw = so_fold(cur, o, s);
        const unsigned long long seen = atomicCAS(&st[p], cur, nw);
        done = seen == cur;
        cur = seen;
      }
      if (!done || ((nw >> SO_PEND_SH) & 15ull) != 0ull) break;
      o = (uint32_t)((nw >> SO_M_SH) & 63ull) + ((nw & SO_TIE) ? 1u : 0u);
      s = (uint32_t)(nw & SO_SUM_MASK);
      p = jpar[p];
    }
  }
}

// ---- so_scatter ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void k_so_scatter(const uint8_t *__restrict__ info,
                                                    const int64_t *__restrict__ offsets, int64_t N,
                                                    const int64_t *__restrict__ pos, const int32_t *__restrict__ J,
                                                    const unsigned long long *__restrict__ st,
                                                    int8_t *__restrict__ strahler, int64_t *__restrict__ shreve,
                                                    int64_t *__restrict__ link) {
  __shared__ uint32_t s_w[4];
  const int64_t f0 = (int64_t)blockIdx.x * DT_SCAN_CHUNK + (int64_t)threadIdx.x * DT_SCAN_CPT;
  const uint2 v = *reinterpret_cast<const uint2 *>(info + f0);
  uint32_t total;
  const uint32_t ex = dt_block_scan_256(so_net_count(v), s_w, &total);
  if (f0 >= N) return;
  int64_t cid = offsets[blockIdx.x] + ex;
  const uint32_t w2[2] = {v.x, v.y};
  uint32_t so[2] = {0u, 0u};
  int64_t sh[DT_SCAN_CPT], lk[DT_SCAN_CPT];
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    const uint32_t b = (w2[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    uint32_t o = 0u;
    int64_t s = 0, l = -100;
    if (b & SO_NET) {
      const int32_t j = J[cid++];
      o = 0x9Cu;  // (int8)-100
      s = -100;
      if (j < 0) {
        const unsigned long long w = st[~j];
        if (((w >> SO_PEND_SH) & 15ull) == 0ull) {
          o = (uint32_t)((w >> SO_M_SH) & 63ull) + ((w & SO_TIE) ? 1u : 0u);
          s = (int64_t)(w & SO_SUM_MASK);
          l = pos[~j];
        }
      }
    }
    so[k >> 2] |= o << (8 * (k & 3));
    sh[k] = s;
    lk[k] = l;
  }
  if (VEC && f0 + DT_SCAN_CPT <= N) {
    *reinterpret_cast<uint2 *>(strahler + f0) = make_uint2(so[0], so[1]);
#pragma unroll
    for (int k = 0; k < DT_SCAN_CPT; k += 2) {
      if (shreve) *reinterpret_cast<longlong2 *>(shreve + f0 + k) = make_longlong2(sh[k], sh[k + 1]);
      if (link) *reinterpret_cast<longlong2 *>(link + f0 + k) = make_longlong2(lk[k], lk[k + 1]);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < DT_SCAN_CPT; k++) {
    if (f0 + k >= N) break;
    strahler[f0 + k] = (int8_t)((so[k >> 2] >> (8 * (k & 3))) & 0xFFu);
    if (shreve) shreve[f0 + k] = sh[k];
    if (link) link[f0 + k] = lk[k];
  }
}

// ---- launcher --------------------------------------------------------------------------------------------------------
struct SoLayout {
  int64_t N;
  DtCountScan scan;
  uint32_t *flags, *down;
  uint8_t *info, *cinfo;
  int32_t *map, *J;  // map: compact id per network cell; jpar once so_links has read it
  int64_t *pos;
  unsigned long long *st;
  size_t bytes;
};

static SoLayout so_layout(int64_t H, int64_t W, void *scratch) {
  SoLayout L;
  L.N = H * W;
  const size_t Np = (size_t)dt_scan_blocks(L.N) * DT_SCAN_CHUNK;
  DtCarver c(scratch);
  L.flags = c.take<uint32_t>(64);
  int64_t *meta = c.take<int64_t>(2);
  L.info = c.take<uint8_t>(Np);
  L.map = c.take<int32_t>(Np);
  L.scan = dt_count_scan_carve(c, L.N, meta);
  // compact arrays: M <= N cells (M is on the device only)
  L.pos = c.take<int64_t>((size_t)L.N);
  L.st = c.take<unsigned long long>((size_t)L.N);
  L.down = c.take<uint32_t>((size_t)L.N);
  L.J = c.take<int32_t>((size_t)L.N);
  L.cinfo = c.take<uint8_t>((size_t)L.N);
  L.bytes = c.bytes();
  return L;
}

DtCountScan dt_count_scan_carve(DtCarver &c, int64_t n, int64_t *meta) {
  DtCountScan cs;
  cs.nblk = dt_scan_blocks(n);
  cs.ng = dt_scan_blocks(cs.nblk);
  cs.meta = meta;
  cs.bcount = c.take<uint32_t>((size_t)cs.nblk);
  cs.offsets = c.take<int64_t>((size_t)cs.nblk);
  cs.gsum = c.take<uint32_t>((size_t)cs.ng);
  cs.goff = c.take<int64_t>((size_t)cs.ng);
  return cs;
}

int dt_launch_count_scan(hipStream_t s, const DtCountScan &cs, int64_t nblk) {
  DT_REQUIRE(nblk <= cs.nblk, "more block counts than the scan was carved for");
  dim3 b(256), gg((unsigned)cs.ng);
  hipLaunchKernelGGL(k_so_gsum, gg, b, 0, s, cs.bcount, nblk, cs.gsum);
  hipLaunchKernelGGL(k_so_gscan, dim3(1), b, 0, s, cs.gsum, cs.ng, cs.goff, cs.meta);
  hipLaunchKernelGGL(k_so_expand, gg, b, 0, s, cs.bcount, nblk, cs.goff, cs.offsets);
  return DT_OK;
}

size_t dt_stream_order_scratch(int64_t H, int64_t W) { return so_layout(H, W, nullptr).bytes; }

int dt_launch_stream_order(hipStream_t s, const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W, void *scratch,
                           size_t scratch_bytes, int8_t *strahler, int64_t *shreve, int64_t *link, int64_t *m_host) {
  if (H == 0 || W == 0) return DT_OK;
  SoLayout L = so_layout(H, W, scratch);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const DtCountScan &cs = L.scan;
  const int R = dt_doubling_rounds(L.N);
  DT_HIP(hipMemsetAsync(L.flags, 0, sizeof(uint32_t) * 64, s));
  dim3 b(256), gr((unsigned)cs.nblk);
  hipLaunchKernelGGL(k_so_info, gr, b, 0, s, fdr, river, H, W, L.info, cs.bcount);
  DT_TRY(dt_launch_count_scan(s, cs, cs.nblk));
  if (m_host) {
    // rasters of 2^31 cells or more: the compact ids are 31-bit, so M is checked before the compact passes
    DT_HIP(hipMemcpyAsync(m_host, cs.meta, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DT_HIP(hipStreamSynchronize(s));
    DT_REQUIRE(*m_host < (1ll << 31), "the river network has 2^31 cells or more");
  }
  hipLaunchKernelGGL(k_so_compact, gr, b, 0, s, L.info, cs.offsets, L.pos, L.map, L.cinfo);
  // compact passes: a grid that covers M <= N cells at one cell per thread up to 8 blocks per CU, strided beyond
  dim3 gc(dt_capped_grid(L.N, 2048));
  hipLaunchKernelGGL(k_so_links, gc, b, 0, s, fdr, H, W, L.info, L.map, cs.meta, L.pos, L.cinfo, L.down, L.J, L.st);
  for (int r = 0; r < R; r++) hipLaunchKernelGGL(k_so_jump, gc, b, 0, s, cs.meta, L.J, L.flags, r);
  int32_t *jpar = L.map;
  hipLaunchKernelGGL(k_so_tails, gc, b, 0, s, cs.meta, L.J, L.down, jpar);
  hipLaunchKernelGGL(k_so_count, gc, b, 0, s, cs.meta, L.cinfo, jpar, L.st);
  const bool vec = ((uintptr_t)strahler & 7u) == 0 && ((uintptr_t)shreve & 15u) == 0 && ((uintptr_t)link & 15u) == 0;
  if (vec)
    hipLaunchKernelGGL(k_so_scatter<true>, gr, b, 0, s, L.info, cs.offsets, L.N, L.pos, L.J, L.st, strahler, shreve, link);
  else
    hipLaunchKernelGGL(k_so_scatter<false>, gr, b, 0, s, L.info, cs.offsets, L.N, L.pos, L.J, L.st, strahler, shreve,
                       link);
  return DT_OK;
}
