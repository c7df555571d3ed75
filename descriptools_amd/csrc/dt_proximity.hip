// dt_proximity.hip -- exact Euclidean nearest-river distance and allocation (net-new; descriptools_amd/proximity.py
// holds the definition).  Integer arithmetic throughout: squared distances in cells, int64.
//
// A source is a cell with river == 1 that is not nodata (nod <= -100).  nearest(c) is the source of smallest
// d2 = dy^2 + dx^2, among equals the one of smallest flat index.  Two separable passes:
//
// Row pass: cx(y, x) = the column of the nearest source in row y, the left one of two equally far, -1 when the row has
// none.  A row is cut into segments of 64 cells, one wave each.
//   k_px_mark   one ballot per segment: the segment's source bits and its first and last source column.
//   k_px_carry  one wave per row scans the segment summaries, 64 at a time with a carry: `last` becomes the last
//               source column to the left of the segment, `first` the first one to its right (the carries across
//               segments; W / 64 steps of work per row whatever the row holds).
//   k_px_row    per cell: the nearest set bit at or left of the lane and at or right of it, the carries where the
//               segment has none on that side, the left one on a tie.
// Column pass (k_px_col): in column x, f(y') = (x - cx(y', x))^2, or 2^62 when row y' has no source, and a(y) = the
// smallest y' that minimises (y - y')^2 + f(y').  The cost matrix is Monge (the cross term -2 y y'), so a is
// non-decreasing in y, and it is solved by divide and conquer, one launch per level: with the virtual rows -1 and H
// (a = 0 and H - 1) the boundaries of level k are B_k(j) = (j (H + 1) >> k) - 1, node j solves the row
// r = B_(k+1)(2 j + 1) strictly between B_k(j) and B_k(j + 1) by scanning the candidate rows a(B_k(j)) .. a(B_k(j + 1))
// only.  The candidates of a level are at most H + 2^k per column and the levels ceil(log2(H + 1)), whatever the
// sources: ~log2 H + 1 evaluations per cell.  Lanes are adjacent columns (reads of cx coalesce, and neighbouring
// columns scan neighbouring rows); a block is 64 columns x 16 nodes.  A node with a short candidate range is scanned
// lane by lane; a long one (all of them at the coarse levels, at the fine levels the nodes across which a(y) jumps) by
// the whole block, each lane's range cut into 16 parts that are combined through LDS (smallest cost, then smallest
// part: the parts are in ascending y').  The solving lane holds d2 and a, so it writes the outputs at once: indices =
// a W + cx(a, x), distance = float32(px * sqrt(float64(d2))) with the float64 sqrt correctly rounded (as dt_dinf.hip
// relies on), -100 where d2 reaches 2^62 (no source at all) or the cell is nodata.  Nodata is not a barrier: such a
// cell still gets its a, which the levels below read.
// The smallest flat index among the nearest sources lies in the smallest minimising row and is that row's own
// nearest source, left on ties: "left" in the row pass and "smallest y'" in the column pass are the tie rule.
// No launch depends on what an earlier one found: the launcher never synchronises.
#include <cmath>

#include "dt_kernels.h"

#define PX_SENT (1ll << 62)  // f of a row without a source; + dy^2 < 2^62 still fits int64
#define PX_NODES 16          // nodes (waves) per block of k_px_col, and the parts a long range is scanned in
#define PX_SHORT 64          // a wave scans lane by lane while its longest candidate range has at most this many rows

// rows of 64-cell segments; segment g = y * nseg + s covers columns 64 s .. 64 s + 63 of row y
struct PxLayout {
  unsigned long long *bits;  // per segment: bit l = cell 64 s + l is a source
  int32_t *first, *last;     // per segment: its first / last source column, then (k_px_carry) the first to its right /
                             // the last to its left; -1 = none
  int32_t *cx;               // per cell: the row pass's result
  int32_t *a;                // per cell: the column pass's minimising row
  int64_t nseg;
  size_t bytes;
};
static PxLayout px_layout(int64_t H, int64_t W, void *scratch) {
  PxLayout L = {};
  DtCarver c(scratch);
  L.nseg = (W + 63) / 64;
  const size_t segs = (size_t)(H * L.nseg), n = (size_t)(H * W);
  L.bits = c.take<unsigned long long>(segs);
  L.first = c.take<int32_t>(segs);
  L.last = c.take<int32_t>(segs);
  L.cx = c.take<int32_t>(n);
  L.a = c.take<int32_t>(n);
  L.bytes = c.bytes();
  return L;
}
size_t dt_proximity_scratch(int64_t H, int64_t W) { return px_layout(H, W, nullptr).bytes; }

// one wave per segment (blocks of 4 waves)
__global__ __launch_bounds__(256) void k_px_mark(const int8_t *__restrict__ river, const float *__restrict__ nod, int W,
                                                 int64_t nseg, int64_t segs, unsigned long long *__restrict__ bits,
                                                 int32_t *__restrict__ first, int32_t *__restrict__ last) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= segs) return;  // wave-uniform
  const int64_t y = g / nseg;
  const int x0 = (int)(g - y * nseg) * 64, x = x0 + lane;
  bool src = false;
  if (x < W) {
    const int64_t i = y * W + x;
    src = river[i] == 1 && !(nod && nod[i] <= DT_NODATA);
  }
  const unsigned long long m = __ballot(src);
  if (lane == 0) {
    bits[g] = m;
    first[g] = m ? x0 + (int)__builtin_ctzll(m) : -1;
    last[g] = m ? x0 + 63 - (int)__builtin_clzll(m) : -1;
  }
}

// one wave per row: an exclusive running max of `last` from the left, an exclusive running min of `first` from the right
__global__ __launch_bounds__(256) void k_px_carry(int64_t H, int64_t nseg, int32_t *__restrict__ first,
                                                  int32_t *__restrict__ last) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t y = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= H) return;  // wave-uniform
  int32_t *fr = first + y * nseg, *lr = last + y * nseg;
  int carry = -1;
  for (int64_t c0 = 0; c0 < nseg; c0 += 64) {
    const int64_t i = c0 + lane;
    int v = i < nseg ? lr[i] : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v = max(v, t);
    }
    int before = __shfl_up(v, 1);
    before = lane == 0 ? carry : max(before, carry);
    if (i < nseg) lr[i] = before;
    carry = max(carry, __shfl(v, 63));
  }
  const int none = 0x7fffffff;
  carry = none;
  for (int64_t c0 = (nseg - 1) / 64 * 64; c0 >= 0; c0 -= 64) {
    const int64_t i = c0 + lane;
    int v = i < nseg ? fr[i] : -1;
    v = v < 0 ? none : v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(v, o);
      if (lane + o < 64) v = min(v, t);
    }
    int after = __shfl_down(v, 1);
    after = lane == 63 ? carry : min(after, carry);
    if (i < nseg) fr[i] = after == none ? -1 : after;
    carry = min(carry, __shfl(v, 0));
  }
}

__global__ __launch_bounds__(256) void k_px_row(int W, int64_t nseg, int64_t segs,
                                                const unsigned long long *__restrict__ bits,
                                                const int32_t *__restrict__ first, const int32_t *__restrict__ last,
                                                int32_t *__restrict__ cx) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= segs) return;
  const int64_t y = g / nseg;
  const int x0 = (int)(g - y * nseg) * 64, x = x0 + lane;
  if (x >= W) return;
  const unsigned long long m = bits[g];
  const unsigned long long lm = m & (~0ull >> (63 - lane)), rm = m >> lane;
  const int left = lm ? x0 + 63 - (int)__builtin_clzll(lm) : last[g];
  const int right = rm ? x + (int)__builtin_ctzll(rm) : first[g];
  int c;
  if (left < 0) c = right;
  else if (right < 0) c = left;
  else c = x - left <= right - x ? left : right;
  cx[y * W + x] = c;
}

// the candidates y0 .. y1 - 1 of column x for row r, ascending; strict <: the smallest y' of equals
__device__ __forceinline__ void px_scan(const int32_t *__restrict__ cx, int W, int x, int64_t r, int64_t y0, int64_t y1,
                                        int64_t &best, int &brow) {
#pragma unroll 4
  for (int64_t yc = y0; yc < y1; yc++) {
    const int c = cx[yc * W + x];
    const int64_t dx = x - c, dy = r - yc;
    const int64_t cost = dy * dy + (c < 0 ? PX_SENT : dx * dx);
    if (cost < best) {
      best = cost;
      brow = (int)yc;
    }
  }
}

// level k of the column pass: a block is 64 columns x PX_NODES nodes, one wave per node.  A wave whose longest
// candidate range is at most PX_SHORT rows scans it lane by lane.  The others (every node of the coarse levels; at the
// fine levels the few nodes across which `a` jumps: the ranges of a level add up to H + 2^k, but one node may hold
// most of that) leave their ranges in LDS, and the whole block scans them, one node after the other, in PX_NODES parts
// per lane combined through LDS: smallest cost, then smallest part (the parts are in ascending y').
__global__ __launch_bounds__(64 * PX_NODES) void k_px_col(const int32_t *__restrict__ cx, const float *__restrict__ nod,
                                                          int H, int W, int k, int xtiles, double px,
                                                          int32_t *__restrict__ a, float *__restrict__ distance,
                                                          int64_t *__restrict__ indices) {
  __shared__ int64_t s_cost[PX_NODES][64];
  __shared__ int32_t s_row[PX_NODES][64], s_lo[PX_NODES][64], s_len[PX_NODES][64];
  __shared__ int s_long[PX_NODES];
  const int lane = (int)threadIdx.x, q = (int)threadIdx.y;
  const int64_t by = blockIdx.x / (unsigned)xtiles;
  const int x = (int)(blockIdx.x - by * xtiles) * 64 + lane;
  const int64_t H1 = (int64_t)H + 1, j = by * PX_NODES + q;
  // the node's row and its enclosing boundaries; rows -1 and H are virtual
  const int64_t lo = ((j * H1) >> k) - 1, hi = (((j + 1) * H1) >> k) - 1, r = (((2 * j + 1) * H1) >> (k + 1)) - 1;
  const bool live = x < W && j < (1ll << k) && r > lo && r < hi;  // r == lo or hi: solved at a level above
  int clo = 0, len = 0;
  if (live) {
    clo = lo < 0 ? 0 : a[lo * W + x];
    len = (hi >= H ? H - 1 : a[hi * W + x]) - clo + 1;
  }
  const bool lng = __any(len > PX_SHORT) != 0;  // the same in every lane of the wave
  if (lane == 0) s_long[q] = lng;
  int64_t best = 0x7fffffffffffffffll;
  int brow = 0;
  if (lng) {
    s_lo[q][lane] = clo;
    s_len[q][lane] = len;
  } else {
    px_scan(cx, W, x, r, clo, (int64_t)clo + len, best, brow);
  }
  __syncthreads();
  for (int t = 0; t < PX_NODES; t++) {
    if (!s_long[t]) continue;  // the same in every thread of the block
    const int64_t rt = (((2 * (by * PX_NODES + t) + 1) * H1) >> (k + 1)) - 1;
    const int64_t l0 = s_lo[t][lane], ln = s_len[t][lane];
    int64_t cost = 0x7fffffffffffffffll;
    int row = 0;
    px_scan(cx, W, x, rt, l0 + ln * q / PX_NODES, l0 + ln * (q + 1) / PX_NODES, cost, row);
    s_cost[q][lane] = cost;
    s_row[q][lane] = row;
    __syncthreads();
    if (q == t) {
      for (int u = 0; u < PX_NODES; u++)
        if (s_cost[u][lane] < best) {
          best = s_cost[u][lane];
          brow = s_row[u][lane];
        }
    }
    __syncthreads();
  }
  if (!live) return;
  const int64_t i = r * W + x;
  a[i] = brow;
  if (best >= PX_SENT || (nod && nod[i] <= DT_NODATA)) {
    distance[i] = DT_NODATA;
    indices[i] = -100;
  } else {
    distance[i] = (float)(px * sqrt((double)best));
    indices[i] = (int64_t)brow * W + cx[(int64_t)brow * W + x];
  }
}

int dt_launch_proximity(hipStream_t s, const int8_t *river, const float *nod, int64_t H, int64_t W, double px,
                        void *scratch, size_t scratch_bytes, float *distance, int64_t *indices) {
  if (H == 0 || W == 0) return DT_OK;
  const PxLayout L = px_layout(H, W, scratch);
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  const int64_t segs = H * L.nseg;
  const unsigned gseg = (unsigned)((segs + 3) / 4);
  hipLaunchKernelGGL(k_px_mark, dim3(gseg), dim3(256), 0, s, river, nod, (int)W, L.nseg, segs, L.bits, L.first, L.last);
  hipLaunchKernelGGL(k_px_carry, dim3((unsigned)((H + 3) / 4)), dim3(256), 0, s, H, L.nseg, L.first, L.last);
  hipLaunchKernelGGL(k_px_row, dim3(gseg), dim3(256), 0, s, (int)W, L.nseg, segs, L.bits, L.first, L.last, L.cx);
  const int64_t xtiles = (W + 63) / 64;
  for (int k = 0; (1ll << k) < H + 1; k++) {
    const int64_t groups = ((1ll << k) + PX_NODES - 1) / PX_NODES;
    hipLaunchKernelGGL(k_px_col, dim3((unsigned)(xtiles * groups)), dim3(64, PX_NODES), 0, s, L.cx, nod, (int)H, (int)W,
                       k, (int)xtiles, px, L.a, distance, indices);
  }
  return DT_OK;
}
