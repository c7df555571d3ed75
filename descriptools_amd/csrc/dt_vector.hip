// dt_vector.hip -- vector rasterisation: polygons, lines and points burnt onto the grid as an int32 label raster
// (vector.py holds the definition, tests/_vector_ref.py is its reference).  Coordinates are float64 pixel-corner
// coordinates, column first; all arithmetic is float64, one rounding per operation (the library is built with
// -ffp-contract=off), in the association the definition states, and every range is clipped to the raster AS A DOUBLE
// before anything becomes an integer: a vertex may lie 10^12 cells beside the raster.  A cell holds the largest id that
// burns it (atomicMax on the label), so no order of work shows in the result.
//
// Polygons, even-odd over all rings of an id:
//   clear   the label to -1, the row counters and info to 0 (memsets)
//   count   k_vr_cross<false>: a thread per edge derives the rows [r0, r1) whose centre lines it crosses and adds 1 to
//           the row's counter; an edge of more than VR_SHORT rows is taken by its whole wave, lanes striding the rows
//   scan    k_vr_scan: one workgroup, exclusive scan of the H counters (dt_block_scan_256); total, largest row and the
//           overflow flag (total > capacity) go to info
//   emit    k_vr_cross<true>: the same traversal writes the key (id << cb) | column at the row's atomic cursor -- the
//           cursor is the row's scanned offset, so after this pass it holds the row's END
//   sort    k_vr_sort: a workgroup per row, the all-ascending bitonic network (a partner index >= n is skipped, so no
//           padding): rows of up to VR_LDS_SMALL keys in 8 KiB of LDS, rows of up to VR_LDS_LARGE keys in 64 KiB (its
//           own launch, so that the many short rows keep their occupancy), longer rows in place in global memory with
//           the same network and __syncthreads between the stages -- slow, counted in info[2], and correct
//   fill    k_vr_fill: a workgroup per row; pairs (2k, 2k+1) of the sorted row are spans; the lanes of a wave read 64
//           spans and the wave fills them one after the other, lanes striding the span: an atomic instruction then
//           covers consecutive cells.  (A lane per span of up to 32 cells took 4.7 times as long on 10^5 small polygons,
//           cells dealt evenly to the lanes by a scan and a bisection the same time: DESIGN.md 4.32.)
// Every kernel after the scan returns at once when the overflow flag is set, and the emit never writes at or past
// `capacity`: the label then stays all -1.
//
// Lines (and the rings of a polygon under all_touched): k_vr_lines, a thread per segment, the wave for a segment of
// more than VR_SHORT columns of its major axis.  Points: k_vr_points.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dt_common.h"
#include "dt_kernels.h"

namespace {

enum { VR_POLYGON = 0, VR_LINE = 1, VR_POINT = 2 };

constexpr int VR_SHORT = 8;          // rows of an edge / columns of a segment that a lane walks itself
constexpr int VR_LDS_SMALL = 1024;   // keys of a row sorted in the small LDS kernel
constexpr int VR_LDS_LARGE = 8192;   // keys of a row sorted in LDS at all (64 KiB)
constexpr int VR_SCAN_ITEMS = 8;     // counters per thread and round of the scan

// the part of vertex v: parts[p] <= v < parts[p + 1] (an empty part is never the answer)
__device__ __forceinline__ int64_t vr_part_of(const int64_t *__restrict__ parts, int64_t P, int64_t v) {
  int64_t lo = 0, hi = P;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (parts[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

struct VrSeg {
  double xa, ya, xb, yb;
  int id;
  bool have;
};
// the segment that starts at vertex v: to the next vertex of its part, from the last one back to the first when
// `closed`; an open part of one vertex is a segment of length zero
__device__ __forceinline__ VrSeg vr_segment(const double *__restrict__ coords, const int64_t *__restrict__ parts,
                                            const int32_t *__restrict__ ids, int64_t P, int64_t N, int64_t v,
                                            bool closed) {
  VrSeg s{0.0, 0.0, 0.0, 0.0, 0, false};
  if (v >= N) return s;
  const int64_t p = vr_part_of(parts, P, v);
  const int64_t b = parts[p], e = parts[p + 1];
  int64_t w = v + 1;
  if (w == e) {
    if (!closed && e - b > 1) return s;
    w = closed ? b : v;
  }
  s.xa = coords[2 * v]; s.ya = coords[2 * v + 1];
  s.xb = coords[2 * w]; s.yb = coords[2 * w + 1];
  s.id = ids[p];
  s.have = true;
  return s;
}

// ---- polygons: crossings ---------------------------------------------------------------------------------------------
template <bool EMIT>
__device__ __forceinline__ void vr_cross_row(int r, double xa, double ya, double xb, double yb, int id, int W, int cb,
                                             uint32_t *__restrict__ rows, uint64_t *__restrict__ keys,
                                             int64_t capacity) {
  if (!EMIT) {
    atomicAdd(&rows[r], 1u);
    return;
  }
  const double yc = (double)r + 0.5;
  const double t = (yc - ya) / (yb - ya);
  const double x = xa + t * (xb - xa);
  double c = ceil(x - 0.5);
  c = !(c >= 0.0) ? 0.0 : (c > (double)W ? (double)W : c);
  const uint32_t pos = atomicAdd(&rows[r], 1u);
  if ((int64_t)pos < capacity) keys[pos] = ((uint64_t)(uint32_t)id << cb) | (uint64_t)(uint32_t)(int)c;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_vr_cross(const double *__restrict__ coords, const int64_t *__restrict__ parts,
                                                  const int32_t *__restrict__ ids, int64_t P, int64_t N, int H, int W,
                                                  int cb, uint32_t *__restrict__ rows, uint64_t *__restrict__ keys,
                                                  int64_t capacity, const int64_t *__restrict__ info) {
  if (EMIT && info[3] != 0) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  VrSeg s = vr_segment(coords, parts, ids, P, N, v, true);
  int r0 = 0, r1 = 0;
  if (s.have && s.ya != s.yb) {
    if (s.ya > s.yb) {  // upward: an edge shared by two polygons gives both the same crossing
      const double tx = s.xa, ty = s.ya;
      s.xa = s.xb; s.ya = s.yb; s.xb = tx; s.yb = ty;
    }
    double d0 = ceil(s.ya - 0.5), d1 = ceil(s.yb - 0.5);
    d0 = d0 < 0.0 ? 0.0 : d0;
    d1 = d1 > (double)H ? (double)H : d1;
    if (d0 < d1) {
      r0 = (int)d0;
      r1 = (int)d1;
    }
  }
  const int n = r1 - r0;
  if (n > 0 && n <= VR_SHORT)
    for (int r = r0; r < r1; r++) vr_cross_row<EMIT>(r, s.xa, s.ya, s.xb, s.yb, s.id, W, cb, rows, keys, capacity);
  unsigned long long longs = __ballot(n > VR_SHORT);
  while (longs) {
    const int src = __ffsll((long long)longs) - 1;
    longs &= longs - 1;
    const double xa = __shfl(s.xa, src), ya = __shfl(s.ya, src), xb = __shfl(s.xb, src), yb = __shfl(s.yb, src);
    const int id = __shfl(s.id, src), q0 = __shfl(r0, src), q1 = __shfl(r1, src);
    for (int r = q0 + lane; r < q1; r += 64) vr_cross_row<EMIT>(r, xa, ya, xb, yb, id, W, cb, rows, keys, capacity);
  }
}

// exclusive scan of the H row counters in place, one workgroup; info = {total, largest row, 0, total > capacity}
__global__ __launch_bounds__(256) void k_vr_scan(uint32_t *__restrict__ rows, int H, int64_t capacity,
                                                 int64_t *__restrict__ info) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_max[4];
  const int tid = (int)threadIdx.x;
  unsigned long long carry = 0;
  uint32_t biggest = 0;
  for (int64_t base = 0; base < H; base += 256 * VR_SCAN_ITEMS) {
    const int64_t first = base + (int64_t)tid * VR_SCAN_ITEMS;
    uint32_t c[VR_SCAN_ITEMS];
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < VR_SCAN_ITEMS; k++) {
      c[k] = first + k < H ? rows[first + k] : 0u;
      biggest = c[k] > biggest ? c[k] : biggest;
      sum += c[k];
    }
    uint32_t total;
    uint32_t before = dt_block_scan_256(sum, s_w, &total);
    // offsets beyond 2^32 belong to a call that overflows its capacity (< 2^31): nothing reads them
    before += (uint32_t)carry;
#pragma unroll
    for (int k = 0; k < VR_SCAN_ITEMS; k++) {
      if (first + k < H) rows[first + k] = before;
      before += c[k];
    }
    carry += total;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)biggest, o);
    biggest = t > biggest ? t : biggest;
  }
  if ((tid & 63) == 0) s_max[tid >> 6] = biggest;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; k++) biggest = s_max[k] > biggest ? s_max[k] : biggest;
    info[0] = (int64_t)carry;
    info[1] = (int64_t)biggest;
    info[2] = 0;
    info[3] = (int64_t)carry > capacity ? 1 : 0;
  }
}

// ---- polygons: the sort of a row ------------------------------------------------------------------------------------------
__device__ __forceinline__ void vr_compare_swap(uint64_t *a, uint32_t i, uint32_t l) {
  const uint64_t x = a[i], y = a[l];
  if (x > y) {
    a[i] = y;
    a[l] = x;
  }
}
// the all-ascending bitonic network on a[0, n), in LDS or in global memory, by the 256 threads of a workgroup: the
// first step of a merge of width k pairs i with i ^ (k - 1), the others pair i with i ^ j; a partner at or beyond n
// stands for +infinity, which never moves, so the pair is skipped
__device__ void vr_bitonic(uint64_t *a, uint32_t n) {
  uint32_t halves = 1;  // half of the smallest power of two >= n
  while (2 * halves < n) halves <<= 1;
  const uint32_t tid = threadIdx.x;
  for (uint32_t half = 1; half < n; half <<= 1) {
    const uint32_t k = half << 1;
    for (uint32_t t = tid; t < halves; t += 256) {
      const uint32_t pos = t & (half - 1), blk = (t - pos) << 1;
      const uint32_t i = blk + pos, l = blk + (k - 1 - pos);
      if (l < n) vr_compare_swap(a, i, l);
    }
    __syncthreads();
    for (uint32_t j = half >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < halves; t += 256) {
        const uint32_t pos = t & (j - 1);
        const uint32_t i = ((t - pos) << 1) | pos, l = i + j;
        if (l < n) vr_compare_swap(a, i, l);
      }
      __syncthreads();
    }
  }
}

// rows of LO < n keys: in LDS up to CAP; beyond CAP in global memory when SPILL, else left to the other launch
template <int CAP, int LO, bool SPILL>
__global__ __launch_bounds__(256) void k_vr_sort(const uint32_t *__restrict__ ends, uint64_t *__restrict__ keys,
                                                 int64_t *__restrict__ info) {
  __shared__ uint64_t s_keys[CAP];
  if (info[3] != 0) return;
  const uint32_t r = blockIdx.x;
  const uint32_t first = r ? ends[r - 1] : 0u;
  const uint32_t n = ends[r] - first;
  if (n < 2u || n <= (uint32_t)LO || (!SPILL && n > (uint32_t)CAP)) return;
  uint64_t *row = keys + first;
  if (n <= (uint32_t)CAP) {
    for (uint32_t t = threadIdx.x; t < n; t += 256) s_keys[t] = row[t];
    __syncthreads();
    vr_bitonic(s_keys, n);
    for (uint32_t t = threadIdx.x; t < n; t += 256) row[t] = s_keys[t];
  } else {
    if (threadIdx.x == 0) atomicAdd((unsigned long long *)&info[2], 1ull);
    vr_bitonic(row, n);
  }
}

// ---- polygons: the fill ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vr_fill(const uint32_t *__restrict__ ends, const uint64_t *__restrict__ keys,
                                                 int W, int cb, int32_t *__restrict__ label,
                                                 const int64_t *__restrict__ info) {
  if (info[3] != 0) return;
  const uint32_t r = blockIdx.x;
  const uint32_t first = r ? ends[r - 1] : 0u;
  const uint32_t pairs = (ends[r] - first) >> 1;
  if (pairs == 0) return;
  const uint64_t *row = keys + first;
  int32_t *out = label + (int64_t)r * W;
  const uint64_t mask = (1ull << cb) - 1ull;
  const int lane = (int)(threadIdx.x & 63u);
  // every lane of a wave makes the same number of rounds: the ballot below is the whole wave's
  for (uint32_t base = (threadIdx.x >> 6) * 64u; base < pairs; base += 256u) {
    const uint32_t q = base + (uint32_t)lane;
    int c0 = 0, c1 = 0, id = 0;
    if (q < pairs) {
      const uint64_t k0 = row[2 * q], k1 = row[2 * q + 1];
      id = (int)(k0 >> cb);
      c0 = (int)(k0 & mask);
      c1 = (int)(k1 & mask);
      c1 = c1 > W ? W : c1;  // a column is at most W by construction; keys that nobody wrote are not trusted
      c0 = c0 > W ? W : c0;
    }
    unsigned long long spans = __ballot(c1 > c0);  // the lanes read 64 spans, the wave fills them one after the other
    while (spans) {
      const int src = __ffsll((long long)spans) - 1;
      spans &= spans - 1;
      const int a = __shfl(c0, src), b = __shfl(c1, src), v = __shfl(id, src);
      for (int c = a + lane; c < b; c += 64) atomicMax(&out[c], v);
    }
  }
}

// ---- lines and points --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void vr_burn(int32_t *__restrict__ label, int H, int W, double fy, double fx, int id) {
  if (fy >= 0.0 && fy < (double)H && fx >= 0.0 && fx < (double)W) atomicMax(&label[(int64_t)(int)fy * W + (int)fx], id);
}
// the minor coordinate at major coordinate m: the endpoints by rule, not by arithmetic
__device__ __forceinline__ double vr_minor(double m, double ma, double na, double mb, double nb) {
  if (m == ma) return na;
  if (m == mb) return nb;
  return na + ((m - ma) / (mb - ma)) * (nb - na);
}
// column c of the major axis of a segment (ma, na) -> (mb, nb), ma < mb
__device__ __forceinline__ void vr_line_column(int c, double ma, double na, double mb, double nb, bool xmajor,
                                               int connectivity, int Wn, int32_t *__restrict__ label, int H, int W,
                                               int id) {
  if (connectivity == 4) {
    const double lo_m = (double)c, hi_m = (double)c + 1.0;
    const double m_in = ma > lo_m ? ma : lo_m, m_out = mb < hi_m ? mb : hi_m;
    const double n1 = vr_minor(m_in, ma, na, mb, nb), n2 = vr_minor(m_out, ma, na, mb, nb);
    double lo = floor(n1 < n2 ? n1 : n2), hi = floor(n1 < n2 ? n2 : n1);
    lo = lo < 0.0 ? 0.0 : lo;
    hi = hi > (double)(Wn - 1) ? (double)(Wn - 1) : hi;
    if (!(lo <= hi)) return;
    for (int q = (int)lo; q <= (int)hi; q++) {
      const int64_t cell = xmajor ? (int64_t)q * W + c : (int64_t)c * W + q;
      atomicMax(&label[cell], id);
    }
  } else {
    double ms = (double)c + 0.5;
    ms = ms > ma ? ms : ma;
    ms = ms < mb ? ms : mb;
    const double n = floor(vr_minor(ms, ma, na, mb, nb));
    if (xmajor) vr_burn(label, H, W, n, (double)c, id);
    else vr_burn(label, H, W, (double)c, n, id);
  }
}

__global__ __launch_bounds__(256) void k_vr_lines(const double *__restrict__ coords, const int64_t *__restrict__ parts,
                                                  const int32_t *__restrict__ ids, int64_t P, int64_t N, int H, int W,
                                                  int connectivity, int closed, int32_t *__restrict__ label,
                                                  const int64_t *__restrict__ info) {
  if (info[3] != 0) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const VrSeg s = vr_segment(coords, parts, ids, P, N, v, closed != 0);
  double ma = 0.0, na = 0.0, mb = 0.0, nb = 0.0;
  int xmajor = 1, c0 = 0, n = 0;
  if (s.have) {
    const double dx = s.xb - s.xa, dy = s.yb - s.ya;
    if (dx == 0.0 && dy == 0.0) {
      vr_burn(label, H, W, floor(s.ya), floor(s.xa), s.id);
    } else {
      if (connectivity == 8) {
        vr_burn(label, H, W, floor(s.ya), floor(s.xa), s.id);
        vr_burn(label, H, W, floor(s.yb), floor(s.xb), s.id);
      }
      xmajor = fabs(dx) >= fabs(dy);
      ma = xmajor ? s.xa : s.ya; na = xmajor ? s.ya : s.xa;
      mb = xmajor ? s.xb : s.yb; nb = xmajor ? s.yb : s.xb;
      if (ma > mb) {
        const double tm = ma, tn = na;
        ma = mb; na = nb; mb = tm; nb = tn;
      }
      const int Wm = xmajor ? W : H;
      double lo = floor(ma), hi = floor(mb);
      lo = lo < 0.0 ? 0.0 : lo;
      hi = hi > (double)(Wm - 1) ? (double)(Wm - 1) : hi;
      if (lo <= hi) {
        c0 = (int)lo;
        n = (int)hi - c0 + 1;
      }
    }
  }
  if (n > 0 && n <= VR_SHORT)
    for (int c = c0; c < c0 + n; c++)
      vr_line_column(c, ma, na, mb, nb, xmajor != 0, connectivity, xmajor ? H : W, label, H, W, s.id);
  unsigned long long longs = __ballot(n > VR_SHORT);
  while (longs) {
    const int src = __ffsll((long long)longs) - 1;
    longs &= longs - 1;
    const double qma = __shfl(ma, src), qna = __shfl(na, src), qmb = __shfl(mb, src), qnb = __shfl(nb, src);
    const int qx = __shfl(xmajor, src), q0 = __shfl(c0, src), qn = __shfl(n, src), id = __shfl(s.id, src);
    for (int c = q0 + lane; c < q0 + qn; c += 64)
      vr_line_column(c, qma, qna, qmb, qnb, qx != 0, connectivity, qx ? H : W, label, H, W, id);
  }
}

__global__ __launch_bounds__(256) void k_vr_points(const double *__restrict__ coords, const int64_t *__restrict__ parts,
                                                   const int32_t *__restrict__ ids, int64_t P, int64_t N, int H, int W,
                                                   int32_t *__restrict__ label) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  const int id = ids[vr_part_of(parts, P, v)];
  vr_burn(label, H, W, floor(coords[2 * v + 1]), floor(coords[2 * v]), id);
}

struct VrScratch {
  uint32_t *rows;
  uint64_t *keys;
  size_t bytes;
  VrScratch(void *p, int64_t H, int64_t capacity) {
    DtCarver c(p);
    rows = c.take<uint32_t>((size_t)H);
    keys = c.take<uint64_t>((size_t)capacity);
    bytes = c.bytes();
  }
};

}  // namespace

// What both tiers require of a rasterisation call, pointers aside (the contract is in include/descriptools_hip.h).
int dt_check_rasterize(int kind, int64_t P, int64_t N, int64_t H, int64_t W, int connectivity, int all_touched,
                       int64_t capacity) {
  DT_REQUIRE(kind >= VR_POLYGON && kind <= VR_POINT, "kind must be 0 (polygon), 1 (line) or 2 (point)");
  DT_REQUIRE(H >= 1 && W >= 1, "empty raster shape");
  DT_REQUIRE(H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31), "raster of 2^31 cells or more");
  DT_REQUIRE(P >= 0 && N >= 0 && P < (1ll << 31) && N < (1ll << 31), "P and N must be in [0, 2^31)");
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
  DT_REQUIRE(all_touched == 0 || all_touched == 1, "all_touched must be 0 or 1");
  DT_REQUIRE(capacity >= 0 && capacity < (1ll << 31), "capacity must be in [0, 2^31) crossings");
  return DT_OK;
}

size_t dt_rasterize_scratch(int64_t H, int64_t capacity) { return VrScratch(nullptr, H, capacity).bytes; }

// The crossings of a polygon geometry with the centre lines of the H rows, and the most on any one row, in host
// arithmetic: the same closed form as k_vr_cross.  parts has passed the caller's checks (non-decreasing from 0).
void dt_rasterize_count_host(const double *coords, const int64_t *parts, int64_t P, int64_t H, int64_t *total,
                             int64_t *largest) {
  std::vector<std::pair<int32_t, int32_t>> events;  // (row, +1 / -1)
  int64_t sum = 0;
  for (int64_t p = 0; p < P; p++) {
    const int64_t b = parts[p], e = parts[p + 1];
    for (int64_t v = b; v < e; v++) {
      const int64_t w = v + 1 == e ? b : v + 1;
      double ya = coords[2 * v + 1], yb = coords[2 * w + 1];
      if (ya == yb) continue;
      if (ya > yb) std::swap(ya, yb);
      double d0 = std::ceil(ya - 0.5), d1 = std::ceil(yb - 0.5);
      d0 = d0 < 0.0 ? 0.0 : d0;
      d1 = d1 > (double)H ? (double)H : d1;
      if (!(d0 < d1)) continue;
      events.emplace_back((int32_t)d0, 1);
      events.emplace_back((int32_t)d1, -1);  // H < 2^31
      sum += (int64_t)d1 - (int64_t)d0;
    }
  }
  std::sort(events.begin(), events.end());
  int64_t open = 0, most = 0;
  for (size_t k = 0; k < events.size(); k++) {
    open += events[k].second;
    if (k + 1 == events.size() || events[k + 1].first != events[k].first) most = open > most ? open : most;
  }
  *total = sum;
  *largest = most;
}

// Arguments that have passed dt_check_rasterize.  info: int64[4] on the device.  scratch: dt_rasterize_scratch(H,
// capacity) bytes (unused for lines and points).  ev: NULL, or 8 events recorded around the seven phases (clear,
// count, scan, emit, sort, fill, lines / points).  Nothing synchronises, nothing is allocated.
int dt_launch_rasterize(hipStream_t s, int kind, const double *coords, const int64_t *parts, const int32_t *ids,
                        int64_t P, int64_t N, int64_t H, int64_t W, int connectivity, int all_touched,
                        int64_t capacity, void *scratch, size_t scratch_bytes, int32_t *label, int64_t *info,
                        hipEvent_t *ev) {
  const VrScratch ws(scratch, H, capacity);
  const bool polygon = kind == VR_POLYGON && N > 0 && P > 0;
  DT_REQUIRE(!polygon || (scratch && scratch_bytes >= ws.bytes), "scratch too small");
  const int h = (int)H, w = (int)W;
  int cb = 1;
  while ((1ll << cb) <= W) cb++;  // bits of the columns 0 .. W
  const dim3 b(256), per_vertex((unsigned)((N + 255) / 256)), per_row((unsigned)H);
  int e = 0;
#define VR_MARK() \
  do { if (ev) DT_HIP(hipEventRecord(ev[e++], s)); } while (0)
  VR_MARK();
  DT_HIP(hipMemsetAsync(label, 0xFF, (size_t)H * W * sizeof(int32_t), s));
  DT_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), s));
  if (polygon) DT_HIP(hipMemsetAsync(ws.rows, 0, (size_t)H * sizeof(uint32_t), s));
  VR_MARK();
  if (polygon)
    hipLaunchKernelGGL(k_vr_cross<false>, per_vertex, b, 0, s, coords, parts, ids, P, N, h, w, cb, ws.rows, ws.keys,
                       capacity, info);
  VR_MARK();
  if (polygon) hipLaunchKernelGGL(k_vr_scan, dim3(1), b, 0, s, ws.rows, h, capacity, info);
  VR_MARK();
  if (polygon)
    hipLaunchKernelGGL(k_vr_cross<true>, per_vertex, b, 0, s, coords, parts, ids, P, N, h, w, cb, ws.rows, ws.keys,
                       capacity, info);
  VR_MARK();
  if (polygon) {
    hipLaunchKernelGGL((k_vr_sort<VR_LDS_SMALL, 0, false>), per_row, b, 0, s, ws.rows, ws.keys, info);
    hipLaunchKernelGGL((k_vr_sort<VR_LDS_LARGE, VR_LDS_SMALL, true>), per_row, b, 0, s, ws.rows, ws.keys, info);
  }
  VR_MARK();
  if (polygon) hipLaunchKernelGGL(k_vr_fill, per_row, b, 0, s, ws.rows, ws.keys, w, cb, label, info);
  VR_MARK();
  if (N > 0 && P > 0) {
    if (kind == VR_POINT)
      hipLaunchKernelGGL(k_vr_points, per_vertex, b, 0, s, coords, parts, ids, P, N, h, w, label);
    else if (kind == VR_LINE || all_touched)
      hipLaunchKernelGGL(k_vr_lines, per_vertex, b, 0, s, coords, parts, ids, P, N, h, w,
                         kind == VR_LINE ? connectivity : 4, kind == VR_POLYGON ? 1 : 0, label, info);
  }
  VR_MARK();
#undef VR_MARK
  return DT_OK;
}
