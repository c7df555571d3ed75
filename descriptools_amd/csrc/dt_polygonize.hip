// dt_polygonize.hip -- polygonisation: an int32 label raster traced into the rings of its regions, the inverse of
// dt_vector.hip's polygon fill (vector.py holds the definition, tests/_polygonize_ref.py is its reference).  A cell with
// a label >= 0 owns up to four directed boundary edges -- its top edge travels east, its right edge south, its bottom
// edge west, its left edge north, the cell on the right of the travel -- wherever the neighbour across differs or lies
// outside.  The successor of an edge follows from the 2 x 2 cells at its head (right turn, straight on, left turn, in
// that order of preference), a `corner` is an edge whose successor turns, and the rings are the cycles of the successor.
// There is no sort, no hash and no search: everything is counting, scanning and pointer doubling.
//
//   count    k_pg_count: a thread per PG_ITEMS cells counts edges and corners; k_pg_scan (one workgroup,
//            dt_block_scan_256, no atomics) scans the per-block sums; totals and the overflow flags go to info
//   link     k_pg_offsets gives every cell the dense index of its first edge (its edges follow in the order E S W N);
//            k_pg_link writes for every edge the word (key << 31) | successor, key = 2 * tail vertex + (not eastward):
//            33 + 31 bits, so that a doubling step is one 8-byte load and one 8-byte store per edge
//   leaders  k_pg_min, double-buffered pointer doubling: (smallest key in the window, jump pointer).  A round that
//            lowers no key means every window covers its cycle; the rounds behind it return at once.
//            The smallest key of a ring is its start vertex, and names the edge that leaves it: the leader
//   ranks    k_pg_rank_init cuts every cycle in front of its leader; k_pg_rank, the same doubling on (done, corners to
//            the end of the list, jump pointer), ranks the corners from the leader
//   rings    k_pg_ring_count / k_pg_scan / k_pg_rings: a thread per PG_ITEMS lattice vertices in vertex order; a leader
//            leaves its start vertex eastward (a shell) or southward (a hole), at most one of each per vertex, so the
//            scan of the vertices IS the order of the parts: parts, ids and the hole marks
//   emit     k_pg_emit: every corner writes its head vertex at parts[ring] + rank
//   shells   k_pg_walk: a wave per hole walks west from the cell above its start vertex, 64 cells per ballot, to the
//            first cell of another label and takes the ring of the edge it crosses; k_pg_shell resolves chains of holes
//            by pointer jumping, again with rounds that return at once behind a quiet one
// Every kernel after the count returns at once when the edges do not fit, every writer of an output when anything does
// not fit: the outputs then stay untouched.  No kernel writes at or past a capacity.
#include "dt_common.h"
#include "dt_kernels.h"

namespace {

constexpr int PG_ITEMS = 4;          // cells / vertices per thread of the scanning kernels
constexpr int PG_BLOCK = 256 * PG_ITEMS;
constexpr int PG_SCAN_ITEMS = 8;     // block sums per thread and round of k_pg_scan
constexpr int PG_GRID = 2048;        // blocks of the kernels whose item count only the device knows
constexpr int PG_CTL = 64;           // words per doubling of the rounds' "lowered something" flags
constexpr uint64_t PG_PTR = (1ull << 31) - 1ull;
constexpr uint64_t PG_DONE = 1ull << 63;

enum { PG_EDGES = 0, PG_VERTICES, PG_RINGS, PG_HOLES, PG_ROUNDS, PG_OVERFLOW, PG_RANK_ROUNDS, PG_SHELL_ROUNDS };
enum { PG_OVER_EDGES = 1, PG_OVER_VERTICES = 2, PG_OVER_RINGS = 4 };

struct PgGrid {
  const int32_t *lab;
  int H, W;
};
// the label of a cell: -1 for every negative value and outside the raster
__device__ __forceinline__ int pg_lab(const PgGrid &g, int i, int j) {
  if (i < 0 || i >= g.H || j < 0 || j >= g.W) return -1;
  const int v = g.lab[(int64_t)i * g.W + j];
  return v < 0 ? -1 : v;
}
// the row of a flat cell index: below 2^31, so the division is a 32-bit one (a 64-bit one is a subroutine of its own,
// and these kernels are made of index arithmetic)
__device__ __forceinline__ int pg_row(const PgGrid &g, int64_t cell) { return (int)((uint32_t)cell / (uint32_t)g.W); }
// directions 0 E, 1 S, 2 W, 3 N as (dy, dx)
__device__ __forceinline__ int pg_dy(int d) { return (d == 1) - (d == 3); }
__device__ __forceinline__ int pg_dx(int d) { return (d == 0) - (d == 2); }
// the edges of cell (i, j): bit d is set when the neighbour on the left of direction d differs
__device__ __forceinline__ int pg_mask(const PgGrid &g, int i, int j, int &L) {
  L = pg_lab(g, i, j);
  if (L < 0) return 0;
  return (int)(pg_lab(g, i - 1, j) != L) | (int)(pg_lab(g, i, j + 1) != L) << 1 | (int)(pg_lab(g, i + 1, j) != L) << 2 |
         (int)(pg_lab(g, i, j - 1) != L) << 3;
}
// the cell diagonally ahead on the left of edge d of cell (i, j)
__device__ __forceinline__ int pg_diag(const PgGrid &g, int i, int j, int d) {
  const int l = (d + 3) & 3;
  return pg_lab(g, i + pg_dy(d) + pg_dy(l), j + pg_dx(d) + pg_dx(l));
}
// does the successor of edge d of cell (i, j) turn?  right when the cell has edge d + 1, left when the diagonal is L
__device__ __forceinline__ bool pg_corner(const PgGrid &g, int i, int j, int d, int L, int mask) {
  return ((mask >> ((d + 1) & 3)) & 1) || pg_diag(g, i, j, d) == L;
}
__device__ __forceinline__ uint64_t pg_key(const PgGrid &g, int i, int j, int d) {
  const int64_t ty = i + (d >= 2), tx = j + (d == 1 || d == 2);
  return 2ull * (uint64_t)(ty * (g.W + 1) + tx) + (d != 0);
}
// the dense index of edge d of cell (i, j), which has it
__device__ __forceinline__ uint32_t pg_edge(const PgGrid &g, const uint32_t *__restrict__ celloff, int i, int j, int d) {
  int L;
  const int m = pg_mask(g, i, j, L);
  return celloff[(int64_t)i * g.W + j] + (uint32_t)__popc(m & ((1 << d) - 1));
}
// the dense index of the successor of edge d of cell (i, j) of label L
__device__ __forceinline__ uint32_t pg_next(const PgGrid &g, const uint32_t *__restrict__ celloff, int i, int j, int d,
                                            int L, int mask, uint32_t first) {
  const int r = (d + 1) & 3;
  if ((mask >> r) & 1) return first + (uint32_t)__popc(mask & ((1 << r) - 1));  // right: the cell's own next edge
  const int fi = i + pg_dy(d), fj = j + pg_dx(d), l = (d + 3) & 3;
  const int di = fi + pg_dy(l), dj = fj + pg_dx(l);
  if (pg_lab(g, di, dj) != L) return pg_edge(g, celloff, fi, fj, d);  // straight on along the next cell
  return pg_edge(g, celloff, di, dj, l);                              // left, around the diagonal cell
}

// ---- count and scan ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pg_cell_counts(const PgGrid &g, int64_t cell, uint32_t &edges, uint32_t &corners) {
  const int i = pg_row(g, cell), j = (int)(cell - (int64_t)i * g.W);
  int L;
  const int m = pg_mask(g, i, j, L);
  edges = (uint32_t)__popc(m);
  corners = 0;
  for (int d = 0; d < 4; d++)
    if ((m >> d) & 1) corners += pg_corner(g, i, j, d, L, m) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_pg_count(PgGrid g, int64_t N, uint32_t *__restrict__ bs_edges,
                                                  uint32_t *__restrict__ bs_corners) {
  __shared__ uint32_t s_w[4];
  const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PG_ITEMS;
  uint32_t e = 0, c = 0;
  for (int k = 0; k < PG_ITEMS; k++)
    if (first + k < N) {
      uint32_t ek, ck;
      pg_cell_counts(g, first + k, ek, ck);
      e += ek;
      c += ck;
    }
  uint32_t te, tc;
  dt_block_scan_256(e, s_w, &te);
  dt_block_scan_256(c, s_w, &tc);
  if (threadIdx.x == 0) {
    bs_edges[blockIdx.x] = te;
    bs_corners[blockIdx.x] = tc;
  }
}

// exclusive scan of the two arrays of nb block sums in place, one workgroup.  rings == 0: the sums are edges and
// corners, info = {edges, corners, ...} and the flags of the edge and vertex capacities; rings == 1: the sums are rings
// and their vertices, info[PG_RINGS] and the flag of the ring capacity.  An offset beyond 2^32 belongs to a call whose
// edges overflow their capacity (< 2^31): nothing reads it.
__global__ __launch_bounds__(256) void k_pg_scan(uint32_t *__restrict__ a, uint32_t *__restrict__ b, int64_t nb,
                                                 int rings, int64_t cap0, int64_t cap1, int64_t *__restrict__ info) {
  __shared__ uint32_t s_w[4];
  if (rings && (info[PG_OVERFLOW] & PG_OVER_EDGES)) return;
  const int tid = (int)threadIdx.x;
  unsigned long long carry_a = 0, carry_b = 0;
  for (int64_t base = 0; base < nb; base += 256 * PG_SCAN_ITEMS) {
    const int64_t first = base + (int64_t)tid * PG_SCAN_ITEMS;
    uint32_t ca[PG_SCAN_ITEMS], cb[PG_SCAN_ITEMS];
    uint32_t sa = 0, sb = 0;
#pragma unroll
    for (int k = 0; k < PG_SCAN_ITEMS; k++) {
      ca[k] = first + k < nb ? a[first + k] : 0u;
      cb[k] = first + k < nb ? b[first + k] : 0u;
      sa += ca[k];
      sb += cb[k];
    }
    uint32_t ta, tb;
    uint32_t before_a = dt_block_scan_256(sa, s_w, &ta) + (uint32_t)carry_a;
    uint32_t before_b = dt_block_scan_256(sb, s_w, &tb) + (uint32_t)carry_b;
#pragma unroll
    for (int k = 0; k < PG_SCAN_ITEMS; k++) {
      if (first + k < nb) {
        a[first + k] = before_a;
        b[first + k] = before_b;
      }
      before_a += ca[k];
      before_b += cb[k];
    }
    carry_a += ta;
    carry_b += tb;
  }
  if (tid == 0) {
    if (!rings) {
      const int64_t over = ((int64_t)carry_a > cap0 ? PG_OVER_EDGES : 0) | ((int64_t)carry_b > cap1 ? PG_OVER_VERTICES : 0);
      info[PG_EDGES] = (int64_t)carry_a;
      info[PG_VERTICES] = (int64_t)carry_b;
      info[PG_RINGS] = info[PG_HOLES] = (over & PG_OVER_EDGES) ? -1 : 0;  // unknown without the edge arrays
      info[PG_OVERFLOW] = over;
    } else {
      info[PG_RINGS] = (int64_t)carry_a;
      if ((int64_t)carry_a > cap0) info[PG_OVERFLOW] |= PG_OVER_RINGS;
    }
  }
}

// ---- link --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_offsets(PgGrid g, int64_t N, const uint32_t *__restrict__ bs_edges,
                                                    uint32_t *__restrict__ celloff, const int64_t *__restrict__ info) {
  __shared__ uint32_t s_w[4];
  if (info[PG_OVERFLOW] & PG_OVER_EDGES) return;
  const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PG_ITEMS;
  uint32_t e[PG_ITEMS];
  uint32_t sum = 0;
  for (int k = 0; k < PG_ITEMS; k++) {
    e[k] = 0;
    if (first + k < N) {
      uint32_t ck;
      pg_cell_counts(g, first + k, e[k], ck);
    }
    sum += e[k];
  }
  uint32_t total;
  uint32_t before = dt_block_scan_256(sum, s_w, &total) + bs_edges[blockIdx.x];
  for (int k = 0; k < PG_ITEMS; k++) {
    if (first + k < N) celloff[first + k] = before;
    before += e[k];
  }
}

__global__ __launch_bounds__(256) void k_pg_link(PgGrid g, int64_t N, const uint32_t *__restrict__ celloff,
                                                 uint64_t *__restrict__ words, int64_t cap_edges,
                                                 const int64_t *__restrict__ info) {
  if (info[PG_OVERFLOW] & PG_OVER_EDGES) return;
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= N) return;
  const int i = pg_row(g, cell), j = (int)(cell - (int64_t)i * g.W);
  int L;
  const int m = pg_mask(g, i, j, L);
  if (!m) return;
  const uint32_t first = celloff[cell];
  uint32_t e = first;
  for (int d = 0; d < 4; d++)
    if ((m >> d) & 1) {
      const uint32_t nx = pg_next(g, celloff, i, j, d, L, m, first);
      if ((int64_t)e < cap_edges) words[e] = (pg_key(g, i, j, d) << 31) | (uint64_t)nx;
      e++;
    }
}

// ---- leaders -----------------------------------------------------------------------------------------------------------
// round r >= 1 of the doubling: dst = (min(key, key of the jump target), the target's jump pointer)
__global__ __launch_bounds__(256) void k_pg_min(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst,
                                                const int64_t *__restrict__ info, uint32_t *__restrict__ ctl, int r) {
  if (info[PG_OVERFLOW] & PG_OVER_EDGES) return;
  if (r > 1 && ctl[r - 1] == 0u) return;
  const int64_t E = info[PG_EDGES];
  bool lowered = false;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
    const uint64_t w = src[e];
    const uint64_t q = src[w & PG_PTR];
    const uint64_t kw = w >> 31, kq = q >> 31;
    dst[e] = ((kq < kw ? kq : kw) << 31) | (q & PG_PTR);
    lowered |= kq < kw;
  }
  if (lowered) ctl[r] = 1u;
}

// ---- ranks -------------------------------------------------------------------------------------------------------------
// the dense index of the edge that leaves the start vertex of key m: eastward the top edge of the cell at the vertex,
// southward the right edge of the cell on its left
__device__ __forceinline__ uint32_t pg_leader(const PgGrid &g, const uint32_t *__restrict__ celloff, uint64_t m) {
  const uint32_t v = (uint32_t)(m >> 1), W1 = (uint32_t)g.W + 1u;  // a vertex index is below 2^32
  const int hole = (int)(m & 1ull);
  const int y = (int)(v / W1), x = (int)(v - (uint32_t)y * W1);
  return pg_edge(g, celloff, y, x - hole, hole);
}

__global__ __launch_bounds__(256) void k_pg_rank_init(PgGrid g, int64_t N, const uint32_t *__restrict__ celloff,
                                                      const uint64_t *__restrict__ mins, uint64_t *__restrict__ words,
                                                      uint32_t *__restrict__ lead, int64_t cap_edges,
                                                      const int64_t *__restrict__ info) {
  if (info[PG_OVERFLOW] & PG_OVER_EDGES) return;
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= N) return;
  const int i = pg_row(g, cell), j = (int)(cell - (int64_t)i * g.W);
  int L;
  const int m = pg_mask(g, i, j, L);
  if (!m) return;
  const uint32_t first = celloff[cell];
  uint32_t e = first;
  for (int d = 0; d < 4; d++)
    if ((m >> d) & 1) {
      if ((int64_t)e < cap_edges) {
        const uint32_t ld = pg_leader(g, celloff, mins[e] >> 31);
        const uint32_t nx = pg_next(g, celloff, i, j, d, L, m, first);
        const uint64_t c = pg_corner(g, i, j, d, L, m) ? 1ull : 0ull;
        lead[e] = ld;
        words[e] = nx == ld ? (PG_DONE | (c << 31) | (uint64_t)e) : ((c << 31) | (uint64_t)nx);
      }
      e++;
    }
}

// round r >= 1: an edge that has not reached the end of its list adds its jump target's corners and takes its pointer
__global__ __launch_bounds__(256) void k_pg_rank(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst,
                                                 const int64_t *__restrict__ info, uint32_t *__restrict__ ctl, int r) {
  if (info[PG_OVERFLOW] & PG_OVER_EDGES) return;
  if (r > 1 && ctl[r - 1] == 0u) return;
  const int64_t E = info[PG_EDGES];
  bool moved = false;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
    uint64_t w = src[e];
    if (!(w & PG_DONE)) {
      const uint64_t q = src[w & PG_PTR];
      const uint64_t sum = ((w >> 31) & 0xFFFFFFFFull) + ((q >> 31) & 0xFFFFFFFFull);
      w = (q & PG_DONE) | (sum << 31) | (q & PG_PTR);
      moved = true;
    }
    dst[e] = w;
  }
  if (moved) ctl[r] = 1u;
}

// ---- rings -------------------------------------------------------------------------------------------------------------
// the leaders that leave lattice vertex u, the shell first: their edges, labels and vertex counts; returns how many
__device__ __forceinline__ int pg_vertex_leaders(const PgGrid &g, const uint32_t *__restrict__ celloff,
                                                 const uint32_t *__restrict__ lead, const uint64_t *__restrict__ ranks,
                                                 int64_t u, uint32_t (&edge)[2], int (&label)[2], uint32_t (&size)[2],
                                                 int (&hole)[2]) {
  const uint32_t W1 = (uint32_t)g.W + 1u;  // H (W + 1) <= 2^32 - 1: 32-bit division
  const int y = (int)((uint32_t)u / W1), x = (int)((uint32_t)u - (uint32_t)y * W1);
  int n = 0;
  for (int h = 0; h < 2; h++) {
    const int j = x - h;
    if (j < 0 || j >= g.W) continue;
    int L;
    const int m = pg_mask(g, y, j, L);
    if (!((m >> h) & 1)) continue;
    const uint32_t e = celloff[(int64_t)y * g.W + j] + (uint32_t)(h ? (m & 1) : 0);
    if (lead[e] != e) continue;
    edge[n] = e;
    label[n] = L;
    size[n] = (uint32_t)((ranks[e] >> 31) & 0xFFFFFFFFull);
    hole[n] = h;
    n++;
  }
  return n;
}

__global__ __launch_bounds__(256) void k_pg_ring_count(PgGrid g, int64_t NV, const uint32_t *__restrict__ celloff,
                                                       const uint32_t *__restrict__ lead,
                                                       const uint64_t *__restrict__ ranks, uint32_t *__restrict__ bs_rings,
                                                       uint32_t *__restrict__ bs_verts, const int64_t *__restrict__ info) {
  __shared__ uint32_t s_w[4];
  if (info[PG_OVERFLOW] & PG_OVER_EDGES) return;
  const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PG_ITEMS;
  uint32_t r = 0, v = 0;
  for (int k = 0; k < PG_ITEMS; k++)
    if (first + k < NV) {
      uint32_t edge[2], size[2];
      int label[2], hole[2];
      const int n = pg_vertex_leaders(g, celloff, lead, ranks, first + k, edge, label, size, hole);
      for (int q = 0; q < n; q++) {
        r++;
        v += size[q];
      }
    }
  uint32_t tr, tv;
  dt_block_scan_256(r, s_w, &tr);
  dt_block_scan_256(v, s_w, &tv);
  if (threadIdx.x == 0) {
    bs_rings[blockIdx.x] = tr;
    bs_verts[blockIdx.x] = tv;
  }
}

// parts, ids, the hole marks (shell = -1, its own position for a shell) and the ring of every leader
__global__ __launch_bounds__(256) void k_pg_rings(PgGrid g, int64_t NV, const uint32_t *__restrict__ celloff,
                                                  const uint32_t *__restrict__ lead, const uint64_t *__restrict__ ranks,
                                                  const uint32_t *__restrict__ bs_rings,
                                                  const uint32_t *__restrict__ bs_verts, uint32_t *__restrict__ ringof,
                                                  int64_t cap_rings, int64_t *__restrict__ parts,
                                                  int32_t *__restrict__ ids, int32_t *__restrict__ shell,
                                                  int64_t *__restrict__ info) {
  __shared__ uint32_t s_w[4];
  if (info[PG_OVERFLOW] != 0) return;
  const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PG_ITEMS;
  uint32_t edge[PG_ITEMS][2], size[PG_ITEMS][2];
  int label[PG_ITEMS][2], hole[PG_ITEMS][2], n[PG_ITEMS];
  uint32_t r = 0, v = 0, holes = 0;
#pragma unroll
  for (int k = 0; k < PG_ITEMS; k++) {
    n[k] = first + k < NV ? pg_vertex_leaders(g, celloff, lead, ranks, first + k, edge[k], label[k], size[k], hole[k]) : 0;
    for (int q = 0; q < n[k]; q++) {
      r++;
      v += size[k][q];
      holes += (uint32_t)hole[k][q];
    }
  }
  uint32_t tr, tv, th;
  uint32_t ring = dt_block_scan_256(r, s_w, &tr) + bs_rings[blockIdx.x];
  uint32_t at = dt_block_scan_256(v, s_w, &tv) + bs_verts[blockIdx.x];
  dt_block_scan_256(holes, s_w, &th);
#pragma unroll
  for (int k = 0; k < PG_ITEMS; k++)
    for (int q = 0; q < n[k]; q++) {
      if ((int64_t)ring < cap_rings) {
        parts[ring] = (int64_t)at;
        ids[ring] = label[k][q];
        shell[ring] = hole[k][q] ? -1 : (int32_t)ring;
        ringof[edge[k][q]] = ring;
      }
      ring++;
      at += size[k][q];
    }
  if (threadIdx.x == 0 && th) atomicAdd((unsigned long long *)&info[PG_HOLES], (unsigned long long)th);
  if (blockIdx.x == 0 && threadIdx.x == 0) parts[info[PG_RINGS]] = info[PG_VERTICES];
}

// ---- emit --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_emit(PgGrid g, int64_t N, const uint32_t *__restrict__ celloff,
                                                 const uint32_t *__restrict__ lead, const uint64_t *__restrict__ ranks,
                                                 const uint32_t *__restrict__ ringof, const int64_t *__restrict__ parts,
                                                 int64_t cap_vertices, double *__restrict__ coords,
                                                 const int64_t *__restrict__ info) {
  if (info[PG_OVERFLOW] != 0) return;
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= N) return;
  const int i = pg_row(g, cell), j = (int)(cell - (int64_t)i * g.W);
  int L;
  const int m = pg_mask(g, i, j, L);
  if (!m) return;
  uint32_t e = celloff[cell];
  for (int d = 0; d < 4; d++)
    if ((m >> d) & 1) {
      if (pg_corner(g, i, j, d, L, m)) {
        const uint32_t ring = ringof[lead[e]];
        const int64_t p0 = parts[ring], n = parts[ring + 1] - p0;
        const int64_t to_end = (int64_t)((ranks[e] >> 31) & 0xFFFFFFFFull);  // corners from e to the list's end, e included
        const int64_t at = p0 + (n > 0 ? (n - to_end + 1) % n : 0);
        if (n > 0 && at >= 0 && at < cap_vertices) {
          coords[2 * at] = (double)(j + (d <= 1));                  // the head vertex of the edge
          coords[2 * at + 1] = (double)(i + (d == 1 || d == 2));
        }
      }
      e++;
    }
}

// ---- shells ------------------------------------------------------------------------------------------------------------
// a wave per ring; a hole walks west along the row above its start vertex
__global__ __launch_bounds__(256) void k_pg_walk(PgGrid g, const uint32_t *__restrict__ celloff,
                                                 const uint32_t *__restrict__ lead, const uint32_t *__restrict__ ringof,
                                                 const int64_t *__restrict__ parts, const double *__restrict__ coords,
                                                 int32_t *__restrict__ shell, const int64_t *__restrict__ info) {
  if (info[PG_OVERFLOW] != 0) return;
  const int64_t P = info[PG_RINGS];
  const int lane = (int)(threadIdx.x & 63u);
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < P; p += (int64_t)gridDim.x * 4) {
    if (shell[p] != -1) continue;  // the same for the whole wave
    const int64_t at = parts[p];
    const int x = (int)coords[2 * at], y = (int)coords[2 * at + 1];
    const int L = pg_lab(g, y - 1, x);
    int stop = x;  // the first column, going west, whose cell is not L
    for (int base = x;; base -= 64) {
      const int col = base - lane;
      const unsigned long long other = __ballot(col < 0 || pg_lab(g, y - 1, col) != L);
      if (other) {
        stop = base - (__ffsll((long long)other) - 1);
        break;
      }
    }
    if (lane == 0 && y >= 1 && stop + 1 <= x) shell[p] = (int32_t)ringof[lead[pg_edge(g, celloff, y - 1, stop + 1, 3)]];
  }
}

// round r >= 1 of the pointer jumping over the hole -> ring links: in place, a link only ever moves towards its shell
__global__ __launch_bounds__(256) void k_pg_shell(int32_t *__restrict__ shell, const int64_t *__restrict__ info,
                                                  uint32_t *__restrict__ ctl, int r) {
  if (info[PG_OVERFLOW] != 0) return;
  if (r > 1 && ctl[r - 1] == 0u) return;
  const int64_t P = info[PG_RINGS];
  bool moved = false;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int32_t s = __atomic_load_n(&shell[p], __ATOMIC_RELAXED);
    if (s < 0 || s >= P || s == p) continue;
    const int32_t t = __atomic_load_n(&shell[s], __ATOMIC_RELAXED);
    if (t >= 0 && t < P && t != s) {
      __atomic_store_n(&shell[p], t, __ATOMIC_RELAXED);
      moved = true;
    }
  }
  if (moved) ctl[r] = 1u;
}

// the rounds the doublings ran, the quiet one included
__global__ void k_pg_finish(const uint32_t *__restrict__ ctl, int issued, int shell_issued, int64_t *__restrict__ info) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (info[PG_OVERFLOW] & PG_OVER_EDGES) return;
  for (int k = 0; k < 2; k++) {
    int r = 1;
    while (r < issued && ctl[k * PG_CTL + r] != 0u) r++;
    info[k ? PG_RANK_ROUNDS : PG_ROUNDS] = r;
  }
  if (info[PG_OVERFLOW] == 0) {
    int r = 1;
    while (r < shell_issued && ctl[2 * PG_CTL + r] != 0u) r++;
    info[PG_SHELL_ROUNDS] = r;
  }
}

struct PgScratch {
  uint32_t *ctl, *bs0, *bs1, *celloff, *lead;
  uint64_t *words0, *words1;
  size_t bytes;
  // count_only: the block sums alone
  PgScratch(void *p, int64_t H, int64_t W, int64_t cap_edges, bool count_only) {
    DtCarver c(p);
    const size_t nb = (size_t)((H * (W + 1) + PG_BLOCK - 1) / PG_BLOCK);
    ctl = c.take<uint32_t>(3 * PG_CTL);
    bs0 = c.take<uint32_t>(nb);
    bs1 = c.take<uint32_t>(nb);
    celloff = c.take<uint32_t>(count_only ? 0 : (size_t)(H * W));
    words0 = c.take<uint64_t>((size_t)cap_edges);
    words1 = c.take<uint64_t>((size_t)cap_edges);
    lead = c.take<uint32_t>((size_t)cap_edges);
    bytes = c.bytes();
  }
};

}  // namespace

// What both tiers require of a polygonisation call, pointers aside (the contract is in include/descriptools_hip.h).
int dt_check_polygonize(int64_t H, int64_t W, int64_t cap_edges, int64_t cap_vertices, int64_t cap_rings) {
  DT_REQUIRE(H >= 1 && W >= 1, "empty raster shape");
  DT_REQUIRE(H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31), "raster of 2^31 cells or more");
  DT_REQUIRE(cap_edges >= 0 && cap_edges < (1ll << 31), "cap_edges must be in [0, 2^31) edges");
  DT_REQUIRE(cap_vertices >= 0 && cap_vertices < (1ll << 31), "cap_vertices must be in [0, 2^31) vertices");
  DT_REQUIRE(cap_rings >= 0 && cap_rings < (1ll << 31), "cap_rings must be in [0, 2^31) rings");
  return DT_OK;
}

size_t dt_polygonize_scratch(int64_t H, int64_t W, int64_t cap_edges, int count_only) {
  return PgScratch(nullptr, H, W, count_only ? 0 : cap_edges, count_only != 0).bytes;
}

// Arguments that have passed dt_check_polygonize.  info: int64[8] on the device.  scratch: dt_polygonize_scratch(H, W,
// cap_edges, count_only) bytes.  count_only: the count phase alone (cap_edges = 0 will do): info[0] = edges, info[1] = corners.  ev:
// NULL, or 8 events recorded around the seven phases (count, link, leaders, ranks, rings, emit, shells).  Nothing
// synchronises, nothing is allocated.
int dt_launch_polygonize(hipStream_t s, const int32_t *labels, int64_t H, int64_t W, int64_t cap_edges,
                         int64_t cap_vertices, int64_t cap_rings, int count_only, void *scratch, size_t scratch_bytes,
                         double *coords, int64_t *parts, int32_t *ids, int32_t *shell, int64_t *info, hipEvent_t *ev) {
  const PgScratch ws(scratch, H, W, count_only ? 0 : cap_edges, count_only != 0);
  DT_REQUIRE(scratch && scratch_bytes >= ws.bytes, "scratch too small");
  const PgGrid g{labels, (int)H, (int)W};
  const int64_t N = H * W, NV = H * (W + 1);
  const dim3 b(256);
  const dim3 cells4((unsigned)((N + PG_BLOCK - 1) / PG_BLOCK)), cells((unsigned)((N + 255) / 256));
  const dim3 verts4((unsigned)((NV + PG_BLOCK - 1) / PG_BLOCK));
  const dim3 per_edge(dt_capped_grid(cap_edges > 0 ? cap_edges : 1, PG_GRID));
  const dim3 per_ring(dt_capped_grid(cap_rings > 0 ? cap_rings : 1, PG_GRID));
  const dim3 per_ring_wave(dt_capped_grid(cap_rings > 0 ? cap_rings * 64 : 1, PG_GRID));
  int e = 0;
#define PG_MARK() \
  do { if (ev) DT_HIP(hipEventRecord(ev[e++], s)); } while (0)
  PG_MARK();
  DT_HIP(hipMemsetAsync(info, 0, 8 * sizeof(int64_t), s));
  DT_HIP(hipMemsetAsync(ws.ctl, 0, 3 * PG_CTL * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_pg_count, cells4, b, 0, s, g, N, ws.bs0, ws.bs1);
  hipLaunchKernelGGL(k_pg_scan, dim3(1), b, 0, s, ws.bs0, ws.bs1, (int64_t)cells4.x, 0,
                     count_only ? (int64_t)1 << 62 : cap_edges, count_only ? (int64_t)1 << 62 : cap_vertices, info);
  PG_MARK();
  if (count_only) return DT_OK;
  hipLaunchKernelGGL(k_pg_offsets, cells4, b, 0, s, g, N, ws.bs0, ws.celloff, info);
  hipLaunchKernelGGL(k_pg_link, cells, b, 0, s, g, N, ws.celloff, ws.words0, cap_edges, info);
  PG_MARK();
  uint64_t *buf[2] = {ws.words0, ws.words1};
  const int rounds = dt_doubling_rounds(cap_edges);  // <= 32 < PG_CTL
  for (int r = 1; r <= rounds; r++)  // round r reads buf[(r - 1) & 1]; the keys of a quiet round's two buffers agree
    hipLaunchKernelGGL(k_pg_min, per_edge, b, 0, s, buf[(r - 1) & 1], buf[r & 1], info, ws.ctl, r);
  PG_MARK();
  hipLaunchKernelGGL(k_pg_rank_init, cells, b, 0, s, g, N, ws.celloff, ws.words0, ws.words1, ws.lead, cap_edges, info);
  for (int r = 1; r <= rounds; r++)  // round r reads buf[r & 1]: after the quiet round both buffers hold the ranks
    hipLaunchKernelGGL(k_pg_rank, per_edge, b, 0, s, buf[r & 1], buf[(r - 1) & 1], info, ws.ctl + PG_CTL, r);
  PG_MARK();
  // the ranks are read from words0 from here on; words1 holds the same and gives its room to the rings of the leaders
  uint32_t *ringof = (uint32_t *)ws.words1;
  hipLaunchKernelGGL(k_pg_ring_count, verts4, b, 0, s, g, NV, ws.celloff, ws.lead, ws.words0, ws.bs0, ws.bs1, info);
  hipLaunchKernelGGL(k_pg_scan, dim3(1), b, 0, s, ws.bs0, ws.bs1, (int64_t)verts4.x, 1, cap_rings, cap_vertices, info);
  hipLaunchKernelGGL(k_pg_rings, verts4, b, 0, s, g, NV, ws.celloff, ws.lead, ws.words0, ws.bs0, ws.bs1, ringof,
                     cap_rings, parts, ids, shell, info);
  PG_MARK();
  hipLaunchKernelGGL(k_pg_emit, cells, b, 0, s, g, N, ws.celloff, ws.lead, ws.words0, ringof, parts, cap_vertices,
                     coords, info);
  PG_MARK();
  hipLaunchKernelGGL(k_pg_walk, per_ring_wave, b, 0, s, g, ws.celloff, ws.lead, ringof, parts, coords, shell, info);
  const int shell_rounds = dt_doubling_rounds(cap_rings);
  for (int r = 1; r <= shell_rounds; r++)
    hipLaunchKernelGGL(k_pg_shell, per_ring, b, 0, s, shell, info, ws.ctl + 2 * PG_CTL, r);
  hipLaunchKernelGGL(k_pg_finish, dim3(1), dim3(64), 0, s, ws.ctl, rounds, shell_rounds, info);
  PG_MARK();
#undef PG_MARK
  return DT_OK;
}
