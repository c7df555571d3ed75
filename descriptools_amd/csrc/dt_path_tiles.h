// dt_path_tiles.h -- the tile scaffold of the operators that follow D8 paths: drainage targets and upslope length
// (dt_watershed.hip), flow-path extremes and path sums (dt_flowpath.hip).  Here: the definition of the drainage graph,
// the tile geometry, the perimeter node graph and its two kinds of node round, the workspace and the host sequence.
// What differs between the operators stays in their files: the word format, the in-tile fold and the payload.
//
// The graph (pt_classify IS its definition).  c -> d when c's code is one of the eight D8 codes, d lies in the raster
// and (with a DEM) neither c nor d is nodata (dem <= -100).  A valid cell with no edge is a terminal.  With a stop
// raster (pour > 0, stop != 0) a path ends at its first stop cell and a terminal is an end that is no stop (NOEND);
// without one the terminals are the stop cells.
//
// Tiles.  64 x 64 cells, one workgroup of 256 lanes per tile, 16 cells per lane (cell l = k * 256 + lane).  A cell
// starts as a kind and a local pointer.  PTR: the pointer is the successor, inside the tile.  STOP / EXIT / FAIL /
// NOEND: the path's end inside the tile (a stop cell; a cell whose successor lies in another tile; nodata or outside
// the raster; a terminal of a call with a stop raster), pointing at itself.  The operator resolves its words in LDS by
// pointer doubling: while a word is PTR its pointer after round r is the 2^r-th successor; an acyclic in-tile path
// makes < 4096 moves, so 12 rounds resolve it, and a word still PTR after 12 rounds is on or drains into an in-tile
// D8 cycle.
//
// Nodes.  Only the 252 perimeter cells of a tile enter a global graph: node = tile * 256 + slot (pt_slot).  An exit
// cell's node points at its successor's node -- that move is its own -- and any other perimeter cell's at the node of
// the exit its in-tile path reaches (pt_exit_successor, pt_exit_own).  Node ids travel in 31 bits (bit 31 of a pointer
// word says "resolved"), so pt_begin refuses a raster of 2^31 nodes or more.
//
// Node rounds.  Between the two tile passes run R = max(2, ceil(log2 N) + 1) launches of one of two kinds.
//   record round   (k_dr_node; fp_dn_round under k_fp_dn_node and k_ps_dn_node: the same round written for two
//     payloads, because a shared body did not compile to their code)  A node's record {pointer, tag, payload} is 16
//     bytes, more than one atomic word, so the rounds ping-pong between two buffers: each reads one and writes the
//     other, with no inter-workgroup protocol, and a cycle never reads a half-updated record.  pointer < 2^31: a
//     node further down the path; PT_RES set: resolved (PT_FAILP: to no value).  tag = the round that resolved the
//     record (-1: pass 1); a record resolved in round r is written again in round r + 1 and then skipped: both buffers
//     hold it.  flags[r + 1] is raised when round r leaves a record open; a round whose predecessor's predecessor left
//     none returns at once, and both buffers are complete by then.
//   scatter round  (pt_scatter_round: upslope length, the upslope extreme)  The nodes form a forest of exact pointers
//     (the node 2^r node-moves down, PT_NONE past a root).  A round sends S(n) -- plus the weight of the pointer, where
//     one travels -- to S(ptr(n)) by an atomic max on one global 64-bit word (one word, so no fence:
//     cdna_hip_programming.md Guideline 16; a max is idempotent and monotone, so S is updated in place) and doubles the
//     pointer into the other buffer.  flags[r + 1] is raised when a pointer is left; a round whose predecessor left
//     none returns at once.
// Why R.  After round r an open record or pointer spans 2^(r+1) node-moves, each at least one move.  A path of >= N
// moves has repeated a cell, so after ceil(log2 N) rounds everything still open lies on or drains into a cycle:
// drainage closes such a record as "no target" when its counts reach N, a max has by then seen the whole cycle (a
// node path that repeats no node is shorter than N <= 2^(R-1)), and a sum that never stops is discarded.  The round
// after that writes what the last one resolved into the other buffer, and the floor of 2 does the same for what pass 1
// and round 0 resolved.  So both record buffers are complete after R rounds for drainage, and the one the last round
// wrote, rec[R & 1], is what the last tile pass reads for every operator.
#pragma once
#include <algorithm>

#include "dt_kernels.h"

#define PT_T 64        // tile edge
#define PT_CPT 16      // cells per lane
#define PT_SLOTS 256   // node ids per tile (252 perimeter cells)
#define PT_ROUNDS 12   // in-tile doubling rounds
#define PT_K_PTR 0u
#define PT_K_STOP 1u
#define PT_K_EXIT 2u
#define PT_K_FAIL 3u
#define PT_K_NOEND 4u
#define PT_NONE 0xFFFFFFFFu   // scatter rounds: no pointer
#define PT_RES 0x80000000u    // record rounds: the pointer word of a resolved record has this bit
#define PT_FAILP 0xFFFFFFFFu  // ... resolved to no value

// ---- geometry ----------------------------------------------------------------------------------------------------
// perimeter slot of a local cell (-1 inside): row 0, row 63, column 0, column 63; and the local cell of slot j < 252
__device__ __forceinline__ int pt_slot(int ly, int lx) {
  if (ly == 0) return lx;
  if (ly == PT_T - 1) return 64 + lx;
  if (lx == 0) return 127 + ly;
  if (lx == PT_T - 1) return 189 + ly;
  return -1;
}
__device__ __forceinline__ int pt_slot_cell(int j) {
  if (j < 64) return j;
  if (j < 128) return (PT_T - 1) * PT_T + (j - 64);
  if (j < 190) return (j - 127) * PT_T;
  return (j - 189) * PT_T + PT_T - 1;
}
__device__ __forceinline__ uint32_t pt_node(int64_t y, int64_t x, int64_t TX) {
  return (uint32_t)(((y >> 6) * TX + (x >> 6)) * PT_SLOTS + pt_slot((int)(y & 63), (int)(x & 63)));
}
struct PtTile {
  int64_t ty, tx, y0, x0;
};
__device__ __forceinline__ PtTile pt_tile(int64_t TX) {  // the tile of this workgroup
  PtTile T;
  T.ty = (int64_t)blockIdx.x / TX;
  T.tx = (int64_t)blockIdx.x - T.ty * TX;
  T.y0 = T.ty * PT_T;
  T.x0 = T.tx * PT_T;
  return T;
}

// ---- the graph ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pt_stops(const int64_t *pour, int64_t c) { return pour[c] > 0; }
__device__ __forceinline__ bool pt_stops(const uint8_t *stop, int64_t c) { return stop[c] != 0; }
// How local cell l of the tile at (y0, x0) starts: its kind, its pointer (the successor's local cell when PTR, else
// the cell itself) and whether its move is diagonal (PTR, EXIT), handed to pack(kind, pointer, diagonal), which makes
// the operator's word of them.  dem and stop may be NULL.  The order of the tests is the definition.
template <typename STOP, class Pack>
__device__ __forceinline__ auto pt_classify(const uint8_t *fdr, const float *dem, const STOP *stop, int64_t H,
                                            int64_t W, int64_t y0, int64_t x0, int l, Pack pack) {
  const uint32_t self = (uint32_t)l;
  const int64_t y = y0 + (l >> 6), x = x0 + (l & 63);
  if (y >= H || x >= W) return pack(PT_K_FAIL, self, false);
  const int64_t c = y * W + x;
  if (dem && dem[c] <= -100.0f) return pack(PT_K_FAIL, self, false);
  if (stop && pt_stops(stop, c)) return pack(PT_K_STOP, self, false);
  const uint32_t term = stop ? PT_K_NOEND : PT_K_STOP;
  const uint32_t code = fdr[c];
  if (!dt_d8_valid(code)) return pack(term, self, false);
  int dy, dx;
  dt_d8_delta(code, dy, dx);
  const int64_t ny = y + dy, nx = x + dx;
  if (ny < 0 || ny >= H || nx < 0 || nx >= W) return pack(term, self, false);
  if (dem && dem[ny * W + nx] <= -100.0f) return pack(term, self, false);
  const int64_t ly = ny - y0, lx = nx - x0;
  const bool diag = dy != 0 && dx != 0;
  if (ly < 0 || ly >= PT_T || lx < 0 || lx >= PT_T) return pack(PT_K_EXIT, self, diag);
  return pack(PT_K_PTR, (uint32_t)(ly * PT_T + lx), diag);
}

// ---- perimeter ---------------------------------------------------------------------------------------------------
// One perimeter slot per lane: this lane's cell of tile T (local index, position); false for the lanes 252-255 and for
// a cell outside the raster.
__device__ __forceinline__ bool pt_lane_cell(const PtTile &T, int64_t H, int64_t W, int &l, int64_t &y, int64_t &x) {
  const int t = (int)threadIdx.x;
  bool inside = false;
  if (t < 252) {
    l = pt_slot_cell(t);
    y = T.y0 + (l >> 6);
    x = T.x0 + (l & 63);
    inside = y < H && x < W;
  }
  return inside;
}
// The node pointer of a perimeter cell whose resolved word is EXIT with pointer p.  The exit cell itself (p is the
// cell) points at its successor's node, and that move -- diagonal or not -- is its record's: pt_exit_successor of its
// code.  Any other cell points at the own tile's node of the exit at p, and the moves up to it are in the cell's word:
// pt_exit_own.
__device__ __forceinline__ uint32_t pt_exit_successor(uint32_t code, int64_t TX, int64_t y, int64_t x, bool &diag) {
  int dy, dx;
  dt_d8_delta(code, dy, dx);
  diag = dy != 0 && dx != 0;
  return pt_node(y + dy, x + dx, TX);
}
__device__ __forceinline__ uint32_t pt_exit_own(uint32_t p) {
  return (uint32_t)(blockIdx.x * PT_SLOTS + pt_slot((int)(p >> 6), (int)(p & 63)));
}

// ---- node rounds -------------------------------------------------------------------------------------------------
// One scatter round.  fold.send(&S(p), sv, w): sv = S(n) (+ w) goes to S(p); WEIGHT: a weight w travels with the
// pointer and doubles with it by fold.join(w(n), w(p)).
template <bool WEIGHT, class Fold>
__device__ __forceinline__ void pt_scatter_round(const uint32_t *psrc, uint32_t *pdst, const unsigned long long *wsrc,
                                                 unsigned long long *wdst, unsigned long long *S, int64_t NN,
                                                 uint32_t *flags, int r, Fold fold) {
  if (r > 0 && flags[r] == 0u) return;
  bool pend = false;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < NN; n += (int64_t)gridDim.x * 256) {
    const uint32_t p = psrc[n];
    if (p == PT_NONE) {
      pdst[n] = PT_NONE;
      continue;
    }
    unsigned long long w = 0ull;
    if constexpr (WEIGHT) w = wsrc[n];
    const unsigned long long sv = __hip_atomic_load(&S[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    fold.send(&S[p], sv, w);
    const uint32_t p2 = psrc[p];
    pdst[n] = p2;
    if constexpr (WEIGHT) {
      if (p2 != PT_NONE) {
        wdst[n] = fold.join(w, wsrc[p]);
        pend = true;
      }
    } else {
      pend |= p2 != PT_NONE;
    }
  }
  if (__ballot(pend) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(&flags[r + 1], 1u);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The workspace of one fold: the flag block, then the record pair (PT_BUF_REC) or the pointer pair, with a weight pair
// beside it (PT_BUF_PTR_WEIGHT), and the value words S.  An operator may carve planes of its own behind them.
enum { PT_BUF_REC = 0, PT_BUF_PTR = 1, PT_BUF_PTR_WEIGHT = 2 };
struct PtLayout {
  int64_t TY, TX, NN;
  int flag_words;
  uint32_t *flags;
  uint4 *rec[2];
  uint32_t *uptr[2];
  unsigned long long *uw[2], *S;
  size_t bytes;
};
static PtLayout pt_layout(DtCarver &c, int64_t H, int64_t W, int buffers, int flag_words = 64) {
  PtLayout L = {};
  L.TY = (H + PT_T - 1) / PT_T;
  L.TX = (W + PT_T - 1) / PT_T;
  L.NN = L.TY * L.TX * PT_SLOTS;
  L.flag_words = flag_words;
  L.flags = c.take<uint32_t>((size_t)flag_words);
  for (int i = 0; i < 2; i++) {
    if (buffers == PT_BUF_REC) L.rec[i] = c.take<uint4>((size_t)L.NN);
    if (buffers != PT_BUF_REC) L.uptr[i] = c.take<uint32_t>((size_t)L.NN);
    if (buffers == PT_BUF_PTR_WEIGHT) L.uw[i] = c.take<unsigned long long>((size_t)L.NN);
  }
  if (buffers != PT_BUF_REC) L.S = c.take<unsigned long long>((size_t)L.NN);
  L.bytes = c.bytes();
  return L;
}
// The start of a launcher: R = the node rounds to run, 0 for an empty raster (nothing to do); the flags are cleared.
static int pt_begin(hipStream_t s, const PtLayout &L, int64_t H, int64_t W, size_t scratch_bytes, int &R) {
  R = 0;
  if (H == 0 || W == 0) return DT_OK;
  DT_REQUIRE(scratch_bytes >= L.bytes, "scratch too small");
  DT_REQUIRE(L.NN < (1ll << 31), "too many tiles: node ids travel in 31 bits");
  DT_HIP(hipMemsetAsync(L.flags, 0, sizeof(uint32_t) * (size_t)L.flag_words, s));
  R = std::max(2, dt_doubling_rounds(H * W));
  return DT_OK;
}
// Pass 1, R node rounds that ping-pong, pass 3: pass1(tile grid, block), round(node grid, block, r, source buffer,
// destination buffer), pass3(tile grid, block, the buffer the last round wrote).
template <class Pass1, class Round, class Pass3>
static void pt_launch_passes(const PtLayout &L, int R, Pass1 pass1, Round round, Pass3 pass3) {
  const dim3 b(256), gt((unsigned)(L.TY * L.TX)), gn(dt_capped_grid(L.NN, 8192));
  pass1(gt, b);
  for (int r = 0; r < R; r++) round(gn, b, r, r & 1, (r & 1) ^ 1);
  pass3(gt, b, R & 1);
}
