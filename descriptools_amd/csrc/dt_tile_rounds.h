// dt_tile_rounds.h -- the schedule of a tile-wise fixed-point iteration: which tiles a round visits and in which
// order, what a visit leaves behind, and the scaffold of the ops that run on it.
//
// The protocol.  The raster is cut into square tiles (the op's size) coloured 2 x 2, and a ROUND is four launches, one
// per colour, one workgroup per tile of that colour.
//   activity bytes  One byte per tile, ONE array used in place.  A visit leaves HY_CHANGED -- the tile's cells changed,
//                   the eight tiles around it have a new halo to look at -- and HY_OPEN -- the visit was cut short, the
//                   tile must be visited again whatever its neighbours do (an op may keep further bits above these).  A
//                   round visits the tiles that are open or have a changed NEIGHBOUR; a workgroup whose tile rests
//                   clears the tile's byte and leaves.  act_prev == NULL: every tile is visited.
//   flag words      One int per round, cleared by the launcher.  A round raises its word when it changed anything; the
//                   launches of a round whose predecessor's word is still 0 return at once, so a batch of rounds is
//                   enqueued without a host synchronisation and the host reads the flags of the batch afterwards.
//   start           The first launcher call of an op's call: it clears the visit counters, and its first round visits
//                   every tile (the activity bytes hold nothing yet).  A later call carries on from the bytes in place.
//   visits          One counter per tile, a diagnostic.  Only the workgroup that visits a tile adds to its word, and
//                   only one workgroup per launch has that tile: no atomics.  The op's finish kernel sums them.
// Users: the conditioning rounds (dt_hydro.hip: the three helpers below, with a window, an uncoloured form and ping-pong
// activity arrays of their own), and on the scaffold (HyRound, hy_round_enter / _leave, hy_visits_sum, HyRoundsScratch,
// hy_launch_rounds) the D-infinity distance (dt_dinf_dist.hip), the cost distance (dt_cost.hip), the modified catchment
// area (dt_wetness.hip), the geodesic reconstruction (dt_morphology.hip) and the harmonic smoother (dt_harmonic.hip: its
// rounds end on a residual key, not a flag, so it has its own round loop around hy_launch_colours).  The host tier's batches are host_tile_rounds in dt_capi.hip.
#pragma once
#include "dt_common.h"

// (HY_CHANGED, since round 4 of the conditioning work: only when a cell of the tile's OUTER RING changed -- what its
// neighbours read.  With one round of sweeps per visit -- the measured optimum, HY_FILL_SWEEPS -- a tile that changed
// is open: round 3's rule.)
#define HY_CHANGED 1
#define HY_OPEN 2
// COLOURED rounds (round 4).  A round that visits all tiles at once reads, in every tile, what the neighbours held
// BEFORE the round: a front moves one tile per round.  The tiles are coloured 2 x 2 (colour = 2 * (row & 1) + (column &
// 1): all eight neighbours of a tile have other colours) and a round is four launches, one colour each: a tile sees what
// the colours before it did in this very round, and a front that crosses tile borders moves two tiles per round for the
// same number of tile visits -- rough 16384^2 terrain: 16 -> 9 fill rounds, 12 -> 7 flat rounds.  The activity flags
// live in ONE array used in place: when a tile of colour c is visited, every neighbour's latest visit lies after the
// tile's own previous one, so the flags it reads are exactly the changes it has not seen yet, and nobody writes them
// during this launch.  colour < 0: every tile (the first round of the fill, which initialises the surface).
__device__ __forceinline__ void hy_tile_of_block(int colour, int tiles_x, int &ty, int &tx) {
  if (colour < 0) {
    ty = (int)blockIdx.x / tiles_x;
    tx = (int)blockIdx.x - ty * tiles_x;
  } else {
    const int cx = (tiles_x - (colour & 1) + 1) >> 1;  // tiles of this colour in a row of tiles
    const int i = (int)blockIdx.x / cx, j = (int)blockIdx.x - i * cx;
    ty = 2 * i + (colour >> 1);
    tx = 2 * j + (colour & 1);
  }
}
// workgroups of a launch over the tiles of one colour
static unsigned hy_colour_blocks(int colour, int tiles_x, int tiles_y) {
  if (colour < 0) return (unsigned)(tiles_x * tiles_y);
  return (unsigned)(((tiles_x - (colour & 1) + 1) >> 1) * ((tiles_y - (colour >> 1) + 1) >> 1));
}
// centre: the bits of the tile's own byte that count (its neighbours' HY_CHANGED always does)
__device__ __forceinline__ bool hy_tile_active(const uint8_t *__restrict__ act_prev, int ty, int tx, int tiles_x,
                                               int tiles_y, int centre = HY_OPEN) {
  if (!act_prev) return true;
  int v = 0;
  if (threadIdx.x < 9) {
    const int y = ty + (int)threadIdx.x / 3 - 1, x = tx + (int)threadIdx.x % 3 - 1;
    if (y >= 0 && y < tiles_y && x >= 0 && x < tiles_x)
      v = act_prev[(size_t)y * tiles_x + x] & (threadIdx.x == 4 ? centre : HY_CHANGED);
  }
  return __syncthreads_or(v) != 0;
}

// ---- the scaffold of a round kernel -------------------------------------------------------------------------------
// What a launch of a round knows about the schedule; the kernel takes it by value.
struct HyRound {
  int *changed;             // this round's flag word (NULL: the op ends its rounds by another test)
  const int *prev;          // the flag word of the round before (NULL: the first round of the launcher call)
  const uint8_t *act_prev;  // the activity bytes to read (NULL: every tile is visited)
  uint8_t *act_cur;         // ... and to write: the same array
  uint32_t *visits;
  int tiles_x, tiles_y, colour;
};
// The tile of this workgroup -> whether it is to be visited; a tile that rests has its byte cleared.
__device__ __forceinline__ bool hy_round_tile(const HyRound &r, int &ty, int &tx) {
  hy_tile_of_block(r.colour, r.tiles_x, ty, tx);
  if (hy_tile_active(r.act_prev, ty, tx, r.tiles_x, r.tiles_y)) return true;
  if (threadIdx.x == 0) r.act_cur[ty * r.tiles_x + tx] = 0;
  return false;
}
// ... after the test of the round before (its flag was written by the previous kernel: a plain load sees it).  false:
// the workgroup has nothing to do.
__device__ __forceinline__ bool hy_round_enter(const HyRound &r, int &ty, int &tx) {
  if (r.prev && *r.prev == 0) return false;
  return hy_round_tile(r, ty, tx);
}
// The end of a visit: the tile's activity byte, the round's flag (any: the visit changed something; 0 for an op
// without flag words), the visit counter.  Every lane may call it, lane 0 writes.
__device__ __forceinline__ void hy_round_leave(const HyRound &r, int tile, int act_byte, int any) {
  if (threadIdx.x != 0) return;
  r.act_cur[tile] = (uint8_t)act_byte;
  if (any) *r.changed = 1;
  r.visits[tile] += 1u;  // (nobody else touches this tile's word during the launch)
}
// A finish kernel's share of the tile-visit sum, for a grid of 256-thread workgroups that covers the tiles (one thread
// per cell does): every thread of the workgroup calls it, one atomic per workgroup that saw a visit goes to the 64-bit
// word at ctl64 (8-byte aligned).
__device__ __forceinline__ void hy_visits_sum(const uint32_t *__restrict__ visits, int tiles, uint32_t *ctl64) {
  __shared__ uint32_t s_visits;
  if (threadIdx.x == 0) s_visits = 0u;
  __syncthreads();
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < tiles && visits[t]) atomicAdd(&s_visits, visits[t]);
  __syncthreads();
  if (threadIdx.x == 0 && s_visits) atomicAdd((unsigned long long *)ctl64, (unsigned long long)s_visits);
}

// ---- the scaffold of a launcher -----------------------------------------------------------------------------------
// The schedule's share of an op's workspace: the control words (the flag words among them), then the tile arrays.
struct HyRoundsScratch {
  uint32_t *ctl;
  uint8_t *act;
  uint32_t *visits;  // per tile: how often a workgroup staged it
  int tiles_x, tiles_y;
  size_t tiles() const { return (size_t)tiles_x * (size_t)tiles_y; }
};
// cells: a byte per cell that the op keeps between its control words and the tile arrays (the D-infinity distance's
// state raster)
static HyRoundsScratch hy_rounds_take(DtCarver &c, int64_t H, int64_t W, int tile, size_t ctl_words,
                                      uint8_t **cells = nullptr) {
  HyRoundsScratch L = {};
  L.tiles_x = (int)((W + tile - 1) / tile);
  L.tiles_y = (int)((H + tile - 1) / tile);
  L.ctl = c.take<uint32_t>(ctl_words);
  if (cells) *cells = c.take<uint8_t>((size_t)(H * W));
  L.act = c.take<uint8_t>(L.tiles());
  L.visits = c.take<uint32_t>(L.tiles());
  return L;
}
// The four launches of one round: launch(dim3 blocks, const HyRound &) issues the op's kernel for one colour.
template <typename Launch>
static void hy_launch_colours(HyRound r, Launch launch) {
  for (r.colour = 0; r.colour < 4; r.colour++) {
    const unsigned nb = hy_colour_blocks(r.colour, r.tiles_x, r.tiles_y);
    if (nb) launch(dim3(nb), r);
  }
}
// `rounds` rounds, round r raising flags[r]; start: see above (the op's own initialisation comes before the call).
template <typename Launch>
static int hy_launch_rounds(hipStream_t s, const HyRoundsScratch &L, uint32_t *flags, int start, int rounds,
                            Launch launch) {
  if (start) DT_HIP(hipMemsetAsync(L.visits, 0, sizeof(uint32_t) * L.tiles(), s));
  if (rounds) DT_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t) * (size_t)rounds, s));
  for (int r = 0; r < rounds; r++) {
    int *flag = (int *)flags + r;
    hy_launch_colours(HyRound{flag, r ? flag - 1 : nullptr, (start && r == 0) ? nullptr : L.act, L.act, L.visits,
                              L.tiles_x, L.tiles_y, 0},
                      launch);
  }
  return DT_OK;
}
