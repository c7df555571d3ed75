// dt_tile_rounds.h -- which tiles a round of a tile-wise fixed-point iteration visits, and in which order: the activity
// flags and the 2 x 2 colouring shared by the conditioning rounds (dt_hydro.hip) and the D-infinity distance rounds
// (dt_dinf_dist.hip).
#pragma once
#include "dt_common.h"

// Which tiles a round has to visit.  A visit makes up to `sweeps` rounds of four directional sweeps over its tile and
// leaves one byte per tile: HY_CHANGED -- its cells changed, the eight tiles around it have a new halo to look at --
// and HY_OPEN -- its last round of sweeps still moved something, so it must be visited again whatever its neighbours
// do.  A round visits the tiles that have a changed NEIGHBOUR or are open themselves; a tile at its local fixed point
// rests until its halo changes.  (With one round of sweeps per visit -- the measured optimum, HY_FILL_SWEEPS -- a
// tile that changed is open: round 3's rule.)  act_prev == NULL: the first round of a phase, every tile is visited.
#define HY_CHANGED 1 /* (round 4, late: only when a cell of the tile's OUTER RING changed -- what its neighbours read) */
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
__device__ __forceinline__ bool hy_tile_active(const uint8_t *__restrict__ act_prev, int ty, int tx, int tiles_x,
                                               int tiles_y) {
  if (!act_prev) return true;
  int v = 0;
  if (threadIdx.x < 9) {
    const int y = ty + (int)threadIdx.x / 3 - 1, x = tx + (int)threadIdx.x % 3 - 1;
    if (y >= 0 && y < tiles_y && x >= 0 && x < tiles_x)
      v = act_prev[(size_t)y * tiles_x + x] & (threadIdx.x == 4 ? HY_OPEN : HY_CHANGED);
  }
  return __syncthreads_or(v) != 0;
}
