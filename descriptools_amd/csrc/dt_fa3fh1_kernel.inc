// dt_fa3fh1_kernel.inc -- flow accumulation's last tile pass + HAND's first (dt_tiles.hip), included twice: FA3_TWI 0 is
// k_fa3fh1<ND>, FA3_TWI 1 is k_fa3fh1_twi (the float32 chain's form), whose accumulation half also writes TI and MTI.
// They are pointwise in (slope, fac); the slope raster is the D8 kernel's (k_d8_slope), and a lane has each cell's
// accumulation in a register when it stores it -- so the chain has no slope + TI + MTI pass and no second read of
// dem + fac.  The lane's four slope vectors are fetched with the pass-1 counts, ahead of the entry walks; at the
// accumulation store the cell goes through what k_slope_twi evaluates from the float32 slope it stores (dt_pct_to_tan,
// sd_twi_fast, -100 where fac <= -100: the same functions on the same bits), and a cell the fast path rejects sets its
// bit in the stencil's marks (TwiOut: 256 x 16 tiles, 4 x 4 patches per lane -- a lane's four cells lie in one row of
// one patch), which k_d8_slope has initialised with the slope flags and k_slope_twi_fix consumes afterwards.  One
// text for both, through the preprocessor, so that k_fa3fh1<ND> stays the code it was instruction for instruction
// (tools/isa_compare.py).
// FA3_WALK 1 (k_fa3fh1w<ND>, k_fa3fh1w_twi; included twice more): the same accumulation half, and HAND's half as
// walks of the fed perimeter entries (fh_walk_body) instead of the tile solve -- no cache words, the last pass solves.
#if FA3_WALK
#define FA3_NAME(n) n##w
#define FA3_NAME_TWI(n) n##w_twi
#else
#define FA3_NAME(n) n
#define FA3_NAME_TWI(n) n##_twi
#endif
#if FA3_TWI
__global__ __launch_bounds__(256, 6) void FA3_NAME_TWI(k_fa3fh1)(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
#else
template <int ND>
__global__ __launch_bounds__(256, 6) void FA3_NAME(k_fa3fh1)(const uint8_t *__restrict__ fdr, const float *__restrict__ dem,
#endif
                                                  const uint8_t *__restrict__ nod4, int ldm, DtWin w, int tiles_x,
                                                  const unsigned long long *__restrict__ rec,
                                                  const unsigned long long *__restrict__ state,
                                                  const unsigned long long *__restrict__ ext,
                                                  const uint16_t *__restrict__ loc16, int32_t *__restrict__ acc32,
                                                  int32_t river_thr, int8_t *__restrict__ river,
                                                  int *__restrict__ status, uint32_t nnodes,
                                                  unsigned long long *__restrict__ nodes,
                                                  unsigned long long *__restrict__ cache,
#if FA3_TWI
                                                  uint8_t *__restrict__ cache_wide, TwiOut tw) {
  constexpr int ND = 2;  // nodata from the D8 kernel's mask (the single raster of the float32 chain)
#else
                                                  uint8_t *__restrict__ cache_wide) {
#endif
#undef FA3_NAME
#undef FA3_NAME_TWI
#define P3(c) ((uint32_t)(c) + (((uint32_t)(c) >> 6) << 2))
#define NT3 (TH * (TW + 4))
  __shared__ __attribute__((aligned(16))) unsigned char smem[NT3 * 6];  // 26112 bytes
  __shared__ unsigned long long s_in;
#if !FA3_WALK
  __shared__ int s_ovf;
#endif
  // accumulation half: delta raster + padded successor indices
  uint32_t *s_delta = reinterpret_cast<uint32_t *>(smem);
  uint16_t *s_nxt = reinterpret_cast<uint16_t *>(smem + NT3 * 4);
  const int tile = dt_tile_of_block((int)blockIdx.x, (int)gridDim.x);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  const uint4 v_fdr = dt_tile_fetch16(fdr, w, y0, x0);
  uint32_t c2[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // see k_fa_tile3
  if (rec) fa_nbr_codes(fdr, w, y0, x0, threadIdx.x, c2);
  unsigned long long e = 0ull;
  if (threadIdx.x < PS && ext) e = ext[(size_t)tile * PS + threadIdx.x];
  constexpr int VPT = NT / 4 / 256;
  uint2 l4[VPT];
  float4 z4[VPT];
#if FA3_TWI
  fa_v4f s4[VPT];  // the cells' slopes: in flight with the counts, behind the staging and the entry walks
#endif
#pragma unroll
  for (int u = 0; u < VPT; u++) {
    int c = 4 * (threadIdx.x + 256 * u);
    int y = y0 + c / TW;
    l4[u] = *reinterpret_cast<const uint2 *>(loc16 + (size_t)tile * NT + c);
    z4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
#if FA3_TWI
    s4[u] = (fa_v4f){0.f, 0.f, 0.f, 0.f};
    if (y < w.H)
      s4[u] = __builtin_nontemporal_load(reinterpret_cast<const fa_v4f *>(tw.slope + (long long)y * w.ld + x0 + c % TW));
#endif
    if (ND == 1 && y < w.H) z4[u] = *reinterpret_cast<const float4 *>(dem + (long long)y * w.ld + x0 + c % TW);
    if (ND == 2 && y < w.H) {  // the four cells' bits, turned into the sentinel where set: finish() tests z <= -100
      const uint32_t m = (uint32_t)reinterpret_cast<const uint16_t *>(nod4)[(long long)(y >> 2) * ldm + ((x0 + c % TW) >> 2)] >>
                         (4 * (y & 3));
      z4[u] = make_float4((m & 1u) ? DT_NODATA : 0.f, (m & 2u) ? DT_NODATA : 0.f, (m & 4u) ? DT_NODATA : 0.f,
                          (m & 8u) ? DT_NODATA : 0.f);
    }
  }
  // successor indices of the 16 cells whose codes this lane fetched (row t / 4, columns 16 (t % 4) ..): straight from
  // its registers, the padded row is contiguous -- four 8-byte stores of indices, four 16-byte stores of zeros
  {
    const int ly = (int)threadIdx.x >> 2, lxb = ((int)threadIdx.x & 3) * 16;
    const uint32_t cv[4] = {v_fdr.x, v_fdr.y, v_fdr.z, v_fdr.w};
    const bool interior = dt_tile_interior(w, y0, x0);
    const int pbase = ly * (TW + 4) + lxb;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t nn[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t code = (cv[q] >> (8 * k)) & 0xFFu;
        const int lx = lxb + 4 * q + k;
        const uint32_t n = interior ? dt_tile_next_interior(code, ly, lx) : dt_tile_next(code, ly, lx, y0, x0, w);
        nn[k] = n < NT ? P3(n) : n;
      }
      *reinterpret_cast<uint2 *>(&s_nxt[pbase + 4 * q]) = make_uint2(nn[0] | (nn[1] << 16), nn[2] | (nn[3] << 16));
      *reinterpret_cast<uint4 *>(&s_delta[pbase + 4 * q]) = make_uint4(0, 0, 0, 0);
    }
  }
  // the feeders' words have been in flight behind the staging
  if (rec) e = fa_inflow(fa_gather(c2, y0, x0, threadIdx.x, tiles_x, rec, state), e);
#if FA3_WALK
  // fed: some neighbour outside the tile points back at this perimeter cell (the launcher takes this form only with
  // the gathered inflow, rec != NULL, so the codes are loaded) -- from the codes, not from the inflow's value
  // (kept as the wave's ballot, in scalar registers: the accumulation half has no vector register to spare)
  bool fed_now = false;
#pragma unroll
  for (int q = 0; q < 8; q++) fed_now = fed_now || c2[q] == fa_back(q);
  const unsigned long long fed_mask = __ballot(fed_now);
#endif
#if !FA3_WALK
  if (threadIdx.x == 0) s_ovf = 0;
#endif
  // (its barrier also publishes the staging)
  if (__syncthreads_or(!(e & FA_CYCLE) && FA_VALUE(e) >= (1ull << 22))) {  // see k_fa_tile3
    if (threadIdx.x == 0) s_in = 0ull;
    __syncthreads();
    if (e != 0ull && !(e & FA_CYCLE)) atomicAdd(&s_in, FA_VALUE(e));
    __syncthreads();
    if (threadIdx.x == 0 && s_in >= (1ull << 31) - (unsigned long long)NT && status) atomicOr(status, DT_STATUS_ACC_OVERFLOW);
  }
  if (e != 0ull) {
    int ly, lx;
    dt_cell_of_slot(threadIdx.x, ly, lx);
    uint32_t c = P3(ly * TW + lx);
    if (e & FA_CYCLE) {
      for (int it = 0; it < NT && c < NT3; it++) {
        atomicOr(&s_delta[c], 0x80000000u);
        c = s_nxt[c];
      }
    } else {
      const uint32_t add = (uint32_t)e;
      for (int it = 0; it < NT && c < NT3; it++) {
        atomicAdd(&s_delta[c], add);
        c = s_nxt[c];
      }
    }
  }
  __syncthreads();
  auto finish = [&](uint32_t l16, uint32_t d, float z) -> int32_t {
    int32_t v = l16 == 0xFFFFu ? -100 : (int32_t)l16;
    if (v != -100) v += (int32_t)(d & 0x7FFFFFFFu);
    if (d & 0x80000000u) v = -100;
    if (ND != 0 && z <= DT_NODATA) v = -100;
    return v;
  };
  uint32_t riv4[VPT];  // the river mask of the lane's 4 x 4 cells, one byte per cell
#pragma unroll
  for (int u = 0; u < VPT; u++) {
    int c = 4 * (threadIdx.x + 256 * u);
    int y = y0 + c / TW;
    riv4[u] = 0u;
    if (y >= w.H) continue;
    long long o = (long long)y * w.ld + x0 + c % TW;
    uint4 d = *reinterpret_cast<const uint4 *>(&s_delta[P3(c)]);
    int4 v = make_int4(finish(l4[u].x & 0xFFFFu, d.x, z4[u].x), finish(l4[u].x >> 16, d.y, z4[u].y),
                       finish(l4[u].y & 0xFFFFu, d.z, z4[u].z), finish(l4[u].y >> 16, d.w, z4[u].w));
    *reinterpret_cast<int4 *>(acc32 + o) = v;
    riv4[u] = (v.x > river_thr ? 1u : 0u) | (v.y > river_thr ? 0x100u : 0u) | (v.z > river_thr ? 0x10000u : 0u) |
              (v.w > river_thr ? 0x1000000u : 0u);
    *reinterpret_cast<uint32_t *>(river + o) = riv4[u];
#if FA3_TWI
    {  // what k_slope_twi evaluates from the float32 slope it stores, on the accumulation just stored
      const int32_t fv[4] = {v.x, v.y, v.z, v.w};
      const double nlnpx2 = tw.n_top * tw.lnpx2;
      fa_v4f tio, mtio;
      uint32_t rej = 0u;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float q = dt_pct_to_tan(s4[u][k]);
        const bool tnod = fv[k] <= -100;  // topoindexes.py:252
        float tv, mv;
        rej |= ((sd_twi_fast(fv[k], q, tw.n_top, tw.lnpx2, nlnpx2, tv, mv) && !tnod) ? 1u : 0u) << k;
        tio[k] = tnod ? DT_NODATA : tv;
        mtio[k] = tnod ? DT_NODATA : mv;
      }
      __builtin_nontemporal_store(tio, reinterpret_cast<fa_v4f *>(tw.ti + o));
      __builtin_nontemporal_store(mtio, reinterpret_cast<fa_v4f *>(tw.mti + o));
      if (rej) {  // ~1e-7 of the cells of a terrain raster, many of a rough one: the cell's bit in the stencil's marks
        const int x = x0 + c % TW;
        const int stile = (y >> 4) * tw.stiles_x + (x >> 8);
        const size_t lane = (size_t)stile * 256 + (size_t)(((y & 15) >> 2) * 64 + ((x & 255) >> 2));
        atomicOr(&tw.lane_mask[lane >> 1], rej << (16 * (int)(lane & 1) + 4 * (y & 3)));
        tw.tile_mark[stile] = (uint8_t)1;
      }
    }
#endif
  }
#if FA3_WALK
  // river cells end HAND's walks: terminals of the successor table (the accumulation walks are over)
#pragma unroll
  for (int u = 0; u < VPT; u++) {
    if (!riv4[u]) continue;
    const uint32_t pc = P3(4 * (threadIdx.x + 256 * u));
    uint2 nx = *reinterpret_cast<const uint2 *>(&s_nxt[pc]);
    if (riv4[u] & 0x1u) nx.x = (nx.x & 0xFFFF0000u) | NX_RIVER;
    if (riv4[u] & 0x100u) nx.x = (nx.x & 0xFFFFu) | (NX_RIVER << 16);
    if (riv4[u] & 0x10000u) nx.y = (nx.y & 0xFFFF0000u) | NX_RIVER;
    if (riv4[u] & 0x1000000u) nx.y = (nx.y & 0xFFFFu) | (NX_RIVER << 16);
    *reinterpret_cast<uint2 *>(&s_nxt[pc]) = nx;
  }
#endif
  __syncthreads();  // everybody is done with the delta raster (and the river cells are in the table)
#if FA3_WALK
  fh_walk_body(s_nxt, fdr, ((fed_mask >> (threadIdx.x & 63u)) & 1ull) != 0ull, w, tile, tiles_x, y0, x0, nodes, cache_wide);
#undef P3
#undef NT3
}
#else
#undef P3
#undef NT3
  uint32_t *s_w = reinterpret_cast<uint32_t *>(smem);             // 16 KiB
  uint8_t *s_fdr = smem + NT * 4;                                  // 4 KiB
  uint8_t *s_kind = smem + NT * 5;                                 // 4 KiB: first the river mask, then the end kinds
  uint32_t *s_lut = reinterpret_cast<uint32_t *>(smem + NT * 6);   // 1 KiB of the 1.5 KiB left
  s_lut[threadIdx.x] = fh_lut_entry(threadIdx.x);
  dt_tile_put16(s_fdr, v_fdr);
  __syncthreads();
  fh_tile1n_body(s_fdr, s_w, s_kind, &s_ovf, s_lut, riv4, w, tile, tiles_x, y0, x0, nnodes, nodes, cache, cache_wide);
}
#endif
