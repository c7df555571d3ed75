// dt_d8_kernel.inc -- the D8 kernel of dt_stencil.hip, included twice: SD_D8_SLOPE 0 is k_d8<NT> (codes and the nodata
// mask), SD_D8_SLOPE 1 is k_d8_slope, which also writes the slope raster from the 3 x 3 neighbourhood the kernel holds
// anyway -- sd_slope_fast, its flag and the nodata rule exactly as k_slope_twi applies them (the float32 chain's first
// kernel: the chain then has no slope + TI + MTI pass, TI / MTI come out of flow accumulation's last tile pass,
// k_fa3fh1_twi).  The slope flags go into marks of their own (s_mark / s_mask, k_slope_twi's layout: the tiles and the
// patches are the same), and EVERY lane's mask word is written: k_fa3fh1_twi ORs the cells its TI / MTI fast path
// rejects into them before k_slope_twi_fix redoes the union.  One text for both, through the preprocessor, so that
// k_d8 stays the code it was instruction for instruction (tools/isa_compare.py).
#if SD_D8_SLOPE
// D8 codes + nodata mask + slope (kc = 100 / px, kd = 100 / (px sqrt 2): see sd_slope_fast)
__global__ __launch_bounds__(256, 7) void k_d8_slope(const float *__restrict__ dem, DtWin w, uint8_t *__restrict__ fdr,
                                                    int tiles_x, int tiles_y, int vec_ok,
                                                    uint8_t *__restrict__ tile_mark, uint16_t *__restrict__ lane_mask,
                                                    uint8_t *__restrict__ nod4, int ldm, double kc, double kd,
                                                    float *__restrict__ slope, uint8_t *__restrict__ s_mark,
                                                    uint16_t *__restrict__ s_mask, uint32_t flag_all) {
  constexpr bool NT = false;
#else
template <bool NT>
__global__ __launch_bounds__(256, 8) void k_d8(const float *__restrict__ dem, DtWin w, uint8_t *__restrict__ fdr,
                                              int tiles_x, int tiles_y, int vec_ok, uint8_t *__restrict__ tile_mark,
                                              uint16_t *__restrict__ lane_mask, uint8_t *__restrict__ nod4, int ldm) {
#endif
  __shared__ __attribute__((aligned(16))) float t[(SD_TY + 2) * SD_LDW];
  const int tile = sd_tile_of_block(blockIdx.x, tiles_x * tiles_y);
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int x0 = txi * SD_TX, y0 = tyi * SD_TY;
  const int H = w.H, W = w.W;
  sd_stage(t, dem, w, x0, y0, vec_ok);
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int cx = tx * 4, ry = ty * 4;
  const int gx = x0 + cx;
  auto load_row = [&](int lr, float *dst) {
    const float *row = &t[lr * SD_LDW];
    float4 m = *reinterpret_cast<const float4 *>(row + 4 + cx);
    float lh = row[3], rh = row[4 + SD_TX];
    dst[0] = sd_from_prev_lane(lh, m.w);
    dst[1] = m.x;
    dst[2] = m.y;
    dst[3] = m.z;
    dst[4] = m.w;
    dst[5] = sd_from_next_lane(rh, m.x);
  };
  const bool full = vec_ok && gx + 3 < W;
  // block-uniform: does the tile touch the border of the GLOBAL raster?  (only there does the border rule apply;
  // the kernel is limited by VALU issue and the rule is a sixth of a cell's instructions)
  const bool on_border = w.gy0 + y0 == 0 || w.gx0 + x0 == 0 || w.gy0 + y0 + SD_TY >= w.Hg || w.gx0 + x0 + SD_TX >= w.Wg;
  float a[6], bb[6], cc[6];
  load_row(ry, a);
  load_row(ry + 1, bb);
  uint32_t mask = 0, nodmask = 0;
#if SD_D8_SLOPE
  uint32_t smask = flag_all;  // test knob, as in k_slope_twi
#endif
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int gy = y0 + ry + j;
    load_row(ry + 2 + j, cc);
    uint32_t codes = 0;
#if SD_D8_SLOPE
    float so[4];
#endif
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float c = bb[k + 1];
      const bool nod = sd_centre(c) <= DT_NODATA;  // staged nodata or below the sentinel: code 0 (NaN, +inf: not)
      nodmask |= (nod ? 1u : 0u) << (4 * j + k);
#if SD_D8_SLOPE
      {  // k_slope_twi's slope: -100 on nodata (slope.py:231), flagged cells redone by k_slope_twi_fix
        float sl;
        const bool sflag = sd_slope_fast(c, a[k], a[k + 1], a[k + 2], bb[k], bb[k + 2], cc[k], cc[k + 1], cc[k + 2], kc, kd, sl);
        so[k] = nod ? DT_NODATA : sl;
        smask |= ((sflag && !nod) ? 1u : 0u) << (4 * j + k);
      }
#endif
      uint32_t code;
      bool flag = sd_d8_fast(c, a[k], a[k + 1], a[k + 2], bb[k], bb[k + 2], cc[k], cc[k + 1], cc[k + 2], code);
      if (on_border) {
        // N1 border rule: a border cell with no lower neighbour drains out of the raster
        const int gyy = w.gy0 + gy, gxx = w.gx0 + gx + k;
        const uint32_t out = gyy == w.Hg - 1 ? 4u : (gyy == 0 ? 64u : (gxx == 0 ? 16u : (gxx == w.Wg - 1 ? 1u : 0u)));
        code = code == 0u ? out : code;
      }
      codes |= (nod ? 0u : code) << (8 * k);
      mask |= ((flag && !nod) ? 1u : 0u) << (4 * j + k);
    }
    if (gy < H) {
      const long long o = (long long)gy * w.ld + gx;
      if (full) {
        if (NT) __builtin_nontemporal_store(codes, reinterpret_cast<uint32_t *>(fdr + o));
        else *reinterpret_cast<uint32_t *>(fdr + o) = codes;
#if SD_D8_SLOPE
        sd_store4(slope + o, so[0], so[1], so[2], so[3]);
#endif
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (gx + k < W) fdr[o + k] = (uint8_t)(codes >> (8 * k));
          else mask &= ~(1u << (4 * j + k));
#if SD_D8_SLOPE
          if (gx + k < W) slope[o + k] = so[k];
          else smask &= ~(1u << (4 * j + k));
#endif
        }
      }
    } else {
      mask &= ~(0xFu << (4 * j));
#if SD_D8_SLOPE
      smask &= ~(0xFu << (4 * j));
#endif
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
      a[q] = bb[q];
      bb[q] = cc[q];
    }
  }
  if (nod4 && gx < W && y0 + ry < H)
    reinterpret_cast<uint16_t *>(nod4)[(long long)((y0 + ry) >> 2) * ldm + (gx >> 2)] = (uint16_t)nodmask;
  const int any = __syncthreads_or(mask != 0u);
  if (threadIdx.x == 0) tile_mark[tile] = (uint8_t)(any != 0);
  if (any) lane_mask[(size_t)tile * 256 + threadIdx.x] = (uint16_t)mask;
#if SD_D8_SLOPE
  const int sany = __syncthreads_or(smask != 0u);
  if (threadIdx.x == 0) s_mark[tile] = (uint8_t)(sany != 0);
  s_mask[(size_t)tile * 256 + threadIdx.x] = (uint16_t)smask;  // every lane: k_fa3fh1_twi ORs into these words
#endif
}
