// dt_kernels.h -- launchers implemented in dt_kernels.hip (all asynchronous on `s`).
#pragma once
#include "dt_common.h"

int dt_launch_synth_dem(hipStream_t s, uint32_t seed, int O, int64_t Hg, int64_t y0, int64_t x0,
                        int64_t h, int64_t w, int nodata_pct, float *out);
int dt_launch_stencil(hipStream_t s, const DtWin &w, const float *dem, double px, float *slope,
                      uint8_t *fdr, float *slope_rad, const void *acc, int acc64, double n_top, float *ti,
                      float *mti, void *aux = nullptr, uint8_t *nod4 = nullptr, int ldm = 0);
// the nodata mask of the D8-only kernel: one 16-bit word per 4 x 4 patch of cells (bit 4 j + k = cell (4 r + j, 4 i + k)
// is nodata), ldm words per row of patches
static inline int dt_nodata4_ld(int64_t W) { return (int)((((W + 3) / 4) + 7) & ~(int64_t)7); }
static inline size_t dt_nodata4_bytes(int64_t H, int64_t W) { return (size_t)((H + 3) / 4) * (size_t)dt_nodata4_ld(W) * 2; }
// workspace of the stencil's hot / fix-up kernel pairs and of the TI / MTI epilogue (dt_tiles.hip): a mark byte and 256
// 16-bit lane masks per 256 x 16 tile; dt_stencil_aux_bytes: for the tiles of an H x W window
struct DtStencilAux {
  uint8_t *mark;
  uint16_t *lmask;
  size_t bytes;
};
static inline DtStencilAux dt_stencil_aux_layout(int64_t ntiles, void *aux) {
  DtStencilAux a;
  DtCarver c(aux);
  a.mark = c.take<uint8_t>((size_t)ntiles);
  a.lmask = c.take<uint16_t>((size_t)ntiles * 256);
  a.bytes = c.bytes();
  return a;
}
size_t dt_stencil_aux_bytes(int64_t H, int64_t W);
// the float32 chain's D8 + slope kernel and the fix-up of the cells it and the TI / MTI epilogue marked (dt_stencil.hip)
int dt_launch_d8_slope(hipStream_t s, const DtWin &w, const float *dem, double px, uint8_t *fdr, float *slope,
                       void *aux, uint8_t *nod4, int ldm, void *smarks);
int dt_launch_slope_twi_fix(hipStream_t s, const DtWin &w, const float *dem, double px, float *slope,
                            const int32_t *acc, double n_top, float *ti, float *mti, void *smarks);
int dt_launch_flowacc(hipStream_t s, const uint8_t *fdr, const float *dem, int64_t H, int64_t W,
                      unsigned long long *state, int32_t *acc32);
int dt_launch_river_mask(hipStream_t s, const int32_t *acc32, int64_t n, int64_t thr, int8_t *river);
int dt_launch_flowhand(hipStream_t s, const float *dem, const uint8_t *fdr, const int8_t *river,
                       const int32_t *acc32, int64_t H, int64_t W, double px,
                       unsigned long long *state, float *fdist, int32_t *idx32, float *hand,
                       int32_t *a_river);
int dt_launch_twi(hipStream_t s, const int32_t *acc32, const float *srad, int64_t n, double px,
                  double n_top, float *ti, float *mti);
int dt_launch_twi_i64(hipStream_t s, const int64_t *fac, const float *srad, int64_t n, double px,
                      double n_top, float *ti, float *mti);
int dt_launch_gfi(hipStream_t s, const float *hand, const int32_t *area, int64_t n, double expo,
                  double b, double size, float *out, int own_cell);
int dt_launch_gfi_i64(hipStream_t s, const float *hand, const int64_t *area, int64_t n, double expo,
                      double b, double size, float *out, int own_cell);
int dt_launch_river_acc_i64(hipStream_t s, const int64_t *fac, const int64_t *idx, int64_t n,
                            int64_t *out);
// The long-walk workspace of a window (dt_kernels.hip, DsQueue): the QUEUE (a 256-byte counter header | one entry per
// two core cells), then the TABLES over the window's memory (two ping-pong skip tables, the 8-move table that is kept,
// which entries exist).  `work` holds both back to back; dt_launch_downslope also takes them at two addresses.
struct DtDsLift {
  uint32_t *qcount;  // walks queued: the first word of the header
  uint4 *qentries;
  uint32_t qcapacity;
  uint2 *tab[3];
  uint8_t *dom;
  size_t queue_bytes, tables_bytes, bytes;
};
DtDsLift dt_downslope_lift_layout(const DtWin &w, void *work);
size_t dt_downslope_lift_bytes(int64_t H, int64_t W);
size_t dt_downslope_queue_bytes(int64_t H, int64_t W);
size_t dt_downslope_tables_bytes(int64_t H, int64_t W);
uint32_t dt_downslope_lift_min(int64_t H, int64_t W);
size_t dt_downslope_tables_bytes_w(const DtWin &w);
size_t dt_downslope_lift_bytes_w(const DtWin &w);
int dt_launch_downslope(hipStream_t s, const DtWin &w, const float *dem, const uint8_t *fdr, double px,
                        double dz, int raw, float *out, int *n_unresolved, void *qwork = nullptr,
                        void *twork = nullptr, int phase = 0, void *walkers = nullptr, size_t walkers_bytes = 0);
int dt_launch_ds_walk(hipStream_t s, const DtWin &w, const float *dem, const uint8_t *fdr, double px, double dz,
                      int64_t n, void *rec, void *work, float *out = nullptr);
int dt_launch_ds_route(hipStream_t s, int64_t n, const void *rec, const int32_t *row_starts, int ty,
                       const int32_t *col_starts, int tx, void *send, int32_t *counts, int32_t *scratch);
int dt_launch_ds_walk_seed(hipStream_t s, const DtWin &w, const float *dem, int64_t n, const int32_t *ys,
                           const int32_t *xs, void *rec);
int dt_launch_downslope_v1(hipStream_t s, const float *dem, const uint8_t *fdr, int64_t H, int64_t W,
                           double px, double dz, int raw, float *out);
int dt_launch_hand_i64(hipStream_t s, const float *dem, const int64_t *idx, int64_t n, float *hand);
// dt_wide.hip: heights in float64
int dt_launch_slope_f64(hipStream_t s, const double *dem, int64_t H, int64_t W, double px, float *slope);
int dt_launch_hand_f64(hipStream_t s, const double *dem, const int64_t *idx, int64_t n, double *hand);
int dt_launch_downslope_f64(hipStream_t s, const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                            double dz, int raw, float *out);
int dt_launch_gfi_f64h(hipStream_t s, const double *hand, const int64_t *fac, const int64_t *idx, int64_t n,
                       double expo, double b, double size, int own_area, float *out);
// the resident chain's float64 tier: D8 + exact slope + nodata proxy and slope + TI + MTI (dt_stencil.hip), windowed
// downslope and HAND + GFI + ln(hl/H) (dt_wide.hip)
int dt_launch_d8_f64(hipStream_t s, const double *dem, int64_t H, int64_t W, double px, uint8_t *fdr, float *slope,
                     float *proxy);
int dt_launch_slope_twi_f64(hipStream_t s, const double *dem, const int32_t *acc32, int64_t H, int64_t W, double px,
                            double n_top, float *slope, float *slope_rad, float *ti, float *mti);
int dt_launch_downslope_win_f64(hipStream_t s, const double *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                                double dz, int raw, float *out);
int dt_launch_hand_gfi_f64(hipStream_t s, const double *dem, const int32_t *idx32, const int32_t *acc32, int64_t n,
                           double expo, double b, double size, double *hand, float *gfi, float *lnhlh);
// ... and on one rank's window (tiling.RankTile(heights="float64")): dt_stencil.hip, dt_wide.hip, dt_kernels.hip (walkers),
// dt_tiles.hip (the rank-level HAND solve with the float64 river height)
int dt_launch_d8_f64_w(hipStream_t s, const DtWin &w, const double *dem, double px, uint8_t *fdr, float *proxy);
int dt_launch_slope_twi_f64_w(hipStream_t s, const DtWin &w, const double *dem, const void *acc, int acc64, double px,
                              double n_top, float *slope, float *slope_rad, float *ti, float *mti);
int dt_launch_downslope_win_f64_w(hipStream_t s, const DtWin &w, const double *dem, const uint8_t *fdr, double px,
                                  double dz, int raw, float *out, int *n_unresolved);
int dt_launch_fh_zr64_w(hipStream_t s, const DtWin &w, const double *dem, int64_t n, const uint8_t *kind,
                        const int32_t *ref, double *zr64);
int64_t dt_hand_f64_table_slots(int64_t n_remote);
int dt_launch_hand_gfi_f64_w(hipStream_t s, const DtWin &w, const double *dem, const int32_t *idx32,
                             const int64_t *idx64, const void *fac, const void *a_river, int acc64, int64_t n_remote,
                             const uint8_t *res_ok, const int64_t *rem_gidx, const double *rem_zr64, void *table,
                             double expo, double b, double size, double *hand, float *gfi, float *lnhlh);
int dt_launch_ds_walk_f64(hipStream_t s, const DtWin &w, const double *dem, const uint8_t *fdr, double px, double dz,
                          int64_t n, void *rec, float *out);
int dt_launch_ds_walk_seed_f64(hipStream_t s, const DtWin &w, const double *dem, int64_t n, const int32_t *ys,
                               const int32_t *xs, void *rec);
int dt_launch_confusion(hipStream_t s, const double *desc, const int8_t *flood, int64_t n,
                        double nodata, const double *th_host, int nth, int under,
                        unsigned long long *counts4);
// dt_curve.hip: hist = uint64[2 (K + 1) + 1], zeroed here; th_dev = K sorted thresholds on the device
int dt_launch_threshold_hist(hipStream_t s, const double *desc, const int8_t *flood, int64_t n, double nodata,
                             const double *th_dev, int K, int under, unsigned long long *hist);
int dt_launch_i32_to_i64(hipStream_t s, const int32_t *a, int64_t n, int64_t *b);
int dt_launch_i64_to_i32(hipStream_t s, const int64_t *a, int64_t n, int32_t *b);

// tile-hierarchical versions (dt_tiles.hip); two phases so that a multi-GPU run can exchange the
// rank-level summaries in between (single GPU: local + finish with no injection)
size_t dt_flowacc_tiled_scratch(int64_t H, int64_t W);
int dt_launch_fa_local(hipStream_t s, const DtWin &w, const uint8_t *fdr, void *scratch, size_t scratch_bytes,
                       int32_t *acc32, int rank_level);
int dt_launch_fa_summary(hipStream_t s, const DtWin &w, void *scratch, int64_t *A, int32_t *xr, uint8_t *code);
int dt_launch_fa_finish(hipStream_t s, const DtWin &w, const uint8_t *fdr, const float *dem, void *scratch,
                        const unsigned long long *ext_perim, int64_t river_thr, void *acc, int acc64,
                        int8_t *river, int *status = nullptr);
// weighted flow accumulation (int64 fixed point, 2^-frac_bits units) into a float64 raster; raises
// DT_STATUS_BAD_WEIGHT on `status` for a weight outside the contract
size_t dt_flowacc_weighted_scratch(int64_t H, int64_t W);
int dt_launch_flowacc_weighted(hipStream_t s, const DtWin &w, const uint8_t *fdr, const float *dem, const double *wt,
                               int frac_bits, void *scratch, size_t scratch_bytes, double *acc, int *status);
size_t dt_flowhand_tiled_scratch(int64_t H, int64_t W);
// TI / MTI out of flow accumulation's last tile pass (the float32 chain): the slope raster the D8 kernel wrote
// (dt_launch_d8_slope), the outputs, and the marks (dt_stencil_aux_bytes) that dt_launch_slope_twi_fix consumes
struct DtTwiEpilogue {
  const float *slope;
  float *ti, *mti;
  double px, n_top;
  void *marks;
};
// nod4 (optional): the D8 kernel's nodata mask; when the fused kernel runs it replaces the read of `dem`
int dt_launch_fa_finish_fh_local(hipStream_t s, const DtWin &w, const uint8_t *fdr, const float *dem, void *fa_scratch,
                                 void *fh_scratch, size_t fh_bytes, const unsigned long long *ext_perim,
                                 int64_t river_thr, void *acc, int acc64, int8_t *river, int *status,
                                 const uint8_t *nod4 = nullptr, int ldm = 0, const DtTwiEpilogue *twi = nullptr,
                                 int *walked = nullptr);
bool dt_twi_epilogue_ok(const DtWin &w, const void *acc, const int8_t *river, const DtTwiEpilogue *twi);
int dt_launch_fh_local(hipStream_t s, const DtWin &w, const uint8_t *fdr, const int8_t *river, void *scratch,
                       size_t scratch_bytes);
int dt_launch_fh_summary(hipStream_t s, const DtWin &w, void *scratch, const float *dem, const void *acc, int acc64,
                         uint8_t *kind, int32_t *ref, int32_t *nc, int32_t *nd, float *zr, long long *ar);
int dt_launch_fh_finish(hipStream_t s, const DtWin &w, const float *dem, const uint8_t *fdr,
                        const int8_t *river, const void *acc, int acc64, double px, void *scratch,
                        const uint8_t *res_ok, const int32_t *res_nc, const int32_t *res_nd,
                        const long long *rem_gidx, const float *rem_zr, const long long *rem_ar, float *fdist,
                        int32_t *idx32, long long *idx64, float *hand, void *a_river, float *gfi = nullptr,
                        float *lnhlh = nullptr, double n_gfi = 0.0, double b_gfi = 1.0, double size = 1.0,
                        int walked = 0);
int dt_launch_gfi_both(hipStream_t s, const float *hand, const void *a_river, const void *fac, int acc64,
                       int64_t n, double expo, double b, double size, float *gfi, float *lnhlh);
int dt_launch_unique_extremes(hipStream_t s, const float *x, int64_t n, uint32_t *work4, float *out3);
int dt_launch_minmax_scale(hipStream_t s, const float *x, int64_t n, float mn, float mx, float nodata,
                           double *out);
int dt_launch_minmax_scale_f32f64(hipStream_t s, const float *x, int64_t n, double mn, double mx, double nodata,
                                  double *out);
int dt_launch_minmax_scale_den_f32(hipStream_t s, const float *x, int64_t n, float mn, float den, float nodata,
                                   float *out);
int dt_launch_minmax_scale_den_f64(hipStream_t s, const double *x, int64_t n, double mn, double den, double nodata,
                                   double *out);
int dt_launch_minmax_scale_f16(hipStream_t s, const void *x, int64_t n, float mn, float den, float nodata, void *out);
int dt_launch_classify_f64(hipStream_t s, const double *desc, const int32_t *bin_in, int8_t *flood, int64_t n,
                           double nodata, double th, int under, int remap, uint8_t *binary, int32_t *klass,
                           unsigned long long *counts4);
int dt_launch_classify_f32(hipStream_t s, const float *desc, const int32_t *bin_in, int8_t *flood, int64_t n,
                           float nodata, float th, int under, int remap, uint8_t *binary, int32_t *klass,
                           unsigned long long *counts4);
int dt_launch_membench_copy(hipStream_t s, const float *a, float *b, int64_t n, int blocks);
int dt_launch_membench_mix(hipStream_t s, const float *r0, const float *r1, float *w0, float *w1, float *w2, int64_t n,
                           int nr, int nw, int nt);
// rank-level solves on all-gathered summary rows (multi-GPU)
size_t dt_rank_solve_scratch(int nranks, int64_t Pmax);
int dt_launch_rank_solve_flowacc(hipStream_t s, int ty, int tx, const int64_t *heights, const int64_t *widths,
                                 int64_t Pmax, const void *rows, int64_t rowbytes, const int64_t *offs, int rank,
                                 int64_t P_rank, void *scratch, unsigned long long *ext_out);
int dt_launch_rank_solve_flowhand(hipStream_t s, int ty, int tx, const int64_t *heights, const int64_t *widths,
                                  int64_t Pmax, const void *rows, int64_t rowbytes, const int64_t *offs, int rank,
                                  int64_t P_rank, void *scratch, uint8_t *res_ok, int32_t *res_nc,
                                  int32_t *res_nd, long long *gidx, float *zr, long long *ar);
int dt_launch_rank_solve_flowhand_f64(hipStream_t s, int ty, int tx, const int64_t *heights, const int64_t *widths,
                                      int64_t Pmax, const void *rows, int64_t rowbytes, const int64_t *offs8, int rank,
                                      int64_t P_rank, void *scratch, uint8_t *res_ok, int32_t *res_nc,
                                      int32_t *res_nd, long long *gidx, float *zr, long long *ar, double *zr64);

// hydrological conditioning (dt_hydro.hip): depression filling + flat resolution; synchronous
size_t dt_hydro_scratch(int64_t H, int64_t W);
int dt_launch_condition(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, float *filled, uint8_t *fdr,
                        void *scratch, int *unresolved_host, int *rounds_host);
int dt_launch_condition_stage(hipStream_t s, const DtWin &w, int stage, int rounds, const float *dem, float *filled,
                              uint8_t *fdr, uint32_t *dist, int *flag_dev, uint8_t *nsame = nullptr);
int dt_launch_condition_async(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, float *filled,
                              uint8_t *fdr, void *scratch, int rounds, int *status);
// ... on float64 heights (a float64 filled surface; the same scratch, rounds and status)
int dt_launch_condition_f64(hipStream_t s, const double *dem, int64_t H, int64_t W, double px, double *filled,
                            uint8_t *fdr, void *scratch, int *unresolved_host, int *rounds_host);
int dt_launch_condition_async_f64(hipStream_t s, const double *dem, int64_t H, int64_t W, double px, double *filled,
                                  uint8_t *fdr, void *scratch, int rounds, int *status);

int dt_flow_impl();  // 1 global kernels, 2 tile-hierarchical (default)

// stream order (dt_streams.hip): Strahler order, Shreve magnitude and link heads of the network river != 0 on fdr;
// shreve / link may be NULL.  m_host != NULL (rasters of 2^31 cells or more) reads the network's cell count back and
// refuses 2^31 or more; otherwise nothing synchronises.
size_t dt_stream_order_scratch(int64_t H, int64_t W);
// The exclusive scan of per-block counts that stream order and the reach catchments share (kernels in dt_streams.hip):
// a counting pass covers DT_SCAN_CHUNK cells per block, the scan groups the block counts by the same number, and
// dt_launch_count_scan leaves offsets[b] = the sum of the counts before block b and meta[0] = the total.
#define DT_SCAN_CPT 8                      // cells per thread of a counting pass
#define DT_SCAN_CHUNK (256 * DT_SCAN_CPT)  // cells per block
static inline int64_t dt_scan_blocks(int64_t n) { return (n + DT_SCAN_CHUNK - 1) / DT_SCAN_CHUNK; }
struct DtCountScan {
  int64_t nblk, ng;  // blocks over the cells, groups over the blocks
  uint32_t *bcount, *gsum;
  int64_t *offsets, *goff, *meta;
};
// the arrays for n cells; `meta` is two words the caller has carved already (stream order keeps two rasters between
// them and the counts: every array stays at the offset it has always had)
DtCountScan dt_count_scan_carve(DtCarver &c, int64_t n, int64_t *meta);
int dt_launch_count_scan(hipStream_t s, const DtCountScan &cs, int64_t nblk);
int dt_launch_stream_order(hipStream_t s, const uint8_t *fdr, const int8_t *river, int64_t H, int64_t W, void *scratch,
                           size_t scratch_bytes, int8_t *strahler, int64_t *shreve, int64_t *link, int64_t *m_host);

// drainage / upslope length (dt_watershed.hip).  dem (nodata mask: <= -100) and pour (> 0: pour point) may be NULL;
// target / length / label may be NULL (label only with pour).  Nothing synchronises.  H * W < 2^31.
size_t dt_drainage_scratch(int64_t H, int64_t W);
size_t dt_upslope_length_scratch(int64_t H, int64_t W);
int dt_launch_drainage(hipStream_t s, const uint8_t *fdr, const float *dem, const int64_t *pour, int64_t H, int64_t W,
                       double px, void *scratch, size_t scratch_bytes, int64_t *target, double *length,
                       int64_t *label);
int dt_launch_upslope_length(hipStream_t s, const uint8_t *fdr, const float *dem, int64_t H, int64_t W, double px,
                             void *scratch, size_t scratch_bytes, double *length);

// flow-path extremes and the carving blend (dt_flowpath.hip; flowpath.py and flowdir.d8_carved hold the definitions).
// kind: 0 max, 1 min.  dem (nodata mask: <= -100) and stop (!= 0: a stop cell) may be NULL, so may value or where
// (both NULL: nothing runs).  filled NULL: no limit on the cut; carved may alias lowest.  Nothing synchronises.
// H * W < 2^31.
size_t dt_flowpath_scratch(int64_t H, int64_t W, int upslope);
int dt_launch_flowpath_upslope(hipStream_t s, const uint8_t *fdr, const float *dem, const float *values, int64_t H,
                               int64_t W, int kind, void *scratch, size_t scratch_bytes, float *value, int64_t *where);
int dt_launch_flowpath_downstream(hipStream_t s, const uint8_t *fdr, const float *dem, const float *values,
                                  const uint8_t *stop, int64_t H, int64_t W, int kind, void *scratch,
                                  size_t scratch_bytes, float *value, int64_t *where);
int dt_launch_carve_blend(hipStream_t s, const float *dem, const float *filled, const float *lowest, int64_t N,
                          float cut, float *carved);
// weighted flow-path sums (dt_flowpath.hip; flowpath.py holds the definitions): the sum of q = rint(wt * 2^frac_bits)
// along each path down to its terminal or first stop cell, and the longest such sum that ends at a cell, as float64
// (-100: no value).  dem and stop may be NULL; out NULL: nothing runs.  Raises DT_STATUS_BAD_WEIGHT on `status` for a
// weight outside dt_launch_flowacc_weighted's contract.  Nothing synchronises.  H * W < 2^31.
size_t dt_pathsum_scratch(int64_t H, int64_t W, int longest);
int dt_launch_pathsum_downstream(hipStream_t s, const uint8_t *fdr, const float *dem, const double *wt,
                                 const uint8_t *stop, int64_t H, int64_t W, int frac_bits, void *scratch,
                                 size_t scratch_bytes, double *out, int *status);
int dt_launch_pathsum_longest(hipStream_t s, const uint8_t *fdr, const float *dem, const double *wt, int64_t H,
                              int64_t W, int frac_bits, void *scratch, size_t scratch_bytes, double *out, int *status);

// reaches (dt_reaches.hip): the rank of every link head (reach ids), reach / catchment rasters, per-reach channel
// counts, stage tables and inundation depth; definitions in include/descriptools_hip.h.  Nothing synchronises.
// H * W < 2^31.  reach / catch / heads may be NULL (own_reach: reach is NULL and the launcher keeps the head ranks in
// scratch); idx is int32 (idx_bytes 4) or int64 (8); hand is float32 (hand_bytes 4) or float64 (8); slope may be NULL.
// slots: 0 the default LDS table, n > 0 at most n slots, < 0 no LDS table (DT_DBG_RC_SLOTS).
size_t dt_reach_catchments_scratch(int64_t N, int own_reach);
int dt_launch_reach_catchments(hipStream_t s, const int64_t *link, const void *idx, int idx_bytes, int64_t N,
                               void *scratch, size_t scratch_bytes, int32_t *reach, int32_t *catch_, int64_t *heads,
                               int64_t cap, int64_t *n_reaches_dev);
int dt_launch_reach_channels(hipStream_t s, const uint8_t *fdr, const int32_t *reach, int64_t H, int64_t W, int64_t R,
                             int64_t *end, int64_t *down, int64_t *n_cells, int64_t *n_card, int64_t *n_diag);
size_t dt_reach_tables_scratch(int K);
int dt_launch_reach_tables(hipStream_t s, const int32_t *catch_, const void *hand, int hand_bytes, const float *slope,
                           int64_t H, int64_t W, const double *stages_host, int K, int64_t R, int frac_bits,
                           void *scratch, size_t scratch_bytes, int64_t *cells, int64_t *Hq, int64_t *Bq, int *status,
                           int slots);
int dt_launch_inundate(hipStream_t s, const int32_t *catch_, const void *hand, int hand_bytes, const double *stage,
                       int64_t N, int64_t R, float *depth);

// D-infinity (dt_dinf.hip): flow angle / slope on the eight triangular facets (fdr, slope may be NULL), and the
// contributing area of an angle raster (wt may be NULL: 1 everywhere).  The accumulation is an in-degree countdown
// (dt_countdown.h holds the protocol, the workspace and the host sequence) and keeps its state in `scratch`:
// start != 0 sets it up and runs round 0 (from the sources), `rounds` queue rounds follow, finish != 0 writes `out`
// (and raises DT_STATUS_NOT_CONVERGED on `status` when queued work is left).  stack_cap: 0 the default (a lane holds the
// cell it carries on with and DI_STACK more), n > 0: at most n cells, the one it carries on with included, so 1 sends
// every second completion to the queue (DT_DBG_DINF_STACK).  Nothing synchronises.  H * W < 2^31.
int dt_launch_dinf_direction(hipStream_t s, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double px,
                             float *angle, float *slope);
#define DI_STACK 8
size_t dt_dinf_accumulate_scratch(int64_t H, int64_t W);
int dt_launch_dinf_accumulate(hipStream_t s, const float *angle, const double *wt, int64_t H, int64_t W, int frac_bits,
                              int start, int rounds, int finish, int stack_cap, void *scratch, size_t scratch_bytes,
                              double *out, int *status);
// the accumulation's control words in `scratch` (8 x uint32 on the device, dt_countdown.h's CD_C_*): queued, window lo,
// window hi, queue rounds that found work, the largest window, two-receiver cells
const uint32_t *dt_dinf_accumulate_ctl(void *scratch, int64_t H, int64_t W);

// The ops on the tile-round schedule (dt_tile_rounds.h): the D-infinity distance, the cost distance, the modified
// catchment area, the geodesic reconstruction and the harmonic smoother.
#define DT_TILE_ROUNDS_MAX 4096      // rounds a call takes at most (the flag words of a launcher call, harmonic's budget)
#define DT_TILE_ROUNDS_BATCH0 8      // the host tier's rounds between two looks at their flags: 8, 16, 32, then ...
#define DT_TILE_ROUNDS_BATCH_MAX 64  // ... 64: also what one dt_launch_dinf_distance call takes at most

// D-infinity distance down to the stream (dt_dinf_dist.hip; dinf.py holds the definition): the horizontal distance h
// and, with heights, the vertical drop v and the surface distance s along the D-infinity flow field to the targets
// (river == 1 and not nodata), stat 0 / 1 / 2 = average / minimum / maximum over the two receivers; the outputs hold
// -100 where a cell does not reach.  dem NULL: h alone (v and s NULL); otherwise v and s are both given.  The state
// lives in `scratch`: start != 0 sets it up, `rounds` (0..DT_TILE_ROUNDS_BATCH_MAX) rounds of tile visits follow, round r raising control
// word r when it settled something (a round that follows a quiet one returns at once), finish != 0 writes -100 on what
// does not reach and counts the reaching / dead / unsettled cells into control words 64 / 65 / 66 and the tile visits
// of the call (64 bits) into words 68-69.  visit_limit: 0, or
// the sweeps a workgroup makes over its tile per visit at most (tests); the result does not depend on it.  An angle
// outside the contract raises DT_STATUS_BAD_ANGLE on `status`.  Nothing synchronises.  H * W < 2^31.
size_t dt_dinf_distance_scratch(int64_t H, int64_t W);
int dt_launch_dinf_distance(hipStream_t s, const float *angle, const int8_t *river, const float *dem, int64_t H,
                            int64_t W, double px, int stat, int check_edges, int visit_limit, int start, int rounds,
                            int finish, void *scratch, size_t scratch_bytes, double *h, double *v, double *sf,
                            int *status);
// the control words in `scratch` (72 x uint32 on the device)
const uint32_t *dt_dinf_distance_ctl(void *scratch, int64_t H, int64_t W);

// Multiple flow direction (dt_mfd.hip; mfd.py holds the definition): the share raster of a DEM (eight uint16 per cell
// by octant, units of 2^-15, 16-byte aligned; fdr may be NULL; exponent in [0, 64]), and the contributing area of a
// share raster (wt may be NULL: 1 everywhere).  The accumulation is the same countdown (dt_countdown.h): it keeps its
// state in `scratch` and takes start, rounds, finish and stack_cap as dt_launch_dinf_accumulate does (the environment
// variable DT_DBG_MFD_STACK; tests); a share word outside the contract raises DT_STATUS_BAD_SHARES on `status`.
// Nothing synchronises.  H * W < 2^31.
int dt_launch_mfd_shares(hipStream_t s, const float *dem, const uint8_t *fdr, int64_t H, int64_t W, double exponent,
                         int contour, uint16_t *shares);
size_t dt_mfd_accumulate_scratch(int64_t H, int64_t W);
int dt_launch_mfd_accumulate(hipStream_t s, const uint16_t *shares, const double *wt, int64_t H, int64_t W,
                             int frac_bits, int start, int rounds, int finish, int stack_cap, void *scratch,
                             size_t scratch_bytes, double *out, int *status);
// the accumulation's control words in `scratch`, as dt_dinf_accumulate_ctl's (cells with two or more receivers)
const uint32_t *dt_mfd_accumulate_ctl(void *scratch, int64_t H, int64_t W);

// Routing (routing.py holds the definition): the same countdowns with a transfer function between "complete" and
// "split": a complete cell with load T passes on O = f(T, param) <= T (mode: DT_ROUTE_DECAY / _RETAIN / _LIMIT) and the
// receivers get the op's split of O.  The workspace, the control words and start / rounds / finish / stack_cap are the
// accumulation's (the *_accumulate_scratch and *_accumulate_ctl functions serve both); the out step writes any of
// inflow (T - q), load (T), outflow (O) and retained (T - O), a NULL pointer is an output not wanted.  A parameter
// outside its contract raises DT_STATUS_BAD_PARAM on `status` and acts as the identity.  Nothing synchronises.
int dt_launch_dinf_route(hipStream_t s, const float *angle, const double *wt, const double *param, int64_t H,
                         int64_t W, int frac_bits, int mode, int start, int rounds, int finish, int stack_cap,
                         void *scratch, size_t scratch_bytes, double *inflow, double *load, double *outflow,
                         double *retained, int *status);
int dt_launch_mfd_route(hipStream_t s, const uint16_t *shares, const double *wt, const double *param, int64_t H,
                        int64_t W, int frac_bits, int mode, int start, int rounds, int finish, int stack_cap,
                        void *scratch, size_t scratch_bytes, double *inflow, double *load, double *outflow,
                        double *retained, int *status);

// Local terrain attributes (dt_terrain.hip; terrain.py holds the definition): the quadratic fitted by least squares
// over the (2 radius + 1)^2 window of every cell, from separable float64 moment sums, and what is derived from its
// first and second derivatives.  out[8] = gradient, aspect, profile, plan, tangential, mean, laplacian, hillshade
// (DT_TERRAIN_OUTPUTS): a NULL entry is neither computed nor stored, at least one is given; -100 wherever the window is
// not complete.  (sx, sy, sz) is the unit vector to the sun (east, north, up).  1 <= radius <= DT_TERRAIN_RADIUS_MAX.
// One launch, no scratch; nothing synchronises.  H * W < 2^31.
#define DT_TERRAIN_OUTPUTS 8
#define DT_TERRAIN_RADIUS_MAX 32
int dt_launch_terrain(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, int radius, double sx,
                      double sy, double sz, float *const out[DT_TERRAIN_OUTPUTS]);

// Focal statistics at any radius (dt_focal.hip; focal.py holds the definition): summed-area tables of [valid], q and q^2
// (q = rint((z - origin) * 2^frac_bits), the latter two modulo 2^64) in `scratch`, then per cell and radius the
// four-corner window sums and a float64 stage.  n_radii == 1: count, mean, std, tpi, dev (and scale = the radius) of
// that window, each where its pointer is not NULL; n_radii > 1: DEVmax over the strictly increasing table `radii`
// (host memory) into dev and scale.  A valid height with q outside [0, dt_focal_qmax(radii[n_radii - 1])] raises
// DT_STATUS_BAD_HEIGHT on `status` and counts as q = 0.  Four launches whatever the rasters hold, nothing
// synchronises.  H * W < 2^31.
#define DT_FOCAL_RADIUS_MAX 4096
#define DT_FOCAL_RADII_MAX 32
#define DT_FOCAL_FRAC_BITS_MAX 24
size_t dt_focal_scratch(int64_t H, int64_t W);
int64_t dt_focal_qmax(int radius);  // the largest q with (2 radius + 1)^2 q^2 < 2^63
int dt_launch_focal(hipStream_t s, const float *dem, int64_t H, int64_t W, double origin, int frac_bits,
                    const int32_t *radii, int n_radii, void *scratch, size_t scratch_bytes, int32_t *count,
                    float *mean, float *std_, float *tpi, float *dev, uint16_t *scale, int *status);

// DEM filters (dt_filters.hip; filters.py holds the definition).  dt_launch_filter_extremes: the minimum, maximum and
// range (maximum - minimum, float64 difference) of the valid heights of the clipped (2 radius + 1)^2 window, the opening
// (the maximum of the minimum raster) and the closing (the minimum of the maximum raster); a NULL output is neither
// computed nor stored, at least one is given; -100 where the cell's own height is not valid.  Three launches per window
// pass (van Herk / Gil-Werman running extremes along rows, then columns), the planes in `scratch` (24 B per cell).
// dt_launch_filter_rank: the height of index table[n] among the n valid heights of the window, sorted ascending
// (table: (2 radius + 1)^2 + 1 entries in host memory, table[n] < max(n, 1)); one launch, no scratch.
// dt_launch_filter_denoise: Sun et al.'s feature-preserving denoising -- unit normals, their thresholded weighted mean
// over the window (cos_threshold = the cosine of the angle threshold), `iterations` Jacobi steps of the heights, each
// change bounded by max_change against the input; 2 + iterations launches, 28 B per cell of `scratch`; `out` must not
// be `dem`.  Nothing synchronises.  H * W < 2^31.
#define DT_FILTER_RADIUS_MAX 4096
#define DT_FILTER_RANK_RADIUS_MAX 16
#define DT_FILTER_DENOISE_RADIUS_MAX 16
#define DT_FILTER_DENOISE_ITERATIONS_MAX 32
size_t dt_filter_extremes_scratch(int64_t H, int64_t W);
int dt_launch_filter_extremes(hipStream_t s, const float *dem, int64_t H, int64_t W, int radius, void *scratch,
                              size_t scratch_bytes, float *minimum, float *maximum, float *range, float *opening,
                              float *closing);
int dt_launch_filter_rank(hipStream_t s, const float *dem, int64_t H, int64_t W, int radius, const uint16_t *table,
                          int n_table, float *out);
size_t dt_filter_denoise_scratch(int64_t H, int64_t W);
int dt_launch_filter_denoise(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, int radius,
                             double cos_threshold, int iterations, double max_change, void *scratch,
                             size_t scratch_bytes, float *out);

// Valley bottom and ridge top flatness (dt_mrvbf.hip; mrvbf.py holds the definition).  dt_launch_percentile: per cell
// the shares of the valid cells of the clipped disc of `radius` that are strictly lower / strictly higher (a NULL
// output is neither computed nor stored, at least one is given; -100 where the centre is not valid).
// dt_launch_coarsen: one generalisation step of a raster of cell size px with the Gaussian weights g6[k] =
// exp(-k^2 / 18) (host memory) -> the smoothed height and its slope in percent at a third of the resolution, rasters of
// ceil(H / 3) x ceil(W / 3) cells.  dt_launch_mrvbf: MRVBF and / or MRRTF over `levels` levels (2 .. 10) with the
// exponents p[L - 2] of the levels L = 2 .. levels (host memory); the pyramid of the levels >= 3 lives in `scratch`
// (16 B per coarse cell), 2 (levels - 2) launches build it and one launch at base resolution writes the outputs.
// Nothing synchronises.  H * W < 2^31.
#define DT_PERCENTILE_RADIUS_MAX 16
#define DT_MRVBF_LEVELS_MAX 10
int dt_launch_percentile(hipStream_t s, const float *dem, int64_t H, int64_t W, int radius, float *lower,
                         float *higher);
int dt_launch_coarsen(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, const double *g6, float *dem3,
                      float *slope3);
size_t dt_mrvbf_scratch(int64_t H, int64_t W, int levels);
int dt_launch_mrvbf(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, double slope_threshold,
                    int levels, double pctl_valley, double pctl_ridge, const double *p, void *scratch,
                    size_t scratch_bytes, float *mrvbf, float *mrrtf);

// Lines of sight (dt_horizon.hip; horizon.py holds the definition): from every cell the largest and the smallest tangent
// of the elevation angle to the samples skip + 1 .. radius of each of the eight compass directions, t = (z_k - z0) *
// (1 / (k step)) in float64 with the reciprocals tabulated here on the host and handed to the kernel by value, and what
// derives from them: landform (uint8, 1 .. 10) and pattern (uint16, the eight ternary digits against flat_tan = tan of
// the flatness angle), positive and negative openness (float32, radians) and the sky-view factor (float32).  A NULL
// output is neither computed nor stored, at least one is given; 0 / 65535 / -100 wherever the centre is not valid or a
// direction has no valid sample.  1 <= radius <= DT_HORIZON_RADIUS_MAX, 0 <= skip < radius, flat_tan finite and >= 0.
// One launch, no scratch; nothing synchronises.  H * W < 2^31.
#define DT_HORIZON_RADIUS_MAX 64
int dt_launch_horizon(hipStream_t s, const float *dem, int64_t H, int64_t W, double px, int radius, int skip,
                      double flat_tan, uint8_t *landform, uint16_t *pattern, float *positive, float *negative,
                      float *sky_view);

// Euclidean proximity (dt_proximity.hip): for every cell the nearest source (river == 1 and, with nod, nod > -100) by
// exact squared distance, ties to the smallest flat index -> distance = float32(px * sqrt(float64(d2))) and indices =
// the source's flat index; -100 where nod <= -100 and when there is no source.  nod may be NULL.  The row pass, the
// per-level launches of the column pass and their state live in `scratch`; nothing synchronises.  H * W < 2^31.
size_t dt_proximity_scratch(int64_t H, int64_t W);
int dt_launch_proximity(hipStream_t s, const int8_t *river, const float *nod, int64_t H, int64_t W, double px,
                        void *scratch, size_t scratch_bytes, float *distance, int64_t *indices);

// Cost distance (dt_cost.hip; cost.py holds the definition): the least accumulated cost over `friction` (passable: 0 <
// f < +inf) from the sources (sources == 1 and passable) under connectivity 4 or 8, the flat index of the source a cell
// is reached from (indices, may be NULL) and the ESRI D8 code of its first step towards it (backlink, may be NULL);
// -100 / -100 / 0 on barriers and unreached cells.  The state lives in `cost` and in `scratch` (laid out with the parent
// plane when indices is given: alloc != 0): start != 0 sets it up, `rounds` (0..DT_TILE_ROUNDS_MAX) rounds of tile
// visits follow, round r raising control word r when it lowered something (a round that follows a quiet one returns at
// once), finish != 0 computes the back-links, the fills and the allocation and counts the reached cells, the reached
// non-source cells without a back-link and the tile visits of the call (64 bits) into control words
// DT_COST_CTL_COUNTS + 0, + 1 and + 2-3; with rounds in the same call it raises DT_STATUS_NOT_CONVERGED on `status` when
// the last round still lowered something, and DT_STATUS_NO_BACKLINK for a cell without a back-link (status may be NULL).
// visit_limit: 0, or the sweeps a workgroup makes over its tile per visit at most (tests); the result does not depend
// on it.  Nothing synchronises.  H * W < 2^31.
#define DT_COST_CTL_COUNTS (DT_TILE_ROUNDS_MAX + 32)
size_t dt_cost_distance_scratch(int64_t H, int64_t W, int alloc);
int dt_launch_cost_distance(hipStream_t s, const float *friction, const int8_t *sources, int64_t H, int64_t W,
                            double px, int connectivity, int visit_limit, int start, int rounds, int finish,
                            void *scratch, size_t scratch_bytes, double *cost, int64_t *indices, uint8_t *backlink,
                            int *status);
// the control words in `scratch` (DT_COST_CTL_COUNTS + 8 x uint32 on the device)
const uint32_t *dt_cost_distance_ctl(void *scratch, int64_t H, int64_t W, int alloc);

// SAGA wetness index (dt_wetness.hip; wetness.py holds the definition).  suction: s of a slope raster (log_t = ln t,
// taken by the caller).  index: swi = float32(log(M / tan(b))) from a modified area.  area: M = the least solution of
// M(v) = max(A(v), fl(s(v) * max over the valid neighbours of M)), -100 on nodata.  The state lives in `modified` and in
// `scratch`: start != 0 sets it up, `rounds` (0..DT_TILE_ROUNDS_MAX) rounds of tile visits follow, round r raising
// control word r when it raised something (a round that follows a quiet one returns at once), finish != 0 writes the
// fills and counts the raised cells and the tile visits of the call (64 bits) into control words DT_WETNESS_CTL_COUNTS
// + 0 and + 2-3; with rounds in the same call it raises DT_STATUS_NOT_CONVERGED on `status` (may be NULL) when the last
// round still raised something.  The scratch may carry a suction plane and an M plane behind the control block (the
// composite call's).  visit_limit as for the cost distance.  Nothing synchronises.  H * W < 2^31.
#define DT_WETNESS_CTL_COUNTS DT_TILE_ROUNDS_MAX
size_t dt_wetness_scratch(int64_t H, int64_t W, int suction_plane, int m_plane);
const uint32_t *dt_wetness_ctl(void *scratch, int64_t H, int64_t W);
float *dt_wetness_suction_plane(void *scratch, int64_t H, int64_t W);
double *dt_wetness_m_plane(void *scratch, int64_t H, int64_t W, int suction_plane);
int dt_launch_wetness_suction(hipStream_t s, const float *slope, int64_t N, double log_t, double weight, double offset,
                              double minimum, float *suction);
int dt_launch_wetness_index(hipStream_t s, const double *modified, const float *slope, int64_t N, double offset,
                            double minimum, float *swi);
int dt_launch_wetness_area(hipStream_t s, const double *area, const float *suction, int64_t H, int64_t W,
                           int visit_limit, int start, int rounds, int finish, void *scratch, size_t scratch_bytes,
                           double *modified, int *status);

// Geodesic reconstruction (dt_morphology.hip; morphology.py holds the definition): the reconstruction by dilation
// (erosion != 0: by erosion) of a marker under `mask`, on order-preserving keys; -100 on invalid cells and on valid
// cells that no marker reaches.  mode (DT_MORPH_*, descriptools_hip.h) says what the marker is: `marker` (MARKER), the
// mask shifted by `h` (SHIFT), the mask's key +- 1 (STEP), the mask on the outlet cells -- `seeds` != 0, or seeds NULL:
// the raster's edge and the 8-neighbours of invalid cells -- (OUTLETS), or the window minimum / maximum of the mask at
// `radius` (WINDOW: dt_launch_filter_extremes into a plane of the scratch).  One output: `out` (float32; it holds the
// keys while the rounds run) or `out8` (uint8, 1 where the result differs from the mask; the keys live in the scratch).
// The state lives in the output and in `scratch`: start != 0 sets it up, `rounds` (0..DT_TILE_ROUNDS_MAX) rounds of
// tile visits follow, round r raising control word r when it stored something (a round that follows a quiet one returns
// at once), finish != 0 writes the output and counts the valid cells whose result is not their start value and the tile
// visits of the call (64 bits) into control words DT_MORPH_CTL_COUNTS + 0 and + 2-3; with rounds in the same call it
// raises DT_STATUS_NOT_CONVERGED on `status` (may be NULL) when the last round still stored something.  Every call of
// one reconstruction names the same arguments.  visit_limit as for the cost distance.  Nothing synchronises.
// H * W < 2^31.
#define DT_MORPH_CTL_COUNTS DT_TILE_ROUNDS_MAX
size_t dt_morph_scratch(int64_t H, int64_t W, int mode, int to_u8);
const uint32_t *dt_morph_ctl(void *scratch, int64_t H, int64_t W);
int dt_launch_morph(hipStream_t s, int mode, int erosion, int connectivity, const float *mask, const float *marker,
                    const uint8_t *seeds, double h, int radius, int64_t H, int64_t W, int visit_limit, int start,
                    int rounds, int finish, void *scratch, size_t scratch_bytes, float *out, uint8_t *out8,
                    int *status);

// Harmonic interpolation (dt_harmonic.hip; harmonic.py holds the definition): out = the discrete harmonic function on
// the domain with the fixed cells held (fixed == 1 and a finite value; domain NULL: everywhere), NaN outside the domain.
// Nested iteration on a pyramid by 2 whose level 0 is `out` itself; the other levels, the masks, the flags and the key
// words live in `scratch`.  level_cap: 0, or the number of levels at most (1: no pyramid; benchmarks).  A call is
// setup -- the masks, the pyramid, the coarsest level's start -- then, from the coarsest level (dt_harmonic_levels - 1)
// down to level 0, rounds [first_round, first_round + rounds) of tile visits, each followed by its residual into key
// word r of the level (the bits of max r; launches behind a round whose key is <= tol's return at once and hand the key
// on), and `prolong` from `level` to level - 1; finish writes DT_HARMONIC_INFO words to `info` (NULL: into the scratch,
// dt_harmonic_info) and raises DT_STATUS_NOT_CONVERGED on `status` (may be NULL) when level 0's last residual exceeds
// tol.  info: 0 levels, 1 rounds on level 0, 2 rounds on all levels, 3 tile visits, 4 the last residual of level 0 as
// a double's bits, 5 whether that is <= tol, DT_HARMONIC_INFO_LEVEL0 + l the rounds on level l.  Precondition: every
// free cell of the domain is joined to a fixed cell through the domain (4-connected); without it those cells hold an
// unspecified constant.  Nothing synchronises.  0 < H * W < 2^31, 1 <= max_rounds <= DT_TILE_ROUNDS_MAX.
#define DT_HARMONIC_LEVELS_MAX 32
#define DT_HARMONIC_INFO_LEVEL0 8
#define DT_HARMONIC_INFO (DT_HARMONIC_INFO_LEVEL0 + DT_HARMONIC_LEVELS_MAX)
size_t dt_harmonic_scratch(int64_t H, int64_t W, int max_rounds, int level_cap);
int dt_harmonic_levels(int64_t H, int64_t W, int level_cap);
const unsigned long long *dt_harmonic_keys(void *scratch, int64_t H, int64_t W, int max_rounds, int level_cap,
                                           int level);
const int64_t *dt_harmonic_info(void *scratch, int64_t H, int64_t W, int max_rounds, int level_cap);
int dt_launch_harmonic_setup(hipStream_t s, const float *values, const int8_t *fixed, const int8_t *domain, int64_t H,
                             int64_t W, int max_rounds, int level_cap, void *scratch, size_t scratch_bytes,
                             double *out);
int dt_launch_harmonic_rounds(hipStream_t s, int64_t H, int64_t W, int max_rounds, int level_cap, int level,
                              int first_round, int rounds, double tol, void *scratch, size_t scratch_bytes,
                              double *out);
int dt_launch_harmonic_prolong(hipStream_t s, int64_t H, int64_t W, int max_rounds, int level_cap, int level,
                               void *scratch, size_t scratch_bytes, double *out);
int dt_launch_harmonic_finish(hipStream_t s, int64_t H, int64_t W, int max_rounds, int level_cap, double tol,
                              void *scratch, size_t scratch_bytes, int64_t *info, int *status);

// Local-inertial flood inundation (dt_inundation.hip; inundation.py holds the scheme).  The state h, qx, qy (float64,
// H x W) is the caller's and is updated in place; its second copy and the control block (DT_IN_CTL words of 8 bytes:
// 0 t, 1 the next step's dt, 2 the time after it, 3 whether no step is left, 4 the steps of this call, 5 the steps in
// all, 6 the smallest dt, 7 the last dt, 8 the steps the limiter acted in, 9 the largest depth, 10-11 accumulators,
// 12 whether t >= t_end; doubles as their bits) live in `scratch`.  z: float32 heights, NaN on a wall; manning, rain:
// float32 rasters, or NULL for the scalars n and rain_s; max_depth, arrival: updated in place, or NULL; cells, times,
// discharge: the inflow table on the device (K may be 0).  begin opens a call at (t0, steps0), `steps` enqueues that
// many guarded steps (one that comes after the end returns at once), finish moves the state back into h, qx, qy when
// it sits in the second copy and writes DT_INUNDATION_INFO_WORDS words to `info` (on the device; may be NULL).
// Nothing synchronises.  0 < H * W < 2^31.
#define DT_IN_CTL 16
struct DtInundation {
  const float *z, *manning, *rain;
  int64_t H, W;
  double px, t_end, n, rain_s, alpha, dt_max, dry, slope, arrival_depth;
  int open;
  const int64_t *cells;
  const double *times, *discharge;
  int K, T;
  int64_t max_steps;  // of this call; < 0: no limit
  double *h, *qx, *qy, *max_depth, *arrival;
};
size_t dt_inundation_scratch(int64_t H, int64_t W);
const unsigned long long *dt_inundation_ctl(void *scratch, int64_t H, int64_t W);
int dt_launch_inundation_begin(hipStream_t s, const DtInundation &d, double t0, int64_t steps0, void *scratch,
                               size_t scratch_bytes);
int dt_launch_inundation_steps(hipStream_t s, const DtInundation &d, int steps, void *scratch, size_t scratch_bytes);
int dt_launch_inundation_finish(hipStream_t s, const DtInundation &d, void *scratch, size_t scratch_bytes,
                                int64_t *info);

// Connected regions (dt_regions.hip; regions.py holds the definition): label = the smallest flat index of the cell's
// region of mask != 0 under connectivity 4 or 8 (-100 on background), size = its cell count (0 on background), keep =
// foreground, seeded (seeds NULL: every region is) and size >= min_cells.  label, size and keep may each be NULL (seeds
// count only with keep).  dt_launch_inundate_connected: dt_launch_inundate's depth, 0 on the wet cells whose wet region
// holds no wet cell with river == 1.  The union-find plane, the counts and the masks live in `scratch`; 3 to 5 launches
// whatever the rasters hold; nothing synchronises.  H * W < 2^31.
size_t dt_regions_scratch(int64_t H, int64_t W);
size_t dt_inundate_connected_scratch(int64_t H, int64_t W);
int dt_launch_regions(hipStream_t s, const uint8_t *mask, const uint8_t *seeds, int64_t H, int64_t W, int connectivity,
                      int64_t min_cells, void *scratch, size_t scratch_bytes, int64_t *label, int64_t *size,
                      uint8_t *keep);
int dt_launch_inundate_connected(hipStream_t s, const int32_t *catch_, const void *hand, int hand_bytes,
                                 const double *stage, const int8_t *river, int64_t H, int64_t W, int64_t R,
                                 int connectivity, void *scratch, size_t scratch_bytes, float *depth);

// n doubles from host memory into device memory as kernel arguments, 128 per launch: no host copy, so the caller's
// array may go away at once (the stages of the reach tables, the edges of the zonal histogram; dt_reaches.hip)
void dt_launch_host_doubles(hipStream_t s, const double *src_host, int n, double *dst);

// zonal statistics (dt_zonal.hip): label compaction, per-zone integer tables, per-zone histograms / cross-tabulation
// and painting a table back onto its zones; definitions in include/descriptools_hip.h.  Nothing synchronises.
// H * W < 2^31.  labels is int32 (label_bytes 4) or int64 (8); values is float32 (value_bytes 4) or float64 (8), and
// for dt_launch_zonal_counts an int32 column raster with value_bytes 0 (cross-tabulation, K columns, edges unused).
// Tables that are NULL are not computed.  slots: 0 the default LDS table, n > 0 at most n slots, < 0 no LDS table
// (DT_DBG_RC_SLOTS).
size_t dt_zonal_compact_scratch(int64_t limit);
int dt_launch_zonal_compact(hipStream_t s, const void *labels, int label_bytes, int64_t N, int64_t limit,
                            void *scratch, size_t scratch_bytes, int32_t *zones, int64_t *labels_of, int64_t cap,
                            int64_t *n_zones_dev);
int dt_launch_zonal_tables(hipStream_t s, const int32_t *zones, const void *values, int value_bytes, int64_t H,
                           int64_t W, int64_t n_zones, double origin, int frac_bits, int has_nodata, double nodata,
                           int64_t *count, int64_t *s1, uint64_t *s2_lo, uint64_t *s2_hi, void *vmin, void *vmax,
                           int *status, int slots);
size_t dt_zonal_counts_scratch(int K);
int dt_launch_zonal_counts(hipStream_t s, const int32_t *zones, const void *values, int value_bytes, int64_t H,
                           int64_t W, int64_t n_zones, const double *edges_host, int K, int has_nodata, double nodata,
                           void *scratch, size_t scratch_bytes, int64_t *counts, int *status, int slots);
int dt_launch_zonal_paint(hipStream_t s, const void *table, int elem_bytes, int64_t n_table, const int32_t *zones,
                          int64_t N, uint64_t fill_bits, void *out);

// Resampling (dt_resample.hip; resample.py holds the definition).  dt_check_resample: what both tiers require of a
// call, pointers aside; each entry runs it once.  dt_launch_resample takes arguments that have passed it and launches
// one kernel: the six matrix entries are read from the host pointer and passed by value.  Nothing synchronises, nothing
// is allocated.
int dt_check_resample(int dtype, int64_t Hs, int64_t Ws, const double *matrix, int method, int64_t nodata, int64_t Hd,
                      int64_t Wd);
int dt_launch_resample(hipStream_t s, const void *src, int dtype, int64_t Hs, int64_t Ws, const double *matrix,
                       int method, int64_t nodata, uint64_t fill_bits, void *dst, int64_t Hd, int64_t Wd);

// Vector rasterisation (dt_vector.hip; vector.py holds the definition).  dt_check_rasterize: what both tiers require of
// a call, pointers aside; each entry runs it once.  dt_rasterize_count_host: a polygon geometry's crossings and the most
// on one row, host arithmetic, no device.  dt_rasterize_scratch: the bytes of 4 H + 8 capacity, each rounded up to 256.
// dt_launch_rasterize takes arguments that have passed the check; info is int64[4] on the device, ev NULL or 8 events
// recorded around the seven phases.  Nothing synchronises, nothing is allocated.
int dt_check_rasterize(int kind, int64_t P, int64_t N, int64_t H, int64_t W, int connectivity, int all_touched,
                       int64_t capacity);
void dt_rasterize_count_host(const double *coords, const int64_t *parts, int64_t P, int64_t H, int64_t *total,
                             int64_t *largest);
size_t dt_rasterize_scratch(int64_t H, int64_t capacity);
int dt_launch_rasterize(hipStream_t s, int kind, const double *coords, const int64_t *parts, const int32_t *ids,
                        int64_t P, int64_t N, int64_t H, int64_t W, int connectivity, int all_touched,
                        int64_t capacity, void *scratch, size_t scratch_bytes, int32_t *label, int64_t *info,
                        hipEvent_t *ev);

// Polygonisation (dt_polygonize.hip; vector.py holds the definition).  dt_check_polygonize: what both tiers require of
// a call, pointers aside.  dt_polygonize_scratch: 768 bytes of round flags, 2 x 4 bytes per 1024 lattice vertices of
// block sums, 4 bytes per cell and 20 bytes per edge of capacity (two 8-byte doubling words and the leader), each array
// rounded up to 256; count_only: the flags and the block sums alone.  dt_launch_polygonize takes arguments that have
// passed the check; info is int64[8] on the device (edges, vertices, rings, holes, rounds of the leader doubling, the
// overflow flags 1 edges | 2 vertices | 4 rings, rounds of the rank doubling, rounds of the shell links), ev NULL or 8
// events recorded around the seven phases.  Nothing synchronises, nothing is allocated.
int dt_check_polygonize(int64_t H, int64_t W, int64_t cap_edges, int64_t cap_vertices, int64_t cap_rings);
size_t dt_polygonize_scratch(int64_t H, int64_t W, int64_t cap_edges, int count_only);
int dt_launch_polygonize(hipStream_t s, const int32_t *labels, int64_t H, int64_t W, int64_t cap_edges,
                         int64_t cap_vertices, int64_t cap_rings, int count_only, void *scratch, size_t scratch_bytes,
                         double *coords, int64_t *parts, int32_t *ids, int32_t *shell, int64_t *info, hipEvent_t *ev);
