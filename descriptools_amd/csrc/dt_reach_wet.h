// dt_reach_wet.h -- the value and the wet predicate of HAND inundation, once: k_rc_inundate (dt_reaches.hip) takes its
// depth from it and connected inundation (dt_regions.hip) its wet mask, so the two cannot drift apart.
#pragma once
#include "dt_common.h"

// dt_inundate's value: -100 where hand == -100; else float32(stage[r] - float64(hand)) when catch r is in range,
// stage[r] is finite and 0 <= hand <= stage[r] -- exactly then the cell is `wet` (at depth 0 when hand == stage[r]);
// else 0.
template <typename HT>
__device__ __forceinline__ float dt_rc_depth(int32_t r, HT hv, const double *__restrict__ stage, int64_t R,
                                             bool &wet) {
  wet = false;
  const double h = (double)hv;
  if (h == -100.0) return DT_NODATA;
  if (r < 0 || r >= R) return 0.f;
  const double st = __ldg(&stage[r]);
  if (!(fabs(st) <= 1.7976931348623157e308)) return 0.f;  // NaN or infinite
  wet = h >= 0.0 && h <= st;
  return wet ? (float)(st - h) : 0.f;
}
