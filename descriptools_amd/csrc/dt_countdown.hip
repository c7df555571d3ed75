// dt_countdown.hip -- the one kernel of the in-degree countdown that is the same for every op (dt_countdown.h holds
// the protocol).
#include "dt_countdown.h"

// the window of the next queue round: what was queued before this kernel ran and has not been drained
__global__ void k_cd_mark(uint32_t *ctl) {
  const uint32_t lo = ctl[CD_C_HI], hi = ctl[CD_C_TAIL];
  ctl[CD_C_LO] = lo;
  ctl[CD_C_HI] = hi;
  if (hi > lo) {
    ctl[CD_C_ROUNDS] += 1u;
    if (hi - lo > ctl[CD_C_HIGH]) ctl[CD_C_HIGH] = hi - lo;
  }
}

void cd_launch_mark(hipStream_t s, uint32_t *ctl) { hipLaunchKernelGGL(k_cd_mark, dim3(1), dim3(1), 0, s, ctl); }
