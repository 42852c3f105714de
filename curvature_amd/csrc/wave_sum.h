// The sum of a float over the 64 lanes of a wave by DPP: six VALU instructions and no LDS traffic per value (a butterfly
// costs six ds_bpermute round trips).  Used where a lane holds many values to reduce: the pairs of persample.hip's joint
// covariance, the class sums of logit_mc.hip.
#pragma once
#include "common.h"

namespace curv {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_lanes(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}

// The sum of `v` over the wave, in lane 63 (a lane outside a step's row mask adds the 0 of `old`).
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_lanes<0xB1, 0xf>(v);       // quad_perm [1, 0, 3, 2]
  v += dpp_lanes<0x4E, 0xf>(v);       // quad_perm [2, 3, 0, 1]
  v += dpp_lanes<0x141, 0xf>(v);      // row_half_mirror
  v += dpp_lanes<0x140, 0xf>(v);      // row_mirror: every lane holds the sum of its row of 16
  v += dpp_lanes<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
  v += dpp_lanes<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3
  return v;
}

}  // namespace curv
