// Phase 2 of the depthwise per-sample line as other sources launch it: the `sq` and `quad` reductions of persample_dw.hip
// (ps_dw_sq_kernel, ps_dw_quad_kernel) over per-sample products p (N, C, n_g) that a phase 1 of their own left in scratch.
// norm_factor.hip ends in them; the kernels exist once.
#pragma once
#include "common.h"

namespace curv {

// dst[c c_rs + j] (+)= alpha sum_n p[n, c, j]**2
struct DwSqArgs {
  const float* p;
  float* dst;
  long long c_rs;
  int N, C, n_g, first;
  float alpha;
};

// out[n o_stride] (+)= alpha sum_c s[c]**2 sum_j W[c w_rs + j] (sum_i T[c t_cs + i t_rs + j] p[n, c, i])**2
struct DwQuadArgs {
  const float* p;
  const float* T;
  const float* W;
  const float* s;
  float* out;
  long long t_cs, t_rs, w_rs, o_stride;
  int N, C, n_g, first;
  float alpha;
};

// The reductions of `n` items on `stream`, up to 16 per launch, in call order.  The arguments are taken as checked.
int dw_launch_sq(const char* name, hipStream_t stream, const DwSqArgs* items, int n);
int dw_launch_quad(const char* name, hipStream_t stream, const DwQuadArgs* items, int n);

}  // namespace curv
