// Standard normal noise: Philox4x32-10 counter-based generator + Box-Muller, 4 values per counter.  One device function
// for every kernel that draws: randn_kernel (gemm.hip: curv_randn / curv_randn_counter) writes the values out, logit_mc.hip
// consumes them in registers - the same counter gives the same four bits in both.
#pragma once
#include "common.h"

namespace curv {

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = 0xD2511F53ull * c[0];
  const unsigned long long p1 = 0xCD9E8D57ull * c[2];
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0;
  const unsigned n1 = (unsigned)p1;
  const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
  const unsigned n3 = (unsigned)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// z[0 .. 4) ~ N(0, 1): the four values of counter `ctr` of the stream keyed by `seed`.
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned long long ctr, float (&z)[4]) {
  unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u};
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = ((float)(c[2 * p] >> 8) + 1.0f) * (1.0f / 16777216.0f);      // (0, 1]
    const float u2 = (float)(c[2 * p + 1] >> 8) * (1.0f / 16777216.0f);           // [0, 1)
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * p] = r * cs;
    z[2 * p + 1] = r * sn;
  }
}

}  // namespace curv
