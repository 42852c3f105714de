// Per-sample products of true depthwise convolutions (curv_persample_dw_sq_accumulate / curv_persample_dw_quad_reduce,
// include/curv_hip.h; DESIGN.md "K14"; curv_persample_dw_project / curv_persample_dw_quad_grid_reduce and the Gram of
// staged rows, curv_persample_gram_reduce: DESIGN.md "K15").
//
// A depthwise layer (in_channels == out_channels == groups) has one 1 x (kh kw [+ 1]) row of [W | b] per channel.  Its
// per-sample gradient is no matrix product but a correlation of two planes,
//     p[n, c, a kw + b] = sum_{oh, ow} g[n, c, oh, ow] * x[n, c, oh sh + a - ph, ow sw + b - pw],     p[n, c, kh kw] = sum g
// that reads x and g once each and leaves n_g = kh kw + has_bias numbers per (sample, channel).  Those are small enough
// to write out, so the work is two phases:
//   1. ps_dw_product_kernel: every (n, c) plane of an item is reduced to its n_g values in workspace (N C n_g floats).
//      Plain VALU fp32 (10 FMAs per output pixel for 3 x 3: the work is HBM-bound).  A plane goes to one wave, or - from
//      DW_SPLIT_L outputs on - to the four waves of a workgroup; lanes take consecutive ow.  Where the output rows are
//      whole aligned groups of four a lane takes four neighbouring outputs: one 16-byte load of g, and the x window of
//      3 sw + kw values per kernel row is loaded once for the four - as aligned 16-byte groups where the rows of x are
//      aligned runs too and pw == kw / 2, per element otherwise.  The n_g accumulators stay in registers (kernel sizes
//      1, 3, 5, 7 squared are compiled in; any other kernel of at most 49 taps takes a tap-at-a-time form with one
//      accumulator).  Sums in a fixed order: lane, wave (DPP), the waves of the workgroup in order.  No atomics.
//   2. one small kernel per reduction: ps_dw_sq_kernel (one thread per (c, j), the samples in order) or
//      ps_dw_quad_kernel (one workgroup per sample: the T / W / s form per channel, a thread's channels in order, then
//      lane, wave, workgroup), ps_dw_project_kernel (one thread per value written) or ps_dw_grid_kernel (as the quad
//      kernel, one chain per grid point).
// How a plane is split follows from its own sizes only, so an item's bits do not depend on the other items of a call.
#include "kernarg.h"
#include "persample_dw_phase2.h"
#include "side_build.h"
#include "wave_sum.h"

#include <vector>

namespace curv {
namespace {

constexpr int DW_THREADS = 256;       // four waves
constexpr int DW_WAVES = DW_THREADS / 64;
constexpr int DW_BATCH = 16;          // items per launch
constexpr int DW_MAX_TAPS = 49;
constexpr int DW_SPLIT_L = 1024;      // outputs of a plane from which its four waves share it

// One item as phase 1 reads it.
struct DwItem {
  const float* x;
  const float* g;
  float* p;                           // (N, C, n_g)
  long long x_sn, g_sn;               // sample strides: the plane base is formed in 64 bits
  unsigned x_sc, x_sh, x_sw, g_sc, g_sh, g_sw;
  int N, C, H, W, Ho, Wo, kh, kw, sh, sw, ph, pw;
  int has_bias, n_g;
  int split;                          // 1: a workgroup per plane; 0: a wave per plane
  int quads;                          // 1: four outputs per lane (Wo % 4 == 0, g rows 16-byte aligned runs)
  int xvec;                           // 1 (with quads): x in aligned groups of four too (dw_plane_quads_xvec)
  long long base;                     // first workgroup of the item in the launch
};
typedef ArgBatch<DwItem, DW_BATCH> DwBatch;

struct DwSq {
  const float* p;
  float* C;
  long long c_rs;
  int N, Cn, n_g, first;
  float alpha;
  long long base;                     // first thread
};
typedef ArgBatch<DwSq, DW_BATCH> DwSqBatch;

struct DwQuad {
  const float* p;
  const float* T;
  const float* W;
  const float* s;
  float* out;
  long long t_cs, t_rs, w_rs, o_stride;
  int N, Cn, n_g, first;
  float alpha;
  long long base;                     // first workgroup (= sample)
};
typedef ArgBatch<DwQuad, DW_BATCH> DwQuadBatch;

struct DwProject {
  const float* p;
  const float* T;
  const float* W;
  const float* s;
  float* y;
  long long t_cs, t_rs, w_rs, y_ns;
  int Cn, n_g;
  long long per;                      // N C n_g: the item's threads
  long long base;                     // first thread
};
typedef ArgBatch<DwProject, DW_BATCH> DwProjectBatch;

constexpr int DW_GRID_MAX = CURV_PERSAMPLE_GRID_MAX;
constexpr int DW_GRID_BATCH = 8;      // items per launch of the grid reduction: an item carries its 2 x 16 grid values
struct DwGrid {
  const float* p;
  const float* T;
  const float* u;
  const float* v;                     // separable: v (C, n_g); dense (u null): V (C, n_g)
  float* out;
  long long t_cs, t_rs, v_rs, o_stride, o_hs;
  int Cn, n_g, H, first;
  float shift[DW_GRID_MAX], gain[DW_GRID_MAX];
  long long base;                     // first workgroup (= sample)
};
typedef ArgBatch<DwGrid, DW_GRID_BATCH> DwGridBatch;

constexpr int GRAM_MAX_K = CURV_PERSAMPLE_COV_MAX_OUTPUTS;
constexpr int GRAM_MAX_PAIRS = GRAM_MAX_K * (GRAM_MAX_K + 1) / 2;
struct GramItem {
  const float* Y;
  float* out;
  long long y_ks, y_ns, o_ns, o_rs;
  int K, E, first;
  float alpha;
  long long base;                     // first workgroup (= sample)
};
typedef ArgBatch<GramItem, DW_BATCH> GramBatch;

static_assert(sizeof(DwBatch) <= 3840 && sizeof(DwSqBatch) <= 3840 && sizeof(DwQuadBatch) <= 3840 &&
              sizeof(DwProjectBatch) <= 3840 && sizeof(DwGridBatch) <= 3840 && sizeof(GramBatch) <= 3840,
              "kernel argument block must stay below 4 KB");

// ------------------------------------------------------------------------------------------------ phase 1
// The sums of one wave's share of a plane, KH x KW compiled in: acc[a KW + b], acc[KH KW] the bias sum.  `first` / `step`:
// the wave's first unit (an output, or a group of four) and the distance to its next.
template <int KH, int KW>
__device__ __forceinline__ void dw_plane_scalar(const DwItem& F, const float* __restrict__ xp, const float* __restrict__ gp,
                                                int first, int step, float (&acc)[KH * KW + 1]) {
  const int L = F.Ho * F.Wo, Wo = F.Wo, sh = F.sh, sw = F.sw, ph = F.ph, pw = F.pw;
  const unsigned H = F.H, W = F.W, x_sh = F.x_sh, x_sw = F.x_sw, g_sh = F.g_sh, g_sw = F.g_sw;
  const int d_oh = step / Wo, d_ow = step - d_oh * Wo;
  int oh = first / Wo, ow = first - oh * Wo;
  for (int l = first; l < L; l += step) {
    const float gv = gp[(unsigned)oh * g_sh + (unsigned)ow * g_sw];
#pragma unroll
    for (int a = 0; a < KH; ++a) {
      const unsigned ih = (unsigned)(oh * sh - ph + a);
#pragma unroll
      for (int b = 0; b < KW; ++b) {
        const unsigned iw = (unsigned)(ow * sw - pw + b);
        const bool ok = (ih < H) & (iw < W);
        const float xv = xp[ok ? ih * x_sh + iw * x_sw : 0u];          // a masked tap reads element 0 and drops it
        acc[a * KW + b] = fmaf(gv, ok ? xv : 0.0f, acc[a * KW + b]);
      }
    }
    acc[KH * KW] += gv;
    ow += d_ow; oh += d_oh;
    if (ow >= Wo) { ow -= Wo; ++oh; }
  }
}

// Four neighbouring outputs of one row per lane: Wo % 4 == 0, g_sw == 1 and every group of four of g 16-byte aligned
// (dw_item_of).  x is read per element (its window starts pw left of an aligned position), once for the four outputs.
template <int KH, int KW, int SW>
__device__ __forceinline__ void dw_plane_quads(const DwItem& F, const float* __restrict__ xp, const float* __restrict__ gp,
                                               int first, int step, float (&acc)[KH * KW + 1]) {
  constexpr int XW = 3 * SW + KW;
  const int Q = (F.Ho * F.Wo) >> 2, Wq = F.Wo >> 2, sh = F.sh, ph = F.ph, pw = F.pw;
  const unsigned H = F.H, W = F.W, x_sh = F.x_sh, x_sw = F.x_sw, g_sh = F.g_sh;
  const int d_oh = step / Wq, d_oq = step - d_oh * Wq;
  int oh = first / Wq, oq = first - oh * Wq;
  for (int q = first; q < Q; q += step) {
    const float4 g4 = *reinterpret_cast<const float4*>(gp + ((unsigned)oh * g_sh + (unsigned)oq * 4u));
    const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
    const int iw0 = oq * 4 * SW - pw;
#pragma unroll
    for (int a = 0; a < KH; ++a) {
      const unsigned ih = (unsigned)(oh * sh - ph + a);
      float xv[XW];
#pragma unroll
      for (int t = 0; t < XW; ++t) {
        const unsigned iw = (unsigned)(iw0 + t);
        const bool ok = (ih < H) & (iw < W);
        const float v = xp[ok ? ih * x_sh + iw * x_sw : 0u];
        xv[t] = ok ? v : 0.0f;
      }
#pragma unroll
      for (int b = 0; b < KW; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a * KW + b] = fmaf(gv[e], xv[e * SW + b], acc[a * KW + b]);
    }
    acc[KH * KW] += (gv[0] + gv[1]) + (gv[2] + gv[3]);
    oq += d_oq; oh += d_oh;
    if (oq >= Wq) { oq -= Wq; ++oh; }
  }
}

// The same with the x window read as whole aligned groups of four: the rows of x are 16-byte aligned runs, W % 4 == 0 and
// pw == KW / 2 (dw_item_of), so the window of the four outputs, x columns [4 SW oq - pw, .. + 3 SW + KW), lies inside the
// NQ aligned groups from column 4 (SW oq - 1) on; a group is inside the row or outside it as a whole.  Neighbouring lanes
// read neighbouring groups: every line a load instruction touches is used in full.
template <int KH, int KW, int SW>
__device__ __forceinline__ void dw_plane_quads_xvec(const DwItem& F, const float* __restrict__ xp,
                                                    const float* __restrict__ gp, int first, int step,
                                                    float (&acc)[KH * KW + 1]) {
  constexpr int LEAD = 4 - KW / 2;                   // window value t is value LEAD + t of the aligned run
  constexpr int XW = 3 * SW + KW, NQ = (LEAD + XW + 3) / 4;
  const int Q = (F.Ho * F.Wo) >> 2, Wq = F.Wo >> 2, sh = F.sh, ph = F.ph;
  const unsigned H = F.H, Wx = (unsigned)F.W >> 2, x_sh = F.x_sh, g_sh = F.g_sh;
  const int d_oh = step / Wq, d_oq = step - d_oh * Wq;
  int oh = first / Wq, oq = first - oh * Wq;
  for (int q = first; q < Q; q += step) {
    const float4 g4 = *reinterpret_cast<const float4*>(gp + ((unsigned)oh * g_sh + (unsigned)oq * 4u));
    const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
    const int q0 = oq * SW - 1;
#pragma unroll
    for (int a = 0; a < KH; ++a) {
      const unsigned ih = (unsigned)(oh * sh - ph + a);
      float xv[4 * NQ];
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const unsigned qi = (unsigned)(q0 + k);
        const bool ok = (ih < H) & (qi < Wx);
        const float4 v = *reinterpret_cast<const float4*>(xp + (ok ? ih * x_sh + qi * 4u : 0u));   // masked: group 0
        xv[4 * k + 0] = ok ? v.x : 0.0f; xv[4 * k + 1] = ok ? v.y : 0.0f;
        xv[4 * k + 2] = ok ? v.z : 0.0f; xv[4 * k + 3] = ok ? v.w : 0.0f;
      }
#pragma unroll
      for (int b = 0; b < KW; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a * KW + b] = fmaf(gv[e], xv[LEAD + e * SW + b], acc[a * KW + b]);
    }
    acc[KH * KW] += (gv[0] + gv[1]) + (gv[2] + gv[3]);
    oq += d_oq; oh += d_oh;
    if (oq >= Wq) { oq -= Wq; ++oh; }
  }
}

// One tap (a, b) of any kernel, or the bias sum (a < 0): the tap-at-a-time form of the kernels that are not compiled in.
__device__ __forceinline__ float dw_plane_tap(const DwItem& F, const float* __restrict__ xp, const float* __restrict__ gp,
                                              int first, int step, int a, int b) {
  const int L = F.Ho * F.Wo, Wo = F.Wo, sh = F.sh, sw = F.sw, ph = F.ph, pw = F.pw;
  const unsigned H = F.H, W = F.W, x_sh = F.x_sh, x_sw = F.x_sw, g_sh = F.g_sh, g_sw = F.g_sw;
  const int d_oh = step / Wo, d_ow = step - d_oh * Wo;
  int oh = first / Wo, ow = first - oh * Wo;
  float acc = 0.0f;
  for (int l = first; l < L; l += step) {
    const float gv = gp[(unsigned)oh * g_sh + (unsigned)ow * g_sw];
    if (a < 0) {
      acc += gv;
    } else {
      const unsigned ih = (unsigned)(oh * sh - ph + a), iw = (unsigned)(ow * sw - pw + b);
      const bool ok = (ih < H) & (iw < W);
      const float xv = xp[ok ? ih * x_sh + iw * x_sw : 0u];
      acc = fmaf(gv, ok ? xv : 0.0f, acc);
    }
    ow += d_ow; oh += d_oh;
    if (ow >= Wo) { ow -= Wo; ++oh; }
  }
  return acc;
}

// The sum over the workgroup's waves of value j (already summed over each wave, in its lane 63), written to dst[j]:
// through LDS where the four waves share the plane, directly otherwise.
__device__ __forceinline__ void dw_store(float v, int j, bool split, float* __restrict__ dst, float (*lds)[DW_MAX_TAPS + 1]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 63) {
    if (split) lds[wave][j] = v;
    else dst[j] = v;
  }
}

// KH = 0: the tap-at-a-time form.  MODE 0: one output per lane and step; 1 / 2: four, with stride 1 / 2 along w;
// 3 / 4: the same with x read in aligned groups of four.
template <int KH, int KW, int MODE>
__global__ void __launch_bounds__(DW_THREADS) ps_dw_product_kernel(const DwBatch batch) {
  __shared__ float lds[DW_WAVES][DW_MAX_TAPS + 1];
  const DwItem& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)((long long)blockIdx.x - F.base);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool split = F.split != 0;                       // uniform over the workgroup: it belongs to one item
  const int plane = split ? local : local * DW_WAVES + wave;
  const int planes = F.N * F.C;
  if (plane >= planes) return;                           // (only without `split`: no barrier follows for these waves)
  const int n = plane / F.C, c = plane - n * F.C;
  const float* xp = F.x + ((long long)n * F.x_sn + (long long)c * F.x_sc);
  const float* gp = F.g + ((long long)n * F.g_sn + (long long)c * F.g_sc);
  float* dst = F.p + (long long)plane * F.n_g;
  const int first = split ? (int)threadIdx.x : lane, step = split ? DW_THREADS : 64;
  const int n_g = F.n_g, taps = F.kh * F.kw;
  if constexpr (KH == 0) {
    const int kw = F.kw;
    for (int j = 0; j < n_g; ++j) {
      const int a = j < taps ? j / kw : -1, b = j < taps ? j - a * kw : 0;
      const float v = wave_sum_dpp(dw_plane_tap(F, xp, gp, first, step, a, b));
      dw_store(v, j, split, dst, lds);
    }
  } else {
    float acc[KH * KW + 1];
#pragma unroll
    for (int j = 0; j <= KH * KW; ++j) acc[j] = 0.0f;
    if constexpr (MODE == 0) dw_plane_scalar<KH, KW>(F, xp, gp, first, step, acc);
    else if constexpr (MODE <= 2) dw_plane_quads<KH, KW, MODE>(F, xp, gp, first, step, acc);
    else dw_plane_quads_xvec<KH, KW, MODE - 2>(F, xp, gp, first, step, acc);
#pragma unroll
    for (int j = 0; j <= KH * KW; ++j) {
      const float v = wave_sum_dpp(acc[j]);
      if (j < n_g) dw_store(v, j, split, dst, lds);
    }
  }
  if (split) {
    __syncthreads();
    if ((int)threadIdx.x < n_g) {
      float v = lds[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < DW_WAVES; ++w) v += lds[w][threadIdx.x];
      dst[threadIdx.x] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ phase 2
// C[c c_rs + j] (+)= alpha sum_n p[n, c, j]**2: one thread per (c, j), the samples in order.
__global__ void __launch_bounds__(DW_THREADS) ps_dw_sq_kernel(const DwSqBatch batch) {
  const long long t = (long long)blockIdx.x * DW_THREADS + threadIdx.x;
  const DwSq& F = batch.e[owner_of(batch, t)];
  const int per = F.Cn * F.n_g;
  if (t - F.base >= per) return;
  const int at = (int)(t - F.base);
  const int c = at / F.n_g, j = at - c * F.n_g;
  float sum = 0.0f;
  for (int n = 0; n < F.N; ++n) {
    const float v = F.p[(long long)n * per + at];
    sum = fmaf(v, v, sum);
  }
  float* out = F.C + ((long long)c * F.c_rs + j);
  *out = F.first ? F.alpha * sum : *out + F.alpha * sum;
}

// out[n o_stride] (+)= alpha sum_c s[c]**2 sum_j W[c w_rs + j] (sum_i T[c t_cs + i t_rs + j] p[n, c, i])**2: one workgroup
// per sample; a thread takes the channels c = thread, thread + 256, ... in order, then lane, wave, workgroup.
__global__ void __launch_bounds__(DW_THREADS) ps_dw_quad_kernel(const DwQuadBatch batch) {
  __shared__ float lds[DW_WAVES];
  const DwQuad& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int n = (int)((long long)blockIdx.x - F.base);
  const int n_g = F.n_g;
  float sum = 0.0f;
  for (int c = threadIdx.x; c < F.Cn; c += DW_THREADS) {
    const float* __restrict__ p = F.p + ((long long)n * F.Cn + c) * n_g;
    const float* __restrict__ T = F.T ? F.T + (long long)c * F.t_cs : nullptr;
    const float* __restrict__ W = F.W ? F.W + (long long)c * F.w_rs : nullptr;
    float v = 0.0f;
    for (int j = 0; j < n_g; ++j) {
      float y;
      if (T) {
        y = 0.0f;
        for (int i = 0; i < n_g; ++i) y = fmaf(T[(long long)i * F.t_rs + j], p[i], y);
      } else {
        y = p[j];
      }
      v = fmaf(W ? W[j] * y : y, y, v);
    }
    const float sc = F.s ? F.s[c] : 1.0f;
    sum = fmaf(sc * sc, v, sum);
  }
  sum = wave_sum_dpp(sum);
  if ((threadIdx.x & 63) == 63) lds[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = lds[0];
#pragma unroll
    for (int w = 1; w < DW_WAVES; ++w) v += lds[w];
    float* out = F.out + (long long)n * F.o_stride;
    *out = F.first ? F.alpha * v : *out + F.alpha * v;
  }
}

// y[n y_ns + c n_g + j] = s[c] W[c w_rs + j] sum_i T[c t_cs + i t_rs + j] p[n, c, i]: one thread per (n, c, j), the i in
// order; neighbouring threads read neighbouring j of T.
__global__ void __launch_bounds__(DW_THREADS) ps_dw_project_kernel(const DwProjectBatch batch) {
  const long long t = (long long)blockIdx.x * DW_THREADS + threadIdx.x;
  const DwProject& F = batch.e[owner_of(batch, t)];
  const long long at = t - F.base;
  if (at >= F.per) return;
  const int n_g = F.n_g, row = F.Cn * n_g;
  const long long n = at / row;
  const int cj = (int)(at - n * row), c = cj / n_g, j = cj - c * n_g;
  const float* __restrict__ p = F.p + (n * F.Cn + c) * n_g;
  float y;
  if (F.T) {
    const float* __restrict__ T = F.T + (long long)c * F.t_cs + j;
    y = 0.0f;
    for (int i = 0; i < n_g; ++i) y = fmaf(T[(long long)i * F.t_rs], p[i], y);
  } else {
    y = p[j];
  }
  if (F.W) y *= F.W[(long long)c * F.w_rs + j];
  if (F.s) y *= F.s[c];
  F.y[n * F.y_ns + cj] = y;
}

// out[h o_hs + n o_stride] (+)= gain[h] sum_c sum_j w_h(c, j) (sum_i T[c t_cs + i t_rs + j] p[n, c, i])**2: one workgroup
// per sample; a thread takes the channels c = thread, thread + 256, ... and their j in order, one chain per grid point,
// then lane, wave, workgroup.  Grid point h sees shift[h] and gain[h] only.
__global__ void __launch_bounds__(DW_THREADS) ps_dw_grid_kernel(const DwGridBatch batch) {
  __shared__ float lds[DW_WAVES][DW_GRID_MAX];
  const DwGrid& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int n = (int)((long long)blockIdx.x - F.base);
  const int n_g = F.n_g, H = F.H;
  float acc[DW_GRID_MAX];
#pragma unroll
  for (int h = 0; h < DW_GRID_MAX; ++h) acc[h] = 0.0f;
  for (int c = threadIdx.x; c < F.Cn; c += DW_THREADS) {
    const float* __restrict__ p = F.p + ((long long)n * F.Cn + c) * n_g;
    const float* __restrict__ T = F.T ? F.T + (long long)c * F.t_cs : nullptr;
    const float* __restrict__ v = F.v + (long long)c * F.v_rs;
    const float uc = F.u ? F.u[c] : 0.0f;
    for (int j = 0; j < n_g; ++j) {
      float y;
      if (T) {
        y = 0.0f;
        for (int i = 0; i < n_g; ++i) y = fmaf(T[(long long)i * F.t_rs + j], p[i], y);
      } else {
        y = p[j];
      }
      const float y2 = y * y, vj = v[j];
#pragma unroll
      for (int h = 0; h < DW_GRID_MAX; ++h)
        if (h < H) {
          const float sh = F.shift[h];
          const float w = F.u ? 1.0f / ((uc + sh) * (vj + sh)) : 1.0f / (vj + sh);
          acc[h] = fmaf(w, y2, acc[h]);
        }
    }
  }
#pragma unroll
  for (int h = 0; h < DW_GRID_MAX; ++h) {
    const float v = wave_sum_dpp(acc[h]);
    if ((threadIdx.x & 63) == 63) lds[threadIdx.x >> 6][h] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < H) {
    const int h = threadIdx.x;
    float v = lds[0][h];
#pragma unroll
    for (int w = 1; w < DW_WAVES; ++w) v += lds[w][h];
    float* out = F.out + ((long long)h * F.o_hs + (long long)n * F.o_stride);
    *out = F.first ? F.gain[h] * v : *out + F.gain[h] * v;
  }
}

// out[n o_ns + k o_rs + k'] (+)= alpha sum_e Y[k y_ks + n y_ns + e] Y[k' y_ks + n y_ns + e]: one workgroup per sample; a
// thread takes e = thread, thread + 256, ... in order with one chain per pair k <= k' in registers (KT: the compiled-in
// number of outputs, K <= KT; the outputs from K on read as 0), then lane, wave, workgroup.  One value per pair goes to
// both triangles.
template <int KT>
__global__ void __launch_bounds__(DW_THREADS) ps_gram_kernel(const GramBatch batch) {
  constexpr int PAIRS = KT * (KT + 1) / 2;
  __shared__ float lds[DW_WAVES][PAIRS];
  const GramItem& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int n = (int)((long long)blockIdx.x - F.base);
  const int K = F.K, E = F.E;
  const float* __restrict__ Y = F.Y + (long long)n * F.y_ns;
  float acc[PAIRS];
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) acc[q] = 0.0f;
  for (int e = threadIdx.x; e < E; e += DW_THREADS) {
    float y[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) y[k] = k < K ? Y[(long long)k * F.y_ks + e] : 0.0f;
    int q = 0;
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
      for (int l = k; l < KT; ++l, ++q) acc[q] = fmaf(y[k], y[l], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) {
    const float v = wave_sum_dpp(acc[q]);
    if ((threadIdx.x & 63) == 63) lds[threadIdx.x >> 6][q] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < PAIRS) {
    int k = 0, at = threadIdx.x;                       // pair `thread` of the KT-wide triangle is (k, l)
    while (at >= KT - k) { at -= KT - k; ++k; }
    const int l = k + at;
    if (l < K) {
      float v = lds[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < DW_WAVES; ++w) v += lds[w][threadIdx.x];
      v *= F.alpha;
      float* o = F.out + (long long)n * F.o_ns;
      float* upper = o + ((long long)k * F.o_rs + l);
      float* lower = o + ((long long)l * F.o_rs + k);
      const float r = F.first ? v : *upper + v;
      *upper = r;
      *lower = r;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// The largest offset (in elements) an (N, C, H, W) view with these strides addresses, or -1 if what one sample spans does
// not fit 31 bits.
long long dw_span(const long long dims[4], const long long strides[4], long long* inside) {
  const long long cap = 1LL << 31;
  long long span = 0;
  for (int k = 1; k < 4; ++k) {
    if (dims[k] > 1 && strides[k] >= cap) return -1;
    span += (dims[k] - 1) * strides[k];
    if (span >= cap) return -1;
  }
  *inside = span;
  return span;
}

// Item `index` as phase 1 reads it (without `p` and `base`), or false with the error text set.  `pointers`: also the
// records' addresses (the host-only queries do not need them).  `Desc`: any descriptor with the record, geometry and
// extent fields of curv_persample_dw_desc.
template <typename Desc>
bool dw_item_of(const Desc& d, int index, const char* who, bool pointers, DwItem* out) {
  side::ConvGeom geo;
  if (!side::conv_geom_of(d, who, "item", index, &geo)) return false;
  if (d.Ho != geo.Ho || d.Wo != geo.Wo) {
    set_error("%s: item %d: output %dx%d, but the geometry gives %dx%d (H %d W %d kernel %dx%d stride %dx%d padding %dx%d)",
              who, index, d.Ho, d.Wo, geo.Ho, geo.Wo, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw);
    return false;
  }
  if ((long long)d.kh * d.kw > DW_MAX_TAPS) {
    set_error("%s: item %d: kernel %dx%d has more than %d taps", who, index, d.kh, d.kw, DW_MAX_TAPS);
    return false;
  }
  const long long planes = (long long)d.N * d.C, L = (long long)d.Ho * d.Wo;
  if (planes >= (1LL << 29) || L >= (1LL << 29) || (long long)d.H * d.sh >= (1LL << 29) || (long long)d.W * d.sw >= (1LL << 29)) {
    set_error("%s: item %d: too large (%lld planes of %lld outputs)", who, index, planes, L);
    return false;
  }
  const long long xs[4] = {d.x_sn, d.x_sc, d.x_sh, d.x_sw}, gs[4] = {d.g_sn, d.g_sc, d.g_sh, d.g_sw};
  for (int k = 0; k < 4; ++k)
    if (xs[k] < 0 || gs[k] < 0) {
      set_error("%s: item %d: negative stride", who, index);
      return false;
    }
  const long long xd[4] = {d.N, d.C, d.H, d.W}, gd[4] = {d.N, d.C, d.Ho, d.Wo};
  long long x_in = 0, g_in = 0;
  if (dw_span(xd, xs, &x_in) < 0 || dw_span(gd, gs, &g_in) < 0) {
    set_error("%s: item %d: a sample spans 2^31 elements or more", who, index);
    return false;
  }
  // the largest addressed offset lies inside the stated extent (by a division: the product may not fit)
  if (d.x_elems < 1 || x_in >= d.x_elems || (d.N > 1 && d.x_sn > (d.x_elems - 1 - x_in) / (d.N - 1)) ||
      d.g_elems < 1 || g_in >= d.g_elems || (d.N > 1 && d.g_sn > (d.g_elems - 1 - g_in) / (d.N - 1))) {
    set_error("%s: item %d: a record's extent (x %lld, g %lld elements) is smaller than the largest offset its sizes and "
              "strides address", who, index, d.x_elems, d.g_elems);
    return false;
  }
  if (pointers) {
    if (!d.x || !d.g) {
      set_error("%s: item %d: null record", who, index);
      return false;
    }
    if ((reinterpret_cast<uintptr_t>(d.x) | reinterpret_cast<uintptr_t>(d.g)) & 3) {
      set_error("%s: item %d: a record is not aligned to its 4-byte elements", who, index);
      return false;
    }
  }
  DwItem F;
  F.x = d.x; F.g = d.g; F.p = nullptr;
  F.x_sn = d.N > 1 ? d.x_sn : 0; F.g_sn = d.N > 1 ? d.g_sn : 0;
  F.x_sc = (unsigned)(d.C > 1 ? d.x_sc : 0); F.x_sh = (unsigned)(d.H > 1 ? d.x_sh : 0); F.x_sw = (unsigned)(d.W > 1 ? d.x_sw : 0);
  F.g_sc = (unsigned)(d.C > 1 ? d.g_sc : 0); F.g_sh = (unsigned)(d.Ho > 1 ? d.g_sh : 0); F.g_sw = (unsigned)(d.Wo > 1 ? d.g_sw : 0);
  F.N = d.N; F.C = d.C; F.H = d.H; F.W = d.W; F.Ho = d.Ho; F.Wo = d.Wo;
  F.kh = d.kh; F.kw = d.kw; F.sh = d.sh; F.sw = d.sw; F.ph = d.ph; F.pw = d.pw;
  F.has_bias = d.has_bias ? 1 : 0;
  F.n_g = d.kh * d.kw + F.has_bias;
  F.split = L >= DW_SPLIT_L;
  // four outputs per lane: whole groups of four per output row, each one aligned 16-byte run of g - decided here, per
  // item, from the address and the strides, so that the kernel's branch is uniform
  F.quads = d.Wo % 4 == 0 && d.g_sw == 1 && (d.Ho == 1 || d.g_sh % 4 == 0) && (d.C == 1 || d.g_sc % 4 == 0) &&
            (d.N == 1 || d.g_sn % 4 == 0) && (reinterpret_cast<uintptr_t>(d.g) & 15) == 0 && (d.sw == 1 || d.sw == 2);
  F.xvec = F.quads && d.pw == d.kw / 2 && d.W % 4 == 0 && d.x_sw == 1 && (d.H == 1 || d.x_sh % 4 == 0) &&
           (d.C == 1 || d.x_sc % 4 == 0) && (d.N == 1 || d.x_sn % 4 == 0) && (reinterpret_cast<uintptr_t>(d.x) & 15) == 0;
  F.base = 0;
  *out = F;
  return true;
}

size_t dw_p_bytes(const DwItem& F) { return align_up((size_t)F.N * F.C * F.n_g * sizeof(float), 256); }

// The kernel an item takes: (class, mode).  Classes 1, 3, 5, 7: that kernel squared; 0: tap at a time.
struct DwVariant { int k, mode; };
DwVariant dw_variant_of(const DwItem& F) {
  const bool square = F.kh == F.kw && (F.kh == 1 || F.kh == 3 || F.kh == 5 || F.kh == 7);
  if (!square) return {0, 0};
  return {F.kh, F.quads ? F.sw + 2 * F.xvec : 0};
}

typedef void (*DwKernel)(DwBatch);
DwKernel dw_kernel_of(DwVariant v) {
  switch (v.k * 8 + v.mode) {
    case 1 * 8 + 0: return ps_dw_product_kernel<1, 1, 0>;
    case 1 * 8 + 1: return ps_dw_product_kernel<1, 1, 1>;
    case 1 * 8 + 2: return ps_dw_product_kernel<1, 1, 2>;
    case 1 * 8 + 3: return ps_dw_product_kernel<1, 1, 3>;
    case 1 * 8 + 4: return ps_dw_product_kernel<1, 1, 4>;
    case 3 * 8 + 0: return ps_dw_product_kernel<3, 3, 0>;
    case 3 * 8 + 1: return ps_dw_product_kernel<3, 3, 1>;
    case 3 * 8 + 2: return ps_dw_product_kernel<3, 3, 2>;
    case 3 * 8 + 3: return ps_dw_product_kernel<3, 3, 3>;
    case 3 * 8 + 4: return ps_dw_product_kernel<3, 3, 4>;
    case 5 * 8 + 0: return ps_dw_product_kernel<5, 5, 0>;
    case 5 * 8 + 1: return ps_dw_product_kernel<5, 5, 1>;
    case 5 * 8 + 2: return ps_dw_product_kernel<5, 5, 2>;
    case 5 * 8 + 3: return ps_dw_product_kernel<5, 5, 3>;
    case 5 * 8 + 4: return ps_dw_product_kernel<5, 5, 4>;
    case 7 * 8 + 0: return ps_dw_product_kernel<7, 7, 0>;
    case 7 * 8 + 1: return ps_dw_product_kernel<7, 7, 1>;
    case 7 * 8 + 2: return ps_dw_product_kernel<7, 7, 2>;
    case 7 * 8 + 3: return ps_dw_product_kernel<7, 7, 3>;
    case 7 * 8 + 4: return ps_dw_product_kernel<7, 7, 4>;
    default: return ps_dw_product_kernel<0, 0, 0>;
  }
}

// Every item planned (nothing is launched before all are), `p` carved out of the workspace in call order.
template <typename Desc>
int dw_plan(const char* name, const Desc* descs, int n, void* workspace, size_t workspace_bytes,
            std::vector<DwItem>* items) {
  CURV_REQUIRE(descs, "%s: null descriptors", name);
  items->resize(n);
  size_t need = 0;
  for (int i = 0; i < n; ++i) {
    if (!dw_item_of(descs[i], i, name, true, &(*items)[i])) return CURV_ERR_INVALID;
    need += dw_p_bytes((*items)[i]);
  }
  const int rc = side::require_workspace(name, workspace, workspace_bytes, need, 256);
  if (rc != CURV_OK) return rc;
  size_t at = 0;
  for (DwItem& F : *items) {
    F.p = (float*)((char*)workspace + at);
    at += dw_p_bytes(F);
  }
  return CURV_OK;
}

// Phase 1 of all items: those of one kernel variant share their launches, in call order.
int dw_products(const char* name, hipStream_t stream, const std::vector<DwItem>& items) {
  std::vector<char> done(items.size(), 0);
  for (size_t i = 0; i < items.size(); ++i) {
    if (done[i]) continue;
    const DwVariant v = dw_variant_of(items[i]);
    std::vector<int> same;
    for (size_t k = i; k < items.size(); ++k) {
      const DwVariant w = dw_variant_of(items[k]);
      if (!done[k] && w.k == v.k && w.mode == v.mode) {
        same.push_back((int)k);
        done[k] = 1;
      }
    }
    DwKernel kernel = dw_kernel_of(v);
    const int rc = for_arg_batches<DwItem, DW_BATCH, 1>(
        (int)same.size(), name,
        [&](int k, DwItem* F, long long* blocks) {
          *F = items[same[k]];
          const long long planes = (long long)F->N * F->C;
          blocks[0] = F->split ? planes : cdivll(planes, DW_WAVES);
        },
        [](int, long long blocks) { return blocks; },
        [&](const DwBatch* b, const long long*, const unsigned* grid) {
          hipLaunchKernelGGL(kernel, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]);
          CURV_LAUNCH_CHECK();
          return CURV_OK;
        });
    if (rc != CURV_OK) return rc;
  }
  return CURV_OK;
}

}  // namespace

int dw_launch_sq(const char* name, hipStream_t stream, const DwSqArgs* items, int n) {
  return for_arg_batches<DwSq, DW_BATCH, 1>(
      n, name,
      [&](int i, DwSq* S, long long* threads) {
        const DwSqArgs& a = items[i];
        S->p = a.p; S->C = a.dst; S->c_rs = a.c_rs;
        S->N = a.N; S->Cn = a.C; S->n_g = a.n_g; S->first = a.first; S->alpha = a.alpha;
        threads[0] = align_up((size_t)a.C * a.n_g, DW_THREADS);          // an item's threads fill whole workgroups
      },
      [](int, long long threads) { return threads / DW_THREADS; },
      [&](const DwSqBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(ps_dw_sq_kernel, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

int dw_launch_quad(const char* name, hipStream_t stream, const DwQuadArgs* items, int n) {
  return for_arg_batches<DwQuad, DW_BATCH, 1>(
      n, name,
      [&](int i, DwQuad* Q, long long* blocks) {
        const DwQuadArgs& a = items[i];
        Q->p = a.p; Q->T = a.T; Q->W = a.W; Q->s = a.s; Q->out = a.out;
        Q->t_cs = a.t_cs; Q->t_rs = a.t_rs; Q->w_rs = a.w_rs; Q->o_stride = a.o_stride;
        Q->N = a.N; Q->Cn = a.C; Q->n_g = a.n_g; Q->first = a.first; Q->alpha = a.alpha;
        blocks[0] = a.N;
      },
      [](int, long long blocks) { return blocks; },
      [&](const DwQuadBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(ps_dw_quad_kernel, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

}  // namespace curv

using namespace curv;

extern "C" size_t curv_persample_dw_workspace_bytes(const curv_persample_dw_desc* descs, int n) {
  const char* const name = "curv_persample_dw_workspace_bytes";
  if (n <= 0) return 0;
  if (!descs) {
    set_error("%s: null descriptors", name);
    return 0;
  }
  size_t need = 0;
  for (int i = 0; i < n; ++i) {
    DwItem F;
    if (!dw_item_of(descs[i], i, name, false, &F)) return 0;
    need += dw_p_bytes(F);
  }
  return need;
}

extern "C" int curv_persample_dw_plan_info(const curv_persample_dw_desc* descs, int n, long long* flops, long long* bytes) {
  const char* const name = "curv_persample_dw_plan_info";
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs && (flops || bytes), "%s: null argument", name);
  for (int i = 0; i < n; ++i) {
    DwItem F;
    if (!dw_item_of(descs[i], i, name, false, &F)) return CURV_ERR_INVALID;
    const long long planes = (long long)F.N * F.C, L = (long long)F.Ho * F.Wo;
    if (flops) flops[i] = 2 * planes * L * F.n_g;
    if (bytes) bytes[i] = 4 * planes * ((long long)F.H * F.W + L);
  }
  return CURV_OK;
}

extern "C" int curv_persample_dw_sq_accumulate(void* stream_, const curv_persample_dw_desc* descs, int n, void* workspace,
                                               size_t workspace_bytes) {
  const char* const name = "curv_persample_dw_sq_accumulate";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<DwItem> items;
  int rc = dw_plan(name, descs, n, workspace, workspace_bytes, &items);
  if (rc != CURV_OK) return rc;
  for (int i = 0; i < n; ++i) {
    CURV_REQUIRE(descs[i].dst, "%s: item %d: null destination", name, i);
    CURV_REQUIRE(descs[i].c_rs >= items[i].n_g || descs[i].C == 1, "%s: item %d: c_rs %lld below n_g = %d", name, i,
                 descs[i].c_rs, items[i].n_g);
  }
  rc = dw_products(name, stream, items);
  if (rc != CURV_OK) return rc;
  std::vector<DwSqArgs> args(n);
  for (int i = 0; i < n; ++i) {
    const DwItem& F = items[i];
    args[i] = DwSqArgs{F.p, descs[i].dst, descs[i].c_rs, F.N, F.C, F.n_g, descs[i].first ? 1 : 0, descs[i].alpha};
  }
  return dw_launch_sq(name, stream, args.data(), n);
}

extern "C" int curv_persample_dw_quad_reduce(void* stream_, const curv_persample_dw_desc* descs, int n, void* workspace,
                                             size_t workspace_bytes) {
  const char* const name = "curv_persample_dw_quad_reduce";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<DwItem> items;
  int rc = dw_plan(name, descs, n, workspace, workspace_bytes, &items);
  if (rc != CURV_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const curv_persample_dw_desc& d = descs[i];
    CURV_REQUIRE(d.out, "%s: item %d: null destination", name, i);
    CURV_REQUIRE(d.o_stride >= 1 || d.N == 1, "%s: item %d: o_stride %lld below 1", name, i, d.o_stride);
    CURV_REQUIRE(!d.T || (d.t_rs >= 0 && d.t_cs >= 0), "%s: item %d: negative stride of T", name, i);
    CURV_REQUIRE(!d.Wt || d.w_rs >= 0, "%s: item %d: negative stride of W", name, i);
  }
  rc = dw_products(name, stream, items);
  if (rc != CURV_OK) return rc;
  std::vector<DwQuadArgs> args(n);
  for (int i = 0; i < n; ++i) {
    const DwItem& F = items[i];
    const curv_persample_dw_desc& d = descs[i];
    args[i] = DwQuadArgs{F.p, d.T, d.Wt, d.s, d.out, d.t_cs, d.t_rs, d.w_rs, d.o_stride, F.N, F.C, F.n_g, d.first ? 1 : 0,
                         d.alpha};
  }
  return dw_launch_quad(name, stream, args.data(), n);
}

// ------------------------------------------------------------------------------------------------ K15: project, grid, Gram
namespace curv {
namespace {

// The fields of item `index` behind its records, or false with the error text set.
bool dw_project_ok(const curv_persample_dw_project_desc& d, int index, const char* who, const DwItem& F, bool pointers) {
  const long long row = (long long)F.C * F.n_g;
  if (row >= (1LL << 31)) {
    set_error("%s: item %d: too large (%lld values per sample)", who, index, row);
    return false;
  }
  if (d.y_ns < row && d.N > 1) {
    set_error("%s: item %d: y_ns %lld below C n_g = %lld", who, index, d.y_ns, row);
    return false;
  }
  if ((d.T && (d.t_rs < 0 || d.t_cs < 0)) || (d.Wt && d.w_rs < 0)) {
    set_error("%s: item %d: negative stride of T or W", who, index);
    return false;
  }
  if (pointers && !d.y) {
    set_error("%s: item %d: null destination", who, index);
    return false;
  }
  return true;
}

bool dw_grid_ok(const curv_persample_dw_grid_desc& d, int index, const char* who, const DwItem&, bool pointers) {
  if (d.Hn < 1 || d.Hn > DW_GRID_MAX || !d.shift || !d.gain) {
    set_error("%s: item %d: H %d (1 to %d grid points, with their shift and gain)", who, index, d.Hn, DW_GRID_MAX);
    return false;
  }
  for (int h = 0; h < d.Hn; ++h)
    if (!(d.shift[h] > 0.0f) || !std::isfinite(d.shift[h]) || !std::isfinite(d.gain[h])) {
      set_error("%s: item %d: grid point %d: shift %g must be finite and > 0, gain %g finite", who, index, h,
                (double)d.shift[h], (double)d.gain[h]);
      return false;
    }
  if ((d.T && (d.t_rs < 0 || d.t_cs < 0)) || d.v_rs < 0) {
    set_error("%s: item %d: negative stride of T or of the weights", who, index);
    return false;
  }
  if ((d.o_stride < 1 && d.N > 1) || (d.o_hs < 1 && d.Hn > 1)) {
    set_error("%s: item %d: o_stride %lld or o_hs %lld below 1", who, index, d.o_stride, d.o_hs);
    return false;
  }
  if (!pointers) return true;
  const bool separable = d.u != nullptr;
  if (!d.out || (separable ? (!d.v || d.V) : (!d.V || d.v))) {
    set_error("%s: item %d: null destination, or weights given neither as u and v (separable) nor as V (dense)", who, index);
    return false;
  }
  return true;
}

template <typename Desc, typename Check>
size_t dw_workspace_bytes_of(const char* name, const Desc* descs, int n, Check check) {
  if (n <= 0) return 0;
  if (!descs) {
    set_error("%s: null descriptors", name);
    return 0;
  }
  size_t need = 0;
  for (int i = 0; i < n; ++i) {
    DwItem F;
    if (!dw_item_of(descs[i], i, name, false, &F) || !check(descs[i], i, name, F, false)) return 0;
    need += dw_p_bytes(F);
  }
  return need;
}

// Per item the FLOPs of phase 1 and of the reduction behind it (`after(F, d)`), and the bytes the algorithm needs.
template <typename Desc, typename Check, typename After>
int dw_plan_info_of(const char* name, const Desc* descs, int n, long long* flops, long long* bytes, Check check, After after) {
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs && (flops || bytes), "%s: null argument", name);
  for (int i = 0; i < n; ++i) {
    DwItem F;
    if (!dw_item_of(descs[i], i, name, false, &F) || !check(descs[i], i, name, F, false)) return CURV_ERR_INVALID;
    const long long planes = (long long)F.N * F.C, L = (long long)F.Ho * F.Wo;
    long long extra_flops = 0, extra_bytes = 0;
    after(F, descs[i], &extra_flops, &extra_bytes);
    if (flops) flops[i] = 2 * planes * L * F.n_g + extra_flops;
    if (bytes) bytes[i] = 4 * planes * ((long long)F.H * F.W + L) + extra_bytes;
  }
  return CURV_OK;
}

void dw_project_cost(const DwItem& F, const curv_persample_dw_project_desc& d, long long* flops, long long* bytes) {
  const long long values = (long long)F.N * F.C * F.n_g;
  *flops = d.T ? 2 * values * F.n_g : 0;
  *bytes = 4 * values;                                                     // y written once
}

void dw_grid_cost(const DwItem& F, const curv_persample_dw_grid_desc& d, long long* flops, long long* bytes) {
  const long long values = (long long)F.N * F.C * F.n_g;
  *flops = (d.T ? 2 * values * F.n_g : 0) + 2 * values * d.Hn;
  *bytes = 0;
}

}  // namespace
}  // namespace curv

extern "C" size_t curv_persample_dw_project_workspace_bytes(const curv_persample_dw_project_desc* descs, int n) {
  return dw_workspace_bytes_of("curv_persample_dw_project_workspace_bytes", descs, n, dw_project_ok);
}

extern "C" int curv_persample_dw_project_plan_info(const curv_persample_dw_project_desc* descs, int n, long long* flops,
                                                   long long* bytes) {
  return dw_plan_info_of("curv_persample_dw_project_plan_info", descs, n, flops, bytes, dw_project_ok, dw_project_cost);
}

extern "C" size_t curv_persample_dw_quad_grid_workspace_bytes(const curv_persample_dw_grid_desc* descs, int n) {
  return dw_workspace_bytes_of("curv_persample_dw_quad_grid_workspace_bytes", descs, n, dw_grid_ok);
}

extern "C" int curv_persample_dw_quad_grid_plan_info(const curv_persample_dw_grid_desc* descs, int n, long long* flops,
                                                     long long* bytes) {
  return dw_plan_info_of("curv_persample_dw_quad_grid_plan_info", descs, n, flops, bytes, dw_grid_ok, dw_grid_cost);
}

extern "C" int curv_persample_dw_project(void* stream_, const curv_persample_dw_project_desc* descs, int n, void* workspace,
                                         size_t workspace_bytes) {
  const char* const name = "curv_persample_dw_project";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<DwItem> items;
  int rc = dw_plan(name, descs, n, workspace, workspace_bytes, &items);
  if (rc != CURV_OK) return rc;
  for (int i = 0; i < n; ++i)
    if (!dw_project_ok(descs[i], i, name, items[i], true)) return CURV_ERR_INVALID;
  rc = dw_products(name, stream, items);
  if (rc != CURV_OK) return rc;
  return for_arg_batches<DwProject, DW_BATCH, 1>(
      n, name,
      [&](int i, DwProject* P, long long* threads) {
        const DwItem& F = items[i];
        const curv_persample_dw_project_desc& d = descs[i];
        P->p = F.p; P->T = d.T; P->W = d.Wt; P->s = d.s; P->y = d.y;
        P->t_cs = d.t_cs; P->t_rs = d.t_rs; P->w_rs = d.w_rs; P->y_ns = F.N > 1 ? d.y_ns : 0;
        P->Cn = F.C; P->n_g = F.n_g; P->per = (long long)F.N * F.C * F.n_g;
        threads[0] = (long long)align_up((size_t)P->per, DW_THREADS);      // an item's threads fill whole workgroups
      },
      [](int, long long threads) { return threads / DW_THREADS; },
      [&](const DwProjectBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(ps_dw_project_kernel, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

extern "C" int curv_persample_dw_quad_grid_reduce(void* stream_, const curv_persample_dw_grid_desc* descs, int n,
                                                  void* workspace, size_t workspace_bytes) {
  const char* const name = "curv_persample_dw_quad_grid_reduce";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<DwItem> items;
  int rc = dw_plan(name, descs, n, workspace, workspace_bytes, &items);
  if (rc != CURV_OK) return rc;
  for (int i = 0; i < n; ++i)
    if (!dw_grid_ok(descs[i], i, name, items[i], true)) return CURV_ERR_INVALID;
  rc = dw_products(name, stream, items);
  if (rc != CURV_OK) return rc;
  return for_arg_batches<DwGrid, DW_GRID_BATCH, 1>(
      n, name,
      [&](int i, DwGrid* Q, long long* blocks) {
        const DwItem& F = items[i];
        const curv_persample_dw_grid_desc& d = descs[i];
        Q->p = F.p; Q->T = d.T; Q->u = d.u; Q->v = d.u ? d.v : d.V; Q->out = d.out;
        Q->t_cs = d.t_cs; Q->t_rs = d.t_rs; Q->v_rs = d.v_rs; Q->o_stride = d.o_stride; Q->o_hs = d.o_hs;
        Q->Cn = F.C; Q->n_g = F.n_g; Q->H = d.Hn; Q->first = d.first ? 1 : 0;
        for (int h = 0; h < DW_GRID_MAX; ++h) {                            // (the slots from H on repeat the last point)
          Q->shift[h] = d.shift[std::min(h, d.Hn - 1)];
          Q->gain[h] = d.gain[std::min(h, d.Hn - 1)];
        }
        blocks[0] = F.N;
      },
      [](int, long long blocks) { return blocks; },
      [&](const DwGridBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(ps_dw_grid_kernel, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

extern "C" int curv_persample_gram_reduce(void* stream_, const curv_persample_gram_desc* descs, int n) {
  const char* const name = "curv_persample_gram_reduce";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  CURV_REQUIRE(descs, "%s: null descriptors", name);
  for (int i = 0; i < n; ++i) {
    const curv_persample_gram_desc& d = descs[i];
    CURV_REQUIRE(d.K >= 1 && d.K <= GRAM_MAX_K, "%s: item %d: K %d (1 to %d outputs)", name, i, d.K, GRAM_MAX_K);
    CURV_REQUIRE(d.N >= 1 && d.E >= 1, "%s: item %d: invalid sizes (N %d, E %d)", name, i, d.N, d.E);
    CURV_REQUIRE(d.y_ks >= 0 && d.y_ns >= 0, "%s: item %d: negative stride of Y", name, i);
    CURV_REQUIRE(d.o_rs >= d.K && (d.N == 1 || d.o_ns >= d.K * d.o_rs), "%s: item %d: o_rs %lld below K = %d or o_ns %lld "
                 "below K o_rs", name, i, d.o_rs, d.K, d.o_ns);
    CURV_REQUIRE(d.Y && d.out, "%s: item %d: null operand or destination", name, i);
    CURV_REQUIRE(((reinterpret_cast<uintptr_t>(d.Y) | reinterpret_cast<uintptr_t>(d.out)) & 3) == 0,
                 "%s: item %d: an address is not aligned to its 4-byte elements", name, i);
  }
  // the items of one compiled-in width share their launches, in call order
  const int widths[] = {1, 4, 8, 16};
  for (int KT : widths) {
    std::vector<int> same;
    for (int i = 0; i < n; ++i) {
      int kt = 1;
      while (kt < descs[i].K) kt = kt == 1 ? 4 : 2 * kt;
      if (kt == KT) same.push_back(i);
    }
    const int rc = for_arg_batches<GramItem, DW_BATCH, 1>(
        (int)same.size(), name,
        [&](int k, GramItem* G, long long* blocks) {
          const curv_persample_gram_desc& d = descs[same[k]];
          G->Y = d.Y; G->out = d.out;
          G->y_ks = d.K > 1 ? d.y_ks : 0; G->y_ns = d.N > 1 ? d.y_ns : 0; G->o_ns = d.N > 1 ? d.o_ns : 0; G->o_rs = d.o_rs;
          G->K = d.K; G->E = d.E; G->first = d.first ? 1 : 0; G->alpha = d.alpha;
          blocks[0] = d.N;
        },
        [](int, long long blocks) { return blocks; },
        [&](const GramBatch* b, const long long*, const unsigned* grid) {
          switch (KT) {
            case 1: hipLaunchKernelGGL(ps_gram_kernel<1>, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]); break;
            case 4: hipLaunchKernelGGL(ps_gram_kernel<4>, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]); break;
            case 8: hipLaunchKernelGGL(ps_gram_kernel<8>, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]); break;
            default: hipLaunchKernelGGL(ps_gram_kernel<16>, dim3(grid[0]), dim3(DW_THREADS), 0, stream, b[0]); break;
          }
          CURV_LAUNCH_CHECK();
          return CURV_OK;
        });
    if (rc != CURV_OK) return rc;
  }
  return CURV_OK;
}
