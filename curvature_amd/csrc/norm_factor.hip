// Curvature of the affine parameters of LayerNorm, GroupNorm and eval-mode BatchNorm2d (curv_kfac_norm_accumulate,
// curv_persample_norm_sq_accumulate / curv_persample_norm_quad_reduce, include/curv_hip.h; DESIGN.md "K22").
//
// y[c] = gamma_c xh[c] + beta_c is a depthwise 1 x 1 convolution of the standardised input xh = (x - mu) rstd, so a layer is
// an item of the depthwise line with n_g = 1 + has_bias - if only xh existed.  It is not recorded, and writing it would cost
// a write and a read of every activation; the passes here form what the line needs straight from x and g:
//   1. norm_stats_kernel: one wave - from NORM_SPLIT_L elements on the four waves of a workgroup - per statistics set
//      ((n, group) or (n, h, w); none for given statistics).  Every lane runs Welford over its elements (count k, mean m,
//      centred sum M2); the set's mean is m_0 + sum k (m - m_0) / count and its variance sum (M2 + k (m - mean)^2) / count,
//      two plain sums in the order lane, wave (DPP), workgroup: centred throughout.  (mean, rstd) go to scratch: 2 floats
//      per set.
//   2. norm_product_kernel<FN>: per (n, c) the sums over the positions of FN 0: (g xh, g)   1: (xh^2, xh)   2: (g^2).
//      Lanes run along the contiguous axis.  Channel stride not 1: a wave or (from NORM_SPLIT_L positions on) a workgroup per
//      (n, c) plane, lanes along the positions.  Channel stride 1 (channels_last, LayerNorm): a thread per channel - or per
//      four, where C % 4 == 0 - over a slice of NORM_SLICE positions, in order: no sum crosses a lane.
//   3. the slices (and, for a factor, the samples) are summed in index order: norm_slices_kernel into p (N, C, n_g),
//      norm_factor_kernel into dst.  The per-sample entry points end in phase 2 of persample_dw.hip (persample_dw_phase2.h).
// Where four neighbouring elements are contiguous and the count is a multiple of four a lane takes them together: one 16-byte
// load where the record is aligned, four 4-byte loads where it is not - the same sums either way, so an item's bits follow
// from its sizes and strides only.  No atomics.  Nothing outside [0, extent) of a record is addressed: every offset is that
// of an index inside the view.
#include "kernarg.h"
#include "persample_dw_phase2.h"
#include "side_build.h"
#include "wave_sum.h"

#include <cmath>
#include <vector>

namespace curv {
namespace {

constexpr int NORM_THREADS = 256;     // four waves
constexpr int NORM_WAVES = NORM_THREADS / 64;
constexpr int NORM_BATCH = 16;        // items per launch
constexpr int NORM_SPLIT_L = CURV_NORM_SPLIT_L;
constexpr int NORM_SLICE = CURV_NORM_SLICE;

// One record ((N, C, L) with L = H W positions) as the kernels address it.
struct NormRecord {
  const float* at;
  long long sn;
  unsigned sc, sh, sw;
  unsigned sl;                        // flat: position l lies at l * sl
  int flat;
  int al_l, al_c;                     // four neighbouring positions of a plane / channels of a position lie in one aligned
};                                    // 16-byte group (address and the strides of the other axes multiples of four)

struct NormItem {
  NormRecord x, g;
  const float* mean;
  const float* var;
  float* stats;                       // (N, sets, 2): mean, rstd
  float* part;                        // (N, S, C, K)
  float* p;                           // (N, C, K): the slices summed (S > 1, per-sample entry points)
  int N, C, W, L;
  int mode, G, cg;
  int K;                              // values kept per (n, c)
  int S;                              // slices of the positions (1 where lanes run along them)
  int cfast, cvec;                    // lanes along c; four channels per thread
  int split_p, quads_p;               // a workgroup per plane; four positions per lane
  int sets, set_cnt;                  // statistics sets per sample, elements of one
  int split_s, run_s, quads_s;        // a workgroup per set; the set is one contiguous run; four elements per lane
  int al_s;                           // ... that lie in one aligned 16-byte group
  int outer_l, inner;                 // the set seen as outer x inner: the outer index is the position (else the channel)
  float eps;
  long long base;
};
typedef ArgBatch<NormItem, NORM_BATCH> NormBatch;

struct NormSum {
  const float* part;
  float* dst;                         // slices: p; factor: dst
  int N, S, C, K;
  int n_g, side, first;
  float scale, count;
  long long base;                     // first thread (slices) / workgroup (factor)
};
typedef ArgBatch<NormSum, NORM_BATCH> NormSumBatch;

static_assert(sizeof(NormBatch) <= 3840 && sizeof(NormSumBatch) <= 3840, "kernel argument block must stay below 4 KB");

__device__ __forceinline__ unsigned norm_loff(const NormRecord& r, unsigned l, unsigned W) {
  if (r.flat) return l * r.sl;
  const unsigned h = l / W;
  return h * r.sh + (l - h * W) * r.sw;
}

// Four neighbouring values: one 16-byte load where the record is aligned.
__device__ __forceinline__ void norm_load4(const float* __restrict__ at, bool aligned, float (&v)[4]) {
  if (aligned) {
    const float4 q = *reinterpret_cast<const float4*>(at);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = at[0]; v[1] = at[1]; v[2] = at[2]; v[3] = at[3];
  }
}

struct Welford {
  float k, m, M2;
  __device__ __forceinline__ void push(float v) {
    k += 1.0f;
    const float d = v - m;
    m += d * __builtin_amdgcn_rcpf(k);
    M2 = fmaf(d, v - m, M2);
  }
};

// The sum of `v` over the team (a wave, or the workgroup's waves in order), in every thread.
__device__ __forceinline__ float norm_team_sum(float v, bool split, float* lds) {
  v = wave_sum_dpp(v);
  v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
  if (!split) return v;
  __syncthreads();                                       // (the previous sum has been read)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = lds[0];
#pragma unroll
  for (int w = 1; w < NORM_WAVES; ++w) s += lds[w];
  return s;
}

// The value thread 0 of the team holds, in every thread.
__device__ __forceinline__ float norm_team_first(float v, bool split, float* lds) {
  v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  if (!split) return v;
  if (threadIdx.x == 0) lds[0] = v;
  __syncthreads();
  return lds[0];
}

// ------------------------------------------------------------------------------------------------ 1: statistics
__global__ void __launch_bounds__(NORM_THREADS) norm_stats_kernel(const NormBatch batch) {
  __shared__ float lds[NORM_WAVES];
  const NormItem& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)((long long)blockIdx.x - F.base);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool split = F.split_s != 0;                     // uniform over the workgroup: it belongs to one item
  const long long set = split ? local : (long long)local * NORM_WAVES + wave;
  if (set >= (long long)F.N * F.sets) return;            // (only without `split`: no barrier follows for these waves)
  const int n = (int)(set / F.sets), j = (int)(set - (long long)n * F.sets);
  const unsigned W = F.W;
  const float* __restrict__ xs = F.x.at + (long long)n * F.x.sn +
      (F.mode == CURV_NORM_GROUP ? (unsigned)(j * F.cg) * F.x.sc : norm_loff(F.x, (unsigned)j, W));
  const int first = split ? (int)threadIdx.x : lane, step = split ? NORM_THREADS : 64;
  const int cnt = F.set_cnt;
  Welford w{0.0f, 0.0f, 0.0f};
  if (F.run_s) {
    if (F.quads_s) {
      const bool aligned = F.al_s != 0;
      for (int q = first; q < (cnt >> 2); q += step) {
        float v[4];
        norm_load4(xs + 4u * (unsigned)q, aligned, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) w.push(v[e]);
      }
    } else {
      for (int e = first; e < cnt; e += step) w.push(xs[e]);
    }
  } else {
    const int inner = F.inner;
    const int d_a = step / inner, d_b = step - d_a * inner;
    int a = first / inner, b = first - a * inner;
    for (int e = first; e < cnt; e += step) {
      const unsigned off = F.outer_l ? norm_loff(F.x, (unsigned)a, W) + (unsigned)b * F.x.sc
                                     : (unsigned)a * F.x.sc + norm_loff(F.x, (unsigned)b, W);
      w.push(xs[off]);
      b += d_b; a += d_a;
      if (b >= inner) { b -= inner; ++a; }
    }
  }
  const float count = (float)cnt;
  // the lanes' means are summed as differences from thread 0's (it always has an element): the rounding of that sum is
  // relative to the spread of the data, not to its offset
  const float ref = norm_team_first(w.m, split, lds);
  const float mean = ref + norm_team_sum(w.k * (w.m - ref), split, lds) / count;
  const float dm = w.m - mean;
  const float var = norm_team_sum(fmaf(w.k * dm, dm, w.M2), split, lds) / count;
  if (split ? threadIdx.x == 0 : lane == 0) {
    float* st = F.stats + 2 * set;
    st[0] = mean;
    st[1] = 1.0f / sqrtf(var + F.eps);
  }
}

// ------------------------------------------------------------------------------------------------ 2: products
template <int FN>
__device__ __forceinline__ void norm_take(float xv, float gv, float mu, float rs, float& a0, float& a1) {
  if constexpr (FN == 0) {
    a0 = fmaf(gv, (xv - mu) * rs, a0);
    a1 += gv;
  } else if constexpr (FN == 1) {
    const float xh = (xv - mu) * rs;
    a0 = fmaf(xh, xh, a0);
    a1 += xh;
  } else {
    a0 = fmaf(gv, gv, a0);
  }
}

// (mean, rstd) of channel c of sample n where they do not depend on the position.
template <int FN>
__device__ __forceinline__ void norm_channel_stats(const NormItem& F, int n, int c, float& mu, float& rs) {
  mu = 0.0f; rs = 1.0f;
  if constexpr (FN != 2) {
    if (F.mode == CURV_NORM_GROUP) {
      const float* st = F.stats + 2 * ((long long)n * F.G + c / F.cg);
      mu = st[0]; rs = st[1];
    } else if (F.mode == CURV_NORM_GIVEN) {
      mu = F.mean[c];
      rs = 1.0f / sqrtf(F.var[c] + F.eps);
    }
  }
}

// Lanes along the positions: a wave or a workgroup per (n, c) plane.
template <int FN>
__device__ __forceinline__ void norm_plane_body(const NormItem& F, int local, float (*lds)[2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool split = F.split_p != 0;
  const long long plane = split ? local : (long long)local * NORM_WAVES + wave;
  if (plane >= (long long)F.N * F.C) return;             // (only without `split`)
  const int n = (int)(plane / F.C), c = (int)(plane - (long long)n * F.C);
  const float* __restrict__ xp = FN != 2 ? F.x.at + ((long long)n * F.x.sn + (long long)c * F.x.sc) : nullptr;
  const float* __restrict__ gp = FN != 1 ? F.g.at + ((long long)n * F.g.sn + (long long)c * F.g.sc) : nullptr;
  float mu, rs;
  norm_channel_stats<FN>(F, n, c, mu, rs);
  const bool by_position = FN != 2 && F.mode == CURV_NORM_POSITION;
  const float* __restrict__ st = by_position ? F.stats + 2 * (long long)n * F.L : nullptr;
  const int first = split ? (int)threadIdx.x : lane, step = split ? NORM_THREADS : 64;
  const int L = F.L;
  const unsigned W = F.W;
  float a0 = 0.0f, a1 = 0.0f;
  if (F.quads_p) {                                       // unit position strides, L % 4 == 0, statistics per channel
    const bool x_al = F.x.al_l != 0, g_al = F.g.al_l != 0;
    for (int q = first; q < (L >> 2); q += step) {
      float xv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (FN != 2) norm_load4(xp + 4u * (unsigned)q, x_al, xv);
      if constexpr (FN != 1) norm_load4(gp + 4u * (unsigned)q, g_al, gv);
#pragma unroll
      for (int e = 0; e < 4; ++e) norm_take<FN>(xv[e], gv[e], mu, rs, a0, a1);
    }
  } else {
    for (int l = first; l < L; l += step) {
      float xv = 0.0f, gv = 0.0f;
      if constexpr (FN != 2) xv = xp[norm_loff(F.x, (unsigned)l, W)];
      if constexpr (FN != 1) gv = gp[norm_loff(F.g, (unsigned)l, W)];
      if (by_position) { mu = st[2 * l]; rs = st[2 * l + 1]; }
      norm_take<FN>(xv, gv, mu, rs, a0, a1);
    }
  }
  a0 = wave_sum_dpp(a0);
  a1 = wave_sum_dpp(a1);
  float* dst = F.part + plane * F.K;
  if (!split) {
    if (lane == 63) {
      dst[0] = a0;
      if (F.K > 1) dst[1] = a1;
    }
    return;
  }
  if (lane == 63) { lds[wave][0] = a0; lds[wave][1] = a1; }
  __syncthreads();
  if ((int)threadIdx.x < F.K) {
    float v = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < NORM_WAVES; ++w) v += lds[w][threadIdx.x];
    dst[threadIdx.x] = v;
  }
}

// Lanes along the channels: a thread per V channels over one slice of the positions, in order.
template <int FN, int V>
__device__ __forceinline__ void norm_chan_body(const NormItem& F, int local) {
  const int Ct = F.C / V, cblocks = (Ct + NORM_THREADS - 1) / NORM_THREADS;
  const int cb = local % cblocks, t = local / cblocks;
  const int s = t % F.S, n = t / F.S;
  const int ct = cb * NORM_THREADS + (int)threadIdx.x;
  if (ct >= Ct) return;
  const int c0 = ct * V;
  const float* __restrict__ xp = FN != 2 ? F.x.at + ((long long)n * F.x.sn + (long long)c0 * F.x.sc) : nullptr;
  const float* __restrict__ gp = FN != 1 ? F.g.at + ((long long)n * F.g.sn + (long long)c0 * F.g.sc) : nullptr;
  float mu[V], rs[V], a0[V], a1[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    norm_channel_stats<FN>(F, n, c0 + e, mu[e], rs[e]);
    a0[e] = 0.0f; a1[e] = 0.0f;
  }
  const bool by_position = FN != 2 && F.mode == CURV_NORM_POSITION;
  const float* __restrict__ st = by_position ? F.stats + 2 * (long long)n * F.L : nullptr;
  const unsigned W = F.W;
  const int l0 = s * NORM_SLICE, l1 = min(F.L, l0 + NORM_SLICE);
  for (int l = l0; l < l1; ++l) {
    float xv[V], gv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { xv[e] = 0.0f; gv[e] = 0.0f; }
    if constexpr (V == 4) {                              // (cvec: unit channel strides, aligned groups of four)
      float x4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (FN != 2) norm_load4(xp + norm_loff(F.x, (unsigned)l, W), true, x4);
      if constexpr (FN != 1) norm_load4(gp + norm_loff(F.g, (unsigned)l, W), true, g4);
#pragma unroll
      for (int e = 0; e < V; ++e) { xv[e] = x4[e]; gv[e] = g4[e]; }
    } else {
      if constexpr (FN != 2) xv[0] = xp[norm_loff(F.x, (unsigned)l, W)];
      if constexpr (FN != 1) gv[0] = gp[norm_loff(F.g, (unsigned)l, W)];
    }
    float m_l = 0.0f, r_l = 1.0f;
    if (by_position) { m_l = st[2 * l]; r_l = st[2 * l + 1]; }
#pragma unroll
    for (int e = 0; e < V; ++e) norm_take<FN>(xv[e], gv[e], by_position ? m_l : mu[e], by_position ? r_l : rs[e], a0[e], a1[e]);
  }
  float* dst = F.part + (((long long)n * F.S + s) * F.C + c0) * F.K;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    dst[e * F.K] = a0[e];
    if (F.K > 1) dst[e * F.K + 1] = a1[e];
  }
}

template <int FN>
__global__ void __launch_bounds__(NORM_THREADS) norm_product_kernel(const NormBatch batch) {
  __shared__ float lds[NORM_WAVES][2];
  const NormItem& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)((long long)blockIdx.x - F.base);
  if (!F.cfast) norm_plane_body<FN>(F, local, lds);      // uniform over the workgroup: it belongs to one item
  else if (F.cvec) norm_chan_body<FN, 4>(F, local);
  else norm_chan_body<FN, 1>(F, local);
}

// ------------------------------------------------------------------------------------------------ 3: slices, samples
// p[n, c, k] = sum_s part[n, s, c, k]: one thread per value, the slices in order.
__global__ void __launch_bounds__(NORM_THREADS) norm_slices_kernel(const NormSumBatch batch) {
  const long long t = (long long)blockIdx.x * NORM_THREADS + threadIdx.x;
  const NormSum& F = batch.e[owner_of(batch, t)];
  const long long at = t - F.base, row = (long long)F.C * F.K;
  if (at >= (long long)F.N * row) return;
  const long long n = at / row, ck = at - n * row;
  const float* __restrict__ src = F.part + n * F.S * row + ck;
  float sum = 0.0f;
  for (int s = 0; s < F.S; ++s) sum += src[(long long)s * row];
  F.dst[at] = sum;
}

// dst[c] (+)= scale * [[sum xh^2, sum xh], [sum xh, count]] (A side; 1 x 1 without a bias) or scale * sum g^2 (G side): a
// workgroup per NORM_SUM_CH channels; a thread sums the rows (sample, slice) r = its row group, + NORM_SUM_ROWS, ... of its
// channel in order, then the row groups in order.
constexpr int NORM_SUM_CH = 16, NORM_SUM_ROWS = NORM_THREADS / NORM_SUM_CH;
__global__ void __launch_bounds__(NORM_THREADS) norm_factor_kernel(const NormSumBatch batch) {
  __shared__ float lds[NORM_SUM_ROWS][NORM_SUM_CH][2];
  const NormSum& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)((long long)blockIdx.x - F.base);
  const int cl = threadIdx.x % NORM_SUM_CH, rg = threadIdx.x / NORM_SUM_CH;
  const long long c = (long long)local * NORM_SUM_CH + cl;
  const long long row = (long long)F.C * F.K;
  float s0 = 0.0f, s1 = 0.0f;
  if (c < F.C) {
    const float* __restrict__ src = F.part + c * F.K;
    const int rows = F.N * F.S;
    for (int r = rg; r < rows; r += NORM_SUM_ROWS) {
      s0 += src[(long long)r * row];
      if (F.K > 1) s1 += src[(long long)r * row + 1];
    }
  }
  lds[rg][cl][0] = s0;
  lds[rg][cl][1] = s1;
  __syncthreads();
  if (rg != 0 || c >= F.C) return;
  s0 = lds[0][cl][0]; s1 = lds[0][cl][1];
#pragma unroll
  for (int k = 1; k < NORM_SUM_ROWS; ++k) { s0 += lds[k][cl][0]; s1 += lds[k][cl][1]; }
  const int n_g = F.side == CURV_NORM_SIDE_A ? F.n_g : 1;
  float* out = F.dst + c * n_g * n_g;
  float v[4] = {F.scale * s0, F.scale * s1, F.scale * s1, F.scale * F.count};
  for (int k = 0; k < n_g * n_g; ++k) out[k] = F.first ? v[k] : out[k] + v[k];
}

// ------------------------------------------------------------------------------------------------ host
enum NormUse { USE_A = 1, USE_G = 2, USE_PS = 3 };       // which records an entry point reads: x, g, both

// The largest offset (in elements) a sample of an (N, C, H, W) view addresses, or -1 if it does not fit 31 bits.
long long norm_span(const long long dims[4], const long long strides[4]) {
  const long long cap = 1LL << 31;
  long long span = 0;
  for (int k = 1; k < 4; ++k) {
    if (dims[k] > 1 && strides[k] >= cap) return -1;
    span += (dims[k] - 1) * strides[k];
    if (span >= cap) return -1;
  }
  return span;
}

bool norm_record_of(const curv_norm_desc& d, bool is_x, int index, const char* who, bool pointers, NormRecord* out) {
  const char* tag = is_x ? "x" : "g";
  const float* at = is_x ? d.x : d.g;
  const long long st[4] = {is_x ? d.x_sn : d.g_sn, is_x ? d.x_sc : d.g_sc, is_x ? d.x_sh : d.g_sh, is_x ? d.x_sw : d.g_sw};
  const long long elems = is_x ? d.x_elems : d.g_elems;
  const long long dims[4] = {d.N, d.C, d.H, d.W};
  for (int k = 0; k < 4; ++k)
    if (st[k] < 0) {
      set_error("%s: item %d: negative stride of %s", who, index, tag);
      return false;
    }
  const long long inside = norm_span(dims, st);
  if (inside < 0) {
    set_error("%s: item %d: a sample of %s spans 2^31 elements or more", who, index, tag);
    return false;
  }
  // the largest addressed offset lies inside the stated extent (by a division: the product may not fit)
  if (elems < 1 || inside >= elems || (d.N > 1 && st[0] > (elems - 1 - inside) / (d.N - 1))) {
    set_error("%s: item %d: the extent of %s (%lld elements) is smaller than the largest offset its sizes and strides "
              "address", who, index, tag, elems);
    return false;
  }
  if (pointers) {
    if (!at) {
      set_error("%s: item %d: null record %s", who, index, tag);
      return false;
    }
    if (reinterpret_cast<uintptr_t>(at) & 3) {
      set_error("%s: item %d: record %s is not aligned to its 4-byte elements", who, index, tag);
      return false;
    }
  }
  NormRecord r;
  r.at = at;
  r.sn = d.N > 1 ? st[0] : 0;
  r.sc = (unsigned)(d.C > 1 ? st[1] : 0); r.sh = (unsigned)(d.H > 1 ? st[2] : 0); r.sw = (unsigned)(d.W > 1 ? st[3] : 0);
  // position l = h W + w lies at l * sl where the rows follow one another at the column stride
  r.flat = d.H == 1 || d.W == 1 || st[2] == d.W * st[3];
  r.sl = d.W > 1 ? r.sw : r.sh;
  const bool at16 = (reinterpret_cast<uintptr_t>(at) & 15) == 0 && (d.N == 1 || st[0] % 4 == 0);
  r.al_l = at16 && (d.C == 1 || st[1] % 4 == 0);
  r.al_c = at16 && (d.H == 1 || st[2] % 4 == 0) && (d.W == 1 || st[3] % 4 == 0);
  *out = r;
  return true;
}

// Item `index` as the kernels read it (without its scratch and `base`), or false with the error text set.  `use`: the
// records the entry point reads; `pointers`: also their addresses (the host-only queries do not need them).
bool norm_item_of(const curv_norm_desc& d, int index, const char* who, int use, bool pointers, NormItem* out) {
  if (d.N < 1 || d.C < 1 || d.H < 1 || d.W < 1) {
    set_error("%s: item %d: invalid geometry (N %d C %d H %d W %d)", who, index, d.N, d.C, d.H, d.W);
    return false;
  }
  if (d.mode != CURV_NORM_GROUP && d.mode != CURV_NORM_POSITION && d.mode != CURV_NORM_GIVEN) {
    set_error("%s: item %d: unknown statistics mode %d", who, index, d.mode);
    return false;
  }
  if (d.mode == CURV_NORM_GROUP && (d.groups < 1 || d.C % d.groups)) {
    set_error("%s: item %d: groups %d does not divide C = %d", who, index, d.groups, d.C);
    return false;
  }
  if (!(d.eps > 0.0f) || !std::isfinite(d.eps)) {
    set_error("%s: item %d: eps %g must be finite and > 0", who, index, (double)d.eps);
    return false;
  }
  if (d.reserved != 0 || d.reserved2 != 0) {
    set_error("%s: item %d: reserved fields must be 0", who, index);
    return false;
  }
  const long long planes = (long long)d.N * d.C, L = (long long)d.H * d.W;
  if (planes >= (1LL << 29) || L >= (1LL << 29) || (long long)d.N * L >= (1LL << 29)) {
    set_error("%s: item %d: too large (%lld planes of %lld positions)", who, index, planes, L);
    return false;
  }
  NormItem F;
  memset(&F, 0, sizeof(F));
  const bool use_x = (use & USE_A) != 0, use_g = (use & USE_G) != 0;
  if (use_x && !norm_record_of(d, true, index, who, pointers, &F.x)) return false;
  if (use_g && !norm_record_of(d, false, index, who, pointers, &F.g)) return false;
  if (use_x && d.mode == CURV_NORM_GIVEN && pointers && (!d.mean || !d.var)) {
    set_error("%s: item %d: given statistics need mean and var (null %s)", who, index, !d.mean ? "mean" : "var");
    return false;
  }
  F.mean = d.mean; F.var = d.var;
  F.N = d.N; F.C = d.C; F.W = d.W; F.L = (int)L;
  F.mode = d.mode;
  F.G = d.mode == CURV_NORM_GROUP ? d.groups : 1;
  F.cg = d.C / F.G;
  F.eps = d.eps;
  const int n_g = 1 + (d.has_bias ? 1 : 0);
  F.K = use == USE_G ? 1 : n_g;
  // lanes run along c where every record the pass reads has unit channel stride
  F.cfast = d.C > 1 && (!use_x || F.x.sc == 1) && (!use_g || F.g.sc == 1);
  F.S = F.cfast ? (int)cdivll(L, NORM_SLICE) : 1;
  const bool x_unit_l = !use_x || (F.x.flat && (L == 1 || F.x.sl == 1));
  const bool g_unit_l = !use_g || (F.g.flat && (L == 1 || F.g.sl == 1));
  F.split_p = L >= NORM_SPLIT_L;
  F.quads_p = !F.cfast && L % 4 == 0 && x_unit_l && g_unit_l && !(use_x && d.mode == CURV_NORM_POSITION);
  // four channels per thread: groups of four channels lie in aligned 16-byte groups at every position
  // (a thread's sums do not depend on how many channels it takes, so this may follow the addresses)
  F.cvec = F.cfast && d.C % 4 == 0 && (!use_x || F.x.al_c) && (!use_g || F.g.al_c);
  if (use_x && d.mode != CURV_NORM_GIVEN) {
    const bool group = d.mode == CURV_NORM_GROUP;
    F.sets = group ? F.G : (int)L;
    F.set_cnt = group ? (int)(F.cg * L) : d.C;
    if ((long long)F.cg * L >= (1LL << 29)) {
      set_error("%s: item %d: too large (%lld elements per group)", who, index, (long long)F.cg * L);
      return false;
    }
    F.split_s = F.set_cnt >= NORM_SPLIT_L;
    if (group) {
      const bool planes_run = F.x.flat && (L == 1 || F.x.sl == 1) && (F.cg == 1 || F.x.sc == L);     // (c, l), l fastest
      const bool chans_run = F.x.flat && (F.cg == 1 || F.x.sc == 1) && (L == 1 || F.x.sl == F.cg);    // (l, c), c fastest
      F.run_s = planes_run || chans_run;
      F.outer_l = !planes_run && F.x.sc == 1 && F.cg > 1;
      F.inner = F.outer_l ? F.cg : (int)L;
      F.al_s = planes_run ? F.x.al_l : F.x.al_c && (F.G == 1 || F.cg % 4 == 0);
    } else {
      F.run_s = d.C == 1 || F.x.sc == 1;
      F.outer_l = 1;
      F.inner = d.C;
      F.al_s = F.x.al_c;
    }
    F.quads_s = F.run_s && F.set_cnt % 4 == 0;
  }
  *out = F;
  return true;
}

size_t norm_floats(long long count) { return align_up((size_t)count * sizeof(float), 256); }
size_t norm_stats_bytes(const NormItem& F) { return F.sets ? norm_floats(2LL * F.N * F.sets) : 0; }
size_t norm_part_bytes(const NormItem& F) { return norm_floats((long long)F.N * F.S * F.C * F.K); }
size_t norm_p_bytes(const NormItem& F, int use) { return use == USE_PS && F.S > 1 ? norm_floats((long long)F.N * F.C * F.K) : 0; }
size_t norm_item_bytes(const NormItem& F, int use) { return norm_stats_bytes(F) + norm_part_bytes(F) + norm_p_bytes(F, use); }

int norm_use_of(const curv_norm_desc& d, bool factor) { return !factor ? USE_PS : d.side == CURV_NORM_SIDE_G ? USE_G : USE_A; }

bool norm_side_ok(const curv_norm_desc& d, int index, const char* who) {
  if (d.side == CURV_NORM_SIDE_A || d.side == CURV_NORM_SIDE_G) return true;
  set_error("%s: item %d: unknown side %d", who, index, d.side);
  return false;
}

size_t norm_workspace_bytes_of(const char* name, const curv_norm_desc* descs, int n, bool factor) {
  if (n <= 0) return 0;
  if (!descs) {
    set_error("%s: null descriptors", name);
    return 0;
  }
  size_t need = 0;
  for (int i = 0; i < n; ++i) {
    NormItem F;
    if (factor && !norm_side_ok(descs[i], i, name)) return 0;
    const int use = norm_use_of(descs[i], factor);
    if (!norm_item_of(descs[i], i, name, use, false, &F)) return 0;
    need += norm_item_bytes(F, use);
  }
  return need;
}

long long norm_flops_of(const NormItem& F, int use) {
  const long long elems = (long long)F.N * F.C * F.L;
  const int n_g = use == USE_G ? 0 : F.K;
  return elems * ((F.sets ? 6 : 0) + 2 + 2 * n_g);
}

// Every item planned (nothing is launched before all are), its scratch carved out of the workspace in call order.
int norm_plan(const char* name, const curv_norm_desc* descs, int n, bool factor, void* workspace, size_t workspace_bytes,
              std::vector<NormItem>* items) {
  CURV_REQUIRE(descs, "%s: null descriptors", name);
  items->resize(n);
  size_t need = 0;
  for (int i = 0; i < n; ++i) {
    if (factor && !norm_side_ok(descs[i], i, name)) return CURV_ERR_INVALID;
    const int use = norm_use_of(descs[i], factor);
    if (!norm_item_of(descs[i], i, name, use, true, &(*items)[i])) return CURV_ERR_INVALID;
    need += norm_item_bytes((*items)[i], use);
  }
  const int rc = side::require_workspace(name, workspace, workspace_bytes, need, 256);
  if (rc != CURV_OK) return rc;
  char* at = (char*)workspace;
  for (int i = 0; i < n; ++i) {
    NormItem& F = (*items)[i];
    const int use = norm_use_of(descs[i], factor);
    F.stats = F.sets ? (float*)at : nullptr;
    at += norm_stats_bytes(F);
    F.part = (float*)at;
    at += norm_part_bytes(F);
    F.p = norm_p_bytes(F, use) ? (float*)at : F.part;
    at += norm_p_bytes(F, use);
  }
  return CURV_OK;
}

typedef void (*NormKernel)(NormBatch);

// One pass over the items `which` selects, in call order: blocks_of(F) workgroups each.
template <typename Which, typename BlocksOf>
int norm_pass(const char* name, hipStream_t stream, const std::vector<NormItem>& items, NormKernel kernel, Which which,
              BlocksOf blocks_of) {
  std::vector<int> take;
  for (size_t i = 0; i < items.size(); ++i)
    if (which((int)i)) take.push_back((int)i);
  return for_arg_batches<NormItem, NORM_BATCH, 1>(
      (int)take.size(), name,
      [&](int k, NormItem* F, long long* blocks) {
        *F = items[take[k]];
        blocks[0] = blocks_of(*F);
      },
      [](int, long long blocks) { return blocks; },
      [&](const NormBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(kernel, dim3(grid[0]), dim3(NORM_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

long long norm_stats_blocks(const NormItem& F) {
  const long long sets = (long long)F.N * F.sets;
  return F.split_s ? sets : cdivll(sets, NORM_WAVES);
}

long long norm_product_blocks(const NormItem& F) {
  if (!F.cfast) {
    const long long planes = (long long)F.N * F.C;
    return F.split_p ? planes : cdivll(planes, NORM_WAVES);
  }
  const long long cblocks = cdivll(F.C / (F.cvec ? 4 : 1), NORM_THREADS);
  return (long long)F.N * F.S * cblocks;
}

// Passes 1 and 2 of all items; `use_of(i)`: the records item i reads.
template <typename UseOf>
int norm_products(const char* name, hipStream_t stream, const std::vector<NormItem>& items, UseOf use_of) {
  int rc = norm_pass(name, stream, items, norm_stats_kernel, [&](int i) { return items[i].sets != 0; }, norm_stats_blocks);
  if (rc != CURV_OK) return rc;
  const NormKernel kernels[3] = {norm_product_kernel<0>, norm_product_kernel<1>, norm_product_kernel<2>};
  const int uses[3] = {USE_PS, USE_A, USE_G};
  for (int fn = 0; fn < 3; ++fn) {
    rc = norm_pass(name, stream, items, kernels[fn], [&](int i) { return use_of(i) == uses[fn]; }, norm_product_blocks);
    if (rc != CURV_OK) return rc;
  }
  return CURV_OK;
}

// What the per-sample entry points run in front of phase 2: passes 1 and 2, then the slices summed into p.
int norm_per_sample_run(const char* name, hipStream_t stream, const std::vector<NormItem>& items) {
  int rc = norm_products(name, stream, items, [](int) { return (int)USE_PS; });
  if (rc != CURV_OK) return rc;
  std::vector<int> sliced;
  for (size_t i = 0; i < items.size(); ++i)
    if (items[i].S > 1) sliced.push_back((int)i);
  return for_arg_batches<NormSum, NORM_BATCH, 1>(
      (int)sliced.size(), name,
      [&](int k, NormSum* R, long long* threads) {
        const NormItem& F = items[sliced[k]];
        memset(R, 0, sizeof(*R));
        R->part = F.part; R->dst = F.p;
        R->N = F.N; R->S = F.S; R->C = F.C; R->K = F.K;
        threads[0] = (long long)align_up((size_t)F.N * F.C * F.K, NORM_THREADS);   // an item's threads fill whole workgroups
      },
      [](int, long long threads) { return threads / NORM_THREADS; },
      [&](const NormSumBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(norm_slices_kernel, dim3(grid[0]), dim3(NORM_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac_norm_workspace_bytes(const curv_norm_desc* descs, int n) {
  return norm_workspace_bytes_of("curv_kfac_norm_workspace_bytes", descs, n, true);
}

extern "C" size_t curv_persample_norm_workspace_bytes(const curv_norm_desc* descs, int n) {
  return norm_workspace_bytes_of("curv_persample_norm_workspace_bytes", descs, n, false);
}

extern "C" int curv_kfac_norm_plan_flops(const curv_norm_desc* descs, int n, long long* out) {
  const char* const name = "curv_kfac_norm_plan_flops";
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs && out, "%s: null argument", name);
  for (int i = 0; i < n; ++i) {
    NormItem F;
    if (!norm_side_ok(descs[i], i, name)) return CURV_ERR_INVALID;
    const int use = norm_use_of(descs[i], true);
    if (!norm_item_of(descs[i], i, name, use, false, &F)) return CURV_ERR_INVALID;
    out[i] = norm_flops_of(F, use);
  }
  return CURV_OK;
}

extern "C" int curv_persample_norm_plan_info(const curv_norm_desc* descs, int n, long long* flops, long long* bytes) {
  const char* const name = "curv_persample_norm_plan_info";
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs && (flops || bytes), "%s: null argument", name);
  for (int i = 0; i < n; ++i) {
    NormItem F;
    if (!norm_item_of(descs[i], i, name, USE_PS, false, &F)) return CURV_ERR_INVALID;
    if (flops) flops[i] = norm_flops_of(F, USE_PS);
    if (bytes) bytes[i] = 4LL * F.N * F.C * F.L * (F.sets ? 3 : 2);
  }
  return CURV_OK;
}

extern "C" int curv_kfac_norm_accumulate(void* stream_, const curv_norm_desc* descs, int n, void* workspace,
                                         size_t workspace_bytes) {
  const char* const name = "curv_kfac_norm_accumulate";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<NormItem> items;
  int rc = norm_plan(name, descs, n, true, workspace, workspace_bytes, &items);
  if (rc != CURV_OK) return rc;
  for (int i = 0; i < n; ++i) {
    CURV_REQUIRE(descs[i].dst, "%s: item %d: null destination", name, i);
    CURV_REQUIRE((reinterpret_cast<uintptr_t>(descs[i].dst) & 3) == 0, "%s: item %d: destination not aligned to its 4-byte "
                 "elements", name, i);
    CURV_REQUIRE(std::isfinite(descs[i].scale), "%s: item %d: scale %g is not finite", name, i, (double)descs[i].scale);
  }
  rc = norm_products(name, stream, items, [&](int i) { return norm_use_of(descs[i], true); });
  if (rc != CURV_OK) return rc;
  return for_arg_batches<NormSum, NORM_BATCH, 1>(
      n, name,
      [&](int i, NormSum* R, long long* threads) {
        const NormItem& F = items[i];
        memset(R, 0, sizeof(*R));
        R->part = F.part; R->dst = descs[i].dst;
        R->N = F.N; R->S = F.S; R->C = F.C; R->K = F.K;
        R->n_g = 1 + (descs[i].has_bias ? 1 : 0); R->side = descs[i].side; R->first = descs[i].first ? 1 : 0;
        R->scale = descs[i].scale; R->count = (float)((long long)F.N * F.L);
        threads[0] = cdivll(F.C, NORM_SUM_CH);                                     // (workgroups)
      },
      [](int, long long blocks) { return blocks; },
      [&](const NormSumBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(norm_factor_kernel, dim3(grid[0]), dim3(NORM_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

extern "C" int curv_persample_norm_sq_accumulate(void* stream_, const curv_norm_desc* descs, int n, void* workspace,
                                                 size_t workspace_bytes) {
  const char* const name = "curv_persample_norm_sq_accumulate";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<NormItem> items;
  int rc = norm_plan(name, descs, n, false, workspace, workspace_bytes, &items);
  if (rc != CURV_OK) return rc;
  std::vector<DwSqArgs> args(n);
  for (int i = 0; i < n; ++i) {
    const NormItem& F = items[i];
    CURV_REQUIRE(descs[i].dst, "%s: item %d: null destination", name, i);
    CURV_REQUIRE(descs[i].c_rs >= F.K || descs[i].C == 1, "%s: item %d: c_rs %lld below n_g = %d", name, i, descs[i].c_rs, F.K);
    args[i] = DwSqArgs{F.p, descs[i].dst, descs[i].c_rs, F.N, F.C, F.K, descs[i].first ? 1 : 0, descs[i].alpha};
  }
  rc = norm_per_sample_run(name, stream, items);
  if (rc != CURV_OK) return rc;
  return dw_launch_sq(name, stream, args.data(), n);
}

extern "C" int curv_persample_norm_quad_reduce(void* stream_, const curv_norm_desc* descs, int n, void* workspace,
                                               size_t workspace_bytes) {
  const char* const name = "curv_persample_norm_quad_reduce";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<NormItem> items;
  int rc = norm_plan(name, descs, n, false, workspace, workspace_bytes, &items);
  if (rc != CURV_OK) return rc;
  std::vector<DwQuadArgs> args(n);
  for (int i = 0; i < n; ++i) {
    const NormItem& F = items[i];
    const curv_norm_desc& d = descs[i];
    CURV_REQUIRE(d.out, "%s: item %d: null destination", name, i);
    CURV_REQUIRE(d.o_stride >= 1 || d.N == 1, "%s: item %d: o_stride %lld below 1", name, i, d.o_stride);
    CURV_REQUIRE(!d.T || (d.t_rs >= 0 && d.t_cs >= 0), "%s: item %d: negative stride of T", name, i);
    CURV_REQUIRE(!d.Wt || d.w_rs >= 0, "%s: item %d: negative stride of W", name, i);
    args[i] = DwQuadArgs{F.p, d.T, d.Wt, d.s, d.out, d.t_cs, d.t_rs, d.w_rs, d.o_stride, F.N, F.C, F.K, d.first ? 1 : 0,
                         d.alpha};
  }
  rc = norm_per_sample_run(name, stream, items);
  if (rc != CURV_OK) return rc;
  return dw_launch_quad(name, stream, args.data(), n);
}
