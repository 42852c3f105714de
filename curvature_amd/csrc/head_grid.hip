// The d2 of the last-layer Laplace predictive over a grid of damping pairs (curv_head_grid, include/curv_hip.h):
//   out[h][r][j] = gain[h] r_h[j] sum_i Y[r][i]^2 / (T[j][i] + shift[h]),   h < H <= 16, r < N, j < K, i < n
// dense (T a K x n table, r_h = 1) or separable (T[j][i] = v[i], r_h[j] = 1 / (u[j] + shift[h])).
//
// One wave is one workgroup.
//
// Dense: a product on v_mfma_f32_32x32x2_f32 with a generated B operand.  A wave = (32 x 32 block of (r, j), chunk of the
// steps of 32 i, group of HGR_GROUP = 2 pairs) keeps one block of accumulators per pair of its group.  Per step lane
// (row = lane & 31, half = lane >> 5) takes the 16 consecutive i = 32 step + 16 half + e of Y row r and of T row j straight
// from global memory (no alignment beyond 4 bytes is assumed; the next step's loads are issued before this step's
// products), squares the Y values - the A operand, shared by the pairs - and for every T value forms the 2 reciprocals
// 1 / (t + shift[h]) in registers: the B operands of 2 MFMAs.  Rows r >= N and columns i >= n enter as Y^2 = 0 against a
// finite weight (t = 1), rows j >= K are computed and not stored; nothing outside the N x n and K x n entries is read.
// The groups of an item read the same Y and T (from L2) and share no arithmetic: T is read once per 2 pairs, no (H, K, n)
// weight tensor exists, and pair h has the same bits in any list.  A block of one chunk is finished there (gain,
// stored); otherwise the sums go to partial[chunk][h][r][j] in the caller's workspace (16 slices per chunk whatever H)
// and a second launch adds the chunks in chunk order and applies the gain.
//
// Separable: a wave = (pair h, input r).  Lane l adds Y[r][i]^2 / (v[i] + shift) over i = l, l + 64, ... in order, the wave
// sums by DPP (wave_sum.h) - the sum does not depend on j and is formed once - and the lanes write
// gain / (u[j] + shift) * sum for j = l, l + 64, ...
//
// Fixed order everywhere (lane, wave, chunk), no atomics; the chunk length follows from the item's own N, K and n
// (hgr_plan_of), so its bits are the same alone and in a batch.  All global stores are plain vector stores.
#include "side_build.h"
#include "wave_sum.h"

#include <cmath>

namespace curv {
namespace {

constexpr int HGR_THREADS = 64;
constexpr int HGR_RED_THREADS = 256;
constexpr int HGR_BATCH = 8;                   // items per launch (tables as kernel arguments)
constexpr int HGR_MAX = CURV_HEAD_GRID_MAX;
constexpr int HGR_GROUP = 2;                   // pairs per wave of the dense form (timed: 1, 2 and 4 - DESIGN.md K24)
constexpr int HGR_WGS_TARGET = 256;            // the steps of a block are cut into chunks until an item has about this many waves per group
constexpr int HGR_MIN_STEPS = 4;               // ... but a wave takes at least this many steps: a short sum is not worth a second pass
static_assert(HGR_MAX % HGR_GROUP == 0, "the groups tile the pairs");

struct HgrItem {
  const float* Y;
  const float* T;              // null: separable
  const float* u;
  const float* v;
  float* out;
  float* partial;              // [chunk][HGR_MAX][N][K], used when chunks > 1
  long long y_rs, t_rs;
  float shift[HGR_MAX], gain[HGR_MAX];
  int N, K, n, H;
  int jblocks;                 // ceil(K / 32)
  int chunk_steps, chunks;     // steps of 32 i per wave, waves per block and group
  long long base;              // first workgroup / reduce block of this item in the launch
};

typedef ArgBatch<HgrItem, HGR_BATCH> HgrBatch;
static_assert(sizeof(HgrBatch) <= 3840, "kernel argument block must stay below 4 KB");

struct HgrPlan {
  bool separable;
  int chunk_steps, chunks;
  long long blocks;
  size_t bytes;
  long long flops;
};

bool hgr_plan_of(const curv_head_grid_desc& d, int index, HgrPlan* p) {
  const char* const who = "curv_head_grid";
  if (d.N < 1 || d.K < 1 || d.n < 1) {
    set_error("%s: item %d: invalid sizes (N %d K %d n %d: all at least 1)", who, index, d.N, d.K, d.n);
    return false;
  }
  const long long cap = 1LL << 31;
  if ((long long)d.N * d.n >= cap || (long long)d.K * d.n >= cap || (long long)HGR_MAX * d.N * d.K >= cap) {
    set_error("%s: item %d: too large (N %d K %d n %d: N n, K n and %d N K must stay below 2^31 elements)", who, index, d.N,
              d.K, d.n, HGR_MAX);
    return false;
  }
  if (d.H < 1 || d.H > HGR_MAX) {
    set_error("%s: item %d: H %d outside 1 .. %d", who, index, d.H, HGR_MAX);
    return false;
  }
  if (!d.shift || !d.gain) {
    set_error("%s: item %d: null shift or gain", who, index);
    return false;
  }
  for (int h = 0; h < d.H; ++h) {
    if (!(d.shift[h] > 0.f) || !std::isfinite(d.shift[h]) || !std::isfinite(d.gain[h])) {
      set_error("%s: item %d: pair %d: shift %g must be finite and > 0, gain %g finite", who, index, h, (double)d.shift[h],
                (double)d.gain[h]);
      return false;
    }
  }
  const bool separable = d.u != nullptr && d.v != nullptr && d.T == nullptr;
  const bool dense = d.T != nullptr && d.u == nullptr && d.v == nullptr;
  if (!separable && !dense) {
    set_error("%s: item %d: give the spectrum as u and v (separable) or as T (dense), not both", who, index);
    return false;
  }
  if (d.y_rs < d.n || (dense && d.t_rs < d.n)) {
    set_error("%s: item %d: invalid strides (y_rs %lld or t_rs %lld below n %d)", who, index, d.y_rs, d.t_rs, d.n);
    return false;
  }
  p->separable = separable;
  p->chunk_steps = p->chunks = 1;
  p->blocks = 0;
  p->bytes = 0;
  p->flops = 0;
  if (separable) return true;
  const long long steps = cdiv(d.n, 32);
  p->blocks = (long long)cdiv(d.N, 32) * cdiv(d.K, 32);
  p->chunk_steps = (int)std::max<long long>(HGR_MIN_STEPS, cdivll(steps, cdivll(HGR_WGS_TARGET, p->blocks)));
  p->chunks = (int)cdivll(steps, p->chunk_steps);
  p->bytes = p->chunks > 1 ? align_up((size_t)p->chunks * HGR_MAX * d.N * d.K * sizeof(float), 256) : 0;
  p->flops = 2LL * 32 * 32 * 32 * steps * p->blocks;
  return true;
}

size_t hgr_bytes_of(const std::vector<HgrPlan>& plans) {
  size_t total = 0;
  for (const HgrPlan& p : plans) total += p.bytes;
  return total;
}

// row of accumulator register `reg` within a 32 x 32 block (column = lane & 31)
__device__ __forceinline__ int hgr_acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ void hgr_dense(const HgrItem& d, long long local) {
  const int lane = threadIdx.x, r = lane & 31, half = lane >> 5;
  const int N = d.N, K = d.K, n = d.n;
  // local = ((block * chunks) + chunk) * groups + group
  const int groups = (d.H + HGR_GROUP - 1) / HGR_GROUP;
  const int group = (int)(local % groups);
  const long long rest = local / groups;
  const int chunk = (int)(rest % d.chunks);
  const long long block = rest / d.chunks;
  const int jb = (int)(block % d.jblocks), nb = (int)(block / d.jblocks);
  const int steps = (n + 31) >> 5;
  const int s0 = chunk * d.chunk_steps, s1 = min(steps, s0 + d.chunk_steps);
  const int h0 = group * HGR_GROUP;

  float shift[HGR_GROUP];
#pragma unroll
  for (int g = 0; g < HGR_GROUP; ++g) shift[g] = h0 + g < d.H ? d.shift[h0 + g] : 1.0f;      // (a pair past H: computed, not stored)

  const int row_y = 32 * nb + r, row_t = 32 * jb + r;
  const float* yp = d.Y + (long long)row_y * d.y_rs;
  const float* tp = d.T + (long long)row_t * d.t_rs;
  // y[e] = Y[row_y][32 step + 16 half + e] (0 outside Y), t[e] = T[row_t][..] (1 outside T)
  auto load = [&](int step, float (&y)[16], float (&t)[16]) {
    const int k0 = 32 * step + 16 * half;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      y[e] = 0.f;
      t[e] = 1.f;
    }
    if (step >= s1) return;                                                         // uniform in the wave
    if (32 * step + 32 <= n) {
      if (row_y < N) {
#pragma unroll
        for (int e = 0; e < 16; ++e) y[e] = yp[k0 + e];
      }
      if (row_t < K) {
#pragma unroll
        for (int e = 0; e < 16; ++e) t[e] = tp[k0 + e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (row_y < N && k0 + e < n) y[e] = yp[k0 + e];
        if (row_t < K && k0 + e < n) t[e] = tp[k0 + e];
      }
    }
  };

  f32x16 acc[HGR_GROUP];
#pragma unroll
  for (int g = 0; g < HGR_GROUP; ++g)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[g][reg] = 0.f;

  float y0[16], t0[16], y1[16], t1[16];
  load(s0, y0, t0);
  for (int step = s0; step < s1; ++step) {
    load(step + 1, y1, t1);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float a = y0[e] * y0[e];
#pragma unroll
      for (int g = 0; g < HGR_GROUP; ++g)
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, 1.0f / (t0[e] + shift[g]), acc[g], 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      y0[e] = y1[e];
      t0[e] = t1[e];
    }
  }

  // block of pair h: rows = inputs 32 nb + hgr_acc_row(reg, half), column = class 32 jb + r
  const int col = 32 * jb + r;
  if (col >= K) return;
#pragma unroll
  for (int g = 0; g < HGR_GROUP; ++g) {
    const int h = h0 + g;
    if (h >= d.H) break;
    float* dst = d.chunks > 1 ? d.partial + ((long long)chunk * HGR_MAX + h) * N * K : d.out + (long long)h * N * K;
    const float scale = d.chunks > 1 ? 1.0f : d.gain[h];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = 32 * nb + hgr_acc_row(reg, half);
      if (row < N) dst[(long long)row * K + col] = scale * acc[g][reg];
    }
  }
}

__device__ __forceinline__ void hgr_separable(const HgrItem& d, long long local) {
  const int lane = threadIdx.x;
  const int h = (int)(local / d.N);
  const int r = (int)(local - (long long)h * d.N);
  const float shift = d.shift[h];
  const float* yp = d.Y + (long long)r * d.y_rs;
  float sum = 0.f;
  for (int i = lane; i < d.n; i += HGR_THREADS) {
    const float y = yp[i];
    sum += (y * y) * (1.0f / (d.v[i] + shift));
  }
  sum = wave_sum_dpp(sum);
  sum = __shfl(sum, 63);
  const float scale = d.gain[h];
  float* dst = d.out + ((long long)h * d.N + r) * d.K;
  for (int j = lane; j < d.K; j += HGR_THREADS) dst[j] = (scale * (1.0f / (d.u[j] + shift))) * sum;
}

__global__ void __launch_bounds__(HGR_THREADS) hgr_kernel(const HgrBatch batch) {
  const HgrItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long local = (long long)blockIdx.x - d.base;
  if (d.T != nullptr) hgr_dense(d, local);
  else hgr_separable(d, local);
}

// The chunks of a dense item in chunk order, then the gain: one thread per (h, r, j).  Blocks of an item:
// ceil(H N K / 256), none where it has one chunk.
__global__ void __launch_bounds__(HGR_RED_THREADS) hgr_reduce_kernel(const HgrBatch batch) {
  const HgrItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long slice = (long long)d.N * d.K;
  const long long idx = ((long long)blockIdx.x - d.base) * HGR_RED_THREADS + threadIdx.x;
  if (idx >= d.H * slice) return;
  const int h = (int)(idx / slice);
  const float* p = d.partial + idx;                // [chunk][HGR_MAX][N][K]: slice h of chunk 0, entry idx - h slice
  float v = 0.f;
  for (int c = 0; c < d.chunks; ++c) v += p[(long long)c * HGR_MAX * slice];
  d.out[idx] = d.gain[h] * v;
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_head_grid_workspace_bytes(const curv_head_grid_desc* descs, int n) {
  return side::workspace_bytes("curv_head_grid_workspace_bytes", descs, n, hgr_plan_of, hgr_bytes_of);
}

extern "C" int curv_head_grid_plan_flops(const curv_head_grid_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_head_grid_plan_flops", descs, n, out, hgr_plan_of);
}

extern "C" int curv_head_grid(void* stream_, const curv_head_grid_desc* descs, int n, void* workspace,
                              size_t workspace_bytes) {
  const char* const name = "curv_head_grid";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<HgrPlan> plans;
  if (!side::plans_of(name, descs, n, hgr_plan_of, &plans)) return CURV_ERR_INVALID;
  for (int i = 0; i < n; ++i) CURV_REQUIRE(descs[i].Y && descs[i].out, "%s: item %d: null Y or out", name, i);
  const size_t need = hgr_bytes_of(plans);
  if (need > 0) {
    const int rc = side::require_workspace(name, workspace, workspace_bytes, need, 256);
    if (rc != CURV_OK) return rc;
  }
  size_t at = 0;
  return for_arg_batches<HgrItem, HGR_BATCH, 2>(
      n, name,
      [&](int i, HgrItem* P, long long* units) {
        const curv_head_grid_desc& d = descs[i];
        const HgrPlan& p = plans[i];
        P->Y = d.Y; P->T = d.T; P->u = d.u; P->v = d.v; P->out = d.out;
        P->partial = p.bytes ? (float*)((char*)workspace + at) : nullptr;
        at += p.bytes;
        P->y_rs = d.y_rs; P->t_rs = d.t_rs;
        for (int h = 0; h < HGR_MAX; ++h) {
          P->shift[h] = h < d.H ? d.shift[h] : 1.0f;
          P->gain[h] = h < d.H ? d.gain[h] : 0.0f;
        }
        P->N = d.N; P->K = d.K; P->n = d.n; P->H = d.H;
        P->jblocks = cdiv(d.K, 32);
        P->chunk_steps = p.chunk_steps; P->chunks = p.chunks;
        P->base = 0;
        units[0] = p.separable ? (long long)d.H * d.N : p.blocks * p.chunks * cdiv(d.H, HGR_GROUP);
        units[1] = p.chunks > 1 ? cdivll((long long)d.H * d.N * d.K, HGR_RED_THREADS) : 0;
      },
      [](int, long long units) { return units; },
      [&](const HgrBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(hgr_kernel, dim3(grid[0]), dim3(HGR_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        if (grid[1] > 0) {
          hipLaunchKernelGGL(hgr_reduce_kernel, dim3(grid[1]), dim3(HGR_RED_THREADS), 0, stream, b[1]);
          CURV_LAUNCH_CHECK();
        }
        return CURV_OK;
      });
}
