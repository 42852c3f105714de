// Monte-Carlo softmax of the last-layer Laplace predictive over ALL classes (curv_head_mc, include/curv_hip.h):
//   f_s = mu_n + M (sqrt(max(d2_n, 0)) o z_{n,s}),   probs[n][c] = (1/S) sum_s softmax(f_s)[c],   K <= 1024
// with one K x K matrix M for the whole batch (KFAC: L_G, lower triangular; EFB: U_G; Diagonal: none) and a per-input
// vector (or scalar) d2_n.  The (N, S, K) draws exist only in MFMA accumulators (unless the caller asks for them).
//
// Workgroup (256 threads, four waves) = (item, input n, chunk of draw tiles); a tile is 32 draws.  Rows of M are cut into
// blocks of 32; wave w owns the blocks g = 4 b + w, b < NB = ceil(ceil(K / 32) / 4) <= 8 (interleaved, so that the waves of
// a triangular M carry the same work), and keeps its NB (32 rows x 32 draws) blocks of F in accumulators of
// v_mfma_f32_32x32x2_f32: at most 8 x 16 registers.  Per tile:
//   1. Products.  k runs in steps of 32.  The B operand of a step, sqrt(d2) o z for (k, draw), is made ONCE per workgroup:
//      thread (draw = tid & 31, quad = tid >> 5) takes one Philox counter (philox.h; or four floats of the caller's Z),
//      scales and writes four values to LDS (two buffers, one barrier per step).  A lane (row r = lane & 31, half
//      h = lane >> 5) takes the 16 consecutive k = 32 step + 16 h + i of its row straight from global memory - M is read
//      from L2 by every workgroup; no alignment beyond 4 bytes is assumed - one block ahead of the MFMAs that use them,
//      and multiplies them with LDS rows 16 h + i (pitch 34: the two halves of a wave read disjoint banks).  A block
//      whose k-range is over (m_lower: k >= 32 g + 32) is skipped; entries with column > row, rows and columns >= K are
//      never read (they count as 0).  Without M the block of F is sqrt(d2) o z itself, made in the accumulator layout.
//   2. Softmax.  + mu (-inf at rows >= K), the maximum and the sum of exponentials per draw: over a lane's 16 NB values,
//      the two halves of the wave, then the four waves through LDS in wave order; one reciprocal per draw, 0 for draws
//      >= S.
//   3. Sum over the 32 draws of the tile: each block goes through a (32 x 33) LDS tile per wave, lane (r, h) adds draws
//      16 h .. 16 h + 15 of row r in order, the halves are added, and the running sums over the tiles of the workgroup
//      stay in NB registers.
// An input with one chunk is finished there (/ S, written); otherwise the K sums go to partial[n][chunk][k] in the
// caller's workspace and a second launch adds the chunks in chunk order.  Fixed order everywhere (lane, wave, workgroup,
// chunk), no atomics; the chunk length follows from the item's own N and S (hmc_plan_of), so its bits are the same alone
// and in a batch.  All global stores are plain vector stores.
//
// curv_head_mc_moments is the same kernel with two more moments of the draws (hmc_block with an HmmItem; the instantiations
// behind curv_head_mc contain none of it): entropy[n] = (1/S) sum_s H(softmax f_s) and probs_sq[n][c] = (1/S) sum_s
// softmax(f_s)[c]^2.  With t_c = f_s[c] - max and e_c = exp(t_c), H_s = ln(sum e) - (sum e t) / (sum e): sum e t is one more
// running sum of pass 2 and goes the way of sum e (lane, halves, waves in wave order; a term with e = 0 - rows >= K, or an
// exponential that underflowed - counts as 0, never as 0 * -inf).  The H_s of the 32 draws of a tile (0 for draws >= S) are
// added by a butterfly over the lanes of a half wave, partners 16, 8, 4, 2, 1 apart in this order: every lane ends with the
// same bits; then tiles in tile order.  The squares take the transposition tile of pass 3 beside the values.  With chunks
// an (input, chunk) leaves 2 K + 1 partial sums - probs, squares, entropy - and the reduce launch finishes all three.
#include "philox.h"
#include "side_build.h"

#include <cmath>

namespace curv {
namespace {

constexpr int HMC_THREADS = 256;
constexpr int HMC_BATCH = 16;                  // items per launch (tables as kernel arguments)
constexpr int HMC_TILE = 32;                   // draws per tile: the N of one MFMA block
constexpr int HMC_WGS_TARGET = 256;            // the tiles of an input are cut into chunks until an item has about this many workgroups
constexpr int HMC_K_MAX = CURV_HEAD_MC_MAX_CLASSES;
constexpr int HMC_S_MAX = 1 << 30;
constexpr int HMC_BP = 34;                     // LDS pitch of the B rows: 16 * 34 = 32 (mod 64), the halves of a wave miss each other
constexpr int HMC_TP = 33;                     // LDS pitch of the transposition tile
static_assert(HMC_K_MAX == 1024, "hmc_kernel instantiates 1, 2, 4 and 8 row blocks per wave: 4 * 8 * 32 rows");

struct HmcItem {
  static constexpr bool moments = false;
  const float* M;              // may be null: identity
  const float* d2;
  const float* mu;
  const float* Z;              // may be null: Philox
  float* probs;
  float* draws;
  float* partial;              // [n][chunk][K], used when chunks > 1
  long long m_rs, d_ns, d_cs, mu_ns, z_ns, z_ss;
  unsigned long long seed, offset;
  int N, K, S, lower;
  int chunk_tiles, chunks;     // draw tiles per workgroup, workgroups per input
  long long base;              // first workgroup / reduce block of this item in the launch
};

typedef ArgBatch<HmcItem, HMC_BATCH> HmcBatch;
static_assert(sizeof(HmcBatch) <= 3840, "kernel argument block must stay below 4 KB");

// curv_head_mc_moments: `partial` is [n][chunk][2 K + 1] - probs, squares, entropy
struct HmmItem : HmcItem {
  static constexpr bool moments = true;
  float* entropy;
  float* probs_sq;
};

typedef ArgBatch<HmmItem, HMC_BATCH> HmmBatch;
static_assert(sizeof(HmmBatch) <= 3840, "kernel argument block must stay below 4 KB");

struct HmcPlan {
  int chunk_tiles, chunks;
  size_t bytes;
  long long flops;
};

// The checks and the plan of both entries: `outputs` says which outputs the entry has (all of them null is refused),
// `per_chunk` how many partial sums an (input, chunk) leaves.
template <typename Desc>
bool hmc_plan_common(const char* who, const Desc& d, int index, bool any_output, const char* outputs, int per_chunk,
                     HmcPlan* p) {
  if (d.K < 1 || d.K > HMC_K_MAX) {
    set_error("%s: item %d: K %d outside 1 .. %d", who, index, d.K, HMC_K_MAX);
    return false;
  }
  if (d.N < 1 || d.S < 1 || d.S > HMC_S_MAX || (long long)d.N * d.S > (1LL << 40)) {
    set_error("%s: item %d: invalid sizes (N %d S %d: both at least 1, S at most 2^30, N S at most 2^40)", who, index, d.N,
              d.S);
    return false;
  }
  if (d.M != nullptr && d.m_rs < d.K) {
    set_error("%s: item %d: invalid strides (m_rs %lld below K %d)", who, index, d.m_rs, d.K);
    return false;
  }
  if ((d.d_cs != 0 && d.d_cs != 1) || d.d_ns < (d.d_cs ? d.K : 1)) {
    set_error("%s: item %d: invalid strides (d_cs %lld neither 0 nor 1, or d_ns %lld below the %s of an input)", who, index,
              d.d_cs, d.d_ns, d.d_cs == 1 ? "K values" : "one value");
    return false;
  }
  if (d.mu_ns < d.K) {
    set_error("%s: item %d: invalid strides (mu_ns %lld below K %d)", who, index, d.mu_ns, d.K);
    return false;
  }
  if (d.Z != nullptr && (d.z_ss < d.K || d.z_ns < (long long)(d.S - 1) * d.z_ss + d.K)) {
    set_error("%s: item %d: invalid strides (z_ss %lld below K %d, or z_ns %lld below (S - 1) z_ss + K)", who, index,
              d.z_ss, d.K, d.z_ns);
    return false;
  }
  if (!any_output) {
    set_error("%s: item %d: no output (%s null)", who, index, outputs);
    return false;
  }
  if (d.reserved != 0) {
    set_error("%s: item %d: reserved must be 0", who, index);
    return false;
  }
  const long long tiles = cdivll(d.S, HMC_TILE);
  p->chunk_tiles = (int)cdivll(tiles, cdivll(HMC_WGS_TARGET, d.N));
  p->chunks = (int)cdivll(tiles, p->chunk_tiles);
  p->bytes = p->chunks > 1 ? align_up((size_t)d.N * p->chunks * per_chunk * sizeof(float), 256) : 0;
  long long steps = 0;                                       // k steps of 32 over the row blocks
  const int blocks = cdiv(d.K, 32);
  for (int g = 0; d.M != nullptr && g < blocks; ++g) steps += d.m_lower ? std::min(blocks, g + 1) : blocks;
  p->flops = 2LL * 32 * 32 * 32 * steps * tiles * d.N;
  return true;
}

bool hmc_plan_of(const curv_head_mc_desc& d, int index, HmcPlan* p) {
  return hmc_plan_common("curv_head_mc", d, index, d.probs || d.draws, "probs and draws are both", d.K, p);
}

bool hmm_plan_of(const curv_head_moments_desc& d, int index, HmcPlan* p) {
  return hmc_plan_common("curv_head_mc_moments", d, index, d.probs || d.draws || d.entropy || d.probs_sq,
                         "probs, draws, entropy and probs_sq are all", 2 * d.K + 1, p);
}

size_t hmc_bytes_of(const std::vector<HmcPlan>& plans) {
  size_t total = 0;
  for (const HmcPlan& p : plans) total += p.bytes;
  return total;
}

// v[e] = sqrt(max(d2[n][4 q + e], 0)) z[n][s][4 q + e]; 0 at classes >= K and draws >= S
__device__ __forceinline__ void hmc_quad(const HmcItem& d, long long n, int s, int q, float (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = 0.f;
  if (s >= d.S || 4 * q >= d.K) return;
  float z[4];
  if (d.Z != nullptr) {
    const float* zp = d.Z + n * d.z_ns + (long long)s * d.z_ss + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = 4 * q + e < d.K ? zp[e] : 0.f;
  } else {
    philox_normal4(d.seed, d.offset + ((unsigned long long)n * d.S + s) * ((d.K + 3) >> 2) + q, z);
  }
  const float* dp = d.d2 + n * d.d_ns;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (4 * q + e < d.K) v[e] = sqrtf(fmaxf(dp[(4 * q + e) * d.d_cs], 0.f)) * z[e];
}

// row of accumulator register `reg` within a 32 x 32 block (column = lane & 31)
__device__ __forceinline__ int hmc_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <int NB, typename Item>
__device__ __forceinline__ void hmc_block(const Item& d, long long local, float (*Bs)[32 * HMC_BP],
                                          float (*Ts)[32 * HMC_TP], float (*red)[4][HMC_TILE], float* mu_s,
                                          float* sq_s = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int K = d.K, S = d.S;
  const long long n = local / d.chunks;
  const int chunk = (int)(local - n * d.chunks);
  const int tiles = (S + HMC_TILE - 1) / HMC_TILE;
  const int t0 = chunk * d.chunk_tiles, t1 = min(tiles, t0 + d.chunk_tiles);
  const int steps = (K + 31) >> 5;
  const bool lower = d.lower != 0;
  constexpr bool MOM = Item::moments;
  auto want = [&]() {                                          // a softmax at all
    if constexpr (MOM) return d.probs != nullptr || d.entropy != nullptr || d.probs_sq != nullptr;
    else return d.probs != nullptr;
  };

  // a[i] = M[32 g + r][32 step + 16 h + i] of block b (g = 4 b + wave), 0 where the entry is outside M or above the diagonal
  auto load_a = [&](int b, int step, float (&a)[16]) {
    const int g = 4 * b + wave, row = 32 * g + r, k0 = 32 * step + 16 * h;
    const int kend = lower ? min(K, 32 * g + 32) : K;
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
    if (step >= steps || 32 * g >= K || 32 * step >= kend) return;                  // uniform in the wave
    const float* mp = d.M + (long long)row * d.m_rs + k0;
    if (32 * g + 32 <= K && 32 * step + 32 <= K && (!lower || step < g)) {
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = mp[i];
    } else if (row < K) {
      const int last = lower ? row : K - 1;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (k0 + i <= last) a[i] = mp[i];
    }
  };
  auto active = [&](int b, int step) {
    const int g = 4 * b + wave;
    return 32 * g < K && 32 * step < (lower ? min(K, 32 * g + 32) : K);
  };

  // the logits of the input, -inf at rows >= K (read after the first barrier of a tile)
  for (int c = tid; c < 128 * NB; c += HMC_THREADS) mu_s[c] = c < K ? d.mu[n * d.mu_ns + c] : -INFINITY;
  if (d.M == nullptr) __syncthreads();

  float rsum[NB];
  float hsum = 0.f;                                            // (moments: the running sum of the entropies)
#pragma unroll
  for (int b = 0; b < NB; ++b) rsum[b] = 0.f;
  // (moments: the running sums of the squares stay in LDS, sq_s[row], written and read by lane (r, h = 0) of the row's
  // wave alone - with NB more registers the instantiation of NB = 8 would spill)
  if constexpr (MOM) {
    if (h == 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b) sq_s[32 * (4 * b + wave) + r] = 0.f;
    }
  }

  for (int tile = t0; tile < t1; ++tile) {
    const int s0 = tile * HMC_TILE;
    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) acc[b][reg] = 0.f;

    if (d.M != nullptr) {
      // ---- 1. F = M B
      auto fill_b = [&](int step, float* buf) {
        float v[4];
        const int q8 = tid >> 5;
        hmc_quad(d, n, s0 + (tid & 31), 8 * step + q8, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) buf[(4 * q8 + e) * HMC_BP + (tid & 31)] = v[e];
      };
      float a0[16], a1[16];
      load_a(0, 0, a0);
      fill_b(0, Bs[0]);
      __syncthreads();
      for (int step = 0; step < steps; ++step) {
        if (step + 1 < steps) fill_b(step + 1, Bs[(step + 1) & 1]);
        const float* bs = Bs[step & 1] + (16 * h) * HMC_BP + r;
        float bf[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) bf[i] = bs[i * HMC_BP];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (b + 1 < NB) load_a(b + 1, step, a1);
          else load_a(0, step + 1, a1);
          if (active(b, step)) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], bf[i], acc[b], 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) a0[i] = a1[i];
        }
        __syncthreads();
      }
    } else {
      // ---- 1'. F = sqrt(d2) o z in the accumulator layout: registers 4 j .. 4 j + 3 are one quad of classes
      // through the wave's LDS tile: the generator stays one rolled loop instead of 4 NB inlined copies
      float* ts = Ts[wave];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll 1
        for (int it = 0; it < 4; ++it) {
          const int ql = 2 * it + h;
          float v[4];
          hmc_quad(d, n, s0 + r, 8 * (4 * b + wave) + ql, v);
#pragma unroll
          for (int e = 0; e < 4; ++e) ts[(4 * ql + e) * HMC_TP + r] = v[e];
        }
        // (a lane reads back the 16 values it wrote itself: no barrier)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[b][reg] = ts[hmc_acc_row(reg, h) * HMC_TP + r];
      }
    }

    // ---- 2. + mu; the draws; softmax over the K rows of every draw
    const bool valid = s0 + r < S;
    float m = -INFINITY;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float f = acc[b][reg] + mu_s[32 * (4 * b + wave) + hmc_acc_row(reg, h)];
        acc[b][reg] = f;
        m = fmaxf(m, f);
      }
    }
    if (d.draws != nullptr && valid) {
      // (the row bound is hidden from the optimiser per tile: hoisted out of the tile loop, the 16 NB comparisons and
      // addresses would live in registers across the products)
      int Kt = K;
      asm volatile("" : "+s"(Kt));
      float* dp = d.draws + (n * S + s0 + r) * K;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = 32 * (4 * b + wave) + hmc_acc_row(reg, h);
          if (row < Kt) dp[row] = acc[b][reg];
        }
      }
    }
    if (!want()) continue;
    m = fmaxf(m, __shfl_xor(m, 32));
    if (h == 0) red[0][wave][r] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][0][r], red[0][1][r]), fmaxf(red[0][2][r], red[0][3][r]));
    float sum = 0.f, et = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float t = acc[b][reg] - m;
        const float e = expf(t);
        acc[b][reg] = e;
        sum += e;
        if constexpr (MOM) et += e > 0.f ? e * t : 0.f;       // (t = -inf at rows >= K)
      }
    }
    sum += __shfl_xor(sum, 32);
    if constexpr (MOM) et += __shfl_xor(et, 32);
    if (h == 0) {
      red[1][wave][r] = sum;
      if constexpr (MOM) red[2][wave][r] = et;
    }
    __syncthreads();
    sum = ((red[1][0][r] + red[1][1][r]) + red[1][2][r]) + red[1][3][r];
    const float inv = valid ? 1.0f / sum : 0.f;
    if constexpr (MOM) {
      // H_s of draw s0 + r, the same bits in all eight half waves; then the 32 draws of the tile
      et = ((red[2][0][r] + red[2][1][r]) + red[2][2][r]) + red[2][3][r];
      float hs = valid ? logf(sum) - et / sum : 0.f;
#pragma unroll
      for (int step = 16; step >= 1; step >>= 1) hs += __shfl_xor(hs, step);
      hsum += hs;
    }

    // ---- 3. sum over the draws of the tile, block by block through the wave's LDS tile
    float* ts = Ts[wave];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) ts[hmc_acc_row(reg, h) * HMC_TP + r] = acc[b][reg] * inv;
      __syncthreads();
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) v += ts[r * HMC_TP + 16 * h + j];
      v += __shfl_xor(v, 32);
      rsum[b] += v;
      if constexpr (MOM) {
        if (d.probs_sq != nullptr) {                           // the same order: draws 16 h .. 16 h + 15, then the halves
          float v2 = 0.f;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const float p = ts[r * HMC_TP + 16 * h + j];
            v2 += p * p;
          }
          v2 += __shfl_xor(v2, 32);
          if (h == 0) sq_s[32 * (4 * b + wave) + r] += v2;
        }
      }
      __syncthreads();
    }
  }
  if (!want()) return;

  if constexpr (MOM) {
    float* part = d.chunks > 1 ? d.partial + (n * d.chunks + chunk) * (2 * K + 1) : nullptr;
    if (h == 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int row = 32 * (4 * b + wave) + r;
        if (row < K) {
          if (part != nullptr) {
            part[row] = rsum[b];
            part[K + row] = sq_s[row];
          } else {
            if (d.probs != nullptr) d.probs[n * K + row] = rsum[b] / (float)S;
            if (d.probs_sq != nullptr) d.probs_sq[n * K + row] = sq_s[row] / (float)S;
          }
        }
      }
    }
    if (tid == 0) {
      if (part != nullptr) part[2 * K] = hsum;
      else if (d.entropy != nullptr) d.entropy[n] = hsum / (float)S;
    }
  } else {
    if (h == 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int row = 32 * (4 * b + wave) + r;
        if (row < K) {
          if (d.chunks > 1) d.partial[(n * d.chunks + chunk) * K + row] = rsum[b];
          else d.probs[n * K + row] = rsum[b] / (float)S;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(HMC_THREADS) hmc_kernel(const HmcBatch batch) {
  __shared__ float Bs[2][32 * HMC_BP];
  __shared__ float Ts[HMC_THREADS / 64][32 * HMC_TP];
  __shared__ float red[2][4][HMC_TILE];
  __shared__ float mu_s[HMC_K_MAX];
  const HmcItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long local = (long long)blockIdx.x - d.base;
  const int nb = (d.K + 127) >> 7;
  if (nb <= 1) hmc_block<1>(d, local, Bs, Ts, red, mu_s);
  else if (nb <= 2) hmc_block<2>(d, local, Bs, Ts, red, mu_s);
  else if (nb <= 4) hmc_block<4>(d, local, Bs, Ts, red, mu_s);
  else hmc_block<8>(d, local, Bs, Ts, red, mu_s);
}

__global__ void __launch_bounds__(HMC_THREADS) hmm_kernel(const HmmBatch batch) {
  __shared__ float Bs[2][32 * HMC_BP];
  __shared__ float Ts[HMC_THREADS / 64][32 * HMC_TP];
  __shared__ float red[3][4][HMC_TILE];
  __shared__ float mu_s[HMC_K_MAX];
  __shared__ float sq_s[HMC_K_MAX];
  const HmmItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long local = (long long)blockIdx.x - d.base;
  const int nb = (d.K + 127) >> 7;
  if (nb <= 1) hmc_block<1>(d, local, Bs, Ts, red, mu_s, sq_s);
  else if (nb <= 2) hmc_block<2>(d, local, Bs, Ts, red, mu_s, sq_s);
  else if (nb <= 4) hmc_block<4>(d, local, Bs, Ts, red, mu_s, sq_s);
  else hmc_block<8>(d, local, Bs, Ts, red, mu_s, sq_s);
}

// The chunks of an input in chunk order: one thread per (n, k).  Blocks of an item: ceil(N K / 256), none where its inputs
// have one chunk.
__global__ void __launch_bounds__(HMC_THREADS) hmc_reduce_kernel(const HmcBatch batch) {
  const HmcItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long idx = ((long long)blockIdx.x - d.base) * HMC_THREADS + threadIdx.x;
  if (idx >= (long long)d.N * d.K) return;
  const long long n = idx / d.K;
  const int k = (int)(idx - n * d.K);
  const float* p = d.partial + n * d.chunks * d.K + k;
  float v = 0.f;
  for (int c = 0; c < d.chunks; ++c) v += p[(long long)c * d.K];
  d.probs[idx] = v / (float)d.S;
}

// The same for the 2 K + 1 sums of an input: one thread per (n, j), j < K a probability, j < 2 K a square, j = 2 K the
// entropy.  Blocks of an item: ceil(N (2 K + 1) / 256).
__global__ void __launch_bounds__(HMC_THREADS) hmm_reduce_kernel(const HmmBatch batch) {
  const HmmItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long idx = ((long long)blockIdx.x - d.base) * HMC_THREADS + threadIdx.x;
  const int per = 2 * d.K + 1;
  if (idx >= (long long)d.N * per) return;
  const long long n = idx / per;
  const int j = (int)(idx - n * per);
  const float* p = d.partial + n * d.chunks * per + j;
  float v = 0.f;
  for (int c = 0; c < d.chunks; ++c) v += p[(long long)c * per];
  v /= (float)d.S;
  float* out = j < d.K ? d.probs : j < 2 * d.K ? d.probs_sq : d.entropy;
  if (out != nullptr) out[j < d.K ? n * d.K + j : j < 2 * d.K ? n * d.K + (j - d.K) : n] = v;
}

// The body of both entries: plans, workspace, the items of a batch (`extra` fills what an Item has beyond HmcItem and
// says whether the item has sums to reduce and how many per input), the main launch and the reduce launch.
template <typename Item, typename Desc, typename Extra>
int hmc_enqueue(const char* name, hipStream_t stream, const Desc* descs, int n, void* workspace, size_t workspace_bytes,
                bool (*plan_of)(const Desc&, int, HmcPlan*), void (*kernel)(const ArgBatch<Item, HMC_BATCH>),
                void (*reduce_kernel)(const ArgBatch<Item, HMC_BATCH>), Extra extra) {
  std::vector<HmcPlan> plans;
  if (!side::plans_of(name, descs, n, plan_of, &plans)) return CURV_ERR_INVALID;
  for (int i = 0; i < n; ++i) CURV_REQUIRE(descs[i].d2 && descs[i].mu, "%s: item %d: null d2 or mu", name, i);
  const size_t need = hmc_bytes_of(plans);
  if (need > 0) {
    const int rc = side::require_workspace(name, workspace, workspace_bytes, need, 256);
    if (rc != CURV_OK) return rc;
  }
  size_t at = 0;
  return for_arg_batches<Item, HMC_BATCH, 2>(
      n, name,
      [&](int i, Item* P, long long* units) {
        const Desc& d = descs[i];
        const HmcPlan& p = plans[i];
        P->M = d.M; P->d2 = d.d2; P->mu = d.mu; P->Z = d.Z;
        P->probs = d.probs; P->draws = d.draws;
        P->partial = p.bytes ? (float*)((char*)workspace + at) : nullptr;
        at += p.bytes;
        P->m_rs = d.m_rs; P->d_ns = d.d_ns; P->d_cs = d.d_cs; P->mu_ns = d.mu_ns; P->z_ns = d.z_ns; P->z_ss = d.z_ss;
        P->seed = d.seed; P->offset = d.offset;
        P->N = d.N; P->K = d.K; P->S = d.S; P->lower = d.m_lower;
        P->chunk_tiles = p.chunk_tiles; P->chunks = p.chunks;
        P->base = 0;
        const long long sums = extra(d, P);                     // per input; 0: nothing to reduce
        units[0] = (long long)d.N * p.chunks;
        units[1] = p.chunks > 1 ? cdivll((long long)d.N * sums, HMC_THREADS) : 0;
      },
      [](int, long long units) { return units; },
      [&](const ArgBatch<Item, HMC_BATCH>* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(kernel, dim3(grid[0]), dim3(HMC_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        if (grid[1] > 0) {
          hipLaunchKernelGGL(reduce_kernel, dim3(grid[1]), dim3(HMC_THREADS), 0, stream, b[1]);
          CURV_LAUNCH_CHECK();
        }
        return CURV_OK;
      });
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_head_mc_workspace_bytes(const curv_head_mc_desc* descs, int n) {
  return side::workspace_bytes("curv_head_mc_workspace_bytes", descs, n, hmc_plan_of, hmc_bytes_of);
}

extern "C" int curv_head_mc_plan_flops(const curv_head_mc_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_head_mc_plan_flops", descs, n, out, hmc_plan_of);
}

extern "C" int curv_head_mc(void* stream_, const curv_head_mc_desc* descs, int n, void* workspace,
                            size_t workspace_bytes) {
  if (n <= 0) return CURV_OK;
  return hmc_enqueue<HmcItem>("curv_head_mc", (hipStream_t)stream_, descs, n, workspace, workspace_bytes, hmc_plan_of,
                              hmc_kernel, hmc_reduce_kernel,
                              [](const curv_head_mc_desc& d, HmcItem*) { return d.probs ? (long long)d.K : 0LL; });
}

extern "C" size_t curv_head_mc_moments_workspace_bytes(const curv_head_moments_desc* descs, int n) {
  return side::workspace_bytes("curv_head_mc_moments_workspace_bytes", descs, n, hmm_plan_of, hmc_bytes_of);
}

extern "C" int curv_head_mc_moments_plan_flops(const curv_head_moments_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_head_mc_moments_plan_flops", descs, n, out, hmm_plan_of);
}

extern "C" int curv_head_mc_moments(void* stream_, const curv_head_moments_desc* descs, int n, void* workspace,
                                    size_t workspace_bytes) {
  if (n <= 0) return CURV_OK;
  return hmc_enqueue<HmmItem>("curv_head_mc_moments", (hipStream_t)stream_, descs, n, workspace, workspace_bytes,
                              hmm_plan_of, hmm_kernel, hmm_reduce_kernel,
                              [](const curv_head_moments_desc& d, HmmItem* P) {
                                P->entropy = d.entropy;
                                P->probs_sq = d.probs_sq;
                                return d.probs || d.entropy || d.probs_sq ? 2LL * d.K + 1 : 0LL;
                              });
}
