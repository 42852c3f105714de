// Monte-Carlo softmax of the linearised Laplace predictive from the joint logit covariance (curv_logit_mc,
// include/curv_hip.h):
//   probs[n][c] = (1/S) sum_s softmax([f_s, rest[n]])[c],   f_s = mu_n + L_n z_s,   L_n L_n^T = Sigma_n   (K x K, K <= 16)
// One kernel reads Sigma and the logits once and writes (N, K): the (N, S, K) draws exist only in registers (unless the
// caller asks for them).
//
// Workgroup (256 threads) = (item, input n, chunk of the draws).  Three phases:
//   1. Cholesky.  The lower triangle of Sigma_n goes to LDS as fp64 (only c' <= c is read), thread i < K owns row i of L
//      and the columns are worked through left to right, one barrier per column: every thread forms the pivot
//      d_j = Sigma_jj - sum_{k < j} L_jk**2 itself from broadcast LDS reads (so the decision about column j is the same
//      in every thread without an exchange), thread i >= j forms L_ij.  fp64 throughout - the library's rule for
//      factorisations - and L is then kept as fp32 rows of 16 in LDS, zero above the diagonal and at or beyond K.
//      Sigma_n is positive SEMI-definite and often singular (more outputs than the rank of the Jacobians, an output
//      without variance): with thr = 16 * 2^-23 * max_c Sigma_cc (the fp32 entries carry about 2^-23 of the largest
//      diagonal entry as error; 16 is the largest K) a pivot d_j <= thr makes column j exact zeros - the draw then has no
//      component along it - and is counted in info[n]; a pivot below -thr (not a covariance) is dropped the same way and
//      info[n] = -(j + 1) names the first one.  Nothing non-finite comes from finite input, nothing aborts or waits.
//      Every chunk of an input repeats the factorisation (about K^3 / 3 fp64 operations spread over K threads) rather
//      than hand L over through memory: chunks exist only where there are few inputs.
//   2. Draws.  Every lane owns whole draws s = chunk start + tid, + 256, ...: z from the caller's Z or from KQ =
//      ceil(K / 4) Philox counters (philox.h: the same four values per counter as curv_randn), f = mu + L z against
//      broadcast ds_read_b128 of the rows of L (whole quads c' < 4 (c / 4 + 1): the zeros above the diagonal cost at most
//      24 of 160 multiply-adds), one max over [f, rest], 4 KQ + 1 exp, one reciprocal, and 4 KQ + 1 running sums in
//      registers.  The kernel is instantiated per KQ so that z, f and the sums stay in registers; classes at or beyond K
//      in the last quad carry mu = -inf and a zero row of L, so they add exactly 0.
//   3. Sums.  Each running sum is reduced over the wave by DPP (wave_sum.h), lane 63 leaves it in LDS, thread k adds the
//      four waves in wave order.  An input with one chunk is finished there (x 1/S, written); otherwise the K + 1 sums go
//      to partial[n][chunk][k] in the caller's workspace and a second launch adds the chunks in chunk order.
// Fixed order everywhere (lane, wave, workgroup, chunks), no atomics; the chunk length of an item follows from its own N
// and S only (lmc_plan_of), so its bits are the same alone and in a batch.  All global stores are plain vector stores.
#include "philox.h"
#include "side_build.h"
#include "wave_sum.h"

#include <cmath>

namespace curv {
namespace {

constexpr int LMC_THREADS = 256;
constexpr int LMC_BATCH = 16;                  // items per launch (tables as kernel arguments)
constexpr int LMC_BLOCKS_TARGET = 1024;        // the draws of an input are cut into chunks until an item has about this many workgroups
constexpr int LMC_K_MAX = CURV_PERSAMPLE_COV_MAX_OUTPUTS;
constexpr int LMC_S_MAX = 1 << 30;
static_assert(LMC_K_MAX == 16, "lmc_kernel instantiates 1 .. 4 quads of classes; rows of L are 16 floats");

struct LmcItem {
  const float* cov;
  const float* mu;
  const float* rest;           // may be null: every class is selected
  const float* Z;              // may be null: Philox
  float* probs;
  float* probs_rest;
  float* draws;
  int* info;
  float* partial;              // [n][chunk][K + 1], used when chunks > 1
  long long o_ns, o_rs, mu_ns, z_ns, z_ss;
  unsigned long long seed, offset;
  int N, K, S;
  int chunk, chunks;           // draws per workgroup (a multiple of 256), workgroups per input
  long long base;              // first workgroup / reduce block of this item in the launch
};

typedef ArgBatch<LmcItem, LMC_BATCH> LmcBatch;
static_assert(sizeof(LmcBatch) <= 3840, "kernel argument block must stay below 4 KB");

struct LmcPlan {
  int chunk, chunks;
  size_t bytes;
  long long flops;
};

bool lmc_plan_of(const curv_logit_mc_desc& d, int index, LmcPlan* p) {
  const char* const who = "curv_logit_mc";
  if (d.K < 1 || d.K > LMC_K_MAX) {
    set_error("%s: item %d: K %d outside 1 .. %d", who, index, d.K, LMC_K_MAX);
    return false;
  }
  if (d.N < 1 || d.S < 1 || d.S > LMC_S_MAX || (long long)d.N * d.S > (1LL << 40)) {
    set_error("%s: item %d: invalid sizes (N %d S %d: both at least 1, S at most 2^30, N S at most 2^40)", who, index, d.N,
              d.S);
    return false;
  }
  if (d.o_rs < d.K || d.o_ns < (long long)d.K * d.o_rs || d.mu_ns < d.K) {
    set_error("%s: item %d: invalid strides (o_rs %lld below K %d, o_ns %lld below K o_rs, or mu_ns %lld below K)", who,
              index, d.o_rs, d.K, d.o_ns, d.mu_ns);
    return false;
  }
  if (d.Z != nullptr && (d.z_ss < d.K || d.z_ns < (long long)(d.S - 1) * d.z_ss + d.K)) {
    set_error("%s: item %d: invalid strides (z_ss %lld below K %d, or z_ns %lld below (S - 1) z_ss + K)", who, index,
              d.z_ss, d.K, d.z_ns);
    return false;
  }
  if (!d.probs && !d.probs_rest && !d.draws && !d.info) {
    set_error("%s: item %d: no output (probs, probs_rest, draws and info are all null)", who, index);
    return false;
  }
  const long long per = cdivll(d.S, cdivll(LMC_BLOCKS_TARGET, d.N));
  p->chunk = (int)std::max<long long>(LMC_THREADS, cdivll(per, LMC_THREADS) * LMC_THREADS);
  p->chunks = cdiv(d.S, p->chunk);
  p->bytes = p->chunks > 1 ? align_up((size_t)d.N * p->chunks * (d.K + 1) * sizeof(float), 256) : 0;
  const int kq = cdiv(d.K, 4);
  p->flops = 2LL * d.N * d.S * (8LL * kq * (kq + 1));        // whole quads of L per row: 16 KQ (KQ + 1) / 2 per draw
  return true;
}

size_t lmc_bytes_of(const std::vector<LmcPlan>& plans) {
  size_t total = 0;
  for (const LmcPlan& p : plans) total += p.bytes;
  return total;
}

template <int KQ>
__device__ __forceinline__ void lmc_block(const LmcItem& d, long long local, double (*A)[LMC_K_MAX + 1],
                                          double (*Ld)[LMC_K_MAX + 1], float (*Lf)[LMC_K_MAX], float* mu_s,
                                          float (*red)[LMC_K_MAX + 1]) {
  constexpr int KP = 4 * KQ;
  const int tid = threadIdx.x, K = d.K, S = d.S;
  const long long n = local / d.chunks;
  const int chunk = (int)(local - n * d.chunks);

  // ---- 1. Sigma_n (lower triangle) as fp64, L zeroed, the logits
  {
    const int c = tid >> 4, c2 = tid & 15;
    if (c < K && c2 <= c) A[c][c2] = (double)d.cov[n * d.o_ns + c * d.o_rs + c2];
    Lf[c][c2] = 0.f;
    if (tid < LMC_K_MAX) mu_s[tid] = tid < K ? d.mu[n * d.mu_ns + tid] : -INFINITY;
  }
  __syncthreads();
  double top = 0.0;
  for (int c = 0; c < K; ++c) top = fmax(top, A[c][c]);
  const double thr = top * (16.0 / 8388608.0);
  int dropped = 0, bad = 0;
  for (int j = 0; j < K; ++j) {
    double dj = A[j][j];
    for (int k = 0; k < j; ++k) dj = fma(-Ld[j][k], Ld[j][k], dj);
    const bool keep = dj > thr;
    if (!keep) {
      ++dropped;
      if (bad == 0 && dj < -thr) bad = -(j + 1);
    }
    if (tid >= j && tid < K) {
      double l = 0.0;
      if (keep) {
        double s = A[tid][j];
        for (int k = 0; k < j; ++k) s = fma(-Ld[tid][k], Ld[j][k], s);
        const double root = sqrt(dj);
        l = tid == j ? root : s / root;
      }
      Ld[tid][j] = l;
      Lf[tid][j] = (float)l;
    }
    __syncthreads();
  }
  if (chunk == 0 && tid == 0 && d.info != nullptr) d.info[n] = bad != 0 ? bad : dropped;

  // ---- 2. the draws of this chunk
  const float rest = d.rest != nullptr ? d.rest[n] : -INFINITY;
  const bool want_probs = d.probs != nullptr || d.probs_rest != nullptr;
  float mu[KP], acc[KP], acc_rest = 0.f;
#pragma unroll
  for (int c = 0; c < KP; ++c) {
    mu[c] = mu_s[c];
    acc[c] = 0.f;
  }
  const int s1 = min(S, (chunk + 1) * d.chunk);        // (chunk + 1) * d.chunk < S + d.chunk <= 2^30 + S
  for (int s = chunk * d.chunk + tid; s < s1; s += LMC_THREADS) {
    float z[KP], f[KP];
    // (L stays in LDS: without the fence the compiler keeps all of it in registers across the loop, 160 of them at KQ = 4,
    // which leaves one workgroup per CU and nothing to run beside another's factorisation)
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    if (d.Z != nullptr) {
      const float* zp = d.Z + n * d.z_ns + (long long)s * d.z_ss;
#pragma unroll
      for (int c = 0; c < KP; ++c) z[c] = c < K ? zp[c] : 0.f;
    } else {
      const unsigned long long ctr = d.offset + ((unsigned long long)n * S + s) * KQ;
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        float z4[4];
        philox_normal4(d.seed, ctr + q, z4);
#pragma unroll
        for (int e = 0; e < 4; ++e) z[4 * q + e] = z4[e];
      }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) {
      float v = mu[c];
#pragma unroll
      for (int q = 0; q <= c / 4; ++q) {
        const float4 l4 = *reinterpret_cast<const float4*>(&Lf[c][4 * q]);
        v = fmaf(l4.x, z[4 * q], v);
        v = fmaf(l4.y, z[4 * q + 1], v);
        v = fmaf(l4.z, z[4 * q + 2], v);
        v = fmaf(l4.w, z[4 * q + 3], v);
      }
      f[c] = v;
    }
    if (d.draws != nullptr) {
      float* dp = d.draws + (n * S + s) * K;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < K) dp[c] = f[c];
    }
    if (want_probs) {
      float m = rest;
#pragma unroll
      for (int c = 0; c < KP; ++c) m = fmaxf(m, f[c]);
      const float e_rest = expf(rest - m);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < KP; ++c) {
        f[c] = expf(f[c] - m);
        sum += f[c];
      }
      const float inv = 1.0f / (sum + e_rest);
#pragma unroll
      for (int c = 0; c < KP; ++c) acc[c] = fmaf(f[c], inv, acc[c]);
      acc_rest = fmaf(e_rest, inv, acc_rest);
    }
  }
  if (!want_probs) return;

  // ---- 3. lane sums -> wave (DPP) -> workgroup (wave order) -> output or partial
  const int wave = tid >> 6;
#pragma unroll
  for (int c = 0; c < KP; ++c) {
    const float v = wave_sum_dpp(acc[c]);
    if ((tid & 63) == 63) red[wave][c] = v;
  }
  acc_rest = wave_sum_dpp(acc_rest);
  if ((tid & 63) == 63) red[wave][LMC_K_MAX] = acc_rest;
  __syncthreads();
  if (tid <= K) {
    const int k = tid < K ? tid : LMC_K_MAX;
    float v = red[0][k];
    for (int w = 1; w < LMC_THREADS / 64; ++w) v += red[w][k];
    if (d.chunks > 1) {
      d.partial[(n * d.chunks + chunk) * (K + 1) + tid] = v;
    } else {
      v /= (float)S;
      if (tid < K) {
        if (d.probs != nullptr) d.probs[n * K + tid] = v;
      } else if (d.probs_rest != nullptr) {
        d.probs_rest[n] = v;
      }
    }
  }
}

__global__ void __launch_bounds__(LMC_THREADS, 2) lmc_kernel(const LmcBatch batch) {
  __shared__ double A[LMC_K_MAX][LMC_K_MAX + 1];
  __shared__ double Ld[LMC_K_MAX][LMC_K_MAX + 1];
  __shared__ __attribute__((aligned(16))) float Lf[LMC_K_MAX][LMC_K_MAX];
  __shared__ float mu_s[LMC_K_MAX];
  __shared__ float red[LMC_THREADS / 64][LMC_K_MAX + 1];
  const LmcItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long local = (long long)blockIdx.x - d.base;
  switch ((d.K + 3) >> 2) {
    case 1: lmc_block<1>(d, local, A, Ld, Lf, mu_s, red); break;
    case 2: lmc_block<2>(d, local, A, Ld, Lf, mu_s, red); break;
    case 3: lmc_block<3>(d, local, A, Ld, Lf, mu_s, red); break;
    default: lmc_block<4>(d, local, A, Ld, Lf, mu_s, red); break;
  }
}

// The chunks of an input in chunk order: one thread per (n, k), k < K the classes, k = K the rest.  Blocks of an item:
// ceil(N (K + 1) / 256), none where its inputs have one chunk.
__global__ void __launch_bounds__(LMC_THREADS) lmc_reduce_kernel(const LmcBatch batch) {
  const LmcItem& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long idx = ((long long)blockIdx.x - d.base) * LMC_THREADS + threadIdx.x;
  const int K1 = d.K + 1;
  if (idx >= (long long)d.N * K1) return;
  const long long n = idx / K1;
  const int k = (int)(idx - n * K1);
  const float* p = d.partial + n * d.chunks * K1 + k;
  float v = 0.f;
  for (int c = 0; c < d.chunks; ++c) v += p[(long long)c * K1];
  v /= (float)d.S;
  if (k < d.K) {
    if (d.probs != nullptr) d.probs[n * d.K + k] = v;
  } else if (d.probs_rest != nullptr) {
    d.probs_rest[n] = v;
  }
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_logit_mc_workspace_bytes(const curv_logit_mc_desc* descs, int n) {
  return side::workspace_bytes("curv_logit_mc_workspace_bytes", descs, n, lmc_plan_of, lmc_bytes_of);
}

extern "C" int curv_logit_mc_plan_flops(const curv_logit_mc_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_logit_mc_plan_flops", descs, n, out, lmc_plan_of);
}

extern "C" int curv_logit_mc(void* stream_, const curv_logit_mc_desc* descs, int n, void* workspace,
                             size_t workspace_bytes) {
  const char* const name = "curv_logit_mc";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<LmcPlan> plans;
  if (!side::plans_of(name, descs, n, lmc_plan_of, &plans)) return CURV_ERR_INVALID;
  for (int i = 0; i < n; ++i) CURV_REQUIRE(descs[i].cov && descs[i].mu, "%s: item %d: null cov or mu", name, i);
  const size_t need = lmc_bytes_of(plans);
  if (need > 0) {
    const int rc = side::require_workspace(name, workspace, workspace_bytes, need, 256);
    if (rc != CURV_OK) return rc;
  }
  size_t at = 0;
  return for_arg_batches<LmcItem, LMC_BATCH, 2>(
      n, name,
      [&](int i, LmcItem* P, long long* units) {
        const curv_logit_mc_desc& d = descs[i];
        const LmcPlan& p = plans[i];
        P->cov = d.cov; P->mu = d.mu; P->rest = d.rest; P->Z = d.Z;
        P->probs = d.probs; P->probs_rest = d.probs_rest; P->draws = d.draws; P->info = d.info;
        P->partial = p.bytes ? (float*)((char*)workspace + at) : nullptr;
        at += p.bytes;
        P->o_ns = d.o_ns; P->o_rs = d.o_rs; P->mu_ns = d.mu_ns; P->z_ns = d.z_ns; P->z_ss = d.z_ss;
        P->seed = d.seed; P->offset = d.offset;
        P->N = d.N; P->K = d.K; P->S = d.S;
        P->chunk = p.chunk; P->chunks = p.chunks;
        P->base = 0;
        units[0] = (long long)d.N * p.chunks;
        units[1] = p.chunks > 1 && (d.probs || d.probs_rest) ? cdivll((long long)d.N * (d.K + 1), LMC_THREADS) : 0;
      },
      [](int, long long units) { return units; },
      [&](const LmcBatch* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(lmc_kernel, dim3(grid[0]), dim3(LMC_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        if (grid[1] > 0) {
          hipLaunchKernelGGL(lmc_reduce_kernel, dim3(grid[1]), dim3(LMC_THREADS), 0, stream, b[1]);
          CURV_LAUNCH_CHECK();
        }
        return CURV_OK;
      });
}
