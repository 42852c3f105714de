// curv_logsum_grid: out[segment][pair] = weight * sum_e log(gain[pair] * max(x_e, 0) + shift[pair]) over whole-model
// arenas, for up to 16 (gain, shift) pairs in one read of the data - the log-determinant part of the Laplace evidence
// (Curvature.log_det_grid), and sum_e x_e^2 for its prior part.  fp64 from the load on, one logarithm per lane and pair
// (of the product of its 16 mantissas, the exponents summed exactly: `ls_take`); no atomics: a workgroup owns one
// 4096-element chunk of one segment and writes one partial per pair, a second stage sums a segment's partials in index
// order and a third the segments in table order, so a result has the same bits alone, in a batch and on a repeat call
// (DESIGN.md K21).
#include <cmath>
#include <vector>

#include "common.h"
#include "kernarg.h"

namespace curv {

constexpr int LS_CHUNK = CURV_LOGSUM_CHUNK;        // elements per workgroup
constexpr int LS_THREADS = 256;
constexpr int LS_PER_THREAD = LS_CHUNK / LS_THREADS;
constexpr int LS_MAX = CURV_LOGSUM_GRID_MAX;
static_assert(LS_PER_THREAD == 16, "four 16-byte loads of fp32 per lane");

// A row of the device table: the caller's descriptor and where the segment's chunks start.
struct LsRow {
  const void* x;
  long long count, stride;
  double weight;
  double gain[LS_MAX], shift[LS_MAX];
  int dtype, mode;
  int first_chunk, chunks;
};
static_assert(sizeof(LsRow) == CURV_LOGSUM_ROW_BYTES, "curv_logsum_workspace_bytes states the row size");
constexpr int LS_UPLOAD_CHUNK = 12;                // rows per launch of the table upload (upload_table, kernarg.h)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // every lane ends with the same bits
  return v;
}

// One element into the lane's running values.  Logarithms (MODE 0): the lane does not take 16 logarithms per pair but ONE -
// gain * x+ + shift is split into mantissa (in [0.5, 1)) and exponent, the mantissas are multiplied (16 of them: at least
// 2^-16, no underflow; 16 roundings of 2^-53, less than the error of 16 logarithms of terms up to 40 in size) and the
// exponents summed exactly; `ls_close` turns the pair into log(product) + exponents * ln 2.  gain, shift >= 0 (checked on the
// host) and x+ >= 0 keep the argument from being negative; 0, inf and NaN pass through the product as through a sum of logs.
// Squares (MODE 1): acc[0] += x * x.
template <int MODE>
__device__ __forceinline__ void ls_take(double (&acc)[LS_MAX], int (&ex)[LS_MAX], double x, const double* __restrict__ gain,
                                        const double* __restrict__ shift, int pairs) {
  if (MODE == 1) {
    acc[0] = fma(x, x, acc[0]);
  } else {
    const double xp = x > 0.0 ? x : 0.0;
#pragma unroll
    for (int p = 0; p < LS_MAX; ++p)
      if (p < pairs) {
        const double y = fma(gain[p], xp, shift[p]);
        acc[p] *= __builtin_amdgcn_frexp_mant(y);
        ex[p] += __builtin_amdgcn_frexp_exp(y);
      }
  }
}

// The lane's sum of logarithms from its product of mantissas and its sum of exponents.
__device__ __forceinline__ void ls_close(double (&acc)[LS_MAX], const int (&ex)[LS_MAX], int pairs) {
  constexpr double LN2 = 0.693147180559945309417232121458;
#pragma unroll
  for (int p = 0; p < LS_MAX; ++p)
    if (p < pairs) acc[p] = fma((double)ex[p], LN2, log(acc[p]));
}

// The 16 elements of a lane in a fixed order.  Contiguous, 16-byte aligned fp32: element 4 (t + 256 u) + c of the chunk
// for u = 0..3, c = 0..3, four at a time; otherwise element t + 256 k for k = 0..15, one at a time.
template <int MODE>
__device__ __forceinline__ void ls_chunk_sums(double (&acc)[LS_MAX], int (&ex)[LS_MAX], const LsRow& d, long long base,
                                              int pairs) {
  const long long left = d.count - base;           // > 0
  const int t = threadIdx.x;
  const bool vec = d.dtype == CURV_DTYPE_F32 && d.stride == 1 && (reinterpret_cast<uintptr_t>(d.x) & 15) == 0;
  if (vec) {
    const float* x = static_cast<const float*>(d.x) + base;          // base is a multiple of 4096: still aligned
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long e = 4LL * (t + LS_THREADS * u);
      if (e + 3 < left) {
        const float4 v = *reinterpret_cast<const float4*>(x + e);
        ls_take<MODE>(acc, ex, (double)v.x, d.gain, d.shift, pairs);
        ls_take<MODE>(acc, ex, (double)v.y, d.gain, d.shift, pairs);
        ls_take<MODE>(acc, ex, (double)v.z, d.gain, d.shift, pairs);
        ls_take<MODE>(acc, ex, (double)v.w, d.gain, d.shift, pairs);
      } else {
        for (long long j = e; j < left && j < e + 4; ++j) ls_take<MODE>(acc, ex, (double)x[j], d.gain, d.shift, pairs);
      }
    }
  } else if (d.dtype == CURV_DTYPE_F32) {
    const float* x = static_cast<const float*>(d.x);
    for (int k = 0; k < LS_PER_THREAD; ++k) {
      const long long e = t + LS_THREADS * k;
      if (e < left) ls_take<MODE>(acc, ex, (double)x[(base + e) * d.stride], d.gain, d.shift, pairs);
    }
  } else {
    const double* x = static_cast<const double*>(d.x);
    for (int k = 0; k < LS_PER_THREAD; ++k) {
      const long long e = t + LS_THREADS * k;
      if (e < left) ls_take<MODE>(acc, ex, x[(base + e) * d.stride], d.gain, d.shift, pairs);
    }
  }
}

// Stage 1: partial[chunk][pair], the chunk's segment found from the prefix of chunk counts (first_chunk ascending;
// a segment without elements has no chunk and shares its first_chunk with its successor, which the search prefers).
__global__ void __launch_bounds__(LS_THREADS)
logsum_chunk_kernel(const LsRow* __restrict__ table, int n, int pairs, double* __restrict__ partial) {
  __shared__ double wave_part[LS_THREADS / 64][LS_MAX];
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_chunk <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const LsRow& d = table[lo];
  const long long base = (long long)((int)blockIdx.x - d.first_chunk) * LS_CHUNK;
  double acc[LS_MAX];
  int ex[LS_MAX];
  const double start = d.mode == 1 ? 0.0 : 1.0;    // an empty sum, an empty product
#pragma unroll
  for (int p = 0; p < LS_MAX; ++p) { acc[p] = start; ex[p] = 0; }
  if (d.mode == 1) {
    ls_chunk_sums<1>(acc, ex, d, base, pairs);
  } else {
    ls_chunk_sums<0>(acc, ex, d, base, pairs);
    ls_close(acc, ex, pairs);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int p = 0; p < LS_MAX; ++p) {
    if (p < pairs) {
      const double s = wave_sum_f64(acc[p]);
      if (lane == 0) wave_part[wave][p] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < pairs) {
    double s = wave_part[0][threadIdx.x];
    for (int w = 1; w < LS_THREADS / 64; ++w) s += wave_part[w][threadIdx.x];
    partial[(long long)blockIdx.x * pairs + threadIdx.x] = s;
  }
}

// Stage 2: out[segment][pair] = weight * (partials of the segment, summed in index order).  A mode-1 segment has a
// column 0 only.
__global__ void __launch_bounds__(64)
logsum_segment_kernel(const LsRow* __restrict__ table, int pairs, const double* __restrict__ partial,
                      double* __restrict__ out, long long out_stride) {
  const LsRow& d = table[blockIdx.x];
  const int p = threadIdx.x;
  if (p >= (d.mode == 1 ? 1 : pairs)) return;
  double s = 0.0;
  const double* part = partial + (long long)d.first_chunk * pairs + p;
  for (int c = 0; c < d.chunks; ++c) s += part[(long long)c * pairs];
  out[(long long)blockIdx.x * out_stride + p] = d.chunks > 0 ? d.weight * s : 0.0;
}

// Stage 3: total[pair] = out[0][pair] + out[1][pair] + ... in table order.
__global__ void __launch_bounds__(64)
logsum_total_kernel(const LsRow* __restrict__ table, int n, int pairs, const double* __restrict__ out,
                    long long out_stride, double* __restrict__ total) {
  const int p = threadIdx.x;
  if (p >= pairs) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i)
    if (p == 0 || table[i].mode != 1) s += out[(long long)i * out_stride + p];
  total[p] = s;
}

static long long ls_chunks(long long count) { return (count + LS_CHUNK - 1) / LS_CHUNK; }

// Checks the table; *chunks gets the number of stage-1 workgroups.
static int ls_validate(const char* who, const curv_logsum_desc* descs, int n, int pairs, long long* chunks) {
  CURV_REQUIRE(n >= 0 && (n == 0 || descs != nullptr), "%s: bad arguments", who);
  CURV_REQUIRE(pairs >= 1 && pairs <= LS_MAX, "%s: pairs %d outside 1 .. %d", who, pairs, LS_MAX);
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    const curv_logsum_desc& s = descs[i];
    CURV_REQUIRE(s.count >= 0, "%s: segment %d: negative count %lld", who, i, (long long)s.count);
    CURV_REQUIRE(s.dtype == CURV_DTYPE_F32 || s.dtype == CURV_DTYPE_F64, "%s: segment %d: unknown dtype %d", who, i,
                 s.dtype);
    CURV_REQUIRE(s.mode == CURV_LOGSUM_LOG || s.mode == CURV_LOGSUM_SQUARES, "%s: segment %d: unknown mode %d", who, i,
                 s.mode);
    CURV_REQUIRE(s.count == 0 || s.x != nullptr, "%s: segment %d: null pointer with count %lld", who, i,
                 (long long)s.count);
    CURV_REQUIRE(s.count == 0 || s.stride >= 1, "%s: segment %d: stride %lld below 1", who, i, (long long)s.stride);
    for (int p = 0; s.mode == CURV_LOGSUM_LOG && p < pairs; ++p)
      CURV_REQUIRE(s.gain[p] >= 0.0 && s.shift[p] >= 0.0, "%s: segment %d: pair %d: gain %g and shift %g must not be negative",
                   who, i, p, s.gain[p], s.shift[p]);
    const uintptr_t width = s.dtype == CURV_DTYPE_F64 ? 8 : 4;
    CURV_REQUIRE((reinterpret_cast<uintptr_t>(s.x) & (width - 1)) == 0, "%s: segment %d: pointer not aligned to its elements",
                 who, i);
    total += ls_chunks(s.count);
    CURV_REQUIRE(total < (1LL << 31) / LS_MAX, "%s: segment %d: too many elements", who, i);
  }
  *chunks = total;
  return CURV_OK;
}

}  // namespace curv

using namespace curv;

extern "C" size_t curv_logsum_workspace_bytes(const curv_logsum_desc* descs, int n, int pairs) {
  long long chunks = 0;
  if (ls_validate("curv_logsum_workspace_bytes", descs, n, pairs, &chunks) != CURV_OK) return 0;
  return (size_t)n * sizeof(LsRow) + (size_t)chunks * pairs * sizeof(double);
}

extern "C" int curv_logsum_grid(void* stream_, const curv_logsum_desc* descs, int n, int pairs, double* out,
                                long long out_stride, double* total, void* workspace, size_t workspace_bytes) {
  if (n == 0) return CURV_OK;
  long long chunks = 0;
  const int rcv = ls_validate("curv_logsum_grid", descs, n, pairs, &chunks);
  if (rcv != CURV_OK) return rcv;
  CURV_REQUIRE(out != nullptr && out_stride >= pairs, "curv_logsum_grid: null output or out_stride %lld below pairs %d",
               out_stride, pairs);
  const size_t need = (size_t)n * sizeof(LsRow) + (size_t)chunks * pairs * sizeof(double);
  if (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) {
    set_error("curv_logsum_grid: workspace too small (%zu < %zu bytes) or not 8-byte aligned", workspace_bytes, need);
    return CURV_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  LsRow* table = static_cast<LsRow*>(workspace);
  double* partial = reinterpret_cast<double*>(table + n);
  std::vector<LsRow> rows((size_t)n);
  long long at = 0;
  for (int i = 0; i < n; ++i) {
    const curv_logsum_desc& s = descs[i];
    LsRow& r = rows[i];
    memset(&r, 0, sizeof(r));
    r.x = s.x; r.count = s.count; r.stride = s.stride; r.weight = s.weight;
    memcpy(r.gain, s.gain, sizeof(r.gain));
    memcpy(r.shift, s.shift, sizeof(r.shift));
    r.dtype = s.dtype; r.mode = s.mode;
    r.first_chunk = (int)at; r.chunks = (int)ls_chunks(s.count);
    at += r.chunks;
  }
  const int rcu = upload_table<LS_UPLOAD_CHUNK>(stream, table, rows.data(), n);
  if (rcu != CURV_OK) return rcu;
  if (chunks > 0) {
    hipLaunchKernelGGL(logsum_chunk_kernel, dim3((unsigned)chunks), dim3(LS_THREADS), 0, stream, table, n, pairs, partial);
    CURV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(logsum_segment_kernel, dim3((unsigned)n), dim3(64), 0, stream, table, pairs, partial, out, out_stride);
  CURV_LAUNCH_CHECK();
  if (total != nullptr) {
    hipLaunchKernelGGL(logsum_total_kernel, dim3(1), dim3(64), 0, stream, table, n, pairs, out, out_stride, total);
    CURV_LAUNCH_CHECK();
  }
  return CURV_OK;
}
