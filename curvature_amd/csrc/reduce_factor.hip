// KFAC-reduce factor build (curv_kfac_reduce_accumulate, include/curv_hip.h).
//
// A layer that applies its weight at L positions per sample is reduced over the positions first; the Gram then runs over
// the N samples only.  Per factor:
//   1. reduce pass: `src` is read once and the (N, dim) float32 row matrix is written into the workspace;
//   2. one curv_kfac_accumulate call on it as an (N, dim) flat source (it appends the ones row): one call per factor, so
//      a factor's launch plan - and with it its bits - follow from the factor's own geometry.
// Plane form (NCHW): row[n, (c, a, b)] = m sum_{oh, ow} xpad[n, c, oh sh + a - ph, ow sw + b - pw].  The output pixels that
// tap (a, b) reads inside the image are a product set R_a x C_b of rows and columns, so the pass forms the column-restricted
// row sums s_b[h] = sum_{w in C_b} x[h, w] (H kw values per plane) and then sum_{h in R_a} s_b[h]: H W kw + H kh kw
// additions per plane and no im2col.  Token form (N, T, E): row[n, e] = m sum_t x[n, t, e].
// A "plane" below is one (n, c) image of H x W values, or one sample of T x E values (H = T, W = E).
//
// A workgroup owns whole planes and every row entry of them: no atomics, and the order of each sum (columns, then rows,
// each on four interleaved accumulators; a plane longer than the tile in pieces of whole rows, ascending) follows from H, W
// and the window alone.
// Every launch goes on the caller's stream; nothing waits on the host or allocates, so the call can be captured.
#include "side_build.h"

#include <string>

namespace curv {
namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_TILE = 4096;            // values of a source run a workgroup stages as float32 (16 KB)
constexpr int RD_STILE = 4096;           // row sums s_b[h] a workgroup holds (16 KB): 32 KB of LDS, five workgroups to a CU
constexpr int RD_MIN_RUN = 1024;         // small planes are packed until a workgroup stages at least this many values ...
constexpr int RD_WGS = 512;              // ... and further while that leaves this many workgroups
constexpr size_t RD_ALIGN = 256;

struct Plan {
  int dim;                    // C kh kw or E (without the ones column)
  unsigned planes, H, W;      // N C planes of H x W, or N samples of T x E
  unsigned outs;              // row entries per plane: kh kw or E
  unsigned PP;                // planes per workgroup (> 1: whole planes only)
  unsigned TR, segw;          // rows and columns of a piece (PP > 1: H and W)
  int Ho, Wo;
  float inv;                  // 1 / L or 1
  size_t stage_bytes, build_bytes;   // the rows; the scratch of their build
  long long flops;
};

// The flat build's descriptor of the row matrix at `rows`.
curv_factor_desc flat_desc(const curv_reduce_factor_desc& d, int dim, const float* rows) {
  curv_factor_desc e{};
  e.src = rows;
  e.dst = d.dst;
  e.N = d.N; e.C = dim; e.H = 1; e.W = 1;
  e.kh = e.kw = e.sh = e.sw = 1;
  e.has_bias = d.has_bias ? 1 : 0;
  e.first = d.first ? 1 : 0;
  e.scale = d.scale;
  e.path_hint = CURV_PATH_AUTO;            // the call holds this factor only
  return e;
}

bool plan_of(const curv_reduce_factor_desc& d, int index, Plan* p) {
  const char* const who = "curv_kfac_reduce";
  *p = Plan{};
  if (d.dtype != CURV_DTYPE_F32 && d.dtype != CURV_DTYPE_BF16 && d.dtype != CURV_DTYPE_F16) {
    set_error("%s: factor %d: unknown dtype %d", who, index, d.dtype);
    return false;
  }
  long long L, adds;
  if (d.form == CURV_REDUCE_PLANE) {
    side::ConvGeom geom;
    if (!side::source_geom_of(d, who, "factor", index, &geom)) return false;      // sizes, stride >= 1, padding >= 0
    const long long Hp = (long long)d.H + 2LL * d.ph, Wp = (long long)d.W + 2LL * d.pw;
    if (d.kh > Hp || d.kw > Wp) {
      set_error("%s: factor %d: kernel larger than the padded input (H %d W %d kernel %dx%d padding %dx%d)", who, index,
                d.H, d.W, d.kh, d.kw, d.ph, d.pw);
      return false;
    }
    const long long taps = (long long)d.kh * d.kw, n = taps <= (1LL << 20) ? taps * d.C : taps;
    const long long planes = (long long)d.N * d.C;
    if (taps > (1LL << 20) || n > (1LL << 20) || planes >= (1LL << 31) || Hp >= (1LL << 30) || Wp >= (1LL << 30) ||
        d.kw > RD_STILE) {
      set_error("%s: factor %d: too large (dim %lld above 2^20, %lld planes of 2^31, a padded input of 2^30 rows or columns, "
                "or a window of %d columns above %d)", who, index, n, planes, d.kw, RD_STILE);
      return false;
    }
    p->dim = (int)n;
    p->planes = (unsigned)planes; p->H = d.H; p->W = d.W;
    p->outs = (unsigned)taps;
    p->Ho = (int)((Hp - d.kh) / d.sh + 1); p->Wo = (int)((Wp - d.kw) / d.sw + 1);
    L = (long long)p->Ho * p->Wo;
    adds = planes * ((long long)d.H * d.W * d.kw + (long long)d.H * taps);
    const long long hw = (long long)d.H * d.W, hk = (long long)d.H * d.kw;
    if (hw <= RD_TILE && hk <= RD_STILE) {
      const long long most = std::min(RD_TILE / hw, RD_STILE / hk);
      const long long least = std::min(most, cdivll(RD_MIN_RUN, hw));
      p->PP = (unsigned)std::min(most, std::max(least, planes / RD_WGS));
      p->TR = d.H; p->segw = d.W;
    } else {
      p->PP = 1;
      p->TR = (unsigned)std::max(1, std::min(d.H, std::min(RD_TILE / d.W, RD_STILE / d.kw)));
      p->segw = (unsigned)std::min(d.W, RD_TILE);
    }
  } else if (d.form == CURV_REDUCE_TOKEN) {
    if (d.N < 1 || d.T < 1 || d.E < 1 || (long long)d.N * d.T * d.E >= (1LL << 40)) {
      set_error("%s: factor %d: invalid geometry or 2^40 source elements or more (N %d T %d E %d)", who, index, d.N, d.T,
                d.E);
      return false;
    }
    if (d.E > (1 << 20) || (long long)d.N * d.T >= (1LL << 31)) {
      set_error("%s: factor %d: too large (dim %d above 2^20 or %lld token rows of 2^31)", who, index, d.E,
                (long long)d.N * d.T);
      return false;
    }
    p->dim = d.E;
    p->planes = d.N; p->H = d.T; p->W = d.E;
    p->outs = d.E;
    L = d.T;
    adds = (long long)d.N * d.T * d.E;
    const long long te = (long long)d.T * d.E;
    if (te <= RD_TILE) {
      const long long most = RD_TILE / te, least = std::min(most, cdivll(RD_MIN_RUN, te));
      p->PP = (unsigned)std::min(most, std::max(least, (long long)d.N / RD_WGS));
      p->TR = d.T; p->segw = d.E;
    } else {
      p->PP = 1;
      p->TR = (unsigned)std::max(1, std::min(d.T, RD_TILE / d.E));
      p->segw = (unsigned)std::min(d.E, RD_TILE);
    }
  } else {
    set_error("%s: factor %d: unknown form %d", who, index, d.form);
    return false;
  }
  p->inv = d.mean ? (float)(1.0 / (double)L) : 1.0f;
  p->stage_bytes = align_up((size_t)d.N * p->dim * sizeof(float), RD_ALIGN);
  // the build of the row matrix: its size limits are this build's
  const curv_factor_desc e = flat_desc(d, p->dim, reinterpret_cast<const float*>(RD_ALIGN));
  size_t need;
  long long flat;
  if (!side::plain_plan(&e, 1, &need, &flat)) {
    const std::string why = curv_last_error();
    set_error("%s: factor %d: the flat build rejected the (N %d, dim %d) row matrix: %s", who, index, d.N, p->dim,
              why.c_str());
    return false;
  }
  p->build_bytes = align_up(need, RD_ALIGN);
  p->flops = adds + flat;
  return true;
}

struct ReduceArgs {
  const void* src;
  float* dst;                 // the (N, dim) rows
  unsigned planes, H, W, outs;
  unsigned PP, TR, segw;
  int kh, kw, sh, sw, ph, pw, Ho, Wo;
  float inv;
};

// A source element type: `VEC` of them make a 16-byte load, `up` is the exact upcast.
template <int DTYPE> struct Elem;
template <> struct Elem<CURV_DTYPE_F32> {
  using T = float;
  static __device__ __forceinline__ float up(float v) { return v; }
};
template <> struct Elem<CURV_DTYPE_BF16> {
  using T = unsigned short;
  static __device__ __forceinline__ float up(unsigned short v) { return __builtin_bit_cast(float, (unsigned)v << 16); }
};
template <> struct Elem<CURV_DTYPE_F16> {
  using T = unsigned short;
  static __device__ __forceinline__ float up(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }
};

// The 16 bytes `v` as float32 values at `t` (16-byte aligned).
template <int DTYPE>
__device__ __forceinline__ void store_up(float* t, const uint4 v) {
  if constexpr (DTYPE == CURV_DTYPE_F32) {
    *reinterpret_cast<uint4*>(t) = v;
  } else {
    using E = Elem<DTYPE>;
    float4 lo, hi;
    lo.x = E::up((unsigned short)(v.x & 0xffffu)); lo.y = E::up((unsigned short)(v.x >> 16));
    lo.z = E::up((unsigned short)(v.y & 0xffffu)); lo.w = E::up((unsigned short)(v.y >> 16));
    hi.x = E::up((unsigned short)(v.z & 0xffffu)); hi.y = E::up((unsigned short)(v.z >> 16));
    hi.z = E::up((unsigned short)(v.w & 0xffffu)); hi.w = E::up((unsigned short)(v.w >> 16));
    *reinterpret_cast<float4*>(t) = lo;
    *reinterpret_cast<float4*>(t + 4) = hi;
  }
}

// The run span[0, count) as float32 in `tile`, element i at tile[shift + i]; returns shift.  16-byte loads from the first
// 16-byte boundary of the run on, single elements before it and behind the last whole vector; the shift (below one vector)
// puts the first vector on a 16-byte boundary of the tile as well.  Nothing outside the run is read.
template <int DTYPE>
__device__ __forceinline__ unsigned stage_run(float* tile, const typename Elem<DTYPE>::T* span, unsigned count,
                                              unsigned tid) {
  using E = Elem<DTYPE>;
  using T = typename E::T;
  constexpr unsigned VEC = 16 / sizeof(T), VECS = RD_TILE / VEC / RD_THREADS;
  const unsigned head = min(count, (unsigned)(((16u - (unsigned)((uintptr_t)span & 15u)) & 15u) / sizeof(T)));
  const unsigned shift = (VEC - head % VEC) % VEC;
  const unsigned vecs = (count - head) / VEC, tail = head + vecs * VEC;
  uint4 v[VECS];
#pragma unroll
  for (unsigned i = 0; i < VECS; ++i)                                  // every load in flight before the first LDS store
    if (tid + RD_THREADS * i < vecs) v[i] = *reinterpret_cast<const uint4*>(span + head + VEC * (tid + RD_THREADS * i));
  if (tid < head) tile[shift + tid] = E::up(span[tid]);
  if (tid < count - tail) tile[shift + tail + tid] = E::up(span[tail + tid]);
#pragma unroll
  for (unsigned i = 0; i < VECS; ++i) {
    const unsigned q = tid + RD_THREADS * i;
    if (q < vecs) store_up<DTYPE>(tile + shift + head + VEC * q, v[i]);
  }
  return shift;
}

// The positions o in [0, No) whose tap o s + t - p falls into [x0, x1): [lo, hi] (empty: hi < lo).  Two divisions.
__device__ __forceinline__ void tap_range(int x0, int x1, int t, int s, int p, int No, int* lo, int* hi) {
  const int c0 = x0 + p - t, c1 = x1 - 1 + p - t;
  *lo = c0 > 0 ? (c0 + s - 1) / s : 0;
  *hi = c1 < 0 ? -1 : min(No - 1, c1 / s);
}

// p[0] + p[stride] + ... (n terms) on four accumulators - terms 0 4 8 .., 1 5 9 .., 2 6 .., 3 7 .., then (0 + 1) + (2 + 3) -
// so that four LDS reads are in flight per addition step; the order is a function of n alone.
__device__ __forceinline__ float strided_sum(const float* p, int n, int stride) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = 0;
  for (; i + 4 <= n; i += 4, p += 4 * stride) {
    a0 += p[0];
    a1 += p[stride];
    a2 += p[2 * stride];
    a3 += p[3 * stride];
  }
  for (; i < n; ++i, p += stride) a0 += *p;
  return (a0 + a1) + (a2 + a3);
}

// Workgroup b owns planes [b PP, (b + 1) PP) and their row entries.  A piece - rows [h0, h0 + TR) of the plane (all rows of
// all its planes when PP > 1), columns [w0, w0 + segw) where a row is longer than the tile - is one contiguous run of
// `src`, staged as float32 in LDS.  Plane form: thread (plane, b, h) sums the row's columns of C_b into s_b[h] (over the
// column pieces in order), then thread (plane, a, b) sums s_b over the piece's rows of R_a.  Token form: thread (plane, e)
// sums column e over the piece's rows.  A plane of several pieces carries its sums from piece to piece: the first entry
// of a thread in a register, any further one (more than 256 entries per plane, or column pieces) in the row entry itself,
// which the owning thread reads back and adds to; the last piece applies 1 / L.  Items are decoded with divisions once
// per item; the element loops have none and index in 32 bits.
template <int DTYPE, int FORM>
__global__ void __launch_bounds__(RD_THREADS) reduce_rows_kernel(const ReduceArgs A) {
  using T = typename Elem<DTYPE>::T;
  __shared__ __attribute__((aligned(16))) float tile[RD_TILE + 8];
  __shared__ float sums[FORM == CURV_REDUCE_PLANE ? RD_STILE : 1];
  const unsigned tid = threadIdx.x, H = A.H, W = A.W;
  const unsigned P0 = blockIdx.x * A.PP, np = min(A.PP, A.planes - P0);
  const T* base = static_cast<const T*>(A.src) + (size_t)P0 * H * W;
  float* out = A.dst + (size_t)P0 * A.outs;
  float carry = 0.f;
  for (unsigned h0 = 0; h0 < H; h0 += A.TR) {
    const unsigned nr = min(A.TR, H - h0);
    const bool last = h0 + nr == H;
    for (unsigned w0 = 0; w0 < W; w0 += A.segw) {
      const unsigned len = min(A.segw, W - w0);
      const unsigned count = np * nr * len;                 // (np or nr above 1 only where the rows are whole) <= RD_TILE
      if (h0 | w0) __syncthreads();                         // the piece before has been summed
      const unsigned shift = stage_run<DTYPE>(tile, base + ((size_t)h0 * W + w0), count, tid);
      __syncthreads();
      const float* t = tile + shift;
      if constexpr (FORM == CURV_REDUCE_PLANE) {
        const unsigned per = (unsigned)A.kw * nr;
        for (unsigned it = tid; it < np * per; it += RD_THREADS) {
          const unsigned p = it / per, r = it - p * per, b = r / nr, hl = r - b * nr;
          int lo, hi;
          tap_range((int)w0, (int)(w0 + len), (int)b, A.sw, A.pw, A.Wo, &lo, &hi);
          const float* row = t + (p * nr + hl) * len;
          const float acc = strided_sum(row + (lo * A.sw + (int)b - A.pw - (int)w0), hi - lo + 1, A.sw);
          sums[it] = w0 ? sums[it] + acc : acc;
        }
      } else {
        for (unsigned it = tid; it < np * len; it += RD_THREADS) {
          const unsigned p = it / len, e = it - p * len;
          float acc = strided_sum(t + p * nr * len + e, (int)nr, (int)len);
          float* o = out + (size_t)p * W + w0 + e;
          const bool own = it == tid && len == W;           // (whole rows: `it` is the entry in every piece)
          if (h0) acc += own ? carry : *o;
          if (last) *o = acc * A.inv;
          else if (own) carry = acc;
          else *o = acc;
        }
      }
    }
    if constexpr (FORM == CURV_REDUCE_PLANE) {
      __syncthreads();
      const unsigned taps = A.outs;
      for (unsigned it = tid; it < np * taps; it += RD_THREADS) {
        const unsigned p = it / taps, r = it - p * taps, a = r / (unsigned)A.kw, b = r - a * (unsigned)A.kw;
        int lo, hi;
        tap_range((int)h0, (int)(h0 + nr), (int)a, A.sh, A.ph, A.Ho, &lo, &hi);
        const float* col = sums + (p * (unsigned)A.kw + b) * nr;
        float acc = strided_sum(col + (lo * A.sh + (int)a - A.ph - (int)h0), hi - lo + 1, A.sh);
        const bool own = it == tid;
        if (h0) acc += own ? carry : out[it];               // (np = 1 here: `it` is the tap)
        if (last) out[it] = acc * A.inv;
        else if (own) carry = acc;
        else out[it] = acc;
      }
    }
  }
}

template <int DTYPE>
int launch_form(hipStream_t stream, int form, unsigned blocks, const ReduceArgs& A) {
  if (form == CURV_REDUCE_PLANE)
    hipLaunchKernelGGL((reduce_rows_kernel<DTYPE, CURV_REDUCE_PLANE>), dim3(blocks), dim3(RD_THREADS), 0, stream, A);
  else
    hipLaunchKernelGGL((reduce_rows_kernel<DTYPE, CURV_REDUCE_TOKEN>), dim3(blocks), dim3(RD_THREADS), 0, stream, A);
  CURV_LAUNCH_CHECK();
  return CURV_OK;
}

int build_one(hipStream_t stream, const curv_reduce_factor_desc& d, const Plan& p, char* stage, void* build_ws) {
  float* rows = reinterpret_cast<float*>(stage);
  ReduceArgs A{};
  A.src = d.src;
  A.dst = rows;
  A.planes = p.planes; A.H = p.H; A.W = p.W; A.outs = p.outs;
  A.PP = p.PP; A.TR = p.TR; A.segw = p.segw;
  A.kh = d.kh; A.kw = d.kw; A.ph = d.ph; A.pw = d.pw; A.Ho = p.Ho; A.Wo = p.Wo;
  if (d.form == CURV_REDUCE_PLANE) {                        // (a stride beyond the padded input leaves one position: the same
    A.sh = std::min(d.sh, d.H + 2 * d.ph);                  // sums, and position x stride stays below 2^31)
    A.sw = std::min(d.sw, d.W + 2 * d.pw);
  }
  A.inv = p.inv;
  const unsigned blocks = (unsigned)cdivll(p.planes, p.PP);
  int rc;
  if (d.dtype == CURV_DTYPE_F32) rc = launch_form<CURV_DTYPE_F32>(stream, d.form, blocks, A);
  else if (d.dtype == CURV_DTYPE_BF16) rc = launch_form<CURV_DTYPE_BF16>(stream, d.form, blocks, A);
  else rc = launch_form<CURV_DTYPE_F16>(stream, d.form, blocks, A);
  if (rc != CURV_OK) return rc;
  const curv_factor_desc e = flat_desc(d, p.dim, rows);
  return curv_kfac_accumulate(stream, &e, 1, build_ws, p.build_bytes);
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac_reduce_workspace_bytes(const curv_reduce_factor_desc* descs, int n_factors) {
  // the sum over the factors (every factor has scratch of its own); never 0 for valid descriptors: 0 reports an error
  return side::workspace_bytes("curv_kfac_reduce_workspace_bytes", descs, n_factors, plan_of, side::staged_bytes<Plan>);
}

extern "C" int curv_kfac_reduce_plan_flops(const curv_reduce_factor_desc* descs, int n_factors, long long* out) {
  return side::plan_flops("curv_kfac_reduce_plan_flops", descs, n_factors, out, plan_of);
}

extern "C" int curv_kfac_reduce_accumulate(void* stream_, const curv_reduce_factor_desc* descs, int n_factors,
                                           void* workspace, size_t workspace_bytes) {
  return side::staged_accumulate("curv_kfac_reduce_accumulate", (hipStream_t)stream_, descs, n_factors, workspace,
                                 workspace_bytes, RD_ALIGN, plan_of, build_one);
}
