// Curvature of an nn.Embedding weight (include/curv_hip.h "Curvature of an nn.Embedding weight"): the token
// histogram that is the layer's diagonal A factor, and the two per-sample reductions, which are one segment walker over a
// position list grouped by the caller.  Bandwidth kernels: plain fp32 VALU arithmetic, int32 atomics for the counts only,
// no floating-point atomics.  Every index read from `idx`, `pos`, `chunks` and `mgroups` is checked before it is used.
#include "common.h"
#include "wave_sum.h"

#include <cmath>
#include <vector>

namespace curv {
namespace {

constexpr int EMB_WAVE = 64;
constexpr int EMB_THREADS = 256;
constexpr int EMB_SLICE = 256;          // contiguous floats of a row one wave owns: 4 per lane
constexpr int EMB_MAX_WAVES = 16;       // waves of a walker workgroup; a wave takes every EMB_MAX_WAVES-th slice beyond
constexpr int EMB_UNROLL = 4;           // rows a wave has in flight
constexpr size_t EMB_ALIGN = 256;

__device__ __forceinline__ long long emb_index(const void* idx, int i64, long long p) {
  return i64 ? ((const long long*)idx)[p] : (long long)((const int*)idx)[p];
}

// ------------------------------------------------------------------------------------------------ histogram
__global__ void emb_zero_kernel(int* counts, int V) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V) counts[v] = 0;
}

// One int32 atomic per distinct token of a wave: the lanes that hold the token of the lowest live lane are counted by
// ballot, that lane adds the count, and they retire.  A position past the end, a padding token or one outside [0, V)
// never goes live.
__global__ void emb_count_kernel(const void* idx, int i64, long long positions, int V, int padding_idx, int* counts) {
  const int lane = threadIdx.x & (EMB_WAVE - 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  // (the loop bound is the wave's first position: all 64 lanes run the same number of rounds and meet in the ballots)
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < positions; base += stride) {
    const long long p = base + lane;
    long long tok = -1;
    if (p < positions) tok = emb_index(idx, i64, p);
    bool live = tok >= 0 && tok < V && tok != padding_idx;
    const int key = live ? (int)tok : -1;
    unsigned long long open = __ballot(live);
    while (open) {
      const int leader = __ffsll((long long)open) - 1;
      const int lead_key = __shfl(key, leader, EMB_WAVE);
      const bool same = live && key == lead_key;
      const unsigned long long mask = __ballot(same);
      if (lane == leader) atomicAdd(&counts[lead_key], __popcll(mask));
      live = live && !same;
      open = __ballot(live);
    }
  }
}

__global__ void emb_finish_kernel(const int* counts, float* a, int V, int padding_idx, float scale, int first) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const float add = v == padding_idx ? 0.f : scale * (float)counts[v];
  a[v] = first ? add : a[v] + add;
}

bool emb_hist_ok(const curv_embedding_desc& d, int i, const char* name) {
  if (d.V < 1 || d.positions < 1 || d.positions >= (1LL << 31)) {
    set_error("%s: item %d: invalid sizes (V %d, positions %lld)", name, i, d.V, d.positions);
    return false;
  }
  if (d.padding_idx < -1 || d.padding_idx >= d.V || d.reserved != 0) {
    set_error("%s: item %d: padding_idx %d outside [-1, V) or nonzero reserved field", name, i, d.padding_idx);
    return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------ the segment walker
struct WalkArgs {
  const void* idx;
  const float* g;
  const float* w;
  const int* pos;
  const int* chunks;
  const int* mgroups;
  float* dst;
  float* out;
  float* slots;        // (n_slots, 3, Dp): head, accumulator, tail of every chunk of a split group
  int* slot_info;      // (n_slots, 4): continues the previous chunk's last segment, has a boundary, head key, tail key
  long long positions, g_sn, g_st, w_rs, dst_rs, o_stride;
  int n_pos, n_chunks, n_mgroups, n_slots;
  int N, T, V, D, Dp, i64, padding_idx, w_kind, vec, wvec;
  float alpha;
};

__device__ __forceinline__ f32x4 emb_load4(const float* row, int d0, int D, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec && d0 + 4 <= D) return *reinterpret_cast<const f32x4*>(row + d0);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (d0 + j < D) v[j] = row[d0 + j];
  return v;
}

// w of inner key `key` at the lane's four columns (quad mode); 1 where the job has no w; 0 for a key that names no row.
template <int MODE>
__device__ __forceinline__ f32x4 emb_weight(const WalkArgs& a, long long key, int d0) {
  f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
  if (MODE == CURV_EMB_SQ || a.w_kind == 0) return one;
  if (key < 0 || key >= a.V) return zero;
  if (a.w_kind == CURV_EMB_W_VECTOR) {
    const float s = a.w[key];
    f32x4 v = {s, s, s, s};
    return v;
  }
  return emb_load4(a.w + key * a.w_rs, d0, a.D, a.wvec != 0);
}

// (outer, inner) key of position p, false where p or its token names nothing.
template <int MODE>
__device__ __forceinline__ bool emb_keys(const WalkArgs& a, long long p, long long* outer, long long* inner, long long* n_of) {
  if (p < 0 || p >= a.positions) return false;
  const long long tok = emb_index(a.idx, a.i64, p);
  if (tok < 0 || tok >= a.V || tok == a.padding_idx) return false;
  const long long n = p / a.T;
  if (n >= a.N) return false;
  *n_of = n;
  *outer = MODE == CURV_EMB_SQ ? tok : n;
  *inner = MODE == CURV_EMB_SQ ? n : tok;
  return true;
}

// The group's value of the lane's four columns goes out: sq adds it to its row of dst, quad hands back the lane's sum.
template <int MODE>
__device__ __forceinline__ float emb_emit(const WalkArgs& a, int group, int d0, f32x4 acc) {
  if (MODE == CURV_EMB_SQ) {
    float* row = a.dst + (long long)group * a.dst_rs;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (d0 + j < a.D) row[d0 + j] += a.alpha * acc[j];
    return 0.f;
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);      // (columns at and past D hold zeros)
}

// The waves' sums of a quad group, added in wave order, into out[group].
__device__ __forceinline__ void emb_quad_store(const WalkArgs& a, int group, float part, float* s_part) {
  const int wave = threadIdx.x / EMB_WAVE, lane = threadIdx.x & (EMB_WAVE - 1), waves = blockDim.x / EMB_WAVE;
  part = wave_sum_dpp(part);
  if (lane == EMB_WAVE - 1) s_part[wave] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.f;
    for (int k = 0; k < waves; ++k) total += s_part[k];
    a.out[(long long)group * a.o_stride] += a.alpha * total;
  }
}

template <int MODE>
__global__ void emb_walk_kernel(WalkArgs a) {
  __shared__ float s_part[EMB_MAX_WAVES];
  const int wave = threadIdx.x / EMB_WAVE, lane = threadIdx.x & (EMB_WAVE - 1), waves = blockDim.x / EMB_WAVE;
  const int* c = a.chunks + 4LL * blockIdx.x;
  const int begin = c[0], end = c[1], group = c[2], slot = c[3];
  // (all four are the same for the whole workgroup: it leaves as one)
  if (begin < 0 || end > a.n_pos || begin >= end || group < 0 || group >= (MODE == CURV_EMB_SQ ? a.V : a.N) ||
      slot >= a.n_slots)
    return;
  const bool direct = slot < 0;
  int continues = 0;
  if (!direct && begin > 0) {
    long long o0, i0, o1, i1, n0;
    if (emb_keys<MODE>(a, a.pos[begin - 1], &o0, &i0, &n0) && emb_keys<MODE>(a, a.pos[begin], &o1, &i1, &n0))
      continues = o0 == group && o1 == group && i0 == i1;
  }
  float part = 0.f;
  for (int slice = wave; slice * EMB_SLICE < a.D; slice += waves) {
    const int d0 = slice * EMB_SLICE + lane * 4;
    f32x4 r = {0.f, 0.f, 0.f, 0.f}, acc = r, head = r;
    bool seen = false, have = false;
    long long prev = -1, head_key = -1;
    for (int i = begin; i < end; i += EMB_UNROLL) {
      f32x4 row[EMB_UNROLL];
      long long key[EMB_UNROLL];
      bool ok[EMB_UNROLL];
#pragma unroll
      for (int u = 0; u < EMB_UNROLL; ++u) {
        ok[u] = false;
        key[u] = -1;
        row[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i + u < end) {
          const long long p = a.pos[i + u];
          long long outer, n;
          if (emb_keys<MODE>(a, p, &outer, &key[u], &n) && outer == group) {
            ok[u] = true;
            row[u] = emb_load4(a.g + n * a.g_sn + (p - n * a.T) * a.g_st, d0, a.D, a.vec != 0);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < EMB_UNROLL; ++u) {
        if (!ok[u]) continue;
        if (have && key[u] != prev) {                  // the segment of `prev` is complete
          if (direct || seen) {
            acc += emb_weight<MODE>(a, prev, d0) * r * r;
          } else {
            head = r;
            head_key = prev;
            seen = true;
          }
          r = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        prev = key[u];
        have = true;
        r += row[u];
      }
    }
    if (direct) {
      if (have) acc += emb_weight<MODE>(a, prev, d0) * r * r;
      part += emb_emit<MODE>(a, group, d0, acc);
      continue;
    }
    // a chunk of a split group: what it knows of its first segment, its whole segments and its last one
    f32x4 tail = {0.f, 0.f, 0.f, 0.f};
    if (!seen) {
      head = r;
      head_key = prev;
    } else {
      tail = r;
    }
    float* base = a.slots + 3LL * slot * a.Dp;
    if (d0 < a.Dp) {
      *reinterpret_cast<f32x4*>(base + d0) = head;
      *reinterpret_cast<f32x4*>(base + a.Dp + d0) = acc;
      *reinterpret_cast<f32x4*>(base + 2LL * a.Dp + d0) = tail;
    }
    if (slice == 0 && lane == 0) {
      int* info = a.slot_info + 4LL * slot;
      info[0] = continues;
      info[1] = seen ? 1 : 0;
      info[2] = (int)head_key;
      info[3] = (int)prev;
    }
  }
  if (MODE == CURV_EMB_QUAD && direct) emb_quad_store(a, group, part, s_part);
}

// The chunks of one split group, in chunk order.
template <int MODE>
__global__ void emb_combine_kernel(WalkArgs a) {
  __shared__ float s_part[EMB_MAX_WAVES];
  const int wave = threadIdx.x / EMB_WAVE, lane = threadIdx.x & (EMB_WAVE - 1), waves = blockDim.x / EMB_WAVE;
  const int* m = a.mgroups + 3LL * blockIdx.x;
  const int s_begin = m[0], s_end = m[1], group = m[2];
  if (s_begin < 0 || s_end > a.n_slots || s_begin >= s_end || group < 0 || group >= (MODE == CURV_EMB_SQ ? a.V : a.N))
    return;
  float part = 0.f;
  for (int slice = wave; slice * EMB_SLICE < a.D; slice += waves) {
    const int d0 = slice * EMB_SLICE + lane * 4;
    f32x4 r = {0.f, 0.f, 0.f, 0.f}, acc = r;
    long long rkey = -1;
    if (d0 < a.Dp) {
      for (int s = s_begin; s < s_end; ++s) {
        const int* info = a.slot_info + 4LL * s;
        const float* base = a.slots + 3LL * s * a.Dp;
        if (!info[0]) {                                // the chunk opens a segment: the one carried so far is complete
          acc += emb_weight<MODE>(a, rkey, d0) * r * r;
          r = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        r += *reinterpret_cast<const f32x4*>(base + d0);
        if (info[2] >= 0) rkey = info[2];
        if (info[1]) {
          acc += emb_weight<MODE>(a, rkey, d0) * r * r;
          acc += *reinterpret_cast<const f32x4*>(base + a.Dp + d0);
          r = *reinterpret_cast<const f32x4*>(base + 2LL * a.Dp + d0);
          rkey = info[3];
        }
      }
      acc += emb_weight<MODE>(a, rkey, d0) * r * r;
    }
    part += emb_emit<MODE>(a, group, d0, acc);
  }
  if (MODE == CURV_EMB_QUAD) emb_quad_store(a, group, part, s_part);
}

// first: rows x cols zeros through a row stride (sq: dst, quad: out as rows of one).
__global__ void emb_fill_kernel(float* p, long long rows, int cols, long long row_stride) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  p[(i / cols) * row_stride + (i % cols)] = 0.f;
}

struct WalkPlan {
  int Dp, waves, vec, wvec;
  size_t slot_bytes, info_bytes;
};

bool emb_walk_plan(const curv_embedding_walk_desc& d, int i, const char* name, int mode, WalkPlan* P) {
  if (d.N < 1 || d.T < 1 || d.V < 1 || d.D < 1 || d.positions != (long long)d.N * d.T || d.positions >= (1LL << 31)) {
    set_error("%s: item %d: invalid sizes (N %d T %d V %d D %d positions %lld)", name, i, d.N, d.T, d.V, d.D, d.positions);
    return false;
  }
  if (d.mode != mode || d.reserved != 0 || d.reserved2 != 0 || d.padding_idx < -1 || d.padding_idx >= d.V) {
    set_error("%s: item %d: mode %d (expected %d), padding_idx %d outside [-1, V) or a nonzero reserved field", name, i, d.mode,
              mode, d.padding_idx);
    return false;
  }
  if (d.g_sn < 0 || d.g_st < 0 || (long long)(d.N - 1) * d.g_sn + (long long)(d.T - 1) * d.g_st + d.D > d.g_elems) {
    set_error("%s: item %d: strides (%lld, %lld) and sizes address more than the extent of %lld elements", name, i, d.g_sn,
              d.g_st, d.g_elems);
    return false;
  }
  if (d.n_pos < 0 || d.n_pos > d.positions || d.n_chunks < 0 || d.n_mgroups < 0 || d.n_slots < 0 || d.n_slots > d.n_chunks ||
      d.n_mgroups > d.n_slots) {
    set_error("%s: item %d: invalid list sizes (n_pos %d n_chunks %d n_mgroups %d n_slots %d)", name, i, d.n_pos, d.n_chunks,
              d.n_mgroups, d.n_slots);
    return false;
  }
  if (mode == CURV_EMB_SQ) {
    if (d.dst_rs < d.D && d.V > 1) {
      set_error("%s: item %d: dst_rs %lld below D = %d", name, i, d.dst_rs, d.D);
      return false;
    }
  } else {
    if (d.w_kind != 0 && d.w_kind != CURV_EMB_W_MATRIX && d.w_kind != CURV_EMB_W_VECTOR) {
      set_error("%s: item %d: unknown w_kind %d", name, i, d.w_kind);
      return false;
    }
    if ((d.w_kind == CURV_EMB_W_MATRIX && d.w_rs < d.D && d.V > 1) || (d.o_stride < 1 && d.N > 1)) {
      set_error("%s: item %d: w_rs %lld below D = %d or o_stride %lld below 1", name, i, d.w_rs, d.D, d.o_stride);
      return false;
    }
  }
  if (!std::isfinite(d.alpha)) {
    set_error("%s: item %d: alpha %g is not finite", name, i, (double)d.alpha);
    return false;
  }
  P->Dp = (d.D + 3) / 4 * 4;
  P->waves = std::min(cdiv(d.D, EMB_SLICE), EMB_MAX_WAVES);
  P->vec = (reinterpret_cast<uintptr_t>(d.g) & 15) == 0 && d.g_sn % 4 == 0 && d.g_st % 4 == 0;
  P->wvec = d.w_kind == CURV_EMB_W_MATRIX && (reinterpret_cast<uintptr_t>(d.w) & 15) == 0 && d.w_rs % 4 == 0;
  P->slot_bytes = align_up((size_t)d.n_slots * 3 * P->Dp * sizeof(float), EMB_ALIGN);
  P->info_bytes = align_up((size_t)d.n_slots * 4 * sizeof(int), EMB_ALIGN);
  return true;
}

size_t emb_walk_bytes(const char* name, const curv_embedding_walk_desc* descs, int n) {
  if (n <= 0 || !descs) {
    set_error("%s: no descriptors", name);
    return 0;
  }
  size_t total = EMB_ALIGN;                            // (never 0 for valid descriptors)
  for (int i = 0; i < n; ++i) {
    WalkPlan P;
    if (descs[i].mode != CURV_EMB_SQ && descs[i].mode != CURV_EMB_QUAD) {
      set_error("%s: item %d: unknown mode %d", name, i, descs[i].mode);
      return 0;
    }
    if (!emb_walk_plan(descs[i], i, name, descs[i].mode, &P)) return 0;
    total += P.slot_bytes + P.info_bytes;
  }
  return total;
}

template <int MODE>
int emb_walk_run(const char* name, hipStream_t stream, const curv_embedding_walk_desc* descs, int n, void* workspace,
                 size_t bytes) {
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs, "%s: null descriptors", name);
  std::vector<WalkPlan> plans(n);
  size_t need = EMB_ALIGN;
  for (int i = 0; i < n; ++i) {
    if (!emb_walk_plan(descs[i], i, name, MODE, &plans[i])) return CURV_ERR_INVALID;
    need += plans[i].slot_bytes + plans[i].info_bytes;
    const curv_embedding_walk_desc& d = descs[i];
    CURV_REQUIRE(d.idx && d.g, "%s: item %d: null record", name, i);
    CURV_REQUIRE(d.n_chunks == 0 || (d.pos && d.chunks), "%s: item %d: null position list", name, i);
    CURV_REQUIRE(d.n_mgroups == 0 || d.mgroups, "%s: item %d: null list of split groups", name, i);
    if (MODE == CURV_EMB_SQ) {
      CURV_REQUIRE(d.dst, "%s: item %d: null destination", name, i);
    } else {
      CURV_REQUIRE(d.out, "%s: item %d: null destination", name, i);
      CURV_REQUIRE(d.w_kind == 0 || d.w, "%s: item %d: null w", name, i);
    }
  }
  if (!workspace || bytes < need || (reinterpret_cast<uintptr_t>(workspace) & (EMB_ALIGN - 1))) {
    set_error("%s: workspace too small (%zu < %zu bytes) or not %zu-byte aligned", name, bytes, need, EMB_ALIGN);
    return CURV_ERR_WORKSPACE;
  }
  char* at = (char*)workspace;
  for (int i = 0; i < n; ++i) {
    const curv_embedding_walk_desc& d = descs[i];
    const WalkPlan& P = plans[i];
    WalkArgs a;
    memset(&a, 0, sizeof(a));
    a.idx = d.idx; a.g = d.g; a.w = d.w; a.pos = d.pos; a.chunks = d.chunks; a.mgroups = d.mgroups;
    a.dst = d.dst; a.out = d.out;
    a.slots = (float*)at; at += P.slot_bytes;
    a.slot_info = (int*)at; at += P.info_bytes;
    a.positions = d.positions; a.g_sn = d.g_sn; a.g_st = d.g_st; a.w_rs = d.w_rs; a.dst_rs = d.dst_rs; a.o_stride = d.o_stride;
    a.n_pos = d.n_pos; a.n_chunks = d.n_chunks; a.n_mgroups = d.n_mgroups; a.n_slots = d.n_slots;
    a.N = d.N; a.T = d.T; a.V = d.V; a.D = d.D; a.Dp = P.Dp; a.i64 = d.idx_i64 ? 1 : 0; a.padding_idx = d.padding_idx;
    a.w_kind = d.w_kind; a.vec = P.vec; a.wvec = P.wvec; a.alpha = d.alpha;
    if (d.first) {                                     // a group that never occurs is written here only
      const long long rows = MODE == CURV_EMB_SQ ? d.V : d.N, stride = MODE == CURV_EMB_SQ ? d.dst_rs : d.o_stride;
      const int cols = MODE == CURV_EMB_SQ ? d.D : 1;
      hipLaunchKernelGGL(emb_fill_kernel, dim3((unsigned)cdivll(rows * cols, EMB_THREADS)), dim3(EMB_THREADS), 0, stream,
                         MODE == CURV_EMB_SQ ? d.dst : d.out, rows, cols, stride);
      CURV_LAUNCH_CHECK();
    }
    if (d.n_chunks > 0) {
      hipLaunchKernelGGL(emb_walk_kernel<MODE>, dim3(d.n_chunks), dim3(P.waves * EMB_WAVE), 0, stream, a);
      CURV_LAUNCH_CHECK();
    }
    if (d.n_mgroups > 0) {
      hipLaunchKernelGGL(emb_combine_kernel<MODE>, dim3(d.n_mgroups), dim3(P.waves * EMB_WAVE), 0, stream, a);
      CURV_LAUNCH_CHECK();
    }
  }
  return CURV_OK;
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac_embedding_workspace_bytes(const curv_embedding_desc* descs, int n) {
  const char* const name = "curv_kfac_embedding_workspace_bytes";
  if (n <= 0 || !descs) {
    set_error("%s: no descriptors", name);
    return 0;
  }
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (!emb_hist_ok(descs[i], i, name)) return 0;
    total += align_up((size_t)descs[i].V * sizeof(int), EMB_ALIGN);
  }
  return total;
}

extern "C" size_t curv_persample_embedding_workspace_bytes(const curv_embedding_walk_desc* descs, int n) {
  return emb_walk_bytes("curv_persample_embedding_workspace_bytes", descs, n);
}

extern "C" int curv_kfac_embedding_plan_flops(const curv_embedding_desc* descs, int n, long long* out) {
  const char* const name = "curv_kfac_embedding_plan_flops";
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs && out, "%s: null argument", name);
  for (int i = 0; i < n; ++i) {
    if (!emb_hist_ok(descs[i], i, name)) return CURV_ERR_INVALID;
    out[i] = descs[i].positions + descs[i].V;
  }
  return CURV_OK;
}

extern "C" int curv_kfac_embedding_accumulate(void* stream_, const curv_embedding_desc* descs, int n, void* workspace,
                                              size_t workspace_bytes) {
  const char* const name = "curv_kfac_embedding_accumulate";
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  CURV_REQUIRE(descs, "%s: null descriptors", name);
  size_t need = 0;
  for (int i = 0; i < n; ++i) {
    if (!emb_hist_ok(descs[i], i, name)) return CURV_ERR_INVALID;
    CURV_REQUIRE(descs[i].idx && descs[i].a, "%s: item %d: null idx or a", name, i);
    CURV_REQUIRE(std::isfinite(descs[i].scale), "%s: item %d: scale %g is not finite", name, i, (double)descs[i].scale);
    need += align_up((size_t)descs[i].V * sizeof(int), EMB_ALIGN);
  }
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & (EMB_ALIGN - 1))) {
    set_error("%s: workspace too small (%zu < %zu bytes) or not %zu-byte aligned", name, workspace_bytes, need, EMB_ALIGN);
    return CURV_ERR_WORKSPACE;
  }
  char* at = (char*)workspace;
  for (int i = 0; i < n; ++i) {
    const curv_embedding_desc& d = descs[i];
    int* counts = (int*)at;
    at += align_up((size_t)d.V * sizeof(int), EMB_ALIGN);
    const unsigned v_blocks = (unsigned)cdiv(d.V, EMB_THREADS);
    const unsigned p_blocks = (unsigned)std::min<long long>(cdivll(d.positions, EMB_THREADS), 2048);
    hipLaunchKernelGGL(emb_zero_kernel, dim3(v_blocks), dim3(EMB_THREADS), 0, stream, counts, d.V);
    CURV_LAUNCH_CHECK();
    hipLaunchKernelGGL(emb_count_kernel, dim3(p_blocks), dim3(EMB_THREADS), 0, stream, d.idx, d.idx_i64 ? 1 : 0, d.positions,
                       d.V, d.padding_idx, counts);
    CURV_LAUNCH_CHECK();
    hipLaunchKernelGGL(emb_finish_kernel, dim3(v_blocks), dim3(EMB_THREADS), 0, stream, (const int*)counts, d.a, d.V,
                       d.padding_idx, d.scale, d.first ? 1 : 0);
    CURV_LAUNCH_CHECK();
  }
  return CURV_OK;
}

extern "C" int curv_persample_embedding_sq_accumulate(void* stream, const curv_embedding_walk_desc* descs, int n,
                                                      void* workspace, size_t workspace_bytes) {
  return emb_walk_run<CURV_EMB_SQ>("curv_persample_embedding_sq_accumulate", (hipStream_t)stream, descs, n, workspace,
                                   workspace_bytes);
}

extern "C" int curv_persample_embedding_quad_reduce(void* stream, const curv_embedding_walk_desc* descs, int n,
                                                    void* workspace, size_t workspace_bytes) {
  return emb_walk_run<CURV_EMB_QUAD>("curv_persample_embedding_quad_reduce", (hipStream_t)stream, descs, n, workspace,
                                     workspace_bytes);
}
