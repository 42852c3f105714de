// KFAC factor build of grouped convolutions (curv_kfac_group_accumulate, include/curv_hip.h): one Kronecker pair per
// group, dst[g] (+)= scale * X_g X_g^T with X_g the implicit im2col of input-channel slice [g cg, (g + 1) cg) of `src`
// (rows (c, kh, kw), columns (n, oh, ow)) plus the row of ones when `has_bias`.
//
// Two regimes, chosen per factor by the patch size P = cg kh kw:
//   narrow (P <= GRP_NARROW_MAX: depthwise 3x3 / 5x5 rows up to 16, the G side of depthwise and ResNeXt-4/8/16 layers):
//     1. Gram pass.  A workgroup takes one group and one slice of GRP_SLICE output pixels; its 256 lanes walk the slice
//        pixel by pixel (adjacent lanes = adjacent pixels, so the gathers of a wave are contiguous at stride 1), gather
//        their patch values straight from `src` (padding reads as 0 through a select; the address of a masked gather is
//        `src` itself, so nothing outside `src` is read) and accumulate the whole lower triangle and the patch sums in
//        registers with fp32 fma (P templated).  The 256 partials are summed by a fixed butterfly inside each wave and
//        the four waves in order; the slice's sums go to scratch.
//     2. Reduce pass.  One thread per lower-triangle entry of each group sums the slices in order, builds the bias row
//        (patch sums) and corner (the pixel count), scales, writes or adds dst[g] and mirrors the upper triangle.
//   wide (P > GRP_NARROW_MAX: ResNeXt / RegNet groups): a group-major copy of the source, (G, N, cg, H, W) with every
//     group's slot 256-byte aligned, feeds the MFMA factor build of ordinary layers (curv_kfac_accumulate, one
//     descriptor per group), one call per factor: that call's launch plan (slicing, tiling, small or grouped form)
//     depends on this factor's geometry alone.  One pass over the tensor buys the existing kernels' fp32 MFMA rate.
// Every launch goes on the caller's stream and nothing waits on the host, so the call can be captured into a graph.
// Narrow factor tables travel as kernel arguments (batches of GRP_BATCH factors): no descriptor upload.
#include "side_build.h"

namespace curv {
namespace {

constexpr int GRP_THREADS = 256;
constexpr int GRP_PIXELS_PER_LANE = 64;
constexpr int GRP_SLICE = GRP_THREADS * GRP_PIXELS_PER_LANE;   // output pixels per Gram workgroup
constexpr int GRP_NARROW_MAX = 16;
constexpr int GRP_BATCH = 8;
constexpr size_t GRP_SLOT_ALIGN = 256;                          // group slots of the wide regime's group-major copy

struct GrpFactor {
  const float* src;
  float* dst;
  float* part;                // this factor's slice partials in the workspace
  int N, C, H, W, G, cg, kh, kw, sh, sw, ph, pw, Ho, Wo;
  int P, n, has_bias, first;
  float scale;
  int K;                      // output pixels N Ho Wo
  int S;                      // slices
  int E;                      // partials per (group, slice)
  int base;                   // first workgroup of this factor in the launch
  int step_n, step_oh, step_ow;   // GRP_THREADS pixels = step_n Ho Wo + step_oh Wo + step_ow
};

typedef ArgBatch<GrpFactor, GRP_BATCH> GrpBatch;

struct Plan {
  int P, n, Ho, Wo, K, S, E;
  bool narrow;
  size_t part_bytes;          // narrow: slice partials
  size_t slot_floats;         // wide: floats per group slot of the group-major copy
  size_t copy_bytes;          // wide: the copy
  size_t build_bytes;         // wide: scratch of the curv_kfac_accumulate call
  long long flops;            // executed multiply-adds x 2
};

// Wide regime: one ordinary factor descriptor per group, reading group g's slot of the group-major copy at `copy`.
void wide_descs(const curv_group_factor_desc& d, const Plan& p, const float* copy, std::vector<curv_factor_desc>* out) {
  out->assign(d.groups, curv_factor_desc{});
  for (int g = 0; g < d.groups; ++g) {
    curv_factor_desc& s = (*out)[g];
    s.src = copy + (size_t)g * p.slot_floats;
    s.dst = d.dst ? d.dst + (size_t)g * p.n * p.n : nullptr;
    s.N = d.N; s.C = d.C / d.groups; s.H = d.H; s.W = d.W;
    s.kh = d.kh; s.kw = d.kw; s.sh = d.sh; s.sw = d.sw; s.ph = d.ph; s.pw = d.pw;
    s.has_bias = d.has_bias; s.first = d.first; s.scale = d.scale;
    s.path_hint = CURV_PATH_AUTO;          // decided on this factor's own geometry: the call holds nothing else
  }
}

bool plan_of(const curv_group_factor_desc& d, int index, Plan* p) {
  side::ConvGeom g;
  if (!side::conv_geom_of(d, "curv_kfac_group", "factor", index, &g)) return false;
  if (d.groups < 1 || d.C % d.groups != 0) {
    set_error("curv_kfac_group: factor %d: C %d must be a multiple of groups %d", index, d.C, d.groups);
    return false;
  }
  p->Ho = g.Ho;
  p->Wo = g.Wo;
  long long K = (long long)d.N * p->Ho * p->Wo;
  long long P = (long long)(d.C / d.groups) * d.kh * d.kw;
  if (K >= (1LL << 30) || P > 8192) {
    set_error("curv_kfac_group: factor %d: too large (%lld output pixels, %lld patch rows)", index, K, P);
    return false;
  }
  p->K = (int)K;
  p->P = (int)P;
  p->n = p->P + (d.has_bias ? 1 : 0);
  p->S = (int)cdivll(K, GRP_SLICE);
  p->narrow = p->P <= GRP_NARROW_MAX;
  p->E = p->P * (p->P + 1) / 2 + p->P;
  p->part_bytes = p->copy_bytes = p->build_bytes = p->slot_floats = 0;
  if (p->narrow) {
    p->flops = 2LL * p->E * K * d.groups;
    p->part_bytes = align_up((size_t)d.groups * p->S * p->E * sizeof(float), 256);
    return true;
  }
  const size_t cg = (size_t)(d.C / d.groups);
  p->slot_floats = align_up(cg * d.N * d.H * d.W * sizeof(float), GRP_SLOT_ALIGN) / sizeof(float);
  p->copy_bytes = p->slot_floats * sizeof(float) * d.groups;
  // the per-group descriptors on a stand-in copy (the plan reads only the geometry and the 16-byte alignment of the
  // sources, which every 256-byte aligned slot has)
  std::vector<curv_factor_desc> sub;
  wide_descs(d, *p, reinterpret_cast<const float*>(GRP_SLOT_ALIGN), &sub);
  if (!side::plain_plan(sub.data(), d.groups, &p->build_bytes, &p->flops)) {
    set_error("curv_kfac_group: factor %d: the per-group build rejected the geometry", index);
    return false;
  }
  return true;
}

__device__ inline float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// Sums `acc` over the workgroup (butterfly in each wave, then the four waves in order) into out[0 .. E).
template <int E>
__device__ inline void block_sum_store(const float (&acc)[E], float* out, float (*red)[E]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    float x = wave_sum(acc[e]);
    if (lane == 0) red[wave][e] = x;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += GRP_THREADS) out[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// Walks the pixels of slice `s` owned by this lane: calls body(n, ih0, iw0) with the top-left input coordinate of each
// patch.
template <typename Body>
__device__ inline void for_pixels(const GrpFactor& F, int s, Body body) {
  const int k0 = s * GRP_SLICE;
  const int k1 = min(F.K, k0 + GRP_SLICE);
  int k = k0 + (int)threadIdx.x;
  if (k >= k1) return;
  const int HoWo = F.Ho * F.Wo;
  int n = k / HoWo, rem = k - n * HoWo;
  int oh = rem / F.Wo, ow = rem - oh * F.Wo;
  for (; k < k1; k += GRP_THREADS) {
    body(n, oh * F.sh - F.ph, ow * F.sw - F.pw);
    ow += F.step_ow;
    oh += F.step_oh;
    n += F.step_n;
    if (ow >= F.Wo) { ow -= F.Wo; ++oh; }
    if (oh >= F.Ho) { oh -= F.Ho; ++n; }
  }
}

// Row r of the patch of group g: input-plane offset of its (c, a, b) relative to the patch origin, and (a, b).
// Rows past the patch get a = -2^20: every bounds test of such a row fails, so its value is 0 in both operands.
__device__ inline void patch_row(const GrpFactor& F, int g, int r, long long* off, int* a, int* b) {
  if (r < F.P) {
    const int khw = F.kh * F.kw;
    const int c = r / khw, q = r - c * khw;
    *a = q / F.kw;
    *b = q - *a * F.kw;
    *off = (long long)(g * F.cg + c) * F.H * F.W + (long long)*a * F.W + *b;
  } else {
    *a = -(1 << 20);
    *b = 0;
    *off = 0;
  }
}

__device__ inline float gather(const GrpFactor& F, const float* base_n, int ih0, int iw0, long long off, int a, int b) {
  const bool ok = (unsigned)(ih0 + a) < (unsigned)F.H && (unsigned)(iw0 + b) < (unsigned)F.W;
  const long long idx = ok ? off + (long long)ih0 * F.W + iw0 : 0;
  const float v = (ok ? base_n : F.src)[idx];
  return ok ? v : 0.f;
}

template <int P>
__global__ void __launch_bounds__(GRP_THREADS) group_gram_narrow_kernel(const GrpBatch batch) {
  constexpr int T = P * (P + 1) / 2;
  constexpr int E = T + P;
  __shared__ float red[4][E];
  const int fi = owner_of(batch, (int)blockIdx.x);
  const GrpFactor& F = batch.e[fi];
  const int b = blockIdx.x - F.base;
  const int g = b / F.S, s = b - g * F.S;
  long long off[P];
  int ra[P], rb[P];
#pragma unroll
  for (int r = 0; r < P; ++r) patch_row(F, g, r, &off[r], &ra[r], &rb[r]);
  float acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;
  const long long plane = (long long)F.C * F.H * F.W;
  for_pixels(F, s, [&](int n, int ih0, int iw0) {
    const float* base_n = F.src + n * plane;
    float v[P];
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = gather(F, base_n, ih0, iw0, off[r], ra[r], rb[r]);
#pragma unroll
    for (int i = 0; i < P; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) acc[i * (i + 1) / 2 + j] = fmaf(v[i], v[j], acc[i * (i + 1) / 2 + j]);
      acc[T + i] += v[i];
    }
  });
  block_sum_store<E>(acc, F.part + ((long long)g * F.S + s) * E, red);
}

// Wide regime: src (N, C, H, W) -> dst (G, N, cg, H, W), group slots `slot` floats apart.  One workgroup per
// (sample, channel) plane.
__global__ void __launch_bounds__(GRP_THREADS) group_major_copy_kernel(const float* __restrict__ src,
                                                                       float* __restrict__ dst, int N, int C, int cg,
                                                                       int HW, long long slot) {
  const int plane = blockIdx.x;
  const int n = plane / C, ch = plane - n * C;
  const int g = ch / cg, c = ch - g * cg;
  const float* in = src + (long long)plane * HW;
  float* out = dst + g * slot + ((long long)n * cg + c) * HW;
  for (int p = threadIdx.x; p < HW; p += GRP_THREADS) out[p] = in[p];
}

// One thread per (group, entry of the n x n square); entries above the diagonal idle.  Workgroups of a factor:
// G x ceil(n^2 / GRP_THREADS).
__global__ void __launch_bounds__(GRP_THREADS) group_reduce_kernel(const GrpBatch batch) {
  const int fi = owner_of(batch, (int)blockIdx.x);
  const GrpFactor& F = batch.e[fi];
  const int n = F.n, P = F.P, S = F.S;
  const int chunks = (n * n + GRP_THREADS - 1) / GRP_THREADS;
  const int b = blockIdx.x - F.base;
  const int g = b / chunks;
  const int idx = (b - g * chunks) * GRP_THREADS + (int)threadIdx.x;
  if (idx >= n * n) return;
  const int i = idx / n, j = idx - i * n;
  if (j > i) return;
  float v = 0.f;
  if (j < P) {                                              // partials [g][s][E]
    const int T = P * (P + 1) / 2;
    const float* src = F.part + (long long)g * S * F.E + (i < P ? i * (i + 1) / 2 + j : T + j);
    for (int s = 0; s < S; ++s) v += src[(long long)s * F.E];
  } else {
    v = (float)F.K;                                         // bias corner: the ones row against itself
  }
  v *= F.scale;
  float* dst = F.dst + (long long)g * n * n;
  const float out = F.first ? v : dst[(long long)i * n + j] + v;
  dst[(long long)i * n + j] = out;
  dst[(long long)j * n + i] = out;
}

template <int P>
void launch_narrow(hipStream_t stream, const GrpBatch& b, int blocks) {
  hipLaunchKernelGGL(group_gram_narrow_kernel<P>, dim3((unsigned)blocks), dim3(GRP_THREADS), 0, stream, b);
}

typedef void (*NarrowLaunch)(hipStream_t, const GrpBatch&, int);
const NarrowLaunch kNarrow[GRP_NARROW_MAX + 1] = {
    nullptr,              launch_narrow<1>,  launch_narrow<2>,  launch_narrow<3>,  launch_narrow<4>,  launch_narrow<5>,
    launch_narrow<6>,     launch_narrow<7>,  launch_narrow<8>,  launch_narrow<9>,  launch_narrow<10>, launch_narrow<11>,
    launch_narrow<12>,    launch_narrow<13>, launch_narrow<14>, launch_narrow<15>, launch_narrow<16>};

// Blocks of factor f in the pass `kind` (0: Gram, 1: reduce).
long long blocks_of(const curv_group_factor_desc& d, const Plan& p, int kind) {
  if (kind == 1) return (long long)d.groups * cdiv(p.n * p.n, GRP_THREADS);
  return (long long)d.groups * p.S;
}

GrpFactor factor_of(const curv_group_factor_desc& d, const Plan& p, float* part) {
  GrpFactor F;
  F.src = d.src;
  F.dst = d.dst;
  F.part = part;
  F.N = d.N; F.C = d.C; F.H = d.H; F.W = d.W; F.G = d.groups; F.cg = d.C / d.groups;
  F.kh = d.kh; F.kw = d.kw; F.sh = d.sh; F.sw = d.sw; F.ph = d.ph; F.pw = d.pw; F.Ho = p.Ho; F.Wo = p.Wo;
  F.P = p.P; F.n = p.n; F.has_bias = d.has_bias ? 1 : 0; F.first = d.first ? 1 : 0; F.scale = d.scale;
  F.K = p.K; F.S = p.S; F.E = p.E; F.base = 0;
  const int HoWo = p.Ho * p.Wo;
  F.step_n = GRP_THREADS / HoWo;
  const int rem = GRP_THREADS - F.step_n * HoWo;
  F.step_oh = rem / p.Wo;
  F.step_ow = rem - F.step_oh * p.Wo;
  return F;
}

// Launches the narrow factors `idx` in batches of GRP_BATCH: their Gram pass (kind 0, patch size narrow_P) or their
// reduce pass (kind 1).
int launch_batches(hipStream_t stream, const curv_group_factor_desc* descs, const Plan* plans, float* const* parts,
                   const int* idx, int count, int kind, int narrow_P) {
  return for_arg_batches<GrpFactor, GRP_BATCH, 1>(
      count, "curv_kfac_group_accumulate",
      [&](int k, GrpFactor* F, long long* blocks) {
        *F = factor_of(descs[idx[k]], plans[idx[k]], parts[idx[k]]);
        blocks[0] = blocks_of(descs[idx[k]], plans[idx[k]], kind);
      },
      [](int, long long blocks) { return blocks; },
      [&](const GrpBatch* b, const long long*, const unsigned* grid) {
        if (kind == 1)
          hipLaunchKernelGGL(group_reduce_kernel, dim3(grid[0]), dim3(GRP_THREADS), 0, stream, b[0]);
        else
          kNarrow[narrow_P](stream, b[0], (int)grid[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

// Wide factor: group-major copy into `copy`, then the ordinary build, one descriptor per group.
int build_wide(hipStream_t stream, const curv_group_factor_desc& d, const Plan& p, float* copy, void* build_ws,
               size_t build_bytes) {
  const long long planes = (long long)d.N * d.C;
  if (planes >= (1LL << 31)) {
    set_error("curv_kfac_group_accumulate: too many planes (%lld)", planes);
    return CURV_ERR_INVALID;
  }
  hipLaunchKernelGGL(group_major_copy_kernel, dim3((unsigned)planes), dim3(GRP_THREADS), 0, stream, d.src, copy, d.N,
                     d.C, d.C / d.groups, d.H * d.W, (long long)p.slot_floats);
  CURV_LAUNCH_CHECK();
  std::vector<curv_factor_desc> sub;
  wide_descs(d, p, copy, &sub);
  return curv_kfac_accumulate(stream, sub.data(), d.groups, build_ws, build_bytes);
}

// Scratch layout: the narrow factors' slice partials one after another, then ONE copy region and ONE build region that
// the wide factors use in turn (their calls are ordered on the stream).
struct Layout {
  size_t parts, copy, build, total;
};

Layout layout_of(const std::vector<Plan>& plans) {
  Layout L{0, 0, 0, 0};
  for (const Plan& p : plans) {
    L.parts += p.part_bytes;
    L.copy = std::max(L.copy, p.copy_bytes);
    L.build = std::max(L.build, align_up(p.build_bytes, 256));
  }
  L.total = L.parts + L.copy + L.build;
  return L;
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac_group_workspace_bytes(const curv_group_factor_desc* descs, int n_factors) {
  return side::workspace_bytes("curv_kfac_group_workspace_bytes", descs, n_factors, plan_of,
                               [](const std::vector<Plan>& plans) { return layout_of(plans).total; });
}

extern "C" int curv_kfac_group_plan_flops(const curv_group_factor_desc* descs, int n_factors, long long* out) {
  return side::plan_flops("curv_kfac_group_plan_flops", descs, n_factors, out, plan_of);
}

extern "C" int curv_kfac_group_accumulate(void* stream_, const curv_group_factor_desc* descs, int n_factors,
                                          void* workspace, size_t workspace_bytes) {
  const char* const name = "curv_kfac_group_accumulate";
  if (n_factors <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<Plan> plans;
  if (!side::plans_of(name, descs, n_factors, plan_of, &plans)) return CURV_ERR_INVALID;
  const Layout L = layout_of(plans);
  int rc = side::require_src_dst(name, descs, n_factors);
  if (rc == CURV_OK) rc = side::require_workspace(name, workspace, workspace_bytes, L.total, GRP_SLOT_ALIGN);
  if (rc != CURV_OK) return rc;
  std::vector<float*> parts(n_factors, nullptr);
  std::vector<int> idx(n_factors);
  size_t at = 0;
  for (int i = 0; i < n_factors; ++i) {
    parts[i] = (float*)((char*)workspace + at);
    at += plans[i].part_bytes;
  }
  float* copy = (float*)((char*)workspace + L.parts);
  void* build_ws = (char*)workspace + L.parts + L.copy;
  // narrow: Gram passes (one class per patch size), then one reduce pass over all of them
  for (int P = 1; P <= GRP_NARROW_MAX && rc == CURV_OK; ++P) {
    int count = 0;
    for (int i = 0; i < n_factors; ++i)
      if (plans[i].narrow && plans[i].P == P) idx[count++] = i;
    rc = launch_batches(stream, descs, plans.data(), parts.data(), idx.data(), count, 0, P);
  }
  if (rc != CURV_OK) return rc;
  int count = 0;
  for (int i = 0; i < n_factors; ++i)
    if (plans[i].narrow) idx[count++] = i;
  rc = launch_batches(stream, descs, plans.data(), parts.data(), idx.data(), count, 1, 0);
  // wide: one group-major copy and one ordinary build per factor, sharing the copy and build regions
  for (int i = 0; i < n_factors && rc == CURV_OK; ++i)
    if (!plans[i].narrow) rc = build_wide(stream, descs[i], plans[i], copy, build_ws, L.build);
  return rc;
}
