// KFAC factor build from bf16 / fp16 sources (curv_kfac16_accumulate, include/curv_hip.h, ABI 12):
//   dst (+)= scale * X X^T
// with X the implicit im2col of a half-precision `src` (rows (c, kh, kw), columns (n, oh, ow)) plus the row of ones when
// `has_bias`.  A product of two bf16 (8 significant bits) or two fp16 (11 bits) numbers is exact in fp32, so the
// v_mfma_f32_32x32x16_bf16 / _f16 build with fp32 accumulation computes what the fp32 build computes on the upcast
// source, up to the order of the sums - at 16x the fp32 MFMA rate.
//
// Three launches per batch of factors (one form for every geometry):
//   1. pack: X of every factor into the workspace in the source dtype, K-contiguous rows of Kp = 16 ceil(K / 16)
//      elements, R = 128 ceil(dim / 128) rows; padding rows and the padded columns of every row - the ones row's
//      included - are 0.  Every later read of the build stays inside this image (no soffset-dependent bounds).
//   2. SYRK: one workgroup per (K slice, 128 x 128 tile on or above the diagonal); 2 x 2 waves of 64 x 64, each 2 x 2
//      MFMAs of 32x32x16 per stage of 16 columns.  Both 128-row panels of a stage arrive by LDS-DMA (buffer_load_dwordx4
//      ... lds, 1 KiB = 32 rows x 32 B per wave-instruction) into a ring of 4 stage buffers (3 stages in flight) whose
//      two 16-byte halves of a row are XOR-swizzled by (row >> 3) & 1, so the operands come back with ds_read_b128
//      (tools/micro/flat_bf16_probe.hip, LAB_NOTEBOOK R6.7).  Every stage is full and straight-line: the padding is
//      zeros in the image.  fp32 accumulation chains are cut every 64 stages.  Each item writes its fp32 128 x 128 slab.
//   3. reduce: one thread per entry of dst; the upper-triangle entry (min, max) of its position sums its slabs in slice
//      order, is scaled, overwrites or adds into dst.  Both (i, j) and (j, i) take the same value: exactly symmetric.
// The slicing and tiling of a factor follow from its own geometry, and every item and reduce thread reads only its own
// factor's image and slabs: a factor's bits do not depend on the other factors of the call.  No atomics, no host
// synchronisation, no device allocation (graph capture works).  Factor tables travel as kernel arguments.
#include "side_build.h"

namespace curv {
namespace {

constexpr int H16_THREADS = 256;
constexpr int H16_TM = 128;                    // tile rows / columns
constexpr int H16_KC = 16;                     // K columns per stage (one 32x32x16 MFMA step)
constexpr int H16_ROW_B = H16_KC * 2;          // 32 B per image row
constexpr int H16_IMG_B = H16_TM * H16_ROW_B;  // 4 KiB per panel per stage
constexpr int H16_AHEAD = 3;                   // stages in flight (LDS-DMA)
constexpr int H16_NBUF = 4;                    // ring of stage buffers: 32 KiB
constexpr int H16_FLUSH = 64;                  // stages per fp32 MFMA accumulation chain
static_assert(H16_NBUF > H16_AHEAD && (H16_NBUF & (H16_NBUF - 1)) == 0 && H16_AHEAD <= 3, "ring and vmcnt waits");
constexpr int H16_BATCH = 16;
constexpr int H16_ITEMS_TARGET = 512;          // a factor is cut into K slices until it has about this many items ...
constexpr int H16_SPI_MIN = 256;               // ... of at least 256 stages (4096 columns) ...
constexpr int H16_SPI_MAX = 512;               // ... and at most 512 (fp32 accumulation chains of <= 8192 products)
constexpr int H16_PACK_PER_THREAD = 8;         // columns per pack thread (one 16-byte store)
constexpr long long H16_K_MAX = 1LL << 23;     // image offsets of a 128-row panel stay below 2^32 bytes

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) char lds_char;

struct H16Factor {
  const uint16_t* src;
  float* dst;
  uint16_t* img;              // X: R x Kp in the source dtype
  float* slabs;               // S x T slabs of 128 x 128 fp32
  int N, C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo;
  int rows;                   // C kh kw (the ones row, if any, is row `rows`)
  int dim, P, T;              // dim = rows + has_bias, P = R / 128 panels, T = P (P + 1) / 2 tiles
  int K, Kp, stages, spi, S;
  int has_bias, first;
  int copy_rows;              // pack rows are plain 16-byte copies of the source (see h16_pack_kernel)
  float scale;
  unsigned short one;         // 1.0 in the source dtype
  long long base;             // first pack thread / item / reduce block of this factor in the launch
};

typedef ArgBatch<H16Factor, H16_BATCH> H16Batch;

struct Plan {
  int Ho, Wo, rows, dim, P, T, K, Kp, stages, spi, S;
  size_t img_bytes, slab_bytes;
  long long flops;
};

bool plan_of(const curv_factor16_desc& d, int index, Plan* p) {
  side::ConvGeom g;
  if (!side::conv_geom_of(d, "curv_kfac16", "factor", index, &g)) return false;
  if (d.dtype != CURV_DTYPE_BF16 && d.dtype != CURV_DTYPE_F16) {
    set_error("curv_kfac16: factor %d: unknown dtype %d (CURV_DTYPE_BF16 = 1, CURV_DTYPE_F16 = 2)", index, d.dtype);
    return false;
  }
  p->Ho = g.Ho;
  p->Wo = g.Wo;
  const long long K = (long long)d.N * p->Ho * p->Wo;
  const long long rows = (long long)d.C * d.kh * d.kw;
  if (K > H16_K_MAX || rows > 65536) {
    set_error("curv_kfac16: factor %d: too large (%lld columns, at most %lld; %lld rows, at most 65536)", index, K,
              H16_K_MAX, rows);
    return false;
  }
  p->K = (int)K;
  p->rows = (int)rows;
  p->dim = p->rows + (d.has_bias ? 1 : 0);
  p->P = cdiv(p->dim, H16_TM);
  p->T = p->P * (p->P + 1) / 2;
  p->stages = cdiv(p->K, H16_KC);
  p->Kp = p->stages * H16_KC;
  const int want = std::max(1, cdiv(H16_ITEMS_TARGET, p->T));
  p->spi = std::min(H16_SPI_MAX, std::max(H16_SPI_MIN, cdiv(p->stages, want)));
  p->spi = std::min(p->spi, p->stages);
  p->S = cdiv(p->stages, p->spi);
  p->img_bytes = align_up((size_t)p->P * H16_TM * p->Kp * 2, 256);
  p->slab_bytes = (size_t)p->S * p->T * H16_TM * H16_TM * sizeof(float);
  p->flops = 2LL * p->T * H16_TM * H16_TM * p->Kp;
  return true;
}

// Pack: one thread per 8 consecutive columns of one image row (one 16-byte store); threads of a factor R x Kp / 8.
__global__ void __launch_bounds__(H16_THREADS) h16_pack_kernel(const H16Batch batch) {
  const long long t = (long long)blockIdx.x * H16_THREADS + threadIdx.x;
  const H16Factor& F = batch.e[owner_of(batch, t)];
  const long long local = t - F.base;
  const int groups_per_row = F.Kp / H16_PACK_PER_THREAD;
  if (local >= (long long)F.P * H16_TM * groups_per_row) return;
  const int r = (int)(local / groups_per_row);
  const int k0 = (int)(local - (long long)r * groups_per_row) * H16_PACK_PER_THREAD;
  unsigned short v[H16_PACK_PER_THREAD];
  if (F.copy_rows && r < F.rows) {
    // 1x1 / stride 1 / no padding, H W a multiple of 8: the 8 columns are 8 consecutive pixels of one (n, c) plane
    const int HW = F.H * F.W, n = k0 / HW, p = k0 - n * HW;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (k0 < F.K) w = *reinterpret_cast<const uint4*>(F.src + ((long long)n * F.C + r) * HW + p);
    *reinterpret_cast<uint4*>(F.img + (long long)r * F.Kp + k0) = w;
    return;
  }
  if (r < F.rows) {
    const int khw = F.kh * F.kw;
    const int c = r / khw, q = r - c * khw;
    const int a = q / F.kw, b = q - a * F.kw;
    const int HoWo = F.Ho * F.Wo;
    int n = k0 / HoWo;
    const int rem = k0 - n * HoWo;
    int oh = rem / F.Wo, ow = rem - oh * F.Wo;
    const long long plane = (long long)F.H * F.W;
#pragma unroll
    for (int e = 0; e < H16_PACK_PER_THREAD; ++e) {
      const int ih = oh * F.sh - F.ph + a, iw = ow * F.sw - F.pw + b;
      // a masked gather reads src[0]: nothing outside `src` is touched
      const bool ok = k0 + e < F.K && (unsigned)ih < (unsigned)F.H && (unsigned)iw < (unsigned)F.W;
      const unsigned short x = F.src[ok ? ((long long)n * F.C + c) * plane + (long long)ih * F.W + iw : 0];
      v[e] = ok ? x : (unsigned short)0;
      if (++ow == F.Wo) {
        ow = 0;
        if (++oh == F.Ho) { oh = 0; ++n; }
      }
    }
  } else {
    const bool ones = F.has_bias && r == F.rows;
#pragma unroll
    for (int e = 0; e < H16_PACK_PER_THREAD; ++e) v[e] = (ones && k0 + e < F.K) ? F.one : (unsigned short)0;
  }
  uint4 w;
  w.x = v[0] | ((unsigned)v[1] << 16);
  w.y = v[2] | ((unsigned)v[3] << 16);
  w.z = v[4] | ((unsigned)v[5] << 16);
  w.w = v[6] | ((unsigned)v[7] << 16);
  *reinterpret_cast<uint4*>(F.img + (long long)r * F.Kp + k0) = w;
}

template <int DT> struct Mfma;
template <> struct Mfma<CURV_DTYPE_BF16> {
  typedef bf16x8 frag;
  static __device__ inline f32x16 run(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mfma<CURV_DTYPE_F16> {
  typedef f16x8 frag;
  static __device__ inline f32x16 run(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// SYRK: one workgroup per item = slice S_idx x T + tile of one factor.  Wave (wm, wn) computes rows 64 wm .. + 64 of
// panel i against rows 64 wn .. + 64 of panel j.  Fragment maps (32x32x16): lane l holds row l & 31, k = 8 (l >> 5) .. + 8
// of both operands; accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
template <int DT>
__global__ void __launch_bounds__(H16_THREADS, 3) h16_syrk_kernel(const H16Batch batch, long long items) {
  typedef typename Mfma<DT>::frag frag;
  __shared__ __attribute__((aligned(1024))) char smem[H16_NBUF * 2 * H16_IMG_B];   // [buffer][panel i, panel j]
  lds_char* lds = (lds_char*)smem;
  long long item;
  {
    // 32 consecutive items on one XCD (they share panels in L2); the grid is a multiple of 256
    const long long bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
    item = ((j >> 5) * 8 + xcd) * 32 + (j & 31);
  }
  if (item >= items) return;
  const H16Factor& F = batch.e[owner_of(batch, item)];
  const int local = (int)(item - F.base);
  const int slice = local / F.T;
  int tile = local - slice * F.T, ti = 0;
  while (tile >= F.P - ti) { tile -= F.P - ti; ++ti; }
  const int tj = ti + tile;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, h = lane >> 5;
  const unsigned panel_b = (unsigned)H16_TM * F.Kp * 2;
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void*)(F.img + (long long)ti * H16_TM * F.Kp), 0, panel_b, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc((void*)(F.img + (long long)tj * H16_TM * F.Kp), 0, panel_b, 0x00020000);
  // DMA: wave w moves rows 32 w .. + 32 of both panels; lane -> row 32 w + (lane >> 1), physical half (lane & 1), which
  // holds logical half (lane & 1) ^ ((row >> 3) & 1)
  const int drow = 32 * wave + (lane >> 1);
  const int lhalf = (lane & 1) ^ ((drow >> 3) & 1);
  const unsigned voff = (unsigned)(drow * F.Kp + 8 * lhalf) * 2;
  auto issue = [&](int t, unsigned buf) {
    const unsigned soff = (unsigned)t * H16_ROW_B;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(lds + buf + wave * 1024), 16, voff, soff, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void*)(lds + buf + H16_IMG_B + wave * 1024), 16, voff, soff, 0, 0);
  };
  unsigned addr_a[2], addr_b[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int rA = 64 * wm + 32 * m + r32, rB = 64 * wn + 32 * m + r32;
    addr_a[m] = rA * H16_ROW_B + ((h ^ ((rA >> 3) & 1)) << 4);
    addr_b[m] = H16_IMG_B + rB * H16_ROW_B + ((h ^ ((rB >> 3) & 1)) << 4);
  }
  f32x16 c[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) c[m][n] = 0.0f;
  const int t0 = slice * F.spi, t1 = min(t0 + F.spi, F.stages);
  // H16_AHEAD stages in flight in a ring of H16_AHEAD + 1 buffers: stage t + H16_AHEAD is issued into the buffer that
  // stage t - 1 used, once every wave has passed the barrier behind its reads
  constexpr unsigned BUF_B = 2 * H16_IMG_B;
  for (int p = 0; p < H16_AHEAD && t0 + p < t1; ++p) issue(t0 + p, (unsigned)p * BUF_B);
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = 0.0f;
  for (int blk = t0; blk < t1; blk += H16_FLUSH) {
    const int blk_end = min(blk + H16_FLUSH, t1);
    for (int t = blk; t < blk_end; ++t) {
      // this wave's pieces of stage t have landed once at most 2 x (stages issued behind it) DMA loads are pending
      const int behind = min(H16_AHEAD - 1, t1 - 1 - t);
      if (behind >= 2)
        __builtin_amdgcn_s_waitcnt(0x0f74);                // vmcnt(4)
      else if (behind == 1)
        __builtin_amdgcn_s_waitcnt(0x0f72);                // vmcnt(2)
      else
        __builtin_amdgcn_s_waitcnt(0x0f70);                // vmcnt(0)
      // everybody's pieces; everybody is done with stage t - 1.  A bare s_barrier: __syncthreads' fence would wait for
      // the stages still in flight (vmcnt(0))
      __builtin_amdgcn_s_barrier();
      const unsigned buf = (unsigned)((t - t0) & (H16_NBUF - 1)) * BUF_B;
      if (t + H16_AHEAD < t1) issue(t + H16_AHEAD, (unsigned)((t + H16_AHEAD - t0) & (H16_NBUF - 1)) * BUF_B);
      frag a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = *reinterpret_cast<const __attribute__((address_space(3))) frag*>(lds + buf + addr_a[m]);
        b[m] = *reinterpret_cast<const __attribute__((address_space(3))) frag*>(lds + buf + addr_b[m]);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) c[m][n] = Mfma<DT>::run(a[m], b[n], c[m][n]);
    }
    // fp32 chains of at most H16_FLUSH stages, then a sum over the chunks in order
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        acc[m][n] += c[m][n];
        c[m][n] = 0.0f;
      }
  }
  float* q = F.slabs + (long long)local * (H16_TM * H16_TM) + (64 * wm) * H16_TM + 64 * wn;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        q[(32 * m + row) * H16_TM + 32 * n + r32] = acc[m][n][reg];
      }
}

// Reduce: one thread per entry (r, c) of dst; it sums, in slice order, the slab entries of the upper-triangle position
// (i, j) = (min, max), so dst[r][c] and dst[c][r] get the same bits.  Blocks of a factor: ceil(dim^2 / 256).
__global__ void __launch_bounds__(H16_THREADS) h16_reduce_kernel(const H16Batch batch) {
  const H16Factor& F = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long idx = (blockIdx.x - F.base) * H16_THREADS + threadIdx.x;
  const int dim = F.dim;
  if (idx >= (long long)dim * dim) return;
  const int r = (int)(idx / dim), c = (int)(idx - (long long)r * dim);
  const int i = min(r, c), j = max(r, c);
  const int ti = i / H16_TM, tj = j / H16_TM;
  const int tile = ti * F.P - ti * (ti - 1) / 2 + (tj - ti);
  const float* s = F.slabs + (long long)tile * (H16_TM * H16_TM) + (i - ti * H16_TM) * H16_TM + (j - tj * H16_TM);
  const long long step = (long long)F.T * (H16_TM * H16_TM);
  float v = 0.f;
#pragma unroll 8
  for (int sl = 0; sl < F.S; ++sl) v += s[sl * step];          // loads independent, adds in slice order
  v *= F.scale;
  float* out = F.dst + idx;
  *out = F.first ? v : *out + v;
}

H16Factor factor_of(const curv_factor16_desc& d, const Plan& p, char* region) {
  H16Factor F;
  F.src = (const uint16_t*)d.src;
  F.dst = d.dst;
  F.img = (uint16_t*)region;
  F.slabs = (float*)(region + p.img_bytes);
  F.N = d.N; F.C = d.C; F.H = d.H; F.W = d.W;
  F.kh = d.kh; F.kw = d.kw; F.sh = d.sh; F.sw = d.sw; F.ph = d.ph; F.pw = d.pw; F.Ho = p.Ho; F.Wo = p.Wo;
  F.rows = p.rows; F.dim = p.dim; F.P = p.P; F.T = p.T;
  F.K = p.K; F.Kp = p.Kp; F.stages = p.stages; F.spi = p.spi; F.S = p.S;
  F.has_bias = d.has_bias ? 1 : 0; F.first = d.first ? 1 : 0; F.scale = d.scale;
  F.one = d.dtype == CURV_DTYPE_BF16 ? 0x3F80 : 0x3C00;
  F.copy_rows = d.kh == 1 && d.kw == 1 && d.sh == 1 && d.sw == 1 && d.ph == 0 && d.pw == 0 && (d.H * d.W) % 8 == 0 &&
                (reinterpret_cast<uintptr_t>(d.src) & 15) == 0;
  F.base = 0;
  return F;
}

// Units of factor `p` in pass `kind`: 0 pack threads, 1 SYRK items, 2 reduce blocks.
long long units_of(const Plan& p, int kind) {
  if (kind == 0) return (long long)p.P * H16_TM * (p.Kp / H16_PACK_PER_THREAD);
  if (kind == 1) return (long long)p.S * p.T;
  return cdivll((long long)p.dim * p.dim, H16_THREADS);
}

// One pass over the factors `idx` (all of one dtype) in batches of H16_BATCH.
int launch_pass(hipStream_t stream, const curv_factor16_desc* descs, const Plan* plans, char* const* regions,
                const int* idx, int count, int kind) {
  return for_arg_batches<H16Factor, H16_BATCH, 1>(
      count, "curv_kfac16_accumulate",
      [&](int k, H16Factor* F, long long* units) {
        *F = factor_of(descs[idx[k]], plans[idx[k]], regions[idx[k]]);
        units[0] = units_of(plans[idx[k]], kind);
      },
      [&](int, long long units) {
        return kind == 0 ? cdivll(units, H16_THREADS) : kind == 1 ? cdivll(units, 256) * 256 : units;
      },
      [&](const H16Batch* b, const long long* units, const unsigned* grid) {
        if (kind == 0)
          hipLaunchKernelGGL(h16_pack_kernel, dim3(grid[0]), dim3(H16_THREADS), 0, stream, b[0]);
        else if (kind == 1 && descs[idx[0]].dtype == CURV_DTYPE_BF16)
          hipLaunchKernelGGL(h16_syrk_kernel<CURV_DTYPE_BF16>, dim3(grid[0]), dim3(H16_THREADS), 0, stream, b[0], units[0]);
        else if (kind == 1)
          hipLaunchKernelGGL(h16_syrk_kernel<CURV_DTYPE_F16>, dim3(grid[0]), dim3(H16_THREADS), 0, stream, b[0], units[0]);
        else
          hipLaunchKernelGGL(h16_reduce_kernel, dim3(grid[0]), dim3(H16_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

// Every factor has a region of its own: image, then slabs.
size_t region_bytes(const Plan& p) { return p.img_bytes + align_up(p.slab_bytes, 256); }

size_t bytes_of(const std::vector<Plan>& plans) {
  size_t total = 0;
  for (const Plan& p : plans) total += region_bytes(p);
  return total;
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac16_workspace_bytes(const curv_factor16_desc* descs, int n_factors) {
  return side::workspace_bytes("curv_kfac16_workspace_bytes", descs, n_factors, plan_of, bytes_of);
}

extern "C" int curv_kfac16_plan_flops(const curv_factor16_desc* descs, int n_factors, long long* out) {
  return side::plan_flops("curv_kfac16_plan_flops", descs, n_factors, out, plan_of);
}

extern "C" int curv_kfac16_accumulate(void* stream_, const curv_factor16_desc* descs, int n_factors, void* workspace,
                                      size_t workspace_bytes) {
  const char* const name = "curv_kfac16_accumulate";
  if (n_factors <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<Plan> plans;
  if (!side::plans_of(name, descs, n_factors, plan_of, &plans)) return CURV_ERR_INVALID;
  int rc = side::require_src_dst(name, descs, n_factors);
  if (rc == CURV_OK) rc = side::require_workspace(name, workspace, workspace_bytes, bytes_of(plans), 256);
  if (rc != CURV_OK) return rc;
  std::vector<char*> regions(n_factors);
  size_t at = 0;
  for (int i = 0; i < n_factors; ++i) {
    regions[i] = (char*)workspace + at;
    at += region_bytes(plans[i]);
  }
  // SYRK batches hold one dtype; pack and reduce take the same batches
  std::vector<int> idx;
  idx.reserve(n_factors);
  for (int dt : {CURV_DTYPE_BF16, CURV_DTYPE_F16})
    for (int i = 0; i < n_factors; ++i)
      if (descs[i].dtype == dt) idx.push_back(i);
  const int split = (int)std::count_if(descs, descs + n_factors, [](const curv_factor16_desc& d) {
    return d.dtype == CURV_DTYPE_BF16;
  });
  for (int kind = 0; kind < 3; ++kind) {
    rc = launch_pass(stream, descs, plans.data(), regions.data(), idx.data(), split, kind);
    if (rc == CURV_OK)
      rc = launch_pass(stream, descs, plans.data(), regions.data(), idx.data() + split, n_factors - split, kind);
    if (rc != CURV_OK) return rc;
  }
  return CURV_OK;
}
