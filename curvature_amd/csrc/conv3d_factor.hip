// KFAC A-factor build of Conv3d layers (curv_kfac_conv3d_accumulate, include/curv_hip.h).
//
// A 3-D convolution over x (N, C, D, H, W) is a 2-D convolution over the depth-unfolded copy
//   x'[(n Do + d), (c kd + a), h, w] = x[n, c, d sd + a - pd, h, w]      (0 where the depth index is outside [0, D))
// with kernel (kh, kw), stride (sh, sw), padding (ph, pw), N Do samples and C kd channels: the 2-D im2col of x' is the 3-D
// im2col of x column for column, its rows in the order of weight.reshape(Cout, -1).  So A is the plain factor of x'.
// Per factor:
//   1. gather pass: `src` is read once and the contiguous (N Do, C kd, H, W) stack is written into the workspace - a pure
//      plane mover: source plane (n, c, z) goes to every (d, a) with d sd + a - pd = z, at most ceil(kd / sd) places; the
//      planes of the stack whose depth index is padding are WRITTEN with zeros (the workspace is never assumed clean);
//   2. one curv_kfac_accumulate call for the stack (has_bias, scale and first of the layer): one call per factor, so the
//      launch plan - and with it the factor's bits - follow from the factor's own geometry.
// Scratch is the stack plus the plain build's scratch, flops are the plain build's for the stack.
// Every launch goes on the caller's stream; nothing waits on the host or allocates, so the call can be captured.
#include "side_build.h"

#include <string>

namespace curv {
namespace {

constexpr int C3_THREADS = 256;
constexpr int C3_TILE = 4096;            // floats of LDS a workgroup stages (16 KB: ten workgroups to a CU)
constexpr int C3_ZSEG = 4 * C3_TILE;     // floats of one (n, d) run a zero workgroup walks
constexpr size_t C3_ALIGN = 256;

struct Plan {
  int n;                      // dim
  int Do;                     // output depth
  long long P;                // H W: floats of a plane
  size_t stage_bytes, build_bytes;   // the stack; the scratch of its plain build
  long long flops;
};

// The plain build's descriptor of the stack at `stack`.
curv_factor_desc stack_desc(const curv_conv3d_factor_desc& d, const Plan& p, const char* stack) {
  curv_factor_desc e{};
  e.src = reinterpret_cast<const float*>(stack);
  e.dst = d.dst;
  e.N = d.N * p.Do; e.C = d.C * d.kd; e.H = d.H; e.W = d.W;
  e.kh = d.kh; e.kw = d.kw; e.sh = d.sh; e.sw = d.sw; e.ph = d.ph; e.pw = d.pw;
  e.has_bias = d.has_bias ? 1 : 0;
  e.first = d.first ? 1 : 0;
  e.scale = d.scale;
  e.path_hint = CURV_PATH_AUTO;          // the call holds this factor only
  return e;
}

bool plan_of(const curv_conv3d_factor_desc& d, int index, Plan* p) {
  const char* const who = "curv_kfac_conv3d";
  *p = Plan{};
  const char* fault = nullptr;
  if (d.N < 1 || d.C < 1 || d.D < 1 || d.H < 1 || d.W < 1 || d.kd < 1 || d.kh < 1 || d.kw < 1 || d.sd < 1 || d.sh < 1 ||
      d.sw < 1 || d.pd < 0 || d.ph < 0 || d.pw < 0)
    fault = "invalid geometry";
  else if ((long long)d.D + 2LL * d.pd < d.kd || (long long)d.H + 2LL * d.ph < d.kh || (long long)d.W + 2LL * d.pw < d.kw)
    fault = "kernel larger than the padded input";
  if (fault) {
    set_error("%s: factor %d: %s (N %d C %d D %d H %d W %d kernel %dx%dx%d stride %dx%dx%d padding %dx%dx%d)", who, index,
              fault, d.N, d.C, d.D, d.H, d.W, d.kd, d.kh, d.kw, d.sd, d.sh, d.sw, d.pd, d.ph, d.pw);
    return false;
  }
  const long long Do = ((long long)d.D + 2LL * d.pd - d.kd) / d.sd + 1;
  const long long P = (long long)d.H * d.W, rows = (long long)d.N * d.C * d.D, samples = (long long)d.N * Do,
                  channels = (long long)d.C * d.kd;
  // the gather counts source planes, the samples and channels of the stack, and the floats of one sample of the stack, in
  // 32 bits; the plain build has limits of its own for the stack
  const long long lim = 1LL << 31;
  if (rows >= lim || samples >= lim || channels >= lim || P >= lim || channels * P >= lim || (long long)d.pd + d.D >= lim ||
      samples * channels * P >= (1LL << 40)) {
    set_error("%s: factor %d: too large (%lld source planes of %lld values, a stack of %lld samples x %lld channels)", who,
              index, rows, P, samples, channels);
    return false;
  }
  p->Do = (int)Do;
  p->P = P;
  p->n = (int)std::min<long long>(channels * d.kh * d.kw + (d.has_bias ? 1 : 0), lim - 1);
  p->stage_bytes = align_up((size_t)(samples * channels * P) * sizeof(float), C3_ALIGN);
  const curv_factor_desc e = stack_desc(d, *p, reinterpret_cast<const char*>(C3_ALIGN));
  size_t need;
  if (!side::plain_plan(&e, 1, &need, &p->flops)) {
    const std::string why = curv_last_error();
    set_error("%s: factor %d: the plain build rejected the depth-unfolded stack (N %d C %d H %d W %d kernel %dx%d stride "
              "%dx%d padding %dx%d): %s", who, index, e.N, e.C, e.H, e.W, e.kh, e.kw, e.sh, e.sw, e.ph, e.pw, why.c_str());
    return false;
  }
  p->build_bytes = align_up(need, C3_ALIGN);
  return true;
}

struct GatherArgs {
  const float* src;
  float* dst;                 // the stack, 256-byte aligned
  unsigned rows;              // N C D source planes
  unsigned C, D, Do, kd, sd, pd;
  unsigned P;                 // floats of a plane
  unsigned TP;                // source planes per copy workgroup (1 when a plane is walked in pieces)
  unsigned pieces;            // pieces of a plane (1: a workgroup stages whole planes)
  unsigned lw_log;            // log2 of the lanes that walk one destination plane
  unsigned copy_blocks;       // workgroups [0, copy_blocks) copy, the others write the padding planes
  unsigned dlo, dhi, nd;      // output depths with padding planes: [0, dlo) and [dhi, Do), nd of them
  unsigned zsegs;             // C3_ZSEG pieces of the C kd P floats of one (n, d) sample of the stack
};

// `len` floats to `out`, whose float offset from the 16-byte aligned stack base is `off`: 16-byte stores between a scalar
// head and tail, walked by LW = 2^lw_log neighbouring lanes.  `row`: the values in LDS.
__device__ __forceinline__ void write_run(float* out, unsigned off, const float* row, unsigned len, unsigned lane_j,
                                          unsigned LW) {
  const unsigned head = min(len, (4u - (off & 3u)) & 3u);
  const unsigned quads = (len - head) >> 2, tail = head + 4 * quads;
  for (unsigned i = lane_j; i < head; i += LW) out[i] = row[i];
  for (unsigned i = tail + lane_j; i < len; i += LW) out[i] = row[i];
  const float* from = row + head;
  float4* to = reinterpret_cast<float4*>(out + head);
  if (((uintptr_t)from & 15u) == 0) {
    for (unsigned q = lane_j; q < quads; q += LW) to[q] = *reinterpret_cast<const float4*>(from + 4 * q);
  } else {
    for (unsigned q = lane_j; q < quads; q += LW) to[q] = make_float4(from[4 * q], from[4 * q + 1], from[4 * q + 2], from[4 * q + 3]);
  }
}

// Copy workgroup b stages source planes [b TP, (b + 1) TP) - or piece b % pieces of plane b / pieces - one contiguous run
// of `src`, in LDS with 16-byte loads (a scalar head and tail where the run does not start or end on a 16-byte boundary:
// the source may be only 4-byte aligned and a plane need not be a whole number of 16-byte groups), then writes it to every
// place it has in the stack: 2^lw_log neighbouring lanes walk one destination plane, 256 >> lw_log (plane, a) pairs are
// written side by side, so short planes still fill the wave.  A source element is read once.  The pair of a lane is
// decoded once per plane (32-bit divisions), not per element.  Plane bases are 64-bit, every index inside a plane 32-bit.
// The workgroups behind the copy ones write the padding planes: workgroup (n, d, segment) walks C3_ZSEG floats of the
// C kd P floats of sample n Do + d of the stack, d one of the output depths that have padding planes, and stores zeros
// where the plane's depth index d sd + a - pd is outside [0, D).
__global__ void __launch_bounds__(C3_THREADS) conv3d_gather_kernel(const GatherArgs A) {
  __shared__ __attribute__((aligned(16))) float tile[C3_TILE];
  const unsigned tid = threadIdx.x, P = A.P, kd = A.kd;
  if (blockIdx.x >= A.copy_blocks) {
    const unsigned z = blockIdx.x - A.copy_blocks;
    const unsigned seg = z % A.zsegs, nd = z / A.zsegs;
    const unsigned n = nd / A.nd, di = nd - n * A.nd;
    const unsigned d = di < A.dlo ? di : A.dhi + (di - A.dlo);
    const unsigned run = A.C * kd * P;                                 // floats of one sample of the stack (< 2^31)
    const long long base = (long long)(n * A.Do + d) * run;            // (n Do + d < 2^31)
    float* out = A.dst + base;
    const unsigned mis = (unsigned)(base & 3);                         // float offset of the run from a 16-byte boundary
    const unsigned e0 = seg * C3_ZSEG, e1 = min(run, e0 + C3_ZSEG);    // (C3_ZSEG is a multiple of 4)
    const int t0 = (int)(d * A.sd) - (int)A.pd;                        // depth index of a = 0
    // aligned groups of four: group q holds the elements [4 q - mis, 4 q - mis + 4) of the run
    for (unsigned q = (e0 + mis) / 4 + tid; 4 * q < e1 + mis; q += C3_THREADS) {
      const unsigned lo = 4 * q < mis + e0 ? e0 : 4 * q - mis, hi = min(e1, 4 * q + 4 - mis);
      unsigned plane = lo / P, left = (plane + 1) * P - lo;            // elements of `plane` from `lo` on
      int t = t0 + (int)(plane % kd);
      bool pad = t < 0 || t >= (int)A.D;
      if (hi - lo == 4 && left >= 4) {
        if (pad) *reinterpret_cast<float4*>(out + lo) = make_float4(0.f, 0.f, 0.f, 0.f);
        continue;
      }
      for (unsigned e = lo; e < hi; ++e) {
        if (left == 0) {
          ++plane;
          left = P;
          t = t0 + (int)(plane % kd);
          pad = t < 0 || t >= (int)A.D;
        }
        if (pad) out[e] = 0.f;
        --left;
      }
    }
    return;
  }
  unsigned R0, nrows, p0, len;
  if (A.pieces == 1) {
    R0 = blockIdx.x * A.TP; nrows = min(A.TP, A.rows - R0); p0 = 0; len = P;
  } else {
    R0 = blockIdx.x / A.pieces; nrows = 1; p0 = (blockIdx.x - R0 * A.pieces) * C3_TILE; len = min((unsigned)C3_TILE, P - p0);
  }
  const unsigned count = nrows * len;                                  // <= C3_TILE
  const float* span = A.src + ((long long)R0 * P + p0);
  constexpr unsigned QUADS = C3_TILE / 4 / C3_THREADS;
  {
    const unsigned head = min(count, (unsigned)((4u - (unsigned)((uintptr_t)span >> 2)) & 3u));
    const unsigned quads = (count - head) >> 2, tail = head + 4 * quads;
    float4 v[QUADS];
#pragma unroll
    for (unsigned i = 0; i < QUADS; ++i)                               // every load in flight before the first LDS store
      if (tid + C3_THREADS * i < quads) v[i] = *reinterpret_cast<const float4*>(span + head + 4 * (tid + C3_THREADS * i));
    if (tid < head) tile[tid] = span[tid];
    if (tail + tid < count) tile[tail + tid] = span[tail + tid];
#pragma unroll
    for (unsigned i = 0; i < QUADS; ++i) {
      const unsigned q = tid + C3_THREADS * i;
      if (q < quads) {
        float* t = tile + head + 4 * q;
        if (head == 0) *reinterpret_cast<float4*>(t) = v[i];
        else { t[0] = v[i].x; t[1] = v[i].y; t[2] = v[i].z; t[3] = v[i].w; }
      }
    }
  }
  __syncthreads();
  const unsigned LW = 1u << A.lw_log, lane_j = tid & (LW - 1), lane_r = tid >> A.lw_log, RP = C3_THREADS >> A.lw_log;
  for (unsigned job = lane_r; job < nrows * kd; job += RP) {
    const unsigned r = job / kd, a = job - r * kd;
    const unsigned R = R0 + r;
    const unsigned nc = R / A.D, z = R - nc * A.D;                     // nc = n C + c
    const unsigned t = z + A.pd;                                       // = d sd + a
    if (t < a) continue;
    const unsigned d = (t - a) / A.sd;
    if (d * A.sd != t - a || d >= A.Do) continue;
    const unsigned n = nc / A.C, c = nc - n * A.C;
    const long long off = (((long long)(n * A.Do + d) * A.C + c) * kd + a) * P + p0;
    write_run(A.dst + off, (unsigned)(off & 3), tile + r * len, len, lane_j, LW);
  }
}

int build_one(hipStream_t stream, const curv_conv3d_factor_desc& d, const Plan& p, char* stack, void* build_ws) {
  GatherArgs A;
  A.src = d.src;
  A.dst = reinterpret_cast<float*>(stack);
  A.rows = (unsigned)((long long)d.N * d.C * d.D);
  A.C = d.C; A.D = d.D; A.Do = p.Do; A.kd = d.kd; A.sd = d.sd; A.pd = d.pd;
  A.P = (unsigned)p.P;
  A.TP = (unsigned)std::max<long long>(1, C3_TILE / p.P);
  A.pieces = (unsigned)cdivll(p.P, C3_TILE);
  const long long walked = std::min<long long>(p.P, C3_TILE);          // floats of one destination run
  A.lw_log = 0;
  while (A.lw_log < 8 && (4LL << A.lw_log) < walked) ++A.lw_log;
  const long long copy_blocks = A.pieces == 1 ? cdivll(A.rows, A.TP) : (long long)A.rows * A.pieces;
  // the output depths that have a padding plane: d sd < pd (below the input) and d sd + kd - 1 >= D + pd (above it)
  const long long dlo = std::min<long long>(p.Do, cdivll(d.pd, d.sd));
  const long long over = (long long)d.D + d.pd - d.kd + 1;             // first d sd that reaches past the input
  const long long dhi = std::max(dlo, std::min<long long>(p.Do, over <= 0 ? 0 : cdivll(over, d.sd)));
  A.dlo = (unsigned)dlo; A.dhi = (unsigned)dhi; A.nd = (unsigned)(dlo + (p.Do - dhi));
  A.zsegs = (unsigned)cdivll((long long)d.C * d.kd * p.P, C3_ZSEG);
  const long long zero_blocks = (long long)d.N * A.nd * A.zsegs;
  if (copy_blocks + zero_blocks >= (1LL << 31)) {
    set_error("curv_kfac_conv3d_accumulate: too many workgroups (%lld)", copy_blocks + zero_blocks);
    return CURV_ERR_INVALID;
  }
  A.copy_blocks = (unsigned)copy_blocks;
  hipLaunchKernelGGL(conv3d_gather_kernel, dim3((unsigned)(copy_blocks + zero_blocks)), dim3(C3_THREADS), 0, stream, A);
  CURV_LAUNCH_CHECK();
  const curv_factor_desc e = stack_desc(d, p, stack);
  return curv_kfac_accumulate(stream, &e, 1, build_ws, p.build_bytes);
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac_conv3d_workspace_bytes(const curv_conv3d_factor_desc* descs, int n_factors) {
  // the sum over the factors (every factor has scratch of its own); never 0 for valid descriptors: 0 reports an error
  return side::workspace_bytes("curv_kfac_conv3d_workspace_bytes", descs, n_factors, plan_of, side::staged_bytes<Plan>);
}

extern "C" int curv_kfac_conv3d_plan_flops(const curv_conv3d_factor_desc* descs, int n_factors, long long* out) {
  return side::plan_flops("curv_kfac_conv3d_plan_flops", descs, n_factors, out, plan_of);
}

extern "C" int curv_kfac_conv3d_accumulate(void* stream_, const curv_conv3d_factor_desc* descs, int n_factors,
                                           void* workspace, size_t workspace_bytes) {
  return side::staged_accumulate("curv_kfac_conv3d_accumulate", (hipStream_t)stream_, descs, n_factors, workspace,
                                 workspace_bytes, C3_ALIGN, plan_of, build_one);
}
