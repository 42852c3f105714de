// KFAC A-factor build of dilated convolutions (curv_kfac_dilated_accumulate, include/curv_hip.h).
//
// A stride-1 convolution with dilation (dh, dw) and padding (dh p'h, dw p'w) reads, for every output pixel, taps that all
// lie in one residue class of the input grid modulo (dh, dw): output (oh, ow) of class rho = (oh mod dh, ow mod dw) reads
// x[oh - ph + a dh, ow - pw + b dw], rows = rho_h (mod dh) only.  Its im2col columns are therefore exactly the union, over
// the dh dw classes, of the im2col columns of the UNDILATED convolution (same kernel, stride 1, padding (p'h, p'w)) over
// the sub-image x[:, :, rho_h::dh, rho_w::dw], and A is the sum of the plain factors of the sub-images.  All classes share
// one tap set, so nothing is scattered afterwards (unlike the phases of csrc/convt_factor.hip).
//
// A sub-image has ceil(H / dh) rows for rho_h < H mod dh (every class when dh divides H) and floor(H / dh) otherwise, columns
// alike: at most 2 x 2 sizes.  Per factor:
//   1. gather pass: `src` is read once and every class sub-image is written into the workspace, the classes of one size
//      stacked as one contiguous (count N, C, Hg, Wg) tensor (class-major, classes in (rho_h, rho_w) order);
//   2. one curv_kfac_accumulate call per size group, one after another on the stream (has_bias and scale of the layer; the
//      first group overwrites dst when the caller's `first` is set, the others add): one call per group, so a group's launch
//      plan - and with it the factor's bits - follow from the factor's own geometry;
//   3. a class whose sub-image is EMPTY (dilation larger than the image) still has output pixels when the padding is large
//      enough: their patches are all padding, so they add scale N (their output count) to the bias corner and nothing else.
// A size group without output pixels (its sub-image plus padding is smaller than the kernel) is neither copied nor built.
// dh = dw = 1 is the plain build on `src` itself: no copy, the bits of curv_kfac_accumulate.
// Every launch goes on the caller's stream; nothing waits on the host or allocates, so the call can be captured.
#include "side_build.h"

#include <string>

namespace curv {
namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_TILE = 4096;            // floats of LDS a workgroup stages (16 KB: ten workgroups to a CU)
constexpr size_t DL_ALIGN = 256;

// Size group (hb, wb), index hb * 2 + wb: sub-images of (Hbig - hb) x (Wbig - wb).
struct Group {
  int Hg, Wg;                 // sub-image size (0: empty)
  int count;                  // classes of this size
  int Ho, Wo;                 // output size of one class: Hg + 2 p'h - kh + 1 (<= 0: no output pixels)
  bool built;                 // copied and built
  size_t off;                 // byte offset of its stack in the gather region
};

struct Plan {
  bool plain;                 // dh = dw = 1: curv_kfac_accumulate on src itself
  int n;                      // dim
  int nbh, nbw;               // classes below these have the larger size
  Group g[4];
  long long corner;           // N x output pixels of the classes with an empty sub-image
  size_t stage_bytes, build_bytes;   // the class stacks; the scratch of the plain builds (which run one after another)
  long long flops;
};

// The plain build's descriptor of size group `q` (of `src` itself for a plain plan), sources at `stacks`.
curv_factor_desc group_desc(const curv_dilated_factor_desc& d, const Plan& p, int q, const char* stacks) {
  curv_factor_desc e{};
  e.C = d.C; e.kh = d.kh; e.kw = d.kw; e.sh = 1; e.sw = 1;
  if (p.plain) {
    e.src = d.src;
    e.N = d.N; e.H = d.H; e.W = d.W; e.sh = d.sh; e.sw = d.sw; e.ph = d.ph; e.pw = d.pw;
  } else {
    e.src = reinterpret_cast<const float*>(stacks + p.g[q].off);
    e.N = d.N * p.g[q].count; e.H = p.g[q].Hg; e.W = p.g[q].Wg; e.ph = d.ph / d.dh; e.pw = d.pw / d.dw;
  }
  e.dst = d.dst;
  e.has_bias = d.has_bias ? 1 : 0;
  e.first = d.first ? 1 : 0;
  e.scale = d.scale;
  e.path_hint = CURV_PATH_AUTO;          // the call holds this group only
  return e;
}

// Scratch and flops of the plain build of `e` alone; false (error text set, the plain build's own text behind it) where
// the plain build refuses it: its size limits are this build's.
bool plain_plan(const curv_factor_desc& e, int index, size_t* bytes, long long* flops) {
  size_t need;
  long long f;
  if (!side::plain_plan(&e, 1, &need, &f)) {
    const std::string why = curv_last_error();
    set_error("curv_kfac_dilated: factor %d: the plain build rejected a class stack (N %d C %d H %d W %d kernel %dx%d "
              "padding %dx%d): %s", index, e.N, e.C, e.H, e.W, e.kh, e.kw, e.ph, e.pw, why.c_str());
    return false;
  }
  *bytes = std::max(*bytes, align_up(need, DL_ALIGN));
  *flops += f;
  return true;
}

bool plan_of(const curv_dilated_factor_desc& d, int index, Plan* p) {
  const char* const who = "curv_kfac_dilated";
  side::ConvGeom geom;
  if (!side::source_geom_of(d, who, "factor", index, &geom)) return false;
  if (d.dh < 1 || d.dw < 1) {
    set_error("%s: factor %d: dilation %dx%d below 1", who, index, d.dh, d.dw);
    return false;
  }
  *p = Plan{};
  p->plain = d.dh == 1 && d.dw == 1;
  p->n = 0;
  if (p->plain) {
    const curv_factor_desc e = group_desc(d, *p, 0, nullptr);
    if (!plain_plan(e, index, &p->build_bytes, &p->flops)) return false;
    p->n = d.C * d.kh * d.kw + (d.has_bias ? 1 : 0);
    return true;
  }
  if (d.sh != 1 || d.sw != 1) {
    set_error("%s: factor %d: stride %dx%d with dilation %dx%d (the class split needs stride 1)", who, index, d.sh, d.sw,
              d.dh, d.dw);
    return false;
  }
  if (d.ph % d.dh != 0 || d.pw % d.dw != 0) {
    set_error("%s: factor %d: padding %dx%d is not a multiple of the dilation %dx%d", who, index, d.ph, d.pw, d.dh, d.dw);
    return false;
  }
  const long long eh = (long long)(d.kh - 1) * d.dh + 1, ew = (long long)(d.kw - 1) * d.dw + 1;
  if (eh > (long long)d.H + 2LL * d.ph || ew > (long long)d.W + 2LL * d.pw) {
    set_error("%s: factor %d: dilated kernel %lldx%lld larger than the padded input (H %d W %d kernel %dx%d dilation %dx%d "
              "padding %dx%d)", who, index, eh, ew, d.H, d.W, d.kh, d.kw, d.dh, d.dw, d.ph, d.pw);
    return false;
  }
  const long long n = (long long)d.C * d.kh * d.kw + (d.has_bias ? 1 : 0);
  // the gather pass counts source rows, and the stacks samples, in 32 bits; a row longer than the staging tile is walked in
  // pieces of whole classes
  if (n > (1LL << 20) || (long long)d.N * d.C * d.H >= (1LL << 31) || (long long)d.N * d.dh * d.dw >= (1LL << 31) ||
      (d.W > DL_TILE && d.dw > DL_TILE)) {
    set_error("%s: factor %d: too large (dim %lld, %lld source rows, %lld class images)", who, index, n,
              (long long)d.N * d.C * d.H, (long long)d.N * d.dh * d.dw);
    return false;
  }
  p->n = (int)n;
  p->nbh = d.H % d.dh ? d.H % d.dh : d.dh;
  p->nbw = d.W % d.dw ? d.W % d.dw : d.dw;
  const int Hbig = (d.H + d.dh - 1) / d.dh, Wbig = (d.W + d.dw - 1) / d.dw;
  const int mh = 2 * (d.ph / d.dh) - d.kh + 1, mw = 2 * (d.pw / d.dw) - d.kw + 1;      // output size - sub-image size
  for (int q = 0; q < 4; ++q) {
    Group& g = p->g[q];
    const int hb = q >> 1, wb = q & 1;
    g.Hg = Hbig - hb; g.Wg = Wbig - wb;
    g.count = (hb ? d.dh - p->nbh : p->nbh) * (wb ? d.dw - p->nbw : p->nbw);
    g.Ho = g.Hg + mh; g.Wo = g.Wg + mw;
    g.built = false;
    g.off = 0;
    if (g.count == 0 || g.Ho <= 0 || g.Wo <= 0) continue;
    if (g.Hg == 0 || g.Wg == 0) {
      p->corner += (long long)d.N * g.count * g.Ho * g.Wo;
      continue;
    }
    g.built = true;
    g.off = p->stage_bytes;
    p->stage_bytes += align_up((size_t)d.N * g.count * d.C * g.Hg * g.Wg * sizeof(float), DL_ALIGN);
    const curv_factor_desc e = group_desc(d, *p, q, reinterpret_cast<const char*>(DL_ALIGN));
    if (!plain_plan(e, index, &p->build_bytes, &p->flops)) return false;
  }
  // (class (0, 0) has the larger size and output pixel (0, 0): the kernel fits, so group 0 is always built, and with it
  // the caller's `first` always has a build that honours it)
  p->build_bytes = std::max(p->build_bytes, DL_ALIGN);
  return true;
}

struct GatherArgs {
  const float* src;
  float* dst;                 // the gather region
  long long goff[4];          // float offset of the stack of size group hb * 2 + wb (-1: not built)
  unsigned rows;              // N C H source rows
  unsigned NC, H, W, dh, dw;
  unsigned nbh, nbw, Hbig, Wbig;
  unsigned TR;                // source rows per workgroup (1 when a row is walked in pieces)
  unsigned segw, js;          // columns per piece, segw = js dw (one piece: segw >= W)
  unsigned lw_log;            // log2 of the lanes that walk one class row
  unsigned dwl;               // min(dw, W): the classes that have columns
};

// Workgroup b stages source rows [b TR, (b + 1) TR) - one contiguous run of `src` - in LDS with 16-byte loads (a scalar
// head and tail where the run does not start or end on a 16-byte boundary), then writes every class row as a contiguous
// run: 2^lw_log neighbouring lanes walk one class row, 256 >> lw_log source rows are written side by side, so short class
// rows (7 values for a 28-wide image with dilation 4) still fill the wave.  The row of a lane is decoded once per source
// row (two 32-bit divisions), not per element; the class loop has none.  Every index below the row offset is 32-bit.
__global__ void __launch_bounds__(DL_THREADS) dilated_gather_kernel(const GatherArgs A) {
  __shared__ __attribute__((aligned(16))) float tile[DL_TILE];
  const unsigned W = A.W, H = A.H, dh = A.dh, dw = A.dw, tid = threadIdx.x;
  const unsigned R0 = blockIdx.x * A.TR;
  const unsigned nrows = min(A.TR, A.rows - R0);
  const unsigned LW = 1u << A.lw_log, lane_j = tid & (LW - 1), lane_r = tid >> A.lw_log, RP = DL_THREADS >> A.lw_log;
  constexpr unsigned QUADS = DL_TILE / 4 / DL_THREADS;
  for (unsigned w0 = 0, j0 = 0; w0 < W; w0 += A.segw, j0 += A.js) {
    const unsigned len = min(A.segw, W - w0);
    const unsigned count = nrows * len;                              // (nrows > 1 only where len == W) <= DL_TILE
    const float* span = A.src + ((long long)R0 * W + w0);
    if (w0) __syncthreads();                                         // the piece before has been written out
    const unsigned head = min(count, (unsigned)((4u - (unsigned)((uintptr_t)span >> 2)) & 3u));
    const unsigned quads = (count - head) >> 2, tail = head + 4 * quads;
    float4 v[QUADS];
#pragma unroll
    for (unsigned i = 0; i < QUADS; ++i)                             // every load in flight before the first LDS store
      if (tid + DL_THREADS * i < quads) v[i] = *reinterpret_cast<const float4*>(span + head + 4 * (tid + DL_THREADS * i));
    if (tid < head) tile[tid] = span[tid];
    if (tail + tid < count) tile[tail + tid] = span[tail + tid];
#pragma unroll
    for (unsigned i = 0; i < QUADS; ++i) {
      const unsigned q = tid + DL_THREADS * i;
      if (q < quads) {
        float* t = tile + head + 4 * q;
        if (head == 0) *reinterpret_cast<float4*>(t) = v[i];
        else { t[0] = v[i].x; t[1] = v[i].y; t[2] = v[i].z; t[3] = v[i].w; }
      }
    }
    __syncthreads();
    for (unsigned r = lane_r; r < nrows; r += RP) {
      const unsigned R = R0 + r;
      const unsigned plane = R / H, h = R - plane * H;               // plane = n C + c
      const unsigned hq = h / dh, rh = h - hq * dh;
      const unsigned hb = rh >= A.nbh, Hg = A.Hbig - hb, lh = hb ? rh - A.nbh : rh;
      const float* row = tile + r * len;
      for (unsigned rw = 0; rw < A.dwl; ++rw) {
        const unsigned wb = rw >= A.nbw, Wg = A.Wbig - wb;
        const long long off = hb ? (wb ? A.goff[3] : A.goff[2]) : (wb ? A.goff[1] : A.goff[0]);
        if (off < 0) continue;
        const unsigned slot = wb ? lh * (dw - A.nbw) + (rw - A.nbw) : lh * A.nbw + rw;      // class index in its group
        float* out = A.dst + off + (((long long)slot * A.NC + plane) * Hg + hq) * Wg;
        const unsigned jend = min(Wg, j0 + A.js);
        for (unsigned j = j0 + lane_j; j < jend; j += LW) out[j] = row[rw + (j - j0) * dw];
      }
    }
  }
}

// The bias corner of the classes with an empty sub-image.
__global__ void dilated_corner_kernel(float* corner, float add) {
  if (threadIdx.x == 0) *corner += add;
}

int build_one(hipStream_t stream, const curv_dilated_factor_desc& d, const Plan& p, char* stacks, void* build_ws) {
  if (p.plain) {
    const curv_factor_desc e = group_desc(d, p, 0, nullptr);
    return curv_kfac_accumulate(stream, &e, 1, build_ws, p.build_bytes);
  }
  GatherArgs A;
  A.src = d.src;
  A.dst = reinterpret_cast<float*>(stacks);
  bool any = false;
  for (int q = 0; q < 4; ++q) {
    A.goff[q] = p.g[q].built ? (long long)(p.g[q].off / sizeof(float)) : -1;
    any = any || p.g[q].built;
  }
  A.rows = (unsigned)((long long)d.N * d.C * d.H);
  A.NC = (unsigned)(d.N * d.C); A.H = d.H; A.W = d.W; A.dh = d.dh; A.dw = d.dw;
  A.nbh = p.nbh; A.nbw = p.nbw; A.Hbig = p.g[0].Hg; A.Wbig = p.g[0].Wg;
  A.TR = (unsigned)std::max(1, DL_TILE / d.W);
  A.js = d.W <= DL_TILE ? (unsigned)p.g[0].Wg : (unsigned)(DL_TILE / d.dw);
  A.segw = A.js * (unsigned)d.dw;
  A.lw_log = 0;
  while (A.lw_log < 6 && (1u << A.lw_log) < A.js) ++A.lw_log;
  A.dwl = (unsigned)std::min(d.dw, d.W);
  if (any) {
    const long long blocks = cdivll(A.rows, A.TR);
    hipLaunchKernelGGL(dilated_gather_kernel, dim3((unsigned)blocks), dim3(DL_THREADS), 0, stream, A);
    CURV_LAUNCH_CHECK();
  }
  bool first = d.first != 0;
  for (int q = 0; q < 4; ++q) {
    if (!p.g[q].built) continue;
    curv_factor_desc e = group_desc(d, p, q, stacks);
    e.first = first ? 1 : 0;
    first = false;
    const int rc = curv_kfac_accumulate(stream, &e, 1, build_ws, p.build_bytes);
    if (rc != CURV_OK) return rc;
  }
  if (p.corner > 0 && d.has_bias) {
    hipLaunchKernelGGL(dilated_corner_kernel, dim3(1), dim3(64), 0, stream, d.dst + (size_t)p.n * p.n - 1,
                       d.scale * (float)p.corner);
    CURV_LAUNCH_CHECK();
  }
  return CURV_OK;
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac_dilated_workspace_bytes(const curv_dilated_factor_desc* descs, int n_factors) {
  // the sum over the factors (every factor has scratch of its own); never 0 for valid descriptors: 0 reports an error
  return side::workspace_bytes("curv_kfac_dilated_workspace_bytes", descs, n_factors, plan_of, side::staged_bytes<Plan>);
}

extern "C" int curv_kfac_dilated_plan_flops(const curv_dilated_factor_desc* descs, int n_factors, long long* out) {
  return side::plan_flops("curv_kfac_dilated_plan_flops", descs, n_factors, out, plan_of);
}

extern "C" int curv_kfac_dilated_accumulate(void* stream_, const curv_dilated_factor_desc* descs, int n_factors,
                                            void* workspace, size_t workspace_bytes) {
  return side::staged_accumulate("curv_kfac_dilated_accumulate", (hipStream_t)stream_, descs, n_factors, workspace,
                                 workspace_bytes, DL_ALIGN, plan_of, build_one);
}
