// KFAC A-factor build of transposed convolutions (curv_kfac_convt_accumulate, include/curv_hip.h).
//
// A ConvTranspose2d output pixel o = (oh, ow) receives tap (a, b) only when a = (oh + ph) (mod sh) and b = (ow + pw)
// (mod sw): its patch, read through the zero-stuffed input, is mostly structural zeros.  The outputs split into sh sw
// phases r = ((oh + ph) mod sh, (ow + pw) mod sw).  Along one dimension (h; w alike), phase r holds the taps
// a = r + s j, j < J = ceil((k - r) / s), and the outputs oh = r - p + s q, q0 <= q <= q1; its patch entry for tap j
// is x[q - j].  With j' = J - 1 - j and q = q0 + qh that is x[qh + j' + off], off = q0 - (J - 1): an ordinary stride-1
// correlation of a window of the input, rows [off, off + Q + J - 1), Q = q1 - q0 + 1, rows outside the input read 0.
// The phase Gram is therefore the KFAC factor of a Conv2d(C, ., (Jh, Jw)) over that window, rows (c, j'h, j'w).
//
// Per factor:
//   1. window pass: every phase whose window is not a symmetrically padded copy of the input gets a zero-bordered
//      (N, C, Qh + Jh - 1, Qw + Jw - 1) copy of its window in the workspace (reads only inside `src`);
//   2. one curv_kfac_accumulate call over the phases (fp32 MFMA, has_bias as the layer, scale 1, first): direct phases
//      read `src` itself with padding -off (every phase when kernel == stride and padding 0, the single phase of a
//      stride-1 layer), and equal direct phases are built once (all s^2 phases of U-Net's ConvTranspose2d(C, C/2, 2, 2));
//      one call per factor, so a factor's launch plan - and its bits - follow from its own geometry;
//   3. assembly pass: 32 x 32 tiles on and below the diagonal; each entry is looked up in its phase's Gram (0.0 between
//      taps of different phases), the bias corner is N Ho Wo, the result is scaled, written or added to dst, and the tile
//      is mirrored through LDS, so dst is exactly symmetric.
// Against a dense im2col of the zero-stuffed input (dim^2 N Ho Wo multiply-adds), the phase Grams execute about
// 1 / (sh sw)^2 of the products: each has 1 / (sh sw) of the rows and 1 / (sh sw) of the pixels.
// Every launch goes on the caller's stream; nothing waits on the host or allocates, so the call can be captured.
#include "side_build.h"

namespace curv {
namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_TILE = 32;
constexpr int CT_MAX_PHASES = CURV_CONVT_MAX_PHASES;
constexpr size_t CT_ALIGN = 256;

long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

// One dimension of one phase.
struct Dim {
  int J;        // taps of the phase
  int Q;        // outputs of the phase
  int off;      // input row of window row 0
};

Dim dim_of(int k, int s, int p, int Ho, int r) {
  Dim d;
  d.J = r < k ? (k - r + s - 1) / s : 0;
  const long long q0 = ceil_div((long long)p - r, s);
  const long long q1 = floor_div((long long)Ho - 1 + p - r, s);
  d.Q = (int)std::max(0LL, q1 - q0 + 1);
  d.off = (int)(q0 - (d.J - 1));
  return d;
}

struct Phase {
  Dim h, w;
  int P;          // patch rows C Jh Jw (0: no taps)
  bool empty;     // no taps or no outputs: its Gram is zero
  bool direct;    // window = the input padded symmetrically by (-h.off, -w.off)
  int slab;       // index of the Gram that holds this phase (-1: empty)
  int window;     // index of its window copy (-1: direct or empty)
};

struct Plan {
  int n, nph;
  long long K;                          // N Ho Wo
  Phase ph[CT_MAX_PHASES];
  std::vector<int> slab_phase;          // slab -> first phase it is built for
  std::vector<size_t> slab_off;         // byte offsets in the slab region
  std::vector<size_t> win_off;          // byte offsets in the window region
  std::vector<int> win_phase;
  size_t slab_bytes, win_bytes, build_bytes;
  long long flops;
};

// The phase descriptors of curv_kfac_accumulate: sources at `src` (direct) or the window copies at `win`, destinations
// at the slabs at `slabs`.
void phase_descs(const curv_convt_factor_desc& d, const Plan& p, const float* src, const char* win, char* slabs,
                 std::vector<curv_factor_desc>* out) {
  out->clear();
  for (size_t s = 0; s < p.slab_phase.size(); ++s) {
    const Phase& f = p.ph[p.slab_phase[s]];
    curv_factor_desc e{};
    e.N = d.N; e.C = d.C;
    e.kh = f.h.J; e.kw = f.w.J; e.sh = 1; e.sw = 1;
    if (f.direct) {
      e.src = src;
      e.H = d.H; e.W = d.W; e.ph = -f.h.off; e.pw = -f.w.off;
    } else {
      e.src = reinterpret_cast<const float*>(win + p.win_off[f.window]);
      e.H = f.h.Q + f.h.J - 1; e.W = f.w.Q + f.w.J - 1; e.ph = 0; e.pw = 0;
    }
    e.dst = reinterpret_cast<float*>(slabs + p.slab_off[s]);
    e.has_bias = d.has_bias ? 1 : 0;
    e.first = 1;
    e.scale = 1.f;
    e.path_hint = CURV_PATH_AUTO;        // the call holds this factor's phases only
    out->push_back(e);
  }
}

bool plan_of(const curv_convt_factor_desc& d, int index, Plan* p) {
  side::ConvGeom g;                      // the source side only: the output size is the caller's
  if (!side::source_geom_of(d, "curv_kfac_convt", "factor", index, &g)) return false;
  const long long ho_min = (long long)(d.H - 1) * d.sh - 2LL * d.ph + d.kh;
  const long long wo_min = (long long)(d.W - 1) * d.sw - 2LL * d.pw + d.kw;
  if (ho_min < 1 || wo_min < 1 || d.Ho < ho_min || d.Ho >= ho_min + d.sh || d.Wo < wo_min || d.Wo >= wo_min + d.sw) {
    set_error("curv_kfac_convt: factor %d: output %dx%d does not fit input %dx%d, kernel %dx%d, stride %dx%d, padding "
              "%dx%d (expected %lld..%lld x %lld..%lld)", index, d.Ho, d.Wo, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph,
              d.pw, ho_min, ho_min + d.sh - 1, wo_min, wo_min + d.sw - 1);
    return false;
  }
  if ((long long)d.sh * d.sw > CT_MAX_PHASES) {
    set_error("curv_kfac_convt: factor %d: stride %dx%d has more than %d phases", index, d.sh, d.sw, CT_MAX_PHASES);
    return false;
  }
  const long long n = (long long)d.C * d.kh * d.kw + (d.has_bias ? 1 : 0);
  const long long K = (long long)d.N * d.Ho * d.Wo;
  if (n > (1LL << 20) || K >= (1LL << 31)) {
    set_error("curv_kfac_convt: factor %d: too large (dim %lld, %lld output pixels)", index, n, K);
    return false;
  }
  p->n = (int)n;
  p->K = K;
  p->nph = d.sh * d.sw;
  p->slab_phase.clear();
  p->slab_off.clear();
  p->win_off.clear();
  p->win_phase.clear();
  p->slab_bytes = p->win_bytes = 0;
  for (int rh = 0; rh < d.sh; ++rh)
    for (int rw = 0; rw < d.sw; ++rw) {
      Phase& f = p->ph[rh * d.sw + rw];
      f.h = dim_of(d.kh, d.sh, d.ph, d.Ho, rh);
      f.w = dim_of(d.kw, d.sw, d.pw, d.Wo, rw);
      f.P = d.C * f.h.J * f.w.J;
      f.empty = f.P == 0 || f.h.Q == 0 || f.w.Q == 0;
      f.direct = !f.empty && f.h.off <= 0 && f.w.off <= 0 && f.h.Q + f.h.J - 1 == d.H - 2 * f.h.off &&
                 f.w.Q + f.w.J - 1 == d.W - 2 * f.w.off;
      f.slab = f.window = -1;
      if (f.empty) continue;
      if (f.direct)                      // equal direct phases read the same window: build their Gram once
        for (int q = 0; q < rh * d.sw + rw; ++q) {
          const Phase& g = p->ph[q];
          if (g.direct && g.h.J == f.h.J && g.w.J == f.w.J && g.h.off == f.h.off && g.w.off == f.w.off) {
            f.slab = g.slab;
            break;
          }
        }
      if (f.slab < 0) {
        f.slab = (int)p->slab_phase.size();
        p->slab_phase.push_back(rh * d.sw + rw);
        p->slab_off.push_back(p->slab_bytes);
        const size_t ns = (size_t)f.P + (d.has_bias ? 1 : 0);
        p->slab_bytes += align_up(ns * ns * sizeof(float), CT_ALIGN);
        if (!f.direct) {
          f.window = (int)p->win_off.size();
          p->win_phase.push_back(rh * d.sw + rw);
          p->win_off.push_back(p->win_bytes);
          p->win_bytes += align_up((size_t)d.N * d.C * (f.h.Q + f.h.J - 1) * (f.w.Q + f.w.J - 1) * sizeof(float),
                                   CT_ALIGN);
        }
      }
    }
  p->build_bytes = 0;
  p->flops = 0;
  if (p->slab_phase.empty()) return true;
  // the build's plan may depend on the 16-byte alignment of a direct source: size the scratch for both cases
  std::vector<curv_factor_desc> sub;
  const char* base = reinterpret_cast<const char*>(CT_ALIGN);
  for (int mis = 0; mis < 2; ++mis) {
    phase_descs(d, *p, reinterpret_cast<const float*>(base + 4 * mis), base, const_cast<char*>(base), &sub);
    size_t bytes;
    if (!side::plain_plan(sub.data(), (int)sub.size(), &bytes, mis ? &p->flops : nullptr)) {   // (one plan query, not two)
      set_error("curv_kfac_convt: factor %d: the phase build rejected the geometry", index);
      return false;
    }
    p->build_bytes = std::max(p->build_bytes, bytes);
  }
  return true;
}

// Zero-bordered window of every (sample, channel) plane: dst[plane][t][u] = src[plane][t + offh][u + offw], 0 outside.
__global__ void __launch_bounds__(CT_THREADS) convt_window_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                   int H, int W, int Hp, int Wp, int offh, int offw,
                                                                   long long total) {
  const long long HpWp = (long long)Hp * Wp;
  for (long long idx = (long long)blockIdx.x * CT_THREADS + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * CT_THREADS) {
    const long long plane = idx / HpWp;
    const int rem = (int)(idx - plane * HpWp);
    const int t = rem / Wp, u = rem - t * Wp;
    const int ih = t + offh, iw = u + offw;
    float v = 0.f;
    if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) v = src[plane * H * W + (long long)ih * W + iw];
    dst[idx] = v;
  }
}

struct AsmArgs {
  float* dst;
  int n, C, kh, kw, sh, sw, has_bias, first;
  float scale, corner;                   // corner: N Ho Wo (the ones row against itself), unscaled
  const float* slab[CT_MAX_PHASES];      // phase Gram (null: the phase contributes nothing)
  int ns[CT_MAX_PHASES];                 // its dimension: P + has_bias
  int P[CT_MAX_PHASES];
  int Jh[CT_MAX_PHASES], Jw[CT_MAX_PHASES];
};

// Tap row i < C kh kw -> (phase, row inside the phase Gram).
__device__ inline int tap_row(const AsmArgs& A, int i, int* phase) {
  const int khw = A.kh * A.kw;
  const int c = i / khw, t = i - c * khw;
  const int a = t / A.kw, b = t - a * A.kw;
  const int jh = a / A.sh, rh = a - jh * A.sh;
  const int jw = b / A.sw, rw = b - jw * A.sw;
  const int r = rh * A.sw + rw;
  *phase = r;
  const int Jh = A.Jh[r], Jw = A.Jw[r];
  return (c * Jh + (Jh - 1 - jh)) * Jw + (Jw - 1 - jw);
}

// Unscaled entry (i, j), j <= i, of the factor.
__device__ inline float entry(const AsmArgs& A, int i, int j) {
  if (A.has_bias && i == A.n - 1) {
    if (j == A.n - 1) return A.corner;
    int r;
    const int rj = tap_row(A, j, &r);
    const float* s = A.slab[r];
    return s ? s[(long long)A.P[r] * A.ns[r] + rj] : 0.f;
  }
  int ri_ph, rj_ph;
  const int ri = tap_row(A, i, &ri_ph);
  const int rj = tap_row(A, j, &rj_ph);
  const float* s = A.slab[ri_ph];
  return (ri_ph == rj_ph && s) ? s[(long long)ri * A.ns[ri_ph] + rj] : 0.f;
}

// Block (x, y) = 32 x 32 tile (row tile y, column tile x) on or below the diagonal: entries j <= i are looked up, scaled
// and written or added; the tile is then mirrored through LDS (coalesced both ways).
__global__ void __launch_bounds__(CT_THREADS) convt_assemble_kernel(const AsmArgs A) {
  const int I = blockIdx.y, J = blockIdx.x;
  if (J > I) return;
  __shared__ float tile[CT_TILE][CT_TILE + 1];
  const int tx = threadIdx.x & (CT_TILE - 1), ty = threadIdx.x / CT_TILE;
  const int n = A.n;
  for (int rr = ty; rr < CT_TILE; rr += CT_THREADS / CT_TILE) {
    const int i = I * CT_TILE + rr, j = J * CT_TILE + tx;
    float out = 0.f;
    if (i < n && j <= i) {
      const float v = entry(A, i, j) * A.scale;
      float* p = A.dst + (long long)i * n + j;
      out = A.first ? v : *p + v;
      *p = out;
    }
    tile[rr][tx] = out;
  }
  __syncthreads();
  for (int rr = ty; rr < CT_TILE; rr += CT_THREADS / CT_TILE) {
    const int j = J * CT_TILE + rr, i = I * CT_TILE + tx;       // upper entry (j, i) = lower entry (i, j)
    if (i < n && j < i) A.dst[(long long)j * n + i] = tile[tx][rr];
  }
}

int build_one(hipStream_t stream, const curv_convt_factor_desc& d, const Plan& p, char* slabs, char* win,
              void* build_ws, size_t build_bytes) {
  for (size_t w = 0; w < p.win_phase.size(); ++w) {
    const Phase& f = p.ph[p.win_phase[w]];
    const int Hp = f.h.Q + f.h.J - 1, Wp = f.w.Q + f.w.J - 1;
    const long long total = (long long)d.N * d.C * Hp * Wp;
    const long long blocks = std::min(cdivll(total, CT_THREADS), 1LL << 16);
    hipLaunchKernelGGL(convt_window_kernel, dim3((unsigned)blocks), dim3(CT_THREADS), 0, stream, d.src,
                       reinterpret_cast<float*>(win + p.win_off[w]), d.H, d.W, Hp, Wp, f.h.off, f.w.off, total);
    CURV_LAUNCH_CHECK();
  }
  if (!p.slab_phase.empty()) {
    std::vector<curv_factor_desc> sub;
    phase_descs(d, p, d.src, win, slabs, &sub);
    const int rc = curv_kfac_accumulate(stream, sub.data(), (int)sub.size(), build_ws, build_bytes);
    if (rc != CURV_OK) return rc;
  }
  AsmArgs A;
  A.dst = d.dst;
  A.n = p.n; A.C = d.C; A.kh = d.kh; A.kw = d.kw; A.sh = d.sh; A.sw = d.sw;
  A.has_bias = d.has_bias ? 1 : 0;
  A.first = d.first ? 1 : 0;
  A.scale = d.scale;
  A.corner = (float)p.K;
  for (int r = 0; r < CT_MAX_PHASES; ++r) {
    A.slab[r] = nullptr;
    A.ns[r] = A.P[r] = 0;
    A.Jh[r] = A.Jw[r] = 1;
  }
  for (int r = 0; r < p.nph; ++r) {
    const Phase& f = p.ph[r];
    A.Jh[r] = std::max(f.h.J, 1);
    A.Jw[r] = std::max(f.w.J, 1);
    A.P[r] = f.P;
    A.ns[r] = f.P + A.has_bias;
    if (f.slab >= 0) A.slab[r] = reinterpret_cast<const float*>(slabs + p.slab_off[f.slab]);
  }
  const int tiles = cdiv(p.n, CT_TILE);
  hipLaunchKernelGGL(convt_assemble_kernel, dim3((unsigned)tiles, (unsigned)tiles), dim3(CT_THREADS), 0, stream, A);
  CURV_LAUNCH_CHECK();
  return CURV_OK;
}

// Scratch: slabs, window copies and the build's own scratch of ONE factor at a time (factors run in turn on the stream).
struct Layout {
  size_t slabs, wins, build, total;
};

Layout layout_of(const std::vector<Plan>& plans) {
  Layout L{0, 0, 0, 0};
  for (const Plan& p : plans) {
    L.slabs = std::max(L.slabs, p.slab_bytes);
    L.wins = std::max(L.wins, p.win_bytes);
    L.build = std::max(L.build, align_up(p.build_bytes, CT_ALIGN));
  }
  L.total = L.slabs + L.wins + L.build;
  return L;
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_kfac_convt_workspace_bytes(const curv_convt_factor_desc* descs, int n_factors) {
  // never 0 for valid descriptors: 0 reports an error
  return side::workspace_bytes("curv_kfac_convt_workspace_bytes", descs, n_factors, plan_of,
                               [](const std::vector<Plan>& plans) { return std::max(layout_of(plans).total, CT_ALIGN); });
}

extern "C" int curv_kfac_convt_plan_flops(const curv_convt_factor_desc* descs, int n_factors, long long* out) {
  return side::plan_flops("curv_kfac_convt_plan_flops", descs, n_factors, out, plan_of);
}

extern "C" int curv_kfac_convt_accumulate(void* stream_, const curv_convt_factor_desc* descs, int n_factors,
                                          void* workspace, size_t workspace_bytes) {
  const char* const name = "curv_kfac_convt_accumulate";
  if (n_factors <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<Plan> plans;
  if (!side::plans_of(name, descs, n_factors, plan_of, &plans)) return CURV_ERR_INVALID;
  const Layout L = layout_of(plans);
  int rc = side::require_src_dst(name, descs, n_factors);
  if (rc == CURV_OK) rc = side::require_workspace(name, workspace, workspace_bytes, L.total, CT_ALIGN);
  if (rc != CURV_OK) return rc;
  char* slabs = (char*)workspace;
  char* win = slabs + L.slabs;
  void* build_ws = win + L.wins;
  for (int i = 0; i < n_factors; ++i) {
    rc = build_one(stream, descs[i], plans[i], slabs, win, build_ws, L.build);
    if (rc != CURV_OK) return rc;
  }
  return CURV_OK;
}
