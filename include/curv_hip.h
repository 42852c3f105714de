/*
 * curv_hip.h -- C ABI of libcurv_hip.so, the gfx950 (MI355X) implementation of the KFAC / EFB / INF
 * curvature hot path of DLR-RM/curvature.
 *
 * Every entry point is what a binding of the reference's `Curvature` plugin API would call for the
 * arithmetic it performs today through torch (reference file:line cited per function, paths relative
 * to the reference checkout).  Conventions:
 *   - plain C types only; all tensors are dense row-major fp32 device buffers unless stated;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls only enqueue work and
 *     never synchronise the device, so they are ordered after whatever produced their inputs on
 *     that stream (e.g. torch's backward);
 *   - the library owns no device memory: scratch comes from the caller (`*_workspace_bytes`);
 *   - return value 0 = ok, otherwise a CURV_ERR_* code with text in curv_last_error();
 *     numerical failure ("not positive definite") is reported through caller-provided device
 *     `info` words so that a whole model can be processed without a host round trip per layer;
 *   - re-entrant; results never depend on library state.  What the library keeps per calling thread (and device)
 *     besides the error string: a set of internal HIP streams and events (curv_init_streams below) on which the
 *     whole-model sweeps of curv_chol_inv_lower* / curv_kfac_accumulate fork and join the caller's stream.  They
 *     carry no data between calls; when they are created relative to the process's other streams can change the
 *     TIME of the unchecked inversion entry points (see curv_init_streams), never a result bit.
 */
#ifndef CURV_HIP_H
#define CURV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CURV_ABI_VERSION 12

#define CURV_OK 0
#define CURV_ERR_NOT_PD 1
#define CURV_ERR_INVALID 2
#define CURV_ERR_WORKSPACE 3
#define CURV_ERR_HIP 4
#define CURV_ERR_NOT_CONVERGED 5

int curv_version(void);
const char* curv_last_error(void);

/* Create the library's internal streams (per calling thread and current device) NOW instead of at the first
 * curv_chol_inv_lower / curv_kfac_accumulate call.  Whole-model inversions run their factor groups on four internal
 * streams; the runtime deals hardware queues onto the four pipes of the command processor in creation order, and a queue
 * that is not empty - the caller's own stream, which waits for the sweep - slows every queue on its pipe.  Whether one of
 * the sweep's two chains shares that pipe depends on how many streams the process created before the set (three raw
 * streams in front of it: invert() of the ResNet-50 factors 6.9 -> 10.9 ms until round 5).  curv_chol_inv_lower_status
 * no longer depends on it (it joins the caller's stream only after the host has the verdict: 6.83 / 6.80 / 6.87 ms for
 * none / three streams after / three before the set); curv_chol_inv_lower and curv_chol_factor_inverse, which never wait
 * on the host, still do: for those call this once, early - but AFTER the caller's own stream has launched something
 * (hardware queues are given out lazily, in order of first use).  The Python estimators do it in their constructor
 * (curvature_amd._lib.init_streams runs a one-element torch kernel first).  Idempotent.  (LAB_NOTEBOOK R5.6) */
int curv_init_streams(void);

/* ------------------------------------------------------------------------------------------------
 * KFAC factor build:  dst (+)= scale * X X^T           (curvature/curvatures.py:312-352)
 *
 * One descriptor per Kronecker factor.  X is never materialised: it is the implicit im2col of
 * `src` (the reference's F.unfold at :329-330, rows ordered (c, kh, kw), columns (n, oh, ow)) plus,
 * when `has_bias`, the row of ones the reference concatenates at :333-335.
 *   A-side of Conv2d : src = layer input  (N,C,H,W), kernel/stride/padding of the layer,
 *                      scale = 1/(N*Ho*Wo)
 *   G-side of Conv2d : src = grad_output  (N,Cout,Ho,Wo) with kh=kw=1, stride 1, padding 0,
 *                      has_bias = 0, scale = N/(Ho*Wo)   (the reference scales grad_output by N
 *                      in its backward hook, :310, and divides by N*Ho*Wo at :343)
 *   Linear           : src = (N,C) viewed as (N,C,1,1); A: scale = 1/N, G: scale = N
 * `dst` is the (dim x dim) fp32 factor, dim = C*kh*kw + has_bias.  `first` != 0 overwrites dst
 * (the reference's `self.state[layer] = [...]` at :350), 0 accumulates (`+=` at :347-348).
 * The result is exactly symmetric.  Dilation is not representable here (the reference ignores it, :329): the A factor of
 * a dilated convolution is built by curv_kfac_dilated_accumulate below.  Grouped convolutions have a build of their own,
 * curv_kfac_group_accumulate below.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_factor_desc {
  const float* src;
  float* dst;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t has_bias;
  int32_t first;
  float scale;
  int32_t path_hint;   /* 0: the library picks the launch form from the launch's own size; CURV_PATH_SMALL / CURV_PATH_GROUPED:
                        * the caller says which form the UNSHARDED model's launch takes, so that a layer-sharded rank
                        * (whose share may fall under the small-launch threshold) sums every factor in the same order as
                        * the unsharded run.  All descriptors of a call carry the same value. */
} curv_factor_desc;
#define CURV_PATH_AUTO 0
#define CURV_PATH_SMALL 1
#define CURV_PATH_GROUPED 2
/* executed multiply-add flops (32 x 32 blocks on and above the diagonal, 2 * 1024 * pairs * K per factor) up to which a
 * launch takes the two-launch small form (csrc/syrk_small.hip) */
#define CURV_SMALL_MAX_FLOP 2.0e9

/* Host-only: the launch form (CURV_PATH_SMALL or CURV_PATH_GROUPED) a curv_kfac_accumulate call with exactly these
 * factors takes on its own - every gate of the small form (executed flops, number of factors, slice length, workgroup
 * count) evaluated by the library itself; `src` / `dst` are not read and any path_hint in `descs` is ignored.  A
 * layer-sharded caller passes the geometry of ALL factors of the model once and puts the answer into the path_hint
 * of its own share's descriptors (curvature/curvatures.py:20-21: layers are independent, so a rank's results must not
 * depend on what else the rank holds). */
int curv_kfac_path_for(const curv_factor_desc* descs, int n_factors);

/* Device scratch needed by curv_kfac_accumulate for this set of factors (bytes). */
size_t curv_kfac_workspace_bytes(const curv_factor_desc* descs, int n_factors);

/* Host-only introspection of the launch plan (tests, tuning): writes CURV_PLAN_INFO_FIELDS values per
 * factor: dim, Ho, Wo, chunk samples, chunk rows, chunk cols, n_chunks, LDS row stride, plane stride,
 * sample stride, channels per panel, n_tiles, chunks per item, k-slices, n_items, item_base, tile edge,
 * float4 staging flag, log2 padded patch row length, 64x64 sub-tiles of the reduce pass (0 for an unsliced factor), the number
 * of serial segments an UNSLICED 128x128-tile factor cuts its K range into (0: k-sliced through slabs; > 0: its items scale,
 * add into dst and write the mirror tile themselves, flushing their accumulators behind every segment), log2 row lanes
 * that walk patch rows while staging (the remaining row lanes split channels), 1 if the patch images are staged
 * by LDS-DMA from a pre-tiled copy of the source (full-width chunks of a kh x kw > 1 convolution), 1 if the factor is built by the LDS-DMA kernel for flattened per-pixel
 * factors (its own work list: item bases count from 0 per kernel; n_chunks = stages of <= 16 pixels), 2 if it is a
 * 3x3 / stride 1 / padding 1 factor assembled from 29 shifted correlations that run as virtual factors of the LDS-DMA
 * kernel (no items of its own; C a multiple of 128: one virtual factor per correlation, C = 64: ten packed pair tiles that
 * hold four correlations each), and last the multiply-add FLOPs (2 per multiply-add) the plan executes for the
 * factor: dim (dim + 1) K for a symmetric product over K = samples x output pixels, the sum over its correlations
 * (C (C + 1) K' for the symmetric ones, 2 C^2 K' for the others) for an assembled factor. */
#define CURV_PLAN_INFO_FIELDS 25
int curv_kfac_plan_info(const curv_factor_desc* descs, int n_factors, long long* out);

/* Grouped build of all factors of a model: a fixed, small number of launches whatever the number of factors (the
 * implicit-im2col kernel, the LDS-DMA kernel for flattened factors, for the shifted correlations of 3x3 / stride 1 /
 * padding 1 factors and for the unfolded copies of stride-2 3x3 / strided 1x1 ones, one reduce launch for each, plus a
 * padding pass and an assembly pass when such 3x3 factors are present and an unfold pass for the strided ones).  A launch that is small as a whole (LeNet scale: at most 2 GFLOP) takes a two-launch build of its own
 * instead (32 x 32 blocks x K slices gathered straight from the tensors, then a reduce pass; path_hint = CURV_PATH_GROUPED
 * keeps such a launch on the grouped kernels).  `descs` is a host array; it may be reused as soon as the call
 * returns.  A factor depends on nothing outside its `src`: the memory around a source may hold any bit pattern, NaN
 * included (every kernel form is tested on sources fenced by NaN).  Two staging forms may still FETCH a few bytes past the
 * end of `src` and discard them: the LDS-DMA kernel for flattened factors in the last 16-byte group of a source whose rows
 * are not a multiple of 4 pixels, and the implicit-im2col kernel in the channel planes of a last panel that ends past C. */
int curv_kfac_accumulate(void* stream, const curv_factor_desc* descs, int n_factors, void* workspace,
                         size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * KFAC factor build of a GROUPED convolution (ABI 11, csrc/group_factor.hip): one Kronecker pair per group.
 *
 * A Conv2d with `groups` = G is G independent convolutions on channel slices; its block-diagonal KFAC stacks G
 * factors: dst is a contiguous (G, n_g, n_g) fp32 tensor, n_g = cg kh kw + has_bias with cg = C / G, and
 *   dst[g] (+)= scale * X_g X_g^T
 * where X_g is the implicit im2col (rows (c, kh, kw), columns (n, oh, ow)) of input-channel slice [g cg, (g + 1) cg)
 * of `src` (N, C, H, W) - C is the TOTAL channel count - plus the row of ones when `has_bias`: exactly what
 * curv_kfac_accumulate computes for a Conv2d(cg, ., kernel, stride, padding) fed that slice.  The G side is the same
 * entry with kh = kw = 1, stride 1, padding 0, src = grad_output (N, C_out, Ho, Wo), has_bias = 0.
 * `scale`, `first`: as for curv_factor_desc.  Dilation is not representable.
 * Deterministic: fixed-order sums, no atomics, and every launch parameter of a factor follows from its own geometry,
 * so its bits do not depend on the other factors of the call.  Never reads outside `src`; enqueues on `stream` only
 * and never waits on the host (graph capture works).
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_group_factor_desc {
  const float* src;
  float* dst;
  int32_t N, C, H, W;
  int32_t groups, kh, kw, sh, sw, ph, pw;
  int32_t has_bias;
  int32_t first;
  float scale;
} curv_group_factor_desc;

/* Device scratch needed by curv_kfac_group_accumulate for these factors (bytes); 0 with the error text set for an
 * invalid geometry.  Host only: src / dst are not read. */
size_t curv_kfac_group_workspace_bytes(const curv_group_factor_desc* descs, int n_factors);

/* Host only: the multiply-add FLOPs (2 per multiply-add) the plan executes per factor, written to out[0 .. n_factors)
 * (sharding cost model, tools).  Narrow groups (cg kh kw <= 16): (P (P + 1) / 2 + P) K G x 2 with P = cg kh kw and
 * K = N Ho Wo; wide groups: the sum over the groups of what curv_kfac_plan_info reports for each group's own factor. */
int curv_kfac_group_plan_flops(const curv_group_factor_desc* descs, int n_factors, long long* out);

/* The build.  Narrow groups: a Gram pass per patch size (one thread holds the group's whole lower triangle) over slices
 * of output pixels, then one reduce pass that sums the slices in order, adds the bias row and
 * corner, scales, writes or adds dst and mirrors the upper triangle.  Wide groups (cg kh kw > 16): a group-major copy
 * of src in the workspace, then one curv_kfac_accumulate call per factor with one descriptor per group (its plan
 * depends on that factor alone).  The workspace must be 256-byte aligned.  `descs` is a host array. */
int curv_kfac_group_accumulate(void* stream, const curv_group_factor_desc* descs, int n_factors, void* workspace,
                               size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * KFAC factor build from bf16 / fp16 sources (ABI 12, csrc/kfac_half.hip): what torch.autocast hands the hooks.
 *
 * Semantics are exactly those of curv_factor_desc: dst (+)= scale * X X^T with X the implicit im2col of `src` (rows
 * (c, kh, kw), columns (n, oh, ow)) plus the row of ones when `has_bias`; `first` != 0 overwrites dst.  `src` is a
 * contiguous (N, C, H, W) or (N, C) tensor of `dtype` (CURV_DTYPE_BF16 / CURV_DTYPE_F16), `dst` the fp32 dim x dim
 * factor.  A bf16 x bf16 or fp16 x fp16 product is exact in fp32, so the v_mfma_f32_32x32x16_bf16 / _f16 build with fp32
 * accumulation computes what the fp32 build computes on the upcast source, up to the order of the sums.
 * Each factor's X is packed into the workspace (K-contiguous rows, zero padded to 128 rows and 16 columns), every
 * 128 x 128 tile on or above the diagonal of every K slice is one MFMA work item writing an fp32 slab, and a fixed-order
 * reduce scales, writes or adds dst and its mirror.  The result is exactly symmetric and bitwise reproducible; the plan
 * of a factor follows from its own descriptor, so its bits never depend on the other factors of the call (no path hint).
 * Never reads outside `src`; enqueues on `stream` only, never waits on the host and allocates nothing (graph capture
 * works).  An empty call is a no-op.  Dilation and groups are not representable.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_DTYPE_F32 0   /* (curv_persample_pack_ex only: curv_kfac16_accumulate builds half-precision factors) */
#define CURV_DTYPE_BF16 1
#define CURV_DTYPE_F16 2
typedef struct curv_factor16_desc {
  const void* src;
  float* dst;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t has_bias;
  int32_t first;
  float scale;
  int32_t dtype;
} curv_factor16_desc;

/* Device scratch needed by curv_kfac16_accumulate for these factors (bytes: the packed X of each factor and its slabs);
 * 0 with the error text set for an invalid geometry or an unknown dtype.  Host only: src / dst are not read. */
size_t curv_kfac16_workspace_bytes(const curv_factor16_desc* descs, int n_factors);

/* Host only: the FLOPs (2 per multiply-add) the plan executes per factor, written to out[0 .. n_factors):
 * 2 x 128^2 x (tiles on and above the diagonal) x K padded to 16 - at least dim (dim + 1) K. */
int curv_kfac16_plan_flops(const curv_factor16_desc* descs, int n_factors, long long* out);

/* The build: a pack, an MFMA and a reduce launch per batch of up to 16 factors of one dtype.  The workspace must be
 * 256-byte aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_kfac16_accumulate(void* stream, const curv_factor16_desc* descs, int n_factors, void* workspace,
                           size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * KFAC A-factor build of a ConvTranspose2d (csrc/convt_factor.hip; groups 1, dilation 1):
 *   dst (+)= scale * sum_o a(o) a(o)^T
 * over the N Ho Wo output pixels o, with a(o)[ci kh kw + a kw + b] = src[n, ci, (oh + ph - a) / sh, (ow + pw - b) / sw]
 * where both quotients are whole numbers inside the input and 0 otherwise, plus a trailing 1 when `has_bias`.  This is
 * the layer matrix Wm = weight.permute(1, 0, 2, 3).reshape(Cout, -1) [| bias] of the layer: dim = C kh kw + has_bias.
 * `src` is the contiguous fp32 (N, C, H, W) layer input; Ho, Wo the spatial size of the layer's OUTPUT (it carries the
 * effective output_padding: (H - 1) sh - 2 ph + kh <= Ho < that + sh).  `scale`, `first` as for curv_factor_desc; the
 * G side of such a layer is an ordinary 1x1 factor of grad_output (curv_kfac_accumulate / curv_kfac16_accumulate).
 *
 * Output pixels split into sh sw phases by ((oh + ph) mod sh, (ow + pw) mod sw); phase r sees only the taps = r
 * (mod stride), as a stride-1 correlation of the original input.  So A is a sum of phase Grams on disjoint tap sets: every
 * entry between taps of different residues is exactly 0.0.  Each phase is built by curv_kfac_accumulate (one call per
 * factor, so its bits depend on its own geometry only): straight from `src` when the phase is a symmetrically padded
 * correlation of it (every phase of kernel == stride, padding 0, the single phase of stride 1; equal phases are built
 * once), otherwise from a zero-bordered window copy of `src` in the workspace.  An assembly pass scatters the phase Grams
 * to their taps, writes exact zeros elsewhere, sets the bias corner to N Ho Wo, scales, writes or adds dst and mirrors
 * it: the result is exactly symmetric.  sh sw <= CURV_CONVT_MAX_PHASES.
 * Never reads outside `src`; deterministic; enqueues on `stream` only, never waits on the host and allocates nothing
 * (graph capture works).  An empty call is a no-op; invalid geometry returns CURV_ERR_INVALID with text.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_CONVT_MAX_PHASES 64
typedef struct curv_convt_factor_desc {
  const float* src;
  float* dst;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t Ho, Wo;
  int32_t has_bias;
  int32_t first;
  float scale;
} curv_convt_factor_desc;

/* Device scratch needed by curv_kfac_convt_accumulate for these factors (bytes; 0 with error text for invalid geometry). */
size_t curv_kfac_convt_workspace_bytes(const curv_convt_factor_desc* descs, int n_factors);

/* Host-only: multiply-add flops (2 per multiply-add) the build executes per factor: the sum of what curv_kfac_plan_info
 * reports for the phase Grams it runs (a dense im2col build of the same factor executes dim (dim + 1) N Ho Wo). */
int curv_kfac_convt_plan_flops(const curv_convt_factor_desc* descs, int n_factors, long long* out);

/* The build of all factors, one after another on `stream`.  `workspace`: curv_kfac_convt_workspace_bytes, 256-byte
 * aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_kfac_convt_accumulate(void* stream, const curv_convt_factor_desc* descs, int n_factors, void* workspace,
                               size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * KFAC A-factor build of a DILATED Conv2d (csrc/dilated_factor.hip; groups 1, stride 1, padding a multiple of the dilation):
 *   dst (+)= scale * X X^T,  X the im2col of `src` with dilation: row (c, a, b) at column (n, oh, ow) is
 *   src[n, c, oh - ph + a dh, ow - pw + b dw] (0 outside the input), plus the row of ones when `has_bias` -
 * F.unfold(src, kernel, dilation, padding, stride 1), which the reference does not compute (it drops the dilation, :329).
 * The descriptor has the fields of curv_factor_desc (without the path hint: a factor's plan is its own) plus dh, dw.
 *
 * All taps of an output pixel lie in one residue class of the input grid modulo (dh, dw), so X is the union over the dh dw
 * classes of the undilated im2col (same kernel, stride 1, padding (ph / dh, pw / dw)) of the sub-images
 * src[:, :, rh::dh, rw::dw], and the factor the sum of their plain factors.  A gather pass reads `src` once and writes the
 * sub-images into the workspace, the classes of equal size stacked as one (count N, C, Hg, Wg) tensor - at most 2 x 2 sizes,
 * one when dh | H and dw | W; curv_kfac_accumulate then runs once per size group, in sequence on `stream`.  A class with an
 * empty sub-image (dilation larger than the image) adds scale * N * (its output pixels) to the bias corner and nothing
 * else.  With dh = dw = 1 the call is curv_kfac_accumulate on `src` itself (any stride and padding, no copy, the same bits).
 * The result is exactly symmetric; sums run in a fixed order without atomics; a factor's launch plan follows from its own
 * geometry, so its bits do not depend on the other factors of the call.  Never reads outside `src`; enqueues on `stream`
 * only, never waits on the host and allocates nothing (graph capture works).  An empty call is a no-op.
 * CURV_ERR_INVALID with the factor named, before anything is launched: dh or dw below 1; with a dilation above 1 a stride
 * other than 1, ph % dh != 0 or pw % dw != 0, a dilated kernel (k - 1) d + 1 larger than the padded input; and the size
 * limits of the plain build, applied to the class stacks.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_dilated_factor_desc {
  const float* src;
  float* dst;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t has_bias;
  int32_t first;
  float scale;
  int32_t dh, dw;
} curv_dilated_factor_desc;

/* Device scratch needed by curv_kfac_dilated_accumulate for these factors (bytes): the SUM over the factors of the scratch
 * each needs alone (its class stacks plus the scratch of its plain builds); 0 with error text for invalid geometry. */
size_t curv_kfac_dilated_workspace_bytes(const curv_dilated_factor_desc* descs, int n_factors);

/* Host-only: multiply-add flops (2 per multiply-add) the build executes per factor: the sum of what curv_kfac_plan_info
 * reports for the plain builds of its class stacks (dh = dw = 1: for the factor itself). */
int curv_kfac_dilated_plan_flops(const curv_dilated_factor_desc* descs, int n_factors, long long* out);

/* The build of all factors, one after another on `stream`.  `workspace`: curv_kfac_dilated_workspace_bytes, 256-byte
 * aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_kfac_dilated_accumulate(void* stream, const curv_dilated_factor_desc* descs, int n_factors, void* workspace,
                                 size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * KFAC A-factor build of a Conv3d (csrc/conv3d_factor.hip; groups 1, dilation 1):
 *   dst (+)= scale * X X^T,  X the 3-D im2col of `src` (N, C, D, H, W): row (c, a, b, e) at column (n, od, oh, ow) is
 *   src[n, c, od sd - pd + a, oh sh - ph + b, ow sw - pw + e] (0 outside the input), plus the row of ones when `has_bias` -
 * the rows in the order of weight.reshape(Cout, -1).  dim = C kd kh kw + has_bias.
 *
 * X is the 2-D im2col - kernel (kh, kw), stride (sh, sw), padding (ph, pw) - of the depth-unfolded stack
 *   x'[(n Do + d), (c kd + a), h, w] = src[n, c, d sd + a - pd, h, w]   (0 where the depth index is outside [0, D)),
 * Do = (D + 2 pd - kd) / sd + 1, column for column.  A gather pass reads `src` once and writes the contiguous
 * (N Do, C kd, H, W) stack into the workspace, whole H W planes at a time (a source plane goes to at most ceil(kd / sd)
 * places; the planes that are padding are written with zeros, the workspace is never assumed clean); curv_kfac_accumulate
 * then runs once for the stack, with every fast path it has for C kd channels.  One call per factor: a factor's launch
 * plan follows from its own geometry, so its bits do not depend on the other factors of the call; they are those of
 * curv_kfac_accumulate on the stack.  The result is exactly symmetric; no atomics.  `src` may be only 4-byte aligned.
 * Never reads outside `src`; enqueues on `stream` only, never waits on the host and allocates nothing (graph capture
 * works).  An empty call is a no-op.
 * CURV_ERR_INVALID with the factor named, before anything is launched: a size below 1, negative padding, a kernel larger
 * than the padded input; 2^31 or more source planes, samples or channels of the stack, or floats in one plane or in one
 * sample of the stack; and the limits of the plain build, applied to the stack (its text follows this build's).
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_conv3d_factor_desc {
  const float* src;
  float* dst;
  int32_t N, C, D, H, W;
  int32_t kd, kh, kw, sd, sh, sw, pd, ph, pw;
  int32_t has_bias;
  int32_t first;
  float scale;
} curv_conv3d_factor_desc;

/* Device scratch needed by curv_kfac_conv3d_accumulate for these factors (bytes): the SUM over the factors of the scratch
 * each needs alone (its stack plus the scratch of its plain build); 0 with error text for invalid geometry. */
size_t curv_kfac_conv3d_workspace_bytes(const curv_conv3d_factor_desc* descs, int n_factors);

/* Host-only: multiply-add flops (2 per multiply-add) the build executes per factor: what curv_kfac_plan_info reports for
 * the plain build of its stack. */
int curv_kfac_conv3d_plan_flops(const curv_conv3d_factor_desc* descs, int n_factors, long long* out);

/* The build of all factors, one after another on `stream`.  `workspace`: curv_kfac_conv3d_workspace_bytes, 256-byte
 * aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_kfac_conv3d_accumulate(void* stream, const curv_conv3d_factor_desc* descs, int n_factors, void* workspace,
                                size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * KFAC-reduce factor build (csrc/reduce_factor.hip): the shared positions of a weight-sharing layer are reduced first and
 * the Gram runs over the N samples only (Eschenhagen et al., NeurIPS 2023):
 *   dst (+)= scale * R R^T,  R the (N, dim) matrix of per-sample rows [plus the column of ones when `has_bias`].
 * `form` = CURV_REDUCE_PLANE: `src` is a contiguous (N, C, H, W) tensor of `dtype`, dim = C kh kw and
 *   row[n, (c, a, b)] = m * sum over the Ho x Wo output pixels (oh, ow) of xpad[n, c, oh sh + a - ph, ow sw + b - pw],
 * the row mean (m = 1 / (Ho Wo), `mean` = 1) or row sum (m = 1, `mean` = 0) of F.unfold(src, kernel, padding, stride) over
 * its columns, without the im2col matrix: the padding adds zeros, a tap that sees padding only gives 0.  The A side of a
 * Conv2d is this with `mean` = 1, its G side the grad_output with kh = kw = 1, stride 1, padding 0 and `mean` = 0.
 * `form` = CURV_REDUCE_TOKEN: `src` is a contiguous (N, T, E) tensor, dim = E and row[n, e] = m * sum_t src[n, t, e] with
 * m = 1 / T or 1 (C, H, W and the window are not read): the two sides of a Linear layer applied to T tokens per sample.
 * `dtype`: CURV_DTYPE_F32, CURV_DTYPE_BF16 or CURV_DTYPE_F16; half values are upcast exactly and summed in fp32.
 *
 * Per factor: one reduce pass reads `src` once and writes the rows (fp32, contiguous, 256-byte aligned) into the workspace,
 * then ONE curv_kfac_accumulate call builds the factor from them as an (N, dim) flat source (CURV_PATH_AUTO; `has_bias`,
 * `scale`, `first` passed through).  No float atomics: every row entry is summed by one workgroup in an order that follows
 * from the factor's own geometry, so the result is bitwise reproducible and independent of the other factors of the call;
 * it is exactly symmetric.  Never reads outside `src`; enqueues on `stream` only, never waits on the host and allocates
 * nothing (graph capture works).  An empty call is a no-op.
 * CURV_ERR_INVALID with the factor named, before anything is launched: unknown dtype or form; sizes below 1, a stride below
 * 1 or a negative padding; a kernel larger than the padded input (no output pixel); dim above 2^20; 2^31 or more planes
 * (N C) or token rows (N T); a window wider than 4096 taps; and whatever curv_kfac_accumulate refuses for the row matrix.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_REDUCE_PLANE 0
#define CURV_REDUCE_TOKEN 1
typedef struct curv_reduce_factor_desc {
  const void* src;
  float* dst;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t has_bias;
  int32_t first;
  float scale;
  int32_t dtype;           /* CURV_DTYPE_* */
  int32_t form;            /* CURV_REDUCE_* */
  int32_t mean;            /* 1: the row is divided by the number of positions, 0: it is their sum */
  int32_t T, E;            /* token form: positions per sample, features */
} curv_reduce_factor_desc;

/* Device scratch needed by curv_kfac_reduce_accumulate for these factors (bytes): the SUM over the factors of the rows of
 * each plus the scratch of its build; 0 with error text for an invalid descriptor.  Host only: src / dst are not read. */
size_t curv_kfac_reduce_workspace_bytes(const curv_reduce_factor_desc* descs, int n_factors);

/* Host-only: per factor the additions of the reduce pass (plane form N C (H W kw + H kh kw), token form N T E) plus the
 * multiply-add flops curv_kfac_plan_info reports for the build of its row matrix. */
int curv_kfac_reduce_plan_flops(const curv_reduce_factor_desc* descs, int n_factors, long long* out);

/* The build of all factors, one after another on `stream`.  `workspace`: curv_kfac_reduce_workspace_bytes, 256-byte
 * aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_kfac_reduce_accumulate(void* stream, const curv_reduce_factor_desc* descs, int n_factors, void* workspace,
                                size_t workspace_bytes);

/* Same, recording HIP events (from curv_event_create) on `stream` around EVERYTHING the call enqueues behind the
 * descriptor-table uploads (padding / pre-tiling passes, the MFMA kernels, the k-slice reductions, the 3x3 assembly), so
 * that a benchmark can time the whole build without a profiler. */
int curv_kfac_accumulate_timed(void* stream, const curv_factor_desc* descs, int n_factors, void* workspace,
                               size_t workspace_bytes, void* ev_start, void* ev_stop);

/* Same with flags (ev_start / ev_stop may be NULL).  CURV_KFAC_TABLE_RESIDENT: the caller vouches that the head of
 * `workspace` (the device descriptor table) has not been written by anybody else since this thread's previous
 * curv_kfac_accumulate* call with the same workspace; argument blocks of the table that did not change (same
 * pointers, geometry, scale and `first` flags - the steady state of a training loop) are then not uploaded again. */
#define CURV_KFAC_TABLE_RESIDENT 1u
int curv_kfac_accumulate_ex(void* stream, const curv_factor_desc* descs, int n_factors, void* workspace,
                            size_t workspace_bytes, unsigned flags, void* ev_start, void* ev_stop);
void* curv_event_create(void);
void curv_event_destroy(void* event);
int curv_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* waits for ev_stop */
int curv_event_synchronize(void* event);                                /* blocks the host until the event has fired */

/* ------------------------------------------------------------------------------------------------
 * KFAC.invert:  L = lower Cholesky factor of (sqrt(multiply) * F + sqrt(add) * I)^-1
 *                                                                (curvature/curvatures.py:354-385)
 * One descriptor per Kronecker factor; all factors of a model are processed by one batched sweep.
 * F is the (n x n) fp32 factor (read only), L the (n x n) fp32 output (zeros above the diagonal, as
 * torch's cholesky returns).  The damped matrix is formed in fp32 exactly as the reference does
 * (:368-375); the factorisation itself runs in fp64.  info[i] (device int32) is 0 on success and
 * 1 + the index of the failing pivot when factor i is not positive definite, in which case L holds
 * garbage: the caller raises the reference's RuntimeError (:380, scripts/hyper.py:141).  The index
 * counts in the order of the sweep, which factorises the index-REVERSED damped factor J (.) J: word w
 * names row n - w of F (what LAPACK reports for J (.) J, not for the factor as given;
 * tests/test_chol_factor_inverse_gpu.py).
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_inv_desc {
  const float* F;
  float* L;
  int32_t n;
  int32_t reserved;
  double add;       /* n of the reference: sqrt(add) goes on the diagonal   */
  double multiply;  /* s of the reference: the factor is scaled by sqrt(s)   */
} curv_inv_desc;

size_t curv_chol_inv_workspace_bytes(const curv_inv_desc* descs, int n_factors);
/* A factor may be up to 2^21 wide (wider: CURV_ERR_INVALID); the work matrices are addressed with 64-bit offsets. */
int curv_chol_inv_lower(void* stream, const curv_inv_desc* descs, int n_factors, int* info, void* workspace,
                        size_t workspace_bytes);
/* The same call with an EARLY verdict for a host that must raise on "not positive definite" before it goes on (the
 * reference's invert() raises from torch.cholesky, curvatures.py:378-380): the n status words are also copied to
 * `host_status` (PINNED host memory, n ints) by an internal stream as soon as the last factorisation step of every factor
 * has run - before the finalize passes that write L, which do not touch them - and `ev_status` (curv_event_create) is
 * recorded behind that copy.  curv_event_synchronize(ev_status) then returns while the finalize passes still run (0.15 ms
 * for a ResNet-50), and the host prepares its next launches in their shadow; work enqueued on `stream` afterwards is
 * ordered behind the whole call as always.  Not available under stream capture (CURV_ERR_INVALID).
 * The call itself WAITS (host) for that copy before it makes `stream` wait for the sweep and returns (the status words are
 * then in `host_status`; curv_event_synchronize(ev_status) returns at once): a stream that sits on an unsatisfied wait for
 * the whole sweep slows the sweep's own streams down whenever they share a pipe of the command processor with it - the
 * "streams created before the estimator" effect (10.9 -> 7.3 ms for a ResNet-50).  curv_chol_inv_lower, which never
 * blocks the host, keeps that sensitivity. */
int curv_chol_inv_lower_status(void* stream, const curv_inv_desc* descs, int n_factors, int* info, void* workspace,
                               size_t workspace_bytes, int* host_status, void* ev_status);

/* X = chol_lower(M + diag_add * I)^-1 in fp64 for a batch of symmetric fp32 matrices (same blocked sweep,
 * no index reversal; M may also be given in fp64): the A_c^-1 and B_c^-1 of INF.pre_sampler (curvatures.py:566-567).  X is (n x n)
 * fp64, lower triangular with zeros above.  info as for curv_chol_inv_lower. */
typedef struct curv_cholinv_desc {
  const void* M;     /* fp32 matrix, or fp64 when m_is_f64 != 0 (diag_add is then added in fp64) */
  double* X;
  int32_t n;
  int32_t m_is_f64;
  double diag_add;
  /* optional (NULL: X = chol(M + d I)^-1 as above).  Non-NULL: RIGHT-HAND SIDE mode - R is an (n x n) fp64 lower-triangular
   * matrix and X receives chol(M + d I)^-1 R (lower triangular): the forward substitution runs inside the sweep, in the place
   * of the inverse accumulation and at its cost, and saves the explicit inverse's product with R afterwards
   * (INF.pre_sampler's B_c^-1 A_c^-1, :566-570).  Needs a third work matrix (curv_chol_factor_inverse_workspace_bytes). */
  const double* R;
  int32_t r_minus;   /* with R: X = R - chol(M + d I)^-1 R (pre_sampler's T = (I - B_c^-1) A_c^-1 in one go) */
  int32_t reserved;
  double pivot_min;  /* a pivot <= pivot_min counts as "not positive definite" (0: the plain test).  info then reports the first
                      * column whose pivot fell to the threshold, i.e. the numerical rank of a Gram matrix whose columns are
                      * in general position: the rank detection of the low-rank eigensolver (curvature_amd/ops.py: eigh) */
} curv_cholinv_desc;

size_t curv_chol_factor_inverse_workspace_bytes(const curv_cholinv_desc* descs, int n_mats);
int curv_chol_factor_inverse(void* stream, const curv_cholinv_desc* descs, int n_mats, int* info, void* workspace,
                             size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * Dense contractions of the samplers and of EFB / INF: a batch of independent strided fp32 GEMMs
 *     C = epilogue(alpha * op(A) op(B)) [+ beta * C]
 * op(A) is M x K with element (i,k) at A[i*a_rs + k*a_cs]; op(B) is K x N with (k,j) at
 * B[k*b_rs + j*b_cs]; C is M x N with (i,j) at C[i*c_rs + j*c_cs] (strides in elements, so transposes
 * and column slices need no copies).  Epilogues: NONE; SQUARE (alpha*acc^2, EFB.update's (.)**2 at
 * curvatures.py:427); MUL_E / ADD_E (multiply by / add an elementwise operand E, used for the
 * lambda scaling of EFB.sample :458 and for writing mean + sample straight into a parameter, :67-82).
 * ---------------------------------------------------------------------------------------------- */
#define CURV_EPI_NONE 0
#define CURV_EPI_SQUARE 1
#define CURV_EPI_MUL_E 2
#define CURV_EPI_ADD_E 3
#define CURV_EPI_MUL_E_ADD_F 4   /* alpha*acc*E + F: INF.sampler's Y_l - r^2 * X_p_s written onto the mean (:596-599) */
/* triangular-operand hints: the K range of every output tile is cut where the operand is known to be 0 */
#define CURV_TRI_NONE 0
#define CURV_TRI_A_LOWER 1   /* op(A)(i,k) = 0 for k > i  (e.g. A = L_G) */
#define CURV_TRI_B_UPPER 2   /* op(B)(k,j) = 0 for k > j  (e.g. B = L_A^T) */

typedef struct curv_gemm_desc {
  const float* A;
  const float* B;
  float* C;
  const float* E;
  long long a_rs, a_cs, b_rs, b_cs, c_rs, c_cs, e_rs, e_cs;
  int32_t M, N, K;
  int32_t epilogue;
  float alpha, beta;
  int32_t tri;
  int32_t reserved;
  const float* F;          /* second elementwise operand (CURV_EPI_MUL_E_ADD_F), else NULL */
  long long f_rs, f_cs;
} curv_gemm_desc;

size_t curv_gemm_workspace_bytes(int n_desc);
/* The same plus room for K slicing: when a call holds fewer output tiles of K-contiguous products than the chip has
 * workgroup slots (a layer-sharded rank sampling one wide layer), products with K >= 1536 are cut into K slices whose
 * partial tiles are summed in a fixed order by a second launch.  With a workspace of only
 * curv_gemm_workspace_bytes the call still works, unsliced. */
size_t curv_gemm_workspace_bytes_for(const curv_gemm_desc* descs, int n_desc);
int curv_gemm_batched(void* stream, const curv_gemm_desc* descs, int n_desc, void* workspace,
                      size_t workspace_bytes);
/* The same with flags.  CURV_GEMM_TABLE_RESIDENT: this exact descriptor array was the previous call's on this
 * workspace and nobody else has written to the workspace since (a launch plan that owns its scratch and replays a fixed
 * list of products): the device copy of the table is not uploaded again. */
#define CURV_GEMM_TABLE_RESIDENT 1u
int curv_gemm_batched_ex(void* stream, const curv_gemm_desc* descs, int n_desc, void* workspace,
                         size_t workspace_bytes, unsigned flags);
/* Host only: what curv_gemm_batched would launch for these descriptors on a workspace of this many bytes; no pointer is
 * dereferenced and nothing runs on the device.  It goes through the launch's own validation and classification, so it
 * returns the launch's refusals with their messages.  out[0 .. CURV_GEMM_PLAN_FIELDS):
 *   0  64 x 64 tiles of the general kernel            4  workgroups of the reduce launch (tiles of split products)
 *   1  128 x 128 tiles of the general kernel          5  32 x 32 blocks of the small-launch kernel
 *   2  items of the NT kernel (tiles x K slices)      6  workgroups of the one-column (gemv) kernel
 *   3  K-sliced products                              7  entries of the K-sorted tile order list (0: not used) */
#define CURV_GEMM_PLAN_FIELDS 8
int curv_gemm_plan_info(const curv_gemm_desc* descs, int n_desc, size_t workspace_bytes, long long* out);

/* fp64 variant (alpha/beta only) for the ill-conditioned products of INF.pre_sampler.  `tri`: triangular operands -
 * entries outside the triangle are neither read nor multiplied (they must be zero in memory where a tile straddles the
 * diagonal): the products of the two triangular inverses of pre_sampler (curvatures.py:566-572) are 2/3 of INF.invert's
 * flops when done densely.  A lower x B lower leaves the tiles above the diagonal of C untouched for beta = 1 and
 * zero for beta = 0.  The products of one call are INDEPENDENT (no C of one may be an operand of another): they run
 * up to 24 to a launch, products with both output edges >= 1024 on 128 x 128 tiles in a launch of their own behind the
 * others - not in the caller's order. */
#define CURV_TRI64_A_LOWER 1
#define CURV_TRI64_A_UPPER 2
#define CURV_TRI64_B_LOWER 4
#define CURV_TRI64_B_UPPER 8
#define CURV_TRI64_C_LOWER 16 /* square product known to be symmetric: tiles strictly above the diagonal are not computed
                                 * (their part of C is left untouched; elements above the diagonal inside diagonal tiles are written) */
typedef struct curv_gemm64_desc {
  const double* A;
  const double* B;
  double* C;
  long long a_rs, a_cs, b_rs, b_cs, c_rs, c_cs;
  int32_t M, N, K;
  int32_t tri;      /* CURV_TRI64_* flags, 0 = dense */
  double alpha, beta;
  /* optional fused epilogues (all NULL: C = alpha * acc + beta * C as above):
   *   E          C = alpha * acc + beta * E with E != C (same strides as C): T = A^-1 - B^-1 A^-1 of INF.pre_sampler
   *              without a copy of A^-1 first; tiles whose K range is empty are still written (beta * E)
   *   C32        fp32 output instead of C (C may be NULL; strides c_rs / c_cs count floats; beta must be 0):
   *              C32[i][j] = (float)(alpha * row_scale[i] * col_scale[j] * acc), either scale vector may be NULL (= 1):
   *              P_c = diag(sigma) L_c diag(sigma) of pre_sampler (:570) straight from the product */
  const double* E;
  const float* row_scale;
  const float* col_scale;
  float* C32;
} curv_gemm64_desc;
int curv_gemm_f64_batched(void* stream, const curv_gemm64_desc* descs, int n_desc);

/* out[0..count) ~ N(0,1): Philox4x32-10 keyed by `seed`, counter starting at `offset` (in units of 4
 * values); the draw of torch.randn at curvatures.py:391, :457, :590 with a device-side generator. */
int curv_randn(void* stream, float* out, long long count, unsigned long long seed, unsigned long long offset);
/* The same stream with its position kept on the DEVICE: the draw starts at *counter (units of 4 values) and a second
 * launch advances *counter by ceil(count / 4).  A captured HIP graph that contains the call therefore draws fresh
 * noise at every replay (a host-side offset would be frozen into the kernel arguments). */
int curv_randn_counter(void* stream, float* out, long long count, unsigned long long seed, unsigned long long* counter);

/* ------------------------------------------------------------------------------------------------
 * Elementwise pieces (Diagonal / EFB / INF)
 * ---------------------------------------------------------------------------------------------- */
/* out = (s*v + n)^(-1/2)     curvatures.py:188 (Diagonal.invert), :449 (EFB.invert), :526 (INF) */
int curv_rsqrt_affine(void* stream, const float* v, double s, double n, float* out, long long count);
/* state (+)= batch_size * [grad_w | grad_b]^2   curvatures.py:160-165 (Diagonal), :431-434 (EFB diags)
 * grad_w is (rows x cols_w), grad_b (rows) or NULL; state is (rows x (cols_w + (grad_b != NULL))). */
int curv_sq_accumulate(void* stream, const float* grad_w, const float* grad_b, int rows, int cols_w,
                       double batch_size, float* state, int first);

/* The same for many layers in one launch (Diagonal.update, the `diags` of EFB.update).  first: overwrite `state`
 * instead of adding to it. */
typedef struct curv_sq_desc {
  const float* grad_w;
  const float* grad_b;     /* may be NULL */
  float* state;            /* (rows, cols_w + (grad_b != NULL)) contiguous */
  int32_t rows, cols_w;
  int32_t first, reserved;
} curv_sq_desc;
int curv_sq_accumulate_batched(void* stream, const curv_sq_desc* descs, int n, double batch_size);

/* ------------------------------------------------------------------------------------------------
 * Exact per-sample Fisher for Diagonal and EFB at any batch size (csrc/persample.hip).
 *
 * curvatures.py:152 (Diagonal) and :427-434 (EFB) square the BATCH gradient [W.grad | b.grad] = sum_n P_n, with
 * P_n = g_n X_n^T the share of sample n (g_n: the layer's grad_output of the sample as m x L, X_n: its unfolded input
 * [+ ones row] as n_in x L).  That is the Fisher diagonal only at batch size 1.  These entry points compute the sum of
 * the squares of the P_n themselves,
 *     C[i][j] (+)= alpha * sum_{n < S} ( sum_{l < L} A[n*a_ns + i*a_rs + l] * B[n*b_ns + j*b_rs + l] )**2
 * without ever writing a P_n: Diagonal's state with A = g, B = X; EFB's with A = U_G^T g, B = U_A^T X.
 *
 * A is S segments of M x L, B is S segments of Nc x L, both contiguous along l; segment strides (a_ns, b_ns) and row
 * strides (a_rs, b_rs) are free (in floats; a row stride may be below L only for a single row, a segment stride may be
 * 0), so grad_output (N, m, Ho*Wo) and the input of a 1x1 / stride-1 convolution (N, C, H*W) are read in place, as is
 * a packed copy in (N, rows, Lp) or (rows, N, Lp) order.  C is M x Nc with row stride c_rs >= Nc; `first` != 0
 * overwrites it.  fp32 MFMA with fp32 accumulation; deterministic (fixed-order sums, no atomics); the plan of an item
 * follows from its own sizes only, so its bits do not depend on the other items of the call.  Enqueues on `stream`
 * only, never waits on the host, allocates nothing (graph capture works).  An empty call is a no-op.
 * l values at or behind L never enter a product (memory there may hold anything, NaN included), but the staging
 * fetches whole 16-byte groups: where L is no multiple of 4 it may FETCH up to 12 bytes behind the end of an operand and
 * discard them.  Pack such operands (below) when the bytes behind them may be unmapped.  Operand extents stay below
 * 2^31 bytes (CURV_ERR_INVALID otherwise).
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_persample_desc {
  const float* A;
  const float* B;
  float* C;
  long long a_ns, a_rs, b_ns, b_rs, c_rs;
  int32_t S, M, Nc, L;
  int32_t first;
  float alpha;
} curv_persample_desc;

/* Device scratch needed by curv_persample_sq_accumulate for these items (bytes: one fp32 slab per output tile and range
 * of samples); 0 with the error text set (naming the item) for invalid sizes.  Host only. */
size_t curv_persample_workspace_bytes(const curv_persample_desc* descs, int n);
/* Host only: the multiply-add FLOPs (2 per multiply-add) the plan executes per item, written to out[0 .. n): whole
 * 128 x 128 tiles (64 x 128 where min(M, Nc) <= 64) over L padded to stages of 32 - at least the algorithmic
 * 2 S M Nc L. */
int curv_persample_plan_flops(const curv_persample_desc* descs, int n, long long* out);
/* The products: an MFMA and a reduce launch per batch of up to 16 items.  The workspace must be 256-byte aligned.
 * `descs` is a host array; it may be reused as soon as the call returns. */
int curv_persample_sq_accumulate(void* stream, const curv_persample_desc* descs, int n, void* workspace,
                                 size_t workspace_bytes);

/* The fp32-contiguous spelling of curv_persample_pack_ex below (an adapter over the same planner and kernel: float32,
 * transposed = 0, strides (CHW, HW, W, 1) or with channels_last (HWC, 1, WC, C), src_elems = N*C*H*W; refusals read
 * "curv_persample_pack: item <i>: ..."; beside the messages it always had, a src that is not 4-byte aligned is now
 * refused, "src is not aligned to its 4-byte elements").  X of a layer, l-contiguous, into caller scratch `dst` - wherever the source
 * cannot be read in place:
 *   dst[(n*R + r)*Lp + l]   (rows_outer = 0)   or   dst[(r*N + n)*Lp + l]   (rows_outer != 0: one R x (N Lp) matrix)
 * for r < R = C*kh*kw + has_bias, l < Lp, with L = Ho*Wo: row r = (c, a, b) is the implicit im2col of `src` (the
 * reference's F.unfold, curvatures.py:329-330), the last row the ones of a biased layer (:333-335), and every l in
 * [L, Lp) is written as 0 by the pack itself.  `src` is (N, C, H, W), or with channels_last != 0 (N, H, W, C): the
 * (N, T, D) input of a Linear layer is C = D, H = T, W = 1, i.e. the transpose to D rows of T.  kh = kw = 1, stride 1,
 * padding 0 is a plain copy with a zero tail (grad_output with L = 196 or 49).  Lp >= L, a multiple of 4; dst 16-byte
 * aligned.  Never reads outside `src` (a masked gather reads src[0] and drops it).  Invalid geometry (kh = 0, sh = 0, an
 * empty output) returns CURV_ERR_INVALID with the item named.  An empty call is a no-op. */
typedef struct curv_persample_pack_desc {
  const float* src;
  float* dst;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t has_bias;
  int32_t channels_last;
  int32_t rows_outer;
  int32_t Lp;
} curv_persample_pack_desc;
int curv_persample_pack(void* stream, const curv_persample_pack_desc* descs, int n);

/* The general form of curv_persample_pack: the same destination (layout, ones row, zero tail, fp32, dst 16-byte aligned,
 * Lp a multiple of 4) from a source of three dtypes, read through strides, forward or transposed.
 *   dtype       CURV_DTYPE_F32, CURV_DTYPE_BF16 or CURV_DTYPE_F16: half values are upcast by the pack (bf16 is its bit
 *               pattern shifted up 16 bits, fp16 the exact conversion: inf, NaN, -0 and subnormals survive).  A product
 *               of two bf16 or two fp16 values is exact in fp32, so the fp32 products on the upcast copy compute what a
 *               half-precision kernel with fp32 accumulation would.
 *   s_n .. s_w  source strides in ELEMENTS: element (n, c, h, w) is src[n*s_n + c*s_c + h*s_h + w*s_w].  (N, C, H, W) is
 *               (CHW, HW, W, 1); the (N, T, D) input of a Linear layer is C = D, H = T, W = 1 with (TD, 1, D, -); the
 *               (T, N, E) record of an attention projection is C = E, H = T, W = 1 with (E, 1, NE, -).  Not negative.
 *   src_elems   the extent of the source in elements: the largest addressed offset must lie inside it.  It may be of
 *               any size (s_n is used in 64 bits), but what one sample spans, (C-1)*s_c + (H-1)*s_h + (W-1)*s_w, must be
 *               below 2^31 elements.  Nothing outside it is read (a masked or padded element reads src[0]).
 *   transposed  != 0: X of a ConvTranspose2d with output Ho x Wo (given; within the range output_size allows,
 *               [(H-1)s - 2p + k, (H-1)s - 2p + k + s - 1]): row r = (ci, a, b) at l = (oh, ow) is
 *               x[n, ci, (oh + ph - a)/sh, (ow + pw - b)/sw] where both divisions are exact and the result lies inside
 *               H x W, 0 elsewhere - the column order of Wm = weight.permute(1, 0, 2, 3).reshape(Cout, -1).  L = Ho*Wo.
 *               == 0: the forward im2col of curv_persample_pack; Ho and Wo are not read.
 *   reserved    the DILATION of the forward im2col: dh in the low and dw in the high 16 bits, a half of 0 standing for 1 - so
 *               0, what every caller wrote so far, is dilation 1 and the layout is unchanged (no second entry point).  Row
 *               (c, a, b) at l = (oh, ow) is x[n, c, oh sh - ph + a dh, ow sw - pw + b dw], and L follows from the dilated
 *               output size, (H + 2 ph - (kh - 1) dh - 1) / sh + 1 (w alike); any stride and any padding.  A transposed
 *               item with a dilation other than 1 is refused.
 * A 1x1 / stride-1 / padding-0 item whose rows are plain runs of the source, with the pointer and the sample and channel
 * strides multiples of four elements, is read with one 8- or 16-byte load per four values; everything else gathers per
 * element.  One launch per 16 items of one dtype; an item's bits do not depend on the other items of the call.  Every item
 * is checked before anything is launched: invalid geometry, an unknown dtype, a transposed output size outside its range,
 * Lp, the element limits ("too large") and a source extent smaller than the largest offset return
 * CURV_ERR_INVALID with the item named.  An empty call is a no-op. */
typedef struct curv_persample_pack_ex_desc {
  const void* src;
  float* dst;
  long long s_n, s_c, s_h, s_w;
  long long src_elems;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t Ho, Wo;
  int32_t has_bias;
  int32_t dtype;
  int32_t transposed;
  int32_t rows_outer;
  int32_t Lp;
  int32_t reserved;
} curv_persample_pack_ex_desc;
int curv_persample_pack_ex(void* stream, const curv_persample_pack_ex_desc* descs, int n);

/* curv_persample_pack_ex with a depth window: X of a Conv3d, the 3-D im2col of a record, written per sample (the same
 * planner and kernel; a 2-D item is D = kd = sd = 1, pd = 0).  The destination is that of curv_persample_pack_ex -
 *   dst[(n*R + r)*Lp + l]   (rows_outer = 0)   or   dst[(r*N + n)*Lp + l]   (rows_outer != 0)
 * fp32, dst 16-byte aligned, Lp a multiple of 4 - with R = C*kd*kh*kw + has_bias and L = Do*Ho*Wo: row r = (c, a, b, e) at
 * l = (od, oh, ow) is x[n, c, od*sd - pd + a, oh*sh - ph + b, ow*sw - pw + e], 0 outside the input - the row order of
 * weight.reshape(Cout, -1) -, the last row the ones of a biased layer for l < L, and every l in [L, Lp) is 0.  The source
 * as in the 2-D form: `dtype` fp32 / bf16 / fp16, upcast exactly; element (n, c, d, h, w) is
 * src[n*s_n + c*s_c + d*s_d + h*s_h + w*s_w] (strides in ELEMENTS, not negative; (N, C, D, H, W) contiguous is
 * (CDHW, DHW, HW, W, 1), channels_last_3d (CDHW, 1, HWC, WC, C)); s_n is used in 64 bits, what one sample spans must be
 * below 2^31 elements; nothing outside [src, src + src_elems) is read (a masked or padded element reads src[0] and drops
 * it).  No dilation and no transposed form; `reserved` must be 0.  A 1x1x1 / stride-1 / padding-0 item whose rows are plain
 * runs of the source (s_w == 1 or W == 1, s_h == W or H == 1, s_d == H*W or D == 1), with the pointer and the sample and
 * channel strides multiples of four elements, is read with one 8- or 16-byte load per four values; everything else
 * gathers per element.  Items with a depth window (D, kd or pd other than 1, 1, 0) are launched apart from those without,
 * 16 of one dtype per launch; an item's bits do not depend on the other items of the call.  Every item is checked before
 * anything is launched, sizes before addresses; CURV_ERR_INVALID with "curv_persample_pack3d: item <i>: ..." for an
 * unknown dtype, a nonzero `reserved`, a size below 1, negative padding, a kernel larger than the padded input in any
 * axis, a negative stride or an extent below 1, "too large" (more than 2^24 rows or positions, a sample span or a thread
 * count of 2^31 or more), a bad Lp, a source extent smaller than the largest offset (a size here: it is checked before
 * the addresses), a null or misaligned src or dst.  An empty call is a no-op. */
typedef struct curv_persample_pack3d_desc {
  const void* src;
  float* dst;
  long long s_n, s_c, s_d, s_h, s_w;
  long long src_elems;
  int32_t N, C, D, H, W;
  int32_t kd, kh, kw, sd, sh, sw, pd, ph, pw;
  int32_t has_bias;
  int32_t dtype;
  int32_t rows_outer;
  int32_t Lp;
  int32_t reserved;
} curv_persample_pack3d_desc;
int curv_persample_pack3d(void* stream, const curv_persample_pack3d_desc* descs, int n);

/* ------------------------------------------------------------------------------------------------
 * Per-sample products of true depthwise convolutions (in_channels == out_channels == groups; csrc/persample_dw.hip,
 * DESIGN.md "K14").  Channel c owns row c of [W | b], a 1 x n_g row with n_g = kh*kw + has_bias, and its per-sample
 * gradient is a correlation of two planes, not a matrix product:
 *     p[n, c, a*kw + b] = sum_{oh, ow} g[n, c, oh, ow] * x[n, c, oh*sh + a - ph, ow*sw + b - pw]     (taps outside H x W: 0)
 *     p[n, c, kh*kw]    = sum_{oh, ow} g[n, c, oh, ow]                                               (has_bias != 0)
 * Phase 1 writes p (N*C*n_g floats per item) to the workspace, phase 2 reduces it:
 *     curv_persample_dw_sq_accumulate:  dst[c*c_rs + j]  (+)= alpha * sum_n p[n,c,j]**2
 *     curv_persample_dw_quad_reduce:    out[n*o_stride]  (+)= alpha * sum_c s[c]**2 * sum_j W[c*w_rs + j] *
 *                                                              ( sum_i T[c*t_cs + i*t_rs + j] * p[n,c,i] )**2
 * T, W and s may each be NULL: the identity, all ones, all ones.  Diagonal: W = inv**2; KFAC: T = L_A stacked
 * (C, n_g, n_g), s = L_G stacked (C, 1, 1) - with one output channel per group ||L_G^T P L_A||_F**2 = l_G**2 ||p L_A||**2.
 *
 * One descriptor serves both entry points (each reads its own destination fields).  x is (N, C, H, W) and g is
 * (N, C, Ho, Wo), float32, each read through four strides in ELEMENTS (not negative; any layout, channels_last included)
 * inside an extent x_elems / g_elems counted from the pointer: nothing outside the extents is read (a masked tap reads
 * x[0] of its plane and drops it).  Ho, Wo must be the output size of the geometry; kh*kw <= 49; what one sample spans
 * stays below 2^31 elements.  Plain fp32 VALU arithmetic (the work is HBM-bound), no atomics, sums in a fixed order
 * (lane, wave, workgroup, then planes / samples / channels in index order); how a plane is split among waves follows
 * from its own sizes only, so an item's bits do not depend on the other items of the call.  Up to 16 items per launch.
 * Enqueues on `stream` only, never waits on the host, allocates nothing.  An empty call is a no-op; invalid geometry,
 * strides or extents return CURV_ERR_INVALID with the item named, before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_persample_dw_desc {
  const float* x;
  const float* g;
  long long x_sn, x_sc, x_sh, x_sw, x_elems;
  long long g_sn, g_sc, g_sh, g_sw, g_elems;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t Ho, Wo;
  int32_t has_bias;
  int32_t first;
  float alpha;
  int32_t reserved;
  /* curv_persample_dw_sq_accumulate */
  float* dst;              /* (C, n_g) with row stride c_rs >= n_g */
  long long c_rs;
  /* curv_persample_dw_quad_reduce */
  const float* T;          /* may be NULL */
  const float* Wt;         /* the weights W of the formula; may be NULL */
  const float* s;          /* may be NULL */
  float* out;
  long long t_cs, t_rs, w_rs, o_stride;
} curv_persample_dw_desc;
/* Device scratch for these items (bytes: p of every item, 256-byte aligned each); 0 with the error text set (naming the
 * item) for invalid geometry.  Host only; the pointers are not read. */
size_t curv_persample_dw_workspace_bytes(const curv_persample_dw_desc* descs, int n);
/* Host only: per item the FLOPs of phase 1 (2 N C Ho Wo n_g) into flops[0 .. n) and the bytes the algorithm needs,
 * 4 N C (H W + Ho Wo), into bytes[0 .. n); either array may be NULL. */
int curv_persample_dw_plan_info(const curv_persample_dw_desc* descs, int n, long long* flops, long long* bytes);
/* The workspace must be 256-byte aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_persample_dw_sq_accumulate(void* stream, const curv_persample_dw_desc* descs, int n, void* workspace,
                                    size_t workspace_bytes);
int curv_persample_dw_quad_reduce(void* stream, const curv_persample_dw_desc* descs, int n, void* workspace,
                                  size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * Curvature of the affine parameters of LayerNorm, GroupNorm and (eval-mode) BatchNorm2d (csrc/norm_factor.hip,
 * DESIGN.md "K22").  y[c] = gamma_c * xh[c] + beta_c is a depthwise 1x1 convolution of the standardised input
 *     xh = (x - mu) * rsqrt(var + eps)          (var the biased variance, computed centred: per-lane Welford sums merged
 *                                                through the set's mean - never E[x^2] - mu^2)
 * so channel c owns the 1 x n_g row [gamma_c | beta_c], n_g = 1 + has_bias, and everything the depthwise line stores fits.
 * xh is never written: a statistics pass reads x once and leaves (mu, rstd) per statistics set, a product pass reads x a
 * second time and g once.  The layer is a logical (N, C, H, W) view of x and of g, float32, each read through four strides
 * in ELEMENTS inside an extent counted from the pointer, with the rules of curv_persample_dw_desc (strides not negative,
 * what one sample spans below 2^31 elements, nothing outside the extents is read).  `mode` names the statistics sets:
 *     CURV_NORM_GROUP     per (n, group) over C / groups channels x H x W          (GroupNorm)
 *     CURV_NORM_POSITION  per (n, h, w) over the C channels                        (LayerNorm on (N, *, D): C = D,
 *                                                                                   H = the middle dims, W = 1, x_sc = 1)
 *     CURV_NORM_GIVEN     `mean` (C) and `var` (C) device arrays                   (BatchNorm2d in eval mode)
 * Entry points (one descriptor type; each reads its own destination fields):
 *     curv_kfac_norm_accumulate, side CURV_NORM_SIDE_A:  dst (C, n_g, n_g) (+)= scale * sum_{n,h,w} [xh, 1][xh, 1]^T   reads x
 *                                side CURV_NORM_SIDE_G:  dst (C, 1, 1)     (+)= scale * sum_{n,h,w} g**2              reads g
 *     curv_persample_norm_sq_accumulate / curv_persample_norm_quad_reduce: phase 1 writes
 *         p[n, c, 0] = sum_{h,w} g * xh      p[n, c, 1] = sum_{h,w} g   (has_bias != 0)
 *     to the workspace; phase 2 is the reduction of curv_persample_dw_sq_accumulate / curv_persample_dw_quad_reduce - the
 *     same kernels - with their fields (dst, c_rs; T, Wt, s, out, t_cs, t_rs, w_rs, o_stride; alpha, first) and formulas.
 * Plain fp32 VALU arithmetic, no atomics, sums in a fixed order: lane, wave, workgroup, then slices and samples in index
 * order.  Lanes run along the contiguous axis (w where the channel stride is not 1, c where it is); how an item is split
 * follows from its own sizes and strides only, so its bits do not depend on the other items of the call, nor on where
 * its records lie (an unaligned record takes the same sums through narrower loads).  Up to 16 items per launch.  Enqueues
 * on `stream` only, never waits on the host, allocates nothing.  An empty call is a no-op.  CURV_ERR_INVALID with the item
 * named, before anything is launched: sizes below 1, an unknown mode or side, `groups` not dividing C, eps not finite or
 * <= 0, negative strides, an extent smaller than what sizes and strides address, a NULL record, a NULL mean / var in
 * given mode, a nonzero `reserved`.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_NORM_GROUP 0
#define CURV_NORM_POSITION 1
#define CURV_NORM_GIVEN 2
#define CURV_NORM_SIDE_A 0
#define CURV_NORM_SIDE_G 1
#define CURV_NORM_SPLIT_L 1024    /* elements of a plane / statistics set from which the four waves of a workgroup share it */
#define CURV_NORM_SLICE 32        /* positions per slice where lanes run along c */
typedef struct curv_norm_desc {
  const float* x;          /* not read by the G side */
  const float* g;          /* not read by the A side */
  long long x_sn, x_sc, x_sh, x_sw, x_elems;
  long long g_sn, g_sc, g_sh, g_sw, g_elems;
  int32_t N, C, H, W;
  int32_t mode;            /* CURV_NORM_* */
  int32_t groups;          /* CURV_NORM_GROUP: divides C; ignored otherwise */
  float eps;
  int32_t has_bias;
  const float* mean;       /* CURV_NORM_GIVEN */
  const float* var;
  int32_t side;            /* curv_kfac_norm_accumulate: CURV_NORM_SIDE_* */
  int32_t first;
  float scale;             /* curv_kfac_norm_accumulate */
  float alpha;             /* the per-sample reductions */
  int32_t reserved;        /* 0 */
  int32_t reserved2;       /* 0 */
  float* dst;              /* factor: (C, n_g, n_g) / (C, 1, 1) contiguous; sq: (C, n_g) with row stride c_rs >= n_g */
  long long c_rs;
  const float* T;          /* curv_persample_norm_quad_reduce, as in curv_persample_dw_desc; each may be NULL */
  const float* Wt;
  const float* s;
  float* out;
  long long t_cs, t_rs, w_rs, o_stride;
} curv_norm_desc;
/* Device scratch (bytes, 256-byte aligned regions) for these factors / items; 0 with the error text set for an invalid
 * descriptor.  Host only; the pointers are not read. */
size_t curv_kfac_norm_workspace_bytes(const curv_norm_desc* descs, int n);
size_t curv_persample_norm_workspace_bytes(const curv_norm_desc* descs, int n);
/* Host only: FLOPs per factor: the statistics pass (6 per element; none on the G side or in given mode) plus the products
 * (A: 2 + 2 n_g per element, G: 2). */
int curv_kfac_norm_plan_flops(const curv_norm_desc* descs, int n, long long* out);
/* Host only: per item the FLOPs (statistics + 2 + 2 n_g per element) and the bytes the algorithm needs, 4 N C H W times
 * 3 (x twice, g once; given mode: 2); either array may be NULL. */
int curv_persample_norm_plan_info(const curv_norm_desc* descs, int n, long long* flops, long long* bytes);
/* The workspace must be 256-byte aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_kfac_norm_accumulate(void* stream, const curv_norm_desc* descs, int n, void* workspace, size_t workspace_bytes);
int curv_persample_norm_sq_accumulate(void* stream, const curv_norm_desc* descs, int n, void* workspace,
                                      size_t workspace_bytes);
int curv_persample_norm_quad_reduce(void* stream, const curv_norm_desc* descs, int n, void* workspace,
                                    size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * Curvature of an nn.Embedding weight (csrc/embedding_factor.hip, DESIGN.md "K26").  The layer is a bias-free Linear on
 * one-hot rows, so its input-side Kronecker factor is exactly diagonal - token counts - and its per-sample gradient row v is
 * the sum of the grad_output rows of the positions that hold token v.  `idx`: the (N, T) token indices, contiguous, int32 or
 * int64 (`idx_i64`), `positions` = N T < 2^31 of them.  Every kernel checks every index it reads: one outside [0, V), or
 * equal to `padding_idx` (-1: none), contributes nothing and never addresses memory.
 *
 * curv_kfac_embedding_accumulate:  a[v] (+)= scale * count_v, count of the padding row 0.  The histogram is taken with
 * int32 atomics into the workspace, one per distinct token of a wave (the lanes of a wave that hold the same token are
 * counted by ballot first), so it does not depend on any order.
 *
 * The two per-sample reductions are one segment walker.  The caller supplies the grouped position list: `pos` (n_pos
 * position numbers n T + t, sorted by an outer key, inside it by an inner key, inside that ascending), cut into `chunks`
 * (n_chunks records {begin, end, group, slot}: pos[begin, end) belongs to outer key `group`, at most CURV_EMB_SPLIT_L
 * positions; slot -1 where the chunk is its whole group, else the chunk's number among the n_slots chunks of split
 * groups) and `mgroups` (n_mgroups records {slot_begin, slot_end, group}, one per split group).  A segment is a run of
 * equal inner keys; its rows g[n, t, :] are summed in list order into r, and w r**2 is added to the group's accumulator
 * in segment order; a split group's chunks leave (head, accumulator, tail) in the workspace and a second kernel adds them
 * in chunk order.  The group is then written once.  No floating-point atomics: the same inputs give the same bits.
 *     CURV_EMB_SQ    outer key = token, inner = sample:  dst[v, :] (+)= alpha * sum_n (sum_{t: idx[n,t] = v} g[n, t, :])**2
 *     CURV_EMB_QUAD  outer key = sample, inner = token:  out[n] (+)= alpha * sum_v sum_d w[v, d] (sum_{t: idx[n,t] = v} g[n, t, d])**2
 *                    w: (V, D) with row stride w_rs (`w_kind` CURV_EMB_W_MATRIX) or (V) (CURV_EMB_W_VECTOR)
 * g is read through its strides g_sn, g_st in ELEMENTS (unit stride along d) inside `g_elems` elements from the pointer;
 * one wave walks 256 contiguous floats of a group, 16 bytes per lane where pointer and strides allow it.  A record list
 * that disagrees with `idx` loses contributions, never reads or writes outside the tensors: every entry is checked.
 * CURV_ERR_INVALID before anything is launched: sizes below 1, N T != positions, negative strides, an extent smaller than
 * what sizes and strides address, a NULL tensor, an unknown mode or w_kind, a nonzero `reserved`.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_EMB_SPLIT_L 128      /* positions per chunk of a group's list */
#define CURV_EMB_SQ 0
#define CURV_EMB_QUAD 1
#define CURV_EMB_W_MATRIX 1
#define CURV_EMB_W_VECTOR 2
typedef struct curv_embedding_desc {
  const void* idx;
  long long positions;
  int32_t idx_i64;
  int32_t V;
  int32_t padding_idx;     /* -1: none */
  int32_t first;
  float scale;
  int32_t reserved;        /* 0 */
  float* a;                /* (V) contiguous */
} curv_embedding_desc;
typedef struct curv_embedding_walk_desc {
  const void* idx;
  const float* g;
  long long positions, g_sn, g_st, g_elems;
  int32_t idx_i64, N, T, V, D, padding_idx, mode, first;
  const int32_t* pos;
  const int32_t* chunks;   /* (n_chunks, 4) */
  const int32_t* mgroups;  /* (n_mgroups, 3); may be NULL when n_mgroups = 0 */
  int32_t n_pos, n_chunks, n_mgroups, n_slots;
  float* dst;              /* CURV_EMB_SQ: (V, D), row stride dst_rs >= D */
  long long dst_rs;
  const float* w;          /* CURV_EMB_QUAD */
  long long w_rs;
  float* out;              /* CURV_EMB_QUAD: (N), stride o_stride >= 1 */
  long long o_stride;
  int32_t w_kind;
  float alpha;
  int32_t reserved;        /* 0 */
  int32_t reserved2;       /* 0 */
} curv_embedding_walk_desc;
/* Device scratch (bytes); 0 with the error text set for an invalid descriptor.  Host only; the pointers are not read. */
size_t curv_kfac_embedding_workspace_bytes(const curv_embedding_desc* descs, int n);
size_t curv_persample_embedding_workspace_bytes(const curv_embedding_walk_desc* descs, int n);
/* Host only: positions + V per histogram (integer adds and the final multiply-add). */
int curv_kfac_embedding_plan_flops(const curv_embedding_desc* descs, int n, long long* out);
/* The workspace must be 256-byte aligned.  `descs` is a host array; it may be reused as soon as the call returns. */
int curv_kfac_embedding_accumulate(void* stream, const curv_embedding_desc* descs, int n, void* workspace,
                                   size_t workspace_bytes);
int curv_persample_embedding_sq_accumulate(void* stream, const curv_embedding_walk_desc* descs, int n, void* workspace,
                                           size_t workspace_bytes);
int curv_persample_embedding_quad_reduce(void* stream, const curv_embedding_walk_desc* descs, int n, void* workspace,
                                         size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The other reductions of a depthwise layer's products (csrc/persample_dw.hip, DESIGN.md "K15"): what the joint output
 * covariance and the damping grid of the linearised predictive need.  Phase 1 is that of the entry points above, so an
 * item's products p have the same bits; the descriptors below carry the record, geometry and extent fields of
 * curv_persample_dw_desc under the same names and rules.  T, the weights and s are each optional (identity, ones, ones).
 *     curv_persample_dw_project:           y[n*y_ns + c*n_g + j] = s[c] * W[c*w_rs + j] * sum_i T[c*t_cs + i*t_rs + j] * p[n,c,i]
 *     curv_persample_dw_quad_grid_reduce:  out[h*o_hs + n*o_stride] (+)= gain[h] * sum_c sum_j w_h(c,j) *
 *                                                                      ( sum_i T[c*t_cs + i*t_rs + j] * p[n,c,i] )**2
 *         separable (u and v given, V NULL):  w_h(c,j) = 1 / ((u[c] + shift[h]) * (v[c*v_rs + j] + shift[h]))
 *         dense     (V given, u and v NULL):  w_h(c,j) = 1 / (V[c*v_rs + j] + shift[h])
 * project: W is the unsquared weight (Diagonal: W = inv; KFAC: T = L_A stacked, s = L_G stacked); y holds N rows of
 * C*n_g values, y_ns >= C*n_g floats apart, and nothing between the rows is touched.  The variance of
 * curv_persample_dw_quad_reduce is sum_e y[n][e]**2; the covariance of K outputs is the Gram of their K rows
 * (curv_persample_gram_reduce).
 * grid: the contract of curv_persample_quad_grid_reduce - 1 <= H <= CURV_PERSAMPLE_GRID_MAX; `shift` and `gain` are HOST
 * arrays of H floats, copied into the kernel arguments during the call; every shift finite and > 0, every gain finite;
 * IEEE divisions; no alpha; grid point h is computed from shift[h] and gain[h] alone, so row h has the same bits
 * whatever other grid points or items share the call.  KFAC: T = U_A stacked (C, n_g, n_g), u = the 1 x 1 G factors (C),
 * v = eig(A) (C, n_g), shift = sqrt(rho); Diagonal: T NULL, V = state, shift = rho.  Up to 8 items per launch of the
 * reduction.
 * Both: fp32 sums in a fixed order (thread, lane, wave by DPP, workgroup), no atomics, an item's plan follows from its
 * own sizes only; the workspace (256-byte aligned) holds the p of every item and every word read from it was written by
 * the same call.  Work goes on `stream` only, nothing is allocated, the host never waits.  An empty call is a no-op;
 * invalid input returns CURV_ERR_INVALID with the item named, before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_persample_dw_project_desc {
  const float* x;
  const float* g;
  long long x_sn, x_sc, x_sh, x_sw, x_elems;
  long long g_sn, g_sc, g_sh, g_sw, g_elems;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t Ho, Wo;
  int32_t has_bias;
  int32_t reserved;
  const float* T;          /* may be NULL */
  const float* Wt;         /* the weights W of the formula; may be NULL */
  const float* s;          /* may be NULL */
  float* y;
  long long t_cs, t_rs, w_rs, y_ns;
} curv_persample_dw_project_desc;
typedef struct curv_persample_dw_grid_desc {
  const float* x;
  const float* g;
  long long x_sn, x_sc, x_sh, x_sw, x_elems;
  long long g_sn, g_sc, g_sh, g_sw, g_elems;
  int32_t N, C, H, W;
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t Ho, Wo;
  int32_t has_bias;
  int32_t first;
  const float* T;          /* may be NULL */
  const float* u;          /* separable form: C values ... */
  const float* v;          /* ... and (C, n_g) with row stride v_rs */
  const float* V;          /* dense form: (C, n_g) with row stride v_rs */
  float* out;
  const float* shift;      /* host, Hn floats */
  const float* gain;       /* host, Hn floats */
  long long t_cs, t_rs, v_rs, o_stride, o_hs;
  int32_t Hn;              /* the H of the formula: grid points (H names the input height above) */
  int32_t reserved;
} curv_persample_dw_grid_desc;
/* Host only, as curv_persample_dw_workspace_bytes and curv_persample_dw_plan_info (the FLOPs include those of the
 * transform and, for the grid, of the Hn weighted sums; the bytes of project include y). */
size_t curv_persample_dw_project_workspace_bytes(const curv_persample_dw_project_desc* descs, int n);
int curv_persample_dw_project_plan_info(const curv_persample_dw_project_desc* descs, int n, long long* flops, long long* bytes);
size_t curv_persample_dw_quad_grid_workspace_bytes(const curv_persample_dw_grid_desc* descs, int n);
int curv_persample_dw_quad_grid_plan_info(const curv_persample_dw_grid_desc* descs, int n, long long* flops, long long* bytes);
int curv_persample_dw_project(void* stream, const curv_persample_dw_project_desc* descs, int n, void* workspace,
                              size_t workspace_bytes);
int curv_persample_dw_quad_grid_reduce(void* stream, const curv_persample_dw_grid_desc* descs, int n, void* workspace,
                                       size_t workspace_bytes);

/* Per-sample Gram of K staged vectors (csrc/persample_dw.hip; no phase 1, no geometry, no workspace):
 *     out[n*o_ns + k*o_rs + k'] (+)= alpha * sum_{e < E} Y[k*y_ks + n*y_ns + e] * Y[k'*y_ks + n*y_ns + e]      k, k' < K
 * 1 <= K <= CURV_PERSAMPLE_COV_MAX_OUTPUTS (defined below: 16).  The output layout and `first` are those of
 * curv_persample_cov_reduce: o_rs >= K, o_ns >= K*o_rs, nothing between the K x K entries is touched; one value per pair
 * k <= k' is computed and stored at both places, so the result is bit-for-bit symmetric.  One workgroup per sample, the
 * pair sums in registers; fp32 sums in a fixed order (thread, lane, wave by DPP, workgroup), no atomics.  The items of
 * a call must not share destinations.  Work goes on `stream` only.  An empty call is a no-op; invalid sizes or strides
 * return CURV_ERR_INVALID with the item named, before anything is launched. */
typedef struct curv_persample_gram_desc {
  const float* Y;
  float* out;
  long long y_ks, y_ns, o_ns, o_rs;
  int32_t N, K, E;
  int32_t first;
  float alpha;
  int32_t reserved;
} curv_persample_gram_desc;
int curv_persample_gram_reduce(void* stream, const curv_persample_gram_desc* descs, int n);

/* ------------------------------------------------------------------------------------------------
 * Linearised Laplace (GLM) predictive: the other reduction of the per-sample products (csrc/persample.hip) - over the
 * entries of P_n = A_n B_n^T, per sample:
 *     out[s*o_stride] (+)= alpha * sum_{i < M, j < Nc} W[i*w_rs + j] * ( sum_{l < L} A[s*a_ns + i*a_rs + l] * B[s*b_ns + j*b_rs + l] )**2
 * With A = the layer's grad_output g_n when sum_n f_c(x_n) is back-propagated and B = X_n, P_n is the Jacobian of
 * output c for sample s with respect to [W | b], and the sum is the layer's share of the variance of f_c(x_s) under the
 * posterior an estimator samples from (no reference counterpart: the reference only offers the Monte-Carlo predictive):
 *     KFAC      sample L_G Z L_A^T              A = L_G^T g,  B = L_A^T X,  W = NULL
 *     Diagonal  sample Z * inv                  A = g,        B = X,        W = inv**2
 *     EFB       sample U_G (Z * inv) U_A^T      A = U_G^T g,  B = U_A^T X,  W = inv**2
 * A, B, S, M, Nc, L and the four operand strides are those of curv_persample_desc, with the same rules (operand
 * extents below 2^31 bytes, l values at or behind L never enter a product, whole 16-byte groups are fetched) and one
 * more: A and B are 16-byte aligned and a_ns, a_rs, b_ns, b_rs are multiples of 4 floats, so that every row starts on
 * a 16-byte boundary (CURV_ERR_INVALID otherwise) - what curv_persample_pack writes and what an operand read in place
 * with L % 4 == 0 has.  W is
 * M x Nc with row stride w_rs >= Nc, or NULL for all ones; it is never read outside its M x Nc entries.  out is S values
 * o_stride >= 1 floats apart (a column of an (N, classes) matrix); `first` != 0 overwrites them.  fp32 MFMA, fp32 sums
 * in a fixed order (lane, wave, workgroup, then tiles in tile order), no atomics; the plan of an item follows from its
 * own sizes only, so its bits do not depend on the other items of the call.  Enqueues on `stream` only, never waits on
 * the host, allocates nothing.  An empty call is a no-op; invalid sizes or strides return CURV_ERR_INVALID with the
 * item named.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_persample_quad_desc {
  const float* A;
  const float* B;
  const float* W;          /* may be NULL */
  float* out;
  long long a_ns, a_rs, b_ns, b_rs, w_rs, o_stride;
  int32_t S, M, Nc, L;
  int32_t first;
  float alpha;
} curv_persample_quad_desc;
/* Device scratch for these items (bytes: one float per output tile and sample); 0 with the error text set (naming the
 * item) for invalid sizes.  Host only. */
size_t curv_persample_quad_workspace_bytes(const curv_persample_quad_desc* descs, int n);
/* Host only: the multiply-add FLOPs the plan executes per item (as curv_persample_plan_flops: at least 2 S M Nc L). */
int curv_persample_quad_plan_flops(const curv_persample_quad_desc* descs, int n, long long* out);
/* An MFMA and a reduce launch per batch of up to 16 items.  The workspace must be 256-byte aligned.  `descs` is a host
 * array; it may be reused as soon as the call returns. */
int curv_persample_quad_reduce(void* stream, const curv_persample_quad_desc* descs, int n, void* workspace,
                               size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The weighted per-sample product projected from the left (csrc/persample.hip; DESIGN.md "K19"), per sample:
 *     Z[s*z_ns + j*z_rs + l*z_cs] (+)= alpha * sum_{i < M} W[i*w_rs + j] * P_s[i][j] * U[i*u_rs + l],    j < Nc, l < R
 * with P_s = A_s B_s^T as above.  INF's posterior weighs the entries of the Jacobian in the parameter basis (W = r**2)
 * before it rotates them into the Kronecker eigenbasis (U = U_G; the other rotation, by U_A, is a plain product on Z), so
 * no rotation of the operands can stand in for this reduction.  At a sample's end the MFMA accumulators, times W, are
 * the A operand of a second v_mfma_f32_32x32x2_f32 straight from the registers: neither P_s nor W o P_s is written.
 * A, B, S, M, Nc, L, the operand strides and W (required here) follow the rules of curv_persample_quad_desc; U is M x R
 * with row stride u_rs >= R, any R >= 1, read only inside its M x R entries; Z is addressed through three positive
 * strides and nothing beside its S x Nc x R entries is touched.  A and B never change places in this plan: M <= 64 takes
 * 64 x 128 tiles, any other M 128 x 128 ones.  fp32 MFMA, fp32 sums in a fixed order (the 64 rows of a wave by the MFMA,
 * then a sample's row tiles and the two wave rows of each in order), no atomics; an item's plan follows from its own
 * sizes only, so its bits do not depend on the other items of the call.  Enqueues on `stream` only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_persample_project_desc {
  const float* A;
  const float* B;
  const float* W;
  const float* U;
  float* Z;
  long long a_ns, a_rs, b_ns, b_rs, w_rs, u_rs, z_ns, z_rs, z_cs;
  int32_t S, M, Nc, L, R;
  int32_t first;
  float alpha;
  int32_t reserved;        /* 0 */
} curv_persample_project_desc;
/* Device scratch for these items (bytes: one Nc x R block per sample and 64-row part of M); 0 with the error text set
 * for invalid sizes.  Host only. */
size_t curv_persample_project_workspace_bytes(const curv_persample_project_desc* descs, int n);
/* Host only: the multiply-add FLOPs the plan executes per item, those of the products plus those of the second MFMA
 * (at least 2 S M Nc (L + R)). */
int curv_persample_project_plan_flops(const curv_persample_project_desc* descs, int n, long long* out);
/* An MFMA and a reduce launch per batch of up to 16 items.  The workspace must be 256-byte aligned. */
int curv_persample_project(void* stream, const curv_persample_project_desc* descs, int n, void* workspace,
                           size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The same reduction for a whole grid of damping pairs (add, multiply) in one pass over the products
 * (csrc/persample.hip; DESIGN.md "K12"): for h < H, per sample,
 *     out[h*o_hs + s*o_stride] (+)= gain[h] * sum_{i < M, j < Nc} w_h(i,j) * ( sum_{l < L} A_s[i][l] * B_s[j][l] )**2
 *     separable (u and v given, V NULL):   w_h(i,j) = 1 / ((u[i] + shift[h]) * (v[j] + shift[h]))     u: M floats, v: Nc floats
 *     dense     (V given, u and v NULL):   w_h(i,j) = 1 / (V[i*v_rs + j] + shift[h])                  V: M x Nc, v_rs >= Nc
 * With the operands in the posterior's eigenbasis the damping enters the variance only through these weights, with
 * rho = add / multiply and gain = 1 / multiply:
 *     KFAC      A = U_G^T g,  B = U_A^T X,  u = eig(G), v = eig(A),  shift = sqrt(rho)
 *     Diagonal  A = g,        B = X,        V = state,               shift = rho
 *     EFB       A = U_G^T g,  B = U_A^T X,  V = state,               shift = rho
 * so one call gives what H calls of curv_persample_quad_reduce behind H inversions give.  1 <= H <=
 * CURV_PERSAMPLE_GRID_MAX.  `shift` and `gain` are HOST arrays of H floats; they are copied into the kernel arguments
 * during the call.  Every shift must be finite and > 0, every gain finite; u, v and V are expected to be >= 0 (an
 * entry + shift of 0 divides by zero).  A, B, S, M, Nc, L and the four operand strides follow the rules of
 * curv_persample_quad_desc: A and B 16-byte aligned, strides multiples of 4 floats, extents below 2^31 bytes, no
 * l >= L enters a product.  u, v and V are never read outside their M / Nc / M x Nc entries.  out is H rows of S values,
 * o_stride >= 1 floats between samples and o_hs >= 1 floats between grid points (H > 1); `first` != 0 overwrites them,
 * nothing between them is touched.  There is no alpha: gain[h] is the scale.
 * The weights are formed with IEEE (correctly rounded) divisions.  fp32 MFMA, fp32 sums in a fixed order (lane, wave
 * by DPP, workgroup, then tiles in tile order), no atomics; the plan of an item follows from its own sizes only and
 * grid point h is computed from shift[h] and gain[h] alone, so row h has the same bits whatever other grid points or
 * items share the call.  Enqueues on `stream` only, never waits on the host, allocates nothing.  An empty call is a
 * no-op; invalid sizes, strides, H, shift or gain return CURV_ERR_INVALID with the item named.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_PERSAMPLE_GRID_MAX 16
typedef struct curv_persample_grid_desc {
  const float* A;
  const float* B;
  const float* u;          /* separable form: M eigenvalues of the A side ... */
  const float* v;          /* ... and Nc of the B side */
  const float* V;          /* dense form: M x Nc */
  float* out;
  const float* shift;      /* host, H floats */
  const float* gain;       /* host, H floats */
  long long a_ns, a_rs, b_ns, b_rs, v_rs, o_stride, o_hs;
  int32_t S, M, Nc, L;
  int32_t H;
  int32_t first;
} curv_persample_grid_desc;
/* Device scratch for these items (bytes: H floats per output tile and sample); 0 with the error text set (naming the
 * item) for invalid input.  Host only. */
size_t curv_persample_quad_grid_workspace_bytes(const curv_persample_grid_desc* descs, int n);
/* Host only: the multiply-add FLOPs of the MFMA products the plan executes per item (those of
 * curv_persample_quad_plan_flops: they do not depend on H; the H weighted sums at a sample's end are not counted). */
int curv_persample_quad_grid_plan_flops(const curv_persample_grid_desc* descs, int n, long long* out);
/* An MFMA and a reduce launch per batch of up to 8 items.  The workspace must be 256-byte aligned.  `descs`, `shift`
 * and `gain` are host arrays; they may be reused as soon as the call returns. */
int curv_persample_quad_grid_reduce(void* stream, const curv_persample_grid_desc* descs, int n, void* workspace,
                                    size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * Joint output covariance of the linearised Laplace predictive: the third reduction of the per-sample products
 * (csrc/persample.hip) - a Gram over K outputs, per sample:
 *     out[s*o_ns + c*o_rs + c'] (+)= alpha * sum_{i < M, j < Nc} W[i*w_rs + j] * P_{s,c}[i][j] * P_{s,c'}[i][j]
 *     P_{s,c}[i][j] = sum_{l < L} A[c*a_cs + s*a_ns + i*a_rs + l] * B[s*b_ns + j*b_rs + l]          for c, c' < K
 * With A_c the (rotated) grad_output of the layer when sum_n f_c(x_n) is back-propagated and B, W as in the table of
 * curv_persample_quad_reduce, out[s] is the layer's share of the covariance of the outputs f_c(x_s) under the posterior;
 * its diagonal is what K calls of curv_persample_quad_reduce give.  The B rows of a stage are staged once and used
 * against all K outputs.  1 <= K <= CURV_PERSAMPLE_COV_MAX_OUTPUTS.  The rules of curv_persample_quad_desc hold: A and B
 * 16-byte aligned; a_cs (>= 0), a_ns, a_rs, b_ns, b_rs multiples of 4 floats; operand extents (all K outputs of A) below
 * 2^31 bytes; l values at or behind L never enter a product; W is M x Nc with row stride w_rs >= Nc or NULL for all ones
 * and is never read outside its entries.  out is S blocks of K x K, o_rs >= K, o_ns >= K*o_rs; `first` != 0 overwrites
 * the K x K entries (nothing between them is touched).  One value per pair c <= c' is computed and stored at [c][c'] and
 * [c'][c]: both triangles are written and are bit-for-bit symmetric.  fp32 MFMA, fp32 sums in a fixed order (lane, wave
 * by DPP, workgroup, then tiles in tile order), no atomics; the plan of an item follows from its own sizes only, so its
 * bits do not depend on the other items of the call.  Enqueues on `stream` only, never waits on the host, allocates
 * nothing.  An empty call is a no-op; invalid sizes or strides return CURV_ERR_INVALID with the item named.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_PERSAMPLE_COV_MAX_OUTPUTS 16
typedef struct curv_persample_cov_desc {
  const float* A;
  const float* B;
  const float* W;          /* may be NULL */
  float* out;
  long long a_cs, a_ns, a_rs, b_ns, b_rs, w_rs, o_ns, o_rs;
  int32_t S, K, M, Nc, L;
  int32_t first;
  float alpha;
} curv_persample_cov_desc;
/* Device scratch for these items (bytes: K (K + 1) / 2 floats per output tile of 8 x 128 and sample); 0 with the error
 * text set (naming the item) for invalid input.  Host only. */
size_t curv_persample_cov_workspace_bytes(const curv_persample_cov_desc* descs, int n);
/* Host only: the multiply-add FLOPs the plan executes per item: whole tiles, K padded to a multiple of 4, L to stages of
 * 32 - at least the algorithmic 2 S K M Nc L. */
int curv_persample_cov_plan_flops(const curv_persample_cov_desc* descs, int n, long long* out);
/* An MFMA and a reduce launch per batch of up to 16 items.  The workspace must be 256-byte aligned.  `descs` is a host
 * array; it may be reused as soon as the call returns. */
int curv_persample_cov_reduce(void* stream, const curv_persample_cov_desc* descs, int n, void* workspace,
                              size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * Monte-Carlo softmax of the linearised Laplace predictive from the joint logit covariance (csrc/logit_mc.hip): for
 * each of N inputs, with Sigma_n the K x K covariance curv_persample_cov_reduce wrote and mu_n the K selected logits,
 *     f_s = mu_n + L_n z_s  (s < S, z_s ~ N(0, I)),   L_n L_n^T = Sigma_n,   lse_s = logsumexp(f_s, rest[n])
 *     probs[n*K + c] = (1/S) sum_s exp(f_s[c] - lse_s)        probs_rest[n] = (1/S) sum_s exp(rest[n] - lse_s)
 * i.e. E softmax(f) under f ~ N(mu_n, Sigma_n) - the predictive the covariance exists for (the logits share every weight
 * below the head, so they are not independent) - in one kernel that reads Sigma and the logits once and writes (N, K);
 * the (N, S, K) draws stay in registers unless `draws` asks for them.  1 <= K <= CURV_PERSAMPLE_COV_MAX_OUTPUTS.
 *
 * Inputs.  cov: N blocks of K x K with strides o_ns >= K o_rs, o_rs >= K (the layout curv_persample_cov_reduce writes);
 * only the lower triangle c' <= c is read, nothing between or above the entries.  mu: K floats per input, mu_ns >= K
 * apart.  rest: N floats or NULL; rest[n] is the log-sum-exp of the logits of the classes that are NOT selected - they are
 * constants, their variance being 0 under the convention of curv_persample_cov_reduce; NULL (or -inf) means every class is
 * selected, and probs_rest is then 0.  Z: explicit standard-normal noise, z_s[c] at Z[n*z_ns + s*z_ss + c] (z_ss >= K,
 * z_ns >= (S - 1) z_ss + K), or NULL: the draws then come from the generator of curv_randn keyed by `seed` - with
 * Kq = ceil(K / 4), draw s of input n takes the counters offset + (n S + s) Kq + q, q < Kq, and value e of counter q is
 * z_s[4 q + e]: exactly the numbers curv_randn(seed, offset) writes into an (N, S, 4 Kq) buffer, so a call with Z = NULL
 * has the bits of a call with that buffer as Z.  The position of the stream is the host-side `offset` only (the caller
 * advances it by N S Kq); a device-side counter as in curv_randn_counter is not offered.
 *
 * Outputs, each may be NULL but not all: probs (N x K, contiguous), probs_rest (N), draws (N x S x K, contiguous: the
 * f_s themselves), info (N status words).
 *
 * Factorisation.  L_n is the lower Cholesky factor, computed in fp64 from the fp32 entries and kept in fp32.  Sigma_n is
 * positive SEMI-definite and often singular, so a tiny or negative pivot is no error: with
 * thr = 16 * 2^-23 * max_c Sigma_cc, a pivot d_j <= thr makes column j of L exact zeros.  info[n] = the number of dropped
 * columns (0 for a definite block); if a pivot lies below -thr the block is not a covariance: info[n] = -(j + 1) for the
 * first such j, and the column is dropped all the same, so finite input never gives a non-finite output.
 *
 * Plan.  The draws of an input are cut into chunks of max(256, 256 ceil(ceil(S / ceil(1024 / N)) / 256)) draws, one
 * workgroup each, so that few inputs still fill the chip; with more than one chunk the partial sums (K + 1 floats per
 * input and chunk) go to the caller's workspace and a second launch adds them in chunk order.  An item whose inputs have
 * one chunk needs no workspace: curv_logit_mc_workspace_bytes is then 0 WITHOUT an error text, and `workspace` may be
 * NULL.  The plan of an item follows from its own N, K and S only.
 *
 * The rules of the library: fp32 sums in a fixed order (lane, wave by DPP, workgroup, then chunks in chunk order), no
 * atomics, so the bits of an item do not depend on the other items of the call nor on the run.  Enqueues on `stream`
 * only, never waits on the host, allocates nothing.  An empty call is a no-op; invalid sizes or strides (K outside
 * 1 .. 16, o_rs < K, o_ns < K o_rs, mu_ns < K, bad Z strides, N or S below 1, S above 2^30, N S above 2^40, every
 * output NULL) return CURV_ERR_INVALID with the item named.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_logit_mc_desc {
  const float* cov;
  const float* mu;
  const float* rest;       /* may be NULL */
  const float* Z;          /* may be NULL */
  float* probs;            /* may be NULL */
  float* probs_rest;       /* may be NULL */
  float* draws;            /* may be NULL */
  int32_t* info;           /* may be NULL */
  long long o_ns, o_rs, mu_ns, z_ns, z_ss;
  unsigned long long seed, offset;
  int32_t N, K, S;
  int32_t reserved;
} curv_logit_mc_desc;
/* Device scratch for these items (bytes: see Plan; 256-byte aligned per item); 0 with the error text set (naming the
 * item) for invalid input - and 0 without one where no item needs scratch.  Host only. */
size_t curv_logit_mc_workspace_bytes(const curv_logit_mc_desc* descs, int n);
/* Host only: the multiply-add FLOPs of f = mu + L z the plan executes per item: whole quads of every row of L,
 * 2 N S 8 Kq (Kq + 1) - at least the algorithmic 2 N S K (K + 1) / 2. */
int curv_logit_mc_plan_flops(const curv_logit_mc_desc* descs, int n, long long* out);
/* One launch per batch of up to 16 items, a second where an item has chunks.  The workspace must be 256-byte aligned.
 * `descs` is a host array; it may be reused as soon as the call returns. */
int curv_logit_mc(void* stream, const curv_logit_mc_desc* descs, int n, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * Monte-Carlo softmax of the LAST-LAYER Laplace predictive over all classes (csrc/head_mc.hip).  The Jacobian of logit c
 * with respect to the head's [W | b] is e_c phi~^T, so for KFAC, EFB and Diagonal the covariance of the K logits of input
 * n is Sigma_n = M diag(d2_n) M^T with ONE K x K matrix M for the whole batch (KFAC: L_G, lower triangular, d2_n a scalar;
 * EFB: U_G; Diagonal: none) and a non-negative vector d2_n per input.  For each of N inputs
 *     f_s = mu_n + M (sqrt(max(d2_n, 0)) o z_{n,s})  (s < S, z ~ N(0, I_K))
 *     probs[n*K + c] = (1/S) sum_s softmax(f_s)[c]                                  c < K
 * in one kernel on v_mfma_f32_32x32x2_f32 (exact fp32): the (N, S, K) draws stay in accumulators unless `draws` asks for
 * them.  1 <= K <= CURV_HEAD_MC_MAX_CLASSES - no backward pass and no cap of 16 outputs as in curv_logit_mc.
 *
 * Inputs.  M: K x K floats, row stride m_rs >= K, unit column stride, no alignment beyond 4 bytes; NULL means the
 * identity (no product at all).  m_lower != 0: entries with column > row are neither read nor multiplied (they may hold
 * anything, NaN included), and the k-range of a block of 32 rows stops at its last row, so a triangular M costs about half
 * the products.  d2: the value of class c of input n at d2[n*d_ns + c*d_cs], d_cs 0 (one scalar per input) or 1, d_ns at
 * least 1 resp. K; negative values count as 0, and a row of zeros gives probs = softmax(mu_n).  mu: K floats per input,
 * mu_ns >= K apart.  Z: explicit standard-normal noise, z_{n,s}[c] at Z[n*z_ns + s*z_ss + c] (z_ss >= K,
 * z_ns >= (S - 1) z_ss + K), or NULL: the generator of curv_randn keyed by `seed`, with the convention of curv_logit_mc -
 * Kq = ceil(K / 4), draw s of input n takes the counters offset + (n S + s) Kq + q, q < Kq, and value e of counter q is
 * z[4 q + e] - so a call with Z = NULL has the bits of a call whose Z is the (N, S, 4 Kq) buffer curv_randn(seed, offset)
 * wrote.  The position of the stream is the host-side `offset` only (the caller advances it by N S Kq).
 *
 * Outputs, either may be NULL but not both: probs (N x K, contiguous), draws (N x S x K, contiguous: the f_s).
 * `reserved` must be 0.
 *
 * Plan.  The draws of an input are cut into tiles of 32 and the T = ceil(S / 32) tiles into chunks of
 * ceil(T / ceil(256 / N)) tiles, one workgroup each, so that few inputs still fill the chip; with more than one chunk the
 * partial sums (K floats per input and chunk) go to the caller's workspace and a second launch adds them in chunk order.
 * An item whose inputs have one chunk needs no workspace: curv_head_mc_workspace_bytes is then 0 WITHOUT an error text,
 * and `workspace` may be NULL.  The plan of an item follows from its own N, K and S only.
 *
 * The rules of the library: fp32 sums in a fixed order (lane, wave, workgroup, then chunks in chunk order), no atomics, so
 * the bits of an item do not depend on the other items of the call nor on the run; nothing non-finite from finite input.
 * Enqueues on `stream` only, never waits on the host, allocates nothing.  An empty call is a no-op; every item is checked
 * before anything is launched, and invalid sizes or strides (K outside 1 .. CURV_HEAD_MC_MAX_CLASSES, N or S below 1, S
 * above 2^30, N S above 2^40, m_rs < K, d_cs neither 0 nor 1, d_ns too small, mu_ns < K, bad Z strides, both outputs NULL,
 * reserved != 0) return CURV_ERR_INVALID with the item named.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_HEAD_MC_MAX_CLASSES 1024
typedef struct curv_head_mc_desc {
  const float* M;          /* may be NULL: identity */
  const float* d2;
  const float* mu;
  const float* Z;          /* may be NULL */
  float* probs;            /* may be NULL */
  float* draws;            /* may be NULL */
  long long m_rs, d_ns, d_cs, mu_ns, z_ns, z_ss;
  unsigned long long seed, offset;
  int32_t N, K, S;
  int32_t m_lower;
  long long reserved;
} curv_head_mc_desc;
/* Device scratch for these items (bytes: see Plan; 256-byte aligned per item); 0 with the error text set (naming the
 * item) for invalid input - and 0 without one where no item needs scratch.  Host only. */
size_t curv_head_mc_workspace_bytes(const curv_head_mc_desc* descs, int n);
/* Host only: the multiply-add FLOPs of the MFMA products the plan executes per item: whole 32 x 32 x 32 steps,
 * 2 N 32 T 32 32 (steps), steps = sum over the row blocks g < ceil(K / 32) of the k-steps of 32 the block takes
 * (ceil(K / 32), with m_lower min(ceil(K / 32), g + 1)); 0 without M. */
int curv_head_mc_plan_flops(const curv_head_mc_desc* descs, int n, long long* out);
/* One launch per batch of up to 16 items, a second where an item has chunks.  The workspace must be 256-byte aligned.
 * `descs` is a host array; it may be reused as soon as the call returns. */
int curv_head_mc(void* stream, const curv_head_mc_desc* descs, int n, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * curv_head_mc with two more moments of the draws (csrc/head_mc.hip; DESIGN.md "K25"): what splits the uncertainty of the
 * last-layer predictive into its aleatoric and its epistemic part without the (N, S, K) draws.  The first 128 bytes of the
 * descriptor are field for field those of curv_head_mc_desc, and f_s is exactly the f_s of curv_head_mc (same M, m_lower,
 * d2, mu, Z / Philox convention, same counters).  Per input n
 *     probs[n*K + c]    = (1/S) sum_s softmax(f_s)[c]        bit-equal to what curv_head_mc writes for the same fields
 *     entropy[n]        = (1/S) sum_s H_s,   H_s = -sum_c p_c ln p_c = ln(sum_c e^{t_c}) - (sum_c e^{t_c} t_c) / (sum_c e^{t_c}),
 *                                            t_c = f_s[c] - max_c f_s[c]
 *     probs_sq[n*K + c] = (1/S) sum_s softmax(f_s)[c]^2
 * so that with total = H(probs): aleatoric = entropy, epistemic (the mutual information) = total - entropy, and the
 * variance of class c over the draws is probs_sq - probs^2.  K = 1 gives entropy = +0.0 and probs_sq = 1.0 exactly.
 *
 * Outputs, any may be NULL but not all four: probs (N x K), draws (N x S x K), entropy (N), probs_sq (N x K), contiguous.
 * `reserved` must be 0.
 *
 * Plan.  The split rule of curv_head_mc.  With more than one chunk the partial sums of an (input, chunk) are 2 K + 1 floats
 * - probs, squares, entropy - so an item needs align_up(N chunks (2 K + 1) 4, 256) bytes of workspace (0 WITHOUT an error
 * text where every input has one chunk), and the reduce launch finishes all three outputs.
 *
 * Order of the sums: sum e t goes the way of sum e (lane, the two halves of a wave, the four waves in wave order; a term
 * with e = 0 counts as 0); the H_s of the 32 draws of a tile are added by a butterfly over partners 16, 8, 4, 2, 1 lanes
 * apart, then the tiles in tile order, then the chunks in chunk order; the squares go the way of probs.  No atomics, the
 * bits of an item do not depend on the other items of the call; nothing non-finite from finite input, logits so far apart
 * that e^t underflows included.  Everything else - validation, error texts naming the item, launches - as curv_head_mc.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_head_moments_desc {
  const float* M;          /* may be NULL: identity */
  const float* d2;
  const float* mu;
  const float* Z;          /* may be NULL */
  float* probs;            /* may be NULL */
  float* draws;            /* may be NULL */
  long long m_rs, d_ns, d_cs, mu_ns, z_ns, z_ss;
  unsigned long long seed, offset;
  int32_t N, K, S;
  int32_t m_lower;
  float* entropy;          /* may be NULL */
  float* probs_sq;         /* may be NULL */
  long long reserved;
} curv_head_moments_desc;
/* As curv_head_mc_workspace_bytes, with 2 K + 1 floats per input and chunk.  Host only. */
size_t curv_head_mc_moments_workspace_bytes(const curv_head_moments_desc* descs, int n);
/* Host only: equal to curv_head_mc_plan_flops for the same fields. */
int curv_head_mc_moments_plan_flops(const curv_head_moments_desc* descs, int n, long long* out);
/* One launch per batch of up to 16 items, a second where an item has chunks.  The workspace must be 256-byte aligned. */
int curv_head_mc_moments(void* stream, const curv_head_moments_desc* descs, int n, void* workspace,
                         size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The d2 of the last-layer Laplace predictive for a whole grid of damping pairs in one pass (csrc/head_grid.hip;
 * DESIGN.md "K24"): for h < H, input r < N and class j < K
 *     out[(h*N + r)*K + j] = gain[h] * r_h[j] * sum_{i < n} Y[r*y_rs + i]**2 / (T[j][i] + shift[h])
 *     dense     (T given, u and v NULL):   T[j][i] = T[j*t_rs + i],  r_h = 1                       T: K x n, t_rs >= n
 *     separable (u and v given, T NULL):   T[j][i] = v[i],  r_h[j] = 1 / (u[j] + shift[h])         u: K floats, v: n floats
 * With Y the head's input [phi | 1] in the posterior's eigenbasis the damping (add, multiply) enters the logit
 * covariance M diag(d2) M^T only through these weights, with rho = add / multiply and gain = 1 / multiply:
 *     KFAC      Y = Phi~ U_A,  u = eig(G), v = eig(A),  shift = sqrt(rho)     (M = U_G)
 *     EFB       Y = Phi~ U_A,  T = state,               shift = rho           (M = U_G)
 *     Diagonal  Y = Phi~,      T = state,               shift = rho           (M = identity)
 * so slice h is the d2 of curv_head_mc for what the inversion with pair h stands for, and one call serves every pair.
 * 1 <= H <= CURV_HEAD_GRID_MAX.  `shift` and `gain` are HOST arrays of H floats; they are copied into the kernel
 * arguments during the call.  Every shift must be finite and > 0, every gain finite; the spectrum entries are read as
 * they are (expected >= 0: an entry + shift of 0 divides by zero).  Y: N x n floats, row stride y_rs >= n, unit column
 * stride; T likewise; no alignment beyond 4 bytes, and nothing outside the N x n, K x n, K and n entries is read.  out is
 * contiguous (H, N, K); every entry is overwritten.  N, K, n >= 1 with N n, K n and CURV_HEAD_GRID_MAX N K below 2^31.
 * The reciprocals are formed with IEEE (correctly rounded) divisions.
 *
 * Dense: a product on v_mfma_f32_32x32x2_f32 (exact fp32) whose B operand is generated - a lane holds a value of T in the
 * B layout, forms the reciprocals of its pairs in registers and feeds one MFMA per pair against the shared A operand
 * Y**2 - so T is read once per two pairs and no (H, K, n) weight tensor exists.  Plan: out is cut into 32 x 32 blocks,
 * B = ceil(N / 32) ceil(K / 32) of them, and the S = ceil(n / 32) steps of i into chunks of
 * max(4, ceil(S / ceil(256 / B))) steps so that few blocks still fill the chip; with more than one chunk the partial sums go to the caller's workspace
 * (CURV_HEAD_GRID_MAX N K floats per chunk, whatever H) and a second launch adds them in chunk order.  An item of one
 * chunk, and every separable item (one wave per (h, r): the sum over i once, then K stores), needs no workspace:
 * curv_head_grid_workspace_bytes is then 0 WITHOUT an error text, and `workspace` may be NULL.  The plan of an item
 * follows from its own N, K and n only - not from H nor from the other items.
 *
 * The rules of the library: fp32 sums in a fixed order (lane, wave, workgroup, then chunks in chunk order), no atomics;
 * pair h is computed from shift[h] and gain[h] alone, so slice h has the same bits whatever other pairs or items share
 * the call.  Enqueues on `stream` only, never waits on the host, allocates nothing.  An empty call is a no-op; every item
 * is checked before anything is launched, and invalid sizes, strides, H, shift, gain or operands (u / v and T both given,
 * or neither) return CURV_ERR_INVALID with the item named.
 * ---------------------------------------------------------------------------------------------- */
#define CURV_HEAD_GRID_MAX 16
typedef struct curv_head_grid_desc {
  const float* Y;
  const float* u;          /* separable form: K eigenvalues of the G side ... */
  const float* v;          /* ... and n of the A side */
  const float* T;          /* dense form: K x n */
  float* out;
  const float* shift;      /* host, H floats */
  const float* gain;       /* host, H floats */
  long long y_rs, t_rs;
  int32_t N, K, n;
  int32_t H;
} curv_head_grid_desc;
/* Device scratch for these items (bytes: see Plan; 256-byte aligned per item); 0 with the error text set (naming the
 * item) for invalid input - and 0 without one where no item needs scratch.  Host only. */
size_t curv_head_grid_workspace_bytes(const curv_head_grid_desc* descs, int n);
/* Host only: the multiply-add FLOPs of the MFMA products the plan executes per item FOR ONE PAIR - whole 32 x 32 x 32
 * steps, 2 32 32 32 B S, at least the algorithmic 2 N K n; a call runs them once per pair, in groups of two pairs.  0
 * for a separable item (no product). */
int curv_head_grid_plan_flops(const curv_head_grid_desc* descs, int n, long long* out);
/* One launch per batch of up to 8 items, a second where an item has chunks.  The workspace must be 256-byte aligned.
 * `descs`, `shift` and `gain` are host arrays; they may be reused as soon as the call returns. */
int curv_head_grid(void* stream, const curv_head_grid_desc* descs, int n, void* workspace, size_t workspace_bytes);
/* v = max(v, 0) in place      curvatures.py:523 */
int curv_clamp_min0(void* stream, float* v, long long count);
/* out = sqrt(s*v)             curvatures.py:525 */
int curv_sqrt_scale(void* stream, const float* v, double s, float* out, long long count);
/* out = a*b */
int curv_mul(void* stream, const float* a, const float* b, float* out, long long count);

/* Batched device-to-device copy: dst[i][0 .. bytes[i]) = src[i][...] for n buffers in one or a few
 * launches (Curvature.sample_and_replace reloads the mean weights with `load_state_dict`,
 * curvatures.py:118: ~320 separate tensors for a ResNet-50, i.e. ~320 copy launches otherwise).
 * Buffers may have any size and alignment; pairs must not overlap. */
typedef struct curv_copy_desc {
  void* dst;
  const void* src;
  unsigned long long bytes;
} curv_copy_desc;
int curv_copy_batched(void* stream, const curv_copy_desc* descs, int n);

/* ------------------------------------------------------------------------------------------------
 * utils.get_eigenvectors (curvature/utils.py:45-60): symmetric eigendecomposition F = U diag(w) U^T of a
 * batch of fp32 matrices by a two-sided block-Jacobi method in fp64.  U (n x n, fp32) holds the
 * eigenvectors as columns in ascending eigenvalue order (the reference's symeig order); w (n, fp32,
 * optional) the eigenvalues of F (the reference decomposes F + F^T: same vectors, doubled values, and it
 * discards the values).  Signs / bases of degenerate clusters are arbitrary, as with LAPACK.
 * The call synchronises the stream once per sweep to test convergence (off(A) <= tol * ||A||_F);
 * max_sweeps <= 0 selects 60; tol <= 0 selects the size-dependent default: 1e-8 for n <= 1024, 5e-6 above (an fp32 phase
 * followed by one fp64 re-orthogonalisation; the reference's fp32 LAPACK reaches 1e-5 on such factors); a positive tol
 * applies to every matrix of the call.  n <= 8192.  If the iteration has not
 * converged after max_sweeps sweeps the outputs hold the last iterate and the call returns
 * CURV_ERR_NOT_CONVERGED (curv_last_error() carries the final off-norm ratio); *sweeps_done is the
 * number of sweeps executed either way.
 * ---------------------------------------------------------------------------------------------- */
typedef struct curv_eigh_desc {
  const float* F;
  float* U;
  float* w;
  int32_t n;
  int32_t reserved;
} curv_eigh_desc;

size_t curv_syevd_workspace_bytes(const curv_eigh_desc* descs, int n_mats);
int curv_syevd(void* stream, const curv_eigh_desc* descs, int n_mats, void* workspace, size_t workspace_bytes,
               int max_sweeps, double tol, int* sweeps_done);
/* With the defaults (max_sweeps <= 0 and tol <= 0) a matrix at least 2048 wide whose numerical rank is below half its width
 * - the Kronecker factor of a layer with more rows than samples went into it (a 4608-wide ResNet-50 factor at N = 32: rank
 * 1568) - is decomposed through its RANGE (csrc/eigh_lowrank.hip, ABI 10; round 5 did this in the Python mirror only): Gaussian range
 * finder, rank from a pivoted Cholesky of its Gram matrix, Cholesky-QR, the iteration on the k x k projected matrix only, an
 * orthonormal basis of the complement for the zero eigenvalues; accepted iff ||F - P F P|| <= 3e-6 ||F||, otherwise the matrix
 * takes the iteration on the whole matrix like all others.  Same outputs, same order.  The workspace size above includes
 * what the projection needs (about 1.2 GB per 4608-wide matrix).  An explicit max_sweeps or an explicit tol selects the
 * plain iteration.
 * curv_syevd_ex: the same call; `ranks` (optional host array, n_mats ints) receives per matrix the rank k of the projected
 * problem, or 0 for a matrix that went through the plain iteration. */
int curv_syevd_ex(void* stream, const curv_eigh_desc* descs, int n_mats, void* workspace, size_t workspace_bytes,
                  int max_sweeps, double tol, int* sweeps_done, int* ranks);

/* ------------------------------------------------------------------------------------------------
 * INF (sparse information form), curvature/curvatures.py:463-672
 * ---------------------------------------------------------------------------------------------- */
/* _dim_reduction's index work (:617-634): indices of the `rank` largest |lambda_vec| (length n*m, index
 * i*m + j) -> I = unique(idx / m), J = unique(idx % m), ascending int64, and counts = {|I|, |J|}.
 * Exact integer results; ties at the threshold magnitude are broken deterministically. n, m <= 8192. */
typedef struct curv_select_desc {
  const float* lambda_vec;
  int64_t* I;
  int64_t* J;
  int32_t* counts;
  int32_t n, m, rank, reserved;
} curv_select_desc;
int curv_inf_select(void* stream, const curv_select_desc* descs, int n_desc);

/* out[p][i*a + k] = U[p][i] * U[p][k]: rows of the Khatri-Rao square in the closed form of V_s^T V_s
 * (pre_sampler :556-564 without the (n m) x (a b) Kronecker matrix). U is n x a with row stride u_rs. */
int curv_colpairs(void* stream, const float* U, int n, int a, long long u_row_stride, float* out);
/* the same in fp64 (exact products of fp32 values), and out = (double) v^2: the closed form of V_s^T V_s is evaluated
 * in fp64 end to end (curv_gemm_f64_batched), because V_s^T V_s is ill-conditioned for strongly varying r (e.g.
 * invert(1, 1000)) and an fp32 evaluation limits P_c to ~1e-3 there */
int curv_colpairs_f64(void* stream, const float* U, int n, int a, long long u_row_stride, double* out);
int curv_square_f64(void* stream, const float* v, double* out, long long count);
/* vtv[(i,j),(k,l)] = (w + w^T)/2, w = sigma_ij sigma_kl V4[(i,k),(j,l)]   (:564-565) */
int curv_inf_vtv_assemble(void* stream, const float* V4, const float* sigma, int a, int b, float* vtv);
int curv_inf_vtv_assemble_f64(void* stream, const double* V4, const float* sigma, int a, int b, double* vtv);
/* Packed forms: the column pairs are symmetric in (i, k), so out[p][t(i,k)] = U[p][i] U[p][k] for i <= k only,
 * t(i,k) = i a - i (i - 1) / 2 + (k - i), a (a + 1) / 2 columns; V4p = PAp^T r^2 PGp is then
 * (a (a + 1) / 2) x (b (b + 1) / 2) and vtv[(i,j),(k,l)] = sigma_ij sigma_kl V4p[t_a(i,k)][t_b(j,l)] - half / a quarter
 * of the flops of the two products of the closed form, same values (the symmetrisation of :565 is exact here). */
int curv_colpairs_sym_f64(void* stream, const float* U, int n, int a, long long u_row_stride, double* out);
int curv_inf_vtv_assemble_sym_f64(void* stream, const double* V4p, const float* sigma, int a, int b, double* vtv);
/* dst[i][j] = src[i][j] * dl[i] * dr[j] (src fp32 or fp64, dst fp32): P_c = diag(s) L_c diag(s) (:570) */
int curv_diag_scale(void* stream, const void* src, int src_is_f64, float* dst, const float* dl, const float* dr,
                    int rows, int cols);
/* out[r][c] = src[(row_index ? row_index[r] : r) * src_rs + (col_index ? col_index[c] : c) * src_cs], out dense
 * (rows x cols): the `.t().flatten()` views of _dim_reduction (:617-618) and its `[:, I]` / `[I x J]` selections
 * (:636-645) with the int64 index lists curv_inf_select produced, without leaving the device. */
int curv_gather2d(void* stream, const float* src, long long src_rs, long long src_cs, const int64_t* row_index,
                  const int64_t* col_index, float* out, int rows, int cols);
/* Kronecker product with the reference's index convention (curvature/utils.py:288-310):
 * out[(i*br + k)][(j*bc + l)] = a[i][j] * b[k][l]; a is ar x ac, b is br x bc, out (ar*br) x (ac*bc), dense
 * row-major.  The estimators never form it (pre_sampler's closed form); exported for `utils.kron`. */
int curv_kron(void* stream, const float* a, int ar, int ac, const float* b, int br, int bc, float* out);
/* out[i][j] = A(i,j) * B(i,j) for strided 2-D views (EFB.sample's z * inv^T, :458) */
int curv_mul2d(void* stream, const float* A, long long a_rs, long long a_cs, const float* B, long long b_rs,
               long long b_cs, float* out, int rows, int cols);

/* ------------------------------------------------------------------------------------------------
 * Laplace evidence: sum log(gain * x + shift) over whole-model arenas for a grid of damping pairs (csrc/logdet.hip)
 * ---------------------------------------------------------------------------------------------- */
/* out[i * out_stride + h] = weight_i * sum_e f_h(x_i[e * stride_i]) for segment i = 0..n-1 and pair h = 0..pairs-1, and,
 * if `total` is given, total[h] = out[0][h] + out[1][h] + ... in table order.  Per segment:
 *   x, dtype    `count` elements of CURV_DTYPE_F32 or CURV_DTYPE_F64, `stride` elements apart (>= 1; the diagonal of a
 *               square matrix is a stride of width + 1); nothing outside them is read;
 *   mode        CURV_LOGSUM_LOG: f_h(x) = log(gain[h] * max(x, 0) + shift[h]), for every pair;
 *               CURV_LOGSUM_SQUARES: f(x) = x * x into column 0 only (the other columns of the row are left alone, and
 *               `total` takes the segment into column 0 only);
 *   gain, shift per-segment rows of the grid (pairs entries are read; none may be negative).
 * fp64 from the load on: the element is widened, then multiply-add, log and sums are double; a lane takes one logarithm
 * per pair for its 16 elements - of the product of their mantissas, with the exponents summed exactly.  No atomics: a workgroup
 * owns one chunk of CURV_LOGSUM_CHUNK elements of one segment and writes one partial per pair into the workspace; a
 * second launch sums a segment's partials in index order, a third the segments in table order - the same bits for a
 * segment alone, in a batch and on a repeat call.  A segment without elements gives 0.  Columns of `out` from `pairs` on
 * are not written (out_stride >= pairs).  The workspace (device memory, 8-byte aligned) holds the table and the
 * partials: curv_logsum_workspace_bytes = n * CURV_LOGSUM_ROW_BYTES + (sum_i ceil(count_i / CURV_LOGSUM_CHUNK)) * pairs *
 * 8, or 0 with the error text set for an invalid table.  Asynchronous on `stream`, nothing allocated.  n == 0 is a no-op
 * that touches no device.  CURV_ERR_INVALID with "segment <i>" named, before anything is launched: a negative count, a
 * null pointer with count > 0, a stride below 1, an unknown dtype or mode, a pointer not aligned to its elements, a
 * negative (or NaN) gain or shift of a CURV_LOGSUM_LOG segment; also
 * `pairs` outside 1 .. CURV_LOGSUM_GRID_MAX. */
#define CURV_DTYPE_F64 3
#define CURV_LOGSUM_GRID_MAX 16
#define CURV_LOGSUM_CHUNK 4096
#define CURV_LOGSUM_ROW_BYTES 304
#define CURV_LOGSUM_LOG 0
#define CURV_LOGSUM_SQUARES 1
typedef struct curv_logsum_desc {
  const void* x;
  int32_t dtype;           /* CURV_DTYPE_F32 or CURV_DTYPE_F64 */
  int32_t mode;            /* CURV_LOGSUM_LOG or CURV_LOGSUM_SQUARES */
  int64_t count, stride;
  double weight;
  double gain[CURV_LOGSUM_GRID_MAX], shift[CURV_LOGSUM_GRID_MAX];
} curv_logsum_desc;
size_t curv_logsum_workspace_bytes(const curv_logsum_desc* descs, int n, int pairs);
int curv_logsum_grid(void* stream, const curv_logsum_desc* descs, int n, int pairs, double* out, long long out_stride,
                     double* total, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * The one collective of the layer-sharded estimators (reference: per-layer independence,
 * curvature/curvatures.py:20-21, sample_and_replace :117-129): every rank has written the sampled parameters of its
 * own layers into `flat` (the parameters of all layers in one vector, grouped by owning rank: rank k's segment is
 * [displs[k], displs[k] + counts[k]) in floats); after the call every rank holds every segment.  Variable counts,
 * nothing padded to the largest shard: one ncclBroadcast per rank in one RCCL group call on `stream`.
 * `comm` is an ncclComm_t (RCCL) of the caller; counts / displs have ncclCommCount(comm) entries and must agree on all
 * ranks.  RCCL is bound at run time (dlopen): the library has no link-time dependency on it.
 * curv_comm_unique_id / curv_comm_init / curv_comm_destroy: thin wrappers of ncclGetUniqueId / ncclCommInitRank /
 * ncclCommDestroy for callers without RCCL bindings (`id` is the 128-byte ncclUniqueId drawn on rank 0 and shipped to
 * the other ranks by the caller; the calling thread's current device is the rank's device).
 * curv_rccl_available: 1 when RCCL could be bound (dlopen and every symbol), 0 otherwise - local, no communicator, no
 * bootstrap socket: the probe to run on every rank before the collective set-up steps.
 * ---------------------------------------------------------------------------------------------- */
int curv_rccl_available(void);
int curv_allgather_weights(void* comm, void* stream, float* flat, const long long* counts, const long long* displs);
int curv_comm_unique_id(void* id_out_128_bytes);
int curv_comm_init(void** comm_out, int n_ranks, const void* id_128_bytes, int rank);
int curv_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* CURV_HIP_H */
