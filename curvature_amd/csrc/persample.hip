// Exact per-sample Fisher products (curv_persample_sq_accumulate / curv_persample_pack_ex, include/curv_hip.h):
//   C[i][j] (+)= alpha * sum_{n < S} ( sum_{l < L} A[n a_ns + i a_rs + l] * B[n b_ns + j b_rs + l] )**2
// For a layer with grad_output g_n (m x L) and unfolded input X_n (n_in x L) the inner sum is P_n = g_n X_n^T, the
// sample's share of [W.grad | b.grad]; the sum of its squares is the Fisher diagonal (Diagonal) and, on operands rotated
// into the Kronecker eigenbasis, EFB's eigenvalue correction.  P_n is never written: a 128 x 128 tile of it lives in the
// MFMA accumulators for the length of one sample, is squared and added into a second accumulator set at the sample's end
// and starts the next sample from zero.
//
// Three launches per batch of up to 16 products:
//   1. (curv_persample_pack_ex, a call of its own) X of a layer into caller scratch wherever the source cannot be read in
//      place: the unfold of a convolution input (rows (c, kh, kw)), the transpose of a Linear input (N, T, D), or a plain
//      copy; plus the ones row of a biased layer; every row padded with zeros to Lp columns by the pack itself.
//   2. product: one workgroup per item = (product, 128 x 128 output tile, range of samples); 2 x 2 waves of 64 x 64, each
//      2 x 2 v_mfma_f32_32x32x2_f32 blocks, on the stage engine (nt_stage.h), a stage being 32 l values of one sample.
//      The stages of all samples of the item form ONE sequence (ps_walk_samples: the prefetch runs across sample
//      boundaries); the last stage of a sample whose L is no multiple of 32 is the engine's tail stage, so what lies behind
//      a row in memory (the next row, the next sample, NaN) never enters a product.  64 + 64 accumulators per lane, two
//      workgroups per CU (registers and 64 KiB of LDS each).  A product whose smaller side has at most 64 rows runs on
//      64 x 128 tiles with that side as the A panel (2 x 1 blocks per wave, the transposed tile when the side is Nc):
//      half the MFMAs of a half-empty 128 x 128 tile.  Each item writes its fp32 slab.
//   3. reduce: one thread per entry of C sums the slabs of its tile in slice order, scales, writes or adds.
// The split of a product into sample ranges follows from its own sizes only, every item and reduce thread reads only its
// own product's operands and slabs, and all sums run in a fixed order without atomics: a product's bits are the same
// alone, in a whole-model call and on a sharded rank.  No host synchronisation, no device allocation; tables travel as
// kernel arguments.
//
// The other reduction of the same products (curv_persample_quad_reduce): over the entries, per sample,
//   out[n] (+)= alpha * sum_ij W[i][j] * P_n[i][j]**2
// - the variance of a network output under a Laplace posterior (curvatures.py: functional_variance).  Same items, same
// staging; the product launch leaves one float per (tile, sample) instead of a slab (see ps_product_tile), the reduce
// launch sums a sample's tiles in tile order.
//
// The same reduction for H <= 16 damping pairs at once (curv_persample_quad_grid_reduce): per sample and grid point,
//   out[h][n] (+)= gain[h] * sum_ij w_h(i, j) * P_n[i][j]**2,   w_h = 1 / ((u_i + shift_h)(v_j + shift_h))  or  1 / (V_ij + shift_h)
// - in the posterior's eigenbasis the damping (add, multiply) enters the variance only through these weights (curvatures.py:
// functional_variance_grid).  Two more modes of ps_product_tile: P_n**2 is formed once per sample and
// summed against the weights of one grid point after the other; partial[tile][sample][h].
//
// The third (curv_persample_cov_reduce): a Gram over K <= 16 outputs, per sample,
//   out[n][c][c'] (+)= alpha * sum_ij W[i][j] * P_{n,c}[i][j] * P_{n,c'}[i][j],   P_{n,c} = A_{c,n} B_n^T
// - the joint covariance of the network outputs (curvatures.py: functional_covariance).  A kernel of its own
// (ps_cov_tile) on the same engine and walk: tiles of 8 rows i x 128 columns j of all outputs, so that a lane holds every output
// of its entries and the Gram is lane-local; the B rows of a stage are staged once for all outputs.
//
// The fourth (curv_persample_project): the weighted product projected from the left, per sample,
//   Z[n][j][l] (+)= alpha * sum_i W[i][j] * P_n[i][j] * U[i][l],   l < R
// - what INF's low-rank term needs of a layer's Jacobian (curvatures.py: INF): the posterior weighs the
// entries in the parameter basis BEFORE the rotation into the Kronecker eigenbasis, so no rotation of the operands can
// stand in for it.  One more mode of ps_product_tile: at a sample's end the accumulators, times W, are the A operand of
// a second MFMA straight from the registers; neither P_n nor W o P_n is written.
#include "nt_stage.h"
#include "side_build.h"
#include "wave_sum.h"

#include <climits>

namespace curv {
namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_TM = nt::TM;                  // tile rows / columns; the stage constants are nt:: (nt_stage.h)
constexpr int PS_BATCH = 16;                   // products per launch (tables as kernel arguments)
constexpr int PS_ITEMS_TARGET = 512;           // a product is cut into sample ranges until it has about this many items ...
constexpr int PS_STAGES_MIN = 64;              // ... of at least 64 stages
constexpr long long PS_BYTES_MAX = 1LL << 31;  // operand extents: 32-bit buffer offsets

// What both kinds of product share: the operands and their tiling, as operands_of fills them.
struct PsOperands {
  const float* A;
  const float* B;
  long long a_ns, a_rs, b_ns, b_rs;
  int S, M, Nc, L;             // as the product kernel sees them: A and B have changed places when `swap`
  int tiles_n, tiles;          // output tiles: tiles = tiles_m tiles_n
  int spi, slices;             // samples per item, sample ranges
  int half, swap;              // 64 x 128 tiles (M <= 64); the kernel computes the transposed tile (C is Nc x M)
  int first;
  float alpha;
  unsigned a_bytes, b_bytes;
  long long base;              // first item / reduce block of this product in the launch
};

struct PsProduct : PsOperands {
  float* C;
  float* slabs;
  long long c_rs;
};

typedef ArgBatch<PsProduct, PS_BATCH> PsBatch;

// A product of curv_persample_quad_reduce: instead of C and slabs the weights W (entry (i, j) of the tile the kernel
// computes at W[i w_is + j w_js]: the strides change places with the operands when `swap`), the fp32
// `partial`[tile][sample] and the S outputs.
struct PsQuad : PsOperands {
  const float* W;              // may be null: all ones
  float* out;
  float* partial;
  long long w_is, w_js, o_stride;
};

typedef ArgBatch<PsQuad, PS_BATCH> PsQuadBatch;

// A product of curv_persample_quad_grid_reduce: H grid points, each with its `shift` and `gain` (by value: the tables of
// the call travel with the kernel arguments), and the weights' source - the eigenvalues u (rows of the tile the kernel
// computes) and v (columns), or the dense V (entry (i, j) at V[i v_is + j v_js]); u / v and the V strides change places
// with the operands when `swap`.  partial[tile][sample][h].  Eight products per launch: the record is 320 bytes.
constexpr int GRID_MAX = CURV_PERSAMPLE_GRID_MAX;
constexpr int PS_GRID_BATCH = 8;

struct PsGrid : PsOperands {
  const float* u;              // separable form (V null)
  const float* v;
  const float* V;              // dense form (u, v null)
  float* out;
  float* partial;
  long long v_is, v_js, o_stride, o_hs;
  int H;
  float shift[GRID_MAX], gain[GRID_MAX];
};

typedef ArgBatch<PsGrid, PS_GRID_BATCH> PsGridBatch;

// A product of curv_persample_cov_reduce: K operands A_c (output c at A + c a_cs) against one B.  Output tiles are
// COV_TI rows i x 128 columns j of ALL outputs (see ps_cov_tile); `half` and `swap` are 0.  partial[tile][sample][pair],
// pair = (c, c') with c <= c' in row-major order of the upper triangle.
constexpr int COV_TI = 8;                      // rows i per output tile
constexpr int COV_K_MAX = CURV_PERSAMPLE_COV_MAX_OUTPUTS;
constexpr int COV_PAIRS_MAX = COV_K_MAX * (COV_K_MAX + 1) / 2;
static_assert(COV_K_MAX == 16, "ps_cov_product_kernel instantiates 1 .. 4 groups of four outputs");

struct PsCov : PsOperands {
  const float* W;              // may be null: all ones
  float* out;
  float* partial;
  long long a_cs, w_rs, o_ns, o_rs;
  int K, pairs;
};

typedef ArgBatch<PsCov, PS_BATCH> PsCovBatch;

// A product of curv_persample_project: the weights W (M x Nc, as PsQuad's; never swapped), U (M x R, row stride u_rs), the
// destination Z (entry (n, j, l) at Z[n z_ns + j z_rs + l z_cs]) and the fp32 `partial`[sample][part][Nc][R]: part = the
// 64-row half of a row tile (half tiles: the one part there is), 2 tm + wave row.
struct PsProject : PsOperands {
  const float* W;
  const float* U;
  float* Z;
  float* partial;
  long long w_is, w_js, u_rs, z_ns, z_rs, z_cs;
  int R, parts;
};

typedef ArgBatch<PsProject, PS_BATCH> PsProjectBatch;

struct Plan {
  int tiles_m, tiles_n, tiles, sps, spi, slices, half, swap;
  int parts;                                   // curv_persample_project: partial blocks per sample
  long long a_bytes, b_bytes;
  size_t slab_bytes;
  long long flops;
};

// The sample ranges of a product of `p->tiles` output tiles: it follows from the product's own sizes only.
void split_samples(Plan* p, int S, int L) {
  p->sps = cdiv(L, nt::KC);
  const int want = std::max(1, cdiv(PS_ITEMS_TARGET, p->tiles));
  const int spi_min = cdiv(PS_STAGES_MIN, p->sps);
  p->spi = std::min(S, std::max(cdiv(S, want), spi_min));
  p->slices = cdiv(S, p->spi);
}

// Sizes, operand strides and extents, tiling and sample ranges: what both kinds of product (C per entry, out per sample)
// share.  `who` names the entry points in the error text.
template <typename Desc>
bool tiling_of(const Desc& d, const char* who, int index, Plan* p) {
  if (d.S < 1 || d.M < 1 || d.Nc < 1 || d.L < 1) {
    set_error("%s: item %d: invalid sizes (S %d M %d Nc %d L %d)", who, index, d.S, d.M, d.Nc, d.L);
    return false;
  }
  if ((d.M > 1 && d.a_rs < d.L) || (d.Nc > 1 && d.b_rs < d.L) || d.a_rs < 0 || d.b_rs < 0 || d.a_ns < 0 || d.b_ns < 0) {
    set_error("%s: item %d: invalid strides (a_rs %lld b_rs %lld below L %d, or negative)", who, index, d.a_rs, d.b_rs,
              d.L);
    return false;
  }
  p->a_bytes = ((long long)(d.S - 1) * d.a_ns + (long long)(d.M - 1) * d.a_rs + d.L) * 4;
  p->b_bytes = ((long long)(d.S - 1) * d.b_ns + (long long)(d.Nc - 1) * d.b_rs + d.L) * 4;
  // voffset + soffset of the LDS-DMA reach at most 16 stages' worth behind the operand's end
  if (p->a_bytes >= PS_BYTES_MAX - 4096 || p->b_bytes >= PS_BYTES_MAX - 4096) {
    set_error("%s: item %d: operand too large for 32-bit offsets (%lld / %lld bytes, below %lld)", who, index,
              p->a_bytes, p->b_bytes, PS_BYTES_MAX - 4096);
    return false;
  }
  // a side of at most 64 rows takes 64 x 128 tiles, as the A side of the kernel (the transposed tile when it is Nc)
  p->half = std::min(d.M, d.Nc) <= PS_TM / 2;
  p->swap = p->half && d.M > PS_TM / 2;
  p->tiles_m = p->half ? 1 : cdiv(d.M, PS_TM);
  p->tiles_n = cdiv(p->swap ? d.M : d.Nc, PS_TM);
  const long long tiles = (long long)p->tiles_m * p->tiles_n;
  if (tiles > (1 << 24)) {
    set_error("%s: item %d: too many output tiles (%lld)", who, index, tiles);
    return false;
  }
  p->tiles = (int)tiles;
  split_samples(p, d.S, d.L);
  const int tile_rows = p->half ? PS_TM / 2 : PS_TM;
  p->flops = 2LL * p->tiles * tile_rows * PS_TM * (long long)d.S * p->sps * nt::KC;
  return true;
}

bool plan_of(const curv_persample_desc& d, int index, Plan* p) {
  if (!tiling_of(d, "curv_persample", index, p)) return false;
  if (d.c_rs < d.Nc) {
    set_error("curv_persample: item %d: invalid strides (c_rs %lld below Nc %d)", index, d.c_rs, d.Nc);
    return false;
  }
  const int tile_rows = p->half ? PS_TM / 2 : PS_TM;
  p->slab_bytes = align_up((size_t)p->slices * p->tiles * tile_rows * PS_TM * sizeof(float), 256);
  return true;
}

// (`slab_bytes`: the partials, one float per output tile and sample)
bool quad_plan_of(const curv_persample_quad_desc& d, int index, Plan* p) {
  if (!tiling_of(d, "curv_persample_quad", index, p)) return false;
  // every staged row starts on a 16-byte boundary: the only form the library's own operands take and the only one tested
  if (((d.a_ns | d.a_rs | d.b_ns | d.b_rs) & 3) != 0) {
    set_error("curv_persample_quad: item %d: operand strides must be multiples of 4 floats (a_ns %lld a_rs %lld b_ns %lld "
              "b_rs %lld)", index, d.a_ns, d.a_rs, d.b_ns, d.b_rs);
    return false;
  }
  if ((d.W != nullptr && d.w_rs < d.Nc) || d.o_stride < 1) {
    set_error("curv_persample_quad: item %d: invalid strides (w_rs %lld below Nc %d, or o_stride %lld below 1)", index,
              d.w_rs, d.Nc, d.o_stride);
    return false;
  }
  p->slab_bytes = align_up((size_t)p->tiles * d.S * sizeof(float), 256);
  return true;
}

// (`slab_bytes`: the partials, H floats per output tile and sample; tiling and FLOPs are those of quad_plan_of)
bool grid_plan_of(const curv_persample_grid_desc& d, int index, Plan* p) {
  const char* const who = "curv_persample_quad_grid";
  if (d.H < 1 || d.H > GRID_MAX) {
    set_error("%s: item %d: H %d outside 1 .. %d", who, index, d.H, GRID_MAX);
    return false;
  }
  if (!d.shift || !d.gain) {
    set_error("%s: item %d: null shift or gain (host arrays of H floats)", who, index);
    return false;
  }
  for (int h = 0; h < d.H; ++h)
    if (!(d.shift[h] > 0.0f) || !std::isfinite(d.shift[h]) || !std::isfinite(d.gain[h])) {
      set_error("%s: item %d: grid point %d: shift %g must be finite and > 0, gain %g finite", who, index, h,
                (double)d.shift[h], (double)d.gain[h]);
      return false;
    }
  if (!tiling_of(d, who, index, p)) return false;
  if (((d.a_ns | d.a_rs | d.b_ns | d.b_rs) & 3) != 0) {
    set_error("%s: item %d: operand strides must be multiples of 4 floats (a_ns %lld a_rs %lld b_ns %lld b_rs %lld)", who,
              index, d.a_ns, d.a_rs, d.b_ns, d.b_rs);
    return false;
  }
  if ((d.V != nullptr && d.v_rs < d.Nc) || d.o_stride < 1 || (d.H > 1 && d.o_hs < 1)) {
    set_error("%s: item %d: invalid strides (v_rs %lld below Nc %d, o_stride %lld or o_hs %lld below 1)", who, index,
              d.v_rs, d.Nc, d.o_stride, d.o_hs);
    return false;
  }
  p->slab_bytes = align_up((size_t)p->tiles * d.S * d.H * sizeof(float), 256);
  return true;
}

// (`slab_bytes`: the partials, K (K + 1) / 2 floats per output tile and sample; the tiling is ps_cov_tile's)
bool cov_plan_of(const curv_persample_cov_desc& d, int index, Plan* p) {
  const char* const who = "curv_persample_cov";
  if (d.K < 1 || d.K > COV_K_MAX) {
    set_error("%s: item %d: K %d outside 1 .. %d", who, index, d.K, COV_K_MAX);
    return false;
  }
  if (!tiling_of(d, who, index, p)) return false;
  if (((d.a_cs | d.a_ns | d.a_rs | d.b_ns | d.b_rs) & 3) != 0 || d.a_cs < 0) {
    set_error("%s: item %d: operand strides must be multiples of 4 floats (a_cs %lld a_ns %lld a_rs %lld b_ns %lld b_rs "
              "%lld), a_cs not negative", who, index, d.a_cs, d.a_ns, d.a_rs, d.b_ns, d.b_rs);
    return false;
  }
  if (d.a_cs >= PS_BYTES_MAX) p->a_bytes = PS_BYTES_MAX;
  else p->a_bytes += (long long)(d.K - 1) * d.a_cs * 4;
  if (p->a_bytes >= PS_BYTES_MAX - 4096) {
    set_error("%s: item %d: operand too large for 32-bit offsets (%lld bytes over %d outputs, below %lld)", who, index,
              p->a_bytes, d.K, PS_BYTES_MAX - 4096);
    return false;
  }
  if ((d.W != nullptr && d.w_rs < d.Nc) || d.o_rs < d.K || d.o_ns < (long long)d.K * d.o_rs) {
    set_error("%s: item %d: invalid strides (w_rs %lld below Nc %d, o_rs %lld below K %d, or o_ns %lld below K o_rs)", who,
              index, d.w_rs, d.Nc, d.o_rs, d.K, d.o_ns);
    return false;
  }
  p->half = p->swap = 0;
  p->tiles_m = cdiv(d.M, COV_TI);
  p->tiles_n = cdiv(d.Nc, PS_TM);
  const long long tiles = (long long)p->tiles_m * p->tiles_n;
  if (tiles > (1 << 24)) {
    set_error("%s: item %d: too many output tiles (%lld)", who, index, tiles);
    return false;
  }
  p->tiles = (int)tiles;
  split_samples(p, d.S, d.L);
  const int groups = cdiv(d.K, 4), pairs = d.K * (d.K + 1) / 2;
  p->flops = 2LL * p->tiles * (4 * groups * COV_TI) * PS_TM * (long long)d.S * p->sps * nt::KC;
  p->slab_bytes = align_up((size_t)p->tiles * d.S * pairs * sizeof(float), 256);
  return true;
}

// (`slab_bytes`: the partials, one Nc x R block per sample and 64-row part.)  This product never changes its operands'
// places: W and U belong to the rows of A.  M <= 64 takes the half tile, anything else the full one, whatever Nc is.
bool project_plan_of(const curv_persample_project_desc& d, int index, Plan* p) {
  const char* const who = "curv_persample_project";
  if (d.R < 1) {
    set_error("%s: item %d: R %d below 1", who, index, d.R);
    return false;
  }
  if (!tiling_of(d, who, index, p)) return false;
  if (((d.a_ns | d.a_rs | d.b_ns | d.b_rs) & 3) != 0) {
    set_error("%s: item %d: operand strides must be multiples of 4 floats (a_ns %lld a_rs %lld b_ns %lld b_rs %lld)", who,
              index, d.a_ns, d.a_rs, d.b_ns, d.b_rs);
    return false;
  }
  if (d.w_rs < d.Nc || d.u_rs < d.R || d.z_cs < 1 || d.z_rs < 1 || d.z_ns < 1) {
    set_error("%s: item %d: invalid strides (w_rs %lld below Nc %d, u_rs %lld below R %d, or z_ns %lld z_rs %lld z_cs %lld "
              "below 1)", who, index, d.w_rs, d.Nc, d.u_rs, d.R, d.z_ns, d.z_rs, d.z_cs);
    return false;
  }
  // U and a partial block are addressed by 32-bit byte offsets that reach a tile's worth behind their last row
  if (d.M > 1 && ((long long)d.M + PS_TM) * d.u_rs * 4 >= PS_BYTES_MAX) {
    set_error("%s: item %d: U too large for 32-bit offsets ((M %d + %d) rows of u_rs %lld floats)", who, index, d.M, PS_TM,
              d.u_rs);
    return false;
  }
  if (((long long)d.Nc + PS_TM) * d.R * 4 >= PS_BYTES_MAX) {
    set_error("%s: item %d: Nc x R block too large for 32-bit offsets (Nc %d R %d)", who, index, d.Nc, d.R);
    return false;
  }
  p->half = d.M <= PS_TM / 2;
  p->swap = 0;
  p->tiles_m = p->half ? 1 : cdiv(d.M, PS_TM);
  p->tiles_n = cdiv(d.Nc, PS_TM);
  const long long tiles = (long long)p->tiles_m * p->tiles_n;
  if (tiles > (1 << 24)) {
    set_error("%s: item %d: too many output tiles (%lld)", who, index, tiles);
    return false;
  }
  p->tiles = (int)tiles;
  split_samples(p, d.S, d.L);
  p->parts = p->half ? 1 : 2 * p->tiles_m;
  const int tile_rows = p->half ? PS_TM / 2 : PS_TM;
  // the products, and at every sample's end the second MFMA: tile_rows x 128 entries against ceil(R / 32) chunks of U
  p->flops = 2LL * p->tiles * tile_rows * PS_TM * (long long)d.S * ((long long)p->sps * nt::KC + 32LL * cdiv(d.R, 32));
  p->slab_bytes = align_up((size_t)d.S * p->parts * d.Nc * d.R * sizeof(float), 256);
  return true;
}

// Product: one workgroup per item = (tile * slices + slice) of one product.  Full tiles (128 x 128): wave (wm, wn) computes
// rows 64 wm .. + 64 of the A panel against rows 64 wn .. + 64 of the B panel, 2 x 2 MFMA blocks.  Half tiles (64 x 128, a
// product whose A side has at most 64 rows): every wave takes all 64 A rows against B rows 32 wave .. + 32, 2 x 1 blocks -
// half the MFMAs per stage instead of a half-empty tile.  C/D map of a 32x32 block: column = lane & 31, row = (reg & 3) +
// 8 (reg >> 2) + 4 (lane >> 5).
//
// What becomes of P_n at the end of a sample is the MODE.  PS_SQ (d a PsProduct): P_n**2 is added per entry into a second
// accumulator set, which goes to the item's slab.  PS_QUAD_W / PS_QUAD_ONES (d a PsQuad): sum_ij W_ij P_n[i][j]**2 over the
// tile - the second register set holds the lane's share of the W tile instead, loaded once per item, with zeros for the
// rows and columns at or beyond M / Nc (W is not read for them); without W nothing is held and those entries are masked
// by their index.  The lane sums its 64 entries, the wave reduces by butterfly, lane 0 of each wave leaves the wave's sum
// in red[sample parity][wave], and behind the next barrier (the next stage's, or one after the last stage) thread 0 adds
// the four in wave order and writes partial[tile][sample]: no barrier of its own, fixed order, no atomics.  The parity
// keeps the waves that run ahead into the next sample's end off the four values thread 0 is still reading.
// PS_GRID_SEP / PS_GRID_DENSE (d a PsGrid): the same sum for H grid points in turn, w_h = 1 / ((u_i + shift_h)(v_j +
// shift_h)) or 1 / (V_ij + shift_h).  The second register set holds what the weights are made of, loaded once per item:
// the lane's 32 u values (its rows) and, beside it, its 2 (half tiles: 1) v values, or its share of the V tile - with
// +inf for rows and columns at or beyond M / Nc (not read), whose weight is then 1 / inf = 0.  At the sample's end the
// lane squares its accumulators in place, once, and for h = 0 .. H - 1 (a loop that is not unrolled: one h is live at a
// time) divides, sums - 34 divisions per h in the separable form, 64 in the dense one - and reduces over the wave by DPP
// (wave_sum.h); lane 63 leaves red[sample parity][wave][h], thread h adds the four behind the next barrier and writes
// partial[tile][sample][h].  Grid point h sees shift[h] only: its bits do not depend on the other grid points.
// PS_PROJECT (d a PsProject): Z_n = (W o P_n)^T U.  The second register set holds W as in PS_QUAD_W.  At the sample's end
// the lane multiplies its accumulators by W in place; what it then holds is, register by register, the A operand of
// another v_mfma_f32_32x32x2_f32: lane (r32, h) has column r32 and row 4 h + roff(m, reg) of the block, and the MFMA
// wants A[i = lane & 31][k = lane >> 5] - so with i = the column and the two k of step (m, reg) = the rows 4 h + roff(m,
// reg), h = 0, 1, the 32 steps of a wave sum its 64 rows, the B operand of a step being U[row][32 lb + r32], read from
// memory (zero, and not read, for rows at or beyond M and columns at or beyond R).  R is walked in chunks lb of 32
// columns (a loop that is not unrolled): 16 BN registers of z per lane.  The result block (column j = 4 h + roff(reg),
// l = 32 lb + r32) goes straight to the wave's partial block; no LDS, no barrier, no hand-over.
enum { PS_SQ = 0, PS_QUAD_W = 1, PS_QUAD_ONES = 2, PS_GRID_SEP = 3, PS_GRID_DENSE = 4, PS_PROJECT = 5 };

// An item of a product launch: its output tile and its range of samples.
struct PsItem {
  int tile, tm, tn, slice;
};
__device__ __forceinline__ PsItem ps_item_of(const PsOperands& d, int local) {
  PsItem it;
  it.slice = local % d.slices;
  it.tile = local / d.slices;
  it.tm = it.tile / d.tiles_n;
  it.tn = it.tile - it.tm * d.tiles_n;
  return it;
}

// The walk over the stages of an item's samples, which all three product tiles share: the stages of samples
// [slice spi, ...) form ONE sequence on the stage engine (nt_stage.h; the prefetch runs across sample boundaries), a
// stage being 32 l values of one sample; the last stage of a sample whose L is no multiple of 32 is the engine's tail
// stage.  The client has filled dma.voff_a / voff_b (the sample and l of a stage travel as soffsets) and brings the
// accumulators c[NA][NB] (not reset here) and two hooks: sample_end(n) right behind the last stage of sample n - P_n is
// complete in c - and flush(n) behind the next barrier after it, the next stage's.  Returns the sample whose flush is
// still due (the item's last), or -1.
template <int NA, int NB, int PA, typename SampleEnd, typename Flush>
__device__ __forceinline__ int ps_walk_samples(const PsOperands& d, int slice, const nt::Dma<PA>& dma,
                                               const unsigned (&addr_a)[NA][nt::STEPS],
                                               const unsigned (&addr_b)[NB][nt::STEPS], f32x16 (&c)[NA][NB], int h,
                                               SampleEnd sample_end, Flush flush) {
  const int L = d.L, s0 = slice * d.spi, s1 = min(s0 + d.spi, d.S);
  const int n_stages = (s1 - s0) * ((L + nt::KC - 1) / nt::KC);
  int n = s0, kk = 0;                                       // sample and first l of the running stage
  int pending = -1;                                         // the sample whose flush is due
  if (n_stages > 0)
    dma.issue_first(dma.live(0, L), (unsigned)((long long)n * d.a_ns * 4), (unsigned)((long long)n * d.b_ns * 4));
  for (int t = 0; t < n_stages; ++t) {
    nt::stage_landed();
    if (pending >= 0) flush(pending);
    pending = -1;
    int kn = kk + nt::KC, nn = n;
    const bool sample_ends = kn >= L;
    if (sample_ends) { kn = 0; ++nn; }
    const bool live_n = t + 1 < n_stages && dma.live(kn, L);
    const unsigned sa = (unsigned)(((long long)nn * d.a_ns + kn) * 4), sb = (unsigned)(((long long)nn * d.b_ns + kn) * 4);
    nt::stage<NA, NB, PA + nt::PIECES>(c, addr_a, addr_b, dma.lds, t, L - kk, h,
                                       [&](int i, unsigned nbuf) { dma.issue(i, live_n, sa, sb, nbuf); });
    if (sample_ends) {
      sample_end(n);
      pending = n;
    }
    n = nn;
    kk = kn;
  }
  return pending;
}

template <bool HALF, int MODE, typename Product>
__device__ __forceinline__ void ps_product_tile(const Product& d, int local, lds_char_t* lds, float* red) {
  constexpr int BN = HALF ? 1 : 2;                         // MFMA blocks per wave along the B side
  constexpr int TA = HALF ? PS_TM / 2 : PS_TM;             // A rows per tile
  constexpr int PA = TA / nt::RPP / 4;                     // DMA pieces per wave of the A panel
  const PsItem it = ps_item_of(d, local);
  const int i0 = it.tm * TA, j0 = it.tn * PS_TM, M = d.M, N = d.Nc;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  const int row_a = HALF ? 0 : 64 * (wave >> 1), row_b = HALF ? 32 * wave : 64 * (wave & 1);

  // rows beyond the matrix are clamped to its last row (their results are never stored, and the PS_QUAD modes leave them
  // out of the sums)
  nt::Dma<PA> dma(d.A, d.a_bytes, d.B, d.b_bytes, lds, wave, lane);
#pragma unroll
  for (int p = 0; p < PA; ++p) dma.voff_a[p] = dma.row_voff(i0, p, M, d.a_rs);
#pragma unroll
  for (int p = 0; p < nt::PIECES; ++p) dma.voff_b[p] = dma.row_voff(j0, p, N, d.b_rs);
  unsigned addr_a[2][nt::STEPS], addr_b[BN][nt::STEPS];
#pragma unroll
  for (int m = 0; m < 2; ++m) nt::read_addrs(addr_a[m], row_a + 32 * m + r32, false, h);
#pragma unroll
  for (int nb = 0; nb < BN; ++nb) nt::read_addrs(addr_b[nb], row_b + 32 * nb + r32, true, h);
  f32x16 c[2][BN], q[2][BN];       // P_n of the running sample; the sum of P_n**2 over the finished samples (PS_QUAD_W: W)
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nb = 0; nb < BN; ++nb) { c[m][nb] = 0.0f; q[m][nb] = 0.0f; }
  // entry (m, nb, reg) of this lane is row i0 + row_a + 4 h + roff(m, reg), column j0 + row_b + 32 nb + r32 of the product
  auto roff = [](int m, int reg) { return 32 * m + (reg & 3) + 8 * (reg >> 2); };
  const int rows_left = M - (i0 + row_a + 4 * h);            // the entry is inside the product iff roff < rows_left ...
  bool col_in[BN];                                           // ... and col_in[nb]
#pragma unroll
  for (int nb = 0; nb < BN; ++nb) col_in[nb] = j0 + row_b + 32 * nb + r32 < N;
  if constexpr (MODE == PS_QUAD_W || MODE == PS_PROJECT) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nb = 0; nb < BN; ++nb)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const long long at = (long long)(i0 + row_a + 4 * h + roff(m, reg)) * d.w_is + (long long)(j0 + row_b + 32 * nb + r32) * d.w_js;
          if (roff(m, reg) < rows_left && col_in[nb]) q[m][nb][reg] = d.W[at];
        }
  }
  float vcol[BN];                                            // PS_GRID_SEP: v of the lane's columns (u is in q[m][0])
  if constexpr (MODE == PS_GRID_SEP) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        q[m][0][reg] = roff(m, reg) < rows_left ? d.u[i0 + row_a + 4 * h + roff(m, reg)] : __builtin_inff();
#pragma unroll
    for (int nb = 0; nb < BN; ++nb) vcol[nb] = col_in[nb] ? d.v[j0 + row_b + 32 * nb + r32] : __builtin_inff();
  }
  if constexpr (MODE == PS_GRID_DENSE) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nb = 0; nb < BN; ++nb)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const long long at = (long long)(i0 + row_a + 4 * h + roff(m, reg)) * d.v_is + (long long)(j0 + row_b + 32 * nb + r32) * d.v_js;
          q[m][nb][reg] = (roff(m, reg) < rows_left && col_in[nb]) ? d.V[at] : __builtin_inff();
        }
  }

  if constexpr (MODE == PS_SQ) {
    // the sample boundary: square the tile of P_n, add it to the running sum, start the next sample from zero
    auto sample_end = [&](int) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < BN; ++nb) {
          q[m][nb] += c[m][nb] * c[m][nb];
          c[m][nb] = 0.0f;
        }
    };
    ps_walk_samples(d, it.slice, dma, addr_a, addr_b, c, h, sample_end, [](int) {});
    // raw partial tile, row-major TA x 128, to this item's slab (every entry is written)
    gfl* slab = (gfl*)d.slabs + (long long)local * (TA * PS_TM);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nb = 0; nb < BN; ++nb) {
        const int col = row_b + 32 * nb + r32;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int r = row_a + 32 * m + (reg & 3) + 8 * (reg >> 2) + 4 * h;
          slab[r * PS_TM + col] = q[m][nb][reg];
        }
      }
  } else if constexpr (MODE == PS_PROJECT) {
    const int R = d.R, chunks = (R + 31) >> 5;
    const int part = HALF ? 0 : 2 * it.tm + (wave >> 1);
    // U and the partial block through buffer descriptors, the whole offset in the voffset (the range check does not see
    // an soffset): rows at or beyond M (of U) and columns at or beyond Nc (of the block) fall behind the descriptor's
    // extent - the load gives 0, the store is dropped - and a lane whose l is at or beyond R carries an out-of-range
    // voffset, which the row offsets cannot bring back into range (project_plan_of bounds them)
    constexpr int OOB = (int)0x80000000;
    const unsigned u_bytes = (unsigned)(((long long)(M - 1) * d.u_rs + R) * 4), z_bytes = (unsigned)((long long)N * R * 4);
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc((void*)d.U, 0, u_bytes, 0x00020000);
    const int u_row = (int)d.u_rs * 4, z_row = R * 4;
    const int u_lane = ((i0 + row_a + 4 * h) * (int)d.u_rs + r32) * 4, z_lane = ((j0 + row_b + 4 * h) * R + r32) * 4;
    // the sample boundary: W o P_n in place, then its 64 rows against U, 32 columns of U at a time
    auto sample_end = [&](int n) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < BN; ++nb) c[m][nb] = c[m][nb] * q[m][nb];
      float* block = d.partial + ((long long)n * d.parts + part) * ((long long)N * R);
      const __amdgpu_buffer_rsrc_t rsz = __builtin_amdgcn_make_buffer_rsrc((void*)block, 0, z_bytes, 0x00020000);
#pragma unroll 1
      for (int lb = 0; lb < chunks; ++lb) {
        const bool l_in = 32 * lb + r32 < R;
        const int u_at = l_in ? u_lane + 128 * lb : OOB, z_at = l_in ? z_lane + 128 * lb : OOB;
        f32x16 z[BN];
#pragma unroll
        for (int nb = 0; nb < BN; ++nb) z[nb] = 0.0f;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const float u = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsu, u_at + roff(m, reg) * u_row, 0, 0));
#pragma unroll
            for (int nb = 0; nb < BN; ++nb) z[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(c[m][nb][reg], u, z[nb], 0, 0, 0);
          }
#pragma unroll
        for (int nb = 0; nb < BN; ++nb)
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const float v = z[nb][reg];          // (a bit cast of the vector element itself stores element 0 sixteen times)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsz,
                                                  z_at + (32 * nb + roff(0, reg)) * z_row, 0, 0);
          }
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < BN; ++nb) c[m][nb] = 0.0f;
    };
    ps_walk_samples(d, it.slice, dma, addr_a, addr_b, c, h, sample_end, [](int) {});
  } else if constexpr (MODE == PS_GRID_SEP || MODE == PS_GRID_DENSE) {
    const int H = d.H;
    auto flush = [&](int n) {
      if (tid < H) {
        const float* r = red + 4 * GRID_MAX * (n & 1) + tid;
        d.partial[((long long)it.tile * d.S + n) * H + tid] = ((r[0] + r[GRID_MAX]) + r[2 * GRID_MAX]) + r[3 * GRID_MAX];
      }
    };
    // the sample boundary: P_n**2 in place, then the weighted sum over the tile for one grid point after the other
    auto sample_end = [&](int n) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < BN; ++nb) c[m][nb] = c[m][nb] * c[m][nb];
      float* r = red + 4 * GRID_MAX * (n & 1) + GRID_MAX * wave;
#pragma unroll 1
      for (int g = 0; g < H; ++g) {
        const float sh = d.shift[g];
        float v = 0.0f;
        if constexpr (MODE == PS_GRID_SEP) {
          float acc[BN];                                       // per column: sum_i P_ij**2 / (u_i + shift)
#pragma unroll
          for (int nb = 0; nb < BN; ++nb) acc[nb] = 0.0f;
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
              const float ru = 1.0f / (q[m][0][reg] + sh);
#pragma unroll
              for (int nb = 0; nb < BN; ++nb) acc[nb] = __builtin_fmaf(ru, c[m][nb][reg], acc[nb]);
            }
#pragma unroll
          for (int nb = 0; nb < BN; ++nb) v = __builtin_fmaf(1.0f / (vcol[nb] + sh), acc[nb], v);
        } else {
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nb = 0; nb < BN; ++nb) {
              float acc = 0.0f;                                // one chain per MFMA block, the blocks added in order
#pragma unroll
              for (int reg = 0; reg < 16; ++reg) acc = __builtin_fmaf(1.0f / (q[m][nb][reg] + sh), c[m][nb][reg], acc);
              v += acc;
            }
        }
        v = wave_sum_dpp(v);
        if (lane == 63) r[g] = v;
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < BN; ++nb) c[m][nb] = 0.0f;
    };
    const int last = ps_walk_samples(d, it.slice, dma, addr_a, addr_b, c, h, sample_end, flush);
    __syncthreads();                 // the wave sums of the item's last sample
    if (last >= 0) flush(last);
  } else {
    auto flush = [&](int n) {
      if (tid == 0) {
        const float* r = red + 4 * (n & 1);
        d.partial[(long long)it.tile * d.S + n] = ((r[0] + r[1]) + r[2]) + r[3];
      }
    };
    // the sample boundary: sum the (weighted) squares of P_n over the tile, this lane's 64 entries first
    auto sample_end = [&](int n) {
      float v = 0.0f;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < BN; ++nb) {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const float p = c[m][nb][reg];
            if constexpr (MODE == PS_QUAD_W) v += q[m][nb][reg] * p * p;
            else v += (roff(m, reg) < rows_left && col_in[nb]) ? p * p : 0.0f;
          }
          c[m][nb] = 0.0f;
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0) red[4 * (n & 1) + wave] = v;
    };
    const int last = ps_walk_samples(d, it.slice, dma, addr_a, addr_b, c, h, sample_end, flush);
    __syncthreads();                 // the wave sums of the item's last sample
    if (last >= 0) flush(last);
  }
}

__global__ void __launch_bounds__(PS_THREADS, 2) ps_product_kernel(const PsBatch batch) {
  __shared__ __attribute__((aligned(1024))) char smem[nt::LDS_B];
  const PsProduct& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)(blockIdx.x - d.base);
  if (d.half) ps_product_tile<true, PS_SQ>(d, local, (lds_char_t*)smem, nullptr);
  else ps_product_tile<false, PS_SQ>(d, local, (lds_char_t*)smem, nullptr);
}

// The same items for curv_persample_quad_reduce: partial[tile][sample] instead of a slab.
__global__ void __launch_bounds__(PS_THREADS, 2) ps_quad_product_kernel(const PsQuadBatch batch) {
  __shared__ __attribute__((aligned(1024))) char smem[nt::LDS_B];
  __shared__ float red[8];                                                  // [sample parity][wave]
  const PsQuad& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)(blockIdx.x - d.base);
  if (d.half) {
    if (d.W) ps_product_tile<true, PS_QUAD_W>(d, local, (lds_char_t*)smem, red);
    else ps_product_tile<true, PS_QUAD_ONES>(d, local, (lds_char_t*)smem, red);
  } else {
    if (d.W) ps_product_tile<false, PS_QUAD_W>(d, local, (lds_char_t*)smem, red);
    else ps_product_tile<false, PS_QUAD_ONES>(d, local, (lds_char_t*)smem, red);
  }
}

// Reduce: one thread per sample sums the partials of its product in tile order, scales, writes or adds.  Blocks of a
// product: ceil(S / 256).
__global__ void __launch_bounds__(PS_THREADS) ps_quad_reduce_kernel(const PsQuadBatch batch) {
  const PsQuad& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long s = (blockIdx.x - d.base) * PS_THREADS + threadIdx.x;
  if (s >= d.S) return;
  float v = 0.f;
#pragma unroll 8
  for (int t = 0; t < d.tiles; ++t) v += d.partial[(long long)t * d.S + s];
  v *= d.alpha;
  float* out = d.out + s * d.o_stride;
  *out = d.first ? v : *out + v;
}

// The same items for curv_persample_quad_grid_reduce: partial[tile][sample][h].
__global__ void __launch_bounds__(PS_THREADS, 2) ps_grid_product_kernel(const PsGridBatch batch) {
  __shared__ __attribute__((aligned(1024))) char smem[nt::LDS_B];
  __shared__ float red[2 * 4 * GRID_MAX];                                   // [sample parity][wave][h]
  const PsGrid& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)(blockIdx.x - d.base);
  if (d.half) {
    if (d.V) ps_product_tile<true, PS_GRID_DENSE>(d, local, (lds_char_t*)smem, red);
    else ps_product_tile<true, PS_GRID_SEP>(d, local, (lds_char_t*)smem, red);
  } else {
    if (d.V) ps_product_tile<false, PS_GRID_DENSE>(d, local, (lds_char_t*)smem, red);
    else ps_product_tile<false, PS_GRID_SEP>(d, local, (lds_char_t*)smem, red);
  }
}

// Reduce: one thread per (sample, h) sums the partials of its product in tile order, applies gain[h], writes or adds.
// Blocks of a product: ceil(S H / 256).
__global__ void __launch_bounds__(PS_THREADS) ps_grid_reduce_kernel(const PsGridBatch batch) {
  const PsGrid& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long idx = (blockIdx.x - d.base) * PS_THREADS + threadIdx.x;
  const long long step = (long long)d.S * d.H;
  if (idx >= step) return;
  const long long s = idx / d.H;
  const int g = (int)(idx - s * d.H);
  const float* p = d.partial + idx;
  float v = 0.f;
#pragma unroll 8
  for (int t = 0; t < d.tiles; ++t) v += p[t * step];
  v *= d.gain[g];
  float* out = d.out + g * d.o_hs + s * d.o_stride;
  *out = d.first ? v : *out + v;
}

// The same items for curv_persample_project: partial[sample][part][Nc][R] instead of a slab.
__global__ void __launch_bounds__(PS_THREADS, 2) ps_project_product_kernel(const PsProjectBatch batch) {
  __shared__ __attribute__((aligned(1024))) char smem[nt::LDS_B];
  const PsProject& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)(blockIdx.x - d.base);
  if (d.half) ps_product_tile<true, PS_PROJECT>(d, local, (lds_char_t*)smem, nullptr);
  else ps_product_tile<false, PS_PROJECT>(d, local, (lds_char_t*)smem, nullptr);
}

// Reduce: one thread per entry (n, j, l) of Z sums the parts of its sample in part order (row tiles, the two wave rows
// of each), scales, writes or adds.  Blocks of a product: ceil(S Nc R / 256).
__global__ void __launch_bounds__(PS_THREADS) ps_project_reduce_kernel(const PsProjectBatch batch) {
  const PsProject& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long idx = (blockIdx.x - d.base) * PS_THREADS + threadIdx.x;
  const long long block = (long long)d.Nc * d.R;
  if (idx >= d.S * block) return;
  const long long s = idx / block, rem = idx - s * block;
  const int j = (int)(rem / d.R), l = (int)(rem - (long long)j * d.R);
  const float* p = d.partial + s * d.parts * block + rem;
  float v = 0.f;
#pragma unroll 4
  for (int t = 0; t < d.parts; ++t) v += p[t * block];
  v *= d.alpha;
  float* out = d.Z + s * d.z_ns + j * d.z_rs + l * d.z_cs;
  *out = d.first ? v : *out + v;
}

// ------------------------------------------------------------------------------------------------ joint covariance
// The third reduction of the same products (curv_persample_cov_reduce): a Gram over K outputs, per sample,
//   out[s][c][c'] (+)= alpha * sum_ij W[i][j] * P_{s,c}[i][j] * P_{s,c'}[i][j],   P_{s,c} = A_{c,s} B_s^T.
// Item = (product, tile of COV_TI = 8 rows i x 128 columns j, range of samples).  The A panel of a stage holds the 8 rows
// of ALL outputs, as rows (group of four outputs, i, output in the group): panel row 32 m + 4 i + c is row i0 + i of
// output 4 m + c (the DMA's voffset is per row, so the order costs nothing); the B panel is K9's 128 rows, staged once
// per stage and used against every output.  Wave w takes all 32 KG A rows (KG = ceil(K / 4) MFMA blocks) against B rows
// 32 w .. + 32.  With the 32x32 C/D map (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) register `reg` of block m is
// output 4 m + (reg & 3) of row i0 + 2 (reg >> 2) + (lane >> 5), column j0 + 32 w + (lane & 31): a lane holds every
// output of its four (i, j) in its own registers, and the Gram over outputs is lane-local - for each pair c <= c' four
// multiply-adds, with the lane's four weights (W, or 1; 0 for i >= M or j >= Nc, where W is not read) folded into the
// first factor.  Outputs c >= K of the last group and rows beyond M are staged from a clamped (valid) row and never
// counted.
//
// At a sample's end every pair is summed over the wave by DPP: four row steps (quad_perm, quad_perm, row_half_mirror,
// row_mirror), then row_bcast:15 and row_bcast:31, i.e. six VALU instructions and no LDS traffic per value, where the
// butterfly of K9 costs six ds_bpermute round trips (up to 136 values per sample make that the larger part of a sample of
// two stages) and a transposing pass through LDS would need 34 KiB per wave beside the panels.  Lane 63 leaves the wave's
// sum in red[sample parity][wave][pair]; behind the next barrier thread `pair` adds the four in wave order and writes
// partial[tile][sample][pair] (K9's hand-over, K (K + 1) / 2 threads wide): fixed order, no atomics.
// (wave_sum_dpp: wave_sum.h)
template <int KG>
__device__ __forceinline__ void ps_cov_tile(const PsCov& d, int local, lds_char_t* lds, float* red) {
  const PsItem it = ps_item_of(d, local);
  const int i0 = it.tm * COV_TI, j0 = it.tn * PS_TM, M = d.M, N = d.Nc, K = d.K;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;

  // piece m of the A panel is group m: row rsub of it is output 4 m + (rsub & 3) of row i0 + (rsub >> 2), both clamped
  // to the last valid one
  nt::Dma<KG> dma(d.A, d.a_bytes, d.B, d.b_bytes, lds, wave, lane);
#pragma unroll
  for (int p = 0; p < KG; ++p)
    dma.voff_a[p] = (int)(((long long)min(4 * p + (dma.rsub & 3), K - 1) * d.a_cs +
                           (long long)min(i0 + (dma.rsub >> 2), M - 1) * d.a_rs + 4 * dma.g_lane) * 4);
#pragma unroll
  for (int p = 0; p < nt::PIECES; ++p) dma.voff_b[p] = dma.row_voff(j0, p, N, d.b_rs);
  unsigned addr_a[KG][nt::STEPS], addr_b[1][nt::STEPS];
  f32x16 c[KG][1];                 // P_{n,c} of the running sample: c[m][0][4 q + cl] = output 4 m + cl, row i0 + 2 q + h
#pragma unroll
  for (int m = 0; m < KG; ++m) {
    nt::read_addrs(addr_a[m], 32 * m + r32, false, h);
    c[m][0] = 0.0f;
  }
  nt::read_addrs(addr_b[0], 32 * wave + r32, true, h);
  float wq[4];                     // the weights of the lane's four entries (row i0 + 2 q + h, column `col`)
  {
    const int col = j0 + 32 * wave + r32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + 2 * q + h;
      const bool in = i < M && col < N;
      wq[q] = in ? 1.0f : 0.0f;
      if (in && d.W) wq[q] = d.W[(long long)i * d.w_rs + col];
    }
  }
  auto flush = [&](int n) {
    if (tid < d.pairs) {
      const float* r = red + 4 * COV_PAIRS_MAX * (n & 1) + tid;
      d.partial[((long long)it.tile * d.S + n) * d.pairs + tid] =
          ((r[0] + r[COV_PAIRS_MAX]) + r[2 * COV_PAIRS_MAX]) + r[3 * COV_PAIRS_MAX];
    }
  };
  // the sample boundary: the weighted Gram of the lane's entries over the outputs, pair by pair, summed over the wave
  auto sample_end = [&](int n) {
    float* r = red + 4 * COV_PAIRS_MAX * (n & 1) + COV_PAIRS_MAX * wave;
    int pair = 0;
#pragma unroll
    for (int ca = 0; ca < 4 * KG; ++ca) {
      if (ca < K) {
        float ta[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ta[q] = wq[q] * c[ca >> 2][0][4 * q + (ca & 3)];
#pragma unroll
        for (int cb = ca; cb < 4 * KG; ++cb) {
          if (cb < K) {
            float v = ta[0] * c[cb >> 2][0][cb & 3];
#pragma unroll
            for (int q = 1; q < 4; ++q) v = __builtin_fmaf(ta[q], c[cb >> 2][0][4 * q + (cb & 3)], v);
            v = wave_sum_dpp(v);
            if (lane == 63) r[pair] = v;
            ++pair;
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < KG; ++m) c[m][0] = 0.0f;
  };
  const int last = ps_walk_samples(d, it.slice, dma, addr_a, addr_b, c, h, sample_end, flush);
  __syncthreads();                   // the wave sums of the item's last sample
  if (last >= 0) flush(last);
}

__global__ void __launch_bounds__(PS_THREADS, 2) ps_cov_product_kernel(const PsCovBatch batch) {
  __shared__ __attribute__((aligned(1024))) char smem[nt::LDS_B];
  __shared__ float red[2 * 4 * COV_PAIRS_MAX];                             // [sample parity][wave][pair]
  const PsCov& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int local = (int)(blockIdx.x - d.base);
  switch ((d.K + 3) >> 2) {
    case 1: ps_cov_tile<1>(d, local, (lds_char_t*)smem, red); break;
    case 2: ps_cov_tile<2>(d, local, (lds_char_t*)smem, red); break;
    case 3: ps_cov_tile<3>(d, local, (lds_char_t*)smem, red); break;
    default: ps_cov_tile<4>(d, local, (lds_char_t*)smem, red); break;
  }
}

// Reduce: one thread per (sample, pair c <= c') sums the partials of its product in tile order, scales, writes or adds,
// and stores the one value at [c][c'] and [c'][c].  Blocks of a product: ceil(S K (K + 1) / 2 / 256).
__global__ void __launch_bounds__(PS_THREADS) ps_cov_reduce_kernel(const PsCovBatch batch) {
  const PsCov& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const long long idx = (blockIdx.x - d.base) * PS_THREADS + threadIdx.x;
  if (idx >= (long long)d.S * d.pairs) return;
  const long long s = idx / d.pairs;
  const int pair = (int)(idx - s * d.pairs);
  int ca = 0, left = pair;
  while (left >= d.K - ca) { left -= d.K - ca; ++ca; }
  const int cb = ca + left;
  const long long step = (long long)d.S * d.pairs;
  const float* p = d.partial + idx;
  float v = 0.f;
#pragma unroll 8
  for (int t = 0; t < d.tiles; ++t) v += p[t * step];
  v *= d.alpha;
  float* out = d.out + s * d.o_ns;
  if (!d.first) v = out[ca * d.o_rs + cb] + v;
  out[ca * d.o_rs + cb] = v;
  out[cb * d.o_rs + ca] = v;
}

// Reduce: one thread per entry (i, j) of C; it sums the slab entries of its tile in slice order, scales, writes or adds.
// Blocks of a product: ceil(M Nc / 256).
__global__ void __launch_bounds__(PS_THREADS) ps_reduce_kernel(const PsBatch batch) {
  const PsProduct& d = batch.e[owner_of(batch, (long long)blockIdx.x)];
  const int rows = d.swap ? d.Nc : d.M, cols = d.swap ? d.M : d.Nc;            // of C
  const long long idx = (blockIdx.x - d.base) * PS_THREADS + threadIdx.x;
  if (idx >= (long long)rows * cols) return;
  const int i = (int)(idx / cols), j = (int)(idx - (long long)i * cols);
  const int ik = d.swap ? j : i, jk = d.swap ? i : j;                           // in the tile the kernel computed
  const int ta = d.half ? PS_TM / 2 : PS_TM;
  const int tm = ik / ta, tn = jk / PS_TM;
  const long long tile = (long long)tm * d.tiles_n + tn, slab = (long long)ta * PS_TM;
  const float* s = d.slabs + tile * d.slices * slab + (ik - tm * ta) * PS_TM + (jk - tn * PS_TM);
  float v = 0.f;
#pragma unroll 8
  for (int sl = 0; sl < d.slices; ++sl) v += s[sl * slab];                      // loads independent, adds in slice order
  v *= d.alpha;
  float* out = d.C + (long long)i * d.c_rs + j;
  *out = d.first ? v : *out + v;
}

// ------------------------------------------------------------------------------------------------ pack
// curv_persample_pack_ex (and curv_persample_pack, its fp32-contiguous spelling): X_n or g_n as K-contiguous fp32 rows,
// from a source of fp32, bf16 or fp16 values addressed through element strides; forward im2col (with a dilation: the
// `reserved` word of the descriptor) or the transposed gather of a ConvTranspose2d input; curv_persample_pack3d: the 3-D
// im2col of a Conv3d input, the same record with a depth window (a 2-D item is D = kd = sd = 1, pd = 0).
struct PsPack {
  const void* src;
  float* dst;
  long long s_n;                // sample stride in elements: the sample base is formed in 64 bits, once per thread
  unsigned s_c, s_h, s_w;       // strides inside a sample, in elements (a sample spans fewer than 2^31: pack_plan_of)
  int N, C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo;
  int dh, dw;                   // dilation of the forward im2col (1, 1 for a transposed item)
  int rows;                     // C kd kh kw (the ones row, if any, is row `rows`)
  int R;                        // rows + has_bias
  int L, Lp;
  int has_bias, transposed, rows_outer;
  int vec;                      // rows are plain runs of the source, every group of four aligned: one vector load each
  long long base;               // first thread of this item in the launch
  // the depth window, read by the DEPTH instantiations of the kernel only (behind everything else: the offsets of the
  // fields the 2-D instantiations read are what they were)
  unsigned s_d;
  int D, kd, sd, pd, Do;
  int depth;                    // the item has one: D, kd or pd differ from (1, 1, 0); it is launched with its like
};

typedef ArgBatch<PsPack, PS_BATCH> PsPackBatch;
static_assert(sizeof(PsBatch) <= 3840 && sizeof(PsQuadBatch) <= 3840 && sizeof(PsPackBatch) <= 3840 &&
                  sizeof(PsCovBatch) <= 3840 && sizeof(PsGridBatch) <= 3840 && sizeof(PsProjectBatch) <= 3840,
              "kernel argument block must stay below 4 KB");

int pack_elem_bytes(int dtype) {
  return dtype == CURV_DTYPE_F32 ? 4 : (dtype == CURV_DTYPE_BF16 || dtype == CURV_DTYPE_F16) ? 2 : 0;
}

// What the planner reads: the general 2-D descriptor with a depth window beside it.  The 2-D entry points hand over
// D = kd = sd = 1, pd = 0, s_d = 0; `volume`: the item came through curv_persample_pack3d (its messages name the depth).
struct PackItem : curv_persample_pack_ex_desc {
  long long s_d;
  int D, kd, sd, pd;
  int volume;
};

PackItem pack_item_of(const curv_persample_pack_ex_desc& d) {
  PackItem it;
  static_cast<curv_persample_pack_ex_desc&>(it) = d;
  it.s_d = 0; it.D = it.kd = it.sd = 1; it.pd = 0; it.volume = 0;
  return it;
}

// What is wrong with the geometry of a 3-D item, nullptr if nothing: side::conv_geom_fault with a depth axis.  *Do:
// the output depth.
const char* volume_geom_fault(const PackItem& d, side::ConvGeom* g, int* Do) {
  if (d.D < 1 || d.kd < 1 || d.sd < 1 || d.pd < 0) return "invalid geometry";
  if (const char* fault = side::source_geom_fault(d, g)) return fault;
  // (N C H W is below 2^40 by now; times D by a division: the product may not fit)
  if ((long long)d.N * d.C * d.H * d.W >= ((1LL << 40) + d.D - 1) / d.D) return "too large (2^40 source elements or more)";
  if ((long long)d.D + 2LL * d.pd < d.kd || (long long)d.H + 2LL * d.ph < d.kh || (long long)d.W + 2LL * d.pw < d.kw)
    return "kernel larger than the padded input";
  *Do = (int)(((long long)d.D + 2LL * d.pd - d.kd) / d.sd + 1);
  g->Ho = (int)(((long long)d.H + 2LL * d.ph - d.kh) / d.sh + 1);
  g->Wo = (int)(((long long)d.W + 2LL * d.pw - d.kw) / d.sw + 1);
  return nullptr;
}

// Item `index` of a call of `who` as the kernel reads it, or false with the error text set.  One order of checks for
// every entry point, that of curv_persample_pack: sizes first, addresses after them, so that a call with null pointers
// learns whether its geometry would be taken.  `pointers`: the one message a caller has for a null src or dst and a
// misaligned dst (curv_persample_pack), in place of one message each.
bool pack_plan_of(const PackItem& d, int index, const char* who, PsPack* out, const char* pointers = nullptr) {
  const int esize = pack_elem_bytes(d.dtype);
  if (esize == 0) {
    set_error("%s: item %d: unknown dtype %d (CURV_DTYPE_F32, CURV_DTYPE_BF16 or CURV_DTYPE_F16)", who, index, d.dtype);
    return false;
  }
  side::ConvGeom g;
  int Do = 1;
  // the dilation rides in `reserved` (a half of 0 is 1): 0, what callers wrote before there was one, is dilation 1
  const int dh = std::max(d.reserved & 0xffff, 1), dw = std::max((d.reserved >> 16) & 0xffff, 1);
  if (d.volume) {                                       // (no dilation and no transposed form: pack_item_of)
    if (d.reserved != 0) {
      set_error("%s: item %d: reserved is %d, must be 0", who, index, d.reserved);
      return false;
    }
    if (const char* fault = volume_geom_fault(d, &g, &Do)) {
      set_error("%s: item %d: %s (N %d C %d D %d H %d W %d kernel %dx%dx%d stride %dx%dx%d padding %dx%dx%d)", who, index,
                fault, d.N, d.C, d.D, d.H, d.W, d.kd, d.kh, d.kw, d.sd, d.sh, d.sw, d.pd, d.ph, d.pw);
      return false;
    }
  } else if (d.transposed) {
    if (dh != 1 || dw != 1) {
      set_error("%s: item %d: dilation %dx%d with the transposed gather", who, index, dh, dw);
      return false;
    }
    if (!side::source_geom_of(d, who, "item", index, &g)) return false;
    // the sizes `output_size` allows: output_padding in [0, stride)
    const long long lo_h = (long long)(d.H - 1) * d.sh - 2LL * d.ph + d.kh, lo_w = (long long)(d.W - 1) * d.sw - 2LL * d.pw + d.kw;
    if (d.Ho < 1 || d.Wo < 1 || d.Ho < lo_h || d.Ho > lo_h + d.sh - 1 || d.Wo < lo_w || d.Wo > lo_w + d.sw - 1) {
      set_error("%s: item %d: transposed output %dx%d outside [%lld, %lld] x [%lld, %lld] (H %d W %d kernel %dx%d stride "
                "%dx%d padding %dx%d)", who, index, d.Ho, d.Wo, lo_h, lo_h + d.sh - 1, lo_w, lo_w + d.sw - 1, d.H, d.W,
                d.kh, d.kw, d.sh, d.sw, d.ph, d.pw);
      return false;
    }
    g.Ho = d.Ho; g.Wo = d.Wo;
  } else if (dh == 1 && dw == 1) {
    if (!side::conv_geom_of(d, who, "item", index, &g)) return false;
  } else {
    // the output of the dilated window: the geometry check of a kernel of (k - 1) d + 1 taps a side
    curv_persample_pack_ex_desc e = d;
    const long long eh = (long long)(d.kh - 1) * dh + 1, ew = (long long)(d.kw - 1) * dw + 1;
    const bool taps = d.kh >= 1 && d.kw >= 1 && eh < (1LL << 31) && ew < (1LL << 31);
    e.kh = taps ? (int)eh : 0; e.kw = taps ? (int)ew : 0;
    if (const char* fault = side::conv_geom_fault(e, &g)) {
      set_error("%s: item %d: %s (N %d C %d H %d W %d kernel %dx%d dilation %dx%d stride %dx%d padding %dx%d)", who, index,
                fault, d.N, d.C, d.H, d.W, d.kh, d.kw, dh, dw, d.sh, d.sw, d.ph, d.pw);
      return false;
    }
    g.kh = d.kh; g.kw = d.kw;
  }
  if (d.s_n < 0 || d.s_c < 0 || d.s_d < 0 || d.s_h < 0 || d.s_w < 0 || d.src_elems < 1) {
    set_error("%s: item %d: negative stride, or source extent %lld elements below 1", who, index, d.src_elems);
    return false;
  }
  PsPack P;
  P.src = d.src; P.dst = d.dst;
  P.N = g.N; P.C = g.C; P.H = g.H; P.W = g.W;
  P.kh = g.kh; P.kw = g.kw; P.sh = g.sh; P.sw = g.sw; P.ph = g.ph; P.pw = g.pw; P.Ho = g.Ho; P.Wo = g.Wo;
  P.dh = dh; P.dw = dw;
  P.D = d.D; P.kd = d.kd; P.sd = d.sd; P.pd = d.pd; P.Do = Do;
  P.depth = d.D != 1 || d.kd != 1 || d.pd != 0;
  // (the depth factors of a 3-D item enter only while the 2-D products are within their limit: nothing overflows)
  long long rows = (long long)d.C * d.kh * d.kw, L = (long long)P.Ho * P.Wo;
  if (rows <= (1 << 24)) rows *= d.kd;
  if (L <= (1 << 24)) L *= Do;
  // what one sample spans, (C-1) s_c + (D-1) s_d + (H-1) s_h + (W-1) s_w, stays below 2^31 elements: offsets inside a
  // sample are 32-bit (a stride of 2^31 or more is refused before it is multiplied)
  const long long dims[5] = {d.N, d.C, d.D, d.H, d.W}, strides[5] = {d.s_n, d.s_c, d.s_d, d.s_h, d.s_w};
  const long long span_max = 1LL << 31;
  long long span = 0;
  for (int k = 1; k < 5 && span < span_max; ++k)
    span = dims[k] > 1 && strides[k] >= span_max ? span_max : span + (dims[k] - 1) * strides[k];
  if (rows > (1 << 24) || L > (1 << 24) || span >= span_max || (long long)d.N * (rows + 1) * (d.Lp / 4 + 1) >= (1LL << 31)) {
    set_error("%s: item %d: too large (%lld rows, %lld positions)", who, index, rows, L);
    return false;
  }
  if (d.Lp < L || (d.Lp & 3)) {
    set_error("%s: item %d: Lp %d must be a multiple of 4 and at least L = %lld", who, index, d.Lp, L);
    return false;
  }
  // the largest addressed offset, span + (N-1) s_n, lies inside the extent (by a division: the product may not fit).  The
  // 3-D form counts the extent among the sizes and checks it before the addresses; the 2-D forms keep their order
  const bool short_extent = span >= d.src_elems || (d.N > 1 && d.s_n > (d.src_elems - 1 - span) / (d.N - 1));
  if (short_extent && d.volume) {
    set_error("%s: item %d: the source extent (%lld elements) is smaller than the largest offset its sizes and strides "
              "address (N %d C %d D %d H %d W %d, strides %lld %lld %lld %lld %lld)", who, index, d.src_elems, d.N, d.C,
              d.D, d.H, d.W, d.s_n, d.s_c, d.s_d, d.s_h, d.s_w);
    return false;
  }
  if (pointers && (!d.src || !d.dst || (reinterpret_cast<uintptr_t>(d.dst) & 15))) {
    set_error("%s: item %d: %s", who, index, pointers);
    return false;
  }
  if (!d.src || !d.dst) {
    set_error("%s: item %d: null src or dst", who, index);
    return false;
  }
  if (reinterpret_cast<uintptr_t>(d.dst) & 15) {
    set_error("%s: item %d: dst is not 16-byte aligned", who, index);
    return false;
  }
  if (reinterpret_cast<uintptr_t>(d.src) % (uintptr_t)esize) {
    set_error("%s: item %d: src is not aligned to its %d-byte elements", who, index, esize);
    return false;
  }
  if (short_extent) {
    set_error("%s: item %d: the source extent (%lld elements) is smaller than the largest offset its sizes and strides "
              "address (N %d C %d H %d W %d, strides %lld %lld %lld %lld)", who, index, d.src_elems, d.N, d.C, d.H, d.W,
              d.s_n, d.s_c, d.s_h, d.s_w);
    return false;
  }
  P.s_n = d.N > 1 ? d.s_n : 0; P.s_c = (unsigned)(d.C > 1 ? d.s_c : 0);
  P.s_h = (unsigned)(d.H > 1 ? d.s_h : 0); P.s_w = (unsigned)(d.W > 1 ? d.s_w : 0);
  P.s_d = (unsigned)(d.D > 1 ? d.s_d : 0);
  P.rows = (int)rows;
  P.has_bias = d.has_bias ? 1 : 0;
  P.R = P.rows + P.has_bias;
  P.L = (int)L;
  P.Lp = d.Lp;
  P.transposed = d.transposed ? 1 : 0;
  P.rows_outer = d.rows_outer ? 1 : 0;
  // the vector path: a row is the run of D H W source values behind (n, c), and every group of four of it starts on a
  // 4-element boundary - decided here, per item, from the pointer and the strides, so that the kernel's branch is uniform
  const bool plain = !P.transposed && d.kh == 1 && d.kw == 1 && d.sh == 1 && d.sw == 1 && d.ph == 0 && d.pw == 0 &&
                     d.kd == 1 && d.sd == 1 && d.pd == 0;
  const bool run = (d.W == 1 || d.s_w == 1) && (d.H == 1 || d.s_h == d.W) && (d.D == 1 || d.s_d == (long long)d.H * d.W);
  const bool aligned = (reinterpret_cast<uintptr_t>(d.src) % (4 * (uintptr_t)esize)) == 0 && (d.N == 1 || d.s_n % 4 == 0) &&
                       (d.C == 1 || d.s_c % 4 == 0);
  P.vec = plain && run && aligned;
  P.base = 0;
  *out = P;
  return true;
}

// The source types: a bf16 value is its bit pattern (the upper half of the fp32 one), fp16 converts exactly.
struct ps_bf16 { unsigned short bits; };
__device__ __forceinline__ float ps_up(float x) { return x; }
__device__ __forceinline__ float ps_up(ps_bf16 x) { return __uint_as_float((unsigned)x.bits << 16); }
__device__ __forceinline__ float ps_up(_Float16 x) { return (float)x; }
template <typename T>
struct alignas(4 * sizeof(T)) PsQuad4 { T v[4]; };

// Pack: one thread per 4 consecutive columns of one row of one sample (one 16-byte store); padding columns are written
// as zeros, a masked or padded element reads element 0 of the source and drops it.  32-bit index arithmetic after the
// sample base (an item has fewer than 2^31 threads and a sample spans fewer than 2^31 elements: pack_plan_of): the
// 64-bit divisions cost more than the copy.  TRANSPOSED: the launch may hold items of the transposed gather (its two
// divisions per element stay out of the code of a launch that holds none: the forward unfolds of a ResNet).  DEPTH:
// the items of the launch have a depth window (curv_persample_pack3d): l = (od, oh, ow) is decoded with two divisions and
// the four elements walk with carries through ow and oh (with Wo = 1 or Ho Wo < 4 one thread crosses several depths); the
// tap is (c, ad, a, b).  Items with a depth window are launched apart from the others (launch_pack), never transposed, so
// a launch without one runs the code it ran before there was a depth.
template <typename T, bool TRANSPOSED, bool DEPTH>
__global__ void __launch_bounds__(PS_THREADS) ps_pack_kernel(const PsPackBatch batch) {
  const long long t = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
  const PsPack& F = batch.e[owner_of(batch, t)];
  const unsigned gpr = F.Lp / 4, R = F.R;
  if (t - F.base >= (long long)F.N * R * gpr) return;
  const unsigned local = (unsigned)(t - F.base);
  const unsigned row = local / gpr;                        // n R + r
  const int k0 = (int)(local - row * gpr) * 4;
  const unsigned n = row / R;
  const int r = (int)(row - n * R);
  const T* first = reinterpret_cast<const T*>(F.src);
  const T* sample = first + (long long)n * F.s_n;
  float v[4];
  if (r >= F.rows) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k0 + e < F.L ? 1.0f : 0.0f;      // the ones row of a biased layer
  } else if (F.vec && k0 + 4 <= F.L) {                                    // (1 x 1: r is the channel)
    const PsQuad4<T> q = *reinterpret_cast<const PsQuad4<T>*>(sample + ((unsigned)r * F.s_c + (unsigned)k0));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ps_up(q.v[e]);
  } else {
    // every field the four elements read is held in a register first: a field read inside the loop is a load from the
    // argument block with a wait of its own, and the four gathers would no longer be in flight together
    const unsigned khw = F.kh * F.kw, kw = F.kw, H = F.H, W = F.W, s_h = F.s_h, s_w = F.s_w;
    const int L = F.L, Wo = F.Wo, sh = F.sh, sw = F.sw, ph = F.ph, pw = F.pw;
    const bool transposed = TRANSPOSED && F.transposed;
    const unsigned taps = DEPTH ? (unsigned)F.kd * khw : khw;            // of one channel
    const int c = (int)((unsigned)r / taps);
    int q = r - c * (int)taps, ad = 0;
    if (DEPTH) { ad = (int)((unsigned)q / khw); q -= ad * (int)khw; }
    const int a = (int)((unsigned)q / kw), b = q - a * (int)kw;
    const int ta = a * F.dh, tb = b * F.dw;                               // the tap's offset in the forward window
    const unsigned D = F.D, s_d = F.s_d;
    const int Ho = F.Ho, sd = F.sd, td = ad - F.pd;
    int od = 0, rest = k0;
    if (DEPTH) { od = (int)((unsigned)k0 / (unsigned)(Ho * Wo)); rest = k0 - od * Ho * Wo; }
    int oh = (int)((unsigned)rest / (unsigned)Wo), ow = rest - oh * Wo;
    const T* plane = sample + (unsigned)c * F.s_c;
    const T* at[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool ok = k0 + e < L;
      unsigned ih, iw;
      if (transposed) {
        // x[n, c, (oh + ph - a) / sh, (ow + pw - b) / sw] where both are whole and inside; no division of a negative
        const int th = oh + ph - a, tw = ow + pw - b;
        ok = ok & (th >= 0) & (tw >= 0);
        const unsigned uh = ok ? (unsigned)th : 0u, uw = ok ? (unsigned)tw : 0u;
        ih = uh / (unsigned)sh;
        iw = uw / (unsigned)sw;
        ok = ok & (ih * (unsigned)sh == uh) & (iw * (unsigned)sw == uw);
      } else {
        ih = (unsigned)(oh * sh - ph + ta);
        iw = (unsigned)(ow * sw - pw + tb);
      }
      ok = ok & (ih < H) & (iw < W);
      if constexpr (DEPTH) {
        const unsigned id = (unsigned)(od * sd + td);
        ok = ok & (id < D);
        at[e] = ok ? plane + (id * s_d + ih * s_h + iw * s_w) : nullptr;
        if (++ow == Wo) {
          ow = 0;
          if (++oh == Ho) { oh = 0; ++od; }
        }
      } else {
        at[e] = ok ? plane + (ih * s_h + iw * s_w) : nullptr;
        if (++ow == Wo) { ow = 0; ++oh; }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = ps_up(*(at[e] ? at[e] : first));                    // a masked gather reads element 0 and drops it
      v[e] = at[e] ? x : 0.0f;
    }
  }
  const long long out = F.rows_outer ? ((long long)r * F.N + n) * F.Lp + k0 : (long long)row * F.Lp + k0;
  *reinterpret_cast<float4*>(F.dst + out) = make_float4(v[0], v[1], v[2], v[3]);
}

// `packs`: the items of one source type that have a depth window (`depth`), or those that have none.
template <typename T>
int launch_pack(hipStream_t stream, const std::vector<PsPack>& packs, bool depth, const char* who) {
  return for_arg_batches<PsPack, PS_BATCH, 1>(
      (int)packs.size(), who,
      [&](int i, PsPack* P, long long* threads) {
        *P = packs[i];
        threads[0] = (long long)P->N * P->R * (P->Lp / 4);
      },
      [](int, long long threads) { return cdivll(threads, PS_THREADS); },
      [&](const PsPackBatch* b, const long long*, const unsigned* grid) {
        const bool transposed = std::any_of(b[0].e, b[0].e + b[0].count, [](const PsPack& P) { return P.transposed != 0; });
        void (*kernel)(PsPackBatch) = ps_pack_kernel<T, false, false>;
        if (transposed) kernel = ps_pack_kernel<T, true, false>;
        if (depth) kernel = ps_pack_kernel<T, false, true>;               // (an item with a depth is never transposed)
        hipLaunchKernelGGL(kernel, dim3(grid[0]), dim3(PS_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

// Every item is planned before anything is launched; the items of one source type share their launches, in call order -
// those with a depth window apart from those without, which so run the instantiations they always ran.
int pack_items(hipStream_t stream, const std::vector<PackItem>& items, const char* who, const char* pointers = nullptr) {
  std::vector<PsPack> packs[2][3];
  for (size_t i = 0; i < items.size(); ++i) {
    PsPack P;
    if (!pack_plan_of(items[i], (int)i, who, &P, pointers)) return CURV_ERR_INVALID;
    packs[P.depth][items[i].dtype].push_back(P);
  }
  int rc = CURV_OK;
  for (int depth = 0; depth < 2 && rc == CURV_OK; ++depth) {
    rc = launch_pack<float>(stream, packs[depth][CURV_DTYPE_F32], depth != 0, who);
    if (rc == CURV_OK) rc = launch_pack<ps_bf16>(stream, packs[depth][CURV_DTYPE_BF16], depth != 0, who);
    if (rc == CURV_OK) rc = launch_pack<_Float16>(stream, packs[depth][CURV_DTYPE_F16], depth != 0, who);
  }
  return rc;
}

size_t bytes_of(const std::vector<Plan>& plans) {
  size_t total = 0;
  for (const Plan& p : plans) total += p.slab_bytes;
  return total;
}

// A Product (PsProduct / PsQuad) with the operands of `d` as the kernels see them; its own fields are the caller's.  The
// one place where A and B change places.  (curv_persample_grid_desc has no alpha: its scale is gain[h].)
inline float alpha_of(const curv_persample_grid_desc&) { return 1.0f; }
template <typename Desc>
float alpha_of(const Desc& d) { return d.alpha; }

template <typename Product, typename Desc>
Product operands_of(const Desc& d, const Plan& p) {
  Product P;
  P.A = d.A; P.B = d.B;
  P.a_ns = d.a_ns; P.a_rs = d.a_rs; P.b_ns = d.b_ns; P.b_rs = d.b_rs;
  P.S = d.S; P.M = d.M; P.Nc = d.Nc; P.L = d.L;
  P.a_bytes = (unsigned)p.a_bytes; P.b_bytes = (unsigned)p.b_bytes;
  if (p.swap) {
    std::swap(P.A, P.B); std::swap(P.a_ns, P.b_ns); std::swap(P.a_rs, P.b_rs); std::swap(P.M, P.Nc);
    std::swap(P.a_bytes, P.b_bytes);
  }
  P.tiles_n = p.tiles_n; P.tiles = p.tiles; P.spi = p.spi; P.slices = p.slices;
  P.half = p.half; P.swap = p.swap;
  P.first = d.first ? 1 : 0; P.alpha = alpha_of(d);
  P.base = 0;
  return P;
}

// The product of `d`, its slabs at `slabs`.
PsProduct product_of(const curv_persample_desc& d, const Plan& p, float* slabs) {
  PsProduct P = operands_of<PsProduct>(d, p);
  P.C = d.C; P.slabs = slabs; P.c_rs = d.c_rs;
  return P;
}

// The same for curv_persample_quad_reduce, its partials at `partial`.
PsQuad quad_of(const curv_persample_quad_desc& d, const Plan& p, float* partial) {
  PsQuad P = operands_of<PsQuad>(d, p);
  P.W = d.W; P.out = d.out; P.partial = partial; P.o_stride = d.o_stride;
  P.w_is = d.w_rs; P.w_js = 1;
  if (p.swap) std::swap(P.w_is, P.w_js);
  return P;
}

// The same for curv_persample_cov_reduce.
PsCov cov_of(const curv_persample_cov_desc& d, const Plan& p, float* partial) {
  PsCov P = operands_of<PsCov>(d, p);
  P.W = d.W; P.out = d.out; P.partial = partial;
  P.a_cs = d.a_cs; P.w_rs = d.w_rs; P.o_ns = d.o_ns; P.o_rs = d.o_rs;
  P.K = d.K; P.pairs = d.K * (d.K + 1) / 2;
  return P;
}

// The same for curv_persample_project (no swap: project_plan_of).
PsProject project_of(const curv_persample_project_desc& d, const Plan& p, float* partial) {
  PsProject P = operands_of<PsProject>(d, p);
  P.W = d.W; P.U = d.U; P.Z = d.Z; P.partial = partial;
  P.w_is = d.w_rs; P.w_js = 1; P.u_rs = d.M > 1 ? d.u_rs : d.R;      // (the stride of a single row says nothing)
  P.z_ns = d.z_ns; P.z_rs = d.z_rs; P.z_cs = d.z_cs;
  P.R = d.R; P.parts = p.parts;
  return P;
}

// The same for curv_persample_quad_grid_reduce: the grid's tables by value; u and v (the rows and columns of the product)
// and the strides of V change places with the operands.
PsGrid grid_of(const curv_persample_grid_desc& d, const Plan& p, float* partial) {
  PsGrid P = operands_of<PsGrid>(d, p);
  P.u = d.u; P.v = d.v; P.V = d.V; P.out = d.out; P.partial = partial;
  P.o_stride = d.o_stride; P.o_hs = d.o_hs; P.H = d.H;
  P.v_is = d.v_rs; P.v_js = 1;
  if (p.swap) { std::swap(P.u, P.v); std::swap(P.v_is, P.v_js); }
  for (int h = 0; h < GRID_MAX; ++h) {
    P.shift[h] = d.shift[std::min(h, d.H - 1)];
    P.gain[h] = d.gain[std::min(h, d.H - 1)];
  }
  return P;
}

// The body of the accumulate entry points: plans, check(name, desc, index) of every descriptor's operands, workspace,
// then one walk and two launches per batch - lane 0 counts the items of the product launch, lane 1 the blocks of the
// reduce launch, reduce_units(desc) of them per product.  make = product_of / quad_of / cov_of / grid_of; BATCH products
// per launch (the kernels' argument type says how many).
template <typename Product, int BATCH, typename Desc, typename Check, typename Units>
int run_products(const char* name, void* stream_, const Desc* descs, int n, void* workspace, size_t workspace_bytes,
                 bool (*plan)(const Desc&, int, Plan*), Check check, Product (*make)(const Desc&, const Plan&, float*),
                 Units reduce_units, void (*product_kernel)(ArgBatch<Product, BATCH>),
                 void (*reduce_kernel)(ArgBatch<Product, BATCH>)) {
  if (n <= 0) return CURV_OK;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<Plan> plans;
  if (!side::plans_of(name, descs, n, plan, &plans)) return CURV_ERR_INVALID;
  for (int i = 0; i < n; ++i) {
    const int rc = check(name, descs[i], i);
    if (rc != CURV_OK) return rc;
  }
  const int rc = side::require_workspace(name, workspace, workspace_bytes, bytes_of(plans), 256);
  if (rc != CURV_OK) return rc;
  size_t at = 0;
  return for_arg_batches<Product, BATCH, 2>(
      n, name,
      [&](int i, Product* P, long long* units) {
        *P = make(descs[i], plans[i], (float*)((char*)workspace + at));
        at += plans[i].slab_bytes;
        units[0] = (long long)plans[i].tiles * plans[i].slices;
        units[1] = reduce_units(descs[i]);
      },
      [](int, long long units) { return units; },
      [&](const ArgBatch<Product, BATCH>* b, const long long*, const unsigned* grid) {
        hipLaunchKernelGGL(product_kernel, dim3(grid[0]), dim3(PS_THREADS), 0, stream, b[0]);
        CURV_LAUNCH_CHECK();
        hipLaunchKernelGGL(reduce_kernel, dim3(grid[1]), dim3(PS_THREADS), 0, stream, b[1]);
        CURV_LAUNCH_CHECK();
        return CURV_OK;
      });
}

}  // namespace
}  // namespace curv

using namespace curv;

extern "C" size_t curv_persample_workspace_bytes(const curv_persample_desc* descs, int n) {
  return side::workspace_bytes("curv_persample_workspace_bytes", descs, n, plan_of, bytes_of);
}

extern "C" int curv_persample_plan_flops(const curv_persample_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_persample_plan_flops", descs, n, out, plan_of);
}

extern "C" int curv_persample_sq_accumulate(void* stream_, const curv_persample_desc* descs, int n, void* workspace,
                                            size_t workspace_bytes) {
  return run_products(
      "curv_persample_sq_accumulate", stream_, descs, n, workspace, workspace_bytes, plan_of,
      [](const char* name, const curv_persample_desc& d, int i) -> int {
        CURV_REQUIRE(d.A && d.B && d.C, "%s: item %d: null operand", name, i);
        return CURV_OK;
      },
      product_of, [](const curv_persample_desc& d) { return cdivll((long long)d.M * d.Nc, PS_THREADS); },
      ps_product_kernel, ps_reduce_kernel);
}

extern "C" size_t curv_persample_quad_workspace_bytes(const curv_persample_quad_desc* descs, int n) {
  return side::workspace_bytes("curv_persample_quad_workspace_bytes", descs, n, quad_plan_of, bytes_of);
}

extern "C" int curv_persample_quad_plan_flops(const curv_persample_quad_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_persample_quad_plan_flops", descs, n, out, quad_plan_of);
}

extern "C" int curv_persample_quad_reduce(void* stream_, const curv_persample_quad_desc* descs, int n, void* workspace,
                                          size_t workspace_bytes) {
  return run_products(
      "curv_persample_quad_reduce", stream_, descs, n, workspace, workspace_bytes, quad_plan_of,
      [](const char* name, const curv_persample_quad_desc& d, int i) -> int {
        CURV_REQUIRE(d.A && d.B && d.out, "%s: item %d: null operand", name, i);
        CURV_REQUIRE(((reinterpret_cast<uintptr_t>(d.A) | reinterpret_cast<uintptr_t>(d.B)) & 15) == 0,
                     "%s: item %d: A and B must be 16-byte aligned", name, i);
        return CURV_OK;
      },
      quad_of, [](const curv_persample_quad_desc& d) { return cdivll(d.S, PS_THREADS); },
      ps_quad_product_kernel, ps_quad_reduce_kernel);
}

extern "C" size_t curv_persample_quad_grid_workspace_bytes(const curv_persample_grid_desc* descs, int n) {
  return side::workspace_bytes("curv_persample_quad_grid_workspace_bytes", descs, n, grid_plan_of, bytes_of);
}

extern "C" int curv_persample_quad_grid_plan_flops(const curv_persample_grid_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_persample_quad_grid_plan_flops", descs, n, out, grid_plan_of);
}

extern "C" int curv_persample_quad_grid_reduce(void* stream_, const curv_persample_grid_desc* descs, int n, void* workspace,
                                               size_t workspace_bytes) {
  return run_products(
      "curv_persample_quad_grid_reduce", stream_, descs, n, workspace, workspace_bytes, grid_plan_of,
      [](const char* name, const curv_persample_grid_desc& d, int i) -> int {
        CURV_REQUIRE(d.A && d.B && d.out, "%s: item %d: null operand", name, i);
        CURV_REQUIRE(((reinterpret_cast<uintptr_t>(d.A) | reinterpret_cast<uintptr_t>(d.B)) & 15) == 0,
                     "%s: item %d: A and B must be 16-byte aligned", name, i);
        CURV_REQUIRE(d.V ? (!d.u && !d.v) : (d.u && d.v),
                     "%s: item %d: the weights are either u and v (separable) or V (dense)", name, i);
        return CURV_OK;
      },
      grid_of, [](const curv_persample_grid_desc& d) { return cdivll((long long)d.S * d.H, PS_THREADS); },
      ps_grid_product_kernel, ps_grid_reduce_kernel);
}

extern "C" size_t curv_persample_cov_workspace_bytes(const curv_persample_cov_desc* descs, int n) {
  return side::workspace_bytes("curv_persample_cov_workspace_bytes", descs, n, cov_plan_of, bytes_of);
}

extern "C" int curv_persample_cov_plan_flops(const curv_persample_cov_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_persample_cov_plan_flops", descs, n, out, cov_plan_of);
}

extern "C" int curv_persample_cov_reduce(void* stream_, const curv_persample_cov_desc* descs, int n, void* workspace,
                                         size_t workspace_bytes) {
  return run_products(
      "curv_persample_cov_reduce", stream_, descs, n, workspace, workspace_bytes, cov_plan_of,
      [](const char* name, const curv_persample_cov_desc& d, int i) -> int {
        CURV_REQUIRE(d.A && d.B && d.out, "%s: item %d: null operand", name, i);
        CURV_REQUIRE(((reinterpret_cast<uintptr_t>(d.A) | reinterpret_cast<uintptr_t>(d.B)) & 15) == 0,
                     "%s: item %d: A and B must be 16-byte aligned", name, i);
        return CURV_OK;
      },
      cov_of, [](const curv_persample_cov_desc& d) { return cdivll((long long)d.S * (d.K * (d.K + 1) / 2), PS_THREADS); },
      ps_cov_product_kernel, ps_cov_reduce_kernel);
}

extern "C" size_t curv_persample_project_workspace_bytes(const curv_persample_project_desc* descs, int n) {
  return side::workspace_bytes("curv_persample_project_workspace_bytes", descs, n, project_plan_of, bytes_of);
}

extern "C" int curv_persample_project_plan_flops(const curv_persample_project_desc* descs, int n, long long* out) {
  return side::plan_flops("curv_persample_project_plan_flops", descs, n, out, project_plan_of);
}

extern "C" int curv_persample_project(void* stream_, const curv_persample_project_desc* descs, int n, void* workspace,
                                      size_t workspace_bytes) {
  return run_products(
      "curv_persample_project", stream_, descs, n, workspace, workspace_bytes, project_plan_of,
      [](const char* name, const curv_persample_project_desc& d, int i) -> int {
        CURV_REQUIRE(d.A && d.B && d.W && d.U && d.Z, "%s: item %d: null operand", name, i);
        CURV_REQUIRE(((reinterpret_cast<uintptr_t>(d.A) | reinterpret_cast<uintptr_t>(d.B)) & 15) == 0,
                     "%s: item %d: A and B must be 16-byte aligned", name, i);
        return CURV_OK;
      },
      project_of, [](const curv_persample_project_desc& d) { return cdivll((long long)d.S * d.Nc * d.R, PS_THREADS); },
      ps_project_product_kernel, ps_project_reduce_kernel);
}

// The fp32-contiguous spelling of curv_persample_pack_ex: (N, C, H, W), or (N, H, W, C) with channels_last.
extern "C" int curv_persample_pack(void* stream_, const curv_persample_pack_desc* descs, int n) {
  const char* const name = "curv_persample_pack";
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs != nullptr, "%s: null descriptors", name);
  // (sizes that a geometry check refuses may be anything: they count as 0 here, and a product saturates)
  auto times = [](long long a, int b) { return b <= 0 ? 0 : a > LLONG_MAX / b ? LLONG_MAX : a * b; };
  std::vector<PackItem> items(n);
  for (int i = 0; i < n; ++i) {
    const curv_persample_pack_desc& d = descs[i];
    PackItem& e = items[i];
    e = pack_item_of(curv_persample_pack_ex_desc{});
    e.src = d.src; e.dst = d.dst;
    e.N = d.N; e.C = d.C; e.H = d.H; e.W = d.W;
    e.kh = d.kh; e.kw = d.kw; e.sh = d.sh; e.sw = d.sw; e.ph = d.ph; e.pw = d.pw;
    e.has_bias = d.has_bias; e.rows_outer = d.rows_outer; e.Lp = d.Lp;
    e.dtype = CURV_DTYPE_F32;
    const long long hw = times(d.H, d.W), wc = times(d.W, d.C), chw = times(hw, d.C);
    if (d.channels_last) { e.s_n = chw; e.s_c = 1; e.s_h = wc; e.s_w = d.C; }
    else { e.s_n = chw; e.s_c = hw; e.s_h = d.W; e.s_w = 1; }
    e.src_elems = times(chw, d.N);
  }
  return pack_items((hipStream_t)stream_, items, name, "null src or dst, or dst not 16-byte aligned");
}

extern "C" int curv_persample_pack_ex(void* stream_, const curv_persample_pack_ex_desc* descs, int n) {
  const char* const name = "curv_persample_pack_ex";
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs != nullptr, "%s: null descriptors", name);
  std::vector<PackItem> items(n);
  for (int i = 0; i < n; ++i) items[i] = pack_item_of(descs[i]);
  return pack_items((hipStream_t)stream_, items, name);
}

// The 3-D im2col of a Conv3d input: the same planner and kernel with the depth window of the descriptor.
extern "C" int curv_persample_pack3d(void* stream_, const curv_persample_pack3d_desc* descs, int n) {
  const char* const name = "curv_persample_pack3d";
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs != nullptr, "%s: null descriptors", name);
  std::vector<PackItem> items(n);
  for (int i = 0; i < n; ++i) {
    const curv_persample_pack3d_desc& d = descs[i];
    PackItem& e = items[i];
    e = pack_item_of(curv_persample_pack_ex_desc{});
    e.src = d.src; e.dst = d.dst;
    e.s_n = d.s_n; e.s_c = d.s_c; e.s_d = d.s_d; e.s_h = d.s_h; e.s_w = d.s_w; e.src_elems = d.src_elems;
    e.N = d.N; e.C = d.C; e.D = d.D; e.H = d.H; e.W = d.W;
    e.kd = d.kd; e.kh = d.kh; e.kw = d.kw; e.sd = d.sd; e.sh = d.sh; e.sw = d.sw; e.pd = d.pd; e.ph = d.ph; e.pw = d.pw;
    e.has_bias = d.has_bias; e.dtype = d.dtype; e.rows_outer = d.rows_outer; e.Lp = d.Lp; e.reserved = d.reserved;
    e.volume = 1;
  }
  return pack_items((hipStream_t)stream_, items, name);
}
