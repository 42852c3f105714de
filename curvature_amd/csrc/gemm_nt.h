// The 128 x 128 NT tile product of the fp32 GEMMs (gemm.hip: samplers, EFB) on the stage engine (nt_stage.h).
#pragma once
#include "nt_stage.h"

namespace curv {

constexpr int GEMM_THREADS = 256;

struct GemmDev {
  const float* A;
  const float* B;
  float* C;
  const float* E;         // optional elementwise operand of the epilogue
  const float* F;         // optional second (additive) operand: CURV_EPI_MUL_E_ADD_F
  long long a_rs, a_cs;   // op(A) is M x K: element (i, k) at A[i*a_rs + k*a_cs]
  long long b_rs, b_cs;   // op(B) is K x N: element (k, j) at B[k*b_rs + j*b_cs]
  long long c_rs, c_cs;
  long long e_rs, e_cs;
  long long f_rs, f_cs;
  int M, N, K;
  int epilogue;
  float alpha, beta;
  int tiles_n, tile_base;
  int tm;                 // tile edge: 64 or 128
  int tri;                // CURV_TRI_*: triangular operand -> shorter K range per tile
  unsigned a_bytes, b_bytes;   // NT kernel: extents of the two operands (buffer range check)
  // NT kernel, split K: a tile's K range is cut into slices of kslice elements; item = tile * n_slices + slice, raw
  // partial tiles go to slabs and gemm_nt_reduce_kernel sums them in slice order and applies the epilogue
  int kslice, n_slices;        // n_slices <= 1: no split
  int red_base, pad2;          // first workgroup of this product in the reduce launch (-1: not split)
  long long slab_base;         // floats into the slab area
};

// ------------------------------------------------------------------------------------------------
// NT products with K-contiguous operands on both sides (A[i][k] at A + i a_rs + k, B[k][j] at B + j b_cs + k):
// every product of KFAC.sample_and_replace (L_G z^T, then (.) L_A^T) and of EFB.sample.  Staging and stages are the
// engine's (nt_stage.h); this file decodes the item, walks the stages of its K range and stores the tile.
// Rows beyond M / N are clamped to the last row (their results are never stored); k beyond K is zeroed in the last
// step; triangular operands cut the K range per tile (what lies beyond the cut inside the last step is stored zeros).
// ------------------------------------------------------------------------------------------------
// C[i][j] = epilogue(alpha * acc) [+ beta * C[i][j]]
__device__ __forceinline__ void nt_epilogue(const GemmDev& d, int i, int j, float acc) {
  gfl* C = (gfl*)d.C;
  const gfl* E = (const gfl*)d.E;
  const gfl* F = (const gfl*)d.F;
  const int ep = d.epilogue;
  const long long ci = i * d.c_rs + j * d.c_cs;
  float v = d.alpha * acc;
  if (ep == CURV_EPI_SQUARE) v = d.alpha * acc * acc;
  else if (ep == CURV_EPI_MUL_E) v *= E[i * d.e_rs + j * d.e_cs];
  else if (ep == CURV_EPI_ADD_E) v += E[i * d.e_rs + j * d.e_cs];
  else if (ep == CURV_EPI_MUL_E_ADD_F) v = v * E[i * d.e_rs + j * d.e_cs] + F[i * d.f_rs + j * d.f_cs];
  if (d.beta != 0.0f) v += d.beta * C[ci];
  C[ci] = v;
}

__device__ __forceinline__ void gemm_nt_tile(const GemmDev& d, int local, lds_char_t* lds, float* __restrict__ slabs) {
  using namespace nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const bool split = d.n_slices > 1;
  const int item = local;
  int slice = 0;
  if (split) { slice = local % d.n_slices; local /= d.n_slices; }
  int tm = local / d.tiles_n, tn = local - tm * d.tiles_n;
  if (d.tri == CURV_TRI_A_LOWER) tm = (d.M + TM - 1) / TM - 1 - tm;        // long tiles first
  else if (d.tri == CURV_TRI_B_UPPER) tn = d.tiles_n - 1 - tn;
  const int i0 = tm * TM, j0 = tn * TM, M = d.M, N = d.N;
  int K = d.K;
  if (d.tri == CURV_TRI_A_LOWER) K = min(K, i0 + TM);
  else if (d.tri == CURV_TRI_B_UPPER) K = min(K, j0 + TM);
  // this item's part of the K range: [kb, K) (K becomes the slice's end)
  int kb = 0;
  if (split) {
    kb = slice * d.kslice;
    if (kb >= K) return;                             // the triangle cut this slice away
    K = min(K, kb + d.kslice);
  }
  const int n_stages = (K - kb + KC - 1) / KC;
  // the last stage holds k values at or behind K when the range is no multiple of KC (never behind a triangular cut or
  // inside a split: those end on whole tiles / slices): what the DMA leaves there is zeroed in the operand registers

  Dma<PIECES> dma(d.A, d.a_bytes, d.B, d.b_bytes, lds, wave, lane);
#pragma unroll
  for (int p = 0; p < PIECES; ++p) {
    dma.voff_a[p] = dma.row_voff(i0, p, M, d.a_rs);
    dma.voff_b[p] = dma.row_voff(j0, p, N, d.b_cs);
  }
  unsigned addr_a[2][STEPS], addr_b[2][STEPS];
  f32x16 c[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    read_addrs(addr_a[m], 64 * wm + 32 * m + r32, false, h);
    read_addrs(addr_b[m], 64 * wn + 32 * m + r32, true, h);
    c[m][0] = 0.0f; c[m][1] = 0.0f;
  }
  if (n_stages > 0) dma.issue_first(dma.live(kb, K), kb * 4, kb * 4);
  for (int t = 0; t < n_stages; ++t) {
    stage_landed();
    const int k0 = kb + t * KC, k0n = k0 + KC;
    const bool live_n = t + 1 < n_stages && dma.live(k0n, K);
    stage<2, 2, Dma<PIECES>::NP>(c, addr_a, addr_b, lds, t, K - k0, h,
                        [&](int i, unsigned nbuf) { dma.issue(i, live_n, k0n * 4, k0n * 4, nbuf); });
  }

  // C/D map of the 32x32 block: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (split) {
    // raw partial tile, row-major 128 x 128, to this item's slab
    gfl* slab = (gfl*)slabs + d.slab_base + (long long)item * (TM * TM);
    auto store_raw = [&](const f32x16& acc, int m, int n) {
      const int c = 64 * wn + 32 * n + r32;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = 64 * wm + 32 * m + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        slab[r * TM + c] = acc[reg];
      }
    };
    store_raw(c[0][0], 0, 0);
    store_raw(c[0][1], 0, 1);
    store_raw(c[1][0], 1, 0);
    store_raw(c[1][1], 1, 1);
    return;
  }
  auto store_block = [&](const f32x16& acc, int m, int n) {
    const int j = j0 + 64 * wn + 32 * n + r32;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = i0 + 64 * wm + 32 * m + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (i < M && j < N) nt_epilogue(d, i, j, acc[reg]);
    }
  };
  store_block(c[0][0], 0, 0);
  store_block(c[0][1], 0, 1);
  store_block(c[1][0], 1, 0);
  store_block(c[1][1], 1, 1);
}

}  // namespace curv
