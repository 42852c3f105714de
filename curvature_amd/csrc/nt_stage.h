// The stage engine of the fp32 NT tile products: the NT GEMM (gemm_nt.h) and the per-sample products (persample.hip).
//
// A stage is KC = 32 k values of two K-contiguous operand panels of up to 128 rows each.  It arrives by LDS-DMA
// (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction, as the flat factor build: syrk_flat.hip) in a double-buffered
// [128 rows][8 x 16 B] image per operand, the 16-byte slots XOR-swizzled by (row >> 1) & 7 on the SOURCE side, and comes
// back by conflict-free ds_read_b128 (one read = 4 k values of one row = the input of 4 MFMAs; lane half h takes k group
// 2 j + h of step j): no staging registers, no LDS store pass, 64 KiB of LDS, two workgroups per CU.  Every stage is
// straight-line code (round 6: step counts, the k tail and the DMA predicate as run-time conditions meant a scalar
// branch around every group of MFMAs and an exec-mask change around every piece).  Instead, a lane whose 16-byte group
// lies at or behind the end of its row - or any lane behind the item's last stage - carries an out-of-range voffset (the
// descriptor's range check drops the fetch; operand extents stay below 2^31 bytes), and the k values at or behind the
// end inside a range's last stage are zeroed in the operand registers, so what lies behind a row in memory never enters
// a product.
//
// The engine owns: the wave's DMA share (Dma: lane geometry, descriptors, the issue of one piece), the read-address
// table (read_addrs), the wait + barrier at a stage's head (stage_landed) and the stage itself (stage: reads, tail mask,
// read-ahead, MFMA groups with one piece of the next stage issued behind each).  A client brings: which rows its pieces
// fetch (voff_a, voff_b), the soffsets and the `live` predicate of the next stage, the accumulator shape NA x NB, and
// whatever happens between stages.
#pragma once
#include "common.h"

namespace curv {

typedef __attribute__((address_space(1))) float gfl;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(3))) char lds_char_t;

namespace nt {
constexpr int TM = 128, KC = 32, ROW_B = KC * 4, SLOTS = KC / 4, STEPS = KC / 8, RPP = 1024 / ROW_B;
constexpr int PIECES = TM / RPP / 4, PANEL_B = TM * ROW_B, LDS_B = 4 * PANEL_B;   // [buffer][A panel, B panel]
constexpr int KEY_SHIFT = 1, LANES_PER_ROW_SHIFT = 3;                              // see syrk_flat.hip
constexpr int WGS = 2;                                                             // workgroups per CU (64 KiB of LDS)

// The wave's share of the DMA of a stage: PA pieces of the A panel, then PIECES of the B panel.  Piece `slot` covers
// panel rows 32 slot + 8 wave + (lane >> 3) =: 32 slot + rsub; the lane fetches 16-byte group g_lane of its row.
template <int PA>
struct Dma {
  static constexpr int NP = PA + PIECES;
  static_assert(NP <= 4 * STEPS, "at most one DMA piece per MFMA group");
  __amdgpu_buffer_rsrc_t rsa, rsb;
  int voff_a[PA], voff_b[PIECES];            // the client's: byte offset of the lane's group in the row of each piece
  lds_char_t* lds;
  int wave, rsub, g_lane;

  __device__ __forceinline__ Dma(const float* A, unsigned a_bytes, const float* B, unsigned b_bytes, lds_char_t* lds_,
                                 int wave_, int lane)
      : rsa(__builtin_amdgcn_make_buffer_rsrc((void*)A, 0, a_bytes, 0x00020000)),
        rsb(__builtin_amdgcn_make_buffer_rsrc((void*)B, 0, b_bytes, 0x00020000)),
        lds(lds_), wave(wave_), rsub(RPP * wave_ + (lane >> LANES_PER_ROW_SHIFT)),
        g_lane((lane & (SLOTS - 1)) ^ ((rsub >> KEY_SHIFT) & (SLOTS - 1))) {}

  // voffset of piece p of a panel whose rows are rows r0 .. of an operand of `rows` rows, `pitch` floats apart: rows
  // beyond the operand are clamped to its last row (their results are never stored)
  __device__ __forceinline__ int row_voff(int r0, int p, int rows, long long pitch) const {
    return (int)(((long long)min(r0 + 4 * RPP * p + rsub, rows - 1) * pitch + 4 * g_lane) * 4);
  }
  // does the lane's group of a stage that starts at k lie inside a row of K values?
  __device__ __forceinline__ bool live(int k, int K) const { return k + 4 * g_lane < K; }

  __device__ __forceinline__ void issue(int i, bool live, unsigned soff_a, unsigned soff_b, unsigned nbuf) const {
    constexpr int OOB = (int)0x80000000;     // "no fetch"
    const bool b_side = i >= PA;
    const int slot = b_side ? i - PA : i;
    const unsigned lbase = (b_side ? 2u * PANEL_B : 0u) + nbuf + (unsigned)(RPP * wave + 4 * RPP * slot) * ROW_B;
    if (!b_side)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lds_void_t*)(lds + lbase), 16, live ? voff_a[slot] : OOB, soff_a, 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsb, (lds_void_t*)(lds + lbase), 16, live ? voff_b[slot] : OOB, soff_b, 0, 0);
  }
  // the first stage of an item, into buffer 0
  __device__ __forceinline__ void issue_first(bool live, unsigned soff_a, unsigned soff_b) const {
#pragma unroll
    for (int i = 0; i < NP; ++i) issue(i, live, soff_a, soff_b, 0u);
  }
};

// The STEPS swizzled LDS addresses (buffer 0) of panel row R of the A or the B panel for lane half h.
__device__ __forceinline__ void read_addrs(unsigned (&addr)[STEPS], int R, bool b_panel, int h) {
  const int rkey = (R >> KEY_SHIFT) & (SLOTS - 1);
#pragma unroll
  for (int j = 0; j < STEPS; ++j) addr[j] = (b_panel ? 2u * PANEL_B : 0u) + R * ROW_B + (((2 * j + h) ^ rkey) << 4);
}

// The head of stage t: this wave's DMA of it has landed (vmcnt(0)), then everybody's.  The barrier also says that every
// wave has finished stage t - 1, whose buffer the pieces issued during stage t overwrite.
__device__ __forceinline__ void stage_landed() {
  __builtin_amdgcn_s_waitcnt(0x0f70);
  __syncthreads();
}

// Stage t of an item, out of buffer t & 1: NA x NB blocks of v_mfma_f32_32x32x2_f32 per wave, c[m][n] += panel rows of
// addr_a[m] times those of addr_b[n].  k_left k values of the stage count (at least KC everywhere but in the last stage
// of a range that is no multiple of KC).  issue_next(i, next_buffer) issues piece i of stage t + 1, i < NP: one behind
// each of the first NP groups of MFMAs.
template <int NA, int NB, int NP, typename IssueNext>
__device__ __forceinline__ void stage(f32x16 (&c)[NA][NB], const unsigned (&addr_a)[NA][STEPS],
                                      const unsigned (&addr_b)[NB][STEPS], lds_char_t* lds, int t, int k_left, int h,
                                      IssueNext issue_next) {
  const unsigned buf = (unsigned)(t & 1) * PANEL_B, nbuf = PANEL_B - buf;
  auto rd = [&](unsigned at) { return *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(lds + at + buf); };
  f32x4 a[NA], b[NB];
#pragma unroll
  for (int m = 0; m < NA; ++m) a[m] = rd(addr_a[m][0]);
#pragma unroll
  for (int n = 0; n < NB; ++n) b[n] = rd(addr_b[n][0]);
#pragma unroll
  for (int j = 0; j < STEPS; ++j) {
    if (k_left < KC) {
      asm volatile("; k tail" ::: "memory");               // keeps this a branch around a VALU-only block
      const int mine = k_left - 4 * (2 * j + h);           // of the lane's four k values of this step
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool gone = e >= mine;
#pragma unroll
        for (int m = 0; m < NA; ++m) a[m][e] = gone ? 0.0f : a[m][e];
#pragma unroll
        for (int n = 0; n < NB; ++n) b[n][e] = gone ? 0.0f : b[n][e];
      }
    }
    f32x4 na[NA], nb[NB];
    if (j + 1 < STEPS) {
#pragma unroll
      for (int m = 0; m < NA; ++m) na[m] = rd(addr_a[m][j + 1]);
#pragma unroll
      for (int n = 0; n < NB; ++n) nb[n] = rd(addr_b[n][j + 1]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int m = 0; m < NA; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) c[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][e], b[n][e], c[m][n], 0, 0, 0);
      if (4 * j + e < NP) issue_next(4 * j + e, nbuf);
    }
    if (j + 1 < STEPS) {
#pragma unroll
      for (int m = 0; m < NA; ++m) a[m] = na[m];
#pragma unroll
      for (int n = 0; n < NB; ++n) b[n] = nb[n];
    }
  }
}
}  // namespace nt

}  // namespace curv
