// What travels to the device as kernel arguments (copied by the runtime at launch time, so a call stays fully
// asynchronous and needs neither pinned staging memory nor a stream synchronisation): argument batches - tables of at
// most N entries that one launch works through, with their host walk and their device lookup - and the upload of a
// descriptor table into device memory, N rows per launch.
#pragma once
#include "common.h"

#include <algorithm>

namespace curv {

// ------------------------------------------------------------------------------------------------ argument batches
// At most N entries as one kernel argument.  `Entry::base` is the first unit (thread, item or workgroup: the kernel's
// choice) of the entry in the launch; the units of the entries of a batch follow one another.  Slots from `count` on
// repeat entry 0.
template <typename Entry, int N>
struct ArgBatch {
  Entry e[N];
  int count;
};

// The entry that owns unit `at`.
template <typename Batch, typename At>
__device__ inline int owner_of(const Batch& b, At at) {
  int f = 0;
  for (int i = 1; i < b.count; ++i)
    if (at >= b.e[i].base) f = i;
  return f;
}

// The same, stopping at the owner instead of reading every base.  The passes of the main factor build take this form:
// with owner_of their many short workgroups ran 1 - 4 % longer ("What travels as kernel arguments").
template <typename Batch, typename At>
__device__ inline int owner_of_early_exit(const Batch& b, At at) {
  int f = 0;
  while (f + 1 < b.count && b.e[f + 1].base <= at) ++f;
  return f;
}

// Walks `count` list entries in batches of N.  fill(k, &entry, units) writes entry k of the list and says how many
// units it has in each of the LANES launches that take the batch (one batch per lane, equal up to `base`);
// grid(lane, units) is the workgroup count of a lane's launch, refused from 2^31 on; launch(batches, units, grids)
// enqueues the launches of the batch and returns their status.
template <typename Entry, int N, int LANES, typename Fill, typename Grid, typename Launch>
int for_arg_batches(int count, const char* who, Fill fill, Grid grid, Launch launch) {
  for (int first = 0; first < count; first += N) {
    ArgBatch<Entry, N> b[LANES];
    long long units[LANES] = {};
    const int n = std::min(N, count - first);
    for (int k = 0; k < n; ++k) {
      Entry e;
      long long has[LANES];
      fill(first + k, &e, has);
      for (int l = 0; l < LANES; ++l) {
        e.base = (decltype(e.base))units[l];
        b[l].e[k] = e;
        units[l] += has[l];
      }
    }
    unsigned grids[LANES];
    for (int l = 0; l < LANES; ++l) {
      b[l].count = n;
      for (int k = n; k < N; ++k) b[l].e[k] = b[l].e[0];
      const long long blocks = grid(l, units[l]);
      CURV_REQUIRE(blocks < (1LL << 31), "%s: too many workgroups (%lld)", who, blocks);
      grids[l] = (unsigned)blocks;
    }
    const int rc = launch(b, units, grids);
    if (rc != CURV_OK) return rc;
  }
  return CURV_OK;
}

// ------------------------------------------------------------------------------------------------ table uploads
// N rows of a device table as one kernel argument ...
template <typename T, int N>
struct TableRows {
  T row[N];
};

constexpr int UPLOAD_PAD_FLOATS = 64;

// ... copied word by word to `table`; `zero_pad`, if given, gets UPLOAD_PAD_FLOATS zeros beside them.
template <typename T, int N>
__global__ void __launch_bounds__(256)
upload_rows_kernel(T* __restrict__ table, TableRows<T, N> rows, int count, float* __restrict__ zero_pad) {
  static_assert(sizeof(rows) <= 3840, "kernel argument block must stay below 4 KB");
  static_assert(sizeof(T) % 4 == 0, "rows are copied in 4-byte words");
  const int words = count * (int)(sizeof(T) / 4);
  const int* in = reinterpret_cast<const int*>(&rows);
  int* out = reinterpret_cast<int*>(table);
  for (int w = threadIdx.x; w < words; w += blockDim.x) out[w] = in[w];
  if (zero_pad != nullptr && threadIdx.x < UPLOAD_PAD_FLOATS) zero_pad[threadIdx.x] = 0.0f;
}

// table[0, n) = rows[0, n), N rows per launch.  The launch of the first block also zeroes `zero_pad` (may be null);
// a block [first, first + count) for which skip(first, count) holds is not launched at all.
template <int N, typename T, typename Skip>
int upload_table(hipStream_t stream, T* table, const T* rows, int n, float* zero_pad, Skip skip) {
  for (int first = 0; first < n; first += N) {
    const int count = std::min(N, n - first);
    if (skip(first, count)) continue;
    TableRows<T, N> block;
    memset(&block, 0, sizeof(block));
    memcpy(block.row, rows + first, (size_t)count * sizeof(T));
    hipLaunchKernelGGL((upload_rows_kernel<T, N>), dim3(1), dim3(256), 0, stream, table + first, block, count,
                       first == 0 ? zero_pad : (float*)nullptr);
    CURV_LAUNCH_CHECK();
  }
  return CURV_OK;
}

template <int N, typename T>
int upload_table(hipStream_t stream, T* table, const T* rows, int n) {
  return upload_table<N>(stream, table, rows, n, nullptr, [](int, int) { return false; });
}

}  // namespace curv
