// What the side builds share (kfac_half.hip, group_factor.hip, convt_factor.hip, persample.hip): the check of a
// convolution geometry, argument batches (tables of at most N entries that travel as kernel arguments) with their host
// walk and their device lookup, and the bodies of the *_workspace_bytes / *_plan_flops / *_accumulate entry points.
// A build brings its own descriptor, `Plan`, `bool plan_of(const Desc&, int index, Plan*)` with its own limits, its
// kernels and its workspace layout.
#pragma once
#include "common.h"

#include <algorithm>
#include <vector>

namespace curv {
namespace side {

// ------------------------------------------------------------------------------------------------ geometry
struct ConvGeom {
  int N, C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo;
};

// The source side of `d` (any descriptor with the fields N C H W kh kw sh sw ph pw): sizes positive, padding not
// negative, fewer than 2^40 source elements.  Errors read "<prefix>: <unit> <index>: ...".  Ho / Wo are left to the caller.
template <typename Desc>
bool source_geom_of(const Desc& d, const char* prefix, const char* unit, int index, ConvGeom* g) {
  if (d.N < 1 || d.C < 1 || d.H < 1 || d.W < 1 || d.kh < 1 || d.kw < 1 || d.sh < 1 || d.sw < 1 || d.ph < 0 ||
      d.pw < 0) {
    set_error("%s: %s %d: invalid geometry (N %d C %d H %d W %d kernel %dx%d stride %dx%d padding %dx%d)", prefix, unit,
              index, d.N, d.C, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw);
    return false;
  }
  const long long elements = (long long)d.N * d.C * d.H * d.W;
  if (elements >= (1LL << 40)) {
    set_error("%s: %s %d: too large (%lld source elements, below %lld)", prefix, unit, index, elements, 1LL << 40);
    return false;
  }
  *g = ConvGeom{d.N, d.C, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, 0, 0};
  return true;
}

// ... and the output of a convolution over it: the kernel fits the padded input; Ho / Wo.
template <typename Desc>
bool conv_geom_of(const Desc& d, const char* prefix, const char* unit, int index, ConvGeom* g) {
  if (!source_geom_of(d, prefix, unit, index, g)) return false;
  if (d.H + 2 * d.ph < d.kh || d.W + 2 * d.pw < d.kw) {
    set_error("%s: %s %d: kernel %dx%d larger than the padded %dx%d input", prefix, unit, index, d.kh, d.kw,
              d.H + 2 * d.ph, d.W + 2 * d.pw);
    return false;
  }
  g->Ho = (d.H + 2 * d.ph - d.kh) / d.sh + 1;
  g->Wo = (d.W + 2 * d.pw - d.kw) / d.sw + 1;
  return true;
}

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

// ------------------------------------------------------------------------------------------------ entry points
// Null check of the descriptors and the plan of every one (the first step of *_workspace_bytes and *_accumulate).
template <typename Desc, typename Plan>
bool plans_of(const char* name, const Desc* descs, int n, bool (*plan_of)(const Desc&, int, Plan*),
              std::vector<Plan>* plans) {
  if (!descs) {
    set_error("%s: null descriptors", name);
    return false;
  }
  plans->resize(n);
  for (int i = 0; i < n; ++i)
    if (!plan_of(descs[i], i, &(*plans)[i])) return false;
  return true;
}

// *_workspace_bytes: bytes_of(plans), 0 after an error.
template <typename Desc, typename Plan, typename BytesOf>
size_t workspace_bytes(const char* name, const Desc* descs, int n, bool (*plan_of)(const Desc&, int, Plan*),
                       BytesOf bytes_of) {
  std::vector<Plan> plans;
  if (n <= 0 || !plans_of(name, descs, n, plan_of, &plans)) return 0;
  return bytes_of(plans);
}

// *_plan_flops: Plan::flops of every descriptor.
template <typename Desc, typename Plan>
int plan_flops(const char* name, const Desc* descs, int n, long long* out, bool (*plan_of)(const Desc&, int, Plan*)) {
  if (n <= 0) return CURV_OK;
  CURV_REQUIRE(descs && out, "%s: null argument", name);
  for (int i = 0; i < n; ++i) {
    Plan p;
    if (!plan_of(descs[i], i, &p)) return CURV_ERR_INVALID;
    out[i] = p.flops;
  }
  return CURV_OK;
}

// *_accumulate, after plans_of: every factor has its two tensors ...
template <typename Desc>
int require_src_dst(const char* name, const Desc* descs, int n) {
  for (int i = 0; i < n; ++i) CURV_REQUIRE(descs[i].src && descs[i].dst, "%s: factor %d: null src or dst", name, i);
  return CURV_OK;
}

// ... and the workspace holds `need` bytes at an `align`-byte boundary.
inline int require_workspace(const char* name, const void* workspace, size_t bytes, size_t need, size_t align) {
  if (!workspace || bytes < need || (reinterpret_cast<uintptr_t>(workspace) & (align - 1))) {
    set_error("%s: workspace too small (%zu < %zu bytes) or not %zu-byte aligned", name, bytes, need, align);
    return CURV_ERR_WORKSPACE;
  }
  return CURV_OK;
}

}  // namespace side
}  // namespace curv
