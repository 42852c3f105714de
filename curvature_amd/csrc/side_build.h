// What the convolution factor builds share: the check of a convolution geometry (the main build of syrk.hip and
// syrk_small.hip takes it too) and, for the side builds (kfac_half.hip, group_factor.hip, convt_factor.hip,
// persample.hip), the bodies of the *_workspace_bytes / *_plan_flops / *_accumulate entry points; the query of the plain
// build that the builds which end in curv_kfac_accumulate make (`plain_plan`), and the whole *_accumulate of the staged
// ones (`staged_accumulate`).  Argument batches live in kernarg.h.  A side build brings its own descriptor, `Plan`,
// `bool plan_of(const Desc&, int index, Plan*)` with its own limits, its kernels and its workspace layout.
#pragma once
#include "kernarg.h"

#include <algorithm>
#include <vector>

namespace curv {
namespace side {

// ------------------------------------------------------------------------------------------------ geometry
struct ConvGeom {
  int N, C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo;
};

// What is wrong with the source side of `d` (any descriptor with the fields N C H W kh kw sh sw ph pw), nullptr if
// nothing: sizes positive, padding not negative, fewer than 2^40 source elements.  Sets no error text.
template <typename Desc>
const char* source_geom_fault(const Desc& d, ConvGeom* g) {
  if (d.N < 1 || d.C < 1 || d.H < 1 || d.W < 1 || d.kh < 1 || d.kw < 1 || d.sh < 1 || d.sw < 1 || d.ph < 0 ||
      d.pw < 0)
    return "invalid geometry";
  if ((long long)d.N * d.C * d.H * d.W >= (1LL << 40)) return "too large (2^40 source elements or more)";
  *g = ConvGeom{d.N, d.C, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, 0, 0};
  return nullptr;
}

// ... and with the output of a convolution over it: the kernel fits the padded input; Ho / Wo.
template <typename Desc>
const char* conv_geom_fault(const Desc& d, ConvGeom* g) {
  if (const char* fault = source_geom_fault(d, g)) return fault;
  if (d.H + 2 * d.ph < d.kh || d.W + 2 * d.pw < d.kw) return "kernel larger than the padded input";
  g->Ho = (d.H + 2 * d.ph - d.kh) / d.sh + 1;
  g->Wo = (d.W + 2 * d.pw - d.kw) / d.sw + 1;
  return nullptr;
}

// The same two with the fault reported: "<prefix>: <unit> <index>: <fault> (<geometry>)".
template <typename Desc>
bool geom_ok(const char* fault, const Desc& d, const char* prefix, const char* unit, int index) {
  if (fault)
    set_error("%s: %s %d: %s (N %d C %d H %d W %d kernel %dx%d stride %dx%d padding %dx%d)", prefix, unit, index, fault,
              d.N, d.C, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw);
  return !fault;
}
template <typename Desc>
bool source_geom_of(const Desc& d, const char* prefix, const char* unit, int index, ConvGeom* g) {
  return geom_ok(source_geom_fault(d, g), d, prefix, unit, index);
}
template <typename Desc>
bool conv_geom_of(const Desc& d, const char* prefix, const char* unit, int index, ConvGeom* g) {
  return geom_ok(conv_geom_fault(d, g), d, prefix, unit, index);
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

// ------------------------------------------------------------------------------------------------ the plain sub-build
// What the plain build (curv_kfac_accumulate) needs for the `count` stand-in descriptors `sub` a side build hands it:
// `*bytes` of scratch and, unless `flops` is null, `*flops` = the sum of its plan's executed flops.  false where it
// refuses them: its text is in curv_last_error(), the caller words its own message.
inline bool plain_plan(const curv_factor_desc* sub, int count, size_t* bytes, long long* flops) {
  *bytes = curv_kfac_workspace_bytes(sub, count);
  if (*bytes == 0) return false;
  if (!flops) return true;
  std::vector<long long> info((size_t)CURV_PLAN_INFO_FIELDS * count);
  if (curv_kfac_plan_info(sub, count, info.data()) != CURV_OK) return false;
  *flops = 0;
  for (int i = 0; i < count; ++i) *flops += info[(size_t)CURV_PLAN_INFO_FIELDS * i + CURV_PLAN_INFO_FIELDS - 1];
  return true;
}

// ------------------------------------------------------------------------------------------------ staged builds
// A staged build (dilated_factor.hip, conv3d_factor.hip, reduce_factor.hip) writes, per factor, a stack or row matrix into
// scratch and runs the plain build on it.  Its Plan names `stage_bytes` (the staging region) and `build_bytes` (the plain
// build's scratch, never 0); the workspace is the SUM over the factors of the two, every factor's staging region followed
// by its build region: no factor waits for another's scratch.
template <typename Plan>
size_t staged_bytes(const std::vector<Plan>& plans) {
  size_t total = 0;
  for (const Plan& p : plans) total += p.stage_bytes + p.build_bytes;
  return total;
}

// *_accumulate of a staged build: build_one(stream, desc, plan, staging region, build region) for one factor after another.
template <typename Desc, typename Plan, typename BuildOne>
int staged_accumulate(const char* name, hipStream_t stream, const Desc* descs, int n, void* workspace, size_t bytes,
                      size_t align, bool (*plan_of)(const Desc&, int, Plan*), BuildOne build_one) {
  if (n <= 0) return CURV_OK;
  std::vector<Plan> plans;
  if (!plans_of(name, descs, n, plan_of, &plans)) return CURV_ERR_INVALID;
  int rc = require_src_dst(name, descs, n);
  if (rc == CURV_OK) rc = require_workspace(name, workspace, bytes, staged_bytes(plans), align);
  char* at = (char*)workspace;
  for (int i = 0; i < n && rc == CURV_OK; ++i) {
    rc = build_one(stream, descs[i], plans[i], at, at + plans[i].stage_bytes);
    at += plans[i].stage_bytes + plans[i].build_bytes;
  }
  return rc;
}

}  // namespace side
}  // namespace curv
