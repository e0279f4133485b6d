// cloud_search.hpp - what cloud_filter.hip (outlier removal, DBSCAN) and cloud_fpfh.hip (the FPFH descriptor) share on top
// of icp_search.hpp: the workspace of a cloud call, rule R1's float64 d^2, the original coordinates in cell order (tp) and
// the ring walk with its widened reach (rule R8).  Everything is in an unnamed namespace: each includer gets its own copy
// of the gather kernel.
//
// The grid only prunes (R8).  Points are filed by their fp32 coordinates relative to the box centre; every decision is
// taken on the float64 d^2 of the ORIGINAL float32 coordinates, which travel in cell order next to tq (W.tp, index in .w;
// gathering them by index instead costs a dependent 12-byte load per candidate and was not pursued).  The ring walk ends
// when lb^2 > reach, lb its fp32 bound on the distance from the query to everything filed outside ring k's box.  That
// bound is off by roundings: of the two relative coordinates (2^-24 of their size each), of the filing
// (v - lo) * inv_h (two roundings, and inv_h and h are each rounded from 1 / h and h), of lo + m h in the walk (two) and
// of the last subtraction.  With G = max over the axes of |lo| + dims h - no smaller than any of those quantities - they
// add up to less than 10 * 2^-24 G.  CloudWalk::reach() therefore hands the walk (sqrt(R) + 2^-19 G)^2 (1 + 1e-6), rounded
// to fp32, for a float64 reach R: the walk ends only when everything outside is provably farther than R.  While a k-best
// list is not full the reach is +inf and the walk ends only when nothing is left outside the box.
#pragma once
#include "icp_search.hpp"

// R1: every product and every sum of d^2 is rounded on its own
#pragma clang fp contract(off)

namespace scorp {
namespace {

constexpr int kCloudThreads = 256;

// The workspace of one call: the ICP layout of a target of n points, then the original coordinates in cell order and
// DBSCAN's arrays.
struct CloudLayout {
  IcpLayout icp;
  size_t tp, core, parent, root, flag, total;
  explicit CloudLayout(int64_t n) : icp(0, n, 0, 1) {
    size_t off = icp.total;
    tp = off; off = align_up(off + (size_t)n * 16, 256);
    core = off; off = align_up(off + (size_t)n, 256);
    parent = off; off = align_up(off + (size_t)n * 4, 256);
    root = off; off = align_up(off + (size_t)n * 4, 256);
    flag = off; off = align_up(off + ((size_t)n + 1) * 4, 256);
    total = off;
  }
};

// R1
__device__ __forceinline__ double cloud_d2(const float4 &a, const float4 &b) {
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// the original coordinates of sorted point t, its index in .w
__global__ void __launch_bounds__(kCloudThreads) cloud_gather_kernel(const float *__restrict__ pts, const float4 *__restrict__ tq, int n,
                                                                     float4 *__restrict__ tp) {
  const int t = blockIdx.x * kCloudThreads + threadIdx.x;
  if (t >= n) return;
  const float w = tq[t].w;
  const float *s = pts + (size_t)__float_as_uint(w) * 3;
  tp[t] = make_float4(s[0], s[1], s[2], w);
}

// IcpWalk with the widened reach.
struct CloudWalk : IcpWalk {
  double slack;   // 2^-19 G
  __device__ __forceinline__ CloudWalk(const float4 &me, const IcpGrid *__restrict__ g) : IcpWalk(me, g) {
    const double G = fmax(fmax(fabs((double)lx) + (double)dx * h, fabs((double)ly) + (double)dy * h), fabs((double)lz) + (double)dz * h);
    slack = G * (1.0 / 524288.0);
  }
  // the fp32 reach that lets the walk end only past a float64 d^2 of R (see the head of the file)
  __device__ __forceinline__ float reach(double R) const {
    const double t = sqrt(R) + slack;
    return (float)(t * t * (1.0 + 1e-6));   // (past FLT_MAX: +inf, the walk then visits everything)
  }
};

// ---- host ----

struct CloudWorkspace {
  IcpWorkspace icp;
  float4 *tp;
  uint8_t *core;
  int32_t *parent, *root;
  uint32_t *flag;
  CloudWorkspace(void *workspace, const CloudLayout &L) : icp(workspace, L.icp) {
    char *w = (char *)workspace;
    tp = (float4 *)(w + L.tp);
    core = (uint8_t *)(w + L.core);
    parent = (int32_t *)(w + L.parent);
    root = (int32_t *)(w + L.root);
    flag = (uint32_t *)(w + L.flag);
  }
};

// (`extra`: what the caller's workspace holds after the CloudLayout)
int cloud_check(const char *who, const float *points, int32_t n, bool pointers, const void *workspace, size_t workspace_bytes,
                size_t extra = 0) {
  if (n < 1) { set_error("%s: empty cloud", who); return SCORP_ERR_INVALID; }
  if (n > (1 << 30)) { set_error("%s: more than 2^30 points", who); return SCORP_ERR_INVALID; }
  if (!points || !pointers) { set_error("%s: NULL argument", who); return SCORP_ERR_INVALID; }
  return check_workspace(who, workspace, workspace_bytes, CloudLayout(n).total + extra);
}

int cloud_check_radius(const char *who, const char *name, double r) {
  if (!(r > 0.0) || !std::isfinite(r)) { set_error("%s: %s must be a positive finite number", who, name); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

// The grid over the cloud, the points sorted by cell, and their original coordinates in that order.
int cloud_build(const float *points, int n, const CloudLayout &L, const CloudWorkspace &W, hipStream_t stream) {
  if (int e = icp_build_target(points, n, L.icp, W.icp, stream)) return e;
  cloud_gather_kernel<<<(n + kCloudThreads - 1) / kCloudThreads, kCloudThreads, 0, stream>>>(points, W.icp.tq, n, W.tp);
  SCORP_KERNEL_CHECK("cloud_gather", 0, stream);
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp
