// cloud_filter.hip - cleaning a point cloud: exact k-nearest mean distances, exact radius counts and DBSCAN
// (scorp_amd/cloud.py; the rules R1 - R8 are the cloud block of include/scorp_gs.h, tests/cloud_reference.py restates them
// as a float64 brute force).  The third includer of icp_search.hpp: the density-sized grid, the stable radix sort by cell
// and the outward ring walk are the ICP's, the union-find is union_find.hpp's (mesh_cluster.hip's).
//
// Every kernel below has one thread per point, in cell order (thread t takes sorted point t, so a wave's queries are
// neighbours), and walks the rings of cells around the point's own cell:
//   knn      the k best (float64 d^2, index) so far sit sorted in the lane's column of two LDS arrays (a runtime-indexed
//            per-thread array would go to scratch).  The arrays are sized by k at the launch: 768 k bytes per workgroup
//            of 64 lanes, 15 KB at k = 20 and 24 KB at k = 32.  The list is icp_search.hpp's KBest WRITTEN OUT, statement
//            for statement: with its three counters members of a struct this kernel (alone of the three that keep such
//            a list) compiled to other code and ran 1 % slower, so it keeps them as locals.  Change the two together.
//   count    |N_r(i)|, and for DBSCAN the core flag and parent[i] = i.
//   link     every core point unites itself with its core neighbours of lower index.
//   roots    root and "is a root" per core point once every hook has landed; icp_scan_kernel numbers the roots.
//   border   a core point takes its root's number, any other point the number of its nearest core neighbour, or -1.
// DBSCAN is three walks (count, link, border) over one grid, built once; no neighbour list is stored.
//
// The grid only prunes (R8): cloud_search.hpp, shared with cloud_fpfh.hip, holds the workspace, rule R1's d^2, the original
// coordinates in cell order (W.tp) and the ring walk whose reach is widened by the bound on its fp32 roundings.
//
// A radius far larger than the cell edge makes each thread visit (2 r / h)^3 cells.  That is accepted: the cell edge
// follows the density (one point per cell on average), and a cleaning radius is a few spacings.
//
// No float atomics anywhere; the only atomics are the union-find's integer min and compare-and-swap, whose outcome (the
// smallest index of a component) does not depend on their order: every output is a function of the input alone.
#include "cloud_search.hpp"
#include "union_find.hpp"

// R1: every product and every sum of d^2 is rounded on its own
#pragma clang fp contract(off)

namespace scorp {
namespace {

constexpr int kCloudKnnThreads = 64;
constexpr int kCloudMaxK = 32;

// R3.  The walk ends when everything outside ring k's box is provably farther than the k-th best.
__global__ void __launch_bounds__(kCloudKnnThreads) cloud_knn_kernel(const float4 *__restrict__ tq, const float4 *__restrict__ tp, int n, int k,
                                                                     int knn, const uint32_t *__restrict__ cell_start,
                                                                     const IcpGrid *__restrict__ g, double *__restrict__ out_mean,
                                                                     int32_t *__restrict__ out_neighbors) {
  extern __shared__ double cloud_knn_lds[];   // k rows of 64 d^2, then k rows of 64 indices: 12 k 64 bytes
  double (*nd)[kCloudKnnThreads] = (double (*)[kCloudKnnThreads])cloud_knn_lds;
  uint32_t (*ni)[kCloudKnnThreads] = (uint32_t (*)[kCloudKnnThreads])(cloud_knn_lds + (size_t)k * kCloudKnnThreads);
  const int lane = threadIdx.x;
  const int i = blockIdx.x * kCloudKnnThreads + lane;
  if (i >= n) return;
  const float4 me = tp[i];
  const uint32_t self = __float_as_uint(me.w);
  const CloudWalk walk(tq[i], g);
  int cnt = 0;
  double kth = __builtin_inf();   // d^2 of the k-th best once the list is full
  uint32_t kth_id = 0xFFFFFFFFu;
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) {
      const float4 q = tp[t];
      const double d2 = cloud_d2(me, q);
      const uint32_t id = __float_as_uint(q.w);
      if (cnt == k && !(d2 < kth || (d2 == kth && id < kth_id))) return;
      int pos = cnt < k ? cnt : k - 1;   // the free slot, or the last entry, which leaves
      while (pos > 0) {
        const double pd = nd[pos - 1][lane];
        const uint32_t pi = ni[pos - 1][lane];
        if (!(pd > d2 || (pd == d2 && pi > id))) break;
        nd[pos][lane] = pd;
        ni[pos][lane] = pi;
        pos--;
      }
      nd[pos][lane] = d2;
      ni[pos][lane] = id;
      if (cnt < k) cnt++;
      if (cnt == k) { kth = nd[k - 1][lane]; kth_id = ni[k - 1][lane]; }
    });
  };
  walk.run(visit, [&]() { return cnt == k ? walk.reach(kth) : (float)__builtin_inf(); });
  double sum = 0.0;
  for (int a = 0; a < cnt; a++) sum = sum + sqrt(nd[a][lane]);
  out_mean[self] = sum / (double)k;
  if (out_neighbors) {
    for (int a = 0; a < knn; a++) out_neighbors[(size_t)self * knn + a] = a < cnt ? (int32_t)ni[a][lane] : -1;
  }
}

// R2, and R4 for DBSCAN (core_sorted and parent non-NULL): the count, the core flag in cell order and by index, parent[i] = i.
__global__ void __launch_bounds__(kCloudThreads) cloud_count_kernel(const float4 *__restrict__ tq, const float4 *__restrict__ tp, int n, double r2,
                                                                    const uint32_t *__restrict__ cell_start, const IcpGrid *__restrict__ g,
                                                                    int32_t *__restrict__ out_count, int min_points,
                                                                    uint8_t *__restrict__ core_sorted, uint8_t *__restrict__ out_core,
                                                                    int32_t *__restrict__ parent) {
  const int i = blockIdx.x * kCloudThreads + threadIdx.x;
  if (i >= n) return;
  const float4 me = tp[i];
  const uint32_t self = __float_as_uint(me.w);
  const CloudWalk walk(tq[i], g);
  const float reach = walk.reach(r2);
  int cnt = 0;
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) { cnt += cloud_d2(me, tp[t]) <= r2; });
  };
  walk.run(visit, [&]() { return reach; });
  if (out_count) out_count[self] = cnt;
  if (core_sorted) {
    const uint8_t c = cnt >= min_points;
    core_sorted[i] = c;
    if (out_core) out_core[self] = c;
    parent[self] = (int32_t)self;
  }
}

// R5: the edges of the core graph.  N_eps is symmetric (R1), so each edge is taken once, from its higher end.
__global__ void __launch_bounds__(kCloudThreads) cloud_link_kernel(const float4 *__restrict__ tq, const float4 *__restrict__ tp, int n, double r2,
                                                                   const uint32_t *__restrict__ cell_start, const IcpGrid *__restrict__ g,
                                                                   const uint8_t *__restrict__ core_sorted, int32_t *parent) {
  const int i = blockIdx.x * kCloudThreads + threadIdx.x;
  if (i >= n || !core_sorted[i]) return;
  const float4 me = tp[i];
  const uint32_t self = __float_as_uint(me.w);
  const CloudWalk walk(tq[i], g);
  const float reach = walk.reach(r2);
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) {
      if (!core_sorted[t]) return;
      const float4 q = tp[t];
      const uint32_t id = __float_as_uint(q.w);
      if (id < self && cloud_d2(me, q) <= r2) unite(parent, (int32_t)self, (int32_t)id);
    });
  };
  walk.run(visit, [&]() { return reach; });
}

// (after the link launch has ended: plain loads)  flag[i] = 1 for the smallest core index of a cluster; flag[n] = 0 is the
// slot in which the exclusive scan leaves the number of clusters.
__global__ void __launch_bounds__(kCloudThreads) cloud_roots_kernel(const float4 *__restrict__ tp, int n, const uint8_t *__restrict__ core_sorted,
                                                                    const int32_t *__restrict__ parent, int32_t *__restrict__ root,
                                                                    uint32_t *__restrict__ flag) {
  const int i = blockIdx.x * kCloudThreads + threadIdx.x;
  if (i == 0) flag[n] = 0u;
  if (i >= n) return;
  const int32_t self = (int32_t)__float_as_uint(tp[i].w);
  const int32_t r = core_sorted[i] ? settled_root(parent, self) : -1;
  root[self] = r;
  flag[self] = r == self;
}

// R5 numbering and R6.  number[] is the exclusive scan of the root flags: number[r] is the label of the cluster whose
// smallest core index is r.
__global__ void __launch_bounds__(kCloudThreads) cloud_border_kernel(const float4 *__restrict__ tq, const float4 *__restrict__ tp, int n, double r2,
                                                                     const uint32_t *__restrict__ cell_start, const IcpGrid *__restrict__ g,
                                                                     const uint8_t *__restrict__ core_sorted, const int32_t *__restrict__ root,
                                                                     const uint32_t *__restrict__ number, int32_t *__restrict__ out_labels,
                                                                     int32_t *__restrict__ out_num_clusters) {
  const int i = blockIdx.x * kCloudThreads + threadIdx.x;
  if (i == 0) *out_num_clusters = (int32_t)number[n];
  if (i >= n) return;
  const float4 me = tp[i];
  const uint32_t self = __float_as_uint(me.w);
  if (core_sorted[i]) {
    out_labels[self] = (int32_t)number[root[self]];
    return;
  }
  const CloudWalk walk(tq[i], g);
  const float reach = walk.reach(r2);
  double best = __builtin_inf();
  uint32_t bidx = 0xFFFFFFFFu;
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) {
      if (!core_sorted[t]) return;
      const float4 q = tp[t];
      const double d2 = cloud_d2(me, q);
      const uint32_t id = __float_as_uint(q.w);
      if (d2 <= r2 && (d2 < best || (d2 == best && id < bidx))) { best = d2; bidx = id; }
    });
  };
  walk.run(visit, [&]() { return reach; });
  out_labels[self] = bidx == 0xFFFFFFFFu ? -1 : (int32_t)number[root[bidx]];
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_cloud_workspace_bytes(int32_t n) { return CloudLayout(n > 0 ? n : 1).total; }

extern "C" int scorp_cloud_knn_distance(const float *points, int32_t n, int32_t knn, double *out_mean_distance, int32_t *out_neighbors,
                                        void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  if (knn < 1 || knn > kCloudMaxK) { set_error("cloud_knn_distance: knn must be in [1, %d]", kCloudMaxK); return SCORP_ERR_INVALID; }
  if (int e = cloud_check("cloud_knn_distance", points, n, out_mean_distance != nullptr, workspace, workspace_bytes)) return e;
  const CloudLayout L(n);
  const CloudWorkspace W(workspace, L);
  hipStream_t s = (hipStream_t)stream;
  if (int e = cloud_build(points, n, L, W, s)) return e;
  const int k = knn < n ? knn : n;
  cloud_knn_kernel<<<(n + kCloudKnnThreads - 1) / kCloudKnnThreads, kCloudKnnThreads, (size_t)k * kCloudKnnThreads * 12, s>>>(
      W.icp.tq, W.tp, n, k, knn, W.icp.cell_start, W.icp.g, out_mean_distance, out_neighbors);
  SCORP_KERNEL_CHECK("cloud_knn", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_cloud_radius_count(const float *points, int32_t n, double radius, int32_t *out_count, void *workspace,
                                        size_t workspace_bytes, scorp_stream_t stream) {
  if (int e = cloud_check_radius("cloud_radius_count", "radius", radius)) return e;
  if (int e = cloud_check("cloud_radius_count", points, n, out_count != nullptr, workspace, workspace_bytes)) return e;
  const CloudLayout L(n);
  const CloudWorkspace W(workspace, L);
  hipStream_t s = (hipStream_t)stream;
  if (int e = cloud_build(points, n, L, W, s)) return e;
  cloud_count_kernel<<<(n + kCloudThreads - 1) / kCloudThreads, kCloudThreads, 0, s>>>(W.icp.tq, W.tp, n, radius * radius, W.icp.cell_start,
                                                                                     W.icp.g, out_count, 0, nullptr, nullptr, nullptr);
  SCORP_KERNEL_CHECK("cloud_count", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_cloud_dbscan(const float *points, int32_t n, double eps, int32_t min_points, int32_t *out_labels, uint8_t *out_core,
                                  int32_t *out_count, int32_t *out_num_clusters, void *workspace, size_t workspace_bytes,
                                  scorp_stream_t stream) {
  if (int e = cloud_check_radius("cloud_dbscan", "eps", eps)) return e;
  if (min_points < 1) { set_error("cloud_dbscan: min_points < 1"); return SCORP_ERR_INVALID; }
  if (int e = cloud_check("cloud_dbscan", points, n, out_labels && out_num_clusters, workspace, workspace_bytes)) return e;
  const CloudLayout L(n);
  const CloudWorkspace W(workspace, L);
  hipStream_t s = (hipStream_t)stream;
  if (int e = cloud_build(points, n, L, W, s)) return e;
  const unsigned blocks = (n + kCloudThreads - 1) / kCloudThreads;
  const double r2 = eps * eps;
  cloud_count_kernel<<<blocks, kCloudThreads, 0, s>>>(W.icp.tq, W.tp, n, r2, W.icp.cell_start, W.icp.g, out_count, min_points, W.core, out_core,
                                                      W.parent);
  SCORP_KERNEL_CHECK("cloud_count", 0, s);
  cloud_link_kernel<<<blocks, kCloudThreads, 0, s>>>(W.icp.tq, W.tp, n, r2, W.icp.cell_start, W.icp.g, W.core, W.parent);
  SCORP_KERNEL_CHECK("cloud_link", 0, s);
  cloud_roots_kernel<<<blocks, kCloudThreads, 0, s>>>(W.tp, n, W.core, W.parent, W.root, W.flag);
  SCORP_KERNEL_CHECK("cloud_roots", 0, s);
  icp_scan_kernel<<<1, 1024, 0, s>>>(W.flag, (int64_t)n + 1);
  SCORP_KERNEL_CHECK("icp_scan", 0, s);
  cloud_border_kernel<<<blocks, kCloudThreads, 0, s>>>(W.icp.tq, W.tp, n, r2, W.icp.cell_start, W.icp.g, W.core, W.root, W.flag, out_labels,
                                                       out_num_clusters);
  SCORP_KERNEL_CHECK("cloud_border", 0, s);
  return SCORP_OK;
}
