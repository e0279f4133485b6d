// mesh_cluster.hip — connected components of a triangle mesh over shared EDGES (Open3D's cluster_connected_triangles, what
// gs2dgs/utils/mesh_utils.py:22-43 post_process_mesh calls): lock-free union-find over the triangles, the triangles of an
// edge found through an open-addressing hash table.  The rules (adjacency, cluster numbering, counts, areas) are in
// include/scorp_gs.h; tests/mesh_cluster_reference.py restates them as a breadth-first search in plain Python.
//
// Three calls with the caller's scan between the last two, as in isosurface.hip:
//   link   fills the table and the parent array itself, then every triangle inserts its three edge keys.  A slot is claimed
//          by ONE 64-bit compare-and-swap on the key; the triangle then takes old = atomicMin(&owner[slot], tri) and, when the
//          slot had an owner, unites itself with it.  The owner is never stored by a separate plain write: the value an
//          arrival gets back is always an earlier arrival of the same edge (or nothing), so the atomicMin returns chain all
//          triangles of an edge together, however many there are.
//   roots  root[t] = find(t) and one byte root[t] == t; the inclusive scan of the bytes numbers the clusters.
//   stats  cluster[t] = scan[root[t]] - 1, triangle counts and float64 areas per cluster.  One component is usually almost
//          the whole mesh: the lanes of a wave that hold the same cluster combine first, and a wave issues one atomic per
//          distinct cluster it holds.  The counts are exact; the float64 area sums depend on the order in which the
//          waves' atomic adds arrive, in their last bits.
// A root is only ever hooked under a SMALLER index, so the root of a finished component is its smallest triangle: labels
// and numbering do not depend on the execution order, two calls give the same integers.  Nothing waits on another lane's
// progress: no locks, no spinning on a value someone else must write.  The union-find is union_find.hpp's; the table's claim, the face load and area, the wave
// loop of stats and the host checks are mesh_common.hpp's.
#include "mesh_common.hpp"
#include "union_find.hpp"

namespace scorp {
namespace {

constexpr int kClusterThreads = 256;

__global__ void __launch_bounds__(kClusterThreads) cluster_init_kernel(uint64_t *__restrict__ keys, int32_t *__restrict__ owner,
                                                                       uint64_t slots, int32_t *__restrict__ parent, int32_t faces) {
  const uint64_t i = (uint64_t)blockIdx.x * kClusterThreads + threadIdx.x;
  if (i < slots) {
    keys[i] = kEmptyKey;
    owner[i] = kEmptyOwner;
  }
  if (i < (uint64_t)faces) parent[i] = (int32_t)i;
}

__global__ void __launch_bounds__(kClusterThreads) cluster_link_kernel(const int32_t *__restrict__ tri_idx, int32_t faces,
                                                                       uint64_t *keys, int32_t *owner, uint64_t slot_mask,
                                                                       int32_t *parent) {
  const int64_t t64 = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
  if (t64 >= faces) return;
  const int32_t t = (int32_t)t64;
  const uint32_t v[3] = {(uint32_t)tri_idx[3 * t64], (uint32_t)tri_idx[3 * t64 + 1], (uint32_t)tri_idx[3 * t64 + 2]};
#pragma unroll
  for (int e = 0; e < 3; e++) {
    const uint32_t a = v[e], b = v[e == 2 ? 0 : e + 1];
    const uint64_t key = (uint64_t)(a < b ? a : b) << 32 | (uint64_t)(a < b ? b : a);
    if (key == kEmptyKey) continue;   // (two indices of -1: not a mesh; the empty marker is never claimed as an edge)
    // (with num_slots >= 6 num_faces at most half the slots are ever taken)
    const int64_t slot = table_claim(keys, slot_mask, key);
    if (slot == kTableFull) continue;
    const int32_t old = atomicMin(owner + slot, t);
    if (old != kEmptyOwner) unite(parent, t, old);
  }
}

// (after the link launch has ended: plain loads)
__global__ void __launch_bounds__(kClusterThreads) cluster_roots_kernel(const int32_t *__restrict__ parent, int32_t faces,
                                                                        int32_t *__restrict__ out_root,
                                                                        uint8_t *__restrict__ out_is_root) {
  const int64_t t = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
  if (t >= faces) return;
  const int32_t x = settled_root(parent, (int32_t)t);
  out_root[t] = x;
  out_is_root[t] = x == (int32_t)t;
}

__global__ void __launch_bounds__(kClusterThreads) cluster_stats_kernel(const int32_t *__restrict__ tri_idx,
                                                                        const float *__restrict__ verts, int64_t num_vertices,
                                                                        const int32_t *__restrict__ root,
                                                                        const int32_t *__restrict__ root_scan, int32_t faces,
                                                                        int32_t clusters, int32_t *__restrict__ out_cluster,
                                                                        int32_t *out_count, double *out_area) {
  const bool with_area = out_area != nullptr;   // (uniform: a kernel argument)
  const int64_t t = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
  int32_t c = -1;
  double area = 0.0;
  if (t < faces) {
    const int32_t r = root[t];
    if (r >= 0 && r < faces) c = root_scan[r] - 1;
    out_cluster[t] = c;
    if (c < 0 || c >= clusters) c = -1;   // (a scan that does not belong to these roots adds nothing out of bounds)
    if (with_area && c >= 0) {
      // (num_vertices has no upper bound here: 2^31 lets every non-negative index through)
      const Face f = load_face(tri_idx, t, (uint32_t)min(num_vertices, (int64_t)1 << 31));
      if (f.ok) area = 0.5 * norm3(face_cross(verts, f));
    }
  }
  // one atomic per distinct cluster in the wave (the lanes past the last triangle come with c = -1)
  wave_combine_equal(c, [&](int32_t lc, bool mine, int count, bool leads) {
    double s = 0.0;
    if (with_area) s = wave_sum_f64(mine ? area : 0.0);
    if (leads) {
      atomicAdd(out_count + lc, count);
      if (with_area) atomicAdd(out_area + lc, s);
    }
  });
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_mesh_cluster_link(const int32_t *faces, int64_t num_faces, uint64_t *keys, int32_t *owner, uint64_t num_slots,
                                       int32_t *parent, scorp_stream_t stream) {
  if (!faces || !keys || !owner || !parent) { set_error("mesh_cluster_link: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_faces(num_faces, "mesh_cluster_link")) return e;
  if (int e = check_slots(num_slots, (uint64_t)num_faces, 6, 32, "mesh_cluster_link", "num_faces")) return e;
  hipStream_t s = (hipStream_t)stream;
  cluster_init_kernel<<<blocks_for(num_slots, kClusterThreads), kClusterThreads, 0, s>>>(keys, owner, num_slots, parent, (int32_t)num_faces);
  SCORP_KERNEL_CHECK("cluster_init", 0, s);
  cluster_link_kernel<<<blocks_for((uint64_t)num_faces, kClusterThreads), kClusterThreads, 0, s>>>(faces, (int32_t)num_faces, keys, owner,
                                                                                     num_slots - 1, parent);
  SCORP_KERNEL_CHECK("cluster_link", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_cluster_roots(const int32_t *parent, int64_t num_faces, int32_t *out_root, uint8_t *out_is_root,
                                        scorp_stream_t stream) {
  if (!parent || !out_root || !out_is_root) { set_error("mesh_cluster_roots: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_faces(num_faces, "mesh_cluster_roots")) return e;
  hipStream_t s = (hipStream_t)stream;
  cluster_roots_kernel<<<blocks_for((uint64_t)num_faces, kClusterThreads), kClusterThreads, 0, s>>>(parent, (int32_t)num_faces, out_root, out_is_root);
  SCORP_KERNEL_CHECK("cluster_roots", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_cluster_stats(const int32_t *faces, const float *vertices, int64_t num_vertices, const int32_t *root,
                                        const int32_t *root_scan, int64_t num_faces, int64_t num_clusters, int32_t *out_cluster,
                                        int32_t *out_count, double *out_area, scorp_stream_t stream) {
  if (!faces || !root || !root_scan || !out_cluster || !out_count) { set_error("mesh_cluster_stats: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_faces(num_faces, "mesh_cluster_stats")) return e;
  if (num_clusters < 1 || num_clusters > num_faces) {
    set_error("mesh_cluster_stats: num_clusters must be in [1, num_faces]"); return SCORP_ERR_INVALID;
  }
  const bool area = out_area && vertices;
  if (area && num_vertices < 0) { set_error("mesh_cluster_stats: num_vertices < 0"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  SCORP_HIP_CHECK(hipMemsetAsync(out_count, 0, (size_t)num_clusters * sizeof(int32_t), s));
  if (area) SCORP_HIP_CHECK(hipMemsetAsync(out_area, 0, (size_t)num_clusters * sizeof(double), s));
  cluster_stats_kernel<<<blocks_for((uint64_t)num_faces, kClusterThreads), kClusterThreads, 0, s>>>(
      faces, area ? vertices : nullptr, area ? num_vertices : 0, root, root_scan, (int32_t)num_faces, (int32_t)num_clusters, out_cluster,
      out_count, area ? out_area : nullptr);
  SCORP_KERNEL_CHECK("cluster_stats", 0, s);
  return SCORP_OK;
}
