// mesh_smooth.hip — face and vertex normals of a triangle mesh, Laplacian / Taubin smoothing half-steps and the normal map of
// a rendered mesh (scorp_amd/mesh/smooth.py; the rules are the numbered mesh-smooth block of include/scorp_gs.h,
// tests/mesh_smooth_reference.py restates them as per-vertex loops in Python floats).
//
//   face normals    one thread per face: rule 5.
//   vertex normals  one thread per vertex: walks its slice of the corner CSR (vertex -> incident faces, ascending), rule 6.
//   smooth step     one thread per vertex: walks its slice of the neighbour CSR (vertex -> neighbouring vertices,
//                   ascending), rule 7.  Jacobi: it reads one buffer and writes another.
//   normal map      one thread per (view, pixel) of a MeshRender's face and barycentric maps.
// Every sum is float64, in the CSR's order, with contraction off, and rounded to float32 once: the results are a function
// of the inputs alone and equal the numpy form bit for bit.  The adjacency is built by torch sorts (smooth.py).  A slice is
// clamped to its array and an index outside its range is skipped, so no input makes a kernel read out of bounds.  The
// valence is unbounded: plain loops, no register arrays.  No kernel uses LDS, scratch or a float atomic
// (tests/test_mesh_smooth_resources.py).  The vector type, the face load and cross product, the CSR slice and the host
// checks are mesh_common.hpp's.
#include "mesh_common.hpp"

namespace scorp {
namespace {

constexpr int kMeshSmoothThreads = 256;
constexpr int kMeshSmoothMaxViews = 65535;     // the views are the grid's y dimension
constexpr int kMeshSmoothMaxSide = 16384;
constexpr int kMeshSmoothMaxSteps = 1 << 20;

// rule 5 (unit3 is its x / sqrt((x^2 + y^2) + z^2)): the cross product of the face's two edges out of its first corner;
// false: an index outside [0, Nv)
__device__ __forceinline__ bool face_cross_at(const float *__restrict__ verts, int32_t Nv, const int32_t *__restrict__ faces, int64_t f,
                                           Vec3d &n) {
  const Face face = load_face(faces, f, Nv);
  if (face.ok) n = face_cross(verts, face);
  return face.ok;
}

__global__ void __launch_bounds__(kMeshSmoothThreads) mesh_face_normals_kernel(const float *__restrict__ verts, int32_t Nv,
                                                                                const int32_t *__restrict__ faces, int64_t F,
                                                                                int normalized, float *__restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * kMeshSmoothThreads + threadIdx.x;
  if (f >= F) return;
  Vec3d n = {0.0, 0.0, 0.0};
  if (face_cross_at(verts, Nv, faces, f, n) && normalized) n = unit3(n);
  store3(out, f, n);
}

__global__ void __launch_bounds__(kMeshSmoothThreads) mesh_vertex_normals_kernel(const float *__restrict__ verts, int32_t Nv,
                                                                                  const int32_t *__restrict__ faces, int64_t F,
                                                                                  const int32_t *__restrict__ corner_offsets,
                                                                                  const int32_t *__restrict__ corner_faces,
                                                                                  int weighting, float *__restrict__ out) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kMeshSmoothThreads + threadIdx.x;
  if (v >= Nv) return;
  const Range r = csr_range(corner_offsets, v, 3 * F);
  Vec3d s = {0.0, 0.0, 0.0};
  for (int64_t k = r.beg; k < r.end; k++) {
    const int32_t f = corner_faces[k];
    Vec3d n;
    if ((uint32_t)f >= (uint32_t)F || !face_cross_at(verts, Nv, faces, f, n)) continue;
    if (weighting == SCORP_MESH_NORMALS_UNIFORM) n = unit3(n);
    s.x = s.x + n.x;
    s.y = s.y + n.y;
    s.z = s.z + n.z;
  }
  store3(out, v, unit3(s));
}

__global__ void __launch_bounds__(kMeshSmoothThreads) mesh_smooth_step_kernel(const float *__restrict__ src, int32_t Nv,
                                                                               const int32_t *__restrict__ offsets,
                                                                               const int32_t *__restrict__ neighbors,
                                                                               const uint8_t *__restrict__ fixed, double factor,
                                                                               int weights, float *__restrict__ dst) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kMeshSmoothThreads + threadIdx.x;
  if (v >= Nv) return;
  const float px = src[3 * v], py = src[3 * v + 1], pz = src[3 * v + 2];
  float ox = px, oy = py, oz = pz;
  if (!(fixed && fixed[v])) {
    const Range r = csr_range(offsets, v, max((int64_t)offsets[Nv], (int64_t)0));
    const Vec3d p = {(double)px, (double)py, (double)pz};
    Vec3d s = {0.0, 0.0, 0.0};
    double W = 0.0;
    int64_t used = 0;
    for (int64_t k = r.beg; k < r.end; k++) {
      const int32_t j = neighbors[k];
      if ((uint32_t)j >= (uint32_t)Nv) continue;
      const Vec3d q = load3(src, j);
      double w = 1.0;
      if (weights == SCORP_MESH_SMOOTH_INVERSE_DISTANCE) {
        w = 1.0 / (norm3(sub3(p, q)) + 1e-12);
      }
      s.x = s.x + w * q.x;
      s.y = s.y + w * q.y;
      s.z = s.z + w * q.z;
      W = W + w;
      used++;
    }
    if (used > 0) {
      ox = (float)(p.x + factor * (s.x / W - p.x));
      oy = (float)(p.y + factor * (s.y / W - p.y));
      oz = (float)(p.z + factor * (s.z / W - p.z));
    }
  }
  dst[3 * v] = ox;
  dst[3 * v + 1] = oy;
  dst[3 * v + 2] = oz;
}

__global__ void __launch_bounds__(kMeshSmoothThreads) mesh_normal_map_kernel(const float *__restrict__ verts, int32_t Nv,
                                                                              const int32_t *__restrict__ faces, int64_t F,
                                                                              const float *__restrict__ normals,
                                                                              const int32_t *__restrict__ face_map,
                                                                              const float *__restrict__ bary, int H, int W,
                                                                              float *__restrict__ out) {
#pragma clang fp contract(off)
  const size_t hw = (size_t)H * (size_t)W;
  const size_t p = (size_t)blockIdx.x * kMeshSmoothThreads + threadIdx.x;
  if (p >= hw) return;
  const size_t view = blockIdx.y;
  const int32_t f = face_map[view * hw + p];
  Vec3d n = {0.0, 0.0, 0.0};
  if ((uint32_t)f < (uint32_t)F) {
    if (normals) {
      const Face face = load_face(faces, f, Nv);
      if (face.ok) {
        const float *b = bary + view * 3 * hw + p;
        const double b0 = (double)b[0], b1 = (double)b[hw], b2 = (double)b[2 * hw];
        const Vec3d na = load3(normals, face.a), nb = load3(normals, face.b), nc = load3(normals, face.c);
        n.x = (b0 * na.x + b1 * nb.x) + b2 * nc.x;
        n.y = (b0 * na.y + b1 * nb.y) + b2 * nc.y;
        n.z = (b0 * na.z + b1 * nb.z) + b2 * nc.z;
        n = unit3(n);
      }
    } else if (face_cross_at(verts, Nv, faces, f, n)) {
      n = unit3(n);
    }
  }
  float *o = out + view * 3 * hw + p;
  o[0] = (float)n.x;
  o[hw] = (float)n.y;
  o[2 * hw] = (float)n.z;
}

int check_sizes(const char *what, int64_t Nv, int64_t F) {
  if (int e = check_vertices(Nv, what, true)) return e;
  return check_faces(F, what, 0, true);
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_mesh_face_normals(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                       int32_t normalized, float *out_normals, scorp_stream_t stream) {
  if (int e = check_sizes("mesh_face_normals", num_vertices, num_faces)) return e;
  if (num_faces == 0) return SCORP_OK;
  if (!vertices || !faces || !out_normals) { set_error("mesh_face_normals: NULL argument"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  mesh_face_normals_kernel<<<blocks_for((size_t)num_faces, kMeshSmoothThreads), kMeshSmoothThreads, 0, s>>>(vertices, (int32_t)num_vertices, faces,
                                                                                               num_faces, normalized != 0, out_normals);
  SCORP_KERNEL_CHECK("mesh_face_normals", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_vertex_normals(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                         const int32_t *corner_offsets, const int32_t *corner_faces, int32_t weighting,
                                         float *out_normals, scorp_stream_t stream) {
  if (int e = check_sizes("mesh_vertex_normals", num_vertices, num_faces)) return e;
  if (weighting != SCORP_MESH_NORMALS_AREA && weighting != SCORP_MESH_NORMALS_UNIFORM) { set_error("mesh_vertex_normals: unknown weighting %d", weighting); return SCORP_ERR_INVALID; }
  if (!vertices || !corner_offsets || !out_normals || (num_faces > 0 && (!faces || !corner_faces))) { set_error("mesh_vertex_normals: NULL argument"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  mesh_vertex_normals_kernel<<<blocks_for((size_t)num_vertices, kMeshSmoothThreads), kMeshSmoothThreads, 0, s>>>(
      vertices, (int32_t)num_vertices, faces, num_faces, corner_offsets, corner_faces, weighting, out_normals);
  SCORP_KERNEL_CHECK("mesh_vertex_normals", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_smooth(const float *vertices, int64_t num_vertices, const int32_t *offsets, const int32_t *neighbors,
                                 const uint8_t *fixed, const double *factors, int32_t num_steps, int32_t weights, float *scratch,
                                 float *out, scorp_stream_t stream) {
  if (int e = check_vertices(num_vertices, "mesh_smooth", true)) return e;
  if (num_steps < 0 || num_steps > kMeshSmoothMaxSteps) { set_error("mesh_smooth: num_steps must be in [0, 2^20]; got %d", num_steps); return SCORP_ERR_INVALID; }
  if (weights != SCORP_MESH_SMOOTH_UNIFORM && weights != SCORP_MESH_SMOOTH_INVERSE_DISTANCE) { set_error("mesh_smooth: unknown weights %d", weights); return SCORP_ERR_INVALID; }
  if (!vertices || !out || (num_steps > 0 && (!offsets || !factors)) || (num_steps > 1 && !scratch)) { set_error("mesh_smooth: NULL argument"); return SCORP_ERR_INVALID; }
  if (out == vertices || (num_steps > 1 && (scratch == vertices || scratch == out))) { set_error("mesh_smooth: vertices, scratch and out must be three buffers"); return SCORP_ERR_INVALID; }
  for (int32_t k = 0; k < num_steps; k++)
    if (!(factors[k] == factors[k]) || factors[k] - factors[k] != 0.0) { set_error("mesh_smooth: factor %d is not finite", k); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  if (num_steps == 0) {
    SCORP_HIP_CHECK(hipMemcpyAsync(out, vertices, (size_t)num_vertices * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SCORP_OK;
  }
  const float *src = vertices;
  for (int32_t k = 0; k < num_steps; k++) {
    float *dst = ((num_steps - 1 - k) & 1) ? scratch : out;   // the last half-step lands in out
    mesh_smooth_step_kernel<<<blocks_for((size_t)num_vertices, kMeshSmoothThreads), kMeshSmoothThreads, 0, s>>>(
        src, (int32_t)num_vertices, offsets, neighbors, fixed, factors[k], weights, dst);
    SCORP_KERNEL_CHECK("mesh_smooth_step", 0, s);
    src = dst;
  }
  return SCORP_OK;
}

extern "C" int scorp_mesh_normal_map(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                     const float *vertex_normals, const int32_t *face_map, const float *barycentric, int32_t num_views,
                                     int32_t height, int32_t width, float *out_normals, scorp_stream_t stream) {
  if (int e = check_sizes("mesh_normal_map", num_vertices, num_faces)) return e;
  if (num_views < 1 || num_views > kMeshSmoothMaxViews) { set_error("mesh_normal_map: num_views must be in [1, 65535]; got %d", num_views); return SCORP_ERR_INVALID; }
  if (height < 1 || height > kMeshSmoothMaxSide || width < 1 || width > kMeshSmoothMaxSide) { set_error("mesh_normal_map: height and width must be in [1, 16384]; got %d x %d", height, width); return SCORP_ERR_INVALID; }
  if (!vertices || !face_map || !out_normals || (num_faces > 0 && !faces)) { set_error("mesh_normal_map: NULL argument"); return SCORP_ERR_INVALID; }
  if (vertex_normals && !barycentric) { set_error("mesh_normal_map: vertex_normals without barycentric"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  mesh_normal_map_kernel<<<dim3(blocks_for((size_t)height * (size_t)width, kMeshSmoothThreads), (unsigned)num_views), kMeshSmoothThreads, 0, s>>>(
      vertices, (int32_t)num_vertices, faces, num_faces, vertex_normals, face_map, barycentric, height, width, out_normals);
  SCORP_KERNEL_CHECK("mesh_normal_map", 0, s);
  return SCORP_OK;
}
