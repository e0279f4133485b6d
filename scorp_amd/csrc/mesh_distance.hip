// mesh_distance.hip — exact unsigned distance from points to a triangle mesh, area-weighted surface sampling, and the ICP
// grid search for plain point clouds (scorp_amd/mesh/distance.py; the rules are the numbered block of include/scorp_gs.h,
// tests/mesh_distance_reference.py restates them by brute force in another formulation).
//
//   build   the grid of icp_search.hpp over the vertices' bounding box, with 8 F as the density so that a cell is about
//           one triangle wide; every triangle is registered in every cell its (slightly padded) bounding box overlaps.  The
//           (cell, triangle) pairs are a CSR built by count, scan and fill.  Before that the pairs are only COUNTED: while
//           there are more than mesh_pair_cap(F) the cell edge grows by 1.25 and the count runs again (a host loop with
//           one small read-back per trip), so two scene-sized triangles never cost more than the cap.
//   query   the queries are sorted by Morton code (icp_sort_source, the ICP source's sort), one thread per query walks rings
//           of cells outward (icp_ring_walk in float64) and tests every candidate by the closest point on the
//           triangle (vertex, edge and face regions; a triangle with a zero normal is its three segments).  The result is
//           the minimum of (d^2, face) in lexicographic order and is written at the query's original position, so it does
//           not depend on the fill order of the pairs (atomics), on the sort or on how often a triangle is met.
//   sample  one thread per sample: stratified area coordinate, binary search in the caller's float64 prefix of the areas.
//   nearest one thin kernel over icp_build_target + icp_build_source + icp_nearest.
// No float is summed by atomics.  No kernel spills (tests/test_mesh_distance_resources.py).  The vector type, the face load
// and the host checks are mesh_common.hpp's; wave_sum_u64 and splitmix64 are common.hpp's.
#include "icp_search.hpp"
#include "mesh_common.hpp"

namespace scorp {
namespace {

constexpr int kMeshDistThreads = 256;
constexpr int64_t kMeshDistMaxQueries = 0x7FFFFFFF;
constexpr int kMeshDistMaxGrow = 64;        // 1.25^64 > 1e6 > kMaxGridDim: the grid is one cell long before
constexpr double kMeshCellPad = 1e-9;       // a triangle's cell range is padded by this many cells on either side

int64_t mesh_cell_cap(int64_t F) { const int64_t c = 8 * F + 64; return c > ((int64_t)1 << 30) ? (int64_t)1 << 30 : c; }
int64_t mesh_pair_cap(int64_t F) { return 8 * F + 4096; }

struct MeshDistLayout {
  size_t grid, total, cell_start, cursor, pairs, keys0, keys1, vals0, vals1, hist, bytes;
  int64_t tiles;
  MeshDistLayout(int64_t F, int64_t Q) {
    if (F < 0) F = 0;
    if (Q < 1) Q = 1;
    tiles = (Q + kRadixTile - 1) / kRadixTile;
    size_t off = 0;
    grid = off; off = align_up(off + sizeof(IcpGrid), 256);
    total = off; off = align_up(off + 8, 256);
    cell_start = off; off = align_up(off + ((size_t)mesh_cell_cap(F) + 1) * 4, 256);
    cursor = off; off = align_up(off + (size_t)mesh_cell_cap(F) * 4, 256);
    pairs = off; off = align_up(off + (size_t)mesh_pair_cap(F) * 4, 256);
    keys0 = off; off = align_up(off + (size_t)Q * 4, 256);
    keys1 = off; off = align_up(off + (size_t)Q * 4, 256);
    vals0 = off; off = align_up(off + (size_t)Q * 4, 256);
    vals1 = off; off = align_up(off + (size_t)Q * 4, 256);
    hist = off; off = align_up(off + (size_t)tiles * 256 * 4, 256);
    bytes = off;
  }
};

// rule 5: the closest point of the segment from a (e = b - a, ap = p - a); no division when the segment is a point
__device__ __forceinline__ Vec3d closest_on_segment(Vec3d a, Vec3d e, Vec3d ap) {
#pragma clang fp contract(off)
  const double t = dot3(ap, e), den = dot3(e, e);
  if (!(t > 0.0)) return a;
  if (t >= den) return along3(a, 1.0, e);
  return along3(a, t / den, e);
}

// rule 4 / 5: the closest point of triangle (A, B, C) to P.  A and P are relative to the grid centre; ab, ac, bc are the
// edges taken from the float32 inputs themselves (float64 differences of float32 values).
__device__ __forceinline__ Vec3d closest_on_triangle(Vec3d P, Vec3d A, Vec3d ab, Vec3d ac, Vec3d bc) {
#pragma clang fp contract(off)
  const Vec3d n = cross3(ab, ac);
  const Vec3d ap = sub3(P, A);
  if (n.x == 0.0 && n.y == 0.0 && n.z == 0.0) {   // collinear or repeated vertices: the union of the three segments
    const Vec3d B = along3(A, 1.0, ab), C = along3(A, 1.0, ac);
    const Vec3d c0 = closest_on_segment(A, ab, ap), c1 = closest_on_segment(B, bc, sub3(P, B));
    const Vec3d ca = {-ac.x, -ac.y, -ac.z};
    const Vec3d c2 = closest_on_segment(C, ca, sub3(P, C));
    const Vec3d u0 = sub3(P, c0), u1 = sub3(P, c1), u2 = sub3(P, c2);
    const double e0 = dot3(u0, u0), e1 = dot3(u1, u1), e2 = dot3(u2, u2);
    Vec3d best = c0;
    double eb = e0;
    if (e1 < eb) { best = c1; eb = e1; }
    if (e2 < eb) { best = c2; }
    return best;
  }
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) return A;                                   // vertex A
  const Vec3d bp = sub3(ap, ab);
  const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) return along3(A, 1.0, ab);                     // vertex B
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return along3(A, d1 / (d1 - d3), ab);   // edge AB
  const Vec3d cp = sub3(ap, ac);
  const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) return along3(A, 1.0, ac);                     // vertex C
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return along3(A, d2 / (d2 - d6), ac);   // edge AC
  const double va = d3 * d6 - d5 * d4;
  if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0)                  // edge BC
    return along3(along3(A, 1.0, ab), (d4 - d3) / ((d4 - d3) + (d5 - d6)), bc);
  const double s = dot3(n, ap) / dot3(n, n);                                 // the face: P minus its offset along the normal
  return {P.x - s * n.x, P.y - s * n.y, P.z - s * n.z};
}

struct MeshView {
  const float *__restrict__ verts;
  const int32_t *__restrict__ faces;
  int32_t Nv, F;
};

// (closest point, d^2) of face f to P; false when an index of the face is out of range
__device__ __forceinline__ bool face_distance(const MeshView &m, const double ct[3], int32_t f, Vec3d P, Vec3d &c, double &d2) {
#pragma clang fp contract(off)
  const Face t = load_face(m.faces, f, m.Nv);
  if (!t.ok) return false;
  const Vec3d a = load3(m.verts, t.a), b = load3(m.verts, t.b), cc = load3(m.verts, t.c);
  const Vec3d A = {a.x - ct[0], a.y - ct[1], a.z - ct[2]};
  c = closest_on_triangle(P, A, sub3(b, a), sub3(cc, a), sub3(cc, b));
  const Vec3d u = sub3(P, c);
  d2 = dot3(u, u);
  return true;
}

// rule 2: the cells [lo, hi] per axis the triangle's padded bounding box overlaps; false for a face with a bad index
__device__ __forceinline__ bool face_cells(const MeshView &m, const IcpGrid *__restrict__ g, int32_t f, int lo[3], int hi[3]) {
  const Face t = load_face(m.faces, f, m.Nv);
  if (!t.ok) return false;
  const double h = (double)g->h;
  for (int d = 0; d < 3; d++) {
    const double a = (double)m.verts[3 * (int64_t)t.a + d], b = (double)m.verts[3 * (int64_t)t.b + d],
                 c = (double)m.verts[3 * (int64_t)t.c + d];
    const double mn = fmin(a, fmin(b, c)) - g->ct[d], mx = fmax(a, fmax(b, c)) - g->ct[d];
    const double top = (double)(g->dims[d] - 1);
    lo[d] = (int)fmin(fmax(floor((mn - (double)g->lo[d]) / h - kMeshCellPad), 0.0), top);
    hi[d] = (int)fmin(fmax(floor((mx - (double)g->lo[d]) / h + kMeshCellPad), 0.0), top);
  }
  return true;
}

// the number of (cell, triangle) pairs of the current grid
__global__ void __launch_bounds__(kMeshDistThreads) mesh_pair_total_kernel(MeshView m, const IcpGrid *__restrict__ g,
                                                                            unsigned long long *total) {
  const int64_t f = (int64_t)blockIdx.x * kMeshDistThreads + threadIdx.x;
  unsigned long long n = 0;
  int lo[3], hi[3];
  if (f < m.F && face_cells(m, g, (int32_t)f, lo, hi))
    n = (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)(hi[1] - lo[1] + 1) * (unsigned long long)(hi[2] - lo[2] + 1);
  n = wave_sum_u64(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(total, n);
}

// rule 3: one more step of the cell edge; the origin and the centre stay
__global__ void mesh_grid_grow_kernel(IcpGrid *g, int last) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double h = (double)g->h * 1.25;
  int cells = 1;
  for (int d = 0; d < 3; d++) {
    const double pad = ((double)g->tlo[d] - g->ct[d]) - (double)g->lo[d];
    const double ext = (((double)g->thi[d] - g->ct[d]) + pad) - (double)g->lo[d];
    const double n = floor(ext / h) + 1.0;
    g->dims[d] = last ? 1 : (n >= 1.0 && n < kMaxGridDim ? (int)n : (n >= kMaxGridDim ? kMaxGridDim : 1));
    cells *= g->dims[d];
  }
  g->h = (float)h;
  g->inv_h = (float)(1.0 / h);
  g->ncells = cells;
}

__global__ void __launch_bounds__(kMeshDistThreads) mesh_pair_count_kernel(MeshView m, const IcpGrid *__restrict__ g, uint32_t *count) {
  const int64_t f = (int64_t)blockIdx.x * kMeshDistThreads + threadIdx.x;
  int lo[3], hi[3];
  if (f >= m.F || !face_cells(m, g, (int32_t)f, lo, hi)) return;
  const int dx = g->dims[0], dy = g->dims[1];
  for (int iz = lo[2]; iz <= hi[2]; iz++)
    for (int iy = lo[1]; iy <= hi[1]; iy++)
      for (int ix = lo[0]; ix <= hi[0]; ix++) atomicAdd(&count[(iz * dy + iy) * dx + ix], 1u);
}

// cursor[c] starts at cell_start[c]; the order inside a cell is the atomics' and no result depends on it
__global__ void __launch_bounds__(kMeshDistThreads) mesh_pair_fill_kernel(MeshView m, const IcpGrid *__restrict__ g, uint32_t *cursor,
                                                                           uint32_t *pairs, uint32_t cap) {
  const int64_t f = (int64_t)blockIdx.x * kMeshDistThreads + threadIdx.x;
  int lo[3], hi[3];
  if (f >= m.F || !face_cells(m, g, (int32_t)f, lo, hi)) return;
  const int dx = g->dims[0], dy = g->dims[1];
  for (int iz = lo[2]; iz <= hi[2]; iz++)
    for (int iy = lo[1]; iy <= hi[1]; iy++)
      for (int ix = lo[0]; ix <= hi[0]; ix++) {
        const uint32_t pos = atomicAdd(&cursor[(iz * dy + iy) * dx + ix], 1u);
        if (pos < cap) pairs[pos] = (uint32_t)f;
      }
}

__device__ __forceinline__ void store_miss(int64_t j, double *out_d2, int32_t *out_face, float *out_closest) {
  out_d2[j] = __builtin_inf();
  out_face[j] = -1;
  out_closest[3 * j] = out_closest[3 * j + 1] = out_closest[3 * j + 2] = __builtin_nanf("");
}

__global__ void __launch_bounds__(kMeshDistThreads) mesh_miss_kernel(int64_t Q, double *out_d2, int32_t *out_face, float *out_closest) {
  const int64_t j = (int64_t)blockIdx.x * kMeshDistThreads + threadIdx.x;
  if (j < Q) store_miss(j, out_d2, out_face, out_closest);
}

// rules 4 - 7: one thread per query, in Morton order; the result goes to the query's own position
__global__ void __launch_bounds__(kMeshDistThreads) mesh_query_kernel(MeshView m, const float *__restrict__ queries,
                                                                       const uint32_t *__restrict__ order, int64_t Q,
                                                                       const IcpGrid *__restrict__ g,
                                                                       const uint32_t *__restrict__ cell_start,
                                                                       const uint32_t *__restrict__ pairs, double max_d2,
                                                                       double *out_d2, int32_t *out_face, float *out_closest) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kMeshDistThreads + threadIdx.x;
  if (i >= Q) return;
  const int64_t j = order[i];
  const float qx = queries[3 * j], qy = queries[3 * j + 1], qz = queries[3 * j + 2];
  if (!(fabsf(qx) <= 3.4028235e38f && fabsf(qy) <= 3.4028235e38f && fabsf(qz) <= 3.4028235e38f)) {   // NaN or infinite
    store_miss(j, out_d2, out_face, out_closest);
    return;
  }
  const double ct[3] = {g->ct[0], g->ct[1], g->ct[2]};
  const Vec3d P = {(double)qx - ct[0], (double)qy - ct[1], (double)qz - ct[2]};
  double best = max_d2;
  {  // the distance to the vertices' bounding box: nothing is closer than that
    const double ex = fmax(fmax(((double)g->tlo[0] - ct[0]) - P.x, P.x - ((double)g->thi[0] - ct[0])), 0.0);
    const double ey = fmax(fmax(((double)g->tlo[1] - ct[1]) - P.y, P.y - ((double)g->thi[1] - ct[1])), 0.0);
    const double ez = fmax(fmax(((double)g->tlo[2] - ct[2]) - P.z, P.z - ((double)g->thi[2] - ct[2])), 0.0);
    if (!((ex * ex + ey * ey) + ez * ez <= best)) {
      store_miss(j, out_d2, out_face, out_closest);
      return;
    }
  }
  const double lx = (double)g->lo[0], ly = (double)g->lo[1], lz = (double)g->lo[2], h = (double)g->h;
  const int dx = g->dims[0], dy = g->dims[1], dz = g->dims[2];
  const int cx = (int)floor(fmin(fmax((P.x - lx) / h, -1.0), (double)dx));
  const int cy = (int)floor(fmin(fmax((P.y - ly) / h, -1.0), (double)dy));
  const int cz = (int)floor(fmin(fmax((P.z - lz) / h, -1.0), (double)dz));
  uint32_t bface = 0xFFFFFFFFu;
  // cells ca..cb of one grid row: one contiguous run of pairs
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) {
      const uint32_t f = pairs[t];
      if (f >= (uint32_t)m.F) return;
      Vec3d c;
      double d2;
      if (!face_distance(m, ct, (int32_t)f, P, c, d2)) return;
      if (d2 < best || (d2 == best && f < bface)) { best = d2; bface = f; }
    });
  };
  icp_ring_walk(P.x, P.y, P.z, cx, cy, cz, lx, ly, lz, h, dx, dy, dz, visit, [&]() { return best; });   // rule 6
  if (bface == 0xFFFFFFFFu) {
    store_miss(j, out_d2, out_face, out_closest);
    return;
  }
  Vec3d c;
  double d2;
  face_distance(m, ct, (int32_t)bface, P, c, d2);
  out_d2[j] = d2;
  out_face[j] = (int32_t)bface;
  out_closest[3 * j] = (float)(c.x + ct[0]);
  out_closest[3 * j + 1] = (float)(c.y + ct[1]);
  out_closest[3 * j + 2] = (float)(c.z + ct[2]);
}

// ---- the sampler ----

// the variate k of sample i: mix(mix(mix(seed) ^ i) ^ k), its upper 53 bits as a float64 in [0, 1)
__device__ __forceinline__ double sample_variate(uint64_t mixed_seed, uint64_t i, uint64_t k) {
  return (double)(splitmix64(splitmix64(mixed_seed ^ i) ^ k) >> 11) * 0x1p-53;
}

__global__ void __launch_bounds__(kMeshDistThreads) mesh_sample_kernel(MeshView m, const double *__restrict__ prefix, int64_t n,
                                                                        uint64_t mixed_seed, float *out_points, int32_t *out_faces,
                                                                        float *out_bary) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kMeshDistThreads + threadIdx.x;
  if (i >= n) return;
  const double total = prefix[m.F - 1];
  double t = (((double)i + sample_variate(mixed_seed, (uint64_t)i, 0)) / (double)n) * total;
  if (!(t < total)) t = nextafter(total, 0.0);
  int32_t lo = 0, hi = m.F - 1;          // the first face whose inclusive prefix exceeds t: never one of zero area
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (prefix[mid] > t) hi = mid; else lo = mid + 1;
  }
  const double s = sqrt(sample_variate(mixed_seed, (uint64_t)i, 1)), r2 = sample_variate(mixed_seed, (uint64_t)i, 2);
  const double w0 = 1.0 - s, w1 = s * (1.0 - r2), w2 = s * r2;
  out_faces[i] = lo;
  out_bary[3 * i] = (float)w0;
  out_bary[3 * i + 1] = (float)w1;
  out_bary[3 * i + 2] = (float)w2;
  const Face f = load_face(m.faces, lo, m.Nv);
  if (!f.ok) {
    out_points[3 * i] = out_points[3 * i + 1] = out_points[3 * i + 2] = __builtin_nanf("");
    return;
  }
  const Vec3d A = load3(m.verts, f.a), B = load3(m.verts, f.b), C = load3(m.verts, f.c);
  out_points[3 * i] = (float)((w0 * A.x + w1 * B.x) + w2 * C.x);
  out_points[3 * i + 1] = (float)((w0 * A.y + w1 * B.y) + w2 * C.y);
  out_points[3 * i + 2] = (float)((w0 * A.z + w1 * B.z) + w2 * C.z);
}

// ---- nearest point of a cloud ----

// sp = the queries in Morton order, order = their original positions; the rule of icp_nearest (fp32 d^2 on centre-relative
// coordinates, ties to the lower original index), then the pair's d^2 once more in float64
__global__ void __launch_bounds__(kMeshDistThreads) nearest_point_kernel(const float4 *__restrict__ sp, const uint32_t *__restrict__ order,
                                                                          int32_t nq, const float *__restrict__ cloud,
                                                                          const IcpGrid *__restrict__ g,
                                                                          const uint32_t *__restrict__ cell_start,
                                                                          const float4 *__restrict__ tq, double r2, float r2f,
                                                                          double *out_d2, int32_t *out_index) {
  const int i = blockIdx.x * kMeshDistThreads + threadIdx.x;
  if (i >= nq) return;
  const uint32_t j = order[i];
  const float4 p = sp[i];
  double d2 = __builtin_inf();
  int id = -1;
  if (fabsf(p.x) <= 3.4028235e38f && fabsf(p.y) <= 3.4028235e38f && fabsf(p.z) <= 3.4028235e38f) {
    const double x0 = (double)p.x - g->ct[0], x1 = (double)p.y - g->ct[1], x2 = (double)p.z - g->ct[2];
    id = icp_nearest((float)x0, (float)x1, (float)x2, r2f, g, cell_start, tq);
    if (id >= 0) {
      const double u0 = x0 - ((double)cloud[(size_t)id * 3 + 0] - g->ct[0]), u1 = x1 - ((double)cloud[(size_t)id * 3 + 1] - g->ct[1]),
                   u2 = x2 - ((double)cloud[(size_t)id * 3 + 2] - g->ct[2]);
      d2 = fma(u0, u0, fma(u1, u1, u2 * u2));
      if (!(d2 <= r2)) { id = -1; d2 = __builtin_inf(); }
    }
  }
  out_d2[j] = d2;
  out_index[j] = id;
}

int check_mesh_counts(int64_t Nv, int64_t F, const char *who) {
  if (int e = check_vertices(Nv, who, true)) return e;
  return check_faces(F, who, 1, true);
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_mesh_distance_workspace_bytes(int64_t num_faces, int64_t num_queries) {
  if (num_faces > kMeshMaxFaces || num_queries > kMeshDistMaxQueries) return 0;
  return MeshDistLayout(num_faces, num_queries).bytes;
}

extern "C" int scorp_mesh_distance_build(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                         void *workspace, size_t workspace_bytes, int64_t *out_header, scorp_stream_t stream) {
  if (!vertices || !faces) { set_error("mesh_distance_build: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_mesh_counts(num_vertices, num_faces, "mesh_distance_build")) return e;
  const MeshDistLayout L(num_faces, 1);
  if (int e = check_workspace("mesh_distance_build", workspace, workspace_bytes, L.bytes)) return e;
  hipStream_t s = (hipStream_t)stream;
  char *w = (char *)workspace;
  IcpGrid *g = (IcpGrid *)(w + L.grid);
  unsigned long long *total = (unsigned long long *)(w + L.total);
  uint32_t *cell_start = (uint32_t *)(w + L.cell_start), *cursor = (uint32_t *)(w + L.cursor), *pairs = (uint32_t *)(w + L.pairs);
  const MeshView m{vertices, faces, (int32_t)num_vertices, (int32_t)num_faces};
  const int64_t cell_cap = mesh_cell_cap(num_faces), pair_cap = mesh_pair_cap(num_faces);
  icp_bbox_kernel<<<1, 1024, 0, s>>>(vertices, (int)num_vertices, g->tlo, g->thi);
  SCORP_KERNEL_CHECK("icp_bbox", 0, s);
  const int64_t density = 8 * num_faces < ((int64_t)1 << 30) ? 8 * num_faces : (int64_t)1 << 30;
  icp_grid_setup_kernel<<<1, 64, 0, s>>>(g, (int)density, (int)cell_cap);
  SCORP_KERNEL_CHECK("icp_grid_setup", 0, s);
  unsigned long long n_pairs = 0;
  int grow = 0;
  for (;; grow++) {
    SCORP_HIP_CHECK(hipMemsetAsync(total, 0, 8, s));
    mesh_pair_total_kernel<<<blocks_for(num_faces, kMeshDistThreads), kMeshDistThreads, 0, s>>>(m, g, total);
    SCORP_KERNEL_CHECK("mesh_pair_total", 0, s);
    SCORP_HIP_CHECK(hipMemcpyAsync(&n_pairs, total, 8, hipMemcpyDeviceToHost, s));
    SCORP_HIP_CHECK(hipStreamSynchronize(s));
    if ((int64_t)n_pairs <= pair_cap) break;
    if (grow > kMeshDistMaxGrow) { set_error("mesh_distance_build: the pair count does not fall under the cap"); return SCORP_ERR_INVALID; }
    mesh_grid_grow_kernel<<<1, 64, 0, s>>>(g, grow == kMeshDistMaxGrow);
    SCORP_KERNEL_CHECK("mesh_grid_grow", 0, s);
  }
  IcpGrid host;
  SCORP_HIP_CHECK(hipMemcpyAsync(&host, g, sizeof(IcpGrid), hipMemcpyDeviceToHost, s));
  SCORP_HIP_CHECK(hipStreamSynchronize(s));
  if (host.ncells < 1 || host.ncells > cell_cap) { set_error("mesh_distance_build: %d cells above the cap", host.ncells); return SCORP_ERR_INVALID; }
  SCORP_HIP_CHECK(hipMemsetAsync(cell_start, 0, ((size_t)host.ncells + 1) * 4, s));
  mesh_pair_count_kernel<<<blocks_for(num_faces, kMeshDistThreads), kMeshDistThreads, 0, s>>>(m, g, cell_start);
  SCORP_KERNEL_CHECK("mesh_pair_count", 0, s);
  icp_scan_kernel<<<1, 1024, 0, s>>>(cell_start, (int64_t)host.ncells + 1);
  SCORP_KERNEL_CHECK("icp_scan", 0, s);
  SCORP_HIP_CHECK(hipMemcpyAsync(cursor, cell_start, (size_t)host.ncells * 4, hipMemcpyDeviceToDevice, s));
  mesh_pair_fill_kernel<<<blocks_for(num_faces, kMeshDistThreads), kMeshDistThreads, 0, s>>>(m, g, cursor, pairs, (uint32_t)pair_cap);
  SCORP_KERNEL_CHECK("mesh_pair_fill", 0, s);
  if (out_header) {
    out_header[0] = (int64_t)n_pairs; out_header[1] = pair_cap; out_header[2] = host.ncells; out_header[3] = cell_cap;
    out_header[4] = host.dims[0]; out_header[5] = host.dims[1]; out_header[6] = host.dims[2]; out_header[7] = grow;
  }
  return SCORP_OK;
}

extern "C" int scorp_mesh_distance_query(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                         const float *queries, int64_t num_queries, double max_distance, double *out_squared_distance,
                                         int32_t *out_face, float *out_closest, void *workspace, size_t workspace_bytes,
                                         scorp_stream_t stream) {
  if (num_queries < 0 || num_queries > kMeshDistMaxQueries) { set_error("mesh_distance_query: num_queries must be in [0, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  if (int e = check_faces(num_faces, "mesh_distance_query", 0)) return e;
  if (!(max_distance >= 0.0)) { set_error("mesh_distance_query: max_distance must not be negative or NaN"); return SCORP_ERR_INVALID; }
  if (num_queries == 0) return SCORP_OK;
  if (!queries || !out_squared_distance || !out_face || !out_closest) { set_error("mesh_distance_query: NULL argument"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  if (num_faces == 0) {   // an empty mesh: every query misses
    mesh_miss_kernel<<<blocks_for(num_queries, kMeshDistThreads), kMeshDistThreads, 0, s>>>(num_queries, out_squared_distance, out_face, out_closest);
    SCORP_KERNEL_CHECK("mesh_miss", 0, s);
    return SCORP_OK;
  }
  if (!vertices || !faces) { set_error("mesh_distance_query: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_mesh_counts(num_vertices, num_faces, "mesh_distance_query")) return e;
  const MeshDistLayout L(num_faces, num_queries);
  if (int e = check_workspace("mesh_distance_query", workspace, workspace_bytes, L.bytes)) return e;
  char *w = (char *)workspace;
  IcpGrid *g = (IcpGrid *)(w + L.grid);
  const uint32_t *order;
  if (int e = icp_sort_source(queries, (int)num_queries, g, (uint32_t *)(w + L.keys0), (uint32_t *)(w + L.vals0), (uint32_t *)(w + L.keys1),
                              (uint32_t *)(w + L.vals1), (uint32_t *)(w + L.hist), L.tiles, s, &order))
    return e;
  const MeshView m{vertices, faces, (int32_t)num_vertices, (int32_t)num_faces};
  const double max_d2 = max_distance * max_distance;
  mesh_query_kernel<<<blocks_for(num_queries, kMeshDistThreads), kMeshDistThreads, 0, s>>>(m, queries, order, num_queries, g, (const uint32_t *)(w + L.cell_start),
                                                                         (const uint32_t *)(w + L.pairs), max_d2, out_squared_distance,
                                                                         out_face, out_closest);
  SCORP_KERNEL_CHECK("mesh_query", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_sample_points(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                        const double *area_prefix, int64_t num_samples, uint64_t seed, float *out_points,
                                        int32_t *out_faces, float *out_barycentric, scorp_stream_t stream) {
  if (num_samples < 0 || num_samples > kMeshDistMaxQueries) { set_error("mesh_sample_points: num_samples must be in [0, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  if (!vertices || !faces || !area_prefix) { set_error("mesh_sample_points: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_mesh_counts(num_vertices, num_faces, "mesh_sample_points")) return e;
  if (num_samples == 0) return SCORP_OK;
  if (!out_points || !out_faces || !out_barycentric) { set_error("mesh_sample_points: NULL argument"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  const MeshView m{vertices, faces, (int32_t)num_vertices, (int32_t)num_faces};
  mesh_sample_kernel<<<blocks_for(num_samples, kMeshDistThreads), kMeshDistThreads, 0, s>>>(m, area_prefix, num_samples, splitmix64(seed), out_points, out_faces,
                                                                          out_barycentric);
  SCORP_KERNEL_CHECK("mesh_sample", 0, s);
  return SCORP_OK;
}

extern "C" size_t scorp_nearest_point_workspace_bytes(int32_t num_points, int32_t num_cloud) {
  return IcpLayout(num_points, num_cloud, 0, 1).total;
}

extern "C" int scorp_nearest_point_distance(const float *points, int32_t num_points, const float *cloud, int32_t num_cloud,
                                            double max_distance, double *out_squared_distance, int32_t *out_index, void *workspace,
                                            size_t workspace_bytes, scorp_stream_t stream) {
  if (num_points < 0) { set_error("nearest_point_distance: num_points < 0"); return SCORP_ERR_INVALID; }
  if (num_cloud < 1 || num_cloud > (1 << 30)) { set_error("nearest_point_distance: num_cloud must be in [1, 2^30]"); return SCORP_ERR_INVALID; }
  if (!(max_distance >= 0.0)) { set_error("nearest_point_distance: max_distance must not be negative or NaN"); return SCORP_ERR_INVALID; }
  if (num_points == 0) return SCORP_OK;
  if (!points || !cloud || !out_squared_distance || !out_index) { set_error("nearest_point_distance: NULL argument"); return SCORP_ERR_INVALID; }
  const IcpLayout L(num_points, num_cloud, 0, 1);
  if (int e = check_workspace("nearest_point_distance", workspace, workspace_bytes, L.total)) return e;
  hipStream_t s = (hipStream_t)stream;
  const IcpWorkspace W(workspace, L);
  const uint32_t *order;
  if (int e = icp_build_target(cloud, num_cloud, L, W, s)) return e;
  if (int e = icp_build_source(points, num_points, L, W, s, &order)) return e;
  const double r2 = max_distance * max_distance;
  const float r2f = (float)r2 * (1.0f + 1e-5f);   // the fp32 search keeps slightly more; the pair test is float64
  nearest_point_kernel<<<blocks_for(num_points, kMeshDistThreads), kMeshDistThreads, 0, s>>>(W.sp, order, num_points, cloud, W.g, W.cell_start, W.tq, r2, r2f,
                                                                           out_squared_distance, out_index);
  SCORP_KERNEL_CHECK("nearest_point", 0, s);
  return SCORP_OK;
}
