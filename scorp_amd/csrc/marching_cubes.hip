// marching_cubes.hip — marching cubes on a dense fp32 grid: one vertex per crossed LATTICE EDGE, shared by the up to four cells
// round it, so the mesh arrives indexed and closed and nothing is merged afterwards.  The triangles of a cell come from the
// 256-case table of mc_table.hpp, which scorp_amd/mc_table.py generates from a written rule (the face rule: the crossings of
// a cube face are joined by that face's four signs alone).  The rules - corner and edge numbering, vertex and face order - are
// in include/scorp_gs.h; tests/marching_cubes_reference.py restates them in numpy float64.
//
// The table row of a cell and the edge ids are read as mc_emit_triangles() of lattice.hpp says; the count / scan / emit scheme
// and the lattice are there too.  One lane per lattice point or cell, z fastest.
#include "lattice.hpp"
#include "mc_table.hpp"

namespace scorp {
namespace {

__global__ void __launch_bounds__(kLatThreads) mc_count_edges_kernel(const float *__restrict__ f, LatticeDims d, uint64_t points, float level,
                                                                    uint8_t *__restrict__ masks, uint8_t *__restrict__ counts) {
  const uint64_t q = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (q >= points) return;
  int i, j, k;
  d.point_ijk(q, i, j, k);
  const bool in = f[q] < level;
  uint32_t e = 0;
  if (i + 1 < d.nx && (f[q + (size_t)d.ny * d.nz] < level) != in) e |= 1u;
  if (j + 1 < d.ny && (f[q + (size_t)d.nz] < level) != in) e |= 2u;
  if (k + 1 < d.nz && (f[q + 1] < level) != in) e |= 4u;
  masks[q] = (uint8_t)e;
  counts[q] = (uint8_t)__builtin_popcount(e);
}

__global__ void __launch_bounds__(kLatThreads) mc_emit_vertices_kernel(const float *__restrict__ f, const float *__restrict__ x,
                                                                      const float *__restrict__ y, const float *__restrict__ z,
                                                                      LatticeDims d, uint64_t points, float level,
                                                                      const uint8_t *__restrict__ masks,
                                                                      const int32_t *__restrict__ edge_scan, int64_t nv,
                                                                      float *__restrict__ verts) {
#pragma clang fp contract(off)
  const uint64_t q = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (q >= points) return;
  const uint32_t e = masks[q] & 7u;
  if (e == 0u) return;
  int i, j, k;
  d.point_ijk(q, i, j, k);
  // (a mask that does not belong to this grid reads nothing out of bounds)
  const uint32_t have = (i + 1 < d.nx ? 1u : 0u) | (j + 1 < d.ny ? 2u : 0u) | (k + 1 < d.nz ? 4u : 0u);
  const float f0 = f[q], x0 = x[i], y0 = y[j], z0 = z[k];
  int64_t id = (int64_t)edge_scan[q] - __builtin_popcount(e);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!((e >> a) & 1u)) continue;
    if (((have >> a) & 1u) && id >= 0 && id < nv) {   // (nor does a foreign scan write out of bounds)
      const float f1 = f[q + (a == 0 ? (size_t)d.ny * d.nz : a == 1 ? (size_t)d.nz : (size_t)1)];
      const float s = (level - f0) / (f1 - f0);
      const float c0 = a == 0 ? x0 : a == 1 ? y0 : z0;
      const float c1 = a == 0 ? x[i + 1] : a == 1 ? y[j + 1] : z[k + 1];
      const float p = c0 + s * (c1 - c0);
      verts[id * 3 + 0] = a == 0 ? p : x0;
      verts[id * 3 + 1] = a == 1 ? p : y0;
      verts[id * 3 + 2] = a == 2 ? p : z0;
    }
    id++;
  }
}

__global__ void __launch_bounds__(kLatThreads) mc_count_faces_kernel(const float *__restrict__ f, LatticeDims d, uint64_t cells, float level,
                                                                    uint8_t *__restrict__ counts) {
  const uint64_t c = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (c >= cells) return;
  float v[8];
  int i, j, k;
  const uint32_t mask = load_cell(f, d, c, level, v, i, j, k);   // (only the case is used: bit n = corner n inside)
  counts[c] = kMcTable[mask * 16 + 15];
}

__global__ void __launch_bounds__(kLatThreads) mc_emit_faces_kernel(const float *__restrict__ f, LatticeDims d, uint64_t cells, float level,
                                                                   const uint8_t *__restrict__ masks,
                                                                   const int32_t *__restrict__ edge_scan,
                                                                   const int32_t *__restrict__ face_scan, int64_t nf,
                                                                   int32_t *__restrict__ faces) {
  const uint64_t c = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (c >= cells) return;
  float v[8];
  int i, j, k;
  const uint32_t mask = load_cell(f, d, c, level, v, i, j, k);   // (only the case is used: bit n = corner n inside)
  if (mask == 0u || mask == 255u) return;
  mc_emit_triangles(kMcTable, mask, masks, edge_scan, face_scan[c], nf, faces,
                    [&](int di, int dj, int dk) { return d.lin(i + di, j + dj, k + dk); });
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_marching_cubes_count_edges(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_masks,
                                                uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_count_edges")) return e;
  if (int e = check_not_null({out_masks, out_counts}, "marching_cubes_count_edges", "output")) return e;
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  mc_count_edges_kernel<<<lattice_blocks(points), kLatThreads, 0, (hipStream_t)stream>>>(f, LatticeDims{nx, ny, nz}, points, level, out_masks,
                                                                                   out_counts);
  SCORP_KERNEL_CHECK("mc_count_edges", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_emit_vertices(const float *f, const float *x, const float *y, const float *z, int32_t nx,
                                                  int32_t ny, int32_t nz, float level, const uint8_t *edge_masks,
                                                  const int32_t *edge_scan, int64_t num_vertices, float *out_vertices,
                                                  scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_emit_vertices")) return e;
  if (int e = check_not_null({x, y, z, edge_masks, edge_scan, out_vertices}, "marching_cubes_emit_vertices", "argument")) return e;
  if (int e = check_count(num_vertices, "marching_cubes_emit_vertices", "num_vertices")) return e;
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  mc_emit_vertices_kernel<<<lattice_blocks(points), kLatThreads, 0, (hipStream_t)stream>>>(f, x, y, z, LatticeDims{nx, ny, nz}, points, level,
                                                                                     edge_masks, edge_scan, num_vertices, out_vertices);
  SCORP_KERNEL_CHECK("mc_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_count_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_counts,
                                                scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_count_faces")) return e;
  if (int e = check_not_null({out_counts}, "marching_cubes_count_faces", "out_counts")) return e;
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  mc_count_faces_kernel<<<lattice_blocks(cells), kLatThreads, 0, (hipStream_t)stream>>>(f, LatticeDims{nx, ny, nz}, cells, level, out_counts);
  SCORP_KERNEL_CHECK("mc_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_emit_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level,
                                               const uint8_t *edge_masks, const int32_t *edge_scan, const int32_t *face_scan,
                                               int64_t num_faces, int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_emit_faces")) return e;
  if (int e = check_not_null({edge_masks, edge_scan, face_scan, out_faces}, "marching_cubes_emit_faces", "argument")) return e;
  if (int e = check_count(num_faces, "marching_cubes_emit_faces", "num_faces")) return e;
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  mc_emit_faces_kernel<<<lattice_blocks(cells), kLatThreads, 0, (hipStream_t)stream>>>(f, LatticeDims{nx, ny, nz}, cells, level, edge_masks,
                                                                                 edge_scan, face_scan, num_faces, out_faces);
  SCORP_KERNEL_CHECK("mc_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
