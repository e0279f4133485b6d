// marching_cubes.hip — marching cubes on a dense fp32 grid: one vertex per crossed LATTICE EDGE, shared by the up to four cells
// round it, so the mesh arrives indexed and closed and nothing is merged afterwards.  The triangles of a cell come from the
// 256-case table of mc_table.hpp, which scorp_amd/mc_table.py generates from a written rule (the face rule: the crossings of
// a cube face are joined by that face's four signs alone).  The rules - corner and edge numbering, vertex and face order - are
// in include/scorp_gs.h; tests/marching_cubes_reference.py restates them in numpy float64.
//
// Two passes with a scan between them, once for the lattice edges and once for the cells: a count kernel writes one byte per
// lattice point (its crossed edges, as a mask and as a count) / per cell (its 0 .. 5 triangles), the caller forms the inclusive
// prefix sums, and an emit kernel writes at the position the scan gives it.  No atomics: the output order is the ascending
// lattice / cell index, the same on every call.  One lane per lattice point or cell, z fastest.  The table row of a cell is
// ONE 16-byte load from a 4 KB global array (the cases of neighbouring lanes differ: a __constant__ index would serialise);
// the (first corner, axis) of an edge id comes out of packed immediates, never out of a per-lane array.  No LDS, no scratch.
#include "common.hpp"
#include "mc_table.hpp"

namespace scorp {
namespace {

constexpr int kMcThreads = 256;
constexpr uint64_t kMcMaxPoints = (uint64_t)0x7FFFFFFF * kMcThreads;
constexpr uint64_t kMcEdgeCorner = 0x642054103210ull;   // nibble e: the first corner of edge e (its axis is e >> 2)

struct McDims {
  int nx, ny, nz;
  __device__ __forceinline__ size_t lin(int i, int j, int k) const { return ((size_t)i * ny + j) * nz + k; }
};

__global__ void __launch_bounds__(kMcThreads) mc_count_edges_kernel(const float *__restrict__ f, McDims d, uint64_t points, float level,
                                                                    uint8_t *__restrict__ masks, uint8_t *__restrict__ counts) {
  const uint64_t q = (uint64_t)blockIdx.x * kMcThreads + threadIdx.x;
  if (q >= points) return;
  const uint64_t t = q / (uint32_t)d.nz;
  const int k = (int)(q - t * (uint32_t)d.nz);
  const int i = (int)(t / (uint32_t)d.ny);
  const int j = (int)(t - (uint64_t)i * (uint32_t)d.ny);
  const bool in = f[q] < level;
  uint32_t e = 0;
  if (i + 1 < d.nx && (f[q + (size_t)d.ny * d.nz] < level) != in) e |= 1u;
  if (j + 1 < d.ny && (f[q + (size_t)d.nz] < level) != in) e |= 2u;
  if (k + 1 < d.nz && (f[q + 1] < level) != in) e |= 4u;
  masks[q] = (uint8_t)e;
  counts[q] = (uint8_t)__builtin_popcount(e);
}

__global__ void __launch_bounds__(kMcThreads) mc_emit_vertices_kernel(const float *__restrict__ f, const float *__restrict__ x,
                                                                      const float *__restrict__ y, const float *__restrict__ z,
                                                                      McDims d, uint64_t points, float level,
                                                                      const uint8_t *__restrict__ masks,
                                                                      const int32_t *__restrict__ edge_scan, int64_t nv,
                                                                      float *__restrict__ verts) {
#pragma clang fp contract(off)
  const uint64_t q = (uint64_t)blockIdx.x * kMcThreads + threadIdx.x;
  if (q >= points) return;
  const uint32_t e = masks[q] & 7u;
  if (e == 0u) return;
  const uint64_t t = q / (uint32_t)d.nz;
  const int k = (int)(q - t * (uint32_t)d.nz);
  const int i = (int)(t / (uint32_t)d.ny);
  const int j = (int)(t - (uint64_t)i * (uint32_t)d.ny);
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

// the case of cell c: bit n set when corner n = 4 di + 2 dj + dk is inside; (i, j, k) = the cell's first corner
__device__ __forceinline__ uint32_t cell_case(const float *__restrict__ f, const McDims &d, uint64_t c, float level, int &i, int &j,
                                              int &k) {
  const uint64_t t = c / (uint32_t)(d.nz - 1);
  k = (int)(c - t * (uint32_t)(d.nz - 1));
  i = (int)(t / (uint32_t)(d.ny - 1));
  j = (int)(t - (uint64_t)i * (uint32_t)(d.ny - 1));
  uint32_t mask = 0;
#pragma unroll
  for (int n = 0; n < 8; n++) mask |= (f[d.lin(i + (n >> 2), j + ((n >> 1) & 1), k + (n & 1))] < level ? 1u : 0u) << n;
  return mask;
}

__global__ void __launch_bounds__(kMcThreads) mc_count_faces_kernel(const float *__restrict__ f, McDims d, uint64_t cells, float level,
                                                                    uint8_t *__restrict__ counts) {
  const uint64_t c = (uint64_t)blockIdx.x * kMcThreads + threadIdx.x;
  if (c >= cells) return;
  int i, j, k;
  const uint32_t mask = cell_case(f, d, c, level, i, j, k);
  counts[c] = kMcTable[mask * 16 + 15];
}

__global__ void __launch_bounds__(kMcThreads) mc_emit_faces_kernel(const float *__restrict__ f, McDims d, uint64_t cells, float level,
                                                                   const uint8_t *__restrict__ masks,
                                                                   const int32_t *__restrict__ edge_scan,
                                                                   const int32_t *__restrict__ face_scan, int64_t nf,
                                                                   int32_t *__restrict__ faces) {
  const uint64_t c = (uint64_t)blockIdx.x * kMcThreads + threadIdx.x;
  if (c >= cells) return;
  int i, j, k;
  const uint32_t mask = cell_case(f, d, c, level, i, j, k);
  if (mask == 0u || mask == 255u) return;
  const uint4 row = *reinterpret_cast<const uint4 *>(kMcTable + mask * 16);
  const uint32_t w[4] = {row.x, row.y, row.z, row.w};   // (indexed by constants only once the loops are unrolled)
  const int n = (int)(row.w >> 24);
  int64_t r = (int64_t)face_scan[c] - n;
#pragma unroll
  for (int t = 0; t < 5; t++) {
    if (t >= n) break;
    int32_t v[3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const int byte = 3 * t + s;
      const uint32_t e = (w[byte >> 2] >> (8 * (byte & 3))) & 15u;   // (a row holds edge ids below 12 there)
      const uint32_t n0 = (uint32_t)(kMcEdgeCorner >> (4 * e)) & 7u, a = e >> 2;
      const size_t q = d.lin(i + (int)(n0 >> 2), j + (int)((n0 >> 1) & 1u), k + (int)(n0 & 1u));
      const uint32_t m = masks[q];
      v[s] = edge_scan[q] - __builtin_popcount(m & 7u) + __builtin_popcount(m & ((1u << a) - 1u));
    }
    if (r >= 0 && r < nf) {   // (a scan that does not belong to this grid writes nothing out of bounds)
      faces[r * 3 + 0] = v[0];
      faces[r * 3 + 1] = v[1];
      faces[r * 3 + 2] = v[2];
    }
    r++;
  }
}

int check_grid(const float *f, int nx, int ny, int nz, const char *what) {
  if (!f) { set_error("%s: NULL grid", what); return SCORP_ERR_INVALID; }
  if (nx < 2 || ny < 2 || nz < 2) { set_error("%s: every dimension must be at least 2", what); return SCORP_ERR_INVALID; }
  // one lane per lattice point, 2^31 - 1 blocks at the most (the int32 scans hold far fewer crossings than that)
  if ((uint64_t)nx * (uint64_t)ny > kMcMaxPoints / (uint64_t)nz) {
    set_error("%s: more than (2^31 - 1) * %d lattice points", what, kMcThreads); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

inline unsigned mc_blocks(uint64_t n) { return (unsigned)((n + kMcThreads - 1) / kMcThreads); }

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_marching_cubes_count_edges(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_masks,
                                                uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_count_edges")) return e;
  if (!out_masks || !out_counts) { set_error("marching_cubes_count_edges: NULL output"); return SCORP_ERR_INVALID; }
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  mc_count_edges_kernel<<<mc_blocks(points), kMcThreads, 0, (hipStream_t)stream>>>(f, McDims{nx, ny, nz}, points, level, out_masks,
                                                                                   out_counts);
  SCORP_KERNEL_CHECK("mc_count_edges", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_emit_vertices(const float *f, const float *x, const float *y, const float *z, int32_t nx,
                                                  int32_t ny, int32_t nz, float level, const uint8_t *edge_masks,
                                                  const int32_t *edge_scan, int64_t num_vertices, float *out_vertices,
                                                  scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_emit_vertices")) return e;
  if (!x || !y || !z || !edge_masks || !edge_scan || !out_vertices) { set_error("marching_cubes_emit_vertices: NULL argument"); return SCORP_ERR_INVALID; }
  if (num_vertices < 1 || num_vertices > 0x7FFFFFFF) { set_error("marching_cubes_emit_vertices: num_vertices must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  mc_emit_vertices_kernel<<<mc_blocks(points), kMcThreads, 0, (hipStream_t)stream>>>(f, x, y, z, McDims{nx, ny, nz}, points, level,
                                                                                     edge_masks, edge_scan, num_vertices, out_vertices);
  SCORP_KERNEL_CHECK("mc_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_count_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_counts,
                                                scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_count_faces")) return e;
  if (!out_counts) { set_error("marching_cubes_count_faces: NULL out_counts"); return SCORP_ERR_INVALID; }
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  mc_count_faces_kernel<<<mc_blocks(cells), kMcThreads, 0, (hipStream_t)stream>>>(f, McDims{nx, ny, nz}, cells, level, out_counts);
  SCORP_KERNEL_CHECK("mc_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_emit_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level,
                                               const uint8_t *edge_masks, const int32_t *edge_scan, const int32_t *face_scan,
                                               int64_t num_faces, int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "marching_cubes_emit_faces")) return e;
  if (!edge_masks || !edge_scan || !face_scan || !out_faces) { set_error("marching_cubes_emit_faces: NULL argument"); return SCORP_ERR_INVALID; }
  if (num_faces < 1 || num_faces > 0x7FFFFFFF) { set_error("marching_cubes_emit_faces: num_faces must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  mc_emit_faces_kernel<<<mc_blocks(cells), kMcThreads, 0, (hipStream_t)stream>>>(f, McDims{nx, ny, nz}, cells, level, edge_masks,
                                                                                 edge_scan, face_scan, num_faces, out_faces);
  SCORP_KERNEL_CHECK("mc_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
