// isosurface.hip — surface extraction from a dense fp32 grid by naive surface nets: one vertex per cell the surface
// crosses, one quad per lattice edge it crosses.  No case tables.  The rules (corner and edge order, quad winding, output
// order) are in include/scorp_gs.h; tests/isosurface_reference.py restates them in numpy float64.  The count / scan / emit
// scheme and the lattice are in lattice.hpp.
#include "lattice.hpp"

namespace scorp {
namespace {

__global__ void __launch_bounds__(kLatThreads) iso_count_cells_kernel(const float *__restrict__ f, LatticeDims d, uint64_t cells,
                                                                      float level, uint8_t *__restrict__ flags) {
  const uint64_t c = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (c >= cells) return;
  float v[8];
  int i, j, k;
  const uint32_t mask = load_cell(f, d, c, level, v, i, j, k);
  flags[c] = mask != 0u && mask != 255u;
}

__global__ void __launch_bounds__(kLatThreads) iso_emit_vertices_kernel(const float *__restrict__ f, const float *__restrict__ x,
                                                                        const float *__restrict__ y, const float *__restrict__ z,
                                                                        LatticeDims d, uint64_t cells, float level,
                                                                        const int32_t *__restrict__ cell_scan, int64_t nv,
                                                                        float *__restrict__ verts) {
#pragma clang fp contract(off)
  const uint64_t c = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (c >= cells) return;
  float v[8];
  int i, j, k;
  const uint32_t mask = load_cell(f, d, c, level, v, i, j, k);
  if (mask == 0u || mask == 255u) return;
  const int64_t id = (int64_t)cell_scan[c] - 1;
  if (id < 0 || id >= nv) return;   // (a scan that does not belong to this grid writes nothing out of bounds)
  float sx, sy, sz;
  const int n = sum_crossings(mask, v, level, sx, sy, sz, [](int, int, float) {});
  const float inv = (float)n;
  const float fx = sx / inv, fy = sy / inv, fz = sz / inv;
  const float x0 = x[i], y0 = y[j], z0 = z[k];
  verts[id * 3 + 0] = x0 + fx * (x[i + 1] - x0);
  verts[id * 3 + 1] = y0 + fy * (y[j + 1] - y0);
  verts[id * 3 + 2] = z0 + fz * (z[k + 1] - z0);
}

// the quads of lattice point q as a 3-bit mask (bit a: the edge q -> q + e_a is crossed and has its four cells); *in = q inside
__device__ __forceinline__ uint32_t point_edges(const float *__restrict__ f, const LatticeDims &d, uint64_t q, float level, int &i,
                                                int &j, int &k, bool &in) {
  d.point_ijk(q, i, j, k);
  const bool mi = i >= 1 && i <= d.nx - 2, mj = j >= 1 && j <= d.ny - 2, mk = k >= 1 && k <= d.nz - 2;
  in = f[q] < level;
  uint32_t e = 0;
  if (i + 1 < d.nx && mj && mk && (f[d.lin(i + 1, j, k)] < level) != in) e |= 1u;
  if (j + 1 < d.ny && mk && mi && (f[d.lin(i, j + 1, k)] < level) != in) e |= 2u;
  if (k + 1 < d.nz && mi && mj && (f[d.lin(i, j, k + 1)] < level) != in) e |= 4u;
  return e;
}

__global__ void __launch_bounds__(kLatThreads) iso_count_faces_kernel(const float *__restrict__ f, LatticeDims d, uint64_t points,
                                                                      float level, uint8_t *__restrict__ counts) {
  const uint64_t q = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (q >= points) return;
  int i, j, k;
  bool in;
  counts[q] = (uint8_t)__builtin_popcount(point_edges(f, d, q, level, i, j, k, in));
}

__global__ void __launch_bounds__(kLatThreads) iso_emit_faces_kernel(const float *__restrict__ f, LatticeDims d, uint64_t points,
                                                                     float level, const int32_t *__restrict__ cell_scan,
                                                                     const int32_t *__restrict__ edge_scan, int64_t nq,
                                                                     int32_t *__restrict__ faces) {
  const uint64_t q = (uint64_t)blockIdx.x * kLatThreads + threadIdx.x;
  if (q >= points) return;
  int i, j, k;
  bool in;
  const uint32_t e = point_edges(f, d, q, level, i, j, k, in);
  if (e == 0u) return;
  int64_t r = (int64_t)edge_scan[q] - __builtin_popcount(e);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!((e >> a) & 1u)) continue;
    // (b, c) = the two axes after a in cyclic order; the cells round the edge step back along them
    const int bi = a == 2, bj = a == 0, bk = a == 1;
    const int ci = a == 1, cj = a == 2, ck = a == 0;
    const int32_t c00 = cell_scan[d.cell(i, j, k)] - 1;
    const int32_t c10 = cell_scan[d.cell(i - bi, j - bj, k - bk)] - 1;
    const int32_t c11 = cell_scan[d.cell(i - bi - ci, j - bj - cj, k - bk - ck)] - 1;
    const int32_t c01 = cell_scan[d.cell(i - ci, j - cj, k - ck)] - 1;
    if (r >= 0 && r < nq) write_quad(faces + r * 6, in, c00, c10, c11, c01);
    r++;
  }
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_isosurface_count_cells(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_flags,
                                            scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_count_cells")) return e;
  if (int e = check_not_null({out_flags}, "isosurface_count_cells", "out_flags")) return e;
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  iso_count_cells_kernel<<<lattice_blocks(cells), kLatThreads, 0, (hipStream_t)stream>>>(f, LatticeDims{nx, ny, nz}, cells, level, out_flags);
  SCORP_KERNEL_CHECK("iso_count_cells", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_emit_vertices(const float *f, const float *x, const float *y, const float *z, int32_t nx,
                                              int32_t ny, int32_t nz, float level, const int32_t *cell_scan,
                                              int64_t num_vertices, float *out_vertices, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_emit_vertices")) return e;
  if (int e = check_not_null({x, y, z, cell_scan, out_vertices}, "isosurface_emit_vertices", "argument")) return e;
  if (int e = check_count(num_vertices, "isosurface_emit_vertices", "num_vertices")) return e;
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  iso_emit_vertices_kernel<<<lattice_blocks(cells), kLatThreads, 0, (hipStream_t)stream>>>(f, x, y, z, LatticeDims{nx, ny, nz}, cells, level,
                                                                                       cell_scan, num_vertices, out_vertices);
  SCORP_KERNEL_CHECK("iso_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_count_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_counts,
                                            scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_count_faces")) return e;
  if (int e = check_not_null({out_counts}, "isosurface_count_faces", "out_counts")) return e;
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  iso_count_faces_kernel<<<lattice_blocks(points), kLatThreads, 0, (hipStream_t)stream>>>(f, LatticeDims{nx, ny, nz}, points, level, out_counts);
  SCORP_KERNEL_CHECK("iso_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_emit_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level,
                                           const int32_t *cell_scan, const int32_t *edge_scan, int64_t num_quads,
                                           int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_emit_faces")) return e;
  if (int e = check_not_null({cell_scan, edge_scan, out_faces}, "isosurface_emit_faces", "argument")) return e;
  if (int e = check_count(num_quads, "isosurface_emit_faces", "num_quads")) return e;
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  iso_emit_faces_kernel<<<lattice_blocks(points), kLatThreads, 0, (hipStream_t)stream>>>(f, LatticeDims{nx, ny, nz}, points, level, cell_scan,
                                                                                     edge_scan, num_quads, out_faces);
  SCORP_KERNEL_CHECK("iso_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
