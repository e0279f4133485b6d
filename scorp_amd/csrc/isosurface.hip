// isosurface.hip — surface extraction from a dense fp32 grid by naive surface nets: one vertex per cell the surface
// crosses, one quad per lattice edge it crosses.  No case tables.  The rules (corner and edge order, quad winding, output
// order) are in include/scorp_gs.h; tests/isosurface_reference.py restates them in numpy float64.
//
// Two passes with a scan between them, once for the cells and once for the lattice edges: a count kernel writes one byte
// per cell (active or not) / per lattice point (its 0..3 quads), the caller forms the inclusive prefix sums, and an emit
// kernel recomputes the verdict and writes at the position the scan gives it.  No atomics: the output order is the
// ascending cell / lattice index, the same on every call.
#include "common.hpp"

namespace scorp {
namespace {

constexpr int kIsoThreads = 256;
constexpr uint64_t kIsoMaxPoints = (uint64_t)0x7FFFFFFF * kIsoThreads;

struct IsoDims {
  int nx, ny, nz;
  __device__ __forceinline__ size_t lin(int i, int j, int k) const { return ((size_t)i * ny + j) * nz + k; }
  __device__ __forceinline__ size_t cell(int i, int j, int k) const { return ((size_t)i * (ny - 1) + j) * (nz - 1) + k; }
};

// the 8 corner values of cell c (corner index 4 di + 2 dj + dk) and the bit mask of the inside ones
__device__ __forceinline__ uint32_t load_cell(const float *__restrict__ f, const IsoDims &d, uint64_t c, float level, float v[8],
                                              int &i, int &j, int &k) {
  const uint64_t t = c / (uint32_t)(d.nz - 1);
  k = (int)(c - t * (uint32_t)(d.nz - 1));
  i = (int)(t / (uint32_t)(d.ny - 1));
  j = (int)(t - (uint64_t)i * (uint32_t)(d.ny - 1));
  uint32_t mask = 0;
#pragma unroll
  for (int n = 0; n < 8; n++) {
    v[n] = f[d.lin(i + (n >> 2), j + ((n >> 1) & 1), k + (n & 1))];
    mask |= (v[n] < level ? 1u : 0u) << n;
  }
  return mask;
}

__global__ void __launch_bounds__(kIsoThreads) iso_count_cells_kernel(const float *__restrict__ f, IsoDims d, uint64_t cells,
                                                                      float level, uint8_t *__restrict__ flags) {
  const uint64_t c = (uint64_t)blockIdx.x * kIsoThreads + threadIdx.x;
  if (c >= cells) return;
  float v[8];
  int i, j, k;
  const uint32_t mask = load_cell(f, d, c, level, v, i, j, k);
  flags[c] = mask != 0u && mask != 255u;
}

__global__ void __launch_bounds__(kIsoThreads) iso_emit_vertices_kernel(const float *__restrict__ f, const float *__restrict__ x,
                                                                        const float *__restrict__ y, const float *__restrict__ z,
                                                                        IsoDims d, uint64_t cells, float level,
                                                                        const int32_t *__restrict__ cell_scan, int64_t nv,
                                                                        float *__restrict__ verts) {
#pragma clang fp contract(off)
  const uint64_t c = (uint64_t)blockIdx.x * kIsoThreads + threadIdx.x;
  if (c >= cells) return;
  float v[8];
  int i, j, k;
  const uint32_t mask = load_cell(f, d, c, level, v, i, j, k);
  if (mask == 0u || mask == 255u) return;
  const int64_t id = (int64_t)cell_scan[c] - 1;
  if (id < 0 || id >= nv) return;   // (a scan that does not belong to this grid writes nothing out of bounds)
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  int n = 0;
#pragma unroll
  for (int axis = 0; axis < 3; axis++) {
    const int step = 4 >> axis;   // corner-index distance along the axis
#pragma unroll
    for (int n0 = 0; n0 < 8; n0++) {
      if (n0 & step) continue;
      const int n1 = n0 + step;
      if (((mask >> n0) & 1u) == ((mask >> n1) & 1u)) continue;
      const float t = (level - v[n0]) / (v[n1] - v[n0]);
      sx += axis == 0 ? t : (float)(n0 >> 2);
      sy += axis == 1 ? t : (float)((n0 >> 1) & 1);
      sz += axis == 2 ? t : (float)(n0 & 1);
      n++;
    }
  }
  const float inv = (float)n;
  const float fx = sx / inv, fy = sy / inv, fz = sz / inv;
  const float x0 = x[i], y0 = y[j], z0 = z[k];
  verts[id * 3 + 0] = x0 + fx * (x[i + 1] - x0);
  verts[id * 3 + 1] = y0 + fy * (y[j + 1] - y0);
  verts[id * 3 + 2] = z0 + fz * (z[k + 1] - z0);
}

// the quads of lattice point q as a 3-bit mask (bit a: the edge q -> q + e_a is crossed and has its four cells); *in = q inside
__device__ __forceinline__ uint32_t point_edges(const float *__restrict__ f, const IsoDims &d, uint64_t q, float level, int &i,
                                                int &j, int &k, bool &in) {
  const uint64_t t = q / (uint32_t)d.nz;
  k = (int)(q - t * (uint32_t)d.nz);
  i = (int)(t / (uint32_t)d.ny);
  j = (int)(t - (uint64_t)i * (uint32_t)d.ny);
  const bool mi = i >= 1 && i <= d.nx - 2, mj = j >= 1 && j <= d.ny - 2, mk = k >= 1 && k <= d.nz - 2;
  in = f[q] < level;
  uint32_t e = 0;
  if (i + 1 < d.nx && mj && mk && (f[d.lin(i + 1, j, k)] < level) != in) e |= 1u;
  if (j + 1 < d.ny && mk && mi && (f[d.lin(i, j + 1, k)] < level) != in) e |= 2u;
  if (k + 1 < d.nz && mi && mj && (f[d.lin(i, j, k + 1)] < level) != in) e |= 4u;
  return e;
}

__global__ void __launch_bounds__(kIsoThreads) iso_count_faces_kernel(const float *__restrict__ f, IsoDims d, uint64_t points,
                                                                      float level, uint8_t *__restrict__ counts) {
  const uint64_t q = (uint64_t)blockIdx.x * kIsoThreads + threadIdx.x;
  if (q >= points) return;
  int i, j, k;
  bool in;
  counts[q] = (uint8_t)__builtin_popcount(point_edges(f, d, q, level, i, j, k, in));
}

__global__ void __launch_bounds__(kIsoThreads) iso_emit_faces_kernel(const float *__restrict__ f, IsoDims d, uint64_t points,
                                                                     float level, const int32_t *__restrict__ cell_scan,
                                                                     const int32_t *__restrict__ edge_scan, int64_t nq,
                                                                     int32_t *__restrict__ faces) {
  const uint64_t q = (uint64_t)blockIdx.x * kIsoThreads + threadIdx.x;
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
    if (r >= 0 && r < nq) {
      int32_t *o = faces + r * 6;
      o[0] = c00; o[1] = in ? c10 : c11; o[2] = in ? c11 : c10;
      o[3] = c00; o[4] = in ? c11 : c01; o[5] = in ? c01 : c11;
    }
    r++;
  }
}

int check_grid(const float *f, int nx, int ny, int nz, const char *what) {
  if (!f) { set_error("%s: NULL grid", what); return SCORP_ERR_INVALID; }
  if (nx < 2 || ny < 2 || nz < 2) { set_error("%s: every dimension must be at least 2", what); return SCORP_ERR_INVALID; }
  // one lane per lattice point, 2^31 - 1 blocks at the most (the int32 scans hold far fewer crossings than that)
  if ((uint64_t)nx * (uint64_t)ny > kIsoMaxPoints / (uint64_t)nz) {
    set_error("%s: more than (2^31 - 1) * %d lattice points", what, kIsoThreads); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

inline unsigned iso_blocks(uint64_t n) { return (unsigned)((n + kIsoThreads - 1) / kIsoThreads); }

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_isosurface_count_cells(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_flags,
                                            scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_count_cells")) return e;
  if (!out_flags) { set_error("isosurface_count_cells: NULL out_flags"); return SCORP_ERR_INVALID; }
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  iso_count_cells_kernel<<<iso_blocks(cells), kIsoThreads, 0, (hipStream_t)stream>>>(f, IsoDims{nx, ny, nz}, cells, level, out_flags);
  SCORP_KERNEL_CHECK("iso_count_cells", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_emit_vertices(const float *f, const float *x, const float *y, const float *z, int32_t nx,
                                              int32_t ny, int32_t nz, float level, const int32_t *cell_scan,
                                              int64_t num_vertices, float *out_vertices, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_emit_vertices")) return e;
  if (!x || !y || !z || !cell_scan || !out_vertices) { set_error("isosurface_emit_vertices: NULL argument"); return SCORP_ERR_INVALID; }
  if (num_vertices < 1 || num_vertices > 0x7FFFFFFF) { set_error("isosurface_emit_vertices: num_vertices must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  const uint64_t cells = (uint64_t)(nx - 1) * (uint64_t)(ny - 1) * (uint64_t)(nz - 1);
  iso_emit_vertices_kernel<<<iso_blocks(cells), kIsoThreads, 0, (hipStream_t)stream>>>(f, x, y, z, IsoDims{nx, ny, nz}, cells, level,
                                                                                       cell_scan, num_vertices, out_vertices);
  SCORP_KERNEL_CHECK("iso_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_count_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_counts,
                                            scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_count_faces")) return e;
  if (!out_counts) { set_error("isosurface_count_faces: NULL out_counts"); return SCORP_ERR_INVALID; }
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  iso_count_faces_kernel<<<iso_blocks(points), kIsoThreads, 0, (hipStream_t)stream>>>(f, IsoDims{nx, ny, nz}, points, level, out_counts);
  SCORP_KERNEL_CHECK("iso_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_emit_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level,
                                           const int32_t *cell_scan, const int32_t *edge_scan, int64_t num_quads,
                                           int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_grid(f, nx, ny, nz, "isosurface_emit_faces")) return e;
  if (!cell_scan || !edge_scan || !out_faces) { set_error("isosurface_emit_faces: NULL argument"); return SCORP_ERR_INVALID; }
  if (num_quads < 1 || num_quads > 0x7FFFFFFF) { set_error("isosurface_emit_faces: num_quads must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  const uint64_t points = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  iso_emit_faces_kernel<<<iso_blocks(points), kIsoThreads, 0, (hipStream_t)stream>>>(f, IsoDims{nx, ny, nz}, points, level, cell_scan,
                                                                                     edge_scan, num_quads, out_faces);
  SCORP_KERNEL_CHECK("iso_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
