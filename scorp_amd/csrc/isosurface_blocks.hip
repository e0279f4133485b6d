// isosurface_blocks.hip — surface nets over a sparse volume of 16^3-voxel blocks: the four kernels of isosurface.hip - count
// cells / emit vertices / count faces / emit faces, the caller's scan between each pair - with the corner fetch going through
// locate(), so a cell at a block's border reads its corners from the adjacent blocks.  An invalid cell carries no vertex, and
// there is no quad round an edge one of whose four cells is invalid.  Vertices come in ascending (block rank, local cell
// index), quads in ascending (block rank, local index of q, axis).  The rules are in include/scorp_gs.h;
// tests/tsdf_blocks_reference.py restates them in numpy float64 over a dictionary of blocks.  The scheme, the block volume and
// its validity rule are in lattice.hpp.
#include "lattice.hpp"

namespace scorp {
namespace {

__global__ void __launch_bounds__(kBlkThreads) iso_blocks_count_cells_kernel(const BlockVolume vol, uint8_t *__restrict__ flags) {
  const BlkLane t = blk_lane();
  int64_t idx[8];
  float v[8];
  uint32_t mask;
  const bool valid = load_cell(vol, t.b, t.lx, t.ly, t.lz, idx, v, mask);
  flags[(size_t)t.b * kBlkVoxels + t.l] = valid && mask != 0u && mask != 255u;
}

__global__ void __launch_bounds__(kBlkThreads) iso_blocks_emit_vertices_kernel(const BlockVolume vol, const float *__restrict__ colour,
                                                                                  const uint64_t *__restrict__ block_keys,
                                                                                  float voxel_length,
                                                                                  const int32_t *__restrict__ cell_scan, int64_t nv,
                                                                                  float *__restrict__ verts, float *__restrict__ cols) {
#pragma clang fp contract(off)
  const auto [b, l, lx, ly, lz] = blk_lane();
  int64_t idx[8];
  float v[8];
  uint32_t mask;
  const bool valid = load_cell(vol, b, lx, ly, lz, idx, v, mask);
  if (!valid || mask == 0u || mask == 255u) return;
  const int64_t id = (int64_t)cell_scan[(size_t)b * kBlkVoxels + l] - 1;
  if (id < 0 || id >= nv) return;   // (a scan that does not belong to this volume writes nothing out of bounds)
  const bool with_colour = colour != nullptr && cols != nullptr;   // (uniform: kernel arguments)
  float sx, sy, sz, cr = 0.0f, cg = 0.0f, cb = 0.0f;
  const int n = sum_crossings(mask, v, 0.0f, sx, sy, sz, [&](int n0, int n1, float t) {
#pragma clang fp contract(off)
    if (with_colour) {
      const float *__restrict__ c0 = colour + idx[n0] * 3, *__restrict__ c1 = colour + idx[n1] * 3;
      cr += c0[0] + t * (c1[0] - c0[0]);
      cg += c0[1] + t * (c1[1] - c0[1]);
      cb += c0[2] + t * (c1[2] - c0[2]);
    }
  });
  const float inv = (float)n;
  int32_t gx, gy, gz;
  blk_voxel_coords(block_keys[b], lx, ly, lz, gx, gy, gz);
  verts[id * 3 + 0] = voxel_length * (((float)gx + 0.5f) + sx / inv);
  verts[id * 3 + 1] = voxel_length * (((float)gy + 0.5f) + sy / inv);
  verts[id * 3 + 2] = voxel_length * (((float)gz + 0.5f) + sz / inv);
  if (with_colour) {
    cols[id * 3 + 0] = cr / inv / 255.0f;
    cols[id * 3 + 1] = cg / inv / 255.0f;
    cols[id * 3 + 2] = cb / inv / 255.0f;
  }
}

// The quads of lattice point q = (lx, ly, lz) of block b as a 3-bit mask (bit a: the edge q -> q + e_a is crossed and its four
// cells are valid); in = q inside.  The four cells round the edge along a have the corners q + {0, 1} e_a + {-1, 0, 1} e_b +
// {-1, 0, 1} e_c: the crossing is tested first (4 loads), the 18 points only for a crossed edge.
__device__ __forceinline__ uint32_t point_edges(const BlockVolume &vol, int32_t b, int lx, int ly, int lz, bool &in) {
  const int64_t q = (int64_t)b * kBlkVoxels + ((lx << 8) | (ly << 4) | lz);
  in = vol.tsdf[q] < 0.0f;
  if (!(vol.weight[q] > 0.0f)) return 0u;
  uint32_t e = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int ax = a == 0, ay = a == 1, az = a == 2;
    const int64_t q1 = locate(vol, b, lx + ax, ly + ay, lz + az);
    if (q1 < 0 || !(vol.weight[q1] > 0.0f) || (vol.tsdf[q1] < 0.0f) == in) continue;
    const int bx = a == 2, by = a == 0, bz = a == 1;   // e_b, e_c: the two axes after a in cyclic order
    const int cx = a == 1, cy = a == 2, cz = a == 0;
    bool ok = true;
    for (int da = 0; da < 2 && ok; da++)
      for (int db = -1; db <= 1 && ok; db++)
        for (int dc = -1; dc <= 1 && ok; dc++)
          ok = point_valid(vol, b, lx + da * ax + db * bx + dc * cx, ly + da * ay + db * by + dc * cy, lz + da * az + db * bz + dc * cz);
    if (ok) e |= 1u << a;
  }
  return e;
}

__global__ void __launch_bounds__(kBlkThreads) iso_blocks_count_faces_kernel(const BlockVolume vol, uint8_t *__restrict__ counts) {
  const BlkLane t = blk_lane();
  bool in;
  counts[(size_t)t.b * kBlkVoxels + t.l] = (uint8_t)__builtin_popcount(point_edges(vol, t.b, t.lx, t.ly, t.lz, in));
}

__global__ void __launch_bounds__(kBlkThreads) iso_blocks_emit_faces_kernel(const BlockVolume vol, const int32_t *__restrict__ cell_scan,
                                                                               const int32_t *__restrict__ edge_scan, int64_t nq,
                                                                               int32_t *__restrict__ faces) {
  const auto [b, l, lx, ly, lz] = blk_lane();
  bool in;
  const uint32_t e = point_edges(vol, b, lx, ly, lz, in);
  if (e == 0u) return;
  int64_t r = (int64_t)edge_scan[(size_t)b * kBlkVoxels + l] - __builtin_popcount(e);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!((e >> a) & 1u)) continue;
    const int bi = a == 2, bj = a == 0, bk = a == 1;
    const int ci = a == 1, cj = a == 2, ck = a == 0;
    // (the four cells are valid, so their blocks exist: locate() returns an index)
    const int64_t i00 = locate(vol, b, lx, ly, lz), i10 = locate(vol, b, lx - bi, ly - bj, lz - bk);
    const int64_t i11 = locate(vol, b, lx - bi - ci, ly - bj - cj, lz - bk - ck), i01 = locate(vol, b, lx - ci, ly - cj, lz - ck);
    if (r >= 0 && r < nq && i00 >= 0 && i10 >= 0 && i11 >= 0 && i01 >= 0) {
      const int32_t c00 = cell_scan[i00] - 1, c10 = cell_scan[i10] - 1, c11 = cell_scan[i11] - 1, c01 = cell_scan[i01] - 1;
      write_quad(faces + r * 6, in, c00, c10, c11, c01);
    }
    r++;
  }
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_isosurface_blocks_count_cells(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                   uint8_t *out_flags, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_count_cells")) return e;
  if (int e = check_not_null({out_flags}, "isosurface_blocks_count_cells", "out_flags")) return e;
  iso_blocks_count_cells_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_flags);
  SCORP_KERNEL_CHECK("iso_blocks_count_cells", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_blocks_emit_vertices(const float *tsdf, const float *weight, const float *colour,
                                                     const uint64_t *block_keys, const int32_t *nbr, int64_t num_blocks,
                                                     float voxel_length, const int32_t *cell_scan, int64_t num_vertices,
                                                     float *out_vertices, float *out_colours, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_emit_vertices")) return e;
  if (int e = check_not_null({block_keys, cell_scan, out_vertices}, "isosurface_blocks_emit_vertices", "argument")) return e;
  if (out_colours && !colour) { set_error("isosurface_blocks_emit_vertices: out_colours without colour"); return SCORP_ERR_INVALID; }
  if (!(voxel_length > 0.0f)) { set_error("isosurface_blocks_emit_vertices: voxel_length must be positive"); return SCORP_ERR_INVALID; }
  if (int e = check_count(num_vertices, "isosurface_blocks_emit_vertices", "num_vertices")) return e;
  iso_blocks_emit_vertices_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_colours ? colour : nullptr, block_keys, voxel_length, cell_scan, num_vertices,
      out_vertices, out_colours);
  SCORP_KERNEL_CHECK("iso_blocks_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_blocks_count_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                   uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_count_faces")) return e;
  if (int e = check_not_null({out_counts}, "isosurface_blocks_count_faces", "out_counts")) return e;
  iso_blocks_count_faces_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_counts);
  SCORP_KERNEL_CHECK("iso_blocks_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_blocks_emit_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                  const int32_t *cell_scan, const int32_t *edge_scan, int64_t num_quads,
                                                  int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_emit_faces")) return e;
  if (int e = check_not_null({cell_scan, edge_scan, out_faces}, "isosurface_blocks_emit_faces", "argument")) return e;
  if (int e = check_count(num_quads, "isosurface_blocks_emit_faces", "num_quads")) return e;
  iso_blocks_emit_faces_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, cell_scan, edge_scan, num_quads, out_faces);
  SCORP_KERNEL_CHECK("iso_blocks_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
