// marching_cubes_blocks.hip — marching cubes over a sparse volume of 16^3-voxel blocks: the four kernels of
// marching_cubes.hip - count edges / emit vertices / count faces / emit faces, the caller's scan between each pair - with
// every fetch outside the lane's own block going through locate().  An invalid cell emits no triangle, and a crossed lattice
// edge carries a vertex only when at least one of the four cells round it is valid, so no vertex is left unused at a rim.  An
// edge belongs to the block of its first point q, a cell to the block of its first corner g: vertices come in ascending
// (block rank, local index of q, axis), triangles in ascending (block rank, local cell index, table order).  The rules are in
// include/scorp_gs.h; tests/marching_cubes_reference.py restates them in numpy float64 over a dictionary of blocks.  The
// scheme, the block volume, its validity rule and the triangle loop are in lattice.hpp.
#include "lattice.hpp"
#include "mc_table.hpp"

namespace scorp {
namespace {

// The vertices of lattice point q = (lx, ly, lz) of block b as a 3-bit mask: bit a is set when the edge q -> q + e_a has two
// valid ends that differ in inside-ness and at least one valid cell round it.  The four cells round the edge along a have the
// corners q + {0, 1} e_a + {-1, 0, 1} e_b + {-1, 0, 1} e_c, nine columns of two points; a cell is valid when its four columns
// are.  The crossing is tested first (4 loads), the other 16 points only for a crossed edge.
__device__ __forceinline__ uint32_t point_edges(const BlockVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int64_t q = (int64_t)b * kBlkVoxels + ((lx << 8) | (ly << 4) | lz);
  if (!(vol.weight[q] > 0.0f)) return 0u;
  const bool in = vol.tsdf[q] < 0.0f;
  uint32_t e = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int ax = a == 0, ay = a == 1, az = a == 2;
    const int64_t q1 = locate(vol, b, lx + ax, ly + ay, lz + az);
    if (q1 < 0 || !(vol.weight[q1] > 0.0f) || (vol.tsdf[q1] < 0.0f) == in) continue;
    const int bx = a == 2, by = a == 0, bz = a == 1;   // e_b, e_c: the two axes after a in cyclic order
    const int cx = a == 1, cy = a == 2, cz = a == 0;
    uint32_t col = 0;   // bit (db + 1) 3 + (dc + 1): both points of that column are valid
#pragma unroll
    for (int db = -1; db <= 1; db++)
#pragma unroll
      for (int dc = -1; dc <= 1; dc++) {
        const int px = lx + db * bx + dc * cx, py = ly + db * by + dc * cy, pz = lz + db * bz + dc * cz;
        const bool ok = (db == 0 && dc == 0) || (point_valid(vol, b, px, py, pz) && point_valid(vol, b, px + ax, py + ay, pz + az));
        col |= (ok ? 1u : 0u) << ((db + 1) * 3 + (dc + 1));
      }
    // cells (db, dc) in {-1, 0}^2: columns (db, dc), (db + 1, dc), (db, dc + 1), (db + 1, dc + 1) = bits s, s + 3, s + 1, s + 4
    const uint32_t cells = col & (col >> 1) & (col >> 3) & (col >> 4) & 0x1Bu;
    if (cells) e |= 1u << a;
  }
  return e;
}

__global__ void __launch_bounds__(kBlkThreads) mc_blocks_count_edges_kernel(const BlockVolume vol, uint8_t *__restrict__ masks,
                                                                             uint8_t *__restrict__ counts) {
  const BlkLane t = blk_lane();
  const uint32_t e = point_edges(vol, t.b, t.lx, t.ly, t.lz);
  masks[(size_t)t.b * kBlkVoxels + t.l] = (uint8_t)e;
  counts[(size_t)t.b * kBlkVoxels + t.l] = (uint8_t)__builtin_popcount(e);
}

__global__ void __launch_bounds__(kBlkThreads) mc_blocks_emit_vertices_kernel(const BlockVolume vol, const float *__restrict__ colour,
                                                                               const uint64_t *__restrict__ block_keys,
                                                                               float voxel_length, const uint8_t *__restrict__ masks,
                                                                               const int32_t *__restrict__ edge_scan, int64_t nv,
                                                                               float *__restrict__ verts, float *__restrict__ cols) {
#pragma clang fp contract(off)
  const auto [b, l, lx, ly, lz] = blk_lane();
  const int64_t q = (int64_t)b * kBlkVoxels + l;
  const uint32_t e = masks[q] & 7u;
  if (e == 0u) return;
  const bool with_colour = colour != nullptr && cols != nullptr;   // (uniform: kernel arguments)
  int32_t ix, iy, iz;
  blk_voxel_coords(block_keys[b], lx, ly, lz, ix, iy, iz);
  const float gx = (float)ix + 0.5f, gy = (float)iy + 0.5f, gz = (float)iz + 0.5f;
  const float f0 = vol.tsdf[q];
  int64_t id = (int64_t)edge_scan[q] - __builtin_popcount(e);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!((e >> a) & 1u)) continue;
    const int64_t q1 = locate(vol, b, lx + (a == 0), ly + (a == 1), lz + (a == 2));
    if (q1 >= 0 && id >= 0 && id < nv) {   // (a mask or scan that does not belong to this volume touches nothing out of bounds)
      const float t = (0.0f - f0) / (vol.tsdf[q1] - f0);
      verts[id * 3 + 0] = voxel_length * (a == 0 ? gx + t : gx);
      verts[id * 3 + 1] = voxel_length * (a == 1 ? gy + t : gy);
      verts[id * 3 + 2] = voxel_length * (a == 2 ? gz + t : gz);
      if (with_colour) {
        const float *__restrict__ c0 = colour + q * 3, *__restrict__ c1 = colour + q1 * 3;
        cols[id * 3 + 0] = (c0[0] + t * (c1[0] - c0[0])) / 255.0f;
        cols[id * 3 + 1] = (c0[1] + t * (c1[1] - c0[1])) / 255.0f;
        cols[id * 3 + 2] = (c0[2] + t * (c1[2] - c0[2])) / 255.0f;
      }
    }
    id++;
  }
}

__global__ void __launch_bounds__(kBlkThreads) mc_blocks_count_faces_kernel(const BlockVolume vol, uint8_t *__restrict__ counts) {
  const BlkLane t = blk_lane();
  int64_t idx[8];
  float v[8];
  uint32_t mask;   // (only the case and the verdict are used)
  const bool valid = load_cell(vol, t.b, t.lx, t.ly, t.lz, idx, v, mask);
  counts[(size_t)t.b * kBlkVoxels + t.l] = valid ? kMcTable[mask * 16 + 15] : (uint8_t)0;
}

__global__ void __launch_bounds__(kBlkThreads) mc_blocks_emit_faces_kernel(const BlockVolume vol, const uint8_t *__restrict__ masks,
                                                                            const int32_t *__restrict__ edge_scan,
                                                                            const int32_t *__restrict__ face_scan, int64_t nf,
                                                                            int32_t *__restrict__ faces) {
  const BlkLane t = blk_lane();
  int64_t idx[8];
  float v[8];
  uint32_t mask;
  if (!load_cell(vol, t.b, t.lx, t.ly, t.lz, idx, v, mask) || mask == 0u || mask == 255u) return;
  // (the cell is valid, so the blocks of its corners exist: locate() returns an index)
  mc_emit_triangles(kMcTable, mask, masks, edge_scan, face_scan[(size_t)t.b * kBlkVoxels + t.l], nf, faces,
                    [&](int di, int dj, int dk) { return locate(vol, t.b, t.lx + di, t.ly + dj, t.lz + dk); });
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_marching_cubes_blocks_count_edges(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                       uint8_t *out_masks, uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_count_edges")) return e;
  if (int e = check_not_null({out_masks, out_counts}, "marching_cubes_blocks_count_edges", "output")) return e;
  mc_blocks_count_edges_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_masks, out_counts);
  SCORP_KERNEL_CHECK("mc_blocks_count_edges", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_blocks_emit_vertices(const float *tsdf, const float *weight, const float *colour,
                                                         const uint64_t *block_keys, const int32_t *nbr, int64_t num_blocks,
                                                         float voxel_length, const uint8_t *edge_masks, const int32_t *edge_scan,
                                                         int64_t num_vertices, float *out_vertices, float *out_colours,
                                                         scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_emit_vertices")) return e;
  if (int e = check_not_null({block_keys, edge_masks, edge_scan, out_vertices}, "marching_cubes_blocks_emit_vertices", "argument")) return e;
  if (out_colours && !colour) { set_error("marching_cubes_blocks_emit_vertices: out_colours without colour"); return SCORP_ERR_INVALID; }
  if (!(voxel_length > 0.0f)) { set_error("marching_cubes_blocks_emit_vertices: voxel_length must be positive"); return SCORP_ERR_INVALID; }
  if (int e = check_count(num_vertices, "marching_cubes_blocks_emit_vertices", "num_vertices")) return e;
  mc_blocks_emit_vertices_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_colours ? colour : nullptr, block_keys, voxel_length, edge_masks, edge_scan,
      num_vertices, out_vertices, out_colours);
  SCORP_KERNEL_CHECK("mc_blocks_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_blocks_count_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                       uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_count_faces")) return e;
  if (int e = check_not_null({out_counts}, "marching_cubes_blocks_count_faces", "out_counts")) return e;
  mc_blocks_count_faces_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_counts);
  SCORP_KERNEL_CHECK("mc_blocks_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_blocks_emit_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                      const uint8_t *edge_masks, const int32_t *edge_scan, const int32_t *face_scan,
                                                      int64_t num_faces, int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_emit_faces")) return e;
  if (int e = check_not_null({edge_masks, edge_scan, face_scan, out_faces}, "marching_cubes_blocks_emit_faces", "argument")) return e;
  if (int e = check_count(num_faces, "marching_cubes_blocks_emit_faces", "num_faces")) return e;
  mc_blocks_emit_faces_kernel<<<(unsigned)(num_blocks * 16), kBlkThreads, 0, (hipStream_t)stream>>>(
      BlockVolume{tsdf, weight, nbr, (int32_t)num_blocks}, edge_masks, edge_scan, face_scan, num_faces, out_faces);
  SCORP_KERNEL_CHECK("mc_blocks_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
