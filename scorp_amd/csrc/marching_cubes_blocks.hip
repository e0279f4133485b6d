// marching_cubes_blocks.hip — marching cubes over a sparse volume of 16^3-voxel blocks (tsdf_blocks.hip): the four kernels of
// marching_cubes.hip - count edges / emit vertices / count faces / emit faces, the caller's scan between each pair - with
// every fetch outside the lane's own block going through the neighbour table nbr[B, 27], so the surface runs through block
// borders without a seam.  The level is 0, inside is tsdf < 0.  A voxel that no view has written (w = 0), or whose block does
// not exist, makes every cell it is a corner of INVALID: such a cell emits no triangle, and a crossed lattice edge carries a
// vertex only when at least one of the four cells round it is valid, so no vertex is left unused at a rim.  The rules are in
// include/scorp_gs.h; tests/marching_cubes_reference.py restates them in numpy float64 over a dictionary of blocks.
//
// One lane per voxel of every block, 16 workgroups per block: the block and its neighbour row are workgroup-uniform.  An edge
// belongs to the block of its first point q, a cell to the block of its first corner g.  No atomics: vertices come in
// ascending (block rank, local index of q, axis), triangles in ascending (block rank, local cell index, table order), the same
// on every call.  The table row is one 16-byte load from the 4 KB global array of mc_table.hpp.  No LDS, no scratch.
#include "common.hpp"
#include "mc_table.hpp"

namespace scorp {
namespace {

constexpr int kMcBlkThreads = 256;
constexpr int kMcBlkVoxels = 4096;
constexpr int32_t kMcBlkBias = 1 << 20;
constexpr int64_t kMcBlkMaxBlocks = 0x7FFFFFFF / 16;
constexpr uint64_t kMcBlkEdgeCorner = 0x642054103210ull;   // nibble e: the first corner of edge e (its axis is e >> 2)

struct McBlkVolume {
  const float *tsdf, *weight;
  const int32_t *nbr;
  int32_t B;
};

// The voxel at local coordinates (lx, ly, lz), each in -1 .. 16, seen from block b: its index in the [B, 4096] arrays, or -1
// when it lies in a block that does not exist.
__device__ __forceinline__ int64_t locate(const McBlkVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int ox = lx < 0 ? 0 : lx > 15 ? 2 : 1, oy = ly < 0 ? 0 : ly > 15 ? 2 : 1, oz = lz < 0 ? 0 : lz > 15 ? 2 : 1;
  const int n = ox * 9 + oy * 3 + oz;
  int32_t r = b;
  if (n != 13) {
    r = vol.nbr[(size_t)b * 27 + n];
    if (r < 0 || r >= vol.B) return -1;   // (a table that does not belong to these blocks reads nothing out of bounds)
  }
  return (int64_t)r * kMcBlkVoxels + (((lx & 15) << 8) | ((ly & 15) << 4) | (lz & 15));
}

// a lattice point is VALID when its block exists and a view has written it
__device__ __forceinline__ bool point_valid(const McBlkVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int64_t i = locate(vol, b, lx, ly, lz);
  return i >= 0 && vol.weight[i] > 0.0f;
}

// The vertices of lattice point q = (lx, ly, lz) of block b as a 3-bit mask: bit a is set when the edge q -> q + e_a has two
// valid ends that differ in inside-ness and at least one valid cell round it.  The four cells round the edge along a have the
// corners q + {0, 1} e_a + {-1, 0, 1} e_b + {-1, 0, 1} e_c, nine columns of two points; a cell is valid when its four columns
// are.  The crossing is tested first (4 loads), the other 16 points only for a crossed edge.
__device__ __forceinline__ uint32_t point_edges(const McBlkVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int64_t q = (int64_t)b * kMcBlkVoxels + ((lx << 8) | (ly << 4) | lz);
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

__global__ void __launch_bounds__(kMcBlkThreads) mc_blocks_count_edges_kernel(const McBlkVolume vol, uint8_t *__restrict__ masks,
                                                                             uint8_t *__restrict__ counts) {
  const int32_t b = blockIdx.x >> 4;   // workgroup-uniform
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  const uint32_t e = point_edges(vol, b, l >> 8, (l >> 4) & 15, l & 15);
  masks[(size_t)b * kMcBlkVoxels + l] = (uint8_t)e;
  counts[(size_t)b * kMcBlkVoxels + l] = (uint8_t)__builtin_popcount(e);
}

__global__ void __launch_bounds__(kMcBlkThreads) mc_blocks_emit_vertices_kernel(const McBlkVolume vol, const float *__restrict__ colour,
                                                                               const uint64_t *__restrict__ block_keys,
                                                                               float voxel_length, const uint8_t *__restrict__ masks,
                                                                               const int32_t *__restrict__ edge_scan, int64_t nv,
                                                                               float *__restrict__ verts, float *__restrict__ cols) {
#pragma clang fp contract(off)
  const int32_t b = blockIdx.x >> 4;
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  const int64_t q = (int64_t)b * kMcBlkVoxels + l;
  const uint32_t e = masks[q] & 7u;
  if (e == 0u) return;
  const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
  const bool with_colour = colour != nullptr && cols != nullptr;   // (uniform: kernel arguments)
  const uint64_t key = block_keys[b];
  const float gx = (float)(((int32_t)((key >> 42) & 0x1FFFFFu) - kMcBlkBias) * 16 + lx) + 0.5f;
  const float gy = (float)(((int32_t)((key >> 21) & 0x1FFFFFu) - kMcBlkBias) * 16 + ly) + 0.5f;
  const float gz = (float)(((int32_t)(key & 0x1FFFFFu) - kMcBlkBias) * 16 + lz) + 0.5f;
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

// the case of cell (lx, ly, lz) of block b (bit n: corner n = 4 di + 2 dj + dk is inside); false when a corner is not valid
__device__ __forceinline__ bool cell_case(const McBlkVolume &vol, int32_t b, int lx, int ly, int lz, uint32_t &mask) {
  mask = 0;
  bool valid = true;
#pragma unroll
  for (int n = 0; n < 8; n++) {
    const int64_t i = locate(vol, b, lx + (n >> 2), ly + ((n >> 1) & 1), lz + (n & 1));
    const bool ok = i >= 0 && vol.weight[i >= 0 ? i : 0] > 0.0f;
    const float v = ok ? vol.tsdf[i] : 0.0f;
    valid = valid && ok;
    mask |= (v < 0.0f ? 1u : 0u) << n;
  }
  return valid;
}

__global__ void __launch_bounds__(kMcBlkThreads) mc_blocks_count_faces_kernel(const McBlkVolume vol, uint8_t *__restrict__ counts) {
  const int32_t b = blockIdx.x >> 4;
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  uint32_t mask;
  const bool valid = cell_case(vol, b, l >> 8, (l >> 4) & 15, l & 15, mask);
  counts[(size_t)b * kMcBlkVoxels + l] = valid ? kMcTable[mask * 16 + 15] : (uint8_t)0;
}

__global__ void __launch_bounds__(kMcBlkThreads) mc_blocks_emit_faces_kernel(const McBlkVolume vol, const uint8_t *__restrict__ masks,
                                                                            const int32_t *__restrict__ edge_scan,
                                                                            const int32_t *__restrict__ face_scan, int64_t nf,
                                                                            int32_t *__restrict__ faces) {
  const int32_t b = blockIdx.x >> 4;
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
  uint32_t mask;
  if (!cell_case(vol, b, lx, ly, lz, mask) || mask == 0u || mask == 255u) return;
  const uint4 row = *reinterpret_cast<const uint4 *>(kMcTable + mask * 16);
  const uint32_t w[4] = {row.x, row.y, row.z, row.w};   // (indexed by constants only once the loops are unrolled)
  const int n = (int)(row.w >> 24);
  int64_t r = (int64_t)face_scan[(size_t)b * kMcBlkVoxels + l] - n;
#pragma unroll
  for (int t = 0; t < 5; t++) {
    if (t >= n) break;
    int32_t v[3];
    bool ok = true;
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const int byte = 3 * t + s;
      const uint32_t e = (w[byte >> 2] >> (8 * (byte & 3))) & 15u;   // (a row holds edge ids below 12 there)
      const uint32_t n0 = (uint32_t)(kMcBlkEdgeCorner >> (4 * e)) & 7u, a = e >> 2;
      // (the cell is valid, so the blocks of its corners exist: locate() returns an index)
      const int64_t q = locate(vol, b, lx + (int)(n0 >> 2), ly + (int)((n0 >> 1) & 1u), lz + (int)(n0 & 1u));
      ok = ok && q >= 0;
      const int64_t qs = q >= 0 ? q : 0;
      const uint32_t m = masks[qs];
      v[s] = edge_scan[qs] - __builtin_popcount(m & 7u) + __builtin_popcount(m & ((1u << a) - 1u));
    }
    if (ok && r >= 0 && r < nf) {   // (a scan that does not belong to this volume writes nothing out of bounds)
      faces[r * 3 + 0] = v[0];
      faces[r * 3 + 1] = v[1];
      faces[r * 3 + 2] = v[2];
    }
    r++;
  }
}

int check_volume(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks, const char *what) {
  if (!tsdf || !weight || !nbr) { set_error("%s: NULL volume", what); return SCORP_ERR_INVALID; }
  if (num_blocks < 1 || num_blocks > kMcBlkMaxBlocks) {
    set_error("%s: num_blocks must be in [1, (2^31 - 1) / 16]", what); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_marching_cubes_blocks_count_edges(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                       uint8_t *out_masks, uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_count_edges")) return e;
  if (!out_masks || !out_counts) { set_error("marching_cubes_blocks_count_edges: NULL output"); return SCORP_ERR_INVALID; }
  mc_blocks_count_edges_kernel<<<(unsigned)(num_blocks * 16), kMcBlkThreads, 0, (hipStream_t)stream>>>(
      McBlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_masks, out_counts);
  SCORP_KERNEL_CHECK("mc_blocks_count_edges", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_blocks_emit_vertices(const float *tsdf, const float *weight, const float *colour,
                                                         const uint64_t *block_keys, const int32_t *nbr, int64_t num_blocks,
                                                         float voxel_length, const uint8_t *edge_masks, const int32_t *edge_scan,
                                                         int64_t num_vertices, float *out_vertices, float *out_colours,
                                                         scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_emit_vertices")) return e;
  if (!block_keys || !edge_masks || !edge_scan || !out_vertices) { set_error("marching_cubes_blocks_emit_vertices: NULL argument"); return SCORP_ERR_INVALID; }
  if (out_colours && !colour) { set_error("marching_cubes_blocks_emit_vertices: out_colours without colour"); return SCORP_ERR_INVALID; }
  if (!(voxel_length > 0.0f)) { set_error("marching_cubes_blocks_emit_vertices: voxel_length must be positive"); return SCORP_ERR_INVALID; }
  if (num_vertices < 1 || num_vertices > 0x7FFFFFFF) { set_error("marching_cubes_blocks_emit_vertices: num_vertices must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  mc_blocks_emit_vertices_kernel<<<(unsigned)(num_blocks * 16), kMcBlkThreads, 0, (hipStream_t)stream>>>(
      McBlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_colours ? colour : nullptr, block_keys, voxel_length, edge_masks, edge_scan,
      num_vertices, out_vertices, out_colours);
  SCORP_KERNEL_CHECK("mc_blocks_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_blocks_count_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                       uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_count_faces")) return e;
  if (!out_counts) { set_error("marching_cubes_blocks_count_faces: NULL out_counts"); return SCORP_ERR_INVALID; }
  mc_blocks_count_faces_kernel<<<(unsigned)(num_blocks * 16), kMcBlkThreads, 0, (hipStream_t)stream>>>(
      McBlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_counts);
  SCORP_KERNEL_CHECK("mc_blocks_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_marching_cubes_blocks_emit_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                      const uint8_t *edge_masks, const int32_t *edge_scan, const int32_t *face_scan,
                                                      int64_t num_faces, int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "marching_cubes_blocks_emit_faces")) return e;
  if (!edge_masks || !edge_scan || !face_scan || !out_faces) { set_error("marching_cubes_blocks_emit_faces: NULL argument"); return SCORP_ERR_INVALID; }
  if (num_faces < 1 || num_faces > 0x7FFFFFFF) { set_error("marching_cubes_blocks_emit_faces: num_faces must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  mc_blocks_emit_faces_kernel<<<(unsigned)(num_blocks * 16), kMcBlkThreads, 0, (hipStream_t)stream>>>(
      McBlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, edge_masks, edge_scan, face_scan, num_faces, out_faces);
  SCORP_KERNEL_CHECK("mc_blocks_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
