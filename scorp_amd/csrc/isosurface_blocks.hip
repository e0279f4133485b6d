// isosurface_blocks.hip — surface nets over a sparse volume of 16^3-voxel blocks (tsdf_blocks.hip): the four kernels of
// isosurface.hip - count cells / emit vertices / count faces / emit faces, the caller's scan between each pair - with the
// corner fetch going through the neighbour table nbr[B, 27], so a cell at a block's border reads its corners from the
// adjacent blocks and the surface runs through block borders without a seam.  The level is 0, inside is tsdf < 0.  A voxel
// that no view has written (w = 0), or whose block does not exist, makes every cell it is a corner of INVALID: no vertex,
// and no quad round an edge one of whose four cells is invalid.  The rules are in include/scorp_gs.h;
// tests/tsdf_blocks_reference.py restates them in numpy float64 over a dictionary of blocks.
//
// One lane per voxel of every block, 16 workgroups per block: the block and its neighbour row are workgroup-uniform.  No
// atomics: vertices come in ascending (block rank, local cell index), quads in ascending (block rank, local index of q,
// axis), the same on every call.  No LDS, no scratch.
#include "common.hpp"

namespace scorp {
namespace {

constexpr int kIsoBlkThreads = 256;
constexpr int kIsoBlkVoxels = 4096;
constexpr int32_t kIsoBlkBias = 1 << 20;
constexpr int64_t kIsoBlkMaxBlocks = 0x7FFFFFFF / 16;

struct BlkVolume {
  const float *tsdf, *weight;
  const int32_t *nbr;
  int32_t B;
};

// The voxel at local coordinates (lx, ly, lz), each in -1 .. 16, seen from block b: its index in the [B, 4096] arrays, or -1
// when it lies in a block that does not exist.
__device__ __forceinline__ int64_t locate(const BlkVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int ox = lx < 0 ? 0 : lx > 15 ? 2 : 1, oy = ly < 0 ? 0 : ly > 15 ? 2 : 1, oz = lz < 0 ? 0 : lz > 15 ? 2 : 1;
  const int n = ox * 9 + oy * 3 + oz;
  int32_t r = b;
  if (n != 13) {
    r = vol.nbr[(size_t)b * 27 + n];
    if (r < 0 || r >= vol.B) return -1;   // (a table that does not belong to these blocks reads nothing out of bounds)
  }
  return (int64_t)r * kIsoBlkVoxels + (((lx & 15) << 8) | ((ly & 15) << 4) | (lz & 15));
}

// a lattice point is VALID when its block exists and a view has written it
__device__ __forceinline__ bool point_valid(const BlkVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int64_t i = locate(vol, b, lx, ly, lz);
  return i >= 0 && vol.weight[i] > 0.0f;
}

// the 8 corners of cell (lx, ly, lz) of block b (corner index 4 di + 2 dj + dk): their indices, values, the mask of the
// inside ones; false when a corner is not valid
__device__ __forceinline__ bool load_cell(const BlkVolume &vol, int32_t b, int lx, int ly, int lz, int64_t idx[8], float v[8],
                                          uint32_t &mask) {
  mask = 0;
  bool valid = true;
#pragma unroll
  for (int n = 0; n < 8; n++) {
    idx[n] = locate(vol, b, lx + (n >> 2), ly + ((n >> 1) & 1), lz + (n & 1));
    const bool ok = idx[n] >= 0 && vol.weight[idx[n] >= 0 ? idx[n] : 0] > 0.0f;
    v[n] = ok ? vol.tsdf[idx[n]] : 0.0f;
    valid = valid && ok;
    mask |= (v[n] < 0.0f ? 1u : 0u) << n;
  }
  return valid;
}

__global__ void __launch_bounds__(kIsoBlkThreads) iso_blocks_count_cells_kernel(const BlkVolume vol, uint8_t *__restrict__ flags) {
  const int32_t b = blockIdx.x >> 4;   // workgroup-uniform
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  int64_t idx[8];
  float v[8];
  uint32_t mask;
  const bool valid = load_cell(vol, b, l >> 8, (l >> 4) & 15, l & 15, idx, v, mask);
  flags[(size_t)b * kIsoBlkVoxels + l] = valid && mask != 0u && mask != 255u;
}

__global__ void __launch_bounds__(kIsoBlkThreads) iso_blocks_emit_vertices_kernel(const BlkVolume vol, const float *__restrict__ colour,
                                                                                  const uint64_t *__restrict__ block_keys,
                                                                                  float voxel_length,
                                                                                  const int32_t *__restrict__ cell_scan, int64_t nv,
                                                                                  float *__restrict__ verts, float *__restrict__ cols) {
#pragma clang fp contract(off)
  const int32_t b = blockIdx.x >> 4;
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
  int64_t idx[8];
  float v[8];
  uint32_t mask;
  const bool valid = load_cell(vol, b, lx, ly, lz, idx, v, mask);
  if (!valid || mask == 0u || mask == 255u) return;
  const int64_t id = (int64_t)cell_scan[(size_t)b * kIsoBlkVoxels + l] - 1;
  if (id < 0 || id >= nv) return;   // (a scan that does not belong to this volume writes nothing out of bounds)
  const bool with_colour = colour != nullptr && cols != nullptr;   // (uniform: kernel arguments)
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
  int n = 0;
#pragma unroll
  for (int axis = 0; axis < 3; axis++) {
    const int step = 4 >> axis;
#pragma unroll
    for (int n0 = 0; n0 < 8; n0++) {
      if (n0 & step) continue;
      const int n1 = n0 + step;
      if (((mask >> n0) & 1u) == ((mask >> n1) & 1u)) continue;
      const float t = (0.0f - v[n0]) / (v[n1] - v[n0]);
      sx += axis == 0 ? t : (float)(n0 >> 2);
      sy += axis == 1 ? t : (float)((n0 >> 1) & 1);
      sz += axis == 2 ? t : (float)(n0 & 1);
      if (with_colour) {
        const float *__restrict__ c0 = colour + idx[n0] * 3, *__restrict__ c1 = colour + idx[n1] * 3;
        cr += c0[0] + t * (c1[0] - c0[0]);
        cg += c0[1] + t * (c1[1] - c0[1]);
        cb += c0[2] + t * (c1[2] - c0[2]);
      }
      n++;
    }
  }
  const float inv = (float)n;
  const uint64_t key = block_keys[b];
  const int32_t gx = ((int32_t)((key >> 42) & 0x1FFFFFu) - kIsoBlkBias) * 16 + lx;
  const int32_t gy = ((int32_t)((key >> 21) & 0x1FFFFFu) - kIsoBlkBias) * 16 + ly;
  const int32_t gz = ((int32_t)(key & 0x1FFFFFu) - kIsoBlkBias) * 16 + lz;
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
__device__ __forceinline__ uint32_t point_edges(const BlkVolume &vol, int32_t b, int lx, int ly, int lz, bool &in) {
  const int64_t q = (int64_t)b * kIsoBlkVoxels + ((lx << 8) | (ly << 4) | lz);
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

__global__ void __launch_bounds__(kIsoBlkThreads) iso_blocks_count_faces_kernel(const BlkVolume vol, uint8_t *__restrict__ counts) {
  const int32_t b = blockIdx.x >> 4;
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  bool in;
  counts[(size_t)b * kIsoBlkVoxels + l] = (uint8_t)__builtin_popcount(point_edges(vol, b, l >> 8, (l >> 4) & 15, l & 15, in));
}

__global__ void __launch_bounds__(kIsoBlkThreads) iso_blocks_emit_faces_kernel(const BlkVolume vol, const int32_t *__restrict__ cell_scan,
                                                                               const int32_t *__restrict__ edge_scan, int64_t nq,
                                                                               int32_t *__restrict__ faces) {
  const int32_t b = blockIdx.x >> 4;
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
  bool in;
  const uint32_t e = point_edges(vol, b, lx, ly, lz, in);
  if (e == 0u) return;
  int64_t r = (int64_t)edge_scan[(size_t)b * kIsoBlkVoxels + l] - __builtin_popcount(e);
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
      int32_t *o = faces + r * 6;
      o[0] = c00; o[1] = in ? c10 : c11; o[2] = in ? c11 : c10;
      o[3] = c00; o[4] = in ? c11 : c01; o[5] = in ? c01 : c11;
    }
    r++;
  }
}

int check_volume(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks, const char *what) {
  if (!tsdf || !weight || !nbr) { set_error("%s: NULL volume", what); return SCORP_ERR_INVALID; }
  if (num_blocks < 1 || num_blocks > kIsoBlkMaxBlocks) {
    set_error("%s: num_blocks must be in [1, (2^31 - 1) / 16]", what); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_isosurface_blocks_count_cells(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                   uint8_t *out_flags, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_count_cells")) return e;
  if (!out_flags) { set_error("isosurface_blocks_count_cells: NULL out_flags"); return SCORP_ERR_INVALID; }
  iso_blocks_count_cells_kernel<<<(unsigned)(num_blocks * 16), kIsoBlkThreads, 0, (hipStream_t)stream>>>(
      BlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_flags);
  SCORP_KERNEL_CHECK("iso_blocks_count_cells", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_blocks_emit_vertices(const float *tsdf, const float *weight, const float *colour,
                                                     const uint64_t *block_keys, const int32_t *nbr, int64_t num_blocks,
                                                     float voxel_length, const int32_t *cell_scan, int64_t num_vertices,
                                                     float *out_vertices, float *out_colours, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_emit_vertices")) return e;
  if (!block_keys || !cell_scan || !out_vertices) { set_error("isosurface_blocks_emit_vertices: NULL argument"); return SCORP_ERR_INVALID; }
  if (out_colours && !colour) { set_error("isosurface_blocks_emit_vertices: out_colours without colour"); return SCORP_ERR_INVALID; }
  if (!(voxel_length > 0.0f)) { set_error("isosurface_blocks_emit_vertices: voxel_length must be positive"); return SCORP_ERR_INVALID; }
  if (num_vertices < 1 || num_vertices > 0x7FFFFFFF) { set_error("isosurface_blocks_emit_vertices: num_vertices must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  iso_blocks_emit_vertices_kernel<<<(unsigned)(num_blocks * 16), kIsoBlkThreads, 0, (hipStream_t)stream>>>(
      BlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_colours ? colour : nullptr, block_keys, voxel_length, cell_scan, num_vertices,
      out_vertices, out_colours);
  SCORP_KERNEL_CHECK("iso_blocks_emit_vertices", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_blocks_count_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                   uint8_t *out_counts, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_count_faces")) return e;
  if (!out_counts) { set_error("isosurface_blocks_count_faces: NULL out_counts"); return SCORP_ERR_INVALID; }
  iso_blocks_count_faces_kernel<<<(unsigned)(num_blocks * 16), kIsoBlkThreads, 0, (hipStream_t)stream>>>(
      BlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, out_counts);
  SCORP_KERNEL_CHECK("iso_blocks_count_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}

extern "C" int scorp_isosurface_blocks_emit_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                                  const int32_t *cell_scan, const int32_t *edge_scan, int64_t num_quads,
                                                  int32_t *out_faces, scorp_stream_t stream) {
  if (int e = check_volume(tsdf, weight, nbr, num_blocks, "isosurface_blocks_emit_faces")) return e;
  if (!cell_scan || !edge_scan || !out_faces) { set_error("isosurface_blocks_emit_faces: NULL argument"); return SCORP_ERR_INVALID; }
  if (num_quads < 1 || num_quads > 0x7FFFFFFF) { set_error("isosurface_blocks_emit_faces: num_quads must be in [1, 2^31 - 1]"); return SCORP_ERR_INVALID; }
  iso_blocks_emit_faces_kernel<<<(unsigned)(num_blocks * 16), kIsoBlkThreads, 0, (hipStream_t)stream>>>(
      BlkVolume{tsdf, weight, nbr, (int32_t)num_blocks}, cell_scan, edge_scan, num_quads, out_faces);
  SCORP_KERNEL_CHECK("iso_blocks_emit_faces", 0, (hipStream_t)stream);
  return SCORP_OK;
}
