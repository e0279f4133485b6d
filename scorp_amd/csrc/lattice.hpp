// lattice.hpp — what the four surface extractors (isosurface.hip, isosurface_blocks.hip, marching_cubes.hip,
// marching_cubes_blocks.hip) and the block fusion (tsdf_blocks.hip) share: the dense lattice, the volume of 16^3-voxel
// blocks, the surface-nets crossing mean and quad, the marching-cubes triangle loop, and the hosts' argument checks.  The
// rules themselves - corner and edge numbering, winding, output order, block keys - are in include/scorp_gs.h.
//
// THE SCHEME of all four extractors: two passes with a scan between them, run once for the vertices and once for the faces.
// A count kernel writes one byte per lattice point or cell (surface nets: cell active or not, then the 0 .. 3 quads of a
// point; marching cubes: the crossed edges of a point as a mask and as a count, then the 0 .. 5 triangles of a cell), the
// caller forms the inclusive prefix sums, and an emit kernel recomputes the verdict and writes at the position the scan
// gives it.  No atomics: the output order is the ascending lattice / cell index, the same on every call.  One lane per
// lattice point, cell or voxel.  An emit kernel checks every position a scan gives it against the output's length, so a scan
// that does not belong to its grid or volume writes nothing out of bounds.  No LDS, no scratch.
//
// THE DENSE LATTICE is a [nx, ny, nz] fp32 grid, z fastest; inside is f < level.
//
// THE BLOCK VOLUME (built by tsdf_blocks.hip) is B blocks of 16^3 voxels in ascending key order, [B, 4096] arrays of tsdf and
// weight, and the neighbour table nbr[B, 27] with the rank of every adjacent block, -1 where there is none.  Every fetch
// outside a lane's own block goes through nbr, so a surface runs through block borders without a seam.  The level is 0,
// inside is tsdf < 0.  A voxel that no view has written (w = 0), or whose block does not exist, makes every cell it is a
// corner of INVALID.  One lane per voxel of every block, 16 workgroups per block: the block and its neighbour row are
// workgroup-uniform.
//
// Every function here that does float arithmetic carries `#pragma clang fp contract(off)` itself: the pragma is scoped to a
// function, and the emit kernels' bits must not depend on which of their statements live in this file.
#pragma once
#include <initializer_list>

#include "common.hpp"

namespace scorp {

// ---- the dense lattice ----
constexpr int kLatThreads = 256;
constexpr uint64_t kLatMaxPoints = (uint64_t)0x7FFFFFFF * kLatThreads;

struct LatticeDims {
  int nx, ny, nz;
  __device__ __forceinline__ size_t lin(int i, int j, int k) const { return ((size_t)i * ny + j) * nz + k; }
  __device__ __forceinline__ size_t cell(int i, int j, int k) const { return ((size_t)i * (ny - 1) + j) * (nz - 1) + k; }
  // lin() and cell() taken apart again
  __device__ __forceinline__ void point_ijk(uint64_t q, int &i, int &j, int &k) const { split(q, ny, nz, i, j, k); }
  __device__ __forceinline__ void cell_ijk(uint64_t c, int &i, int &j, int &k) const { split(c, ny - 1, nz - 1, i, j, k); }
  __device__ static __forceinline__ void split(uint64_t q, int my, int mz, int &i, int &j, int &k) {
    const uint64_t t = q / (uint32_t)mz;
    k = (int)(q - t * (uint32_t)mz);
    i = (int)(t / (uint32_t)my);
    j = (int)(t - (uint64_t)i * (uint32_t)my);
  }
};

// the 8 corner values of cell c (corner index 4 di + 2 dj + dk) and the bit mask of the inside ones; (i, j, k) = the
// cell's first corner
__device__ __forceinline__ uint32_t load_cell(const float *__restrict__ f, const LatticeDims &d, uint64_t c, float level, float v[8],
                                              int &i, int &j, int &k) {
  d.cell_ijk(c, i, j, k);
  uint32_t mask = 0;
#pragma unroll
  for (int n = 0; n < 8; n++) {
    v[n] = f[d.lin(i + (n >> 2), j + ((n >> 1) & 1), k + (n & 1))];
    mask |= (v[n] < level ? 1u : 0u) << n;
  }
  return mask;
}

inline int check_grid(const float *f, int nx, int ny, int nz, const char *what) {
  if (!f) { set_error("%s: NULL grid", what); return SCORP_ERR_INVALID; }
  if (nx < 2 || ny < 2 || nz < 2) { set_error("%s: every dimension must be at least 2", what); return SCORP_ERR_INVALID; }
  // one lane per lattice point, 2^31 - 1 blocks at the most (the int32 scans hold far fewer crossings than that)
  if ((uint64_t)nx * (uint64_t)ny > kLatMaxPoints / (uint64_t)nz) {
    set_error("%s: more than (2^31 - 1) * %d lattice points", what, kLatThreads); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

inline unsigned lattice_blocks(uint64_t n) { return (unsigned)((n + kLatThreads - 1) / kLatThreads); }

// ---- the block volume ----
constexpr int kBlkThreads = 256;
constexpr int kBlkSide = 16, kBlkVoxels = 4096;
constexpr int32_t kBlkBias = 1 << 20;               // block coordinates lie in [-2^20, 2^20)
constexpr int64_t kBlkMaxBlocks = 0x7FFFFFFF / 16;  // 16 workgroups per block in the per-voxel launches

__device__ __forceinline__ uint64_t blk_key(int32_t bx, int32_t by, int32_t bz) {
  return (uint64_t)(uint32_t)(bx + kBlkBias) << 42 | (uint64_t)(uint32_t)(by + kBlkBias) << 21 | (uint64_t)(uint32_t)(bz + kBlkBias);
}

__device__ __forceinline__ void blk_coords(uint64_t key, int32_t &bx, int32_t &by, int32_t &bz) {
  bx = (int32_t)((key >> 42) & 0x1FFFFFu) - kBlkBias;
  by = (int32_t)((key >> 21) & 0x1FFFFFu) - kBlkBias;
  bz = (int32_t)(key & 0x1FFFFFu) - kBlkBias;
}

// the global integer coordinates of voxel (lx, ly, lz) of the block with this key
__device__ __forceinline__ void blk_voxel_coords(uint64_t key, int lx, int ly, int lz, int32_t &gx, int32_t &gy, int32_t &gz) {
  int32_t bx, by, bz;
  blk_coords(key, bx, by, bz);
  gx = bx * 16 + lx;
  gy = by * 16 + ly;
  gz = bz * 16 + lz;
}

struct BlockVolume {
  const float *tsdf, *weight;
  const int32_t *nbr;
  int32_t B;
};

// a lane of the per-voxel launches: its block (workgroup-uniform), its voxel l = (lx << 8) | (ly << 4) | lz
struct BlkLane {
  int32_t b;
  int l, lx, ly, lz;
};
__device__ __forceinline__ BlkLane blk_lane() {
  const int32_t b = blockIdx.x >> 4;
  const int l = ((blockIdx.x & 15) << 8) | threadIdx.x;
  return {b, l, l >> 8, (l >> 4) & 15, l & 15};
}

// The voxel at local coordinates (lx, ly, lz), each in -1 .. 16, seen from block b: its index in the [B, 4096] arrays, or -1
// when it lies in a block that does not exist.
__device__ __forceinline__ int64_t locate(const BlockVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int ox = lx < 0 ? 0 : lx > 15 ? 2 : 1, oy = ly < 0 ? 0 : ly > 15 ? 2 : 1, oz = lz < 0 ? 0 : lz > 15 ? 2 : 1;
  const int n = ox * 9 + oy * 3 + oz;
  int32_t r = b;
  if (n != 13) {
    r = vol.nbr[(size_t)b * 27 + n];
    if (r < 0 || r >= vol.B) return -1;   // (a table that does not belong to these blocks reads nothing out of bounds)
  }
  return (int64_t)r * kBlkVoxels + (((lx & 15) << 8) | ((ly & 15) << 4) | (lz & 15));
}

// a lattice point is VALID when its block exists and a view has written it
__device__ __forceinline__ bool point_valid(const BlockVolume &vol, int32_t b, int lx, int ly, int lz) {
  const int64_t i = locate(vol, b, lx, ly, lz);
  return i >= 0 && vol.weight[i] > 0.0f;
}

// the 8 corners of cell (lx, ly, lz) of block b (corner index 4 di + 2 dj + dk): their indices, values, the mask of the
// inside ones; false when a corner is not valid
__device__ __forceinline__ bool load_cell(const BlockVolume &vol, int32_t b, int lx, int ly, int lz, int64_t idx[8], float v[8],
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

inline int check_num_blocks(int64_t num_blocks, const char *what) {
  if (num_blocks < 1 || num_blocks > kBlkMaxBlocks) {
    set_error("%s: num_blocks must be in [1, (2^31 - 1) / 16]", what); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

inline int check_volume(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks, const char *what) {
  if (!tsdf || !weight || !nbr) { set_error("%s: NULL volume", what); return SCORP_ERR_INVALID; }
  return check_num_blocks(num_blocks, what);
}

// ---- surface nets ----
// The crossings of the cell with the corner values v[8] (corner index 4 di + 2 dj + dk) and inside mask `mask`, over its 12
// edges in the fixed order (axis, first corner): their coordinates inside the cell summed into (sx, sy, sz), their number
// returned.  on_crossing(n0, n1, t) is called for each, t = the crossing's place between corners n0 and n1.
template <class OnCrossing>
__device__ __forceinline__ int sum_crossings(uint32_t mask, const float (&v)[8], float level, float &sx, float &sy, float &sz,
                                             OnCrossing &&on_crossing) {
#pragma clang fp contract(off)
  sx = 0.0f; sy = 0.0f; sz = 0.0f;
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
      on_crossing(n0, n1, t);
      n++;
    }
  }
  return n;
}

// The quad round a crossed lattice edge q -> q + e_a, as two triangles at o[0 .. 5]: c00 is the vertex of q's own cell, c10,
// c11, c01 those of the cells one step back along b, along b and c, along c ((b, c) = the two axes after a in cyclic
// order); `in` (q inside) turns the winding, so that the normal points from inside to outside.
__device__ __forceinline__ void write_quad(int32_t *__restrict__ o, bool in, int32_t c00, int32_t c10, int32_t c11, int32_t c01) {
  o[0] = c00; o[1] = in ? c10 : c11; o[2] = in ? c11 : c10;
  o[3] = c00; o[4] = in ? c11 : c01; o[5] = in ? c01 : c11;
}

// ---- marching cubes ----
constexpr uint64_t kMcEdgeCorner = 0x642054103210ull;   // nibble e: the first corner of edge e (its axis is e >> 2)

// The triangles of a cell of case `mask` (neither 0 nor 255), written at faces[3 (face_scan - n) ...] where they lie below nf.
// `table` is kMcTable of mc_table.hpp: the row of a case is ONE 16-byte load from that 4 KB global array (the cases of
// neighbouring lanes differ: a __constant__ index would serialise), and the (first corner, axis) of an edge id comes out of
// the packed immediate, never out of a per-lane array.  A vertex index is that of the lattice edge (cell + corner n0, axis a):
// edge_scan[q] - popc(masks[q]) + popc(masks[q] below bit a).  point(di, dj, dk) gives q, the linear index of the lattice point
// (di, dj, dk) from the cell's first corner; where it may be -1 (locate()) the triangle is dropped and nothing is read there -
// an unsigned index has no -1, and the guard folds away.
template <class Point>
__device__ __forceinline__ void mc_emit_triangles(const uint8_t *__restrict__ table, uint32_t mask, const uint8_t *__restrict__ masks,
                                                  const int32_t *__restrict__ edge_scan, int32_t face_scan, int64_t nf,
                                                  int32_t *__restrict__ faces, Point &&point) {
  const uint4 row = *reinterpret_cast<const uint4 *>(table + mask * 16);
  const uint32_t w[4] = {row.x, row.y, row.z, row.w};   // (indexed by constants only once the loops are unrolled)
  const int n = (int)(row.w >> 24);
  int64_t r = (int64_t)face_scan - n;
#pragma unroll
  for (int t = 0; t < 5; t++) {
    if (t >= n) break;
    int32_t v[3];
    bool ok = true;
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const int byte = 3 * t + s;
      const uint32_t e = (w[byte >> 2] >> (8 * (byte & 3))) & 15u;   // (a row holds edge ids below 12 there)
      const uint32_t n0 = (uint32_t)(kMcEdgeCorner >> (4 * e)) & 7u, a = e >> 2;
      const auto q = point((int)(n0 >> 2), (int)((n0 >> 1) & 1u), (int)(n0 & 1u));
      ok = ok && q >= 0;
      const auto qs = q >= 0 ? q : 0;
      const uint32_t m = masks[qs];
      v[s] = edge_scan[qs] - __builtin_popcount(m & 7u) + __builtin_popcount(m & ((1u << a) - 1u));
    }
    if (ok && r >= 0 && r < nf) {
      faces[r * 3 + 0] = v[0];
      faces[r * 3 + 1] = v[1];
      faces[r * 3 + 2] = v[2];
    }
    r++;
  }
}

// ---- host: the checks every entry point repeats, `what` = its name without the scorp_ prefix ----
inline int check_count(int64_t n, const char *what, const char *name) {
  if (n < 1 || n > 0x7FFFFFFF) { set_error("%s: %s must be in [1, 2^31 - 1]", what, name); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

// "<what>: NULL <name>" when one of the pointers is NULL
inline int check_not_null(std::initializer_list<const void *> pointers, const char *what, const char *name) {
  for (const void *p : pointers)
    if (!p) { set_error("%s: NULL %s", what, name); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

}  // namespace scorp
