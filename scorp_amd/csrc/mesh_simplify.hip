// mesh_simplify.hip — mesh simplification by vertex clustering: the vertices that fall into one cell of a regular grid
// become one vertex (their mean, or the minimiser of the cell's accumulated plane quadrics), the faces are mapped through
// the cells, and the faces that collapse or repeat are dropped.  The rules (cells, numbering, placement, faces) are in
// include/scorp_gs.h; tests/mesh_simplify_reference.py restates them in plain Python over a dictionary of cells.
//
// Five calls with the caller's scans between them, as in mesh_cluster.hip:
//   cells       fills the cell table itself, then every vertex inserts its 63-bit cell key.  A slot is claimed by ONE 64-bit
//               compare-and-swap on the key and the vertex takes atomicMin(&owner[slot], v): when the launch has ended the
//               owner of a slot is the smallest vertex index of its cell, whatever order the lanes ran in.
//   roots       rep[v] = owner[slot[v]] and one byte rep[v] == v; the inclusive scan of the bytes numbers the cells.
//   accumulate  vertex_cell[v] = scan[rep[v]] - 1; every vertex adds its position, colour and 1 to its cell, and - with the
//               quadric placement - every triangle of non-zero area adds a n n^T and a d n to the cell of each corner, the
//               lanes of a wave that hold the same cell combined first.  float64 atomic adds: the sums depend on the order
//               of arrival in their last bits.
//   place       one thread per cell: means, and the truncated solve of the 3x3 quadric through svd3.hpp.
//   faces       remap, rotate the smallest cell first, and a second open-addressing table of FACE INDICES whose key is the
//               ordered triple of the face stored in the slot: equal triples meet in one slot and atomicMin leaves the
//               smallest face index there, so keep[t] does not depend on the execution order either.
// Nothing waits on another lane's progress: no locks, no spinning on a value someone else must write.  The cell table's
// claim, the face load and cross product, the wave loop of the quadrics and the host checks are mesh_common.hpp's.
#include "mesh_common.hpp"
#include "svd3.hpp"

namespace scorp {
namespace {

constexpr int kSimplifyThreads = 256;
constexpr int32_t kCellSide = 1 << 21;          // cell indices per axis
constexpr int kAcc = 16;                        // doubles per cell: position 3, colour 3, count, A 6 (xx xy xz yy yz zz), b 3

// The grid: origin = double(min_bound) - 0.5 h per axis; cell index floor((double(x) - origin) / h), one subtraction and one
// division, each rounded on its own.
struct Grid {
  double o[3], h;
};

__device__ __forceinline__ Grid load_grid(const float *__restrict__ min_bound, double h) {
#pragma clang fp contract(off)
  Grid g;
  g.h = h;
  const double half = 0.5 * h;
  for (int k = 0; k < 3; k++) g.o[k] = (double)min_bound[k] - half;
  return g;
}

// false when an index falls outside [0, 2^21) (or the coordinate is not finite); cell[] is then clamped into the range
__device__ __forceinline__ bool cell_of(const Grid &g, const float *__restrict__ p, int32_t cell[3]) {
#pragma clang fp contract(off)
  bool ok = true;
  for (int k = 0; k < 3; k++) {
    const double q = floor(((double)p[k] - g.o[k]) / g.h);
    const bool in = q >= 0.0 && q < (double)kCellSide;   // (false for NaN)
    ok = ok && in;
    cell[k] = in ? (int32_t)q : 0;
  }
  return ok;
}

__device__ __forceinline__ double cell_centre(const Grid &g, int32_t i, int k) {
#pragma clang fp contract(off)
  return g.o[k] + ((double)i + 0.5) * g.h;
}

__global__ void __launch_bounds__(kSimplifyThreads) simplify_init_kernel(uint64_t *__restrict__ keys, int32_t *__restrict__ owner,
                                                                         uint64_t slots, int32_t *__restrict__ overflow) {
  const uint64_t i = (uint64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (i < slots) {
    keys[i] = kEmptyKey;
    owner[i] = kEmptyOwner;
  }
  if (i == 0) *overflow = 0;
}

__global__ void __launch_bounds__(kSimplifyThreads) simplify_cells_kernel(const float *__restrict__ verts, int32_t num_vertices,
                                                                          const float *__restrict__ min_bound, double h, uint64_t *keys,
                                                                          int32_t *owner, uint64_t slot_mask, int32_t *__restrict__ out_slot,
                                                                          int32_t *overflow) {
  const int64_t v64 = (int64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (v64 >= num_vertices) return;
  const int32_t v = (int32_t)v64;
  const Grid g = load_grid(min_bound, h);
  const float p[3] = {verts[3 * v64], verts[3 * v64 + 1], verts[3 * v64 + 2]};
  int32_t c[3];
  int32_t found = -1;
  if (!cell_of(g, p, c)) {
    atomicOr(overflow, 1);
  } else {
    const uint64_t key = (uint64_t)c[0] << 42 | (uint64_t)c[1] << 21 | (uint64_t)c[2];
    // (with num_slots >= 2 num_vertices at most half the slots are ever taken)
    const int64_t slot = table_claim(keys, slot_mask, key);
    if (slot != kTableFull) {
      atomicMin(owner + slot, v);
      found = (int32_t)slot;
    }
  }
  out_slot[v64] = found;
}

// (after the cells launch has ended: plain loads)
__global__ void __launch_bounds__(kSimplifyThreads) simplify_roots_kernel(const int32_t *__restrict__ owner, uint64_t slots,
                                                                          const int32_t *__restrict__ slot, int32_t num_vertices,
                                                                          int32_t *__restrict__ out_rep, uint8_t *__restrict__ out_is_root) {
  const int64_t v = (int64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (v >= num_vertices) return;
  const int32_t s = slot[v];
  int32_t r = (int32_t)v;   // a vertex the cells call could not place (overflow), or a slot array that is not its: a cell of its own
  if (s >= 0 && (uint64_t)s < slots) {
    const int32_t o = owner[s];
    if (o >= 0 && o < (int32_t)v) r = o;
  }
  out_rep[v] = r;
  out_is_root[v] = r == (int32_t)v;
}

// scan[rep[v]] - 1, or -1 when the arrays do not belong together (nothing is then added out of bounds)
__device__ __forceinline__ int32_t cell_number(const int32_t *__restrict__ rep, const int32_t *__restrict__ rep_scan, int64_t v,
                                               int32_t num_vertices, int32_t cells) {
  const int32_t r = rep[v];
  if (r < 0 || r >= num_vertices) return -1;
  const int32_t c = rep_scan[r] - 1;
  return c >= 0 && c < cells ? c : -1;
}

__global__ void __launch_bounds__(kSimplifyThreads) simplify_vertex_sums_kernel(const float *__restrict__ verts, const float *__restrict__ colors,
                                                                                int32_t num_vertices, const float *__restrict__ min_bound,
                                                                                double h, const int32_t *__restrict__ rep,
                                                                                const int32_t *__restrict__ rep_scan, int32_t cells,
                                                                                int32_t *__restrict__ out_vertex_cell,
                                                                                int32_t *__restrict__ out_cell_ijk, double *acc) {
  const int64_t v = (int64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (v >= num_vertices) return;
  const int32_t c = cell_number(rep, rep_scan, v, num_vertices, cells);
  out_vertex_cell[v] = c;
  if (c < 0) return;
  const float p[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
  if (rep[v] == (int32_t)v) {   // the cell's first vertex records where the cell is
    const Grid g = load_grid(min_bound, h);
    int32_t ijk[3];
    cell_of(g, p, ijk);
    for (int k = 0; k < 3; k++) out_cell_ijk[3 * (int64_t)c + k] = ijk[k];
  }
  double *a = acc + (int64_t)c * kAcc;
  for (int k = 0; k < 3; k++) {
    unsafeAtomicAdd(a + k, (double)p[k]);
    unsafeAtomicAdd(a + 3 + k, (double)colors[3 * v + k]);
  }
  unsafeAtomicAdd(a + 6, 1.0);
}

// Every triangle of non-zero area adds a n n^T and a d n to the cell of each corner.  Surface extraction emits triangles in
// lattice order, so the lanes of a wave share few cells: the lanes that hold the same cell combine first and the wave issues
// one atomic per distinct cell, corner and term instead of one per lane (measured against the per-lane form on the meshes of
// scripts/time_mesh_simplify.py: 1.4x faster at cells of 2 voxels, 2.4x at 4, 3.7x at 8).
__global__ void __launch_bounds__(kSimplifyThreads) simplify_quadrics_kernel(const int32_t *__restrict__ tri_idx, int32_t faces,
                                                                             const float *__restrict__ verts, int32_t num_vertices,
                                                                             const float *__restrict__ min_bound, double h,
                                                                             const int32_t *__restrict__ rep, const int32_t *__restrict__ rep_scan,
                                                                             int32_t cells, double *acc) {
#pragma clang fp contract(off)   // every product and sum rounded on its own, as the float64 restatements round
  const int64_t t = (int64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  Face f = {0, 0, 0, false};
  if (t < faces) f = load_face(tri_idx, t, num_vertices);
  bool live = f.ok;
  const int32_t idx[3] = {f.a, f.b, f.c};
  float p[3][3] = {};
  double n[3] = {0.0, 0.0, 0.0}, area = 0.0;
  if (live) {
    for (int k = 0; k < 3; k++)
      for (int d = 0; d < 3; d++) p[k][d] = verts[3 * (int64_t)idx[k] + d];
    const Vec3d N = face_cross(verts, f);
    const double len = norm3(N);
    live = len > 0.0;
    if (live) {
      area = 0.5 * len;
      n[0] = N.x / len; n[1] = N.y / len; n[2] = N.z / len;
    }
  }
  const double an[3] = {area * n[0], area * n[1], area * n[2]};
  const Grid g = load_grid(min_bound, h);
  for (int k = 0; k < 3; k++) {
    int32_t c = -1;
    double term[9] = {};
    if (live) c = cell_number(rep, rep_scan, idx[k], num_vertices, cells);
    if (c >= 0) {
      int32_t ijk[3];
      cell_of(g, p[k], ijk);
      const double d = -((n[0] * ((double)p[0][0] - cell_centre(g, ijk[0], 0)) + n[1] * ((double)p[0][1] - cell_centre(g, ijk[1], 1))) +
                         n[2] * ((double)p[0][2] - cell_centre(g, ijk[2], 2)));
      const double ad = area * d;
      term[0] = an[0] * n[0]; term[1] = an[0] * n[1]; term[2] = an[0] * n[2];
      term[3] = an[1] * n[1]; term[4] = an[1] * n[2]; term[5] = an[2] * n[2];
      term[6] = ad * n[0]; term[7] = ad * n[1]; term[8] = ad * n[2];
    }
    wave_combine_equal(c, [&](int32_t lc, bool mine, int count, bool leads) {
      const bool alone = count == 1;   // (uniform: the butterfly is skipped for a cell only one lane holds)
      double *a = acc + (int64_t)lc * kAcc + 7;
#pragma unroll
      for (int j = 0; j < 9; j++) {
        const double s = alone ? term[j] : wave_sum_f64(mine ? term[j] : 0.0);
        if (leads) unsafeAtomicAdd(a + j, s);
      }
    });
  }
}

__global__ void __launch_bounds__(kSimplifyThreads) simplify_place_kernel(const double *__restrict__ acc, const int32_t *__restrict__ cell_ijk,
                                                                          int32_t cells, const float *__restrict__ min_bound, double h,
                                                                          int quadric, float *__restrict__ out_verts,
                                                                          float *__restrict__ out_colors) {
#pragma clang fp contract(off)
  const int64_t c = (int64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (c >= cells) return;
  const double *a = acc + c * kAcc;
  const double count = a[6];
  double mean[3];
  for (int k = 0; k < 3; k++) {
    mean[k] = a[k] / count;
    out_colors[3 * c + k] = (float)(a[3 + k] / count);
  }
  float out[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  if (quadric && count > 1.0) {   // (a single member lies on every plane of its cell: it is the minimiser, bit for bit)
    const Grid g = load_grid(min_bound, h);
    const double A[3][3] = {{a[7], a[8], a[9]}, {a[8], a[10], a[11]}, {a[9], a[11], a[12]}};
    double pc[3], m[3], r[3];
    for (int k = 0; k < 3; k++) {
      pc[k] = cell_centre(g, cell_ijk[3 * c + k], k);
      m[k] = mean[k] - pc[k];
    }
    for (int k = 0; k < 3; k++) r[k] = -a[13 + k] - ((A[k][0] * m[0] + A[k][1] * m[1]) + A[k][2] * m[2]);
    // A is symmetric and positive semi-definite: its singular values are its eigenvalues and the columns of V its
    // eigenvectors, sorted descending; sigma_i = |A v_i|
    double U[3][3], V[3][3], sigma[3];
    svd3(A, U, V);
    for (int i = 0; i < 3; i++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) {
        const double w = (A[k][0] * V[0][i] + A[k][1] * V[1][i]) + A[k][2] * V[2][i];
        s += w * w;
      }
      sigma[i] = sqrt(s);
    }
    if (sigma[0] > 0.0) {
      double x[3] = {m[0], m[1], m[2]};
      for (int i = 0; i < 3; i++) {
        if (!(sigma[i] > 1e-3 * sigma[0])) continue;
        const double w = ((V[0][i] * r[0] + V[1][i] * r[1]) + V[2][i] * r[2]) / sigma[i];
        for (int k = 0; k < 3; k++) x[k] += V[k][i] * w;
      }
      if (fabs(x[0]) <= h && fabs(x[1]) <= h && fabs(x[2]) <= h)   // (false for NaN: the mean stands in)
        for (int k = 0; k < 3; k++) out[k] = (float)(pc[k] + x[k]);
    }
  }
  for (int k = 0; k < 3; k++) out_verts[3 * c + k] = out[k];
}

// ---- faces ----

__device__ __forceinline__ uint64_t triple_hash(int32_t a, int32_t b, int32_t c) {
  return mix64(mix64((uint64_t)(uint32_t)a << 32 | (uint32_t)b) ^ (uint64_t)(uint32_t)c);
}

// fills the table, maps every face through vertex_cell and rotates the smallest cell to the front; a face with two equal
// cells (or an index out of range) gets the triple (-1, -1, -1) and keep = 0
__global__ void __launch_bounds__(kSimplifyThreads) simplify_faces_remap_kernel(const int32_t *__restrict__ tri_idx, int32_t faces,
                                                                                const int32_t *__restrict__ vertex_cell, int32_t num_vertices,
                                                                                int32_t *__restrict__ table, uint64_t slots,
                                                                                int32_t *__restrict__ out_faces, uint8_t *__restrict__ out_keep) {
  const uint64_t i = (uint64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (i < slots) table[i] = kEmptyOwner;
  if (i >= (uint64_t)faces) return;
  int32_t c[3] = {-1, -1, -1};
  bool ok = true;
  for (int k = 0; k < 3; k++) {
    const int32_t v = tri_idx[3 * i + k];
    if (v >= 0 && v < num_vertices) c[k] = vertex_cell[v];
    ok = ok && c[k] >= 0;
  }
  ok = ok && c[0] != c[1] && c[1] != c[2] && c[2] != c[0];
  int32_t r0 = -1, r1 = -1, r2 = -1;
  if (ok) {
    if (c[0] < c[1] && c[0] < c[2]) { r0 = c[0]; r1 = c[1]; r2 = c[2]; }
    else if (c[1] < c[2]) { r0 = c[1]; r1 = c[2]; r2 = c[0]; }
    else { r0 = c[2]; r1 = c[0]; r2 = c[1]; }
  }
  out_faces[3 * i] = r0;
  out_faces[3 * i + 1] = r1;
  out_faces[3 * i + 2] = r2;
  out_keep[i] = 0;
}

// (the rotated triples come from the launch before: plain loads)
__global__ void __launch_bounds__(kSimplifyThreads) simplify_faces_insert_kernel(const int32_t *__restrict__ rotated, int32_t faces, int32_t *table,
                                                                                 uint64_t slot_mask) {
  const int64_t t64 = (int64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (t64 >= faces) return;
  const int32_t t = (int32_t)t64;
  const int32_t a = rotated[3 * t64], b = rotated[3 * t64 + 1], c = rotated[3 * t64 + 2];
  if (a < 0) return;
  uint64_t slot = triple_hash(a, b, c) & slot_mask;
  for (uint64_t probe = 0; probe <= slot_mask; probe++) {
    // The slot holds a face index; its key is that face's triple.  atomicMin only ever replaces the index by a smaller one
    // with the SAME triple, so whichever value is read here names the slot's key.
    const int32_t prev = atomicCAS(table + slot, kEmptyOwner, t);
    if (prev == kEmptyOwner) break;
    if (prev >= 0 && prev < faces && rotated[3 * (int64_t)prev] == a && rotated[3 * (int64_t)prev + 1] == b &&
        rotated[3 * (int64_t)prev + 2] == c) {
      atomicMin(table + slot, t);
      break;
    }
    slot = (slot + 1) & slot_mask;
  }
}

// (after the insert launch has ended: plain loads) keep[t] = the slot of t's triple holds t
__global__ void __launch_bounds__(kSimplifyThreads) simplify_faces_keep_kernel(const int32_t *__restrict__ rotated, int32_t faces,
                                                                               const int32_t *__restrict__ table, uint64_t slot_mask,
                                                                               uint8_t *__restrict__ out_keep) {
  const int64_t t64 = (int64_t)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (t64 >= faces) return;
  const int32_t t = (int32_t)t64;
  const int32_t a = rotated[3 * t64], b = rotated[3 * t64 + 1], c = rotated[3 * t64 + 2];
  if (a < 0) return;
  uint64_t slot = triple_hash(a, b, c) & slot_mask;
  for (uint64_t probe = 0; probe <= slot_mask; probe++) {
    const int32_t f = table[slot];
    if (f < 0 || f >= faces) break;   // an empty slot: a table the insert launch did not fill
    if (rotated[3 * (int64_t)f] == a && rotated[3 * (int64_t)f + 1] == b && rotated[3 * (int64_t)f + 2] == c) {
      out_keep[t64] = f == t;
      break;
    }
    slot = (slot + 1) & slot_mask;
  }
}

int check_voxel(double h, const char *what) {
  if (!(h > 0.0) || !std::isfinite(h)) { set_error("%s: voxel_size must be positive and finite", what); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_mesh_simplify_cells(const float *vertices, int64_t num_vertices, const float *min_bound, double voxel_size,
                                         uint64_t *keys, int32_t *owner, uint64_t num_slots, int32_t *out_slot, int32_t *out_overflow,
                                         scorp_stream_t stream) {
  if (!vertices || !min_bound || !keys || !owner || !out_slot || !out_overflow) {
    set_error("mesh_simplify_cells: NULL argument"); return SCORP_ERR_INVALID;
  }
  if (int e = check_vertices(num_vertices, "mesh_simplify_cells")) return e;
  if (int e = check_voxel(voxel_size, "mesh_simplify_cells")) return e;
  if (int e = check_slots(num_slots, (uint64_t)num_vertices, 2, 31, "mesh_simplify_cells", "num_vertices")) return e;
  hipStream_t s = (hipStream_t)stream;
  simplify_init_kernel<<<blocks_for(num_slots, kSimplifyThreads), kSimplifyThreads, 0, s>>>(keys, owner, num_slots, out_overflow);
  SCORP_KERNEL_CHECK("simplify_init", 0, s);
  simplify_cells_kernel<<<blocks_for((uint64_t)num_vertices, kSimplifyThreads), kSimplifyThreads, 0, s>>>(vertices, (int32_t)num_vertices, min_bound, voxel_size,
                                                                                           keys, owner, num_slots - 1, out_slot, out_overflow);
  SCORP_KERNEL_CHECK("simplify_cells", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_simplify_roots(const int32_t *owner, uint64_t num_slots, const int32_t *slot, int64_t num_vertices,
                                         int32_t *out_rep, uint8_t *out_is_root, scorp_stream_t stream) {
  if (!owner || !slot || !out_rep || !out_is_root) { set_error("mesh_simplify_roots: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_vertices(num_vertices, "mesh_simplify_roots")) return e;
  if (int e = check_slots(num_slots, (uint64_t)num_vertices, 2, 31, "mesh_simplify_roots", "num_vertices")) return e;
  hipStream_t s = (hipStream_t)stream;
  simplify_roots_kernel<<<blocks_for((uint64_t)num_vertices, kSimplifyThreads), kSimplifyThreads, 0, s>>>(owner, num_slots, slot, (int32_t)num_vertices, out_rep,
                                                                                           out_is_root);
  SCORP_KERNEL_CHECK("simplify_roots", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_simplify_accumulate(const float *vertices, const float *colors, int64_t num_vertices, const int32_t *faces,
                                              int64_t num_faces, const float *min_bound, double voxel_size, const int32_t *rep,
                                              const int32_t *rep_scan, int64_t num_cells, int32_t quadric, int32_t *out_vertex_cell,
                                              int32_t *out_cell_ijk, double *out_acc, scorp_stream_t stream) {
  if (!vertices || !colors || !min_bound || !rep || !rep_scan || !out_vertex_cell || !out_cell_ijk || !out_acc || (quadric && !faces)) {
    set_error("mesh_simplify_accumulate: NULL argument"); return SCORP_ERR_INVALID;
  }
  if (int e = check_vertices(num_vertices, "mesh_simplify_accumulate")) return e;
  if (int e = check_voxel(voxel_size, "mesh_simplify_accumulate")) return e;
  if (num_cells < 1 || num_cells > num_vertices) {
    set_error("mesh_simplify_accumulate: num_cells must be in [1, num_vertices]"); return SCORP_ERR_INVALID;
  }
  if (quadric)
    if (int e = check_faces(num_faces, "mesh_simplify_accumulate")) return e;
  hipStream_t s = (hipStream_t)stream;
  SCORP_HIP_CHECK(hipMemsetAsync(out_acc, 0, (size_t)num_cells * kAcc * sizeof(double), s));
  simplify_vertex_sums_kernel<<<blocks_for((uint64_t)num_vertices, kSimplifyThreads), kSimplifyThreads, 0, s>>>(
      vertices, colors, (int32_t)num_vertices, min_bound, voxel_size, rep, rep_scan, (int32_t)num_cells, out_vertex_cell, out_cell_ijk, out_acc);
  SCORP_KERNEL_CHECK("simplify_vertex_sums", 0, s);
  if (quadric) {
    simplify_quadrics_kernel<<<blocks_for((uint64_t)num_faces, kSimplifyThreads), kSimplifyThreads, 0, s>>>(
        faces, (int32_t)num_faces, vertices, (int32_t)num_vertices, min_bound, voxel_size, rep, rep_scan, (int32_t)num_cells, out_acc);
    SCORP_KERNEL_CHECK("simplify_quadrics", 0, s);
  }
  return SCORP_OK;
}

extern "C" int scorp_mesh_simplify_place(const double *acc, const int32_t *cell_ijk, int64_t num_cells, const float *min_bound,
                                         double voxel_size, int32_t quadric, float *out_vertices, float *out_colors, scorp_stream_t stream) {
  if (!acc || !cell_ijk || !min_bound || !out_vertices || !out_colors) { set_error("mesh_simplify_place: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_count(num_cells, 1, kMeshMaxVertices, "mesh_simplify_place", "num_cells", "2^30")) return e;
  if (int e = check_voxel(voxel_size, "mesh_simplify_place")) return e;
  hipStream_t s = (hipStream_t)stream;
  simplify_place_kernel<<<blocks_for((uint64_t)num_cells, kSimplifyThreads), kSimplifyThreads, 0, s>>>(acc, cell_ijk, (int32_t)num_cells, min_bound, voxel_size,
                                                                                        quadric ? 1 : 0, out_vertices, out_colors);
  SCORP_KERNEL_CHECK("simplify_place", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_simplify_faces(const int32_t *faces, int64_t num_faces, const int32_t *vertex_cell, int64_t num_vertices,
                                         int32_t *table, uint64_t num_slots, int32_t *out_faces, uint8_t *out_keep, scorp_stream_t stream) {
  if (!faces || !vertex_cell || !table || !out_faces || !out_keep) { set_error("mesh_simplify_faces: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_faces(num_faces, "mesh_simplify_faces")) return e;
  if (int e = check_vertices(num_vertices, "mesh_simplify_faces")) return e;
  if (int e = check_slots(num_slots, (uint64_t)num_faces, 2, 31, "mesh_simplify_faces", "num_faces")) return e;
  hipStream_t s = (hipStream_t)stream;
  const uint64_t n = num_slots > (uint64_t)num_faces ? num_slots : (uint64_t)num_faces;
  simplify_faces_remap_kernel<<<blocks_for(n, kSimplifyThreads), kSimplifyThreads, 0, s>>>(faces, (int32_t)num_faces, vertex_cell, (int32_t)num_vertices, table,
                                                                             num_slots, out_faces, out_keep);
  SCORP_KERNEL_CHECK("simplify_faces_remap", 0, s);
  simplify_faces_insert_kernel<<<blocks_for((uint64_t)num_faces, kSimplifyThreads), kSimplifyThreads, 0, s>>>(out_faces, (int32_t)num_faces, table, num_slots - 1);
  SCORP_KERNEL_CHECK("simplify_faces_insert", 0, s);
  simplify_faces_keep_kernel<<<blocks_for((uint64_t)num_faces, kSimplifyThreads), kSimplifyThreads, 0, s>>>(out_faces, (int32_t)num_faces, table, num_slots - 1,
                                                                                             out_keep);
  SCORP_KERNEL_CHECK("simplify_faces_keep", 0, s);
  return SCORP_OK;
}
