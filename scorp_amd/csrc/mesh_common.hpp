// mesh_common.hpp — what the six mesh_*.hip files share: the bounds of a mesh and their host checks, the launch grid, the
// float64 3-vector every bit-exact rule of include/scorp_gs.h is computed in, the checked face load, the clamped CSR slice,
// the open-addressing claim of mesh_cluster.hip and mesh_simplify.hip, and the wave loop that combines equal keys before an
// atomic.  (wave_sum_f64, wave_sum_u64, mix64 and splitmix64 are in common.hpp.)
#pragma once
#include "common.hpp"

namespace scorp {

constexpr int64_t kMeshMaxVertices = (int64_t)1 << 30;
constexpr int64_t kMeshMaxFaces = (int64_t)1 << 28;

inline unsigned blocks_for(uint64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// ---- host range checks: "<what>: <name> must be in [<least>, <bound>]", and "; got <n>" after it for the callers that say so ----

inline int check_count(int64_t n, int64_t least, int64_t most, const char *what, const char *name, const char *bound, bool got = false) {
  if (n >= least && n <= most) return SCORP_OK;
  if (got) set_error("%s: %s must be in [%lld, %s]; got %lld", what, name, (long long)least, bound, (long long)n);
  else set_error("%s: %s must be in [%lld, %s]", what, name, (long long)least, bound);
  return SCORP_ERR_INVALID;
}
inline int check_vertices(int64_t n, const char *what, bool got = false) {
  return check_count(n, 1, kMeshMaxVertices, what, "num_vertices", "2^30", got);
}
inline int check_faces(int64_t n, const char *what, int64_t least = 1, bool got = false) {
  return check_count(n, least, kMeshMaxFaces, what, "num_faces", "2^28", got);
}
// a table of num_slots for `entries` keys: a power of two, at least factor * entries (factor <of> in the message), at most 2^max_log2
inline int check_slots(uint64_t num_slots, uint64_t entries, unsigned factor, int max_log2, const char *what, const char *of) {
  if (num_slots == 0 || (num_slots & (num_slots - 1)) != 0) {
    set_error("%s: num_slots must be a power of two", what); return SCORP_ERR_INVALID;
  }
  if (num_slots < factor * entries) {
    set_error("%s: num_slots must be at least %u %s (%llu < %llu)", what, factor, of, (unsigned long long)num_slots,
              (unsigned long long)(factor * entries));
    return SCORP_ERR_INVALID;
  }
  if (num_slots > ((uint64_t)1 << max_log2)) { set_error("%s: num_slots above 2^%d", what, max_log2); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

#ifdef __HIPCC__
// ---- the float64 3-vector ----
// Every helper rounds each product and sum on its own (hipcc's default contracts across statements, so a caller's pragma
// does not reach into a helper) and keeps the association the rules fix: (x x + y y) + z z.

struct Vec3d {
  double x, y, z;
};

__device__ __forceinline__ Vec3d load3(const float *__restrict__ p, int64_t i) {
  return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]};
}
__device__ __forceinline__ Vec3d load3(const double *__restrict__ p, int64_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ void store3(float *__restrict__ out, int64_t i, const Vec3d &v) {
  out[3 * i] = (float)v.x;
  out[3 * i + 1] = (float)v.y;
  out[3 * i + 2] = (float)v.z;
}
__device__ __forceinline__ Vec3d sub3(Vec3d a, Vec3d b) {
#pragma clang fp contract(off)
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
__device__ __forceinline__ double dot3(Vec3d u, Vec3d w) {
#pragma clang fp contract(off)
  return (u.x * w.x + u.y * w.y) + u.z * w.z;
}
__device__ __forceinline__ Vec3d cross3(Vec3d u, Vec3d w) {
#pragma clang fp contract(off)
  return {u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
__device__ __forceinline__ Vec3d along3(Vec3d a, double t, Vec3d e) {   // a + t e
#pragma clang fp contract(off)
  return {a.x + t * e.x, a.y + t * e.y, a.z + t * e.z};
}
__device__ __forceinline__ double norm3(Vec3d v) {
#pragma clang fp contract(off)
  return sqrt(dot3(v, v));
}
__device__ __forceinline__ Vec3d div3(Vec3d v, double s) {
#pragma clang fp contract(off)
  return {v.x / s, v.y / s, v.z / s};
}
// v over its length; a zero length (or a NaN) gives +0
__device__ __forceinline__ Vec3d unit3(Vec3d v) {
  const double len = norm3(v);
  if (!(len > 0.0)) return {0.0, 0.0, 0.0};
  return div3(v, len);
}

// ---- faces ----

struct Face {
  int32_t a, b, c;
  bool ok;   // all three in [0, num_vertices)
};
// (one unsigned compare per index; num_vertices may be 2^31, which lets every non-negative int32 through)
__device__ __forceinline__ Face load_face(const int32_t *__restrict__ faces, int64_t t, uint32_t num_vertices) {
  Face f = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2], false};
  f.ok = (uint32_t)f.a < num_vertices && (uint32_t)f.b < num_vertices && (uint32_t)f.c < num_vertices;
  return f;
}
// (b - a) x (c - a) from float32 vertices: float64 differences of the float32 values out of corner 0.  Its length is twice
// the face's area (the cluster areas, the quadrics of mesh_simplify.hip, rule 5 of the mesh-smooth block).
__device__ __forceinline__ Vec3d face_cross(const float *__restrict__ verts, const Face &f) {
  const Vec3d a = load3(verts, f.a);
  return cross3(sub3(load3(verts, f.b), a), sub3(load3(verts, f.c), a));
}

// row `row` of a CSR clamped to its array of `entries` (offsets that do not belong to the array are never followed out of it)
struct Range {
  int64_t beg, end;
};
__device__ __forceinline__ Range csr_range(const int32_t *__restrict__ offsets, int64_t row, int64_t entries) {
  const int64_t b = min(max((int64_t)offsets[row], (int64_t)0), entries);
  return {b, min(max((int64_t)offsets[row + 1], b), entries)};
}

// ---- the open-addressing table of 64-bit keys with an int32 owner per slot ----

constexpr uint64_t kEmptyKey = ~(uint64_t)0;   // no edge and no cell has it: vertex indices are non-negative int32, a cell key has 63 bits
constexpr int32_t kEmptyOwner = 0x7FFFFFFF;    // above every vertex and face index
constexpr int64_t kTableFull = -1;

// The slot of `key`: claimed by ONE 64-bit compare-and-swap, linear probing bounded by the table's size (the callers keep
// at most half the slots taken).  Whoever gets the slot back then takes atomicMin(&owner[slot], self).
__device__ __forceinline__ int64_t table_claim(uint64_t *keys, uint64_t slot_mask, uint64_t key) {
  uint64_t slot = mix64(key) & slot_mask;
  for (uint64_t probe = 0; probe <= slot_mask; probe++) {
    const uint64_t prev = atomicCAS((unsigned long long *)(keys + slot), (unsigned long long)kEmptyKey, (unsigned long long)key);
    if (prev == kEmptyKey || prev == key) return (int64_t)slot;
    slot = (slot + 1) & slot_mask;
  }
  return kTableFull;
}

// Lanes of the wave that hold the same key combine, and the first of them issues the atomics: one per distinct key in the
// wave instead of 64 on one address.  group(key, mine, count, leads) runs once per distinct key >= 0: mine = this lane
// holds it, count = how many lanes do, leads = this lane is the first of them.  The loop is wave-uniform (every lane runs
// every round, the lanes without a contribution with key = -1), so the ballots and a butterfly inside group see all 64
// lanes.
template <typename G>
__device__ __forceinline__ void wave_combine_equal(int32_t key, G group) {
  const int lane = threadIdx.x & 63;
  uint64_t todo = __ballot(key >= 0);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const int32_t lk = __shfl(key, leader);
    const bool mine = key == lk;
    const uint64_t same = __ballot(mine);
    group(lk, mine, (int)__builtin_popcountll(same), lane == leader);
    todo &= ~same;
  }
}
#endif  // __HIPCC__

}  // namespace scorp
