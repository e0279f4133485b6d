// mesh_decimate.hip — edge-collapse decimation of a triangle mesh to a target triangle count (Open3D's
// simplify_quadric_decimation is the use; the rules are this project's own).  Rules 0 - 11 are in include/scorp_gs.h;
// tests/mesh_decimate_reference.py restates them in plain Python over dictionaries.
//
// The collapses of one ROUND are an independent set of edges (no vertex of one equals or neighbours a vertex of another),
// so one launch applies them all and nothing a test read is changed by another collapse.  The caller keeps the sorts, the
// `unique` that numbers the edges, the prefix sums and the compaction; seven calls do the rest:
//   quadrics    once: Q[v] GATHERED per vertex over its faces in ascending face index (a vertex -> face CSR), the plane of
//               every face of non-zero area and a second plane through every one-face edge at the vertex.
//   flags       per round: bit 0 of flags[v] = v is on an edge with one face, bit 1 = on an edge with three or more
//               (atomicOr on int32: the bits do not depend on the order).
//   candidates  one thread per edge: placement by the closed-form 3x3 solve or the best of lo, hi, mid; cost; the link
//               condition and the flip test by walking the two vertices' face lists.  +inf = not a candidate.
//   hash        the priority of the window's edges.
//   select      vmin by int32 atomicMin over the ranked window, vmin2 by int32 atomicMin over all edges, then
//               selected[r] = (r == vmin2[lo] == vmin2[hi]).  No spin, no retry.
//   apply       the selected edges within the budget: P[lo] = x, Q[lo] += Q[hi], colours, counts, vmap[hi] = lo.
//   faces       faces mapped through vmap, keep[t] = 0 for a face with two equal indices.
// All arithmetic is float64 with fp contraction off; no float is summed by atomics, so every bit of the result is a
// function of the input alone.  No kernel uses LDS or scratch (tests/test_mesh_decimate_resources.py).  The vector type, the
// face load, the CSR slice and the host checks are mesh_common.hpp's; splitmix64 is common.hpp's.
#include "mesh_common.hpp"

namespace scorp {
namespace {

constexpr int kDecimateThreads = 256;
constexpr int32_t kNoRank = 0x7FFFFFFF;
constexpr int kQ = 10;   // doubles per quadric: A as xx xy xz yy yz zz, b 3, c
constexpr double kDetFloor = 1e-9, kReach = 4.0;

struct Quadric {
  double xx, xy, xz, yy, yz, zz, b0, b1, b2, c;
};

__device__ __forceinline__ Quadric load_q(const double *__restrict__ q, int64_t v) {
  const double *p = q + v * kQ;
  return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]};
}
__device__ __forceinline__ void store_q(double *__restrict__ q, int64_t v, const Quadric &a) {
  double *p = q + v * kQ;
  p[0] = a.xx; p[1] = a.xy; p[2] = a.xz; p[3] = a.yy; p[4] = a.yz; p[5] = a.zz; p[6] = a.b0; p[7] = a.b1; p[8] = a.b2; p[9] = a.c;
}
__device__ __forceinline__ Quadric add_q(const Quadric &a, const Quadric &b) {
#pragma clang fp contract(off)
  return {a.xx + b.xx, a.xy + b.xy, a.xz + b.xz, a.yy + b.yy, a.yz + b.yz, a.zz + b.zz, a.b0 + b.b0, a.b1 + b.b1, a.b2 + b.b2, a.c + b.c};
}
// q += w (n n^T, d n, d^2)
__device__ __forceinline__ void add_plane(Quadric &q, Vec3d n, double d, double w) {
#pragma clang fp contract(off)
  const double w0 = w * n.x, w1 = w * n.y, w2 = w * n.z, wd = w * d;
  q.xx += w0 * n.x; q.xy += w0 * n.y; q.xz += w0 * n.z;
  q.yy += w1 * n.y; q.yz += w1 * n.z; q.zz += w2 * n.z;
  q.b0 += wd * n.x; q.b1 += wd * n.y; q.b2 += wd * n.z;
  q.c += wd * d;
}
__device__ __forceinline__ double cost_of(const Quadric &q, Vec3d x) {
#pragma clang fp contract(off)
  const double s2 = (q.xx * (x.x * x.x) + q.yy * (x.y * x.y)) + q.zz * (x.z * x.z);
  const double s1 = (q.xy * (x.x * x.y) + q.xz * (x.x * x.z)) + q.yz * (x.y * x.z);
  const double s0 = (q.b0 * x.x + q.b1 * x.y) + q.b2 * x.z;
  const double c = ((s2 + 2.0 * s1) + 2.0 * s0) + q.c;
  return c > 0.0 ? c : 0.0;
}

// rule 4: the point of the collapse and its cost
__device__ __forceinline__ Vec3d place(const Quadric &q, Vec3d plo, Vec3d phi, double *cost) {
#pragma clang fp contract(off)
  const double c00 = q.yy * q.zz - q.yz * q.yz;
  const double c01 = q.xz * q.yz - q.xy * q.zz;
  const double c02 = q.xy * q.yz - q.xz * q.yy;
  const double c11 = q.xx * q.zz - q.xz * q.xz;
  const double c12 = q.xy * q.xz - q.xx * q.yz;
  const double c22 = q.xx * q.yy - q.xy * q.xy;
  const double det = (q.xx * c00 + q.xy * c01) + q.xz * c02;
  const double t = (q.xx + q.yy) + q.zz;
  const Vec3d mid = {0.5 * (plo.x + phi.x), 0.5 * (plo.y + phi.y), 0.5 * (plo.z + phi.z)};
  if (det > kDetFloor * ((t * t) * t)) {
    const Vec3d x = {-((c00 * q.b0 + c01 * q.b1) + c02 * q.b2) / det, -((c01 * q.b0 + c11 * q.b1) + c12 * q.b2) / det,
                  -((c02 * q.b0 + c12 * q.b1) + c22 * q.b2) / det};
    const Vec3d dx = sub3(x, mid), de = sub3(phi, plo);
    if (dot3(dx, dx) <= kReach * dot3(de, de)) {   // (false for NaN)
      *cost = cost_of(q, x);
      return x;
    }
  }
  Vec3d best = plo;
  double best_cost = cost_of(q, plo);
  const double ch = cost_of(q, phi), cm = cost_of(q, mid);
  if (ch < best_cost) { best = phi; best_cost = ch; }
  if (cm < best_cost) { best = mid; best_cost = cm; }
  *cost = best_cost;
  return best;
}

__device__ __forceinline__ bool edge_ends(const int64_t *__restrict__ keys, int64_t e, int32_t num_vertices, int32_t *lo, int32_t *hi) {
  const uint64_t k = (uint64_t)keys[e];
  *lo = (int32_t)(k >> 32);
  *hi = (int32_t)(k & 0xFFFFFFFFull);
  return (k >> 32) < (uint64_t)num_vertices && (k & 0xFFFFFFFFull) < (uint64_t)num_vertices;
}

// Rule 1.  One thread per vertex; its faces come in ascending index from the CSR.  Per face: the face's plane, then the
// planes of its one-face edges k = 0, 1, 2 (from corner k to corner k + 1) that touch the vertex.
__global__ void __launch_bounds__(kDecimateThreads) decimate_quadrics_kernel(const double *__restrict__ P, int32_t num_vertices,
                                                                             const int32_t *__restrict__ faces, int32_t num_faces,
                                                                             const int32_t *__restrict__ face_edge,
                                                                             const int32_t *__restrict__ edge_faces, int32_t num_edges,
                                                                             const int32_t *__restrict__ vf_start,
                                                                             const int32_t *__restrict__ vf_face, double boundary_weight,
                                                                             double *__restrict__ out_Q) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (v >= num_vertices) return;
  Quadric q = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const Range r = csr_range(vf_start, v, 3 * (int64_t)num_faces);
  for (int64_t i = r.beg; i < r.end; i++) {
    const int32_t t = vf_face[i];
    if (t < 0 || t >= num_faces) continue;
    const Face f = load_face(faces, t, num_vertices);
    if (!f.ok) continue;
    const Vec3d p0 = load3(P, f.a), p1 = load3(P, f.b), p2 = load3(P, f.c);
    const Vec3d N = cross3(sub3(p1, p0), sub3(p2, p0));
    const double len = norm3(N);
    if (!(len > 0.0)) continue;
    const Vec3d n = div3(N, len);
    add_plane(q, n, -dot3(n, p0), 0.5 * len);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int32_t va = k == 0 ? f.a : k == 1 ? f.b : f.c, vb = k == 0 ? f.b : k == 1 ? f.c : f.a;
      if (va != (int32_t)v && vb != (int32_t)v) continue;
      const int32_t e = face_edge[3 * (int64_t)t + k];
      if (e < 0 || e >= num_edges || edge_faces[e] != 1) continue;
      const Vec3d pa = k == 0 ? p0 : k == 1 ? p1 : p2, pb = k == 0 ? p1 : k == 1 ? p2 : p0;
      const Vec3d ev = sub3(pb, pa);
      const Vec3d m = cross3(ev, n);
      const double ml = norm3(m);
      if (!(ml > 0.0)) continue;
      const Vec3d mu = div3(m, ml);
      add_plane(q, mu, -dot3(mu, pa), boundary_weight * dot3(ev, ev));
    }
  }
  store_q(out_Q, v, q);
}

__global__ void __launch_bounds__(kDecimateThreads) decimate_flags_kernel(const int64_t *__restrict__ keys,
                                                                          const int32_t *__restrict__ edge_faces, int32_t num_edges,
                                                                          int32_t num_vertices, int32_t *flags) {
  const int64_t e = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (e >= num_edges) return;
  int32_t lo, hi;
  if (!edge_ends(keys, e, num_vertices, &lo, &hi)) return;
  const int32_t n = edge_faces[e];
  const int32_t bits = (n == 1 ? 1 : 0) | (n >= 3 ? 2 : 0);
  if (bits) {
    atomicOr(flags + lo, bits);
    atomicOr(flags + hi, bits);
  }
}

// true when some face of vertex v contains u
__device__ __forceinline__ bool has_neighbour(const int32_t *__restrict__ faces, int32_t num_faces, int32_t num_vertices,
                                              const int32_t *__restrict__ vf_face, Range r, int32_t u) {
  bool found = false;
  for (int64_t i = r.beg; i < r.end; i++) {
    const int32_t t = vf_face[i];
    if (t < 0 || t >= num_faces) continue;
    const Face f = load_face(faces, t, num_vertices);
    found = found || f.a == u || f.b == u || f.c == u;
  }
  return found;
}

// Rule 5 for one face that holds `moved` and not the edge's other end: the normal before and after `moved` goes to x
__device__ __forceinline__ bool flip_ok(const double *__restrict__ P, Face f, int32_t moved, Vec3d x) {
#pragma clang fp contract(off)
  const Vec3d p0 = load3(P, f.a), p1 = load3(P, f.b), p2 = load3(P, f.c);
  const Vec3d old_n = cross3(sub3(p1, p0), sub3(p2, p0));
  const Vec3d q0 = f.a == moved ? x : p0, q1 = f.b == moved ? x : p1, q2 = f.c == moved ? x : p2;
  const Vec3d new_n = cross3(sub3(q1, q0), sub3(q2, q0));
  return dot3(old_n, new_n) > 0.0;
}

__global__ void __launch_bounds__(kDecimateThreads) decimate_candidates_kernel(const double *__restrict__ P, const double *__restrict__ Q,
                                                                               int32_t num_vertices, const int32_t *__restrict__ faces,
                                                                               int32_t num_faces, const int64_t *__restrict__ keys,
                                                                               const int32_t *__restrict__ edge_faces, int32_t num_edges,
                                                                               const int32_t *__restrict__ vf_start,
                                                                               const int32_t *__restrict__ vf_face,
                                                                               const int32_t *__restrict__ flags, double maximum_error,
                                                                               double *__restrict__ out_cost, double *__restrict__ out_x) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (e >= num_edges) return;
  const double inf = __builtin_inf();
  double cost = inf;
  Vec3d x = {0.0, 0.0, 0.0};
  int32_t lo, hi;
  bool ok = edge_ends(keys, e, num_vertices, &lo, &hi) && lo != hi;
  const int32_t n = edge_faces[e];
  ok = ok && (n == 1 || n == 2);
  if (ok) {
    const int32_t fl = flags[lo], fh = flags[hi];
    ok = !((fl | fh) & 2) && !(n == 2 && (fl & 1) && (fh & 1));
  }
  if (ok) {
    const Vec3d plo = load3(P, lo), phi = load3(P, hi);
    double c;
    x = place(add_q(load_q(Q, lo), load_q(Q, hi)), plo, phi, &c);
    ok = c <= maximum_error;   // (false for NaN)
    const int64_t entries = 3 * (int64_t)num_faces;
    const Range rlo = csr_range(vf_start, lo, entries), rhi = csr_range(vf_start, hi, entries);
    // the faces of lo: those with hi give the apexes
    int32_t apex0 = -1, apex1 = -1, shared = 0;
    if (ok) {
      for (int64_t i = rlo.beg; i < rlo.end; i++) {
        const int32_t t = vf_face[i];
        if (t < 0 || t >= num_faces) continue;
        const Face f = load_face(faces, t, num_vertices);
        if (!f.ok) { ok = false; continue; }
        if (f.a == hi || f.b == hi || f.c == hi) {
          const int32_t apex = (f.a != lo && f.a != hi) ? f.a : (f.b != lo && f.b != hi) ? f.b : f.c;
          if (shared == 0) apex0 = apex; else apex1 = apex;
          shared++;
        }
      }
      // as many distinct apexes as the edge has faces
      ok = ok && shared == n && !(n == 2 && apex0 == apex1);
    }
    if (ok) {
      // the link condition: a vertex next to lo and to hi is an apex; and the flip test of lo's faces
      for (int64_t i = rlo.beg; i < rlo.end && ok; i++) {
        const int32_t t = vf_face[i];
        if (t < 0 || t >= num_faces) continue;
        const Face f = load_face(faces, t, num_vertices);
        if (f.a == hi || f.b == hi || f.c == hi) continue;
        // the two vertices of the face that are not lo
        const int32_t u0 = f.a == lo ? f.b : f.a, u1 = f.c == lo ? f.b : f.c;
        if (u0 != apex0 && u0 != apex1 && has_neighbour(faces, num_faces, num_vertices, vf_face, rhi, u0)) ok = false;
        if (u1 != apex0 && u1 != apex1 && has_neighbour(faces, num_faces, num_vertices, vf_face, rhi, u1)) ok = false;
        ok = ok && flip_ok(P, f, lo, x);
      }
      for (int64_t i = rhi.beg; i < rhi.end && ok; i++) {
        const int32_t t = vf_face[i];
        if (t < 0 || t >= num_faces) continue;
        const Face f = load_face(faces, t, num_vertices);
        if (!f.ok) { ok = false; continue; }
        if (f.a == lo || f.b == lo || f.c == lo) continue;
        ok = ok && flip_ok(P, f, hi, x);
      }
    }
    if (ok) cost = c;
  }
  out_cost[e] = cost;
  out_x[3 * e] = x.x;
  out_x[3 * e + 1] = x.y;
  out_x[3 * e + 2] = x.z;
}

__global__ void __launch_bounds__(kDecimateThreads) decimate_hash_kernel(const int64_t *__restrict__ keys, int32_t num_edges,
                                                                         const int32_t *__restrict__ window, int32_t num_window,
                                                                         uint64_t round_mix, int64_t *__restrict__ out_hash) {
  const int64_t i = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (i >= num_window) return;
  const int32_t e = window[i];
  out_hash[i] = e >= 0 && e < num_edges ? (int64_t)(splitmix64((uint64_t)keys[e] ^ round_mix) >> 1) : 0x7FFFFFFFFFFFFFFFll;
}

__global__ void __launch_bounds__(kDecimateThreads) decimate_vmin_init_kernel(int32_t *__restrict__ vmin, int32_t num_vertices) {
  const int64_t v = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (v < num_vertices) vmin[v] = kNoRank;
}

// (ranked[r] = the window's edge of rank r)
__global__ void __launch_bounds__(kDecimateThreads) decimate_vmin_kernel(const int64_t *__restrict__ keys, int32_t num_edges,
                                                                         const int32_t *__restrict__ ranked, int32_t num_window,
                                                                         int32_t num_vertices, int32_t *vmin) {
  const int64_t r = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (r >= num_window) return;
  const int32_t e = ranked[r];
  int32_t lo, hi;
  if (e < 0 || e >= num_edges || !edge_ends(keys, e, num_vertices, &lo, &hi)) return;
  atomicMin(vmin + lo, (int32_t)r);
  atomicMin(vmin + hi, (int32_t)r);
}

// (after the vmin launch has ended: plain loads of vmin; vmin2 starts as a copy of vmin)
__global__ void __launch_bounds__(kDecimateThreads) decimate_vmin2_kernel(const int64_t *__restrict__ keys, int32_t num_edges,
                                                                          int32_t num_vertices, const int32_t *__restrict__ vmin,
                                                                          int32_t *vmin2) {
  const int64_t e = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (e >= num_edges) return;
  int32_t lo, hi;
  if (!edge_ends(keys, e, num_vertices, &lo, &hi)) return;
  const int32_t a = vmin[lo], b = vmin[hi];
  if (b != kNoRank) atomicMin(vmin2 + lo, b);
  if (a != kNoRank) atomicMin(vmin2 + hi, a);
}

__global__ void __launch_bounds__(kDecimateThreads) decimate_select_kernel(const int64_t *__restrict__ keys, int32_t num_edges,
                                                                           const int32_t *__restrict__ ranked, int32_t num_window,
                                                                           int32_t num_vertices, const int32_t *__restrict__ vmin2,
                                                                           uint8_t *__restrict__ out_selected) {
  const int64_t r = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (r >= num_window) return;
  const int32_t e = ranked[r];
  int32_t lo, hi;
  bool sel = e >= 0 && e < num_edges && edge_ends(keys, e, num_vertices, &lo, &hi);
  sel = sel && vmin2[lo] == (int32_t)r && vmin2[hi] == (int32_t)r;
  out_selected[r] = sel;
}

__global__ void __launch_bounds__(kDecimateThreads) decimate_identity_kernel(int32_t *__restrict__ vmap, int32_t num_vertices) {
  const int64_t v = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (v < num_vertices) vmap[v] = (int32_t)v;
}

// Rule 10.  The applied edges are independent: lo and hi of one are no vertex of another, so every load here reads what
// the round began with and every store has one writer.
__global__ void __launch_bounds__(kDecimateThreads) decimate_apply_kernel(const int64_t *__restrict__ keys, int32_t num_edges,
                                                                          const int32_t *__restrict__ ranked,
                                                                          const uint8_t *__restrict__ applied, int32_t num_window,
                                                                          const double *__restrict__ x, int32_t num_vertices, double *P,
                                                                          double *Q, double *C, int32_t *count, int32_t *vmap) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (r >= num_window || !applied[r]) return;
  const int32_t e = ranked[r];
  int32_t lo, hi;
  if (e < 0 || e >= num_edges || !edge_ends(keys, e, num_vertices, &lo, &hi) || lo == hi) return;
  store_q(Q, lo, add_q(load_q(Q, lo), load_q(Q, hi)));
  const int32_t cl = count[lo], ch = count[hi];
  const double nl = (double)cl, nh = (double)ch, total = nl + nh;
  for (int k = 0; k < 3; k++) {
    P[3 * (int64_t)lo + k] = x[3 * (int64_t)e + k];
    C[3 * (int64_t)lo + k] = (nl * C[3 * (int64_t)lo + k] + nh * C[3 * (int64_t)hi + k]) / total;
  }
  count[lo] = cl + ch;
  vmap[hi] = lo;
}

__global__ void __launch_bounds__(kDecimateThreads) decimate_faces_kernel(const int32_t *__restrict__ faces, int32_t num_faces,
                                                                          const int32_t *__restrict__ vmap, int32_t num_vertices,
                                                                          int32_t *__restrict__ out_faces, uint8_t *__restrict__ out_keep) {
  const int64_t t = (int64_t)blockIdx.x * kDecimateThreads + threadIdx.x;
  if (t >= num_faces) return;
  int32_t m[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int32_t v = faces[3 * t + k];
    const bool in = v >= 0 && v < num_vertices;
    m[k] = in ? vmap[v] : -1;
    ok = ok && in;
    out_faces[3 * t + k] = m[k];
  }
  out_keep[t] = ok && m[0] != m[1] && m[1] != m[2] && m[2] != m[0];
}

int check_mesh(int64_t num_vertices, int64_t num_faces, const char *what) {
  if (int e = check_vertices(num_vertices, what)) return e;
  return check_faces(num_faces, what);
}
// every face has three edges and every edge at least one face
int check_edges(int64_t num_edges, int64_t num_faces, const char *what) {
  if (num_edges < 1 || num_edges > 3 * num_faces) {
    set_error("%s: num_edges must be in [1, 3 num_faces]", what); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}
int check_window(int64_t num_window, int64_t num_edges, const char *what) {
  if (num_window < 1 || num_window > num_edges) {
    set_error("%s: num_window must be in [1, num_edges]", what); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_mesh_decimate_quadrics(const double *positions, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                            const int32_t *face_edge, const int32_t *edge_faces, int64_t num_edges,
                                            const int32_t *vf_start, const int32_t *vf_face, double boundary_weight,
                                            double *out_quadrics, scorp_stream_t stream) {
  if (!positions || !faces || !face_edge || !edge_faces || !vf_start || !vf_face || !out_quadrics) {
    set_error("mesh_decimate_quadrics: NULL argument"); return SCORP_ERR_INVALID;
  }
  if (int e = check_mesh(num_vertices, num_faces, "mesh_decimate_quadrics")) return e;
  if (int e = check_edges(num_edges, num_faces, "mesh_decimate_quadrics")) return e;
  if (!(boundary_weight >= 0.0) || !std::isfinite(boundary_weight)) {
    set_error("mesh_decimate_quadrics: boundary_weight must be finite and not negative"); return SCORP_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  decimate_quadrics_kernel<<<blocks_for(num_vertices, kDecimateThreads), kDecimateThreads, 0, s>>>(
      positions, (int32_t)num_vertices, faces, (int32_t)num_faces, face_edge, edge_faces, (int32_t)num_edges, vf_start, vf_face,
      boundary_weight, out_quadrics);
  SCORP_KERNEL_CHECK("decimate_quadrics", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_decimate_flags(const int64_t *edge_keys, const int32_t *edge_faces, int64_t num_edges, int64_t num_vertices,
                                         int32_t *out_flags, scorp_stream_t stream) {
  if (!edge_keys || !edge_faces || !out_flags) { set_error("mesh_decimate_flags: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_vertices(num_vertices, "mesh_decimate_flags")) return e;
  if (int e = check_edges(num_edges, kMeshMaxFaces, "mesh_decimate_flags")) return e;
  hipStream_t s = (hipStream_t)stream;
  SCORP_HIP_CHECK(hipMemsetAsync(out_flags, 0, (size_t)num_vertices * sizeof(int32_t), s));
  decimate_flags_kernel<<<blocks_for(num_edges, kDecimateThreads), kDecimateThreads, 0, s>>>(edge_keys, edge_faces, (int32_t)num_edges,
                                                                                (int32_t)num_vertices, out_flags);
  SCORP_KERNEL_CHECK("decimate_flags", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_decimate_candidates(const double *positions, const double *quadrics, int64_t num_vertices,
                                              const int32_t *faces, int64_t num_faces, const int64_t *edge_keys,
                                              const int32_t *edge_faces, int64_t num_edges, const int32_t *vf_start,
                                              const int32_t *vf_face, const int32_t *flags, double maximum_error, double *out_cost,
                                              double *out_x, scorp_stream_t stream) {
  if (!positions || !quadrics || !faces || !edge_keys || !edge_faces || !vf_start || !vf_face || !flags || !out_cost || !out_x) {
    set_error("mesh_decimate_candidates: NULL argument"); return SCORP_ERR_INVALID;
  }
  if (int e = check_mesh(num_vertices, num_faces, "mesh_decimate_candidates")) return e;
  if (int e = check_edges(num_edges, num_faces, "mesh_decimate_candidates")) return e;
  if (!(maximum_error >= 0.0)) { set_error("mesh_decimate_candidates: maximum_error must not be negative or NaN"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  decimate_candidates_kernel<<<blocks_for(num_edges, kDecimateThreads), kDecimateThreads, 0, s>>>(
      positions, quadrics, (int32_t)num_vertices, faces, (int32_t)num_faces, edge_keys, edge_faces, (int32_t)num_edges, vf_start, vf_face,
      flags, maximum_error, out_cost, out_x);
  SCORP_KERNEL_CHECK("decimate_candidates", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_decimate_hash(const int64_t *edge_keys, int64_t num_edges, const int32_t *window, int64_t num_window,
                                        int64_t round, int64_t *out_hash, scorp_stream_t stream) {
  if (!edge_keys || !window || !out_hash) { set_error("mesh_decimate_hash: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_edges(num_edges, kMeshMaxFaces, "mesh_decimate_hash")) return e;
  if (int e = check_window(num_window, num_edges, "mesh_decimate_hash")) return e;
  if (round < 1) { set_error("mesh_decimate_hash: round counts from 1"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  decimate_hash_kernel<<<blocks_for(num_window, kDecimateThreads), kDecimateThreads, 0, s>>>(edge_keys, (int32_t)num_edges, window, (int32_t)num_window,
                                                                                splitmix64((uint64_t)round), out_hash);
  SCORP_KERNEL_CHECK("decimate_hash", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_decimate_select(const int64_t *edge_keys, int64_t num_edges, const int32_t *ranked, int64_t num_window,
                                          int64_t num_vertices, int32_t *vmin, int32_t *vmin2, uint8_t *out_selected,
                                          scorp_stream_t stream) {
  if (!edge_keys || !ranked || !vmin || !vmin2 || !out_selected) { set_error("mesh_decimate_select: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_vertices(num_vertices, "mesh_decimate_select")) return e;
  if (int e = check_edges(num_edges, kMeshMaxFaces, "mesh_decimate_select")) return e;
  if (int e = check_window(num_window, num_edges, "mesh_decimate_select")) return e;
  hipStream_t s = (hipStream_t)stream;
  const int32_t E = (int32_t)num_edges, W = (int32_t)num_window, Nv = (int32_t)num_vertices;
  decimate_vmin_init_kernel<<<blocks_for(num_vertices, kDecimateThreads), kDecimateThreads, 0, s>>>(vmin, Nv);
  SCORP_KERNEL_CHECK("decimate_vmin_init", 0, s);
  decimate_vmin_kernel<<<blocks_for(num_window, kDecimateThreads), kDecimateThreads, 0, s>>>(edge_keys, E, ranked, W, Nv, vmin);
  SCORP_KERNEL_CHECK("decimate_vmin", 0, s);
  SCORP_HIP_CHECK(hipMemcpyAsync(vmin2, vmin, (size_t)num_vertices * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  decimate_vmin2_kernel<<<blocks_for(num_edges, kDecimateThreads), kDecimateThreads, 0, s>>>(edge_keys, E, Nv, vmin, vmin2);
  SCORP_KERNEL_CHECK("decimate_vmin2", 0, s);
  decimate_select_kernel<<<blocks_for(num_window, kDecimateThreads), kDecimateThreads, 0, s>>>(edge_keys, E, ranked, W, Nv, vmin2, out_selected);
  SCORP_KERNEL_CHECK("decimate_select", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_decimate_apply(const int64_t *edge_keys, int64_t num_edges, const int32_t *ranked, const uint8_t *applied,
                                         int64_t num_window, const double *x, int64_t num_vertices, double *positions,
                                         double *quadrics, double *colors, int32_t *count, int32_t *out_vmap, scorp_stream_t stream) {
  if (!edge_keys || !ranked || !applied || !x || !positions || !quadrics || !colors || !count || !out_vmap) {
    set_error("mesh_decimate_apply: NULL argument"); return SCORP_ERR_INVALID;
  }
  if (int e = check_vertices(num_vertices, "mesh_decimate_apply")) return e;
  if (int e = check_edges(num_edges, kMeshMaxFaces, "mesh_decimate_apply")) return e;
  if (int e = check_window(num_window, num_edges, "mesh_decimate_apply")) return e;
  hipStream_t s = (hipStream_t)stream;
  decimate_identity_kernel<<<blocks_for(num_vertices, kDecimateThreads), kDecimateThreads, 0, s>>>(out_vmap, (int32_t)num_vertices);
  SCORP_KERNEL_CHECK("decimate_identity", 0, s);
  decimate_apply_kernel<<<blocks_for(num_window, kDecimateThreads), kDecimateThreads, 0, s>>>(edge_keys, (int32_t)num_edges, ranked, applied,
                                                                                 (int32_t)num_window, x, (int32_t)num_vertices, positions,
                                                                                 quadrics, colors, count, out_vmap);
  SCORP_KERNEL_CHECK("decimate_apply", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_mesh_decimate_faces(const int32_t *faces, int64_t num_faces, const int32_t *vmap, int64_t num_vertices,
                                         int32_t *out_faces, uint8_t *out_keep, scorp_stream_t stream) {
  if (!faces || !vmap || !out_faces || !out_keep) { set_error("mesh_decimate_faces: NULL argument"); return SCORP_ERR_INVALID; }
  if (int e = check_mesh(num_vertices, num_faces, "mesh_decimate_faces")) return e;
  hipStream_t s = (hipStream_t)stream;
  decimate_faces_kernel<<<blocks_for(num_faces, kDecimateThreads), kDecimateThreads, 0, s>>>(faces, (int32_t)num_faces, vmap, (int32_t)num_vertices, out_faces,
                                                                                out_keep);
  SCORP_KERNEL_CHECK("decimate_faces", 0, s);
  return SCORP_OK;
}
