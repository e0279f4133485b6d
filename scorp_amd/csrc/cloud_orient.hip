// cloud_orient.hip - consistent orientation of a cloud's normals by sign propagation along the minimum spanning forest of
// its neighbour graph (scorp_amd/global_registration.py: orient_normals_consistent_tangent_plane; the rules O1 - O6 are in
// the global-registration block of include/scorp_gs.h, tests/orient_reference.py restates them with Kruskal in float64).
//
// Boruvka.  Two words per vertex carry the forest:
//   snap[i]  (root of i's component, parity of i relative to that root) as the LAST compression left it.  Written by the
//            compression launch alone, each lane its own word: every other launch reads a settled snapshot.
//   par[x]   (an ancestor of x, parity of x relative to it); par[x] = (x, 0) while x is a root.  One 32-bit word, 30 bits
//            of index and the parity in bit 30, so a reader always has a consistent pair whichever store it sees.
// A round is four launches, one lane per vertex in each:
//   weight    every listed edge {i, j} whose ends lie in different components offers the order-preserving 64-bit code of
//             its weight to BOTH components' slots by atomicMin (i's own slot once per vertex, j's behind a read of the
//             slot): an edge only the other side lists is offered too, and no symmetrised list is built.  Any such edge
//             raises the round's work flag.
//   edge      the same walk; among the edges whose code equals the slot's minimum, atomicMin of lo << 32 | hi.  After the
//             two launches a component's slot holds its smallest outgoing edge in O3's order, exactly.
//   hook      the lane of a root r reads that edge, finds the other component's root o in the snapshot and stores
//             par[r] = (o, f(u) ^ f(v) ^ [dot < 0]).  When o chose the same edge only the larger root is hooked; O3's order is
//             strict and total, so no other cycle can arise.  Each root is written by its own lane only, and the edge goes
//             into row r of the tree output: a vertex stops being a root once and for all, so the rows never collide.
//   compress  every lane walks from its snapshot's root to the new root, adding parities, halving the path on the way (a
//             halving store replaces one valid (ancestor, parity) word by another, so concurrent walks cannot be misled),
//             stores its snapshot and clears its slot for the next round.
// ceil(log2 n) + 1 rounds are launched unconditionally; a round whose predecessor found no edge between components returns
// at once on the device flag.  Nothing is read back, no lane waits for a value another lane must still write, and every
// walk ends after n steps at the latest.  The finish takes the smallest index of every component (atomicMin), the O5 votes
// (integer atomicAdd) and writes the outputs.  Only integer atomics whose result does not depend on their order: every
// output is a function of the input alone.
#include <cmath>

#include "common.hpp"

// O2, O5: every product and every sum is rounded on its own
#pragma clang fp contract(off)

namespace scorp {
namespace {

constexpr int kOrientThreads = 256;
constexpr int kOrientMaxK = 64;
constexpr int kOrientMaxRounds = 32;               // ceil(log2 2^30) + 1 = 31
constexpr uint32_t kParity = 1u << 30, kIndexMask = kParity - 1u;
constexpr unsigned long long kNoEdge = ~0ull;
// O5's default centre: lane g of kCenterLanes adds the points g, g + kCenterLanes, ... in ascending order, lane t of the
// second launch the partial sums kCenterRun t .. kCenterRun t + kCenterRun - 1, and its lane 0 those 256
constexpr int kCenterLanes = 16384, kCenterThreads = 256, kCenterRun = kCenterLanes / kCenterThreads;

struct OrientLayout {
  size_t snap, par, best_w, best_e, low, votes, work, partial, center, total;
  explicit OrientLayout(int64_t n) {
    size_t off = 0;
    snap = off; off = align_up(off + (size_t)n * 4, 256);
    par = off; off = align_up(off + (size_t)n * 4, 256);
    best_w = off; off = align_up(off + (size_t)n * 8, 256);
    best_e = off; off = align_up(off + (size_t)n * 8, 256);
    low = off; off = align_up(off + (size_t)n * 4, 256);
    votes = off; off = align_up(off + (size_t)n * 4, 256);
    work = off; off = align_up(off + (size_t)kOrientMaxRounds * 4, 256);
    partial = off; off = align_up(off + (size_t)kCenterLanes * 3 * 8, 256);
    center = off; off = align_up(off + 3 * 8, 256);
    total = off;
  }
};

__device__ __forceinline__ uint32_t load_word(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_word(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// O2 (a product commutes, so dot(i, j) and dot(j, i) are the same bits)
__device__ __forceinline__ double orient_dot(const float *__restrict__ nrm, uint32_t i, uint32_t j) {
  const float *a = nrm + (size_t)i * 3, *b = nrm + (size_t)j * 3;
  return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
}
// w = 1 - |dot| as a u64 whose unsigned order is w's (w is finite, and never -0.0)
__device__ __forceinline__ unsigned long long weight_code(double dot) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(1.0 - fabs(dot));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// O1: the entry of a row that names another vertex
__device__ __forceinline__ bool listed(int32_t j, uint32_t i, int n) { return j >= 0 && j < n && (uint32_t)j != i; }

__global__ void __launch_bounds__(kOrientThreads) orient_init_kernel(int n, uint32_t *__restrict__ snap, uint32_t *__restrict__ par,
                                                                     unsigned long long *__restrict__ best_w,
                                                                     unsigned long long *__restrict__ best_e, int32_t *__restrict__ low,
                                                                     int32_t *__restrict__ votes, uint32_t *__restrict__ work,
                                                                     int32_t *__restrict__ tree, int32_t *__restrict__ counts, int have_center,
                                                                     double cx, double cy, double cz, double *__restrict__ center) {
  const int64_t i = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (i == 0) {
    counts[0] = 0;
    counts[1] = 0;
    if (have_center) { center[0] = cx; center[1] = cy; center[2] = cz; }
  }
  if (i < kOrientMaxRounds) work[i] = 0;
  if (i >= n) return;
  snap[i] = (uint32_t)i;
  par[i] = (uint32_t)i;
  best_w[i] = kNoEdge;
  best_e[i] = kNoEdge;
  low[i] = n;
  votes[i] = 0;
  if (tree) { tree[2 * i] = -1; tree[2 * i + 1] = -1; }
}

__global__ void __launch_bounds__(kOrientThreads) orient_center_partial_kernel(const float *__restrict__ pts, int n, double *__restrict__ partial) {
  const int g = blockIdx.x * kOrientThreads + threadIdx.x;   // the grid is exactly kCenterLanes lanes
  double x = 0.0, y = 0.0, z = 0.0;
  for (int64_t i = g; i < n; i += kCenterLanes) {
    x = x + (double)pts[i * 3];
    y = y + (double)pts[i * 3 + 1];
    z = z + (double)pts[i * 3 + 2];
  }
  partial[g * 3] = x;
  partial[g * 3 + 1] = y;
  partial[g * 3 + 2] = z;
}

__global__ void __launch_bounds__(kCenterThreads) orient_center_kernel(const double *__restrict__ partial, int n, double *__restrict__ center) {
  __shared__ double sums[kCenterThreads][3];
  const int t = threadIdx.x;
  double x = 0.0, y = 0.0, z = 0.0;
  for (int a = 0; a < kCenterRun; a++) {
    const double *p = partial + (size_t)(t * kCenterRun + a) * 3;
    x = x + p[0];
    y = y + p[1];
    z = z + p[2];
  }
  sums[t][0] = x; sums[t][1] = y; sums[t][2] = z;
  __syncthreads();
  if (t != 0) return;
  x = 0.0; y = 0.0; z = 0.0;
  for (int a = 0; a < kCenterThreads; a++) {
    x = x + sums[a][0];
    y = y + sums[a][1];
    z = z + sums[a][2];
  }
  center[0] = x / (double)n;
  center[1] = y / (double)n;
  center[2] = z / (double)n;
}

// first pass of a round: the smallest weight leaving every component
__global__ void __launch_bounds__(kOrientThreads) orient_weight_kernel(const float *__restrict__ nrm, const int32_t *__restrict__ nbr, int n, int k,
                                                                       int round, const uint32_t *__restrict__ snap,
                                                                       unsigned long long *best_w, uint32_t *work) {
  if (round > 0 && work[round - 1] == 0) return;
  const int64_t t = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (t >= n) return;
  const uint32_t i = (uint32_t)t, ci = snap[i] & kIndexMask;
  unsigned long long mine = kNoEdge;
  for (int a = 0; a < k; a++) {
    const int32_t j = nbr[(size_t)i * k + a];
    if (!listed(j, i, n)) continue;
    const uint32_t cj = snap[j] & kIndexMask;
    if (cj == ci) continue;
    const unsigned long long code = weight_code(orient_dot(nrm, i, (uint32_t)j));
    // the other end's slot: it only falls during the launch, so one that is seen at or below the code already makes the
    // atomic a no-op.  (Offering to the other end in a launch of its own, after every component's own edges are in, leaves
    // hardly an atomic to send; measured, it was 3 % faster at 10^6 points and 4 % slower at 10^5: not kept.)
    if (code < __hip_atomic_load(best_w + cj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(best_w + cj, code);
    mine = code < mine ? code : mine;
  }
  if (mine != kNoEdge) atomicMin(best_w + ci, mine);
  // the round's flag: one lane of a wave that found an edge, and only while the flag still reads 0 (a store per vertex to
  // the one word was 4.4 of the call's 6.9 ms at 10^6 points: such stores go out to memory one by one)
  if (__ballot(mine != kNoEdge) != 0 && (uint32_t)t == (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)t) && load_word(work + round) == 0)
    store_word(work + round, 1u);
}

// second pass: among the edges of that weight, the smallest (lo, hi)
__global__ void __launch_bounds__(kOrientThreads) orient_edge_kernel(const float *__restrict__ nrm, const int32_t *__restrict__ nbr, int n, int k,
                                                                     int round, const uint32_t *__restrict__ snap,
                                                                     const unsigned long long *__restrict__ best_w, unsigned long long *best_e,
                                                                     const uint32_t *__restrict__ work) {
  if (work[round] == 0) return;
  const int64_t t = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (t >= n) return;
  const uint32_t i = (uint32_t)t, ci = snap[i] & kIndexMask;
  const unsigned long long wi = best_w[ci];
  unsigned long long mine = kNoEdge;
  for (int a = 0; a < k; a++) {
    const int32_t j = nbr[(size_t)i * k + a];
    if (!listed(j, i, n)) continue;
    const uint32_t cj = snap[j] & kIndexMask;
    if (cj == ci) continue;
    const unsigned long long code = weight_code(orient_dot(nrm, i, (uint32_t)j));
    const uint32_t lo = i < (uint32_t)j ? i : (uint32_t)j, hi = i < (uint32_t)j ? (uint32_t)j : i;
    const unsigned long long e = ((unsigned long long)lo << 32) | hi;
    if (code == best_w[cj]) atomicMin(best_e + cj, e);
    if (code == wi && e < mine) mine = e;
  }
  if (mine != kNoEdge) atomicMin(best_e + ci, mine);
}

// O4 on the chosen edges: one lane per live root
__global__ void __launch_bounds__(kOrientThreads) orient_hook_kernel(const float *__restrict__ nrm, int n, int round, const uint32_t *__restrict__ snap,
                                                                     const unsigned long long *__restrict__ best_e, uint32_t *__restrict__ par,
                                                                     int32_t *__restrict__ tree, const uint32_t *__restrict__ work) {
  if (work[round] == 0) return;
  const int64_t t = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (t >= n) return;
  const uint32_t r = (uint32_t)t;
  if ((snap[r] & kIndexMask) != r) return;
  const unsigned long long e = best_e[r];
  if (e == kNoEdge) return;
  const uint32_t lo = (uint32_t)(e >> 32), hi = (uint32_t)e;
  if (lo >= (uint32_t)n || hi >= (uint32_t)n) return;   // (cannot be: the slot holds an edge of the list)
  const uint32_t su = snap[lo], sv = snap[hi];
  const uint32_t ru = su & kIndexMask, rv = sv & kIndexMask;
  if ((ru != r && rv != r) || ru == rv) return;          // (cannot be: the edge leaves r's component)
  const uint32_t o = ru == r ? rv : ru;
  if (best_e[o] == e && r < o) return;                   // both chose this edge: the larger root goes under the smaller
  const uint32_t flip = orient_dot(nrm, lo, hi) < 0.0 ? kParity : 0u;
  par[r] = o | (((su ^ sv) & kParity) ^ flip);
  if (tree) { tree[2 * (size_t)r] = (int32_t)lo; tree[2 * (size_t)r + 1] = (int32_t)hi; }
}

__global__ void __launch_bounds__(kOrientThreads) orient_compress_kernel(int n, int round, uint32_t *__restrict__ snap, uint32_t *par,
                                                                         unsigned long long *__restrict__ best_w,
                                                                         unsigned long long *__restrict__ best_e, const uint32_t *__restrict__ work) {
  if (work[round] == 0) return;
  const int64_t t = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (t >= n) return;
  best_w[t] = kNoEdge;
  best_e[t] = kNoEdge;
  const uint32_t s = snap[t];
  uint32_t x = s & kIndexMask, p = s & kParity;
  for (int step = 0; step < n; step++) {
    const uint32_t pw = load_word(par + x), px = pw & kIndexMask;
    if (px == x) break;
    const uint32_t gw = load_word(par + px), gx = gw & kIndexMask;
    if (gx != px) store_word(par + x, gx | ((pw ^ gw) & kParity));
    p ^= pw & kParity;
    x = px;
  }
  snap[t] = x | p;
}

// O4's m: the smallest member of every component, at its root
__global__ void __launch_bounds__(kOrientThreads) orient_label_kernel(int n, const uint32_t *__restrict__ snap, int32_t *low) {
  const int64_t t = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (t >= n) return;
  const uint32_t r = snap[t] & kIndexMask;
  // a wave whose lanes share a root sends one atomic, from its first lane (the smallest index)
  const uint32_t r0 = __builtin_amdgcn_readfirstlane(r), t0 = __builtin_amdgcn_readfirstlane((uint32_t)t);
  if (__ballot(r != r0) == 0) {
    if ((uint32_t)t == t0) atomicMin(low + r, (int32_t)t);
  } else {
    atomicMin(low + r, (int32_t)t);
  }
}

// O5
__global__ void __launch_bounds__(kOrientThreads) orient_vote_kernel(const float *__restrict__ pts, const float *__restrict__ nrm, int n,
                                                                     const uint32_t *__restrict__ snap, const int32_t *__restrict__ low,
                                                                     const double *__restrict__ center, int32_t *votes) {
  const int64_t t = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (t >= n) return;
  const uint32_t s = snap[t], r = s & kIndexMask;
  const uint32_t rel = (s ^ snap[low[r]]) & kParity;
  const double dx = (double)pts[t * 3] - center[0], dy = (double)pts[t * 3 + 1] - center[1], dz = (double)pts[t * 3 + 2] - center[2];
  const double dd = ((double)nrm[t * 3] * dx + (double)nrm[t * 3 + 1] * dy) + (double)nrm[t * 3 + 2] * dz;
  int v = dd > 0.0 ? 1 : (dd < 0.0 ? -1 : 0);   // (negating n negates every product and sum exactly)
  if (rel) v = -v;
  const uint32_t r0 = __builtin_amdgcn_readfirstlane(r), t0 = __builtin_amdgcn_readfirstlane((uint32_t)t);
  if (__ballot(r != r0) == 0) {
    const int sum = __popcll(__ballot(v > 0)) - __popcll(__ballot(v < 0));
    if ((uint32_t)t == t0 && sum != 0) atomicAdd(votes + r, sum);
  } else if (v != 0) {
    atomicAdd(votes + r, v);
  }
}

// O6
__global__ void __launch_bounds__(kOrientThreads) orient_output_kernel(const float *__restrict__ nrm, int n, int majority,
                                                                       const uint32_t *__restrict__ snap, const uint32_t *__restrict__ par,
                                                                       const int32_t *__restrict__ low, const int32_t *__restrict__ votes,
                                                                       float *__restrict__ out_normals, uint8_t *__restrict__ out_flip,
                                                                       int32_t *__restrict__ out_label, int32_t *counts) {
  const int64_t t = (int64_t)blockIdx.x * kOrientThreads + threadIdx.x;
  if (t >= n) return;
  const uint32_t s = snap[t], r = s & kIndexMask;
  const int32_t m = low[r];
  uint32_t flip = (s ^ snap[m]) & kParity;
  if (majority && votes[r] < 0) flip ^= kParity;
  const uint32_t sign = flip ? 0x80000000u : 0u;
#pragma unroll
  for (int c = 0; c < 3; c++) out_normals[t * 3 + c] = __uint_as_float(__float_as_uint(nrm[t * 3 + c]) ^ sign);
  if (out_flip) out_flip[t] = flip ? 1 : 0;
  if (out_label) out_label[t] = m;
  const int roots = __popcll(__ballot((int64_t)m == t));
  const int hooked = __popcll(__ballot((par[t] & kIndexMask) != (uint32_t)t));
  if ((uint32_t)t == __builtin_amdgcn_readfirstlane((uint32_t)t)) {
    if (roots) atomicAdd(counts, roots);
    if (hooked) atomicAdd(counts + 1, hooked);
  }
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_cloud_orient_workspace_bytes(int32_t n, int32_t k) {
  (void)k;   // (the list is read in place: nothing in the workspace is sized by k)
  return OrientLayout(n > 0 ? n : 1).total;
}

extern "C" int scorp_cloud_orient_normals(const float *points, const float *normals, const int32_t *neighbors, int32_t n, int32_t k,
                                          const double *center, int32_t component_sign, float *out_normals, uint8_t *out_flip,
                                          int32_t *out_label, int32_t *out_tree, int32_t *out_counts, void *workspace,
                                          size_t workspace_bytes, scorp_stream_t stream) {
  const char *who = "cloud_orient_normals";
  if (n < 1) { set_error("%s: empty cloud", who); return SCORP_ERR_INVALID; }
  if (n > (1 << 30)) { set_error("%s: more than 2^30 points", who); return SCORP_ERR_INVALID; }
  if (k < 1 || k > kOrientMaxK) { set_error("%s: k must be in [1, %d]", who, kOrientMaxK); return SCORP_ERR_INVALID; }
  if (component_sign != SCORP_ORIENT_MAJORITY_AWAY && component_sign != SCORP_ORIENT_FIRST) {
    set_error("%s: unknown component_sign %d", who, component_sign); return SCORP_ERR_INVALID;
  }
  if (!points || !normals || !neighbors || !out_normals || !out_counts) { set_error("%s: NULL argument", who); return SCORP_ERR_INVALID; }
  if (center && !(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]))) {
    set_error("%s: center must be finite", who); return SCORP_ERR_INVALID;
  }
  const OrientLayout L(n);
  if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace & 255)) {
    set_error("%s: workspace NULL, too small or not 256-byte aligned (%zu < %zu)", who, workspace_bytes, L.total);
    return SCORP_ERR_INVALID;
  }
  char *w = (char *)workspace;
  uint32_t *snap = (uint32_t *)(w + L.snap), *par = (uint32_t *)(w + L.par), *work = (uint32_t *)(w + L.work);
  unsigned long long *best_w = (unsigned long long *)(w + L.best_w), *best_e = (unsigned long long *)(w + L.best_e);
  int32_t *low = (int32_t *)(w + L.low), *votes = (int32_t *)(w + L.votes);
  double *partial = (double *)(w + L.partial), *c = (double *)(w + L.center);
  hipStream_t s = (hipStream_t)stream;
  const bool majority = component_sign == SCORP_ORIENT_MAJORITY_AWAY;
  const unsigned grid = (unsigned)(((int64_t)n + kOrientThreads - 1) / kOrientThreads);
  const unsigned init_grid = grid > 0 ? grid : 1;

  orient_init_kernel<<<init_grid, kOrientThreads, 0, s>>>(n, snap, par, best_w, best_e, low, votes, work, out_tree, out_counts,
                                                           center ? 1 : 0, center ? center[0] : 0.0, center ? center[1] : 0.0,
                                                           center ? center[2] : 0.0, c);
  SCORP_KERNEL_CHECK("orient_init", 0, s);
  if (majority && !center) {
    orient_center_partial_kernel<<<kCenterLanes / kOrientThreads, kOrientThreads, 0, s>>>(points, n, partial);
    SCORP_KERNEL_CHECK("orient_center_partial", 0, s);
    orient_center_kernel<<<1, kCenterThreads, 0, s>>>(partial, n, c);
    SCORP_KERNEL_CHECK("orient_center", 0, s);
  }
  int rounds = 1;   // ceil(log2 n) + 1
  while ((1ll << (rounds - 1)) < n) rounds++;
  for (int round = 0; round < rounds; round++) {
    orient_weight_kernel<<<grid, kOrientThreads, 0, s>>>(normals, neighbors, n, k, round, snap, best_w, work);
    SCORP_KERNEL_CHECK("orient_weight", 0, s);
    orient_edge_kernel<<<grid, kOrientThreads, 0, s>>>(normals, neighbors, n, k, round, snap, best_w, best_e, work);
    SCORP_KERNEL_CHECK("orient_edge", 0, s);
    orient_hook_kernel<<<grid, kOrientThreads, 0, s>>>(normals, n, round, snap, best_e, par, out_tree, work);
    SCORP_KERNEL_CHECK("orient_hook", 0, s);
    orient_compress_kernel<<<grid, kOrientThreads, 0, s>>>(n, round, snap, par, best_w, best_e, work);
    SCORP_KERNEL_CHECK("orient_compress", 0, s);
  }
  orient_label_kernel<<<grid, kOrientThreads, 0, s>>>(n, snap, low);
  SCORP_KERNEL_CHECK("orient_label", 0, s);
  if (majority) {
    orient_vote_kernel<<<grid, kOrientThreads, 0, s>>>(points, normals, n, snap, low, c, votes);
    SCORP_KERNEL_CHECK("orient_vote", 0, s);
  }
  orient_output_kernel<<<grid, kOrientThreads, 0, s>>>(normals, n, majority ? 1 : 0, snap, par, low, votes, out_normals, out_flip, out_label,
                                                       out_counts);
  SCORP_KERNEL_CHECK("orient_output", 0, s);
  return SCORP_OK;
}
