// union_find.hpp - the lock-free union-find mesh_cluster.hip (triangles over shared edges) and cloud_filter.hip (DBSCAN's
// core points) share.  A root is only ever hooked under a SMALLER index, so the root of a finished component is its
// smallest member: labels and numbering do not depend on the execution order.  Nothing waits on another lane's progress:
// no locks, no spinning on a value someone else must write.
#pragma once
#include "common.hpp"

namespace scorp {
namespace {

// parent[] while other lanes hook roots: an agent-scope relaxed atomic load.  A plain load may be served from a line of the
// CU's vector cache that another CU's compare-and-swap has rewritten since, for as long as the loop runs.  (A stale value
// would still be a former parent - the index itself - and the compare-and-swap in unite() is what decides; the fresh load
// saves the retries.)
__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x, halving the path on the way.  The only write is atomicMin(&parent[x], grandparent): parent[x] goes
// down to another ancestor of x and can never rise, so it cannot undo a hook that lands at the same time (a plain store of
// the grandparent could: it might overwrite the smaller parent a concurrent hook has just given x).  A root has
// parent[x] == x and is not written here.
__device__ __forceinline__ int32_t find_root(int32_t *parent, int32_t x) {
  int32_t p = load_parent(parent, x);
  while (p != x) {
    const int32_t g = load_parent(parent, p);
    if (g != p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// Joins the trees of a and b.  Terminates: parent[hi] == hi holds only while hi is a root, and parent[x] <= x always.  A
// failed compare-and-swap returns the parent hi has by now, old < hi, and the loop goes on from (old, lo): every retry
// replaces one of the two indices by a strictly smaller one, and indices are bounded below by 0.  The walk inside find_root
// descends strictly as well.  No step depends on what another lane does next.
__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}

// The root above x once every hook has landed (a later launch: plain loads).  p < x while x is not a root, and an entry
// outside [0, x] - an array nobody filled - ends the walk.
__device__ __forceinline__ int32_t settled_root(const int32_t *__restrict__ parent, int32_t x) {
  int32_t p = parent[x];
  while (p != x && p >= 0 && p < x) {
    x = p;
    p = parent[x];
  }
  return x;
}

}  // namespace
}  // namespace scorp
