// icp_search.hpp - what icp.hip (both ICP estimators and the normal estimation) and mesh_distance.hip (point-to-mesh
// distance, nearest point of a cloud) share: the uniform grid over the target, the stable radix sort that orders the
// target by cell and the source or the queries by Morton code, the exact outward ring walk over the grid (fp32 for the
// point searches, float64 for the mesh's) with the one loop over a run of cells (icp_cell_run) and the one k-best list
// (KBest) that the kernels put inside it, the workspace check and the host calls that build all of it once per call.
// cloud_filter.hip and cloud_fpfh.hip include it through cloud_search.hpp.  Everything is in an unnamed namespace: each
// includer gets its own copy of the kernels.
#pragma once
#include <cmath>
#include <vector>

#include "common.hpp"

namespace scorp {
namespace {

constexpr int kIcpThreads = 256;
constexpr int kIcpPerThread = 4;
constexpr int kIcpChunk = kIcpThreads * kIcpPerThread;   // source points per pass block
constexpr int kIcpPollEvery = 4;                         // iterations between two reads of the active flags
constexpr int kRadixTile = 256;                          // keys per radix-sort block
constexpr int kMaxGridDim = 1024;

struct IcpGrid {
  double ct[3];      // fixed centre: the target's bounding-box centre (every coordinate below is relative to it)
  float lo[3];       // grid origin (relative)
  float h, inv_h;    // cell edge
  int dims[3];
  int ncells;
  float tlo[3], thi[3];   // bounding boxes of the target and the source (absolute)
  float slo[3], shi[3];
};

size_t icp_cell_cap(int64_t nt) { return (size_t)(nt * 2 > 64 ? nt * 2 : 64); }

// The workspace of one call: `row` doubles per (pass block, init) partial row.  ns = 0: no source (the normal estimation).
struct IcpLayout {
  size_t grid, keys0, keys1, vals0, vals1, hist, cell_start, tq, src, rows, active, total;
  int64_t nmax, tiles;
  IcpLayout(int64_t ns, int64_t nt, int64_t ni, int row) {
    nmax = ns > nt ? ns : nt;
    if (nmax < 1) nmax = 1;
    tiles = (nmax + kRadixTile - 1) / kRadixTile;
    const int64_t nblk = (ns + kIcpChunk - 1) / kIcpChunk;
    size_t off = 0;
    grid = off; off = align_up(off + sizeof(IcpGrid), 256);
    keys0 = off; off = align_up(off + (size_t)nmax * 4, 256);
    keys1 = off; off = align_up(off + (size_t)nmax * 4, 256);
    vals0 = off; off = align_up(off + (size_t)nmax * 4, 256);
    vals1 = off; off = align_up(off + (size_t)nmax * 4, 256);
    hist = off; off = align_up(off + (size_t)tiles * 256 * 4, 256);
    cell_start = off; off = align_up(off + (icp_cell_cap(nt) + 1) * 4, 256);
    tq = off; off = align_up(off + (size_t)(nt > 0 ? nt : 1) * 16, 256);
    src = off; off = align_up(off + (size_t)(ns > 0 ? ns : 1) * 16, 256);
    rows = off; off = align_up(off + (size_t)(nblk > 0 ? nblk : 1) * (size_t)(ni > 0 ? ni : 1) * row * 8, 256);
    active = off; off = align_up(off + (size_t)(ni > 0 ? ni : 1) * 4, 256);
    total = off;
  }
};

// ---- set-up: bounding boxes, grid, sorts ----

// min / max per axis of n points (one workgroup; exact, so order-free)
__global__ void __launch_bounds__(1024) icp_bbox_kernel(const float *__restrict__ p, int n, float *lo, float *hi) {
  __shared__ float s[6][1024];
  float a[6] = {3.4e38f, 3.4e38f, 3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f};
  for (int i = threadIdx.x; i < n; i += 1024) {
    for (int d = 0; d < 3; d++) {
      const float v = p[(size_t)i * 3 + d];
      a[d] = fminf(a[d], v);
      a[3 + d] = fmaxf(a[3 + d], v);
    }
  }
  for (int d = 0; d < 6; d++) s[d][threadIdx.x] = a[d];
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int d = 0; d < 6; d++)
        s[d][threadIdx.x] = d < 3 ? fminf(s[d][threadIdx.x], s[d][threadIdx.x + w]) : fmaxf(s[d][threadIdx.x], s[d][threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    lo[threadIdx.x] = s[threadIdx.x][0];
    hi[threadIdx.x] = s[3 + threadIdx.x][0];
  }
}

// Cell edge from the density: h = cbrt(V / nt) over the (slightly padded) target box, grown until the grid has at most
// `cap` cells; a flat or degenerate box gets extents of at least 1/1024 of its largest one.
__global__ void icp_grid_setup_kernel(IcpGrid *g, int nt, int cap) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double ext[3], maxe = 0.0;
  for (int d = 0; d < 3; d++) {
    g->ct[d] = 0.5 * ((double)g->tlo[d] + (double)g->thi[d]);
    ext[d] = (double)g->thi[d] - (double)g->tlo[d];
    maxe = fmax(maxe, ext[d]);
  }
  const double pad = maxe > 0.0 ? 1e-5 * maxe : 1e-6 * fmax(1.0, fabs(g->ct[0]) + fabs(g->ct[1]) + fabs(g->ct[2]));
  double vol = 1.0;
  for (int d = 0; d < 3; d++) {
    ext[d] += 2.0 * pad;
    vol *= fmax(ext[d], (maxe + 2.0 * pad) / kMaxGridDim);
  }
  double h = fmax(cbrt(vol / (nt > 0 ? nt : 1)), (maxe + 2.0 * pad) / kMaxGridDim);
  if (!(h > 0.0) || !isfinite(h)) h = 1.0;   // (non-finite input: any finite grid ends the loop below)
  int dims[3];
  for (int grow = 0; grow < 200; grow++) {
    long long cells = 1;
    for (int d = 0; d < 3; d++) {
      const double n = floor(ext[d] / h) + 1.0;
      dims[d] = n >= 1.0 && n < kMaxGridDim ? (int)n : (n >= kMaxGridDim ? kMaxGridDim : 1);
      cells *= dims[d];
    }
    if (cells <= cap) break;
    h *= 1.25;
    if (grow == 199) dims[0] = dims[1] = dims[2] = 1;
  }
  for (int d = 0; d < 3; d++) {
    g->lo[d] = (float)((double)g->tlo[d] - g->ct[d] - pad);
    g->dims[d] = dims[d];
  }
  g->h = (float)h;
  g->inv_h = (float)(1.0 / h);
  g->ncells = dims[0] * dims[1] * dims[2];
}

__device__ __forceinline__ int icp_cell_axis(float v, float lo, float inv_h, int dim) {
  const int c = (int)floorf((v - lo) * inv_h);
  return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

// target: key = raster cell id, val = index
__global__ void __launch_bounds__(256) icp_target_keys_kernel(const float *__restrict__ q, int nt, const IcpGrid *__restrict__ g,
                                                              uint32_t *keys, uint32_t *vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  int c[3];
  for (int d = 0; d < 3; d++) {
    const float v = (float)((double)q[(size_t)i * 3 + d] - g->ct[d]);
    c[d] = icp_cell_axis(v, g->lo[d], g->inv_h, g->dims[d]);
  }
  keys[i] = (uint32_t)((c[2] * g->dims[1] + c[1]) * g->dims[0] + c[0]);
  vals[i] = (uint32_t)i;
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// source: key = 30-bit Morton code over the source's bounding box, val = index
__global__ void __launch_bounds__(256) icp_source_keys_kernel(const float *__restrict__ p, int ns, const IcpGrid *__restrict__ g,
                                                              uint32_t *keys, uint32_t *vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  float e = 0.0f;
  for (int d = 0; d < 3; d++) e = fmaxf(e, g->shi[d] - g->slo[d]);
  const float s = e > 0.0f ? 1023.0f / e : 0.0f;
  uint32_t m = 0;
  for (int d = 0; d < 3; d++) {
    const float v = fminf(fmaxf((p[(size_t)i * 3 + d] - g->slo[d]) * s, 0.0f), 1023.0f);
    m |= spread10((uint32_t)v) << d;
  }
  keys[i] = m;
  vals[i] = (uint32_t)i;
}

// One stable LSD pass on the 8-bit digit at `shift`: per tile of 256 keys a digit histogram (digit-major, so that one
// exclusive scan gives every (digit, tile) its output offset), then a stable scatter (rank inside the tile = the earlier
// keys of the tile with the same digit).  Integer counts only: the order is fully determined.
__global__ void __launch_bounds__(kRadixTile) icp_radix_hist_kernel(const uint32_t *__restrict__ keys, int n, int shift,
                                                                    int tiles, uint32_t *hist) {
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * kRadixTile + threadIdx.x;
  if (i < n) atomicAdd(&cnt[(keys[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[(size_t)threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of n u32 in place (one workgroup: a serial run per thread, then a scan of the run totals)
__global__ void __launch_bounds__(1024) icp_scan_kernel(uint32_t *a, int64_t n) {
  __shared__ uint32_t tot[1024];
  const int64_t per = (n + 1023) / 1024, b = threadIdx.x * per, e = b + per < n ? b + per : n;
  uint32_t s = 0;
  for (int64_t i = b; i < e; i++) s += a[i];
  tot[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = 0; t < 1024; t++) { const uint32_t v = tot[t]; tot[t] = run; run += v; }
  }
  __syncthreads();
  uint32_t run = tot[threadIdx.x];
  for (int64_t i = b; i < e; i++) { const uint32_t v = a[i]; a[i] = run; run += v; }
}

__global__ void __launch_bounds__(kRadixTile) icp_radix_scatter_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                       int n, int shift, int tiles, const uint32_t *__restrict__ offs,
                                                                       uint32_t *okeys, uint32_t *ovals) {
  __shared__ uint32_t dig[kRadixTile];
  const int i = blockIdx.x * kRadixTile + threadIdx.x;
  const uint32_t k = i < n ? keys[i] : 0u;
  const uint32_t d = i < n ? (k >> shift) & 255u : 256u;
  dig[threadIdx.x] = d;
  __syncthreads();
  if (i >= n) return;
  uint32_t rank = 0;
  for (int s = 0; s < (int)threadIdx.x; s++) rank += dig[s] == d;
  const uint32_t o = offs[(size_t)d * tiles + blockIdx.x] + rank;
  okeys[o] = k;
  ovals[o] = vals[i];
}

// cell_start[c] = first sorted position whose cell is >= c, for c in [0, ncells]
__global__ void __launch_bounds__(256) icp_cell_start_kernel(const uint32_t *__restrict__ keys, int nt, const IcpGrid *__restrict__ g,
                                                             uint32_t *cell_start) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nt) return;
  const int ncells = g->ncells;
  const int prev = i == 0 ? -1 : (int)keys[i - 1];
  const int cur = i == nt ? ncells : (int)keys[i];
  for (int c = prev + 1; c <= cur; c++) cell_start[c] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) icp_gather_target_kernel(const float *__restrict__ q, const uint32_t *__restrict__ order, int nt,
                                                                const IcpGrid *__restrict__ g, float4 *tq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  const uint32_t j = order[i];
  const float *s = q + (size_t)j * 3;
  tq[i] = make_float4((float)((double)s[0] - g->ct[0]), (float)((double)s[1] - g->ct[1]), (float)((double)s[2] - g->ct[2]),
                      __uint_as_float(j));
}

__global__ void __launch_bounds__(256) icp_gather_source_kernel(const float *__restrict__ p, const uint32_t *__restrict__ order, int ns,
                                                                float4 *sp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  const float *s = p + (size_t)order[i] * 3;
  sp[i] = make_float4(s[0], s[1], s[2], 0.0f);
}

__global__ void icp_init_kernel(const double *__restrict__ inits, int ni, double *T, double *fitness, double *rmse, int32_t *iters,
                                int32_t *active) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ni) return;
  for (int e = 0; e < 16; e++) T[(size_t)j * 16 + e] = inits[(size_t)j * 16 + e];
  fitness[j] = 0.0;
  rmse[j] = 0.0;
  iters[j] = 0;
  active[j] = 1;
}

// ---- the search ----

// The outward walk every search shares: rings of cells at Chebyshev distance k around cell (cx, cy, cz), clipped to the
// grid; visit(ca, cb) takes the cells ca..cb of one grid row (cell ids are raster order, x fastest, so their entries are
// one contiguous run).  After ring k, everything outside its box is at least lb away: the walk ends when lb^2 exceeds
// reach() - the d^2 that still matters to the caller - or nothing is left outside the box.  F: float for the point
// searches (icp_nearest, the normals' k nearest), double for the mesh distance; `none` is F's "no side left".
template <class F, class Visit, class Reach>
__device__ __forceinline__ void icp_ring_walk(F x, F y, F z, int cx, int cy, int cz, F lx, F ly, F lz, F h, int dx, int dy, int dz,
                                              Visit visit, Reach reach) {
  const F none = sizeof(F) == sizeof(float) ? (F)3.4e38f : (F)__builtin_inf();
  for (int k = 0;; k++) {
    const int z0 = max(cz - k, 0), z1 = min(cz + k, dz - 1), y0 = max(cy - k, 0), y1 = min(cy + k, dy - 1);
    const int x0 = max(cx - k, 0), x1 = min(cx + k, dx - 1);
    for (int iz = z0; iz <= z1; iz++) {
      for (int iy = y0; iy <= y1; iy++) {
        const int row = (iz * dy + iy) * dx;
        if (iz == cz - k || iz == cz + k || iy == cy - k || iy == cy + k) {   // a face of the ring: the whole row
          if (x0 <= x1) visit(row + x0, row + x1);
        } else {                                                                 // inside: the row's two ends
          if (cx - k >= 0) visit(row + cx - k, row + cx - k);
          if (cx + k < dx) visit(row + cx + k, row + cx + k);
        }
      }
    }
    // what lies outside ring k's box is at least this far away (sides past the grid hold no points)
    F lb = none;
    if (cx - k > 0) lb = fmin(lb, x - (lx + (cx - k) * h));
    if (cx + k < dx - 1) lb = fmin(lb, (lx + (cx + k + 1) * h) - x);
    if (cy - k > 0) lb = fmin(lb, y - (ly + (cy - k) * h));
    if (cy + k < dy - 1) lb = fmin(lb, (ly + (cy + k + 1) * h) - y);
    if (cz - k > 0) lb = fmin(lb, z - (lz + (cz - k) * h));
    if (cz + k < dz - 1) lb = fmin(lb, (lz + (cz + k + 1) * h) - z);
    if (lb >= none) break;
    lb = fmax(lb, (F)0);
    if (!(lb * lb <= reach())) break;   // (a NaN query ends here too)
  }
}

// The body of every visit(ca, cb): cell ids are raster order (x fastest), so the entries of the cells ca..cb of one grid
// row are one contiguous run of sorted positions; body(t) takes each.
template <class Body>
__device__ __forceinline__ void icp_cell_run(const uint32_t *cell_start, int ca, int cb, Body body) {
  const uint32_t e = cell_start[cb + 1];
  for (uint32_t t = cell_start[ca]; t < e; t++) body(t);
}

// What a walk from a filed point needs of the grid, and the point's own cell (inside the grid: icp_cell_axis clamps as the
// filing did).  cloud_search.hpp's CloudWalk adds the widened reach; icp_nearest and the mesh query start from points that
// were never filed and set their walks up themselves.
struct IcpWalk {
  float x, y, z, lx, ly, lz, h;
  int cx, cy, cz, dx, dy, dz;
  __device__ __forceinline__ IcpWalk(const float4 &me, const IcpGrid *__restrict__ g) {
    x = me.x; y = me.y; z = me.z;
    lx = g->lo[0]; ly = g->lo[1]; lz = g->lo[2]; h = g->h;
    dx = g->dims[0]; dy = g->dims[1]; dz = g->dims[2];
    const float ih = g->inv_h;
    cx = icp_cell_axis(x, lx, ih, dx); cy = icp_cell_axis(y, ly, ih, dy); cz = icp_cell_axis(z, lz, ih, dz);
  }
  template <class Visit, class Reach>
  __device__ __forceinline__ void run(Visit visit, Reach reach) const {
    icp_ring_walk(x, y, z, cx, cy, cz, lx, ly, lz, h, dx, dy, dz, visit, reach);
  }
};

// The k best (d^2, index) a lane has seen, sorted ascending by that pair, in the lane's column of two LDS arrays the
// kernel owns (a runtime-indexed per-thread array would go to scratch): the one tie rule of the normals' list, the FPFH
// search (F1) and the cloud kNN (R3; cloud_knn_kernel keeps the same statements on locals of its own, see there).  D is the kernel's d^2 type, float or double; the list only compares and moves, so
// it holds nothing a contraction setting could change.  Workgroups of kKBestLanes lanes.
constexpr int kKBestLanes = 64;

template <class D>
struct KBest {
  D (*nd)[kKBestLanes];
  uint32_t (*ni)[kKBestLanes];
  int lane, k, cnt;
  D kth_d2;          // d^2 of the k-th best once the list is full; until then the kernel's `none`
  uint32_t kth_id;
  // none: what kth() gives while the list is not full (the reach of a walk that must not end yet)
  __device__ __forceinline__ KBest(D (*nd_)[kKBestLanes], uint32_t (*ni_)[kKBestLanes], int lane_, int k_, D none)
      : nd(nd_), ni(ni_), lane(lane_), k(k_), cnt(0), kth_d2(none), kth_id(0xFFFFFFFFu) {}
  // a candidate enters when the list is not full or it is below the last entry, ties on d^2 by the lower index
  // (cnt >= k is full(): cnt never passes k.  Written as cnt == k here, the compiler puts k for cnt on the path that
  // skips and then carries the count in two registers in icp_normals_kernel, with a move more on every insertion.)
  __device__ __forceinline__ void offer(D d2, uint32_t id) {
    if (cnt >= k && !(d2 < kth_d2 || (d2 == kth_d2 && id < kth_id))) return;
    int pos = cnt < k ? cnt : k - 1;   // the free slot, or the last entry, which leaves
    while (pos > 0) {
      const D pd = nd[pos - 1][lane];
      const uint32_t pi = ni[pos - 1][lane];
      if (!(pd > d2 || (pd == d2 && pi > id))) break;
      nd[pos][lane] = pd;
      ni[pos][lane] = pi;
      pos--;
    }
    nd[pos][lane] = d2;
    ni[pos][lane] = id;
    if (cnt < k) cnt++;
    if (cnt == k) { kth_d2 = nd[k - 1][lane]; kth_id = ni[k - 1][lane]; }
  }
  __device__ __forceinline__ bool full() const { return cnt == k; }
  __device__ __forceinline__ D kth() const { return kth_d2; }
  __device__ __forceinline__ int count() const { return cnt; }
  __device__ __forceinline__ D d2(int a) const { return nd[a][lane]; }
  __device__ __forceinline__ uint32_t id(int a) const { return ni[a][lane]; }
  // the list's indices into row `row` of out [., width], padded with -1
  __device__ __forceinline__ void write_neighbors(int32_t *out, size_t row, int width) const {
    for (int a = 0; a < width; a++) out[row * width + a] = a < cnt ? (int32_t)ni[a][lane] : -1;
  }
};

// Original index of the nearest target point to x (relative fp32) with d^2 <= best on entry, -1 if none; ties go to the
// lower original index.  icp_ring_walk around x's cell (clamped to one cell outside the grid), until the distance from x
// to everything outside ring k's box exceeds the best d^2 so far, or nothing is left outside it.
__device__ __forceinline__ int icp_nearest(float x, float y, float z, float best, const IcpGrid *__restrict__ g,
                                           const uint32_t *__restrict__ cell_start, const float4 *__restrict__ tq) {
  const float lx = g->lo[0], ly = g->lo[1], lz = g->lo[2], h = g->h, ih = g->inv_h;
  const int dx = g->dims[0], dy = g->dims[1], dz = g->dims[2];
  {  // distance to the grid box: nothing can be closer than that
    const float ex = fmaxf(fmaxf(lx - x, x - (lx + dx * h)), 0.0f), ey = fmaxf(fmaxf(ly - y, y - (ly + dy * h)), 0.0f),
                ez = fmaxf(fmaxf(lz - z, z - (lz + dz * h)), 0.0f);
    if (!(ex * ex + ey * ey + ez * ez <= best)) return -1;
  }
  const int cx = (int)floorf(fminf(fmaxf((x - lx) * ih, -1.0f), (float)dx));
  const int cy = (int)floorf(fminf(fmaxf((y - ly) * ih, -1.0f), (float)dy));
  const int cz = (int)floorf(fminf(fmaxf((z - lz) * ih, -1.0f), (float)dz));
  uint32_t bidx = 0xFFFFFFFFu;
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) {
      const float4 q = tq[t];
      const float ux = q.x - x, uy = q.y - y, uz = q.z - z;
      const float d2 = __builtin_fmaf(ux, ux, __builtin_fmaf(uy, uy, uz * uz));
      const uint32_t id = __float_as_uint(q.w);
      if (d2 < best || (d2 == best && id < bidx)) { best = d2; bidx = id; }
    });
  };
  icp_ring_walk(x, y, z, cx, cy, cz, lx, ly, lz, h, dx, dy, dz, visit, [&]() { return best; });
  return bidx == 0xFFFFFFFFu ? -1 : (int)bidx;
}

// ---- host ----

int radix_sort(uint32_t *&keys, uint32_t *&vals, uint32_t *&keys_alt, uint32_t *&vals_alt, int n, int bits, int64_t tiles_cap,
               uint32_t *hist, hipStream_t stream) {
  const int tiles = (n + kRadixTile - 1) / kRadixTile;
  if (tiles > tiles_cap) { set_error("icp: radix sort tiles"); return SCORP_ERR_INVALID; }
  for (int shift = 0; shift < bits; shift += 8) {
    icp_radix_hist_kernel<<<tiles, kRadixTile, 0, stream>>>(keys, n, shift, tiles, hist);
    SCORP_KERNEL_CHECK("icp_radix_hist", 0, stream);
    icp_scan_kernel<<<1, 1024, 0, stream>>>(hist, (int64_t)tiles * 256);
    SCORP_KERNEL_CHECK("icp_scan", 0, stream);
    icp_radix_scatter_kernel<<<tiles, kRadixTile, 0, stream>>>(keys, vals, n, shift, tiles, hist, keys_alt, vals_alt);
    SCORP_KERNEL_CHECK("icp_radix_scatter", 0, stream);
    uint32_t *tk = keys; keys = keys_alt; keys_alt = tk;
    uint32_t *tv = vals; vals = vals_alt; vals_alt = tv;
  }
  return SCORP_OK;
}

// The pointers of a workspace laid out by L.
struct IcpWorkspace {
  IcpGrid *g;
  uint32_t *k0, *k1, *v0, *v1, *hist, *cell_start;
  float4 *tq, *sp;
  double *rows;
  int32_t *active;
  IcpWorkspace(void *workspace, const IcpLayout &L) {
    char *w = (char *)workspace;
    g = (IcpGrid *)(w + L.grid);
    k0 = (uint32_t *)(w + L.keys0); k1 = (uint32_t *)(w + L.keys1);
    v0 = (uint32_t *)(w + L.vals0); v1 = (uint32_t *)(w + L.vals1);
    hist = (uint32_t *)(w + L.hist); cell_start = (uint32_t *)(w + L.cell_start);
    tq = (float4 *)(w + L.tq); sp = (float4 *)(w + L.src);
    rows = (double *)(w + L.rows);
    active = (int32_t *)(w + L.active);
  }
};

// The target's side of a call: its bounding box, the grid, the points sorted by cell (W.tq) and W.cell_start.
int icp_build_target(const float *target, int nt, const IcpLayout &L, const IcpWorkspace &W, hipStream_t stream) {
  const int cap = (int)icp_cell_cap(nt);
  icp_bbox_kernel<<<1, 1024, 0, stream>>>(target, nt, W.g->tlo, W.g->thi);
  SCORP_KERNEL_CHECK("icp_bbox", 0, stream);
  icp_grid_setup_kernel<<<1, 64, 0, stream>>>(W.g, nt, cap);
  SCORP_KERNEL_CHECK("icp_grid_setup", 0, stream);
  icp_target_keys_kernel<<<(nt + 255) / 256, 256, 0, stream>>>(target, nt, W.g, W.k0, W.v0);
  SCORP_KERNEL_CHECK("icp_target_keys", 0, stream);
  int bits = 8;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)cap) bits += 8;
  uint32_t *a = W.k0, *b = W.v0, *c = W.k1, *d = W.v1;
  if (int e = radix_sort(a, b, c, d, nt, bits, L.tiles, W.hist, stream)) return e;
  icp_cell_start_kernel<<<(nt + 1 + 255) / 256, 256, 0, stream>>>(a, nt, W.g, W.cell_start);
  SCORP_KERNEL_CHECK("icp_cell_start", 0, stream);
  icp_gather_target_kernel<<<(nt + 255) / 256, 256, 0, stream>>>(target, b, nt, W.g, W.tq);
  SCORP_KERNEL_CHECK("icp_gather_target", 0, stream);
  return SCORP_OK;
}

// The Morton order of n points (an ICP source, the queries of a distance call): their bounding box into g->slo / shi, the
// keys, the sort over the two buffer pairs.  *order: whichever of v0 / v1 holds the sorted original indices.
int icp_sort_source(const float *points, int n, IcpGrid *g, uint32_t *k0, uint32_t *v0, uint32_t *k1, uint32_t *v1, uint32_t *hist,
                    int64_t tiles, hipStream_t stream, const uint32_t **order) {
  icp_bbox_kernel<<<1, 1024, 0, stream>>>(points, n, g->slo, g->shi);
  SCORP_KERNEL_CHECK("icp_bbox", 0, stream);
  icp_source_keys_kernel<<<(n + 255) / 256, 256, 0, stream>>>(points, n, g, k0, v0);
  SCORP_KERNEL_CHECK("icp_source_keys", 0, stream);
  if (int e = radix_sort(k0, v0, k1, v1, n, 32, tiles, hist, stream)) return e;
  *order = v0;   // (radix_sort swaps its pointer arguments: v0 is the sorted side here)
  return SCORP_OK;
}

// The source's side: the points in Morton order (W.sp) and, where the caller wants it, that order.
int icp_build_source(const float *source, int ns, const IcpLayout &L, const IcpWorkspace &W, hipStream_t stream,
                     const uint32_t **order = nullptr) {
  const uint32_t *sorted;
  if (int e = icp_sort_source(source, ns, W.g, W.k0, W.v0, W.k1, W.v1, W.hist, L.tiles, stream, &sorted)) return e;
  icp_gather_source_kernel<<<(ns + 255) / 256, 256, 0, stream>>>(source, sorted, ns, W.sp);
  SCORP_KERNEL_CHECK("icp_gather_source", 0, stream);
  if (order) *order = sorted;
  return SCORP_OK;
}

// The loop of a call: step(k) launches pass k and its solve; the per-init active flags are read every kIcpPollEvery
// iterations, and the loop ends when every init has stopped.
template <class Step>
int icp_iterate(int ni, int max_iteration, const int32_t *active, hipStream_t stream, Step step) {
  std::vector<int32_t> flags(ni);
  for (int k = 0; k <= max_iteration; k++) {
    if (int e = step(k)) return e;
    if (k < max_iteration && (k + 1) % kIcpPollEvery == 0) {
      SCORP_HIP_CHECK(hipMemcpyAsync(flags.data(), active, (size_t)ni * 4, hipMemcpyDeviceToHost, stream));
      SCORP_HIP_CHECK(hipStreamSynchronize(stream));
      bool any = false;
      for (int j = 0; j < ni; j++) any |= flags[j] != 0;
      if (!any) break;
    }
  }
  return SCORP_OK;
}

// The workspace of every entry point built on this file: there, large enough, 256-byte aligned.
int check_workspace(const char *who, const void *workspace, size_t bytes, size_t need) {
  if (!workspace || bytes < need || ((uintptr_t)workspace & 255)) {
    set_error("%s: workspace NULL, too small or not 256-byte aligned (%zu < %zu)", who, bytes, need);
    return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

// The argument checks the two ICP entry points share (`pointers`: every pointer argument but the workspace is non-NULL).
int icp_check_args(const char *who, double r, int32_t ns, int32_t nt, int32_t max_iteration, int32_t ni, bool pointers) {
  if (!(r > 0.0) || !std::isfinite(r)) { set_error("%s: max_correspondence_distance must be a positive finite number", who); return SCORP_ERR_INVALID; }
  if (ns <= 0) { set_error("%s: empty source", who); return SCORP_ERR_INVALID; }
  if (nt <= 0) { set_error("%s: empty target", who); return SCORP_ERR_INVALID; }
  if (max_iteration < 0) { set_error("%s: max_iteration < 0", who); return SCORP_ERR_INVALID; }
  if (ni <= 0 || ni > 65535) { set_error("%s: n_init must be in [1, 65535]", who); return SCORP_ERR_INVALID; }
  if (nt > (1 << 30)) { set_error("%s: more than 2^30 target points", who); return SCORP_ERR_INVALID; }
  if (!pointers) { set_error("%s: NULL argument", who); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp
