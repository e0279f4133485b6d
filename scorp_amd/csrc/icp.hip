// icp.hip — multi-start point-to-point ICP (Open3D registration_icp with TransformationEstimationPointToPoint, no
// scaling), every init of a call in one batch.  The reference's alignment scripts run it from 67 initial poses with
// max_iteration = 400 (align_3dgs_clpe_9dof.py:42-115 get_ICP_fitting_transformation_best).
//
// Built once per call:
//   * the target Q in a uniform grid (cell edge from the point density, not from r), its points sorted by cell (a stable
//     LSD radix sort on the cell id) as float4 {q - c_t (fp32), original index};
//   * the source P sorted by a 30-bit Morton code over its own bounding box (same sort), so that the 64 queries of a wave
//     stay neighbours under every rigid T_i and the target cells they visit are shared through L2.
// Per iteration (no host synchronisation; the host reads the active flags every kIcpPollEvery iterations):
//   * icp_pass_kernel, grid (source blocks, inits): x = T_i p in float64 (the cumulative transform on the original point),
//     exact nearest target point within r by an outward ring search over the grid in fp32, the chosen pair's d^2 and the
//     moments in float64 relative to c_t; one fixed row of 17 sums per block, no float atomics;
//   * icp_solve_kernel, one wave per init: the rows reduced in a fixed order, fitness / rmse, the stop rule, the Umeyama
//     update (3x3 one-sided Jacobi SVD in float64, svd3.hpp, reflection rule) composed onto T in float64.
// A block's row depends only on (its source range, its init's T), and the rows are reduced in a fixed order: two calls
// give the same bits, and init j run alone gives the bits of row j of a batch.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "svd3.hpp"

namespace scorp {
namespace {

constexpr int kIcpThreads = 256;
constexpr int kIcpPerThread = 4;
constexpr int kIcpChunk = kIcpThreads * kIcpPerThread;   // source points per pass block
constexpr int kIcpRow = 18;                              // doubles per partial row: 17 sums + pad
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

struct IcpLayout {
  size_t grid, keys0, keys1, vals0, vals1, hist, cell_start, tq, src, rows, active, total;
  int64_t nmax, tiles;
  IcpLayout(int64_t ns, int64_t nt, int64_t ni) {
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
    rows = off; off = align_up(off + (size_t)(nblk > 0 ? nblk : 1) * (size_t)(ni > 0 ? ni : 1) * kIcpRow * 8, 256);
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

// ---- the correspondence pass ----

__device__ __forceinline__ double wave_sum_f64(double v) {   // fixed butterfly: the same order on every call
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Original index of the nearest target point to x (relative fp32) with d^2 <= best on entry, -1 if none; ties go to the
// lower original index.  Rings of cells at Chebyshev distance k around x's cell (clamped to one cell outside the grid),
// clipped to the grid, until the distance from x to everything outside ring k's box exceeds the best d^2 so far, or
// nothing is left outside it.
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
  // cells ca..cb of one grid row: cell ids are raster order (x fastest), so their points are one contiguous run
  auto visit = [&](int ca, int cb) {
    const uint32_t e = cell_start[cb + 1];
    for (uint32_t t = cell_start[ca]; t < e; t++) {
      const float4 q = tq[t];
      const float ux = q.x - x, uy = q.y - y, uz = q.z - z;
      const float d2 = __builtin_fmaf(ux, ux, __builtin_fmaf(uy, uy, uz * uz));
      const uint32_t id = __float_as_uint(q.w);
      if (d2 < best || (d2 == best && id < bidx)) { best = d2; bidx = id; }
    }
  };
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
    float lb = 3.4e38f;
    if (cx - k > 0) lb = fminf(lb, x - (lx + (cx - k) * h));
    if (cx + k < dx - 1) lb = fminf(lb, (lx + (cx + k + 1) * h) - x);
    if (cy - k > 0) lb = fminf(lb, y - (ly + (cy - k) * h));
    if (cy + k < dy - 1) lb = fminf(lb, (ly + (cy + k + 1) * h) - y);
    if (cz - k > 0) lb = fminf(lb, z - (lz + (cz - k) * h));
    if (cz + k < dz - 1) lb = fminf(lb, (lz + (cz + k + 1) * h) - z);
    if (lb >= 3.4e38f) break;
    lb = fmaxf(lb, 0.0f);
    if (!(lb * lb <= best)) break;   // (a NaN query ends here too)
  }
  return bidx == 0xFFFFFFFFu ? -1 : (int)bidx;
}

// grid (source blocks, inits).  Row layout: [c, sum d^2, sum x (3), sum q (3), sum x_a q_b (9, a-major), pad]
__global__ void __launch_bounds__(kIcpThreads) icp_pass_kernel(const float4 *__restrict__ sp, int ns, const float4 *__restrict__ tq,
                                                               const float *__restrict__ tgt, const uint32_t *__restrict__ cell_start,
                                                               const IcpGrid *__restrict__ g, const double *__restrict__ T,
                                                               const int32_t *__restrict__ active, double r2, float r2f,
                                                               double *__restrict__ rows) {
  const int j = blockIdx.y;
  if (!active[j]) return;
  const double *M = T + (size_t)j * 16;
  const double m00 = M[0], m01 = M[1], m02 = M[2], m03 = M[3] - g->ct[0];
  const double m10 = M[4], m11 = M[5], m12 = M[6], m13 = M[7] - g->ct[1];
  const double m20 = M[8], m21 = M[9], m22 = M[10], m23 = M[11] - g->ct[2];
  const double c0 = g->ct[0], c1 = g->ct[1], c2 = g->ct[2];
  double acc[17];
#pragma unroll
  for (int a = 0; a < 17; a++) acc[a] = 0.0;
  const int base = blockIdx.x * kIcpChunk + threadIdx.x;
  for (int k = 0; k < kIcpPerThread; k++) {
    const int i = base + k * kIcpThreads;
    if (i >= ns) break;
    const float4 p = sp[i];
    const double px = p.x, py = p.y, pz = p.z;
    // x - c_t in float64: T applied to the original point
    const double x0 = fma(m00, px, fma(m01, py, fma(m02, pz, m03)));
    const double x1 = fma(m10, px, fma(m11, py, fma(m12, pz, m13)));
    const double x2 = fma(m20, px, fma(m21, py, fma(m22, pz, m23)));
    const int id = icp_nearest((float)x0, (float)x1, (float)x2, r2f, g, cell_start, tq);
    if (id < 0) continue;
    const double q0 = (double)tgt[(size_t)id * 3 + 0] - c0, q1 = (double)tgt[(size_t)id * 3 + 1] - c1,
                 q2 = (double)tgt[(size_t)id * 3 + 2] - c2;
    const double u0 = x0 - q0, u1 = x1 - q1, u2 = x2 - q2;
    const double d2 = fma(u0, u0, fma(u1, u1, u2 * u2));
    if (!(d2 <= r2)) continue;
    acc[0] += 1.0;
    acc[1] += d2;
    acc[2] += x0; acc[3] += x1; acc[4] += x2;
    acc[5] += q0; acc[6] += q1; acc[7] += q2;
    acc[8] = fma(x0, q0, acc[8]); acc[9] = fma(x0, q1, acc[9]); acc[10] = fma(x0, q2, acc[10]);
    acc[11] = fma(x1, q0, acc[11]); acc[12] = fma(x1, q1, acc[12]); acc[13] = fma(x1, q2, acc[13]);
    acc[14] = fma(x2, q0, acc[14]); acc[15] = fma(x2, q1, acc[15]); acc[16] = fma(x2, q2, acc[16]);
  }
  __shared__ double part[kIcpThreads / 64][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 17; a++) {
    const double v = wave_sum_f64(acc[a]);
    if (lane == 0) part[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < 17) {
    double s = 0.0;
    for (int w = 0; w < kIcpThreads / 64; w++) s += part[w][threadIdx.x];
    rows[((size_t)j * gridDim.x + blockIdx.x) * kIcpRow + threadIdx.x] = s;
  }
}

// ---- the solve ----

// one wave per init, after pass `k` (every active init has run the same number of passes)
__global__ void __launch_bounds__(64) icp_solve_kernel(const double *__restrict__ rows, int nblk, int ns, const IcpGrid *__restrict__ g,
                                                       int k, int max_iteration, double rel_fitness, double rel_rmse, double *T,
                                                       double *fitness, double *rmse, int32_t *iters, int32_t *active) {
  const int j = blockIdx.x;
  if (!active[j]) return;
  const int lane = threadIdx.x;
  double S[17];
#pragma unroll
  for (int a = 0; a < 17; a++) S[a] = 0.0;
  for (int b = lane; b < nblk; b += 64) {
    const double *r = rows + ((size_t)j * nblk + b) * kIcpRow;
#pragma unroll
    for (int a = 0; a < 17; a++) S[a] += r[a];
  }
#pragma unroll
  for (int a = 0; a < 17; a++) S[a] = wave_sum_f64(S[a]);
  if (lane != 0) return;
  const double c = S[0];
  const double fit = c > 0.0 ? c / (double)ns : 0.0;
  const double rm = c > 0.0 ? sqrt(S[1] / c) : 0.0;
  if (k > 0) {
    const double pf = fitness[j], pr = rmse[j];
    fitness[j] = fit;
    rmse[j] = rm;
    if (fabs(pf - fit) < rel_fitness && fabs(pr - rm) < rel_rmse) { iters[j] = k; active[j] = 0; return; }
  } else {
    fitness[j] = fit;
    rmse[j] = rm;
  }
  if (k >= max_iteration) { iters[j] = k; active[j] = 0; return; }
  if (c <= 0.0) return;   // the update is the identity: T stays
  // Umeyama without scale: Sigma = (1/c) sum (q - qm)(x - xm)^T = U S V^T, R = U D V^T, t = qm - R xm (relative to c_t)
  double xm[3], qm[3], A[3][3];
  for (int a = 0; a < 3; a++) { xm[a] = S[2 + a] / c; qm[a] = S[5 + a] / c; }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) A[a][b] = S[8 + b * 3 + a] / c - qm[a] * xm[b];   // S[8 + 3b + a] = sum x_b q_a
  // A Sigma at the rounding level of its raw moments (one pair; every pair at one point) is exactly zero in the
  // reference's demeaned form: take it as zero, so that R = I as there, not a rotation of the rounding noise
  double scale = 0.0, amax = 0.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      scale = fmax(scale, fabs(S[8 + b * 3 + a] / c) + fabs(qm[a] * xm[b]));
      amax = fmax(amax, fabs(A[a][b]));
    }
  if (amax <= 1e-12 * scale)
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) A[a][b] = 0.0;
  double U[3][3], V[3][3];
  svd3(A, U, V);
  const double dsign = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
  double R[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) R[a][b] = U[a][0] * V[b][0] + U[a][1] * V[b][1] + dsign * U[a][2] * V[b][2];
  double t[3];
  for (int a = 0; a < 3; a++) {
    // absolute: q = R x + t with x = x' + c_t, q = q' + c_t  ->  t = (qm' - R xm') + (c_t - R c_t)
    double rx = 0.0, rc = 0.0;
    for (int b = 0; b < 3; b++) { rx += R[a][b] * xm[b]; rc += R[a][b] * g->ct[b]; }
    t[a] = (qm[a] - rx) + (g->ct[a] - rc);
  }
  double *M = T + (size_t)j * 16, N[12];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 4; b++)
      N[a * 4 + b] = R[a][0] * M[b] + R[a][1] * M[4 + b] + R[a][2] * M[8 + b] + (b == 3 ? t[a] : 0.0);
  for (int e = 0; e < 12; e++) M[e] = N[e];
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

int icp_impl(const float *source, int32_t ns, const float *target, int32_t nt, const double *inits, int32_t ni, double r,
             int32_t max_iteration, double rel_fitness, double rel_rmse, double *out_T, double *out_fitness, double *out_rmse,
             int32_t *out_iters, void *workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!(r > 0.0) || !std::isfinite(r)) { set_error("icp: max_correspondence_distance must be a positive finite number"); return SCORP_ERR_INVALID; }
  if (ns <= 0) { set_error("icp: empty source"); return SCORP_ERR_INVALID; }
  if (nt <= 0) { set_error("icp: empty target"); return SCORP_ERR_INVALID; }
  if (max_iteration < 0) { set_error("icp: max_iteration < 0"); return SCORP_ERR_INVALID; }
  if (ni <= 0 || ni > 65535) { set_error("icp: n_init must be in [1, 65535]"); return SCORP_ERR_INVALID; }
  if (nt > (1 << 30)) { set_error("icp: more than 2^30 target points"); return SCORP_ERR_INVALID; }
  if (!source || !target || !inits || !out_T || !out_fitness || !out_rmse || !out_iters || !workspace) {
    set_error("icp: NULL argument"); return SCORP_ERR_INVALID;
  }
  const IcpLayout L(ns, nt, ni);
  if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) {
    set_error("icp: workspace too small or not 256-byte aligned (%zu < %zu)", workspace_bytes, L.total);
    return SCORP_ERR_INVALID;
  }
  char *w = (char *)workspace;
  IcpGrid *g = (IcpGrid *)(w + L.grid);
  uint32_t *k0 = (uint32_t *)(w + L.keys0), *k1 = (uint32_t *)(w + L.keys1), *v0 = (uint32_t *)(w + L.vals0),
           *v1 = (uint32_t *)(w + L.vals1), *hist = (uint32_t *)(w + L.hist), *cell_start = (uint32_t *)(w + L.cell_start);
  float4 *tq = (float4 *)(w + L.tq), *sp = (float4 *)(w + L.src);
  double *rows = (double *)(w + L.rows);
  int32_t *active = (int32_t *)(w + L.active);
  const int cap = (int)icp_cell_cap(nt);

  icp_bbox_kernel<<<1, 1024, 0, stream>>>(target, nt, g->tlo, g->thi);
  SCORP_KERNEL_CHECK("icp_bbox", 0, stream);
  icp_bbox_kernel<<<1, 1024, 0, stream>>>(source, ns, g->slo, g->shi);
  SCORP_KERNEL_CHECK("icp_bbox", 0, stream);
  icp_grid_setup_kernel<<<1, 64, 0, stream>>>(g, nt, cap);
  SCORP_KERNEL_CHECK("icp_grid_setup", 0, stream);
  // target: sorted by cell, cell_start
  icp_target_keys_kernel<<<(nt + 255) / 256, 256, 0, stream>>>(target, nt, g, k0, v0);
  SCORP_KERNEL_CHECK("icp_target_keys", 0, stream);
  int bits = 8;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)cap) bits += 8;
  {
    uint32_t *a = k0, *b = v0, *c = k1, *d = v1;
    if (int e = radix_sort(a, b, c, d, nt, bits, L.tiles, hist, stream)) return e;
    icp_cell_start_kernel<<<(nt + 1 + 255) / 256, 256, 0, stream>>>(a, nt, g, cell_start);
    SCORP_KERNEL_CHECK("icp_cell_start", 0, stream);
    icp_gather_target_kernel<<<(nt + 255) / 256, 256, 0, stream>>>(target, b, nt, g, tq);
    SCORP_KERNEL_CHECK("icp_gather_target", 0, stream);
  }
  // source: Morton order
  icp_source_keys_kernel<<<(ns + 255) / 256, 256, 0, stream>>>(source, ns, g, k0, v0);
  SCORP_KERNEL_CHECK("icp_source_keys", 0, stream);
  {
    uint32_t *a = k0, *b = v0, *c = k1, *d = v1;
    if (int e = radix_sort(a, b, c, d, ns, 32, L.tiles, hist, stream)) return e;
    icp_gather_source_kernel<<<(ns + 255) / 256, 256, 0, stream>>>(source, b, ns, sp);
    SCORP_KERNEL_CHECK("icp_gather_source", 0, stream);
  }
  icp_init_kernel<<<(ni + 63) / 64, 64, 0, stream>>>(inits, ni, out_T, out_fitness, out_rmse, out_iters, active);
  SCORP_KERNEL_CHECK("icp_init", 0, stream);

  const int nblk = (ns + kIcpChunk - 1) / kIcpChunk;
  const double r2 = r * r;
  const float r2f = (float)r2 * (1.0f + 1e-5f);   // the fp32 search keeps slightly more; the pair test is float64
  std::vector<int32_t> flags(ni);
  for (int k = 0; k <= max_iteration; k++) {
    icp_pass_kernel<<<dim3(nblk, ni), kIcpThreads, 0, stream>>>(sp, ns, tq, target, cell_start, g, out_T, active, r2, r2f, rows);
    SCORP_KERNEL_CHECK("icp_pass", 0, stream);
    icp_solve_kernel<<<ni, 64, 0, stream>>>(rows, nblk, ns, g, k, max_iteration, rel_fitness, rel_rmse, out_T, out_fitness,
                                            out_rmse, out_iters, active);
    SCORP_KERNEL_CHECK("icp_solve", 0, stream);
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

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_icp_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init) {
  return IcpLayout(n_source, n_target, n_init).total;
}

extern "C" int scorp_icp_point_to_point(const float *source, int32_t n_source, const float *target, int32_t n_target,
                                        const double *inits, int32_t n_init, double max_correspondence_distance,
                                        int32_t max_iteration, double relative_fitness, double relative_rmse,
                                        double *out_transformation, double *out_fitness, double *out_inlier_rmse,
                                        int32_t *out_iterations, void *workspace, size_t workspace_bytes,
                                        scorp_stream_t stream) {
  return icp_impl(source, n_source, target, n_target, inits, n_init, max_correspondence_distance, max_iteration,
                  relative_fitness, relative_rmse, out_transformation, out_fitness, out_inlier_rmse, out_iterations, workspace,
                  workspace_bytes, (hipStream_t)stream);
}
