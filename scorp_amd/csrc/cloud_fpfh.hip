// cloud_fpfh.hip - the FPFH descriptor of a cloud with normals (scorp_amd/global_registration.py; the rules F1 - F5 are
// the global-registration block of include/scorp_gs.h, tests/fpfh_reference.py restates them as a float64 brute force).
// The fourth includer of icp_search.hpp, through cloud_search.hpp: the grid, the ring walk with its widened reach, rule
// R1's d^2 and the original coordinates in cell order are cloud_filter.hip's.
//
// Three kernels:
//   search   one thread per point in cell order.  The max_nn best (float64 d^2, index) within the radius, the point itself
//            left out by index, sit sorted in the lane's column of two LDS arrays sized at the launch: icp_search.hpp's
//            KBest, icp_normals_kernel's list (768 max_nn bytes per workgroup of 64 lanes, 48 KB at 64).  The walk's reach
//            is the radius until the list is full and the max_nn-th d^2 after that.  It writes the neighbour list
//            [n, max_nn] and the degree, ONCE; both later passes read them.
//   spfh     one lane per (point, slot of its list).  The pair feature of F2, its three bins of F3, and three integer
//            atomic increments straight into the point's 33 global int32 counts (zeroed by a memset): integers, so the
//            order of arrival is free.
//   fpfh     one lane per (point, bin), 7 points per workgroup of 256.  Each lane runs down its point's list serially in
//            list order (F5), reading one int32 of the neighbour's contiguous 33-count row, so the order of the float64
//            sum is fixed and no reduction is needed.  The 33 sums of a point then meet in LDS, where every lane adds up
//            its own block of 11 in ascending order.  d^2(i, j) is formed again from the coordinates by R1's expression:
//            the same bits as in the search.
//
// All arithmetic is float64 from the float32 inputs with contraction off; sqrt and the divisions are the correctly rounded
// ones.  atan2 is the only operation whose last place may differ from another library's.  No float atomics: every output
// is a function of the input alone.
#include "cloud_search.hpp"

#pragma clang fp contract(off)

namespace scorp {
namespace {

constexpr int kFpfhSearchThreads = kKBestLanes;
constexpr int kFpfhMaxNn = 64;
constexpr int kFpfhBins = 11, kFpfhDim = 33;
constexpr int kFpfhThreads = 256;
constexpr int kFpfhPointsPerBlock = kFpfhThreads / kFpfhDim;   // 7: lanes 231 .. 255 idle

// what a call's workspace holds after the CloudLayout
struct FpfhLayout {
  size_t nbr, deg, count, extra;
  FpfhLayout(int64_t n, int max_nn, size_t base) {
    size_t off = base;
    nbr = off; off = align_up(off + (size_t)n * max_nn * 4, 256);
    deg = off; off = align_up(off + (size_t)n * 4, 256);
    count = off; off = align_up(off + (size_t)n * kFpfhDim * 4, 256);
    extra = off - base;
  }
};

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 load3(const float *__restrict__ p, size_t i) { return {(double)p[i * 3], (double)p[i * 3 + 1], (double)p[i * 3 + 2]}; }
__device__ __forceinline__ double dot3(const D3 &a, const D3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross3(const D3 &a, const D3 &b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// R1 on the points' own rows (p_j - p_i and p_i - p_j have the same squares)
__device__ __forceinline__ double pair_d2(const D3 &pi, const D3 &pj) {
  const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
  return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ int fpfh_bin(double x) { return (int)fmin(fmax(floor(x), 0.0), 10.0); }

// F1
__global__ void __launch_bounds__(kFpfhSearchThreads) fpfh_search_kernel(const float4 *__restrict__ tq, const float4 *__restrict__ tp, int n,
                                                                         int max_nn, double r2, const uint32_t *__restrict__ cell_start,
                                                                         const IcpGrid *__restrict__ g, int32_t *__restrict__ nbr,
                                                                         int32_t *__restrict__ deg) {
  extern __shared__ double fpfh_lds[];   // max_nn rows of 64 d^2, then max_nn rows of 64 indices
  double (*nd)[kFpfhSearchThreads] = (double (*)[kFpfhSearchThreads])fpfh_lds;
  uint32_t (*ni)[kFpfhSearchThreads] = (uint32_t (*)[kFpfhSearchThreads])(fpfh_lds + (size_t)max_nn * kFpfhSearchThreads);
  const int lane = threadIdx.x;
  const int i = blockIdx.x * kFpfhSearchThreads + lane;
  if (i >= n) return;
  const float4 me = tp[i];
  const uint32_t self = __float_as_uint(me.w);
  const CloudWalk walk(tq[i], g);
  const float reach_r = walk.reach(r2);
  KBest<double> best(nd, ni, lane, max_nn, __builtin_inf());   // (its k-th d^2 is never above r2)
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) {
      const float4 q = tp[t];
      const uint32_t id = __float_as_uint(q.w);
      const double d2 = cloud_d2(me, q);
      if (id == self || !(d2 <= r2)) return;
      best.offer(d2, id);
    });
  };
  walk.run(visit, [&]() { return best.full() ? walk.reach(best.kth()) : reach_r; });
  best.write_neighbors(nbr, self, max_nn);
  deg[self] = best.count();
}

// F2 - F4: the counts
__global__ void __launch_bounds__(kFpfhThreads) fpfh_spfh_kernel(const float *__restrict__ pts, const float *__restrict__ nrm, int n, int max_nn,
                                                                 const int32_t *__restrict__ nbr, const int32_t *__restrict__ deg,
                                                                 int32_t *count) {
  const int64_t t = (int64_t)blockIdx.x * kFpfhThreads + threadIdx.x;
  if (t >= (int64_t)n * max_nn) return;
  const int i = (int)(t / max_nn), a = (int)(t % max_nn);
  if (a >= deg[i]) return;
  const int j = nbr[t];
  const D3 pi = load3(pts, i), pj = load3(pts, j), ni = load3(nrm, i), nj = load3(nrm, j);
  D3 dp = {pj.x - pi.x, pj.y - pi.y, pj.z - pi.z};
  const double f4 = sqrt((dp.x * dp.x + dp.y * dp.y) + dp.z * dp.z);
  if (f4 == 0.0) return;
  const double a1 = dot3(ni, dp) / f4, a2 = dot3(nj, dp) / f4;
  D3 u = ni, n2 = nj;
  double f3 = a1;
  if (fabs(a1) < fabs(a2)) {
    u = nj; n2 = ni;
    dp = {-dp.x, -dp.y, -dp.z};
    f3 = -a2;
  }
  D3 v = cross3(dp, u);
  const double vn = sqrt(dot3(v, v));
  if (vn == 0.0) return;
  v = {v.x / vn, v.y / vn, v.z / vn};
  const D3 w = cross3(u, v);
  const double f2 = dot3(v, n2);
  const double f1 = atan2(dot3(w, n2), dot3(u, n2));
  const int b1 = fpfh_bin((11.0 * (f1 + M_PI)) / (2.0 * M_PI));
  const int b2 = fpfh_bin(11.0 * ((f2 + 1.0) * 0.5));
  const int b3 = fpfh_bin(11.0 * ((f3 + 1.0) * 0.5));
  int32_t *row = count + (size_t)i * kFpfhDim;
  atomicAdd(row + b1, 1);
  atomicAdd(row + kFpfhBins + b2, 1);
  atomicAdd(row + 2 * kFpfhBins + b3, 1);
}

// F4's scaling and F5
__global__ void __launch_bounds__(kFpfhThreads) fpfh_feature_kernel(const float *__restrict__ pts, int n, int max_nn,
                                                                    const int32_t *__restrict__ nbr, const int32_t *__restrict__ deg,
                                                                    const int32_t *__restrict__ count, double *__restrict__ out) {
  __shared__ double sums[kFpfhPointsPerBlock][kFpfhDim];
  const int p = threadIdx.x / kFpfhDim, b = threadIdx.x % kFpfhDim;
  const int64_t i = (int64_t)blockIdx.x * kFpfhPointsPerBlock + p;
  const bool live = p < kFpfhPointsPerBlock && i < n;
  double s = 0.0;
  int m = 0;
  if (live) {
    m = deg[i];
    const D3 pi = load3(pts, i);
    for (int a = 0; a < m; a++) {
      const int j = nbr[i * max_nn + a];
      const double d2 = pair_d2(pi, load3(pts, j));
      const int mj = deg[j];
      if (d2 > 0.0 && mj > 0) {
        const double spfh = (double)count[(size_t)j * kFpfhDim + b] * (100.0 / (double)mj);
        s = s + spfh / d2;
      }
    }
    sums[p][b] = s;
  }
  __syncthreads();
  if (!live) return;
  const int k0 = b / kFpfhBins * kFpfhBins;
  double t = 0.0;
  for (int e = 0; e < kFpfhBins; e++) t = t + sums[p][k0 + e];
  if (t != 0.0) s = s * (100.0 / t);
  const double own = m > 0 ? (double)count[i * kFpfhDim + b] * (100.0 / (double)m) : 0.0;
  out[i * kFpfhDim + b] = s + own;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_cloud_fpfh_workspace_bytes(int32_t n, int32_t max_nn) {
  const int64_t nn = n > 0 ? n : 1;
  const int k = max_nn < 1 ? 1 : (max_nn > kFpfhMaxNn ? kFpfhMaxNn : max_nn);
  const size_t base = CloudLayout(nn).total;
  return base + FpfhLayout(nn, k, base).extra;
}

extern "C" int scorp_cloud_fpfh(const float *points, const float *normals, int32_t n, double radius, int32_t max_nn, double *out_feature,
                                int32_t *out_spfh_count, int32_t *out_neighbors, int32_t *out_degree, void *workspace,
                                size_t workspace_bytes, scorp_stream_t stream) {
  if (int e = cloud_check_radius("cloud_fpfh", "radius", radius)) return e;
  if (max_nn < 1 || max_nn > kFpfhMaxNn) { set_error("cloud_fpfh: max_nn must be in [1, %d]", kFpfhMaxNn); return SCORP_ERR_INVALID; }
  const CloudLayout L(n > 0 ? n : 1);
  const FpfhLayout F(n > 0 ? n : 1, max_nn, L.total);
  if (int e = cloud_check("cloud_fpfh", points, n, normals && out_feature, workspace, workspace_bytes, F.extra)) return e;
  const CloudWorkspace W(workspace, L);
  char *w = (char *)workspace;
  int32_t *nbr = out_neighbors ? out_neighbors : (int32_t *)(w + F.nbr);
  int32_t *deg = out_degree ? out_degree : (int32_t *)(w + F.deg);
  int32_t *count = out_spfh_count ? out_spfh_count : (int32_t *)(w + F.count);
  hipStream_t s = (hipStream_t)stream;
  if (int e = cloud_build(points, n, L, W, s)) return e;
  fpfh_search_kernel<<<(n + kFpfhSearchThreads - 1) / kFpfhSearchThreads, kFpfhSearchThreads, (size_t)max_nn * kFpfhSearchThreads * 12, s>>>(
      W.icp.tq, W.tp, n, max_nn, radius * radius, W.icp.cell_start, W.icp.g, nbr, deg);
  SCORP_KERNEL_CHECK("fpfh_search", 0, s);
  SCORP_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)n * kFpfhDim * sizeof(int32_t), s));
  const int64_t pairs = (int64_t)n * max_nn;
  fpfh_spfh_kernel<<<(unsigned)((pairs + kFpfhThreads - 1) / kFpfhThreads), kFpfhThreads, 0, s>>>(points, normals, n, max_nn, nbr, deg, count);
  SCORP_KERNEL_CHECK("fpfh_spfh", 0, s);
  fpfh_feature_kernel<<<(n + kFpfhPointsPerBlock - 1) / kFpfhPointsPerBlock, kFpfhThreads, 0, s>>>(points, n, max_nn, nbr, deg, count,
                                                                                                  out_feature);
  SCORP_KERNEL_CHECK("fpfh_feature", 0, s);
  return SCORP_OK;
}
