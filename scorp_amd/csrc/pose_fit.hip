// pose_fit.hip — the pose fit from matched 3-D point pairs of the alignment scripts (align_3dgs_clpe_9dof.py:437 / :450):
// pc_align_ransac (utils/solution.py:476-557) and adam_algorithm_3d3d_9dof (utils/solution.py:363-446).
//
// Everything is float64: a pair set is a few thousand points, the cost is launches and latency, not arithmetic, and float64
// makes the inlier test the reference's own (numpy float64).  No float atomics: the per-hypothesis inlier counts are
// integers (integer atomics), every float sum is a per-block row reduced in a fixed order.  Two calls give the same bits,
// and a hypothesis run alone gets the count it gets in a batch.  The library draws no random numbers: the sample triples
// are an input.
//
// RANSAC (scorp_pose_ransac):
//   ransac_fit_kernel     one lane per hypothesis: Umeyama / Kabsch on its three pairs (svd3.hpp; the rank-2 covariance's
//                         third singular vectors are the zero-singular-value completion there, fixed by the determinant rule)
//   ransac_count_kernel   grid (blocks of pairs, hypotheses): |R (s p) + t - q| < threshold, one integer count per hypothesis
//   ransac_select_kernel  one wave: the first hypothesis with the highest count, or (min_inlier_ratio > 0) the first whose
//                         count exceeds min_inlier_ratio * n
//   pose_sums_kernel      the winner's inlier mask; per block: count, sum p, sum q
//   pose_moments_kernel   per block, about the two centroids: sum qc pc^T, sum pc pc^T, sum qc.qc
//   ransac_final_kernel   one wave: the rows reduced in a fixed order, one solve
// 9-DoF Adam (scorp_pose_adam_9dof): pose_sums_kernel + pose_moments_kernel over all pairs, then pose_adam_kernel, ONE wave
// and one launch for all iterations: with M = R(q) Ro(qo)^T diag(s) Ro(qo) the data term mean |M p + t - q|^2 and its
// gradient depend on the points only through those moments, so a step is a few hundred float64 operations on 14 numbers.
#include <cmath>

#include "common.hpp"
#include "svd3.hpp"

namespace scorp {
namespace {

constexpr int kPoseThreads = 256;
constexpr int kPosePerThread = 4;
constexpr int kPoseChunk = kPoseThreads * kPosePerThread;   // pairs per block
constexpr int kModelStride = 16;                             // doubles per hypothesis: R (9), t (3), s, valid, pad
constexpr int kSumsRow = 8;                                  // count, sum p (3), sum q (3), pad
constexpr int kMomRow = 16;                                  // sum qc pc^T (9, q-major), sum pc pc^T (xx xy xz yy yz zz), sum qc.qc
constexpr int kMaxAdamIterations = 1000000;

struct PoseSelect {
  int32_t winner, count, status, pad;   // status bit 0: a sample index outside [0, n); bit 1: fewer than 3 inliers
};

struct PoseLayout {
  size_t sel, models, sums, moms, mask, total;
  int64_t nblk;
  PoseLayout(int64_t n, int64_t nh) {
    if (n < 1) n = 1;
    if (nh < 1) nh = 1;
    nblk = (n + kPoseChunk - 1) / kPoseChunk;
    size_t off = 0;
    sel = off; off = align_up(off + sizeof(PoseSelect), 256);
    models = off; off = align_up(off + (size_t)nh * kModelStride * 8, 256);
    sums = off; off = align_up(off + (size_t)nblk * kSumsRow * 8, 256);
    moms = off; off = align_up(off + (size_t)nblk * kMomRow * 8, 256);
    mask = off; off = align_up(off + (size_t)n, 256);
    total = off;
  }
};

// The similarity q ~ s R p + t from centred moments: A = sum qc pc^T = U S V^T, D = diag(1, 1, det U det V < 0 ? -1 : 1),
// R = U D V^T, s = sum(S diag D) / spp = trace(R^T A) / spp (Umeyama) or 1 (Kabsch), t = qm - s R pm.
__device__ void pose_solve(const double A[3][3], double spp, const double pm[3], const double qm[3], bool with_scale, double R[3][3],
                           double t[3], double *s) {
  double U[3][3], V[3][3];
  svd3(A, U, V);
  const double dsign = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
  double tr = 0.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      R[a][b] = U[a][0] * V[b][0] + U[a][1] * V[b][1] + dsign * U[a][2] * V[b][2];
      tr += R[a][b] * A[a][b];
    }
  const double sc = with_scale ? tr / spp : 1.0;
  for (int a = 0; a < 3; a++) t[a] = qm[a] - sc * (R[a][0] * pm[0] + R[a][1] * pm[1] + R[a][2] * pm[2]);
  *s = sc;
}

// ---- RANSAC ----

__global__ void __launch_bounds__(64) ransac_fit_kernel(const double *__restrict__ P, const double *__restrict__ Q, int n,
                                                        const int32_t *__restrict__ samples, int nh, int with_scale,
                                                        double *__restrict__ models, PoseSelect *sel) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= nh) return;
  double *m = models + (size_t)h * kModelStride;
  int idx[3];
  bool ok = true;
  for (int k = 0; k < 3; k++) {
    idx[k] = samples[(size_t)h * 3 + k];
    ok = ok && idx[k] >= 0 && idx[k] < n;
  }
  if (!ok) {
    atomicOr(&sel->status, 1);
    for (int e = 0; e < kModelStride; e++) m[e] = 0.0;
    return;
  }
  double p[3][3], q[3][3], pm[3], qm[3];
  for (int k = 0; k < 3; k++)
    for (int a = 0; a < 3; a++) { p[k][a] = P[(size_t)idx[k] * 3 + a]; q[k][a] = Q[(size_t)idx[k] * 3 + a]; }
  for (int a = 0; a < 3; a++) {
    pm[a] = (p[0][a] + p[1][a] + p[2][a]) / 3.0;
    qm[a] = (q[0][a] + q[1][a] + q[2][a]) / 3.0;
  }
  double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, spp = 0.0;
  for (int k = 0; k < 3; k++)
    for (int a = 0; a < 3; a++) {
      const double pc = p[k][a] - pm[a];
      spp += pc * pc;
      for (int b = 0; b < 3; b++) A[b][a] += (q[k][b] - qm[b]) * pc;
    }
  double R[3][3], t[3], s;
  pose_solve(A, spp, pm, qm, with_scale != 0, R, t, &s);
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) m[a * 3 + b] = R[a][b];
    m[9 + a] = t[a];
  }
  m[12] = s;
  m[13] = 1.0;
  m[14] = 0.0;
  m[15] = 0.0;
}

// the reference's compute_residuals: | R (s p) + t - q |, strict <  (a NaN model counts nothing)
__device__ __forceinline__ bool pose_inlier(const double *__restrict__ m, const double *__restrict__ p, const double *__restrict__ q,
                                            double threshold) {
  const double s = m[12];
  const double x = s * p[0], y = s * p[1], z = s * p[2];
  const double d0 = (m[0] * x + m[1] * y + m[2] * z) + m[9] - q[0];
  const double d1 = (m[3] * x + m[4] * y + m[5] * z) + m[10] - q[1];
  const double d2 = (m[6] * x + m[7] * y + m[8] * z) + m[11] - q[2];
  return sqrt(d0 * d0 + d1 * d1 + d2 * d2) < threshold;
}

__global__ void __launch_bounds__(kPoseThreads) ransac_count_kernel(const double *__restrict__ P, const double *__restrict__ Q, int n,
                                                                    const double *__restrict__ models, double threshold,
                                                                    int32_t *__restrict__ counts) {
  const int h = blockIdx.y;
  const double *m = models + (size_t)h * kModelStride;
  if (m[13] == 0.0) return;
  int c = 0;
  const int base = blockIdx.x * kPoseChunk + threadIdx.x;
  for (int k = 0; k < kPosePerThread; k++) {
    const int i = base + k * kPoseThreads;
    if (i >= n) break;
    c += pose_inlier(m, P + (size_t)i * 3, Q + (size_t)i * 3, threshold) ? 1 : 0;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) c += __shfl_xor(c, w, 64);
  if ((threadIdx.x & 63) == 0 && c > 0) atomicAdd(&counts[h], c);   // integers: the order does not matter
}

// one wave.  min_ratio_n = min_inlier_ratio * n, or < 0 for "no early exit".
__global__ void __launch_bounds__(64) ransac_select_kernel(const int32_t *__restrict__ counts, int nh, double min_ratio_n,
                                                           PoseSelect *sel) {
  const int lane = threadIdx.x;
  int best_c = -1, best_h = 0x7fffffff, first_h = 0x7fffffff;
  for (int h = lane; h < nh; h += 64) {
    const int c = counts[h];
    if (c > best_c) { best_c = c; best_h = h; }   // (ascending h per lane: the first maximum of the lane)
    if (min_ratio_n > 0.0 && (double)c > min_ratio_n && c > 0 && h < first_h) first_h = h;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const int oc = __shfl_xor(best_c, w, 64), oh = __shfl_xor(best_h, w, 64), of = __shfl_xor(first_h, w, 64);
    if (oc > best_c || (oc == best_c && oh < best_h)) { best_c = oc; best_h = oh; }
    first_h = min(first_h, of);
  }
  if (lane != 0) return;
  if (first_h != 0x7fffffff) { best_h = first_h; best_c = counts[first_h]; }
  sel->winner = best_h;
  sel->count = best_c;
  if (best_c < 3) atomicOr(&sel->status, 2);
}

// ---- moments (shared by the RANSAC final fit and the Adam fit) ----

// Per block: count, sum p, sum q over the pairs that take part: all of them (models == nullptr), or the inliers of the
// selected hypothesis, whose mask is written on the way.
__global__ void __launch_bounds__(kPoseThreads) pose_sums_kernel(const double *__restrict__ P, const double *__restrict__ Q, int n,
                                                                 const double *__restrict__ models, const PoseSelect *__restrict__ sel,
                                                                 double threshold, uint8_t *__restrict__ mask,
                                                                 double *__restrict__ rows) {
  const double *m = models ? models + (size_t)sel->winner * kModelStride : nullptr;
  double acc[7];
#pragma unroll
  for (int a = 0; a < 7; a++) acc[a] = 0.0;
  const int base = blockIdx.x * kPoseChunk + threadIdx.x;
  for (int k = 0; k < kPosePerThread; k++) {
    const int i = base + k * kPoseThreads;
    if (i >= n) break;
    const double *p = P + (size_t)i * 3, *q = Q + (size_t)i * 3;
    bool in = true;
    if (m) {
      in = pose_inlier(m, p, q, threshold);
      mask[i] = in ? 1 : 0;
    }
    if (!in) continue;
    acc[0] += 1.0;
    acc[1] += p[0]; acc[2] += p[1]; acc[3] += p[2];
    acc[4] += q[0]; acc[5] += q[1]; acc[6] += q[2];
  }
  __shared__ double part[kPoseThreads / 64][7];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 7; a++) {
    const double v = wave_sum_f64(acc[a]);
    if (lane == 0) part[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSumsRow) {
    double s = 0.0;
    if (threadIdx.x < 7)
      for (int w = 0; w < kPoseThreads / 64; w++) s += part[w][threadIdx.x];
    rows[(size_t)blockIdx.x * kSumsRow + threadIdx.x] = s;
  }
}

// count and the two centroids from the rows of pose_sums_kernel, in row order (every caller gets the same bits)
__device__ __forceinline__ double pose_centroids(const double *__restrict__ rows, int nblk, double pm[3], double qm[3]) {
  double S[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < nblk; b++)
    for (int a = 0; a < 7; a++) S[a] += rows[(size_t)b * kSumsRow + a];
  const double c = S[0] > 0.0 ? S[0] : 1.0;
  for (int a = 0; a < 3; a++) { pm[a] = S[1 + a] / c; qm[a] = S[4 + a] / c; }
  return S[0];
}

// Per block, about the two centroids so that nothing cancels: sum qc pc^T, sum pc pc^T, sum qc.qc
__global__ void __launch_bounds__(kPoseThreads) pose_moments_kernel(const double *__restrict__ P, const double *__restrict__ Q, int n,
                                                                    const uint8_t *__restrict__ mask, const double *__restrict__ sums,
                                                                    int nblk, double *__restrict__ rows) {
  __shared__ double cen[6];
  __shared__ double part[kPoseThreads / 64][kMomRow];
  if (threadIdx.x == 0) {
    double pm[3], qm[3];
    pose_centroids(sums, nblk, pm, qm);
    for (int a = 0; a < 3; a++) { cen[a] = pm[a]; cen[3 + a] = qm[a]; }
  }
  __syncthreads();
  double acc[kMomRow];
#pragma unroll
  for (int a = 0; a < kMomRow; a++) acc[a] = 0.0;
  const int base = blockIdx.x * kPoseChunk + threadIdx.x;
  for (int k = 0; k < kPosePerThread; k++) {
    const int i = base + k * kPoseThreads;
    if (i >= n) break;
    if (mask && !mask[i]) continue;
    const double p0 = P[(size_t)i * 3 + 0] - cen[0], p1 = P[(size_t)i * 3 + 1] - cen[1], p2 = P[(size_t)i * 3 + 2] - cen[2];
    const double q0 = Q[(size_t)i * 3 + 0] - cen[3], q1 = Q[(size_t)i * 3 + 1] - cen[4], q2 = Q[(size_t)i * 3 + 2] - cen[5];
    acc[0] = fma(q0, p0, acc[0]); acc[1] = fma(q0, p1, acc[1]); acc[2] = fma(q0, p2, acc[2]);
    acc[3] = fma(q1, p0, acc[3]); acc[4] = fma(q1, p1, acc[4]); acc[5] = fma(q1, p2, acc[5]);
    acc[6] = fma(q2, p0, acc[6]); acc[7] = fma(q2, p1, acc[7]); acc[8] = fma(q2, p2, acc[8]);
    acc[9] = fma(p0, p0, acc[9]); acc[10] = fma(p0, p1, acc[10]); acc[11] = fma(p0, p2, acc[11]);
    acc[12] = fma(p1, p1, acc[12]); acc[13] = fma(p1, p2, acc[13]); acc[14] = fma(p2, p2, acc[14]);
    acc[15] += fma(q0, q0, fma(q1, q1, q2 * q2));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < kMomRow; a++) {
    const double v = wave_sum_f64(acc[a]);
    if (lane == 0) part[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMomRow) {
    double s = 0.0;
    for (int w = 0; w < kPoseThreads / 64; w++) s += part[w][threadIdx.x];
    rows[(size_t)blockIdx.x * kMomRow + threadIdx.x] = s;
  }
}

// lane a < 16 of a wave: moment a summed over the blocks in block order; broadcast through LDS by the callers
__device__ __forceinline__ double pose_moment_sum(const double *__restrict__ rows, int nblk, int a) {
  double s = 0.0;
  for (int b = 0; b < nblk; b++) s += rows[(size_t)b * kMomRow + a];
  return s;
}

// out_sel[2]: the winner and its count; out_R / out_t / out_s: the fit over its inliers (left alone on a status)
__global__ void __launch_bounds__(64) ransac_final_kernel(const double *__restrict__ sums, const double *__restrict__ moms, int nblk,
                                                          int with_scale, const PoseSelect *__restrict__ sel, double *__restrict__ out_R,
                                                          double *__restrict__ out_t, double *__restrict__ out_s, int32_t *__restrict__ out_sel) {
  __shared__ double S[kMomRow];
  if (threadIdx.x < kMomRow) S[threadIdx.x] = pose_moment_sum(moms, nblk, threadIdx.x);
  __syncthreads();
  if (threadIdx.x != 0) return;
  out_sel[0] = sel->winner;
  out_sel[1] = sel->count;
  if (sel->status != 0) return;
  double pm[3], qm[3], A[3][3];
  pose_centroids(sums, nblk, pm, qm);
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) A[a][b] = S[a * 3 + b];
  double R[3][3], t[3], s;
  pose_solve(A, S[9] + S[12] + S[14], pm, qm, with_scale != 0, R, t, &s);
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) out_R[a * 3 + b] = R[a][b];
    out_t[a] = t[a];
  }
  *out_s = s;
}

// ---- 9-DoF Adam ----

struct PoseAdamArgs {
  double lr, lambda_scale, lambda_rot, scale_min, scale_max;
  double start[14];   // t (3), q (4), qo (4), scale logits (3)
  int32_t iterations, loss_every, loss_capacity, pad;
};

// R = I + (2 / q.q) B(q)  (utils/geometry.py:43-72; q = (r, i, j, k))
__device__ __forceinline__ void quat_to_matrix(const double q[4], double R[3][3]) {
  const double r = q[0], i = q[1], j = q[2], k = q[3];
  const double ts = 2.0 / (r * r + i * i + j * j + k * k);
  R[0][0] = 1.0 - ts * (j * j + k * k); R[0][1] = ts * (i * j - k * r); R[0][2] = ts * (i * k + j * r);
  R[1][0] = ts * (i * j + k * r); R[1][1] = 1.0 - ts * (i * i + k * k); R[1][2] = ts * (j * k - i * r);
  R[2][0] = ts * (i * k - j * r); R[2][1] = ts * (j * k + i * r); R[2][2] = 1.0 - ts * (i * i + j * j);
}

// g = dL/dq from G = dL/dR: ts <G, dB/dq> + <G, B> dts/dq with dts/dq = -4 q / (q.q)^2 and ts B = R - I
__device__ __forceinline__ void quat_backward(const double q[4], const double R[3][3], const double G[3][3], double g[4]) {
  const double r = q[0], i = q[1], j = q[2], k = q[3];
  const double n = r * r + i * i + j * j + k * k, ts = 2.0 / n;
  double gb = 0.0;   // <G, ts B>
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) gb += G[a][b] * (R[a][b] - (a == b ? 1.0 : 0.0));
  const double w = -2.0 * gb / n;   // <G, B> dts/dq = (gb / ts) (-4 q / n^2) = -2 gb q / n
  g[0] = ts * (-k * G[0][1] + j * G[0][2] + k * G[1][0] - i * G[1][2] - j * G[2][0] + i * G[2][1]) + w * r;
  g[1] = ts * (j * G[0][1] + k * G[0][2] + j * G[1][0] - 2.0 * i * G[1][1] - r * G[1][2] + k * G[2][0] + r * G[2][1] - 2.0 * i * G[2][2]) + w * i;
  g[2] = ts * (-2.0 * j * G[0][0] + i * G[0][1] + r * G[0][2] + i * G[1][0] + k * G[1][2] - r * G[2][0] + k * G[2][1] - 2.0 * j * G[2][2]) + w * j;
  g[3] = ts * (-2.0 * k * G[0][0] - r * G[0][1] + i * G[0][2] + r * G[1][0] - 2.0 * k * G[1][1] + j * G[1][2] + i * G[2][0] + j * G[2][1]) + w * k;
}

__device__ __forceinline__ void mat3_mul(const double A[3][3], const double B[3][3], double C[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) C[a][b] = A[a][0] * B[0][b] + A[a][1] * B[1][b] + A[a][2] * B[2][b];
}

// One wave; lane 0 runs the chain.  out: R (9), t (3), s (3), Ro (9), the last step's loss.  With pc = p - pm, qc = q - qm,
// App = sum pc pc^T, Aqp = sum qc pc^T, sqq = sum qc.qc and d = M pm + t - qm:
//   sum |M p + t - q|^2 = tr(M App M^T) - 2 <M, Aqp> + sqq + N |d|^2
//   dL/dM = 2 (M App - Aqp + N d pm^T) / (3N),   dL/dt = 2 N d / (3N)
// The rotation term arccos(c)^2 with c = clamp((tr R - 1) / 2, -1, 1) has the derivative -arccos(c) / sqrt(1 - c^2) in tr R;
// where the reference's autograd gives NaN or an infinity (|c| >= 1: the identity, or a half turn) the kernel takes that
// derivative as 0 and goes on.
__global__ void __launch_bounds__(64) pose_adam_kernel(const double *__restrict__ sums, const double *__restrict__ moms, int nblk,
                                                       PoseAdamArgs args, double *__restrict__ out, double *__restrict__ loss_trace) {
  __shared__ double S[kMomRow];
  if (threadIdx.x < kMomRow) S[threadIdx.x] = pose_moment_sum(moms, nblk, threadIdx.x);
  __syncthreads();
  if (threadIdx.x != 0) return;
  double pm[3], qm[3];
  const double N = pose_centroids(sums, nblk, pm, qm);
  const double inv3n = 1.0 / (3.0 * N);
  double Aqp[3][3], App[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) Aqp[a][b] = S[a * 3 + b];
  App[0][0] = S[9]; App[0][1] = App[1][0] = S[10]; App[0][2] = App[2][0] = S[11];
  App[1][1] = S[12]; App[1][2] = App[2][1] = S[13]; App[2][2] = S[14];
  const double sqq = S[15];

  double par[14], m1[14], m2[14];
#pragma unroll
  for (int e = 0; e < 14; e++) { par[e] = args.start[e]; m1[e] = 0.0; m2[e] = 0.0; }
  const double b1 = 0.9, b2 = 0.999, eps = 1e-8, span = args.scale_max - args.scale_min;
  double b1t = 1.0, b2t = 1.0, loss = 0.0;
  int traced = 0;
  for (int it = 0; it < args.iterations; it++) {
    double R[3][3], Ro[3][3], sig[3], sc[3];
    quat_to_matrix(par + 3, R);
    quat_to_matrix(par + 7, Ro);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      sig[a] = 1.0 / (1.0 + exp(-par[11 + a]));
      sc[a] = args.scale_min + span * sig[a];
    }
    double SRo[3][3], K[3][3], M[3][3];   // K = Ro^T diag(s) Ro (symmetric), M = R K
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) SRo[a][b] = sc[a] * Ro[a][b];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) K[a][b] = Ro[0][a] * SRo[0][b] + Ro[1][a] * SRo[1][b] + Ro[2][a] * SRo[2][b];
    mat3_mul(R, K, M);
    double MA[3][3], d[3];
    mat3_mul(M, App, MA);
    double quad = 0.0, cross = 0.0, dd = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      d[a] = M[a][0] * pm[0] + M[a][1] * pm[1] + M[a][2] * pm[2] + par[a] - qm[a];
      dd += d[a] * d[a];
#pragma unroll
      for (int b = 0; b < 3; b++) { quad += MA[a][b] * M[a][b]; cross += M[a][b] * Aqp[a][b]; }
    }
    const double mean_s = (sc[0] + sc[1] + sc[2]) / 3.0;
    double reg_logit = 0.0, reg_mean = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      reg_logit += (par[11 + a] - 1.0) * (par[11 + a] - 1.0);
      reg_mean += (sc[a] - mean_s) * (sc[a] - mean_s);
    }
    const double c = fmin(fmax((R[0][0] + R[1][1] + R[2][2] - 1.0) * 0.5, -1.0), 1.0);
    const double theta = acos(c);
    loss = (quad - 2.0 * cross + sqq + N * dd) * inv3n + args.lambda_scale * (reg_logit + reg_mean) / 3.0 +
           args.lambda_rot * theta * theta;
    if (loss_trace && args.loss_every > 0 && (it + 1) % args.loss_every == 0 && traced < args.loss_capacity)
      loss_trace[traced++] = loss;

    double g[14], G[3][3];   // G = dL/dM
#pragma unroll
    for (int a = 0; a < 3; a++) {
      g[a] = 2.0 * N * d[a] * inv3n;
#pragma unroll
      for (int b = 0; b < 3; b++) G[a][b] = 2.0 * (MA[a][b] - Aqp[a][b] + N * d[a] * pm[b]) * inv3n;
    }
    double GR[3][3], H[3][3];   // dL/dR = G K^T = G K, H = dL/dK = R^T G
    mat3_mul(G, K, GR);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) H[a][b] = R[0][a] * G[0][b] + R[1][a] * G[1][b] + R[2][a] * G[2][b];
    const double sin2 = 1.0 - c * c;
    const double dreg = sin2 > 0.0 ? -theta / sqrt(sin2) : 0.0;   // d theta^2 / d tr R
#pragma unroll
    for (int a = 0; a < 3; a++) GR[a][a] += args.lambda_rot * dreg;
    quat_backward(par + 3, R, GR, g + 3);
    // K = Ro^T diag(s) Ro: dL/dRo = diag(s) Ro (H + H^T), dL/ds_a = (Ro H Ro^T)_aa
    double Hs[3][3], GRo[3][3], RoH[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) Hs[a][b] = H[a][b] + H[b][a];
    mat3_mul(SRo, Hs, GRo);
    quat_backward(par + 7, Ro, GRo, g + 7);
    mat3_mul(Ro, H, RoH);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double ds = RoH[a][0] * Ro[a][0] + RoH[a][1] * Ro[a][1] + RoH[a][2] * Ro[a][2] +
                        args.lambda_scale * 2.0 * (sc[a] - mean_s) / 3.0;
      g[11 + a] = ds * span * sig[a] * (1.0 - sig[a]) + args.lambda_scale * 2.0 * (par[11 + a] - 1.0) / 3.0;
    }
    // torch.optim.Adam: betas 0.9 / 0.999, eps 1e-8, bias corrections, no weight decay
    b1t *= b1;
    b2t *= b2;
    const double step = args.lr / (1.0 - b1t), rs2 = 1.0 / sqrt(1.0 - b2t);
#pragma unroll
    for (int e = 0; e < 14; e++) {
      m1[e] = b1 * m1[e] + (1.0 - b1) * g[e];
      m2[e] = b2 * m2[e] + (1.0 - b2) * g[e] * g[e];
      par[e] -= step * m1[e] / (sqrt(m2[e]) * rs2 + eps);
    }
  }
  double R[3][3], Ro[3][3];
  quat_to_matrix(par + 3, R);
  quat_to_matrix(par + 7, Ro);
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) { out[a * 3 + b] = R[a][b]; out[15 + a * 3 + b] = Ro[a][b]; }
    out[9 + a] = par[a];
    out[12 + a] = args.scale_min + span / (1.0 + exp(-par[11 + a]));
  }
  out[24] = loss;
}

// ---- host ----

int check_pairs(const char *what, const void *source, const void *target, int32_t n, const void *workspace, size_t workspace_bytes,
                const PoseLayout &L) {
  if (n < 3) { set_error("%s: at least 3 pairs are required (got %d)", what, n); return SCORP_ERR_INVALID; }
  if (!source || !target || !workspace) { set_error("%s: NULL argument", what); return SCORP_ERR_INVALID; }
  if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) {
    set_error("%s: workspace too small or not 256-byte aligned (%zu < %zu)", what, workspace_bytes, L.total);
    return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

int ransac_impl(const double *P, const double *Q, int32_t n, const int32_t *samples, int32_t nh, double threshold,
                double min_inlier_ratio, int32_t method, double *out_R, double *out_t, double *out_s, int32_t *out_sel,
                int32_t *out_counts, uint8_t *out_mask, void *workspace, size_t workspace_bytes, hipStream_t stream) {
  const PoseLayout L(n, nh);
  if (int e = check_pairs("pose_ransac", P, Q, n, workspace, workspace_bytes, L)) return e;
  if (nh < 1 || nh > 65535) { set_error("pose_ransac: n_hypotheses must be in [1, 65535]"); return SCORP_ERR_INVALID; }
  if (!std::isfinite(threshold)) { set_error("pose_ransac: threshold is not finite"); return SCORP_ERR_INVALID; }
  if (std::isnan(min_inlier_ratio)) { set_error("pose_ransac: min_inlier_ratio is NaN"); return SCORP_ERR_INVALID; }
  if (method != SCORP_POSE_UMEYAMA && method != SCORP_POSE_KABSCH) { set_error("pose_ransac: unknown method %d", method); return SCORP_ERR_INVALID; }
  if (!samples || !out_R || !out_t || !out_s || !out_sel || !out_counts || !out_mask) {
    set_error("pose_ransac: NULL argument"); return SCORP_ERR_INVALID;
  }
  char *w = (char *)workspace;
  PoseSelect *sel = (PoseSelect *)(w + L.sel);
  double *models = (double *)(w + L.models), *sums = (double *)(w + L.sums), *moms = (double *)(w + L.moms);
  const int nblk = (int)L.nblk, with_scale = method == SCORP_POSE_UMEYAMA;
  SCORP_HIP_CHECK(hipMemsetAsync(sel, 0, sizeof(PoseSelect), stream));
  SCORP_HIP_CHECK(hipMemsetAsync(out_counts, 0, (size_t)nh * 4, stream));
  ransac_fit_kernel<<<(nh + 63) / 64, 64, 0, stream>>>(P, Q, n, samples, nh, with_scale, models, sel);
  SCORP_KERNEL_CHECK("ransac_fit", 0, stream);
  ransac_count_kernel<<<dim3(nblk, nh), kPoseThreads, 0, stream>>>(P, Q, n, models, threshold, out_counts);
  SCORP_KERNEL_CHECK("ransac_count", 0, stream);
  ransac_select_kernel<<<1, 64, 0, stream>>>(out_counts, nh, min_inlier_ratio > 0.0 ? min_inlier_ratio * (double)n : -1.0, sel);
  SCORP_KERNEL_CHECK("ransac_select", 0, stream);
  pose_sums_kernel<<<nblk, kPoseThreads, 0, stream>>>(P, Q, n, models, sel, threshold, out_mask, sums);
  SCORP_KERNEL_CHECK("pose_sums", 0, stream);
  pose_moments_kernel<<<nblk, kPoseThreads, 0, stream>>>(P, Q, n, out_mask, sums, nblk, moms);
  SCORP_KERNEL_CHECK("pose_moments", 0, stream);
  ransac_final_kernel<<<1, 64, 0, stream>>>(sums, moms, nblk, with_scale, sel, out_R, out_t, out_s, out_sel);
  SCORP_KERNEL_CHECK("ransac_final", 0, stream);
  PoseSelect host;
  SCORP_HIP_CHECK(hipMemcpyAsync(&host, sel, sizeof(PoseSelect), hipMemcpyDeviceToHost, stream));
  SCORP_HIP_CHECK(hipStreamSynchronize(stream));
  if (host.status & 1) { set_error("pose_ransac: a sample index outside [0, %d)", n); return SCORP_ERR_INVALID; }
  if (host.status & 2) { set_error("pose_ransac: the best hypothesis has %d inliers, fewer than 3", host.count); return SCORP_ERR_NO_INLIERS; }
  return SCORP_OK;
}

int adam_impl(const double *P, const double *Q, int32_t n, int32_t iterations, double lr, double lambda_reg_scale,
              double lambda_reg_rot, double scale_min, double scale_max, const double *init_scale, double *out,
              double *out_loss, int32_t loss_every, int32_t loss_capacity, void *workspace, size_t workspace_bytes,
              hipStream_t stream) {
  const PoseLayout L(n, 1);
  if (int e = check_pairs("pose_adam_9dof", P, Q, n, workspace, workspace_bytes, L)) return e;
  if (iterations < 0 || iterations > kMaxAdamIterations) {
    set_error("pose_adam_9dof: iterations must be in [0, %d]", kMaxAdamIterations); return SCORP_ERR_INVALID;
  }
  if (!init_scale || !out) { set_error("pose_adam_9dof: NULL argument"); return SCORP_ERR_INVALID; }
  if (!std::isfinite(lr) || !std::isfinite(lambda_reg_scale) || !std::isfinite(lambda_reg_rot) || !std::isfinite(scale_min) ||
      !std::isfinite(scale_max) || !(scale_max > scale_min)) {
    set_error("pose_adam_9dof: lr, the lambdas and the scale bounds must be finite, scale_max > scale_min"); return SCORP_ERR_INVALID;
  }
  if (out_loss && (loss_every < 1 || loss_capacity < 0)) { set_error("pose_adam_9dof: loss_every < 1 with a loss buffer"); return SCORP_ERR_INVALID; }
  PoseAdamArgs a{};
  a.lr = lr; a.lambda_scale = lambda_reg_scale; a.lambda_rot = lambda_reg_rot; a.scale_min = scale_min; a.scale_max = scale_max;
  a.iterations = iterations; a.loss_every = out_loss ? loss_every : 0; a.loss_capacity = out_loss ? loss_capacity : 0;
  // the reference's start (utils/solution.py:387-399), its constants rounded to fp32 as there
  double s0[3] = {init_scale[0], init_scale[1], init_scale[2]};
  bool inside = true;
  for (int k = 0; k < 3; k++) inside = inside && s0[k] >= scale_min && s0[k] <= scale_max;   // (a NaN goes to the mid-point too)
  if (!inside) s0[0] = s0[1] = s0[2] = scale_min + (scale_max - scale_min) / 2;
  const double start[11] = {(double)0.01f, (double)0.01f, (double)0.01f, (double)0.9f, (double)0.01f, (double)0.01f, (double)0.01f,
                            1.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < 11; k++) a.start[k] = start[k];
  for (int k = 0; k < 3; k++) {
    const double u = (s0[k] - scale_min) / (scale_max - scale_min);
    a.start[11 + k] = std::log(u / (1.0 - u));
  }
  char *w = (char *)workspace;
  double *sums = (double *)(w + L.sums), *moms = (double *)(w + L.moms);
  const int nblk = (int)L.nblk;
  pose_sums_kernel<<<nblk, kPoseThreads, 0, stream>>>(P, Q, n, nullptr, nullptr, 0.0, nullptr, sums);
  SCORP_KERNEL_CHECK("pose_sums", 0, stream);
  pose_moments_kernel<<<nblk, kPoseThreads, 0, stream>>>(P, Q, n, nullptr, sums, nblk, moms);
  SCORP_KERNEL_CHECK("pose_moments", 0, stream);
  pose_adam_kernel<<<1, 64, 0, stream>>>(sums, moms, nblk, a, out, out_loss);
  SCORP_KERNEL_CHECK("pose_adam", 0, stream);
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_pose_fit_workspace_bytes(int32_t n_pairs, int32_t n_hypotheses) {
  return PoseLayout(n_pairs, n_hypotheses).total;
}

extern "C" int scorp_pose_ransac(const double *source, const double *target, int32_t n_pairs, const int32_t *samples,
                                 int32_t n_hypotheses, double threshold, double min_inlier_ratio, int32_t method, double *out_R,
                                 double *out_t, double *out_s, int32_t *out_winner, int32_t *out_counts, uint8_t *out_inlier_mask,
                                 void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  return ransac_impl(source, target, n_pairs, samples, n_hypotheses, threshold, min_inlier_ratio, method, out_R, out_t, out_s,
                     out_winner, out_counts, out_inlier_mask, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int scorp_pose_adam_9dof(const double *source, const double *target, int32_t n_pairs, int32_t iterations, double lr,
                                    double lambda_reg_scale, double lambda_reg_rot, double scale_min, double scale_max,
                                    const double *init_scale, double *out, double *out_loss, int32_t loss_every,
                                    int32_t loss_capacity, void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  return adam_impl(source, target, n_pairs, iterations, lr, lambda_reg_scale, lambda_reg_rot, scale_min, scale_max, init_scale, out,
                   out_loss, loss_every, loss_capacity, workspace, workspace_bytes, (hipStream_t)stream);
}
