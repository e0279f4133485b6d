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
// The grid, the sorts, the ring search and the host calls that build them are in icp_search.hpp, shared with
// icp_plane.hip.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "icp_search.hpp"
#include "svd3.hpp"

namespace scorp {
namespace {

constexpr int kIcpRow = 18;                              // doubles per partial row: 17 sums + pad

// ---- the correspondence pass ----

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

int icp_impl(const float *source, int32_t ns, const float *target, int32_t nt, const double *inits, int32_t ni, double r,
             int32_t max_iteration, double rel_fitness, double rel_rmse, double *out_T, double *out_fitness, double *out_rmse,
             int32_t *out_iters, void *workspace, size_t workspace_bytes, hipStream_t stream) {
  if (int e = icp_check_args("icp", r, ns, nt, max_iteration, ni,
                             source && target && inits && out_T && out_fitness && out_rmse && out_iters && workspace))
    return e;
  const IcpLayout L(ns, nt, ni, kIcpRow);
  if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) {
    set_error("icp: workspace too small or not 256-byte aligned (%zu < %zu)", workspace_bytes, L.total);
    return SCORP_ERR_INVALID;
  }
  const IcpWorkspace W(workspace, L);
  if (int e = icp_build_target(target, nt, L, W, stream)) return e;
  if (int e = icp_build_source(source, ns, L, W, stream)) return e;
  icp_init_kernel<<<(ni + 63) / 64, 64, 0, stream>>>(inits, ni, out_T, out_fitness, out_rmse, out_iters, W.active);
  SCORP_KERNEL_CHECK("icp_init", 0, stream);

  const int nblk = (ns + kIcpChunk - 1) / kIcpChunk;
  const double r2 = r * r;
  const float r2f = (float)r2 * (1.0f + 1e-5f);   // the fp32 search keeps slightly more; the pair test is float64
  return icp_iterate(ni, max_iteration, W.active, stream, [&](int k) -> int {
    icp_pass_kernel<<<dim3(nblk, ni), kIcpThreads, 0, stream>>>(W.sp, ns, W.tq, target, W.cell_start, W.g, out_T, W.active, r2, r2f,
                                                                W.rows);
    SCORP_KERNEL_CHECK("icp_pass", 0, stream);
    icp_solve_kernel<<<ni, 64, 0, stream>>>(W.rows, nblk, ns, W.g, k, max_iteration, rel_fitness, rel_rmse, out_T, out_fitness,
                                            out_rmse, out_iters, W.active);
    SCORP_KERNEL_CHECK("icp_solve", 0, stream);
    return SCORP_OK;
  });
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_icp_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init) {
  return IcpLayout(n_source, n_target, n_init, kIcpRow).total;
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
