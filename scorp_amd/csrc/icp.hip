// icp.hip — multi-start ICP (Open3D registration_icp, every init of a call in one batch) with one of four estimators, the
// normal estimation that feeds the second one when the target brings no normals, and the colour gradients that feed the
// fourth.  The rules are written down in
// include/scorp_gs.h.  The reference's alignment scripts run the point-to-point form from 67 initial poses with
// max_iteration = 400 (align_3dgs_clpe_9dof.py:42-115 get_ICP_fitting_transformation_best).
//
// Built once per call (icp_search.hpp, shared with mesh_distance.hip):
//   * the target Q in a uniform grid (cell edge from the point density, not from r), its points sorted by cell (a stable
//     LSD radix sort on the cell id) as float4 {q - c_t (fp32), original index};
//   * the source P sorted by a 30-bit Morton code over its own bounding box (same sort), so that the 64 queries of a wave
//     stay neighbours under every rigid T_i and the target cells they visit are shared through L2; the generalized
//     estimator's source covariances, and the coloured estimator's source intensities, are gathered into that order once,
//     behind the shared workspace.
// Per iteration (no host synchronisation; the host reads the active flags every kIcpPollEvery iterations), one body each
// for every estimator (icp_pass, icp_solve) behind thin kernels:
//   * icp_pass_kernel / icp_plane_pass_kernel / icp_generalized_pass_kernel / icp_colored_pass_kernel, grid (source blocks,
//     inits): x = T_i p in float64 (the cumulative transform
//     on the original point), exact nearest target point q within r by an outward ring search over the grid in fp32, the
//     chosen pair's d^2 in float64 relative to c_t, then the estimator's sums: one fixed row per block, no float atomics;
//   * icp_solve_kernel / icp_plane_solve_kernel (the generalized and coloured estimators' too), one wave per init: the rows reduced in a fixed order, fitness / rmse, the
//     stop rule, the estimator's update [R | tau] about c_t, composed onto T in float64.
// The estimators differ in their sums and their update alone:
//   * PointToPoint (TransformationEstimationPointToPoint, no scaling): 17 sums (c, sum d^2, the first and second moments
//     of x and q); Umeyama without scale by a 3x3 one-sided Jacobi SVD in float64 (svd3.hpp), reflection rule;
//   * PointToPlane (TransformationEstimationPointToPlane, no robust kernel): with the normal n of q, J = [(x x n) / s ; n],
//     rho = n . (x - q), 29 sums (c, sum d^2, the 21 of the upper triangle of J J^T, the 6 of J rho); A = V L V^T by
//     cyclic Jacobi in float64 (A and V in LDS), the minimum-norm step over the eigenvalues above 1e-12 of the largest,
//     R = Rz Ry Rx;
//   * Generalized (Segal et al. 2009): with the covariances C_p, C_q of the pair, W = (C_q + A_T C_p A_T^T)^-1 by cofactors
//     where that matrix is positive definite, J = [-[x]x / s | I], the same 29 sums (J^T W J, J^T W (x - q)) and
//     PointToPlane's solve; W = n n^T would give PointToPlane's sums;
//   * Colored (Park, Zhou, Koltun 2017): with the normal n, the colour gradient d and the intensity I_q of q and the
//     intensity I_p of the source point, PointToPlane's term at the weight lambda and the same term on d with
//     rho_C = d . (x - q) + (I_q - I_p) at 1 - lambda, the same 29 sums and PointToPlane's solve; lambda = 1 gives
//     PointToPlane's sums bit for bit.
// A block's row depends only on (its source range, its init's T), and the rows are reduced in a fixed order: two calls
// give the same bits, and init j run alone gives the bits of row j of a batch.
// scorp_estimate_normals, one thread per point: its k exact nearest neighbours by the same outward ring walk, the list of
// the k best (d^2, index) kept sorted in LDS (one column per lane; icp_search.hpp's KBest, the list of the FPFH
// search too), their float64 covariance, the eigenvector of its smallest eigenvalue from svd3.hpp.
// scorp_color_gradients, one thread per point: the least-squares gradient of the intensity over the stored neighbour row,
// held in the tangent plane by a normal-normal term in its 3x3 system, solved through svd3.hpp.
#include <cmath>

#include "common.hpp"
#include "icp_search.hpp"
#include "svd3.hpp"

namespace scorp {
namespace {

constexpr int kNormalsThreads = kKBestLanes;
constexpr int kNormalsMaxK = 32;

// ---- the estimators: kSums sums per pair in a row of kRow doubles (the sums + pad), sums 0 and 1 are c and sum d^2 ----

// Row layout: [c, sum d^2, sum x (3), sum q (3), sum x_a q_b (9, a-major), pad]
struct PointToPoint {
  static constexpr int kSums = 17, kRow = 18;
  static constexpr bool kNormals = false, kCovariances = false, kColors = false;
  static constexpr const char *kWho = "icp";
  __device__ PointToPoint(const IcpGrid *, const double *, const float *) {}

  __device__ __forceinline__ void accumulate(double (&acc)[kSums], const double x[3], const double q[3], const double[3], double d2,
                                             const float *, int, int) const {
    acc[0] += 1.0;
    acc[1] += d2;
    acc[2] += x[0]; acc[3] += x[1]; acc[4] += x[2];
    acc[5] += q[0]; acc[6] += q[1]; acc[7] += q[2];
    acc[8] = fma(x[0], q[0], acc[8]); acc[9] = fma(x[0], q[1], acc[9]); acc[10] = fma(x[0], q[2], acc[10]);
    acc[11] = fma(x[1], q[0], acc[11]); acc[12] = fma(x[1], q[1], acc[12]); acc[13] = fma(x[1], q[2], acc[13]);
    acc[14] = fma(x[2], q[0], acc[14]); acc[15] = fma(x[2], q[1], acc[15]); acc[16] = fma(x[2], q[2], acc[16]);
  }

  // Umeyama without scale: Sigma = (1/c) sum (q - qm)(x - xm)^T = U S V^T, R = U D V^T, tau = qm - R xm (relative to c_t)
  static __device__ __forceinline__ bool update(const double *S, double c, const IcpGrid *, double R[3][3], double tau[3]) {
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
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) R[a][b] = U[a][0] * V[b][0] + U[a][1] * V[b][1] + dsign * U[a][2] * V[b][2];
    for (int a = 0; a < 3; a++) {
      double rx = 0.0;
      for (int b = 0; b < 3; b++) rx += R[a][b] * xm[b];
      tau[a] = qm[a] - rx;
    }
    return true;
  }
};

// Row layout: [c, sum d^2, A_00 A_01 .. A_05 A_11 .. A_55 (21), b (6), pad]
struct PointToPlane {
  static constexpr int kSums = 29, kRow = 30;
  static constexpr bool kNormals = true, kCovariances = false, kColors = false;
  static constexpr const char *kWho = "icp point-to-plane";
  double s;
  __device__ PointToPlane(const IcpGrid *g, const double *, const float *) : s(scale(g)) {}

  // s: half the largest edge of the target's bounding box, 1 if that is 0 (it brings the rotational part of J to the
  // magnitude of the translational one)
  static __device__ __forceinline__ double scale(const IcpGrid *__restrict__ g) {
    double e = 0.0;
    for (int d = 0; d < 3; d++) e = fmax(e, (double)g->thi[d] - (double)g->tlo[d]);
    return e > 0.0 ? 0.5 * e : 1.0;
  }

  __device__ __forceinline__ void accumulate(double (&acc)[kSums], const double x[3], const double[3], const double u[3], double d2,
                                             const float *__restrict__ tn, int id, int) const {
    const double n0 = tn[(size_t)id * 3 + 0], n1 = tn[(size_t)id * 3 + 1], n2 = tn[(size_t)id * 3 + 2];
    double J[6];
    J[0] = (x[1] * n2 - x[2] * n1) / s;
    J[1] = (x[2] * n0 - x[0] * n2) / s;
    J[2] = (x[0] * n1 - x[1] * n0) / s;
    J[3] = n0; J[4] = n1; J[5] = n2;
    const double rho = fma(n0, u[0], fma(n1, u[1], n2 * u[2]));
    acc[0] += 1.0;
    acc[1] += d2;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b = a; b < 6; b++) {
        const int e = 2 + a * 6 - a * (a - 1) / 2 + (b - a);
        acc[e] = fma(J[a], J[b], acc[e]);
      }
      acc[23 + a] = fma(J[a], rho, acc[23 + a]);
    }
  }

  // A = V L V^T, the minimum-norm step xi, R = Rz Ry Rx of xi[0:3] / s, tau = xi[3:6]; false when nothing constrains it
  static __device__ __forceinline__ bool update(const double *S, double, const IcpGrid *g, double R[3][3], double tau[3]) {
    __shared__ double A[6][6], V[6][6];   // the one lane that solves indexes them by loop variables: LDS, not registers
    double b6[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b = a; b < 6; b++) {
        const double v = S[2 + a * 6 - a * (a - 1) / 2 + (b - a)];
        A[a][b] = v;
        A[b][a] = v;
      }
#pragma unroll
      for (int b = 0; b < 6; b++) V[a][b] = a == b ? 1.0 : 0.0;
      b6[a] = S[23 + a];
    }
    // cyclic Jacobi: every (p, q) of a sweep in row order, until a sweep rotates nothing
    for (int sweep = 0; sweep < 64; sweep++) {
      bool rotated = false;
      for (int p = 0; p < 5; p++) {
        for (int q = p + 1; q < 6; q++) {
          const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
          if (apq == 0.0 || fabs(apq) <= 1e-17 * sqrt(fabs(app) * fabs(aqq))) continue;
          rotated = true;
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
          A[p][p] = app - t * apq;
          A[q][q] = aqq + t * apq;
          A[p][q] = 0.0;
          A[q][p] = 0.0;
          for (int r = 0; r < 6; r++) {
            if (r != p && r != q) {
              const double arp = A[r][p], arq = A[r][q];
              const double np_ = cs * arp - sn * arq, nq_ = sn * arp + cs * arq;
              A[r][p] = np_; A[p][r] = np_;
              A[r][q] = nq_; A[q][r] = nq_;
            }
            const double vp = V[r][p], vq = V[r][q];
            V[r][p] = cs * vp - sn * vq;
            V[r][q] = sn * vp + cs * vq;
          }
        }
      }
      if (!rotated) break;
    }
    double lmax = 0.0;
    for (int i = 0; i < 6; i++) lmax = fmax(lmax, A[i][i]);
    if (!(lmax > 0.0)) return false;   // no constraint at all (every normal zero): the identity
    // the minimum-norm step: only along the directions the pairs constrain
    double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 6; i++) {
      const double l = A[i][i];
      if (!(l > 1e-12 * lmax)) continue;
      double vb = 0.0;
#pragma unroll
      for (int a = 0; a < 6; a++) vb += V[a][i] * b6[a];
      const double f = vb / l;
#pragma unroll
      for (int a = 0; a < 6; a++) xi[a] -= V[a][i] * f;
    }
    const double s = scale(g);
    const double wx = xi[0] / s, wy = xi[1] / s, wz = xi[2] / s;
    const double cx = cos(wx), sx = sin(wx), cy = cos(wy), sy = sin(wy), cz = cos(wz), sz = sin(wz);
    // R = Rz(wz) Ry(wy) Rx(wx)
    R[0][0] = cz * cy; R[0][1] = cz * sy * sx - sz * cx; R[0][2] = cz * sy * cx + sz * sx;
    R[1][0] = sz * cy; R[1][1] = sz * sy * sx + cz * cx; R[1][2] = sz * sy * cx - cz * sx;
    R[2][0] = -sy; R[2][1] = cy * sx; R[2][2] = cy * cx;
    for (int a = 0; a < 3; a++) tau[a] = xi[3 + a];
    return true;
  }
};

// Row layout and solve: PointToPlane's (the 21 sums of J^T W J, the 6 of J^T W u; icp_plane_solve_kernel reduces them).
// sc: the source's covariances in the order of W.sp; the target's come by the pair's original index, as normals do.
struct Generalized {
  static constexpr int kSums = PointToPlane::kSums, kRow = PointToPlane::kRow;
  static constexpr bool kNormals = true, kCovariances = true, kColors = false;
  static constexpr const char *kWho = "icp generalized";
  double s;
  double a00, a01, a02, a10, a11, a12, a20, a21, a22;   // A_T: the rotation block of the init's T, uniform per block
  const float *__restrict__ sc;
  __device__ Generalized(const IcpGrid *g, const double *M, const float *source_covariances)
      : s(PointToPlane::scale(g)), a00(M[0]), a01(M[1]), a02(M[2]), a10(M[4]), a11(M[5]), a12(M[6]), a20(M[8]), a21(M[9]),
        a22(M[10]), sc(source_covariances) {}

  static constexpr int at(int a, int b) { return 2 + a * 6 - a * (a - 1) / 2 + (b - a); }   // A_ab, a <= b, in the row

  __device__ __forceinline__ void accumulate(double (&acc)[kSums], const double x[3], const double[3], const double u[3], double d2,
                                             const float *__restrict__ tc, int id, int i) const {
    acc[0] += 1.0;
    acc[1] += d2;
    double w00, w01, w02, w11, w12, w22;
    {
      const float *__restrict__ cp = sc + (size_t)i * 6, *__restrict__ cq = tc + (size_t)id * 6;
      const double p0 = cp[0], p1 = cp[1], p2 = cp[2], p3 = cp[3], p4 = cp[4], p5 = cp[5];
      // B = A_T C_p, then the upper triangle of M = C_q + B A_T^T
      const double b00 = fma(a00, p0, fma(a01, p1, a02 * p2)), b01 = fma(a00, p1, fma(a01, p3, a02 * p4)),
                   b02 = fma(a00, p2, fma(a01, p4, a02 * p5));
      const double b10 = fma(a10, p0, fma(a11, p1, a12 * p2)), b11 = fma(a10, p1, fma(a11, p3, a12 * p4)),
                   b12 = fma(a10, p2, fma(a11, p4, a12 * p5));
      const double b20 = fma(a20, p0, fma(a21, p1, a22 * p2)), b21 = fma(a20, p1, fma(a21, p3, a22 * p4)),
                   b22 = fma(a20, p2, fma(a21, p4, a22 * p5));
      const double m00 = (double)cq[0] + fma(b00, a00, fma(b01, a01, b02 * a02));
      const double m01 = (double)cq[1] + fma(b00, a10, fma(b01, a11, b02 * a12));
      const double m02 = (double)cq[2] + fma(b00, a20, fma(b01, a21, b02 * a22));
      const double m11 = (double)cq[3] + fma(b10, a10, fma(b11, a11, b12 * a12));
      const double m12 = (double)cq[4] + fma(b10, a20, fma(b11, a21, b12 * a22));
      const double m22 = (double)cq[5] + fma(b20, a20, fma(b21, a21, b22 * a22));
      // W = M^-1 by cofactors; M must be finite and positive definite (Sylvester), or the pair adds nothing more
      const double k00 = m11 * m22 - m12 * m12, k01 = m02 * m12 - m01 * m22, k02 = m01 * m12 - m02 * m11;
      const double k11 = m00 * m22 - m02 * m02, k12 = m01 * m02 - m00 * m12, k22 = m00 * m11 - m01 * m01;
      const double det = fma(m00, k00, fma(m01, k01, m02 * k02));
      const bool finite = isfinite(m00) && isfinite(m01) && isfinite(m02) && isfinite(m11) && isfinite(m12) && isfinite(m22);
      if (!(finite && m00 > 0.0 && k22 > 0.0 && det > 0.0)) return;
      w00 = k00 / det; w01 = k01 / det; w02 = k02 / det; w11 = k11 / det; w12 = k12 / det; w22 = k22 / det;
    }
    // J = [ -[x]x / s | I ]: with y = x / s its rotational columns are g_a = e_a cross y
    const double y0 = x[0] / s, y1 = x[1] / s, y2 = x[2] / s;
    {  // b = J^T W u = [ y cross (W u) ; W u ]
      const double v0 = fma(w00, u[0], fma(w01, u[1], w02 * u[2])), v1 = fma(w01, u[0], fma(w11, u[1], w12 * u[2])),
                   v2 = fma(w02, u[0], fma(w12, u[1], w22 * u[2]));
      acc[23] += y1 * v2 - y2 * v1;
      acc[24] += y2 * v0 - y0 * v2;
      acc[25] += y0 * v1 - y1 * v0;
      acc[26] += v0; acc[27] += v1; acc[28] += v2;
    }
    // A = J^T W J, a column k = W g_a of W J at a time: A_ba = g_b . k for b <= a, A_a(3+c) = k_c, the last block W
    {
      const double k0 = y1 * w02 - y2 * w01, k1 = y1 * w12 - y2 * w11, k2 = y1 * w22 - y2 * w12;   // g_0 = (0, -y2, y1)
      acc[at(0, 0)] += y1 * k2 - y2 * k1;
      acc[at(0, 3)] += k0; acc[at(0, 4)] += k1; acc[at(0, 5)] += k2;
    }
    {
      const double k0 = y2 * w00 - y0 * w02, k1 = y2 * w01 - y0 * w12, k2 = y2 * w02 - y0 * w22;   // g_1 = (y2, 0, -y0)
      acc[at(0, 1)] += y1 * k2 - y2 * k1;
      acc[at(1, 1)] += y2 * k0 - y0 * k2;
      acc[at(1, 3)] += k0; acc[at(1, 4)] += k1; acc[at(1, 5)] += k2;
    }
    {
      const double k0 = y0 * w01 - y1 * w00, k1 = y0 * w11 - y1 * w01, k2 = y0 * w12 - y1 * w02;   // g_2 = (-y1, y0, 0)
      acc[at(0, 2)] += y1 * k2 - y2 * k1;
      acc[at(1, 2)] += y2 * k0 - y0 * k2;
      acc[at(2, 2)] += y0 * k1 - y1 * k0;
      acc[at(2, 3)] += k0; acc[at(2, 4)] += k1; acc[at(2, 5)] += k2;
    }
    acc[at(3, 3)] += w00; acc[at(3, 4)] += w01; acc[at(3, 5)] += w02;
    acc[at(4, 4)] += w11; acc[at(4, 5)] += w12;
    acc[at(5, 5)] += w22;
  }
};

// what the Colored estimator reads besides the normals: the target's colour gradients and intensities by the pair's
// original index, and the weight of the geometric term
struct IcpColors {
  const float *__restrict__ target_gradients, *__restrict__ target_intensity;
  double lambda;
};

// Row layout and solve: PointToPlane's (A = sum lambda J_G J_G^T + (1 - lambda) J_C J_C^T, b likewise with rho_G, rho_C).
// si: the source's intensities in the order of W.sp; the target's normals, gradients and intensities come by the pair's
// original index.  lambda = 1 leaves PointToPlane's sums bit for bit.
struct Colored {
  static constexpr int kSums = PointToPlane::kSums, kRow = PointToPlane::kRow;
  static constexpr bool kNormals = true, kCovariances = false, kColors = true;
  static constexpr const char *kWho = "icp colored";
  double s, wg, wc;
  const float *__restrict__ si, *__restrict__ tg, *__restrict__ ti;
  __device__ Colored(const IcpGrid *g, const double *, const float *source_intensity, const IcpColors &c)
      : s(PointToPlane::scale(g)), wg(c.lambda), wc(1.0 - c.lambda), si(source_intensity), tg(c.target_gradients),
        ti(c.target_intensity) {}

  // one term: acc += w J J^T, w J rho with J = [(x cross v) / s ; v]
  __device__ __forceinline__ void term(double (&acc)[kSums], const double x[3], double v0, double v1, double v2, double rho,
                                       double w) const {
    double J[6], wJ[6];
    J[0] = (x[1] * v2 - x[2] * v1) / s;
    J[1] = (x[2] * v0 - x[0] * v2) / s;
    J[2] = (x[0] * v1 - x[1] * v0) / s;
    J[3] = v0; J[4] = v1; J[5] = v2;
#pragma unroll
    for (int a = 0; a < 6; a++) wJ[a] = w * J[a];
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b = a; b < 6; b++) {
        const int e = 2 + a * 6 - a * (a - 1) / 2 + (b - a);
        acc[e] = fma(wJ[a], J[b], acc[e]);
      }
      acc[23 + a] = fma(wJ[a], rho, acc[23 + a]);
    }
  }

  __device__ __forceinline__ void accumulate(double (&acc)[kSums], const double x[3], const double[3], const double u[3], double d2,
                                             const float *__restrict__ tn, int id, int i) const {
    acc[0] += 1.0;
    acc[1] += d2;
    {
      const double n0 = tn[(size_t)id * 3 + 0], n1 = tn[(size_t)id * 3 + 1], n2 = tn[(size_t)id * 3 + 2];
      term(acc, x, n0, n1, n2, fma(n0, u[0], fma(n1, u[1], n2 * u[2])), wg);
    }
    {
      const double d0 = tg[(size_t)id * 3 + 0], d1 = tg[(size_t)id * 3 + 1], dz = tg[(size_t)id * 3 + 2];
      const double di = (double)ti[id] - (double)si[i];
      term(acc, x, d0, d1, dz, fma(d0, u[0], fma(d1, u[1], dz * u[2])) + di, wc);
    }
  }
};

// ---- the correspondence pass ----

// grid (source blocks, inits); tn: the target's normals or covariances where Est::kNormals; sc: the source's covariances
// (Est::kCovariances) or intensities (Est::kColors) in sp's order; extra: what else the estimator's constructor takes
template <class Est, class... Extra>
__device__ __forceinline__ void icp_pass(const float4 *__restrict__ sp, const float *__restrict__ sc, int ns,
                                         const float4 *__restrict__ tq, const float *__restrict__ tgt, const float *__restrict__ tn,
                                         const uint32_t *__restrict__ cell_start, const IcpGrid *__restrict__ g,
                                         const double *__restrict__ T, const int32_t *__restrict__ active, double r2, float r2f,
                                         double *__restrict__ rows, const Extra &...extra) {
  const int j = blockIdx.y;
  if (!active[j]) return;
  const double *M = T + (size_t)j * 16;
  const double m00 = M[0], m01 = M[1], m02 = M[2], m03 = M[3] - g->ct[0];
  const double m10 = M[4], m11 = M[5], m12 = M[6], m13 = M[7] - g->ct[1];
  const double m20 = M[8], m21 = M[9], m22 = M[10], m23 = M[11] - g->ct[2];
  const double c0 = g->ct[0], c1 = g->ct[1], c2 = g->ct[2];
  const Est est(g, M, sc, extra...);
  double acc[Est::kSums];
#pragma unroll
  for (int a = 0; a < Est::kSums; a++) acc[a] = 0.0;
  const int base = blockIdx.x * kIcpChunk + threadIdx.x;
  for (int k = 0; k < kIcpPerThread; k++) {
    const int i = base + k * kIcpThreads;
    if (i >= ns) break;
    const float4 p = sp[i];
    const double px = p.x, py = p.y, pz = p.z;
    // x - c_t in float64: T applied to the original point
    const double x[3] = {fma(m00, px, fma(m01, py, fma(m02, pz, m03))), fma(m10, px, fma(m11, py, fma(m12, pz, m13))),
                         fma(m20, px, fma(m21, py, fma(m22, pz, m23)))};
    const int id = icp_nearest((float)x[0], (float)x[1], (float)x[2], r2f, g, cell_start, tq);
    if (id < 0) continue;
    const double q[3] = {(double)tgt[(size_t)id * 3 + 0] - c0, (double)tgt[(size_t)id * 3 + 1] - c1,
                         (double)tgt[(size_t)id * 3 + 2] - c2};
    const double u[3] = {x[0] - q[0], x[1] - q[1], x[2] - q[2]};
    const double d2 = fma(u[0], u[0], fma(u[1], u[1], u[2] * u[2]));
    if (!(d2 <= r2)) continue;
    est.accumulate(acc, x, q, u, d2, tn, id, i);
  }
  __shared__ double part[kIcpThreads / 64][Est::kSums];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < Est::kSums; a++) {
    const double v = wave_sum_f64(acc[a]);
    if (lane == 0) part[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < Est::kSums) {
    double s = 0.0;
    for (int w = 0; w < kIcpThreads / 64; w++) s += part[w][threadIdx.x];
    rows[((size_t)j * gridDim.x + blockIdx.x) * Est::kRow + threadIdx.x] = s;
  }
}

__global__ void __launch_bounds__(kIcpThreads) icp_pass_kernel(const float4 *__restrict__ sp, int ns, const float4 *__restrict__ tq,
                                                               const float *__restrict__ tgt, const uint32_t *__restrict__ cell_start,
                                                               const IcpGrid *__restrict__ g, const double *__restrict__ T,
                                                               const int32_t *__restrict__ active, double r2, float r2f,
                                                               double *__restrict__ rows) {
  icp_pass<PointToPoint>(sp, nullptr, ns, tq, tgt, nullptr, cell_start, g, T, active, r2, r2f, rows);
}

__global__ void __launch_bounds__(kIcpThreads) icp_plane_pass_kernel(const float4 *__restrict__ sp, int ns, const float4 *__restrict__ tq,
                                                                     const float *__restrict__ tgt, const float *__restrict__ tn,
                                                                     const uint32_t *__restrict__ cell_start,
                                                                     const IcpGrid *__restrict__ g, const double *__restrict__ T,
                                                                     const int32_t *__restrict__ active, double r2, float r2f,
                                                                     double *__restrict__ rows) {
  icp_pass<PointToPlane>(sp, nullptr, ns, tq, tgt, tn, cell_start, g, T, active, r2, r2f, rows);
}

__global__ void __launch_bounds__(kIcpThreads) icp_generalized_pass_kernel(
    const float4 *__restrict__ sp, const float *__restrict__ sc, int ns, const float4 *__restrict__ tq, const float *__restrict__ tgt,
    const float *__restrict__ tc, const uint32_t *__restrict__ cell_start, const IcpGrid *__restrict__ g, const double *__restrict__ T,
    const int32_t *__restrict__ active, double r2, float r2f, double *__restrict__ rows) {
  icp_pass<Generalized>(sp, sc, ns, tq, tgt, tc, cell_start, g, T, active, r2, r2f, rows);
}

__global__ void __launch_bounds__(kIcpThreads) icp_colored_pass_kernel(
    const float4 *__restrict__ sp, const float *__restrict__ si, int ns, const float4 *__restrict__ tq, const float *__restrict__ tgt,
    const float *__restrict__ tn, const IcpColors colors, const uint32_t *__restrict__ cell_start, const IcpGrid *__restrict__ g,
    const double *__restrict__ T, const int32_t *__restrict__ active, double r2, float r2f, double *__restrict__ rows) {
  icp_pass<Colored>(sp, si, ns, tq, tgt, tn, cell_start, g, T, active, r2, r2f, rows, colors);
}

// the source's covariances [ns, 6] in the Morton order of W.sp
__global__ void __launch_bounds__(256) icp_gather_covariances_kernel(const float *__restrict__ cov, const uint32_t *__restrict__ order,
                                                                     int ns, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  const float *c = cov + (size_t)order[i] * 6;
  for (int e = 0; e < 6; e++) out[(size_t)i * 6 + e] = c[e];
}

// the source's intensities [ns] in the Morton order of W.sp
__global__ void __launch_bounds__(256) icp_gather_intensity_kernel(const float *__restrict__ intensity, const uint32_t *__restrict__ order,
                                                                   int ns, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ns) out[i] = intensity[order[i]];
}

// ---- the solve ----

// one wave per init, after pass `k` (every active init has run the same number of passes)
template <class Est>
__device__ __forceinline__ void icp_solve(const double *__restrict__ rows, int nblk, int ns, const IcpGrid *__restrict__ g, int k,
                                          int max_iteration, double rel_fitness, double rel_rmse, double *T, double *fitness,
                                          double *rmse, int32_t *iters, int32_t *active) {
  const int j = blockIdx.x;
  if (!active[j]) return;
  const int lane = threadIdx.x;
  double S[Est::kSums];
#pragma unroll
  for (int a = 0; a < Est::kSums; a++) S[a] = 0.0;
  for (int b = lane; b < nblk; b += 64) {
    const double *r = rows + ((size_t)j * nblk + b) * Est::kRow;
#pragma unroll
    for (int a = 0; a < Est::kSums; a++) S[a] += r[a];
  }
#pragma unroll
  for (int a = 0; a < Est::kSums; a++) S[a] = wave_sum_f64(S[a]);
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
  double R[3][3], tau[3], t[3];
  if (!Est::update(S, c, g, R, tau)) return;
  for (int a = 0; a < 3; a++) {
    // absolute: x' -> R x' + tau about c_t  ->  t = tau + c_t - R c_t
    double rc = 0.0;
    for (int b = 0; b < 3; b++) rc += R[a][b] * g->ct[b];
    t[a] = tau[a] + (g->ct[a] - rc);
  }
  double *M = T + (size_t)j * 16, N[12];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 4; b++)
      N[a * 4 + b] = R[a][0] * M[b] + R[a][1] * M[4 + b] + R[a][2] * M[8 + b] + (b == 3 ? t[a] : 0.0);
  for (int e = 0; e < 12; e++) M[e] = N[e];
}

__global__ void __launch_bounds__(64) icp_solve_kernel(const double *__restrict__ rows, int nblk, int ns, const IcpGrid *__restrict__ g,
                                                       int k, int max_iteration, double rel_fitness, double rel_rmse, double *T,
                                                       double *fitness, double *rmse, int32_t *iters, int32_t *active) {
  icp_solve<PointToPoint>(rows, nblk, ns, g, k, max_iteration, rel_fitness, rel_rmse, T, fitness, rmse, iters, active);
}

__global__ void __launch_bounds__(64) icp_plane_solve_kernel(const double *__restrict__ rows, int nblk, int ns,
                                                             const IcpGrid *__restrict__ g, int k, int max_iteration,
                                                             double rel_fitness, double rel_rmse, double *T, double *fitness,
                                                             double *rmse, int32_t *iters, int32_t *active) {
  icp_solve<PointToPlane>(rows, nblk, ns, g, k, max_iteration, rel_fitness, rel_rmse, T, fitness, rmse, iters, active);
}

// ---- the normal estimation ----

// One thread per point, in cell order (thread i takes sorted point i, so a wave's queries are neighbours).  The k best
// (fp32 d^2, original index) so far sit sorted in the lane's column of nd / ni (KBest).  The walk is icp_nearest's
// (icp_ring_walk); it ends when everything outside ring k's box is farther than the k-th best, or nothing is left outside it.
__global__ void __launch_bounds__(kNormalsThreads) icp_normals_kernel(const float4 *__restrict__ tq, const float *__restrict__ pts, int n,
                                                                      int k, int knn, const uint32_t *__restrict__ cell_start,
                                                                      const IcpGrid *__restrict__ g, float *__restrict__ out_normals,
                                                                      int32_t *__restrict__ out_neighbors) {
  __shared__ float nd[kNormalsMaxK][kNormalsThreads];
  __shared__ uint32_t ni[kNormalsMaxK][kNormalsThreads];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * kNormalsThreads + lane;
  if (i >= n) return;
  const float4 me = tq[i];
  const uint32_t self = __float_as_uint(me.w);
  const IcpWalk walk(me, g);
  KBest<float> best(nd, ni, lane, k, 3.4e38f);
  auto visit = [&](int ca, int cb) {
    icp_cell_run(cell_start, ca, cb, [&](uint32_t t) {
      const float4 q = tq[t];
      const float ux = q.x - walk.x, uy = q.y - walk.y, uz = q.z - walk.z;
      best.offer(__builtin_fmaf(ux, ux, __builtin_fmaf(uy, uy, uz * uz)), __float_as_uint(q.w));
    });
  };
  walk.run(visit, [&]() { return best.kth(); });
  if (out_neighbors) best.write_neighbors(out_neighbors, self, knn);
  const int cnt = best.count();
  float *o = out_normals + (size_t)self * 3;
  if (cnt < 3) { o[0] = 0.0f; o[1] = 0.0f; o[2] = 1.0f; return; }
  // float64 covariance of the neighbours about their mean (coordinates relative to c_t)
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  for (int a = 0; a < cnt; a++) {
    const float *p = pts + (size_t)best.id(a) * 3;
    m0 += (double)p[0] - g->ct[0]; m1 += (double)p[1] - g->ct[1]; m2 += (double)p[2] - g->ct[2];
  }
  m0 /= cnt; m1 /= cnt; m2 /= cnt;
  double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
  for (int a = 0; a < cnt; a++) {
    const float *p = pts + (size_t)best.id(a) * 3;
    const double e0 = ((double)p[0] - g->ct[0]) - m0, e1 = ((double)p[1] - g->ct[1]) - m1, e2 = ((double)p[2] - g->ct[2]) - m2;
    c00 = fma(e0, e0, c00); c01 = fma(e0, e1, c01); c02 = fma(e0, e2, c02);
    c11 = fma(e1, e1, c11); c12 = fma(e1, e2, c12); c22 = fma(e2, e2, c22);
  }
  const double C[3][3] = {{c00 / cnt, c01 / cnt, c02 / cnt}, {c01 / cnt, c11 / cnt, c12 / cnt}, {c02 / cnt, c12 / cnt, c22 / cnt}};
  double U[3][3], W[3][3];
  svd3(C, U, W);   // C symmetric and positive semi-definite: the columns of W are its eigenvectors, the last the smallest's
  double v0 = W[0][2], v1 = W[1][2], v2 = W[2][2];
  const double len = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  v0 /= len; v1 /= len; v2 /= len;
  // the sign: the component of largest magnitude (the first of equal ones) is positive
  double big = v0;
  if (fabs(v1) > fabs(big)) big = v1;
  if (fabs(v2) > fabs(big)) big = v2;
  if (big < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
  o[0] = (float)v0; o[1] = (float)v1; o[2] = (float)v2;
}

// ---- the colour gradients ----

// One thread per point: the least-squares gradient of the intensity over the point's stored neighbours, in its tangent
// plane (the rule is in include/scorp_gs.h).  The neighbour row is walked, not copied; an entry outside [0, n) is skipped.
__global__ void __launch_bounds__(256) icp_color_gradients_kernel(const float *__restrict__ pts, const float *__restrict__ normals,
                                                                  const float *__restrict__ intensity,
                                                                  const int32_t *__restrict__ neighbors, int n, int knn,
                                                                  float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double p0 = pts[(size_t)i * 3 + 0], p1 = pts[(size_t)i * 3 + 1], p2 = pts[(size_t)i * 3 + 2], Ii = intensity[i];
  double h0 = normals[(size_t)i * 3 + 0], h1 = normals[(size_t)i * 3 + 1], h2 = normals[(size_t)i * 3 + 2];
  {
    const double len = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
    if (len > 0.0 && isfinite(len)) { h0 /= len; h1 /= len; h2 /= len; } else { h0 = 0.0; h1 = 0.0; h2 = 0.0; }
  }
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, ee = 0.0;
  int used = 0;
  const int32_t *row = neighbors + (size_t)i * knn;
  for (int a = 0; a < knn; a++) {
    const int j = row[a];
    if (j < 0 || j >= n || j == i) continue;
    const double u0 = (double)pts[(size_t)j * 3 + 0] - p0, u1 = (double)pts[(size_t)j * 3 + 1] - p1,
                 u2 = (double)pts[(size_t)j * 3 + 2] - p2;
    const double un = fma(u0, h0, fma(u1, h1, u2 * h2));
    const double e0 = u0 - un * h0, e1 = u1 - un * h1, e2 = u2 - un * h2;
    const double delta = (double)intensity[j] - Ii;
    m00 = fma(e0, e0, m00); m01 = fma(e0, e1, m01); m02 = fma(e0, e2, m02);
    m11 = fma(e1, e1, m11); m12 = fma(e1, e2, m12); m22 = fma(e2, e2, m22);
    g0 = fma(e0, delta, g0); g1 = fma(e1, delta, g1); g2 = fma(e2, delta, g2);
    ee += fma(e0, e0, fma(e1, e1, e2 * e2));
    used++;
  }
  float *o = out + (size_t)i * 3;
  o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
  if (used < 2) return;
  const double M[3][3] = {{fma(ee * h0, h0, m00), fma(ee * h0, h1, m01), fma(ee * h0, h2, m02)},
                          {fma(ee * h0, h1, m01), fma(ee * h1, h1, m11), fma(ee * h1, h2, m12)},
                          {fma(ee * h0, h2, m02), fma(ee * h1, h2, m12), fma(ee * h2, h2, m22)}};
  double U[3][3], V[3][3];
  svd3(M, U, V);   // M symmetric and positive semi-definite: the columns of V are its eigenvectors
  double l[3], lmax = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) {   // l_k = v_k . M v_k
    const double w0 = fma(M[0][0], V[0][k], fma(M[0][1], V[1][k], M[0][2] * V[2][k]));
    const double w1 = fma(M[1][0], V[0][k], fma(M[1][1], V[1][k], M[1][2] * V[2][k]));
    const double w2 = fma(M[2][0], V[0][k], fma(M[2][1], V[1][k], M[2][2] * V[2][k]));
    l[k] = fma(V[0][k], w0, fma(V[1][k], w1, V[2][k] * w2));
    lmax = fmax(lmax, l[k]);
  }
  if (!(lmax > 0.0)) return;
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (!(l[k] > 1e-12 * lmax)) continue;
    const double f = fma(V[0][k], g0, fma(V[1][k], g1, V[2][k] * g2)) / l[k];
    d0 = fma(V[0][k], f, d0); d1 = fma(V[1][k], f, d1); d2 = fma(V[2][k], f, d2);
  }
  o[0] = (float)d0; o[1] = (float)d1; o[2] = (float)d2;
}

// ---- host ----

// what a Generalized call needs after IcpLayout::total: the source's covariances in sorted order
size_t icp_sorted_covariances_bytes(int64_t ns) { return align_up((size_t)(ns > 0 ? ns : 1) * 6 * 4, 256); }
// and a Colored call: the source's intensities in sorted order
size_t icp_sorted_intensity_bytes(int64_t ns) { return align_up((size_t)(ns > 0 ? ns : 1) * 4, 256); }

// normals: the target's per-point attribute where Est::kNormals (normals, or covariances); source_covariances where
// Est::kCovariances, the source's intensities where Est::kColors; colors: the rest of what Colored reads
template <class Est>
int icp_run(const float *source, const float *source_covariances, int32_t ns, const float *target, const float *normals, int32_t nt,
            const double *inits, int32_t ni,
            double r, int32_t max_iteration, double rel_fitness, double rel_rmse, double *out_T, double *out_fitness,
            double *out_rmse, int32_t *out_iters, void *workspace, size_t workspace_bytes, hipStream_t stream,
            const IcpColors &colors = IcpColors{nullptr, nullptr, 1.0}) {
  if (int e = icp_check_args(Est::kWho, r, ns, nt, max_iteration, ni,
                             source && target && (normals || !Est::kNormals) && (source_covariances || !(Est::kCovariances || Est::kColors)) &&
                                 ((colors.target_gradients && colors.target_intensity) || !Est::kColors) && inits && out_T && out_fitness && out_rmse && out_iters))
    return e;
  if (Est::kColors && !(colors.lambda >= 0.0 && colors.lambda <= 1.0)) {
    set_error("%s: lambda_geometric must be in [0, 1]", Est::kWho);
    return SCORP_ERR_INVALID;
  }
  const IcpLayout L(ns, nt, ni, Est::kRow);
  if (int e = check_workspace(Est::kWho, workspace, workspace_bytes,
                              L.total + (Est::kCovariances ? icp_sorted_covariances_bytes(ns) : Est::kColors ? icp_sorted_intensity_bytes(ns) : 0)))
    return e;
  const IcpWorkspace W(workspace, L);
  if (int e = icp_build_target(target, nt, L, W, stream)) return e;
  const uint32_t *order;
  if (int e = icp_build_source(source, ns, L, W, stream, &order)) return e;
  float *sc = (float *)((char *)workspace + L.total);
  if constexpr (Est::kCovariances) {
    icp_gather_covariances_kernel<<<(ns + 255) / 256, 256, 0, stream>>>(source_covariances, order, ns, sc);
    SCORP_KERNEL_CHECK("icp_gather_covariances", 0, stream);
  }
  if constexpr (Est::kColors) {
    icp_gather_intensity_kernel<<<(ns + 255) / 256, 256, 0, stream>>>(source_covariances, order, ns, sc);
    SCORP_KERNEL_CHECK("icp_gather_intensity", 0, stream);
  }
  icp_init_kernel<<<(ni + 63) / 64, 64, 0, stream>>>(inits, ni, out_T, out_fitness, out_rmse, out_iters, W.active);
  SCORP_KERNEL_CHECK("icp_init", 0, stream);

  const int nblk = (ns + kIcpChunk - 1) / kIcpChunk;
  const double r2 = r * r;
  const float r2f = (float)r2 * (1.0f + 1e-5f);   // the fp32 search keeps slightly more; the pair test is float64
  return icp_iterate(ni, max_iteration, W.active, stream, [&](int k) -> int {
    const dim3 grid(nblk, ni);
    if constexpr (Est::kCovariances)
      icp_generalized_pass_kernel<<<grid, kIcpThreads, 0, stream>>>(W.sp, sc, ns, W.tq, target, normals, W.cell_start, W.g, out_T,
                                                                    W.active, r2, r2f, W.rows);
    else if constexpr (Est::kColors)
      icp_colored_pass_kernel<<<grid, kIcpThreads, 0, stream>>>(W.sp, sc, ns, W.tq, target, normals, colors, W.cell_start, W.g, out_T,
                                                                W.active, r2, r2f, W.rows);
    else if constexpr (Est::kNormals)
      icp_plane_pass_kernel<<<grid, kIcpThreads, 0, stream>>>(W.sp, ns, W.tq, target, normals, W.cell_start, W.g, out_T, W.active, r2,
                                                              r2f, W.rows);
    else
      icp_pass_kernel<<<grid, kIcpThreads, 0, stream>>>(W.sp, ns, W.tq, target, W.cell_start, W.g, out_T, W.active, r2, r2f, W.rows);
    SCORP_KERNEL_CHECK("icp_pass", 0, stream);
    (Est::kNormals ? icp_plane_solve_kernel : icp_solve_kernel)<<<ni, 64, 0, stream>>>(
        W.rows, nblk, ns, W.g, k, max_iteration, rel_fitness, rel_rmse, out_T, out_fitness, out_rmse, out_iters, W.active);
    SCORP_KERNEL_CHECK("icp_solve", 0, stream);
    return SCORP_OK;
  });
}

int normals_impl(const float *points, int32_t n, int32_t knn, float *out_normals, int32_t *out_neighbors, void *workspace,
                 size_t workspace_bytes, hipStream_t stream) {
  if (knn < 3 || knn > kNormalsMaxK) { set_error("estimate_normals: knn must be in [3, %d]", kNormalsMaxK); return SCORP_ERR_INVALID; }
  if (n <= 0) { set_error("estimate_normals: empty cloud"); return SCORP_ERR_INVALID; }
  if (n > (1 << 30)) { set_error("estimate_normals: more than 2^30 points"); return SCORP_ERR_INVALID; }
  if (!points || !out_normals) { set_error("estimate_normals: NULL argument"); return SCORP_ERR_INVALID; }
  const IcpLayout L(0, n, 0, PointToPlane::kRow);
  if (int e = check_workspace("estimate_normals", workspace, workspace_bytes, L.total)) return e;
  const IcpWorkspace W(workspace, L);
  if (int e = icp_build_target(points, n, L, W, stream)) return e;
  const int k = knn < n ? knn : n;
  icp_normals_kernel<<<(n + kNormalsThreads - 1) / kNormalsThreads, kNormalsThreads, 0, stream>>>(
      W.tq, points, n, k, knn, W.cell_start, W.g, out_normals, out_neighbors);
  SCORP_KERNEL_CHECK("icp_normals", 0, stream);
  return SCORP_OK;
}

int color_gradients_impl(const float *points, const float *normals, const float *intensity, const int32_t *neighbors, int32_t n,
                         int32_t knn, float *out_gradients, hipStream_t stream) {
  if (knn < 3 || knn > kNormalsMaxK) { set_error("color_gradients: knn must be in [3, %d]", kNormalsMaxK); return SCORP_ERR_INVALID; }
  if (n <= 0) { set_error("color_gradients: empty cloud"); return SCORP_ERR_INVALID; }
  if (n > (1 << 30)) { set_error("color_gradients: more than 2^30 points"); return SCORP_ERR_INVALID; }
  if (!points || !normals || !intensity || !neighbors || !out_gradients) { set_error("color_gradients: NULL argument"); return SCORP_ERR_INVALID; }
  icp_color_gradients_kernel<<<(n + 255) / 256, 256, 0, stream>>>(points, normals, intensity, neighbors, n, knn, out_gradients);
  SCORP_KERNEL_CHECK("icp_color_gradients", 0, stream);
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_icp_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init) {
  return IcpLayout(n_source, n_target, n_init, PointToPoint::kRow).total;
}

extern "C" int scorp_icp_point_to_point(const float *source, int32_t n_source, const float *target, int32_t n_target,
                                        const double *inits, int32_t n_init, double max_correspondence_distance,
                                        int32_t max_iteration, double relative_fitness, double relative_rmse,
                                        double *out_transformation, double *out_fitness, double *out_inlier_rmse,
                                        int32_t *out_iterations, void *workspace, size_t workspace_bytes,
                                        scorp_stream_t stream) {
  return icp_run<PointToPoint>(source, nullptr, n_source, target, nullptr, n_target, inits, n_init, max_correspondence_distance, max_iteration,
                               relative_fitness, relative_rmse, out_transformation, out_fitness, out_inlier_rmse, out_iterations,
                               workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t scorp_icp_point_to_plane_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init) {
  return IcpLayout(n_source, n_target, n_init, PointToPlane::kRow).total;
}

extern "C" int scorp_icp_point_to_plane(const float *source, int32_t n_source, const float *target, const float *target_normals,
                                        int32_t n_target, const double *inits, int32_t n_init,
                                        double max_correspondence_distance, int32_t max_iteration, double relative_fitness,
                                        double relative_rmse, double *out_transformation, double *out_fitness,
                                        double *out_inlier_rmse, int32_t *out_iterations, void *workspace,
                                        size_t workspace_bytes, scorp_stream_t stream) {
  return icp_run<PointToPlane>(source, nullptr, n_source, target, target_normals, n_target, inits, n_init, max_correspondence_distance,
                               max_iteration, relative_fitness, relative_rmse, out_transformation, out_fitness, out_inlier_rmse,
                               out_iterations, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t scorp_icp_generalized_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init) {
  return IcpLayout(n_source, n_target, n_init, Generalized::kRow).total + icp_sorted_covariances_bytes(n_source);
}

extern "C" int scorp_icp_generalized(const float *source, const float *source_covariances, int32_t n_source, const float *target,
                                     const float *target_covariances, int32_t n_target, const double *inits, int32_t n_init,
                                     double max_correspondence_distance, int32_t max_iteration, double relative_fitness,
                                     double relative_rmse, double *out_transformation, double *out_fitness, double *out_inlier_rmse,
                                     int32_t *out_iterations, void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  return icp_run<Generalized>(source, source_covariances, n_source, target, target_covariances, n_target, inits, n_init,
                              max_correspondence_distance, max_iteration, relative_fitness, relative_rmse, out_transformation,
                              out_fitness, out_inlier_rmse, out_iterations, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t scorp_icp_colored_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init) {
  return IcpLayout(n_source, n_target, n_init, Colored::kRow).total + icp_sorted_intensity_bytes(n_source);
}

extern "C" int scorp_icp_colored(const float *source, const float *source_intensity, int32_t n_source, const float *target,
                                 const float *target_normals, const float *target_intensity, const float *target_gradients,
                                 int32_t n_target, const double *inits, int32_t n_init, double max_correspondence_distance,
                                 int32_t max_iteration, double relative_fitness, double relative_rmse, double lambda_geometric,
                                 double *out_transformation, double *out_fitness, double *out_inlier_rmse, int32_t *out_iterations,
                                 void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  return icp_run<Colored>(source, source_intensity, n_source, target, target_normals, n_target, inits, n_init,
                          max_correspondence_distance, max_iteration, relative_fitness, relative_rmse, out_transformation, out_fitness,
                          out_inlier_rmse, out_iterations, workspace, workspace_bytes, (hipStream_t)stream,
                          IcpColors{target_gradients, target_intensity, lambda_geometric});
}

extern "C" int scorp_color_gradients(const float *points, const float *normals, const float *intensity, const int32_t *neighbors,
                                     int32_t n, int32_t knn, float *out_gradients, scorp_stream_t stream) {
  return color_gradients_impl(points, normals, intensity, neighbors, n, knn, out_gradients, (hipStream_t)stream);
}

extern "C" size_t scorp_estimate_normals_workspace_bytes(int32_t n) { return IcpLayout(0, n, 0, PointToPlane::kRow).total; }

extern "C" int scorp_estimate_normals(const float *points, int32_t n, int32_t knn, float *out_normals, int32_t *out_neighbors,
                                      void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  return normals_impl(points, n, knn, out_normals, out_neighbors, workspace, workspace_bytes, (hipStream_t)stream);
}
