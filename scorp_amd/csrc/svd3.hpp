// svd3.hpp - the 3x3 float64 SVD (one-sided Jacobi) and determinant that every pose solve of the library shares: the
// ICP update (icp.hip) and the RANSAC / final fits of pose_fit.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace scorp {

// A = U S V^T by one-sided Jacobi (rotations on the columns of B = A V until they are orthogonal), singular values sorted
// descending; columns of U for zero singular values completed to an orthonormal basis with det U = +1.
static __device__ void svd3(const double A[3][3], double U[3][3], double V[3][3]) {
  double B[3][3];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) { B[i][k] = A[i][k]; V[i][k] = i == k ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 40; sweep++) {
    bool rotated = false;
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double al = 0.0, be = 0.0, ga = 0.0;
      for (int i = 0; i < 3; i++) { al += B[i][p] * B[i][p]; be += B[i][q] * B[i][q]; ga += B[i][p] * B[i][q]; }
      if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
      rotated = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      for (int i = 0; i < 3; i++) {
        const double bp = B[i][p], bq = B[i][q];
        B[i][p] = c * bp - s * bq; B[i][q] = s * bp + c * bq;
        const double vp = V[i][p], vq = V[i][q];
        V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double sg[3];
  for (int k = 0; k < 3; k++) sg[k] = sqrt(B[0][k] * B[0][k] + B[1][k] * B[1][k] + B[2][k] * B[2][k]);
  for (int a = 0; a < 2; a++)   // sort descending (columns of B and V together)
    for (int b = 0; b < 2 - a; b++)
      if (sg[b] < sg[b + 1]) {
        const double ts = sg[b]; sg[b] = sg[b + 1]; sg[b + 1] = ts;
        for (int i = 0; i < 3; i++) {
          double tb = B[i][b]; B[i][b] = B[i][b + 1]; B[i][b + 1] = tb;
          double tv = V[i][b]; V[i][b] = V[i][b + 1]; V[i][b + 1] = tv;
        }
      }
  const double tiny = 1e-13 * sg[0];
  int rank = 0;
  for (int k = 0; k < 3; k++) {
    if (sg[k] > tiny && sg[k] > 0.0) {
      for (int i = 0; i < 3; i++) U[i][k] = B[i][k] / sg[k];
      rank++;
    }
  }
  if (rank == 0) { U[0][0] = 1.0; U[1][0] = 0.0; U[2][0] = 0.0; }
  if (rank <= 1) {   // any unit vector orthogonal to U0: from the axis least aligned with it
    int ax = 0;
    for (int i = 1; i < 3; i++) if (fabs(U[i][0]) < fabs(U[ax][0])) ax = i;
    double e[3] = {0.0, 0.0, 0.0};
    e[ax] = 1.0;
    const double d = U[ax][0];
    double n = 0.0;
    for (int i = 0; i < 3; i++) { e[i] -= d * U[i][0]; n += e[i] * e[i]; }
    n = 1.0 / sqrt(n);
    for (int i = 0; i < 3; i++) U[i][1] = e[i] * n;
  }
  if (rank <= 2) {
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
}

static __device__ __forceinline__ double det3(const double M[3][3]) {
  return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
         M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

}  // namespace scorp
