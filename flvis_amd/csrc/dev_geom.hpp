// flvis_amd: device-side point geometry (fp64): camera maps, DLT triangulation, the fundamental matrix's point error,
// projection edge + small SPD solves (the minimal solvers are in cv_solvers.hpp).  Reference call sites: src/processing/lkorb_tracking.cpp:55-61,87,133-135,170-177;
// src/processing/camera_frame.cpp:113-131; src/processing/triangulation.cpp:9-97;
// 3rdPartLib/g2o/g2o/types/sba/types_six_dof_expmap.cpp:389-433.
#pragma once
#include "dev_math.hpp"

namespace flvis {

// cv::projectPoints for one Point3f (k1 k2 p1 p2 model) -> Point2f
FD void project_point(const float* p3, const M3& R, V3 t, const double* K, const double* D, float* out) {
  V3 P{(double)p3[0], (double)p3[1], (double)p3[2]};
  V3 X = R * P + t;
  double z = X.z ? 1. / X.z : 1;
  double x = X.x * z, y = X.y * z;
  double r2 = x * x + y * y, r4 = r2 * r2;
  double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
  double cdist = 1 + D[0] * r2 + D[1] * r4;
  double xd = x * cdist + D[2] * a1 + D[3] * a2;
  double yd = y * cdist + D[2] * a3 + D[3] * a1;
  out[0] = (float)(xd * K[0] + K[2]);
  out[1] = (float)(yd * K[1] + K[3]);
}

// cv::undistortPoints for one Point2f with (K, D, R, P)
FD void undistort_point(const float* src, const double* K, const double* D, const double* R9, const double* P12,
                        float* dst) {
  double x = (src[0] - K[2]) / K[0], y = (src[1] - K[3]) / K[1];
  double x0 = x, y0 = y;
  for (int j = 0; j < 5; j++) {
    double r2 = x * x + y * y;
    double icdist = 1. / (1 + (D[1] * r2 + D[0]) * r2);
    double deltaX = 2 * D[2] * x * y + D[3] * (r2 + 2 * x * x);
    double deltaY = D[2] * (r2 + 2 * y * y) + 2 * D[3] * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  double xx = R9[0] * x + R9[1] * y + R9[2];
  double yy = R9[3] * x + R9[4] * y + R9[5];
  double ww = 1. / (R9[6] * x + R9[7] * y + R9[8]);
  x = xx * ww;
  y = yy * ww;
  dst[0] = (float)(x * P12[0] + P12[2]);
  dst[1] = (float)(y * P12[5] + P12[6]);
}

// Triangulation::triangulationPt: smallest right singular vector of the 4x4 DLT matrix (one-sided Jacobi)
__device__ inline V3 triangulate_dlt(double u1, double v1, double u2, double v2, const double* P1, const double* P2) {
  double A[4][4], V[4][4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    A[0][j] = v1 * P1[8 + j] - P1[4 + j];
    A[1][j] = P1[j] - u1 * P1[8 + j];
    A[2][j] = v2 * P2[8 + j] - P2[4 + j];
    A[3][j] = P2[j] - u2 * P2[8 + j];
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++) {
    int off = 0;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          alpha += A[i][p] * A[i][p];
          beta += A[i][q] * A[i][q];
          gamma += A[i][p] * A[i][q];
        }
        // orthogonal to 10 eps (OpenCV's Jacobi SVD test).  Round 2's 1e-16 was below the rounding of the dot product: one problem in
        // twelve chattered through all 30 sweeps, and a wave runs as long as its slowest lane -- nearly every wave ran 30 sweeps.
        if (gamma * gamma <= 4.930380657631324e-30 * (alpha * beta)) continue;
        off = 1;
        double zeta = (beta - alpha) / (2.0 * gamma);
        double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          double ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - s * aq;
          A[i][q] = s * ap + c * aq;
          double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq;
          V[i][q] = s * vp + c * vq;
        }
      }
    if (!off) break;
  }
  int best = 0;
  double bn = 1.7976931348623157e308;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    double nn = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) nn += A[i][j] * A[i][j];
    if (nn < bn) {
      bn = nn;
      best = j;
    }
  }
  double vx = 0, vy = 0, vz = 0, vw = 1;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j == best) {
      vx = V[0][j];
      vy = V[1][j];
      vz = V[2][j];
      vw = V[3][j];
    }
  return V3{vx / vw, vy / vw, vz / vw};
}

__device__ inline V3 triangulate_two_view(double u1, double v1, double u2, double v2, const SE3d& T1, const SE3d& T2,
                                          double fx, double fy, double cx, double cy) {
  double P1[12], P2[12];
  for (int k = 0; k < 2; k++) {
    const SE3d& T = k == 0 ? T1 : T2;
    double* P = k == 0 ? P1 : P2;
    M3 R = q_to_mat(T.q);
    double T34[3][4] = {{R.m[0][0], R.m[0][1], R.m[0][2], T.t.x}, {R.m[1][0], R.m[1][1], R.m[1][2], T.t.y},
                        {R.m[2][0], R.m[2][1], R.m[2][2], T.t.z}};
    for (int j = 0; j < 4; j++) {
      P[j] = fx * T34[0][j] + 0 * T34[1][j] + cx * T34[2][j];
      P[4 + j] = 0 * T34[0][j] + fy * T34[1][j] + cy * T34[2][j];
      P[8 + j] = 0 * T34[0][j] + 0 * T34[1][j] + 1 * T34[2][j];
    }
  }
  return triangulate_dlt(u1, v1, u2, v2, P1, P2);
}

// OpenCV FMEstimatorCallback::computeError (max of the two squared point-line distances, float)
FD float f_error(const double* F, double x1, double y1, double x2, double y2) {
  double a = F[0] * x1 + F[1] * y1 + F[2], b = F[3] * x1 + F[4] * y1 + F[5], c = F[6] * x1 + F[7] * y1 + F[8];
  double s2 = 1. / (a * a + b * b);
  double dd2 = x2 * a + y2 * b + c;
  a = F[0] * x2 + F[3] * y2 + F[6];
  b = F[1] * x2 + F[4] * y2 + F[7];
  c = F[2] * x2 + F[5] * y2 + F[8];
  double s1 = 1. / (a * a + b * b);
  double dd1 = x1 * a + y1 * b + c;
  return (float)fmax(dd1 * dd1 * s1, dd2 * dd2 * s2);
}

// g2o EdgeSE3ProjectXYZ error + pose Jacobian (tangent = omega, upsilon)
FD void proj_edge(const SE3d& T, V3 pw, double zu, double zv, double fx, double fy, double cx, double cy, double* e,
                  double (*J)[6]) {
  V3 X = g2o_map(T, pw);
  double x = X.x, y = X.y, zz = X.z, z2 = zz * zz;
  e[0] = zu - (x / zz * fx + cx);
  e[1] = zv - (y / zz * fy + cy);
  if (J) {
    J[0][0] = x * y / z2 * fx;
    J[0][1] = -(1 + (x * x / z2)) * fx;
    J[0][2] = y / zz * fx;
    J[0][3] = -1. / zz * fx;
    J[0][4] = 0;
    J[0][5] = x / z2 * fx;
    J[1][0] = (1 + y * y / z2) * fy;
    J[1][1] = -x * y / z2 * fy;
    J[1][2] = -x / zz * fy;
    J[1][3] = 0;
    J[1][4] = -1. / zz * fy;
    J[1][5] = y / z2 * fy;
  }
}

// 6x6 SPD solve by Cholesky; false if not positive definite
__device__ inline bool solve_spd6(const double* H, const double* b, double* x) {
  double L[36];
  for (int i = 0; i < 36; i++) L[i] = 0;
  for (int j = 0; j < 6; j++) {
    double s = H[6 * j + j];
    for (int k = 0; k < j; k++) s -= L[6 * j + k] * L[6 * j + k];
    if (!(s > 0)) return false;
    L[6 * j + j] = sqrt(s);
    for (int i = j + 1; i < 6; i++) {
      double v = H[6 * i + j];
      for (int k = 0; k < j; k++) v -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = v / L[6 * j + j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double v = b[i];
    for (int k = 0; k < i; k++) v -= L[6 * i + k] * y[k];
    y[i] = v / L[6 * i + i];
  }
  for (int i = 5; i >= 0; i--) {
    double v = y[i];
    for (int k = i + 1; k < 6; k++) v -= L[6 * k + i] * x[k];
    x[i] = v / L[6 * i + i];
  }
  return true;
}

FD double huber_rho(double e) { return e <= 1.0 ? e : 2 * sqrt(e) - 1.0; }
FD double huber_w(double e) { return e <= 1.0 ? 1.0 : 1.0 / sqrt(e); }

}  // namespace flvis
