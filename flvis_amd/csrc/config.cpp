// flvis_amd: configuration surface of the drop-in boundary (host side).
//   flvis_config_load      accepts the reference's yaml files unchanged (flat "key: scalar" / "key: [list]" with '#' comments,
//                          src/utils/include/yamlRead.h; keys per launch/EuRoC_MAV/euroc.yaml, launch/d435i/*_stereo.yaml)
//   flvis_config_finalize  derives what TrackingNodeletClass::onInit derives (src/frontend/vo_tracking.cpp:155-306): camera
//                          type, skip/equalise flags and the rectification R0,R1,P0,P1 of cv::stereoRectify(CALIB_ZERO_DISPARITY,
//                          alpha = 0) restated from OpenCV 3.x's cvStereoRectify (external dependency of the reference).
#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"

namespace {

struct M3h {
  double m[3][3];
};
struct V3h {
  double v[3];
};
M3h mul(const M3h& a, const M3h& b) {
  M3h r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return r;
}
V3h mulv(const M3h& a, const V3h& x) {
  V3h r;
  for (int i = 0; i < 3; i++) r.v[i] = a.m[i][0] * x.v[0] + a.m[i][1] * x.v[1] + a.m[i][2] * x.v[2];
  return r;
}
M3h transp(const M3h& a) {
  M3h r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r.m[i][j] = a.m[j][i];
  return r;
}
M3h ident() { return M3h{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}}; }
// cvRodrigues2 (OpenCV 3.x) as cvStereoRectify calls it, operation for operation: matrix -> vector by
// r = (R32 - R23, R13 - R31, R21 - R12), s = sqrt(r.r / 4), theta = acos((trace - 1) / 2), r *= theta / (2 s) (without OpenCV's SVD
// re-orthonormalisation: the rig rotations are orthonormal to rounding); vector -> matrix by R = c I + (1 - c) r r^T + s [r]x
V3h rotvec_from_mat(const M3h& R) {
  double rx = R.m[2][1] - R.m[1][2], ry = R.m[0][2] - R.m[2][0], rz = R.m[1][0] - R.m[0][1];
  const double s = std::sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
  double c = (R.m[0][0] + R.m[1][1] + R.m[2][2] - 1) * 0.5;
  c = c > 1. ? 1. : (c < -1. ? -1. : c);
  const double theta = std::acos(c);
  if (s < 1e-5) {
    if (c > 0) return V3h{{0, 0, 0}};
    double t;
    t = (R.m[0][0] + 1) * 0.5;
    rx = std::sqrt(std::max(t, 0.));
    t = (R.m[1][1] + 1) * 0.5;
    ry = std::sqrt(std::max(t, 0.)) * (R.m[0][1] < 0 ? -1. : 1.);
    t = (R.m[2][2] + 1) * 0.5;
    rz = std::sqrt(std::max(t, 0.)) * (R.m[0][2] < 0 ? -1. : 1.);
    if (std::fabs(rx) < std::fabs(ry) && std::fabs(rx) < std::fabs(rz) && (R.m[1][2] > 0) != (ry * rz > 0)) rz = -rz;
    const double k = theta / std::sqrt(rx * rx + ry * ry + rz * rz);
    return V3h{{rx * k, ry * k, rz * k}};
  }
  double vth = 1 / (2 * s);
  vth *= theta;
  return V3h{{rx * vth, ry * vth, rz * vth}};
}
M3h mat_from_rotvec(const V3h& r) {
  const double theta = std::sqrt(r.v[0] * r.v[0] + r.v[1] * r.v[1] + r.v[2] * r.v[2]);
  if (theta < DBL_EPSILON) return ident();
  const double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, itheta = 1. / theta;
  const double x = r.v[0] * itheta, y = r.v[1] * itheta, z = r.v[2] * itheta;
  const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
  const double r_x[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  M3h R;
  for (int k = 0; k < 9; k++) R.m[k / 3][k % 3] = c * I[k] + c1 * rrt[k] + s * r_x[k];
  return R;
}

// cv::undistortPoints(pt, K, D, R, P) for one point (5 iterations)
void undistort_pt(double u, double v, const double* K, const double* D, const M3h& R, const double* P, double& ou, double& ov) {
  double x = (u - K[2]) / K[0], y = (v - K[3]) / K[1], x0 = x, y0 = y;
  for (int j = 0; j < 5; j++) {
    double r2 = x * x + y * y;
    double icdist = 1. / (1 + (D[1] * r2 + D[0]) * r2);
    double dX = 2 * D[2] * x * y + D[3] * (r2 + 2 * x * x), dY = D[2] * (r2 + 2 * y * y) + 2 * D[3] * x * y;
    x = (x0 - dX) * icdist;
    y = (y0 - dY) * icdist;
  }
  double xx = R.m[0][0] * x + R.m[0][1] * y + R.m[0][2], yy = R.m[1][0] * x + R.m[1][1] * y + R.m[1][2];
  double ww = 1. / (R.m[2][0] * x + R.m[2][1] * y + R.m[2][2]);
  ou = (double)(float)(xx * ww * P[0] + P[2]);
  ov = (double)(float)(yy * ww * P[5] + P[6]);
}

void stereo_rectify(const double* K1, const double* D1, const double* K2, const double* D2, int nx, int ny, const M3h& R,
                    const V3h& T, M3h& R1, M3h& R2, double* P1, double* P2) {
  V3h om = rotvec_from_mat(R);
  for (int i = 0; i < 3; i++) om.v[i] *= -0.5;
  M3h r_r = mat_from_rotvec(om);
  V3h t = mulv(r_r, T);
  int idx = std::fabs(t.v[0]) > std::fabs(t.v[1]) ? 0 : 1;
  double c = t.v[idx], nt = std::sqrt(t.v[0] * t.v[0] + t.v[1] * t.v[1] + t.v[2] * t.v[2]);
  V3h uu{{0, 0, 0}};
  uu.v[idx] = c > 0 ? 1 : -1;
  V3h ww{{t.v[1] * uu.v[2] - t.v[2] * uu.v[1], t.v[2] * uu.v[0] - t.v[0] * uu.v[2], t.v[0] * uu.v[1] - t.v[1] * uu.v[0]}};
  double nw = std::sqrt(ww.v[0] * ww.v[0] + ww.v[1] * ww.v[1] + ww.v[2] * ww.v[2]);
  if (nw > 0.0) {
    double k = std::acos(std::fabs(c) / nt) / nw;
    for (int i = 0; i < 3; i++) ww.v[i] *= k;
  }
  M3h wR = mat_from_rotvec(ww);
  R1 = mul(wR, transp(r_r));
  R2 = mul(wR, r_r);
  t = mulv(R2, T);
  double fc_new = DBL_MAX;
  const double* Ks[2] = {K1, K2};
  const double* Ds[2] = {D1, D2};
  for (int k = 0; k < 2; k++) {
    double dk1 = Ds[k][0];
    double fc = idx == 0 ? Ks[k][1] : Ks[k][0];
    if (dk1 < 0) fc *= 1 + dk1 * (nx * nx + ny * ny) / (4 * fc * fc);
    fc_new = std::min(fc_new, fc);
  }
  double ccx[2], ccy[2];
  const M3h* Rs[2] = {&R1, &R2};
  const double Pn[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int k = 0; k < 2; k++) {
    double ax = 0, ay = 0;
    for (int i = 0; i < 4; i++) {
      int j = (i < 2) ? 0 : 1;
      double px = (double)(float)((i % 2) * (nx - 1)), py = (double)(float)(j * (ny - 1));
      double ux, uy;
      undistort_pt(px, py, Ks[k], Ds[k], ident(), Pn, ux, uy);
      V3h X = mulv(*Rs[k], V3h{{ux, uy, 1.0}});
      ax += (double)(float)(fc_new * X.v[0] / X.v[2]);
      ay += (double)(float)(fc_new * X.v[1] / X.v[2]);
    }
    ccx[k] = (nx - 1) / 2 - ax / 4;  // integer (nx-1)/2 as in cvStereoRectify
    ccy[k] = (ny - 1) / 2 - ay / 4;
  }
  ccx[0] = ccx[1] = (ccx[0] + ccx[1]) * 0.5;
  ccy[0] = ccy[1] = (ccy[0] + ccy[1]) * 0.5;
  for (int i = 0; i < 12; i++) P1[i] = P2[i] = 0;
  P1[0] = P1[5] = P2[0] = P2[5] = fc_new;
  P1[2] = ccx[0];
  P1[6] = ccy[0];
  P2[2] = ccx[1];
  P2[6] = ccy[1];
  P1[10] = P2[10] = 1;
  P2[4 * idx + 3] = t.v[idx] * fc_new;
  double inner[2][4];
  double* Ps[2] = {P1, P2};
  for (int k = 0; k < 2; k++) {
    const int N = 9;
    float iX0 = -FLT_MAX, iX1 = FLT_MAX, iY0 = -FLT_MAX, iY1 = FLT_MAX;
    for (int y = 0; y < N; y++)
      for (int x = 0; x < N; x++) {
        double qx, qy;
        undistort_pt((double)((float)x * nx / (N - 1)), (double)((float)y * ny / (N - 1)), Ks[k], Ds[k], *Rs[k], Ps[k], qx, qy);
        if (x == 0) iX0 = std::max(iX0, (float)qx);
        if (x == N - 1) iX1 = std::min(iX1, (float)qx);
        if (y == 0) iY0 = std::max(iY0, (float)qy);
        if (y == N - 1) iY1 = std::min(iY1, (float)qy);
      }
    inner[k][0] = iX0;
    inner[k][1] = iY0;
    inner[k][2] = iX1 - iX0;
    inner[k][3] = iY1 - iY0;
  }
  double cx1 = ccx[0], cy1 = ccy[0], cx2 = ccx[1], cy2 = ccy[1];
  double s0 = std::max(std::max(std::max(cx1 / (cx1 - inner[0][0]), cy1 / (cy1 - inner[0][1])),
                                (nx - cx1) / (inner[0][0] + inner[0][2] - cx1)),
                       (ny - cy1) / (inner[0][1] + inner[0][3] - cy1));
  s0 = std::max(std::max(std::max(std::max(cx2 / (cx2 - inner[1][0]), cy2 / (cy2 - inner[1][1])),
                                  (nx - cx2) / (inner[1][0] + inner[1][2] - cx2)),
                         (ny - cy2) / (inner[1][1] + inner[1][3] - cy2)),
                s0);
  fc_new *= s0;
  P1[0] = P1[5] = P2[0] = P2[5] = fc_new;
  P2[4 * idx + 3] = s0 * P2[4 * idx + 3];
}

// Rig transforms the way the reference composes them: Sophus SE3 objects (vo_tracking.cpp:183-236), i.e. a quaternion taken from
// the yaml's rotation matrix (Eigen's matrix -> quaternion, not renormalised), products and inverses on quaternions with a
// renormalisation after each (se3.cpp:59-83), translations rotated by Eigen's quaternion formula, and rotation_matrix() by
// Eigen's toRotationMatrix.  A 4x4 matrix product agrees with that only to ~1e-13 for a general rotation (EuRoC), and a rig that
// differs in the thirteenth digit ends in other RANSAC inlier sets after a few hundred frames.
struct RigT {
  double w, x, y, z;  // rotation
  double t[3];
};
RigT rig_from_mat44(const double* m) {
  const double R[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
  RigT r;
  double tr = R[0][0] + R[1][1] + R[2][2];
  if (tr > 0) {
    double s = std::sqrt(tr + 1.0);
    r.w = 0.5 * s;
    s = 0.5 / s;
    r.x = (R[2][1] - R[1][2]) * s;
    r.y = (R[0][2] - R[2][0]) * s;
    r.z = (R[1][0] - R[0][1]) * s;
  } else {
    int i = 0;
    if (R[1][1] > R[0][0]) i = 1;
    if (R[2][2] > R[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
    double v[3];
    v[i] = 0.5 * s;
    s = 0.5 / s;
    r.w = (R[k][j] - R[j][k]) * s;
    v[j] = (R[j][i] + R[i][j]) * s;
    v[k] = (R[k][i] + R[i][k]) * s;
    r.x = v[0], r.y = v[1], r.z = v[2];
  }
  r.t[0] = m[3], r.t[1] = m[7], r.t[2] = m[11];
  return r;
}
void rig_normalise(RigT& r) {
  const double n = std::sqrt(r.w * r.w + r.x * r.x + r.y * r.y + r.z * r.z);
  r.w = r.w / n, r.x = r.x / n, r.y = r.y / n, r.z = r.z / n;
}
void rig_rotate(const RigT& q, const double* v, double* o) {  // Eigen QuaternionBase::_transformVector
  double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
  for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
  const double c2[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
  for (int k = 0; k < 3; k++) o[k] = (v[k] + q.w * uv[k]) + c2[k];
}
RigT rig_mul(const RigT& a, const RigT& b) {
  RigT r;
  double rt[3];
  rig_rotate(a, b.t, rt);
  for (int k = 0; k < 3; k++) r.t[k] = a.t[k] + rt[k];
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
  r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
  rig_normalise(r);
  return r;
}
RigT rig_inverse(const RigT& a) {
  RigT r;
  r.w = a.w, r.x = -a.x, r.y = -a.y, r.z = -a.z;
  rig_normalise(r);
  const double nt[3] = {-1.0 * a.t[0], -1.0 * a.t[1], -1.0 * a.t[2]};
  rig_rotate(r, nt, r.t);
  return r;
}
void rig_rotation_matrix(const RigT& q, double R[3][3]) {  // Eigen QuaternionBase::toRotationMatrix
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0][0] = 1 - (tyy + tzz), R[0][1] = txy - twz, R[0][2] = txz + twy;
  R[1][0] = txy + twz, R[1][1] = 1 - (txx + tzz), R[1][2] = tyz - twx;
  R[2][0] = txz - twy, R[2][1] = tyz + twx, R[2][2] = 1 - (txx + tyy);
}
void rig_to_mat44(const RigT& a, double* o) {
  double R[3][3];
  rig_rotation_matrix(a, R);
  const double m[16] = {R[0][0], R[0][1], R[0][2], a.t[0], R[1][0], R[1][1], R[1][2], a.t[1], R[2][0], R[2][1], R[2][2], a.t[2], 0, 0, 0, 1};
  memcpy(o, m, sizeof(m));
}

}  // namespace

extern "C" int flvis_config_finalize(flvis_cfg* c) {
  if (!c) return FLVIS_ERR_INVALID_ARG;
  switch (c->type_of_vi) {
    case 1:
      c->cam_type = 1;  // STEREO_UNRECT
      c->imu_type = 1;  // EuRoC axis remap
      c->skip_first_n_imgs = 0;
      c->need_equal_hist = 1;
      break;
    case 3:
      c->cam_type = 0;  // STEREO_RECT
      c->imu_type = 0;  // D435i remap
      c->skip_first_n_imgs = 50;
      c->need_equal_hist = 0;
      break;
    case 5:
      c->cam_type = 0;
      c->imu_type = 2;  // pixhawk
      c->skip_first_n_imgs = 50;
      c->need_equal_hist = 0;
      break;
    case 0:
    case 2: {
      // DEPTH_D435 (vo_tracking.cpp:142-170): pinhole K from cam0_intrinsics, no distortion, no second camera
      c->cam_type = 2;
      c->imu_type = c->type_of_vi == 0 ? 0 : 2;
      c->skip_first_n_imgs = 50;
      c->need_equal_hist = 0;
      const double P[12] = {c->cam0_intrinsics[0], 0, c->cam0_intrinsics[2], 0, 0, c->cam0_intrinsics[1], c->cam0_intrinsics[3], 0,
                            0, 0, 1, 0};
      memcpy(c->P0, P, sizeof(P));
      memset(c->P1, 0, sizeof(c->P1));
      for (int i = 0; i < 9; i++) c->R0[i] = c->R1[i] = (i % 4 == 0) ? 1.0 : 0.0;
      return c->depth_factor > 0 ? FLVIS_OK : FLVIS_ERR_CONFIG;
    }
    case 4: {
      // VI_TYPE_KITTI_STEREO (vo_tracking.cpp:146,265-306): STEREO_RECT without IMU.  The rig comes from the two projection
      // matrices (flvis_config_load put their first three rows into P0 / P1): K0 = K1 = K0_rect = P0(0:3,0:3), no distortion,
      // R0 = R1 = I, T_c0_c1 = [I | K^-1 * P1(:,3)] with K^-1 as Eigen's 3x3 inverse computes it (cofactors * (1 / det)),
      // T_i_c0 is the dummy SE3(), init(..., 0, false): no skipped frames, no equalizeHist.
      c->cam_type = 0;
      c->imu_type = 3;  // NONE: imu_callback has no remap for it; flvis_imu_feed refuses samples for such a rig
      c->skip_first_n_imgs = 0;
      c->need_equal_hist = 0;
      const double fx = c->P0[0], fy = c->P0[5], cx = c->P0[2], cy = c->P0[6];
      if (!(fx > 0) || !(fy > 0)) return FLVIS_ERR_CONFIG;
      const double K[4] = {fx, fy, cx, cy}, Z[4] = {0, 0, 0, 0};
      memcpy(c->cam0_intrinsics, K, sizeof(K));
      memcpy(c->cam1_intrinsics, K, sizeof(K));
      memcpy(c->cam0_distortion, Z, sizeof(Z));
      memcpy(c->cam1_distortion, Z, sizeof(Z));
      for (int i = 0; i < 9; i++) c->R0[i] = c->R1[i] = (i % 4 == 0) ? 1.0 : 0.0;
      // Eigen compute_inverse_size3 on K = [fx 0 cx; 0 fy cy; 0 0 1]: cofactor(i,j) * invdet, det = fx * cof00 (+ 0 + 0)
      const double c00 = fy * 1.0 - cy * 0.0, det = fx * c00, invdet = 1.0 / det;
      const double i00 = c00 * invdet, i01 = (cx * 0.0 - 0.0 * 1.0) * invdet, i02 = (0.0 * cy - cx * fy) * invdet;
      const double i10 = (cy * 0.0 - 0.0 * 1.0) * invdet, i11 = (fx * 1.0 - cx * 0.0) * invdet, i12 = (0.0 * cx - fx * cy) * invdet;
      const double i20 = (0.0 * 0.0 - 0.0 * fy) * invdet, i21 = (0.0 * 0.0 - fx * 0.0) * invdet, i22 = (fx * fy - 0.0 * 0.0) * invdet;
      const double p0 = c->P1[3], p1 = c->P1[7], p2 = c->P1[11];  // P1(:,3); the 4x4's last row is zero in the yaml
      const double tx = i00 * p0 + i01 * p1 + i02 * p2, ty = i10 * p0 + i11 * p1 + i12 * p2, tz = i20 * p0 + i21 * p1 + i22 * p2;
      const double T01[16] = {1, 0, 0, tx, 0, 1, 0, ty, 0, 0, 1, tz, 0, 0, 0, 1};
      const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      memcpy(c->T_cam0_cam1, T01, sizeof(T01));
      memcpy(c->T_imu_cam0, eye, sizeof(eye));
      return FLVIS_OK;
    }
    default:
      return FLVIS_ERR_CONFIG;
  }
  // SE3 T_c1_c0 = T_c0_c1.inverse(); its rotation_matrix() and translation() go into cv::stereoRectify (vo_tracking.cpp:190-200,237-247)
  const RigT T10 = rig_inverse(rig_from_mat44(c->T_cam0_cam1));
  double R10[3][3];
  rig_rotation_matrix(T10, R10);
  M3h R{{{R10[0][0], R10[0][1], R10[0][2]}, {R10[1][0], R10[1][1], R10[1][2]}, {R10[2][0], R10[2][1], R10[2][2]}}};
  V3h T{{T10.t[0], T10.t[1], T10.t[2]}};
  M3h R0, R1;
  stereo_rectify(c->cam0_intrinsics, c->cam0_distortion, c->cam1_intrinsics, c->cam1_distortion, c->image_width,
                 c->image_height, R, T, R0, R1, c->P0, c->P1);
  for (int i = 0; i < 9; i++) {
    c->R0[i] = R0.m[i / 3][i % 3];
    c->R1[i] = R1.m[i / 3][i % 3];
  }
  return FLVIS_OK;
}

extern "C" int flvis_config_load(const char* path, flvis_cfg* c, char* err, int errlen) {
  auto fail = [&](const std::string& m) {
    if (err && errlen > 0) snprintf(err, errlen, "%s", m.c_str());
    return (int)FLVIS_ERR_CONFIG;
  };
  if (!path || !c) return FLVIS_ERR_INVALID_ARG;
  std::ifstream f(path);
  if (!f) return fail(std::string("cannot open ") + path);
  std::map<std::string, std::vector<double>> kv;
  std::string line, key, acc;
  bool in_list = false;
  auto flush_list = [&](const std::string& k, std::string s) {
    for (char& ch : s)
      if (ch == '[' || ch == ']' || ch == ',') ch = ' ';
    std::istringstream is(s);
    double v;
    std::vector<double> out;
    while (is >> v) out.push_back(v);
    kv[k] = out;
  };
  while (std::getline(f, line)) {
    size_t h = line.find('#');
    if (h != std::string::npos) line = line.substr(0, h);
    if (in_list) {
      acc += " " + line;
      if (line.find(']') != std::string::npos) {
        flush_list(key, acc);
        in_list = false;
      }
      continue;
    }
    size_t col = line.find(':');
    if (col == std::string::npos) continue;
    key = line.substr(0, col);
    size_t a = key.find_first_not_of(" \t");
    if (a == std::string::npos) continue;
    key = key.substr(a);
    key.erase(key.find_last_not_of(" \t") + 1);
    std::string val = line.substr(col + 1);
    if (val.find('[') != std::string::npos) {
      acc = val;
      if (val.find(']') != std::string::npos)
        flush_list(key, acc);
      else
        in_list = true;
    } else {
      size_t b = val.find_first_not_of(" \t\r");
      if (b == std::string::npos) {
        acc = "";
        in_list = true;
        continue;
      }
      val = val.substr(b);
      val.erase(val.find_last_not_of(" \t\r") + 1);
      if (val == "True" || val == "true")
        kv[key] = {1};
      else if (val == "False" || val == "false")
        kv[key] = {0};
      else
        kv[key] = {atof(val.c_str())};
    }
  }
  std::string missing;
  auto need = [&](const char* k, size_t n, double* dst) -> bool {
    auto it = kv.find(k);
    if (it == kv.end() || it->second.size() < n) {
      missing = k;
      return false;
    }
    for (size_t i = 0; i < n; i++) dst[i] = it->second[i];
    return true;
  };
  memset(c, 0, sizeof(*c));
  double v;
  if (!need("type_of_vi", 1, &v)) return fail("yaml key missing: type_of_vi");
  c->type_of_vi = (int)v;
  if (!need("image_width", 1, &v)) return fail("yaml key missing: image_width");
  c->image_width = (int)v;
  if (!need("image_height", 1, &v)) return fail("yaml key missing: image_height");
  c->image_height = (int)v;
  const bool depth_mode = c->type_of_vi == 0 || c->type_of_vi == 2;
  if (!need("cam0_intrinsics", 4, c->cam0_intrinsics) || !need("cam0_distortion_coeffs", 4, c->cam0_distortion))
    return fail("yaml key missing or short: " + missing);
  if (depth_mode) {  // vo_tracking.cpp:149-154 reads only cam0, depth_factor and T_imu_cam0
    if (!need("depth_factor", 1, &c->depth_factor) || !need("T_imu_cam0", 16, c->T_imu_cam0))
      return fail("yaml key missing or short: " + missing);
    const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    memcpy(c->T_cam0_cam1, eye, sizeof(eye));
  } else if (!need("cam1_intrinsics", 4, c->cam1_intrinsics) || !need("cam1_distortion_coeffs", 4, c->cam1_distortion)) {
    return fail("yaml key missing or short: " + missing);
  }
  if (depth_mode) {
  } else if (c->type_of_vi == 4) {  // KITTI: vo_tracking.cpp:267-270 reads the two 4x4 projection matrices
    double a[16], b[16];
    if (!need("cam0_projection_matrix", 16, a) || !need("cam1_projection_matrix", 16, b)) return fail("yaml key missing or short: " + missing);
    memcpy(c->P0, a, sizeof(double) * 12);
    memcpy(c->P1, b, sizeof(double) * 12);
  } else if (c->type_of_vi == 1) {
    double a[16], b[16], m[16];
    if (!need("T_mavimu_cam0", 16, a) || !need("T_mavimu_cam1", 16, b) || !need("T_imu_mavimu", 16, m))
      return fail("yaml key missing or short: " + missing);
    // vo_tracking.cpp:229-236: T_c0_c1 = T_mavi_c0.inverse() * T_mavi_c1, T_i_c0 = T_i_mavi * T_mavi_c0, as Sophus SE3 objects
    const RigT Ta = rig_from_mat44(a), Tb = rig_from_mat44(b), Tm = rig_from_mat44(m);
    rig_to_mat44(rig_mul(rig_inverse(Ta), Tb), c->T_cam0_cam1);
    rig_to_mat44(rig_mul(Tm, Ta), c->T_imu_cam0);
  } else {
    if (!need("T_imu_cam0", 16, c->T_imu_cam0) || !need("T_cam0_cam1", 16, c->T_cam0_cam1))
      return fail("yaml key missing or short: " + missing);
  }
  const char* vk[6] = {"vifusion_para1", "vifusion_para2", "vifusion_para3", "vifusion_para4", "vifusion_para5", "vifusion_para6"};
  const char* fk[6] = {"feature_para1", "feature_para2", "feature_para3", "feature_para4", "feature_para5", "feature_para6"};
  const char* dk[3] = {"dr_para1", "dr_para2", "dr_para3"};
  for (int i = 0; i < 6; i++)
    if (!need(vk[i], 1, &c->vifusion_para[i]) || !need(fk[i], 1, &c->feature_para[i])) return fail("yaml key missing: " + missing);
  for (int i = 0; i < 3; i++)
    if (!need(dk[i], 1, &c->dr_para[i])) return fail("yaml key missing: " + missing);
  if (!need("window_size", 1, &v)) return fail("yaml key missing: window_size");
  c->window_size = (int)v;
  if (c->window_size < 3 || c->window_size > 100) c->window_size = 10;  // vo_localmap.cpp:443-447
  int rc = flvis_config_finalize(c);
  if (rc != FLVIS_OK) return fail("unsupported type_of_vi for this path");
  return FLVIS_OK;
}

// getBoolVariableFromYaml (yamlRead.h): YAML::LoadFile(path)[key].as<bool>() with yaml-cpp 0.6.2, whose convert<bool>::decode accepts the
// scalars y/n, yes/no, true/false, on/off when they are entirely lower case, Capitalised or entirely UPPER case (IsFlexibleCase) and
// throws on anything else.  The files are flat maps of "key: scalar" lines with '#' comments, as flvis_config_load reads them, and
// this is a reader for such files, not yaml-cpp: a key matches at any indentation (a nested key would match too), and a line is cut
// at its first '#' even inside quotes.
extern "C" int flvis_config_get_bool(const char* path, const char* key, int* out, char* err, int errlen) {
  auto fail = [&](const std::string& m) {
    if (err && errlen > 0) snprintf(err, errlen, "%s", m.c_str());
    return (int)FLVIS_ERR_CONFIG;
  };
  if (!path || !key || !out) return FLVIS_ERR_INVALID_ARG;
  std::ifstream f(path);
  if (!f) return fail(std::string("cannot open ") + path);
  std::string line;
  while (std::getline(f, line)) {
    const size_t h = line.find('#');
    if (h != std::string::npos) line = line.substr(0, h);
    const size_t col = line.find(':');
    if (col == std::string::npos) continue;
    std::string k = line.substr(0, col);
    const size_t a = k.find_first_not_of(" \t");
    if (a == std::string::npos) continue;
    k = k.substr(a);
    k.erase(k.find_last_not_of(" \t") + 1);
    if (k != key) continue;
    std::string v = line.substr(col + 1);
    const size_t b = v.find_first_not_of(" \t\r");
    if (b == std::string::npos) return fail(std::string("yaml key ") + key + " has no value");
    v = v.substr(b);
    v.erase(v.find_last_not_of(" \t\r") + 1);
    if (v.size() >= 2 && (v.front() == '"' || v.front() == '\'') && v.back() == v.front()) v = v.substr(1, v.size() - 2);
    // IsFlexibleCase: lower, Capitalised (first upper, rest lower) or UPPER
    auto all = [&](size_t from, int (*is)(int)) {
      for (size_t i = from; i < v.size(); i++)
        if (!is((unsigned char)v[i])) return false;
      return true;
    };
    const bool flexible = !v.empty() && (all(0, islower) || all(0, isupper) || (isupper((unsigned char)v[0]) && all(1, islower)));
    if (flexible) {
      std::string low = v;
      for (char& ch : low) ch = (char)tolower((unsigned char)ch);
      static const char* names[4][2] = {{"y", "n"}, {"yes", "no"}, {"true", "false"}, {"on", "off"}};
      for (auto& n : names)
        for (int side = 0; side < 2; side++)
          if (low == n[side]) {
            *out = side == 0 ? 1 : 0;
            return FLVIS_OK;
          }
    }
    return fail(std::string("yaml key ") + key + ": '" + v + "' is not a boolean (y/n, yes/no, true/false, on/off)");
  }
  return fail(std::string("yaml key missing: ") + key);
}
