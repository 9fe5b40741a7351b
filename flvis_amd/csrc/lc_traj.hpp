// flvis_amd: whole trajectories in the map frame (lc_traj.hip; include/flvis_hip.h has the definition) -- what the loop closer's calls
// (loop_closer.hip) share with the kernel-level entry, and the pose7 products both sides of the device boundary use.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/flvis_hip.h"

struct flvis_ctx;

namespace flvis {

// ---- pose7 = tx ty tz qx qy qz qw: the products of loop_closer.hip (q_mul, q_rot, pose_mul), operation for operation, for host and
// device; the build has no contraction, so both sides give the same bits ------------------------------------------------------------------
__host__ __device__ __forceinline__ void lct_q_mul(const double* a, const double* b, double* o) {  // Hamilton product, x y z w
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  const double z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = x, o[1] = y, o[2] = z, o[3] = w;
}
__host__ __device__ __forceinline__ void lct_q_rot(const double* q, const double* v, double* o) {  // R(q) v
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * (y * v[2] - z * v[1]), ty = 2 * (z * v[0] - x * v[2]), tz = 2 * (x * v[1] - y * v[0]);
  const double ox = v[0] + w * tx + (y * tz - z * ty);
  const double oy = v[1] + w * ty + (z * tx - x * tz);
  const double oz = v[2] + w * tz + (x * ty - y * tx);
  o[0] = ox, o[1] = oy, o[2] = oz;
}
__host__ __device__ __forceinline__ void lct_pose_mul(const double* a, const double* b, double* o) {  // T_a * T_b (o may be a or b)
  double t[3], q[4];
  lct_q_rot(a + 3, b, t);
  lct_q_mul(a + 3, b + 3, q);
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  o[0] = t[0] + a[0], o[1] = t[1] + a[1], o[2] = t[2] + a[2];
  o[3] = q[0] / n, o[4] = q[1] / n, o[5] = q[2] / n, o[6] = q[3] / n;
}
__host__ __device__ __forceinline__ void lct_pose_inv(const double* T, double* o) {  // (-(R(q*) t), q*), q* = (-x, -y, -z, w)
  const double qc[4] = {-T[3], -T[4], -T[5], T[6]};
  double r[3];
  lct_q_rot(qc, T, r);
  o[0] = -r[0], o[1] = -r[1], o[2] = -r[2];
  o[3] = qc[0], o[4] = qc[1], o[5] = qc[2], o[6] = qc[3];
}

// doubles per row of a kind (FLVIS_LC_ROWS_*), 0 for no such kind
inline int lct_row_width(int kind) { return kind == FLVIS_LC_ROWS_POSE8 ? 8 : kind == FLVIS_LC_ROWS_TRAJ9 ? 9 : kind == FLVIS_LC_ROWS_IMU11 ? 11 : 0; }

// the argument checks of flvis_hip_lc_map_poses that need no device: FLVIS_OK, or the code with the message in the context
int lc_map_poses_check(flvis_ctx* ctx, const char* what, int n_seq, int kf_stride, const int* h_nkf, int n_jobs, const flvis_lc_traj_job* h_jobs,
                       int mode);
// flvis_hip_lc_map_poses.  check_stamps: the sequences' stamps are looked at on the device (the closer has checked its own on the host).
// Returns synchronised with the context's stream: the rows are written, and host memory handed in may go away.
int lc_map_poses_dev(flvis_ctx* ctx, const char* what, int n_seq, int kf_stride, const int* h_nkf, const double* d_T_odom, const double* d_T_map,
                     const double* d_stamps, const double* h_drift7, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode, bool check_stamps);
// The tracker of the context with everything it has queued waited for: its stream count and image shape and, per stream, the device rows
// of its trajectory record ([cap][9]; NULL without a record).  FLVIS_ERR_INVALID_ARG without a tracker.
int lc_traj_tracker_rows(flvis_ctx* ctx, int& S, int& w, int& h, int& cam_type, std::vector<const double*>& d_rows, std::vector<int>& cap);

}  // namespace flvis
