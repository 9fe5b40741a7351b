// flvis_amd: the solver calls of the front-end's tracking step on caller arrays -- what LKORBTracking::tracking
// (src/processing/lkorb_tracking.cpp:9-202) and OptimizeInFrame::optimize (src/processing/optimize_in_frame.cpp:10-91) call between the
// optical flow and the pose, each as one call batched over n_sets independent sets (a set is one frame), on the context's stream:
//   flvis_hip_find_fundamental_ransac  cv::findFundamentalMat(FM_RANSAC)   k_fund_ransac_sets (track_kernels.hip: the tracker's search)
//   flvis_hip_optimize_in_frame        OptimizeInFrame::optimize           k_pose_lm_sets     (track_kernels.hip: the tracker's pose LM)
//   flvis_hip_undistort_points         cv::undistortPoints(K, D, R, P)     k_undistort_points_sets   (here; dev_geom.hpp's undistort_point)
//   flvis_hip_project_points           cv::projectPoints                   k_project_points_sets     (here; dev_geom.hpp's project_point)
// A count above cap reads as cap, a negative one as 0; rows from the count on are never written; argument errors are refused before
// anything is launched or written; host arrays go to the device (scratch) before the call returns.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "dev_common.hpp"
#include "dev_geom.hpp"
#include "dev_math.hpp"
#include "track_kernels.hpp"

namespace flvis {

// one thread per point, blockIdx.y the set (as k_sd_seeds); set s's camera at cam + cam_stride * s
__global__ __launch_bounds__(256) void k_undistort_points_sets(const float* __restrict__ src, const int* __restrict__ count, int cap,
                                                               const double* __restrict__ cam, int cam_stride, float* __restrict__ dst) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count[s] || i >= cap) return;
  const size_t k = (size_t)s * cap + i;
  const double* const c = cam + (size_t)cam_stride * s;
  const float in[2] = {src[2 * k], src[2 * k + 1]};
  float out[2];
  undistort_point(in, c, c + 4, c + 8, c + 17, out);
  dst[2 * k] = out[0];
  dst[2 * k + 1] = out[1];
}

__global__ __launch_bounds__(256) void k_project_points_sets(const float* __restrict__ p3d, const int* __restrict__ count, int cap,
                                                             const double* __restrict__ pose7, const double* __restrict__ cam,
                                                             int cam_stride, float* __restrict__ dst) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count[s] || i >= cap) return;
  const size_t k = (size_t)s * cap + i;
  const double* const c = cam + (size_t)cam_stride * s;
  const SE3d T = load_pose7(pose7 + 7 * (size_t)s);
  const float p3[3] = {p3d[3 * k], p3d[3 * k + 1], p3d[3 * k + 2]};
  float out[2];
  project_point(p3, q_to_mat(T.q), T.t, c, c + 4, out);
  dst[2 * k] = out[0];
  dst[2 * k + 1] = out[1];
}

void launch_undistort_points_sets(hipStream_t st, const float* src, const int* count, int cap, int n_sets, const double* d_cam, int cam_stride,
                                  float* dst) {
  hipLaunchKernelGGL(k_undistort_points_sets, dim3((cap + 255) / 256, n_sets), dim3(256), 0, st, src, count, cap, d_cam, cam_stride, dst);
}
void launch_project_points_sets(hipStream_t st, const float* p3d, const int* count, int cap, int n_sets, const double* d_pose7,
                                const double* d_cam, int cam_stride, float* dst) {
  hipLaunchKernelGGL(k_project_points_sets, dim3((cap + 255) / 256, n_sets), dim3(256), 0, st, p3d, count, cap, d_pose7, d_cam, cam_stride, dst);
}

// host doubles -> a named scratch buffer, complete when this returns (the caller's arrays are pageable and may be freed)
static int upload_doubles(flvis_ctx* ctx, const char* name, const std::vector<double>& h, double** out) {
  double* d = (double*)ctx->scratch(name, sizeof(double) * h.size());
  if (!d) return ctx->fail(FLVIS_ERR_HIP, std::string(name) + ": scratch allocation failed");
  hipError_t e = hipMemcpyAsync(d, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, name);
  *out = d;
  return FLVIS_OK;
}

}  // namespace flvis

using namespace flvis;

#define CHECK_CTX(c) \
  if (!(c)) return FLVIS_ERR_INVALID_ARG;
#define CHECK_LAUNCH(c, what)                           \
  do {                                                  \
    hipError_t e__ = hipGetLastError();                 \
    if (e__ != hipSuccess) return (c)->hip_fail(e__, what); \
  } while (0)

// the grid's y extent is the number of sets
static constexpr int GEOM_MAX_SETS = 65535;

extern "C" {

int flvis_hip_find_fundamental_ransac(flvis_ctx* ctx, const float* d_m1, const float* d_m2, const int* d_count, int cap, int n_sets,
                                      double thr_px, double confidence, uint8_t* d_mask, int* d_n_inliers) {
  CHECK_CTX(ctx);
  if (!d_m1 || !d_m2 || !d_count || !d_mask || !d_n_inliers || cap <= 0 || n_sets <= 0)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "find_fundamental_ransac: bad args");
  if (!(thr_px > 0.0) || !std::isfinite(thr_px) || !(confidence > 0.0 && confidence < 1.0))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "find_fundamental_ransac: thr_px must be > 0 and confidence inside (0, 1)");
  if (cap > fund_ransac_max_points())
    return ctx->fail(FLVIS_ERR_CAPACITY, "find_fundamental_ransac: cap > 1024 (the candidate tables and the LDS staging hold 1024 points)");
  hipSetDevice(ctx->device);
  launch_fund_ransac_sets(ctx->stream, d_m1, d_m2, d_count, cap, n_sets, thr_px, confidence, d_mask, d_n_inliers);
  CHECK_LAUNCH(ctx, "find_fundamental_ransac");
  return FLVIS_OK;
}

int flvis_hip_optimize_in_frame(flvis_ctx* ctx, const double* d_lm_3d_w, const double* d_lm_2d_undistort, const int64_t* d_lm_id,
                                const int* d_count, int cap, int n_sets, const double* h_K4, int n_K, double* d_pose7, uint8_t* d_ok) {
  CHECK_CTX(ctx);
  if (!d_lm_3d_w || !d_lm_2d_undistort || !d_lm_id || !d_count || !h_K4 || !d_pose7 || !d_ok || cap <= 0 || n_sets <= 0 ||
      (n_K != 1 && n_K != n_sets))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "optimize_in_frame: bad args (n_K is 1 or n_sets)");
  if (cap > pose_lm_max_edges())
    return ctx->fail(FLVIS_ERR_CAPACITY, "optimize_in_frame: cap > 512 (the edges of one pose optimisation are held in LDS)");
  hipSetDevice(ctx->device);
  double* k4 = nullptr;
  const int rc = upload_doubles(ctx, "geom_K4", std::vector<double>(h_K4, h_K4 + 4 * (size_t)n_K), &k4);
  if (rc != FLVIS_OK) return rc;
  const hipError_t e = launch_pose_lm_sets(ctx->stream, d_lm_3d_w, d_lm_2d_undistort, (const long long*)d_lm_id, d_count, cap, n_sets, k4,
                                           n_K == 1 ? 0 : 4, d_pose7, d_ok);
  if (e != hipSuccess) return ctx->hip_fail(e, "optimize_in_frame");
  CHECK_LAUNCH(ctx, "optimize_in_frame");
  return FLVIS_OK;
}

int flvis_hip_undistort_points(flvis_ctx* ctx, const float* d_src, const int* d_count, int cap, int n_sets, const double* h_K4,
                               const double* h_D4, const double* h_R9, const double* h_P12, int n_cam, float* d_dst) {
  CHECK_CTX(ctx);
  if (!d_src || !d_count || !h_K4 || !h_D4 || !h_R9 || !h_P12 || !d_dst || cap <= 0 || n_sets <= 0 || n_sets > GEOM_MAX_SETS ||
      (n_cam != 1 && n_cam != n_sets))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "undistort_points: bad args (n_cam is 1 or n_sets, n_sets <= 65535)");
  hipSetDevice(ctx->device);
  std::vector<double> h((size_t)GEOM_CAM_N * n_cam);
  for (int c = 0; c < n_cam; c++) {
    double* o = &h[(size_t)GEOM_CAM_N * c];
    memcpy(o, h_K4 + 4 * (size_t)c, 32);
    memcpy(o + 4, h_D4 + 4 * (size_t)c, 32);
    memcpy(o + 8, h_R9 + 9 * (size_t)c, 72);
    memcpy(o + 17, h_P12 + 12 * (size_t)c, 96);
  }
  double* cam = nullptr;
  const int rc = upload_doubles(ctx, "geom_cam", h, &cam);
  if (rc != FLVIS_OK) return rc;
  launch_undistort_points_sets(ctx->stream, d_src, d_count, cap, n_sets, cam, n_cam == 1 ? 0 : GEOM_CAM_N, d_dst);
  CHECK_LAUNCH(ctx, "undistort_points");
  return FLVIS_OK;
}

int flvis_hip_project_points(flvis_ctx* ctx, const float* d_p3d, const int* d_count, int cap, int n_sets, const double* h_pose7,
                             const double* h_K4, const double* h_D4, int n_cam, float* d_dst) {
  CHECK_CTX(ctx);
  if (!d_p3d || !d_count || !h_pose7 || !h_K4 || !h_D4 || !d_dst || cap <= 0 || n_sets <= 0 || n_sets > GEOM_MAX_SETS ||
      (n_cam != 1 && n_cam != n_sets))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "project_points: bad args (n_cam is 1 or n_sets, n_sets <= 65535)");
  hipSetDevice(ctx->device);
  // one upload: the cameras (K, D; the R / P slots stay empty), then the poses
  std::vector<double> h((size_t)GEOM_CAM_N * n_cam + 7 * (size_t)n_sets, 0.0);
  for (int c = 0; c < n_cam; c++) {
    double* o = &h[(size_t)GEOM_CAM_N * c];
    memcpy(o, h_K4 + 4 * (size_t)c, 32);
    memcpy(o + 4, h_D4 + 4 * (size_t)c, 32);
  }
  memcpy(&h[(size_t)GEOM_CAM_N * n_cam], h_pose7, sizeof(double) * 7 * (size_t)n_sets);
  double* cam = nullptr;
  const int rc = upload_doubles(ctx, "geom_cam", h, &cam);
  if (rc != FLVIS_OK) return rc;
  launch_project_points_sets(ctx->stream, d_p3d, d_count, cap, n_sets, cam + (size_t)GEOM_CAM_N * n_cam, cam, n_cam == 1 ? 0 : GEOM_CAM_N,
                             d_dst);
  CHECK_LAUNCH(ctx, "project_points");
  return FLVIS_OK;
}

}  // extern "C"
