// flvis_amd: what loop_kernels.hip offers the loop closer (loop_closer.hip) beside the C ABI -- the two kernels that read a camera, on a
// camera table that is already resident on the device.
#pragma once
#include <cstdint>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"

namespace flvis {

// one camera of the loop closing (a row of the device table k_lc_landmarks and k_pnp_ransac_sets index)
struct LcCam {
  double P0[12], P1[12];  // STEREO_RECT: the rectified projection matrices (dc.P0_, dc.P1_)
  double fx, fy, cx, cy;  // DEPTH_D435 back-projection and the K of solvePnPRansac (dc.K0_rect)
};
constexpr int LC_CAM_DOUBLES = 28;  // a row as doubles: the stride of &cams[0].fx for pnp_ransac_dev
static_assert(sizeof(LcCam) == LC_CAM_DOUBLES * sizeof(double), "LcCam is a plain row of doubles");

// flvis_hip_lc_keyframe_landmarks_rigs on a DEVICE table: image i uses d_cams[d_cam_of ? d_cam_of[i] : i].  Uploads nothing.
int lc_keyframe_landmarks_dev(flvis_ctx* ctx, const uint8_t* d_img0, const void* d_img1, int w, int h, int n_img, int cam_type, const LcCam* d_cams,
                              const int* d_cam_of, const float* d_kps, const uint8_t* d_desc, const int* d_count, int cap, float* d_lm_2d,
                              double* d_lm_3d, uint8_t* d_lm_desc, int* d_lm_count);
// what flvis_hip_lc_keyframe_landmarks_unrect reads of a STEREO_UNRECT rig beside its row's P0 / P1: both raw cameras' pinhole + radtan
// models and rectifying rotations.  A table of its own with the same row index, so that LcCam -- and with it every load of the
// STEREO_RECT / DEPTH_D435 kernel and of the PnP RANSAC -- stays as it is.
struct LcCamUnrect {
  double K0[4], D0[4], R0[9], K1[4], D1[4], R1[9];
};
// flvis_hip_lc_keyframe_landmarks_unrect on DEVICE tables: image i uses row d_cam_of ? d_cam_of[i] : i of both.  Uploads nothing.
int lc_keyframe_landmarks_unrect_dev(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, int w, int h, int n_img, const LcCam* d_cams,
                                     const LcCamUnrect* d_ucams, const int* d_cam_of, const float* d_kps, const uint8_t* d_desc,
                                     const int* d_count, int cap, float* d_lm_2d, double* d_lm_3d, uint8_t* d_lm_desc, int* d_lm_count);
// the two rows of a finalized config
void lc_cam_of_cfg(const flvis_cfg& c, LcCam* cam);
void lc_cam_unrect_of_cfg(const flvis_cfg& c, LcCamUnrect* cam);
// flvis_hip_pnp_ransac_rigs on a DEVICE table: set i uses fx fy cx cy = d_K4 + k4_stride * (d_cam_of ? d_cam_of[i] : i) (k4_stride in
// doubles).  d_K4 == nullptr: every set uses h_K4.  (h_seeds is uploaded as in flvis_hip_pnp_ransac.)  iterative: the tracker's branch
// (flvis_hip_debug_pnp_ransac_iterative) with set i's fallback pose at d_guess7 + 7 i, on the device; h_seeds may then be nullptr.
int pnp_ransac_dev(flvis_ctx* ctx, const float* d_p3d, const float* d_p2d, const int* d_count, int cap, int n_sets, const double* h_K4,
                   const double* d_K4, int k4_stride, const int* d_cam_of, int iterations, double reproj_px, double confidence,
                   const uint64_t* h_seeds, double* d_pose7, uint8_t* d_inlier_mask, int* d_n_inliers, bool iterative = false,
                   const double* d_guess7 = nullptr);
// flvis_hip_lc_select_maps, and with compact its form for rows that hold segment d_map[q] alone ([n_q][seg_len], every d_map[q] >= 0): the
// loop closer's layout for a call in which no query searches all maps.  d_skip: flvis_hip_lc_select_maps_skip's excluded ranges [n_q][2] in
// global indices (both row forms), or nullptr: none, the kernel without the range test
int lc_select_maps_dev(flvis_ctx* ctx, int n_q, const double* d_scores, int n_seg, int seg_len, const int* d_seg_n, const int* d_map,
                       const int* d_skip, bool compact, int n_best, double min_score, int* d_idx, double* d_score, int* d_count);

// flvis_loop_closer_merge's two kernels.  A sequence of a group, as the apply kernel sees it: its keyframes are database slots db_base ..
// db_base + n - 1 and rows v_base .. v_base + n - 1 of the batch of virtual sequences; keyframes first .. v_s are vertices of the joint graph.
struct LcMergeSeq {
  int db_base, v_base, first, v_s, n;
};
// d_V[r] = d_db_T[d_src[r]], or the identity pose for an absent row (d_src[r] < 0): every group's virtual sequence in one launch
int lc_merge_gather_dev(flvis_ctx* ctx, const int* d_src, int n_rows, const double* d_db_T, double* d_V);
// the optimised rows back into d_db_T, the rows behind a sequence's last vertex times its drift, the drifts into d_drift7 [n_seqs][7]
int lc_merge_apply_dev(flvis_ctx* ctx, const LcMergeSeq* d_seqs, int n_seqs, const double* d_V, double* d_db_T, double* d_drift7);

}  // namespace flvis
