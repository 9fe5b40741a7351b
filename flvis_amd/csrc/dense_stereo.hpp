// flvis_amd: dense stereo (dense_stereo.hip) for the calls that feed it from the keyframe log
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/flvis_hip.h"

struct flvis_ctx;

namespace flvis {
// the samples a cloud call keeps of a Z16 image: u = u0 + i * su (i < nu), v = v0 + j * sv (j < nv); su == 0: every pixel
struct DsGrid {
  int u0, v0, su, sv, nu, nv;
};
// the host-only argument check of flvis_hip_dense_stereo (h_cam2 [n_cam][2] = bf, depth_factor); *why names the refusal
int ds_check(int n_img, int w, int h, int n_cam, const double* h_cam2, const flvis_dense_stereo_params* prm, std::string* why);
// flvis_hip_dense_stereo under another call's name.  h_src (may be NULL) [n_img]: item i reads image h_src[i] of d_img0 / d_img1 and writes
// output image i.  grid (may be NULL; then d_disp16 must be): d_z16 is [n_img][nv][nu] and holds the grid's samples alone.
int ds_run(flvis_ctx* ctx, const char* what, const uint8_t* d_img0, const uint8_t* d_img1, int n_img, int w, int h, int n_cam,
           const double* h_cam2, const flvis_dense_stereo_params* prm, uint16_t* d_disp16, uint16_t* d_z16, const int* h_src, const DsGrid* grid);
}  // namespace flvis
