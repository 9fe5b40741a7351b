// flvis_amd: rectification of raw image batches (rectify.hip) for the calls that feed it from the keyframe log
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/flvis_hip.h"

struct flvis_ctx;

namespace flvis {
constexpr int RC_BATCH = 64;  // pairs rectified at a time by the calls that read the keyframe log (the workspace holds one batch)
// a camera of flvis_hip_rectify from a config's fields: K (4) | D (4) | R (9) | fx' fy' cx' cy' of P (3 x 4, row-major)
void rc_cam21(const double* K4, const double* D4, const double* R9, const double* P12, double* cam21);
// the host-only argument check of flvis_hip_rectify but for the pointers (every camera, n_cam against n_img and h_cam_of); *why names
// the refusal
int rc_check(int n_img, int w, int h, int n_cam, const double* h_cam21, const int* h_cam_of, std::string* why);
// flvis_hip_rectify under another call's name, arguments checked by the caller.  h_src_of (may be NULL) [n_img]: item i reads image
// h_src_of[i] of d_src and writes image i of d_dst (and d_covered).
int rc_run(flvis_ctx* ctx, const char* what, const uint8_t* d_src, int n_img, int w, int h, int n_cam, const double* h_cam21,
           const int* h_cam_of, const int* h_src_of, uint8_t* d_dst, uint8_t* d_covered);
}  // namespace flvis
