// flvis_amd: what occupancy.hip shares with the loop closer (flvis_loop_closer_occupancy lists the logged images under the closer's stored
// poses and ends in the same batched walk as flvis_keyframe_log_occupancy).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>

#include "../../include/flvis_hip.h"

struct flvis_ctx;

namespace flvis {

// The listed images of a call, named as dc_cloud names them (map_cloud.hpp): item e reads image img[e] of d_depth [..][h][w] with the pose
// at d_pose + pose[e] * pose_stride (doubles) and the camera cam5[5 * cam[e]]; map m holds the items eptr[m] .. eptr[m + 1] - 1, which are
// its scans 0, 1, .. in this order.
struct OcLists {
  const uint16_t* d_depth;
  int w, h;
  const double* d_pose;
  size_t pose_stride;
  int n_maps;
  const int *eptr, *img, *pose, *cam;
  int n_cams;
  const double* cam5;
};
struct OcOut {
  int out_cap;
  int64_t* d_key;  // [n_maps][out_cap]
  float* d_l;      // [n_maps][out_cap]
  float* d_xyz;    // [n_maps][out_cap][3] or NULL
};

// leaf and the four log-odds of a call
int oc_check_values(double leaf, const flvis_occupancy_params* occ, std::string* why);
// The scans of `L` in batches of at most max_records records (0: 2^26), the map carried from batch to batch as the prior in two buffers of
// the context; the last batch writes `out`.  name_of(e): what to call item e in a message.  Arguments are the caller's to check
// (dc_check_sampling, oc_check_values).
int oc_batched(flvis_ctx* ctx, const char* what, const OcLists& L, const flvis_depth_cloud_params* prm, double leaf,
               const flvis_occupancy_params* occ, int64_t max_records, const OcOut& out, int64_t* h_n_out, int64_t* h_n_rays,
               int64_t* h_n_dropped, int* h_n_batches, const std::function<std::string(int)>& name_of);
// _host forms: the rows of n maps staged in the context's buffer, then copied out (rows below min(h_n_out, out_cap))
int oc_host_alloc(flvis_ctx* ctx, const char* what, int n, int out_cap, bool xyz, OcOut* out);
int oc_host_fetch(flvis_ctx* ctx, const char* what, int n, const OcOut& dev, const int64_t* h_n_out, int64_t* h_key, float* h_l, float* h_xyz);

}  // namespace flvis
