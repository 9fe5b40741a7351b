// flvis_amd: what map_cloud.hip shares with lm_cloud.hip (the local map's cloud ends in the same kernels) and with depth_cloud.hip (the
// dense cloud writes its own points into the voxel workspace and ends in the same sort and output kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"
#include "dev_math.hpp"

namespace flvis {

constexpr int MC_KEY_DIGITS = 8;
constexpr uint64_t MC_DROPPED = 1ull << 63;  // key of a dropped point: behind every voxel of its cloud
constexpr double MC_HALF_RANGE = 1048576.0;  // 2^20

FD uint64_t mc_key(V3 p, double leaf) {
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return MC_DROPPED;
  if (leaf == 0) return 0;
  const double ix = floor(p.x / leaf), iy = floor(p.y / leaf), iz = floor(p.z / leaf);
  if (!(ix >= -MC_HALF_RANGE && ix < MC_HALF_RANGE && iy >= -MC_HALF_RANGE && iy < MC_HALF_RANGE && iz >= -MC_HALF_RANGE && iz < MC_HALF_RANGE))
    return MC_DROPPED;
  return ((uint64_t)((long long)iz + (1 << 20)) << 42) | ((uint64_t)((long long)iy + (1 << 20)) << 21) | (uint64_t)((long long)ix + (1 << 20));
}

// The camera-frame point p_c of pose T (qi = q_conj(T.q)) at canonical index i of the call: the map-frame point (fp64, stored), its voxel
// key and its index go to the voxel workspace, and the key's bytes are marked in the workgroup's table seen [MC_KEY_DIGITS][256] (LDS).
// Both front ends (k_mc_keys, k_dc_keys) put every point through this one function: the bits of a point do not depend on the front end.
FD void mc_put(const SE3d& T, const Q4& qi, V3 p_c, double leaf, size_t i, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
               double* __restrict__ pts, uint8_t* seen) {
  const V3 p = q_rotate(qi, p_c - T.t);
  const uint64_t key = mc_key(p, leaf);
  keys[i] = key;
  idx[i] = (uint32_t)i;
  pts[3 * i] = p.x, pts[3 * i + 1] = p.y, pts[3 * i + 2] = p.z;
  if (key == MC_DROPPED) {
    seen[7 * 256 + 0x80] = 1;  // (a dropped point counts in the top byte alone: it must end up behind the voxels, nothing else)
  } else {
#pragma unroll
    for (int d = 0; d < MC_KEY_DIGITS; d++) seen[d * 256 + (int)((key >> (8 * d)) & 255)] = 1;
  }
}

// One stable sort of N (key, index) pairs by (cloud | key) with map_cloud.hip's radix passes, on the context's stream.
//   h_occ [8][256]: which values each key byte takes over the whole call (a byte with one value is skipped); keys / idx: the two buffers
//   of the passes, the input in [0]; d_cstart [n_clouds + 1]: the clouds' first canonical indices (device), h_cs the same on the host;
//   d_tab: mc_sort_table_ints(N) 32-bit words of workspace.  *cur: the buffer that holds the result.  passes / cloud_digits may be NULL.
size_t mc_sort_table_ints(int N);
int mc_sort(flvis_ctx* ctx, const int* h_occ, uint64_t* const keys[2], uint32_t* const idx[2], int N, int n_clouds, const int* d_cstart,
            const long long* h_cs, uint32_t* d_tab, int* cur, int* passes, int* cloud_digits);

// ---- the parts of a voxel call behind its front end (mc_voxel_cloud and the dense cloud of depth_cloud.hip share them)
// d_off [n + 1]: the running sum of the n counts d_cnt (64-bit); cloud c starts at count d_eptr[c]: d_cs64 / d_cstart [n_clouds + 1]
void mc_offsets(hipStream_t st, const int* d_cnt, long long n, long long* d_off, const int* d_eptr, int n_clouds, long long* d_cs64,
                int* d_cstart);
// the workspace of a call's N points (the context's "mc_points" / "mc_tables" buffers, the byte table cleared on the context's stream)
struct McWork {
  uint64_t* keys[2];   // [N] each; the front end fills [0]
  double* pts;         // [N][3] map-frame points in canonical order
  uint32_t* idx[2];    // [N] each; the front end fills [0] with the canonical index
  int* occ;            // [MC_KEY_DIGITS][256]: the front end sets the byte values its keys take
  uint32_t* hist;      // the passes' tables
  int* bsum;           // output rows per block of sorted positions
  long long* idc;      // [N] ids in canonical order, or NULL
  size_t pt_bytes, tab_ints;
  int n_chunks;
  double* ms_sort_rows = nullptr;  // not NULL: mc_tail waits behind the sort as well and leaves the milliseconds of sort and rows here
};
int mc_work(flvis_ctx* ctx, const char* what, int N, bool ids, McWork& W);
// Everything behind the keys: reads the byte table, sorts, finds and writes the rows, fills h_n_out / h_n_dropped and the context's
// voxel_cloud_stats.  d_kend: 2 (n_clouds + 1) ints of workspace (first dropped positions | first output ranks); h_cs [n_clouds + 1]: the
// clouds' first canonical indices; rows_bytes: what the front end's own tables took (for the stats).
int mc_tail(flvis_ctx* ctx, const char* what, const McWork& W, int N, int n_clouds, const int* d_cstart, int* d_kend, const long long* h_cs,
            double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, long long* d_id_out, int64_t* h_n_out, int64_t* h_n_dropped,
            size_t rows_bytes);

// flvis_hip_voxel_cloud, and with leaf == 0 optionally the id of every output row: d_id_rows [n_rows][cap] the input points' ids,
// d_id_out [n_clouds][out_cap] (both NULL: the public call)
int mc_voxel_cloud(flvis_ctx* ctx, const double* d_p3, const int* d_count, const double* d_T_c_w7, int n_rows, int cap, int n_clouds,
                   const int* h_cloud_ptr, const int* h_range2, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                   const long long* d_id_rows, long long* d_id_out, int64_t* h_n_out, int64_t* h_n_dropped);

// ---- the dense cloud's front end (depth_cloud.hip; include/flvis_hip.h: flvis_hip_depth_cloud).  A listed image and its pose are named
// apart: item e reads image h_img[e] of d_depth [..][h][w] with the pose at d_pose + h_pose[e] * pose_stride (doubles) and the camera
// h_cam5[5 * h_cam[e]]; cloud c holds the items h_eptr[c] .. h_eptr[c + 1].  Arguments are the caller's to check (dc_check_sampling does
// the window, the limits and the cameras).
int dc_check_sampling(int w, int h, const flvis_depth_cloud_params* prm, int n_cams, const double* h_cam5, std::string* why);
int dc_cloud(flvis_ctx* ctx, const char* what, const uint16_t* d_depth, int w, int h, const double* d_pose, size_t pose_stride, int n_clouds,
             const int* h_eptr, const int* h_img, const int* h_pose, const int* h_cam, int n_cams, const double* h_cam5,
             const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out,
             int64_t* h_n_dropped, int64_t* h_n_valid, bool packed = false);
// The stereo forms (flvis_keyframe_log_stereo_cloud, flvis_loop_closer_stereo_cloud): the Z16 values of the log entries `slot` (item e:
// camera h_cam2[2 * cam[e]] = bf, depth_factor) at the samples of `prm` ALONE, 2 bytes per sample, in the context's workspace -- the images
// dc_cloud reads with packed = true and the image list `iota` (item e: image e)
struct KfLogRec;
struct DsGrid;
struct DcUnrect;
int dc_stereo_samples(flvis_ctx* ctx, const char* what, const KfLogRec& rec, const std::vector<int>& slot, const std::vector<int>& cam,
                      const double* h_cam2, const flvis_dense_stereo_params* sprm, const flvis_depth_cloud_params* prm, const uint16_t** d_z,
                      std::vector<int>& iota, const DcUnrect* unrect = nullptr);
// The unrectified rig (cam_type 1): `unrect` names the raw cameras of flvis_hip_rectify (rectify.hip), camera cam[e] of item e in both
// tables; the listed pairs are then rectified RC_BATCH at a time into a workspace of one batch in front of the matcher.
struct DcUnrect {
  int n_cams;
  const double *cam21_0, *cam21_1;  // [n_cams][21]: camera 0 (K0, D0, R0, P0) and camera 1 (K1, D1, R1, P1)
};
// the two cameras of a config (rc_cam21 of its fields)
void dc_unrect_cams(const flvis_cfg& g, double* cam21_0, double* cam21_1);
// items slot[0 .. nb) of the log, rectified into d_out0 / d_out1 [nb][h][w] (either may be NULL)
int dc_rectify_batch(flvis_ctx* ctx, const char* what, const KfLogRec& rec, const int* slot, const int* cam, int nb, const DcUnrect& un,
                     uint8_t* d_out0, uint8_t* d_out1);
// rectify + flvis_hip_dense_stereo batch by batch: item e with camera h_cam2[2 * e] into image e of d_z16 (whole images, or with `grid`
// the samples alone)
int dc_unrect_match(flvis_ctx* ctx, const char* what, const KfLogRec& rec, const int* slot, const int* cam, int n, const DcUnrect& un,
                    const double* h_cam2, const flvis_dense_stereo_params* sprm, uint16_t* d_z16, const DsGrid* grid);
// _host forms: rows of n_clouds clouds staged in the context's `name` buffer, then copied out (rows below min(h_n_out, out_cap))
int mc_host_rows_alloc(flvis_ctx* ctx, const char* what, int n_clouds, int out_cap, float** d_xyz, int** d_npts);
int mc_host_rows_fetch(flvis_ctx* ctx, const char* what, int n_clouds, int out_cap, const int64_t* h_n_out, const float* d_xyz,
                       const int* d_npts, float* h_xyz, int* h_npts);

}  // namespace flvis
