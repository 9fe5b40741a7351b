// flvis_amd: a dense map from depth keyframes (flvis_hip_depth_cloud, flvis_keyframe_log_depth_cloud; include/flvis_hip.h has the
// definition).
//
// The reference's octomap feeder (src/octofeeder/octomap_feeder.cpp:18-80) back-projects the depth image of every /vo_kf message into a
// camera-frame cloud.  Here the samples of every listed image go straight into the voxel filter of map_cloud.hip: this file is a second
// front end of that call, and the 24-byte camera-frame rows a caller of flvis_hip_voxel_cloud would have to build never exist.
//
// Steps of one call (every cloud of the call goes through each of them together):
//   k_dc_count                 one workgroup per listed image and row chunk (whole sampled rows, about DC_CHUNK samples): its valid samples
//   mc_offsets                 map_cloud.hip's scan over (image, chunk): where each chunk's points start in canonical order
//   k_dc_keys                  the same workgroups again: every valid sample's camera-frame point by the tracker's depth rule, then mc_put
//                              (map_cloud.hpp) -- map-frame point, voxel key, index, key bytes -- at the sample's canonical position
//   mc_tail                    map_cloud.hip from the sort on, unchanged
// Raster order inside a chunk comes from the layout alone: a round is 256 consecutive samples, wave w of the workgroup owns 64 consecutive
// ones, a lane's position is the round's base + the valid samples of the waves before its own (per-wave counts in LDS) + the valid lanes
// below it in its wave (ballot, prefix popcount).  No atomic decides a position.
// Loads: a lane reads one 16-bit pixel; with step_u == 1 a wave reads 128 contiguous bytes, with step_u == 7 it touches 7 lines of 128
// bytes for 64 pixels.  Reading whole row segments instead would cut the lines touched but the kernel is bound by what it WRITES (36
// bytes per valid sample); profiles/r25_depth_cloud.md has the figures.
// A second image layout (DcSamp::packed) serves the stereo forms (flvis_keyframe_log_stereo_cloud, flvis_loop_closer_stereo_cloud): the
// Z16 values dense_stereo.hip computes are kept at the samples alone, [item][nv][nu], so a sample is read at its own index and still
// back-projected from its pixel.  Everything else -- lists, poses read in place, counts, keys, the tail -- is the depth-rig path.
// The unrectified stereo rig (cam_type 1: flvis_keyframe_log_unrect_stereo_cloud, flvis_loop_closer_unrect_stereo_cloud) adds a source
// stage in front of the matcher: the listed pairs go through rectify.hip RC_BATCH at a time into a workspace of one batch, and the matcher
// runs batch by batch with its outputs offset (dc_unrect_match).  The workspace does not grow with the number of listed keyframes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "dc_samp.hpp"
#include "dense_stereo.hpp"
#include "dev_math.hpp"
#include "kf_log.hpp"
#include "map_cloud.hpp"
#include "pipeline_host.hpp"
#include "rectify.hpp"

namespace {

using namespace flvis;

// the call's listed images ("items"), cloud after cloud in the caller's order
struct DcItems {
  const int *img, *pose, *cam;  // [R]: the image, its pose row and its camera
  const double* cam5;           // [n_cams][5] fx fy cx cy depth_factor
  const uint16_t* depth;
  const double* pose7;
  size_t pose_stride;  // doubles between two pose rows
};

// grid: items x chunks (chunk fastest); cnt[block] = the chunk's valid samples
__global__ __launch_bounds__(DC_T) void k_dc_count(DcItems it, DcSamp s, int* __restrict__ cnt) {
  __shared__ int wsum[DC_T / 64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int e = blockIdx.x / s.chunks, c = blockIdx.x - e * s.chunks;
  const uint16_t* img = it.depth + (size_t)it.img[e] * s.img_px();
  const double df = it.cam5[5 * (size_t)it.cam[e] + 4];
  const int n = dc_chunk_samples(s, c);
  int mine = 0;  // (lane 0: the wave's count)
  for (int j0 = 0; j0 < n; j0 += DC_T) {
    const int j = j0 + t;
    bool f = false;
    if (j < n) {
      int u, v;
      float z;
      const size_t at = dc_pixel(s, c, j, u, v);
      f = dc_valid(img[at], df, s, z);
    }
    mine += __popcll(__ballot(f));
  }
  if (lane == 0) wsum[w] = mine;
  __syncthreads();
  if (t == 0) {
    int a = 0;
#pragma unroll
    for (int k = 0; k < DC_T / 64; k++) a += wsum[k];
    cnt[blockIdx.x] = a;
  }
}

// the same grid; off[block]: the chunk's first canonical index
__global__ __launch_bounds__(DC_T) void k_dc_keys(DcItems it, DcSamp s, const int* __restrict__ cnt, const long long* __restrict__ off, double leaf,
                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, double* __restrict__ pts,
                                                  int* __restrict__ occ) {
  __shared__ uint8_t seen[MC_KEY_DIGITS * 256];
  __shared__ int wsum[DC_T / 64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (cnt[blockIdx.x] == 0) return;
  for (int i = t; i < MC_KEY_DIGITS * 256; i += DC_T) seen[i] = 0;
  __syncthreads();
  const int e = blockIdx.x / s.chunks, c = blockIdx.x - e * s.chunks;
  const uint16_t* img = it.depth + (size_t)it.img[e] * s.img_px();
  const double* cam = it.cam5 + 5 * (size_t)it.cam[e];
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], df = cam[4];
  const SE3d T = load_pose7(it.pose7 + (size_t)it.pose[e] * it.pose_stride);
  const Q4 qi = q_conj(T.q);
  const size_t base = (size_t)off[blockIdx.x];
  const int n = dc_chunk_samples(s, c);
  int done = 0;
  for (int j0 = 0; j0 < n; j0 += DC_T) {
    const int j = j0 + t;
    bool f = false;
    int u = 0, v = 0;
    float z = 0.f;
    if (j < n) {
      const size_t at = dc_pixel(s, c, j, u, v);
      f = dc_valid(img[at], df, s, z);
    }
    const unsigned long long bal = __ballot(f);
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int at = done + __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int k = 0; k < DC_T / 64; k++) {
      at += k < w ? wsum[k] : 0;
      total += wsum[k];
    }
    if (f) {
      const double zd = (double)z;
      const V3 p_c{((double)u - cx) * zd / fx, ((double)v - cy) * zd / fy, zd};
      mc_put(T, qi, p_c, leaf, base + (size_t)at, keys, idx, pts, seen);
    }
    __syncthreads();
    done += total;
  }
#pragma unroll
  for (int d = 0; d < MC_KEY_DIGITS; d++)
    if (seen[d * 256 + t]) occ[d * 256 + t] = 1;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

namespace flvis {

int dc_check_sampling(int w, int h, const flvis_depth_cloud_params* prm, int n_cams, const double* h_cam5, std::string* why) {
  DcSamp s;
  std::string m;
  int rc = dc_resolve(w, h, prm, s, m);
  if (rc == FLVIS_OK && n_cams > 0 && !h_cam5) rc = FLVIS_ERR_INVALID_ARG, m = "NULL cameras";
  for (int k = 0; rc == FLVIS_OK && k < n_cams; k++) {
    const double* c = h_cam5 + 5 * (size_t)k;
    bool ok = c[0] != 0 && c[1] != 0 && c[4] != 0;
    for (int j = 0; j < 5; j++) ok = ok && std::isfinite(c[j]);
    if (!ok) rc = FLVIS_ERR_INVALID_ARG, m = "camera " + std::to_string(k) + " is not finite or has a zero fx, fy or depth_factor";
  }
  if (why) *why = m;
  return rc;
}

int dc_grid(int w, int h, const flvis_depth_cloud_params* prm, DsGrid* g) {
  DcSamp s;
  std::string why;
  const int rc = dc_resolve(w, h, prm, s, why);
  if (rc == FLVIS_OK) *g = DsGrid{s.u0, s.v0, s.su, s.sv, s.nu, s.nv};
  return rc;
}

void dc_unrect_cams(const flvis_cfg& g, double* cam21_0, double* cam21_1) {
  rc_cam21(g.cam0_intrinsics, g.cam0_distortion, g.R0, g.P0, cam21_0);
  rc_cam21(g.cam1_intrinsics, g.cam1_distortion, g.R1, g.P1, cam21_1);
}

int dc_rectify_batch(flvis_ctx* ctx, const char* what, const KfLogRec& rec, const int* slot, const int* cam, int nb, const DcUnrect& un,
                     uint8_t* d_out0, uint8_t* d_out1) {
  int rc = FLVIS_OK;
  if (d_out0) rc = rc_run(ctx, what, rec.img0, nb, rec.w, rec.h, un.n_cams, un.cam21_0, cam, slot, d_out0, nullptr);
  if (rc == FLVIS_OK && d_out1) rc = rc_run(ctx, what, rec.img1, nb, rec.w, rec.h, un.n_cams, un.cam21_1, cam, slot, d_out1, nullptr);
  return rc;
}

int dc_unrect_match(flvis_ctx* ctx, const char* what, const KfLogRec& rec, const int* slot, const int* cam, int n, const DcUnrect& un,
                    const double* h_cam2, const flvis_dense_stereo_params* sprm, uint16_t* d_z16, const DsGrid* grid) {
  const size_t px = rec.px(), out_px = grid ? (size_t)grid->nu * grid->nv : px;
  uint8_t* const pair = (uint8_t*)ctx->scratch("rc_pair", 2 * (size_t)std::min(n, RC_BATCH) * px);
  if (!pair) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  uint8_t* const pair1 = pair + (size_t)std::min(n, RC_BATCH) * px;
  for (int i0 = 0; i0 < n; i0 += RC_BATCH) {
    const int nb = std::min(RC_BATCH, n - i0);
    int rc = dc_rectify_batch(ctx, what, rec, slot + i0, cam + i0, nb, un, pair, pair1);
    if (rc != FLVIS_OK) return rc;
    rc = ds_run(ctx, what, pair, pair1, nb, rec.w, rec.h, nb, h_cam2 + 2 * (size_t)i0, sprm, nullptr, d_z16 + (size_t)i0 * out_px, nullptr, grid);
    if (rc != FLVIS_OK) return rc;
  }
  return FLVIS_OK;
}

int dc_stereo_samples(flvis_ctx* ctx, const char* what, const KfLogRec& rec, const std::vector<int>& slot, const std::vector<int>& cam,
                      const double* h_cam2, const flvis_dense_stereo_params* sprm, const flvis_depth_cloud_params* prm, const uint16_t** d_z,
                      std::vector<int>& iota, const DcUnrect* unrect) {
  DsGrid g;
  int rc = dc_grid(rec.w, rec.h, prm, &g);
  if (rc != FLVIS_OK) return ctx->fail(rc, std::string(what) + ": bad sampling");
  const size_t R = slot.size();
  iota.resize(R);
  std::vector<double> cam2(2 * std::max<size_t>(R, 1));
  for (size_t e = 0; e < R; e++) iota[e] = (int)e, cam2[2 * e] = h_cam2[2 * (size_t)cam[e]], cam2[2 * e + 1] = h_cam2[2 * (size_t)cam[e] + 1];
  uint16_t* z = (uint16_t*)ctx->scratch("ds_z16", 2 * std::max<size_t>(R, 1) * g.nu * g.nv);
  if (!z) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  *d_z = z;
  if (R == 0) return FLVIS_OK;
  if (unrect) return dc_unrect_match(ctx, what, rec, slot.data(), cam.data(), (int)R, *unrect, cam2.data(), sprm, z, &g);
  return ds_run(ctx, what, rec.img0, rec.img1, (int)R, rec.w, rec.h, (int)R, cam2.data(), sprm, nullptr, z, slot.data(), &g);
}

int dc_cloud(flvis_ctx* ctx, const char* what, const uint16_t* d_depth, int w, int h, const double* d_pose, size_t pose_stride, int n_clouds,
             const int* h_eptr, const int* h_img, const int* h_pose, const int* h_cam, int n_cams, const double* h_cam5,
             const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out,
             int64_t* h_n_dropped, int64_t* h_n_valid, bool packed) {
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  if (!d_depth || !d_pose || !h_n_out || n_clouds <= 0 || !h_eptr) return bad("a NULL required pointer or no cloud");
  if (!(leaf >= 0) || !std::isfinite(leaf)) return bad("leaf must be finite and >= 0");
  if (min_points < 1) return bad("min_points < 1");
  if (out_cap < 0) return bad("out_cap < 0");
  if (!d_xyz && out_cap != 0) return bad("NULL rows with out_cap > 0");
  DcSamp s;
  std::string why;
  int rc = dc_check_sampling(w, h, prm, n_cams, h_cam5, &why);
  if (rc == FLVIS_OK) rc = dc_resolve(w, h, prm, s, why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  s.packed = packed ? 1 : 0;
  const int R = h_eptr[n_clouds], NC1 = n_clouds + 1;
  for (int c = 0; c < n_clouds; c++) {
    h_n_out[c] = 0;
    if (h_n_dropped) h_n_dropped[c] = 0;
    if (h_n_valid) h_n_valid[c] = 0;
  }
  memset(ctx->mc_stats, 0, sizeof(ctx->mc_stats));
  if (R == 0) return FLVIS_OK;
  const long long M64 = (long long)R * s.chunks;
  if (M64 > INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 (listed image, row chunk) pairs or more");
  const int M = (int)M64;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const bool timing = ctx->dc_timing != 0;
  if (timing) hipStreamSynchronize(st);
  auto t0 = std::chrono::steady_clock::now();
  // ---- tables: off64 [M + 1] | cs64 [NC1] | cam5 [n_cams][5] || eptr * chunks [NC1] | img [R] | pose [R] | cam [R] || cnt [M] | cstart [NC1] |
  //      kend [NC1] | cg [NC1]   (|| .. ||: one upload)
  const size_t up_bytes = 8 * 5 * (size_t)n_cams + 4 * ((size_t)NC1 + 3 * (size_t)R);
  const size_t rows_bytes = 8 * ((size_t)M + 1 + NC1) + up_bytes + 4 * ((size_t)M + 3 * (size_t)NC1);
  uint8_t* const rb = (uint8_t*)ctx->scratch("dc_rows", rows_bytes);
  if (!rb) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, pre + "device allocation failed");
  }
  long long* const d_off = (long long*)rb;
  long long* const d_cs64 = d_off + M + 1;
  double* const d_cam5 = (double*)(d_cs64 + NC1);
  int* const d_eptrc = (int*)(d_cam5 + 5 * (size_t)n_cams);
  int* const d_img = d_eptrc + NC1;
  int* const d_posei = d_img + R;
  int* const d_cami = d_posei + R;
  int* const d_cnt = d_cami + R;
  int* const d_cstart = d_cnt + M;
  int* const d_kend = d_cstart + NC1;  // (and cg behind it: mc_tail)
  std::vector<uint8_t> stage(up_bytes);
  {
    memcpy(stage.data(), h_cam5, 8 * 5 * (size_t)n_cams);
    int* p = (int*)(stage.data() + 8 * 5 * (size_t)n_cams);
    for (int c = 0; c <= n_clouds; c++) p[c] = h_eptr[c] * s.chunks;  // (<= M)
    memcpy(p + NC1, h_img, 4 * (size_t)R);
    memcpy(p + NC1 + R, h_pose, 4 * (size_t)R);
    memcpy(p + NC1 + 2 * (size_t)R, h_cam, 4 * (size_t)R);
  }
  hipError_t e = hipMemcpyAsync(d_cam5, stage.data(), up_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  auto fail_sync = [&](int code) {  // (`stage` goes away on return)
    hipStreamSynchronize(st);
    return code;
  };
  const DcItems it{d_img, d_posei, d_cami, d_cam5, d_depth, d_pose, pose_stride};
  k_dc_count<<<M, DC_T, 0, st>>>(it, s, d_cnt);
  mc_offsets(st, d_cnt, (long long)M, d_off, d_eptrc, n_clouds, d_cs64, d_cstart);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, (pre + "counts").c_str()));
  std::vector<long long> cs((size_t)NC1);
  e = hipMemcpyAsync(cs.data(), d_cs64, sizeof(long long) * NC1, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, (pre + "counts").c_str());
  if (timing) ctx->dc_ms[0] = ms_since(t0), ctx->dc_ms[1] = ctx->dc_ms[2] = ctx->dc_ms[3] = 0, t0 = std::chrono::steady_clock::now();
  if (h_n_valid)
    for (int c = 0; c < n_clouds; c++) h_n_valid[c] = cs[c + 1] - cs[c];
  if (cs[n_clouds] > (long long)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 valid samples or more");
  const int N = (int)cs[n_clouds];
  if (N == 0) return FLVIS_OK;
  McWork W;
  rc = mc_work(ctx, what, N, false, W);
  if (rc != FLVIS_OK) return rc;
  k_dc_keys<<<M, DC_T, 0, st>>>(it, s, d_cnt, d_off, leaf, W.keys[0], W.idx[0], W.pts, W.occ);
  e = hipGetLastError();
  if (e != hipSuccess) return ctx->hip_fail(e, (pre + "keys").c_str());
  if (timing) {
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, (pre + "keys").c_str());
    ctx->dc_ms[1] = ms_since(t0);
    W.ms_sort_rows = ctx->dc_ms + 2;
  }
  return mc_tail(ctx, what, W, N, n_clouds, d_cstart, d_kend, cs.data(), leaf, min_points, out_cap, d_xyz, d_npts, nullptr, h_n_out,
                 h_n_dropped, rows_bytes);
}

}  // namespace flvis

namespace {

// the listed images of flvis_hip_depth_cloud's ranges: image and pose row are one index, the camera is the range's
int dc_items_of_ranges(int n_clouds, const int* h_cloud_ptr, const int* h_range2, std::vector<int>& eptr, std::vector<int>& img,
                       std::vector<int>& cam) {
  long long R64 = 0;
  for (int r = 0; r < h_cloud_ptr[n_clouds]; r++) R64 += h_range2[2 * r + 1];
  if (R64 > INT_MAX) return FLVIS_ERR_CAPACITY;
  eptr.resize((size_t)n_clouds + 1);
  img.reserve((size_t)R64), cam.reserve((size_t)R64);
  for (int c = 0; c < n_clouds; c++) {
    eptr[c] = (int)img.size();
    for (int r = h_cloud_ptr[c]; r < h_cloud_ptr[c + 1]; r++)
      for (int k = 0; k < h_range2[2 * r + 1]; k++) img.push_back(h_range2[2 * r] + k), cam.push_back(r);
  }
  eptr[n_clouds] = (int)img.size();
  return FLVIS_OK;
}

int dc_check_public(int n_img, int w, int h, int n_clouds, const int* h_cloud_ptr, const int* h_range2, const double* h_cam5,
                    const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, std::string& why) {
  int rc = flvis_voxel_cloud_check(n_img, 1, n_clouds, h_cloud_ptr, h_range2, leaf, min_points, out_cap);
  if (rc != FLVIS_OK) return why = "the voxel call's check of the ranges, leaf, min_points and out_cap failed (flvis_voxel_cloud_check)", rc;
  if (!h_cam5) return why = "NULL cameras", FLVIS_ERR_INVALID_ARG;
  return dc_check_sampling(w, h, prm, h_cloud_ptr[n_clouds], h_cam5, &why);
}

// flvis_keyframe_log_depth_cloud: the refusals, then (unless check_only) the call
int kfl_depth_cloud(flvis_ctx* ctx, const char* what, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                    double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped,
                    int64_t* h_n_valid, bool check_only, const flvis_dense_stereo_params* sprm = nullptr, double stereo_df = 0,
                    bool unrect = false) {
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  Pipeline* pl = ctx->pipe;
  if (!pl) return bad("no tracker (flvis_tracker_create)");
  if (!sprm && pl->cfg.cam_type != CAM_DEPTH) return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's rig has no depth image");
  if (sprm && !unrect && pl->cfg.cam_type != CAM_STEREO_RECT)
    return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's rig is no rectified stereo pair (cam_type 0)");
  if (sprm && unrect && pl->cfg.cam_type != CAM_STEREO_UNRECT)
    return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's rig is no unrectified stereo pair (cam_type 1)");
  if (pl->kfl.cap <= 0) return bad("the keyframe log is off (flvis_keyframe_log_enable)");
  if (n <= 0 || !h_stream || !h_n_out || !prm) return bad("bad stream list, or a NULL prm or h_n_out");
  std::vector<double> cam5(5 * (size_t)n), cam2(2 * (size_t)n), cam21_0(unrect ? 21 * (size_t)n : 0), cam21_1(cam21_0.size());
  for (int c = 0; c < n; c++) {
    const int s = h_stream[c];
    if (s < 0 || s >= pl->S) return bad("stream out of range");
    if (h_slice2 && (h_slice2[2 * c] < 0 || h_slice2[2 * c + 1] < 0)) return bad("a negative slice");
    const flvis_cfg& g = pl->cfgs[s];  // (rig_from_cfg: the intrinsics the tracker itself back-projects with)
    const double v[5] = {g.P0[0], g.P0[5], g.P0[2], g.P0[6], sprm ? stereo_df : g.depth_factor};
    memcpy(&cam5[5 * (size_t)c], v, sizeof(v));
    cam2[2 * (size_t)c] = -g.P1[3], cam2[2 * (size_t)c + 1] = stereo_df;
    if (unrect) dc_unrect_cams(g, &cam21_0[21 * (size_t)c], &cam21_1[21 * (size_t)c]);
  }
  const DcUnrect un{n, cam21_0.data(), cam21_1.data()};
  std::string why;
  int rc = FLVIS_OK;
  if (unrect) rc = rc_check(n, pl->kfl.w, pl->kfl.h, n, cam21_0.data(), nullptr, &why);
  if (unrect && rc == FLVIS_OK) rc = rc_check(n, pl->kfl.w, pl->kfl.h, n, cam21_1.data(), nullptr, &why);
  for (int c = 0; sprm && rc == FLVIS_OK && c < n; c++) rc = ds_check(1, pl->kfl.w, pl->kfl.h, 1, &cam2[2 * (size_t)c], sprm, &why);
  if (rc == FLVIS_OK) rc = dc_check_sampling(pl->kfl.w, pl->kfl.h, prm, n, cam5.data(), &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  if (!(leaf >= 0) || !std::isfinite(leaf) || min_points < 1 || out_cap < 0 || (!d_xyz && out_cap > 0))
    return bad("leaf must be finite and >= 0, min_points >= 1, out_cap >= 0 with rows to write to");
  if (check_only) return FLVIS_OK;
  KfLogRec rec{};
  int S = 0, cam_type = 0;
  std::vector<long long> logged, dropped;
  rc = kf_log_settle(ctx, what, rec, S, cam_type, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  std::vector<int> eptr((size_t)n + 1), img, cam;
  for (int c = 0; c < n; c++) {
    const int s = h_stream[c];
    eptr[c] = (int)img.size();
    const long long first = h_slice2 ? h_slice2[2 * c] : 0, last = h_slice2 ? std::min(logged[s], first + h_slice2[2 * c + 1]) : logged[s];
    for (long long k = first; k < last; k++) {  // (logged <= cap, and streams * cap fits an int: flvis_keyframe_log_enable)
      if (img.size() >= (size_t)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 listed keyframes or more");
      img.push_back((int)((long long)s * rec.cap + k)), cam.push_back(c);
    }
  }
  eptr[n] = (int)img.size();
  static_assert(offsetof(KeyFrameDev, T_c_w) % 8 == 0 && sizeof(KeyFrameDev) % 8 == 0, "the logged poses are read in place as rows of doubles");
  const double* d_pose = reinterpret_cast<const double*>(reinterpret_cast<const char*>(rec.kf) + offsetof(KeyFrameDev, T_c_w));
  if (sprm) {
    const uint16_t* d_z = nullptr;
    std::vector<int> iota;
    rc = dc_stereo_samples(ctx, what, rec, img, cam, cam2.data(), sprm, prm, &d_z, iota, unrect ? &un : nullptr);
    if (rc != FLVIS_OK) return rc;
    return dc_cloud(ctx, what, d_z, rec.w, rec.h, d_pose, sizeof(KeyFrameDev) / 8, n, eptr.data(), iota.data(), img.data(), cam.data(), n,
                    cam5.data(), prm, leaf, min_points, out_cap, d_xyz, d_npts, h_n_out, h_n_dropped, h_n_valid, true);
  }
  return dc_cloud(ctx, what, reinterpret_cast<const uint16_t*>(rec.img1), rec.w, rec.h, d_pose, sizeof(KeyFrameDev) / 8, n, eptr.data(), img.data(),
                  img.data(), cam.data(), n, cam5.data(), prm, leaf, min_points, out_cap, d_xyz, d_npts, h_n_out, h_n_dropped, h_n_valid);
}

}  // namespace

extern "C" {

int flvis_depth_cloud_check(int n_img, int w, int h, int n_clouds, const int* h_cloud_ptr, const int* h_range2, const double* h_cam5,
                            const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap) {
  std::string why;
  return dc_check_public(n_img, w, h, n_clouds, h_cloud_ptr, h_range2, h_cam5, prm, leaf, min_points, out_cap, why);
}

int flvis_hip_depth_cloud(flvis_ctx* ctx, const uint16_t* d_depth, const double* d_T_c_w7, int n_img, int w, int h, int n_clouds,
                          const int* h_cloud_ptr, const int* h_range2, const double* h_cam5, const flvis_depth_cloud_params* prm, double leaf,
                          int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!d_depth || !d_T_c_w7 || !h_n_out || (!d_xyz && out_cap != 0)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "depth_cloud: a NULL required pointer");
  std::string why;
  int rc = dc_check_public(n_img, w, h, n_clouds, h_cloud_ptr, h_range2, h_cam5, prm, leaf, min_points, out_cap, why);
  if (rc != FLVIS_OK) return ctx->fail(rc, "depth_cloud: " + why);
  std::vector<int> eptr, img, cam;
  rc = dc_items_of_ranges(n_clouds, h_cloud_ptr, h_range2, eptr, img, cam);
  if (rc != FLVIS_OK) return ctx->fail(rc, "depth_cloud: the call lists 2^31 images or more");
  return flvis::dc_cloud(ctx, "depth_cloud", d_depth, w, h, d_T_c_w7, 7, n_clouds, eptr.data(), img.data(), img.data(), cam.data(),
                         h_cloud_ptr[n_clouds], h_cam5, prm, leaf, min_points, out_cap, d_xyz, d_npts, h_n_out, h_n_dropped, h_n_valid);
}

int flvis_hip_depth_cloud_times(flvis_ctx* ctx, int enable, double* h_ms4) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  ctx->dc_timing = enable != 0;
  if (h_ms4) memcpy(h_ms4, ctx->dc_ms, sizeof(ctx->dc_ms));
  return FLVIS_OK;
}

int flvis_keyframe_log_depth_cloud(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                                   double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out,
                                   int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  return kfl_depth_cloud(ctx, "keyframe_log_depth_cloud", n, h_stream, h_slice2, prm, leaf, min_points, out_cap, d_xyz, d_npts, h_n_out,
                         h_n_dropped, h_n_valid, false);
}

int flvis_keyframe_log_depth_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                                        double leaf, int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out,
                                        int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  const char* what = "keyframe_log_depth_cloud_host";
  // every refusal before anything is allocated (the host rows stand in for the device form's)
  int rc = kfl_depth_cloud(ctx, what, n, h_stream, h_slice2, prm, leaf, min_points, out_cap, h_xyz, nullptr, h_n_out, h_n_dropped, h_n_valid, true);
  if (rc != FLVIS_OK) return rc;
  float* d_xyz = nullptr;
  int* d_npts = nullptr;
  rc = flvis::mc_host_rows_alloc(ctx, what, n, out_cap, &d_xyz, &d_npts);
  if (rc != FLVIS_OK) return rc;
  rc = kfl_depth_cloud(ctx, what, n, h_stream, h_slice2, prm, leaf, min_points, out_cap, d_xyz, h_npts ? d_npts : nullptr, h_n_out, h_n_dropped,
                       h_n_valid, false);
  if (rc != FLVIS_OK) return rc;
  return flvis::mc_host_rows_fetch(ctx, what, n, out_cap, h_n_out, d_xyz, d_npts, h_xyz, h_npts);
}

}  // extern "C"

namespace {

// the stereo forms of the two cloud calls; unrect: the cam_type 1 forms (a rectification in front of the matcher)
int kfl_stereo_cloud(flvis_ctx* ctx, const char* what, bool unrect, int n, const int* h_stream, const int* h_slice2,
                     const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm, double leaf, int min_points,
                     int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!sprm) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": NULL stereo params");
  return kfl_depth_cloud(ctx, what, n, h_stream, h_slice2, prm, leaf, min_points, out_cap, d_xyz, d_npts, h_n_out, h_n_dropped, h_n_valid, false,
                         sprm, depth_factor, unrect);
}

int kfl_stereo_cloud_host(flvis_ctx* ctx, const char* what, bool unrect, int n, const int* h_stream, const int* h_slice2,
                          const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm, double leaf,
                          int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!sprm) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": NULL stereo params");
  int rc = kfl_depth_cloud(ctx, what, n, h_stream, h_slice2, prm, leaf, min_points, out_cap, h_xyz, nullptr, h_n_out, h_n_dropped, h_n_valid, true,
                           sprm, depth_factor, unrect);
  if (rc != FLVIS_OK) return rc;
  float* d_xyz = nullptr;
  int* d_npts = nullptr;
  rc = flvis::mc_host_rows_alloc(ctx, what, n, out_cap, &d_xyz, &d_npts);
  if (rc != FLVIS_OK) return rc;
  rc = kfl_depth_cloud(ctx, what, n, h_stream, h_slice2, prm, leaf, min_points, out_cap, d_xyz, h_npts ? d_npts : nullptr, h_n_out, h_n_dropped,
                       h_n_valid, false, sprm, depth_factor, unrect);
  if (rc != FLVIS_OK) return rc;
  return flvis::mc_host_rows_fetch(ctx, what, n, out_cap, h_n_out, d_xyz, d_npts, h_xyz, h_npts);
}

// the listed entries (h_stream[i], h_index[i]) of the settled log: their slots, and on the unrectified rig a camera per DISTINCT stream in
// order of first appearance (entries listed stream by stream then form long runs of one camera: rectify.hip)
struct KflEntries {
  KfLogRec rec{};
  std::vector<int> slot, cam;
  std::vector<double> cam21_0, cam21_1;
  int n_cams = 0;
};

int kfl_entries(flvis_ctx* ctx, const char* what, int n, const int* h_stream, const int* h_index, bool unrect, KflEntries& E) {
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  Pipeline* pl = ctx->pipe;
  E.cam.resize((size_t)n);
  if (unrect) {
    std::vector<int> cam_of_stream((size_t)pl->S, -1);
    for (int i = 0; i < n; i++) {
      int& c = cam_of_stream[h_stream[i]];
      if (c < 0) {
        c = E.n_cams++;
        E.cam21_0.resize(21 * (size_t)E.n_cams), E.cam21_1.resize(21 * (size_t)E.n_cams);
        dc_unrect_cams(pl->cfgs[h_stream[i]], &E.cam21_0[21 * (size_t)c], &E.cam21_1[21 * (size_t)c]);
      }
      E.cam[i] = c;
    }
    std::string why;
    int rc = rc_check(E.n_cams, pl->kfl.w, pl->kfl.h, E.n_cams, E.cam21_0.data(), nullptr, &why);
    if (rc == FLVIS_OK) rc = rc_check(E.n_cams, pl->kfl.w, pl->kfl.h, E.n_cams, E.cam21_1.data(), nullptr, &why);
    if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  }
  int S = 0, cam_type = 0;
  std::vector<long long> logged, dropped;
  int rc = kf_log_settle(ctx, what, E.rec, S, cam_type, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  E.slot.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    if (h_index[i] < 0 || h_index[i] >= logged[h_stream[i]]) return bad("an entry that is not logged");
    E.slot[i] = (int)((long long)h_stream[i] * E.rec.cap + h_index[i]);
  }
  return FLVIS_OK;
}

int kfl_stereo_z16(flvis_ctx* ctx, const char* what, bool unrect, int n, const int* h_stream, const int* h_index,
                   const flvis_dense_stereo_params* sprm, double depth_factor, uint16_t* d_z16) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  Pipeline* pl = ctx->pipe;
  if (!pl) return bad("no tracker (flvis_tracker_create)");
  if (!unrect && pl->cfg.cam_type != CAM_STEREO_RECT)
    return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's rig is no rectified stereo pair (cam_type 0)");
  if (unrect && pl->cfg.cam_type != CAM_STEREO_UNRECT)
    return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's rig is no unrectified stereo pair (cam_type 1)");
  if (pl->kfl.cap <= 0) return bad("the keyframe log is off (flvis_keyframe_log_enable)");
  if (n <= 0 || !h_stream || !h_index || !sprm || !d_z16) return bad("no entry, or a NULL h_stream, h_index, prm or d_z16");
  std::vector<double> cam2(2 * (size_t)n);
  std::string why;
  for (int i = 0; i < n; i++) {
    const int s = h_stream[i];
    if (s < 0 || s >= pl->S) return bad("stream out of range");
    cam2[2 * (size_t)i] = -pl->cfgs[s].P1[3], cam2[2 * (size_t)i + 1] = depth_factor;
    const int rc = ds_check(1, pl->kfl.w, pl->kfl.h, 1, &cam2[2 * (size_t)i], sprm, &why);
    if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  }
  KflEntries E;
  int rc = kfl_entries(ctx, what, n, h_stream, h_index, unrect, E);
  if (rc != FLVIS_OK) return rc;
  const KfLogRec& rec = E.rec;
  if (unrect) {
    const DcUnrect un{E.n_cams, E.cam21_0.data(), E.cam21_1.data()};
    return dc_unrect_match(ctx, what, rec, E.slot.data(), E.cam.data(), n, un, cam2.data(), sprm, d_z16, nullptr);
  }
  return ds_run(ctx, what, rec.img0, rec.img1, n, rec.w, rec.h, n, cam2.data(), sprm, nullptr, d_z16, E.slot.data(), nullptr);
}

}  // namespace

extern "C" {

int flvis_keyframe_log_stereo_cloud(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_dense_stereo_params* sprm,
                                    double depth_factor, const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap,
                                    float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  return kfl_stereo_cloud(ctx, "keyframe_log_stereo_cloud", false, n, h_stream, h_slice2, sprm, depth_factor, prm, leaf, min_points, out_cap, d_xyz,
                          d_npts, h_n_out, h_n_dropped, h_n_valid);
}

int flvis_keyframe_log_stereo_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_dense_stereo_params* sprm,
                                         double depth_factor, const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap,
                                         float* h_xyz, int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  return kfl_stereo_cloud_host(ctx, "keyframe_log_stereo_cloud_host", false, n, h_stream, h_slice2, sprm, depth_factor, prm, leaf, min_points,
                               out_cap, h_xyz, h_npts, h_n_out, h_n_dropped, h_n_valid);
}

int flvis_keyframe_log_stereo_z16(flvis_ctx* ctx, int n, const int* h_stream, const int* h_index, const flvis_dense_stereo_params* sprm,
                                  double depth_factor, uint16_t* d_z16) {
  return kfl_stereo_z16(ctx, "keyframe_log_stereo_z16", false, n, h_stream, h_index, sprm, depth_factor, d_z16);
}

int flvis_keyframe_log_unrect_stereo_cloud(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_dense_stereo_params* sprm,
                                           double depth_factor, const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap,
                                           float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  return kfl_stereo_cloud(ctx, "keyframe_log_unrect_stereo_cloud", true, n, h_stream, h_slice2, sprm, depth_factor, prm, leaf, min_points, out_cap,
                          d_xyz, d_npts, h_n_out, h_n_dropped, h_n_valid);
}

int flvis_keyframe_log_unrect_stereo_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2,
                                                const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm,
                                                double leaf, int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out,
                                                int64_t* h_n_dropped, int64_t* h_n_valid) {
  return kfl_stereo_cloud_host(ctx, "keyframe_log_unrect_stereo_cloud_host", true, n, h_stream, h_slice2, sprm, depth_factor, prm, leaf,
                               min_points, out_cap, h_xyz, h_npts, h_n_out, h_n_dropped, h_n_valid);
}

int flvis_keyframe_log_unrect_stereo_z16(flvis_ctx* ctx, int n, const int* h_stream, const int* h_index, const flvis_dense_stereo_params* sprm,
                                         double depth_factor, uint16_t* d_z16) {
  return kfl_stereo_z16(ctx, "keyframe_log_unrect_stereo_z16", true, n, h_stream, h_index, sprm, depth_factor, d_z16);
}

int flvis_keyframe_log_rectified_pair(flvis_ctx* ctx, int n, const int* h_stream, const int* h_index, uint8_t* d_img0, uint8_t* d_img1) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  const char* what = "keyframe_log_rectified_pair";
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  Pipeline* pl = ctx->pipe;
  if (!pl) return bad("no tracker (flvis_tracker_create)");
  if (pl->cfg.cam_type != CAM_STEREO_UNRECT) return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's rig is no unrectified stereo pair (cam_type 1)");
  if (pl->kfl.cap <= 0) return bad("the keyframe log is off (flvis_keyframe_log_enable)");
  if (n <= 0 || !h_stream || !h_index || (!d_img0 && !d_img1)) return bad("no entry, a NULL h_stream or h_index, or both outputs NULL");
  for (int i = 0; i < n; i++)
    if (h_stream[i] < 0 || h_stream[i] >= pl->S) return bad("stream out of range");
  KflEntries E;
  int rc = kfl_entries(ctx, what, n, h_stream, h_index, true, E);
  if (rc != FLVIS_OK) return rc;
  const DcUnrect un{E.n_cams, E.cam21_0.data(), E.cam21_1.data()};
  return dc_rectify_batch(ctx, what, E.rec, E.slot.data(), E.cam.data(), n, un, d_img0, d_img1);
}

}  // extern "C"
