// flvis_amd: LKORBTracking::tracking (src/processing/lkorb_tracking.cpp:9-202) in ONE call on caller arrays, batched over n_sets independent
// frames, for the three camera types -- flvis_hip_lkorb_tracking.  The batched tracker's own path (track_prepare_dev, track_collect_dev,
// k_ransac_f_body, pnp_ransac_core and the tail of k_ransac_pnp_body, track_kernels.hip) lifted to the kernel-level boundary; nothing runs
// on the host between the optical flow and the pose:
//   k_trk_seeds         the tracker's initial guesses: the pixel itself, cv::projectPoints(K0, D0) with the guess (stereo rigs) or camera2pixel
//                       of the float-narrowed landmark (depth camera); use_guess is per set
//   launch_lk_track     cv::calcOpticalFlowPyrLK(31 x 31, maxLevel 10, 30 / 0.001, OPTFLOW_USE_INITIAL_FLOW)
//   k_trk_collect_sets  the survivors: `to` in descending index order (quirk A1), m1 / m2 ascending, undistortPoints on the unrectified rig
//   launch_fund_ransac_sets   cv::findFundamentalMat(FM_RANSAC, 5.0, 0.99) on the scratch rows (the tracker's search)
//   k_trk_after_f       the mirrored mask, F_inlier_cnt, the (has_3d && is_tracking_inlier) pairs in `to` order
//   launch_pnp_ransac_sets    cv::solvePnPRansac(100, 3.0, 0.99), once per branch (P3P without a guess, ITERATIVE with one) on that
//                       branch's contiguous scratch rows: the host groups the sets by branch before anything is launched
//   k_trk_finish        CameraFrame::updateLMState, the pose, pnp_inlier_cnt and the return value -- of the sets that reached the PnP
// A set that leaves early (fewer than 10 survivors / flags) hands count 0 to the later stages, which then write scratch alone: its outputs stay
// as the stage it reached wrote them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "dev_common.hpp"
#include "dev_geom.hpp"
#include "dev_math.hpp"
#include "track_kernels.hpp"

namespace flvis {

struct TrkCam {
  double K0[4], D0[4], R0[9], P0[12];
  double fx, fy, cx, cy;  // rectified (from P0): the K of camera2pixel and of solvePnPRansac
  int cam_type, w, h, pad;
};

FD int trk_count(const int* count, int s, int cap) {
  const int n = count[s];
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// one thread per landmark, blockIdx.y the set (track_prepare_dev on caller arrays)
__global__ __launch_bounds__(256) void k_trk_seeds(TrkCam cam, const float* __restrict__ from_plane, const float* __restrict__ from_3d_w,
                                                   const int* __restrict__ count, int cap, const double* __restrict__ guess7,
                                                   const uint8_t* __restrict__ use_guess, float* __restrict__ seeds) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= trk_count(count, s, cap)) return;
  const size_t k = (size_t)s * cap + i;
  float* np = seeds + 2 * k;
  if (use_guess[s]) {
    const SE3d g = load_pose7(guess7 + 7 * (size_t)s);
    const float p3[3] = {from_3d_w[3 * k], from_3d_w[3 * k + 1], from_3d_w[3 * k + 2]};
    if (cam.cam_type == CAM_DEPTH) {  // lkorb_tracking.cpp:41-52: pinhole projection of the float-narrowed landmark
      const V3 pc = se3_act(g, V3{(double)p3[0], (double)p3[1], (double)p3[2]});
      np[0] = (float)(cam.fx * pc.x / pc.z + cam.cx);
      np[1] = (float)(cam.fy * pc.y / pc.z + cam.cy);
    } else {
      project_point(p3, q_to_mat(g.q), g.t, cam.K0, cam.D0, np);
    }
  } else {
    np[0] = from_plane[2 * k];
    np[1] = from_plane[2 * k + 1];
  }
}

// lkorb_tracking.cpp:76-125, track_collect_dev's scheme on caller arrays: one workgroup per set, every wave takes chunks of 64 landmarks
// (the loops' bounds are wave-uniform: every lane of a wave reaches the ballots), the chunks' survivor counts meet in LDS.
constexpr int TC_T = 256;
constexpr int TRK_NCH = NMAX / 64;
__global__ __launch_bounds__(TC_T) void k_trk_collect_sets(TrkCam cam, const float* __restrict__ from_plane, const float* __restrict__ from_und,
                                                           const uint8_t* __restrict__ from_flags, const int* __restrict__ count, int cap,
                                                           const float* __restrict__ tracked, const uint8_t* __restrict__ status,
                                                           int* __restrict__ to_from, float* __restrict__ to_plane, float* __restrict__ to_und,
                                                           uint8_t* __restrict__ to_flags, float* __restrict__ m1, float* __restrict__ m2,
                                                           int* __restrict__ f_count, int* __restrict__ counts4, uint8_t* __restrict__ ret) {
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  __shared__ int s_cnt[TRK_NCH];
  const int n = trk_count(count, s, cap);
  const size_t row = (size_t)s * cap;
  const float* const tr = tracked + row * 2;
  const uint8_t* const stt = status + row;
  const int w = cam.w - 1, h = cam.h - 1;
  const int nch = (n + 63) / 64;  // <= TRK_NCH: cap <= NMAX is the caller's check
  for (int c = wv; c < TRK_NCH; c += TC_T / 64) {
    const int i = 64 * c + lane;
    const bool pass = i < n && stt[i] == 1 && tr[2 * i] > 0 && tr[2 * i + 1] > 0 && tr[2 * i] < (float)w && tr[2 * i + 1] < (float)h;
    const int cnt = __popcll(__ballot(pass));
    if (lane == 0) s_cnt[c] = cnt;
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int c = 0; c < TRK_NCH; c++) total += s_cnt[c];
  for (int c = wv; c < nch; c += TC_T / 64) {
    int before = 0;  // survivors with a smaller index than this chunk's
    for (int k = 0; k < c; k++) before += s_cnt[k];
    const int i = 64 * c + lane;
    const bool pass = i < n && stt[i] == 1 && tr[2 * i] > 0 && tr[2 * i + 1] > 0 && tr[2 * i] < (float)w && tr[2 * i + 1] < (float)h;
    const unsigned long long b = __ballot(pass);
    if (pass) {
      const int k = before + lane_prefix(b);  // ascending rank
      const int j = total - 1 - k;            // position in to.landmarks (descending)
      const float tx = tr[2 * i], ty = tr[2 * i + 1];
      float und[2] = {tx, ty};
      float fu[2];
      if (cam.cam_type != CAM_STEREO_UNRECT) {  // STEREO_RECT and DEPTH_D435 (lkorb_tracking.cpp:76-85)
        fu[0] = from_plane[(row + i) * 2];
        fu[1] = from_plane[(row + i) * 2 + 1];
      } else {
        const float src[2] = {tx, ty};
        undistort_point(src, cam.K0, cam.D0, cam.R0, cam.P0, und);
        fu[0] = from_und[(row + i) * 2];
        fu[1] = from_und[(row + i) * 2 + 1];
      }
      to_from[row + j] = i;
      to_plane[(row + j) * 2] = tx;
      to_plane[(row + j) * 2 + 1] = ty;
      to_und[(row + j) * 2] = und[0];
      to_und[(row + j) * 2 + 1] = und[1];
      to_flags[row + j] = from_flags[row + i];
      m1[(row + k) * 2] = fu[0];
      m1[(row + k) * 2 + 1] = fu[1];
      m2[(row + k) * 2] = und[0];
      m2[(row + k) * 2 + 1] = und[1];
    }
  }
  if (tid == 0) {
    counts4[4 * s] = total;
    counts4[4 * s + 1] = 0;
    counts4[4 * s + 2] = 0;
    counts4[4 * s + 3] = 0;
    ret[s] = 0;
    f_count[s] = total < 10 ? 0 : total;  // (a set that fails here never reaches the F search)
  }
}

// lkorb_tracking.cpp:136-168: one wave per set.  mask[i] == 0 clears the flag of to.landmarks[i] -- the mirrored index (quirk A1), kept; then the
// pairs of the PnP in `to` order into the set's scratch row `slot[s]` (its place among the sets of its PnP branch), with each pair's row in `to`.
__global__ __launch_bounds__(64) void k_trk_after_f(const int* __restrict__ f_count, const uint8_t* __restrict__ mask_f, int cap,
                                                    const int* __restrict__ to_from, const float* __restrict__ to_und,
                                                    const float* __restrict__ from_3d_w, uint8_t* __restrict__ to_flags,
                                                    const int* __restrict__ slot, float* __restrict__ p3d, float* __restrict__ p2d,
                                                    int* __restrict__ pnp_row, int* __restrict__ pnp_count, int* __restrict__ stage,
                                                    int* __restrict__ counts4) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int m = f_count[s];
  const size_t row = (size_t)s * cap, prow = (size_t)slot[s] * cap;
  int fc = 0, np = 0;
  for (int base = 0; base < m; base += 64) {
    const int i = base + lane;
    uint8_t fl = 0;
    if (i < m) {
      fl = to_flags[row + i];
      if (mask_f[row + i] == 0 && (fl & 2)) {
        fl &= (uint8_t)~2;
        to_flags[row + i] = fl;
      }
    }
    const bool inl = (fl & 2) != 0, sel = (fl & 3) == 3;
    fc += __popcll(__ballot(inl));
    const unsigned long long b = __ballot(sel);
    if (sel) {
      const size_t k = prow + np + lane_prefix(b);
      const size_t f = row + to_from[row + i];
      p2d[2 * k] = to_und[(row + i) * 2];
      p2d[2 * k + 1] = to_und[(row + i) * 2 + 1];
      p3d[3 * k] = from_3d_w[3 * f];
      p3d[3 * k + 1] = from_3d_w[3 * f + 1];
      p3d[3 * k + 2] = from_3d_w[3 * f + 2];
      pnp_row[k] = i;
    }
    np += __popcll(b);
  }
  if (lane == 0) {
    const bool go = m > 0 && fc >= 10;
    if (m > 0) counts4[4 * s + 1] = fc;
    if (go) counts4[4 * s + 2] = np;
    pnp_count[slot[s]] = go ? np : 0;  // (a set that ended hands the PnP nothing)
    stage[s] = go ? 1 : 0;
  }
}

// lkorb_tracking.cpp:170-201 behind the solver: CameraFrame::updateLMState, the pose, the count and the return value; one wave per set, and only
// the sets that reached the PnP
__global__ __launch_bounds__(64) void k_trk_finish(const int* __restrict__ stage, const int* __restrict__ slot, int cap,
                                                   const int* __restrict__ pnp_count, const int* __restrict__ pnp_row,
                                                   const uint8_t* __restrict__ pnp_mask, const double* __restrict__ pnp_pose7,
                                                   const int* __restrict__ pnp_inl, uint8_t* __restrict__ to_flags, int* __restrict__ counts4,
                                                   double* __restrict__ pose7, uint8_t* __restrict__ ret) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (!stage[s]) return;
  const int q = slot[s];
  const size_t row = (size_t)s * cap, prow = (size_t)q * cap;
  const int np = pnp_count[q];
  for (int i = lane; i < np; i += 64)
    if (pnp_mask[prow + i] == 0) to_flags[row + pnp_row[prow + i]] &= (uint8_t)~2;
  if (lane < 7) pose7[7 * (size_t)s + lane] = pnp_pose7[7 * (size_t)q + lane];
  if (lane == 0) {
    const int inl = pnp_inl[q];
    counts4[4 * s + 3] = inl;
    ret[s] = inl >= 10 ? 1 : 0;
  }
}

}  // namespace flvis

using namespace flvis;

extern "C" int flvis_hip_lkorb_tracking(flvis_ctx* ctx, const flvis_cfg* cfg, const uint8_t* d_img_from, const uint8_t* d_img_to, int n_sets,
                                        const float* d_from_2d_plane, const float* d_from_2d_undistort, const float* d_from_3d_w,
                                        const uint8_t* d_from_flags, const int* d_count, int cap, const double* h_guess7,
                                        const uint8_t* h_use_guess, int* d_to_from, float* d_to_2d_plane, float* d_to_2d_undistort,
                                        uint8_t* d_to_flags, uint8_t* d_mask_F, int* d_counts4, double* d_pose7, uint8_t* d_ret) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!cfg || !d_img_from || !d_img_to || !d_from_2d_plane || !d_from_2d_undistort || !d_from_3d_w || !d_from_flags || !d_count ||
      !d_to_from || !d_to_2d_plane || !d_to_2d_undistort || !d_to_flags || !d_counts4 || !d_pose7 || !d_ret || n_sets <= 0 || cap <= 0 ||
      n_sets > 65535)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "lkorb_tracking: bad args (null pointer, cap <= 0, n_sets outside 1 .. 65535)");
  int n_iter = 0;
  if (h_use_guess)
    for (int s = 0; s < n_sets; s++) n_iter += h_use_guess[s] ? 1 : 0;
  if (n_iter && !h_guess7) return ctx->fail(FLVIS_ERR_INVALID_ARG, "lkorb_tracking: use_guess is set and h_guess7 is null");
  if (cap > fund_ransac_max_points() || cap > pnp_ransac_max_points())
    return ctx->fail(FLVIS_ERR_CAPACITY, "lkorb_tracking: cap > 1024 (the F-matrix candidate tables and the PnP's LDS staging hold 1024 points)");
  const int w = cfg->image_width, h = cfg->image_height;
  if (w < 32 || h < 32) return ctx->fail(FLVIS_ERR_CONFIG, "lkorb_tracking: image below 32 x 32");
  if (cfg->cam_type < CAM_STEREO_RECT || cfg->cam_type > CAM_DEPTH || cfg->P0[0] == 0.0 || cfg->P0[5] == 0.0)
    return ctx->fail(FLVIS_ERR_CONFIG, "lkorb_tracking: the configuration is not finalised (flvis_config_finalize: cam_type / P0 are empty)");
  hipSetDevice(ctx->device);
  TrkCam cam;
  memset(&cam, 0, sizeof(cam));
  {
    RigParams rg;
    rig_from_cfg(*cfg, rg);  // (the tracker's own rig: the same constants reach the same device functions)
    memcpy(cam.K0, rg.K0, 32);
    memcpy(cam.D0, rg.D0, 32);
    memcpy(cam.R0, rg.R0, 72);
    memcpy(cam.P0, rg.P0, 96);
    cam.fx = rg.fx, cam.fy = rg.fy, cam.cx = rg.cx, cam.cy = rg.cy;
    cam.cam_type = cfg->cam_type, cam.w = w, cam.h = h;
  }
  // the sets grouped by PnP branch: slot[s] = set s's scratch row, the P3P sets (no guess) first, then the ITERATIVE ones, each in set order
  const int n_p3p = n_sets - n_iter;
  const size_t N = (size_t)n_sets, NC = N * cap;
  // one host block, one upload: guess by set [N][7] | guess by slot [N][7] | seeds [N] (u64, zero: cv::RNG((uint64)-1) per call) | slot [N] | use_guess [N]
  std::vector<double> hb(7 * N + 7 * N + N + (N + 1) / 2 + (N + 7) / 8, 0.0);
  double* const h_g_set = hb.data();
  double* const h_g_slot = h_g_set + 7 * N;
  int* const h_slot = (int*)(h_g_slot + 7 * N + N);
  uint8_t* const h_ug = (uint8_t*)((double*)h_slot + (N + 1) / 2);
  {
    int a = 0, b = n_p3p;
    for (int s = 0; s < n_sets; s++) {
      const bool ug = h_use_guess && h_use_guess[s];
      const int q = ug ? b++ : a++;
      h_slot[s] = q;
      h_ug[s] = ug ? 1 : 0;
      double* const g = h_g_set + 7 * (size_t)s;
      if (h_guess7) memcpy(g, h_guess7 + 7 * (size_t)s, 56);
      else g[6] = 1.0;
      memcpy(h_g_slot + 7 * (size_t)q, g, 56);
    }
  }
  double* const d_hb = (double*)ctx->scratch("trk_host", sizeof(double) * hb.size());
  float* const seeds = (float*)ctx->scratch("trk_seeds", sizeof(float) * 2 * NC);
  uint8_t* const status = (uint8_t*)ctx->scratch("trk_status", NC);
  float* const m12 = (float*)ctx->scratch("trk_m12", sizeof(float) * 4 * NC);
  uint8_t* const mask_f = d_mask_F ? d_mask_F : (uint8_t*)ctx->scratch("trk_mask_f", NC);
  float* const p32 = (float*)ctx->scratch("trk_pnp_pts", sizeof(float) * 5 * NC);
  int* const pnp_row = (int*)ctx->scratch("trk_pnp_row", sizeof(int) * NC);
  uint8_t* const pnp_mask = (uint8_t*)ctx->scratch("trk_pnp_mask", NC);
  double* const pnp_pose = (double*)ctx->scratch("trk_pnp_pose", sizeof(double) * 7 * N);
  int* const ints = (int*)ctx->scratch("trk_ints", sizeof(int) * 5 * N);  // f_count | f_inl | pnp_count | pnp_inl | stage
  if (!d_hb || !seeds || !status || !m12 || !mask_f || !p32 || !pnp_row || !pnp_mask || !pnp_pose || !ints)
    return ctx->fail(FLVIS_ERR_HIP, "lkorb_tracking: scratch allocation failed");
  int L = lk_pyr_levels(w, h, 31, 10);
  if (L >= LK_MAX_LEVELS) L = LK_MAX_LEVELS - 1;
  PyrSel pp, pn;
  int rc = build_pyramid(ctx, "lk_pyr_prev", d_img_from, w, h, n_sets, L, pp);
  if (rc) return rc;
  rc = build_pyramid(ctx, "lk_pyr_next", d_img_to, w, h, n_sets, L, pn);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(d_hb, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (hb is a local; the caller's arrays may be freed when the call returns)
  if (e != hipSuccess) return ctx->hip_fail(e, "lkorb_tracking upload");
  const double* const g_set = d_hb;
  const double* const g_slot = d_hb + 7 * N;
  const unsigned long long* const rng0 = (const unsigned long long*)(g_slot + 7 * N);
  const int* const slot = (const int*)(rng0 + N);
  const uint8_t* const ug = (const uint8_t*)((const double*)slot + (N + 1) / 2);
  float* const m1 = m12;
  float* const m2 = m12 + 2 * NC;
  float* const p3d = p32;
  float* const p2d = p32 + 3 * NC;
  int* const f_count = ints;
  int* const f_inl = ints + N;
  int* const pnp_count = ints + 2 * N;
  int* const pnp_inl = ints + 3 * N;
  int* const stage = ints + 4 * N;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_trk_seeds, dim3((cap + 255) / 256, n_sets), dim3(256), 0, st, cam, d_from_2d_plane, d_from_3d_w, d_count, cap, g_set, ug,
                     seeds);
  LKParams prm;
  prm.max_iter = 30;
  prm.eps2 = 1e-3 * 1e-3;
  prm.min_eig = 1e-4f;
  prm.use_initial = 1;
  launch_lk_track(st, pp, pn, d_from_2d_plane, seeds, status, d_count, cap, n_sets, prm, nullptr);
  hipLaunchKernelGGL(k_trk_collect_sets, dim3(n_sets), dim3(TC_T), 0, st, cam, d_from_2d_plane, d_from_2d_undistort, d_from_flags, d_count, cap,
                     seeds, status, d_to_from, d_to_2d_plane, d_to_2d_undistort, d_to_flags, m1, m2, f_count, d_counts4, d_ret);
  launch_fund_ransac_sets(st, m1, m2, f_count, cap, n_sets, 5.0, 0.99, mask_f, f_inl);
  hipLaunchKernelGGL(k_trk_after_f, dim3(n_sets), dim3(64), 0, st, f_count, mask_f, cap, d_to_from, d_to_2d_undistort, d_from_3d_w, d_to_flags,
                     slot, p3d, p2d, pnp_row, pnp_count, stage, d_counts4);
  const double K4[4] = {cam.fx, cam.fy, cam.cx, cam.cy};
  for (int br = 0; br < 2; br++) {  // P3P on the rows [0, n_p3p), ITERATIVE from the guess on [n_p3p, n_sets)
    const size_t o = br ? (size_t)n_p3p : 0;
    const int nb = br ? n_iter : n_p3p;
    if (!nb) continue;
    launch_pnp_ransac_sets(st, p3d + 3 * o * cap, p2d + 2 * o * cap, pnp_count + o, cap, nb, K4, nullptr, 0, nullptr, br, g_slot + 7 * o, rng0 + o,
                           100, 3.0, 0.99, pnp_pose + 7 * o, pnp_mask + o * cap, pnp_inl + o);
  }
  hipLaunchKernelGGL(k_trk_finish, dim3(n_sets), dim3(64), 0, st, stage, slot, cap, pnp_count, pnp_row, pnp_mask, pnp_pose, pnp_inl, d_to_flags,
                     d_counts4, d_pose7, d_ret);
  e = hipGetLastError();
  if (e != hipSuccess) return ctx->hip_fail(e, "lkorb_tracking");
  return FLVIS_OK;
}
