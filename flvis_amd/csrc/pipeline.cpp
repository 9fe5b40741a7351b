// flvis_amd: host orchestration of the batched front-end + local map behind the C ABI (include/flvis_hip.h).
// Host-side mirror of the reference's F2FTracking / TrackingNodeletClass::process / LocalMapNodeletClass call sequence
// (src/frontend/f2f_tracking.cpp:59-400, src/frontend/vo_tracking.cpp:326-371,396-430, src/backend/vo_localmap.cpp:87-380):
// the host only stages the per-frame inputs and enqueues a FIXED kernel sequence per frame; every decision the reference
// takes per frame is taken on the device by the kernels in track_kernels.hip / ba_solve.hip.
//
// Lanes.  The per-frame chain of a stream is a recurrence of ~15 dependent kernels, most of them one workgroup per stream
// (geometry on <= 240 landmarks): with all S streams of a tracker in ONE chain those kernels occupy S of the 256 CUs while
// everything waits for them, and only the image kernels (LK, pyramids, corner response) fill the chip.  A tracker
// therefore splits its streams into LANES (sub-batches): every lane owns its streams' state, its own HIP streams (tracking
// chain + corner detection) and runs the same fixed sequence on its slice of the batch, so the LK of one lane overlaps the
// geometry chain of the others.  Streams never interact, so the partition changes no result.  The
// local-map workers of all lanes share two low-priority HIP streams (the number of hardware queues is limited: streams
// beyond it share a queue and serialise behind each other's long kernels).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <limits>
#include <vector>

#include "pipeline_host.hpp"

using namespace flvis;

static const char* kStageNames[PROF_STAGES] = {
    "imu_feed+frame_begin", "ingest(equalize)", "pyr_down(left)", "track_prepare", "lk_track(temporal)", "track_collect",
    "ransac_f", "ransac_pnp", "track_post+pose_lm", "reproj_filter", "gftt:eig_cand", "gftt:(merged)", "gftt:pick",
    "feature_dem+add_new", "depth_prepare", "lk_track(stereo)", "depth_innovate", "frame_end",
    "ba_worker(launch)", "frame(chain)"};

namespace {

int lk_levels(int w, int h, int win, int max_level) {
  int level = 0;
  for (; level <= max_level; ++level) {
    w = (w + 1) / 2;
    h = (h + 1) / 2;
    if (w <= win || h <= win) return level;
  }
  return max_level;
}

}  // namespace
namespace flvis {
// SE3 from a row-major 4x4 as Sophus builds it (SO3(Matrix3d): Eigen's matrix -> quaternion, no normalisation) and, with
// `inverse`, Sophus' SE3::inverse() (se3.cpp:76-83): q^-1 = normalised conjugate, t^-1 = q^-1 * (-t) by the quaternion
// rotation formula -- the same operations in the same order as the CPU restatement, so that T_c_i / T_c1_c0 are bit-identical
// on both sides for a general extrinsic rotation (EuRoC), not only for an axis permutation (D435).
void pose7_from_mat44(const double* m, double* out7, bool inverse) {
  const double R[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
  double t[3] = {m[3], m[7], m[11]};
  double q[4];  // w x y z
  double tr = R[0][0] + R[1][1] + R[2][2];
  if (tr > 0) {
    double s = std::sqrt(tr + 1.0);
    q[0] = 0.5 * s;
    s = 0.5 / s;
    q[1] = (R[2][1] - R[1][2]) * s;
    q[2] = (R[0][2] - R[2][0]) * s;
    q[3] = (R[1][0] - R[0][1]) * s;
  } else {
    int i = 0;
    if (R[1][1] > R[0][0]) i = 1;
    if (R[2][2] > R[i][i]) i = 2;
    int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
    double v[3];
    v[i] = 0.5 * s;
    s = 0.5 / s;
    q[0] = (R[k][j] - R[j][k]) * s;
    v[j] = (R[j][i] + R[i][j]) * s;
    v[k] = (R[k][i] + R[i][k]) * s;
    q[1] = v[0];
    q[2] = v[1];
    q[3] = v[2];
  }
  if (inverse) {
    const double cw = q[0], cx = -q[1], cy = -q[2], cz = -q[3];
    const double n = std::sqrt(cw * cw + cx * cx + cy * cy + cz * cz);
    q[0] = cw / n;
    q[1] = cx / n;
    q[2] = cy / n;
    q[3] = cz / n;
    // quat_rotate(q, -t): uv = cross(qv, v); uv += uv; v + w * uv + cross(qv, uv)
    const double v[3] = {-1.0 * t[0], -1.0 * t[1], -1.0 * t[2]};
    double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double c2[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
    for (int k = 0; k < 3; k++) t[k] = (v[k] + q[0] * uv[k]) + c2[k];
  }
  out7[0] = t[0];
  out7[1] = t[1];
  out7[2] = t[2];
  out7[3] = q[1];
  out7[4] = q[2];
  out7[5] = q[3];
  out7[6] = q[0];
}

// the per-stream part of a finalized config (RigParams): the one place a rig is made, for tracker creation and flvis_reset_streams_rigs
void rig_from_cfg(const flvis_cfg& cfg, RigParams& r) {
  memset(&r, 0, sizeof(r));
  r.fx = cfg.P0[0];
  r.fy = cfg.P0[5];
  r.cx = cfg.P0[2];
  r.cy = cfg.P0[6];
  memcpy(r.K0, cfg.cam0_intrinsics, 32);
  memcpy(r.D0, cfg.cam0_distortion, 32);
  memcpy(r.K1, cfg.cam1_intrinsics, 32);
  memcpy(r.D1, cfg.cam1_distortion, 32);
  memcpy(r.R0, cfg.R0, 72);
  memcpy(r.R1, cfg.R1, 72);
  memcpy(r.P0, cfg.P0, 96);
  memcpy(r.P1, cfg.P1, 96);
  pose7_from_mat44(cfg.T_cam0_cam1, r.T_c1_c0, true);
  pose7_from_mat44(cfg.T_imu_cam0, r.T_i_c, false);
  pose7_from_mat44(cfg.T_imu_cam0, r.T_c_i, true);
  r.iir_ratio = (float)cfg.dr_para[0];
  r.range = (float)cfg.dr_para[1];
  r.depth_scale = cfg.depth_factor;
  r.enable_dummy = !(cfg.dr_para[2] < 0.5);
  for (int i = 0; i < 4; i++) r.vi_para[i] = cfg.vifusion_para[i];
}

}  // namespace flvis
namespace {
}  // namespace


static void lane_destroy(Lane* L) {
  if (!L) return;
  if (L->st) hipStreamSynchronize(L->st);
  if (L->det_stream) {
    hipStreamSynchronize(L->det_stream);
    hipStreamDestroy(L->det_stream);
  }
  if (L->own_st && L->st) hipStreamDestroy(L->st);
  for (Join& j : L->join)
    if (j.ev) hipEventDestroy(j.ev);
  if (L->ev_stagger) hipEventDestroy(L->ev_stagger);
  for (hipEvent_t e : L->ev_end)
    if (e) hipEventDestroy(e);
  for (void* p : L->allocs) hipFree(p);
  for (hipEvent_t e : L->prof_ev) hipEventDestroy(e);
  for (int k = 0; k < Lane::PIN_RING; k++)
    if (L->pinned[k]) hipHostFree(L->pinned[k]);
  if (L->h_progress) hipHostFree((void*)L->h_progress);
  delete L;
}

extern "C" void flvis_pipeline_sync_internal(flvis_ctx* ctx) {
  if (ctx && ctx->pipe) sync_all(ctx);
}

// the sequence number a timed-out join stored (k_wait_flag's err_word = word 2 of the lane's host-mapped progress block), or 0; cleared when read
extern "C" long long flvis_pipeline_join_timeout_internal(flvis_ctx* ctx) {
  long long seq = 0;
  if (ctx && ctx->pipe)
    for (Lane* L : ctx->pipe->lanes)
      if (L->h_progress && L->h_progress[2]) {
        seq = L->h_progress[2];
        L->h_progress[2] = 0;
      }
  return seq;
}

// the stream (context-wide index) + 1 whose reset command met a full keyframe queue (word 3 of a lane's host-mapped block), or 0; cleared when read
extern "C" int flvis_pipeline_reset_overflow_internal(flvis_ctx* ctx) {
  int s = 0;
  if (ctx && ctx->pipe)
    for (Lane* L : ctx->pipe->lanes)
      if (L->h_progress && L->h_progress[3]) {
        s = L->s0 + (int)L->h_progress[3];
        L->h_progress[3] = 0;
      }
  return s;
}

// a local-map window that exceeded a capacity (word 4 of a lane's host-mapped block): BA_OVF_* bits << 32 | context-wide stream + 1, or 0;
// cleared when read
extern "C" long long flvis_pipeline_ba_overflow_internal(flvis_ctx* ctx) {
  long long v = 0;
  if (ctx && ctx->pipe)
    for (Lane* L : ctx->pipe->lanes)
      if (L->h_progress && L->h_progress[4]) {
        const long long w = L->h_progress[4];
        v = (w & ~0xffffffffll) | (long long)(L->s0 + (int)(w & 0xffffffffll));
        L->h_progress[4] = 0;
      }
  return v;
}

static void lm_cloud_free(Pipeline* pl) {
  if (pl->lmc.hdr) hipFree(pl->lmc.hdr);
  if (pl->lmc.ids) hipFree(pl->lmc.ids);
  if (pl->lmc.pts) hipFree(pl->lmc.pts);
  pl->lmc = LmCloudRec{};
}

extern "C" void flvis_pipeline_destroy_internal(flvis_ctx* ctx) {
  if (!ctx || !ctx->pipe) return;
  Pipeline* pl = ctx->pipe;
  for (int k = 0; k < Pipeline::NBA; k++)
    if (pl->ba_stream[k]) hipStreamSynchronize(pl->ba_stream[k]);
  for (Lane* L : pl->lanes) lane_destroy(L);
  for (int k = 0; k < Pipeline::NBA; k++)
    if (pl->ba_stream[k]) hipStreamDestroy(pl->ba_stream[k]);
  if (pl->hf.strm) {
    hipStreamSynchronize(pl->hf.strm);
    hipStreamDestroy(pl->hf.strm);
    for (int k = 0; k < 2; k++) {
      if (pl->hf.ev_done[k]) hipEventDestroy(pl->hf.ev_done[k]);
      if (pl->hf.ev_free[k]) hipEventDestroy(pl->hf.ev_free[k]);
      if (pl->hf.ev_t0[k]) hipEventDestroy(pl->hf.ev_t0[k]);
      if (pl->hf.ev_t1[k]) hipEventDestroy(pl->hf.ev_t1[k]);
    }
    if (pl->hf.h_up) hipHostFree((void*)pl->hf.h_up);
    for (long long* fp : pl->hf.h_flag)
      if (fp) hipHostFree(fp);
  }
  if (pl->ev_in) hipEventDestroy(pl->ev_in);
  if (pl->lmc_ev) hipEventDestroy(pl->lmc_ev);
  lm_cloud_free(pl);
  kf_log_free(pl);
  for (void* p : pl->allocs) hipFree(p);
  delete pl;
  ctx->pipe = nullptr;
}

// LDS a local-map workgroup claims (FLVIS_BA_LDS_KB, 64 .. 159; other values are ignored): whatever it leaves of the CU's 160 KB lets LK /
// corner-response waves run on the same CU, whose SIMDs a latency-bound BA workgroup keeps mostly idle.  A/B knob, see DESIGN.md section 4;
// a tracker is only created with a budget that holds its window (check_cfg)
static int ba_lds_bytes_env() {
  int bytes = ba_lds_budget_max();
  if (const char* e = getenv("FLVIS_BA_LDS_KB")) {
    const int kb = atoi(e);
    if (kb >= 64 && kb * 1024 <= ba_lds_budget_max()) bytes = kb * 1024;
  }
  return bytes;
}

// device state + streams of one lane; false on any allocation failure (the caller destroys the pipeline)
static bool lane_create(flvis_ctx* ctx, Pipeline* pl, Lane* L, int s0, int S, uint64_t seed_base, int traj_capacity, bool own_stream) {
  const flvis_cfg* cfg = &pl->cfg;
  const int w = cfg->image_width, h = cfg->image_height;
  L->s0 = s0;
  L->S = S;
  Pipe& p = L->pipe;
  memset(&p, 0, sizeof(p));
  p.S = S;
  CamParams& c = p.cam;
  c.cam_type = cfg->cam_type;
  c.w = w;
  c.h = h;
  c.need_equal_hist = cfg->need_equal_hist;
  c.skip_first_n = cfg->skip_first_n_imgs;
  c.dem.regionWidth = (int)std::floor(w / 4.0);
  c.dem.regionHeight = (int)std::floor(h / 4.0);
  c.dem.boundary_dis = (int)std::floor(cfg->feature_para[2] / 2.0);
  c.dem.max_region_feature_num = (unsigned)cfg->feature_para[0];
  c.gftt_num = (int)cfg->feature_para[3];
  c.gftt_ql = cfg->feature_para[4];
  c.gftt_dis = (int)cfg->feature_para[5];
  c.window = cfg->window_size;
  c.seed = seed_base;

  bool ok = true;
#define DA(field, T, n) ok = ok && ((p.field = dalloc<T>(L->allocs, (n))) != nullptr)
  RigParams* rig = dalloc<RigParams>(L->allocs, S);
  ok = ok && rig;
  p.rig = rig;
  DA(st, StreamState, S);
  DA(lm, Landmark, (size_t)2 * S * NMAX);
  DA(vi, MotionState, (size_t)S * VI_QUEUE);
  DA(imu_out, double, (size_t)S * IMU_OUT_CAP * 11);
  DA(prev_pts, float, (size_t)S * NMAX * 2);
  DA(next_pts, float, (size_t)S * NMAX * 2);
  DA(lk_status, uint8_t, (size_t)S * NMAX);
  DA(lk_count, int, S);
  DA(lk_slot, int, (size_t)S * NMAX);
  DA(lk_tag, long long, S);
  DA(m1, float, (size_t)S * NMAX * 2);
  DA(m2, float, (size_t)S * NMAX * 2);
  DA(tri, double, (size_t)S * NMAX * 3);
  DA(tri_mask, uint8_t, (size_t)S * NMAX);
  DA(new_xy, float, (size_t)S * NEW_MAX * 2);
  DA(n_new, int, S);
  DA(exist_xy, double, (size_t)S * NMAX * 2);
  DA(n_exist, int, S);
  DA(act_img, int, S);
  DA(act_track, int, S);
  DA(det_mode, int, S);
  DA(det_maxc, int, S);
  DA(gftt_act, int, S);
  DA(gftt_maxc, int, S);
  DA(img_slot, int, S);
  DA(img_slot_in, int, S);
  DA(out, FrameOut, S);
  DA(kfq, KeyFrameDev, (size_t)S * KFQ);
  DA(kfq_tail, unsigned, S);
  DA(kfq_head, unsigned, S);
  DA(kfq_cmd, unsigned, S);
  DA(kfq_skip, unsigned, S);
  DA(kfq_base, unsigned, S);
  DA(kfq_kf, unsigned, S);
  DA(ba_busy, int, S);
  DA(win, WindowDev, S);
  DA(kfs_ring, KeyFrameDev, (size_t)S * BA_WMAX);
  DA(corr, CorrectionDev, S);
  DA(rec_id, int, (size_t)S * POSE_REC);
  DA(rec_T, double, (size_t)S * POSE_REC * 7);
  p.corr_in = nullptr;  // allocated by the first flvis_correction_feed
  DA(counters, long long, 64);
  p.ba_scratch_stride = ba_scratch_doubles();
  p.imu_factor = 0;
  p.imu_sigma_g = 0;
  p.imu_sigma_a = 0;
  // Keyframes a local-map workgroup takes from its stream's queue per launch.  A workgroup that kept draining a busy stream's queue
  // (0: the behaviour up to round 4) made its LAUNCH last as long as that stream stayed busy, the launches behind it on the same HIP
  // stream -- with every other stream's keyframes -- waited, and the tracker either met the back-pressure below (5-8 ms frame chains in
  // one run of three at KFQ = 16) or left the local map a backlog at the end of the run (7-18 ms at KFQ = 32), although no queue was
  // near full.  With one keyframe per launch every launch is one optimisation long, the launch that follows every frame takes the
  // stream's next keyframe, and the two local-map streams never fall behind: 54.2-54.3k frames/s in four runs of four, against
  // 36.8-54.1k (profiles/r04_local_map_and_streams_ab.md).
  p.ba_drain = 1;
  // ... with a bound: an owner that finds KFQ / 2 or more keyframes still waiting after its share stays and goes on (a stream whose
  // optimisations take longer than its keyframes arrive -- every frame a keyframe -- would otherwise grow a backlog that only ends at
  // the full queue, where k_frame_end drops keyframes).  A launch takes at least the keyframes of the frames between two launches.
  p.ba_drain = std::max(p.ba_drain, pl->ba_every);
  p.ba_backlog = KFQ / 2;
  // FLVIS_KF_CHECK=1 (test knob): k_frame_end leaves a checksum of the keyframe's landmark arrays (written by all of its waves) in the
  // payload, the local-map worker -- another workgroup, usually on another XCD -- recomputes it from what it reads after its acquire:
  // debug counters 30 (payloads checked) and 31 (mismatches).  The hand-over publishes with ONE agent-scope release by one thread behind a
  // workgroup barrier; tests/test_gpu_pipeline.py runs 64 streams under this check.
  p.kf_check = pl->kf_check;
  p.ba_lds_bytes = ba_lds_bytes_env();  // (admitted for the config's window by check_cfg)
  DA(ba_scratch, double, (size_t)S * p.ba_scratch_stride);
  // FLVIS_PNP_TAIL=cv (opt-in fidelity mode, round 6): behind k_ransac_pnp the pose of the ITERATIVE flag is replaced by what
  // cv::solvePnP(ITERATIVE, useExtrinsicGuess = false) leaves on the RANSAC's inliers -- a DLT start and CvLevMarq, the very function the
  // checker's `make -C oracle TAIL=cv` build runs (cv_solvers.hpp), bit-identical to it (tests/test_gpu_pipeline.py) -- instead of the
  // Gauss-Newton refinement of the winning model.  One wave per stream: the small dense algebra (the 12 x 12 and 6 x 6 Jacobi SVDs, OpenCV's
  // loops as they are written) redundantly in every lane, the sums over the correspondences dealt to the lanes; still milliseconds per
  // frame, which is why it is not the default (the two tails agree to 4.4e-9 m on the first tracked frames: the checker's README).
  p.pnp_tail_cv = pl->pnp_tail_cv;
  p.pnp_tail_ws = nullptr;
  p.pnp_tail_stride = 0;
  if (p.pnp_tail_cv) {
    p.pnp_tail_stride = (size_t)29 * NMAX + 192;  // world points (3 n), pixels (2 n), find_extrinsic_iterative's work (24 n + 192)
    DA(pnp_tail_ws, double, (size_t)S * p.pnp_tail_stride);
  }
  unsigned long long* seeds = dalloc<unsigned long long>(L->allocs, S);
  ok = ok && seeds;
  p.seeds = seeds;
  p.traj_cap = traj_capacity > 0 ? traj_capacity : 0;
  if (p.traj_cap) DA(traj, double, (size_t)S * p.traj_cap * 9);
#undef DA
  // per-frame input block
  const size_t off_imu = sizeof(double) * S, off_tab = off_imu + sizeof(double) * (size_t)S * IMU_MAX * 7,
               off_n = off_tab + 2 * sizeof(void*);
  const size_t off_pres = off_n + sizeof(int) * S;
  L->input_bytes = off_pres + sizeof(int) * S;
  L->in_off_imu = off_imu, L->in_off_tab = off_tab, L->in_off_n = off_n, L->in_off_pres = off_pres;
  p.present = nullptr;
  ok = ok && ((L->d_inputs = dalloc<uint8_t>(L->allocs, L->input_bytes)) != nullptr);
  if (ok) {
    L->d_time = reinterpret_cast<double*>(L->d_inputs);
    p.imu_in = reinterpret_cast<double*>(L->d_inputs + off_imu);
    L->d_tab = reinterpret_cast<const uint8_t**>(L->d_inputs + off_tab);
    p.in_tab = L->d_tab;
    p.n_imu = reinterpret_cast<int*>(L->d_inputs + off_n);
  }
  // image pyramids
  for (int l = 0; l <= pl->levels; l++) {
    for (int k = 0; k < 2; k++) ok = ok && ((L->pyr0[k][l] = dalloc<uint8_t>(L->allocs, pl->lstride[l] * S + 256)) != nullptr);
    ok = ok && ((L->pyr1[l] = dalloc<uint8_t>(L->allocs, pl->lstride[l] * S + 256)) != nullptr);
    if (ok) {  // the level pointers address pixel (0, 0) of stream 0 inside the padded buffers
      const size_t org = (size_t)pl->lby * pl->lpitch[l] + pl->lbx;
      for (int k = 0; k < 2; k++) L->pyr0[k][l] += org;
      L->pyr1[l] += org;
    }
  }
  // LK template cache: the stereo matcher's templates of frame t are the temporal tracker's templates of frame t + 1 (LKParams::tc).
  // Only rigs with a stereo matcher have one; FLVIS_LK_TCACHE=0 turns it off (A/B knob, and the reference point of the cache's test).
  p.tc_cap = 0;
  p.tc = nullptr;
  p.tc_stride = 0;
  L->tc = nullptr;
  {
    const bool on = pl->lk_tcache && pl->cfg.cam_type != CAM_DEPTH && pl->levels_s == pl->levels_t;
    // (Templates made ahead of the stereo launch on a stream of their own were not faster: profiles/r06_templates_ahead.md.)
    if (ok && on) {
      const int cap = std::min(NMAX, (pl->max_pts + 63) / 64 * 64);  // slots: the stereo launch's points
      L->tc_stride = lk_tc_slot_dwords(pl->levels_t);
      const size_t n = (size_t)S * cap * L->tc_stride;
      L->tc = dalloc<uint32_t>(L->allocs, n, false);
      if (L->tc) {
        hipMemset(L->tc, 0xff, n * sizeof(uint32_t));  // no header matches a position or a frame id
        p.tc_cap = cap;
        p.tc = L->tc;
        p.tc_stride = L->tc_stride;
      } else {
        (void)hipGetLastError();  // no memory for it: run without
      }
    }
  }
  // GFTT scratch
  const int cap = gftt_key_cap(w, h);
  L->gftt.cap = cap;
  ok = ok && ((L->gftt.maxenc = dalloc<unsigned>(L->allocs, S)) != nullptr);
  ok = ok && ((L->gftt.nkeys = dalloc<int>(L->allocs, S)) != nullptr);
  ok = ok && ((L->gftt.keys = dalloc<unsigned long long>(L->allocs, (size_t)cap * S, false)) != nullptr);
  ok = ok && ((L->gftt_xy = dalloc<float>(L->allocs, (size_t)S * 2 * c.gftt_num * 2)) != nullptr);
  ok = ok && ((L->gftt_n = dalloc<int>(L->allocs, S)) != nullptr);
  ok = ok && ((L->dem_sorted = dalloc<float>(L->allocs, (size_t)S * 2 * c.gftt_num * 2)) != nullptr);
  ok = ok && ((L->dem_roff = dalloc<int>(L->allocs, (size_t)S * 17)) != nullptr);
  ok = ok && ((L->eq_hist = dalloc<unsigned>(L->allocs, (size_t)S * 256)) != nullptr);
  ok = ok && ((L->eq_lut = dalloc<uint8_t>(L->allocs, (size_t)S * 256)) != nullptr);
  ok = ok && ((L->d_join = dalloc<long long>(L->allocs, (size_t)JOIN_IDS * 8)) != nullptr);
  ok = ok && ((L->d_join_cnt = dalloc<unsigned>(L->allocs, (size_t)JOIN_IDS)) != nullptr);
  if (!ok) return false;
  for (int id = 0; id < JOIN_IDS; id++) L->join[id].word = L->d_join + 8 * id, L->join[id].cnt = L->d_join_cnt + id;
  // initial per-stream state (F2FTracking::init, VIMOTION ctor, landmark id counter 100, glibc rand seed 1): the kernel flvis_reset_streams
  // runs, so that a reset stream and a new one cannot differ (tracker_create synchronises the device before it returns)
  for (int b = 0; b < S; b += RESET_LIST) {
    ResetList rl{};
    rl.n = std::min(RESET_LIST, S - b);
    for (int i = 0; i < rl.n; i++) rl.s[i] = b + i, rl.mode[i] = RS_TRACKER | RS_CREATE;
    launch_stream_reset(nullptr, p, rl, nullptr);
  }
  std::vector<unsigned long long> hseed(S);
  for (int s = 0; s < S; s++) hseed[s] = seed_base + (unsigned long long)(s0 + s);  // the seed of a stream does not depend on the lane partition
  hipMemcpy(seeds, hseed.data(), sizeof(unsigned long long) * S, hipMemcpyHostToDevice);
  hipMemcpy(rig, pl->rigs.data() + s0, sizeof(RigParams) * S, hipMemcpyHostToDevice);
  L->cmd_frame.assign(S, -1);
  L->h_imu.assign((size_t)S * IMU_MAX * 7, 0.0);
  L->h_nimu.assign(S, 0);
  L->imu_read.assign(S, 0);
  for (int k = 0; k < Lane::PIN_RING; k++)
    if (hipHostMalloc(&L->pinned[k], L->input_bytes, hipHostMallocMapped) != hipSuccess) return false;
  for (int k = 0; k < Lane::PIN_RING; k++) {
    void* dv = nullptr;
    if (hipHostGetDevicePointer(&dv, L->pinned[k], 0) != hipSuccess) {
      (void)hipGetLastError();
      dv = nullptr;
    }
    L->pinned_dev[k] = (uint8_t*)dv;
  }
  {
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) return false;
    L->h_progress = (volatile long long*)hp;
    L->d_progress = (long long*)dp;
    for (int k = 0; k < 8; k++) L->h_progress[k] = 0;  // (word 0: frame progress, 1: unused, 2: a timed-out join's sequence number,
                                                        // 3: stream + 1 of a reset command that met a full keyframe queue,
                                                        // 4: BA_OVF_* << 32 | stream + 1 of a local-map window that exceeded a capacity)
    L->pipe.ba_ovf_word = L->d_progress + 4;
  }
  if (own_stream) {
    if (hipStreamCreateWithFlags(&L->st, hipStreamNonBlocking) != hipSuccess) return false;
    L->own_st = true;
  } else {
    L->st = ctx->stream;
  }
  // (the detection stream at the default priority; the lowest was measured no faster: DESIGN.md section 4)
  bool evok = hipStreamCreateWithFlags(&L->det_stream, hipStreamNonBlocking) == hipSuccess;
  for (int id = 0; id < JOIN_IDS && evok; id++) evok = hipEventCreateWithFlags(&L->join[id].ev, pl->ev_flags) == hipSuccess;
  evok = evok && hipEventCreateWithFlags(&L->ev_stagger, pl->ev_flags) == hipSuccess;
  for (hipEvent_t& e : L->ev_end) evok = evok && hipEventCreateWithFlags(&e, pl->ev_flags) == hipSuccess;
  return evok;
}

extern "C" {

}  // extern "C"

// The checks a tracker's config has to pass (every stream's, with a prefix naming it, for the per-stream entry points)
static int check_cfg(flvis_ctx* ctx, const flvis_cfg* cfg, const std::string& pre) {
  const int w = cfg->image_width, h = cfg->image_height;
  if (w < 64 || h < 64) return ctx->fail(FLVIS_ERR_CONFIG, pre + "image must be at least 64 x 64");
  if (cfg->need_equal_hist && (w & 15)) return ctx->fail(FLVIS_ERR_CONFIG, pre + "equalizeHist rigs need an image width that is a multiple of 16");
  if (cfg->feature_para[5] > 64.0) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "feature_para6 (GFTT minDistance) > 64 is not supported");
  if (cfg->window_size > BA_WMAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "window_size exceeds the LDS-resident solver (16)");
  if (!ba_lds_admits(ba_lds_bytes_env(), cfg->window_size)) {
    char msg[192];
    snprintf(msg, sizeof msg, "FLVIS_BA_LDS_KB=%d is below the %d KB the local-map solver needs for window_size %d", ba_lds_bytes_env() / 1024,
             ba_lds_min_bytes(cfg->window_size) / 1024, cfg->window_size);
    return ctx->fail(FLVIS_ERR_CONFIG, pre + msg);
  }
  if (16 * (int)cfg->feature_para[0] > 512) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "feature_para1 (landmarks per region) must be <= 32: the pose LM holds 512 edges");
  if ((int)cfg->feature_para[3] * 2 > 4096) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "feature_para4 (gftt_num) must be <= 2048");
  if ((size_t)((w + 31) / 32) * h * 4 > 96 * 1024) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "image too large for the GFTT LDS bitmap");
  if (cfg->cam_type == CAM_DEPTH && !(cfg->depth_factor > 0)) return ctx->fail(FLVIS_ERR_CONFIG, pre + "depth mode needs depth_factor > 0");
  return FLVIS_OK;
}

// The batch-wide fields (CamParams: buffer sizes, launch geometry, code paths): the name of the first one in which c differs from ref, or
// nullptr when they all agree.  Compared bit for bit (memcmp): a config loaded from the same yaml always matches.
static const char* batch_field_mismatch(const flvis_cfg& ref, const flvis_cfg& c) {
  if (c.type_of_vi != ref.type_of_vi) return "type_of_vi";
  if (c.cam_type != ref.cam_type) return "cam_type";
  if (c.imu_type != ref.imu_type) return "imu_type";
  if (c.image_width != ref.image_width) return "image_width";
  if (c.image_height != ref.image_height) return "image_height";
  static const char* const fp[6] = {"feature_para[0]", "feature_para[1]", "feature_para[2]", "feature_para[3]", "feature_para[4]", "feature_para[5]"};
  for (int i = 0; i < 6; i++)
    if (memcmp(&c.feature_para[i], &ref.feature_para[i], sizeof(double))) return fp[i];
  if (c.window_size != ref.window_size) return "window_size";
  if (c.skip_first_n_imgs != ref.skip_first_n_imgs) return "skip_first_n_imgs";
  if (c.need_equal_hist != ref.need_equal_hist) return "need_equal_hist";
  return nullptr;
}

// Every config of a per-stream entry point: flvis_tracker_create's checks, and the batch-wide fields of `ref`
static int check_stream_cfgs(flvis_ctx* ctx, const flvis_cfg& ref, int n, const flvis_cfg* cfgs, const int* streams, const char* what) {
  for (int i = 0; i < n; i++) {
    const int s = streams ? streams[i] : i;
    const std::string pre = std::string(what) + ": stream " + std::to_string(s) + ": ";
    const int rc = check_cfg(ctx, &cfgs[i], pre);
    if (rc != FLVIS_OK) return rc;
    if (const char* f = batch_field_mismatch(ref, cfgs[i]))
      return ctx->fail(FLVIS_ERR_CONFIG, pre + "batch-wide field " + f + " differs from the tracker's (stream 0)");
  }
  return FLVIS_OK;
}

// Every environment knob the tracker honours, read once when it is created (INTEGRATION.md's table lists them with their defaults).
// (FLVIS_BA_LDS_KB is read by ba_lds_bytes_env: check_cfg needs it before a tracker exists.)
static bool env_is(const char* name, int v) {
  const char* e = getenv(name);
  return e && atoi(e) == v;
}
static void read_knobs(Pipeline* pl) {
  const char* j = getenv("FLVIS_JOIN");
  pl->flag_joins = !(j && !strcmp(j, "event"));  // (default since round 6: 58.6k -> 60.4k frames/s, chain p50 1.047 -> 1.012 ms; "event": rounds 1-5)
  // Under a profiler that collects hardware counters (rocprofv3 --pmc sets ROCPROF_COUNTER_COLLECTION in the application's environment)
  // kernels run ONE AT A TIME: a k_wait_flag that sleeps until a kernel of another stream has stored its word would wait for a kernel
  // that cannot start, and end by its 4 s limit.  Events are resolved by the command processor between kernels: taken there unless
  // FLVIS_JOIN says otherwise.  (The wait for an upload is not affected: the copy engine runs beside a serialised kernel.)
  if (!j) {
    const char* cc = getenv("ROCPROF_COUNTER_COLLECTION");
    if (cc && cc[0] && strcmp(cc, "0") && strcmp(cc, "False") && strcmp(cc, "false")) pl->flag_joins = false;
  }
  pl->fold_joins = pl->flag_joins && !env_is("FLVIS_JOIN_FOLD", 0);
  if (const char* e = getenv("FLVIS_LANES")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 16) pl->n_lanes_req = v;
  }
  pl->lk_border = !env_is("FLVIS_LK_BORDER", 0);
  pl->lk_tcache = !env_is("FLVIS_LK_TCACHE", 0);
  pl->head_prepare = !env_is("FLVIS_HEAD_PREPARE", 0);
  if (const char* e = getenv("FLVIS_HOST_LEAD")) pl->host_lead = std::max(1, std::min(atoi(e), (int)Lane::PIN_RING));
  if (const char* e = getenv("FLVIS_SYNC_EACH_FRAME")) pl->sync_each_frame = atoi(e) != 0;
  if (const char* e = getenv("FLVIS_CHAIN_MERGE")) pl->chain_merge = atoi(e) & 31;
  if (const char* e = getenv("FLVIS_BA_EVERY")) {
    const int v = atoi(e);
    if (v >= 1 && v <= KFQ / 4) pl->ba_every = v;  // (the back-pressure in lane_frame needs (D + 2) * ba_every <= KFQ / 2)
  }
  pl->kf_check = env_is("FLVIS_KF_CHECK", 1);
  if (const char* e = getenv("FLVIS_PNP_TAIL")) pl->pnp_tail_cv = !strcmp(e, "cv");
  if (const char* e = getenv("FLVIS_H2D_MODE")) pl->hf.mode = atoi(e) == 1 ? 1 : 2;
  if (const char* e = getenv("FLVIS_PROF_EVENT_SCOPE")) pl->prof_scope = !strcmp(e, "agent") ? hipEventReleaseToDevice : 0u;
}

// cfgs: one config for all streams (n_cfgs 1, flvis_tracker_create) or one per stream (n_cfgs = n_streams), checked by the caller
static int tracker_create_impl(flvis_ctx* ctx, const flvis_cfg* cfgs, int n_cfgs, int n_streams, uint64_t seed_base, int traj_capacity) {
  const flvis_cfg* cfg = &cfgs[0];
  const int w = cfg->image_width, h = cfg->image_height;
  hipSetDevice(ctx->device);
  Pipeline* pl = new Pipeline();
  ctx->pipe = pl;
  read_knobs(pl);
  const int S = n_streams;
  pl->S = S;
  pl->cfg = *cfg;
  pl->cfgs.resize(S);
  pl->rigs.resize(S);
  for (int k = 0; k < S; k++) {
    pl->cfgs[k] = cfgs[n_cfgs == 1 ? 0 : k];
    if (k > 0 && n_cfgs == 1) pl->rigs[k] = pl->rigs[0];
    else rig_from_cfg(pl->cfgs[k], pl->rigs[k]);
  }
  pl->max_pts = std::min(NMAX, 16 * (int)cfg->feature_para[0]);
  // pyramid geometry
  pl->levels_t = lk_levels(w, h, 31, 10);
  pl->levels_s = lk_levels(w, h, 31, 5);
  pl->levels = std::max(pl->levels_t, pl->levels_s);
  if (pl->levels >= LK_MAX_LEVELS) pl->levels = LK_MAX_LEVELS - 1;
  pl->lbx = pl->lk_border ? LK_BORDER_X : 0;
  pl->lby = pl->lk_border ? LK_BORDER_Y : 0;
  int lw = w, lh = h;
  for (int l = 0; l <= pl->levels; l++) {
    pl->lw[l] = lw;
    pl->lh[l] = lh;
    // levels are stored with a physical BORDER_REFLECT_101 border (img_kernels.hpp: LK_BORDER_X / LK_BORDER_Y; FLVIS_LK_BORDER=0: none,
    // A/B knob): the level pointers address pixel (0, 0), rows -lby .. lh + lby - 1 and columns -lbx .. pitch - lbx - 1 are storage
    pl->lpitch[l] = align_up(lw, 16) + 2 * pl->lbx;
    pl->lstride[l] = (size_t)pl->lpitch[l] * (lh + 2 * pl->lby) + 64;
    pl->lstride[l] = (pl->lstride[l] + 63) / 64 * 64;
    lw = (lw + 1) / 2;
    lh = (lh + 1) / 2;
  }
  // lanes: one by default.  Measured on MI355X with 64 streams (bench.py, round 2): 1 lane 1.67 ms per step, 2 lanes 2.23 ms,
  // 4 lanes 2.94 ms -- a lane's one-workgroup-per-stream geometry kernels share their CUs with the other lanes' LK waves and
  // slow down by more than the overlap gains.  FLVIS_LANES (1..16) is kept as a tuning knob.
  int n_lanes = std::min(pl->n_lanes_req, S);
  pl->lane_size = (S + n_lanes - 1) / n_lanes;
  n_lanes = (S + pl->lane_size - 1) / pl->lane_size;
  pl->nba_lane = std::max(1, std::min(pl->nba_lane, Pipeline::NBA / n_lanes));
  pl->nba = std::min(Pipeline::NBA, pl->nba_lane * n_lanes);  // (more than NBA / nba_lane lanes share local-map streams)
  bool ok = true;
  for (int k = 0; k < n_lanes && ok; k++) {
    Lane* L = new Lane();
    L->idx = k;
    pl->lanes.push_back(L);
    const int s0 = k * pl->lane_size;
    ok = lane_create(ctx, pl, L, s0, std::min(pl->lane_size, S - s0), seed_base, traj_capacity, n_lanes > 1);
  }
  // the local map must not displace the tracking chain: its streams get the lowest queue priority
  int prio_least = 0, prio_greatest = 0;
  hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  for (int k = 0; k < pl->nba && ok; k++)
    ok = hipStreamCreateWithPriority(&pl->ba_stream[k], hipStreamNonBlocking, prio_least) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&pl->ev_in, pl->ev_flags) == hipSuccess;
  if (!ok) {
    flvis_pipeline_destroy_internal(ctx);
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, "tracker_create: device / pinned allocation or stream creation failed");
  }
  if (ba_kernels_init() != hipSuccess || track_kernels_init() != hipSuccess) {
    (void)hipGetLastError();
    flvis_pipeline_destroy_internal(ctx);
    return ctx->fail(FLVIS_ERR_HIP, "tracker_create: cannot reserve LDS for the BA kernel");
  }
  hipDeviceSynchronize();
  return FLVIS_OK;
}

extern "C" {

int flvis_tracker_create(flvis_ctx* ctx, const flvis_cfg* cfg, int n_streams, uint64_t seed_base, int traj_capacity) {
  if (!ctx || !cfg || n_streams <= 0) return FLVIS_ERR_INVALID_ARG;
  if (ctx->pipe) flvis_pipeline_destroy_internal(ctx);
  const int rc = check_cfg(ctx, cfg, "");
  if (rc != FLVIS_OK) return rc;
  return tracker_create_impl(ctx, cfg, 1, n_streams, seed_base, traj_capacity);
}

int flvis_tracker_create_rigs(flvis_ctx* ctx, const flvis_cfg* cfgs, int n_streams, uint64_t seed_base, int traj_capacity) {
  if (!ctx || !cfgs || n_streams <= 0) return FLVIS_ERR_INVALID_ARG;
  const int rc = check_stream_cfgs(ctx, cfgs[0], n_streams, cfgs, nullptr, "tracker_create_rigs");
  if (rc != FLVIS_OK) return rc;  // (nothing created: a tracker the context holds stays)
  if (ctx->pipe) flvis_pipeline_destroy_internal(ctx);
  return tracker_create_impl(ctx, cfgs, n_streams, n_streams, seed_base, traj_capacity);
}

int flvis_get_stream_cfg(flvis_ctx* ctx, int stream, flvis_cfg* out) {
  if (!ctx || !out) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (!pl) return ctx->fail(FLVIS_ERR_INVALID_ARG, "get_stream_cfg: no tracker (flvis_tracker_create)");
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "get_stream_cfg: stream out of range");
  *out = pl->cfgs[stream];
  return FLVIS_OK;
}

// The reference integrates every IMU message as it arrives, without a limit.  Here samples are staged per stream and consumed
// by the next image_feed; when a stream's staging slot (IMU_MAX samples) is full -- an IMU that leads the camera, a dropped
// image -- the staged samples of the lane are integrated at once (blocking upload + k_imu_feed: a rare path) and staging goes on.
static int lane_flush_imu(flvis_ctx* ctx, Lane& L) {
  hipError_t e = hipStreamSynchronize(L.st);
  // (the device block of the copying mode: idle after the synchronisation whichever mode the frames use)
  L.pipe.imu_in = reinterpret_cast<double*>(L.d_inputs + L.in_off_imu);
  L.pipe.n_imu = reinterpret_cast<int*>(L.d_inputs + L.in_off_n);
  if (e == hipSuccess) e = hipMemcpy(L.pipe.imu_in, L.h_imu.data(), sizeof(double) * L.h_imu.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(L.pipe.n_imu, L.h_nimu.data(), sizeof(int) * L.S, hipMemcpyHostToDevice);
  if (e != hipSuccess) return ctx->hip_fail(e, "imu_feed (flush)");
  launch_imu_feed(L.st, L.pipe);
  e = hipStreamSynchronize(L.st);
  if (e != hipSuccess) return ctx->hip_fail(e, "imu_feed (flush)");
  std::fill(L.h_nimu.begin(), L.h_nimu.end(), 0);
  return FLVIS_OK;
}

int flvis_imu_feed_flvis_frame(flvis_ctx* ctx, int stream, int n, const double* samples7) {
  if (!ctx || !ctx->pipe || !samples7) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S || n < 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "imu_feed: bad stream");
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  while (n > 0) {
    int& cnt = L.h_nimu[ls];
    if (cnt == IMU_MAX) {
      hipSetDevice(ctx->device);
      const int rc = lane_flush_imu(ctx, L);
      if (rc != FLVIS_OK) return rc;
    }
    const int m = std::min(n, IMU_MAX - L.h_nimu[ls]);
    memcpy(&L.h_imu[((size_t)ls * IMU_MAX + L.h_nimu[ls]) * 7], samples7, sizeof(double) * 7 * m);
    L.h_nimu[ls] += m;
    samples7 += 7 * (size_t)m;
    n -= m;
  }
  return FLVIS_OK;
}

int flvis_imu_feed(flvis_ctx* ctx, int stream, double t, const double* a, const double* g) {
  if (!ctx || !ctx->pipe || !a || !g) return FLVIS_ERR_INVALID_ARG;
  double s[7];
  s[0] = t;
  if (ctx->pipe->cfg.imu_type == 3) return ctx->fail(FLVIS_ERR_CONFIG, "imu_feed: this rig has no IMU (type_of_vi 4: imu_type NONE)");
  switch (ctx->pipe->cfg.imu_type) {  // src/frontend/vo_tracking.cpp:331-357
    case 0:                            // D435I
      s[1] = -a[2]; s[2] = a[0]; s[3] = a[1];
      s[4] = g[2]; s[5] = -g[0]; s[6] = -g[1];
      break;
    case 1:  // EuRoC_MAV
      s[1] = -a[2]; s[2] = a[1]; s[3] = -a[0];
      s[4] = g[2]; s[5] = -g[1]; s[6] = g[0];
      break;
    default:  // PIXHAWK
      s[1] = -a[0]; s[2] = -a[1]; s[3] = -a[2];
      s[4] = g[0]; s[5] = g[1]; s[6] = g[2];
      break;
  }
  return flvis_imu_feed_flvis_frame(ctx, stream, 1, s);
}

// F2FTracking::imu_feed's outputs (f2f_tracking.cpp:46-57), fetched in batches: the rows written since the previous call.
int flvis_get_imu_states(flvis_ctx* ctx, int stream, int cap, double* h_rows11, int* n_out, int* n_dropped) {
  if (!ctx || !ctx->pipe || !n_out || cap < 0 || (cap > 0 && !h_rows11)) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "get_imu_states: bad stream");
  hipSetDevice(ctx->device);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  // samples staged since the last image feed are integrated now (same arithmetic, same order as at the next frame head)
  bool staged = false;
  for (int s = 0; s < L.S; s++) staged = staged || L.h_nimu[s] > 0;
  if (staged) {
    const int rc = lane_flush_imu(ctx, L);
    if (rc != FLVIS_OK) return rc;
  } else {
    hipError_t e = hipStreamSynchronize(L.st);
    if (e != hipSuccess) return ctx->hip_fail(e, "get_imu_states");
  }
  long long seen = 0;
  hipError_t e = hipMemcpy(&seen, reinterpret_cast<const char*>(L.pipe.st + ls) + offsetof(StreamState, imu_seen), sizeof(seen),
                           hipMemcpyDeviceToHost);
  if (e != hipSuccess) return ctx->hip_fail(e, "get_imu_states");
  long long first = L.imu_read[ls];
  int dropped = 0;
  if (seen - first > IMU_OUT_CAP) {  // the ring wrapped since the last fetch: the oldest rows are gone
    dropped = (int)std::min<long long>(seen - first - IMU_OUT_CAP, 0x7fffffff);
    first = seen - IMU_OUT_CAP;
  }
  const long long avail = seen - first;
  const int n = (int)std::min<long long>(avail, cap);
  const double* ring = L.pipe.imu_out + (size_t)ls * IMU_OUT_CAP * 11;
  for (int done = 0; done < n && e == hipSuccess;) {  // at most two pieces (ring wrap)
    const int r0 = (int)((first + done) % IMU_OUT_CAP);
    const int m = std::min(n - done, IMU_OUT_CAP - r0);
    e = hipMemcpy(h_rows11 + (size_t)done * 11, ring + (size_t)r0 * 11, sizeof(double) * 11 * m, hipMemcpyDeviceToHost);
    done += m;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, "get_imu_states");
  L.imu_read[ls] = first + n;  // rows beyond cap stay for the next call
  *n_out = n;
  if (n_dropped) *n_dropped = dropped;
  return FLVIS_OK;
}

// The call-for-call form of F2FTracking::imu_feed(time, acc, gyro, q_w_i&, pos_w_i&, vel_w_i&): the sample is integrated NOW
// (upload + k_imu_feed + read-back, ~0.1 ms) and its state returned, as imu_callback needs it for /imu_pose, /imu_odom and
// /imu_path (vo_tracking.cpp:362-369).
int flvis_imu_feed_out(flvis_ctx* ctx, int stream, double t, const double* acc3, const double* gyro3, double* q_w_i_wxyz,
                       double* pos_w_i, double* vel_w_i) {
  if (!q_w_i_wxyz || !pos_w_i || !vel_w_i) return FLVIS_ERR_INVALID_ARG;
  int rc = flvis_imu_feed(ctx, stream, t, acc3, gyro3);
  if (rc != FLVIS_OK) return rc;
  Pipeline* pl = ctx->pipe;
  hipSetDevice(ctx->device);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  rc = lane_flush_imu(ctx, L);
  if (rc != FLVIS_OK) return rc;
  long long seen = 0;
  hipError_t e = hipMemcpy(&seen, reinterpret_cast<const char*>(L.pipe.st + ls) + offsetof(StreamState, imu_seen), sizeof(seen),
                           hipMemcpyDeviceToHost);
  double row[11];
  if (e == hipSuccess && seen > 0)
    e = hipMemcpy(row, L.pipe.imu_out + ((size_t)ls * IMU_OUT_CAP + (size_t)((seen - 1) % IMU_OUT_CAP)) * 11, sizeof(row),
                  hipMemcpyDeviceToHost);
  if (e != hipSuccess) return ctx->hip_fail(e, "imu_feed_out");
  if (seen <= 0) return ctx->fail(FLVIS_ERR_HIP, "imu_feed_out: the sample was not integrated");
  memcpy(q_w_i_wxyz, row + 1, 32);
  memcpy(pos_w_i, row + 5, 24);
  memcpy(vel_w_i, row + 8, 24);
  return FLVIS_OK;
}


int flvis_prof_enable(flvis_ctx* ctx, int max_steps) { return flvis_prof_enable_stages(ctx, max_steps, ~0ull); }

int flvis_prof_enable_stages(flvis_ctx* ctx, int max_steps, uint64_t stage_mask) {
  if (!ctx || !ctx->pipe || max_steps < 0) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  pl->prof_mask = stage_mask;
  sync_all(ctx);
  pl->prof_cap = max_steps;
  pl->prof_step = 0;
  // release scope of the stage events (FLVIS_PROF_EVENT_SCOPE=agent|system; default: what the pipeline's own events use)
  const unsigned prof_scope = pl->prof_scope;
  for (Lane* L : pl->lanes) {
    for (hipEvent_t e : L->prof_ev) hipEventDestroy(e);
    L->prof_ev.clear();
    L->prof_ev.resize((size_t)max_steps * (2 * PROF_STAGES));
    L->prof18_rec.assign((size_t)max_steps + 1, 0);
    for (auto& e : L->prof_ev)
      if (hipEventCreateWithFlags(&e, prof_scope) != hipSuccess) return ctx->fail(FLVIS_ERR_HIP, "prof_enable: hipEventCreate failed");
  }
  return FLVIS_OK;
}

int flvis_prof_stage_count(void) { return PROF_STAGES; }
const char* flvis_prof_stage_name(int i) { return (i >= 0 && i < PROF_STAGES) ? kStageNames[i] : ""; }
int flvis_tracker_lanes(flvis_ctx* ctx) { return (ctx && ctx->pipe) ? (int)ctx->pipe->lanes.size() : 0; }

static bool prof_stage_timed(const Pipeline* pl, int i) {
  if (!((pl->prof_mask >> i) & 1ull)) return false;
  if (i >= 10 && i <= 12 && ((pl->prof_mask >> 10) & 7ull) != 7ull) return false;  // the GFTT chain is timed as a whole
  return true;
}

// per stage: the elapsed time of one LAUNCH (one lane's kernel(s) of that stage), summed over the armed frames and averaged
// over the lanes -- with several lanes the stages of different lanes overlap, so the sum over stages exceeds the step time
int flvis_prof_read(flvis_ctx* ctx, double* h_ms_per_stage, int* n_steps) {
  if (!ctx || !ctx->pipe || !h_ms_per_stage || !n_steps) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  sync_all(ctx);
  for (int i = 0; i < PROF_STAGES; i++) h_ms_per_stage[i] = 0;
  size_t rec18 = 0;
  for (Lane* L : pl->lanes)
    for (int k = 0; k < pl->prof_step; k++)
      for (int i = 0; i < PROF_STAGES; i++) {
        float ms = 0;
        if (!prof_stage_timed(pl, i)) continue;
        if (i == 18) {
          if (!L->prof18_rec[(size_t)k]) continue;
          rec18++;
        }
        // (a stage that was not enqueued in this frame -- a deferred local-map launch (Pipeline::defer_ba) -- has no recorded events: it counts 0)
        if (hipEventElapsedTime(&ms, L->prof_ev[(size_t)k * (2 * PROF_STAGES) + 2 * i], L->prof_ev[(size_t)k * (2 * PROF_STAGES) + 2 * i + 1]) != hipSuccess) {
          (void)hipGetLastError();
          ms = 0;
        }
        h_ms_per_stage[i] += ms / (double)pl->lanes.size();
      }
  // (stage 18 as the mean over the steps that timed a launch: the caller divides every stage's sum by n_steps)
  if (rec18 > 0 && rec18 < pl->lanes.size() * (size_t)pl->prof_step) h_ms_per_stage[18] *= (double)(pl->lanes.size() * (size_t)pl->prof_step) / (double)rec18;
  *n_steps = pl->prof_step;
  return FLVIS_OK;
}

// per armed frame: the slowest lane's elapsed time of the stage
int flvis_prof_read_steps(flvis_ctx* ctx, int stage, double* h_ms, int cap) {
  if (!ctx || !ctx->pipe || !h_ms || stage < 0 || stage >= PROF_STAGES || cap < 0) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (!prof_stage_timed(pl, stage)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "prof_read_steps: stage was not enabled");
  sync_all(ctx);
  int n = 0;
  for (int k = 0; k < pl->prof_step && n < cap; k++, n++) {
    double worst = 0;
    for (Lane* L : pl->lanes) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, L->prof_ev[(size_t)k * (2 * PROF_STAGES) + 2 * stage], L->prof_ev[(size_t)k * (2 * PROF_STAGES) + 2 * stage + 1]) != hipSuccess) {
        (void)hipGetLastError();
        ms = 0;
      }
      worst = std::max(worst, (double)ms);
    }
    h_ms[n] = worst;
  }
  return n;
}

int flvis_get_landmarks(flvis_ctx* ctx, int stream, int cap, int64_t* h_id, double* h_2d, double* h_2du, double* h_3d,
                        uint8_t* h_flags) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  sync_all(ctx);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  StreamState st;
  hipMemcpy(&st, L.pipe.st + ls, sizeof(st), hipMemcpyDeviceToHost);
  int n = st.n_lm[st.cur];
  std::vector<Landmark> lm(n);
  if (n) hipMemcpy(lm.data(), L.pipe.lm + ((size_t)st.cur * L.S + ls) * NMAX, sizeof(Landmark) * n, hipMemcpyDeviceToHost);
  for (int i = 0; i < n && i < cap; i++) {
    h_id[i] = lm[i].id;
    h_2d[2 * i] = lm[i].p2d[0];
    h_2d[2 * i + 1] = lm[i].p2d[1];
    h_2du[2 * i] = lm[i].p2u[0];
    h_2du[2 * i + 1] = lm[i].p2u[1];
    for (int j = 0; j < 3; j++) h_3d[3 * i + j] = lm[i].p3w[j];
    h_flags[i] = (uint8_t)((lm[i].has3d ? 1 : 0) | (lm[i].inlier ? 2 : 0));
  }
  return n;
}

int flvis_get_keyframe(flvis_ctx* ctx, int stream, int cap, int64_t* frame_id, double* T7, int64_t* h_id, double* h_2d,
                       double* h_3d) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  sync_all(ctx);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  std::vector<KeyFrameDev> kfv(1);
  KeyFrameDev& kf = kfv[0];
  FrameOut fo;
  hipMemcpy(&fo, L.pipe.out + ls, sizeof(FrameOut), hipMemcpyDeviceToHost);
  if (!fo.new_keyframe) return 0;  // the last frame of this stream did not become a keyframe
  unsigned tl = 0;  // (the stream's last keyframe entry: the queue's last entry may be a reset command)
  hipMemcpy(&tl, L.pipe.kfq_kf + ls, sizeof(unsigned), hipMemcpyDeviceToHost);
  if (tl == 0) return 0;
  hipMemcpy(&kf, L.pipe.kfq + (size_t)ls * KFQ + ((tl - 1) % KFQ), sizeof(KeyFrameDev), hipMemcpyDeviceToHost);
  *frame_id = kf.frame_id;
  memcpy(T7, kf.T_c_w, 56);
  for (int i = 0; i < kf.lm_count && i < cap; i++) {
    h_id[i] = kf.lm_id[i];
    h_2d[2 * i] = kf.lm_2d[i][0];
    h_2d[2 * i + 1] = kf.lm_2d[i][1];
    for (int j = 0; j < 3; j++) h_3d[3 * i + j] = kf.lm_3d[i][j];
  }
  return kf.lm_count;
}

int flvis_get_keyframe_msg(flvis_ctx* ctx, int stream, int cap, flvis_keyframe* kf, int64_t* h_id, double* h_2d, double* h_3d,
                           uint8_t* h_img0, uint8_t* h_img1) {
  if (!ctx || !ctx->pipe || !kf || cap < 0 || (cap && (!h_id || !h_2d || !h_3d))) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  int64_t fid = 0;
  const int n = flvis_get_keyframe(ctx, stream, cap, &fid, kf->T_c_w, h_id, h_2d, h_3d);
  if (n <= 0) return n;
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  const int w = pl->cfg.image_width, h = pl->cfg.image_height;
  const bool depth_cam = pl->cfg.cam_type == CAM_DEPTH;
  unsigned tl = 0;
  double stamp = 0;
  int slot = 0;
  hipMemcpy(&tl, L.pipe.kfq_kf + ls, sizeof(unsigned), hipMemcpyDeviceToHost);
  hipMemcpy(&stamp, &L.pipe.kfq[(size_t)ls * KFQ + ((tl - 1) % KFQ)].stamp, sizeof(double), hipMemcpyDeviceToHost);
  hipMemcpy(&slot, L.pipe.img_slot + ls, sizeof(int), hipMemcpyDeviceToHost);
  kf->frame_id = fid;
  kf->command = 0;  // KFMSG_CMD_NONE (keyframe_msg.h:10)
  kf->stamp = stamp;
  kf->lm_count = n;
  kf->lm_id = h_id;
  kf->lm_2d = h_2d;
  kf->lm_3d = h_3d;
  kf->img0 = flvis_image{h_img0, w, h, w, 1, stamp};
  kf->img1 = flvis_image{h_img1, w, h, depth_cam ? 2 * w : w, 1, stamp};
  hipError_t e = hipSuccess;
  if (h_img0)  // level 0 of the left pyramid, the slot of the stream's last processed frame (after equalizeHist where used)
    e = hipMemcpy2D(h_img0, w, L.pyr0[slot & 1][0] + (size_t)ls * pl->lstride[0], pl->lpitch[0], w, h, hipMemcpyDeviceToHost);
  if (e == hipSuccess && h_img1) {
    const bool eq = pl->cfg.need_equal_hist != 0, aligned = (w & 15) == 0;
    const uint8_t* tab[2] = {nullptr, nullptr};
    if (depth_cam || (!eq && aligned)) {  // read in place from the caller's buffer of that frame (still the table's entry)
      tab[0] = L.h_tab[0], tab[1] = L.h_tab[1];
      const size_t bpp = depth_cam ? 2 : 1;
      if (e == hipSuccess) e = hipMemcpy(h_img1, tab[1] + (size_t)ls * w * h * bpp, (size_t)w * h * bpp, hipMemcpyDeviceToHost);
    } else {
      e = hipMemcpy2D(h_img1, w, L.pyr1[0] + (size_t)ls * pl->lstride[0], pl->lpitch[0], w, h, hipMemcpyDeviceToHost);
    }
  }
  if (e != hipSuccess) return ctx->hip_fail(e, "get_keyframe_msg");
  return n;
}

static int read_correction(Lane& L, int ls, int cap, int64_t* frame_id, double* T7, int* lm_count, int64_t* h_id,
                           double* h_3d, int* oc, int64_t* h_oid) {
  std::vector<CorrectionDev> cv(1);
  CorrectionDev& c = cv[0];
  hipMemcpy(&c, L.pipe.corr + ls, sizeof(CorrectionDev), hipMemcpyDeviceToHost);
  if (!c.valid) return 0;
  *frame_id = c.frame_id;
  memcpy(T7, c.T_c_w, 56);
  *lm_count = c.lm_count;
  for (int i = 0; i < c.lm_count && i < cap; i++) {
    h_id[i] = c.lm_id[i];
    for (int j = 0; j < 3; j++) h_3d[3 * i + j] = c.lm_3d[i][j];
  }
  *oc = c.lm_outlier_count;
  for (int i = 0; i < c.lm_outlier_count && i < cap; i++) h_oid[i] = c.lm_outlier_id[i];
  return 1;
}

int flvis_get_correction(flvis_ctx* ctx, int stream, int cap, int64_t* frame_id, double* T7, int* lm_count, int64_t* h_id,
                         double* h_3d, int* oc, int64_t* h_oid) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  if (stream < 0 || stream >= ctx->pipe->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  sync_all(ctx);
  int ls;
  Lane& L = ctx->pipe->lane_of(stream, ls);
  return read_correction(L, ls, cap, frame_id, T7, lm_count, h_id, h_3d, oc, h_oid);
}

int flvis_get_trajectory(flvis_ctx* ctx, int stream, int first, int n, double* h_rows9) {
  if (!ctx || !ctx->pipe || !h_rows9) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "get_trajectory: out of range");
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  if (first < 0 || n < 0 || first + n > L.pipe.traj_cap) return ctx->fail(FLVIS_ERR_INVALID_ARG, "get_trajectory: out of range");
  sync_all(ctx);
  hipMemcpy(h_rows9, L.pipe.traj + ((size_t)ls * L.pipe.traj_cap + first) * 9, sizeof(double) * 9 * n, hipMemcpyDeviceToHost);
  return n;
}

int flvis_write_trajectory(flvis_ctx* ctx, int stream, int first, int n, const char* path, int format, double min_dt) {
  if (!ctx || !ctx->pipe || !path || (format != 0 && format != 1)) return FLVIS_ERR_INVALID_ARG;
  std::vector<double> rows((size_t)(n > 0 ? n : 0) * 9);
  int got = flvis_get_trajectory(ctx, stream, first, n, rows.data());
  if (got < 0) return got;
  FILE* f = fopen(path, "w");
  if (!f) return ctx->fail(FLVIS_ERR_INVALID_ARG, "write_trajectory: cannot open the output file");
  int written = 0;
  bool have_first = false;
  double first_t = 0;
  for (int i = 0; i < got; i++) {
    const double* r = &rows[(size_t)i * 9];
    if (((int)r[8] & 15) != 1) continue;  // only frames of a TRACKING stream carry a pose
    const double t = r[0];
    if (min_dt > 0) {
      // vo_repub_rec.cpp:77-78: `last_time` is a function-static initialised at the FIRST call and never updated, so the
      // recorder drops the poses of the first min_dt (0.1 s of wall clock there, stamps here) and writes every pose after
      if (!have_first) {
        have_first = true;
        first_t = t;
      }
      if (!(t - first_t > min_dt)) continue;
    }
    // T_c_w = (t, q) -> T_w_c: R_w_c = R^T, centre = -R^T t
    double qx = r[4], qy = r[5], qz = r[6], qw = r[7];
    const double qn = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    qx /= qn; qy /= qn; qz /= qn; qw /= qn;
    const double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)},
                            {2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)},
                            {2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)}};
    double c[3];
    for (int k = 0; k < 3; k++) c[k] = -(R[0][k] * r[1] + R[1][k] * r[2] + R[2][k] * r[3]);
    if (format == 0) {
      // operator<< with setprecision(6) (default float notation) == %.6g; the stamp prints like ros::Time (sec.nsec)
      fprintf(f, "%.9f %.6g %.6g %.6g %.6g %.6g %.6g %.6g\n", t, c[0], c[1], c[2], qw, -qx, -qy, -qz);
    } else {
      fprintf(f, "%.6g %.6g %.6g %.6g %.6g %.6g %.6g %.6g %.6g %.6g %.6g %.6g\n", R[0][0], R[1][0], R[2][0], c[0], R[0][1], R[1][1],
              R[2][1], c[1], R[0][2], R[1][2], R[2][2], c[2]);
    }
    written++;
  }
  fclose(f);
  return written;
}


// The recorder on /imu_pose (launch/flvis_euroc_mav.launch:83-103: vo_repub_rec with sub_type PoseStamped, sub_topic /imu_pose,
// output est.txt): pubPose(q_w_i, pos_w_i, stamp) of every IMU sample, `stamp x y z qw qx qy qz` (vo_repub_rec.cpp:74-91), with
// the throttle as written there (see flvis_write_trajectory).  Rows as flvis_get_imu_states returns them.
int flvis_write_imu_trajectory_run(const double* h_rows11, int n, const char* path, double min_dt, int append, double t_first) {
  if (!path || n < 0 || (n > 0 && !h_rows11)) return FLVIS_ERR_INVALID_ARG;
  FILE* f = fopen(path, append ? "a" : "w");
  if (!f) return FLVIS_ERR_CONFIG;
  int written = 0;
  // the recorder's `last_time` is the stamp of the first message of the RUN (vo_repub_rec.cpp:77-78) and is never updated: rows within
  // min_dt of THAT stamp are dropped, whichever batch they arrive in
  const bool throttle = min_dt > 0 && (t_first == t_first);
  for (int i = 0; i < n; i++) {
    const double* r = h_rows11 + (size_t)i * 11;
    if (throttle && !(r[0] - t_first > min_dt)) continue;
    fprintf(f, "%.9f %.6g %.6g %.6g %.6g %.6g %.6g %.6g\n", r[0], r[5], r[6], r[7], r[1], r[2], r[3], r[4]);
    written++;
  }
  fclose(f);
  return written;
}

// (the two-argument form of the run: the batch that creates the file carries the run's first stamp; a batch that is appended without
// naming it is written in full -- callers whose first batch may be shorter than min_dt use flvis_write_imu_trajectory_run)
int flvis_write_imu_trajectory(const double* h_rows11, int n, const char* path, double min_dt, int append) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  return flvis_write_imu_trajectory_run(h_rows11, n, path, min_dt, append, (!append && n > 0 && h_rows11) ? h_rows11[0] : nan);
}

int flvis_get_counters_n(flvis_ctx* ctx, int n, int64_t* h) {
  if (!ctx || !ctx->pipe || !h || n < 1 || n > 4) return FLVIS_ERR_INVALID_ARG;
  sync_all(ctx);
  int64_t v[4] = {ctx->pipe->stream_frames, 0, 0, 0};
  for (Lane* L : ctx->pipe->lanes) {
    long long c[8];
    hipError_t e = hipMemcpy(c, L->pipe.counters, sizeof(c), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return ctx->hip_fail(e, "get_counters");
    for (int k = 1; k < 4; k++) v[k] += c[k];
  }
  for (int k = 0; k < n; k++) h[k] = v[k];
  return FLVIS_OK;
}

int flvis_get_counters(flvis_ctx* ctx, int64_t* h3) { return flvis_get_counters_n(ctx, 3, h3); }

// per stream: keyframes the tracker has emitted (KeyFrame messages of /vo_kf) and optimisations its local map has run
int flvis_get_local_map_counts(flvis_ctx* ctx, int64_t* h_keyframes, int64_t* h_ba_runs) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  sync_all(ctx);
  for (Lane* L : ctx->pipe->lanes) {
    if (h_keyframes) {  // (the entries behind the stream's last reset command)
      std::vector<unsigned> tl(L->S), base(L->S);
      hipError_t e = hipMemcpy(tl.data(), L->pipe.kfq_tail, sizeof(unsigned) * L->S, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(base.data(), L->pipe.kfq_base, sizeof(unsigned) * L->S, hipMemcpyDeviceToHost);
      if (e != hipSuccess) return ctx->hip_fail(e, "get_local_map_counts");
      for (int i = 0; i < L->S; i++) h_keyframes[L->s0 + i] = tl[i] - base[i];
    }
    if (h_ba_runs) {
      std::vector<long long> r(L->S);
      hipError_t e = hipMemcpy2D(r.data(), sizeof(long long), reinterpret_cast<const char*>(L->pipe.win) + offsetof(WindowDev, ba_runs),
                                 sizeof(WindowDev), sizeof(long long), L->S, hipMemcpyDeviceToHost);
      if (e != hipSuccess) return ctx->hip_fail(e, "get_local_map_counts");
      for (int i = 0; i < L->S; i++) h_ba_runs[L->s0 + i] = r[i];
    }
  }
  return FLVIS_OK;
}

// Per-stream reset (include/flvis_hip.h).  Host side: the stream's staged IMU samples and the IMU-state rows not yet fetched are dropped;
// device side, in stream order on the lane's tracking stream: k_stream_reset (the tracker state of a new stream, and a reset command
// in the keyframe queue that the local map applies in order with the keyframes).  No host synchronisation.
// cfgs (flvis_reset_streams_rigs): the config each named stream starts over on, validated before anything changes; its rig reaches the
// device in stream order ahead of the stream's k_stream_reset (k_set_rig), so the frames before the reset read the old rig and those after
// it the new one.  The local map needs no such point: a keyframe carries the rig it was made with (KeyFrameDev::rig_K).
static int reset_impl(flvis_ctx* ctx, int n, const int* streams, bool tracker, const char* what, const flvis_cfg* cfgs = nullptr) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (!pl) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": no tracker (flvis_tracker_create)");
  if (n < 0 || (n > 0 && !streams)) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": bad stream list");
  for (int i = 0; i < n; i++)
    if (streams[i] < 0 || streams[i] >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": stream out of range");
  if (cfgs) {
    const int rc = check_stream_cfgs(ctx, pl->cfg, n, cfgs, streams, what);
    if (rc != FLVIS_OK) return rc;
  }
  if (n == 0) return FLVIS_OK;
  hipSetDevice(ctx->device);
  std::vector<char> named(pl->S, 0);
  std::vector<int> cfg_of(pl->S, -1);
  for (int i = 0; i < n; i++) named[streams[i]] = 1, cfg_of[streams[i]] = i;  // (duplicates: one reset, on the last entry's config)
  for (Lane* L : pl->lanes) {
    std::vector<std::pair<int, unsigned char>> todo;
    bool new_cmd = false;
    for (int ls = 0; ls < L->S; ls++) {
      if (!named[L->s0 + ls]) continue;
      // a command appended since the lane's last frame with nothing behind it already does what a second one would: a stream reset makes
      // it skip what is queued ahead of it, a local-map reset adds nothing
      const bool queued = L->cmd_frame[ls] == L->frames_uploaded;
      if (!tracker && queued) continue;
      unsigned char mode = (unsigned char)((tracker ? RS_TRACKER | RS_SKIP : 0) | (queued ? 0 : RS_CMD));
      if (!queued) {
        L->cmd_frame[ls] = L->frames_uploaded;
        new_cmd = true;
      }
      if (tracker) {
        L->h_nimu[ls] = 0;
        L->imu_read[ls] = 0;
      }
      todo.emplace_back(ls, mode);
    }
    if (todo.empty()) continue;
    if (new_cmd) {
      L->lmc_cmds++;
      // the command takes a queue entry: the back-pressure of a keyframe append, counting it (lane_backpressure_wait)
      if (L->cmd_steps.empty() || L->cmd_steps.back() != L->frames_uploaded) L->cmd_steps.push_back(L->frames_uploaded);
      L->cmd_since_frame = true;
      lane_backpressure_wait(pl, L, nullptr);
    }
    if (cfgs) {
      for (const auto& e : todo) {
        const int g = L->s0 + e.first;
        pl->cfgs[g] = cfgs[cfg_of[g]];
        rig_from_cfg(pl->cfgs[g], pl->rigs[g]);
        launch_set_rig(L->st, L->pipe, e.first, pl->rigs[g]);
      }
    }
    for (size_t b = 0; b < todo.size(); b += RESET_LIST) {
      ResetList rl{};
      rl.n = (int)std::min(todo.size() - b, (size_t)RESET_LIST);
      for (int i = 0; i < rl.n; i++) rl.s[i] = todo[b + i].first, rl.mode[i] = todo[b + i].second;
      launch_stream_reset(L->st, L->pipe, rl, L->d_progress + 3);
    }
    // the keyframe log of a stream that starts over is the old sequence's: emptied in order with the reset
    if (tracker && pl->kfl.cap > 0)
      for (const auto& e : todo) kf_log_reset_stream(pl, L, e.first);
    // the next frame's image ingest (detection stream) writes the slot k_stream_reset chose: it waits for a signal behind this launch, not
    // for the word the last k_frame_end stored
    L->endf_valid = false;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}

int flvis_reset_streams(flvis_ctx* ctx, int n, const int* streams) { return reset_impl(ctx, n, streams, true, "reset_streams"); }

int flvis_reset_streams_rigs(flvis_ctx* ctx, int n, const int* streams, const flvis_cfg* cfgs) {
  if (ctx && n > 0 && !cfgs) return ctx->fail(FLVIS_ERR_INVALID_ARG, "reset_streams_rigs: no configs");
  return reset_impl(ctx, n, streams, true, "reset_streams_rigs", cfgs);
}

int flvis_local_map_reset(flvis_ctx* ctx, int n, const int* streams) { return reset_impl(ctx, n, streams, false, "local_map_reset"); }

// ---- the local map's sparse map cloud: the record (include/flvis_hip.h; the kernels and the fetch are lm_cloud.hip's)
int flvis_local_map_cloud_enable(flvis_ctx* ctx, int64_t max_points) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (!pl) return ctx->fail(FLVIS_ERR_INVALID_ARG, "local_map_cloud_enable: no tracker (flvis_tracker_create)");
  if (max_points > (int64_t)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, "local_map_cloud_enable: max_points >= 2^31");
  hipSetDevice(ctx->device);
  sync_all(ctx);  // (no append kernel is in flight when its record goes away)
  lm_cloud_free(pl);
  if (max_points <= 0) return FLVIS_OK;
  const size_t S = (size_t)pl->S, cap = (size_t)max_points;
  LmCloudRec r{};
  r.cap = (long long)max_points;
  if (hipMalloc((void**)&r.hdr, sizeof(long long) * LMC_HDR * S) != hipSuccess || hipMalloc((void**)&r.ids, sizeof(long long) * S * cap) != hipSuccess ||
      hipMalloc((void**)&r.pts, sizeof(double) * 3 * S * cap) != hipSuccess) {
    (void)hipGetLastError();
    pl->lmc = r;
    lm_cloud_free(pl);
    return ctx->fail(FLVIS_ERR_HIP, "local_map_cloud_enable: device allocation failed");
  }
  pl->lmc = r;
  for (Lane* L : pl->lanes) launch_lm_cloud_init(ctx->stream, L->pipe, lane_lmc(pl, L), 0, L->S);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, "local_map_cloud_enable");
  return FLVIS_OK;
}

int flvis_local_map_cloud_clear(flvis_ctx* ctx, int n, const int* streams) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (!pl || pl->lmc.cap <= 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "local_map_cloud_clear: no tracker, or its record is off");
  if (n < 0 || (n > 0 && !streams)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "local_map_cloud_clear: bad stream list");
  for (int i = 0; i < n; i++)
    if (streams[i] < 0 || streams[i] >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "local_map_cloud_clear: stream out of range");
  if (n == 0) return FLVIS_OK;
  hipSetDevice(ctx->device);
  sync_all(ctx);
  for (int i = 0; i < n; i++) {
    int ls;
    Lane& L = pl->lane_of(streams[i], ls);
    launch_lm_cloud_init(ctx->stream, L.pipe, lane_lmc(pl, &L), ls, 1);
  }
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, "local_map_cloud_clear");
  return FLVIS_OK;
}

}  // extern "C"
namespace flvis {
// what == nullptr: the checks alone
int lm_cloud_settle(flvis_ctx* ctx, const char* what, LmCloudRec& rec, int& S) {
  Pipeline* pl = ctx->pipe;
  if (!pl || pl->lmc.cap <= 0) return FLVIS_ERR_INVALID_ARG;
  rec = pl->lmc;
  S = pl->S;
  if (!what) return FLVIS_OK;
  for (Lane* L : pl->lanes)
    if (L->ba_pending) launch_local_map(pl, L, J_FE, true, nullptr);  // (a launch deferred into the next frame: there is none)
  if (!pl->lmc_ev && hipEventCreateWithFlags(&pl->lmc_ev, Pipeline::ev_flags) != hipSuccess) return ctx->hip_fail(hipGetLastError(), what);
  // the context's stream behind the lanes' tracking streams (a reset's kernel) and the local-map streams (the workers, their append kernels)
  auto behind = [&](hipStream_t s) {
    if (!s || s == ctx->stream) return;
    hipEventRecord(pl->lmc_ev, s);
    hipStreamWaitEvent(ctx->stream, pl->lmc_ev, 0);
  };
  for (Lane* L : pl->lanes) behind(L->st);
  for (int k = 0; k < Pipeline::NBA; k++) behind(pl->ba_stream[k]);
  // what the last launches left unrecorded (a window that was owned when its append kernel looked), and a reset not yet applied
  for (Lane* L : pl->lanes) launch_lm_cloud_append(ctx->stream, L->pipe, lane_lmc(pl, L));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}
}  // namespace flvis
extern "C" {

int flvis_local_map_cloud_info(flvis_ctx* ctx, int stream, int64_t* h_info4) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  LmCloudRec rec{};
  int S = 0;
  if (!h_info4 || lm_cloud_settle(ctx, nullptr, rec, S) != FLVIS_OK || stream < 0 || stream >= S)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "local_map_cloud_info: no tracker, its record is off, or bad arguments");
  hipSetDevice(ctx->device);
  const int rc = lm_cloud_settle(ctx, "local_map_cloud_info", rec, S);
  if (rc != FLVIS_OK) return rc;
  long long h[LMC_HDR];
  hipError_t e = hipMemcpyAsync(h, rec.hdr + (size_t)stream * LMC_HDR, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, "local_map_cloud_info");
  h_info4[0] = h[LMC_POINTS], h_info4[1] = h[LMC_RUNS], h_info4[2] = h[LMC_DROPPED], h_info4[3] = rec.cap;
  return FLVIS_OK;
}

// test aid: the tracker's pyramid construction on its own (see include/flvis_hip.h for the layout of d_out)
int flvis_debug_pyramid(flvis_ctx* ctx, const uint8_t* d_src, int w, int h, int n_img, int levels, int bx, int by, int ingest, uint8_t* d_out,
                        size_t out_bytes) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!d_src || !d_out || w < 2 || h < 2 || (w & 3) || n_img <= 0 || levels < 1 || levels >= LK_MAX_LEVELS || bx < 0 || by < 0 || (bx & 15) ||
      ((uintptr_t)d_src & 3) || ((uintptr_t)d_out & 63))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "debug_pyramid: bad args (w % 4 == 0, 1 <= levels <= 5, bx % 16 == 0, d_out 64-byte aligned)");
  PyrSel q{};
  q.levels = levels;
  size_t off = 0;
  int lw = w, lh = h;
  for (int l = 0; l <= levels; l++) {
    q.w[l] = lw, q.h[l] = lh, q.bx[l] = bx, q.by[l] = by;
    q.pitch[l] = ((lw + 15) & ~15) + 2 * bx;
    q.stride[l] = (size_t)q.pitch[l] * (lh + 2 * by);
    q.lvl[l] = img_plain(d_out + off + (size_t)by * q.pitch[l] + bx);
    off += (q.stride[l] * n_img + 63) & ~(size_t)63;
    lw = (lw + 1) / 2, lh = (lh + 1) / 2;
  }
  if (off > out_bytes) return ctx->fail(FLVIS_ERR_CAPACITY, "debug_pyramid: d_out too small");
  const bool bordered = bx > 0 || by > 0;
  unsigned left = pyramid_levels(ctx->stream, bordered, img_plain(d_src), w, (size_t)w * h, ingest != 0, ingest != 0, q, n_img, nullptr);
  if (left) launch_pyr_border(ctx->stream, q, n_img, nullptr, left);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->fail(FLVIS_ERR_HIP, hipGetErrorString(e));
  return FLVIS_OK;
}

// measurement aid: from now on the tracker's two LK launches per frame count Gauss-Newton iterations and points per pyramid level
// (flvis_debug_counters [36 + 2 l], [37 + 2 l]: temporal LK, level l; [48 + 2 l], [49 + 2 l]: stereo LK); costs one atomic per point and level
int flvis_debug_lk_stats(flvis_ctx* ctx, int enable) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  ctx->pipe->lk_stats = enable != 0;
  return FLVIS_OK;
}

// sums over the lanes; [3] = keyframes dropped because a stream's queue was full (0 unless the back-pressure was defeated)
int flvis_debug_counters(flvis_ctx* ctx, int64_t* h64) {
  if (!ctx || !ctx->pipe || !h64) return FLVIS_ERR_INVALID_ARG;
  sync_all(ctx);
  for (int i = 0; i < 64; i++) h64[i] = 0;
  for (Lane* L : ctx->pipe->lanes) {
    long long c[64];
    hipMemcpy(c, L->pipe.counters, sizeof(c), hipMemcpyDeviceToHost);
    for (int i = 0; i < 64; i++) h64[i] = i == 25 ? std::max<int64_t>(h64[i], c[i]) : h64[i] + c[i];  // ([25] is a maximum)
  }
  return FLVIS_OK;
}

// Multi-lane trackers: how many later flvis_image_feed calls the caller leaves the input buffers of a call untouched (it cycles
// through n + 1 buffers).  0 (default): the context's stream waits for every lane to finish the frame before it goes on.
int flvis_set_input_hold(flvis_ctx* ctx, int n_frames) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  if (n_frames < 0 || n_frames >= Lane::HOLD_RING) return ctx->fail(FLVIS_ERR_INVALID_ARG, "set_input_hold: 0 .. 7 frames");
  ctx->pipe->input_hold = n_frames;
  return FLVIS_OK;
}
// Tuning aid: host milliseconds spent inside flvis_image_feed since the tracker was created, [0] in total, [1] of it blocked on
// the pinned upload ring (the host running PIN_RING frames ahead of the GPU), [2] calls.
int flvis_debug_host_times(flvis_ctx* ctx, double* h_out3) {
  if (!ctx || !ctx->pipe || !h_out3) return FLVIS_ERR_INVALID_ARG;
  h_out3[0] = ctx->pipe->host_ms_total;
  h_out3[1] = ctx->pipe->host_ms_wait;
  h_out3[2] = (double)ctx->pipe->frames_fed;
  return FLVIS_OK;
}
// ... of flvis_image_feed_host: [0] blocked on the previous call's uploads, [1] issuing this call's uploads, [2] inside flvis_image_feed
// (whose share blocked on the host lead is flvis_debug_host_times [1]), [3] calls
int flvis_debug_host_feed_times(flvis_ctx* ctx, double* h_out4) {
  if (!ctx || !ctx->pipe || !h_out4) return FLVIS_ERR_INVALID_ARG;
  const Pipeline::HostFeed& hf = ctx->pipe->hf;
  h_out4[0] = hf.ms_wait_uploads, h_out4[1] = hf.ms_issue, h_out4[2] = hf.ms_feed, h_out4[3] = (double)hf.n;
  return FLVIS_OK;
}

int flvis_debug_host_feed_timing(flvis_ctx* ctx, int enable, double* h_out3) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  Pipeline::HostFeed& hf = ctx->pipe->hf;
  if (enable >= 0) hf.timing = enable != 0;
  if (h_out3) h_out3[0] = hf.up_ms, h_out3[1] = hf.up_bytes, h_out3[2] = hf.up_calls;
  return FLVIS_OK;
}

// IMU rotation factor of the window BA (an addition: the reference's window holds reprojection edges only).  Off by default.
int flvis_set_imu_factor(flvis_ctx* ctx, int enable, double sigma_gyro) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  if (enable && !(sigma_gyro > 0)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "set_imu_factor: sigma_gyro must be positive");
  sync_all(ctx);  // the flag travels in the kernel arguments of the next local-map launch
  for (Lane* L : ctx->pipe->lanes) {
    L->pipe.imu_factor = enable ? 1 : 0;
    L->pipe.imu_sigma_g = sigma_gyro;
  }
  return FLVIS_OK;
}

// Position rows of the factor on top of the rotation rows (flvis_set_imu_factor must be on): sigma_acc = accelerometer noise density
// [m/s^2/sqrt(Hz)], information I3 / (sigma_acc^2 dt^3 / 3); <= 0 switches the position rows off again.
int flvis_set_imu_factor_accel(flvis_ctx* ctx, double sigma_acc) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  sync_all(ctx);
  for (Lane* L : ctx->pipe->lanes) L->pipe.imu_sigma_a = sigma_acc > 0 ? sigma_acc : 0.0;
  return FLVIS_OK;
}

// the position part of the last keyframe's preintegration (flvis_get_keyframe_imu gives the rotation part and says whether it links)
int flvis_get_keyframe_imu_pos(flvis_ctx* ctx, int stream, double* dp3, double* va3) {
  if (!ctx || !ctx->pipe || !dp3 || !va3) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  sync_all(ctx);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  unsigned tl = 0;
  hipMemcpy(&tl, L.pipe.kfq_kf + ls, sizeof(unsigned), hipMemcpyDeviceToHost);
  if (tl == 0) return 0;
  double h[6];
  static_assert(offsetof(KeyFrameDev, imu_va) == offsetof(KeyFrameDev, imu_dp) + 24, "KeyFrameDev imu position block layout");
  const char* src = reinterpret_cast<const char*>(L.pipe.kfq + (size_t)ls * KFQ + ((tl - 1) % KFQ)) + offsetof(KeyFrameDev, imu_dp);
  if (hipMemcpy(h, src, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return ctx->fail(FLVIS_ERR_HIP, "get_keyframe_imu_pos");
  memcpy(dp3, h, 24);
  memcpy(va3, h + 3, 24);
  return 1;
}

int flvis_get_keyframe_imu(flvis_ctx* ctx, int stream, double* dq_wxyz, double* dt) {
  if (!ctx || !ctx->pipe || !dq_wxyz || !dt) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  sync_all(ctx);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  FrameOut fo;
  hipMemcpy(&fo, L.pipe.out + ls, sizeof(FrameOut), hipMemcpyDeviceToHost);
  unsigned tl = 0;
  hipMemcpy(&tl, L.pipe.kfq_kf + ls, sizeof(unsigned), hipMemcpyDeviceToHost);
  if (!fo.new_keyframe || tl == 0) return 0;
  struct {
    double dq[4], dt;
    int valid, pad;
  } h;
  static_assert(offsetof(KeyFrameDev, imu_valid) == offsetof(KeyFrameDev, imu_dq) + 40, "KeyFrameDev imu block layout");
  const char* src = reinterpret_cast<const char*>(L.pipe.kfq + (size_t)ls * KFQ + ((tl - 1) % KFQ)) + offsetof(KeyFrameDev, imu_dq);
  hipMemcpy(&h, src, sizeof(h), hipMemcpyDeviceToHost);
  memcpy(dq_wxyz, h.dq, 32);
  *dt = h.dt;
  return h.valid ? 1 : 0;
}

static int ba_push_impl(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T7, const double* imu_dq, double imu_dt,
                        int lm_count, const int64_t* h_id, const double* h_2d, const double* h_3d, int cap, int64_t* out_frame_id,
                        double* out_T7, int* out_lm_count, int64_t* out_lm_id, double* out_lm_3d, int* out_oc, int64_t* out_oid,
                        const double* imu_dp = nullptr, const double* imu_va = nullptr);

int flvis_ba_push_keyframe(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T7, int lm_count, const int64_t* h_id,
                           const double* h_2d, const double* h_3d, int cap, int64_t* out_frame_id, double* out_T7,
                           int* out_lm_count, int64_t* out_lm_id, double* out_lm_3d, int* out_oc, int64_t* out_oid) {
  return ba_push_impl(ctx, stream, frame_id, T7, nullptr, 0.0, lm_count, h_id, h_2d, h_3d, cap, out_frame_id, out_T7, out_lm_count,
                      out_lm_id, out_lm_3d, out_oc, out_oid);
}
int flvis_ba_push_keyframe_imu(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T7, const double* imu_dq_wxyz,
                               double imu_dt, int lm_count, const int64_t* h_id, const double* h_2d, const double* h_3d, int cap,
                               int64_t* out_frame_id, double* out_T7, int* out_lm_count, int64_t* out_lm_id, double* out_lm_3d,
                               int* out_oc, int64_t* out_oid) {
  return ba_push_impl(ctx, stream, frame_id, T7, imu_dq_wxyz, imu_dt, lm_count, h_id, h_2d, h_3d, cap, out_frame_id, out_T7,
                      out_lm_count, out_lm_id, out_lm_3d, out_oc, out_oid);
}

int flvis_ba_push_keyframe_imu_pos(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T7, const double* imu_dq_wxyz,
                                   double imu_dt, const double* imu_dp3, const double* imu_va3, int lm_count, const int64_t* h_id,
                                   const double* h_2d, const double* h_3d, int cap, int64_t* out_frame_id, double* out_T7,
                                   int* out_lm_count, int64_t* out_lm_id, double* out_lm_3d, int* out_oc, int64_t* out_oid) {
  return ba_push_impl(ctx, stream, frame_id, T7, imu_dq_wxyz, imu_dt, lm_count, h_id, h_2d, h_3d, cap, out_frame_id, out_T7,
                      out_lm_count, out_lm_id, out_lm_3d, out_oc, out_oid, imu_dp3, imu_va3);
}

static int ba_push_impl(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T7, const double* imu_dq, double imu_dt,
                        int lm_count, const int64_t* h_id, const double* h_2d, const double* h_3d, int cap, int64_t* out_frame_id,
                        double* out_T7, int* out_lm_count, int64_t* out_lm_id, double* out_lm_3d, int* out_oc, int64_t* out_oid,
                        const double* imu_dp, const double* imu_va) {
  if (!ctx || !ctx->pipe || !T7 || lm_count < 0 || lm_count > KF_MAXLM) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  std::vector<KeyFrameDev> kfv(1);
  KeyFrameDev& kf = kfv[0];
  memset(&kf, 0, sizeof(kf));
  kf.frame_id = frame_id;
  kf.lm_count = lm_count;
  kf.valid = 1;
  memcpy(kf.T_c_w, T7, 56);
  {  // the stream's rig, as k_frame_end gives it to the keyframes it makes
    const RigParams& r = pl->rigs[stream];
    kf.rig_K[0] = r.fx, kf.rig_K[1] = r.fy, kf.rig_K[2] = r.cx, kf.rig_K[3] = r.cy;
    memcpy(kf.rig_T_c_i, r.T_c_i, 56);
  }
  kf.imu_dq[0] = 1.0;
  if (imu_dq && imu_dt > 0) {
    memcpy(kf.imu_dq, imu_dq, 32);
    kf.imu_dt = imu_dt;
    kf.imu_valid = 1;
    if (imu_dp && imu_va) {
      memcpy(kf.imu_dp, imu_dp, 24);
      memcpy(kf.imu_va, imu_va, 24);
    }
  }
  for (int i = 0; i < lm_count; i++) {
    kf.lm_id[i] = h_id[i];
    kf.lm_2d[i][0] = h_2d[2 * i];
    kf.lm_2d[i][1] = h_2d[2 * i + 1];
    for (int j = 0; j < 3; j++) kf.lm_3d[i][j] = h_3d[3 * i + j];
  }
  sync_all(ctx);
  const int zero = 0;
  unsigned tl = 0;
  hipMemcpy(&tl, L.pipe.kfq_tail + ls, sizeof(unsigned), hipMemcpyDeviceToHost);
  hipMemcpy(L.pipe.kfq + (size_t)ls * KFQ + (tl % KFQ), &kf, sizeof(kf), hipMemcpyHostToDevice);
  tl++;
  hipMemcpy(L.pipe.kfq_tail + ls, &tl, sizeof(unsigned), hipMemcpyHostToDevice);
  L.cmd_frame[ls] = -1;  // (a reset command queued before this keyframe is no longer the last entry)
  hipMemcpy(L.pipe.kfq_kf + ls, &tl, sizeof(unsigned), hipMemcpyHostToDevice);
  hipMemcpy(&L.pipe.corr[ls].valid, &zero, sizeof(int), hipMemcpyHostToDevice);
  local_map_work(pl, &L, pl->ba_stream[0], 1, nullptr);
  hipError_t e = hipStreamSynchronize(pl->ba_stream[0]);
  if (e != hipSuccess) return ctx->hip_fail(e, "ba_push_keyframe");
  sync_all(ctx);
  return read_correction(L, ls, cap, out_frame_id, out_T7, out_lm_count, out_lm_id, out_lm_3d, out_oc, out_oid);
}

// F2FTracking::correction_feed (src/frontend/f2f_tracking.cpp:40-44) -- the sink the reference's
// correction_feedback_callback (vo_tracking.cpp:373-385) unpacks for and never calls.  Opt-in: nothing changes for a
// caller that never feeds a correction.  Applied at the stream's next Tracking frame (f2f_tracking.cpp:189-219).
int flvis_correction_feed(flvis_ctx* ctx, int stream, int64_t frame_id, const double* T_c_w7, int lm_count,
                          const int64_t* h_lm_id, const double* h_lm_3d, int lm_outlier_count,
                          const int64_t* h_lm_outlier_id) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S || !T_c_w7 || lm_count < 0 || lm_outlier_count < 0 || (lm_count && (!h_lm_id || !h_lm_3d)) ||
      (lm_outlier_count && !h_lm_outlier_id))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "correction_feed: bad args");
  if (lm_count > BA_LMAX || lm_outlier_count > BA_EMAX) return ctx->fail(FLVIS_ERR_CAPACITY, "correction_feed: too many entries");
  hipSetDevice(ctx->device);
  if (!pl->feedback_used) {
    for (Lane* L : pl->lanes) {
      hipStreamSynchronize(L->st);
      L->pipe.corr_in = dalloc<CorrectionDev>(L->allocs, L->S);
      if (!L->pipe.corr_in) return ctx->fail(FLVIS_ERR_HIP, "correction_feed: device allocation failed");
    }
  }
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  hipStream_t st = L.st;
  // the previous frame may still be running and reads/clears the slot: order the upload after it on the same stream
  CorrectionDev* d = L.pipe.corr_in + ls;
  struct Head {
    long long frame_id;
    int lm_count, lm_outlier_count, valid, pad;
    double T_c_w[7];
  } hd;
  static_assert(offsetof(CorrectionDev, lm_id) == sizeof(Head), "CorrectionDev header layout");
  hd.frame_id = frame_id;
  hd.lm_count = lm_count;
  hd.lm_outlier_count = lm_outlier_count;
  hd.valid = 1;
  hd.pad = 0;
  for (int j = 0; j < 7; j++) hd.T_c_w[j] = T_c_w7[j];
  hipError_t e = hipSuccess;
  if (lm_count) {
    e = hipMemcpyAsync(d->lm_id, h_lm_id, sizeof(int64_t) * lm_count, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d->lm_3d, h_lm_3d, sizeof(double) * 3 * lm_count, hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess && lm_outlier_count)
    e = hipMemcpyAsync(d->lm_outlier_id, h_lm_outlier_id, sizeof(int64_t) * lm_outlier_count, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d, &hd, sizeof(hd), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the caller's buffers and `hd` may go away after return
  if (e != hipSuccess) return ctx->hip_fail(e, "correction_feed");
  pl->feedback_used = true;
  return FLVIS_OK;
}

// stage poses of a stream's last Tracking frame (test aid): pose7 right after PnP-RANSAC, pose7 after the pose-only LM
int flvis_debug_stage_poses(flvis_ctx* ctx, int stream, double* h_out21) {
  if (!ctx || !ctx->pipe || !h_out21) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "bad stream");
  sync_all(ctx);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  StreamState st;
  hipMemcpy(&st, L.pipe.st + ls, sizeof(st), hipMemcpyDeviceToHost);
  memcpy(h_out21, st.dbg_T_pnp, 56);
  memcpy(h_out21 + 7, st.dbg_T_lm, 56);
  memcpy(h_out21 + 14, st.dbg_T_pre, 56);
  return FLVIS_OK;
}

// pose_records of a stream (f2f_tracking.h:59), oldest first: rows (frame_id, tx ty tz qx qy qz qw); returns the count
int flvis_get_pose_records(flvis_ctx* ctx, int stream, int cap, double* h_rows8) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S || cap < 0 || (cap && !h_rows8)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "get_pose_records: bad args");
  hipSetDevice(ctx->device);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  hipStreamSynchronize(ctx->stream);
  hipStreamSynchronize(L.st);
  StreamState st;
  std::vector<int> ids(POSE_REC);
  std::vector<double> T((size_t)POSE_REC * 7);
  if (hipMemcpy(&st, L.pipe.st + ls, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(ids.data(), L.pipe.rec_id + (size_t)ls * POSE_REC, sizeof(int) * POSE_REC, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(T.data(), L.pipe.rec_T + (size_t)ls * POSE_REC * 7, sizeof(double) * 7 * POSE_REC, hipMemcpyDeviceToHost) != hipSuccess)
    return ctx->fail(FLVIS_ERR_HIP, "get_pose_records: copy failed");
  for (int i = 0; i < st.rec_count && i < cap; i++) {
    const int k = (st.rec_head + i) % POSE_REC;
    h_rows8[8 * i] = (double)ids[k];
    for (int j = 0; j < 7; j++) h_rows8[8 * i + 1 + j] = T[(size_t)k * 7 + j];
  }
  return st.rec_count;
}

// the visual-inertial filter of a stream (test aid): VIMOTION's `states` oldest first as rows (t, qw qx qy qz, pos, vel), its two
// biases and (has_imu, vi_first, vi_initialized, vi_count); staged samples are integrated first (as flvis_get_imu_states does).
// Returns the count.
int flvis_debug_vi_state(flvis_ctx* ctx, int stream, int cap, double* h_rows11, double* h_biases6, int* h_flags4) {
  if (!ctx || !ctx->pipe) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (stream < 0 || stream >= pl->S || cap < 0 || (cap && !h_rows11)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "debug_vi_state: bad args");
  hipSetDevice(ctx->device);
  sync_all(ctx);
  int ls;
  Lane& L = pl->lane_of(stream, ls);
  bool staged = false;
  for (int s = 0; s < L.S; s++) staged = staged || L.h_nimu[s] > 0;
  if (staged) {
    const int rc = lane_flush_imu(ctx, L);
    if (rc != FLVIS_OK) return rc;
  }
  StreamState st;
  std::vector<MotionState> ring(VI_QUEUE);
  if (hipMemcpy(&st, L.pipe.st + ls, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(ring.data(), L.pipe.vi + (size_t)ls * VI_QUEUE, sizeof(MotionState) * VI_QUEUE, hipMemcpyDeviceToHost) != hipSuccess)
    return ctx->fail(FLVIS_ERR_HIP, "debug_vi_state: copy failed");
  if (st.vi_count < 0 || st.vi_count > VI_QUEUE || st.vi_head < 0 || st.vi_head >= VI_QUEUE)
    return ctx->fail(FLVIS_ERR_HIP, "debug_vi_state: ring cursor out of range");
  for (int i = 0; i < st.vi_count && i < cap; i++) {
    const MotionState& m = ring[(st.vi_head + i) % VI_QUEUE];
    double* r = h_rows11 + (size_t)11 * i;
    r[0] = m.t;
    memcpy(r + 1, m.q, 32);
    memcpy(r + 5, m.pos, 24);
    memcpy(r + 8, m.vel, 24);
  }
  if (h_biases6) {
    memcpy(h_biases6, st.acc_bias, 24);
    memcpy(h_biases6 + 3, st.gyro_bias, 24);
  }
  if (h_flags4) h_flags4[0] = st.has_imu, h_flags4[1] = st.vi_first, h_flags4[2] = st.vi_initialized, h_flags4[3] = st.vi_count;
  return st.vi_count;
}

}  // extern "C"
