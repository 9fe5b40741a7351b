// flvis_amd: device-resident state of the batched front-end (F2FTracking mirror) and local map (LocalMap mirror).
//
// One context tracks S independent streams.  All per-stream state lives in HBM; the host only enqueues a fixed
// sequence of kernels per frame step (no host round trip unless the caller asks for outputs), every kernel masks
// itself by the stream's state machine flags.  Reference anchors: src/frontend/f2f_tracking.cpp (state machine),
// src/processing/camera_frame.cpp / landmark.cpp (frame + landmark records), src/processing/vi_motion.cpp (IMU filter),
// src/backend/vo_localmap.cpp + poselmbag.cpp (sliding window).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "img_kernels.hpp"

namespace flvis {

constexpr int NMAX = 1024;        // landmark capacity per stream and frame slot
constexpr int IMU_MAX = 64;       // IMU samples accepted per stream between two frames
constexpr int IMU_OUT_CAP = 512;  // rows of the per-stream ring behind F2FTracking::imu_feed's outputs (flvis_get_imu_states)
constexpr int VI_QUEUE = 400;     // STATES_QUEUE_SIZE (src/processing/include/vi_motion.h:10)
constexpr int KF_MAXLM = 1024;    // landmarks per keyframe payload
constexpr int KFQ = 32;            // per-stream keyframe queue between the tracker and the local map (48 KB per entry)
constexpr int BA_WMAX = 16;       // window sizes supported by the LDS-resident solver
constexpr int BA_LMAX = 4096;     // landmarks in the window
constexpr int BA_EMAX = 8192;     // observations (edges) in the window
// WindowDev::overflow: which capacity a window exceeded (published to the host once, flvis_hip_synchronize reports it)
constexpr int BA_OVF_LMAX = 1;   // more than BA_LMAX landmarks
constexpr int BA_OVF_EMAX = 2;   // more than BA_EMAX observations
constexpr int BA_OVF_CHUNK = 4;  // the Schur phase's chunk table (BA_MAXCHUNK entries) could not hold the window
constexpr int POSE_REC = 1024;    // ring behind F2FTracking::pose_records (the reference keeps < 1000, f2f_tracking.cpp:334)

enum { ST_UNINIT = 0, ST_TRACKING = 1, ST_TRACKFAIL = 2 };
enum { PH_IDLE = 0, PH_TRACK = 1, PH_INIT = 2 };
enum { CAM_STEREO_RECT = 0, CAM_STEREO_UNRECT = 1, CAM_DEPTH = 2 };  // enum TYPEOFCAMERA (depth_camera.h:6-9)

// LandMarkInFrame (src/processing/include/landmark.h:8-35), AoS so that a frame-to-frame copy is one record move
struct Landmark {
  long long id;
  double p3w[3];
  double p2d[2];
  double p2u[2];
  double p3c[3];
  double first2d[2];
  double first_pose[7];  // tx ty tz qx qy qz qw
  unsigned char has3d, inlier;
  short tslot;  // slot of the LK template cache that holds this landmark's templates at p2d in its frame's left image (k_depth_seeds), -1: none
  unsigned char pad[4];
};
static_assert(sizeof(Landmark) == 21 * 8, "Landmark layout");

struct MotionState {  // MOTION_STATE (vi_motion.h:12-17)
  double pos[3], vel[3], q[4] /*w x y z*/, acc[3], gyro[3], t;
};

// The batch-wide part of a tracker's configuration: what sizes buffers, sets the launch geometry or picks a code path.  Every stream
// of a tracker shares it (flvis_tracker_create_rigs checks that every stream's config agrees on it).
struct CamParams {
  int cam_type, w, h;
  int need_equal_hist, skip_first_n;
  DemParams dem;
  int gftt_num;
  double gftt_ql;
  int gftt_dis;
  int window;
  unsigned long long seed;
};

// The per-stream part: one camera's calibration and the tuning that goes with it (Pipe::rig, one per stream).  Built from a stream's
// flvis_cfg by rig_from_cfg (pipeline.cpp), at tracker creation and at flvis_reset_streams_rigs.
struct RigParams {
  double fx, fy, cx, cy;  // rectified (from P0)
  double K0[4], D0[4], K1[4], D1[4];
  double R0[9], R1[9], P0[12], P1[12];
  double T_c1_c0[7];  // pose7
  double T_i_c[7], T_c_i[7];
  double depth_scale;  // DEPTH_D435: cam_scale_factor (Z16 units per metre)
  double vi_para[4];
  float iir_ratio, range;
  int enable_dummy, pad;
};
static_assert(sizeof(RigParams) % 8 == 0, "RigParams layout");
// a stream's rig as the kernels see it (rig_of, track_kernels.hpp)
#define FLVIS_CONST_AS __attribute__((address_space(4)))
typedef const FLVIS_CONST_AS RigParams CRig;
// a rig array as a value in registers, for the helpers that take plain pointers
template <int N>
struct RigArr {
  double v[N];
};
template <int N>
__device__ inline RigArr<N> rig_arr(const FLVIS_CONST_AS double (&a)[N]) {
  RigArr<N> r;
#pragma unroll
  for (int i = 0; i < N; i++) r.v[i] = a[i];
  return r;
}

struct StreamState {
  int state, phase, ok, cur;
  int skip_n, has_imu, cont_fail, tf_cnt;
  long long frameCount, lm_id_counter;
  int n_lm[2];
  long long frame_id[2];
  double frame_time[2];
  double T_c_w[2][7];
  double T_kf[7];
  int use_guess;
  double guess[7];
  int new_kf, reset_cmd;
  int n_surv, of_cnt, f_cnt, pnp_cnt;
  int orig_size, n_new;
  double reproj_err;
  int rnd_r[34], rnd_pos;
  // VIMOTION scalars
  int vi_initialized, vi_first, vi_head, vi_count;  // ring: oldest at head, count entries
  double acc_bias[3], gyro_bias[3];
  // local map
  int lm_state;  // 0 UN_INITIALIZED, 1 SLIDING_WINDOW
  int kf_pending;
  // pose_records (f2f_tracking.h:59, ID_POSE): ring in Pipe::rec_id / rec_T, oldest at rec_head
  int rec_head, rec_count;
  double dbg_T_pnp[7], dbg_T_lm[7], dbg_T_pre[7];  // pose right after PnP-RANSAC / after the pose LM of the last Tracking frame (tests)
  double kf_dq[4], kf_dt;  // gyro rotation preintegration since the last keyframe (w, x, y, z), see KeyFrameDev::imu_dq
  int feeds;  // image_feed calls seen by this stream (= row of the device-side trajectory the frame is recorded in)
  // position / velocity preintegration of the bias-corrected accelerometer samples since the last keyframe (body frame of that keyframe)
  // and the filter's body velocity (world) when that keyframe was made: inputs of the IMU factor's position rows
  double kf_dp[3], kf_dv[3], kf_va[3];
  long long imu_seen;  // IMU samples integrated so far (= rows ever written to the stream's IMU-state output ring)
  int vi_corr_due;     // k_reproj_filter: this Tracking frame's viCorrectionFromVision is still to run (k_vi_correction)
  int pad_vi;
};

struct FrameOut {  // per stream, per image_feed
  int state, new_keyframe, reset_cmd, n_landmarks;
  long long frame_id;
  double T_c_w[7];
  int of_cnt, f_cnt, pnp_cnt, pad;
  double reproj_err;
};

// KeyFrame payload (msg/KeyFrame.msg without the images): what KeyFrameMsg::pub packs (src/utils/keyframe_msg.cpp:30-124)
struct KeyFrameDev {
  long long frame_id;
  int lm_count, valid;
  double T_c_w[7];
  double stamp;  // header.stamp of the message: the frame's image time
  // (addition, not in KeyFrame.msg) gyro rotation preintegration since the previous keyframe of the chain: dq (w, x, y, z) =
  // R_body(previous)^T R_body(this) as integrated from the bias-corrected gyro samples, over imu_dt seconds
  double imu_dq[4], imu_dt;
  int imu_valid, imu_pad;
  // ... with the position part: dp = preintegrated body displacement over the same interval (body frame of the previous keyframe),
  // va = the filter's body velocity (world frame) when the previous keyframe was made
  double imu_dp[3], imu_va[3];
  // (addition) the intrinsics (fx, fy, cx, cy) and the camera-from-IMU pose7 of the rig the keyframe was made with: the local map's
  // optimisation of the stream's window reads them (WindowDev::K)
  double rig_K[4], rig_T_c_i[7];
  long long lm_id[KF_MAXLM];
  double lm_2d[KF_MAXLM][2];
  double lm_3d[KF_MAXLM][3];
};

// CorrectionInf (msg/CorrectionInf.msg)
struct CorrectionDev {
  long long frame_id;
  int lm_count, lm_outlier_count, valid, pad;
  double T_c_w[7];
  long long lm_id[BA_LMAX];
  double lm_3d[BA_LMAX][3];
  long long lm_outlier_id[BA_EMAX];
};

// sliding-window graph of one stream (PoseLMBag + the g2o graph the callback maintains)
struct WindowDev {
  // PoseLMBag
  int newest, oldest, wp_init, initialized;
  long long pose_frame_id[BA_WMAX];
  double bag_pose[BA_WMAX][7];
  int n_lm;
  long long lm_id[BA_LMAX];
  int lm_count[BA_LMAX];
  double lm_p3d[BA_LMAX][3];  // bag's p3d_w (running mean during init / first seen)
  // graph
  double pose_est[BA_WMAX][7];
  int pose_fixed[BA_WMAX], pose_present[BA_WMAX];
  double lm_est[BA_LMAX][3];  // vertex estimate, parallel to lm_id (vertex exists iff bag entry exists)
  int n_edge;
  long long edge_next_id;
  long long e_id[BA_EMAX];
  long long e_lm[BA_EMAX];  // landmark id
  int e_pose[BA_EMAX];
  int e_lidx[BA_EMAX];  // index of e_lm in the bag arrays (kept consistent across bag compaction)
  double e_uv[BA_EMAX][2];
  // IMU rotation factor (optional): the preintegration that links ring slot j to its predecessor (j - 1 + W) % W
  double imu_dq[BA_WMAX][4], imu_dt[BA_WMAX];
  int imu_has[BA_WMAX];
  double imu_dp[BA_WMAX][3], imu_va[BA_WMAX][3];
  // keyframe queue (the `kfs` deque of vo_localmap.cpp:55): ring of the last `window` payloads, storage in Pipe::kfs_ring
  int kfs_head, kfs_size;
  int solve;        // set by the bookkeeping kernel when this keyframe triggers an optimisation
  int overflow;     // a capacity was exceeded (BA_OVF_* bits); the window stops accepting work until the stream's local map is reset
  long long ba_runs;
  // the rig of the window's keyframes (KeyFrameDev::rig_K / rig_T_c_i of the last one added): what its optimisation projects with
  double K[4], T_c_i[7];
};

// KeyFrameDev::valid of a keyframe queue entry: a keyframe, or KFMSG_CMD_RESET_LM (keyframe_msg.h:11) -- the local map empties its window
// when it reaches the entry, in order with the keyframes (flvis_local_map_reset, flvis_reset_streams)
enum { KFQ_KEYFRAME = 1, KFQ_CMD_RESET = 2 };

// host helpers shared by the tracker set-up and the one-call entry points (pipeline.cpp)
void pose7_from_mat44(const double* m44, double* out7, bool inverse);
}  // namespace flvis
struct flvis_cfg;
namespace flvis {
void rig_from_cfg(const flvis_cfg& cfg, RigParams& r);  // a stream's rig from its finalized config

// the state srand(s) leaves: the last 34 words of glibc's TYPE_3 table (r[i] = r[i - 31] + r[i - 3] over 344 words, kept in a ring of 34)
__host__ __device__ inline void glibc_seed(unsigned s, int* r34) {
  int v[34];
  v[0] = (int)s;
  for (int i = 1; i < 31; i++) {
    long long w = (16807LL * v[i - 1]) % 2147483647;
    if (w < 0) w += 2147483647;
    v[i] = (int)w;
  }
  for (int i = 31; i < 34; i++) v[i] = v[i - 31];
  for (int i = 34; i < 344; i++) v[i % 34] = (int)((unsigned)v[(i - 31) % 34] + (unsigned)v[(i - 3) % 34]);
  for (int i = 0; i < 34; i++) r34[i] = v[(344 - 34 + i) % 34];
}

// The state of a stream that has seen nothing (F2FTracking::init + the VIMOTION ctor, f2f_tracking.cpp:5-38: landmark id counter 100,
// glibc rand seeded with 1, skip_first_n_imgs to skip).  Written by k_stream_reset, at tracker creation and at flvis_reset_streams.
__host__ __device__ inline void stream_state_init(StreamState& st, int skip_first_n) {
  int* w = reinterpret_cast<int*>(&st);
  for (int i = 0; i < (int)(sizeof(StreamState) / sizeof(int)); i++) w[i] = 0;
  st.state = ST_UNINIT;
  st.cur = 0;
  st.skip_n = skip_first_n;
  st.lm_id_counter = 100;
  st.vi_first = 1;
  st.kf_dq[0] = 1.0;
  for (int k = 0; k < 2; k++) st.T_c_w[k][6] = 1.0;
  st.T_kf[6] = 1.0;
  st.guess[6] = 1.0;
  glibc_seed(1, st.rnd_r);
  st.rnd_pos = 0;
}

}  // namespace flvis
