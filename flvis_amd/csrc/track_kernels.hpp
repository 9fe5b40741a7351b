// flvis_amd: kernel-argument bundle and launch prototypes of the batched front-end / local-map kernels.
#pragma once
#include "pipeline.hpp"

namespace flvis {

constexpr int NEW_MAX = 1024;  // capacity of FeatureDEM's output per stream and frame

struct Pipe {
  int S;
  CamParams cam;            // batch-wide
  const RigParams* rig;     // [S] each stream's calibration (rig_of)
  StreamState* st;          // [S]
  Landmark* lm;             // [2][S][NMAX]
  MotionState* vi;          // [S][VI_QUEUE]
  const unsigned long long* seeds;  // [S] RANSAC seeds
  double* imu_in;           // [S][IMU_MAX][7]  (t, acc, gyro) in the FLVIS IMU frame
  int* n_imu;               // [S]
  const int* present;       // [S] this step's presence (flvis_image_feed_present): 0 = the stream has no frame in it; nullptr: all present
  double* imu_out;          // [S][IMU_OUT_CAP][11]  F2FTracking::imu_feed's outputs per sample: (t, q_w_i wxyz, pos_w_i, vel_w_i)
  float* prev_pts;          // [S][NMAX][2]
  float* next_pts;          // [S][NMAX][2]
  uint8_t* lk_status;       // [S][NMAX]
  int* lk_count;            // [S]
  int* lk_slot;             // [S][NMAX] temporal LK: template-cache slot of each previous point (Landmark::tslot), -1: none
  long long* lk_tag;        // [S] identity of the LK launch's template image (frame id of the stream's current / last frame)
  int tc_cap;               // slots per stream of the lane's template cache (0: no cache)
  const uint32_t* tc;       // the cache itself (k_track_prepare compares the slot headers) and its slot size in dwords
  int tc_stride;
  float* m1;                // [S][NMAX][2]  F-RANSAC inputs (ascending survivors)
  float* m2;
  double* tri;              // [S][NMAX][3]
  uint8_t* tri_mask;        // [S][NMAX]
  float* new_xy;            // [S][NEW_MAX][2]
  int* n_new;               // [S]
  double* exist_xy;         // [S][NMAX][2]
  int* n_exist;             // [S]
  int* act_img;             // [S]
  int* act_track;           // [S]
  int* det_mode;            // [S] 0 none, 1 detect (init), 2 redetect
  int* det_maxc;            // [S]
  int* gftt_act;            // [S] corner detection planned at frame begin (init frames; tracking frames speculatively)
  int* gftt_maxc;           // [S] its maxCorners
  int* img_slot;            // [S] image slot of the current frame
  int* img_slot_in;         // [S] image slot the NEXT frame's left image is written to (k_frame_end; known before k_frame_head runs)
  FrameOut* out;            // [S]
  double* traj;             // [S][traj_cap][9]  (t, pose7, state|kf<<4) or nullptr
  int traj_cap;
  // keyframe queue tracker -> local map (the `/vo_kf` topic of the reference): frame_end appends, the local-map worker
  // consumes at its own pace (monotonic counters, slot = counter % KFQ)
  KeyFrameDev* kfq;         // [S][KFQ]
  unsigned* kfq_tail;       // [S] keyframes produced
  unsigned* kfq_head;       // [S] keyframes consumed
  // reset commands in the queue (k_stream_reset): the entry index + 1 of the stream's last command (0: none), the entries the local map
  // discards unread (index < kfq_skip: queued ahead of a flvis_reset_streams), and the tail behind the last command (the keyframes the
  // stream has emitted since its last reset are kfq_tail - kfq_base, flvis_get_local_map_counts)
  unsigned* kfq_cmd;        // [S]
  unsigned* kfq_skip;       // [S]
  unsigned* kfq_base;       // [S]
  unsigned* kfq_kf;         // [S] entry index + 1 of the stream's last keyframe (0: none since creation or its last flvis_reset_streams): the
                            // keyframe getters read it, the last entry may be a command
  int* ba_busy;             // [S] a worker workgroup owns the stream's window
  // local map
  WindowDev* win;           // [S]
  KeyFrameDev* kfs_ring;    // [S][BA_WMAX]
  CorrectionDev* corr;      // [S]
  double* ba_scratch;       // [S][ba_scratch_stride]
  size_t ba_scratch_stride;
  int imu_factor;          // window BA: add the gyro rotation-preintegration edge between consecutive keyframes (off by default)
  double imu_sigma_a;      // accelerometer noise density [m/s^2/sqrt(Hz)] of the factor's position rows (information 1 / (sigma_a^2 dt^3 / 3)); <= 0: rotation rows only
  double imu_sigma_g;      // its gyro noise density [rad/s/sqrt(Hz)]: information = 1 / (sigma_g^2 dt)
  int ba_lds_bytes;         // dynamic LDS of a k_ba_worker workgroup: what it leaves of a CU's 160 KB is there for the tracker's waves
  int ba_drain;             // keyframes a local-map workgroup takes from its stream's queue per launch (0: until the queue is empty) ...
  int ba_backlog;           // ... and it goes on while the queue still holds this many or more: the bound the back-pressure relies on
  // FLVIS_PNP_TAIL=cv: the final solve of solvePnPRansac(ITERATIVE) as OpenCV runs it (DLT start + CvLevMarq on the inliers,
  // cv_solvers.hpp: find_extrinsic_iterative) in a kernel of its own behind k_ransac_pnp; workspace [S][pnp_tail_stride] doubles
  int pnp_tail_cv;
  double* pnp_tail_ws;
  size_t pnp_tail_stride;
  int kf_check;             // keyframe payloads carry a checksum the local-map worker verifies (FLVIS_KF_CHECK=1: stress test of the hand-over's fences)
  long long* counters;      // [8]: frames, keyframes, ba_runs, track_fail frames ...
  long long* ba_ovf_word;   // host-mapped: a window that exceeds a capacity stores (BA_OVF_* bits) << 32 | (lane-local stream + 1) (k_ba_worker)
  // local-map feedback (F2FTracking::correction_feed, dead in the reference's v2)
  int* rec_id;              // [S][POSE_REC]  ID_POSE::frame_id (an int in the reference)
  double* rec_T;            // [S][POSE_REC][7]
  // device table of this frame's input image bases (entry 0: img0, entry 1: img1 or, on DEPTH_D435 rigs, the Z16 depth image
  // [S][h][w]).  Rounds 1-3 uploaded it per frame and read the images through it; since round 4 the image bases are kernel arguments
  // (img_plain, in_img1) and the table is only filled by the copying fallback of the inputs (no mapped staging slot, lane_frame)
  const uint8_t* const* in_tab;
  // ... and the second image's base itself (a kernel argument: it changes from frame to frame with the caller's buffer)
  const uint8_t* in_img1;
  CorrectionDev* corr_in;   // [S] correction waiting for the stream's next Tracking frame (valid flag), or nullptr
  KJoin kj;                 // joins folded into THIS launch (set by the host in front of it, cleared behind it)
};

// The rig of stream s, read through the constant address space: with a workgroup-uniform s the fields are scalar loads, as they were
// when the one calibration of the tracker was a kernel argument (a thread-per-stream kernel reads them per lane).  The array is only
// written between kernels (tracker creation, k_set_rig).
__device__ inline CRig& rig_of(const Pipe& p, int s) { return ((CRig*)p.rig)[s]; }

// KFMSG_CMD_RESET_LM as vo_localmap.cpp:87-98 applies it (optimizer_state = UN_INITIALIZED, bag->reset(), kfs.clear(), optimizer.clear(),
// edges.clear()): the stream's window back to the state of a new tracker, the published correction withdrawn.  All threads of one
// workgroup, by the owner of the stream's window (k_ba_worker) or where no local map runs (k_kfq_drop).
__device__ inline void window_reset_dev(const Pipe& p, int s) {
  long long* w = reinterpret_cast<long long*>(p.win + s);
  static_assert(sizeof(WindowDev) % 8 == 0, "WindowDev is cleared in 8-byte words");
  for (int i = threadIdx.x; i < (int)(sizeof(WindowDev) / 8); i += blockDim.x) w[i] = 0;
  if (threadIdx.x == 0) {
    p.corr[s].valid = 0;
    p.st[s].lm_state = 0;
  }
  __syncthreads();
}

int ba_lds_budget_max();
// whether a dynamic LDS of `bytes` holds k_ba_worker's reduced system, IMU blocks and chunk table for every window of `window` keyframes,
// and the smallest such budget (a whole number of KB, as FLVIS_BA_LDS_KB sets it)
bool ba_lds_admits(int bytes, int window);
int ba_lds_min_bytes(int window);
void launch_imu_feed(hipStream_t st, const Pipe& p);
void launch_frame_begin(hipStream_t st, const Pipe& p, const double* d_time);
// cv::solvePnPRansac on caller arrays (one workgroup per correspondence set): the loop closing's geometric check
int pnp_ransac_max_points();
constexpr int EPNP_DBG_N = 160;  // doubles per set of launch_epnp_sets's output
void launch_epnp_sets(hipStream_t st, const float* p3d, const float* p2d, const int* count, int cap, int n_sets, const double* K4, double* out);
// K4: fx fy cx cy of every set (host); or d_cams (device, non-null): set b's four doubles at d_cams + cam_stride * (d_cam_of ? d_cam_of[b] : b)
void launch_pnp_ransac_sets(hipStream_t st, const float* p3d, const float* p2d, const int* count, int cap, int n_sets, const double* K4,
                            const double* d_cams, int cam_stride, const int* d_cam_of, int iterative, const double* guess7,
                            const unsigned long long* seeds, int max_iters, double reproj_px, double conf, double* pose7, unsigned char* mask,
                            int* n_inliers);
// cv::findFundamentalMat(FM_RANSAC) on caller arrays (one workgroup per set; cap <= fund_ransac_max_points())
int fund_ransac_max_points();
void launch_fund_ransac_sets(hipStream_t st, const float* m1, const float* m2, const int* count, int cap, int n_sets, double thr_px,
                             double conf, unsigned char* mask, int* n_inliers);
// OptimizeInFrame::optimize on caller arrays (one workgroup per set; cap <= pose_lm_max_edges()); set b's camera at d_K4 + k_stride * b
int pose_lm_max_edges();
hipError_t launch_pose_lm_sets(hipStream_t st, const double* lm3d, const double* lm2d, const long long* lm_id, const int* count, int cap,
                               int n_sets, const double* d_K4, int k_stride, double* pose7, unsigned char* ok);
// cv::undistortPoints / cv::projectPoints on caller arrays (geom_calls.hip), one thread per point; d_cam: [n_cam][GEOM_CAM_N] doubles
// K (4) D (4) R (9) P (12), cam_stride GEOM_CAM_N or 0 (one camera); d_pose7 [n_sets][7]
constexpr int GEOM_CAM_N = 29;
void launch_undistort_points_sets(hipStream_t st, const float* src, const int* count, int cap, int n_sets, const double* d_cam, int cam_stride,
                                  float* dst);
void launch_project_points_sets(hipStream_t st, const float* p3d, const int* count, int cap, int n_sets, const double* d_pose7,
                                const double* d_cam, int cam_stride, float* dst);
void launch_store_progress(hipStream_t st, long long* host_word, long long v);  // stream-ordered store into host-mapped memory
void launch_store_flag(hipStream_t st, long long* word, long long v);  // stream-ordered store of a sequence number into a device word
void launch_wait_flag(hipStream_t st, const long long* flag, int n_words, long long seq, long long* err_word);  // stream-ordered wait for an upload's sequence block
void launch_frame_head(hipStream_t st, const Pipe& p, const double* d_time, long long* host_progress, long long frame_no);  // imu_feed + frame_begin in one launch
// ... + track_prepare (only when nothing runs between the two: no local-map feedback to apply)
void launch_frame_head_prepare(hipStream_t st, const Pipe& p, const double* d_time, long long* host_progress, long long frame_no);
void launch_apply_correction(hipStream_t st, const Pipe& p);
void launch_track_prepare(hipStream_t st, const Pipe& p);
void launch_track_collect(hipStream_t st, const Pipe& p);
void launch_ransac_f(hipStream_t st, const Pipe& p, bool with_collect = false);  // (with_collect: k_track_collect's work as its prologue)
void launch_ransac_pnp(hipStream_t st, const Pipe& p);
void launch_pnp_tail_cv(hipStream_t st, const Pipe& p);
void launch_track_post(hipStream_t st, const Pipe& p);
void launch_pose_lm(hipStream_t st, const Pipe& p);
void launch_reproj_filter(hipStream_t st, const Pipe& p);
void launch_pose_lm_filter(hipStream_t st, const Pipe& p);  // the two above in one launch
void launch_vi_correction(hipStream_t st, const Pipe& p);  // viCorrectionFromVision of the streams k_reproj_filter marked
void launch_add_new(hipStream_t st, const Pipe& p);
void launch_depth_seeds(hipStream_t st, const Pipe& p);        // stereo-LK seeds of the current landmarks (critical path)
void launch_add_new_seeds(hipStream_t st, const Pipe& p);      // the two above in one launch
// ... behind k_feature_dem's work in the same launch (launch_feature_dem's arguments that are not the Pipe's); with_seeds: up to and
// including k_depth_seeds' work, else up to k_add_new's
struct DemLaunch {
  int w, h;
  const float* sorted_xy;
  const int* region_off;
  int corner_cap;
};
void launch_dem_add_new_seeds(hipStream_t st, const Pipe& p, const DemLaunch& d, bool with_seeds);
void launch_depth_triangulate(hipStream_t st, const Pipe& p);  // two-view triangulation for k_depth_innovate (beside the stereo LK)
void launch_depth_innovate(hipStream_t st, const Pipe& p);
void launch_frame_end(hipStream_t st, const Pipe& p);
void launch_depth_innovate_end(hipStream_t st, const Pipe& p);  // the two above in one launch (a step in which every stream has a frame)
// per-stream reset (flvis_reset_streams / flvis_local_map_reset, and the initial state at tracker creation): one workgroup per listed stream
constexpr int RESET_LIST = 64;  // streams per launch
enum { RS_TRACKER = 1, RS_CMD = 2, RS_SKIP = 4, RS_CREATE = 8 };  // what k_stream_reset does for a stream (bits)
struct ResetList {
  int n;
  int s[RESET_LIST];              // lane-local stream indices
  unsigned char mode[RESET_LIST];  // RS_* bits
};
// err_word (host-mapped): a command that met a full queue stores the stream's lane-local index + 1 there (flvis_hip_synchronize reports it)
void launch_stream_reset(hipStream_t st, const Pipe& p, const ResetList& list, long long* err_word);
void launch_kfq_drop(hipStream_t st, const Pipe& p);
// flvis_reset_streams_rigs: stream ls (lane-local) of the lane takes the rig r -- in stream order, ahead of its k_stream_reset
void launch_set_rig(hipStream_t st, const Pipe& p, int ls, const RigParams& r);  // the queues emptied without a local map, a pending reset command applied
// local map
void launch_ba_worker(hipStream_t st, const Pipe& p);
hipError_t ba_kernels_init();
hipError_t track_kernels_init();
size_t ba_scratch_doubles();

}  // namespace flvis
