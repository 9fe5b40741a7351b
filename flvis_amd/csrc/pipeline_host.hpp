// flvis_amd: the host side's own types -- a tracker (Pipeline), its sub-batches of streams (Lane) and the joins between a lane's HIP
// streams (Join) -- shared by pipeline.cpp (create / destroy / entry points), frame_schedule.cpp (the order in which a frame's kernels
// and joins are enqueued) and host_feed.cpp (flvis_image_feed_host).  Private: not installed, no kernel reads it.
#pragma once
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "kf_log.hpp"
#include "lm_cloud.hpp"
#include "track_kernels.hpp"

namespace flvis {

constexpr int PROF_STAGES = 20;  // every stage has its own (begin, end) event pair on the stream it runs on

// The joins between a lane's streams ("stream a has reached this point" / "stream b goes on when that point has been reached").
// FLVIS_JOIN (round 6; "flag" is the default, "event" the form of rounds 1-5): as device words instead of events -- the producing stream
// stores a sequence number behind its last kernel (k_store_flag), the consuming stream waits for it with one sleeping lane (k_wait_flag).
// An event record is a system-scope barrier packet and a wait a barrier packet that polls the record's signal for as long as it is pending
// (and slows the queues beside it, profiles/r06_h2d.md); a word in HBM costs two one-lane launches.
// J_BA0 + i % BAQ follows the lane's i-th local-map launch (back-pressure on the keyframe queues in stream order: the tracking stream
// waits for the launches of KFQ-3 frames ago before it appends new keyframes, lane_backpressure_wait).
constexpr int BAQ = 64;
enum JoinId {
  J_IMG,   // the left pyramid of the frame (detection stream)
  J_DET,   // the corner detection and the right pyramid (detection stream)
  J_GFTT,  // FeatureDEM's image part (detection stream)
  J_FE,    // a point of the tracking stream a local-map launch starts behind
  J_LM,    // the tracking stream's hand-overs to the detection stream within a frame
  J_TRI,   // the two-view triangulation (detection stream)
  J_HEAD,  // k_frame_head's decisions
  J_ENDF,  // "k_frame_end has finished": the next frame's ingest and an immediate local-map launch wait for it (folded joins)
  J_BA0,
  JOIN_IDS = J_BA0 + BAQ
};
inline JoinId J_BA(long long launch) { return (JoinId)(J_BA0 + (int)(launch % BAQ)); }
struct Join {
  hipEvent_t ev = nullptr;     // FLVIS_JOIN=event
  long long* word = nullptr;   // Lane::d_join + 8 * id (64 bytes apart)
  unsigned* cnt = nullptr;     // Lane::d_join_cnt + id: arrival counter of the launches that signal the word themselves (KJoin)
  long long seq = 0;           // the last sequence number signalled
};

// One sub-batch of streams [s0, s0 + S): all device state of those streams and the HIP streams their frames run on.
struct Lane {
  int s0 = 0, S = 0;
  Pipe pipe;
  hipStream_t st = nullptr;  // tracking chain (the context's stream when the tracker has a single lane)
  bool own_st = false;
  // images
  uint8_t* pyr0[2][LK_MAX_LEVELS] = {};
  uint8_t* pyr1[LK_MAX_LEVELS] = {};
  uint32_t* tc = nullptr;  // LK template cache [S][pipe.tc_cap][tc_stride dwords] (LKParams::tc), or nullptr
  int tc_stride = 0;
  GfttScratch gftt;
  float* gftt_xy = nullptr;
  float* dem_sorted = nullptr;  // [S][2 gftt_num][2] FeatureDEM: the corners in region-major, score-sorted order (k_feature_dem_prep)
  int* dem_roff = nullptr;      // [S][17] ... and the offset of every region in that list
  int* gftt_n = nullptr;
  unsigned* eq_hist = nullptr;
  uint8_t* eq_lut = nullptr;
  // per-frame inputs of the lane, uploaded as ONE block: [times S][imu S*IMU_MAX*7][input image bases 2][n_imu S][present S]
  uint8_t* d_inputs = nullptr;
  double* d_time = nullptr;
  const uint8_t** d_tab = nullptr;
  size_t input_bytes = 0;
  std::vector<double> h_imu;  // [S][IMU_MAX][7] staged between two frames
  std::vector<int> h_nimu;
  std::vector<long long> imu_read;  // [S] rows of the stream's IMU-state ring the caller has fetched (flvis_get_imu_states)
  // Host staging: a ring of pinned slots, each guarded by an event recorded after its upload, so that image_feed never
  // waits for the previous frame -- the host runs several frames ahead of the GPU and a frame's launches are already queued
  // when the GPU gets to them.
  static constexpr int PIN_RING = 4;
  void* pinned[PIN_RING] = {};      // page-locked staging of a frame's inputs (host view) ...
  uint8_t* pinned_dev[PIN_RING] = {};  // ... and the same memory as the device sees it (k_frame_head reads it in place)
  const uint8_t* h_tab[2] = {nullptr, nullptr};  // the image bases of the last frame fed (host copy of the table)
  size_t in_off_imu = 0, in_off_tab = 0, in_off_n = 0, in_off_pres = 0;
  // the slot of frame n may be refilled once frame n's upload is done: k_frame_head (the first kernel after the upload) stores the
  // frame number into this host-mapped word and the host polls it.  (hipEventSynchronize on an event recorded after the upload
  // returned only when EVERYTHING enqueued so far had finished -- measured: the host then slept through four queued frames and the
  // GPU ran dry once per burst, a 0.9 ms hole in every fifth frame.)
  volatile long long* h_progress = nullptr;  // host view
  long long* d_progress = nullptr;           // device view of the same word
  long long frames_uploaded = 0;             // frames this lane has enqueued
  std::vector<void*> allocs;
  std::vector<hipEvent_t> prof_ev;  // optional per-stage HIP-event timing (flvis_prof_enable)
  std::vector<unsigned char> prof18_rec;  // per armed step: the local-map launch's event pair (stage 18) was recorded -- a deferred launch
                                          // (Pipeline::defer_ba) belongs to the NEXT step, the first step of a batch has none, the last one two
  // corner detection on its own HIP stream: goodFeaturesToTrack only needs the new image, so it runs beside the temporal
  // tracking chain (LK -> RANSACs -> pose LM) and joins before FeatureDEM consumes the corners
  hipStream_t det_stream = nullptr;
  Join join[JOIN_IDS];
  long long* d_join = nullptr;     // [JOIN_IDS] words, 64 bytes apart (Join::word)
  unsigned* d_join_cnt = nullptr;  // [JOIN_IDS] (Join::cnt)
  bool endf_valid = false;       // the last k_frame_end carried J_ENDF's signal
  int idx = 0;  // position in Pipeline::lanes
  // multi-lane trackers: ev_end[n % HOLD_RING] follows the lane's n-th frame (the context's stream waits for the frame whose
  // input buffers the caller may reuse next, see flvis_set_input_hold); ev_stagger follows the temporal LK of the lane's first
  // processed frame (the next lane starts its first frame there, so that the lanes run out of phase)
  static constexpr int HOLD_RING = 8;
  hipEvent_t ev_end[HOLD_RING] = {};
  hipEvent_t ev_stagger = nullptr;
  long long ba_launches = 0;
  bool ba_pending = false;       // the local-map launch for the last frame's keyframes has not been enqueued yet (Pipeline::defer_ba)
  // reset commands in the keyframe queues (flvis_reset_streams / flvis_local_map_reset): per stream, the lane frame count when its last
  // command was appended (-1: none, or keyframes pushed behind it) -- a second request before the next frame adds no entry; and the lane
  // frame counts at which any stream of the lane had one appended, for the back-pressure (lane_backpressure_wait)
  std::vector<long long> cmd_frame;
  std::vector<long long> cmd_steps;
  int lmc_cmds = 0;              // reset calls that appended a command since the lane's last local-map launch (local_map_work)
  bool cmd_since_frame = false;  // a command was appended since the lane's last frame (a frame without the local map applies it: k_kfq_drop)
  long long kfl_seq = 0;         // k_kf_log_append launches of the lane since the log was enabled: the next one's parity (kf_log.hpp)
};

struct Pipeline {
  int S = 0;
  flvis_cfg cfg;                 // the batch-wide fields every stream shares (stream 0's config)
  std::vector<flvis_cfg> cfgs;   // [S] the config each stream runs on (flvis_get_stream_cfg) ...
  std::vector<RigParams> rigs;   // [S] ... and its rig as the device has it (host mirror of the lanes' Pipe::rig)
  int lane_size = 0;
  std::vector<Lane*> lanes;
  int levels_t = 0, levels_s = 0, levels = 0;
  int lw[LK_MAX_LEVELS], lh[LK_MAX_LEVELS], lpitch[LK_MAX_LEVELS];
  size_t lstride[LK_MAX_LEVELS];
  int lbx = 0, lby = 0;  // physical border of every pyramid level (columns / rows on each side)
  int max_pts = 0;  // bound on the landmarks of a frame (16 regions x max_region_feature_num): sizes the LK grid
  // The environment knobs the tracker honours, read once when it is created (read_knobs; INTEGRATION.md lists them)
  int n_lanes_req = 1;  // FLVIS_LANES: sub-batches of streams (1 .. 16)
  bool lk_border = true;  // FLVIS_LK_BORDER: pyramid levels with a physical border
  bool lk_tcache = true;  // FLVIS_LK_TCACHE: the LK template cache between a frame's stereo and the next frame's temporal LK
  int chain_merge = 31;  // FLVIS_CHAIN_MERGE: launches of the frame's chain folded into their neighbours (Frame::merge_collect ...)
  bool head_prepare = true;  // FLVIS_HEAD_PREPARE: k_frame_head and k_track_prepare as one launch
  bool kf_check = false;  // FLVIS_KF_CHECK (Pipe field)
  bool pnp_tail_cv = false;  // FLVIS_PNP_TAIL=cv
  unsigned prof_scope = 0;  // FLVIS_PROF_EVENT_SCOPE: release scope of the stage-timing events
  long long frames_fed = 0;
  long long stream_frames = 0;  // stream-frames fed (flvis_get_counters [0]): frames_fed * S unless steps left streams absent
  std::vector<void*> allocs;  // context-level device allocations (host-feed staging)
  int prof_cap = 0, prof_step = 0;
  unsigned long long prof_mask = ~0ull;  // stages that record events (an event record costs a few us on the GPU queue)
  // The local map runs beside the front-end: k_frame_end appends KeyFrame payloads to per-stream queues, k_ba_worker (one
  // launch per lane and frame on one of the shared local-map streams, round-robin) drains them.  Its output is never fed
  // back into the tracker in the reference (src/frontend/vo_tracking.cpp:373-385).
  static constexpr int NBA = 8;
  int nba = 2;                   // local-map streams in use: 2 per lane (profiles/r04_local_map_and_streams_ab.md) ...
  int nba_lane = 2;              // ... of which every lane uses its own nba_lane
  int host_lead = 3;             // frames the host may run ahead of the GPU (FLVIS_HOST_LEAD, 1 .. PIN_RING; 2 until round 6: a host thread that is held up for a millisecond then leaves the GPU dry)
  int host_lead_cap = 4;         // (flvis_image_feed_host lowers it to 1 for its call: its copies and events add to the queued commands)
  int input_hold = 0;            // flvis_set_input_hold: frames the caller keeps its input buffers untouched after handing them over
  double host_ms_total = 0, host_ms_wait = 0;  // host time inside flvis_image_feed / of it blocked on the pinned ring
  bool sync_each_frame = false;  // FLVIS_SYNC_EACH_FRAME=1: image_feed waits for the previous frame (tuning knob)
  int ba_every = 1;              // launch the local-map worker every n-th frame (FLVIS_BA_EVERY)
  bool lk_stats = false;         // flvis_debug_lk_stats: the LK launches count their iterations per level into counters[36 .. 59]
  hipStream_t ba_stream[NBA] = {};
  long long ba_rr = 0;           // round-robin counter over the local-map streams
  hipEvent_t ev_in = nullptr;    // the caller's inputs are ready (recorded on the context's stream)
  bool defer_ba = false;         // inside flvis_run_steps, not its last step: the local-map launch of this frame waits for the next frame (stage_pnp_pose)
  bool feedback_used = false;    // flvis_correction_feed was called: k_apply_correction runs after every frame_begin
  // flvis_image_feed_host: double-buffered device staging filled by async H2D copies on a copy stream, so that the upload of
  // frame N+1 overlaps the kernels of frame N (allocated by the first call)
  struct HostFeed {
    hipStream_t strm = nullptr;
    static constexpr int SLOTS = 3;   // (mode 2 cycles through three staging slots, mode 1 through two)
    uint8_t* raw[SLOTS][2] = {};   // [slot][camera]: the images as handed over (tightly packed rows of w * bytes-per-pixel)
    uint8_t* gray[SLOTS][2] = {};  // [slot][camera]: cvtColor output for 3/4-channel input
    // mode 2 (round 6, default): nothing but copies on the copy stream.  Behind the images of a call the copy engine writes a block of
    // sequence numbers (FLAG_WORDS x the call's number, from a page-locked ring: large enough not to be turned into a blit kernel);
    // k_wait_flag on the stream that ingests the images waits for it; the host learns that the uploads are done from hipStreamQuery
    // and that a slot is free from the frame-progress word.  No event, no kernel, no AQL barrier packet on the copy stream's queue.
    int mode = 2;  // FLVIS_H2D_MODE
    static constexpr int FLAG_WORDS = 4096, FLAG_RING = 4;
    long long* h_flag[FLAG_RING] = {};
    long long* d_flag = nullptr;
    long long slot_frame[SLOTS] = {0, 0, 0};  // the lane frame number (frames_uploaded) that read the slot last
    long long last_call_frame = -1;           // frames_fed behind this entry's last call (another entry in between: the chain is not continuous)
    size_t raw_bytes[2] = {}, gray_bytes = 0;
    hipEvent_t ev_done[2] = {}, ev_free[2] = {};
    long long n = 0;
    volatile long long* h_up = nullptr;  // host-mapped: number of calls whose uploads have finished (stored by the copy stream)
    long long* d_up = nullptr;
    std::vector<double> times;
    double ms_wait_uploads = 0, ms_issue = 0, ms_feed = 0;  // host time of the calls: blocked on the previous uploads, issuing, in flvis_image_feed
    // flvis_debug_host_feed_timing: the uploads of a call bracketed by two timing events on the copy stream (their own durations, what
    // bench.py's with_h2d.upload_GBs is made of); read back when the slot comes round again
    bool timing = false;
    hipEvent_t ev_t0[2] = {}, ev_t1[2] = {};
    bool timed[2] = {false, false};
    size_t timed_bytes[2] = {0, 0};
    double up_ms = 0, up_bytes = 0, up_calls = 0;
  } hf;
  hipEvent_t up_event = nullptr;  // set by flvis_image_feed_host for its flvis_image_feed call: the upload's event, waited for on the stream that ingests the images
  const long long* up_flag = nullptr;  // ... or (mode 2) the sequence block the copy engine writes behind the images, and the number to wait for
  long long up_seq = 0;
  static constexpr unsigned ev_flags = hipEventDisableTiming;  // flags of every event of the pipeline (system scope: profiles/r06_h2d.md)
  bool flag_joins = false;                    // FLVIS_JOIN=flag
  bool fold_joins = false;                    // FLVIS_JOIN_FOLD: the chain's own kernels wait for / store the words (KJoin)
  bool chain_continuous = false;              // this frame follows the previous one on the main stream with nothing of the caller's in between
  // flvis_local_map_cloud_enable: the streams' map-cloud records (cap 0: off, and no k_lm_cloud_append is launched) and the event that
  // orders the context's stream behind the tracker's for a fetch
  LmCloudRec lmc{};
  hipEvent_t lmc_ev = nullptr;
  // flvis_keyframe_log_enable: the streams' keyframe logs (cap 0: off, and no k_kf_log_append is launched)
  KfLogRec kfl{};
  Lane& lane_of(int stream, int& local) {
    const int k = stream / lane_size;
    local = stream - k * lane_size;
    return *lanes[k];
  }
};

template <typename T>
T* dalloc(std::vector<void*>& allocs, size_t n, bool zero = true) {
  void* p = nullptr;
  if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) return nullptr;
  if (zero) hipMemset(p, 0, n * sizeof(T));
  allocs.push_back(p);
  return (T*)p;
}

// frame_schedule.cpp
unsigned pyramid_levels(hipStream_t ds, bool bordered, ImgSel src0, int spitch0, size_t sstride0, bool ingest, bool level0_is_buffer,
                        const PyrSel& pyr, int S, const int* active);
void sync_all(flvis_ctx* ctx);
LmCloudRec lane_lmc(const Pipeline* pl, const Lane* L);
void local_map_work(Pipeline* pl, Lane* L, hipStream_t bs, int pairs, hipEvent_t prof_end);
void launch_local_map(Pipeline* pl, Lane* L, JoinId at, bool signal, hipEvent_t* prof_begin_end);
// kf_log.hip: the lane's part of the log, its append kernel behind the lane's k_frame_end on `st`, a stream's record emptied in order
// with its reset on the lane's tracking stream, and the log freed
KfLogRec lane_kfl(const Pipeline* pl, const Lane* L);
void kf_log_frame(Pipeline* pl, Lane* L, hipStream_t st, const uint8_t* in1, bool in_place);
void kf_log_reset_stream(Pipeline* pl, Lane* L, int ls);
void kf_log_free(Pipeline* pl);
struct LaunchJoins;
void lane_backpressure_wait(Pipeline* pl, Lane* L, LaunchJoins* folded, int k0 = 0, int k1 = 1 << 30);

}  // namespace flvis
