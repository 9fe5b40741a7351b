// flvis_amd: the frame schedule -- the order in which a frame's kernels and the joins between the lane's HIP streams are enqueued
// (lane_frame and its stages), the local-map launches beside it, and the entry points that feed frames resident on the device.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "pipeline_host.hpp"

using namespace flvis;

static void fill_pyr(Pipeline* pl, PyrSel& ps, uint8_t* const* l0, uint8_t* const* l1, const int* cur, int flip, int levels) {
  ps.levels = levels;
  for (int l = 0; l <= levels; l++) {
    ps.lvl[l] = ImgSel{{l0[l], l1 ? l1[l] : l0[l]}, cur, flip, nullptr};
    ps.w[l] = pl->lw[l];
    ps.h[l] = pl->lh[l];
    ps.pitch[l] = pl->lpitch[l];
    ps.stride[l] = pl->lstride[l];
    ps.bx[l] = pl->lbx;
    ps.by[l] = pl->lby;
  }
}

// Levels 1 .. levels of the pyramid `pyr` (level 0 too when `ingest` is set: the copy of the caller's image src0).  Level 0 is read from
// src0 (the caller's image when ingest or in place, else pyr.lvl[0] itself, which another kernel wrote).  The levels' physical borders are
// written by the kernel that produces the level wherever it can; the return value is the mask of the levels whose border is still to
// fill (k_pyr_border).  level0_todo: level 0 has a border that nobody has written yet (equalizeHist / the unaligned copy made it).
// Walking kernels (pyr_walk.hip) where the geometry allows -- 16-pixel lanes: widths that are multiples of 16 up to 1024 --, else the
// LDS-tile kernels level by level.
unsigned flvis::pyramid_levels(hipStream_t ds, bool bordered, ImgSel src0, int spitch0, size_t sstride0, bool ingest, bool level0_is_buffer,
                               const PyrSel& pyr, int S, const int* active) {
  const int levels = pyr.levels;
  unsigned border_left = bordered ? (1u << (levels + 1)) - 1u : 0u;
  if (!level0_is_buffer && !ingest) border_left &= ~1u;  // (level 0 is the caller's buffer: no border to fill)
  // levels per walking launch: one, then two ("12": the fastest for 640-pixel rows; other plans: profiles/r04_lk_ab.md) -- unless level 1
  // is not a whole number of 16-pixel lanes while level 0 is (752-pixel rows: 376): then the first launch takes two levels ("21") and only
  // the last one is left to the tile kernels
  const char* plan = (pyr.w[0] & 15) == 0 && (((pyr.w[0] + 1) >> 1) & 15) != 0 ? "21" : "12";
  int step = 0, l = 0;
  while (l < levels) {
    int nout = plan[step] ? plan[step] - '0' : 1;
    if (plan[step]) step++;
    if (nout > levels - l) nout = levels - l;
    const bool from0 = l == 0 && (ingest || !level0_is_buffer);
    ImgSel src = from0 ? src0 : pyr.lvl[l];
    const int spitch = from0 ? spitch0 : pyr.pitch[l];
    const size_t sstride = from0 ? sstride0 : pyr.stride[l];
    const bool copy0 = l == 0 && ingest;
    PyrSel q = pyr;
    for (int j = 0; j <= nout; j++)  // a level too small to mirror into its border in one pass keeps it for k_pyr_border
      if (!(bordered && pyr_border_fusable(pyr.w[l + j], pyr.h[l + j], pyr.bx[l + j], pyr.by[l + j]))) q.bx[l + j] = q.by[l + j] = 0;
    if (pyr_walk_ok(pyr.w[l], pyr.h[l], nout, q.bx + l, q.by + l, copy0)) {
      launch_pyr_walk(ds, src, pyr.w[l], pyr.h[l], spitch, sstride, q, l, nout, copy0, S, active);
      for (int j = copy0 ? 0 : 1; j <= nout; j++)
        if (q.bx[l + j]) border_left &= ~(1u << (l + j));
      l += nout;
      continue;
    }
    // one level by the tile kernels
    const int d = l + 1;
    if (copy0) {
      const bool f = q.bx[0] && q.bx[1];
      launch_pyr_down_ingest(ds, src, pyr.w[0], pyr.h[0], spitch, sstride, pyr.lvl[0], pyr.pitch[0], pyr.stride[0], pyr.lvl[1], pyr.pitch[1],
                             pyr.stride[1], S, active, f ? pyr.bx[1] : 0, f ? pyr.by[1] : 0);
      if (f) border_left &= ~3u;
    } else {
      const bool f = q.bx[d] != 0;
      const bool sf = !from0 && bordered && !((border_left >> l) & 1u);  // (the source level's border is complete)
      launch_pyr_down(ds, src, pyr.w[l], pyr.h[l], spitch, sstride, pyr.lvl[d], pyr.pitch[d], pyr.stride[d], S, active, f ? pyr.bx[d] : 0,
                      f ? pyr.by[d] : 0, sf ? pyr.bx[l] : 0, sf ? pyr.by[l] : 0);
      if (f) border_left &= ~(1u << d);
    }
    l = d;
  }
  return border_left;
}

// "stream s has reached this point" / "stream s goes on when that point has been reached": an event, or (FLVIS_JOIN=flag) a device word
static void join_signal(Pipeline* pl, Lane* L, JoinId id, hipStream_t s) {
  Join& j = L->join[id];
  ++j.seq;
  if (pl->flag_joins) launch_store_flag(s, j.word, j.seq);
  else hipEventRecord(j.ev, s);
}
static void join_wait(Pipeline* pl, Lane* L, hipStream_t s, JoinId id) {
  const Join& j = L->join[id];
  if (pl->flag_joins) launch_wait_flag(s, j.word, 1, j.seq, L->d_progress + 2);
  else hipStreamWaitEvent(s, j.ev, 0);
}

namespace flvis {
// The joins ONE launch on stream `s` carries itself (KJoin; FLVIS_JOIN_FOLD): the launch that is handed `kj` waits for up to two words in
// front of its first workgroup, stores a word behind its last one, or does not END before a word is there (post: the launch behind it,
// an LK launch, needs no wait of its own).  Requests are made in front of the launch; where the joins are not folded a wait is enqueued
// at once, a signal and a post (as a wait) when the scope ends, behind the launch.  The fold_ forms leave that fallback to the caller
// (false: not folded), for the sites that emit it further down the stream.  The scope's end clears `kj`: no later launch repeats a join.
struct LaunchJoins {
  Pipeline* pl;
  Lane* L;
  hipStream_t s;
  KJoin& kj;
  int n_wait = 0, sig_later = -1, post_later = -1;
  LaunchJoins(Pipeline* pl_, Lane* L_, hipStream_t s_, KJoin& kj_) : pl(pl_), L(L_), s(s_), kj(kj_) {}
  LaunchJoins(const LaunchJoins&) = delete;
  ~LaunchJoins() { end(); }
  bool fold_signal(JoinId id) {
    if (!pl->fold_joins) return false;
    Join& j = L->join[id];
    kj.sig = j.word;
    kj.sig_seq = ++j.seq;
    kj.sig_cnt = j.cnt;
    return true;
  }
  bool fold_wait(JoinId id) {
    if (!pl->fold_joins || n_wait == (int)(sizeof(kj.wait) / sizeof(kj.wait[0]))) return false;
    kj.wait[n_wait] = L->join[id].word;
    kj.wait_seq[n_wait++] = L->join[id].seq;
    kj.err = L->d_progress + 2;
    return true;
  }
  bool fold_post(JoinId id) {
    if (!pl->fold_joins) return false;
    kj.post = L->join[id].word;
    kj.post_seq = L->join[id].seq;
    kj.err = L->d_progress + 2;
    return true;
  }
  void signal(JoinId id) {
    if (!fold_signal(id)) sig_later = id;
  }
  void wait(JoinId id) {
    if (!fold_wait(id)) join_wait(pl, L, s, id);
  }
  void post(JoinId id) {
    if (!fold_post(id)) post_later = id;
  }
  // behind the launch (the scope may be used for another launch afterwards)
  void end() {
    kj = KJoin{};
    if (sig_later >= 0) join_signal(pl, L, (JoinId)sig_later, s);
    if (post_later >= 0) join_wait(pl, L, s, (JoinId)post_later);
    n_wait = 0, sig_later = post_later = -1;
  }
};
}  // namespace flvis

// the lane's part of the map-cloud record, and its append kernel behind a local-map launch of the lane on `bs`
LmCloudRec flvis::lane_lmc(const Pipeline* pl, const Lane* L) {
  LmCloudRec r = pl->lmc;
  r.hdr += (size_t)L->s0 * LMC_HDR;
  r.ids += (size_t)L->s0 * r.cap;
  r.pts += (size_t)L->s0 * r.cap * 3;
  return r;
}
// The worker of one local-map launch on `bs`.  Record off: k_ba_worker as ever.  Record on: every optimisation must be looked at
// before the next one of its stream overwrites the correction, and k_lm_cloud_append can only run between two kernels.  So a worker
// then takes ONE queue entry per stream (ba_drain 1: at most one optimisation) with the append kernel behind it, `pairs` times -- as
// many entries as the one launch would have taken -- and nothing else of the lane's local map runs meanwhile (launch_local_map orders
// the lane's launches one behind the other; the other callers wait on the host).  An owner still stays past its share at KFQ / 2
// waiting entries, the back-pressure's last resort; that is out of reach here: a launch takes what the frames since the previous
// launch can have queued.
void flvis::local_map_work(Pipeline* pl, Lane* L, hipStream_t bs, int pairs, hipEvent_t prof_end) {
  if (pl->lmc.cap <= 0) {
    launch_ba_worker(bs, L->pipe);
    if (prof_end) hipEventRecord(prof_end, bs);
    return;
  }
  Pipe one = L->pipe;
  one.ba_drain = 1;
  const LmCloudRec r = lane_lmc(pl, L);
  for (int k = 0; k < pairs; k++) {
    launch_ba_worker(bs, one);
    if (prof_end && k == 0) hipEventRecord(prof_end, bs);
    launch_lm_cloud_append(bs, one, r);
  }
}

// One local-map launch for the lane (a workgroup per stream takes the stream's next keyframe): on the lane's next local-map HIP stream,
// behind the join `at` of the tracking stream (signalled here when `signal` is set), its completion kept as a join for the back-pressure.
void flvis::launch_local_map(Pipeline* pl, Lane* L, JoinId at, bool signal, hipEvent_t* prof_begin_end) {
  const int bi = (L->idx * pl->nba_lane + (int)(L->ba_launches % pl->nba_lane)) % pl->nba;
  hipStream_t bs = pl->ba_stream[bi];
  if (prof_begin_end) {  // (one timed launch per armed step: the first; a second one in the same step keeps its hands off the pair)
    unsigned char& rec = L->prof18_rec[(size_t)pl->prof_step];
    if (rec) prof_begin_end = nullptr;
    else rec = 1;
  }
  if (signal) join_signal(pl, L, at, L->st);
  join_wait(pl, L, bs, at);
  // record on: behind the lane's previous launch and its append kernel (it ran on the lane's other local-map stream)
  const bool rec_on = pl->lmc.cap > 0;
  if (rec_on && L->ba_launches > 0) join_wait(pl, L, bs, J_BA(L->ba_launches - 1));
  if (prof_begin_end) hipEventRecord(prof_begin_end[0], bs);
  // (a reset command takes a queue entry like a keyframe, at most one per stream and frame)
  local_map_work(pl, L, bs, pl->ba_every + std::min(L->lmc_cmds, pl->ba_every), prof_begin_end ? prof_begin_end[1] : nullptr);
  L->lmc_cmds = 0;
  join_signal(pl, L, J_BA(L->ba_launches), bs);
  L->ba_launches++;
  L->ba_pending = false;
}

static void sync_streams(flvis_ctx* ctx) {
  hipStreamSynchronize(ctx->stream);
  Pipeline* pl = ctx->pipe;
  if (!pl) return;
  for (Lane* L : pl->lanes) {
    hipStreamSynchronize(L->st);
    hipStreamSynchronize(L->det_stream);
  }
  for (int k = 0; k < Pipeline::NBA; k++)
    if (pl->ba_stream[k]) hipStreamSynchronize(pl->ba_stream[k]);
}
// waits for everything that was enqueued AND for the local map to have consumed every queued keyframe (a keyframe that
// slipped in while a worker workgroup was releasing its window is picked up by one more worker launch)
void flvis::sync_all(flvis_ctx* ctx) {
  if (ctx->pipe)
    for (Lane* L : ctx->pipe->lanes)
      if (L->ba_pending) launch_local_map(ctx->pipe, L, J_FE, true, nullptr);  // (a launch deferred into the next frame: there is none)
  sync_streams(ctx);
  Pipeline* pl = ctx->pipe;
  if (!pl) return;
  for (Lane* L : pl->lanes) {
    std::vector<unsigned> hd(L->S), tl(L->S);
    for (int guard = 0; guard < 64; guard++) {
      hipMemcpy(hd.data(), L->pipe.kfq_head, sizeof(unsigned) * L->S, hipMemcpyDeviceToHost);
      hipMemcpy(tl.data(), L->pipe.kfq_tail, sizeof(unsigned) * L->S, hipMemcpyDeviceToHost);
      bool pending = false;
      for (int i = 0; i < L->S; i++) pending = pending || hd[i] != tl[i];
      if (!pending) break;
      local_map_work(pl, L, pl->ba_stream[0], 1, nullptr);
      hipStreamSynchronize(pl->ba_stream[0]);
    }
  }
}

// How many local-map launches back the tracking stream waits before it appends to the keyframe queues.  A reset command
// (k_stream_reset) takes a queue entry like a keyframe: every lane frame with a command among the frames the bound counts moves the wait
// one launch closer.  Without commands: the depth of rounds 1-6.
static long long lane_backpressure_depth(Pipeline* pl, Lane* L) {
  long long D = std::max(0, KFQ / 2 / pl->ba_every - 3);  // (-2, and -1 because a deferred launch is one frame late)
  if (L->cmd_steps.empty()) return D;
  const long long window = (D + pl->nba_lane + 2) * pl->ba_every;
  std::vector<long long>& c = L->cmd_steps;
  c.erase(std::remove_if(c.begin(), c.end(), [&](long long f) { return L->frames_uploaded - f > window; }), c.end());
  return std::max(0LL, D - (long long)c.size());
}

// Keyframe-queue back-pressure, expressed in stream order (never by spinning inside a kernel).  Once every local-map launch of
// this lane up to index j has finished, less than ba_backlog = KFQ / 2 keyframes of the frames up to j * ba_every are left in any
// queue: the last workgroup that owned the stream's window among those launches stayed until fewer were waiting (k_ba_worker),
// and every launch behind it found the queue empty.  The frames since then add at most (D + nba_lane) * ba_every keyframes, so
// waiting for the launches of D frames ago (the last one on each of the lane's local-map streams) keeps a queue at
// KFQ / 2 - 1 + (D + 2) * ba_every < KFQ when k_frame_end appends: no keyframe is dropped, whatever the optimiser's pace.
// (ba_every <= KFQ / 4, flvis_tracker_create.)  A reset command counts as a keyframe: lane_backpressure_depth.
// The waits go into the launch `folded` carries the joins of (k_frame_end) as far as it has room, else on the tracking stream.
// [k0, k1): which of the lane's local-map streams, newest launch first (all of them: 0, nba_lane) -- a caller may hand the older ones to
// an earlier launch of the same frame, which waits no later than k_frame_end would (Frame::stage_new_landmarks).
void flvis::lane_backpressure_wait(Pipeline* pl, Lane* L, LaunchJoins* folded, int k0, int k1) {
  const long long D = lane_backpressure_depth(pl, L);
  for (int k = k0; k < std::min(k1, pl->nba_lane); k++) {
    const long long j = L->ba_launches - 1 - D - k;
    if (j < 0 || L->ba_launches - j > BAQ) continue;
    if (folded) folded->wait(J_BA(j));
    else join_wait(pl, L, L->st, J_BA(j));
  }
}

namespace {

// What the stages of one lane frame share
struct Frame {
  Pipeline* pl;
  Lane* L;
  Pipe& p;
  hipStream_t st, ds;  // the tracking chain's stream and the detection stream
  int S, w, h;
  int with_local_map;
  long long frame_no;  // 1-based count of the frames this lane has been fed
  bool zerocopy;       // k_frame_head reads the inputs where the host staged them
  bool prof;           // this step records its stages' events: pev[2 i], pev[2 i + 1]
  hipEvent_t* pev;
  hipEvent_t* prof18;  // stage 18's pair (the local-map launch), or nullptr
  bool skipped, idle_step;
  bool eq, aligned, depth_cam, r_in_place;
  ImgSel in0, in1, l0cur;
  bool cmd_pending;  // a reset command appended since the lane's last frame (flvis_reset_streams / flvis_local_map_reset)
  bool first_processed;
  bool head_prepare;   // k_frame_head and k_track_prepare as one launch
  bool head_posts;     // the head kernel does not end before the left pyramid is there
  bool merge_collect;  // k_track_collect as the prologue of k_ransac_f
  bool merge_end;      // k_depth_innovate and k_frame_end as one launch
  bool merge_dem;      // k_feature_dem in the launch of k_add_new (and of k_depth_seeds where they are one)
  bool merge_filter;   // k_reproj_filter as the epilogue of k_pose_lm
  // the begin (end = 0) / end (end = 1) event of stage i on the stream it runs on
  void mark(int i, int end, hipStream_t s) const {
    if (prof && ((pl->prof_mask >> i) & 1ull)) hipEventRecord(pev[2 * i + end], s);
  }
  void pb(int i, hipStream_t s) const { mark(i, 0, s); }
  void pe(int i, hipStream_t s) const { mark(i, 1, s); }
  // the stages, in the order lane_frame runs them, and what they share
  void stage_host_inputs(const uint8_t* d_img0, const uint8_t* d_img1, const double* h_times, const uint8_t* present);
  void stage_ingest_left(), stage_head(), stage_idle_tail(), stage_temporal_lk(), stage_collect_ransac_f(), stage_detection_fork();
  void stage_pnp_pose(), stage_new_landmarks(), stage_stereo_depth(), stage_frame_end();
  void local_map_tail(hipEvent_t* p18, bool timed), frame_end(bool backpressure, bool with_innovate);
  LKParams lk_params(int stats_at, int tc_mode, int order) const;
};

// ---- stage host inputs (pinned) and upload: [times][imu][input image bases][n_imu]
void Frame::stage_host_inputs(const uint8_t* d_img0, const uint8_t* d_img1, const double* h_times, const uint8_t* present) {
  frame_no = ++L->frames_uploaded;
  const int pslot = (int)((frame_no - 1) % Lane::PIN_RING);
  uint8_t* pin = (uint8_t*)L->pinned[pslot];
  if (pl->sync_each_frame) hipStreamSynchronize(st);
  // run at most host_lead frames ahead of the GPU (<= PIN_RING: the staging slot of frame N - PIN_RING must be free).  Not further:
  // beyond ~5 queued frames (~300 commands) the HIP runtime itself blocks the enqueuing thread for 7-9 ms at a time and the GPU
  // then runs dry while the queue is refilled (measured)
  // (zero-copy inputs: k_frame_head publishes its progress word when it STARTS, while its other workgroups may still be reading the
  // slot -- one slot of slack, so that the slot the host refills belongs to a frame whose successor has started, i.e. that is over)
  const long long lead = std::min(std::min(pl->host_lead, pl->host_lead_cap), (int)Lane::PIN_RING - 1);
  if (frame_no > lead && *L->h_progress < frame_no - lead) {
    const auto tw = std::chrono::steady_clock::now();
    int polls = 0;
    while (*L->h_progress < frame_no - lead) {
      if ((++polls & 255) == 0 && hipStreamQuery(st) == hipSuccess && *L->h_progress < frame_no - lead) break;  // (idle stream: a failed launch)
      std::this_thread::sleep_for(std::chrono::microseconds(30));
    }
    pl->host_ms_wait += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw).count();
  }
  double* pt = (double*)pin;
  double* pi = pt + S;
  const uint8_t** ptab = (const uint8_t**)(pi + (size_t)S * IMU_MAX * 7);
  int* pn = (int*)(ptab + 2);
  int* ppres = (int*)((uint8_t*)pin + L->in_off_pres);
  // presence: the stream's word in the table (read by k_frame_head, k_frame_end and the left image's ingest); a lane whose streams all
  // have a frame passes nullptr, the form of a plain flvis_image_feed
  int n_present = S;
  if (present) {
    n_present = 0;
    for (int s = 0; s < S; s++) n_present += (ppres[s] = present[s] ? 1 : 0);
  }
  const bool all_present = n_present == S, none_present = n_present == 0;
  memcpy(pt, h_times, sizeof(double) * S);
  // only the staged samples travel (the block keeps its layout: [S][IMU_MAX][7])
  for (int s = 0; s < S; s++)
    memcpy(pi + (size_t)s * IMU_MAX * 7, &L->h_imu[(size_t)s * IMU_MAX * 7], sizeof(double) * 7 * L->h_nimu[s]);
  ptab[0] = d_img0;
  ptab[1] = d_img1;
  memcpy(pn, L->h_nimu.data(), sizeof(int) * S);
  std::fill(L->h_nimu.begin(), L->h_nimu.end(), 0);
  cmd_pending = L->cmd_since_frame;
  L->cmd_since_frame = false;
  // No copy: k_frame_head reads the block where the host staged it (page-locked, mapped into the device's address space: a few KB per
  // stream over PCIe, in parallel over the streams), and the image bases travel as kernel arguments.  A staging slot is rewritten PIN_RING
  // frames later, when the frame that read it is long over (the host-lead wait above).  Copying forms: profiles/r04_lk_ab.md.  (The copy
  // below only serves a runtime that maps no device pointer for the staging slot.)
  zerocopy = L->pinned_dev[pslot] != nullptr;
  L->h_tab[0] = d_img0, L->h_tab[1] = d_img1;
  p.in_img1 = d_img1;
  {
    uint8_t* din = zerocopy ? L->pinned_dev[pslot] : L->d_inputs;
    L->d_time = reinterpret_cast<double*>(din);
    p.imu_in = reinterpret_cast<double*>(din + L->in_off_imu);
    p.n_imu = reinterpret_cast<int*>(din + L->in_off_n);
    p.present = all_present ? nullptr : reinterpret_cast<const int*>(din + L->in_off_pres);
  }
  if (!zerocopy) hipMemcpyAsync(L->d_inputs, pin, L->input_bytes, hipMemcpyHostToDevice, st);
  // ---- what the fixed kernel sequence of this frame is made of
  prof = pl->prof_cap > 0 && pl->prof_step < pl->prof_cap;
  pev = prof ? &L->prof_ev[(size_t)pl->prof_step * (2 * PROF_STAGES)] : nullptr;
  prof18 = (prof && ((pl->prof_mask >> 18) & 1ull)) ? &pev[2 * 18] : nullptr;
  skipped = pl->frames_fed < (long long)pl->cfg.skip_first_n_imgs;
  // a step in which no stream of the lane has a frame runs as a skipped one (the IMU, and k_frame_end, which writes nothing for an absent
  // stream) -- plus the local map, which goes on with the keyframes queued before.  (While frames_fed < skip_first_n_imgs every stream that
  // has a frame is in its skip window, whichever steps it was absent from: the skipped form holds with presence too.)
  idle_step = skipped || none_present;
  first_processed = pl->frames_fed == (long long)pl->cfg.skip_first_n_imgs;
  depth_cam = pl->cfg.cam_type == CAM_DEPTH;  // the second image is the Z16 depth map, read in place
  eq = pl->cfg.need_equal_hist != 0;
  // rows of whole 16-byte lanes at 16-byte aligned bases (the walking kernels' dwordx4 loads); otherwise (KITTI: 1241 x 376 tightly packed
  // rows, or a caller's buffer at an odd offset) both images are copied into pitch-aligned level 0
  aligned = (w & 15) == 0 && !(((uintptr_t)d_img0 | (depth_cam ? (uintptr_t)0 : (uintptr_t)d_img1)) & 15);
  // The right image is only read within this frame: without equalizeHist the caller's buffer IS level 0 of the right pyramid (no copy;
  // that level then has no border, and the few stereo search regions that leave the image at level 0 are staged by the kernel's
  // index-reflecting path; a bordered copy: DESIGN.md section 4).
  r_in_place = !eq && aligned;
  in0 = img_plain(d_img0), in1 = img_plain(d_img1);  // (kernel arguments: no graph is captured)
  l0cur = ImgSel{{L->pyr0[0][0], L->pyr0[1][0]}, p.img_slot, 0, nullptr};
  // the staged IMU samples and frame_begin take the temporal tracker's inputs into the same launch unless the local-map feedback has to be
  // applied in between (FLVIS_HEAD_PREPARE=0, A/B knob: two launches)
  head_prepare = pl->head_prepare && !pl->feedback_used && !idle_step;
  // FLVIS_CHAIN_MERGE (round 6; bits, default 31): launches of the frame's chain folded into their neighbours -- every launch on the chain
  // costs dispatch, ramp and drain whatever it computes (1-3 us between two one-workgroup-per-stream kernels, ~8 us around LK).
  // Bit 0: k_add_new + k_depth_seeds as one launch (a barrier between them);
  // bit 1: k_track_collect as the prologue of k_ransac_f (and by sixteen waves instead of one).  0: rounds 1-5's launches.
  // Bit 2: k_depth_innovate + k_frame_end as one launch of NMAX threads -- in a step in which every stream has a frame; an absent stream
  // and an idle step keep the stand-alone k_frame_end.  Bit 3: k_feature_dem in front of k_add_new (+ k_depth_seeds with bit 0) in their
  // launch.  Bit 4: k_reproj_filter as the epilogue of k_pose_lm, by its 256 threads.  (profiles/r26_chain_folds.md)
  merge_collect = (pl->chain_merge & 2) != 0;
  merge_end = (pl->chain_merge & 4) != 0 && !idle_step && all_present;
  merge_dem = (pl->chain_merge & 8) != 0;
  merge_filter = (pl->chain_merge & 16) != 0;
}

// left image -> level 0 of the slot this frame is going to use (+ the pyramid), on the detection stream BESIDE k_frame_head (the two
// swapped: profiles/r05_local_map_cost.md): the slot was fixed when the previous frame ended (img_slot_in), so the image work does not
// wait for the IMU integration and the state machine (one thread per stream, 45 us).  Every present stream's image is ingested, also that
// of a stream this frame leaves idle.  Without equalizeHist the first pyrDown reads the caller's image and writes level 0 and level 1 in
// one pass; with it the equalised image is level 0.
void Frame::stage_ingest_left() {
  ImgSel l0in{{L->pyr0[0][0], L->pyr0[1][0]}, p.img_slot_in, 0, nullptr};
  // what the detection stream needs from the main one here is k_frame_end of the previous frame (the slot the image goes to) and, in
  // the copying mode, the upload of the input table: a signal of its own -- or, folded, the word the last k_frame_end stored itself
  // (only where nothing can have been enqueued on the main stream since that k_frame_end: between the steps of one flvis_run_steps call,
  // and for host images that arrive through the copy stream -- a caller of flvis_image_feed may have produced its images on this stream)
  if (pl->fold_joins && zerocopy && L->endf_valid && pl->chain_continuous) {
    join_wait(pl, L, ds, J_ENDF);
  } else {
    join_signal(pl, L, J_LM, st);  // (the frame's input table has been uploaded)
    join_wait(pl, L, ds, J_LM);
  }
  // host images (flvis_image_feed_host, single-lane stereo): the upload's signal is waited for by the stream that ingests the left image; the
  // main stream only sees the joins it has anyway (left pyramid in front of the temporal LK, right pyramid in front of the stereo LK)
  if (pl->up_event) hipStreamWaitEvent(ds, pl->up_event, 0);
  if (pl->up_flag) launch_wait_flag(ds, pl->up_flag, Pipeline::HostFeed::FLAG_WORDS, pl->up_seq, L->d_progress + 2);
  pb(1, ds);
  // (an absent stream's workgroups retire at once: its image is not read, the slots of its pyramid are not written)
  const int* pg = p.present;
  if (eq) launch_equalize_hist(ds, in0, l0in, w, h, w, pl->lpitch[0], (size_t)w * h, pl->lstride[0], S, L->eq_hist, L->eq_lut, pg);
  else if (!aligned) launch_copy_image_any(ds, in0, l0in, w, h, w, pl->lpitch[0], (size_t)w * h, pl->lstride[0], S, pg);
  pe(1, ds);
  pb(2, ds);
  // the borders of the levels: written by the pyrDown kernel that produces the level (every pixel also goes to the border positions
  // that mirror it); k_pyr_border only for what is left (level 0 when another kernel makes it, levels smaller than the border)
  PyrSel pyl;
  fill_pyr(pl, pyl, L->pyr0[0], L->pyr0[1], p.img_slot_in, 0, pl->levels);
  unsigned border_left = pyramid_levels(ds, pl->lbx != 0, in0, w, (size_t)w * h, !eq && aligned, true, pyl, S, pg);
  if (pl->levels == 0 && !eq && aligned) launch_copy_image(ds, in0, l0in, w, h, w, pl->lpitch[0], (size_t)w * h, pl->lstride[0], S, pg);
  if (border_left) launch_pyr_border(ds, pyl, S, pg, border_left);
  pe(2, ds);
  join_signal(pl, L, J_IMG, ds);
}

// the staged IMU samples, then frame_begin (and the temporal tracker's inputs: Frame::head_prepare)
void Frame::stage_head() {
  pb(0, st);
  bool head_signals;
  {
    LaunchJoins j(pl, L, st, p.kj);
    head_signals = !pl->feedback_used && j.fold_signal(J_HEAD);  // (the head kernel is the last one in front of the signal)
    // ... and it does not end before the left pyramid is there (the temporal LK follows it, directly or behind k_track_prepare)
    head_posts = !idle_step && j.fold_post(J_IMG);
    if (head_prepare) launch_frame_head_prepare(st, p, L->d_time, L->d_progress, frame_no);
    else launch_frame_head(st, p, L->d_time, L->d_progress, frame_no);
  }
  if (pl->feedback_used) launch_apply_correction(st, p);  // STEP1 of the Tracking case (local-map feedback, opt-in)
  pe(0, st);
  // the detection stream's kernels that read what k_frame_head decides (act_img, gftt_act, gftt_maxc, img_slot) wait for this signal:
  // the corner detection and the right pyramid (they start behind the F-RANSAC anyway)
  if (!head_signals) join_signal(pl, L, J_HEAD, st);
}

// behind k_frame_end: the local-map launch for the lane (or, without a local map, the keyframe queues' drop); `timed`: stage 18's pair.
// The local-map launch for the keyframes of frame n is enqueued inside frame n + 1, behind its PnP RANSAC, where the ~0.3 ms in which two
// launches hold CUs fall on the one-workgroup-per-stream geometry kernels (other placements: profiles/r05_local_map_cost.md).  Only
// between the steps of one flvis_run_steps call -- the next frame is known to follow at once; a per-frame caller (the ROS wrapper) gets
// its local-map launch when its frame ends, and so does the last step of a batch.
void Frame::local_map_tail(hipEvent_t* p18, bool timed) {
  if (with_local_map && (pl->frames_fed % pl->ba_every) == 0) {
    if (L->ba_pending) launch_local_map(pl, L, J_FE, true, nullptr);  // (a deferred launch this frame had no place for: skipped frames)
    if (pl->defer_ba) L->ba_pending = true;
    else if (L->endf_valid) launch_local_map(pl, L, J_ENDF, false, p18);  // (k_frame_end has stored the word itself)
    else launch_local_map(pl, L, J_FE, true, p18);
  } else if (!with_local_map) {
    // without a local map nobody consumes the keyframe queue: drop what frame_end appended (and apply a reset command queued since the
    // last frame: k_kfq_drop)
    // (a reset command is applied to the window here: behind the lane's last local-map launch, so that no workgroup of it owns the window)
    if (cmd_pending) {
      if (L->ba_launches > 0) join_wait(pl, L, st, J_BA(L->ba_launches - 1));
      launch_kfq_drop(st, p);
    } else hipMemcpyAsync(p.kfq_head, p.kfq_tail, sizeof(unsigned) * S, hipMemcpyDeviceToDevice, st);
    if (timed) {
      pb(18, st);
      pe(18, st);
      L->prof18_rec[(size_t)pl->prof_step] = 1;
    }
  }
}

// k_frame_end, behind the keyframe queues' back-pressure where it may append keyframes; it stores J_ENDF's word itself where the joins
// are folded (Lane::endf_valid)
// with_innovate (Frame::merge_end): k_depth_innovate's work in front of it in the same launch, which then also waits for the two-view
// triangulation; stage 16 is the launch, stage 17 reads ~0.  The older of the back-pressure waits went into an earlier launch
// (stage_new_landmarks): the launch has two wait slots.
void Frame::frame_end(bool backpressure, bool with_innovate) {
  LaunchJoins j(pl, L, st, p.kj);
  if (with_innovate) j.wait(J_TRI);
  if (backpressure) lane_backpressure_wait(pl, L, &j, 0, with_innovate ? 1 : pl->nba_lane);
  pb(with_innovate ? 16 : 17, st);
  L->endf_valid = j.fold_signal(J_ENDF);
  if (with_innovate) launch_depth_innovate_end(st, p);
  else launch_frame_end(st, p);
  j.end();
  if (with_innovate) {
    pe(16, st);
    pb(17, st);
  }
  pe(17, st);
  pe(19, st);
}

// the reference drops the first skip_first_n_imgs frames before any processing (vo_tracking.cpp image callback): every
// stream is idle for this frame, so only the IMU filter, the frame counter and the per-frame outputs are advanced
void Frame::stage_idle_tail() {
  frame_end(false, false);
  if (prof)
    for (int i = 1; i < PROF_STAGES; i++)
      if (i != 17 && i != 19) {
        pb(i, st);
        pe(i, st);
      }
  // no stream of the lane has a frame: the keyframes queued before this step keep being optimised (the skip window's steps come before
  // any keyframe)
  if (!skipped) local_map_tail(nullptr, false);
}

// What the temporal (stats_at 36, tc_mode 2) and the stereo launch (48, tc_mode 1) of k_lk_track share
// (one min_eig for both: the template cache holds a level's 1 / D only where the level passed the STEREO launch's tests, lk_kernel.hip)
LKParams Frame::lk_params(int stats_at, int tc_mode, int order) const {
  LKParams prm{30, 1e-3 * 1e-3, 1e-4f, 1};
  if (pl->lk_stats) prm.stats = reinterpret_cast<unsigned long long*>(p.counters) + stats_at;  // counters[36 .. 47] / [48 .. 59]
  if (pl->lk_stats) prm.stats_tc = reinterpret_cast<unsigned long long*>(p.counters) + 61;      // both launches: counters[61 .. 63]
  // the template cache: the stereo matcher stores its templates for the next frame's temporal tracker (same image, same pixel), which takes
  // them instead of computing them
  if (L->tc) {
    prm.tc = L->tc;
    prm.tc_mode = tc_mode;
    prm.tc_cap = p.tc_cap;
    prm.tc_stride = L->tc_stride;
    prm.tc_slot = p.lk_slot;
    prm.tc_tag = p.lk_tag;
  }
  prm.dbg_slot = (int)(pl->frames_fed & 7);
  prm.order = order;
  return prm;
}

void Frame::stage_temporal_lk() {
  // lanes out of phase: a lane's first processed frame starts when the previous lane has finished the temporal LK of its own, so
  // that from then on the image kernels of one lane overlap the one-workgroup-per-stream geometry chain of another
  if (first_processed && L->idx > 0) hipStreamWaitEvent(st, pl->lanes[L->idx - 1]->ev_stagger, 0);
  // (the guesses of the temporal tracker only need the state frame_begin left)
  pb(3, st);
  if (!head_prepare) launch_track_prepare(st, p);
  pe(3, st);
  if (!head_posts) join_wait(pl, L, st, J_IMG);  // join: the left pyramid
  pb(4, st);
  PyrSel prev, next;
  fill_pyr(pl, prev, L->pyr0[0], L->pyr0[1], p.img_slot, 1, pl->levels_t);
  fill_pyr(pl, next, L->pyr0[0], L->pyr0[1], p.img_slot, 0, pl->levels_t);
  launch_lk_track(st, prev, next, p.prev_pts, p.next_pts, p.lk_status, p.lk_count, NMAX, S, lk_params(36, 2, 0), p.act_track, pl->max_pts, 1);
  pe(4, st);
}

void Frame::stage_collect_ransac_f() {
  pb(5, st);
  if (!merge_collect) launch_track_collect(st, p);
  pe(5, st);
  if (first_processed && pl->lanes.size() > 1) hipEventRecord(L->ev_stagger, st);
  pb(6, st);
  {
    LaunchJoins j(pl, L, st, p.kj);
    j.signal(J_LM);
    launch_ransac_f(st, p, merge_collect);
    pe(6, st);
  }
}

// fork, behind the F-RANSAC: the corner detection of the new left image (speculative for tracking frames: used only if tracking
// succeeds), then the right pyramid (first used by the stereo matcher), on the detection stream beside the PnP RANSAC / pose
// optimisation -- latency chains on 64 CUs that leave the rest of the chip to the detection (other placements and orders:
// profiles/r03_stream_structure_ab.md)
void Frame::stage_detection_fork() {
  // (the head kernel's word first: that wait is over long before the F-RANSAC ends, and the corner detection starts behind the F-RANSAC's
  // word at once -- the other way round a k_wait_flag launch, ~5 us, stood between them on the frame's longer arm.  It also covers the
  // right pyramid below: same stream, same word.  profiles/r26_chain_folds.md)
  join_wait(pl, L, ds, J_HEAD);
  join_wait(pl, L, ds, J_LM);
  launch_gftt(ds, l0cur, w, h, pl->lpitch[0], pl->lstride[0], S, L->gftt, nullptr, p.cam.gftt_ql, p.gftt_maxc, p.cam.gftt_num,
              (double)p.cam.gftt_dis, L->gftt_xy, L->gftt_n, 2 * p.cam.gftt_num, p.gftt_act,
              (prof && ((pl->prof_mask >> 10) & 7ull) == 7ull) ? &pev[2 * 10] : nullptr, false);
  {  // FeatureDEM's image part (regions, Harris scores, per-region order of the corners) follows at once, off the critical path
    KJoin prep_kj{};
    LaunchJoins j(pl, L, ds, prep_kj);
    j.signal(J_GFTT);
    launch_feature_dem_prep(ds, l0cur, w, h, pl->lpitch[0], pl->lstride[0], S, p.cam.dem, L->gftt_xy, L->gftt_n, 2 * p.cam.gftt_num,
                            p.gftt_act, L->dem_sorted, L->dem_roff, &prep_kj);
  }
  if (!depth_cam) {
    if (eq) launch_equalize_hist(ds, in1, img_plain(L->pyr1[0]), w, h, w, pl->lpitch[0], (size_t)w * h, pl->lstride[0], S, L->eq_hist, L->eq_lut, p.act_img);
    else if (!aligned) launch_copy_image_any(ds, in1, img_plain(L->pyr1[0]), w, h, w, pl->lpitch[0], (size_t)w * h, pl->lstride[0], S, p.act_img);
    PyrSel pyr_r;
    fill_pyr(pl, pyr_r, L->pyr1, nullptr, nullptr, 0, pl->levels);
    unsigned border_left = pyramid_levels(ds, pl->lbx != 0, in1, w, (size_t)w * h, false, !r_in_place, pyr_r, S, p.act_img);
    if (border_left) launch_pyr_border(ds, pyr_r, S, p.act_img, border_left);
  }
  join_signal(pl, L, J_DET, ds);
}

void Frame::stage_pnp_pose() {
  pb(7, st);
  const bool ba_here = L->ba_pending;
  bool pnp_signals;
  {
    LaunchJoins j(pl, L, st, p.kj);
    pnp_signals = ba_here && j.fold_signal(J_FE);  // (the deferred local-map launch starts behind this kernel)
    launch_ransac_pnp(st, p);
  }
  if (p.pnp_tail_cv) launch_pnp_tail_cv(st, p);
  pe(7, st);
  if (ba_here) launch_local_map(pl, L, J_FE, !pnp_signals, prof18);
  pb(8, st);
  if (merge_filter) {  // (stage 9 reads ~0)
    LaunchJoins j(pl, L, st, p.kj);
    j.signal(J_LM);
    launch_pose_lm_filter(st, p);
    pe(8, st);
    pb(9, st);
    pe(9, st);
  } else {
    launch_pose_lm(st, p);  // (with k_track_post's work in its prologue)
    pe(8, st);
    pb(9, st);
    LaunchJoins j(pl, L, st, p.kj);
    j.signal(J_LM);
    launch_reproj_filter(st, p);
    pe(9, st);
  }
  // the IMU filter's correction from this frame's pose: on the detection stream (joined with the triangulation before the depth innovation)
  join_wait(pl, L, ds, J_LM);
  launch_vi_correction(ds, p);
}

void Frame::stage_new_landmarks() {
  // join: FeatureDEM (init: detect, tracking: redetect) consumes the corners; the right pyramid is joined before the stereo LK
  if (!merge_dem) {
    KJoin dem_kj{};
    LaunchJoins j(pl, L, st, dem_kj);
    j.wait(J_GFTT);
    pb(13, st);
    launch_feature_dem(st, w, h, S, p.cam.dem, L->dem_sorted, L->dem_roff, 2 * p.cam.gftt_num, p.det_mode, p.exist_xy, p.n_exist, NMAX,
                       p.new_xy, p.n_new, NEW_MAX, &dem_kj);
  }
  const bool merge_seeds = (pl->chain_merge & 1) != 0;  // (k_add_new_seeds carries both launches' joins)
  const DemLaunch dem{w, h, L->dem_sorted, L->dem_roff, 2 * p.cam.gftt_num};
  bool an_signals, seeds_post;
  {
    LaunchJoins j(pl, L, st, p.kj);
    if (merge_dem) {  // (FeatureDEM in k_add_new's launch: the launch waits for the corners)
      j.wait(J_GFTT);
      pb(13, st);
    }
    // the merged frame end has one wait slot left behind the triangulation's: the keyframe queues' older back-pressure wait is this launch's
    if (merge_end && with_local_map) lane_backpressure_wait(pl, L, &j, 1, pl->nba_lane);
    // k_add_new (one wave per stream) stores the word the two-view triangulation waits for: that kernel reads the landmarks as k_add_new
    // leaves them and nothing k_depth_seeds writes
    // (k_depth_seeds and k_depth_triangulate store no word themselves: 256 workgroups each -- every workgroup's release is a write-back of its
    // XCD's L2, and beside the stereo LK's template stores the kernels doubled their time: 5.9 -> 12.7 us, 87 -> 180 us)
    an_signals = j.fold_signal(J_LM);
    if (!merge_seeds) {
      if (merge_dem) launch_dem_add_new_seeds(st, p, dem, false);
      else launch_add_new(st, p);
      j.end();
    }
    pe(13, st);
    // depth innovation: stereo LK img0 -> img1 + DLT + IIR
    pb(14, st);
    // ... and k_depth_seeds does not end before the right pyramid is there (the stereo LK follows it)
    seeds_post = j.fold_post(J_DET);
    if (!merge_seeds) launch_depth_seeds(st, p);
    else if (merge_dem) launch_dem_add_new_seeds(st, p, dem, true);
    else launch_add_new_seeds(st, p);
  }
  pe(14, st);
  // the two-view triangulation that k_depth_innovate consumes: on the detection stream (idle by now), under the stereo LK
  if (!an_signals) join_signal(pl, L, J_LM, st);
  join_wait(pl, L, ds, J_LM);
  launch_depth_triangulate(ds, p);
  join_signal(pl, L, J_TRI, ds);
  if (!seeds_post) join_wait(pl, L, st, J_DET);
}

void Frame::stage_stereo_depth() {
  pb(15, st);
  if (!depth_cam) {
    PyrSel prev, next;
    fill_pyr(pl, prev, L->pyr0[0], L->pyr0[1], p.img_slot, 0, pl->levels_s);
    fill_pyr(pl, next, L->pyr1, nullptr, nullptr, 0, pl->levels_s);
    next.lvl[0] = r_in_place ? in1 : img_plain(L->pyr1[0]);
    next.pitch[0] = r_in_place ? w : pl->lpitch[0];
    next.stride[0] = r_in_place ? (size_t)w * h : pl->lstride[0];
    if (r_in_place) next.bx[0] = next.by[0] = 0;  // the caller's buffer has no border
    // order 1: the frame's new landmarks, which have no depth to start from, first (profiles/r06_chain_ab.md)
    launch_lk_track(st, prev, next, p.prev_pts, p.next_pts, p.lk_status, p.lk_count, NMAX, S, lk_params(48, 1, 1), p.det_mode, pl->max_pts, 2);
  }
  pe(15, st);
  if (merge_end) return;  // (the depth innovation is the head of the frame's last launch: frame_end)
  LaunchJoins j(pl, L, st, p.kj);
  j.wait(J_TRI);
  pb(16, st);
  launch_depth_innovate(st, p);
  j.end();
  pe(16, st);
}

void Frame::stage_frame_end() {
  frame_end(with_local_map != 0, merge_end);
  // the keyframe log (opt-in): the streams that made a keyframe in this frame keep its message; in stream order behind k_frame_end, ahead
  // of everything of the next step that overwrites what the kernel reads (kf_log.hip)
  if (pl->kfl.cap > 0) kf_log_frame(pl, L, st, in1.b[0], depth_cam || r_in_place);
  local_map_tail(prof18, prof);
}

}  // namespace

// One frame of one lane: stages the lane's host inputs, uploads them as one block and enqueues the fixed kernel sequence
// on the lane's streams.  d_img0 / d_img1 already point at the lane's first stream.
// present: the lane's slice of the step's presence bytes (flvis_image_feed_present), nullptr when every stream has a frame.
static void lane_frame(Pipeline* pl, Lane* L, const uint8_t* d_img0, const uint8_t* d_img1, const double* h_times, const uint8_t* present,
                       int with_local_map) {
  Frame f{pl, L, L->pipe, L->st, L->det_stream, L->S, pl->cfg.image_width, pl->cfg.image_height, with_local_map};
  f.stage_host_inputs(d_img0, d_img1, h_times, present);
  f.pb(19, f.st);  // the whole main-stream chain of this frame: per-frame GPU latency (p50/p99 in bench.py)
  if (!f.idle_step) f.stage_ingest_left();  // detection stream
  f.stage_head();
  if (f.idle_step) return f.stage_idle_tail();
  f.stage_temporal_lk();
  f.stage_collect_ransac_f();
  f.stage_detection_fork();    // detection stream: gftt, FeatureDEM's image part, the right pyramid
  f.stage_pnp_pose();          // PnP RANSAC + the deferred local-map launch + pose LM + reprojection filter
  f.stage_new_landmarks();     // FeatureDEM + new landmarks + depth seeds (+ the triangulation on the detection stream)
  f.stage_stereo_depth();      // stereo LK + depth innovation
  f.stage_frame_end();         // back-pressure + k_frame_end + the local-map launch
}

extern "C" {

int flvis_image_feed(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, const double* h_times,
                     flvis_frame_out* h_out, int with_local_map) {
  return flvis_image_feed_present(ctx, d_img0, d_img1, h_times, nullptr, h_out, with_local_map);
}

// h_present (may be NULL: every stream): the streams that have a frame in this step (include/flvis_hip.h)
int flvis_image_feed_present(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, const double* h_times, const uint8_t* h_present,
                             flvis_frame_out* h_out, int with_local_map) {
  if (!ctx || !ctx->pipe || !d_img0 || !d_img1 || !h_times) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (h_present) {
    bool all = true;
    for (int s = 0; s < pl->S && all; s++) all = h_present[s] != 0;
    if (all) h_present = nullptr;  // (the plain step)
  }
  hipSetDevice(ctx->device);
  const size_t img_px = (size_t)pl->cfg.image_width * pl->cfg.image_height;
  const size_t img1_bytes = img_px * (pl->cfg.cam_type == CAM_DEPTH ? 2 : 1);
  const bool multi = pl->lanes.size() > 1;
  const auto t_host0 = std::chrono::steady_clock::now();
  // the caller's images were produced on the context's stream; lanes with their own streams wait for them, and the
  // context's stream waits for the lanes afterwards, so that the caller may recycle its buffers in stream order -- the buffers
  // of THIS frame by default, those handed over input_hold frames ago when the caller cycles through more buffers
  // (flvis_set_input_hold): only then can the lanes drift apart by more than a frame
  if (multi) hipEventRecord(pl->ev_in, ctx->stream);
  for (Lane* L : pl->lanes) {
    if (multi) hipStreamWaitEvent(L->st, pl->ev_in, 0);
    lane_frame(pl, L, d_img0 + (size_t)L->s0 * img_px, d_img1 + (size_t)L->s0 * img1_bytes, h_times + L->s0,
               h_present ? h_present + L->s0 : nullptr, with_local_map);
    if (multi) {
      hipEventRecord(L->ev_end[pl->frames_fed % Lane::HOLD_RING], L->st);
      const long long rel = pl->frames_fed - pl->input_hold;
      if (rel >= 0) hipStreamWaitEvent(ctx->stream, L->ev_end[rel % Lane::HOLD_RING], 0);
    }
  }
  pl->host_ms_total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  const bool prof = pl->prof_cap > 0 && pl->prof_step < pl->prof_cap;
  if (prof) pl->prof_step++;
  pl->frames_fed++;
  if (h_present) {
    for (int s = 0; s < pl->S; s++) pl->stream_frames += h_present[s] != 0;
  } else {
    pl->stream_frames += pl->S;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx->hip_fail(e, "image_feed launch");
  if (h_out) {
    static_assert(sizeof(flvis_frame_out) == sizeof(FrameOut), "FrameOut layout");
    for (Lane* L : pl->lanes) {
      e = hipMemcpyAsync(h_out + L->s0, L->pipe.out, sizeof(FrameOut) * L->S, hipMemcpyDeviceToHost, L->st);
      if (e != hipSuccess) return ctx->hip_fail(e, "image_feed readback");
    }
    for (Lane* L : pl->lanes) {
      e = hipStreamSynchronize(L->st);
      if (e != hipSuccess) return ctx->hip_fail(e, "image_feed readback");
    }
  }
  return FLVIS_OK;
}


int flvis_imu_feed_all(flvis_ctx* ctx, const int* h_counts, const double* h_samples, int samples_per_stream) {
  if (!ctx || !ctx->pipe || !h_counts || !h_samples || samples_per_stream <= 0) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  for (int s = 0; s < pl->S; s++) {
    int n = h_counts[s];
    if (n < 0 || n > samples_per_stream) return ctx->fail(FLVIS_ERR_INVALID_ARG, "imu_feed_all: bad count");
    int rc = flvis_imu_feed_flvis_frame(ctx, s, n, h_samples + (size_t)s * samples_per_stream * 7);
    if (rc) return rc;
  }
  return FLVIS_OK;
}

// The caller's per-frame loop (IMU samples, then the stereo pair) for n_steps frames in ONE call: a driver that feeds frames already
// resident in HBM -- a replay, bench.py's timed region, one rank of a multi-GPU job -- does not come back to its host language between
// frames (eight Python interpreters on one host contending for cores are then not on the path).
int flvis_run_steps(flvis_ctx* ctx, int n_steps, const flvis_step* steps, int with_local_map, double* h_call_ms) {
  return flvis_run_steps_present(ctx, n_steps, steps, nullptr, with_local_map, h_call_ms);
}

// h_present (may be NULL: every stream in every step): [n_steps][n_streams], row k for step k as flvis_image_feed_present takes it
int flvis_run_steps_present(flvis_ctx* ctx, int n_steps, const flvis_step* steps, const uint8_t* h_present, int with_local_map,
                            double* h_call_ms) {
  if (!ctx || !ctx->pipe || n_steps < 0 || (n_steps > 0 && !steps)) return FLVIS_ERR_INVALID_ARG;
  for (int k = 0; k < n_steps; k++) {
    const flvis_step& f = steps[k];
    const auto t0 = std::chrono::steady_clock::now();
    if (f.h_imu_counts) {
      const int rc = flvis_imu_feed_all(ctx, f.h_imu_counts, f.h_imu_samples, f.imu_samples_per_stream);
      if (rc != FLVIS_OK) return rc;
    }
    ctx->pipe->defer_ba = k + 1 < n_steps;
    ctx->pipe->chain_continuous = k > 0;
    const int rc = flvis_image_feed_present(ctx, f.d_img0, f.d_img1, f.h_times, h_present ? h_present + (size_t)k * ctx->pipe->S : nullptr,
                                            nullptr, with_local_map);
    ctx->pipe->defer_ba = false;
    ctx->pipe->chain_continuous = false;
    if (rc != FLVIS_OK) return rc;
    if (h_call_ms) h_call_ms[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return FLVIS_OK;
}

}  // extern "C"
