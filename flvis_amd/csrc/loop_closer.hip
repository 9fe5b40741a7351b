// flvis_amd: the loop-closing nodelet's control flow around the keyframe-rate kernels -- the caller of
// orb_kernels.hip / loop_kernels.hip, for a BATCH of independent sequences on one GPU:
//
//   flvis_loop_closer_add_keyframes  <- kfmsgProcess   src/backend/vo_loopclosing.cpp:191-391   ORB, bag of words, 3-D landmarks,
//                                                      T_c_w = T_c_w_odom * T_odom_map, the keyframe appended to the sequence's map
//   flvis_loop_closer_process        <- pgoProcess     :393-518   similarity row, the `size < 50` gate, isLoopCandidate (:520-590),
//                                                      isLoopClosureKF (:593-735), the loop list, the PGO trigger (:488-497),
//                                                      loopClosureOnCovGraphG2ONew (:742-944) and T_odom_map *= Tw1_w2 (:908)
//   flvis_loop_closer_localize_in    (the project's own) a query frame against a sequence's whole database, or all of them: the candidates
//                                                      are ranked across maps (flvis_hip_lc_select_maps), isLoopClosureKF's check on the n_best
//                                                      best-scoring keyframes with the query's camera, its pose in the map frame; stores nothing
//   flvis_loop_closer_localize       (the project's own) localize_in on the query's own sequence's map
//   flvis_loop_closer_link           (the project's own) localize_in with a STORED keyframe as the query: its database slot takes the query
//                                                      slot's place, no feature kernel runs; any number of queries, its own keyframes left out
//                                                      -- the three are one candidate search (lc_search) on queries that differ in where they
//                                                      come from
//   flvis_loop_closer_merge          (the project's own) several sequences' maps into one: loopClosureOnCovGraphG2ONew on the sequences'
//                                                      keyframes side by side, tied by links between keyframes of different sequences
//
// The keyframe database (bag-of-words vectors, compacted ORB descriptors with their pixels and 3-D positions, T_c_w) lives in HBM
// for the whole run -- 76 KB per keyframe -- and never returns to the host; per keyframe the host sees one similarity row, and per
// candidate three integers and a pose.  Integer / threshold logic stays on the host, as in the reference's pgoProcess thread.
// That thread looks at whatever keyframe is newest whenever it comes round (a keyframe can be looked at twice or never); here
// every keyframe is processed exactly once, in order (deterministic).  tf / path / image publishing is the ROS wrapper's business.
//
// A batch may hold one calibrated camera per sequence (flvis_loop_closer_create_rigs): the sequences' cameras are rows of one table
// resident on the device, which the two kernels that read a camera index by the sequence of their keyframe / candidate; and a
// sequence's slot can start over, also on another camera (flvis_loop_closer_reset[_rigs]) -- the host bookkeeping of Seq is all there
// is to empty, the slot's database entries are unreachable once Seq::n is 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "dense_stereo.hpp"
#include "kf_log.hpp"
#include "lc_traj.hpp"
#include "loop_kernels.hpp"
#include "map_cloud.hpp"
#include "occupancy.hpp"
#include "rectify.hpp"
#include "pipeline_host.hpp"

namespace {

constexpr int LCC_CAP = 1024;   // keypoints per keyframe (the reference extracts 1000) = correspondences per PnP set
constexpr int LCC_VCAP = 1024;  // bag-of-words entries per keyframe
constexpr size_t LCC_STAGE = 7 * sizeof(double) + 2 * sizeof(int);  // bytes per keyframe of an add call's one upload, per query of a localize call's
constexpr int LCC_NBEST = FLVIS_LC_FIX_CAND;                        // candidates per query of a localize call

// ---- pose7 = tx ty tz qx qy qz qw on the host (Sophus::SE3 products of :377, :908) -------------------------------------------
void q_mul(const double* a, const double* b, double* o) {  // Hamilton product, x y z w
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  const double z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = x, o[1] = y, o[2] = z, o[3] = w;
}
void q_rot(const double* q, const double* v, double* o) {  // R(q) v
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * (y * v[2] - z * v[1]), ty = 2 * (z * v[0] - x * v[2]), tz = 2 * (x * v[1] - y * v[0]);
  o[0] = v[0] + w * tx + (y * tz - z * ty);
  o[1] = v[1] + w * ty + (z * tx - x * tz);
  o[2] = v[2] + w * tz + (x * ty - y * tx);
}
void pose_mul(const double* a, const double* b, double* o) {  // T_a * T_b
  double t[3], q[4];
  q_rot(a + 3, b, t);
  q_mul(a + 3, b + 3, q);
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  o[0] = t[0] + a[0], o[1] = t[1] + a[1], o[2] = t[2] + a[2];
  o[3] = q[0] / n, o[4] = q[1] / n, o[5] = q[2] / n, o[6] = q[3] / n;
}

// ---- device helpers ---------------------------------------------------------------------------------------------------------
// copies the batch results of one add call into the keyframe slots of their sequences (slot = stream * maxkf + keyframe)
__global__ __launch_bounds__(256) void k_lcc_store(const int* __restrict__ slot, const int* __restrict__ ids, const double* __restrict__ vals,
                                                   const int* __restrict__ nnz, const float* __restrict__ lm2, const double* __restrict__ lm3,
                                                   const uint8_t* __restrict__ lmd, const int* __restrict__ lmc, const double* __restrict__ T,
                                                   int* db_ids, double* db_vals, int* db_nnz, float* db_lm2, double* db_lm3, uint8_t* db_lmd,
                                                   int* db_lmc, double* db_T) {
  const int i = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;  // t: element of the keyframe's row, 0..1023
  const size_t s = (size_t)slot[i];
  if (t >= LCC_CAP) return;
  const int nv = nnz[i], nl = lmc[i];
  if (t < 7) db_T[s * 7 + t] = T[(size_t)i * 7 + t];
  if (t < nv) {
    db_ids[s * LCC_VCAP + t] = ids[(size_t)i * LCC_VCAP + t];
    db_vals[s * LCC_VCAP + t] = vals[(size_t)i * LCC_VCAP + t];
  }
  if (t < nl) {
    const size_t a = (size_t)i * LCC_CAP + t, b = s * LCC_CAP + t;
    db_lm2[b * 2] = lm2[a * 2], db_lm2[b * 2 + 1] = lm2[a * 2 + 1];
    db_lm3[b * 3] = lm3[a * 3], db_lm3[b * 3 + 1] = lm3[a * 3 + 1], db_lm3[b * 3 + 2] = lm3[a * 3 + 2];
    const uint4* q = reinterpret_cast<const uint4*>(lmd + a * 32);
    uint4* r = reinterpret_cast<uint4*>(db_lmd + b * 32);
    r[0] = q[0], r[1] = q[1];
  }
  if (t == 0) db_nnz[s] = nv, db_lmc[s] = nl;
}

// descriptors of the two keyframes of every candidate pair into the contiguous arrays flvis_hip_orb_match reads
__global__ __launch_bounds__(256) void k_lcc_fetch(const int* __restrict__ slot_a, const int* __restrict__ slot_b, const uint8_t* __restrict__ db_lmd,
                                                   const int* __restrict__ db_lmc, uint8_t* a, int* na, uint8_t* b, int* nb) {
  const int i = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= LCC_CAP) return;
  const size_t sa = (size_t)slot_a[i], sb = (size_t)slot_b[i];
  const uint4 z = make_uint4(0, 0, 0, 0);
  const int ca = db_lmc[sa], cb = db_lmc[sb];
  const uint4* qa = reinterpret_cast<const uint4*>(db_lmd + (sa * LCC_CAP + t) * 32);
  const uint4* qb = reinterpret_cast<const uint4*>(db_lmd + (sb * LCC_CAP + t) * 32);
  uint4* oa = reinterpret_cast<uint4*>(a + ((size_t)i * LCC_CAP + t) * 32);
  uint4* ob = reinterpret_cast<uint4*>(b + ((size_t)i * LCC_CAP + t) * 32);
  oa[0] = t < ca ? qa[0] : z, oa[1] = t < ca ? qa[1] : z;
  ob[0] = t < cb ? qb[0] : z, ob[1] = t < cb ? qb[1] : z;
  if (t == 0) na[i] = ca, nb[i] = cb;
}

// cv::Point3f(kf0->lm_3d[queryIdx]), cv::Point2f(kf1->lm_2d[trainIdx]) of the selected matches (:643-652)
__global__ __launch_bounds__(256) void k_lcc_correspondences(const int* __restrict__ slot_a, const int* __restrict__ slot_b,
                                                             const int* __restrict__ pairs, const int* __restrict__ npairs,
                                                             const double* __restrict__ db_lm3, const float* __restrict__ db_lm2, float* p3d,
                                                             float* p2d) {
  const int i = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= LCC_CAP) return;
  const size_t o = (size_t)i * LCC_CAP + t;
  float x = 0.f, y = 0.f, z = 0.f, u = 0.f, v = 0.f;
  if (t < npairs[i]) {
    const size_t qa = (size_t)slot_a[i] * LCC_CAP + pairs[o * 2], qb = (size_t)slot_b[i] * LCC_CAP + pairs[o * 2 + 1];
    x = (float)db_lm3[qa * 3], y = (float)db_lm3[qa * 3 + 1], z = (float)db_lm3[qa * 3 + 2];
    u = db_lm2[qb * 2], v = db_lm2[qb * 2 + 1];
  }
  p3d[o * 3] = x, p3d[o * 3 + 1] = y, p3d[o * 3 + 2] = z;
  p2d[o * 2] = u, p2d[o * 2 + 1] = v;
}

// What a localize call brings back in ONE copy: per set (= query * n_best + rank) the candidate and its pair check, per query the counts.
// Laid out for the closer's capacity (ns_cap = n_streams * LCC_NBEST sets, q_cap = n_streams queries), whatever a call uses of it.
struct LcFixOut {
  double *score, *pose, *T_kf;  // [ns_cap], [ns_cap][7] the PnP pose, [ns_cap][7] the candidate's T_c_w in the database
  int *kf, *npairs, *ninl;      // [ns_cap] keyframe index (-1: an empty rank), matches, inliers
  int *ncand, *nlm;             // [q_cap] candidates, the query's kept landmarks
  static size_t bytes(size_t ns_cap, size_t q_cap) { return ns_cap * (15 * sizeof(double) + 3 * sizeof(int)) + q_cap * 2 * sizeof(int); }
  static LcFixOut at(void* base, size_t ns_cap, size_t q_cap) {
    LcFixOut o;
    o.score = (double*)base, o.pose = o.score + ns_cap, o.T_kf = o.pose + 7 * ns_cap;
    o.kf = (int*)(o.T_kf + 7 * ns_cap), o.npairs = o.kf + ns_cap, o.ninl = o.npairs + ns_cap;
    o.ncand = o.ninl + ns_cap, o.nlm = o.ncand + q_cap;
    return o;
  }
};

// The sets of a candidate search, one wave per query, from the candidates k_lc_select_maps (loop_kernels.hip) has chosen across maps: per
// set (= query * n_best + rank) what the pair check reads (side a the candidate's slot, side b the query's, the camera row the QUERY's
// sequence: solvePnPRansac needs the K of the camera that saw the pixels) and what the host gets back.  sel_idx is the candidate's database
// slot (sequence * maxkf + keyframe; -1: an empty rank) and goes to the host as it is; an empty rank gets the closer's empty slot on both
// sides (landmark count 0): its set is empty from k_lcc_fetch on.
// lmc: the queries' landmark counts, per query (the call's feature buffers) or, BY_SLOT, per database slot (a link call's stored queries).
template <bool BY_SLOT>
__global__ __launch_bounds__(64) void k_lcc_select_sets(const int* __restrict__ q_slot, const int* __restrict__ q_seq, const int* __restrict__ sel_idx,
                                                        const double* __restrict__ sel_score, const int* __restrict__ sel_cnt, int n_best,
                                                        int empty_slot, const int* __restrict__ lmc, const double* __restrict__ db_T, int* slot_a,
                                                        int* slot_b, int* cam_of, LcFixOut out) {
  const int i = blockIdx.x, lane = threadIdx.x;
  for (int r = 0; r < n_best; r++) {
    const int set = i * n_best + r;
    const int g = sel_idx[set];
    const bool more = g >= 0;
    const int ks = more ? g : empty_slot;
    if (lane < 7) out.T_kf[(size_t)set * 7 + lane] = more ? db_T[(size_t)ks * 7 + lane] : (lane == 6 ? 1.0 : 0.0);
    if (lane == 0) {
      slot_a[set] = ks;
      slot_b[set] = more ? q_slot[i] : empty_slot;
      cam_of[set] = q_seq[i];
      out.kf[set] = g;
      out.score[set] = sel_score[set];
    }
  }
  if (lane == 0) out.ncand[i] = sel_cnt[i], out.nlm[i] = lmc[BY_SLOT ? q_slot[i] : i];
}

using flvis::LcCam;
using flvis::LcCamUnrect;
using flvis::lc_cam_of_cfg;
using flvis::lc_cam_unrect_of_cfg;
using flvis::LcMergeSeq;

struct Seq {
  int n = 0;
  bool fresh = false;
  std::vector<double> T_odom;  // 7 per keyframe
  std::vector<double> stamp;   // 1 per keyframe, NaN: never set (flvis_loop_closer_set_keyframe_stamps, add_logged)
  int uploaded = 0;            // keyframes whose T_odom and stamp the map_poses tables on the device hold
  double T_odom_map[7] = {0, 0, 0, 0, 0, 0, 1};
  std::vector<int> loop_ids;       // (earlier, later) per loop
  std::vector<double> loop_poses;  // 7 per loop
  long long last_pgo = -5000;      // :141
};

}  // namespace

struct flvis_loop_closer {
  flvis_ctx* ctx = nullptr;
  std::vector<flvis_cfg> cfgs;  // per sequence; cam_type / w / h below are batch-wide
  flvis_lc_params prm;
  flvis_orb_params orb{1000, 1.2f, 8, 20};  // :242
  std::vector<int8_t> pattern;
  int S = 0, maxkf = 0, w = 0, h = 0, cam_type = 0, device = 0;
  // the sequences' cameras: [S] rows on the device, written in stream order from the pinned host copy (a reset does not wait)
  LcCam* h_cams = nullptr;
  LcCam* d_cams = nullptr;
  // ... and, on a STEREO_UNRECT closer alone, the rows the opt-in rule reads beside them (flvis_loop_closer_set_stereo_unrect), kept like
  // the first table: the switch may be thrown at any time the database is empty
  LcCamUnrect* h_ucams = nullptr;
  LcCamUnrect* d_ucams = nullptr;
  bool stereo_unrect = false;
  // keyframe database, [S * maxkf] slots; behind them one query slot per sequence (what a localize call holds of its query, stream s at
  // S * maxkf + s) and one slot that stays empty (S * maxkf + S: no landmarks, no words)
  int* db_ids = nullptr;
  double* db_vals = nullptr;
  int* db_nnz = nullptr;
  float* db_lm2 = nullptr;
  double* db_lm3 = nullptr;
  uint8_t* db_lmd = nullptr;
  int* db_lmc = nullptr;
  double* db_T = nullptr;  // [S][maxkf][7] T_c_w
  // per-call staging, [S] items
  float *kps = nullptr, *lm2 = nullptr, *p3d = nullptr, *p2d = nullptr;
  uint8_t *desc = nullptr, *da = nullptr, *db = nullptr, *mask = nullptr;
  int *cnt = nullptr, *ovf = nullptr, *ids = nullptr, *nnz = nullptr, *lmc = nullptr, *slot_a = nullptr, *na = nullptr,
      *nb = nullptr, *pairs = nullptr, *npairs = nullptr, *ninl = nullptr;
  uint8_t* stage = nullptr;  // one upload per add call: [n][7] poses, [n] slots, [n] sequences
  double *vals = nullptr, *lm3 = nullptr, *rows = nullptr, *pose = nullptr, *loop_pose = nullptr, *drift = nullptr, *stats = nullptr, *pgo_T = nullptr;
  // a candidate search (localize, localize_in, link): the result block (LcFixOut) and its host copy; sets_cap: the pair-check buffers
  // (slot_a .. mask) hold this many sets -- S until the first search
  uint8_t* fix_out = nullptr;
  std::vector<uint8_t> h_fix_out;
  int sets_cap = 0;
  // ... all allocated by the first search: the queries' score rows ([S][maxkf], one searched map per query; [S][S * maxkf] from the first
  // call that searches all maps on; mrows_cap: doubles -- `rows` is what similarity_row reports: not touched), the searched maps and the
  // sequences' keyframe counts ([2 S], one upload from h_in_stage), and what k_lc_select_maps leaves per set / per query
  double* mrows = nullptr;
  size_t mrows_cap = 0;
  int *in_stage = nullptr, *sel_idx = nullptr, *sel_cnt = nullptr;
  double* sel_score = nullptr;
  std::vector<int> h_in_stage;
  // merge, all allocated by its first call and regrown by a call that needs more: the batch of virtual sequences (mg_V_cap doubles), the
  // call's one upload (loop poses, row table, LcMergeSeq table; mg_stage_cap bytes) and what comes back in one copy (per group k_pgo's
  // drift [7] and stats [5], then per sequence its drift [7]; mg_out_cap doubles)
  double *mg_V = nullptr, *mg_out = nullptr;
  uint8_t* mg_stage = nullptr;
  size_t mg_V_cap = 0, mg_stage_cap = 0, mg_out_cap = 0;
  std::vector<uint8_t> h_mg_stage;
  std::vector<double> h_mg_out;
  // map_poses, allocated by its first call: T_odom [S][maxkf][7] and the stamps [S][maxkf], filled up to Seq::uploaded
  double *tj_T_odom = nullptr, *tj_stamps = nullptr;
  std::vector<void*> owned;
  std::vector<Seq> seq;
  std::vector<double> h_rows;
  std::vector<uint8_t> h_stage;

  template <class T>
  bool alloc(T*& p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return false;
    owned.push_back(q);
    p = (T*)q;
    return true;
  }
  // a larger buffer in place of p (contents dropped); the caller has waited for the stream
  template <class T>
  bool regrow(T*& p, size_t count) {
    void* const old = (void*)p;
    if (!alloc(p, count)) return false;
    owned.erase(std::find(owned.begin(), owned.end(), old));
    hipFree(old);
    return true;
  }
  // a buffer of at least `count` items, allocated on its first use (contents dropped); the caller has waited for the stream
  template <class T>
  bool reserve(T*& p, size_t& cap, size_t count) {
    if (cap >= count) return true;
    if (!(p ? regrow(p, count) : alloc(p, count))) return false;
    cap = count;
    return true;
  }
  int query_slot(int s) const { return S * maxkf + s; }
  int empty_slot() const { return S * maxkf + S; }
};

extern "C" {

// the LC_PARAS block of the yaml (vo_loopclosing.cpp:955-963)
int flvis_lc_params_load(const char* yaml_path, flvis_lc_params* prm, char* err, int errlen) {
  auto fail = [&](const std::string& m) {
    if (err && errlen > 0) snprintf(err, errlen, "%s", m.c_str());
    return (int)FLVIS_ERR_CONFIG;
  };
  if (!yaml_path || !prm) return FLVIS_ERR_INVALID_ARG;
  std::ifstream f(yaml_path);
  if (!f) return fail(std::string("cannot open ") + yaml_path);
  struct Key {
    const char* name;
    int* i;
    double* d;
    bool seen;
  } keys[] = {{"lcKFStart", &prm->lcKFStart, nullptr, false},   {"lcKFDist", &prm->lcKFDist, nullptr, false},
              {"lcKFMaxDist", &prm->lcKFMaxDist, nullptr, false}, {"lcKFLast", &prm->lcKFLast, nullptr, false},
              {"lcNKFClosest", &prm->lcNKFClosest, nullptr, false}, {"minPts", &prm->minPts, nullptr, false},
              {"ratioMax", nullptr, &prm->ratioMax, false},     {"ratioRansac", nullptr, &prm->ratioRansac, false},
              {"minScore", nullptr, &prm->minScore, false}};
  std::string line;
  while (std::getline(f, line)) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    const size_t colon = line.find(':');
    if (colon == std::string::npos) continue;
    std::string k = line.substr(0, colon);
    k.erase(0, k.find_first_not_of(" \t"));
    k.erase(k.find_last_not_of(" \t") + 1);
    for (Key& key : keys)
      if (k == key.name) {
        std::istringstream is(line.substr(colon + 1));
        double v;
        if (!(is >> v)) return fail(std::string("yaml key ") + key.name + " has no number");
        if (key.i) *key.i = (int)v;
        if (key.d) *key.d = v;
        key.seen = true;
      }
  }
  for (const Key& key : keys)
    if (!key.seen) return fail(std::string("yaml key ") + key.name + " is missing (loop-closing parameters)");
  return FLVIS_OK;
}

// the fields every sequence of a closer shares (they size buffers and pick the kernels' paths): null, or the name of the first that differs
static const char* lc_batch_field_mismatch(const flvis_loop_closer* lc, const flvis_cfg& c) {
  if (c.cam_type != lc->cam_type) return "cam_type";
  if (c.image_width != lc->w) return "image_width";
  if (c.image_height != lc->h) return "image_height";
  return nullptr;
}

int flvis_loop_closer_create_rigs(flvis_ctx* ctx, const flvis_cfg* cfgs, const flvis_lc_params* prm, int n_streams, int max_keyframes,
                                  const int8_t* h_orb_pattern, flvis_loop_closer** out) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!cfgs || !prm || !out || n_streams <= 0 || max_keyframes <= 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_create: bad args");
  *out = nullptr;
  if (ctx->voc_nodes < 2)
    return ctx->fail(FLVIS_ERR_CONFIG, "loop_closer_create: no vocabulary (flvis_hip_bow_load_vocabulary / flvis_hip_bow_set_vocabulary first)");
  if ((long long)n_streams * (max_keyframes + 1) + 1 > (1ll << 31) / LCC_CAP)  // keyframe, query and empty slots: int indices * LCC_CAP
    return ctx->fail(FLVIS_ERR_CAPACITY, "loop_closer_create: n_streams * max_keyframes is too large");
  hipSetDevice(ctx->device);
  flvis_loop_closer* lc = new flvis_loop_closer();
  lc->ctx = ctx, lc->device = ctx->device, lc->prm = *prm, lc->S = n_streams, lc->maxkf = max_keyframes;
  lc->w = cfgs[0].image_width, lc->h = cfgs[0].image_height, lc->cam_type = cfgs[0].cam_type;
  for (int s = 1; s < n_streams; s++)
    if (const char* f = lc_batch_field_mismatch(lc, cfgs[s])) {
      delete lc;
      return ctx->fail(FLVIS_ERR_CONFIG, "loop_closer_create_rigs: stream " + std::to_string(s) + ": batch-wide field " + f +
                                             " differs from the closer's (stream 0)");
    }
  lc->cfgs.assign(cfgs, cfgs + n_streams);
  if (h_orb_pattern) lc->pattern.assign(h_orb_pattern, h_orb_pattern + 1024);
  const size_t slots = (size_t)n_streams * max_keyframes, S = (size_t)n_streams, dbs = slots + S + 1;
  bool ok = lc->alloc(lc->db_ids, dbs * LCC_VCAP) && lc->alloc(lc->db_vals, dbs * LCC_VCAP) && lc->alloc(lc->db_nnz, dbs) &&
            lc->alloc(lc->db_lm2, dbs * LCC_CAP * 2) && lc->alloc(lc->db_lm3, dbs * LCC_CAP * 3) &&
            lc->alloc(lc->db_lmd, dbs * LCC_CAP * 32) && lc->alloc(lc->db_lmc, dbs) && lc->alloc(lc->db_T, dbs * 7) &&
            lc->alloc(lc->fix_out, LcFixOut::bytes(S * LCC_NBEST, S)) &&
            lc->alloc(lc->kps, S * LCC_CAP * 6) && lc->alloc(lc->desc, S * LCC_CAP * 32) && lc->alloc(lc->cnt, S) && lc->alloc(lc->ovf, S) &&
            lc->alloc(lc->ids, S * LCC_VCAP) && lc->alloc(lc->vals, S * LCC_VCAP) && lc->alloc(lc->nnz, S) &&
            lc->alloc(lc->lm2, S * LCC_CAP * 2) && lc->alloc(lc->lm3, S * LCC_CAP * 3) && lc->alloc(lc->lmc, S) &&
            lc->alloc(lc->slot_a, S * 3) && lc->alloc(lc->da, S * LCC_CAP * 32) &&
            lc->alloc(lc->db, S * LCC_CAP * 32) && lc->alloc(lc->na, S) && lc->alloc(lc->nb, S) && lc->alloc(lc->pairs, S * LCC_CAP * 2) &&
            lc->alloc(lc->npairs, S) && lc->alloc(lc->p3d, S * LCC_CAP * 3) && lc->alloc(lc->p2d, S * LCC_CAP * 2) &&
            lc->alloc(lc->mask, S * LCC_CAP) && lc->alloc(lc->ninl, S) && lc->alloc(lc->pose, S * 7) && lc->alloc(lc->rows, slots) &&
            lc->alloc(lc->loop_pose, slots * 7) && lc->alloc(lc->drift, S * 7) && lc->alloc(lc->stats, S * 5) && lc->alloc(lc->pgo_T, slots * 7) &&
            lc->alloc(lc->stage, S * LCC_STAGE) && lc->alloc(lc->d_cams, S) &&
            hipHostMalloc((void**)&lc->h_cams, S * sizeof(LcCam), hipHostMallocDefault) == hipSuccess;
  if (ok && lc->cam_type == 1)
    ok = lc->alloc(lc->d_ucams, S) && hipHostMalloc((void**)&lc->h_ucams, S * sizeof(LcCamUnrect), hipHostMallocDefault) == hipSuccess;
  if (ok) {
    for (int s = 0; s < n_streams; s++) lc_cam_of_cfg(cfgs[s], &lc->h_cams[s]);
    ok = hipMemcpyAsync(lc->d_cams, lc->h_cams, S * sizeof(LcCam), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    if (ok && lc->h_ucams) {
      for (int s = 0; s < n_streams; s++) lc_cam_unrect_of_cfg(cfgs[s], &lc->h_ucams[s]);
      ok = hipMemcpyAsync(lc->d_ucams, lc->h_ucams, S * sizeof(LcCamUnrect), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    }
    // the empty slot: its two counts are all that is ever read of it
    ok = ok && hipMemsetAsync(lc->db_lmc + slots + S, 0, sizeof(int), ctx->stream) == hipSuccess &&
         hipMemsetAsync(lc->db_nnz + slots + S, 0, sizeof(int), ctx->stream) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    hipStreamSynchronize(ctx->stream);
    for (void* p : lc->owned) hipFree(p);
    if (lc->h_cams) hipHostFree(lc->h_cams);
    if (lc->h_ucams) hipHostFree(lc->h_ucams);
    delete lc;
    return ctx->fail(FLVIS_ERR_HIP, "loop_closer_create: device allocation failed (76 KB per keyframe slot)");
  }
  lc->seq.resize(n_streams);
  lc->h_rows.resize(slots);
  lc->h_stage.resize(S * LCC_STAGE);
  lc->h_fix_out.resize(LcFixOut::bytes(S * LCC_NBEST, S));
  lc->sets_cap = n_streams;
  *out = lc;
  return FLVIS_OK;
}

// one config for every sequence: the same call on n_streams copies
int flvis_loop_closer_create(flvis_ctx* ctx, const flvis_cfg* cfg, const flvis_lc_params* prm, int n_streams, int max_keyframes,
                             const int8_t* h_orb_pattern, flvis_loop_closer** out) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!cfg || n_streams <= 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_create: bad args");
  const std::vector<flvis_cfg> cfgs((size_t)n_streams, *cfg);
  return flvis_loop_closer_create_rigs(ctx, cfgs.data(), prm, n_streams, max_keyframes, h_orb_pattern, out);
}

// Start over on the named sequences, each on cfgs[i] when cfgs is given.  Host bookkeeping plus, for a new camera, one row copy in
// stream order from the closer's pinned table: nothing waits for the device.
static int lc_reset(flvis_loop_closer* lc, int n, const int* streams, const flvis_cfg* cfgs, const char* what) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  if (n < 0 || (n > 0 && !streams)) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": bad args");
  std::vector<char> named((size_t)lc->S, 0);
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    if (s < 0 || s >= lc->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": stream out of range");
    if (named[s]) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": stream " + std::to_string(s) + " is listed twice");
    named[s] = 1;
    if (cfgs)
      if (const char* f = lc_batch_field_mismatch(lc, cfgs[i]))
        return ctx->fail(FLVIS_ERR_CONFIG, std::string(what) + ": stream " + std::to_string(s) + ": batch-wide field " + f +
                                               " differs from the closer's (stream 0)");
  }
  if (n == 0) return FLVIS_OK;
  hipSetDevice(ctx->device);
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    lc->seq[s] = Seq();  // n, the pending keyframe, T_odom_map, the loop list and last_pgo (the slot's database entries: unreachable with n = 0)
    std::fill(lc->h_rows.begin() + (size_t)s * lc->maxkf, lc->h_rows.begin() + (size_t)(s + 1) * lc->maxkf, 0.0);
    if (!cfgs) continue;
    lc->cfgs[s] = cfgs[i];
    // (a copy of this row that a previous reset queued has run: every call that reads the table returns synchronised, and with no such
    //  call in between nothing has looked at the row the earlier reset wrote)
    lc_cam_of_cfg(cfgs[i], &lc->h_cams[s]);
    hipError_t e = hipMemcpyAsync(lc->d_cams + s, lc->h_cams + s, sizeof(LcCam), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && lc->h_ucams) {
      lc_cam_unrect_of_cfg(cfgs[i], &lc->h_ucams[s]);
      e = hipMemcpyAsync(lc->d_ucams + s, lc->h_ucams + s, sizeof(LcCamUnrect), hipMemcpyHostToDevice, ctx->stream);
    }
    if (e != hipSuccess) return ctx->hip_fail(e, what);
  }
  return FLVIS_OK;
}

int flvis_loop_closer_reset(flvis_loop_closer* lc, int n, const int* streams) { return lc_reset(lc, n, streams, nullptr, "loop_closer_reset"); }

int flvis_loop_closer_reset_rigs(flvis_loop_closer* lc, int n, const int* streams, const flvis_cfg* cfgs) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  if (n > 0 && !cfgs) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_reset_rigs: bad args");
  return lc_reset(lc, n, streams, cfgs, "loop_closer_reset_rigs");
}

int flvis_loop_closer_stream_cfg(flvis_loop_closer* lc, int stream, flvis_cfg* out) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  if (stream < 0 || stream >= lc->S || !out) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_stream_cfg: bad args");
  *out = lc->cfgs[stream];
  return FLVIS_OK;
}

void flvis_loop_closer_destroy(flvis_loop_closer* lc) {
  if (!lc) return;
  hipSetDevice(lc->device);  // (the context may already be gone: nothing of it is touched here)
  hipDeviceSynchronize();
  for (void* p : lc->owned) hipFree(p);
  hipHostFree(lc->h_cams);
  if (lc->h_ucams) hipHostFree(lc->h_ucams);
  delete lc;
}

// The reference's STEREO_UNRECT case is empty: a keyframe of such a rig stores no landmark (the default here).  enable != 0 fills it with
// this project's rule (k_lc_landmarks_unrect) for every frame that goes through a keyframe's steps from now on.  The switch belongs to the
// whole database -- a map of keyframes with and without landmarks, in raw and in rectified pixels, would be neither -- so it is refused
// while any sequence holds a keyframe.
int flvis_loop_closer_set_stereo_unrect(flvis_loop_closer* lc, int enable) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  if (lc->cam_type != 1) return ctx->fail(FLVIS_ERR_CONFIG, "loop_closer_set_stereo_unrect: the closer's rig is not STEREO_UNRECT (cam_type 1)");
  for (int s = 0; s < lc->S; s++)
    if (lc->seq[s].n > 0)
      return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_set_stereo_unrect: sequence " + std::to_string(s) +
                                                  " holds keyframes (reset every sequence first)");
  lc->stereo_unrect = enable != 0;
  return FLVIS_OK;
}

// STEP 1.3 / 1.4 / 1.5 / 1.6 (:236-372) for n images into the per-call buffers: ORB, bag of words of ALL descriptors, 3-D positions with
// the camera of each image's sequence (d_seq), then the lists without the rest -- a keyframe's, and a localize call's query's
static int lc_features(flvis_loop_closer* lc, int n, const uint8_t* d_img0, const void* d_img1, const int* d_seq) {
  flvis_ctx* ctx = lc->ctx;
  int rc = flvis_hip_orb_detect_and_compute(ctx, d_img0, lc->w, lc->h, n, &lc->orb, lc->pattern.empty() ? nullptr : lc->pattern.data(), lc->kps,
                                            lc->desc, lc->cnt, LCC_CAP, lc->ovf);
  if (rc == FLVIS_OK) rc = flvis_hip_bow_transform(ctx, lc->desc, lc->cnt, LCC_CAP, n, LCC_VCAP, lc->ids, lc->vals, lc->nnz);
  if (rc == FLVIS_OK && lc->stereo_unrect)
    rc = flvis::lc_keyframe_landmarks_unrect_dev(ctx, d_img0, (const uint8_t*)d_img1, lc->w, lc->h, n, lc->d_cams, lc->d_ucams, d_seq, lc->kps,
                                                 lc->desc, lc->cnt, LCC_CAP, lc->lm2, lc->lm3, lc->desc, lc->lmc);
  else if (rc == FLVIS_OK)
    rc = flvis::lc_keyframe_landmarks_dev(ctx, d_img0, d_img1, lc->w, lc->h, n, lc->cam_type, lc->d_cams, d_seq, lc->kps, lc->desc, lc->cnt,
                                          LCC_CAP, lc->lm2, lc->lm3, lc->desc, lc->lmc);
  return rc;
}

int flvis_loop_closer_add_keyframes(flvis_loop_closer* lc, int n, const int* h_stream, const uint8_t* d_img0, const void* d_img1,
                                    const double* h_T_c_w_odom7, int64_t* h_kf_id) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  if (n <= 0 || n > lc->S || !h_stream || !d_img0 || !h_T_c_w_odom7) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_add_keyframes: bad args");
  std::vector<char> used((size_t)lc->S, 0);
  for (int i = 0; i < n; i++) {
    const int s = h_stream[i];
    if (s < 0 || s >= lc->S || used[s]) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_add_keyframes: one keyframe per sequence and call");
    used[s] = 1;
    if (lc->seq[s].n >= lc->maxkf) return ctx->fail(FLVIS_ERR_CAPACITY, "loop_closer_add_keyframes: a sequence's keyframe capacity is used up");
  }
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  // STEP 2's host part first (:374-383, T_c_w = T_c_w_odom * T_odom_map): the poses, the keyframes' slots and their sequences -- the
  // index of each keyframe's camera -- go to the device in ONE copy, ahead of the kernels that read them
  double* const T = reinterpret_cast<double*>(lc->h_stage.data());
  int* const slot = reinterpret_cast<int*>(lc->h_stage.data() + 7 * sizeof(double) * (size_t)n);
  for (int i = 0; i < n; i++) {
    const Seq& q = lc->seq[h_stream[i]];
    slot[i] = h_stream[i] * lc->maxkf + q.n;
    slot[n + i] = h_stream[i];
    pose_mul(h_T_c_w_odom7 + 7 * i, q.T_odom_map, T + 7 * (size_t)i);
  }
  const double* const d_T = reinterpret_cast<const double*>(lc->stage);
  const int* const d_slot = reinterpret_cast<const int*>(lc->stage + 7 * sizeof(double) * (size_t)n);
  hipError_t e = hipMemcpyAsync(lc->stage, lc->h_stage.data(), LCC_STAGE * (size_t)n, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_add_keyframes");
  int rc = lc_features(lc, n, d_img0, d_img1, d_slot + n);
  if (rc != FLVIS_OK) {
    hipStreamSynchronize(st);  // (h_stage is reused by the next call)
    return rc;
  }
  // STEP 2 on the device: the keyframe joins its sequence's map
  k_lcc_store<<<dim3(LCC_CAP / 256, n), 256, 0, st>>>(d_slot, lc->ids, lc->vals, lc->nnz, lc->lm2, lc->lm3, lc->desc, lc->lmc, d_T, lc->db_ids,
                                                       lc->db_vals, lc->db_nnz, lc->db_lm2, lc->db_lm3, lc->db_lmd, lc->db_lmc, lc->db_T);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the batch is stored when the call returns (and h_stage is free again)
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_add_keyframes");
  for (int i = 0; i < n; i++) {
    Seq& q = lc->seq[h_stream[i]];
    q.T_odom.insert(q.T_odom.end(), h_T_c_w_odom7 + 7 * i, h_T_c_w_odom7 + 7 * i + 7);
    q.stamp.push_back(NAN);
    if (h_kf_id) h_kf_id[i] = q.n;
    q.n++;
    q.fresh = true;
  }
  return FLVIS_OK;
}

// KeyFrameMsg::unpack (:206) hands the nodelet HOST images; this is the same call on host buffers: mono8 img0, mono8 or 16UC1 img1
// the host images of an add_keyframes_host / localize_host call: first checked (nothing is queued), ...
static int lc_host_images_check(flvis_loop_closer* lc, int n, const int* h_stream, const flvis_image* h_img0, const flvis_image* h_img1,
                                const std::string& what) {
  flvis_ctx* ctx = lc->ctx;
  const int bpp1 = lc->cam_type == 2 ? 2 : 1;
  for (int i = 0; i < n; i++) {
    const flvis_image &a = h_img0[i], &b = h_img1[i];
    if (h_stream[i] < 0 || h_stream[i] >= lc->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, what + ": bad stream index");
    if (!a.data || !b.data || a.width != lc->w || a.height != lc->h || b.width != lc->w || b.height != lc->h || a.channels != 1 || b.channels != 1 ||
        a.pitch < lc->w || b.pitch < lc->w * bpp1)
      return ctx->fail(FLVIS_ERR_INVALID_ARG, what + ": images must be mono8 (img1: 16UC1 on a depth rig) of the configured size");
  }
  return FLVIS_OK;
}
// ... and queued for upload into the context's staging images (the caller waits for the stream before its images may go away)
static int lc_host_images_stage(flvis_loop_closer* lc, int n, const flvis_image* h_img0, const flvis_image* h_img1, const std::string& what,
                                uint8_t** d_img0, uint8_t** d_img1) {
  flvis_ctx* ctx = lc->ctx;
  const int bpp1 = lc->cam_type == 2 ? 2 : 1;
  const size_t px = (size_t)lc->w * lc->h;
  hipSetDevice(ctx->device);
  uint8_t* d0 = (uint8_t*)ctx->scratch("lc_host_img0", px * (size_t)lc->S);
  uint8_t* d1 = (uint8_t*)ctx->scratch("lc_host_img1", px * 2 * (size_t)lc->S);
  if (!d0 || !d1) return ctx->fail(FLVIS_ERR_HIP, what + ": staging allocation failed");
  hipError_t e = hipSuccess;
  for (int i = 0; i < n && e == hipSuccess; i++) {
    const flvis_image &a = h_img0[i], &b = h_img1[i];
    e = hipMemcpy2DAsync(d0 + px * i, (size_t)lc->w, a.data, (size_t)a.pitch, (size_t)lc->w, (size_t)lc->h, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(d1 + px * bpp1 * i, (size_t)lc->w * bpp1, b.data, (size_t)b.pitch, (size_t)lc->w * bpp1, (size_t)lc->h,
                           hipMemcpyHostToDevice, ctx->stream);
  }
  if (e != hipSuccess) {
    hipStreamSynchronize(ctx->stream);  // copies from the caller's images may still be in flight
    return ctx->hip_fail(e, what.c_str());
  }
  *d_img0 = d0, *d_img1 = d1;
  return FLVIS_OK;
}
// ... around the device-image call of the same name: call(d_img0, d_img1) synchronises when it succeeds, and on its error paths the uploads
// are waited for here.  Every argument is checked BEFORE a copy is queued (the caller has checked its own): the caller may free its images
// as soon as the call returns with an error.
static int lc_on_host_images(flvis_loop_closer* lc, int n, const int* h_stream, const flvis_image* h_img0, const flvis_image* h_img1,
                             const std::string& what, const std::function<int(const uint8_t*, const uint8_t*)>& call) {
  int rc = lc_host_images_check(lc, n, h_stream, h_img0, h_img1, what);
  uint8_t *d0 = nullptr, *d1 = nullptr;
  if (rc == FLVIS_OK) rc = lc_host_images_stage(lc, n, h_img0, h_img1, what, &d0, &d1);
  if (rc != FLVIS_OK) return rc;
  rc = call(d0, d1);
  if (rc != FLVIS_OK) hipStreamSynchronize(lc->ctx->stream);
  return rc;
}

int flvis_loop_closer_add_keyframes_host(flvis_loop_closer* lc, int n, const int* h_stream, const flvis_image* h_img0, const flvis_image* h_img1,
                                         const double* h_T_c_w_odom7, int64_t* h_kf_id) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* const what = "loop_closer_add_keyframes_host";
  if (n <= 0 || n > lc->S || !h_img0 || !h_img1 || !h_stream || !h_T_c_w_odom7)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_add_keyframes_host: bad args");
  return lc_on_host_images(lc, n, h_stream, h_img0, h_img1, what, [&](const uint8_t* d0, const uint8_t* d1) {
    return flvis_loop_closer_add_keyframes(lc, n, h_stream, d0, d1, h_T_c_w_odom7, h_kf_id);
  });
}

// isLoopClosureKF (:593-686) on the device for nc pairs of database slots (a: the keyframe whose 3-D points are used, b: the one whose
// pixels are; cam_of: the pair's camera row): mutual / ratio matches, the correspondences, solvePnPRansac in its P3P form (100 iterations,
// 2.0 px, 0.99).  Leaves the matches, the pose and the inliers per pair in d_npairs / d_pose / d_ninl; a pair with a side that has no
// landmarks runs through as an empty set (0 matches, the identity, 0 inliers).  nc <= lc->sets_cap.
static int lc_pair_check(flvis_loop_closer* lc, int nc, const int* slot_a, const int* slot_b, const int* cam_of, const uint64_t* h_seeds,
                         int* d_npairs, double* d_pose, int* d_ninl) {
  flvis_ctx* ctx = lc->ctx;
  hipStream_t st = ctx->stream;
  k_lcc_fetch<<<dim3(LCC_CAP / 256, nc), 256, 0, st>>>(slot_a, slot_b, lc->db_lmd, lc->db_lmc, lc->da, lc->na, lc->db, lc->nb);
  int rc = flvis_hip_orb_match(ctx, lc->da, lc->na, LCC_CAP, lc->db, lc->nb, LCC_CAP, nc, lc->prm.ratioMax, lc->pairs, d_npairs);
  if (rc != FLVIS_OK) return rc;
  k_lcc_correspondences<<<dim3(LCC_CAP / 256, nc), 256, 0, st>>>(slot_a, slot_b, lc->pairs, d_npairs, lc->db_lm3, lc->db_lm2, lc->p3d, lc->p2d);
  return flvis::pnp_ransac_dev(ctx, lc->p3d, lc->p2d, d_npairs, LCC_CAP, nc, nullptr, &lc->d_cams[0].fx, flvis::LC_CAM_DOUBLES, cam_of, 100, 2.0,
                               0.99, h_seeds, d_pose, lc->mask, d_ninl);
}

// ... and its verdict on the host (:666-686) from the matches m, the inliers and the PnP pose T: process' rule, and localize's
static bool lc_pair_accepted(const flvis_lc_params& p, int m, int inl, const double* T) {
  if (m < 5) return false;                                            // "p3d not enough" (:666)
  if (inl * 1.0 / m < p.ratioRansac || inl < p.minPts) return false;  // :677
  const double tn = std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
  const double vn = std::sqrt(T[3] * T[3] + T[4] * T[4] + T[5] * T[5]);
  const double angle = 2.0 * std::atan2(vn, std::fabs(T[6]));  // |so3().log()|
  return tn < 3 && angle < 1.5;                                // :686
}

int flvis_loop_closer_process(flvis_loop_closer* lc, flvis_lc_event* h_events) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  if (!h_events) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_process: no event array");
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const flvis_lc_params& p = lc->prm;
  for (int s = 0; s < lc->S; s++) {
    flvis_lc_event& ev = h_events[s];
    memset(&ev, 0, sizeof(ev));
    ev.kf_prev = -1;
    ev.kf_curr = lc->seq[s].fresh ? lc->seq[s].n - 1 : -1;
    ev.loop_pose7[6] = 1.0;
  }
  // STEP 3 (:417-437): the newest keyframe of every sequence that got one against all keyframes of that sequence -- one launch for all
  // sequences, one strided copy of the rows
  std::vector<int> jobs;
  int max_n = 0;
  for (int s = 0; s < lc->S; s++) {
    const Seq& q = lc->seq[s];
    if (!q.fresh) continue;
    const int base = s * lc->maxkf;
    jobs.push_back(base + q.n - 1);
    jobs.push_back(base);
    jobs.push_back(q.n);
    max_n = std::max(max_n, q.n);
  }
  if (jobs.empty()) return FLVIS_OK;
  int rc0 = flvis_hip_bow_score_jobs(ctx, (int)(jobs.size() / 3), jobs.data(), lc->db_ids, lc->db_vals, lc->db_nnz, LCC_VCAP, lc->rows);
  if (rc0 != FLVIS_OK) return rc0;
  hipError_t e = hipMemcpy2DAsync(lc->h_rows.data(), sizeof(double) * (size_t)lc->maxkf, lc->rows, sizeof(double) * (size_t)lc->maxkf,
                                  sizeof(double) * (size_t)max_n, (size_t)lc->S, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_process");
  // :453 + isLoopCandidate (:520-590) on the host
  std::vector<int> cand;  // sequences with a candidate
  std::vector<int> sa, sb;  // the pair's database slots
  for (int s = 0; s < lc->S; s++) {
    Seq& q = lc->seq[s];
    if (!q.fresh) continue;
    q.fresh = false;
    if (q.n < 50) continue;
    const std::vector<uint8_t> present((size_t)q.n, 1);
    int64_t prev = -1;
    const int r = flvis_loop_candidate(q.n, &lc->h_rows[(size_t)s * lc->maxkf], present.data(), p.lcKFDist, p.lcKFMaxDist, p.lcNKFClosest, p.minScore,
                                       &prev);
    if (r != 1) continue;
    h_events[s].candidate = 1;
    h_events[s].kf_prev = prev;
    cand.push_back(s);
    sa.push_back(s * lc->maxkf + (int)prev);
    sb.push_back(s * lc->maxkf + q.n - 1);
  }
  const int nc = (int)cand.size();
  if (nc == 0) return FLVIS_OK;
  // isLoopClosureKF (:593-686) for all candidates at once
  // one copy: the earlier keyframes' slots, the later ones', the candidates' sequences (= their cameras' rows)
  sa.insert(sa.end(), sb.begin(), sb.end());
  sa.insert(sa.end(), cand.begin(), cand.end());
  const int *const slot_a = lc->slot_a, *const slot_b = lc->slot_a + nc, *const cam_of = lc->slot_a + 2 * nc;
  e = hipMemcpyAsync(lc->slot_a, sa.data(), sizeof(int) * 3 * (size_t)nc, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_process");
  std::vector<uint64_t> seeds((size_t)nc);
  for (int i = 0; i < nc; i++) seeds[i] = ((uint64_t)(cand[i] + 1) << 32) + (uint64_t)lc->seq[cand[i]].n;  // (stream + 1) << 32 | kf_curr + 1
  int rc = lc_pair_check(lc, nc, slot_a, slot_b, cam_of, seeds.data(), lc->npairs, lc->pose, lc->ninl);
  if (rc != FLVIS_OK) return rc;
  std::vector<int> h_np((size_t)nc), h_ni((size_t)nc);
  std::vector<double> h_pose((size_t)nc * 7);
  e = hipMemcpyAsync(h_np.data(), lc->npairs, sizeof(int) * (size_t)nc, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_ni.data(), lc->ninl, sizeof(int) * (size_t)nc, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_pose.data(), lc->pose, sizeof(double) * 7 * (size_t)nc, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_process");
  std::vector<int> pgo;  // sequences whose pose graph is due (:492-497)
  for (int i = 0; i < nc; i++) {
    const int s = cand[i];
    Seq& q = lc->seq[s];
    flvis_lc_event& ev = h_events[s];
    const int m = h_np[i], inl = h_ni[i];
    const double* T = &h_pose[7 * (size_t)i];
    ev.n_matches = m;
    if (m < 5) continue;  // "p3d not enough" (:666)
    ev.n_inliers = inl;
    memcpy(ev.loop_pose7, T, 7 * sizeof(double));
    if (!lc_pair_accepted(p, m, inl, T)) continue;
    ev.loop_accepted = 1;
    q.loop_ids.push_back((int)ev.kf_prev);
    q.loop_ids.push_back(q.n - 1);
    q.loop_poses.insert(q.loop_poses.end(), T, T + 7);
    const int thre = (int)(((double)q.n / 100) * 2);  // :490
    if ((long long)(q.n - 1) - q.last_pgo > thre) {
      pgo.push_back(s);
      q.last_pgo = q.n - 1;
    }
  }
  // loopClosureOnCovGraphG2ONew (:742-944) for every sequence that asked for it, ONE launch (one workgroup per pose graph): the
  // sequences' pose arrays are gathered into one contiguous batch, optimised, and copied back
  const int ng = (int)pgo.size();
  if (ng == 0) return FLVIS_OK;
  std::vector<int> n_kf((size_t)ng), n_loops((size_t)ng), ids, ran((size_t)ng, 0);
  std::vector<uint8_t> present;
  std::vector<double> lp;
  size_t off = 0;
  e = hipSuccess;
  for (int g = 0; g < ng; g++) {
    const Seq& q = lc->seq[pgo[g]];
    n_kf[g] = q.n;
    n_loops[g] = (int)(q.loop_ids.size() / 2);
    ids.insert(ids.end(), q.loop_ids.begin(), q.loop_ids.end());
    lp.insert(lp.end(), q.loop_poses.begin(), q.loop_poses.end());
    present.insert(present.end(), (size_t)q.n, 1);
    if (e == hipSuccess)
      e = hipMemcpyAsync(lc->pgo_T + off * 7, lc->db_T + (size_t)pgo[g] * lc->maxkf * 7, sizeof(double) * 7 * (size_t)q.n, hipMemcpyDeviceToDevice, st);
    off += (size_t)q.n;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(lc->loop_pose, lp.data(), sizeof(double) * lp.size(), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_process");
  rc = flvis_hip_pgo_loop_closure(ctx, ng, n_kf.data(), lc->pgo_T, present.data(), n_loops.data(), ids.data(), lc->loop_pose, 100, 1, lc->drift,
                                  lc->stats, ran.data());
  if (rc != FLVIS_OK) return rc;
  std::vector<double> drift((size_t)ng * 7), stats((size_t)ng * 5);
  off = 0;
  for (int g = 0; g < ng && e == hipSuccess; g++) {
    if (ran[g])
      e = hipMemcpyAsync(lc->db_T + (size_t)pgo[g] * lc->maxkf * 7, lc->pgo_T + off * 7, sizeof(double) * 7 * (size_t)n_kf[g], hipMemcpyDeviceToDevice, st);
    off += (size_t)n_kf[g];
  }
  if (e == hipSuccess) e = hipMemcpyAsync(drift.data(), lc->drift, sizeof(double) * drift.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(stats.data(), lc->stats, sizeof(double) * stats.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_process");
  for (int g = 0; g < ng; g++) {
    if (!ran[g]) continue;
    Seq& q = lc->seq[pgo[g]];
    flvis_lc_event& ev = h_events[pgo[g]];
    double m2[7];
    pose_mul(q.T_odom_map, &drift[7 * (size_t)g], m2);  // T_odom_map = T_odom_map * Tw1_w2 (:908)
    memcpy(q.T_odom_map, m2, sizeof(m2));
    ev.optimised = 1;
    ev.pgo_iterations = (int)stats[5 * (size_t)g];
    ev.chi2_before = stats[5 * (size_t)g + 1];
    ev.chi2_after = stats[5 * (size_t)g + 2];
    // (:922-925 re-derives the keyframes BEHIND the last optimised one from their odometry pose; the newest keyframe is the last
    //  optimised one here, so there is none)
  }
  return FLVIS_OK;
}

// the arguments of a localize call that both forms share, checked before anything is queued
static int lc_localize_check(flvis_loop_closer* lc, int n, const int* h_stream, int n_best, const flvis_lc_fix* h_fix, const std::string& what) {
  flvis_ctx* ctx = lc->ctx;
  if (n <= 0 || n > lc->S || !h_stream || !h_fix) return ctx->fail(FLVIS_ERR_INVALID_ARG, what + ": bad args");
  if (n_best < 1 || n_best > LCC_NBEST) return ctx->fail(FLVIS_ERR_INVALID_ARG, what + ": n_best must be 1 .. " + std::to_string(LCC_NBEST));
  std::vector<char> used((size_t)lc->S, 0);
  for (int i = 0; i < n; i++) {
    const int s = h_stream[i];
    if (s < 0 || s >= lc->S || used[s]) return ctx->fail(FLVIS_ERR_INVALID_ARG, what + ": one query per sequence and call");
    used[s] = 1;
  }
  return FLVIS_OK;
}

// the buffers of a candidate search beyond what create allocates, grown by the first call that needs them: the pair-check buffers for
// LCC_NBEST sets per sequence, the score rows and the selection buffers -- all_maps: rows for all segments
static int lc_search_reserve(flvis_loop_closer* lc, bool all_maps, const char* what) {
  flvis_ctx* ctx = lc->ctx;
  hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  const int ns_cap = lc->S * LCC_NBEST;
  if (lc->sets_cap < ns_cap) {  // the first search: the pair-check buffers grow from one set per sequence to LCC_NBEST
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, what);
    const size_t c = (size_t)ns_cap;
    if (!(lc->regrow(lc->slot_a, c * 3) && lc->regrow(lc->da, c * LCC_CAP * 32) && lc->regrow(lc->db, c * LCC_CAP * 32) && lc->regrow(lc->na, c) &&
          lc->regrow(lc->nb, c) && lc->regrow(lc->pairs, c * LCC_CAP * 2) && lc->regrow(lc->p3d, c * LCC_CAP * 3) &&
          lc->regrow(lc->p2d, c * LCC_CAP * 2) && lc->regrow(lc->mask, c * LCC_CAP))) {
      (void)hipGetLastError();
      // (a buffer that did not grow keeps its size, and sets_cap its value: process goes on, the next search tries again)
      return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
    }
    lc->sets_cap = ns_cap;
  }
  const size_t S = (size_t)lc->S, need = (all_maps ? S * S : S) * (size_t)lc->maxkf;
  if (need > (size_t)INT_MAX - 64) return ctx->fail(FLVIS_ERR_CAPACITY, std::string(what) + ": n_streams^2 * max_keyframes is too large");
  if (lc->mrows_cap < need || !lc->sel_cnt) {  // the first search, and the first that searches all maps
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, what);
    bool ok = lc->mrows ? lc->regrow(lc->mrows, need) : lc->alloc(lc->mrows, need);
    if (ok) lc->mrows_cap = need;
    ok = ok && (lc->in_stage || lc->alloc(lc->in_stage, 2 * S)) && (lc->sel_idx || lc->alloc(lc->sel_idx, S * LCC_NBEST)) &&
         (lc->sel_score || lc->alloc(lc->sel_score, S * LCC_NBEST)) && (lc->sel_cnt || lc->alloc(lc->sel_cnt, S));
    if (!ok) {
      (void)hipGetLastError();
      // (the rows keep the size they had: calls that need no more go on, the next one that does tries again)
      return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation of the score rows failed");
    }
    lc->h_in_stage.resize(2 * S);
  }
  return FLVIS_OK;
}

// the host's part of a fix: query i of a call with n_best ranks per query from the result block h (cand_kf: what h.kf holds)
static void lc_fix_fill(const flvis_loop_closer* lc, const LcFixOut& h, int i, int n_best, flvis_lc_fix& f) {
  memset(&f, 0, sizeof(f));
  f.n_landmarks = h.nlm[i];
  f.n_candidates = h.ncand[i];
  f.best = -1;
  f.T_c_map7[6] = 1.0;
  for (int r = 0; r < LCC_NBEST; r++) f.cand_kf[r] = -1, f.cand_pose7[r][6] = 1.0;
  for (int r = 0; r < f.n_candidates; r++) {
    const int set = i * n_best + r, m = h.npairs[set];
    f.cand_kf[r] = h.kf[set];
    f.cand_score[r] = h.score[set];
    f.cand_matches[r] = m;
    if (m < 5) continue;  // "p3d not enough" (:666): no inliers, the identity, as in an event
    const double* const P = h.pose + 7 * (size_t)set;
    f.cand_inliers[r] = h.ninl[set];
    memcpy(f.cand_pose7[r], P, 7 * sizeof(double));
    f.cand_accepted[r] = lc_pair_accepted(lc->prm, m, h.ninl[set], P) ? 1 : 0;
    if (f.cand_accepted[r] && (f.best < 0 || f.cand_inliers[r] > f.cand_inliers[f.best])) f.best = r;
  }
  if (f.best >= 0) pose_mul(f.cand_pose7[f.best], h.T_kf + 7 * (size_t)(i * n_best + f.best), f.T_c_map7);
}

// ... and of a localize_in fix: the candidates come back as database slots and are split into (sequence, keyframe)
static void lc_fix_in_split(const flvis_loop_closer* lc, flvis_lc_fix_in& f) {
  for (int r = 0; r < LCC_NBEST; r++) {
    const int64_t g = f.fix.cand_kf[r];
    f.cand_seq[r] = g < 0 ? -1 : (int)(g / lc->maxkf);
    if (g >= 0) f.fix.cand_kf[r] = g % lc->maxkf;
  }
  f.map = f.fix.best >= 0 ? f.cand_seq[f.fix.best] : -1;
  f.reserved = 0;
}

// The queries of a candidate search, per query: the database slot that stands for it (its sequence's query slot, or a stored keyframe's
// own slot), its sequence (= its camera's row), the searched map (< 0: every map) and, skip != null, the slots [skip[2i], skip[2i + 1]) that
// are no candidates of it.  slot, seq and skip are host arrays and the same on the device, in the one upload the caller has queued.
struct LcQueries {
  const int *slot, *seq, *skip, *map;  // host
  const int *d_slot, *d_seq, *d_skip;  // device
};

// The candidate search of localize, localize_in and link for n <= n_streams queries: every query is scored against the keyframes of its
// searched maps -- one launch for all (query, map that holds candidates) jobs, a row per query of one segment per sequence (all_maps) or of
// the one segment it searches --, k_lc_select_maps picks the n_best best across the maps, and each (keyframe, query) pair goes through
// isLoopClosureKF's check as process runs it: n * n_best sets, empty where there is no candidate.  One copy brings the results back; fix i
// is written at fix_base + i * fix_stride, a flvis_lc_fix_in (fix_in: the candidates split into sequence and keyframe) or a flvis_lc_fix
// (the keyframe alone).  by_slot: the queries are stored keyframes (their landmark counts are the database's, not the call's feature
// buffers').  Nothing of the sequences' state is written: not Seq, not the database's keyframe slots, not `rows`.  The one exit waits for
// the stream when the search fails: h_stage, which the caller filled, is reused by the next call.
static int lc_search(flvis_loop_closer* lc, int n, const LcQueries& q, bool all_maps, bool by_slot, int n_best, char* fix_base, size_t fix_stride,
                     bool fix_in, const char* what) {
  flvis_ctx* ctx = lc->ctx;
  hipStream_t st = ctx->stream;
  const int S = lc->S, maxkf = lc->maxkf, ns = n * n_best, ns_cap = S * LCC_NBEST;
  auto hip = [&](hipError_t e) { return e == hipSuccess ? (int)FLVIS_OK : ctx->hip_fail(e, what); };
  // the searched maps and the sequences' keyframe counts (one upload); one job per (query, searched map that holds candidates)
  const size_t stride = (size_t)(all_maps ? S : 1) * maxkf;
  int* const hm = lc->h_in_stage.data();
  std::vector<int> jobs;
  for (int m = 0; m < S; m++) hm[n + m] = lc->seq[m].n;
  for (int i = 0; i < n; i++) {
    hm[i] = q.map[i] < 0 ? -1 : q.map[i];
    for (int m = hm[i] < 0 ? 0 : hm[i]; m < (hm[i] < 0 ? S : hm[i] + 1); m++) {
      const int first = m * maxkf, nk = lc->seq[m].n;
      // (a map wholly excluded: its part of the row is never written, and never read)
      if (nk > 0 && !(q.skip && q.skip[2 * i] <= first && first + nk <= q.skip[2 * i + 1]))
        jobs.insert(jobs.end(), {q.slot[i], first, nk, (int)(stride * i + (all_maps ? (size_t)first : 0))});
    }
  }
  int rc = hip(hipMemcpyAsync(lc->in_stage, hm, sizeof(int) * (size_t)(n + S), hipMemcpyHostToDevice, st));
  const int n_jobs = (int)(jobs.size() / 4);
  for (int j0 = 0; j0 < n_jobs && rc == FLVIS_OK; j0 += 65535)  // (a launch takes 65535 jobs: one launch up to 255 sequences)
    rc = flvis_hip_bow_score_jobs_at(ctx, std::min(65535, n_jobs - j0), jobs.data() + 4 * (size_t)j0, lc->db_ids, lc->db_vals, lc->db_nnz, LCC_VCAP,
                                     lc->mrows);
  if (rc == FLVIS_OK)
    rc = flvis::lc_select_maps_dev(ctx, n, lc->mrows, S, maxkf, lc->in_stage + n, lc->in_stage, q.d_skip, !all_maps, n_best, lc->prm.minScore,
                                   lc->sel_idx, lc->sel_score, lc->sel_cnt);
  int *const slot_a = lc->slot_a, *const slot_b = lc->slot_a + ns, *const cam_of = lc->slot_a + 2 * ns;
  const LcFixOut out = LcFixOut::at(lc->fix_out, (size_t)ns_cap, (size_t)S);
  if (rc == FLVIS_OK) {
    if (by_slot)
      k_lcc_select_sets<true><<<n, 64, 0, st>>>(q.d_slot, q.d_seq, lc->sel_idx, lc->sel_score, lc->sel_cnt, n_best, lc->empty_slot(), lc->db_lmc,
                                                lc->db_T, slot_a, slot_b, cam_of, out);
    else
      k_lcc_select_sets<false><<<n, 64, 0, st>>>(q.d_slot, q.d_seq, lc->sel_idx, lc->sel_score, lc->sel_cnt, n_best, lc->empty_slot(), lc->lmc,
                                                 lc->db_T, slot_a, slot_b, cam_of, out);
    std::vector<uint64_t> seeds((size_t)ns);
    for (int i = 0; i < ns; i++) seeds[i] = ((uint64_t)(q.seq[i / n_best] + 1) << 32) + (uint64_t)(i % n_best + 1);  // (stream + 1) << 32 | rank + 1
    rc = lc_pair_check(lc, ns, slot_a, slot_b, cam_of, seeds.data(), out.npairs, out.pose, out.ninl);
  }
  if (rc == FLVIS_OK) rc = hip(hipMemcpyAsync(lc->h_fix_out.data(), lc->fix_out, lc->h_fix_out.size(), hipMemcpyDeviceToHost, st));
  if (rc == FLVIS_OK) rc = hip(hipStreamSynchronize(st));
  if (rc != FLVIS_OK) {
    hipStreamSynchronize(st);
    return rc;
  }
  const LcFixOut h = LcFixOut::at(lc->h_fix_out.data(), (size_t)ns_cap, (size_t)S);
  for (int i = 0; i < n; i++) {
    flvis_lc_fix& f = *reinterpret_cast<flvis_lc_fix*>(fix_base + fix_stride * (size_t)i);
    lc_fix_fill(lc, h, i, n_best, f);  // (cand_kf: database slots)
    if (fix_in) lc_fix_in_split(lc, *reinterpret_cast<flvis_lc_fix_in*>(&f));
    else
      for (int r = 0; r < f.n_candidates; r++) f.cand_kf[r] %= maxkf;
  }
  return FLVIS_OK;
}

// Relocalisation: where is this frame's camera in the map of sequence h_map[i], or in whichever map knows the place (< 0)?  h_map ==
// nullptr is localize: every query in the map its own sequence has built.  What is this run's own comes before the search: the queries go
// through a keyframe's steps into their sequences' query slots, so that the kernels which take database slots address them as they address
// a keyframe.  The fix of query i is written at fix_base + i * fix_stride (lc_search).
static int lc_localize_run(flvis_loop_closer* lc, int n, const int* h_stream, const int* h_map, const uint8_t* d_img0, const void* d_img1,
                           int n_best, char* fix_base, size_t fix_stride, const char* what) {
  flvis_ctx* ctx = lc->ctx;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  bool all_maps = false;
  for (int i = 0; h_map && i < n; i++) all_maps = all_maps || h_map[i] < 0;
  int rc = lc_search_reserve(lc, all_maps, what);
  if (rc != FLVIS_OK) return rc;
  // one upload: identity poses for k_lcc_store, the queries' slots, their sequences (= camera rows)
  double* const T = reinterpret_cast<double*>(lc->h_stage.data());
  int* const hq = reinterpret_cast<int*>(lc->h_stage.data() + 7 * sizeof(double) * (size_t)n);
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 7; k++) T[7 * (size_t)i + k] = k == 6 ? 1.0 : 0.0;
    hq[i] = lc->query_slot(h_stream[i]), hq[n + i] = h_stream[i];
  }
  const double* const d_T = reinterpret_cast<const double*>(lc->stage);
  const int* const d_q = reinterpret_cast<const int*>(lc->stage + 7 * sizeof(double) * (size_t)n);
  hipError_t e = hipMemcpyAsync(lc->stage, lc->h_stage.data(), LCC_STAGE * (size_t)n, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  rc = lc_features(lc, n, d_img0, d_img1, d_q + n);
  if (rc == FLVIS_OK) {
    k_lcc_store<<<dim3(LCC_CAP / 256, n), 256, 0, st>>>(d_q, lc->ids, lc->vals, lc->nnz, lc->lm2, lc->lm3, lc->desc, lc->lmc, d_T, lc->db_ids,
                                                         lc->db_vals, lc->db_nnz, lc->db_lm2, lc->db_lm3, lc->db_lmd, lc->db_lmc, lc->db_T);
    e = hipGetLastError();
    if (e != hipSuccess) rc = ctx->hip_fail(e, what);
  }
  if (rc != FLVIS_OK) {
    hipStreamSynchronize(st);  // (h_stage is reused by the next call)
    return rc;
  }
  const LcQueries q{hq, hq + n, nullptr, h_map ? h_map : h_stream, d_q, d_q + n, nullptr};
  return lc_search(lc, n, q, all_maps, false, n_best, fix_base, fix_stride, h_map != nullptr, what);
}

int flvis_loop_closer_localize(flvis_loop_closer* lc, int n, const int* h_stream, const uint8_t* d_img0, const void* d_img1, int n_best,
                               flvis_lc_fix* h_fix) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* const what = "loop_closer_localize";
  const int rc = lc_localize_check(lc, n, h_stream, n_best, h_fix, what);
  if (rc != FLVIS_OK) return rc;
  if (!d_img0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_localize: bad args");
  return lc_localize_run(lc, n, h_stream, nullptr, d_img0, d_img1, n_best, reinterpret_cast<char*>(h_fix), sizeof(flvis_lc_fix), what);
}

int flvis_loop_closer_localize_host(flvis_loop_closer* lc, int n, const int* h_stream, const flvis_image* h_img0, const flvis_image* h_img1,
                                    int n_best, flvis_lc_fix* h_fix) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* const what = "loop_closer_localize_host";
  const int rc = lc_localize_check(lc, n, h_stream, n_best, h_fix, what);
  if (rc != FLVIS_OK) return rc;
  if (!h_img0 || !h_img1) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_localize_host: bad args");
  return lc_on_host_images(lc, n, h_stream, h_img0, h_img1, what, [&](const uint8_t* d0, const uint8_t* d1) {
    return flvis_loop_closer_localize(lc, n, h_stream, d0, d1, n_best, h_fix);
  });
}

// the arguments of a localize_in call that both forms share, checked before anything is queued
static int lc_localize_in_check(flvis_loop_closer* lc, int n, const int* h_stream, const int* h_map, int n_best, const flvis_lc_fix_in* h_fix,
                                const std::string& what) {
  flvis_ctx* ctx = lc->ctx;
  if (!h_map || !h_fix) return ctx->fail(FLVIS_ERR_INVALID_ARG, what + ": bad args");
  const int rc = lc_localize_check(lc, n, h_stream, n_best, &h_fix->fix, what);
  if (rc != FLVIS_OK) return rc;
  for (int i = 0; i < n; i++)
    if (h_map[i] < FLVIS_LC_ALL_MAPS || h_map[i] >= lc->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, what + ": no such map");
  return FLVIS_OK;
}

// Where is this frame's camera in the map ANOTHER sequence has built, or in whichever map knows the place?
int flvis_loop_closer_localize_in(flvis_loop_closer* lc, int n, const int* h_stream, const int* h_map, const uint8_t* d_img0, const void* d_img1,
                                  int n_best, flvis_lc_fix_in* h_fix) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* const what = "loop_closer_localize_in";
  int rc = lc_localize_in_check(lc, n, h_stream, h_map, n_best, h_fix, what);
  if (rc != FLVIS_OK) return rc;
  if (!d_img0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_localize_in: bad args");
  return lc_localize_run(lc, n, h_stream, h_map, d_img0, d_img1, n_best, reinterpret_cast<char*>(h_fix), sizeof(flvis_lc_fix_in), what);
}

int flvis_loop_closer_localize_in_host(flvis_loop_closer* lc, int n, const int* h_stream, const int* h_map, const flvis_image* h_img0,
                                       const flvis_image* h_img1, int n_best, flvis_lc_fix_in* h_fix) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* const what = "loop_closer_localize_in_host";
  const int rc = lc_localize_in_check(lc, n, h_stream, h_map, n_best, h_fix, what);
  if (rc != FLVIS_OK) return rc;
  if (!h_img0 || !h_img1) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_localize_in_host: bad args");
  return lc_on_host_images(lc, n, h_stream, h_img0, h_img1, what, [&](const uint8_t* d0, const uint8_t* d1) {
    return flvis_loop_closer_localize_in(lc, n, h_stream, h_map, d0, d1, n_best, h_fix);
  });
}

// One pass of a link call: n <= n_streams queries (kf resolved), each the search's query by its keyframe's own database slot, with
// own_gap as a range of excluded slots.  all_maps: the call's row layout.
static int lc_link_pass(flvis_loop_closer* lc, int n, const flvis_lc_link_query* q, bool all_maps, int n_best, flvis_lc_fix_in* h_fix,
                        const char* what) {
  flvis_ctx* ctx = lc->ctx;
  const int maxkf = lc->maxkf;
  // one upload: the queries' slots, their sequences (= camera rows) and excluded ranges
  int* const hq = reinterpret_cast<int*>(lc->h_stage.data());
  std::vector<int> map((size_t)n);
  for (int i = 0; i < n; i++) {
    const int s = q[i].stream, kf = (int)q[i].kf;
    const int g = (int)std::min<int64_t>(q[i].own_gap, maxkf);
    hq[i] = s * maxkf + kf, hq[n + i] = s, map[i] = q[i].map;
    hq[2 * n + 2 * i] = s * maxkf + (g < 0 ? 0 : std::max(0, kf - g));
    hq[2 * n + 2 * i + 1] = g < 0 ? (s + 1) * maxkf : s * maxkf + std::min(lc->seq[s].n, kf + g + 1);
  }
  const int* const d_q = reinterpret_cast<const int*>(lc->stage);
  const hipError_t e = hipMemcpyAsync(lc->stage, hq, sizeof(int) * 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  const LcQueries lq{hq, hq + n, hq + 2 * n, map.data(), d_q, d_q + n, d_q + 2 * n};
  return lc_search(lc, n, lq, all_maps, true, n_best, reinterpret_cast<char*>(h_fix), sizeof(flvis_lc_fix_in), true, what);
}

int flvis_lc_links_from_fix(const flvis_lc_fix_in* fix, int stream, int64_t kf, int cap, flvis_lc_link* out) {
  if (!fix || cap < 0 || (cap > 0 && !out)) return -1;
  int cnt = 0;
  for (int r = 0; r < fix->fix.n_candidates && r < LCC_NBEST; r++) {
    if (!fix->fix.cand_accepted[r]) continue;
    if (cnt < cap) {
      flvis_lc_link& l = out[cnt];
      l.seq_from = fix->cand_seq[r], l.seq_to = stream, l.kf_from = fix->fix.cand_kf[r], l.kf_to = kf;
      memcpy(l.pose7, fix->fix.cand_pose7[r], sizeof(l.pose7));
    }
    cnt++;
  }
  return cnt;
}

int flvis_lc_link_reverse(const flvis_lc_link* in, flvis_lc_link* out) {
  if (!in || !out) return FLVIS_ERR_INVALID_ARG;
  double n2 = 0.0;
  for (int k = 0; k < 7; k++) {
    if (!std::isfinite(in->pose7[k])) return FLVIS_ERR_INVALID_ARG;
    if (k >= 3) n2 += in->pose7[k] * in->pose7[k];
  }
  const double nq = std::sqrt(n2);
  if (!(nq > 0.0) || !std::isfinite(nq)) return FLVIS_ERR_INVALID_ARG;
  // inv(q, t) = (conj(q), -R(conj(q)) t), as the device's iso_inv
  const double qi[4] = {-in->pose7[3] / nq, -in->pose7[4] / nq, -in->pose7[5] / nq, in->pose7[6] / nq};
  const double mt[3] = {-in->pose7[0], -in->pose7[1], -in->pose7[2]};
  flvis_lc_link o;
  o.seq_from = in->seq_to, o.seq_to = in->seq_from, o.kf_from = in->kf_to, o.kf_to = in->kf_from;
  q_rot(qi, mt, o.pose7);
  memcpy(o.pose7 + 3, qi, sizeof(qi));
  *out = o;
  return FLVIS_OK;
}

// Links and loops from stored keyframes: the arguments are checked before anything is queued, then the queries run in passes of n_streams
// (what the buffers are laid out for); the links are made on the host from the fixes.
int flvis_loop_closer_link(flvis_loop_closer* lc, int n, const flvis_lc_link_query* h_q, int n_best, flvis_lc_fix_in* h_fix, int link_cap,
                           flvis_lc_link* h_links, int* n_links) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* const what = "loop_closer_link";
  if (n <= 0 || !h_q || !h_fix || !n_links || link_cap < 0 || (link_cap > 0 && !h_links))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_link: bad args");
  if (n_best < 1 || n_best > LCC_NBEST) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_link: n_best must be 1 .. " + std::to_string(LCC_NBEST));
  std::vector<flvis_lc_link_query> q(h_q, h_q + n);
  bool all_maps = false;
  for (int i = 0; i < n; i++) {
    if (q[i].stream < 0 || q[i].stream >= lc->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_link: no such sequence");
    if (q[i].map < FLVIS_LC_ALL_MAPS || q[i].map >= lc->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_link: no such map");
    const int nk = lc->seq[q[i].stream].n;
    if (q[i].kf < -1 || q[i].kf >= nk || nk == 0)  // (-1 on an empty sequence names no keyframe: its slot was never written)
      return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_link: no such keyframe");
    if (q[i].own_gap < -1) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_link: own_gap must be -1 or >= 0");
    if (q[i].kf < 0) q[i].kf = nk - 1;
    all_maps = all_maps || q[i].map < 0;
  }
  hipSetDevice(ctx->device);
  int rc = lc_search_reserve(lc, all_maps, what);
  if (rc != FLVIS_OK) return rc;
  for (int i0 = 0; i0 < n; i0 += lc->S) {
    rc = lc_link_pass(lc, std::min(lc->S, n - i0), q.data() + i0, all_maps, n_best, h_fix + i0, what);
    if (rc != FLVIS_OK) return rc;
  }
  int cnt = 0;
  for (int i = 0; i < n; i++)
    for (int r = 0; r < h_fix[i].fix.n_candidates; r++) {
      if (!h_fix[i].fix.cand_accepted[r] || h_fix[i].cand_seq[r] == q[i].stream) continue;  // (its own sequence's: a loop, not a link)
      if (cnt < link_cap) {
        flvis_lc_link& l = h_links[cnt];
        l.seq_from = h_fix[i].cand_seq[r], l.seq_to = q[i].stream, l.kf_from = h_fix[i].fix.cand_kf[r], l.kf_to = q[i].kf;
        memcpy(l.pose7, h_fix[i].fix.cand_pose7[r], sizeof(l.pose7));
      }
      cnt++;
    }
  *n_links = cnt;
  return FLVIS_OK;
}

int flvis_loop_closer_set_drift(flvis_loop_closer* lc, int stream, const double* h_T_odom_map7) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  if (stream < 0 || stream >= lc->S || !h_T_odom_map7) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_set_drift: bad args");
  const double* const T = h_T_odom_map7;
  for (int k = 0; k < 7; k++)
    if (!std::isfinite(T[k])) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_set_drift: the pose is not finite");
  const double qn = std::sqrt(T[3] * T[3] + T[4] * T[4] + T[5] * T[5] + T[6] * T[6]);
  if (!(qn > 0) || !std::isfinite(qn)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_set_drift: zero quaternion");
  double* const M = lc->seq[stream].T_odom_map;
  for (int k = 0; k < 3; k++) M[k] = T[k];
  for (int k = 3; k < 7; k++) M[k] = T[k] / qn;
  return FLVIS_OK;
}

// Several sequences' maps into one map per group (include/flvis_hip.h has the definition).  Host: the checks, the virtual sequences' row
// table, loop lists and the sequences' vertex ranges; device: the rows out of the pose database (one launch), k_pgo through
// flvis_hip_pgo_loop_closure (one workgroup per group), the rows back with the tails and the drifts (one launch).  No pose but the
// sequences' drifts crosses to the host.
int flvis_loop_closer_merge(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, int n_links, const flvis_lc_link* h_links,
                            int iterations, flvis_lc_merge* h_out, double* h_drift7) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_merge: " + m); };
  if (!h_group_ptr || !h_seq || !h_links || !h_out || n_groups <= 0 || n_links < 0 || iterations < 0) return bad("bad args");
  if (h_group_ptr[0] != 0) return bad("h_group_ptr must start at 0");
  // ---- the groups: grp_of / pos_of per sequence of the closer (-1: in no group)
  std::vector<int> grp_of((size_t)lc->S, -1), pos_of((size_t)lc->S, -1);
  for (int g = 0; g < n_groups; g++) {
    const int b = h_group_ptr[g], e = h_group_ptr[g + 1];
    if (e < b || e - b < 2) return bad("a group needs at least two sequences");
    if (e > lc->S) return bad("the groups list more sequences than the closer has");
    for (int i = b; i < e; i++) {
      const int s = h_seq[i];
      if (s < 0 || s >= lc->S) return bad("sequence out of range");
      if (grp_of[s] >= 0) return bad("sequence " + std::to_string(s) + " is listed twice");
      if (lc->seq[s].n == 0) return bad("sequence " + std::to_string(s) + " is empty");
      grp_of[s] = g, pos_of[s] = i - b;
    }
  }
  // ---- the links; `root` joins the sequences a link ties (every non-anchor sequence must end up with its anchor)
  std::vector<int> root((size_t)lc->S);
  for (int s = 0; s < lc->S; s++) root[s] = s;
  auto find = [&](int s) {
    while (root[s] != s) s = root[s] = root[root[s]];
    return s;
  };
  std::vector<double> qnorm((size_t)n_links);  // |quaternion| per link: the pose is normalised as set_drift normalises its own
  for (int k = 0; k < n_links; k++) {
    const flvis_lc_link& l = h_links[k];
    const std::string lk = "link " + std::to_string(k);
    if (l.seq_from < 0 || l.seq_from >= lc->S || l.seq_to < 0 || l.seq_to >= lc->S) return bad(lk + ": sequence out of range");
    if (l.seq_from == l.seq_to) return bad(lk + ": both ends are in one sequence");
    if (grp_of[l.seq_from] < 0 || grp_of[l.seq_from] != grp_of[l.seq_to]) return bad(lk + ": its sequences are not both in one group");
    if (pos_of[l.seq_from] > pos_of[l.seq_to]) return bad(lk + ": its `from` sequence comes after its `to` sequence in the group");
    if (l.kf_from < 0 || l.kf_from >= lc->seq[l.seq_from].n || l.kf_to < 0 || l.kf_to >= lc->seq[l.seq_to].n) return bad(lk + ": no such keyframe");
    for (int c = 0; c < 7; c++)
      if (!std::isfinite(l.pose7[c])) return bad(lk + ": the pose is not finite");
    const double* const P = l.pose7;
    const double qn = std::sqrt(P[3] * P[3] + P[4] * P[4] + P[5] * P[5] + P[6] * P[6]);
    if (!(qn > 0) || !std::isfinite(qn)) return bad(lk + ": zero quaternion");
    qnorm[k] = qn;
    root[find(l.seq_from)] = find(l.seq_to);
  }
  const int NS = h_group_ptr[n_groups];
  for (int g = 0; g < n_groups; g++)
    for (int i = h_group_ptr[g] + 1; i < h_group_ptr[g + 1]; i++)
      if (find(h_seq[i]) != find(h_seq[h_group_ptr[g]]))
        return bad("no chain of links connects sequence " + std::to_string(h_seq[i]) + " to its group's anchor");
  // ---- the virtual sequences: rows (src: database slot, -1 absent), present flags, loop lists; per sequence its vertex range
  std::vector<int> n_kf((size_t)n_groups), n_loops((size_t)n_groups), ids, src, ran((size_t)n_groups, 0), v_off((size_t)NS);
  std::vector<uint8_t> present;
  std::vector<double> lp;
  std::vector<LcMergeSeq> tab((size_t)NS);
  std::vector<std::vector<int>> glinks((size_t)n_groups);  // a group's links, in the caller's order
  for (int k = 0; k < n_links; k++) glinks[grp_of[h_links[k].seq_from]].push_back(k);
  for (int g = 0; g < n_groups; g++) {
    const int b = h_group_ptr[g], e = h_group_ptr[g + 1];
    const size_t row0 = src.size(), loop0 = ids.size();
    for (int i = b; i < e; i++) {
      const int s = h_seq[i];
      const Seq& q = lc->seq[s];
      if (i > b) {  // five absent keyframes in a row cut the odometry chain (its edges reach the next five keyframes)
        src.insert(src.end(), 5, -1);
        present.insert(present.end(), 5, 0);
      }
      v_off[i] = (int)(src.size() - row0);
      tab[i] = LcMergeSeq{s * lc->maxkf, (int)src.size(), 0, q.n - 1, q.n};
      for (int k = 0; k < q.n; k++) src.push_back(s * lc->maxkf + k);
      present.insert(present.end(), (size_t)q.n, 1);
      for (int v : q.loop_ids) ids.push_back(v_off[i] + v);
      lp.insert(lp.end(), q.loop_poses.begin(), q.loop_poses.end());
    }
    for (int k : glinks[g]) {
      const flvis_lc_link& l = h_links[k];
      const double* const P = l.pose7;
      const double qn = qnorm[k];
      ids.push_back(v_off[b + pos_of[l.seq_from]] + (int)l.kf_from);
      ids.push_back(v_off[b + pos_of[l.seq_to]] + (int)l.kf_to);
      for (int c = 0; c < 7; c++) lp.push_back(c < 3 ? P[c] : P[c] / qn);
    }
    n_kf[g] = (int)(src.size() - row0);
    n_loops[g] = (int)((ids.size() - loop0) / 2);
    // the vertices run from min(earlier) to max(later) (vo_loopclosing.cpp:747-756).  Every link runs from an earlier to a later
    // sequence and every sequence hangs on the anchor, so the anchor starts some link and the last sequence ends one: min(earlier) is a
    // keyframe of the anchor, max(later) one of the last sequence, and every sequence has a vertex
    int kf_prev = INT_MAX, kf_curr = 0;
    for (size_t k = loop0; k < ids.size(); k += 2) kf_prev = std::min(kf_prev, ids[k]), kf_curr = std::max(kf_curr, ids[k + 1]);
    tab[b].first = kf_prev;
    tab[e - 1].v_s = kf_curr - v_off[e - 1];
  }
  // ---- buffers, on the first call and when a call needs more
  const size_t n_rows = src.size(), lp_bytes = sizeof(double) * lp.size(), src_bytes = sizeof(int) * n_rows;
  const size_t stage_bytes = lp_bytes + src_bytes + sizeof(LcMergeSeq) * (size_t)NS, n_out = (size_t)n_groups * 12 + (size_t)NS * 7;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  if (lc->mg_V_cap < n_rows * 7 || lc->mg_stage_cap < stage_bytes || lc->mg_out_cap < n_out) {
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_merge");
    if (!(lc->reserve(lc->mg_V, lc->mg_V_cap, n_rows * 7) && lc->reserve(lc->mg_stage, lc->mg_stage_cap, stage_bytes) &&
          lc->reserve(lc->mg_out, lc->mg_out_cap, n_out))) {
      (void)hipGetLastError();
      // (a buffer that did not grow keeps its size: a call that needs no more goes on, the next one that does tries again)
      return ctx->fail(FLVIS_ERR_HIP, "loop_closer_merge: device allocation failed");
    }
  }
  // ---- the call's one upload: loop poses | row table | sequence table
  lc->h_mg_stage.resize(stage_bytes);
  memcpy(lc->h_mg_stage.data(), lp.data(), lp_bytes);
  memcpy(lc->h_mg_stage.data() + lp_bytes, src.data(), src_bytes);
  memcpy(lc->h_mg_stage.data() + lp_bytes + src_bytes, tab.data(), sizeof(LcMergeSeq) * (size_t)NS);
  const double* const d_lp = reinterpret_cast<const double*>(lc->mg_stage);
  const int* const d_src = reinterpret_cast<const int*>(lc->mg_stage + lp_bytes);
  const LcMergeSeq* const d_tab = reinterpret_cast<const LcMergeSeq*>(lc->mg_stage + lp_bytes + src_bytes);
  double *const d_gdrift = lc->mg_out, *const d_stats = d_gdrift + 7 * (size_t)n_groups, *const d_drift = d_stats + 5 * (size_t)n_groups;
  e = hipMemcpyAsync(lc->mg_stage, lc->h_mg_stage.data(), stage_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_merge");
  int rc = flvis::lc_merge_gather_dev(ctx, d_src, (int)n_rows, lc->db_T, lc->mg_V);
  if (rc == FLVIS_OK)
    rc = flvis_hip_pgo_loop_closure(ctx, n_groups, n_kf.data(), lc->mg_V, present.data(), n_loops.data(), ids.data(), d_lp, iterations, 1, d_gdrift,
                                    d_stats, ran.data());
  // (a graph runs for every group that passed the checks: its loop ends are present keyframes inside min(earlier) .. max(later) and no
  //  loop ties a keyframe to itself.  A group that did not run would keep its gathered rows: the apply kernel then writes back what it
  //  read, with the identity as drift)
  if (rc == FLVIS_OK) rc = flvis::lc_merge_apply_dev(ctx, d_tab, NS, lc->mg_V, lc->db_T, d_drift);
  if (rc != FLVIS_OK) {
    hipStreamSynchronize(st);  // (h_mg_stage is reused by the next call)
    return rc;
  }
  lc->h_mg_out.resize(n_out);
  e = hipMemcpyAsync(lc->h_mg_out.data(), lc->mg_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_merge");
  const double *const stats = lc->h_mg_out.data() + 7 * (size_t)n_groups, *const drift = stats + 5 * (size_t)n_groups;
  for (int g = 0; g < n_groups; g++) {
    flvis_lc_merge& o = h_out[g];
    o.optimised = ran[g];
    o.iterations = (int)stats[5 * (size_t)g];
    o.chi2_before = stats[5 * (size_t)g + 1];
    o.chi2_after = stats[5 * (size_t)g + 2];
    o.n_vertices = (int)stats[5 * (size_t)g + 3];
    o.n_edges = (int)stats[5 * (size_t)g + 4];
  }
  for (int i = 0; i < NS; i++) {
    Seq& q = lc->seq[h_seq[i]];
    double m2[7];
    pose_mul(q.T_odom_map, drift + 7 * (size_t)i, m2);  // T_odom_map = T_odom_map * Tw1_w2 (:908), for every sequence of the group
    memcpy(q.T_odom_map, m2, sizeof(m2));
  }
  if (h_drift7) memcpy(h_drift7, drift, sizeof(double) * 7 * (size_t)NS);
  return FLVIS_OK;
}

// The maps as voxel clouds (include/flvis_hip.h): one row range per sequence over the landmark and pose databases, then
// flvis_hip_voxel_cloud.  Reads the database and writes nothing of the closer's.
static int lc_map_cloud_ranges(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int64_t* h_n_out,
                               std::vector<int>& range2) {
  flvis_ctx* ctx = lc->ctx;
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_map_cloud: " + m); };
  if (!h_group_ptr || !h_seq || !h_n_out || n_groups <= 0) return bad("bad args");
  if (h_group_ptr[0] != 0) return bad("h_group_ptr must start at 0");
  std::vector<int> seen((size_t)lc->S, -1);  // the last group that listed the sequence
  for (int g = 0; g < n_groups; g++) {
    if (h_group_ptr[g + 1] < h_group_ptr[g]) return bad("h_group_ptr decreases");
    for (int i = h_group_ptr[g]; i < h_group_ptr[g + 1]; i++) {
      const int s = h_seq[i];
      if (s < 0 || s >= lc->S) return bad("sequence out of range");
      if (seen[s] == g) return bad("sequence " + std::to_string(s) + " is listed twice in group " + std::to_string(g));
      seen[s] = g;
      range2.push_back(s * lc->maxkf);
      range2.push_back(lc->seq[s].n);
    }
  }
  return FLVIS_OK;
}

int flvis_loop_closer_map_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, double leaf, int min_points,
                                int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  std::vector<int> range2;
  const int rc = lc_map_cloud_ranges(lc, n_groups, h_group_ptr, h_seq, h_n_out, range2);
  if (rc != FLVIS_OK) return rc;
  return flvis_hip_voxel_cloud(lc->ctx, lc->db_lm3, lc->db_lmc, lc->db_T, lc->S * lc->maxkf, LCC_CAP, n_groups, h_group_ptr, range2.data(), leaf,
                               min_points, out_cap, d_xyz, d_npts, h_n_out, h_n_dropped);
}

int flvis_loop_closer_map_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, double leaf, int min_points,
                                     int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  std::vector<int> range2;
  int rc = lc_map_cloud_ranges(lc, n_groups, h_group_ptr, h_seq, h_n_out, range2);
  if (rc != FLVIS_OK) return rc;
  if (!h_xyz && out_cap > 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_map_cloud_host: NULL h_xyz");
  float* d_xyz = nullptr;
  int* d_npts = nullptr;
  if (out_cap > 0) {  // rows and counts of every group in one staging buffer of the context
    const size_t rows = (size_t)n_groups * (size_t)out_cap;
    d_xyz = (float*)ctx->scratch("mc_host_rows", rows * (3 * sizeof(float) + sizeof(int)));
    if (!d_xyz) {
      (void)hipGetLastError();
      return ctx->fail(FLVIS_ERR_HIP, "loop_closer_map_cloud_host: device allocation failed");
    }
    d_npts = (int*)(d_xyz + 3 * rows);
  }
  rc = flvis_hip_voxel_cloud(ctx, lc->db_lm3, lc->db_lmc, lc->db_T, lc->S * lc->maxkf, LCC_CAP, n_groups, h_group_ptr, range2.data(), leaf,
                             min_points, out_cap, d_xyz, h_npts ? d_npts : nullptr, h_n_out, h_n_dropped);
  if (rc != FLVIS_OK) return rc;
  hipError_t e = hipSuccess;
  bool any = false;
  for (int g = 0; g < n_groups && e == hipSuccess; g++) {
    const size_t n = (size_t)std::min<int64_t>(h_n_out[g], out_cap), at = (size_t)g * (size_t)out_cap;
    if (n == 0) continue;
    any = true;
    e = hipMemcpyAsync(h_xyz + 3 * at, d_xyz + 3 * at, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && h_npts) e = hipMemcpyAsync(h_npts + at, d_npts + at, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream);
  }
  if (any || e != hipSuccess) {
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_map_cloud_host");
  return FLVIS_OK;
}

// The dense map (include/flvis_hip.h): the tracker's logged depth images under the closer's stored poses.  Reads the log, the pose
// database and the sequences' configs; writes nothing of the closer's, the log's or the tracker's.
static int lc_dense_cloud(flvis_loop_closer* lc, const char* what, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                          const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                          int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid, bool check_only,
                          const flvis_dense_stereo_params* sprm = nullptr, double stereo_df = 0, bool unrect = false) {
  flvis_ctx* ctx = lc->ctx;
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  flvis::Pipeline* pl = ctx->pipe;
  if (!pl || pl->kfl.cap <= 0) return bad("the closer's context holds no tracker, or its keyframe log is off (flvis_keyframe_log_enable)");
  if (pl->S != lc->S || pl->kfl.w != lc->w || pl->kfl.h != lc->h || pl->cfg.cam_type != lc->cam_type)
    return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's n_streams, image_width, image_height and cam_type must be the closer's");
  if (!sprm && lc->cam_type != 2) return ctx->fail(FLVIS_ERR_CONFIG, pre + "the rig has no depth image");
  if (sprm && !unrect && lc->cam_type != 0) return ctx->fail(FLVIS_ERR_CONFIG, pre + "the rig is no rectified stereo pair (cam_type 0)");
  if (sprm && unrect && lc->cam_type != 1) return ctx->fail(FLVIS_ERR_CONFIG, pre + "the rig is no unrectified stereo pair (cam_type 1)");
  if (!prm) return bad("NULL prm");
  std::vector<int> range2;  // (first row of the pose database, stored keyframes) per listed sequence: the group checks of map_cloud
  int rc = lc_map_cloud_ranges(lc, n_groups, h_group_ptr, h_seq, h_n_out, range2);
  if (rc != FLVIS_OK) return rc;
  const int E = h_group_ptr[n_groups];
  std::vector<double> cam5(5 * (size_t)std::max(E, 1)), cam2(2 * (size_t)std::max(E, 1));
  std::vector<double> cam21_0(unrect ? 21 * (size_t)std::max(E, 1) : 0), cam21_1(cam21_0.size());  // (the raw cameras: rectify.hip)
  std::string why;
  for (int e = 0; e < E; e++) {
    const int s = h_seq[e], first = h_first_kf ? h_first_kf[e] : 0;
    if (first < 0 || first > lc->seq[s].n) return bad("a first keyframe outside [0, stored keyframes]");
    const flvis_cfg& g = lc->cfgs[s];
    const double v[5] = {g.P0[0], g.P0[5], g.P0[2], g.P0[6], sprm ? stereo_df : g.depth_factor};
    memcpy(&cam5[5 * (size_t)e], v, sizeof(v));
    cam2[2 * (size_t)e] = -g.P1[3], cam2[2 * (size_t)e + 1] = stereo_df;
    if (unrect) flvis::dc_unrect_cams(g, &cam21_0[21 * (size_t)e], &cam21_1[21 * (size_t)e]);
  }
  const flvis::DcUnrect un{E, cam21_0.data(), cam21_1.data()};
  rc = unrect && E > 0 ? flvis::rc_check(E, lc->w, lc->h, E, cam21_0.data(), nullptr, &why) : FLVIS_OK;
  if (unrect && E > 0 && rc == FLVIS_OK) rc = flvis::rc_check(E, lc->w, lc->h, E, cam21_1.data(), nullptr, &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  const double unit_cam[2] = {1.0, 1.0};
  rc = sprm ? flvis::ds_check(1, lc->w, lc->h, 1, unit_cam, sprm, &why) : FLVIS_OK;  // (the params alone, then each sequence's camera)
  for (int e = 0; sprm && rc == FLVIS_OK && e < E; e++) rc = flvis::ds_check(1, lc->w, lc->h, 1, &cam2[2 * (size_t)e], sprm, &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  rc = flvis::dc_check_sampling(lc->w, lc->h, prm, E, cam5.data(), &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  if (!(leaf >= 0) || !std::isfinite(leaf) || min_points < 1 || out_cap < 0 || (!d_xyz && out_cap > 0))
    return bad("leaf must be finite and >= 0, min_points >= 1, out_cap >= 0 with rows to write to");
  if (check_only) return FLVIS_OK;
  flvis::KfLogRec rec{};
  int S = 0, cam = 0;
  std::vector<long long> logged, dropped;
  rc = flvis::kf_log_settle(ctx, what, rec, S, cam, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  std::vector<int> eptr((size_t)n_groups + 1), img, pose, camv;
  for (int g = 0; g < n_groups; g++) {
    eptr[g] = (int)img.size();
    for (int e = h_group_ptr[g]; e < h_group_ptr[g + 1]; e++) {
      const int s = h_seq[e], first = h_first_kf ? h_first_kf[e] : 0;
      const long long n = std::min<long long>(logged[s], (long long)lc->seq[s].n - first);
      for (long long i = 0; i < n; i++) {
        if (img.size() >= (size_t)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 listed keyframes or more");
        img.push_back((int)((long long)s * rec.cap + i));
        pose.push_back((int)((long long)s * lc->maxkf + first + i));  // (first + i < stored <= maxkf)
        camv.push_back(e);
      }
    }
  }
  eptr[n_groups] = (int)img.size();
  if (sprm) {
    const uint16_t* d_z = nullptr;
    std::vector<int> iota;
    rc = flvis::dc_stereo_samples(ctx, what, rec, img, camv, cam2.data(), sprm, prm, &d_z, iota, unrect ? &un : nullptr);
    if (rc != FLVIS_OK) return rc;
    return flvis::dc_cloud(ctx, what, d_z, rec.w, rec.h, lc->db_T, 7, n_groups, eptr.data(), iota.data(), pose.data(), camv.data(), E,
                           cam5.data(), prm, leaf, min_points, out_cap, d_xyz, d_npts, h_n_out, h_n_dropped, h_n_valid, true);
  }
  return flvis::dc_cloud(ctx, what, reinterpret_cast<const uint16_t*>(rec.img1), rec.w, rec.h, lc->db_T, 7, n_groups, eptr.data(), img.data(),
                         pose.data(), camv.data(), E, cam5.data(), prm, leaf, min_points, out_cap, d_xyz, d_npts, h_n_out, h_n_dropped, h_n_valid);
}

int flvis_loop_closer_dense_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                  const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                                  int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  return lc_dense_cloud(lc, "loop_closer_dense_cloud", n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, d_xyz, d_npts,
                        h_n_out, h_n_dropped, h_n_valid, false);
}

int flvis_loop_closer_dense_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                       const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* h_xyz,
                                       int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  const char* what = "loop_closer_dense_cloud_host";
  int rc = lc_dense_cloud(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, h_xyz, nullptr, h_n_out, h_n_dropped,
                          h_n_valid, true);
  if (rc != FLVIS_OK) return rc;
  float* d_xyz = nullptr;
  int* d_npts = nullptr;
  rc = flvis::mc_host_rows_alloc(lc->ctx, what, n_groups, out_cap, &d_xyz, &d_npts);
  if (rc != FLVIS_OK) return rc;
  rc = lc_dense_cloud(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, d_xyz, h_npts ? d_npts : nullptr,
                      h_n_out, h_n_dropped, h_n_valid, false);
  if (rc != FLVIS_OK) return rc;
  return flvis::mc_host_rows_fetch(lc->ctx, what, n_groups, out_cap, h_n_out, d_xyz, d_npts, h_xyz, h_npts);
}

// The occupancy map (include/flvis_hip.h): lc_dense_cloud's lists -- the tracker's logged depth images under the closer's stored poses --
// through occupancy.hip's batched walk.  Reads the log, the pose database and the sequences' configs; writes nothing of theirs.
static int lc_occupancy(flvis_loop_closer* lc, const char* what, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                        const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int64_t max_records,
                        const flvis::OcOut& out, int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped, int* h_n_batches, bool check_only) {
  flvis_ctx* ctx = lc->ctx;
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  flvis::Pipeline* pl = ctx->pipe;
  if (!pl || pl->kfl.cap <= 0) return bad("the closer's context holds no tracker, or its keyframe log is off (flvis_keyframe_log_enable)");
  if (pl->S != lc->S || pl->kfl.w != lc->w || pl->kfl.h != lc->h || pl->cfg.cam_type != lc->cam_type)
    return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's n_streams, image_width, image_height and cam_type must be the closer's");
  if (lc->cam_type != 2) return ctx->fail(FLVIS_ERR_CONFIG, pre + "the rig has no depth image");
  if (!prm) return bad("NULL prm");
  std::vector<int> range2;
  int rc = lc_map_cloud_ranges(lc, n_groups, h_group_ptr, h_seq, h_n_out, range2);
  if (rc != FLVIS_OK) return rc;
  const int E = h_group_ptr[n_groups];
  std::vector<double> cam5(5 * (size_t)std::max(E, 1));
  for (int e = 0; e < E; e++) {
    const int s = h_seq[e], first = h_first_kf ? h_first_kf[e] : 0;
    if (first < 0 || first > lc->seq[s].n) return bad("a first keyframe outside [0, stored keyframes]");
    const flvis_cfg& g = lc->cfgs[s];
    const double v[5] = {g.P0[0], g.P0[5], g.P0[2], g.P0[6], g.depth_factor};
    memcpy(&cam5[5 * (size_t)e], v, sizeof(v));
  }
  std::string why;
  rc = flvis::dc_check_sampling(lc->w, lc->h, prm, E, cam5.data(), &why);
  if (rc == FLVIS_OK) rc = flvis::oc_check_values(leaf, occ, &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  if (max_records < 0 || out.out_cap < 0 || ((!out.d_key || !out.d_l) && out.out_cap > 0))
    return bad("max_records >= 0 and out_cap >= 0 with rows to write to");
  if (check_only) return FLVIS_OK;
  flvis::KfLogRec rec{};
  int S = 0, cam = 0;
  std::vector<long long> logged, dropped;
  rc = flvis::kf_log_settle(ctx, what, rec, S, cam, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  std::vector<int> eptr((size_t)n_groups + 1), img, pose, camv, item_seq, item_entry;
  for (int g = 0; g < n_groups; g++) {
    eptr[g] = (int)img.size();
    for (int e = h_group_ptr[g]; e < h_group_ptr[g + 1]; e++) {
      const int s = h_seq[e], first = h_first_kf ? h_first_kf[e] : 0;
      const long long n = std::min<long long>(logged[s], (long long)lc->seq[s].n - first);
      for (long long i = 0; i < n; i++) {
        if (img.size() >= (size_t)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 listed keyframes or more");
        img.push_back((int)((long long)s * rec.cap + i));
        pose.push_back((int)((long long)s * lc->maxkf + first + i));  // (first + i < stored <= maxkf)
        camv.push_back(e), item_seq.push_back(s), item_entry.push_back((int)i);
      }
    }
  }
  eptr[n_groups] = (int)img.size();
  const flvis::OcLists L{reinterpret_cast<const uint16_t*>(rec.img1), rec.w, rec.h, lc->db_T, 7, n_groups, eptr.data(), img.data(), pose.data(),
                         camv.data(), E, cam5.data()};
  return flvis::oc_batched(ctx, what, L, prm, leaf, occ, max_records, out, h_n_out, h_n_rays, h_n_dropped, h_n_batches, [&](int e) {
    return "entry " + std::to_string(item_entry[e]) + " of stream " + std::to_string(item_seq[e]);
  });
}

int flvis_loop_closer_occupancy(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int64_t max_records,
                                int out_cap, int64_t* d_key, float* d_l, float* d_xyz, int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped,
                                int* h_n_batches) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  return lc_occupancy(lc, "loop_closer_occupancy", n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, occ, max_records,
                      flvis::OcOut{out_cap, d_key, d_l, d_xyz}, h_n_out, h_n_rays, h_n_dropped, h_n_batches, false);
}

int flvis_loop_closer_occupancy_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                     const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int64_t max_records,
                                     int out_cap, int64_t* h_key, float* h_l, float* h_xyz, int64_t* h_n_out, int64_t* h_n_rays,
                                     int64_t* h_n_dropped, int* h_n_batches) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  const char* what = "loop_closer_occupancy_host";
  int rc = lc_occupancy(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, occ, max_records, flvis::OcOut{out_cap, h_key, h_l, h_xyz},
                        h_n_out, h_n_rays, h_n_dropped, h_n_batches, true);
  if (rc != FLVIS_OK) return rc;
  flvis::OcOut dev;
  rc = flvis::oc_host_alloc(lc->ctx, what, n_groups, out_cap, h_xyz != nullptr, &dev);
  if (rc != FLVIS_OK) return rc;
  rc = lc_occupancy(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, occ, max_records, dev, h_n_out, h_n_rays, h_n_dropped, h_n_batches,
                    false);
  if (rc != FLVIS_OK) return rc;
  return flvis::oc_host_fetch(lc->ctx, what, n_groups, dev, h_n_out, h_key, h_l, h_xyz);
}

int flvis_loop_closer_stereo_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                   const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm, double leaf,
                                   int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out, int64_t* h_n_dropped,
                                   int64_t* h_n_valid) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  if (!sprm) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_stereo_cloud: NULL stereo params");
  return lc_dense_cloud(lc, "loop_closer_stereo_cloud", n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, d_xyz, d_npts,
                        h_n_out, h_n_dropped, h_n_valid, false, sprm, depth_factor);
}

int flvis_loop_closer_stereo_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                        const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm,
                                        double leaf, int min_points, int out_cap, float* h_xyz, int* h_npts, int64_t* h_n_out,
                                        int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  const char* what = "loop_closer_stereo_cloud_host";
  if (!sprm) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": NULL stereo params");
  int rc = lc_dense_cloud(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, h_xyz, nullptr, h_n_out, h_n_dropped,
                          h_n_valid, true, sprm, depth_factor);
  if (rc != FLVIS_OK) return rc;
  float* d_xyz = nullptr;
  int* d_npts = nullptr;
  rc = flvis::mc_host_rows_alloc(lc->ctx, what, n_groups, out_cap, &d_xyz, &d_npts);
  if (rc != FLVIS_OK) return rc;
  rc = lc_dense_cloud(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, d_xyz, h_npts ? d_npts : nullptr,
                      h_n_out, h_n_dropped, h_n_valid, false, sprm, depth_factor);
  if (rc != FLVIS_OK) return rc;
  return flvis::mc_host_rows_fetch(lc->ctx, what, n_groups, out_cap, h_n_out, d_xyz, d_npts, h_xyz, h_npts);
}

// the same on the unrectified rig (cam_type 1): the logged pairs are rectified in front of the matcher (rectify.hip)
int flvis_loop_closer_unrect_stereo_cloud(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq, const int* h_first_kf,
                                          const flvis_dense_stereo_params* sprm, double depth_factor, const flvis_depth_cloud_params* prm,
                                          double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, int64_t* h_n_out,
                                          int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  if (!sprm) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_unrect_stereo_cloud: NULL stereo params");
  return lc_dense_cloud(lc, "loop_closer_unrect_stereo_cloud", n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, d_xyz,
                        d_npts, h_n_out, h_n_dropped, h_n_valid, false, sprm, depth_factor, true);
}

int flvis_loop_closer_unrect_stereo_cloud_host(flvis_loop_closer* lc, int n_groups, const int* h_group_ptr, const int* h_seq,
                                               const int* h_first_kf, const flvis_dense_stereo_params* sprm, double depth_factor,
                                               const flvis_depth_cloud_params* prm, double leaf, int min_points, int out_cap, float* h_xyz,
                                               int* h_npts, int64_t* h_n_out, int64_t* h_n_dropped, int64_t* h_n_valid) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  const char* what = "loop_closer_unrect_stereo_cloud_host";
  if (!sprm) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": NULL stereo params");
  int rc = lc_dense_cloud(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, h_xyz, nullptr, h_n_out, h_n_dropped,
                          h_n_valid, true, sprm, depth_factor, true);
  if (rc != FLVIS_OK) return rc;
  float* d_xyz = nullptr;
  int* d_npts = nullptr;
  rc = flvis::mc_host_rows_alloc(lc->ctx, what, n_groups, out_cap, &d_xyz, &d_npts);
  if (rc != FLVIS_OK) return rc;
  rc = lc_dense_cloud(lc, what, n_groups, h_group_ptr, h_seq, h_first_kf, prm, leaf, min_points, out_cap, d_xyz, h_npts ? d_npts : nullptr,
                      h_n_out, h_n_dropped, h_n_valid, false, sprm, depth_factor, true);
  if (rc != FLVIS_OK) return rc;
  return flvis::mc_host_rows_fetch(lc->ctx, what, n_groups, out_cap, h_n_out, d_xyz, d_npts, h_xyz, h_npts);
}

// ---- keyframe stamps and whole trajectories in the map frame (include/flvis_hip.h; the rule and the kernels: lc_traj.hip) ---------------
// may keyframes first .. first + n - 1 of the sequence get these stamps?  Finite, strictly increasing, above the last set stamp before
// them and below the first set stamp behind them
static bool lc_stamps_fit(const Seq& q, int first, int n, const double* t) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(t[i]) || (i > 0 && !(t[i - 1] < t[i]))) return false;
  if (n == 0) return true;
  for (int k = first - 1; k >= 0; k--)
    if (!std::isnan(q.stamp[k])) {
      if (!(q.stamp[k] < t[0])) return false;
      break;
    }
  for (int k = first + n; k < q.n; k++)
    if (!std::isnan(q.stamp[k])) {
      if (!(t[n - 1] < q.stamp[k])) return false;
      break;
    }
  return true;
}

// the stamp of the keyframe add_logged has just stored, where the sequence's stamps stay strictly increasing with it (a log fed twice:
// the second copy stays unset)
static void lc_stamp_logged(Seq& q, double stamp) {
  if (lc_stamps_fit(q, q.n - 1, 1, &stamp)) q.stamp[(size_t)q.n - 1] = stamp;
}

int flvis_loop_closer_set_keyframe_stamps(flvis_loop_closer* lc, int stream, int first_kf, int n, const double* h_stamps) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* what = "loop_closer_set_keyframe_stamps";
  if (stream < 0 || stream >= lc->S || first_kf < 0 || n < 0 || (n > 0 && !h_stamps))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": bad args");
  Seq& q = lc->seq[stream];
  if ((long long)first_kf + n > (long long)q.n)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": the sequence holds no such keyframes");
  if (!lc_stamps_fit(q, first_kf, n, h_stamps))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": the stamps of sequence " + std::to_string(stream) +
                                                " would not be finite and strictly increasing");
  if (n == 0) return FLVIS_OK;
  std::copy(h_stamps, h_stamps + n, q.stamp.begin() + first_kf);
  q.uploaded = std::min(q.uploaded, first_kf);  // (the device tables are behind from here on)
  return FLVIS_OK;
}

int flvis_loop_closer_keyframe_stamps(flvis_loop_closer* lc, int stream, double* h_stamps, int cap, int* n_out) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  if (stream < 0 || stream >= lc->S || !h_stamps || !n_out || cap < 0) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_keyframe_stamps: bad args");
  const Seq& q = lc->seq[stream];
  *n_out = q.n;
  std::copy(q.stamp.begin(), q.stamp.begin() + std::min(cap, q.n), h_stamps);
  return FLVIS_OK;
}

// What a map_poses call needs before its kernels: the jobs checked, every named sequence fully stamped, and O_k / tau_k of the keyframes
// added since a sequence's last upload queued for the device tables (the caller synchronises).  h_nkf [S], h_drift [S][7]: the
// sequences' counts and T_odom_map.
static int lc_traj_prepare(flvis_loop_closer* lc, const char* what, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode, std::vector<int>& h_nkf,
                           std::vector<double>& h_drift) {
  flvis_ctx* ctx = lc->ctx;
  h_nkf.resize((size_t)lc->S), h_drift.resize(7 * (size_t)lc->S);
  for (int s = 0; s < lc->S; s++) {
    h_nkf[s] = lc->seq[s].n;
    memcpy(&h_drift[7 * (size_t)s], lc->seq[s].T_odom_map, 56);
  }
  int rc = flvis::lc_map_poses_check(ctx, what, lc->S, lc->maxkf, h_nkf.data(), n_jobs, h_jobs, mode);
  if (rc != FLVIS_OK) return rc;
  std::vector<char> named((size_t)lc->S, 0);
  for (int i = 0; i < n_jobs; i++)
    if (h_jobs[i].n > 0) named[h_jobs[i].seq] = 1;
  for (int s = 0; s < lc->S; s++) {
    if (!named[s]) continue;
    const Seq& q = lc->seq[s];
    for (int k = 0; k < q.n; k++)
      if (std::isnan(q.stamp[k]))
        return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": sequence " + std::to_string(s) + ": keyframe " + std::to_string(k) +
                                                    " has no stamp (flvis_loop_closer_set_keyframe_stamps)");
  }
  hipSetDevice(ctx->device);
  const size_t slots = (size_t)lc->S * lc->maxkf;
  if (!((lc->tj_T_odom || lc->alloc(lc->tj_T_odom, slots * 7)) && (lc->tj_stamps || lc->alloc(lc->tj_stamps, slots)))) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  hipError_t e = hipSuccess;
  for (int s = 0; s < lc->S && e == hipSuccess; s++) {
    Seq& q = lc->seq[s];
    if (!named[s] || q.uploaded >= q.n) continue;
    const size_t at = (size_t)s * lc->maxkf + q.uploaded, cnt = (size_t)(q.n - q.uploaded);
    e = hipMemcpyAsync(lc->tj_T_odom + at * 7, &q.T_odom[7 * (size_t)q.uploaded], sizeof(double) * 7 * cnt, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lc->tj_stamps + at, &q.stamp[(size_t)q.uploaded], sizeof(double) * cnt, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e != hipSuccess) {
    hipStreamSynchronize(ctx->stream);  // (copies out of the host mirrors may be in flight)
    return ctx->hip_fail(e, what);
  }
  return FLVIS_OK;
}

// ... and behind them: lc_map_poses_dev returns synchronised, so the uploads are done, whatever it says
static int lc_traj_run(flvis_loop_closer* lc, const char* what, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode, const std::vector<int>& h_nkf,
                       const std::vector<double>& h_drift) {
  const int rc = flvis::lc_map_poses_dev(lc->ctx, what, lc->S, lc->maxkf, h_nkf.data(), lc->tj_T_odom, lc->db_T, lc->tj_stamps, h_drift.data(),
                                         n_jobs, h_jobs, mode, false);
  if (hipStreamSynchronize(lc->ctx->stream) == hipSuccess)
    for (int i = 0; i < n_jobs; i++)
      if (h_jobs[i].n > 0) lc->seq[h_jobs[i].seq].uploaded = lc->seq[h_jobs[i].seq].n;
  return rc;
}

int flvis_loop_closer_map_poses(flvis_loop_closer* lc, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  const char* what = "loop_closer_map_poses";
  std::vector<int> h_nkf;
  std::vector<double> h_drift;
  const int rc = lc_traj_prepare(lc, what, n_jobs, h_jobs, mode, h_nkf, h_drift);
  if (rc != FLVIS_OK) return rc;
  return lc_traj_run(lc, what, n_jobs, h_jobs, mode, h_nkf, h_drift);
}

int flvis_loop_closer_map_poses_host(flvis_loop_closer* lc, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* what = "loop_closer_map_poses_host";
  std::vector<int> h_nkf;
  std::vector<double> h_drift;
  int rc = lc_traj_prepare(lc, what, n_jobs, h_jobs, mode, h_nkf, h_drift);
  if (rc != FLVIS_OK) return rc;
  // the jobs' rows behind one another in the context's workspace (mapped in place), the anchors behind the rows
  size_t n_dbl = 0, n_rows = 0;
  for (int i = 0; i < n_jobs; i++) n_dbl += (size_t)h_jobs[i].n * flvis::lct_row_width(h_jobs[i].kind), n_rows += (size_t)h_jobs[i].n;
  hipStream_t st = ctx->stream;
  if (n_rows == 0) {
    hipStreamSynchronize(st);
    return FLVIS_OK;
  }
  double* const d_rows = (double*)ctx->scratch("lct_host_rows", n_dbl * sizeof(double) + n_rows * sizeof(int));
  if (!d_rows) {
    (void)hipGetLastError();
    hipStreamSynchronize(st);
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  int* const d_anchor = reinterpret_cast<int*>(d_rows + n_dbl);
  std::vector<flvis_lc_traj_job> jobs(h_jobs, h_jobs + n_jobs);
  hipError_t e = hipSuccess;
  size_t at = 0, row = 0;
  for (int i = 0; i < n_jobs && e == hipSuccess; i++) {
    flvis_lc_traj_job& j = jobs[i];
    const size_t cnt = (size_t)j.n * flvis::lct_row_width(j.kind);
    j.d_in = j.d_out = d_rows + at;
    j.d_anchor = d_anchor + row;
    if (cnt) e = hipMemcpyAsync(d_rows + at, h_jobs[i].d_in, cnt * sizeof(double), hipMemcpyHostToDevice, st);
    at += cnt, row += (size_t)j.n;
  }
  if (e != hipSuccess) {
    hipStreamSynchronize(st);
    return ctx->hip_fail(e, what);
  }
  rc = lc_traj_run(lc, what, n_jobs, jobs.data(), mode, h_nkf, h_drift);
  if (rc != FLVIS_OK) return rc;
  for (int i = 0; i < n_jobs && e == hipSuccess; i++) {
    const flvis_lc_traj_job& j = jobs[i];
    if (j.n == 0) continue;
    e = hipMemcpyAsync(h_jobs[i].d_out, j.d_out, (size_t)j.n * flvis::lct_row_width(j.kind) * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && h_jobs[i].d_anchor) e = hipMemcpyAsync(h_jobs[i].d_anchor, j.d_anchor, (size_t)j.n * sizeof(int), hipMemcpyDeviceToHost, st);
  }
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}

int flvis_loop_closer_map_trajectory(flvis_loop_closer* lc, int n, const int* h_stream, int first_frame, int n_frames, int mode, double* d_out_rows9,
                                     double* h_out_rows9, int* h_anchor) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* what = "loop_closer_map_trajectory";
  if (n <= 0 || !h_stream) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": bad args");
  for (int i = 0; i < n; i++)
    if (h_stream[i] < 0 || h_stream[i] >= lc->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": stream out of range");
  int S = 0, w = 0, h = 0, cam = 0;
  std::vector<const double*> d_traj;
  std::vector<int> cap;
  if (flvis::lc_traj_tracker_rows(ctx, S, w, h, cam, d_traj, cap) != FLVIS_OK)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": the closer's context holds no tracker (flvis_tracker_create)");
  if (S != lc->S || w != lc->w || h != lc->h || cam != lc->cam_type)
    return ctx->fail(FLVIS_ERR_CONFIG, std::string(what) + ": the tracker's n_streams, image_width, image_height and cam_type must be the closer's");
  for (int i = 0; i < n; i++) {
    const int s = h_stream[i];
    if (!d_traj[s]) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": the tracker keeps no trajectory record (traj_capacity)");
    if (first_frame < 0 || n_frames < 0 || (long long)first_frame + n_frames > (long long)cap[s])
      return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": out of range");
  }
  const size_t rows = (size_t)n * (size_t)n_frames;
  double* d_out = d_out_rows9;
  int* d_anchor = nullptr;
  if (rows > 0 && (!d_out || h_anchor)) {  // the outputs the caller keeps on the host alone: through the context's workspace
    uint8_t* const p = (uint8_t*)ctx->scratch("lct_traj_out", rows * (9 * sizeof(double) + sizeof(int)));
    if (!p) {
      (void)hipGetLastError();
      return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
    }
    if (!d_out) d_out = reinterpret_cast<double*>(p);
    if (h_anchor) d_anchor = reinterpret_cast<int*>(p + rows * 9 * sizeof(double));
  }
  std::vector<flvis_lc_traj_job> jobs((size_t)n);
  for (int i = 0; i < n; i++) {
    const size_t at = (size_t)i * (size_t)n_frames;
    jobs[i] = flvis_lc_traj_job{h_stream[i], FLVIS_LC_ROWS_TRAJ9, n_frames, d_traj[h_stream[i]] + (size_t)first_frame * 9,
                                d_out ? d_out + at * 9 : nullptr, d_anchor ? d_anchor + at : nullptr};
  }
  std::vector<int> h_nkf;
  std::vector<double> h_drift;
  int rc = lc_traj_prepare(lc, what, n, jobs.data(), mode, h_nkf, h_drift);
  if (rc != FLVIS_OK) return rc;
  rc = lc_traj_run(lc, what, n, jobs.data(), mode, h_nkf, h_drift);
  if (rc != FLVIS_OK || rows == 0) return rc;
  hipError_t e = hipSuccess;
  if (h_out_rows9) e = hipMemcpyAsync(h_out_rows9, d_out, rows * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && h_anchor) e = hipMemcpyAsync(h_anchor, d_anchor, rows * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (h_out_rows9 || h_anchor) {
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}

// The tracker's keyframe log (flvis_keyframe_log_enable) into the closer, without an image leaving the device.  Round r takes entry r of
// every stream that has one: k_kf_log_gather lays their images out as add_keyframes takes them, and the round IS that call (and process).
// Sequences are independent in the closer and a stream has at most one keyframe per step, so each sequence sees its keyframes one by one
// in order, exactly as a caller that adds and processes after every keyframe.
int flvis_loop_closer_add_logged(flvis_loop_closer* lc, int process, flvis_lc_event* h_events, int events_cap, int* n_rounds) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  const char* what = "loop_closer_add_logged";
  flvis::KfLogRec rec{};
  int S = 0, cam = 0;
  std::vector<long long> logged, dropped;
  int rc = flvis::kf_log_settle(ctx, what, rec, S, cam, logged, dropped);
  if (rc == FLVIS_ERR_INVALID_ARG)
    return ctx->fail(rc, std::string(what) + ": the closer's context holds no tracker, or its keyframe log is off (flvis_keyframe_log_enable)");
  if (rc != FLVIS_OK) return rc;
  if (S != lc->S || rec.w != lc->w || rec.h != lc->h || cam != lc->cam_type)
    return ctx->fail(FLVIS_ERR_CONFIG, std::string(what) + ": the tracker's n_streams, image_width, image_height and cam_type must be the closer's");
  // all or nothing: every refusal before anything is stored
  int rounds = 0;
  for (int s = 0; s < S; s++) {
    if ((long long)lc->seq[s].n + logged[s] > (long long)lc->maxkf)
      return ctx->fail(FLVIS_ERR_CAPACITY, std::string(what) + ": sequence " + std::to_string(s) + " has no room for its logged keyframes");
    rounds = std::max(rounds, (int)logged[s]);
  }
  if (process && h_events && events_cap < rounds)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": events_cap is smaller than the number of rounds");
  if (n_rounds) *n_rounds = rounds;
  if (rounds == 0) return FLVIS_OK;
  hipStream_t st = ctx->stream;
  const size_t px = rec.px();
  // the logged poses (KeyFrame.msg T_c_w: the round's T_c_w_odom) and, behind each, its header.stamp, stream by stream
  static_assert(offsetof(flvis::KeyFrameDev, stamp) == offsetof(flvis::KeyFrameDev, T_c_w) + 56, "T_c_w and stamp are copied as one block");
  std::vector<std::vector<double>> T((size_t)S);
  for (int s = 0; s < S; s++) {
    if (logged[s] == 0) continue;
    T[s].resize(8 * (size_t)logged[s]);
    const char* src = reinterpret_cast<const char*>(rec.kf + (size_t)s * rec.cap) + offsetof(flvis::KeyFrameDev, T_c_w);
    const hipError_t e = hipMemcpy2D(T[s].data(), 64, src, sizeof(flvis::KeyFrameDev), 64, (size_t)logged[s], hipMemcpyDeviceToHost);
    if (e != hipSuccess) return ctx->hip_fail(e, what);
  }
  // every round's stream and entry lists in one upload: [rounds][2][S]
  std::vector<int> lists((size_t)rounds * 2 * S, -1);
  std::vector<int> cnt((size_t)rounds, 0);
  for (int r = 0; r < rounds; r++)
    for (int s = 0; s < S; s++)
      if (logged[s] > r) {
        int* l = &lists[(size_t)r * 2 * S];
        l[cnt[r]] = s, l[S + cnt[r]] = r;
        cnt[r]++;
      }
  int* const d_lists = (int*)ctx->scratch("lc_log_lists", sizeof(int) * lists.size());
  uint8_t* const d0 = (uint8_t*)ctx->scratch("lc_log_img0", px * (size_t)S);
  uint8_t* const d1 = (uint8_t*)ctx->scratch("lc_log_img1", px * rec.bpp1 * (size_t)S);
  if (!d_lists || !d0 || !d1) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": staging allocation failed");
  }
  hipError_t e = hipMemcpyAsync(d_lists, lists.data(), sizeof(int) * lists.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  std::vector<double> Tr(7 * (size_t)S);
  std::vector<flvis_lc_event> ev_tmp;
  if (process && !h_events) ev_tmp.resize((size_t)S);
  for (int r = 0; r < rounds; r++) {
    const int n = cnt[r];
    const int* l = &lists[(size_t)r * 2 * S];
    for (int i = 0; i < n; i++) memcpy(&Tr[7 * (size_t)i], &T[l[i]][8 * (size_t)r], 56);
    flvis::launch_kf_log_gather(st, rec, n, d_lists + (size_t)r * 2 * S, d_lists + (size_t)r * 2 * S + S, d0, d1);
    e = hipGetLastError();
    if (e != hipSuccess) return ctx->hip_fail(e, what);
    rc = flvis_loop_closer_add_keyframes(lc, n, l, d0, d1, Tr.data(), nullptr);
    if (rc == FLVIS_OK)
      for (int i = 0; i < n; i++) lc_stamp_logged(lc->seq[l[i]], T[l[i]][8 * (size_t)r + 7]);
    if (rc == FLVIS_OK && process) rc = flvis_loop_closer_process(lc, h_events ? h_events + (size_t)r * S : ev_tmp.data());
    if (rc != FLVIS_OK) return rc;
  }
  return FLVIS_OK;
}

int flvis_loop_closer_poses(flvis_loop_closer* lc, int stream, double* h_T_c_w7, int cap, int* n_out) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  if (stream < 0 || stream >= lc->S || !h_T_c_w7 || !n_out || cap < 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_poses: bad args");
  const int n = std::min(cap, lc->seq[stream].n);
  *n_out = lc->seq[stream].n;
  if (n == 0) return FLVIS_OK;
  hipSetDevice(ctx->device);
  hipError_t e = hipMemcpyAsync(h_T_c_w7, lc->db_T + (size_t)stream * lc->maxkf * 7, sizeof(double) * 7 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_poses");
  return FLVIS_OK;
}

// one keyframe of the database back on the host (KeyFrameLC: lm_2d / lm_3d / lm_descriptor / kf_bv, :100-112); any output may be NULL
int flvis_loop_closer_keyframe(flvis_loop_closer* lc, int stream, int kf, int cap, float* h_lm_2d, double* h_lm_3d, uint8_t* h_lm_desc,
                               int* lm_count, int* h_bow_ids, double* h_bow_vals, int* bow_count) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  flvis_ctx* ctx = lc->ctx;
  if (stream < 0 || stream >= lc->S || kf < 0 || kf >= lc->seq[stream].n || cap < 0)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_keyframe: no such keyframe");
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t slot = (size_t)stream * lc->maxkf + kf;
  int cnt[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(&cnt[0], lc->db_lmc + slot, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&cnt[1], lc->db_nnz + slot, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_keyframe");
  const size_t nl = (size_t)std::min(cnt[0], cap), nv = (size_t)std::min(cnt[1], cap);
  if (h_lm_2d && nl) e = hipMemcpyAsync(h_lm_2d, lc->db_lm2 + slot * LCC_CAP * 2, sizeof(float) * 2 * nl, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && h_lm_3d && nl) e = hipMemcpyAsync(h_lm_3d, lc->db_lm3 + slot * LCC_CAP * 3, sizeof(double) * 3 * nl, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && h_lm_desc && nl) e = hipMemcpyAsync(h_lm_desc, lc->db_lmd + slot * LCC_CAP * 32, 32 * nl, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && h_bow_ids && nv) e = hipMemcpyAsync(h_bow_ids, lc->db_ids + slot * LCC_VCAP, sizeof(int) * nv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && h_bow_vals && nv) e = hipMemcpyAsync(h_bow_vals, lc->db_vals + slot * LCC_VCAP, sizeof(double) * nv, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, "loop_closer_keyframe");
  if (lm_count) *lm_count = cnt[0];
  if (bow_count) *bow_count = cnt[1];
  return FLVIS_OK;
}

int flvis_loop_closer_drift(flvis_loop_closer* lc, int stream, double* h_T_odom_map7) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  if (stream < 0 || stream >= lc->S || !h_T_odom_map7) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_drift: bad args");
  memcpy(h_T_odom_map7, lc->seq[stream].T_odom_map, 7 * sizeof(double));
  return FLVIS_OK;
}

int flvis_loop_closer_similarity_row(flvis_loop_closer* lc, int stream, double* h_row, int cap, int* n_out) {
  if (!lc) return FLVIS_ERR_INVALID_ARG;
  if (stream < 0 || stream >= lc->S || !h_row || !n_out || cap < 0) return lc->ctx->fail(FLVIS_ERR_INVALID_ARG, "loop_closer_similarity_row: bad args");
  const int n = lc->seq[stream].n;
  *n_out = n;
  memcpy(h_row, &lc->h_rows[(size_t)stream * lc->maxkf], sizeof(double) * (size_t)std::min(n, cap));
  return FLVIS_OK;
}
}
