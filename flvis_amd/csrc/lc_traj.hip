// flvis_amd: whole trajectories in the map frame (flvis_hip_lc_map_poses; include/flvis_hip.h has the definition).
//
// The loop closer corrects keyframes: after its pose graphs and merges the database holds M_k = T_c_w of keyframe k in the map frame,
// while the tracker's per-frame record and the /imu_pose rows stay in the odometry frame.  The reference shows them through ONE tf
// map -> odom, the newest drift (vo_loopclosing.cpp:908), which is right only for frames at or after the newest keyframe.  Here every
// keyframe carries its own drift D_k = inv(O_k) * M_k (O_k: the odometry pose it was added with), a row with stamp t is anchored at the
// last keyframe at or before t, and takes that keyframe's drift or, in blend mode, the chord between it and the next one.
//   k_lc_kf_drift    one thread per keyframe of the sequences the call names: D_k (and, for the kernel-level call, whether the
//                    sequence's stamps are finite and strictly increasing)
//   k_lc_map_poses   grid (row tiles, jobs), one thread per row: the tile's rows through LDS (coalesced both ways: a row is 8, 9 or 11
//                    doubles), the anchor search, the blend, the product
// The kernel moves bytes -- 72 in, 72 out and 4 of anchor per trajectory row -- and the tables (64 bytes per keyframe) stay in L2, where
// each row does its own upper-bound search: rows of a tile that lie close in time (the common case: a trajectory in order) walk the same
// few cache lines.  Staging the tile's span of stamps and drifts in LDS was built and measured (profiles/r24_lc_traj.md): it bought
// nothing over the cached search and its LDS cost occupancy, so the rows are all the LDS holds -- sized by the call's widest row kind,
// eight workgroups per CU for trajectory rows.  One search, one table: a row's result does not depend on where it stands in a job.
// No atomics; every store is a vector store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "lc_traj.hpp"
#include "pipeline_host.hpp"

namespace {

using namespace flvis;

constexpr int LCT_T = 256;  // threads per workgroup = rows per tile

// what the kernels read of a job and of a sequence (one upload per call)
struct LctJob {
  const double* in;
  double* out;
  int* anchor;
  int seq, kind, n, pad;
};
struct LctSeq {
  double drift[7];  // T_odom_map: the drift of every row of an empty sequence
  int n_kf, pad;
};

__global__ __launch_bounds__(LCT_T) void k_lc_kf_drift(const int* __restrict__ named, const LctSeq* __restrict__ seqs, int kf_stride,
                                                       const double* __restrict__ T_odom, const double* __restrict__ T_map,
                                                       const double* __restrict__ stamps, double* __restrict__ D, int* flag, int check) {
  const int s = named[blockIdx.y], k = blockIdx.x * LCT_T + threadIdx.x;
  if (k >= seqs[s].n_kf) return;
  const size_t at = (size_t)s * kf_stride + k;
  double O[7], M[7], I[7], o[7];
  for (int i = 0; i < 7; i++) O[i] = T_odom[at * 7 + i], M[i] = T_map[at * 7 + i];
  lct_pose_inv(O, I);
  lct_pose_mul(I, M, o);
  for (int i = 0; i < 7; i++) D[at * 7 + i] = o[i];
  if (check) {
    const double tau = stamps[at];
    // (every thread that finds a fault stores the same word: no order among them matters)
    if (!(tau - tau == 0.0) || (k > 0 && !(stamps[at - 1] < tau))) *flag = 1;
  }
}

// the number of k in [0, n) with tau[k] <= t, tau strictly increasing
__device__ __forceinline__ int lct_upper_bound(const double* tau, int n, double t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tau[mid] <= t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// one tile of a job of rows W doubles wide: in through LDS, one thread per row, out through LDS
template <int W>
__device__ __forceinline__ void lct_tile(const LctJob& j, int n, const double* __restrict__ drift0, int kf_stride, const double* __restrict__ stamps,
                                         const double* __restrict__ D, int mode, double* rows) {
  constexpr int LW = W | 1;  // the LDS row stride in doubles: odd, so that the lanes' 8-byte reads of a column fall on distinct banks
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * LCT_T;
  const int nr = min(LCT_T, j.n - r0);
  const double* const src = j.in + (size_t)r0 * W;  // (out may be in: no __restrict__ on either)
  for (int i = tid; i < nr * W; i += LCT_T) rows[(i / W) * LW + (i % W)] = src[i];
  __syncthreads();
  const bool live = tid < nr;
  double* const row = rows + tid * LW;
  const double t = live ? row[0] : 0.0;
  const bool has = live && t == t;  // (a NaN stamp: the row is copied as it is, anchor -2)
  const double* const tau = stamps + (size_t)j.seq * kf_stride;
  const double* const Ds = D + (size_t)j.seq * kf_stride * 7;
  int a = n > 0 ? -2 : -1;
  if (!live) a = 0;
  else if (!has) a = -2;
  if (has) {
    double Dr[7];
    if (n == 0) {
      for (int i = 0; i < 7; i++) Dr[i] = drift0[i];
    } else {
      const int ub = lct_upper_bound(tau, n, t);
      a = max(ub - 1, 0);
      const double* const Da = Ds + (size_t)a * 7;
      if (mode == FLVIS_LC_TRAJ_BLEND && ub > 0 && a < n - 1) {
        const double* const Db = Da + 7;
        const double ta = tau[a], tb = tau[a + 1];
        const double u = (t - ta) / (tb - ta);
        const double w0 = 1.0 - u;
        for (int i = 0; i < 3; i++) Dr[i] = w0 * Da[i] + u * Db[i];
        const double dot = Da[3] * Db[3] + Da[4] * Db[4] + Da[5] * Db[5] + Da[6] * Db[6];
        const double us = u * (dot < 0 ? -1.0 : 1.0);
        double b[4];
        for (int i = 0; i < 4; i++) b[i] = w0 * Da[3 + i] + us * Db[3 + i];
        const double nn = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
        for (int i = 0; i < 4; i++) Dr[3 + i] = b[i] / nn;
      } else {
        for (int i = 0; i < 7; i++) Dr[i] = Da[i];
      }
    }
    if (W == 11) {  // (t, qw qx qy qz, p, v): the body pose in the world frame
      double E[7], P[7], v[3];
      lct_pose_inv(Dr, E);
      const double B[7] = {row[5], row[6], row[7], row[2], row[3], row[4], row[1]};
      lct_pose_mul(E, B, P);
      lct_q_rot(E + 3, row + 8, v);
      row[1] = P[6], row[2] = P[3], row[3] = P[4], row[4] = P[5];
      row[5] = P[0], row[6] = P[1], row[7] = P[2];
      row[8] = v[0], row[9] = v[1], row[10] = v[2];
    } else {  // (t, T_c_w7[, state]): the camera pose
      double P[7];
      lct_pose_mul(row + 1, Dr, P);
      for (int i = 0; i < 7; i++) row[1 + i] = P[i];
    }
  }
  __syncthreads();
  double* const dst = j.out + (size_t)r0 * W;
  for (int i = tid; i < nr * W; i += LCT_T) dst[i] = rows[(i / W) * LW + (i % W)];
  if (live && j.anchor) j.anchor[r0 + tid] = a;
}

__global__ __launch_bounds__(LCT_T) void k_lc_map_poses(const LctJob* __restrict__ jobs, const LctSeq* __restrict__ seqs, int kf_stride,
                                                        const double* __restrict__ stamps, const double* __restrict__ D,
                                                        const int* __restrict__ flag, int mode) {
  extern __shared__ double rows[];  // [LCT_T][widest row of the call | 1]
  if (*flag) return;  // a sequence's stamps are refused: nothing is written
  const LctJob j = jobs[blockIdx.y];
  if (blockIdx.x * LCT_T >= j.n) return;
  const int n = seqs[j.seq].n_kf;
  const double* const q = seqs[j.seq].drift;
  if (j.kind == FLVIS_LC_ROWS_POSE8) lct_tile<8>(j, n, q, kf_stride, stamps, D, mode, rows);
  else if (j.kind == FLVIS_LC_ROWS_TRAJ9) lct_tile<9>(j, n, q, kf_stride, stamps, D, mode, rows);
  else lct_tile<11>(j, n, q, kf_stride, stamps, D, mode, rows);
}

}  // namespace

namespace flvis {

int lc_map_poses_check(flvis_ctx* ctx, const char* what, int n_seq, int kf_stride, const int* h_nkf, int n_jobs, const flvis_lc_traj_job* h_jobs,
                       int mode) {
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": " + m); };
  if (mode != FLVIS_LC_TRAJ_ANCHOR && mode != FLVIS_LC_TRAJ_BLEND) return bad("no such mode");
  if (n_seq <= 0 || kf_stride < 0 || n_jobs < 0 || !h_nkf || (n_jobs > 0 && !h_jobs)) return bad("bad args");
  if (n_jobs > 65535) return ctx->fail(FLVIS_ERR_CAPACITY, std::string(what) + ": more than 65535 jobs in one call");
  for (int s = 0; s < n_seq; s++)
    if (h_nkf[s] < 0 || h_nkf[s] > kf_stride) return bad("a sequence's keyframe count is outside [0, kf_stride]");
  for (int i = 0; i < n_jobs; i++) {
    const flvis_lc_traj_job& j = h_jobs[i];
    const std::string at = "job " + std::to_string(i) + ": ";
    if (j.seq < 0 || j.seq >= n_seq) return bad(at + "sequence out of range");
    if (!lct_row_width(j.kind)) return bad(at + "no such row kind");
    if (j.n < 0) return bad(at + "negative row count");
    if (j.n > 0 && (!j.d_in || !j.d_out)) return bad(at + "NULL rows");
  }
  return FLVIS_OK;
}

int lc_map_poses_dev(flvis_ctx* ctx, const char* what, int n_seq, int kf_stride, const int* h_nkf, const double* d_T_odom, const double* d_T_map,
                     const double* d_stamps, const double* h_drift7, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode, bool check_stamps) {
  int rc = lc_map_poses_check(ctx, what, n_seq, kf_stride, h_nkf, n_jobs, h_jobs, mode);
  if (rc != FLVIS_OK) return rc;
  // the jobs with rows, the sequences they name, the largest of each
  std::vector<LctJob> jobs;
  std::vector<int> named;
  std::vector<char> is_named((size_t)n_seq, 0);
  int max_rows = 0, max_kf = 0, max_w = 0;
  bool any_empty = false;
  for (int i = 0; i < n_jobs; i++) {
    const flvis_lc_traj_job& j = h_jobs[i];
    if (j.n == 0) continue;
    jobs.push_back(LctJob{j.d_in, j.d_out, j.d_anchor, j.seq, j.kind, j.n, 0});
    max_rows = std::max(max_rows, j.n);
    max_w = std::max(max_w, lct_row_width(j.kind));
    if (is_named[j.seq]) continue;
    is_named[j.seq] = 1;
    if (h_nkf[j.seq] > 0) named.push_back(j.seq);  // (k_lc_kf_drift has nothing to do for an empty sequence)
    else any_empty = true;
    max_kf = std::max(max_kf, h_nkf[j.seq]);
  }
  if (jobs.empty()) return FLVIS_OK;
  if (max_kf > 0 && (!d_T_odom || !d_T_map || !d_stamps)) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": NULL keyframe table");
  if (any_empty && !h_drift7) return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": NULL h_drift7 with an empty sequence named");
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  // one upload: the flag (8 bytes, so that what follows stays aligned), the sequences, the jobs, the named sequences
  const size_t o_seq = 8, o_job = o_seq + sizeof(LctSeq) * (size_t)n_seq, o_named = o_job + sizeof(LctJob) * jobs.size();
  const size_t bytes = o_named + sizeof(int) * std::max<size_t>(named.size(), 1);
  std::vector<uint8_t> h_tab(bytes, 0);
  LctSeq* const hs = reinterpret_cast<LctSeq*>(h_tab.data() + o_seq);
  for (int s = 0; s < n_seq; s++) {
    hs[s].n_kf = h_nkf[s];
    if (h_drift7) memcpy(hs[s].drift, h_drift7 + 7 * (size_t)s, 56);
    else hs[s].drift[6] = 1.0;
  }
  memcpy(h_tab.data() + o_job, jobs.data(), sizeof(LctJob) * jobs.size());
  if (!named.empty()) memcpy(h_tab.data() + o_named, named.data(), sizeof(int) * named.size());
  uint8_t* const d_tab = (uint8_t*)ctx->scratch("lct_tab", bytes);
  double* const d_D = (double*)ctx->scratch("lct_drift", sizeof(double) * 7 * std::max<size_t>((size_t)n_seq * kf_stride, 1));
  if (!d_tab || !d_D) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  int* const d_flag = reinterpret_cast<int*>(d_tab);
  const LctSeq* const d_seq = reinterpret_cast<const LctSeq*>(d_tab + o_seq);
  hipError_t e = hipMemcpyAsync(d_tab, h_tab.data(), bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && !named.empty()) {
    k_lc_kf_drift<<<dim3((max_kf + LCT_T - 1) / LCT_T, (unsigned)named.size()), LCT_T, 0, st>>>(
        reinterpret_cast<const int*>(d_tab + o_named), d_seq, kf_stride, d_T_odom, d_T_map, d_stamps, d_D, d_flag, check_stamps ? 1 : 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    k_lc_map_poses<<<dim3((max_rows + LCT_T - 1) / LCT_T, (unsigned)jobs.size()), LCT_T, sizeof(double) * LCT_T * (max_w | 1), st>>>(
        reinterpret_cast<const LctJob*>(d_tab + o_job), d_seq, kf_stride, d_stamps, d_D, d_flag, mode);
    e = hipGetLastError();
  }
  int flag = 0;
  if (e == hipSuccess && check_stamps) e = hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);  // (h_tab is in flight until here, also after an error)
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  if (flag)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": the keyframe stamps of a named sequence are not finite and strictly increasing");
  return FLVIS_OK;
}

int lc_traj_tracker_rows(flvis_ctx* ctx, int& S, int& w, int& h, int& cam_type, std::vector<const double*>& d_rows, std::vector<int>& cap) {
  Pipeline* pl = ctx->pipe;
  if (!pl) return FLVIS_ERR_INVALID_ARG;
  hipSetDevice(ctx->device);
  sync_all(ctx);
  S = pl->S, w = pl->cfg.image_width, h = pl->cfg.image_height, cam_type = pl->cfg.cam_type;
  d_rows.assign((size_t)S, nullptr), cap.assign((size_t)S, 0);
  for (int s = 0; s < S; s++) {
    int ls;
    Lane& L = pl->lane_of(s, ls);
    if (!L.pipe.traj) continue;
    d_rows[s] = L.pipe.traj + (size_t)ls * L.pipe.traj_cap * 9;
    cap[s] = L.pipe.traj_cap;
  }
  return FLVIS_OK;
}

}  // namespace flvis

extern "C" int flvis_hip_lc_map_poses(flvis_ctx* ctx, int n_seq, int kf_stride, const int* h_nkf, const double* d_T_odom, const double* d_T_map,
                                      const double* d_stamps, const double* h_drift7, int n_jobs, const flvis_lc_traj_job* h_jobs, int mode) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  return flvis::lc_map_poses_dev(ctx, "lc_map_poses", n_seq, kf_stride, h_nkf, d_T_odom, d_T_map, d_stamps, h_drift7, n_jobs, h_jobs, mode, true);
}
