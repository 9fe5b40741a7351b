// flvis_amd: the local map's sparse map cloud (include/flvis_hip.h: flvis_local_map_cloud*).
//
// LocalMapNodeletClass::frame_callback, with output_sparse_map set, appends the optimised position of every multi-view landmark
// (bag->getMultiViewLMs(lms, 4)) to `map` after each window optimisation and publishes it as /map_cloud (vo_localmap.cpp:329-377,
// :454-461).  Here the window optimiser leaves the same ids and fp64 positions in Pipe::corr[s] (CorrectionInf), which the next
// optimisation overwrites; the record keeps them:
//   k_lm_cloud_append   behind every k_ba_worker launch, one workgroup per stream: when the window's run counter has moved and the
//                       correction is valid, the correction's ids and points go behind the stream's record, whole or not at all
//   k_lm_cloud_init     empties records (enable, clear)
// and the fetch turns records into clouds:
//   k_lmc_keys / mc_sort / k_lmc_last   LATEST: a stable sort of the entries by (stream | id) with map_cloud.hip's radix passes; the last
//                       entry of each run of equal ids -- the newest, the sort is stable -- is kept
//   k_lmc_gather        the kept entries of each listed stream in record order, as one row of points under an identity pose
//   mc_voxel_cloud      flvis_hip_voxel_cloud on those rows (map_cloud.hip): rounding, dropping, the voxel rule and the counts are its
//
// When the append kernel runs.  It can only look between two kernels, and the next optimisation of a stream overwrites the correction.
// So while the record is on the host (pipeline.cpp, local_map_work) launches workers that take ONE queue entry per stream, each with an
// append kernel behind it, and orders a lane's local-map launches one behind the other instead of letting its two HIP streams overlap:
// between two optimisations of a stream there is always an append kernel, and no worker runs beside one.  The kernel does not rely on
// that for memory safety: it leaves a window that is owned (Pipe::ba_busy) alone, writes the header "seen" words first and counts last
// and reads them counts first, and a run counter that moved by more than one is counted as dropped runs, never passed over in silence.
// On the paths above neither happens.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "lm_cloud.hpp"
#include "map_cloud.hpp"

namespace {

using namespace flvis;

constexpr int LMC_T = 256;
constexpr long long LMC_NO_FRAME = LLONG_MIN;  // LMC_SEEN_FRAME of a window that has not optimised since it was emptied

__device__ __forceinline__ long long lmc_ld(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lmc_st(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The header of stream s after the event this launch may have to record; n >= 0: the correction's n entries go to `at` first.
struct LmcPlan {
  long long h[6];
  long long at;
  int n, write;
};

// thread 0 of the stream's workgroup: what is there to do?
__device__ void lmc_plan(const Pipe& p, const LmCloudRec& r, int s, LmcPlan& o) {
  const long long* h = r.hdr + (size_t)s * LMC_HDR;
  o.n = -1, o.write = 0, o.at = 0;
  long long points = lmc_ld(h + LMC_POINTS), runs = lmc_ld(h + LMC_RUNS), dropped = lmc_ld(h + LMC_DROPPED);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  long long seen = lmc_ld(h + LMC_SEEN_RUNS), fseen = lmc_ld(h + LMC_SEEN_FRAME);
  const long long skseen = lmc_ld(h + LMC_SEEN_SKIP);
  if (__hip_atomic_load(&p.ba_busy[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // (owned: the host keeps workers and append kernels apart, see above)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  long long skip = (long long)__hip_atomic_load(&p.kfq_skip[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (skip != skseen) {
    // flvis_reset_streams since the header was written (k_stream_reset moved the skip word to its command's entry): the record is the
    // old sequence's.  Until the local map has taken the command -- the head is behind it -- the window may still finish an optimisation
    // of the old sequence: the record stays empty and nothing is recorded.  Then the window is empty and counts from 0.
    const unsigned head = __hip_atomic_load(&p.kfq_head[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool taken = (int)(head - (unsigned)skip) > 0;
    o.write = points != 0 || runs != 0 || dropped != 0 || taken;
    points = runs = dropped = 0;
    if (!taken) {
      o.h[LMC_POINTS] = 0, o.h[LMC_RUNS] = 0, o.h[LMC_DROPPED] = 0, o.h[LMC_SEEN_RUNS] = seen, o.h[LMC_SEEN_FRAME] = fseen,
      o.h[LMC_SEEN_SKIP] = skseen;
      return;
    }
    seen = 0, fseen = LMC_NO_FRAME;
  }
  const long long now = p.win[s].ba_runs;
  const CorrectionDev& c = p.corr[s];
  const int valid = c.valid, n = c.lm_count;
  const long long fid = c.frame_id;
  // window_reset_dev (both resets) zeroes the window, its run counter with it: a counter below the copy, or the copy's value under
  // another frame id, counts from 0 again
  long long delta = now - seen;
  if (now < seen || (now == seen && now > 0 && valid && fid != fseen)) delta = now, o.write = 1;
  if (delta > 0 && valid && n >= 0 && n <= BA_LMAX) {
    o.write = 1;
    // the record stays a prefix: after a dropped run nothing more is recorded.  A counter that moved by more than one has left runs
    // behind that nobody saw: the host launches workers that optimise a stream once, so this is a safeguard, not a path
    if (dropped > 0 || delta > 1 || points < 0 || points + n > r.cap) dropped += delta;
    else o.n = n, o.at = points, points += n, runs += 1;
    seen = now, fseen = fid;
  } else if (now < seen) {
    seen = 0, fseen = LMC_NO_FRAME;
  } else if (delta > 0) {
    o.write = 0;  // (a counter ahead of its correction: wait for the correction)
    return;
  }
  o.h[LMC_POINTS] = points, o.h[LMC_RUNS] = runs, o.h[LMC_DROPPED] = dropped, o.h[LMC_SEEN_RUNS] = seen, o.h[LMC_SEEN_FRAME] = fseen,
  o.h[LMC_SEEN_SKIP] = skip;
}

__global__ __launch_bounds__(LMC_T) void k_lm_cloud_append(Pipe p, LmCloudRec r) {
  __shared__ LmcPlan pl;
  const int s = blockIdx.x, t = threadIdx.x;
  if (t == 0) lmc_plan(p, r, s, pl);
  __syncthreads();
  if (!pl.write) return;
  const int n = pl.n;
  if (n > 0) {
    const CorrectionDev& c = p.corr[s];
    long long* const ids = r.ids + (size_t)s * r.cap + pl.at;
    double* const pts = r.pts + ((size_t)s * r.cap + pl.at) * 3;
    const double* const src = &c.lm_3d[0][0];
    for (int i = t; i < n; i += LMC_T) ids[i] = c.lm_id[i];
    for (int i = t; i < 3 * n; i += LMC_T) pts[i] = src[i];
  }
  __syncthreads();
  if (t != 0) return;
  // a window that was taken while the rows were copied may have rewritten them: leave the header, the taker's launch looks again
  if (n >= 0 && (__hip_atomic_load(&p.ba_busy[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || p.win[s].ba_runs != pl.h[LMC_SEEN_RUNS]))
    return;
  long long* h = r.hdr + (size_t)s * LMC_HDR;
  lmc_st(h + LMC_SEEN_RUNS, pl.h[LMC_SEEN_RUNS]);
  lmc_st(h + LMC_SEEN_FRAME, pl.h[LMC_SEEN_FRAME]);
  lmc_st(h + LMC_SEEN_SKIP, pl.h[LMC_SEEN_SKIP]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the rows and the "seen" words before the counts
  lmc_st(h + LMC_POINTS, pl.h[LMC_POINTS]);
  lmc_st(h + LMC_RUNS, pl.h[LMC_RUNS]);
  lmc_st(h + LMC_DROPPED, pl.h[LMC_DROPPED]);
}

// (nothing else runs on the tracker: the host has waited for it)
__global__ void k_lm_cloud_init(Pipe p, LmCloudRec r, int first) {
  if (threadIdx.x != 0) return;
  const int s = first + blockIdx.x;
  long long* h = r.hdr + (size_t)s * LMC_HDR;
  h[LMC_POINTS] = 0, h[LMC_RUNS] = 0, h[LMC_DROPPED] = 0;
  h[LMC_SEEN_RUNS] = p.win[s].ba_runs;
  h[LMC_SEEN_FRAME] = p.corr[s].valid ? p.corr[s].frame_id : LMC_NO_FRAME;
  h[LMC_SEEN_SKIP] = (long long)p.kfq_skip[s];
  h[6] = 0, h[7] = 0;
}

// ---------------------------------------------------------------------------------------------------------------- the fetch
// the last listed stream e with cstart[e] <= i (an empty one shares its start with the next)
__device__ __forceinline__ int lmc_slot_of(const int* __restrict__ cstart, int n, int i) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cstart[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// one workgroup per listed stream: key = the landmark id, payload = the entry's canonical index, and which values each key byte takes
__global__ __launch_bounds__(LMC_T) void k_lmc_keys(LmCloudRec r, const int* __restrict__ streams, const int* __restrict__ cnt,
                                                    const int* __restrict__ cstart, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                    int* __restrict__ occ) {
  __shared__ uint8_t seen[8 * 256];
  const int t = threadIdx.x, e = blockIdx.x, n = cnt[e];
  if (n == 0) return;
  for (int i = t; i < 8 * 256; i += LMC_T) seen[i] = 0;
  __syncthreads();
  const long long* ids = r.ids + (size_t)streams[e] * r.cap;
  const size_t base = (size_t)cstart[e];
  for (int i = t; i < n; i += LMC_T) {
    const uint64_t key = (uint64_t)ids[i];
    keys[base + i] = key;
    idx[base + i] = (uint32_t)(base + i);
#pragma unroll
    for (int d = 0; d < 8; d++) seen[d * 256 + (int)((key >> (8 * d)) & 255)] = 1;
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < 8; d++)
    if (seen[d * 256 + t]) occ[d * 256 + t] = 1;
}

// sorted position j holds the newest entry of its id iff the next position belongs to another stream or another id
__global__ __launch_bounds__(LMC_T) void k_lmc_last(const uint64_t* __restrict__ K, const uint32_t* __restrict__ I, const int* __restrict__ cstart,
                                                    int n_slots, int N, uint8_t* __restrict__ keep) {
  const int j = blockIdx.x * LMC_T + threadIdx.x;
  if (j >= N) return;
  const int e = lmc_slot_of(cstart, n_slots, j);
  keep[I[j]] = (j + 1 == cstart[e + 1] || K[j + 1] != K[j]) ? 1 : 0;
}

// one workgroup per listed stream: its kept entries in record order -> row e of p3 / id (K entries per row), count and identity pose
__global__ __launch_bounds__(LMC_T) void k_lmc_gather(LmCloudRec r, const int* __restrict__ streams, const int* __restrict__ cnt,
                                                      const int* __restrict__ cstart, const uint8_t* __restrict__ keep, int K,
                                                      double* __restrict__ p3, long long* __restrict__ id, double* __restrict__ T7,
                                                      int* __restrict__ kept) {
  __shared__ int wsum[LMC_T / 64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63, e = blockIdx.x, n = cnt[e];
  const size_t src = (size_t)streams[e] * r.cap, base = (size_t)cstart[e], dst = (size_t)e * K;
  int done = 0;
  for (int i0 = 0; i0 < n; i0 += LMC_T) {
    const int i = i0 + t;
    const bool f = i < n && (!keep || keep[base + i]);
    const unsigned long long bal = __ballot(f);
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = done + __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int k = 0; k < LMC_T / 64; k++) {
      off += k < w ? wsum[k] : 0;
      total += wsum[k];
    }
    if (f && off < K) {
      id[dst + off] = r.ids[src + i];
      const double* q = r.pts + (src + i) * 3;
      double* o = p3 + (dst + off) * 3;
      o[0] = q[0], o[1] = q[1], o[2] = q[2];
    }
    __syncthreads();
    done += total;
  }
  if (t < 7) T7[7 * (size_t)e + t] = t == 6 ? 1.0 : 0.0;
  if (t == 0) kept[e] = min(done, K);
}

int lmc_fetch(flvis_ctx* ctx, const char* what, int n, const int* h_stream, int mode, double leaf, int min_points, int out_cap, float* d_xyz,
              int* d_npts, bool want_ids, int64_t* d_id, int64_t* h_n_out, int64_t* h_n_dropped, bool check_only = false) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  const std::string w = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, w + m); };
  LmCloudRec rec{};
  int S = 0;
  int rc = lm_cloud_settle(ctx, nullptr, rec, S);  // (the checks alone)
  if (rc != FLVIS_OK) return bad("no tracker, or its record is off (flvis_local_map_cloud_enable)");
  if (n <= 0 || !h_stream || !h_n_out) return bad("bad stream list or a NULL h_n_out");
  if (mode != FLVIS_LM_CLOUD_ALL && mode != FLVIS_LM_CLOUD_LATEST) return bad("unknown mode");
  if (!(leaf >= 0) || !std::isfinite(leaf)) return bad("leaf must be finite and >= 0");
  if (min_points < 1) return bad("min_points < 1");
  if (out_cap < 0) return bad("out_cap < 0");
  if (!d_xyz && out_cap > 0) return bad("NULL rows with out_cap > 0");
  if (want_ids && leaf > 0) return bad("ids go with leaf == 0 only");
  {
    std::vector<char> listed((size_t)S, 0);
    for (int e = 0; e < n; e++) {
      if (h_stream[e] < 0 || h_stream[e] >= S) return bad("stream out of range");
      if (listed[h_stream[e]]) return bad("stream " + std::to_string(h_stream[e]) + " is listed twice");
      listed[h_stream[e]] = 1;
    }
  }
  if (check_only) return FLVIS_OK;
  for (int e = 0; e < n; e++) h_n_out[e] = 0;
  if (h_n_dropped)
    for (int e = 0; e < n; e++) h_n_dropped[e] = 0;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  rc = lm_cloud_settle(ctx, what, rec, S);
  if (rc != FLVIS_OK) return rc;
  // ---- the listed records' sizes
  std::vector<long long> hdr((size_t)S * LMC_HDR);
  hipError_t e = hipMemcpyAsync(hdr.data(), rec.hdr, sizeof(long long) * hdr.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  std::vector<int> tab(3 * (size_t)n + 1);  // streams | counts | first canonical indices
  std::vector<long long> cs((size_t)n + 1);
  long long N64 = 0;
  int K = 0;
  for (int i = 0; i < n; i++) {
    const long long c = std::min(std::max(hdr[(size_t)h_stream[i] * LMC_HDR + LMC_POINTS], 0LL), rec.cap);
    cs[i] = N64;
    N64 += c;
    if (N64 > INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, w + "2^31 recorded points or more in one call");
    tab[i] = h_stream[i], tab[n + i] = (int)c, tab[2 * (size_t)n + i] = (int)cs[i];
    K = std::max(K, (int)c);
  }
  cs[n] = N64;
  tab[3 * (size_t)n] = (int)N64;
  const int N = (int)N64;
  if (N == 0) return FLVIS_OK;
  auto no_mem = [&]() {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, w + "device allocation failed");
  };
  int* const d_tab = (int*)ctx->scratch("lmc_list", sizeof(int) * tab.size());
  auto fail_sync = [&](int code) {  // (`tab` goes away on return)
    hipStreamSynchronize(st);
    return code;
  };
  // rows: points [n][K][3] | ids [n][K] | poses [n][7] | kept counts [n]
  const size_t nk = (size_t)n * (size_t)K;
  uint8_t* const rb = (uint8_t*)ctx->scratch("lmc_rows", 8 * (4 * nk + 7 * (size_t)n) + 4 * (size_t)n);
  if (!d_tab || !rb) return no_mem();
  double* const d_p3 = (double*)rb;
  long long* const d_ids = (long long*)(d_p3 + 3 * nk);
  double* const d_T7 = (double*)(d_ids + nk);
  int* const d_kept = (int*)(d_T7 + 7 * (size_t)n);
  e = hipMemcpyAsync(d_tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
  const int *d_streams = d_tab, *d_cnt = d_tab + n, *d_cstart = d_tab + 2 * (size_t)n;
  const uint8_t* d_keep = nullptr;
  if (mode == FLVIS_LM_CLOUD_LATEST) {
    // keys [2][N] | indices [2][N] | byte values [8][256] + the passes' tables | keep [N]
    const size_t tab_ints = 8 * 256 + mc_sort_table_ints(N);
    uint8_t* const sb = (uint8_t*)ctx->scratch("lmc_sort", (size_t)N * (2 * 8 + 2 * 4 + 1) + 4 * tab_ints);
    if (!sb) return fail_sync(no_mem());
    uint64_t* keys[2] = {(uint64_t*)sb, (uint64_t*)sb + N};
    uint32_t* idx[2] = {(uint32_t*)(keys[1] + N), (uint32_t*)(keys[1] + N) + N};
    int* const d_occ = (int*)(idx[1] + N);
    uint8_t* const keep = (uint8_t*)(d_occ + tab_ints);
    e = hipMemsetAsync(d_occ, 0, sizeof(int) * 8 * 256, st);
    if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
    k_lmc_keys<<<n, LMC_T, 0, st>>>(rec, d_streams, d_cnt, d_cstart, keys[0], idx[0], d_occ);
    int occ[8 * 256];
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(occ, d_occ, sizeof(occ), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
    int cur = 0;
    rc = mc_sort(ctx, occ, keys, idx, N, n, d_cstart, cs.data(), (uint32_t*)(d_occ + 8 * 256), &cur, nullptr, nullptr);
    if (rc != FLVIS_OK) return fail_sync(rc);
    k_lmc_last<<<(N + LMC_T - 1) / LMC_T, LMC_T, 0, st>>>(keys[cur], idx[cur], d_cstart, n, N, keep);
    d_keep = keep;
  }
  k_lmc_gather<<<n, LMC_T, 0, st>>>(rec, d_streams, d_cnt, d_cstart, d_keep, K, d_p3, d_ids, d_T7, d_kept);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
  std::vector<int> ptr((size_t)n + 1), range2(2 * (size_t)n);
  for (int i = 0; i <= n; i++) ptr[i] = i;
  for (int i = 0; i < n; i++) range2[2 * i] = i, range2[2 * i + 1] = 1;
  rc = mc_voxel_cloud(ctx, d_p3, d_kept, d_T7, n, K, n, ptr.data(), range2.data(), leaf, min_points, out_cap, d_xyz, d_npts,
                      d_id ? d_ids : nullptr, (long long*)d_id, h_n_out, h_n_dropped);
  return rc == FLVIS_OK ? rc : fail_sync(rc);
}

}  // namespace

namespace flvis {

void launch_lm_cloud_append(hipStream_t st, const Pipe& p, const LmCloudRec& r) {
  hipLaunchKernelGGL(k_lm_cloud_append, dim3(p.S), dim3(LMC_T), 0, st, p, r);
}
void launch_lm_cloud_init(hipStream_t st, const Pipe& p, const LmCloudRec& r, int first, int n) {
  if (n > 0) hipLaunchKernelGGL(k_lm_cloud_init, dim3(n), dim3(64), 0, st, p, r, first);
}

}  // namespace flvis

extern "C" {

int flvis_local_map_cloud(flvis_ctx* ctx, int n, const int* h_stream, int mode, double leaf, int min_points, int out_cap, float* d_xyz,
                          int* d_npts, int64_t* d_id, int64_t* h_n_out, int64_t* h_n_dropped) {
  return lmc_fetch(ctx, "local_map_cloud", n, h_stream, mode, leaf, min_points, out_cap, d_xyz, d_npts, d_id != nullptr, d_id, h_n_out,
                   h_n_dropped);
}

int flvis_local_map_cloud_host(flvis_ctx* ctx, int n, const int* h_stream, int mode, double leaf, int min_points, int out_cap, float* h_xyz,
                               int* h_npts, int64_t* h_id, int64_t* h_n_out, int64_t* h_n_dropped) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  const char* what = "local_map_cloud_host";
  // every refusal before anything is allocated (the rows stand in for the device form's: h_xyz must be there when out_cap > 0)
  int rc = lmc_fetch(ctx, what, n, h_stream, mode, leaf, min_points, out_cap, (float*)h_xyz, nullptr, h_id != nullptr, nullptr, h_n_out,
                     h_n_dropped, /*check_only=*/true);
  if (rc != FLVIS_OK) return rc;
  float* d_xyz = nullptr;
  int* d_npts = nullptr;
  int64_t* d_id = nullptr;
  const size_t rows = (size_t)n * (size_t)out_cap;
  if (rows > 0) {  // ids, rows and counts of every listed stream in one staging buffer of the context
    d_id = (int64_t*)ctx->scratch("lmc_host_rows", rows * (sizeof(int64_t) + 3 * sizeof(float) + sizeof(int)));
    if (!d_id) {
      (void)hipGetLastError();
      return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
    }
    d_xyz = (float*)(d_id + rows);
    d_npts = (int*)(d_xyz + 3 * rows);
  }
  rc = lmc_fetch(ctx, what, n, h_stream, mode, leaf, min_points, out_cap, d_xyz, h_npts ? d_npts : nullptr, h_id != nullptr,
                 h_id ? d_id : nullptr, h_n_out, h_n_dropped);
  if (rc != FLVIS_OK) return rc;
  hipError_t e = hipSuccess;
  bool any = false;
  for (int g = 0; g < n && e == hipSuccess; g++) {
    const size_t k = (size_t)std::min<int64_t>(h_n_out[g], out_cap), at = (size_t)g * (size_t)out_cap;
    if (k == 0) continue;
    any = true;
    e = hipMemcpyAsync(h_xyz + 3 * at, d_xyz + 3 * at, sizeof(float) * 3 * k, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && h_npts) e = hipMemcpyAsync(h_npts + at, d_npts + at, sizeof(int) * k, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && h_id) e = hipMemcpyAsync(h_id + at, d_id + at, sizeof(int64_t) * k, hipMemcpyDeviceToHost, ctx->stream);
  }
  if (any || e != hipSuccess) {
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}
}
