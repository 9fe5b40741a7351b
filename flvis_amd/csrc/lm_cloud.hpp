// flvis_amd: the local map's sparse map cloud (flvis_local_map_cloud*, include/flvis_hip.h): the per-stream record and its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "track_kernels.hpp"

struct flvis_ctx;

namespace flvis {

// header words of a stream's record
enum { LMC_POINTS = 0, LMC_RUNS, LMC_DROPPED, LMC_SEEN_RUNS, LMC_SEEN_FRAME, LMC_SEEN_SKIP, LMC_HDR = 8 };

// The record of a tracker's streams (or of one lane's: the pointers then start at the lane's first stream).  cap == 0: off.
struct LmCloudRec {
  long long* hdr;  // [S][LMC_HDR]
  long long* ids;  // [S][cap]
  double* pts;     // [S][cap][3]
  long long cap;
};

// k_lm_cloud_append behind a k_ba_worker launch of the lane (one workgroup per stream of `p`)
void launch_lm_cloud_append(hipStream_t st, const Pipe& p, const LmCloudRec& r);
// empties the records of the streams first .. first + n - 1 of `p` and takes their windows' counters as seen
void launch_lm_cloud_init(hipStream_t st, const Pipe& p, const LmCloudRec& r, int first, int n);

// pipeline.cpp: the tracker's record and stream count (FLVIS_ERR_INVALID_ARG without a tracker or with the record off), with the
// context's stream ordered behind everything the tracker and the local map have queued and one append pass run on it
int lm_cloud_settle(flvis_ctx* ctx, const char* what, LmCloudRec& rec, int& S);

}  // namespace flvis
