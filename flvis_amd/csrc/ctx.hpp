// flvis_amd: context object behind the C ABI (include/flvis_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>

#include "img_kernels.hpp"

namespace flvis {
struct Pipeline;  // full front-end + local-map state (pipeline.hpp); null for kernel-level-only contexts
}

struct flvis_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;

  struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
  };
  std::map<std::string, Buf> bufs;  // named scratch buffers, grown on demand (never inside a steady-state loop)
  flvis::Pipeline* pipe = nullptr;
  int voc_nodes = 0, voc_words = 0, voc_depth = 0;  // the DBoW3 vocabulary resident in the `voc_*` scratch buffers (flvis_hip_bow_set_vocabulary)
  int64_t mc_stats[4] = {0, 0, 0, 0};  // the last flvis_hip_voxel_cloud call: sort passes run / skipped, workspace bytes, input points
  int dc_timing = 0;                  // flvis_hip_depth_cloud_times: time the stages of the dense calls
  double dc_ms[4] = {0, 0, 0, 0};     // ... the last timed call's count, keys, sort, rows
  double oc_ms[4] = {0, 0, 0, 0};     // the last timed occupancy call's count, emit, sort, reduce (summed over its batches)
  int64_t oc_stats[4] = {0, 0, 0, 0};  // the last occupancy call: records, rays, batches, workspace bytes
  int ocq_lookup = 0;                  // flvis_hip_occupancy_cast_lookup: 0 the line directory, 1 the plain search
  double ocq_ms[2] = {0, 0};           // the last timed occupancy cast's index build (key check, line directory) and walk
  int64_t ocq_stats[4] = {0, 0, 0, 0};  // the last occupancy cast: queries, cells tested, index bytes, workspace bytes
  std::string orb_pattern;  // the BRIEF pattern currently resident in the `orb_pattern` scratch buffer (1024 bytes) or empty

  // returns a device buffer of at least `bytes` bytes (contents undefined after growth)
  void* scratch(const std::string& name, size_t bytes, bool zero_on_alloc = false);
  int fail(int code, const std::string& msg) {
    err = msg;
    return code;
  }
  int hip_fail(hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return -3;
  }
};

static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

namespace flvis {
// the pyramids of the kernel-level LK calls (capi.cpp; flvis_hip_lk_track, flvis_hip_stereo_depth, flvis_hip_lkorb_tracking): the highest level
// cv::calcOpticalFlowPyrLK builds for a w x h image, and levels 1 .. L of `d_img` ([n_img][h][w]) built into the scratch buffer `name`
int lk_pyr_levels(int w, int h, int win, int max_level);
int build_pyramid(flvis_ctx* ctx, const char* name, const uint8_t* d_img, int w, int h, int n_img, int L, PyrSel& pyr);
}  // namespace flvis
