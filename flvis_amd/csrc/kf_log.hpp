// flvis_amd: the keyframe log (flvis_keyframe_log_*, include/flvis_hip.h): the per-stream record of whole KeyFrame messages, its kernels
// and what the loop closer reads of it (flvis_loop_closer_add_logged).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "track_kernels.hpp"

struct flvis_ctx;

namespace flvis {

// Header words of a stream's record.  The counts are kept twice: the append launch of parity q READS [q] and writes [q ^ 1], so the slot
// of a stream's keyframe comes from a word that no workgroup of the same launch changes; the launches of a lane alternate (Lane::kfl_seq),
// and clear / reset / enable write both.
enum { KFL_LOGGED = 0, KFL_DROPPED = 2, KFL_HDR = 4 };

// The record of a tracker's streams (or of one lane's: the pointers then start at the lane's first stream).  cap == 0: off.
struct KfLogRec {
  long long* hdr;    // [S][KFL_HDR]
  uint8_t* img0;     // [S][cap][h * w]
  uint8_t* img1;     // [S][cap][h * w * bpp1]
  KeyFrameDev* kf;   // [S][cap] (the header fields and the first lm_count entries of each array are written)
  int cap, w, h, bpp1;
  __host__ __device__ size_t px() const { return (size_t)w * h; }
};

// where a frame's two images lie when k_kf_log_append runs: level 0 of the left pyramid's two slots (Pipe::img_slot picks one per stream)
// and the right / depth image (level 0 of the right pyramid, or the caller's buffer where it is read in place)
struct KfLogSrc {
  const uint8_t* img0[2];
  int pitch0;
  size_t stride0;
  const uint8_t* img1;
  int pitch1;  // bytes
  size_t stride1;
  int vec0, vec1;  // every row of the image starts 16-byte aligned on both sides and is a whole number of 16-byte lanes
};

// k_kf_log_append behind the lane's k_frame_end (grid: image chunks x streams of `p`); parity: Lane::kfl_seq & 1 of this launch
void launch_kf_log_append(hipStream_t st, const Pipe& p, const KfLogRec& r, const KfLogSrc& src, int parity);
// empties the records of the streams first .. first + n - 1 of `r`
void launch_kf_log_init(hipStream_t st, const KfLogRec& r, int first, int n);
// entry d_index[i] of stream d_stream[i] -> image i of d_img0 [n][h][w] and d_img1 [n][h][w * bpp1] (k_kf_log_gather)
void launch_kf_log_gather(hipStream_t st, const KfLogRec& r, int n, const int* d_stream, const int* d_index, uint8_t* d_img0, uint8_t* d_img1);

// the tracker's log with everything it has queued waited for: the record, the stream count, the tracker's image shape and, per stream,
// the entries logged and the keyframes dropped.  FLVIS_ERR_INVALID_ARG without a tracker or with the log off.
int kf_log_settle(flvis_ctx* ctx, const char* what, KfLogRec& rec, int& S, int& cam_type, std::vector<long long>& logged,
                  std::vector<long long>& dropped);

}  // namespace flvis
