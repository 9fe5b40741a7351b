// flvis_amd: the keyframe log (include/flvis_hip.h: flvis_keyframe_log_*).
//
// The tracker publishes a flvis/KeyFrame message per keyframe (/vo_kf, KeyFrameMsg::pub, src/utils/keyframe_msg.cpp:30-124): the two images
// it worked on and the payload k_frame_end appends to the stream's keyframe queue.  flvis_get_keyframe_msg can only return a stream's LAST
// keyframe, and its images only until the next frame overwrites them; inside a flvis_run_steps batch the host sees nothing between the
// steps.  The log keeps the whole message on the device, per stream, for a prefix of the stream's keyframes:
//   k_kf_log_append   behind every k_frame_end of a lane while the log is on, grid (image chunks, streams of the lane): a stream that made
//                     a keyframe in this step gets level 0 of its left pyramid, its right / depth image and the payload copied behind its
//                     record; every other stream's workgroups retire at once
//   k_kf_log_init     empties records (enable, clear, flvis_reset_streams)
//   k_kf_log_gather   entries of several streams -> the contiguous [n][h][w] images the loop closer's feature kernels take
//
// Which slot.  Every workgroup of a stream must agree on the slot, and one of them has to move the count.  The count is therefore kept
// twice (KFL_LOGGED + 0 / + 1, the dropped count likewise): a launch of parity q reads word q and its payload workgroup writes word
// q ^ 1 -- also for a stream without a keyframe, whose counts it carries over -- and the lane's launches alternate in stream order.  No
// workgroup reads a word that another one of the same launch writes, nothing is atomic, and the record is bit-reproducible.
//
// When it runs.  On the lane's tracking stream, directly behind k_frame_end (the kernel that decides new_kf and writes the payload).  What
// it reads of frame k is safe from step k + 1 by the schedule's existing order: the left image of step k + 1 goes to the OTHER slot of the
// left pyramid, and step k + 2's ingest waits for k_frame_end of step k + 1, which is behind this kernel; level 0 of the right pyramid is
// one buffer, rewritten on the detection stream behind a join the tracking stream signals from step k + 1's F-RANSAC; and the caller's
// buffers are released by an event recorded behind the lane's frame (flvis_image_feed_present).  No stream or queue is added.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "kf_log.hpp"
#include "pipeline_host.hpp"

namespace {

using namespace flvis;

constexpr int KFL_T = 256;
constexpr int KFL_ROWS = 16;     // image rows per workgroup of k_kf_log_append
constexpr int KFL_GATHER = 32;   // workgroups per image of k_kf_log_gather
constexpr int KFL_HEAD_WORDS = (int)(offsetof(KeyFrameDev, lm_id) / 8);
static_assert(offsetof(KeyFrameDev, lm_id) % 8 == 0 && sizeof(KeyFrameDev) % 8 == 0, "the payload is copied in 8-byte words");

// rows r0 .. r1 - 1 of an image whose rows are rb bytes: pitched source rows -> tight destination rows.  vec: 16-byte lanes
__device__ __forceinline__ void kfl_copy_rows(const uint8_t* __restrict__ src, int spitch, uint8_t* __restrict__ dst, int rb, int r0, int r1,
                                              int vec) {
  const int t = threadIdx.x;
  if (vec) {
    const int vpr = rb >> 4, nv = (r1 - r0) * vpr;
    for (int i = t; i < nv; i += KFL_T) {
      const int r = i / vpr, c = i - r * vpr;
      const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)(r0 + r) * spitch + 16 * c);
      *reinterpret_cast<uint4*>(dst + (size_t)(r0 + r) * rb + 16 * c) = v;
    }
  } else {  // (KITTI's 1241-byte rows, a caller's buffer at an odd address)
    for (int r = r0; r < r1; r++)
      for (int c = t; c < rb; c += KFL_T) dst[(size_t)r * rb + c] = src[(size_t)r * spitch + c];
  }
}

// grid (2 * chunks, streams): workgroups [0, chunks) copy the left image's rows, [chunks, 2 chunks) the right / depth image's; workgroup 0 of
// a stream also copies the payload and writes the header
__global__ __launch_bounds__(KFL_T) void k_kf_log_append(Pipe p, KfLogRec r, KfLogSrc src, int parity, int chunks) {
  const int s = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  long long* const h = r.hdr + (size_t)s * KFL_HDR;
  const long long n = h[KFL_LOGGED + parity], d = h[KFL_DROPPED + parity];
  // a keyframe of THIS step: the stream had a frame, k_frame_end reported one and its queue entry is the stream's last keyframe (a
  // keyframe that met a full queue has no payload: the back-pressure excludes it, and it is no message either)
  bool kf = false;
  const KeyFrameDev* q = nullptr;
  if (!p.present || p.present[s]) {
    const unsigned e = p.kfq_kf[s];
    if (p.out[s].new_keyframe && e != 0u) {
      q = p.kfq + (size_t)s * KFQ + ((e - 1u) % KFQ);
      kf = q->valid == KFQ_KEYFRAME && q->frame_id == p.out[s].frame_id;
    }
  }
  // the record stays a prefix: after the first keyframe that did not fit nothing more is recorded
  const bool fits = kf && d == 0 && n >= 0 && n < (long long)r.cap;
  if (c == 0 && t == 0) {
    h[KFL_LOGGED + (parity ^ 1)] = n + (fits ? 1 : 0);
    h[KFL_DROPPED + (parity ^ 1)] = d + (kf && !fits ? 1 : 0);
  }
  if (!fits) return;
  const size_t e = (size_t)s * r.cap + (size_t)n;
  if (c < chunks) {
    const int r0 = c * KFL_ROWS, r1 = min(r0 + KFL_ROWS, r.h);
    kfl_copy_rows(src.img0[p.img_slot[s] & 1] + (size_t)s * src.stride0, src.pitch0, r.img0 + e * r.px(), r.w, r0, r1, src.vec0);
  } else {
    const int r0 = (c - chunks) * KFL_ROWS, r1 = min(r0 + KFL_ROWS, r.h);
    kfl_copy_rows(src.img1 + (size_t)s * src.stride1, src.pitch1, r.img1 + e * r.px() * r.bpp1, r.w * r.bpp1, r0, r1, src.vec1);
  }
  if (c != 0) return;
  const int m = min(max(q->lm_count, 0), KF_MAXLM);
  const long long* qs = reinterpret_cast<const long long*>(q);
  long long* o = reinterpret_cast<long long*>(r.kf + e);
  for (int i = t; i < KFL_HEAD_WORDS; i += KFL_T) o[i] = qs[i];
  const int w_id = (int)(offsetof(KeyFrameDev, lm_id) / 8), w_2d = (int)(offsetof(KeyFrameDev, lm_2d) / 8),
            w_3d = (int)(offsetof(KeyFrameDev, lm_3d) / 8);
  for (int i = t; i < m; i += KFL_T) o[w_id + i] = qs[w_id + i];
  for (int i = t; i < 2 * m; i += KFL_T) o[w_2d + i] = qs[w_2d + i];
  for (int i = t; i < 3 * m; i += KFL_T) o[w_3d + i] = qs[w_3d + i];
}

__global__ void k_kf_log_init(KfLogRec r, int first) {
  if (threadIdx.x >= KFL_HDR) return;
  r.hdr[(size_t)(first + blockIdx.x) * KFL_HDR + threadIdx.x] = 0;
}

// grid (2 * KFL_GATHER, n): the two images of entry index[i] of stream stream[i] -> image i of the contiguous outputs
__global__ __launch_bounds__(KFL_T) void k_kf_log_gather(KfLogRec r, const int* __restrict__ stream, const int* __restrict__ index,
                                                         uint8_t* __restrict__ o0, uint8_t* __restrict__ o1, int vec) {
  const int i = blockIdx.y, t = threadIdx.x;
  const int k = index[i];
  if (k < 0 || k >= r.cap) return;
  const size_t e = (size_t)stream[i] * r.cap + (size_t)k;
  const bool second = blockIdx.x >= KFL_GATHER;
  const int c = second ? blockIdx.x - KFL_GATHER : blockIdx.x;
  const size_t bytes = second ? r.px() * r.bpp1 : r.px();
  const uint8_t* src = second ? r.img1 + e * bytes : r.img0 + e * bytes;
  uint8_t* dst = second ? o1 + (size_t)i * bytes : o0 + (size_t)i * bytes;
  const size_t len = ((bytes + KFL_GATHER - 1) / KFL_GATHER + 15) & ~(size_t)15;
  const size_t b0 = min((size_t)c * len, bytes), b1 = min(b0 + len, bytes);
  if (vec) {
    for (size_t j = b0 + 16 * (size_t)t; j < b1; j += 16 * KFL_T)
      *reinterpret_cast<uint4*>(dst + j) = *reinterpret_cast<const uint4*>(src + j);
  } else {
    for (size_t j = b0 + t; j < b1; j += KFL_T) dst[j] = src[j];
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

namespace flvis {

void launch_kf_log_append(hipStream_t st, const Pipe& p, const KfLogRec& r, const KfLogSrc& src, int parity) {
  const int chunks = (r.h + KFL_ROWS - 1) / KFL_ROWS;
  hipLaunchKernelGGL(k_kf_log_append, dim3(2 * chunks, p.S), dim3(KFL_T), 0, st, p, r, src, parity, chunks);
}
void launch_kf_log_init(hipStream_t st, const KfLogRec& r, int first, int n) {
  if (n > 0) hipLaunchKernelGGL(k_kf_log_init, dim3(n), dim3(64), 0, st, r, first);
}
void launch_kf_log_gather(hipStream_t st, const KfLogRec& r, int n, const int* d_stream, const int* d_index, uint8_t* d_img0, uint8_t* d_img1) {
  const int vec = (r.px() & 15) == 0 && aligned16(r.img0) && aligned16(r.img1) && aligned16(d_img0) && aligned16(d_img1);
  if (n > 0) hipLaunchKernelGGL(k_kf_log_gather, dim3(2 * KFL_GATHER, n), dim3(KFL_T), 0, st, r, d_stream, d_index, d_img0, d_img1, vec);
}

// the lane's part of the log
KfLogRec lane_kfl(const Pipeline* pl, const Lane* L) {
  KfLogRec r = pl->kfl;
  const size_t e = (size_t)L->s0 * r.cap;
  r.hdr += (size_t)L->s0 * KFL_HDR;
  r.img0 += e * r.px();
  r.img1 += e * r.px() * r.bpp1;
  r.kf += e;
  return r;
}

// k_kf_log_append for the lane's frame, on `st` behind its k_frame_end.  in1: the caller's right / depth image of the lane's first stream,
// read in place when `in_place` (depth rigs; stereo rigs whose right image needs no copy), else level 0 of the right pyramid
void kf_log_frame(Pipeline* pl, Lane* L, hipStream_t st, const uint8_t* in1, bool in_place) {
  const KfLogRec r = lane_kfl(pl, L);
  KfLogSrc s{};
  s.img0[0] = L->pyr0[0][0], s.img0[1] = L->pyr0[1][0];
  s.pitch0 = pl->lpitch[0], s.stride0 = pl->lstride[0];
  const bool dst0 = (r.w & 15) == 0 && aligned16(r.img0), dst1 = ((r.w * r.bpp1) & 15) == 0 && aligned16(r.img1);
  s.vec0 = dst0 && aligned16(s.img0[0]) && aligned16(s.img0[1]) && (s.pitch0 & 15) == 0 && (s.stride0 & 15) == 0;
  if (in_place) s.img1 = in1, s.pitch1 = r.w * r.bpp1, s.stride1 = r.px() * r.bpp1;
  else s.img1 = L->pyr1[0], s.pitch1 = pl->lpitch[0], s.stride1 = pl->lstride[0];
  s.vec1 = dst1 && aligned16(s.img1) && (s.pitch1 & 15) == 0 && (s.stride1 & 15) == 0;
  launch_kf_log_append(st, L->pipe, r, s, (int)(L->kfl_seq & 1));
  L->kfl_seq++;
}

void kf_log_reset_stream(Pipeline* pl, Lane* L, int ls) { launch_kf_log_init(L->st, lane_kfl(pl, L), ls, 1); }

void kf_log_free(Pipeline* pl) {
  if (pl->kfl.hdr) hipFree(pl->kfl.hdr);
  if (pl->kfl.img0) hipFree(pl->kfl.img0);
  if (pl->kfl.img1) hipFree(pl->kfl.img1);
  if (pl->kfl.kf) hipFree(pl->kfl.kf);
  pl->kfl = KfLogRec{};
}

int kf_log_settle(flvis_ctx* ctx, const char* what, KfLogRec& rec, int& S, int& cam_type, std::vector<long long>& logged,
                  std::vector<long long>& dropped) {
  Pipeline* pl = ctx->pipe;
  if (!pl || pl->kfl.cap <= 0) return FLVIS_ERR_INVALID_ARG;
  hipSetDevice(ctx->device);
  sync_all(ctx);
  rec = pl->kfl;
  S = pl->S;
  cam_type = pl->cfg.cam_type;
  std::vector<long long> hdr((size_t)S * KFL_HDR);  // the streams' headers in one copy
  const hipError_t e = hipMemcpy(hdr.data(), rec.hdr, sizeof(long long) * hdr.size(), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  logged.assign(S, 0), dropped.assign(S, 0);
  for (const Lane* L : pl->lanes)
    for (int i = 0; i < L->S; i++) {
      const long long* h = &hdr[(size_t)(L->s0 + i) * KFL_HDR];
      const int q = (int)(L->kfl_seq & 1);  // (the word the lane's next launch would read)
      logged[L->s0 + i] = std::min(std::max(h[KFL_LOGGED + q], 0LL), (long long)rec.cap);
      dropped[L->s0 + i] = h[KFL_DROPPED + q];
    }
  return FLVIS_OK;
}

}  // namespace flvis

extern "C" {

int flvis_keyframe_log_enable(flvis_ctx* ctx, int max_keyframes) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (!pl) return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_enable: no tracker (flvis_tracker_create)");
  hipSetDevice(ctx->device);
  sync_all(ctx);  // (no append kernel is in flight when its record goes away)
  kf_log_free(pl);
  if (max_keyframes <= 0) return FLVIS_OK;
  KfLogRec r{};
  r.cap = max_keyframes, r.w = pl->cfg.image_width, r.h = pl->cfg.image_height, r.bpp1 = pl->cfg.cam_type == CAM_DEPTH ? 2 : 1;
  // entry indices are ints and every byte offset a size_t: S * cap entries of px * (1 + bpp1) + payload bytes
  const unsigned long long entries = (unsigned long long)pl->S * (unsigned long long)max_keyframes;
  const unsigned long long per = (unsigned long long)r.px() * (1 + r.bpp1) + sizeof(KeyFrameDev);
  if (entries > (unsigned long long)INT_MAX || entries > (1ull << 62) / per)
    return ctx->fail(FLVIS_ERR_CAPACITY, "keyframe_log_enable: n_streams * max_keyframes entries do not fit the index arithmetic");
  if (hipMalloc((void**)&r.hdr, sizeof(long long) * KFL_HDR * (size_t)pl->S) != hipSuccess ||
      hipMalloc((void**)&r.img0, (size_t)entries * r.px()) != hipSuccess || hipMalloc((void**)&r.img1, (size_t)entries * r.px() * r.bpp1) != hipSuccess ||
      hipMalloc((void**)&r.kf, (size_t)entries * sizeof(KeyFrameDev)) != hipSuccess) {
    (void)hipGetLastError();
    pl->kfl = r;
    kf_log_free(pl);
    return ctx->fail(FLVIS_ERR_HIP, "keyframe_log_enable: device allocation failed");
  }
  pl->kfl = r;
  for (Lane* L : pl->lanes) L->kfl_seq = 0;
  launch_kf_log_init(ctx->stream, r, 0, pl->S);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, "keyframe_log_enable");
  return FLVIS_OK;
}

int flvis_keyframe_log_clear(flvis_ctx* ctx, int n, const int* streams) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  if (!pl || pl->kfl.cap <= 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_clear: no tracker, or its log is off");
  if (n < 0 || (n > 0 && !streams)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_clear: bad stream list");
  for (int i = 0; i < n; i++)
    if (streams[i] < 0 || streams[i] >= pl->S) return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_clear: stream out of range");
  if (n == 0) return FLVIS_OK;
  hipSetDevice(ctx->device);
  sync_all(ctx);
  for (int i = 0; i < n; i++) launch_kf_log_init(ctx->stream, pl->kfl, streams[i], 1);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, "keyframe_log_clear");
  return FLVIS_OK;
}

int flvis_keyframe_log_info(flvis_ctx* ctx, int stream, int64_t* h_info3) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  KfLogRec rec{};
  int S = 0, cam = 0;
  std::vector<long long> logged, dropped;
  if (!h_info3 || !ctx->pipe || ctx->pipe->kfl.cap <= 0 || stream < 0 || stream >= ctx->pipe->S)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_info: no tracker, its log is off, or bad arguments");
  const int rc = kf_log_settle(ctx, "keyframe_log_info", rec, S, cam, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  h_info3[0] = logged[stream], h_info3[1] = dropped[stream], h_info3[2] = rec.cap;
  return FLVIS_OK;
}

int flvis_keyframe_log_get(flvis_ctx* ctx, int stream, int index, int cap, flvis_keyframe* kf, int64_t* h_id, double* h_2d, double* h_3d,
                           uint8_t* h_img0, uint8_t* h_img1) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!kf || cap < 0 || (cap && (!h_id || !h_2d || !h_3d)) || !ctx->pipe || ctx->pipe->kfl.cap <= 0 || stream < 0 || stream >= ctx->pipe->S)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_get: no tracker, its log is off, or bad arguments");
  KfLogRec rec{};
  int S = 0, cam = 0;
  std::vector<long long> logged, dropped;
  const int rc = kf_log_settle(ctx, "keyframe_log_get", rec, S, cam, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  if (index < 0 || index >= logged[stream]) return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_get: no such entry");
  const size_t e = (size_t)stream * rec.cap + (size_t)index;
  std::vector<KeyFrameDev> kfv(1);
  KeyFrameDev& q = kfv[0];
  hipError_t err = hipMemcpy(&q, rec.kf + e, sizeof(KeyFrameDev), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return ctx->hip_fail(err, "keyframe_log_get");
  const int n = std::min(std::max(q.lm_count, 0), KF_MAXLM);
  for (int i = 0; i < n && i < cap; i++) {
    h_id[i] = q.lm_id[i];
    h_2d[2 * i] = q.lm_2d[i][0], h_2d[2 * i + 1] = q.lm_2d[i][1];
    for (int j = 0; j < 3; j++) h_3d[3 * i + j] = q.lm_3d[i][j];
  }
  kf->frame_id = q.frame_id;
  kf->command = 0;  // KFMSG_CMD_NONE
  kf->stamp = q.stamp;
  kf->lm_count = n;
  kf->lm_id = h_id, kf->lm_2d = h_2d, kf->lm_3d = h_3d;
  memcpy(kf->T_c_w, q.T_c_w, 56);
  kf->img0 = flvis_image{h_img0, rec.w, rec.h, rec.w, 1, q.stamp};
  kf->img1 = flvis_image{h_img1, rec.w, rec.h, rec.w * rec.bpp1, 1, q.stamp};
  if (h_img0) err = hipMemcpy(h_img0, rec.img0 + e * rec.px(), rec.px(), hipMemcpyDeviceToHost);
  if (err == hipSuccess && h_img1) err = hipMemcpy(h_img1, rec.img1 + e * rec.px() * rec.bpp1, rec.px() * rec.bpp1, hipMemcpyDeviceToHost);
  if (err != hipSuccess) return ctx->hip_fail(err, "keyframe_log_get");
  return n;
}

int flvis_keyframe_log_images(flvis_ctx* ctx, int stream, int index, const uint8_t** d_img0, const void** d_img1) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!ctx->pipe || ctx->pipe->kfl.cap <= 0 || stream < 0 || stream >= ctx->pipe->S)
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_images: no tracker, its log is off, or bad arguments");
  KfLogRec rec{};
  int S = 0, cam = 0;
  std::vector<long long> logged, dropped;
  const int rc = kf_log_settle(ctx, "keyframe_log_images", rec, S, cam, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  if (index < 0 || index >= logged[stream]) return ctx->fail(FLVIS_ERR_INVALID_ARG, "keyframe_log_images: no such entry");
  const size_t e = (size_t)stream * rec.cap + (size_t)index;
  if (d_img0) *d_img0 = rec.img0 + e * rec.px();
  if (d_img1) *d_img1 = rec.img1 + e * rec.px() * rec.bpp1;
  return FLVIS_OK;
}

}  // extern "C"
