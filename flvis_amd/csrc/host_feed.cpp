// flvis_amd: flvis_image_feed_host -- a frame's images handed over in host memory (pipeline_host.hpp: Pipeline::HostFeed)
#include <chrono>
#include <thread>

#include "pipeline_host.hpp"

using namespace flvis;

extern "C" {

// TrackingNodeletClass::image_input_callback (src/frontend/vo_tracking.cpp:396-430) hands F2FTracking::image_feed two HOST
// cv::Mat (mono8, or 3/4 channels converted by cvtColor, f2f_tracking.cpp:74-111; depth rigs: img1 = 16UC1 depth): the same
// hand-over with plain structs.  Uploads run on a copy stream into double-buffered device staging.
int flvis_image_feed_host(flvis_ctx* ctx, const flvis_image* h_img0, const flvis_image* h_img1, flvis_frame_out* h_out,
                          int with_local_map, int hold_buffers) {
  return flvis_image_feed_host_present(ctx, h_img0, h_img1, nullptr, h_out, with_local_map, hold_buffers);
}

// h_present (may be NULL: every stream): an absent stream's two flvis_image entries are not looked at and nothing of it is uploaded
int flvis_image_feed_host_present(flvis_ctx* ctx, const flvis_image* h_img0, const flvis_image* h_img1, const uint8_t* h_present,
                                  flvis_frame_out* h_out, int with_local_map, int hold_buffers) {
  if (!ctx || !ctx->pipe || !h_img0 || !h_img1) return FLVIS_ERR_INVALID_ARG;
  Pipeline* pl = ctx->pipe;
  const int S = pl->S, w = pl->cfg.image_width, h = pl->cfg.image_height;
  const bool depth_cam = pl->cfg.cam_type == CAM_DEPTH;
  auto present = [&](int s) { return !h_present || h_present[s] != 0; };
  int first = 0;  // the first stream with a frame: its images set the channel counts every other one must match
  while (first < S && !present(first)) first++;
  const bool any = first < S;
  const int ch0 = any ? h_img0[first].channels : 1, ch1 = any ? h_img1[first].channels : 1;
  if ((ch0 != 1 && ch0 != 3 && ch0 != 4) || (ch1 != 1 && ch1 != 3 && ch1 != 4) || (depth_cam && ch1 != 1))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "image_feed_host: channels must be 1, 3 or 4 (depth image: 1)");
  const size_t bpp[2] = {(size_t)ch0, depth_cam ? (size_t)2 : (size_t)ch1};  // bytes per pixel as handed over
  for (int s = 0; s < S; s++) {
    if (!present(s)) continue;
    const flvis_image* im[2] = {&h_img0[s], &h_img1[s]};
    for (int c = 0; c < 2; c++)
      if (!im[c]->data || im[c]->width != w || im[c]->height != h || im[c]->channels != (c ? ch1 : ch0) ||
          (size_t)im[c]->pitch < (size_t)w * bpp[c])
        return ctx->fail(FLVIS_ERR_INVALID_ARG, "image_feed_host: image size/channels/pitch do not match the configuration");
  }
  hipSetDevice(ctx->device);
  Pipeline::HostFeed& hf = pl->hf;
  if (!hf.strm) {
    bool ok = hipStreamCreateWithFlags(&hf.strm, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < 2 && ok; k++)
      ok = hipEventCreateWithFlags(&hf.ev_done[k], pl->ev_flags) == hipSuccess &&
           hipEventCreateWithFlags(&hf.ev_free[k], pl->ev_flags) == hipSuccess && hipEventCreate(&hf.ev_t0[k]) == hipSuccess &&
           hipEventCreate(&hf.ev_t1[k]) == hipSuccess;
    if (!ok) return ctx->fail(FLVIS_ERR_HIP, "image_feed_host: cannot create the copy stream");
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess)
      return ctx->fail(FLVIS_ERR_HIP, "image_feed_host: cannot map the progress word");
    hf.h_up = (volatile long long*)hp;
    hf.d_up = (long long*)dp;
    *hf.h_up = 0;
    hf.times.assign(S, 0.0);
    if (hf.mode == 2) {
      // (fine-grained device memory: the copy engine writes it past the XCDs' L2 caches, the waiting wave must never see a cached line)
      void* dfp = nullptr;
      bool fok = hipExtMallocWithFlags(&dfp, sizeof(long long) * Pipeline::HostFeed::FLAG_WORDS, hipDeviceMallocFinegrained) == hipSuccess;
      if (fok) {
        hipMemset(dfp, 0, sizeof(long long) * Pipeline::HostFeed::FLAG_WORDS);
        pl->allocs.push_back(dfp);
        hf.d_flag = (long long*)dfp;
      }
      for (int k = 0; k < Pipeline::HostFeed::FLAG_RING && fok; k++) {
        void* fp = nullptr;
        fok = hipHostMalloc(&fp, sizeof(long long) * Pipeline::HostFeed::FLAG_WORDS, hipHostMallocDefault) == hipSuccess;
        hf.h_flag[k] = (long long*)fp;
      }
      if (!fok) return ctx->fail(FLVIS_ERR_HIP, "image_feed_host: cannot allocate the sequence blocks");
    }
  }
  const int n_slots = hf.mode == 2 ? Pipeline::HostFeed::SLOTS : 2;
  const size_t npix = (size_t)S * w * h;
  for (int c = 0; c < 2; c++) {
    const size_t need = npix * bpp[c] + 256;
    if (hf.raw_bytes[c] < need) {
      hipStreamSynchronize(hf.strm);
      hipStreamSynchronize(ctx->stream);
      for (Lane* L : pl->lanes) hipStreamSynchronize(L->det_stream);
      for (int k = 0; k < n_slots; k++)
        if (!(hf.raw[k][c] = dalloc<uint8_t>(pl->allocs, need, false))) return ctx->fail(FLVIS_ERR_HIP, "image_feed_host: device allocation failed");
      hf.raw_bytes[c] = need;
    }
  }
  if ((ch0 > 1 || (ch1 > 1 && !depth_cam)) && hf.gray_bytes < npix + 256) {
    for (int k = 0; k < n_slots; k++)
      for (int c = 0; c < 2; c++)
        if (!(hf.gray[k][c] = dalloc<uint8_t>(pl->allocs, npix + 256, false))) return ctx->fail(FLVIS_ERR_HIP, "image_feed_host: device allocation failed");
    hf.gray_bytes = npix + 256;
  }
  const int slot = (int)(hf.n % n_slots), tslot = (int)(hf.n & 1);
  // hold_buffers contract: the previous call's buffers are free when this call returns -- its uploads must be done.
  // Mode 1: polled on a host-mapped counter a kernel of the copy stream stores after the uploads (hipEventSynchronize on its event also
  // waited for the KERNELS of the previous frame, so uploads and frames never overlapped: measured 2.25 ms per step = upload + frame).
  // Mode 2: hipStreamQuery on the copy stream, which holds nothing but the copies (the host reads the last copy's signal; no packet).
  auto wait_uploads = [&](long long calls) {
    int polls = 0;
    if (hf.mode == 2) {
      while (hipStreamQuery(hf.strm) == hipErrorNotReady) {
        if (++polls > 16) std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
      (void)hipGetLastError();
      return;
    }
    while (*hf.h_up < calls) {
      if ((++polls & 255) == 0 && hipStreamQuery(hf.strm) == hipSuccess && *hf.h_up < calls) break;  // (idle copy stream: a failed copy)
      std::this_thread::sleep_for(std::chrono::microseconds(30));
    }
  };
  const auto th0 = std::chrono::steady_clock::now();
  if (hf.n >= 1) wait_uploads(hf.n);
  const auto th1 = std::chrono::steady_clock::now();
  // the frame that used this slot has been consumed.  (NOT implied by the host lead: the uploads are issued before this call waits for the
  // previous frame to start, i.e. while the frame before that may still be reading the slot -- without this wait the leg's poses differ from
  // the resident run's, bench.py's check caught it in round 5)
  // Mode 1: the copy stream waits for an event recorded behind that frame.  Mode 2: the HOST looks at the lanes' progress words -- the slot
  // was read by lane frame slot_frame[slot]; once a later frame of every lane has started (k_frame_head publishes its number when it
  // starts, behind k_frame_end of its predecessor and the joins in front of that), or the lane's stream has run dry, nothing reads it any
  // more.  With three slots the frame in question lies three calls back: the test is true when it is made.
  if (hf.mode == 2) {
    const long long need = hf.slot_frame[slot] + 1;
    if (hf.slot_frame[slot] > 0)
      for (Lane* L : pl->lanes) {
        int polls = 0;
        while (*L->h_progress < need) {
          if ((++polls & 63) == 0 && hipStreamQuery(L->st) == hipSuccess) break;  // (an idle stream: the frame is over, or its launch failed)
          std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
      }
  } else if (hf.n >= 2) {
    hipStreamWaitEvent(hf.strm, hf.ev_free[slot], 0);
  }
  if (hf.timed[tslot]) {  // the uploads of two calls ago: done (the previous call's are, and the copy stream is in order)
    float ms = 0;
    if (hipEventElapsedTime(&ms, hf.ev_t0[tslot], hf.ev_t1[tslot]) == hipSuccess) hf.up_ms += ms, hf.up_bytes += (double)hf.timed_bytes[tslot], hf.up_calls += 1;
    else (void)hipGetLastError();
    hf.timed[tslot] = false;
  }
  if (hf.timing) hipEventRecord(hf.ev_t0[tslot], hf.strm);
  // (Measured in round 4, profiles/r04_h2d_full_timeline_*.txt: beside an SDMA upload the chain's latency-bound kernels run 2-3 x slower,
  // the LK launches do not.  Gating the uploads under LK launches -- left image under the previous frame's stereo LK, right image under
  // the frame's own head / temporal LK -- made the leg slower, 40k -> 31k frames/s: k_frame_head / k_track_prepare are latency-bound too
  // and the later start of the copies costs host lead.  A copy KERNEL of 8 .. 128 workgroups reading the caller's page-locked buffer over
  // PCIe instead of the SDMA engine: 19-34k frames/s against 35.3k (profiles/r04_lk_ab.md).  The uploads start as soon as their
  // staging slot is free, on the SDMA engine.  Round 6: what slowed the chain was not the copy but the barrier packets that waited for
  // it on the copy stream's hardware queue -- mode 2 has none, profiles/r06_h2d.md.)
  hipError_t e = hipSuccess;
  for (int c = 0; c < 2 && e == hipSuccess; c++) {
    const flvis_image* im = c ? h_img1 : h_img0;
    const size_t row = (size_t)w * bpp[c], img_bytes = row * h;
    bool contiguous = !h_present;  // one block [S][h][w*bpp]: a single copy (every stream's image)
    for (int s = 0; s < S && contiguous; s++)
      contiguous = (size_t)im[s].pitch == row && im[s].data == im[0].data + (size_t)s * img_bytes;
    // (in one piece: chunked uploads were slower, profiles/r05_h2d.md)
    if (contiguous) {
      e = hipMemcpyAsync(hf.raw[slot][c], im[0].data, img_bytes * S, hipMemcpyHostToDevice, hf.strm);
    } else {
      for (int s = 0; s < S && e == hipSuccess; s++)
        if (present(s))
          e = hipMemcpy2DAsync(hf.raw[slot][c] + (size_t)s * img_bytes, row, im[s].data, (size_t)im[s].pitch, row, h,
                               hipMemcpyHostToDevice, hf.strm);
    }
  }
  if (hf.timing && e == hipSuccess) {
    hipEventRecord(hf.ev_t1[tslot], hf.strm);
    hf.timed[tslot] = true;
    hf.timed_bytes[tslot] = (size_t)w * h * S * (bpp[0] + bpp[1]);
  }
  const long long seq = hf.n + 1;
  if (hf.mode == 2) {
    // the sequence block behind the images (page-locked ring of FLAG_RING blocks: the block of call n is rewritten by call n + FLAG_RING,
    // whose predecessors' uploads the host has seen finish)
    long long* fb = hf.h_flag[hf.n % Pipeline::HostFeed::FLAG_RING];
    for (int k = 0; k < Pipeline::HostFeed::FLAG_WORDS; k++) fb[k] = seq;
    if (e == hipSuccess) e = hipMemcpyAsync(hf.d_flag, fb, sizeof(long long) * Pipeline::HostFeed::FLAG_WORDS, hipMemcpyHostToDevice, hf.strm);
    if (e != hipSuccess) return ctx->hip_fail(e, "image_feed_host upload");
  } else {
    if (e == hipSuccess) e = hipEventRecord(hf.ev_done[slot], hf.strm);
    if (e != hipSuccess) return ctx->hip_fail(e, "image_feed_host upload");
    launch_store_progress(hf.strm, hf.d_up, seq);
  }
  hipStream_t st = ctx->stream;
  // Which stream waits for the uploads.  In mode 2 the detection stream, in front of the left image's ingest: every reader of the staged
  // images is ordered behind that stream already -- the left pyramid's join in front of the temporal LK, the right pyramid's in front of
  // the stereo LK, which reads the right image in place.  Only for single-channel stereo input on a single lane past the skipped start-up
  // frames; otherwise, and in mode 1, the main stream waits, in front of the frame (rounds 1-5: always; profiles/r06_h2d.md).
  const bool wait_on_det = hf.mode == 2 && ch0 == 1 && ch1 == 1 && !depth_cam && pl->lanes.size() == 1 &&
                           pl->frames_fed >= (long long)pl->cfg.skip_first_n_imgs;
  if (hf.mode == 2) {
    if (wait_on_det) pl->up_flag = hf.d_flag, pl->up_seq = seq;
    else launch_wait_flag(st, hf.d_flag, Pipeline::HostFeed::FLAG_WORDS, seq, pl->lanes[0]->d_progress + 2);
  } else {
    if (wait_on_det) pl->up_event = hf.ev_done[slot];
    else hipStreamWaitEvent(st, hf.ev_done[slot], 0);
  }
  const uint8_t* d0 = hf.raw[slot][0];
  const uint8_t* d1 = hf.raw[slot][1];
  if (ch0 > 1) {
    launch_bgr_to_gray(st, hf.raw[slot][0], ch0, hf.gray[slot][0], npix);
    d0 = hf.gray[slot][0];
  }
  if (ch1 > 1 && !depth_cam) {
    launch_bgr_to_gray(st, hf.raw[slot][1], ch1, hf.gray[slot][1], npix);
    d1 = hf.gray[slot][1];
  }
  for (int s = 0; s < S; s++) hf.times[s] = present(s) ? h_img0[s].t : 0.0;
  // one frame of lead in this mode: with two, the uploads' copies and events push the queued commands over what the HIP runtime
  // accepts without blocking the caller for milliseconds (measured: 16k vs 28k frames/s when that happened mid-run, profiles/r05_h2d.md)
  pl->host_lead_cap = 1;
  const auto th2 = std::chrono::steady_clock::now();
  pl->chain_continuous = wait_on_det && hf.mode == 2 && hf.last_call_frame == pl->frames_fed;  // (the previous frame was this entry's too)
  const int rc = flvis_image_feed_present(ctx, d0, d1, hf.times.data(), h_present, h_out, with_local_map);
  pl->chain_continuous = false;
  hf.last_call_frame = pl->frames_fed;
  pl->up_event = nullptr;
  pl->up_flag = nullptr;
  const auto th3 = std::chrono::steady_clock::now();
  hf.ms_wait_uploads += std::chrono::duration<double, std::milli>(th1 - th0).count();
  hf.ms_issue += std::chrono::duration<double, std::milli>(th2 - th1).count();
  hf.ms_feed += std::chrono::duration<double, std::milli>(th3 - th2).count();
  pl->host_lead_cap = 4;
  if (hf.mode == 2) hf.slot_frame[slot] = pl->lanes[0]->frames_uploaded;
  else hipEventRecord(hf.ev_free[slot], st);
  hf.n++;
  if (rc != FLVIS_OK) return rc;
  if (!hold_buffers) wait_uploads(hf.n);  // the caller may reuse its buffers at once: wait for the uploads (not for the frame)
  return FLVIS_OK;
}

}  // extern "C"
