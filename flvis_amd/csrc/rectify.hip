// flvis_amd: a raw, distorted image batch into rectified images (flvis_hip_rectify; include/flvis_hip.h has the definition).
//
// The reference never remaps an image: it undistorts POINTS (cv::undistortPoints with R0 / P0).  The dense matcher needs whole rectified
// images, so this is the project's own definition -- the inverse map of cv::initUndistortRectifyMap in fp64, its result rounded ONCE to
// 1/32 px, then an integer bilinear blend -- and is defined bit for bit.
//
// One kernel, k_rectify, and no map table in HBM.  A workgroup of 32 x 8 threads owns 128 columns x 8 rows of the output; a thread owns four
// adjacent pixels of a row.  It evaluates the map of its camera once per pixel (fp64: four divisions, about sixty operations), keeps the
// source offset and the two 5-bit weights of each pixel in registers, and then walks the RUN of images that share the camera: per image
// four gathered reads per pixel (a tap of weight 0 is not read, so no read leaves the image), one blend, one store.  The host groups a
// call's images into runs of equal camera and cuts long runs so that the launch fills the chip; blockIdx.z is the run.
// Stores: a thread's four bytes leave as one dword where their address is 4-byte aligned (rows of a width that is a multiple of 4 on an
// aligned array: always; odd widths: the rows that happen to be aligned) and as bytes otherwise and at the row's tail.  A wave covers two
// rows of 128 contiguous bytes.  Reads: the neighbourhood of a tile's sources is a tile of about the same shape, shifted by the lens.
// No atomic, no LDS, no scratch; exactly one writer per output byte, so a second run and any batching give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "rectify.hpp"

namespace {

constexpr int RC_TX = 32, RC_TY = 8;  // threads of a workgroup: columns of four pixels x rows
constexpr int RC_PX = 4;              // adjacent pixels of a thread
constexpr int RC_MIN_RUN = 8;         // a run is cut no shorter than this: the map is then under a fifth of a thread's work
constexpr int RC_BLOCKS = 2048;       // workgroups that fill the chip (256 CUs x 8)

struct RcArgs {
  const uint8_t* src;   // [..][h][w]
  uint8_t *dst, *cov;   // [items][h][w]; cov may be NULL
  const double* cam21;  // [n_cam][21] on the device
  const int* run3;      // [runs][3]: first item, items, camera
  const int* src_of;    // item i reads image src_of[i] (NULL: image i)
  int w, h, run0;       // blockIdx.z counts runs from run0
};

// the map of output pixel (u, v) under camera c: the source offset sy * w + sx and ax | ay << 8, or -1 where the pixel is uncovered
__device__ __forceinline__ int rc_map(const double* __restrict__ c, int u, int v, int w, int h, long long& at) {
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3], k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7];
  const double* R = c + 8;
  const double fxn = c[17], fyn = c[18], cxn = c[19], cyn = c[20];
  const double x = ((double)u - cxn) / fxn, y = ((double)v - cyn) / fyn;
  const double X = R[0] * x + R[3] * y + R[6], Y = R[1] * x + R[4] * y + R[7], W = R[2] * x + R[5] * y + R[8];
  const double xp = X / W, yp = Y / W;
  const double r2 = xp * xp + yp * yp, rad = 1 + k1 * r2 + k2 * r2 * r2;
  const double xd = xp * rad + 2 * p1 * xp * yp + p2 * (r2 + 2 * xp * xp), yd = yp * rad + p1 * (r2 + 2 * yp * yp) + 2 * p2 * xp * yp;
  const double mx = fx * xd + cx, my = fy * yd + cy;
  const double tx = mx * 32, ty = my * 32;
  at = 0;
  if (!(fabs(tx) < 1073741824.0) || !(fabs(ty) < 1073741824.0)) return -1;  // (a NaN compares false)
  const int ix = (int)rint(tx), iy = (int)rint(ty);
  const int sx = ix >> 5, ax = ix & 31, sy = iy >> 5, ay = iy & 31;
  if (sx < 0 || sy < 0 || sx + (ax > 0 ? 1 : 0) > w - 1 || sy + (ay > 0 ? 1 : 0) > h - 1) return -1;
  at = (long long)sy * w + sx;
  return ax | (ay << 8);
}

// n <= 4 bytes of `v` (the lowest first) to p: one dword where it is whole and aligned
__device__ __forceinline__ void rc_store(uint8_t* p, uint32_t v, int n) {
  if (n == RC_PX && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(p) = v;
  } else {
    for (int j = 0; j < n; j++) p[j] = (uint8_t)(v >> (8 * j));
  }
}

__global__ __launch_bounds__(RC_TX* RC_TY) void k_rectify(RcArgs a) {
  const int w = a.w, h = a.h;
  const int u0 = ((int)blockIdx.x * RC_TX + (int)threadIdx.x) * RC_PX, v = (int)blockIdx.y * RC_TY + (int)threadIdx.y;
  if (u0 >= w || v >= h) return;
  const int* run = a.run3 + 3 * (size_t)(a.run0 + (int)blockIdx.z);
  const int first = run[0], count = run[1];
  const double* cam = a.cam21 + 21 * (size_t)run[2];
  const int n = min(RC_PX, w - u0);
  long long at[RC_PX];
  int axy[RC_PX];
  uint32_t covered = 0;
#pragma unroll
  for (int j = 0; j < RC_PX; j++) {
    axy[j] = -1, at[j] = 0;
    if (j < n) axy[j] = rc_map(cam, u0 + j, v, w, h, at[j]);
    if (axy[j] >= 0) covered |= 1u << (8 * j);
  }
  const size_t px = (size_t)w * h, row = (size_t)v * w + u0;
  for (int k = 0; k < count; k++) {
    const int item = first + k;
    const uint8_t* I = a.src + (size_t)(a.src_of ? a.src_of[item] : item) * px;
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < RC_PX; j++) {
      if (axy[j] < 0) continue;
      const int ax = axy[j] & 31, ay = axy[j] >> 8;
      const uint8_t* p = I + at[j];
      const int i00 = p[0], i01 = ax ? p[1] : 0, i10 = ay ? p[w] : 0, i11 = (ax && ay) ? p[w + 1] : 0;
      const int val = ((32 - ax) * (32 - ay) * i00 + ax * (32 - ay) * i01 + (32 - ax) * ay * i10 + ax * ay * i11 + 512) >> 10;
      out |= (uint32_t)val << (8 * j);
    }
    rc_store(a.dst + (size_t)item * px + row, out, n);
    if (a.cov) rc_store(a.cov + (size_t)item * px + row, covered, n);
  }
}

// do [a, a + na) and [b, b + nb) share a byte?
bool rc_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

int rc_check_ptrs(const uint8_t* d_src, int n_img, int w, int h, const double* h_cam21, const uint8_t* d_dst, const uint8_t* d_covered,
                  std::string* why) {
  std::string m;
  if (w <= 0 || h <= 0 || n_img <= 0)
    m = "the image shape and count must be positive";
  else if (!d_src || !d_dst || !h_cam21)
    m = "a NULL d_src, d_dst or h_cam21";
  else {
    const size_t bytes = (size_t)n_img * w * h;
    if (rc_overlap(d_src, bytes, d_dst, bytes) || (d_covered && rc_overlap(d_src, bytes, d_covered, bytes)))
      m = "an output overlaps the source: the call is a gather and cannot run in place";
  }
  if (why) *why = m;
  return m.empty() ? FLVIS_OK : FLVIS_ERR_INVALID_ARG;
}

}  // namespace

namespace flvis {

void rc_cam21(const double* K4, const double* D4, const double* R9, const double* P12, double* cam21) {
  memcpy(cam21, K4, 4 * sizeof(double));
  memcpy(cam21 + 4, D4, 4 * sizeof(double));
  memcpy(cam21 + 8, R9, 9 * sizeof(double));
  cam21[17] = P12[0], cam21[18] = P12[5], cam21[19] = P12[2], cam21[20] = P12[6];
}

int rc_check(int n_img, int w, int h, int n_cam, const double* h_cam21, const int* h_cam_of, std::string* why) {
  std::string m;
  if (w <= 0 || h <= 0 || n_img <= 0 || n_cam <= 0)
    m = "the image shape and the counts must be positive";
  else if (!h_cam21)
    m = "NULL cameras";
  else if (!h_cam_of && n_cam != 1 && n_cam != n_img)
    m = "without h_cam_of n_cam must be 1 or n_img";
  for (int i = 0; m.empty() && h_cam_of && i < n_img; i++)
    if (h_cam_of[i] < 0 || h_cam_of[i] >= n_cam) m = "image " + std::to_string(i) + ": camera index out of range";
  for (int k = 0; m.empty() && k < n_cam; k++) {
    const double* c = h_cam21 + 21 * (size_t)k;
    bool ok = c[0] > 0 && c[1] > 0 && c[17] > 0 && c[18] > 0;
    for (int j = 0; j < 21; j++) ok = ok && std::isfinite(c[j]);
    if (!ok) m = "camera " + std::to_string(k) + ": an entry is not finite, or fx, fy, fx' or fy' is not positive";
  }
  if (why) *why = m;
  return m.empty() ? FLVIS_OK : FLVIS_ERR_INVALID_ARG;
}

int rc_run(flvis_ctx* ctx, const char* what, const uint8_t* d_src, int n_img, int w, int h, int n_cam, const double* h_cam21,
           const int* h_cam_of, const int* h_src_of, uint8_t* d_dst, uint8_t* d_covered) {
  const std::string pre = std::string(what) + ": ";
  const unsigned gx = (unsigned)((w + RC_TX * RC_PX - 1) / (RC_TX * RC_PX)), gy = (unsigned)((h + RC_TY - 1) / RC_TY);
  if (gy > 65535u) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "more than 524280 rows");
  // ---- runs of equal camera, none longer than what leaves the chip full (and none cut below RC_MIN_RUN)
  const long long tiles = (long long)gx * gy;
  const long long runs_wanted = std::max<long long>(1, (RC_BLOCKS + tiles - 1) / tiles);
  const int max_run = (int)std::max<long long>(RC_MIN_RUN, ((long long)n_img + runs_wanted - 1) / runs_wanted);
  auto cam_of = [&](int i) { return h_cam_of ? h_cam_of[i] : (n_cam == 1 ? 0 : i); };
  std::vector<int> run3;
  for (int i = 0; i < n_img;) {
    int j = i + 1;
    while (j < n_img && j - i < max_run && cam_of(j) == cam_of(i)) j++;
    run3.push_back(i), run3.push_back(j - i), run3.push_back(cam_of(i));
    i = j;
  }
  const size_t n_runs = run3.size() / 3;
  // ---- tables: cam21 [n_cam][21] | run3 [runs][3] | src_of [n_img]
  const size_t cam_bytes = 21 * sizeof(double) * (size_t)n_cam, run_bytes = 4 * run3.size(), src_bytes = h_src_of ? 4 * (size_t)n_img : 0;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  uint8_t* const tab = (uint8_t*)ctx->scratch("rc_tab", cam_bytes + run_bytes + src_bytes);
  if (!tab) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, pre + "device allocation failed");
  }
  double* const d_cam = (double*)tab;
  int* const d_run = (int*)(tab + cam_bytes);
  int* const d_srcof = h_src_of ? d_run + run3.size() : nullptr;
  hipError_t e = hipMemcpyAsync(d_cam, h_cam21, cam_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_run, run3.data(), run_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && h_src_of) e = hipMemcpyAsync(d_srcof, h_src_of, src_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the caller's arrays and run3 are free again on return)
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  for (size_t r0 = 0; r0 < n_runs; r0 += 65535) {
    const RcArgs a{d_src, d_dst, d_covered, d_cam, d_run, d_srcof, w, h, (int)r0};
    k_rectify<<<dim3(gx, gy, (unsigned)std::min<size_t>(65535, n_runs - r0)), dim3(RC_TX, RC_TY), 0, st>>>(a);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}

}  // namespace flvis

extern "C" {

int flvis_rectify_check(const uint8_t* d_src, int n_img, int w, int h, int n_cam, const double* h_cam21, const int* h_cam_of,
                        const uint8_t* d_dst, const uint8_t* d_covered) {
  int rc = rc_check_ptrs(d_src, n_img, w, h, h_cam21, d_dst, d_covered, nullptr);
  if (rc == FLVIS_OK) rc = flvis::rc_check(n_img, w, h, n_cam, h_cam21, h_cam_of, nullptr);
  return rc;
}

int flvis_hip_rectify(flvis_ctx* ctx, const uint8_t* d_src, int n_img, int w, int h, int n_cam, const double* h_cam21, const int* h_cam_of,
                      uint8_t* d_dst, uint8_t* d_covered) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  std::string why;
  int rc = rc_check_ptrs(d_src, n_img, w, h, h_cam21, d_dst, d_covered, &why);
  if (rc == FLVIS_OK) rc = flvis::rc_check(n_img, w, h, n_cam, h_cam21, h_cam_of, &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, "rectify: " + why);
  return flvis::rc_run(ctx, "rectify", d_src, n_img, w, h, n_cam, h_cam21, h_cam_of, nullptr, d_dst, d_covered);
}

}  // extern "C"
