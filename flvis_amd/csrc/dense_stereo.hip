// flvis_amd: dense stereo on a rectified pair (flvis_hip_dense_stereo; include/flvis_hip.h has the definition).
//
// The reference has no dense matcher: like the voxel filter this is the project's own definition -- census 9 x 7, Hamming cost, a box
// sum of radius agg_r, lowest-d argmin, uniqueness, left-right check, parabola in 1/16 px, depth as Z16 -- integer until one fp64 division.
//
// No cost volume exists.  One kernel, k_ds_match<R, RIGHT>, runs twice per batch of images:
//   RIGHT = true   the right view's argmin per pixel u' (cost A(u' + d, v, d)) into a 2-byte-per-pixel workspace map (skipped with lr_tol -1)
//   RIGHT = false  the left view: argmin, the three smallest other costs, the neighbours of the best, the checks, both outputs
// A workgroup of 256 threads owns 8 rows x (256 - 2 R) columns of one image; thread t is column xs + t of the tile and its halo.
//   census     the raw bytes of the band (8 + 2 R + 6 rows) go to LDS once; each thread keeps the census words of its OWN column (8 + 2 R
//              rows, as two 32-bit halves each) in registers, and the other image's words of the columns a chunk of <= 64 disparities
//              reaches go to LDS (restaged per chunk: LDS stays under 64 KiB at n_disp 256)
//   per d      vertical: the thread's column of Hamming costs (xor, two bit counts per row) as a running sum over 2 R + 1 rows, two output rows
//              packed in one 32-bit word (a box sum is at most 62 * 81 < 2^16: no carry between the halves), written to LDS;
//              horizontal: 2 R + 1 packed words summed per row pair; one barrier per d (the packed rows are double-buffered)
//   state      per pixel in registers: the four smallest (cost << 16 | d) keys -- a min / max insertion, the lowest d wins a tie by the key's
//              order, and the smallest cost more than one step from the best is among four keys because only two can be that close --
//              the cost of the previous d, and the costs at best - 1 and best + 1
// Every pixel of both outputs is written by exactly one thread; nothing is accumulated between threads but through the barrier-ordered
// LDS rows, so a second run and any batching give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "dense_stereo.hpp"

namespace {

constexpr int DS_T = 256;    // threads = columns of a tile with its halo
constexpr int DS_BH = 8;     // output rows of a tile
constexpr int DS_DCH = 64;   // disparities per staging of the other image's census words
constexpr int DS_WO = DS_T + DS_DCH - 1;
constexpr int DS_RAWO = DS_WO + 9;  // (WO + 8 raw columns, rounded up to a multiple of 4)
constexpr int DS_RAWB = DS_T + 8;
constexpr int DS_BATCH = 64;  // images per pair of launches: the right-view map is 2 bytes per pixel of one batch
constexpr uint32_t DS_NONE = 0xffffffffu;

struct DsArgs {
  const uint8_t *img0, *img1;  // [..][h][w]
  const int* src;              // item i reads image src[i] (NULL: image i)
  int w, h;
  int d_min, n_disp, uniq, lr_tol;
  const double* cam2;  // [n_cam][2] on the device; camera of item i: cam_stride * i
  int first, cam_stride;  // the launch's first item (blockIdx.z counts from it)
  uint16_t* rmap;  // [batch][h][w]: the right view's argmin, 0xffff: none
  uint16_t *disp16, *z16;  // [items][h][w], either may be NULL; with a grid z16 is [items][nv][nu]
  flvis::DsGrid grid;      // su == 0: every pixel
};

// the census word of the window whose top-left raw byte is `raw` (rows `stride` apart): 62 comparisons neighbour < centre
__device__ __forceinline__ uint2 ds_census(const uint8_t* raw, int stride) {
  const uint32_t c = raw[3 * stride + 4];
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int dy = 0; dy < 7; dy++)
#pragma unroll
    for (int dx = 0; dx < 9; dx++) {
      const int k = dy * 9 + dx;
      if (k == 31) continue;
      const uint32_t b = (uint32_t)raw[dy * stride + dx] < c ? 1u : 0u;
      if (k < 31)
        lo = (lo << 1) | b;
      else
        hi = (hi << 1) | b;
    }
  return make_uint2(lo, hi);
}

struct DsPix {
  uint32_t m0, m1, m2, m3;  // the four smallest keys, ascending
  uint32_t prev, p, n;      // A(d - 1), A(best - 1), A(best + 1)
};

__device__ __forceinline__ void ds_update(DsPix& s, uint32_t A, int d) {
  uint32_t key = (A << 16) | (uint32_t)d;
  if (d == (int)(s.m0 & 0xffffu) + 1 && s.m0 != DS_NONE) s.n = A;
  if (key < s.m0) s.p = s.prev;
  s.prev = A;
  uint32_t t;
  t = min(s.m0, key), key = max(s.m0, key), s.m0 = t;
  t = min(s.m1, key), key = max(s.m1, key), s.m1 = t;
  t = min(s.m2, key), key = max(s.m2, key), s.m2 = t;
  s.m3 = min(s.m3, key);
}

// rows [r0, r0 + rows) x columns [c0, c0 + cols) of `img` into LDS (row stride `stride`), 0 outside the image
__device__ __forceinline__ void ds_stage_raw(uint8_t* dst, int stride, const uint8_t* img, int w, int h, int r0, int rows, int c0, int cols) {
  for (int k = 0; k < rows; k++) {
    const int v = r0 + k;
    for (int j = threadIdx.x; j < cols; j += DS_T) {
      const int u = c0 + j;
      dst[k * stride + j] = (v >= 0 && v < h && u >= 0 && u < w) ? img[(size_t)v * w + u] : (uint8_t)0;
    }
  }
}

template <int R, bool RIGHT>
__global__ __launch_bounds__(DS_T) void k_ds_match(DsArgs a) {
  constexpr int RC = DS_BH + 2 * R;  // census rows of the band
  constexpr int RR = RC + 6;         // raw rows
  constexpr int TW = DS_T - 2 * R;   // output columns
  __shared__ uint2 co[RC * DS_WO];
  __shared__ uint32_t v2[2 * (DS_BH / 2) * DS_T];
  __shared__ uint8_t rawo[RR * DS_RAWO];
  __shared__ uint8_t rawb[RR * DS_RAWB];

  const int t = threadIdx.x;
  const int w = a.w, h = a.h;
  const int xs = (int)blockIdx.x * TW - R, x = xs + t;
  const int vb = (int)blockIdx.y * DS_BH;  // first output row; census row k is vb - R + k, raw row k is vb - R - 3 + k
  const int item = a.first + (int)blockIdx.z;
  const size_t in_off = (size_t)(a.src ? a.src[item] : item) * w * h;
  const size_t map_off = (size_t)blockIdx.z * w * h, out_off = (size_t)item * w * h;
  const uint8_t* base = (RIGHT ? a.img1 : a.img0) + in_off;
  const uint8_t* other = (RIGHT ? a.img0 : a.img1) + in_off;

  // ---- this thread's own column of census words
  ds_stage_raw(rawb, DS_RAWB, base, w, h, vb - R - 3, RR, xs - 4, DS_RAWB);
  __syncthreads();
  uint2 cb[RC];
#pragma unroll
  for (int k = 0; k < RC; k++) {
    const int vc = vb - R + k;
    const bool def = x >= 4 && x <= w - 5 && vc >= 3 && vc <= h - 4;
    cb[k] = def ? ds_census(rawb + k * DS_RAWB + t, DS_RAWB) : make_uint2(0u, 0u);
  }

  DsPix px[DS_BH];
#pragma unroll
  for (int i = 0; i < DS_BH; i++) px[i] = DsPix{DS_NONE, DS_NONE, DS_NONE, DS_NONE, 0u, 0u, 0u};

  const int d_last = a.d_min + a.n_disp - 1;
  // the highest d with A defined at this column (the row conditions and the far column condition do not depend on d: checked at the end)
  const int d_hi = min(d_last, RIGHT ? w - 5 - R - x : x - R - 4);
  const bool col_out = t >= R && t < DS_T - R && x < w;
  int buf = 0;

  for (int dc0 = a.d_min; dc0 <= d_last; dc0 += DS_DCH) {
    const int dc1 = min(d_last, dc0 + DS_DCH - 1), nd = dc1 - dc0 + 1;
    const int wo = DS_T + nd - 1;                  // columns of the other image this chunk reaches
    const int col0 = RIGHT ? xs + dc0 : xs - dc1;  // ... the first of them
    __syncthreads();  // (the raw rows of the previous chunk's census are read no more)
    ds_stage_raw(rawo, DS_RAWO, other, w, h, vb - R - 3, RR, col0 - 4, wo + 8);
    __syncthreads();
    for (int i = t; i < RC * wo; i += DS_T) {
      const int k = i / wo, j = i - k * wo;
      const int vc = vb - R + k, u = col0 + j;
      const bool def = u >= 4 && u <= w - 5 && vc >= 3 && vc <= h - 4;
      co[k * DS_WO + j] = def ? ds_census(rawo + k * DS_RAWO + j, DS_RAWO) : make_uint2(0u, 0u);
    }
    __syncthreads();

    for (int d = dc0; d <= dc1; d++) {
      const int oi = RIGHT ? t + d - dc0 : t + dc1 - d;  // in [0, wo)
      uint32_t H[RC];
#pragma unroll
      for (int k = 0; k < RC; k++) {
        const uint2 o = co[k * DS_WO + oi];
        H[k] = __popc(cb[k].x ^ o.x) + __popc(cb[k].y ^ o.y);
      }
      uint32_t V[DS_BH];
      uint32_t run = 0;
#pragma unroll
      for (int k = 0; k <= 2 * R; k++) run += H[k];
      V[0] = run;
#pragma unroll
      for (int i = 1; i < DS_BH; i++) {
        run = run + H[i + 2 * R] - H[i - 1];
        V[i] = run;
      }
      uint32_t* vrow = v2 + buf * (DS_BH / 2) * DS_T;
#pragma unroll
      for (int j = 0; j < DS_BH / 2; j++) vrow[j * DS_T + t] = V[2 * j] | (V[2 * j + 1] << 16);
      __syncthreads();
      if (col_out && d <= d_hi) {
#pragma unroll
        for (int j = 0; j < DS_BH / 2; j++) {
          uint32_t S = 0;
#pragma unroll
          for (int du = -R; du <= R; du++) S += vrow[j * DS_T + t + du];
          if (RIGHT) {
            px[2 * j].m0 = min(px[2 * j].m0, ((S & 0xffffu) << 16) | (uint32_t)d);
            px[2 * j + 1].m0 = min(px[2 * j + 1].m0, (S & 0xffff0000u) | (uint32_t)d);
          } else {
            ds_update(px[2 * j], S & 0xffffu, d);
            ds_update(px[2 * j + 1], S >> 16, d);
          }
        }
      }
      buf ^= 1;
    }
  }

  if (!col_out) return;
  const bool col_def = RIGHT ? x - R >= 4 : x + R <= w - 5;  // (the other column condition is d <= d_hi)
  double bf16 = 0, df = 0;
  if (!RIGHT && a.z16) {
    const double* c = a.cam2 + (size_t)a.cam_stride * item * 2;
    bf16 = c[0] * 16.0, df = c[1];
  }
#pragma unroll
  for (int i = 0; i < DS_BH; i++) {
    const int v = vb + i;
    if (v >= h) break;
    const size_t px_at = (size_t)v * w + x;
    const DsPix& s = px[i];
    bool ok = col_def && v - R >= 3 && v + R <= h - 4 && s.m0 != DS_NONE;
    const int best = (int)(s.m0 & 0xffffu);
    if (RIGHT) {
      a.rmap[map_off + px_at] = ok ? (uint16_t)best : (uint16_t)0xffffu;
      continue;
    }
    uint32_t d16 = 0;
    if (ok) {
      const uint32_t c = s.m0 >> 16;
      // uniqueness: the smallest cost more than one step away (the keys ascend by cost)
      uint32_t far = DS_NONE;
      const uint32_t ms[3] = {s.m1, s.m2, s.m3};
#pragma unroll
      for (int k = 2; k >= 0; k--)
        if (ms[k] != DS_NONE && abs((int)(ms[k] & 0xffffu) - best) > 1) far = ms[k] >> 16;
      if (far != DS_NONE && far * (uint32_t)(100 - a.uniq) < c * 100u) ok = false;
      if (ok && a.lr_tol >= 0) {
        const int br = (int)a.rmap[map_off + px_at - (size_t)best];
        if (abs(br - best) > a.lr_tol) ok = false;
      }
      if (best - 1 < a.d_min || best + 1 > d_hi) ok = false;
      if (ok) {
        const int p = (int)s.p, n = (int)s.n, ci = (int)c;
        const int den = max(p + n - 2 * ci, 1);
        const int num = (p - n) * 16 + den;
        const int q = num >= 0 ? num / (2 * den) : -((-num + 2 * den - 1) / (2 * den));  // floor
        d16 = (uint32_t)(16 * best + q);
      }
    }
    if (a.disp16) a.disp16[out_off + px_at] = (uint16_t)d16;
    if (a.z16) {
      uint16_t z = 0;
      if (d16) {
        const double zm = bf16 / (double)d16;
        const double raw = rint(zm * df);
        if (raw >= 1.0 && raw <= 65535.0) z = (uint16_t)raw;
      }
      if (a.grid.su == 0) {
        a.z16[out_off + px_at] = z;
      } else {  // only the cloud's samples are kept: sample (iu, iv) of the item at [item][iv][iu]
        const flvis::DsGrid& g = a.grid;
        const int du = x - g.u0, dv = v - g.v0;
        if (du >= 0 && dv >= 0 && du % g.su == 0 && dv % g.sv == 0 && du / g.su < g.nu && dv / g.sv < g.nv)
          a.z16[((size_t)item * g.nv + dv / g.sv) * g.nu + du / g.su] = z;
      }
    }
  }
}

template <bool RIGHT>
void ds_launch(int R, dim3 grid, hipStream_t st, const DsArgs& a) {
  switch (R) {
    case 0: k_ds_match<0, RIGHT><<<grid, DS_T, 0, st>>>(a); break;
    case 1: k_ds_match<1, RIGHT><<<grid, DS_T, 0, st>>>(a); break;
    case 2: k_ds_match<2, RIGHT><<<grid, DS_T, 0, st>>>(a); break;
    case 3: k_ds_match<3, RIGHT><<<grid, DS_T, 0, st>>>(a); break;
    default: k_ds_match<4, RIGHT><<<grid, DS_T, 0, st>>>(a); break;
  }
}

}  // namespace

namespace flvis {

int ds_check(int n_img, int w, int h, int n_cam, const double* h_cam2, const flvis_dense_stereo_params* prm, std::string* why) {
  std::string m;
  int rc = FLVIS_OK;
  auto bad = [&](const char* s) { m = s, rc = FLVIS_ERR_INVALID_ARG; };
  if (!prm)
    bad("NULL params");
  else if (w <= 0 || h <= 0 || n_img <= 0)
    bad("the image shape and count must be positive");
  else if (prm->n_disp < 1 || prm->n_disp > 256)
    bad("n_disp outside 1..256");
  else if (prm->d_min < 0)
    bad("d_min < 0");
  else if (prm->d_min > 4095 - prm->n_disp)
    bad("d_min + n_disp > 4095: sixteen times the disparity must fit 16 bits");
  else if (prm->agg_r < 0 || prm->agg_r > 4)
    bad("agg_r outside 0..4");
  else if (prm->uniq < 0 || prm->uniq > 99)
    bad("uniq outside 0..99");
  else if (prm->lr_tol < -1)
    bad("lr_tol < -1");
  else if (!h_cam2)
    bad("NULL cameras");
  else if (n_cam != 1 && n_cam != n_img)
    bad("n_cam must be 1 or n_img");
  for (int k = 0; rc == FLVIS_OK && k < n_cam; k++)
    for (int j = 0; j < 2; j++)
      if (!std::isfinite(h_cam2[2 * (size_t)k + j]) || !(h_cam2[2 * (size_t)k + j] > 0))
        m = "camera " + std::to_string(k) + ": bf and depth_factor must be finite and positive", rc = FLVIS_ERR_INVALID_ARG;
  if (why) *why = m;
  return rc;
}

int ds_run(flvis_ctx* ctx, const char* what, const uint8_t* d_img0, const uint8_t* d_img1, int n_img, int w, int h, int n_cam,
           const double* h_cam2, const flvis_dense_stereo_params* prm, uint16_t* d_disp16, uint16_t* d_z16, const int* h_src, const DsGrid* grid) {
  const std::string pre = std::string(what) + ": ";
  if (!d_img0 || !d_img1) return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + "a NULL image");
  if (!d_disp16 && !d_z16) return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + "both outputs are NULL");
  std::string why;
  int rc = ds_check(n_img, w, h, n_cam, h_cam2, prm, &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const bool lr = prm->lr_tol >= 0;
  uint16_t* d_rmap = nullptr;
  if (lr) {
    d_rmap = (uint16_t*)ctx->scratch("ds_rmap", 2 * (size_t)std::min(n_img, DS_BATCH) * w * h);
    if (!d_rmap) {
      (void)hipGetLastError();
      return ctx->fail(FLVIS_ERR_HIP, pre + "device allocation failed");
    }
  }
  double* d_cam2 = (double*)ctx->scratch("ds_cam", 16 * (size_t)n_cam + (h_src ? 4 * (size_t)n_img : 0));
  if (!d_cam2) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, pre + "device allocation failed");
  }
  int* const d_src = h_src ? (int*)(d_cam2 + 2 * (size_t)n_cam) : nullptr;
  hipError_t e = hipMemcpyAsync(d_cam2, h_cam2, 16 * (size_t)n_cam, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && h_src) e = hipMemcpyAsync(d_src, h_src, 4 * (size_t)n_img, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the caller's arrays are free again on return)
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  const int R = prm->agg_r, TW = DS_T - 2 * R;
  for (int i0 = 0; i0 < n_img; i0 += DS_BATCH) {
    const int nb = std::min(DS_BATCH, n_img - i0);
    DsArgs a{d_img0, d_img1, d_src, w, h, prm->d_min, prm->n_disp, prm->uniq, prm->lr_tol, d_cam2, i0, n_cam == 1 ? 0 : 1, d_rmap,
             d_disp16, d_z16, grid ? *grid : DsGrid{0, 0, 0, 0, 0, 0}};
    const dim3 grid((unsigned)((w + TW - 1) / TW), (unsigned)((h + DS_BH - 1) / DS_BH), (unsigned)nb);
    if (grid.y > 65535u) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "more than 524280 rows");
    if (lr) ds_launch<true>(R, grid, st, a);
    ds_launch<false>(R, grid, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return ctx->hip_fail(e, what);
  }
  return FLVIS_OK;
}

}  // namespace flvis

extern "C" {

int flvis_dense_stereo_check(const uint8_t* d_img0, const uint8_t* d_img1, int n_img, int w, int h, int n_cam, const double* h_cam2,
                             const flvis_dense_stereo_params* prm, const uint16_t* d_disp16, const uint16_t* d_z16) {
  if (!d_img0 || !d_img1 || (!d_disp16 && !d_z16)) return FLVIS_ERR_INVALID_ARG;
  return flvis::ds_check(n_img, w, h, n_cam, h_cam2, prm, nullptr);
}

int flvis_hip_dense_stereo(flvis_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, int n_img, int w, int h, int n_cam,
                           const double* h_cam2, const flvis_dense_stereo_params* prm, uint16_t* d_disp16, uint16_t* d_z16) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  return flvis::ds_run(ctx, "dense_stereo", d_img0, d_img1, n_img, w, h, n_cam, h_cam2, prm, d_disp16, d_z16, nullptr, nullptr);
}

}  // extern "C"
