// flvis_amd: an occupancy map from depth keyframes (flvis_hip_occupancy, flvis_keyframe_log_occupancy; include/flvis_hip.h has the
// definition).
//
// The consumer of the reference's octomap feeder (src/octofeeder/octomap_feeder.cpp:18-80 hands a cloud and the sensor pose to an octomap
// server) casts a ray from the sensor to every point and keeps a clamped log-odds value per voxel.  Here every valid sample of the dense
// cloud's front end (dc_samp.hpp: the same samples, the same raster order, the same map-frame point) is a ray, every voxel a ray crosses is
// a RECORD (voxel key, canonical index, scan << 1 | hit), and the records go through the voxel cloud's stable radix sort (mc_sort,
// unchanged).  Behind the sort the records of one (voxel, scan) lie together and a voxel's scans ascend, so the map is one reduction.
//
// Steps of one call (every map of the call goes through each of them together):
//   k_oc_prior_check           the prior's keys ascend strictly per map (a flag the host reads with the counts)
//   k_oc_count                 one workgroup per listed image and row chunk (k_dc_count's grid): its rays, its dropped rays and its records.
//                              A ray's records are |ie - io|_1 + 1, known from its two end cells: nothing is walked here.
//   mc_offsets                 the scan over (image, chunk): where each chunk's records start in canonical order (map, scan, raster, step)
//   k_oc_prior_emit            a map's prior rows are its FIRST records (they stand for a scan before scan 0)
//   k_oc_emit                  the same workgroups again: a lane walks its ray and writes key, index and payload at exact positions -- the
//                              round's base + the records of the waves before its own (LDS) + those of the lanes below it (wave prefix sum)
//   mc_sort                    stable, by (map | key): equal keys keep canonical order
//   k_oc_flags / k_oc_scan / k_oc_obs   runs of one (voxel, scan) collapse to one OBSERVATION each: head flags, a segmented "any hit" inside
//                              the workgroup's 1024 positions (LDS) and across workgroups (see below), positions by prefix counts
//   k_oc_map_rank              every map's first output row
//   k_oc_apply                 one lane per voxel starts from the prior's value or 0 and applies the voxel's observations in scan order
// No atomic decides a position or a value: LDS atomics only add counts, take a minimum and OR hit bits, which no order changes.
//
// THE WORST RUN.  Every ray of a scan emits the scan's origin voxel, so a step-1 VGA scan leaves ~300 k records of one key and scan next
// to each other.  No lane walks raw records: k_oc_flags / k_oc_obs read every sorted position once, in parallel.  A run that spans
// workgroups is closed by the workgroup that holds its head: wave 0 reads the summaries (has a head, any hit before it) of the following
// workgroups 64 at a time until one has a head -- a run holds at most one record per ray of its scan (the walk visits no cell twice), so
// at most samples-per-image / 1024 summaries, 300 for VGA, five rounds of one wave.  Sequential work starts only in k_oc_apply, whose lane
// walks OBSERVATIONS: at most one per scan of the map plus the prior.
// Lanes of k_oc_emit walk rays of different lengths and store 8-byte keys to per-lane runs; profiles/r29_occupancy.md has what that costs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "dc_samp.hpp"
#include "dev_math.hpp"
#include "kf_log.hpp"
#include "map_cloud.hpp"
#include "oc_cell.hpp"
#include "occupancy.hpp"
#include "pipeline_host.hpp"

namespace {

using namespace flvis;

constexpr int OC_T = 256;
constexpr int OC_RB = 1024;                                 // sorted positions per workgroup of the reduce kernels
constexpr int OC_PER = OC_RB / OC_T;                        // ... per lane, consecutive
constexpr int OC_BYTES_PER_RECORD = 2 * 8 + 2 * 4 + 4 + 4;  // two key buffers, two index buffers, payload, voxel rank of an observation
constexpr int OC_BYTES_PER_RAY = 0;                         // a ray is never stored: count and emit both derive it from its sample
constexpr int OC_BYTES_PER_IMAGE = 5 * 4;                   // image, pose row, camera, map, scan (+ OC_BYTES_PER_CHUNK per row chunk)
constexpr int OC_BYTES_PER_CHUNK = 8 + 3 * 4;               // running sum; records, rays, dropped rays
constexpr uint32_t OC_PRIOR_PAY = 0xfffffffeu;              // payload of a prior row: a scan number no image has
constexpr long long OC_DEFAULT_MAX_RECORDS = 1ll << 26;

#define OC_LAUNCH(c, what)                                   \
  do {                                                       \
    hipError_t e__ = hipGetLastError();                      \
    if (e__ != hipSuccess) return (c)->hip_fail(e__, what);  \
  } while (0)

struct OcItems {
  const int *img, *pose, *cam, *map, *scan;  // [R]
  const double* cam5;                        // [n_cams][5]
  const uint16_t* depth;
  const double* pose7;
  size_t pose_stride;
};

// the sample's camera-frame point by the dense cloud's rule, through the dense cloud's transform
FD V3 oc_end(const SE3d& T, const Q4& qi, int u, int v, float z, double fx, double fy, double cx, double cy) {
  const double zd = (double)z;
  const V3 p_c{((double)u - cx) * zd / fx, ((double)v - cy) * zd / fy, zd};
  return q_rotate(qi, p_c - T.t);
}

// sums of one value per lane over the workgroup, in t == 0 (LDS tree; `red` [OC_T])
template <class V>
FD V oc_block_sum(V v, V* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = OC_T / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const V r = red[0];
  __syncthreads();
  return r;
}

// grid: items x chunks (chunk fastest); per block its records (clamped to INT_MAX: the call is refused then), rays and dropped rays
__global__ __launch_bounds__(OC_T) void k_oc_count(OcItems it, DcSamp s, double leaf, int* __restrict__ cnt, int* __restrict__ rays,
                                                   int* __restrict__ drops) {
  __shared__ long long red[OC_T];
  const int t = threadIdx.x;
  const int e = blockIdx.x / s.chunks, c = blockIdx.x - e * s.chunks;
  const uint16_t* img = it.depth + (size_t)it.img[e] * s.img_px();
  const double* cam = it.cam5 + 5 * (size_t)it.cam[e];
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], df = cam[4];
  const SE3d T = load_pose7(it.pose7 + (size_t)it.pose[e] * it.pose_stride);
  const Q4 qi = q_conj(T.q);
  const V3 o = q_rotate(qi, V3{0, 0, 0} - T.t);
  int iox = 0, ioy = 0, ioz = 0;
  const bool o_ok = oc_cell(o, leaf, iox, ioy, ioz);
  const int n = dc_chunk_samples(s, c);
  long long rec = 0, nr = 0, nd = 0;
  for (int j = t; j < n; j += OC_T) {
    int u, v;
    float z;
    const size_t at = dc_pixel(s, c, j, u, v);
    if (!dc_valid(img[at], df, s, z)) continue;
    const V3 p = oc_end(T, qi, u, v, z, fx, fy, cx, cy);
    int iex, iey, iez;
    if (o_ok && oc_cell(p, leaf, iex, iey, iez)) {
      nr++;
      rec += (long long)abs(iex - iox) + abs(iey - ioy) + abs(iez - ioz) + 1;
    } else {
      nd++;
    }
  }
  rec = oc_block_sum(rec, red);
  nr = oc_block_sum(nr, red);
  nd = oc_block_sum(nd, red);
  if (t == 0) {
    cnt[blockIdx.x] = (int)min(rec, (long long)INT_MAX);
    rays[blockIdx.x] = (int)nr;
    drops[blockIdx.x] = (int)nd;
  }
}

// one block per map: its rays and dropped rays over its chunks eptrc[m] .. eptrc[m + 1]
__global__ __launch_bounds__(OC_T) void k_oc_map_sums(const int* __restrict__ eptrc, const int* __restrict__ rays, const int* __restrict__ drops,
                                                      long long* __restrict__ out2) {
  __shared__ long long red[OC_T];
  const int m = blockIdx.x;
  long long a = 0, b = 0;
  for (int i = eptrc[m] + threadIdx.x; i < eptrc[m + 1]; i += OC_T) a += rays[i], b += drops[i];
  a = oc_block_sum(a, red);
  b = oc_block_sum(b, red);
  if (threadIdx.x == 0) out2[2 * m] = a, out2[2 * m + 1] = b;
}

// grid (row slabs, maps): *bad = 1 if a map's prior keys do not ascend strictly or a key has its top bit set
__global__ __launch_bounds__(OC_T) void k_oc_prior_check(const int64_t* __restrict__ pkey, int prior_cap, const int* __restrict__ nprior,
                                                         int* __restrict__ bad) {
  const int m = blockIdx.y, r = blockIdx.x * OC_T + threadIdx.x;
  if (r >= nprior[m]) return;
  const int64_t k = pkey[(size_t)m * prior_cap + r];
  if (k < 0 || (r > 0 && pkey[(size_t)m * prior_cap + r - 1] >= k)) *bad = 1;
}

FD void oc_mark(uint8_t* seen, uint64_t key, uint64_t diff) {
#pragma unroll
  for (int d = 0; d < MC_KEY_DIGITS; d++)
    if ((diff >> (8 * d)) & 255) seen[d * 256 + (int)((key >> (8 * d)) & 255)] = 1;
}

// grid (row slabs, maps): prior row r of map m is canonical record cstart[m] + r
__global__ __launch_bounds__(OC_T) void k_oc_prior_emit(const int64_t* __restrict__ pkey, int prior_cap, const int* __restrict__ nprior,
                                                        const int* __restrict__ cstart, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                        uint32_t* __restrict__ pay, int* __restrict__ occ) {
  __shared__ uint8_t seen[MC_KEY_DIGITS * 256];
  const int t = threadIdx.x, m = blockIdx.y, r = blockIdx.x * OC_T + t;
  if (blockIdx.x * OC_T >= nprior[m]) return;  // (uniform)
  for (int i = t; i < MC_KEY_DIGITS * 256; i += OC_T) seen[i] = 0;
  __syncthreads();
  if (r < nprior[m]) {
    const uint64_t k = (uint64_t)pkey[(size_t)m * prior_cap + r];
    const size_t pos = (size_t)cstart[m] + r;
    keys[pos] = k, idx[pos] = (uint32_t)pos, pay[pos] = OC_PRIOR_PAY;
    oc_mark(seen, k, ~0ull);
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < MC_KEY_DIGITS; d++)
    if (seen[d * 256 + t]) occ[d * 256 + t] = 1;
}

// k_oc_count's grid; off[block]: the chunk's first record among the scans' records, shift[map]: the prior rows of the maps up to its own
__global__ __launch_bounds__(OC_T) void k_oc_emit(OcItems it, DcSamp s, double leaf, const int* __restrict__ cnt, const long long* __restrict__ off,
                                                  const int* __restrict__ shift, int n_total, uint64_t* __restrict__ keys,
                                                  uint32_t* __restrict__ idx, uint32_t* __restrict__ pay, int* __restrict__ occ) {
  __shared__ uint8_t seen[MC_KEY_DIGITS * 256];
  __shared__ int wsum[OC_T / 64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (cnt[blockIdx.x] == 0) return;
  for (int i = t; i < MC_KEY_DIGITS * 256; i += OC_T) seen[i] = 0;
  __syncthreads();
  const int e = blockIdx.x / s.chunks, c = blockIdx.x - e * s.chunks;
  const uint16_t* img = it.depth + (size_t)it.img[e] * s.img_px();
  const double* cam = it.cam5 + 5 * (size_t)it.cam[e];
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], df = cam[4];
  const SE3d T = load_pose7(it.pose7 + (size_t)it.pose[e] * it.pose_stride);
  const Q4 qi = q_conj(T.q);
  const V3 o = q_rotate(qi, V3{0, 0, 0} - T.t);
  int iox = 0, ioy = 0, ioz = 0;
  const bool o_ok = oc_cell(o, leaf, iox, ioy, ioz);  // (false: the chunk has no record and returned above)
  const uint32_t scan2 = (uint32_t)it.scan[e] << 1;
  const long long base = off[blockIdx.x] + shift[it.map[e]];
  const int n = dc_chunk_samples(s, c);
  long long done = 0;
  for (int j0 = 0; j0 < n; j0 += OC_T) {
    const int j = j0 + t;
    int iex = 0, iey = 0, iez = 0, mine = 0;
    V3 p{0, 0, 0};
    if (j < n) {
      int u, v;
      float z;
      const size_t at = dc_pixel(s, c, j, u, v);
      if (dc_valid(img[at], df, s, z)) {
        p = oc_end(T, qi, u, v, z, fx, fy, cx, cy);
        if (o_ok && oc_cell(p, leaf, iex, iey, iez)) mine = abs(iex - iox) + abs(iey - ioy) + abs(iez - ioz) + 1;
      }
    }
    int incl = mine;  // the wave's running sum, this lane included
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    long long pos = base + done + (incl - mine), total = 0;
#pragma unroll
    for (int k = 0; k < OC_T / 64; k++) {
      pos += k < w ? wsum[k] : 0;
      total += wsum[k];
    }
    if (mine > 0) {
      int rx = abs(iex - iox), ry = abs(iey - ioy), rz = abs(iez - ioz);
      const int sx = iex >= iox ? 1 : -1, sy = iey >= ioy ? 1 : -1, sz = iez >= ioz ? 1 : -1;
      const double dx = p.x - o.x, dy = p.y - o.y, dz = p.z - o.z;
      double tx = 0, ty = 0, tz = 0, ex = 0, ey = 0, ez = 0;
      if (rx > 0) tx = ((double)(iox + (sx > 0 ? 1 : 0)) * leaf - o.x) / dx, ex = leaf / fabs(dx);
      if (ry > 0) ty = ((double)(ioy + (sy > 0 ? 1 : 0)) * leaf - o.y) / dy, ey = leaf / fabs(dy);
      if (rz > 0) tz = ((double)(ioz + (sz > 0 ? 1 : 0)) * leaf - o.z) / dz, ez = leaf / fabs(dz);
      int x = iox, y = ioy, zc = ioz;
      uint64_t prev = 0, diff = ~0ull;
      for (int k = 0; k < mine; k++, pos++) {  // (mine = the steps + 1: the loop cannot run on, whatever the tmax are)
        const uint64_t key = oc_key(x, y, zc);
        if (k) diff = key ^ prev;
        prev = key;
        if (pos < n_total) {
          keys[pos] = key;
          idx[pos] = (uint32_t)pos;
          pay[pos] = scan2 | (k == mine - 1 ? 1u : 0u);
        }
        oc_mark(seen, key, diff);
        int a = -1;
        double best = 0;
        if (rx > 0) a = 0, best = tx;
        if (ry > 0 && (a < 0 || ty < best)) a = 1, best = ty;
        if (rz > 0 && (a < 0 || tz < best)) a = 2;
        if (a == 0) x += sx, rx--, tx += ex;
        else if (a == 1) y += sy, ry--, ty += ey;
        else if (a == 2) zc += sz, rz--, tz += ez;
      }
    }
    __syncthreads();
    done += total;
  }
#pragma unroll
  for (int d = 0; d < MC_KEY_DIGITS; d++)
    if (seen[d * 256 + t]) occ[d * 256 + t] = 1;
}

// out[i] = in[0] + .. + in[i - 1] for i in 0 .. n, one workgroup (map_cloud.hip's k_mc_scan: a count per OC_RB sorted positions)
__global__ __launch_bounds__(1024) void k_oc_scan(const int* in, int n, int* out) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024, lo = min(n, t * per), hi = min(n, lo + per);
  int s = 0;
  for (int i = lo; i < hi; i++) s += in[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int a = 0;
    for (int k = 0; k < 1024; k++) {
      const int v = part[k];
      part[k] = a;
      a += v;
    }
    out[n] = a;
  }
  __syncthreads();
  int a = part[t];
  for (int i = lo; i < hi; i++) {
    const int v = in[i];
    out[i] = a;
    a += v;
  }
}

// the sorted records: K keys, I canonical indices, P payloads BY CANONICAL INDEX; cstart [n_maps + 1] the maps' first positions
struct OcSorted {
  const uint64_t* K;
  const uint32_t* I;
  const uint32_t* P;
  const int* cstart;
  int n_maps, n;
};
FD bool oc_is_map_start(const OcSorted& s, int i) {  // (an empty map shares its start with the next one: `i` starts the one that holds it)
  int lo = 0, hi = s.n_maps;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s.cstart[mid] <= i) lo = mid;
    else hi = mid;
  }
  return s.cstart[lo] == i;
}
FD bool oc_vhead(const OcSorted& s, int i) { return i == 0 || s.K[i - 1] != s.K[i] || oc_is_map_start(s, i); }
enum { OC_HIT = 1, OC_OHEAD = 2, OC_VHEAD = 4 };
// flags of the lane's OC_PER consecutive positions from `base` on (0 behind the end)
FD void oc_lane_flags(const OcSorted& s, int base, uint32_t* f) {
  const uint32_t last = (uint32_t)(s.n - 1);  // (an index is a canonical position < n; the min keeps a read inside the buffer regardless)
  uint32_t pprev = base > 0 && base < s.n ? s.P[min(s.I[base - 1], last)] : 0u;
#pragma unroll
  for (int k = 0; k < OC_PER; k++) {
    const int i = base + k;
    f[k] = 0;
    if (i >= s.n) continue;
    const uint32_t p = s.P[min(s.I[i], last)];
    const bool vh = oc_vhead(s, i);
    f[k] = (p & 1u) | (vh || (p >> 1) != (pprev >> 1) ? OC_OHEAD : 0) | (vh ? OC_VHEAD : 0);
    pprev = p;
  }
}

// per workgroup of OC_RB positions: observation heads, voxel heads, and bsum = has a head | (a hit before its first head) << 1
__global__ __launch_bounds__(OC_T) void k_oc_flags(OcSorted s, int* __restrict__ bo, int* __restrict__ bv, int* __restrict__ bsum) {
  __shared__ int s_o, s_v, s_first, s_pre;
  const int t = threadIdx.x;
  if (t == 0) s_o = 0, s_v = 0, s_first = INT_MAX, s_pre = 0;
  __syncthreads();
  const int base = blockIdx.x * OC_RB + t * OC_PER;
  uint32_t f[OC_PER];
  oc_lane_flags(s, base, f);
  int co = 0, cv = 0, first = INT_MAX;
#pragma unroll
  for (int k = 0; k < OC_PER; k++) {
    if ((f[k] & OC_OHEAD) && first == INT_MAX) first = base + k;
    co += (f[k] & OC_OHEAD) ? 1 : 0;
    cv += (f[k] & OC_VHEAD) ? 1 : 0;
  }
  if (co) atomicAdd(&s_o, co), atomicMin(&s_first, first);
  if (cv) atomicAdd(&s_v, cv);
  __syncthreads();
  bool pre = false;
#pragma unroll
  for (int k = 0; k < OC_PER; k++) pre = pre || ((f[k] & OC_HIT) && base + k < s_first);
  if (pre) atomicOr(&s_pre, 1);
  __syncthreads();
  if (t == 0) bo[blockIdx.x] = s_o, bv[blockIdx.x] = s_v, bsum[blockIdx.x] = (s_first != INT_MAX ? 1 : 0) | (s_pre << 1);
}

// opre / vpre: k_oc_flags' counts after the scan.  Observation j: okey[j] its voxel, oci[j] the canonical index of its first record with
// the "any hit" in bit 31, ovox[j] the rank of its voxel among the call's voxels
__global__ __launch_bounds__(OC_T) void k_oc_obs(OcSorted s, const int* __restrict__ opre, const int* __restrict__ vpre,
                                                 const int* __restrict__ bsum, int nblk, uint64_t* __restrict__ okey, uint32_t* __restrict__ oci,
                                                 int* __restrict__ ovox) {
  __shared__ int sc_o[OC_T], sc_v[OC_T];
  __shared__ int seg_or[OC_RB + 1];
  __shared__ int s_tail;
  const int t = threadIdx.x;
  const int base = blockIdx.x * OC_RB + t * OC_PER;
  uint32_t f[OC_PER];
  oc_lane_flags(s, base, f);
  int co = 0, cv = 0;
#pragma unroll
  for (int k = 0; k < OC_PER; k++) co += (f[k] & OC_OHEAD) ? 1 : 0, cv += (f[k] & OC_VHEAD) ? 1 : 0;
  sc_o[t] = co, sc_v[t] = cv;
  for (int i = t; i < OC_RB + 1; i += OC_T) seg_or[i] = 0;
  if (t == 0) s_tail = 0;
  __syncthreads();
  for (int d = 1; d < OC_T; d <<= 1) {
    const int a = t >= d ? sc_o[t - d] : 0, b = t >= d ? sc_v[t - d] : 0;
    __syncthreads();
    sc_o[t] += a, sc_v[t] += b;
    __syncthreads();
  }
  const int total_o = sc_o[OC_T - 1];
  int seg = sc_o[t] - co;  // observation heads of the workgroup before this lane's positions
#pragma unroll
  for (int k = 0; k < OC_PER; k++) {
    seg += (f[k] & OC_OHEAD) ? 1 : 0;
    if (f[k] & OC_HIT) atomicOr(&seg_or[seg], 1);  // (segment 0: the run a workgroup before this one began)
  }
  if (t < 64 && total_o > 0) {  // wave 0: does the workgroup's last run go on into a hit?
    int tail = 0;
    bool found = false;
    for (int b0 = blockIdx.x + 1; b0 < nblk && !found; b0 += 64) {
      const int bb = b0 + t, v = bb < nblk ? bsum[bb] : 1;
      const unsigned long long hh = __ballot(v & 1), pp = __ballot((v >> 1) & 1);
      if (hh) {
        const int fh = __ffsll((long long)hh) - 1;
        const unsigned long long upto = fh == 63 ? ~0ull : ((1ull << (fh + 1)) - 1ull);
        tail |= (pp & upto) ? 1 : 0;
        found = true;
      } else {
        tail |= pp ? 1 : 0;
      }
    }
    if (t == 0) s_tail = tail;
  }
  __syncthreads();
  seg = sc_o[t] - co;
  int vin = sc_v[t] - cv;
#pragma unroll
  for (int k = 0; k < OC_PER; k++) {
    vin += (f[k] & OC_VHEAD) ? 1 : 0;
    if (!(f[k] & OC_OHEAD)) continue;
    seg++;
    const int i = base + k;
    const size_t at = (size_t)opre[blockIdx.x] + seg - 1;
    const uint32_t hit = (uint32_t)(seg_or[seg] | (seg == total_o ? s_tail : 0));
    okey[at] = s.K[i];
    oci[at] = s.I[i] | (hit << 31);
    ovox[at] = vpre[blockIdx.x] + vin - 1;
  }
}

// mv[m]: the voxels before map m (m == n_maps: of the whole call); mv[n_maps + 1] = the observations of the call
__global__ __launch_bounds__(OC_T) void k_oc_map_rank(OcSorted s, const int* __restrict__ vpre, const int* __restrict__ opre, int nblk,
                                                      int* __restrict__ mv) {
  __shared__ int red[OC_T];
  const int pos = s.cstart[blockIdx.x];  // (cstart[n_maps] == n)
  const int chunk = pos / OC_RB;
  int cnt = 0;
  for (int i = chunk * OC_RB + threadIdx.x; i < pos; i += OC_T) cnt += oc_vhead(s, i) ? 1 : 0;
  cnt = oc_block_sum(cnt, red);
  if (threadIdx.x == 0) {
    mv[blockIdx.x] = vpre[chunk] + cnt;
    if ((int)blockIdx.x == s.n_maps) mv[s.n_maps + 1] = opre[nblk];
  }
}

struct OcApply {
  const uint64_t* okey;
  const uint32_t* oci;
  const int* ovox;
  const int *mv, *cstart, *nprior;  // [n_maps + 1], [n_maps + 1], [n_maps]
  const float* prior_l;
  int prior_cap, n_maps, n_obs, out_cap;
  float l_hit, l_miss, l_min, l_max;
  double leaf;
  int64_t* key;
  float *l, *xyz;
};
// one lane per observation; the lane of a voxel's first one walks the voxel's observations (at most one per scan and the prior's)
__global__ __launch_bounds__(OC_T) void k_oc_apply(OcApply a) {
  const int j = blockIdx.x * OC_T + threadIdx.x;
  if (j >= a.n_obs) return;
  const int v = a.ovox[j];
  if (j > 0 && a.ovox[j - 1] == v) return;
  int lo = 0, hi = a.n_maps;  // the last map m with mv[m] <= v
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.mv[mid] <= v) lo = mid;
    else hi = mid;
  }
  const int m = lo, row = v - a.mv[m];
  if (row >= a.out_cap) return;
  float l = 0.0f;
  for (int q = j; q < a.n_obs && a.ovox[q] == v; q++) {
    const uint32_t ci = a.oci[q] & 0x7fffffffu;
    const int r = (int)ci - a.cstart[m];
    if (q == j && r >= 0 && r < a.nprior[m]) {
      l = a.prior_l[(size_t)m * a.prior_cap + r];
      continue;
    }
    l = l + ((a.oci[q] >> 31) ? a.l_hit : a.l_miss);
    l = l < a.l_min ? a.l_min : (l > a.l_max ? a.l_max : l);
  }
  const size_t at = (size_t)m * a.out_cap + row;
  const uint64_t k = a.okey[j];
  a.key[at] = (int64_t)k;
  a.l[at] = l;
  if (a.xyz) {
    const int ix = (int)(k & 0x1fffff) - (1 << 20), iy = (int)((k >> 21) & 0x1fffff) - (1 << 20), iz = (int)((k >> 42) & 0x1fffff) - (1 << 20);
    a.xyz[3 * at] = (float)(((double)ix + 0.5) * a.leaf);
    a.xyz[3 * at + 1] = (float)(((double)iy + 0.5) * a.leaf);
    a.xyz[3 * at + 2] = (float)(((double)iz + 0.5) * a.leaf);
  }
}

double oc_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct OcPrior {
  const int64_t* d_key;
  const float* d_l;
  int cap;
  const int64_t* h_n;  // [n_maps] or NULL
};
// the rows' destination, asked for once the maps' row counts are known and before any row is written
using OcOutHook = std::function<int(const int64_t* n_out, OcOut* out)>;

// the chunk counts a count-only call left in the context's "oc_counts" buffer: records [m_all] | rays [m_all] | dropped [m_all] of ALL
// listed items; a batch reads the slice of its own items (from first_item on) in place of counting them again
struct OcCounted {
  const int* d;
  size_t m_all;
  int first_item;
};

// One call over the lists `L`.  item_records != NULL: the count pass alone -- the records of every item, read once, and the chunks'
// counts kept on the device (*kept).  counted != NULL: this call's items were counted by such a call.  h_n_rays / h_n_dropped are ADDED
// to (a batched caller sums over its batches), h_n_out is set.
int oc_core(flvis_ctx* ctx, const char* what, const OcLists& L, const flvis_depth_cloud_params* prm, double leaf,
            const flvis_occupancy_params* occ, const OcPrior& prior, const OcOutHook& hook, int64_t* h_n_out, int64_t* h_n_rays,
            int64_t* h_n_dropped, std::vector<long long>* item_records, OcCounted* kept = nullptr, const OcCounted* counted = nullptr) {
  const std::string pre = std::string(what) + ": ";
  DcSamp s;
  std::string why;
  int rc = dc_resolve(L.w, L.h, prm, s, why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  const int n_maps = L.n_maps, R = L.eptr[n_maps], NM1 = n_maps + 1;
  auto no_mem = [&]() {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, pre + "device allocation failed");
  };
  std::vector<int> nprior((size_t)n_maps, 0);
  int max_prior = 0;
  long long n_prior_all = 0;
  for (int m = 0; m < n_maps; m++) {
    nprior[m] = prior.h_n ? (int)prior.h_n[m] : 0;
    max_prior = std::max(max_prior, nprior[m]);
    n_prior_all += nprior[m];
  }
  if (item_records) item_records->assign((size_t)R, 0);
  const long long M64 = (long long)R * s.chunks;
  if (M64 > INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 (listed image, row chunk) pairs or more");
  const int M = (int)M64;
  if (R == 0 && n_prior_all == 0) {
    for (int m = 0; m < n_maps; m++) h_n_out[m] = 0;
    return FLVIS_OK;
  }
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const bool timing = ctx->dc_timing != 0;
  if (timing) hipStreamSynchronize(st);
  auto t0 = std::chrono::steady_clock::now();
  // ---- tables: off64 [M + 1] | cs64 [NM1] | sums [n_maps][2] | cam5 [n_cams][5] || eptr * chunks [NM1] | nprior [n_maps] | img [R] | pose [R] |
  //      cam [R] | map [R] | scan [R] || cnt [M] | rays [M] | drops [M] | cstart0 [NM1] | cstart [NM1] | shift [n_maps] | mv [NM1 + 1] | bad [1]
  //      (|| .. ||: one upload)
  const size_t up_bytes = 8 * 5 * (size_t)L.n_cams + 4 * ((size_t)NM1 + n_maps + 5 * (size_t)R);
  const size_t rows_bytes = 8 * ((size_t)M + 1 + NM1 + 2 * (size_t)n_maps) + up_bytes + 4 * (3 * (size_t)M + 3 * (size_t)NM1 + n_maps + 2);
  uint8_t* const rb = (uint8_t*)ctx->scratch("oc_rows", rows_bytes);
  if (!rb) return no_mem();
  long long* const d_off = (long long*)rb;
  long long* const d_cs64 = d_off + M + 1;
  long long* const d_sums = d_cs64 + NM1;
  double* const d_cam5 = (double*)(d_sums + 2 * (size_t)n_maps);
  int* const d_eptrc = (int*)(d_cam5 + 5 * (size_t)L.n_cams);
  int* const d_nprior = d_eptrc + NM1;
  int* const d_img = d_nprior + n_maps;
  int* const d_posei = d_img + R;
  int* const d_cami = d_posei + R;
  int* const d_mapi = d_cami + R;
  int* const d_scani = d_mapi + R;
  int* const d_cnt = d_scani + R;
  int* const d_rays = d_cnt + M;
  int* const d_drops = d_rays + M;
  int* const d_cstart0 = d_drops + M;
  int* const d_cstart = d_cstart0 + NM1;
  int* const d_shift = d_cstart + NM1;
  int* const d_mv = d_shift + n_maps;
  int* const d_bad = d_mv + NM1 + 1;
  std::vector<uint8_t> stage(up_bytes);
  {
    if (L.n_cams > 0) memcpy(stage.data(), L.cam5, 8 * 5 * (size_t)L.n_cams);
    int* p = (int*)(stage.data() + 8 * 5 * (size_t)L.n_cams);
    for (int m = 0; m <= n_maps; m++) p[m] = L.eptr[m] * s.chunks;  // (<= M)
    memcpy(p + NM1, nprior.data(), 4 * (size_t)n_maps);
    int* q = p + NM1 + n_maps;
    if (R > 0) {
      memcpy(q, L.img, 4 * (size_t)R);
      memcpy(q + R, L.pose, 4 * (size_t)R);
      memcpy(q + 2 * (size_t)R, L.cam, 4 * (size_t)R);
    }
    for (int m = 0; m < n_maps; m++)
      for (int e = L.eptr[m]; e < L.eptr[m + 1]; e++) q[3 * (size_t)R + e] = m, q[4 * (size_t)R + e] = e - L.eptr[m];
  }
  auto fail_sync = [&](int code) {  // (`stage` goes away on return)
    hipStreamSynchronize(st);
    return code;
  };
  hipError_t e = hipMemcpyAsync(d_cam5, stage.data(), up_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, sizeof(int), st);
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
  const OcItems it{d_img, d_posei, d_cami, d_mapi, d_scani, d_cam5, L.d_depth, L.d_pose, L.pose_stride};
  const dim3 pgrid((unsigned)((max_prior + OC_T - 1) / OC_T), (unsigned)n_maps);
  if (max_prior > 0 && !item_records) k_oc_prior_check<<<pgrid, OC_T, 0, st>>>(prior.d_key, prior.cap, d_nprior, d_bad);
  if (M > 0 && counted) {
    const int* src = counted->d + (size_t)counted->first_item * s.chunks;
    for (int k = 0; k < 3 && e == hipSuccess; k++)
      e = hipMemcpyAsync(d_cnt + (size_t)k * M, src + (size_t)k * counted->m_all, sizeof(int) * (size_t)M, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
  } else if (M > 0) {
    k_oc_count<<<M, OC_T, 0, st>>>(it, s, leaf, d_cnt, d_rays, d_drops);
  }
  if (M > 0 && kept) {  // (cnt | rays | drops are adjacent)
    int* keep = (int*)ctx->scratch("oc_counts", sizeof(int) * 3 * (size_t)M);
    if (!keep) return fail_sync(no_mem());
    e = hipMemcpyAsync(keep, d_cnt, sizeof(int) * 3 * (size_t)M, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
    *kept = OcCounted{keep, (size_t)M, 0};
  }
  mc_offsets(st, d_cnt, (long long)M, d_off, d_eptrc, n_maps, d_cs64, d_cstart0);
  k_oc_map_sums<<<n_maps, OC_T, 0, st>>>(d_eptrc, d_rays, d_drops, d_sums);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, (pre + "counts").c_str()));
  // back: cs64 [NM1] | sums [n_maps][2] (adjacent), the flag, and for a count-only call the chunks' counts
  std::vector<long long> back((size_t)NM1 + 2 * (size_t)n_maps);
  std::vector<int> h_cnt(item_records ? (size_t)M : 0);
  int h_bad = 0;
  e = hipMemcpyAsync(back.data(), d_cs64, sizeof(long long) * back.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && item_records && M > 0) e = hipMemcpyAsync(h_cnt.data(), d_cnt, sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st);
  {
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, (pre + "counts").c_str());
  if (timing) ctx->oc_ms[0] += oc_ms_since(t0), t0 = std::chrono::steady_clock::now();
  if (item_records) {
    for (int r = 0; r < R; r++)
      for (int c = 0; c < s.chunks; c++) (*item_records)[r] += h_cnt[(size_t)r * s.chunks + c];
    return FLVIS_OK;
  }
  if (h_bad) return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + "a map's prior keys are not valid keys in strictly ascending order");
  const long long* cs = back.data();
  for (int m = 0; m < n_maps; m++) {
    if (h_n_rays) h_n_rays[m] += back[(size_t)NM1 + 2 * m];
    if (h_n_dropped) h_n_dropped[m] += back[(size_t)NM1 + 2 * m + 1];
  }
  // (a chunk's count is clamped to INT_MAX, so a sum below it is exact)
  if (cs[n_maps] + n_prior_all >= (long long)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 - 1 records or more in one call");
  const int N = (int)(cs[n_maps] + n_prior_all);
  ctx->oc_stats[0] += N;
  for (int m = 0; m < n_maps; m++) ctx->oc_stats[1] += back[(size_t)NM1 + 2 * m];
  if (N == 0) {
    for (int m = 0; m < n_maps; m++) h_n_out[m] = 0;
    return FLVIS_OK;
  }
  // ---- the maps' first records with the prior rows in front, and what that adds to a chunk's offset
  std::vector<long long> cs2((size_t)NM1);
  std::vector<int> up2(2 * (size_t)NM1);  // cstart [NM1] | shift [n_maps] (adjacent on the device)
  {
    long long pr = 0;
    for (int m = 0; m < n_maps; m++) {
      cs2[m] = cs[m] + pr;
      pr += nprior[m];
      up2[(size_t)NM1 + m] = (int)pr;
    }
    cs2[n_maps] = N;
    for (int m = 0; m <= n_maps; m++) up2[m] = (int)cs2[m];
  }
  e = hipMemcpyAsync(d_cstart, up2.data(), sizeof(int) * ((size_t)NM1 + n_maps), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
  // ---- per record: keys [2][N] | idx [2][N] | pay [N] | ovox [N]; tables: byte values | the sort's | bo, bv [nblk + 1] each | bsum [nblk]
  const int nblk = (N + OC_RB - 1) / OC_RB;
  const size_t tab_sort = mc_sort_table_ints(N);
  const size_t tab_ints = (size_t)MC_KEY_DIGITS * 256 + tab_sort + 3 * (size_t)nblk + 2;
  uint8_t* const pb = (uint8_t*)ctx->scratch("oc_records", (size_t)N * OC_BYTES_PER_RECORD);
  if (!pb) return fail_sync(no_mem());
  int* const d_occ = (int*)ctx->scratch("oc_tables", sizeof(int) * tab_ints);
  if (!d_occ) return fail_sync(no_mem());
  uint64_t* const keys[2] = {(uint64_t*)pb, (uint64_t*)pb + N};
  uint32_t* const idx[2] = {(uint32_t*)(keys[1] + N), (uint32_t*)(keys[1] + N) + N};
  uint32_t* const pay = idx[1] + N;
  int* const ovox = (int*)(pay + N);
  uint32_t* const d_hist = (uint32_t*)(d_occ + MC_KEY_DIGITS * 256);
  int* const d_bo = (int*)(d_hist + tab_sort);
  int* const d_bv = d_bo + nblk + 1;
  int* const d_bsum = d_bv + nblk + 1;
  ctx->oc_stats[3] = std::max<int64_t>(ctx->oc_stats[3], (int64_t)((size_t)N * OC_BYTES_PER_RECORD + sizeof(int) * tab_ints + rows_bytes));
  e = hipMemsetAsync(d_occ, 0, sizeof(int) * MC_KEY_DIGITS * 256, st);
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
  if (max_prior > 0) k_oc_prior_emit<<<pgrid, OC_T, 0, st>>>(prior.d_key, prior.cap, d_nprior, d_cstart, keys[0], idx[0], pay, d_occ);
  if (M > 0) k_oc_emit<<<M, OC_T, 0, st>>>(it, s, leaf, d_cnt, d_off, d_shift, N, keys[0], idx[0], pay, d_occ);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, (pre + "emit").c_str()));
  int occ_tab[MC_KEY_DIGITS * 256];
  e = hipMemcpyAsync(occ_tab, d_occ, sizeof(occ_tab), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (behind it `up2` and `stage` may go)
  if (e != hipSuccess) return ctx->hip_fail(e, (pre + "emit").c_str());
  if (timing) ctx->oc_ms[1] += oc_ms_since(t0), t0 = std::chrono::steady_clock::now();
  int cur = 0;
  rc = mc_sort(ctx, occ_tab, keys, idx, N, n_maps, d_cstart, cs2.data(), d_hist, &cur, nullptr, nullptr);
  if (rc != FLVIS_OK) return rc;
  if (timing) {
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, (pre + "sort").c_str());
    ctx->oc_ms[2] += oc_ms_since(t0), t0 = std::chrono::steady_clock::now();
  }
  // ---- the reduction; the observations go to the sort's other buffers
  const OcSorted so{keys[cur], idx[cur], pay, d_cstart, n_maps, N};
  k_oc_flags<<<nblk, OC_T, 0, st>>>(so, d_bo, d_bv, d_bsum);
  k_oc_scan<<<1, 1024, 0, st>>>(d_bo, nblk, d_bo);
  k_oc_scan<<<1, 1024, 0, st>>>(d_bv, nblk, d_bv);
  k_oc_obs<<<nblk, OC_T, 0, st>>>(so, d_bo, d_bv, d_bsum, nblk, keys[cur ^ 1], idx[cur ^ 1], ovox);
  k_oc_map_rank<<<NM1, OC_T, 0, st>>>(so, d_bv, d_bo, nblk, d_mv);
  OC_LAUNCH(ctx, (pre + "reduce").c_str());
  std::vector<int> mv((size_t)NM1 + 1);
  e = hipMemcpyAsync(mv.data(), d_mv, sizeof(int) * mv.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, (pre + "reduce").c_str());
  for (int m = 0; m < n_maps; m++) h_n_out[m] = (int64_t)mv[m + 1] - mv[m];
  OcOut out{0, nullptr, nullptr, nullptr};
  rc = hook(h_n_out, &out);
  if (rc != FLVIS_OK) return rc;
  const int n_obs = mv[(size_t)NM1];
  if (out.out_cap > 0 && n_obs > 0) {
    const OcApply a{keys[cur ^ 1], idx[cur ^ 1], ovox,       d_mv,        d_cstart,   d_nprior,   prior.d_l, prior.cap, n_maps, n_obs,
                    out.out_cap,   occ->l_hit,   occ->l_miss, occ->l_min, occ->l_max, leaf,       out.d_key, out.d_l,   out.d_xyz};
    k_oc_apply<<<(n_obs + OC_T - 1) / OC_T, OC_T, 0, st>>>(a);
    OC_LAUNCH(ctx, (pre + "apply").c_str());
  }
  if (timing) {
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, (pre + "apply").c_str());
    ctx->oc_ms[3] += oc_ms_since(t0);
  }
  return FLVIS_OK;
}

int oc_check_public(int n_img, int w, int h, int n_maps, const int* h_map_ptr, const int* h_range2, const double* h_cam5,
                    const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int prior_cap, const int64_t* h_n_prior,
                    int out_cap, std::string& why) {
  int rc = flvis_depth_cloud_check(n_img, w, h, n_maps, h_map_ptr, h_range2, h_cam5, prm, leaf, 1, out_cap);
  if (rc != FLVIS_OK) return why = "the dense cloud's check of the images, ranges, cameras, sampling, leaf and out_cap failed (flvis_depth_cloud_check)", rc;
  rc = oc_check_values(leaf, occ, &why);
  if (rc != FLVIS_OK) return rc;
  if (prior_cap < 0) return why = "prior_cap < 0", FLVIS_ERR_INVALID_ARG;
  for (int m = 0; h_n_prior && m < n_maps; m++)
    if (h_n_prior[m] < 0 || h_n_prior[m] > prior_cap) return why = "h_n_prior[" + std::to_string(m) + "] is outside [0, prior_cap]", FLVIS_ERR_INVALID_ARG;
  return FLVIS_OK;
}

void oc_reset_stats(flvis_ctx* ctx) {
  memset(ctx->oc_ms, 0, sizeof(ctx->oc_ms));
  memset(ctx->oc_stats, 0, sizeof(ctx->oc_stats));
}

// flvis_keyframe_log_occupancy: the refusals, then (unless check_only) the call
int kfl_occupancy(flvis_ctx* ctx, const char* what, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                  double leaf, const flvis_occupancy_params* occ, int64_t max_records, const OcOut& out, int64_t* h_n_out, int64_t* h_n_rays,
                  int64_t* h_n_dropped, int* h_n_batches, bool check_only) {
  const std::string pre = std::string(what) + ": ";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + m); };
  Pipeline* pl = ctx->pipe;
  if (!pl) return bad("no tracker (flvis_tracker_create)");
  if (pl->cfg.cam_type != CAM_DEPTH) return ctx->fail(FLVIS_ERR_CONFIG, pre + "the tracker's rig has no depth image");
  if (pl->kfl.cap <= 0) return bad("the keyframe log is off (flvis_keyframe_log_enable)");
  if (n <= 0 || !h_stream || !h_n_out || !prm) return bad("bad stream list, or a NULL prm or h_n_out");
  std::vector<double> cam5(5 * (size_t)n);
  for (int c = 0; c < n; c++) {
    const int s = h_stream[c];
    if (s < 0 || s >= pl->S) return bad("stream out of range");
    if (h_slice2 && (h_slice2[2 * c] < 0 || h_slice2[2 * c + 1] < 0)) return bad("a negative slice");
    const flvis_cfg& g = pl->cfgs[s];
    const double v[5] = {g.P0[0], g.P0[5], g.P0[2], g.P0[6], g.depth_factor};
    memcpy(&cam5[5 * (size_t)c], v, sizeof(v));
  }
  std::string why;
  int rc = dc_check_sampling(pl->kfl.w, pl->kfl.h, prm, n, cam5.data(), &why);
  if (rc == FLVIS_OK) rc = oc_check_values(leaf, occ, &why);
  if (rc != FLVIS_OK) return ctx->fail(rc, pre + why);
  if (max_records < 0 || out.out_cap < 0 || ((!out.d_key || !out.d_l) && out.out_cap > 0))
    return bad("max_records >= 0 and out_cap >= 0 with rows to write to");
  if (check_only) return FLVIS_OK;
  KfLogRec rec{};
  int S = 0, cam_type = 0;
  std::vector<long long> logged, dropped;
  rc = kf_log_settle(ctx, what, rec, S, cam_type, logged, dropped);
  if (rc != FLVIS_OK) return rc;
  std::vector<int> eptr((size_t)n + 1), img, cam, item_stream, item_entry;
  for (int c = 0; c < n; c++) {
    const int s = h_stream[c];
    eptr[c] = (int)img.size();
    const long long first = h_slice2 ? h_slice2[2 * c] : 0, last = h_slice2 ? std::min(logged[s], first + h_slice2[2 * c + 1]) : logged[s];
    for (long long k = first; k < last; k++) {
      if (img.size() >= (size_t)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 listed keyframes or more");
      img.push_back((int)((long long)s * rec.cap + k)), cam.push_back(c), item_stream.push_back(s), item_entry.push_back((int)k);
    }
  }
  eptr[n] = (int)img.size();
  static_assert(offsetof(KeyFrameDev, T_c_w) % 8 == 0 && sizeof(KeyFrameDev) % 8 == 0, "the logged poses are read in place as rows of doubles");
  const double* d_pose = reinterpret_cast<const double*>(reinterpret_cast<const char*>(rec.kf) + offsetof(KeyFrameDev, T_c_w));
  const OcLists L{reinterpret_cast<const uint16_t*>(rec.img1), rec.w, rec.h, d_pose, sizeof(KeyFrameDev) / 8, n, eptr.data(), img.data(), img.data(),
                  cam.data(), n, cam5.data()};
  return oc_batched(ctx, what, L, prm, leaf, occ, max_records, out, h_n_out, h_n_rays, h_n_dropped, h_n_batches, [&](int e) {
    return "entry " + std::to_string(item_entry[e]) + " of stream " + std::to_string(item_stream[e]);
  });
}

}  // namespace

namespace flvis {

int oc_check_values(double leaf, const flvis_occupancy_params* occ, std::string* why) {
  std::string m;
  int rc = FLVIS_OK;
  if (!(leaf > 0) || !std::isfinite(leaf)) rc = FLVIS_ERR_INVALID_ARG, m = "leaf must be finite and > 0";
  else if (!occ) rc = FLVIS_ERR_INVALID_ARG, m = "NULL occupancy params";
  else if (!(std::isfinite(occ->l_hit) && std::isfinite(occ->l_miss) && std::isfinite(occ->l_min) && std::isfinite(occ->l_max)) ||
           !(occ->l_hit > 0) || !(occ->l_miss < 0) || !(occ->l_min < 0) || !(occ->l_max > 0))
    rc = FLVIS_ERR_INVALID_ARG, m = "the log-odds must be finite with l_hit > 0, l_miss < 0, l_min < 0 and l_max > 0";
  if (why) *why = m;
  return rc;
}

int oc_batched(flvis_ctx* ctx, const char* what, const OcLists& L, const flvis_depth_cloud_params* prm, double leaf,
               const flvis_occupancy_params* occ, int64_t max_records, const OcOut& out, int64_t* h_n_out, int64_t* h_n_rays,
               int64_t* h_n_dropped, int* h_n_batches, const std::function<std::string(int)>& name_of) {
  const std::string pre = std::string(what) + ": ";
  const int n = L.n_maps, R = L.eptr[n];
  const long long cap_rec = max_records == 0 ? OC_DEFAULT_MAX_RECORDS : (long long)max_records;
  oc_reset_stats(ctx);
  for (int m = 0; m < n; m++) {
    h_n_out[m] = 0;
    if (h_n_rays) h_n_rays[m] = 0;
    if (h_n_dropped) h_n_dropped[m] = 0;
  }
  if (h_n_batches) *h_n_batches = 0;
  if (R == 0) return FLVIS_OK;
  // ---- the scans' record counts: one count pass over every listed image, read once
  std::vector<long long> rec;
  const OcPrior none{nullptr, nullptr, 0, nullptr};
  OcCounted counted{nullptr, 0, 0};
  int rc = oc_core(ctx, what, L, prm, leaf, occ, none, nullptr, h_n_out, nullptr, nullptr, &rec, &counted);
  if (rc != FLVIS_OK) return rc;
  std::vector<int> cut{0};  // batch b: the items cut[b] .. cut[b + 1] - 1
  long long acc = 0;
  for (int e = 0; e < R; e++) {
    if (rec[e] > cap_rec)
      return ctx->fail(FLVIS_ERR_CAPACITY, pre + name_of(e) + " alone makes " + std::to_string(rec[e]) + " records, above max_records");
    if (acc + rec[e] > cap_rec) cut.push_back(e), acc = 0;
    acc += rec[e];
  }
  cut.push_back(R);
  const int n_batches = (int)cut.size() - 1;
  // ---- the carried map: keys [n][cap] | values [n][cap] in "oc_carry0" / "oc_carry1", written by one batch and read by the next
  int64_t* carry_key[2] = {nullptr, nullptr};
  float* carry_l[2] = {nullptr, nullptr};
  int carry_cap[2] = {0, 0};
  std::vector<int64_t> n_prior((size_t)n, 0);
  std::vector<int> eptr((size_t)n + 1);
  int cur = 0;
  for (int b = 0; b < n_batches; b++) {
    const int a0 = cut[b], a1 = cut[b + 1];
    for (int m = 0; m <= n; m++) eptr[m] = std::min(std::max(L.eptr[m], a0), a1) - a0;
    OcLists B = L;
    B.eptr = eptr.data(), B.img = L.img + a0, B.pose = L.pose + a0, B.cam = L.cam + a0;
    const bool last = b == n_batches - 1;
    const int to = cur ^ 1;
    const OcPrior prior{b ? carry_key[cur] : nullptr, b ? carry_l[cur] : nullptr, b ? carry_cap[cur] : 0, b ? n_prior.data() : nullptr};
    const OcOutHook hook = [&](const int64_t* n_out, OcOut* o) -> int {
      if (last) return *o = out, FLVIS_OK;
      int64_t need = 1;
      for (int m = 0; m < n; m++) need = std::max(need, n_out[m]);
      const size_t rows = (size_t)n * (size_t)need;
      void* p = ctx->scratch(to ? "oc_carry1" : "oc_carry0", rows * (sizeof(int64_t) + sizeof(float)));
      if (!p) {
        (void)hipGetLastError();
        return ctx->fail(FLVIS_ERR_HIP, pre + "device allocation failed");
      }
      carry_key[to] = (int64_t*)p, carry_l[to] = (float*)(carry_key[to] + rows), carry_cap[to] = (int)need;
      *o = OcOut{(int)need, carry_key[to], carry_l[to], nullptr};
      return FLVIS_OK;
    };
    counted.first_item = a0;
    rc = oc_core(ctx, what, B, prm, leaf, occ, prior, hook, h_n_out, h_n_rays, h_n_dropped, nullptr, nullptr, counted.d ? &counted : nullptr);
    if (rc != FLVIS_OK) return rc;
    for (int m = 0; m < n; m++) n_prior[m] = h_n_out[m];
    cur = to;
  }
  ctx->oc_stats[2] = n_batches;
  if (h_n_batches) *h_n_batches = n_batches;
  return FLVIS_OK;
}

int oc_host_alloc(flvis_ctx* ctx, const char* what, int n, int out_cap, bool xyz, OcOut* out) {
  *out = OcOut{out_cap, nullptr, nullptr, nullptr};
  if (out_cap <= 0 || n <= 0) return FLVIS_OK;
  const size_t rows = (size_t)n * (size_t)out_cap;
  void* p = ctx->scratch("oc_host_rows", rows * (sizeof(int64_t) + 4 * sizeof(float)));
  if (!p) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  out->d_key = (int64_t*)p;
  out->d_l = (float*)(out->d_key + rows);
  out->d_xyz = xyz ? out->d_l + rows : nullptr;
  return FLVIS_OK;
}

int oc_host_fetch(flvis_ctx* ctx, const char* what, int n, const OcOut& dev, const int64_t* h_n_out, int64_t* h_key, float* h_l, float* h_xyz) {
  hipError_t e = hipSuccess;
  bool any = false;
  for (int g = 0; g < n && e == hipSuccess; g++) {
    const size_t k = (size_t)std::min<int64_t>(h_n_out[g], dev.out_cap), at = (size_t)g * (size_t)dev.out_cap;
    if (k == 0) continue;
    any = true;
    e = hipMemcpyAsync(h_key + at, dev.d_key + at, sizeof(int64_t) * k, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_l + at, dev.d_l + at, sizeof(float) * k, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && h_xyz) e = hipMemcpyAsync(h_xyz + 3 * at, dev.d_xyz + 3 * at, sizeof(float) * 3 * k, hipMemcpyDeviceToHost, ctx->stream);
  }
  if (any || e != hipSuccess) {
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}

}  // namespace flvis

extern "C" {

void flvis_occupancy_params_default(flvis_occupancy_params* p) {
  if (!p) return;
  p->l_hit = 0.85f, p->l_miss = -0.4f, p->l_min = -2.0f, p->l_max = 3.5f;
}

int flvis_hip_occupancy_info(int* h_info4) {
  if (!h_info4) return FLVIS_ERR_INVALID_ARG;
  h_info4[0] = OC_T;
  h_info4[1] = OC_BYTES_PER_RECORD;
  h_info4[2] = OC_BYTES_PER_RAY;
  h_info4[3] = OC_BYTES_PER_IMAGE;
  return FLVIS_OK;
}

int flvis_occupancy_check(int n_img, int w, int h, int n_maps, const int* h_map_ptr, const int* h_range2, const double* h_cam5,
                          const flvis_depth_cloud_params* prm, double leaf, const flvis_occupancy_params* occ, int prior_cap,
                          const int64_t* h_n_prior, int out_cap) {
  std::string why;
  return oc_check_public(n_img, w, h, n_maps, h_map_ptr, h_range2, h_cam5, prm, leaf, occ, prior_cap, h_n_prior, out_cap, why);
}

int flvis_hip_occupancy(flvis_ctx* ctx, const uint16_t* d_depth, const double* d_T_c_w7, int n_img, int w, int h, int n_maps, const int* h_map_ptr,
                        const int* h_range2, const double* h_cam5, const flvis_depth_cloud_params* prm, double leaf,
                        const flvis_occupancy_params* occ, const int64_t* d_prior_key, const float* d_prior_l, int prior_cap,
                        const int64_t* h_n_prior, int out_cap, int64_t* d_key, float* d_l, float* d_xyz, int64_t* h_n_out, int64_t* h_n_rays,
                        int64_t* h_n_dropped) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, "occupancy: " + m); };
  if (!d_depth || !d_T_c_w7 || !h_n_out) return bad("a NULL required pointer");
  if ((!d_key || !d_l) && out_cap > 0) return bad("NULL d_key or d_l with out_cap > 0");
  std::string why;
  int rc = oc_check_public(n_img, w, h, n_maps, h_map_ptr, h_range2, h_cam5, prm, leaf, occ, prior_cap, h_n_prior, out_cap, why);
  if (rc != FLVIS_OK) return ctx->fail(rc, "occupancy: " + why);
  bool any_prior = false;
  for (int m = 0; h_n_prior && m < n_maps; m++) any_prior = any_prior || h_n_prior[m] > 0;
  if (any_prior && (!d_prior_key || !d_prior_l)) return bad("a NULL prior table with a non-zero count");
  if (any_prior && out_cap > 0) {  // the prior is read while the rows are written
    const size_t pr = (size_t)n_maps * (size_t)prior_cap, orows = (size_t)n_maps * (size_t)out_cap;
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
      const char *x = (const char*)a, *y = (const char*)b;
      return a && b && x < y + nb && y < x + na;
    };
    const void* outs[3] = {d_key, d_l, d_xyz};
    const size_t out_bytes[3] = {8 * orows, 4 * orows, 12 * orows};
    for (int k = 0; k < 3; k++)
      if (overlap(d_prior_key, 8 * pr, outs[k], out_bytes[k]) || overlap(d_prior_l, 4 * pr, outs[k], out_bytes[k]))
        return bad("the prior may not alias the output");
  }
  std::vector<int> eptr((size_t)n_maps + 1), img, cam;
  for (int m = 0; m < n_maps; m++) {
    eptr[m] = (int)img.size();
    for (int r = h_map_ptr[m]; r < h_map_ptr[m + 1]; r++)
      for (int k = 0; k < h_range2[2 * r + 1]; k++) {
        if (img.size() >= (size_t)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, "occupancy: the call lists 2^31 images or more");
        img.push_back(h_range2[2 * r] + k), cam.push_back(r);
      }
  }
  eptr[n_maps] = (int)img.size();
  oc_reset_stats(ctx);
  for (int m = 0; m < n_maps; m++) {
    h_n_out[m] = 0;
    if (h_n_rays) h_n_rays[m] = 0;
    if (h_n_dropped) h_n_dropped[m] = 0;
  }
  const OcLists L{d_depth, w, h, d_T_c_w7, 7, n_maps, eptr.data(), img.data(), img.data(), cam.data(), h_map_ptr[n_maps], h_cam5};
  const OcPrior prior{d_prior_key, d_prior_l, prior_cap, any_prior ? h_n_prior : nullptr};
  const OcOut out{out_cap, d_key, d_l, d_xyz};
  rc = oc_core(ctx, "occupancy", L, prm, leaf, occ, prior, [&](const int64_t*, OcOut* o) -> int { return *o = out, FLVIS_OK; }, h_n_out, h_n_rays,
               h_n_dropped, nullptr);
  if (rc == FLVIS_OK) ctx->oc_stats[2] = 1;
  return rc;
}

int flvis_hip_occupancy_stats(flvis_ctx* ctx, int64_t* h_stats4, double* h_ms4) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (h_stats4) memcpy(h_stats4, ctx->oc_stats, sizeof(ctx->oc_stats));
  if (h_ms4) memcpy(h_ms4, ctx->oc_ms, sizeof(ctx->oc_ms));
  return FLVIS_OK;
}

int flvis_keyframe_log_occupancy(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm, double leaf,
                                 const flvis_occupancy_params* occ, int64_t max_records, int out_cap, int64_t* d_key, float* d_l, float* d_xyz,
                                 int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped, int* h_n_batches) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  return kfl_occupancy(ctx, "keyframe_log_occupancy", n, h_stream, h_slice2, prm, leaf, occ, max_records, OcOut{out_cap, d_key, d_l, d_xyz}, h_n_out,
                       h_n_rays, h_n_dropped, h_n_batches, false);
}

int flvis_keyframe_log_occupancy_host(flvis_ctx* ctx, int n, const int* h_stream, const int* h_slice2, const flvis_depth_cloud_params* prm,
                                      double leaf, const flvis_occupancy_params* occ, int64_t max_records, int out_cap, int64_t* h_key, float* h_l,
                                      float* h_xyz, int64_t* h_n_out, int64_t* h_n_rays, int64_t* h_n_dropped, int* h_n_batches) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  const char* what = "keyframe_log_occupancy_host";
  int rc = kfl_occupancy(ctx, what, n, h_stream, h_slice2, prm, leaf, occ, max_records, OcOut{out_cap, h_key, h_l, h_xyz}, h_n_out, h_n_rays,
                         h_n_dropped, h_n_batches, true);
  if (rc != FLVIS_OK) return rc;
  OcOut dev;
  rc = flvis::oc_host_alloc(ctx, what, n, out_cap, h_xyz != nullptr, &dev);
  if (rc != FLVIS_OK) return rc;
  rc = kfl_occupancy(ctx, what, n, h_stream, h_slice2, prm, leaf, occ, max_records, dev, h_n_out, h_n_rays, h_n_dropped, h_n_batches, false);
  if (rc != FLVIS_OK) return rc;
  return flvis::oc_host_fetch(ctx, what, n, dev, h_n_out, h_key, h_l, h_xyz);
}

}  // extern "C"
