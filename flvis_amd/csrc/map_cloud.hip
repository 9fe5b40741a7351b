// flvis_amd: a map's landmarks as one voxel-filtered point cloud (flvis_hip_voxel_cloud; include/flvis_hip.h has the definition).
//
// The reference's LocalMapNodeletClass publishes /map_cloud (vo_localmap.cpp:335-377, :458-461) and sets up a pcl::VoxelGrid of 0.08 m that it
// never runs.  The local map's own cloud is flvis_local_map_cloud (lm_cloud.hip), which ends in this call; the loop closer's database goes
// through it as flvis_loop_closer_map_cloud.  The radix passes (mc_sort) and the call with landmark ids (mc_voxel_cloud) are shared with
// lm_cloud.hip through map_cloud.hpp.  The call is cut in three so that the dense cloud (depth_cloud.hip) can bring its own front end:
// the front end (counts, offsets, keys: here k_mc_counts .. k_mc_keys), mc_work (the workspace of the call's points) and mc_tail
// (everything from the byte table and the sort on).  A point enters the workspace through mc_put (map_cloud.hpp) in both front ends.
//
// Steps of one call (every cloud of the call goes through each of them together):
//   k_mc_counts, k_mc_scan     the listed rows' clamped counts and their running sum: where each row's points start in canonical order
//   k_mc_keys                  one workgroup per listed row: map-frame point (fp64, stored), voxel key, and which values each key byte takes
//   k_mc_hist / k_mc_scan_rows / k_mc_scan / k_mc_scatter   one stable LSD radix pass over an 8-bit digit of (cloud | key), payload = the canonical index.
//                              A digit that takes one value over the whole call is skipped (the host reads k_mc_keys' byte table).
//   k_mc_bounds                per cloud: where its dropped points (top key bit) begin
//   k_mc_flags / k_mc_scan / k_mc_cloud_rank   which sorted positions start an output row, and every cloud's first output rank
//   k_mc_emit                  one lane per output row adds the voxel's points one after another in canonical order (the stable sort left
//                              them in it), divides and rounds to float
// Stability is what the definition needs: equal keys keep the order of their canonical indices through every pass, so no pass ever looks at
// the index.  Inside a workgroup the order comes from the layout -- wave w owns a contiguous quarter of the tile, round r of a wave 64
// consecutive elements -- and from ranking equal digits inside a wave with eight ballots.
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
#include "dev_math.hpp"
#include "map_cloud.hpp"

namespace {

using namespace flvis;

constexpr int MC_T = 256;                    // workgroup of the sort kernels: four waves
constexpr int MC_ITEMS = 16;                 // elements per lane and tile (keys and indices stay in registers between count and scatter)
constexpr int MC_TILE = MC_T * MC_ITEMS;     // 4096: the sort tile (flvis_hip_voxel_cloud_info)
constexpr int MC_WAVE_SPAN = 64 * MC_ITEMS;  // a wave's contiguous part of a tile
constexpr int MC_MAX_BLK = 2048;             // sort workgroups per pass at most (8 per CU): bounds a row of the histogram table
constexpr int MC_RB = 1024;                  // sorted positions per workgroup of the output kernels
constexpr int MC_BYTES_PER_POINT = 2 * 8 + 2 * 4 + 24;  // two key buffers, two index buffers, the map-frame point
constexpr int MC_BYTES_PER_ROW = 8 + 2 * 4;             // running sum, row, count (+ 24 per cloud)

#define MC_LAUNCH(c, what)                                   \
  do {                                                       \
    hipError_t e__ = hipGetLastError();                      \
    if (e__ != hipSuccess) return (c)->hip_fail(e__, what);  \
  } while (0)

// the last cloud c with cstart[c] <= i (empty clouds share their start with the next one: a position belongs to the one that holds it)
FD int mc_cloud_of(const int* __restrict__ cstart, int n_clouds, uint32_t i) {
  int lo = 0, hi = n_clouds;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((uint32_t)cstart[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_mc_counts(const int* __restrict__ rows, int n_entries, const int* __restrict__ d_count, int cap,
                                                   int* __restrict__ cnt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n_entries) cnt[e] = min(max(d_count[rows[e]], 0), cap);
}

// out[i] = in[0] + .. + in[i - 1] for i in 0 .. n (n + 1 values; in == out is allowed when the types match).  One workgroup: the tables it
// walks are small next to the points (a count per listed row, the 256 digit totals of a pass, a count per MC_RB sorted positions).
template <class Tin, class Tout>
__global__ __launch_bounds__(1024) void k_mc_scan(const Tin* in, long long n, Tout* out) {
  __shared__ Tout part[1024];
  const int t = threadIdx.x;
  const long long per = (n + 1023) / 1024, lo = min(n, t * per), hi = min(n, lo + per);
  Tout s = 0;
  for (long long i = lo; i < hi; i++) s += (Tout)in[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    Tout a = 0;
    for (int k = 0; k < 1024; k++) {
      const Tout v = part[k];
      part[k] = a;
      a += v;
    }
    out[n] = a;
  }
  __syncthreads();
  Tout a = part[t];
  for (long long i = lo; i < hi; i++) {
    const Tout v = (Tout)in[i];
    out[i] = a;
    a += v;
  }
}

// one workgroup per digit d: hist[d][0 .. nblk) becomes its running sum inside the row, tot[d] the row's total (the digits' own running
// sum is a 256-value k_mc_scan)
__global__ __launch_bounds__(1024) void k_mc_scan_rows(uint32_t* hist, int nblk, uint32_t* __restrict__ tot) {
  __shared__ uint32_t part[1024];
  const int t = threadIdx.x;
  uint32_t* const row = hist + (size_t)blockIdx.x * nblk;
  const int per = (nblk + 1023) / 1024, lo = min(nblk, t * per), hi = min(nblk, lo + per);
  uint32_t s = 0;
  for (int i = lo; i < hi; i++) s += row[i];
  part[t] = s;
  __syncthreads();
  for (int k = 1; k < 1024; k <<= 1) {
    const uint32_t v = t >= k ? part[t - k] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t a = part[t] - s;
  for (int i = lo; i < hi; i++) {
    const uint32_t v = row[i];
    row[i] = a;
    a += v;
  }
  if (t == 1023) tot[blockIdx.x] = part[1023];
}

// the clouds' first canonical indices from the rows' running sums (64-bit for the host's capacity check, 32-bit for the kernels)
__global__ __launch_bounds__(256) void k_mc_cloud_starts(const long long* __restrict__ off, const int* __restrict__ eptr, int n_clouds,
                                                         long long* __restrict__ cs64, int* __restrict__ cstart) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > n_clouds) return;
  const long long v = off[eptr[c]];
  cs64[c] = v;
  cstart[c] = (int)min(v, (long long)INT_MAX);
}

// one workgroup per listed row
__global__ __launch_bounds__(256) void k_mc_keys(const int* __restrict__ rows, const int* __restrict__ cnt, const long long* __restrict__ off,
                                                 const double* __restrict__ p3, const double* __restrict__ T7, int cap, double leaf,
                                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, double* __restrict__ pts,
                                                 int* __restrict__ occ, const long long* __restrict__ id_rows, long long* __restrict__ idc) {
  __shared__ uint8_t seen[MC_KEY_DIGITS * 256];
  const int tid = threadIdx.x;
  const int e = blockIdx.x, n = cnt[e];
  if (n == 0) return;
  for (int i = tid; i < MC_KEY_DIGITS * 256; i += 256) seen[i] = 0;
  __syncthreads();
  const int row = rows[e];
  const size_t base = (size_t)off[e];
  const SE3d T = load_pose7(T7 + 7 * (size_t)row);
  const Q4 qi = q_conj(T.q);
  for (int lm = tid; lm < n; lm += 256) {
    const double* s = p3 + ((size_t)row * cap + lm) * 3;
    const size_t i = base + lm;
    mc_put(T, qi, V3{s[0], s[1], s[2]}, leaf, i, keys, idx, pts, seen);
    if (id_rows) idc[i] = id_rows[(size_t)row * cap + lm];  // (mc_voxel_cloud: the points' ids, in canonical order like the points)
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < MC_KEY_DIGITS; d++)
    if (seen[d * 256 + tid]) occ[d * 256 + tid] = 1;
}

struct McDigit {
  int shift, by_cloud, n_clouds;
  const int* cstart;
};
FD uint32_t mc_digit(const McDigit& g, uint64_t key, uint32_t idx) {
  return g.by_cloud ? (((uint32_t)mc_cloud_of(g.cstart, g.n_clouds, idx) >> g.shift) & 255u) : ((uint32_t)(key >> g.shift) & 255u);
}

// workgroup b sorts the tiles b * tiles_per_blk ..; hist[digit][b] = how many of its elements carry the digit
__global__ __launch_bounds__(MC_T) void k_mc_hist(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, int n, int tiles_per_blk,
                                                  McDigit g, uint32_t* __restrict__ hist, int nblk) {
  __shared__ uint32_t h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * tiles_per_blk * MC_TILE, hi = min((long long)n, lo + (long long)tiles_per_blk * MC_TILE);
  for (long long i = lo + tid; i < hi; i += MC_T) atomicAdd(&h[mc_digit(g, keys[i], g.by_cloud ? idx[i] : 0u)], 1u);
  __syncthreads();
  hist[(size_t)tid * nblk + blockIdx.x] = h[tid];
}

// offs: k_mc_hist's table after k_mc_scan_rows, dbase: the digits' first positions: workgroup b's first element with digit d goes to
// dbase[d] + offs[d][b]
__global__ __launch_bounds__(MC_T) void k_mc_scatter(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, int n, int tiles_per_blk,
                                                     McDigit g, const uint32_t* __restrict__ offs, const uint32_t* __restrict__ dbase, int nblk,
                                                     uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out) {
  __shared__ uint32_t cnt[MC_T / 64][256];
  __shared__ uint32_t run_s[MC_T / 64][256];
  __shared__ uint32_t gbase[256];
  volatile uint32_t(*run)[256] = run_s;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  gbase[tid] = dbase[tid] + offs[(size_t)tid * nblk + blockIdx.x];
  for (int t = 0; t < tiles_per_blk; t++) {
    const long long tile0 = ((long long)blockIdx.x * tiles_per_blk + t) * MC_TILE;
    if (tile0 >= n) break;  // (uniform over the workgroup)
#pragma unroll
    for (int k = 0; k < MC_T / 64; k++) cnt[k][tid] = 0;
    __syncthreads();
    uint64_t kk[MC_ITEMS];
    uint32_t id[MC_ITEMS], dg[MC_ITEMS];
#pragma unroll
    for (int r = 0; r < MC_ITEMS; r++) {
      const long long i = tile0 + (long long)w * MC_WAVE_SPAN + r * 64 + lane;
      dg[r] = 256;  // no element
      kk[r] = 0, id[r] = 0;
      if (i < n) {
        kk[r] = keys[i], id[r] = idx[i];
        dg[r] = mc_digit(g, kk[r], id[r]);
        atomicAdd(&cnt[w][dg[r]], 1u);
      }
    }
    __syncthreads();
    {  // lane `tid` owns digit `tid`: the waves' first positions, in wave order
      uint32_t b = gbase[tid];
#pragma unroll
      for (int k = 0; k < MC_T / 64; k++) {
        run_s[k][tid] = b;
        b += cnt[k][tid];
      }
      gbase[tid] = b;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MC_ITEMS; r++) {
      const bool valid = dg[r] < 256;
      uint64_t m = __ballot(valid);  // the lanes of this round that carry my digit
#pragma unroll
      for (int b = 0; b < 8; b++) {
        const bool bit = (dg[r] >> b) & 1;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
      }
      uint32_t prior = 0;
      const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1));
      if (valid) {
        prior = run[w][dg[r]];
        const uint32_t pos = prior + rank;
        if (pos < (uint32_t)n) keys_out[pos] = kk[r], idx_out[pos] = id[r];
      }
      __builtin_amdgcn_wave_barrier();  // every lane has read the wave's counter before the digit's first lane moves it on
      if (valid && rank == 0) run[w][dg[r]] = prior + (uint32_t)__popcll(m);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
}

// kend[c]: the first sorted position of cloud c that holds a dropped point (the cloud's end when it has none)
__global__ __launch_bounds__(256) void k_mc_bounds(const uint64_t* __restrict__ K, const int* __restrict__ cstart, int n_clouds, int* __restrict__ kend) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_clouds) return;
  int lo = cstart[c], hi = cstart[c + 1];
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (K[mid] >> 63) hi = mid;
    else lo = mid + 1;
  }
  kend[c] = lo;
}

struct McOut {
  const uint64_t* K;
  const int *cstart, *kend;
  int n_clouds, raw, min_points;
};
// does sorted position i start an output row?  c: its cloud
FD bool mc_emits(const McOut& o, int i, int& c) {
  c = mc_cloud_of(o.cstart, o.n_clouds, (uint32_t)i);
  const int end = o.kend[c];
  if (i >= end) return false;
  if (o.raw) return true;
  const uint64_t k = o.K[i];
  if (i > o.cstart[c] && o.K[i - 1] == k) return false;
  const long long last = (long long)i + o.min_points - 1;  // (sorted: the voxel holds min_points points iff this one is still in it)
  return last < end && o.K[last] == k;
}

__global__ __launch_bounds__(256) void k_mc_flags(McOut o, int n, int* __restrict__ bsum) {
  __shared__ int s;
  if (threadIdx.x == 0) s = 0;
  __syncthreads();
  int cnt = 0, c;
  const long long lo = (long long)blockIdx.x * MC_RB, hi = min((long long)n, lo + MC_RB);
  for (long long i = lo + threadIdx.x; i < hi; i += 256) cnt += mc_emits(o, (int)i, c) ? 1 : 0;
  if (cnt) atomicAdd(&s, cnt);
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// cg[b]: how many output rows start before cloud b (b == n_clouds: in the whole call); bpre: k_mc_flags' counts after the scan
__global__ __launch_bounds__(256) void k_mc_cloud_rank(McOut o, int n, const int* __restrict__ bpre, int* __restrict__ cg) {
  __shared__ int s;
  if (threadIdx.x == 0) s = 0;
  __syncthreads();
  const int pos = o.cstart[blockIdx.x];  // (cstart[n_clouds] == n)
  const int chunk = pos / MC_RB;
  int cnt = 0, c;
  for (int i = chunk * MC_RB + threadIdx.x; i < pos; i += 256) cnt += mc_emits(o, i, c) ? 1 : 0;
  if (cnt) atomicAdd(&s, cnt);
  __syncthreads();
  if (threadIdx.x == 0) cg[blockIdx.x] = bpre[chunk] + s;
}

__global__ __launch_bounds__(256) void k_mc_emit(McOut o, int n, const uint32_t* __restrict__ I, const double* __restrict__ pts,
                                                 const int* __restrict__ bpre, const int* __restrict__ cg, int out_cap, float* __restrict__ xyz,
                                                 int* __restrict__ npts, const long long* __restrict__ idc, long long* __restrict__ id_out) {
  __shared__ int sc[256];
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * MC_RB + tid * (MC_RB / 256);
  bool f[MC_RB / 256];
  int c[MC_RB / 256], loc = 0;
#pragma unroll
  for (int k = 0; k < MC_RB / 256; k++) {
    c[k] = 0;
    f[k] = base + k < n && mc_emits(o, (int)(base + k), c[k]);
    loc += f[k] ? 1 : 0;
  }
  sc[tid] = loc;
  __syncthreads();
  for (int s = 1; s < 256; s <<= 1) {
    const int v = tid >= s ? sc[tid - s] : 0;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  int g = bpre[blockIdx.x] + sc[tid] - loc;
#pragma unroll
  for (int k = 0; k < MC_RB / 256; k++) {
    if (!f[k]) continue;
    const int row = g - cg[c[k]];
    g++;
    if (row >= out_cap) continue;
    const int i = (int)(base + k), end = o.kend[c[k]];
    const uint64_t key = o.K[i];
    const double* p = pts + 3 * (size_t)I[i];
    double sx = p[0], sy = p[1], sz = p[2];
    int cnt = 1;
    if (!o.raw)
      for (int j = i + 1; j < end && o.K[j] == key; j++) {  // one after another, in canonical order: the definition allows no tree
        p = pts + 3 * (size_t)I[j];
        sx += p[0], sy += p[1], sz += p[2];
        cnt++;
      }
    const size_t at = (size_t)c[k] * out_cap + row;
    const double d = (double)cnt;
    xyz[3 * at] = (float)(sx / d), xyz[3 * at + 1] = (float)(sy / d), xyz[3 * at + 2] = (float)(sz / d);
    if (npts) npts[at] = cnt;
    if (id_out) id_out[at] = idc[I[i]];  // (raw rows only: mc_voxel_cloud)
  }
}

int mc_check(int n_rows, int cap, int n_clouds, const int* h_cloud_ptr, const int* h_range2, double leaf, int min_points, int out_cap,
             std::string& why) {
  if (n_rows <= 0 || cap <= 0) return why = "n_rows and cap must be positive", FLVIS_ERR_INVALID_ARG;
  if (n_clouds <= 0) return why = "n_clouds <= 0", FLVIS_ERR_INVALID_ARG;
  if (!h_cloud_ptr || !h_range2) return why = "a NULL table", FLVIS_ERR_INVALID_ARG;
  if (!(leaf >= 0) || !std::isfinite(leaf)) return why = "leaf must be finite and >= 0", FLVIS_ERR_INVALID_ARG;
  if (min_points < 1) return why = "min_points < 1", FLVIS_ERR_INVALID_ARG;
  if (out_cap < 0) return why = "out_cap < 0", FLVIS_ERR_INVALID_ARG;
  if (h_cloud_ptr[0] != 0) return why = "h_cloud_ptr must start at 0", FLVIS_ERR_INVALID_ARG;
  for (int c = 0; c < n_clouds; c++)
    if (h_cloud_ptr[c + 1] < h_cloud_ptr[c]) return why = "h_cloud_ptr decreases", FLVIS_ERR_INVALID_ARG;
  for (int r = 0; r < h_cloud_ptr[n_clouds]; r++) {
    const int first = h_range2[2 * r], cnt = h_range2[2 * r + 1];
    if (first < 0 || cnt < 0 || first > n_rows || cnt > n_rows - first)
      return why = "range " + std::to_string(r) + " is outside [0, n_rows)", FLVIS_ERR_INVALID_ARG;
  }
  // (the points of a cloud are known once the device has read the counts; a cloud that LISTS 2^31 rows is refused here already)
  for (int c = 0; c < n_clouds; c++) {
    long long rows = 0;
    for (int r = h_cloud_ptr[c]; r < h_cloud_ptr[c + 1]; r++) rows += h_range2[2 * r + 1];
    if (rows > INT_MAX) return why = "cloud " + std::to_string(c) + " lists 2^31 rows or more", FLVIS_ERR_CAPACITY;
  }
  return FLVIS_OK;
}

void mc_tiling(int N, int& tiles_per_blk, int& nblk) {
  const int n_tiles = (N + MC_TILE - 1) / MC_TILE;
  tiles_per_blk = (n_tiles + MC_MAX_BLK - 1) / MC_MAX_BLK;
  nblk = (n_tiles + tiles_per_blk - 1) / tiles_per_blk;
}

}  // namespace

namespace flvis {

size_t mc_sort_table_ints(int N) {
  int tiles_per_blk, nblk;
  mc_tiling(N, tiles_per_blk, nblk);
  return 256 * (size_t)nblk + 257;
}

// the passes: a key byte with two values or more; then, if any ran, the bytes of the cloud index that tell two non-empty clouds apart
int mc_sort(flvis_ctx* ctx, const int* occ, uint64_t* const d_keys[2], uint32_t* const d_idx[2], int N, int n_clouds, const int* d_cstart,
            const long long* cs, uint32_t* d_hist, int* cur_out, int* n_passes, int* n_cloud_digits) {
  hipStream_t st = ctx->stream;
  int tiles_per_blk, nblk;
  mc_tiling(N, tiles_per_blk, nblk);
  uint32_t* const d_tot = d_hist + 256 * (size_t)nblk;  // [257]
  std::vector<McDigit> passes;
  for (int d = 0; d < MC_KEY_DIGITS; d++) {
    int used = 0;
    for (int v = 0; v < 256; v++) used += occ[d * 256 + v] ? 1 : 0;
    if (used > 1) passes.push_back(McDigit{8 * d, 0, n_clouds, d_cstart});
  }
  int cloud_digits = 0;
  while (cloud_digits < 4 && ((long long)(n_clouds - 1) >> (8 * cloud_digits)) > 0) cloud_digits++;
  if (!passes.empty())
    for (int d = 0; d < cloud_digits; d++) {
      int first = -1;
      bool two = false;
      for (int c = 0; c < n_clouds && !two; c++) {
        if (cs[c + 1] == cs[c]) continue;
        const int v = (c >> (8 * d)) & 255;
        if (first < 0) first = v;
        else two = v != first;
      }
      if (two) passes.push_back(McDigit{8 * d, 1, n_clouds, d_cstart});
    }
  int cur = 0;
  for (const McDigit& g : passes) {
    k_mc_hist<<<nblk, MC_T, 0, st>>>(d_keys[cur], d_idx[cur], N, tiles_per_blk, g, d_hist, nblk);
    k_mc_scan_rows<<<256, 1024, 0, st>>>(d_hist, nblk, d_tot);
    k_mc_scan<uint32_t, uint32_t><<<1, 1024, 0, st>>>(d_tot, 256LL, d_tot);
    k_mc_scatter<<<nblk, MC_T, 0, st>>>(d_keys[cur], d_idx[cur], N, tiles_per_blk, g, d_hist, d_tot, nblk, d_keys[cur ^ 1], d_idx[cur ^ 1]);
    MC_LAUNCH(ctx, "voxel_cloud: sort");
    cur ^= 1;
  }
  *cur_out = cur;
  if (n_passes) *n_passes = (int)passes.size();
  if (n_cloud_digits) *n_cloud_digits = cloud_digits;
  return FLVIS_OK;
}

void mc_offsets(hipStream_t st, const int* d_cnt, long long n, long long* d_off, const int* d_eptr, int n_clouds, long long* d_cs64,
                int* d_cstart) {
  k_mc_scan<int, long long><<<1, 1024, 0, st>>>(d_cnt, n, d_off);
  k_mc_cloud_starts<<<(n_clouds + 1 + 255) / 256, 256, 0, st>>>(d_off, d_eptr, n_clouds, d_cs64, d_cstart);
}

// per point: keys [2][N] | points [N][3] | indices [2][N]; tables: byte values [8][256] | histogram [256][nblk] + 1 | output counts
int mc_work(flvis_ctx* ctx, const char* what, int N, bool ids, McWork& W) {
  const std::string w = std::string(what) + ": ";
  auto no_mem = [&]() {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, w + "device allocation failed");
  };
  int tiles_per_blk, nblk;
  mc_tiling(N, tiles_per_blk, nblk);
  W.n_chunks = (N + MC_RB - 1) / MC_RB;
  W.pt_bytes = (size_t)N * MC_BYTES_PER_POINT;
  W.tab_ints = (size_t)MC_KEY_DIGITS * 256 + 256 * (size_t)nblk + 257 + (size_t)W.n_chunks + 1;
  uint8_t* const pb = (uint8_t*)ctx->scratch("mc_points", W.pt_bytes);
  if (!pb) return no_mem();
  W.occ = (int*)ctx->scratch("mc_tables", sizeof(int) * W.tab_ints);
  if (!W.occ) return no_mem();
  W.keys[0] = (uint64_t*)pb, W.keys[1] = (uint64_t*)pb + N;
  W.pts = (double*)(W.keys[1] + N);
  W.idx[0] = (uint32_t*)(W.pts + 3 * (size_t)N), W.idx[1] = W.idx[0] + N;
  W.hist = (uint32_t*)(W.occ + MC_KEY_DIGITS * 256);
  W.bsum = (int*)(W.hist + 256 * (size_t)nblk + 257);
  const hipError_t e = hipMemsetAsync(W.occ, 0, sizeof(int) * MC_KEY_DIGITS * 256, ctx->stream);
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  W.idc = nullptr;  // the points' ids in canonical order (only for a caller that wants the rows' ids)
  if (ids) {
    W.idc = (long long*)ctx->scratch("mc_ids", sizeof(long long) * (size_t)N);
    if (!W.idc) return no_mem();
  }
  return FLVIS_OK;
}

int mc_tail(flvis_ctx* ctx, const char* what, const McWork& W, int N, int n_clouds, const int* d_cstart, int* d_kend, const long long* cs,
            double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts, long long* d_id_out, int64_t* h_n_out, int64_t* h_n_dropped,
            size_t rows_bytes) {
  hipStream_t st = ctx->stream;
  const int NC1 = n_clouds + 1, n_chunks = W.n_chunks;
  int* const d_cg = d_kend + NC1;
  const std::string ws = std::string(what) + ": sort", wr = std::string(what) + ": rows", wk = std::string(what) + ": keys";
  int occ[MC_KEY_DIGITS * 256];
  hipError_t e = hipMemcpyAsync(occ, W.occ, sizeof(occ), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, wk.c_str());
  const auto t_sort = std::chrono::steady_clock::now();
  int cur = 0, n_passes = 0, cloud_digits = 0;
  const int rc = mc_sort(ctx, occ, W.keys, W.idx, N, n_clouds, d_cstart, cs, W.hist, &cur, &n_passes, &cloud_digits);
  if (rc != FLVIS_OK) return rc;
  auto t_rows = t_sort;
  if (W.ms_sort_rows) {  // (a caller that times its stages: one more wait, behind the sort)
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ctx->hip_fail(e, ws.c_str());
    t_rows = std::chrono::steady_clock::now();
    W.ms_sort_rows[0] = std::chrono::duration<double, std::milli>(t_rows - t_sort).count();
  }
  // ---- the rows
  const McOut o{W.keys[cur], d_cstart, d_kend, n_clouds, leaf == 0 ? 1 : 0, min_points};
  k_mc_bounds<<<(n_clouds + 255) / 256, 256, 0, st>>>(W.keys[cur], d_cstart, n_clouds, d_kend);
  k_mc_flags<<<n_chunks, 256, 0, st>>>(o, N, W.bsum);
  k_mc_scan<int, int><<<1, 1024, 0, st>>>(W.bsum, (long long)n_chunks, W.bsum);
  k_mc_cloud_rank<<<NC1, 256, 0, st>>>(o, N, W.bsum, d_cg);
  if (out_cap > 0) k_mc_emit<<<n_chunks, 256, 0, st>>>(o, N, W.idx[cur], W.pts, W.bsum, d_cg, out_cap, d_xyz, d_npts, W.idc, d_id_out);
  MC_LAUNCH(ctx, wr.c_str());
  std::vector<int> back(2 * (size_t)NC1);  // kend | cg (adjacent on the device)
  e = hipMemcpyAsync(back.data(), d_kend, sizeof(int) * back.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, wr.c_str());
  if (W.ms_sort_rows) W.ms_sort_rows[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_rows).count();
  for (int c = 0; c < n_clouds; c++) {
    h_n_out[c] = (int64_t)back[(size_t)NC1 + c + 1] - back[(size_t)NC1 + c];
    if (h_n_dropped) h_n_dropped[c] = cs[c + 1] - back[c];
  }
  ctx->mc_stats[0] = n_passes;
  ctx->mc_stats[1] = MC_KEY_DIGITS + cloud_digits - n_passes;
  ctx->mc_stats[2] = (int64_t)(W.pt_bytes + rows_bytes + sizeof(int) * W.tab_ints);
  ctx->mc_stats[3] = N;
  return FLVIS_OK;
}

// rows and counts of every cloud in one staging buffer of the context
int mc_host_rows_alloc(flvis_ctx* ctx, const char* what, int n_clouds, int out_cap, float** d_xyz, int** d_npts) {
  *d_xyz = nullptr, *d_npts = nullptr;
  if (out_cap <= 0 || n_clouds <= 0) return FLVIS_OK;
  const size_t rows = (size_t)n_clouds * (size_t)out_cap;
  *d_xyz = (float*)ctx->scratch("mc_host_rows", rows * (3 * sizeof(float) + sizeof(int)));
  if (!*d_xyz) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  *d_npts = (int*)(*d_xyz + 3 * rows);
  return FLVIS_OK;
}

int mc_host_rows_fetch(flvis_ctx* ctx, const char* what, int n_clouds, int out_cap, const int64_t* h_n_out, const float* d_xyz,
                       const int* d_npts, float* h_xyz, int* h_npts) {
  hipError_t e = hipSuccess;
  bool any = false;
  for (int g = 0; g < n_clouds && e == hipSuccess; g++) {
    const size_t n = (size_t)std::min<int64_t>(h_n_out[g], out_cap), at = (size_t)g * (size_t)out_cap;
    if (n == 0) continue;
    any = true;
    e = hipMemcpyAsync(h_xyz + 3 * at, d_xyz + 3 * at, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && h_npts) e = hipMemcpyAsync(h_npts + at, d_npts + at, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream);
  }
  if (any || e != hipSuccess) {
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}

int mc_voxel_cloud(flvis_ctx* ctx, const double* d_p3, const int* d_count, const double* d_T_c_w7, int n_rows, int cap, int n_clouds,
                   const int* h_cloud_ptr, const int* h_range2, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                   const long long* d_id_rows, long long* d_id_out, int64_t* h_n_out, int64_t* h_n_dropped) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!d_p3 || !d_count || !d_T_c_w7 || !h_n_out || (!d_xyz && out_cap != 0))
    return ctx->fail(FLVIS_ERR_INVALID_ARG, "voxel_cloud: a NULL required pointer");
  std::string why;
  int rc = mc_check(n_rows, cap, n_clouds, h_cloud_ptr, h_range2, leaf, min_points, out_cap, why);
  if (rc != FLVIS_OK) return ctx->fail(rc, "voxel_cloud: " + why);
  if (d_id_out && (leaf != 0 || !d_id_rows)) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voxel_cloud: ids go with leaf == 0 only");
  // ---- the listed rows, cloud after cloud in the caller's order: [eptr (n_clouds + 1) | rows (R)]
  long long R64 = 0;
  for (int r = 0; r < h_cloud_ptr[n_clouds]; r++) R64 += h_range2[2 * r + 1];
  if (R64 > INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, "voxel_cloud: the call lists 2^31 rows or more");
  const int R = (int)R64, NC1 = n_clouds + 1;
  std::vector<int> stage((size_t)NC1 + (size_t)R);
  {
    size_t at = (size_t)NC1;
    for (int c = 0; c < n_clouds; c++) {
      stage[c] = (int)(at - (size_t)NC1);
      for (int r = h_cloud_ptr[c]; r < h_cloud_ptr[c + 1]; r++)
        for (int k = 0; k < h_range2[2 * r + 1]; k++) stage[at++] = h_range2[2 * r] + k;
    }
    stage[n_clouds] = R;
  }
  for (int c = 0; c < n_clouds; c++) h_n_out[c] = 0;
  if (h_n_dropped)
    for (int c = 0; c < n_clouds; c++) h_n_dropped[c] = 0;
  memset(ctx->mc_stats, 0, sizeof(ctx->mc_stats));
  if (R == 0) return FLVIS_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  auto no_mem = [&]() {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, "voxel_cloud: device allocation failed");
  };
  // ---- per row and per cloud: off64 [R + 1] | cs64 [NC1] | eptr [NC1] | rows [R] | cnt [R] | cstart [NC1] | kend [NC1] | cg [NC1]
  const size_t rows_bytes = 8 * ((size_t)R + 1 + NC1) + 4 * (2 * (size_t)R + 4 * (size_t)NC1);
  uint8_t* const rb = (uint8_t*)ctx->scratch("mc_rows", rows_bytes);
  if (!rb) return no_mem();
  long long* const d_off = (long long*)rb;
  long long* const d_cs64 = d_off + R + 1;
  int* const d_eptr = (int*)(d_cs64 + NC1);
  int* const d_rows = d_eptr + NC1;
  int* const d_cnt = d_rows + R;
  int* const d_cstart = d_cnt + R;
  int* const d_kend = d_cstart + NC1;
  int* const d_cg = d_kend + NC1;
  hipError_t e = hipMemcpyAsync(d_eptr, stage.data(), sizeof(int) * stage.size(), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return ctx->hip_fail(e, "voxel_cloud");
  auto fail_sync = [&](int code) {  // (`stage` goes away on return)
    hipStreamSynchronize(st);
    return code;
  };
  k_mc_counts<<<(R + 255) / 256, 256, 0, st>>>(d_rows, R, d_count, cap, d_cnt);
  mc_offsets(st, d_cnt, (long long)R, d_off, d_eptr, n_clouds, d_cs64, d_cstart);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, "voxel_cloud: counts"));
  std::vector<long long> cs((size_t)NC1);
  e = hipMemcpyAsync(cs.data(), d_cs64, sizeof(long long) * NC1, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return ctx->hip_fail(e, "voxel_cloud: counts");
  if (cs[n_clouds] > (long long)INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, "voxel_cloud: 2^31 input points or more");
  const int N = (int)cs[n_clouds];
  if (N == 0) return FLVIS_OK;
  McWork W;
  rc = mc_work(ctx, "voxel_cloud", N, d_id_out != nullptr, W);
  if (rc != FLVIS_OK) return rc;
  k_mc_keys<<<R, 256, 0, st>>>(d_rows, d_cnt, d_off, d_p3, d_T_c_w7, cap, leaf, W.keys[0], W.idx[0], W.pts, W.occ, W.idc ? d_id_rows : nullptr,
                               W.idc);
  MC_LAUNCH(ctx, "voxel_cloud: keys");
  return mc_tail(ctx, "voxel_cloud", W, N, n_clouds, d_cstart, d_kend, cs.data(), leaf, min_points, out_cap, d_xyz, d_npts, d_id_out, h_n_out,
                 h_n_dropped, rows_bytes);
}

}  // namespace flvis
extern "C" {

int flvis_hip_voxel_cloud_info(int* h_info4) {
  if (!h_info4) return FLVIS_ERR_INVALID_ARG;
  h_info4[0] = MC_TILE;
  h_info4[1] = MC_T;
  h_info4[2] = MC_BYTES_PER_POINT;
  h_info4[3] = MC_BYTES_PER_ROW;
  return FLVIS_OK;
}

int flvis_voxel_cloud_check(int n_rows, int cap, int n_clouds, const int* h_cloud_ptr, const int* h_range2, double leaf, int min_points,
                            int out_cap) {
  std::string why;
  return mc_check(n_rows, cap, n_clouds, h_cloud_ptr, h_range2, leaf, min_points, out_cap, why);
}

int flvis_hip_voxel_cloud_stats(flvis_ctx* ctx, int64_t* h_stats4) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!h_stats4) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voxel_cloud_stats: NULL output");
  memcpy(h_stats4, ctx->mc_stats, sizeof(ctx->mc_stats));
  return FLVIS_OK;
}

int flvis_hip_voxel_cloud(flvis_ctx* ctx, const double* d_p3, const int* d_count, const double* d_T_c_w7, int n_rows, int cap, int n_clouds,
                          const int* h_cloud_ptr, const int* h_range2, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                          int64_t* h_n_out, int64_t* h_n_dropped) {
  return flvis::mc_voxel_cloud(ctx, d_p3, d_count, d_T_c_w7, n_rows, cap, n_clouds, h_cloud_ptr, h_range2, leaf, min_points, out_cap, d_xyz, d_npts,
                               nullptr, nullptr, h_n_out, h_n_dropped);
}
}
