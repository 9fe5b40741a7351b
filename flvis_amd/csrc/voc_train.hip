// flvis_amd: training of a DBoW3 vocabulary on the device -- Vocabulary::create (3rdPartLib/DBow3/src/Vocabulary.cpp:142-569:
// HKmeansStep :231-392, initiateClustersKMpp :407-489, createWords :494-513, setNodeWeights :518-569; DescManip::meanValue,
// DescManip.cpp:25-74) for the 32-byte descriptors flvis_hip_orb_detect_and_compute leaves in HBM.  DESIGN.md section 8 f4
// "training" holds the definition; in short:
//   * the tree is built level by level.  A node of n descriptors at a level < L is split: n <= k gives one cluster per descriptor
//     (no random number drawn); otherwise k-means++ seeding, then passes of {assign every descriptor to the FIRST nearest centre,
//     bit-majority means (bit set when sum >= n/2 + n%2; an empty cluster keeps its centre)} until the association repeats.
//     Every cluster becomes a child; a child is split further when its level < L and it holds more than one descriptor.
//   * departures from DBoW3: (a) a split node draws from its own glibc stream srand(seed + node id), nodes are numbered
//     breadth-first -- children of a level consecutively, by (parent id, cluster index) --, so L = 1 is Vocabulary::create after
//     srand(seed); (b) a node's k-means ends after max_iters association passes.
//   * weights: every training descriptor goes down the FINISHED tree (voc_descend, the descent of the transform); Ni = images
//     with a feature at word i; weight = log(NDocs / Ni) in fp64 on the host.
// All sums are integer sums (distances, bit counts, cluster sizes, Ni): partial sums in LDS, then integer atomics, so the tree is
// the same bit for bit from run to run and whichever of the two paths clusters a node:
//   small nodes (n <= small_node_max): one workgroup per node, every such node of a level in ONE launch (k_vt_small): descriptors,
//     labels and bit counts stay in LDS from the seeding to the stable regrouping;
//   large nodes: kernels over the node's contiguous descriptor range, driven from the host (k_vt_lg_*); at most N / small_node_max
//     of them per level.
// Descriptors of a level's nodes lie in one buffer, each node a contiguous range in its parent's order; a split writes the node's
// range regrouped by cluster (stable) into the other buffer, where the children's ranges follow from the cluster sizes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/flvis_hip.h"
#include "ctx.hpp"
#include "voc_descent.hpp"
#include "voc_file.hpp"

namespace flvis {

constexpr int VT_T = 256;                 // threads per workgroup: one per descriptor bit in the majority phases
constexpr int VT_KMAX = 64;               // clusters per node (labels are bytes, a wave's ballot ranks at most 64 labels)
constexpr int VT_TILE = 1024;             // descriptors per workgroup of the large-node kernels
constexpr int VT_SMALL_DEFAULT = 2048;    // 2048 x 32 B = 64 KB of descriptors: two resident workgroups per CU (160 KB LDS)
constexpr int VT_LDS_MAX = 150 * 1024;    // dynamic LDS a workgroup may claim
constexpr int VT_MAXF = 2048;             // descriptors per image
constexpr int VT_MAXIMG = 65535;          // images per training: k_vt_gather has one grid row per image
constexpr int VT_REDRAWS = 1 << 16;       // bound on `do cut = .. while (cut == 0.0)` (rand() returns 0 once in 2^31 draws)

// ---- glibc rand() (TYPE_3): srand(seed) leaves the last 34 words of r[i] = r[i - 31] + r[i - 3] over 344 words ------------------
struct VtRand {
  int r[34];
  int pos;
};
__host__ __device__ inline void vt_srand(VtRand& g, unsigned seed) {
  int* v = g.r;  // the ring holds word i at i % 34: after 344 words the next one is written at 344 % 34
  v[0] = seed == 0 ? 1 : (int)seed;  // srandom_r: seed 0 is seed 1
  for (int i = 1; i < 31; i++) {
    long long w = (16807LL * v[i - 1]) % 2147483647;
    if (w < 0) w += 2147483647;
    v[i] = (int)w;
  }
  for (int i = 31; i < 34; i++) v[i] = v[i - 31];
  for (int i = 34; i < 344; i++) v[i % 34] = (int)((unsigned)v[(i - 31) % 34] + (unsigned)v[(i - 3) % 34]);
  g.pos = 344 % 34;
}
__host__ __device__ inline int vt_rand(VtRand& g) {
  const int pos = g.pos;
  const int n = (int)((unsigned)g.r[(pos + 34 - 31) % 34] + (unsigned)g.r[(pos + 34 - 3) % 34]);
  g.r[pos] = n;
  g.pos = (pos + 1) % 34;
  return (int)(((unsigned)n) >> 1);
}
// the cut of initiateClustersKMpp as the integer the prefix sums are compared with: prefix >= cut <=> prefix >= ceil(cut)
__host__ __device__ inline long long vt_draw_cut(VtRand& g, long long dist_sum) {
  double cut = 0.0;
  for (int i = 0; i < VT_REDRAWS && cut == 0.0; i++) cut = ((double)vt_rand(g) / (double)2147483647) * (double)dist_sum;
  if (cut == 0.0) return 1;  // every redraw was 0: both paths then take the first descriptor with min_dist > 0
  return (long long)ceil(cut);
}

struct U256 {
  unsigned long long w[4];
};
__device__ inline U256 vt_load(const uint8_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  U256 r;
  r.w[0] = (unsigned long long)a.x | ((unsigned long long)a.y << 32);
  r.w[1] = (unsigned long long)a.z | ((unsigned long long)a.w << 32);
  r.w[2] = (unsigned long long)b.x | ((unsigned long long)b.y << 32);
  r.w[3] = (unsigned long long)b.z | ((unsigned long long)b.w << 32);
  return r;
}
__device__ inline int vt_ham(const U256& a, const U256& b) {
  return __popcll(a.w[0] ^ b.w[0]) + __popcll(a.w[1] ^ b.w[1]) + __popcll(a.w[2] ^ b.w[2]) + __popcll(a.w[3] ^ b.w[3]);
}
__device__ inline void vt_copy32(uint8_t* dst, const uint8_t* src) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  const uint4 a = s[0], b = s[1];
  d[0] = a;
  d[1] = b;
}

// sum of one int per thread over the workgroup (VT_T / 64 waves)
__device__ inline int vt_block_sum(int v, int* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  int tot = 0;
#pragma unroll
  for (int i = 0; i < VT_T / 64; i++) tot += s_red[i];
  return tot;
}
// exclusive prefix of one int per thread over the workgroup
__device__ inline int vt_block_excl(int v, int* s_red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  __syncthreads();
  if (lane == 63) s_red[wv] = inc;
  __syncthreads();
  int off = 0;
#pragma unroll
  for (int i = 0; i < VT_T / 64; i++)
    if (i < wv) off += s_red[i];
  return off + inc - v;
}

// the nearest centre of one descriptor: the FIRST of minimal distance (strict `<` in centre order, HKmeansStep :307-318)
__device__ inline int vt_nearest(const U256& f, const uint8_t* s_cen, int ncl) {
  int best = 0, best_d = vt_ham(f, vt_load(s_cen));
  for (int c = 1; c < ncl; c++) {
    const int d = vt_ham(f, vt_load(s_cen + c * 32));
    if (d < best_d) {
      best_d = d;
      best = c;
    }
  }
  return best;
}

// per-cluster bit counts of n descriptors in LDS: thread t owns bit (t & 7) of byte (t >> 3) -- a column of s_cnt [ncl][VT_T]
__device__ inline void vt_bitcount(const uint8_t* s_desc, const uint8_t* s_lab, int n, unsigned short* s_cnt) {
  const int t = threadIdx.x, byte = t >> 3, sh = t & 7;
  for (int i = 0; i < n; i++) {
    const int c = s_lab[i];
    s_cnt[c * VT_T + t] = (unsigned short)(s_cnt[c * VT_T + t] + ((s_desc[i * 32 + byte] >> sh) & 1));
  }
}
// DescManip::meanValue from the bit counts of a cluster of sz > 0 members: bit set when count >= sz/2 + sz%2 (one member: its copy).
// The 64 lanes of a wave hold the 64 bits of 8 consecutive bytes in memory order, so the ballot IS those bytes.
__device__ inline void vt_majority(int count, int sz, uint8_t* centre) {
  const unsigned long long m = __ballot(count >= sz / 2 + sz % 2);
  if ((threadIdx.x & 63) == 0) *reinterpret_cast<unsigned long long*>(centre + (threadIdx.x >> 6) * 8) = m;
}

// Stable partition by label, one tile of VT_T items in item order: s_run[c] is where the next member of cluster c goes; returns the
// position of this thread's item (valid or not, every thread of the workgroup calls).  s_wcnt: [VT_T / 64][VT_KMAX].
__device__ inline int vt_tile_pos(bool valid, int lab, int ncl, int* s_run, int* s_wcnt) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  s_wcnt[t] = 0;  // VT_T == (VT_T / 64) * VT_KMAX
  __syncthreads();
  unsigned long long todo = __ballot(valid);
  int rank = 0;
  for (int it = 0; it < 64 && todo != 0; it++) {  // one round per distinct label of the wave
    const int leader = __ffsll((long long)todo) - 1;
    const int c = __shfl(lab, leader, 64);
    const unsigned long long m = __ballot(valid && lab == c);
    if (valid && lab == c) rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == leader) s_wcnt[wv * VT_KMAX + c] = __popcll(m);
    todo &= ~m;
  }
  __syncthreads();
  int pos = 0;
  if (valid) {
    pos = s_run[lab] + rank;
    for (int w = 0; w < wv; w++) pos += s_wcnt[w * VT_KMAX + lab];
  }
  __syncthreads();
  if (t < ncl) {
    int add = 0;
    for (int w = 0; w < VT_T / 64; w++) add += s_wcnt[w * VT_KMAX + t];
    s_run[t] += add;
  }
  __syncthreads();
  return pos;
}

// ---- the training set as one list: image-major, row order within an image (getFeatures) ----------------------------------------
__global__ __launch_bounds__(VT_T) void k_vt_gather(const uint8_t* __restrict__ desc, const int* __restrict__ img_off, int cap,
                                                    uint8_t* __restrict__ out) {
  const int img = blockIdx.y, r = blockIdx.x * VT_T + threadIdx.x;
  const int n = img_off[img + 1] - img_off[img];
  if (r < n) vt_copy32(out + ((size_t)img_off[img] + r) * 32, desc + ((size_t)img * cap + r) * 32);
}

// ---- small nodes: one workgroup per node ----------------------------------------------------------------------------------------
struct VtJob {
  int off, n;     // the node's descriptors: rows [off, off + n) of the level's buffer
  unsigned seed;  // srand(seed) of this node
  int pad;
};

extern __shared__ uint4 vt_smem[];

// dynamic LDS of k_vt_small for nodes of at most nmax descriptors: descriptors, centres, {min distances | bit counts}, labels
static size_t vt_small_lds(int nmax, int k) {
  const size_t n16 = (size_t)(nmax + 15) / 16 * 16;
  return n16 * 32 + (size_t)k * 32 + std::max(n16 * 2, (size_t)k * VT_T * 2) + n16;
}

// res_info[job] = {clusters, association passes, hit max_iters}; res_size [job][k]; res_cen [job][k][32]
__global__ __launch_bounds__(VT_T) void k_vt_small(const VtJob* __restrict__ jobs, const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                   int k, int max_iters, int nmax, int* __restrict__ res_info, int* __restrict__ res_size,
                                                   uint8_t* __restrict__ res_cen) {
  __shared__ int s_size[VT_KMAX], s_run[VT_KMAX], s_wcnt[VT_T], s_red[VT_T / 64];
  __shared__ int s_pick, s_changed, s_stop;
  __shared__ VtRand s_g;
  const int t = threadIdx.x;
  const VtJob job = jobs[blockIdx.x];
  const int n = min(job.n, nmax);  // (the host never hands over more than the LDS it sized for)
  const size_t n16 = (size_t)(nmax + 15) / 16 * 16;
  uint8_t* s_desc = reinterpret_cast<uint8_t*>(vt_smem);
  uint8_t* s_cen = s_desc + n16 * 32;
  unsigned short* s_u = reinterpret_cast<unsigned short*>(s_cen + (size_t)k * 32);  // seeding: min_dist [n]; k-means: bit counts [ncl][VT_T]
  uint8_t* s_lab = reinterpret_cast<uint8_t*>(s_u) + max(n16 * 2, (size_t)k * VT_T * 2);

  {
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)job.off * 32);
    uint4* dst = reinterpret_cast<uint4*>(s_desc);
    for (int i = t; i < n * 2; i += VT_T) dst[i] = src[i];
  }
  if (t < VT_KMAX) s_size[t] = 0;
  __syncthreads();

  int ncl = 0, passes = 0, capped = 0;
  if (n <= k) {
    // trivial case (HKmeansStep :246-256): one cluster per descriptor, in order
    ncl = n;
    if (t < n) {
      vt_copy32(s_cen + t * 32, s_desc + t * 32);
      s_lab[t] = (uint8_t)t;
      s_size[t] = 1;
    }
    __syncthreads();
  } else {
    // ---- initiateClustersKMpp: wave 0's first lane runs the generator ----
    VtRand& g = s_g;
    if (t == 0) {
      vt_srand(g, job.seed);
      s_pick = vt_rand(g) % n;
    }
    __syncthreads();
    for (int j = 0; j < k; j++) {  // centre j is descriptor s_pick
      const int pick = s_pick;
      if (t < 2) reinterpret_cast<uint4*>(s_cen + j * 32)[t] = reinterpret_cast<const uint4*>(s_desc + pick * 32)[t];
      ncl = j + 1;
      if (ncl == k) break;
      __syncthreads();
      const U256 cj = vt_load(s_cen + j * 32);
      int part = 0;
      for (int i = t; i < n; i += VT_T) {
        const int d = vt_ham(vt_load(s_desc + i * 32), cj);
        int m = d;
        if (j > 0) {
          m = s_u[i];
          if (m > 0) m = min(m, d);
        }
        s_u[i] = (unsigned short)m;
        part += m;
      }
      const int dist_sum = vt_block_sum(part, s_red);  // (n <= 4 K descriptors x 256 bits: an int holds it)
      if (dist_sum == 0) break;                         // every descriptor already equals a centre
      if (t == 0) {
        s_stop = (int)vt_draw_cut(g, dist_sum);
        s_pick = n - 1;
      }
      __syncthreads();
      // the first i whose prefix sum reaches the cut: a contiguous chunk per thread, an exclusive scan of the chunk sums, and the
      // one thread whose chunk crosses the cut walks it
      const int chunk = (n + VT_T - 1) / VT_T, i0 = min(n, t * chunk), i1 = min(n, i0 + chunk);
      int local = 0;
      for (int i = i0; i < i1; i++) local += s_u[i];
      const int before = vt_block_excl(local, s_red);
      const int cut = s_stop;
      if (before < cut && cut <= before + local) {
        int run = before;
        for (int i = i0; i < i1; i++) {
          run += s_u[i];
          if (run >= cut) {
            s_pick = i;
            break;
          }
        }
      }
      __syncthreads();
    }
    __syncthreads();

    // ---- k-means: at most max_iters association passes ----
    for (int pass = 1; pass <= max_iters; pass++) {
      if (pass > 1) {
        for (int i = t; i < ncl * VT_T; i += VT_T) s_u[i] = 0;
        __syncthreads();
        vt_bitcount(s_desc, s_lab, n, s_u);
        __syncthreads();
        for (int c = 0; c < ncl; c++) {
          const int sz = s_size[c];
          if (sz > 0) vt_majority(s_u[c * VT_T + t], sz, s_cen + c * 32);  // an empty cluster keeps its centre
        }
        __syncthreads();
      }
      if (t < VT_KMAX) s_size[t] = 0;
      if (t == 0) s_changed = 0;
      __syncthreads();
      for (int i = t; i < n; i += VT_T) {
        const int best = vt_nearest(vt_load(s_desc + i * 32), s_cen, ncl);
        if (pass > 1 && s_lab[i] != best) s_changed = 1;
        s_lab[i] = (uint8_t)best;
        atomicAdd(&s_size[best], 1);
      }
      __syncthreads();
      passes = pass;
      const bool same = pass > 1 && s_changed == 0;
      __syncthreads();
      if (same) break;
      if (pass == max_iters) capped = 1;
    }
  }

  // ---- results, and the node's descriptors regrouped by cluster (stable) for the next level ----
  int* info = res_info + (size_t)blockIdx.x * 3;
  if (t == 0) {
    info[0] = ncl;
    info[1] = passes;
    info[2] = capped;
    int run = 0;
    for (int c = 0; c < ncl; c++) {
      s_run[c] = run;
      run += s_size[c];
    }
  }
  if (t < ncl) res_size[(size_t)blockIdx.x * k + t] = s_size[t];
  for (int i = t; i < ncl * 2; i += VT_T)
    reinterpret_cast<uint4*>(res_cen + (size_t)blockIdx.x * k * 32)[i] = reinterpret_cast<const uint4*>(s_cen)[i];
  __syncthreads();
  for (int base = 0; base < n; base += VT_T) {
    const int i = base + t;
    const bool valid = i < n;
    const int pos = vt_tile_pos(valid, valid ? (int)s_lab[i] : 0, ncl, s_run, s_wcnt);
    if (valid && pos < n) vt_copy32(out + ((size_t)job.off + pos) * 32, s_desc + i * 32);
  }
}

// ---- large nodes: kernels over the node's range [off, off + n) -------------------------------------------------------------------
// one step of the seeding: min_dist against the newest centre (descriptor `pick` of the node) and its sum per workgroup
__global__ __launch_bounds__(VT_T) void k_vt_lg_seed(const uint8_t* __restrict__ in, int off, int n, int pick, int first,
                                                     int* __restrict__ md, int* __restrict__ blocksum) {
  __shared__ int s_red[VT_T / 64];
  const int i = blockIdx.x * VT_T + threadIdx.x;
  int m = 0;
  if (i < n) {
    const int d = vt_ham(vt_load(in + ((size_t)off + i) * 32), vt_load(in + ((size_t)off + pick) * 32));
    m = d;
    if (!first) {
      m = md[i];
      if (m > 0) m = min(m, d);
    }
    md[i] = m;
  }
  const int s = vt_block_sum(m, s_red);
  if (threadIdx.x == 0) blocksum[blockIdx.x] = s;
}

// one association pass over a tile of VT_TILE descriptors: labels, `changed`, and the tile's cluster sizes and bit counts -- summed in
// LDS, then added to the node's with integer atomics.  hist [tile][ncl] keeps the tile's cluster sizes for the regrouping.
__global__ __launch_bounds__(VT_T) void k_vt_lg_assign(const uint8_t* __restrict__ in, int off, int n, const uint8_t* __restrict__ cen, int ncl,
                                                       int compare, uint8_t* __restrict__ lab, int* __restrict__ changed, int* __restrict__ cnt,
                                                       int* __restrict__ size, int* __restrict__ hist) {
  __shared__ int s_size[VT_KMAX];
  __shared__ int s_changed;
  const int t = threadIdx.x;
  uint8_t* s_desc = reinterpret_cast<uint8_t*>(vt_smem);  // [VT_TILE][32]
  uint8_t* s_cen = s_desc + VT_TILE * 32;                 // [VT_KMAX][32]
  uint8_t* s_lab = s_cen + VT_KMAX * 32;                  // [VT_TILE]
  unsigned short* s_cnt = reinterpret_cast<unsigned short*>(s_lab + VT_TILE);  // [ncl][VT_T]
  const int i0 = blockIdx.x * VT_TILE, nt = min(VT_TILE, n - i0);
  {
    const uint4* src = reinterpret_cast<const uint4*>(in + ((size_t)off + i0) * 32);
    uint4* dst = reinterpret_cast<uint4*>(s_desc);
    for (int i = t; i < nt * 2; i += VT_T) dst[i] = src[i];
    for (int i = t; i < ncl * 2; i += VT_T) reinterpret_cast<uint4*>(s_cen)[i] = reinterpret_cast<const uint4*>(cen)[i];
    for (int i = t; i < ncl * VT_T; i += VT_T) s_cnt[i] = 0;
  }
  if (t < VT_KMAX) s_size[t] = 0;
  if (t == 0) s_changed = 0;
  __syncthreads();
  for (int i = t; i < nt; i += VT_T) {
    const int best = vt_nearest(vt_load(s_desc + i * 32), s_cen, ncl);
    if (compare && lab[(size_t)off + i0 + i] != best) s_changed = 1;
    lab[(size_t)off + i0 + i] = (uint8_t)best;
    s_lab[i] = (uint8_t)best;
    atomicAdd(&s_size[best], 1);
  }
  __syncthreads();
  vt_bitcount(s_desc, s_lab, nt, s_cnt);
  __syncthreads();
  for (int i = t; i < ncl * VT_T; i += VT_T) {
    const int v = s_cnt[i];
    if (v) atomicAdd(&cnt[i], v);
  }
  if (t < ncl) {
    hist[(size_t)blockIdx.x * ncl + t] = s_size[t];
    if (s_size[t]) atomicAdd(&size[t], s_size[t]);
  }
  if (t == 0 && s_changed) *changed = 1;
}

// the centres of the next pass from the node's bit counts: one workgroup per cluster
__global__ __launch_bounds__(VT_T) void k_vt_lg_means(const int* __restrict__ cnt, const int* __restrict__ size, uint8_t* __restrict__ cen) {
  const int c = blockIdx.x, sz = size[c];
  if (sz > 0) vt_majority(cnt[c * VT_T + threadIdx.x], sz, cen + c * 32);
}

// hist [tile][ncl] of cluster sizes -> where each tile's members of each cluster start in the regrouped range
__global__ __launch_bounds__(VT_KMAX) void k_vt_lg_scan(int* __restrict__ hist, int n_tiles, int ncl, const int* __restrict__ size) {
  const int c = threadIdx.x;
  if (c >= ncl) return;
  int run = 0;
  for (int i = 0; i < c; i++) run += size[i];
  for (int b = 0; b < n_tiles; b++) {
    const int h = hist[(size_t)b * ncl + c];
    hist[(size_t)b * ncl + c] = run;
    run += h;
  }
}

__global__ __launch_bounds__(VT_T) void k_vt_lg_scatter(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int off, int n,
                                                        const uint8_t* __restrict__ lab, const int* __restrict__ hist, int ncl) {
  __shared__ int s_run[VT_KMAX], s_wcnt[VT_T];
  const int t = threadIdx.x;
  if (t < ncl) s_run[t] = hist[(size_t)blockIdx.x * ncl + t];
  __syncthreads();
  const int i0 = blockIdx.x * VT_TILE;
  for (int base = 0; base < VT_TILE; base += VT_T) {
    const int i = i0 + base + t;
    const bool valid = i < n;
    const int l = valid ? (int)lab[(size_t)off + i] : 0;
    const int pos = vt_tile_pos(valid, min(l, ncl - 1), ncl, s_run, s_wcnt);
    if (valid && pos < n) vt_copy32(out + ((size_t)off + pos) * 32, in + ((size_t)off + i) * 32);
  }
}

// ---- setNodeWeights: Ni [word] = images with a feature at the word; one workgroup per image ------------------------------------
__global__ __launch_bounds__(VT_T) void k_vt_ni(VocDev v, const uint8_t* __restrict__ desc, const int* __restrict__ count, int cap,
                                                int* __restrict__ ni) {
  __shared__ int s_w[VT_MAXF];
  const int img = blockIdx.x, t = threadIdx.x;
  const int n = max(0, min(count[img], min(cap, VT_MAXF)));
  for (int r = t; r < n; r += VT_T) {
    const uint4* f = reinterpret_cast<const uint4*>(desc + ((size_t)img * cap + r) * 32);
    bool leaf;
    const int node = voc_descend(v, f[0], f[1], leaf);
    const int w = leaf ? v.word_id[node] : -1;
    s_w[r] = (w >= 0 && w < v.n_words) ? w : -1;
  }
  __syncthreads();
  for (int r = t; r < n; r += VT_T) {
    const int w = s_w[r];
    if (w < 0) continue;
    bool first = true;  // `counted[word_id]`: only the image's first feature at a word counts
    for (int q = 0; q < r; q++)
      if (s_w[q] == w) {
        first = false;
        break;
      }
    if (first) atomicAdd(&ni[w], 1);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
namespace {

struct DevMem {  // device allocations of one training run
  std::vector<void*> ptrs;
  ~DevMem() {
    for (void* p : ptrs) hipFree(p);
  }
  template <class T>
  T* get(size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return (T*)p;
  }
};

struct SplitNode {
  int id, off, n;
};
struct SplitResult {
  int ncl = 0, passes = 0, capped = 0;
  std::vector<int> size;
  std::vector<uint8_t> cen;
};

struct Trainer {
  flvis_ctx* ctx;
  hipStream_t st;
  int k, max_iters;
  long long launches = 0;
  // large-node scratch
  uint8_t* d_lab = nullptr;
  int *d_md = nullptr, *d_blocksum = nullptr, *d_hist = nullptr, *d_cnt = nullptr, *d_size = nullptr, *d_changed = nullptr;
  uint8_t* d_cen = nullptr;
  std::vector<int> h_blocksum, h_md;

  hipError_t large(const uint8_t* in, uint8_t* out, const SplitNode& nd, unsigned seed, SplitResult& r) {
    hipError_t e;
    const int n = nd.n, off = nd.off;
    r.size.assign(k, 0);
    r.cen.assign((size_t)k * 32, 0);
    if (n <= k) {  // trivial: the descriptors are the centres, and already in cluster order
      if ((e = hipMemcpyAsync(out + (size_t)off * 32, in + (size_t)off * 32, (size_t)n * 32, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
      if ((e = hipMemcpyAsync(r.cen.data(), in + (size_t)off * 32, (size_t)n * 32, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
      r.ncl = n;
      for (int c = 0; c < n; c++) r.size[c] = 1;
      return hipStreamSynchronize(st);
    }
    VtRand g;
    vt_srand(g, seed);
    std::vector<int> picks{vt_rand(g) % n};
    const int nb = (n + VT_T - 1) / VT_T;
    h_blocksum.resize(nb);
    h_md.resize(VT_T);
    for (int j = 0; (int)picks.size() < k; j++) {
      k_vt_lg_seed<<<nb, VT_T, 0, st>>>(in, off, n, picks.back(), j == 0, d_md, d_blocksum);
      launches++;
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = hipMemcpyAsync(h_blocksum.data(), d_blocksum, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
      long long dist_sum = 0;
      for (int b = 0; b < nb; b++) dist_sum += h_blocksum[b];
      if (dist_sum == 0) break;
      const long long cut = vt_draw_cut(g, dist_sum);
      int pick = n - 1;
      long long run = 0;
      for (int b = 0; b < nb; b++) {  // the exact prefix search: the workgroup whose sums cross the cut, then its descriptors
        if (run + h_blocksum[b] >= cut) {
          const int cntb = std::min(VT_T, n - b * VT_T);
          if ((e = hipMemcpyAsync(h_md.data(), d_md + (size_t)b * VT_T, (size_t)cntb * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
          if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
          for (int i = 0; i < cntb; i++) {
            run += h_md[i];
            if (run >= cut) {
              pick = b * VT_T + i;
              break;
            }
          }
          break;
        }
        run += h_blocksum[b];
      }
      picks.push_back(pick);
    }
    const int ncl = (int)picks.size();
    for (int c = 0; c < ncl; c++)
      if ((e = hipMemcpyAsync(d_cen + (size_t)c * 32, in + ((size_t)off + picks[c]) * 32, 32, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
    const int tiles = (n + VT_TILE - 1) / VT_TILE;
    const size_t lds = (size_t)VT_TILE * 32 + VT_KMAX * 32 + VT_TILE + (size_t)ncl * VT_T * 2;
    for (int pass = 1; pass <= max_iters; pass++) {
      if (pass > 1) {
        k_vt_lg_means<<<ncl, VT_T, 0, st>>>(d_cnt, d_size, d_cen);
        launches++;
      }
      if ((e = hipMemsetAsync(d_cnt, 0, (size_t)ncl * VT_T * sizeof(int), st)) != hipSuccess) return e;
      if ((e = hipMemsetAsync(d_size, 0, VT_KMAX * sizeof(int), st)) != hipSuccess) return e;
      if ((e = hipMemsetAsync(d_changed, 0, sizeof(int), st)) != hipSuccess) return e;
      k_vt_lg_assign<<<tiles, VT_T, lds, st>>>(in, off, n, d_cen, ncl, pass > 1, d_lab, d_changed, d_cnt, d_size, d_hist);
      launches++;
      if ((e = hipGetLastError()) != hipSuccess) return e;
      int changed = 0;
      if ((e = hipMemcpyAsync(&changed, d_changed, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
      r.passes = pass;
      if (pass > 1 && !changed) break;
      if (pass == max_iters) r.capped = 1;
    }
    k_vt_lg_scan<<<1, VT_KMAX, 0, st>>>(d_hist, tiles, ncl, d_size);
    k_vt_lg_scatter<<<tiles, VT_T, 0, st>>>(in, out, off, n, d_lab, d_hist, ncl);
    launches += 2;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    r.ncl = ncl;
    if ((e = hipMemcpyAsync(r.size.data(), d_size, (size_t)ncl * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(r.cen.data(), d_cen, (size_t)ncl * 32, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    return hipStreamSynchronize(st);
  }
};

}  // namespace
}  // namespace flvis

using namespace flvis;

extern "C" int flvis_hip_voc_train(flvis_ctx* ctx, const uint8_t* d_desc, const int* d_count, int cap, int n_img,
                                   const flvis_voc_train_params* prm, flvis_voc_file** out, int64_t* stats8) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (!d_desc || !d_count || !prm || !out) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: null argument");
  if (prm->k < 2 || prm->k > VT_KMAX) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: k must lie in 2 .. 64");
  if (prm->L < 1 || prm->L > 10) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: L must lie in 1 .. 10");
  if (prm->weighting != 0 && prm->weighting != 1) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: weighting must be 0 (TF_IDF) or 1 (TF)");
  if (prm->max_iters < 0 || prm->small_node_max < 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: negative max_iters or small_node_max");
  if (cap <= 0 || cap > VT_MAXF) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: cap must lie in 1 .. 2048");
  if (n_img <= 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: no image");
  if (n_img > VT_MAXIMG) return ctx->fail(FLVIS_ERR_CAPACITY, "voc_train: more than 65535 images");  // k_vt_gather's gridDim.y
  const int k = prm->k, L = prm->L, max_iters = prm->max_iters ? prm->max_iters : 100;
  hipStream_t st = ctx->stream;
  hipError_t e;
  hipSetDevice(ctx->device);
#define VT_HIP(call)                                                  \
  do {                                                                \
    if ((e = (call)) != hipSuccess) return ctx->hip_fail(e, "voc_train"); \
  } while (0)

  // the counts decide everything that is allocated and launched: read them first
  std::vector<int> img_off(n_img + 1, 0);
  {
    std::vector<int> cnt(n_img);
    VT_HIP(hipMemcpyAsync(cnt.data(), d_count, (size_t)n_img * sizeof(int), hipMemcpyDeviceToHost, st));
    VT_HIP(hipStreamSynchronize(st));
    long long tot = 0;
    for (int i = 0; i < n_img; i++) {
      tot += std::max(0, std::min(cnt[i], cap));
      if (tot > INT_MAX / 64) return ctx->fail(FLVIS_ERR_CAPACITY, "voc_train: more than 2^25 descriptors");
      img_off[i + 1] = (int)tot;
    }
  }
  const int N = img_off[n_img];
  if (N == 0) return ctx->fail(FLVIS_ERR_INVALID_ARG, "voc_train: no descriptor at all");

  // small_node_max: what one workgroup's LDS holds
  int snm = prm->small_node_max ? prm->small_node_max : VT_SMALL_DEFAULT;
  {
    int fit = 16;
    while (vt_small_lds(fit + 16, k) <= (size_t)VT_LDS_MAX) fit += 16;
    snm = std::min(snm, fit);
  }
  // per call, so on the context's device whichever it is (an offline tool: two host calls do not count)
  VT_HIP(hipFuncSetAttribute((const void*)k_vt_small, hipFuncAttributeMaxDynamicSharedMemorySize, VT_LDS_MAX));
  VT_HIP(hipFuncSetAttribute((const void*)k_vt_lg_assign, hipFuncAttributeMaxDynamicSharedMemorySize, VT_LDS_MAX));

  DevMem mem;
  Trainer tr{ctx, st, k, max_iters};
  uint8_t* buf[2] = {mem.get<uint8_t>((size_t)N * 32), mem.get<uint8_t>((size_t)N * 32)};
  int* d_img_off = mem.get<int>(n_img + 1);
  tr.d_lab = mem.get<uint8_t>(N);
  tr.d_md = mem.get<int>(N);
  tr.d_blocksum = mem.get<int>((N + VT_T - 1) / VT_T);
  tr.d_hist = mem.get<int>((size_t)((N + VT_TILE - 1) / VT_TILE) * VT_KMAX);
  tr.d_cnt = mem.get<int>(VT_KMAX * VT_T);
  tr.d_size = mem.get<int>(VT_KMAX);
  tr.d_changed = mem.get<int>(1);
  tr.d_cen = mem.get<uint8_t>(VT_KMAX * 32);
  if (!buf[0] || !buf[1] || !d_img_off || !tr.d_lab || !tr.d_md || !tr.d_blocksum || !tr.d_hist || !tr.d_cnt || !tr.d_size || !tr.d_changed ||
      !tr.d_cen)
    return ctx->fail(FLVIS_ERR_HIP, "voc_train: device allocation failed");
  VT_HIP(hipMemcpyAsync(d_img_off, img_off.data(), (size_t)(n_img + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  k_vt_gather<<<dim3((cap + VT_T - 1) / VT_T, n_img), VT_T, 0, st>>>(d_desc, d_img_off, cap, buf[0]);
  tr.launches++;
  VT_HIP(hipGetLastError());

  // ---- the tree, level by level; node ids are breadth-first, so the children of node n are child_ptr[n] + 1 .. ----
  std::vector<uint8_t> desc(32, 0);  // node 0: the root
  std::vector<int> nchild(1, 0);
  std::vector<SplitNode> level{{0, 0, N}}, next;
  long long passes_total = 0, n_capped = 0, n_empty = 0, n_trivial = 0;
  int cur = 0;
  std::vector<VtJob> jobs;
  std::vector<int> job_of, h_info, h_size;
  std::vector<uint8_t> h_cen;
  std::vector<SplitResult> lg;
  for (int lv = 0; lv < L && !level.empty(); lv++) {
    const uint8_t* in = buf[cur];
    uint8_t* outb = buf[cur ^ 1];
    jobs.clear();
    job_of.assign(level.size(), -1);
    lg.clear();
    int nmax = 0;
    for (size_t i = 0; i < level.size(); i++)
      if (level[i].n <= snm) {
        job_of[i] = (int)jobs.size();
        jobs.push_back(VtJob{level[i].off, level[i].n, prm->seed + (unsigned)level[i].id, 0});
        nmax = std::max(nmax, level[i].n);
      }
    if (!jobs.empty()) {  // every small node of the level in one launch
      DevMem lm;
      VtJob* d_jobs = lm.get<VtJob>(jobs.size());
      int* d_info = lm.get<int>(jobs.size() * 3);
      int* d_sz = lm.get<int>(jobs.size() * k);
      uint8_t* d_cn = lm.get<uint8_t>(jobs.size() * k * 32);
      if (!d_jobs || !d_info || !d_sz || !d_cn) return ctx->fail(FLVIS_ERR_HIP, "voc_train: device allocation failed");
      VT_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(VtJob), hipMemcpyHostToDevice, st));
      k_vt_small<<<(unsigned)jobs.size(), VT_T, vt_small_lds(nmax, k), st>>>(d_jobs, in, outb, k, max_iters, nmax, d_info, d_sz, d_cn);
      tr.launches++;
      VT_HIP(hipGetLastError());
      h_info.resize(jobs.size() * 3);
      h_size.resize(jobs.size() * k);
      h_cen.resize(jobs.size() * k * 32);
      VT_HIP(hipMemcpyAsync(h_info.data(), d_info, h_info.size() * sizeof(int), hipMemcpyDeviceToHost, st));
      VT_HIP(hipMemcpyAsync(h_size.data(), d_sz, h_size.size() * sizeof(int), hipMemcpyDeviceToHost, st));
      VT_HIP(hipMemcpyAsync(h_cen.data(), d_cn, h_cen.size(), hipMemcpyDeviceToHost, st));
      VT_HIP(hipStreamSynchronize(st));
    }
    for (size_t i = 0; i < level.size(); i++)
      if (job_of[i] < 0) {
        lg.emplace_back();
        VT_HIP(tr.large(in, outb, level[i], prm->seed + (unsigned)level[i].id, lg.back()));
      }
    next.clear();
    size_t li = 0;
    for (size_t i = 0; i < level.size(); i++) {  // ascending node id: the children are numbered by (parent id, cluster index)
      const SplitNode& nd = level[i];
      int ncl, passes, capped;
      const int* size;
      const uint8_t* cen;
      if (job_of[i] >= 0) {
        const int j = job_of[i];
        ncl = h_info[j * 3], passes = h_info[j * 3 + 1], capped = h_info[j * 3 + 2];
        size = &h_size[(size_t)j * k];
        cen = &h_cen[(size_t)j * k * 32];
      } else {
        const SplitResult& r = lg[li++];
        ncl = r.ncl, passes = r.passes, capped = r.capped;
        size = r.size.data();
        cen = r.cen.data();
      }
      if (ncl < 1 || ncl > k) return ctx->fail(FLVIS_ERR_HIP, "voc_train: a node came back without clusters");
      passes_total += passes;
      n_capped += capped;
      n_trivial += nd.n <= k;
      int off = nd.off;
      for (int c = 0; c < ncl; c++) {
        const int id = (int)nchild.size();
        nchild.push_back(0);
        nchild[nd.id]++;
        desc.insert(desc.end(), cen + (size_t)c * 32, cen + (size_t)c * 32 + 32);
        if (size[c] < 0 || off + size[c] > nd.off + nd.n) return ctx->fail(FLVIS_ERR_HIP, "voc_train: cluster sizes beyond the node");
        n_empty += size[c] == 0;
        if (lv + 1 < L && size[c] > 1) next.push_back(SplitNode{id, off, size[c]});
        off += size[c];
      }
    }
    level.swap(next);
    cur ^= 1;
  }

  flvis_voc_file* v = new flvis_voc_file();
  const int n_nodes = (int)nchild.size();
  v->k = k, v->L = L, v->scoring = 0, v->weighting = prm->weighting, v->format = 4;
  v->n_nodes = n_nodes;
  v->child_ptr.assign(n_nodes + 1, 0);
  for (int n = 0; n < n_nodes; n++) v->child_ptr[n + 1] = v->child_ptr[n] + nchild[n];
  v->child_idx.resize(n_nodes - 1);
  for (int c = 0; c < n_nodes - 1; c++) v->child_idx[c] = c + 1;
  v->desc = desc;
  v->weight.assign(n_nodes, 0.0);
  v->word_id.assign(n_nodes, -1);
  int n_words = 0;
  for (int n = 1; n < n_nodes; n++)  // createWords: ascending node id over the leaves
    if (nchild[n] == 0) v->word_id[n] = n_words++;
  v->n_words = n_words;

  if (prm->weighting == 1) {
    for (int n = 1; n < n_nodes; n++)
      if (nchild[n] == 0) v->weight[n] = 1.0;
  } else {
    DevMem wm;
    int* d_cp = wm.get<int>(n_nodes + 1);
    int* d_ci = wm.get<int>(n_nodes - 1);
    int* d_wi = wm.get<int>(n_nodes);
    uint8_t* d_ds = wm.get<uint8_t>((size_t)n_nodes * 32);
    int* d_ni = wm.get<int>(n_words);
    if (!d_cp || !d_ci || !d_wi || !d_ds || !d_ni) {
      delete v;
      return ctx->fail(FLVIS_ERR_HIP, "voc_train: device allocation failed");
    }
    std::vector<int> ni(n_words, 0);
    e = hipMemcpyAsync(d_cp, v->child_ptr.data(), (size_t)(n_nodes + 1) * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ci, v->child_idx.data(), (size_t)(n_nodes - 1) * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_wi, v->word_id.data(), (size_t)n_nodes * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ds, v->desc.data(), (size_t)n_nodes * 32, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_ni, 0, (size_t)n_words * sizeof(int), st);
    if (e == hipSuccess) {
      const VocDev vd{d_cp, d_ci, d_ds, d_wi, nullptr, nullptr, n_nodes, n_words, L};
      k_vt_ni<<<n_img, VT_T, 0, st>>>(vd, d_desc, d_count, cap, d_ni);
      tr.launches++;
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ni.data(), d_ni, (size_t)n_words * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      delete v;
      return ctx->hip_fail(e, "voc_train");
    }
    for (int n = 1; n < n_nodes; n++)
      if (nchild[n] == 0 && ni[v->word_id[n]] > 0) v->weight[n] = std::log((double)n_img / (double)ni[v->word_id[n]]);
  }
#undef VT_HIP
  if (stats8) {
    const int64_t s[8] = {N, n_nodes, n_words, passes_total, n_capped, n_empty, n_trivial, tr.launches};
    memcpy(stats8, s, sizeof(s));
  }
  *out = v;
  return FLVIS_OK;
}
