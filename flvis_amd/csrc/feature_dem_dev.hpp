// flvis_amd: FeatureDEM's part on the frame's chain as a device function -- k_feature_dem (img_kernels.hip) and the tracker's merged
// launch k_dem_add_new_seeds (track_kernels.hip, FLVIS_CHAIN_MERGE bit 3) carry the same body.
#pragma once
#include "dev_common.hpp"
#include "img_kernels.hpp"

namespace flvis {

constexpr int DEM_MAXC = 4096;   // max GFTT corners per call (2*gftt_num; KITTI.yaml asks for 2 x 2000); candidate arrays in dynamic LDS
constexpr int DEM_MAXR = 192;    // entries of a region held in LDS (existing + new): img_kernels.hip, FeatureDEM
constexpr int DEM_T = 256;
// dynamic LDS of the body: the sorted candidates, 8 bytes per corner
inline size_t dem_body_lds(int corner_cap) { return (size_t)(((corner_cap < DEM_MAXC ? corner_cap : DEM_MAXC) + 1) & ~1) * 8; }

// (DEM_T threads, one workgroup per stream; its early exit is uniform per workgroup and leaves the function, not the kernel)
__device__ __forceinline__ void k_feature_dem_body(int w, int h, DemParams prm, const float* __restrict__ sorted_xy,
                                                       const int* __restrict__ region_off, int corner_cap, const int* __restrict__ mode,
                                                       const double* __restrict__ exist_xy, const int* __restrict__ nexist,
                                                       int exist_cap, float* __restrict__ out_xy, int* __restrict__ out_n,
                                                       int out_cap) {
  const int s = blockIdx.x;
  const int md = mode ? mode[s] : 1;
  if (md == 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // the sorted candidates, staged once (dynamic LDS: 8 bytes per corner)
  extern __shared__ __attribute__((aligned(16))) unsigned char dem_smem[];
  const int cmax = ((corner_cap < DEM_MAXC ? corner_cap : DEM_MAXC) + 1) & ~1;
  float* cx = reinterpret_cast<float*>(dem_smem);
  float* cy = cx + cmax;
  __shared__ int roff[17];
  __shared__ float kx[16][DEM_MAXR], ky[16][DEM_MAXR];
  __shared__ int kcount[16], knew0[16], ooff[17], kover[16];
  __shared__ int wcnt[DEM_T / 64][16];
  if (tid < 17) roff[tid] = region_off[(size_t)s * 17 + tid];
  if (tid < 16) kcount[tid] = 0, kover[tid] = 0;
  __syncthreads();
  {
    const float* const SX = sorted_xy + (size_t)s * corner_cap * 2;
    const int tot = roff[16] < cmax ? roff[16] : cmax;
    for (int j = tid; j < tot; j += DEM_T) {
      cx[j] = SX[2 * j];
      cy[j] = SX[2 * j + 1];
    }
  }
  // existing features (redetect) fill their regions in landmark order: ordered per-region ranks by ballots, chunk by chunk
  if (md == 2) {
    int ne = nexist[s];
    if (ne > exist_cap) ne = exist_cap;
    const double* E = exist_xy + (size_t)s * exist_cap * 2;
    for (int base = 0; base < ne; base += DEM_T) {
      const int i = base + tid;
      int r = -1;
      float px = 0.f, py = 0.f;
      if (i < ne) {
        px = (float)E[2 * i];
        py = (float)E[2 * i + 1];
        if (px >= 3 && px < (w - 3) && py >= 3 && py < (h - 3))
          r = (int)(4.f * floorf(py / (float)prm.regionHeight) + px / (float)prm.regionWidth);
      }
      int myrank = 0;
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const unsigned long long bq = __ballot(r == q);
        if (lane == 0) wcnt[wv][q] = __popcll(bq);
        if (r == q) myrank = lane_prefix(bq);
      }
      __syncthreads();
      if (r >= 0) {
        int k = kcount[r] + myrank;
        for (int v = 0; v < wv; v++) k += wcnt[v][r];
        if (k < DEM_MAXR) {
          kx[r][k] = px;
          ky[r][k] = py;
        }
      }
      __syncthreads();
      if (tid < 16) {
        int k = kcount[tid];
        for (int v = 0; v < DEM_T / 64; v++) k += wcnt[v][tid];
        kcount[tid] = k < DEM_MAXR ? k : DEM_MAXR;
        if (k >= DEM_MAXR) kover[tid] = 1;  // (at DEM_MAXR too: no slot is left for the one new point)
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid < 16) knew0[tid] = kcount[tid];
  __syncthreads();
  // greedy spacing per region: 16 lanes per region, the lanes split the already kept points of the region
  {
    const int r = tid >> 4, sub = tid & 15;  // 256 threads = 16 regions x 16 lanes (a quarter wave each)
    const int bd = prm.boundary_dis;
    int kept = kcount[r];
    unsigned count = 0;
    const int j0 = roff[r], j1 = roff[r + 1];
    if (md == 2 && kover[r]) {
      // DEM_MAXR existing points or more: the region is full (DEM_MAXR >= max_region_feature_num), the first candidate clear of
      // ALL its existing points is pushed and the walk ends.  The existing points are read again, the 16 lanes splitting the stream's list.
      int ne = nexist[s];
      if (ne > exist_cap) ne = exist_cap;
      const double* E = exist_xy + (size_t)s * exist_cap * 2;
      int found = 0;
      for (int j = j0; j < j1 && !found; j++) {
        const float px = (float)__float2int_rn(cx[j]), py = (float)__float2int_rn(cy[j]);
        int bad = 0;
        for (int i = sub; i < ne; i += 16) {
          const float ex = (float)E[2 * i], ey = (float)E[2 * i + 1];
          if (!(ex >= 3 && ex < (w - 3) && ey >= 3 && ey < (h - 3))) continue;
          if ((int)(4.f * floorf(ey / (float)prm.regionHeight) + ex / (float)prm.regionWidth) != r) continue;
          if (fabsf(px - ex) <= (float)bd || fabsf(py - ey) <= (float)bd) bad = 1;
        }
        bad = (int)((__ballot(bad != 0) >> (lane & 48)) & 0xFFFFull);
        if (!bad) {
          if (sub == 0) {
            kx[r][0] = px;
            ky[r][0] = py;
          }
          found = 1;
        }
      }
      // (the existing entries of kx / ky are not read again: slot 0 is the region's output)
      if (sub == 0) {
        knew0[r] = 0;
        kcount[r] = found;
      }
    } else {
    for (int j = j0; j < j1; j++) {
      float px = cx[j], py = cy[j];
      if (md == 2) {  // cv::Point pt = Point2f (rounds), feature_dem.cpp:174
        px = (float)__float2int_rn(px);
        py = (float)__float2int_rn(py);
      }
      int bad = 0;
      for (int k = sub; k < kept; k += 16) {
        float dis_x = fabsf(px - kx[r][k]);
        float dis_y = fabsf(py - ky[r][k]);
        if (dis_x <= (float)bd || dis_y <= (float)bd) bad = 1;
      }
      // OR over the 16 lanes of this region (one row of 16 lanes of the wave): one ballot of the whole wave, this row's 16 bits
      // (a row that has left the loop contributes zeros and does not look)
      bad = (int)((__ballot(bad != 0) >> (lane & 48)) & 0xFFFFull);
      if (!bad) {
        if (kept < DEM_MAXR && sub == 0) {
          kx[r][kept] = px;
          ky[r][kept] = py;
        }
        kept++;
        count++;
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        if (md == 1) {
          if (count >= prm.max_region_feature_num) break;
        } else {
          if ((unsigned)kept >= prm.max_region_feature_num) break;
        }
      }
    }
    if (sub == 0) kcount[r] = kept < DEM_MAXR ? kept : DEM_MAXR;
    }
  }
  __syncthreads();
  // output: new points, regions in order 0..15, per region in acceptance order
  if (tid == 0) {
    int o = 0;
    for (int r = 0; r < 16; r++) {
      ooff[r] = o;
      o += kcount[r] - knew0[r];
    }
    ooff[16] = o;
    out_n[s] = o < out_cap ? o : out_cap;
  }
  __syncthreads();
  {
    float* O = out_xy + (size_t)s * out_cap * 2;
    const int r = tid >> 4, sub = tid & 15;
    for (int k = knew0[r] + sub; k < kcount[r]; k += 16) {
      const int o = ooff[r] + (k - knew0[r]);
      if (o < out_cap) {
        O[2 * o] = kx[r][k];
        O[2 * o + 1] = ky[r][k];
      }
    }
  }
}

}  // namespace flvis
