// flvis_amd: what map_cloud.hip shares with lm_cloud.hip (the local map's cloud ends in the same kernels).
#pragma once
#include <cstddef>
#include <cstdint>

struct flvis_ctx;

namespace flvis {

// One stable sort of N (key, index) pairs by (cloud | key) with map_cloud.hip's radix passes, on the context's stream.
//   h_occ [8][256]: which values each key byte takes over the whole call (a byte with one value is skipped); keys / idx: the two buffers
//   of the passes, the input in [0]; d_cstart [n_clouds + 1]: the clouds' first canonical indices (device), h_cs the same on the host;
//   d_tab: mc_sort_table_ints(N) 32-bit words of workspace.  *cur: the buffer that holds the result.  passes / cloud_digits may be NULL.
size_t mc_sort_table_ints(int N);
int mc_sort(flvis_ctx* ctx, const int* h_occ, uint64_t* const keys[2], uint32_t* const idx[2], int N, int n_clouds, const int* d_cstart,
            const long long* h_cs, uint32_t* d_tab, int* cur, int* passes, int* cloud_digits);

// flvis_hip_voxel_cloud, and with leaf == 0 optionally the id of every output row: d_id_rows [n_rows][cap] the input points' ids,
// d_id_out [n_clouds][out_cap] (both NULL: the public call)
int mc_voxel_cloud(flvis_ctx* ctx, const double* d_p3, const int* d_count, const double* d_T_c_w7, int n_rows, int cap, int n_clouds,
                   const int* h_cloud_ptr, const int* h_range2, double leaf, int min_points, int out_cap, float* d_xyz, int* d_npts,
                   const long long* d_id_rows, long long* d_id_out, int64_t* h_n_out, int64_t* h_n_dropped);

}  // namespace flvis
