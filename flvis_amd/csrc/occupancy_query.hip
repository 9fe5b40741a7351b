// flvis_amd: queries against occupancy maps (flvis_hip_occupancy_cast; include/flvis_hip.h has the definition).
//
// A map is the sorted (key, l) rows the occupancy calls return, a query a segment o -> p in the map's frame.  One lane per query, in the
// caller's order: the lane walks its segment with k_oc_emit's integer-bounded walk (occupancy.hip: the same cells in the same order, by
// the same oc_cell.hpp functions), and at every cell finds the cell's row by a binary search over the map's keys.  The maps never leave
// HBM; nothing is sorted, no atomic is used.
//
// Steps of one call (every map of the call goes through each of them together):
//   k_ocq_check    the maps' keys ascend strictly and are non-negative (a flag the host reads BEFORE the walk is queued: a refused map
//                  writes no output)
//   k_ocq_cast     the walk; per query the six outputs and, in the workspace, the cells it tested
//   k_ocq_sums     one workgroup per map: its queries per status and its cells tested (LDS tree; the host adds the maps)
// Lanes of a wave stop at different cells and search different rows: profiles/r30_occupancy_cast.md has what that costs.
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
#include "oc_cell.hpp"

namespace {

using namespace flvis;

constexpr int OCQ_T = 256;
enum { OCQ_END = 0, OCQ_OCCUPIED = 1, OCQ_UNKNOWN = 2, OCQ_DROPPED = 3, OCQ_LIMIT = 4 };

struct OcqMaps {
  const int64_t* key;  // [n_maps][cap]
  const float* l;      // [n_maps][cap]
  int cap, n_maps;
  const int* nrows;  // [n_maps]
  const int* qptr;   // [n_maps + 1]
};
// the line directory: map m's lines are the slots ptr[m] .. ptr[m + 1] - 2, ascending; line[j] = key >> 21, first[j] its first row, and the
// slot behind a map's last line holds first = the map's row count (so a line's rows end at first[j + 1])
struct OcqDir {
  const int64_t* line;
  const int* first;
  const int* ptr;  // [n_maps + 1]
};
struct OcqOut {
  int* status;
  int* k;
  int64_t* cell;
  int* row;
  float* l;
  double* t;
};

// is row r of a map the first of its (iz, iy) line?
FD bool ocq_head(const int64_t* __restrict__ tab, int r) { return r == 0 || (tab[r - 1] >> 21) != (tab[r] >> 21); }

// grid (row slabs, maps): *bad = 1 if a map's keys do not ascend strictly or a key is negative (k_oc_prior_check's rule); heads[m][slab]:
// the line heads among the slab's rows (0 for a slab behind the map's rows)
__global__ __launch_bounds__(OCQ_T) void k_ocq_check(OcqMaps mp, int n_slabs, int* __restrict__ bad, int* __restrict__ heads) {
  __shared__ int wsum[OCQ_T / 64];
  const int m = blockIdx.y, t = threadIdx.x, r = blockIdx.x * OCQ_T + t;
  const int64_t* __restrict__ tab = mp.key + (size_t)m * mp.cap;
  bool head = false;
  if (r < mp.nrows[m]) {
    const int64_t k = tab[r];
    if (k < 0 || (r > 0 && tab[r - 1] >= k)) *bad = 1;
    head = ocq_head(tab, r);
  }
  const unsigned long long hh = __ballot(head);
  if ((t & 63) == 0) wsum[t >> 6] = __popcll(hh);
  __syncthreads();
  if (t == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < OCQ_T / 64; w++) c += wsum[w];
    heads[(size_t)m * n_slabs + blockIdx.x] = c;
  }
}

// workgroup b: out[b * stride + i] = the sum of in[b * stride + j] + add over j < i, for i < n, and total[b] that sum over all j (k_oc_scan's
// scheme; `out` may be `in`).  The line heads of a map's slabs become the lines in front of each slab; the maps' lines become the maps'
// first directory slots.
__global__ __launch_bounds__(1024) void k_ocq_scan(const int* in, int add, int n, int stride, int* out, int* __restrict__ total) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int* const v = in + (size_t)blockIdx.x * stride;
  int* const w = out + (size_t)blockIdx.x * stride;
  const int per = (n + 1023) / 1024, lo = min(n, t * per), hi = min(n, lo + per);
  int s = 0;
  for (int i = lo; i < hi; i++) s += v[i] + add;
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int a = 0;
    for (int k = 0; k < 1024; k++) {
      const int c = part[k];
      part[k] = a;
      a += c;
    }
    total[blockIdx.x] = a;
  }
  __syncthreads();
  int a = part[t];
  for (int i = lo; i < hi; i++) {
    const int c = v[i] + add;
    w[i] = a;
    a += c;
  }
}

// k_ocq_check's grid; off[m][slab]: the lines of map m in front of the slab.  A head's slot is a prefix count: nothing is claimed by an atomic.
__global__ __launch_bounds__(OCQ_T) void k_ocq_dir(OcqMaps mp, int n_slabs, const int* __restrict__ off, const int* __restrict__ dptr,
                                                   int64_t* __restrict__ line, int* __restrict__ first) {
  __shared__ int wsum[OCQ_T / 64];
  const int m = blockIdx.y, t = threadIdx.x, r = blockIdx.x * OCQ_T + t, n_rows = mp.nrows[m];
  const int64_t* __restrict__ tab = mp.key + (size_t)m * mp.cap;
  const bool head = r < n_rows && ocq_head(tab, r);
  const unsigned long long hh = __ballot(head);
  if ((t & 63) == 0) wsum[t >> 6] = __popcll(hh);
  __syncthreads();
  if (blockIdx.x == 0 && t == 0) first[dptr[m + 1] - 1] = n_rows;
  if (!head) return;
  int at = dptr[m] + off[(size_t)m * n_slabs + blockIdx.x] + __popcll(hh & ((1ull << (t & 63)) - 1ull));
  for (int w = 0; w < (t >> 6); w++) at += wsum[w];
  line[at] = tab[r] >> 21;
  first[at] = r;
}

// the first index in [lo, hi) with tab[i] >= key, hi if there is none.  Reads indices below hi alone.
FD int ocq_lower(const int64_t* __restrict__ tab, int lo, int hi, int64_t key) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (tab[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// A lane's place in its map.  Plain search (DIR false): nothing is kept, every cell is a search over all rows.  With the directory: the
// current line's slot `j` and rows [r0, r1), and `pos`, the first row of the line at or above the current key -- each a LOWER BOUND, kept
// whether the line or the cell is there or not, so that a step of one along x (the key changes by one) or along y (the line by one) finds
// its lower bound next to the old one with a single load: between k and k + 1 there is no other key.
template <bool DIR>
struct OcqPlace {
  int j = 0, r0 = 0, r1 = 0, pos = 0;
  bool line_ok = false, cell_ok = false;
  // axis: the axis of the step that led to `cell` (-1: the first cell), up: its direction -> the cell's row or -1
  FD int find(const int64_t* __restrict__ tab, int n_rows, const int64_t* __restrict__ dl, const int* __restrict__ df, int nl, int64_t cell,
              int axis, bool up) {
    if (!DIR) {
      const int at = ocq_lower(tab, 0, n_rows, cell);
      return at < n_rows && tab[at] == cell ? at : -1;
    }
    if (axis != 0) {
      const int64_t L = cell >> 21;
      if (axis < 0) j = ocq_lower(dl, 0, nl, L);
      else if (axis == 1) j = up ? j + (line_ok ? 1 : 0) : (j > 0 && dl[j - 1] == L ? j - 1 : j);
      else j = up ? ocq_lower(dl, j + (line_ok ? 1 : 0), nl, L) : ocq_lower(dl, 0, j, L);
      line_ok = j < nl && dl[j] == L;
      if (line_ok) r0 = df[j], r1 = df[j + 1], pos = ocq_lower(tab, r0, r1, cell);
    } else if (line_ok) {
      pos = up ? pos + (cell_ok ? 1 : 0) : (pos > r0 && tab[pos - 1] == cell ? pos - 1 : pos);
    }
    cell_ok = line_ok && pos < r1 && tab[pos] == cell;
    return cell_ok ? pos : -1;
  }
};

// one lane per query; cells[q]: the cells query q tested
template <bool DIR>
__global__ __launch_bounds__(OCQ_T) void k_ocq_cast(OcqMaps mp, OcqDir dir, int n_q, const double* __restrict__ seg, double leaf, float thres,
                                                    int ignore_unknown, int max_cells, OcqOut out, int* __restrict__ cells) {
  const long long q64 = (long long)blockIdx.x * OCQ_T + threadIdx.x;
  if (q64 >= n_q) return;
  const int q = (int)q64;
  int lo = 0, hi = mp.n_maps;  // the last map m with qptr[m] <= q (maps without queries share a start: the last one holds q)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (mp.qptr[mid] <= q) lo = mid;
    else hi = mid;
  }
  const int m = lo, n_rows = mp.nrows[m];
  const int64_t* __restrict__ tab = mp.key + (size_t)m * mp.cap;
  const float* __restrict__ val = mp.l + (size_t)m * mp.cap;
  const int64_t* __restrict__ dl = nullptr;
  const int* __restrict__ df = nullptr;
  int nl = 0;
  if (DIR) dl = dir.line + dir.ptr[m], df = dir.first + dir.ptr[m], nl = dir.ptr[m + 1] - dir.ptr[m] - 1;
  const double* s = seg + 6 * (size_t)q;
  const V3 o{s[0], s[1], s[2]}, p{s[3], s[4], s[5]};
  int iox = 0, ioy = 0, ioz = 0, iex = 0, iey = 0, iez = 0;
  const bool o_ok = oc_cell(o, leaf, iox, ioy, ioz), p_ok = oc_cell(p, leaf, iex, iey, iez);
  int status = OCQ_DROPPED, k = 0, row = -1, tested = 0;
  int64_t cell = -1;
  float l = 0.0f;
  double t = 0.0;
  if (o_ok && p_ok) {
    int rx = abs(iex - iox), ry = abs(iey - ioy), rz = abs(iez - ioz);
    const int sx = iex >= iox ? 1 : -1, sy = iey >= ioy ? 1 : -1, sz = iez >= ioz ? 1 : -1;
    const double dx = p.x - o.x, dy = p.y - o.y, dz = p.z - o.z;
    double tx = 0, ty = 0, tz = 0, ex = 0, ey = 0, ez = 0;
    if (rx > 0) tx = ((double)(iox + (sx > 0 ? 1 : 0)) * leaf - o.x) / dx, ex = leaf / fabs(dx);
    if (ry > 0) ty = ((double)(ioy + (sy > 0 ? 1 : 0)) * leaf - o.y) / dy, ey = leaf / fabs(dy);
    if (rz > 0) tz = ((double)(ioz + (sz > 0 ? 1 : 0)) * leaf - o.z) / dz, ez = leaf / fabs(dz);
    int x = iox, y = ioy, zc = ioz, a = -1;
    OcqPlace<DIR> place;
    for (;;) {  // (every round but the last takes one of the rx + ry + rz steps: the loop cannot run on, whatever the tmax are)
      cell = (int64_t)oc_key(x, y, zc);
      if (max_cells > 0 && k == max_cells) {
        status = OCQ_LIMIT, tested = k;
        break;
      }
      tested = k + 1;
      row = place.find(tab, n_rows, dl, df, nl, cell, a, (a == 0 ? sx : (a == 1 ? sy : sz)) > 0);
      l = row >= 0 ? val[row] : 0.0f;
      if (row >= 0 && l > thres) {
        status = OCQ_OCCUPIED;
        break;
      }
      if (row < 0 && !ignore_unknown) {
        status = OCQ_UNKNOWN;
        break;
      }
      if (rx + ry + rz == 0) {
        status = OCQ_END;
        break;
      }
      a = -1;
      double best = 0;
      if (rx > 0) a = 0, best = tx;
      if (ry > 0 && (a < 0 || ty < best)) a = 1, best = ty;
      if (rz > 0 && (a < 0 || tz < best)) a = 2, best = tz;
      if (a == 0) x += sx, rx--, tx += ex;
      else if (a == 1) y += sy, ry--, ty += ey;
      else zc += sz, rz--, tz += ez;
      t = best;
      row = -1, l = 0.0f;
      k++;
    }
  }
  out.status[q] = status;
  if (out.k) out.k[q] = k;
  if (out.cell) out.cell[q] = cell;
  if (out.row) out.row[q] = row;
  if (out.l) out.l[q] = l;
  if (out.t) out.t[q] = t;
  cells[q] = tested;
}

// one workgroup per map: sums[m][0 .. 4] its queries per status, sums[m][5] its cells tested
__global__ __launch_bounds__(OCQ_T) void k_ocq_sums(const int* __restrict__ qptr, const int* __restrict__ status, const int* __restrict__ cells,
                                                    long long* __restrict__ sums) {
  __shared__ long long red[6][OCQ_T];
  const int m = blockIdx.x, t = threadIdx.x;
  long long v[6] = {0, 0, 0, 0, 0, 0};
  for (int i = qptr[m] + t; i < qptr[m + 1]; i += OCQ_T) {
    const int s = status[i];
#pragma unroll
    for (int c = 0; c < 5; c++) v[c] += s == c ? 1 : 0;
    v[5] += cells[i];
  }
#pragma unroll
  for (int c = 0; c < 6; c++) red[c][t] = v[c];
  __syncthreads();
  for (int d = OCQ_T / 2; d > 0; d >>= 1) {
    if (t < d) {
#pragma unroll
      for (int c = 0; c < 6; c++) red[c][t] += red[c][t + d];
    }
    __syncthreads();
  }
  if (t < 6) sums[6 * (size_t)m + t] = red[t][0];
}

double ocq_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int ocq_check_host(int n_maps, int map_cap, const int64_t* h_n_rows, double leaf, const flvis_occupancy_cast_params* prm, const int* h_q_ptr,
                   std::string& why) {
  auto bad = [&](const std::string& m) { return why = m, FLVIS_ERR_INVALID_ARG; };
  if (!(leaf > 0) || !std::isfinite(leaf)) return bad("leaf must be finite and > 0");
  if (!prm) return bad("NULL cast params");
  if (!std::isfinite(prm->thres)) return bad("thres must be finite");
  if (prm->max_cells < 0) return bad("max_cells < 0");
  if (prm->ignore_unknown != 0 && prm->ignore_unknown != 1) return bad("ignore_unknown must be 0 or 1");
  if (n_maps < 1) return bad("n_maps < 1");
  if (map_cap < 0) return bad("map_cap < 0");
  if (!h_n_rows || !h_q_ptr) return bad("NULL h_n_rows or h_q_ptr");
  for (int m = 0; m < n_maps; m++)
    if (h_n_rows[m] < 0 || h_n_rows[m] > map_cap) return bad("h_n_rows[" + std::to_string(m) + "] is outside [0, map_cap]");
  if (h_q_ptr[0] != 0) return bad("h_q_ptr does not start at 0");
  for (int m = 0; m < n_maps; m++)
    if (h_q_ptr[m + 1] < h_q_ptr[m]) return bad("h_q_ptr descends");
  return FLVIS_OK;
}

bool ocq_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char *x = (const char*)a, *y = (const char*)b;
  return a && b && na > 0 && nb > 0 && x < y + nb && y < x + na;
}

// the call on device arrays; the arguments passed ocq_check_host
int ocq_core(flvis_ctx* ctx, const char* what, int n_maps, const int64_t* d_key, const float* d_l, int map_cap, const int64_t* h_n_rows,
             double leaf, const flvis_occupancy_cast_params* prm, const double* d_seg, const int* h_q_ptr, const OcqOut& out,
             int64_t* h_counts5) {
  const std::string pre = std::string(what) + ": ";
  const int n_q = h_q_ptr[n_maps];
  int max_rows = 0;
  for (int m = 0; m < n_maps; m++) max_rows = std::max(max_rows, (int)h_n_rows[m]);
  memset(ctx->ocq_ms, 0, sizeof(ctx->ocq_ms));
  memset(ctx->ocq_stats, 0, sizeof(ctx->ocq_stats));
  if (h_counts5) memset(h_counts5, 0, sizeof(int64_t) * 5 * (size_t)n_maps);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const bool timing = ctx->dc_timing != 0;
  if (timing) hipStreamSynchronize(st);
  auto t0 = std::chrono::steady_clock::now();
  // ---- workspace: sums [n_maps][6] (int64) | nrows [n_maps] | qptr [n_maps + 1] | dptr [n_maps + 1] | lines [n_maps] | bad [1] |
  //      cells [n_q] | heads [n_maps][n_slabs]   (nrows | qptr: one upload; lines | bad: one download)
  const bool use_dir = ctx->ocq_lookup == 0;
  const int n_slabs = std::max(1, (max_rows + OCQ_T - 1) / OCQ_T);
  const size_t ws_bytes = 8 * 6 * (size_t)n_maps + 4 * (4 * (size_t)n_maps + 3 + (size_t)n_q + (size_t)n_maps * n_slabs);
  uint8_t* const ws = (uint8_t*)ctx->scratch("ocq_rows", ws_bytes);
  auto no_mem = [&]() {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, pre + "device allocation failed");
  };
  if (!ws) return no_mem();
  long long* const d_sums = (long long*)ws;
  int* const d_nrows = (int*)(d_sums + 6 * (size_t)n_maps);
  int* const d_qptr = d_nrows + n_maps;
  int* const d_dptr = d_qptr + n_maps + 1;
  int* const d_lines = d_dptr + n_maps + 1;
  int* const d_bad = d_lines + n_maps;
  int* const d_cells = d_bad + 1;
  int* const d_heads = d_cells + n_q;
  // ---- the line directory: a map's lines and one closing slot, map after map; room for a line per row, so that nothing waits for a count
  long long slots = n_maps;
  for (int m = 0; m < n_maps; m++) slots += h_n_rows[m];
  if (use_dir && slots > INT_MAX) return ctx->fail(FLVIS_ERR_CAPACITY, pre + "2^31 rows or more in the maps of one call");
  OcqDir dir{nullptr, nullptr, d_dptr};
  if (use_dir) {
    uint8_t* const db = (uint8_t*)ctx->scratch("ocq_dir", (size_t)slots * 12);
    if (!db) return no_mem();
    dir = OcqDir{(int64_t*)db, (int*)((int64_t*)db + slots), d_dptr};
  }
  std::vector<int> up(2 * (size_t)n_maps + 1), back((size_t)n_maps + 1, 0);
  for (int m = 0; m < n_maps; m++) up[m] = (int)h_n_rows[m];
  memcpy(up.data() + n_maps, h_q_ptr, sizeof(int) * ((size_t)n_maps + 1));
  auto fail_sync = [&](int code) {  // (`up` and `back` go away on return)
    hipStreamSynchronize(st);
    return code;
  };
  hipError_t e = hipMemcpyAsync(d_nrows, up.data(), sizeof(int) * up.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_lines, 0, sizeof(int) * ((size_t)n_maps + 1), st);
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, what));
  const OcqMaps mp{d_key, d_l, map_cap, n_maps, d_nrows, d_qptr};
  const dim3 rgrid((unsigned)n_slabs, (unsigned)n_maps);
  k_ocq_check<<<rgrid, OCQ_T, 0, st>>>(mp, n_slabs, d_bad, d_heads);
  if (use_dir) {
    k_ocq_scan<<<n_maps, 1024, 0, st>>>(d_heads, 0, n_slabs, n_slabs, d_heads, d_lines);
    k_ocq_scan<<<1, 1024, 0, st>>>(d_lines, 1, n_maps, 0, d_dptr, d_dptr + n_maps);
    k_ocq_dir<<<rgrid, OCQ_T, 0, st>>>(mp, n_slabs, d_heads, d_dptr, (int64_t*)dir.line, (int*)dir.first);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(back.data(), d_lines, sizeof(int) * back.size(), hipMemcpyDeviceToHost, st);
  {
    const hipError_t e2 = hipStreamSynchronize(st);  // (behind it `up` may go)
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, (pre + "key check").c_str());
  if (back[n_maps]) return ctx->fail(FLVIS_ERR_INVALID_ARG, pre + "a map's keys are not valid keys in strictly ascending order");
  ctx->ocq_stats[0] = n_q;
  ctx->ocq_stats[3] = (int64_t)ws_bytes + (use_dir ? slots * 12 : 0);
  if (use_dir) {
    long long used = n_maps;
    for (int m = 0; m < n_maps; m++) used += back[m];
    ctx->ocq_stats[2] = used * 12 + 4 * (int64_t)n_maps * n_slabs;
  }
  if (timing) ctx->ocq_ms[0] = ocq_ms_since(t0), t0 = std::chrono::steady_clock::now();
  if (n_q == 0) return FLVIS_OK;
  const unsigned qgrid = (unsigned)(((size_t)n_q + OCQ_T - 1) / OCQ_T);
  if (use_dir) k_ocq_cast<true><<<qgrid, OCQ_T, 0, st>>>(mp, dir, n_q, d_seg, leaf, prm->thres, prm->ignore_unknown, prm->max_cells, out, d_cells);
  else k_ocq_cast<false><<<qgrid, OCQ_T, 0, st>>>(mp, dir, n_q, d_seg, leaf, prm->thres, prm->ignore_unknown, prm->max_cells, out, d_cells);
  k_ocq_sums<<<n_maps, OCQ_T, 0, st>>>(d_qptr, out.status, d_cells, d_sums);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_sync(ctx->hip_fail(e, (pre + "walk").c_str()));
  std::vector<long long> sums(6 * (size_t)n_maps);
  e = hipMemcpyAsync(sums.data(), d_sums, sizeof(long long) * sums.size(), hipMemcpyDeviceToHost, st);
  {
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, (pre + "walk").c_str());
  if (timing) ctx->ocq_ms[1] = ocq_ms_since(t0);
  for (int m = 0; m < n_maps; m++) {
    for (int c = 0; h_counts5 && c < 5; c++) h_counts5[5 * (size_t)m + c] = sums[6 * (size_t)m + c];
    ctx->ocq_stats[1] += sums[6 * (size_t)m + 5];
  }
  return FLVIS_OK;
}

}  // namespace

extern "C" {

void flvis_occupancy_cast_params_default(flvis_occupancy_cast_params* p) {
  if (!p) return;
  p->thres = 0.0f, p->ignore_unknown = 0, p->max_cells = 0;
}

int flvis_occupancy_cast_check(int n_maps, int map_cap, const int64_t* h_n_rows, double leaf, const flvis_occupancy_cast_params* prm,
                               const int* h_q_ptr) {
  std::string why;
  return ocq_check_host(n_maps, map_cap, h_n_rows, leaf, prm, h_q_ptr, why);
}

int flvis_hip_occupancy_cast(flvis_ctx* ctx, int n_maps, const int64_t* d_key, const float* d_l, int map_cap, const int64_t* h_n_rows, double leaf,
                             const flvis_occupancy_cast_params* prm, const double* d_seg, const int* h_q_ptr, int* d_status, int* d_k,
                             int64_t* d_cell, int* d_row, float* d_l_out, double* d_t, int64_t* h_counts5) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, "occupancy_cast: " + m); };
  std::string why;
  const int rc = ocq_check_host(n_maps, map_cap, h_n_rows, leaf, prm, h_q_ptr, why);
  if (rc != FLVIS_OK) return ctx->fail(rc, "occupancy_cast: " + why);
  bool any_rows = false;
  for (int m = 0; m < n_maps; m++) any_rows = any_rows || h_n_rows[m] > 0;
  if (any_rows && (!d_key || !d_l)) return bad("NULL d_key or d_l with a non-empty map");
  const size_t n_q = (size_t)h_q_ptr[n_maps], rows = (size_t)n_maps * (size_t)map_cap;
  if (n_q > 0 && (!d_seg || !d_status)) return bad("NULL d_seg or d_status with a query");
  const void* outs[6] = {d_status, d_k, d_cell, d_row, d_l_out, d_t};
  const size_t out_bytes[6] = {4 * n_q, 4 * n_q, 8 * n_q, 4 * n_q, 4 * n_q, 8 * n_q};
  for (int a = 0; a < 6; a++) {
    if (ocq_overlap(outs[a], out_bytes[a], d_key, 8 * rows) || ocq_overlap(outs[a], out_bytes[a], d_l, 4 * rows) ||
        ocq_overlap(outs[a], out_bytes[a], d_seg, 48 * n_q))
      return bad("an output overlaps a map or the segments");
    for (int b = a + 1; b < 6; b++)
      if (ocq_overlap(outs[a], out_bytes[a], outs[b], out_bytes[b])) return bad("two outputs overlap");
  }
  return ocq_core(ctx, "occupancy_cast", n_maps, d_key, d_l, map_cap, h_n_rows, leaf, prm, d_seg, h_q_ptr,
                  OcqOut{d_status, d_k, d_cell, d_row, d_l_out, d_t}, h_counts5);
}

int flvis_hip_occupancy_cast_host(flvis_ctx* ctx, int n_maps, const int64_t* d_key, const float* d_l, int map_cap, const int64_t* h_n_rows,
                                  double leaf, const flvis_occupancy_cast_params* prm, const double* h_seg, const int* h_q_ptr, int* h_status,
                                  int* h_k, int64_t* h_cell, int* h_row, float* h_l_out, double* h_t, int64_t* h_counts5) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  const char* what = "occupancy_cast_host";
  auto bad = [&](const std::string& m) { return ctx->fail(FLVIS_ERR_INVALID_ARG, std::string(what) + ": " + m); };
  std::string why;
  int rc = ocq_check_host(n_maps, map_cap, h_n_rows, leaf, prm, h_q_ptr, why);
  if (rc != FLVIS_OK) return ctx->fail(rc, std::string(what) + ": " + why);
  bool any_rows = false;
  for (int m = 0; m < n_maps; m++) any_rows = any_rows || h_n_rows[m] > 0;
  if (any_rows && (!d_key || !d_l)) return bad("NULL d_key or d_l with a non-empty map");
  const size_t n_q = (size_t)h_q_ptr[n_maps];
  if (n_q > 0 && (!h_seg || !h_status)) return bad("NULL h_seg or h_status with a query");
  // ---- staged: seg [n_q][6] | t [n_q] | cell [n_q] (8 bytes each) | status | k | row | l [n_q] (4 bytes each)
  const size_t nq1 = std::max<size_t>(n_q, 1);
  uint8_t* const sb = (uint8_t*)ctx->scratch("ocq_host_rows", nq1 * (48 + 2 * 8 + 4 * 4));
  if (!sb) {
    (void)hipGetLastError();
    return ctx->fail(FLVIS_ERR_HIP, std::string(what) + ": device allocation failed");
  }
  double* const s_seg = (double*)sb;
  double* const s_t = s_seg + 6 * nq1;
  int64_t* const s_cell = (int64_t*)(s_t + nq1);
  int* const s_status = (int*)(s_cell + nq1);
  int* const s_k = s_status + nq1;
  int* const s_row = s_k + nq1;
  float* const s_l = (float*)(s_row + nq1);
  hipSetDevice(ctx->device);
  hipError_t e = hipSuccess;
  if (n_q > 0) {
    e = hipMemcpyAsync(s_seg, h_seg, 48 * n_q, hipMemcpyHostToDevice, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);  // (the caller's array may be pageable: behind this it is read)
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return ctx->hip_fail(e, what);
  }
  rc = ocq_core(ctx, what, n_maps, d_key, d_l, map_cap, h_n_rows, leaf, prm, s_seg, h_q_ptr,
                OcqOut{s_status, h_k ? s_k : nullptr, h_cell ? s_cell : nullptr, h_row ? s_row : nullptr, h_l_out ? s_l : nullptr,
                       h_t ? s_t : nullptr},
                h_counts5);
  if (rc != FLVIS_OK || n_q == 0) return rc;
  e = hipMemcpyAsync(h_status, s_status, 4 * n_q, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && h_k) e = hipMemcpyAsync(h_k, s_k, 4 * n_q, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && h_cell) e = hipMemcpyAsync(h_cell, s_cell, 8 * n_q, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && h_row) e = hipMemcpyAsync(h_row, s_row, 4 * n_q, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && h_l_out) e = hipMemcpyAsync(h_l_out, s_l, 4 * n_q, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && h_t) e = hipMemcpyAsync(h_t, s_t, 8 * n_q, hipMemcpyDeviceToHost, ctx->stream);
  {
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return ctx->hip_fail(e, what);
  return FLVIS_OK;
}

int flvis_hip_occupancy_cast_lookup(flvis_ctx* ctx, int lookup) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (lookup != 0 && lookup != 1) return ctx->fail(FLVIS_ERR_INVALID_ARG, "occupancy_cast_lookup: 0 (line directory) or 1 (plain search)");
  ctx->ocq_lookup = lookup;
  return FLVIS_OK;
}

int flvis_hip_occupancy_cast_stats(flvis_ctx* ctx, int64_t* h_stats4, double* h_ms2) {
  if (!ctx) return FLVIS_ERR_INVALID_ARG;
  if (h_stats4) memcpy(h_stats4, ctx->ocq_stats, sizeof(ctx->ocq_stats));
  if (h_ms2) memcpy(h_ms2, ctx->ocq_ms, sizeof(ctx->ocq_ms));
  return FLVIS_OK;
}

}  // extern "C"
