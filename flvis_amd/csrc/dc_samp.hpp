// flvis_amd: the sampling of the dense calls -- which pixels of a listed image are samples, which samples are valid, and how a workgroup
// walks them -- shared by the dense cloud (depth_cloud.hip) and the occupancy map (occupancy.hip): both read the same samples in the same
// raster order by these functions.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/flvis_hip.h"
#include "dev_math.hpp"

namespace flvis {

constexpr int DC_T = 256;
constexpr int DC_CHUNK = 4096;  // samples per workgroup, in whole sampled rows (a row wider than this is a chunk of its own)

// the sampling of a call with the window's defaults filled in: nu x nv samples per image, chunk_rows sampled rows per workgroup
struct DcSamp {
  int u0, v0, su, sv, nu, nv, chunk_rows, chunks, w, h;
  double z_min, z_max;
  int packed;  // the images hold the samples alone, [nv][nu] (the stereo forms: dense_stereo.hip writes them so), not [h][w]
  __host__ __device__ size_t img_px() const { return packed ? (size_t)nu * nv : (size_t)w * h; }
};

// the tracker's depth rule (track_kernels.hip, the depth arm of the landmark depth kernel): metres = Z16 / depth_factor narrowed to float
FD bool dc_valid(uint16_t raw, double depth_factor, const DcSamp& s, float& z) {
  z = (float)((double)raw / depth_factor);
  return (double)z >= s.z_min && (double)z <= s.z_max;
}

// sample j of chunk c (raster order inside the chunk): its pixel -> where the image holds it
FD size_t dc_pixel(const DcSamp& s, int c, int j, int& u, int& v) {
  const int jr = j / s.nu, ji = j - jr * s.nu, iv = c * s.chunk_rows + jr;
  u = s.u0 + ji * s.su;
  v = s.v0 + iv * s.sv;
  return s.packed ? (size_t)iv * s.nu + ji : (size_t)v * s.w + u;
}
FD int dc_chunk_samples(const DcSamp& s, int c) { return (min(s.nv, (c + 1) * s.chunk_rows) - c * s.chunk_rows) * s.nu; }

inline int dc_resolve(int w, int h, const flvis_depth_cloud_params* prm, DcSamp& s, std::string& why) {
  if (!prm) return why = "NULL params", FLVIS_ERR_INVALID_ARG;
  if (w <= 0 || h <= 0) return why = "the image shape must be positive", FLVIS_ERR_INVALID_ARG;
  if (prm->step_u < 1 || prm->step_v < 1) return why = "a step below 1", FLVIS_ERR_INVALID_ARG;
  const int u1 = prm->u1 <= 0 ? w : prm->u1, v1 = prm->v1 <= 0 ? h : prm->v1;
  if (prm->u0 < 0 || prm->v0 < 0 || u1 > w || v1 > h || prm->u0 >= u1 || prm->v0 >= v1)
    return why = "the window is empty or not inside the image", FLVIS_ERR_INVALID_ARG;
  if (!std::isfinite(prm->z_min) || !std::isfinite(prm->z_max) || prm->z_min > prm->z_max)
    return why = "the z limits must be finite with z_min <= z_max", FLVIS_ERR_INVALID_ARG;
  s.u0 = prm->u0, s.v0 = prm->v0, s.su = prm->step_u, s.sv = prm->step_v, s.w = w, s.h = h;
  s.nu = (int)(((long long)u1 - prm->u0 + prm->step_u - 1) / prm->step_u);  // (the last sample is u0 + (nu - 1) * step_u < u1 <= w)
  s.nv = (int)(((long long)v1 - prm->v0 + prm->step_v - 1) / prm->step_v);
  s.chunk_rows = std::max(1, DC_CHUNK / s.nu);
  s.chunks = (s.nv + s.chunk_rows - 1) / s.chunk_rows;
  s.z_min = prm->z_min, s.z_max = prm->z_max;
  s.packed = 0;
  return FLVIS_OK;
}

}  // namespace flvis
