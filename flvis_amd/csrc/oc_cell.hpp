// flvis_amd: a point's voxel and a voxel's key, shared by the occupancy map (occupancy.hip) and its queries (occupancy_query.hip): both
// name a cell by these functions, so a query finds the cell a ray of the map wrote.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dev_math.hpp"
#include "map_cloud.hpp"

namespace flvis {

// floor(x / leaf) as mc_key computes it; false: not finite or outside [-2^20, 2^20)
FD bool oc_index(double x, double leaf, int& i) {
  const double f = floor(x / leaf);
  if (!(f >= -MC_HALF_RANGE && f < MC_HALF_RANGE)) return false;
  i = (int)f;
  return true;
}
FD bool oc_cell(V3 p, double leaf, int& ix, int& iy, int& iz) {
  const bool a = oc_index(p.x, leaf, ix), b = oc_index(p.y, leaf, iy), c = oc_index(p.z, leaf, iz);
  return a && b && c;
}
FD uint64_t oc_key(int ix, int iy, int iz) {
  return ((uint64_t)(iz + (1 << 20)) << 42) | ((uint64_t)(iy + (1 << 20)) << 21) | (uint64_t)(ix + (1 << 20));
}

}  // namespace flvis
