// Prints the layout of flvis_lc_fix as a C++ caller of include/flvis_hip.h sees it: "sizeof N" and one "field offset" line per member
// (tests/test_loop_localize_abi.py compares them with the ctypes harness' FlvisLcFix).  Header only: nothing is linked.
#include <cstddef>
#include <cstdio>

#include "flvis_hip.h"

#define FIELD(f) std::printf(#f " %zu\n", offsetof(flvis_lc_fix, f))

int main() {
  std::printf("sizeof %zu\n", sizeof(flvis_lc_fix));
  std::printf("FLVIS_LC_FIX_CAND %d\n", FLVIS_LC_FIX_CAND);
  FIELD(n_landmarks);
  FIELD(n_candidates);
  FIELD(best);
  FIELD(reserved);
  FIELD(cand_kf);
  FIELD(cand_score);
  FIELD(cand_matches);
  FIELD(cand_inliers);
  FIELD(cand_accepted);
  FIELD(cand_pose7);
  FIELD(T_c_map7);
  return 0;
}
