// Prints the layout of flvis_lc_fix_in as a C++ caller of include/flvis_hip.h sees it: "sizeof N" and one "field offset" line per member
// (tests/test_loop_localize_in_abi.py compares them with the ctypes harness' FlvisLcFixIn).  Header only: nothing is linked.
#include <cstddef>
#include <cstdio>

#include "flvis_hip.h"

#define FIELD(f) std::printf(#f " %zu\n", offsetof(flvis_lc_fix_in, f))

int main() {
  std::printf("sizeof %zu\n", sizeof(flvis_lc_fix_in));
  std::printf("sizeof_fix %zu\n", sizeof(flvis_lc_fix));
  std::printf("FLVIS_LC_ALL_MAPS %d\n", FLVIS_LC_ALL_MAPS);
  FIELD(fix);
  FIELD(cand_seq);
  FIELD(map);
  FIELD(reserved);
  return 0;
}
