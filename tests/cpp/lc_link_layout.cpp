// Prints the layouts of flvis_lc_link and flvis_lc_merge as a C++ caller of include/flvis_hip.h sees them: "link.sizeof N" /
// "merge.sizeof N" and one "struct.field offset" line per member (tests/test_loop_merge_abi.py compares them with the ctypes harness'
// FlvisLcLink and FlvisLcMerge).  Header only: nothing is linked.
#include <cstddef>
#include <cstdio>

#include "flvis_hip.h"

#define LINK(f) std::printf("link." #f " %zu\n", offsetof(flvis_lc_link, f))
#define MERGE(f) std::printf("merge." #f " %zu\n", offsetof(flvis_lc_merge, f))

int main() {
  std::printf("link.sizeof %zu\n", sizeof(flvis_lc_link));
  LINK(seq_from);
  LINK(seq_to);
  LINK(kf_from);
  LINK(kf_to);
  LINK(pose7);
  std::printf("merge.sizeof %zu\n", sizeof(flvis_lc_merge));
  MERGE(optimised);
  MERGE(n_vertices);
  MERGE(n_edges);
  MERGE(iterations);
  MERGE(chi2_before);
  MERGE(chi2_after);
  return 0;
}
