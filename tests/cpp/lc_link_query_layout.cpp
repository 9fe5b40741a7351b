// Prints the layout of flvis_lc_link_query, and the sizes of the structs flvis_loop_closer_link fills, as a C++ caller of
// include/flvis_hip.h sees them: "query.sizeof N", one "query.field offset" line per member, "fix_in.sizeof N", "link.sizeof N"
// (tests/test_loop_link_abi.py compares them with the ctypes harness).  Header only: nothing is linked.
#include <cstddef>
#include <cstdio>

#include "flvis_hip.h"

#define QUERY(f) std::printf("query." #f " %zu\n", offsetof(flvis_lc_link_query, f))

int main() {
  std::printf("query.sizeof %zu\n", sizeof(flvis_lc_link_query));
  QUERY(stream);
  QUERY(map);
  QUERY(kf);
  QUERY(own_gap);
  std::printf("fix_in.sizeof %zu\n", sizeof(flvis_lc_fix_in));
  std::printf("link.sizeof %zu\n", sizeof(flvis_lc_link));
  return 0;
}
