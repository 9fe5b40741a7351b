// flvis_amd: a DBoW3 vocabulary on the host -- what flvis_voc_file_open reads (voc_file.cpp) and flvis_hip_voc_train builds
// (voc_train.hip): the flat arrays flvis_hip_bow_set_vocabulary takes.
#pragma once
#include <cstdint>
#include <vector>

struct flvis_voc_file {
  int k = 0, L = 0, scoring = 0, weighting = 0, format = 0;  // format: info8.layout (0 .. 3 the file's layout, 4 trained)
  int n_nodes = 0, n_words = 0;
  std::vector<int> child_ptr, child_idx, word_id;
  std::vector<uint8_t> desc;
  std::vector<double> weight;
};
