// flvis_amd: the descent of Vocabulary::transform(feature, word_id) (3rdPartLib/DBow3/src/Vocabulary.cpp:836-874) through a
// vocabulary resident on the device: from the root to the FIRST child of minimal Hamming distance until a leaf is reached.  Shared by
// the bag-of-words transform (loop_kernels.hip) and the node weights of the training (voc_train.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace flvis {

struct VocDev {
  const int* child_ptr;
  const int* child_idx;
  const uint8_t* desc;      // [n_nodes][32]
  const int* word_id;       // per node (leaves)
  const double* weight;     // per node (leaves: idf)
  const double* word_weight;  // per word id
  int n_nodes, n_words;
  int depth;  // levels below the root (bounds the descent)
};

__device__ inline int hamming256(const uint4 a0, const uint4 a1, const uint8_t* b) {
  const uint4* q = reinterpret_cast<const uint4*>(b);
  const uint4 b0 = q[0], b1 = q[1];
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// the node the descriptor (f0, f1) ends at; leaf = false when no leaf was reached within v.depth levels (only trees are accepted as
// vocabularies, so the descent ends after at most `depth` levels; the bound keeps a corrupted table from hanging the GPU)
__device__ inline int voc_descend(const VocDev& v, const uint4 f0, const uint4 f1, bool& leaf) {
  int node = 0;
  leaf = false;
  for (int level = 0; level <= v.depth; level++) {
    const int c0 = v.child_ptr[node], c1 = v.child_ptr[node + 1];
    if (c0 == c1) {
      leaf = true;
      break;
    }
    int best_d = INT_MAX, best = node;
    for (int c = c0; c < c1; c++) {
      const int id = v.child_idx[c];
      const int d = hamming256(f0, f1, v.desc + (size_t)id * 32);
      if (d < best_d) {
        best_d = d;
        best = id;
      }
    }
    node = best;
  }
  return node;
}

}  // namespace flvis
