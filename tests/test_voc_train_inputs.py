"""CPU: the inputs of the vocabulary-training tests (tests/test_gpu_voc_train.py) and the definition they are checked against
(tests/_voc_train.py).  No product code runs here: the restatement reports how often each branch of the algorithm ran per input, and
every branch the GPU tests rely on must have run; and at L = 1 the per-node random streams are DBoW3's one stream after srand(seed)."""
import numpy as np
import pytest

import _voc as V
import _voc_train as T


@pytest.fixture(scope="module")
def runs():
    return {
        "8x300..500 k10 L3": [T.train(V.make_keyframes(s, n_img=8, per_img=(300, 500)), 10, 3, seed=1) for s in (1, 2, 3)],
        "6x60..90 k4 L3": T.train(V.make_keyframes(1, n_img=6, per_img=(60, 90)), 4, 3, seed=1),
        "4x20..40 k3 L4": T.train(V.make_keyframes(1, n_img=4, per_img=(20, 40)), 3, 4, seed=1),
    }


def test_the_deep_inputs_reach_ties_empty_clusters_and_trivial_nodes(runs):
    for r in runs["8x300..500 k10 L3"]:
        c = r["counts"]
        assert c["assign_ties"] > 1000 and c["majority_ties"] > 0 and c["empty_kept"] > 0 and c["trivial"] > 0, c
        assert r["stats"][5] > 0 and r["stats"][6] == c["trivial"] and r["stats"][4] == 0
    c = runs["6x60..90 k4 L3"]["counts"]
    assert c["assign_ties"] > 0 and c["majority_ties"] > 0 and c["empty_kept"] > 0 and c["trivial"] == 0, c
    r = runs["4x20..40 k3 L4"]
    assert r["counts"]["trivial"] > 0 and r["counts"]["assign_ties"] > 0
    # leaves above level L (single-descriptor children that are not split): some word lies less than L levels below the root
    child_ptr, child_idx = r["arrays"][0], r["arrays"][1]
    depth = np.zeros(len(child_ptr) - 1, int)
    for n in range(len(depth)):
        depth[child_idx[child_ptr[n]:child_ptr[n + 1]]] = depth[n] + 1
    leaf = np.diff(child_ptr) == 0
    assert depth[leaf].min() < 4 and depth.max() == 4


def test_the_passes_stay_far_below_the_default_cap(runs):
    # departure (b): max_iters = 100 by default; these inputs converge in a handful of passes per node
    for r in runs["8x300..500 k10 L3"]:
        n_kmeans = r["stats"][1] - r["stats"][2] - r["stats"][6]       # inner nodes less the trivially split: the nodes that ran k-means
        assert r["stats"][4] == 0 and r["stats"][3] <= 12 * n_kmeans


def test_the_cap_is_hit_at_one_and_two_passes():
    kfs = V.make_keyframes(1, n_img=8, per_img=(300, 500))
    for cap in (1, 2):
        r = T.train(kfs, 10, 3, seed=1, max_iters=cap)
        assert r["counts"]["capped"] > 0 and r["stats"][4] == r["counts"]["capped"]


def test_duplicates_stop_the_seeding_early():
    r = T.train(T.duplicate_node(4), 4, 3, seed=1)
    assert r["counts"]["seed_early_stop"] > 0 and r["counts"]["trivial"] == 0
    assert r["arrays"][0][1] == 2                                   # two distinct descriptors: two clusters under the root
    same = [np.tile(np.arange(32, dtype=np.uint8), (300, 1))]
    r = T.train(same, 4, 3, seed=1)
    assert r["counts"]["seed_early_stop"] == 3
    assert r["arrays"][0].tolist() == [0, 1, 2, 3, 3]               # a single-child chain down to level L
    assert r["stats"][:3] == [300, 4, 1]


def test_an_empty_image_still_counts_as_a_document():
    kfs = V.make_keyframes(2, n_img=4, per_img=(41, 60))
    images = [kfs[0][:40], np.zeros((0, 32), np.uint8), kfs[2][:33], kfs[3][:40]]
    r = T.train(images, 3, 2, seed=1)
    assert r["ndocs"] == 4 and 0 < r["ni"].min() and r["ni"].max() <= 3
    leaf = np.diff(r["arrays"][0]) == 0
    assert np.all(r["arrays"][3][leaf] >= np.log(4.0 / 3.0))           # NDocs = 4: even a word seen in all three images has a weight
    assert np.all(T.train(images, 3, 2, seed=1, weighting=1)["arrays"][3][leaf] == 1.0)


@pytest.mark.parametrize("k", [2, 3, 10])
@pytest.mark.parametrize("seed", [1, 7])
def test_one_level_is_dbow3_create_after_srand(k, seed):
    """departure (a) changes nothing at L = 1: a straight transcription of HKmeansStep + initiateClustersKMpp on ONE libc stream seeded
    with srand(seed) gives the centres of the per-node rule (the root is node 0: srand(seed + 0))"""
    feats = np.concatenate(V.make_keyframes(4, n_img=2, per_img=(100, 130)))
    want = T.create_one_level(feats, k, seed)
    got = T.train([feats], k, 1, seed=seed)
    assert np.array_equal(got["arrays"][2][1:], want)
    assert got["arrays"][0].tolist() == [0] + [len(want)] * (len(want) + 1)
    assert got["arrays"][4].tolist() == [-1] + list(range(len(want)))
    few = feats[:k]                                                  # n <= k: no random number, one cluster per descriptor
    assert np.array_equal(T.train([few], k, 1, seed=seed)["arrays"][2][1:], T.create_one_level(few, k, seed))
