"""GPU: the vocabulary training (flvis_hip_voc_train, DBoW3's Vocabulary::create on the device) against the independent numpy
restatement of tests/_voc_train.py -- EXACTLY: the tree (child_ptr, child_idx), every node descriptor, the word ids, which words
have a weight, and the counters; the weights within 1 ulp of math.log(NDocs / Ni).  tests/test_voc_train_inputs.py shows on the CPU
that these inputs reach the ties, empty clusters, trivial nodes, early seeding stops and capped nodes the comparison relies on."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _voc as V
import _voc_train as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _batch(images, cap, counts=None):
    import torch
    d = np.zeros((len(images), cap, 32), np.uint8)
    cnt = np.zeros(len(images), np.int32)
    for i, im in enumerate(images):
        m = min(len(im), cap)
        d[i, :m] = im[:m]
        cnt[i] = len(im)
    if counts is not None:
        cnt[:] = counts
    return torch.from_numpy(d).cuda(), torch.from_numpy(cnt).cuda()


def _images(feats, per=700):
    return [feats[i:i + per] for i in range(0, len(feats), per)]


def _check(got, want, what=""):
    a = got.info
    child_ptr, child_idx, desc, weight, word_id = want["arrays"]
    assert np.array_equal(a["child_ptr"], child_ptr), what
    assert np.array_equal(a["child_idx"], child_idx), what
    assert np.array_equal(a["desc"], desc), what
    assert np.array_equal(a["word_id"], word_id), what
    assert a["n_words"] == want["stats"][2] and a["layout"] == "trained" and a["scoring"] == 0
    assert np.array_equal(a["weight"] != 0, weight != 0), what                   # the Ni-derived pattern: Ni = 0 and Ni = NDocs give 0
    assert np.all(np.abs(a["weight"] - weight) <= np.spacing(np.abs(weight))), what
    assert [got.stats[k] for k in got.STATS[:7]] == want["stats"], (what, got.stats, want["stats"])
    assert got.stats["launches"] > 0


def _train(ctx, images, k, L, cap=None, counts=None, **kw):
    cap = cap or max(64, max(len(i) for i in images))
    desc, cnt = _batch(images, cap, counts)
    v = ctx.voc_train(desc, cnt, k=k, L=L, **kw)
    return v


@pytest.fixture(scope="module")
def pool():
    return np.concatenate(V.make_keyframes(5, n_img=6, per_img=(350, 420)))


@pytest.fixture(scope="module")
def big():
    kfs = V.make_keyframes(1, n_img=8, per_img=(300, 500))
    return kfs, T.train(kfs, 10, 3, seed=1)


@pytest.mark.parametrize("seed", [1, 7])
@pytest.mark.parametrize("k", [2, 3, 10])
def test_one_level_trees_at_the_wave_workgroup_and_threshold_edges(ctx, pool, k, seed):
    for n in (63, 64, 65, 255, 256, 257, 2047, 2049):
        images = _images(pool[:n])
        got = _train(ctx, images, k, 1, seed=seed)
        _check(got, T.train(images, k, 1, seed=seed), (k, seed, n))
        assert got.stats["nodes"] == k + 1 and got.stats["passes"] >= 2 and got.stats["trivial"] == 0
        got.close()


@pytest.mark.parametrize("n_img,per,k,L", [(6, (60, 90), 4, 3), (8, (300, 500), 10, 3), (4, (20, 40), 3, 4)])
def test_deep_trees(ctx, n_img, per, k, L):
    kfs = V.make_keyframes(1, n_img=n_img, per_img=per)
    got = _train(ctx, kfs, k, L, seed=1)
    _check(got, T.train(kfs, k, L, seed=1))
    got.close()


@pytest.mark.parametrize("small_node_max", [1, 64, 0, 1 << 20])
def test_both_paths_give_the_same_tree(ctx, big, small_node_max):
    kfs, want = big
    got = _train(ctx, kfs, 10, 3, seed=1, small_node_max=small_node_max)
    _check(got, want, small_node_max)
    got.close()


def test_launches_for_small_nodes_do_not_grow_with_the_node_count(ctx, big):
    kfs, want = big
    a = _train(ctx, kfs, 10, 3, seed=1, small_node_max=1 << 20)
    # everything resident: the gather, one launch per level, the weights
    assert a.stats["launches"] == 1 + 3 + 1 and a.stats["nodes"] > 400
    a.close()


def test_identical_descriptors_give_a_single_child_chain(ctx):
    same = [np.tile(np.arange(32, dtype=np.uint8), (300, 1))]
    want = T.train(same, 4, 3, seed=1)
    for snm in (0, 1):
        got = _train(ctx, same, 4, 3, seed=1, small_node_max=snm)
        _check(got, want, snm)
        assert got.info["child_ptr"].tolist() == [0, 1, 2, 3, 3]
        got.close()


def test_duplicates_stop_the_seeding_early(ctx):
    node = T.duplicate_node(4)
    want = T.train(node, 4, 3, seed=1)
    assert want["counts"]["seed_early_stop"] > 0
    for snm in (0, 1):
        got = _train(ctx, node, 4, 3, seed=1, small_node_max=snm)
        _check(got, want, snm)
        got.close()


def test_empty_and_overfull_counts_and_a_larger_cap(ctx):
    kfs = V.make_keyframes(2, n_img=4, per_img=(41, 60))
    # a buffer of cap 40 whose counts run over (reads as cap), are 0 or negative (reads as 0; the rows behind are not descriptors)
    for c1 in (0, -5):
        counts = [len(kfs[0]), c1, 33, 1000]
        desc, cnt = _batch(kfs, 40, counts=counts)
        images = [kfs[0][:40], np.zeros((0, 32), np.uint8), kfs[2][:33], kfs[3][:40]]
        want = T.train(images, 3, 2, seed=1)
        assert want["ndocs"] == 4 and want["ni"].max() <= 3                  # the empty image counts in NDocs: no word has weight 0
        got = ctx.voc_train(desc, cnt, k=3, L=2, seed=1)
        _check(got, want, c1)
        assert np.all(got.info["weight"][got.info["word_id"] >= 0] > 0)
        got.close()
    # the same descriptors in a buffer with a larger cap: the same tree
    a = _train(ctx, images, 3, 2, cap=64, seed=1)
    b = _train(ctx, images, 3, 2, cap=2048, seed=1)
    _check(a, want)
    _check(b, want)
    a.close()
    b.close()
    tf = _train(ctx, images, 3, 2, cap=64, seed=1, weighting=1)
    _check(tf, T.train(images, 3, 2, seed=1, weighting=1))
    assert tf.info["weighting"] == 1 and np.all(tf.info["weight"][tf.info["word_id"] >= 0] == 1.0)
    tf.close()


@pytest.mark.parametrize("max_iters", [1, 2])
def test_the_iteration_cap(ctx, big, max_iters):
    kfs, _ = big
    want = T.train(kfs, 10, 3, seed=1, max_iters=max_iters)
    for snm in (0, 64):
        got = _train(ctx, kfs, 10, 3, seed=1, max_iters=max_iters, small_node_max=snm)
        _check(got, want, snm)
        assert got.stats["capped"] > 0
        got.close()


def test_refusals_write_nothing_and_two_runs_are_bit_identical(ctx, big):
    import torch
    import flvis_amd
    lib = flvis_amd.load_library()
    kfs, _ = big
    desc, cnt = _batch(kfs[:2], 512)
    SENT = 0x5A5A5A5A

    def call(d=desc, c=cnt, cap=512, n_img=2, prm=(10, 3, 0, 1, 0, 0), no_prm=False, no_out=False):
        p = flvis_amd.VocTrainParams(*prm)
        h = C.c_void_p(SENT)
        stats = (C.c_int64 * 8)(*([SENT] * 8))
        rc = lib.flvis_hip_voc_train(ctx._h, C.c_void_p(d.data_ptr()) if d is not None else None,
                                     C.c_void_p(c.data_ptr()) if c is not None else None, cap, n_img, None if no_prm else C.byref(p),
                                     None if no_out else C.byref(h), stats)
        return rc, h.value, list(stats)

    zero = torch.zeros_like(cnt)
    cases = [dict(d=None), dict(c=None), dict(no_prm=True), dict(no_out=True), dict(prm=(1, 3, 0, 1, 0, 0)), dict(prm=(65, 3, 0, 1, 0, 0)),
             dict(prm=(10, 0, 0, 1, 0, 0)), dict(prm=(10, 11, 0, 1, 0, 0)), dict(cap=0), dict(cap=-3), dict(cap=2049), dict(n_img=0),
             dict(n_img=-1), dict(c=zero), dict(c=zero - 4)]
    for kw in cases:
        rc, h, stats = call(**kw)
        assert rc == flvis_amd.FLVIS_ERR_INVALID_ARG, kw
        assert stats == [SENT] * 8 and h == SENT, kw                          # neither the handle nor the counters are touched
    assert lib.flvis_hip_voc_train(None, None, None, 1, 1, None, None, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    # more images than the gather's grid has rows: FLVIS_ERR_CAPACITY (-4), before the counts are even read
    rc, h, stats = call(c=torch.ones(65536, dtype=torch.int32, device="cuda"), n_img=65536)
    assert rc == -4 and stats == [SENT] * 8 and h == SENT
    a = ctx.voc_train(desc, cnt, k=10, L=3, seed=1)
    b = ctx.voc_train(desc, cnt, k=10, L=3, seed=1)
    for key in ("child_ptr", "child_idx", "desc", "word_id"):
        assert np.array_equal(a.info[key], b.info[key]), key
    assert np.array_equal(a.info["weight"].view(np.uint64), b.info["weight"].view(np.uint64)) and a.stats == b.stats
    c = ctx.voc_train(desc, cnt, k=10, L=3, seed=2)
    assert not np.array_equal(a.info["desc"], c.info["desc"])                 # the seed matters
    for v in (a, b, c):
        v.close()


def test_trained_vocabulary_in_use(ctx, tmp_path):
    """ORB descriptors of six rendered frames -> training -> the bag of words of the loop closing, through a saved file too"""
    import flvis_amd
    from flvis_amd import synth
    tr = [synth.Trajectory(s) for s in range(6)]
    i0, _ = synth.Renderer("cuda").stereo_frame(tr, 0.5, 10)
    _, desc, cnt, _ = ctx.orb_detect_and_compute(i0, cap=1024)
    hd, hc = desc.cpu().numpy(), cnt.cpu().numpy()
    assert hc.min() > 200
    train = [hd[i, :hc[i]] for i in range(6)]
    voc = ctx.voc_train(desc, cnt, k=8, L=3)
    _check(voc, T.train(train, 8, 3, seed=1))
    ctx.bow_set_vocabulary(*voc.arrays)

    def transform():
        ids, vals, nnz = [t.cpu().numpy() for t in ctx.bow_transform(desc, cnt, vcap=1024)]
        return [(ids[i, :nnz[i]].copy(), vals[i, :nnz[i]].copy()) for i in range(6)]

    vecs = transform()
    for i in range(6):
        wi, wv = V.py_transform(voc.arrays, train[i])
        assert len(wi) > 20 and np.array_equal(vecs[i][0], wi) and np.array_equal(vecs[i][1], wv), i
    for i in range(6):
        scores = [V.py_score(*vecs[i], *vecs[j]) for j in range(6)]
        assert int(np.argmax(scores)) == i and abs(scores[i] - 1.0) < 1e-12, (i, scores)
    p = str(tmp_path / "trained.dbow3")
    voc.save(p)
    back = flvis_amd.read_vocabulary_file(p)
    assert back["layout"] == "binary" and (back["k"], back["L"]) == (8, 3)
    for key in ("child_ptr", "child_idx", "desc", "word_id", "weight"):
        assert np.array_equal(back[key], voc.info[key]), key
    ctx.bow_set_vocabulary(*V.build_vocabulary(train[:2], k=3, depth=2))     # something else resident first
    ctx.bow_load_vocabulary(p)
    again = transform()
    for i in range(6):
        assert np.array_equal(again[i][0], vecs[i][0]) and np.array_equal(again[i][1], vecs[i][1]), i
    voc.close()


def test_train_vocabulary_script(ctx, tmp_path):
    """The file is the restatement's tree of the same six frames' descriptors.  Six images of about a thousand features over at most
    36 words: every word may well occur in every image, Ni = NDocs, and then its weight is log(1) = 0 as setNodeWeights has it -- so
    the weights are compared with the restatement's, not asked to be positive."""
    import json
    import flvis_amd
    from flvis_amd import synth
    out = str(tmp_path / "tmp.dbow3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_vocabulary.py"), "--synth", "6", "--k", "6", "--L", "2",
                        "--out", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    v = flvis_amd.read_vocabulary_file(out)
    assert v["layout"] == "binary" and (v["k"], v["L"]) == (6, 2) and 6 < v["n_words"] <= 36
    assert (v["scoring"], v["weighting"]) == (0, 0)
    tr = [synth.Trajectory(s) for s in range(6)]
    i0, _ = synth.Renderer("cuda").stereo_frame(tr, 0.5, 10)
    _, desc, cnt, _ = ctx.orb_detect_and_compute(i0, cap=1024)
    hd, hc = desc.cpu().numpy(), cnt.cpu().numpy()
    want = T.train([hd[i, :hc[i]] for i in range(6)], 6, 2, seed=1)
    child_ptr, child_idx, wdesc, weight, word_id = want["arrays"]
    assert np.array_equal(v["child_ptr"], child_ptr) and np.array_equal(v["child_idx"], child_idx)
    assert np.array_equal(v["desc"], wdesc) and np.array_equal(v["word_id"], word_id)
    assert np.array_equal(v["weight"] != 0, weight != 0)
    assert np.all(np.abs(v["weight"] - weight) <= np.spacing(np.abs(weight)))
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert [line[k] for k in flvis_amd.TrainedVocabulary.STATS[:7]] == want["stats"]
    words = v["word_id"] >= 0
    assert line["words_without_weight"] == int(np.sum(v["weight"][words] == 0))
