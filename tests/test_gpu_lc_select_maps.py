"""GPU: the two kernel-level steps flvis_loop_closer_localize_in adds.

flvis_hip_lc_select_maps on synthetic score rows against numpy's sorted(key=(-score, index)): row lengths around the wave (64), the
workgroup's wave count times 64 (1024) and their multiples, segments that are empty, partly and wholly filled (with large scores behind the
filled part, which must never be read), n_best 1 .. 8, ties inside a wave's chunk, across chunks, across waves and across segments, the
threshold rules (score > 0 and >= min_score, NaN never), and a searched segment and all segments mixed in one call.

flvis_hip_bow_score_jobs_at: two queries against one database range give two rows, each bit for bit flvis_hip_bow_score_jobs' row for
that query alone."""
import numpy as np
import pytest

import _voc as V

pytestmark = pytest.mark.gpu
BEYOND = 1e9          # behind a segment's count: would win every rank if it were read


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def want_rows(scores, seg_n, maps, n_best, min_score):
    n_q, n_seg, seg_len = scores.shape
    idx = np.full((n_q, n_best), -1, np.int32)
    sc = np.zeros((n_q, n_best))
    cnt = np.zeros(n_q, np.int32)
    for q in range(n_q):
        segs = range(n_seg) if maps[q] < 0 else [maps[q]]
        ent = [(scores[q, s, j], s * seg_len + j) for s in segs for j in range(min(seg_n[s], seg_len))
               if scores[q, s, j] > 0 and scores[q, s, j] >= min_score]
        ent = sorted(ent, key=lambda e: (-e[0], e[1]))[:n_best]
        cnt[q] = len(ent)
        for r, (v, g) in enumerate(ent):
            idx[q, r], sc[q, r] = g, v
    return idx, sc, cnt


def check(ctx, scores, seg_n, maps, min_score, n_bests=range(1, 9)):
    import torch
    scores = np.ascontiguousarray(scores, np.float64)
    seg_n, maps = np.asarray(seg_n, np.int32), np.asarray(maps, np.int32)
    d = [torch.from_numpy(a).cuda() for a in (scores, seg_n, maps)]
    out = {}
    for n_best in n_bests:
        got = [t.cpu().numpy() for t in ctx.lc_select_maps(*d, n_best, min_score)]
        want = want_rows(scores, seg_n, maps, n_best, min_score)
        for name, g, w in zip(("idx", "score", "count"), got, want):
            assert np.array_equal(g, w), (name, n_best, scores.shape, g, w)
        out[n_best] = got
    return out


def fill_beyond(scores, seg_n):
    for s, n in enumerate(seg_n):
        scores[:, s, n:] = BEYOND
    return scores


@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_lengths_segments_and_n_best(ctx, total):
    rng = np.random.default_rng(total)
    # one segment, wholly filled; scores on a grid of 40 values: many ties at every length
    one = rng.integers(0, 40, (2, 1, total)) / 40.0
    check(ctx, one, [total], [0, -1], 0.1)
    # five segments of this length: empty, full, half, one entry, full -- every query form in one call
    seg_n = [0, total, total // 2, 1, total]
    five = fill_beyond(rng.integers(0, 40, (7, 5, total)) / 40.0, seg_n)
    check(ctx, five, seg_n, [-1, 0, 1, 2, 3, 4, -1], 0.1)


def test_bench_shape_row(ctx):
    """64 segments of 2000: an all-maps row of the loop closer at its benchmark shape, next to a one-segment query"""
    rng = np.random.default_rng(7)
    seg_n = rng.integers(0, 2001, 64)
    seg_n[[0, 5, 63]] = [2000, 0, 2000]
    scores = fill_beyond(rng.integers(0, 5000, (3, 64, 2000)) / 5000.0, seg_n)
    scores[0, 63, 1999] = scores[0, 0, 0] = 2.0          # the row's first and last entry tie for the top
    got = check(ctx, scores, seg_n, [-1, 63, -1], 0.5, n_bests=(8,))[8]
    assert got[0][0, :2].tolist() == [0, 63 * 2000 + 1999]


def test_ties(ctx):
    # all scores equal: the lowest indices, in order, across chunks, waves and segments
    check(ctx, np.full((2, 3, 700), 0.25), [700, 650, 700], [-1, 2], 0.0)
    # equal scores 64 and 256 indices apart (the next chunk of the next wave; the same lane four waves on), in either order of appearance
    for gap in (64, 256):
        row = np.linspace(0.01, 0.2, 1400).reshape(1, 1, 1400)[:, :, ::-1].copy()
        row[0, 0, 700] = row[0, 0, 700 + gap] = 0.9
        row[0, 0, 3 + gap] = row[0, 0, 3] = 0.8
        got = check(ctx, row, [1400], [0], 0.0)[4]
        assert got[0][0].tolist() == [700, 700 + gap, 3, 3 + gap]
    # equal scores in two segments: the lower segment first, whatever the position inside
    two = np.zeros((1, 4, 100))
    two[0, 3, 2] = two[0, 1, 90] = 0.7
    two[0, 2, 50] = 0.6
    got = check(ctx, two, [100] * 4, [-1], 0.0)[8]
    assert got[0][0, :3].tolist() == [190, 302, 250] and got[2][0] == 3


def test_thresholds(ctx):
    row = np.zeros((1, 2, 130))
    row[0, 0, [5, 70, 129]] = [0.5, 0.3, 0.1]
    row[0, 1, [0, 64]] = [0.3, np.nan]
    # fewer qualifying entries than n_best; a score equal to min_score is kept, the one below is not
    got = check(ctx, row, [130, 130], [-1], 0.3)[8]
    assert got[0][0].tolist() == [5, 70, 130, -1, -1, -1, -1, -1] and got[2][0] == 3
    # none at all
    got = check(ctx, row, [130, 130], [-1], 0.9)[8]
    assert got[2][0] == 0 and np.all(got[0] == -1) and np.all(got[1] == 0)
    # a score of exactly 0 is dropped even with a negative min_score; so are negatives by "> 0"; a NaN is never picked
    row[0, 1, 100] = -0.2
    got = check(ctx, row, [130, 130], [-1], -1.0)[8]
    assert got[0][0].tolist() == [5, 70, 130, 129, -1, -1, -1, -1]
    nan = np.full((2, 1, 200), np.nan)
    nan[1, 0, 199] = 1e-300
    got = check(ctx, nan, [200], [0, 0], 0.0)[8]
    assert got[2].tolist() == [0, 1] and got[0][1, 0] == 199


def test_bow_score_jobs_at_rows(ctx):
    """two queries against ONE database range: two rows, each what bow_score_jobs gives for that query alone"""
    kfs = V.make_keyframes(4, n_img=24, per_img=(250, 400))
    voc = V.build_vocabulary(kfs[:12], k=8, depth=3)
    ctx.bow_set_vocabulary(*voc)
    import torch
    cap = 512
    desc = np.zeros((len(kfs), cap, 32), np.uint8)
    for i, k in enumerate(kfs):
        desc[i, :len(k)] = k
    cnt = torch.tensor([len(k) for k in kfs], dtype=torch.int32).cuda()
    ids, vals, nnz = ctx.bow_transform(torch.from_numpy(desc).cuda(), cnt, vcap=512)
    first, n = 2, 19
    rows = {}
    for q in (22, 23):
        rows[q] = ctx.bow_score_jobs([(q, first, n)], ids, vals, nnz).cpu().numpy()[first:first + n]
    assert not np.array_equal(rows[22], rows[23]) and rows[22].max() > 0 and rows[23].max() > 0
    # rows of 25 entries: query 23 at offset 0 of row 0, query 22 at offset 3 of row 1, and a second range for query 23 behind its first
    jobs = [(23, first, n, 0), (22, first, n, 25 + 3), (23, 0, 2, n), (22, 5, 0, 49)]
    got = ctx.bow_score_jobs_at(jobs, ids, vals, nnz, 50).cpu().numpy()
    assert np.array_equal(got[0:n], rows[23]) and np.array_equal(got[28:28 + n], rows[22])
    assert np.array_equal(got[n:n + 2], ctx.bow_score_jobs([(23, 0, 2)], ids, vals, nnz).cpu().numpy()[0:2])
    assert np.all(got[n + 2:28] == -1) and np.all(got[28 + n:] == -1)
