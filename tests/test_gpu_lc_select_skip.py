"""GPU: flvis_hip_lc_select_maps_skip, the candidate choice of flvis_loop_closer_link -- flvis_hip_lc_select_maps with a range of global
indices per query that is never a candidate and never read -- on synthetic score rows against numpy's sorted(key=(-score, index)) with the
range removed (the scheme of tests/test_gpu_lc_select_maps.py): segments of 1, 63, 64, 65 and 130 entries (below, at and above a wave's
chunk of 64; three chunks), 1 and 3 segments, range edges on and beside chunk and segment edges, a whole segment, a range across two
segments, empty and inverted ranges, a range over everything, ties across the range's edge, NaN / 1e300 inside the range, n_best 1 and 8,
the closer's compact rows, and with empty ranges the bits of flvis_hip_lc_select_maps."""
import numpy as np
import pytest

from test_gpu_lc_select_maps import BEYOND, fill_beyond, want_rows

pytestmark = pytest.mark.gpu
SEG_LENS = (1, 63, 64, 65, 130)
N_BESTS = (1, 8)


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def want_skip(scores, seg_n, maps, skip, n_best, min_score):
    """want_rows on rows whose excluded entries cannot qualify (score 0), whatever they held"""
    n_q, n_seg, seg_len = scores.shape
    clean = scores.reshape(n_q, -1).copy()
    for q, (lo, hi) in enumerate(skip):
        clean[q, max(0, lo):max(0, hi)] = 0.0
    return want_rows(clean.reshape(scores.shape), seg_n, maps, n_best, min_score)


def check(ctx, scores, seg_n, maps, skip, min_score, compact=False):
    import torch
    scores = np.ascontiguousarray(scores, np.float64)
    seg_n, maps, skip = np.asarray(seg_n, np.int32), np.asarray(maps, np.int32), np.asarray(skip, np.int32).reshape(-1, 2)
    rows = scores if not compact else np.ascontiguousarray(np.stack([scores[q, m] for q, m in enumerate(maps)]))
    d = [torch.from_numpy(a).cuda() for a in (rows, seg_n, maps, skip)]
    out = {}
    for n_best in N_BESTS:
        got = [t.cpu().numpy() for t in ctx.lc_select_maps_skip(*d, n_best, min_score)]
        want = want_skip(scores, seg_n, maps, skip, n_best, min_score)
        for name, g, w in zip(("idx", "score", "count"), got, want):
            assert np.array_equal(g, w), (name, n_best, scores.shape, compact, skip.tolist(), g, w)
        for q, (lo, hi) in enumerate(skip):
            assert not np.any((got[0][q] >= max(0, lo)) & (got[0][q] < hi)), (q, lo, hi, got[0][q])
        out[n_best] = got
    return out


def edges(seg_len):
    return sorted({0, 1, 63, 64, 65, seg_len, seg_len + 1})


@pytest.mark.parametrize("seg_len", SEG_LENS)
def test_range_edges_one_segment(ctx, seg_len):
    """every (lo, hi) of the edge set as one query each, in one call: lo >= hi among them (nothing excluded), hi beyond the row, the
    whole segment; scores on a grid of 12 values, so ties lie on both sides of every edge"""
    rng = np.random.default_rng(seg_len)
    skip = [(lo, hi) for lo in edges(seg_len) for hi in edges(seg_len)]
    one = np.repeat(rng.integers(0, 12, (1, 1, seg_len)) / 12.0, len(skip), 0)
    check(ctx, one, [seg_len], [0] * len(skip), skip, 0.1)
    check(ctx, one, [seg_len], [-1] * len(skip), skip, 0.1)
    check(ctx, one, [seg_len], [0] * len(skip), skip, 0.1, compact=True)


@pytest.mark.parametrize("seg_len", SEG_LENS)
def test_range_edges_three_segments(ctx, seg_len):
    """three segments (full, partly filled with large scores behind the count, full): ranges in the middle segment at the edge set, the
    whole middle segment, ranges from inside one segment into the next, over everything; all maps, the segment of the range, another
    segment, and the compact rows"""
    rng = np.random.default_rng(100 + seg_len)
    seg_n = [seg_len, max(1, seg_len - 2), seg_len]
    L = seg_len
    skip = [(L + lo, L + hi) for lo in edges(L) for hi in edges(L) if lo <= L and hi <= L + 1]
    skip += [(L, 2 * L), (0, L), (2 * L, 3 * L), (L // 2, L + (L + 1) // 2), (L + L // 2, 3 * L), (L - 1, L + 1), (2 * L - 1, 2 * L + 1),
             (0, 3 * L), (-5, 3 * L + 70), (5, 5), (2 * L, L)]
    three = fill_beyond(np.repeat(rng.integers(0, 12, (1, 3, L)) / 12.0, len(skip), 0), seg_n)
    for maps in ([-1] * len(skip), [1] * len(skip), [2] * len(skip)):
        check(ctx, three, seg_n, maps, skip, 0.1)
    got = check(ctx, three, seg_n, [-1] * len(skip), skip, 0.0)
    for q in (skip.index((0, 3 * L)), skip.index((-5, 3 * L + 70))):          # over every candidate: count 0, all ranks -1, scores 0
        assert got[8][2][q] == 0 and np.all(got[8][0][q] == -1) and np.all(got[8][1][q] == 0.0)
    for m in (0, 1, 2):
        check(ctx, three, seg_n, [m] * len(skip), skip, 0.1, compact=True)
    mixed = [(-1, 1, 2, 0)[q % 4] for q in range(len(skip))]                   # every query form in one call
    check(ctx, three, seg_n, mixed, skip, 0.1)


def test_ties_across_the_edge(ctx):
    """equal scores, one inside the range and one outside: the one outside is picked, at the rank the tie rule gives it"""
    row = np.full((4, 3, 130), 0.01)
    row[:, 0, 63] = row[:, 0, 64] = 0.9            # either side of a chunk edge
    row[:, 1, 129] = row[:, 2, 0] = 0.8            # either side of a segment edge (global 259 | 260)
    skip = [(64, 65), (63, 64), (260, 390), (0, 260)]
    got = check(ctx, row, [130] * 3, [-1] * 4, skip, 0.0)[8]
    assert got[0][0, :3].tolist() == [63, 259, 260] and got[0][1, :3].tolist() == [64, 259, 260]
    assert got[0][2, :3].tolist() == [63, 64, 259] and got[0][3, :2].tolist() == [260, 261]
    # all scores equal: the lowest indices outside the range, in order, across chunks and segments
    check(ctx, np.full((3, 3, 130), 0.25), [130, 100, 130], [-1, 1, -1], [(0, 7), (130, 195), (60, 262)], 0.0)


@pytest.mark.parametrize("poison", [np.nan, 1e300, BEYOND, -np.inf])
def test_poison_inside_the_range_is_never_picked(ctx, poison):
    """what lies in the range would win every rank (or, a NaN, poison a comparison) if it were looked at"""
    rng = np.random.default_rng(5)
    base = rng.integers(1, 12, (1, 3, 130)) / 12.0
    skip = [(130, 260), (60, 70), (0, 64), (129, 131), (200, 390), (0, 390), (64, 128), (259, 260)]
    rows = np.repeat(base, len(skip), 0).reshape(len(skip), -1)
    for q, (lo, hi) in enumerate(skip):
        rows[q, lo:hi] = poison
    rows = rows.reshape(len(skip), 3, 130)
    for maps in ([-1] * len(skip), [0] * len(skip), [1] * len(skip)):
        got = check(ctx, rows, [130] * 3, maps, skip, 0.0)[8]
        assert np.all(np.isfinite(got[1])) and got[1].max() < 1.0
    check(ctx, rows, [130] * 3, [1] * len(skip), skip, 0.0, compact=True)


def test_empty_ranges_give_the_bits_of_select_maps(ctx):
    import torch
    rng = np.random.default_rng(9)
    for seg_len in SEG_LENS + (1025,):
        seg_n = [seg_len, seg_len // 2, 0, seg_len]
        scores = fill_beyond(rng.integers(0, 40, (6, 4, seg_len)) / 40.0, seg_n)
        scores[0, 3, seg_len - 1] = np.nan
        maps = np.array([-1, 0, 1, 2, 3, -1], np.int32)
        skip = np.array([(0, 0), (5, 5), (seg_len, 1), (4 * seg_len, 4 * seg_len), (2 ** 30, -2 ** 30), (-3, -1)], np.int32)
        d = [torch.from_numpy(a).cuda() for a in (scores, np.asarray(seg_n, np.int32), maps)]
        for n_best in N_BESTS:
            want = ctx.lc_select_maps(*d, n_best, 0.1)
            got = ctx.lc_select_maps_skip(*d, torch.from_numpy(skip).cuda(), n_best, 0.1)
            for g, w in zip(got, want):
                assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (seg_len, n_best)
        # the compact rows without a range table: the segment's own answer
        m = np.array([0, 1, 3], np.int32)
        rows = np.ascontiguousarray(scores[[0, 1, 2]][np.arange(3), m])
        got = ctx.lc_select_maps_skip(torch.from_numpy(rows).cuda(), d[1], torch.from_numpy(m).cuda(), None, 8, 0.1)
        want = ctx.lc_select_maps(torch.from_numpy(np.ascontiguousarray(scores[:3])).cuda(), d[1], torch.from_numpy(m).cuda(), 8, 0.1)
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), seg_len
