"""GPU (-m gpu, MI355X): ORB extraction and Hamming matching at their tie, capacity and size edges, through the C ABI, bit for bit
against the CPU oracle (oracle/ref_orb.cpp).  The inputs and what the oracle says about them come from tests/_orb_edges.py, whose
recipes check themselves (tests/test_orb_edges_inputs.py runs them without a GPU); the contract pinned here is the comment above
flvis_hip_orb_detect_and_compute in include/flvis_hip.h.

Every output buffer is filled with a sentinel and carries guard rows behind its end: what a call must not write is checked byte for
byte, not only what it must."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _orb_edges as E

pytestmark = pytest.mark.gpu

OK, ERR_INVALID_ARG, ERR_CAPACITY = 0, -1, -4        # flvis_status of include/flvis_hip.h
SENT = 0xA5                                          # every byte of an output buffer before a call
GUARD = 64                                           # rows behind the last image's cap rows
INT_SENT = int(np.frombuffer(bytes([SENT] * 4), np.int32)[0])


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Bufs:
    """sentinel-filled outputs of one extraction call: kps [n*cap + GUARD][24 bytes], desc [n*cap + GUARD][32], cnt / ovf [n + 1]"""

    def __init__(self, n, cap):
        import torch
        self.n, self.cap = n, cap
        self.kps = torch.full(((n * cap + GUARD) * 24,), SENT, dtype=torch.uint8, device="cuda")
        self.desc = torch.full(((n * cap + GUARD) * 32,), SENT, dtype=torch.uint8, device="cuda")
        self.cnt = torch.full((n + 1,), INT_SENT, dtype=torch.int32, device="cuda")
        self.ovf = torch.full((n + 1,), INT_SENT, dtype=torch.int32, device="cuda")

    def host(self):
        import torch
        torch.cuda.synchronize()
        k = self.kps.cpu().numpy().reshape(-1, 24)
        d = self.desc.cpu().numpy().reshape(-1, 32)
        return k, d, self.cnt.cpu().numpy(), self.ovf.cpu().numpy()

    def untouched(self):
        k, d, c, o = self.host()
        return bool((k == SENT).all() and (d == SENT).all() and (c == INT_SENT).all() and (o == INT_SENT).all())


def orb_call(ctx, imgs, cap, prm, bufs=None, null_ovf=False, w=None, h=None):
    """flvis_hip_orb_detect_and_compute on a batch of host images with the oracle's parameter names -> (status, Bufs)"""
    import flvis_amd
    imgs = np.ascontiguousarray(imgs, np.uint8)
    n, ih, iw = imgs.shape
    bufs = bufs or Bufs(n, cap)
    assert bufs.n >= n and bufs.cap == cap
    d = _cuda(imgs)
    p = flvis_amd.OrbParams(int(prm["nfeatures"]), float(prm["sf"]), int(prm["nlevels"]), int(prm["fast_thr"]))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx._lib.flvis_hip_orb_detect_and_compute(ctx._h, ptr(d), int(w or iw), int(h or ih), n, C.byref(p), C.c_void_p(0), ptr(bufs.kps),
                                                   ptr(bufs.desc), ptr(bufs.cnt), int(cap), C.c_void_p(0) if null_ovf else ptr(bufs.ovf))
    ctx.synchronize()
    return rc, bufs


def check_image(bufs, i, want_k, want_d, want_ovf, what=""):
    """image i of a call: count, overflow flag, every field of every row, and rows [count, cap) never written"""
    k, d, cnt, ovf = bufs.host()
    cap = bufs.cap
    assert cnt[i] == len(want_k), (what, i, "count", int(cnt[i]), len(want_k))
    if want_ovf is not None:
        assert (ovf[i] != 0) == want_ovf and ovf[i] != INT_SENT, (what, i, "overflow flag", int(ovf[i]), want_ovf)
    c = int(cnt[i])
    g = k[i * cap:i * cap + c].copy().view(np.uint32)
    w = np.ascontiguousarray(want_k, np.float32).view(np.uint32).reshape(-1, 6)
    for col, name in enumerate(("x", "y", "size", "angle", "response", "octave")):
        bad = np.nonzero(g[:, col] != w[:, col])[0]
        assert len(bad) == 0, (what, i, name, "first differing row %d of %d" % (bad[0], c), g[bad[0]].view(np.float32), want_k[bad[0]])
    bad = np.nonzero((d[i * cap:i * cap + c] != want_d).any(1))[0]
    assert len(bad) == 0, (what, i, "descriptor", "first differing row %d of %d" % (bad[0], c))
    assert (k[i * cap + c:(i + 1) * cap] == SENT).all() and (d[i * cap + c:(i + 1) * cap] == SENT).all(), (what, i, "rows beyond the count were written")


def check_guards(bufs, n=None, what=""):
    k, d, cnt, ovf = bufs.host()
    n = bufs.n if n is None else n
    assert (k[n * bufs.cap:] == SENT).all() and (d[n * bufs.cap:] == SENT).all(), (what, "rows behind the last image were written")
    assert (cnt[n:] == INT_SENT).all() and (ovf[n:] == INT_SENT).all(), (what, "count / flag behind the last image was written")


def run_cases(ctx, names, cap, what=""):
    """one call on a batch of cases of one size and parameter set; every image against Case.expected(cap)"""
    cs = [E.case(n) for n in names]
    assert all(c.prm == cs[0].prm and c.img.shape == cs[0].img.shape for c in cs)
    rc, b = orb_call(ctx, np.stack([c.img for c in cs]), cap, cs[0].prm)
    assert rc == OK
    out = []
    for i, c in enumerate(cs):
        k, d, ovf = c.expected(cap)
        check_image(b, i, k, d, ovf, what or "+".join(names))
        out.append((len(k), ovf))
    check_guards(b, what=what)
    return out


# ---- extraction ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [("dots14", "corners", "flat"), ("dots16", "corners81", "dots14"), ("small_dots", "small")])
def test_tie_class_across_the_harris_cut_is_kept_whole(ctx, names):
    """a level holds more keypoints than its budget because they tie at the cut, and fewer than lvl_cap: nothing overflows, every
    member of the class comes back, beside ordinary images in the same call"""
    out = run_cases(ctx, names, 4096)
    assert not any(ovf for _, ovf in out)
    c = E.case(names[0])
    assert out[0][0] == c.total and c.lvl_cap >= c.counts[0] > c.budget[0]


def test_caller_capacity_alone_truncates_to_the_first_cap_rows(ctx):
    """the loop closer's own call: 1094 keypoints into cap = 1024.  The first 1024 rows of the untruncated list, the flag, and nothing
    behind row 1024; the image beside it is complete; at a capacity that holds everything the same batch is complete"""
    p10, cor = E.case("paste10"), E.case("corners")
    assert p10.total > E.CLOSER_CAP >= cor.total and p10.counts.max() <= p10.lvl_cap
    out = run_cases(ctx, ("corners", "paste10"), E.CLOSER_CAP)          # the overflowing image last: its guard rows are the buffer's end
    assert out == [(cor.total, False), (E.CLOSER_CAP, True)]
    out = run_cases(ctx, ("corners", "paste10"), 2048)
    assert out == [(cor.total, False), (p10.total, False)]
    # an ordinary image at a small capacity, one row short, and exactly full
    for cap, ovf in ((512, True), (cor.total - 1, True), (cor.total, False), (cor.total + 1, False)):
        assert run_cases(ctx, ("corners",), cap, "corners at cap %d" % cap) == [(min(cap, cor.total), ovf)]
    assert run_cases(ctx, ("paste8",), E.CLOSER_CAP) == [(E.CLOSER_CAP, True)]


def test_level_overflow_keeps_the_first_lvl_cap_of_the_level(ctx):
    """more tied keypoints in level 0 than the per-level capacity: the level's first lvl_cap in raster order at the Harris threshold
    over ALL candidates, the other levels complete and in place, the flag set"""
    names = ("dots17", "field7", "paste12")
    for n in names:
        c = E.case(n)
        assert c.counts[0] > c.lvl_cap >= c.counts[1:].max()
    out = run_cases(ctx, names, 4096)
    assert [ovf for _, ovf in out] == [True] * 3
    assert [k for k, _ in out] == [E.case(n).total - (E.case(n).counts[0] - E.case(n).lvl_cap) for n in names]
    # both truncations at once, beside an image that only meets the caller's and one that meets none
    out = run_cases(ctx, ("paste10", "corners", "paste12"), E.CLOSER_CAP)
    assert out == [(E.CLOSER_CAP, True), (E.case("corners").total, False), (E.CLOSER_CAP, True)]


def test_candidate_overflow_returns_valid_keypoints_and_stays_in_its_image(ctx):
    """more FAST survivors than the select kernel holds: the overflowed level returns keypoints that are each right (a dot inside the
    border, the oracle's response, angle and descriptor at that position), the other levels and the other image are exact"""
    f4, cor = E.case("field4"), E.case("corners")
    assert f4.survivors(0)[0] > E.CAND_CAP
    cap = 4096
    rc, b = orb_call(ctx, np.stack([f4.img, cor.img]), cap, f4.prm)
    assert rc == OK
    k, d, cnt, ovf = b.host()
    assert ovf[0] != 0 and 0 < cnt[0] <= cap
    g = k[:cnt[0]].copy().view(np.float32)
    gd = d[:cnt[0]]
    octv = g[:, 5].astype(int)
    assert np.all(np.diff(octv) >= 0)
    n0 = int((octv == 0).sum())
    assert 0 < n0 <= f4.lvl_cap
    ok, od = f4.level(0)
    at = {(int(r[0]), int(r[1])): j for j, r in enumerate(ok)}
    h, w = f4.img.shape
    xs, ys = g[:n0, 0].astype(int), g[:n0, 1].astype(int)
    assert np.array_equal(xs, g[:n0, 0]) and np.array_equal(ys, g[:n0, 1])
    assert np.all(np.diff(ys * 65536 + xs) > 0)                                                 # raster order, nothing twice
    assert np.all((xs >= E.EDGE) & (xs < w - E.EDGE) & (ys >= E.EDGE) & (ys < h - E.EDGE)) and np.all(f4.img[ys, xs] == E.DOT)
    for r in range(n0):
        x, y = int(xs[r]), int(ys[r])
        assert g[r, 4:5].view(np.uint32)[0] == np.float32(O.orb_harris(f4.pyr[0], x, y)).view(np.uint32), (r, x, y)
        assert g[r, 3:4].view(np.uint32)[0] == np.float32(O.orb_ic_angle(f4.pyr[0], x, y)).view(np.uint32), (r, x, y)
        j = at[(x, y)]
        assert np.array_equal(g[r].view(np.uint32), ok[j].view(np.uint32)) and np.array_equal(gd[r], od[j]), (r, x, y)
    # the levels above are the oracle's, whole
    rest_k = np.concatenate([f4.level(l)[0] for l in range(1, 8)])
    rest_d = np.concatenate([f4.level(l)[1] for l in range(1, 8)])
    assert f4.counts[1:].max() <= f4.lvl_cap and cnt[0] == n0 + len(rest_k)
    assert np.array_equal(g[n0:].view(np.uint32), rest_k.view(np.uint32)) and np.array_equal(gd[n0:], rest_d)
    assert (k[cnt[0]:cap] == SENT).all() and (d[cnt[0]:cap] == SENT).all()
    # the ordinary image beside it: no flag, bit-equal
    check_image(b, 1, cor.kps, cor.desc, False, "corners beside field4")
    check_guards(b)


def test_overflow_flags_are_cleared_by_the_next_call_and_optional(ctx):
    d17, cor, fl = E.case("dots17"), E.case("corners"), E.case("flat")
    cap = 2048
    b = Bufs(2, cap)
    rc, _ = orb_call(ctx, np.stack([d17.img, d17.img]), cap, d17.prm, bufs=b)
    assert rc == OK and (b.host()[3][:2] != 0).all()
    b.kps.fill_(SENT), b.desc.fill_(SENT)
    rc, _ = orb_call(ctx, np.stack([cor.img, fl.img]), cap, cor.prm, bufs=b)                    # the same flag tensor, a plain batch
    assert rc == OK and list(b.host()[3][:2]) == [0, 0]
    check_image(b, 0, cor.kps, cor.desc, False), check_image(b, 1, fl.kps, fl.desc, False), check_guards(b)
    b.ovf[:2] = 1                                                                               # ... and whatever else was in it
    rc, _ = orb_call(ctx, np.stack([cor.img, d17.img]), cap, cor.prm, bufs=b)
    assert rc == OK and b.host()[3][0] == 0 and b.host()[3][1] != 0
    # d_overflow = NULL: the same results, truncated or not, and the flag tensor is not touched
    for names, cap in ((("corners", "dots17"), 2048), (("paste10",), E.CLOSER_CAP)):
        cs = [E.case(n) for n in names]
        rc, b = orb_call(ctx, np.stack([c.img for c in cs]), cap, cs[0].prm, null_ovf=True)
        assert rc == OK
        for i, c in enumerate(cs):
            k, d, _ = c.expected(cap)
            check_image(b, i, k, d, None, "NULL flag")
        check_guards(b)
        assert (b.host()[3] == INT_SENT).all()


def test_kitti_frame_and_levels_without_a_border_box(ctx):
    """1241 x 376 (level-0 pitch = width: no multiple of the 16-byte loads or the 64 x 32 tiles) and 131 x 100 on five levels, the upper
    two of which have no border box"""
    kit, sm = E.case("kitti"), E.case("small")
    assert E.empty_box_levels(sm) == [3, 4] and sm.counts[3:].sum() == 0 and sm.counts[:3].min() > 0
    assert run_cases(ctx, ("kitti", "kitti"), 1024) == [(kit.total, False)] * 2 and kit.total > 500
    assert run_cases(ctx, ("small",), 256) == [(sm.total, False)]


@pytest.mark.parametrize("thr", [1, 254])
def test_fast_threshold_extremes(ctx, thr):
    import _synth as S
    c = E.Case("thr%d" % thr, S.corner_img(200, 260, 84), dict(E.CLOSER, fast_thr=thr)).check(cand_under=True)
    assert (c.total == 0) == (thr == 254)
    k, d, ovf = c.expected(2048)
    rc, b = orb_call(ctx, c.img[None], 2048, c.prm)
    assert rc == OK
    check_image(b, 0, k, d, ovf, "fast_threshold %d" % thr), check_guards(b)


def test_refusals_write_nothing(ctx):
    import _synth as S
    img = S.corner_img(200, 260, 84)
    cap = 4096
    b = Bufs(1, cap)

    def refused(status, imgs, prm, **kw):
        rc, _ = orb_call(ctx, imgs, cap, prm, bufs=b, **kw)
        assert rc == status, (rc, status, prm, kw)
        assert b.untouched(), (prm, kw)

    refused(ERR_INVALID_ARG, S.corner_img(100, 63, 1)[None], E.CLOSER)                          # w = 63
    refused(ERR_INVALID_ARG, S.corner_img(63, 100, 1)[None], E.CLOSER)
    refused(ERR_INVALID_ARG, S.corner_img(64, 64, 1)[None], dict(E.CLOSER, sf=1.5, nlevels=7))  # level 6: round(64 / 1.5^6) = 6 px
    assert O.orb_level_sizes(64, 64, 7, 1.5)[0][6] < 8 <= O.orb_level_sizes(64, 64, 6, 1.5)[0][5]
    refused(ERR_INVALID_ARG, img[None], dict(E.CLOSER, nlevels=13))
    refused(ERR_INVALID_ARG, img[None], dict(E.CLOSER, nlevels=0))
    refused(ERR_INVALID_ARG, img[None], dict(E.CLOSER, sf=1.0))
    refused(ERR_INVALID_ARG, img[None], dict(E.CLOSER, nfeatures=0))
    refused(ERR_INVALID_ARG, img[None], dict(E.CLOSER, fast_thr=0))
    refused(ERR_INVALID_ARG, img[None], dict(E.CLOSER, fast_thr=255))
    # twice the largest level budget must fit three quarters of the candidate buffer: 2 m <= 6144
    budget = lambda nf: int(O.orb_features_per_level(nf, 8, 1.2).max())
    nf = 3072 * 4
    while budget(nf + 1) <= 3072:
        nf += 1
    assert budget(nf) == 3072 and budget(nf + 1) == 3073
    refused(ERR_CAPACITY, img[None], dict(E.CLOSER, nfeatures=nf + 1))
    c = E.Case("largest nfeatures", img, dict(E.CLOSER, nfeatures=nf)).check(level_under=True, total_under=cap, cand_under=True)
    assert c.total > 300 and E.empty_box_levels(c) == [7]
    rc, _ = orb_call(ctx, img[None], cap, c.prm, bufs=b)
    assert rc == OK
    check_image(b, 0, c.kps, c.desc, False, "nfeatures %d" % nf), check_guards(b)


# ---- matching -----------------------------------------------------------------------------------------------------------------------
def match_batch(ctx, sets, acap, bcap, na=None, nb=None, ratio=0.8, A=None, B=None):
    """sets: [(a, b)] -> flvis_hip_orb_match and flvis_hip_hamming_knn2 on the batch (counts na / nb default to the sets' sizes)"""
    import torch
    p = len(sets)
    A = np.full((p, acap, 32), SENT, np.uint8) if A is None else A
    B = np.full((p, bcap, 32), SENT, np.uint8) if B is None else B
    for i, (a, b) in enumerate(sets):
        A[i, :len(a)], B[i, :len(b)] = a, b
    na = np.array([len(a) for a, _ in sets] if na is None else na, np.int32)
    nb = np.array([len(b) for _, b in sets] if nb is None else nb, np.int32)
    dA, dB, dna, dnb = _cuda(A), _cuda(B), _cuda(na), _cuda(nb)
    idx, dist = ctx.hamming_knn2(dA, dna, dB, dnb)              # outputs prefilled with -7
    pairs, npairs = ctx.orb_match(dA, dna, dB, dnb, ratio)       # pairs prefilled with -1
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), pairs.cpu().numpy(), npairs.cpu().numpy()


def check_match(res, i, a, b, ratio=0.8):
    """pair i of a batch against the oracle on the sets (a, b) the kernel was allowed to read"""
    idx, dist, pairs, npairs = res
    if len(a) and len(b):
        wi, wd = O.hamming_knn2(a, b)
        assert np.array_equal(idx[i, :len(a)], wi) and np.array_equal(dist[i, :len(a)], wd), i
    else:                                                       # no train descriptor: -1 / INT_MAX
        assert (idx[i, :len(a)] == -1).all() and (dist[i, :len(a)] == np.iinfo(np.int32).max).all(), i
    assert (idx[i, len(a):] == -7).all() and (dist[i, len(a):] == -7).all(), i
    want = O.orb_match(a, b, ratio) if len(a) else np.zeros((0, 2), np.int32)
    assert npairs[i] == len(want), (i, int(npairs[i]), len(want))
    assert np.array_equal(pairs[i, :len(want)], want) and (pairs[i, len(want):] == -1).all(), i
    return len(want)


def test_match_rejects_exact_duplicates(ctx):
    """b holds ten of a's descriptors twice: their two nearest neighbours are both at distance 0, and 0/0 passes no ratio test"""
    rng = np.random.default_rng(11)
    a = E.random_desc(rng, 50)
    same = np.repeat(a[3:4], 20, axis=0)                        # every train descriptor identical: d0 = d1 for every query
    sets = [(a, np.concatenate([a, a[:10]])), (a, same), (same, a), (same, same)]
    res = match_batch(ctx, sets, 64, 64)
    # (20 equal queries against a: all of them find a[3] at distance 0, a[3] finds the first of them)
    assert [check_match(res, i, x, y) for i, (x, y) in enumerate(sets)] == [40, 0, 1, 0]
    assert [tuple(p) for p in res[2][0, :40]] == [(i, i) for i in range(10, 50)]
    assert np.array_equal(res[1][0, :10], np.zeros((10, 2), np.int32)) and np.array_equal(res[0][0, :10, 0], np.arange(10))


def test_match_counts_above_the_capacity_are_clamped_and_negative_ones_are_empty(ctx):
    rng = np.random.default_rng(12)
    acap, bcap = 200, 300
    a0, b0 = E.related_sets(rng, acap, bcap, 120)
    a1, b1 = E.related_sets(rng, 90, 110, 60)
    # what lies behind pair 0's capacity is pair 1's storage: exact copies of pair 0's descriptors there would change pair 0's
    # result if the counts acap + 5 / bcap + 300 were believed
    a1[:5], b1[:100] = b0[5:10], a0[:100]
    sets = [(a0, b0), (a1, b1)]
    res = match_batch(ctx, sets, acap, bcap, na=[acap + 5, 90], nb=[bcap + 300, 110])
    assert check_match(res, 0, a0, b0) > 60 and check_match(res, 1, a1, b1) > 0
    assert len(O.orb_match(a0, np.concatenate([b0, b1[:100]]), 0.8)) != len(O.orb_match(a0, b0, 0.8))
    # negative counts: no pair, nothing written; an empty train set leaves -1 / INT_MAX
    a, b = E.related_sets(rng, 50, 50, 30)
    sets = [(a, b)] * 4
    res = match_batch(ctx, sets, 64, 64, na=[-1, 50, -2, 50], nb=[50, -3, -2, 50])
    idx, dist, pairs, npairs = res
    assert list(npairs[:3]) == [0, 0, 0] and (pairs[:3] == -1).all()
    assert (idx[0] == -7).all() and (idx[2] == -7).all() and (dist[0] == -7).all() and (dist[2] == -7).all()
    assert (idx[1, :50] == -1).all() and (dist[1, :50] == np.iinfo(np.int32).max).all() and (idx[1, 50:] == -7).all()
    assert check_match(res, 3, a, b) >= 20


@pytest.mark.parametrize("acap,bcap,sizes", [
    (257, 255, [(257, 255, 200), (256, 255, 100), (257, 1, 0), (1, 255, 1), (2, 2, 2)]),     # one descriptor past a tile of 256 / one short
    (1024, 1024, [(1000, 1024, 600), (1024, 1024, 1000), (1024, 1023, 500)]),                    # the closer's capacity, filled exactly
])
def test_match_at_capacity_shapes(ctx, acap, bcap, sizes):
    rng = np.random.default_rng(13)
    sets = [E.related_sets(rng, n1, n2, k) for n1, n2, k in sizes]
    res = match_batch(ctx, sets, acap, bcap)
    n = [check_match(res, i, a, b) for i, (a, b) in enumerate(sets)]
    assert n[0] > 0.5 * sizes[0][2]


def test_match_batch_of_64_ragged_pairs(ctx):
    rng = np.random.default_rng(14)
    sizes = [(int(rng.integers(0, 301)), int(rng.integers(0, 301))) for _ in range(64)]
    sizes[5], sizes[17], sizes[40], sizes[63] = (300, 300), (0, 0), (1, 300), (300, 257)
    sets = [E.related_sets(rng, n1, n2, min(n1, n2) // 2) for n1, n2 in sizes]
    res = match_batch(ctx, sets, 300, 300)
    n = [check_match(res, i, a, b) for i, (a, b) in enumerate(sets)]
    assert sum(n) > 1500 and n[17] == 0 and n[40] == 0


# ---- the loop closer's silent truncation ----------------------------------------------------------------------------------------------
def test_loop_closer_stores_a_keyframe_from_its_first_1024_orb_rows():
    """a keyframe with 1094 keypoints at the closer's own ORB settings (cap 1024, flag not read): the call succeeds and the database
    holds what the oracle chain -- landmarks from the depth image, bag of words -- makes of the first 1024 rows of the oracle's list"""
    import os
    import tempfile
    import torch
    import flvis_amd
    from flvis_amd import synth
    import _loop_chain as LC
    import _voc as V
    from test_oracle_bow import RefVoc
    c = E.case("paste10")
    assert c.total > E.CLOSER_CAP and c.counts.max() <= c.lvl_cap
    ctx = flvis_amd.Context(0)
    p = os.path.join(tempfile.gettempdir(), "flvis_orb_edges_depth_gpu.yaml")
    open(p, "w").write(synth.D435I_DEPTH_YAML)
    cfg = flvis_amd.load_config(p)
    assert cfg.cam_type == 2 and (cfg.image_height, cfg.image_width) == c.img.shape
    K4 = np.array([cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6]])
    voc = V.build_vocabulary([E.case(n).desc for n in ("corners", "corners81", "paste10")], k=6, depth=3)
    ctx.bow_set_vocabulary(*voc)
    # Z16 depth, 0.4 m at the left edge to 6.79 m at the right: the reference's integer metres drop the columns below 1 m
    d16 = np.ascontiguousarray(np.broadcast_to((400 + 10 * np.arange(640)).astype(np.uint16), (480, 640)))
    lc = flvis_amd.LoopCloser(ctx, cfg, LC.LC_PARAMS, n_streams=1, max_keyframes=4)
    ids = lc.add_keyframes([0], _cuda(c.img[None]), torch.from_numpy(d16.view(np.int16)[None].copy()).cuda(), [[0, 0, 0, 0, 0, 0, 1.0]])
    assert ids.tolist() == [0]
    ev = lc.process()
    assert ev[0]["kf_curr"] == 0
    kf = lc.keyframe(0, 0)
    k, d, ovf = c.expected(E.CLOSER_CAP)
    assert ovf and len(k) == E.CLOSER_CAP
    lm2, lm3, lmd = O.lc_keyframe_landmarks(None, d16, 2, k, d, K4=K4)
    assert 800 < len(lm2) < E.CLOSER_CAP
    assert np.array_equal(kf["lm2"], lm2) and np.array_equal(kf["lm3"], lm3) and np.array_equal(kf["lmd"], lmd)
    wi, wv = RefVoc(voc).transform(d)
    assert len(wi) > 20 and np.array_equal(kf["bow"][0], wi) and np.array_equal(kf["bow"][1], wv)
    # ... which is not what the whole list would have given
    full = O.lc_keyframe_landmarks(None, d16, 2, c.kps, c.desc, K4=K4)
    assert len(full[0]) > len(lm2)
    lc.close()
    ctx.close()
