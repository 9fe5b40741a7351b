"""GPU: flvis_loop_closer_link -- localize_in with STORED keyframes as the queries -- against flvis_loop_closer_localize_in on the images
the keyframes were stored from (bit for bit, every field), against the oracle-assembled chain with the excluded set (tests/_loop_link.py),
against itself (a query's result does not depend on the call it is in), into flvis_loop_closer_merge, and that it leaves no trace.
Scenes: tests/_loop_localize.py's tour -- 9 keyframes as sequence 0, the 4 query frames stored as sequence 1 -- and the two-camera
cross_scene() of tests/_loop_localize_in.py, rendered on the CPU once per process and uploaded."""
import ctypes as C

import numpy as np
import pytest

import _loop_chain as LC
import _loop_link as LK
import _loop_localize as LL
import _loop_localize_in as LI
import _pgo_synth as PS
import test_gpu_loop_localize as TL
from test_oracle_loop_merge import MEASURED_FIX, fix_odometry

pytestmark = pytest.mark.gpu
EXACT = TL.EXACT
ALL = LI.ALL_MAPS


class Tour:
    """a closer of two sequences: 0 holds the tour's 9 keyframes at ground truth, 1 the 4 query frames under a drifted odometry of its
    own; what localize_in says of each query frame (n_best 8, in map 0), asked right after the frame was stored; the chain's refs"""

    def __init__(self, w, n_streams=2, max_keyframes=9):
        sc = w.sc
        self.lc = lc = w.closer(n_streams, max_keyframes)
        self.refs = {s: LC.RefLoopCloser(w.K4, prm=LL.PARAMS, stream=s) for s in range(n_streams)}
        for i in range(9):
            lc.add_keyframes([0], w.kf0[i:i + 1], w.kf1[i:i + 1], [sc.kf_gt[i]])
            self.refs[0].add(w.kf_feat[i], sc.kf_gt[i])
        self.q_odom = fix_odometry(sc)
        self.in_fix = []
        for k in range(4):
            lc.add_keyframes([1], w.q0[k:k + 1], w.q1[k:k + 1], [self.q_odom[k]])
            self.refs[1].add(w.q_feat[k], self.q_odom[k])
            self.in_fix.append(lc.localize_in([1], [0], w.q0[k:k + 1], w.q1[k:k + 1], n_best=8)[0])


@pytest.fixture(scope="module")
def world():
    w = TL.World()
    w.tour = Tour(w)
    yield w
    w.tour.lc.close()
    w.ctx.close()


def _accepted(fix):
    return sum(c["accepted"] for c in fix["candidates"])


def _same_bits(a, b):
    """two fixes as the harness reports them: every field equal, poses bit for bit"""
    LI.same_fix_in(a, b, tol=EXACT)
    assert a.keys() == b.keys()
    for x, y in zip(a["candidates"], b["candidates"]):
        assert x.keys() == y.keys() and all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in x), (x, y)
    assert (a["T_c_map"] is None) == (b["T_c_map"] is None) and (a["T_c_map"] is None or np.array_equal(a["T_c_map"], b["T_c_map"]))


def _raw_link(lc, queries, n_best, link_cap=None):
    """the call through the C ABI: the structs as they come back (fixes as bytes: every field, the padding of an empty rank too)"""
    import flvis_amd
    n = len(queries)
    arr = (flvis_amd.FlvisLcLinkQuery * n)(*[flvis_amd.FlvisLcLinkQuery(*q) for q in queries])
    fix = (flvis_amd.FlvisLcFixIn * n)()
    cap = n * 8 if link_cap is None else link_cap
    links = (flvis_amd.FlvisLcLink * max(1, cap))()
    cnt = C.c_int(-1)
    lib = lc._lib
    rc = lib.flvis_loop_closer_link(lc._h, n, arr, n_best, fix, cap, links if cap else None, C.byref(cnt))
    return rc, [bytes(f) for f in fix], [bytes(l) for l in links[:max(0, min(cap, cnt.value))]], cnt.value


def _raw_localize_in(lc, stream, m, img0, img1, n_best):
    import flvis_amd
    fix = (flvis_amd.FlvisLcFixIn * 1)()
    st, mp = (C.c_int * 1)(stream), (C.c_int * 1)(m)
    lib = lc._lib
    assert lib.flvis_loop_closer_localize_in(lc._h, 1, st, mp, flvis_amd._ptr(img0), flvis_amd._ptr(img1), n_best, fix) == flvis_amd.FLVIS_OK
    return bytes(fix[0])


def test_equals_localize_in_bit_for_bit(world):
    """each keyframe of sequence 1 into map 0 with its own sequence left out = localize_in on the images it was stored from: the
    flvis_lc_fix_in structs byte for byte; FLVIS_LC_ALL_MAPS without the own sequence is the same search on this closer"""
    w, t = world, world.tour
    for n_best in (8, 3):
        for k in range(4):
            want = _raw_localize_in(t.lc, 1, 0, w.q0[k:k + 1].contiguous(), w.q1[k:k + 1].contiguous(), n_best)
            for m in (0, ALL):
                rc, fix, _, _ = _raw_link(t.lc, [(1, m, k, -1)], n_best)
                assert rc == 0 and fix[0] == want, (k, m, n_best)
    for k in range(4):
        got = t.lc.link([(1, 0, k, -1)], n_best=8)[0][0]
        _same_bits(got, t.in_fix[k])
        assert _accepted(got) >= 2 and got["best"] >= 0 and got["map"] == 0, got                    # an empty result cannot pass
    # kf = -1 names the newest keyframe
    _same_bits(t.lc.link([(1, 0, -1, -1)], n_best=8)[0][0], t.in_fix[3])


def test_equals_localize_in_on_two_cameras(world):
    """unit 2's frames stored as sequence 1 (its own K), unit 1's map as sequence 0: PnP runs with the QUERY keyframe's sequence's K"""
    import torch
    import flvis_amd
    w = world
    sc = LI.cross_scene()
    cfgs = sc.cfgs()
    up = lambda pairs, k: torch.from_numpy(np.stack([p[k] for p in pairs])).cuda()
    m0, m1, q0, q1 = up(sc.map.kf, 0), up(sc.map.kf, 1), up(sc.query.q, 0), up(sc.query.q, 1)
    fleet = flvis_amd.LoopCloser(w.ctx, cfgs, LL.PARAMS, max_keyframes=4)
    for i, T in enumerate(sc.map.kf_gt):
        fleet.add_keyframes([0], m0[i:i + 1], m1[i:i + 1], [T])
    for k, T in enumerate(sc.query.q_gt):
        fleet.add_keyframes([1], q0[k:k + 1], q1[k:k + 1], [T])
    for k in range(len(sc.query.q)):
        want = _raw_localize_in(fleet, 1, 0, q0[k:k + 1].contiguous(), q1[k:k + 1].contiguous(), 8)
        for m in (0, ALL):
            rc, fix, _, _ = _raw_link(fleet, [(1, m, k, -1)], 8)
            assert rc == 0 and fix[0] == want, (k, m)
        got = fleet.link([(1, 0, k, -1)], n_best=8)[0][0]
        assert _accepted(got) >= 2 and got["map"] == 0, got
    # from the map's side the K is unit 1's: another answer than unit 2's K would give (localize_in with the streams swapped)
    back = fleet.link([(0, 1, 1, -1)], n_best=8)[0][0]
    _same_bits(back, fleet.localize_in([0], [1], m0[1:2].contiguous(), m1[1:2].contiguous(), n_best=8)[0])
    fleet.close()


def test_equals_the_chain_with_exclusion(world):
    """keyframe 8 of sequence 0 in its own map without its neighbourhood; a sequence-1 keyframe in all maps without itself"""
    w, t = world, world.tour
    cases = [(0, 0, 8, g) for g in (0, 1, 3)] + [(0, 0, 4, 1), (1, ALL, 2, 0), (1, ALL, 0, 1), (0, ALL, 3, 2), (1, 1, 1, 0)]
    fixes, _ = t.lc.link(cases, n_best=8)
    for (s, m, kf, g), got in zip(cases, fixes):
        want, out = LK.ref_link(t.refs, m, s, kf, g, w.K4, 8)
        LI.same_fix_in(got, want)                                                                   # (T_c_map within 1e-12)
        assert not any(c["seq"] == s and c["kf"] in out for c in got["candidates"]), (s, m, kf, g, got["candidates"])
        assert kf in out and len(out) == min(len(t.refs[s].kfs) - 1, kf + g) - max(0, kf - g) + 1
        print("LOOP-LINK chain (%d, %d, %d, %d): candidates %s accepted %d" % (s, m, kf, g, [(c["seq"], c["kf"]) for c in got["candidates"]],
                                                                                 _accepted(got)))
    assert _accepted(fixes[4]) >= 2, fixes[4]                                                       # an empty result cannot pass


def test_a_result_does_not_depend_on_the_batch(world):
    """9 queries on a closer of 2 sequences (five passes): all 4 keyframes of sequence 1 and 3 of sequence 0, sequences listed several
    times, one keyframe against three maps, mixed gaps"""
    t = world.tour
    qs = [(1, 0, 0, -1), (0, 0, 8, 1), (1, ALL, 1, 0), (1, 0, 2, -1), (0, 1, 3, -1), (1, 0, 3, -1), (0, ALL, 5, 0), (1, 1, 3, 2), (1, ALL, 3, -1)]
    rc, fixes, links, n_links = _raw_link(t.lc, qs, 8)
    assert rc == 0 and n_links == len(links) > 0
    single = [_raw_link(t.lc, [q], 8) for q in qs]
    assert all(s[0] == 0 for s in single)
    assert fixes == [s[1][0] for s in single]
    assert links == [l for s in single for l in s[2]]
    order = [6, 2, 8, 0, 5, 3, 1, 7, 4]
    rc, pfix, plinks, _ = _raw_link(t.lc, [qs[i] for i in order], 8)
    assert rc == 0 and pfix == [fixes[i] for i in order] and plinks == [l for i in order for l in single[i][2]]
    for n_best in (1, 4):                                                                           # and the ranks of a shorter list
        rc, short, _, _ = _raw_link(t.lc, qs, n_best)
        assert rc == 0 and short == [_raw_link(t.lc, [q], n_best)[1][0] for q in qs]
    got, _ = t.lc.link(qs, n_best=8)
    assert all(_accepted(got[i]) >= 2 for i in (0, 3, 5, 8)), [_accepted(f) for f in got]


def test_links_feed_merge(world):
    import flvis_amd
    w, t = world, world.tour
    sc = w.sc
    want = [l for k in range(4) for l in flvis_amd.links_from_fix(t.in_fix[k], 1, k)]
    assert all(_accepted(t.in_fix[k]) >= 2 for k in range(4))
    lc = Tour(w).lc                                                                                 # (merge moves poses: a closer of its own)
    fixes, links = lc.link([(1, 0, k, -1) for k in range(4)], n_best=8)
    assert links == want and len(links) >= 8
    # from sequence 0's side: links 1 -> 0, which merge refuses under [0, 1] until they are turned round
    _, back = lc.link([(0, 1, j, -1) for j in range(9)], n_best=8)
    assert len(back) >= 2 and all(l["seq_from"] == 1 and l["seq_to"] == 0 for l in back)
    before = [lc.poses(s) for s in range(2)]
    with pytest.raises(flvis_amd.FlvisError) as e:
        lc.merge([[0, 1]], back)
    assert "loop_closer_merge failed (-1)" in str(e.value) and all(np.array_equal(lc.poses(s), before[s]) for s in range(2))
    turned = flvis_amd.links_reverse(back)
    assert [(l["seq_from"], l["kf_from"], l["seq_to"], l["kf_to"]) for l in turned] == [(l["seq_to"], l["kf_to"], l["seq_from"], l["kf_from"]) for l in back]
    twin = Tour(w).lc
    out, _ = twin.merge([[0, 1]], turned)
    assert out[0]["optimised"] and out[0]["n_edges"] > len(turned)
    errs = [LL.pose_error(twin.poses(1)[k], sc.q_gt[k]) for k in range(4)]
    print("LOOP-LINK merge from the anchor's side: %d links, at most %.4f m %.4f rad" % (len(turned), max(e[0] for e in errs), max(e[1] for e in errs)))
    twin.close()
    off = max(LL.pose_error(before[1][k], sc.q_gt[k])[0] for k in range(4))
    out, _ = lc.merge([[0, 1]], links)
    errs = [LL.pose_error(lc.poses(1)[k], sc.q_gt[k]) for k in range(4)]
    print("LOOP-LINK merge: %d links, sequence 1 off by %.2f m before, at most %.4f m %.4f rad after" %
          (len(links), off, max(e[0] for e in errs), max(e[1] for e in errs)))
    assert out[0]["optimised"]
    assert off > 5.0 and max(e[0] for e in errs) <= 2 * MEASURED_FIX[0] and max(e[1] for e in errs) <= 2 * MEASURED_FIX[1], errs
    lc.close()


def test_link_has_no_side_effects(world):
    """twin closers get the same keyframes; one is asked for links before the first keyframe's process, between add_keyframes and process
    (the pending keyframe as the query) and after it: events, similarity rows, poses, drift, keyframe contents and localize fixes stay
    identical bit for bit"""
    w = world
    sc = w.sc
    a, b = w.closer(2, 6), w.closer(2, 6)
    for i in range(5):
        streams = [0, 1] if i != 2 else [1]
        args = (streams, TL._sel(w.kf0, [i] * len(streams)), TL._sel(w.kf1, [i] * len(streams)), [sc.kf_gt[i]] * len(streams))
        assert a.add_keyframes(*args).tolist() == b.add_keyframes(*args).tolist()
        pending, _ = b.link([(1, ALL, -1, 0), (1, 0 if i else 1, -1, -1), (1, 1, 0, 0)], n_best=4)     # the new keyframe is still pending
        assert i in (0, 2) or len(pending[0]["candidates"]) >= 1                                    # (the same image in sequence 0's map)
        ea, eb = a.process(), b.process()
        assert ea == eb and [e["kf_curr"] >= 0 for e in eb] == [s in streams for s in range(2)], (i, ea, eb)
        TL._same_state(TL._state(a, 2, i == 4), TL._state(b, 2, i == 4))
        fa = a.localize([0, 1], w.q0[:2], w.q1[:2], n_best=8)
        b.link([(0, 1, 0, -1), (1, 0, -1, -1), (0, ALL, -1, 1)], n_best=8)
        fb = b.localize([0, 1], w.q0[:2], w.q1[:2], n_best=8)
        for x, y in zip(fa, fb):
            LL.same_fix(x, y, tol=EXACT)
        b.link([(1, ALL, 0, 0)] * 5, n_best=8)                                                      # (several passes)
        TL._same_state(TL._state(a, 2, i == 4), TL._state(b, 2, i == 4))
        assert b.process() == a.process()                                                           # nothing became pending
    a.close()
    b.close()


def test_current_poses(world):
    """T_c_map7 is made from the candidate's pose as the database holds it NOW: after set_drift and a merge that moved map 0"""
    w = world
    lc = Tour(w).lc
    before, _ = lc.link([(1, 0, 1, -1)], n_best=8)
    X = np.array([0.4, -0.3, 0.2, 0.0, 0.0, np.sin(0.15), np.cos(0.15)])
    lc.set_drift(1, X)
    old = lc.poses(0)
    # sequence 1 as the anchor: map 0 is the one that moves
    _, links = lc.link([(0, 1, j, -1) for j in range(9)], n_best=8)
    out, _ = lc.merge([[1, 0]], links)
    new = lc.poses(0)
    assert out[0]["optimised"] and np.abs(new[:, :3] - old[:, :3]).max() > 1.0                        # (it did move: metres)
    after, _ = lc.link([(1, 0, 1, -1)], n_best=8)
    f, g = after[0], before[0]
    assert f["best"] == g["best"] >= 0 and [c["kf"] for c in f["candidates"]] == [c["kf"] for c in g["candidates"]]
    c = f["candidates"][f["best"]]
    assert np.array_equal(c["pose"], g["candidates"][g["best"]]["pose"])                            # the pair check saw no pose
    assert np.abs(np.asarray(f["T_c_map"]) - PS.mul7(c["pose"], new[c["kf"]])).max() < 1e-12
    assert np.abs(np.asarray(f["T_c_map"]) - np.asarray(g["T_c_map"]))[:3].max() > 1.0
    lc.close()


def test_arguments_and_empties(world):
    import flvis_amd
    w, t = world, world.tour
    lc = w.closer(3, 9)
    for i in range(4):
        lc.add_keyframes([0, 1] if i < 2 else [0], TL._sel(w.kf0, [i] * (2 if i < 2 else 1)), TL._sel(w.kf1, [i] * (2 if i < 2 else 1)),
                         [w.sc.kf_gt[i]] * (2 if i < 2 else 1))                                     # 0: 4 keyframes, 1: 2, 2: none
    state = lambda: TL._state(lc, 3)
    start = state()
    INVALID = flvis_amd.FLVIS_ERR_INVALID_ARG
    good = (0, 1, 1, -1)
    bad = {
        "n_best 0": ([good], 0), "n_best 9": ([good], 9), "no queries": ([], 4),
        "stream out of range": ([good, (3, 0, 0, -1)], 4), "stream negative": ([(-1, 0, 0, -1)], 4),
        "map out of range": ([(0, 3, 0, -1)], 4), "map below ALL_MAPS": ([(0, -2, 0, -1)], 4),
        "kf beyond the count": ([good, (1, 0, 2, -1)], 4), "kf below -1": ([(0, 1, -2, -1)], 4),
        "newest of an empty sequence": ([(2, 0, -1, -1)], 4), "kf 0 of an empty sequence": ([(2, 0, 0, -1)], 4),
        "own_gap below -1": ([(0, 0, 1, -2)], 4),
    }
    for what, (qs, n_best) in bad.items():
        with pytest.raises(flvis_amd.FlvisError) as e:
            lc.link(qs, n_best=n_best)
        assert "loop_closer_link failed (-1)" in str(e.value), (what, str(e.value))
        TL._same_state(state(), start)
    # through the C ABI: link_cap, NULL arguments
    n = len(lc.link([good], n_best=8)[1])
    assert n >= 1
    assert _raw_link(lc, [good], 8, link_cap=-1)[0] == INVALID
    lib = lc._lib
    q = (flvis_amd.FlvisLcLinkQuery * 1)(flvis_amd.FlvisLcLinkQuery(*good))
    fix, links, cnt = (flvis_amd.FlvisLcFixIn * 1)(), (flvis_amd.FlvisLcLink * 8)(), C.c_int(-5)
    assert lib.flvis_loop_closer_link(lc._h, 1, q, 8, fix, 8, None, C.byref(cnt)) == INVALID           # link_cap > 0 and no h_links
    assert lib.flvis_loop_closer_link(lc._h, 1, None, 8, fix, 8, links, C.byref(cnt)) == INVALID
    assert lib.flvis_loop_closer_link(lc._h, 1, q, 8, None, 8, links, C.byref(cnt)) == INVALID
    assert lib.flvis_loop_closer_link(lc._h, 1, q, 8, fix, 8, links, None) == INVALID
    assert lib.flvis_loop_closer_link(None, 1, q, 8, fix, 8, links, C.byref(cnt)) == INVALID
    assert lib.flvis_loop_closer_link(lc._h, 0, q, 8, fix, 8, links, C.byref(cnt)) == INVALID
    assert lib.flvis_loop_closer_link(lc._h, -1, q, 8, fix, 8, links, C.byref(cnt)) == INVALID
    assert cnt.value == -5
    TL._same_state(state(), start)
    # link_cap smaller than the count: link_cap entries, the full count; link_cap 0 with NULL h_links: the count alone
    rc, fx, full, cnt_full = _raw_link(lc, [good], 8)
    assert rc == 0 and cnt_full == n == len(full)
    for cap in (0, 1, n - 1 if n > 1 else 0):
        rc, fx2, part, c2 = _raw_link(lc, [good], 8, link_cap=cap)
        assert rc == 0 and c2 == n and part == full[:cap] and fx2 == fx
    # empties: an empty searched map; map == stream with the whole own sequence left out; all maps when only the own one holds keyframes
    solo = w.closer(2, 4)
    solo.add_keyframes([0], w.kf0[:1], w.kf1[:1], [w.sc.kf_gt[0]])
    for qq, owner in (((0, 2, 1, -1), lc), ((0, 0, 1, -1), lc), ((1, 1, -1, -1), lc), ((0, ALL, 0, -1), solo), ((0, ALL, 0, 0), solo), ((0, 1, 0, 5), solo)):
        fixes, links = owner.link([qq], n_best=8)
        f = fixes[0]
        assert f["candidates"] == [] and f["best"] == -1 and f["map"] == -1 and f["T_c_map"] is None and links == [], (qq, f)
        assert f["n_landmarks"] > 100
    # kf = -1: the newest; a gap wider than the sequence is all of it
    newest, _ = lc.link([(0, 1, -1, -1), (0, 1, 3, -1), (0, 0, 2, 100), (0, 0, 2, 2 ** 40)], n_best=8)
    _same_bits(newest[0], newest[1])
    assert newest[2]["candidates"] == [] and newest[3]["candidates"] == []
    TL._same_state(state(), start)
    solo.close()
    lc.close()
