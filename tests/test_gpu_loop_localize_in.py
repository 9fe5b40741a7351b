"""GPU: flvis_loop_closer_localize_in / _localize_in_host against flvis_loop_closer_localize, against closers that hold one map, and
against the oracle-assembled chain (tests/_loop_localize_in.py) on the device's features: the searched map named per query, several
queries in one map, a query camera that is not the map's (PnP with the query's K), the ranking across all maps, and that the call leaves
no trace in any sequence.  Scenes: tests/_loop_localize.py's tour (shared with test_gpu_loop_localize.py) and the two-camera scene of
tests/test_oracle_loop_localize_in.py, rendered on the CPU and uploaded.

The PnP seed of a set names the query's sequence and the candidate's rank in THIS call's list, as in localize.  Where a result is
compared with another closer's bit for bit, the twin therefore keeps the query's sequence index; and a candidate of an all-maps call is
compared with a one-map call's inliers and pose where it has the same rank in both (matches, score and identity: always) -- every
candidate of the all-maps call is compared with the chain run at its own rank."""
import ctypes

import numpy as np
import pytest

import _loop_chain as LC
import _loop_localize as LL
import _loop_localize_in as LI
import test_gpu_loop_localize as TL

pytestmark = pytest.mark.gpu
EXACT = TL.EXACT
ALL = LI.ALL_MAPS
_sel = TL._sel


@pytest.fixture(scope="module")
def world():
    w = TL.World()
    yield w
    w.ctx.close()


def _fill(w, lc, refs, plan, odom=None):
    """plan: {sequence: keyframe images of the tour it stores, in order}; the closer and the chain's refs get the same keyframes"""
    sc = w.sc
    for step in range(max(len(v) for v in plan.values())):
        streams = [s for s in sorted(plan) if step < len(plan[s])]
        kfs = [plan[s][step] for s in streams]
        T = [(odom[s] if odom and s in odom else sc.kf_gt)[k] for s, k in zip(streams, kfs)]
        lc.add_keyframes(streams, _sel(w.kf0, kfs), _sel(w.kf1, kfs), T)
        for s, k, t in zip(streams, kfs, T):
            if refs is not None:
                refs[s].add(w.kf_feat[k], t)


def _refs(w, n):
    return {s: LC.RefLoopCloser(w.K4, prm=LL.PARAMS, stream=s) for s in range(n)}


def _same_candidate(a, b, pnp=True):
    keys = ("seq", "kf", "score", "n_matches") + (("n_inliers", "accepted") if pnp else ())
    assert all(a[k] == b[k] for k in keys), (a, b)
    if pnp:
        assert np.array_equal(a["pose"], b["pose"]), (a, b)


def test_own_map_equals_localize(world):
    """three sequences holding 9 (exactly full), 5 and 0 keyframes: maps = streams gives localize's result bit for bit"""
    w = world
    lc = w.closer(3, 9)
    _fill(w, lc, None, {0: list(range(9)), 1: list(range(5))}, odom={1: LC.drifted_odometry(w.sc.kf_gt, 3, sigma_t=0.008, sigma_r=0.002)})
    lc.process()
    order = [2, 0, 1]
    for n_best in (1, 4, 8):
        want = lc.localize(order, w.q0[:3], w.q1[:3], n_best=n_best)
        got = lc.localize_in(order, order, w.q0[:3], w.q1[:3], n_best=n_best)
        for k, s in enumerate(order):
            LI.same_fix_in(got[k], LI.as_fix_in(want[k], s), tol=EXACT)
            assert all(c["seq"] == s for c in got[k]["candidates"])
        assert got[0]["candidates"] == [] and got[0]["map"] == -1 and got[0]["n_landmarks"] > 100           # the empty sequence: no error
        assert got[1]["best"] >= 0 and got[1]["map"] == 0 and len(got[1]["candidates"]) == n_best
    sub = lc.localize_in([1], [1], w.q0[3:4], w.q1[3:4], n_best=8)                                          # a subset, another query
    LI.same_fix_in(sub[0], LI.as_fix_in(lc.localize([1], w.q0[3:4], w.q1[3:4], n_best=8)[0], 1), tol=EXACT)
    lc.close()


def test_one_map_several_queries(world):
    """queries of sequences 0 and 2 both look into sequence 1's map: two score rows over one database range"""
    w = world
    lc = w.closer(3, 6)
    refs = _refs(w, 3)
    _fill(w, lc, refs, {1: [0, 1, 2, 3, 4], 2: [6, 7]})                    # (sequence 2's own map is another place: it must not show up)
    got = lc.localize_in([0, 2], [1, 1], w.q0[1:3], w.q1[1:3], n_best=8)
    assert got[0]["best"] >= 0 and got[1]["best"] >= 0 and got[0]["candidates"][0]["kf"] != got[1]["candidates"][0]["kf"], got
    for k, s in enumerate((0, 2)):
        assert got[k]["map"] == 1 and all(c["seq"] == 1 for c in got[k]["candidates"])
        LI.same_fix_in(got[k], LI.ref_localize_in(refs, 1, w.q_feat[1 + k], s, w.K4, 8))
        # a closer in which the query's own sequence holds that map, and nothing else: localize there (a one-sequence closer for query 0)
        twin = w.closer(s + 1, 6)
        _fill(w, twin, None, {s: [0, 1, 2, 3, 4]})
        one = twin.localize([s], w.q0[1 + k:2 + k], w.q1[1 + k:2 + k], n_best=8)[0]
        LI.same_fix_in(got[k], dict(LI.as_fix_in(one, 1)), tol=EXACT)
        twin.close()
    # ... and each alone gives what it gives next to the other
    for k, s in enumerate((0, 2)):
        LI.same_fix_in(lc.localize_in([s], [1], w.q0[1 + k:2 + k], w.q1[1 + k:2 + k], n_best=8)[0], got[k], tol=EXACT)
    lc.close()


def test_another_camera(world):
    """unit 1's map, unit 2's frames: the chain with the map's landmarks (unit 1's P0 / P1), the query's (unit 2's) and the QUERY's K"""
    import torch
    import flvis_amd
    w = world
    sc = LI.cross_scene()
    cfgs = sc.cfgs()
    cam_m, cam_q = LL.cam_of(cfgs[0]), LL.cam_of(cfgs[1])
    up = lambda pairs, k: torch.from_numpy(np.stack([p[k] for p in pairs])).cuda()
    m0, m1, q0, q1 = up(sc.map.kf, 0), up(sc.map.kf, 1), up(sc.query.q, 0), up(sc.query.q, 1)
    fleet = flvis_amd.LoopCloser(w.ctx, cfgs, LL.PARAMS, max_keyframes=4)
    ref = LC.RefLoopCloser(cam_m[2], prm=LL.PARAMS, stream=0)
    for i, (f, T) in enumerate(zip(w.features(m0, m1, cam_m[0], cam_m[1]), sc.map.kf_gt)):
        fleet.add_keyframes([0], m0[i:i + 1], m1[i:i + 1], [T])
        ref.add(f, T)
    q_feat = w.features(q0, q1, cam_q[0], cam_q[1])
    for k in range(len(sc.query.q)):
        got = fleet.localize_in([1], [0], q0[k:k + 1], q1[k:k + 1], n_best=8)[0]
        want = LI.ref_localize_in({0: ref}, 0, q_feat[k], 1, cam_q[2], 8)
        LI.same_fix_in(got, want)
        assert got["best"] >= 0 and got["map"] == 0 and sum(c["accepted"] for c in got["candidates"]) >= 2, got    # the precondition
        et, ea = LL.pose_error(got["T_c_map"], sc.query.q_gt[k])
        print("query %d: inliers %s, pose error %.6f m %.6f rad" % (k, [c["n_inliers"] for c in got["candidates"]], et, ea))
        # the map's K in the query's place gives another answer: this scene tells the two apart
        other = LI.ref_localize_in({0: ref}, 0, q_feat[k], 1, cam_m[2], 8)
        assert [c["kf"] for c in other["candidates"]] == [c["kf"] for c in want["candidates"]]
        assert any(a["n_matches"] >= 5 and not np.array_equal(a["pose"], b["pose"]) for a, b in zip(want["candidates"], other["candidates"]))
        assert other["best"] < 0 or not np.array_equal(other["T_c_map"], want["T_c_map"])
    fleet.close()


def test_all_maps(world):
    w = world
    lc = w.closer(4, 9)
    refs = _refs(w, 4)
    # sequence 0: the whole tour; 1: its first five keyframes again (equal scores in two maps); 2: empty; 3: the tour's end
    _fill(w, lc, refs, {0: list(range(9)), 1: list(range(5)), 3: [6, 7, 8]}, odom={1: LC.drifted_odometry(w.sc.kf_gt, 3, sigma_t=0.008, sigma_r=0.002)})
    order = [2, 0, 3]
    per = [lc.localize_in(order, [m] * 3, w.q0[:3], w.q1[:3], n_best=8) for m in range(4)]
    assert all(f["candidates"] == [] for f in per[2])
    for n_best in (8, 3):
        got = lc.localize_in(order, [ALL] * 3, w.q0[:3], w.q1[:3], n_best=n_best)
        for k, s in enumerate(order):
            merged = sorted((c for m in range(4) for c in per[m][k]["candidates"]), key=lambda c: (-c["score"], c["seq"], c["kf"]))[:n_best]
            assert len(got[k]["candidates"]) == len(merged) == n_best
            for r, (a, b) in enumerate(zip(got[k]["candidates"], merged)):
                rank_there = [(c["seq"], c["kf"]) for c in per[b["seq"]][k]["candidates"]].index((b["seq"], b["kf"]))
                _same_candidate(a, b, pnp=rank_there == r)
            LI.same_fix_in(got[k], LI.ref_localize_in(refs, ALL, w.q_feat[k], s, w.K4, n_best))
            assert got[k]["best"] >= 0 and got[k]["map"] == got[k]["candidates"][got[k]["best"]]["seq"]
        # the same keyframe image in sequences 0 and 1: equal scores, the lower sequence first
        c = got[0]["candidates"]
        pairs = [(r, r2) for r in range(len(c)) for r2 in range(len(c)) if c[r]["seq"] == 0 and c[r2]["seq"] == 1 and c[r]["kf"] == c[r2]["kf"]]
        assert pairs and all(c[r]["score"] == c[r2]["score"] and r2 == r + 1 for r, r2 in pairs), c
    # one map and all maps mixed in one call
    mixed = lc.localize_in(order, [3, ALL, 1], w.q0[:3], w.q1[:3], n_best=8)
    LI.same_fix_in(mixed[0], per[3][0], tol=EXACT)
    LI.same_fix_in(mixed[1], lc.localize_in(order, [ALL] * 3, w.q0[:3], w.q1[:3], n_best=8)[1], tol=EXACT)
    LI.same_fix_in(mixed[2], per[1][2], tol=EXACT)
    lc.close()
    empty = w.closer(2, 4)
    for f in empty.localize_in([0, 1], [ALL, ALL], w.q0[:2], w.q1[:2], n_best=8):
        assert f["candidates"] == [] and f["best"] == -1 and f["map"] == -1 and f["T_c_map"] is None and f["n_landmarks"] > 100
    empty.close()


def test_localize_in_has_no_side_effects(world):
    """twin closers get the same keyframes; one is asked to localize_in (one map, all maps) before the first keyframe, between
    add_keyframes and process, and after process: events, similarity rows, poses, drift and keyframe contents stay identical"""
    w = world
    sc = w.sc
    a, b = w.closer(2, 6), w.closer(2, 6)
    first = b.localize_in([1, 0], [0, ALL], w.q0[:2], w.q1[:2], n_best=8)
    assert all(f["candidates"] == [] and f["best"] == -1 for f in first)
    for i in range(5):
        streams = [0, 1] if i != 2 else [1]
        args = (streams, _sel(w.kf0, [i] * len(streams)), _sel(w.kf1, [i] * len(streams)), [sc.kf_gt[i]] * len(streams))
        assert a.add_keyframes(*args).tolist() == b.add_keyframes(*args).tolist()
        b.localize_in([0, 1], [1, ALL] if i % 2 else [ALL, 0], w.q0[:2], w.q1[:2], n_best=4)               # the new keyframe is still pending
        ea, eb = a.process(), b.process()
        assert ea == eb and [e["kf_curr"] >= 0 for e in eb] == [s in streams for s in range(2)], (i, ea, eb)
        TL._same_state(TL._state(a, 2, i == 4), TL._state(b, 2, i == 4))
        fix = b.localize_in([0, 1], [1, ALL], w.q0[1:3], w.q1[1:3], n_best=8)
        assert len(fix[0]["candidates"]) >= 1 and len(fix[1]["candidates"]) >= 2
        TL._same_state(TL._state(a, 2, i == 4), TL._state(b, 2, i == 4))
        assert b.process() == a.process()                                                                   # nothing became pending
    # ... nor in what localize itself returns afterwards
    for x, y in zip(a.localize([0, 1], w.q0[:2], w.q1[:2], n_best=8), b.localize([0, 1], w.q0[:2], w.q1[:2], n_best=8)):
        LL.same_fix(x, y, tol=EXACT)
    a.close()
    b.close()


def test_host_images_argument_errors_and_reset(world):
    import flvis_amd
    w = world
    sc = w.sc
    lc = w.closer(3, 6)
    _fill(w, lc, None, {0: [0, 1, 2], 1: [2, 3, 4], 2: [5]})
    streams, maps = [1, 0], [0, ALL]
    want = lc.localize_in(streams, maps, w.q0[:2], w.q1[:2], n_best=8)
    assert want[0]["best"] >= 0 and want[1]["best"] >= 0
    # localize_in_host on padded-pitch host images = localize_in
    pad = [[np.zeros((480, 704), np.uint8) for _ in range(2)] for _ in range(2)]
    for k in range(2):
        pad[k][0][:, :640], pad[k][1][:, :640] = sc.q[k][0], sc.q[k][1]
    h0, h1 = [pad[0][0][:, :640], pad[1][0][:, :640]], [pad[0][1][:, :640], pad[1][1][:, :640]]
    host = lambda: lc.localize_in_host(streams, maps, h0, h1, n_best=8)
    for x, y in zip(host(), want):
        LI.same_fix_in(x, y, tol=EXACT)
    # argument errors: FLVIS_ERR_INVALID_ARG, and the next valid call is unchanged
    bad = ((dict(n_best=0), streams, maps), (dict(n_best=9), streams, maps), (dict(n_best=8), [1, 1], maps), (dict(n_best=8), [3, 0], maps),
           (dict(n_best=8), [-1, 0], maps), (dict(n_best=8), streams, [3, 0]), (dict(n_best=8), streams, [0, -2]))
    for kwargs, st, mp in bad:
        with pytest.raises(flvis_amd.FlvisError) as e:
            lc.localize_in(st, mp, w.q0[:2], w.q1[:2], **kwargs)
        assert "loop_closer_localize_in failed (-1)" in str(e.value), (kwargs, st, mp)                     # FLVIS_ERR_INVALID_ARG
        with pytest.raises(flvis_amd.FlvisError) as e:
            lc.localize_in_host(st, mp, h0, h1, **kwargs)
        assert "loop_closer_localize_in_host failed (-1)" in str(e.value), (kwargs, st, mp)
    with pytest.raises(flvis_amd.FlvisError) as e:                                  # a wrong image shape (width 704: the padded array itself)
        lc.localize_in_host(streams, maps, [pad[0][0], pad[1][0]], [pad[0][1], pad[1][1]], n_best=8)
    assert "failed (-1)" in str(e.value)
    fix = (flvis_amd.FlvisLcFixIn * 2)()
    img = (flvis_amd.FlvisImage * 2)()
    st, mp = (ctypes.c_int * 2)(1, 0), (ctypes.c_int * 2)(0, -1)
    lib, P = w.ctx._lib, flvis_amd._ptr
    INVALID = flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_localize_in(lc._h, 0, st, mp, P(w.q0), P(w.q1), 4, fix) == INVALID      # n <= 0
    assert lib.flvis_loop_closer_localize_in(lc._h, -1, st, mp, P(w.q0), P(w.q1), 4, fix) == INVALID
    assert lib.flvis_loop_closer_localize_in(lc._h, 2, st, None, P(w.q0), P(w.q1), 4, fix) == INVALID    # NULL h_map
    assert lib.flvis_loop_closer_localize_in(lc._h, 2, st, mp, P(w.q0), P(w.q1), 4, None) == INVALID     # NULL h_fix
    assert lib.flvis_loop_closer_localize_in_host(lc._h, 2, st, None, img, img, 4, fix) == INVALID
    assert lib.flvis_loop_closer_localize_in_host(lc._h, 2, st, mp, img, img, 4, None) == INVALID
    assert lib.flvis_loop_closer_localize_in_host(lc._h, 0, st, mp, img, img, 4, fix) == INVALID
    for x, y in zip(host(), want):
        LI.same_fix_in(x, y, tol=EXACT)
    for x, y in zip(lc.localize_in(streams, maps, w.q0[:2], w.q1[:2], n_best=8), want):
        LI.same_fix_in(x, y, tol=EXACT)
    # after a reset of map 0: it gives no candidates, the other maps' results are unchanged
    per = [lc.localize_in([2], [m], w.q0[1:2], w.q1[1:2], n_best=8)[0] for m in range(3)]
    assert len(per[0]["candidates"]) >= 2 and len(per[1]["candidates"]) >= 2
    lc.reset([0])
    after = [lc.localize_in([2], [m], w.q0[1:2], w.q1[1:2], n_best=8)[0] for m in range(3)]
    assert after[0]["candidates"] == [] and after[0]["best"] == -1 and after[0]["map"] == -1
    assert after[0]["n_landmarks"] == per[0]["n_landmarks"]
    for m in (1, 2):
        LI.same_fix_in(after[m], per[m], tol=EXACT)
    everywhere = lc.localize_in([2], [ALL], w.q0[1:2], w.q1[1:2], n_best=8)[0]
    assert everywhere["candidates"] and all(c["seq"] != 0 for c in everywhere["candidates"])
    lc.close()
