"""GPU: the loop closer fed from the keyframe log (flvis_loop_closer_add_logged, include/flvis_hip.h) against the parent's only way:
one image_feed per frame, the message's HOST images through flvis_loop_closer_add_keyframes_host and flvis_loop_closer_process after
every frame's keyframes.  Everything bit for bit: the log and the gather are copies, and the closer runs the same kernels on the same
bytes.  The vocabulary is built from the device's descriptors of the run's own keyframes, as test_gpu_lc_unrect.py does."""
import numpy as np
import pytest

import _kf_log as KL
import _voc as V
from test_gpu_kf_log import CAP, IDS, S, _logged_tracker, _reference
from test_gpu_stream_reset import RIGS, _cfg

pytestmark = pytest.mark.gpu

CFG_ERR, CAP_ERR, INV = -5, -4, -1
PRM = dict(lcKFStart=25, lcKFDist=18, lcKFMaxDist=50, lcKFLast=20, lcNKFClosest=2, ratioMax=0.5, ratioRansac=0.5, minPts=20, minScore=0.12)
EV_FIELDS = ("kf_prev", "kf_curr", "candidate", "n_matches", "n_inliers", "accepted", "optimised", "pgo_iterations", "pose", "chi2_before",
             "chi2_after")


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def _same_event(a, b):
    return [k for k in EV_FIELDS if (_bits(a[k]) != _bits(b[k]) if isinstance(a[k], (float, list)) else a[k] != b[k])]


def _vocabulary(ctx, hist):
    """from the device's descriptors of every third keyframe image of stream 0"""
    import torch
    train = []
    for m in [m for m in hist[0] if m is not None][::3]:
        _, d, c, _ = ctx.orb_detect_and_compute(torch.from_numpy(m["img0"][None]).cuda(), cap=1024)
        train.append(d[0, :int(c[0])].cpu().numpy())
    ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))


def _closer(ctx, cfg, n, unrect, prm=PRM, max_keyframes=CAP, **kw):
    import flvis_amd
    lc = flvis_amd.LoopCloser(ctx, cfg, prm, n_streams=n, max_keyframes=max_keyframes, **kw)
    if unrect:
        lc.set_stereo_unrect(True)
    return lc


def _feed_per_frame(lc, hist):
    """closer A: after every frame, the keyframes that frame made (host images) -> add_keyframes_host + process; events[s][i]"""
    n = len(hist)
    events = [[] for _ in range(n)]
    for f in range(len(hist[0])):
        st = [s for s in range(n) if hist[s][f] is not None]
        if not st:
            continue
        lc.add_keyframes_host(st, [hist[s][f]["img0"] for s in st], [hist[s][f]["img1"] for s in st], [hist[s][f]["pose7"] for s in st])
        ev = lc.process()
        for s in range(n):
            assert (ev[s]["kf_curr"] >= 0) == (s in st)
            if s in st:
                events[s].append(ev[s])
    return events


def _state(lc, s, n_kf):
    return dict(kfs=[lc.keyframe(s, i) for i in range(n_kf)], row=lc.similarity_row(s), poses=lc.poses(s), drift=lc.drift(s))


def _same_state(a, b, what):
    assert len(a["kfs"]) == len(b["kfs"])
    for i, (x, y) in enumerate(zip(a["kfs"], b["kfs"])):
        for k in ("lm2", "lm3", "lmd"):
            assert x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (what, "keyframe", i, k)
        assert np.array_equal(x["bow"][0], y["bow"][0]) and x["bow"][1].tobytes() == y["bow"][1].tobytes(), (what, "keyframe", i, "bow")
    for k in ("row", "poses", "drift"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _check_rounds(rounds, events_a, logged):
    """row r of the logged feed's events: the event of each stream's r-th keyframe, kf_curr = -1 for a stream without one"""
    assert len(rounds) == max(logged)
    for r, row in enumerate(rounds):
        for s, ev in enumerate(row):
            if r < logged[s]:
                assert ev["kf_curr"] == r and _same_event(ev, events_a[s][r]) == [], (r, s, _same_event(ev, events_a[s][r]))
            else:
                assert ev["kf_curr"] == -1


# ---- 7. short run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["d435_stereo", "euroc_like"])
def test_logged_feed_equals_the_per_frame_host_feed(ctx, rig):
    ref = _reference(ctx, rig)
    hist, made = ref["hist"], ref["made"]
    unrect = rig == "euroc_like"
    _vocabulary(ctx, hist)
    A = _closer(ctx, _cfg(rig), S, unrect)
    events_a = _feed_per_frame(A, hist)
    state_a = [_state(A, s, made[s]) for s in range(S)]
    assert all(len(k["lm2"]) > 50 for st in state_a for k in st["kfs"]), "the keyframes store landmarks"
    trk = _logged_tracker(ctx, rig)
    trk.run_steps(ref["steps"], with_local_map=True)
    B = _closer(ctx, _cfg(rig), S, unrect)
    rounds = B.add_logged(process=True)
    _check_rounds(rounds, events_a, made)
    for s in range(S):
        _same_state(state_a[s], _state(B, s, made[s]), (rig, s))
    # the log is not consumed: feeding it again stores it again
    C2 = _closer(ctx, _cfg(rig), S, unrect, max_keyframes=2 * CAP)
    assert len(C2.add_logged(process=False)) == max(made) and len(C2.add_logged(process=False)) == max(made)
    for s in range(S):
        assert len(C2.poses(s)) == 2 * made[s]
        x, y = C2.keyframe(s, 0), C2.keyframe(s, made[s])
        assert x["lmd"].tobytes() == y["lmd"].tobytes() and x["lm3"].tobytes() == y["lm3"].tobytes()
    for c in (A, B, C2):
        c.close()
    del trk


# ---- 8. long run ------------------------------------------------------------------------------------------------------------------
LONG_RIG, LONG_STEPS, LONG_CAP = "euroc_like", 125, 80     # the closer looks for candidates from a sequence's 50th keyframe on


def test_a_long_logged_run_reaches_the_pair_check(ctx):
    """one stream, long enough for loop candidates (the slow sway of the synthetic trajectory brings earlier views back): the pair
    check and the pose graph through the log, against the per-frame host feed"""
    import flvis_amd
    from test_gpu_stream_reset import _frames
    cfg = _cfg(LONG_RIG)
    steps = _frames(1, LONG_STEPS, [IDS[0]], LONG_RIG)
    trk = flvis_amd.Tracker(ctx, cfg, 1, seed_base=1)
    hist = [[]]
    for i0, i1, ts, cnt, blk in steps:
        if cnt[0]:
            trk.imu_feed_flvis(0, blk[0, :cnt[0]])
        out = trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True)
        hist[0].append(trk.keyframe_msg(0) if out[0]["new_keyframe"] else None)
    del trk
    made = sum(m is not None for m in hist[0])
    assert 50 < made <= LONG_CAP, made
    _vocabulary(ctx, hist)
    A = _closer(ctx, cfg, 1, True, max_keyframes=LONG_CAP)
    events_a = _feed_per_frame(A, hist)
    state_a = _state(A, 0, made)
    trk = flvis_amd.Tracker(ctx, cfg, 1, seed_base=1)
    trk.keyframe_log_enable(LONG_CAP)
    trk.run_steps(steps, with_local_map=True)
    assert trk.keyframe_log_info(0) == dict(logged=made, dropped=0, capacity=LONG_CAP)
    B = _closer(ctx, cfg, 1, True, max_keyframes=LONG_CAP)
    rounds = B.add_logged(process=True)
    cand = [r[0] for r in rounds if r[0]["candidate"]]
    print("%d keyframes, %d candidates, %d accepted, %d pose-graph runs" % (made, len(cand), sum(e["accepted"] for e in cand),
                                                                            sum(e["optimised"] for e in cand)))
    assert len(cand) >= 1 and all(e["kf_prev"] >= 0 and e["n_matches"] > 0 for e in cand)
    _check_rounds(rounds, events_a, [made])
    _same_state(state_a, _state(B, 0, made), "long run")
    A.close()
    B.close()
    del trk


# ---- 9. error paths ---------------------------------------------------------------------------------------------------------------
def test_capacity_and_config_are_checked_before_anything_is_stored(ctx):
    import flvis_amd
    rig = "d435_stereo"
    ref = _reference(ctx, rig)
    made = ref["made"]
    _vocabulary(ctx, ref["hist"])
    trk = _logged_tracker(ctx, rig)
    trk.run_steps(ref["steps"], with_local_map=True)
    # one slot short for the stream with the most keyframes -- after a first keyframe of each stream, so that there is a state to keep
    lc = _closer(ctx, _cfg(rig), S, False, max_keyframes=max(made))
    first = [[m for m in h if m is not None][0] for h in ref["hist"]]
    lc.add_keyframes_host(list(range(S)), [m["img0"] for m in first], [m["img1"] for m in first], [m["pose7"] for m in first])
    lc.process()
    before = [_state(lc, s, 1) for s in range(S)]
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CAP_ERR):
        lc.add_logged(process=True)
    for s in range(S):
        _same_state(before[s], _state(lc, s, 1), ("after the refusal", s))
        with pytest.raises(flvis_amd.FlvisError):
            lc.keyframe(s, 1)
    # too few event rows: refused as well, nothing stored
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        _closer(ctx, _cfg(rig), S, False).add_logged(process=True, max_rounds=max(made) - 1)
    lc.close()
    # a closer of another image size
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        _closer(ctx, _cfg("euroc_like"), S, False).add_logged()
    # ... of another stream count
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        _closer(ctx, _cfg(rig), S + 1, False).add_logged()
    # the log off
    trk.keyframe_log_enable(0)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        _closer(ctx, _cfg(rig), S, False).add_logged()
    del trk
