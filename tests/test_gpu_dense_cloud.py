"""GPU: the dense map through the pipeline (flvis_keyframe_log_depth_cloud, flvis_loop_closer_dense_cloud; include/flvis_hip.h) against
the restatement (tests/_depth_cloud.py) on what the host can fetch: keyframe_log_get's depth images and poses, LoopCloser.poses.

Two streams of the synthetic D435i depth rig on rigs with different depth_factor, the step count test_gpu_kf_log.py uses for its depth
case.  The run is made twice with the same seed, once making every dense call and once making none: everything a caller can fetch
afterwards is compared bit for bit.  The context holds one tracker at a time."""
import numpy as np
import pytest

import _depth_cloud as DC
import _kf_log as KL
import _voc as V
from test_gpu_kf_log import CAP, IDS, STEPS
from test_gpu_kf_log_closer import PRM, _closer, _same_event, _vocabulary
from test_gpu_stream_reset import _cfg, _frames

pytestmark = pytest.mark.gpu

RIG, S, TAIL = "d435_depth", 2, 5
CFG_ERR, INV = -5, -1
SAMPLING = dict(step=7, z_min=0.3, z_max=10.0)
PRM_DICT = DC.params(None, (7, 7), 0.3, 10.0)
DRIFT = [0.3, -0.2, 0.1, 0.0, 0.0, np.sin(0.1), np.cos(0.1)]


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _cfgs():
    a, b = _cfg(RIG), _cfg(RIG)
    b.depth_factor = a.depth_factor * 1.0025          # another rig: the same scene a quarter of a percent nearer
    return [a, b]


def _cam(cfg):
    return [cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6], cfg.depth_factor]


def _case(entries, poses, seqs):
    """one cloud over the listed sequences' entries, each sequence a range on its own camera.  poses[s]: one pose per used entry"""
    cfgs = _cfgs()
    depth, T, ranges, cams = [], [], [], []
    for s in seqs:
        n = len(poses[s])
        ranges.append((len(depth), n))
        cams.append(_cam(cfgs[s]))
        depth += [e["img1"] for e in entries[s][:n]]
        T += list(poses[s])
    return dict(depth=np.stack(depth), T=np.array(T), clouds=[ranges], cams=cams, prm=PRM_DICT)


def _check(got, g, want, what):
    xyz, npts, n_out, n_drop, n_valid = got
    assert (int(n_out[g]), int(n_drop[g]), int(n_valid[g])) == (want["n_out"], want["n_dropped"], want["n_valid"]), what
    assert xyz[g].tobytes() == want["xyz"].tobytes() and np.array_equal(npts[g], want["npts"]), what


def _pipeline(ctx, frames, calls):
    """the batch, the log into a closer, a drift and the log again, then TAIL more frames one by one.  calls: make the dense calls (and
    check them against the restatement) between those steps -> everything a caller can fetch"""
    import flvis_amd
    cfgs = _cfgs()
    trk = flvis_amd.Tracker(ctx, cfgs, S, seed_base=1)
    trk.keyframe_log_enable(CAP)
    trk.run_steps(frames[:STEPS[RIG]], with_local_map=True)
    made = [trk.keyframe_log_info(s)["logged"] for s in range(S)]
    assert min(made) >= 2 and max(made) <= CAP, made
    entries = [[trk.keyframe_log_get(s, i) for i in range(made[s])] for s in range(S)]
    logged = [[e["pose7"] for e in entries[s]] for s in range(S)]
    if calls:
        for s in range(S):
            for i, e in enumerate(entries[s]):
                assert len(DC.samples(e["img1"], _cam(cfgs[s]), PRM_DICT)[0]) >= 1, (s, i)
        for leaf in (0.08, 0.0):
            got = trk.keyframe_log_depth_cloud([0, 1, 1], leaf=leaf, slices=None, **SAMPLING)
            for g, s in enumerate([0, 1, 1]):
                _check(got, g, DC.restate(_case(entries, logged, [s]), 0, leaf), ("log", leaf, s))
        host = trk.keyframe_log_depth_cloud([1, 0], leaf=0.08, host=True, slices=[(1, 1), (0, 10 ** 6)], **SAMPLING)
        one = dict(depth=entries[1][1]["img1"][None], T=np.array([logged[1][1]]), clouds=[[(0, 1)]], cams=[_cam(cfgs[1])], prm=PRM_DICT)
        _check(host, 0, DC.restate(one, 0, 0.08), "host, a slice of one entry")
        _check(host, 1, DC.restate(_case(entries, logged, [0]), 0, 0.08), "host, a slice past the log")
        # the camera is the stream's own: stream 1 under stream 0's depth_factor gives other bits
        wrong = _case(entries, logged, [1])
        wrong["cams"] = [_cam(cfgs[0])]
        assert DC.restate(wrong, 0, 0.08)["xyz"].tobytes() != DC.restate(_case(entries, logged, [1]), 0, 0.08)["xyz"].tobytes()
        for bad in ([S], [-1], []):
            with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
                trk.keyframe_log_depth_cloud(bad, **SAMPLING)
    _vocabulary(ctx, entries)
    lc = _closer(ctx, cfgs, S, False, max_keyframes=2 * CAP)
    rounds = lc.add_logged(process=True)
    if calls:
        poses = [lc.poses(s) for s in range(S)]
        got = lc.dense_cloud([[0], [1], [1, 0]], leaf=0.08, **SAMPLING)
        for g, seqs in enumerate([[0], [1], [1, 0]]):
            _check(got, g, DC.restate(_case(entries, poses, seqs), 0, 0.08), ("closer", seqs))
        _check(lc.dense_cloud([[0]], leaf=0.0, host=True, **SAMPLING), 0, DC.restate(_case(entries, poses, [0]), 0, 0.0), "closer, host")
    lc.set_drift(1, DRIFT)
    lc.add_logged(process=False)                                          # the log is not consumed: each sequence holds it twice now
    if calls:
        poses = [lc.poses(s) for s in range(S)]
        assert [len(p) for p in poses] == [2 * m for m in made]
        second = [poses[s][made[s]:] for s in range(S)]
        assert second[1].tobytes() != poses[1][:made[1]].tobytes(), "sequence 1's second copy is stored under the drift"
        got = lc.dense_cloud([[1], [0], [1]], first_kf=[[made[1]], [made[0]], [2 * made[1] - 1]], leaf=0.08, **SAMPLING)
        _check(got, 0, DC.restate(_case(entries, second, [1]), 0, 0.08), "after set_drift")
        _check(got, 1, DC.restate(_case(entries, second, [0]), 0, 0.08), "the other sequence")
        _check(got, 2, DC.restate(_case(entries, [None, poses[1][-1:]], [1]), 0, 0.08), "a first keyframe that leaves one stored keyframe")
        before = lc.dense_cloud([[1]], leaf=0.08, **SAMPLING)
        assert before[0][0].tobytes() != got[0][0].tobytes(), "the cloud follows the drift"
        for bad in ([[2 * made[1] + 1]], [[-1]]):
            with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
                lc.dense_cloud([[1]], first_kf=bad, **SAMPLING)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            lc.dense_cloud([[0, 0]], **SAMPLING)
    # (the newest similarity row is the one the last process computed: made[s] entries, although the sequence holds twice as many by now;
    # what lies behind them in the buffer was never written)
    state = [dict(poses=lc.poses(s), drift=lc.drift(s), row=lc.similarity_row(s)[:made[s]]) for s in range(S)]
    print("dense cloud run (calls: %s): keyframes per stream %s" % (calls, made))
    after = [[trk.keyframe_log_get(s, i) for i in range(made[s])] for s in range(S)]
    outs = []
    for i0, i1, ts, cnt, blk in frames[STEPS[RIG]:]:
        for s in range(S):
            if cnt[s]:
                trk.imu_feed_flvis(s, blk[s, :cnt[s]])
        outs.append(trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True))
    info = [trk.keyframe_log_info(s) for s in range(S)]
    lc.close()
    del trk
    return dict(entries=entries, after=after, rounds=rounds, state=state, outs=outs, info=info)


def test_dense_clouds_equal_the_restatement_and_change_nothing(ctx):
    frames = _frames(S, STEPS[RIG] + TAIL, IDS[:S], RIG)
    a = _pipeline(ctx, frames, calls=True)
    b = _pipeline(ctx, frames, calls=False)
    for s in range(S):
        assert len(a["entries"][s]) == len(b["entries"][s])
        for x, y, z in zip(a["entries"][s], a["after"][s], b["after"][s]):
            assert KL.differences(x, y) == [] and KL.differences(x, z) == [], "the log's entries"
        for k in ("poses", "drift", "row"):
            assert a["state"][s][k].tobytes() == b["state"][s][k].tobytes(), (s, k)
    assert a["info"] == b["info"]
    assert len(a["rounds"]) == len(b["rounds"])
    for ra, rb in zip(a["rounds"], b["rounds"]):
        for ea, eb in zip(ra, rb):
            assert _same_event(ea, eb) == []
    assert len(a["outs"]) == TAIL
    for oa, ob in zip(a["outs"], b["outs"]):
        for s in range(S):
            for k in oa[s]:
                assert np.asarray(oa[s][k]).tobytes() == np.asarray(ob[s][k]).tobytes(), ("the tracker's next frames", s, k)


def test_a_stereo_rig_and_a_log_that_is_off_are_refused(ctx):
    import flvis_amd
    trk = flvis_amd.Tracker(ctx, _cfg("d435_stereo"), 1, seed_base=1)
    trk.keyframe_log_enable(4)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        trk.keyframe_log_depth_cloud([0], **SAMPLING)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        trk.keyframe_log_depth_cloud([0], host=True, **SAMPLING)
    ctx.bow_set_vocabulary(*V.build_vocabulary([np.random.default_rng(4).integers(0, 256, (600, 32)).astype(np.uint8)], k=8, depth=3))
    lc = _closer(ctx, _cfg("d435_stereo"), 1, False)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        lc.dense_cloud([[0]], **SAMPLING)
    lc.close()
    del trk
    trk = flvis_amd.Tracker(ctx, _cfg(RIG), 1, seed_base=1)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        trk.keyframe_log_depth_cloud([0], **SAMPLING)                     # the log is off
    trk.keyframe_log_enable(4)
    got = trk.keyframe_log_depth_cloud([0], **SAMPLING)                   # on and empty
    assert got[2][0] == 0 and got[4][0] == 0 and len(got[0][0]) == 0
    del trk
