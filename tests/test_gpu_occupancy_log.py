"""GPU: the occupancy map through the pipeline (flvis_keyframe_log_occupancy, flvis_loop_closer_occupancy; include/flvis_hip.h) against
the core call and the restatement (tests/_occupancy.py) on what the host can fetch: keyframe_log_get's depth images and poses,
LoopCloser.poses.

The set-up is test_gpu_dense_cloud.py's: two streams of the synthetic D435i depth rig on rigs with different depth_factor.  The run is
made twice with the same seed, once making every occupancy call and once making none: everything a caller can fetch afterwards is compared
bit for bit.  The context holds one tracker at a time."""
import numpy as np
import pytest

import _depth_cloud as DC
import _kf_log as KL
import _occupancy as OC
import _voc as V
from test_gpu_dense_cloud import DRIFT, RIG, S, TAIL, _cam, _case, _cfgs
from test_gpu_kf_log import CAP, IDS, STEPS
from test_gpu_kf_log_closer import _closer, _same_event, _vocabulary
from test_gpu_stream_reset import _cfg, _frames

pytestmark = pytest.mark.gpu

CFG_ERR, INV, CAPACITY = -5, -1, -4
LEAF = 0.16
SAMPLING = dict(step=16, z_min=0.3, z_max=6.5)
PRM_DICT = DC.params(None, (16, 16), 0.3, 6.5)


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _map_case(entries, poses, seqs):
    return dict(_case(entries, poses, seqs), prm=PRM_DICT)


def _same_rows(a, b, g, h, what):
    assert np.array_equal(a[0][g], b[0][h]) and a[1][g].tobytes() == b[1][h].tobytes() and a[2][g].tobytes() == b[2][h].tobytes(), what
    assert (a[3][g], a[4][g], a[5][g]) == (b[3][h], b[4][h], b[5][h]), what


def _check(got, g, want, what):
    assert (int(got[3][g]), int(got[4][g]), int(got[5][g])) == (want["n_out"], want["n_rays"], want["n_dropped"]), what
    assert np.array_equal(got[0][g], want["keys"]) and got[1][g].tobytes() == want["l"].tobytes() and got[2][g].tobytes() == want["xyz"].tobytes(), what


def _core(ctx, case):
    import torch
    d = torch.from_numpy(case["depth"].view(np.int16).copy()).cuda()
    T = torch.from_numpy(np.ascontiguousarray(case["T"], np.float64)).cuda()
    return ctx.occupancy(d, T, case["clouds"], case["cams"], leaf=LEAF, **SAMPLING)


def _pipeline(ctx, frames, calls):
    """test_gpu_dense_cloud.py's pipeline with the occupancy calls in the dense calls' places -> everything a caller can fetch"""
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
        got = trk.keyframe_log_occupancy([0, 1, 1], leaf=LEAF, **SAMPLING)
        assert got[6] == 1, "2^26 records hold this log: one batch"
        for g, s in enumerate([0, 1, 1]):
            case = _map_case(entries, logged, [s])
            _same_rows(got, _core(ctx, case), g, 0, ("log against the core call", s))
        _check(got, 0, OC.restate(_map_case(entries, logged, [0]), 0, LEAF), "log against the restatement")
        assert (got[1][0] > 0).any() and (got[1][0] < 0).any()
        # batches: the per-scan records from the restatement's own count; a limit that holds the largest scan and no two of the larger ones
        rec = [OC.restate(dict(_map_case(entries, logged, [s]), clouds=[[(i, 1)]]), 0, LEAF)["records"] for s in (0, 1) for i in range(made[s])]
        small = max(rec)
        batched = trk.keyframe_log_occupancy([0, 1, 1], leaf=LEAF, max_records=small, **SAMPLING)
        assert batched[6] >= 3, (batched[6], rec)
        for g in range(3):
            _same_rows(batched, got, g, g, ("batches against one batch", g))
        assert ctx.occupancy_stats()["batches"] == batched[6]
        host = trk.keyframe_log_occupancy([1, 0], leaf=LEAF, host=True, max_records=small, slices=[(1, 1), (0, 10 ** 6)], **SAMPLING)
        one = dict(depth=entries[1][1]["img1"][None], T=np.array([logged[1][1]]), clouds=[[(0, 1)]], cams=[_cam(cfgs[1])], prm=PRM_DICT)
        _check(host, 0, OC.restate(one, 0, LEAF), "host, a slice of one entry")
        _same_rows(host, got, 1, 0, "host, a slice past the log")
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\).*entry \d+ of stream \d+" % CAPACITY):
            trk.keyframe_log_occupancy([0, 1], leaf=LEAF, max_records=small - 1, **SAMPLING)
        for bad in ([S], [-1], []):
            with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
                trk.keyframe_log_occupancy(bad, leaf=LEAF, **SAMPLING)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            trk.keyframe_log_occupancy([0], leaf=LEAF, max_records=-1, **SAMPLING)
    _vocabulary(ctx, entries)
    lc = _closer(ctx, cfgs, S, False, max_keyframes=2 * CAP)
    rounds = lc.add_logged(process=True)
    if calls:
        poses = [lc.poses(s) for s in range(S)]
        got = lc.occupancy([[0], [1, 0]], leaf=LEAF, **SAMPLING)
        for g, seqs in enumerate([[0], [1, 0]]):
            _same_rows(got, _core(ctx, _map_case(entries, poses, seqs)), g, 0, ("closer against the core call", seqs))
        _same_rows(lc.occupancy([[1, 0]], leaf=LEAF, host=True, max_records=small, **SAMPLING), got, 0, 1, "closer, host, batches")
    lc.set_drift(1, DRIFT)
    lc.add_logged(process=False)                                          # the log is not consumed: each sequence holds it twice now
    if calls:
        poses = [lc.poses(s) for s in range(S)]
        second = [poses[s][made[s]:] for s in range(S)]
        got = lc.occupancy([[1]], first_kf=[[made[1]]], leaf=LEAF, **SAMPLING)
        _same_rows(got, _core(ctx, _map_case(entries, second, [1])), 0, 0, "after set_drift")
        before = lc.occupancy([[1]], leaf=LEAF, **SAMPLING)
        assert before[0][0].tobytes() != got[0][0].tobytes(), "the map moves with the drift"
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            lc.occupancy([[1]], first_kf=[[2 * made[1] + 1]], leaf=LEAF, **SAMPLING)
    state = [dict(poses=lc.poses(s), drift=lc.drift(s), row=lc.similarity_row(s)[:made[s]]) for s in range(S)]
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


def test_occupancy_maps_equal_the_core_call_and_change_nothing(ctx):
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
    for host in (False, True):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
            trk.keyframe_log_occupancy([0], leaf=LEAF, host=host, **SAMPLING)
    ctx.bow_set_vocabulary(*V.build_vocabulary([np.random.default_rng(4).integers(0, 256, (600, 32)).astype(np.uint8)], k=8, depth=3))
    lc = _closer(ctx, _cfg("d435_stereo"), 1, False)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        lc.occupancy([[0]], leaf=LEAF, **SAMPLING)
    lc.close()
    del trk
    trk = flvis_amd.Tracker(ctx, _cfg(RIG), 1, seed_base=1)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        trk.keyframe_log_occupancy([0], leaf=LEAF, **SAMPLING)                # the log is off
    trk.keyframe_log_enable(4)
    got = trk.keyframe_log_occupancy([0], leaf=LEAF, **SAMPLING)              # on and empty
    assert got[3][0] == 0 and got[4][0] == 0 and len(got[0][0]) == 0 and got[6] == 0
    del trk
