"""FLVIS_CHAIN_MERGE bits 2-4: three more launches of the frame's chain folded into their neighbours -- k_depth_innovate + k_frame_end
(4), k_feature_dem in front of k_add_new + k_depth_seeds (8), k_reproj_filter as the epilogue of k_pose_lm (16).  Every form must leave
what the launches of FLVIS_CHAIN_MERGE=3 leave, bit for bit: the folds change where a kernel boundary lies, not one operation or the
order of one sum.  Same rig and helpers as test_chain_merge_forms_leave_the_same_results; 3 streams, the skip window + 14 frames, the
first half frame by frame (FrameOut per frame), the second half as one flvis_run_steps batch.

(The s_full branch of the merged frame end -- a keyframe met by a full queue -- has no case here: no entry point fills a stream's
keyframe queue, the back-pressure keeps it below its capacity whatever the local map's pace, and a test that blocks the local map on
purpose is not one to have.)"""
import numpy as np
import pytest

from test_gpu_pipeline import _assert_same_run, _cfgs, _mode_frames

pytestmark = pytest.mark.gpu

S = 3
NPROC = 14  # processed frames behind the skip window
KNOBS = ("FLVIS_CHAIN_MERGE", "FLVIS_JOIN", "FLVIS_JOIN_FOLD")


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rig(ctx):
    """(cfg, skip, the frames): rendered once, read only"""
    cfg, _ = _cfgs()
    skip = int(cfg.skip_first_n_imgs)
    return cfg, skip, _mode_frames(S, skip + NPROC, [2 + 5 * i for i in range(S)])


def _result(trk, ctx, n):
    """_mode_result's tuple with the landmarks and the CorrectionInf of every stream"""
    ctx.synchronize()
    rows = np.stack([trk.trajectory(i, 0, n) for i in range(S)])
    kf, ba = trk.local_map_counts()
    return rows, [trk.landmarks(i) for i in range(S)], [trk.correction(i) for i in range(S)], list(trk.counters()), kf, ba


def _run(ctx, monkeypatch, rig, env, with_local_map=True, absent=(), reset_at=None, frames=None):
    """One run under the environment `env`.  absent: (step, stream) pairs without a frame; reset_at: the step in front of which stream 1
    is reset.  -> (FrameOut of the frame-by-frame half, _result)"""
    import flvis_amd
    cfg, skip, fr = rig
    fr = fr if frames is None else frames
    n = len(fr)
    half = skip + NPROC // 2
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pres = np.ones((n, S), np.uint8)
    for k, s in absent:
        pres[k, s] = 0
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715, traj_capacity=n)
    outs = []
    for k, (i0, i1, ts, cnt, blk) in enumerate(fr[:half]):
        if reset_at == k:
            trk.reset_streams([1])
        for i in range(S):
            trk.imu_feed_flvis(i, blk[i, :cnt[i]])
        o = trk.image_feed(i0, i1, ts, want_out=True, with_local_map=with_local_map, present=None if pres[k].all() else pres[k])
        outs.append([(d["state"], d["new_keyframe"], d["reset_cmd"], d["n_landmarks"], d["frame_id"], d["pose7"].tobytes(),
                      d["dbg"].tobytes(), np.float64(d["reprojection_error"]).tobytes()) for d in o])
    if reset_at is not None and reset_at >= half:
        trk.reset_streams([1])
    trk.run_steps(fr[half:], with_local_map=with_local_map, present=None if pres[half:].all() else pres[half:])
    res = _result(trk, ctx, n)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    del trk
    return outs, res


def _assert_same(a, b, what):
    assert a[0] == b[0], (what, "FrameOut", [k for k, (x, y) in enumerate(zip(a[0], b[0])) if x != y][:4])
    _assert_same_run(a[1], b[1], what)


def _kf_bits(res, skip):
    """[S][NPROC] new_keyframe of the processed frames, from the trajectory rows"""
    return (res[1][0][:, skip:, 8].astype(int) >> 4) & 1


def test_fold_settings_leave_the_same_results(ctx, monkeypatch, rig):
    """FLVIS_CHAIN_MERGE = 7, 11, 19, 31 and the knob unset against 3: FrameOut of every frame fed singly, the trajectory rows of every
    frame, the landmarks of the last frame, the local map's counts and the last CorrectionInf, bit for bit.  Every stream makes a
    keyframe in some frames and none in others: both ways through the merged frame end."""
    skip = rig[1]
    ref = _run(ctx, monkeypatch, rig, {"FLVIS_CHAIN_MERGE": "3"})
    rows = ref[1][0]
    assert np.all((rows[:, skip:, 8].astype(int) & 15) == 1), "every stream tracks from its first processed frame on"
    kf = _kf_bits(ref, skip)
    assert np.all(kf.any(axis=1)) and not np.any(kf.all(axis=1)), kf
    for m in ("7", "11", "19", "31", None):
        _assert_same(ref, _run(ctx, monkeypatch, rig, {} if m is None else {"FLVIS_CHAIN_MERGE": m}), ("FLVIS_CHAIN_MERGE", m))


def _pair(ctx, monkeypatch, rig, env=None, **kw):
    a = _run(ctx, monkeypatch, rig, dict(env or {}, FLVIS_CHAIN_MERGE="3"), **kw)
    b = _run(ctx, monkeypatch, rig, dict(env or {}, FLVIS_CHAIN_MERGE="31"), **kw)
    return a, b


def test_folds_without_local_map(ctx, monkeypatch, rig):
    """with_local_map = 0: the merged frame end without the back-pressure waits, the queues dropped behind it"""
    a, b = _pair(ctx, monkeypatch, rig, with_local_map=False)
    assert _kf_bits(a, rig[1]).any()
    _assert_same(a, b, "no local map")


def test_folds_with_an_absent_stream(ctx, monkeypatch, rig):
    """stream 1 has no frame in one step fed singly and in one step of the batch: those steps keep the stand-alone k_frame_end, the
    merged launches around them go on"""
    skip = rig[1]
    absent = ((skip + 3, 1), (skip + NPROC // 2 + 2, 1))
    a, b = _pair(ctx, monkeypatch, rig, absent=absent)
    o = a[0]
    assert o[skip + 3][1] == o[skip + 2][1] and o[skip + 3][0] != o[skip + 2][0], "an absent stream's FrameOut stays its last frame's"
    _assert_same(a, b, "absent stream")


def test_folds_with_a_stream_reset(ctx, monkeypatch, rig):
    """flvis_reset_streams([1]) in the middle: the stream initialises again (init_frame through the merged FeatureDEM launch and the
    merged frame end) beside streams that track"""
    skip = rig[1]
    a, b = _pair(ctx, monkeypatch, rig, reset_at=skip + 4)
    _assert_same(a, b, "stream reset")
    plain = _run(ctx, monkeypatch, rig, {"FLVIS_CHAIN_MERGE": "3"})
    assert a[0][skip + 4][1] != plain[0][skip + 4][1] and a[0][skip + 4][0] == plain[0][skip + 4][0], "the reset shows in stream 1 alone"


def test_folds_with_a_tracking_failure(ctx, monkeypatch, rig):
    """stream 1 sees a constant image for three frames: its tracking fails in front of the pose optimisation (track_fail in k_pose_lm's
    prologue), so the merged launch's filter epilogue meets a stream that left the frame; the stream then initialises again"""
    cfg, skip, fr = rig
    frames = list(fr)
    for k in range(skip + 3, skip + 6):
        i0, i1, ts, cnt, blk = fr[k]
        i0, i1 = i0.clone(), i1.clone()
        i0[1] = 128
        i1[1] = 128
        frames[k] = (i0, i1, ts, cnt, blk)
    a, b = _pair(ctx, monkeypatch, rig, frames=frames)
    st = a[1][0][:, skip:, 8].astype(int) & 15
    assert np.any(st[1] != 1) and np.all(st[0] == 1) and np.all(st[2] == 1), st
    _assert_same(a, b, "tracking failure")


@pytest.mark.parametrize("env", [{"FLVIS_JOIN": "event"}, {"FLVIS_JOIN_FOLD": "0"}], ids=["event", "unfolded"])
def test_folds_with_other_joins(ctx, monkeypatch, rig, env):
    """the joins as events, and as flag launches beside the kernels: the merged launches' waits and signals on the stream instead of
    inside them"""
    a, b = _pair(ctx, monkeypatch, rig, env=env)
    _assert_same(a, b, env)
