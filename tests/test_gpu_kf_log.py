"""GPU: the keyframe log (flvis_keyframe_log_*, include/flvis_hip.h) -- the per-stream record k_kf_log_append fills behind k_frame_end --
against the flvis/KeyFrame messages a per-frame caller gets from flvis_get_keyframe_msg right after every keyframe, bit for bit, and the
numpy restatement of the record (tests/_kf_log.py).

3 streams on different trajectories of a synthetic rig (so that a step has a keyframe in some streams and not in others).  The context
holds one tracker at a time: the reference (one image_feed per frame, keyframe_msg after every keyframe) and the logged runs are made one
after the other with the same seed_base.  The references are computed once per rig, shared and left unchanged."""
import numpy as np
import pytest

import _kf_log as KL
from test_gpu_stream_reset import RIGS, _cfg, _frames

pytestmark = pytest.mark.gpu

S = 3
IDS = [3, 120, 250]
CAP = 40
INV = -1            # FLVIS_ERR_INVALID_ARG
# steps per rig: the D435i rigs make their first keyframe at step 50 (the IMU filter initialises first), the other two in their first
# steps; from then on a stream makes one every one to three steps -- 8 or more per stream by the end
STEPS = {"d435_stereo": 75, "euroc_like": 24, "d435_depth": 75, "kitti_like": 24}


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _per_frame(ctx, rig, steps, traj=True):
    """one image_feed per frame, keyframe_msg after every keyframe -> (history[s][f] = message or None, trajectory rows per stream)"""
    import flvis_amd
    trk = flvis_amd.Tracker(ctx, _cfg(rig), S, seed_base=1, traj_capacity=len(steps))
    hist = [[] for _ in range(S)]
    for i0, i1, ts, cnt, blk in steps:
        for s in range(S):
            if cnt[s]:
                trk.imu_feed_flvis(s, blk[s, :cnt[s]])
        out = trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True)
        for s in range(S):
            msg = trk.keyframe_msg(s) if out[s]["new_keyframe"] else None
            assert (msg is not None) == out[s]["new_keyframe"]
            hist[s].append(msg)
    ctx.synchronize()
    rows = [trk.trajectory(s, 0, len(steps)) for s in range(S)]
    del trk
    return hist, rows


_refs = {}


def _reference(ctx, rig):
    if rig not in _refs:
        steps = _frames(S, STEPS[rig], IDS, rig)
        hist, rows = _per_frame(ctx, rig, steps)
        made = [sum(m is not None for m in h) for h in hist]
        print("%s: keyframes per stream %s" % (rig, made))
        assert min(made) >= 4, made
        flags = np.array([[m is not None for m in h] for h in hist])           # [S][steps]
        mixed = int((flags.any(axis=0) & ~flags.all(axis=0)).sum())
        print("%s: steps with a keyframe in some streams and not in others: %d" % (rig, mixed))
        assert mixed >= 3
        _refs[rig] = dict(steps=steps, hist=hist, rows=rows, made=made)
    return _refs[rig]


def _logged_tracker(ctx, rig, cap=CAP, traj=0):
    import flvis_amd
    trk = flvis_amd.Tracker(ctx, _cfg(rig), S, seed_base=1, traj_capacity=traj)
    if cap is not None:
        trk.keyframe_log_enable(cap)
    return trk


def _check_log(trk, s, want, cap=CAP, what=""):
    """stream s's log == the restated record `want` (KL.record): counts, and every entry equal to its message in every field"""
    info = trk.keyframe_log_info(s)
    assert info == dict(logged=len(want["entries"]), dropped=want["dropped"], capacity=cap), (what, s, info, len(want["entries"]), want["dropped"])
    for i, msg in enumerate(want["entries"]):
        got = trk.keyframe_log_get(s, i)
        assert KL.differences(got, msg) == [], (what, "stream", s, "entry", i, KL.differences(got, msg))


# ---- 1. the four rigs: each another copy path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["d435_stereo", "euroc_like", "kitti_like", "d435_depth"])
def test_log_equals_the_per_frame_messages(ctx, rig):
    """D435i stereo 640 x 480: the right image read in place; EuRoC-like 752 x 480: both images the tracker's own, img0 equalised;
    KITTI-like 1241 x 376: rows not dword aligned; D435i depth: the 16-bit img1 read in place"""
    import torch
    ref = _reference(ctx, rig)
    trk = _logged_tracker(ctx, rig)
    trk.run_steps(ref["steps"], with_local_map=True)
    for s in range(S):
        _check_log(trk, s, KL.record(ref["hist"][s], CAP), what=rig)
    # the device views are the same bytes
    g = trk.keyframe_log_get(1, 2)
    v0, v1 = trk.keyframe_log_images(1, 2)
    assert np.array_equal(v0.cpu().numpy(), g["img0"]) and np.array_equal(v1.cpu().numpy().view(g["img1"].dtype), g["img1"])
    assert g["img1"].dtype == (np.uint16 if rig == "d435_depth" else np.uint8)
    with pytest.raises(Exception, match=r"failed \(%d\)" % INV):
        trk.keyframe_log_get(1, ref["made"][1])                         # one past the last entry
    if rig == "euroc_like":
        # img0 is the EQUALISED image: not the frame's input, but equalizeHist of it
        f = [k for k, m in enumerate(ref["hist"][1]) if m is not None][2]
        raw = ref["steps"][f][0][1]
        assert not np.array_equal(g["img0"], raw.cpu().numpy())
        assert np.array_equal(g["img0"], ctx.equalize_hist(raw[None].contiguous())[0].cpu().numpy())
    elif rig != "kitti_like":
        f = [k for k, m in enumerate(ref["hist"][1]) if m is not None][2]
        assert np.array_equal(g["img0"], ref["steps"][f][0][1].cpu().numpy())
    del trk


# ---- 2. capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity_two_keeps_a_prefix_and_clear_starts_over(ctx):
    rig = "d435_stereo"
    ref = _reference(ctx, rig)
    steps, hist = ref["steps"], ref["hist"]
    # the first batch ends when every stream has made three keyframes or more: each has dropped at least one
    M = 1 + max([k for k, m in enumerate(h) if m is not None][2] for h in hist)
    assert all(sum(m is not None for m in h[M:]) >= 1 for h in hist), "no keyframe is left for the second batch"
    trk = _logged_tracker(ctx, rig, cap=2)
    trk.run_steps(steps[:M], with_local_map=True)
    for s in range(S):
        want = KL.record(hist[s][:M], 2)
        assert len(want["entries"]) == 2 and want["dropped"] == sum(m is not None for m in hist[s][:M]) - 2 >= 1
        _check_log(trk, s, want, cap=2, what="first batch")
    # the records lie one behind the other: stream 1's starts where stream 0's two entries end -- and holds what a log with room for
    # everything holds (test 1), although stream 0 went on making keyframes after its record was full
    px = steps[0][0].shape[1] * steps[0][0].shape[2]
    a0, _ = trk.keyframe_log_images(0, 0)
    b0, _ = trk.keyframe_log_images(1, 0)
    assert b0.data_ptr() - a0.data_ptr() == 2 * px
    # cleared, the streams log again from entry 0
    trk.keyframe_log_clear([0, 2])
    assert trk.keyframe_log_info(0) == dict(logged=0, dropped=0, capacity=2)
    assert trk.keyframe_log_info(1)["logged"] == 2
    trk.run_steps(steps[M:], with_local_map=True)
    for s in (0, 2):
        _check_log(trk, s, KL.record(hist[s][M:], 2), cap=2, what="after clear")
    _check_log(trk, 1, KL.record(hist[1], 2), cap=2, what="not cleared")
    del trk


# ---- 3. presence ------------------------------------------------------------------------------------------------------------------
def test_an_absent_stream_logs_as_if_fed_its_present_frames_alone(ctx):
    """stream 1 absent in every third step (KITTI-like rig: no IMU, so the run of its present frames alone is those steps in order)"""
    rig = "kitti_like"
    ref = _reference(ctx, rig)
    steps = ref["steps"]
    pres = np.ones((len(steps), S), np.uint8)
    pres[2::3, 1] = 0
    trk = _logged_tracker(ctx, rig)
    trk.run_steps(steps, with_local_map=True, present=pres)
    n1 = trk.keyframe_log_info(1)
    got = [trk.keyframe_log_get(1, i) for i in range(n1["logged"])]
    for s in (0, 2):                                                     # (the streams that are always present: as without presence)
        _check_log(trk, s, KL.record(ref["hist"][s], CAP), what="present throughout")
    del trk
    alone = [st for k, st in enumerate(steps) if pres[k, 1]]
    trk = _logged_tracker(ctx, rig)
    trk.run_steps(alone, with_local_map=True)
    n1a = trk.keyframe_log_info(1)
    assert n1 == n1a and n1["logged"] >= 3 and n1["dropped"] == 0, (n1, n1a)
    for i, g in enumerate(got):
        assert KL.differences(g, trk.keyframe_log_get(1, i)) == [], i
    del trk


# ---- 4. reset ---------------------------------------------------------------------------------------------------------------------
def test_reset_streams_empties_the_named_record_only(ctx):
    """KITTI-like rig (a new sequence tracks from its first frames): stream 1 reset between two batches"""
    import flvis_amd
    rig = "kitti_like"
    ref = _reference(ctx, rig)
    steps, hist = ref["steps"], ref["hist"]
    M = len(steps) // 2
    assert all(sum(m is not None for m in h[:M]) >= 1 for h in hist)
    trk = _logged_tracker(ctx, rig)
    trk.run_steps(steps[:M], with_local_map=True)
    trk.local_map_reset([0])                                              # (leaves the record alone)
    trk.reset_streams([1])
    trk.run_steps(steps[M:], with_local_map=True)
    for s in (0, 2):
        _check_log(trk, s, KL.record(hist[s], CAP), what="not reset")
    n1 = trk.keyframe_log_info(1)
    got = [trk.keyframe_log_get(1, i) for i in range(n1["logged"])]
    del trk
    # the new sequence: stream 1 of a new tracker fed the second batch from its first frame
    fresh, _ = _per_frame(ctx, rig, steps[M:])
    want = KL.record(fresh[1], CAP)
    assert n1 == dict(logged=len(want["entries"]), dropped=0, capacity=CAP) and n1["logged"] >= 2, n1
    for g, w in zip(got, want["entries"]):
        assert KL.differences(g, w) == []
    # entry 0 is the new sequence's first keyframe (its stamp lies in the second batch), not the old sequence's
    assert got[0]["stamp"] >= steps[M][2][1] > [m for m in hist[1] if m is not None][0]["stamp"]


# ---- 5. lanes ---------------------------------------------------------------------------------------------------------------------
def test_two_lanes_with_input_hold_log_the_same(ctx, monkeypatch):
    rig = "d435_stereo"
    ref = _reference(ctx, rig)
    monkeypatch.setenv("FLVIS_LANES", "2")
    trk = _logged_tracker(ctx, rig)
    assert trk.lib.flvis_tracker_lanes(ctx._h) == 2
    trk.set_input_hold(2)                                                 # (every step has buffers of its own)
    trk.run_steps(ref["steps"], with_local_map=True)
    for s in range(S):
        _check_log(trk, s, KL.record(ref["hist"][s], CAP), what="two lanes")
    del trk


# ---- 6. log off -------------------------------------------------------------------------------------------------------------------
def test_log_on_changes_nothing_and_log_off_refuses(ctx):
    import flvis_amd
    rig = "d435_stereo"
    ref = _reference(ctx, rig)
    n = len(ref["steps"])
    rows = {}
    for on in (False, True):
        trk = _logged_tracker(ctx, rig, cap=CAP if on else None, traj=n)
        trk.run_steps(ref["steps"], with_local_map=False)                 # (no local map: logged as well)
        ctx.synchronize()
        rows[on] = [trk.trajectory(s, 0, n) for s in range(S)]
        if on:
            for s in range(S):
                _check_log(trk, s, KL.record(ref["hist"][s], CAP), what="without the local map")
            trk.keyframe_log_enable(0)                                    # off again: freed
        for call in (lambda: trk.keyframe_log_info(0), lambda: trk.keyframe_log_get(0, 0), lambda: trk.keyframe_log_clear([0]),
                     lambda: trk.keyframe_log_images(0, 0)):
            with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
                call()
        del trk
    for s in range(S):
        # poses, states and keyframe flags of every frame: the same bits with the log on, off, and frame by frame
        assert np.array_equal(rows[True][s].view(np.uint64), rows[False][s].view(np.uint64))
        assert np.array_equal(rows[True][s].view(np.uint64), ref["rows"][s].view(np.uint64))
        assert (rows[True][s][:, 8].astype(np.int64) >> 4).sum() == ref["made"][s]
