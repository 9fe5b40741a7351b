"""Per-stream reset (flvis_reset_streams / flvis_local_map_reset): a stream reset between two frame steps and then fed sequence B
must return, bit for bit, what the same stream of a new tracker returns when fed B from step 0; the other streams must not notice.
Runs are spliced from the synthetic sequences of test_gpu_pipeline.py (_mode_frames) on the D435i stereo, EuRoC-like, D435i depth
and KITTI-like rigs."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0xF1715


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


# rig: (yaml, synth rig, depth range of the depth camera's Z16 image or None, IMU, first step a reset may fall on, steps after it)
# (the D435i rigs track once the IMU filter has initialised, ~45 frames, the depth rig after skip_first_n_imgs = 50 more; EuRoC-like
# and KITTI-like from the first frames)
RIGS = {
    "d435_stereo": ("D435I_STEREO_YAML", None, None, True, 100, 100),
    "euroc_like": ("EUROC_LIKE_YAML", "euroc_rig", None, True, 60, 80),
    "d435_depth": ("D435I_DEPTH_YAML", None, 3.3, True, 110, 100),
    "kitti_like": ("KITTI_LIKE_YAML", "kitti_like_rig", None, False, 40, 80),
}


def _cfg(rig="d435_stereo"):
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_reset_%s.yaml" % rig)
    open(p, "w").write(getattr(synth, RIGS[rig][0]))
    return flvis_amd.load_config(p)


def _frames(S, nframes, traj_ids, rig="d435_stereo"):
    """per step: (img0 [S,H,W], img1, times [S], imu counts [S], imu samples [S, n, 7]) -- as test_gpu_pipeline._mode_frames"""
    from flvis_amd import synth
    _, rname, depth_range, imu, _, _ = RIGS[rig]
    trajs = [synth.Trajectory(s) for s in traj_ids]
    rnd = synth.Renderer("cuda", rig=getattr(synth, rname)() if rname else None)
    frames, t_prev = [], -0.05
    for f in range(nframes):
        t = f / synth.FRAME_HZ
        smp = [synth.imu_samples(trajs[i], s, t_prev, t) if imu else np.zeros((0, 7)) for i, s in enumerate(traj_ids)]
        t_prev = t
        cnt = np.array([len(x) for x in smp], np.int32)
        blk = np.zeros((S, max(max(len(x) for x in smp), 1), 7))
        for i, x in enumerate(smp):
            blk[i, :len(x)] = x
        if depth_range is None:
            i0, i1 = rnd.stereo_frame(trajs, t, f)
        else:  # the second image is the Z16 depth image aligned to cam0; beyond the range: no depth (the rand() dummy depth runs)
            i0, i1 = rnd.depth_frame(trajs, t, f, max_range=depth_range)
        frames.append((i0.clone(), i1.clone(), [t] * S, cnt, blk))
    return frames


def _splice(A, B, R, streams):
    """steps 0 .. R-1: A; steps R ..: A, with the named streams fed B from its frame 0"""
    out = list(A[:R])
    for g in range(len(A) - R):
        a, b = A[R + g], B[g]
        i0, i1 = a[0].clone(), a[1].clone()
        ts, cnt = list(a[2]), a[3].copy()
        n = max(a[4].shape[1], b[4].shape[1])
        blk = np.zeros((len(ts), n, 7))
        blk[:, :a[4].shape[1]] = a[4]
        for k in streams:
            i0[k], i1[k] = b[0][k], b[1][k]
            ts[k], cnt[k] = b[2][k], b[3][k]
            blk[k] = 0
            blk[k, :b[4].shape[1]] = b[4][k]
        out.append((i0, i1, ts, cnt, blk))
    return out


def _feed(trk, steps, mode, resets=(), hook=None):
    """Feeds `steps`; before step f calls trk.reset_streams(lst) for every (f, lst) in resets (and hook(trk, f) if given).
    Returns the per-step frame outputs (frame-by-frame forms) or None (run_steps)."""
    outs = []
    at = {}
    for f, lst in resets:
        at.setdefault(f, []).append(lst)
    if mode == "batches":
        cuts = sorted(set([0, len(steps)] + [f for f, _ in resets]))
        for a, b in zip(cuts[:-1], cuts[1:]):
            for lst in at.get(a, []):
                trk.reset_streams(lst)
            trk.run_steps(steps[a:b], with_local_map=True)
        return None
    keep = []
    for f, (i0, i1, ts, cnt, blk) in enumerate(steps):
        for lst in at.get(f, []):
            trk.reset_streams(lst)
        if hook:
            hook(trk, f)
        for s in range(trk.S):
            if cnt[s]:
                trk.imu_feed_flvis(s, blk[s, :cnt[s]])
        if mode == "frames":
            outs.append(trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True))
        else:  # host images, hold_buffers = 1: the arrays stay untouched until the next call has returned
            h0, h1 = i0.cpu().numpy(), i1.cpu().numpy()
            keep = keep[-2:] + [(h0, h1)]
            outs.append(trk.image_feed_host(list(h0), list(h1), ts, want_out=True, with_local_map=True, hold_buffers=True))
    return outs


def _stream_result(trk, s, n):
    return dict(rows=trk.trajectory(s, 0, n), lms=trk.landmarks(s), corr=trk.correction(s), kf=trk.keyframe(s),
                kf_imu=trk.get_keyframe_imu(s), kf_imu_pos=trk.get_keyframe_imu_pos(s), recs=trk.pose_records(s), imu=trk.imu_states(s))


def _result(trk, ctx, n):
    ctx.synchronize()
    kf, ba = trk.local_map_counts()
    return [_stream_result(trk, s, n) for s in range(trk.S)], kf, ba


def _same(x, y, what):
    if isinstance(x, dict):
        assert isinstance(y, dict) and x.keys() == y.keys(), what
        for k in x:
            _same(x[k], y[k], (what, k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), what
        for i, (a, b) in enumerate(zip(x, y)):
            _same(a, b, (what, i))
    elif isinstance(x, np.ndarray):
        assert isinstance(y, np.ndarray) and x.shape == y.shape and np.array_equal(x, y), what
    else:
        assert x == y, (what, x, y)


def _check(res, outs, fresh, fresh_outs, undist, undist_outs, R, reset):
    (rs, kf, ba), (fs, fkf, fba), (us, ukf, uba) = res, fresh, undist
    for s in range(len(rs)):
        if s in reset:
            _same(rs[s], fs[s], ("reset stream", s))
            assert kf[s] == fkf[s] and ba[s] == fba[s], (s, kf[s], fkf[s], ba[s], fba[s])
            if outs is not None:
                for g in range(len(fresh_outs)):
                    _same(outs[R + g][s], fresh_outs[g][s], ("frame", R + g, s))
        else:
            _same(rs[s], us[s], ("other stream", s))
            assert kf[s] == ukf[s] and ba[s] == uba[s], s
            if outs is not None:
                for f in range(len(undist_outs)):
                    _same(outs[f][s], undist_outs[f][s], ("frame", f, s))


S8 = 8
_cache = {}


def _scenario(ctx, rig="d435_stereo"):
    """A (steps 0 .. R + N - 1) and B (N steps) for 8 streams; R = the step right after stream 2 made a keyframe once its window
    has optimised (an optimisation of the old sequence is queued or running at the reset); the fresh and undisturbed runs"""
    if rig in _cache:
        return _cache[rig]
    import flvis_amd
    cfg = _cfg(rig)
    r_min, N = RIGS[rig][4], RIGS[rig][5]
    total = r_min + 40 + N
    A = _frames(S8, total, [3 + 7 * i for i in range(S8)], rig)
    B = _frames(S8, N, [4 + 7 * i for i in range(S8)], rig)
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=total)
    uo = _feed(trk, A, "frames")
    del trk
    kfs = [f for f in range(r_min, total - N + 1) if uo[f - 1][2]["new_keyframe"]]
    assert kfs, "stream 2 makes no keyframe between steps %d and %d" % (r_min, total - N)
    R = kfs[0]
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=total)
    trk.run_steps(A[:R - 1], with_local_map=True)
    ctx.synchronize()
    assert trk.local_map_counts()[1][2] >= 1, "stream 2's old window optimises before the reset"
    del trk
    A = A[:R + N]
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=R + N)
    uo = _feed(trk, A, "frames")
    und = _result(trk, ctx, R + N)
    del trk
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=R + N)
    fo = _feed(trk, B, "frames")
    fr = _result(trk, ctx, R + N)
    del trk
    assert fr[2][2] >= 2 and fr[2][5] >= 2, ("the new windows must optimise at least twice", R, fr[1], fr[2], und[1], und[2])
    _cache[rig] = (cfg, A, B, R, N, uo, und, fo, fr)
    return _cache[rig]


@pytest.mark.parametrize("rig,mode", [("d435_stereo", "frames"), ("d435_stereo", "batches"), ("d435_stereo", "host"),
                                      ("euroc_like", "frames"), ("d435_depth", "frames"), ("kitti_like", "frames")])
def test_reset_equals_fresh(ctx, rig, mode):
    """8 streams, local map on: streams 2 and 5 reset at step R and fed B; every per-stream output of the two equals a new tracker's
    fed B, the other six equal the undisturbed run.  On the four rigs frame by frame (EuRoC-like: equalizeHist, distortion; depth
    camera: the rand() dummy depth, skip_first_n_imgs starting over per stream; KITTI-like: no IMU, unaligned rows); on the D435i stereo
    rig also through run_steps batches with the reset between two of them (a deferred local-map launch never outlives a run_steps call:
    its last step launches at once) and through host images with hold_buffers = 1."""
    import flvis_amd
    cfg, A, B, R, N, uo, und, fo, fr = _scenario(ctx, rig)
    reset = [2, 5]
    steps = _splice(A, B, R, reset)
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=R + N)
    outs = _feed(trk, steps, mode, resets=[(R, reset)])
    res = _result(trk, ctx, R + N)
    assert trk.dropped_keyframes() == 0
    _check(res, outs, fr, fo, und, uo, R, reset)


def test_reset_equals_fresh_with_two_lanes(ctx, monkeypatch):
    """FLVIS_LANES=2: one reset stream in each lane (lane-local index and lane mapping)"""
    import flvis_amd
    monkeypatch.setenv("FLVIS_LANES", "2")
    cfg, A, B, R, N, uo, und, fo, fr = _scenario(ctx)
    reset = [2, 5]
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=R + N)
    outs = _feed(trk, _splice(A, B, R, reset), "frames", resets=[(R, reset)])
    _check(_result(trk, ctx, R + N), outs, fr, fo, und, uo, R, reset)


def test_reset_discards_leftovers_and_repeats(ctx):
    """Before the reset stream 2 gets IMU samples that are never integrated, a correction_feed it never applies and IMU-state rows nobody
    fetches; the reset is requested twice, with a duplicate index, and a local-map reset of the same stream follows it: the result is
    one reset (fresh equivalence, imu_states as the new tracker's)."""
    import flvis_amd
    cfg, A, B, R, N, uo, und, fo, fr = _scenario(ctx)
    reset = [2]
    steps = _splice(A, B, R, reset)
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=R + N)

    outs = []
    for f, (i0, i1, ts, cnt, blk) in enumerate(steps):
        if f == R:
            trk.imu_feed_flvis(2, np.array(steps[R - 1][4][2, :cnt[2]]))  # staged, never integrated
            trk.correction_feed(2, 5, np.array([0.1, 0, 0, 0, 0, 0, 1.0]), np.array([100, 101], np.int64), np.ones((2, 3)),
                                np.array([102], np.int64))  # handed over, never applied
            trk.reset_streams([2, 2])
            trk.reset_streams([2])
            trk.local_map_reset([2])
            kf, kimu, kpos = trk.keyframe(2), trk.get_keyframe_imu(2), trk.get_keyframe_imu_pos(2)
            assert len(kf["lm_id"]) == 0 and not kimu[0] and not kpos[0].any() and not kpos[1].any(), "as a new stream's: none"
        for s in range(S8):
            trk.imu_feed_flvis(s, blk[s, :cnt[s]])
        outs.append(trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True))
    res = _result(trk, ctx, R + N)
    assert trk.dropped_keyframes() == 0
    for s in range(S8):
        if s in reset:
            _same(res[0][s], fr[0][s], ("reset stream", s))
            assert res[1][s] == fr[1][s] and res[2][s] == fr[2][s]
            for g in range(N):
                _same(outs[R + g][s], fo[g][s], ("frame", R + g, s))
        else:  # (the correction feeding switches k_apply_correction on for every frame: the same results)
            _same(res[0][s], und[0][s], ("other stream", s))


def test_reset_arguments(ctx):
    """an index of -1 or S: FlvisError, nothing changes (the run stays bit-identical to the undisturbed one); n == 0: no-op"""
    import flvis_amd
    cfg, A, B, R, N, uo, und, fo, fr = _scenario(ctx)
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=R + N)

    def hook(t, f):
        if f == R:
            for bad in ([-1], [S8], [1, S8]):
                with pytest.raises(flvis_amd.FlvisError):
                    t.reset_streams(bad)
                with pytest.raises(flvis_amd.FlvisError):
                    t.local_map_reset(bad)
            t.reset_streams([])
            t.local_map_reset([])

    outs = _feed(trk, A, "frames", hook=hook)
    res = _result(trk, ctx, R + N)
    _check(res, outs, fr, fo, und, uo, R, [])


def test_reset_needs_a_tracker(ctx):
    lib = ctx._lib
    import flvis_amd
    c = flvis_amd.Context(0)
    one = (C.c_int * 1)(0)
    try:
        assert lib.flvis_reset_streams(c._h, 1, one) != 0
        assert lib.flvis_local_map_reset(c._h, 1, one) != 0
    finally:
        c.close()


def _push_seq(trk, s, kfs):
    got = []
    for k in kfs:
        got.append(trk.ba_push_keyframe(s, k["frame_id"], k["pose7"], k["lm_id"], k["lm_2d"], k["lm_3d"]))
    return got


def test_local_map_reset_equals_fresh_window(ctx):
    """flvis_local_map_reset through flvis_ba_push_keyframe: keyframes of sequence A, the reset, then K1 .. Kn give the corrections
    and per-stream counts of a new tracker pushed K1 .. Kn alone; the tracker is not touched"""
    import flvis_amd
    import _ba_synth as BS
    cfg = _cfg()
    seq_a = BS.make_sequence(3, n_kf=14, n_lm=260, outlier_frac=0.03)
    seq_b = BS.make_sequence(11, n_kf=14, n_lm=260, outlier_frac=0.03)
    trk = flvis_amd.Tracker(ctx, cfg, 2)
    _push_seq(trk, 1, seq_a["kfs"])
    trk.local_map_reset([1])
    got = _push_seq(trk, 1, seq_b["kfs"])
    kf, ba = trk.local_map_counts()
    ref = flvis_amd.Tracker(ctx, cfg, 2)
    want = _push_seq(ref, 1, seq_b["kfs"])
    rkf, rba = ref.local_map_counts()
    _same(got, want, "corrections")
    assert kf[1] == rkf[1] and ba[1] == rba[1] and ba[1] >= 1


def test_local_map_reset_processes_what_is_queued(ctx, monkeypatch):
    """a local-map reset right behind a keyframe that is still queued: the keyframe is optimised first (the context's BA-run counter,
    cumulative, counts it), then the window empties -- the stream's counts start from 0 and its correction is withdrawn; its tracker and
    its last keyframe (flvis_get_keyframe, _imu, _imu_pos) are those of the undisturbed run.  Deterministic: with FLVIS_BA_EVERY=2 the
    local map is launched behind even frames only; the queues are drained (synchronize) before an odd frame K at which stream 2 makes a
    keyframe, so that keyframe waits in the queue, with no local-map workgroup running, when the reset is appended behind it."""
    import flvis_amd
    cfg, A, B, R, N, uo, und, fo, fr = _scenario(ctx)
    K = next(f for f in range(R, len(A)) if f % 2 == 1 and uo[f][2]["new_keyframe"])
    monkeypatch.setenv("FLVIS_BA_EVERY", "2")
    runs = {}
    for name in ("reset", "ref"):
        trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=K + 1)
        _feed(trk, A[:K], "frames")
        ctx.synchronize()
        before = trk.local_map_counts()[1][2]
        _feed(trk, A[K:K + 1], "frames")
        if name == "reset":
            trk.local_map_reset([2])
        ctx.synchronize()
        kf, ba = trk.local_map_counts()
        runs[name] = dict(before=before, kf=kf, ba=ba, n=trk.counters(), corr=trk.correction(2),
                          res=[_stream_result(trk, s, K + 1) for s in range(S8)])
        del trk
    r, ref = runs["reset"], runs["ref"]
    assert ref["ba"][2] == ref["before"] + 1, "frame K's keyframe makes stream 2's window optimise"
    assert r["n"][2] == ref["n"][2], (r["n"], ref["n"])      # ... also when the reset follows it in the queue
    assert r["kf"][2] == 0 and r["ba"][2] == 0 and r["corr"] is None and ref["corr"] is not None
    for s in range(S8):
        if s != 2:
            assert r["kf"][s] == ref["kf"][s] and r["ba"][s] == ref["ba"][s]
            _same(r["res"][s], ref["res"][s], s)
        else:
            for k in ("rows", "lms", "kf", "kf_imu", "kf_imu_pos", "recs", "imu"):
                _same(r["res"][s][k], ref["res"][s][k], (s, k))
    assert len(ref["res"][2]["kf"]["lm_id"]) > 0


def test_reset_out_of_tracking_fail(ctx):
    """A stream driven into TrackingFail (state 2) by the feature-starvation scene of test_frontend_parity_when_the_features_run_out
    (KITTI-like rig: all but three textured patches vanish), reset there and fed the full scene, returns what a new tracker's stream
    returns for that scene; stream 1 sees the full scene throughout and does not notice."""
    import flvis_amd
    import torch
    from test_gpu_pipeline import _patch_frame, _patch_scene
    cfg = _cfg("kitti_like")
    xs, ys, Z, tex = _patch_scene(40)
    full = np.ones(40, bool)
    starve = full.copy()
    starve[3:] = False
    nA, nB = 12, 8

    def frame(keep0, f0, f1):
        L0, R0 = _patch_frame(xs, ys, Z, tex, keep0, 1.0 * f0)
        L1, R1 = _patch_frame(xs, ys, Z, tex, full, 1.0 * f1)
        return (torch.from_numpy(np.stack([L0, L1])).cuda(), torch.from_numpy(np.stack([R0, R1])).cuda(), [0.1 * f0, 0.1 * f1],
                np.zeros(2, np.int32), np.zeros((2, 1, 7)))

    A = [frame(full if f < 3 else starve, f, f) for f in range(nA)]
    trk = flvis_amd.Tracker(ctx, cfg, 2, seed_base=SEED, traj_capacity=nA + nB)
    uo = _feed(trk, A, "frames")
    del trk
    fail = [f for f in range(nA) if uo[f][0]["state"] == 2]
    assert fail, [o[0]["state"] for o in uo]
    R = fail[0] + 1
    steps = A[:R] + [frame(full, g, R + g) for g in range(nB)]
    und_steps = A[:R] + [frame(starve, R + g, R + g) for g in range(nB)]
    fresh_steps = [frame(full, g, g) for g in range(nB)]
    runs = {}
    for name, st, resets in (("reset", steps, [(R, [0])]), ("und", und_steps, []), ("fresh", fresh_steps, [])):
        trk = flvis_amd.Tracker(ctx, cfg, 2, seed_base=SEED, traj_capacity=nA + nB)
        runs[name] = (_feed(trk, st, "frames", resets=resets), _result(trk, ctx, nA + nB))
        del trk
    outs, res = runs["reset"]
    _check(res, outs, runs["fresh"][1], runs["fresh"][0], runs["und"][1], runs["und"][0], R, [0])
    assert any(o[0]["state"] == 1 for o in outs[R:]), "the reset stream tracks the full scene"


def test_reset_sixteen_of_sixty_four_streams(ctx):
    """64 streams, host images, local map on: 16 of them reset at one step and fed B; each equals the same stream of one new tracker
    fed B, the other 48 the undisturbed run; no keyframe met a full queue"""
    import flvis_amd
    cfg = _cfg()
    S, R, N = 64, 60, 60
    A = _frames(S, R + N, list(range(S)))
    B = _frames(S, N, [100 + s for s in range(S)])
    reset = list(range(0, S, 4))
    runs = {}
    for name, st, resets, n in (("und", A, [], R + N), ("fresh", B, [], R + N), ("reset", _splice(A, B, R, reset), [(R, reset)], R + N)):
        trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=SEED, traj_capacity=n)
        runs[name] = (_feed(trk, st, "host", resets=resets), _result(trk, ctx, n), trk.dropped_keyframes())
        del trk
    outs, res, dropped = runs["reset"]
    assert dropped == 0
    _check(res, outs, runs["fresh"][1], runs["fresh"][0], runs["und"][1], runs["und"][0], R, reset)
