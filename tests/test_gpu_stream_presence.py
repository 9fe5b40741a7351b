"""Per-stream frame presence (flvis_image_feed_present, flvis_image_feed_host_present, flvis_run_steps_present): a step advances only
the streams that have a frame in it.  Stream s under any presence schedule must return, bit for bit, what stream s of a tracker with
the same configs, n_streams, seed_base and traj_capacity returns when it is fed only its present frames (the "compacted" run: step j
gives every stream its j-th present frame, its stamp and the IMU samples since its previous present frame).  Runs are built from the
synthetic sequences the way tests/test_gpu_stream_reset.py builds them, on the D435i stereo, EuRoC-like, D435i depth and KITTI-like
rigs; an absent stream's device image slot holds another stream's image, so a read of it would show."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

SEED = 0xF1715
S8 = 8

# rig: (yaml, synth rig, depth range of the depth camera's Z16 image or None, IMU, present frames per stream)
RIGS = {
    "d435_stereo": ("D435I_STEREO_YAML", None, None, True, 110),
    "euroc_like": ("EUROC_LIKE_YAML", "euroc_rig", None, True, 80),
    "d435_depth": ("D435I_DEPTH_YAML", None, 3.3, True, 120),
    "kitti_like": ("KITTI_LIKE_YAML", "kitti_like_rig", None, False, 80),
}


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _cfg(rig):
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_presence_%s.yaml" % rig)
    open(p, "w").write(getattr(synth, RIGS[rig][0]))
    return flvis_amd.load_config(p)


def _frames(S, nframes, traj_ids, rig):
    """per step: (img0 [S,H,W], img1, times [S], IMU samples per stream (list of [n, 7]))"""
    from flvis_amd import synth
    _, rname, depth_range, imu, _ = RIGS[rig]
    trajs = [synth.Trajectory(s) for s in traj_ids]
    rnd = synth.Renderer("cuda", rig=getattr(synth, rname)() if rname else None)
    frames, t_prev = [], -0.05
    for f in range(nframes):
        t = f / synth.FRAME_HZ
        smp = [synth.imu_samples(trajs[i], s, t_prev, t) if imu else np.zeros((0, 7)) for i, s in enumerate(traj_ids)]
        t_prev = t
        if depth_range is None:
            i0, i1 = rnd.stereo_frame(trajs, t, f)
        else:
            i0, i1 = rnd.depth_frame(trajs, t, f, max_range=depth_range)
        frames.append((i0.clone(), i1.clone(), [t] * S, smp))
    return frames


def _imu_block(smp):
    cnt = np.array([len(x) for x in smp], np.int32)
    blk = np.zeros((len(smp), max(int(cnt.max()) if len(cnt) else 0, 1), 7))
    for i, x in enumerate(smp):
        blk[i, :len(x)] = x
    return cnt, blk


def _presence_run(A, pres):
    """The steps of the run with presence pres [T][S]: an absent stream's image slots hold stream (s + 1) % S's images of the step,
    its stamp is NaN; its IMU samples flow up to its last present step (the compacted run integrates nothing after its last frame)"""
    T, S = pres.shape
    last = [int(np.nonzero(pres[:, s])[0][-1]) if pres[:, s].any() else -1 for s in range(S)]
    steps = []
    for k in range(T):
        i0, i1, ts, smp = A[k]
        i0, i1, ts = i0.clone(), i1.clone(), list(ts)
        for s in range(S):
            if not pres[k, s]:
                i0[s], i1[s] = A[k][0][(s + 1) % S], A[k][1][(s + 1) % S]
                ts[s] = float("nan")
        smp = [smp[s] if k <= last[s] else np.zeros((0, 7)) for s in range(S)]
        steps.append((i0, i1, ts, smp))
    return steps


def _compacted(A, pres):
    """step j: every stream's j-th present frame, with the IMU samples of the steps since its previous present frame"""
    T, S = pres.shape
    idx = [np.nonzero(pres[:, s])[0] for s in range(S)]
    N = len(idx[0])
    assert all(len(x) == N for x in idx), "every stream must be present in the same number of steps"
    steps = []
    for j in range(N):
        i0, i1 = A[0][0].clone(), A[0][1].clone()
        ts, smp = [], []
        for s in range(S):
            k = int(idx[s][j])
            k0 = int(idx[s][j - 1]) + 1 if j > 0 else 0
            i0[s], i1[s] = A[k][0][s], A[k][1][s]
            ts.append(A[k][2][s])
            smp.append(np.concatenate([A[q][3][s] for q in range(k0, k + 1)]).reshape(-1, 7))
        steps.append((i0, i1, ts, smp))
    return steps


def _feed(trk, steps, mode, pres=None, every=10, hook=None):
    """Feeds `steps` (with presence rows pres[k], or None: the plain entry points).  Returns the per-step outputs (None for run_steps)."""
    S = trk.S
    if mode == "batches":
        for a in range(0, len(steps), every):
            blk = []
            for i0, i1, ts, smp in steps[a:a + every]:
                cnt, b = _imu_block(smp)
                blk.append((i0, i1, ts, cnt, b))
            trk.run_steps(blk, with_local_map=True, present=None if pres is None else pres[a:a + every])
        return None
    outs, keep = [], []
    for k, (i0, i1, ts, smp) in enumerate(steps):
        if hook:
            hook(trk, k)
        for s in range(S):
            if len(smp[s]):
                trk.imu_feed_flvis(s, smp[s])
        row = None if pres is None else pres[k]
        if mode == "frames":
            outs.append(trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True, present=row))
        else:  # host images, hold_buffers: the arrays stay untouched until the next call has returned; an absent stream's are None
            h0, h1 = i0.cpu().numpy(), i1.cpu().numpy()
            keep = keep[-2:] + [(h0, h1)]
            l0 = [h0[s] if row is None or row[s] else None for s in range(S)]
            l1 = [h1[s] if row is None or row[s] else None for s in range(S)]
            outs.append(trk.image_feed_host(l0, l1, ts, want_out=True, with_local_map=True, hold_buffers=True, present=row))
    return outs


def _stream_result(trk, s, n):
    return dict(rows=trk.trajectory(s, 0, n), lms=trk.landmarks(s), corr=trk.correction(s), kf=trk.keyframe(s),
                kf_imu=trk.get_keyframe_imu(s), kf_imu_pos=trk.get_keyframe_imu_pos(s), recs=trk.pose_records(s), imu=trk.imu_states(s))


def _result(trk, ctx, n, streams=None):
    ctx.synchronize()
    kf, ba = trk.local_map_counts()
    streams = range(trk.S) if streams is None else streams
    return {s: _stream_result(trk, s, n) for s in streams}, kf, ba, trk.counters()[0]


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


def _check_outs(outs, couts, pres, streams):
    """present steps: the compacted run's output of that frame; absent steps: the stream's last output (zero before its first frame)"""
    for s in streams:
        j, last = 0, None
        for k in range(pres.shape[0]):
            if pres[k, s]:
                _same(outs[k][s], couts[j][s], ("present step", k, "stream", s, "frame", j))
                last = outs[k][s]
                j += 1
            elif last is not None:
                _same(outs[k][s], last, ("absent step", k, "stream", s))
            else:
                o = outs[k][s]
                assert o["frame_id"] == 0 and o["state"] == 0 and not o["pose7"].any(), ("absent before the first frame", k, s, o)


def _check_result(res, cres, streams, what):
    (r, kf, ba, n), (cr, ckf, cba, cn) = res, cres
    for s in streams:
        _same(r[s], cr[s], (what, "stream", s))
        assert kf[s] == ckf[s] and ba[s] == cba[s], (what, s, kf[s], ckf[s], ba[s], cba[s])
    assert n == cn, (what, "frames fed", n, cn)


def _first_n(mask, N):
    """the first N True steps of mask (the rest absent)"""
    idx = np.nonzero(mask)[0]
    assert len(idx) >= N, (len(idx), N)
    out = np.zeros(len(mask), bool)
    out[idx[:N]] = True
    return out


def _schedules(T, N, burst_at):
    """[T][8]: every stream present in exactly N steps, each on its own schedule"""
    k = np.arange(T)
    rng = np.random.default_rng(1234)
    sub = np.zeros(T, bool)
    sub[np.sort(rng.choice(T - 30, N, replace=False))] = True
    skip_gaps = np.ones(T, bool)
    skip_gaps[[1, 2, 3] + list(range(10, 20)) + list(range(45, 55))] = False
    cols = [
        k < N,                                                      # every step (while it runs)
        _first_n(k % 2 == 0, N),                                    # every other step
        _first_n(k % 4 != 3, N),                                    # one drop in four
        _first_n((k < burst_at) | (k >= burst_at + 12), N),         # a burst of 12 absent steps while tracking, right after a keyframe
        _first_n(k >= 30, N),                                       # joins after 30 steps (its IMU filter initialises meanwhile)
        sub,                                                        # absent for the last 30 steps
        _first_n(np.random.default_rng(77).random(T) >= 0.3, N),   # 30 % random drops
        _first_n(skip_gaps, N),                                     # absent partly inside the skip_first_n_imgs window
    ]
    return np.stack(cols, 1)


_cache = {}


def _rig_case(ctx, rig):
    """frames A (T = 2 N steps), the presence schedules and the compacted run's outputs and results"""
    if rig in _cache:
        return _cache[rig]
    import flvis_amd
    cfg = _cfg(rig)
    N = RIGS[rig][4]
    T = 2 * N
    A = _frames(S8, T, [3 + 7 * i for i in range(S8)], rig)
    # the burst starts right after a keyframe of stream 3 in the second half of its run, once its window has optimised
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    po = _feed(trk, A[:N], "frames")
    ctx.synchronize()
    kfs = [f for f in range(N // 2, N - 12) if po[f][3]["new_keyframe"]]
    del trk
    burst_at = kfs[0] + 1 if kfs else N // 2
    pres = _schedules(T, N, burst_at)
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    comp = _compacted(A, pres)
    couts = _feed(trk, comp, "frames")
    cres = _result(trk, ctx, T)
    del trk
    assert max(cres[2]) >= 1, ("no window optimises", rig, cres[1], cres[2])
    _cache[rig] = (cfg, A, pres, T, N, couts, cres)
    return _cache[rig]


@pytest.mark.parametrize("rig", list(RIGS))
def test_presence_equals_compacted_run(ctx, rig):
    """8 streams, each present in N of 2 N steps on its own schedule, in the three entry forms (device images, host images with NULL
    for an absent stream, run_steps in batches of 10): every per-stream result, every output at a present step (and the last one
    again at an absent step) and the local-map counts equal the compacted run's, bit for bit."""
    import flvis_amd
    cfg, A, pres, T, N, couts, cres = _rig_case(ctx, rig)
    steps = _presence_run(A, pres)
    for mode in ("frames", "host", "batches"):
        trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
        outs = _feed(trk, steps, mode, pres)
        res = _result(trk, ctx, T)
        assert trk.dropped_keyframes() == 0
        del trk
        _check_result(res, cres, range(S8), (rig, mode))
        if outs is not None:
            _check_outs(outs, couts, pres, range(S8))


def test_all_present_equals_plain_entries(ctx):
    """An all-ones presence array and a NULL one are the plain entry points, bit for bit (device images, host images, run_steps)."""
    import flvis_amd
    rig = "d435_stereo"
    cfg = _cfg(rig)
    M = 70
    A = _frames(S8, M, [5 + 7 * i for i in range(S8)], rig)
    ones = np.ones((M, S8), np.uint8)

    def run(mode, pres, null=False):
        trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=M)
        if null:  # the _present entry with a NULL array
            outs = []
            fn = trk.lib.flvis_image_feed_present
            for i0, i1, ts, smp in A:
                for s in range(S8):
                    if len(smp[s]):
                        trk.imu_feed_flvis(s, smp[s])
                t = np.ascontiguousarray(ts, np.float64)
                trk.ctx._check(fn(trk.ctx._h, i0.data_ptr(), i1.data_ptr(), t.ctypes.data, None, C.cast(trk._out, C.c_void_p), 1), "feed")
                outs.append(trk._frame_outs())
        else:
            outs = _feed(trk, A, mode, pres)
        res = _result(trk, ctx, M)
        del trk
        return outs, res

    for mode in ("frames", "host", "batches"):
        po, pr = run(mode, None)
        qo, qr = run(mode, ones)
        _same(qr[0], pr[0], (mode, "all ones"))
        assert np.array_equal(qr[1], pr[1]) and np.array_equal(qr[2], pr[2]) and qr[3] == pr[3] == M * S8
        _same(qo, po, (mode, "outputs"))
    po, pr = run("frames", None)
    no, nr = run("frames", None, null=True)
    _same(nr[0], pr[0], "NULL")
    _same(no, po, "NULL outputs")


def test_step_with_no_stream_present(ctx):
    """Steps with no stream present: only the IMU-state rows move (outputs, trajectories and counters [0] stay); the frames after them
    equal the compacted run's."""
    import flvis_amd
    rig = "d435_stereo"
    cfg = _cfg(rig)
    T = 90
    A = _frames(S8, T, [6 + 7 * i for i in range(S8)], rig)
    pres = np.ones((T, S8), bool)
    pres[60:63] = False
    pres[T - 3:] = True
    steps = _presence_run(A, pres)
    comp = _compacted(A, pres)
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    couts = _feed(trk, comp, "frames")
    cres = _result(trk, ctx, T)
    del trk
    seen = {}

    def hook(trk, k):
        if k in (60, 63):
            ctx.synchronize()
            seen[k] = (trk.counters()[0], [trk.trajectory(s, 0, T) for s in range(S8)], [trk.imu_states(s) for s in range(S8)])

    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    outs = _feed(trk, steps, "frames", pres, hook=hook)
    res = _result(trk, ctx, T)
    del trk
    assert seen[60][0] == seen[63][0] == 60 * S8
    _same(seen[63][1], seen[60][1], "trajectories over the empty steps")
    for s in range(S8):
        rows, dropped = seen[63][2][s]
        assert len(rows) == sum(len(A[k][3][s]) for k in (60, 61, 62)) > 0 and dropped == 0, s
    for k in (60, 61, 62):
        _same(outs[k], outs[59], ("empty step", k))
    _check_outs(outs, couts, pres, range(S8))
    # (the IMU rows fetched in the hook are the compacted run's too: compare the trajectories and the rest)
    for s in range(S8):
        for key in ("rows", "lms", "corr", "kf", "kf_imu", "kf_imu_pos", "recs"):
            _same(res[0][s][key], cres[0][s][key], ("stream", s, key))
    assert np.array_equal(res[1], cres[1]) and np.array_equal(res[2], cres[2]) and res[3] == cres[3]


def test_presence_with_two_lanes(ctx, monkeypatch):
    """FLVIS_LANES=2 and flvis_set_input_hold(2): lane 1 (streams 4-7) fully absent for 10 steps, random drops elsewhere; equal to the
    compacted run."""
    import flvis_amd
    monkeypatch.setenv("FLVIS_LANES", "2")
    rig = "d435_stereo"
    cfg = _cfg(rig)
    N = 90
    T = 150
    A = _frames(S8, T, [2 + 7 * i for i in range(S8)], rig)
    rng = np.random.default_rng(5)
    k = np.arange(T)
    cols = []
    for s in range(S8):
        m = rng.random(T) >= 0.2
        if s >= 4:
            m &= (k < 40) | (k >= 50)
        cols.append(_first_n(m, N))
    pres = np.stack(cols, 1)
    assert not pres[40:50, 4:].any() and pres[40:50, :4].any()
    comp = _compacted(A, pres)
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    couts = _feed(trk, comp, "frames")
    cres = _result(trk, ctx, T)
    del trk
    steps = _presence_run(A, pres)
    for mode in ("frames", "batches"):
        trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
        trk.set_input_hold(2)
        outs = _feed(trk, steps, mode, pres)
        res = _result(trk, ctx, T)
        del trk
        _check_result(res, cres, range(S8), ("two lanes", mode))
        if outs is not None:
            _check_outs(outs, couts, pres, range(S8))


def test_reset_while_absent(ctx):
    """A stream reset during its absence starts over at its next present frame: from then on it equals a fresh tracker's stream fed
    sequence B from frame 0; the other streams are not disturbed."""
    import flvis_amd
    rig = "d435_stereo"
    cfg = _cfg(rig)
    R, NB = 60, 70
    T = R + 10 + NB
    A = _frames(S8, T, [4 + 7 * i for i in range(S8)], rig)
    B = _frames(S8, NB, [1 + 7 * i for i in range(S8)], rig)
    pres = np.ones((T, S8), bool)
    pres[R:R + 10, 2] = False
    steps = []
    for k in range(T):
        i0, i1, ts, smp = A[k]
        i0, i1, ts, smp = i0.clone(), i1.clone(), list(ts), list(smp)
        if R <= k < R + 10:
            i0[2], i1[2] = A[k][0][3], A[k][1][3]
            if k >= R + 5:
                smp[2] = np.zeros((0, 7))   # (after the reset: the new sequence's samples start with its first frame)
        elif k >= R + 10:
            b = B[k - R - 10]
            i0[2], i1[2] = b[0][2], b[1][2]
            ts[2] = b[2][2]
            smp[2] = b[3][2]
        steps.append((i0, i1, ts, smp))

    def hook(trk, k):
        if k == R + 5:
            trk.reset_streams([2])

    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    outs = _feed(trk, steps, "frames", pres, hook=hook)
    res = _result(trk, ctx, T)
    del trk
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    fo = _feed(trk, B, "frames")
    fr = _result(trk, ctx, T)
    del trk
    trk = flvis_amd.Tracker(ctx, cfg, S8, seed_base=SEED, traj_capacity=T)
    uo = _feed(trk, A, "frames")
    ur = _result(trk, ctx, T)
    del trk
    _same(res[0][2], fr[0][2], "reset stream")
    assert res[1][2] == fr[1][2] and res[2][2] == fr[2][2]
    for g in range(NB):
        _same(outs[R + 10 + g][2], fo[g][2], ("frame", g))
    for k in range(R, R + 5):
        _same(outs[k][2], outs[R - 1][2], ("absent", k))
    for k in range(R + 5, R + 10):  # (reset while absent: the output k_stream_reset leaves, all zero)
        assert outs[k][2]["frame_id"] == 0 and not outs[k][2]["pose7"].any(), ("absent after the reset", k)
    for s in range(S8):
        if s != 2:
            _same(res[0][s], ur[0][s], ("other stream", s))
            assert res[1][s] == ur[1][s] and res[2][s] == ur[2][s]
            for k in range(T):
                _same(outs[k][s], uo[k][s], ("other stream", s, k))


def test_presence_64_streams_with_local_map(ctx):
    """64 streams in two groups of 32 on alternating steps, plus 10 % random drops, local map on, run_steps in batches of 10: no
    keyframe is dropped and the sampled streams equal the compacted run."""
    import flvis_amd
    rig = "d435_stereo"
    cfg = _cfg(rig)
    S, N = 64, 70
    T = 2 * N + 40
    A = _frames(S, T, [s for s in range(S)], rig)
    rng = np.random.default_rng(9)
    k = np.arange(T)
    pres = np.stack([_first_n((k % 2 == (s // 32)) & (rng.random(T) >= 0.1), N) for s in range(S)], 1)
    sample = [0, 17, 31, 32, 50, 63]
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=SEED, traj_capacity=T)
    _feed(trk, _compacted(A, pres), "batches")
    cres = _result(trk, ctx, T, sample)
    del trk
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=SEED, traj_capacity=T)
    _feed(trk, _presence_run(A, pres), "batches", pres)
    res = _result(trk, ctx, T, sample)
    assert trk.dropped_keyframes() == 0
    del trk
    _check_result(res, cres, sample, "64 streams")
    assert sum(res[1]) > 0 and sum(res[2]) > 0, (res[1], res[2])


def test_presence_arguments(ctx):
    """A present stream with NULL host data: FLVIS_ERR_INVALID_ARG, nothing enqueued, and the calls after it are undisturbed."""
    import flvis_amd
    rig = "d435_stereo"
    cfg = _cfg(rig)
    M = 30
    A = _frames(4, M, [8, 15, 22, 29], rig)
    pres = np.ones((M, 4), bool)
    pres[::3, 1] = False

    def run(bad):
        trk = flvis_amd.Tracker(ctx, cfg, 4, seed_base=SEED, traj_capacity=M)

        def hook(trk, k):
            if bad and k in (0, 10):
                h0, h1 = A[k][0].cpu().numpy(), A[k][1].cpu().numpy()
                imgs0 = [h0[0], None, h0[2], h0[3]]
                a = (flvis_amd.FlvisImage * 4)()
                b = (flvis_amd.FlvisImage * 4)()
                for arr, src in ((a, imgs0), (b, list(h1))):
                    for s, im in enumerate(src):
                        if im is not None:
                            arr[s].data = C.cast(im.ctypes.data, C.POINTER(C.c_uint8))
                            arr[s].width, arr[s].height, arr[s].pitch, arr[s].channels = im.shape[1], im.shape[0], im.strides[0], 1
                pr = np.ones(4, np.uint8)
                fn = trk.lib.flvis_image_feed_host_present
                rc = fn(trk.ctx._h, C.cast(a, C.c_void_p), C.cast(b, C.c_void_p), pr.ctypes.data, None, 1, 0)
                assert rc == flvis_amd.FLVIS_ERR_INVALID_ARG, rc
                with pytest.raises(flvis_amd.FlvisError):
                    trk.image_feed_host(imgs0, list(h1), A[k][2], present=pr)
                assert trk.counters()[0] == (4 * k - sum(1 for q in range(k) if not pres[q, 1]))

        outs = _feed(trk, A, "host", pres, hook=hook)
        res = _result(trk, ctx, M)
        del trk
        return outs, res

    po, pr_ = run(False)
    qo, qr = run(True)
    _same(qo, po, "outputs")
    _same(qr[0], pr_[0], "results")
    assert qr[3] == pr_[3] == 4 * M - int((~pres[:, 1]).sum())


@pytest.mark.parametrize("rig", ["d435_stereo", "euroc_like"])
def test_presence_lockstep_with_checker(ctx, rig):
    """The oracle lockstep of test_gpu_pipeline's frontend parity with presence: two streams, the IMU samples fed to both sides at
    every step, the checker handed an image only when the stream is present.  State, keyframe flag, counts, ids, pixels, 3-D points,
    pose, keyframe payloads and IMU rows are identical."""
    import flvis_amd
    from flvis_amd import synth
    cfg = _cfg(rig)
    ocfg = O.RefConfig()
    assert C.sizeof(ocfg) == C.sizeof(cfg)
    C.memmove(C.byref(ocfg), C.byref(cfg), C.sizeof(cfg))
    streams = [3, 140] if rig == "d435_stereo" else [9, 16]
    S = 2
    T = 130 if rig == "d435_stereo" else 90
    rname = RIGS[rig][1]
    trajs = [synth.Trajectory(s) for s in streams]
    rnd = synth.Renderer("cuda", rig=getattr(synth, rname)() if rname else None)
    k = np.arange(T)
    pres = np.stack([k % 3 != 2, ((k < 50) | (k >= 62)) & (np.random.default_rng(3).random(T) >= 0.15)], 1)
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=SEED, traj_capacity=T)
    refs = [O.Tracker(ocfg, SEED + i) for i in range(S)]
    imu_want = [[] for _ in range(S)]
    t_prev = -0.05
    lock = [0, 0]
    n_kf = 0
    for f in range(T):
        t = f / synth.FRAME_HZ
        for i, s in enumerate(streams):
            smp = synth.imu_samples(trajs[i], s, t_prev, t)
            trk.imu_feed_flvis(i, smp)
            for r in smp:
                imu_want[i].append(np.concatenate([[r[0]], refs[i].imu(r[0], r[1:4], r[4:7])]))
        t_prev = t
        i0, i1 = rnd.stereo_frame(trajs, t, f)
        h0, h1 = i0.cpu().numpy(), i1.cpu().numpy()
        outs = trk.image_feed(i0, i1, [t] * S, with_local_map=False, present=pres[f])
        for i in range(S):
            if f % 3 == 2 or f == T - 1:
                rows, dropped = trk.imu_states(i)
                assert dropped == 0 and np.array_equal(rows, np.array(imu_want[i]).reshape(-1, 11)), ("IMU states", f, i)
                imu_want[i] = []
            if not pres[f, i]:
                continue
            want = refs[i].image(t, h0[i], h1[i])
            got = outs[i]
            where = "frame %d stream %d" % (f, i)
            assert got["state"] == want["state"] and got["new_keyframe"] == want["new_keyframe"], where
            assert got["n_landmarks"] == want["n_landmarks"], where
            assert np.array_equal(got["dbg"], want["dbg"]), where
            assert np.array_equal(got["pose7"], want["pose7"]), where
            if want["state"] == 1:
                lock[i] += 1
                gl, wl = trk.landmarks(i), refs[i].landmarks()
                for key in ("ids", "flags", "p2d", "p2u", "p3w"):
                    assert np.array_equal(gl[key], wl[key]), (where, key)
            if want["new_keyframe"]:
                n_kf += 1
                gk, wk = trk.keyframe(i), refs[i].keyframe()
                assert gk["frame_id"] == wk["frame_id"] and np.array_equal(gk["lm_id"], wk["lm_id"]), where
                assert np.array_equal(gk["lm_2d"], wk["lm_2d"]) and np.array_equal(gk["lm_3d"], wk["lm_3d"]), where
                assert np.array_equal(gk["pose7"], wk["pose7"]), where
                assert trk.get_keyframe_imu(i)[0] == refs[i].keyframe_imu()[0], where
                gdp, gva = trk.get_keyframe_imu_pos(i)
                wdp, wva = refs[i].keyframe_imu_pos()
                assert np.array_equal(gdp, wdp) and np.array_equal(gva, wva), where
    assert min(lock) >= 20 and n_kf >= 2, (lock, n_kf)
