"""GPU: the loop closer's stamps and whole trajectories in the map frame (flvis_loop_closer_set_keyframe_stamps / _keyframe_stamps /
_map_poses / _map_poses_host / _map_trajectory, include/flvis_hip.h).  The three routes to the kernels -- the closer on device rows, on
host rows, and the kernel-level call on poses() and the odometry poses handed in -- must agree BIT FOR BIT with the numpy restatement
(tests/_lc_traj.py) and leave the closer as a twin that never made the calls."""
import ctypes as C

import numpy as np
import pytest

import _geom as G
import _lc_traj as T
import _loop_chain as LC
import _loop_localize as LL
import _pgo_synth as PS
import _voc as V
import test_gpu_loop_localize as TL
from test_gpu_kf_log import CAP, IDS
from test_gpu_stream_reset import _cfg, _frames

pytestmark = pytest.mark.gpu
INV, CFG_ERR = -1, -5
KINDS = (T.POSE8, T.TRAJ9, T.IMU11)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _agree(ctx, lc, odom, rng, rows_per_job=70):
    """rows of every kind on every sequence, both modes: closer (device rows) == closer (host rows) == kernel-level call on poses() and
    the odometry poses handed in == restatement; the closer's state is not touched.  -> the anchors of the TRAJ9 jobs"""
    import torch
    S = lc.n_streams
    before = TL._state(lc, S, keyframes=False)
    M = [lc.poses(s) for s in range(S)]
    tau = [lc.keyframe_stamps(s) for s in range(S)]
    O = [np.asarray(odom[s], np.float64).reshape(-1, 7) for s in range(S)]
    drift = np.stack([lc.drift(s) for s in range(S)])
    assert all(len(M[s]) == len(tau[s]) == len(O[s]) for s in range(S))
    stride = max(len(t) for t in tau) + 1
    tab = [np.zeros((S, stride, 7)), np.zeros((S, stride, 7)), np.full((S, stride), np.nan)]
    for s in range(S):
        tab[0][s, :len(O[s])], tab[1][s, :len(O[s])], tab[2][s, :len(O[s])] = O[s], M[s], tau[s]
    jobs = [(s, kind, T.rows_of(rng, kind, T.row_stamps(rng, tau[s], rows_per_job, sort=(s + kind) % 2 == 0), 3.0))
            for s in range(S) for kind in KINDS]
    anchors = None
    for mode in (T.ANCHOR, T.BLEND):
        want = [T.map_rows(kind, rows, O[s], M[s], tau[s], mode, drift[s]) for s, kind, rows in jobs]
        on_dev = lc.map_poses([(s, kind, dev(rows)) for s, kind, rows in jobs], mode)
        on_host = lc.map_poses(jobs, mode, host=True)
        kernel = ctx.lc_map_poses(dev(tab[0]), dev(tab[1]), dev(tab[2]), [len(t) for t in tau],
                                  [dict(seq=s, kind=kind, rows=dev(rows)) for s, kind, rows in jobs], mode, drift)
        for k, (w_out, w_anc) in enumerate(want):
            for name, (out, anc) in (("device", on_dev[k]), ("host", on_host[k]), ("kernel", kernel[k])):
                out, anc = (out.cpu().numpy(), anc.cpu().numpy()) if isinstance(out, torch.Tensor) else (out, anc)
                assert T.same_bits(out, w_out) and np.array_equal(anc, w_anc), (name, jobs[k][:2], mode)
        anchors = [w[1] for w, j in zip(want, jobs) if j[1] == T.TRAJ9]
    TL._same_state(before, TL._state(lc, S, keyframes=False))
    return anchors


@pytest.fixture(scope="module")
def world():
    w = TL.World()
    yield w
    w.ctx.close()


def test_stamps(world):
    """three sequences of 6, 4 and 0 blank keyframes: stamps set in pieces, read back, refused where they would not increase"""
    import flvis_amd
    w = world
    lc = w.closer(3, 6)
    for i in range(6):
        streams = [0, 1] if i < 4 else [0]
        blank = w.blank.expand(len(streams), -1, -1).contiguous()
        lc.add_keyframes(streams, blank, blank, [LL.IDENT] * len(streams))
    assert all(np.isnan(lc.keyframe_stamps(s)).all() for s in range(3))
    assert [len(lc.keyframe_stamps(s)) for s in range(3)] == [6, 4, 0]
    t = T.EUROC_T0 + 0.05 * np.arange(6)
    lc.set_keyframe_stamps(0, 0, t[:2])
    lc.set_keyframe_stamps(0, 4, t[4:])
    got = lc.keyframe_stamps(0)
    assert T.same_bits(got[[0, 1, 4, 5]], t[[0, 1, 4, 5]]) and np.isnan(got[2:4]).all()
    for first, bad in ((2, [t[1], t[3]]), (2, [t[2], t[4]]), (2, [t[3], t[2]]), (2, [t[2], np.nan]), (2, [np.inf, t[3]]), (0, [t[1], t[1]]),
                       (5, [t[4]]), (5, [t[5], t[5] + 1]), (-1, [t[0]]), (6, [t[5] + 1])):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            lc.set_keyframe_stamps(0, first, bad)
        assert T.same_bits(lc.keyframe_stamps(0)[[0, 1, 4, 5]], t[[0, 1, 4, 5]]) and np.isnan(lc.keyframe_stamps(0)[2:4]).all()
    for stream in (-1, 3):
        with pytest.raises(flvis_amd.FlvisError):
            lc.set_keyframe_stamps(stream, 0, [1.0])
    lc.set_keyframe_stamps(0, 2, t[2:4])
    lc.set_keyframe_stamps(0, 1, [t[1] + 0.01])                          # a set stamp may be moved while the order holds
    t[1] += 0.01
    lc.set_keyframe_stamps(1, 0, t[:4] - 7.0)
    lc.set_keyframe_stamps(2, 0, [])
    assert T.same_bits(lc.keyframe_stamps(0), t) and T.same_bits(lc.keyframe_stamps(1), t[:4] - 7.0) and len(lc.keyframe_stamps(2)) == 0
    # a sequence with every stamp set maps; reset forgets the stamps, and the slot's next keyframe has none
    rng = np.random.default_rng(0)
    _agree(w.ctx, lc, [[LL.IDENT] * 6, [LL.IDENT] * 4, []], rng)
    lc.reset([0])
    assert len(lc.keyframe_stamps(0)) == 0 and T.same_bits(lc.keyframe_stamps(1), t[:4] - 7.0)
    lc.add_keyframes([0], w.blank, w.blank, [LL.IDENT])
    assert np.isnan(lc.keyframe_stamps(0)).tolist() == [True]
    lc.close()


def test_unstamped_keyframes_refuse_the_job_and_nothing_is_written(world):
    import flvis_amd
    import torch
    w = world
    lc = w.closer(2, 4)
    for i in range(3):
        blank = w.blank.expand(2, -1, -1).contiguous()
        lc.add_keyframes([0, 1], blank, blank, [LL.IDENT] * 2)
    lc.set_keyframe_stamps(0, 0, [1.0, 2.0, 3.0])
    lc.set_keyframe_stamps(1, 0, [1.0])
    lc.set_keyframe_stamps(1, 2, [3.0])                                  # keyframe 1 of sequence 1 stays unstamped
    before = TL._state(lc, 2)
    rows = dev(T.rows_of(np.random.default_rng(1), T.TRAJ9, np.linspace(0, 4, 50)))
    out = torch.full_like(rows, 777.25)
    fn = w.ctx._lib.flvis_loop_closer_map_poses
    arr = (flvis_amd.FlvisLcTrajJob * 2)(flvis_amd.FlvisLcTrajJob(0, T.TRAJ9, 50, rows.data_ptr(), out.data_ptr(), None),
                                         flvis_amd.FlvisLcTrajJob(1, T.TRAJ9, 50, rows.data_ptr(), out.data_ptr(), None))
    assert fn(lc._h, 2, arr, T.ANCHOR) == INV
    msg = w.ctx._lib.flvis_last_error(w.ctx._h).decode()
    assert "sequence 1" in msg and "keyframe 1" in msg, msg
    assert bool((out == 777.25).all())
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        lc.map_poses([(1, T.POSE8, np.zeros((1, 8)))], host=True)
    for bad_mode in (-1, 2):
        assert fn(lc._h, 1, arr, bad_mode) == INV and bool((out == 777.25).all())
    assert fn(lc._h, 1, arr, T.BLEND) == 0 and not bool((out == 777.25).any())       # sequence 0 alone is fine
    TL._same_state(before, TL._state(lc, 2))
    # no tracker on this context: map_trajectory has nothing to read
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        lc.map_trajectory([0], 0, 1)
    lc.close()


def test_before_and_after_a_pose_graph_set_drift_and_merge():
    """The two-trajectory run of tests/test_gpu_loop_closer.py (62 keyframes, the same parameters: both sequences accept loops and run
    pose graphs); a third sequence stays empty until set_drift.  The agreement is checked with a keyframe pending, right after the first
    pose graph, at the end, after set_drift and after merge."""
    import os
    import tempfile
    import torch
    import flvis_amd
    from flvis_amd import synth
    ctx = flvis_amd.Context(0)
    p = os.path.join(tempfile.gettempdir(), "flvis_lc_traj_gpu.yaml")
    open(p, "w").write(synth.D435I_STEREO_YAML)
    cfg = flvis_amd.load_config(p)
    trs = [LC.LoopTrajectory(phase=0.0), LC.LoopTrajectory(phase=0.9)]
    rnd = synth.Renderer("cuda")
    n_kf, per = 62, 50
    times = LC.keyframe_times(n_kf, per)
    frames = [rnd.stereo_frame(trs, t, i) for i, t in enumerate(times)]
    gt = [[G.pose7(*tr.T_c_w(t, rnd.rig)) for t in times] for tr in trs]
    odom = [LC.drifted_odometry(gt[s], 10 + s, sigma_t=0.008, sigma_r=0.002) for s in range(2)]
    train = []
    for i in range(0, n_kf, 6):
        _, d, c, _ = ctx.orb_detect_and_compute(frames[i][0][0:1], cap=1024)
        train.append(d[0, :int(c[0])].cpu().numpy())
    ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))
    lc = flvis_amd.LoopCloser(ctx, cfg, LC.LC_PARAMS, n_streams=3, max_keyframes=64)
    rng = np.random.default_rng(62)
    given = [[], [], []]                                                 # the odometry poses handed in, per sequence
    graphs = 0
    for i in range(n_kf):
        streams = [0] if i % 9 == 4 else [0, 1]
        sel = torch.tensor(streams, device="cuda")
        ids = lc.add_keyframes(streams, frames[i][0][sel].contiguous(), frames[i][1][sel].contiguous(), np.array([odom[s][i] for s in streams]))
        for s, k in zip(streams, ids):
            given[s].append(odom[s][i])
            lc.set_keyframe_stamps(s, int(k), [T.EUROC_T0 + times[i]])
        if i in (3, 55):
            _agree(ctx, lc, given, rng)                                  # the new keyframes are pending: they count, and stay pending
        ev = lc.process()
        assert [e["kf_curr"] >= 0 for e in ev] == [s in streams for s in range(3)]
        ran = sum(e["optimised"] for e in ev)
        if ran and not graphs:
            assert not np.array_equal(lc.drift(0), LL.IDENT) or not np.array_equal(lc.drift(1), LL.IDENT)
            _agree(ctx, lc, given, rng)                                  # right after the first pose graph
        graphs += ran
    assert graphs >= 1 and [len(g) for g in given] == [62, 55, 0]
    anchors = _agree(ctx, lc, given, rng, rows_per_job=300)
    assert len(np.unique(anchors[0])) > 40                               # the rows do spread over the sequence's keyframes
    # the keyframes' own drifts differ after a pose graph: ONE drift per sequence is not the answer for old rows
    D = T.drift_table(np.array(given[0]), lc.poses(0))
    assert np.abs(D[:, :3] - D[-1, :3]).max() > 1e-3
    # set_drift on the empty sequence: its rows take X; a keyframe added afterwards carries X as its own drift
    X = np.array([0.3, -0.2, 0.1, 0.02, -0.05, 0.1, 1.0])
    lc.set_drift(2, X)
    _agree(ctx, lc, given, rng)
    lc.add_keyframes([2], frames[0][0][0:1].contiguous(), frames[0][1][0:1].contiguous(), [odom[0][0]])
    given[2].append(odom[0][0])
    lc.set_keyframe_stamps(2, 0, [T.EUROC_T0 + times[0]])
    _agree(ctx, lc, given, rng)
    D2 = T.drift_table(np.array(given[2]), lc.poses(2))
    assert np.abs(D2[0] - lc.drift(2)).max() < 1e-12
    # merge: the pose database is rewritten for both sequences, the rows follow it
    old = [lc.poses(0), lc.poses(1)]
    gt1 = [gt[1][i] for i in range(n_kf) if i % 9 != 4]
    links = [dict(seq_from=0, kf_from=a, seq_to=1, kf_to=b, pose=PS.loop_pose(dict(gt=[gt[0][a], gt1[b]]), 0, 1, loop_noise=PS.LOOP_NOISE, rng=rng))
             for a, b in ((6, 3), (30, 28), (55, 50))]
    out, _ = lc.merge([[0, 1]], links)
    assert out[0]["optimised"] and not np.array_equal(lc.poses(1), old[1])
    _agree(ctx, lc, given, rng, rows_per_job=300)
    lc.close()
    ctx.close()


def test_the_tracker_path():
    """a two-stream run_steps batch with the keyframe log on (the rig and image size of tests/test_gpu_kf_log_closer.py): add_logged
    brings the stamps, and map_trajectory is map_poses_host on flvis_get_trajectory's rows without the trip through the host"""
    import torch
    import flvis_amd
    rig, S, n = "euroc_like", 2, 24
    ctx = flvis_amd.Context(0)
    steps = _frames(S, n, IDS[:S], rig)
    trk = flvis_amd.Tracker(ctx, _cfg(rig), S, seed_base=1, traj_capacity=n)
    trk.keyframe_log_enable(CAP)
    trk.run_steps(steps, with_local_map=True)
    logged = [trk.keyframe_log_info(s)["logged"] for s in range(S)]
    assert min(logged) >= 4, logged
    msgs = [[trk.keyframe_log_get(s, i) for i in range(logged[s])] for s in range(S)]
    train = []
    for m in msgs[0][::3]:
        _, d, c, _ = ctx.orb_detect_and_compute(torch.from_numpy(m["img0"][None]).cuda(), cap=1024)
        train.append(d[0, :int(c[0])].cpu().numpy())
    ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))
    prm = dict(lcKFStart=25, lcKFDist=18, lcKFMaxDist=50, lcKFLast=20, lcNKFClosest=2, ratioMax=0.5, ratioRansac=0.5, minPts=20, minScore=0.12)
    lc = flvis_amd.LoopCloser(ctx, _cfg(rig), prm, n_streams=S, max_keyframes=CAP)
    lc.set_stereo_unrect(True)
    lc.set_drift(1, [0.5, 0.1, -0.2, 0.0, 0.0, 0.1, 1.0])               # (nothing closes in 24 frames: sequence 1 gets a drift to show)
    lc.add_logged(process=True)
    for s in range(S):
        assert T.same_bits(lc.keyframe_stamps(s), np.array([m["stamp"] for m in msgs[s]]))
    rows = [trk.trajectory(s, 0, n) for s in range(S)]
    state = TL._state(lc, S, keyframes=False)
    for mode in (T.ANCHOR, T.BLEND):
        for streams, first, cnt in (([1, 0], 0, n), ([0], 5, 7), ([1], n - 1, 1), ([0, 1], 3, 0)):
            want = lc.map_poses([(s, T.TRAJ9, rows[s][first:first + cnt]) for s in streams], mode, host=True)
            got, anc = lc.map_trajectory(streams, first, cnt, mode)
            on_dev, anc2 = lc.map_trajectory(streams, first, cnt, mode, device=True)
            assert got.shape == (len(streams), cnt, 9) and anc.shape == (len(streams), cnt)
            for k in range(len(streams)):
                assert T.same_bits(got[k], want[k][0]) and np.array_equal(anc[k], want[k][1]), (mode, streams, k)
            assert T.same_bits(on_dev.cpu().numpy(), got) and np.array_equal(anc, anc2)
    full, anc = lc.map_trajectory([0, 1], 0, n, T.ANCHOR)
    assert anc[0].max() == logged[0] - 1 and anc.min() == 0
    assert np.abs(full[0] - rows[0]).max() < 1e-12 * (1 + np.abs(rows[0][:, 1:4]).max())        # sequence 0 never drifted: its rows stay
    assert np.abs(full[1, :, 1:4] - rows[1][:, 1:4]).max() > 0.1                                  # sequence 1's rows moved by its drift
    for s in range(S):
        assert T.same_bits(trk.trajectory(s, 0, n), rows[s])             # the record itself is unchanged
    TL._same_state(state, TL._state(lc, S, keyframes=False))
    # refusals: a range outside the record, a stream out of range, a closer of another stream count
    for streams, first, cnt in (([0], 0, n + 1), ([0], -1, 2), ([0], 2, -1), ([2], 0, 1), ([], 0, 1)):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            lc.map_trajectory(streams, first, cnt)
    other = flvis_amd.LoopCloser(ctx, _cfg(rig), prm, n_streams=S + 1, max_keyframes=4)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        other.map_trajectory([0], 0, 1)
    other.close()
    lc.close()
    del trk
    ctx.close()
