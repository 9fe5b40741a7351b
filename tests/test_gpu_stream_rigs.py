"""Per-stream calibration (flvis_tracker_create_rigs / flvis_reset_streams_rigs / flvis_get_stream_cfg): a batch whose streams run on
different units of one camera model (synth.rig_variant), each stream rendered with its own rig.  Every stream must equal, bit for bit,
the same stream of a uniform tracker built with that stream's config; every stream must stay in lockstep with the oracle's tracker
loaded from its own yaml; the local map must optimise every window with its stream's K and T_imu_cam0; a stream reset onto another
rig must equal a fresh stream on that rig; and a config that disagrees on a batch-wide field must be refused."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import _ba_synth as B
import _oracle as O
from test_gpu_stream_reset import RIGS, _feed, _result, _same, _splice

pytestmark = pytest.mark.gpu

SEED = 0xF1715
S8 = 8
VARIANTS = [0, 1, 2, 3, 0, 1, 2, 3]  # 8 streams on 4 rigs
# synth.rig_variant's kinds -> the rig table of test_gpu_stream_reset (depth range, IMU, first tracked step)
KINDS = {"d435i_stereo": "d435_stereo", "euroc_like": "euroc_like", "d435i_depth": "d435_depth", "kitti_like": "kitti_like"}


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _yaml_path(kind, k):
    from flvis_amd import synth
    _, text = synth.rig_variant(kind, k)
    p = os.path.join(tempfile.gettempdir(), "flvis_rigs_%s_%d.yaml" % (kind, k))
    open(p, "w").write(text)
    return p


def _cfg(kind, k):
    import flvis_amd
    return flvis_amd.load_config(_yaml_path(kind, k))


def _frames(kind, variants, traj_ids, nframes):
    """per step: (img0 [S,H,W], img1, times [S], imu counts [S], imu samples [S, n, 7]); stream i rendered with rig_variant(kind,
    variants[i]) -- as test_gpu_stream_reset._frames, one renderer per rig"""
    import torch
    from flvis_amd import synth
    _, depth_range, imu, _, _ = RIGS[KINDS[kind]][1:]
    S = len(variants)
    trajs = [synth.Trajectory(s) for s in traj_ids]
    groups = {}
    for i, v in enumerate(variants):
        groups.setdefault(v, []).append(i)
    rnds = {v: synth.Renderer("cuda", rig=synth.rig_variant(kind, v)[0]) for v in groups}
    frames, t_prev = [], -0.05
    for f in range(nframes):
        t = f / synth.FRAME_HZ
        smp = [synth.imu_samples(trajs[i], s, t_prev, t) if imu else np.zeros((0, 7)) for i, s in enumerate(traj_ids)]
        t_prev = t
        cnt = np.array([len(x) for x in smp], np.int32)
        blk = np.zeros((S, max(max(len(x) for x in smp), 1), 7))
        for i, x in enumerate(smp):
            blk[i, :len(x)] = x
        i0 = i1 = None
        for v, idx in groups.items():
            tr = [trajs[i] for i in idx]
            r = rnds[v]
            if depth_range is None:
                a, b = r.stereo_frame(tr, t, f)
            else:
                a, b = r.depth_frame(tr, t, f, depth_factor=r.rig.depth_factor, max_range=depth_range)
            if i0 is None:
                i0 = torch.empty((S,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
                i1 = torch.empty((S,) + tuple(b.shape[1:]), dtype=b.dtype, device=b.device)
            for j, i in enumerate(idx):
                i0[i], i1[i] = a[j], b[j]
        frames.append((i0, i1, [t] * S, cnt, blk))
    return frames


def _nframes(kind):
    return RIGS[KINDS[kind]][4] + 40


_mixed_cache = {}


def _mixed(kind):
    if kind not in _mixed_cache:
        n = _nframes(kind)
        _mixed_cache[kind] = _frames(kind, VARIANTS, [3 + 7 * i for i in range(S8)], n)
    return _mixed_cache[kind]


def _check_streams(res, outs, ref, ref_outs, streams, what):
    (rs, kf, ba), (fs, fkf, fba) = res, ref
    for s in streams:
        _same(rs[s], fs[s], (what, "stream", s))
        assert kf[s] == fkf[s] and ba[s] == fba[s], (what, s, kf[s], fkf[s], ba[s], fba[s])
        if outs is not None:
            for f in range(len(outs)):
                _same(outs[f][s], ref_outs[f][s], (what, "frame", f, s))


@pytest.mark.parametrize("kind,mode,lanes", [("d435i_stereo", "frames", 1), ("d435i_stereo", "batches", 1), ("d435i_stereo", "host", 1),
                                             ("d435i_stereo", "frames", 2), ("euroc_like", "frames", 1), ("d435i_depth", "frames", 1),
                                             ("kitti_like", "frames", 1)])
def test_mixed_batch_equals_uniform_batches(ctx, monkeypatch, kind, mode, lanes):
    """8 streams on 4 rig variants, local map on: every stream's frame outputs, pose, landmarks, keyframe payloads, trajectory rows,
    IMU-state rows, local-map counts and corrections equal those of the same stream of a uniform tracker on that stream's config,
    fed the same images with the same seed."""
    import flvis_amd
    if lanes > 1:
        monkeypatch.setenv("FLVIS_LANES", str(lanes))
    steps = _mixed(kind)
    n = len(steps)
    cfgs = [_cfg(kind, v) for v in VARIANTS]
    trk = flvis_amd.Tracker(ctx, cfgs, S8, seed_base=SEED, traj_capacity=n)
    if lanes > 1:
        assert trk.lib.flvis_tracker_lanes(ctx._h) == lanes
    for s in range(S8):
        assert bytes(trk.stream_cfg(s)) == bytes(cfgs[s])
    outs = _feed(trk, steps, mode)
    res = _result(trk, ctx, n)
    assert trk.dropped_keyframes() == 0
    del trk
    kf_total = 0
    for v in sorted(set(VARIANTS)):
        uni = flvis_amd.Tracker(ctx, _cfg(kind, v), S8, seed_base=SEED, traj_capacity=n)
        uo = _feed(uni, steps, mode)
        ur = _result(uni, ctx, n)
        del uni
        streams = [s for s in range(S8) if VARIANTS[s] == v]
        _check_streams(res, outs, ur, uo, streams, (kind, mode, "variant", v))
        kf_total += sum(int(ur[1][s]) for s in streams)
    assert kf_total >= S8, "the run must make keyframes on every rig"
    assert sum(int(x) for x in res[2]) >= 1, "and optimise some windows"


def _lockstep(ctx, kind, variants, traj_ids, nframes, min_lock, min_kf):
    """test_gpu_pipeline._run_frontend_parity per stream: stream i against O.Tracker(O.load_config(its own yaml), seed_base + i)"""
    import flvis_amd
    from flvis_amd import synth
    S = len(variants)
    imu = RIGS[KINDS[kind]][3]
    steps = _frames(kind, variants, traj_ids, nframes)
    cfgs = [_cfg(kind, v) for v in variants]
    trk = flvis_amd.Tracker(ctx, cfgs, S, seed_base=SEED, traj_capacity=nframes)
    refs = [O.Tracker(O.load_config(_yaml_path(kind, v)), SEED + i) for i, v in enumerate(variants)]
    imu_want = [[] for _ in range(S)]
    lock = [0] * S
    n_kf = 0
    for f, (i0, i1, ts, cnt, blk) in enumerate(steps):
        t = ts[0]
        for i in range(S):
            if not imu:
                break
            smp = blk[i, :cnt[i]]
            trk.imu_feed_flvis(i, smp)
            for r in smp:
                imu_want[i].append(np.concatenate([[r[0]], refs[i].imu(r[0], r[1:4], r[4:7])]))
        h0, h1 = i0.cpu().numpy(), i1.cpu().numpy()
        outs = trk.image_feed(i0, i1, ts, with_local_map=False)
        for i in range(S):
            where = "frame %d stream %d (variant %d)" % (f, i, variants[i])
            if imu and (f % 3 == 2 or f == nframes - 1):
                rows, dropped = trk.imu_states(i)
                assert dropped == 0 and len(rows) == len(imu_want[i]), where
                assert np.array_equal(rows, np.array(imu_want[i]).reshape(-1, 11)), "IMU states, " + where
                imu_want[i] = []
            want = refs[i].image(t, h0[i], h1[i])
            got = outs[i]
            assert got["state"] == want["state"] and got["new_keyframe"] == want["new_keyframe"], where
            assert got["n_landmarks"] == want["n_landmarks"], where
            assert np.array_equal(got["dbg"], want["dbg"]), (where, got["dbg"], want["dbg"])
            assert np.array_equal(got["pose7"], want["pose7"]), (where, got["pose7"] - want["pose7"])
            if want["state"] == 1:
                lock[i] += 1
                gl, wl = trk.landmarks(i), refs[i].landmarks()
                assert np.array_equal(gl["ids"], wl["ids"]) and np.array_equal(gl["flags"], wl["flags"]), where
                assert np.array_equal(gl["p2d"], wl["p2d"]) and np.array_equal(gl["p2u"], wl["p2u"]), where
                assert np.array_equal(gl["p3w"], wl["p3w"]), where
            if want["new_keyframe"]:
                n_kf += 1
                gk, wk = trk.keyframe(i), refs[i].keyframe()
                assert gk["frame_id"] == wk["frame_id"] and np.array_equal(gk["lm_id"], wk["lm_id"]), where
                assert np.array_equal(gk["lm_2d"], wk["lm_2d"]) and np.array_equal(gk["lm_3d"], wk["lm_3d"]), where
                assert np.array_equal(gk["pose7"], wk["pose7"]), where
                gv, gdq, gdt = trk.get_keyframe_imu(i)
                wv, wdq, wdt = refs[i].keyframe_imu()
                assert gv == wv and gdt == wdt and np.array_equal(gdq, wdq), where
    assert n_kf >= min_kf
    assert min(lock) >= min_lock, lock


def test_mixed_batch_lockstep_with_the_oracle_d435i(ctx):
    """4 streams on 4 D435i stereo units, each beside the oracle's tracker on its own yaml: every frame bit-identical"""
    _lockstep(ctx, "d435i_stereo", [0, 1, 2, 3], [3, 140, 10, 17], 100, 30, 4)


def test_mixed_batch_lockstep_with_the_oracle_euroc_like(ctx):
    """3 streams on 3 EuRoC-like units (other intrinsics, distortion, baseline, IMU-camera rotation), beside the oracle"""
    _lockstep(ctx, "euroc_like", [0, 1, 2], [9, 16, 23], 60, 30, 3)


def _quat_wxyz(R):
    import _geom as G
    p7 = G.pose7(R, np.zeros(3))
    return np.array([p7[6], p7[3], p7[4], p7[5]])


@pytest.mark.parametrize("imu_factor", [False, True])
def test_local_map_uses_each_streams_rig(ctx, imu_factor):
    """flvis_ba_push_keyframe on two streams of one tracker whose rigs differ in K and T_imu_cam0: each window's corrections equal the
    oracle's LocalMap with that stream's K4 (and, with the IMU rotation factor on, that stream's camera-body rotation)."""
    import flvis_amd
    import _geom as G
    cfgs = [_cfg("d435i_stereo", 0), _cfg("d435i_stereo", 1)]
    sigma_g = 0.004
    trk = flvis_amd.Tracker(ctx, cfgs, 2, seed_base=1)
    if imu_factor:
        trk.set_imu_factor(True, sigma_g)
    for stream, seed in ((0, 21), (1, 22)):
        cfg = cfgs[stream]
        K4 = np.array([cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6]])
        Rcb = np.array(list(cfg.T_imu_cam0)).reshape(4, 4)[:3, :3].T
        seq = B.make_sequence(seed, n_kf=14, n_lm=260, outlier_frac=0.03)
        rng = np.random.default_rng(seed)
        ref = O.LocalMap(cfg.window_size, K4)
        if imu_factor:
            ref.set_imu_factor(True, sigma_g, _quat_wxyz(Rcb))
        produced = 0
        for k, kf in enumerate(seq["kfs"]):
            dq, dt = None, 0.0
            if imu_factor and k > 0:
                Ra, Rb = seq["gt"][k - 1][0], seq["gt"][k][0]
                dq, dt = _quat_wxyz((Ra.T @ Rcb).T @ (Rb.T @ Rcb) @ G.rodrigues(rng.normal(0, 1e-3, 3))), 0.1 + 0.02 * (k % 3)
                ref.next_imu(dq, dt)
            want = ref.push(kf["frame_id"], kf["pose7"], kf["lm_id"], kf["lm_2d"], kf["lm_3d"])
            got = trk.ba_push_keyframe(stream, kf["frame_id"], kf["pose7"], kf["lm_id"], kf["lm_2d"], kf["lm_3d"], imu_dq=dq, imu_dt=dt)
            assert (want is None) == (got is None), (stream, k)
            if want is None:
                continue
            produced += 1
            assert got["frame_id"] == want["frame_id"] and np.array_equal(got["lm_id"], want["lm_id"]), (stream, k)
            assert np.array_equal(got["outlier_id"], want["outlier_id"]), (stream, k)
            assert np.allclose(got["pose7"], want["pose7"], atol=1e-6, rtol=0), (stream, k, got["pose7"] - want["pose7"])
            assert np.allclose(got["lm_3d"], want["lm_3d"], atol=1e-6, rtol=0), (stream, k)
        assert produced == len(seq["kfs"]) - cfg.window_size + 1


_reset_cache = {}


def _reset_scenario(ctx):
    """D435i stereo, 8 streams on variants 0-3; stream 2 (variant 2) goes over to variant 5 at step R, right after it made a keyframe
    once its window has optimised.  A: the streams on their rigs; Bf: N steps with stream 2 rendered on variant 5."""
    if _reset_cache:
        return _reset_cache["v"]
    import flvis_amd
    kind = "d435i_stereo"
    r_min, N = RIGS["d435_stereo"][4], RIGS["d435_stereo"][5]
    total = r_min + 40 + N
    A = _frames(kind, VARIANTS, [3 + 7 * i for i in range(S8)], total)
    newv = list(VARIANTS)
    newv[2] = 5
    Bf = _frames(kind, newv, [4 + 7 * i for i in range(S8)], N)
    cfgs = [_cfg(kind, v) for v in VARIANTS]
    cfgs_new = [_cfg(kind, v) for v in newv]
    trk = flvis_amd.Tracker(ctx, cfgs, S8, seed_base=SEED, traj_capacity=total)
    uo = _feed(trk, A, "frames")
    del trk
    kfs = [f for f in range(r_min, total - N + 1) if uo[f - 1][2]["new_keyframe"]]
    assert kfs, "stream 2 makes no keyframe"
    R = kfs[0]
    A = A[:R + N]
    trk = flvis_amd.Tracker(ctx, cfgs, S8, seed_base=SEED, traj_capacity=R + N)
    uo = _feed(trk, A, "frames")
    und = _result(trk, ctx, R + N)
    del trk
    trk = flvis_amd.Tracker(ctx, cfgs_new, S8, seed_base=SEED, traj_capacity=R + N)
    fo = _feed(trk, Bf, "frames")
    fr = _result(trk, ctx, R + N)
    del trk
    assert fr[2][2] >= 1, "the new window optimises"
    _reset_cache["v"] = (cfgs, cfgs_new, A, Bf, R, N, uo, und, fo, fr)
    return _reset_cache["v"]


@pytest.mark.parametrize("lanes", [1, 2])
def test_reset_onto_a_new_rig_equals_fresh(ctx, monkeypatch, lanes):
    """Stream 2 of a running mixed batch (keyframes queued, local map on) reset onto another unit's calibration: it equals stream 2 of
    a fresh tracker on the new config, the other streams equal the undisturbed run, stream_cfg reports the new rig."""
    import flvis_amd
    if lanes > 1:
        monkeypatch.setenv("FLVIS_LANES", str(lanes))
    cfgs, cfgs_new, A, Bf, R, N, uo, und, fo, fr = _reset_scenario(ctx)
    trk = flvis_amd.Tracker(ctx, cfgs, S8, seed_base=SEED, traj_capacity=R + N)

    def hook(t, f):
        if f == R:
            t.reset_streams([2], [cfgs_new[2]])
            assert bytes(t.stream_cfg(2)) == bytes(cfgs_new[2])
            assert bytes(t.stream_cfg(3)) == bytes(cfgs[3])

    outs = _feed(trk, _splice(A, Bf, R, [2]), "frames", hook=hook)
    res = _result(trk, ctx, R + N)
    assert trk.dropped_keyframes() == 0
    _check_streams(res, None, fr, None, [2], "reset stream")
    for g in range(N):
        _same(outs[R + g][2], fo[g][2], ("frame", R + g))
    _check_streams(res, outs, und, uo, [s for s in range(S8) if s != 2], "other streams")


def test_batch_wide_fields_are_checked(ctx):
    """each batch-wide field in turn differs on stream 3: FLVIS_ERR_CONFIG naming the field and the stream, nothing created"""
    import flvis_amd
    base = _cfg("d435i_stereo", 0)
    other = _cfg("d435i_stereo", 1)
    changes = [("type_of_vi", 5), ("cam_type", 1), ("imu_type", 2), ("image_width", 656), ("image_height", 496), ("window_size", 6),
               ("skip_first_n_imgs", 3), ("need_equal_hist", 1)] + [("feature_para[%d]" % i, None) for i in range(6)]
    for name, val in changes:
        c = flvis_amd.FlvisCfg.from_buffer_copy(bytes(other))
        if name.startswith("feature_para"):
            i = int(name[-2])
            c.feature_para[i] = c.feature_para[i] * 0.5 if i != 4 else 0.002
        else:
            setattr(c, name, val)
        cfgs = [base, other, base, c]
        with pytest.raises(flvis_amd.FlvisError) as e:
            flvis_amd.Tracker(ctx, cfgs, 4)
        msg = str(e.value)
        assert "(-5)" in msg and name in msg and "stream 3" in msg, (name, msg)
    with pytest.raises(ValueError):
        flvis_amd.Tracker(ctx, [base, other], 3)


def test_bad_reset_entry_changes_nothing(ctx):
    """flvis_reset_streams_rigs with one bad entry among good ones: FlvisError, every stream keeps its config and the run stays
    bit-identical to the undisturbed one"""
    import flvis_amd
    cfgs, cfgs_new, A, Bf, R, N, uo, und, fo, fr = _reset_scenario(ctx)
    bad = flvis_amd.FlvisCfg.from_buffer_copy(bytes(cfgs_new[2]))
    bad.window_size = 5
    trk = flvis_amd.Tracker(ctx, cfgs, S8, seed_base=SEED, traj_capacity=R + N)

    def hook(t, f):
        if f == R:
            with pytest.raises(flvis_amd.FlvisError):
                t.reset_streams([2, 5], [cfgs_new[2], bad])
            with pytest.raises(flvis_amd.FlvisError):
                t.reset_streams([2, S8], [cfgs_new[2], cfgs_new[2]])
            for s in range(S8):
                assert bytes(t.stream_cfg(s)) == bytes(cfgs[s])

    outs = _feed(trk, A, "frames", hook=hook)
    res = _result(trk, ctx, R + N)
    _check_streams(res, outs, und, uo, list(range(S8)), "undisturbed")


def test_create_rigs_with_one_config_equals_create(ctx):
    """flvis_tracker_create_rigs given S copies of one config equals flvis_tracker_create"""
    import flvis_amd
    kind = "euroc_like"
    steps = _frames(kind, [1] * 4, [3, 10, 17, 24], _nframes(kind))
    cfg = _cfg(kind, 1)
    n = len(steps)
    a = flvis_amd.Tracker(ctx, [cfg] * 4, 4, seed_base=SEED, traj_capacity=n)
    ao = _feed(a, steps, "frames")
    ar = _result(a, ctx, n)
    del a
    b = flvis_amd.Tracker(ctx, cfg, 4, seed_base=SEED, traj_capacity=n)
    bo = _feed(b, steps, "frames")
    br = _result(b, ctx, n)
    for s in range(4):
        assert bytes(b.stream_cfg(s)) == bytes(cfg)
    del b
    _check_streams(ar, ao, br, bo, list(range(4)), "create_rigs vs create")
