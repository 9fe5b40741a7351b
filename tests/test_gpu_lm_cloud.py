"""The local map's sparse map cloud on the device (flvis_local_map_cloud*, include/flvis_hip.h): the per-stream record that
k_lm_cloud_append fills behind the window optimiser, and the fetch, against the corrections the optimiser returned and the numpy
restatement (tests/_lm_cloud.py).

Stand-alone local map: Tracker.ba_push_keyframe on 2 streams of _ba_synth.make_sequence(n_kf=14, n_lm=260) at the config's window, as
test_local_map_parity runs it (7 optimisations of ~200 multi-view landmarks per stream; tests/test_lm_cloud_inputs.py shows that ids
recur with gaps).  Tracker: 3 streams of the synthetic D435i stereo rig."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import _ba_synth as B
import _lm_cloud as LC
import _oracle as O

pytestmark = pytest.mark.gpu

SEEDS = (11, 12)
BIG = 4096          # room for every run of a stream (7 x ~200)
INV = -1            # FLVIS_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _cfg():
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_lm_cloud.yaml")
    open(p, "w").write(synth.D435I_STEREO_YAML)
    return flvis_amd.load_config(p)


_seq = {}


def _sequence(seed):
    if seed not in _seq:
        _seq[seed] = B.make_sequence(seed, n_kf=14, n_lm=260, outlier_frac=0.03)
    return _seq[seed]


def _push(trk, stream, seed, first=0, last=14):
    """keyframes first .. last - 1 of the seed's sequence into the stream -> the corrections returned (None: no optimisation)"""
    return [trk.ba_push_keyframe(stream, kf["frame_id"], kf["pose7"], kf["lm_id"], kf["lm_2d"], kf["lm_3d"])
            for kf in _sequence(seed)["kfs"][first:last]]


def _tracker(ctx, max_points=BIG, n=2, shared=False):
    """a new tracker on the context (which holds one at a time: the shared history's tracker is gone with it)"""
    import flvis_amd
    if not shared:
        _hist.clear()
    trk = flvis_amd.Tracker(ctx, _cfg(), n, seed_base=1)
    if max_points is not None:
        trk.local_map_cloud_enable(max_points)
    return trk


_hist = {}


def _history(ctx):
    """both streams driven once with a record that holds everything: the tracker and each stream's runs.  Shared and left unchanged
    (the tests that change a record make their own tracker)."""
    if "trk" not in _hist:
        trk = _tracker(ctx, shared=True)
        _hist["runs"] = [LC.runs_from_corrections(_push(trk, s, seed)) for s, seed in enumerate(SEEDS)]
        _hist["trk"] = trk
    return _hist["trk"], _hist["runs"]


def _raw_equal(got, s, rec, mode, ids=None):
    xyz, npts, n_out, n_drop = got[:4]
    want_xyz, want_ids, want_drop = LC.raw(rec, mode)
    assert n_out[s] == len(want_xyz) and n_drop[s] == want_drop
    assert xyz[s].dtype == np.float32 and np.array_equal(xyz[s].view(np.uint32), want_xyz.view(np.uint32))
    assert np.all(npts[s] == 1)
    if ids is not None:
        assert np.array_equal(ids[s], want_ids)


def test_raw_record_is_the_concatenation_of_the_corrections(ctx):
    trk, runs = _history(ctx)
    cfg = _cfg()
    K4 = np.array([cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6]])
    xyz, npts, n_out, n_drop, ids = trk.local_map_cloud([0, 1], "all", ids=True)
    for s, seed in enumerate(SEEDS):
        assert len(runs[s]) == 14 - cfg.window_size + 1
        rec = LC.record(runs[s], BIG)
        info = trk.local_map_cloud_info(s)
        assert info == dict(points=len(rec["ids"]), runs=len(runs[s]), dropped=0, capacity=BIG)
        # bit for bit the corrections' ids and fp64 points, narrowed once to float
        assert np.array_equal(ids[s], np.concatenate([r[1] for r in runs[s]]))
        assert np.array_equal(xyz[s].view(np.uint32), np.concatenate([r[2] for r in runs[s]]).astype(np.float32).view(np.uint32))
        _raw_equal((xyz, npts, n_out, n_drop), s, rec, LC.ALL, ids)
        # against the oracle's local map: ids exactly, positions within the tolerance test_local_map_parity holds for the same numbers
        ref = O.LocalMap(cfg.window_size, K4)
        want = LC.runs_from_corrections([ref.push(kf["frame_id"], kf["pose7"], kf["lm_id"], kf["lm_2d"], kf["lm_3d"])
                                         for kf in _sequence(seed)["kfs"]])
        assert np.array_equal(ids[s], np.concatenate([r[1] for r in want]))
        assert np.allclose(rec["pts"], np.concatenate([r[2] for r in want]), atol=1e-6, rtol=0)


def test_latest_equals_the_restatement(ctx):
    trk, runs = _history(ctx)
    got = trk.local_map_cloud([0, 1], "latest", ids=True)
    for s in range(2):
        rec = LC.record(runs[s], BIG)
        assert len(LC.select(rec, LC.LATEST)) < len(rec["ids"])
        _raw_equal(got, s, rec, LC.LATEST, got[4])


@pytest.mark.parametrize("mode", ["all", "latest"])
def test_voxel_clouds_equal_the_voxel_cloud_call_on_the_corrections(ctx, mode):
    import torch
    trk, runs = _history(ctx)
    m = LC.ALL if mode == "all" else LC.LATEST
    pts = []
    for s in range(2):
        rec = LC.record(runs[s], BIG)
        pts.append(rec["pts"][LC.select(rec, m)])
    case, clouds = LC.as_case(pts)
    for min_points in (1, 2):
        want = ctx.voxel_cloud(torch.from_numpy(case["p3"]).cuda(), torch.from_numpy(case["count"]).cuda(), torch.from_numpy(case["T"]).cuda(),
                               clouds, leaf=0.08, min_points=min_points)
        got = trk.local_map_cloud([0, 1], mode, leaf=0.08, min_points=min_points)
        for s in range(2):
            assert got[2][s] == want[2][s] and got[3][s] == want[3][s] and (min_points > 1 or 0 < got[2][s] <= len(pts[s]))
            if mode == "all" and min_points == 1:          # (the estimates of one landmark share voxels: the filter has work to do)
                assert got[2][s] < len(pts[s]) and got[1][s].max() > 1
            assert np.array_equal(got[0][s].view(np.uint32), want[0][s].view(np.uint32))
            assert np.array_equal(got[1][s], want[1][s])
    res = LC.voxel(LC.record(runs[0], BIG), m, 0.08)          # and the restatement, for stream 0
    got = trk.local_map_cloud([0], mode, leaf=0.08)
    assert np.array_equal(got[0][0].view(np.uint32), res["xyz"].view(np.uint32)) and np.array_equal(got[1][0], res["npts"])


def test_batches_repeats_and_the_host_form_give_the_same_bits(ctx):
    trk, runs = _history(ctx)
    for mode, leaf, ids in (("all", 0.0, True), ("latest", 0.0, True), ("all", 0.08, False), ("latest", 0.08, False)):
        both = trk.local_map_cloud([1, 0], mode, leaf=leaf, ids=ids)          # (listed in another order than the streams')
        again = trk.local_map_cloud([1, 0], mode, leaf=leaf, ids=ids)
        host = trk.local_map_cloud([1, 0], mode, leaf=leaf, ids=ids, host=True)
        for k, s in enumerate((1, 0)):
            one = trk.local_map_cloud([s], mode, leaf=leaf, ids=ids)
            for other, at in ((again, k), (host, k), (one, 0)):
                assert both[2][k] == other[2][at] and both[3][k] == other[3][at]
                assert np.array_equal(both[0][k].view(np.uint32), other[0][at].view(np.uint32))
                assert np.array_equal(both[1][k], other[1][at])
                if ids:
                    assert np.array_equal(both[4][k], other[4][at])
    # out_cap below n_out: the first rows are written and the full count returned
    full = trk.local_map_cloud([0, 1], "latest", ids=True)
    for host in (False, True):
        cut = trk.local_map_cloud([0, 1], "latest", cap=100, ids=True, host=host)
        for s in range(2):
            assert cut[2][s] == full[2][s] > 100 and len(cut[0][s]) == 100
            assert np.array_equal(cut[0][s], full[0][s][:100]) and np.array_equal(cut[4][s], full[4][s][:100])
    none = trk.local_map_cloud([0, 1], "all", leaf=0.08, cap=0)
    assert np.array_equal(none[2], trk.local_map_cloud([0, 1], "all", leaf=0.08)[2])


def test_the_fetch_leaves_corrections_and_record_alone(ctx):
    trk, runs = _history(ctx)
    before = [trk.correction(s) for s in range(2)]
    info = [trk.local_map_cloud_info(s) for s in range(2)]
    trk.local_map_cloud([0, 1], "latest", leaf=0.08)
    trk.local_map_cloud([0], "all", host=True)
    for s in range(2):
        after = trk.correction(s)
        assert after["frame_id"] == before[s]["frame_id"] and np.array_equal(after["lm_3d"], before[s]["lm_3d"])
        assert np.array_equal(after["lm_id"], before[s]["lm_id"]) and np.array_equal(after["pose7"], before[s]["pose7"])
        assert trk.local_map_cloud_info(s) == info[s]


def test_capacity_is_per_run(ctx):
    _, runs = _history(ctx)
    total = [sum(len(r[1]) for r in rs) for rs in runs]
    first = len(runs[0][0][1])
    # (capacity, stream 0's expected record): exactly the total; one short: the last run goes whole; below the first run: nothing
    for cap in (total[0], total[0] - 1, first - 1):
        trk = _tracker(ctx, cap, n=1)
        got_runs = LC.runs_from_corrections(_push(trk, 0, SEEDS[0]))
        for a, b in zip(got_runs, runs[0]):                                   # the optimiser does what it did: the record is beside it
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        rec = LC.record(runs[0], cap)
        info = trk.local_map_cloud_info(0)
        assert info == dict(points=len(rec["ids"]), runs=rec["runs"], dropped=rec["dropped"], capacity=cap)
        got = trk.local_map_cloud([0], "all", ids=True)
        _raw_equal(got, 0, rec, LC.ALL, got[4])
        del trk
    assert LC.record(runs[0], total[0])["dropped"] == 0 and LC.record(runs[0], total[0] - 1)["dropped"] == 1
    assert LC.record(runs[0], first - 1)["runs"] == 0 and LC.record(runs[0], first - 1)["dropped"] == len(runs[0])


def test_resets_clear_and_enabling_again(ctx):
    _, runs = _history(ctx)
    trk = _tracker(ctx)
    a = [LC.runs_from_corrections(_push(trk, s, seed, 0, 11)) for s, seed in enumerate(SEEDS)]
    assert all(len(r) == 4 for r in a)
    # KFMSG_CMD_RESET_LM leaves `map` alone: the record stays, and what the emptied window optimises next goes behind it
    trk.local_map_reset([0])
    kept = trk.local_map_cloud([0, 1], "all", ids=True)
    for s in range(2):
        _raw_equal(kept, s, LC.record(a[s], BIG), LC.ALL, kept[4])
    b0 = LC.runs_from_corrections(_push(trk, 0, SEEDS[1], 0, 10))          # (another sequence: a window filled anew, 3 optimisations)
    assert len(b0) == 3
    assert trk.local_map_counts()[1][0] == 3
    got = trk.local_map_cloud([0, 1], "all", ids=True)
    _raw_equal(got, 0, LC.record(a[0] + b0, BIG), LC.ALL, got[4])
    _raw_equal(got, 1, LC.record(a[1], BIG), LC.ALL, got[4])
    assert trk.local_map_cloud_info(0)["runs"] == 7
    # a new sequence takes the slot: that stream's record is emptied, the other's is not
    trk.reset_streams([0])
    got = trk.local_map_cloud([0, 1], "all", ids=True)
    assert got[2][0] == 0 and len(got[0][0]) == 0
    assert trk.local_map_cloud_info(0) == dict(points=0, runs=0, dropped=0, capacity=BIG)
    _raw_equal(got, 1, LC.record(a[1], BIG), LC.ALL, got[4])
    c0 = LC.runs_from_corrections(_push(trk, 0, SEEDS[0], 0, 9))
    assert len(c0) == 2
    got = trk.local_map_cloud([0], "all", ids=True)
    _raw_equal(got, 0, LC.record(c0, BIG), LC.ALL, got[4])
    # clear: the named stream alone
    trk.local_map_cloud_clear([1])
    assert trk.local_map_cloud_info(1) == dict(points=0, runs=0, dropped=0, capacity=BIG)
    got = trk.local_map_cloud([0, 1], "latest", ids=True)
    assert got[2][1] == 0
    _raw_equal(got, 0, LC.record(c0, BIG), LC.LATEST, got[4])
    d1 = LC.runs_from_corrections(_push(trk, 1, SEEDS[1], 11, 12))          # the window goes on where it was: one more optimisation
    assert len(d1) == 1
    got = trk.local_map_cloud([1], "all", ids=True)
    _raw_equal(got, 0, LC.record(d1, BIG), LC.ALL, got[4])
    # a record that dropped a run records again after clear
    trk.local_map_cloud_enable(len(c0[0][1]) + 1)
    assert trk.local_map_cloud_info(0) == dict(points=0, runs=0, dropped=0, capacity=len(c0[0][1]) + 1)     # enabling again starts empty
    e0 = LC.runs_from_corrections(_push(trk, 0, SEEDS[0], 9, 12))
    assert len(e0) == 3
    rec = LC.record(e0, len(c0[0][1]) + 1)
    assert rec["dropped"] >= 1
    info = trk.local_map_cloud_info(0)
    assert (info["points"], info["runs"], info["dropped"]) == (len(rec["ids"]), rec["runs"], rec["dropped"])
    trk.local_map_cloud_clear([0])
    f0 = LC.runs_from_corrections(_push(trk, 0, SEEDS[0], 12, 13))
    info = trk.local_map_cloud_info(0)
    want = LC.record(f0, len(c0[0][1]) + 1)
    assert (info["points"], info["runs"], info["dropped"]) == (len(want["ids"]), want["runs"], want["dropped"])
    # off: the calls refuse, the optimiser goes on
    trk.local_map_cloud_enable(0)
    import flvis_amd
    for call in (lambda: trk.local_map_cloud([0]), lambda: trk.local_map_cloud([0], host=True), lambda: trk.local_map_cloud_info(0),
                 lambda: trk.local_map_cloud_clear([0])):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):          # FLVIS_ERR_INVALID_ARG
            call()
    assert len(LC.runs_from_corrections(_push(trk, 0, SEEDS[0], 13, 14))) == 1
    del trk


def test_refusals_change_nothing(ctx):
    import torch
    import flvis_amd
    trk, runs = _history(ctx)
    lib, h = ctx._lib, ctx._h
    fn = lib.flvis_local_map_cloud
    xyz = torch.full((2, 16, 3), 7.0, dtype=torch.float32, device="cuda")
    npts = torch.full((2, 16), 7, dtype=torch.int32, device="cuda")
    ids = torch.full((2, 16), 7, dtype=torch.int64, device="cuda")
    n_out = np.full(2, -5, np.int64)

    def call(streams, mode=0, leaf=0.0, min_points=1, cap=16, x=xyz, i=None, out=n_out, n=None):
        arr = (C.c_int * max(len(streams), 1))(*streams)
        return fn(h, len(streams) if n is None else n, arr, mode, leaf, min_points, cap, C.c_void_p(x.data_ptr()) if x is not None else None,
                  C.c_void_p(npts.data_ptr()), C.c_void_p(i.data_ptr()) if i is not None else None,
                  out.ctypes.data_as(C.POINTER(C.c_int64)) if out is not None else None, None)
    info = [trk.local_map_cloud_info(s) for s in range(2)]
    for rc in (call([0, 2]), call([-1]), call([1, 1]), call([0], mode=2), call([0], mode=-1), call([0], leaf=0.08, i=ids),
               call([0], leaf=-0.1), call([0], leaf=float("nan")), call([0], leaf=float("inf")), call([0], min_points=0), call([0], cap=-1),
               call([0], x=None), call([0], out=None), call([], n=0), call([0], n=-1)):
        assert rc == INV
    assert torch.all(xyz == 7.0) and torch.all(npts == 7) and torch.all(ids == 7) and np.all(n_out == -5)
    assert [trk.local_map_cloud_info(s) for s in range(2)] == info
    assert call([0], i=ids) == 0 and n_out[0] == info[0]["points"]           # (the same call is accepted without the fault)
    with pytest.raises(flvis_amd.FlvisError):
        trk.local_map_cloud_info(2)
    with pytest.raises(flvis_amd.FlvisError):
        trk.local_map_cloud_clear([2])
    # the record is off on a tracker that never enabled it
    del trk
    off = _tracker(ctx, None)
    for call in (lambda: off.local_map_cloud([0]), lambda: off.local_map_cloud([0], host=True), lambda: off.local_map_cloud_info(0),
                 lambda: off.local_map_cloud_clear([0])):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            call()
    del off


# ---------------------------------------------------------------------------------------------------------------- the tracker
N_FRAMES = 100     # the rig tracks from frame ~50 (IMU initialisation), the windows fill by ~75: 6 / 5 / 4 optimisations by frame 100


def _frames(S, nframes):
    """per step: (img0 [S,H,W], img1, times [S], imu counts [S], imu samples [S, n, 7]) of the synthetic D435i stereo rig"""
    from flvis_amd import synth
    ids = [3 + 7 * i for i in range(S)]
    trajs = [synth.Trajectory(s) for s in ids]
    rnd = synth.Renderer("cuda")
    frames, t_prev = [], -0.05
    for f in range(nframes):
        t = f / synth.FRAME_HZ
        smp = [synth.imu_samples(trajs[i], s, t_prev, t) for i, s in enumerate(ids)]
        t_prev = t
        cnt = np.array([len(x) for x in smp], np.int32)
        blk = np.zeros((S, max(max(len(x) for x in smp), 1), 7))
        for i, x in enumerate(smp):
            blk[i, :len(x)] = x
        i0, i1 = rnd.stereo_frame(trajs, t, f)
        frames.append((i0.clone(), i1.clone(), [t] * S, cnt, blk))
    return frames


def test_tracker_batch_records_every_correction_and_changes_nothing(ctx):
    import flvis_amd
    S = 3
    cfg = _cfg()
    _hist.clear()
    steps = _frames(S, N_FRAMES)

    def final(trk):
        ctx.synchronize()
        kf, ba = trk.local_map_counts()
        return dict(rows=[trk.trajectory(s, 0, N_FRAMES) for s in range(S)], kf=kf, ba=ba, corr=[trk.correction(s) for s in range(S)])
    # frame by frame, the correction fetched after every step: the distinct ones, in order
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=1, traj_capacity=N_FRAMES)
    seen = [[] for _ in range(S)]
    for i0, i1, ts, cnt, blk in steps:
        for s in range(S):
            if cnt[s]:
                trk.imu_feed_flvis(s, blk[s, :cnt[s]])
        trk.image_feed(i0, i1, ts, want_out=False, with_local_map=True)
        for s in range(S):
            c = trk.correction(s)
            if c is not None and (not seen[s] or seen[s][-1]["frame_id"] != c["frame_id"]):
                seen[s].append(c)
    off = final(trk)
    del trk
    assert all(n >= 3 for n in off["ba"]), off["ba"]
    for s in range(S):
        assert len(seen[s]) == off["ba"][s]
    # one batch, record on
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=1, traj_capacity=N_FRAMES)
    trk.local_map_cloud_enable(1 << 16)
    trk.run_steps(steps, with_local_map=True)
    on = final(trk)
    got = trk.local_map_cloud(list(range(S)), "all", ids=True)
    for s in range(S):
        rec = LC.record(LC.runs_from_corrections(seen[s]), 1 << 16)
        info = trk.local_map_cloud_info(s)
        assert info["runs"] == on["ba"][s] == off["ba"][s] and info["dropped"] == 0 and info["points"] == len(rec["ids"])
        _raw_equal(got, s, rec, LC.ALL, got[4])
        # record on against record off: the same trajectories, keyframe counts and final corrections, bit for bit
        assert np.array_equal(on["rows"][s], off["rows"][s]) and on["kf"][s] == off["kf"][s]
        a, b = on["corr"][s], off["corr"][s]
        assert a["frame_id"] == b["frame_id"] and all(np.array_equal(a[k], b[k]) for k in ("pose7", "lm_id", "lm_3d", "outlier_id"))
    latest = trk.local_map_cloud(list(range(S)), "latest", ids=True)
    for s in range(S):
        _raw_equal(latest, s, LC.record(LC.runs_from_corrections(seen[s]), 1 << 16), LC.LATEST, latest[4])
    del trk


# ------------------------------------------------------------------- every optimisation is looked at, whatever the local map's pace
# A lane's local-map launches alternate between two HIP streams; a stream whose window is released early in one launch can be taken by
# the next launch before anything looked at its correction, and a launch that takes several keyframes of a stream optimises it several
# times.  With the record on the library launches one-keyframe workers with an append kernel behind each, one launch behind the other.
# Driven here flat out (one run_steps batch, nothing read back): 8 streams whose windows differ in size (so their optimisations end at
# different times inside a launch) with keyframes one or two frames apart; the local map launched every 2nd and every 8th frame (a
# lagging local map: a launch has up to 8 keyframes of a stream to take); one stream alone (the next launch follows at kernel-to-kernel
# distance).  Each against the corrections of a frame-by-frame run that fetches the correction after every step.
RACE_S, RACE_FRAMES = 8, 140
_race = {}


def _race_reference(ctx):
    if not _race:
        import flvis_amd
        _hist.clear()
        steps = _frames(RACE_S, RACE_FRAMES)
        trk = flvis_amd.Tracker(ctx, _cfg(), RACE_S, seed_base=1)
        seen = [[] for _ in range(RACE_S)]
        gap = 10 ** 6
        for f, (i0, i1, ts, cnt, blk) in enumerate(steps):
            for s in range(RACE_S):
                if cnt[s]:
                    trk.imu_feed_flvis(s, blk[s, :cnt[s]])
            trk.image_feed(i0, i1, ts, want_out=False, with_local_map=True)
            for s in range(RACE_S):
                c = trk.correction(s)
                if c is not None and (not seen[s] or seen[s][-1]["frame_id"] != c["frame_id"]):
                    gap = min(gap, c["frame_id"] - seen[s][-1]["frame_id"]) if seen[s] else gap
                    seen[s].append(c)
        _, ba = trk.local_map_counts()
        del trk
        assert all(len(seen[s]) == ba[s] >= 10 for s in range(RACE_S)), ba
        print("smallest distance of two optimisations of a stream: %d frames" % gap)
        assert gap <= 2                                                      # a stream optimises again within two frames
        sizes = [np.mean([len(c["lm_id"]) for c in seen[s]]) for s in range(RACE_S)]
        print("multi-view landmarks per optimisation, by stream:", np.round(sizes, 1))
        assert max(sizes) > 1.05 * min(sizes), sizes                         # windows of unequal size
        _race.update(steps=steps, seen=seen, ba=ba)
    return _race


@pytest.mark.parametrize("S,every", [(RACE_S, None), (RACE_S, "2"), (RACE_S, "8"), (1, None)])
def test_no_optimisation_is_missed_at_any_pace(ctx, monkeypatch, S, every):
    import flvis_amd
    ref = _race_reference(ctx)
    _hist.clear()
    if every is None:
        monkeypatch.delenv("FLVIS_BA_EVERY", raising=False)
    else:
        monkeypatch.setenv("FLVIS_BA_EVERY", every)
    trk = flvis_amd.Tracker(ctx, _cfg(), S, seed_base=1)
    trk.local_map_cloud_enable(1 << 15)
    steps = [(i0[:S].contiguous(), i1[:S].contiguous(), ts[:S], cnt[:S].copy(), blk[:S].copy()) for i0, i1, ts, cnt, blk in ref["steps"]]
    trk.run_steps(steps, with_local_map=True)
    ctx.synchronize()
    kf, ba = trk.local_map_counts()
    assert trk.dropped_keyframes() == 0
    got = trk.local_map_cloud(list(range(S)), "all", ids=True)
    for s in range(S):
        rec = LC.record(LC.runs_from_corrections(ref["seen"][s]), 1 << 15)
        info = trk.local_map_cloud_info(s)
        assert info["dropped"] == 0 and info["runs"] == ba[s] == ref["ba"][s], (s, info, ba[s], ref["ba"][s])
        assert info["points"] == len(rec["ids"])
        _raw_equal(got, s, rec, LC.ALL, got[4])
    del trk
