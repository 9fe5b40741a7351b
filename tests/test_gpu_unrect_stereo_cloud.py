"""GPU: the dense map on the unrectified stereo rig through the pipeline (flvis_keyframe_log_rectified_pair,
flvis_keyframe_log_unrect_stereo_z16, flvis_keyframe_log_unrect_stereo_cloud, flvis_loop_closer_unrect_stereo_cloud; include/flvis_hip.h)
against the restatement -- tests/_rectify.py on keyframe_log_get's images, tests/_dense_stereo.py on the rectified pair, then
tests/_depth_cloud.py under the fetched poses -- bit for bit.

Two streams of the synthetic EuRoC-like rig on units of different distortion, focal length and baseline (synth.rig_variant 1 and 2).  The
cloud samples every 7th pixel of rows 216 .. 239, so the restatement needs the matcher only on a band of rows around them, and the first
three keyframes per stream keep it to seconds.  The run is made twice with the same seed, once making every new call and once making
none: everything a caller can fetch afterwards is compared bit for bit."""
import numpy as np
import pytest

import _dense_stereo as DS
import _depth_cloud as DC
import _kf_log as KL
import _rectify as RC
import _voc as V
from test_gpu_kf_log import CAP, IDS, STEPS
from test_gpu_kf_log_closer import _closer, _same_event, _vocabulary
from test_gpu_stream_reset import _cfg as _stock_cfg
from test_gpu_stream_rigs import _cfg, _frames

pytestmark = pytest.mark.gpu

KIND, VARIANTS, S, TAIL, NSTEPS = "euroc_like", [1, 2], 2, 5, STEPS["euroc_like"]
CFG_ERR, INV = -5, -1
V0, V1, B0, B1 = 216, 240, 208, 248           # the sampled rows; the band of rows the restatement runs the matcher on
SAMPLING = dict(window=(0, V0, 0, V1), step=7, z_min=0.3, z_max=10.0)
PRM_DICT = DC.params((0, V0, 0, V1), (7, 7), 0.3, 10.0)
STEREO = dict(n_disp=64)
SPRM = DS.params(**STEREO)
DF = 1000.0
USE = 3                                       # keyframes per stream the clouds are cut to
DRIFT = [0.3, -0.2, 0.1, 0.0, 0.0, np.sin(0.1), np.cos(0.1)]


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _cfgs():
    return [_cfg(KIND, v) for v in VARIANTS]


def _cam(cfg):
    return [cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6], DF]


_pair_cache, _z_cache = {}, {}


def _pair(entry, cfg, key):
    """the entry's rectified pair by the restatement -> (img0, img1)"""
    if key not in _pair_cache:
        rect, _ = RC.restate(RC.one(np.stack([entry["img0"], entry["img1"]]), RC.cameras_of_cfg(cfg)))
        _pair_cache[key] = (rect[0], rect[1])
    return _pair_cache[key]


def _z16(entry, cfg, key):
    """the entry's Z16 image by the restatement: the band's rows whose whole support lies in the band, 0 elsewhere (never sampled)"""
    if key not in _z_cache:
        r0, r1 = _pair(entry, cfg, key)
        _, zb = DS.restate_one(r0[B0:B1], r1[B0:B1], -cfg.P1[3], DF, SPRM)
        z = np.zeros(r0.shape, np.uint16)
        m = 3 + SPRM["agg_r"]
        z[B0 + m:B1 - m] = zb[m:B1 - B0 - m]
        _z_cache[key] = z
    return _z_cache[key]


def _case(entries, poses, seqs):
    """one cloud over the listed sequences' first entries, each sequence a range on its own camera.  poses[s]: one pose per used entry"""
    cfgs = _cfgs()
    depth, T, ranges, cams = [], [], [], []
    for s in seqs:
        n = len(poses[s])
        ranges.append((len(depth), n))
        cams.append(_cam(cfgs[s]))
        depth += [_z16(e, cfgs[s], (s, i)) for i, e in enumerate(entries[s][:n])]
        T += list(poses[s])
    return dict(depth=np.stack(depth), T=np.array(T), clouds=[ranges], cams=cams, prm=PRM_DICT)


def _check(got, g, want, what):
    xyz, npts, n_out, n_drop, n_valid = got
    assert (int(n_out[g]), int(n_drop[g]), int(n_valid[g])) == (want["n_out"], want["n_dropped"], want["n_valid"]), \
        (what, int(n_out[g]), int(n_drop[g]), int(n_valid[g]), want["n_out"], want["n_dropped"], want["n_valid"])
    assert xyz[g].tobytes() == want["xyz"].tobytes() and np.array_equal(npts[g], want["npts"]), what


def _pipeline(ctx, frames, calls):
    """the batch, the log into a closer, a drift and the log again, then TAIL more frames one by one.  calls: make the new calls (and check
    them against the restatement) between those steps -> everything a caller can fetch"""
    import flvis_amd
    cfgs = _cfgs()
    assert cfgs[0].cam_type == 1 and abs(cfgs[0].P1[3] / cfgs[1].P1[3] - 1) > 0.01, "the unrectified rig, two baselines"
    assert abs(cfgs[0].cam0_distortion[0] / cfgs[1].cam0_distortion[0] - 1) > 0.01, "two lenses"
    trk = flvis_amd.Tracker(ctx, cfgs, S, seed_base=1)
    trk.keyframe_log_enable(CAP)
    trk.run_steps(frames[:NSTEPS], with_local_map=True)
    made = [trk.keyframe_log_info(s)["logged"] for s in range(S)]
    assert min(made) >= USE and max(made) <= CAP, made
    entries = [[trk.keyframe_log_get(s, i) for i in range(made[s])] for s in range(S)]
    logged = [[e["pose7"] for e in entries[s][:USE]] for s in range(S)]
    cut = [(0, USE)] * 3
    if calls:
        m = 3 + SPRM["agg_r"]
        listed = [(0, 0), (1, 2), (0, 0), (0, 1)]
        r0, r1 = trk.keyframe_log_rectified_pair(listed)
        only1 = trk.keyframe_log_rectified_pair(listed[1:2], want0=False)
        z = trk.keyframe_log_unrect_stereo_z16(listed[:3], depth_factor=DF, **STEREO)
        ctx.synchronize()
        r0, r1, z = r0.cpu().numpy(), r1.cpu().numpy(), z.cpu().numpy().view(np.uint16)
        assert only1[0] is None and np.array_equal(only1[1].cpu().numpy()[0], r1[1])
        for k, (s, i) in enumerate(listed):
            w0, w1 = _pair(entries[s][i], cfgs[s], (s, i))
            assert np.array_equal(r0[k], w0) and np.array_equal(r1[k], w1), ("rectified pair", s, i)
            assert not np.array_equal(w0, entries[s][i]["img0"]), "the raw image is another one"
        for k, (s, i) in enumerate(listed[:3]):
            want = _z16(entries[s][i], cfgs[s], (s, i))
            assert (want[V0:V1] > 0).mean() > 0.4, "the restatement finds depth in the sampled rows"
            assert np.array_equal(z[k][B0 + m:B1 - m], want[B0 + m:B1 - m]), ("z16", s, i)
        for leaf in (0.08, 0.0):
            got = trk.keyframe_log_unrect_stereo_cloud([0, 1, 1], leaf=leaf, slices=cut, depth_factor=DF, **STEREO, **SAMPLING)
            for g, s in enumerate([0, 1, 1]):
                want = DC.restate(_case(entries, logged, [s]), 0, leaf)
                assert want["n_valid"] > 200, (s, want["n_valid"])
                _check(got, g, want, ("log", leaf, s))
        host = trk.keyframe_log_unrect_stereo_cloud([1, 0], leaf=0.08, host=True, slices=[(1, 1), (0, USE)], depth_factor=DF, **STEREO, **SAMPLING)
        one = dict(depth=_z16(entries[1][1], cfgs[1], (1, 1))[None], T=np.array([logged[1][1]]), clouds=[[(0, 1)]], cams=[_cam(cfgs[1])],
                   prm=PRM_DICT)
        _check(host, 0, DC.restate(one, 0, 0.08), "host, a slice of one entry")
        _check(host, 1, DC.restate(_case(entries, logged, [0]), 0, 0.08), "host, the first entries")
        # the lens is the stream's own: stream 1's pair under stream 0's cameras is another pair
        other, _ = RC.restate(RC.one(entries[1][0]["img0"], RC.cameras_of_cfg(cfgs[0])[:1]))
        assert not np.array_equal(other[0], _pair(entries[1][0], cfgs[1], (1, 0))[0])
        for bad in ([S], [-1], []):
            with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
                trk.keyframe_log_unrect_stereo_cloud(bad, **STEREO, **SAMPLING)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            trk.keyframe_log_unrect_stereo_cloud([0], n_disp=300, **SAMPLING)
        for call in (trk.keyframe_log_unrect_stereo_z16, trk.keyframe_log_rectified_pair):
            for bad in ([(0, made[0])], [(S, 0)], [(0, -1)], []):
                with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
                    call(bad)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            trk.keyframe_log_rectified_pair([(0, 0)], want0=False, want1=False)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
            trk.keyframe_log_stereo_cloud([0], **SAMPLING)                # the rectified rig's call keeps refusing this rig
    _vocabulary(ctx, entries)
    lc = _closer(ctx, cfgs, S, True, max_keyframes=2 * CAP)
    rounds = lc.add_logged(process=True)
    if calls:
        poses = [lc.poses(s) for s in range(S)]
        # the closer's calls take a sequence's logged entries 0 .. stored - first - 1: a first keyframe near the end keeps the restatement
        # to one or two images per cloud
        got = lc.unrect_stereo_cloud([[1]], first_kf=[[made[1] - 1]], leaf=0.08, depth_factor=DF, **STEREO, **SAMPLING)
        _check(got, 0, DC.restate(_case(entries, [None, poses[1][-1:]], [1]), 0, 0.08), "closer, entry 0 under the last stored pose")
        got = lc.unrect_stereo_cloud([[0], [1, 0]], first_kf=[[made[0] - 2], [made[1] - 1, made[0] - 2]], leaf=0.08, depth_factor=DF, **STEREO,
                                     **SAMPLING)
        _check(got, 0, DC.restate(_case(entries, [poses[0][-2:], None], [0]), 0, 0.08), "closer, two entries")
        _check(got, 1, DC.restate(_case(entries, [poses[0][-2:], poses[1][-1:]], [1, 0]), 0, 0.08), "closer, two sequences in one cloud")
        host = lc.unrect_stereo_cloud([[0]], first_kf=[[made[0] - 2]], leaf=0.0, host=True, depth_factor=DF, **STEREO, **SAMPLING)
        _check(host, 0, DC.restate(_case(entries, [poses[0][-2:], None], [0]), 0, 0.0), "closer, host")
    lc.set_drift(1, DRIFT)
    lc.add_logged(process=False)                                          # the log is not consumed: each sequence holds it twice now
    if calls:
        poses = [lc.poses(s) for s in range(S)]
        assert [len(p) for p in poses] == [2 * m_ for m_ in made]
        got = lc.unrect_stereo_cloud([[1], [0]], first_kf=[[2 * made[1] - 2], [2 * made[0] - 1]], leaf=0.08, depth_factor=DF, **STEREO, **SAMPLING)
        _check(got, 0, DC.restate(_case(entries, [None, poses[1][-2:]], [1]), 0, 0.08), "after set_drift")
        _check(got, 1, DC.restate(_case(entries, [poses[0][-1:], None], [0]), 0, 0.08), "the other sequence")
        before = lc.unrect_stereo_cloud([[1]], first_kf=[[made[1] - 2]], leaf=0.08, depth_factor=DF, **STEREO, **SAMPLING)
        assert before[0][0].tobytes() != got[0][0].tobytes(), "the cloud follows the drift"
        for bad in ([[2 * made[1] + 1]], [[-1]]):
            with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
                lc.unrect_stereo_cloud([[1]], first_kf=bad, **STEREO, **SAMPLING)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
            lc.stereo_cloud([[0]], **SAMPLING)
    state = [dict(poses=lc.poses(s), drift=lc.drift(s), row=lc.similarity_row(s)[:made[s]]) for s in range(S)]
    print("unrectified stereo cloud run (calls: %s): keyframes per stream %s" % (calls, made))
    after = [[trk.keyframe_log_get(s, i) for i in range(made[s])] for s in range(S)]
    outs = []
    for i0, i1, ts, cnt, blk in frames[NSTEPS:]:
        for s in range(S):
            if cnt[s]:
                trk.imu_feed_flvis(s, blk[s, :cnt[s]])
        outs.append(trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True))
    info = [trk.keyframe_log_info(s) for s in range(S)]
    lc.close()
    del trk
    return dict(entries=entries, after=after, rounds=rounds, state=state, outs=outs, info=info)


def test_unrect_stereo_clouds_equal_the_restatement_and_change_nothing(ctx):
    frames = _frames(KIND, VARIANTS, IDS[:S], NSTEPS + TAIL)
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


@pytest.mark.parametrize("rig", ["d435_depth", "d435_stereo"])
def test_a_depth_rig_and_the_rectified_rig_are_refused(ctx, rig):
    import flvis_amd
    trk = flvis_amd.Tracker(ctx, _stock_cfg(rig), 1, seed_base=1)
    trk.keyframe_log_enable(4)
    for host in (False, True):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
            trk.keyframe_log_unrect_stereo_cloud([0], host=host, **SAMPLING)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        trk.keyframe_log_unrect_stereo_z16([(0, 0)])
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
        trk.keyframe_log_rectified_pair([(0, 0)])
    ctx.bow_set_vocabulary(*V.build_vocabulary([np.random.default_rng(4).integers(0, 256, (600, 32)).astype(np.uint8)], k=8, depth=3))
    lc = _closer(ctx, _stock_cfg(rig), 1, False)
    for host in (False, True):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % CFG_ERR):
            lc.unrect_stereo_cloud([[0]], host=host, **SAMPLING)
    lc.close()
    del trk


def test_a_log_that_is_off_is_refused_and_an_empty_one_gives_nothing(ctx):
    import flvis_amd
    trk = flvis_amd.Tracker(ctx, _stock_cfg("euroc_like"), 1, seed_base=1)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        trk.keyframe_log_unrect_stereo_cloud([0], **SAMPLING)
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        trk.keyframe_log_rectified_pair([(0, 0)])
    trk.keyframe_log_enable(4)
    got = trk.keyframe_log_unrect_stereo_cloud([0], **SAMPLING)
    assert got[2][0] == 0 and got[4][0] == 0 and len(got[0][0]) == 0
    with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
        trk.keyframe_log_rectified_pair([(0, 0)])                       # nothing is logged yet
    del trk
