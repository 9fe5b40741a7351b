"""GPU: flvis_loop_closer_localize / _localize_host / _set_drift against the oracle-assembled chain (tests/_loop_localize.py) on the scene
tests/test_oracle_loop_localize.py vetted -- rendered on the CPU and uploaded, so it is bit for bit that scene.  The features the chain
works on are the device's (each kernel has its own parity test); compared is everything the call adds: the candidate choice with its
tie rule, the pair check per candidate, best and T_c_map -- and that the call leaves no trace in the closer."""
import os
import tempfile

import numpy as np
import pytest

import _loop_chain as LC
import _loop_localize as LL
import _pgo_synth as PS
import _voc as V

pytestmark = pytest.mark.gpu
EXACT = 5e-324      # same_fix asserts |difference| < tol: with the smallest positive double, equality


class World:
    def __init__(self):
        import torch
        import flvis_amd
        self.ctx = flvis_amd.Context(0)
        self.cfg = LL.stereo_cfg()
        self.P0, self.P1, self.K4 = LL.cam_of(self.cfg)
        sc = self.sc = LL.scene()
        up = lambda pairs, k: torch.from_numpy(np.stack([p[k] for p in pairs])).cuda()
        self.kf0, self.kf1 = up(sc.kf, 0), up(sc.kf, 1)
        self.q0, self.q1 = up(sc.q, 0), up(sc.q, 1)
        self.blank = torch.zeros((1, 480, 640), dtype=torch.uint8, device="cuda")
        _, d, c, _ = self.ctx.orb_detect_and_compute(self.kf0, cap=1024)
        self.voc = V.build_vocabulary([d[i, :int(c[i])].cpu().numpy() for i in range(len(sc.kf))], k=6, depth=3)
        self.ctx.bow_set_vocabulary(*self.voc)
        self.kf_feat = self.features(self.kf0, self.kf1)
        self.q_feat = self.features(self.q0, self.q1)

    def features(self, a0, a1, P0=None, P1=None):
        """what add_keyframes stores for these images, through the separate entry points"""
        ctx = self.ctx
        kps, desc, cnt, _ = ctx.orb_detect_and_compute(a0, cap=1024)
        bi, bv, bn = [t.cpu().numpy() for t in ctx.bow_transform(desc, cnt, vcap=1024)]
        lm2, lm3, lmd, lmc = [t.cpu().numpy() for t in ctx.lc_keyframe_landmarks(a0, a1, 0, kps, desc, cnt, P0=self.P0 if P0 is None else P0,
                                                                                 P1=self.P1 if P1 is None else P1)]
        return [dict(bow=(bi[j, :bn[j]].copy(), bv[j, :bn[j]].copy()), lm2=lm2[j, :lmc[j]].copy(), lm3=lm3[j, :lmc[j]].copy(),
                     lmd=lmd[j, :lmc[j]].copy()) for j in range(a0.shape[0])]

    def closer(self, n_streams, max_keyframes, prm=LL.PARAMS, cfg=None):
        import flvis_amd
        return flvis_amd.LoopCloser(self.ctx, self.cfg if cfg is None else cfg, prm, n_streams=n_streams, max_keyframes=max_keyframes)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ctx.close()


def _sel(t, idx):
    import torch
    return t[torch.tensor(list(idx), device=t.device)].contiguous()


def test_localize_against_the_chain(world):
    """three sequences holding 9 (exactly full), 5 and 0 keyframes; queries named in the order [2, 0, 1], then a subset; n_best prefixes"""
    w = world
    sc = w.sc
    lc = w.closer(3, 9)
    ref = [LC.RefLoopCloser(w.K4, prm=LL.PARAMS, stream=s) for s in range(3)]
    odom = [sc.kf_gt, LC.drifted_odometry(sc.kf_gt, 3, sigma_t=0.008, sigma_r=0.002)]
    for i in range(9):
        streams = [0, 1] if i < 5 else [0]
        lc.add_keyframes(streams, _sel(w.kf0, [i] * len(streams)), _sel(w.kf1, [i] * len(streams)), [odom[s][i] for s in streams])
        for s in streams:
            ref[s].add(w.kf_feat[i], odom[s][i])
        lc.process()
    # query k of the scene for the sequence named k-th
    order = [2, 0, 1]
    got8 = lc.localize(order, w.q0[:3], w.q1[:3], n_best=8)
    for k, s in enumerate(order):
        want = LL.ref_localize(ref[s], w.q_feat[k], 8)
        LL.same_fix(got8[k], want)
    assert got8[0]["candidates"] == [] and got8[0]["best"] == -1 and got8[0]["n_landmarks"] > 100      # the empty sequence: no error
    assert got8[1]["best"] >= 0 and len(got8[1]["candidates"]) >= 3, got8[1]                            # (the CPU test's precondition)
    for n_best in (1, 4):
        got = lc.localize(order, w.q0[:3], w.q1[:3], n_best=n_best)
        for k in range(3):
            a, b = got[k]["candidates"], got8[k]["candidates"][:n_best]
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert all(x[key] == y[key] for key in ("kf", "score", "n_matches", "n_inliers", "accepted")) and np.array_equal(x["pose"], y["pose"])
            LL.same_fix(got[k], LL.ref_localize(ref[order[k]], w.q_feat[k], n_best))
    sub = lc.localize([1], w.q0[3:4], w.q1[3:4], n_best=8)                                              # a subset, another query
    LL.same_fix(sub[0], LL.ref_localize(ref[1], w.q_feat[3], 8))
    again = lc.localize([0], w.q0[1:2], w.q1[1:2], n_best=8)
    LL.same_fix(again[0], LL.ref_localize(ref[0], w.q_feat[1], 8))
    lc.close()


def test_ties_and_empties(world):
    w = world
    lc = w.closer(1, 4)
    ref = LC.RefLoopCloser(w.K4, prm=LL.PARAMS)
    blank_feat = w.features(w.blank, w.blank)[0]
    assert len(blank_feat["lmd"]) == 0 and len(blank_feat["bow"][0]) == 0
    for img0, img1, f in ((w.kf0[2:3], w.kf1[2:3], w.kf_feat[2]), (w.blank, w.blank, blank_feat), (w.kf0[2:3], w.kf1[2:3], w.kf_feat[2]),
                          (w.kf0[3:4], w.kf1[3:4], w.kf_feat[3])):
        lc.add_keyframes([0], img0, img1, [LL.IDENT])
        ref.add(f, LL.IDENT)
    fix = lc.localize([0], w.kf0[2:3], w.kf1[2:3], n_best=8)[0]
    LL.same_fix(fix, LL.ref_localize(ref, w.kf_feat[2], 8))
    kfs = [c["kf"] for c in fix["candidates"]]
    assert kfs[:2] == [0, 2] and fix["candidates"][0]["score"] == fix["candidates"][1]["score"]        # equal scores: the lower index first
    assert abs(fix["candidates"][0]["score"] - 1.0) < 1e-12 and 1 not in kfs                            # the blank keyframe: never a candidate
    assert fix["best"] == 0 and fix["kf"] == 0                                                          # equal inliers: the earlier candidate
    blank = lc.localize([0], w.blank, w.blank, n_best=8)[0]
    assert blank["n_landmarks"] == 0 and blank["candidates"] == [] and blank["best"] == -1 and blank["T_c_map"] is None
    lc.close()
    high = w.closer(1, 4, prm=dict(LL.PARAMS, minScore=1.5))                                            # above every score
    high.add_keyframes([0], w.kf0[2:3], w.kf1[2:3], [LL.IDENT])
    fix = high.localize([0], w.kf0[2:3], w.kf1[2:3], n_best=4)[0]
    assert fix["candidates"] == [] and fix["best"] == -1 and fix["n_landmarks"] == len(w.kf_feat[2]["lmd"])
    high.close()


def _state(lc, n_streams, keyframes=True):
    out = []
    for s in range(n_streams):
        P = lc.poses(s)
        kfs = [lc.keyframe(s, j) for j in range(len(P))] if keyframes else []
        out.append((P, lc.drift(s), lc.similarity_row(s), kfs))
    return out


def _same_state(a, b):
    for (Pa, Da, Ra, Ka), (Pb, Db, Rb, Kb) in zip(a, b):
        assert np.array_equal(Pa, Pb) and np.array_equal(Da, Db) and np.array_equal(Ra, Rb) and len(Ka) == len(Kb)
        for x, y in zip(Ka, Kb):
            assert all(np.array_equal(x[k], y[k]) for k in ("lm2", "lm3", "lmd")) and np.array_equal(x["bow"][0], y["bow"][0]) and \
                np.array_equal(x["bow"][1], y["bow"][1])


def test_localize_has_no_side_effects(world):
    """twin closers get the same keyframes; one is asked to localize before the first keyframe, between add_keyframes and process, and
    after process: events, similarity rows, poses, drift and keyframe contents stay identical bit for bit"""
    w = world
    sc = w.sc
    a, b = w.closer(2, 6), w.closer(2, 6)
    first = b.localize([1, 0], w.q0[:2], w.q1[:2], n_best=8)
    assert all(f["candidates"] == [] and f["best"] == -1 for f in first)
    for i in range(5):
        streams = [0, 1] if i != 2 else [1]
        args = (streams, _sel(w.kf0, [i] * len(streams)), _sel(w.kf1, [i] * len(streams)), [sc.kf_gt[i]] * len(streams))
        assert a.add_keyframes(*args).tolist() == b.add_keyframes(*args).tolist()
        b.localize([0, 1] if i % 2 else [1], w.q0[:2 if i % 2 else 1], w.q1[:2 if i % 2 else 1], n_best=4)   # the new keyframe is still pending
        ea, eb = a.process(), b.process()
        assert ea == eb and [e["kf_curr"] >= 0 for e in eb] == [s in streams for s in range(2)], (i, ea, eb)
        _same_state(_state(a, 2, i == 4), _state(b, 2, i == 4))
        fix = b.localize([0], w.q0[1:2], w.q1[1:2], n_best=8)
        assert len(fix[0]["candidates"]) >= 1
        _same_state(_state(a, 2, i == 4), _state(b, 2, i == 4))
        assert b.process() == a.process()                                                        # nothing became pending
    a.close()
    b.close()


def test_fleet_two_cameras_and_reset(world):
    """a closer on two different cameras: each sequence's result equals a one-sequence closer's on that camera, bit for bit (the PnP
    of a set reads its own sequence's K); after a reset the sequence has no candidates and the other's result is unchanged"""
    import torch
    import flvis_amd
    from flvis_amd import synth
    w = world
    rigs, cfgs, scenes = [], [], []
    for k in (1, 2):
        rig, text = synth.rig_variant("d435i_stereo", k)
        p = os.path.join(tempfile.gettempdir(), "flvis_loop_localize_rig%d.yaml" % k)
        open(p, "w").write(text)
        rigs.append(rig)
        cfgs.append(flvis_amd.load_config(p))
        scenes.append(LL.Scene(phase=0.3 * k, rig=rig, n_kf=3, query_times=(1.8,)))
    up = lambda imgs: torch.from_numpy(np.stack(imgs)).cuda()
    fleet = flvis_amd.LoopCloser(w.ctx, cfgs, LL.PARAMS, max_keyframes=4)
    solo = [flvis_amd.LoopCloser(w.ctx, cfgs[s], LL.PARAMS, n_streams=1, max_keyframes=4) for s in range(2)]
    for i in range(3):
        i0, i1 = up([scenes[s].kf[i][0] for s in range(2)]), up([scenes[s].kf[i][1] for s in range(2)])
        T = [scenes[s].kf_gt[i] for s in range(2)]
        fleet.add_keyframes([0, 1], i0, i1, T)
        for s in range(2):
            solo[s].add_keyframes([0], i0[s:s + 1], i1[s:s + 1], [T[s]])
    q0, q1 = up([scenes[s].q[0][0] for s in range(2)]), up([scenes[s].q[0][1] for s in range(2)])
    both = fleet.localize([0, 1], q0, q1, n_best=8)
    for s in range(2):
        one = solo[s].localize([0], q0[s:s + 1], q1[s:s + 1], n_best=8)[0]
        LL.same_fix(both[s], one, tol=EXACT)
        assert one["best"] >= 0 and len(one["candidates"]) >= 2, one
    # the chain with each unit's own camera agrees; (the same chain with the other unit's K would not: test_gpu_loop_closer_rigs)
    for s in range(2):
        P0, P1, K4 = LL.cam_of(cfgs[s])
        ref = LC.RefLoopCloser(K4, prm=LL.PARAMS, stream=s)
        i0, i1 = up([p[0] for p in scenes[s].kf]), up([p[1] for p in scenes[s].kf])
        for f, T in zip(w.features(i0, i1, P0, P1), scenes[s].kf_gt):
            ref.add(f, T)
        LL.same_fix(both[s], LL.ref_localize(ref, w.features(q0[s:s + 1], q1[s:s + 1], P0, P1)[0], 8))
    fleet.reset([0])
    after = fleet.localize([0, 1], q0, q1, n_best=8)
    assert after[0]["candidates"] == [] and after[0]["best"] == -1 and after[0]["n_landmarks"] == both[0]["n_landmarks"]
    LL.same_fix(after[1], both[1], tol=EXACT)
    for c in solo + [fleet]:
        c.close()


def test_set_drift_host_images_and_argument_errors(world):
    import flvis_amd
    w = world
    sc = w.sc
    lc = w.closer(2, 6)
    for i in range(3):
        lc.add_keyframes([0, 1], _sel(w.kf0, [i, i]), _sel(w.kf1, [i, i]), [sc.kf_gt[i]] * 2)
    before = [lc.poses(s) for s in range(2)]
    X = np.array([0.3, -0.2, 0.1, 0.02, -0.05, 0.1, 2.0])                      # (the quaternion is normalised by the call)
    Xn = np.concatenate([X[:3], X[3:] / np.linalg.norm(X[3:])])
    lc.set_drift(0, X)
    assert np.abs(lc.drift(0) - Xn).max() < 1e-15 and np.array_equal(lc.drift(1), LL.IDENT)
    lc.add_keyframes([0, 1], _sel(w.kf0, [3, 3]), _sel(w.kf1, [3, 3]), [sc.kf_gt[3]] * 2)
    P0, P1 = lc.poses(0), lc.poses(1)
    assert np.abs(P0[3] - PS.mul7(sc.kf_gt[3], Xn)).max() < 1e-12 and np.abs(P1[3] - sc.kf_gt[3]).max() < 1e-12
    assert np.array_equal(P0[:3], before[0]) and np.array_equal(P1[:3], before[1])       # earlier poses: untouched
    for bad in ([0, 0, 0, 0, 0, 0, 0.0], [np.nan, 0, 0, 0, 0, 0, 1.0], [0, 0, 0, np.inf, 0, 0, 1.0]):
        with pytest.raises(flvis_amd.FlvisError):
            lc.set_drift(0, bad)
    with pytest.raises(flvis_amd.FlvisError):
        lc.set_drift(2, LL.IDENT)
    assert np.abs(lc.drift(0) - Xn).max() < 1e-15
    # localize_host on padded-pitch host images = localize
    want = lc.localize([1, 0], w.q0[:2], w.q1[:2], n_best=8)
    pad = [[np.zeros((480, 704), np.uint8) for _ in range(2)] for _ in range(2)]
    for k in range(2):
        pad[k][0][:, :640], pad[k][1][:, :640] = sc.q[k][0], sc.q[k][1]
    host = lambda: lc.localize_host([1, 0], [pad[0][0][:, :640], pad[1][0][:, :640]], [pad[0][1][:, :640], pad[1][1][:, :640]], n_best=8)
    got = host()
    for a, b in zip(got, want):
        LL.same_fix(a, b, tol=EXACT)
    assert want[1]["best"] >= 0
    # argument errors: FLVIS_ERR_INVALID_ARG, and the next valid call is unchanged
    for kwargs, streams in ((dict(n_best=0), [1, 0]), (dict(n_best=9), [1, 0]), (dict(n_best=8), [1, 1])):
        with pytest.raises(flvis_amd.FlvisError) as e:
            lc.localize(streams, w.q0[:2], w.q1[:2], **kwargs)
        assert "loop_closer_localize failed (-1)" in str(e.value)                 # FLVIS_ERR_INVALID_ARG
        with pytest.raises(flvis_amd.FlvisError):
            lc.localize_host(streams, [pad[0][0][:, :640], pad[1][0][:, :640]], [pad[0][1][:, :640], pad[1][1][:, :640]], **kwargs)
    with pytest.raises(flvis_amd.FlvisError):
        lc.localize([2, 0], w.q0[:2], w.q1[:2], n_best=4)                       # a stream out of range
    with pytest.raises(flvis_amd.FlvisError):                                   # a wrong image shape (width 704: the padded array itself)
        lc.localize_host([1, 0], [pad[0][0], pad[1][0]], [pad[0][1], pad[1][1]], n_best=8)
    import ctypes
    fix = (flvis_amd.FlvisLcFix * 2)()
    st = (ctypes.c_int * 2)(1, 0)
    lib = w.ctx._lib
    assert lib.flvis_loop_closer_localize(lc._h, 2, st, flvis_amd._ptr(w.q0), flvis_amd._ptr(w.q1), 9, fix) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_localize(lc._h, 0, st, flvis_amd._ptr(w.q0), flvis_amd._ptr(w.q1), 4, fix) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_localize(lc._h, 2, st, flvis_amd._ptr(w.q0), flvis_amd._ptr(w.q1), 4, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    for a, b in zip(host(), want):
        LL.same_fix(a, b, tol=EXACT)
    for a, b in zip(lc.localize([1, 0], w.q0[:2], w.q1[:2], n_best=8), want):
        LL.same_fix(a, b, tol=EXACT)
    lc.reset([0])
    assert np.array_equal(lc.drift(0), LL.IDENT)                                # reset: back to the identity
    lc.close()
