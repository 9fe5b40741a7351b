"""GPU: loop closing on an unrectified stereo rig (the EuRoC camera) -- flvis_hip_lc_keyframe_landmarks_unrect against the checker composed
from the CPU oracle (tests/_lc_unrect.py: O.lk, O.undistort_points twice, O.triangulate_dlt, the keep rule) on the inputs
tests/test_lc_unrect_inputs.py vetted, and flvis_loop_closer with flvis_loop_closer_set_stereo_unrect against the oracle chain of
tests/_loop_chain.py.  The reference's own STEREO_UNRECT case is empty; with the switch off the closer still is."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import _lc_unrect as U
import _loop_chain as LC
import _loop_localize as LL
import _pgo_synth as PS
import _voc as V

pytestmark = pytest.mark.gpu
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
N_KF, PER, MAXKF = 62, 50, 64          # the reference's 50-keyframe gate (:453) sets the size
PHASES = (0.0, 0.9)


class World:
    """shared and never changed: the context, the CPU-rendered inputs on the device, the two tours of the stock rig with the device's
    features of every keyframe, a vocabulary, and two other units of the rig"""

    def __init__(self):
        import torch
        import flvis_amd
        from flvis_amd import synth
        self.ctx = flvis_amd.Context(0)
        inp = self.inp = U.inputs()
        self.cfg, self.cam = inp.cfg, inp.cam
        up = lambda imgs: torch.from_numpy(np.stack(imgs)).cuda()
        # the keyframes of the parity call: the true pair, the flat second image, a keyframe whose count is 0, the second image that keeps
        # nothing, and another true pair
        self.i0 = up([inp.a0, inp.a0, inp.a0, inp.a0, inp.b0])
        self.i1 = up([inp.a1, inp.flat, inp.a1, inp.moved, inp.b1])
        self.kps, self.desc, cnt, _ = self.ctx.orb_detect_and_compute(self.i0, cap=1024)
        self.cnt = cnt.clone()
        self.cnt[2] = 0
        self.variant = {k: U.load_cfg(k) for k in (1, 2)}       # (Rig, cfg)
        self._tours = None

    def want(self, j, cam=None, i0=None, i1=None, kps=None, desc=None, cnt=None):
        """the checker on keyframe j of a call's inputs (default: the parity call's)"""
        i0, i1 = (self.i0 if i0 is None else i0), (self.i1 if i1 is None else i1)
        kps, desc, cnt = (self.kps if kps is None else kps), (self.desc if desc is None else desc), (self.cnt if cnt is None else cnt)
        c = int(cnt[j])
        return U.check(i0[j].cpu().numpy(), i1[j].cpu().numpy(), kps[j, :c].cpu().numpy(), desc[j, :c].cpu().numpy(), self.cam if cam is None else cam)

    def features(self, a0, a1, cfgs):
        """what add_keyframes stores for these images with the switch on, through the separate entry points"""
        ctx = self.ctx
        kps, desc, cnt, _ = ctx.orb_detect_and_compute(a0, cap=1024)
        bi, bv, bn = [t.cpu().numpy() for t in ctx.bow_transform(desc, cnt, vcap=1024)]
        lm2, lm3, lmd, lmc = [t.cpu().numpy() for t in ctx.lc_keyframe_landmarks_unrect(a0, a1, cfgs, kps, desc, cnt)]
        return [dict(bow=(bi[j, :bn[j]].copy(), bv[j, :bn[j]].copy()), lm2=lm2[j, :lmc[j]].copy(), lm3=lm3[j, :lmc[j]].copy(),
                     lmd=lmd[j, :lmc[j]].copy()) for j in range(a0.shape[0])]

    def tours(self):
        """the two sequences of the loop test, rendered on the device once: frames[i] = (img0 [2,h,w], img1), gt[s][i] in the RECTIFIED frame"""
        if self._tours is None:
            from flvis_amd import synth
            rnd = synth.Renderer("cuda", rig=self.inp.rig)
            trs = [LC.LoopTrajectory(phase=p) for p in PHASES]
            times = LC.keyframe_times(N_KF, PER)
            frames = [rnd.stereo_frame(trs, t, i) for i, t in enumerate(times)]
            gt = [[U.rectified_gt(tr, t, self.inp.rig, self.cfg) for t in times] for tr in trs]
            train = []
            for i in range(0, N_KF, 6):     # vocabulary from the device's descriptors of every sixth keyframe of sequence 0
                _, d, c, _ = self.ctx.orb_detect_and_compute(frames[i][0][0:1], cap=1024)
                train.append(d[0, :int(c[0])].cpu().numpy())
            self.ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))
            self._tours = (frames, gt)
        return self._tours


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ctx.close()


def sentinels(n, cap, desc=None):
    import torch
    return (torch.full((n, cap, 2), -7.5, dtype=torch.float32, device="cuda"), torch.full((n, cap, 3), -9.25, dtype=torch.float64, device="cuda"),
            torch.full((n, cap, 32), 0xA5, dtype=torch.uint8, device="cuda") if desc is None else desc,
            torch.full((n,), -3, dtype=torch.int32, device="cuda"))


def untouched(out):
    lm2, lm3, lmd, cnt = [t.cpu().numpy() for t in out]
    return (lm2 == -7.5).all() and (lm3 == -9.25).all() and (lmd == 0xA5).all() and (cnt == -3).all()


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
def test_landmarks_equal_the_composed_checker(world):
    """one call over the five keyframes: the kept set and its order, lm_2d and the descriptors bit for bit, lm_3d within the STEREO_RECT
    test's 1e-9 * max(1, |want|); rows from the count on are never written; the in-place descriptor form gives the same"""
    w = world
    n, cap = w.i0.shape[0], w.kps.shape[1]
    out = sentinels(n, cap)
    w.ctx.lc_keyframe_landmarks_unrect(w.i0, w.i1, w.cfg, w.kps, w.desc, w.cnt, out=out)
    lm2, lm3, lmd, lmc = [t.cpu().numpy() for t in out]
    desc2 = w.desc.clone()
    ip = [t.cpu().numpy() for t in w.ctx.lc_keyframe_landmarks_unrect(w.i0, w.i1, w.cfg, w.kps, desc2, w.cnt, in_place=True, out=sentinels(n, cap, desc2))]
    assert np.array_equal(ip[0], lm2) and np.array_equal(ip[1], lm3) and np.array_equal(ip[3], lmc)
    kept = []
    for j in range(n):
        want = w.want(j)
        c = int(lmc[j])
        kept.append(c)
        print("keyframe %d: %d keypoints, %d kept (checker %d)" % (j, int(w.cnt[j]), c, len(want["lm2"])))
        assert c == len(want["lm2"]), (j, c, len(want["lm2"]))
        assert np.array_equal(lmd[j, :c], want["lmd"]), j                      # the kept set and its order
        assert np.array_equal(lm2[j, :c], want["lm2"]), (j, np.abs(lm2[j, :c] - want["lm2"]).max())
        err = np.abs(lm3[j, :c] - want["lm3"]) / np.maximum(1.0, np.abs(want["lm3"]))
        print("    lm_3d: largest error / max(1, |want|) = %.3e" % (err.max() if c else 0.0))
        assert (err < 1e-9).all(), (j, err.max())
        assert (lm2[j, c:] == -7.5).all() and (lm3[j, c:] == -9.25).all() and (lmd[j, c:] == 0xA5).all(), j
        assert np.array_equal(ip[2][j, :c], want["lmd"]) and np.array_equal(ip[2][j, c:], w.desc[j, c:].cpu().numpy()), j
    nk = int(w.cnt[0])
    assert kept[0] > 100 and 0 < kept[1] < nk and kept[2] == 0 and kept[3] == 0 and kept[4] > 100, kept
    # the existing calls keep the reference's empty case
    old = w.ctx.lc_keyframe_landmarks(w.i0, w.i1, 1, w.kps, w.desc, w.cnt, P0=w.cam["P0"], P1=w.cam["P1"])
    assert not old[3].cpu().numpy().any()


# ---- 2. a rig per image -------------------------------------------------------------------------------------------------------
def test_a_rig_per_image_equals_the_single_calls(world):
    import torch
    from flvis_amd import synth
    w = world
    tr = LC.LoopTrajectory(phase=0.4)
    cfgs, i0, i1 = [], [], []
    for j, k in enumerate((1, 2)):
        rig, cfg = w.variant[k]
        a, b = synth.Renderer("cuda", rig=rig).stereo_frame([tr], 1.2 * j, j)
        cfgs.append(cfg), i0.append(a), i1.append(b)
    i0, i1 = torch.cat(i0).contiguous(), torch.cat(i1).contiguous()
    kps, desc, cnt, _ = w.ctx.orb_detect_and_compute(i0, cap=1024)
    both = [t.cpu().numpy() for t in w.ctx.lc_keyframe_landmarks_unrect(i0, i1, cfgs, kps, desc, cnt)]
    for j in range(2):
        s = slice(j, j + 1)
        one = [t.cpu().numpy() for t in w.ctx.lc_keyframe_landmarks_unrect(i0[s], i1[s], cfgs[j], kps[s], desc[s], cnt[s])]
        c = int(both[3][j])
        assert one[3][0] == c > 100, (j, c)
        assert np.array_equal(one[0][0], both[0][j]) and np.array_equal(one[1][0], both[1][j]) and np.array_equal(one[2][0, :c], both[2][j, :c]), j
        want = w.want(j, cam=U.cam_of(cfgs[j]), i0=i0, i1=i1, kps=kps, desc=desc, cnt=cnt)        # ... and it is that rig's result
        assert c == len(want["lm2"]) and np.array_equal(both[0][j, :c], want["lm2"]), j
    # image 1 with image 0's rig is another result: the rows are read per image
    s = slice(1, 2)
    wrong = w.ctx.lc_keyframe_landmarks_unrect(i0[s], i1[s], cfgs[0], kps[s], desc[s], cnt[s])[1].cpu().numpy()
    assert not np.array_equal(wrong[0], both[1][1])


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(world):
    import torch
    import flvis_amd
    w = world
    n, cap = 3, w.kps.shape[1]
    i0, i1, kps, desc, cnt = w.i0[:n], w.i1[:n], w.kps[:n], w.desc[:n], w.cnt[:n]
    copy = lambda: type(w.cfg).from_buffer_copy(w.cfg)
    rect, small = copy(), copy()
    rect.cam_type = 0
    small.image_width = 640
    for cfgs, code in (([rect], -5), ([w.cfg, rect, w.cfg], -5), ([small], -5), ([w.cfg, w.cfg, small], -5), ([w.cfg, w.cfg], -1), ([], -1)):
        out = sentinels(n, cap)
        with pytest.raises(flvis_amd.FlvisError) as e:
            w.ctx.lc_keyframe_landmarks_unrect(i0, i1, cfgs, kps, desc, cnt, out=out)
        assert "(%d)" % code in str(e.value), (code, str(e.value))
        assert untouched(out)
    # cap > 2048: FLVIS_ERR_CAPACITY
    big = 2049
    out = sentinels(1, big)
    with pytest.raises(flvis_amd.FlvisError) as e:
        w.ctx.lc_keyframe_landmarks_unrect(i0[:1], i1[:1], w.cfg, torch.zeros((1, big, 6), device="cuda"), torch.zeros((1, big, 32), dtype=torch.uint8, device="cuda"),
                                           cnt[:1], out=out)
    assert "(-4)" in str(e.value) and untouched(out)
    # null pointers: every device pointer in turn
    out = sentinels(n, cap)
    fn = w.ctx._lib.flvis_hip_lc_keyframe_landmarks_unrect
    ptrs = [t.data_ptr() for t in (i0.contiguous(), i1.contiguous(), kps.contiguous(), desc.contiguous(), cnt.contiguous()) + out]
    arr = (flvis_amd.FlvisCfg * 1)(w.cfg)
    for k in range(len(ptrs)):
        p = [C.c_void_p(0 if j == k else v) for j, v in enumerate(ptrs)]
        assert fn(w.ctx._h, p[0], p[1], U.W, U.H, n, arr, 1, p[2], p[3], p[4], cap, p[5], p[6], p[7], p[8]) == flvis_amd.FLVIS_ERR_INVALID_ARG, k
    assert fn(w.ctx._h, *[C.c_void_p(v) for v in ptrs[:2]], U.W, U.H, n, None, 1, *[C.c_void_p(v) for v in ptrs[2:5]], cap,
              *[C.c_void_p(v) for v in ptrs[5:]]) == flvis_amd.FLVIS_ERR_INVALID_ARG
    w.ctx.synchronize()
    assert untouched(out)


# ---- 4. / 5. the closer's switch ------------------------------------------------------------------------------------------------
def test_closer_switch_off_is_the_reference_s_empty_case(world):
    import flvis_amd
    w = world
    w.tours()
    lc = flvis_amd.LoopCloser(w.ctx, w.cfg, LC.LC_PARAMS, n_streams=1, max_keyframes=4)
    lc.add_keyframes([0], w.i0[0:1], w.i1[0:1], [IDENT])
    lc.process()
    kf = lc.keyframe(0, 0)
    assert len(kf["lm2"]) == 0 and len(kf["lm3"]) == 0 and len(kf["lmd"]) == 0 and len(kf["bow"][0]) > 20
    fix = lc.localize([0], w.i0[4:5], w.i1[4:5])[0]
    assert fix["n_landmarks"] == 0 and fix["best"] == -1
    lc.close()


def test_closer_switch_on_stores_the_kernel_level_call_s_landmarks(world):
    import torch
    import flvis_amd
    from flvis_amd import synth
    w = world
    w.tours()
    units = [w.variant[1], w.variant[2]]
    cfgs = [c for _, c in units]
    rnd = [synth.Renderer("cuda", rig=r) for r, _ in units]
    trs = [LC.LoopTrajectory(phase=0.0), LC.LoopTrajectory(phase=2.0)]
    frames = []
    for i, t in enumerate(LC.keyframe_times(4, PER)):
        fr = [rnd[s].stereo_frame([trs[s]], t, i) for s in range(2)]
        frames.append((torch.cat([f[0] for f in fr]).contiguous(), torch.cat([f[1] for f in fr]).contiguous()))
    lc = flvis_amd.LoopCloser(w.ctx, cfgs, LC.LC_PARAMS, max_keyframes=8)
    lc.set_stereo_unrect(True)
    lc.set_stereo_unrect(False)                  # ... both ways while the database is empty
    lc.set_stereo_unrect(True)
    for i0, i1 in frames:
        lc.add_keyframes([0, 1], i0, i1, np.array([IDENT] * 2))
        lc.process()
    for i in (0, 3):
        feat = w.features(frames[i][0], frames[i][1], cfgs)
        for s in range(2):
            kf = lc.keyframe(s, i)
            assert len(kf["lm2"]) == len(feat[s]["lm2"]) > 100, (i, s, len(kf["lm2"]))
            assert all(np.array_equal(kf[k], feat[s][k]) for k in ("lm2", "lm3", "lmd")), (i, s)
            assert np.array_equal(kf["bow"][0], feat[s]["bow"][0]) and np.array_equal(kf["bow"][1], feat[s]["bow"][1])
    # sequence 1 with sequence 0's rig is another result: the device table's rows are read per sequence
    wrong = w.features(frames[3][0][1:2], frames[3][1][1:2], cfgs[0])[0]
    assert not np.array_equal(wrong["lm3"], lc.keyframe(1, 3)["lm3"])
    # the switch belongs to the whole database
    for v in (False, True):
        with pytest.raises(flvis_amd.FlvisError) as e:
            lc.set_stereo_unrect(v)
        assert "(-1)" in str(e.value)
    lc.reset([0])
    with pytest.raises(flvis_amd.FlvisError):    # sequence 1 still holds keyframes
        lc.set_stereo_unrect(False)
    assert len(lc.keyframe(1, 3)["lm2"]) == len(w.features(frames[3][0], frames[3][1], cfgs)[1]["lm2"])
    lc.reset([1])
    lc.set_stereo_unrect(False)                  # allowed again once every sequence has been reset
    lc.add_keyframes([0], frames[0][0][0:1], frames[0][1][0:1], [IDENT])
    assert len(lc.keyframe(0, 0)["lm2"]) == 0
    lc.close()
    # a rectified-stereo closer has no such switch
    p = os.path.join(tempfile.gettempdir(), "flvis_lc_unrect_d435_%d.yaml" % os.getpid())
    open(p, "w").write(synth.D435I_STEREO_YAML)
    d435 = flvis_amd.LoopCloser(w.ctx, flvis_amd.load_config(p), LC.LC_PARAMS, n_streams=1, max_keyframes=2)
    os.remove(p)
    for v in (True, False):
        with pytest.raises(flvis_amd.FlvisError) as e:
            d435.set_stereo_unrect(v)
        assert "(-5)" in str(e.value)
    d435.close()


# ---- 6. a loop closes -----------------------------------------------------------------------------------------------------------
def test_a_loop_closes_on_the_unrectified_rig(world):
    """62 keyframes of two tours that come back to their start, odometry drifting in the RECTIFIED camera frame: the product's events,
    similarity rows and PnP poses equal the oracle chain fed the device's features, poses and drift within 1e-7, and the translation gap
    PS.loop_gap(., ., 2, n - 1) after closing is below 0.5 of the odometry's -- first on the reference chain's own poses."""
    import flvis_amd
    w = world
    frames, gt = w.tours()
    odom = [LC.drifted_odometry(gt[s], 10 + s, sigma_t=0.02, sigma_r=0.004) for s in range(2)]
    K4 = U.K4_of(w.cfg)
    lc = flvis_amd.LoopCloser(w.ctx, w.cfg, LC.LC_PARAMS, n_streams=2, max_keyframes=MAXKF)
    lc.set_stereo_unrect(True)
    ref = [LC.RefLoopCloser(K4, stream=s) for s in range(2)]
    log = [[], []]
    for i in range(N_KF):
        i0, i1 = frames[i]
        T = np.array([odom[s][i] for s in range(2)])
        assert lc.add_keyframes([0, 1], i0, i1, T).tolist() == [i, i]
        feat = w.features(i0, i1, w.cfg)
        ev = lc.process()
        for s in range(2):
            ref[s].add(feat[s], T[s])
            if i % 20 == 3:
                kf = lc.keyframe(s, i)
                assert all(np.array_equal(kf[k], feat[s][k]) for k in ("lm2", "lm3", "lmd")) and len(kf["lm2"]) > 100, (i, s)
            want, got = ref[s].process(), ev[s]
            assert np.array_equal(lc.similarity_row(s), ref[s].rows[-1]), (i, s)
            for key in ("kf_curr", "kf_prev", "candidate", "n_matches", "n_inliers", "accepted", "optimised"):
                assert got[key] == want[key], (i, s, key, got, want)
            if want["pose"] is not None:
                assert np.array_equal(np.array(got["pose"]), want["pose"]), (i, s)
            log[s].append(want)
            Tg, Tw = lc.poses(s), np.array(ref[s].T_c_w)
            assert Tg.shape == Tw.shape and np.abs(Tg - Tw).max() < 1e-7, (i, s, np.abs(Tg - Tw).max())
            assert np.abs(lc.drift(s) - ref[s].T_odom_map).max() < 1e-7
    for s in range(2):
        n = N_KF
        closing = [e for e in log[s] if e["accepted"] and e["kf_curr"] - e["kf_prev"] >= 40]
        g, od = np.array(gt[s]), np.array(odom[s])
        gap0 = PS.loop_gap(od, g, 2, n - 1)
        gap_ref = PS.loop_gap(np.array(ref[s].T_c_w), g, 2, n - 1)
        gap1 = PS.loop_gap(lc.poses(s), g, 2, n - 1)
        print("sequence %d: %d closing loops, translation gap %.4f m (odometry) -> %.4f m (reference chain, ratio %.3f), %.4f m (device, ratio %.3f)"
              % (s, len(closing), gap0[0], gap_ref[0], gap_ref[0] / gap0[0], gap1[0], gap1[0] / gap0[0]))
        assert len(closing) >= 2 and any(e["optimised"] for e in log[s]), (s, [(e["kf_prev"], e["kf_curr"]) for e in log[s] if e["accepted"]])
        assert gap_ref[0] < 0.5 * gap0[0], (s, gap0, gap_ref)            # the input first: the reference chain closes the loop
        assert gap1[0] < 0.5 * gap0[0], (s, gap0, gap1)
    lc.close()


# ---- 7. localize, reset_rigs --------------------------------------------------------------------------------------------------
def test_localize_and_reset_onto_another_unit(world):
    import flvis_amd
    from flvis_amd import synth
    w = world
    frames, gt = w.tours()
    lc = flvis_amd.LoopCloser(w.ctx, w.cfg, LL.PARAMS, n_streams=2, max_keyframes=9)
    lc.set_stereo_unrect(True)
    ref = LC.RefLoopCloser(U.K4_of(w.cfg), prm=LL.PARAMS, stream=0)
    for i in range(9):
        lc.add_keyframes([0], frames[i][0][0:1], frames[i][1][0:1], [gt[0][i]])
        ref.add(w.features(frames[i][0][0:1], frames[i][1][0:1], w.cfg)[0], gt[0][i])
        lc.process()
    # frame 50 of the tour is keyframe 0's pose one period later (another noise draw)
    q0, q1 = frames[PER][0][0:1], frames[PER][1][0:1]
    got = lc.localize([0], q0, q1, n_best=4)[0]
    want = LL.ref_localize(ref, w.features(q0, q1, w.cfg)[0], 4)
    assert want["best"] >= 0 and want["n_landmarks"] > 100, want
    LL.same_fix(got, want)
    assert got["best"] >= 0
    et, ea = LL.pose_error(got["T_c_map"], gt[0][PER])
    print("localize at the revisited pose: keyframe %d, %d inliers, %.4f m and %.3f deg from the truth (rectified frame)"
          % (got["kf"], got["candidates"][got["best"]]["n_inliers"], et, np.degrees(ea)))
    into = lc.localize_in([1], [0], q0, q1, n_best=4)[0]          # the same query from the other (empty) sequence, with ITS row of the table
    assert into["best"] >= 0 and into["map"] == 0 and into["n_landmarks"] == got["n_landmarks"]
    # sequence 0 changes to another unit: three keyframes, bit for bit sequence 0 of a new closer on that config
    rig, other = w.variant[1]
    rnd = synth.Renderer("cuda", rig=rig)
    tr = LC.LoopTrajectory(phase=2.6)
    lc.reset([0], [other])
    fresh = flvis_amd.LoopCloser(w.ctx, other, LL.PARAMS, n_streams=1, max_keyframes=9)
    fresh.set_stereo_unrect(True)
    for i, t in enumerate(LC.keyframe_times(3, PER)):
        a, b = rnd.stereo_frame([tr], t, i)
        assert lc.add_keyframes([0], a, b, [IDENT]).tolist() == fresh.add_keyframes([0], a, b, [IDENT]).tolist() == [i]
        e1, e2 = lc.process(), fresh.process()
        assert e1[0] == e2[0]
        k1, k2 = lc.keyframe(0, i), fresh.keyframe(0, i)
        assert len(k1["lm2"]) > 100 and all(np.array_equal(k1[k], k2[k]) for k in ("lm2", "lm3", "lmd"))
        assert np.array_equal(k1["bow"][0], k2["bow"][0]) and np.array_equal(k1["bow"][1], k2["bow"][1])
        assert np.array_equal(lc.similarity_row(0), fresh.similarity_row(0))
        f = w.features(a, b, other)[0]
        assert np.array_equal(k1["lm3"], f["lm3"]) and not np.array_equal(k1["lm3"], w.features(a, b, w.cfg)[0]["lm3"])
    lc.close(), fresh.close()
