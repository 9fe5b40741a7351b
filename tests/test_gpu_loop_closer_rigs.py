"""GPU: the loop closer on a fleet -- one calibrated camera per sequence (flvis_loop_closer_create_rigs, with the two kernel-level
entry points that take a camera per set / per image underneath) and a slot that starts over, also on another camera
(flvis_loop_closer_reset[_rigs]).  Checked against the CPU oracle chain of tests/_loop_chain.py run with each sequence's own
intrinsics, against one-sequence closers (a sequence of a fleet is bit for bit the sequence alone) and against twins that were
never reset.

The cameras are synth.rig_variant's units of the D435i: fx / fy up to 4 % and cx / cy up to 8 px away from the stock calibration,
which a geometric check with a 2.0 px threshold cannot absorb -- every test asserts that on its own data."""
import os
import tempfile

import numpy as np
import pytest

import _geom as G
import _loop_chain as LC
import _oracle as O
import _voc as V

pytestmark = pytest.mark.gpu

# the units of the mixed fleet: the stock calibration and two of synth.rig_variant("d435i_stereo", k), k = 1..8 -- chosen on the GPU as
# the first two on which the oracle chain closes a loop over >= 40 keyframes on this tour (profiles/r10_loop_closer_rigs.md)
FLEET = (0, 1, 2)
OTHER = 3            # the unit that takes over slot 1 in the reset-onto-another-rig test
N_KF, PER, MAXKF = 62, 50, 64
PHASES = (0.0, 0.9, 1.8)
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
EV_KEYS = ("kf_curr", "kf_prev", "candidate", "n_matches", "n_inliers", "accepted", "optimised", "pgo_iterations", "pose", "chi2_before",
           "chi2_after")


def load_variant(kind, k):
    import flvis_amd
    from flvis_amd import synth
    rig, text = synth.rig_variant(kind, k)
    p = os.path.join(tempfile.gettempdir(), "flvis_lc_rigs_%s_%d.yaml" % (kind, k))
    open(p, "w").write(text)
    return rig, flvis_amd.load_config(p)


def K4_of(cfg):
    return np.array([cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6]])


def cfg_bytes(cfg):
    import ctypes as C
    return C.string_at(C.addressof(cfg), C.sizeof(cfg))


class Sequence:
    """one camera's tour: its keyframes' images on the device and its drifting odometry"""

    def __init__(self, rnd, phase, seed, n=N_KF):
        tr = LC.LoopTrajectory(phase=phase)
        times = LC.keyframe_times(n, PER)
        fr = [rnd.stereo_frame([tr], t, i) for i, t in enumerate(times)]
        self.img0, self.img1 = [f[0] for f in fr], [f[1] for f in fr]
        gt = [G.pose7(*tr.T_c_w(t, rnd.rig)) for t in times]
        self.odom = LC.drifted_odometry(gt, seed, sigma_t=0.008, sigma_r=0.002)


class Fleet:
    """what the long tests share: the context with its vocabulary, the units' rigs / configs / renderers, the fleet's three tours and
    the two tours that take over slot 1.  Nothing here is changed by a test."""

    def __init__(self):
        import flvis_amd
        from flvis_amd import synth
        self.ctx = flvis_amd.Context(0)
        self.cfg, self.rnd = {}, {}
        for k in FLEET + (OTHER,):
            rig, self.cfg[k] = load_variant("d435i_stereo", k)
            self.rnd[k] = synth.Renderer("cuda", rig=rig)
        self.seq = [Sequence(self.rnd[k], PHASES[s], 10 + s) for s, k in enumerate(FLEET)]
        self.takeover_same = Sequence(self.rnd[FLEET[1]], 2.6, 20)     # slot 1's next tour on its own unit ...
        self.takeover_other = Sequence(self.rnd[OTHER], 2.6, 21)      # ... and on another one
        train = []
        for i in range(0, N_KF, 6):     # vocabulary from the device's descriptors of every sixth keyframe of sequence 0
            k, d, c, _ = self.ctx.orb_detect_and_compute(self.seq[0].img0[i], cap=1024)
            train.append(d[0, :int(c[0])].cpu().numpy())
        self.ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))
        self.cfgs = [self.cfg[k] for k in FLEET]


@pytest.fixture(scope="module")
def fleet():
    f = Fleet()
    yield f
    f.ctx.close()


def feed(lc, items):
    """items: [(stream, Sequence, index)] -> one add_keyframes + process; returns (ids, events)"""
    import torch
    i0 = torch.cat([q.img0[i] for _, q, i in items]).contiguous()
    i1 = torch.cat([q.img1[i] for _, q, i in items]).contiguous()
    ids = lc.add_keyframes([s for s, _, _ in items], i0, i1, np.array([q.odom[i] for _, q, i in items]))
    return ids.tolist(), lc.process()


def state(lc, s, ev):
    """everything a caller can see of sequence s after a call, as comparable values"""
    return dict(ev={k: ev[s][k] for k in EV_KEYS}, row=lc.similarity_row(s).tobytes(), poses=lc.poses(s).tobytes(), drift=lc.drift(s).tobytes())


def same_keyframe(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("lm2", "lm3", "lmd")) and all(np.array_equal(x, y) for x, y in zip(a["bow"], b["bow"]))


# ---- 1. PnP, a camera per set ---------------------------------------------------------------------------------------------------
def test_pnp_ransac_a_camera_per_set():
    """flvis_hip_pnp_ransac_rigs: every set with its own K equals the oracle's solvePnPRansac with that K and the single-K entry point on
    that set alone, bit for bit; with equal rows the batch equals the single-K entry point on the batch"""
    import torch
    import flvis_amd
    ctx = flvis_amd.Context(0)
    rng = np.random.default_rng(8)
    cap, sets, Ks = 700, [], []
    for n, outl in ((650, 0.3), (120, 0.1), (40, 0.5), (3, 0.0), (0, 0.0), (700, 0.6), (4, 0.0)):
        K4 = np.array([384.0 * (1 + rng.uniform(-0.04, 0.04)), 385.0 * (1 + rng.uniform(-0.04, 0.04)), 320.0 + rng.uniform(-8, 8),
                       240.0 + rng.uniform(-8, 8)])
        R = G.rodrigues(rng.normal(0, 0.3, 3))
        t = rng.normal(0, 0.5, 3)
        P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2, 8, n)], 1)
        X = P @ R.T + t
        uv = np.stack([K4[0] * X[:, 0] / X[:, 2] + K4[2], K4[1] * X[:, 1] / X[:, 2] + K4[3]], 1) + rng.normal(0, 0.4, (n, 2))
        bad = rng.random(n) < outl
        uv[bad] = np.stack([rng.uniform(0, 640, bad.sum()), rng.uniform(0, 480, bad.sum())], 1)
        sets.append((P.astype(np.float32), uv.astype(np.float32)))
        Ks.append(K4)
    Ks = np.array(Ks)
    p3 = np.zeros((len(sets), cap, 3), np.float32)
    p2 = np.zeros((len(sets), cap, 2), np.float32)
    cnt = np.zeros(len(sets), np.int32)
    for k, (P, uv) in enumerate(sets):
        p3[k, :len(P)], p2[k, :len(P)], cnt[k] = P, uv, len(P)
    seeds = np.array([0x1234 + 77 * k for k in range(len(sets))], np.uint64)
    d3, d2, dc = torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda(), torch.from_numpy(cnt).cuda()
    pose, mask, ninl = [t.cpu().numpy() for t in ctx.pnp_ransac(d3, d2, dc, Ks, seeds)]
    own, with_k0 = [], []
    for k, (P, uv) in enumerate(sets):
        n_want, pose_want, mask_want = O.solve_pnp_ransac(P, uv, Ks[k], iterative=False, iterations=100, reproj=2.0, conf=0.99, seed=int(seeds[k]))
        assert ninl[k] == n_want, (k, ninl[k], n_want)
        assert np.array_equal(mask[k, :len(P)], mask_want) and not mask[k, len(P):].any(), k
        assert np.array_equal(pose[k], pose_want), (k, pose[k] - pose_want)
        one = [t.cpu().numpy() for t in ctx.pnp_ransac(d3[k:k + 1], d2[k:k + 1], dc[k:k + 1], Ks[k], seeds[k:k + 1])]
        assert np.array_equal(one[0][0], pose[k]) and np.array_equal(one[1][0], mask[k]) and one[2][0] == ninl[k], k
        own.append(n_want)
        with_k0.append(O.solve_pnp_ransac(P, uv, Ks[0], iterative=False, iterations=100, reproj=2.0, conf=0.99, seed=int(seeds[k]))[0])
    assert any(a != b for a, b in zip(own[1:], with_k0[1:])), (own, with_k0)      # another camera's K is not good enough: the rows matter
    assert ninl[3] == 0 and ninl[4] == 0 and own[0] > 300
    rows = np.tile(Ks[2], (len(sets), 1))
    a = [t.cpu().numpy() for t in ctx.pnp_ransac(d3, d2, dc, rows, seeds)]
    b = [t.cpu().numpy() for t in ctx.pnp_ransac(d3, d2, dc, Ks[2], seeds)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ctx.close()


# ---- 2. landmarks, a camera per image ---------------------------------------------------------------------------------------------
def test_keyframe_landmarks_a_camera_per_image():
    """flvis_hip_lc_keyframe_landmarks_rigs, stereo (P0 / P1 per image) and depth (K4 per image): image i equals the single-camera call on
    image i alone bit for bit, also in place and for one image"""
    import torch
    import flvis_amd
    from flvis_amd import synth
    ctx = flvis_amd.Context(0)
    tr = LC.LoopTrajectory(phase=0.4)

    def check(kind, variants, cam_type, render):
        cfgs, i0, i1 = [], [], []
        for j, k in enumerate(variants):
            rig, cfg = load_variant(kind, k)
            a, b = render(synth.Renderer("cuda", rig=rig), 1.2 * j, j)
            cfgs.append(cfg), i0.append(a), i1.append(b)
        i0, i1 = torch.cat(i0).contiguous(), torch.cat(i1).contiguous()
        n = len(variants)
        kps, desc, cnt, _ = ctx.orb_detect_and_compute(i0, cap=1024)
        P0, P1 = np.array([list(c.P0) for c in cfgs]), np.array([list(c.P1) for c in cfgs])
        K4 = np.array([K4_of(c) for c in cfgs])
        cam = (lambda s: dict(P0=P0[s], P1=P1[s])) if cam_type == 0 else (lambda s: dict(K4=K4[s]))
        img0 = (lambda s: i0[s]) if cam_type == 0 else (lambda s: None)
        lm2, lm3, lmd, lmc = [t.cpu().numpy() for t in ctx.lc_keyframe_landmarks(img0(slice(None)), i1, cam_type, kps, desc, cnt, **cam(slice(None)))]
        for j in range(n):
            s = slice(j, j + 1)
            one = [t.cpu().numpy() for t in ctx.lc_keyframe_landmarks(img0(s), i1[s], cam_type, kps[s], desc[s], cnt[s], **cam(j))]
            c = int(lmc[j])
            assert one[3][0] == c > 50, (kind, j, c)
            assert np.array_equal(one[0][0], lm2[j]) and np.array_equal(one[1][0], lm3[j]) and np.array_equal(one[2][0, :c], lmd[j, :c]), (kind, j)
            # n_img = 1 through the per-image entry point ([1,12] / [1,4] rows)
            rig1 = [t.cpu().numpy() for t in ctx.lc_keyframe_landmarks(img0(s), i1[s], cam_type, kps[s], desc[s], cnt[s], **cam(s))]
            assert all(np.array_equal(x, y) for x, y in zip(rig1, one)), (kind, j)
        # in place: the compacted descriptors overwrite the ORB descriptors
        d2 = desc.clone()
        ip = ctx.lc_keyframe_landmarks(img0(slice(None)), i1, cam_type, kps, d2, cnt, in_place=True, **cam(slice(None)))
        assert ip[2].data_ptr() == d2.data_ptr()
        assert np.array_equal(ip[0].cpu().numpy(), lm2) and np.array_equal(ip[1].cpu().numpy(), lm3) and np.array_equal(ip[3].cpu().numpy(), lmc)
        for j in range(n):
            assert np.array_equal(d2[j, :int(lmc[j])].cpu().numpy(), lmd[j, :int(lmc[j])])
        # image 1 with image 0's camera is another result: the rows are read per image
        s = slice(1, 2)
        wrong = ctx.lc_keyframe_landmarks(img0(s), i1[s], cam_type, kps[s], desc[s], cnt[s], **cam(0))[1].cpu().numpy()
        assert not np.array_equal(wrong[0], lm3[1])

    check("d435i_stereo", (0, 1, 2), 0, lambda rnd, t, j: rnd.stereo_frame([tr], t, j))
    check("d435i_depth", (0, 1), 2, lambda rnd, t, j: rnd.depth_frame([tr], t, j))        # (depth_frame's default factor: 1000)
    ctx.close()


# ---- 3. a mixed fleet against the oracle chain -------------------------------------------------------------------------------------
def test_mixed_fleet_against_the_oracle_chain(fleet):
    """three sequences on three units in one closer: each equals the oracle chain run with ITS intrinsics on the device's features
    (computed with ITS P0 / P1), and a one-sequence closer on its config bit for bit"""
    import flvis_amd
    ctx, cfgs = fleet.ctx, fleet.cfgs
    lc = flvis_amd.LoopCloser(ctx, cfgs, LC.LC_PARAMS, max_keyframes=MAXKF)
    assert lc.n_streams == 3
    solo = [flvis_amd.LoopCloser(ctx, cfgs[s], LC.LC_PARAMS, n_streams=1, max_keyframes=MAXKF) for s in range(3)]
    ref = [LC.RefLoopCloser(K4_of(cfgs[s]), stream=s) for s in range(3)]
    shadow = {s: LC.RefLoopCloser(K4_of(cfgs[0]), stream=s) for s in (1, 2)}     # the same chain with unit 0's K: must NOT agree
    k0_differs = False
    n_added = [0, 0, 0]
    log = [[], [], []]
    for i in range(N_KF):
        streams = [0, 1] if i % 9 == 4 else [0, 1, 2]       # sequence 2 misses every ninth call
        items = [(s, fleet.seq[s], n_added[s]) for s in streams]
        ids, ev = feed(lc, items)
        assert ids == [n_added[s] for s in streams]
        for j, (s, q, k) in enumerate(items):
            # the same keyframe through the separate entry points with the sequence's own camera, for the oracle chain
            kps, desc, cnt, _ = ctx.orb_detect_and_compute(q.img0[k], cap=1024)
            bi, bv, bn = [t.cpu().numpy() for t in ctx.bow_transform(desc, cnt, vcap=1024)]
            lm2, lm3, lmd, lmc = [t.cpu().numpy() for t in ctx.lc_keyframe_landmarks(q.img0[k], q.img1[k], 0, kps, desc, cnt, P0=list(cfgs[s].P0),
                                                                                      P1=list(cfgs[s].P1))]
            f = dict(bow=(bi[0, :bn[0]].copy(), bv[0, :bn[0]].copy()), lm2=lm2[0, :lmc[0]].copy(), lm3=lm3[0, :lmc[0]].copy(),
                     lmd=lmd[0, :lmc[0]].copy())
            ref[s].add(f, q.odom[k])
            if s in shadow:
                shadow[s].add(f, q.odom[k])
            n_added[s] += 1
            if i % 20 == 3:
                assert same_keyframe(lc.keyframe(s, k), f), (i, s)
            want, got = ref[s].process(), ev[s]
            row = lc.similarity_row(s)
            assert np.array_equal(row, ref[s].rows[-1]), (i, s)
            for key in ("kf_curr", "kf_prev", "candidate", "n_matches", "n_inliers", "accepted", "optimised"):
                assert got[key] == want[key], (i, s, key, got, want)
            if want["pose"] is not None:
                assert np.array_equal(np.array(got["pose"]), want["pose"]), (i, s)
            if s in shadow and n_added[s] >= 50:        # (nothing reads K before the reference's own gate, :453)
                other = shadow[s].process()
                if want["pose"] is not None and other["pose"] is not None:
                    if other["kf_prev"] == want["kf_prev"]:
                        k0_differs |= other["n_inliers"] != want["n_inliers"] or not np.array_equal(other["pose"], want["pose"])
                    del shadow[s]                       # its history is the stream's only up to its first verified candidate
            log[s].append(want)
            Tg, Tw = lc.poses(s), np.array(ref[s].T_c_w)
            assert Tg.shape == Tw.shape and np.abs(Tg - Tw).max() < 1e-7, (i, s, np.abs(Tg - Tw).max())
            assert np.abs(lc.drift(s) - ref[s].T_odom_map).max() < 1e-7
            # ... and the sequence alone in a closer of its own
            ids1, ev1 = feed(solo[s], [(0, q, k)])
            assert ids1 == [k] and state(solo[s], 0, ev1) == state(lc, s, ev), (i, s)
        for s in range(3):
            if s not in streams:
                assert ev[s]["kf_curr"] == -1 and not ev[s]["candidate"]
    # on the reference chain's own log: a loop over >= 40 keyframes on every stream, a pose graph on one, and unit 0's K told apart
    for s in range(3):
        assert any(e["accepted"] and e["kf_curr"] - e["kf_prev"] >= 40 for e in log[s]), (s, [(e["kf_prev"], e["kf_curr"]) for e in log[s] if e["accepted"]])
    assert any(e["optimised"] for s in range(3) for e in log[s])
    assert k0_differs
    for c in solo + [lc]:
        c.close()


# ---- 4. depth fleet ---------------------------------------------------------------------------------------------------------------
def test_depth_fleet_uses_each_slot_s_intrinsics():
    import torch
    import flvis_amd
    from flvis_amd import synth
    ctx = flvis_amd.Context(0)
    rigs_cfgs = [load_variant("d435i_depth", k) for k in (0, 1)]
    cfgs = [c for _, c in rigs_cfgs]
    assert all(c.cam_type == 2 for c in cfgs)
    rnd = [synth.Renderer("cuda", rig=r) for r, _ in rigs_cfgs]
    trs = [LC.LoopTrajectory(phase=0.0), LC.LoopTrajectory(phase=2.0)]
    frames = []
    for i, t in enumerate(LC.keyframe_times(4, 50)):
        fr = [rnd[s].depth_frame([trs[s]], t, i) for s in range(2)]
        frames.append((torch.cat([f[0] for f in fr]).contiguous(), torch.cat([f[1] for f in fr]).contiguous()))
    train = []
    for i0, _ in frames:
        k, d, c, _ = ctx.orb_detect_and_compute(i0, cap=1024)
        train += [d[s, :int(c[s])].cpu().numpy() for s in range(2)]
    ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=6, depth=3))
    lc = flvis_amd.LoopCloser(ctx, cfgs, LC.LC_PARAMS, max_keyframes=8)
    for i0, d16 in frames:
        lc.add_keyframes([0, 1], i0, d16, np.array([IDENT] * 2))
        lc.process()
    kps, desc, cnt, _ = ctx.orb_detect_and_compute(frames[3][0], cap=1024)
    K4 = np.array([K4_of(c) for c in cfgs])
    lm2, lm3, lmd, lmc = [t.cpu().numpy() for t in ctx.lc_keyframe_landmarks(None, frames[3][1], 2, kps, desc, cnt, K4=K4)]
    for s in range(2):
        kf = lc.keyframe(s, 3)
        assert len(kf["lm2"]) == lmc[s] > 50
        assert np.array_equal(kf["lm2"], lm2[s, :lmc[s]]) and np.array_equal(kf["lm3"], lm3[s, :lmc[s]]) and np.array_equal(kf["lmd"], lmd[s, :lmc[s]])
    wrong = ctx.lc_keyframe_landmarks(None, frames[3][1][1:2], 2, kps[1:2], desc[1:2], cnt[1:2], K4=K4[0])[1].cpu().numpy()
    assert not np.array_equal(wrong[0, :lmc[1]], lc.keyframe(1, 3)["lm3"])
    lc.close()
    ctx.close()


# ---- 5. / 6. reset equals fresh, the others undisturbed ---------------------------------------------------------------------------
def run_reset(fleet, takeover, new_cfg):
    """the fleet for N_KF calls; slot 1 reset (onto new_cfg if given); slot 1 on its next tour for N_KF calls beside a fresh
    one-sequence closer, slots 0 and 2 going on beside a twin closer that is never reset until their capacity ends"""
    import flvis_amd
    ctx, cfgs = fleet.ctx, fleet.cfgs
    lc = flvis_amd.LoopCloser(ctx, cfgs, LC.LC_PARAMS, max_keyframes=MAXKF)
    twin = flvis_amd.LoopCloser(ctx, cfgs, LC.LC_PARAMS, max_keyframes=MAXKF)
    seen = dict(accepted=False, optimised=False)
    for i in range(N_KF):
        items = [(s, fleet.seq[s], i) for s in range(3)]
        (_, ev), (_, ev2) = feed(lc, items), feed(twin, items)
        assert all(state(lc, s, ev) == state(twin, s, ev2) for s in range(3))
        seen["accepted"] |= ev[1]["accepted"]
        seen["optimised"] |= ev[1]["optimised"]
    # what could leak: slot 1 has closed a loop, optimised its pose graph and carries a drift correction
    assert seen["accepted"] and seen["optimised"] and not np.array_equal(lc.drift(1), IDENT)
    assert len(lc.poses(1)) == N_KF
    if new_cfg is None:
        lc.reset([1])
    else:
        lc.reset([1], [new_cfg])
    assert len(lc.poses(1)) == 0 and len(lc.similarity_row(1)) == 0 and np.array_equal(lc.drift(1), IDENT)
    with pytest.raises(flvis_amd.FlvisError):
        lc.keyframe(1, 0)
    fresh = flvis_amd.LoopCloser(ctx, cfgs[1] if new_cfg is None else new_cfg, LC.LC_PARAMS, n_streams=1, max_keyframes=MAXKF)
    again = dict(accepted=False, optimised=False)
    for i in range(N_KF):       # N_KF more keyframes in a slot of MAXKF: refused without the reset
        k = N_KF + i
        going = k < MAXKF       # slots 0 and 2 go on until their own capacity ends; their tours repeat a keyframe, which is as good as any
        items = [(1, takeover, i)] + ([(0, fleet.seq[0], i), (2, fleet.seq[2], i)] if going else [])
        ids, ev = feed(lc, items)
        ids1, ev1 = feed(fresh, [(0, takeover, i)])
        assert ids[0] == ids1[0] == i
        assert state(lc, 1, ev) == state(fresh, 0, ev1), i
        if i % 10 == 1 or i == N_KF - 1:
            assert same_keyframe(lc.keyframe(1, i), fresh.keyframe(0, i)), i
        again["accepted"] |= ev[1]["accepted"]
        again["optimised"] |= ev[1]["optimised"]
        if going:
            ids2, ev2 = feed(twin, items[1:])
            assert ids[1:] == ids2 == [k, k]
            assert all(state(lc, s, ev) == state(twin, s, ev2) for s in (0, 2)), i
            assert same_keyframe(lc.keyframe(2, k), twin.keyframe(2, k))
        else:
            assert ev[0]["kf_curr"] == ev[2]["kf_curr"] == -1
    assert again["accepted"] and again["optimised"]             # the new sequence went through the whole chain as well
    for s in (0, 2):
        assert lc.poses(s).tobytes() == twin.poses(s).tobytes() and len(lc.poses(s)) == MAXKF
    with pytest.raises(flvis_amd.FlvisError) as e:              # ... which is where slots 0 and 2 end
        feed(lc, [(0, fleet.seq[0], 0)])
    assert "capacity" in str(e.value)
    out = lc
    twin.close(), fresh.close()
    return out


def test_reset_equals_a_fresh_closer_and_leaves_the_others_alone(fleet):
    import flvis_amd
    lc = run_reset(fleet, fleet.takeover_same, None)
    assert cfg_bytes(lc.stream_cfg(1)) == cfg_bytes(fleet.cfgs[1])
    lc.close()
    # a keyframe that was added and not processed goes with the reset
    q = fleet.seq[0]
    lc = flvis_amd.LoopCloser(fleet.ctx, fleet.cfgs, LC.LC_PARAMS, max_keyframes=MAXKF)
    feed(lc, [(0, q, 0), (1, fleet.seq[1], 0)])
    lc.add_keyframes([0], q.img0[1], q.img1[1], [q.odom[1]])
    lc.reset([0])
    ev = lc.process()
    assert ev[0]["kf_curr"] == -1 and ev[1]["kf_curr"] == -1
    assert len(lc.poses(0)) == 0 and len(lc.similarity_row(0)) == 0 and np.array_equal(lc.drift(0), IDENT)
    with pytest.raises(flvis_amd.FlvisError):
        lc.keyframe(0, 0)
    assert len(lc.poses(1)) == 1
    ids, ev = feed(lc, [(0, q, 2)])
    assert ids == [0] and ev[0]["kf_curr"] == 0 and len(lc.similarity_row(0)) == 1 and abs(lc.similarity_row(0)[0] - 1.0) < 1e-12
    lc.close()


def test_reset_onto_another_rig(fleet):
    other = fleet.cfg[OTHER]
    assert cfg_bytes(other) != cfg_bytes(fleet.cfgs[1])
    lc = run_reset(fleet, fleet.takeover_other, other)
    assert cfg_bytes(lc.stream_cfg(1)) == cfg_bytes(other)
    assert cfg_bytes(lc.stream_cfg(0)) == cfg_bytes(fleet.cfgs[0]) and cfg_bytes(lc.stream_cfg(2)) == cfg_bytes(fleet.cfgs[2])
    lc.close()


# ---- 7. refusals and identities ---------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_equal_configs_are_create(fleet):
    import flvis_amd
    ctx, cfgs = fleet.ctx, fleet.cfgs
    _, depth = load_variant("d435i_depth", 0)
    with pytest.raises(flvis_amd.FlvisError) as e:
        flvis_amd.LoopCloser(ctx, [cfgs[0], cfgs[1], depth], LC.LC_PARAMS, max_keyframes=4)
    assert "cam_type" in str(e.value) and "stream 2" in str(e.value)
    wide = type(cfgs[1]).from_buffer_copy(cfgs[1])
    wide.image_width = 848
    with pytest.raises(flvis_amd.FlvisError) as e:
        flvis_amd.LoopCloser(ctx, [cfgs[0], wide], LC.LC_PARAMS, max_keyframes=4)
    assert "image_width" in str(e.value) and "stream 1" in str(e.value)
    # refused resets: the closer goes on exactly as a twin that was never asked
    lc = flvis_amd.LoopCloser(ctx, cfgs, LC.LC_PARAMS, max_keyframes=8)
    twin = flvis_amd.LoopCloser(ctx, cfgs, LC.LC_PARAMS, max_keyframes=8)
    same = flvis_amd.LoopCloser(ctx, [cfgs[0]] * 3, LC.LC_PARAMS, max_keyframes=8)      # n equal configs ...
    plain = flvis_amd.LoopCloser(ctx, cfgs[0], LC.LC_PARAMS, n_streams=3, max_keyframes=8)  # ... are flvis_loop_closer_create
    items = lambda i: [(s, fleet.seq[s], i) for s in range(3)]
    feed(lc, items(0)), feed(twin, items(0))
    for bad in (([3], None), ([-1], None), ([1, 1], None), ([0, 3], [cfgs[0], cfgs[1]]), ([2, 2], [cfgs[1], cfgs[2]]), ([0, 1], [cfgs[1], depth]),
                ([1], [wide])):
        with pytest.raises(flvis_amd.FlvisError):
            lc.reset(*bad)
    for s in range(3):
        assert cfg_bytes(lc.stream_cfg(s)) == cfg_bytes(cfgs[s])
    for i in (1, 2, 3):
        (ids, ev), (ids2, ev2) = feed(lc, items(i)), feed(twin, items(i))
        assert ids == ids2 == [i] * 3
        for s in range(3):
            assert state(lc, s, ev) == state(twin, s, ev2) and same_keyframe(lc.keyframe(s, i), twin.keyframe(s, i)), (i, s)
    for i in range(3):
        one = [(s, fleet.seq[0], i) for s in range(3)]
        (ids, ev), (ids2, ev2) = feed(same, one), feed(plain, one)
        assert ids == ids2
        for s in range(3):
            assert state(same, s, ev) == state(plain, s, ev2) and same_keyframe(same.keyframe(s, i), plain.keyframe(s, i)), (i, s)
    lc.reset([])                                                    # nothing named: nothing happens
    assert len(lc.poses(0)) == 4
    for c in (lc, twin, same, plain):
        c.close()
