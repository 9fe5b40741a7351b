"""Test helper: relocalisation (flvis_loop_closer_localize) assembled from the CPU oracle's functions -- the chain that pins `process`
(tests/_loop_chain.py) around the candidate choice the product defines:

    candidates   the n_best keyframes with the highest ref_score against the query among those with score > 0 and >= minScore, by
                 score descending, equal scores by keyframe index ascending; no temporal exclusion, no 50-keyframe gate
    pair check   isLoopClosureKF (vo_loopclosing.cpp:593-686) on (database keyframe, query): O.orb_match, (3-D of the keyframe, pixel of
                 the query), O.solve_pnp_ransac in its P3P form, the acceptance rule of RefLoopCloser.process
    best         the accepted candidate with the most inliers (the earlier one on a tie); T_c_map = pose * T_c_w(keyframe)  (PS.mul7)

and the small scene the CPU and the GPU test share: a tour of 9 keyframes through the rendered room, queries between keyframes, rendered
on the CPU once per module (the GPU test uploads these very images)."""
import os
import tempfile

import numpy as np

import _geom as G
import _loop_chain as LC
import _oracle as O
import _pgo_synth as PS
from test_oracle_bow import RefVoc, ref_score

IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
N_KF, PER = 9, 50                      # keyframes every 1.2 s of the 60 s tour: neighbours overlap, the ends do not
# queries between keyframes (keyframe spacing 1.2 s): a third, a half, two thirds of the way to the next one
QUERY_TIMES = (0.4, 3.0, 5.6, 8.0)
# the small vocabulary (k = 6, depth 3: ~200 words) scores lower than the reference's 10^6 words do: minScore below every true neighbour
PARAMS = dict(LC.LC_PARAMS, minScore=0.02)


def pnp_seed(stream, rank):
    return ((stream + 1) << 32) + rank + 1


def ref_localize(ref, feat, n_best):
    """ref: LC.RefLoopCloser (its kfs / T_c_w / prm / K4 / stream), feat: the query's feature dict.  -> dict like LoopCloser.localize's"""
    p = ref.prm
    scores = [ref_score(feat["bow"], kf["bow"]) for kf in ref.kfs]
    order = sorted((j for j, s in enumerate(scores) if s > 0 and s >= p["minScore"]), key=lambda j: (-scores[j], j))[:n_best]
    cands, best = [], -1
    for r, j in enumerate(order):
        c = dict(kf=j, score=scores[j], n_matches=0, n_inliers=0, accepted=False, pose=IDENT.copy())
        cands.append(c)
        k0 = ref.kfs[j]
        if len(k0["lmd"]) == 0 or len(feat["lmd"]) == 0:
            continue
        pairs = np.array(O.orb_match(k0["lmd"], feat["lmd"], p["ratioMax"])).reshape(-1, 2)
        c["n_matches"] = len(pairs)
        if len(pairs) < 5:                                                      # :666
            continue
        p3d = k0["lm3"][pairs[:, 0]].astype(np.float32)
        p2d = feat["lm2"][pairs[:, 1]].astype(np.float32)
        ninl, pose, _ = O.solve_pnp_ransac(p3d, p2d, ref.K4, iterative=False, iterations=100, reproj=2.0, conf=0.99,
                                           seed=pnp_seed(ref.stream, r))
        c["n_inliers"], c["pose"] = int(ninl), pose
        if ninl * 1.0 / len(pairs) < p["ratioRansac"] or ninl < p["minPts"]:    # :677
            continue
        if not (np.linalg.norm(pose[:3]) < 3 and LC.so3_log_norm(pose[3:7]) < 1.5):  # :686
            continue
        c["accepted"] = True
        if best < 0 or c["n_inliers"] > cands[best]["n_inliers"]:
            best = r
    return dict(n_landmarks=len(feat["lmd"]), candidates=cands, best=best, kf=cands[best]["kf"] if best >= 0 else -1,
                T_c_map=PS.mul7(cands[best]["pose"], ref.T_c_w[cands[best]["kf"]]) if best >= 0 else None)


def same_fix(got, want, tol=1e-12):
    """a product result against the chain's: everything equal, T_c_map within tol (the host closer's pose-composition tolerance)"""
    assert got["n_landmarks"] == want["n_landmarks"], (got["n_landmarks"], want["n_landmarks"])
    assert len(got["candidates"]) == len(want["candidates"]), (got["candidates"], want["candidates"])
    for r, (a, b) in enumerate(zip(got["candidates"], want["candidates"])):
        for key in ("kf", "score", "n_matches", "n_inliers", "accepted"):
            assert a[key] == b[key], (r, key, a, b)
        assert np.array_equal(np.asarray(a["pose"]), np.asarray(b["pose"])), (r, a, b)
    assert got["best"] == want["best"] and got["kf"] == want["kf"], (got["best"], want["best"])
    if want["best"] >= 0:
        assert np.abs(np.asarray(got["T_c_map"]) - want["T_c_map"]).max() < tol
    else:
        assert got["T_c_map"] is None


def stereo_cfg():
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_loop_localize.yaml")
    open(p, "w").write(synth.D435I_STEREO_YAML)
    return flvis_amd.load_config(p)


def cam_of(cfg):
    P0, P1 = np.array(list(cfg.P0)), np.array(list(cfg.P1))
    return P0, P1, np.array([P0[0], P0[5], P0[2], P0[6]])


class Scene:
    """the tour: keyframe images kf[i] = (img0, img1) uint8 [480, 640] numpy, queries q[i], ground-truth T_c_w pose7 of both"""

    def __init__(self, phase=0.0, rig=None, n_kf=N_KF, query_times=QUERY_TIMES):
        from flvis_amd import synth
        tr = LC.LoopTrajectory(phase=phase)
        rnd = synth.Renderer("cpu", rig=rig)
        self.kf_times = LC.keyframe_times(n_kf, PER)
        self.q_times = list(query_times)
        pair = lambda t, i: tuple(x[0].numpy() for x in rnd.stereo_frame([tr], t, i))
        self.kf = [pair(t, i) for i, t in enumerate(self.kf_times)]
        self.q = [pair(t, 100 + i) for i, t in enumerate(self.q_times)]
        self.kf_gt = [G.pose7(*tr.T_c_w(t, rnd.rig)) for t in self.kf_times]
        self.q_gt = [G.pose7(*tr.T_c_w(t, rnd.rig)) for t in self.q_times]


_SCENE = {}


def scene():
    """the shared scene, rendered once per process"""
    if "s" not in _SCENE:
        _SCENE["s"] = Scene()
    return _SCENE["s"]


def oracle_features(img0, img1, P0, P1, voc=None):
    """a keyframe's steps (vo_loopclosing.cpp:236-372) by the oracle: ORB, (with a vocabulary) the bag of words of ALL descriptors, the
    kept landmarks"""
    kps, desc = O.orb_detect_and_compute(img0, cap=8192)
    kps, desc = kps[:1024], desc[:1024]
    lm2, lm3, lmd = O.lc_keyframe_landmarks(img0, img1, 0, kps, desc, P0, P1)
    f = dict(desc=desc, lm2=lm2, lm3=lm3, lmd=lmd)
    if voc is not None:
        f["bow"] = voc.transform(desc)
    return f


def pose_error(T, gt):
    """(translation of the camera centre in metres, rotation angle in radians) between two T_c_w pose7"""
    d = PS.mul7(T, PS.inv7(gt))
    Rg, tg = G.pose7_to_Rt(gt)
    R, t = G.pose7_to_Rt(T)
    return float(np.linalg.norm(-R.T @ t + Rg.T @ tg)), float(LC.so3_log_norm(d[3:7]))
