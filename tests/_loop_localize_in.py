"""Test helper: localisation in another sequence's map (flvis_loop_closer_localize_in) assembled from the CPU oracle's functions --
tests/_loop_localize.py's chain with (sequence, keyframe) candidates:

    candidates   the n_best keyframes of the searched sequences with the highest ref_score against the query among those with score > 0
                 and >= minScore, by score descending, equal scores by sequence ascending, then keyframe index ascending
    pair check   isLoopClosureKF on (database keyframe, query): the keyframe's 3-D points -- made with the camera of the sequence that
                 stored it --, the query's pixels, solvePnPRansac with the K of the QUERY's camera; the seed names the query's sequence
    best         as in ref_localize; T_c_map = pose * T_c_w(sequence, keyframe): the query camera in the frame of that sequence's map

and the small scene of the two-camera tests: one tour seen by two units of the fleet (synth.rig_variant("d435i_stereo", 1 / 2)), unit 1's
keyframes as the map, unit 2's frames between them as queries; rendered on the CPU once per process."""
import os
import tempfile

import numpy as np

import _loop_chain as LC
import _loop_localize as LL
import _oracle as O
import _pgo_synth as PS
from test_oracle_bow import ref_score

ALL_MAPS = -1
CROSS_QUERY_TIMES = (0.4, 1.8, 3.0)


def ref_localize_in(refs, maps, feat, stream, K4, n_best):
    """refs: {sequence: LC.RefLoopCloser} (kfs / T_c_w / prm of every sequence that may be searched), maps: the searched sequence or
    ALL_MAPS, feat: the query's feature dict (made with its own camera), stream: the query's sequence, K4: the query camera's
    -> dict like LoopCloser.localize_in's"""
    p = refs[min(refs)].prm
    searched = sorted(refs) if maps < 0 else [maps]
    scored = [(ref_score(feat["bow"], kf["bow"]), s, j) for s in searched for j, kf in enumerate(refs[s].kfs)]
    order = sorted((e for e in scored if e[0] > 0 and e[0] >= p["minScore"]), key=lambda e: (-e[0], e[1], e[2]))[:n_best]
    cands, best = [], -1
    for r, (score, s, j) in enumerate(order):
        c = dict(seq=s, kf=j, score=score, n_matches=0, n_inliers=0, accepted=False, pose=LL.IDENT.copy())
        cands.append(c)
        k0 = refs[s].kfs[j]
        if len(k0["lmd"]) == 0 or len(feat["lmd"]) == 0:
            continue
        pairs = np.array(O.orb_match(k0["lmd"], feat["lmd"], p["ratioMax"])).reshape(-1, 2)
        c["n_matches"] = len(pairs)
        if len(pairs) < 5:                                                      # :666
            continue
        p3d = k0["lm3"][pairs[:, 0]].astype(np.float32)
        p2d = feat["lm2"][pairs[:, 1]].astype(np.float32)
        ninl, pose, _ = O.solve_pnp_ransac(p3d, p2d, np.asarray(K4, np.float64), iterative=False, iterations=100, reproj=2.0, conf=0.99,
                                           seed=LL.pnp_seed(stream, r))
        c["n_inliers"], c["pose"] = int(ninl), pose
        if ninl * 1.0 / len(pairs) < p["ratioRansac"] or ninl < p["minPts"]:    # :677
            continue
        if not (np.linalg.norm(pose[:3]) < 3 and LC.so3_log_norm(pose[3:7]) < 1.5):  # :686
            continue
        c["accepted"] = True
        if best < 0 or c["n_inliers"] > cands[best]["n_inliers"]:
            best = r
    b = cands[best] if best >= 0 else None
    return dict(n_landmarks=len(feat["lmd"]), candidates=cands, best=best, kf=b["kf"] if b else -1, map=b["seq"] if b else -1,
                T_c_map=PS.mul7(b["pose"], refs[b["seq"]].T_c_w[b["kf"]]) if b else None)


def same_fix_in(got, want, tol=1e-12):
    """LL.same_fix, and the candidates' sequences and the map"""
    LL.same_fix(got, want, tol)
    assert [c["seq"] for c in got["candidates"]] == [c["seq"] for c in want["candidates"]], (got["candidates"], want["candidates"])
    assert got["map"] == want["map"], (got["map"], want["map"])


def as_fix_in(fix, seq):
    """a LoopCloser.localize result of sequence seq as localize_in reports it"""
    out = dict(fix, candidates=[dict(c, seq=seq) for c in fix["candidates"]])
    out["map"] = seq if fix["best"] >= 0 else -1
    return out


class CrossScene:
    """unit 1 maps the tour (4 keyframes), unit 2 drives it later (3 frames between them): rigs, yaml texts, images, ground truth"""

    def __init__(self):
        from flvis_amd import synth
        (self.rig_m, self.yaml_m), (self.rig_q, self.yaml_q) = (synth.rig_variant("d435i_stereo", k) for k in (1, 2))
        self.map = LL.Scene(phase=0.0, rig=self.rig_m, n_kf=4, query_times=())
        self.query = LL.Scene(phase=0.0, rig=self.rig_q, n_kf=0, query_times=CROSS_QUERY_TIMES)

    def cfgs(self):
        import flvis_amd
        out = []
        for k, text in ((1, self.yaml_m), (2, self.yaml_q)):
            p = os.path.join(tempfile.gettempdir(), "flvis_loop_localize_in_rig%d.yaml" % k)
            open(p, "w").write(text)
            out.append(flvis_amd.load_config(p))
        return out


_CROSS = {}


def cross_scene():
    if "s" not in _CROSS:
        _CROSS["s"] = CrossScene()
    return _CROSS["s"]
