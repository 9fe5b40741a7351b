"""CPU: relocalisation as the oracle-assembled chain defines it (tests/_loop_localize.py), on the scene the GPU test reuses: a tour of 9
keyframes, queries rendered between keyframes.  Features come from the oracle's ORB / bag-of-words / landmark functions.  What is checked
here is the chain itself and the scene's preconditions -- a query equal to a keyframe finds it, every in-between query is localised --
and how good the answer is against the ground-truth camera pose: the bounds are twice what profiles/r11_loop_closer_localize.md records
as measured (the margin is for the renderer's noise seeds, not for the code)."""
import numpy as np
import pytest

import _loop_chain as LC
import _loop_localize as LL
import _pgo_synth as PS
import _voc as V
from test_oracle_bow import RefVoc

# measured maxima (profiles/r11_loop_closer_localize.md), translation in metres and angle in radians
MEASURED_QUERY = (0.025535, 0.006858)
MEASURED_CONTINUE = (0.020825, 0.004665)


@pytest.fixture(scope="module")
def world():
    sc = LL.scene()
    P0, P1, K4 = LL.cam_of(LL.stereo_cfg())
    raw = [LL.oracle_features(a, b, P0, P1) for a, b in sc.kf]
    voc = V.build_vocabulary([f["desc"] for f in raw], k=6, depth=3)
    rv = RefVoc(voc)
    feat = lambda f: dict(f, bow=rv.transform(f["desc"]))
    kfs = [feat(f) for f in raw]
    qs = [feat(LL.oracle_features(a, b, P0, P1)) for a, b in sc.q]
    return dict(sc=sc, K4=K4, kfs=kfs, qs=qs)


def _closer(w, n, poses):
    ref = LC.RefLoopCloser(w["K4"], prm=LL.PARAMS)
    for j in range(n):
        ref.add(w["kfs"][j], poses[j])
    return ref


def test_a_query_equal_to_a_keyframe_finds_it(world):
    ref = _closer(world, LL.N_KF, world["sc"].kf_gt)
    for j in (0, 4, 8):
        fix = LL.ref_localize(ref, world["kfs"][j], 4)
        top = fix["candidates"][0]
        assert top["kf"] == j and abs(top["score"] - 1.0) < 1e-12 and top["accepted"], (j, fix)
        assert [c["score"] for c in fix["candidates"]] == sorted((c["score"] for c in fix["candidates"]), reverse=True)
        assert fix["best"] >= 0


def test_queries_between_keyframes_are_localised_within_the_measured_bound(world):
    sc = world["sc"]
    ref = _closer(world, LL.N_KF, sc.kf_gt)
    worst = [0.0, 0.0]
    for q, gt in zip(world["qs"], sc.q_gt):
        fix = LL.ref_localize(ref, q, 8)
        assert fix["n_landmarks"] > 100
        assert any(c["accepted"] for c in fix["candidates"]) and fix["best"] >= 0, fix       # the scene's precondition (the GPU test relies on it)
        assert [c["kf"] for c in LL.ref_localize(ref, q, 2)["candidates"]] == [c["kf"] for c in fix["candidates"][:2]]
        et, ea = LL.pose_error(fix["T_c_map"], gt)
        worst = [max(worst[0], et), max(worst[1], ea)]
    print("localize: max pose error of T_c_map: %.6f m, %.6f rad" % tuple(worst))
    assert worst[0] <= 2 * MEASURED_QUERY[0] and worst[1] <= 2 * MEASURED_QUERY[1], worst


def test_relocalise_and_continue(world):
    """keyframes 0..5 in the map; the odometry restarts at the identity on frame 6 (flvis_reset_streams); frame 6 is localised,
    T_odom_map = inv(T_c_odom) * T_c_map, and keyframes 7..8 of the new odometry frame land in the old map"""
    sc = world["sc"]
    ref = _closer(world, 6, sc.kf_gt)
    fix = LL.ref_localize(ref, world["kfs"][6], 4)
    assert fix["best"] >= 0, fix
    odom = lambda j: PS.mul7(sc.kf_gt[j], PS.inv7(sc.kf_gt[6]))      # the restarted tracker: frame 6's camera is its world
    ref.T_odom_map = PS.mul7(PS.inv7(odom(6)), fix["T_c_map"])        # set_drift
    worst = [0.0, 0.0]
    for j in (7, 8):
        ref.add(world["kfs"][j], odom(j))
        et, ea = LL.pose_error(ref.T_c_w[-1], sc.kf_gt[j])
        worst = [max(worst[0], et), max(worst[1], ea)]
    print("relocalise and continue: max map-pose error of keyframes 7..8: %.6f m, %.6f rad" % tuple(worst))
    assert worst[0] <= 2 * MEASURED_CONTINUE[0] and worst[1] <= 2 * MEASURED_CONTINUE[1], worst
