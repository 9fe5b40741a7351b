"""CPU: localisation in another unit's map as the oracle-assembled chain defines it (tests/_loop_localize_in.py), on the two-camera scene
the GPU test reuses: unit 1 of the fleet (synth.rig_variant("d435i_stereo", 1)) stores 4 keyframes of the tour, unit 2 sees the tour
between them.  Features come from the oracle's ORB / bag-of-words / landmark functions, each with the camera that took the image.
Checked: every query is localised in unit 1's map with the QUERY's K, the map's K gives another answer (the scene can tell the two
apart), and the pose error of T_c_map against the ground-truth pose of unit 2's camera -- the bounds are twice what
profiles/r12_loop_closer_localize_in.md records as measured (the margin is for the renderer's noise seeds, not for the code)."""
import numpy as np
import pytest

import _loop_chain as LC
import _loop_localize as LL
import _loop_localize_in as LI
import _voc as V
from test_oracle_bow import RefVoc

# measured maxima (profiles/r12_loop_closer_localize_in.md), translation in metres and angle in radians
MEASURED = (0.223435, 0.051096)


@pytest.fixture(scope="module")
def world():
    import flvis_amd  # noqa: F401  (the configs are parsed by the library's loader)
    sc = LI.cross_scene()
    cfg_m, cfg_q = sc.cfgs()
    cam_m, cam_q = LL.cam_of(cfg_m), LL.cam_of(cfg_q)
    raw_m = [LL.oracle_features(a, b, cam_m[0], cam_m[1]) for a, b in sc.map.kf]
    raw_q = [LL.oracle_features(a, b, cam_q[0], cam_q[1]) for a, b in sc.query.q]
    rv = RefVoc(V.build_vocabulary([f["desc"] for f in raw_m], k=6, depth=3))
    feat = lambda f: dict(f, bow=rv.transform(f["desc"]))
    ref = LC.RefLoopCloser(cam_m[2], prm=LL.PARAMS, stream=0)
    for f, T in zip(raw_m, sc.map.kf_gt):
        ref.add(feat(f), T)
    return dict(sc=sc, ref=ref, qs=[feat(f) for f in raw_q], K_m=cam_m[2], K_q=cam_q[2])


def test_queries_of_another_camera_are_localised_with_their_own_K(world):
    sc = world["sc"]
    assert not np.array_equal(world["K_m"], world["K_q"])
    worst, differ = [0.0, 0.0], 0
    for k, (q, gt) in enumerate(zip(world["qs"], sc.query.q_gt)):
        fix = LI.ref_localize_in({0: world["ref"]}, 0, q, 1, world["K_q"], 8)                  # the query is sequence 1's
        assert fix["n_landmarks"] > 100
        assert fix["best"] >= 0 and fix["map"] == 0 and len(fix["candidates"]) >= 2, fix       # the precondition the GPU test relies on
        assert all(c["seq"] == 0 for c in fix["candidates"])
        other = LI.ref_localize_in({0: world["ref"]}, 0, q, 1, world["K_m"], 8)                # the WRONG camera: the map's
        assert [c["kf"] for c in other["candidates"]] == [c["kf"] for c in fix["candidates"]]  # (the K enters after the choice)
        same = all(a["n_inliers"] == b["n_inliers"] and np.array_equal(a["pose"], b["pose"])
                   for a, b in zip(fix["candidates"], other["candidates"]))
        differ += not same
        et, ea = LL.pose_error(fix["T_c_map"], gt)
        print("query %d: accepted %d of %d, inliers %s (map's K: %s), pose error %.6f m %.6f rad" % (
            k, sum(c["accepted"] for c in fix["candidates"]), len(fix["candidates"]), [c["n_inliers"] for c in fix["candidates"]],
            [c["n_inliers"] for c in other["candidates"]], et, ea))
        worst = [max(worst[0], et), max(worst[1], ea)]
    print("localize_in: max pose error of T_c_map: %.6f m, %.6f rad" % tuple(worst))
    assert differ == len(world["qs"]), "the scene does not tell the two cameras apart"
    assert worst[0] <= 2 * MEASURED[0] and worst[1] <= 2 * MEASURED[1], worst
