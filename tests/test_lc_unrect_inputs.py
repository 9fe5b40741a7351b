"""CPU: the inputs of the STEREO_UNRECT landmark tests reach their edges on the composed checker (tests/_lc_unrect.py) -- a pair that keeps
nearly everything, one that loses keypoints to BOTH drop causes, two that keep nothing, and a pair of keyframes that passes the reference's
acceptance rule -- and the two entry points are part of the C ABI and refuse a call without a context or closer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _binding
import _lc_unrect as U
import _loop_chain as LC
import _oracle as O
import _pgo_synth as PS
from _loop_localize import pose_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("flvis_hip_lc_keyframe_landmarks_unrect", "flvis_loop_closer_set_stereo_unrect")


@pytest.fixture(scope="module")
def world():
    inp = U.inputs()
    kps, desc = U.oracle_orb(inp.a0)
    return dict(inp=inp, kps=kps, desc=desc, true=U.check(inp.a0, inp.a1, kps, desc, inp.cam))


def test_the_true_pair_keeps_its_keypoints_on_one_rectified_row(world):
    r, n = world["true"], len(world["kps"])
    row = np.abs(r["u1"][r["keep"], 1] - r["u0"][r["keep"], 1])
    print("true pair: %d keypoints, %d kept, rectified row error median %.3f px, max %.3f px" % (n, r["keep"].sum(), np.median(row), row.max()))
    assert r["keep"].sum() > 100
    assert len(r["lm2"]) == len(r["lm3"]) == len(r["lmd"]) == r["keep"].sum()
    # the rendered pair IS the rig the config describes: after both undistortions a match lies on its keypoint's row
    assert np.median(row) < 0.5
    # lm_2d is the rectified pixel, not the raw one: on this rig (k1 = -0.28) they differ by pixels
    assert np.abs(r["lm2"] - world["kps"][r["keep"], :2]).max() > 2.0


def test_a_flat_second_image_meets_both_drop_causes(world):
    inp = world["inp"]
    r = U.check(inp.a0, inp.flat, world["kps"], world["desc"], inp.cam)
    n, lost = len(world["kps"]), int((r["status"] != 1).sum())
    behind = int((r["z"][r["status"] == 1] < 0).sum())
    far = int((r["z"][r["status"] == 1] > U.RANGE).sum())
    print("flat img1: %d keypoints, %d status 0, %d z < 0, %d z > range, %d kept" % (n, lost, behind, far, r["keep"].sum()))
    assert 0 < r["keep"].sum() < n
    assert lost > 0 and behind > 0                                                 # both causes: no match, and a match behind the camera
    assert r["keep"].sum() == n - lost - behind - far
    assert np.array_equal(r["lmd"], world["desc"][r["keep"]])                      # order kept


def test_two_inputs_keep_nothing(world):
    inp = world["inp"]
    r = U.check(inp.a0, inp.a1, world["kps"][:0], world["desc"][:0], inp.cam)
    assert len(r["lm2"]) == len(r["lm3"]) == len(r["lmd"]) == 0
    r = U.check(inp.a0, inp.moved, world["kps"], world["desc"], inp.cam)
    ok = r["status"] == 1
    print("img0 moved 40 px right: %d keypoints, %d status 1, their largest z %.4f" % (len(ok), ok.sum(), r["z"][ok].max() if ok.any() else np.nan))
    assert ok.sum() > 100                        # ... and not because the matcher gave up: it followed, and every depth is negative
    assert r["keep"].sum() == 0 and len(r["lm2"]) == 0


def test_two_keyframes_pass_the_reference_s_acceptance_rule(world):
    inp, p = world["inp"], LC.LC_PARAMS
    kb, db = U.oracle_orb(inp.b0)
    a, b = world["true"], U.check(inp.b0, inp.b1, kb, db, inp.cam)
    pairs = np.array(O.orb_match(a["lmd"], b["lmd"], p["ratioMax"])).reshape(-1, 2)
    assert p["ratioMax"] == 0.5 and len(pairs) >= 5
    ninl, pose, _ = O.solve_pnp_ransac(a["lm3"][pairs[:, 0]].astype(np.float32), b["lm2"][pairs[:, 1]].astype(np.float32), U.K4_of(inp.cfg),
                                       iterative=False, iterations=100, reproj=2.0, conf=0.99, seed=LC.pnp_seed(0, 1))
    et, ea = pose_error(pose, PS.mul7(inp.gt_b, PS.inv7(inp.gt_a)))
    print("t = 0 / t = 1.2: %d matches, %d inliers, %.3f deg and %.4f m from the truth (rectified frame)" % (len(pairs), ninl, np.degrees(ea), et))
    assert ninl * 1.0 / len(pairs) >= p["ratioRansac"] and ninl >= p["minPts"]             # vo_loopclosing.cpp:677
    assert np.linalg.norm(pose[:3]) < 3 and LC.so3_log_norm(pose[3:7]) < 1.5               # :686


def test_entry_points_are_declared_exported_and_bound():
    import flvis_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    src = _binding.source()
    lib = flvis_amd.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared in include/flvis_hip.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert re.search(r"_lib\.%s\b" % name, src), "%s is not bound by flvis_amd" % name
    assert callable(flvis_amd.Context.lc_keyframe_landmarks_unrect) and callable(flvis_amd.LoopCloser.set_stereo_unrect)


def test_null_handles_are_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    cfg = flvis_amd.FlvisCfg()
    null = C.c_void_p(0)
    fn = lib.flvis_hip_lc_keyframe_landmarks_unrect
    assert fn(null, null, null, U.W, U.H, 1, C.byref(cfg), 1, null, null, null, 1024, null, null, null, null) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_set_stereo_unrect(null, 1) == flvis_amd.FLVIS_ERR_INVALID_ARG
