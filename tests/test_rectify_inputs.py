"""CPU: the definition of flvis_hip_rectify (include/flvis_hip.h) as tests/_rectify.py restates it.  The two write-ups agree on every edge
case, each case reaches the edge it is named for, the unquantised map agrees with the rig's own projection model, rectifying the rendered
EuRoC-like pair is what makes the dense matcher work on it, and the library's host-only check refuses what the header says."""
import ctypes as C

import numpy as np
import pytest

import _dense_stereo as DS
import _rectify as RC

CASES = RC.edge_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_write_ups_agree(name):
    a, b = RC.restate(CASES[name]), RC.restate_loops(CASES[name])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


def test_the_two_write_ups_agree_on_a_lens_and_interleaved_cameras():
    case = RC.lens_case(33, 21, n=5, cam_of=[0, 1, 0, 1, 1], n_cam=2)
    a, b = RC.restate(case), RC.restate_loops(case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert 0.5 < a[1].mean() < 1.0 and not np.array_equal(a[1][0], a[1][1])


def test_an_identity_camera_reproduces_its_image():
    case = CASES["identity"]
    dst, cov, maps = RC.restate(case, detail=True)
    h, w = case["src"].shape[1:]
    assert np.array_equal(maps[0]["ix"], np.broadcast_to(32 * np.arange(w)[None, :], (h, w)))
    assert np.array_equal(maps[0]["iy"], np.broadcast_to(32 * np.arange(h)[:, None], (h, w)))
    assert cov.all() and np.array_equal(dst, case["src"]), "last row and column included"


def test_ties_round_to_even_odd_and_even_alike():
    case = CASES["ties"]
    _, cov, maps = RC.restate(case, detail=True)
    m = maps[0]
    h, w = case["src"].shape[1:]
    U, V = np.broadcast_to(np.arange(w)[None, :], (h, w)), np.broadcast_to(np.arange(h)[:, None], (h, w))
    assert np.array_equal(m["tx"], 32.0 * U + 0.5) and np.array_equal(m["ty"], 32.0 * V + 1.5), "an integer plus exactly a half"
    assert np.array_equal(m["ix"], 32 * U), "an even integer plus a half rounds down"
    assert np.array_equal(m["iy"], 32 * V + 2), "an odd one rounds up"


def test_the_borders_in_both_axes():
    case = CASES["borders"]
    dst, cov, maps = RC.restate(case, detail=True)
    h, w = case["src"].shape[1:]
    by = dict(zip(RC.BORDER_SHIFTS, maps))
    for axis, (i, s, a, n) in {"x": ("ix", "sx", "ax", w), "y": ("iy", "sy", "ay", h)}.items():
        at = (lambda m, cond: m["covered"][cond])
        m = by[-1]
        hit = m[i] == -1
        assert hit.any() and (m[s][hit] == -1).all() and (m[a][hit] == 31).all() and not at(m, hit).any(), (axis, "ix = -1")
        m = by[-32]
        hit = m[i] == -32
        assert hit.any() and (m[s][hit] == -1).all() and (m[a][hit] == 0).all() and not at(m, hit).any(), (axis, "ix = -32")
        m = by[0]
        hit = (m[s] == n - 1) & (m[a] == 0)
        assert hit.any() and at(m, hit).all(), (axis, "the last column with weight 0 on the next")
        m = by[1]
        hit = (m[s] == n - 1) & (m[a] == 1)
        assert hit.any() and not at(m, hit).any(), (axis, "the last column with a weight on the next")
    assert np.array_equal(dst[2], case["src"][2]) and cov[2].all()
    assert cov[3][:-1, :-1].all() and not cov[3][-1].any() and not cov[3][:, -1].any()


def test_non_finite_and_huge_positions_are_uncovered():
    case = CASES["non-finite"]
    dst, cov, maps = RC.restate(case, detail=True)
    m = maps[0]
    nonfinite = ~np.isfinite(m["tx"]) | ~np.isfinite(m["ty"])
    with np.errstate(invalid="ignore"):
        huge = ~nonfinite & ((np.abs(m["tx"]) >= RC.LIMIT) | (np.abs(m["ty"]) >= RC.LIMIT))
    assert nonfinite[:, 10].all() and np.isnan(m["ty"]).any() and huge.any()
    assert not cov[0][nonfinite | huge].any() and not dst[0][nonfinite | huge].any()
    assert cov.any(), "and some pixels of the case are covered"


def test_every_pair_of_weights_occurs():
    case = CASES["weights"]
    _, cov, maps = RC.restate(case, detail=True)
    m = maps[0]
    pairs = set(zip(m["ax"][m["covered"]].tolist(), m["ay"][m["covered"]].tolist()))
    assert len(pairs) == 1024


def test_the_map_agrees_with_the_rigs_own_projection():
    """20000 random points in front of the rig: their rectified pixel (P0 on the point rotated by R0; camera 1 at column u - bf / z, the
    same row) goes through the unquantised map and must land where the rig's own model -- pinhole and radtan of the raw camera, camera 1
    behind the rig's extrinsics -- projects the point.  6e-11 px was measured; the bound leaves room for another libm or numpy."""
    from flvis_amd import synth
    cfg = RC.euroc_cfg(0)
    cams = RC.cameras_of_cfg(cfg)
    rig = synth.euroc_rig()
    rng = np.random.default_rng(20)
    z = rng.uniform(1.0, 12.0, 20000)
    P = np.stack([rng.uniform(-0.45, 0.45, 20000) * z, rng.uniform(-0.3, 0.3, 20000) * z, z], 1)     # raw camera 0's frame
    Pr = P @ np.array(list(cfg.R0)).reshape(3, 3).T
    fxn, fyn, cxn, cyn = cams[0][17:21]
    u, v = fxn * Pr[:, 0] / Pr[:, 2] + cxn, fyn * Pr[:, 1] / Pr[:, 2] + cyn
    bf = -float(cfg.P1[3])
    P1 = (P - rig.t_c0_c1) @ rig.R_c0_c1                            # X_c1 = R^T (X_c0 - t)
    worst = []
    for cam, K, D, pts, uu in ((cams[0], rig.K0, rig.D0, P, u), (cams[1], rig.K1, rig.D1, P1, u - bf / Pr[:, 2])):
        mx, my = RC.map_points(cam, uu, v)
        want = RC.project_radtan(K, D, pts)
        worst.append(float(max(np.abs(mx - want[:, 0]).max(), np.abs(my - want[:, 1]).max())))
    print("map against the rig's projection: %.3g px (camera 0), %.3g px (camera 1)" % tuple(worst))
    assert max(worst) <= 1e-8


def test_rectifying_is_what_makes_the_matcher_work_on_the_euroc_pair():
    """Rows 208 .. 271 of the rendered EuRoC-like pair, 64 disparities, the matcher's other parameters at their defaults.  Measured with
    these write-ups, the matcher given the rows' whole support (5 more rows above and below): rectified pair 0.8804 valid, 0.0212 of the
    valid pixels with ground truth more than 1 px off; raw pair 0.2250 valid; uncovered 0 of camera 0, 0.00013 of camera 1.  (Given the
    64 rows alone the matcher cannot validate the band's first and last 5 rows: 0.7383, 0.0232 and 0.1920 of all 64 rows, which is 0.8750
    and 0.2276 of the 54 rows it can -- the figures 87.5 %, 2.3 % and 22.8 % this feature was proposed with.)"""
    r = RC.rendered_euroc()
    v0, v1 = r["rows"]
    prm = DS.params(n_disp=64)
    m = 3 + prm["agg_r"]                                            # the matcher sees the rows' whole support: m rows above and below
    d16 = DS.restate_one(r["rect0"][v0 - m:v1 + m], r["rect1"][v0 - m:v1 + m], r["bf"], 1000.0, prm)[0][m:-m]
    valid = d16 > 0
    gt = r["gt"][v0:v1]
    known = valid & np.isfinite(gt)
    off = np.abs(d16[known] / 16.0 - gt[known]) > 1.0
    raw16 = DS.restate_one(r["raw0"][v0 - m:v1 + m], r["raw1"][v0 - m:v1 + m], r["bf"], 1000.0, prm)[0][m:-m]
    unc = [1.0 - float(r["cov0"].mean()), 1.0 - float(r["cov1"].mean())]
    print("rectified: valid %.4f, more than 1 px off %.4f (of %d with ground truth); raw: valid %.4f; uncovered %.5f, %.5f"
          % (valid.mean(), off.mean(), known.sum(), (raw16 > 0).mean(), unc[0], unc[1]))
    assert known.sum() > 0.1 * valid.sum(), "the ground truth reaches a tenth of the valid pixels at least"
    assert valid.mean() > 0.80
    assert off.mean() < 0.04
    assert (raw16 > 0).mean() < 0.40
    assert max(unc) < 0.001


# ---- the library's own argument check ---------------------------------------------------------------------------------------------------
GOOD = RC.camera((64.0, 64.0, 20.0, 9.0))


def _check(n_img=3, w=37, h=23, n_cam=1, cams=(GOOD,), cam_of=None, src=1 << 20, dst=1 << 22, cov=0):
    from flvis_amd import load_library
    lib = load_library()
    cam21 = None if cams is None else np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 21))
    of = None if cam_of is None else np.ascontiguousarray(cam_of, np.int32)
    return lib.flvis_rectify_check(C.c_void_p(src), n_img, w, h, n_cam, None if cam21 is None else cam21.ctypes.data_as(C.c_void_p),
                                   None if of is None else of.ctypes.data_as(C.c_void_p), C.c_void_p(dst), C.c_void_p(cov))


def _with(index, value):
    c = GOOD.copy()
    c[index] = value
    return c


def test_the_library_check_accepts_and_refuses_what_the_header_says():
    from flvis_amd import FLVIS_ERR_INVALID_ARG, FLVIS_OK
    n = 3 * 37 * 23
    assert _check() == FLVIS_OK
    assert _check(cov=1 << 24) == FLVIS_OK
    assert _check(n_cam=3, cams=(GOOD,) * 3) == FLVIS_OK
    assert _check(n_cam=2, cams=(GOOD,) * 2, cam_of=[0, 1, 1]) == FLVIS_OK
    assert _check(n_cam=5, cams=(GOOD,) * 5, cam_of=[4, 0, 4]) == FLVIS_OK
    assert _check(n_img=1, w=1, h=1) == FLVIS_OK
    assert _check(dst=(1 << 20) + n) == FLVIS_OK and _check(dst=(1 << 20) - n) == FLVIS_OK, "arrays that touch do not overlap"
    assert _check(cams=(_with(2, -5.0),)) == FLVIS_OK and _check(cams=(_with(4, -0.3),)) == FLVIS_OK, "cx and k1 may be negative"
    bad = [dict(w=0), dict(h=0), dict(n_img=0), dict(w=-2), dict(n_cam=0), dict(n_cam=-1), dict(src=0), dict(dst=0), dict(cams=None),
           dict(n_cam=2, cams=(GOOD,) * 2), dict(n_cam=2, cams=(GOOD,) * 2, cam_of=[0, 2, 1]), dict(n_cam=2, cams=(GOOD,) * 2, cam_of=[0, -1, 1]),
           dict(cams=(_with(5, float("nan")),)), dict(cams=(_with(12, float("inf")),)), dict(cams=(_with(20, float("-inf")),)),
           dict(cams=(_with(0, 0.0),)), dict(cams=(_with(1, -64.0),)), dict(cams=(_with(17, 0.0),)), dict(cams=(_with(18, -1.0),)),
           dict(n_cam=2, cams=(GOOD, _with(0, 0.0)), cam_of=[0, 0, 0]),
           dict(dst=1 << 20), dict(dst=(1 << 20) + n - 1), dict(dst=(1 << 20) - n + 1), dict(cov=1 << 20), dict(cov=(1 << 20) + 5)]
    for kw in bad:
        assert _check(**kw) == FLVIS_ERR_INVALID_ARG, kw


def test_the_new_entry_points_are_declared_exported_and_bound():
    import os
    import re

    import _binding
    import flvis_amd
    lib = flvis_amd.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "flvis_hip.h")).read(), flags=re.S)
    src = _binding.source()
    for name in ("flvis_hip_rectify", "flvis_rectify_check", "flvis_keyframe_log_rectified_pair", "flvis_keyframe_log_unrect_stereo_z16",
                 "flvis_keyframe_log_unrect_stereo_cloud", "flvis_keyframe_log_unrect_stereo_cloud_host",
                 "flvis_loop_closer_unrect_stereo_cloud", "flvis_loop_closer_unrect_stereo_cloud_host"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared" % name
        assert hasattr(lib, name), "%s is not exported" % name
    for name in ("flvis_hip_rectify", "flvis_keyframe_log_rectified_pair", "flvis_keyframe_log_unrect_stereo_z16"):
        assert re.search(r"lib\.%s\b" % name, src), "%s is not bound by flvis_amd" % name
    for cls, meth in ((flvis_amd.Context, "rectify"), (flvis_amd.Tracker, "keyframe_log_rectified_pair"),
                      (flvis_amd.Tracker, "keyframe_log_unrect_stereo_z16"), (flvis_amd.Tracker, "keyframe_log_unrect_stereo_cloud"),
                      (flvis_amd.LoopCloser, "unrect_stereo_cloud")):
        assert callable(getattr(cls, meth)), (cls, meth)
