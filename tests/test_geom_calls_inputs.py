"""CPU: every input of tests/_geom_calls.py reaches, on the oracle, the edge it is there for -- so that tests/test_gpu_geom_calls.py, which
compares the kernels with these figures, cannot pass on inputs that have drifted away from their edges."""
import time

import numpy as np
import pytest

import _geom_calls as E
import _oracle as O

needs_product_sums = pytest.mark.skipif(O.lib().ref_sum_order() != 0, reason="the REF_ORDER=g2o checker sums the pose LM in another order")


def test_f_counts_cover_every_branch_of_the_dispatch():
    S = E.f_sets()
    assert len(S) == 65
    for n in E.F_COUNTS:
        a, b = S["clean_%d" % n]
        assert a.shape == b.shape == (n, 2) and a.dtype == np.float32
    assert E.f_expected("clean_0") == (0, E.f_expected("clean_0")[1]) and E.f_expected("clean_6")[0] == 0
    assert not E.f_expected("clean_6")[1].any()
    assert E.f_expected("clean_7")[0] == 7 and E.f_expected("clean_7")[1].all()
    # 20 % gross outliers: the clean sets from 15 points on find the motion -- most of the inliers in, most of the outliers out
    for n in (15, 16, 64, 65, 240, 1024):
        got, mask = E.f_expected("clean_%d" % n)
        assert got == mask.sum() and 0.7 * n <= got <= 0.95 * n, (n, got)


def test_lmeds_sets_take_the_lmeds_branch():
    """8 .. 14 points: OpenCV runs the LMedS registrator, whose inlier rule (2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median)) does not look at
    thr_px -- the RANSAC branch does.  A threshold no pair can meet empties a RANSAC mask and leaves an LMedS mask as it is."""
    for name in ("clean_8", "clean_14", "lmeds_9", "lmeds_11_outl", "dup_all_10"):
        assert 8 <= len(E.f_sets()[name][0]) <= 14
        a, b = E.f_expected(name), E.f_expected(name, thr=1e-9)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert E.f_expected("clean_8")[0] >= 7 and E.f_expected("clean_14")[0] >= 7 and E.f_expected("lmeds_9")[0] >= 7
    ransac = E.f_expected("clean_15", thr=1e-9)                # ... while the 15-point set is the RANSAC branch's
    assert ransac[0] < E.f_expected("clean_15")[0]


def test_all_outlier_set_ends_without_a_model():
    for name in ("outliers_40", "outliers_300"):               # at image scale seven pairs always carry their own model
        got, mask = E.f_expected(name)
        assert 7 <= got == mask.sum() < 0.5 * len(mask)
    got, mask = E.f_expected("no_model_40")                    # ... at 1e20 no model keeps more than 6: the mask stays empty
    assert got == 0 and not mask.any() and len(mask) == 40
    a, b = E.f_sets()["no_model_40"]
    assert np.isfinite(a).all() and np.isfinite(b).all() and len(np.unique(a, axis=0)) == 40


def test_collinear_and_duplicate_sets_make_get_subset_give_up():
    for name in ("collinear_30", "collinear_12", "dup_all_30", "dup_all_10"):
        t0 = time.perf_counter()
        got, mask = O.find_fundamental_ransac(*E.f_sets()[name])
        dt = time.perf_counter() - t0
        assert got == 0 and not mask.any(), name
        assert dt < 1.0, "%s: the checker took %.2f s" % (name, dt)
    a, _ = E.f_sets()["collinear_30"]
    d = a - a[0]
    assert np.abs(d[:, 0] * d[1, 1] - d[:, 1] * d[1, 0]).max() == 0.0
    got, mask = E.f_expected("dup_half_60")                    # half of the pairs one and the same: subsets are refused and redrawn, a model is found
    assert got >= 30 and mask[0] == 1 and mask[::2].all()


@needs_product_sums
def test_pose_lm_counts_and_cull_edges():
    S = E.lm_sets()
    assert not S["count_9"].expected[0] and np.array_equal(S["count_9"].expected[1], S["count_9"].pose0)
    for n in E.LM_COUNTS[1:]:
        s = S["count_%d" % n]
        ok, pose = s.expected
        assert ok and s.n == n and not np.array_equal(pose, s.pose0)
        c = E.chi2_at(pose, s)                                 # the 40 px observations are what the cull drops
        k = E.lm_outliers(n)
        assert (c[:k] > 100).all() and (c[k:] < 3).all() and (k > 0 or n == 10)
    # 14 edges each; at the pose the 10-alive set converges to, exactly 10 (and of the other set exactly 9) are below chi2 = 3, all others far above
    ok10, pose10 = S["cull_10"].expected
    ok9, pose9 = S["cull_9"].expected
    assert ok10 and not ok9 and np.array_equal(pose9, S["cull_9"].pose0)
    c10, c9 = E.chi2_at(pose10, S["cull_10"]), E.chi2_at(pose10, S["cull_9"])
    assert (c10 < 1.5).sum() == 10 and (c10 > 300).sum() == 4
    assert (c9 < 1.5).sum() == 9 and (c9 > 300).sum() == 5
    assert S["cull_9"].n == S["cull_10"].n == 14


@needs_product_sums
def test_pose_lm_id_orders():
    S = E.lm_sets()
    for name in ("ids_descending", "ids_negative", "ids_duplicate", "ids_all_equal", "ids_duplicate_swapped"):
        assert S[name].expected[0], name
    assert (np.diff(S["ids_descending"].ids) < 0).all() and (S["ids_negative"].ids < -(1 << 39)).all()
    # equal ids are taken in input order: exchanging the two edges of every equal-id pair changes the order of the sums, and the pose with it
    a, b = S["ids_duplicate"], S["ids_duplicate_swapped"]
    assert np.array_equal(a.ids, b.ids) and not np.array_equal(a.p3, b.p3)
    assert not np.array_equal(a.expected[1], b.expected[1])
    assert np.abs(a.expected[1] - b.expected[1]).max() < 1e-9   # (the same optimum, rounded differently)
    # ... while the order of edges with DIFFERENT ids does not matter: sorted by id they are the same sequence
    d = S["ids_descending"]
    o = np.arange(d.n)[::-1]
    r = E.LmSet(d.p3[o], d.z[o], d.ids[o], d.pose0, d.K)
    assert np.array_equal(r.expected[1], d.expected[1])


@needs_product_sums
def test_pose_lm_cameras_differ():
    S = E.lm_sets()
    a, b = S["camera_0"], S["camera_1"]
    assert a.expected[0] and b.expected[0] and not np.array_equal(a.K, b.K)
    wrong = E.LmSet(b.p3, b.z, b.ids, b.pose0, a.K)            # camera 1's set with camera 0's K: another answer
    assert not np.array_equal(wrong.expected[1], b.expected[1])


def test_point_sets_reach_their_edges():
    R = E.rigs()
    assert not R["pinhole"][1].any() and R["euroc"][1][0] < -0.1
    for rig in E.RIGS:
        for n in E.PT_COUNTS:
            und, prj = E.pt_expected(rig, n)
            assert und.shape == prj.shape == (n, 2) and und.dtype == np.float32
        und, prj = E.pt_expected(rig, 65)
        s = E.pt_sets()[(rig, 65)]
        assert s["p3d"][0, 2] == 0 and s["p3d"][1, 2] < 0
        K, D = R[rig][0], R[rig][1]
        assert np.isfinite(prj[:3]).all()
        if rig == "pinhole":                                   # z == 0 reads as 1 / z = 1: the pixel of (x, y, 1)
            assert np.array_equal(prj[0], np.array([1.0 * K[0] + K[2], 2.0 * K[1] + K[3]], np.float32))
        assert np.isposinf(prj[3, 0]) and np.isneginf(prj[3, 1])
        assert not np.isfinite(und[:2]).any() and np.isfinite(und[3:]).all() and np.isfinite(prj[4:]).all()
    # the distortion matters: the EuRoC rig's undistorted pixels are not the pinhole's identity map
    s = E.pt_sets()[("pinhole", 64)]
    assert np.abs(E.pt_expected("pinhole", 64)[0][3:] - s["src"][3:]).max() < 1e-3
    s = E.pt_sets()[("euroc", 64)]
    assert np.abs(E.pt_expected("euroc", 64)[0][3:] - s["src"][3:]).max() > 5
