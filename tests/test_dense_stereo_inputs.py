"""CPU: the dense stereo restatement (tests/_dense_stereo.py) against its second write-up, proof that every edge case reaches its edge,
exact recovery of a shift, the definition's accuracy on a rendered pair, and the host part of flvis_hip_dense_stereo's argument checks
(flvis_dense_stereo_check, no device)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _dense_stereo as DS


@functools.lru_cache(maxsize=None)
def _detail(name):
    case = DS.edge_cases()[name]
    out = []
    for i in range(len(case["img0"])):
        bf, df = DS.cam_of(case, i)
        out.append(DS.restate_one(case["img0"][i], case["img1"][i], bf, df, case["prm"], detail=True))
    return case, out


@pytest.mark.parametrize("name", sorted(DS.edge_cases()))
def test_the_two_write_ups_agree(name):
    case, out = _detail(name)
    for i, (d16, z16, _) in enumerate(out):
        bf, df = DS.cam_of(case, i)
        d2, z2 = DS.restate_loops(case["img0"][i], case["img1"][i], bf, df, case["prm"])
        assert np.array_equal(d16, d2) and np.array_equal(z16, z2), (name, i)


def test_the_two_write_ups_agree_on_a_window_of_the_rendered_band():
    """(the loops take minutes on the whole band: 24 rows x 200 columns of it, 32 disparities)"""
    i0, i1, _, bf = DS.rendered_band()
    a, b = i0[20:44, 300:500], i1[20:44, 300:500]
    prm = DS.params(n_disp=32)
    d16, z16 = DS.restate_one(a, b, bf, 1000.0, prm)
    d2, z2 = DS.restate_loops(a, b, bf, 1000.0, prm)
    assert (d16 > 0).mean() > 0.3
    assert np.array_equal(d16, d2) and np.array_equal(z16, z2)


def test_floor_differs_from_truncation_somewhere():
    _, out = _detail("random")
    D = out[0][2]
    trunc = np.where(D["num"] < 0, -((-D["num"]) // (2 * D["den"])), D["num"] // (2 * D["den"]))
    at = D["valid"] & (D["num"] < 0) & (trunc != D["num"] // (2 * D["den"]))
    assert at.sum() >= 10
    d16 = out[0][0].astype(np.int64)
    assert np.array_equal(d16[at], (16 * D["best"] + trunc - 1)[at])


def test_the_clamp_of_den_cannot_engage_on_a_valid_pixel():
    """p + n - 2 c = 0 needs p = c, and then best - 1, which must be in D, would be the lowest d among equals: the argmin's tie rule and
    the interior condition exclude it.  The clamp only keeps the division defined; the numerator is negative for n well above p > c."""
    seen = 0
    for name in DS.edge_cases():
        for _, _, D in _detail(name)[1]:
            v = D["valid"]
            seen += int(v.sum())
            assert ((D["p"] > D["c"]) & (D["n"] >= D["c"]))[v].all(), name
            assert (D["den"][v] >= 1).all() and ((D["p"] + D["n"] - 2 * D["c"])[v] >= 1).all()
    assert seen > 5000


def test_a_far_tie_is_rejected_by_uniqueness_and_kept_lowest_without():
    case, out = _detail("periodic uniq 10")
    _, out0 = _detail("periodic uniq 0")
    D, D0 = out[0][2], out0[0][2]
    A = D["A"]
    # the tie is exact: d and d + 8 cost the same wherever both are defined, and the best cost is not 0
    both = (A[:16] < DS.INF) & (A[8:24] < DS.INF)
    assert both.sum() > 5000 and np.array_equal(A[:16][both], A[8:24][both])
    tied = D["some"] & (D["c"] > 0) & (np.take_along_axis(A, np.clip(D["best"] + 8, 0, 23)[None], 0)[0] == D["c"])
    assert tied.sum() > 500
    assert D["rej_uniq"][tied].all() and (out[0][0][tied] == 0).all()
    assert not D0["rej_uniq"].any()
    kept = tied & D0["valid"]
    assert kept.sum() > 500 and (D0["best"][kept] < 8).all() and (out0[0][0][kept] > 0).all()


def test_a_pixel_is_rejected_by_the_left_right_check_alone():
    _, out = _detail("occlusion")
    _, off = _detail("occlusion no lr")
    D = out[0][2]
    only = D["some"] & ~D["rej_uniq"] & D["interior"] & D["rej_lr"]
    assert only.sum() >= 10
    assert (out[0][0][only] == 0).all() and (off[0][0][only] > 0).all()


def test_a_raw_depth_above_65535_is_invalid_in_z16_only():
    _, out = _detail("far")
    d16, z16, D = out[0]
    at = D["valid"] & (D["raw"] > 65535)
    assert at.sum() >= 10 and (z16[at] == 0).all() and (d16[at] > 0).all()
    assert (z16[D["valid"] & ~at] > 0).all()


def test_an_exact_half_rounds_to_even():
    _, out = _detail("half")
    for (d16, z16, D), (exact, want) in zip(out, [(10.5, 10), (11.5, 12)]):
        at = D["valid"] & (d16 == 64)
        assert at.sum() > 500 and (D["exact"][at] == exact).all() and (z16[at] == want).all()


@pytest.mark.parametrize("d_min,n_disp", [(0, 64), (3, 16)])
def test_a_shift_is_recovered(d_min, n_disp):
    """A noise image and its copy k columns over, k = d_min + 1 and d_min + n_disp - 2.  Every pixel with k - 1, k, k + 1 in D is valid with
    best = k: the cost there is 0 and nowhere else.  d16 is 16 k + floor(1 / 2 + 8 (p - n) / (p + n)), which is 16 k exactly where
    16 |p - n| < p + n; p and n are two independent sums of noise, so about 1 pixel in 100 lies one step of 1/16 px off (measured here: 3 to 28
    of about 1500): "d16 == 16 k at every pixel" does not follow from the definition.  The test asserts best = k and the formula at every
    pixel, and d16 == 16 k wherever the condition holds."""
    for k in (d_min + 1, d_min + n_disp - 2):
        a, b = DS.shifted(np.random.default_rng(k), 23, 130, k)
        d16, _, D = DS.restate_one(a, b, 30.0, 1000.0, DS.params(d_min=d_min, n_disp=n_disp), detail=True)
        A = D["A"]
        inD = (A[k - 1 - d_min] < DS.INF) & (A[k - d_min] < DS.INF) & (A[k + 1 - d_min] < DS.INF)
        assert inD.sum() > 500
        assert D["valid"][inD].all() and (D["best"][inD] == k).all() and (D["c"][inD] == 0).all()
        p, n = D["p"][inD], D["n"][inD]
        got = d16[inD].astype(np.int64)
        assert np.array_equal(got, 16 * k + ((p - n) * 16 + p + n) // (2 * (p + n)))
        sure = 16 * np.abs(p - n) < p + n
        assert (got[sure] == 16 * k).all() and (np.abs(got - 16 * k) <= 8).all()


def test_accuracy_on_the_rendered_pair():
    """Rows 208 .. 271 of the rendered D435i pair, defaults: 0.7285 of the band's pixels are valid and 0.0103 of the valid ones are more than
    1 px from the renderer's disparity (median error 0.20 px; the full frame gives 0.8405 and 0.0131).  This tests the definition, not
    the kernel."""
    i0, i1, gt, bf = DS.rendered_band()
    d16, _ = DS.restate_one(i0, i1, bf, 1000.0, DS.params())
    valid = d16 > 0
    off = np.abs(d16 / 16.0 - gt)[valid] > 1.0
    print("valid %.4f, more than 1 px off %.4f" % (valid.mean(), off.mean()))
    assert valid.mean() >= 0.6
    assert off.mean() <= 0.05


# ---- the library's own argument check ---------------------------------------------------------------------------------------------------
def _check(n_img=2, w=97, h=23, n_cam=1, cam=((30.0, 1000.0),), prm=None, img0=1, img1=1, disp=1, z=1, **kw):
    from flvis_amd import dense_stereo_params, load_library
    lib = load_library()
    cam2 = None if cam is None else np.ascontiguousarray(np.asarray(cam, np.float64).reshape(-1, 2))
    p = dense_stereo_params(**kw) if prm is None else prm
    ptr = lambda x: C.c_void_p(4096 * x)                        # (only compared with NULL)
    return lib.flvis_dense_stereo_check(ptr(img0), ptr(img1), n_img, w, h, n_cam, None if cam2 is None else cam2.ctypes.data_as(C.c_void_p),
                                        C.byref(p) if p is not False else None, ptr(disp), ptr(z))


def test_the_library_check_accepts_the_defaults_and_refuses_each_error():
    from flvis_amd import FLVIS_ERR_INVALID_ARG, FLVIS_OK, dense_stereo_params
    p = dense_stereo_params()
    assert (p.d_min, p.n_disp, p.agg_r, p.uniq, p.lr_tol) == (0, 64, 2, 10, 1)
    assert _check() == FLVIS_OK
    assert _check(n_cam=2, cam=((30.0, 1000.0), (31.0, 5000.0))) == FLVIS_OK
    assert _check(n_disp=1) == FLVIS_OK and _check(n_disp=256) == FLVIS_OK and _check(agg_r=0) == FLVIS_OK and _check(agg_r=4) == FLVIS_OK
    assert _check(uniq=0) == FLVIS_OK and _check(uniq=99) == FLVIS_OK and _check(lr_tol=-1) == FLVIS_OK and _check(lr_tol=0) == FLVIS_OK
    assert _check(disp=0) == FLVIS_OK and _check(z=0) == FLVIS_OK
    assert _check(w=5, h=3) == FLVIS_OK, "an image too small for a valid pixel is not an error"
    bad = [dict(n_disp=0), dict(n_disp=257), dict(d_min=-1), dict(agg_r=-1), dict(agg_r=5), dict(uniq=-1), dict(uniq=100), dict(lr_tol=-2),
           dict(w=0), dict(h=0), dict(n_img=0), dict(w=-3), dict(cam=((float("nan"), 1000.0),)), dict(cam=((30.0, float("inf")),)),
           dict(cam=((0.0, 1000.0),)), dict(cam=((30.0, -1.0),)), dict(n_cam=2, cam=((30.0, 1000.0), (30.0, 0.0))), dict(disp=0, z=0),
           dict(img0=0), dict(img1=0), dict(cam=None), dict(prm=False), dict(n_cam=3, cam=((30.0, 1000.0),) * 3), dict(d_min=4000, n_disp=200)]
    for kw in bad:
        assert _check(**kw) == FLVIS_ERR_INVALID_ARG, kw
