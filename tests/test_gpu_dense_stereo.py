"""GPU: flvis_hip_dense_stereo (include/flvis_hip.h) against its restatement (tests/_dense_stereo.py), bit for bit on both outputs:
small pairs whose width is neither a multiple of 64 nor of the tile, every radius, every edge case of test_dense_stereo_inputs.py, the
ends of the disparity range, the smallest heights, flat and periodic textures, an occlusion, batching, and a 640-wide rendered band
(three column tiles, 64 disparities)."""
import numpy as np
import pytest

import _dense_stereo as DS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _run(ctx, case, want_disp=True, want_z=True, cams=None):
    import torch
    i0, i1 = torch.from_numpy(case["img0"]).cuda(), torch.from_numpy(case["img1"]).cuda()
    cams = np.asarray(case["cams"] if cams is None else cams, np.float64).reshape(-1, 2)
    p = case["prm"]
    d, z = ctx.dense_stereo(i0, i1, cams[:, 0], cams[:, 1], p["d_min"], p["n_disp"], p["agg_r"], p["uniq"], p["lr_tol"], want_disp=want_disp,
                            want_z=want_z)
    ctx.synchronize()
    u16 = lambda t: None if t is None else t.cpu().numpy().view(np.uint16)
    return u16(d), u16(z)


def _same(got, want, what):
    for k, name in enumerate(("disp16", "z16")):
        if got[k] is None:
            continue
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, name, len(bad), [(tuple(int(x) for x in b), int(got[k][tuple(b)]), int(want[k][tuple(b)])) for b in bad[:5]])


def _check_case(ctx, case, what, some=True):
    want = DS.restate(case)
    assert not some or (want[0] > 0).any(), (what, "the case has no valid pixel")
    _same(_run(ctx, case), want, what)
    return want


@pytest.mark.parametrize("agg_r", [0, 2, 4])
@pytest.mark.parametrize("shape", [(97, 23), (64, 13), (130, 40)])
def test_random_pairs(ctx, shape, agg_r):
    w, h = shape
    _check_case(ctx, DS.random_case(100 * w + agg_r, h, w, agg_r=agg_r, n_disp=16 if w > 64 else 9), (shape, agg_r), some=h - 2 * agg_r > 7)


@pytest.mark.parametrize("agg_r", [1, 3])
def test_the_other_radii_and_a_second_column_tile(ctx, agg_r):
    """300 columns: the second tile starts at 256 - 2 agg_r"""
    _check_case(ctx, DS.random_case(40 + agg_r, 19, 300, agg_r=agg_r, n_disp=12), agg_r)


@pytest.mark.parametrize("name", sorted(DS.edge_cases()))
def test_the_edge_cases(ctx, name):
    _check_case(ctx, DS.edge_cases()[name], name, some=name != "flat")


@pytest.mark.parametrize("n_disp", [1, 2, 3, 256])
def test_the_ends_of_the_disparity_range(ctx, n_disp):
    """1 and 2 disparities leave no interior: all 0.  256 > w crosses four stagings of the other image's census words."""
    want = _check_case(ctx, DS.random_case(20 + n_disp, 23, 97, n_disp=n_disp, d_min=3 if n_disp < 4 else 0), n_disp, some=n_disp > 2)
    assert n_disp > 2 or not want[0].any()


def test_more_disparities_than_one_staging_on_a_wide_pair(ctx):
    """a shift of 70 at n_disp 80: the best lies in the second staging of 64, its neighbours' costs cross the boundary at k = 64"""
    for k in (64, 70):
        a, b = DS.shifted(np.random.default_rng(k), 17, 200, k, noise=5)
        want = _check_case(ctx, DS.one(a, b, n_disp=80), k)
        assert ((want[0] + 8) // 16 == k).sum() > 500


@pytest.mark.parametrize("d_min", [1, 5])
def test_an_offset_search(ctx, d_min):
    _check_case(ctx, DS.random_case(30 + d_min, 23, 97, d_min=d_min, n_disp=7), d_min)


@pytest.mark.parametrize("agg_r", [0, 2])
def test_the_smallest_heights(ctx, agg_r):
    """h = 7 + 2 agg_r leaves exactly one valid row, one less none -- and that is no error"""
    h = 7 + 2 * agg_r
    case = DS.random_case(50 + agg_r, h, 97, agg_r=agg_r)
    want = _check_case(ctx, case, ("one row", agg_r))
    assert (want[0] > 0).any(axis=2).sum() == 1
    less = DS.one(case["img0"][:, :h - 1], case["img1"][:, :h - 1], **case["prm"])
    want = _check_case(ctx, less, ("no row", agg_r), some=False)
    assert not want[0].any() and not want[1].any()
    tiny = DS.one(np.zeros((3, 5), np.uint8), np.zeros((3, 5), np.uint8))
    _check_case(ctx, tiny, "3 x 5", some=False)


def test_flat_and_periodic_textures(ctx):
    want = _check_case(ctx, DS.flat_case(13, 200), "flat", some=False)
    assert not want[0].any()
    for uniq in (0, 10, 99):
        _check_case(ctx, DS.periodic_case(19, 150, uniq=uniq, lr_tol=1), ("period 8", uniq), some=False)


def test_an_occlusion_strip(ctx):
    for tol in (-1, 0, 1, 3):
        _check_case(ctx, DS.occlusion_case(29, 140, lr_tol=tol), ("occlusion", tol))


def test_batching(ctx):
    """3 images with a camera each against three single calls; one camera against the same camera per image; each output alone"""
    case = DS.random_case(77, 23, 97, n=3)
    case["cams"] = np.array([[30.0, 1000.0], [19.2, 5000.0], [42.0, 250.0]])
    want = DS.restate(case)
    both = _run(ctx, case)
    _same(both, want, "three in one call")
    for i in range(3):
        single = dict(case, img0=case["img0"][i:i + 1].copy(), img1=case["img1"][i:i + 1].copy(), cams=case["cams"][i:i + 1])
        got = _run(ctx, single)
        assert np.array_equal(got[0][0], both[0][i]) and np.array_equal(got[1][0], both[1][i]), i
    one = _run(ctx, case, cams=case["cams"][1:2])
    per = _run(ctx, case, cams=np.tile(case["cams"][1:2], (3, 1)))
    assert np.array_equal(one[0], per[0]) and np.array_equal(one[1], per[1]) and np.array_equal(one[0], both[0])
    d_only, z_only = _run(ctx, case, want_z=False), _run(ctx, case, want_disp=False)
    assert d_only[1] is None and z_only[0] is None
    assert np.array_equal(d_only[0], both[0]) and np.array_equal(z_only[1], both[1])
    again = _run(ctx, case)
    assert np.array_equal(again[0], both[0]) and np.array_equal(again[1], both[1])


def test_more_images_than_one_launch_takes(ctx):
    """70 images of 40 x 9: the call runs them 64 at a time"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (70, 9, 40)).astype(np.uint8)
    case = DS.one(a, np.roll(a, -2, axis=2), n_disp=5, agg_r=0, cams=np.stack([np.linspace(20, 40, 70), np.full(70, 1000.0)], 1))
    _check_case(ctx, case, "70 images")


def test_the_rendered_band(ctx):
    i0, i1, _, bf = DS.rendered_band()
    want = _check_case(ctx, DS.one(i0, i1, cams=[[bf, 1000.0]]), "rendered band")
    assert (want[0] > 0).mean() > 0.6


def test_argument_errors_leave_the_context_usable(ctx):
    import flvis_amd
    case = DS.random_case(1, 23, 97)
    want = DS.restate(case)
    for kw in (dict(n_disp=0), dict(n_disp=257), dict(d_min=-1), dict(agg_r=5), dict(uniq=100), dict(lr_tol=-2)):
        with pytest.raises(flvis_amd.FlvisError):
            _run(ctx, dict(case, prm=DS.params(**kw)))
    with pytest.raises(flvis_amd.FlvisError):
        _run(ctx, case, cams=[[float("nan"), 1000.0]])
    with pytest.raises(flvis_amd.FlvisError):
        _run(ctx, case, cams=[[30.0, 0.0]])
    with pytest.raises(flvis_amd.FlvisError):
        _run(ctx, case, want_disp=False, want_z=False)
    _same(_run(ctx, case), want, "after the refusals")
