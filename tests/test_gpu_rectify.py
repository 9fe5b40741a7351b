"""GPU: flvis_hip_rectify (include/flvis_hip.h) against its restatement (tests/_rectify.py), bit for bit on both outputs: every edge case
of test_rectify_inputs.py, sizes from 1 x 1 to 752 x 480 (odd widths take the byte stores, widths that are no multiple of the tile the
tail), one camera, a camera per image, interleaved cameras (runs of length 1 and 2), a run longer than the host leaves whole, batching,
a second run, no `covered` output, and the refusals."""
import functools

import numpy as np
import pytest

import _rectify as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _run(ctx, case, want_covered=True):
    import torch
    dst, cov = ctx.rectify(torch.from_numpy(case["src"]).cuda(), case["cams"], case.get("cam_of"), want_covered=want_covered)
    ctx.synchronize()
    return dst.cpu().numpy(), None if cov is None else cov.cpu().numpy()


def _same(got, want, what):
    for k, name in enumerate(("dst", "covered")):
        if got[k] is None:
            continue
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, name, len(bad), [(tuple(int(x) for x in b), int(got[k][tuple(b)]), int(want[k][tuple(b)])) for b in bad[:5]])


def _check_case(ctx, case, what):
    want = RC.restate(case)
    _same(_run(ctx, case), want, what)
    return want


@pytest.mark.parametrize("name", sorted(RC.edge_cases()))
def test_the_edge_cases(ctx, name):
    want = _check_case(ctx, RC.edge_cases()[name], name)
    assert want[1].any()


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (3, 2), (63, 5), (64, 5), (65, 5), (70, 37), (129, 96)])
def test_sizes(ctx, shape):
    """(w, h): below one thread's four pixels, one short of / exactly / one beyond half a tile row, two column tiles, many row tiles"""
    w, h = shape
    want = _check_case(ctx, RC.lens_case(w, h, n=3, seed=w * 100 + h), shape)
    assert w * h < 10 or (want[1].any() and not want[1].all()), "covered and uncovered pixels both occur"
    # (the lens covers nothing of a 1 x 1 or 1 x 7 image; the identity camera below covers all of every size)
    _check_case(ctx, RC.one(RC.noise(1, 2, h, w), [RC.camera((64.0, 64.0, 0.25 * w, 0.5 * h))]), (shape, "identity"))


@functools.lru_cache(maxsize=None)
def _euroc_cams():
    return RC.cameras_of_cfg(RC.euroc_cfg(0))


def test_the_euroc_size_once(ctx):
    """752 x 480 under the stock rig's two cameras: six column tiles, sixty row tiles"""
    case = RC.one(RC.noise(7, 2, 480, 752), _euroc_cams())
    want = _check_case(ctx, case, "752 x 480")
    assert want[1][0].all() and 0.999 < want[1][1].mean() < 1.0


def test_cameras_per_image_and_interleaved(ctx):
    w, h = 70, 37
    per = RC.lens_case(w, h, n=3, n_cam=3)
    want = _check_case(ctx, per, "a camera per image")
    assert not np.array_equal(want[1][0], want[1][1]) and not np.array_equal(want[1][1], want[1][2])
    mixed = RC.lens_case(w, h, n=5, n_cam=2, cam_of=[0, 1, 0, 1, 1])
    want = _check_case(ctx, mixed, "a, b, a, b, b")
    assert np.array_equal(want[1][0], want[1][2]) and np.array_equal(want[1][1], want[1][4]) and not np.array_equal(want[1][0], want[1][1])
    unused = RC.lens_case(w, h, n=2, n_cam=3, cam_of=[2, 2])
    _check_case(ctx, unused, "cameras that no image names")


def test_a_long_run_of_one_camera(ctx):
    """70 images of one camera: the host cuts the run"""
    _check_case(ctx, RC.lens_case(33, 9, n=70, seed=70), "70 images")
    _check_case(ctx, RC.lens_case(33, 9, n=70, seed=71, n_cam=2, cam_of=[0] * 37 + [1] * 33), "runs of 37 and 33")


def test_batching_a_second_run_and_no_covered_output(ctx):
    case = RC.lens_case(65, 21, n=4, n_cam=2, cam_of=[1, 0, 0, 1])
    want = RC.restate(case)
    both = _run(ctx, case)
    _same(both, want, "four in one call")
    for i in range(4):
        single = RC.one(case["src"][i:i + 1].copy(), case["cams"][case["cam_of"][i]])
        got = _run(ctx, single)
        assert np.array_equal(got[0][0], both[0][i]) and np.array_equal(got[1][0], both[1][i]), i
    again = _run(ctx, case)
    assert np.array_equal(again[0], both[0]) and np.array_equal(again[1], both[1])
    alone = _run(ctx, case, want_covered=False)
    assert alone[1] is None and np.array_equal(alone[0], both[0])


def test_refusals_leave_the_context_usable(ctx):
    import torch
    import flvis_amd
    case = RC.lens_case(37, 23, n=3)
    good = case["cams"][0]

    def broken(i, x):
        c = good.copy()
        c[i] = x
        return c
    for kw in (dict(cams=[broken(0, 0.0)]), dict(cams=[broken(18, -2.0)]), dict(cams=[broken(9, float("nan"))]), dict(cams=[good, good]),
               dict(cams=[good, good], cam_of=[0, 1, 2]), dict(cams=[good], cam_of=[0, -1, 0])):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(-1\)"):
            _run(ctx, dict(case, **kw))
    src = torch.from_numpy(case["src"]).cuda()
    lib, n = flvis_amd.load_library(), int(src.numel())
    cam = np.ascontiguousarray(good)
    for dst, cov in ((src.data_ptr(), 0), (src.data_ptr() + n - 1, 0), (src.data_ptr() + n, src.data_ptr() + 1)):
        rc = lib.flvis_hip_rectify(ctx._h, src.data_ptr(), 3, 37, 23, 1, cam.ctypes.data, None, dst, cov)
        assert rc == flvis_amd.FLVIS_ERR_INVALID_ARG, "in place or overlapping"
    ctx.synchronize()
    assert np.array_equal(src.cpu().numpy(), case["src"]), "nothing was written"
    _same(_run(ctx, case), RC.restate(case), "after the refusals")
