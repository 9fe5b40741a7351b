"""GPU: flvis_hip_depth_cloud (include/flvis_hip.h) against its restatement (tests/_depth_cloud.py, which ends in _map_cloud.restate), bit
for bit: rows, counts per voxel, n_out, n_dropped, n_valid.  Small images whose width is neither a multiple of 64 nor of the step, more
than one row chunk per image (129 x 96 at step 1), every edge case of test_depth_cloud_inputs.py, and one 640 x 480 image at step 1 whose
samples cross the sort tile."""
import numpy as np
import pytest

import _depth_cloud as DC
import _map_cloud as MC

pytestmark = pytest.mark.gpu

INV = -1
SHAPES = [(70, 37), (129, 96)]          # (w, h)


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _dev(case):
    import torch
    d = torch.from_numpy(case["depth"].view(np.int16).copy()).cuda()
    return d, torch.from_numpy(np.ascontiguousarray(case["T"], np.float64)).cuda()


def _run(ctx, case, leaf, min_points=1, cap=None, dev=None, clouds=None, cams=None):
    d, T = dev or _dev(case)
    p = case["prm"]
    return ctx.depth_cloud(d, T, clouds or case["clouds"], cams or case["cams"], window=(p["u0"], p["v0"], p["u1"], p["v1"]),
                           step=(p["step_u"], p["step_v"]), z_min=p["z_min"], z_max=p["z_max"], leaf=leaf, min_points=min_points, cap=cap)


def _check(got, c, want, what):
    xyz, npts, n_out, n_drop, n_valid = got
    assert (int(n_out[c]), int(n_drop[c]), int(n_valid[c])) == (want["n_out"], want["n_dropped"], want["n_valid"]), \
        (what, int(n_out[c]), int(n_drop[c]), int(n_valid[c]), want["n_out"], want["n_dropped"], want["n_valid"])
    assert xyz[c].shape == want["xyz"].shape and xyz[c].tobytes() == want["xyz"].tobytes(), (what, "rows")
    assert np.array_equal(npts[c], want["npts"]), (what, "npts")


def _check_case(ctx, case, leaves, what, min_points=1):
    dev = _dev(case)
    for leaf in leaves:
        got = _run(ctx, case, leaf, min_points, dev=dev)
        for c in range(len(case["clouds"])):
            _check(got, c, DC.restate(case, c, leaf, min_points), (what, leaf, c))


@pytest.mark.parametrize("step", [(1, 1), (7, 7), (3, 5)])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_images_under_random_poses(ctx, shape, step):
    """leaf 0 checks the raster order itself; the window ends mid-step"""
    w, h = shape
    case = DC.random_case(10 * w + step[0], 3, h, w, DC.params((1, 2, w - 1, h - 1), step))
    assert step == (1, 1) or ((w - 2) % step[0] and (h - 3) % step[1]), "the window ends mid-step on both axes"
    _check_case(ctx, case, (0.0, 0.125, 0.08), (shape, step))


def test_the_edge_cases(ctx):
    cases = {"zmin 0.3": DC.limit_case(0.3)[0], "zmin 0.5": DC.limit_case(0.5)[0], "empty between": DC.empty_between_case(),
             "65 apart": DC.apart_case(65), "64 apart": DC.apart_case(64), "first and last": DC.first_last_case(),
             "whole image, no valid sample": DC.one_cloud(np.zeros((2, 37, 70), np.uint16))}
    for name, case in cases.items():
        _check_case(ctx, case, (0.0, 0.08), name)
    got = _run(ctx, cases["whole image, no valid sample"], 0.08)
    assert got[2][0] == 0 and got[4][0] == 0 and len(got[0][0]) == 0


def test_a_flat_wall_fills_voxels_with_hundreds_of_samples(ctx):
    """the sum of a voxel is sequential in canonical order: hundreds of samples of ONE image per voxel, and three images per voxel"""
    rng = np.random.default_rng(8)
    d = DC.wall(rng, 3, 96, 129, raw=500, spread=5, holes=0.05)
    case = DC.one_cloud(d, cam=[120.0, 118.0, 64.2, 47.9, 1000.0])
    want = DC.restate(case, 0, 0.125)
    assert want["npts"].max() >= 300, want["npts"].max()
    _check_case(ctx, case, (0.125, 0.08), "wall")
    _check_case(ctx, case, (0.125,), "wall, min_points", min_points=200)


def test_two_cameras_shared_images_and_batch_against_single_calls(ctx):
    """ranges on two cameras in one cloud, an image in two clouds (once per camera), an empty cloud; and the batch equals single calls"""
    prm = DC.params((0, 1, 70, 37), (3, 5))
    clouds = [[(0, 2), (3, 1)], [(1, 2)], [], [(2, 0)], [(3, 1), (0, 1)]]
    cams = [DC.CAM_A, DC.CAM_B, DC.CAM_B, DC.CAM_A, DC.CAM_A, DC.CAM_B]
    case = DC.random_case(77, 4, 37, 70, prm, cams=cams, clouds=clouds)
    dev = _dev(case)
    for leaf in (0.0, 0.08):
        got = _run(ctx, case, leaf, dev=dev)
        for c in range(len(clouds)):
            _check(got, c, DC.restate(case, c, leaf), ("batch", leaf, c))
        assert got[2][2] == 0 and got[2][3] == 0
        r0 = 0
        for c, cl in enumerate(clouds):
            if cl:
                one = _run(ctx, case, leaf, dev=dev, clouds=[cl], cams=cams[r0:r0 + len(cl)])
                assert one[0][0].tobytes() == got[0][c].tobytes() and np.array_equal(one[1][0], got[1][c]) and one[2][0] == got[2][c]
            r0 += len(cl)
        again = _run(ctx, case, leaf, dev=dev)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[0], got[0]))


def test_out_cap_below_at_and_above_and_the_dropped_count(ctx):
    """an image whose pose puts its points outside the voxel range: dropped, not valid-less"""
    case = DC.random_case(31, 2, 37, 70, DC.params(step=(3, 5)))
    case["T"][1, :3] = [1.0e6, 0, 0]
    leaf = 0.08
    want = DC.restate(case, 0, leaf)
    n1 = len(DC.samples(case["depth"][1], case["cams"][0], case["prm"])[0])
    assert want["n_dropped"] == n1 > 0 and want["n_out"] > 8
    dev = _dev(case)
    for cap in (want["n_out"] - 5, want["n_out"], want["n_out"] + 7, 0):
        xyz, npts, n_out, n_drop, n_valid = _run(ctx, case, leaf, cap=cap, dev=dev)
        k = min(cap, want["n_out"])
        assert (n_out[0], n_drop[0], n_valid[0]) == (want["n_out"], want["n_dropped"], want["n_valid"])
        assert xyz[0].tobytes() == want["xyz"][:k].tobytes() and np.array_equal(npts[0], want["npts"][:k])
    _check(_run(ctx, case, 0.0, dev=dev), 0, DC.restate(case, 0, 0.0), "leaf 0: only finite coordinates")


def test_equals_the_voxel_call_fed_the_restated_rows(ctx):
    import torch
    case = DC.random_case(55, 3, 96, 129, DC.params((1, 2, 127, 95), (3, 5)), cams=(DC.CAM_A, DC.CAM_B), clouds=[[(0, 2), (1, 2)]])
    mc, n_valid = DC.rows_case(case, 0)
    for leaf in (0.0, 0.08):
        got = _run(ctx, case, leaf)
        vx, vn, v_out, v_drop = ctx.voxel_cloud(torch.from_numpy(mc["p3"]).cuda(), torch.from_numpy(mc["count"]).cuda(),
                                                torch.from_numpy(mc["T"]).cuda(), [[(0, len(mc["count"]))]], leaf=leaf)
        assert got[0][0].tobytes() == vx[0].tobytes() and np.array_equal(got[1][0], vn[0]) and got[2][0] == v_out[0] and got[3][0] == v_drop[0]
        assert got[4][0] == n_valid == int(mc["count"].sum())


def test_a_vga_image_at_step_1_crosses_the_sort_tile(ctx):
    import flvis_amd
    rng = np.random.default_rng(12)
    d = DC.wall(rng, 1, 480, 640, raw=2500, spread=60, holes=0.03)
    case = DC.one_cloud(d, cam=[385.0, 385.5, 321.3, 238.9, 1000.0], T=MC.random_unit_poses(rng, 1))
    want = DC.restate(case, 0, 0.08)
    tile = flvis_amd.voxel_cloud_info()["sort_tile"]
    assert want["n_valid"] > 64 * tile
    _check(_run(ctx, case, 0.08), 0, want, "vga")
    st = ctx.voxel_cloud_stats()
    assert st["input_points"] == want["n_valid"] and st["passes_run"] >= 2
    assert st["workspace_bytes"] >= 48 * want["n_valid"]


def test_argument_errors_leave_the_context_usable(ctx):
    import flvis_amd
    case = DC.random_case(9, 2, 37, 70, DC.params(step=(7, 7)))
    dev = _dev(case)
    want = DC.restate(case, 0, 0.08)
    bad = [dict(step=(0, 1)), dict(window=(0, 0, 71, 37)), dict(window=(5, 0, 5, 37)), dict(z_min=float("nan")), dict(z_min=2.0, z_max=1.0),
           dict(cams=[[61.5, 0.0, 33.7, 18.2, 1000.0]]), dict(cams=[[61.5, 60.0, 33.7, 18.2, 0.0]]), dict(leaf=-1.0), dict(min_points=0),
           dict(clouds=[[(1, 2)]])]
    for kw in bad:
        a = dict(dict(clouds=case["clouds"], cams=case["cams"], window=None, step=(7, 7), z_min=0.3, z_max=10.0, leaf=0.08, min_points=1), **kw)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            ctx.depth_cloud(dev[0], dev[1], a.pop("clouds"), a.pop("cams"), **a)
        _check(_run(ctx, case, 0.08, dev=dev), 0, want, ("after", kw))
