"""GPU: flvis_hip_occupancy (include/flvis_hip.h) against its restatement (tests/_occupancy.py), bit for bit: keys, values, centres, n_out,
n_rays, n_dropped.  The random cases and every edge case of test_occupancy_inputs.py, several maps in one call, out_cap, dropped rays, the
prior on the device, and one image whose origin voxel alone holds a run of more than 10 000 records behind the sort."""
import numpy as np
import pytest

import _depth_cloud as DC
import _occupancy as OC

pytestmark = pytest.mark.gpu

INV = -1
F32 = np.float32


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


def _run(ctx, case, leaf, dev=None, maps=None, cams=None, **kw):
    d, T = dev or _dev(case)
    p = case["prm"]
    return ctx.occupancy(d, T, maps or case["clouds"], cams or case["cams"], window=(p["u0"], p["v0"], p["u1"], p["v1"]),
                         step=(p["step_u"], p["step_v"]), z_min=p["z_min"], z_max=p["z_max"], leaf=leaf, **kw)


def _check(got, m, want, what, k=None):
    keys, l, xyz, n_out, n_rays, n_drop = got
    assert (int(n_out[m]), int(n_rays[m]), int(n_drop[m])) == (want["n_out"], want["n_rays"], want["n_dropped"]), \
        (what, int(n_out[m]), int(n_rays[m]), int(n_drop[m]), want["n_out"], want["n_rays"], want["n_dropped"])
    k = want["n_out"] if k is None else k
    assert np.array_equal(keys[m], want["keys"][:k]), (what, "keys")
    assert l[m].tobytes() == want["l"][:k].tobytes(), (what, "values")
    assert xyz[m].tobytes() == want["xyz"][:k].tobytes(), (what, "centres")


def _check_case(ctx, case, leaves, what):
    dev = _dev(case)
    for leaf in leaves:
        got = _run(ctx, case, leaf, dev=dev)
        for m in range(len(case["clouds"])):
            _check(got, m, OC.restate(case, m, leaf), (what, leaf, m))


@pytest.mark.parametrize("poses", [True, False], ids=["random poses", "identity"])
@pytest.mark.parametrize("leaf", [0.08, 0.125])
@pytest.mark.parametrize("spec", [dict(seed=3, n=3, h=37, w=70, step=(7, 7)), dict(seed=4, n=3, h=24, w=33, step=(1, 1))],
                         ids=["37x70 step 7", "24x33 step 1"])
def test_random_cases(ctx, spec, leaf, poses):
    _check_case(ctx, OC.random_case(poses=poses, **spec), (leaf,), (spec, poses))


def test_the_edge_cases(ctx):
    leaf = 0.125
    cases = {"diagonal tie": OC.diagonal_case(leaf), "origin on a face": OC.face_case(leaf),
             "axis-parallel and zero-step": OC.ray_case([1.0, 0.05], origins=[[leaf / 2] * 3] * 2),
             "zero-step alone": dict(OC.ray_case([1.0, 0.05], origins=[[leaf / 2] * 3] * 2), clouds=[[(1, 1)]]),
             "crossed and hit": OC.crossed_and_hit_case(leaf)[0], "wall, six scans": OC.wall_scans(6, leaf),
             "hits then miss": OC.order_case(True, leaf)[0], "miss then hits": OC.order_case(False, leaf)[0],
             "no valid sample": DC.one_cloud(np.zeros((2, 37, 70), np.uint16))}
    one = OC.random_case(seed=6, n=1, h=24, w=33, step=(1, 1))
    cases["listed twice"] = dict(one, clouds=[[(0, 1), (0, 1)]], cams=one["cams"] * 2)
    for name, case in cases.items():
        _check_case(ctx, case, (leaf,), name)
    got = _run(ctx, cases["no valid sample"], leaf)
    assert got[3][0] == 0 and got[4][0] == 0 and len(got[0][0]) == 0
    wall = _run(ctx, cases["wall, six scans"], leaf)
    assert wall[1][0].max() == F32(3.5) and wall[1][0].min() == F32(-2.0)


def test_two_cameras_shared_images_and_three_maps_against_single_calls(ctx):
    maps = [[(0, 2), (3, 1)], [(1, 2)], [], [(3, 1), (0, 1)]]
    cams = [DC.CAM_A, DC.CAM_B, DC.CAM_B, DC.CAM_A, DC.CAM_B]
    case = OC.random_case(seed=77, n=4, h=37, w=70, step=(3, 5), cams=cams, clouds=maps)
    dev = _dev(case)
    leaf = 0.08
    got = _run(ctx, case, leaf, dev=dev)
    r0 = 0
    for m, mp in enumerate(maps):
        _check(got, m, OC.restate(case, m, leaf), ("batch", m))
        if mp:
            one = _run(ctx, case, leaf, dev=dev, maps=[mp], cams=cams[r0:r0 + len(mp)])
            assert np.array_equal(one[0][0], got[0][m]) and one[1][0].tobytes() == got[1][m].tobytes() and one[3][0] == got[3][m]
        r0 += len(mp)
    assert got[3][2] == 0
    again = _run(ctx, case, leaf, dev=dev)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[0] + again[1] + again[2], got[0] + got[1] + got[2]))


def test_out_cap_below_at_and_above_and_the_dropped_rays(ctx):
    """an image whose pose puts its rays outside the voxel range: dropped, and counted"""
    case = OC.random_case(seed=31, n=2, h=37, w=70, step=(3, 5))
    case["T"][1, :3] = [1.0e6, 0, 0]
    leaf = 0.08
    want = OC.restate(case, 0, leaf)
    n1 = len(DC.samples(case["depth"][1], case["cams"][0], case["prm"])[0])
    assert want["n_dropped"] == n1 > 0 and want["n_rays"] > 0 and want["n_out"] > 8
    dev = _dev(case)
    for cap in (want["n_out"] - 5, want["n_out"], want["n_out"] + 7, 0):
        _check(_run(ctx, case, leaf, dev=dev, cap=cap), 0, want, ("cap", cap), k=min(cap, want["n_out"]))
    assert _run(ctx, case, leaf, dev=dev, centres=False)[2] is None


def test_the_prior_on_the_device(ctx):
    import flvis_amd
    leaf = 0.08
    case = OC.random_case(seed=9, n=4, h=37, w=70, step=(7, 7))
    dev = _dev(case)
    whole = OC.restate(case, 0, leaf)
    _check(_run(ctx, case, leaf, dev=dev), 0, whole, "whole")
    for k in (1, 2, 3):
        first = _run(ctx, case, leaf, dev=dev, maps=[[(0, k)]])
        both = _run(ctx, case, leaf, dev=dev, maps=[[(k, 4 - k)]], prior=[(first[0][0], first[1][0])])
        assert np.array_equal(both[0][0], whole["keys"]) and both[1][0].tobytes() == whole["l"].tobytes() \
            and both[2][0].tobytes() == whole["xyz"].tobytes(), k
    # a prior voxel that nothing observes comes out unchanged, in its place; two maps with priors of different lengths
    far = np.array([int(OC.key_of([-1000, 5, 7])), int(OC.key_of([900000, -3, 2]))], np.int64)
    far.sort()
    pl = np.array([1.25, -0.75], F32)
    maps = [[(0, 2)], [(2, 2)]]
    two = dict(case, clouds=maps, cams=case["cams"] * 2)
    got = _run(ctx, two, leaf, dev=dev, prior=[(far, pl), (far[:1], pl[:1])])
    for m, (pk, pv) in enumerate([(far, pl), (far[:1], pl[:1])]):
        want = OC.restate(two, m, leaf, prior=(pk, pv))
        _check(got, m, want, ("far prior", m))
        for k_, v_ in zip(pk, pv):
            assert got[1][m][np.flatnonzero(got[0][m] == k_)[0]] == v_
    # keys that do not ascend are refused after the device check, and nothing is written
    for bad in (far[::-1].copy(), np.array([far[0], far[0]], np.int64), np.array([-5, far[1]], np.int64)):
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            _run(ctx, case, leaf, dev=dev, prior=[(bad, pl)], cap=whole["n_out"] + 2)
    _check(_run(ctx, case, leaf, dev=dev), 0, whole, "after a refused prior")


def test_the_hazard_case_one_run_of_more_than_10000_records(ctx):
    import flvis_amd
    leaf = 0.05
    case = OC.hazard_case()
    want = OC.restate(case, 0, leaf)
    assert want["records"] > 16 * flvis_amd.voxel_cloud_info()["sort_tile"], "the records cross the sort tile"
    assert want["n_rays"] > 10000, "every ray starts in the origin voxel: its run behind the sort holds one record per ray"
    o = OC.scan_rays(case, 0, case["cams"][0], leaf)[0]
    origin = int(OC.key_of(OC.cells(o[:1], leaf)[1][0]))
    _check(_run(ctx, case, leaf), 0, want, "hazard")
    assert want["l"][np.flatnonzero(want["keys"] == origin)[0]] == F32(-0.4)
    st = ctx.occupancy_stats()
    assert st["records"] == want["records"] and st["rays"] == want["n_rays"] and st["batches"] == 1
    assert st["workspace_bytes"] >= flvis_amd.occupancy_info()["bytes_per_record"] * want["records"]


def test_argument_errors_leave_the_context_usable(ctx):
    import flvis_amd
    case = OC.random_case(seed=9, n=2, h=37, w=70, step=(7, 7))
    dev = _dev(case)
    want = OC.restate(case, 0, 0.08)
    O = flvis_amd.OccupancyParams
    bad = [dict(leaf=0.0), dict(leaf=-1.0), dict(leaf=float("nan")), dict(occ=O(0.0, -0.4, -2.0, 3.5)), dict(occ=O(0.85, 0.4, -2.0, 3.5)),
           dict(occ=O(0.85, -0.4, 2.0, 3.5)), dict(occ=O(0.85, -0.4, -2.0, float("inf"))), dict(step=(0, 1)), dict(window=(0, 0, 71, 37)),
           dict(z_min=2.0, z_max=1.0), dict(cams=[[61.5, 0.0, 33.7, 18.2, 1000.0]]), dict(maps=[[(1, 2)]])]
    for kw in bad:
        a = dict(dict(maps=case["clouds"], cams=case["cams"], window=None, step=(7, 7), z_min=0.3, z_max=6.5, leaf=0.08), **kw)
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            ctx.occupancy(dev[0], dev[1], a.pop("maps"), a.pop("cams"), **a)
        _check(_run(ctx, case, 0.08, dev=dev), 0, want, ("after", kw))
