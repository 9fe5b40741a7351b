"""CPU: the occupancy map's restatement (tests/_occupancy.py) against its second write-up, proof that every edge case reaches its edge,
and the host part of flvis_hip_occupancy's argument checks (flvis_occupancy_check, no device)."""
import ctypes as C

import numpy as np
import pytest

import _depth_cloud as DC
import _map_cloud as MC
import _occupancy as OC

RANDOM = [dict(seed=3, n=3, h=37, w=70, step=(7, 7)), dict(seed=4, n=3, h=24, w=33, step=(1, 1))]
F32 = np.float32


def _l(r, key):
    i = np.flatnonzero(r["keys"] == key)
    assert len(i) == 1, "the voxel is in the map"
    return r["l"][i[0]]


@pytest.mark.parametrize("leaf", [0.08, 0.125])
@pytest.mark.parametrize("spec", RANDOM, ids=["37x70 step 7", "24x33 step 1"])
def test_the_two_write_ups_agree_on_random_cases(spec, leaf):
    case = OC.random_case(**spec)
    a, b = OC.restate(case, 0, leaf), OC.restate_loops(case, 0, leaf)
    OC.same(a, b, (spec, leaf))
    assert a["n_rays"] > 100 and a["n_dropped"] == 0 and a["n_out"] > a["n_rays"]
    assert (a["l"] > 0).any() and (a["l"] < 0).any()


@pytest.mark.parametrize("leaf", [0.08, 0.125])
def test_every_walk_ends_in_the_end_cell_and_visits_rem_plus_one_distinct_cells(leaf):
    case = OC.random_case(**RANDOM[1])
    for image in range(3):
        o, p, _ = OC.scan_rays(case, image, case["cams"][0], leaf)
        free, hit, steps = OC.walk(o, p, leaf)                      # (asserts that every ray ends in its end cell)
        for r in range(0, len(o), 37):
            cells_free, cell_hit = OC.walk_loops(tuple(o[r]), tuple(p[r]), leaf)
            assert len(cells_free) == steps[r] and len(set(cells_free + [cell_hit])) == steps[r] + 1
            assert int(OC.key_of(cell_hit)) == hit[r]
        assert sum(len(f) for f in free) == steps.sum()


def test_an_exact_tie_goes_to_the_lowest_axis():
    leaf = 0.125
    case = OC.diagonal_case(leaf)
    o, p, _ = OC.scan_rays(case, 0, case["cams"][0], leaf)
    assert o.tolist() == [[leaf / 2] * 3] and p.tolist() == [[4.5 * leaf] * 3]
    trace = []
    OC.walk(o, p, leaf, trace)
    assert len(trace) == 12
    _, axis, tmax = trace[0]
    assert tmax[0, 0] == tmax[0, 1] == tmax[0, 2] == 0.125 and axis[0] == 0, "three equal tmax: x goes first"
    assert [int(t[1][0]) for t in trace] == [0, 1, 2] * 4
    _, axis, tmax = trace[1]
    assert tmax[0, 1] == tmax[0, 2] < tmax[0, 0] and axis[0] == 1
    free, hit = OC.walk_loops(tuple(o[0]), tuple(p[0]), leaf)
    assert free[:4] == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)] and hit == (4, 4, 4)
    OC.same(OC.restate(case, 0, leaf), OC.restate_loops(case, 0, leaf), "diagonal")


def test_an_origin_on_a_voxel_face_walking_down_has_tmax_zero():
    leaf = 0.125
    case = OC.face_case(leaf)
    o, p, _ = OC.scan_rays(case, 0, case["cams"][0], leaf)
    assert o[0, 0] == 2 * leaf and p[0, 0] < o[0, 0]
    trace = []
    OC.walk(o, p, leaf, trace)
    assert trace[0][2][0, 0] == 0.0 and trace[0][1][0] == 0, "tmax.x == 0: the first step leaves the origin's cell along x"
    free, hit = OC.walk_loops(tuple(o[0]), tuple(p[0]), leaf)
    assert free[0] == (2, 0, 0) and free[1] == (1, 0, 0) and hit == (-2, 0, 4)
    OC.same(OC.restate(case, 0, leaf), OC.restate_loops(case, 0, leaf), "face")


def test_an_axis_parallel_and_a_zero_step_ray():
    leaf = 0.125
    case = OC.ray_case([1.0, 0.05], origins=[[leaf / 2] * 3] * 2)
    o, p, _ = OC.scan_rays(case, 0, case["cams"][0], leaf)
    free, hit = OC.walk_loops(tuple(o[0]), tuple(p[0]), leaf)
    assert free == [(0, 0, k) for k in range(8)] and hit == (0, 0, 8), "axis-parallel: only z steps"
    o, p, _ = OC.scan_rays(case, 1, case["cams"][0], leaf)
    free, hit = OC.walk_loops(tuple(o[0]), tuple(p[0]), leaf)
    assert free == [] and hit == (0, 0, 0), "zero steps: a hit and no free cell"
    one = dict(case, clouds=[[(1, 1)]])
    r = OC.restate(one, 0, leaf)
    assert r["n_out"] == 1 and r["l"][0] == F32(0.85) and r["records"] == 1
    for c in (case, one):
        OC.same(OC.restate(c, 0, leaf), OC.restate_loops(c, 0, leaf), "rays")


def test_a_voxel_crossed_and_ended_in_within_one_scan_is_one_hit():
    leaf = 0.125
    case, key = OC.crossed_and_hit_case(leaf)
    o, p, _ = OC.scan_rays(case, 0, case["cams"][0], leaf)
    free, hit, _ = OC.walk(o, p, leaf)
    assert hit[0] == key and any(key in f for f in free), "ray 0 ends in the voxel, ray 1 crosses it"
    free1, _ = OC.walk_loops(tuple(o[1]), tuple(p[1]), leaf)
    assert (0, 0, 8) in free1
    r = OC.restate(case, 0, leaf)
    assert _l(r, key) == F32(0.85)
    OC.same(r, OC.restate_loops(case, 0, leaf), "crossed and hit")


def test_the_origin_voxel_gets_one_miss_per_scan_however_many_rays():
    leaf = 0.125
    case = OC.random_case(**RANDOM[1])
    one = dict(case, clouds=[[(0, 1)]])
    o, _, _ = OC.scan_rays(one, 0, one["cams"][0], leaf)
    r = OC.restate(one, 0, leaf)
    assert len(o) > 500 and _l(r, int(OC.key_of(OC.cells(o[:1], leaf)[1][0]))) == F32(-0.4)


def test_saturation_reaches_both_clamps_exactly():
    leaf = 0.125
    r = OC.restate(OC.wall_scans(6, leaf), 0, leaf)
    wall = OC.index_of(r["keys"])[:, 2] == 8
    assert wall.sum() == 63 and (r["l"][wall] == F32(3.5)).all()
    assert _l(r, int(OC.key_of([0, 0, 0]))) == F32(-2.0) and (r["l"][~wall] == F32(-2.0)).all()
    r4 = OC.restate(OC.wall_scans(4, leaf), 0, leaf)
    assert (r4["l"][OC.index_of(r4["keys"])[:, 2] == 8] == F32(0.85) + F32(0.85) + F32(0.85) + F32(0.85)).all(), "four scans: not clamped yet"
    OC.same(r, OC.restate_loops(OC.wall_scans(6, leaf), 0, leaf), "wall")


def test_the_scan_order_is_load_bearing():
    leaf = 0.125
    a, key = OC.order_case(True, leaf)
    b, _ = OC.order_case(False, leaf)
    la, lb = _l(OC.restate(a, 0, leaf), key), _l(OC.restate(b, 0, leaf), key)
    assert la == F32(F32(3.5) + F32(-0.4)) and lb == F32(3.5) and la != lb
    OC.same(OC.restate(a, 0, leaf), OC.restate_loops(a, 0, leaf), "order")


def test_chaining_at_every_split_equals_the_whole():
    leaf = 0.08
    case = OC.random_case(seed=9, n=4, h=37, w=70, step=(7, 7))
    whole = OC.restate(case, 0, leaf)
    for k in range(5):
        first = OC.restate(case, 0, leaf, scans=slice(0, k))
        both = OC.restate(case, 0, leaf, prior=(first["keys"], first["l"]), scans=slice(k, 4))
        assert np.array_equal(both["keys"], whole["keys"]) and both["l"].tobytes() == whole["l"].tobytes(), k
    half = OC.restate(case, 0, leaf, scans=slice(0, 2))
    OC.same(OC.restate_loops(dict(case, clouds=[[(2, 2)]]), 0, leaf, prior=(half["keys"], half["l"])),
            dict(whole, n_rays=whole["n_rays"] - half["n_rays"]), "the second write-up's prior")


def test_an_image_listed_twice_is_two_scans():
    leaf = 0.125
    case = OC.random_case(seed=6, n=1, h=24, w=33, step=(1, 1))
    twice = dict(case, clouds=[[(0, 1), (0, 1)]], cams=case["cams"] * 2)
    copies = dict(case, depth=np.repeat(case["depth"], 2, axis=0), T=np.repeat(case["T"], 2, axis=0), clouds=[[(0, 2)]])
    a, b, once = OC.restate(twice, 0, leaf), OC.restate(copies, 0, leaf), OC.restate(case, 0, leaf)
    OC.same(a, b, "twice")
    assert np.array_equal(a["keys"], once["keys"]) and (a["l"] != once["l"]).all() and a["n_rays"] == 2 * once["n_rays"]
    OC.same(a, OC.restate_loops(twice, 0, leaf), "twice, loops")


def test_argument_errors_without_a_device():
    """flvis_occupancy_check is the host part of flvis_hip_occupancy's checks; the entries themselves refuse a NULL context / closer"""
    import flvis_amd
    lib = flvis_amd.load_library()
    ints = lambda *v: (C.c_int * len(v))(*v)  # noqa: E731
    i64 = lambda *v: (C.c_int64 * len(v))(*v)  # noqa: E731
    dbl = lambda *v: (C.c_double * len(v))(*v)  # noqa: E731
    P, O = flvis_amd.DepthCloudParams, flvis_amd.OccupancyParams
    good = dict(n_img=10, w=70, h=37, n_maps=2, ptr=ints(0, 1, 3), rng=ints(0, 4, 2, 2, 9, 1), cams=dbl(*(DC.CAM_A + DC.CAM_B + DC.CAM_A)),
                prm=P(0, 0, 0, 0, 1, 1, 0.3, 10.0), leaf=0.08, occ=flvis_amd.occupancy_params(), prior_cap=7, n_prior=i64(0, 7), out_cap=5)
    order = ("n_img", "w", "h", "n_maps", "ptr", "rng", "cams", "prm", "leaf", "occ", "prior_cap", "n_prior", "out_cap")

    def call(**kw):
        a = dict(good, **kw)
        for k in ("prm", "occ"):
            a[k] = C.byref(a[k]) if a[k] is not None else None
        return lib.flvis_occupancy_check(*[a[k] for k in order])

    d = flvis_amd.occupancy_params()
    assert [F32(v) for v in (d.l_hit, d.l_miss, d.l_min, d.l_max)] == [F32(0.85), F32(-0.4), F32(-2.0), F32(3.5)]
    assert call() == flvis_amd.FLVIS_OK and call(n_prior=None, prior_cap=0) == flvis_amd.FLVIS_OK
    nan, inf = float("nan"), float("inf")
    bad = [dict(leaf=0.0), dict(leaf=-0.08), dict(leaf=nan), dict(leaf=inf), dict(occ=None), dict(occ=O(0.0, -0.4, -2.0, 3.5)),
           dict(occ=O(0.85, 0.0, -2.0, 3.5)), dict(occ=O(0.85, -0.4, 0.0, 3.5)), dict(occ=O(0.85, -0.4, -2.0, 0.0)), dict(occ=O(nan, -0.4, -2.0, 3.5)),
           dict(occ=O(0.85, -inf, -2.0, 3.5)), dict(occ=O(0.85, -0.4, nan, 3.5)), dict(occ=O(0.85, -0.4, -2.0, inf)), dict(n_prior=i64(0, 8)),
           dict(n_prior=i64(-1, 0)), dict(prior_cap=-1), dict(out_cap=-1),
           # ... and flvis_hip_depth_cloud's
           dict(prm=P(0, 0, 0, 0, 0, 1, 0.3, 10.0)), dict(prm=P(0, 0, 71, 0, 1, 1, 0.3, 10.0)), dict(prm=P(0, 0, 0, 0, 1, 1, 2.0, 1.0)), dict(prm=None),
           dict(cams=dbl(*([61.5, 0.0, 33.7, 18.2, 1000.0] * 3))), dict(cams=None), dict(w=0), dict(rng=ints(0, 4, 2, 2, 9, 2)), dict(ptr=ints(1, 1, 3)),
           dict(n_maps=0)]
    for kw in bad:
        assert call(**kw) == flvis_amd.FLVIS_ERR_INVALID_ARG, kw
    one = i64(0)
    assert lib.flvis_hip_occupancy(None, None, None, 1, 70, 37, 1, ints(0, 1), ints(0, 1), good["cams"], C.byref(good["prm"]), 0.08,
                                   C.byref(good["occ"]), None, None, 0, None, 0, None, None, None, one, None, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_keyframe_log_occupancy(None, 1, ints(0), None, C.byref(good["prm"]), 0.08, C.byref(good["occ"]), 0, 0, None, None, None, one,
                                            None, None, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_occupancy(None, 1, ints(0, 1), ints(0), None, C.byref(good["prm"]), 0.08, C.byref(good["occ"]), 0, 0, None, None,
                                           None, one, None, None, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    info = flvis_amd.occupancy_info()
    assert info["workgroup"] == 256 and info["bytes_per_record"] == 32 and info["bytes_per_ray"] == 0 and info["bytes_per_image"] == 20
    assert MC.HALF == 1 << 20
