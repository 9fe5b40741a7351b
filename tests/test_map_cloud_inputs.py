"""CPU tests of the voxel cloud's test kit: the numpy restatement (tests/_map_cloud.py) agrees with an independent dictionary-of-voxels
write-up, every edge input of tests/test_gpu_map_cloud.py hits the edge it is named for, the PLY pair round-trips, and the argument errors
of flvis_hip_voxel_cloud that need no device are refused through the C ABI."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _map_cloud as MC


def _same(a, b):
    assert a["n_out"] == b["n_out"] and a["n_dropped"] == b["n_dropped"]
    assert np.array_equal(a["npts"], b["npts"])
    assert np.array_equal(a["xyz"].view(np.uint32), b["xyz"].view(np.uint32))


@pytest.mark.parametrize("leaf,min_points,poses", [(0.08, 1, True), (0.5, 2, True), (0.125, 1, False), (1.0, 3, True)])
def test_restatement_agrees_with_the_dictionary_of_voxels(leaf, min_points, poses):
    case = MC.random_case(21, [40, 0, 64, 70, -2, 13], cap=64, poses=poses)
    case["p3"][2, 5, 1] = np.nan
    case["p3"][3, 9] = [np.inf, 0, 0]
    case["p3"][0, 0] = [4e5, 0, 0]                                    # outside the index range for the small leaves
    for cloud in ([(0, 6)], [(3, 2), (0, 1)], [(2, 1), (2, 1)], [(1, 1)]):
        a, b = MC.restate(case, cloud, leaf, min_points), MC.restate_dict(case, cloud, leaf, min_points)
        _same(a, b)
        assert np.all(np.diff(a["keys"]) > 0)                         # one row per voxel, ascending by key
    full = MC.restate(case, [(0, 6)], leaf, 1)
    assert full["npts"].sum() + full["n_dropped"] == 40 + 64 + 64 + 13 and full["n_dropped"] >= 2


def test_raw_list_is_the_canonical_order():
    case = MC.random_case(22, [3, 0, 2], cap=4, poses=False)
    case["p3"][0, 1, 2] = -np.inf
    r = MC.restate(case, [(2, 1), (0, 2)], 0.0)
    want = np.concatenate([case["p3"][2, :2], case["p3"][0, [0, 2]]]).astype(np.float32)
    assert r["n_dropped"] == 1 and np.array_equal(r["xyz"], want) and np.all(r["npts"] == 1)


def test_identity_pose_returns_the_point():
    p = np.random.default_rng(1).normal(size=(50, 3)) * 10
    assert np.array_equal(MC.transform(p, np.tile(MC.IDENT, (50, 1))), p)


@pytest.mark.parametrize("leaf", [0.125, 0.08])
def test_boundary_points_land_in_the_stated_voxel(leaf):
    for name, (v, want) in MC.boundary_values(leaf).items():
        assert MC.voxel_index(v, leaf) == want, (name, v)
    v = MC.boundary_values(leaf)
    assert v["below 0"][0] < 0 and v["below leaf"][0] < leaf and np.signbit(v["-0.0"][0])
    case = MC.boundary_case(leaf, extra=(3, 7))
    r = MC.restate(case, [(0, 3)], leaf)
    ix = sorted(set(((r["keys"] & ((1 << 21) - 1)) - MC.HALF).tolist()))
    assert ix[:4] == [-2, -1, 0, 1] and 5 in ix and r["n_dropped"] == 0
    _same(r, MC.restate_dict(case, [(0, 3)], leaf))


def test_range_case_keeps_and_drops_what_it_names():
    leaf = 0.125
    case, kept, dropped = MC.range_case(leaf)
    ik = MC.voxel_index(kept, leaf)
    assert sorted(set(ik[ik != 0].tolist())) == [-MC.HALF, MC.HALF - 1]
    with np.errstate(invalid="ignore"):
        idr = MC.voxel_index(dropped, leaf)
    assert (idr == MC.HALF).sum() == 3 and (idr == -MC.HALF - 1).sum() == 3 and np.isnan(dropped).sum() == 3 and np.isinf(dropped).sum() == 6
    r = MC.restate(case, [(0, 2)], leaf)
    assert r["npts"].sum() == len(kept) == 6 and r["n_dropped"] == len(dropped) == 15
    counts = MC.restate(case, [(2, 2)], leaf)
    assert case["count"][2] < 0 and case["count"][3] > 16 and counts["npts"].sum() == 16        # the negative row: nothing; the other: cap


def test_order_and_digit_cases():
    leaf = 0.125
    r = MC.restate(MC.order_case(leaf), [(0, 2)], leaf)
    assert r["n_out"] == 20 and np.all(r["npts"] == 1) and np.all(np.diff(r["keys"]) > 0)
    i = np.stack([(r["keys"] >> s & ((1 << 21) - 1)) - MC.HALF for s in (0, 21, 42)], axis=1)
    for a in range(3):
        assert {-2, -1, 0, 1, 3} <= set(i[:, a].tolist())                                       # either side of the bias on every axis
    d = MC.restate(MC.digit_case(leaf), [(0, 2)], leaf)
    byte = lambda b: (d["keys"] >> (8 * b)) & 255  # noqa: E731
    assert d["n_dropped"] == 0 and all(len(set(byte(b).tolist())) >= 2 and np.bitwise_or.reduce(byte(b)) != 0 for b in range(8))


def test_canonical_sum_cases_depend_on_the_order():
    case, cloud, leaf16 = MC.three_row_case()
    r = MC.restate(case, cloud, leaf16)
    up, down = np.nextafter(np.float32(1), np.float32(2)), np.float32(1)
    assert r["n_out"] == 1 and r["npts"][0] == 8 and r["n_dropped"] == 0 and r["xyz"][0].tolist() == [up, down, up]
    _same(r, MC.restate_dict(case, cloud, leaf16))
    for perm in itertools.permutations((4, 1, 2)):
        other = MC.restate(case, [(k, 1) for k in perm], leaf16)
        assert (perm == (4, 1, 2)) == np.array_equal(other["xyz"], r["xyz"]), perm          # every other order of the rows shows in a float
    leaf = 0.125
    long = MC.long_run_case(leaf)
    import flvis_amd
    info = flvis_amd.voxel_cloud_info()
    r = MC.restate(long, [(0, 5)], leaf)
    assert r["n_out"] == 1 and r["npts"][0] == 5120 >= 5000 and 5120 > info["sort_tile"] >= info["workgroup"]
    P = long["p3"].reshape(-1, 3)
    seq = np.add.accumulate(P, axis=0)[-1]
    shuffled = np.add.accumulate(P[np.random.default_rng(0).permutation(len(P))], axis=0)[-1]
    tree = np.array([P[:, a].copy().sum() for a in range(3)])                                   # numpy's pairwise sum of a contiguous vector
    assert (seq != shuffled).any() and (seq != tree).any()                                      # order matters, and so does a tree


def test_ply_round_trip(tmp_path):
    from flvis_amd import traj_io
    rng = np.random.default_rng(3)
    xyz = (rng.normal(size=(200, 3)) * np.array([1e-3, 1.0, 1e4])).astype(np.float32)
    xyz[0] = [0.1, -0.0, np.float32(1) / np.float32(3)]
    npts = rng.integers(1, 9000, 200).astype(np.int32)
    traj_io.write_ply(str(tmp_path / "a.ply"), xyz, npts)
    a, n = traj_io.read_ply(str(tmp_path / "a.ply"))
    assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(n, npts)
    traj_io.write_ply(str(tmp_path / "b.ply"), xyz)
    b, n = traj_io.read_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(b.view(np.uint32), xyz.view(np.uint32)) and n is None
    traj_io.write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3), np.float32), np.zeros(0, np.int32))
    e, n = traj_io.read_ply(str(tmp_path / "e.ply"))
    assert e.shape == (0, 3) and len(n) == 0
    head = open(str(tmp_path / "a.ply")).read().split("end_header")[0].split("\n")
    assert head[:2] == ["ply", "format ascii 1.0"] and "element vertex 200" in head and "property int npts" in head
    (tmp_path / "bad.ply").write_text("plx\n")
    with pytest.raises(ValueError):
        traj_io.read_ply(str(tmp_path / "bad.ply"))
    with pytest.raises(ValueError):
        traj_io.write_ply(str(tmp_path / "c.ply"), xyz, npts[:5])


def test_argument_errors_without_a_device():
    """flvis_voxel_cloud_check is the host part of flvis_hip_voxel_cloud's checks; the entries themselves refuse a NULL context / closer"""
    import flvis_amd
    lib = flvis_amd.load_library()
    chk = lib.flvis_voxel_cloud_check
    ints = lambda *v: (C.c_int * len(v))(*v)  # noqa: E731
    ptr, rng = ints(0, 1, 3), ints(0, 4, 2, 2, 9, 1)
    good = dict(n_rows=10, cap=16, n_clouds=2, ptr=ptr, rng=rng, leaf=0.08, min_points=1, out_cap=5)
    call = lambda **kw: chk(*[dict(good, **kw)[k] for k in ("n_rows", "cap", "n_clouds", "ptr", "rng", "leaf", "min_points", "out_cap")])  # noqa: E731
    assert call() == 0 and call(leaf=0.0) == 0 and call(out_cap=0) == 0 and call(ptr=ints(0, 0, 3)) == 0 and call(rng=ints(0, 0, 2, 2, 10, 0)) == 0
    bad = [dict(leaf=-0.08), dict(leaf=float("nan")), dict(leaf=float("inf")), dict(min_points=0), dict(min_points=-1), dict(out_cap=-1),
           dict(n_clouds=0), dict(n_clouds=-2), dict(ptr=ints(1, 1, 3)), dict(ptr=ints(0, 2, 1)), dict(ptr=None), dict(rng=None),
           dict(rng=ints(0, 4, 2, 2, 9, 2)), dict(rng=ints(-1, 4, 2, 2, 9, 1)), dict(rng=ints(0, 4, 2, -1, 9, 1)), dict(rng=ints(0, 11, 2, 2, 9, 1)),
           dict(rng=ints(0, 4, 2, 2, 11, 0)), dict(n_rows=0), dict(cap=0)]
    for kw in bad:
        assert call(**kw) == flvis_amd.FLVIS_ERR_INVALID_ARG, kw
    info = flvis_amd.voxel_cloud_info()
    assert info["sort_tile"] % info["workgroup"] == 0 and info["workgroup"] % 64 == 0 and info["bytes_per_point"] == 48
    assert lib.flvis_hip_voxel_cloud_info(None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    vc = lib.flvis_hip_voxel_cloud
    n_out = (C.c_int64 * 2)()
    assert vc(None, None, None, None, 10, 16, 2, ptr, rng, 0.08, 1, 5, None, None, n_out, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    for name in ("flvis_loop_closer_map_cloud", "flvis_loop_closer_map_cloud_host"):
        fn = getattr(lib, name)
        assert fn(None, 1, ints(0, 1), ints(0), 0.08, 1, 5, None, None, n_out, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
