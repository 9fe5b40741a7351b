"""GPU tests of the voxel cloud (flvis_hip_voxel_cloud, flvis_loop_closer_map_cloud) against the numpy restatement of tests/_map_cloud.py.
Every comparison is bit for bit: the order of the rows (ascending by key), the float rows, the counts, n_out and n_dropped.
tests/test_map_cloud_inputs.py shows on the CPU that each edge input used here hits the edge it is named for."""
import numpy as np
import pytest

import _map_cloud as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _up(case):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(case["p3"])).cuda(), torch.from_numpy(np.ascontiguousarray(case["count"], np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(case["T"])).cuda())


def _run(ctx, case, clouds, leaf, min_points=1, cap=None, want_npts=True, dev=None):
    return ctx.voxel_cloud(*(dev or _up(case)), clouds, leaf=leaf, min_points=min_points, cap=cap, want_npts=want_npts)


def _check(ctx, case, clouds, leaf, min_points=1, cap=None, dev=None):
    """one call for all `clouds` against one restatement per cloud; -> the restatements"""
    xyz, npts, n_out, n_drop = _run(ctx, case, clouds, leaf, min_points, cap, dev=dev)
    want = [MC.restate(case, c, leaf, min_points) for c in clouds]
    for k, w in enumerate(want):
        rows = w["n_out"] if cap is None else min(cap, w["n_out"])
        assert n_out[k] == w["n_out"] and n_drop[k] == w["n_dropped"], (k, n_out[k], w["n_out"], n_drop[k], w["n_dropped"])
        assert xyz[k].shape == (rows, 3) and np.array_equal(xyz[k].view(np.uint32), w["xyz"][:rows].view(np.uint32)), k
        assert np.array_equal(npts[k], w["npts"][:rows]), k
    return want


@pytest.mark.parametrize("leaf", [0.125, 0.08])
def test_boundaries(ctx, leaf):
    case = MC.boundary_case(leaf, extra=() if leaf == 0.125 else (3, 7))
    w = _check(ctx, case, [[(0, 3)]], leaf)[0]
    assert w["n_dropped"] == 0 and np.all(np.diff(w["keys"]) > 0)
    _check(ctx, case, [[(0, 3)]], 0.0)


def test_range_and_refusals(ctx):
    case, kept, dropped = MC.range_case(0.125)
    w = _check(ctx, case, [[(0, 2)], [(2, 2)], [(2, 1)], [(0, 4)]], 0.125)
    assert w[0]["n_dropped"] == len(dropped) and w[0]["npts"].sum() == len(kept)
    assert w[1]["npts"].sum() == 16 and w[2]["n_out"] == 0                          # a count above cap reads cap, a negative one nothing
    raw = _check(ctx, case, [[(0, 2)]], 0.0)[0]
    assert raw["n_dropped"] == 9 and raw["n_out"] == len(kept) + 6                  # leaf 0: only what is not finite goes


def test_order_and_packing(ctx):
    w = _check(ctx, MC.order_case(0.125), [[(0, 2)]], 0.125)[0]
    assert w["n_out"] == 20 and np.all(np.diff(w["keys"]) > 0)
    d = _check(ctx, MC.digit_case(0.125), [[(0, 2)]], 0.125)[0]
    st = ctx.voxel_cloud_stats()
    assert st["passes_run"] == 8 and st["input_points"] == 96 and d["n_out"] >= 90  # every digit of the key took two values or more
    _check(ctx, MC.digit_case(0.125), [[(1, 1)], [(0, 1)], [(0, 2)]], 0.125)        # and with the cloud digit behind them
    assert ctx.voxel_cloud_stats()["passes_run"] == 9


def test_canonical_sums(ctx):
    case, cloud, leaf = MC.three_row_case()
    w = _check(ctx, case, [cloud], leaf)[0]
    assert w["n_out"] == 1 and w["npts"][0] == 8
    for perm in ((4, 2, 1), (1, 4, 2), (1, 2, 4), (2, 4, 1), (2, 1, 4)):             # the order is the caller's, whatever it is
        o = _check(ctx, case, [[(k, 1) for k in perm]], leaf)[0]
        assert not np.array_equal(o["xyz"], w["xyz"])
    long = MC.long_run_case(0.125)
    w = _check(ctx, long, [[(0, 5)]], 0.125)[0]
    assert w["n_out"] == 1 and w["npts"][0] == 5120
    w = _check(ctx, long, [[(3, 2), (0, 3)], [(0, 5)]], 0.125)                        # the same points in another order: another sum
    assert w[0]["npts"][0] == 5120


def test_sizes(ctx):
    import flvis_amd
    tile = flvis_amd.voxel_cloud_info()["sort_tile"]
    for total in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1):
        case = MC.sized_case(total)
        n = len(case["count"])
        w = _check(ctx, case, [[(0, n)]], 0.08)[0]
        assert w["npts"].sum() == total
        raw = _check(ctx, case, [[(0, n)]], 0.0)[0]
        assert raw["n_out"] == total
    case = MC.sized_case(3 * tile + 77)                                              # several tiles and workgroups, empty rows between full ones
    assert (case["count"] == 1024).sum() >= 12 and (case["count"] == 0).sum() >= 12
    _check(ctx, case, [[(0, len(case["count"]))]], 0.08)


def test_output_limits(ctx):
    case = MC.random_case(31, [200, 150, 0, 256], cap=256, reach=0.6)
    dev = _up(case)
    cloud = [[(0, 4)]]
    full = _check(ctx, case, cloud, 0.08, dev=dev)[0]
    assert full["n_out"] > 100 and full["npts"].max() >= 3
    for cap in (full["n_out"] - 1, 17, 1, 0):
        _check(ctx, case, cloud, 0.08, cap=cap, dev=dev)
    xyz, npts, n_out, _ = _run(ctx, case, cloud, 0.08, want_npts=False, dev=dev)      # d_npts = NULL
    assert npts is None and n_out[0] == full["n_out"] and np.array_equal(xyz[0].view(np.uint32), full["xyz"].view(np.uint32))
    for mp in (1, 2, int(full["npts"].max()), int(full["npts"].max()) + 1):
        w = _check(ctx, case, cloud, 0.08, min_points=mp, dev=dev)[0]
        assert (w["n_out"] == 0) == (mp > full["npts"].max())
    raw = _check(ctx, case, cloud, 0.0, min_points=5, dev=dev)[0]                      # leaf 0: the canonical list, min_points not used
    assert raw["n_out"] == 606
    _check(ctx, case, cloud, 0.0, cap=100, dev=dev)


def test_transform(ctx):
    rng = np.random.default_rng(41)
    counts = rng.integers(0, 33, 200)
    case = MC.random_case(42, counts, cap=32, poses=True)
    assert np.abs(np.linalg.norm(case["T"][:, 3:], axis=1) - 1).max() < 1e-15
    w = _check(ctx, case, [[(0, 200)]], 0.08)[0]
    assert w["npts"].sum() == counts.sum()
    _check(ctx, case, [[(0, 200)]], 0.0)
    ident = dict(case, T=np.tile(MC.IDENT, (200, 1)))                                 # the control: the same rows under identity poses
    raw = _check(ctx, ident, [[(0, 200)]], 0.0)[0]
    rows, lms = MC.canonical(ident, [(0, 200)])
    assert np.array_equal(raw["xyz"], ident["p3"][rows, lms].astype(np.float32))
    _check(ctx, ident, [[(0, 200)]], 0.08)


def test_batch(ctx):
    """5 clouds of different sizes in one call, one empty, one sharing rows with another = the 5 single calls; and a second run"""
    case = MC.random_case(51, [300, 0, 512, 77, 512, 1, 400, 512], cap=512, poses=True, reach=0.8)
    dev = _up(case)
    clouds = [[(0, 3)], [(1, 1)], [(2, 4)], [(7, 1), (0, 1)], [(4, 4), (3, 1)]]
    for leaf in (0.08, 0.0):
        a = _run(ctx, case, clouds, leaf, dev=dev)
        b = _run(ctx, case, clouds, leaf, dev=dev)
        for k, c in enumerate(clouds):
            one = _run(ctx, case, [c], leaf, dev=dev)
            assert a[2][k] == one[2][0] == b[2][k] and a[3][k] == one[3][0] == b[3][k]
            for j in (0, 1):
                assert np.array_equal(a[j][k].view(np.uint32), one[j][0].view(np.uint32))
                assert np.array_equal(a[j][k].view(np.uint32), b[j][k].view(np.uint32))
        assert a[2][1] == 0 and len(a[0][1]) == 0
        _check(ctx, case, clouds, leaf, dev=dev)


def test_argument_errors_leave_the_context_usable(ctx):
    import flvis_amd
    case = MC.random_case(61, [10, 10], cap=16)
    dev = _up(case)
    for kw in (dict(leaf=-1.0), dict(leaf=float("nan")), dict(leaf=float("inf")), dict(min_points=0), dict(cap=-1)):
        with pytest.raises(flvis_amd.FlvisError) as e:
            ctx.voxel_cloud(*dev, [[(0, 2)]], **kw)
        assert "voxel_cloud failed (-1)" in str(e.value)
    for clouds in ([[(0, 3)]], [[(-1, 1)]], [[(2, 1)]], []):
        with pytest.raises(flvis_amd.FlvisError):
            ctx.voxel_cloud(*dev, clouds)
    _check(ctx, case, [[(0, 2)], [(2, 0)]], 0.08, dev=dev)


# ---- the closer ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    import test_gpu_loop_localize as TL
    w = TL.World()
    yield w
    w.ctx.close()


def _closer_check(lc, groups, leaf, host=False, min_points=1):
    seqs = sorted({s for g in groups for s in g})
    case, where = MC.closer_case(lc, seqs)
    got = lc.map_cloud(groups, leaf=leaf, min_points=min_points, host=host)
    for k, g in enumerate(groups):
        w = MC.restate(case, [where[s] for s in g], leaf, min_points)
        assert got[2][k] == w["n_out"] and got[3][k] == w["n_dropped"], (k, got[2][k], w["n_out"])
        assert np.array_equal(got[0][k].view(np.uint32), w["xyz"].view(np.uint32)) and np.array_equal(got[1][k], w["npts"]), k
    return got


def test_closer_map_cloud(world):
    import flvis_amd
    import test_gpu_loop_localize as TL
    import _loop_localize as LL
    import _pgo_synth as PS
    w = world
    sc = w.sc
    sel = TL._sel
    lc = w.closer(5, 8)
    # sequences 0, 1, 3 loaded (1 holds a blank keyframe); 2 and 4 stay empty; sequence 3's last keyframe is added and not processed
    for i in range(3):
        lc.add_keyframes([0, 3], sel(w.kf0, [i, i + 1]), sel(w.kf1, [i, i + 1]), [sc.kf_gt[i], sc.kf_gt[i + 1]])
        img0, img1 = (w.blank, w.blank) if i == 1 else (w.kf0[i + 2:i + 3], w.kf1[i + 2:i + 3])
        lc.add_keyframes([1], img0, img1, [sc.kf_gt[i + 2]])
        lc.process()
    lc.add_keyframes([3], w.kf0[4:5], w.kf1[4:5], [sc.kf_gt[4]])
    groups = [[3, 0], [1]]
    before = TL._state(lc, 5)
    first = _closer_check(lc, groups, 0.08)
    assert first[2][0] > 100 and first[2][1] > 50 and len(lc.poses(3)) == 4
    _closer_check(lc, groups, 0.0)
    _closer_check(lc, [[2, 4], [0], [4, 3, 2]], 0.08)                                    # empty sequences; a sequence in two groups
    host = _closer_check(lc, groups, 0.08, host=True)
    for k in range(2):
        assert np.array_equal(host[0][k].view(np.uint32), first[0][k].view(np.uint32)) and np.array_equal(host[1][k], first[1][k])
    cut = lc.map_cloud(groups, leaf=0.08, cap=40)
    cut_h = lc.map_cloud(groups, leaf=0.08, cap=40, host=True)
    for k in range(2):
        assert cut[2][k] == first[2][k] and np.array_equal(cut[0][k], first[0][k][:40]) and np.array_equal(cut_h[0][k], first[0][k][:40])
        assert np.array_equal(cut[1][k], first[1][k][:40]) and np.array_equal(cut_h[1][k], first[1][k][:40])
    TL._same_state(before, TL._state(lc, 5))
    ev = lc.process()                                                                   # the pending keyframe is still pending
    assert ev[3]["kf_curr"] == 3 and all(ev[s]["kf_curr"] == -1 for s in (0, 1, 2, 4))
    # the argument errors change nothing
    state = TL._state(lc, 5)
    for bad, kw in (([[0, 0]], {}), ([[5]], {}), ([[-1]], {}), ([], {}), (groups, dict(leaf=-0.1)), (groups, dict(leaf=float("nan"))),
                    (groups, dict(min_points=0)), (groups, dict(cap=-1))):
        for host in (False, True):
            with pytest.raises(flvis_amd.FlvisError) as e:
                lc.map_cloud(bad, host=host, **kw)
            assert "(-1)" in str(e.value)
    TL._same_state(state, TL._state(lc, 5))
    # a new drift and further keyframes
    lc.set_drift(0, np.array([0.3, -0.2, 0.1, 0.02, -0.05, 0.1, 2.0]))
    lc.add_keyframes([0, 1], sel(w.kf0, [3, 0]), sel(w.kf1, [3, 0]), [sc.kf_gt[3], sc.kf_gt[0]])
    lc.process()
    drifted = _closer_check(lc, groups, 0.08)
    assert drifted[2][0] > first[2][0]
    # a merge of the first group: two links from sequence 3 to sequence 0, as tests/_loop_merge.py's "pair-12" has them
    P3, P0 = lc.poses(3), lc.poses(0)
    rng = np.random.default_rng(9)

    def link(kf_from, kf_to):
        rel = PS.mul7(P0[kf_to], PS.inv7(P3[kf_from]))
        rel[:3] += rng.normal(0, 0.05, 3)
        return dict(seq_from=3, kf_from=kf_from, seq_to=0, kf_to=kf_to, pose=rel)
    out, _ = lc.merge([[3, 0]], [link(0, 1), link(2, 3)])
    assert out[0]["optimised"]
    assert not np.array_equal(lc.poses(0), P0)
    merged = _closer_check(lc, groups, 0.08)
    assert not (merged[2][0] == drifted[2][0] and np.array_equal(merged[0][0], drifted[0][0]))
    assert merged[2][1] == drifted[2][1] and np.array_equal(merged[0][1], drifted[0][1])     # sequence 1 was in no merge
    _closer_check(lc, groups, 0.08, host=True)
    # a reset sequence gives no rows
    lc.reset([1])
    after = _closer_check(lc, groups, 0.08)
    assert after[2][1] == 0 and len(after[0][1]) == 0 and np.array_equal(after[0][0], merged[0][0])
    lc.close()
