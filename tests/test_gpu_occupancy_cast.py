"""GPU: flvis_hip_occupancy_cast (include/flvis_hip.h) against its restatement (tests/_occupancy_cast.py), bit for bit in all six outputs
and the counts: every edge case of test_occupancy_cast_inputs.py, several maps in one call against single calls, NULL outputs, the _host
form, keys out of order, the point lookup, a map made by Context.occupancy fed straight back in, the statistics and a second run."""
import ctypes as C

import numpy as np
import pytest

import _occupancy as OC
import _occupancy_cast as Q

pytestmark = pytest.mark.gpu

INV = -1
LEAF = Q.LEAF


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _result(got, m=0):
    out = {f: got[i][m] for i, f in enumerate(Q.FIELDS)}
    out["counts"] = got[6][m]
    return out


def _same(got, m, want, what):
    r = _result(got, m)
    for f in Q.FIELDS:
        assert r[f].dtype == want[f].dtype and r[f].tobytes() == want[f].tobytes(), (what, f, r[f], want[f])
    assert np.array_equal(r["counts"], want["counts"]), (what, "counts", r["counts"], want["counts"])


def _run(ctx, job, **kw):
    return ctx.occupancy_cast([(job["keys"], job["l"])], [job["seg"]], job["leaf"], **dict(job["prm"], **kw))


def _want(job):
    return Q.cast(job["keys"], job["l"], job["seg"], job["leaf"], **job["prm"])


@pytest.fixture(scope="module")
def wanted():
    """the restatement of every job, made once"""
    return {job["name"]: _want(job) for job in Q.all_jobs()}


@pytest.mark.parametrize("plain", [False, True], ids=["line directory", "plain search"])
def test_every_edge_case(ctx, wanted, plain):
    ctx.occupancy_cast_lookup(plain=plain)
    try:
        for job in Q.all_jobs():
            if "slack" in job:
                continue
            want = wanted[job["name"]]
            _same(_run(ctx, job), 0, want, job["name"])
            st = ctx.occupancy_cast_stats()
            assert st["queries"] == len(job["seg"]) and st["cells"] == want["cells_tested"], (job["name"], st)
            assert (st["index_bytes"] == 0) == plain
    finally:
        ctx.occupancy_cast_lookup()


def test_the_two_lookups_against_each_other_on_the_directory_shapes(ctx):
    """longer segments than the restatement is asked to walk: 4096 of them through the slab and far out of it, both ways"""
    keys, l = Q.slab_map()
    rng = np.random.default_rng(11)
    nx, ny, nz = Q.SLAB
    a = rng.uniform([-3, -5, -5], [nx + 3, ny + 5, nz + 5], (4096, 3)) * LEAF
    b = rng.uniform([-3, -5, -5], [nx + 3, ny + 5, nz + 5], (4096, 3)) * LEAF
    seg = np.concatenate([a, b], axis=1)
    lines = [Q.make_map(Q.line_rows(300, axis)) for axis in range(3)]
    runs = np.array([Q.seg_cells((0, 0, 0), (299, 0, 0)), Q.seg_cells((0, 299, 0), (0, 0, 0)), Q.seg_cells((-3, -3, -3), (5, 290, 3))])
    for kw in (dict(), dict(ignore_unknown=True), dict(ignore_unknown=True, thres=2.0), dict(ignore_unknown=True, max_cells=25)):
        got = {}
        for plain in (False, True):
            ctx.occupancy_cast_lookup(plain=plain)
            got[plain] = ctx.occupancy_cast([(keys, l)] + lines, [seg, runs, runs, runs], LEAF, **kw)
        ctx.occupancy_cast_lookup()
        for i in range(6):
            for m in range(4):
                assert got[False][i][m].tobytes() == got[True][i][m].tobytes(), (kw, Q.FIELDS[i], m)
        assert np.array_equal(got[False][6], got[True][6])
        if kw.get("ignore_unknown") and not kw.get("max_cells"):
            assert got[False][1][0].max() > 60, "walks of many cells"


def test_rows_beyond_n_rows_are_not_seen(ctx):
    import torch
    for job in Q.slack_jobs():
        key = torch.from_numpy(np.concatenate([job["keys"], job["slack"][0]])[None].copy()).cuda()
        l = torch.from_numpy(np.concatenate([job["l"], job["slack"][1]])[None].copy()).cuda()
        got = ctx.occupancy_cast((key, l), [job["seg"]], job["leaf"], rows=[len(job["keys"])], **job["prm"])
        _same(got, 0, _want(job), job["name"])
        seen = ctx.occupancy_cast((key, l), [job["seg"]], job["leaf"], rows=[int(key.shape[1])], **job["prm"])
        assert (seen[0][0] == Q.OCCUPIED).all(), "with the rows counted in, the same arrays answer otherwise"


def _slab_jobs():
    jobs = {j["name"]: j for j in Q.directory_jobs() + Q.table_end_jobs()}
    return [jobs["slab of 3000 lines"], jobs["300 cells along y"], jobs["table ends"]]


def test_three_maps_of_different_sizes_and_one_without_queries_against_single_calls(ctx):
    a, b, c = _slab_jobs()
    maps = [(a["keys"], a["l"]), (b["keys"], b["l"]), (c["keys"], c["l"]), (b["keys"], b["l"])]
    segs = [a["seg"], b["seg"], np.zeros((0, 6)), c["seg"]]
    got = ctx.occupancy_cast(maps, segs, LEAF)
    st = ctx.occupancy_cast_stats()
    cells = 0
    for m, (mp, sg) in enumerate(zip(maps, segs)):
        want = Q.cast(mp[0], mp[1], sg, LEAF)
        _same(got, m, want, ("batch", m))
        cells += want["cells_tested"]
        if len(sg):
            one = ctx.occupancy_cast([mp], [sg], LEAF)
            assert all(one[i][0].tobytes() == got[i][m].tobytes() for i in range(6)) and np.array_equal(one[6][0], got[6][m]), m
    assert got[6][2].tolist() == [0] * 5 and len(got[0][2]) == 0
    assert st["queries"] == sum(len(s) for s in segs) and st["cells"] == cells and st["index_bytes"] > 0 and st["workspace_bytes"] > 0
    again = ctx.occupancy_cast(maps, segs, LEAF)
    assert all(x.tobytes() == y.tobytes() for i in range(6) for x, y in zip(again[i], got[i])) and np.array_equal(again[6], got[6])


def test_null_outputs_and_the_host_form(ctx):
    a = _slab_jobs()[0]
    want = _want(a)
    only = _run(ctx, a, outputs=False)
    assert only[0][0].tobytes() == want["status"].tobytes() and all(only[i] is None for i in range(1, 6))
    assert np.array_equal(only[6][0], want["counts"])
    _same(_run(ctx, a, host=True), 0, want, "host")
    only = _run(ctx, a, host=True, outputs=False)
    assert only[0][0].tobytes() == want["status"].tobytes() and only[1] is None and np.array_equal(only[6][0], want["counts"])
    _same(ctx.occupancy_cast([(a["keys"], a["l"])], [np.zeros((0, 6))], LEAF, host=True), 0, Q.cast(a["keys"], a["l"], np.zeros((0, 6)), LEAF), "host, no query")


def test_keys_out_of_order_are_refused_and_nothing_is_written(ctx):
    import flvis_amd
    import torch
    (job,) = Q.table_end_jobs()
    lib, nq = ctx._lib, len(job["seg"])
    seg = torch.from_numpy(job["seg"]).cuda()
    l = torch.from_numpy(job["l"][None].copy()).cuda()
    prm = flvis_amd.occupancy_cast_params()
    keys = job["keys"]
    for bad in (keys[::-1].copy(), np.array([keys[0], keys[1], keys[1], keys[3]], np.int64), np.array([-5, keys[1], keys[2], keys[3]], np.int64)):
        key = torch.from_numpy(bad[None].copy()).cuda()
        status = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        row = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        counts = np.full(5, 77, np.int64)
        rc = lib.flvis_hip_occupancy_cast(ctx._h, 1, key.data_ptr(), l.data_ptr(), 4, (C.c_int64 * 1)(4), LEAF, C.byref(prm), seg.data_ptr(),
                                          (C.c_int * 2)(0, nq), status.data_ptr(), None, None, row.data_ptr(), None, None,
                                          counts.ctypes.data_as(C.c_void_p))
        assert rc == INV and (status.cpu().numpy() == 77).all() and (row.cpu().numpy() == 77).all()
        with pytest.raises(flvis_amd.FlvisError, match=r"failed \(%d\)" % INV):
            ctx.occupancy_cast([(bad, job["l"])], [job["seg"]], LEAF)
    # an output that overlaps the segments or a map, and a NULL the rule needs
    key = torch.from_numpy(keys[None].copy()).cuda()
    args = lambda **kw: [kw.get(k, v) for k, v in (("status", seg.data_ptr()), ("k", None), ("cell", None), ("row", None), ("l", None), ("t", None))]  # noqa: E731
    head = (ctx._h, 1, key.data_ptr(), l.data_ptr(), 4, (C.c_int64 * 1)(4), LEAF, C.byref(prm), seg.data_ptr(), (C.c_int * 2)(0, nq))
    assert lib.flvis_hip_occupancy_cast(*head, *args(), None) == INV
    status = torch.zeros(nq, dtype=torch.int32, device="cuda")
    assert lib.flvis_hip_occupancy_cast(*head, *args(status=status.data_ptr(), cell=key.data_ptr()), None) == INV
    assert lib.flvis_hip_occupancy_cast(*head, *args(status=None), None) == INV
    assert lib.flvis_hip_occupancy_cast(*head, *args(status=status.data_ptr()), None) == flvis_amd.FLVIS_OK
    _same(_run(ctx, job), 0, _want(job), "after the refusals")


def test_the_point_lookup(ctx):
    (job,) = Q.table_end_jobs()
    pts = job["seg"][:, :3]
    status, row, l, counts = ctx.occupancy_lookup([(job["keys"], job["l"])], [pts], LEAF)
    want = _want(job)
    assert status[0].tobytes() == want["status"].tobytes() and row[0].tobytes() == want["row"].tobytes() and l[0].tobytes() == want["l"].tobytes()
    assert np.array_equal(counts[0], want["counts"])
    status, row, l, _ = ctx.occupancy_lookup([(job["keys"], job["l"])], [pts], LEAF, thres=1.0)
    assert status[0].tolist() == [Q.END, Q.OCCUPIED, Q.UNKNOWN, Q.UNKNOWN, Q.UNKNOWN, Q.UNKNOWN, Q.END]


def test_a_map_made_on_the_device_fed_straight_back_in(ctx):
    import torch
    case, o, p, steps = Q.builder_case(LEAF)
    d = torch.from_numpy(case["depth"].view(np.int16).copy()).cuda()
    T = torch.from_numpy(np.ascontiguousarray(case["T"], np.float64)).cuda()
    prm = case["prm"]
    keys, l = ctx.occupancy(d, T, case["clouds"], case["cams"], window=(prm["u0"], prm["v0"], prm["u1"], prm["v1"]),
                            step=(prm["step_u"], prm["step_v"]), z_min=prm["z_min"], z_max=prm["z_max"], leaf=LEAF)[:2]
    whole = OC.restate(case, 0, LEAF)
    assert np.array_equal(keys[0], whole["keys"]) and l[0].tobytes() == whole["l"].tobytes()
    seg = np.concatenate([o, p], axis=1)
    got = ctx.occupancy_cast([(keys[0], l[0])], [seg], LEAF)
    _same(got, 0, Q.cast(whole["keys"], whole["l"], seg, LEAF), "the scan's rays through the device's map")
    assert (got[0][0] == Q.OCCUPIED).all() and (got[1][0] <= steps).all() and (got[1][0] < steps).sum() == 1
    free = ctx.occupancy_cast([(keys[0], l[0])], [seg], LEAF, thres=100.0)
    assert (free[0][0] == Q.END).all() and np.array_equal(free[1][0], steps)
    st = ctx.occupancy_cast_stats()
    assert st["cells"] == int(steps.sum()) + len(steps)
