"""CPU: the two write-ups of the occupancy map queries (tests/_occupancy_cast.py) against each other on every edge case, proof that every
case reaches its edge, the queries against the occupancy map's own restatement, and the host part of flvis_hip_occupancy_cast's argument
checks (flvis_occupancy_cast_check, no device)."""
import ctypes as C

import numpy as np

import _occupancy as OC
import _occupancy_cast as Q

F32 = np.float32
LEAF = Q.LEAF


def _key(cell):
    return int(OC.key_of(list(cell)))


def test_an_empty_and_a_one_row_map():
    stop, go = [Q.both(j) for j in Q.empty_jobs()]
    n = [12, 8, 0, 10]
    assert (stop["status"] == Q.UNKNOWN).all() and (stop["k"] == 0).all() and (stop["row"] == -1).all() and (stop["t"] == 0).all()
    assert stop["cell"].tolist() == [_key((0, 0, 0)), _key((0, 0, 0)), _key((2, -1, 3)), _key((3, 1, 0))]
    assert (go["status"] == Q.END).all() and go["k"].tolist() == n and (go["row"] == -1).all() and (go["l"] == 0).all()
    assert go["cell"].tolist() == [_key((4, 4, 4)), _key((0, 0, 8)), _key((2, -1, 3)), _key((-2, 5, -1))]
    assert stop["cells_tested"] == 4 and go["cells_tested"] == sum(n) + 4
    occ, occ_stop, free = [Q.both(j) for j in Q.one_row_jobs()]
    assert occ["status"].tolist() == [Q.OCCUPIED, Q.OCCUPIED, Q.END, Q.END] and occ["k"].tolist() == [1, 0, 0, 0]
    assert occ["row"].tolist() == [0, 0, -1, -1] and occ["l"].tolist() == [1.0, 1.0, 0.0, 0.0] and occ["t"][0] == 0.0625 / 0.375
    assert occ_stop["status"].tolist() == [Q.UNKNOWN, Q.OCCUPIED, Q.UNKNOWN, Q.UNKNOWN] and occ_stop["k"].tolist() == [0, 0, 0, 0]
    assert free["status"].tolist() == [Q.END] * 4 and free["k"].tolist() == [3, 0, 0, 0] and free["row"].tolist() == [-1, 0, -1, -1]
    assert free["l"][1] == F32(-1.0)


def test_the_ends_of_the_table():
    (j,) = Q.table_end_jobs()
    r = Q.both(j)
    keys = j["keys"]
    q = OC.key_of(OC.cells(j["seg"][:, :3], LEAF)[1])
    assert q[0] == keys[0] and q[1] == keys[-1] and (q[2:4] < keys[0]).all() and (q[4:6] > keys[-1]).all()
    assert r["status"].tolist() == [Q.END, Q.OCCUPIED, Q.UNKNOWN, Q.UNKNOWN, Q.UNKNOWN, Q.UNKNOWN, Q.OCCUPIED]
    assert r["row"].tolist() == [0, 3, -1, -1, -1, -1, 1] and r["l"].tolist() == [-0.5, 2.0, 0, 0, 0, 0, 0.75]
    assert np.array_equal(r["cell"], q) and (r["k"] == 0).all()


def test_the_ends_of_the_index_range_and_coordinates_that_are_not_finite():
    (j,) = Q.range_jobs()
    r = Q.both(j)
    seg = j["seg"]
    assert np.floor(seg[0, 0] / LEAF) == -Q.HALF and np.floor(seg[1, 0] / LEAF) == Q.HALF - 1, "the two cells at the ends of the range"
    assert np.floor(seg[2, 0] / LEAF) == -Q.HALF - 1 and np.floor(seg[3, 0] / LEAF) == Q.HALF, "one ulp outside either end"
    assert seg[2, 0] == np.nextafter(seg[0, 0], -np.inf) and seg[1, 0] == np.nextafter(seg[3, 0], 0.0)
    assert r["status"][:2].tolist() == [Q.OCCUPIED] * 2 and r["row"][:2].tolist() == [0, 3]
    assert r["cell"][:2].tolist() == [_key((-Q.HALF, 0, 0)), _key((Q.HALF - 1, 0, 0))]
    assert (r["status"][2:8] == Q.DROPPED).all(), "an end outside the range, whichever end and axis"
    assert r["status"][8] == Q.OCCUPIED and r["k"][8] == 2 and r["row"][8] == 0, "a walk into the lowest cell"
    assert len(seg) == 9 + 18 and not np.isfinite(seg[9:]).all(axis=1).any() and (r["status"][9:] == Q.DROPPED).all()
    d = r["status"] == Q.DROPPED
    assert (r["k"][d] == 0).all() and (r["cell"][d] == -1).all() and (r["row"][d] == -1).all() and (r["l"][d] == 0).all() and (r["t"][d] == 0).all()
    assert r["counts"].tolist() == [0, 3, 0, 24, 0] and r["cells_tested"] == 1 + 1 + 3


def test_the_walk_edges_tie_face_axis_parallel_and_zero_step():
    jobs = {j["name"]: Q.both(j) for j in Q.walk_edge_jobs()}
    cells = [(1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1)]
    for k in (1, 2, 3, 4):
        r = jobs["diagonal tie, limit %d" % k]
        assert r["status"][0] == Q.LIMIT and r["k"][0] == k and r["cell"][0] == _key(cells[k - 1]), "three equal tmax: x, then y, then z"
        assert r["t"][0] == (0.125 if k < 4 else 0.375) and r["row"][0] == -1
    r = jobs["diagonal tie"]
    assert r["status"][0] == Q.END and r["k"][0] == 12 and r["cell"][0] == _key((4, 4, 4)) and r["t"][0] == 0.875
    r = jobs["origin on a face, limit 1"]
    assert r["status"][0] == Q.LIMIT and r["k"][0] == 1 and r["t"][0] == 0.0 and r["cell"][0] == _key((1, 0, 0)), "tmax.x == 0: t_1 == 0.0"
    r = jobs["origin on a face"]
    assert r["status"][0] == Q.END and r["cell"][0] == _key((-2, 0, 4)) and r["k"][0] == 8
    r = jobs["axis-parallel and zero-step"]
    assert r["status"].tolist() == [Q.END, Q.END] and r["k"].tolist() == [8, 0] and r["row"].tolist() == [8, 3] and r["t"][1] == 0.0


def test_values_at_the_threshold():
    at, neg, ray = [Q.both(j) for j in Q.value_jobs()]
    assert at["status"].tolist() == [Q.END, Q.OCCUPIED, Q.END, Q.END, Q.END, Q.END], "l == thres is FREE, one ulp above is OCCUPIED, NaN is FREE"
    assert at["l"][1] == np.nextafter(F32(0.5), F32(1)) and np.isnan(at["l"][2]) and at["row"].tolist() == [0, 1, 2, 3, 4, 5]
    assert neg["status"].tolist() == [Q.OCCUPIED, Q.OCCUPIED, Q.END, Q.END, Q.OCCUPIED, Q.END], "a negative thres: -0.25 is FREE, -0.2 OCCUPIED"
    assert ray["status"][0] == Q.END and ray["k"][0] == 1, "a NaN value does not stop a ray"


def test_max_cells_at_one_at_n_and_above_n():
    one, at_n, above = [Q.both(j) for j in Q.limit_jobs()]
    assert (one["status"][0], one["k"][0], one["row"][0], one["cell"][0]) == (Q.LIMIT, 1, -1, _key((1, 0, 0))) and one["cells_tested"] == 1
    assert (at_n["status"][0], at_n["k"][0], at_n["row"][0], at_n["l"][0]) == (Q.LIMIT, 5, -1, 0.0), "the last cell is in the map and not looked up"
    assert at_n["cell"][0] == _key((5, 0, 0)) and at_n["cells_tested"] == 5
    assert (above["status"][0], above["k"][0], above["row"][0], above["l"][0]) == (Q.END, 5, 5, -1.0) and above["cells_tested"] == 6


def test_unknown_cells_on_the_ray():
    stop, go = [Q.both(j) for j in Q.unknown_jobs()]
    assert (stop["status"][0], stop["k"][0], stop["row"][0]) == (Q.UNKNOWN, 1, -1), "UNKNOWN wins in front of an occupied cell"
    assert (go["status"][0], go["k"][0], go["row"][0], go["l"][0]) == (Q.OCCUPIED, 2, 1, 1.0)
    for r in (stop, go):
        assert (r["status"][1], r["k"][1], r["row"][1], r["t"][1]) == (Q.OCCUPIED, 0, 1, 0.0), "an occupied cell at k = 0"


def test_rows_beyond_n_rows_would_match():
    for j in Q.slack_jobs():
        r = Q.both(j)
        seen = Q.cast(np.concatenate([j["keys"], j["slack"][0]]), np.concatenate([j["l"], j["slack"][1]]), j["seg"], j["leaf"], **j["prm"])
        assert (seen["status"] == Q.OCCUPIED).all() and (r["status"] != Q.OCCUPIED).all() and (r["row"][1:] == -1).all()
        assert np.isin(j["slack"][0], OC.key_of(OC.cells(j["seg"][:, 3:], LEAF)[1])).all(), "the slack holds keys the queries ask for"


def test_the_directory_shapes():
    jobs = {j["name"]: (j, Q.both(j)) for j in Q.directory_jobs()}
    for axis, name in enumerate("xyz"):
        j, r = jobs["300 cells along " + name]
        lines = np.unique(j["keys"] >> 21)
        assert len(j["keys"]) == 300 and len(lines) == (1 if axis == 0 else 300), "one full line, or 300 lines of a single row"
        assert r["status"].tolist() == [Q.OCCUPIED, Q.OCCUPIED] and r["k"].tolist() == [299, 0] and r["row"].tolist() == [299, 299]
        j, r = jobs["300 cells along %s, all free" % name]
        assert r["status"].tolist() == [Q.END, Q.END] and r["k"].tolist() == [299, 299] and r["row"].tolist() == [299, 0]
        assert r["cells_tested"] == 600
    j, r = jobs["slab of 3000 lines"]
    assert len(np.unique(j["keys"] >> 21)) == 3000 > 1024 and (np.diff(j["keys"]) > 0).all()
    assert all((r["status"] == s).sum() >= 5 for s in (Q.END, Q.OCCUPIED, Q.UNKNOWN)) and r["k"].max() > 20
    j, r = jobs["slab of 3000 lines, unknown ignored"]
    assert (r["status"] != Q.UNKNOWN).all() and ((r["status"] == Q.END) & (r["row"] == -1)).any()
    j, r = jobs["slab of 3000 lines, nothing occupied"]
    assert set(r["status"].tolist()) == {Q.END, Q.LIMIT} and (r["k"][r["status"] == Q.LIMIT] == 40).all()


def test_the_rays_of_a_scan_through_the_maps_that_hold_it():
    case, o, p, steps = Q.builder_case(LEAF)
    assert len(o) == 54
    seg = np.concatenate([o, p], axis=1)
    alone, whole = OC.restate(dict(case, clouds=[[(0, 1)]]), 0, LEAF), OC.restate(case, 0, LEAF)
    for name, mp in (("the scan alone", alone), ("all three scans", whole)):
        r = Q.both(Q.job(name, (mp["keys"], mp["l"]), seg))
        assert (r["status"] == Q.OCCUPIED).all() and (r["k"] <= steps).all() and (r["k"] < steps).sum() == 1, name
        free = Q.both(Q.job(name + ", nothing occupied", (mp["keys"], mp["l"]), seg, thres=100.0))
        assert (free["status"] == Q.END).all() and np.array_equal(free["k"], steps), "no ray of a scan meets an UNKNOWN cell in a map that holds it"
    keep = alone["l"] <= 0
    far = np.concatenate([o, o + 1.5 * (p - o)], axis=1)
    r = Q.both(Q.job("stretched rays, occupied rows removed", (alone["keys"][keep], alone["l"][keep]), far))
    assert keep.sum() < len(keep) and (r["status"] == Q.UNKNOWN).all()


def test_every_other_job_agrees_too():
    for j in Q.all_jobs():
        Q.both(j)


def test_argument_errors_without_a_device():
    """flvis_occupancy_cast_check is the host part of flvis_hip_occupancy_cast's checks; the entries themselves refuse a NULL context"""
    import flvis_amd
    lib = flvis_amd.load_library()
    ints = lambda *v: (C.c_int * len(v))(*v)  # noqa: E731
    i64 = lambda *v: (C.c_int64 * len(v))(*v)  # noqa: E731
    P = flvis_amd.OccupancyCastParams
    good = dict(n_maps=3, map_cap=9, n_rows=i64(0, 9, 4), leaf=0.08, prm=P(0.0, 0, 0), q_ptr=ints(0, 5, 5, 7))
    order = ("n_maps", "map_cap", "n_rows", "leaf", "prm", "q_ptr")

    def call(**kw):
        a = dict(good, **kw)
        a["prm"] = C.byref(a["prm"]) if a["prm"] is not None else None
        return lib.flvis_occupancy_cast_check(*[a[k] for k in order])

    d = flvis_amd.occupancy_cast_params()
    assert (d.thres, d.ignore_unknown, d.max_cells) == (0.0, 0, 0)
    d = flvis_amd.occupancy_cast_params(thres=-0.5, ignore_unknown=True, max_cells=7)
    assert (d.thres, d.ignore_unknown, d.max_cells) == (-0.5, 1, 7)
    assert call() == flvis_amd.FLVIS_OK and call(prm=P(-1.5, 1, 12)) == flvis_amd.FLVIS_OK
    assert call(n_maps=1, n_rows=i64(0), q_ptr=ints(0, 0), map_cap=0) == flvis_amd.FLVIS_OK
    nan, inf = float("nan"), float("inf")
    bad = [dict(leaf=0.0), dict(leaf=-0.08), dict(leaf=nan), dict(leaf=inf), dict(prm=None), dict(prm=P(nan, 0, 0)), dict(prm=P(inf, 0, 0)),
           dict(prm=P(-inf, 0, 0)), dict(prm=P(0.0, 0, -1)), dict(prm=P(0.0, 2, 0)), dict(prm=P(0.0, -1, 0)), dict(n_rows=i64(0, 10, 4)),
           dict(n_rows=i64(-1, 9, 4)), dict(n_rows=None), dict(map_cap=-1), dict(map_cap=8), dict(q_ptr=ints(1, 5, 5, 7)), dict(q_ptr=ints(0, 5, 4, 7)),
           dict(q_ptr=ints(0, 5, 5, -7)), dict(q_ptr=None), dict(n_maps=0), dict(n_maps=-1)]
    for kw in bad:
        assert call(**kw) == flvis_amd.FLVIS_ERR_INVALID_ARG, kw
    assert lib.flvis_hip_occupancy_cast(None, 1, None, None, 0, i64(0), 0.08, C.byref(good["prm"]), None, ints(0, 0), None, None, None, None, None,
                                        None, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_hip_occupancy_cast_host(None, 1, None, None, 0, i64(0), 0.08, C.byref(good["prm"]), None, ints(0, 0), None, None, None, None,
                                             None, None, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_hip_occupancy_cast_stats(None, None, None) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert flvis_amd.OCCUPANCY_CAST_STATUS == ("end", "occupied", "unknown", "dropped", "limit")
