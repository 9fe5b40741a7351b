"""Test helper: the local map's sparse map cloud (flvis_local_map_cloud, include/flvis_hip.h) restated in numpy.

A stream's history is a list of runs (frame_id, lm_id int64 [k], lm_3d float64 [k, 3]): what flvis_get_correction returns after each
optimisation, in order.  `record` is the device record after those runs at a capacity; `select` the entries a mode keeps, in record
order; `raw` and `voxel` the two outputs (voxel: through tests/_map_cloud.py's restatement of flvis_hip_voxel_cloud, one row of points
under an identity pose)."""
import numpy as np

import _map_cloud as MC

ALL, LATEST = 0, 1


def record(runs, capacity):
    """-> dict(ids int64 [n], pts float64 [n, 3], run int64 [n] the run each entry came from, runs recorded, dropped).  A run whose
    points do not fit whole is dropped, and every run after the first dropped one."""
    ids, pts, src = [np.zeros(0, np.int64)], [np.zeros((0, 3))], [np.zeros(0, np.int64)]
    n, recorded, dropped = 0, 0, 0
    for k, (_, lm_id, lm_3d) in enumerate(runs):
        lm_id, lm_3d = np.asarray(lm_id, np.int64), np.asarray(lm_3d, np.float64).reshape(-1, 3)
        assert len(lm_id) == len(lm_3d) and len(np.unique(lm_id)) == len(lm_id), "an id occurs at most once per run"
        if dropped or n + len(lm_id) > capacity:
            dropped += 1
            continue
        ids.append(lm_id), pts.append(lm_3d), src.append(np.full(len(lm_id), k, np.int64))
        n += len(lm_id)
        recorded += 1
    return dict(ids=np.concatenate(ids), pts=np.concatenate(pts), run=np.concatenate(src), runs=recorded, dropped=dropped)


def select(rec, mode):
    """indices into the record that the mode keeps, ascending (= record order)"""
    n = len(rec["ids"])
    if mode == ALL:
        return np.arange(n)
    assert mode == LATEST
    last = {}
    for i in range(n):            # a later entry of the same id replaces the earlier one
        last[int(rec["ids"][i])] = i
    return np.array(sorted(last.values()), np.int64)


def raw(rec, mode):
    """leaf == 0 -> (xyz float32 [k, 3], ids int64 [k], n_dropped): every kept entry with finite coordinates, rounded once to float"""
    sel = select(rec, mode)
    P, I = rec["pts"][sel], rec["ids"][sel]
    fin = np.isfinite(P).all(axis=1)
    return P[fin].astype(np.float32), I[fin], int((~fin).sum())


def as_case(points):
    """a list of fp64 point sets as flvis_hip_voxel_cloud's input: one row each, identity poses -> (case, clouds)"""
    cap = max([len(p) for p in points] + [1])
    p3 = np.zeros((len(points), cap, 3))
    for r, p in enumerate(points):
        p3[r, :len(p)] = p
    case = dict(p3=p3, count=np.array([len(p) for p in points], np.int32), T=np.tile(MC.IDENT, (len(points), 1)))
    return case, [[(r, 1)] for r in range(len(points))]


def voxel(rec, mode, leaf, min_points=1):
    """leaf > 0 -> tests/_map_cloud.py's restate() of the kept entries"""
    case, clouds = as_case([rec["pts"][select(rec, mode)]])
    return MC.restate(case, clouds[0], leaf, min_points)


def runs_from_corrections(corrs):
    """the non-None corrections of a stream (dicts of Tracker.correction / ba_push_keyframe) as runs"""
    return [(c["frame_id"], c["lm_id"], c["lm_3d"]) for c in corrs if c is not None]


def edge_runs(seed=5):
    """A hand-made history that reaches the edges the device tests rely on: ids listed by several runs with other estimates, an id that
    is absent from a run between two that list it, a run without landmarks, a non-finite point."""
    rng = np.random.default_rng(seed)
    def pts(ids, k):
        return np.stack([0.1 * ids + 0.01 * k, 0.05 * ids - 0.02 * k, 2.0 + 0.001 * ids * k], 1).astype(np.float64) + rng.normal(0, 1e-3, (len(ids), 3))
    r0 = np.array([100, 101, 102, 103, 104], np.int64)
    r1 = np.array([101, 103, 104, 105], np.int64)             # 100 and 102 leave
    r2 = np.zeros(0, np.int64)                                # a run without multi-view landmarks
    r3 = np.array([100, 101, 105, 106, 107, 102], np.int64)   # 100 and 102 come back (absent from r1), in another order
    runs = [(10, r0, pts(r0, 0)), (13, r1, pts(r1, 1)), (16, r2, pts(r2, 2)), (19, r3, pts(r3, 3))]
    runs[3][2][4, 1] = np.inf                                 # id 107: dropped by the cloud, kept by the record
    return runs
