"""Test helper: the voxel cloud (flvis_hip_voxel_cloud, include/flvis_hip.h) restated in numpy, and the inputs of its edge tests.

`restate` performs the definition's operations in the definition's order on fp64 scalars (numpy's elementwise + - * / floor on float64 are
the IEEE operations the kernels use, and nothing here is fused): the transform of dev_math.hpp's q_rotate(q_conj(q), p_c - t), one
division and a floor per axis, the key, a stable sort by key, and per voxel a sum that starts with the first point and adds the others one
after another (np.add.accumulate; never np.sum, which adds pairwise).  `restate_dict` is a second write-up with Python floats and a
dictionary of voxels that shares no code with it.

A case is dict(p3 [n_rows, cap, 3] float64, count [n_rows] int32, T [n_rows, 7] float64); clouds are lists of (first row, row count)."""
import itertools
import math

import numpy as np

IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
HALF = 1 << 20


def clamp_counts(count, cap):
    return np.minimum(np.maximum(np.asarray(count, np.int64), 0), cap)


def canonical(case, cloud):
    """(row, landmark) of a cloud's points in canonical order: ranges in the caller's order, rows ascending, landmarks ascending"""
    cap = case["p3"].shape[1]
    cnt = clamp_counts(case["count"], cap)
    rows, lms = [], []
    for first, n in cloud:
        for r in range(first, first + n):
            rows.append(np.full(cnt[r], r, np.int64))
            lms.append(np.arange(cnt[r], dtype=np.int64))
    if not rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(rows), np.concatenate(lms)


def transform(p_c, T):
    """q_rotate(q_conj(q), p_c - t) per point, the operations of dev_math.hpp in their order; p_c [n, 3], T [n, 7] (tx ty tz qx qy qz qw)"""
    with np.errstate(all="ignore"):
        vx, vy, vz = p_c[:, 0] - T[:, 0], p_c[:, 1] - T[:, 1], p_c[:, 2] - T[:, 2]
        qx, qy, qz, qw = -T[:, 3], -T[:, 4], -T[:, 5], T[:, 6]
        ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx          # cross(qv, v)
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        cx, cy, cz = qy * uz - qz * uy, qz * ux - qx * uz, qx * uy - qy * ux          # cross(qv, uv)
        return np.stack([(vx + qw * ux) + cx, (vy + qw * uy) + cy, (vz + qw * uz) + cz], axis=1)


def voxel_index(p, leaf):
    """floor(p / leaf) per axis as float64 (one division, then floor)"""
    with np.errstate(all="ignore"):
        return np.floor(np.asarray(p, np.float64) / np.float64(leaf))


def keys_of(P, leaf):
    """-> (kept mask, int64 keys of the kept points)"""
    finite = np.isfinite(P).all(axis=1)
    if leaf == 0:
        return finite, np.zeros(int(finite.sum()), np.int64)
    idx = voxel_index(P, leaf)
    with np.errstate(invalid="ignore"):
        keep = finite & ((idx >= -HALF) & (idx < HALF)).all(axis=1)
    i = idx[keep].astype(np.int64) + HALF
    return keep, (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0]


def restate(case, cloud, leaf, min_points=1):
    """-> dict(xyz float32 [k, 3], npts int32 [k], keys int64 [k], n_out, n_dropped) of one cloud, nothing cut"""
    rows, lms = canonical(case, cloud)
    P = transform(case["p3"][rows, lms], case["T"][rows])
    keep, keys = keys_of(P, leaf)
    P = P[keep]
    n_dropped = int(len(rows) - len(P))
    if leaf == 0:
        return dict(xyz=P.astype(np.float32), npts=np.ones(len(P), np.int32), keys=keys, n_out=len(P), n_dropped=n_dropped)
    order = np.argsort(keys, kind="stable")
    ks, Ps = keys[order], P[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if len(ks) else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [len(ks)]]).astype(np.int64)
    xyz, npts, okeys = [], [], []
    for a, b in zip(starts, ends):
        if b - a < min_points:
            continue
        s = np.add.accumulate(Ps[a:b], axis=0)[-1]            # the first point, then one after another
        xyz.append((s / np.float64(b - a)).astype(np.float32))
        npts.append(b - a)
        okeys.append(ks[a])
    return dict(xyz=np.array(xyz, np.float32).reshape(-1, 3), npts=np.array(npts, np.int32), keys=np.array(okeys, np.int64), n_out=len(xyz),
                n_dropped=n_dropped)


def restate_dict(case, cloud, leaf, min_points=1):
    """the same result from Python floats and a dictionary of voxels (leaf > 0)"""
    cap = case["p3"].shape[1]
    vox, dropped = {}, 0
    for first, n in cloud:
        for r in range(first, first + n):
            tx, ty, tz, qx, qy, qz, qw = [float(v) for v in case["T"][r]]
            qx, qy, qz = -qx, -qy, -qz
            for lm in range(min(max(int(case["count"][r]), 0), cap)):
                x, y, z = [float(v) for v in case["p3"][r, lm]]
                vx, vy, vz = x - tx, y - ty, z - tz
                ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx
                ux, uy, uz = ux + ux, uy + uy, uz + uz
                p = (vx + qw * ux + (qy * uz - qz * uy), vy + qw * uy + (qz * ux - qx * uz), vz + qw * uz + (qx * uy - qy * ux))
                if not all(math.isfinite(c) for c in p):
                    dropped += 1
                    continue
                q = [c / leaf for c in p]
                if not all(math.isfinite(c) and -HALF <= math.floor(c) < HALF for c in q):
                    dropped += 1
                    continue
                i = tuple(math.floor(c) for c in q)
                vox.setdefault((i[2], i[1], i[0]), []).append(p)
    xyz, npts = [], []
    for k in sorted(vox):
        pts = vox[k]
        if len(pts) < min_points:
            continue
        s = list(pts[0])
        for p in pts[1:]:
            s = [s[0] + p[0], s[1] + p[1], s[2] + p[2]]
        xyz.append([np.float32(c / float(len(pts))) for c in s])
        npts.append(len(pts))
    return dict(xyz=np.array(xyz, np.float32).reshape(-1, 3), npts=np.array(npts, np.int32), n_out=len(xyz), n_dropped=dropped)


# ---- input builders ----------------------------------------------------------------------------------------------------------------------
def pack(point_rows, cap, counts=None, T=None, fill=None):
    """rows of points (lists of [k, 3]) -> case; slots past a row's points hold `fill` (default NaN: reading one would show)"""
    n = len(point_rows)
    p3 = np.full((n, cap, 3), np.nan if fill is None else fill)
    cnt = np.zeros(n, np.int32)
    for r, pts in enumerate(point_rows):
        pts = np.asarray(pts, np.float64).reshape(-1, 3)
        p3[r, :len(pts)] = pts
        cnt[r] = len(pts)
    if counts is not None:
        cnt = np.asarray(counts, np.int32)
    return dict(p3=p3, count=cnt, T=np.tile(IDENT, (n, 1)) if T is None else np.asarray(T, np.float64).reshape(n, 7))


def random_unit_poses(rng, n, reach=3.0):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    return np.concatenate([rng.uniform(-reach, reach, (n, 3)), q], axis=1)


def random_case(seed, counts, cap, poses=False, reach=2.0):
    """rows of `counts` random points a few metres out (every slot of a row is filled, so a count above cap reads real points)"""
    rng = np.random.default_rng(seed)
    n = len(counts)
    p3 = rng.uniform(-reach, reach, (n, cap, 3)) + np.array([0.0, 0.0, 4.0])
    return dict(p3=p3, count=np.asarray(counts, np.int32), T=random_unit_poses(rng, n) if poses else np.tile(IDENT, (n, 1)))


def boundary_values(leaf):
    """name -> (coordinate, the voxel index it must land in)"""
    leaf = np.float64(leaf)
    v = {"k=%d" % k: (np.float64(k) * leaf, k) for k in (-2, -1, 0, 1)}
    v["-0.0"] = (np.float64(-0.0), 0)
    v["below 0"] = (np.nextafter(np.float64(0), np.float64(-1)), -1)
    v["below leaf"] = (np.nextafter(leaf, np.float64(0)), 0)
    return v


def boundary_case(leaf, extra=()):
    """every boundary value on every axis (the other two axes inside voxel 5), and on all three at once; one point per row slot"""
    inside = 5.5 * leaf
    pts = []
    for v in [c for c, _ in boundary_values(leaf).values()] + [np.float64(k) * np.float64(leaf) for k in extra]:
        for a in range(3):
            p = [inside] * 3
            p[a] = v
            pts.append(p)
        pts.append([v, v, v])
    return pack([pts[:9], pts[9:20], pts[20:]], cap=16)


def range_case(leaf=0.125):
    """index 2^20 - 1 and -2^20 kept, 2^20 and -2^20 - 1 dropped, NaN / +Inf / -Inf dropped, on each axis; then a row with a negative count
    and one with a count above cap (its slots are all real points).  -> (case, kept points, dropped points) for the first row range"""
    kept, dropped = [], []
    for a in range(3):
        for i, keep in ((HALF - 1, True), (HALF, False), (-HALF, True), (-HALF - 1, False)):
            p = [0.5 * leaf] * 3
            p[a] = (i + 0.5) * leaf
            (kept if keep else dropped).append(p)
        for bad in (np.nan, np.inf, -np.inf):
            p = [0.5 * leaf] * 3
            p[a] = bad
            dropped.append(p)
    rng = np.random.default_rng(7)
    mixed = kept + dropped
    order = rng.permutation(len(mixed))
    rows = [[mixed[i] for i in order[:11]], [mixed[i] for i in order[11:]], rng.uniform(0, 1, (8, 3)), rng.uniform(0, 1, (8, 3))]
    case = pack(rows, cap=16, fill=0.25)
    case["p3"][2:] = rng.uniform(0, 1, (2, 16, 3))
    case["count"][2], case["count"][3] = -3, 16 + 5
    return case, np.array(kept), np.array(dropped)


def order_case(leaf=0.125):
    """points that differ in one axis alone, indices either side of 0 on each axis (the key's bias), given in descending key order"""
    idx = []
    for a in range(3):
        for i in (3, 1, 0, -1, -2):
            v = [7, 7, 7]
            v[a] = i
            idx.append(v)
    idx += [[-1, -1, -1], [0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    idx = np.array(idx, np.float64)
    keys = ((idx[:, 2].astype(np.int64) + HALF) << 42) | ((idx[:, 1].astype(np.int64) + HALF) << 21) | (idx[:, 0].astype(np.int64) + HALF)
    pts = (idx[np.argsort(-keys, kind="stable")] + 0.5) * leaf
    return pack([pts[:7], pts[7:]], cap=16)


def digit_case(leaf=0.125, n=96):
    """voxel indices over the whole range: every byte of the key takes many values, so every pass of an 8-bit radix sort runs"""
    rng = np.random.default_rng(11)
    idx = rng.integers(-HALF, HALF, (n, 3)).astype(np.float64)
    idx[0], idx[1] = [HALF - 1] * 3, [-HALF] * 3
    return pack([(idx[:40] + 0.5) * leaf, (idx[40:] + 0.5) * leaf], cap=64)


def three_row_case():
    """one voxel (leaf 16) fed from rows 4, 1, 2 -- two ranges, given as [(4, 1), (1, 2)] -- with 3 + 3 + 2 = 8 points, so the mean is the
    sum's exact eighth.  Per axis one point is B = 8 (1 + 2^-24), eight times the midpoint between two floats, and the others are fractions
    of B's last place u = 2^-49: a small point added to B is lost, small points added up BEFORE B move it by one u.  The sum is B (the mean
    is the midpoint: it rounds down, to even) or B + u (it rounds up), by which rows come before the row that holds B:
      x: B leads row 1; row 4 brings 1.2 u, row 2 0.02 u: up iff row 4 is before row 1          canonical: up
      y: B leads row 4; rows 1 and 2 bring 1.2 u and 0.8 u: up iff any row is before row 4       canonical: down
      z: B leads row 2; rows 4 and 1 bring 0.3 u each:      up iff both are before row 2         canonical: up
    so each of the five other orders of the rows changes the last bit of a float of the result.  -> (case, cloud, leaf)"""
    u, B = 2.0 ** -49, 8.0 * (1.0 + 2.0 ** -24)
    rows = [[], [[B, .4 * u, .1 * u], [.01 * u, .4 * u, .1 * u], [.01 * u, .4 * u, .1 * u]], [[.01 * u, .4 * u, B], [.01 * u, .4 * u, .1 * u]], [],
            [[.4 * u, B, .1 * u], [.4 * u, .3 * u, .1 * u], [.4 * u, .3 * u, .1 * u]]]
    return pack(rows, cap=4), [(4, 1), (1, 2)], 16.0


def long_run_case(leaf=0.125, rows=5, cap=1024):
    """rows * cap points (5120: more than a sort tile of 4096 and than any workgroup) in ONE voxel, every row full"""
    rng = np.random.default_rng(5)
    return dict(p3=(1000 + rng.uniform(0.01, 0.99, (rows, cap, 3))) * leaf, count=np.full(rows, cap, np.int32), T=np.tile(IDENT, (rows, 1)))


def sized_case(total, cap=1024, seed=3):
    """`total` points in full rows of cap with an empty row between them and the remainder in the last row"""
    counts = []
    left = total
    while left > 0:
        counts += [min(left, cap), 0]
        left -= min(left, cap)
    counts = counts or [0]
    return random_case(seed + total, counts, cap)


def closer_case(lc, seqs, cap=1024):
    """the database of a LoopCloser's sequences as a case: rows = the sequences' keyframes one after another (lc.keyframe's landmarks,
    lc.poses' T_c_w).  -> (case, {sequence: (first row, row count)})"""
    rows, T, where = [], [], {}
    for s in seqs:
        P = lc.poses(s)
        where[s] = (len(rows), len(P))
        for k in range(len(P)):
            rows.append(lc.keyframe(s, k, cap=cap)["lm3"])
            T.append(P[k])
    if not rows:
        return dict(p3=np.zeros((1, cap, 3)), count=np.zeros(1, np.int32), T=np.tile(IDENT, (1, 1))), where
    return pack(rows, cap, T=np.array(T)), where

