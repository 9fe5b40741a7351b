"""Test helper: occupancy map queries (flvis_hip_occupancy_cast, include/flvis_hip.h) restated twice, and the inputs of their edge tests.

`cast` is vectorised over the queries of one map: the cells and entry parameters come from _occupancy.walk through its `trace` (the
occupancy map's own walk, so a query visits the cells a ray of the map visited), all queries advance one cell per round, and a cell's row
is np.searchsorted over the map's keys.  `cast_loops` is a second write-up with Python floats, its own walk loop, a dict from key to
row and struct-narrowed float32; it shares no code with the first.

A JOB is dict(name, keys int64 [k], l float32 [k], seg float64 [q, 6], leaf, prm=dict(thres, ignore_unknown, max_cells)) and, for the
rows-beyond-n_rows case, slack=(keys, l): rows that stand behind the map's rows in the caller's arrays and are not part of the map.
A result is dict(status, k, cell, row, l, t, counts [5], cells_tested)."""
import math
import struct

import numpy as np

import _occupancy as OC

HALF = OC.HALF
END, OCCUPIED, UNKNOWN, DROPPED, LIMIT = range(5)
F32 = np.float32
LEAF = 0.125                     # a power of two: cell centres, faces and tmax are exact
FIELDS = ("status", "k", "cell", "row", "l", "t")
KINDS = (np.int32, np.int32, np.int64, np.int32, np.float32, np.float64)


def _finish(out):
    out["counts"] = np.bincount(out["status"], minlength=5).astype(np.int64)
    live = out["status"] != DROPPED
    out["cells_tested"] = int((out["k"][live].astype(np.int64) + (out["status"][live] != LIMIT)).sum())
    return out


def cast(keys, l, seg, leaf, thres=0.0, ignore_unknown=False, max_cells=0):
    keys, l, thres = np.asarray(keys, np.int64), np.asarray(l, np.float32), np.float32(thres)
    seg = np.asarray(seg, np.float64).reshape(-1, 6)
    nq = len(seg)
    out = dict(status=np.full(nq, DROPPED, np.int32), k=np.zeros(nq, np.int32), cell=np.full(nq, -1, np.int64), row=np.full(nq, -1, np.int32),
               l=np.zeros(nq, np.float32), t=np.zeros(nq, np.float64))
    idx = np.flatnonzero(OC.cells(seg[:, :3], leaf)[0] & OC.cells(seg[:, 3:], leaf)[0])
    if len(idx) == 0:
        return _finish(out)
    o, p = seg[idx, :3], seg[idx, 3:]
    trace = []
    steps = OC.walk(o, p, leaf, trace)[2]
    c = OC.cells(o, leaf)[1].copy()
    sgn = np.where(OC.cells(p, leaf)[1] >= c, 1, -1).astype(np.int64)
    t = np.zeros(len(idx))
    todo = np.ones(len(idx), bool)
    tab_k = np.concatenate([keys, [np.int64(-1)]])          # (a row behind the end, so that an index of len(keys) reads something)
    tab_l = np.concatenate([l, [np.float32(0)]]).astype(np.float32)
    kk = 0

    def put(who, status, row, val):
        g = idx[who]
        out["status"][g], out["k"][g], out["cell"][g], out["t"][g] = status, kk, OC.key_of(c[who]), t[who]
        out["row"][g], out["l"][g] = row, val

    while todo.any():
        u = np.flatnonzero(todo)
        if max_cells > 0 and kk == max_cells:
            put(u, LIMIT, -1, np.float32(0))
            break
        ck = OC.key_of(c[u])
        pos = np.searchsorted(keys, ck)
        found = tab_k[pos] == ck
        row = np.where(found, pos, -1)
        val = np.where(found, tab_l[pos], np.float32(0)).astype(np.float32)
        with np.errstate(invalid="ignore"):
            occ = found & (val > thres)
        unk = ~found & (not ignore_unknown)
        stop = occ | unk | (steps[u] == kk)
        put(u[stop], np.where(occ, OCCUPIED, np.where(unk, UNKNOWN, END))[stop], row[stop], val[stop])
        todo[u[stop]] = False
        go = u[~stop]
        if len(go):
            live, axis, tmax = trace[kk]
            assert live[go].all()
            a = axis[go]
            t[go] = tmax[go, a]
            c[go, a] += sgn[go, a]
        kk += 1
    return _finish(out)


# ---- the second write-up ----------------------------------------------------------------------------------------------------------
def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _index(x, leaf):
    if not math.isfinite(x):
        return None
    f = math.floor(x / leaf)
    return f if -HALF <= f < HALF else None


def _one(table, vals, s, leaf, th, ignore_unknown, max_cells):
    io = [_index(s[a], leaf) for a in range(3)]
    ie = [_index(s[3 + a], leaf) for a in range(3)]
    if None in io or None in ie:
        return DROPPED, 0, -1, -1, 0.0, 0.0
    rem = [abs(ie[a] - io[a]) for a in range(3)]
    up = [ie[a] >= io[a] for a in range(3)]
    tmax, tdel = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for a in range(3):
        if rem[a]:
            d = s[3 + a] - s[a]
            tmax[a] = (float(io[a] + (1 if up[a] else 0)) * leaf - s[a]) / d
            tdel[a] = leaf / abs(d)
    c, k, t = list(io), 0, 0.0
    while True:
        key = ((c[2] + HALF) << 42) | ((c[1] + HALF) << 21) | (c[0] + HALF)
        if max_cells > 0 and k == max_cells:
            return LIMIT, k, key, -1, 0.0, t
        row = table.get(key, -1)
        if row >= 0 and vals[row] > th:
            return OCCUPIED, k, key, row, vals[row], t
        if row < 0 and not ignore_unknown:
            return UNKNOWN, k, key, -1, 0.0, t
        if rem == [0, 0, 0]:
            return END, k, key, row, (vals[row] if row >= 0 else 0.0), t
        pick = None
        for a in range(3):
            if rem[a] and (pick is None or tmax[a] < tmax[pick]):
                pick = a
        t = tmax[pick]
        tmax[pick] = tmax[pick] + tdel[pick]
        c[pick] += 1 if up[pick] else -1
        rem[pick] -= 1
        k += 1


def cast_loops(keys, l, seg, leaf, thres=0.0, ignore_unknown=False, max_cells=0):
    table = {int(key): r for r, key in enumerate(keys)}
    vals = [_f32(float(v)) for v in l]
    th = _f32(float(thres))
    rows = [_one(table, vals, [float(v) for v in s], float(leaf), th, bool(ignore_unknown), int(max_cells))
            for s in np.asarray(seg, np.float64).reshape(-1, 6).tolist()]
    out = {f: np.array([r[i] for r in rows], kind).reshape(-1) for i, (f, kind) in enumerate(zip(FIELDS, KINDS))}
    return _finish(out)


def same(a, b, what=""):
    for f in FIELDS:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), (what, f, a[f], b[f])
    assert np.array_equal(a["counts"], b["counts"]) and a["cells_tested"] == b["cells_tested"], (what, "counts")


def both(job):
    """the job through both write-ups, which must agree -> the result"""
    a = cast(job["keys"], job["l"], job["seg"], job["leaf"], **job["prm"])
    same(a, cast_loops(job["keys"], job["l"], job["seg"], job["leaf"], **job["prm"]), job["name"])
    return a


# ---- input builders ---------------------------------------------------------------------------------------------------------------
def centre(cell, leaf=LEAF):
    return [(float(i) + 0.5) * leaf for i in cell]


def seg_cells(a, b, leaf=LEAF):
    """the segment from the centre of cell a to the centre of cell b"""
    return centre(a, leaf) + centre(b, leaf)


def make_map(rows):
    """[(cell, l), ..] -> (keys ascending, l)"""
    keys = OC.key_of(np.array([c for c, _ in rows], np.int64).reshape(-1, 3))
    order = np.argsort(keys, kind="stable")
    return keys[order], np.array([v for _, v in rows], np.float32)[order]


def job(name, rows, seg, leaf=LEAF, slack=None, **prm):
    keys, l = make_map(rows) if isinstance(rows, list) else rows
    p = dict(dict(thres=0.0, ignore_unknown=False, max_cells=0), **prm)
    j = dict(name=name, keys=keys, l=l, seg=np.asarray(seg, np.float64).reshape(-1, 6), leaf=leaf, prm=p)
    if slack is not None:
        j["slack"] = slack
    return j


WALKS = [seg_cells((0, 0, 0), (4, 4, 4)), seg_cells((0, 0, 0), (0, 0, 8)), seg_cells((2, -1, 3), (2, -1, 3)), seg_cells((3, 1, 0), (-2, 5, -1))]
NONE = (np.zeros(0, np.int64), np.zeros(0, np.float32))


def empty_jobs():
    return [job("empty map", NONE, WALKS), job("empty map, unknown ignored", NONE, WALKS, ignore_unknown=True)]


def one_row_jobs():
    seg = [seg_cells((0, 0, 0), (3, 0, 0)), seg_cells((1, 0, 0), (1, 0, 0)), seg_cells((0, 0, 0), (0, 0, 0)), seg_cells((2, 0, 0), (2, 0, 0))]
    return [job("one occupied row", [((1, 0, 0), 1.0)], seg, ignore_unknown=True), job("one occupied row, unknown stops", [((1, 0, 0), 1.0)], seg),
            job("one free row", [((1, 0, 0), -1.0)], seg, ignore_unknown=True)]


TABLE = [((-3, 0, 0), -0.5), ((0, 0, 0), 0.75), ((1, 0, 0), -1.0), ((5, 2, 1), 2.0)]


def table_end_jobs():
    """point lookups: the first row, the last row, a key below the smallest (two of them), a key above the largest (two)"""
    pts = [(-3, 0, 0), (5, 2, 1), (-4, 0, 0), (0, 0, -1), (6, 2, 1), (0, 0, 2), (0, 0, 0)]
    return [job("table ends", TABLE, [seg_cells(c, c) for c in pts])]


def range_jobs():
    """leaf 0.125: x = -131072.0 is exactly the lower face of cell -2^20, the double below 131072.0 lies in cell 2^20 - 1"""
    lo, hi = -HALF * LEAF, np.nextafter(HALF * LEAF, 0.0)
    lo_out, hi_out = np.nextafter(lo, -np.inf), HALF * LEAF
    h = LEAF / 2
    rows = [((-HALF, 0, 0), 1.0), ((HALF - 1, 0, 0), 1.0), ((-HALF + 1, 0, 0), -1.0), ((-HALF + 2, 0, 0), -1.0)]
    seg = [[lo, h, h, lo, h, h], [hi, h, h, hi, h, h], [lo_out, h, h, lo_out, h, h], [hi_out, h, h, hi_out, h, h],
           [h, h, h, lo_out, h, h], [hi_out, h, h, h, h, h], [h, lo_out, h, h, h, h], [h, h, h, h, h, hi_out],
           centre((-HALF + 2, 0, 0)) + [lo, h, h]]
    for a in range(6):
        for v in (np.nan, np.inf, -np.inf):
            s = seg_cells((0, 0, 0), (2, 1, 0))
            s[a] = v
            seg.append(s)
    return [job("index range", rows, seg)]


def line_rows(n, axis, last=1.0):
    """n cells along one axis from the origin's cell, free but the last"""
    cells = np.zeros((n, 3), np.int64)
    cells[:, axis] = np.arange(n)
    return [(tuple(int(v) for v in c), -1.0) for c in cells[:-1]] + [(tuple(int(v) for v in cells[-1]), last)]


def cube_rows(n, l=-1.0):
    return [((x, y, z), l) for z in range(n) for y in range(n) for x in range(n)]


def walk_edge_jobs():
    diag, face = seg_cells((0, 0, 0), (4, 4, 4)), [2 * LEAF, LEAF / 2, LEAF / 2, -1.5 * LEAF, LEAF / 2, 4.5 * LEAF]
    cube = cube_rows(5)
    slab = [((x, 0, z), -1.0) for x in range(-2, 3) for z in range(5)]
    jobs = [job("diagonal tie, limit %d" % k, cube, [diag], max_cells=k) for k in (1, 2, 3, 4)]
    jobs += [job("diagonal tie", cube, [diag]), job("origin on a face, limit 1", slab, [face], max_cells=1), job("origin on a face", slab, [face]),
             job("axis-parallel and zero-step", line_rows(9, 2, last=-1.0), [seg_cells((0, 0, 0), (0, 0, 8)), seg_cells((0, 0, 3), (0, 0, 3))])]
    return jobs


def value_jobs():
    above = float(np.nextafter(F32(0.5), F32(1.0)))
    rows = [((0, 0, 0), 0.5), ((1, 0, 0), above), ((2, 0, 0), float("nan")), ((3, 0, 0), -0.25), ((4, 0, 0), -0.2), ((5, 0, 0), -0.3)]
    pts = [seg_cells((x, 0, 0), (x, 0, 0)) for x in range(6)]
    return [job("values at thres 0.5", rows, pts, thres=0.5), job("values at a negative thres", rows, pts, thres=-0.25),
            job("a NaN value on a ray", rows, [seg_cells((2, 0, 0), (3, 0, 0))], thres=0.5)]


def limit_jobs():
    rows, seg = line_rows(6, 0, last=-1.0), [seg_cells((0, 0, 0), (5, 0, 0))]
    return [job("max_cells %d of n = 5" % k, rows, seg, max_cells=k) for k in (1, 5, 6)]


def unknown_jobs():
    rows = [((0, 0, 0), -1.0), ((2, 0, 0), 1.0), ((3, 0, 0), -1.0)]
    seg = [seg_cells((0, 0, 0), (3, 0, 0)), seg_cells((2, 0, 0), (0, 0, 0))]
    return [job("occupied behind unknown", rows, seg), job("occupied behind unknown, ignored", rows, seg, ignore_unknown=True)]


def slack_jobs():
    """the caller's arrays hold rows behind the map's rows whose keys the queries ask for"""
    rows = [((0, 0, 0), -1.0), ((1, 0, 0), -1.0)]
    slack = make_map([((2, 0, 0), 1.0), ((3, 0, 0), 1.0)])
    seg = [seg_cells((0, 0, 0), (3, 0, 0)), seg_cells((2, 0, 0), (2, 0, 0)), seg_cells((3, 0, 0), (3, 0, 0))]
    return [job("rows beyond n_rows", rows, seg, slack=slack), job("rows beyond n_rows, unknown ignored", rows, seg, slack=slack, ignore_unknown=True)]


SLAB = (4, 60, 50)      # 3000 (iz, iy) lines of four rows: more lines than a workgroup has lanes


def slab_map():
    nx, ny, nz = SLAB
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cells = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    l = np.where((cells.sum(axis=1) % 97) == 0, 1.5, -1.0).astype(np.float32)
    l[0] = -1.0
    return OC.key_of(cells), l          # (z-major, then y, then x: ascending as built)


def slab_segments(n=192, seed=5):
    rng = np.random.default_rng(seed)
    nx, ny, nz = SLAB
    a = rng.uniform([0, 0, 0], [nx, ny, nz], (n, 3)) * LEAF
    b = rng.uniform([-1, -2, -2], [nx + 1, ny + 2, nz + 2], (n, 3)) * LEAF
    return np.concatenate([a, b], axis=1)


def directory_jobs():
    jobs = []
    for axis, name in enumerate("xyz"):
        end = [0, 0, 0]
        end[axis] = 299
        back = seg_cells(tuple(end), (0, 0, 0))
        jobs.append(job("300 cells along " + name, line_rows(300, axis), [seg_cells((0, 0, 0), tuple(end)), back]))
        jobs.append(job("300 cells along %s, all free" % name, line_rows(300, axis, last=-1.0), [seg_cells((0, 0, 0), tuple(end)), back]))
    keys_l = slab_map()
    jobs += [job("slab of 3000 lines", keys_l, slab_segments()), job("slab of 3000 lines, unknown ignored", keys_l, slab_segments(), ignore_unknown=True),
             job("slab of 3000 lines, nothing occupied", keys_l, slab_segments(), thres=2.0, ignore_unknown=True, max_cells=40)]
    return jobs


def all_jobs():
    return (empty_jobs() + one_row_jobs() + table_end_jobs() + range_jobs() + walk_edge_jobs() + value_jobs() + limit_jobs() + unknown_jobs() +
            slack_jobs() + directory_jobs())


def builder_case(leaf=LEAF):
    """the occupancy map's own random case -> (case, o, p of the first scan's rays, their step counts)"""
    case = OC.random_case(seed=3, n=3, h=37, w=70, step=(7, 7))
    o, p, _ = OC.scan_rays(case, 0, case["cams"][0], leaf)
    return case, o, p, OC.walk(o, p, leaf)[2]
