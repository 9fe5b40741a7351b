"""Test helper: the occupancy map (flvis_hip_occupancy, include/flvis_hip.h) restated twice in numpy, and the inputs of its edge tests.

`restate` is vectorised over the rays of a scan: the rays' end points are _depth_cloud.samples through _map_cloud.transform (the dense
cloud's own restatement, so a ray ends in the dense cloud's point), the origin is the same transform of (0, 0, 0), the walk advances all
rays of the scan together one step at a time with numpy's elementwise float64 operations (the IEEE operations of the kernel; nothing is
fused), observations are np.unique over (key, hit), and the value is a float32 fold in scan order.  `restate_loops` is a second write-up
with Python floats, plain loops, a dict per voxel and struct-narrowed float32 that shares no code with the first -- not the sampling, not
the transform, not the walk.

A case is _depth_cloud's: dict(depth uint16 [n, h, w], T float64 [n, 7], clouds = maps [[(first image, count), ..], ..], cams one per
range, prm).  OCC is octomap's documented log-odds, the defaults of flvis_occupancy_params_default."""
import math
import struct

import numpy as np

import _depth_cloud as DC
import _map_cloud as MC

HALF = MC.HALF
OCC = dict(l_hit=0.85, l_miss=-0.4, l_min=-2.0, l_max=3.5)


def key_of(i):
    """int64 keys of index triples [.., 3] (x, y, z)"""
    i = np.asarray(i, np.int64) + HALF
    return (i[..., 2] << 42) | (i[..., 1] << 21) | i[..., 0]


def index_of(keys):
    k = np.asarray(keys, np.int64)
    return np.stack([(k & 0x1FFFFF) - HALF, ((k >> 21) & 0x1FFFFF) - HALF, ((k >> 42) & 0x1FFFFF) - HALF], axis=-1)


def centres(keys, leaf):
    return ((index_of(keys).astype(np.float64) + 0.5) * np.float64(leaf)).astype(np.float32).reshape(-1, 3)


def cells(P, leaf):
    """-> (ok mask, int64 indices [n, 3]; rows that are not ok hold 0)"""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(P, np.float64) / np.float64(leaf))
        ok = ((f >= -HALF) & (f < HALF)).all(axis=1)                 # (NaN and Inf compare false)
    return ok, np.where(ok[:, None], f, 0).astype(np.int64)


def walk(o, p, leaf, trace=None):
    """the walk of n rays o -> p (float64 [n, 3], every one inside the index range) -> (free keys as a list of int64 arrays, one per step
    round, hit keys [n], steps [n]).  trace: a list that receives per round (stepping mask, chosen axis, tmax before the step)."""
    leaf = np.float64(leaf)
    _, io = cells(o, leaf)
    _, ie = cells(p, leaf)
    rem = np.abs(ie - io)
    sgn = np.where(ie >= io, 1, -1).astype(np.int64)
    steps = rem.sum(axis=1)
    with np.errstate(all="ignore"):
        d = p - o
        tmax = ((io + (sgn > 0)).astype(np.float64) * leaf - o) / d
        tdel = leaf / np.fabs(d)
    c = io.copy()
    free = []
    for _ in range(int(steps.max()) if len(steps) else 0):
        live = rem.sum(axis=1) > 0
        free.append(key_of(c[live]))
        a = np.full(len(c), -1)
        best = np.zeros(len(c))
        for ax in range(3):
            with np.errstate(invalid="ignore"):
                take = (rem[:, ax] > 0) & ((a < 0) | (tmax[:, ax] < best))
            a = np.where(take, ax, a)
            best = np.where(take, tmax[:, ax], best)
        if trace is not None:
            trace.append((live.copy(), a.copy(), tmax.copy()))
        r = np.flatnonzero(live)
        ar = a[r]
        c[r, ar] += sgn[r, ar]
        rem[r, ar] -= 1
        tmax[r, ar] = tmax[r, ar] + tdel[r, ar]
    assert (c == ie).all(), "a walk ends in its end cell by construction"
    return free, key_of(ie), steps


def scan_rays(case, image, cam, leaf):
    """one scan -> (o [k, 3], p [k, 3] of the rays cast, n_dropped)"""
    p_c, _ = DC.samples(case["depth"][image], cam, case["prm"])
    T = np.tile(np.asarray(case["T"][image], np.float64), (len(p_c), 1))
    p = MC.transform(p_c, T)
    o = MC.transform(np.zeros_like(p_c), T)
    ok = cells(o, leaf)[0] & cells(p, leaf)[0]
    return o[ok], p[ok], int((~ok).sum())


def observe(o, p, leaf):
    """one scan's observations -> (keys ascending, hit bool) with at most one row per voxel: occupied wins"""
    free, hit, _ = walk(o, p, leaf)
    hk = np.unique(hit)
    fk = np.unique(np.concatenate(free)) if free else np.zeros(0, np.int64)
    fk = fk[~np.isin(fk, hk)]
    keys = np.concatenate([hk, fk])
    hits = np.concatenate([np.ones(len(hk), bool), np.zeros(len(fk), bool)])
    order = np.argsort(keys, kind="stable")
    return keys[order], hits[order]


def fold(vox, keys, hits, occ=OCC):
    """applies one scan's observations to vox {key: float32}"""
    lh, lm, lo, hi = (np.float32(occ[k]) for k in ("l_hit", "l_miss", "l_min", "l_max"))
    for k, h in zip(keys.tolist(), hits.tolist()):
        l = np.float32(vox.get(k, np.float32(0.0)) + (lh if h else lm))
        vox[k] = lo if l < lo else (hi if l > hi else l)


def restate(case, m, leaf, occ=OCC, prior=None, scans=None):
    """map m -> dict(keys int64 [k], l float32 [k], xyz float32 [k, 3], n_out, n_rays, n_dropped, records).  prior: (keys, l); scans: a
    slice of the map's scans (default all)"""
    vox = {}
    if prior is not None:
        vox = {int(k): np.float32(v) for k, v in zip(prior[0], prior[1])}
    items = DC.listed(case, m)
    n_rays = n_dropped = records = 0
    for image, cam in (items if scans is None else items[scans]):
        o, p, nd = scan_rays(case, image, cam, leaf)
        n_rays, n_dropped = n_rays + len(o), n_dropped + nd
        if len(o):
            keys, hits = observe(o, p, leaf)
            records += int(walk(o, p, leaf)[2].sum()) + len(o)
            fold(vox, keys, hits, occ)
    keys = np.array(sorted(vox), np.int64)
    return dict(keys=keys, l=np.array([vox[k] for k in keys.tolist()], np.float32), xyz=centres(keys, leaf), n_out=len(keys), n_rays=n_rays,
                n_dropped=n_dropped, records=records)


# ---- the second write-up ----------------------------------------------------------------------------------------------------------
def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _rot(T, x, y, z):
    tx, ty, tz, qx, qy, qz, qw = [float(v) for v in T]
    qx, qy, qz = -qx, -qy, -qz
    vx, vy, vz = x - tx, y - ty, z - tz
    ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return (vx + qw * ux + (qy * uz - qz * uy), vy + qw * uy + (qz * ux - qx * uz), vz + qw * uz + (qx * uy - qy * ux))


def _cell(p, leaf):
    out = []
    for c in p:
        if not math.isfinite(c):
            return None
        f = math.floor(c / leaf)
        if not -HALF <= f < HALF:
            return None
        out.append(f)
    return out


def walk_loops(o, p, leaf):
    """one ray -> (free cells as (x, y, z) tuples in walk order, the hit cell)"""
    io, ie = _cell(o, leaf), _cell(p, leaf)
    rem = [abs(ie[a] - io[a]) for a in range(3)]
    sgn = [1 if ie[a] >= io[a] else -1 for a in range(3)]
    tmax, tdel = [0.0] * 3, [0.0] * 3
    for a in range(3):
        if rem[a] > 0:
            tmax[a] = (float(io[a] + (1 if sgn[a] > 0 else 0)) * leaf - o[a]) / (p[a] - o[a])
            tdel[a] = leaf / abs(p[a] - o[a])
    c, free = list(io), []
    for _ in range(sum(rem)):
        free.append(tuple(c))
        pick = -1
        for a in range(3):
            if rem[a] > 0 and (pick < 0 or tmax[a] < tmax[pick]):
                pick = a
        c[pick] += sgn[pick]
        rem[pick] -= 1
        tmax[pick] = tmax[pick] + tdel[pick]
    assert c == ie
    return free, tuple(ie)


def restate_loops(case, m, leaf, occ=OCC, prior=None):
    lh, lm, lo, hi = (_f32(occ[k]) for k in ("l_hit", "l_miss", "l_min", "l_max"))
    vox = {}
    if prior is not None:
        for k, v in zip(prior[0], prior[1]):
            x, y, z = [int(t) for t in index_of(int(k))]
            vox[(z, y, x)] = float(v)
    n_rays = n_dropped = 0
    r0 = sum(len(c) for c in case["clouds"][:m])
    for k, (first, n) in enumerate(case["clouds"][m]):
        cam = case["cams"][r0 + k]
        for image in range(first, first + n):
            pts, _ = DC.samples_loops(case["depth"][image].tolist(), cam, case["prm"])
            T = case["T"][image]
            o = _rot(T, 0.0, 0.0, 0.0)
            seen = {}                                               # this scan's observations: cell -> hit
            for x, y, z in pts.tolist():
                p = _rot(T, x, y, z)
                if _cell(o, leaf) is None or _cell(p, leaf) is None:
                    n_dropped += 1
                    continue
                n_rays += 1
                free, hit = walk_loops(o, p, leaf)
                for c in free:
                    seen.setdefault((c[2], c[1], c[0]), False)
                seen[(hit[2], hit[1], hit[0])] = True
            for c, h in seen.items():                               # (a voxel's value depends on its own observations alone)
                l = _f32(vox.get(c, 0.0) + (lh if h else lm))
                vox[c] = lo if l < lo else (hi if l > hi else l)
    order = sorted(vox)
    keys = np.array([((z + HALF) << 42) | ((y + HALF) << 21) | (x + HALF) for z, y, x in order], np.int64)
    xyz = np.array([[np.float32((x + 0.5) * leaf), np.float32((y + 0.5) * leaf), np.float32((z + 0.5) * leaf)] for z, y, x in order],
                   np.float32).reshape(-1, 3)
    return dict(keys=keys, l=np.array([vox[c] for c in order], np.float32), xyz=xyz, n_out=len(order), n_rays=n_rays, n_dropped=n_dropped)


def same(a, b, what=""):
    assert (a["n_out"], a["n_rays"], a["n_dropped"]) == (b["n_out"], b["n_rays"], b["n_dropped"]), (what, "counts")
    assert np.array_equal(a["keys"], b["keys"]), (what, "keys")
    assert a["l"].tobytes() == b["l"].tobytes(), (what, "values")
    assert a["xyz"].tobytes() == b["xyz"].tobytes(), (what, "centres")


# ---- input builders ---------------------------------------------------------------------------------------------------------------
CAM_UNIT = [1.0, 1.0, 0.0, 0.0, 1000.0]     # p_c = (u z, v z, z): with z a power of two, exact


def ray_case(ends, origins=None):
    """one scan of ONE ray each: a 1 x 1 image whose pixel (0, 0) under CAM_UNIT at depth z = ends[i] is p_c = (0, 0, z), under an identity
    rotation.  -> a case with one map of len(ends) scans whose rays run from origins[i] to origins[i] + (0, 0, ends[i]): the
    axis-parallel and zero-step rays"""
    ends = np.asarray(ends, np.float64).reshape(-1)
    n = len(ends)
    origins = np.zeros((n, 3)) if origins is None else np.asarray(origins, np.float64).reshape(n, 3)
    depth = np.round(ends * 1000).astype(np.uint16).reshape(n, 1, 1)
    T = np.tile(MC.IDENT, (n, 1))
    T[:, :3] = -origins             # (T is T_c_w, p = q^-1 (p_c - t): under the identity rotation the ray starts at 0 - t)
    return dict(depth=depth, T=T, clouds=[[(0, n)]], cams=[CAM_UNIT], prm=DC.params(z_min=0.0005, z_max=60.0))


def pixel_case(pixels, z, w, h, T=None, n=1, cam=CAM_UNIT):
    """n identical images (n scans of one map) that are valid at `pixels` [(u, v), ..] alone, all at depth z metres"""
    d = np.zeros((n, h, w), np.uint16)
    for u, v in pixels:
        d[:, v, u] = int(round(z * 1000))
    return dict(depth=d, T=np.tile(MC.IDENT, (n, 1)) if T is None else np.asarray(T, np.float64).reshape(n, 7), clouds=[[(0, n)]],
                cams=[list(cam)], prm=DC.params(z_min=0.0005, z_max=60.0))


def diagonal_case(leaf=0.125, cells_out=4):
    """origin at the centre of voxel (0, 0, 0), end at the centre of voxel (k, k, k): the camera sits at (leaf / 2,) * 3 and pixel (1, 1)
    at depth k * leaf under CAM_UNIT is p_c = (k leaf, k leaf, k leaf) -- every number a small multiple of a power of two, so tmax is
    exact and the three tmax are EQUAL at every third step"""
    z = cells_out * leaf
    T = np.array([[-leaf / 2, -leaf / 2, -leaf / 2, 0, 0, 0, 1.0]])
    return pixel_case([(1, 1)], z, 2, 2, T=T)


def face_case(leaf=0.125):
    """origin exactly on the voxel face x = 2 leaf, walking towards -x: io.x = 2, sgn.x = -1, tmax.x = (2 leaf - o.x) / d.x = 0"""
    T = np.array([[-2 * leaf, -leaf / 2, -leaf / 2, 0, 0, 0, 1.0]])
    case = pixel_case([(0, 0)], 4 * leaf, 2, 2, T=T, cam=[1.0, 1.0, 1.0, 0.0, 1000.0])   # p_c = (-z, 0, z)
    return case


def wall_scans(n, leaf=0.125, w=9, h=7, z=1.0):
    """n scans of one flat wall from one pose: every wall voxel is hit n times, every crossed cell missed n times"""
    return pixel_case([(u, v) for u in range(w) for v in range(h)], z, w, h, n=n, cam=[8.0, 8.0, 4.0, 3.0, 1000.0])


def order_case(hits_first, leaf=0.125):
    """six scans along one line: the voxel at z = 1 m is the END of five of them (z = 1.0) and CROSSED by one (z = 2.0); hits_first puts
    the five hits in front.  -> (case, the voxel's key)"""
    z = [1.0] * 5 + [2.0] if hits_first else [2.0] + [1.0] * 5
    case = ray_case(z, origins=np.tile([leaf / 2, leaf / 2, leaf / 2], (6, 1)))
    i = int(math.floor((leaf / 2 + 1.0) / leaf))
    return case, int(key_of([0, 0, i]))


def crossed_and_hit_case(leaf=0.125):
    """one scan of two nearly parallel rays from the centre of voxel (0, 0, 0) (focal length 1000): the ray of pixel (0, 0) ENDS in voxel
    (0, 0, 8), the ray of pixel (1, 0) goes on to z = 2 m and CROSSES it.  -> (case, the voxel's key)"""
    d = np.array([[[1000, 2000]]], np.uint16)
    T = np.array([[-leaf / 2, -leaf / 2, -leaf / 2, 0, 0, 0, 1.0]])
    case = dict(depth=d, T=T, clouds=[[(0, 1)]], cams=[[1000.0, 1000.0, 0.0, 0.0, 1000.0]], prm=DC.params(z_min=0.0005, z_max=60.0))
    return case, int(key_of([0, 0, 8]))


def random_case(seed, n, h, w, step, poses=True, **kw):
    return DC.random_case(seed, n, h, w, DC.params(step=step, z_min=0.3, z_max=6.5), poses=poses, **kw)


def hazard_case():
    """one 129 x 96 image at step 1: every ray starts in the origin voxel, so that voxel's run holds one record per ray"""
    rng = np.random.default_rng(41)
    d = DC.wall(rng, 1, 96, 129, raw=1500, spread=40, holes=0.02)
    return DC.one_cloud(d, cam=[120.0, 118.0, 64.2, 47.9, 1000.0], prm=DC.params(z_min=0.3, z_max=6.5), T=MC.random_unit_poses(rng, 1))
