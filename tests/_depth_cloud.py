"""Test helper: the dense cloud (flvis_hip_depth_cloud, include/flvis_hip.h) restated in numpy, and the inputs of its edge tests.

`samples` performs the sample rule's operations in the rule's order -- raw as unsigned 16 bit, z = float32(float64(raw) / depth_factor),
valid iff z_min <= float64(z) <= z_max, p_c = ((u - cx) * z / fx, (v - cy) * z / fy, z) in float64, left to right (numpy's elementwise
float32 / float64 operations are the IEEE operations of the kernel; nothing is fused) -- and `restate` hands the listed images' valid
p_c in canonical order, with their poses, to _map_cloud.restate: the definition of the result.  `samples_loops` / `restate_loops` are
a second write-up with Python floats (struct narrows to float32) and plain loops that shares no code with the first.

A case is dict(depth uint16 [n, h, w], T float64 [n, 7], clouds [[(first image, count), ..], ..], cams [[fx, fy, cx, cy, depth_factor]
per range], prm dict(u0, v0, u1, v1, step_u, step_v, z_min, z_max))."""
import struct

import numpy as np

import _map_cloud as MC

CAM_A = [61.5, 60.25, 33.7, 18.2, 1000.0]      # for the small images: a few metres at raw ~ 2000 land in a metre or two of map
CAM_B = [58.0, 63.5, 36.1, 17.4, 5000.0]       # another camera on another depth_factor


def params(window=None, step=(1, 1), z_min=0.3, z_max=10.0):
    u0, v0, u1, v1 = window if window is not None else (0, 0, 0, 0)
    return dict(u0=u0, v0=v0, u1=u1, v1=v1, step_u=step[0], step_v=step[1], z_min=z_min, z_max=z_max)


def grid(prm, w, h):
    """the sampled columns and rows of a w x h image"""
    u1 = prm["u1"] if prm["u1"] > 0 else w
    v1 = prm["v1"] if prm["v1"] > 0 else h
    return np.arange(prm["u0"], u1, prm["step_u"]), np.arange(prm["v0"], v1, prm["step_v"])


def samples(img, cam, prm):
    """-> (p_c float64 [k, 3] of the valid samples in raster order, valid mask [nv, nu] over the sampled grid)"""
    assert img.dtype == np.uint16
    h, w = img.shape
    us, vs = grid(prm, w, h)
    fx, fy, cx, cy, df = [np.float64(c) for c in cam]
    raw = img[np.ix_(vs, us)]
    z = (raw.astype(np.float64) / df).astype(np.float32)
    zd = z.astype(np.float64)
    valid = (zd >= np.float64(prm["z_min"])) & (zd <= np.float64(prm["z_max"]))
    U, V = np.meshgrid(us.astype(np.float64), vs.astype(np.float64))
    x = (U - cx) * zd / fx
    y = (V - cy) * zd / fy
    return np.stack([x[valid], y[valid], zd[valid]], axis=1), valid       # (boolean indexing walks in raster order)


def listed(case, cloud_index):
    """(image, camera) of a cloud's listed images in canonical order; a camera belongs to a RANGE"""
    r0 = sum(len(c) for c in case["clouds"][:cloud_index])
    out = []
    for k, (first, n) in enumerate(case["clouds"][cloud_index]):
        out += [(i, case["cams"][r0 + k]) for i in range(first, first + n)]
    return out


def rows_case(case, cloud_index, sampler=None):
    """the _map_cloud case flvis_hip_voxel_cloud would be fed: one row per listed image with its valid p_c and its pose -> (case, n_valid)"""
    sampler = sampler or samples
    items = listed(case, cloud_index)
    if not items:
        return None, 0
    rows = [sampler(case["depth"][i], cam, case["prm"])[0] for i, cam in items]
    cap = max([len(r) for r in rows] + [1])
    T = np.array([case["T"][i] for i, _ in items], np.float64).reshape(-1, 7)
    return MC.pack(rows, cap, T=T), int(sum(len(r) for r in rows))


def restate(case, cloud_index, leaf, min_points=1):
    """-> _map_cloud.restate's dict plus n_valid"""
    mc, n_valid = rows_case(case, cloud_index)
    if mc is None:
        return dict(xyz=np.zeros((0, 3), np.float32), npts=np.zeros(0, np.int32), n_out=0, n_dropped=0, n_valid=0)
    out = MC.restate(mc, [(0, len(mc["count"]))], leaf, min_points)
    out["n_valid"] = n_valid
    return out


# ---- the second write-up ----------------------------------------------------------------------------------------------------------
def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def samples_loops(img, cam, prm):
    h, w = len(img), len(img[0])
    fx, fy, cx, cy, df = [float(c) for c in cam]
    u_end = prm["u1"] if prm["u1"] > 0 else w
    v_end = prm["v1"] if prm["v1"] > 0 else h
    pts, mask = [], []
    v = prm["v0"]
    while v < v_end:
        line = []
        u = prm["u0"]
        while u < u_end:
            raw = int(img[v][u]) & 0xFFFF
            z = _f32(raw / df)
            ok = prm["z_min"] <= z <= prm["z_max"]
            line.append(ok)
            if ok:
                pts.append([(float(u) - cx) * z / fx, (float(v) - cy) * z / fy, z])
            u += prm["step_u"]
        mask.append(line)
        v += prm["step_v"]
    return np.array(pts, np.float64).reshape(-1, 3), np.array(mask, bool)


def restate_loops(case, cloud_index, leaf, min_points=1):
    """leaf > 0: through _map_cloud.restate_dict; leaf == 0: the transformed rows themselves, by loops"""
    mc, n_valid = rows_case(case, cloud_index, sampler=samples_loops)
    if mc is None:
        return dict(xyz=np.zeros((0, 3), np.float32), npts=np.zeros(0, np.int32), n_out=0, n_dropped=0, n_valid=0)
    if leaf > 0:
        out = MC.restate_dict(mc, [(0, len(mc["count"]))], leaf, min_points)
    else:
        xyz = []
        for r in range(len(mc["count"])):
            tx, ty, tz, qx, qy, qz, qw = [float(v) for v in mc["T"][r]]
            qx, qy, qz = -qx, -qy, -qz
            for x, y, z in mc["p3"][r, :mc["count"][r]].tolist():
                vx, vy, vz = x - tx, y - ty, z - tz
                ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx
                ux, uy, uz = ux + ux, uy + uy, uz + uz
                xyz.append([vx + qw * ux + (qy * uz - qz * uy), vy + qw * uy + (qz * ux - qx * uz), vz + qw * uz + (qx * uy - qy * ux)])
        xyz = np.array(xyz, np.float64).reshape(-1, 3).astype(np.float32)
        out = dict(xyz=xyz, npts=np.ones(len(xyz), np.int32), n_out=len(xyz), n_dropped=0)
    out["n_valid"] = n_valid
    return out


# ---- input builders ---------------------------------------------------------------------------------------------------------------
def one_cloud(depth, cam=CAM_A, prm=None, T=None):
    depth = np.ascontiguousarray(depth, np.uint16)
    n = len(depth)
    return dict(depth=depth, T=np.tile(MC.IDENT, (n, 1)) if T is None else np.asarray(T, np.float64).reshape(n, 7), clouds=[[(0, n)]],
                cams=[list(cam)], prm=prm or params())


def limit_case(z_min):
    """depth_factor 1000: raw = 1000 z_min is valid -- float32(z_min) >= z_min must hold, as for 0.3 and 0.5 -- and one below is not;
    40000 (negative as a signed pixel) is 40 m and valid under z_max = 50; 0 and 65535 are invalid.  One 70 x 37 image that holds each
    value a few times among invalid filler.  -> (case, {raw: expected validity})"""
    edge = int(round(1000 * z_min))
    want = {edge: True, edge - 1: False, 40000: True, 0: False, 65535: False, 50000: True, 50001: False}
    img = np.zeros((37, 70), np.uint16)
    vals = list(want)
    for k in range(60):
        img[(k * 7) % 37, (k * 13) % 70] = vals[k % len(vals)]
    return one_cloud(img[None], cam=[61.5, 60.25, 33.7, 18.2, 1000.0], prm=params(z_min=z_min, z_max=50.0)), want


def wall(rng, n, h, w, raw=2000, spread=30, holes=0.1):
    """a near flat wall at raw +- spread with a share of invalid pixels (0)"""
    d = rng.integers(raw - spread, raw + spread + 1, (n, h, w)).astype(np.uint16)
    d[rng.random((n, h, w)) < holes] = 0
    return d


def empty_between_case(h=37, w=70):
    """three images, the middle one without a valid sample"""
    rng = np.random.default_rng(21)
    d = wall(rng, 3, h, w)
    d[1] = 0
    return one_cloud(d, prm=params(step=(3, 5)), T=MC.random_unit_poses(rng, 3))


def apart_case(gap=65, h=96, w=129):
    """valid samples exactly `gap` sampled positions apart in raster order (step 1): every wave of 64 holds at most one, and a workgroup's
    waves compact across their boundaries"""
    d = np.zeros(h * w, np.uint16)
    d[::gap] = 1500 + (np.arange(len(d[::gap])) % 700)
    return one_cloud(d.reshape(1, h, w))


def first_last_case(h=37, w=70, step=(7, 7), window=(2, 1, 66, 35)):
    """only the first and only the last SAMPLED pixel of the window are valid; every other pixel of the image is valid-looking at
    positions the sampling must not read (off the grid) and invalid on the grid"""
    prm = params(window, step)
    us, vs = grid(prm, w, h)
    d = np.full((h, w), 2000, np.uint16)
    d[np.ix_(vs, us)] = 0
    d[vs[0], us[0]], d[vs[-1], us[-1]] = 1800, 2200
    return one_cloud(d[None], prm=prm)


def random_case(seed, n, h, w, prm, poses=True, cams=(CAM_A,), clouds=None):
    rng = np.random.default_rng(seed)
    d = wall(rng, n, h, w, spread=400, holes=0.2)
    return dict(depth=d, T=MC.random_unit_poses(rng, n) if poses else np.tile(MC.IDENT, (n, 1)), clouds=clouds or [[(0, n)]],
                cams=[list(c) for c in cams], prm=prm)
