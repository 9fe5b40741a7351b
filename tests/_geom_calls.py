"""Inputs that drive the front-end's solver calls on caller arrays -- flvis_hip_find_fundamental_ransac (k_fund_ransac_sets),
flvis_hip_optimize_in_frame (k_pose_lm_sets), flvis_hip_undistort_points / flvis_hip_project_points (geom_calls.hip) -- to their count,
branch, cull, order and camera edges, with what the CPU oracle (oracle/ref_geom.cpp: find_fundamental_ransac, optimize_in_frame,
ref_undistort_points, ref_project_points) says about each of them.  No GPU is needed here: tests/test_geom_calls_inputs.py builds every
input and proves on the oracle that it reaches the edge it is there for; tests/test_gpu_geom_calls.py compares the kernels, bit for bit,
against what is built here.  Every expected value is computed once (functools caches) and shared."""
import functools
import os
import tempfile

import numpy as np

import _geom as G
import _oracle as O

K4 = np.array([384.0, 385.0, 320.0, 240.0])
K4_B = np.array([458.654, 457.296, 367.215, 248.375])          # the second camera of the per-set-camera launches
GARBAGE = np.float32(1.0e6)                                   # rows at and beyond a set's count: never read
F_CAP, F_THR, F_CONF = 1024, 5.0, 0.99                        # NMAX; lkorb_tracking.cpp:134's arguments
F_COUNTS = (0, 6, 7, 8, 14, 15, 16, 64, 65, 240, 1024)
LM_CAP = 512                                                  # PL_EMAX
LM_COUNTS = (9, 10, 31, 32, 33, 256, 257, 512)                # the 10-edge rule, the 32-edge chunk of a sum, PL_T = 256 threads, the capacity
PT_COUNTS = (0, 1, 63, 64, 65)
PT_CAP = 80


# ---- F-matrix RANSAC ---------------------------------------------------------------------------------------------------------------------
def two_view(seed, n, outl=0.2, noise=0.3):
    """n correspondences of a scene seen by two cameras a small motion apart, round(outl n) of them with the second pixel anywhere"""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2, 8, n)], 1)
    R = G.rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 0.2, 3)
    m1 = G.project(np.eye(3), np.zeros(3), P, K4) + rng.normal(0, noise, (n, 2))
    m2 = G.project(R, t, P, K4) + rng.normal(0, noise, (n, 2))
    nb = int(round(outl * n))
    bad = rng.permutation(n)[:nb]
    m2[bad] = np.stack([rng.uniform(0, 640, nb), rng.uniform(0, 480, nb)], 1)
    return m1.astype(np.float32), m2.astype(np.float32)


def pure_outliers(seed, n, scale=1.0):
    """both pixels of every pair drawn anywhere in an image `scale` times 640 x 480"""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1) * scale
    b = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1) * scale
    return a.astype(np.float32), b.astype(np.float32)


# At image scale seven random pairs always carry a model that fits them (7 inliers > 6), so "pure outliers" alone never gives the empty
# mask.  At this scale the residuals of a model on its OWN seven points -- a relative 1e-13 or so of coordinates around 1e22, squared --
# are far above 25 px^2: every model scores 0, none beats the 6-inlier floor of RANSACPointSetRegistrator::run.  checkSubset compares
# relative to the coordinates' size, so the subsets drawn are those of the image-scale set.
NO_MODEL_SCALE = 1.0e20


def collinear(n, seed=3):
    """every point of either image on one line: checkSubset refuses every subset, getSubset gives up after its 10000 attempts (RANSAC,
    n >= 15)"""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.permutation(300)[:n]).astype(np.float32)  # (whole numbers: y = 2 x + 20 is exact in float, the cross products are 0)
    m1 = np.stack([s, 2 * s + 20], 1)
    m2 = np.stack([s + 4, 2 * s + 31], 1)
    return m1.astype(np.float32), m2.astype(np.float32)


def duplicates(n, of=None):
    """two-view data in which the pairs listed in `of` (default: all) are exact copies of pair 0"""
    m1, m2 = two_view(11, n)
    of = range(n) if of is None else of
    for i in of:
        m1[i], m2[i] = m1[0], m2[0]
    return m1, m2


@functools.lru_cache(None)
def f_sets():
    """name -> (m1 [n,2], m2 [n,2]): the sets of the F-RANSAC launches, ragged"""
    sets = {}
    for n in F_COUNTS:
        sets["clean_%d" % n] = two_view(100 + n, n)
    sets["lmeds_9"] = two_view(31, 9, outl=0.0)
    sets["lmeds_11_outl"] = two_view(32, 11, outl=0.3)
    sets["outliers_40"] = pure_outliers(5, 40)
    sets["outliers_300"] = pure_outliers(6, 300)
    sets["no_model_40"] = pure_outliers(5, 40, NO_MODEL_SCALE)
    sets["collinear_30"] = collinear(30)
    sets["collinear_12"] = collinear(12)                      # (the LMedS branch's getSubset: 1000 attempts)
    sets["dup_all_30"] = duplicates(30)
    sets["dup_half_60"] = duplicates(60, range(0, 60, 2))
    sets["dup_all_10"] = duplicates(10)
    rng = np.random.default_rng(9)
    k = 0
    while len(sets) < 65:                                     # ragged counts up to 65 sets: 65 workgroups, more than one per XCD
        n = int(rng.integers(15, 500))
        sets["ragged%02d_%d" % (k, n)] = two_view(500 + k, n, outl=float(rng.uniform(0.0, 0.6)))
        k += 1
    return sets


@functools.lru_cache(None)
def f_expected(name, thr=F_THR, conf=F_CONF):
    """the oracle's (inliers, mask) of a set"""
    m1, m2 = f_sets()[name]
    if len(m1) == 0:
        return 0, np.zeros(0, np.uint8)
    n, mask = O.find_fundamental_ransac(m1, m2, thr, conf)
    return int(n), mask


def f_rows(names, cap=F_CAP):
    """(m1 [s,cap,2], m2 [s,cap,2], count [s]) of the named sets, garbage beyond each count"""
    m1 = np.full((len(names), cap, 2), GARBAGE, np.float32)
    m2 = np.full((len(names), cap, 2), GARBAGE, np.float32)
    cnt = np.zeros(len(names), np.int32)
    for k, nm in enumerate(names):
        a, b = f_sets()[nm]
        m1[k, :len(a)], m2[k, :len(a)], cnt[k] = a, b, len(a)
    return m1, m2, cnt


# ---- pose-only LM ------------------------------------------------------------------------------------------------------------------------
class LmSet:
    """one set of flvis_hip_optimize_in_frame: the edges in input order, the pose to start from, the camera"""

    def __init__(self, p3, z, ids, pose0, K):
        self.p3, self.z = np.ascontiguousarray(p3, np.float64), np.ascontiguousarray(z, np.float64)
        self.ids, self.pose0, self.K = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(pose0, np.float64), np.asarray(K, np.float64)
        self.n = len(self.p3)

    @functools.cached_property
    def expected(self):
        """the oracle's (ok, pose7); the pose of an ok = 0 set is the input's"""
        ok, pose = O.optimize_in_frame(self.pose0, self.p3, self.z, self.ids, self.K)
        return ok, pose

    def swapped(self, i, j):
        o = np.arange(self.n)
        o[[i, j]] = o[[j, i]]
        return LmSet(self.p3[o], self.z[o], self.ids[o], self.pose0, self.K)


def lm_scene(seed, n, n_out=0, K=K4, noise=0.3, out_px=40.0):
    """n landmarks seen from a pose, the first n_out observations `out_px` pixels off; the start pose a small step from the true one.
    -> (world points, undistorted pixels, true pose7, start pose7)"""
    rng = np.random.default_rng(seed)
    R = G.rodrigues(rng.normal(0, 0.2, 3))
    t = rng.normal(0, 0.5, 3)
    Pc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 8, n)], 1)
    Pw = (Pc - t) @ R                                          # X_c = R X_w + t
    z = G.project(R, t, Pw, K) + rng.normal(0, noise, (n, 2))
    ang = rng.uniform(0, 2 * np.pi, n_out)
    z[:n_out] += out_px * np.stack([np.cos(ang), np.sin(ang)], 1)
    R0 = G.rodrigues(rng.normal(0, 0.01, 3)) @ R
    return Pw, z, G.pose7(R, t), G.pose7(R0, t + rng.normal(0, 0.02, 3))


def chi2_at(pose7, s):
    """the squared reprojection error of every edge of LmSet s at a pose (numpy; what the cull compares with 3)"""
    R, t = G.pose7_to_Rt(pose7)
    d = G.project(R, t, s.p3, s.K) - s.z
    return (d * d).sum(1)


def lm_outliers(n):
    """how many of a count set's observations are 40 px off (none in the smallest sets: they must keep their 10 edges)"""
    return (n - 10) // 8 if n >= 10 else 0


@functools.lru_cache(None)
def lm_sets():
    sets = {}
    for n in LM_COUNTS:
        Pw, z, _, p0 = lm_scene(200 + n, n, n_out=lm_outliers(n))
        sets["count_%d" % n] = LmSet(Pw, z, np.arange(n) * 3 + 7, p0, K4)
    # the cull: 14 edges, of which 5 / 4 are 40 px off -- 9 / 10 stay alive
    for alive in (9, 10):
        Pw, z, _, p0 = lm_scene(77, 14, n_out=14 - alive)
        sets["cull_%d" % alive] = LmSet(Pw, z, np.arange(14), p0, K4)
    Pw, z, _, p0 = lm_scene(41, 40, n_out=4)
    sets["ids_descending"] = LmSet(Pw, z, 1000 - np.arange(40), p0, K4)
    sets["ids_negative"] = LmSet(Pw, z, np.random.default_rng(2).permutation(40) - 20 - (1 << 40), p0, K4)
    sets["ids_duplicate"] = LmSet(Pw, z, np.arange(40) // 2, p0, K4)       # pairs of equal ids: input order decides
    sets["ids_all_equal"] = LmSet(Pw, z, np.zeros(40, np.int64), p0, K4)
    sets["ids_duplicate_swapped"] = swap_pairs(sets["ids_duplicate"])
    for k, K in enumerate((K4, K4_B)):                                     # two cameras
        Pw, z, _, p0 = lm_scene(300 + k, 60, n_out=6, K=K)
        sets["camera_%d" % k] = LmSet(Pw, z, np.arange(60), p0, K)
    return sets


def swap_pairs(s):
    """every pair (2k, 2k + 1) of edges exchanged: with ids k // 2 the same multiset of edges under equal ids, in another input order"""
    o = np.arange(s.n).reshape(-1, 2)[:, ::-1].reshape(-1)
    return LmSet(s.p3[o], s.z[o], s.ids[o], s.pose0, s.K)


def lm_rows(names, cap=LM_CAP):
    """(lm3d [s,cap,3], lm2d [s,cap,2], ids [s,cap], count [s], pose7 [s,7], K [s,4]) of the named sets, garbage beyond each count"""
    S = lm_sets()
    p3 = np.full((len(names), cap, 3), float(GARBAGE))
    z = np.full((len(names), cap, 2), float(GARBAGE))
    ids = np.full((len(names), cap), -5, np.int64)
    cnt = np.zeros(len(names), np.int32)
    pose = np.zeros((len(names), 7))
    K = np.zeros((len(names), 4))
    for k, nm in enumerate(names):
        s = S[nm]
        p3[k, :s.n], z[k, :s.n], ids[k, :s.n], cnt[k], pose[k], K[k] = s.p3, s.z, s.ids, s.n, s.pose0, s.K
    return p3, z, ids, cnt, pose, K


# ---- undistortPoints / projectPoints ------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def rigs():
    """name -> (K4, D4, R [3,3], P [3,4]): a pinhole camera without distortion, and camera 0 of the EuRoC-like rig of flvis_amd.synth with
    the rectification flvis_config_load derives for it"""
    import flvis_amd
    from flvis_amd import synth
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "euroc.yaml")
        open(p, "w").write(synth.EUROC_LIKE_YAML)
        cfg = flvis_amd.load_config(p)
    e = (np.array(cfg.cam0_intrinsics), np.array(cfg.cam0_distortion), np.array(cfg.R0).reshape(3, 3), np.array(cfg.P0).reshape(3, 4))
    assert e[1][0] != 0 and e[3][0, 0] != 0 and not np.array_equal(e[2], np.eye(3))
    P = np.array([[K4[0], 0, K4[2], 0], [0, K4[1], K4[3], 0], [0, 0, 1, 0]])
    return {"pinhole": (K4, np.zeros(4), np.eye(3), P), "euroc": e}


RIGS = ("pinhole", "euroc")


@functools.lru_cache(None)
def pt_sets():
    """(rig, count) -> dict(src [n,2] f32, p3d [n,3] f32, pose7): pixels all over (and beyond) the image, and world points of which the
    first few lie on and behind the camera's plane z = 0 or overflow the float pixel"""
    out = {}
    for r, rig in enumerate(RIGS):
        for n in PT_COUNTS:
            rng = np.random.default_rng(1000 * r + n)
            src = np.stack([rng.uniform(-50, 800, n), rng.uniform(-50, 530, n)], 1).astype(np.float32)
            pose = G.pose7(G.rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3))
            R, t = G.pose7_to_Rt(pose)
            Pc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 8, n)], 1)
            p3 = ((Pc - t) @ R).astype(np.float32)
            if n >= 63:
                pose = np.array([0, 0, 0, 0, 0, 0, 1.0])      # the identity: the camera-frame z is the float itself
                p3 = Pc.astype(np.float32)
                p3[0] = (1.0, 2.0, 0.0)                        # z == 0: 1 / z reads as 1
                p3[1] = (1.0, -2.0, -3.0)                      # behind the camera
                p3[2] = (0.0, 0.0, 0.0)
                p3[3] = (3.0e38, -3.0e38, 1.0e-30)             # overflows the float pixel: +inf / -inf
                src[0] = (np.inf, 3.0)                         # undistortPoints of a non-finite pixel
                src[1] = (np.nan, 100.0)
                src[2] = (3.0e38, -3.0e38)
            out[(rig, n)] = dict(src=src, p3d=p3, pose7=pose)
    return out


@functools.lru_cache(None)
def pt_expected(rig, n):
    """the oracle's (undistorted [n,2], projected [n,2]) float32 of a set"""
    s = pt_sets()[(rig, n)]
    K, D, R, P = rigs()[rig]
    if n == 0:
        return np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    with np.errstate(all="ignore"):
        return O.undistort_points(s["src"], K, D, R, P), O.project_points(s["p3d"], s["pose7"], K, D)


def bits(a):
    """float32 values as their bit patterns: the comparison of the tests (NaN == NaN of the same bits, -0 != +0)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
