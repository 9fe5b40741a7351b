"""Inputs that drive the PnP RANSAC (pnp_ransac_core of flvis_amd/csrc/track_kernels.hip, through k_pnp_ransac_sets) to its count, batch
and stop-rule edges in both branches, with what the CPU oracle (oracle/ref_geom.cpp: solve_pnp_ransac, pinned to OpenCV's solvers by
tests/test_oracle_cv_solvers.py) says about each of them.  No GPU is needed here: tests/test_pnp_edges_inputs.py builds every recipe and
pins its figures with the oracle alone, tests/test_gpu_pnp_edges.py compares the kernel against what is built here.

The two branches:
  P3P        (flvis_hip_pnp_ransac: the loop closing's check, 100 iterations, 2.0 px, 0.99)  4-point subsets; the first 16 hypotheses from a
             table, then batches of 64 drawn serially; scored in sub-batches [0,16), [16,32), ...; final solve: EPnP on the inliers
  iterative  (flvis_hip_debug_pnp_ransac_iterative: the tracker's, 100 iterations, 3.0 px, 0.99)  5-point subsets; the first 8 from a table,
             then batches of 8; scored batch by batch; final solve: Gauss-Newton on the inliers; a set without a model gets its guess back
In either, one thread replays RANSACUpdateNumIters over a scored sub-batch in order: a better hypothesis of the same sub-batch that lies
behind the shrunken limit has been scored and must be ignored.

The subsets of a run depend on the number of correspondences alone (every run starts from cv::RNG((uint64)-1)), so the index of the
winning hypothesis is exact: the smallest k for which the oracle, limited to k + 1 iterations, returns the final count and mask.
A recipe asserts the class it is there for when it is built (Case.check): a generator that drifts fails here, on the CPU."""
import functools
import zlib

import numpy as np

import _geom as G
import _oracle as O

K4 = np.array([384.0, 385.0, 320.0, 240.0])
P3P, ITER = "p3p", "iterative"
BRANCHES = (P3P, ITER)
MODEL_POINTS = {P3P: 4, ITER: 5}
DEFAULT = {P3P: (100, 2.0, 0.99), ITER: (100, 3.0, 0.99)}     # isLoopClosureKF's and LKORBTracking::tracking's solvePnPRansac
SUB_BATCH = {P3P: 16, ITER: 8}                                # hypotheses scored before the stop rule is replayed
CAP = 1024                                                    # PNP_MAXN: the launches' buffer, but for the clamp recipes'
CLAMP_CAP = 32
GARBAGE = 1.0e6                                               # rows at and beyond a set's count
COUNTS = tuple(range(25)) + (63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024)
LIMITS = {P3P: (1, 15, 16, 17, 79, 80, 81, 100), ITER: (1, 7, 8, 9, 16, 17, 100)}
CONFS = (0.5, 0.99, 0.999999)
REPROJS = (0.5, 2.0, 3.0, 50.0)
# found by seed search over scene(seed, n, outliers): where the winner's index of the default run lies
LIMIT_SETS = {P3P: dict(n=60, outl=0.5, seeds={"w15": 44, "w16": 21, "w17_79": 2, "w80": 80}),
              ITER: dict(n=50, outl=0.6, seeds={"w7": 419, "w8": 92, "w16": 1})}
LIMIT_WANT = {(P3P, "w15"): lambda w: w == 15, (P3P, "w16"): lambda w: w == 16, (P3P, "w17_79"): lambda w: 17 <= w <= 79,
              (P3P, "w80"): lambda w: w >= 80, (ITER, "w7"): lambda w: w == 7, (ITER, "w8"): lambda w: w == 8, (ITER, "w16"): lambda w: w >= 16}
# ... and where confidence 0.5 stops the search in front of a strictly better hypothesis of the same scored sub-batch
CUT_SETS = {P3P: dict(n=65, outl=0.5, seeds=(4, 23)), ITER: dict(n=65, outl=0.5, seeds=(63, 166))}


def sub_batch(branch, k):
    """P3P: [0,16) of the tabulated batch, then groups of 16 from index 16; iterative: groups of 8"""
    return k // SUB_BATCH[branch]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def observe(P, seed, noise=0.4):
    """pixels of the world points P from a camera drawn from `seed`, with pixel noise; float32 as the kernels take them"""
    rng = np.random.default_rng(seed)
    R = G.rodrigues(rng.normal(0, 0.3, 3))
    t = rng.normal(0, 0.5, 3)
    uv = G.project(R, t, P, K4) + rng.normal(0, noise, (len(P), 2))
    return P.astype(np.float32), uv.astype(np.float32)


def scene(seed, n, outl, noise=0.4):
    """n points in front of a camera, round(outl n) of them with a pixel drawn anywhere in the image"""
    rng = np.random.default_rng(seed)
    R = G.rodrigues(rng.normal(0, 0.3, 3))
    t = rng.normal(0, 0.5, 3)
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2, 8, n)], 1)
    uv = G.project(R, t, P, K4) + rng.normal(0, noise, (n, 2))
    nb = int(round(outl * n))
    bad = rng.permutation(n)[:nb]
    uv[bad] = np.stack([rng.uniform(0, 640, nb), rng.uniform(0, 480, nb)], 1)
    return P.astype(np.float32), uv.astype(np.float32)


def _flat(kind, n=60, seed=6):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-3, 3, n)
    if kind == "planar":                                       # the plane z = 5 of the world frame
        return np.stack([s, rng.uniform(-2, 2, n), np.full(n, 5.0)], 1)
    return np.stack([s, 0.5 * s, np.full(n, 5.0)], 1)          # collinear, in that plane


def guess_for(name):
    """the pose an iterative set falls back on: w > 0 (in fact > 0.9: the quaternion survives the kernel's matrix round trip to a few
    roundings) and not the identity, so that a returned guess cannot be mistaken for one"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    g = G.pose7(G.rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3))
    assert g[6] > 0.9 and np.abs(g[3:6]).max() > 1e-3 and abs(np.linalg.norm(g[3:7]) - 1) < 1e-15
    return g


# ---- recipes ----------------------------------------------------------------------------------------------------------------------------
class Recipe:
    def __init__(self, cls, branch, build, iterations=None, reproj=None, conf=None, cap=CAP, count=None, fill=None, tag=None):
        d = DEFAULT[branch]
        self.cls, self.branch, self.build, self.cap, self.count, self.fill, self.tag = cls, branch, build, cap, count, fill, tag
        self.iterations = d[0] if iterations is None else iterations
        self.reproj = d[1] if reproj is None else reproj
        self.conf = d[2] if conf is None else conf

    @property
    def key(self):
        return (self.branch, self.iterations, self.reproj, self.conf, self.cap)


RECIPES = {}


def _empty():
    return np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)


def _exact(branch, outlier):
    def build():
        P, uv = scene(77, MODEL_POINTS[branch], 0.0, noise=0.1)
        if outlier:
            uv[-1] += np.float32(200.0)
        return P, uv
    return build


def _dup(seed):
    def build():
        P, uv = scene(seed, 60, 0.2)
        return np.concatenate([P, P]), np.concatenate([uv, uv])
    return build


def _negated():
    P, uv = scene(13, 60, 0.2)
    return -P, uv


def _ident3d():
    P, uv = scene(3, 60, 0.2)
    return np.repeat(P[:1], 60, 0), uv


def _ident2d():
    P, uv = scene(3, 60, 0.2)
    return P, np.repeat(uv[:1], 60, 0)


for _b in BRANCHES:
    _mp = MODEL_POINTS[_b]
    # count: every count around the model size, the wave (64), the workgroup (512) and the capacity (1024); 20 % outliers, 0.4 px
    for _n in COUNTS:
        RECIPES["count_%s_%d" % (_b, _n)] = Recipe("count", _b, functools.partial(scene, 1000 + _n, _n, 0.2) if _n else _empty)
    RECIPES["count_%s_exact_clean" % _b] = Recipe("count", _b, _exact(_b, False), tag="exact_clean")
    RECIPES["count_%s_exact_outlier" % _b] = Recipe("count", _b, _exact(_b, True), tag="exact_outlier")
    # ... and a count beyond / below the buffer: clamped to the capacity (the oracle sees 32 rows) / to zero
    RECIPES["clamp_%s_2000" % _b] = Recipe("count", _b, functools.partial(scene, 2000, CLAMP_CAP, 0.2), cap=CLAMP_CAP, count=2000)
    RECIPES["clamp_%s_-5" % _b] = Recipe("count", _b, _empty, cap=CLAMP_CAP, count=-5, fill=functools.partial(scene, 2001, CLAMP_CAP, 0.2))
    # limit: one set under iteration limits at and around the batch edges
    _s = LIMIT_SETS[_b]
    for _tag, _seed in _s["seeds"].items():
        for _L in LIMITS[_b]:
            RECIPES["limit_%s_%s_%d" % (_b, _tag, _L)] = Recipe("limit", _b, functools.partial(scene, _seed, _s["n"], _s["outl"]), iterations=_L, tag=_tag)
    # cut: the stop rule inside a scored sub-batch
    _s = CUT_SETS[_b]
    for _seed in _s["seeds"]:
        for _c in CONFS:
            RECIPES["cut_%s_%d_%g" % (_b, _seed, _c)] = Recipe("cut", _b, functools.partial(scene, _seed, _s["n"], _s["outl"]), conf=_c, tag=_seed)
    # threshold
    for _r in REPROJS:
        RECIPES["threshold_%s_%g" % (_b, _r)] = Recipe("threshold", _b, functools.partial(scene, 7, 120, 0.1), reproj=_r)
    # no model
    RECIPES["nomodel_%s_outliers" % _b] = Recipe("no model", _b, functools.partial(scene, 0, 60, 1.0))
    RECIPES["nomodel_%s_ident3d" % _b] = Recipe("no model", _b, _ident3d)
    # degenerate but solvable
    RECIPES["degenerate_%s_negated" % _b] = Recipe("degenerate", _b, _negated)
    RECIPES["degenerate_%s_duplicated" % _b] = Recipe("degenerate", _b, _dup(3))
RECIPES["nomodel_p3p_ident2d"] = Recipe("no model", P3P, _ident2d)   # (iterative: the oracle's pose has magnitude 1e14 -- no meaningful bits)
for _k in ("planar", "collinear"):                                  # a model under P3P, every hypothesis fails under iterative
    RECIPES["degenerate_p3p_%s" % _k] = Recipe("degenerate", P3P, functools.partial(observe, _flat(_k), 11))
    RECIPES["nomodel_iterative_%s" % _k] = Recipe("no model", ITER, functools.partial(observe, _flat(_k), 11))

CLASSES = ("count", "limit", "cut", "threshold", "no model", "degenerate")
GROUPS = {}                      # (branch, iterations, reproj, conf, cap) -> names: the sets of one launch
for _name, _r in RECIPES.items():
    GROUPS.setdefault(_r.key, []).append(_name)
DEFAULT_GROUP = {b: (b,) + DEFAULT[b] + (CAP,) for b in BRANCHES}


def recipe(name):
    """-> (P float32 [n,3], uv float32 [n,2], branch, iterations, reproj, conf, guess7)"""
    r = RECIPES[name]
    P, uv = r.build()
    P, uv = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(uv, np.float32)
    return P, uv, r.branch, r.iterations, r.reproj, r.conf, guess_for(name) if r.branch == ITER else None


def oracle(P, uv, branch, iterations, reproj, conf, guess7):
    """-> (inliers, pose7, mask); no model: 0, the guess untouched (iterative) or the identity (P3P), a zero mask"""
    return O.solve_pnp_ransac(P, uv, K4, iterative=branch == ITER, pose7=guess7, iterations=iterations, reproj=reproj, conf=conf)


@functools.lru_cache(maxsize=None)
def _winner(name, iterations, conf):
    r = RECIPES[name]
    P, uv, branch, _, reproj, _, g = recipe(name)
    n_want, _, mask = oracle(P, uv, branch, iterations, reproj, conf, g)
    if n_want == 0:
        return -1, 0
    for k in range(iterations):
        n, _, m = oracle(P, uv, branch, k + 1, reproj, conf, g)
        if n == n_want and np.array_equal(m, mask):
            return k, n_want
    raise AssertionError("%s: no iteration limit reproduces the full run" % name)


class Case:
    def __init__(self, name):
        self.name, self.r = name, RECIPES[name]
        self.P, self.uv, self.branch, self.iterations, self.reproj, self.conf, self.guess = recipe(name)
        self.n = len(self.P)
        self.count = self.n if self.r.count is None else self.r.count       # what the kernel is told
        self.cap = self.r.cap
        self.inliers, self.pose, self.mask = oracle(self.P, self.uv, self.branch, self.iterations, self.reproj, self.conf, self.guess)
        # the keeping rule: no model, or a pose whose bits mean something
        assert self.inliers == 0 or np.linalg.norm(self.pose[:3]) < 1e3, name
        if self.inliers == 0:
            assert not self.mask.any() and np.array_equal(self.pose, self.guess if self.branch == ITER else [0, 0, 0, 0, 0, 0, 1]), name

    @property
    def winner(self):
        return _winner(self.name, self.iterations, self.conf)[0]

    def rows(self):
        """the set's rows of a launch buffer: the correspondences, then finite garbage up to the capacity"""
        p3 = np.full((self.cap, 3), GARBAGE, np.float32)
        p2 = np.full((self.cap, 2), GARBAGE, np.float32)
        if self.r.fill is not None:                            # (count < 0: what the kernel must not read is a solvable scene)
            fp, fu = self.r.fill()
            p3[:len(fp)], p2[:len(fu)] = fp, fu
        p3[:self.n], p2[:self.n] = self.P, self.uv
        return p3, p2

    def pinned(self):
        return (self.n, int(self.inliers), self.winner, self.r.cls)

    def check(self):
        """the class conditions (CPU, oracle only)"""
        r, mp, name = self.r, MODEL_POINTS[self.branch], self.name
        if r.cls == "count":
            if self.n < mp:
                assert self.inliers == 0, name
            if self.n >= 8:
                assert self.inliers > 0, name
            if r.tag == "exact_clean":
                assert self.n == mp and self.inliers == mp and self.winner == 0, name
            if r.tag == "exact_outlier":
                assert self.n == mp and self.inliers < mp, name
            if r.count is not None:
                assert self.n == (CLAMP_CAP if r.count > 0 else 0) and r.cap == CLAMP_CAP, name
        elif r.cls == "limit":
            w, full = _winner(name, 100, self.conf)            # of the default run of the same set
            assert LIMIT_WANT[self.branch, r.tag](w), (name, w)
            if self.iterations > w:
                assert self.inliers == full and self.winner == w, name
            else:
                assert self.inliers < full and self.winner < self.iterations, name
        elif r.cls == "cut":
            (wa, a), (wb, b) = _winner(name, 100, CONFS[0]), _winner(name, 100, CONFS[-1])
            assert 0 < a < b and wa < wb and sub_batch(self.branch, wa) == sub_batch(self.branch, wb), (name, wa, a, wb, b)
        elif r.cls == "threshold":
            if self.reproj == REPROJS[-1]:                     # nearly all inliers: the first such model, in the tabulated batch, ends the search
                assert self.inliers >= 0.9 * self.n, name
                w = self.winner
                assert w < SUB_BATCH[self.branch], name
                assert w == 0 or oracle(self.P, self.uv, self.branch, w, self.reproj, self.conf, self.guess)[0] < 0.5 * self.n, name
            else:
                assert 0 < self.inliers < 0.95 * self.n, name
        elif r.cls == "no model":
            assert self.inliers == 0 and self.n >= mp, name
        elif r.cls == "degenerate":
            assert self.inliers > 0, name
        return self


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name).check()
