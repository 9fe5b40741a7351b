"""Inputs that drive ORB extraction (flvis_hip_orb_detect_and_compute) to its tie, capacity and size edges, with what the CPU oracle
(oracle/ref_orb.cpp) says about each of them.  No GPU is needed here: tests/test_orb_edges_inputs.py checks every recipe with the
oracle alone, tests/test_gpu_orb_edges.py compares the kernels against what is built here.

A "dot grid" is a flat image of value FLAT with single pixels of value DOT every p pixels.  Every dot is an isolated FAST corner with
the same score and, the surroundings being the same, the same Harris response (an integer sum): one exact tie class.  OpenCV's
retainBest keeps everything >= the n-th best, so a tie class that straddles a level's budget is kept whole.

A Case asserts its own counts when it is built (level count against the level's budget and the kernels' per-level capacity, total
against the caller's capacity): a recipe that drifts to the wrong side fails there instead of testing nothing."""
import functools

import numpy as np

import _oracle as O
import _synth as S

FLAT, DOT = 40, 210
EDGE = 31                   # edgeThreshold: keypoints live in [EDGE, W - EDGE) x [EDGE, H - EDGE) of their level
CAND_CAP = 8192             # ORB_CAND_CAP of orb_kernels.hip: FAST survivors per (image, level) held in LDS
CLOSER = dict(nfeatures=1000, nlevels=8, sf=1.2, fast_thr=20)      # the loop closer's cv::ORB::create(1000, 1.2f, 8, ..., 20)
CLOSER_CAP = 1024           # LCC_CAP of loop_closer.hip
SMALL = dict(nfeatures=100, nlevels=5, sf=1.2, fast_thr=7)


def lvl_cap(nfeatures=1000, nlevels=8, sf=1.2, **_):
    """the kernels' per-level capacity, as flvis_hip_orb_detect_and_compute computes it: the largest level budget, a quarter of it again
    and 64 -- room for ties at the cut"""
    m = int(O.orb_features_per_level(nfeatures, nlevels, sf).max())
    return m + m // 4 + 64


def gpu_kwargs(prm):
    """oracle parameter names -> flvis_amd.Context.orb_detect_and_compute's"""
    return dict(nfeatures=prm["nfeatures"], nlevels=prm["nlevels"], scale_factor=prm["sf"], fast_threshold=prm["fast_thr"])


def flat(h, w):
    return np.full((h, w), FLAT, np.uint8)


def dot_rect(h, w, p, ny, nx, y0, x0):
    """ny x nx dots every p pixels, the first at (x0, y0)"""
    img = flat(h, w)
    img[y0:y0 + ny * p:p, x0:x0 + nx * p:p] = DOT
    return img


def dot_field(h, w, p):
    """dots every p pixels over the whole image, the first at (p // 2, p // 2)"""
    img = flat(h, w)
    img[p // 2::p, p // 2::p] = DOT
    return img


def corners_with_dots(ny, h=480, w=640, seed=80, nx=20, p=12, y0=40, x0=40, rim=6):
    """S.corner_img with the patch under an ny x nx dot grid (and a rim around it) flattened, and the grid pasted on it"""
    img = S.corner_img(h, w, seed).copy()
    img[y0 - rim:y0 + (ny - 1) * p + 1 + rim, x0 - rim:x0 + (nx - 1) * p + 1 + rim] = FLAT
    img[y0:y0 + ny * p:p, x0:x0 + nx * p:p] = DOT
    return img


def fast_survivors(level_img, fast_thr, nfeat):
    """how many corners of one level come out of retainBest(2 * nfeat) on the FAST score (>= the (2n)-th best stay): what the select
    kernel has to hold in LDS.  -> (count, number of distinct scores among them)"""
    h, w = level_img.shape
    if w <= 2 * EDGE or h <= 2 * EDGE:
        return 0, 0
    kp = O.fast_detect(level_img, fast_thr)
    kp = kp[(kp[:, 0] >= EDGE) & (kp[:, 0] < w - EDGE) & (kp[:, 1] >= EDGE) & (kp[:, 1] < h - EDGE)]
    sc = np.sort(kp[:, 2])[::-1]
    if len(sc) > 2 * nfeat:
        sc = sc[sc >= sc[2 * nfeat - 1]]
    return len(sc), len(np.unique(sc))


class Case:
    """one input with the oracle's untruncated answer.  kps [n,6] / desc [n,32] level-major, raster within a level; counts[l];
    budget[l]; lvl_cap; pyr[l] the oracle's level images"""

    def __init__(self, name, img, prm):
        self.name, self.img, self.prm = name, np.ascontiguousarray(img), dict(prm)
        self.kps, self.desc, self.pyr, _ = O.orb_detect_and_compute(self.img, cap=32768, want_pyr=True, **prm)
        self.octave = self.kps[:, 5].astype(int)
        assert np.all(np.diff(self.octave) >= 0), name
        self.budget = O.orb_features_per_level(prm["nfeatures"], prm["nlevels"], prm["sf"])
        self.counts = np.bincount(self.octave, minlength=prm["nlevels"])
        self.lvl_cap = lvl_cap(**prm)
        self.total = len(self.kps)

    def level(self, l):
        sel = self.octave == l
        return self.kps[sel], self.desc[sel]

    def survivors(self, l):
        return fast_survivors(self.pyr[l], self.prm["fast_thr"], int(self.budget[l]))

    def tie_class_at_cut(self, l):
        """size of the response class that holds the level's weakest kept keypoint: > 1 and counts[l] > budget[l] means a tie class
        straddles the Harris cut"""
        r = self.level(l)[0][:, 4]
        return int((r == r.min()).sum()) if len(r) else 0

    def expected(self, cap):
        """what the kernels return at caller capacity `cap`: every level's list cut to its first lvl_cap entries (the Harris threshold
        is still the one over all candidates), concatenated, cut to its first `cap` rows.  -> (kps, desc, overflowed)"""
        ks, ds = [], []
        for l in range(self.prm["nlevels"]):
            k, d = self.level(l)
            ks.append(k[:self.lvl_cap]), ds.append(d[:self.lvl_cap])
        k, d = np.concatenate(ks), np.concatenate(ds)
        ovf = bool((self.counts > self.lvl_cap).any() or len(k) > cap)
        return k[:cap], d[:cap], ovf

    # ---- the properties a recipe is there for
    def check(self, ties_at=None, level_over=None, level_under=None, total_over=None, total_under=None, cand_over=None, cand_under=None):
        n = self.name
        if ties_at is not None:
            l = ties_at
            assert self.counts[l] > self.budget[l], (n, "level %d: %d keypoints do not exceed the budget %d" % (l, self.counts[l], self.budget[l]))
            assert self.tie_class_at_cut(l) > self.counts[l] - self.budget[l], (n, "no tie class across the cut of level %d" % l)
        if level_over is not None:
            assert self.counts[level_over] > self.lvl_cap, (n, self.counts[level_over], self.lvl_cap)
        if level_under is not None:
            assert self.counts.max() <= self.lvl_cap, (n, self.counts, self.lvl_cap)
        if total_over is not None:
            assert self.expected(1 << 20)[0].shape[0] > total_over, (n, self.total, total_over)
        if total_under is not None:
            assert self.total <= total_under, (n, self.total, total_under)
        if cand_over is not None:
            assert self.survivors(cand_over)[0] > CAND_CAP, (n, self.survivors(cand_over))
        if cand_under is not None:
            assert all(self.survivors(l)[0] <= CAND_CAP for l in range(self.prm["nlevels"])), n
        return self


# ---- the recipes.  Each is built once per process; nothing that holds one changes it ------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    return RECIPES[name]()


def _dots(rows):
    """rows x 20 dots, p = 12, from (60, 60) on 480 x 640: level 0 holds them all"""
    return dot_rect(480, 640, 12, rows, 20, 60, 60)


RECIPES = {
    # ties without overflow: the tie class straddles the Harris cut of level 0 (budget 217), every level stays below lvl_cap (335)
    "dots14": lambda: Case("dots14", _dots(14), CLOSER).check(ties_at=0, level_under=True, total_under=4096, cand_under=True),
    "dots16": lambda: Case("dots16", _dots(16), CLOSER).check(ties_at=0, level_under=True, total_under=4096, cand_under=True),
    "small_dots": lambda: Case("small_dots", dot_field(100, 131, 6), SMALL).check(ties_at=0, level_under=True, total_under=4096,
                                                                                   cand_under=True),
    # level overflow: more tied keypoints than lvl_cap, candidates still within CAND_CAP
    "dots17": lambda: Case("dots17", _dots(17), CLOSER).check(ties_at=0, level_over=0, cand_under=True),
    "field7": lambda: Case("field7", dot_field(480, 640, 7), CLOSER).check(ties_at=0, level_over=0, cand_under=True),
    "paste12": lambda: Case("paste12", corners_with_dots(12), CLOSER).check(ties_at=0, level_over=0, total_over=CLOSER_CAP, cand_under=True),
    # candidate overflow: more FAST survivors than CAND_CAP, all of one score
    "field4": lambda: Case("field4", dot_field(480, 640, 4), CLOSER).check(cand_over=0, level_over=0),
    # the caller's capacity alone: the loop closer's own call (cap 1024) drops the tail of the list
    "paste8": lambda: Case("paste8", corners_with_dots(8), CLOSER).check(ties_at=0, level_under=True, total_over=CLOSER_CAP, cand_under=True),
    "paste10": lambda: Case("paste10", corners_with_dots(10), CLOSER).check(ties_at=0, level_under=True, total_over=CLOSER_CAP,
                                                                            cand_under=True),
    "corners": lambda: Case("corners", S.corner_img(480, 640, 80), CLOSER).check(level_under=True, total_over=512, total_under=CLOSER_CAP,
                                                                                 cand_under=True),
    "corners81": lambda: Case("corners81", S.corner_img(480, 640, 81), CLOSER).check(level_under=True, total_under=CLOSER_CAP, cand_under=True),
    "flat": lambda: Case("flat", flat(480, 640), CLOSER).check(total_under=0),
    # shapes: KITTI's frame (level-0 pitch 1241: no multiple of 16, of the 64-wide tiles or of anything else), and an image whose
    # upper levels have no border box at all (W <= 62 or H <= 62)
    "kitti": lambda: Case("kitti", S.corner_img(376, 1241, 85), CLOSER).check(level_under=True, total_under=4096, cand_under=True),
    "small": lambda: Case("small", S.corner_img(100, 131, 87), SMALL).check(level_under=True, total_under=4096, cand_under=True),
}


def empty_box_levels(c):
    """levels of a case whose border box is empty"""
    return [l for l in range(c.prm["nlevels"]) if c.pyr[l].shape[1] <= 2 * EDGE or c.pyr[l].shape[0] <= 2 * EDGE]


# ---- descriptor sets for the matcher ------------------------------------------------------------------------------------------------
def random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def related_sets(rng, na, nb, nshared, flips=14):
    """two descriptor sets that share nshared members up to a few flipped bits (a's last ones are b's first ones)"""
    a, b = random_desc(rng, na), random_desc(rng, nb)
    k = min(nshared, na, nb)
    if k:
        b[:k] = a[na - k:]
        b[:k] ^= ((rng.integers(0, 256, (k, 32)) < flips) * (1 << rng.integers(0, 8, (k, 32)))).astype(np.uint8)
    return a, b
