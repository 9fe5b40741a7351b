"""Inputs that drive the corner selection behind the corner-response pass (k_gftt_pick and the two FeatureDEM kernels of
flvis_amd/csrc/img_kernels.hip) to its tier, plateau, capacity and spacing edges, with what the CPU oracle (oracle/ref_image.cpp) says
about each of them.  No GPU is needed here: tests/test_gftt_edges_inputs.py builds every recipe and pins its figures with the oracle
alone, tests/test_gpu_gftt_edges.py compares the kernels against what is built here.

k_gftt_pick does not sort all candidates.  It builds a histogram of the top 12 bits of the (order preserving) response, takes the best
bins that fit a tier (the first one max(3 maxCorners, 1024) keys where 3 maxCorners < 4096, every other one 4096), sorts and walks the
tier, and goes on to the next one while maxCorners is not reached and bins are left.  A bin that alone holds more than 4096 keys sends
it to the full sort ("s_full": bitmap cleared, everything sorted through L2, the sorted array walked in slices of 4096).  tier_model()
restates that DECISION in numpy from the oracle's candidates and the oracle's corners; it says which path an input takes and is never
the expected output.  A recipe asserts the path it is there for when it is built: a generator that drifts fails here, on the CPU."""
import functools

import numpy as np

import _oracle as O
import _synth as S

SORT_LDS = 4096             # keys of one LDS tier / one slice of the fully sorted array (img_kernels.hip)
PICK_BINS = 4096            # histogram bins: the top 12 bits of the ordered response
DEM_MAXC = 4096             # FeatureDEM: most GFTT corners of one call
DEM_MAXR = 192              # FeatureDEM: entries kept per region in LDS


def old_key_cap(w, h):
    """the key scratch as it was sized until this suite existed ("strict maxima cannot exceed ~w*h/4")"""
    cap = 1
    while cap < (w // 2 + 1) * (h // 2 + 1):
        cap <<= 1
    return cap


def key_cap(w, h):
    """gftt_key_cap of img_kernels.hpp: every interior pixel can be a candidate"""
    cap = 1
    while cap < (w - 2) * (h - 2):
        cap <<= 1
    return cap


# ---- images ---------------------------------------------------------------------------------------------------------------------------
def blocks(h, w, b):
    """block checkerboard: plateaus of equal positive response around every block corner"""
    return (((np.arange(h)[:, None] // b + np.arange(w)[None, :] // b) % 2) * 255).astype(np.uint8)


def tiled(h, w, seed, period=16):
    """one period x period texture patch repeated over the image (the _tiled of test_gpu_image.py): every corner recurs with the same
    neighbourhood, so responses and FeatureDEM's integer-built scores tie by the dozen"""
    t = S.texture_u8(3 * period, 3 * period, seed)[period:2 * period, period:2 * period]
    return np.tile(t, (h // period + 1, w // period + 1))[:h, :w].copy()


def texture_over_blocks(h, w, seed, b, split):
    """rows < split: texture (many response bins, the best ones); rows >= split: a block checkerboard at low contrast (one response value
    below the texture's strong corners)"""
    img = S.texture_u8(h, w, seed)
    lo = (blocks(h, w, b) // 255 * 24 + 100).astype(np.uint8)
    img[split:] = lo[split:]
    return img


# ---- the candidate list of goodFeaturesToTrack, from the oracle's response map ----------------------------------------------------------
def _ordered(f32):
    b = np.asarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b >> np.uint64(31), b ^ np.uint64(0xFFFFFFFF), b ^ np.uint64(0x80000000))


def candidates(img):
    """-> (max ordered bits, ordered response [n], pixel offset [n]) of every 3x3 maximum (e > 0 and no neighbour greater, interior
    pixels), in walk order: response descending, offset descending"""
    e = O.min_eigen_map(img)
    h, w = e.shape
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = e
    nb = np.full((h, w), -np.inf, np.float32)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                nb = np.maximum(nb, pad[dy:dy + h, dx:dx + w])
    ismax = (e > 0) & ~(nb > e)
    ismax[0, :] = ismax[-1, :] = False
    ismax[:, 0] = ismax[:, -1] = False
    ys, xs = np.nonzero(ismax)
    o = _ordered(e[ys, xs])
    off = (ys * w + xs).astype(np.uint64)
    order = np.argsort((o << np.uint64(32)) | off)[::-1]
    return float(e.max()), o[order], off[order].astype(np.int64)


def response_keys(img):
    """what debug_corner_response returns for img: (ordered bits of the maximum, the sorted keys ~((ordered << 32) | offset))"""
    mx, o, off = candidates(img)
    return int(_ordered(np.float32(mx))), np.sort(~((o << np.uint64(32)) | off.astype(np.uint64)))


def tier_model(img, maxc, q, md):
    """which way k_gftt_pick goes on this input -> dict of figures.  ranks are 1-based positions in walk order."""
    h, w = img.shape
    mx, o, off = candidates(img)
    want = O.gftt(img, maxc, q, md)
    thr = _ordered(np.float32(np.float64(np.float32(mx)) * q))
    keep = o > thr
    ko, koff = o[keep], off[keep]              # (a prefix: the order is response descending)
    assert keep[:len(ko)].all()
    bins = (ko >> np.uint64(20)).astype(np.int64)
    count = np.bincount(bins, minlength=PICK_BINS)
    suffix = np.concatenate([np.cumsum(count[::-1])[::-1], [0]])       # suffix[b] = keys in bins >= b
    # rank of every accepted corner
    pos = {int(p): i for i, p in enumerate(koff)}
    ranks = np.array([pos[int(y) * w + int(x)] + 1 for x, y in want], np.int64)
    assert np.all(np.diff(ranks) > 0)
    last = int(ranks[-1]) if len(ranks) else 0
    tiers, hi, full, done = [], PICK_BINS, False, 0
    while hi > 0:
        tier = SORT_LDS
        if hi == PICK_BINS and 3 * maxc < SORT_LDS:
            tier = max(3 * maxc, 1024)
        base = suffix[hi]
        if count[hi - 1] > SORT_LDS:
            full = True
            break
        if count[hi - 1] > tier:
            tier = SORT_LDS
        lo = hi - 1
        while lo > 0 and suffix[lo - 1] - base <= tier:
            lo -= 1
        m = int(suffix[lo] - base)
        hi = lo
        if m == 0:                      # (only empty bins above a bin that does not fit: the device walks an empty tier and looks again)
            continue
        tiers.append(m)
        done += m
        if int((ranks <= done).sum()) >= maxc:
            break
    exhausted = len(want) < maxc
    slices = 0
    if full:
        slices = -(-len(ko) // SORT_LDS) if exhausted else -(-last // SORT_LDS)
    vals, cls = np.unique(ko, return_counts=True)
    return dict(cand=len(o), kept=len(ko), bin=int(count.max()) if len(ko) else 0, tiers=tiers, full=full, slices=slices,
                accepted=len(want), last=last, tied=int(cls.max()) if len(ko) else 0, exhausted=exhausted)


class GCase:
    """one goodFeaturesToTrack call: img, maxc, q, md; want = the oracle's corners; fig = tier_model's figures"""

    def __init__(self, name, img, maxc, q, md):
        self.name, self.img, self.maxc, self.q, self.md = name, np.ascontiguousarray(img), int(maxc), float(q), float(md)
        self.want = O.gftt(self.img, self.maxc, self.q, self.md)
        self.fig = tier_model(self.img, self.maxc, self.q, self.md)
        self.h, self.w = self.img.shape

    @property
    def args(self):
        return self.img, self.maxc, self.q, self.md

    def pinned(self):
        f = self.fig
        return (f["cand"], f["kept"], f["bin"], tuple(f["tiers"]), f["full"], f["accepted"], f["last"], f["tied"])

    def check(self, tiers=None, first_tier=None, second_tier=None, exhausted=None, full=None, tiers_before_full=None, slices=None,
              over_old_cap=None, accepted=None, all_kept=None, one_value=None, near_borders=None):
        f, n = self.fig, self.name
        if tiers is not None:
            assert len(f["tiers"]) == tiers and not f["full"], (n, "walks %d tiers, not %d" % (len(f["tiers"]), tiers), f)
        if first_tier is not None:      # the size the first tier is cut to
            want = SORT_LDS if 3 * self.maxc >= SORT_LDS else max(3 * self.maxc, 1024)
            assert want == first_tier and f["tiers"] and f["tiers"][0] <= first_tier, (n, "first tier", want, f)
        if second_tier:
            assert len(f["tiers"]) >= 2 and f["last"] > f["tiers"][0], (n, "the second tier is not walked", f)
        if exhausted is not None:
            assert f["exhausted"] == exhausted, (n, "exhausted" if f["exhausted"] else "stops at maxCorners", f)
            if exhausted and not f["full"]:
                assert sum(f["tiers"]) == f["kept"], (n, "tiers left over", f)
        if full is not None:
            assert f["full"] == full, (n, "s_full" if f["full"] else "no s_full", f)
        if tiers_before_full is not None:
            assert f["full"] and len(f["tiers"]) >= tiers_before_full, (n, "tiers walked before s_full", f)
        if slices is not None:
            assert f["full"] and f["slices"] >= slices, (n, "slices of the sorted array walked", f)
        if over_old_cap:
            assert old_key_cap(self.w, self.h) < f["cand"] <= key_cap(self.w, self.h), (n, f["cand"], old_key_cap(self.w, self.h))
        elif over_old_cap is not None:
            assert f["cand"] <= old_key_cap(self.w, self.h), (n, f["cand"], old_key_cap(self.w, self.h))
        if accepted is not None:
            assert f["accepted"] == accepted, (n, f["accepted"], accepted)
        if all_kept:
            assert f["accepted"] == f["kept"] == f["cand"] < self.maxc, (n, f)
        if one_value is not None:       # at most this many keys outside the largest class of equal responses
            assert f["kept"] - f["tied"] <= one_value and f["tied"] > 1, (n, "ties", f)
        if near_borders:
            x, y = self.want[:, 0], self.want[:, 1]
            r = self.md
            assert (x < r).any() and (y < r).any() and (x > self.w - 1 - r).any() and (y > self.h - 1 - r).any(), (n, "no corner near a border")
        return self


# ---- FeatureDEM -----------------------------------------------------------------------------------------------------------------------
def dem_regions(img, fp, pts):
    """fillIntoRegion's region of every point, -1 for the 3-pixel rim and outside"""
    h, w = img.shape
    rw, rh = np.float32(w // 4), np.float32(h // 4)
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    inside = (x >= 3) & (x < w - 3) & (y >= 3) & (y < h - 3)
    r = (np.float32(4) * np.floor(y / rh) + x / rw).astype(np.int64)
    return np.where(inside, r, -1)


class DCase:
    """one FeatureDEM call: img, fp (f_para), exist (None: detect; [n,2] float64: redetect); want = the oracle's features"""

    def __init__(self, name, img, fp, exist=None):
        self.name, self.img, self.fp = name, np.ascontiguousarray(img), [float(v) for v in fp]
        self.exist = None if exist is None else np.ascontiguousarray(exist, np.float64).reshape(-1, 2)
        self.h, self.w = self.img.shape
        if self.exist is None:
            self.want = O.dem_detect(self.img, self.fp)
            self.gftt = O.gftt(self.img, 2 * int(self.fp[3]), self.fp[4], float(int(self.fp[5])))
        else:
            self.want = O.dem_redetect(self.img, self.fp, self.exist)
            self.gftt = O.gftt(self.img, int(self.fp[3]), self.fp[4], float(int(self.fp[5])))
        self.regions = np.bincount(dem_regions(self.img, self.fp, self.want) + 1, minlength=17)[1:]
        self.cand_regions = np.bincount(dem_regions(self.img, self.fp, self.gftt) + 1, minlength=17)[1:]
        self.exist_regions = (np.zeros(16, np.int64) if self.exist is None else
                              np.bincount(dem_regions(self.img, self.fp, self.exist) + 1, minlength=17)[1:])

    def pinned(self):
        return (len(self.gftt), len(self.want), int(self.regions.max()), int(self.exist_regions.max()))

    def check(self, features=None, fullest=None, corners=None, exist_over=None, region_full=None, min_features=None, tied=None):
        n = self.name
        if tied:                        # a region of more than 16 candidates (std::sort leaves its insertion sort) with equal scores in it
            cand, cls = tied_region(self)
            assert cand > 16 and cls > 1, (n, "no tied region", cand, cls)
        if features is not None:
            assert len(self.want) == features, (n, len(self.want), features)
        if min_features is not None:
            assert len(self.want) >= min_features, (n, len(self.want), min_features)
        if fullest is not None:
            assert self.regions.max() == fullest, (n, self.regions)
        if corners is not None:
            assert len(self.gftt) == corners, (n, len(self.gftt), corners)
        if exist_over is not None:
            assert self.exist_regions.max() > exist_over, (n, self.exist_regions)
        if region_full is not None:     # a region holds max_region_feature_num existing points or more, and has candidates
            mx = int(self.fp[0])
            assert ((self.exist_regions >= mx) & (self.cand_regions > 0)).any(), (n, self.exist_regions, self.cand_regions)
        return self


def tied_region(c):
    """-> (candidates, size of the largest class of equal Harris scores) of the region of a detect case where that class is largest;
    the scores are calHarrisR's (the oracle's FeatureDEM holds the only implementation, so they are restated from feature_dem.cpp:59-88
    as the device restates them)"""
    img = c.img.astype(np.int64)
    reg = dem_regions(c.img, c.fp, c.gftt)
    best = (0, 0)
    for r in range(16):
        p = c.gftt[reg == r].astype(np.int64)
        if not len(p):
            continue
        x, y = p[:, 0], p[:, 1]
        p0, p1, p2 = img[y - 1, x - 1], img[y - 1, x], img[y - 1, x + 1]
        p3, p5 = img[y, x - 1], img[y + 1, x + 1]
        p6, p7, p8 = img[y + 1, x - 1], img[y + 1, x], img[y + 1, x + 1]
        trunc = lambda v: np.sign(v) * (np.abs(v) // 3)          # C++ integer division
        ix, iy = trunc(p0 + p3 + p6 - (p2 + p5 + p8)), trunc(p0 + p1 + p2 - (p6 + p7 + p8))
        _, cls = np.unique(np.stack([ix, iy], 1), axis=0, return_counts=True)   # equal (IX, IY) <=> equal score inputs
        if cls.max() > best[1]:
            best = (len(p), int(cls.max()))
    return best


def _T(h, w, seed):
    return S.texture_u8(h, w, seed)


def _exist_grid(x0, y0, nx, ny, step):
    """nx x ny existing points from (x0, y0), `step` apart, off the integer grid"""
    xs, ys = np.meshgrid(x0 + step * np.arange(nx), y0 + step * np.arange(ny))
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)


FP_SMALL = [8, 30, 5, 200, 0.001, 3]


def _redetect_crowded():
    """more than DEM_MAXR existing points in region 0 of 96 x 128 (regions 32 x 24), all in its upper left corner; the 193rd and later
    ones sit ON the region's strongest candidates further down, where the reference refuses them"""
    img = _T(96, 128, 47)
    first = O.dem_redetect(img, FP_SMALL, np.zeros((0, 2)))
    reg = dem_regions(img, FP_SMALL, first)
    mine = first[reg == 0].astype(np.float64)
    ex = np.concatenate([_exist_grid(3.25, 3.25, 20, 10, 0.0625), mine])
    c = DCase("redetect_crowded", img, FP_SMALL, ex).check(exist_over=DEM_MAXR, region_full=True)
    late = np.nonzero(dem_regions(img, FP_SMALL, ex) == 0)[0][DEM_MAXR:]
    short = O.dem_redetect(img, FP_SMALL, np.delete(ex, late, axis=0))
    assert len(short) == len(c.want) + 1, (c.name, "the existing points behind the first %d of the region decide nothing" % DEM_MAXR)
    return c


def _redetect_cluster(name, n):
    """n existing points in the upper left corner of region 0 and nowhere else: the region is full before the walk and takes exactly
    one new point, its best candidate off the cluster's cross"""
    img = _T(96, 128, 47)
    ex = _exist_grid(3.25, 3.25, 20, 11, 0.0625)[:n]
    c = DCase(name, img, FP_SMALL, ex).check(region_full=True)
    assert c.exist_regions[0] == n == len(ex) and c.regions[0] == 1, (name, c.exist_regions, c.regions)
    return c


def _redetect_places():
    """existing points in the 3-pixel rim, outside the image, exactly on region borders and inside"""
    img = _T(96, 128, 48)
    ex = np.array([[1.0, 1.0], [2.99, 50.0], [125.0, 40.0], [124.99, 40.0], [-5.0, 10.0], [300.0, 20.0], [60.0, 93.0], [60.0, 92.99],
                   [32.0, 24.0], [64.0, 48.0], [31.99, 24.0], [96.0, 72.0], [63.5, 23.5], [40.4, 60.6], [100.2, 30.7], [3.0, 3.0]])
    c = DCase("redetect_places", img, FP_SMALL, ex).check(min_features=48)
    assert (dem_regions(img, FP_SMALL, ex) < 0).sum() == 6 and c.exist_regions.sum() == 10, (c.name, c.exist_regions)
    return c


def _redetect_full_region():
    """regions already at max_region_feature_num (8) or above before the walk: "push, then check the size" still lets one new point in"""
    img = _T(96, 128, 49)
    ex = np.concatenate([_exist_grid(4.3, 4.3, 4, 2, 0.125),            # region 0: exactly 8
                         _exist_grid(40.3, 30.3, 3, 3, 0.125),          # region 5: 9
                         _exist_grid(100.3, 80.3, 7, 1, 0.125)])        # region 15: 7, one short
    c = DCase("redetect_full_region", img, FP_SMALL, ex).check(region_full=True)
    assert list(c.exist_regions[[0, 5, 15]]) == [8, 9, 7] and list(c.regions[[0, 5, 15]]) == [1, 1, 1], (c.name, c.exist_regions, c.regions)
    return c


# ---- the recipes.  Each is built once per process; nothing that holds one changes it -------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    return RECIPES[name]()


def _G(name, img, maxc, q, md, **chk):
    return lambda: GCase(name, img() if callable(img) else img, maxc, q, md).check(**chk)


def _D(name, img, fp, exist=None, **chk):
    return lambda: DCase(name, img(), fp, exist() if callable(exist) else exist).check(**chk)


_T41 = lambda: _T(240, 320, 41)
_T42 = lambda: _T(96, 128, 42)
_T137 = lambda: _T(240, 320, 137)       # its best bins hold 846 and 1025 keys: the tier sizes 1024 and 1026 cut it at different bins


def _patch():
    """128 x 160, flat but for a 50 x 60 texture patch: fewer spaced corners than any maxCorners used on it"""
    img = np.full((128, 160), 90, np.uint8)
    img[40:90, 50:110] = _T(128, 160, 51)[40:90, 50:110]
    return img


def _tied_exist():
    first = O.dem_detect(tiled(128, 128, 7, 8), FP_TIED)
    return first[::3].astype(np.float64) + np.array([0.37, -0.21])


FP_TIED = [30, 30, 3, 1000, 0.001, 1]
FP_MAXC = [192, 30, 2, 2048, 1e-6, 1]
RAGGED = (150, 0.01, 3)                 # one call: the full sort, a flat image, an exhausted walk and a plain one
RAGGED_NEXT = (300, 0.01, 2.5)          # the call right after it, on images of another size

RECIPES = {
    # ---- tier hand-over and exhaustion
    "tier_second": _G("tier_second", _T41, 300, 0.001, 12, tiers=2, first_tier=1024, second_tier=True, exhausted=False, full=False),
    "tier_first_only": _G("tier_first_only", _T41, 100, 0.001, 12, tiers=1, first_tier=1024, exhausted=False),
    "switch_341": _G("switch_341", _T137, 341, 0.001, 12, tiers=2, first_tier=1024, second_tier=True),
    "switch_342": _G("switch_342", _T137, 342, 0.001, 12, tiers=2, first_tier=1026, second_tier=True),
    "switch_1365": _G("switch_1365", _T41, 1365, 0.001, 1, tiers=1, first_tier=4095, exhausted=False),
    "switch_1366": _G("switch_1366", _T41, 1366, 0.001, 1, tiers=1, first_tier=4096, exhausted=False),
    "exhausted": _G("exhausted", _T41, 2000, 0.001, 20, tiers=2, exhausted=True, accepted=132),
    # ---- the full sort
    "full_md3": _G("full_md3", lambda: blocks(128, 160, 4), 150, 0.01, 3, full=True, slices=1, one_value=0, over_old_cap=False),
    "full_md0": _G("full_md0", lambda: blocks(128, 160, 4), 150, 0.01, 0, full=True, slices=1, one_value=0, over_old_cap=False),
    "full_slices": _G("full_slices", lambda: blocks(160, 192, 4), 1500, 0.01, 2, full=True, slices=2, exhausted=False, over_old_cap=False),
    "full_after_tiers": _G("full_after_tiers", lambda: texture_over_blocks(160, 192, 44, 4, 60), 4000, 0.0005, 2, tiers_before_full=1,
                           slices=2, over_old_cap=False),
    # ---- plateaus: the order inside a class of equal responses is pixel offset descending alone
    "plateau_tile_a": _G("plateau_tile_a", lambda: tiled(128, 128, 7, 8), 500, 0.01, 3, tiers=1, over_old_cap=False),
    "plateau_tile_b": _G("plateau_tile_b", lambda: tiled(128, 128, 8, 8), 500, 0.01, 3, tiers=1, over_old_cap=False),
    "plateau_b5": _G("plateau_b5", lambda: blocks(120, 160, 5), 300, 0.01, 4, tiers=1, one_value=0, over_old_cap=False),
    # ---- more candidates than (w / 2 + 1)(h / 2 + 1)
    "over_b2_64": _G("over_b2_64", lambda: blocks(64, 64, 2), 200, 0.01, 3, over_old_cap=True, full=False),
    "over_b3_64": _G("over_b3_64", lambda: blocks(64, 64, 3), 200, 0.01, 3, over_old_cap=True, full=False),
    "over_b2_96": _G("over_b2_96", lambda: blocks(96, 128, 2), 200, 0.01, 3, over_old_cap=True, full=True),
    "over_b3_96": _G("over_b3_96", lambda: blocks(96, 128, 3), 200, 0.01, 3, over_old_cap=True, full=True),
    # ---- spacing: use_dist off, lrint / __double2int_rn on halves, the strict disc test, the largest radius, the clamped rows
    "space_0": _G("space_0", _T42, 300, 0.01, 0, accepted=300),
    "space_0.99": _G("space_0.99", _T42, 300, 0.01, 0.99, accepted=300),
    "space_1": _G("space_1", _T42, 300, 0.01, 1.0, accepted=300),
    "space_1.5": _G("space_1.5", _T42, 300, 0.01, 1.5, accepted=300),
    "space_2": _G("space_2", _T42, 300, 0.01, 2.0, accepted=300),
    "space_2.5": _G("space_2.5", _T42, 300, 0.01, 2.5, accepted=300),
    "space_4.5": _G("space_4.5", _T42, 300, 0.01, 4.5, exhausted=True),
    "far_63.5": _G("far_63.5", _T41, 300, 0.01, 63.5, exhausted=True, accepted=19),
    "far_64": _G("far_64", _T41, 300, 0.01, 64.0, exhausted=True, accepted=19),
    "borders_w132": _G("borders_w132", lambda: _T(100, 132, 43), 300, 0.001, 6, near_borders=True, exhausted=True),
    # ---- quality
    "quality_1": _G("quality_1", _T42, 300, 1.0, 3, accepted=0),
    "quality_tiny": _G("quality_tiny", _T42, 3000, 1e-12, 1, all_kept=True),
    # ---- one ragged call, and the call after it
    "ragged_full": _G("ragged_full", lambda: blocks(128, 160, 4), *RAGGED, full=True),
    "ragged_flat": _G("ragged_flat", lambda: np.full((128, 160), 100, np.uint8), *RAGGED, accepted=0),
    "ragged_exhausted": _G("ragged_exhausted", _patch, *RAGGED, exhausted=True, tiers=1),
    "ragged_plain": _G("ragged_plain", lambda: _T(128, 160, 52), *RAGGED, exhausted=False, tiers=1),
    "next_plain": _G("next_plain", _T42, *RAGGED_NEXT, accepted=300),
    "next_over": _G("next_over", lambda: blocks(96, 128, 3), *RAGGED_NEXT, over_old_cap=True, full=True),
    # ---- FeatureDEM: sizes (the 3-pixel rim leaves little or nothing of the small ones)
    "dem_8x8": _D("dem_8x8", lambda: _T(8, 8, 45), FP_SMALL, features=0),
    "dem_12x16": _D("dem_12x16", lambda: _T(12, 16, 45), FP_SMALL, min_features=1),
    "dem_32x32": _D("dem_32x32", lambda: _T(32, 32, 45), FP_SMALL, min_features=8),
    "dem_64x64": _D("dem_64x64", lambda: _T(64, 64, 45), FP_SMALL, min_features=16),
    "dem_96x128": _D("dem_96x128", lambda: _T(96, 128, 45), FP_SMALL, min_features=64),
    "dem_100x132": _D("dem_100x132", lambda: _T(100, 132, 45), FP_SMALL, min_features=64),
    "dem_re_12x16": _D("dem_re_12x16", lambda: _T(12, 16, 45), FP_SMALL, np.zeros((0, 2)), min_features=1),
    "dem_re_100x132": _D("dem_re_100x132", lambda: _T(100, 132, 45), FP_SMALL, np.zeros((0, 2)), min_features=64),       # nexist = 0
    # ---- FeatureDEM: parameters and capacities
    "dem_maxc": _D("dem_maxc", lambda: _T(240, 320, 46), FP_MAXC, corners=DEM_MAXC, features=375, fullest=26),
    "dem_int_md": _D("dem_int_md", lambda: _T(96, 128, 45), [8, 30, 5, 200, 0.001, 0.9], min_features=64),
    "dem_bd0": _D("dem_bd0", lambda: _T(96, 128, 45), [8, 30, 1, 200, 0.001, 3], features=128, fullest=8),
    "redetect_crowded": _redetect_crowded,
    "redetect_at_capacity": lambda: _redetect_cluster("redetect_at_capacity", DEM_MAXR),
    "redetect_over_capacity": lambda: _redetect_cluster("redetect_over_capacity", DEM_MAXR + 25),
    "redetect_places": _redetect_places,
    "redetect_full_region": _redetect_full_region,
    # ---- FeatureDEM: tied scores in a region of more than 16 candidates (std::sort's quicksort phase)
    "dem_tied": _D("dem_tied", lambda: tiled(128, 128, 7, 8), FP_TIED, min_features=100, tied=True),
    "dem_tied_re": _D("dem_tied_re", lambda: tiled(128, 128, 7, 8), FP_TIED, _tied_exist, min_features=30, tied=True),
}

BATCHES = {"ragged": ("ragged_full", "ragged_flat", "ragged_exhausted", "ragged_plain"), "ragged_next": ("next_plain", "next_over")}
GFTT = sorted(n for n in RECIPES if not n.startswith(("dem_", "redetect_")))
DEM = sorted(n for n in RECIPES if n.startswith(("dem_", "redetect_")))
PLATEAUS = ("plateau_tile_a", "plateau_tile_b", "plateau_b5")
OVER = ("over_b2_64", "over_b3_64", "over_b2_96", "over_b3_96")
