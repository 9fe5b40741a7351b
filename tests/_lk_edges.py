"""Inputs that drive the pyramidal Lucas-Kanade tracker (flvis_hip_lk_track, flvis_amd/csrc/lk_kernel.hip) to its border, restage, flat
and contrast edges, with what the CPU oracle (oracle/ref_image.cpp::calc_optical_flow_pyr_lk) says about each of them.  No GPU is needed
here: tests/test_lk_edges_inputs.py checks every recipe with the oracle's per-visit trace (O.lk_trace) alone, tests/test_gpu_lk_edges.py
compares the kernel against what is built here, bit for bit.

A Case is one image pair with its points, start positions and the call's parameters; it carries the oracle's answer and trace.  Every
recipe ends in a check that asserts, from the trace, that the input reaches the edge it is there for: a generator that drifts fails
there instead of testing nothing.

The kernel stages a 41-row x 52-byte search region per level around the first iteration's window (4 px margin, the left edge aligned
down to a multiple of 4) and re-stages it when `inx < RX0 || inx - RX0 > 15 || iny < RY0 || iny - RY0 > 8`: a window that has moved more
than 4 px up, down or left, or more than 11 px right, since the level's first iteration has certainly left it."""
import functools

import numpy as np

import _oracle as O
import _synth as S

WIN = 31
H, W = 120, 160
CAUSE = {n: i for i, n in enumerate(O.LK_CAUSES)}
HESSIAN_BOUND = 961 * 4080 ** 2          # 31 x 31 Scharr values of at most 16 * 255


class Case:
    """one image pair.  pts / init [n,2] float32; kw: max_level, max_iter, eps, use_initial as O.lk and Context.lk_track take them;
    out / st: the oracle's answer; tr: its trace (O.lk_trace)"""

    def __init__(self, name, prev, nxt, pts, init, **kw):
        self.name = name
        self.prev, self.nxt = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8)
        self.pts, self.init = np.ascontiguousarray(pts, np.float32).reshape(-1, 2), np.ascontiguousarray(init, np.float32).reshape(-1, 2)
        assert self.prev.shape == self.nxt.shape and self.pts.shape == self.init.shape
        self.kw = dict(dict(max_level=10, max_iter=30, eps=1e-3, use_initial=True), **kw)
        self.out, self.st, self.tr = O.lk_trace(self.prev, self.nxt, self.pts, self.init, **self.kw)
        self.n = len(self.pts)
        for a in (self.prev, self.nxt, self.pts, self.init, self.out, self.st):
            a.setflags(write=False)

    @property
    def levels(self):
        return self.tr["levels"]

    def level_sizes(self):
        h, w = self.prev.shape
        out = [(h, w)]
        for _ in range(self.levels):
            h, w = (h + 1) // 2, (w + 1) // 2
            out.append((h, w))
        return out

    def cause(self, name, level=None):
        """number of points that left a level (the level where that happens most often, if none is named) through `name`"""
        c = (self.tr["cause"] == CAUSE[name]).sum(1)
        return int(c.max() if level is None else c[level])

    def moved(self, axis, more_than):
        """number of points whose window moved more than `more_than` px along `axis` within one level, at the level where most did"""
        return int((self.tr["move_" + axis] > more_than).sum(1).max())

    def hessian(self):
        return int(max(self.tr["a11"].max(), self.tr["a22"].max()))

    def residual(self):
        return int(max(self.tr["b1"].max(), self.tr["b2"].max()))

    def figures(self):
        """what test_lk_edges_inputs.py pins"""
        return dict(n=self.n, ok=int(self.st.sum()), y4=self.moved("y", 4), x4=self.moved("x", 4), x11=self.moved("x", 11),
                    exhausted=self.cause("exhausted"), left=self.cause("left_image"), flat0=self.cause("flat", 0))

    def check(self, **at_least):
        """at_least: figure name -> lower bound.  Every case: at most ~200 points unless the recipe says otherwise, no level below 32 px
        (the oracle reflects once: its reads stay inside its buffers only then; lk_num_levels guarantees it)"""
        assert all(h >= 32 and w >= 32 for h, w in self.level_sizes()), (self.name, self.level_sizes())
        f = self.figures()
        for k, v in at_least.items():
            assert f[k] >= v, (self.name, k, f[k], "expected at least", v)
        return self


@functools.lru_cache(maxsize=None)
def case(name):
    return RECIPES[name]()


def grid(h, w, step, x0, y0):
    """points every `step` px over the whole image, the first at (x0, y0)"""
    ys, xs = np.meshgrid(np.arange(y0, h, step), np.arange(x0, w, step), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


# ---- far_start: starts far from the answer --------------------------------------------------------------------------------------------
def _texture_pair(seed=300, dx=2.3, dy=-1.6, h=H, w=W, npts=150):
    prev, nxt = S.shifted_pair(h, w, seed, dx, dy)
    return prev, nxt, O.gftt(prev, npts, 0.01, 6)


def far_start(name, lo, hi, max_level, seed, npts=150):
    """corners of a texture pair, each start displaced by uniform [lo, hi) px per axis (lo, hi: pairs)"""
    prev, nxt, pts = _texture_pair(npts=npts)
    rng = np.random.default_rng(seed)
    init = pts + rng.uniform(lo, hi, pts.shape).astype(np.float32)
    return Case(name, prev, nxt, pts, init, max_level=max_level)


# ---- flat: templates without texture --------------------------------------------------------------------------------------------------
def flat_image():
    """gray with one random-texture block, one 4-px vertical bar and one 4-px horizontal bar (pure aperture: a singular Hessian)"""
    img = np.full((H, W), 128, np.uint8)
    img[14:54, 12:60] = np.random.default_rng(310).integers(0, 256, (40, 48), dtype=np.uint8)
    img[8:112, 100:104] = 230
    img[84:88, 8:92] = 20
    return img


def flat_case():
    img = flat_image()
    pts = grid(H, W, 9, 6.3, 5.6)
    return Case("flat", img, np.roll(img, (1, 2), (0, 1)), pts, pts, max_level=10)


def flat_figures(c):
    """flat at level 0 / flat at a coarser level / flat at one level and iterated at the other / status 1"""
    assert c.levels == 1
    fl = c.tr["cause"] == CAUSE["flat"]
    ran = c.tr["iters"] > 0
    return dict(flat0=int(fl[0].sum()), flat1=int(fl[1].sum()), mixed=int(((fl[1] & ran[0]) | (fl[0] & ran[1])).sum()), ok=int(c.st.sum()))


def constant_case():
    img = np.full((H, W), 77, np.uint8)
    pts = grid(H, W, 12, 3.25, 4.5)
    return Case("constant", img, img, pts, pts + np.float32(1.5))


# ---- contrast: the largest sums ---------------------------------------------------------------------------------------------------------
def blocks(cell, seed=320, h=H, w=W):
    """binary 0 / 255 random blocks of cell x cell px"""
    b = np.random.default_rng(seed + cell).integers(0, 2, ((h + cell - 1) // cell, (w + cell - 1) // cell), dtype=np.uint8) * 255
    return np.kron(b, np.ones((cell, cell), np.uint8))[:h, :w]


def stripes(vertical, h=H, w=W):
    """period-4 stripes (two px of 0, two of 255) whose phase flips every 16 px along them: stripes alone are pure aperture (a singular
    Hessian, rejected before the first iteration); the flips give the other gradient its few non-zero rows.  Shifted by one px across
    the stripes, every residual has the sign of the gradient under it."""
    a, b = np.arange(w if vertical else h), np.arange(h if vertical else w)
    img = (((a[None, :] // 2 + b[:, None] // 16) % 2) * 255).astype(np.uint8)
    return np.ascontiguousarray(img if vertical else img.T)


def contrast(name, prev, how):
    nxt = {"inverse": 255 - prev, "roll": np.roll(prev, (1, 1), (0, 1)), "same": prev, "rollx": np.roll(prev, 1, 1), "rolly": np.roll(prev, 1, 0)}[how]
    pts = grid(H, W, 12, 20.37, 18.71)
    pts = pts[(pts[:, 0] < W - 18) & (pts[:, 1] < H - 16)]
    return Case(name, prev, nxt, pts, pts)


# ---- tiny: images down to the smallest the entry accepts ----------------------------------------------------------------------------------
TINY_SIZES = ((32, 32), (64, 64), (33, 47), (64, 40), (40, 200))


def tiny(h, w):
    """points every 4 px over the whole image (more than 200 on the larger sizes: the grid is the recipe)"""
    prev, nxt = S.shifted_pair(h, w, 330 + h + w, 1.4, -0.8, margin=16)
    pts = grid(h, w, 4, 1.5, 2.25)
    return Case("tiny_%dx%d" % (h, w), prev, nxt, pts, pts + np.float32(0.5))


# ---- rim: window starts on the status thresholds ---------------------------------------------------------------------------------------------
# A window (template or search) starts at floor(x - 15); the point is dropped when that start is < -31 or >= W (and the same in y).
def rim_starts(n):
    """window-start coordinates around both thresholds of an axis of n px -> [(start, inside)]: -32, -31, -31 + ulp, n - 1, n as the
    threshold tests have them, the float next to each, half-integer starts on either side, and starts up to 3 px inside.  (A window that
    starts exactly at -31 or n - 1 holds one image column, the border column, whose derivative across the border is 0 by the reflection:
    that template is singular whatever the image, so the status-1 points of a template threshold are the ones a little further in.)"""
    f = np.float32
    lo, hi = f(-31.0), f(n)
    out = [(f(-32.0), False), (np.nextafter(lo, f(-40)), False), (lo, True), (np.nextafter(lo, f(0)), True), (f(-31.5), False), (f(-30.5), True),
           (f(n - 1), True), (np.nextafter(hi, f(0)), True), (hi, False), (np.nextafter(hi, f(2 * n)), False), (f(n - 0.5), True), (f(n + 0.5), False),
           (f(n - 1.5), True), (f(-29.0), True), (f(-28.25), True), (f(n - 3.0), True), (f(n - 3.75), True)]
    for s, inside in out:
        assert (-31 <= np.floor(s) < n) == inside
    return out


RIM_ALONG = (28.0, 44.5, 59.999, 75.0, 91.5, 106.999)    # the coordinate along the edge: integer, half-integer, just below an integer


def rim_case(search):
    """template rim (search False): the point itself sits on a threshold and the second image is the first, so the status says whether
    the template was taken (a sliver of image under a window that hangs out by 30 px is enough texture on binary blocks) and nothing
    about where the iteration went.  search rim (search True): the point is well inside and only its start sits on a threshold, on an
    image that has moved by a pixel.  max_level 0: level 0 sees the coordinates as they are given.
    group[i]: the threshold point i belongs to, inside[i]: on which side of it."""
    prev = blocks(1, seed=340)
    nxt = np.roll(prev, (1, 1), (0, 1)) if search else prev
    pts, init, group, inside = [], [], [], []
    for axis, n in ((0, W), (1, H)):
        for s, ins in rim_starts(n):
            for t in RIM_ALONG:
                q, home = [0, 0], [0, 0]
                q[axis], q[1 - axis] = np.float32(s) + np.float32(15), np.float32(t)
                home[axis], home[1 - axis] = np.float32(24.0 if s < 0 else n - 25.0), np.float32(t)     # (the point whose start has left it)
                pts.append(home if search else q), init.append(q), inside.append(ins)
                group.append(("left", "top")[axis] if s < 0 else ("right", "bottom")[axis])
    c = Case("rim_search" if search else "rim_template", prev, nxt, pts, init, max_level=0)
    c.group, c.inside = np.array(group), np.array(inside)
    return c


def rim_check(c):
    """every threshold: outside it every point is dropped for that very reason before anything is computed, inside it both status values
    occur"""
    why = CAUSE["left_image" if c.name == "rim_search" else "template_outside"]
    for g in ("left", "right", "top", "bottom"):
        m = c.group == g
        out, ins = m & ~c.inside, m & c.inside
        assert out.sum() >= 12 and ins.sum() >= 12, (c.name, g)
        assert not c.st[out].any() and (c.tr["cause"][0][out] == why).all() and (c.tr["iters"][0][out] == 0).all(), (c.name, g)
        assert c.st[ins].any() and not c.st[ins].all(), (c.name, g, c.st[ins])
    return c


def step_out_case():
    """a start that is inside and whose first step leads outside: points whose search window starts a few px from the right / bottom
    threshold, on an image pair that moves 6 px further that way"""
    prev = S.texture_u8(H, W, 350)
    nxt = np.roll(prev, (6, 6), (0, 1))
    pts, init = [], []
    for k in range(12):
        t = np.float32(20.25 + 7 * k)
        pts.append([W - 26.0, t]), init.append([W + 15 - 2.5 - 0.25 * (k % 4), t])
        pts.append([t, H - 26.0]), init.append([t, H + 15 - 2.5 - 0.25 * (k % 4)])
    return Case("step_out", prev, nxt, pts, init, max_level=0)


# ---- clamps: the argument ranges ---------------------------------------------------------------------------------------------------------
def clamps(name, **kw):
    """one texture pair, 7 px apart (no whole number of px: on an exact copy the residual reaches 0 and even eps = 0 converges); starts
    displaced by up to 12 px so that the iteration limits matter"""
    prev, nxt, pts = _texture_pair(seed=360, dx=6.7, dy=-2.2, npts=100)
    init = pts + np.random.default_rng(361).uniform(-12, 12, pts.shape).astype(np.float32)
    return Case(name, prev, nxt, pts, init, **kw)


RECIPES = {
    "far12_l0": lambda: far_start("far12_l0", (-12, -12), (12, 12), 0, 301).check(y4=20, x4=20, x11=5, exhausted=5),
    "far12_l1": lambda: far_start("far12_l1", (-12, -12), (12, 12), 1, 302).check(y4=20, x4=20),
    "far25_l0": lambda: far_start("far25_l0", (-25, -25), (25, 25), 0, 303).check(y4=20, x4=20, x11=5, exhausted=5, left=3),
    "far25_l1": lambda: far_start("far25_l1", (-25, -25), (25, 25), 1, 304, npts=137).check(y4=20, x4=20, x11=5, exhausted=5, left=3),
    # RX0 is aligned down to a multiple of 4: a move toward -x leaves the region after 4..7 px, one toward +x after 12..15
    "far_neg_x": lambda: far_start("far_neg_x", (-14, 0), (-3, 0), 0, 305).check(x4=20),
    "far_neg_y": lambda: far_start("far_neg_y", (0, -14), (0, -3), 0, 306).check(y4=20),
    "flat": flat_case,
    "constant": constant_case,
    **{"blocks%d_%s" % (c, how): (lambda c=c, how=how: contrast("blocks%d_%s" % (c, how), blocks(c), how).check())
       for c in (1, 2, 4) for how in ("inverse", "roll", "same")},
    "stripes_v": lambda: contrast("stripes_v", stripes(True), "rollx").check(),
    "stripes_h": lambda: contrast("stripes_h", stripes(False), "rolly").check(),
    **{"tiny_%dx%d" % s: (lambda s=s: tiny(*s).check()) for s in TINY_SIZES},
    "rim_template": lambda: rim_check(rim_case(False)),
    "rim_search": lambda: rim_check(rim_case(True)),
    "step_out": lambda: step_out_case().check(left=3),
    "clamp_it0": lambda: clamps("clamp_it0", max_iter=0).check(),
    "clamp_it1": lambda: clamps("clamp_it1", max_iter=1).check(),
    "clamp_it100": lambda: clamps("clamp_it100", max_iter=100, max_level=0).check(),
    "clamp_it250": lambda: clamps("clamp_it250", max_iter=250, max_level=0).check(),
    "clamp_eps0": lambda: clamps("clamp_eps0", eps=0.0).check(),
    "clamp_eps10": lambda: clamps("clamp_eps10", eps=10.0).check(),
    "clamp_eps50": lambda: clamps("clamp_eps50", eps=50.0).check(),
    "clamp_level0": lambda: clamps("clamp_level0", max_level=0).check(),
    "clamp_noinit": lambda: clamps("clamp_noinit", use_initial=False).check(),
}


# the recipes grouped into calls: cases of one image size and one parameter set share a batch (n_img > 1, ragged counts)
BATCHES = (
    ("far12_l0", "far25_l0", "far_neg_x", "far_neg_y", "rim_template", "rim_search", "step_out", "clamp_level0"),
    ("far12_l1", "far25_l1"),
    ("flat", "constant", "blocks1_inverse", "blocks1_roll", "blocks1_same", "blocks2_inverse", "blocks2_roll", "blocks2_same", "blocks4_inverse",
     "blocks4_roll", "blocks4_same", "stripes_v", "stripes_h"),
    ("tiny_32x32",), ("tiny_64x64",), ("tiny_33x47",), ("tiny_64x40",), ("tiny_40x200",),
    ("clamp_it0",), ("clamp_it1",), ("clamp_it100", ), ("clamp_it250",), ("clamp_eps0",), ("clamp_eps10",), ("clamp_eps50",), ("clamp_noinit",),
)


# ---- a crafted stereo sequence for the tracker's own LK launches (cached templates, templates ahead, bordered pyramids) -------------------
# KITTI-like rectified rig (376 x 1241, fx 718.856, baseline 0.12 m).  Binary and textured 21 x 21 patches on gray, each at its own depth;
# the camera moves sideways, 4 frames one way and 8 frames back, so a patch moves by fx * step / Z px per frame (14 px for the farthest,
# 43 px for the nearest) and sits at its disparity in the right image: a rigid scene.  Two thirds of the patches start within 120 px of
# the left or the right image edge: their landmarks approach the edge, hang over it and leave.
SCENE_H, SCENE_W, SCENE_FX, SCENE_B = 376, 1241, 718.856, 0.12
SCENE_FRAMES, SCENE_STEP, SCENE_TURN = 12, 0.18, 4


def _scene_patches(n_edge=60, n_mid=30, seed=2, band=100, z=(3.0, 9.0)):
    rng = np.random.default_rng(seed)
    xs = np.concatenate([rng.uniform(20, 20 + band, n_edge), rng.uniform(SCENE_W - 20 - band, SCENE_W - 20, n_edge),
                         rng.uniform(190, SCENE_W - 190, n_mid)])
    n = len(xs)
    ys = rng.uniform(30, SCENE_H - 30, n)
    Z = rng.uniform(z[0], z[1], n)
    tex = []
    for i in range(n):
        tex.append((rng.integers(0, 2, (21, 21)) * 255).astype(np.uint8) if i % 2 else rng.integers(0, 256, (21, 21)).astype(np.uint8))
    return xs, ys, Z, tex


def _paste(img, tex, x, y):
    """a patch centred on (round(x), round(y)), clipped at the image edges"""
    h, w = img.shape
    x0, y0 = int(round(x)) - 10, int(round(y)) - 10
    xa, xb, ya, yb = max(x0, 0), min(x0 + 21, w), max(y0, 0), min(y0 + 21, h)
    if xa < xb and ya < yb:
        img[ya:yb, xa:xb] = tex[ya - y0:yb - y0, xa - x0:xb - x0]


@functools.lru_cache(maxsize=None)
def scene_frames():
    """-> [(left, right)] uint8 [376, 1241], read-only"""
    xs, ys, Z, tex = _scene_patches()
    frames, cam_x = [], 0.0
    for f in range(SCENE_FRAMES):
        L = np.full((SCENE_H, SCENE_W), 110, np.uint8)
        R = L.copy()
        for i in np.argsort(-Z):                  # nearer patches over farther ones
            x = xs[i] - SCENE_FX * cam_x / Z[i]
            _paste(L, tex[i], x, ys[i]), _paste(R, tex[i], x - SCENE_FX * SCENE_B / Z[i], ys[i])
        L.setflags(write=False), R.setflags(write=False)
        frames.append((L, R))
        cam_x += SCENE_STEP if f < SCENE_TURN else -SCENE_STEP
    return frames


BORDER_X, BORDER_Y = 32, 24         # LK_BORDER_X / LK_BORDER_Y of img_kernels.hpp: the physical border of the tracker's pyramid levels


def border_misses(tr, h, w):
    """(level, point) visits of a traced call whose FIRST search region (41 rows x 52 columns from ((inx - 4) & ~3, iny - 4)) reaches over
    the physical border of its level: stagings the kernel must do on its index-reflecting path even with the border on"""
    n = 0
    for l in range(tr["levels"] + 1):
        ran = tr["iters"][l] > 0
        x0, y0 = (tr["first_x"][l] - 4) & ~3, tr["first_y"][l] - 4
        n += int((ran & ((x0 < -BORDER_X) | (x0 + 51 >= w + BORDER_X) | (y0 < -BORDER_Y) | (y0 + 41 > h + BORDER_Y))).sum())
        h, w = (h + 1) // 2, (w + 1) // 2
    return n


def scene_oracle(ocfg, seed=0xF1715):
    """the oracle tracker over the sequence -> (per-frame outputs with the frame's landmarks under "lm", figures).  figures, from the
    oracle alone: frames in state 1; landmark-frames within 16 px of an image edge; landmarks lost at the temporal LK step between two
    tracked frames (status 0, or status 1 and outside the image) and, of these, the ones lost to status 0 -- the temporal LK call
    repeated on the oracle's own landmarks (no pose guess on this rig: the start is the previous position); border_misses() of those
    calls"""
    ref = O.Tracker(ocfg, seed)
    outs, near, lost, lost_status, slow = [], 0, 0, 0, 0
    prev = None
    for f, (L, R) in enumerate(scene_frames()):
        if prev is not None and prev["state"] == 1 and len(prev["lm"]["p2d"]):
            pp = prev["lm"]["p2d"].astype(np.float32)
            assert np.array_equal(pp.astype(np.float64), prev["lm"]["p2d"])
            o, st, tr = O.lk_trace(scene_frames()[f - 1][0], L, pp, pp, max_level=10)
            slow += border_misses(tr, SCENE_H, SCENE_W)
            inside = (o[:, 0] > 0) & (o[:, 1] > 0) & (o[:, 0] < SCENE_W - 1) & (o[:, 1] < SCENE_H - 1)
            survivors, n_st0 = int(((st == 1) & inside).sum()), int((st == 0).sum())
        else:
            survivors = n_st0 = None
        w = ref.image(0.1 * f, L, R)
        w["lm"] = ref.landmarks()
        if survivors is not None:
            assert survivors == w["dbg"][0], (f, survivors, w["dbg"])          # (the repeated call is the tracker's own)
            lost += prev["n_landmarks"] - survivors
            lost_status += n_st0
        if w["state"] == 1:
            p = w["lm"]["p2d"]
            near += int(((p[:, 0] < 16) | (p[:, 0] > SCENE_W - 1 - 16) | (p[:, 1] < 16) | (p[:, 1] > SCENE_H - 1 - 16)).sum())
        outs.append(w)
        prev = w
    fig = dict(state1=sum(w["state"] == 1 for w in outs), near_edge=near, lost_at_lk=lost, lost_to_status=lost_status, border_misses=slow,
               landmarks=[w["n_landmarks"] for w in outs])
    return outs, fig
