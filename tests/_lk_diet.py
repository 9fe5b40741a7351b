"""Inputs for what a cut in the instruction count of the Lucas-Kanade iteration (flvis_amd/csrc/lk_kernel.hip) can break and
tests/_lk_edges.py does not pin, with the CPU oracle's answer and trace for each (the Case of _lk_edges.py).  tests/test_lk_diet_inputs.py
checks every recipe with the oracle alone, tests/test_gpu_lk_diet.py compares the kernel against them bit for bit.

1. Bilinear weights at the corners of the unit square on saturated pixels.  The kernel interpolates a pixel as
   acc = w00 p00 + w01 p01 + w10 p10 + w11 p11 + 2^8 with 14-bit weights, w11 = 2^14 - (w00 + w01 + w10), and takes acc >> 9 as a packed
   16-bit logical shift of bytes 1..2 of acc: right only while 0 <= acc < 2^24.  The recipes put the sub-pixel parts on 0, the smallest
   part a float32 coordinate next to 15 can have (2^-20), 2^-15, 1/2 -+ 2^-20, 1 - 2^-15 and 1 - 2^-20, in both axes, plus two pairs of
   parts at which the three rounded weights sum to 2^14 + 1 and w11 comes out -1, on images that are 255 everywhere, 0 everywhere, a 0 / 255
   checkerboard and single 255 pixels on 0 (a quad (0, 0, 0, 255) under w11 = -1 gives the smallest acc there is, 2^8 - 255 = 1; 255
   everywhere gives the largest, 255 * 2^14 + 2^8).
2. Every way out of the iteration loop in ONE call of two streams with different counts: converged (eps test), oscillation, iterations
   exhausted, left the image mid-iteration, flat template -- so that neighbouring waves take the wave-uniform branches differently.

Images are the smallest that hold one window: 32 x 32 and 40 x 64."""
import functools

import numpy as np

import _lk_edges as E
import _oracle as O
import _synth as S

f32 = np.float32
ULP = f32(2.0 ** -20)            # of a float32 coordinate in [8, 16): the smallest sub-pixel part a window start next to 0 can have
# sub-pixel parts, as (window start) - floor(window start): the point is 15 + part, exact in float32
PARTS = (f32(0), ULP, f32(2.0 ** -15), f32(0.5) - ULP, f32(0.5) + ULP, f32(1) - f32(2.0 ** -15), f32(1) - ULP)
# pairs (a, b) at which the fourth weight comes out -1 (found by search; weights() below says so again)
MINUS_ONE = ((f32(1583) * ULP, f32(2214) * ULP), (f32(2416) * ULP, f32(4846) * ULP))


def weights(a, b):
    """the four 14-bit weights of sub-pixel part (a, b), float32 arithmetic and round-to-nearest-even as the kernel and the oracle do it"""
    a, b, one, s = f32(a), f32(b), f32(1), f32(16384)
    w00, w01, w10 = (int(np.rint((one - a) * (one - b) * s)), int(np.rint(a * (one - b) * s)), int(np.rint((one - a) * b * s)))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def part_pairs():
    """every pair of PARTS and the two MINUS_ONE pairs -> [n, 2] float32"""
    p = [(a, b) for b in PARTS for a in PARTS] + list(MINUS_ONE)
    return np.array(p, f32)


def checker(h, w, cell):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // cell) + (y // cell)) % 2) * 255).astype(np.uint8)


def dots(h, w):
    """255 at the pixels with odd x and odd y on 0: under a window that starts on an even pixel every other quad is (0, 0, 0, 255)"""
    y, x = np.mgrid[0:h, 0:w]
    return (((x % 2) & (y % 2)) * 255).astype(np.uint8)


def image(kind, h, w):
    return {"255": np.full((h, w), 255, np.uint8), "0": np.zeros((h, w), np.uint8), "chk1": checker(h, w, 1), "chk3": checker(h, w, 3),
            "dots": dots(h, w), "tex": S.texture_u8(h, w, 410 + h)}[kind]


SIZES = ((32, 32), (40, 64))


def corner_case(tmpl, search, h, w, max_level):
    """template image `tmpl`, search image `search`; a point per pair of parts with its window start at (a, b) (only next to 0 does a
    float32 coordinate have parts this small: on 32 x 32 the window covers the image, on 40 x 64 its upper left); the start positions
    carry the pairs in reverse order, so template and search weights differ.  A second half repeats the points with start = point (the first iteration interpolates at the very part)."""
    x0, y0 = 0, 0
    pp = part_pairs()
    pts = pp + np.array([15 + x0, 15 + y0], f32)
    assert np.array_equal((pts - np.array([15 + x0, 15 + y0], f32)), pp)                  # (the parts survive the float32 coordinate)
    init = np.concatenate([pts[::-1], pts])
    pts = np.concatenate([pts, pts])
    c = E.Case("corner_%s_%s_%dx%d_l%d" % (tmpl, search, h, w, max_level), image(tmpl, h, w), image(search, h, w), pts, init, max_level=max_level)
    c.tmpl, c.search = tmpl, search
    return c


# (template, search): a textured template against saturated search images iterates; a saturated template is rejected as flat after its
# template was interpolated (the template path's accumulator); chk1's Scharr derivative is 0 everywhere (period 2): flat as well
CORNER_PAIRS = (("tex", "255"), ("tex", "0"), ("tex", "chk1"), ("tex", "dots"), ("chk3", "chk3"), ("chk3", "255"), ("chk3", "dots"),
                ("255", "255"), ("0", "0"), ("chk1", "chk1"), ("255", "chk1"), ("0", "dots"))
ITERATES = ("tex", "chk3")


def corner_check(c):
    """every point is visited: a textured template iterates at level 0 (at least once, from the start it was given), a saturated one is
    taken, found flat and dropped"""
    assert c.levels == 0 and c.n == 2 * (len(PARTS) ** 2 + len(MINUS_ONE)) <= 120, (c.name, c.levels, c.n)
    if c.tmpl in ITERATES:
        assert (c.tr["iters"][0] >= 1).all() and (c.tr["cause"][0] != E.CAUSE["flat"]).all(), (c.name, c.tr["cause"][0])
    else:
        assert (c.tr["cause"][0] == E.CAUSE["flat"]).all() and not c.st.any(), (c.name, c.tr["cause"][0])
    return c


def first_visit_acc(c):
    """(smallest, largest) accumulator of the FIRST iteration's interpolation over all points of a case that iterates, recomputed here
    from the start positions (31 x 31 window from floor(start - 15), weights(); the image reflected as BORDER_REFLECT_101)"""
    h, w = c.nxt.shape
    big = np.pad(c.nxt.astype(np.int64), 40, mode="reflect")
    lo, hi = 1 << 30, -(1 << 30)
    for x, y in c.init:
        sx, sy = f32(x) - f32(15), f32(y) - f32(15)
        ix, iy = int(np.floor(sx)), int(np.floor(sy))
        w00, w01, w10, w11 = weights(sx - f32(ix), sy - f32(iy))
        win = big[40 + iy:40 + iy + 32, 40 + ix:40 + ix + 32]
        acc = w00 * win[:31, :31] + w01 * win[:31, 1:] + w10 * win[1:, :31] + w11 * win[1:, 1:] + 256
        lo, hi = min(lo, int(acc.min())), max(hi, int(acc.max()))
    return lo, hi


# ---- exits: every way out of the iteration loop in one call ------------------------------------------------------------------------------
EXIT_KW = dict(max_level=1, max_iter=10, eps=1e-4)
EXIT_CAUSES = ("converged", "oscillation", "exhausted", "left_image", "flat")


def exits_case(which):
    """40 x 64, eps small enough that steps which cancel end a point before the eps test does.  Stream "a": a texture pair 5.3 px apart,
    starts displaced by up to 9 px, and twelve points whose search window starts 2-3 px inside the right threshold (the first step leads
    outside); stream "b": a texture beside a flat third, on a 2.6 px shift, fewer points (flat templates among them)."""
    h, w = 40, 64
    rng = np.random.default_rng(420 + (which == "b"))
    if which == "a":
        prev, nxt = S.shifted_pair(h, w, 421, 5.3, 0.6, margin=16)
        pts = E.grid(h, w, 5, 2.5, 3.25)
        init = pts + rng.uniform(-9, 9, pts.shape).astype(f32)
        t = f32(6.25) + f32(2.5) * np.arange(12, dtype=f32)
        pts = np.concatenate([pts, np.stack([np.full(12, w - 26.0, f32), t], 1)])
        init = np.concatenate([init, np.stack([f32(w + 15 - 2.5) - f32(0.25) * (np.arange(12) % 4).astype(f32), t], 1)])
    else:
        prev, nxt = S.shifted_pair(h, w, 422, -2.6, 0.4, margin=16)
        prev, nxt = prev.copy(), nxt.copy()
        prev[:, :24] = 90
        nxt[:, :24] = 90
        pts = E.grid(h, w, 7, 3.5, 4.75)
        init = pts + rng.uniform(-5, 5, pts.shape).astype(f32)
    return E.Case("exits_" + which, prev, nxt, pts, init, **EXIT_KW)


def exit_counts(c):
    return {k: int((c.tr["cause"][0] == E.CAUSE[k]).sum()) for k in EXIT_CAUSES}


def exits_check(c):
    assert c.levels == 0 and c.n <= 200, (c.name, c.levels, c.n)
    return c


RECIPES = {
    **{"corner_%s_%s_%dx%d_l%d" % (t, s, h, w, lvl): (lambda t=t, s=s, h=h, w=w, lvl=lvl: corner_check(corner_case(t, s, h, w, lvl)))
       for (t, s) in CORNER_PAIRS for (h, w), lvl in zip(SIZES, (0, 1))},
    "exits_a": lambda: exits_check(exits_case("a")),
    "exits_b": lambda: exits_check(exits_case("b")),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return RECIPES[name]()


# one call per image size for the corner recipes (12 streams, the same count: every stream's points are the same pairs of parts -- the
# ragged counts are the exits batch's), one call for the two exit streams
BATCHES = tuple(tuple("corner_%s_%s_%dx%d_l%d" % (t, s, h, w, lvl) for (t, s) in CORNER_PAIRS) for (h, w), lvl in zip(SIZES, (0, 1))) + (
    ("exits_a", "exits_b"),)


# ---- a crafted stereo sequence of saturated patches for the tracker's own LK launches (cached templates, bordered pyramids) -------------
# The sequence of tests/_lk_edges.py (same rig, same motion) with every patch binary 0 / 255 in 1-, 2- and 3-px cells on a background that
# is 255 on the left half of the image and 0 on the right half: the temporal launch (templates from the cache) and the stereo launch (which
# stores them) interpolate saturated pixels under whatever sub-pixel parts the landmarks take.
@functools.lru_cache(maxsize=None)
def scene_frames():
    xs, ys, Z, _ = E._scene_patches()
    rng = np.random.default_rng(430)
    tex = [np.kron((rng.integers(0, 2, (21, 21)) * 255).astype(np.uint8), np.ones((c, c), np.uint8))[:21, :21] for c in (1 + np.arange(len(xs)) % 3)]
    frames, cam_x = [], 0.0
    for f in range(E.SCENE_FRAMES):
        L = np.zeros((E.SCENE_H, E.SCENE_W), np.uint8)
        L[:, :E.SCENE_W // 2] = 255
        R = L.copy()
        for i in np.argsort(-Z):
            x = xs[i] - E.SCENE_FX * cam_x / Z[i]
            E._paste(L, tex[i], x, ys[i]), E._paste(R, tex[i], x - E.SCENE_FX * E.SCENE_B / Z[i], ys[i])
        L.setflags(write=False), R.setflags(write=False)
        frames.append((L, R))
        cam_x += E.SCENE_STEP if f < E.SCENE_TURN else -E.SCENE_STEP
    return frames


def scene_oracle(ocfg, seed=0xF1715):
    """the oracle tracker over the saturated sequence -> (per-frame outputs with the frame's landmarks under "lm", figures: frames in
    state 1, the landmark count per frame, the share of saturated pixels (0 or 255) in the left images)"""
    ref = O.Tracker(ocfg, seed)
    outs = []
    for f, (L, R) in enumerate(scene_frames()):
        w = ref.image(0.1 * f, L, R)
        w["lm"] = ref.landmarks()
        outs.append(w)
    sat = float(np.mean([((L == 0) | (L == 255)).mean() for L, _ in scene_frames()]))
    return outs, dict(state1=sum(w["state"] == 1 for w in outs), landmarks=[w["n_landmarks"] for w in outs], saturated=sat)
