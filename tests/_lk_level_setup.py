"""Inputs for what the Lucas-Kanade template cache hands from the stereo launch to the temporal launch (flvis_amd/csrc/lk_kernel.hip: the
floats A11, A12, A22, D, minEig, 1 / D of a level instead of its three Hessian sums), with what the CPU oracle says about them.

A stereo sequence on the KITTI-like rig of tests/_lk_edges.py (same patch positions, depths and camera motion) whose patches are chosen
for the Hessian of the templates the tracker's landmarks get:

  kind 0  a 1-px checkerboard of 0 / 255: the largest derivative magnitudes at the patch rim (the int64 -> float rounding of the sums)
          and none inside (Scharr of a period-2 pattern is 0); its pyramid levels are 127.5 rounded, next to the background's 128, so the
          coarse levels see gradients of a gray value or two: templates next to the min_eig threshold, and flat ones
  kind 1  3-px stripes along x - y = const: I = f(x - y), so Ix = f' and Iy = -f' and every product Ix Iy is <= 0: a negative A12
  kind 2  random binary 0 / 255 cells (what the tracker holds on to)
  kind 3  random gray

in an image `w` pixels wide: 1241 (rows not dword aligned: the tracker copies both images, level-0 pitch 1248, no multiple of 64) or 1248
(the right image is read in place through the indirect level-0 slot).

The oracle's LK takes min_eig as an argument, so on which side of a threshold a template lies is found on the CPU: a (level, point) visit
that is flat at min_eig and not at min_eig / K lies within a factor K below the threshold, one that is not flat at min_eig and flat at
K min_eig within a factor K above it."""
import functools

import numpy as np

import _lk_edges as E
import _oracle as O

FRAMES = 6
BG = 128
MIN_EIG = 1e-4
WIDTHS = (1241, 1248)


def _texture(kind, rng):
    y, x = np.mgrid[0:21, 0:21]
    if kind == 0:
        return (((x + y) % 2) * 255).astype(np.uint8)
    if kind == 1:
        return ((((x - y + 42) // 3) % 2) * 255).astype(np.uint8)
    if kind == 2:
        return (rng.integers(0, 2, (21, 21)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (21, 21)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene_frames(w):
    """-> [(left, right)] uint8 [376, w], read-only; kinds[i] of patch i"""
    xs, ys, Z, _ = E._scene_patches()
    rng = np.random.default_rng(520)
    tex = [_texture(i % 4, rng) for i in range(len(xs))]
    frames, cam_x = [], 0.0
    for f in range(FRAMES):
        L = np.full((E.SCENE_H, w), BG, np.uint8)
        R = L.copy()
        for i in np.argsort(-Z):
            x = xs[i] - E.SCENE_FX * cam_x / Z[i]
            E._paste(L, tex[i], x, ys[i]), E._paste(R, tex[i], x - E.SCENE_FX * E.SCENE_B / Z[i], ys[i])
        L.setflags(write=False), R.setflags(write=False)
        frames.append((L, R))
        cam_x += E.SCENE_STEP if f < E.SCENE_TURN else -E.SCENE_STEP
    return frames


def a12_estimate(img, pts):
    """sum of Scharr dx * dy over the 31 x 31 window around each point (integer window, no interpolation), as a fraction of
    sqrt(sum dx^2 * sum dy^2): the sign and rough size of A12 at level 0"""
    I = np.pad(img.astype(np.int64), 20, mode="reflect")
    dx = 3 * (I[:-2, 2:] - I[:-2, :-2]) + 10 * (I[1:-1, 2:] - I[1:-1, :-2]) + 3 * (I[2:, 2:] - I[2:, :-2])
    dy = 3 * (I[2:, :-2] - I[:-2, :-2]) + 10 * (I[2:, 1:-1] - I[:-2, 1:-1]) + 3 * (I[2:, 2:] - I[:-2, 2:])
    out = []
    for x, y in pts:
        x0, y0 = int(np.floor(x)) - 15 + 19, int(np.floor(y)) - 15 + 19          # (dx[r, c] is the derivative at padded (r + 1, c + 1))
        a, b = dx[y0:y0 + 31, x0:x0 + 31], dy[y0:y0 + 31, x0:x0 + 31]
        out.append(float((a * b).sum()) / max(1.0, float(np.sqrt(float((a * a).sum()) * float((b * b).sum())))))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def scene_oracle(w, ocfg_bytes, seed=0xF1715, factor=1.1, skip=-1):
    """the oracle tracker over the sequence -> (per-frame outputs with the frame's landmarks under "lm", figures).  Figures, from the
    temporal LK call repeated on the oracle's own landmarks (the templates the cache hands over) at min_eig, min_eig / factor and
    min_eig * factor: visits that are flat with all-zero sums (D = 0), flat with non-zero sums, within `factor` below / above the min_eig
    threshold, the largest Hessian sum, landmarks with a clearly negative A12 estimate, first search regions that reach over the physical
    border of their level (E.border_misses).  skip: a frame the stream does not get (its entry of the outputs is None)."""
    import ctypes as C
    ocfg = O.RefConfig()
    C.memmove(C.byref(ocfg), ocfg_bytes, C.sizeof(ocfg))
    ref = O.Tracker(ocfg, seed)
    frames = scene_frames(w)
    outs, prev, prev_f = [], None, -1
    fig = dict(flat_zero=0, flat_nonzero=0, below=0, above=0, max_sum=0, neg_a12=0, visits=0, border_misses=0)
    for f, (L, R) in enumerate(frames):
        if f == skip:
            outs.append(None)
            continue
        if prev is not None and prev["state"] == 1 and len(prev["lm"]["p2d"]):
            pp = prev["lm"]["p2d"].astype(np.float32)
            P = frames[prev_f][0]
            tr = {m: O.lk_trace(P, L, pp, pp, max_level=10, min_eig=m)[2] for m in (MIN_EIG, MIN_EIG / factor, MIN_EIG * factor)}
            t = tr[MIN_EIG]
            flat = t["cause"] == E.CAUSE["flat"]
            zero = (t["a11"] == 0) & (t["a22"] == 0)
            fig["visits"] += int((t["cause"] != E.CAUSE["not_visited"]).sum())
            fig["flat_zero"] += int((flat & zero).sum())
            fig["flat_nonzero"] += int((flat & ~zero).sum())
            fig["below"] += int((flat & (tr[MIN_EIG / factor]["cause"] != E.CAUSE["flat"])).sum())
            # (a visit that is flat only at the higher threshold; visited at all there: a level's start does not depend on min_eig at the
            # top level, and below it a changed path shows as another cause, not as "flat")
            fig["above"] += int((~flat & (t["cause"] != E.CAUSE["not_visited"]) & (tr[MIN_EIG * factor]["cause"] == E.CAUSE["flat"])).sum())
            fig["max_sum"] = max(fig["max_sum"], int(t["a11"].max()), int(t["a22"].max()))
            fig["neg_a12"] += int((a12_estimate(P, pp) < -0.2).sum())
            fig["border_misses"] += E.border_misses(t, E.SCENE_H, w)
        wv = ref.image(0.1 * f, L, R)
        wv["lm"] = ref.landmarks()
        outs.append(wv)
        prev, prev_f = wv, f
    fig["state1"] = sum(o is not None and o["state"] == 1 for o in outs)
    fig["landmarks"] = [o["n_landmarks"] for o in outs if o is not None]
    return outs, fig
