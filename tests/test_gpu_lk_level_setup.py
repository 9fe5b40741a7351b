"""GPU (-m gpu, MI355X): what a pyramid level's set-up in the Lucas-Kanade kernels (flvis_amd/csrc/lk_kernel.hip) can break -- the level
descriptors, the level scale, the fixed lane maps of the two staging fast paths and the floats the template cache hands from the stereo
launch to the temporal launch -- bit for bit against the CPU oracle.

* levels: one flvis_hip_lk_track call per max_level 0, 1, 3 and LK_MAX_LEVELS - 1 on 96 x 128 images;
* staging: points whose template patch (36 x 34 from (ipx - 1, ipy - 1)) and first search region (52 x 41 from ((inx - 4) & ~3, iny - 4))
  start on the first and the last position the fast-path tests admit on each side of an image without a border, one pixel beyond each
  (the index-reflecting path), and on every column residue mod 4;
* the tracker's own launches on the sequence of tests/_lk_level_setup.py, whose patches are chosen for the templates the cache hands over
  (1-px checkerboards of 0 / 255, stripes with a negative A12, flat levels with D = 0, levels next to min_eig on either side): two streams
  of one tracker, one absent for a frame (the streams' slots then differ), on the rig that copies both images (pitch 1248, no multiple of
  64) and on the one that reads the right image in place (indirect level 0); cache and border on and off; every frame in lockstep with
  the oracle; the debug counters say that cached templates were taken in every frame after the first and that both staging paths ran.

The stand-alone entry has neither a physical border nor the staging counters (both belong to the tracker), and the tracker's points are
its own landmarks, which cannot be placed: the corner positions are therefore placed on a border-less image (where X0 = 0 is X0 = -bx),
and the bordered pyramids are checked through the tracker, whose slow-region counter is held against the oracle's count of regions that
reach over the physical border.

No tolerance anywhere: status bytes equal, positions equal as uint32."""
import numpy as np
import pytest

import _lk_edges as E
import _lk_level_setup as T
import _synth as S
from test_gpu_lk_diet import check, ctx, track  # noqa: F401  (ctx: the module-scoped fixture)

pytestmark = pytest.mark.gpu

f32 = np.float32
H, W = 96, 128
LK_MAX_LEVELS = 6          # img_kernels.hpp


# ---- levels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_level", (0, 1, 3, LK_MAX_LEVELS - 1))
def test_levels_bit_exact(ctx, max_level):
    """corners of a 96 x 128 texture pair, starts displaced by up to 6 px, two streams with different counts in one call.  On an image this
    small the pyramid has two levels (a level below 32 px cannot hold a window), so max_level 3 and LK_MAX_LEVELS - 1 cover the host-side
    clamp only; the descriptors of levels 2 and 3 are read by the tracker tests below (376 x 1241: levels 0 .. 3)."""
    prev, nxt, pts = E._texture_pair(seed=500, dx=1.7, dy=-1.2, h=H, w=W, npts=70)
    init = pts + np.random.default_rng(501 + max_level).uniform(-6, 6, pts.shape).astype(f32)
    a = E.Case("levels_a_l%d" % max_level, prev, nxt, pts, init, max_level=max_level)
    b = E.Case("levels_b_l%d" % max_level, nxt, prev, pts[::-1], pts[::-1], max_level=max_level)
    assert a.levels == min(max_level, 1) and a.n >= 40, (a.levels, a.n)      # (96 rows: level 2 would be below the 32 px a window needs)
    streams = [(a, a.n), (b, b.n - 7)]
    check(streams, track(ctx, streams, a.n + 2), "max_level %d" % max_level)


# ---- staging -----------------------------------------------------------------------------------------------------------------------------
# Without a border the patch takes the fast path when 0 <= X0, X0 + 39 < W, 0 <= Y0, Y0 + 34 <= H, the region when 0 <= RX0, RX0 + 51 < W,
# 0 <= RY0, RY0 + 41 <= H.  Window starts ipx = X0 + 1 and inx (RX0 = (inx - 4) & ~3) below; the point is start + 15 + a sub-pixel part.
PATCH_X = (-1, 0, 1, 2, 3, 4, W - 40, W - 39)            # X0: one beyond, first, residues 1 2 3 0, last, one beyond
PATCH_Y = (-1, 0, 1, H - 34, H - 33)
REGION_INX = (3, 4, 5, 6, 7, 8, W - 52 + 4, W - 52 + 7, W - 52 + 8)   # RX0 = -4 | 0 0 0 0 4 | W - 52 (last) twice | W - 48 (beyond)
REGION_INY = (3, 4, 5, H - 41 + 4, H - 41 + 5)                        # RY0 = -1, 0, 1, H - 41 (last), H - 40 (beyond)


def staging_case(max_level):
    prev, nxt = S.shifted_pair(H, W, 510, 0.8, -0.6, margin=16)
    mid_x, mid_y = 40, 30
    starts = [(x + 1, mid_y) for x in PATCH_X] + [(mid_x, y + 1) for y in PATCH_Y] + [(x, mid_y + 1) for x in REGION_INX] + \
             [(mid_x + 1, y) for y in REGION_INY] + [(x + 1, y + 1) for x in (PATCH_X[0], PATCH_X[1], PATCH_X[-2], PATCH_X[-1])
                                                     for y in (PATCH_Y[0], PATCH_Y[1], PATCH_Y[-2], PATCH_Y[-1])] + \
             [(x, y) for x in (REGION_INX[0], REGION_INX[1], REGION_INX[-2], REGION_INX[-1])
              for y in (REGION_INY[0], REGION_INY[1], REGION_INY[-2], REGION_INY[-1])]
    pts = np.array(starts, f32) + f32(15) + np.array([0.37, 0.61], f32)
    assert np.array_equal(np.floor(pts - f32(15)).astype(int), np.array(starts))
    return E.Case("staging_l%d" % max_level, prev, nxt, pts, pts, max_level=max_level)


def staging_paths(c):
    """(patches on the fast path, on the slow path, first regions on the fast path, on the slow path) at level 0, from the oracle's trace"""
    ipx, ipy = np.floor(c.pts[:, 0] - f32(15)).astype(int) - 1, np.floor(c.pts[:, 1] - f32(15)).astype(int) - 1
    pf = (ipx >= 0) & (ipx + 39 < W) & (ipy >= 0) & (ipy + 34 <= H)
    ran = c.tr["iters"][0] > 0
    rx, ry = (c.tr["first_x"][0] - 4) & ~3, c.tr["first_y"][0] - 4
    rf = (rx >= 0) & (rx + 51 < W) & (ry >= 0) & (ry + 41 <= H)
    return int(pf.sum()), int((~pf).sum()), int((ran & rf).sum()), int((ran & ~rf).sum())


@pytest.mark.parametrize("max_level", (0, 1))
def test_staging_corners_bit_exact(ctx, max_level):
    c = staging_case(max_level)
    pf, ps, rf, rs = staging_paths(c)
    assert min(pf, ps, rf, rs) >= 8, (pf, ps, rf, rs)                       # both paths of both stagings are taken
    assert {int(x) & 3 for x in np.floor(c.pts[:, 0] - f32(15)) - 1} == {0, 1, 2, 3}
    streams = [(c, c.n), (c, 5)]
    check(streams, track(ctx, streams, c.n + 1), c.name)


# ---- the tracker's launches: cached floats, both rigs, counters ------------------------------------------------------------------------------
ABSENT = (2, 1)        # (frame, stream) without an image


def _cfgs(w):
    """the KITTI-like rig at image width w: 1241 (both images copied, level-0 pitch 1248) or 1248 (no equalisation and rows of whole
    16-byte groups: the right image is read in place, level 0 of its pyramid through the indirect slot)"""
    import ctypes as C
    import os
    import tempfile
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_lk_level_setup_%d.yaml" % w)
    open(p, "w").write(synth.KITTI_LIKE_YAML.replace("image_width: 1241", "image_width: %d" % w))
    cfg = flvis_amd.load_config(p)
    assert cfg.image_width == w and not cfg.need_equal_hist and ((w & 15) == 0) == (w == 1248)
    return cfg, bytes(C.string_at(C.byref(cfg), C.sizeof(cfg)))


def _oracle(w):
    """stream 0 sees every frame of T.scene_frames(w), stream 1 all but frame ABSENT[0]; seeds as the tracker gives them"""
    _, raw = _cfgs(w)
    return [T.scene_oracle(w, raw, seed=0xF1715 + s, skip=ABSENT[0] if s == ABSENT[1] else -1) for s in range(2)]


def _run_two_streams(ctx, cfg, w, env, monkeypatch):
    import ctypes as C
    import torch
    import flvis_amd
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    trk = flvis_amd.Tracker(ctx, cfg, 2, seed_base=0xF1715)
    ctx._check(ctx._lib.flvis_debug_lk_stats(ctx._h, 1), "lk_stats")
    rec, counters = [], []
    for f, (L, R) in enumerate(T.scene_frames(w)):
        pres = [0 if (f, s) == ABSENT else 1 for s in range(2)]
        outs = trk.image_feed(torch.from_numpy(np.stack([L, L])).cuda(), torch.from_numpy(np.stack([R, R])).cuda(), [0.1 * f] * 2,
                              with_local_map=False, present=pres)
        for s in range(2):
            if pres[s]:
                outs[s]["lm"] = trk.landmarks(s)
        rec.append([outs[s] if pres[s] else None for s in range(2)])
        dbg = (C.c_int64 * 64)()
        ctx._check(ctx._lib.flvis_debug_counters(ctx._h, dbg), "debug_counters")
        counters.append([int(v) for v in dbg])
    ctx._check(ctx._lib.flvis_debug_lk_stats(ctx._h, 0), "lk_stats")
    del trk
    return rec, counters


def test_cache_scene_reaches_its_templates():
    """(no GPU work) what the oracle says about the templates the cache hands over in T.scene_frames, per rig and stream: flat ones with
    D = 0 exactly, flat ones with non-zero sums, one within 10 % on each side of min_eig (the nearest this recipe has: none within 3 %),
    Hessian sums above 2^32 (the int64 -> float conversion rounds), negative A12.  D = 1.1920929e-07 has no template of its own: a level
    that passes min_eig has minEig = lambda_min / 1922 >= 1e-4, so D = lambda_min lambda_max >= 0.19^2 -- only a level that min_eig stops
    anyway can lie below that threshold, and the D = 0 templates are those."""
    for w in T.WIDTHS:
        for s, (_, fig) in enumerate(_oracle(w)):
            print(w, s, fig)
            assert fig["flat_zero"] >= 2 and fig["flat_nonzero"] >= 20 and fig["below"] >= 1 and fig["above"] >= 1, (w, s, fig)
            assert fig["max_sum"] > 1 << 32 and fig["neg_a12"] >= 50 and fig["border_misses"] >= 1, (w, s, fig)
        assert _oracle(w)[0][1]["state1"] == T.FRAMES


@pytest.mark.parametrize("tc,border", (("1", "1"), ("1", "0"), ("0", "1")))
@pytest.mark.parametrize("w", T.WIDTHS)
def test_tracker_cached_floats_two_rigs(ctx, monkeypatch, w, tc, border):
    """Two streams of one tracker on the sequence of tests/_lk_level_setup.py, stream 1 without frame 2 (from then on the streams' image
    slots differ), on the rig that copies both images and on the one that reads the right image in place; cache on / off, border on /
    off; every frame in lockstep with the oracle."""
    cfg, _ = _cfgs(w)
    want = _oracle(w)
    rec, dbg = _run_two_streams(ctx, cfg, w, {"FLVIS_LK_TCACHE": tc, "FLVIS_LK_BORDER": border}, monkeypatch)
    for f in range(T.FRAMES):
        for s in range(2):
            g, wv = rec[f][s], want[s][0][f]
            where = (w, tc, border, "frame %d stream %d" % (f, s))
            assert (g is None) == (wv is None), where
            if wv is None:
                continue
            assert g["state"] == wv["state"] and g["new_keyframe"] == wv["new_keyframe"] and g["n_landmarks"] == wv["n_landmarks"], (where, g, wv)
            assert np.array_equal(g["pose7"], wv["pose7"]), (where, g["pose7"] - wv["pose7"])
            if wv["state"] == 1:
                for k in ("ids", "flags", "p2d", "p2u", "p3w"):
                    assert np.array_equal(g["lm"][k], wv["lm"][k]), (where, k)
    # counter 61: templates taken from the cache (cumulative): in every frame after the first (stream 0 tracks in all of them)
    taken = [d[61] for d in dbg]
    if tc == "1":
        assert all(taken[f] > taken[f - 1] for f in range(1, T.FRAMES)), taken
    else:
        assert taken[-1] == 0, taken
    # Counters 62 / 63: patches / search regions staged by the index-reflecting path.  The fast stagings follow from the visits: every
    # (level, point) visit that iterated staged at least one search region, and every such visit of the stereo launch computed its
    # template from a staged patch -- more visits than slow stagings means that some staging took the fast path.
    it_temporal = sum(dbg[-1][36 + 2 * l + 1] for l in range(6))
    it_stereo = sum(dbg[-1][48 + 2 * l + 1] for l in range(6))
    slow_patches, slow_regions = dbg[-1][62], dbg[-1][63]
    print("visits that iterated: temporal %d, stereo %d; slow patches %d, slow regions %d" % (it_temporal, it_stereo, slow_patches, slow_regions))
    assert it_temporal + it_stereo > slow_regions and it_stereo > slow_patches, dbg[-1][36:64]
    # The slow ones.  With the border on a patch of a point inside the image cannot leave the bordered storage (LK_BORDER_X / LK_BORDER_Y,
    # img_kernels.hpp), and a region does only around a point tracked out of the image: the oracle's trace counts the temporal launch's
    # first regions that reach over the physical border (E.border_misses), each of which the kernel must have staged the slow way.
    misses = sum(fig["border_misses"] for _, fig in want)
    if border == "1":
        assert slow_regions >= misses >= 2, (slow_regions, misses)
    else:
        assert slow_patches > 0 and slow_regions > misses, (slow_patches, slow_regions, misses)
