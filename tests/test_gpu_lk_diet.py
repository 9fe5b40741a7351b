"""GPU (-m gpu, MI355X): the Lucas-Kanade kernel on the inputs of tests/_lk_diet.py -- bilinear weights at the corners of the unit square
on saturated pixels, and every way out of the iteration loop in one call -- through flvis_hip_lk_track, bit for bit against the CPU oracle,
and a sequence of saturated patches through the tracker's own temporal (cached templates) and stereo (stores them) launches, in lockstep
with the oracle tracker.  tests/test_lk_diet_inputs.py checks the inputs without a GPU.

No tolerance anywhere: status bytes equal, positions equal as uint32, slots at or behind a stream's count untouched."""
import numpy as np
import pytest

import _lk_diet as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sentinel(n_img, nmax):
    """start positions of the slots no point owns: distinct finite values no result can equal"""
    return (-7000.0 - np.arange(n_img * nmax * 2, dtype=np.float32) * 0.25).reshape(n_img, nmax, 2)


def track(ctx, streams, nmax):
    """one flvis_hip_lk_track call.  streams: [(case, k)]: stream s tracks the first k points of its case
    -> (out [n_img, nmax, 2], status [n_img, nmax], init as passed)"""
    c0 = streams[0][0]
    n_img = len(streams)
    assert all(c.prev.shape == c0.prev.shape and c.kw == c0.kw for c, _ in streams) and all(k <= min(nmax, c.n) for c, k in streams)
    pp = np.zeros((n_img, nmax, 2), np.float32)
    init = _sentinel(n_img, nmax)
    for s, (c, k) in enumerate(streams):
        pp[s, :k], init[s, :k] = c.pts[:k], c.init[:k]
    cnt = np.array([k for _, k in streams], np.int32)
    out, st = ctx.lk_track(_cuda(np.stack([c.prev for c, _ in streams])), _cuda(np.stack([c.nxt for c, _ in streams])), _cuda(pp), _cuda(init),
                           _cuda(cnt), **c0.kw)
    ctx.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), init


def check(streams, res, what=""):
    """every stream against the single-stream oracle answer of its case"""
    out, st, init = res
    for s, (c, k) in enumerate(streams):
        where = (what, "stream %d" % s, c.name)
        bad = np.nonzero(st[s, :k] != c.st[:k])[0]
        assert len(bad) == 0, (where, "status", "first differing point %d of %d" % (bad[0], k), int(st[s, bad[0]]), c.pts[bad[0]], c.init[bad[0]])
        g, w = out[s, :k].view(np.uint32), c.out[:k].view(np.uint32)
        bad = np.nonzero((g != w).any(1))[0]
        assert len(bad) == 0, (where, "position", "%d of %d points differ, the first at %d" % (len(bad), k, bad[0]), out[s, bad[0]], c.out[bad[0]],
                               c.pts[bad[0]], c.init[bad[0]], D.E.O.LK_CAUSES[c.tr["cause"][0, bad[0]]], c.tr["iters"][0, bad[0]])
        assert np.array_equal(out[s, k:].view(np.uint32), init[s, k:].view(np.uint32)), (where, "a slot behind the count was written")
        assert not st[s, k:].any(), (where, "a status behind the count was written")


@pytest.mark.parametrize("names", D.BATCHES, ids=lambda names: "%s..%s" % (names[0], names[-1]))
def test_recipes_bit_exact(ctx, names):
    """the corner recipes of one image size in one call (twelve streams), the two exit streams in one call with their different counts"""
    cs = [D.case(n) for n in names]
    streams = [(c, c.n) for c in cs]
    check(streams, track(ctx, streams, max(c.n for c in cs) + 3), names[0])


def test_ragged_counts_and_single_points(ctx):
    """the exit streams again with counts that split them elsewhere (a wave's neighbours change), and the corner recipes one point per
    stream: every grid is one wave wide"""
    a, b = D.case("exits_a"), D.case("exits_b")
    for ka, kb in ((a.n, 1), (7, b.n), (64, 33)):
        streams = [(a, ka), (b, kb)]
        check(streams, track(ctx, streams, 128), "counts %d %d" % (ka, kb))
    cs = [D.case(n) for n in D.BATCHES[0]]
    streams = [(c, 1) for c in cs]
    check(streams, track(ctx, streams, 1), "one point per stream")


# ---- the tracker's own LK launches (the helper pattern of tests/test_gpu_lk_edges.py) ----------------------------------------------------
def _kitti_cfgs():
    import ctypes as C
    import os
    import tempfile
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_lk_diet_kitti_like_gpu.yaml")
    open(p, "w").write(synth.KITTI_LIKE_YAML)
    cfg = flvis_amd.load_config(p)
    ocfg = D.O.RefConfig()
    assert C.sizeof(ocfg) == C.sizeof(cfg)
    C.memmove(C.byref(ocfg), C.byref(cfg), C.sizeof(cfg))          # identical layout: both sides get the same numbers
    return cfg, ocfg


def _run_scene(ctx, cfg, env, monkeypatch):
    """the saturated sequence through one tracker created under `env` -> (per frame: output + landmarks, debug counters)"""
    import ctypes as C
    import torch
    import flvis_amd
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    trk = flvis_amd.Tracker(ctx, cfg, 1, seed_base=0xF1715)           # (the knobs are read here)
    ctx._check(ctx._lib.flvis_debug_lk_stats(ctx._h, 1), "lk_stats")
    rec = []
    for f, (L, R) in enumerate(D.scene_frames()):
        got = trk.image_feed(torch.from_numpy(L[None].copy()).cuda(), torch.from_numpy(R[None].copy()).cuda(), [0.1 * f], with_local_map=False)[0]
        got["lm"] = trk.landmarks(0)
        rec.append(got)
    dbg = (C.c_int64 * 64)()
    ctx._check(ctx._lib.flvis_debug_counters(ctx._h, dbg), "debug_counters")
    ctx._check(ctx._lib.flvis_debug_lk_stats(ctx._h, 0), "lk_stats")
    del trk
    return rec, [int(v) for v in dbg]


def test_tracker_lk_launches_on_saturated_patches(ctx, monkeypatch):
    """The temporal launch with cached templates and the stereo launch that stores them are compiled apart from the stand-alone entry:
    the saturated sequence runs through the tracker with the template cache and the pyramid border on and off, every frame in lockstep
    with the oracle tracker, and cached templates were used."""
    cfg, ocfg = _kitti_cfgs()
    want, fig = D.scene_oracle(ocfg)
    assert fig["state1"] >= 10 and min(fig["landmarks"][1:]) >= 40, fig
    runs = {}
    for tc in ("1", "0"):
        runs[tc] = _run_scene(ctx, cfg, {"FLVIS_LK_TCACHE": tc, "FLVIS_LK_BORDER": tc}, monkeypatch)
    for key, (rec, _) in runs.items():
        prev_state = 0
        for f, (g, w) in enumerate(zip(rec, want)):
            where = (key, "frame %d" % f)
            assert g["state"] == w["state"] and g["new_keyframe"] == w["new_keyframe"] and g["n_landmarks"] == w["n_landmarks"], (where, g, w)
            if prev_state == 1:   # the frame ran LKORBTracking::tracking (otherwise the oracle's counters are those of an older frame)
                assert np.array_equal(g["dbg"], w["dbg"]), (where, g["dbg"], w["dbg"])
            assert np.array_equal(g["pose7"], w["pose7"]), (where, g["pose7"] - w["pose7"])
            if w["state"] == 1:
                for k in ("ids", "flags", "p2d", "p2u", "p3w"):
                    assert np.array_equal(g["lm"][k], w["lm"][k]), (where, k)
            prev_state = w["state"]
    cached, plain = runs["1"][1], runs["0"][1]
    assert cached[61] > 0 and plain[61] == 0, (cached[61:64], plain[61:64])        # cached templates were used
