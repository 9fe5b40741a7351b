"""GPU (-m gpu, MI355X): the pyramidal Lucas-Kanade kernel at its border, restage, flat and contrast edges, through flvis_hip_lk_track, bit
for bit against the CPU oracle (oracle/ref_image.cpp::calc_optical_flow_pyr_lk).  The inputs and what the oracle says about them come
from tests/_lk_edges.py, whose recipes check themselves with the oracle's trace (tests/test_lk_edges_inputs.py runs them without a GPU).

There is no tolerance anywhere: status bytes equal, positions equal as uint32, and every slot at or behind a stream's count still holds
what the caller put there."""
import numpy as np
import pytest

import _lk_edges as E

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


def track(ctx, streams, nmax, counts=None):
    """one flvis_hip_lk_track call.  streams: [(case, k)]: stream s tracks the first k points of its case, repeated cyclically when k
    exceeds the case's points; counts: what the call is told (default: k; more than nmax is the kernel's to clamp).
    -> (out [n_img, nmax, 2], status [n_img, nmax], init as passed)"""
    c0 = streams[0][0]
    n_img = len(streams)
    assert all(c.prev.shape == c0.prev.shape and c.kw == c0.kw for c, _ in streams) and all(k <= nmax for _, k in streams)
    pp = np.zeros((n_img, nmax, 2), np.float32)
    init = _sentinel(n_img, nmax)
    for s, (c, k) in enumerate(streams):
        idx = np.arange(k) % max(c.n, 1)
        pp[s, :k], init[s, :k] = c.pts[idx], c.init[idx]
    cnt = np.array([k for _, k in streams] if counts is None else counts, np.int32)
    out, st = ctx.lk_track(_cuda(np.stack([c.prev for c, _ in streams])), _cuda(np.stack([c.nxt for c, _ in streams])), _cuda(pp), _cuda(init),
                           _cuda(cnt), **c0.kw)
    ctx.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), init


def check(streams, res, what=""):
    """every stream against the single-stream oracle answer of its case"""
    out, st, init = res
    for s, (c, k) in enumerate(streams):
        idx = np.arange(k) % max(c.n, 1)
        where = (what, "stream %d" % s, c.name)
        bad = np.nonzero(st[s, :k] != c.st[idx])[0]
        assert len(bad) == 0, (where, "status", "first differing point %d of %d" % (bad[0], k), int(st[s, bad[0]]), c.pts[idx[bad[0]]], c.init[idx[bad[0]]])
        g, w = out[s, :k].view(np.uint32), c.out[idx].view(np.uint32)
        bad = np.nonzero((g != w).any(1))[0]
        assert len(bad) == 0, (where, "position", "%d of %d points differ, the first at %d" % (len(bad), k, bad[0]), out[s, bad[0]], c.out[idx[bad[0]]],
                               [E.O.LK_CAUSES[v] for v in c.tr["cause"][:, idx[bad[0]]]], c.tr["iters"][:, idx[bad[0]]])
        assert np.array_equal(out[s, k:].view(np.uint32), init[s, k:].view(np.uint32)), (where, "a slot behind the count was written")
        assert not st[s, k:].any(), (where, "a status behind the count was written")


@pytest.mark.parametrize("names", E.BATCHES, ids=lambda names: "+".join(names) if len(names) < 3 else "%s..%s" % (names[0], names[-1]))
def test_recipes_bit_exact(ctx, names):
    """every recipe; those of one image size and one parameter set in one call, each stream with its own count"""
    cs = [E.case(n) for n in names]
    streams = [(c, c.n) for c in cs]
    nmax = max(c.n for c in cs) + 3
    check(streams, track(ctx, streams, nmax), "+".join(names))


# the eight recipes of the 120 x 160 / max_level 0 batch: restage-heavy, rim and step-out points, 24 to 204 points each
SHAPE_CASES = E.BATCHES[0]


@pytest.mark.parametrize("n_img", [1, 3, 8])
@pytest.mark.parametrize("nmax", [8, 127, 128, 513, 600])
def test_launch_shapes(ctx, nmax, n_img):
    """grid = min(nmax, 512) x n_img workgroups: multiples of 8 (the XCD renumbering runs; 127 x 8 with an odd width) and others, more
    than 512 points per stream (a second trip of the stride loop), counts that fill nmax, of 1 and of 0, and counts above nmax (clamped).
    Whatever the grid, every stream's result is the single-stream oracle's."""
    assert len(SHAPE_CASES) == 8
    cs = [E.case(n) for n in SHAPE_CASES]
    want = [nmax + 5, 1, 0, nmax, nmax // 2, nmax - 1, 3, nmax][:n_img]
    for shift in (0, 1):                                   # (twice, so that n_img = 1 sees a clamped and a single-point count as well)
        told = (want[shift:] + want[:shift])
        streams = [(cs[(s + shift) % 8], min(k, nmax)) for s, k in enumerate(told)]
        check(streams, track(ctx, streams, nmax, counts=told), "nmax %d n_img %d counts %s" % (nmax, n_img, told))


def test_repeated_calls_reuse_the_scratch_pyramids(ctx):
    """the far_start batch twice in one context, another image size in between: identical bits"""
    cs = [E.case(n) for n in E.BATCHES[0][:4]]
    streams = [(c, c.n) for c in cs]
    a = track(ctx, streams, 160)
    small = E.case("tiny_33x47")
    check([(small, small.n)], track(ctx, [(small, small.n)], small.n), "in between")
    b = track(ctx, streams, 160)
    check(streams, a, "first"), check(streams, b, "second")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


# ---- the tracker's own LK launches: cached templates, templates ahead, bordered pyramids -------------------------------------------------
def _kitti_cfgs():
    import ctypes as C
    import os
    import tempfile
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_lk_edges_kitti_like_gpu.yaml")
    open(p, "w").write(synth.KITTI_LIKE_YAML)
    cfg = flvis_amd.load_config(p)
    ocfg = E.O.RefConfig()
    assert C.sizeof(ocfg) == C.sizeof(cfg)
    C.memmove(C.byref(ocfg), C.byref(cfg), C.sizeof(cfg))          # identical layout: both sides get the same numbers
    return cfg, ocfg


def _run_scene(ctx, cfg, env, monkeypatch):
    """the crafted sequence through one tracker created under `env` -> (per frame: output + landmarks, debug counters)"""
    import ctypes as C
    import torch
    import flvis_amd
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    trk = flvis_amd.Tracker(ctx, cfg, 1, seed_base=0xF1715)           # (the knobs are read here)
    ctx._check(ctx._lib.flvis_debug_lk_stats(ctx._h, 1), "lk_stats")
    rec = []
    for f, (L, R) in enumerate(E.scene_frames()):
        got = trk.image_feed(torch.from_numpy(L[None].copy()).cuda(), torch.from_numpy(R[None].copy()).cuda(), [0.1 * f], with_local_map=False)[0]
        got["lm"] = trk.landmarks(0)
        rec.append(got)
    dbg = (C.c_int64 * 64)()
    ctx._check(ctx._lib.flvis_debug_counters(ctx._h, dbg), "debug_counters")
    ctx._check(ctx._lib.flvis_debug_lk_stats(ctx._h, 0), "lk_stats")
    del trk
    return rec, [int(v) for v in dbg]


def test_tracker_lk_launches_on_landmarks_that_cross_the_image_edges(ctx, monkeypatch):
    """The temporal launch with cached templates and the stereo launch that stores them have no entry of their own: a crafted stereo
    sequence whose landmarks approach, hang over and leave the left and right image edges (tests/_lk_edges.py; what the oracle says about
    it is pinned in tests/test_lk_edges_inputs.py) runs through the tracker.  Every frame is in lockstep with the oracle tracker, whatever
    the template cache and the pyramid border are set to, and the cached and the slow staging paths were both taken."""
    cfg, ocfg = _kitti_cfgs()
    want, fig = E.scene_oracle(ocfg)
    assert fig["state1"] >= 10 and fig["near_edge"] >= 30 and fig["lost_to_status"] >= 10, fig
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
    # a region that reaches over the physical border is staged by the reflecting path, border or not: at least the first regions of the
    # temporal launch that the oracle's trace counts
    assert cached[62] + cached[63] > 0 and cached[63] >= fig["border_misses"] > 0, (cached[61:64], fig)
    assert plain[62] + plain[63] > cached[62] + cached[63], (cached[61:64], plain[61:64])
