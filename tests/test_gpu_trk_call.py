"""GPU (-m gpu, MI355X): flvis_hip_lkorb_tracking -- LKORBTracking::tracking as one call on caller arrays (tracking_call.hip) -- against the
checker composed in tests/_trk_call.py from the oracle's exported functions (proved on the oracle's own lk_tracking, and every scene on its
edge, by tests/test_trk_call_inputs.py without a GPU).  BIT FOR BIT, no tolerance anywhere: to_from, both point arrays as their uint32
patterns, the flags, mask_F, counts4, every double of pose7, ret.

Every output buffer is filled with a sentinel before the call: rows of `to` from of_inlier_cnt on, mask_F rows the F step did not reach, and
all outputs of a refused call must come back as they went in; pose7 goes in as a pose of its own per set, which a set that ends early hands
back."""
import ctypes as C

import numpy as np
import pytest

import _trk_call as T

pytestmark = pytest.mark.gpu
RIGS = ("rect", "unrect", "depth")


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outputs(call):
    """sentinel-filled device outputs of a call (pose7: each set's pose_in)"""
    import torch
    e = call.expected()
    o = {}
    for k in T.OUT_NAMES:
        if k in ("counts4", "ret", "pose7"):
            continue
        o[k] = _dev(np.full_like(e[k], {"to_from": T.SENT_I, "to_flags": T.SENT_B, "mask_F": T.SENT_B}.get(k, T.SENT_F)))
    o["counts4"] = torch.full(e["counts4"].shape, T.SENT_I, dtype=torch.int32, device="cuda")
    o["ret"] = torch.full(e["ret"].shape, T.SENT_B, dtype=torch.uint8, device="cuda")
    return o


def _run(ctx, call, cfg=None, a=None):
    """one call -> the outputs on the host"""
    a = call.arrays() if a is None else a
    o = _outputs(call)
    pose = _dev(a["pose_in"])
    any_guess = bool(a["use_guess"].any())
    r = ctx.lkorb_tracking(call.rig.lib_cfg() if cfg is None else cfg, _dev(a["img_from"]), _dev(a["img_to"]), _dev(a["p2d"]), _dev(a["p2u"]),
                           _dev(a["p3w"]), _dev(a["flags"]), _dev(a["count"]), a["guess"] if any_guess else None,
                           a["use_guess"] if any_guess else None, pose7=pose, out=o)
    ctx.synchronize()
    return {k: r[k].cpu().numpy() for k in T.OUT_NAMES}


def _differences(call, got):
    e = call.expected()
    bad = []
    for i, s in enumerate(call.sets):
        why = [k for k in T.OUT_NAMES if not np.array_equal(T.raw(got[k][i]), T.raw(e[k][i]))]
        if why:
            bad.append("%s: %s differ; counts %s, checker %s" % (s.name, ", ".join(why), got["counts4"][i].tolist(), e["counts4"][i].tolist()))
    return bad


@pytest.mark.parametrize("kind", RIGS)
def test_edge_scenes_equal_the_checker(ctx, kind):
    """every edge scene of the rig (with and without a guess) but the 1024-landmark one, in one call of mixed branches"""
    S = T.scenes(kind)
    call = T.Call([s for k, s in S.items() if k != "n_1024"])
    got = _run(ctx, call)
    bad = _differences(call, got)
    print("%s: %d sets, %d differ; counts4 %s" % (kind, len(call.sets), len(bad), {s.name: got["counts4"][i].tolist() for i, s in enumerate(call.sets)}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", RIGS)
def test_1024_landmarks(ctx, kind):
    call = T.Call([T.scenes(kind)["n_1024"]])
    assert call.cap == 1024
    bad = _differences(call, _run(ctx, call))
    assert not bad, "\n".join(bad)


def test_640x480(ctx):
    call = T.Call([T.scene_640()])
    got = _run(ctx, call)
    print("counts4", got["counts4"].tolist())
    bad = _differences(call, got)
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module")
def batch(ctx):
    call = T.batch65("unrect")
    return call, _run(ctx, call)


def test_batch65_equals_the_checker(batch):
    call, got = batch
    bad = _differences(call, got)
    assert len(call.sets) == 65 and not bad, "\n".join(bad)


def test_batch65_sets_equal_themselves_alone_and_early_exits_keep_their_pose(ctx, batch):
    call, got = batch
    a = call.arrays()
    early = 0
    for i, s in enumerate(call.sets):
        one = _run(ctx, call.alone(i))
        for k in T.OUT_NAMES:
            assert np.array_equal(T.raw(one[k][0]), T.raw(got[k][i])), (s.name, k)
        if got["counts4"][i][1] < 10:                                      # ended at the survivor or at the F exit
            early += 1
            assert np.array_equal(T.raw(got["pose7"][i]), T.raw(a["pose_in"][i])), s.name
    assert early >= 10


@pytest.mark.parametrize("n_sets", (1, 2))
def test_small_batches(ctx, n_sets):
    S = T.scenes("depth")
    call = T.Call([S["plain_guess"], S["surv_9"]][:n_sets])
    bad = _differences(call, _run(ctx, call))
    assert not bad, "\n".join(bad)


def test_two_calls_give_identical_bytes_and_scratch_is_reused(ctx):
    S = T.scenes("rect")
    big = T.Call([S["n_1024"], S["plain"], S["F_9_guess"], S["no_model_guess"]])
    small = T.Call([S["plain_guess"], S["pairs_9"]])
    first = _run(ctx, small)
    _run(ctx, big)
    second, third = _run(ctx, small), _run(ctx, small)
    for k in T.OUT_NAMES:
        assert np.array_equal(T.raw(first[k]), T.raw(second[k])) and np.array_equal(T.raw(second[k]), T.raw(third[k])), k
    assert not _differences(small, second)


def test_mask_F_may_be_null(ctx):
    import torch
    call = T.Call([T.scenes("rect")["plain"]])
    a = call.arrays()
    o = _outputs(call)
    f = ctx._lib.flvis_hip_lkorb_tracking
    cfg = call.rig.lib_cfg()
    d = {k: _dev(a[k]) for k in ("img_from", "img_to", "p2d", "p2u", "p3w", "flags", "count", "pose_in")}
    rc = f(ctx._h, C.byref(cfg), *(d[k].data_ptr() for k in ("img_from", "img_to")), 1, *(d[k].data_ptr() for k in ("p2d", "p2u", "p3w", "flags", "count")),
           call.cap, None, None, o["to_from"].data_ptr(), o["to_2d_plane"].data_ptr(), o["to_2d_undistort"].data_ptr(), o["to_flags"].data_ptr(), None,
           o["counts4"].data_ptr(), d["pose_in"].data_ptr(), o["ret"].data_ptr())
    ctx.synchronize()
    assert rc == 0
    e = call.expected()
    for k in ("to_from", "to_flags", "counts4", "ret"):
        assert np.array_equal(o[k].cpu().numpy(), e[k]), k
    assert np.array_equal(T.raw(d["pose_in"].cpu().numpy()), T.raw(e["pose7"]))


def test_refusals_leave_the_outputs_untouched(ctx):
    import flvis_amd
    import torch
    call = T.Call([T.scenes("rect")["surv_10"]])
    a = call.arrays()
    cfg = call.rig.lib_cfg()
    f = ctx._lib.flvis_hip_lkorb_tracking
    d = {k: _dev(a[k]) for k in ("img_from", "img_to", "p2d", "p2u", "p3w", "flags", "count")}
    big = {k: _dev(np.zeros((1, 1025) + a[k].shape[2:], a[k].dtype)) for k in ("p2d", "p2u", "p3w", "flags")}
    ones = np.ones(1, np.uint8)

    def attempt(want, cfg_=cfg, n_sets=1, cap=call.cap, null=None, use_guess=None, guess7=None, src=d):
        o = _outputs(call)
        pose = _dev(a["pose_in"])
        args = dict(img_from=d["img_from"].data_ptr(), img_to=d["img_to"].data_ptr(), p2d=src["p2d"].data_ptr(), p2u=src["p2u"].data_ptr(),
                    p3w=src["p3w"].data_ptr(), flags=src["flags"].data_ptr(), count=d["count"].data_ptr(), to_from=o["to_from"].data_ptr(),
                    to_2d_plane=o["to_2d_plane"].data_ptr(), to_2d_undistort=o["to_2d_undistort"].data_ptr(), to_flags=o["to_flags"].data_ptr(),
                    mask_F=o["mask_F"].data_ptr(), counts4=o["counts4"].data_ptr(), pose7=pose.data_ptr(), ret=o["ret"].data_ptr())
        if null:
            args[null] = None
        rc = f(ctx._h, None if cfg_ is None else C.byref(cfg_), args["img_from"], args["img_to"], n_sets, args["p2d"], args["p2u"], args["p3w"],
               args["flags"], args["count"], cap, None if guess7 is None else guess7.ctypes.data, None if use_guess is None else use_guess.ctypes.data,
               args["to_from"], args["to_2d_plane"], args["to_2d_undistort"], args["to_flags"], args["mask_F"], args["counts4"], args["pose7"], args["ret"])
        ctx.synchronize()
        assert rc == want, (rc, want, null)
        fresh = _outputs(call)
        for k in fresh:
            assert torch.equal(o[k], fresh[k]), (k, null)
        assert np.array_equal(T.raw(pose.cpu().numpy()), T.raw(a["pose_in"]))

    for name in ("img_from", "img_to", "p2d", "p2u", "p3w", "flags", "count", "to_from", "to_2d_plane", "to_2d_undistort", "to_flags", "counts4",
                 "pose7", "ret"):
        attempt(flvis_amd.FLVIS_ERR_INVALID_ARG, null=name)
    attempt(flvis_amd.FLVIS_ERR_INVALID_ARG, cfg_=None)
    attempt(flvis_amd.FLVIS_ERR_INVALID_ARG, n_sets=0)
    attempt(flvis_amd.FLVIS_ERR_INVALID_ARG, n_sets=-1)
    attempt(flvis_amd.FLVIS_ERR_INVALID_ARG, cap=0)
    attempt(flvis_amd.FLVIS_ERR_INVALID_ARG, use_guess=ones)                 # a guess asked for, none given
    attempt(flvis_amd.FLVIS_ERR_CAPACITY, cap=1025, src=big)
    small = call.rig.lib_cfg()
    small.image_width = 31
    attempt(flvis_amd.FLVIS_ERR_CONFIG, cfg_=small)
    small = call.rig.lib_cfg()
    small.image_height = 31
    attempt(flvis_amd.FLVIS_ERR_CONFIG, cfg_=small)
    raw_cfg = type(cfg)()                                                    # never finalised: P0 is empty
    raw_cfg.image_width, raw_cfg.image_height = cfg.image_width, cfg.image_height
    attempt(flvis_amd.FLVIS_ERR_CONFIG, cfg_=raw_cfg)
    # (and the call still works afterwards, guess given and used)
    call2 = T.Call([T.scenes("rect")["plain_guess"]])
    assert not _differences(call2, _run(ctx, call2))
