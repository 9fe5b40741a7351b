"""GPU parity tests (run with -m gpu on MI355X): the corner selection behind the corner-response pass -- k_gftt_pick and the two FeatureDEM
kernels -- at its tier, plateau, capacity and spacing edges, against the CPU oracle, through the C ABI.  The inputs come from
tests/_gftt_edges.py, which asserts on the CPU that each of them reaches the edge it is named for (tests/test_gftt_edges_inputs.py pins
the figures).  Everything here is integer pixel coordinates in float32: count and coordinates are compared bit for bit."""
import numpy as np
import pytest

import _gftt_edges as E

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


def _gftt(ctx, cases):
    """one flvis_hip_gftt call on the images of `cases` (one size, one parameter set) -> [corners of every image]"""
    c0 = cases[0]
    xy, cnt = ctx.gftt(_cuda(np.stack([c.img for c in cases])), c0.maxc, c0.q, c0.md)
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    return [xy[i, :cnt[i]] for i in range(len(cases))]


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, int(np.nonzero((got != want).any(1))[0][0]))


@pytest.mark.parametrize("name", E.GFTT)
def test_gftt_recipe_equals_the_oracle(ctx, name):
    c = E.case(name)
    _same(_gftt(ctx, [c])[0], c.want, name)


@pytest.mark.parametrize("name", E.OVER)
def test_gftt_above_the_old_key_capacity_three_times(ctx, name):
    """more candidates than (w / 2 + 1)(h / 2 + 1): which keys a too small scratch drops depends on the order of the atomics, so one
    good pass proves nothing -- every one of three calls equals the oracle"""
    c = E.case(name)
    for k in range(3):
        _same(_gftt(ctx, [c])[0], c.want, (name, k))


@pytest.mark.parametrize("variant,rows", [(0, 0), (1, 0), (2, 60)])
@pytest.mark.parametrize("name", E.PLATEAUS + E.OVER)
def test_corner_response_keeps_every_plateau_candidate(ctx, name, variant, rows):
    """the complete key set of the response pass (LDS tiles, strip-mined tiles, wave walk) on images whose plateaus make every pixel of
    a plateau a candidate: the maximum and every (response bits, offset) key equal the oracle's"""
    c = E.case(name)
    wmax, wkeys = E.response_keys(c.img)
    mx, keys = ctx.debug_corner_response(_cuda(c.img[None]), variant, rows, key_cap=max(1024, c.h * c.w))
    assert int(mx[0]) == wmax, (hex(int(mx[0])), hex(wmax))
    assert len(keys[0]) == len(wkeys) and np.array_equal(keys[0], wkeys), (len(keys[0]), len(wkeys))


def test_ragged_batch_and_the_call_after_it(ctx):
    """one call holds a full-sort image, a flat one, an exhausted walk and a plain one; the next call, on images of another size, finds
    the counters zeroed and reuses the scratch by name: neither depends on the other, in either order"""
    first = [E.case(n) for n in E.BATCHES["ragged"]]
    nxt = [E.case(n) for n in E.BATCHES["ragged_next"]]
    for rnd in range(2):
        for cases in (first, nxt):
            for c, got in zip(cases, _gftt(ctx, cases)):
                _same(got, c.want, (rnd, c.name))
    for c, got in zip(first[::-1], _gftt(ctx, first[::-1])):      # the streams are independent of their slot
        _same(got, c.want, ("reversed", c.name))


@pytest.mark.parametrize("name", E.DEM)
def test_feature_dem_recipe_equals_the_oracle(ctx, name):
    c = E.case(name)
    if c.exist is None:
        xy, cnt = ctx.feature_dem_detect(_cuda(c.img[None]), c.fp)
    else:
        cap = max(16, len(c.exist))
        ex = np.zeros((1, cap, 2), np.float64)
        ex[0, :len(c.exist)] = c.exist
        xy, cnt = ctx.feature_dem_redetect(_cuda(c.img[None]), c.fp, _cuda(ex), _cuda(np.array([len(c.exist)], np.int32)))
    n = int(cnt[0])
    _same(xy[0, :n].cpu().numpy(), c.want, name)


def test_feature_dem_redetect_batch_mixes_crowded_and_empty_streams(ctx):
    """the redetect recipes of one size in ONE call: a region with more existing points than the kernel keeps in LDS next to streams
    with a few and with none"""
    names = ("redetect_crowded", "redetect_places", "redetect_over_capacity", "redetect_full_region", "redetect_at_capacity")
    cases = [E.case(n) for n in names]
    cap = max(len(c.exist) for c in cases)
    ex = np.zeros((len(cases) + 1, cap, 2), np.float64)
    nex = np.zeros(len(cases) + 1, np.int32)
    for i, c in enumerate(cases):
        ex[i, :len(c.exist)], nex[i] = c.exist, len(c.exist)
    imgs = np.stack([c.img for c in cases] + [cases[0].img])          # the last stream: the crowded image without existing points
    xy, cnt = ctx.feature_dem_redetect(_cuda(imgs), cases[0].fp, _cuda(ex), _cuda(nex))
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    for i, c in enumerate(cases):
        _same(xy[i, :cnt[i]], c.want, c.name)
    import _oracle as O
    _same(xy[-1, :cnt[-1]], O.dem_redetect(cases[0].img, cases[0].fp, np.zeros((0, 2))), "no existing points")


def test_feature_dem_refuses_more_features_per_region_than_it_keeps(ctx):
    """max_region_feature_num (f_para[0]) above the kernel's per-region capacity is FLVIS_ERR_CAPACITY (-4) before anything is launched;
    at the capacity the call goes through"""
    import flvis_amd
    c = E.case("dem_maxc")
    assert c.fp[0] == E.DEM_MAXR
    img = _cuda(c.img[None])
    for call in (lambda fp: ctx.feature_dem_detect(img, fp),
                 lambda fp: ctx.feature_dem_redetect(img, fp, _cuda(np.zeros((1, 16, 2))), _cuda(np.zeros(1, np.int32)))):
        with pytest.raises(flvis_amd.FlvisError, match=r"\(-4\).*192"):
            call([E.DEM_MAXR + 1] + c.fp[1:])
        with pytest.raises(flvis_amd.FlvisError, match=r"\(-4\).*192"):
            call([300.0] + c.fp[1:])
    xy, cnt = ctx.feature_dem_detect(img, c.fp)
    _same(xy[0, :int(cnt[0])].cpu().numpy(), c.want, "at the capacity")
