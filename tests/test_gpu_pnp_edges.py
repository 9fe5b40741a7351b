"""The PnP RANSAC on the device (k_pnp_ransac_sets: pnp_ransac_core of track_kernels.hip) against the CPU oracle at its count, batch and
stop-rule edges, in both branches: P3P through flvis_hip_pnp_ransac, the tracker's iterative branch through the test hook
flvis_hip_debug_pnp_ransac_iterative.  The inputs and what the oracle says about them come from tests/_pnp_edges.py (pinned, without a
GPU, by tests/test_pnp_edges_inputs.py); recipes that share (branch, iterations, threshold, confidence, capacity) share a launch.

For every set: the oracle's inlier count, its mask on [:n] and zeros on [n:cap], and -- with a model -- its pose bit for bit (the sums run
in the oracle's order).  Without a model: P3P the identity; iterative the guess, which the kernel takes through quaternion -> matrix ->
quaternion and the oracle leaves untouched: the translation exactly, the quaternion up to its overall sign within 1e-15 per component (a
few roundings of values <= 1, each 2.2e-16)."""
import numpy as np
import pytest

import _pnp_edges as E

pytestmark = pytest.mark.gpu
GROUPS = sorted(E.GROUPS)


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _launch(ctx, cases):
    """one launch on the cases' sets, in the order given -> (pose7 [s,7], mask [s,cap], inliers [s]) on the host"""
    import torch
    c0 = cases[0]
    assert len({(c.branch, c.iterations, c.reproj, c.conf, c.cap) for c in cases}) == 1
    rows = [c.rows() for c in cases]
    p3 = torch.from_numpy(np.stack([r[0] for r in rows])).cuda()
    p2 = torch.from_numpy(np.stack([r[1] for r in rows])).cuda()
    cnt = torch.from_numpy(np.array([c.count for c in cases], np.int32)).cuda()
    if c0.branch == E.ITER:
        out = ctx.debug_pnp_ransac_iterative(p3, p2, cnt, E.K4, np.stack([c.guess for c in cases]), c0.iterations, c0.reproj, c0.conf)
    else:
        out = ctx.pnp_ransac(p3, p2, cnt, E.K4, np.zeros(len(cases), np.uint64), c0.iterations, c0.reproj, c0.conf)
    return [t.cpu().numpy() for t in out]


def _differences(cases, pose, mask, ninl):
    bad = []
    for k, c in enumerate(cases):
        why = []
        if ninl[k] != c.inliers:
            why.append("inliers %d, oracle %d (winner %d)" % (ninl[k], c.inliers, c.winner))
        if not np.array_equal(mask[k, :c.n], c.mask):
            why.append("mask differs at %s" % np.flatnonzero(mask[k, :c.n] != c.mask)[:8])
        if mask[k, c.n:].any():
            why.append("mask set beyond the count")
        if c.inliers > 0 or c.branch == E.P3P:
            if not np.array_equal(pose[k], c.pose):
                why.append("pose - oracle = %s" % (pose[k] - c.pose))
        else:
            sign = 1.0 if pose[k, 6] * c.guess[6] >= 0 else -1.0
            dq = np.abs(sign * pose[k, 3:7] - c.guess[3:7]).max()
            if not np.array_equal(pose[k, :3], c.guess[:3]) or not dq <= 1e-15:
                why.append("guess not returned: t %s, quaternion off by %.3g" % (pose[k, :3] - c.guess[:3], dq))
        if why:
            bad.append("%s: %s" % (c.name, "; ".join(why)))
    return bad


@pytest.mark.parametrize("key", GROUPS, ids=["%s-it%d-px%g-conf%g-cap%d" % k for k in GROUPS])
def test_sets_equal_the_oracle(ctx, key):
    cases = [E.case(n) for n in E.GROUPS[key]]
    pose, mask, ninl = _launch(ctx, cases)
    bad = _differences(cases, pose, mask, ninl)
    print("%s: %d sets, %d with a model, %d differ" % (key, len(cases), sum(c.inliers > 0 for c in cases), len(bad)))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("branch", E.BRANCHES)
def test_sets_do_not_depend_on_their_block_or_neighbours(ctx, branch):
    """the default launch with its sets in reverse order: every set's outputs bit for bit those of the first launch"""
    cases = [E.case(n) for n in E.GROUPS[E.DEFAULT_GROUP[branch]]]
    a = _launch(ctx, cases)
    b = _launch(ctx, cases[::-1])
    for x, y in zip(a, b):
        assert np.array_equal(x, y[::-1], equal_nan=True)
    assert sum(c.inliers > 0 for c in cases) >= 30 and sum(c.inliers == 0 for c in cases) >= 8


def test_hook_refuses_what_pnp_ransac_refuses(ctx):
    import flvis_amd
    import torch
    g = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    for cap, kw, what in ((1025, {}, "at most 1024"), (8, dict(iterations=0), "bad args"), (8, dict(reproj_px=0.0), "bad args"),
                          (8, dict(confidence=1.0), "bad args")):
        p3 = torch.zeros((1, cap, 3), dtype=torch.float32, device="cuda")
        p2 = torch.zeros((1, cap, 2), dtype=torch.float32, device="cuda")
        for fn, last in ((ctx.debug_pnp_ransac_iterative, g), (ctx.pnp_ransac, np.zeros(1, np.uint64))):
            with pytest.raises(flvis_amd.FlvisError) as e:
                fn(p3, p2, cnt, E.K4, last, **kw)
            assert what in str(e.value)
