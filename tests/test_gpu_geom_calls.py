"""GPU (-m gpu, MI355X): the front-end's solver calls on caller arrays -- flvis_hip_find_fundamental_ransac (k_fund_ransac_sets),
flvis_hip_optimize_in_frame (k_pose_lm_sets), flvis_hip_undistort_points / flvis_hip_project_points -- against the CPU oracle, BIT FOR BIT:
masks, inlier counts, ok flags, every double of a pose, every float of a point as its uint32 pattern.  No tolerance anywhere.  The inputs
and what the oracle says about them come from tests/_geom_calls.py (pinned, without a GPU, by tests/test_geom_calls_inputs.py).

Every output buffer is filled with a sentinel before the call: rows from a set's count on, the outputs of a refused call and the pose of
an ok = 0 set must come back as they went in.

One bit is left open, in one place: where the oracle's pixel is a NaN, the kernel's must be a NaN with the same quiet bit and payload, but
its SIGN is not compared.  IEEE 754 leaves the sign of a NaN that an invalid operation produces (inf - inf, 0 * inf: undistortPoints of an
infinite pixel) to the implementation: the x86 the oracle runs on delivers the negative default NaN (0xFFC00000), gfx950 the positive one
(0x7FC00000), from the same source line -- measured: 0x7FC00000 against 0xFFC00000 on that row, every other value equal.  A NaN that
comes in with the input, +-inf, -0 and every finite value are compared on all 32 bits."""
import numpy as np
import pytest

import _geom_calls as E
import _oracle as O

pytestmark = pytest.mark.gpu
needs_product_sums = pytest.mark.skipif(O.lib().ref_sum_order() != 0, reason="the REF_ORDER=g2o checker sums the pose LM in another order")
SENT_U8, SENT_I32 = 0xAB, -77
SENT_F32_BITS = int(np.array([0xDEADBEEF], np.uint32).view(np.int32)[0])     # the float outputs' sentinel, as the int32 of its pattern


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- F-matrix RANSAC ---------------------------------------------------------------------------------------------------------------------
def _f_launch(ctx, m1, m2, cnt, **kw):
    """one call on sentinel-filled outputs -> (mask [s,cap], inliers [s]) on the host"""
    import torch
    s, cap, _ = m1.shape
    mask = torch.full((s, cap), SENT_U8, dtype=torch.uint8, device="cuda")
    ninl = torch.full((s,), SENT_I32, dtype=torch.int32, device="cuda")
    ctx.find_fundamental_ransac(_dev(m1), _dev(m2), _dev(cnt), mask=mask, n_inliers=ninl, **kw)
    return mask.cpu().numpy(), ninl.cpu().numpy()


def _f_differences(names, mask, ninl):
    bad = []
    for k, nm in enumerate(names):
        want_n, want = E.f_expected(nm)
        n = len(want)
        why = []
        if ninl[k] != want_n:
            why.append("inliers %d, oracle %d" % (ninl[k], want_n))
        if not np.array_equal(mask[k, :n], want):
            why.append("mask differs at %s" % np.flatnonzero(mask[k, :n] != want)[:8])
        if not (mask[k, n:] == SENT_U8).all():
            why.append("rows beyond the count written")
        if why:
            bad.append("%s: %s" % (nm, "; ".join(why)))
    return bad


@pytest.fixture(scope="module")
def f_batch(ctx):
    """all 65 sets in one launch (ragged counts 0 .. 1024, cap 1024)"""
    names = list(E.f_sets())
    return names, _f_launch(ctx, *E.f_rows(names))


def test_f_ransac_batch_equals_the_oracle(f_batch):
    names, (mask, ninl) = f_batch
    bad = _f_differences(names, mask, ninl)
    print("%d sets, %d differ; inliers %s" % (len(names), len(bad), dict(zip(names, ninl.tolist()))))
    assert len(names) == 65 and not bad, "\n".join(bad)


def test_f_ransac_sets_alone_and_in_pairs_equal_the_batch(ctx, f_batch):
    names, (mask, ninl) = f_batch
    for k, nm in enumerate(names):                            # n_sets = 1: every set alone
        m, c = _f_launch(ctx, *E.f_rows([nm]))
        assert np.array_equal(m[0], mask[k]) and c[0] == ninl[k], nm
    for k in range(0, 12, 2):                                  # n_sets = 2
        m, c = _f_launch(ctx, *E.f_rows(names[k:k + 2]))
        assert np.array_equal(m, mask[k:k + 2]) and np.array_equal(c, ninl[k:k + 2]), names[k:k + 2]


def test_f_ransac_clamps_the_count(ctx):
    """a count above cap reads as cap, a negative one as 0"""
    cap = 32
    a, b = E.f_sets()["clean_64"]
    m1 = np.stack([a[:cap], a[:cap], a[:cap]])
    m2 = np.stack([b[:cap], b[:cap], b[:cap]])
    mask, ninl = _f_launch(ctx, m1, m2, np.array([40, -3, 20], np.int32))
    for k, n in enumerate((32, 0, 20)):
        want_n, want = (0, np.zeros(0, np.uint8)) if n == 0 else O.find_fundamental_ransac(a[:n], b[:n], E.F_THR, E.F_CONF)
        assert ninl[k] == want_n and np.array_equal(mask[k, :n], want) and (mask[k, n:] == SENT_U8).all(), (k, n)


def test_f_ransac_other_threshold_and_confidence(ctx):
    names = ["clean_240", "clean_14", "outliers_300"]
    for thr, conf in ((1.0, 0.99), (5.0, 0.5)):
        mask, ninl = _f_launch(ctx, *E.f_rows(names), thr_px=thr, confidence=conf)
        for k, nm in enumerate(names):
            want_n, want = E.f_expected(nm, thr, conf)
            assert ninl[k] == want_n and np.array_equal(mask[k, :len(want)], want), (nm, thr, conf)


def test_f_ransac_refusals_write_nothing(ctx):
    import flvis_amd
    cnt = np.array([20], np.int32)
    for cap, kw, code in ((1025, {}, flvis_amd.FLVIS_ERR_CAPACITY), (32, dict(thr_px=0.0), flvis_amd.FLVIS_ERR_INVALID_ARG),
                          (32, dict(thr_px=-1.0), flvis_amd.FLVIS_ERR_INVALID_ARG), (32, dict(confidence=1.0), flvis_amd.FLVIS_ERR_INVALID_ARG),
                          (32, dict(confidence=0.0), flvis_amd.FLVIS_ERR_INVALID_ARG)):
        import torch
        m = np.zeros((1, cap, 2), np.float32)
        mask = torch.full((1, cap), SENT_U8, dtype=torch.uint8, device="cuda")
        ninl = torch.full((1,), SENT_I32, dtype=torch.int32, device="cuda")
        with pytest.raises(flvis_amd.FlvisError) as e:
            ctx.find_fundamental_ransac(_dev(m), _dev(m), _dev(cnt), mask=mask, n_inliers=ninl, **kw)
        assert "(%d)" % code in str(e.value)
        ctx.synchronize()
        assert (mask.cpu().numpy() == SENT_U8).all() and ninl.cpu().numpy()[0] == SENT_I32


# ---- pose-only LM ------------------------------------------------------------------------------------------------------------------------
def _lm_launch(ctx, rows, K):
    """one call; the pose buffer goes in as the start poses -> (pose7 [s,7], ok [s]) on the host"""
    import torch
    p3, z, ids, cnt, pose, _ = rows
    d_pose = _dev(pose)
    ok = torch.full((len(cnt),), SENT_U8, dtype=torch.uint8, device="cuda")
    ctx.optimize_in_frame(_dev(p3), _dev(z), _dev(ids), _dev(cnt), K, d_pose, ok=ok)
    return d_pose.cpu().numpy(), ok.cpu().numpy()


def _lm_differences(names, pose, ok):
    bad = []
    for k, nm in enumerate(names):
        s = E.lm_sets()[nm]
        want_ok, want = s.expected
        if ok[k] != (1 if want_ok else 0):
            bad.append("%s: ok %d, oracle %d" % (nm, ok[k], want_ok))
        elif not np.array_equal(pose[k].view(np.uint64), (want if want_ok else s.pose0).view(np.uint64)):
            bad.append("%s: pose - oracle = %s" % (nm, pose[k] - want))
    return bad


@pytest.fixture(scope="module")
def lm_batch(ctx):
    """every set in one launch, one camera per set (n_K = n_sets)"""
    names = list(E.lm_sets())
    rows = E.lm_rows(names)
    return names, rows, _lm_launch(ctx, rows, rows[5])


@needs_product_sums
def test_pose_lm_batch_equals_the_oracle(lm_batch):
    names, rows, (pose, ok) = lm_batch
    bad = _lm_differences(names, pose, ok)
    print("%d sets (counts %s), ok %s, %d differ" % (len(names), rows[3].tolist(), ok.tolist(), len(bad)))
    assert not bad, "\n".join(bad)
    S = E.lm_sets()
    assert ok[names.index("count_9")] == 0 and ok[names.index("cull_9")] == 0 and ok[names.index("cull_10")] == 1
    # equal ids: input order decides -- the swapped set's pose is the oracle's OTHER pose
    a, b = names.index("ids_duplicate"), names.index("ids_duplicate_swapped")
    assert not np.array_equal(pose[a], pose[b]) and np.array_equal(pose[b], S["ids_duplicate_swapped"].expected[1])


@needs_product_sums
def test_pose_lm_one_camera_for_all_equals_one_per_set(ctx, lm_batch):
    names, _, (pose, ok) = lm_batch
    for K, mine in ((E.K4, [n for n in names if n != "camera_1"]), (E.K4_B, ["camera_1"])):
        rows = E.lm_rows(mine)
        assert (rows[5] == K).all()
        p, o = _lm_launch(ctx, rows, K)                        # n_K = 1
        idx = [names.index(n) for n in mine]
        assert np.array_equal(p, pose[idx]) and np.array_equal(o, ok[idx])
    p, o = _lm_launch(ctx, E.lm_rows(["count_33"]), E.K4)      # n_sets = 1
    assert np.array_equal(p[0], pose[names.index("count_33")]) and o[0] == 1


@needs_product_sums
def test_pose_lm_clamps_the_count(ctx):
    cap = 32
    s = E.lm_sets()["count_33"]
    rows = list(E.lm_rows(["count_33", "count_33", "count_33"], cap=33))
    rows = [np.ascontiguousarray(r[:, :cap]) if r.ndim > 1 and r.shape[1] == 33 else r for r in rows]
    rows[3] = np.array([40, -3, 9], np.int32)
    pose, ok = _lm_launch(ctx, rows, E.K4)
    want_ok, want = O.optimize_in_frame(s.pose0, s.p3[:cap], s.z[:cap], s.ids[:cap], E.K4)
    assert want_ok and ok.tolist() == [1, 0, 0]
    assert np.array_equal(pose[0], want) and np.array_equal(pose[1], s.pose0) and np.array_equal(pose[2], s.pose0)


def test_pose_lm_refuses_more_than_512_edges(ctx):
    import flvis_amd
    import torch
    cap = 513
    pose = torch.zeros((1, 7), dtype=torch.float64, device="cuda")
    pose[0, 6] = 1.0
    before = pose.cpu().numpy().copy()
    ok = torch.full((1,), SENT_U8, dtype=torch.uint8, device="cuda")
    with pytest.raises(flvis_amd.FlvisError) as e:
        ctx.optimize_in_frame(torch.zeros((1, cap, 3), dtype=torch.float64, device="cuda"), torch.zeros((1, cap, 2), dtype=torch.float64, device="cuda"),
                              torch.zeros((1, cap), dtype=torch.int64, device="cuda"), _dev(np.array([20], np.int32)), E.K4, pose, ok=ok)
    assert "(%d)" % flvis_amd.FLVIS_ERR_CAPACITY in str(e.value)
    ctx.synchronize()
    assert ok.cpu().numpy()[0] == SENT_U8 and np.array_equal(pose.cpu().numpy(), before)


# ---- undistortPoints / projectPoints ------------------------------------------------------------------------------------------------------
PT_KEYS = [(rig, n) for rig in E.RIGS for n in E.PT_COUNTS]


def _pt_rows(keys):
    src = np.full((len(keys), E.PT_CAP, 2), E.GARBAGE, np.float32)
    p3 = np.full((len(keys), E.PT_CAP, 3), E.GARBAGE, np.float32)
    cnt = np.zeros(len(keys), np.int32)
    pose = np.zeros((len(keys), 7))
    for k, key in enumerate(keys):
        s = E.pt_sets()[key]
        src[k, :key[1]], p3[k, :key[1]], cnt[k], pose[k] = s["src"], s["p3d"], key[1], s["pose7"]
    cams = [E.rigs()[key[0]] for key in keys]
    return src, p3, cnt, pose, [np.stack([c[i] for c in cams]) for i in range(4)]


def _pt_launch(ctx, keys, per_set):
    """undistort + project of the sets on sentinel-filled outputs, with one camera per set or (all sets of one rig) one camera"""
    import torch
    src, p3, cnt, pose, (K, D, R, P) = _pt_rows(keys)
    if not per_set:
        K, D, R, P = K[0], D[0], R[0], P[0]
    und = torch.full((len(keys), E.PT_CAP, 2), SENT_F32_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    prj = torch.full((len(keys), E.PT_CAP, 2), SENT_F32_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    ctx.undistort_points(_dev(src), _dev(cnt), K, D, R, P, dst=und)
    ctx.project_points(_dev(p3), _dev(cnt), pose, K, D, dst=prj)
    return E.bits(und.cpu().numpy()), E.bits(prj.cpu().numpy())


def _same_bits(got, want):
    """uint32 patterns equal; where the oracle has a NaN, equal but for the sign bit (see the module's docstring)"""
    nan = (want & 0x7FFFFFFF) > 0x7F800000
    return (got == want) | (nan & ((got & 0x7FFFFFFF) == (want & 0x7FFFFFFF)))


def _pt_differences(keys, und, prj):
    bad = []
    for k, (rig, n) in enumerate(keys):
        wu, wp = E.pt_expected(rig, n)
        for what, got, want in (("undistort", und[k], E.bits(wu)), ("project", prj[k], E.bits(wp))):
            if not _same_bits(got[:n], want).all():
                i = np.flatnonzero((~_same_bits(got[:n], want)).any(1))[:4]
                bad.append("%s %s/%d: rows %s: %s, oracle %s" % (what, rig, n, i, got[i].tolist(), want[i].tolist()))
            if not (got[n:] == 0xDEADBEEF).all():
                bad.append("%s %s/%d: rows beyond the count written" % (what, rig, n))
    return bad


def test_points_equal_the_oracle_bit_for_bit(ctx):
    und, prj = _pt_launch(ctx, PT_KEYS, per_set=True)          # 10 sets, two rigs: n_cam = n_sets
    bad = _pt_differences(PT_KEYS, und, prj)
    assert not bad, "\n".join(bad)
    for rig in E.RIGS:                                         # n_cam = 1: the sets of one rig
        keys = [k for k in PT_KEYS if k[0] == rig]
        u, p = _pt_launch(ctx, keys, per_set=False)
        idx = [PT_KEYS.index(k) for k in keys]
        assert np.array_equal(u, und[idx]) and np.array_equal(p, prj[idx]), rig


def test_points_clamp_the_count_and_refuse_a_camera_count(ctx):
    import flvis_amd
    import torch
    K, D, R, P = E.rigs()["euroc"]
    s = E.pt_sets()[("euroc", 65)]
    cap = 40
    src = np.stack([s["src"][:cap]] * 2)
    p3 = np.stack([s["p3d"][:cap]] * 2)
    cnt = _dev(np.array([65, -1], np.int32))
    und = torch.zeros((2, cap, 2), dtype=torch.float32, device="cuda")
    prj = torch.zeros((2, cap, 2), dtype=torch.float32, device="cuda")
    ctx.undistort_points(_dev(src), cnt, K, D, R, P, dst=und)
    ctx.project_points(_dev(p3), cnt, np.stack([s["pose7"]] * 2), K, D, dst=prj)
    wu, wp = E.pt_expected("euroc", 65)
    assert _same_bits(E.bits(und.cpu().numpy()[0]), E.bits(wu[:cap])).all() and np.array_equal(E.bits(prj.cpu().numpy()[0]), E.bits(wp[:cap]))
    assert not und.cpu().numpy()[1].any() and not prj.cpu().numpy()[1].any()
    # three sets, two cameras: refused, nothing written
    import ctypes as C
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    src3, cnt3 = _dev(np.zeros((3, 8, 2), np.float32)), _dev(np.full(3, 8, np.int32))
    dst3 = torch.full((3, 8, 2), SENT_F32_BITS, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx._lib.flvis_hip_undistort_points(ctx._h, p(src3), p(cnt3), 8, 3, d(np.stack([K, K])), d(np.stack([D, D])), d(np.stack([R, R])),
                                             d(np.stack([P, P])), 2, p(dst3))
    assert rc == flvis_amd.FLVIS_ERR_INVALID_ARG
    rc = ctx._lib.flvis_hip_project_points(ctx._h, p(_dev(np.zeros((3, 8, 3), np.float32))), p(cnt3), 8, 3, d(np.zeros((3, 7))), d(np.stack([K, K])),
                                           d(np.stack([D, D])), 2, p(dst3))
    assert rc == flvis_amd.FLVIS_ERR_INVALID_ARG
    ctx.synchronize()
    assert (dst3.cpu().numpy() == SENT_F32_BITS).all()
