"""CPU: the dense cloud's restatement (tests/_depth_cloud.py) against its second write-up, proof that every edge case reaches its edge,
and the host part of flvis_hip_depth_cloud's argument checks (flvis_depth_cloud_check, no device)."""
import ctypes as C

import numpy as np
import pytest

import _depth_cloud as DC
import _map_cloud as MC


def _same(a, b, what):
    for k in ("n_out", "n_dropped", "n_valid"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["xyz"].tobytes() == b["xyz"].tobytes() and np.array_equal(a["npts"], b["npts"]), what


def _cases():
    out = {"zmin 0.3": DC.limit_case(0.3)[0], "zmin 0.5": DC.limit_case(0.5)[0], "empty between": DC.empty_between_case(),
           "65 apart": DC.apart_case(65, h=37, w=70), "first and last": DC.first_last_case(),
           "two cameras": DC.random_case(3, 3, 37, 70, DC.params((1, 2, 68, 36), (3, 5)), cams=(DC.CAM_A, DC.CAM_B), clouds=[[(0, 2), (1, 2)]])}
    return out


@pytest.mark.parametrize("leaf", [0.0, 0.125, 0.08])
def test_the_two_write_ups_agree(leaf):
    for name, case in _cases().items():
        for c in range(len(case["clouds"])):
            a, b = DC.restate(case, c, leaf), DC.restate_loops(case, c, leaf)
            _same(a, b, (name, c, leaf))
            for i, cam in DC.listed(case, c):
                pa, ma = DC.samples(case["depth"][i], cam, case["prm"])
                pb, mb = DC.samples_loops(case["depth"][i].tolist(), cam, case["prm"])
                assert pa.tobytes() == pb.tobytes() and np.array_equal(ma, mb), (name, i)


@pytest.mark.parametrize("z_min", [0.3, 0.5])
def test_the_limits_are_inclusive_and_the_pixel_is_unsigned(z_min):
    case, want = DC.limit_case(z_min)
    img, prm = case["depth"][0], case["prm"]
    edge = int(round(1000 * z_min))
    assert np.float64(np.float32(z_min)) >= z_min, "the float of the limit is not below the limit: raw = 1000 z_min is valid"
    p, mask = DC.samples(img, case["cams"][0], prm)
    for raw, valid in want.items():
        at = img == raw
        assert at.sum() >= 3, raw
        assert (mask[at] == valid).all(), (raw, valid)
    assert want[edge] and not want[edge - 1] and want[40000] and not want[0] and not want[65535]
    # 40000 read as a signed pixel would be -25536: 40 m must come out
    assert np.any(p[:, 2] == 40.0)
    assert len(p) == sum(int((img == raw).sum()) for raw, v in want.items() if v)


def test_an_image_without_a_valid_sample_lies_between_two_with_some():
    case = DC.empty_between_case()
    n = [len(DC.samples(case["depth"][i], case["cams"][0], case["prm"])[0]) for i in range(3)]
    assert n[0] > 0 and n[1] == 0 and n[2] > 0
    r = DC.restate(case, 0, 0.0)
    assert r["n_valid"] == n[0] + n[2] == r["n_out"]


def test_samples_65_apart_cross_every_wave_boundary():
    case = DC.apart_case(65)
    _, mask = DC.samples(case["depth"][0], case["cams"][0], case["prm"])
    pos = np.flatnonzero(mask.ravel())
    assert len(pos) > 128 and (np.diff(pos) == 65).all()
    # a wave is 64 consecutive samples wherever a workgroup's rounds start: none holds two valid samples, while any 256 consecutive
    # samples -- the four waves of a round -- hold three or four, so a position always adds up counts of other waves
    for start in (0, 1, 63, 129, 3999):
        rounds = np.bincount((pos[pos >= start] - start) // 256)[:-1]
        assert ((rounds == 3) | (rounds == 4)).all() and (rounds == 4).sum() > 20, start
        waves = (pos[pos >= start] - start) // 64
        assert len(set(waves)) == len(waves)


def test_only_the_first_and_the_last_sampled_pixel_are_valid():
    case = DC.first_last_case()
    p, mask = DC.samples(case["depth"][0], case["cams"][0], case["prm"])
    assert mask.sum() == 2 and mask[0, 0] and mask[-1, -1] and mask.shape == (5, 10)
    assert p[0, 2] == np.float64(np.float32(1800 / 1000.0))
    assert p[1, 2] == np.float64(np.float32(2200 / 1000.0))
    # the window ends mid-step: the last sampled column is 65 < 66 and the next would be 72
    us, vs = DC.grid(case["prm"], 70, 37)
    assert us[-1] == 65 and vs[-1] == 29


def test_an_identity_pose_and_leaf_0_return_the_samples_rounded():
    case = DC.random_case(5, 1, 37, 70, DC.params(step=(7, 7)), poses=False)
    p, _ = DC.samples(case["depth"][0], case["cams"][0], case["prm"])
    r = DC.restate(case, 0, 0.0)
    assert r["xyz"].tobytes() == (p + 0.0).astype(np.float32).tobytes() and r["n_dropped"] == 0


def test_argument_errors_without_a_device():
    """flvis_depth_cloud_check is the host part of flvis_hip_depth_cloud's checks; the entries themselves refuse a NULL context / closer"""
    import flvis_amd
    lib = flvis_amd.load_library()
    chk = lib.flvis_depth_cloud_check
    ints = lambda *v: (C.c_int * len(v))(*v)  # noqa: E731
    dbl = lambda *v: (C.c_double * len(v))(*v)  # noqa: E731
    P = flvis_amd.DepthCloudParams
    cams = dbl(*(DC.CAM_A + DC.CAM_B + DC.CAM_A))
    good = dict(n_img=10, w=70, h=37, n_clouds=2, ptr=ints(0, 1, 3), rng=ints(0, 4, 2, 2, 9, 1), cams=cams, prm=P(0, 0, 0, 0, 1, 1, 0.3, 10.0), leaf=0.08,
                min_points=1, out_cap=5)
    order = ("n_img", "w", "h", "n_clouds", "ptr", "rng", "cams", "prm", "leaf", "min_points", "out_cap")

    def call(**kw):
        a = dict(good, **kw)
        a["prm"] = C.byref(a["prm"]) if a["prm"] is not None else None
        return chk(*[a[k] for k in order])

    def cam(i, v):
        c = DC.CAM_A + DC.CAM_B + DC.CAM_A
        c[i] = v
        return dbl(*c)
    ok = [dict(), dict(leaf=0.0), dict(out_cap=0), dict(prm=P(2, 1, 66, 35, 7, 7, 0.5, 6.5)), dict(prm=P(69, 36, 70, 37, 1, 1, 0.0, 0.0)),
          dict(prm=P(0, 0, -1, -1, 100, 100, 1.0, 1.0)), dict(cams=cam(2, 0.0)), dict(cams=cam(3, -4.0))]
    for kw in ok:
        assert call(**kw) == 0, kw
    inf, nan = float("inf"), float("nan")
    bad = [dict(prm=P(0, 0, 0, 0, 0, 1, 0.3, 10.0)), dict(prm=P(0, 0, 0, 0, 1, 0, 0.3, 10.0)), dict(prm=P(0, 0, 0, 0, -3, 1, 0.3, 10.0)),
           dict(prm=P(0, 0, 71, 0, 1, 1, 0.3, 10.0)), dict(prm=P(0, 0, 0, 38, 1, 1, 0.3, 10.0)), dict(prm=P(-1, 0, 0, 0, 1, 1, 0.3, 10.0)),
           dict(prm=P(0, -1, 0, 0, 1, 1, 0.3, 10.0)), dict(prm=P(5, 0, 5, 0, 1, 1, 0.3, 10.0)), dict(prm=P(0, 9, 0, 8, 1, 1, 0.3, 10.0)),
           dict(prm=P(70, 0, 0, 0, 1, 1, 0.3, 10.0)), dict(prm=P(0, 0, 0, 0, 1, 1, nan, 10.0)), dict(prm=P(0, 0, 0, 0, 1, 1, 0.3, inf)),
           dict(prm=P(0, 0, 0, 0, 1, 1, -inf, 1.0)), dict(prm=P(0, 0, 0, 0, 1, 1, 2.0, 1.0)), dict(prm=None), dict(cams=None),
           dict(cams=cam(0, 0.0)), dict(cams=cam(6, 0.0)), dict(cams=cam(14, 0.0)), dict(cams=cam(4, nan)), dict(cams=cam(7, inf)),
           dict(cams=cam(13, nan)), dict(w=0), dict(h=-1),
           # the voxel call's own
           dict(leaf=-0.08), dict(leaf=nan), dict(min_points=0), dict(out_cap=-1), dict(n_clouds=0), dict(ptr=ints(1, 1, 3)),
           dict(ptr=ints(0, 2, 1)), dict(ptr=None), dict(rng=None), dict(rng=ints(0, 4, 2, 2, 9, 2)), dict(rng=ints(-1, 4, 2, 2, 9, 1)),
           dict(n_img=0)]
    for kw in bad:
        assert call(**kw) == flvis_amd.FLVIS_ERR_INVALID_ARG, kw
    nul = [None] * 5
    assert lib.flvis_hip_depth_cloud(None, None, None, 1, 70, 37, 1, ints(0, 1), ints(0, 1), cams, C.byref(good["prm"]), 0.08, 1, 0, *nul) == \
        flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_keyframe_log_depth_cloud(None, 1, ints(0), None, C.byref(good["prm"]), 0.08, 1, 0, *nul) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_keyframe_log_depth_cloud_host(None, 1, ints(0), None, C.byref(good["prm"]), 0.08, 1, 0, *nul) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_dense_cloud(None, 1, ints(0, 1), ints(0), None, C.byref(good["prm"]), 0.08, 1, 0, *nul) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_dense_cloud_host(None, 1, ints(0, 1), ints(0), None, C.byref(good["prm"]), 0.08, 1, 0, *nul) == \
        flvis_amd.FLVIS_ERR_INVALID_ARG
    # the feeder's sampling, as the header states it
    f = flvis_amd.octomap_feeder_params(480)
    assert (f.v0, f.v1, f.step_u, f.step_v, f.z_min, f.z_max) == (218, 261, 7, 7, 0.5, 6.5)
    assert list(range(f.v0, f.v1, 7)) == list(range(480 // 2 - 7 * 3 - 1, 480 // 2 + 7 * 3, 7))
