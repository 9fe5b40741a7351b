"""synth.rig_variant: a variant's yaml loads to the same flvis_cfg through the product's loader and the oracle's (bit for bit, as
test_abi does for the stock rigs), and the Rig it renders with carries that yaml's intrinsics, distortion and extrinsics."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_both(kind, k):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _oracle as O
    import flvis_amd
    from flvis_amd import synth
    rig, text = synth.rig_variant(kind, k)
    p = os.path.join(tempfile.gettempdir(), "flvis_rigvar_%s_%d.yaml" % (kind, k))
    open(p, "w").write(text)
    return rig, flvis_amd.load_config(p), O.load_config(p)


@pytest.mark.parametrize("kind", ["d435i_stereo", "euroc_like", "d435i_depth", "kitti_like"])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_variant_yaml_loads_identically_and_matches_the_rendered_rig(kind, k):
    from flvis_amd import synth
    rig, a, b = _load_both(kind, k)
    assert C.sizeof(a) == C.sizeof(b)
    fb = {getattr(type(b), n).offset: n for n, _ in b._fields_}
    for name, _ in a._fields_:
        if name == "imu_type":
            continue
        va, vb = getattr(a, name), getattr(b, fb[getattr(type(a), name).offset])
        if hasattr(va, "__len__"):
            assert list(va) == list(vb), (kind, k, name)
        else:
            assert va == vb, (kind, k, name, va, vb)
    # the rendered rig is the one the yaml describes
    assert (rig.width, rig.height) == (a.image_width, a.image_height)
    assert np.allclose(list(a.cam0_intrinsics), rig.K0, rtol=1e-15, atol=0)
    assert np.allclose(list(a.cam0_distortion), rig.D0, rtol=1e-15, atol=0)
    if kind != "d435i_depth":
        assert np.allclose(list(a.cam1_intrinsics), rig.K1, rtol=1e-15, atol=0)
        assert np.allclose(list(a.cam1_distortion), rig.D1, rtol=1e-15, atol=0)
        T01 = np.array(list(a.T_cam0_cam1)).reshape(4, 4)
        if kind == "kitti_like":  # (flvis_config_finalize derives it from P1 = K [I | -fx b]: cam0 as seen from cam1)
            T01 = np.linalg.inv(T01)
        assert np.allclose(T01[:3, :3], rig.R_c0_c1, atol=1e-12) and np.allclose(T01[:3, 3], rig.t_c0_c1, atol=1e-12)
    if kind != "kitti_like":  # (the KITTI-like rig has no IMU: its yaml carries no T_imu_cam0)
        T = np.array(list(a.T_imu_cam0)).reshape(4, 4)
        assert np.allclose(T[:3, :3], rig.R_i_c, atol=1e-12) and np.allclose(T[:3, 3], rig.t_i_c, atol=1e-12)
    if kind == "d435i_depth":
        assert a.depth_factor == rig.depth_factor
    # every variant of a kind shares the batch-wide fields of the stock rig ...
    _, s0, _ = _load_both(kind, 0)
    for name in ("type_of_vi", "cam_type", "imu_type", "image_width", "image_height", "window_size", "skip_first_n_imgs", "need_equal_hist"):
        assert getattr(a, name) == getattr(s0, name), name
    assert list(a.feature_para) == list(s0.feature_para)
    # ... and a variant other than the stock one differs in its calibration
    if k:
        assert list(a.P0) != list(s0.P0)
        if kind == "euroc_like":
            assert list(a.cam0_distortion) != list(s0.cam0_distortion)
        if kind == "d435i_depth":
            assert a.depth_factor != s0.depth_factor
        if kind in ("d435i_stereo", "euroc_like", "d435i_depth"):
            assert list(a.T_imu_cam0) != list(s0.T_imu_cam0)
        if kind != "d435i_depth":
            assert list(a.T_cam0_cam1) != list(s0.T_cam0_cam1)


def test_stock_variant_is_the_stock_rig():
    from flvis_amd import synth
    for kind, stock in (("d435i_stereo", synth.d435_rig()), ("euroc_like", synth.euroc_rig()), ("kitti_like", synth.kitti_like_rig())):
        rig, _ = synth.rig_variant(kind, 0)
        assert np.allclose(rig.K0, stock.K0, rtol=0, atol=0) and np.allclose(rig.D0, stock.D0, rtol=0, atol=0)
        assert np.allclose(rig.t_c0_c1, stock.t_c0_c1, atol=1e-15) and np.allclose(rig.R_i_c, stock.R_i_c, atol=1e-15)
    with pytest.raises(ValueError):
        synth.rig_variant("no_such_rig", 1)
