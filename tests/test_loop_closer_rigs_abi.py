"""CPU: the fleet entry points of the loop closing are part of the C ABI -- declared in include/flvis_hip.h, exported by the library and
bound by the ctypes harness -- and refuse a call without a context or closer instead of touching a device."""
import ctypes as C
import os
import re

import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("flvis_loop_closer_create_rigs", "flvis_loop_closer_reset", "flvis_loop_closer_reset_rigs", "flvis_loop_closer_stream_cfg",
       "flvis_hip_lc_keyframe_landmarks_rigs", "flvis_hip_pnp_ransac_rigs")


def test_fleet_entry_points_are_declared_and_exported():
    import flvis_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    lib = flvis_amd.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared in include/flvis_hip.h" % name
        assert hasattr(lib, name), "%s is not exported" % name


def test_harness_binds_the_fleet_entry_points():
    import flvis_amd
    for name in ("reset", "stream_cfg"):
        assert callable(getattr(flvis_amd.LoopCloser, name))
    src = _binding.source()
    for name in NEW:
        assert re.search(r"_lib\.%s\b" % name, src), "%s is not bound by flvis_amd" % name


def test_null_handles_are_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    cfg = flvis_amd.FlvisCfg()
    one = (C.c_int * 1)(0)
    out = C.c_void_p(0)
    null = C.c_void_p(0)
    assert lib.flvis_loop_closer_create_rigs(null, C.byref(cfg), null, 1, 1, null, C.byref(out)) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert not out.value
    assert lib.flvis_loop_closer_reset(null, 1, one) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_reset_rigs(null, 1, one, C.byref(cfg)) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_stream_cfg(null, 0, C.byref(cfg)) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_hip_pnp_ransac_rigs(null, null, null, null, 1, 1, null, 100, 2.0, 0.99, null, null, null,
                                         null) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_hip_lc_keyframe_landmarks_rigs(null, null, null, 640, 480, 1, 0, null, null, null, null, null, null, 1024, null, null, null,
                                                    null) == flvis_amd.FLVIS_ERR_INVALID_ARG
