"""CPU: flvis_hip_lkorb_tracking is part of the C ABI -- declared in include/flvis_hip.h with its argument list, named in the header's
opening list, exported by the library, bound by flvis_amd.Context.lkorb_tracking with the documented argument order -- and refuses a
call without a context instead of touching a device."""
import ctypes as C
import inspect
import os
import re

import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flvis_hip_lkorb_tracking"
DECL = ("flvis_ctx* ctx, const flvis_cfg* cfg, const uint8_t* d_img_from, const uint8_t* d_img_to, int n_sets, const float* d_from_2d_plane, "
        "const float* d_from_2d_undistort, const float* d_from_3d_w, const uint8_t* d_from_flags, const int* d_count, int cap, "
        "const double* h_guess7, const uint8_t* h_use_guess, int* d_to_from, float* d_to_2d_plane, float* d_to_2d_undistort, uint8_t* d_to_flags, "
        "uint8_t* d_mask_F, int* d_counts4, double* d_pose7, uint8_t* d_ret")
WRAPPER_ARGS = ["self", "cfg", "img_from", "img_to", "from_2d_plane", "from_2d_undistort", "from_3d_w", "from_flags", "count", "guess7", "use_guess",
                "pose7", "out"]


def _header():
    return open(os.path.join(ROOT, "include", "flvis_hip.h")).read()


def test_call_is_declared_with_its_argument_list():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, txt, re.S)
    assert m, "%s is not declared in include/flvis_hip.h" % NAME
    assert re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", m.group(1))).strip() == DECL


def test_call_is_in_the_opening_list_with_its_anchor():
    head = _header().split("*/")[0]
    line = [l for l in head.splitlines() if NAME in l]
    assert line and "lkorb_tracking.cpp:9-202" in line[0]


def test_call_is_exported_and_bound():
    import flvis_amd
    lib = flvis_amd.load_library()
    assert hasattr(lib, NAME), "%s is not exported" % NAME
    src = _binding.source()
    assert re.search(r"_lib\.%s\b" % NAME, src)
    assert list(inspect.signature(flvis_amd.Context.lkorb_tracking).parameters) == WRAPPER_ARGS
    assert flvis_amd.FLVIS_ERR_CONFIG == -5


def test_null_handle_is_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    f = getattr(lib, NAME)
    assert f(*([None] * 4), 1, *([None] * 5), 32, *([None] * 10)) == flvis_amd.FLVIS_ERR_INVALID_ARG
