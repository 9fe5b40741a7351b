"""CPU: the front-end's solver calls on caller arrays are part of the C ABI -- declared in include/flvis_hip.h with the argument lists the
integration guide shows, named in the header's opening list, exported by the library, bound by flvis_amd.Context -- and refuse a call
without a context instead of touching a device."""
import ctypes as C
import os
import re

import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "flvis_hip_find_fundamental_ransac":
        "flvis_ctx* ctx, const float* d_m1, const float* d_m2, const int* d_count, int cap, int n_sets, double thr_px, double confidence, "
        "uint8_t* d_mask, int* d_n_inliers",
    "flvis_hip_optimize_in_frame":
        "flvis_ctx* ctx, const double* d_lm_3d_w, const double* d_lm_2d_undistort, const int64_t* d_lm_id, const int* d_count, int cap, "
        "int n_sets, const double* h_K4, int n_K, double* d_pose7, uint8_t* d_ok",
    "flvis_hip_undistort_points":
        "flvis_ctx* ctx, const float* d_src, const int* d_count, int cap, int n_sets, const double* h_K4, const double* h_D4, "
        "const double* h_R9, const double* h_P12, int n_cam, float* d_dst",
    "flvis_hip_project_points":
        "flvis_ctx* ctx, const float* d_p3d, const int* d_count, int cap, int n_sets, const double* h_pose7, const double* h_K4, "
        "const double* h_D4, int n_cam, float* d_dst",
}
WRAPPERS = {"flvis_hip_find_fundamental_ransac": "find_fundamental_ransac", "flvis_hip_optimize_in_frame": "optimize_in_frame",
            "flvis_hip_undistort_points": "undistort_points", "flvis_hip_project_points": "project_points"}


def _header():
    return open(os.path.join(ROOT, "include", "flvis_hip.h")).read()


def test_calls_are_declared_with_their_argument_lists():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, want in DECLS.items():
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
        assert m, "%s is not declared in include/flvis_hip.h" % name
        assert re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", m.group(1))).strip() == want, name


def test_calls_are_in_the_opening_list_with_their_anchors():
    head = _header().split("*/")[0]
    for name, anchor in (("flvis_hip_find_fundamental_ransac", "lkorb_tracking.cpp:134"), ("flvis_hip_optimize_in_frame", "optimize_in_frame.cpp:10-91"),
                         ("flvis_hip_undistort_points", "lkorb_tracking.cpp:87"), ("flvis_hip_project_points", "lkorb_tracking.cpp:58")):
        line = [k for k, l in enumerate(head.splitlines()) if name in l]
        assert line, "%s is missing from the header's list of kernel-level entry points" % name
        assert anchor in "\n".join(head.splitlines()[line[0]:line[0] + 2]), (name, anchor)


def test_calls_are_exported_and_bound():
    import flvis_amd
    lib = flvis_amd.load_library()
    src = _binding.source()
    for name, wrapper in WRAPPERS.items():
        assert hasattr(lib, name), "%s is not exported" % name
        assert re.search(r"_lib\.%s\b" % name, src), "%s is not bound by flvis_amd" % name
        assert callable(getattr(flvis_amd.Context, wrapper))


def test_null_handle_is_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    null = C.c_void_p(0)
    K = (C.c_double * 4)(384, 385, 320, 240)
    bad = flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_hip_find_fundamental_ransac(null, null, null, null, 32, 1, 5.0, 0.99, null, null) == bad
    assert lib.flvis_hip_optimize_in_frame(null, null, null, null, null, 32, 1, K, 1, null, null) == bad
    assert lib.flvis_hip_undistort_points(null, null, null, 32, 1, K, K, null, null, 1, null) == bad
    assert lib.flvis_hip_project_points(null, null, null, 32, 1, null, K, K, 1, null) == bad
