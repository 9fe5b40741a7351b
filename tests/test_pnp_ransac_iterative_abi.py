"""CPU: the test hook of the PnP RANSAC's iterative branch is part of the C ABI -- declared in include/flvis_hip.h, exported by the library
and bound by the ctypes harness -- and refuses a call without a context instead of touching a device."""
import ctypes as C
import os
import re

import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flvis_hip_debug_pnp_ransac_iterative"


def test_hook_is_declared_exported_and_bound():
    import flvis_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, txt), "%s is not declared in include/flvis_hip.h" % NAME
    assert hasattr(flvis_amd.load_library(), NAME), "%s is not exported" % NAME
    assert re.search(r"_lib\.%s\b" % NAME, _binding.source()), "%s is not bound by flvis_amd" % NAME
    assert callable(flvis_amd.Context.debug_pnp_ransac_iterative)


def test_hook_takes_the_arguments_of_pnp_ransac_with_guesses_for_seeds():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    args = {n: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, txt, re.S).group(1)))
            for n in (NAME, "flvis_hip_pnp_ransac")}
    assert args[NAME] == args["flvis_hip_pnp_ransac"].replace("const uint64_t* h_seeds", "const double* h_guess7")


def test_null_handle_is_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    null = C.c_void_p(0)
    K = (C.c_double * 4)(384, 385, 320, 240)
    g = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
    fn = getattr(lib, NAME)
    assert fn(null, null, null, null, 1, 1, null, 100, 3.0, 0.99, null, null, null, null) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert fn(null, null, null, null, 32, 1, K, 100, 3.0, 0.99, g, null, null, null) == flvis_amd.FLVIS_ERR_INVALID_ARG
