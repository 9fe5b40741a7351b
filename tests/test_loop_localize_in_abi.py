"""CPU: localisation in another sequence's map is part of the C ABI -- flvis_loop_closer_localize_in, _localize_in_host and the two
kernel-level steps flvis_hip_bow_score_jobs_at / flvis_hip_lc_select_maps are declared in include/flvis_hip.h, exported by the library and
bound by the ctypes harness, the closer's calls refuse a NULL closer without touching a device, and flvis_lc_fix_in has the same layout
for a C++ caller of the header (tests/cpp/lc_fix_in_layout.cpp, built with g++) as for the harness."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("flvis_loop_closer_localize_in", "flvis_loop_closer_localize_in_host", "flvis_hip_bow_score_jobs_at", "flvis_hip_lc_select_maps")


def test_entry_points_are_declared_exported_and_bound():
    import flvis_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    src = _binding.source()
    lib = flvis_amd.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared in include/flvis_hip.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert re.search(r"_lib\.%s\b" % name, src), "%s is not bound by flvis_amd" % name
    assert re.search(r"#define\s+FLVIS_LC_ALL_MAPS\s+\(-1\)", txt) and flvis_amd.FLVIS_LC_ALL_MAPS == -1
    for name in ("localize_in", "localize_in_host"):
        assert callable(getattr(flvis_amd.LoopCloser, name))
    for name in ("bow_score_jobs_at", "lc_select_maps"):
        assert callable(getattr(flvis_amd.Context, name))


def test_null_closer_is_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    null = C.c_void_p(0)
    one = (C.c_int * 1)(0)
    fix = flvis_amd.FlvisLcFixIn()
    img = flvis_amd.FlvisImage()
    assert lib.flvis_loop_closer_localize_in(null, 1, one, one, null, null, 4, C.byref(fix)) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_localize_in_host(null, 1, one, one, C.byref(img), C.byref(img), 4, C.byref(fix)) == \
        flvis_amd.FLVIS_ERR_INVALID_ARG
    # ... and the kernel-level steps a NULL context
    assert lib.flvis_hip_bow_score_jobs_at(null, 1, one, null, null, null, 8, null) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_hip_lc_select_maps(null, 1, null, 1, 1, null, null, 1, 0.0, null, null, null) == flvis_amd.FLVIS_ERR_INVALID_ARG


def test_flvis_lc_fix_in_layout_matches_the_header():
    import flvis_amd
    exe = os.path.join(tempfile.mkdtemp(prefix="flvis_lc_fix_in_"), "lc_fix_in_layout")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lc_fix_in_layout.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=30)
    assert out.returncode == 0
    got = dict((k, int(v)) for k, v in (line.split() for line in out.stdout.decode().splitlines()))
    assert got.pop("sizeof") == C.sizeof(flvis_amd.FlvisLcFixIn)
    assert got.pop("sizeof_fix") == C.sizeof(flvis_amd.FlvisLcFix)          # nested as it is: its own layout is pinned by its own test
    assert got.pop("FLVIS_LC_ALL_MAPS") == flvis_amd.FLVIS_LC_ALL_MAPS == -1
    fields = [name for name, _ in flvis_amd.FlvisLcFixIn._fields_]
    assert fields[0] == "fix" and got["fix"] == 0
    assert sorted(got) == sorted(fields)
    for name in fields:
        assert got[name] == getattr(flvis_amd.FlvisLcFixIn, name).offset, name
