"""CPU: relocalisation is part of the C ABI -- flvis_loop_closer_localize, _localize_host and _set_drift are declared in
include/flvis_hip.h, exported by the library and bound by the ctypes harness, refuse a NULL closer without touching a device, and
flvis_lc_fix has the same layout for a C++ caller of the header (tests/cpp/lc_fix_layout.cpp, built with g++) as for the harness."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("flvis_loop_closer_localize", "flvis_loop_closer_localize_host", "flvis_loop_closer_set_drift")


def test_entry_points_are_declared_exported_and_bound():
    import flvis_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    src = _binding.source()
    lib = flvis_amd.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared in include/flvis_hip.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert re.search(r"_lib\.%s\b" % name, src), "%s is not bound by flvis_amd" % name
    for name in ("localize", "localize_host", "set_drift"):
        assert callable(getattr(flvis_amd.LoopCloser, name))


def test_null_closer_is_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    null = C.c_void_p(0)
    one = (C.c_int * 1)(0)
    fix = flvis_amd.FlvisLcFix()
    img = flvis_amd.FlvisImage()
    T = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
    assert lib.flvis_loop_closer_localize(null, 1, one, null, null, 4, C.byref(fix)) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_localize_host(null, 1, one, C.byref(img), C.byref(img), 4, C.byref(fix)) == flvis_amd.FLVIS_ERR_INVALID_ARG
    assert lib.flvis_loop_closer_set_drift(null, 0, T) == flvis_amd.FLVIS_ERR_INVALID_ARG


def test_flvis_lc_fix_layout_matches_the_header():
    import flvis_amd
    exe = os.path.join(tempfile.mkdtemp(prefix="flvis_lc_fix_"), "lc_fix_layout")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lc_fix_layout.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=30)
    assert out.returncode == 0
    got = dict((k, int(v)) for k, v in (line.split() for line in out.stdout.decode().splitlines()))
    assert got.pop("sizeof") == C.sizeof(flvis_amd.FlvisLcFix)
    assert got.pop("FLVIS_LC_FIX_CAND") == flvis_amd.FLVIS_LC_FIX_CAND == 8
    fields = [name for name, _ in flvis_amd.FlvisLcFix._fields_]
    assert sorted(got) == sorted(fields)
    for name in fields:
        assert got[name] == getattr(flvis_amd.FlvisLcFix, name).offset, name
