"""CPU: merging sequences' maps is part of the C ABI -- flvis_loop_closer_merge is declared in include/flvis_hip.h, exported by the library
and bound by the ctypes harness (LoopCloser.merge, links_from_fix), it refuses a NULL closer without touching a device, and flvis_lc_link /
flvis_lc_merge have the same layout for a C++ caller of the header (tests/cpp/lc_link_layout.cpp, built with g++) as for the harness."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    import flvis_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    src = _binding.source()
    lib = flvis_amd.load_library()
    name = "flvis_loop_closer_merge"
    assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared in include/flvis_hip.h" % name
    assert hasattr(lib, name), "%s is not exported" % name
    assert re.search(r"_lib\.%s\b" % name, src), "%s is not bound by flvis_amd" % name
    for struct in ("flvis_lc_link", "flvis_lc_merge"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct, txt), struct
    assert callable(flvis_amd.LoopCloser.merge) and callable(flvis_amd.links_from_fix)


def test_null_closer_is_refused_without_a_device():
    import flvis_amd
    lib = flvis_amd.load_library()
    ptr, seq = (C.c_int * 2)(0, 2), (C.c_int * 2)(0, 1)
    link = flvis_amd.FlvisLcLink(0, 1, 0, 0, (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1))
    out = flvis_amd.FlvisLcMerge()
    assert lib.flvis_loop_closer_merge(None, 1, ptr, seq, 1, C.byref(link), 100, C.byref(out), None) == flvis_amd.FLVIS_ERR_INVALID_ARG


def test_links_from_fix_takes_the_accepted_candidates():
    import flvis_amd
    cand = lambda seq, kf, ok: dict(seq=seq, kf=kf, score=0.5, n_matches=40, n_inliers=30, accepted=ok, pose=[0.1 * kf, 0, 0, 0, 0, 0, 1.0])
    fix = dict(candidates=[cand(0, 3, True), cand(2, 5, False), cand(0, 4, True)], best=0, map=0)
    links = flvis_amd.links_from_fix(fix, 1, 7)
    assert [(l["seq_from"], l["kf_from"], l["seq_to"], l["kf_to"]) for l in links] == [(0, 3, 1, 7), (0, 4, 1, 7)]
    assert links[1]["pose"] == [0.4, 0, 0, 0, 0, 0, 1.0]
    assert flvis_amd.links_from_fix(dict(candidates=[], best=-1, map=-1), 1, 0) == []


def test_struct_layouts_match_the_header():
    import flvis_amd
    exe = os.path.join(tempfile.mkdtemp(prefix="flvis_lc_link_"), "lc_link_layout")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lc_link_layout.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=30)
    assert out.returncode == 0
    got = dict((k, int(v)) for k, v in (line.split() for line in out.stdout.decode().splitlines()))
    for prefix, cls in (("link", flvis_amd.FlvisLcLink), ("merge", flvis_amd.FlvisLcMerge)):
        mine = dict((k.split(".", 1)[1], v) for k, v in got.items() if k.startswith(prefix + "."))
        assert mine.pop("sizeof") == C.sizeof(cls)
        fields = [name for name, _ in cls._fields_]
        assert sorted(mine) == sorted(fields)
        for name in fields:
            assert mine[name] == getattr(cls, name).offset, (prefix, name)
