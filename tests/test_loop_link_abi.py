"""CPU: links from stored keyframes are part of the C ABI -- flvis_loop_closer_link, flvis_hip_lc_select_maps_skip, flvis_lc_links_from_fix
and flvis_lc_link_reverse are declared in include/flvis_hip.h, exported by the library and bound by the ctypes harness; flvis_lc_link_query
has the same layout for a C++ caller of the header (tests/cpp/lc_link_query_layout.cpp, built with g++) as for the harness; NULL arguments
are refused without touching a device; and the two host helpers compute what their Python counterparts compute:
flvis_lc_link_reverse against tests/_pgo_synth.inv7 (which goes through the rotation matrix, so a quaternion counts as equal to its
negative), flvis_lc_links_from_fix against flvis_amd.links_from_fix."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import _binding
import _pgo_synth as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("flvis_loop_closer_link", "flvis_hip_lc_select_maps_skip", "flvis_lc_links_from_fix", "flvis_lc_link_reverse")


def _lib():
    import flvis_amd
    lib = flvis_amd.load_library()
    return lib


def test_entry_points_are_declared_exported_and_bound():
    import flvis_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flvis_hip.h")).read(), flags=re.S)
    src = _binding.source()
    lib = flvis_amd.load_library()
    for name in SYMBOLS + ("flvis_hip_lc_select_maps_skip_compact",):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "%s is not declared in include/flvis_hip.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        if name != "flvis_lc_links_from_fix":                                   # (Python has its own: flvis_amd.links_from_fix, compared below)
            assert re.search(r"\b%s\b" % name, src), "%s is not bound by flvis_amd" % name
    assert re.search(r"typedef\s+struct\s+flvis_lc_link_query\s*\{", txt)
    assert callable(flvis_amd.LoopCloser.link) and callable(flvis_amd.links_reverse) and callable(flvis_amd.Context.lc_select_maps_skip)


def test_struct_sizes_match_the_header():
    import flvis_amd
    exe = os.path.join(tempfile.mkdtemp(prefix="flvis_lc_link_query_"), "lc_link_query_layout")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lc_link_query_layout.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=30)
    assert out.returncode == 0
    got = dict((k, int(v)) for k, v in (line.split() for line in out.stdout.decode().splitlines()))
    assert got.pop("fix_in.sizeof") == C.sizeof(flvis_amd.FlvisLcFixIn) and got.pop("link.sizeof") == C.sizeof(flvis_amd.FlvisLcLink)
    assert got.pop("query.sizeof") == C.sizeof(flvis_amd.FlvisLcLinkQuery) == 24
    fields = [name for name, _ in flvis_amd.FlvisLcLinkQuery._fields_]
    assert sorted(got) == sorted("query." + f for f in fields)
    for name in fields:
        assert got["query." + name] == getattr(flvis_amd.FlvisLcLinkQuery, name).offset, name


def test_null_arguments_are_refused_without_a_device():
    import flvis_amd
    lib, INVALID = _lib(), flvis_amd.FLVIS_ERR_INVALID_ARG
    q = flvis_amd.FlvisLcLinkQuery(0, 1, -1, -1)
    fix, link, n = flvis_amd.FlvisLcFixIn(), flvis_amd.FlvisLcLink(0, 1, 0, 0, (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)), C.c_int(0)
    assert lib.flvis_loop_closer_link(None, 1, C.byref(q), 4, C.byref(fix), 1, C.byref(link), C.byref(n)) == INVALID
    assert lib.flvis_hip_lc_select_maps_skip(None, 1, None, 1, 1, None, None, None, 1, 0.0, None, None, None) == INVALID
    assert lib.flvis_lc_link_reverse(None, C.byref(link)) == INVALID and lib.flvis_lc_link_reverse(C.byref(link), None) == INVALID
    assert lib.flvis_lc_links_from_fix(None, 0, 0, 1, C.byref(link)) == -1
    assert lib.flvis_lc_links_from_fix(C.byref(fix), 0, 0, 1, None) == -1 and lib.flvis_lc_links_from_fix(C.byref(fix), 0, 0, -1, C.byref(link)) == -1
    assert lib.flvis_lc_links_from_fix(C.byref(fix), 0, 0, 0, None) == 0                              # (cap 0: out may be NULL)
    # a pose that cannot be inverted, and the output is left as it was
    out = flvis_amd.FlvisLcLink(7, 8, 9, 10, (C.c_double * 7)(1, 2, 3, 0, 0, 0, 1))
    for k, v in ((0, np.nan), (5, np.inf), (6, 0.0)):
        bad = flvis_amd.FlvisLcLink(0, 1, 0, 0, (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1))
        bad.pose7[k] = v
        assert lib.flvis_lc_link_reverse(C.byref(bad), C.byref(out)) == INVALID
        assert (out.seq_from, out.seq_to, out.kf_from, out.kf_to, list(out.pose7)) == (7, 8, 9, 10, [1, 2, 3, 0, 0, 0, 1])
    with __import__("pytest").raises(flvis_amd.FlvisError):
        flvis_amd.links_reverse([dict(seq_from=0, kf_from=0, seq_to=1, kf_to=0, pose=[0, 0, 0, 0, 0, 0, 0.0])])


def _poses(n, seed):
    """unit quaternions in every octant, translations within a metre: 1e-15 is then 4 ulp of the largest component"""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    return np.concatenate([rng.uniform(-1, 1, (n, 3)), q], 1)


def _pdiff(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    flip = -1.0 if np.dot(a[3:], b[3:]) < 0 else 1.0
    return max(np.abs(a[:3] - b[:3]).max(), np.abs(a[3:] - flip * b[3:]).max())


def test_link_reverse_against_inv7_and_twice():
    import flvis_amd
    lib = _lib()
    worst = [0.0, 0.0, 0.0]
    for k, p in enumerate(np.concatenate([_poses(40, 1), [[0, 0, 0, 0, 0, 0, 1.0], [0.5, -0.25, 1.0, 1, 0, 0, 0.0]]])):
        a = flvis_amd.FlvisLcLink(3, 1, 10 + k, 2 ** 40 + k, (C.c_double * 7)(*p))
        b, c = flvis_amd.FlvisLcLink(), flvis_amd.FlvisLcLink()
        assert lib.flvis_lc_link_reverse(C.byref(a), C.byref(b)) == flvis_amd.FLVIS_OK
        assert (b.seq_from, b.seq_to, b.kf_from, b.kf_to) == (1, 3, 2 ** 40 + k, 10 + k)
        worst[0] = max(worst[0], _pdiff(list(b.pose7), PS.inv7(p)))
        assert lib.flvis_lc_link_reverse(C.byref(b), C.byref(c)) == flvis_amd.FLVIS_OK
        assert (c.seq_from, c.seq_to, c.kf_from, c.kf_to) == (3, 1, 10 + k, 2 ** 40 + k)
        worst[1] = max(worst[1], np.abs(np.array(c.pose7) - p).max())                                 # (no sign flip on the way back)
        # the quaternion is normalised first: a scaled one gives the same link; and in place
        s = flvis_amd.FlvisLcLink(3, 1, 10 + k, 2 ** 40 + k, (C.c_double * 7)(*np.concatenate([p[:3], 3.0 * p[3:]])))
        assert lib.flvis_lc_link_reverse(C.byref(s), C.byref(s)) == flvis_amd.FLVIS_OK
        worst[2] = max(worst[2], np.abs(np.array(s.pose7) - np.array(b.pose7)).max())
        assert (s.seq_from, s.kf_from) == (1, 2 ** 40 + k)
    print("LINK-REVERSE worst difference: inv7 %.3g, twice %.3g, scaled quaternion %.3g" % tuple(worst))
    assert max(worst) <= 1e-15, worst
    # the Python form, on dicts
    l = dict(seq_from=0, kf_from=4, seq_to=2, kf_to=1, pose=list(_poses(1, 2)[0]))
    r = flvis_amd.links_reverse([l])[0]
    assert (r["seq_from"], r["kf_from"], r["seq_to"], r["kf_to"]) == (2, 1, 0, 4) and _pdiff(r["pose"], PS.inv7(np.array(l["pose"]))) <= 1e-15


def _fix(accepted, seqs=None):
    """a hand-made fix of len(accepted) candidates (the C struct and LoopCloser.localize_in's dict)"""
    import flvis_amd
    f = flvis_amd.FlvisLcFixIn()
    n = len(accepted)
    poses = _poses(8, 3)
    f.fix.n_landmarks, f.fix.n_candidates, f.fix.best = 500, n, -1
    for r in range(8):
        f.fix.cand_kf[r] = 2 ** 33 + 11 * r if r < n else -1
        f.cand_seq[r] = (seqs[r] if seqs else r % 3) if r < n else -1
        f.fix.cand_accepted[r] = int(r < n and accepted[r])
        f.fix.cand_inliers[r] = 30 + r
        for k in range(7):
            f.fix.cand_pose7[r][k] = poses[r][k]
        if f.fix.cand_accepted[r] and f.fix.best < 0:
            f.fix.best = r
    f.map = f.cand_seq[f.fix.best] if f.fix.best >= 0 else -1
    return f, flvis_amd.LoopCloser._fixes_in([f])[0]


def test_links_from_fix_equals_the_python_form():
    import flvis_amd
    lib = _lib()
    for accepted in ([], [False] * 5, [True] * 8, [True, False, True, True, False, True], [False, True]):
        f, d = _fix(accepted)
        want = flvis_amd.links_from_fix(d, 1, 2 ** 35 + 5)                     # (candidates of sequence 1 itself included: localize_in's)
        assert len(want) == sum(accepted)
        for cap in sorted({0, 1, max(0, len(want) - 1), len(want), 8}):
            out = (flvis_amd.FlvisLcLink * 9)()
            for l in out:
                l.seq_from = -7
            assert lib.flvis_lc_links_from_fix(C.byref(f), 1, 2 ** 35 + 5, cap, out) == len(want), (accepted, cap)
            got = [flvis_amd._link_dict(l) for l in out[:min(cap, len(want))]]
            assert got == want[:cap], (accepted, cap)
            assert all(l.seq_from == -7 for l in out[min(cap, len(want)):])    # nothing behind cap, or behind the count
