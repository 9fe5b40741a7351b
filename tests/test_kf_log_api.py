"""CPU: the keyframe log's boundary (flvis_keyframe_log_*, flvis_loop_closer_add_logged) -- declared in the header, exported by the
library, wrapped in Python -- and the numpy restatement the GPU tests compare against (tests/_kf_log.py) on hand-made sequences."""
import os
import re

import numpy as np

import _kf_log as KL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("flvis_keyframe_log_enable", "flvis_keyframe_log_clear", "flvis_keyframe_log_info", "flvis_keyframe_log_get",
           "flvis_keyframe_log_images", "flvis_loop_closer_add_logged")


def test_the_entry_points_are_declared_and_exported():
    import flvis_amd
    hdr = open(os.path.join(ROOT, "include", "flvis_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = flvis_amd.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s + " is not declared in include/flvis_hip.h"
        assert hasattr(lib, s), s + " is not exported"
    # the header states what the issue asks it to state
    assert "EQUIVALENCE" in hdr and "LIFETIME clause" in hdr and "feeding twice" in hdr


def test_the_python_wrappers_exist():
    import flvis_amd
    for name in ("keyframe_msg", "keyframe_log_enable", "keyframe_log_clear", "keyframe_log_info", "keyframe_log_get", "keyframe_log_images"):
        assert callable(getattr(flvis_amd.Tracker, name, None)), "Tracker." + name
    assert callable(getattr(flvis_amd.LoopCloser, "add_logged", None))
    # flvis_keyframe as ctypes sees it: the C struct's layout on this ABI (int64, int8 + padding, double, two 32-byte images, ...)
    import ctypes as C
    K = flvis_amd.FlvisKeyframe
    assert C.sizeof(flvis_amd.FlvisImage) == 32
    assert (K.frame_id.offset, K.command.offset, K.stamp.offset, K.img0.offset, K.img1.offset) == (0, 8, 16, 24, 56)
    assert (K.lm_count.offset, K.lm_id.offset, K.lm_2d.offset, K.lm_3d.offset, K.T_c_w.offset) == (88, 96, 104, 112, 120)
    assert C.sizeof(K) == 176


def test_record_is_a_prefix_and_the_first_drop_ends_it():
    m = [KL.fake_msg(k) for k in range(5)]
    hist = [None, m[0], None, None, m[1], m[2], None, m[3], m[4], None]
    full = KL.record(hist, 8)
    assert full["dropped"] == 0 and [e["frame_id"] for e in full["entries"]] == [x["frame_id"] for x in m]
    two = KL.record(hist, 2)
    assert two["dropped"] == 3 and [e["frame_id"] for e in two["entries"]] == [m[0]["frame_id"], m[1]["frame_id"]]
    assert KL.record(hist, 0) == dict(entries=[], dropped=5)
    assert KL.record([None, None], 4) == dict(entries=[], dropped=0)
    # exactly full is no drop; one more keyframe is one
    assert KL.record(hist, 5)["dropped"] == 0 and KL.record(hist + [KL.fake_msg(9)], 5)["dropped"] == 1
    # a record that was cleared starts at entry 0 of what follows
    later = KL.record(hist[6:], 2)
    assert [e["frame_id"] for e in later["entries"]] == [m[3]["frame_id"], m[4]["frame_id"]] and later["dropped"] == 0


def test_rounds_take_entry_r_of_every_stream_that_has_one():
    assert KL.rounds([3, 0, 1, 2]) == [[0, 2, 3], [0, 3], [0]]
    assert KL.rounds([0, 0]) == [] and KL.rounds([]) == []
    assert KL.rounds([2, 2]) == [[0, 1], [0, 1]]


def test_differences_compare_every_field_by_its_bits():
    a = KL.fake_msg(1)
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    assert KL.differences(a, b) == []
    b["pose7"][3] = np.nextafter(b["pose7"][3], 1.0)
    b["img1"][2, 5] ^= 1
    b["stamp"] = np.nextafter(b["stamp"], 1.0)
    assert KL.differences(a, b) == ["stamp", "pose7", "img1"]
    c = dict(a, lm_id=a["lm_id"][:-1])
    assert KL.differences(a, c) == ["lm_id"]
    z0, z1 = dict(a, stamp=0.0), dict(a, stamp=-0.0)                                   # equal as numbers, not as bits
    assert KL.differences(z0, z1) == ["stamp"]
