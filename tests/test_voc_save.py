"""The vocabulary writer (flvis_voc_file_save / flvis_voc_file_save_arrays, host only): layout 0 is the uncompressed binary stream of
Vocabulary::toStream(out, false) (3rdPartLib/DBow3/src/Vocabulary.cpp:1180-1256), byte for byte what the independent writer of
tests/_vocfile.py emits, and what flvis_voc_file_open reads back bit for bit; a handle opened from any readable file can be saved, which
converts it to .dbow3."""
import ctypes as C
import os

import numpy as np
import pytest

import _voc as V
import _vocfile as VF
import flvis_amd

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INVALID = flvis_amd.FLVIS_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def voc():
    return V.build_vocabulary(V.make_keyframes(3, n_img=6), k=6, depth=3)


def _save_arrays(lib, path, layout, voc, k, L, null=None):
    cp, ci, ds, wt, wi = (np.ascontiguousarray(a, t) for a, t in zip(voc, (np.int32, np.int32, np.uint8, np.float64, np.int32)))
    ptrs = [cp.ctypes.data, ci.ctypes.data, ds.ctypes.data, wt.ctypes.data, wi.ctypes.data]
    if null is not None and null >= 0:
        ptrs[null] = None
    return lib.flvis_voc_file_save_arrays(None if null == -1 else os.fsencode(path), layout, len(cp) - 1, *ptrs, k, L, 0, 0)


def _same(got, voc):
    child_ptr, child_idx, desc, weight, word_id = voc
    leaf = np.diff(child_ptr) == 0
    assert np.array_equal(got["child_ptr"], child_ptr) and np.array_equal(got["child_idx"], child_idx)
    assert np.array_equal(got["desc"][1:], np.asarray(desc)[1:])
    assert np.array_equal(got["weight"][1:].view(np.uint64), np.asarray(weight, np.float64)[1:].view(np.uint64))     # bit for bit
    assert np.array_equal(got["word_id"][leaf], np.asarray(word_id)[leaf]) and np.all(got["word_id"][~leaf] == -1)


def test_writer_is_byte_identical_and_reads_back(voc, tmp_path):
    lib = flvis_amd.load_library()
    mine, want = str(tmp_path / "mine.dbow3"), str(tmp_path / "want.dbow3")
    assert _save_arrays(lib, mine, 0, voc, 6, 3) == 0
    VF.write_binary(want, voc, 6, 3)
    assert open(mine, "rb").read() == open(want, "rb").read()
    got = flvis_amd.read_vocabulary_file(mine)
    assert got["layout"] == "binary" and (got["k"], got["L"], got["scoring"], got["weighting"]) == (6, 3, 0, 0)
    _same(got, voc)
    # the Python wrapper writes the same file
    flvis_amd.save_vocabulary_file(mine, voc, 6, 3)
    assert open(mine, "rb").read() == open(want, "rb").read()


def test_writer_refusals(voc, tmp_path):
    lib = flvis_amd.load_library()
    p = str(tmp_path / "no.dbow3")
    for layout in (1, 2, 3):
        assert _save_arrays(lib, p, layout, voc, 6, 3) == INVALID
    for null in (-1, 0, 1, 2, 3, 4):
        assert _save_arrays(lib, p, 0, voc, 6, 3, null=null) == INVALID
    assert lib.flvis_voc_file_save(None, os.fsencode(p), 0) == INVALID
    assert not os.path.exists(p)
    # links that do not form a tree are refused, not written
    bad = (voc[0], np.full_like(voc[1], 1), voc[2], voc[3], voc[4])
    assert _save_arrays(lib, p, 0, bad, 6, 3) == INVALID and not os.path.exists(p)
    assert _save_arrays(lib, str(tmp_path / "no" / "such" / "dir.dbow3"), 0, voc, 6, 3) == -5      # FLVIS_ERR_CONFIG


def test_converter_from_the_quicklz_golden(tmp_path):
    src = os.path.join(GOLD, "voc_k6_quicklz.dbow3")
    lib = flvis_amd.load_library()
    h = C.c_void_p(0)
    assert lib.flvis_voc_file_open(os.fsencode(src), C.byref(h), None, 0) == 0
    dst = str(tmp_path / "plain.dbow3")
    try:
        for layout in (1, 2, 3):
            assert lib.flvis_voc_file_save(h, os.fsencode(dst), layout) == INVALID
        assert lib.flvis_voc_file_save(h, None, 0) == INVALID
        assert lib.flvis_voc_file_save(h, os.fsencode(dst), 0) == 0
    finally:
        lib.flvis_voc_file_close(h)
    a = flvis_amd.read_vocabulary_file(src)
    arrays = (a["child_ptr"], a["child_idx"], a["desc"], a["weight"], a["word_id"])
    raw = open(dst, "rb").read()
    assert raw[:13] == VF.struct.pack("<Q?I", VF.MAGIC, False, len(a["child_ptr"]) - 1)
    assert raw[13:] == VF.payload(arrays, a["k"], a["L"], a["scoring"], a["weighting"])      # the golden's decompressed payload
    b = flvis_amd.read_vocabulary_file(dst)
    assert a["layout"] == "binary-quicklz" and b["layout"] == "binary"
    for key in ("child_ptr", "child_idx", "desc", "word_id", "k", "L", "scoring", "weighting", "n_words"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["weight"].view(np.uint64), b["weight"].view(np.uint64))
    # the wrapper does the same
    dst2 = str(tmp_path / "plain2.dbow3")
    flvis_amd.convert_vocabulary_file(src, dst2)
    assert open(dst2, "rb").read() == raw


def test_symbols_exported():
    lib = flvis_amd.load_library()
    for name in ("flvis_voc_file_save", "flvis_voc_file_save_arrays", "flvis_hip_voc_train"):
        assert hasattr(lib, name), name
