"""DBoW3 vocabulary files (flvis_voc_file_*, host only) and the vocabulary a device training run returns."""
import ctypes as C
import os

import numpy as np

from ._loader import FLVIS_OK, FlvisError, load_library


def read_vocabulary_file(path):
    """flvis_voc_file_* (host only): a DBoW3 vocabulary file as the flat arrays `Context.bow_set_vocabulary` takes.

    Returns a dict: child_ptr, child_idx, desc [n,32], weight, word_id (-1 on inner nodes), k, L, scoring, weighting, n_words,
    layout ("binary" | "binary-quicklz" | "text" | "yaml")."""
    lib = load_library()
    h = C.c_void_p(0)
    err = C.create_string_buffer(512)
    rc = lib.flvis_voc_file_open(os.fsencode(path), C.byref(h), err, 512)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_voc_file_open(%s): %s" % (path, err.value.decode(errors="replace") or rc))
    try:
        return _voc_handle_dict(lib, h)
    finally:
        lib.flvis_voc_file_close(h)


_VOC_LAYOUTS = ["binary", "binary-quicklz", "text", "yaml", "trained"]


def _voc_handle_dict(lib, h):
    """the content of a flvis_voc_file handle, copied out"""
    info = (C.c_int * 8)()
    lib.flvis_voc_file_info(h, info)
    n, n_words, k, L, scoring, weighting, n_edges, layout = list(info)
    ptrs = [C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_double)(), C.POINTER(C.c_int)()]
    lib.flvis_voc_file_arrays(h, *[C.byref(q) for q in ptrs])
    take = lambda q, cnt, dt: np.ctypeslib.as_array(q, shape=(cnt,)).astype(dt, copy=True) if cnt else np.zeros(0, dt)
    return {"child_ptr": take(ptrs[0], n + 1, np.int32), "child_idx": take(ptrs[1], n_edges, np.int32),
            "desc": take(ptrs[2], n * 32, np.uint8).reshape(n, 32), "weight": take(ptrs[3], n, np.float64),
            "word_id": take(ptrs[4], n, np.int32), "k": k, "L": L, "scoring": scoring, "weighting": weighting,
            "n_words": n_words, "layout": _VOC_LAYOUTS[layout]}


def save_vocabulary_file(path, arrays, k, L, scoring=0, weighting=0):
    """flvis_voc_file_save_arrays (host only): the flat arrays (child_ptr, child_idx, desc [n,32], weight, word_id) as an uncompressed
    binary .dbow3 file, byte for byte what DBoW3's Vocabulary::save(path, false) writes."""
    lib = load_library()
    cp = np.ascontiguousarray(arrays[0], np.int32)
    ci = np.ascontiguousarray(arrays[1], np.int32)
    ds = np.ascontiguousarray(arrays[2], np.uint8)
    wt = np.ascontiguousarray(arrays[3], np.float64)
    wi = np.ascontiguousarray(arrays[4], np.int32)
    n = len(cp) - 1
    if ds.shape != (n, 32) or len(wt) != n or len(wi) != n or len(ci) != n - 1:
        raise FlvisError("save_vocabulary_file: the arrays do not describe one tree of %d nodes" % n)
    rc = lib.flvis_voc_file_save_arrays(os.fsencode(path), 0, n, cp.ctypes.data, ci.ctypes.data, ds.ctypes.data, wt.ctypes.data,
                                        wi.ctypes.data, int(k), int(L), int(scoring), int(weighting))
    if rc != FLVIS_OK:
        raise FlvisError("flvis_voc_file_save_arrays(%s) failed (%d)" % (path, rc))


def convert_vocabulary_file(src, dst):
    """flvis_voc_file_open + flvis_voc_file_save (host only): any readable vocabulary file rewritten as an uncompressed .dbow3."""
    lib = load_library()
    h = C.c_void_p(0)
    err = C.create_string_buffer(512)
    rc = lib.flvis_voc_file_open(os.fsencode(src), C.byref(h), err, 512)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_voc_file_open(%s): %s" % (src, err.value.decode(errors="replace") or rc))
    try:
        rc = lib.flvis_voc_file_save(h, os.fsencode(dst), 0)
        if rc != FLVIS_OK:
            raise FlvisError("flvis_voc_file_save(%s) failed (%d)" % (dst, rc))
    finally:
        lib.flvis_voc_file_close(h)


class TrainedVocabulary:
    """What Context.voc_train returns: .arrays (child_ptr, child_idx, desc, weight, word_id with 0 on inner nodes -- the 5-tuple
    Context.bow_set_vocabulary takes), .info (the dict read_vocabulary_file returns, word_id -1 on inner nodes), .stats (descriptors,
    nodes, words, passes, capped, empty, trivial, launches), .save(path), .close()."""
    STATS = ("descriptors", "nodes", "words", "passes", "capped", "empty", "trivial", "launches")

    def __init__(self, lib, h, stats):
        self._lib, self._h = lib, h
        self.info = _voc_handle_dict(lib, h)
        self.stats = dict(zip(self.STATS, [int(x) for x in stats]))
        i = self.info
        self.arrays = (i["child_ptr"], i["child_idx"], i["desc"], i["weight"], np.maximum(i["word_id"], 0).astype(np.int32))

    def save(self, path):
        """flvis_voc_file_save: an uncompressed binary .dbow3 file"""
        if not self._h:
            raise FlvisError("TrainedVocabulary.save: closed")
        rc = self._lib.flvis_voc_file_save(self._h, os.fsencode(path), 0)
        if rc != FLVIS_OK:
            raise FlvisError("flvis_voc_file_save(%s) failed (%d)" % (path, rc))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.flvis_voc_file_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
