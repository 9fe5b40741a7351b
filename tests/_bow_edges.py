"""Inputs that drive the bag-of-words transform (k_bow_words / voc_descend, k_bow_vector) and the L1 score kernels (bow_score_wave in
k_bow_score, k_bow_score_jobs<3> and <4>) to their edges.  No GPU is needed here: tests/test_bow_edges_inputs.py checks every
recipe with the CPU oracle (oracle/ref_bow.cpp) and the plain-Python restatements of tests/_voc.py, and shows by restated alternative
rules which mistake each recipe would catch; tests/test_gpu_bow_edges.py compares the kernels against what is built here.

A transform recipe is a list of Parts.  A Part is one vocabulary (the five flat arrays of flvis_hip_bow_set_vocabulary) and one launch:
desc [n, dcap, 32], the RAW count [n] handed to the call (it may exceed dcap or be negative), vcap, a name per row.  The keyframe a row
stands for is desc[i, :clip(count[i], 0, dcap)].  A score recipe is a Store of hand-made sparse vectors with the query / database
layout the score calls take.  Every recipe asserts its own defining property when it is built: one that drifts fails there instead of
testing nothing."""
import ctypes as C
import functools

import numpy as np

import _oracle as O
import _voc as V
from test_oracle_bow import RefVoc, ref_score

BOW_MAXF = 2048             # BOW_MAXF of loop_kernels.hip: descriptors per keyframe


# ---- containers ----------------------------------------------------------------------------------------------------------------
class Part:
    def __init__(self, name, voc, kfs, dcap, vcap=None, counts=None):
        """kfs: [(row name, [m, 32] uint8 with m <= dcap)]; counts: raw counts (default: the lengths)"""
        self.name, self.voc, self.dcap = name, tuple(np.ascontiguousarray(a) for a in voc), int(dcap)
        self.names = [k for k, _ in kfs]
        assert len(set(self.names)) == len(self.names)
        n = len(kfs)
        self.desc = np.zeros((n, dcap, 32), np.uint8)
        for i, (_, d) in enumerate(kfs):
            assert d.dtype == np.uint8 and d.ndim == 2 and d.shape[1] == 32 and len(d) <= dcap, (name, i)
            self.desc[i, :len(d)] = d
        self.count = np.array([len(d) for _, d in kfs] if counts is None else counts, np.int32)
        assert len(self.count) == n
        self.n_words = int(self.voc[4].max()) + 1
        self.vcap = int(min(dcap, self.n_words) if vcap is None else vcap)
        assert 0 < dcap <= BOW_MAXF and self.vcap >= min(dcap, self.n_words)

    def row(self, name):
        return self.names.index(name)

    def keyframe(self, i):
        """the descriptors row i stands for: counts above dcap read as dcap, below 0 as 0"""
        return self.desc[i, :int(np.clip(self.count[i], 0, self.dcap))]

    def keyframes(self):
        return [self.keyframe(i) for i in range(len(self.names))]


class Recipe:
    def __init__(self, name, parts, **figures):
        self.name, self.parts, self.figures = name, parts, figures

    def part(self, name):
        return [p for p in self.parts if p.name == name][0]


class Store:
    """vectors: [(ids int32 ascending, vals float64) or None (absent: nnz -1)]; queries: {name: index}; db: {query name: (first, n)}"""

    def __init__(self, name, vectors, queries, db, vcap):
        self.name, self.vectors, self.queries, self.db, self.vcap = name, vectors, queries, db, vcap
        n = len(vectors)
        self.ids = np.full((n, vcap), -1, np.int32)
        self.vals = np.zeros((n, vcap))
        self.nnz = np.full(n, -1, np.int32)
        for i, v in enumerate(vectors):
            if v is None:
                continue
            assert len(v[0]) == len(v[1]) <= vcap and np.all(np.diff(v[0]) > 0), (name, i)
            self.nnz[i] = len(v[0])
            self.ids[i, :len(v[0])], self.vals[i, :len(v[0])] = v

    def vec(self, i):
        v = self.vectors[i]
        return (np.zeros(0, np.int32), np.zeros(0)) if v is None else v


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def ref_words(rv, d):
    """oracle (rv: a RefVoc): the word id of every descriptor and the weight of the node it ends at, both as word_of of
    oracle/ref_bow.cpp finds them (the discrete half of the transform; weight <= 0: a stopped descriptor)"""
    d = np.ascontiguousarray(d, np.uint8)
    w = np.zeros(len(d), np.int32)
    wt = np.zeros(len(d))
    O.lib().ref_voc_words_weights.restype = None
    O.lib().ref_voc_words_weights(rv.h, len(d), d.ctypes.data_as(C.POINTER(C.c_uint8)), w.ctypes.data_as(C.POINTER(C.c_int)),
                                  wt.ctypes.data_as(C.POINTER(C.c_double)))
    return w, wt


def ref_transform(part):
    """oracle: [(ids, vals)] per row of the part"""
    rv = RefVoc(part.voc)
    return [rv.transform(k) for k in part.keyframes()]


def ref_scores(store, q, first, n):
    """oracle: score(query vector q, store vector first + j) for j < n; an absent vector on either side scores 0.0"""
    out = np.zeros(n)
    for j in range(n):
        if store.vectors[q] is not None and store.vectors[first + j] is not None:
            out[j] = ref_score(store.vec(q), store.vec(first + j))
    return out


# ---- restatements with the rule as a parameter (the alternatives are what a subtly wrong kernel would compute) --------------------
def _pm1(d):
    return 1.0 - 2.0 * np.unpackbits(np.ascontiguousarray(d, np.uint8), axis=1).astype(np.float32)


def descend(voc, d, pick="first", bound=None):
    """the leaf node of every descriptor, all descriptors at once (Hamming distances as an exact +-1 product: (256 - a.b) / 2).
    pick: "first" (DBoW3) or "last" child of minimal distance.  bound: None walks until a leaf; an integer restates voc_descend's
    `for (level = 0; level <= bound; level++)`, -1 where no leaf is met within it.  -> (node [n], ties [n, levels] number of children
    at the minimal distance on each level of the path, 0 beyond its end)"""
    child_ptr, child_idx, desc = voc[0], voc[1], voc[2]
    n = len(d)
    node = np.zeros(n, np.int64)
    leaf = np.zeros(n, bool)
    A, B = _pm1(d) if n else np.zeros((0, 256), np.float32), _pm1(desc)
    ties, level = [], 0
    while True:
        is_leaf = child_ptr[node + 1] == child_ptr[node]
        leaf |= is_leaf
        if leaf.all() or (bound is not None and level == bound):         # (the kernel's last pass only finds out whether it is at a leaf)
            break
        t = np.zeros(n, np.int64)
        for nd in np.unique(node[~leaf]):
            rows = np.nonzero((node == nd) & ~leaf)[0]
            ch = child_idx[child_ptr[nd]:child_ptr[nd + 1]]
            dist = ((256.0 - A[rows] @ B[ch].T) / 2.0).astype(np.int64)
            m = dist.min(1, keepdims=True)
            t[rows] = (dist == m).sum(1)
            k = dist.argmin(1) if pick == "first" else dist.shape[1] - 1 - dist[:, ::-1].argmin(1)
            node[rows] = ch[k]
        ties.append(t)
        level += 1
    out = np.where(leaf, node, -1)
    return out, (np.stack(ties, 1) if ties else np.zeros((n, 0), np.int64))


def alt_transform(voc, d, pick="first", stop=True, value="add", norm="seq", bound=None):
    """Vocabulary::transform with each rule a parameter; the defaults are DBoW3's.  stop: drop words of weight <= 0.  value: "add" the
    weight once per occurrence, or "mul" count * weight.  norm: the L1 norm summed "seq" (ascending word id), "desc" (descending) or
    "pairwise" (np.sum).  -> (ids, vals)"""
    weight, word_id = voc[3], voc[4]
    node, _ = descend(voc, d, pick, bound)
    bow, cnt, wt = {}, {}, {}
    for nd in node.tolist():
        if nd < 0 or (stop and not weight[nd] > 0):
            continue
        w = int(word_id[nd])
        bow[w] = bow.get(w, 0.0) + float(weight[nd])
        cnt[w] = cnt.get(w, 0) + 1
        wt[w] = float(weight[nd])
    ids = sorted(bow)
    vals = [bow[i] if value == "add" else cnt[i] * wt[i] for i in ids]
    if norm == "pairwise":
        s = float(np.sum(np.abs(np.array(vals)))) if vals else 0.0
    else:
        s = 0.0
        for v in (vals if norm == "seq" else vals[::-1]):
            s += abs(v)
    if s > 0:
        vals = [v / s for v in vals]
    return np.array(ids, np.int32), np.array(vals, np.float64)


def alt_score(a, b, order="seq"):
    """L1Scoring::score with the order of the sum a parameter: "seq" (ascending common word, DBoW3), "reverse", "pairwise" (np.sum)"""
    bd = dict(zip(b[0].tolist(), b[1].tolist()))
    terms = [abs(v - bd[i]) - abs(v) - abs(bd[i]) for i, v in zip(a[0].tolist(), a[1].tolist()) if i in bd]
    if order == "pairwise":
        return -float(np.sum(np.array(terms, np.float64))) / 2.0
    s = 0.0
    for t in (terms if order == "seq" else terms[::-1]):
        s += t
    return -s / 2.0


def same(a, b):
    """two (ids, vals) vectors equal bit for bit"""
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


# ---- transform recipes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def stop_flat():
    """a flat vocabulary with exact zero weights on every 7th word (and one negative weight: the filter is `> 0`, not `!= 0`)"""
    n = 50
    rng = np.random.default_rng(11)
    w = rng.uniform(0.1, 3.0, n)
    w[::7] = 0.0
    w[1] = -0.5
    voc, leaf = V.flat_vocabulary(w, seed=12)
    stopped = np.nonzero(~(w > 0))[0]
    alive = np.nonzero(w > 0)[0]
    kfs = [("only_stopped", leaf[np.concatenate([stopped, stopped[::-1], [0, 7, 1]])]),
           ("mixed", leaf[rng.integers(0, n, 200)]),
           ("one_survivor", leaf[np.array([0, 7, 3, 14, 3, 1, 3, 21])]),
           ("no_stopped", leaf[rng.choice(alive, 120)])]
    part = Part("stop_flat", voc, kfs, dcap=256)
    assert (voc[3][voc[4] >= 0] == 0).sum() == 8 and len(stopped) == 9
    rv = RefVoc(voc)
    words = [ref_words(rv, k) for k in part.keyframes()]
    assert all(not (wt > 0).any() for _, wt in words[:1]) and (words[2][1] > 0).sum() == 3 and len(set(words[2][0][words[2][1] > 0])) == 1
    n_stop = int((~(words[1][1] > 0)).sum())
    assert 20 <= n_stop <= 60 and (words[3][1] > 0).all()
    return Recipe("stop_flat", [part], zero_words=8, nonpositive_words=9, mixed_stopped=n_stop)


@functools.lru_cache(None)
def stop_tree():
    """a trained tree that has stop words: eight training images, words seen in all of them get idf log(8/8) = 0"""
    kfs = V.make_keyframes(2, n_img=8)
    voc = V.build_vocabulary(kfs)
    part = Part("stop_tree", voc, [("kf%d" % i, k) for i, k in enumerate(kfs)], dcap=512)
    zero = int((voc[3][voc[4] >= 0] == 0).sum())
    wts = ref_words(RefVoc(voc), np.concatenate(part.keyframes()))[1]
    frac = float((~(wts > 0)).mean())
    assert zero >= 3 and frac >= 0.10, (zero, frac)
    return Recipe("stop_tree", [part], zero_words=zero, stopped=int((~(wts > 0)).sum()), descriptors=len(wts))


TIE_PAT = (0x000F, 0x00F0, 0x0F00, 0xF000)      # a level's 16-bit field of children 0..3: pairwise distance 8
TIE_FIELD = {"c0": 0x000F, "c1": 0x00F0, "c2": 0x0F00, "c3": 0xF000,     # distance 0 to one child, 8 to the others: no tie
             "t01": 0x00FF, "t23": 0xFF00,                                  # distance 4 to two children, 12 to the others
             "t4": 0x0000}                                                  # distance 4 to all four
TIE_IDENT = (3, 1, 2)       # below node "root child 3": children 1 and 2 carry the same descriptor


def _put16(d, field, v):
    d[..., 2 * field] = v & 0xFF
    d[..., 2 * field + 1] = v >> 8


@functools.lru_cache(None)
def ties_voc():
    """depth 3, 4 children per node; the children of a node at level l differ only in the 16-bit field l - 1 (TIE_PAT)"""
    rng = np.random.default_rng(21)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    _put16(base, 0, 0), _put16(base, 1, 0), _put16(base, 2, 0)
    nodes = [dict(desc=base.copy(), children=[], path=())]

    def grow(nid, level):
        if level == 3:
            return
        for c in range(4):
            d = nodes[nid]["desc"].copy()
            pat = TIE_PAT[c]
            if nodes[nid]["path"] == TIE_IDENT[:1] and c == TIE_IDENT[2]:
                pat = TIE_PAT[TIE_IDENT[1]]                                 # the bit-identical sibling
            _put16(d, level, pat)
            nodes.append(dict(desc=d, children=[], path=nodes[nid]["path"] + (c,)))
            nodes[nid]["children"].append(len(nodes) - 1)
            grow(len(nodes) - 1, level + 1)

    grow(0, 0)
    n = len(nodes)
    assert n == 85
    child_ptr = np.zeros(n + 1, np.int32)
    child_idx = []
    for i, nd in enumerate(nodes):
        child_idx += nd["children"]
        child_ptr[i + 1] = len(child_idx)
    word_id = np.full(n, -1, np.int32)
    weight = np.zeros(n)
    k = 0
    for i, nd in enumerate(nodes):
        if not nd["children"]:
            word_id[i], weight[i] = k, rng.uniform(0.2, 4.0)
            k += 1
    assert k == 64
    desc = np.stack([nd["desc"] for nd in nodes])
    a, b = [i for i, nd in enumerate(nodes) if nd["path"] in ((3, 1), (3, 2))]
    # exactly one pair of identical siblings (their four children each are then cousins with equal descriptors, never compared)
    assert np.array_equal(desc[a], desc[b]) and len(np.unique(desc[1:], axis=0)) == n - 1 - 5
    for nd in nodes:
        ch = desc[nd["children"]]
        assert len(np.unique(ch, axis=0)) == len(ch) - (nd["path"] == TIE_IDENT[:1]) or not len(ch)
    return (child_ptr, np.array(child_idx, np.int32), desc, weight, word_id), base


def tie_descriptor(base, fields, rng):
    """a descriptor whose level fields are TIE_FIELD[fields[l]]; the other 13 fields differ from every node's by random bits, which
    adds the same distance to all siblings"""
    d = base.copy()
    noise = rng.integers(0, 256, 32, dtype=np.uint8) & rng.integers(0, 256, 32, dtype=np.uint8) & rng.integers(0, 256, 32, dtype=np.uint8)
    d ^= noise
    for l, f in enumerate(fields):
        _put16(d, l, TIE_FIELD[f])
    return d


@functools.lru_cache(None)
def ties():
    voc, base = ties_voc()
    rng = np.random.default_rng(22)
    kinds = list(TIE_FIELD)
    tie_kinds = ("t01", "t23", "t4")
    kfs, used = [], []
    for i in range(8):                                                      # random mixes; every descriptor ties on some level
        fs = [tuple(kinds[int(rng.integers(0, len(kinds)))] for _ in range(3)) for _ in range(120)]
        cand = np.stack([tie_descriptor(base, f, rng) for f in fs])
        keep = np.nonzero(descend(voc, cand)[1].max(1) >= 2)[0][:60]          # (e.g. below the identical pair t23 singles out child 3)
        assert len(keep) == 60
        used += [fs[j] for j in keep]
        kfs.append(("mix%d" % i, cand[keep]))
    kfs.append(("every_level", np.stack([tie_descriptor(base, f, rng) for f in
                                         [(a, b, c) for a in tie_kinds for b in tie_kinds for c in tie_kinds]])))
    # below root child 3 the children 1 and 2 are the same descriptor: c1 (= c2 there) ties at distance 0, t01 / t23 tie three ways
    kfs.append(("identical", np.stack([tie_descriptor(base, f, rng) for f in
                                       [("c3", "c1", "c0"), ("c3", "c1", "t4"), ("c3", "c2", "c2"), ("c3", "t01", "c2"), ("c3", "t01", "t01"),
                                        ("c3", "c1", "c1"), ("c3", "c1", "t23"), ("c3", "t4", "c0")]])))
    part = Part("ties", voc, kfs, dcap=64)
    t = [descend(voc, k)[1] for k in part.keyframes()]
    assert all(x.shape[1] == 3 and (x.max(1) >= 2).all() for x in t)         # every descriptor ties on at least one level
    allt = np.concatenate(t)
    fig = dict(descriptors=len(allt), two_way=int((allt == 2).sum()), three_way=int((allt == 3).sum()), four_way=int((allt == 4).sum()),
               every_level=int((allt >= 2).all(1).sum()))
    assert fig["every_level"] >= 27 and fig["four_way"] >= 50 and fig["three_way"] >= 2
    for lvl in range(3):                                                    # both two-way kinds and the four-way kind on every level
        assert {"t01", "t23", "t4"} <= {f[lvl] for f in used}
    return Recipe("ties", [part], **fig)


UNEVEN_DEEP = 13            # levels below the root of the deepest leaf


@functools.lru_cache(None)
def uneven():
    """a hand-built tree: a leaf under the root, nodes with 1, 2 and 20 children, a one-child chain, a branch UNEVEN_DEEP levels deep
    that ends in a leaf, word ids permuted against node order and with gaps.  The children of a node at level l differ in the 16-bit field
    l - 1 (child c carries c + 1), so a descriptor assembled from a leaf's path descends to that leaf."""
    # spec: a node is a list of children, a leaf is None
    deep = [None]                                                           # the deepest node: a leaf, alone on its level
    for _ in range(UNEVEN_DEEP - 2):
        deep = [None, deep]                                                 # a leaf beside the branch that goes on
    spec = [None,                                                           # a leaf directly under the root
            [[[None]]],                                                     # a one-child chain: three nodes of one child, then a leaf
            [None, [None, None]],                                           # two children
            [None] * 20,                                                    # twenty children
            deep]
    nodes = [dict(desc=np.zeros(32, np.uint8), children=[], path=(), leaf=False)]

    def grow(nid, sp, level):
        for c, s in enumerate(sp):
            d = nodes[nid]["desc"].copy()
            _put16(d, level, c + 1)
            nodes.append(dict(desc=d, children=[], path=nodes[nid]["path"] + (c,), leaf=s is None))
            nodes[nid]["children"].append(len(nodes) - 1)
            if s is not None:
                grow(len(nodes) - 1, s, level + 1)

    grow(0, spec, 0)
    n = len(nodes)
    child_ptr = np.zeros(n + 1, np.int32)
    child_idx = []
    for i, nd in enumerate(nodes):
        child_idx += nd["children"]
        child_ptr[i + 1] = len(child_idx)
    leaves = [i for i, nd in enumerate(nodes) if nd["leaf"]]
    rng = np.random.default_rng(31)
    ids = rng.permutation(np.arange(len(leaves)) * 3 + 2)                   # out of node order, gaps of 2 between ids, 0 and 1 unused
    word_id = np.full(n, -1, np.int32)
    weight = np.zeros(n)
    word_id[leaves] = ids
    weight[leaves] = rng.uniform(0.2, 4.0, len(leaves))
    voc = (child_ptr, np.array(child_idx, np.int32), np.stack([nd["desc"] for nd in nodes]), weight, word_id)
    nch = np.diff(child_ptr)
    depth = np.array([len(nd["path"]) for nd in nodes])
    assert nch[0] == 5 and {1, 2, 20} <= set(nch.tolist()) and depth.max() == UNEVEN_DEEP >= 12
    assert [nodes[i]["leaf"] for i in np.nonzero(depth == UNEVEN_DEEP)[0]] == [True]         # the deepest node is a leaf, the only one there
    assert nodes[leaves[0]]["path"] == (0,)                                 # a leaf directly under the root
    assert int(ids.max()) + 1 > len(leaves) and not np.all(np.diff(word_id[leaves]) > 0)
    deepest = int(np.nonzero(depth == UNEVEN_DEEP)[0][0])

    def to_leaf(i, r):
        d = np.zeros(32, np.uint8)
        for l, c in enumerate(nodes[i]["path"]):
            _put16(d, l, c + 1)
        d[2 * UNEVEN_DEEP:] = r.integers(0, 256, 32 - 2 * UNEVEN_DEEP, dtype=np.uint8)     # fields no node uses
        # fields below the leaf's level: anything (every node on the path carries 0 there, all siblings alike)
        for l in range(len(nodes[i]["path"]), UNEVEN_DEEP):
            _put16(d, l, int(r.integers(0, 1 << 16)))
        return d

    order = rng.permutation(len(leaves))
    kfs = [("every_leaf", np.stack([to_leaf(leaves[j], rng) for j in order])),
           ("repeats", np.stack([to_leaf(leaves[j], rng) for j in rng.integers(0, len(leaves), 150)])),
           ("deepest_only", np.stack([to_leaf(deepest, rng) for _ in range(5)])),
           ("deep_branch", np.stack([to_leaf(i, rng) for i in leaves if nodes[i]["path"][0] == 4] * 2))]
    part = Part("uneven", voc, kfs, dcap=256)
    got = descend(voc, part.keyframe(0))[0]
    assert np.array_equal(got, np.array(leaves)[order])                     # a descriptor ends in every leaf
    assert part.n_words == 3 * len(leaves) and part.vcap == min(256, part.n_words)
    return Recipe("uneven", [part], nodes=n, leaves=len(leaves), n_words=part.n_words, depth=int(depth.max()), deepest_node=deepest)


def _run_positions(words):
    """sorted position of the first and the last occurrence of every distinct word"""
    s = np.sort(words)
    first = np.nonzero(np.concatenate([[True], s[1:] != s[:-1]]))[0]
    last = np.concatenate([first[1:], [len(s)]]) - 1
    return first, last


@functools.lru_cache(None)
def full():
    """k_bow_vector at its own limits: dcap == count == BOW_MAXF, nnz == vcap, long runs across the thread and wave boundaries"""
    n = 2100
    rng = np.random.default_rng(41)
    w = rng.uniform(0.5, 8.0, n)
    voc, leaf = V.flat_vocabulary(w, seed=42)
    a = rng.permutation(np.concatenate([[n - 1, 0], 1 + rng.permutation(n - 2)[:BOW_MAXF - 2]]))    # the first and the last word among them
    assert len(set(a.tolist())) == BOW_MAXF
    b = np.full(BOW_MAXF, 1234)
    c = rng.integers(0, n, BOW_MAXF - 1)
    # (d) runs of 1, 2, 3, ... 63 occurrences (2016 descriptors), the lengths dealt to ascending word ids in a shuffled order: the first
    # seed whose runs start at odd and at even sorted positions and straddle positions 127/128 and 1023/1024
    d = None
    for seed in range(64):
        r = np.random.default_rng(1000 + seed)
        wd = np.sort(r.choice(n, 63, replace=False))
        lens = r.permutation(np.arange(1, 64))
        cand = r.permutation(np.repeat(wd, lens))
        first, last = _run_positions(cand)
        strad = lambda p: bool(np.any((first <= p) & (last >= p + 1)))
        if strad(127) and strad(1023) and (first % 2 == 1).sum() >= 10 and (first % 2 == 0).sum() >= 10:
            d = cand
            break
    assert d is not None and len(d) == 2016
    main = Part("full", voc, [("a_distinct", leaf[a]), ("b_one_word", leaf[b]), ("c_2047", leaf[c]), ("d_runs", leaf[d])], dcap=BOW_MAXF)
    assert main.vcap == BOW_MAXF == main.dcap and list(main.count) == [2048, 2048, 2047, 2016]
    # the second vocabulary: fewer words than dcap, every one of them hit
    w2 = rng.uniform(0.5, 8.0, 300)
    voc2, leaf2 = V.flat_vocabulary(w2, seed=43)
    hit = np.concatenate([rng.permutation(300), rng.integers(0, 300, 212)])
    small = Part("full_vcap300", voc2, [("all_300", leaf2[hit])], dcap=512)
    assert small.vcap == 300 == small.n_words < small.dcap and len(set(hit.tolist())) == 300
    return Recipe("full", [main, small], run_lengths=63)


CAPS_DCAP = (1, 2, 255, 257, 1023, 1025, 2047)


@functools.lru_cache(None)
def caps():
    """dcap odd, one off the 256 of k_bow_words' workgroup, one off the 1024 threads of k_bow_vector; raw counts beyond both ends"""
    rng = np.random.default_rng(51)
    w = rng.uniform(0.5, 8.0, 40)
    voc, leaf = V.flat_vocabulary(w, seed=52)
    parts = []
    for dcap in CAPS_DCAP:
        rows = [("over", leaf[rng.integers(0, 40, dcap)]), ("full", leaf[rng.integers(0, 40, dcap)]), ("zero", leaf[rng.integers(0, 40, dcap)]),
                ("negative", leaf[rng.integers(0, 40, dcap)]), ("last", leaf[rng.integers(0, 40, dcap)])]
        p = Part("caps_%d" % dcap, voc, rows, dcap=dcap, counts=[dcap + 5, dcap, 0, -3, dcap])
        assert [len(k) for k in p.keyframes()] == [dcap, dcap, 0, 0, dcap] and p.vcap == min(dcap, 40)
        parts.append(p)
    return Recipe("caps", parts)


TRANSFORM_RECIPES = (stop_flat, stop_tree, ties, uneven, full, caps)


# ---- score recipes ---------------------------------------------------------------------------------------------------------------
CHUNK_NQ = (0, 1, 63, 64, 65, 128, 129, 200)
CHUNK_NDB = (1, 3, 4, 5, 9)
CHUNK_KINDS = ("first_chunk", "last_chunk", "chunks_0_2", "pos_63_64", "disjoint", "empty", "one_hit", "one_miss", "lane_63", "lane_0",
               "q_above", "q_below", "identical", "absent", "all_other_vals")


def _vals(rng, n):
    """values that need not be normalised: both signs, and -0.0 / 0.0 among them"""
    v = rng.uniform(-1.0, 1.0, n)
    if n >= 3:
        v[rng.integers(0, n)] = -0.0
        v[rng.integers(0, n)] = 0.0
    return v


@functools.lru_cache(None)
def chunks():
    """query lengths around the 64 lanes of a wave; database vectors whose common words with the query lie in chosen chunks / lanes.
    Query word i is 100 + 2 i; words that are not the query's are odd, or below 100, or above every query word."""
    rng = np.random.default_rng(61)
    vectors, queries, db, expect_hits = [], {}, {}, {}

    def vec(ids):
        ids = np.array(sorted(set(int(i) for i in ids)), np.int32)
        return ids, _vals(rng, len(ids))

    for nq in CHUNK_NQ:
        qi = (100 + 2 * np.arange(nq)).astype(np.int32)
        q = (qi, _vals(rng, nq))
        name = "q%d" % nq
        queries[name] = len(vectors)
        vectors.append(q)
        first = len(vectors)
        odd = lambda lo, hi, k: (101 + 2 * rng.choice(np.arange(lo, hi), min(k, hi - lo), replace=False)).tolist()
        at = lambda pos: [int(qi[p]) for p in pos if p < nq]
        last0 = 64 * ((nq - 1) // 64) if nq else 0
        kinds = dict(
            first_chunk=at(range(0, 64, 3)) + odd(0, 260, 40),
            last_chunk=at(range(last0, nq, 2)) + odd(0, 260, 40),
            chunks_0_2=at(list(range(1, 64, 5)) + list(range(128, 192, 7))) + odd(64, 128, 30),
            pos_63_64=at([63, 64]) + odd(0, 260, 50),
            disjoint=odd(0, 260, 200),
            empty=[],
            one_hit=at([nq // 2]),
            one_miss=[101 + 2 * (nq // 2)],
            lane_63=at([63, 127, 191]) + odd(0, 260, 20),
            lane_0=at([0, 64, 128, 192]) + odd(0, 260, 20),
            q_above=list(range(3, 60, 4)) + at([0]),                        # every database word but one lies below the query's
            q_below=list(range(1001, 1060, 4)) + at([nq - 1] if nq else []),  # ... above the query's
            identical=None, absent=None,
            all_other_vals=qi.tolist())
        hits = {}
        for k in CHUNK_KINDS:
            if k == "identical":
                v = (q[0].copy(), q[1].copy())
            elif k == "absent":
                v = None
            else:
                v = vec(kinds[k])
            vectors.append(v)
            hits[k] = 0 if v is None else len(np.intersect1d(v[0], qi))
        db[name] = (first, len(CHUNK_KINDS))
        expect_hits[name] = hits
        assert hits["disjoint"] == hits["empty"] == hits["one_miss"] == hits["absent"] == 0
        assert hits["identical"] == hits["all_other_vals"] == nq and hits["one_hit"] == min(nq, 1)
        assert hits["pos_63_64"] == (nq > 63) + (nq > 64) and hits["lane_63"] == nq // 64 and hits["lane_0"] == (nq + 63) // 64
    st = Store("chunks", vectors, queries, db, vcap=256)
    # in q200 against chunks_0_2 no word of query positions 64..127 is common, words of positions 0..63 and 128..191 are
    f, _ = db["q200"]
    common = np.intersect1d(st.vec(f + CHUNK_KINDS.index("chunks_0_2"))[0], st.vec(queries["q200"])[0])
    pos = (common - 100) // 2
    assert (pos < 64).any() and (pos >= 128).any() and not ((pos >= 64) & (pos < 128)).any()
    st.hits = expect_hits
    return st


@functools.lru_cache(None)
def order():
    """two vectors of 200 common words whose magnitudes spread over 2^-60 .. 2^-1, shuffled: the sum of the terms depends on its order"""
    rng = np.random.default_rng(71)
    ids = np.sort(rng.choice(5000, 200, replace=False)).astype(np.int32)

    def mags():
        e = rng.permutation(np.linspace(-60, -1, 200))
        return rng.uniform(1.0, 2.0, 200) * np.exp2(np.floor(e)) * np.where(rng.random(200) < 0.3, -1.0, 1.0)

    a, b, c = (ids, mags()), (ids.copy(), mags()), (ids.copy(), mags())
    st = Store("order", [a, b, c], dict(a=0), dict(a=(0, 3)), vcap=200)
    lo, hi = np.abs(a[1]).min(), np.abs(a[1]).max()
    assert lo < 2.0 ** -58 and hi >= 2.0 ** -2
    return st


SCORE_RECIPES = (chunks, order)
