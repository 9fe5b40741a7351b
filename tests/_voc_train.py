"""Test helper: an independent restatement of the vocabulary training (flvis_hip_voc_train; DESIGN.md section 8 f4 "training"),
written in numpy from DBoW3's Vocabulary::create (3rdPartLib/DBow3/src/Vocabulary.cpp:142-569: HKmeansStep :231-392,
initiateClustersKMpp :407-489, createWords :494-513, setNodeWeights :518-569) and DescManip::meanValue (DescManip.cpp:25-74).

The random numbers are the real libc's (`srand` / `rand` through ctypes), so nothing here is shared with the product's own
restatement of glibc's generator.  Two departures from DBoW3, the same two the product states:
  (a) every split node draws from its own stream srand(seed + node_id) (unsigned wrap), and nodes are numbered breadth-first, the
      children of a level consecutively in (parent id, cluster index) order;
  (b) a node's k-means ends after `max_iters` association passes (DBoW3 has no cap).
`create_one_level` below is a straight transcription with ONE libc stream; at L = 1 the two agree (tests/test_voc_train_inputs.py)."""
import ctypes as C
import ctypes.util
import math

import numpy as np

_libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libc.srand.argtypes = [C.c_uint]
_libc.srand.restype = None
_libc.rand.restype = C.c_int
RAND_MAX = 2147483647

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def distances(d, centres):
    """d [n,32], centres [c,32] uint8 -> [n,c] Hamming distances"""
    out = np.empty((len(d), len(centres)), np.int64)
    for c in range(len(centres)):
        out[:, c] = _POP[np.bitwise_xor(d, centres[c][None, :])].sum(1)
    return out


def new_counts():
    return dict(assign_ties=0, majority_ties=0, empty_kept=0, trivial=0, seed_early_stop=0, capped=0)


def mean_value(members, old, counts):
    """DescManip::meanValue: bit set when sum >= n/2 + n%2; nothing happens for an empty set; a single member is copied"""
    n = len(members)
    if n == 0:
        counts["empty_kept"] += 1
        return old
    if n == 1:
        return members[0].copy()
    s = np.unpackbits(members, axis=1).astype(np.int64).sum(0)
    if n % 2 == 0:
        counts["majority_ties"] += int(np.count_nonzero(s == n // 2))
    return np.packbits((s >= n // 2 + n % 2).astype(np.uint8))


def seed_kmpp(d, k, counts, rand=_libc.rand):
    """initiateClustersKMpp -> indices of the chosen descriptors"""
    n = len(d)
    picks = [rand() % n]
    min_d = distances(d, d[picks[-1]][None])[:, 0]
    while len(picks) < k:
        dist = distances(d, d[picks[-1]][None])[:, 0]
        upd = min_d > 0
        min_d = np.where(upd, np.minimum(min_d, dist), min_d)
        dist_sum = int(min_d.sum())                       # integers: exact, whatever the order
        if dist_sum == 0:
            counts["seed_early_stop"] += 1
            break
        while True:
            cut = (float(rand()) / float(RAND_MAX)) * float(dist_sum)
            if cut != 0.0:
                break
        up = np.cumsum(min_d).astype(np.float64)          # (exact: the sums stay far below 2^53)
        hit = np.nonzero(up >= cut)[0]
        picks.append(int(hit[0]) if len(hit) else n - 1)
    return picks


def kmeans_node(d, k, max_iters, counts, rand=_libc.rand):
    """the `else` arm of HKmeansStep for one node of more than k descriptors -> (centres [c,32], labels [n], passes, capped)"""
    centres = d[seed_kmpp(d, k, counts, rand)].copy()
    last = None
    passes = 0
    while True:
        if last is not None:
            for c in range(len(centres)):
                centres[c] = mean_value(d[last == c], centres[c], counts)
        dist = distances(d, centres)
        cur = dist.argmin(1)                              # first minimum: strict `<` in centre order
        counts["assign_ties"] += int(np.count_nonzero((dist == dist.min(1)[:, None]).sum(1) > 1))
        passes += 1
        if last is not None and np.array_equal(cur, last):
            return centres, cur, passes, False
        if passes >= max_iters:
            counts["capped"] += 1
            return centres, cur, passes, True
        last = cur


def descend(voc, f):
    """Vocabulary::transform(feature, word_id): the first child at minimum distance, down to a leaf -> node id"""
    child_ptr, child_idx, desc = voc[0], voc[1], voc[2]
    node = 0
    while child_ptr[node + 1] > child_ptr[node]:
        ch = child_idx[child_ptr[node]:child_ptr[node + 1]]
        node = int(ch[int(np.argmin(_POP[np.bitwise_xor(desc[ch], f[None, :])].sum(1)))])
    return node


def train(images, k, L, seed=1, weighting=0, max_iters=100):
    """images: list of [n_i,32] uint8 (an image may be empty).  Returns a dict: arrays (child_ptr, child_idx, desc, weight,
    word_id with -1 on inner nodes), ni (per word), stats (the first seven entries of the product's stats8), counts (how often
    each branch ran)."""
    max_iters = max_iters or 100
    feats = np.concatenate([np.asarray(i, np.uint8).reshape(-1, 32) for i in images])      # getFeatures: image-major
    counts = new_counts()
    desc = [np.zeros(32, np.uint8)]
    children = [[]]
    level_nodes = [(0, np.arange(len(feats)))]            # nodes of the current level that are split, ascending id
    passes_total = capped = empty_children = 0
    for level in range(L):
        nxt = []
        for nid, mem in level_nodes:
            d = feats[mem]
            if len(d) <= k:
                counts["trivial"] += 1
                centres, lab = d.copy(), np.arange(len(d))
            else:
                _libc.srand(C.c_uint((seed + nid) & 0xFFFFFFFF))
                centres, lab, p, cap = kmeans_node(d, k, max_iters, counts)
                passes_total += p
                capped += int(cap)
            for c in range(len(centres)):
                cid = len(desc)
                desc.append(centres[c].copy())
                children.append([])
                children[nid].append(cid)
                sub = mem[lab == c]                       # the parent's order
                empty_children += int(len(sub) == 0)
                if level + 1 < L and len(sub) > 1:
                    nxt.append((cid, sub))
        level_nodes = nxt
    n = len(desc)
    child_ptr = np.zeros(n + 1, np.int32)
    child_idx = []
    for i in range(n):
        child_idx += children[i]
        child_ptr[i + 1] = len(child_idx)
    child_idx = np.array(child_idx, np.int32)
    desc = np.stack(desc)
    word_id = np.full(n, -1, np.int32)
    leaves = [i for i in range(1, n) if not children[i]]  # createWords: ascending node id
    word_id[leaves] = np.arange(len(leaves), dtype=np.int32)
    weight = np.zeros(n)
    voc = (child_ptr, child_idx, desc, weight, word_id)
    ni = np.zeros(len(leaves), np.int64)
    cache = {}
    for img in images:                                    # setNodeWeights: every feature goes down the FINISHED tree
        seen = set()
        for f in np.asarray(img, np.uint8).reshape(-1, 32):
            key = f.tobytes()
            if key not in cache:
                cache[key] = int(word_id[descend(voc, f)])
            seen.add(cache[key])
        for w in seen:
            ni[w] += 1
    for w, node in enumerate(leaves):
        if weighting == 1:
            weight[node] = 1.0
        elif ni[w] > 0:
            weight[node] = math.log(float(len(images)) / float(ni[w]))
    stats = [len(feats), n, len(leaves), passes_total, capped, empty_children, counts["trivial"]]
    return dict(arrays=voc, ni=ni, stats=stats, counts=counts, ndocs=len(images))


def create_one_level(feats, k, seed):
    """A straight transcription of HKmeansStep + initiateClustersKMpp for the root alone, as Vocabulary::create runs it in a process
    that called srand(seed): ONE libc stream, plain Python loops, doubles where DBoW3 has doubles.  -> centres [c,32]"""
    feats = [np.asarray(f, np.uint8) for f in feats]
    n = len(feats)

    def dist(a, b):
        return float(int(_POP[np.bitwise_xor(a, b)].sum()))

    _libc.srand(C.c_uint(seed & 0xFFFFFFFF))
    if n <= k:
        return np.stack(feats)
    clusters = [feats[_libc.rand() % n]]
    min_dists = [dist(f, clusters[-1]) for f in feats]
    while len(clusters) < k:
        for i, f in enumerate(feats):
            if min_dists[i] > 0:
                dd = dist(f, clusters[-1])
                if dd < min_dists[i]:
                    min_dists[i] = dd
        dist_sum = 0.0
        for m in min_dists:
            dist_sum += m
        if not dist_sum > 0:
            break
        while True:
            cut_d = (float(_libc.rand()) / float(RAND_MAX)) * dist_sum
            if cut_d != 0.0:
                break
        d_up_now, pick = 0.0, n - 1
        for i, m in enumerate(min_dists):
            d_up_now += m
            if d_up_now >= cut_d:
                pick = i
                break
        clusters.append(feats[pick])
    clusters = [c.copy() for c in clusters]
    first_time, last = True, None
    while True:
        if not first_time:
            for c in range(len(clusters)):
                grp = [feats[i] for i in range(n) if last[i] == c]
                if not grp:
                    continue
                if len(grp) == 1:
                    clusters[c] = grp[0].copy()
                    continue
                s = [0] * 256
                for g in grp:
                    for j in range(32):
                        for b in range(8):
                            if g[j] & (1 << (7 - b)):
                                s[j * 8 + b] += 1
                n2 = len(grp) // 2 + len(grp) % 2
                m = np.zeros(32, np.uint8)
                for i in range(256):
                    if s[i] >= n2:
                        m[i // 8] |= 1 << (7 - (i % 8))
                clusters[c] = m
        cur = []
        for f in feats:
            best, ic = dist(f, clusters[0]), 0
            for c in range(1, len(clusters)):
                dd = dist(f, clusters[c])
                if dd < best:
                    best, ic = dd, c
            cur.append(ic)
        if first_time:
            first_time = False
        elif cur == last:
            break
        last = cur
    return np.stack(clusters)


def duplicate_node(k, seed=3):
    """the hand-built input of the early stop of the seeding: 3k copies of two distinct descriptors, interleaved, as one image"""
    rng = np.random.default_rng(seed)
    two = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    which = rng.integers(0, 2, 3 * k)
    which[:2] = (0, 1)
    return [two[which]]
