"""Test helper: links and loops from stored keyframes (flvis_loop_closer_link) assembled from the CPU oracle's functions --
tests/_loop_localize_in.py's chain with a stored keyframe as the query and an excluded set:

    query        keyframe kf of sequence stream: the feature dict its sequence's RefLoopCloser holds
    candidates   ref_localize_in's line over the searched sequences WITHOUT the excluded keyframes of the query's own sequence:
                 own_gap = -1 all of them, g >= 0 those with |j - kf| <= g
    pair check   ref_localize_in's own, run on refs in which the excluded keyframes carry an empty bag of words (score 0: never a
                 candidate, indices unchanged) -- the candidates it then finds are asserted to be the line's"""
import numpy as np

import _loop_localize_in as LI
from test_oracle_bow import ref_score

_NO_WORDS = (np.zeros(0, np.int32), np.zeros(0))


def excluded(stream, kf, own_gap, count):
    """the keyframes of sequence `stream` (holding `count`) that a query (stream, kf, own_gap) leaves out"""
    return set(range(count)) if own_gap < 0 else {j for j in range(count) if abs(j - kf) <= own_gap}


class _Without:
    """a RefLoopCloser as ref_localize_in reads it (kfs, T_c_w, prm), the excluded keyframes without words"""

    def __init__(self, ref, out):
        self.prm, self.T_c_w = ref.prm, ref.T_c_w
        self.kfs = [dict(kf, bow=_NO_WORDS) if j in out else kf for j, kf in enumerate(ref.kfs)]


def ref_link(refs, maps, stream, kf, own_gap, K4, n_best):
    """refs: {sequence: LC.RefLoopCloser}, maps: the searched sequence or LI.ALL_MAPS, K4: the QUERY sequence's camera
    -> (dict like LoopCloser.link's fix, the excluded set)"""
    feat = refs[stream].kfs[kf]
    out = excluded(stream, kf, own_gap, len(refs[stream].kfs))
    p = refs[min(refs)].prm
    searched = sorted(refs) if maps < 0 else [maps]
    scored = [(ref_score(feat["bow"], k["bow"]), s, j) for s in searched for j, k in enumerate(refs[s].kfs) if not (s == stream and j in out)]
    order = sorted((e for e in scored if e[0] > 0 and e[0] >= p["minScore"]), key=lambda e: (-e[0], e[1], e[2]))[:n_best]
    assert not ref_score(feat["bow"], _NO_WORDS) > 0
    view = dict(refs)
    view[stream] = _Without(refs[stream], out)
    fix = LI.ref_localize_in(view, maps, feat, stream, K4, n_best)
    assert [(c["score"], c["seq"], c["kf"]) for c in fix["candidates"]] == order
    return fix, out
