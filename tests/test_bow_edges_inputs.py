"""CPU: the recipes of tests/_bow_edges.py checked without a GPU.  The oracle (oracle/ref_bow.cpp), the plain-Python restatements of
tests/_voc.py and the parametrised restatement of _bow_edges agree bit for bit on every recipe; the figures the recipes rest on are
pinned; and each recipe is shown to discriminate the mistake it is there for: the alternative rule, restated in Python, gives another
result than the oracle's on it.  (tests/test_gpu_bow_edges.py then holds the kernels to the oracle's result on the same inputs.)"""
import numpy as np
import pytest

import _bow_edges as E
import _voc as V
from test_oracle_bow import ref_score


@pytest.fixture(scope="module")
def want():
    """the oracle's vectors: {part name: [(ids, vals)]}"""
    return {p.name: E.ref_transform(p) for f in E.TRANSFORM_RECIPES for p in f().parts}


def _parts():
    return [p for f in E.TRANSFORM_RECIPES for p in f().parts]


def test_oracle_and_both_restatements_agree_on_every_transform_recipe(want):
    rows = 0
    for p in _parts():
        for i, k in enumerate(p.keyframes()):
            w = want[p.name][i]
            assert E.same(w, E.alt_transform(p.voc, k)), (p.name, p.names[i])
            assert E.same(w, V.py_transform(p.voc, k)), (p.name, p.names[i])
            assert np.all(np.diff(w[0]) > 0) and len(w[0]) <= p.vcap
            rows += 1
    assert rows >= 60


def test_oracle_and_both_restatements_agree_on_every_score_recipe():
    pairs = 0
    for f in E.SCORE_RECIPES:
        st = f()
        for qn, q in st.queries.items():
            first, n = st.db[qn]
            got = E.ref_scores(st, q, first, n)
            for j in range(n):
                a, b = st.vec(q), st.vec(first + j)
                if st.vectors[first + j] is None:
                    assert got[j] == 0.0
                    continue
                assert got[j] == V.py_score(*a, *b) == E.alt_score(a, b) == ref_score(a, b), (st.name, qn, j)
                pairs += 1
    assert pairs >= 8 * 14 + 3


def test_figures_the_recipes_rest_on(want):
    assert E.stop_flat().figures == dict(zero_words=8, nonpositive_words=9, mixed_stopped=36)
    sf = want["stop_flat"]
    assert [len(v[0]) for v in sf] == [0, 41, 1, 39] and sf[2][1][0] == 1.0 and sf[2][0][0] == 3
    assert E.stop_tree().figures == dict(zero_words=6, stopped=949, descriptors=3391)            # 28 % of the descriptors stopped
    assert E.ties().figures == dict(descriptors=515, two_way=557, three_way=15, four_way=301, every_level=75)
    assert E.uneven().figures == dict(nodes=56, leaves=37, n_words=111, depth=13, deepest_node=55)
    un = want["uneven"]
    assert len(un[0][0]) == 37 and len(un[2][0]) == 1 and un[2][1][0] == 1.0 and len(un[3][0]) == 12
    fu = want["full"]
    assert [len(v[0]) for v in fu] == [2048, 1, 1331, 63] and fu[1][1][0] == 1.0 and fu[1][0][0] == 1234
    assert fu[0][0][0] == 0 and fu[0][0][-1] == 2099
    assert len(want["full_vcap300"][0][0]) == 300
    for dcap in E.CAPS_DCAP:
        nn = [len(v[0]) for v in want["caps_%d" % dcap]]
        assert nn[2] == nn[3] == 0 and all(1 <= x <= min(dcap, 40) for x in (nn[0], nn[1], nn[4])), (dcap, nn)
        assert dcap < 255 or nn[0] == nn[1] == nn[4] == 40                  # nnz == vcap == n_words from 255 descriptors on
    ch = E.chunks()
    assert len(ch.vectors) == 8 * 16 and sorted(ch.nnz[list(ch.queries.values())].tolist()) == list(E.CHUNK_NQ)
    assert ch.hits["q200"]["chunks_0_2"] == 13 + 10 and ch.hits["q129"]["last_chunk"] == 1 and ch.hits["q65"]["pos_63_64"] == 2
    assert (ch.nnz == -1).sum() == 8 and (ch.nnz == 0).sum() >= 8 and (ch.nnz == 1).sum() >= 8
    assert any(np.signbit(v[1]).any() and (v[1] == 0).any() for v in ch.vectors if v is not None)          # a -0.0 among the values


# ---- what each recipe rules out ------------------------------------------------------------------------------------------------------
def test_ties_rule_out_the_last_minimal_child(want):
    p = E.ties().parts[0]
    changed = [not E.same(want["ties"][i], E.alt_transform(p.voc, k, pick="last")) for i, k in enumerate(p.keyframes())]
    assert sum(changed) > len(changed) // 2, changed
    assert sum(changed) == len(changed) == 10                                # (all of them, in fact)
    # ... and the identical siblings alone do: the first of the pair is taken, the last rule ends below the second
    i = p.row("identical")
    first, last = E.descend(p.voc, p.keyframe(i))[0], E.descend(p.voc, p.keyframe(i), pick="last")[0]
    assert (first != last).all()


def test_stop_recipes_rule_out_a_missing_stop_word_filter(want):
    p = E.stop_flat().parts[0]
    for name in ("only_stopped", "mixed", "one_survivor"):
        i = p.row(name)
        assert not E.same(want["stop_flat"][i], E.alt_transform(p.voc, p.keyframe(i), stop=False)), name
    i = p.row("no_stopped")
    assert E.same(want["stop_flat"][i], E.alt_transform(p.voc, p.keyframe(i), stop=False))            # the control
    p = E.stop_tree().parts[0]
    for i, k in enumerate(p.keyframes()):
        assert not E.same(want["stop_tree"][i], E.alt_transform(p.voc, k, stop=False)), i


def test_full_runs_rule_out_count_times_weight(want):
    p = E.full().part("full")
    i = p.row("d_runs")
    w = want["full"][i]
    alt = E.alt_transform(p.voc, p.keyframe(i), value="mul")
    assert np.array_equal(w[0], alt[0]) and not E.same(w, alt)
    print("values that differ between repeated addition and multiplication: %d of %d" % ((w[1] != alt[1]).sum(), len(w[1])))
    assert (w[1] != alt[1]).sum() > len(w[1]) // 2


def test_full_distinct_rules_out_another_order_of_the_norm(want):
    p = E.full().part("full")
    i = p.row("a_distinct")
    for rule in ("pairwise", "desc"):
        assert not E.same(want["full"][i], E.alt_transform(p.voc, p.keyframe(i), norm=rule)), rule


def test_order_rules_out_another_order_of_the_score_sum():
    st = E.order()
    for j in (1, 2):
        a, b = st.vec(0), st.vec(j)
        s = ref_score(a, b)
        assert s == E.alt_score(a, b, "seq")
        assert s != E.alt_score(a, b, "reverse") and s != E.alt_score(a, b, "pairwise"), j


def test_uneven_rules_out_a_depth_bound_one_level_short(want):
    """voc_descend's `level <= depth` with depth = 13 here.  One level less loses the deepest leaf.  One level MORE cannot change any
    result on a tree (the descent has stopped at a leaf by then), so what is pinned is that `depth` is the tight bound: the smallest
    that gives the oracle's vectors."""
    r = E.uneven()
    p, depth = r.parts[0], r.figures["depth"]
    for i, k in enumerate(p.keyframes()):
        assert E.same(want["uneven"][i], E.alt_transform(p.voc, k, bound=depth)), i
        assert E.same(want["uneven"][i], E.alt_transform(p.voc, k, bound=depth + 1)), i
        assert not E.same(want["uneven"][i], E.alt_transform(p.voc, k, bound=depth - 1)), i
    i = p.row("deepest_only")
    assert len(E.alt_transform(p.voc, p.keyframe(i), bound=depth - 1)[0]) == 0
    # the descents end on every level from 1 to the deepest
    node = E.descend(p.voc, p.keyframe(p.row("every_leaf")))
    assert set((node[1] > 0).sum(1).tolist()) == set(range(1, depth + 1))
