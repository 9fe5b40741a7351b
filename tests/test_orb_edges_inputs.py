"""CPU: the inputs of tests/test_gpu_orb_edges.py do what they are there for, by the oracle alone (tests/_orb_edges.py builds them and
asserts each recipe's counts; here every recipe is built, and the figures the recipes rest on are pinned)."""
import numpy as np
import pytest

import _oracle as O
import _orb_edges as E


@pytest.mark.parametrize("name", sorted(E.RECIPES))
def test_recipe_lands_on_its_side_of_every_capacity(name):
    c = E.case(name)                    # its own check() has run
    assert c.total == c.counts.sum() and len(c.desc) == c.total
    k, d, ovf = c.expected(1 << 20)
    assert ovf == bool((c.counts > c.lvl_cap).any()) and len(k) == np.minimum(c.counts, c.lvl_cap).sum()
    if not ovf:
        assert np.array_equal(k, c.kps) and np.array_equal(d, c.desc)


def test_budgets_and_level_capacity_of_the_two_parameter_sets():
    assert list(O.orb_features_per_level(1000, 8, 1.2)) == [217, 181, 151, 126, 105, 87, 73, 60] and E.lvl_cap(**E.CLOSER) == 335
    assert list(O.orb_features_per_level(100, 5, 1.2)) == [28, 23, 19, 16, 14] and E.lvl_cap(**E.SMALL) == 99


def test_the_counts_the_recipes_were_chosen_for():
    lvl0 = {n: int(E.case(n).counts[0]) for n in ("dots14", "dots16", "dots17", "field4", "paste8", "paste10", "paste12", "corners")}
    assert lvl0 == dict(dots14=280, dots16=320, dots17=340, field4=14976, paste8=274, paste10=306, paste12=348, corners=147)
    assert E.case("paste8").total == 1057 and E.case("paste10").total == 1094 and E.case("kitti").total == 680
    assert E.case("small").total == 64 and E.empty_box_levels(E.case("small")) == [3, 4] == E.empty_box_levels(E.case("small_dots"))
    assert E.case("field7").counts[0] > 10 * E.case("field7").lvl_cap
    # one tie class: every dot of a grid has one FAST score and one Harris response
    for n in ("dots14", "dots16", "dots17", "field7", "field4", "small_dots"):
        c = E.case(n)
        assert c.survivors(0) == (c.counts[0], 1) and c.tie_class_at_cut(0) == c.counts[0], n
    # the pasted grids tie among themselves across the cut, beside corners of other responses
    for n, ny in (("paste8", 8), ("paste10", 10), ("paste12", 12)):
        assert E.case(n).tie_class_at_cut(0) == 20 * ny


def test_expected_truncation_keeps_prefixes():
    c = E.case("paste12")
    k, d, ovf = c.expected(E.CLOSER_CAP)
    assert ovf and len(k) == E.CLOSER_CAP
    lvl0 = c.level(0)[0]
    assert np.array_equal(k[:c.lvl_cap], lvl0[:c.lvl_cap]) and len(lvl0) == c.lvl_cap + 13
    assert np.array_equal(k[c.lvl_cap:c.lvl_cap + c.counts[1]], c.level(1)[0])          # a level that did not overflow is complete
    c = E.case("paste10")
    k, d, ovf = c.expected(E.CLOSER_CAP)
    assert ovf and np.array_equal(k, c.kps[:E.CLOSER_CAP]) and np.array_equal(d, c.desc[:E.CLOSER_CAP]) and c.total - len(k) == 70
    assert not c.expected(2048)[2]


def test_duplicate_descriptors_fail_the_ratio_test_in_the_oracle():
    rng = np.random.default_rng(11)
    a = E.random_desc(rng, 50)
    pairs = O.orb_match(a, np.concatenate([a, a[:10]]), 0.8)
    assert [tuple(p) for p in pairs] == [(i, i) for i in range(10, 50)]      # d0 = d1 = 0 for the duplicated ten: 0/0 is no ratio < 0.8
    assert len(O.orb_match(a, np.repeat(a[3:4], 20, axis=0), 0.8)) == 0
