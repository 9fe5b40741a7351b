"""CPU: the inputs of tests/test_gpu_gftt_edges.py reach the edges they are there for, by the oracle and the tier model of
tests/_gftt_edges.py alone (every recipe asserts its own path when it is built; here every recipe is built and its figures are pinned)."""
import numpy as np
import pytest

import _gftt_edges as E
import _oracle as O

# goodFeaturesToTrack: candidates, kept above the quality threshold, largest histogram bin, keys of every walked tier, full sort taken,
# accepted corners, rank (1-based, in walk order) of the last accepted one, largest class of equal responses
# FeatureDEM: GFTT corners, features, features of the fullest region, existing points of the fullest region
FIG = {
    "tier_second": (4313, 4313, 366, (906, 3407), False, 300, 1926, 1),
    "tier_first_only": (4313, 4313, 366, (906,), False, 100, 163, 1),
    "switch_341": (4205, 4205, 297, (846, 3359), False, 333, 4202, 2),
    "switch_342": (4205, 4205, 297, (1025, 3180), False, 333, 4202, 2),
    "switch_1365": (4313, 4313, 366, (4039,), False, 1365, 1365, 1),
    "switch_1366": (4313, 4313, 366, (4039,), False, 1366, 1366, 1),
    "exhausted": (4313, 4313, 366, (4039, 274), False, 132, 4147, 1),
    "full_md3": (4836, 4836, 4836, (), True, 150, 533, 4836),
    "full_md0": (4836, 4836, 4836, (), True, 150, 150, 4836),
    "full_slices": (7332, 7332, 7332, (), True, 1500, 5913, 7332),
    "full_after_tiers": (5215, 5215, 4522, (59,), True, 1831, 5215, 4512),
    "plateau_tile_a": (736, 736, 256, (736,), False, 500, 500, 256),
    "plateau_tile_b": (1233, 1233, 272, (1233,), False, 500, 980, 256),
    "plateau_b5": (2852, 2852, 2852, (2852,), False, 300, 1157, 2852),
    "over_b2_64": (3600, 3600, 3596, (4, 3596), False, 200, 1668, 3596),
    "over_b3_64": (3600, 3600, 3600, (3600,), False, 200, 1678, 3600),
    "over_b2_96": (11408, 11408, 11404, (4,), True, 200, 1575, 11404),
    "over_b3_96": (11500, 11500, 11500, (), True, 200, 1594, 11500),
    "space_0": (754, 754, 55, (754,), False, 300, 300, 1),
    "space_0.99": (754, 754, 55, (754,), False, 300, 300, 1),
    "space_1": (754, 754, 55, (754,), False, 300, 300, 1),
    "space_1.5": (754, 754, 55, (754,), False, 300, 300, 1),
    "space_2": (754, 754, 55, (754,), False, 300, 300, 1),
    "space_2.5": (754, 754, 55, (754,), False, 300, 365, 1),
    "space_4.5": (754, 754, 55, (754,), False, 263, 748, 1),
    "far_63.5": (4313, 4313, 366, (906, 3407), False, 19, 1036, 1),
    "far_64": (4313, 4313, 366, (906, 3407), False, 19, 1036, 1),
    "borders_w132": (749, 749, 53, (749,), False, 200, 741, 1),
    "quality_1": (754, 0, 0, (), False, 0, 0, 0),
    "quality_tiny": (754, 754, 55, (754,), False, 754, 754, 1),
    "ragged_full": (4836, 4836, 4836, (), True, 150, 533, 4836),
    "ragged_flat": (0, 0, 0, (), False, 0, 0, 0),
    "ragged_exhausted": (188, 188, 14, (188,), False, 135, 188, 1),
    "ragged_plain": (1154, 1154, 92, (1010,), False, 150, 163, 1),
    "next_plain": (754, 754, 55, (754,), False, 300, 365, 1),
    "next_over": (11500, 11500, 11500, (), True, 300, 2641, 11500),
    "dem_8x8": (2, 0, 0, 0),
    "dem_12x16": (7, 4, 1, 0),
    "dem_32x32": (37, 19, 2, 0),
    "dem_64x64": (160, 47, 4, 0),
    "dem_96x128": (400, 88, 7, 0),
    "dem_100x132": (400, 83, 7, 0),
    "dem_re_12x16": (7, 4, 1, 0),
    "dem_re_100x132": (200, 68, 5, 0),
    "dem_maxc": (4096, 375, 26, 0),
    "dem_int_md": (400, 82, 7, 0),
    "dem_bd0": (400, 128, 8, 0),
    "redetect_crowded": (200, 63, 6, 204),
    "redetect_at_capacity": (200, 64, 6, 192),
    "redetect_over_capacity": (200, 64, 6, 217),
    "redetect_places": (200, 64, 5, 2),
    "redetect_full_region": (200, 55, 6, 9),
    "dem_tied": (736, 117, 8, 0),
    "dem_tied_re": (736, 78, 6, 3),
}


def test_every_recipe_is_pinned():
    assert sorted(FIG) == sorted(E.RECIPES) == sorted(E.GFTT + E.DEM)
    assert all(n in E.RECIPES for names in E.BATCHES.values() for n in names) and set(E.PLATEAUS + E.OVER) <= set(E.GFTT)


@pytest.mark.parametrize("name", sorted(E.RECIPES))
def test_recipe_reaches_its_edge(name):
    c = E.case(name)                    # its own check() has run
    assert c.pinned() == FIG[name]


def test_batches_share_their_size_and_parameters():
    for names in E.BATCHES.values():
        cs = [E.case(n) for n in names]
        assert len({(c.img.shape, c.maxc, c.q, c.md) for c in cs}) == 1
    assert E.case("ragged_full").img.shape != E.case("next_over").img.shape


def test_the_paths_the_recipes_cover_between_them():
    f = {n: E.case(n).fig for n in E.GFTT}
    assert f["tier_second"]["last"] > f["tier_second"]["tiers"][0] == 906 < 1024                      # a second tier after a small first one
    assert f["switch_341"]["tiers"][0] < 1025 == f["switch_342"]["tiers"][0]                          # 1024 and 1026 cut at different bins
    assert 3 * 1365 < E.SORT_LDS <= 3 * 1366
    assert f["exhausted"]["exhausted"] and sum(f["exhausted"]["tiers"]) == f["exhausted"]["kept"]      # hi == 0 below maxCorners
    assert f["full_md3"]["full"] and not f["full_md3"]["tiers"]                                      # the full sort at first look
    assert f["full_after_tiers"]["full"] and f["full_after_tiers"]["tiers"] == [59]                  # ... and after a walked tier
    assert f["full_slices"]["last"] > E.SORT_LDS and f["full_slices"]["slices"] == 2                 # the walk crosses a slice boundary
    assert E.case("space_0").md < 1 and E.case("space_0.99").md < 1                                   # use_dist off
    assert f["quality_1"]["kept"] == 0 and f["quality_tiny"]["accepted"] == f["quality_tiny"]["cand"]
    for n in E.OVER + ("next_over",):
        c = E.case(n)
        assert E.old_key_cap(c.w, c.h) < f[n]["cand"] <= (c.w - 2) * (c.h - 2) <= E.key_cap(c.w, c.h)
    assert (E.old_key_cap(64, 64), E.old_key_cap(128, 96), E.key_cap(64, 64), E.key_cap(128, 96)) == (2048, 4096, 4096, 16384)
    assert (E.old_key_cap(640, 480), E.key_cap(640, 480)) == (131072, 524288)
    # plateaus: whole classes of equal response, ordered by pixel offset (descending) alone
    for n in E.PLATEAUS:
        c = E.case(n)
        mx, o, off = E.candidates(c.img)
        same = o[1:] == o[:-1]
        assert same.sum() >= 255 and np.all(off[1:][same] < off[:-1][same])


def test_half_distances_round_to_even_and_the_disc_is_strict():
    """lrint (the oracle's grid cell) and __double2int_rn (the device's row range) round halves to even: 1.5 -> 2, 2.5 -> 2, 4.5 -> 4,
    63.5 -> 64; dx^2 + dy^2 < minDistance^2 strictly, so a neighbour at exactly minDistance survives"""
    assert [int(np.rint(v)) for v in (1.5, 2.5, 4.5, 63.5)] == [2, 2, 4, 64]
    for n in ("space_1", "space_1.5", "space_2", "space_2.5", "space_4.5", "far_63.5", "far_64"):
        c = E.case(n)
        d = c.want[:, None, :].astype(np.float64) - c.want[None, :, :]
        d2 = (d ** 2).sum(-1) + np.eye(len(c.want)) * 1e9
        assert d2.min() >= c.md ** 2, (n, d2.min())
    d = E.case("space_2").want
    assert ((d[:, None, :] - d[None, :, :]) ** 2).sum(-1)[~np.eye(len(d), dtype=bool)].min() == 4.0   # neighbours at exactly minDistance
    assert not np.array_equal(E.case("space_2.5").want, E.case("space_2").want)
    assert np.array_equal(E.case("space_0").want, E.case("space_0.99").want)


def test_feature_dem_recipes_touch_their_capacities():
    assert len(E.case("dem_maxc").gftt) == E.DEM_MAXC
    c = E.case("redetect_crowded")
    assert c.exist_regions[0] == 204 > E.DEM_MAXR and c.regions[0] == 0                 # the late existing points block region 0 altogether
    for n, k in (("redetect_at_capacity", E.DEM_MAXR), ("redetect_over_capacity", E.DEM_MAXR + 25)):    # ... or leave it one new point
        assert E.case(n).exist_regions[0] == k and E.case(n).regions[0] == 1
    c = E.case("redetect_full_region")
    assert int(c.fp[0]) == 8 and list(c.exist_regions[[0, 5, 15]]) == [8, 9, 7] and list(c.regions[[0, 5, 15]]) == [1, 1, 1]
    assert E.tied_region(E.case("dem_tied")) == (40, 16)
    assert int(E.case("dem_int_md").fp[5]) == 0 and not np.array_equal(E.case("dem_int_md").want, E.case("dem_96x128").want)
    assert E.case("dem_8x8").want.shape == (0, 2)
