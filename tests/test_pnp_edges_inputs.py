"""CPU: the inputs of tests/test_gpu_pnp_edges.py reach the edges they are there for, by the oracle alone (every recipe of
tests/_pnp_edges.py asserts its own class when it is built; here every recipe is built and its figures are pinned)."""
import numpy as np
import pytest

import _pnp_edges as E

# correspondences the oracle sees, its inlier count, the index of the winning hypothesis (-1: no model), class
FIG = {
    "count_p3p_0": (0, 0, -1, 'count'),
    "count_p3p_1": (1, 0, -1, 'count'),
    "count_p3p_2": (2, 0, -1, 'count'),
    "count_p3p_3": (3, 0, -1, 'count'),
    "count_p3p_4": (4, 0, -1, 'count'),
    "count_p3p_5": (5, 4, 7, 'count'),
    "count_p3p_6": (6, 5, 1, 'count'),
    "count_p3p_7": (7, 6, 14, 'count'),
    "count_p3p_8": (8, 6, 10, 'count'),
    "count_p3p_9": (9, 7, 13, 'count'),
    "count_p3p_10": (10, 8, 6, 'count'),
    "count_p3p_11": (11, 9, 1, 'count'),
    "count_p3p_12": (12, 10, 2, 'count'),
    "count_p3p_13": (13, 9, 16, 'count'),
    "count_p3p_14": (14, 11, 5, 'count'),
    "count_p3p_15": (15, 12, 1, 'count'),
    "count_p3p_16": (16, 13, 5, 'count'),
    "count_p3p_17": (17, 14, 0, 'count'),
    "count_p3p_18": (18, 14, 4, 'count'),
    "count_p3p_19": (19, 14, 7, 'count'),
    "count_p3p_20": (20, 15, 2, 'count'),
    "count_p3p_21": (21, 15, 13, 'count'),
    "count_p3p_22": (22, 17, 8, 'count'),
    "count_p3p_23": (23, 16, 4, 'count'),
    "count_p3p_24": (24, 18, 9, 'count'),
    "count_p3p_63": (63, 48, 10, 'count'),
    "count_p3p_64": (64, 51, 6, 'count'),
    "count_p3p_65": (65, 52, 10, 'count'),
    "count_p3p_127": (127, 96, 5, 'count'),
    "count_p3p_128": (128, 102, 11, 'count'),
    "count_p3p_129": (129, 87, 10, 'count'),
    "count_p3p_511": (511, 400, 1, 'count'),
    "count_p3p_512": (512, 408, 5, 'count'),
    "count_p3p_513": (513, 391, 12, 'count'),
    "count_p3p_1023": (1023, 785, 4, 'count'),
    "count_p3p_1024": (1024, 813, 6, 'count'),
    "count_p3p_exact_clean": (4, 4, 0, 'count'),
    "count_p3p_exact_outlier": (4, 0, -1, 'count'),
    "clamp_p3p_2000": (32, 24, 16, 'count'),
    "clamp_p3p_-5": (0, 0, -1, 'count'),
    "limit_p3p_w15_1": (60, 0, -1, 'limit'),
    "limit_p3p_w15_15": (60, 0, -1, 'limit'),
    "limit_p3p_w15_16": (60, 30, 15, 'limit'),
    "limit_p3p_w15_17": (60, 30, 15, 'limit'),
    "limit_p3p_w15_79": (60, 30, 15, 'limit'),
    "limit_p3p_w15_80": (60, 30, 15, 'limit'),
    "limit_p3p_w15_81": (60, 30, 15, 'limit'),
    "limit_p3p_w15_100": (60, 30, 15, 'limit'),
    "limit_p3p_w16_1": (60, 0, -1, 'limit'),
    "limit_p3p_w16_15": (60, 0, -1, 'limit'),
    "limit_p3p_w16_16": (60, 0, -1, 'limit'),
    "limit_p3p_w16_17": (60, 29, 16, 'limit'),
    "limit_p3p_w16_79": (60, 29, 16, 'limit'),
    "limit_p3p_w16_80": (60, 29, 16, 'limit'),
    "limit_p3p_w16_81": (60, 29, 16, 'limit'),
    "limit_p3p_w16_100": (60, 29, 16, 'limit'),
    "limit_p3p_w17_79_1": (60, 0, -1, 'limit'),
    "limit_p3p_w17_79_15": (60, 0, -1, 'limit'),
    "limit_p3p_w17_79_16": (60, 22, 15, 'limit'),
    "limit_p3p_w17_79_17": (60, 22, 15, 'limit'),
    "limit_p3p_w17_79_79": (60, 26, 24, 'limit'),
    "limit_p3p_w17_79_80": (60, 26, 24, 'limit'),
    "limit_p3p_w17_79_81": (60, 26, 24, 'limit'),
    "limit_p3p_w17_79_100": (60, 26, 24, 'limit'),
    "limit_p3p_w80_1": (60, 0, -1, 'limit'),
    "limit_p3p_w80_15": (60, 24, 9, 'limit'),
    "limit_p3p_w80_16": (60, 24, 9, 'limit'),
    "limit_p3p_w80_17": (60, 24, 9, 'limit'),
    "limit_p3p_w80_79": (60, 28, 23, 'limit'),
    "limit_p3p_w80_80": (60, 28, 23, 'limit'),
    "limit_p3p_w80_81": (60, 28, 23, 'limit'),
    "limit_p3p_w80_100": (60, 30, 90, 'limit'),
    "cut_p3p_4_0.5": (65, 30, 17, 'cut'),
    "cut_p3p_4_0.99": (65, 33, 27, 'cut'),
    "cut_p3p_4_0.999999": (65, 33, 27, 'cut'),
    "cut_p3p_23_0.5": (65, 29, 39, 'cut'),
    "cut_p3p_23_0.99": (65, 32, 46, 'cut'),
    "cut_p3p_23_0.999999": (65, 32, 46, 'cut'),
    "threshold_p3p_0.5": (120, 56, 66, 'threshold'),
    "threshold_p3p_2": (120, 107, 5, 'threshold'),
    "threshold_p3p_3": (120, 108, 5, 'threshold'),
    "threshold_p3p_50": (120, 108, 1, 'threshold'),
    "nomodel_p3p_outliers": (60, 0, -1, 'no model'),
    "nomodel_p3p_ident3d": (60, 0, -1, 'no model'),
    "degenerate_p3p_negated": (60, 4, 27, 'degenerate'),
    "degenerate_p3p_duplicated": (120, 86, 3, 'degenerate'),
    "count_iterative_0": (0, 0, -1, 'count'),
    "count_iterative_1": (1, 0, -1, 'count'),
    "count_iterative_2": (2, 0, -1, 'count'),
    "count_iterative_3": (3, 0, -1, 'count'),
    "count_iterative_4": (4, 0, -1, 'count'),
    "count_iterative_5": (5, 0, -1, 'count'),
    "count_iterative_6": (6, 5, 8, 'count'),
    "count_iterative_7": (7, 6, 3, 'count'),
    "count_iterative_8": (8, 6, 7, 'count'),
    "count_iterative_9": (9, 7, 3, 'count'),
    "count_iterative_10": (10, 8, 4, 'count'),
    "count_iterative_11": (11, 9, 3, 'count'),
    "count_iterative_12": (12, 10, 1, 'count'),
    "count_iterative_13": (13, 10, 16, 'count'),
    "count_iterative_14": (14, 11, 2, 'count'),
    "count_iterative_15": (15, 12, 11, 'count'),
    "count_iterative_16": (16, 13, 3, 'count'),
    "count_iterative_17": (17, 14, 0, 'count'),
    "count_iterative_18": (18, 14, 6, 'count'),
    "count_iterative_19": (19, 15, 13, 'count'),
    "count_iterative_20": (20, 16, 5, 'count'),
    "count_iterative_21": (21, 16, 2, 'count'),
    "count_iterative_22": (22, 18, 9, 'count'),
    "count_iterative_23": (23, 18, 3, 'count'),
    "count_iterative_24": (24, 19, 2, 'count'),
    "count_iterative_63": (63, 50, 3, 'count'),
    "count_iterative_64": (64, 51, 0, 'count'),
    "count_iterative_65": (65, 52, 7, 'count'),
    "count_iterative_127": (127, 97, 6, 'count'),
    "count_iterative_128": (128, 102, 2, 'count'),
    "count_iterative_129": (129, 98, 8, 'count'),
    "count_iterative_511": (511, 402, 3, 'count'),
    "count_iterative_512": (512, 410, 1, 'count'),
    "count_iterative_513": (513, 408, 13, 'count'),
    "count_iterative_1023": (1023, 810, 2, 'count'),
    "count_iterative_1024": (1024, 805, 3, 'count'),
    "count_iterative_exact_clean": (5, 5, 0, 'count'),
    "count_iterative_exact_outlier": (5, 0, -1, 'count'),
    "clamp_iterative_2000": (32, 26, 12, 'count'),
    "clamp_iterative_-5": (0, 0, -1, 'count'),
    "limit_iterative_w7_1": (50, 0, -1, 'limit'),
    "limit_iterative_w7_7": (50, 0, -1, 'limit'),
    "limit_iterative_w7_8": (50, 14, 7, 'limit'),
    "limit_iterative_w7_9": (50, 14, 7, 'limit'),
    "limit_iterative_w7_16": (50, 14, 7, 'limit'),
    "limit_iterative_w7_17": (50, 14, 7, 'limit'),
    "limit_iterative_w7_100": (50, 14, 7, 'limit'),
    "limit_iterative_w8_1": (50, 0, -1, 'limit'),
    "limit_iterative_w8_7": (50, 0, -1, 'limit'),
    "limit_iterative_w8_8": (50, 0, -1, 'limit'),
    "limit_iterative_w8_9": (50, 20, 8, 'limit'),
    "limit_iterative_w8_16": (50, 20, 8, 'limit'),
    "limit_iterative_w8_17": (50, 20, 8, 'limit'),
    "limit_iterative_w8_100": (50, 20, 8, 'limit'),
    "limit_iterative_w16_1": (50, 0, -1, 'limit'),
    "limit_iterative_w16_7": (50, 0, -1, 'limit'),
    "limit_iterative_w16_8": (50, 0, -1, 'limit'),
    "limit_iterative_w16_9": (50, 0, -1, 'limit'),
    "limit_iterative_w16_16": (50, 0, -1, 'limit'),
    "limit_iterative_w16_17": (50, 0, -1, 'limit'),
    "limit_iterative_w16_100": (50, 20, 41, 'limit'),
    "cut_iterative_63_0.5": (65, 31, 49, 'cut'),
    "cut_iterative_63_0.99": (65, 32, 54, 'cut'),
    "cut_iterative_63_0.999999": (65, 32, 54, 'cut'),
    "cut_iterative_166_0.5": (65, 30, 43, 'cut'),
    "cut_iterative_166_0.99": (65, 33, 45, 'cut'),
    "cut_iterative_166_0.999999": (65, 33, 45, 'cut'),
    "threshold_iterative_0.5": (120, 63, 14, 'threshold'),
    "threshold_iterative_2": (120, 108, 4, 'threshold'),
    "threshold_iterative_3": (120, 108, 2, 'threshold'),
    "threshold_iterative_50": (120, 108, 1, 'threshold'),
    "nomodel_iterative_outliers": (60, 0, -1, 'no model'),
    "nomodel_iterative_ident3d": (60, 0, -1, 'no model'),
    "degenerate_iterative_negated": (60, 40, 64, 'degenerate'),
    "degenerate_iterative_duplicated": (120, 88, 1, 'degenerate'),
    "nomodel_p3p_ident2d": (60, 0, -1, 'no model'),
    "degenerate_p3p_planar": (60, 53, 2, 'degenerate'),
    "nomodel_iterative_planar": (60, 0, -1, 'no model'),
    "degenerate_p3p_collinear": (60, 55, 12, 'degenerate'),
    "nomodel_iterative_collinear": (60, 0, -1, 'no model'),
}


def test_every_recipe_is_pinned():
    assert sorted(FIG) == sorted(E.RECIPES)
    assert sorted(n for names in E.GROUPS.values() for n in names) == sorted(E.RECIPES)
    assert {r.cls for r in E.RECIPES.values()} == set(E.CLASSES)
    assert max(len(v) for v in E.GROUPS.values()) <= 60 and all(E.DEFAULT_GROUP[b] in E.GROUPS for b in E.BRANCHES)


@pytest.mark.parametrize("name", sorted(E.RECIPES))
def test_recipe_reaches_its_edge(name):
    c = E.case(name)                    # its own check() has run
    assert c.pinned() == FIG[name]


def test_recipes_follow_the_tuple_contract():
    for name in E.RECIPES:
        P, uv, branch, iterations, reproj, conf, g = E.recipe(name)
        assert P.dtype == uv.dtype == np.float32 and P.shape == (len(uv), 3) and uv.shape == (len(P), 2) and len(P) <= E.RECIPES[name].cap
        assert branch in E.BRANCHES and iterations >= 1 and reproj > 0 and 0 < conf < 1
        assert (g is None) == (branch == E.P3P)
        if g is not None:                                            # w > 0, unit, and not the identity
            assert g[6] > 0 and abs(np.linalg.norm(g[3:7]) - 1) < 1e-15 and np.abs(g[:6]).max() > 1e-3


def test_count_recipes_cover_every_count_and_yield_a_model_from_eight():
    for b in E.BRANCHES:
        mp = E.MODEL_POINTS[b]
        ns = [E.case("count_%s_%d" % (b, n)) for n in E.COUNTS]
        assert [c.n for c in ns] == list(E.COUNTS) and set(range(25)) | {63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024} == set(E.COUNTS)
        assert all(c.inliers > 0 for c in ns if c.n >= 8) and all(c.inliers == 0 and c.winner == -1 for c in ns if c.n < mp)
        assert FIG["count_%s_%d" % (b, mp - 1)][1] == 0
        assert FIG["count_%s_exact_clean" % b][:3] == (mp, mp, 0) and FIG["count_%s_exact_outlier" % b][:2] == (mp, 0)
        big, none = E.case("clamp_%s_2000" % b), E.case("clamp_%s_-5" % b)
        assert (big.count, big.n, big.cap, none.count, none.n, none.cap) == (2000, 32, 32, -5, 0, 32) and big.inliers > 0
        p3, p2 = none.rows()                                         # a solvable scene lies where a negative count must not look
        assert np.abs(p3).max() < 100 and E.oracle(p3, p2, b, *E.DEFAULT[b], E.guess_for("x"))[0] > 0
    p3, p2 = E.case("count_p3p_7").rows()
    assert p3.shape == (1024, 3) and np.all(p3[7:] == E.GARBAGE) and np.all(p2[7:] == E.GARBAGE) and np.abs(p3[:7]).max() < 100


def test_limit_recipes_put_the_winner_on_both_sides_of_every_batch_edge():
    w = {(b, t): FIG["limit_%s_%s_100" % (b, t)][2] for b in E.BRANCHES for t in E.LIMIT_SETS[b]["seeds"]}
    assert (w["p3p", "w15"], w["p3p", "w16"], w["iterative", "w7"], w["iterative", "w8"]) == (15, 16, 7, 8)
    assert 17 <= w["p3p", "w17_79"] <= 79 and w["p3p", "w80"] >= 80 and w["iterative", "w16"] >= 16
    assert E.LIMITS[E.P3P] == (1, 15, 16, 17, 79, 80, 81, 100) and E.LIMITS[E.ITER] == (1, 7, 8, 9, 16, 17, 100)
    for (b, t), wk in w.items():
        full = FIG["limit_%s_%s_100" % (b, t)][1]
        for L in E.LIMITS[b]:
            n, inl, win, _ = FIG["limit_%s_%s_%d" % (b, t, L)]
            assert (inl, win) == (full, wk) if L > wk else (inl < full and win < L), (b, t, L)   # one iteration short of the winner loses it


def test_cut_recipes_stop_in_front_of_a_better_hypothesis_of_their_sub_batch():
    assert all(len(E.CUT_SETS[b]["seeds"]) >= 2 for b in E.BRANCHES) and E.CONFS == (0.5, 0.99, 0.999999)
    assert [E.sub_batch(E.P3P, k) for k in (0, 15, 16, 31, 32)] == [0, 0, 1, 1, 2] and [E.sub_batch(E.ITER, k) for k in (7, 8, 15, 16)] == [0, 1, 1, 2]
    for b in E.BRANCHES:
        for s in E.CUT_SETS[b]["seeds"]:
            lo, hi = FIG["cut_%s_%d_0.5" % (b, s)], FIG["cut_%s_%d_0.999999" % (b, s)]
            assert 0 < lo[1] < hi[1] and lo[2] < hi[2] and E.sub_batch(b, lo[2]) == E.sub_batch(b, hi[2]), (b, s)


def test_threshold_and_degenerate_recipes():
    for b in E.BRANCHES:
        inl = [FIG["threshold_%s_%g" % (b, r)][1] for r in E.REPROJS]
        assert inl == sorted(inl) and inl[0] < 0.6 * 120 and inl[-1] >= 0.9 * 120 and E.REPROJS == (0.5, 2.0, 3.0, 50.0)
        assert FIG["threshold_%s_50" % b][2] < E.SUB_BATCH[b]
    none = sorted(n for n, f in FIG.items() if f[3] == "no model")
    assert none == sorted(["nomodel_%s_%s" % (b, k) for b in E.BRANCHES for k in ("outliers", "ident3d")] +
                          ["nomodel_p3p_ident2d", "nomodel_iterative_planar", "nomodel_iterative_collinear"])
    assert all(FIG[n][1] == 0 for n in none) and "nomodel_iterative_ident2d" not in FIG          # (dropped by the keeping rule: |t| = 1e14)
    deg = sorted(n for n, f in FIG.items() if f[3] == "degenerate")
    assert deg == sorted(["degenerate_%s_%s" % (b, k) for b in E.BRANCHES for k in ("negated", "duplicated")] +
                         ["degenerate_p3p_planar", "degenerate_p3p_collinear"]) and all(FIG[n][1] > 0 for n in deg)
    for b in E.BRANCHES:                                             # the duplicated set: twice the inliers of the set itself
        P, uv, _, it, rp, cf, g = E.recipe("degenerate_%s_duplicated" % b)
        assert E.oracle(P[:60], uv[:60], b, it, rp, cf, g)[0] * 2 == FIG["degenerate_%s_duplicated" % b][1]


def test_the_final_epnp_fails_on_the_flat_scenes_so_the_p3p_pose_is_kept():
    """solvePnPRansac's fallback: EPnP on the inliers of the planar and the collinear scene finds no pose, the winning P3P hypothesis is
    returned; everywhere else under P3P the final EPnP succeeds"""
    import _oracle as O
    failed = []
    for name, r in E.RECIPES.items():
        c = E.case(name)
        if r.branch == E.P3P and c.inliers > 0:
            idx = np.flatnonzero(c.mask)
            if not O.solve_epnp(c.P[idx], c.uv[idx], E.K4)[0]:
                failed.append(name)
    assert failed == ["degenerate_p3p_planar", "degenerate_p3p_collinear"]
