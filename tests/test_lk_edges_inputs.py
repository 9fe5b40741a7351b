"""CPU: the inputs of tests/test_gpu_lk_edges.py do what they are there for, by the oracle's trace alone (tests/_lk_edges.py builds them
and asserts each recipe's conditions; here every recipe is built, and the figures the recipes rest on are pinned: a changed generator
fails here instead of silently no longer reaching its edge)."""
import numpy as np
import pytest

import _oracle as O
import _lk_edges as E

# per recipe: points, status-1 points, points that moved > 4 px in y / > 4 px in x / > 11 px in x within a level, that exhausted the
# iterations, that left the image mid-iteration (each at the level where most did), that were flat at level 0; largest Hessian sum
# (|iA11|, |iA22|) and largest residual sum (|ib1|, |ib2|) over all visits
COLS = ("n", "ok", "y4", "x4", "x11", "exhausted", "left", "flat0", "hessian", "residual")
FIG = {
    "far12_l0": (150, 149, 91, 90, 17, 12, 1, 0, 32688925, 128528196),
    "far12_l1": (150, 150, 38, 33, 0, 0, 0, 0, 45738597, 121284364),
    "far25_l0": (150, 137, 102, 112, 50, 39, 13, 0, 32688925, 120481071),
    "far25_l1": (137, 132, 93, 89, 14, 6, 5, 0, 45738597, 161333780),
    "far_neg_x": (150, 149, 18, 143, 55, 15, 1, 0, 32688925, 67272444),
    "far_neg_y": (150, 150, 110, 4, 0, 4, 0, 0, 32688925, 196253027),
    "flat": (234, 107, 0, 0, 0, 18, 0, 127, 575524518, 713247124),
    "constant": (140, 0, 0, 0, 0, 0, 0, 140, 0, 0),
    "blocks1_inverse": (88, 88, 7, 9, 0, 79, 0, 0, 1990216975, 370321500),
    "blocks1_roll": (88, 88, 0, 0, 0, 5, 0, 0, 1990216975, 1983703093),
    "blocks1_same": (88, 88, 0, 0, 0, 0, 0, 0, 1990216975, 0),
    "blocks2_inverse": (88, 88, 24, 17, 0, 78, 0, 0, 4016910306, 1143339854),
    "blocks2_roll": (88, 88, 0, 0, 0, 0, 0, 0, 4016910306, 814265254),
    "blocks2_same": (88, 88, 0, 0, 0, 0, 0, 0, 4016910306, 0),
    "blocks4_inverse": (88, 88, 29, 15, 0, 74, 0, 0, 3430184479, 2803201716),
    "blocks4_roll": (88, 88, 0, 0, 0, 0, 0, 0, 3430184479, 1459026411),
    "blocks4_same": (88, 88, 0, 0, 0, 0, 0, 0, 3430184479, 0),
    "stripes_v": (88, 85, 24, 24, 24, 29, 3, 0, 8005381320, 8772830628),
    "stripes_h": (88, 80, 22, 22, 22, 37, 8, 0, 8728597341, 9816877715),
    "tiny_32x32": (64, 64, 0, 0, 0, 0, 0, 0, 72073874, 77474388),
    "tiny_64x64": (256, 256, 0, 0, 0, 0, 0, 0, 135822762, 99541970),
    "tiny_33x47": (96, 96, 0, 0, 0, 0, 0, 0, 63417717, 67119740),
    "tiny_64x40": (160, 160, 0, 0, 0, 0, 0, 0, 86125940, 93008204),
    "tiny_40x200": (500, 500, 0, 0, 0, 0, 0, 0, 38882691, 50873220),
    "rim_template": (204, 60, 0, 0, 0, 0, 0, 66, 457740287, 0),
    "rim_search": (204, 94, 0, 0, 0, 69, 110, 0, 3872173725, 736603200),
    "step_out": (24, 14, 6, 10, 0, 7, 10, 0, 49635736, 103908970),
    "clamp_it0": (100, 100, 0, 0, 0, 100, 0, 0, 50551611, 0),
    "clamp_it1": (100, 100, 0, 0, 0, 100, 0, 0, 50551611, 116113787),
    "clamp_it100": (100, 98, 47, 69, 30, 2, 2, 0, 31050535, 110063679),
    "clamp_it250": (100, 98, 47, 69, 30, 2, 2, 0, 31050535, 110063679),
    "clamp_eps0": (100, 98, 22, 43, 1, 1, 2, 0, 50551611, 116113787),
    "clamp_eps10": (100, 100, 0, 0, 0, 0, 0, 0, 50551611, 116113787),
    "clamp_eps50": (100, 100, 0, 0, 0, 0, 0, 0, 50551611, 116113787),
    "clamp_level0": (100, 99, 46, 69, 29, 10, 1, 0, 31050535, 110063679),
    "clamp_noinit": (100, 99, 0, 1, 1, 0, 1, 0, 50551611, 74905504),
}


def test_every_recipe_is_pinned():
    assert sorted(FIG) == sorted(E.RECIPES)


@pytest.mark.parametrize("name", sorted(E.RECIPES))
def test_the_counts_the_recipe_was_chosen_for(name):
    c = E.case(name)                        # its own check has run
    f = dict(c.figures(), hessian=c.hessian(), residual=c.residual())
    assert tuple(f[k] for k in COLS) == FIG[name], (name, f)
    assert c.n <= 240 or name.startswith("tiny")
    assert c.hessian() <= E.HESSIAN_BOUND
    # the trace changes nothing: the untraced entry returns the same bits
    out, st = O.lk(c.prev, c.nxt, c.pts, c.init, **c.kw)
    assert np.array_equal(out.view(np.uint32), c.out.view(np.uint32)) and np.array_equal(st, c.st)
    # a visit that iterated ended for one of the four reasons an iteration can end; one that did not was rejected or had max_iter = 0
    ran = c.tr["iters"] > 0
    assert np.isin(c.tr["cause"][ran], [E.CAUSE[k] for k in ("converged", "oscillation", "exhausted", "left_image")]).all()
    assert (c.tr["cause"] != E.CAUSE["not_visited"]).all() and c.tr["iters"].max() <= 100


def test_far_starts_leave_the_staged_region_in_every_direction():
    """the issue's conditions, each at some level of some far_start case: >= 20 points move > 4 px in y, >= 20 in x, >= 5 move > 11 px in
    x, >= 5 exhaust the iterations, >= 3 leave the image mid-iteration; and the one-sided variants move most points their own way"""
    far = [E.case(n) for n in ("far12_l0", "far12_l1", "far25_l0", "far25_l1")]
    assert all(c.moved("y", 4) >= 20 and c.moved("x", 4) >= 20 for c in far)
    assert all(c.moved("x", 11) >= 5 and c.cause("exhausted") >= 5 for c in (far[0], far[2], far[3]))
    assert all(c.cause("left_image") >= 3 for c in far[2:])
    assert [c.levels for c in far] == [0, 1, 0, 1]
    nx, ny = E.case("far_neg_x"), E.case("far_neg_y")
    assert (nx.init[:, 0] < nx.pts[:, 0] - 2.9).all() and np.array_equal(nx.init[:, 1], nx.pts[:, 1])
    assert (ny.init[:, 1] < ny.pts[:, 1] - 2.9).all() and np.array_equal(ny.init[:, 0], ny.pts[:, 0])
    # toward -x the aligned-down region edge is 4..7 px away: some windows move 5..7 px, enough to leave it at some alignments only
    mx = nx.tr["move_x"][0]
    assert ((mx > 4) & (mx <= 7)).sum() >= 20 and (mx > 7).sum() >= 20


def test_flat_templates_at_either_level():
    c = E.case("flat")
    assert E.flat_figures(c) == dict(flat0=127, flat1=57, mixed=70, ok=107)
    f = E.flat_figures(c)
    assert f["flat0"] >= 50 and f["flat1"] >= 20 and f["mixed"] >= 10 and f["ok"] >= 10
    # status 0 at level 0 exactly where the template is flat there (nothing leaves this image)
    assert np.array_equal(c.st == 0, c.tr["cause"][0] == E.CAUSE["flat"])
    # a pure-aperture template: a Hessian with one large sum and the other 0
    a11, a22 = c.tr["a11"][0], c.tr["a22"][0]
    assert (((a11 > 10 ** 7) & (a22 == 0)) | ((a22 > 10 ** 7) & (a11 == 0))).sum() >= 10
    k = E.case("constant")
    assert not k.st.any() and (k.tr["cause"] == E.CAUSE["flat"]).all() and k.levels == 1
    # nothing iterated: the output is the start position carried down the levels (x / 2 * 2: itself)
    assert np.array_equal(k.out, k.init)


def test_contrast_reaches_a_quarter_of_the_hessian_bound():
    names = [n for n in E.RECIPES if n.startswith(("blocks", "stripes"))]
    assert len(names) == 11
    assert max(E.case(n).hessian() for n in names if n.startswith("blocks")) == 4016910306 >= 2e9
    assert max(E.case(n).hessian() for n in names) == 8728597341 > 0.5 * E.HESSIAN_BOUND
    assert max(E.case(n).residual() for n in names) == 9816877715 > 2 ** 33                   # beyond any 32-bit sum
    for cell in (1, 2, 4):
        assert E.case("blocks%d_inverse" % cell).cause("exhausted") >= 50
        same = E.case("blocks%d_same" % cell)
        assert (same.tr["cause"] == E.CAUSE["converged"]).all() and (same.tr["iters"] == 1).all() and same.residual() == 0
        assert np.array_equal(same.out, same.pts)


def test_tiny_images_have_no_level_below_32():
    assert [E.case("tiny_%dx%d" % s).level_sizes() for s in E.TINY_SIZES] == [[(32, 32)], [(64, 64), (32, 32)], [(33, 47)], [(64, 40)], [(40, 200)]]
    for s in E.TINY_SIZES:
        c = E.case("tiny_%dx%d" % s)
        assert c.n == ((s[0] + 1) // 4) * ((s[1] + 2) // 4) and c.st.all()


def test_rim_points_sit_on_both_sides_of_every_threshold():
    want = {"rim_template": dict(left=(12, 30), right=(18, 36), top=(12, 30), bottom=(18, 36)),
            "rim_search": dict(left=(15, 30), right=(29, 36), top=(20, 30), bottom=(30, 36))}
    for name, w in want.items():
        c = E.case(name)
        got = {g: (int(c.st[(c.group == g) & c.inside].sum()), int(((c.group == g) & c.inside).sum())) for g in w}
        assert got == w, (name, got)
        assert int((~c.inside).sum()) == 2 * 6 * 6 and not c.st[~c.inside].any()
    # window starts: exactly on the thresholds, and one float off them
    c = E.case("rim_template")
    sx = np.floor(c.pts[:, 0] - np.float32(15))
    for v in (-32, -31, E.W - 1, E.W):
        assert (sx == v).sum() >= 6, v
    assert (c.pts[:, 0] - np.float32(15) == np.nextafter(np.float32(-31), np.float32(0))).sum() == 6
    # inside starts whose first step leads outside
    s = E.case("step_out")
    gone = (s.tr["cause"][0] == E.CAUSE["left_image"]) & (s.tr["iters"][0] >= 1)
    assert gone.sum() == 10 and not s.st[gone].any()


def test_clamped_arguments_equal_their_clamps():
    it0, it1, it100, it250 = (E.case("clamp_it%d" % k) for k in (0, 1, 100, 250))
    assert (it0.tr["iters"] == 0).all() and it0.st.all() and (it1.tr["iters"] == 1).all()
    assert np.array_equal(it0.out, it0.init)                 # 0 iterations: the start, halved and doubled
    assert np.array_equal(it100.out.view(np.uint32), it250.out.view(np.uint32)) and np.array_equal(it100.st, it250.st)
    assert int((it100.tr["iters"] > 30).sum()) == 10 and it100.tr["iters"].max() == 100
    lvl0 = E.case("clamp_level0")
    assert not np.array_equal(it100.out, lvl0.out)           # (the same call at 30 iterations)
    e0, e10, e50 = (E.case("clamp_eps%d" % k) for k in (0, 10, 50))
    assert e0.cause("converged") == 0 and e0.cause("oscillation") == 99
    assert np.array_equal(e10.out.view(np.uint32), e50.out.view(np.uint32)) and (e10.tr["iters"] == 1).all()
    assert (e10.tr["cause"] == E.CAUSE["converged"]).all()
    assert lvl0.levels == 0 and E.case("clamp_eps0").levels == 1
    ni = E.case("clamp_noinit")
    d = ni.out[ni.st == 1] - ni.pts[ni.st == 1]
    assert np.median(np.hypot(d[:, 0] - 6.7, d[:, 1] + 2.2)) < 0.05


def test_batches_mix_recipes_of_one_size():
    b = E.BATCHES
    assert sorted(n for names in b for n in names) == sorted(E.RECIPES)
    assert max(len(names) for names in b) == 13 and sum(len(names) > 1 for names in b) == 3
    for names in b:
        assert len({(E.case(n).prev.shape, tuple(sorted(E.case(n).kw.items()))) for n in names}) == 1, names
        assert len(names) == 1 or len({E.case(n).n for n in names}) > 1, names          # ragged counts


def test_the_crafted_sequence_keeps_tracking_while_landmarks_cross_the_image_edges():
    """tests/test_gpu_lk_edges.py runs the tracker's own LK launches on this sequence; by the oracle tracker alone: state 1 throughout,
    landmarks next to the edges, landmarks lost to the LK status, and search regions that reach over the pyramids' physical border"""
    import os
    import tempfile
    from flvis_amd import synth
    assert (synth.KITTI_W, synth.KITTI_H, synth.KITTI_FX, synth.KITTI_LIKE_BASELINE) == (E.SCENE_W, E.SCENE_H, E.SCENE_FX, E.SCENE_B)
    p = os.path.join(tempfile.gettempdir(), "flvis_lk_edges_kitti_like.yaml")
    open(p, "w").write(synth.KITTI_LIKE_YAML)
    outs, fig = E.scene_oracle(O.load_config(p))
    assert fig["state1"] >= 10 and fig["near_edge"] >= 30 and fig["lost_to_status"] >= 10, fig
    lms = fig.pop("landmarks")
    assert fig == dict(state1=12, near_edge=43, lost_at_lk=36, lost_to_status=15, border_misses=34) and 90 <= min(lms) <= max(lms) <= 130, (fig, lms)
