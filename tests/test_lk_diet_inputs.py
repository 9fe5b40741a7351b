"""CPU: the inputs of tests/test_gpu_lk_diet.py reach what they are there for, by the oracle's trace and plain integer arithmetic alone
(tests/_lk_diet.py builds them and asserts each recipe's conditions; here every recipe is built and the figures it rests on are pinned)."""
import numpy as np
import pytest

import _lk_diet as D
import _lk_edges as E
import _oracle as O

ACC_MAX = 255 * 16384 + 256        # every pixel 255: the weights sum to 2^14 whatever they are
ACC_MIN = 256 - 255                # fourth weight -1 on a 255 pixel, the other three pixels 0


def test_the_sub_pixel_parts_are_the_corners_of_the_unit_square():
    p = [float(v) for v in D.PARTS]
    assert p == [0.0, 2.0 ** -20, 2.0 ** -15, 0.5 - 2.0 ** -20, 0.5 + 2.0 ** -20, 1 - 2.0 ** -15, 1 - 2.0 ** -20]
    # next to the coordinate 15 a float32 has no smaller part than 2^-20, and 1/2 -+ 2^-20 are the floats next to 15.5
    f = np.float32
    assert np.nextafter(f(15), f(16)) - f(15) == D.ULP and f(16) - np.nextafter(f(16), f(15)) == D.ULP
    assert np.nextafter(f(15.5), f(16)) - f(15) == D.PARTS[4] and np.nextafter(f(15.5), f(15)) - f(15) == D.PARTS[3]
    pp = D.part_pairs()
    assert pp.shape == (51, 2) and len({(float(a), float(b)) for a, b in pp}) == 51
    w = np.array([D.weights(a, b) for a, b in pp])
    assert (w.sum(1) == 16384).all() and (w[:, :3] >= 0).all() and w.max() == 16384
    assert w[:, 3].min() == -1 and [D.weights(a, b)[3] for a, b in D.MINUS_ONE] == [-1, -1]
    assert D.weights(*D.MINUS_ONE[0]) == (16325, 25, 35, -1)
    # the corners themselves: one weight takes everything, or two share it evenly to within one
    assert D.weights(0, 0) == (16384, 0, 0, 0) and D.weights(D.PARTS[6], D.PARTS[6]) == (0, 0, 0, 16384)
    assert D.weights(D.PARTS[3], 0) == (8192, 8192, 0, 0) and D.weights(0, D.PARTS[4]) == (8192, 0, 8192, 0)


@pytest.mark.parametrize("name", sorted(D.RECIPES))
def test_every_point_of_the_recipe_is_visited(name):
    c = D.case(name)                        # its own check has run
    assert c.prev.shape in D.SIZES and c.n <= 200 and c.levels == 0
    assert (c.tr["cause"] != E.CAUSE["not_visited"]).all() and (c.tr["cause"] != E.CAUSE["template_outside"]).all()
    out, st = O.lk(c.prev, c.nxt, c.pts, c.init, **c.kw)          # the trace changes nothing
    assert np.array_equal(out.view(np.uint32), c.out.view(np.uint32)) and np.array_equal(st, c.st)


def test_the_accumulator_reaches_both_ends_of_its_range():
    """first iteration of every corner case that iterates, recomputed from the start positions: 1 <= acc <= 255 * 2^14 + 2^8 < 2^22 and
    both ends are reached (the smallest on the single-pixel image under a fourth weight of -1), at both image sizes"""
    for (h, w), lvl in zip(D.SIZES, (0, 1)):
        got = {}
        for t, s in D.CORNER_PAIRS:
            if t in D.ITERATES:
                got[(t, s)] = D.first_visit_acc(D.case("corner_%s_%s_%dx%d_l%d" % (t, s, h, w, lvl)))
        assert len(got) == 7
        assert all(ACC_MIN <= lo and hi <= ACC_MAX < 2 ** 22 for lo, hi in got.values()), got
        assert got[("tex", "255")] == (ACC_MAX, ACC_MAX) and got[("tex", "0")] == (256, 256)
        assert got[("tex", "dots")][0] == ACC_MIN and got[("chk3", "dots")][0] == ACC_MIN
        assert got[("tex", "chk1")] == (256, ACC_MAX)


def test_saturated_templates_are_interpolated_and_found_flat():
    for (h, w), lvl in zip(D.SIZES, (0, 1)):
        for t, s in D.CORNER_PAIRS:
            c = D.case("corner_%s_%s_%dx%d_l%d" % (t, s, h, w, lvl))
            if t in D.ITERATES:
                assert c.st.all() and (c.tr["iters"][0] >= 1).all()
            else:
                assert not c.st.any() and (c.tr["iters"][0] == 0).all() and (c.tr["a11"][0] == 0).all() and (c.tr["a22"][0] == 0).all()
                assert np.array_equal(c.out, c.init)        # nothing iterated: the start comes back
    # the pinned mix of ways out on the saturated search images
    c = D.case("corner_chk3_chk3_32x32_l0")
    assert D.exit_counts(c) == dict(converged=58, oscillation=44, exhausted=0, left_image=0, flat=0)
    assert D.exit_counts(D.case("corner_tex_255_32x32_l0"))["exhausted"] == 102


def test_every_way_out_of_the_iteration_in_one_call():
    a, b = D.case("exits_a"), D.case("exits_b")
    assert a.prev.shape == b.prev.shape == (40, 64) and a.kw == b.kw and a.n != b.n
    ca, cb = D.exit_counts(a), D.exit_counts(b)
    assert ca == dict(converged=2, oscillation=45, exhausted=67, left_image=2, flat=0), ca
    assert cb == dict(converged=1, oscillation=37, exhausted=10, left_image=0, flat=6), cb
    assert all(ca[k] + cb[k] >= 1 for k in D.EXIT_CAUSES)
    # left the image MID-iteration: after at least one step, status 0
    gone = (a.tr["cause"][0] == E.CAUSE["left_image"]) & (a.tr["iters"][0] >= 1)
    assert gone.sum() == 2 and not a.st[gone].any()
    # neighbouring points (neighbouring waves) leave differently
    ch = a.tr["cause"][0]
    assert (ch[1:] != ch[:-1]).sum() >= 20


def test_batches_cover_the_recipes():
    assert sorted(n for names in D.BATCHES for n in names) == sorted(D.RECIPES) and len(D.BATCHES) == 3
    for names in D.BATCHES:
        assert len({(D.case(n).prev.shape, tuple(sorted(D.case(n).kw.items()))) for n in names}) == 1, names


def test_the_saturated_sequence_keeps_tracking():
    """tests/test_gpu_lk_diet.py runs the tracker's own LK launches on this sequence: by the oracle tracker alone it stays in state 1 with
    landmarks to track, on images of which nearly every pixel is 0 or 255"""
    import os
    import tempfile
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_lk_diet_kitti_like.yaml")
    open(p, "w").write(synth.KITTI_LIKE_YAML)
    outs, fig = D.scene_oracle(O.load_config(p))
    assert fig["state1"] >= 10 and min(fig["landmarks"][1:]) >= 40 and fig["saturated"] > 0.99, fig
