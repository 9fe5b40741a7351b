"""The inputs of tests/test_gpu_stereo_depth_edges.py, checked without a GPU: every recipe of tests/_sd_edges.py is run through the oracle
(O.Tracker.stereo_depth) alone and must reach the edge it was written for -- failures and successes in every batch of 1024 landmarks,
every class of wrong seed populated, both mask values either side of a range, a z beyond 1e6 at zero disparity.  The figures are printed
(pytest -s) and the ones that decide whether an edge is reached are pinned from below.

As measured when the recipes were written: failures per batch 240 / 239 / 1 in the sets of 1023 to 2049 landmarks (240 + 1 and 8 of 17 on the
KITTI-like and EuRoC-like rig); 37 of 96 and 17 of 40 where the count exceeds the capacity; 192 of 200 landmarks matched at d = 1, 8 and
40, of which 0 / 96 / 97 / 192 pass the four ranges (98 / 99 at d = 8); 108 of 203 pass at d = 0, 60 of them with z > 1e6 and the 3 with a
NaN pixel with a NaN z (no other input produced a non-finite z); all 200 fail at d = -8; per class of wrong seed 6 landmarks on and 6 behind
the plane of camera 1 (none on it on the EuRoC-like rig), 9 next to it, 6 outside each side of the image, 8 next to each border of which
4 to 7 are matched; 198, 122, 158 and 76 draws per slot over the four carried calls."""
import numpy as np

import _oracle as O
import _sd_edges as E


def test_batch_boundary_recipe_has_failures_and_successes_in_every_batch():
    c = E.batch_call()
    assert [s.n for s in c.sets] == [0, 1, 1023, 1024, 1025, 2048, 2049] and c.cap == 2049
    assert not np.array_equal(c.sets[0].pose7, E.POSE_I)
    for s in c.sets:
        bf = s.batch_fails()
        print(s.name, "failures per batch", bf)
        for b, f in enumerate(bf):
            nb = min(E.SD_T, s.n - b * E.SD_T)
            if nb >= E.SD_T - 1:
                assert f >= 35 and nb - f >= 35, (s.name, b, f)
        if s.n >= 2048:
            assert bf[0] != bf[1]
        if s.n > 4:                                         # interleaved: no run of one outcome longer than a few landmarks
            runs = np.diff(np.flatnonzero(np.diff(s.wantm.astype(int)) != 0))
            assert runs.max() <= 12, (s.name, runs.max())
    # a set's answer is the first landmarks of a longer set's answer: the oracle walks the landmarks in order, one draw per failure
    long = c.sets[-1]
    for s in c.sets:
        assert np.array_equal(s.wantm, long.wantm[:s.n]) and np.array_equal(s.want3.view(np.uint64), long.want3[:s.n].view(np.uint64))


def test_third_rigs_batch_recipe():
    for name in ("kitti", "euroc"):
        c = E.batch_call(name, (1025, 17), "G")
        assert [s.n for s in c.sets] == [1025, 17] and (c.rig.w, c.rig.h) == ((1241, 376) if name == "kitti" else (752, 480))
        bf = c.sets[0].batch_fails()
        print(c.name, "failures per batch", bf, "of the 17:", c.sets[1].fails)
        assert bf[0] >= 35 and E.SD_T - bf[0] >= 35 and 0 < c.sets[1].fails < 17
    assert E.rig("euroc").D1[0] != 0 and not E.rig("euroc").parallel and E.rig("kitti").w % 4 != 0


def test_overcount_recipe():
    c = E.overcount_call()
    assert c.cap == 96 and list(c.counts) == [96, 97, 1096, 40] and [s.n for s in c.sets] == [96, 96, 96, 40]
    print("overcount (n, failures)", [(s.n, s.fails) for s in c.sets])
    assert all(s.fails >= 10 and s.n - s.fails >= 10 for s in c.sets)


def test_extremes_recipe():
    c = E.extremes_call()
    allf, none, one_f, one_s, allf2 = c.sets
    print("extremes (n, failures)", [(s.name, s.n, s.fails) for s in c.sets])
    assert allf.n >= 70 and not allf.wantm.any() and not allf2.wantm.any()
    assert none.n >= 150 and none.wantm.all()
    assert (one_f.n, one_f.fails, one_s.n, one_s.fails) == (1, 1, 1, 0)
    for n in (1, 75, 1100):
        assert E.flat_set(n).fails == n


def test_range_recipe_brackets_the_triangulated_depths():
    for d in (1, 8, 40):
        sets = E.range_sets(d)
        big = sets["inf"]
        z = big.want3[big.wantm == 1, 2]
        print("d = %d: %d matched, z in [%.9g, %.9g]" % (d, len(z), z.min(), z.max()), {k: (s.rng, int(s.wantm.sum())) for k, s in sets.items()})
        assert abs(np.median(z) * d / (big.rig.fx * 0.05) - 1) < 0.05                      # depth = fx b / d
        assert not (z == z.astype(np.float32)).any()                                       # no z is a float: no range equals one
        assert set(sets) == set(E.RANGE_LABELS)
        assert np.float32(sets["below_min"].rng) < z.min() <= np.nextafter(np.float32(sets["below_min"].rng), np.float32(np.inf))
        assert np.nextafter(np.float32(sets["above_max"].rng), np.float32(-np.inf)) <= z.max() < np.float32(sets["above_max"].rng)
        assert np.nextafter(np.float32(sets["mid_down"].rng), np.float32(np.inf)) == np.float32(sets["mid_up"].rng)
        assert not sets["below_min"].wantm.any()
        for k, s in sets.items():
            if k != "below_min":
                assert s.wantm.any() and not s.wantm.all(), (d, k)                         # both mask values
        assert int(sets["mid_up"].wantm.sum()) == int(sets["mid_down"].wantm.sum()) + 1    # one ulp of the range moves one landmark
        assert int(sets["above_max"].wantm.sum()) == len(z)


def test_zero_and_negative_disparity_recipes():
    sets = E.zero_disparity_sets()
    a, b = sets["inf"], sets["1e30"]
    z = a.want3[a.wantm == 1, 2]
    print("d = 0: %d of %d pass; z > 1e6: %d, non-finite: %d, NaN: %d; smallest passing z %.6g" %
          (len(z), a.n, (z > 1e6).sum(), (~np.isfinite(z)).sum(), np.isnan(z).sum(), np.nanmin(z)))
    assert ((~np.isfinite(z)) | (z > 1e6)).sum() >= 1
    assert a.wantm.any() and not a.wantm.all()
    for k in range(3):                                      # exact, + 1 ulp, - 1 ulp
        assert (a.kind == k).sum() >= 50
    nan = a.kind == 3                                        # a NaN z passes `!(z < 0 || z > range)` under every range: mask 1, NaN point
    assert nan.sum() == 3 and a.wantm[nan].all() and b.wantm[nan].all() and np.isnan(a.want3[nan]).all() and np.isnan(z).sum() == 3
    zb = b.want3[b.wantm == 1, 2]
    assert not (zb > 1e30).any()
    s = E.negative_disparity_set()
    print("d = -8: %d of %d fail" % (s.fails, s.n))
    assert s.fails == s.n >= 150


def test_wrong_seed_recipes_populate_every_class():
    for name in ("d435", "kitti", "euroc"):
        c = E.wrong_seed_call(name)
        s = c.sets[0]
        pop = E.seed_populations(s)
        ok = {n: int(s.wantm[(s.kind == i) & (s.has == 1)].sum()) for i, n in enumerate(E.SEED_CLASSES)}
        print(name, "landmarks per class", pop, "of which the oracle triangulates", ok)
        assert not np.array_equal(s.pose7, E.POSE_I)
        flagged = s.has == 1
        for i, n in enumerate(E.SEED_CLASSES):
            m = flagged & (s.kind == i)
            if n == "z0":
                assert m.sum() == (6 if s.rig.parallel else 0) and (s.cam1_z[m] == 0).all()
                continue
            assert m.sum() >= 4, (name, n)
            twin = (~flagged) & (s.kind == i)                                       # the same pixels without a depth flag
            assert np.array_equal(s.p2d[m], s.p2d[twin])
        assert (s.cam1_z[flagged & (s.kind == 1)] < 0).all()
        tiny = s.cam1_z[flagged & (s.kind == 2)]
        assert ((np.abs(tiny) < 1e-6) & (tiny != 0)).all() and (tiny > 0).any() and (tiny < 0).any()
        if s.rig.parallel:
            assert np.isinf(s.seed_pix[flagged & (s.kind == 2)]).any()                   # a seed beyond float's range
        near = flagged & (s.kind >= 7)
        assert s.wantm[near].any() and not s.wantm[near].all()
        assert [t.n for t in c.sets] == [s.n, 17] and c.cap == s.n + 5


def test_oracle_is_a_function_of_its_inputs_and_the_generator():
    s = E.batch_call().sets[4]
    a3, am = s.oracle(O.Tracker(s.rig.cfg, 1))
    b3, bm = s.oracle(O.Tracker(s.rig.cfg, 1))
    assert a3.tobytes() == b3.tobytes() == s.want3.tobytes() and am.tobytes() == bm.tobytes() == s.wantm.tobytes()
    t = O.Tracker(s.rig.cfg, 1)                              # ... and of the generator: a second call on one tracker draws on
    s.oracle(t)
    c3, cm = s.oracle(t)
    assert np.array_equal(cm, am) and not np.array_equal(c3[am == 0], a3[am == 0]) and np.array_equal(c3[am == 1], a3[am == 1])


def test_dummy_depths_are_the_glibc_sequence_in_landmark_order():
    first = np.float32(0.3 + np.float64(np.float32(1804289383) / np.float32(2147483647 / 0.4)))      # rand() after srand(1) is 1804289383
    assert E.glibc_depths(3)[0] == np.float64(first)
    sets = list(E.batch_call().sets) + list(E.extremes_call().sets) + [E.wrong_seed_set("euroc"), E.negative_disparity_set(), E.flat_set(1100)]
    for s in sets:
        fail = np.flatnonzero(s.wantm == 0)
        z = s.want3[fail, 2]
        assert np.array_equal(z, E.glibc_depths(len(fail))), s.name
        if len(fail):
            assert z[0] == np.float64(first)
            r = s.rig
            u = s.p2u[fail].astype(np.float64)
            assert np.array_equal(s.want3[fail, 0], (u[:, 0] - r.cx) * z / r.fx) and np.array_equal(s.want3[fail, 1], (u[:, 1] - r.cy) * z / r.fy)


def test_carry_over_recipe():
    calls, want, draws = E.carry_calls()
    per_call = [[int((want[k][s][1] == 0).sum()) for k in range(4)] for s in range(4)]
    print("carry-over: failures per slot and call", per_call, "draws", draws)
    assert len(calls) == 4 and all(len(c.sets) == 4 for c in calls)
    for p in per_call:
        assert min(p) == 0 and max(p) >= 35
    assert len(set(draws)) == 4
    # a slot's dummy depths over the four calls are one glibc sequence
    for s in range(4):
        z = np.concatenate([want[k][s][0][want[k][s][1] == 0, 2] for k in range(4)])
        assert np.array_equal(z, E.glibc_depths(draws[s]))


def test_every_call_builds_under_its_name_and_packs_its_arrays():
    calls = [E.call(n) for n in E.CALLS]
    assert len(calls) >= 30 and len(E.extremes_call().sets) == 5
    a = E.overcount_call().arrays()
    assert a["p2d"].shape == (4, 96, 2) and a["count"].tolist() == [96, 97, 1096, 40] and not a["p2d"][3, 40:].any()
    moved = sum(not np.array_equal(c.sets[0].pose7, E.POSE_I) for c in calls)
    assert 2 * moved >= len(calls)                                                # the pose is not the identity in at least half of them
