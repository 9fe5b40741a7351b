"""The co-visibility patterns of tests/_ba_synth.py (the capacity-edge tests of the local-map BA are built on them): their structure, the
unchanged default path, and the oracle's window BA on each of them."""
import hashlib

import numpy as np
import pytest

import _ba_synth as B
import _oracle as O


def _digest(seq):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(seq["Pw"]).tobytes())
    for R, t in seq["gt"]:
        h.update(R.tobytes())
        h.update(t.tobytes())
    for kf in seq["kfs"]:
        h.update(np.int64(kf["frame_id"]).tobytes())
        for k in ("pose7", "lm_id", "lm_2d", "lm_3d", "outlier"):
            h.update(np.ascontiguousarray(kf[k]).tobytes())
    return h.hexdigest()[:16]


def test_default_sequences_are_unchanged():
    """the default path draws exactly what it drew before the patterns existed (every existing local-map test runs on it)"""
    assert _digest(B.make_sequence(11, n_kf=14, n_lm=260, outlier_frac=0.03)) == "97512550b39a9180"
    assert _digest(B.make_sequence(5)) == "880d6af973b97e18"
    with pytest.raises(ValueError):
        B.make_sequence(5, lm_per_kf=100)


@pytest.mark.parametrize("covis", B.COVIS)
def test_pattern_structure(covis):
    m, n_kf = 90, 9
    seq = B.make_sequence(3, n_kf=n_kf, lm_per_kf=m, covis=covis, outlier_kfs=(4,), outlier_frac=0.0)
    kfs = seq["kfs"]
    views = {}
    for k, kf in enumerate(kfs):
        assert len(kf["lm_id"]) == m and len(np.unique(kf["lm_id"])) == m
        assert np.array_equal(kf["lm_id"], kf["idx"] + 100)
        assert kf["outlier"].all() == (k == 4) and kf["outlier"].any() == (k == 4)
        for i in kf["idx"]:
            views.setdefault(int(i), []).append(k)
        # inliers are the projections of the pool's points (pixel noise 0.5)
        R, t = seq["gt"][k]
        uv = B.G.project(R, t, seq["Pw"][kf["idx"]], B.K4)
        err = np.abs(uv - kf["lm_2d"]).max(1)
        assert (err[~kf["outlier"]] < 4.0).all()
    counts = np.array([len(v) for v in views.values()])
    if covis == "dense":
        assert (counts == n_kf).all()
    elif covis == "sparse":
        assert set(counts) == {1, 2}
        assert all(v == list(range(v[0], v[0] + len(v))) for v in views.values())  # consecutive keyframes
    else:
        core = [i for i in views if i < m // 2]
        assert len(core) == m // 2 and all(len(views[i]) == n_kf for i in core)
        assert set(len(views[i]) for i in views if i >= m // 2) == {1, 2}
    assert B.window_size_of(kfs, 0, n_kf) == (len(views), m * n_kf)


def test_per_keyframe_counts():
    ms = [819] * 9 + [821, 820]
    seq = B.make_sequence(1, n_kf=len(ms), lm_per_kf=ms, covis="dense")
    assert [len(kf["lm_id"]) for kf in seq["kfs"]] == ms
    assert B.window_size_of(seq["kfs"], 0, 10) == (821, 8192)
    assert B.window_size_of(seq["kfs"], 1, 10) == (821, 8193)
    with pytest.raises(ValueError):
        B.make_sequence(1, n_kf=2, lm_per_kf=[B.KF_MAXLM + 1] * 2, covis="dense")


@pytest.mark.parametrize("covis", B.COVIS)
def test_oracle_window_on_patterns(covis):
    """the oracle's window BA on each pattern: the newest keyframe's Huber cost (numpy, from the outputs) drops below its cost at the
    pushed state, and (where landmarks have more than two views) most gross outliers of the outlier keyframe are culled"""
    W = 5
    seq = B.make_sequence(8, n_kf=W + 3, lm_per_kf=80, covis=covis, outlier_kfs=(W + 1,), outlier_frac=0.0, pix_sigma=0.3)
    ref = O.LocalMap(W, B.K4)
    produced = 0
    for k, kf in enumerate(seq["kfs"]):
        r = ref.push(kf["frame_id"], kf["pose7"], kf["lm_id"], kf["lm_2d"], kf["lm_3d"])
        assert (r is None) == (k < W - 1), k
        if r is None:
            continue
        produced += 1
        if k == W + 1 and covis != "sparse":  # (one or two views fit a gross outlier: sparse windows keep many of them)
            assert len(set(r["outlier_id"].tolist()) & set(kf["lm_id"].tolist())) > len(kf["lm_id"]) // 2
        if len(r["lm_id"]) and k != W + 1:
            pos = {int(i): j for j, i in enumerate(kf["lm_id"])}
            c, n = B.huber_cost(r["pose7"], r["lm_id"], r["lm_3d"], kf, B.K4, r["outlier_id"])
            c0, n0 = B.huber_cost(kf["pose7"], r["lm_id"], kf["lm_3d"][[pos[int(i)] for i in r["lm_id"]]], kf, B.K4, r["outlier_id"])
            assert n == n0 > 0 and c < 0.1 * c0, (k, c, c0)
    assert produced == 4
