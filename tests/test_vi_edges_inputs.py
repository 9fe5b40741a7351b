"""CPU: every recipe of tests/_vi_edges.py on the oracle alone, with the proof that it reaches the edge it is there for.  The evidence is
read from O.Tracker.vi_states() (the filter's queue, biases and flags) before and after the steps, the oracle's tracking state and its
pose_records: a recipe that drifts away from its edge fails here instead of testing nothing on the device.

The only floating tolerances are the norms of the bias estimates of `bias_clamps`, recovered by inverting the bias update in double:
1e-9 relative."""
import numpy as np
import pytest

import _vi_edges as E


def _last_vi(name, stream=0):
    return [e["vi"][stream] for e in E.expected(name) if stream in e["vi"]][-1]


def _frames(name):
    """[(Frame, expected entry)]"""
    ex = E.expected(name)
    return [(st, ex[i]) for i, st in E.frame_steps(name)]


def _untouched(e):
    """the frame left queue and biases as they were"""
    return np.array_equal(e["vi_before"]["rows"], e["vi"][0]["rows"]) and np.array_equal(e["vi_before"]["biases"], e["vi"][0]["biases"])


def _find_idx(rows, t):
    """viFindStateIdx on the stamps of a queue: (index, answer)"""
    later = rows[:, 0] - t > 0
    idx = len(rows) - 1
    while idx > 0 and later[idx]:
        idx -= 1
    return idx, len(rows) > 0 and idx > 0


def test_every_recipe_is_proven_here():
    tests = [n[5:] for n in globals() if n.startswith("test_")]
    for n in E.RECIPES:
        assert any(n == t or n.startswith(t + "_") for t in tests), n


# ---- IMU only -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", E.CHUNK_FORMS)
def test_chunks(form):
    """the filter initialises on its 31st pushed state (here the 31st sample); every form ends in the same rows, queue, biases and flags;
    the call that carries the 31st sample is where the two loops of imu_feed_dev meet"""
    name = "chunks_%s" % form
    ex = E.expected(name)
    rows = np.concatenate([e["rows"][0] for e in ex])
    base = np.concatenate([e["rows"][0] for e in E.expected("chunks_1")])
    assert len(rows) == E.N_CHUNKS and np.array_equal(rows, base)
    for k in ("rows", "biases", "flags"):
        assert np.array_equal(_last_vi(name)[k], _last_vi("chunks_1")[k]), k
    per_sample = E.expected("chunks_1")
    flips = [i for i, e in enumerate(per_sample) if e["vi"][0]["flags"][2]][0]
    assert flips == 30 and per_sample[30]["vi"][0]["flags"][3] == 31 and per_sample[29]["vi"][0]["flags"][3] == 30
    # identity rows while the attitude initialises (but the first one), moving rows afterwards
    assert np.all(base[1:31, 1:] == np.array([1, 0, 0, 0, 0, 0, 0, 0, 0, 0.0])) and np.all(np.any(base[31:, 5:] != 0, axis=1))
    if form != "out":
        sizes = [len(e["rows"][0]) for e in ex]
        first = np.cumsum([0] + sizes[:-1])
        inside = [f < 30 < f + n - 1 for f, n in zip(first, sizes)]        # the 31st sample neither opens nor closes its call
        assert any(inside) == (form in (32, 63, 64, 65, 150, E.N_CHUNKS)), (form, sizes[:3])
        assert any(f + n == 31 for f, n in zip(first, sizes)) == (form in (1, 31)) and any(f == 31 for f in first) == (form in (1, 31))


def test_gate():
    """of the three values around g + 0.3 only the double below passes; refused leading samples leave the queue empty with vi_first and
    has_imu set; failing samples during the initialisation and the propagation are pushed all the same"""
    passes = [bool((abs(-((E.G + 0.3) + d)) - E.G) < 0.3) for d in E.GATE_D]
    assert passes == [True, False, False]
    ex = E.expected("gate")
    steps = E.recipe("gate").steps
    lead = ex[0]
    assert len(lead["vi"][0]["rows"]) == 0 and lead["vi"][0]["flags"].tolist() == [1, 1, 0, 0]
    assert np.all(lead["rows"][0][:, 1:] == np.array([1, 0, 0, 0, 0, 0, 0, 0, 0, 0.0]))
    assert ex[1]["vi"][0]["flags"].tolist() == [1, 0, 0, 1]                  # the double below the threshold started the filter
    n = 1
    for i in (2, 3, 4):
        smp = steps[i].feeds[0][1]
        norms = np.linalg.norm(smp[:, 1:4], axis=1)
        assert np.sum(norms - E.G >= 0.3) == {2: 4, 3: 0, 4: 6}[i]                # failing samples among passing ones
        n += len(smp)
        assert ex[i]["vi"][0]["flags"][3] == n                                   # every one of them was pushed
    assert ex[2]["vi"][0]["flags"][2] == 0 and ex[3]["vi"][0]["flags"][2] == 1
    # "without feedback": the attitude a failing sample gives does not depend on its acceleration at all (gyro alone), so another failing
    # acceleration in its place leaves every attitude of the queue bit-equal; a passing sample's acceleration does enter
    smp = np.concatenate([st.feeds[0][1] for st in steps])

    def attitudes(s):
        o = E.O.Tracker(E.ocfg(), E.SEED)
        for r in s:
            o.imu(r[0], r[1:4], r[4:7])
        return o.vi_states()["rows"][:, 1:5]

    failing = np.nonzero(np.linalg.norm(smp[:, 1:4], axis=1) - E.G >= 0.3)[0]
    failing = failing[failing > 5]
    assert len(failing) == 10 and np.sum(failing < 5 + 1 + 12) == 4
    other = smp.copy()
    other[failing, 1:4] *= 1.3
    base = attitudes(smp)
    assert len(base) == len(smp) - 5 and np.array_equal(attitudes(other), base)
    for k in (11, 85):                                                          # a passing sample of the initialisation / the propagation
        assert k not in failing
        other = smp.copy()
        other[k, 1] += 0.05                                                     # (the feedback normalises: a scaled copy would not show)
        got = attitudes(other)
        assert np.array_equal(got[:k - 5], base[:k - 5]) and not np.array_equal(got[k - 5], base[k - 5])


@pytest.mark.parametrize("more", E.WRAP_MORE)
def test_wrap(more):
    """the queue reaches VI_QUEUE - 1 = 399 states and stays there; its oldest stamp is the expected one"""
    ex = E.expected("wrap_%d" % more)
    vi = _last_vi("wrap_%d" % more)
    smp = np.concatenate([st.feeds[0][1] for st in E.recipe("wrap_%d" % more).steps])
    assert len(smp) == 31 + more and len(vi["rows"]) == E.VI_QUEUE - 1 == 399 and vi["flags"][3] == 399
    assert np.array_equal(vi["rows"][:, 0], smp[-399:, 0]) and vi["rows"][0, 0] == smp[len(smp) - 399, 0]
    assert (len(smp) - 399 > 0) == (more > 368)                              # 368: the head has not moved yet
    if more == 850:
        assert len(ex[1]["rows"][0]) - E.IMU_OUT_CAP == 338 and len(smp) - E.IMU_OUT_CAP == 369


@pytest.mark.parametrize("which", ("zero", "epoch"))
def test_stamps(which):
    """dt = 0, dt < 0 and a gap of 1.5 s occur in the initialisation and in the propagation; at epoch stamps the float narrowing of dt sees
    other values than at small ones"""
    name = "stamps_" + which
    smp = np.concatenate([st.feeds[0][1] for st in E.recipe(name).steps])
    dt = np.diff(smp[:, 0])
    for lo, hi in ((0, 30), (30, len(dt))):
        d = dt[lo:hi]
        assert np.sum(d == 0) == 1 and np.sum(d < 0) == 1 and np.sum(d > 1.4) == 1, (lo, hi)
    vi = _last_vi(name)
    assert vi["flags"].tolist() == [1, 0, 1, len(smp)] and np.all(np.isfinite(vi["rows"]))
    if which == "epoch":
        z = np.concatenate([st.feeds[0][1] for st in E.recipe("stamps_zero").steps])
        assert smp[0, 0] > 1.6e9 and np.array_equal(smp[:, 1:], z[:, 1:])
        assert np.any(np.diff(z[:, 0]).astype(np.float32) != dt.astype(np.float32))
        assert not np.array_equal(vi["rows"][:, 1:], _last_vi("stamps_zero")["rows"][:, 1:])


def test_phases_65():
    """in the step that is staged as a whole: stream 0 refused, stream 1 initialised inside its chunk, stream 2 across the queue's wrap,
    stream 64 with a 65th sample on a full slot; stream 3 without a sample"""
    r = E.recipe("phases_65")
    ex = E.expected("phases_65")
    assert r.n_streams == 65 and r.lanes == 1 and r.fed == [0, 1, 2, 63, 64]
    s1 = {s: (smp, chunks) for s, smp, chunks in r.steps[1].feeds}
    assert ex[1]["vi"][0]["flags"].tolist() == [1, 1, 0, 0]
    assert ex[1]["vi"][1]["flags"].tolist() == [1, 0, 1, 45] and len(s1[1][0]) == 45 > 31
    assert ex[0]["vi"][2]["flags"][3] == 380 and ex[1]["vi"][2]["flags"][3] == 399 and ex[1]["vi"][2]["rows"][0, 0] == 22 / E.HZ
    assert ex[1]["vi"][2]["rows"][0, 0] > ex[0]["vi"][2]["rows"][0, 0]         # the head moved in this step
    assert len(s1[64][0]) == E.IMU_MAX + 1 and list(s1)[-1] == 64              # fed last: everyone else is staged when its slot overflows
    assert all(len(smp) <= E.IMU_MAX for s, (smp, _) in s1.items() if s != 64)
    assert ex[1]["vi"][63]["flags"].tolist() == [1, 0, 1, 60]
    assert ex[2]["vi"][0]["flags"].tolist() == [1, 0, 1, 35]                   # the refused stream starts afterwards


# ---- with frames --------------------------------------------------------------------------------------------------------------------------
def test_early_frames():
    fr = _frames("early_frames")
    assert [len(e["vi_before"]["rows"]) for _, e in fr[:4]] == [0, 1, 30, 31]
    assert [int(e["vi_before"]["flags"][2]) for _, e in fr[:4]] == [0, 0, 0, 1]
    assert all(e["vi_before"]["flags"][0] == 1 for _, e in fr)                 # has_imu from the refused sample on
    assert [e["out"]["state"] for _, e in fr] == [E.UNINIT] * 3 + [E.TRACKING] * 4
    assert all(_untouched(e) and len(e["rec"]) == 0 for _, e in fr[:3])
    assert fr[3][1]["out"]["new_keyframe"] and len(fr[3][1]["vi"][0]["rows"]) == 1   # the trigger cleared the queue
    assert not _untouched(fr[-1][1])                                           # a correction ran at the end


def test_refused_start():
    fr = _frames("refused_start")
    assert [e["vi_before"]["flags"].tolist() for _, e in fr[:3]] == [[1, 1, 0, 0]] * 3
    assert [e["out"]["state"] for _, e in fr] == [E.UNINIT] * 4 + [E.TRACKING] * 3
    assert fr[3][1]["vi_before"]["flags"].tolist() == [1, 0, 0, 20] and fr[4][1]["vi_before"]["flags"].tolist() == [1, 0, 1, 40]
    assert all(_untouched(e) and len(e["rec"]) == 0 for _, e in fr[:4]) and len(fr[4][1]["vi"][0]["rows"]) == 1


def test_one_state_ring():
    fr = _frames("one_state_ring")
    st, e = fr[1]
    assert e["vi_before"]["flags"].tolist() == [1, 0, 1, 1] and _find_idx(e["vi_before"]["rows"], st.t) == (0, False)
    assert e["out"]["state"] == E.TRACKING and _untouched(e)
    assert all(x["out"]["state"] == E.TRACKING for _, x in fr) and not _untouched(fr[2][1])


def test_no_sample_between():
    fr = _frames("no_sample_between")
    (sa, ea), (sb, eb), (sc, ec) = fr[2], fr[3], fr[4]
    rows = eb["vi_before"]["rows"]
    ia, ib = _find_idx(rows, sa.t), _find_idx(rows, sb.t)
    assert ia == ib and ia[1] and sb.t > sa.t                               # both stamps answer, with the same index
    assert _untouched(eb) and eb["out"]["state"] == E.TRACKING
    for e in (ea, ec):                                                          # the frames around it change queue and biases
        assert not np.array_equal(e["vi_before"]["biases"], e["vi"][0]["biases"]) and not np.array_equal(e["vi_before"]["rows"], e["vi"][0]["rows"])


def test_stamp_ties():
    fr = _frames("stamp_ties")
    assert all(e["out"]["state"] == E.TRACKING for _, e in fr)
    kinds = []
    for st, e in fr[1:]:
        ts = e["vi_before"]["rows"][:, 0]
        kinds.append("tie" if st.t in ts else "below" if np.nextafter(st.t, np.inf) in ts else
                     "above" if np.nextafter(st.t, -np.inf) in ts else "late" if st.t > ts[-1] + 0.5 / E.HZ else "?")
    assert kinds == ["tie", "below", "above", "late", "tie", "tie"], kinds
    st, e = fr[4]                                                               # the late frame: its samples arrive after it
    assert e["vi_before"]["rows"][-1, 0] == fr[3][1]["vi"][0]["rows"][-1, 0] and _untouched(e)
    later = E.expected("stamp_ties")[E.frame_steps("stamp_ties")[4][0] + 1]["rows"][0][:, 0]
    assert np.sum(later <= st.t) == 10 and np.sum(later > st.t) == 10


def test_slow_frames():
    fr = _frames("slow_frames")
    assert all(e["out"]["state"] == E.TRACKING for _, e in fr)
    dts = [b.t - a.t for (a, _), (b, _) in zip(fr[:-1], fr[1:])]
    assert 0.09999999999999998 in dts and 0.10000000000000003 in dts and sum(abs(d - 0.2) < 1e-9 for d in dts) == 2
    n_lt = n_ge = 0
    for (st, e), dt in zip(fr[2:], dts[1:]):                                    # (frame 1 follows the trigger: its t_last is the queue's index 0)
        bias_same = np.array_equal(e["vi_before"]["biases"], e["vi"][0]["biases"])
        moved = not np.array_equal(e["vi_before"]["rows"][:, 1:8], e["vi"][0]["rows"][:, 1:8])
        assert moved, st.idx                                                    # the queue is re-anchored on both sides of the rule
        assert bias_same == (not dt < 0.1), (st.idx, dt)
        n_lt += dt < 0.1
        n_ge += not dt < 0.1
    assert n_lt >= 3 and n_ge >= 5


@pytest.mark.parametrize("variant", list(E.WRAPPED_VARIANTS))
def test_wrapped_ring(variant):
    fr = _frames("wrapped_ring_" + variant)
    assert all(e["out"]["state"] == E.TRACKING for _, e in fr)
    (sp, _), (sg, eg), (sn, en) = fr[2], fr[3], fr[4]
    rows = eg["vi_before"]["rows"]
    assert len(rows) == 399 and sp.t < rows[0, 0] and _find_idx(rows, sp.t) == (0, False)      # older than the whole queue
    assert _find_idx(rows, sg.t) == (398, True) and _untouched(eg)                              # a guess, no correction
    rows = en["vi_before"]["rows"]
    want = 0 if variant == "idx0" else 1
    assert len(rows) == 399 and rows[want, 0] == sg.t and _find_idx(rows, sg.t) == (want, want > 0)
    assert _untouched(en) == (variant == "idx0")
    for _, e in fr[5:]:                                                         # corrections across the wrapped head
        assert len(e["vi_before"]["rows"]) == 399 and not _untouched(e)


def test_bias_clamps():
    """the estimates recovered from the bias update: above 0.5 both clamps act (norms 0.5 and 0.1), between 0.1 and 0.5 only the gyro
    clamp (norm 0.1), below 0.1 neither"""
    ex = E.expected("bias_clamps")
    est = {st.idx: E.bias_estimates(ex, i) for i, st in E.frame_steps("bias_clamps")}
    na = {k: np.linalg.norm(a) for k, (a, g) in est.items()}
    ng = {k: np.linalg.norm(g) for k, (a, g) in est.items()}
    assert na[4] == pytest.approx(0.5, rel=1e-9) and ng[4] == pytest.approx(0.1, rel=1e-9)       # offset 3 m/s^2: both clamps
    assert 0.1 < na[7] < 0.5 * (1 - 1e-9) and ng[7] == pytest.approx(0.1, rel=1e-9)              # offset 0.15: the gyro clamp alone
    assert na[10] < 0.1 * (1 - 1e-9) and ng[10] < 0.1 * (1 - 1e-9)                                # cancelled: neither
    # the unclamped gyro estimate of this scene is small (frame 10 shows it): at frame 7 the clamp scaled it UP to 0.1, which only the
    # test on the acc norm does
    assert ng[10] < 0.01


@pytest.mark.parametrize("stale", (False, True))
def test_fail_and_recover(stale):
    """both outcomes of a third failed frame.  Plain: the queue answers at frame 7, whose flat image has no corner (swapped back), and at
    frame 10, which re-initialises.  Stale: frame 7 is textured but its stamp is older than the whole queue, which cannot answer."""
    name = "fail_and_recover_stale" if stale else "fail_and_recover"
    fr = _frames(name)
    states = [e["out"]["state"] for _, e in fr]
    assert states == [1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1]
    st, e = fr[7]                                                               # a third failed frame, swapped back
    rows = e["vi_before"]["rows"]
    if stale:
        assert not st.flat and len(rows) == 399 and st.t < rows[0, 0] and _find_idx(rows, st.t) == (0, False)
    else:
        assert st.flat and _find_idx(rows, st.t) == (len(rows) - 1, True)
    assert e["out"]["state"] == E.TRACKFAIL and not e["out"]["new_keyframe"] and _untouched(e) and len(e["rec"]) == len(fr[6][1]["rec"])
    st, e = fr[10]                                                              # the next third one: re-initialised from the filter's state
    rows = e["vi_before"]["rows"]
    assert not st.flat and _find_idx(rows, st.t) == (len(rows) - 1, True)
    assert e["out"]["new_keyframe"] and _untouched(e) and len(e["rec"]) == len(fr[9][1]["rec"]) + 1
    assert not e["kf_imu"][0]                                                   # no trigger, and a keyframe of init_frame starts a new chain
    assert all(not x["out"]["new_keyframe"] for _, x in fr[4:10])
    assert not _untouched(fr[11][1])
