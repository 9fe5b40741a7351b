"""GPU (-m gpu, MI355X): the visual-inertial filter at its ring, gate, chunk and frame-timing edges, bit for bit against the CPU oracle
(ref::VIMOTION inside ref::F2FTracking).  The recipes and what the oracle says after each of their steps come from tests/_vi_edges.py
(tests/test_vi_edges_inputs.py proves without a GPU that each recipe reaches its edge).

After every step: the output rows of imu_states() and the filter's queue, biases and flags (debug_vi_state); after every frame also
state, keyframe flag, pose, landmark ids and flags and pose_records; at every keyframe the preintegration the sample loop wrote back
(get_keyframe_imu, get_keyframe_imu_pos).  There is no tolerance anywhere (np.array_equal)."""
import ctypes as C

import numpy as np
import pytest

import _vi_edges as E

pytestmark = pytest.mark.gpu

IDENTITY_VI = dict(rows=np.zeros((0, 11)), biases=np.zeros(6), flags=np.array([0, 1, 0, 0], np.int32))   # a stream without a sample


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


def _cfg():
    """the oracle's config, byte for byte: both sides get the same numbers"""
    import flvis_amd
    o = E.ocfg()
    cfg = flvis_amd.FlvisCfg()
    assert C.sizeof(cfg) == C.sizeof(o)
    C.memmove(C.byref(cfg), C.byref(o), C.sizeof(o))
    return cfg


def _cuda(img):
    import torch
    return torch.tensor(img[None]).cuda()


def _tracker(ctx, rcp, traj_capacity=0):
    import flvis_amd
    return flvis_amd.Tracker(ctx, _cfg(), rcp.n_streams, seed_base=E.SEED, traj_capacity=traj_capacity)


def check_vi(trk, s, want, where):
    got = trk.debug_vi_state(s)
    assert got["flags"].tolist() == want["flags"].tolist(), (where, "flags (has_imu, vi_first, vi_initialized, vi_count)", s)
    assert got["rows"].shape == want["rows"].shape, (where, "queue length", s)
    bad = np.nonzero(np.any(got["rows"] != want["rows"], axis=1))[0]
    assert len(bad) == 0, (where, "stream %d: queue differs at %d of %d states, first at index %d" % (s, len(bad), len(want["rows"]), bad[0]),
                           got["rows"][bad[0]] - want["rows"][bad[0]])
    assert np.array_equal(got["biases"], want["biases"]), (where, "biases", s, got["biases"] - want["biases"])


def check_rows(trk, s, want, where):
    """the output rows since the previous fetch; more than the ring holds: the newest IMU_OUT_CAP, the others reported lost"""
    got, dropped = trk.imu_states(s, cap=E.IMU_OUT_CAP)
    lost = max(0, len(want) - E.IMU_OUT_CAP)
    assert dropped == lost and len(got) == len(want) - lost, (where, "rows of stream %d" % s, len(got), dropped, len(want))
    bad = np.nonzero(np.any(got != want[lost:], axis=1))[0]
    assert len(bad) == 0, (where, "stream %d: %d of %d rows differ, first %d" % (s, len(bad), len(got), bad[0]), got[bad[0]] - want[lost + bad[0]])


def check_frame(trk, got, e, where):
    want = e["out"]
    assert got["state"] == want["state"] and got["new_keyframe"] == want["new_keyframe"], (where, got["state"], want["state"])
    assert np.array_equal(got["pose7"], want["pose7"]), (where, got["pose7"] - want["pose7"])
    assert got["n_landmarks"] == want["n_landmarks"], (where, got["n_landmarks"], want["n_landmarks"])
    lm = trk.landmarks(0)
    assert np.array_equal(lm["ids"], e["lm"]["ids"]) and np.array_equal(lm["flags"], e["lm"]["flags"]), where
    rec = trk.pose_records(0)
    assert rec.shape == e["rec"].shape and np.array_equal(rec, e["rec"]), (where, "pose_records")
    if want["new_keyframe"]:
        gv, gdq, gdt = trk.get_keyframe_imu(0)
        wv, wdq, wdt = e["kf_imu"]
        assert gv == wv and gdt == wdt and np.array_equal(gdq, wdq), (where, "keyframe preintegration", gdq - wdq, gdt - wdt)
        gdp, gva = trk.get_keyframe_imu_pos(0)
        assert np.array_equal(gdp, e["kf_imu_pos"][0]) and np.array_equal(gva, e["kf_imu_pos"][1]), (where, "keyframe preintegration (position)")


def run_recipe(ctx, name, every_step=True, traj_capacity=0):
    """the recipe on the device, compared with the oracle after every step (every_step) or, for the samples, only after the next frame:
    the staged samples are then integrated by the frame's head kernel, as in production, not by a read-back's flush.  -> the tracker"""
    rcp, ex = E.recipe(name), E.expected(name)
    trk = _tracker(ctx, rcp, traj_capacity)
    watch = rcp.fed + ([3] if rcp.n_streams > 3 else [])
    vi = {s: IDENTITY_VI for s in watch}
    pending = {s: np.zeros((0, 11)) for s in watch}

    def compare(where):
        for s in watch:
            check_rows(trk, s, pending[s], where)
            pending[s] = np.zeros((0, 11))
            check_vi(trk, s, vi[s], where)

    for i, (st, e) in enumerate(zip(rcp.steps, ex)):
        where = "%s step %d" % (name, i)
        if isinstance(st, E.Imu):
            for s, smp, chunks in st.feeds:
                k = 0
                for c in chunks:
                    trk.imu_feed_flvis(s, smp[k:k + c])
                    k += c
        elif isinstance(st, E.ImuOut):
            for r, w in zip(st.samples, e["rows"][st.stream]):
                q, p, v = trk.imu_feed_out(st.stream, r[0], *E.to_sensor(r))
                assert np.array_equal(np.concatenate([q, p, v]), w[1:]), (where, r[0])
        else:
            i0, i1 = E.frame_images(rcp, st)
            got = trk.image_feed(_cuda(i0), _cuda(i1), [st.t], with_local_map=False)[0]
            check_frame(trk, got, e, where + " (frame %d)" % st.idx)
        for s, rows in e["rows"].items():
            pending[s] = np.concatenate([pending[s], rows])
        vi.update(e["vi"])
        if every_step or isinstance(st, E.Frame) or i == len(rcp.steps) - 1:
            compare(where)
    return trk


@pytest.mark.parametrize("name", [n for n in E.IMU_ONLY if n != "phases_65"])
def test_imu_only(ctx, name):
    """chunks_*: 500 samples in calls of 1 .. 500 and one by one through imu_feed_out (the call that carries the 31st sample runs both loops of
    imu_feed_dev); gate: the threshold and its neighbours, refused, during initialisation, during propagation; wrap_*: the queue at
    399 states with the head at 0 and moving, the 512-row output ring wrapped (all 11 columns of the rows kept); stamps_*: dt = 0,
    dt < 0, a 1.5 s gap, at small and at epoch-sized stamps"""
    run_recipe(ctx, name)


def test_phases_65(ctx, monkeypatch):
    """65 streams in one lane: two workgroups of k_imu_feed, streams in different phases in one launch, the blocking flush caused by
    stream 64's 65th sample with every other stream staged, stream 3 untouched"""
    monkeypatch.setenv("FLVIS_LANES", "1")
    run_recipe(ctx, "phases_65")


@pytest.mark.parametrize("every_step", (True, False), ids=("every_step", "at_frames"))
@pytest.mark.parametrize("name", E.WITH_FRAMES)
def test_with_frames(ctx, name, every_step):
    """one stream in lockstep with the oracle through early_frames, refused_start, one_state_ring, no_sample_between, stamp_ties,
    slow_frames, wrapped_ring_idx0 / idx1, bias_clamps, fail_and_recover and fail_and_recover_stale"""
    run_recipe(ctx, name, every_step)


def _final(trk, n_frames):
    lm = trk.landmarks(0)
    vi = trk.debug_vi_state(0)
    return dict(rows=vi["rows"], biases=vi["biases"], flags=vi["flags"], traj=trk.trajectory(0, 0, n_frames), ids=lm["ids"], lm_flags=lm["flags"],
                p2d=lm["p2d"], p3w=lm["p3w"], rec=trk.pose_records(0))


@pytest.mark.parametrize("name", E.RUN_STEPS)
def test_run_steps_batches(ctx, name):
    """the recipe's frames with their samples through flvis_run_steps, as one batch and as batches of 1, 5 and the rest: the same queue,
    biases, trajectory rows, landmarks and pose_records as the frame-by-frame run (which equals the oracle)"""
    rcp = E.recipe(name)
    frames = E.frame_steps(name)
    base = _final(run_recipe(ctx, name, every_step=False, traj_capacity=len(frames)), len(frames))
    assert np.array_equal(base["rows"], E.expected(name)[-1]["vi"][0]["rows"])
    steps, keep, smp = [], [], np.zeros((0, 7))
    for st in rcp.steps:
        if isinstance(st, E.Imu):
            smp = np.concatenate([smp] + [f[1] for f in st.feeds])
            continue
        assert len(smp) <= E.IMU_MAX
        i0, i1 = E.frame_images(rcp, st)
        buf = np.zeros((1, max(len(smp), 1), 7))
        buf[0, :len(smp)] = smp
        steps.append((_cuda(i0), _cuda(i1), [st.t], np.array([len(smp)], np.int32), buf))
        smp = np.zeros((0, 7))
    assert len(smp) == 0 and len(steps) == len(frames) > 6
    for split in ((len(steps),), (1, 5, len(steps) - 6)):
        trk = _tracker(ctx, rcp, traj_capacity=len(frames))
        k = 0
        for n in split:
            trk.run_steps(steps[k:k + n], with_local_map=False)
            k += n
        ctx.synchronize()
        got = _final(trk, len(frames))
        for key in base:
            assert np.array_equal(got[key], base[key]), (name, split, key)
