"""Inputs that drive the visual-inertial filter (flvis_amd/csrc/vi_motion.hpp, imu_feed_dev of track_kernels.hip, the staging and the
blocking flush of pipeline.cpp) to its ring, gate, chunk and frame-timing edges, with what the CPU oracle (ref::VIMOTION inside
ref::F2FTracking, oracle/ref_tracking.cpp) says after every step.  No GPU is needed here: tests/test_vi_edges_inputs.py proves on the
oracle alone that every recipe reaches the edge it is there for, tests/test_gpu_vi_edges.py runs the recipes on the device and compares
with what is built here, bit for bit.

A recipe is a list of steps:
  Imu(feeds)   feeds: [(stream, samples [n, 7] (t, acc, gyro in the FLVIS IMU frame), chunk sizes)]: the samples of each stream are
               handed over in calls of the given sizes, stream after stream, and nothing is read back before the step ends
  ImuOut(stream, samples)   the samples one by one through the call-for-call form (imu_feed_out), in the sensor frame
  Frame(t, idx, flat)       a stereo frame of the recipe's trajectory at stamp t (trajectory time t - t_add); flat: a grey image
expected(name) runs one oracle per stream through the steps and keeps, per step, what the device must show after it."""
import functools
import os
import tempfile

import numpy as np

import _oracle as O
from flvis_amd import synth

SID = 9                       # synth.Trajectory(9): the stream the whole-tracker tests use on this rig
VI_QUEUE = 400                # STATES_QUEUE_SIZE: the queue holds at most VI_QUEUE - 1 states
IMU_MAX = 64                  # samples a stream's staging slot holds
IMU_OUT_CAP = 512             # rows of the output ring behind imu_states()
HZ = synth.IMU_HZ
G = 9.81
BA = np.array([0.05, -0.03, 0.02])       # the bias and noise model of synth.imu_samples
BG = np.array([0.002, -0.001, 0.0015])
UNINIT, TRACKING, TRACKFAIL = 0, 1, 2


class Imu:
    def __init__(self, feeds):
        self.feeds = [(int(s), np.ascontiguousarray(smp, np.float64).reshape(-1, 7), tuple(int(c) for c in chunks)) for s, smp, chunks in feeds]
        for s, smp, chunks in self.feeds:
            assert sum(chunks) == len(smp) and all(c > 0 for c in chunks), (s, len(smp), chunks)


class ImuOut:
    def __init__(self, stream, samples):
        self.stream, self.samples = int(stream), np.ascontiguousarray(samples, np.float64).reshape(-1, 7)


class Frame:
    def __init__(self, t, idx, flat=False):
        self.t, self.idx, self.flat = float(t), int(idx), bool(flat)


class Recipe:
    def __init__(self, name, steps, n_streams=1, speed=1.0, t_add=0.0, lanes=None):
        self.name, self.steps, self.n_streams, self.speed, self.t_add, self.lanes = name, steps, n_streams, speed, t_add, lanes
        self.fed = sorted({f[0] for st in steps if isinstance(st, Imu) for f in st.feeds} | {st.stream for st in steps if isinstance(st, ImuOut)})
        self.has_frames = any(isinstance(st, Frame) for st in steps)
        assert not self.has_frames or n_streams == 1


def traj(speed=1.0):
    return synth.Trajectory(SID, speed=speed)


def sample_at(tr, k, t, noise_stream=SID):
    """one sample of synth.imu_samples' model at trajectory time t; k: the sample index that keys its noise"""
    R = tr.R_w_i(t)
    rng = np.random.default_rng((0x1A2B0000 + noise_stream) * 100003 + int(k))
    acc = R.T @ (tr.acc(t) + np.array([0.0, 0.0, -G])) + BA + rng.normal(0, 0.02, 3)
    gyro = tr.omega_body(t) + BG + rng.normal(0, 0.002, 3)
    return np.concatenate([[t], acc, gyro])


def samples(ks, speed=1.0, stamps=None, t_add=0.0, noise_stream=SID):
    """samples with indices ks at stamps k / HZ (or `stamps`, trajectory times), t_add added to the stamp after the evaluation"""
    tr = traj(speed)
    ks = list(ks)
    ts = [k / HZ for k in ks] if stamps is None else list(stamps)
    out = np.array([sample_at(tr, k, t, noise_stream) for k, t in zip(ks, ts)]).reshape(-1, 7)
    out[:, 0] += t_add
    return out


def chunked(n, c):
    """n samples in calls of c (the last one shorter)"""
    return tuple([c] * (n // c) + ([n % c] if n % c else []))


def to_sensor(r):
    """inverse of the EuRoC remap of imu_callback (acc = (-z, y, -x), gyro = (z, -y, x)): exact, signs and places only"""
    return [-r[3], r[2], -r[1]], [r[6], -r[5], r[4]]


@functools.lru_cache(maxsize=None)
def ocfg():
    p = os.path.join(tempfile.gettempdir(), "flvis_vi_edges_%d.yaml" % os.getpid())
    with open(p, "w") as f:
        f.write(synth.EUROC_LIKE_YAML)
    cfg = O.load_config(p)
    os.unlink(p)
    assert cfg.has_imu_type == 1 and cfg.cam_type == 1
    return cfg


@functools.lru_cache(maxsize=None)
def _renderer():
    return synth.Renderer("cpu", rig=synth.euroc_rig())


@functools.lru_cache(maxsize=256)
def images(speed, t_traj, idx, flat=False):
    """the stereo pair [2][H, W] uint8 of a frame (read-only)"""
    if flat:
        g = np.full((synth.euroc_rig().height, synth.euroc_rig().width), 128, np.uint8)
        g.setflags(write=False)
        return g, g
    i0, i1 = _renderer().stereo_frame([traj(speed)], t_traj, idx)
    a, b = i0[0].numpy().copy(), i1[0].numpy().copy()
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def frame_images(rcp, st):
    return images(rcp.speed, st.t - rcp.t_add, st.idx, st.flat)


SEED = 0xF1715


def _vi(o):
    v = o.vi_states()
    for a in v.values():
        a.setflags(write=False)
    return v


def run_oracle(rcp):
    """-> per step a dict: vi {stream: vi_states()}, rows {stream: [n, 11] output rows of the step}; a frame step also: out (state,
    new_keyframe, pose7, n_landmarks), lm (ids, flags), rec (pose_records), vi_before, and kf_imu / kf_imu_pos at a keyframe"""
    ref = {s: O.Tracker(ocfg(), SEED + s) for s in (rcp.fed if rcp.fed else [0])}
    res = []
    for st in rcp.steps:
        e = dict(rows={}, vi={})
        if isinstance(st, Frame):
            o = ref[0]
            e["vi_before"] = _vi(o)
            i0, i1 = frame_images(rcp, st)
            e["out"] = o.image(st.t, i0, i1)
            lm = o.landmarks()
            e["lm"] = dict(ids=lm["ids"], flags=lm["flags"])
            e["rec"] = o.pose_records()
            if e["out"]["new_keyframe"]:
                e["kf_imu"], e["kf_imu_pos"] = o.keyframe_imu(), o.keyframe_imu_pos()
            touched = [0]
        else:
            feeds = st.feeds if isinstance(st, Imu) else [(st.stream, st.samples, None)]
            for s, smp, _ in feeds:
                rows = [np.concatenate([[r[0]], ref[s].imu(r[0], r[1:4], r[4:7])]) for r in smp]
                e["rows"][s] = np.concatenate([e["rows"][s], rows]) if s in e["rows"] else np.array(rows).reshape(-1, 11)
            touched = sorted(e["rows"])
        for s in touched:
            e["vi"][s] = _vi(ref[s])
        res.append(e)
    return res


@functools.lru_cache(maxsize=None)
def recipe(name):
    r = RECIPES[name]()
    assert r.name == name
    return r


@functools.lru_cache(maxsize=None)
def expected(name):
    return run_oracle(recipe(name))


# ---- IMU only ---------------------------------------------------------------------------------------------------------------------------
N_CHUNKS = 500
CHUNK_FORMS = (1, 30, 31, 32, 63, 64, 65, 150, N_CHUNKS, "out")


def chunks_recipe(form):
    """500 samples in calls of `form` samples, every call a step; "out": one by one through imu_feed_out.  The filter initialises on its
    31st pushed state: a call boundary falls before it (30), on it (31), after it (32), and 63, 64, 65, 150 and 500 carry it inside
    a call, where the start-up loop and the register loop of imu_feed_dev meet"""
    smp = samples(range(1, N_CHUNKS + 1))
    name = "chunks_%s" % form
    if form == "out":
        return Recipe(name, [ImuOut(0, smp)])
    steps, i = [], 0
    for c in chunked(N_CHUNKS, form):
        steps.append(Imu([(0, smp[i:i + c], (c,))]))
        i += c
    return Recipe(name, steps)


def _exact_down(d):
    """a sample whose acceleration is (0, 0, -(g + 0.3 + d)) as a double: its norm is that double's magnitude, exactly"""
    return np.array([0.0, 0.0, -((G + 0.3) + d)])


GATE_D = (-np.spacing(G + 0.3), 0.0, np.spacing(G + 0.3))    # the doubles on either side of g + 0.3, and g + 0.3 itself


def gate_recipe():
    """the gate (|acc - bias| - g) < 0.3 with zero biases.  Steps: 0 leading samples that fail (scaled copies of real ones, then the
    exact threshold and the double above it) -- refused; 1 the double below the threshold -- starts the filter; 2 real samples with
    failing ones among them during the initialisation (the three threshold values and scaled copies); 3 the rest of the initialisation;
    4 propagation with failing samples among the real ones"""
    smp = samples(range(1, 141))
    k = 0

    def take(n):
        nonlocal k
        out = smp[k:k + n].copy()
        k += n
        return out

    lead = take(5)
    lead[0:3, 1:4] *= 1.05                     # |acc| ~ 10.3 > g + 0.3
    lead[3, 1:4] = _exact_down(GATE_D[1])
    lead[4, 1:4] = _exact_down(GATE_D[2])
    first = take(1)
    first[0, 1:4] = _exact_down(GATE_D[0])
    init_a = take(12)
    for j, d in zip((2, 3, 4), GATE_D):
        init_a[j, 1:4] = _exact_down(d)
    init_a[7:9, 1:4] *= 1.05
    init_b = take(30)                          # the 31st pushed state falls in here
    prop = take(60)
    for j, d in zip((10, 11, 12), GATE_D):
        prop[j, 1:4] = _exact_down(d)
    prop[30:33, 1:4] *= 1.05
    prop[45, 1:4] *= 1.2
    return Recipe("gate", [Imu([(0, x, (len(x),))]) for x in (lead, first, init_a, init_b, prop)])


WRAP_MORE = (368, 369, 370, 850)


def wrap_recipe(more):
    """31 samples initialise (31 states), `more` further ones: 368 leave 399 states with the head at 0, 369 and 370 move the head, 850
    wrap the 512-row output ring as well (881 rows, 369 dropped)"""
    smp = samples(range(1, 32 + more))
    return Recipe("wrap_%d" % more, [Imu([(0, smp[:31], (31,))]), Imu([(0, smp[31:], (more,))])])


def stamps_recipe(t_add):
    """a repeated stamp (dt = 0), a stamp that goes back (dt < 0) and a gap of 1.5 s, each once during the initialisation and once during
    the propagation; t_add = 1.6e9 repeats it at epoch-sized stamps, where (float)dt narrows differences of large doubles"""
    ks = list(range(1, 131))
    ts = [k / HZ for k in ks]
    for j in (10, 60):
        ts[j] = ts[j - 1]                      # repeated
    for j in (15, 70):
        ts[j] = ts[j - 1] - 0.003              # goes back
    for j in range(20, len(ts)):
        ts[j] += 1.5                           # gap in the initialisation
    for j in range(90, len(ts)):
        ts[j] += 1.5                           # gap in the propagation
    smp = samples(ks, stamps=ts, t_add=t_add)
    return Recipe("stamps_%s" % ("epoch" if t_add else "zero"), [Imu([(0, smp[i:i + 26], (len(smp[i:i + 26]),))]) for i in range(0, len(smp), 26)],
                  t_add=t_add)


def phases_65_recipe():
    """65 streams in one lane: k_imu_feed has two workgroups (streams 0 .. 63 and stream 64).  Step 0 brings stream 2 to 380 states
    (31 + 349) and stream 63 past its initialisation; step 1 stages, without a read-back, 20 refused samples on stream 0, 45 samples on
    stream 1 (initialised by the 31st), 40 on stream 2 (the queue fills at the 19th: the head moves), 20 on stream 63 and then 65 on
    stream 64, whose 65th finds the slot full: the blocking flush integrates every stream's staged samples; step 2 goes on with all
    five.  Stream 3 never gets a sample."""
    def smp(s, k0, n):
        return samples(range(k0, k0 + n), noise_stream=SID + s)

    refused = smp(0, 1, 20)
    refused[:, 1:4] *= 1.05
    s0 = Imu([(2, smp(2, 1, 380), (380,)), (63, smp(63, 1, 40), (40,))])
    s1 = Imu([(0, refused, (20,)), (1, smp(1, 1, 45), (45,)), (2, smp(2, 381, 40), (25, 15)), (63, smp(63, 41, 20), (20,)),
              (64, smp(64, 1, 65), (65,))])
    s2 = Imu([(64, smp(64, 66, 10), (10,)), (0, smp(0, 21, 35), (35,)), (1, smp(1, 46, 5), (5,)), (2, smp(2, 421, 5), (5,)),
              (63, smp(63, 61, 5), (5,))])
    return Recipe("phases_65", [s0, s1, s2], n_streams=65, lanes=1)


RECIPES = {}
for _f in CHUNK_FORMS:
    RECIPES["chunks_%s" % _f] = functools.partial(chunks_recipe, _f)
RECIPES["gate"] = gate_recipe
for _m in WRAP_MORE:
    RECIPES["wrap_%d" % _m] = functools.partial(wrap_recipe, _m)
RECIPES["stamps_zero"] = functools.partial(stamps_recipe, 0.0)
RECIPES["stamps_epoch"] = functools.partial(stamps_recipe, 1.6e9)
RECIPES["phases_65"] = phases_65_recipe
IMU_ONLY = tuple(RECIPES)


# ---- with frames: one stream in lockstep with the oracle ------------------------------------------------------------------------------------
def _ks(k0, k1, speed=1.0):
    """the samples k0 .. k1 (inclusive) of the recipe's trajectory as one step, handed over in one call"""
    return Imu([(0, samples(range(k0, k1 + 1), speed), (k1 - k0 + 1,))])


def _bad(step):
    """the step's samples scaled so that they fail the gate (|acc| ~ 10.3)"""
    (s, smp, chunks), = step.feeds
    smp = smp.copy()
    smp[:, 1:4] *= 1.05
    return Imu([(s, smp, chunks)])


def nominal(frames, speed=1.0, k_first=1, idx0=0):
    """frames: sample indices (stamps k / HZ) at which a frame arrives; each is preceded by the samples since the previous one"""
    steps, k_prev = [], k_first - 1
    for j, k in enumerate(frames):
        if k > k_prev:
            steps.append(_ks(k_prev + 1, k, speed))
        steps.append(Frame(k / HZ, idx0 + j))
        k_prev = max(k, k_prev)
    return steps


def early_frames_recipe():
    """frames while the queue holds 0 (one refused sample: has_imu is set), 1, 30 and 31 states; the 31st sets vi_initialized, the frame
    after it triggers and initialises; three Tracking frames follow"""
    steps = [_bad(_ks(1, 1)), Frame(0.006, 0), _ks(2, 2), Frame(0.011, 1), _ks(3, 31), Frame(0.156, 2), _ks(32, 32), Frame(0.161, 3)]
    steps += [_ks(33, 40), Frame(0.2, 4), _ks(41, 50), Frame(0.25, 5), _ks(51, 60), Frame(0.3, 6)]
    return Recipe("early_frames", steps)


def refused_start_recipe():
    """30 samples that all fail the gate, a frame after every 10: has_imu is set, the filter never starts, the frames are passed over;
    then normal samples: a frame at 20 states is still passed over, the one after the 31st state triggers"""
    steps = [_bad(_ks(1, 10)), Frame(0.05, 0), _bad(_ks(11, 20)), Frame(0.10, 1), _bad(_ks(21, 30)), Frame(0.15, 2)]
    steps += [_ks(31, 50), Frame(0.25, 3), _ks(51, 70), Frame(0.35, 4), _ks(71, 80), Frame(0.4, 5), _ks(81, 90), Frame(0.45, 6)]
    return Recipe("refused_start", steps)


def one_state_ring_recipe():
    """the frame after the trigger frame arrives with no sample in between: one state in the queue, viFindStateIdx answers false"""
    return Recipe("one_state_ring", nominal([40, 40])[:2] + [Frame(0.25, 1)] + nominal([60, 70, 80], k_first=41, idx0=2))


def no_sample_between_recipe():
    """frame 3 (stamp 0.3025) follows frame 2 (0.3) with no sample between them: idx_last == idx_curr"""
    steps = nominal([40, 50, 60]) + [Frame(0.3025, 3)] + nominal([70, 80, 90], k_first=61, idx0=4)
    return Recipe("no_sample_between", steps)


def stamp_ties_recipe():
    """Tracking frames at exactly a sample's stamp (frames 1, 5, 6), at the double below a sample's stamp (2), at the double above (3),
    and later than every sample fed so far (4: its samples arrive after it)"""
    steps = nominal([40, 50]) + [_ks(51, 60), Frame(np.nextafter(60 / HZ, -np.inf), 2), _ks(61, 70), Frame(np.nextafter(70 / HZ, np.inf), 3),
                                Frame(80 / HZ, 4), _ks(71, 90), Frame(90 / HZ, 5), _ks(91, 100), Frame(100 / HZ, 6)]
    return Recipe("stamp_ties", steps)


SLOW = 0.3
SLOW_FRAMES_J = (2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 14, 15)      # stamps j / 10


def slow_frames_recipe():
    """a slow trajectory with frames at j / 10: the differences of neighbouring stamps fall on both sides of 0.1, two are 0.2"""
    steps, k_prev = [], 0
    for i, j in enumerate(SLOW_FRAMES_J):
        k = 20 * j
        steps += [_ks(k_prev + 1, k, SLOW), Frame(j / 10.0, i)]
        k_prev = k
    return Recipe("slow_frames", steps, speed=SLOW)


CRAWL = 0.05
WRAPPED_VARIANTS = {"idx0": 398, "idx1": 397}


def wrapped_ring_recipe(variant):
    """frames 0 .. 2 nominal; 450 samples (dropped images), frame 3: the previous frame's stamp is older than the whole queue; then 398
    (idx0) or 397 (idx1) samples, frame 4: the previous frame's stamp is the queue's oldest / second oldest state; frames 5, 6 nominal"""
    n2 = WRAPPED_VARIANTS[variant]
    k3 = 60 + 450
    k4 = k3 + n2
    steps = nominal([40, 50, 60], CRAWL) + [_ks(61, k3, CRAWL), Frame(k3 / HZ, 3), _ks(k3 + 1, k4, CRAWL), Frame(k4 / HZ, 4)]
    steps += nominal([k4 + 10, k4 + 20], CRAWL, k_first=k4 + 1, idx0=5)
    return Recipe("wrapped_ring_%s" % variant, steps, speed=CRAWL)


# frame index -> the acceleration offset (body frame) added to the samples of the interval in front of that frame
BIAS_OFFSETS = {4: np.array([3.0, 0.0, 0.0]), 7: np.array([0.0, 0.15, 0.0]), 10: None}
BIAS_FRAMES = 13


def bias_clamps_recipe(cancel=None):
    """frames every 10 samples; the samples in front of frames 4 and 7 carry a constant acceleration offset, which the correction sees as
    half of it in the acc-bias estimate; `cancel`: the offset in front of frame 10, chosen (BIAS_CANCEL) to take that frame's estimate
    below 0.1"""
    steps = nominal([40 + 10 * f for f in range(BIAS_FRAMES)])
    offs = dict(BIAS_OFFSETS)
    offs[10] = cancel
    out = []
    for i, st in enumerate(steps):
        if isinstance(st, Imu) and isinstance(steps[i + 1], Frame) and offs.get(steps[i + 1].idx) is not None:
            (s, smp, chunks), = st.feeds
            smp = smp.copy()
            smp[:, 1:4] += offs[steps[i + 1].idx]
            st = Imu([(s, smp, chunks)])
        out.append(st)
    return Recipe("bias_clamps", out)


P3, P4 = 0.001, 0.001         # vifusion_para3 / 4 of synth.EUROC_LIKE_YAML


def bias_estimates(ex, i):
    """the (clamped) estimates of frame step i, recovered from the bias update b' = (1 - p3) b + p3 est (gyro: p4 est)"""
    b0, b1 = ex[i]["vi_before"]["biases"], ex[i]["vi"][0]["biases"]
    return (b1[:3] - (1 - P3) * b0[:3]) / P3, (b1[3:] - (1 - P3) * b0[3:]) / P4


def bias_cancel_search():
    """how BIAS_CANCEL was found: twice the negative of the estimate frame 10 gives without an offset (the estimate moves by about half
    the offset), refined on the oracle's own answer until the estimate is below 0.05"""
    off = np.zeros(3)
    for _ in range(3):
        r = bias_clamps_recipe(off)
        ex = run_oracle(r)
        i = [j for j, st in enumerate(r.steps) if isinstance(st, Frame) and st.idx == 10][0]
        est, _ = bias_estimates(ex, i)
        if np.linalg.norm(est) < 0.05:
            break
        off = off - 2.0 * est
    return off


BIAS_CANCEL = np.array([-0.092, 0.143, -0.164])      # bias_cancel_search(), rounded; test_vi_edges_inputs.py checks what it achieves


def fail_and_recover_recipe(stale=False):
    """frames 0 .. 2 track; 3 .. 7 are flat grey: two failures give TRACKFAIL (frame 4), frame 7 is the third failed frame and
    re-initialises on an image without a corner; texture returns with frame 8, frame 10 is the next third one and re-initialises from the
    filter's state at its stamp; frames 11, 12 track.
    stale: 410 samples arrive in front of frame 7 (the images lag the IMU by 2 s), frame 7 is textured and keeps its stamp 0.55, older than
    the whole queue: the queue cannot answer and the frame is swapped back; the later frames carry current stamps again"""
    if not stale:
        steps = nominal([40 + 10 * f for f in range(13)])
    else:
        steps = nominal([40 + 10 * f for f in range(7)]) + [_ks(101, 510), Frame(110 / HZ, 7)] + nominal([520 + 10 * f for f in range(5)], k_first=511, idx0=8)
    for st in steps:
        if isinstance(st, Frame) and 3 <= st.idx <= (6 if stale else 7):
            st.flat = True
    return Recipe("fail_and_recover_stale" if stale else "fail_and_recover", steps)


RECIPES["early_frames"] = early_frames_recipe
RECIPES["refused_start"] = refused_start_recipe
RECIPES["one_state_ring"] = one_state_ring_recipe
RECIPES["no_sample_between"] = no_sample_between_recipe
RECIPES["stamp_ties"] = stamp_ties_recipe
RECIPES["slow_frames"] = slow_frames_recipe
for _v in WRAPPED_VARIANTS:
    RECIPES["wrapped_ring_%s" % _v] = functools.partial(wrapped_ring_recipe, _v)
RECIPES["bias_clamps"] = lambda: bias_clamps_recipe(BIAS_CANCEL)
RECIPES["fail_and_recover"] = fail_and_recover_recipe
RECIPES["fail_and_recover_stale"] = functools.partial(fail_and_recover_recipe, True)
WITH_FRAMES = tuple(n for n in RECIPES if n not in IMU_ONLY)
RUN_STEPS = ("stamp_ties", "no_sample_between", "slow_frames")


def frame_steps(name):
    """[(step index, Frame)] of a recipe"""
    return [(i, st) for i, st in enumerate(recipe(name).steps) if isinstance(st, Frame)]
