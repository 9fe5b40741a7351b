"""Test helper: the keyframe log (flvis_keyframe_log_*, include/flvis_hip.h) restated in numpy.

A stream's history is the list of what a per-frame caller sees: one item per frame the stream was fed, the flvis/KeyFrame message
(the dict of Tracker.keyframe_msg) when the frame became a keyframe, else None.  `record` is the device log after those frames at a
capacity: a prefix of the messages in order; the first keyframe that does not fit ends it, and it and every later one count as dropped.
`rounds` is the order in which flvis_loop_closer_add_logged drains the logs of several streams."""
import numpy as np

FIELDS = ("frame_id", "command", "stamp", "pose7", "lm_id", "lm_2d", "lm_3d", "img0", "img1")


def record(history, capacity):
    """-> dict(entries: the logged messages, dropped: keyframes not recorded)"""
    entries, dropped = [], 0
    for msg in history:
        if msg is None:
            continue
        if dropped or len(entries) >= capacity:
            dropped += 1
            continue
        entries.append(msg)
    return dict(entries=entries, dropped=dropped)


def rounds(logged):
    """logged[s] = entries of stream s -> per round r the streams that have an r-th entry, in stream order"""
    return [[s for s, n in enumerate(logged) if n > r] for r in range(max(list(logged) + [0]))]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1) if a.dtype.kind == "f" else a.reshape(-1)


def differences(a, b):
    """the fields in which two messages differ, floats compared by their bits ([]: the same message)"""
    bad = []
    for k in FIELDS:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(_bits(x), _bits(y)):
                bad.append(k)
        elif isinstance(x, float):
            if np.float64(x).tobytes() != np.float64(y).tobytes():
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad


def fake_msg(k, n_lm=3, shape=(4, 6)):
    """a hand-made message, distinct for every k"""
    rng = np.random.default_rng(100 + k)
    return dict(frame_id=10 + 3 * k, command=0, stamp=0.05 * k, pose7=rng.normal(size=7), lm_id=np.arange(n_lm, dtype=np.int64) + 100 * k,
                lm_2d=rng.normal(size=(n_lm, 2)), lm_3d=rng.normal(size=(n_lm, 3)), img0=rng.integers(0, 256, shape).astype(np.uint8),
                img1=rng.integers(0, 256, shape).astype(np.uint8))
