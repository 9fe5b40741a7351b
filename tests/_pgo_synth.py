"""Synthetic loop-closure problems for the pose-graph optimisation (pattern of g2o's examples/sphere: a trajectory that returns to
its start, odometry with drift, one verified loop)."""
import numpy as np

import _geom as G


def inv7(p):
    R, t = G.pose7_to_Rt(p)
    return G.pose7(R.T, -R.T @ t)


def mul7(a, b):
    Ra, ta = G.pose7_to_Rt(a)
    Rb, tb = G.pose7_to_Rt(b)
    return G.pose7(Ra @ Rb, ta + Ra @ tb)


def make_loop(seed, n_kf=70, drift=(0.02, 0.004), loop_noise=(0.002, 0.001), extra_loops=0, radius=3.0):
    """Keyframes on a circle (the camera returns to its start).  Returns ground-truth T_c_w, drifted T_c_w (what the tracker
    produced), the loop list [(earlier, later)] and the verified relative poses T_later_earlier (what isLoopClosureKF yields)."""
    rng = np.random.default_rng(seed)
    gt = []
    for k in range(n_kf):
        a = 2 * np.pi * k / (n_kf - 4)                      # slightly more than one revolution
        c = np.array([radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(3 * a)])
        R_wc = G.rodrigues(np.array([0.0, 0.0, a + np.pi / 2])) @ G.rodrigues(np.array([0.1 * np.sin(a), 0.05, 0.0]))
        gt.append(G.pose7(R_wc.T, -R_wc.T @ c))            # T_c_w
    # odometry = true relative motion + noise, accumulated
    est = [gt[0].copy()]
    for k in range(1, n_kf):
        rel = mul7(gt[k], inv7(gt[k - 1]))                  # T_k_(k-1)
        R, t = G.pose7_to_Rt(rel)
        R = G.rodrigues(rng.normal(0, drift[1], 3)) @ R
        t = t + rng.normal(0, drift[0], 3)
        est.append(mul7(G.pose7(R, t), est[-1]))
    loops = [(2, n_kf - 1)]
    for e in range(extra_loops):
        loops.append((6 + 5 * e, n_kf - 8 - 3 * e))
    loop_poses = []
    for a, b in loops:
        rel = mul7(gt[b], inv7(gt[a]))                      # T_b_a (se_ji: from the earlier keyframe's camera to the later one's)
        R, t = G.pose7_to_Rt(rel)
        loop_poses.append(G.pose7(G.rodrigues(rng.normal(0, loop_noise[1], 3)) @ R, t + rng.normal(0, loop_noise[0], 3)))
    return dict(gt=np.array(gt), est=np.array(est), loops=np.array(loops, np.int32), loop_poses=np.array(loop_poses))


SMALL_DRIFT = (0.004, 0.0008)                               # for the long trajectories: converges in 6 - 9 iterations at n = 1500
LOOP_NOISE = (0.002, 0.001)


def loop_pose(case, a, b, loop_noise=None, rng=None):
    """The relative pose T_b_a a verified loop (a, b) of a make_loop case carries: the true one from `gt`, with noise (translation
    sigma [m], rotation sigma [rad]) when `loop_noise` and a generator are given.  a > b is allowed."""
    rel = mul7(case["gt"][b], inv7(case["gt"][a]))
    if loop_noise is None:
        return rel
    R, t = G.pose7_to_Rt(rel)
    return G.pose7(G.rodrigues(rng.normal(0, loop_noise[1], 3)) @ R, t + rng.normal(0, loop_noise[0], 3))


def _graph(base, loops, seed, pose_of=None):
    """a pose graph on the trajectory `base`: every loop carries its noisy true pose (or that of the pair pose_of[k] instead); a loop
    listed twice carries the same pose twice"""
    rng = np.random.default_rng(seed)
    poses, seen = [], {}
    for k, (a, b) in enumerate(loops):
        if (a, b) not in seen:
            seen[(a, b)] = loop_pose(base, *((pose_of or {}).get(k, (a, b))), loop_noise=LOOP_NOISE, rng=rng)
        poses.append(seen[(a, b)])
    return dict(gt=base["gt"], est=base["est"], present=np.ones(len(base["est"]), np.uint8),
                loops=np.array(loops, np.int32).reshape(-1, 2), loop_poses=np.array(poses).reshape(-1, 7))


_EDGE_CASES = {}


def edge_case(name):
    """The pose graphs at the size and topology edges of the optimisation, by name -> dict(gt, est, present, loops, loop_poses).
    The dicts are cached: callers must not write into them.

    big-N           one loop (2, N - 1) on N keyframes (N > 256: more vertices than the workgroup has threads)
    nested-N        loops (2, N-1), (10, N-20), (N/4, 3N/4), (N/3, N/3+40): three wide block rows, nested
    nested-absent   nested-300 without the keyframes next to the loop ends N/4 and 3N/4 and without a run of four (150..153)
    kf0             loop (0, 119): kf_prev == 0
    chain           loops (1, 5), (5, 100): keyframe 5 is the later end of one loop and the earlier end of the next
    gauge-free      loops (30, 10), (10, 100): kf_prev = 10 is first named as a later end, so no vertex is fixed
    gap5 / gap4     make_loop(4, n_kf=120) without keyframes 40..44 (the odometry chain is cut) / 40..43 (one edge bridges the gap)
    adjacent+duplicate   loops (2, 119), (50, 52), (2, 119): a loop on an existing odometry block, the same loop twice
    tiny-B          one loop (10, B), B = 11, 12, 16, 17: graphs of 2, 3, 7, 8 vertices (below, at and above the 5-neighbour band)
    false-loop      loops (2, 119), (20, 80), the second with the pose of (20, 50): Cauchy weights far from 1, many rejected trials
    bfs-order       loops (2, 119), (97, 104): the initial guess reaches 104 (from 119, downwards) before 97, so 97 is queued first
                    only if neighbours are visited in ascending index, and 98 then hangs on 97 -- in edge order the guess moves by 0.1 m
    out-of-window   loops (5, 40), (50, 10): keyframe 50 lies outside min(earlier) .. max(later) and has no vertex -> must not run
    self-loop       loops (2, 119), (30, 30) -> must not run
    no-loops        120 keyframes, no loop -> does not run"""
    if name in _EDGE_CASES:
        return _EDGE_CASES[name]
    kind, _, arg = name.partition("-")
    if kind in ("big", "nested") and arg.isdigit():
        N = int(arg)
        base = make_loop(N, n_kf=N, drift=SMALL_DRIFT)
        c = dict(gt=base["gt"], est=base["est"], present=np.ones(N, np.uint8), loops=base["loops"], loop_poses=base["loop_poses"])
        if kind == "nested":
            more = _graph(base, [(10, N - 20), (N // 4, 3 * N // 4), (N // 3, N // 3 + 40)], N + 1)
            c["loops"] = np.concatenate([c["loops"], more["loops"]])
            c["loop_poses"] = np.concatenate([c["loop_poses"], more["loop_poses"]])
    elif name == "nested-absent":
        c = dict(edge_case("nested-300"))
        c["present"] = c["present"].copy()
        c["present"][[300 // 4 + 1, 3 * 300 // 4 - 1, 150, 151, 152, 153]] = 0
    elif name == "kf0":
        c = _graph(make_loop(21, n_kf=120), [(0, 119)], 121)
    elif name == "chain":
        c = _graph(make_loop(22, n_kf=120), [(1, 5), (5, 100)], 122)
    elif name == "gauge-free":
        c = _graph(make_loop(23, n_kf=120), [(30, 10), (10, 100)], 123)
    elif name in ("gap5", "gap4"):
        base = make_loop(4, n_kf=120)
        c = dict(gt=base["gt"], est=base["est"], present=np.ones(120, np.uint8), loops=base["loops"], loop_poses=base["loop_poses"])
        c["present"][40:(45 if name == "gap5" else 44)] = 0
    elif name == "adjacent+duplicate":
        c = _graph(make_loop(24, n_kf=120), [(2, 119), (50, 52), (2, 119)], 124)
    elif kind == "tiny":
        c = _graph(make_loop(25, n_kf=40), [(10, int(arg))], 125)
    elif name == "false-loop":
        c = _graph(make_loop(26, n_kf=120), [(2, 119), (20, 80)], 126, pose_of={1: (20, 50)})
    elif name == "bfs-order":
        c = _graph(make_loop(30, n_kf=120), [(2, 119), (97, 104)], 130)
    elif name == "out-of-window":
        c = _graph(make_loop(27, n_kf=120), [(5, 40), (50, 10)], 127)
    elif name == "self-loop":
        c = _graph(make_loop(28, n_kf=120), [(2, 119), (30, 30)], 128)
    elif name == "no-loops":
        c = _graph(make_loop(29, n_kf=120), [], 129)
    else:
        raise KeyError(name)
    _EDGE_CASES[name] = c
    return c


def centre_error(T_c_w, gt, idx):
    """camera-centre distance between estimate and ground truth after aligning at keyframe idx[0]"""
    def centre(p):
        R, t = G.pose7_to_Rt(p)
        return -R.T @ t
    return np.array([np.linalg.norm(centre(T_c_w[i]) - centre(gt[i])) for i in idx])


def loop_gap(T_c_w, gt, a, b):
    """how far the relative pose between keyframes a and b is from the true one: (translation [m], rotation [rad])"""
    rel, rel_gt = mul7(T_c_w[b], inv7(T_c_w[a])), mul7(gt[b], inv7(gt[a]))
    d = mul7(rel, inv7(rel_gt))
    R, t = G.pose7_to_Rt(d)
    return np.linalg.norm(t), np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
