"""Test helper: merging sequences' maps (flvis_loop_closer_merge) stated with the pieces the pose-graph tests already have.

A merge case is ONE ground-truth tour (tests/_pgo_synth.make_loop: the circle depends on the keyframe count alone) that several units
drove: every sequence is a drifted copy with a seed of its own, cut to the keyframes the unit stored, and every sequence but the first
(the anchor) lives in a world frame of its own -- its poses are moved by a fixed rigid transform, metres away from the anchor's.  Links
between keyframes of different sequences carry the true relative pose with _pgo_synth.LOOP_NOISE, as a verified localize_in candidate
would.

The joint graph is the reference's graph rule on the virtual sequence V = [a | 5 absent | b | 5 absent | c ...] (include/flvis_hip.h):
`assemble` builds V's rows, present flags and loop list from per-sequence poses, the sequences' own loops and the links, in the form
tests/test_oracle_pgo.pgo_case takes; `apply` turns an optimised V (and the drift of its last vertex) into what the closer must hold per
sequence afterwards."""
import numpy as np

import _geom as G
import _pgo_synth as PS

GAP = 5                                                     # absent rows between two sequences: the odometry edges reach five keyframes
# the frames of the non-anchor maps (T_world_anchor-world): 6.6 m and 7.3 m away, tens of degrees turned
WORLDS = [G.pose7(G.rodrigues(np.array([0.1, -0.2, 0.7])), np.array([5.0, -4.0, 1.5])),
          G.pose7(G.rodrigues(np.array([-0.3, 0.1, -1.1])), np.array([-3.0, 6.0, -2.0]))]


def assemble(poses, own_loops, links):
    """poses: per sequence [n, 7] T_c_w; own_loops: per sequence (ids [k, 2], poses [k, 7]) in recorded order; links: dicts seq_from /
    kf_from / seq_to / kf_to / pose with seq_* indices INTO `poses` (group positions).  -> dict(est, present, loops, loop_poses, offsets)"""
    rows, present, offsets = [], [], []
    for k, P in enumerate(poses):
        if k:
            rows.append(np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (GAP, 1)))
            present.append(np.zeros(GAP, np.uint8))
        offsets.append(sum(len(r) for r in rows))
        rows.append(np.asarray(P, np.float64).reshape(-1, 7))
        present.append(np.ones(len(P), np.uint8))
    loops, lposes = [], []
    for k, (ids, lp) in enumerate(own_loops):
        for (a, b), p in zip(np.asarray(ids).reshape(-1, 2), np.asarray(lp).reshape(-1, 7)):
            loops.append((offsets[k] + int(a), offsets[k] + int(b)))
            lposes.append(np.asarray(p, np.float64))
    for l in links:
        loops.append((offsets[l["seq_from"]] + int(l["kf_from"]), offsets[l["seq_to"]] + int(l["kf_to"])))
        p = np.asarray(l["pose"], np.float64).copy()
        p[3:] /= float(np.sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]))       # as the call normalises it: this sum, in this order
        lposes.append(p)
    return dict(est=np.concatenate(rows), present=np.concatenate(present), loops=np.array(loops, np.int32).reshape(-1, 2),
                loop_poses=np.array(lposes).reshape(-1, 7), offsets=offsets)


def last_vertices(V, counts):
    """v_s per sequence: its last keyframe, in the last sequence the one at max(later); and the anchor's first vertex min(earlier)"""
    lo, hi = int(V["loops"][:, 0].min()), int(V["loops"][:, 1].max())
    v = [n - 1 for n in counts]
    v[-1] = hi - V["offsets"][-1]
    return lo, v


def apply(V, counts, T_opt):
    """what the sequences hold after the merge, from the optimised rows T_opt of V: vertex rows as optimised, the rows behind v_s times
    drift_s = inv(old(v_s)) * new(v_s).  -> (per-sequence poses, per-sequence drift)"""
    lo, vs = last_vertices(V, counts)
    out, drifts = [], []
    for k, n in enumerate(counts):
        o = V["offsets"][k]
        old, new = V["est"][o:o + n], T_opt[o:o + n].copy()
        d = PS.mul7(PS.inv7(old[vs[k]]), new[vs[k]])
        for j in range(vs[k] + 1, n):
            new[j] = PS.mul7(old[j], d)
        out.append(new)
        drifts.append(d)
    return out, drifts


def _sequence(n_tour, seed, first, count, world, drift, own_loop, rng):
    """`count` keyframes from `first` on of a drifted copy (seed) of the n_tour-keyframe tour, in the frame `world` (None: the tour's)"""
    base = PS.make_loop(seed, n_kf=n_tour, drift=drift)
    gt, est = base["gt"][first:first + count], base["est"][first:first + count]
    if world is not None:                                    # p_world' = W p_world: T_c_w' = T_c_w * W^-1
        Wi = PS.inv7(world)
        est = np.array([PS.mul7(p, Wi) for p in est])
    ids, lp = np.zeros((0, 2), np.int32), np.zeros((0, 7))
    if own_loop is not None:                                 # a loop the sequence closed itself: the pose is frame-free (a relative one)
        a, b = own_loop
        ids = np.array([[a, b]], np.int32)
        lp = np.array([PS.loop_pose(dict(gt=gt), a, b, loop_noise=PS.LOOP_NOISE, rng=rng)])
    return dict(gt=gt, est=est, loops=ids, loop_poses=lp)


def _link(seqs, sf, kf, st, kt, rng):
    rel = PS.mul7(seqs[st]["gt"][kt], PS.inv7(seqs[sf]["gt"][kf]))                  # T_to_from from the ground truth
    R, t = G.pose7_to_Rt(rel)
    noisy = G.pose7(G.rodrigues(rng.normal(0, PS.LOOP_NOISE[1], 3)) @ R, t + rng.normal(0, PS.LOOP_NOISE[0], 3))
    return dict(seq_from=sf, kf_from=kf, seq_to=st, kf_to=kt, pose=noisy)


# name -> (tour keyframes, drift, [(seed, first, count, own loop)], [(from, kf, to, kf)])
_SPEC = {
    "pair-12": (12, (0.02, 0.004), [(41, 0, 12, None), (42, 2, 9, None)], [(0, 2, 1, 1), (0, 7, 1, 5)]),
    "one-link": (12, (0.02, 0.004), [(41, 0, 12, None), (42, 2, 9, None)], [(0, 4, 1, 3)]),
    "tail": (20, (0.02, 0.004), [(43, 0, 20, None), (44, 3, 16, None)], [(0, 4, 1, 2), (0, 9, 1, 6), (0, 13, 1, 9)]),
    "chain-3": (14, (0.02, 0.004), [(45, 0, 14, None), (46, 1, 10, None), (47, 3, 11, None)], [(0, 3, 1, 2), (0, 9, 1, 8), (1, 4, 2, 2), (1, 9, 2, 6)]),
    "own-loops": (70, (0.02, 0.004), [(48, 0, 70, (2, 69)), (49, 5, 60, (1, 59))], [(0, 10, 1, 5), (0, 40, 1, 36)]),
    "wide-300": (300, PS.SMALL_DRIFT, [(50, 0, 300, None), (51, 0, 300, None)], [(0, 20 * k + 5, 1, 20 * k + 19) for k in range(14)]),
}
NAMES = list(_SPEC)
_CASES = {}


def case(name):
    """-> dict(seqs: per sequence gt (in the ANCHOR's frame) / est (its own frame) / loops / loop_poses, links, V: the assembled joint
    graph (assemble's dict), counts).  Cached: callers must not write into it."""
    if name in _CASES:
        return _CASES[name]
    n_tour, drift, seq_spec, link_spec = _SPEC[name]
    rng = np.random.default_rng(1000 + NAMES.index(name))
    seqs = [_sequence(n_tour, seed, first, count, None if k == 0 else WORLDS[k - 1], drift, own, rng)
            for k, (seed, first, count, own) in enumerate(seq_spec)]
    links = [_link(seqs, sf, kf, st, kt, rng) for sf, kf, st, kt in link_spec]
    V = assemble([s["est"] for s in seqs], [(s["loops"], s["loop_poses"]) for s in seqs], links)
    c = dict(seqs=seqs, links=links, V=V, counts=[len(s["est"]) for s in seqs])
    _CASES[name] = c
    return c


def centres(T_c_w):
    return np.array([-G.pose7_to_Rt(p)[0].T @ G.pose7_to_Rt(p)[1] for p in T_c_w])


def centre_errors(poses, gt):
    """distance of every keyframe's camera centre from the ground truth's"""
    return np.linalg.norm(centres(poses) - centres(gt), axis=1)
