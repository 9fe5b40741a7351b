"""GPU: flvis_loop_closer_merge -- several sequences' maps into one by a joint pose graph -- against the kernel-level call
(Context.pgo_loop_closure: the same k_pgo on the same device, bit for bit) and the CPU oracle (oracle/ref_pgo.cpp) on the virtual sequence
of the definition, which tests/_loop_merge.assemble builds from what the closer itself reports before the merge (poses, drift, accepted
loops).  Tolerances are the scheme of tests/test_gpu_pgo_edges.py on the oracle's own spread (pinned by tests/test_oracle_loop_merge.py).

Where only poses matter the keyframes are blank images: they store no landmarks and no words, their poses are what was fed times the
sequence's T_odom_map.  Compared against numpy products (PS.mul7, which goes through rotation matrices and so fixes the quaternion's
sign) a pose counts as equal to its negated quaternion; against the kernel-level call and the oracle, which form the same products as the
closer, it does not."""
import ctypes as C

import numpy as np
import pytest

import _geom as G
import _loop_chain as LC
import _loop_localize as LL
import _loop_merge as LM
import _pgo_synth as PS
import _voc as V
import test_gpu_loop_localize as TL
from test_oracle_loop_merge import MEASURED_FIX, fix_odometry
from test_oracle_pgo import perturbation_spread

pytestmark = pytest.mark.gpu
IDENT = LL.IDENT
NO_LOOPS = (np.zeros((0, 2), np.int32), np.zeros((0, 7)))


@pytest.fixture(scope="module")
def world():
    w = TL.World()
    yield w
    w.ctx.close()


def _load(w, lc, plan):
    """plan: {stream: [n, 7] odometry poses}: blank keyframes, one call per step for the streams that still have one"""
    for step in range(max(len(v) for v in plan.values())):
        streams = [s for s in sorted(plan) if step < len(plan[s])]
        blank = w.blank.expand(len(streams), -1, -1).contiguous()
        lc.add_keyframes(streams, blank, blank, [plan[s][step] for s in streams])


def _links(case, streams):
    """the case's links (group positions) on the closer's streams"""
    return [dict(l, seq_from=streams[l["seq_from"]], seq_to=streams[l["seq_to"]]) for l in case["links"]]


def _pdiff(a, b):
    """largest component difference of two pose arrays, a quaternion and its negative being one rotation"""
    a, b = np.asarray(a).reshape(-1, 7), np.asarray(b).reshape(-1, 7)
    flip = np.where((a[:, 3:] * b[:, 3:]).sum(1) < 0, -1.0, 1.0)[:, None]
    return max(np.abs(a[:, :3] - b[:, :3]).max(), np.abs(a[:, 3:] - flip * b[:, 3:]).max())


def _close(a, b, rel=1e-9):
    """within 1e-9 relative; 1e-300 lets the exact 0 of a tree equal itself"""
    return abs(a - b) <= rel * abs(b) + 1e-300


def _state(lc, n):
    return [(lc.poses(s), lc.drift(s)) for s in range(n)]


def _same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _check_against_references(ctx, name, V, counts, old, new, out, drift, iterations, floor, cap):
    """the merged group against the kernel-level call (bits) and the oracle (the scheme) on V; -> (oracle result, tolerance)"""
    s, ref = perturbation_spread(V, iterations, True)
    tol = max(floor, 10 * s)
    assert tol <= cap, (name, s)
    T, kdrift, stats, ran = ctx.pgo_loop_closure([V["est"]], [V["present"]], [V["loops"]], [V["loop_poses"]], iterations=iterations,
                                                   use_initial_guess=True)
    assert int(ran[0]) == 1 and ref[0] == 1 and out["optimised"]
    lo, vs = LM.last_vertices(V, counts)
    worst = 0.0
    for k, n in enumerate(counts):
        o, first = V["offsets"][k], lo if k == 0 else 0
        rows = slice(first, vs[k] + 1)
        assert np.array_equal(new[k][rows], T[0][o:o + n][rows]), (name, k)                     # the parent's kernel: bit for bit
        assert np.array_equal(new[k][:first], old[k][:first])                                   # before the anchor's first vertex
        worst = max(worst, np.abs(new[k][rows] - ref[1][o:o + n][rows]).max())
    assert np.abs(drift[-1] - kdrift[0]).max() < 1e-12                                          # k_pgo's own drift of its last vertex
    worst = max(worst, np.abs(drift[-1] - ref[2]).max())
    print("LOOP-MERGE %-10s iterations=%-3d s=%.2g tol=%.2g observed=%.2g stopped gpu/oracle=%d/%d chi2 %.9g -> %.9g"
          % (name, iterations, s, tol, worst, out["iterations"], ref[3][0], out["chi2_before"], out["chi2_after"]))
    assert worst <= tol, (name, iterations, worst, tol)
    assert (out["n_vertices"], out["n_edges"]) == (ref[3][3], ref[3][4]) == (stats[0][3], stats[0][4])
    assert _close(out["chi2_before"], ref[3][1]) and _close(out["chi2_after"], ref[3][2]), (out, ref[3])
    assert out["chi2_before"] == stats[0][1] and out["chi2_after"] == stats[0][2] and out["iterations"] == stats[0][0]
    return ref, tol


# the group's sequences on the closer's streams: not in stream order, not adjacent
_STREAMS = {2: [3, 0], 3: [4, 1, 2]}


@pytest.mark.parametrize("name", ["pair-12", "one-link", "tail", "chain-3"])
def test_joint_graph_against_the_kernel_level_call_and_the_oracle(world, name):
    """A closer of 5 sequences, max_keyframes = the largest count, the group on streams that are neither sorted nor adjacent.  Run to
    the end: vertex rows bit for bit the kernel-level call's on V, within max(1e-10, 10 s) of the oracle (cap 1e-6); stopped after 3
    iterations within max(1e-11, 10 s) (cap 1e-9) with the same iteration count; chi2 within 1e-9, vertex and edge counts equal; one
    link alone is a tree (chi2 exactly 0, one iteration)."""
    w = world
    case = LM.case(name)
    counts = case["counts"]
    streams = _STREAMS[len(counts)]
    lc = w.closer(5, max(counts))
    for iterations, floor, cap in ((100, 1e-10, 1e-6), (3, 1e-11, 1e-9)):
        lc.reset(list(range(5)))
        _load(w, lc, {s: q["est"] for s, q in zip(streams, case["seqs"])})
        old = [lc.poses(s) for s in streams]
        assert all(_pdiff(o, q["est"]) < 1e-15 for o, q in zip(old, case["seqs"]))               # identity T_odom_map: what was fed
        V = LM.assemble(old, [NO_LOOPS] * len(counts), case["links"])
        out, drift = lc.merge([streams], _links(case, streams), iterations=iterations)
        new = [lc.poses(s) for s in streams]
        ref, _ = _check_against_references(w.ctx, name, V, counts, old, new, out[0], drift, iterations, floor, cap)
        assert out[0]["iterations"] == ref[3][0] if iterations == 3 else out[0]["iterations"] >= 1
        if name == "one-link":
            assert out[0]["chi2_before"] == 0.0 and out[0]["chi2_after"] == 0.0 and out[0]["iterations"] == 1
        others = [s for s in range(5) if s not in streams]
        assert all(len(lc.poses(s)) == 0 and np.array_equal(lc.drift(s), IDENT) for s in others)
    lc.close()


def test_tail_drift_and_the_frame_of_later_keyframes(world):
    """`tail`: the links end at b's keyframe 9 of 16.  b was stored under a T_odom_map of its own (set_drift before its keyframes)."""
    w = world
    case = LM.case("tail")
    counts, (a, b) = case["counts"], (1, 2)
    lc = w.closer(3, 21)
    M = PS.mul7(LM.WORLDS[1], IDENT)
    lc.set_drift(b, M)
    _load(w, lc, {a: case["seqs"][0]["est"], b: case["seqs"][1]["est"]})
    old, before = [lc.poses(a), lc.poses(b)], [lc.drift(a), lc.drift(b)]
    assert _pdiff(old[1], [PS.mul7(p, M) for p in case["seqs"][1]["est"]]) < 1e-12
    V = LM.assemble(old, [NO_LOOPS] * 2, case["links"])
    lo, vs = LM.last_vertices(V, counts)
    assert (lo, vs) == (4, [19, 9])
    out, drift = lc.merge([[a, b]], _links(case, [a, b]))
    new = [lc.poses(a), lc.poses(b)]
    ref, tol = _check_against_references(w.ctx, "tail", V, counts, old, new, out[0], drift, 100, 1e-10, 1e-6)
    assert np.abs(drift[1] - ref[2]).max() <= tol                                                # the last sequence's drift: the oracle's
    for k, s in enumerate((a, b)):
        v = vs[k]
        assert _pdiff(PS.mul7(old[k][v], drift[k]), new[k][v]) < 1e-12                           # drift_s = inv(old(v_s)) * new(v_s)
        for j in range(v + 1, counts[k]):
            assert _pdiff(PS.mul7(old[k][j], drift[k]), new[k][j]) < 1e-12, (s, j)               # behind v_s: old * drift_s
        assert _pdiff(lc.drift(s), PS.mul7(before[k], drift[k])) < 1e-12                         # T_odom_map *= drift_s
    assert np.abs(new[1][10:] - old[1][10:]).max() > 1.0                                         # (the tail did move: metres)
    assert np.array_equal(new[0][:4], old[0][:4])                                                # the anchor before its first vertex
    # a keyframe added to b afterwards lands in the merged frame
    X = case["seqs"][1]["est"][-1]
    lc.add_keyframes([b], w.blank, w.blank, [X])
    assert _pdiff(lc.poses(b)[-1], PS.mul7(X, lc.drift(b))) < 1e-12
    assert _pdiff(lc.poses(b)[-1], new[1][-1]) < 1e-9                                            # the same odometry pose: the same place
    lc.close()


def test_batch_and_isolation(world):
    """Closers that got the same keyframes: `both` merges two disjoint groups in one call, `one` / `two` one group each, `never` none.
    The last keyframe of every sequence is still pending (added, not processed)."""
    w = world
    p12, tail = LM.case("pair-12"), LM.case("tail")
    g1, g2, outside = [0, 1], [3, 2], 4
    plan = {0: p12["seqs"][0]["est"], 1: p12["seqs"][1]["est"], 3: tail["seqs"][0]["est"], 2: tail["seqs"][1]["est"],
            outside: LM.case("chain-3")["seqs"][2]["est"]}
    closers = {}
    for key in ("both", "one", "two", "never"):
        lc = closers[key] = w.closer(5, 20)
        _load(w, lc, {s: p[:-1] for s, p in plan.items()})
        lc.process()
        blank = w.blank.expand(5, -1, -1).contiguous()
        lc.add_keyframes([0, 1, 2, 3, 4], blank, blank, [plan[s][-1] for s in range(5)])          # pending from here on
    l1, l2 = _links(p12, g1), _links(tail, g2)
    start = _state(closers["never"], 5)
    assert all(_same(_state(closers[k], 5), start) for k in closers)
    out_b, drift_b = closers["both"].merge([g1, g2], [l2[0], l1[0], l2[1], l1[1], l2[2]])         # the groups' links interleaved
    out_1, drift_1 = closers["one"].merge([g1], l1)
    out_2, drift_2 = closers["two"].merge([g2], l2)
    assert out_b == out_1 + out_2 and np.array_equal(drift_b, np.concatenate([drift_1, drift_2]))
    sb, s1, s2 = _state(closers["both"], 5), _state(closers["one"], 5), _state(closers["two"], 5)
    assert _same([sb[0], sb[1]], [s1[0], s1[1]]) and _same([sb[2], sb[3]], [s2[2], s2[3]])
    assert not np.array_equal(sb[1][0], start[1][0]) and not np.array_equal(sb[2][0], start[2][0])  # (and they did merge)
    # outside the groups nothing moved by a bit
    assert _same([sb[outside]], [start[outside]])
    assert _same([s1[2], s1[3], s1[4]], [start[2], start[3], start[4]]) and _same([s2[0], s2[1], s2[4]], [start[0], start[1], start[4]])
    # the pending keyframes, loop lists and the trigger: the next process reports what a closer that never merged reports
    want = closers["never"].process()
    assert [e["kf_curr"] for e in want] == [len(plan[s]) - 1 for s in range(5)]
    for key in ("both", "one", "two"):
        assert closers[key].process() == want, key
        assert all(np.array_equal(closers[key].similarity_row(s), closers["never"].similarity_row(s)) for s in range(5))
    assert _same(_state(closers["both"], 5), sb)                                                  # (process moved no pose)
    # a second merge is another run on the current poses
    again, _ = closers["both"].merge([g1], l1)
    assert again[0]["optimised"] and (again[0]["n_vertices"], again[0]["n_edges"]) == (out_b[0]["n_vertices"], out_b[0]["n_edges"])
    assert np.isfinite(closers["both"].poses(1)).all() and _same(_state(closers["both"], 5)[2:], sb[2:])
    for lc in closers.values():
        lc.close()


def test_arguments(world):
    import flvis_amd
    w = world
    case = LM.case("pair-12")
    lc = w.closer(5, 12)
    _load(w, lc, {0: case["seqs"][0]["est"], 1: case["seqs"][1]["est"], 2: case["seqs"][1]["est"][:4], 3: case["seqs"][0]["est"][:5]})
    ok = _links(case, [0, 1])                     # sequence 4 stays empty
    L = lambda sf, kf, st, kt, pose=None: dict(seq_from=sf, kf_from=kf, seq_to=st, kf_to=kt, pose=IDENT if pose is None else pose)
    nan, inf, zero_q = IDENT.copy(), IDENT.copy(), IDENT.copy()
    nan[1], inf[5], zero_q[6] = np.nan, np.inf, 0.0
    bad = {
        "no groups": ([], ok, 100),
        "a group of one": ([[0]], ok, 100),
        "a group of one beside a good one": ([[0, 1], [2]], ok, 100),
        "sequence out of range": ([[0, 5]], ok, 100),
        "negative sequence": ([[-1, 1]], ok, 100),
        "twice within a group": ([[0, 1, 0]], ok, 100),
        "twice across groups": ([[0, 1], [2, 1]], ok + [L(2, 0, 1, 0)], 100),
        "an empty sequence": ([[0, 1, 4]], ok + [L(0, 0, 4, 0)], 100),
        "a link out of the groups": ([[0, 1]], ok + [L(0, 0, 2, 0)], 100),
        "a link across groups": ([[0, 1], [2, 3]], ok + [L(2, 0, 3, 0), L(0, 0, 3, 0)], 100),
        "a link of an unknown sequence": ([[0, 1]], ok + [L(0, 0, 7, 0)], 100),
        "a link within a sequence": ([[0, 1]], ok + [L(1, 0, 1, 3)], 100),
        "a link against the group's order": ([[0, 1]], ok + [L(1, 0, 0, 3)], 100),
        "kf_from outside": ([[0, 1]], ok + [L(0, 12, 1, 0)], 100),
        "kf_to outside": ([[0, 1]], ok + [L(0, 0, 1, 9)], 100),
        "kf negative": ([[0, 1]], ok + [L(0, -1, 1, 0)], 100),
        "pose nan": ([[0, 1]], ok + [L(0, 0, 1, 0, nan)], 100),
        "pose inf": ([[0, 1]], ok + [L(0, 0, 1, 0, inf)], 100),
        "zero quaternion": ([[0, 1]], ok + [L(0, 0, 1, 0, zero_q)], 100),
        "no links": ([[0, 1]], [], 100),
        "an unconnected sequence": ([[0, 1, 2]], ok, 100),
        "connected to each other, not to the anchor": ([[0, 1, 2, 3]], ok + [L(2, 0, 3, 0)], 100),
        "iterations < 0": ([[0, 1]], ok, -1),
    }
    start = _state(lc, 5)
    for what, (groups, links, iterations) in bad.items():
        with pytest.raises(flvis_amd.FlvisError) as e:
            lc.merge(groups, links, iterations=iterations)
        assert "loop_closer_merge failed (-1)" in str(e.value), (what, str(e.value))             # FLVIS_ERR_INVALID_ARG
        assert _same(_state(lc, 5), start), what
    # NULL arguments and a group table that does not start at 0, through the C ABI
    lib, INVALID = w.ctx._lib, flvis_amd.FLVIS_ERR_INVALID_ARG
    ptr, seq, ptr1 = (C.c_int * 2)(0, 2), (C.c_int * 2)(0, 1), (C.c_int * 2)(1, 3)
    arr = (flvis_amd.FlvisLcLink * 2)(*[flvis_amd.FlvisLcLink(l["seq_from"], l["seq_to"], l["kf_from"], l["kf_to"], (C.c_double * 7)(*l["pose"]))
                                        for l in ok])
    out = (flvis_amd.FlvisLcMerge * 1)()
    assert lib.flvis_loop_closer_merge(lc._h, 1, None, seq, 2, arr, 100, out, None) == INVALID
    assert lib.flvis_loop_closer_merge(lc._h, 1, ptr, None, 2, arr, 100, out, None) == INVALID
    assert lib.flvis_loop_closer_merge(lc._h, 1, ptr, seq, 2, None, 100, out, None) == INVALID
    assert lib.flvis_loop_closer_merge(lc._h, 1, ptr, seq, 2, arr, 100, None, None) == INVALID
    assert lib.flvis_loop_closer_merge(lc._h, 0, ptr, seq, 2, arr, 100, out, None) == INVALID
    assert lib.flvis_loop_closer_merge(lc._h, -1, ptr, seq, 2, arr, 100, out, None) == INVALID
    assert lib.flvis_loop_closer_merge(lc._h, 1, ptr, seq, -1, arr, 100, out, None) == INVALID
    assert lib.flvis_loop_closer_merge(lc._h, 1, ptr1, seq, 2, arr, 100, out, None) == INVALID
    assert _same(_state(lc, 5), start)
    # the closer works afterwards: NULL h_drift7 is fine, the quaternion of a link is normalised, and the result is the plain call's
    twin = w.closer(2, 12)
    _load(w, twin, {0: case["seqs"][0]["est"], 1: case["seqs"][1]["est"]})
    want, _ = twin.merge([[0, 1]], ok, iterations=3)        # (stopped early: the two runs take the same steps)
    scaled = [dict(l, pose=np.concatenate([l["pose"][:3], 3.0 * np.asarray(l["pose"][3:])])) for l in ok]
    for k, l in enumerate(scaled):
        arr[k] = flvis_amd.FlvisLcLink(l["seq_from"], l["seq_to"], l["kf_from"], l["kf_to"], (C.c_double * 7)(*l["pose"]))
    assert lib.flvis_loop_closer_merge(lc._h, 1, ptr, seq, 2, arr, 3, out, None) == flvis_amd.FLVIS_OK
    assert out[0].optimised == 1 and (out[0].n_vertices, out[0].n_edges) == (want[0]["n_vertices"], want[0]["n_edges"])
    assert np.abs(lc.poses(1) - twin.poses(1)).max() < 1e-11 and np.abs(lc.drift(1) - twin.drift(1)).max() < 1e-11
    assert _same(_state(lc, 5)[2:], start[2:])
    twin.close()
    lc.close()


def test_own_loops_enter_the_graph():
    """The two-trajectory run of tests/test_gpu_loop_closer.py (62 keyframes rendered on the device, the same parameters) through
    process, so that both sequences have accepted loops of their own and optimised pose graphs behind them; then merge [0, 1] with three
    links from the ground truth of the two trajectories.  The joint graph is the oracle's on a V whose loop list holds both sequences'
    accepted loops in recorded order, then the links."""
    import os
    import tempfile
    import torch
    import flvis_amd
    from flvis_amd import synth
    ctx = flvis_amd.Context(0)
    p = os.path.join(tempfile.gettempdir(), "flvis_loopcloser_gpu.yaml")
    open(p, "w").write(synth.D435I_STEREO_YAML)
    cfg = flvis_amd.load_config(p)
    trs = [LC.LoopTrajectory(phase=0.0), LC.LoopTrajectory(phase=0.9)]
    rnd = synth.Renderer("cuda")
    n_kf, per = 62, 50
    times = LC.keyframe_times(n_kf, per)
    frames = [rnd.stereo_frame(trs, t, i) for i, t in enumerate(times)]
    gt = [[G.pose7(*tr.T_c_w(t, rnd.rig)) for t in times] for tr in trs]
    gt[1] = [gt[1][i] for i in range(n_kf) if i % 9 != 4]              # sequence 1 misses every ninth call
    odom = [LC.drifted_odometry([G.pose7(*tr.T_c_w(t, rnd.rig)) for t in times], 10 + s, sigma_t=0.008, sigma_r=0.002) for s, tr in enumerate(trs)]
    train = []
    for i in range(0, n_kf, 6):
        k, d, c, _ = ctx.orb_detect_and_compute(frames[i][0][0:1], cap=1024)
        train.append(d[0, :int(c[0])].cpu().numpy())
    ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))
    lc = flvis_amd.LoopCloser(ctx, cfg, LC.LC_PARAMS, n_streams=2, max_keyframes=64)
    own = [([], []), ([], [])]
    for i in range(n_kf):
        streams = [0] if i % 9 == 4 else [0, 1]
        sel = torch.tensor(streams, device="cuda")
        lc.add_keyframes(streams, frames[i][0][sel].contiguous(), frames[i][1][sel].contiguous(), np.array([odom[s][i] for s in streams]))
        for s, e in enumerate(lc.process()):
            if e["accepted"]:
                own[s][0].append((e["kf_prev"], e["kf_curr"]))
                own[s][1].append(e["pose"])
    assert all(len(o[0]) >= 2 for o in own), own
    old, before = [lc.poses(0), lc.poses(1)], [lc.drift(0), lc.drift(1)]
    counts = [len(o) for o in old]
    assert counts == [62, 55] and not np.array_equal(before[0], IDENT) and not np.array_equal(before[1], IDENT)   # pose graphs have run
    rng = np.random.default_rng(4)
    links = [dict(seq_from=0, kf_from=a, seq_to=1, kf_to=b, pose=PS.loop_pose(dict(gt=[gt[0][a], gt[1][b]]), 0, 1, loop_noise=PS.LOOP_NOISE, rng=rng))
             for a, b in ((6, 3), (30, 28), (55, 50))]
    Vg = LM.assemble(old, [(np.array(o[0], np.int32), np.array(o[1])) for o in own], links)
    assert len(Vg["loops"]) == len(own[0][0]) + len(own[1][0]) + 3
    out, drift = lc.merge([[0, 1]], links)
    new = [lc.poses(0), lc.poses(1)]
    _check_against_references(ctx, "own-loops", Vg, counts, old, new, out[0], drift, 100, 1e-10, 1e-6)
    for s in range(2):
        assert _pdiff(lc.drift(s), PS.mul7(before[s], drift[s])) < 1e-12
    assert out[0]["chi2_after"] < out[0]["chi2_before"] and out[0]["n_vertices"] > 100, out
    lc.close()
    ctx.close()


def test_from_a_real_fix(world):
    """The unit-enters-a-map flow on the tour of tests/_loop_localize.py: sequence 0 holds the 9 keyframes at ground truth; the 4 query
    frames are stored as sequence 1's keyframes (a drifted odometry in a world frame of its own) AND localised in sequence 0's map;
    links_from_fix, merge.  The joint graph is the oracle's on the same links; sequence 1 lands on the queries' true poses within twice
    what the oracle-assembled chain leaves on the CPU (test_oracle_loop_merge.MEASURED_FIX: the margin for the device's features)."""
    import flvis_amd
    w = world
    sc = w.sc
    lc = w.closer(2, 9)
    for i in range(9):
        lc.add_keyframes([0], w.kf0[i:i + 1], w.kf1[i:i + 1], [sc.kf_gt[i]])
    q_odom = fix_odometry(sc)
    links = []
    for k in range(4):
        kid = lc.add_keyframes([1], w.q0[k:k + 1], w.q1[k:k + 1], [q_odom[k]])
        fix = lc.localize_in([1], [0], w.q0[k:k + 1], w.q1[k:k + 1], n_best=8)[0]
        mine = flvis_amd.links_from_fix(fix, 1, int(kid[0]))
        assert len(mine) == sum(c["accepted"] for c in fix["candidates"]) >= 2 and all(l["seq_from"] == 0 and l["kf_to"] == k for l in mine)
        links += mine
    old = [lc.poses(0), lc.poses(1)]
    off = max(LL.pose_error(old[1][k], sc.q_gt[k])[0] for k in range(4))
    Vg = LM.assemble(old, [NO_LOOPS] * 2, links)                     # (group positions = streams here)
    out, drift = lc.merge([[0, 1]], links)
    new = [lc.poses(0), lc.poses(1)]
    _check_against_references(w.ctx, "real-fix", Vg, [9, 4], old, new, out[0], drift, 100, 1e-10, 1e-6)
    errs = [LL.pose_error(new[1][k], sc.q_gt[k]) for k in range(4)]
    print("LOOP-MERGE real-fix: %d links, sequence 1 off by %.2f m before, at most %.4f m %.4f rad after" %
          (len(links), off, max(e[0] for e in errs), max(e[1] for e in errs)))
    assert off > 5.0 and max(e[0] for e in errs) <= 2 * MEASURED_FIX[0] and max(e[1] for e in errs) <= 2 * MEASURED_FIX[1], errs
    lc.close()
