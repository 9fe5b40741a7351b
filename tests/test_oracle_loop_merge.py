"""CPU: the joint pose graph of several sequences' maps (flvis_loop_closer_merge's definition) on the oracle alone -- the reference's
graph rule (oracle/ref_pgo.cpp, unchanged) applied to the virtual sequence [a | 5 absent | b | ...] of tests/_loop_merge.py with the
inter-map links as loops: the graph it builds, that it brings the other maps into the anchor's frame, and the oracle's own spread under
last-bit perturbations, from which tests/test_gpu_loop_merge.py takes its tolerances (the scheme of tests/test_gpu_pgo_edges.py)."""
import numpy as np

import _loop_chain as LC
import _loop_localize as LL
import _loop_localize_in as LI
import _loop_merge as LM
import _pgo_synth as PS
import _voc as V
from test_oracle_bow import RefVoc
from test_oracle_pgo import expected_counts, perturbation_spread, pgo_case

# s of perturbation_spread (K = 8, seed 0) measured on the oracle alone: case -> (converged, stopped after 3 iterations)
SPREAD = {"pair-12": (1.3e-9, 4.5e-14), "one-link": (5.8e-14, 5.8e-14), "tail": (9.8e-10, 4.8e-14), "chain-3": (4.9e-10, 8.2e-14),
          "own-loops": (3.3e-8, 6.3e-14), "wide-300": (1.4e-10, 4.6e-13)}
# (vertices, edges, iterations run to the end) of the same runs
GRAPH = {"pair-12": (16, 52, 6), "one-link": (12, 32, 1), "tail": (26, 103, 10), "chain-3": (28, 99, 5), "own-loops": (128, 614, 7),
         "wide-300": (575, 2859, 12)}

# what the oracle-assembled chain leaves of the queries' pose errors in test_merge_from_real_fixes (metres, radians), measured
MEASURED_FIX = (0.026677, 0.016364)


def fix_odometry(sc):
    """the visiting unit's odometry of the tour's 4 query frames: drifted, in a world frame of its own"""
    Wi = PS.inv7(LM.WORLDS[0])
    return [PS.mul7(p, Wi) for p in LC.drifted_odometry(sc.q_gt, 5, sigma_t=0.008, sigma_r=0.002)]


def drift_bound(name):
    """What odometry drift alone leaves of a map's accuracy, 3 sigma: per step sigma_t metres and sigma_r radians (the case's drift), a
    random walk over the tour's n steps, the rotation on the tour's 6 m diameter as lever.  The merged map cannot beat the anchor's own
    drift where the links attach, and no link pulls harder than the chains: this is the scale the other maps must come down to."""
    n_tour, drift = LM._SPEC[name][:2]
    return 3 * np.sqrt(n_tour) * (drift[0] + 6.0 * drift[1])


def test_assembly_is_the_virtual_sequence_of_the_definition():
    c = LM.case("chain-3")
    V = c["V"]
    assert V["offsets"] == [0, 14 + 5, 14 + 5 + 10 + 5] and len(V["est"]) == 14 + 10 + 11 + 10
    assert V["present"].tolist() == [1] * 14 + [0] * 5 + [1] * 10 + [0] * 5 + [1] * 11
    assert V["loops"].tolist() == [[3, 21], [9, 27], [23, 36], [28, 40]]
    assert np.array_equal(V["est"][19:29], c["seqs"][1]["est"]) and np.array_equal(V["est"][14], [0, 0, 0, 0, 0, 0, 1])
    o = LM.case("own-loops")["V"]                              # own loops first, sequence by sequence, then the links
    assert o["loops"].tolist() == [[2, 69], [76, 134], [10, 80], [40, 111]]
    assert LM.last_vertices(LM.case("tail")["V"], [20, 16]) == (4, [19, 9])


def test_joint_graph_brings_the_other_maps_into_the_anchors_frame():
    for name in LM.NAMES:
        c = LM.case(name)
        V = c["V"]
        r, T, drift, stats = pgo_case(V)
        assert r == 1 and (stats[3], stats[4]) == expected_counts(V) == GRAPH[name][:2] and stats[0] == GRAPH[name][2], (name, stats)
        keep = np.ones(len(T), bool)
        lo, hi = int(V["loops"][:, 0].min()), int(V["loops"][:, 1].max())
        keep[lo:hi + 1] = V["present"][lo:hi + 1] == 0
        assert np.array_equal(T[keep], V["est"][keep]), name    # before the anchor's first vertex, behind max(later), the absent rows
        new, drifts = LM.apply(V, c["counts"], T)
        d = drifts[-1] if drifts[-1][3:] @ drift[3:] >= 0 else np.concatenate([drifts[-1][:3], -drifts[-1][3:]])   # (q and -q: one pose)
        assert np.abs(d - drift).max() < 1e-12, name             # the last sequence's drift is the graph's
        bound = drift_bound(name)
        for k in range(1, len(c["seqs"])):
            before = LM.centre_errors(c["seqs"][k]["est"], c["seqs"][k]["gt"]).max()
            after = LM.centre_errors(new[k], c["seqs"][k]["gt"]).max()
            print("LOOP-MERGE %-10s sequence %d: centres off by %.2f m before, %.3f m after (bound %.2f m)" % (name, k, before, after, bound))
            assert before > 5.0 and after <= bound and after < 0.1 * before, (name, k, before, after)
        assert LM.centre_errors(new[0], c["seqs"][0]["gt"]).max() <= bound


def test_one_link_is_a_tree():
    """one link between two chains: the initial guess carries the other map over and satisfies every edge -- chi2 exactly 0, one iteration"""
    st = pgo_case(LM.case("one-link")["V"])[3]
    assert st[0] == 1 and st[1] == 0.0 and st[2] == 0.0


def test_perturbation_spread_stays_inside_the_tolerance_scheme():
    """every case within a factor of 10 of the recorded table, converged s <= 1e-7 (tolerance max(1e-10, 10 s) <= 1e-6), stopped after 3
    iterations s <= 1e-10 (tolerance max(1e-11, 10 s) <= 1e-9) with the cap reached on every case but the tree"""
    assert sorted(SPREAD) == sorted(LM.NAMES) == sorted(GRAPH)
    for name, (s_conv, s_early) in SPREAD.items():
        V = LM.case(name)["V"]
        s, _ = perturbation_spread(V, 100, True)
        assert s <= 10 * s_conv and s <= 1e-7, (name, s)
        s, ref = perturbation_spread(V, 3, True)
        assert s <= 10 * s_early and s <= 1e-10, (name, s)
        assert ref[3][0] == (1 if name == "one-link" else 3), (name, ref[3])


def test_merge_from_real_fixes():
    """The unit-enters-a-map flow on the oracle's side: the tour's 9 keyframes at ground truth as map 0, the 4 query frames stored as
    sequence 1 (fix_odometry) and localised in map 0 by the oracle-assembled chain (tests/_loop_localize_in.ref_localize_in on the
    oracle's features); every accepted candidate is a link; the oracle's joint graph.  Sequence 1 comes from metres off to the accuracy
    of the fixes: MEASURED_FIX pins the figure, tests/test_gpu_loop_merge.py asserts twice that of the device's run."""
    sc = LL.scene()
    P0, P1, K4 = LL.cam_of(LL.stereo_cfg())
    raw = [LL.oracle_features(a, b, P0, P1) for a, b in sc.kf]
    rv = RefVoc(V.build_vocabulary([f["desc"] for f in raw], k=6, depth=3))
    feat = lambda f: dict(f, bow=rv.transform(f["desc"]))
    refs = {0: LC.RefLoopCloser(K4, prm=LL.PARAMS, stream=0)}
    for f, T in zip(raw, sc.kf_gt):
        refs[0].add(feat(f), T)
    q_odom = fix_odometry(sc)
    links = []
    for k, (a, b) in enumerate(sc.q):
        fix = LI.ref_localize_in(refs, 0, feat(LL.oracle_features(a, b, P0, P1)), 1, K4, 8)
        links += [dict(seq_from=0, kf_from=c["kf"], seq_to=1, kf_to=k, pose=c["pose"]) for c in fix["candidates"] if c["accepted"]]
    assert len(links) >= 8
    Vg = LM.assemble([np.array(sc.kf_gt), np.array(q_odom)], [(np.zeros((0, 2), np.int32), np.zeros((0, 7)))] * 2, links)
    s, ref = perturbation_spread(Vg, 100, True)
    assert ref[0] == 1 and s <= 1e-7, s
    new, _ = LM.apply(Vg, [9, 4], ref[1])
    before = max(LL.pose_error(q_odom[k], sc.q_gt[k])[0] for k in range(4))
    errs = [LL.pose_error(new[1][k], sc.q_gt[k]) for k in range(4)]
    et, ea = max(e[0] for e in errs), max(e[1] for e in errs)
    print("LOOP-MERGE real-fix (oracle chain): %d links, s=%.2g, off by %.2f m before, at most %.6f m %.6f rad after" % (len(links), s, before, et, ea))
    assert before > 5.0 and et <= MEASURED_FIX[0] * 1.001 and ea <= MEASURED_FIX[1] * 1.001, (et, ea)
    assert np.array_equal(new[0][:int(Vg["loops"][:, 0].min())], np.array(sc.kf_gt)[:int(Vg["loops"][:, 0].min())])
