#!/usr/bin/env python3
"""flvis_loop_closer on one GPU: S sequences that each circle the rendered room and come back, one keyframe per sequence and call.
Times add_keyframes (ORB + bag of words + 3-D landmarks + store) and process (similarity row, candidates, verification of all
candidates at once, pose graphs) per batch with HIP events around the calls; prints one JSON line.

--rigs: a mixed fleet instead of one config -- sequence s runs on unit s % 4 of synth.rig_variant("d435i_stereo", .), rendered with that
unit's rig, all in one closer (flvis_loop_closer_create_rigs).

--localize: after the tour, one flvis_loop_closer_localize call for all sequences (a frame rendered between two keyframes of each) at
n_best = 1, 4 and 8: ms per call, and per stage -- the query's features timed through the separate entry points on the same batch (ORB,
bag of words, landmarks), the rest of the call (store, scores, candidate selection, n_streams * n_best pair checks, the result copy) as the
difference -- next to this run's add_keyframes + process time for one batch; a second JSON line.

--localize-in: after the tour, flvis_loop_closer_localize_in for all sequences on the same frame, next to localize in the same run, at
n_best = 1, 4 and 8: with every query in its own map (the same kernels as localize apart from the selection), in its neighbour's map
(sequence s in the map of s + 1), and in all maps (n_streams x n_streams score jobs, candidates ranked across the maps); ms per call, the
calls taken in turns; the size of the score rows; a further JSON line.  --localize-in=all: only the all-maps calls at n_best = 8 (a run
under a profiler then holds nothing else of the new kernels).  max_keyframes sizes the databases and the score rows (default: n_keyframes).

--link: after the tour, flvis_loop_closer_link with the NEWEST stored keyframe of every sequence as the query, next to
flvis_loop_closer_localize_in on the images that keyframe was stored from, at n_best = 1, 4 and 8: into the neighbour's map (sequence s in
the map of s + 1; link with own_gap = -1) and into all maps (localize_in: all maps, its own included -- it has no exclusion; link: all
OTHER maps); ms per call, the calls taken in turns; then every keyframe of sequence s against map s + 1 in ONE link call (n_streams *
n_keyframes queries, n_best = 4): ms per call and per query; a further JSON line.  With a library that has no flvis_loop_closer_link
(FLVIS_LIB_PATH: the parent commit's) only the localize_in legs run: the same script then gives the parent's figures.

--unrect: instead of all the above, what the opt-in landmarks of an unrectified stereo rig cost (flvis_loop_closer_set_stereo_unrect): S
sequences on the EuRoC-like rig (752 x 480), add_keyframes per call with the switch on against the switch off -- off is the same ORB and
bag of words without landmarks, so the difference is the feature's own cost -- the two closers taken in turns on the same frames; beside
them, as an indication only (another image size), the rectified-stereo case of the D435i rig (640 x 480) in the same turns; one JSON line.

usage: loop_closer_bench.py [--rigs] [--localize] [--localize-in[=all]] [--link] [--unrect] [n_streams=64] [n_keyframes=60] [max_keyframes]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import flvis_amd
from flvis_amd import synth
import _geom as G
import _loop_chain as LC
import _pgo_synth as PS
import _voc as V

RIGS = "--rigs" in sys.argv[1:]
LOCALIZE = "--localize" in sys.argv[1:]
LOCALIZE_IN = [a for a in sys.argv[1:] if a.split("=")[0] == "--localize-in"]
LINK = "--link" in sys.argv[1:]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(args[0]) if len(args) > 0 else 64
N = int(args[1]) if len(args) > 1 else 60
MAXKF = int(args[2]) if len(args) > 2 else N
PER = 50
N_UNITS = 4

ctx = flvis_amd.Context(0)
if "--unrect" in sys.argv[1:]:
    trs = [LC.LoopTrajectory(phase=2 * np.pi * s / S) for s in range(S)]
    times = LC.keyframe_times(N, PER)
    ident = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (S, 1))
    legs, frames = {}, {}
    for name, rig, text in (("euroc", synth.euroc_rig(), synth.EUROC_LIKE_YAML), ("d435i", synth.d435_rig(), synth.D435I_STEREO_YAML)):
        p = os.path.join(tempfile.gettempdir(), "flvis_loop_closer_bench_%s.yaml" % name)
        open(p, "w").write(text)
        rnd = synth.Renderer("cuda", rig=rig)
        frames[name] = [rnd.stereo_frame(trs, t, i) for i, t in enumerate(times)]
        legs[name] = flvis_amd.load_config(p)
    train = []
    for i in range(0, N, 6):
        k, d, c, _ = ctx.orb_detect_and_compute(frames["euroc"][i][0][0:1], cap=1024)
        train.append(d[0, :int(c[0])].cpu().numpy())
    ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))
    closers = {"unrect_off": ("euroc", flvis_amd.LoopCloser(ctx, legs["euroc"], LC.LC_PARAMS, n_streams=S, max_keyframes=MAXKF)),
               "unrect_on": ("euroc", flvis_amd.LoopCloser(ctx, legs["euroc"], LC.LC_PARAMS, n_streams=S, max_keyframes=MAXKF)),
               "rect_d435i": ("d435i", flvis_amd.LoopCloser(ctx, legs["d435i"], LC.LC_PARAMS, n_streams=S, max_keyframes=MAXKF))}
    closers["unrect_on"][1].set_stereo_unrect(True)
    ms = {k: [] for k in closers}
    streams = list(range(S))
    torch.cuda.synchronize()
    for i in range(N):                                                     # the legs in turns: a drift of the clocks hits all alike
        for k, (rig, lc) in closers.items():
            t0 = time.perf_counter()
            lc.add_keyframes(streams, frames[rig][i][0], frames[rig][i][1], ident)      # returns after the batch is stored (it synchronises)
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"n_streams": S, "n_keyframes": N, "image_size": {"unrect": [752, 480], "rect_d435i": [640, 480]}}
    for k, (rig, lc) in closers.items():
        v = np.array(ms[k][5:])                                            # (the first calls also allocate and load code objects)
        out["add_keyframes_ms_%s" % k] = {"median": float(np.median(v)), "mean": float(v.mean()), "min": float(v.min()), "max": float(v.max())}
        out["landmarks_per_keyframe_%s" % k] = float(np.mean([len(lc.keyframe(s, N - 1)["lm2"]) for s in range(0, S, max(1, S // 8))]))
    d = np.array(ms["unrect_on"][5:]) - np.array(ms["unrect_off"][5:])
    out["unrect_landmarks_cost_ms_per_call"] = {"median": float(np.median(d)), "mean": float(d.mean()), "min": float(d.min()), "max": float(d.max())}
    out["timing"] = "host wall clock around calls that return synchronised, calls 5 .. n_keyframes - 1, the three closers in turns"
    print(json.dumps(out))
    for _, lc in closers.values():
        lc.close()
    ctx.close()
    sys.exit(0)
trs = [LC.LoopTrajectory(phase=2 * np.pi * s / S) for s in range(S)]
times = LC.keyframe_times(N, PER)
if RIGS:
    units = []
    for k in range(N_UNITS):
        rig, text = synth.rig_variant("d435i_stereo", k)
        p = os.path.join(tempfile.gettempdir(), "flvis_loop_closer_bench_%d.yaml" % k)
        open(p, "w").write(text)
        units.append((synth.Renderer("cuda", rig=rig), flvis_amd.load_config(p)))
    cfg = [units[s % N_UNITS][1] for s in range(S)]
    rigs = [units[s % N_UNITS][0].rig for s in range(S)]
    order = [s for k in range(N_UNITS) for s in range(k, S, N_UNITS)]   # every unit renders its own sequences; then back in sequence order
    back = torch.tensor(np.argsort(order), device="cuda")
    frames = []
    for i, t in enumerate(times):
        parts = [units[k][0].stereo_frame([trs[s] for s in range(k, S, N_UNITS)], t, i) for k in range(min(N_UNITS, S))]
        frames.append(tuple(torch.cat([q[c] for q in parts])[back].contiguous() for c in range(2)))
else:
    p = os.path.join(tempfile.gettempdir(), "flvis_loop_closer_bench.yaml")
    open(p, "w").write(synth.D435I_STEREO_YAML)
    cfg = flvis_amd.load_config(p)
    rnd = synth.Renderer("cuda")
    rigs = [rnd.rig] * S
    frames = [rnd.stereo_frame(trs, t, i) for i, t in enumerate(times)]
gt = [[G.pose7(*trs[s].T_c_w(t, rigs[s])) for t in times] for s in range(S)]
odom = [LC.drifted_odometry(gt[s], 100 + s, sigma_t=0.008, sigma_r=0.002) for s in range(S)]
train = []
for i in range(0, N, 6):
    k, d, c, _ = ctx.orb_detect_and_compute(frames[i][0][0:1], cap=1024)
    train.append(d[0, :int(c[0])].cpu().numpy())
ctx.bow_set_vocabulary(*V.build_vocabulary(train, k=8, depth=3))
lc = flvis_amd.LoopCloser(ctx, cfg, LC.LC_PARAMS, n_streams=S, max_keyframes=MAXKF)
streams = list(range(S))
t_add, t_proc, n_cand, n_acc, n_opt = [], [], [], [], []
torch.cuda.synchronize()
for i in range(N):
    T = np.array([odom[s][i] for s in range(S)])
    t0 = time.perf_counter()
    lc.add_keyframes(streams, frames[i][0], frames[i][1], T)          # returns after the batch is stored (it synchronises)
    t1 = time.perf_counter()
    ev = lc.process()                                                  # returns with the events on the host
    t2 = time.perf_counter()
    t_add.append((t1 - t0) * 1e3)
    t_proc.append((t2 - t1) * 1e3)
    n_cand.append(sum(e["candidate"] for e in ev))
    n_acc.append(sum(e["accepted"] for e in ev))
    n_opt.append(sum(e["optimised"] for e in ev))
gap0 = np.mean([PS.loop_gap(np.array(odom[s]), np.array(gt[s]), 2, N - 1)[0] for s in range(S)])
gap1 = np.mean([PS.loop_gap(lc.poses(s), np.array(gt[s]), 2, N - 1)[0] for s in range(S)])
quiet = [i for i in range(5, N) if n_cand[i] == 0]
busy = [i for i in range(N) if n_opt[i] > 0]
print(json.dumps({
    "n_streams": S, "n_keyframes": N, "rig_units": N_UNITS if RIGS else 1,
    "add_keyframes_ms_per_batch": float(np.mean([t_add[i] for i in range(5, N)])),
    "process_ms_per_batch_no_candidate": float(np.mean([t_proc[i] for i in quiet])) if quiet else None,
    "process_ms_per_batch_with_pose_graphs": float(np.mean([t_proc[i] for i in busy])) if busy else None,
    "pose_graphs_per_busy_batch": float(np.mean([n_opt[i] for i in busy])) if busy else None,
    "candidates": int(sum(n_cand)), "loops_accepted": int(sum(n_acc)), "pose_graph_runs": int(sum(n_opt)),
    "mean_loop_gap_m_odometry": float(gap0), "mean_loop_gap_m_after": float(gap1),
    "timing": "host wall clock around calls that return synchronised"}))

if LOCALIZE or LOCALIZE_IN or LINK:
    tq = 0.5 * (times[N // 2] + times[N // 2 + 1])                    # between two keyframes of the tour
    if RIGS:
        parts = [units[k][0].stereo_frame([trs[s] for s in range(k, S, N_UNITS)], tq, N) for k in range(min(N_UNITS, S))]
        q0, q1 = (torch.cat([q[c] for q in parts])[back].contiguous() for c in range(2))
    else:
        q0, q1 = rnd.stereo_frame(trs, tq, N)
    cfg0 = cfg[0] if RIGS else cfg
    P0, P1 = np.array(list(cfg0.P0)), np.array(list(cfg0.P1))

    def timed(f, reps=5):
        f()                                                            # warm-up (the first localize call also grows the pair-check buffers)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps, r

if LOCALIZE:
    t_orb, (kps, desc, cnt, _) = timed(lambda: ctx.orb_detect_and_compute(q0, cap=1024))
    t_bow, _ = timed(lambda: ctx.bow_transform(desc, cnt, vcap=1024))
    t_lm, _ = timed(lambda: ctx.lc_keyframe_landmarks(q0, q1, 0, kps, desc, cnt, P0=P0, P1=P1))
    out = {"n_streams": S, "n_keyframes": N, "rig_units": N_UNITS if RIGS else 1,
           "query_orb_ms": t_orb, "query_bow_ms": t_bow, "query_landmarks_ms": t_lm,
           "add_keyframes_plus_process_ms_per_batch": float(np.mean([t_add[i] + t_proc[i] for i in range(5, N)]))}
    for n_best in (1, 4, 8):
        ms, fix = timed(lambda: lc.localize(streams, q0, q1, n_best=n_best))
        out["localize_ms_n_best_%d" % n_best] = ms
        out["select_and_pair_checks_ms_n_best_%d" % n_best] = ms - (t_orb + t_bow + t_lm)
        out["localised_n_best_%d" % n_best] = int(sum(f["best"] >= 0 for f in fix))
        out["candidates_n_best_%d" % n_best] = int(sum(len(f["candidates"]) for f in fix))
    out["timing"] = "host wall clock around synchronised calls, mean of 5 after a warm-up; stages: separate entry points on the same batch"
    print(json.dumps(out))

if LOCALIZE_IN:
    only_all = LOCALIZE_IN[-1].endswith("=all")
    ALL = flvis_amd.FLVIS_LC_ALL_MAPS
    legs = {"all_maps": [ALL] * S} if only_all else {"localize": None, "own_map": streams, "next_map": [(s + 1) % S for s in streams], "all_maps": [ALL] * S}
    call = lambda maps, n_best: lc.localize(streams, q0, q1, n_best=n_best) if maps is None else lc.localize_in(streams, maps, q0, q1, n_best=n_best)
    out = {"n_streams": S, "n_keyframes": N, "max_keyframes": MAXKF, "rig_units": N_UNITS if RIGS else 1,
           "score_rows_bytes_one_map": 8 * S * MAXKF, "score_rows_bytes_all_maps": 8 * S * S * MAXKF}
    for n_best in ((8,) if only_all else (1, 4, 8)):
        ms = {k: [] for k in legs}
        for k, maps in legs.items():
            call(maps, n_best)                                         # warm-up (the first calls also allocate and grow buffers)
        for _ in range(3 if only_all else 7):                          # the legs in turns: a drift of the clocks hits all alike
            for k, maps in legs.items():
                ms[k].append(timed(lambda: call(maps, n_best), reps=3)[0])
        for k, maps in legs.items():
            fix = call(maps, n_best)
            out["%s_ms_n_best_%d" % (k, n_best)] = float(np.median(ms[k]))
            out["%s_ms_min_max_n_best_%d" % (k, n_best)] = [float(min(ms[k])), float(max(ms[k]))]
            out["%s_localised_n_best_%d" % (k, n_best)] = int(sum(f["best"] >= 0 for f in fix))
            out["%s_candidates_n_best_%d" % (k, n_best)] = int(sum(len(f["candidates"]) for f in fix))
            if maps is not None and maps[0] == ALL:
                out["all_maps_found_in_own_map_n_best_%d" % n_best] = int(sum(f["map"] == s for s, f in zip(streams, fix)))
    out["timing"] = "host wall clock around synchronised calls: median (and min, max) of 7 rounds of 3 calls, the legs in turns, each round after a warm-up call"
    print(json.dumps(out))

if LINK:
    ALL = flvis_amd.FLVIS_LC_ALL_MAPS
    has_link = hasattr(flvis_amd.load_library(), "flvis_loop_closer_link")
    k0, k1 = frames[N - 1]                                             # what the newest keyframe of every sequence was stored from
    nxt = [(s + 1) % S for s in streams]
    legs = {"localize_in_next_map": lambda nb: lc.localize_in(streams, nxt, k0, k1, n_best=nb),
            "localize_in_all_maps": lambda nb: lc.localize_in(streams, [ALL] * S, k0, k1, n_best=nb)}
    if has_link:
        legs["link_next_map"] = lambda nb: lc.link([(s, nxt[s], -1, -1) for s in streams], n_best=nb)[0]
        legs["link_all_other_maps"] = lambda nb: lc.link([(s, ALL, -1, -1) for s in streams], n_best=nb)[0]
    out = {"n_streams": S, "n_keyframes": N, "max_keyframes": MAXKF, "rig_units": N_UNITS if RIGS else 1, "library_has_link": has_link}
    for n_best in (1, 4, 8):
        ms = {k: [] for k in legs}
        for k, f in legs.items():
            f(n_best)                                                  # warm-up (the first calls also allocate and grow buffers)
        for _ in range(7):                                             # the legs in turns: a drift of the clocks hits all alike
            for k, f in legs.items():
                ms[k].append(timed(lambda: f(n_best), reps=3)[0])
        for k, f in legs.items():
            fix = f(n_best)
            out["%s_ms_n_best_%d" % (k, n_best)] = float(np.median(ms[k]))
            out["%s_ms_min_max_n_best_%d" % (k, n_best)] = [float(min(ms[k])), float(max(ms[k]))]
            out["%s_localised_n_best_%d" % (k, n_best)] = int(sum(f_["best"] >= 0 for f_ in fix))
            out["%s_accepted_n_best_%d" % (k, n_best)] = int(sum(c["accepted"] for f_ in fix for c in f_["candidates"]))
        if has_link:                                                   # the same stored frames: link's fix is localize_in's
            a, b = legs["localize_in_next_map"](n_best), legs["link_next_map"](n_best)
            out["link_equals_localize_in_n_best_%d" % n_best] = bool(all(
                x["best"] == y["best"] and [(c["seq"], c["kf"], c["n_inliers"]) for c in x["candidates"]] ==
                [(c["seq"], c["kf"], c["n_inliers"]) for c in y["candidates"]] for x, y in zip(a, b)))
    if has_link:
        whole = [(s, nxt[s], k, -1) for s in streams for k in range(N)]
        ms = [timed(lambda: lc.link(whole, n_best=4), reps=1)[0] for _ in range(3)]
        fixes, links = lc.link(whole, n_best=4)
        out["whole_map_queries"] = len(whole)
        out["whole_map_ms_n_best_4"] = float(np.median(ms))
        out["whole_map_ms_min_max_n_best_4"] = [float(min(ms)), float(max(ms))]
        out["whole_map_us_per_query_n_best_4"] = float(np.median(ms)) * 1e3 / len(whole)
        out["whole_map_links_n_best_4"] = len(links)
        out["whole_map_localised_n_best_4"] = int(sum(f_["best"] >= 0 for f_ in fixes))
    out["timing"] = ("host wall clock around synchronised calls: median (and min, max) of 7 rounds of 3 calls, the legs in turns, each round "
                     "after a warm-up call; whole map: median of 3 single calls, each after a warm-up call")
    print(json.dumps(out))
