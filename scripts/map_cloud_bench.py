#!/usr/bin/env python3
"""flvis_loop_closer_map_cloud on one GPU: the maps of 64 sequences as voxel clouds, as 64 single-sequence clouds and as 16 groups of 4, at
leaf = 0.08 and leaf = 0, while the sequences grow (the keyframe counts of --kfs).  Keyframes are stored from the test scene's images
(tests/_loop_localize.scene), taken in turns, each lap of the scene moved on by half a metre so that the map keeps growing.

Per point of the sweep one JSON line: ms per call (host wall clock around the call, which returns synchronised on its own counts: median,
min and max of --reps calls after a warm-up call), the input points, the rows out, the sort passes run and skipped, the workspace bytes,
the bytes the call moves as counted from the implementation (csrc/map_cloud.hip) and the time those bytes take at --tbps (2.7: the 2.6-2.8
TB/s the pyramid ingest reached), and the call's fraction of that bound.  For one sequence also the route that exists
without the call: flvis_loop_closer_keyframe for every keyframe + flvis_loop_closer_poses + the numpy restatement (tests/_map_cloud.py).

--md FILE appends the lines as a markdown table.  --trace: a short run for a kernel trace (rocprofv3 --kernel-trace --stats -- python
scripts/map_cloud_bench.py --trace): fills to the first --kfs count and makes 5 calls of each configuration, nothing else.

usage: map_cloud_bench.py [--kfs 10,50,200] [--streams 64] [--reps 7] [--tbps 2.7] [--md FILE] [--trace]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import flvis_amd
import _loop_localize as LL
import _map_cloud as MC
import _pgo_synth as PS
import _voc as V

ap = argparse.ArgumentParser()
ap.add_argument("--kfs", default="10,50,200")
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--tbps", type=float, default=2.7)
ap.add_argument("--md", default=None)
ap.add_argument("--trace", action="store_true")
a = ap.parse_args()
KFS = [int(k) for k in a.kfs.split(",")]
S = a.streams
if a.trace:
    KFS = KFS[:1]

ctx = flvis_amd.Context(0)
sc = LL.scene()
kf0 = torch.from_numpy(np.stack([p[0] for p in sc.kf])).cuda()
kf1 = torch.from_numpy(np.stack([p[1] for p in sc.kf])).cuda()
_, d, c, _ = ctx.orb_detect_and_compute(kf0, cap=1024)
ctx.bow_set_vocabulary(*V.build_vocabulary([d[i, :int(c[i])].cpu().numpy() for i in range(len(sc.kf))], k=6, depth=3))
lc = flvis_amd.LoopCloser(ctx, LL.stereo_cfg(), LL.PARAMS, n_streams=S, max_keyframes=max(KFS))
streams = list(range(S))
n_img = len(sc.kf)
info = flvis_amd.voxel_cloud_info()


def add(k):
    """keyframe k of every sequence: sequence s takes image (k + s) % n_img; lap k // n_img lies half a metre further along x, and every
    sequence in a map frame of its own two metres from the next"""
    idx = torch.tensor([(k + s) % n_img for s in streams], device="cuda")
    T = []
    for s in streams:
        shift = np.array([0.5 * (k // n_img) + 2.0 * s, 0, 0, 0, 0, 0, 1.0])
        T.append(PS.mul7(sc.kf_gt[(k + s) % n_img], PS.inv7(shift)))
    lc.add_keyframes(streams, kf0[idx].contiguous(), kf1[idx].contiguous(), np.array(T))


def timed(f, reps):
    f()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def model_bytes(n, rows, n_out, st, n_clouds):
    """what one call moves, from the kernels: counts and starts; k_mc_keys reads a point and writes point, key and index; a pass reads
    the keys (and the indices for a cloud digit) for its histogram, then reads and writes keys and indices; the output kernels read the
    keys twice (flags, emit), the indices and the points once, and write the rows"""
    keys = 24 * n + 56 * rows + (24 + 8 + 4) * n + 16 * rows
    cloud_passes = 1 if (n_clouds > 1 and st["passes_run"] > 0) else 0
    passes = st["passes_run"] * (8 + 12 + 12) * n + cloud_passes * 4 * n
    out = (8 + 8 + 4 + 24) * n + 16 * n_out
    return keys + passes + out


configs = {"64x1": [[s] for s in streams], "16x4": [streams[4 * g:4 * g + 4] for g in range(S // 4)]}
lines = []
done = 0
for K in KFS:
    while done < K:
        add(done)
        done += 1
    lc.process()
    for name, groups in configs.items():
        for leaf in (0.08, 0.0):
            n_out = lc.map_cloud(groups, leaf=leaf, cap=0)[2]
            cap = int(n_out.max())
            ng = len(groups)
            xyz = torch.empty((ng, cap, 3), dtype=torch.float32, device="cuda")
            npts = torch.empty((ng, cap), dtype=torch.int32, device="cuda")
            ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), np.int32)
            seqs = np.ascontiguousarray([s for g in groups for s in g], np.int32)
            no, nd = np.zeros(ng, np.int64), np.zeros(ng, np.int64)
            fn = lc._lib.flvis_loop_closer_map_cloud
            P = flvis_amd._P

            def call():
                rc = fn(lc._h, ng, P(ptr, C.c_int), P(seqs, C.c_int), leaf, 1, cap, flvis_amd._ptr(xyz), flvis_amd._ptr(npts), P(no, C.c_int64),
                        P(nd, C.c_int64))
                assert rc == 0, rc
            if a.trace:
                for _ in range(5):
                    call()
                continue
            med, lo, hi = timed(call, a.reps)
            st = ctx.voxel_cloud_stats()
            b = model_bytes(st["input_points"], S * K, int(no.sum()), st, ng)
            bound_ms = b / (a.tbps * 1e12) * 1e3
            lines.append(dict(config=name, leaf=leaf, keyframes_per_sequence=K, input_points=st["input_points"], rows_out=int(no.sum()),
                              dropped=int(nd.sum()), ms=med, ms_min=lo, ms_max=hi, passes_run=st["passes_run"], passes_skipped=st["passes_skipped"],
                              workspace_bytes=st["workspace_bytes"], model_bytes=int(b), bound_ms=bound_ms, fraction_of_bound=bound_ms / med))
            print(json.dumps(lines[-1]), flush=True)
    if a.trace:
        continue
    # the route without the call, one sequence: every keyframe and the poses to the host, then the restatement
    t0 = time.perf_counter()
    case, where = MC.closer_case(lc, [0])
    t1 = time.perf_counter()
    want = MC.restate(case, [where[0]], 0.08)
    t2 = time.perf_counter()
    got = lc.map_cloud([[0]], leaf=0.08)
    same = bool(got[2][0] == want["n_out"] and np.array_equal(got[0][0].view(np.uint32), want["xyz"].view(np.uint32)))
    lines.append(dict(config="host route, 1 sequence", leaf=0.08, keyframes_per_sequence=K, fetch_ms=(t1 - t0) * 1e3, restate_ms=(t2 - t1) * 1e3,
                      ms=(t2 - t0) * 1e3, ms_times_streams=(t2 - t0) * 1e3 * S, rows_out=want["n_out"], equals_the_call=same))
    print(json.dumps(lines[-1]), flush=True)

if a.md and lines:
    with open(a.md, "a") as f:
        f.write("| config | leaf | kf/seq | input points | rows out | ms (min .. max) | passes run / skipped | workspace MB | model MB | bound ms | bound / ms |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for l in lines:
            if "passes_run" in l:
                f.write("| %s | %g | %d | %d | %d | %.3f (%.3f .. %.3f) | %d / %d | %.1f | %.1f | %.3f | %.3f |\n" % (
                    l["config"], l["leaf"], l["keyframes_per_sequence"], l["input_points"], l["rows_out"], l["ms"], l["ms_min"], l["ms_max"],
                    l["passes_run"], l["passes_skipped"], l["workspace_bytes"] / 1e6, l["model_bytes"] / 1e6, l["bound_ms"], l["fraction_of_bound"]))
            else:
                f.write("| %s | %g | %d | | %d | %.1f (fetch %.1f + numpy %.1f); x %d sequences = %.0f | | | | | equal bits: %s |\n" % (
                    l["config"], l["leaf"], l["keyframes_per_sequence"], l["rows_out"], l["ms"], l["fetch_ms"], l["restate_ms"], S,
                    l["ms_times_streams"], l["equals_the_call"]))
lc.close()
ctx.close()
