#!/usr/bin/env python3
"""What the local map's map-cloud record costs the batched tracker, and what a fetch costs: 64 synthetic D435i stereo streams with IMU and
the local map on, images resident in HBM, fed by flvis_run_steps in batches of 10 steps.  Legs in one session, each on a new tracker over
the same frames: record off / on / off / on (the off legs are the launch sequence of a tracker that never heard of the record; in the on legs a lane's local-map launches run one behind
the other with an append kernel behind each).  An
untimed pre-roll brings every stream's window to its steady state; then every batch is timed and the leg's rate is the median over
its batches.  Behind each "on" leg the fetch of all streams is timed in both modes at leaf 0 and 0.08 (median of --reps calls, the
rows staying on the device), and the record's counters are summed.  One JSON line; profiles/r22_local_map_cloud.md holds the numbers.

usage: python scripts/lm_cloud_bench.py [--streams 64] [--preroll 110] [--steps 100] [--reps 5] [--max-points 65536]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import flvis_amd
    from flvis_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--preroll", type=int, default=110)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-points", type=int, default=1 << 16)
    args = ap.parse_args()
    S, every = args.streams, 10
    total = args.preroll + args.steps
    ypath = os.path.join(tempfile.gettempdir(), "flvis_lm_cloud_bench_d435.yaml")
    open(ypath, "w").write(synth.D435I_STEREO_YAML)
    cfg = flvis_amd.load_config(ypath)
    trajs = [synth.Trajectory(s) for s in range(S)]
    rnd = synth.Renderer(torch.device("cuda", 0))
    frames, t_prev = [], -0.05
    for f in range(total):
        t = f / synth.FRAME_HZ
        smp = [synth.imu_samples(trajs[s], s, t_prev, t) for s in range(S)]
        t_prev = t
        cnt = np.array([len(x) for x in smp], np.int32)
        blk = np.zeros((S, max(max(len(x) for x in smp), 1), 7))
        for s, x in enumerate(smp):
            blk[s, :len(x)] = x
        i0, i1 = rnd.stereo_frame(trajs, t, f)
        frames.append((i0.clone(), i1.clone(), [t] * S, cnt, blk))
    ctx = flvis_amd.Context(0)
    res = {"streams": S, "preroll": args.preroll, "steps": args.steps, "batch": every, "max_points": args.max_points, "legs": []}
    for leg, on in enumerate((False, True, False, True)):
        trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715, traj_capacity=total)
        if on:
            trk.local_map_cloud_enable(args.max_points)
        trk.run_steps(frames[:args.preroll], with_local_map=True)
        ctx.synchronize()
        rates = []
        for b in range(args.preroll, total, every):
            t0 = time.perf_counter()
            trk.run_steps(frames[b:b + every], with_local_map=True)
            ctx.synchronize()
            rates.append(S * len(frames[b:b + every]) / (time.perf_counter() - t0))
        kf, ba = trk.local_map_counts()
        out = {"record": "on" if on else "off", "frames_per_s_median": round(statistics.median(rates), 1),
               "frames_per_s_min": round(min(rates), 1), "frames_per_s_max": round(max(rates), 1), "ba_runs": int(ba.sum()),
               "dropped_keyframes": trk.dropped_keyframes()}
        if on:
            info = [trk.local_map_cloud_info(s) for s in range(S)]
            out["recorded_points"] = sum(i["points"] for i in info)
            out["recorded_runs"] = sum(i["runs"] for i in info)
            out["dropped_runs"] = sum(i["dropped"] for i in info)
            fetch = {}
            for mode in ("all", "latest"):
                for leaf in (0.0, 0.08):
                    n_out = trk.local_map_cloud(range(S), mode, leaf=leaf, cap=0)[2]
                    cap = int(max(n_out.max(), 1))
                    xyz = torch.empty((S, cap, 3), dtype=torch.float32, device="cuda")
                    npts = torch.empty((S, cap), dtype=torch.int32, device="cuda")
                    arr = np.arange(S, dtype=np.int32)
                    no, nd = np.zeros(S, np.int64), np.zeros(S, np.int64)
                    fn = trk.lib.flvis_local_map_cloud
                    ms = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        rc = fn(ctx._h, S, arr.ctypes.data_as(C.POINTER(C.c_int)), 0 if mode == "all" else 1, float(leaf), 1, cap,
                                C.c_void_p(xyz.data_ptr()), C.c_void_p(npts.data_ptr()), None, no.ctypes.data_as(C.POINTER(C.c_int64)),
                                nd.ctypes.data_as(C.POINTER(C.c_int64)))
                        ms.append((time.perf_counter() - t0) * 1e3)
                        ctx._check(rc, "local_map_cloud")
                    fetch["%s_leaf_%g" % (mode, leaf)] = {"ms_median": round(statistics.median(ms), 3), "rows": int(no.sum())}
            out["fetch"] = fetch
        res["legs"].append(out)
        del trk
    off = [l["frames_per_s_median"] for l in res["legs"] if l["record"] == "off"]
    on = [l["frames_per_s_median"] for l in res["legs"] if l["record"] == "on"]
    res["off_median"], res["on_median"] = round(statistics.mean(off), 1), round(statistics.mean(on), 1)
    res["off_spread"] = round(max(off) - min(off), 1)
    res["on_minus_off_percent"] = round(100.0 * (res["on_median"] - res["off_median"]) / res["off_median"], 3)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
