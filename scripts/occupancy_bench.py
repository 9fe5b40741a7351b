#!/usr/bin/env python3
"""The occupancy map from the keyframe log (flvis_keyframe_log_occupancy) and what free space costs over points: --streams synthetic
D435i depth streams with IMU and the local map on, one flvis_run_steps batch of --steps frames with the keyframe log on (the log of
scripts/depth_cloud_bench.py), then per (step, leaf) of steps 7 and 4 and leaves 0.08 and 0.16, z_max 6.5:

 occupancy:   one map per stream over every logged keyframe; time per call (median of --reps after one untimed call that grows the
              workspace; the rows' copy to the host by the Python layer included), and from one more, timed call
              (flvis_hip_depth_cloud_times: it waits behind every stage) the milliseconds of count, emit, sort and reduce, the records,
              records per ray, batches and workspace bytes (flvis_hip_occupancy_stats).
 depth cloud: flvis_keyframe_log_depth_cloud on the same log and sampling in the same process, the two calls alternating: the yardstick.
 hazard:      ONE keyframe at step 1 (a VGA scan: ~300 k rays that all start in one voxel), alone, the same way.
One JSON line; profiles/r29_occupancy.md holds the numbers.

usage: python scripts/occupancy_bench.py [--streams 64] [--steps 75] [--reps 5] [--max-records 0]"""
import argparse
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
    ap.add_argument("--steps", type=int, default=75)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-records", type=int, default=0)
    ap.add_argument("--max-range", type=float, default=3.3)
    args = ap.parse_args()
    S = args.streams
    ypath = os.path.join(tempfile.gettempdir(), "flvis_occupancy_bench_d435.yaml")
    open(ypath, "w").write(synth.D435I_DEPTH_YAML)
    cfg = flvis_amd.load_config(ypath)
    W, H = int(cfg.image_width), int(cfg.image_height)
    trajs = [synth.Trajectory(s) for s in range(S)]
    rnd = synth.Renderer(torch.device("cuda", 0))
    frames, t_prev = [], -0.05
    for f in range(args.steps):
        t = f / synth.FRAME_HZ
        smp = [synth.imu_samples(trajs[s], s, t_prev, t) for s in range(S)]
        t_prev = t
        cnt = np.array([len(x) for x in smp], np.int32)
        blk = np.zeros((S, max(max(len(x) for x in smp), 1), 7))
        for s, x in enumerate(smp):
            blk[s, :len(x)] = x
        i0, i1 = rnd.depth_frame(trajs, t, f, max_range=args.max_range)
        frames.append((i0.clone(), i1.clone(), [t] * S, cnt, blk))
    ctx = flvis_amd.Context(0)
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715)
    trk.keyframe_log_enable(args.steps)
    trk.run_steps(frames, with_local_map=True)
    ctx.synchronize()
    logged = [trk.keyframe_log_info(s)["logged"] for s in range(S)]
    n_kf = sum(logged)
    res = {"streams": S, "steps": args.steps, "width": W, "height": H, "keyframes": n_kf, "keyframes_per_stream_min_max": [min(logged), max(logged)],
           "max_records": args.max_records or 1 << 26, "info": flvis_amd.occupancy_info()}

    def measure(streams, slices, step, leaf):
        kw = dict(step=step, z_min=0.3, z_max=6.5, leaf=leaf, slices=slices)
        occ_cap = int(max(trk.keyframe_log_occupancy(streams, cap=0, max_records=args.max_records, **kw)[3]))
        dc_cap = int(max(trk.keyframe_log_depth_cloud(streams, cap=0, **kw)[2]))
        trk.keyframe_log_occupancy(streams, cap=occ_cap, max_records=args.max_records, **kw)           # (both grow their workspace)
        trk.keyframe_log_depth_cloud(streams, cap=dc_cap, **kw)
        ms_occ, ms_dc = [], []
        for _ in range(args.reps):                                                                      # alternating, in one process
            t0 = time.perf_counter()
            got = trk.keyframe_log_occupancy(streams, cap=occ_cap, max_records=args.max_records, **kw)
            ms_occ.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            dc = trk.keyframe_log_depth_cloud(streams, cap=dc_cap, **kw)
            ms_dc.append(1e3 * (time.perf_counter() - t0))
        ctx.depth_cloud_times(True)
        trk.keyframe_log_occupancy(streams, cap=occ_cap, max_records=args.max_records, **kw)
        st = ctx.occupancy_stats()
        trk.keyframe_log_depth_cloud(streams, cap=dc_cap, **kw)
        dc_stages = ctx.depth_cloud_times(False)
        rays = int(got[4].sum())
        l = np.concatenate(got[1]) if got[1] else np.zeros(0)
        return {"occupancy": {"ms_per_call": round(statistics.median(ms_occ), 3), "ms_min": round(min(ms_occ), 3), "ms_max": round(max(ms_occ), 3),
                              "stage_ms": dict(zip(("count", "emit", "sort", "reduce"), (round(v, 3) for v in st["ms"]))),
                              "records": st["records"], "rays": rays, "records_per_ray": round(st["records"] / max(rays, 1), 1),
                              "dropped_rays": int(got[5].sum()), "batches": got[6], "workspace_bytes": st["workspace_bytes"],
                              "voxels": int(got[3].sum()), "occupied": int((l > 0).sum()), "free": int((l < 0).sum())},
                "depth_cloud": {"ms_per_call": round(statistics.median(ms_dc), 3), "ms_min": round(min(ms_dc), 3), "ms_max": round(max(ms_dc), 3),
                                "stage_ms": {k: round(v, 3) for k, v in dc_stages.items()}, "points": int(dc[2].sum()),
                                "valid_samples": int(dc[4].sum())},
                "occupancy_over_depth_cloud": round(statistics.median(ms_occ) / max(statistics.median(ms_dc), 1e-9), 2)}

    for step in (7, 4):
        for leaf in (0.08, 0.16):
            res["step_%d_leaf_%.2f" % (step, leaf)] = measure(list(range(S)), None, step, leaf)
    res["hazard_one_vga_scan_step_1_leaf_0.08"] = measure([0], [(0, 1)], 1, 0.08)
    del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
