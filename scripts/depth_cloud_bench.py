#!/usr/bin/env python3
"""The dense map from the keyframe log (flvis_keyframe_log_depth_cloud) against the route a caller had without it: --streams synthetic
D435i depth streams with IMU and the local map on, one flvis_run_steps batch of --steps frames with the keyframe log on, then one cloud
per stream over every logged keyframe at 640 x 480, leaf --leaf, steps 1 and 7.

 device: one call for all streams; time per call (median of --reps, after one untimed call that grows the workspace), per keyframe, and
         by stage -- count, keys, sort, rows -- from a timed call (flvis_hip_depth_cloud_times: it waits once more, behind the sort).
         Depth bytes read per second (the count and the key kernel each read every sampled row: at step 1 the whole image twice) against
         the device-to-device copy bandwidth of a buffer of the log's size.
 host:   per keyframe flvis_keyframe_log_get to the host, numpy back-projection, upload of 24 bytes per valid sample, then ONE
         flvis_hip_voxel_cloud over all rows -- timed over --host-streams streams (it is slow), reported per keyframe.
One JSON line; profiles/r25_depth_cloud.md holds the numbers.

usage: python scripts/depth_cloud_bench.py [--streams 64] [--steps 75] [--leaf 0.08] [--reps 5] [--host-streams 4]"""
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
    ap.add_argument("--leaf", type=float, default=0.08)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-streams", type=int, default=4)
    ap.add_argument("--max-range", type=float, default=3.3)
    args = ap.parse_args()
    S = args.streams
    ypath = os.path.join(tempfile.gettempdir(), "flvis_depth_cloud_bench_d435.yaml")
    open(ypath, "w").write(synth.D435I_DEPTH_YAML)
    cfg = flvis_amd.load_config(ypath)
    W, H = int(cfg.image_width), int(cfg.image_height)
    cam = [cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6], cfg.depth_factor]
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
    res = {"streams": S, "steps": args.steps, "leaf": args.leaf, "width": W, "height": H, "keyframes": n_kf,
           "keyframes_per_stream_min_max": [min(logged), max(logged)]}
    # the copy bandwidth of a buffer as large as the logged depth images
    buf = torch.empty(max(n_kf, 1) * W * H * 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        dst.copy_(buf)
    torch.cuda.synchronize()
    res["copy_GB_per_s"] = round(5 * 2 * buf.numel() / (time.perf_counter() - t0) / 1e9, 1)      # read + write
    del buf, dst
    streams = list(range(S))
    for step in (1, 7):
        kw = dict(step=step, z_min=0.3, z_max=10.0, leaf=args.leaf)
        cap = int(max(trk.keyframe_log_depth_cloud(streams, cap=0, **kw)[2]))
        trk.keyframe_log_depth_cloud(streams, cap=cap, **kw)                               # (grows the workspace)
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = trk.keyframe_log_depth_cloud(streams, cap=cap, **kw)
            ms.append(1e3 * (time.perf_counter() - t0))
        ctx.depth_cloud_times(True)
        t0 = time.perf_counter()
        trk.keyframe_log_depth_cloud(streams, cap=cap, **kw)
        timed_ms = 1e3 * (time.perf_counter() - t0)
        stages = ctx.depth_cloud_times(False)
        rows = len(range(0, H, step))
        read = 2 * n_kf * rows * W * 2                                                     # whole sampled rows, by two kernels
        med = statistics.median(ms)
        res["device_step_%d" % step] = {
            "ms_per_call": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "us_per_keyframe": round(1e3 * med / max(n_kf, 1), 2),
            "includes": "the rows' copy to the host by the Python layer", "valid_samples": int(got[4].sum()), "points": int(got[2].sum()),
            "stage_ms": {k: round(v, 3) for k, v in stages.items()}, "timed_call_ms": round(timed_ms, 3),
            "depth_GB_per_s_count": round(read / 2 / max(stages["count"], 1e-9) / 1e6, 1),
            "depth_GB_per_s_keys": round(read / 2 / max(stages["keys"], 1e-9) / 1e6, 1),
            "sort": ctx.voxel_cloud_stats()}
        # ---- the route without the call
        hs = list(range(min(args.host_streams, S)))
        us = np.arange(0, W, step, dtype=np.float64)
        vs = np.arange(0, H, step, dtype=np.float64)
        U, V = np.meshgrid(us, vs)
        t0 = time.perf_counter()
        rows_p, rows_T = [], []
        t_get = t_np = 0.0
        for s in hs:
            for k in range(logged[s]):
                t1 = time.perf_counter()
                m = trk.keyframe_log_get(s, k)
                t2 = time.perf_counter()
                z = (m["img1"][::step, ::step].astype(np.float64) / cam[4]).astype(np.float32).astype(np.float64)
                ok = (z >= 0.3) & (z <= 10.0)
                rows_p.append(np.stack([((U - cam[2]) * z / cam[0])[ok], ((V - cam[3]) * z / cam[1])[ok], z[ok]], axis=1))
                rows_T.append(m["pose7"])
                t_get += t2 - t1
                t_np += time.perf_counter() - t2
        n_host = len(rows_p)
        pcap = max([len(r) for r in rows_p] + [1])
        p3 = np.zeros((max(n_host, 1), pcap, 3))
        for i, r in enumerate(rows_p):
            p3[i, :len(r)] = r
        t1 = time.perf_counter()
        d_p3 = torch.from_numpy(p3).cuda()
        d_cnt = torch.from_numpy(np.array([len(r) for r in rows_p] + ([0] if not rows_p else []), np.int32)).cuda()
        d_T = torch.from_numpy(np.array(rows_T + ([[0, 0, 0, 0, 0, 0, 1.0]] if not rows_T else []), np.float64)).cuda()
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t1
        clouds, at = [], 0
        for s in hs:
            clouds.append([(at, logged[s])])
            at += logged[s]
        t1 = time.perf_counter()
        hv = ctx.voxel_cloud(d_p3, d_cnt, d_T, clouds, leaf=args.leaf, cap=cap)
        t_vox = time.perf_counter() - t1
        total = time.perf_counter() - t0
        same = all(hv[0][i].tobytes() == got[0][s].tobytes() for i, s in enumerate(hs))
        res["host_step_%d" % step] = {
            "streams": len(hs), "keyframes": n_host, "us_per_keyframe": round(1e6 * total / max(n_host, 1), 1),
            "us_per_keyframe_by_part": {"keyframe_log_get": round(1e6 * t_get / max(n_host, 1), 1), "numpy": round(1e6 * t_np / max(n_host, 1), 1),
                                        "upload": round(1e6 * t_up / max(n_host, 1), 1), "voxel_cloud": round(1e6 * t_vox / max(n_host, 1), 1)},
            "same_bits_as_the_device_call": bool(same)}
    del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
