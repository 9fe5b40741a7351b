#!/usr/bin/env python3
"""Dense stereo (flvis_hip_dense_stereo) and the dense map on stereo rigs (flvis_keyframe_log_stereo_cloud).

 kernel: 640 x 480 pairs of the synthetic D435i stereo rig (64 streams rendered once, tiled to the batch), defaults but n_disp 64 and 128,
         batches of 1, 64 and 1024 pairs, both outputs: ms per call (median of --reps after one untimed call that grows the workspace) and
         per pair.  A pair should move 2 reads of w * h bytes and two 2-byte outputs; the rate that makes against the device-to-device copy
         bandwidth of a buffer of the batch's size (what the project's roofline uses).  The numpy restatement's seconds per pair (one
         64-row band, scaled) for scale only.
 log:    --streams stereo streams with IMU and the local map on, one flvis_run_steps batch of --steps frames with the keyframe log on, then
         one cloud per stream over every logged keyframe, leaf --leaf, steps 7 and 1 -- beside profiles/r25_depth_cloud.md's depth-rig
         call -- and the context's stereo workspace.
One JSON line; profiles/r27_dense_stereo.md holds the numbers.

usage: python scripts/dense_stereo_bench.py [--streams 64] [--steps 75] [--leaf 0.08] [--reps 5] [--no-log]"""
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
    ap.add_argument("--no-log", action="store_true")
    ap.add_argument("--restatement", action="store_true")
    args = ap.parse_args()
    S = args.streams
    ypath = os.path.join(tempfile.gettempdir(), "flvis_dense_stereo_bench_d435.yaml")
    open(ypath, "w").write(synth.D435I_STEREO_YAML)
    cfg = flvis_amd.load_config(ypath)
    W, H = int(cfg.image_width), int(cfg.image_height)
    bf = -cfg.P1[3]
    trajs = [synth.Trajectory(s) for s in range(S)]
    rnd = synth.Renderer(torch.device("cuda", 0))
    ctx = flvis_amd.Context(0)
    res = {"width": W, "height": H, "bf": bf}

    def clock(fn, reps):
        fn()
        ctx.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms), min(ms), max(ms)

    # ---- the kernel
    p0, p1 = rnd.stereo_frame(trajs[:min(S, 64)], 1.0, frame_idx=5)
    pair_bytes = 2 * W * H + 2 * 2 * W * H
    res["bytes_per_pair"] = pair_bytes
    kern = {}
    for batch in (1, 64, 1024):
        k = (batch + len(p0) - 1) // len(p0)
        i0, i1 = p0.repeat(k, 1, 1)[:batch].contiguous(), p1.repeat(k, 1, 1)[:batch].contiguous()
        buf = torch.empty(batch * pair_bytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(buf)
        dst.copy_(buf)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            dst.copy_(buf)
        torch.cuda.synchronize()
        copy = 5 * 2 * buf.numel() / (time.perf_counter() - t0) / 1e9
        del buf, dst
        for nd in (64, 128):
            for lr in (1, -1):
                med, lo, hi = clock(lambda: ctx.dense_stereo(i0, i1, bf, 1000.0, n_disp=nd, lr_tol=lr), args.reps)
                kern["batch_%d_ndisp_%d%s" % (batch, nd, "" if lr >= 0 else "_no_lr")] = {
                    "ms_per_call": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "ms_per_pair": round(med / batch, 4),
                    "GB_per_s": round(batch * pair_bytes / med / 1e6, 1), "copy_GB_per_s": round(copy, 1),
                    "fraction_of_copy": round(batch * pair_bytes / med / 1e6 / copy, 4)}
        d, z = ctx.dense_stereo(i0[:1], i1[:1], bf, 1000.0)
        ctx.synchronize()
        res["valid_share"] = round(float((d != 0).float().mean()), 4)
        del i0, i1
    res["kernel"] = kern
    if args.restatement:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _dense_stereo as DS
        a, b = p0[0].cpu().numpy()[208:272], p1[0].cpu().numpy()[208:272]
        t0 = time.perf_counter()
        DS.restate_one(a, b, bf, 1000.0, DS.params())
        res["numpy_restatement_s_per_pair"] = round((time.perf_counter() - t0) * H / 64, 2)
    if args.no_log:
        ctx.close()
        print(json.dumps(res))
        return

    # ---- the log to the cloud
    frames, t_prev = [], -0.05
    for f in range(args.steps):
        t = f / synth.FRAME_HZ
        smp = [synth.imu_samples(trajs[s], s, t_prev, t) for s in range(S)]
        t_prev = t
        cnt = np.array([len(x) for x in smp], np.int32)
        blk = np.zeros((S, max(max(len(x) for x in smp), 1), 7))
        for s, x in enumerate(smp):
            blk[s, :len(x)] = x
        i0, i1 = rnd.stereo_frame(trajs, t, f)
        frames.append((i0.clone(), i1.clone(), [t] * S, cnt, blk))
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715)
    trk.keyframe_log_enable(args.steps)
    trk.run_steps(frames, with_local_map=True)
    ctx.synchronize()
    logged = [trk.keyframe_log_info(s)["logged"] for s in range(S)]
    n_kf = sum(logged)
    res["log"] = {"streams": S, "steps": args.steps, "leaf": args.leaf, "keyframes": n_kf, "keyframes_per_stream_min_max": [min(logged), max(logged)]}
    streams = list(range(S))
    for step in (7, 1):
        kw = dict(step=step, z_min=0.3, z_max=10.0, leaf=args.leaf)
        cap = int(max(trk.keyframe_log_stereo_cloud(streams, cap=0, **kw)[2]))
        got = [None]

        def call():
            got[0] = trk.keyframe_log_stereo_cloud(streams, cap=cap, **kw)
        med, lo, hi = clock(call, args.reps)
        nu, nv = len(range(0, W, step)), len(range(0, H, step))
        res["log"]["step_%d" % step] = {
            "ms_per_call": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "us_per_keyframe": round(1e3 * med / max(n_kf, 1), 2),
            "includes": "the rows' copy to the host by the Python layer", "valid_samples": int(got[0][4].sum()), "points": int(got[0][2].sum()),
            "stereo_workspace_bytes": {"samples": 2 * n_kf * nu * nv, "lists": 20 * n_kf, "left_right_map": 2 * min(n_kf, 64) * W * H},
            "cloud_workspace": ctx.voxel_cloud_stats()}
    del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
