#!/usr/bin/env python3
"""Rectification (flvis_hip_rectify) and the dense map on the unrectified stereo rig (flvis_keyframe_log_unrect_stereo_cloud).

 kernel: 752 x 480 pairs of the synthetic EuRoC-like rig, --batch pairs of one stream's two cameras (the batch the log calls rectify at a
         time): ms per call and per pair (median of --reps after one untimed call), the bytes a pair moves (two reads and two writes of
         w * h) against the device-to-device copy bandwidth of a buffer of the batch's size, and beside it flvis_hip_dense_stereo on those
         same rectified pairs (64 disparities, defaults).  The same with the images' cameras interleaved (runs of length 1): what the map
         costs when it is evaluated per image.
 log:    --streams EuRoC-like streams with IMU and the local map on, one flvis_run_steps batch of --steps frames with the keyframe log on,
         then one cloud per stream over its first --keyframes logged keyframes (step 7, leaf --leaf) by
         flvis_keyframe_log_unrect_stereo_cloud -- and flvis_keyframe_log_stereo_cloud on a cam_type 0 log of equal size: the KITTI-like
         rig's yaml at 752 x 480, the same streams, steps and keyframe count (one tracker after the other: a context holds one).
One JSON line; profiles/r28_rectify.md holds the numbers.

usage: python scripts/rectify_bench.py [--batch 64] [--streams 16] [--steps 30] [--keyframes 10] [--leaf 0.08] [--reps 5] [--no-log]"""
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--leaf", type=float, default=0.08)
    ap.add_argument("--keyframes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-log", action="store_true")
    args = ap.parse_args()
    S, B = args.streams, args.batch
    ypath = os.path.join(tempfile.gettempdir(), "flvis_rectify_bench_euroc.yaml")
    open(ypath, "w").write(synth.EUROC_LIKE_YAML)
    cfg = flvis_amd.load_config(ypath)
    W, H = int(cfg.image_width), int(cfg.image_height)
    bf = -cfg.P1[3]

    def cam21(K, D, R, P):
        return list(K) + list(D) + list(R) + [P[0], P[5], P[2], P[6]]
    cams = np.array([cam21(cfg.cam0_intrinsics, cfg.cam0_distortion, cfg.R0, cfg.P0),
                     cam21(cfg.cam1_intrinsics, cfg.cam1_distortion, cfg.R1, cfg.P1)])
    trajs = [synth.Trajectory(s) for s in range(S)]
    dev = torch.device("cuda", 0)
    rnd = synth.Renderer(dev, rig=synth.euroc_rig())
    ctx = flvis_amd.Context(0)
    res = {"width": W, "height": H, "bf": bf, "batch": B}

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

    # ---- the kernel: B pairs as 2 B images, camera 0's first (two runs the host cuts to fill the chip), then interleaved
    n_src = min(S, 8)
    p0, p1 = rnd.stereo_frame(trajs[:n_src], 1.0, frame_idx=5)
    k = (B + n_src - 1) // n_src
    raw = torch.cat([p0.repeat(k, 1, 1)[:B], p1.repeat(k, 1, 1)[:B]]).contiguous()
    pair_bytes = 4 * W * H
    buf = torch.empty(B * pair_bytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        dst.copy_(buf)
    torch.cuda.synchronize()
    copy = 5 * 2 * buf.numel() / (time.perf_counter() - t0) / 1e9
    del buf, dst
    kern = {}
    for name, cam_of in (("grouped", [0] * B + [1] * B), ("interleaved", [0, 1] * B)):
        src = raw if name == "grouped" else raw.view(2, B, H, W).transpose(0, 1).reshape(2 * B, H, W).contiguous()
        med, lo, hi = clock(lambda: ctx.rectify(src, cams, cam_of, want_covered=False), args.reps)
        kern[name] = {"ms_per_call": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "ms_per_pair": round(med / B, 5),
                      "GB_per_s": round(B * pair_bytes / med / 1e6, 1), "copy_GB_per_s": round(copy, 1),
                      "fraction_of_copy": round(B * pair_bytes / med / 1e6 / copy, 4)}
    rect, cov = ctx.rectify(raw, cams, [0] * B + [1] * B)
    ctx.synchronize()
    res["uncovered_share"] = [round(1.0 - float(cov[:B].float().mean()), 6), round(1.0 - float(cov[B:].float().mean()), 6)]
    r0, r1 = rect[:B].contiguous(), rect[B:].contiguous()
    med, lo, hi = clock(lambda: ctx.dense_stereo(r0, r1, bf, 1000.0, n_disp=64), args.reps)
    kern["matcher_on_the_rectified_pairs"] = {"ms_per_call": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                                              "ms_per_pair": round(med / B, 5)}
    kern["rectify_over_matcher"] = round(kern["grouped"]["ms_per_pair"] / kern["matcher_on_the_rectified_pairs"]["ms_per_pair"], 4)
    d, _ = ctx.dense_stereo(r0[:1], r1[:1], bf, 1000.0, n_disp=64)
    d_raw, _ = ctx.dense_stereo(raw[:1], raw[B:B + 1], bf, 1000.0, n_disp=64)
    ctx.synchronize()
    res["valid_share_rectified_raw"] = [round(float((d != 0).float().mean()), 4), round(float((d_raw != 0).float().mean()), 4)]
    res["kernel"] = kern
    del raw, rect, cov, r0, r1
    if args.no_log:
        ctx.close()
        print(json.dumps(res))
        return

    # ---- the log to the cloud, on this rig and on a rectified rig of the same image size
    K = (synth.KITTI_FX, synth.KITTI_FX, W / 2.0, H / 2.0)
    b = synth.KITTI_LIKE_BASELINE
    P0 = [[K[0], 0.0, K[2], 0.0], [0.0, K[1], K[3], 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    P1 = [[K[0], 0.0, K[2], -K[0] * b], [0.0, K[1], K[3], 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    y = synth.KITTI_LIKE_YAML
    for key, val in (("image_width", str(W)), ("image_height", str(H)), ("cam0_intrinsics", synth._vec(K)), ("cam1_intrinsics", synth._vec(K))):
        y = synth._replace_key(y, key, val)
    y = synth._replace_key(y, "cam0_projection_matrix", "\n" + synth._mat44(P0), lines=5)
    y = synth._replace_key(y, "cam1_projection_matrix", "\n" + synth._mat44(P1), lines=5)
    rpath = os.path.join(tempfile.gettempdir(), "flvis_rectify_bench_rect.yaml")
    open(rpath, "w").write(y)
    T_i_c, T01 = np.eye(4), np.eye(4)
    T_i_c[:3, :3] = synth.R_I_C
    T01[0, 3] = b
    zero = (0.0, 0.0, 0.0, 0.0)
    rigs = {"unrect": (cfg, rnd, True), "rect": (flvis_amd.load_config(rpath), synth.Renderer(dev, rig=synth.Rig(W, H, K, zero, K, zero, T_i_c, T01)),
                                                 False)}
    res["log"] = {"streams": S, "steps": args.steps, "leaf": args.leaf}
    streams = list(range(S))
    for name, (c, r, imu) in rigs.items():  # (a context holds one tracker: one rig after the other)
        frames, t_prev = [], -0.05
        for f in range(args.steps):
            t = f / synth.FRAME_HZ
            smp = [synth.imu_samples(trajs[s], s, t_prev, t) if imu else np.zeros((0, 7)) for s in range(S)]
            t_prev = t
            cnt = np.array([len(x) for x in smp], np.int32)
            blk = np.zeros((S, max(max(len(x) for x in smp), 1), 7))
            for s, x in enumerate(smp):
                blk[s, :len(x)] = x
            i0, i1 = r.stereo_frame(trajs, t, f)
            frames.append((i0.clone(), i1.clone(), [t] * S, cnt, blk))
        trk = flvis_amd.Tracker(ctx, c, S, seed_base=0xF1715)
        trk.keyframe_log_enable(args.steps)
        trk.run_steps(frames, with_local_map=True)
        ctx.synchronize()
        del frames
        logged = [trk.keyframe_log_info(s)["logged"] for s in range(S)]
        use = min(args.keyframes, min(logged))
        kw = dict(step=7, z_min=0.3, z_max=10.0, leaf=args.leaf, n_disp=64, slices=[(0, use)] * S)
        fn = trk.keyframe_log_unrect_stereo_cloud if name == "unrect" else trk.keyframe_log_stereo_cloud
        cap = int(max(fn(streams, cap=0, **kw)[2]))
        got = [None]

        def call():
            got[0] = fn(streams, cap=cap, **kw)
        med, lo, hi = clock(call, args.reps)
        res["log"][name] = {"logged_min_max": [min(logged), max(logged)], "keyframes_per_stream_used": use, "keyframes": use * S,
                            "ms_per_call": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                            "us_per_keyframe": round(1e3 * med / max(use * S, 1), 2), "valid_samples": int(got[0][4].sum()),
                            "points": int(got[0][2].sum()), "includes": "the rows' copy to the host by the Python layer"}
        del trk
    res["log"]["rectified_pair_workspace_bytes"] = 2 * min(res["log"]["unrect"]["keyframes"], 64) * W * H
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
