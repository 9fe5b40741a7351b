#!/usr/bin/env python3
"""What the keyframe log costs the batched tracker, and what it saves the loop closer: 64 synthetic D435i stereo streams with IMU and the
local map on, images resident in HBM.

 1. flvis_run_steps in batches of --batch steps, log off / on / off / on, each leg on a new tracker over the same frames after an
    untimed pre-roll; the log's capacity holds a batch (it is cleared, untimed, between batches).  A leg's rate is the median over its
    batches.  With the logged keyframes per step: the bytes one k_kf_log_append launch copies (its time comes from a kernel trace of
    this script: rocprofv3 --kernel-trace --stats).
 2. tracker + local map + loop closing over the timed frames, two ways:
      log:  run_steps per batch, then flvis_loop_closer_add_logged (process on) and flvis_keyframe_log_clear;
      host: the only way without the log -- one flvis_image_feed per frame with its outputs, flvis_get_keyframe_msg for every stream that
            made a keyframe, flvis_loop_closer_add_keyframes_host + process per frame.
    Reported: frames/s end to end, and the closer's intake per keyframe (log: add_logged without process over its keyframes; host:
    get_keyframe_msg + add_keyframes_host per keyframe).
One JSON line; profiles/r23_keyframe_log.md holds the numbers.

usage: python scripts/keyframe_log_bench.py [--streams 64] [--preroll 60] [--steps 60] [--batch 10] [--host-steps 20]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LC_PRM = dict(lcKFStart=25, lcKFDist=18, lcKFMaxDist=50, lcKFLast=20, lcNKFClosest=2, ratioMax=0.5, ratioRansac=0.5, minPts=20, minScore=0.12)


def main():
    import numpy as np
    import torch
    import flvis_amd
    from flvis_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--preroll", type=int, default=60)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--host-steps", type=int, default=20, help="timed frames of the host way (it is slow)")
    ap.add_argument("--skip-closer", action="store_true")
    ap.add_argument("--host-only", action="store_true", help="only the host way of part 2 (runs on a library without the log)")
    args = ap.parse_args()
    S, every = args.streams, args.batch
    total = args.preroll + args.steps
    ypath = os.path.join(tempfile.gettempdir(), "flvis_kf_log_bench_d435.yaml")
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
    px = int(cfg.image_width) * int(cfg.image_height)
    kf_bytes = 2 * px + 264 + 1024 * 48          # two mono8 images + the payload's header and full arrays (an upper bound: lm_count <= 1024)
    res = {"streams": S, "preroll": args.preroll, "steps": args.steps, "batch": every, "legs": []}

    def make(on, cap=None):
        trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715)
        if on:
            trk.keyframe_log_enable(cap or every)
        trk.run_steps(frames[:args.preroll], with_local_map=True)
        ctx.synchronize()
        if on:
            trk.keyframe_log_clear(range(S))
        return trk

    # ---- 1. the tracker alone
    for on in (() if args.host_only else (False, True, False, True)):
        trk = make(on)
        rates, logged, dropped = [], 0, 0
        for b in range(args.preroll, total, every):
            t0 = time.perf_counter()
            trk.run_steps(frames[b:b + every], with_local_map=True)
            ctx.synchronize()
            rates.append(S * len(frames[b:b + every]) / (time.perf_counter() - t0))
            if on:
                info = [trk.keyframe_log_info(s) for s in range(S)]
                logged += sum(i["logged"] for i in info)
                dropped += sum(i["dropped"] for i in info)
                trk.keyframe_log_clear(range(S))
        out = {"log": "on" if on else "off", "frames_per_s_median": round(statistics.median(rates), 1), "frames_per_s_min": round(min(rates), 1),
               "frames_per_s_max": round(max(rates), 1), "dropped_queue_keyframes": trk.dropped_keyframes()}
        if on:
            out.update(logged_keyframes=logged, dropped_keyframes=dropped, keyframes_per_launch=round(logged / args.steps, 2),
                       bytes_per_launch=int(kf_bytes * logged / args.steps))
        res["legs"].append(out)
        del trk
    if res["legs"]:
        off = [l["frames_per_s_median"] for l in res["legs"] if l["log"] == "off"]
        on = [l["frames_per_s_median"] for l in res["legs"] if l["log"] == "on"]
        res["off_median"], res["on_median"] = round(statistics.mean(off), 1), round(statistics.mean(on), 1)
        res["off_spread"] = round(max(off) - min(off), 1)
        res["on_minus_off_percent"] = round(100.0 * (res["on_median"] - res["off_median"]) / res["off_median"], 3)

    # ---- 2. with the loop closer
    if not args.skip_closer:
        maxkf = args.preroll + args.steps + 8
        # a vocabulary trained on the device from the descriptors of one frame's images
        _, d, c, _ = ctx.orb_detect_and_compute(frames[args.preroll][0][:min(S, 16)].contiguous(), cap=1024)
        voc = ctx.voc_train(d, c, k=8, L=3)
        ctx.bow_set_vocabulary(*voc.arrays)
        # through the log
        def log_way():
            trk = make(True)
            lc = flvis_amd.LoopCloser(ctx, cfg, LC_PRM, n_streams=S, max_keyframes=maxkf)
            n_kf, t_add = 0, 0.0
            t0 = time.perf_counter()
            last = range(args.preroll, total, every)[-1]
            for b in range(args.preroll, total, every):
                trk.run_steps(frames[b:b + every], with_local_map=True)
                t1 = time.perf_counter()
                rounds = lc.add_logged(process=True)
                t_add += time.perf_counter() - t1
                n_kf += sum(e["kf_curr"] >= 0 for r in rounds for e in r)
                if b != last:
                    trk.keyframe_log_clear(range(S))
            ctx.synchronize()
            dt = time.perf_counter() - t0
            res["closer_log"] = {"frames_per_s": round(S * args.steps / dt, 1), "keyframes": n_kf,
                                 "add_and_process_ms_per_keyframe": round(1e3 * t_add / max(n_kf, 1), 4)}
            # the intake alone: the last batch's log once more, into a new closer, without process
            lc.close()
            lc = flvis_amd.LoopCloser(ctx, cfg, LC_PRM, n_streams=S, max_keyframes=maxkf)
            n_in = sum(trk.keyframe_log_info(s)["logged"] for s in range(S))
            t1 = time.perf_counter()
            lc.add_logged(process=False)
            res["closer_log"]["intake_ms_per_keyframe"] = round(1e3 * (time.perf_counter() - t1) / max(n_in, 1), 4)
            res["closer_log"]["intake_keyframes"] = n_in
            lc.close()
            del trk
        if not args.host_only:
            log_way()
        # through the host
        hs = min(args.host_steps, args.steps)
        trk = make(False)
        lc = flvis_amd.LoopCloser(ctx, cfg, LC_PRM, n_streams=S, max_keyframes=maxkf)
        n_kf, t_in = 0, 0.0
        t0 = time.perf_counter()
        for i0, i1, ts, cnt, blk in frames[args.preroll:args.preroll + hs]:
            for s in range(S):
                if cnt[s]:
                    trk.imu_feed_flvis(s, blk[s, :cnt[s]])
            out = trk.image_feed(i0, i1, ts, want_out=True, with_local_map=True)
            st = [s for s in range(S) if out[s]["new_keyframe"]]
            if not st:
                continue
            t1 = time.perf_counter()
            msgs = [trk.keyframe_msg(s) for s in st]
            lc.add_keyframes_host(st, [m["img0"] for m in msgs], [m["img1"] for m in msgs], [m["pose7"] for m in msgs])
            t_in += time.perf_counter() - t1
            lc.process()
            n_kf += len(st)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        res["closer_host"] = {"frames": hs, "frames_per_s": round(S * hs / dt, 1), "keyframes": n_kf,
                              "intake_ms_per_keyframe": round(1e3 * t_in / max(n_kf, 1), 4),
                              "bytes_over_pcie_per_keyframe": 2 * 2 * px}
        lc.close()
        del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
