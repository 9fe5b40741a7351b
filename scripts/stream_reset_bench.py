#!/usr/bin/env python3
"""Per-stream reset at scale: 64 D435i stereo streams with the local map on, images resident in HBM, fed by flvis_run_steps in batches
of 10 steps, in two modes -- no reset, and one stream reset (flvis_reset_streams) between every two batches, in rotation.  The
no-reset mode runs before and after the reset mode (the first tracker of a process has been seen to run slower).  Prints frames/s
for all three (one JSON line).  profiles/r07_stream_reset.md holds the numbers.

usage: python scripts/stream_reset_bench.py [steps] [streams]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import flvis_amd
    from flvis_amd import synth
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    every = 10
    ypath = os.path.join(tempfile.gettempdir(), "flvis_reset_bench_d435.yaml")
    open(ypath, "w").write(synth.D435I_STEREO_YAML)
    cfg = flvis_amd.load_config(ypath)
    trajs = [synth.Trajectory(s) for s in range(S)]
    rnd = synth.Renderer(torch.device("cuda", 0))
    frames = []
    for f in range(steps):
        t = f / synth.FRAME_HZ
        i0, i1 = rnd.stereo_frame(trajs, t, f)
        frames.append((i0.clone(), i1.clone(), [t] * S))
    ctx = flvis_amd.Context(0)
    res = {"streams": S, "steps": steps, "reset_every": every}
    for mode in ("no_reset", "reset", "no_reset_after"):
        trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715, traj_capacity=steps)
        trk.run_steps(frames[:every], with_local_map=True)  # warm-up batch (first launches, the init frames)
        ctx.synchronize()
        t0 = time.perf_counter()
        nxt = 0
        for b in range(every, steps, every):
            if mode == "reset":
                trk.reset_streams([nxt])
                nxt = (nxt + 1) % S
            trk.run_steps(frames[b:b + every], with_local_map=True)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        res[mode + "_frames_per_s"] = round(S * (steps - every) / dt, 1)
        res[mode + "_dropped_keyframes"] = trk.dropped_keyframes()
        del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
