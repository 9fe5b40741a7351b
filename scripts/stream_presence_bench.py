#!/usr/bin/env python3
"""Per-stream frame presence at scale: 64 D435i stereo streams with the local map on, images resident in HBM, fed by flvis_run_steps /
flvis_run_steps_present in batches of 10 steps, under five schedules -- the plain entry, all present through the _present entry, two
groups of 32 on alternating steps, 50 % and 25 % of the streams present (random, fixed seed).  Prints, per schedule, ms per step,
present frames/s, keyframes, local-map optimisations and dropped keyframes (one JSON line).  profiles/r09_stream_presence.md holds the
numbers.

usage: python scripts/stream_presence_bench.py [steps] [streams] [schedule,...]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHEDULES = ("plain", "all_present", "alternate_32_32", "random_50", "random_25")


def presence(name, steps, S):
    if name in ("plain", "all_present"):
        return np.ones((steps, S), np.uint8)
    if name == "alternate_32_32":
        k = np.arange(steps)[:, None]
        return ((np.arange(S)[None, :] * 2 // S) == (k % 2)).astype(np.uint8)
    p = {"random_50": 0.5, "random_25": 0.25}[name]
    return (np.random.default_rng(2026).random((steps, S)) < p).astype(np.uint8)


def main():
    import torch
    import flvis_amd
    from flvis_amd import synth
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    names = sys.argv[3].split(",") if len(sys.argv) > 3 else SCHEDULES
    every = 10
    ypath = os.path.join(tempfile.gettempdir(), "flvis_presence_bench_d435.yaml")
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
    res = {"streams": S, "steps": steps, "batch": every}
    for name in names:
        pres = presence(name, steps, S)
        pres[:every] = 1  # warm-up batch: every stream (first launches, the init frames)
        trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715, traj_capacity=steps)
        trk.run_steps(frames[:every], with_local_map=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        for b in range(every, steps, every):
            trk.run_steps(frames[b:b + every], with_local_map=True, present=None if name == "plain" else pres[b:b + every])
        ctx.synchronize()
        dt = time.perf_counter() - t0
        kf, ba = trk.local_map_counts()
        n_present = int(pres[every:].sum())
        res[name] = {"ms_per_step": round(1e3 * dt / (steps - every), 3), "present_frames_per_s": round(n_present / dt, 1),
                     "present_fraction": round(n_present / float(S * (steps - every)), 3), "keyframes": int(kf.sum()),
                     "optimisations": int(ba.sum()), "dropped_keyframes": trk.dropped_keyframes()}
        del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
