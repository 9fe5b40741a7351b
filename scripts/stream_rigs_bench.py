#!/usr/bin/env python3
"""Mixed rigs at scale: 64 D435i stereo streams with the local map on, images resident in HBM, fed by flvis_run_steps in batches of
10 steps -- once as a uniform batch (every stream on the stock calibration, flvis_tracker_create) and once as a mixed batch (stream s on
synth.rig_variant("d435i_stereo", s % 4), flvis_tracker_create_rigs, each stream rendered with its own rig).  The uniform batch runs
before and after the mixed one (the first tracker of a process has been seen to run slower).  Prints frames/s for all three (one JSON
line).  profiles/r08_stream_rigs.md holds the numbers.

usage: python scripts/stream_rigs_bench.py [steps] [streams]"""
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
    nv = 4

    def cfg_of(k):
        p = os.path.join(tempfile.gettempdir(), "flvis_rigs_bench_%d.yaml" % k)
        open(p, "w").write(synth.rig_variant("d435i_stereo", k)[1])
        return flvis_amd.load_config(p)

    dev = torch.device("cuda", 0)
    trajs = [synth.Trajectory(s) for s in range(S)]
    rnds = [synth.Renderer(dev, rig=synth.rig_variant("d435i_stereo", k)[0]) for k in range(nv)]
    uniform, mixed = [], []
    for f in range(steps):
        t = f / synth.FRAME_HZ
        i0, i1 = rnds[0].stereo_frame(trajs, t, f)
        uniform.append((i0.clone(), i1.clone(), [t] * S))
        m0, m1 = i0.clone(), i1.clone()
        for k in range(1, nv):
            idx = list(range(k, S, nv))
            a, b = rnds[k].stereo_frame([trajs[s] for s in idx], t, f)
            m0[idx], m1[idx] = a, b
        mixed.append((m0, m1, [t] * S))
    cfgs = [cfg_of(k) for k in range(nv)]
    ctx = flvis_amd.Context(0)
    res = {"streams": S, "steps": steps, "rigs": nv}
    for mode in ("uniform", "mixed", "uniform_after"):
        frames = mixed if mode == "mixed" else uniform
        cfg = [cfgs[s % nv] for s in range(S)] if mode == "mixed" else cfgs[0]
        trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715, traj_capacity=steps)
        trk.run_steps(frames[:every], with_local_map=True)  # warm-up batch (first launches, the init frames)
        ctx.synchronize()
        t0 = time.perf_counter()
        for b in range(every, steps, every):
            trk.run_steps(frames[b:b + every], with_local_map=True)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        res[mode + "_frames_per_s"] = round(S * (steps - every) / dt, 1)
        res[mode + "_keyframes"], res[mode + "_ba_runs"] = [int(x.sum()) for x in trk.local_map_counts()]
        res[mode + "_dropped_keyframes"] = trk.dropped_keyframes()
        del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
