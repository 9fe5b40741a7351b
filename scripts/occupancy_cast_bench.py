#!/usr/bin/env python3
"""Queries against occupancy maps (flvis_hip_occupancy_cast) and what a lookup per cell costs over a walk that looks nothing up: the log
of scripts/occupancy_bench.py (--streams synthetic D435i depth streams with IMU and the local map on, one flvis_run_steps batch of
--steps frames with the keyframe log on), one occupancy map per stream at step 7, z_max 6.5, at leaf 0.08 and at leaf 0.16; the maps
stay on the device.  Then, per leaf, three workloads over all maps in ONE call each:

 rays:    per map the rays of that stream's last keyframe at step 7 -- the sensor's own rays, camera to sample
 bundle:  per map 4096 segments of 2 m from the last keyframe's position in directions on a fixed (Fibonacci) lattice: a planner's bundle
 lookup:  per map 65 536 point lookups (p == o): points on the rays at parameters 0 .. 1.2 on a fixed lattice
 merged:  ONE map of the rows of all maps (the union of their keys) and the rays of all streams
 tiled:   ONE map of --tiles copies of the merged map, copy i moved by 2048 i cells along y -- the synthetic streams all look at one
          scene, so their union is no larger than one of them; this is the row count of a fleet's merged map with the local structure
          of a real one -- and the same rays, ray j moved into copy j % tiles

For each, with the line directory and with the plain search (flvis_hip_occupancy_cast_lookup): ms per call (host clock around the C call
on device arrays, which ends in the counts' copy; median of --reps after one untimed call), and from one more, timed call
(flvis_hip_depth_cloud_times: it waits behind the index build) the milliseconds of index build and walk, the cells tested
(flvis_hip_occupancy_cast_stats), queries/s and cells/s over the walk, the queries per status.  The two lookups take turns, and their six
outputs are compared byte for byte.
The yardstick is k_oc_emit of the same process: it walks the same kind of rays and looks nothing up; its records/s are from the emit stage
of one timed flvis_keyframe_log_occupancy per leaf, and every cells/s above is also given as a fraction of it.
One JSON line; profiles/r30_occupancy_cast.md holds the numbers.

usage: python scripts/occupancy_cast_bench.py [--streams 64] [--steps 75] [--reps 5]"""
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
    from flvis_amd import synth, traj_io
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=75)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-range", type=float, default=3.3)
    ap.add_argument("--bundle", type=int, default=4096)
    ap.add_argument("--lookups", type=int, default=65536)
    ap.add_argument("--tiles", type=int, default=128)
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
    lib = ctx._lib
    trk = flvis_amd.Tracker(ctx, cfg, S, seed_base=0xF1715)
    trk.keyframe_log_enable(args.steps)
    trk.run_steps(frames, with_local_map=True)
    ctx.synchronize()
    logged = [trk.keyframe_log_info(s)["logged"] for s in range(S)]
    assert min(logged) >= 1, "every stream logged a keyframe"
    res = {"streams": S, "steps": args.steps, "width": W, "height": H, "keyframes": sum(logged), "reps": args.reps}

    # ---- the queries, made on the host once: the last keyframe's rays (the dense calls' sampling and back-projection), the bundle, the points
    fx, fy, cx, cy, df = cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6], cfg.depth_factor
    v, u = np.meshgrid(np.arange(0, H, 7), np.arange(0, W, 7), indexing="ij")
    k = np.arange(args.bundle) + 0.5
    polar, turn = np.arccos(1 - 2 * k / args.bundle), np.pi * (1 + 5 ** 0.5) * k
    lattice = np.stack([np.cos(turn) * np.sin(polar), np.sin(turn) * np.sin(polar), np.cos(polar)], axis=1)
    rays, bundle, points = [], [], []
    for s in range(S):
        e = trk.keyframe_log_get(s, logged[s] - 1)
        p7 = np.asarray(e["pose7"], np.float64)
        R = traj_io.quat_to_rot(p7[6], p7[3], p7[4], p7[5])
        z = (e["img1"][v, u].astype(np.float64) / df).astype(np.float32).astype(np.float64)
        ok = (z >= 0.3) & (z <= 6.5)
        p_c = np.stack([(u[ok] - cx) * z[ok] / fx, (v[ok] - cy) * z[ok] / fy, z[ok]], axis=1)
        p = (p_c - p7[:3]) @ R
        o = np.broadcast_to(-p7[:3] @ R, p.shape)
        rays.append(np.concatenate([o, p], axis=1))
        bundle.append(np.concatenate([np.broadcast_to(o[:1], lattice.shape), o[:1] + 2.0 * lattice], axis=1))
        j = np.arange(args.lookups)
        pt = o[j % len(o)] + ((j * 0.6180339887498949) % 1.0 * 1.2)[:, None] * (p[j % len(p)] - o[j % len(o)])
        points.append(np.concatenate([pt, pt], axis=1))
    work = {"rays": rays, "bundle": bundle, "lookup": points}

    def measure(key, lo, cap, n_rows, leaf, segs):
        S = len(n_rows)
        qptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(x) for x in segs])]), np.int32)
        nq = int(qptr[-1])
        seg = torch.from_numpy(np.ascontiguousarray(np.concatenate(segs))).cuda()
        kinds = (torch.int32, torch.int32, torch.int64, torch.int32, torch.float32, torch.float64)
        outs = {plain: [torch.zeros(nq, dtype=t, device="cuda") for t in kinds] for plain in (False, True)}
        counts = np.zeros((S, 5), np.int64)
        prm = flvis_amd.occupancy_cast_params()

        def call(plain):
            ctx.occupancy_cast_lookup(plain=plain)
            t0 = time.perf_counter()
            rc = lib.flvis_hip_occupancy_cast(ctx._h, S, key.data_ptr(), lo.data_ptr(), cap, n_rows.ctypes.data_as(C.c_void_p), leaf, C.byref(prm),
                                              seg.data_ptr(), qptr.ctypes.data_as(C.c_void_p), *[o.data_ptr() for o in outs[plain]],
                                              counts.ctypes.data_as(C.c_void_p))
            ms = 1e3 * (time.perf_counter() - t0)
            ctx._check(rc, "occupancy_cast")
            return ms

        call(False), call(True)                                              # (both grow the workspace)
        ms = {False: [], True: []}
        for _ in range(args.reps):                                           # the two lookups take turns
            for plain in (False, True):
                ms[plain].append(call(plain))
        out = {"queries": nq}
        for plain, name in ((False, "line_directory"), (True, "plain_search")):
            ctx.depth_cloud_times(True)
            call(plain)
            st = ctx.occupancy_cast_stats()
            ctx.depth_cloud_times(False)
            build, walk = st["ms"]
            out[name] = {"ms_per_call": round(statistics.median(ms[plain]), 3), "ms_min": round(min(ms[plain]), 3), "ms_max": round(max(ms[plain]), 3),
                         "index_build_ms": round(build, 3), "walk_ms": round(walk, 3), "cells": st["cells"],
                         "queries_per_s_walk": round(nq / max(walk, 1e-9) * 1e3), "cells_per_s_walk": round(st["cells"] / max(walk, 1e-9) * 1e3),
                         "cells_per_s_call": round(st["cells"] / max(statistics.median(ms[plain]), 1e-9) * 1e3),
                         "index_bytes": st["index_bytes"], "workspace_bytes": st["workspace_bytes"]}
        out["status_counts"] = dict(zip(flvis_amd.OCCUPANCY_CAST_STATUS, (int(c) for c in counts.sum(axis=0))))
        out["cells_per_query"] = round(out["line_directory"]["cells"] / max(nq, 1), 2)
        out["same_bits"] = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(outs[False], outs[True]))
        ctx.occupancy_cast_lookup()
        return out

    for leaf in (0.08, 0.16):
        kw = dict(step=7, z_min=0.3, z_max=6.5, leaf=leaf)
        keys, l = trk.keyframe_log_occupancy(list(range(S)), centres=False, **kw)[:2]
        ctx.depth_cloud_times(True)
        trk.keyframe_log_occupancy(list(range(S)), centres=False, **kw)      # the yardstick: this call's emit stage
        st = ctx.occupancy_stats()
        ctx.depth_cloud_times(False)
        emit = st["records"] / max(st["ms"][1], 1e-9) * 1e3
        n_rows = np.ascontiguousarray([len(x) for x in keys], np.int64)
        cap = int(n_rows.max())
        hk, hl = np.zeros((S, cap), np.int64), np.zeros((S, cap), np.float32)
        for m in range(S):
            hk[m, :len(keys[m])], hl[m, :len(keys[m])] = keys[m], l[m]
        key, lo = torch.from_numpy(hk).cuda(), torch.from_numpy(hl).cuda()
        lines = [len(np.unique(x >> 21)) for x in keys]
        r = {"rows": int(n_rows.sum()), "rows_per_map_min_max": [int(n_rows.min()), int(n_rows.max())], "lines": int(sum(lines)),
             "rows_per_line": round(float(n_rows.sum()) / max(sum(lines), 1), 2),
             "emit_yardstick": {"records": st["records"], "emit_ms": round(st["ms"][1], 3), "records_per_s": round(emit)}}
        for name, segs in work.items():
            r[name] = measure(key, lo, cap, n_rows, leaf, segs)
            for v_ in ("line_directory", "plain_search"):
                r[name][v_]["cells_per_s_walk_over_emit"] = round(r[name][v_]["cells_per_s_walk"] / max(emit, 1e-9), 4)
        uk, first = np.unique(np.concatenate(keys), return_index=True)
        ul = np.concatenate(l)[first]
        key, lo = torch.from_numpy(uk[None].copy()).cuda(), torch.from_numpy(ul[None].copy()).cuda()
        r["merged"] = dict(measure(key, lo, len(uk), np.array([len(uk)], np.int64), leaf, [np.concatenate(rays)]), rows=len(uk),
                           lines=len(np.unique(uk >> 21)))
        for v_ in ("line_directory", "plain_search"):
            r["merged"][v_]["cells_per_s_walk_over_emit"] = round(r["merged"][v_]["cells_per_s_walk"] / max(emit, 1e-9), 4)
        tk = (uk[None, :] + ((np.arange(args.tiles, dtype=np.int64) * 2048) << 21)[:, None]).ravel()
        order = np.argsort(tk, kind="stable")
        tk, tl = tk[order], np.tile(ul, args.tiles)[order]
        all_rays = np.concatenate(rays).copy()
        shift = (np.arange(len(all_rays)) % args.tiles) * 2048.0 * leaf
        all_rays[:, 1] += shift
        all_rays[:, 4] += shift
        key, lo = torch.from_numpy(tk[None].copy()).cuda(), torch.from_numpy(tl[None].copy()).cuda()
        r["tiled"] = dict(measure(key, lo, len(tk), np.array([len(tk)], np.int64), leaf, [all_rays]), rows=len(tk), lines=len(np.unique(tk >> 21)))
        for v_ in ("line_directory", "plain_search"):
            r["tiled"][v_]["cells_per_s_walk_over_emit"] = round(r["tiled"][v_]["cells_per_s_walk"] / max(emit, 1e-9), 4)
        res["leaf_%.2f" % leaf] = r
        del key, lo
    del trk
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
