#!/usr/bin/env python3
"""Times of the front-end's solver calls on caller arrays -- flvis_hip_find_fundamental_ransac, flvis_hip_optimize_in_frame,
flvis_hip_undistort_points, flvis_hip_project_points -- at 64 sets of 240 and of 480 points, the two configured frame sizes.

Each (call, size) is warmed up, then timed with HIP events around REPS back-to-back calls on the context's stream, five windows, median and
range reported.  A call includes what it does on the host (argument checks, the upload of cameras / poses and the wait for it), so the
figures are call times, not kernel times.  Needs a GPU: fails without one.  --out FILE appends the table as markdown."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import flvis_amd  # noqa: E402
import _geom_calls as E  # noqa: E402

SETS, REPS, WINDOWS = 64, 200, 5


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / REPS * 1e3)
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the table (markdown) to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("geom_calls_bench: no GPU")
    ctx = flvis_amd.Context(0)
    K, D, R, P = E.rigs()["euroc"]
    rows = []
    for n in (240, 480):
        cap = 512
        m1 = np.zeros((SETS, cap, 2), np.float32)
        m2 = np.zeros((SETS, cap, 2), np.float32)
        p3 = np.zeros((SETS, cap, 3))
        z = np.zeros((SETS, cap, 2))
        pose = np.zeros((SETS, 7))
        for s in range(SETS):
            m1[s, :n], m2[s, :n] = E.two_view(9000 + s, n, outl=0.2)
            p3[s, :n], z[s, :n], _, pose[s] = E.lm_scene(9100 + s, n, n_out=n // 10)
        cnt = torch.full((SETS,), n, dtype=torch.int32, device="cuda")
        d_m1, d_m2 = torch.from_numpy(m1).cuda(), torch.from_numpy(m2).cuda()
        d_p3, d_z = torch.from_numpy(p3).cuda(), torch.from_numpy(z).cuda()
        d_ids = torch.arange(cap, dtype=torch.int64, device="cuda").repeat(SETS, 1).contiguous()
        d_pose0 = torch.from_numpy(pose).cuda()
        d_pose = d_pose0.clone()
        d_p3f = d_p3.float().contiguous()
        mask = torch.zeros((SETS, cap), dtype=torch.uint8, device="cuda")
        ninl = torch.zeros((SETS,), dtype=torch.int32, device="cuda")
        ok = torch.zeros((SETS,), dtype=torch.uint8, device="cuda")
        dst = torch.zeros((SETS, cap, 2), dtype=torch.float32, device="cuda")

        def lm():
            d_pose.copy_(d_pose0)                              # (in / out: every call starts from the same poses)
            ctx.optimize_in_frame(d_p3, d_z, d_ids, cnt, E.K4, d_pose, ok=ok)

        calls = (("flvis_hip_find_fundamental_ransac", lambda: ctx.find_fundamental_ransac(d_m1, d_m2, cnt, mask=mask, n_inliers=ninl)),
                 ("flvis_hip_optimize_in_frame (+ the 3.5 KB pose reset)", lm),
                 ("flvis_hip_undistort_points", lambda: ctx.undistort_points(d_m1, cnt, K, D, R, P, dst=dst)),
                 ("flvis_hip_project_points", lambda: ctx.project_points(d_p3f, cnt, pose, K, D, dst=dst)))
        for name, fn in calls:
            med, lo, hi = timed(fn)
            note = ""
            if "fundamental" in name:
                note = "mean inliers %.0f" % float(ninl.float().mean())
            if "optimize" in name:
                note = "ok %d / %d" % (int(ok.sum()), SETS)
            rows.append((name, n, med, lo, hi, note))
            print("%-56s %d sets of %3d: %8.1f us per call (windows %.1f .. %.1f)  %s" % (name, SETS, n, med, lo, hi, note), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("| call | sets x points | us per call (median of %d windows of %d calls) | range | |\n|---|---|---|---|---|\n" % (WINDOWS, REPS))
            for name, n, med, lo, hi, note in rows:
                f.write("| `%s` | %d x %d | %.1f | %.1f .. %.1f | %s |\n" % (name, SETS, n, med, lo, hi, note))
    ctx.close()


if __name__ == "__main__":
    main()
