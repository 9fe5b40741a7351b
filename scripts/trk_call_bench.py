#!/usr/bin/env python3
"""flvis_hip_lkorb_tracking (LKORBTracking::tracking as ONE call) against the call-by-call binding of INTEGRATION.md section A3, for 64 sets
of 640 x 480 with about 300 landmarks each on the unrectified rig, every second set with an IMU guess (so both PnP branches run).

--mode call: the one call.  --mode chain: the six library calls of section A3 (project_points, lk_track, undistort_points,
find_fundamental_ransac, pnp_ransac, debug_pnp_ransac_iterative) with their three downloads, the survivor loop, the mirrored F-mask loop
and updateLMState on the host (numpy, per set), and the three uploads; it needs none of the new code and runs on an older build of the
library too (FLVIS_LIB_PATH).  Both are checked against each other before they are timed (--mode both): same counts, same poses.

A run is warmed up, then timed as wall time around REPS repetitions that end in a stream synchronisation, five windows, median and range.
Host synchronisations per repetition are counted: blocking downloads of the caller, and the waits inside the calls for an upload of
their host arguments (one each in project_points, undistort_points, both PnP calls and the one call).  Needs a GPU: fails without one.
--out FILE appends a markdown row."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import flvis_amd  # noqa: E402
import _trk_call as T  # noqa: E402

SETS, REPS, WINDOWS, CAP = 64, 20, 5, 320


def inputs():
    """64 sets on one image pair: each set another 300 survivors-to-be and 10 patch landmarks of the pool, every second one with a guess"""
    P = T.pool("unrect", 640, 480)
    sets = []
    for s in range(SETS):
        g = np.roll(P["good"], -3 * s)[:300]
        idx = np.concatenate([P["bad"][:5], g, P["bad"][5:10]])
        sets.append(T.Scene("bench%02d" % s, "unrect", idx, guess=bool(s & 1), w=640, h=480))
    return T.Call(sets, CAP)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Chain:
    """INTEGRATION.md A3 for the whole batch: what an integrator at the reference's call sites runs per frame"""

    def __init__(self, ctx, call):
        self.ctx, self.r, self.a = ctx, call.rig, call.arrays()
        a = self.a
        self.d = {k: dev(a[k]) for k in ("img_from", "img_to", "p2d", "p3w", "count")}
        self.n = np.clip(a["count"], 0, CAP)
        self.syncs = 0

    def run(self):
        ctx, r, a, d, S = self.ctx, self.r, self.a, self.d, SETS
        self.syncs = 0
        R0, P0 = r.R0.reshape(3, 3), r.P0.reshape(3, 4)
        # :58 projectPoints for the sets with a guess (the others keep the pixel), :64 LK, :87 undistortPoints
        trk = d["p2d"].clone()
        if a["use_guess"].any():
            proj = ctx.project_points(d["p3w"], d["count"], a["guess"], r.K0, r.D0)
            self.syncs += 1
            ug = dev(a["use_guess"]).bool()
            trk[ug] = proj[ug]
        trk, status = ctx.lk_track(d["img_from"], d["img_to"], d["p2d"], trk, d["count"], 10, 30, 1e-3, True)
        und = ctx.undistort_points(trk, d["count"], r.K0, r.D0, R0, P0)
        self.syncs += 1
        h_trk, h_und, h_st = trk.cpu().numpy(), und.cpu().numpy(), status.cpu().numpy()           # download 1
        self.syncs += 1
        # :94-125 the survivor loop
        m1 = np.zeros((S, CAP, 2), np.float32)
        m2 = np.zeros((S, CAP, 2), np.float32)
        cnt = np.zeros(S, np.int32)
        to = []
        for s in range(S):
            n = self.n[s]
            t = h_trk[s, :n]
            ok = (h_st[s, :n] == 1) & (t[:, 0] > 0) & (t[:, 1] > 0) & (t[:, 0] < np.float32(r.w - 1)) & (t[:, 1] < np.float32(r.h - 1))
            surv = np.flatnonzero(ok)
            desc = surv[::-1]
            to.append(dict(frm=desc, und=h_und[s, desc], flags=a["flags"][s, desc].copy(), of=len(surv)))
            if len(surv) >= 10:
                cnt[s] = len(surv)
                m1[s, :len(surv)], m2[s, :len(surv)] = a["p2u"][s, surv], h_und[s, surv]
        # :134 findFundamentalMat
        mask, _ = ctx.find_fundamental_ransac(dev(m1), dev(m2), dev(cnt))                          # upload 1
        h_mask = mask.cpu().numpy()                                                                # download 2
        self.syncs += 1
        # :138-168 the mirrored index, the counts, the pairs
        order = [s for s in range(S) if not a["use_guess"][s]] + [s for s in range(S) if a["use_guess"][s]]
        n_p3p = int((a["use_guess"] == 0).sum())
        p3 = np.zeros((S, CAP, 3), np.float32)
        p2 = np.zeros((S, CAP, 2), np.float32)
        k = np.zeros(S, np.int32)
        counts = np.zeros((S, 4), np.int32)
        for q, s in enumerate(order):
            t = to[s]
            counts[s, 0] = t["of"]
            if cnt[s] == 0:
                continue
            t["flags"][:cnt[s]][h_mask[s, :cnt[s]] == 0] &= np.uint8(0xFD)
            counts[s, 1] = int(((t["flags"] >> 1) & 1).sum())
            if counts[s, 1] < 10:
                continue
            sel = np.flatnonzero((t["flags"] & 3) == 3)
            t["sel"] = sel
            k[q] = counts[s, 2] = len(sel)
            p2[q, :len(sel)], p3[q, :len(sel)] = t["und"][sel], a["p3w"][s, t["frm"][sel]]
        d3, d2, dk = dev(p3), dev(p2), dev(k)                                                      # upload 2
        pose, pm, ninl = np.zeros((S, 7)), np.zeros((S, CAP), np.uint8), np.zeros(S, np.int32)
        if n_p3p:
            o = ctx.pnp_ransac(d3[:n_p3p], d2[:n_p3p], dk[:n_p3p], r.K4, np.zeros(n_p3p, np.uint64), 100, 3.0, 0.99)
            self.syncs += 1
            pose[:n_p3p], pm[:n_p3p], ninl[:n_p3p] = (v.cpu().numpy() for v in o)                  # download 3
        if n_p3p < S:
            g = a["guess"][order[n_p3p:]]
            o = ctx.debug_pnp_ransac_iterative(d3[n_p3p:], d2[n_p3p:], dk[n_p3p:], r.K4, g, 100, 3.0, 0.99)
            self.syncs += 1
            pose[n_p3p:], pm[n_p3p:], ninl[n_p3p:] = (v.cpu().numpy() for v in o)
        self.syncs += 1
        # :188-200 updateLMState, the pose, the return value
        out_pose, ret = a["pose_in"].copy(), np.zeros(S, np.uint8)
        for q, s in enumerate(order):
            if "sel" not in to[s]:
                continue
            sel = to[s]["sel"]
            to[s]["flags"][sel[pm[q, :len(sel)] == 0]] &= np.uint8(0xFD)
            counts[s, 3], out_pose[s], ret[s] = ninl[q], pose[q], ninl[q] >= 10
        return counts, out_pose, ret


class OneCall:
    def __init__(self, ctx, call):
        a = call.arrays()
        self.ctx, self.a, self.cfg = ctx, a, call.rig.lib_cfg()
        self.d = [dev(a[k]) for k in ("img_from", "img_to", "p2d", "p2u", "p3w", "flags", "count")]
        self.pose0 = dev(a["pose_in"])
        self.pose = self.pose0.clone()
        self.out = None
        self.syncs = 1                                                      # the wait for the upload of the guesses inside the call

    def run(self):
        self.pose.copy_(self.pose0)
        self.out = self.ctx.lkorb_tracking(self.cfg, *self.d, self.a["guess"], self.a["use_guess"], pose7=self.pose, out=self.out)
        return self.out


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / REPS * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("call", "chain", "both"), default="both")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", help="append the rows (markdown) to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trk_call_bench: no GPU")
    ctx = flvis_amd.Context(0)
    call = inputs()
    rows = []
    chain = Chain(ctx, call) if args.mode != "call" else None
    one = OneCall(ctx, call) if args.mode != "chain" else None
    if args.mode == "both":
        c, p, r = chain.run()
        o = one.run()
        torch.cuda.synchronize()
        assert np.array_equal(c, o["counts4"].cpu().numpy()) and np.array_equal(r, o["ret"].cpu().numpy())
        oc = o["pose7"].cpu().numpy()
        found = c[:, 3] > 0                                                 # (no model: the chain's hook hands the guess back untouched)
        assert np.array_equal(p[found], oc[found])
        print("chain and call agree: of %s, ret %d / %d" % (c[:4, 0].tolist(), int(r.sum()), SETS), flush=True)
    for name, obj in (("one call (flvis_hip_lkorb_tracking)", one), ("A3 chain (six calls, host loops)", chain)):
        if obj is None:
            continue
        med, lo, hi = timed(obj.run)
        rows.append((name, med, lo, hi, obj.syncs))
        print("%-40s %s %d sets: %8.2f ms per batch (windows %.2f .. %.2f), %d host synchronisations" % (name, args.label, SETS, med, lo, hi, obj.syncs),
              flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for name, med, lo, hi, syncs in rows:
                f.write("| %s | %s | %.2f | %.2f .. %.2f | %d |\n" % (name, args.label, med, lo, hi, syncs))
    ctx.close()


if __name__ == "__main__":
    main()
