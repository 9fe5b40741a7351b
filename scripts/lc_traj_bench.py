#!/usr/bin/env python3
"""flvis_hip_lc_map_poses on one GPU: the trajectories of a fleet into the map frame in one call -- 64 sequences of 512 keyframes, 8192
FLVIS_LC_ROWS_TRAJ9 rows per sequence, anchor and blend mode, rows in order and shuffled -- against a device-to-device copy that moves the
same bytes, and against the route a caller has without the call (flvis_get_trajectory per stream, then numpy).

Bytes per call: rows in + rows out + anchors = (72 + 72 + 4) per row; the copy is of a buffer of half that, read once and written once.
Per configuration one JSON line:
  call_ms     host clock around the call, which returns synchronised (median, min, max of --reps calls after a warm-up call; the
              configurations take turns, so that drift of the machine hits all alike) -- upload, two launches and the wait included
  copy_ms     the same clock around the copy and a synchronise
  copy_ev_ms  the copy alone by device events over --reps back-to-back copies: what the kernels can be compared with (their own times
              come from a kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/lc_traj_bench.py --trace)
  gbps        the call's bytes over call_ms; ratio_to_copy = copy_ms / call_ms
The host route is timed for --host-streams streams and scaled: flvis_get_trajectory's copy per stream from a tracker of 64 streams with
a record of 8192 frames, then the numpy restatement of the rule (tests/_lc_traj.py) on the call's rows; its result must equal the
call's bits.  No GPU: the script fails (flvis_amd.Context raises).

usage: lc_traj_bench.py [--seqs 64] [--kfs 512] [--rows 8192] [--reps 50] [--host-streams 4] [--md FILE] [--trace]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import flvis_amd
import _lc_traj as T

ap = argparse.ArgumentParser()
ap.add_argument("--seqs", type=int, default=64)
ap.add_argument("--kfs", type=int, default=512)
ap.add_argument("--rows", type=int, default=8192)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--host-streams", type=int, default=4)
ap.add_argument("--md", default=None)
ap.add_argument("--trace", action="store_true")
a = ap.parse_args()
S, K, R = a.seqs, a.kfs, a.rows

ctx = flvis_amd.Context(0)
rng = np.random.default_rng(24)
seqs = [T.sequence(rng, K, scale=50.0, t0=T.EUROC_T0) for _ in range(S)]
O = torch.from_numpy(np.stack([s[0] for s in seqs])).cuda()
M = torch.from_numpy(np.stack([s[1] for s in seqs])).cuda()
tau = torch.from_numpy(np.stack([s[2] for s in seqs])).cuda()
nkf = np.full(S, K, np.int32)
rows = {"sorted": np.stack([T.rows_of(rng, T.TRAJ9, T.row_stamps(rng, s[2], R, T.EUROC_T0), 50.0) for s in seqs])}
rows["shuffled"] = np.stack([r[rng.permutation(R)] for r in rows["sorted"]])
d_rows = {k: torch.from_numpy(v).cuda() for k, v in rows.items()}
out = torch.empty((S, R, 9), dtype=torch.float64, device="cuda")
anc = torch.empty((S, R), dtype=torch.int32, device="cuda")
call_bytes = S * R * (72 + 72 + 4)
src = torch.empty(call_bytes // 2, dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)

fn = ctx._lib.flvis_hip_lc_map_poses
jobs = {}
for order, d in d_rows.items():
    arr = (flvis_amd.FlvisLcTrajJob * S)()
    for s in range(S):
        arr[s] = flvis_amd.FlvisLcTrajJob(s, T.TRAJ9, R, d[s].data_ptr(), out[s].data_ptr(), anc[s].data_ptr())
    jobs[order] = arr


def call(order, mode):
    rc = fn(ctx._h, S, K, flvis_amd._P(nkf, C.c_int), O.data_ptr(), M.data_ptr(), tau.data_ptr(), None, S, jobs[order], mode)
    assert rc == 0, (rc, ctx._lib.flvis_last_error(ctx._h))


def copy():
    dst.copy_(src)
    torch.cuda.synchronize()


configs = [(order, mode) for order in ("sorted", "shuffled") for mode in (T.ANCHOR, T.BLEND)]
if a.trace:
    for _ in range(10):
        for order, mode in configs:
            call(order, mode)
        copy()
    ctx.close()
    sys.exit(0)

for order, mode in configs:
    call(order, mode)
copy()
ms = {c: [] for c in configs}
ms["copy"] = []
for _ in range(a.reps):
    for c in configs + ["copy"]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        copy() if c == "copy" else call(*c)
        ms[c].append((time.perf_counter() - t0) * 1e3)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
e0.record()
for _ in range(a.reps):
    dst.copy_(src)
e1.record()
torch.cuda.synchronize()
copy_ev = e0.elapsed_time(e1) / a.reps
copy_med = float(np.median(ms["copy"]))
lines = []
for order, mode in configs:
    v = ms[order, mode]
    med = float(np.median(v))
    lines.append(dict(config="%s, %s" % (order, "blend" if mode else "anchor"), sequences=S, keyframes_per_sequence=K, rows_per_sequence=R,
                      bytes=call_bytes, call_ms=med, call_ms_min=float(min(v)), call_ms_max=float(max(v)), gbps=call_bytes / med / 1e6,
                      copy_ms=copy_med, copy_ms_min=float(min(ms["copy"])), copy_ms_max=float(max(ms["copy"])), copy_ev_ms=copy_ev,
                      copy_ev_gbps=call_bytes / copy_ev / 1e6, ratio_to_copy=copy_med / med))
    print(json.dumps(lines[-1]), flush=True)

# the route without the call: every pose to the host (flvis_get_trajectory's copy per stream), then numpy
host = None
try:
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_lc_traj_bench.yaml")
    open(p, "w").write(synth.D435I_STEREO_YAML)
    trk = flvis_amd.Tracker(ctx, flvis_amd.load_config(p), S, traj_capacity=R)
    H = min(a.host_streams, S)
    call("sorted", T.BLEND)
    got = out[:H].cpu().numpy()
    t0 = time.perf_counter()
    for s in range(H):
        trk.trajectory(s, 0, R)                      # (the record of a tracker that has seen no frame: the copy is the same)
    t1 = time.perf_counter()
    same = True
    for s in range(H):
        same = same and T.same_bits(T.map_rows(T.TRAJ9, rows["sorted"][s], *seqs[s], T.BLEND)[0], got[s])
    t2 = time.perf_counter()
    host = dict(config="host route, blend", streams_timed=H, fetch_ms_per_stream=(t1 - t0) * 1e3 / H, numpy_ms_per_stream=(t2 - t1) * 1e3 / H,
                ms_for_all_sequences=(t2 - t0) * 1e3 / H * S, equals_the_call=bool(same))
    del trk
except flvis_amd.FlvisError as e:
    host = dict(config="host route", not_measured=str(e))
print(json.dumps(host), flush=True)

if a.md:
    with open(a.md, "a") as f:
        f.write("| config | call ms (min .. max) | GB/s | copy ms (min .. max) | copy by events ms | GB/s | copy / call |\n|---|---|---|---|---|---|---|\n")
        for l in lines:
            f.write("| %s | %.3f (%.3f .. %.3f) | %.0f | %.3f (%.3f .. %.3f) | %.4f | %.0f | %.2f |\n" % (
                l["config"], l["call_ms"], l["call_ms_min"], l["call_ms_max"], l["gbps"], l["copy_ms"], l["copy_ms_min"], l["copy_ms_max"],
                l["copy_ev_ms"], l["copy_ev_gbps"], l["ratio_to_copy"]))
        f.write("\n%s\n" % json.dumps(host))
ctx.close()
