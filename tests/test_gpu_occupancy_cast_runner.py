"""GPU: scripts/run_sequence.py --occupancy --occupancy-path-check on a short synthetic depth run (the D435i depth rig of the occupancy log
test, written as an ASL folder whose second image is the 16-bit depth PNG): the segments between consecutive logged keyframe positions
cast through the finished map.  The JSON line's counts per status must equal a cast of the same segments through
Context.occupancy_cast on the map of the same run made in this process."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_dataset_runner import ROOT, _write_asl

pytestmark = pytest.mark.gpu

FRAMES, BATCH, STEP, LEAF = 62, 16, 16, 0.16      # (the rig's IMU filter initialises first: its first keyframe comes at step 50)
T0_NS = 1403636579000000000


def _depth_folder():
    """-> (root, yaml): FRAMES frames of one D435i depth stream with its IMU samples in the sensor's frame (the inverse of the D435I remap
    of traj_io.sensor_to_flvis_imu)"""
    from flvis_amd import synth
    yaml = os.path.join(tempfile.gettempdir(), "flvis_ds_d435_depth.yaml")
    open(yaml, "w").write(synth.D435I_DEPTH_YAML)
    tr = synth.Trajectory(3)
    rnd = synth.Renderer("cuda")
    frames, imu_sensor, gt_rows, t_prev = [], [], [], -0.05
    for f in range(FRAMES):
        t = f / synth.FRAME_HZ
        ns = T0_NS + int(round(t * 1e9))
        i0, d16 = rnd.depth_frame([tr], t, f, max_range=3.3)
        frames.append((ns, (i0[0].cpu().numpy(), d16[0].cpu().numpy().view(np.uint16))))
        for r in synth.imu_samples(tr, 3, t_prev, t):
            a, g = r[1:4], r[4:7]
            imu_sensor.append([T0_NS + int(round(r[0] * 1e9)), -g[1], -g[2], g[0], a[1], a[2], -a[0]])
        t_prev = t
        gt_rows.append([ns] + list(tr.pos(t)))
    root = tempfile.mkdtemp(prefix="flvis_asl_depth_")
    _write_asl(root, frames, imu_sensor, gt_rows)
    return root, yaml


def test_the_path_check_of_the_runner_equals_a_cast_of_the_same_segments():
    import torch
    import flvis_amd
    from flvis_amd import traj_io
    root, yaml = _depth_folder()
    out = os.path.join(root, "traj.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_sequence.py"), root, yaml, out, "--backend", "hip", "--batch", str(BATCH),
                        "--dense-step", str(STEP), "--occupancy", os.path.join(root, "occ.ply"), "--occupancy-leaf", str(LEAF),
                        "--occupancy-path-check"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=400)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    res = json.loads(r.stdout.decode().strip().splitlines()[-1])["occupancy"]
    check = res["path_check"]
    assert res["keyframes"] >= 3 and check["segments"] == res["keyframes"] - 1
    assert sum(check[k] for k in flvis_amd.OCCUPANCY_CAST_STATUS) == check["segments"]
    # the same run in this process: the runner's chunks through run_steps, the log's map, the log's poses
    seq = traj_io.open_sequence(root)
    dep = seq.frames(0, 1).__next__()[2]
    assert dep.dtype == np.uint16 and dep.max() > 300, "the second image came back as a depth image"
    cfg = flvis_amd.load_config(yaml)
    ctx = flvis_amd.Context(0)
    trk = flvis_amd.Tracker(ctx, cfg, 1, traj_capacity=FRAMES)
    trk.keyframe_log_enable(FRAMES)
    chunk = []
    for t, i0, i1, imu in seq.frames(0, FRAMES):
        smp = np.zeros((1, max(len(imu), 1), 7))
        for j, row in enumerate(imu):
            a, g = traj_io.sensor_to_flvis_imu(0, row[4:7], row[1:4])
            smp[0, j] = np.concatenate([[row[0]], a, g])
        chunk.append((torch.from_numpy(i0[None]).cuda(), torch.from_numpy(i1[None]).cuda(), [t], np.array([len(imu)], np.int32), smp))
        if len(chunk) == BATCH:
            trk.run_steps(chunk, with_local_map=False)
            ctx.synchronize()
            chunk = []
    if chunk:
        trk.run_steps(chunk, with_local_map=False)
    logged = trk.keyframe_log_info(0)["logged"]
    assert logged == res["keyframes"]
    got = trk.keyframe_log_occupancy([0], step=STEP, z_min=0.3, z_max=float(cfg.dr_para[1]), leaf=LEAF)
    assert int(got[3][0]) == res["voxels"] and int((got[1][0] > 0).sum()) == res["occupied"]
    path = traj_io.path_segments([trk.keyframe_log_get(0, i, images=False)["pose7"] for i in range(logged)])
    cast = ctx.occupancy_cast([(got[0][0], got[1][0])], [path], LEAF)
    assert {k: int(c) for k, c in zip(flvis_amd.OCCUPANCY_CAST_STATUS, cast[6][0])} == {k: check[k] for k in flvis_amd.OCCUPANCY_CAST_STATUS}
    assert np.array_equal(np.bincount(cast[0][0], minlength=5), cast[6][0])
    del trk
    ctx.close()
