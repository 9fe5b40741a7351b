"""GPU: scripts/run_sequence.py --lc-traj-out / --lc-imu-out: the full-rate trajectories in the map frame next to the keyframe path.
On runs this short no loop closes and no drift is set, so every keyframe's drift is the identity up to rounding: the corrected files
must be the odometry files to the writers' six digits -- and the frame-by-frame run (stamps set per keyframe) and the --batch run
(stamps from the keyframe log) must write the same file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from flvis_amd import traj_io
from test_dataset_runner import ROOT, make_asl_folder, make_kitti_folder, make_vocabulary_file
from test_lc_unrect_runner import LC_BLOCK

pytestmark = pytest.mark.gpu


def _run(root, yaml, tag, extra):
    out = os.path.join(root, "traj_%s.txt" % tag)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_sequence.py"), root, yaml, out, "--backend", "hip"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=400)
    assert r.returncode == 0, (tag, r.stderr.decode()[-2000:])
    return json.loads(r.stdout.decode().strip().splitlines()[-1]), out


def _close(a, b):
    """two `stamp x y z qw qx qy qz` files: the same stamps, the poses within the writers' digits (q and -q are one rotation)"""
    ta, pa, qa = [np.asarray(x) for x in traj_io.read_stamped(a)]
    tb, pb, qb = [np.asarray(x) for x in traj_io.read_stamped(b)]
    assert len(ta) == len(tb) >= 3 and np.abs(ta - tb).max() < 1e-6
    flip = np.where((qa * qb).sum(1) < 0, -1.0, 1.0)[:, None]
    return np.abs(pa - pb).max() < 1e-4 * (1 + np.abs(pb).max()) and np.abs(qa - flip * qb).max() < 1e-4


def test_camera_trajectory_frames_and_batch():
    root, yaml, imgs = make_kitti_folder(9)
    voc = make_vocabulary_file(root, imgs[0][0])
    res, files = {}, {}
    for tag, extra in (("frames", []), ("batch", ["--batch", "4"])):
        files[tag] = os.path.join(root, "lc_traj_%s.txt" % tag)
        res[tag], odom = _run(root, yaml, tag, ["--loop-closing", "--voc", voc, "--lc-traj-out", files[tag], "--lc-traj-mode", "blend"] + extra)
        assert res[tag]["loop_closing"]["trajectory_mode"] == "blend" and res[tag]["loop_closing"]["keyframes"] >= 2
        assert _close(files[tag], odom)
    assert open(files["frames"]).read() == open(files["batch"]).read()


def test_imu_rate_trajectory_and_argument_errors():
    root, yaml, frames, _, _, _ = make_asl_folder(17)
    cfg = os.path.join(root, "euroc_lc.yaml")
    open(cfg, "w").write(open(yaml).read() + LC_BLOCK)            # (the EuRoC-like yaml carries no loop-closing block)
    voc = make_vocabulary_file(root, frames[0][1][0])
    imu, lc_imu, lc_cam = [os.path.join(root, n) for n in ("imu.txt", "lc_imu.txt", "lc_cam.txt")]
    res, odom = _run(root, cfg, "asl", ["--loop-closing", "--voc", voc, "--imu-out", imu, "--lc-imu-out", lc_imu, "--lc-traj-out", lc_cam])
    assert res["loop_closing"]["trajectory_mode"] == "anchor" and res["loop_closing"]["keyframes"] >= 1
    assert _close(lc_imu, imu) and _close(lc_cam, odom)
    script = os.path.join(ROOT, "scripts", "run_sequence.py")
    for extra in (["--lc-traj-out", lc_cam], ["--loop-closing", "--voc", voc, "--lc-imu-out", lc_imu, "--batch", "4"]):
        r = subprocess.run([sys.executable, script, root, cfg, odom, "--backend", "hip"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=120)
        assert r.returncode != 0 and b"--lc-" in r.stderr
