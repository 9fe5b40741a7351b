"""GPU: scripts/run_sequence.py --batch N (the frames through flvis_run_steps in chunks, the loop closing fed from the keyframe log)
against the same run frame by frame: the same trajectory file and the same keyframe path."""
import json
import os
import subprocess
import sys

import pytest

from test_dataset_runner import ROOT, make_asl_folder, make_kitti_folder, make_vocabulary_file

pytestmark = pytest.mark.gpu


def _run(root, yaml, tag, extra):
    out = os.path.join(root, "traj_%s.txt" % tag)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_sequence.py"), root, yaml, out, "--backend", "hip"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=400)
    assert r.returncode == 0, (tag, r.stderr.decode()[-2000:])
    return json.loads(r.stdout.decode().strip().splitlines()[-1]), open(out).read()


def test_batched_run_with_loop_closing_equals_the_per_frame_run():
    """KITTI folder, 9 frames in chunks of 4 (the last chunk is short): no equalizeHist on this rig, so the closer sees the same images
    either way and the two keyframe paths are the same file"""
    root, yaml, imgs = make_kitti_folder(9)
    voc = make_vocabulary_file(root, imgs[0][0])
    res, traj, path = {}, {}, {}
    for tag, extra in (("frames", []), ("batch", ["--batch", "4"])):
        lc_out = os.path.join(root, "kf_%s.txt" % tag)
        res[tag], traj[tag] = _run(root, yaml, tag, ["--loop-closing", "--voc", voc, "--lc-out", lc_out] + extra)
        path[tag] = open(lc_out).read()
    assert res["batch"]["tracked"] == res["frames"]["tracked"] == 9 and traj["batch"] == traj["frames"]
    assert res["batch"]["loop_closing"] == res["frames"]["loop_closing"] and res["batch"]["loop_closing"]["keyframes"] >= 2
    assert path["batch"] == path["frames"] and res["batch"]["batch"] == dict(steps=4, keyframes_dropped_by_the_log=0)
    assert "batch" not in res["frames"]


def test_batched_run_with_imu_equals_the_per_frame_run():
    """EuRoC ASL folder (stereo + IMU, the local map on): the IMU samples of a chunk reach run_steps step by step"""
    root, yaml = make_asl_folder(17)[:2]
    a, ta = _run(root, yaml, "frames", ["--local-map"])
    b, tb = _run(root, yaml, "batch", ["--local-map", "--batch", "5"])
    assert a["tracked"] == b["tracked"] >= 6 and ta == tb
