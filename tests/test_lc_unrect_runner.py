"""CPU: scripts/run_sequence.py --loop-closing on an EuRoC ASL folder (unrectified stereo).  Without --lc-stereo-unrect the loop closing is
the reference's: its STEREO_UNRECT case is empty and no keyframe gets a landmark.  With it the CPU backend's keyframes get theirs from the
checker composed from the oracle's functions (tests/_lc_unrect.py); the tracker's own output does not change."""
import json
import os
import subprocess
import sys

from test_dataset_runner import make_asl_folder, make_vocabulary_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC_BLOCK = "lcKFStart: 25\nlcKFDist: 18\nlcKFMaxDist: 50\nlcKFLast: 20\nlcNKFClosest: 2\nratioMax: 0.5\nratioRansac: 0.5\nminPts: 20\nminScore: 0.12\n"


def test_run_sequence_cpu_backend_with_and_without_the_switch():
    root, yaml, frames, _, _, _ = make_asl_folder(5)
    cfg = os.path.join(root, "euroc_lc.yaml")
    open(cfg, "w").write(open(yaml).read() + LC_BLOCK)            # (the EuRoC-like yaml carries no loop-closing block)
    voc = make_vocabulary_file(root, frames[0][1][0])
    run = lambda out, *extra: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_sequence.py"), root, cfg, out, "--backend", "cpu"] +
                                             list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    outs = [os.path.join(root, "traj_%d.txt" % k) for k in range(3)]
    r = run(outs[0], "--loop-closing", "--voc", voc)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    off = json.loads(r.stdout.decode().strip().splitlines()[-1])["loop_closing"]
    assert off["keyframes"] >= 1 and "stereo_unrect_landmarks" not in off
    r = run(outs[1], "--loop-closing", "--voc", voc, "--lc-stereo-unrect")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    on = json.loads(r.stdout.decode().strip().splitlines()[-1])["loop_closing"]
    assert on["keyframes"] == off["keyframes"] and on["stereo_unrect_landmarks"] > 100 * on["keyframes"], on
    assert open(outs[0]).read() == open(outs[1]).read()           # the tracker's output does not change
    r = run(outs[2], "--lc-stereo-unrect")
    assert r.returncode != 0 and b"--loop-closing" in r.stderr
