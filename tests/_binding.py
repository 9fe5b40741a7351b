"""The Python binding's source text, for the tests that check an entry point is bound: flvis_amd/__init__.py and the modules behind it
(flvis_amd/_*.py), not the package's tools (synth, traj_io, ...)."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source():
    return "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "flvis_amd", "_*.py"))))
