"""Loads libflvis_hip.so once per process and declares its C signatures from the header (_abi); the status codes and pointer helpers."""
import ctypes as C
import os

from . import _abi
from . import build as _build
from ._abi import FlvisError  # noqa: F401  (defined where the header is read, which raises it too)

_LIB = None

FLVIS_OK = 0
FLVIS_ERR_INVALID_ARG = -1
FLVIS_ERR_NO_DEVICE = -2
FLVIS_ERR_CAPACITY = -4
FLVIS_ERR_CONFIG = -5


def lib_path():
    return _build.LIB


def load_library(rebuild_if_stale=True):
    """Loads libflvis_hip.so (building it in-tree with hipcc when sources are newer). Raises if unavailable."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Import it FIRST so that libflvis_hip.so binds
    # to the HIP runtime torch already loaded; two runtimes in one process cannot both own the device.
    import torch  # noqa: F401
    if rebuild_if_stale and os.path.exists(_build.HIPCC):
        try:
            if _build.stale():
                _build.build()
        except Exception as e:  # stale-but-present library is still usable; a missing one is fatal below
            if not os.path.exists(_build.LIB):
                raise FlvisError("cannot build libflvis_hip.so: %s" % e)
    if not os.path.exists(_build.LIB):
        raise FlvisError("libflvis_hip.so is missing (run python -c 'import __graft_entry__ as g; g.build()')")
    # FLVIS_LIB_PATH: load another build of the same library (A/B runs of a kernel variant inside one benchmark session)
    _LIB = C.CDLL(os.environ.get("FLVIS_LIB_PATH") or _build.LIB)
    _abi.declare(_LIB)
    return _LIB


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _P(a, t):
    return a.ctypes.data_as(C.POINTER(t))
