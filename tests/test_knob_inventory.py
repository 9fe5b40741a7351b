"""The environment knobs the library reads, against INTEGRATION.md's table, and the knobs and build variants that were retired.

Reads the sources only (no build, no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flvis_amd", "csrc")
SOURCE_EXT = (".cpp", ".hip", ".hpp", ".h", ".c", ".cc", ".py", ".md", ".txt", ".xml", ".launch", ".yaml", ".sh")

# measured, lost or tied, and removed: the default each one had is the only path (INTEGRATION.md lists where they were measured)
RETIRED_KNOBS = [
    "FLVIS_DET_START", "FLVIS_DET_ORDER", "FLVIS_HEAD_STREAM", "FLVIS_RIGHT_COPY", "FLVIS_LK_ORDER", "FLVIS_INPUT_ZEROCOPY",
    "FLVIS_BA_START", "FLVIS_DET_PRIO", "FLVIS_EVENT_SCOPE", "FLVIS_LANE_STAGGER", "FLVIS_BA_STREAMS", "FLVIS_BA_PRIORITY",
    "FLVIS_TPL_PRIO", "FLVIS_TPL_QPAD", "FLVIS_BA_REMAP", "FLVIS_BA_DRAIN", "FLVIS_H2D_WAIT", "FLVIS_H2D_QPAD", "FLVIS_H2D_LEAD",
    "FLVIS_H2D_CHUNK_MB", "FLVIS_PYR_PLAN", "FLVIS_PYR_BAND", "FLVIS_PYR_BAND2", "FLVIS_PYR_BAND3",
    "FLVIS_BA_MFMA", "FLVIS_BA_BALANCE", "FLVIS_TPL_AHEAD", "FLVIS_TPL_START",
]
RETIRED_BUILD_MACROS = ["FLVIS_LK_DIET", "FLVIS_LK_PREFETCH", "FLVIS_DEM_SORT_LANES", "FLVIS_BA_SOLVE_MFMA", "FLVIS_BA_CHOL_WG",
                        "FLVIS_BA_WG_FENCES", "FLVIS_BA_T", "FLVIS_BA_WAVES", "FLVIS_BA_PHASE_FN",
                        "FLVIS_SOLVERS_PRODUCT", "FLVIS_SPW_S", "FLVIS_RF_T", "FLVIS_EPNP_WAVES", "FLVIS_CHAIN_PRIO",
                        "FLVIS_LK_NO_TC_STORE", "FLVIS_LK_EARLY_REGION"]


def _files(*dirs, ext=SOURCE_EXT):
    for d in dirs:
        for base, subdirs, names in os.walk(os.path.join(ROOT, d)):
            subdirs[:] = [s for s in subdirs if s not in ("build", "__pycache__")]
            for n in sorted(names):
                if n.endswith(ext):
                    yield os.path.join(base, n)


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _knob_table():
    """The variables named in the first column of INTEGRATION.md's knob table."""
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    head = text.index("| variable | default | effect | measured in |")
    names = set()
    for line in text[head:].splitlines()[2:]:
        if not line.startswith("|"):
            break
        names.update(re.findall(r"`(FLVIS_[A-Z0-9_]+)", line.split("|")[1]))
    return names


def _env_reads():
    """Every FLVIS_* name the native sources read from the environment: the quoted names handed to getenv or to a helper around it."""
    names = {}
    for path in _files("flvis_amd/csrc", ext=(".cpp", ".hip", ".hpp")):
        for m in re.finditer(r'"(FLVIS_[A-Z0-9_]+)"', _read(path)):
            names.setdefault(m.group(1), os.path.relpath(path, ROOT))
    return names


def test_env_reads_are_found():
    reads = _env_reads()
    # (a guard on the scan itself: knobs that are read today in three different ways)
    for n in ("FLVIS_LANES", "FLVIS_JOIN_FOLD", "FLVIS_BA_LDS_KB", "FLVIS_EIG_WALK", "FLVIS_PYR_TILES", "FLVIS_H2D_MODE"):
        assert n in reads, n


def test_every_knob_read_is_in_the_integration_table():
    table = _knob_table()
    missing = sorted("%s (%s)" % (n, f) for n, f in _env_reads().items() if n not in table)
    assert not missing, "environment knobs read by the library but missing from INTEGRATION.md's table: " + ", ".join(missing)


def test_retired_knobs_are_gone():
    pat = re.compile(r"\b(%s)\b" % "|".join(RETIRED_KNOBS + RETIRED_BUILD_MACROS))
    hits = []
    for path in _files("flvis_amd", "include", "ros"):
        for i, line in enumerate(_read(path).splitlines(), 1):
            m = pat.search(line)
            if m:
                hits.append("%s:%d: %s" % (os.path.relpath(path, ROOT), i, m.group(1)))
    assert not hits, "retired knobs still named:\n" + "\n".join(hits)


def test_no_retired_build_variant_arms():
    pat = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b.*\b(%s)\b" % "|".join(RETIRED_BUILD_MACROS), re.M)
    hits = []
    for path in _files("flvis_amd/csrc", "include", ext=(".cpp", ".hip", ".hpp", ".h")):
        for m in pat.finditer(_read(path)):
            hits.append("%s: %s" % (os.path.relpath(path, ROOT), m.group(0).strip()))
    assert not hits, "preprocessor arms on retired build variants:\n" + "\n".join(hits)


def test_the_frame_path_reads_no_environment():
    """The knobs are read once, when a tracker is created: the files of the per-frame path do not name getenv at all, and pipeline.cpp
    only inside the three functions that read the knobs."""
    for name in ("frame_schedule.cpp", "host_feed.cpp"):
        assert "getenv" not in _read(os.path.join(CSRC, name)), name
    src = _read(os.path.join(CSRC, "pipeline.cpp"))
    readers = []
    for fn in ("read_knobs", "env_is", "ba_lds_bytes_env"):
        m = re.search(r"^(?:static )?\w[\w:<>*& ]*\b%s\(" % fn, src, re.M)
        assert m, fn
        body_start = src.index("{", m.end())
        depth, i = 0, body_start
        while True:
            c = src[i]
            depth += (c == "{") - (c == "}")
            if depth == 0:
                break
            i += 1
        assert "getenv" in src[body_start:i], fn
        readers.append((body_start, i))
    for m in re.finditer("getenv", src):
        assert any(a < m.start() < b for a, b in readers), "pipeline.cpp:%d" % (src.count("\n", 0, m.start()) + 1)
