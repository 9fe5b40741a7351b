"""CPU tests of the drop-in boundary: the C-ABI library loads and exports every symbol include/*.h declares,
and the product path fails loudly (never falls back to the CPU) when no HIP device is present."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = []
    for hdr in glob.glob(os.path.join(ROOT, "include", "*.h")):
        txt = open(hdr).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        for m in re.finditer(r"\b(flvis_[a-z0-9_]+)\s*\(", txt):
            syms.append(m.group(1))
    return sorted(set(syms))


def test_library_exports_every_declared_symbol():
    import flvis_amd
    lib = flvis_amd.load_library()
    syms = declared_symbols()
    assert len(syms) >= 10
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, "declared in include/*.h but not exported: %s" % missing
    assert b"gfx950" in lib.flvis_version()


def test_no_cpu_fallback_without_gpu():
    import torch
    import flvis_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = flvis_amd.load_library()
    h = C.c_void_p(0)
    rc = lib.flvis_hip_create(0, C.c_void_p(0), C.byref(h))
    assert rc == flvis_amd.FLVIS_ERR_NO_DEVICE and not h.value
    with pytest.raises(flvis_amd.FlvisError):
        flvis_amd.Context(0)


def test_product_does_not_reference_oracle():
    bad = []
    for path in glob.glob(os.path.join(ROOT, "flvis_amd", "**", "*"), recursive=True):
        if os.path.isfile(path) and path.endswith((".py", ".cpp", ".hip", ".hpp", ".h")):
            txt = open(path, errors="replace").read()
            if re.search(r"oracle/|libflvis_ref|ref_api\.h|ref_math\.hpp", txt):
                bad.append(path)
    assert not bad, "product sources must not use the oracle: %s" % bad


def test_config_loader_matches_oracle_on_both_rigs():
    """Host logic of the boundary: the product's yaml loader + stereoRectify (csrc/config.cpp, no GPU involved) and the
    oracle's are independent implementations; they must produce the same flvis_cfg -- every integer and every double BIT FOR BIT --
    for the synthetic rigs and for the reference's own launch files: both compose the rig transforms as Sophus SE3 objects the way
    vo_tracking.cpp:183-236 does and run cvStereoRectify / cvRodrigues2 in OpenCV's operation order.  (Round 2 allowed 1e-9: a 4x4
    matrix product instead of the quaternion composition moved the EuRoC extrinsics by 1e-13, which a run with the two loaders --
    scripts/run_sequence.py hip vs cpu -- turned into 3e-4 m of trajectory after 17 frames through differing RANSAC inlier sets.)
    The one field with a different meaning on the two sides (IMU axis-remap selector vs. an unused flag) is skipped."""
    import tempfile
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _oracle as O
    import flvis_amd
    from flvis_amd import synth
    files = []
    for tag, text in (("d435", synth.D435I_STEREO_YAML), ("euroc", synth.EUROC_LIKE_YAML), ("kitti", synth.KITTI_LIKE_YAML),
                      ("depth", synth.D435I_DEPTH_YAML)):
        p = os.path.join(tempfile.gettempdir(), "flvis_cfgpar_%s.yaml" % tag)
        open(p, "w").write(text)
        files.append((tag, p))
    for name in ("euroc", "d435i_stereo", "d435i_depth", "d435_stereo_px4", "kitti"):   # the reference's launch files, stored as fixtures
        files.append((name, os.path.join(ROOT, "tests", "golden", "yaml_ref_%s.yaml" % name)))
    for tag, p in files:
        a, b = flvis_amd.load_config(p), O.load_config(p)
        assert C.sizeof(a) == C.sizeof(b)
        fb = {getattr(type(b), n).offset: n for n, _ in b._fields_}
        for name, _ in a._fields_:
            if name == "imu_type":
                continue
            va, vb = getattr(a, name), getattr(b, fb[getattr(type(a), name).offset])
            if hasattr(va, "__len__"):
                assert list(va) == list(vb), (tag, name, [x - y for x, y in zip(va, vb)])
            else:
                assert va == vb, (tag, name, va, vb)


def test_config_loader_rejects_bad_files():
    import tempfile
    import flvis_amd
    p = os.path.join(tempfile.gettempdir(), "flvis_cfg_bad.yaml")
    open(p, "w").write("type_of_vi: 3\nimage_width: 640\n")
    with pytest.raises(flvis_amd.FlvisError):
        flvis_amd.load_config(p)
    with pytest.raises(flvis_amd.FlvisError):
        flvis_amd.load_config(os.path.join(tempfile.gettempdir(), "flvis_does_not_exist.yaml"))


def test_orb_default_pattern_matches_the_oracle_generator():
    """host-only entry point: the built-in BRIEF pattern is OpenCV's makeRandomPattern(31, ., 512), as in the oracle."""
    import flvis_amd
    import _oracle as O
    assert np.array_equal(flvis_amd.orb_default_pattern(), O.orb_default_pattern())


def test_ros_wrappers_are_compile_gated_and_call_only_declared_entry_points():
    """ros/: the three nodelet wrappers (flvis/TrackingNodeletClass, flvis/LocalMapNodeletClass, flvis/LoopClosingNodeletClass) cannot be built here (no ROS); what
    can be checked: the package configures to nothing without catkin, the plugin description names the reference's classes, and
    every flvis_* function the wrappers call is declared in include/flvis_hip.h."""
    import re
    import shutil
    import subprocess
    import tempfile
    hdr = open(os.path.join(ROOT, "include", "flvis_hip.h")).read()
    declared = set(re.findall(r"\b(flvis_[a-z0-9_]+)\s*\(", hdr))
    for f in ("tracking_nodelet.cpp", "localmap_nodelet.cpp", "loopclosing_nodelet.cpp"):
        src = open(os.path.join(ROOT, "ros", "src", f)).read()
        called = set(re.findall(r"\b(flvis_[a-z0-9_]+)\s*\(", src))
        assert called and called <= declared, (f, called - declared)
        assert "PLUGINLIB_EXPORT_CLASS" in src
    xml = open(os.path.join(ROOT, "ros", "flvis_hip_nodelets.xml")).read()
    assert 'name="flvis/TrackingNodeletClass"' in xml and 'name="flvis/LocalMapNodeletClass"' in xml
    assert 'name="flvis/LoopClosingNodeletClass"' in xml                       # flvis.xml:17 of the reference
    import xml.etree.ElementTree as ET
    for lf, classes in (("flvis_hip_kitti.launch", ("TrackingNodeletClass", "LocalMapNodeletClass", "LoopClosingNodeletClass")),
                        ("flvis_hip_euroc.launch", ("TrackingNodeletClass", "LocalMapNodeletClass"))):
        tree = ET.parse(os.path.join(ROOT, "ros", "launch", lf))                # well-formed
        loads = [n.get("args") for n in tree.getroot().iter("node") if n.get("pkg") == "nodelet" and "load" in (n.get("args") or "")]
        assert sorted(a.split()[1] for a in loads) == sorted("flvis/" + c for c in classes), (lf, loads)
        params = [n.get("name") for n in tree.getroot().iter("param")]
        assert "/yamlconfigfile" in params
    if shutil.which("cmake"):
        d = tempfile.mkdtemp(prefix="flvis_ros_cfg_")
        r = subprocess.run(["cmake", "-S", os.path.join(ROOT, "ros"), "-B", d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode == 0 and b"catkin not found" in r.stdout, r.stdout.decode()[-1500:]


def test_header_is_plain_c_and_cxx():
    """the boundary is a C ABI: include/flvis_hip.h compiles as C99 and as C++11 on its own (no torch, no HIP types in a signature)"""
    import shutil
    import subprocess
    import tempfile
    hdr = os.path.join(ROOT, "include", "flvis_hip.h")
    d = tempfile.mkdtemp(prefix="flvis_hdr_")
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if not shutil.which(cc):
            pytest.skip("no " + cc)
        src = os.path.join(d, "t." + ext)
        open(src, "w").write('#include "flvis_hip.h"\nint main(void) { flvis_lc_params p; flvis_lc_event e; flvis_image i; (void)p; (void)e; (void)i; '
                             'return sizeof(flvis_cfg) > 0 ? 0 : 1; }\n')
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.dirname(hdr), src], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()[-2000:]


def test_imu_trajectory_recorder_throttle_is_per_run_not_per_batch(tmp_path):
    """flvis_write_imu_trajectory (host code of the boundary, no GPU involved): the recorder drops what lies within min_dt of the first
    message of the RUN (vo_repub_rec.cpp:77-78, `last_time` is set once).  flvis_get_imu_states hands the rows out in batches of at most
    512: the batch that creates the file is throttled, appended batches are written in full -- the file equals the one a single call
    with all rows writes."""
    import flvis_amd
    lib = flvis_amd.load_library()
    rows = np.zeros((900, 11))
    rows[:, 0] = 100.0 + np.arange(900) * 0.005          # 200 Hz
    rows[:, 1] = 1.0                                     # q_w_i = identity
    rows[:, 5:8] = np.arange(2700).reshape(900, 3) * 1e-3
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    one = str(tmp_path / "one.txt").encode()
    two = str(tmp_path / "two.txt").encode()
    n_one = lib.flvis_write_imu_trajectory(ptr(rows), 900, one, 0.1, 0)
    a, b = np.ascontiguousarray(rows[:512]), np.ascontiguousarray(rows[512:])
    n_a = lib.flvis_write_imu_trajectory(ptr(a), 512, two, 0.1, 0)
    n_b = lib.flvis_write_imu_trajectory(ptr(b), 388, two, 0.1, 1)
    assert n_one == 900 - 21 and n_a == 512 - 21 and n_b == 388      # stamps 0.000 .. 0.100 s after the first are dropped once
    assert open(one).read() == open(two).read()
    assert lib.flvis_write_imu_trajectory(ptr(rows), 900, str(tmp_path / "no" / "such" / "dir.txt").encode(), 0.1, 0) == -5      # FLVIS_ERR_CONFIG


def test_imu_trajectory_recorder_first_batch_shorter_than_the_throttle(tmp_path):
    """flvis_write_imu_trajectory_run: a run fetched in small batches (an early flvis_get_imu_states after 8 samples = 0.035 s, less
    than min_dt) -- with the run's first stamp named in every call the appended batches are throttled against THAT stamp too, and the
    file equals the one a single call with all rows writes."""
    import flvis_amd
    lib = flvis_amd.load_library()
    rows = np.zeros((300, 11))
    rows[:, 0] = 1403636579.0 + np.arange(300) * 0.005
    rows[:, 1] = 1.0
    rows[:, 5:8] = np.arange(900).reshape(300, 3) * 1e-3
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    one = str(tmp_path / "one.txt").encode()
    many = str(tmp_path / "many.txt").encode()
    n_one = lib.flvis_write_imu_trajectory(ptr(rows), 300, one, 0.1, 0)
    t0 = float(rows[0, 0])
    n_many, first = 0, True
    for lo, hi in ((0, 8), (8, 15), (15, 40), (40, 300)):
        part = np.ascontiguousarray(rows[lo:hi])
        n_many += lib.flvis_write_imu_trajectory_run(ptr(part), hi - lo, many, 0.1, 0 if first else 1, t0)
        first = False
    assert n_one == n_many == 300 - 21
    assert open(one).read() == open(many).read()
    # NaN as the first stamp: no throttle
    assert lib.flvis_write_imu_trajectory_run(ptr(rows), 300, many, 0.1, 0, float("nan")) == 300


# ---- the C signatures come from the header, once (flvis_amd/_abi.py) ---------------------------------------------------------------

PUBLIC_NAMES = """FLVIS_OK FLVIS_ERR_INVALID_ARG FLVIS_ERR_NO_DEVICE FLVIS_ERR_CAPACITY FLVIS_ERR_CONFIG FlvisError lib_path load_library
Context voxel_cloud_info loop_candidate read_vocabulary_file save_vocabulary_file convert_vocabulary_file VocTrainParams TrainedVocabulary
OrbParams orb_default_pattern FlvisCfg FrameOut load_config config_get_bool FlvisImage FlvisKeyframe LcParams LcEvent FLVIS_LC_FIX_CAND
FlvisLcFix FLVIS_LC_ALL_MAPS FlvisLcFixIn FlvisLcLink FlvisLcMerge LC_TRAJ_ANCHOR LC_TRAJ_BLEND LC_ROWS_POSE8 LC_ROWS_TRAJ9 LC_ROWS_IMU11
LC_ROW_WIDTH FlvisLcTrajJob links_from_fix FlvisLcLinkQuery links_reverse load_lc_params LoopCloser Tracker _ptr _P _link_dict""".split()


def test_every_declared_signature_is_in_force_on_the_loaded_library():
    import flvis_amd
    from flvis_amd import _abi
    table = _abi.signatures()
    assert sorted(table) == declared_symbols() and len(table) >= 150
    lib = flvis_amd.load_library()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)                                   # (AttributeError: declared and not exported)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name


def test_signatures_match_the_header_where_written_out_by_hand():
    from flvis_amd import _abi
    t = _abi.signatures()
    p, i = C.c_void_p, C.c_int
    assert t["flvis_version"] == (C.c_char_p, [])
    assert t["flvis_hip_stream"] == (C.c_void_p, [p])
    assert t["flvis_prof_enable_stages"] == (i, [p, i, C.c_uint64])
    assert t["flvis_debug_pyramid"] == (i, [p, p, i, i, i, i, i, i, i, p, C.c_size_t])
    assert t["flvis_hip_stereo_depth"] == (i, [p, p, p, p, i, p, p, p, p, p, i, p, C.c_float, p, p, p])
    assert t["flvis_lc_links_from_fix"] == (i, [p, i, C.c_int64, i, p])
    assert t["flvis_hip_destroy"] == (None, [p])
    assert t["flvis_hip_rand_seed"] == (i, [p, C.c_uint32, p, i])
    assert t["flvis_set_imu_factor"] == (i, [p, i, C.c_double])


def test_a_type_outside_the_table_is_an_error_not_a_guess():
    import flvis_amd
    from flvis_amd import _abi
    assert _abi.parse("int flvis_a(int n, const double* x);\nvoid flvis_b(void);\n") == {"flvis_a": (C.c_int, [C.c_int, C.c_void_p]),
                                                                                       "flvis_b": (None, [])}
    for text, bad in (("int flvis_ok(int n);\nint flvis_odd(int n, long double x);\n", "long double"),
                      ("int flvis_ok(int n);\nint flvis_odd(flvis_cfg by_value);\n", "flvis_cfg"),
                      ("int flvis_ok(int n);\nint flvis_odd(short n);\n", "short"),
                      ("int flvis_ok(int n);\ndouble flvis_odd(int n);\n", "double"),
                      ("int flvis_ok(int n);\nunsigned int flvis_odd(int n);\n", "unsigned int")):
        with pytest.raises(flvis_amd.FlvisError) as e:
            _abi.parse(text)
        assert "flvis_odd" in str(e.value) and "'%s'" % bad in str(e.value), (text, str(e.value))


def _fix_with_one_accepted_candidate(seq, kf):
    import flvis_amd
    fix = flvis_amd.FlvisLcFixIn()
    fix.fix.n_candidates, fix.fix.best = 1, 0
    fix.fix.cand_kf[0], fix.cand_seq[0], fix.fix.cand_accepted[0] = kf, seq, 1
    for k, v in enumerate((0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 1.0)):
        fix.fix.cand_pose7[0][k] = v
    return fix


def test_a_64_bit_argument_survives_unwrapped():
    import flvis_amd
    lib = flvis_amd.load_library()
    fix = _fix_with_one_accepted_candidate(seq=0, kf=3)
    out = (flvis_amd.FlvisLcLink * 1)()
    kf = 2 ** 40 + 5
    assert lib.flvis_lc_links_from_fix(C.byref(fix), 1, kf, 1, out) == 1
    assert out[0].kf_to == kf and (out[0].seq_from, out[0].kf_from, out[0].seq_to) == (0, 3, 1)
    assert list(out[0].pose7) == [0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 1.0]
    with pytest.raises(C.ArgumentError):                          # a ctypes instance of another width is refused: the declaration is in force
        lib.flvis_lc_links_from_fix(C.byref(fix), 1, C.c_int(7), 1, out)


def test_too_few_arguments_are_a_type_error():
    import flvis_amd
    from flvis_amd import _abi
    lib = flvis_amd.load_library()
    for name, (_, argtypes) in _abi.signatures().items():
        if argtypes:
            with pytest.raises(TypeError):
                getattr(lib, name)(*([None] * (len(argtypes) - 1)))


def test_no_signature_is_assigned_by_hand():
    assign = re.compile(r"\.(argtypes|restype)\s*=[^=]")
    for path in glob.glob(os.path.join(ROOT, "flvis_amd", "*.py")):
        if os.path.basename(path) != "_abi.py":
            hits = [l for l in open(path) if assign.search(l)]
            assert not hits, (path, hits)
    declared = "|".join(declared_symbols())
    on_declared = re.compile(r"\b(%s)\.(argtypes|restype)\s*=[^=]" % declared)
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "scripts", "*.py")):
        hits = [l for l in open(path) if on_declared.search(l)]
        assert not hits, (path, hits)


def test_the_package_file_only_gathers_names():
    import ast
    import flvis_amd
    tree = ast.parse(open(os.path.join(ROOT, "flvis_amd", "__init__.py")).read())
    own = [getattr(n, "name", "lambda") for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef, ast.Lambda))]
    assert not own, own
    missing = [n for n in PUBLIC_NAMES if not hasattr(flvis_amd, n)]
    assert not missing, missing
    assert flvis_amd.load_library() is flvis_amd.load_library()              # (the cache)
