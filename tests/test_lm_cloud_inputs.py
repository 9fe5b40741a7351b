"""CPU: the numpy restatement of the local map's map cloud (tests/_lm_cloud.py) on inputs that reach the edges the device tests rely on, and
flvis_config_get_bool (csrc/config.cpp) against yaml-cpp 0.6.2's as<bool> -- on the committed yaml-cpp dumps and on the spellings."""
import glob
import os

import numpy as np
import pytest

import _ba_synth as B
import _lm_cloud as LC
import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _presence(runs):
    ids = sorted(set(int(i) for r in runs for i in r[1]))
    return {i: [i in set(r[1].tolist()) for r in runs] for i in ids}


def _has_gap(pres):
    s = "".join("1" if p else "0" for p in pres).strip("0")
    return "0" in s


def test_edge_history_reaches_its_edges():
    runs = LC.edge_runs()
    pres = _presence(runs)
    # an id listed by two or more runs, with different estimates
    twice = [i for i, p in pres.items() if sum(p) >= 2]
    assert twice
    for i in twice:
        est = [r[2][list(r[1]).index(i)] for r in runs if i in r[1]]
        assert not np.array_equal(est[0], est[-1])
    # an id absent from a run between two that list it; a run with no landmark; a point that is not finite
    assert any(_has_gap(p) for p in pres.values())
    assert any(len(r[1]) == 0 for r in runs)
    assert any(not np.isfinite(r[2]).all() for r in runs)


def test_all_is_the_concatenation_and_latest_keeps_the_newest_in_record_order():
    runs = LC.edge_runs()
    rec = LC.record(runs, 1000)
    assert rec["runs"] == 4 and rec["dropped"] == 0
    assert np.array_equal(rec["ids"], np.concatenate([r[1] for r in runs]))
    assert np.array_equal(rec["pts"], np.concatenate([r[2] for r in runs]))
    assert np.array_equal(LC.select(rec, LC.ALL), np.arange(len(rec["ids"])))
    sel = LC.select(rec, LC.LATEST)
    assert np.all(np.diff(sel) > 0)
    ids = rec["ids"][sel]
    assert len(np.unique(ids)) == len(ids) and set(ids.tolist()) == set(rec["ids"].tolist())
    for i, at in zip(ids, sel):          # the entry of the newest run that lists the id (a second write-up: per id, the last run)
        newest = max(k for k, r in enumerate(runs) if i in r[1])
        assert rec["run"][at] == newest and np.array_equal(rec["pts"][at], runs[newest][2][list(runs[newest][1]).index(i)])
    # 103 and 104 were last listed by run 1: they stay ahead of run 3's entries; 100 and 102 (absent from run 1) come from run 3
    assert ids.tolist() == [103, 104, 100, 101, 105, 106, 107, 102]
    xyz, rid, dropped = LC.raw(rec, LC.LATEST)
    assert dropped == 1 and 107 not in rid and len(xyz) == 7 and xyz.dtype == np.float32
    xyz_all, rid_all, dropped_all = LC.raw(rec, LC.ALL)
    assert dropped_all == 1 and len(xyz_all) == 14


def test_capacity_is_per_run_and_the_record_stays_a_prefix():
    runs = LC.edge_runs()
    total = sum(len(r[1]) for r in runs)                      # 5 + 4 + 0 + 6
    assert total == 15
    exact = LC.record(runs, total)                            # a total that lands on the capacity
    assert (exact["runs"], exact["dropped"], len(exact["ids"])) == (4, 0, total)
    short = LC.record(runs, total - 1)                        # one point over: the last run goes whole
    assert (short["runs"], short["dropped"], len(short["ids"])) == (3, 1, 9)
    assert np.array_equal(short["ids"], exact["ids"][:9])
    # after the first dropped run nothing is recorded, even a run that would fit (the empty one)
    mid = LC.record(runs, 8)
    assert (mid["runs"], mid["dropped"], len(mid["ids"])) == (1, 3, 5)
    none = LC.record(runs, 4)
    assert (none["runs"], none["dropped"], len(none["ids"])) == (0, 4, 0)


def test_voxel_output_is_the_voxel_clouds_restatement_of_the_kept_points():
    import _map_cloud as MC
    rec = LC.record(LC.edge_runs(), 1000)
    for mode in (LC.ALL, LC.LATEST):
        got = LC.voxel(rec, mode, 0.08)
        P = rec["pts"][LC.select(rec, mode)]
        case, clouds = LC.as_case([P])
        want = MC.restate_dict(case, clouds[0], 0.08)
        assert np.array_equal(got["xyz"], want["xyz"]) and np.array_equal(got["npts"], want["npts"])
        assert got["n_dropped"] == 1 and got["npts"].sum() == len(P) - 1


def test_the_device_tests_driver_reaches_recurring_ids_with_gaps():
    """tests/test_gpu_lm_cloud.py drives the stand-alone local map with these sequences; through the oracle's local map they list ids in
    several runs with other estimates, and some ids leave the multi-view set and return."""
    import tempfile
    import flvis_amd
    from flvis_amd import synth
    p = os.path.join(tempfile.gettempdir(), "flvis_lmc_inputs.yaml")
    open(p, "w").write(synth.D435I_STEREO_YAML)
    cfg = flvis_amd.load_config(p)
    K4 = np.array([cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6]])
    for seed in (11, 12):
        seq = B.make_sequence(seed, n_kf=14, n_lm=260, outlier_frac=0.03)
        ref = O.LocalMap(cfg.window_size, K4)
        runs = LC.runs_from_corrections([ref.push(kf["frame_id"], kf["pose7"], kf["lm_id"], kf["lm_2d"], kf["lm_3d"]) for kf in seq["kfs"]])
        assert len(runs) == 14 - cfg.window_size + 1
        pres = _presence(runs)
        assert sum(_has_gap(p) for p in pres.values()) >= 1
        rec = LC.record(runs, 10 ** 6)
        sel = LC.select(rec, LC.LATEST)
        assert len(sel) == len(pres) < len(rec["ids"])
        assert len(set(rec["run"][sel].tolist())) >= 3                     # survivors from old runs too, not the last run alone
        total = len(rec["ids"])
        assert LC.record(runs, total)["dropped"] == 0 and LC.record(runs, total - 1)["dropped"] == 1
        assert LC.record(runs, len(runs[0][1]) - 1)["runs"] == 0


# ------------------------------------------------------------------------------------------------ flvis_config_get_bool
def _dump_scalars(path):
    out = {}
    for line in open(path).read().splitlines():
        f = line.split()
        if len(f) >= 3 and f[1] == "s":
            out[f[0]] = f[2]
    return out


def _yaml_of(dump):
    """the yaml file whose yaml-cpp dump is `dump`: the reference's launch files are stored beside their dumps, the synthetic ones are
    flvis_amd.synth's texts"""
    import tempfile
    from flvis_amd import synth
    name = os.path.basename(dump)[len("yaml_"):-len(".txt")]
    if name.startswith("ref_"):
        return os.path.join(GOLD, "yaml_%s.yaml" % name)
    text = {"d435i_stereo": synth.D435I_STEREO_YAML, "euroc_like": synth.EUROC_LIKE_YAML, "d435i_depth": synth.D435I_DEPTH_YAML,
            "kitti_like": synth.KITTI_LIKE_YAML}[name[len("synth_"):]]
    p = os.path.join(tempfile.gettempdir(), "flvis_getbool_%s.yaml" % name)
    open(p, "w").write(text)
    return p


DUMPS = sorted(glob.glob(os.path.join(GOLD, "yaml_ref_*.txt")) + glob.glob(os.path.join(GOLD, "yaml_synth_*.txt")))


def test_there_are_dumps():
    assert len(DUMPS) >= 9


@pytest.mark.parametrize("dump", DUMPS, ids=[os.path.basename(d) for d in DUMPS])
def test_get_bool_agrees_with_the_yaml_cpp_dumps(dump):
    import flvis_amd
    scalars = _dump_scalars(dump)
    path = _yaml_of(dump)
    for key in ("output_sparse_map", "is_lite_version"):
        assert scalars[key] in ("True", "False"), (dump, key)          # what yaml-cpp returned for the key, as written in the file
        assert flvis_amd.config_get_bool(path, key) == (scalars[key] == "True"), (dump, key)


def test_the_north_star_launch_file_asks_for_the_cloud():
    import flvis_amd
    assert flvis_amd.config_get_bool(os.path.join(GOLD, "yaml_ref_euroc.yaml"), "output_sparse_map") is True
    assert flvis_amd.config_get_bool(os.path.join(GOLD, "yaml_ref_kitti.yaml"), "output_sparse_map") is False


def _spellings():
    out = []
    for t, f in (("y", "n"), ("yes", "no"), ("true", "false"), ("on", "off")):
        for form in (str.lower, str.capitalize, str.upper):
            out += [(form(t), True), (form(f), False)]
    return out


def test_get_bool_spellings(tmp_path):
    """yaml-cpp 0.6.2 convert<bool>: four pairs of names, each entirely lower case, Capitalised or entirely UPPER -- 24 spellings ("Y" and
    "N" are both Capitalised and UPPER) -- and nothing else."""
    import flvis_amd
    sp = _spellings()
    assert len(sp) == 24 and len(set(s for s, _ in sp)) == 22
    p = str(tmp_path / "b.yaml")
    for text, want in sp:
        open(p, "w").write("first: 1\nflag:   %s   # a comment\nlast: [1, 2]\n" % text)
        assert flvis_amd.config_get_bool(p, "flag") is want, text
    for text in ("tRue", "yEs", "oN", "FALSe", "nO", "1", "0", "2.5", "", "maybe", "truee", "[true]"):
        open(p, "w").write("flag: %s\nother: true\n" % text)
        with pytest.raises(flvis_amd.FlvisError) as e:
            flvis_amd.config_get_bool(p, "flag")
        assert "flag" in str(e.value), text
        assert flvis_amd.config_get_bool(p, "other") is True
    with pytest.raises(flvis_amd.FlvisError) as e:
        flvis_amd.config_get_bool(p, "absent")
    assert "missing" in str(e.value) and "absent" in str(e.value)
    with pytest.raises(flvis_amd.FlvisError) as e:
        flvis_amd.config_get_bool(str(tmp_path / "none.yaml"), "flag")
    assert "cannot open" in str(e.value)


def test_get_bool_leaves_flvis_cfg_alone():
    """the key is read on its own: flvis_cfg's layout is what the ctypes mirror and the checker hold"""
    import ctypes as C
    import flvis_amd
    assert C.sizeof(flvis_amd.FlvisCfg) == C.sizeof(O.RefConfig)
    assert not any(n in ("output_sparse_map", "is_lite_version") for n, _ in flvis_amd.FlvisCfg._fields_)
