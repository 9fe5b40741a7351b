"""Test helper: the STEREO_UNRECT case of the loop-closing keyframe (flvis_hip_lc_keyframe_landmarks_unrect) composed from the CPU oracle's
functions, and the inputs its CPU and GPU tests share.

The reference leaves the case empty (vo_loopclosing.cpp:318-324: "track to another image / go to undistor plane / triangulation").  The
rule is this project's: the STEREO_RECT case (:274-315) with the tracker's undistortion (camera_frame.cpp:130-131) in front of the DLT --

    calcOpticalFlowPyrLK(img0, img1, 31x31, maxLevel 5, 30 / 0.001, USE_INITIAL_FLOW) seeded at the keypoint      O.lk
    u0 = undistortPoints(keypoint, K0, D0, R0, P0),  u1 = undistortPoints(match, K1, D1, R1, P1)  (Point2f)       O.undistort_points
    pc = Triangulation::triangulationPt(u0, u1, P0, P1)                                                          O.triangulate_dlt
    kept where status == 1 and not (pc.z < 0 or pc.z > 100);  lm_2d = u0, lm_3d = pc, the descriptor; order kept

Inputs: synth.EUROC_LIKE_YAML / synth.euroc_rig(), frames of Renderer(rig=...).stereo_frame on LoopTrajectory(phase=0.0), rendered on the
CPU once per process (a GPU test uploads these very images)."""
import os
import tempfile

import numpy as np

import _geom as G
import _loop_chain as LC
import _oracle as O

W, H = 752, 480
RANGE = 100.0                     # triangulation.h:24
KIND = "euroc_like"               # synth.rig_variant's name of the rig


def load_cfg(k=0):
    """(Rig, finalized FlvisCfg) of variant k of the EuRoC-like rig; k = 0 is synth.EUROC_LIKE_YAML / synth.euroc_rig() itself"""
    import flvis_amd
    from flvis_amd import synth
    rig, text = (synth.euroc_rig(), synth.EUROC_LIKE_YAML) if k == 0 else synth.rig_variant(KIND, k)
    p = os.path.join(tempfile.gettempdir(), "flvis_lc_unrect_%d_%d.yaml" % (k, os.getpid()))
    with open(p, "w") as f:
        f.write(text)
    cfg = flvis_amd.load_config(p)
    os.remove(p)
    assert cfg.cam_type == 1 and (cfg.image_width, cfg.image_height) == (W, H)
    return rig, cfg


def cam_of(cfg):
    """what the rule reads of a finalized config"""
    a = lambda v: np.array(list(v), np.float64)
    return dict(K0=a(cfg.cam0_intrinsics), D0=a(cfg.cam0_distortion), R0=a(cfg.R0), P0=a(cfg.P0), K1=a(cfg.cam1_intrinsics),
                D1=a(cfg.cam1_distortion), R1=a(cfg.R1), P1=a(cfg.P1))


def K4_of(cfg):
    return np.array([cfg.P0[0], cfg.P0[5], cfg.P0[2], cfg.P0[6]])


def check(img0, img1, kps, desc, cam):
    """the composed checker on one keyframe: kps [n,6] (x, y first), desc [n,32] -> dict(lm2 [k,2] f32, lm3 [k,3] f64, lmd [k,32] u8,
    keep [n] bool, status [n] u8, z [n] (nan where status is 0), u0 / u1 [n,2] f32)"""
    kps = np.ascontiguousarray(kps, np.float32).reshape(-1, 6)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(kps)
    if n == 0:
        e2 = np.zeros((0, 2), np.float32)
        return dict(lm2=e2, lm3=np.zeros((0, 3)), lmd=np.zeros((0, 32), np.uint8), keep=np.zeros(0, bool), status=np.zeros(0, np.uint8),
                    z=np.zeros(0), u0=e2, u1=e2)
    pts = np.ascontiguousarray(kps[:, :2])
    nxt, st = O.lk(img0, img1, pts, pts, max_level=5, max_iter=30, eps=1e-3, use_initial=True)
    u0 = O.undistort_points(pts, cam["K0"], cam["D0"], cam["R0"], cam["P0"])
    u1 = O.undistort_points(nxt, cam["K1"], cam["D1"], cam["R1"], cam["P1"])
    keep = np.zeros(n, bool)
    pc = np.full((n, 3), np.nan)
    for i in range(n):
        if st[i] != 1:
            continue
        pc[i] = O.triangulate_dlt(u0[i].astype(np.float64), u1[i].astype(np.float64), cam["P0"], cam["P1"])
        keep[i] = not (pc[i, 2] < 0 or pc[i, 2] > RANGE)
    return dict(lm2=u0[keep].copy(), lm3=pc[keep].copy(), lmd=desc[keep].copy(), keep=keep, status=st, z=pc[:, 2].copy(), u0=u0, u1=u1)


def oracle_orb(img0):
    """the keyframe's ORB step by the oracle, cut to the closer's 1024 rows"""
    kps, desc = O.orb_detect_and_compute(img0, cap=8192)
    return kps[:1024], desc[:1024]


def rectified_gt(tr, t, rig, cfg):
    """ground-truth T_c_w pose7 of the RECTIFIED camera 0 (R0 R, R0 t): the frame of lm_3d and of every pose of such a closer"""
    R, tt = tr.T_c_w(t, rig)
    R0 = np.array(list(cfg.R0)).reshape(3, 3)
    return G.pose7(R0 @ R, R0 @ tt)


class Inputs:
    """rendered on the CPU: the true pair at t = 0 and at t = 1.2, and the two second images that replace the first pair's img1 --
    all 128 (the matcher still reports status 1 for part of the keypoints, with matches that triangulate behind the camera or not), and
    img0 itself moved 40 px to the RIGHT: wherever the matcher follows, the disparity has the wrong sign and z < 0; where it does not,
    the status is 0 -- nothing is kept (test_lc_unrect_inputs proves it on the checker)."""
    T_A, T_B = 0.0, 1.2

    def __init__(self):
        from flvis_amd import synth
        self.rig, self.cfg = load_cfg(0)
        self.cam = cam_of(self.cfg)
        self.tr = LC.LoopTrajectory(phase=0.0)
        rnd = synth.Renderer("cpu", rig=self.rig)
        pair = lambda t, i: tuple(x[0].numpy() for x in rnd.stereo_frame([self.tr], t, i))
        self.a0, self.a1 = pair(self.T_A, 0)
        self.b0, self.b1 = pair(self.T_B, 1)
        self.flat = np.full_like(self.a1, 128)
        self.moved = np.roll(self.a0, 40, axis=1)
        self.gt_a = rectified_gt(self.tr, self.T_A, self.rig, self.cfg)
        self.gt_b = rectified_gt(self.tr, self.T_B, self.rig, self.cfg)


_INPUTS = {}


def inputs():
    if "i" not in _INPUTS:
        _INPUTS["i"] = Inputs()
    return _INPUTS["i"]
