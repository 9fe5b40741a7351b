"""The ctypes structures and constants that mirror include/flvis_hip.h, and the host-only loaders that fill them."""
import ctypes as C
import os

import numpy as np

from ._loader import FLVIS_OK, FlvisError, _P, _ptr, load_library


class VocTrainParams(C.Structure):
    """flvis_voc_train_params of include/flvis_hip.h."""
    _fields_ = [("k", C.c_int), ("L", C.c_int), ("weighting", C.c_int), ("seed", C.c_uint), ("max_iters", C.c_int),
                ("small_node_max", C.c_int)]


class OrbParams(C.Structure):
    """flvis_orb_params of include/flvis_hip.h."""
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int), ("fast_threshold", C.c_int)]


def orb_default_pattern():
    """flvis_orb_default_pattern (host only): the built-in 256-pair sampling pattern as int8 [512,2]."""
    p = np.zeros((512, 2), np.int8)
    rc = load_library().flvis_orb_default_pattern(C.c_void_p(p.ctypes.data))
    if rc != FLVIS_OK:
        raise FlvisError("flvis_orb_default_pattern failed")
    return p


class FlvisCfg(C.Structure):
    """flvis_cfg of include/flvis_hip.h."""
    _fields_ = [("type_of_vi", C.c_int), ("image_width", C.c_int), ("image_height", C.c_int),
                ("cam0_intrinsics", C.c_double * 4), ("cam0_distortion", C.c_double * 4),
                ("cam1_intrinsics", C.c_double * 4), ("cam1_distortion", C.c_double * 4),
                ("T_imu_cam0", C.c_double * 16), ("T_cam0_cam1", C.c_double * 16),
                ("vifusion_para", C.c_double * 6), ("feature_para", C.c_double * 6), ("dr_para", C.c_double * 3),
                ("window_size", C.c_int),
                ("cam_type", C.c_int), ("imu_type", C.c_int), ("skip_first_n_imgs", C.c_int),
                ("need_equal_hist", C.c_int),
                ("R0", C.c_double * 9), ("R1", C.c_double * 9), ("P0", C.c_double * 12), ("P1", C.c_double * 12),
                ("depth_factor", C.c_double)]


class FrameOut(C.Structure):
    """flvis_frame_out of include/flvis_hip.h."""
    _fields_ = [("state", C.c_int), ("new_keyframe", C.c_int), ("reset_cmd", C.c_int), ("n_landmarks", C.c_int),
                ("frame_id", C.c_int64), ("T_c_w", C.c_double * 7),
                ("of_inliers", C.c_int), ("f_inliers", C.c_int), ("pnp_inliers", C.c_int), ("pad_", C.c_int),
                ("reprojection_error", C.c_double)]


def load_config(yaml_path):
    """flvis_config_load: accepts the reference's yaml files unchanged.  Host-only (no GPU needed)."""
    lib = load_library()
    cfg = FlvisCfg()
    err = C.create_string_buffer(256)
    rc = lib.flvis_config_load(yaml_path.encode(), C.byref(cfg), err, 256)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_config_load(%s) failed (%d): %s" % (yaml_path, rc, err.value.decode()))
    return cfg


def config_get_bool(yaml_path, key):
    """flvis_config_get_bool: one boolean key of a yaml file as getBoolVariableFromYaml reads it (y/n, yes/no, true/false, on/off; lower,
    Capitalised or UPPER).  FlvisError for a missing key or any other value.  Host-only."""
    lib = load_library()
    out = C.c_int(0)
    err = C.create_string_buffer(256)
    rc = lib.flvis_config_get_bool(yaml_path.encode(), key.encode(), C.byref(out), err, 256)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_config_get_bool(%s, %s) failed (%d): %s" % (yaml_path, key, rc, err.value.decode()))
    return bool(out.value)


class FlvisImage(C.Structure):
    """flvis_image of include/flvis_hip.h: one host image (pitch in bytes)."""
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("width", C.c_int), ("height", C.c_int), ("pitch", C.c_int), ("channels", C.c_int),
                ("t", C.c_double)]


class FlvisStep(C.Structure):
    """flvis_step of include/flvis_hip.h: one frame step of flvis_run_steps, images on the device, times and IMU samples on the host."""
    _fields_ = [("d_img0", C.c_void_p), ("d_img1", C.c_void_p), ("h_times", C.c_void_p), ("h_imu_counts", C.c_void_p),
                ("h_imu_samples", C.c_void_p), ("imu_samples_per_stream", C.c_int)]


class FlvisKeyframe(C.Structure):
    """flvis_keyframe of include/flvis_hip.h: the flvis/KeyFrame message on host arrays."""
    _fields_ = [("frame_id", C.c_int64), ("command", C.c_int8), ("stamp", C.c_double), ("img0", FlvisImage), ("img1", FlvisImage),
                ("lm_count", C.c_int32), ("lm_id", C.POINTER(C.c_int64)), ("lm_2d", C.POINTER(C.c_double)), ("lm_3d", C.POINTER(C.c_double)),
                ("T_c_w", C.c_double * 7)]


class LcParams(C.Structure):
    """flvis_lc_params of include/flvis_hip.h (LC_PARAS, vo_loopclosing.cpp:86-97)."""
    _fields_ = [("lcKFStart", C.c_int), ("lcKFDist", C.c_int), ("lcKFMaxDist", C.c_int), ("lcKFLast", C.c_int), ("lcNKFClosest", C.c_int),
                ("minPts", C.c_int), ("ratioMax", C.c_double), ("ratioRansac", C.c_double), ("minScore", C.c_double)]


class LcEvent(C.Structure):
    """flvis_lc_event of include/flvis_hip.h."""
    _fields_ = [("kf_prev", C.c_int64), ("kf_curr", C.c_int64), ("candidate", C.c_int), ("n_matches", C.c_int), ("n_inliers", C.c_int),
                ("loop_accepted", C.c_int), ("optimised", C.c_int), ("pgo_iterations", C.c_int), ("loop_pose7", C.c_double * 7),
                ("chi2_before", C.c_double), ("chi2_after", C.c_double)]


FLVIS_LC_FIX_CAND = 8


class FlvisLcFix(C.Structure):
    """flvis_lc_fix of include/flvis_hip.h: what flvis_loop_closer_localize reports for one query."""
    _fields_ = [("n_landmarks", C.c_int), ("n_candidates", C.c_int), ("best", C.c_int), ("reserved", C.c_int),
                ("cand_kf", C.c_int64 * FLVIS_LC_FIX_CAND), ("cand_score", C.c_double * FLVIS_LC_FIX_CAND),
                ("cand_matches", C.c_int * FLVIS_LC_FIX_CAND), ("cand_inliers", C.c_int * FLVIS_LC_FIX_CAND),
                ("cand_accepted", C.c_int * FLVIS_LC_FIX_CAND), ("cand_pose7", (C.c_double * 7) * FLVIS_LC_FIX_CAND),
                ("T_c_map7", C.c_double * 7)]


FLVIS_LC_ALL_MAPS = -1


class FlvisLcFixIn(C.Structure):
    """flvis_lc_fix_in of include/flvis_hip.h: what flvis_loop_closer_localize_in reports for one query."""
    _fields_ = [("fix", FlvisLcFix), ("cand_seq", C.c_int * FLVIS_LC_FIX_CAND), ("map", C.c_int), ("reserved", C.c_int)]


class FlvisLcLink(C.Structure):
    """flvis_lc_link of include/flvis_hip.h: keyframe kf_from of sequence seq_from seen from keyframe kf_to of sequence seq_to (pose7: the
    `to` camera from the `from` camera)."""
    _fields_ = [("seq_from", C.c_int), ("seq_to", C.c_int), ("kf_from", C.c_int64), ("kf_to", C.c_int64), ("pose7", C.c_double * 7)]


class FlvisLcMerge(C.Structure):
    """flvis_lc_merge of include/flvis_hip.h: what flvis_loop_closer_merge reports for one group."""
    _fields_ = [("optimised", C.c_int), ("n_vertices", C.c_int), ("n_edges", C.c_int), ("iterations", C.c_int),
                ("chi2_before", C.c_double), ("chi2_after", C.c_double)]


LC_TRAJ_ANCHOR, LC_TRAJ_BLEND = 0, 1                       # FLVIS_LC_TRAJ_*
LC_ROWS_POSE8, LC_ROWS_TRAJ9, LC_ROWS_IMU11 = 0, 1, 2      # FLVIS_LC_ROWS_*
LC_ROW_WIDTH = {LC_ROWS_POSE8: 8, LC_ROWS_TRAJ9: 9, LC_ROWS_IMU11: 11}


class FlvisLcTrajJob(C.Structure):
    """flvis_lc_traj_job of include/flvis_hip.h: n rows of one kind of one sequence for flvis_hip_lc_map_poses / flvis_loop_closer_map_poses."""
    _fields_ = [("seq", C.c_int), ("kind", C.c_int), ("n", C.c_int), ("d_in", C.c_void_p), ("d_out", C.c_void_p), ("d_anchor", C.c_void_p)]


class FlvisLcLinkQuery(C.Structure):
    """flvis_lc_link_query of include/flvis_hip.h: a stored keyframe as the query of flvis_loop_closer_link."""
    _fields_ = [("stream", C.c_int), ("map", C.c_int), ("kf", C.c_int64), ("own_gap", C.c_int64)]


class DepthCloudParams(C.Structure):
    """flvis_depth_cloud_params of include/flvis_hip.h: the sampled window (u1 / v1 <= 0: the image's width / height), the steps and the
    inclusive z limits in metres of flvis_hip_depth_cloud."""
    _fields_ = [("u0", C.c_int), ("v0", C.c_int), ("u1", C.c_int), ("v1", C.c_int), ("step_u", C.c_int), ("step_v", C.c_int),
                ("z_min", C.c_double), ("z_max", C.c_double)]


def depth_cloud_params(window=None, step=1, z_min=0.3, z_max=10.0):
    """-> DepthCloudParams.  window: (u0, v0, u1, v1), None: the whole image; step: one int or (step_u, step_v)."""
    if isinstance(window, DepthCloudParams):
        return window
    u0, v0, u1, v1 = (0, 0, 0, 0) if window is None else [int(x) for x in window]
    su, sv = (step, step) if np.isscalar(step) else step
    return DepthCloudParams(u0, v0, u1, v1, int(su), int(sv), float(z_min), float(z_max))


def octomap_feeder_params(height):
    """The sampling of the reference's octomap feeder (octomap_feeder.cpp:35-61): every 7th pixel of every 7th row from height / 2 - 22
    to height / 2 + 20 (seven rows), 0.5 m to 6.5 m."""
    return DepthCloudParams(0, height // 2 - 22, 0, height // 2 + 21, 7, 7, 0.5, 6.5)


class DenseStereoParams(C.Structure):
    """flvis_dense_stereo_params of include/flvis_hip.h: the disparities d_min .. d_min + n_disp - 1, the box sum's radius, the uniqueness
    margin in per cent and the left-right tolerance in px (-1: no check) of flvis_hip_dense_stereo."""
    _fields_ = [("d_min", C.c_int), ("n_disp", C.c_int), ("agg_r", C.c_int), ("uniq", C.c_int), ("lr_tol", C.c_int)]


def dense_stereo_params(d_min=0, n_disp=64, agg_r=2, uniq=10, lr_tol=1):
    """-> DenseStereoParams (d_min may be one already)."""
    if isinstance(d_min, DenseStereoParams):
        return d_min
    return DenseStereoParams(int(d_min), int(n_disp), int(agg_r), int(uniq), int(lr_tol))


class OccupancyParams(C.Structure):
    """flvis_occupancy_params of include/flvis_hip.h: the float log-odds a hit / a miss observation adds, and the clamp."""
    _fields_ = [("l_hit", C.c_float), ("l_miss", C.c_float), ("l_min", C.c_float), ("l_max", C.c_float)]


def occupancy_params(l_hit=None, l_miss=None, l_min=None, l_max=None):
    """-> OccupancyParams: flvis_occupancy_params_default (octomap's documented 0.85, -0.4, -2.0, 3.5) with the given fields replaced
    (l_hit may be an OccupancyParams already)."""
    if isinstance(l_hit, OccupancyParams):
        return l_hit
    p = OccupancyParams()
    load_library().flvis_occupancy_params_default(C.byref(p))
    for k, v in (("l_hit", l_hit), ("l_miss", l_miss), ("l_min", l_min), ("l_max", l_max)):
        if v is not None:
            setattr(p, k, float(v))
    return p


class OccupancyCastParams(C.Structure):
    """flvis_occupancy_cast_params of include/flvis_hip.h: a row is OCCUPIED when l > thres; ignore_unknown 1 lets a walk pass UNKNOWN
    cells; max_cells > 0 stops a walk with LIMIT before the test of that cell."""
    _fields_ = [("thres", C.c_float), ("ignore_unknown", C.c_int), ("max_cells", C.c_int)]


def occupancy_cast_params(thres=None, ignore_unknown=None, max_cells=None):
    """-> OccupancyCastParams: flvis_occupancy_cast_params_default (0.0, 0, 0) with the given fields replaced (thres may be an
    OccupancyCastParams already)."""
    if isinstance(thres, OccupancyCastParams):
        return thres
    p = OccupancyCastParams()
    load_library().flvis_occupancy_cast_params_default(C.byref(p))
    if thres is not None:
        p.thres = float(thres)
    if ignore_unknown is not None:
        p.ignore_unknown = int(ignore_unknown)
    if max_cells is not None:
        p.max_cells = int(max_cells)
    return p


def occupancy_rows(call, n, cap, n_out, device, host=False, centres=True):
    """Runs an occupancy call with fitting row buffers.  call(cap, key, l, xyz) makes the C call with the three row pointers (None with
    cap 0) and fills n_out; cap None: found by a call of its own.  -> (keys [n] of int64 [k], logodds [n] of float32 [k], centres [n] of
    float32 [k, 3] or None) as numpy arrays, k = min(n_out, cap)."""
    import torch
    if cap is None:
        call(0, None, None, None)
        cap = int(max(list(n_out[:n]) + [0]))
    cap = int(cap)
    shape = (max(n, 1), max(cap, 0))
    if host:
        hk, hl = np.zeros(shape, np.int64), np.zeros(shape, np.float32)
        hx = np.zeros(shape + (3,), np.float32) if centres else None
        call(cap, _P(hk, C.c_int64), _P(hl, C.c_float), _P(hx, C.c_float) if centres else None)
    else:
        key = torch.empty(shape, dtype=torch.int64, device=device)
        l = torch.empty(shape, dtype=torch.float32, device=device)
        xyz = torch.empty(shape + (3,), dtype=torch.float32, device=device) if centres else None
        call(cap, _ptr(key), _ptr(l), _ptr(xyz))
        hk, hl, hx = key.cpu().numpy(), l.cpu().numpy(), xyz.cpu().numpy() if centres else None
    k = [int(min(c, cap)) for c in n_out[:n]]
    return ([hk[g, :k[g]].copy() for g in range(n)], [hl[g, :k[g]].copy() for g in range(n)],
            [hx[g, :k[g]].copy() for g in range(n)] if centres else None)


def cloud_rows(xyz, npts, n_out, cap, n):
    """the rows a cloud call wrote (arrays [n, cap, ...]) as per-cloud numpy arrays of min(n_out, cap) rows"""
    k = [int(min(c, cap)) for c in n_out[:n]]
    return [xyz[g, :k[g]].copy() for g in range(n)], [npts[g, :k[g]].copy() for g in range(n)]


def load_lc_params(yaml_path):
    """flvis_lc_params_load: the loop-closing block of the reference's yaml files.  Host-only."""
    prm = LcParams()
    err = C.create_string_buffer(256)
    rc = load_library().flvis_lc_params_load(os.fsencode(yaml_path), C.byref(prm), err, 256)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_lc_params_load(%s) failed (%d): %s" % (yaml_path, rc, err.value.decode()))
    return prm
