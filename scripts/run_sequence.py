#!/usr/bin/env python3
"""Runs one EuRoC ASL sequence (stereo + IMU) or KITTI odometry sequence (image_0/ image_1/, no IMU: type_of_vi 4) through the tracker and writes the trajectory the reference's recorder would write
(`stamp x y z qw qx qy qz`, camera pose T_w_c); with ground truth present, prints the Umeyama-aligned ATE.

  run_sequence.py <sequence folder> <config yaml> <out.txt> [--backend hip|cpu] [--frames N] [--local-map] [--imu-out <est.txt>]
                  [--loop-closing --voc <DBoW3 vocabulary file> [--lc-out <keyframes.txt>] [--map-cloud <map.ply> [--leaf 0.08]]
                   [--lc-stereo-unrect] [--lc-traj-out <camera.txt>] [--lc-imu-out <imu.txt>] [--lc-traj-mode anchor|blend]]
                  [--local-map --lm-cloud <cloud.ply> [--lm-cloud-mode all|latest] [--leaf 0.08]]
                  [--batch N]

--imu-out : rigs with an IMU: additionally the IMU-rate trajectory of F2FTracking::imu_feed's outputs (pos_w_i, q_w_i per sample) -- the
/imu_pose topic, which is what the reference's EuRoC launch file records as est.txt (launch/flvis_euroc_mav.launch:83-103) and scores;
with ground truth present its ATE is printed as ate_rmse_m_imu_pose (the body frame itself: no camera-to-body step).

--backend hip : the product (flvis_amd, needs an MI355X)          -- BASELINE.json configs[1..2] on real data
--backend cpu : the CPU restatement under oracle/ (test infrastructure) -- configs[0], "the reference CPU path"
Comparing the two output files with flvis_amd.traj_io.ate_from_files gives the metric's "ATE vs CPU ref".

--loop-closing : the tracker's keyframes additionally go through the loop closing (vo_loopclosing.cpp: the third nodelet of the launch
files) with the vocabulary of --voc (.dbow3 / .txt / .yml[.gz]) and the lcKF* / ratio* / min* block of the yaml; the keyframe path it
maintains (T_w_c of every keyframe, corrected by the pose graph whenever a loop closes) is written to --lc-out in the same format.
hip: flvis_loop_closer; cpu: the same control flow assembled from the oracle's functions (tests/_loop_chain.py).

--lc-stereo-unrect : unrectified stereo rigs (cam_type 1: EuRoC).  The reference's loop closing leaves their case empty -- no keyframe gets a
landmark and no loop is ever verified, which stays the default here.  With this switch the keyframes' landmarks come from this project's
rule: LK into the raw second image, both ends undistorted into the rectified plane, DLT (hip: flvis_loop_closer_set_stereo_unrect; cpu:
the checker composed from the oracle's functions, tests/_lc_unrect.py).

--lc-traj-out / --lc-imu-out : (hip) the FULL-RATE trajectories in the map frame, next to the keyframe path of --lc-out: every frame of the
tracker's record (flvis_loop_closer_map_trajectory: no pose goes through the host) and every /imu_pose row (flvis_loop_closer_map_poses_host),
each with the drift of the keyframe it follows -- --lc-traj-mode anchor, the reference's tf rule per keyframe -- or blended between that
keyframe's drift and the next one's (blend: no jump at a keyframe).  Same `stamp x y z qw qx qy qz` writer; with ground truth present
their ATE is printed beside the odometry's (ate_rmse_m_lc_traj, ate_rmse_m_lc_imu_pose).  The keyframes' stamps are the frames' times:
set per keyframe (flvis_loop_closer_set_keyframe_stamps), or with --batch taken from the log.  --lc-imu-out goes without --batch.

--map-cloud : (hip) the corrected map next to the corrected keyframe path: the landmarks of every keyframe in the map frame, one point per
voxel of --leaf metres (0: every landmark, what the reference's /map_cloud carries), as ASCII PLY with the voxels' point counts
(flvis_loop_closer_map_cloud, flvis_amd.traj_io.write_ply).

--lm-cloud : (hip, with --local-map) the local map's own /map_cloud, which the reference publishes when the yaml says
output_sparse_map: True (vo_localmap.cpp:329-377): the optimised multi-view landmarks of every window optimisation, kept on the device
(flvis_local_map_cloud_enable) and fetched once at the end (flvis_local_map_cloud), as ASCII PLY.  --lm-cloud-mode all: every recorded
estimate, the reference's cloud; latest: each landmark's newest estimate.  --leaf is shared with --map-cloud and defaults to 0.08: the
file is then the voxel-filtered cloud; the reference's raw /map_cloud, point for point, is --lm-cloud-mode all --leaf 0.
--lm-cloud-points: the record's capacity in points (32 bytes each; default 2^22), which the device record needs up front; a run that
outgrows it is reported as runs_dropped in the JSON line.  When the yaml sets the key and no file is named, the JSON line says so.

--dense-cloud FILE.ply : (hip, depth rigs -- cam_type 2 -- with --batch) the dense map: every logged keyframe's depth image back-projected
and voxel-filtered on the device, as ASCII PLY with the voxels' sample counts.  Every --dense-step'th pixel of every --dense-step'th row
(default 7, the reference's octomap feeder) between 0.3 m and the config's depth range (dr_para[1]), one point per voxel of --leaf metres.
With --loop-closing the keyframes enter with the closer's stored poses (flvis_loop_closer_dense_cloud: the map frame), otherwise with the
logged ones (flvis_keyframe_log_depth_cloud).  The log then holds the whole run (one entry per frame at most; 3 bytes per pixel and
entry) and is handed to the closer once, after the last chunk, instead of chunk by chunk.

--dense-stereo FILE.ply : (hip, stereo rigs -- cam_type 0 and 1 -- with --batch) the same dense map on a stereo rig: every logged
keyframe's pair through the dense matcher (flvis_hip_dense_stereo; --stereo-disp disparities, default 64, the other parameters at their
defaults, depth in millimetres), then as --dense-cloud (flvis_keyframe_log_stereo_cloud / flvis_loop_closer_stereo_cloud).  Not both
in one run: a rig has a depth image or a second view.  The EuRoC rig (cam_type 1) logs an unrectified pair: it is rectified on the device
in front of the matcher (flvis_keyframe_log_unrect_stereo_cloud / flvis_loop_closer_unrect_stereo_cloud).

--occupancy FILE.ply [--occupancy-leaf L] : (hip, depth rigs -- cam_type 2 -- with --batch) the occupancy map of the same logged
keyframes: every valid sample of --dense-cloud's sampling is a ray from the camera, the voxels it crosses are seen free and its end voxel
occupied, one clamped log-odds value per voxel of L metres (default 0.08; flvis_keyframe_log_occupancy, or with --loop-closing
flvis_loop_closer_occupancy under the closer's stored poses).  The file holds the centres of the voxels with log-odds > 0; the JSON line
counts occupied, free and all voxels.  Goes with or without --dense-cloud; the log holds the whole run as for that option.
--occupancy-path-check : with --occupancy, the straight segments between consecutive keyframe positions (the logged poses, or with
--loop-closing the closer's stored ones) are cast through the finished map on the device (flvis_hip_occupancy_cast, unknown cells
stop a segment); the JSON line gets the segments per status under occupancy.path_check.  The vehicle flew there: an OCCUPIED segment
is a finding about the map.

--batch N : (hip) the frames go through flvis_run_steps in chunks of N -- the host sees nothing between the steps of a chunk -- with the
keyframe log on (flvis_keyframe_log_enable, N entries): after each chunk the loop closing takes the chunk's keyframes from the log on the
device (flvis_loop_closer_add_logged: the images the tracker worked on, img0 after equalizeHist where the rig uses it, as the KeyFrame
message carries them) and the log is cleared.  Not with --imu-out (the IMU-rate rows are fetched per frame).  Without --batch: one
flvis_image_feed per frame, the closer fed the caller's own images, as before."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from flvis_amd import traj_io  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sequence")
    ap.add_argument("config")
    ap.add_argument("out")
    ap.add_argument("--backend", choices=["hip", "cpu"], default="hip")
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--local-map", action="store_true")
    ap.add_argument("--loop-closing", action="store_true")
    ap.add_argument("--voc", default=None)
    ap.add_argument("--lc-out", default=None)
    ap.add_argument("--imu-out", default=None)
    ap.add_argument("--map-cloud", default=None)
    ap.add_argument("--leaf", type=float, default=0.08)
    ap.add_argument("--lc-stereo-unrect", action="store_true")
    ap.add_argument("--lm-cloud", default=None)
    ap.add_argument("--lm-cloud-mode", choices=["all", "latest"], default="all")
    ap.add_argument("--lm-cloud-points", type=int, default=1 << 22)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--dense-cloud", default=None)
    ap.add_argument("--dense-stereo", default=None)
    ap.add_argument("--stereo-disp", type=int, default=64)
    ap.add_argument("--dense-step", type=int, default=7)
    ap.add_argument("--occupancy", default=None)
    ap.add_argument("--occupancy-leaf", type=float, default=0.08)
    ap.add_argument("--occupancy-path-check", action="store_true")
    ap.add_argument("--lc-traj-out", default=None)
    ap.add_argument("--lc-imu-out", default=None)
    ap.add_argument("--lc-traj-mode", choices=["anchor", "blend"], default="anchor")
    args = ap.parse_args()
    if (args.lc_traj_out or args.lc_imu_out) and not (args.loop_closing and args.backend == "hip"):
        ap.error("--lc-traj-out / --lc-imu-out need --loop-closing and --backend hip")
    if args.lc_stereo_unrect and not args.loop_closing:
        ap.error("--lc-stereo-unrect needs --loop-closing")
    if args.loop_closing and not args.voc:
        ap.error("--loop-closing needs --voc <vocabulary file>")
    if args.map_cloud and not (args.loop_closing and args.backend == "hip"):
        ap.error("--map-cloud needs --loop-closing and --backend hip")
    if args.lm_cloud and not (args.local_map and args.backend == "hip"):
        ap.error("--lm-cloud needs --local-map and --backend hip")
    if args.batch and (args.backend != "hip" or args.imu_out or args.lc_imu_out or args.batch < 0):
        ap.error("--batch N (N > 0) needs --backend hip and goes without --imu-out and --lc-imu-out")
    if args.dense_cloud and not (args.batch and args.backend == "hip" and args.dense_step >= 1):
        ap.error("--dense-cloud needs --backend hip, --batch N and --dense-step >= 1")
    if args.dense_stereo and (args.dense_cloud or not (args.batch and args.backend == "hip" and args.dense_step >= 1)):
        ap.error("--dense-stereo needs --backend hip, --batch N and --dense-step >= 1, and goes without --dense-cloud")
    if args.occupancy and (args.dense_stereo or not (args.batch and args.backend == "hip" and args.dense_step >= 1 and args.occupancy_leaf > 0)):
        ap.error("--occupancy needs --backend hip, --batch N, --dense-step >= 1 and --occupancy-leaf > 0, and goes without --dense-stereo")
    if args.occupancy_path_check and not args.occupancy:
        ap.error("--occupancy-path-check needs --occupancy")
    dense_out = args.dense_cloud or args.dense_stereo
    keep_log = dense_out or args.occupancy                         # (any of them: the log keeps the whole run)
    seq = traj_io.open_sequence(args.sequence)
    kitti = isinstance(seq, traj_io.KittiSequence)
    stamps, pos, quat = [], [], []
    imu_rows = []            # (t, q_w_i wxyz, pos_w_i, vel_w_i) per IMU sample
    if args.backend == "cpu":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _oracle as O
        cfg = O.load_config(args.config)
        imu_type = {1: 1, 3: 0, 5: 2, 0: 0, 2: 2, 4: 3}[cfg.type_of_vi]
        trk = O.Tracker(cfg, 0xF1715)
        closer, lc_events, kf_stamps = None, [], []
        if args.loop_closing:
            import flvis_amd
            import _loop_chain as LC
            from test_oracle_bow import RefVoc
            v = flvis_amd.read_vocabulary_file(args.voc)              # (host-side file reader of the product library)
            rv = RefVoc((v["child_ptr"], v["child_idx"], v["desc"], v["weight"], v["word_id"]))
            prm = flvis_amd.load_lc_params(args.config)
            P0, P1 = np.array(list(cfg.P0)), np.array(list(cfg.P1))
            K4 = np.array([P0[0], P0[5], P0[2], P0[6]])
            closer = LC.RefLoopCloser(K4, {k: getattr(prm, k) for k, _ in prm._fields_})
            if args.lc_stereo_unrect:
                if cfg.cam_type != 1:
                    ap.error("--lc-stereo-unrect: the config's rig is not unrectified stereo (cam_type 1)")
                import _lc_unrect as U
                unrect_cam = U.cam_of(cfg)
        for t, i0, i1, imu in seq.frames(0, args.frames):
            for r in imu:
                a, g = traj_io.sensor_to_flvis_imu(imu_type, r[4:7], r[1:4])
                imu_rows.append(np.concatenate([[r[0]], trk.imu(r[0], a, g)]))
            res = trk.image(t, i0, i1)
            if closer is not None and res["new_keyframe"]:
                k, d = O.orb_detect_and_compute(i0)
                if args.lc_stereo_unrect:
                    k, d = k[:1024], d[:1024]                                  # (the closer's keyframe capacity)
                    f = U.check(i0, i1, k, d, unrect_cam)
                    lm2, lm3, lmd = f["lm2"], f["lm3"], f["lmd"]
                else:
                    lm2, lm3, lmd = O.lc_keyframe_landmarks(i0, i1, cfg.cam_type, k, d, P0, P1, K4)
                closer.add(dict(bow=rv.transform(d), lm2=lm2, lm3=lm3, lmd=lmd), res["pose7"])
                lc_events.append(closer.process())
                kf_stamps.append(t)
            if res["state"] == 1:
                stamps.append(t)
                p7 = res["pose7"]
                R = traj_io.quat_to_rot(p7[6], p7[3], p7[4], p7[5])           # T_c_w
                pos.append(-R.T @ p7[:3])
                quat.append(traj_io.rot_to_quat(R.T))
        traj_io.write_stamped(args.out, stamps, pos, quat)
        imu_rows = np.array(imu_rows).reshape(-1, 11)
        if args.imu_out and len(imu_rows):
            traj_io.write_stamped(args.imu_out, imu_rows[:, 0], imu_rows[:, 5:8], imu_rows[:, 1:5])
        T_imu_cam = np.array(list(cfg.T_imu_cam0)).reshape(4, 4)
        kf_T_c_w = np.array(closer.T_c_w).reshape(-1, 7) if closer is not None else None
        kf_landmarks = [len(f["lm2"]) for f in closer.kfs] if closer is not None else []
    else:
        import torch
        import flvis_amd
        cfg = flvis_amd.load_config(args.config)
        ctx = flvis_amd.Context(0)
        n = len(seq) if args.frames is None else min(len(seq), args.frames)
        trk = flvis_amd.Tracker(ctx, cfg, 1, traj_capacity=n)
        if args.lm_cloud:
            trk.local_map_cloud_enable(args.lm_cloud_points)
        closer, lc_events, kf_stamps = None, [], []
        if args.loop_closing:
            ctx.bow_load_vocabulary(args.voc)                                  # Vocabulary voc(path), vo_loopclosing.cpp:1097
            closer = flvis_amd.LoopCloser(ctx, cfg, flvis_amd.load_lc_params(args.config), n_streams=1, max_keyframes=max(n, 1))
            if args.lc_stereo_unrect:
                closer.set_stereo_unrect(True)                                 # (FlvisError on a rig that is not cam_type 1)
        if (args.dense_cloud or args.occupancy) and cfg.cam_type != 2:
            ap.error("--dense-cloud / --occupancy: the config's rig has no depth image (cam_type 2)")
        if args.dense_stereo and cfg.cam_type not in (0, 1):
            ap.error("--dense-stereo: the config's rig is no stereo pair (cam_type 0 or 1)")
        if args.batch:
            trk.keyframe_log_enable(max(n, 1) if keep_log else args.batch)  # (the dense map reads the whole run's log at the end)
            imu_type = {1: 1, 3: 0, 5: 2, 0: 0, 2: 2, 4: 3}[cfg.type_of_vi]
            dropped_logged, chunk = 0, []

            def flush(last=False):
                """the chunk through run_steps; its keyframes from the log into the closer; the log cleared"""
                nonlocal dropped_logged
                if not chunk and not (last and keep_log):
                    return
                if chunk:
                    trk.run_steps(chunk, with_local_map=args.local_map)
                if keep_log and not last:                               # (the log keeps the run; the closer gets it after the last chunk)
                    ctx.synchronize()
                    del chunk[:]
                    return
                info = trk.keyframe_log_info(0)
                dropped_logged += info["dropped"]
                if closer is not None:
                    kf_stamps.extend(trk.keyframe_log_get(0, i, images=False)["stamp"] for i in range(info["logged"]))
                    rounds = max(info["logged"], 1) if keep_log else args.batch
                    lc_events.extend(r[0] for r in closer.add_logged(process=True, max_rounds=rounds))
                if not keep_log:
                    trk.keyframe_log_clear([0])
                del chunk[:]
        for t, i0, i1, imu in seq.frames(0, n):
            if args.batch:
                smp = np.zeros((1, max(len(imu), 1), 7))
                for j, r in enumerate(imu):
                    a, g = traj_io.sensor_to_flvis_imu(imu_type, r[4:7], r[1:4])
                    smp[0, j] = np.concatenate([[r[0]], a, g])
                chunk.append((torch.from_numpy(i0[None]).cuda(), torch.from_numpy(i1[None]).cuda(), [t], np.array([len(imu)], np.int32), smp))
                if len(chunk) == args.batch:
                    flush()
                continue
            for r in imu:
                trk.imu_feed_sensor(0, r[0], r[4:7], r[1:4])                   # the library applies the axis remap
            d0, d1 = torch.from_numpy(i0[None]).cuda(), torch.from_numpy(i1[None]).cuda()
            res = trk.image_feed(d0, d1, [t], want_out=closer is not None, with_local_map=args.local_map)
            if (args.imu_out or args.lc_imu_out) and len(imu):
                imu_rows.append(trk.imu_states(0)[0])
            if closer is not None and res[0]["new_keyframe"]:
                kid = closer.add_keyframes([0], d0, d1, [res[0]["pose7"]])
                closer.set_keyframe_stamps(0, int(kid[0]), [t])
                lc_events.append(closer.process()[0])
                kf_stamps.append(t)
        if args.batch:
            flush(last=True)
        trk.write_trajectory(0, 0, n, args.out, 0)
        imu_rows = np.concatenate(imu_rows) if imu_rows else np.zeros((0, 11))
        if args.imu_out and len(imu_rows):
            trk.write_imu_trajectory(imu_rows, args.imu_out)
        kf_T_c_w = closer.poses(0) if closer is not None else None
        lc_traj, lc_imu = None, None
        lc_mode = flvis_amd.LC_TRAJ_BLEND if args.lc_traj_mode == "blend" else flvis_amd.LC_TRAJ_ANCHOR
        if args.lc_traj_out:
            rows9 = closer.map_trajectory([0], 0, n, lc_mode)[0][0]
            rows9 = rows9[(rows9[:, 8].astype(np.int64) & 15) == 1]            # only frames of a TRACKING stream carry a pose
            lc_pos, lc_quat = [], []
            for p7 in rows9[:, 1:8]:
                R = traj_io.quat_to_rot(p7[6], p7[3], p7[4], p7[5])
                lc_pos.append(-R.T @ p7[:3])
                lc_quat.append(traj_io.rot_to_quat(R.T))
            traj_io.write_stamped(args.lc_traj_out, rows9[:, 0], lc_pos, lc_quat)
            lc_traj = (rows9[:, 0], np.asarray(lc_pos).reshape(-1, 3), np.asarray(lc_quat).reshape(-1, 4))
        if args.lc_imu_out and len(imu_rows):
            lc_imu = closer.map_poses([(0, flvis_amd.LC_ROWS_IMU11, imu_rows)], lc_mode, host=True)[0][0]
            traj_io.write_stamped(args.lc_imu_out, lc_imu[:, 0], lc_imu[:, 5:8], lc_imu[:, 1:5])
        kf_landmarks = [len(closer.keyframe(0, i)["lm2"]) for i in range(len(kf_stamps))] if args.lc_stereo_unrect else []
        map_cloud = None
        if args.map_cloud:
            xyz, npts, n_out, n_drop = closer.map_cloud([[0]], leaf=args.leaf)
            traj_io.write_ply(args.map_cloud, xyz[0], npts[0])
            map_cloud = {"points": int(n_out[0]), "dropped": int(n_drop[0]), "leaf": args.leaf}
        dense_cloud = None
        if dense_out:
            sampling = dict(step=args.dense_step, z_min=0.3, z_max=float(cfg.dr_para[1]), leaf=args.leaf)
            if args.dense_stereo:
                sampling.update(n_disp=args.stereo_disp, depth_factor=1000.0)
                if cfg.cam_type == 1:                                          # (EuRoC: the logged pair is rectified in front of the matcher)
                    got = (closer.unrect_stereo_cloud([[0]], **sampling) if closer is not None else
                           trk.keyframe_log_unrect_stereo_cloud([0], **sampling))
                else:
                    got = closer.stereo_cloud([[0]], **sampling) if closer is not None else trk.keyframe_log_stereo_cloud([0], **sampling)
            else:
                got = closer.dense_cloud([[0]], **sampling) if closer is not None else trk.keyframe_log_depth_cloud([0], **sampling)
            traj_io.write_ply(dense_out, got[0][0], got[1][0])
            dense_cloud = {"points": int(got[2][0]), "dropped": int(got[3][0]), "valid_samples": int(got[4][0]), "leaf": args.leaf,
                           "step": args.dense_step, "keyframes": trk.keyframe_log_info(0)["logged"],
                           "frame": "map" if closer is not None else "odometry", "from": "stereo" if args.dense_stereo else "depth"}
        occupancy = None
        if args.occupancy:
            sampling = dict(step=args.dense_step, z_min=0.3, z_max=float(cfg.dr_para[1]), leaf=args.occupancy_leaf)
            got = closer.occupancy([[0]], **sampling) if closer is not None else trk.keyframe_log_occupancy([0], **sampling)
            l, centres = got[1][0], got[2][0]
            traj_io.write_ply(args.occupancy, centres[l > 0])
            occupancy = {"occupied": int((l > 0).sum()), "free": int((l < 0).sum()), "voxels": int(got[3][0]), "rays": int(got[4][0]),
                         "dropped_rays": int(got[5][0]), "batches": got[6], "leaf": args.occupancy_leaf, "step": args.dense_step,
                         "keyframes": trk.keyframe_log_info(0)["logged"], "frame": "map" if closer is not None else "odometry"}
            if args.occupancy_path_check:
                logged = trk.keyframe_log_info(0)["logged"]
                poses = closer.poses(0) if closer is not None else [trk.keyframe_log_get(0, i, images=False)["pose7"] for i in range(logged)]
                path = traj_io.path_segments(poses)
                counts = ctx.occupancy_cast([(got[0][0], l)], [path], args.occupancy_leaf, outputs=False)[6][0]
                occupancy["path_check"] = dict(zip(flvis_amd.OCCUPANCY_CAST_STATUS, (int(c) for c in counts)), segments=len(path))
        lm_cloud = None
        if args.lm_cloud:
            trk.local_map_counts()                                             # (drains the keyframe queue: the last optimisations too)
            xyz, npts, n_out, n_drop = trk.local_map_cloud([0], args.lm_cloud_mode, leaf=args.leaf)
            traj_io.write_ply(args.lm_cloud, xyz[0], npts[0])
            info = trk.local_map_cloud_info(0)
            lm_cloud = {"points": int(n_out[0]), "dropped": int(n_drop[0]), "leaf": args.leaf, "mode": args.lm_cloud_mode,
                        "recorded_points": info["points"], "runs": info["runs"], "runs_dropped": info["dropped"]}
        T_imu_cam = np.array(list(cfg.T_imu_cam0)).reshape(4, 4)
        stamps, pos, quat = traj_io.read_stamped(args.out)
    out = {"backend": args.backend, "frames": len(seq) if args.frames is None else args.frames, "tracked": len(stamps)}
    if args.backend == "hip":
        import flvis_amd
        if args.batch:
            out["batch"] = {"steps": args.batch, "keyframes_dropped_by_the_log": dropped_logged}
        try:
            wants_cloud = flvis_amd.config_get_bool(args.config, "output_sparse_map")
        except flvis_amd.FlvisError:
            wants_cloud = False                                                # (a yaml without the key: the reference would refuse it)
        if dense_out:
            out["dense_cloud"] = dense_cloud
        if args.occupancy:
            out["occupancy"] = occupancy
        if args.lm_cloud:
            out["local_map_cloud"] = lm_cloud
        elif wants_cloud:
            out["local_map_cloud"] = "output_sparse_map is set in the yaml: --local-map --lm-cloud <file.ply> writes the cloud"
    if args.loop_closing:
        kf_pos, kf_quat = [], []
        for p7 in kf_T_c_w:
            R = traj_io.quat_to_rot(p7[6], p7[3], p7[4], p7[5])
            kf_pos.append(-R.T @ p7[:3])
            kf_quat.append(traj_io.rot_to_quat(R.T))
        if args.lc_out:
            traj_io.write_stamped(args.lc_out, kf_stamps, kf_pos, kf_quat)
        out["loop_closing"] = {"keyframes": len(kf_stamps), "candidates": int(sum(bool(e["candidate"]) for e in lc_events)),
                               "loops_accepted": int(sum(bool(e["accepted"]) for e in lc_events)),
                               "pose_graph_runs": int(sum(bool(e["optimised"]) for e in lc_events))}
        if args.lc_stereo_unrect:
            out["loop_closing"]["stereo_unrect_landmarks"] = int(sum(kf_landmarks))
        if args.map_cloud:
            out["loop_closing"]["map_cloud"] = map_cloud
        if args.lc_traj_out or args.lc_imu_out:
            out["loop_closing"]["trajectory_mode"] = args.lc_traj_mode
    if seq.groundtruth is not None and len(stamps) >= 3:
        gt_t, gt_p, _ = seq.groundtruth
        if kitti:   # KITTI ground truth is the camera itself
            body_p = np.asarray(pos)
        else:
            body_p, _ = traj_io.camera_to_body(np.asarray(pos), np.asarray(quat), T_imu_cam)
        ia, ib = traj_io.associate(np.asarray(stamps), gt_t, 0.02)
        if len(ia) >= 3:
            out["ate_rmse_m"] = traj_io.ate_rmse(body_p[ia], gt_p[ib])
            out["associated"] = int(len(ia))
        if args.imu_out and len(imu_rows) >= 3:       # /imu_pose: the trajectory the reference records and scores on EuRoC
            ja, jb = traj_io.associate(imu_rows[:, 0], gt_t, 0.02)
            if len(ja) >= 3:
                out["ate_rmse_m_imu_pose"] = traj_io.ate_rmse(imu_rows[ja, 5:8], gt_p[jb])
                out["associated_imu_pose"] = int(len(ja))
        if args.loop_closing and len(kf_stamps) >= 3:
            kp = np.asarray(kf_pos) if kitti else traj_io.camera_to_body(np.asarray(kf_pos), np.asarray(kf_quat), T_imu_cam)[0]
            ka, kb = traj_io.associate(np.asarray(kf_stamps), gt_t, 0.02)
            if len(ka) >= 3:
                out["loop_closing"]["ate_rmse_m_keyframe_path"] = traj_io.ate_rmse(kp[ka], gt_p[kb])
        if args.lc_traj_out and len(lc_traj[0]) >= 3:   # the corrected full-rate trajectories, beside ate_rmse_m / ate_rmse_m_imu_pose
            lp = lc_traj[1] if kitti else traj_io.camera_to_body(lc_traj[1], lc_traj[2], T_imu_cam)[0]
            la, lb = traj_io.associate(lc_traj[0], gt_t, 0.02)
            if len(la) >= 3:
                out["loop_closing"]["ate_rmse_m_lc_traj"] = traj_io.ate_rmse(lp[la], gt_p[lb])
        if args.lc_imu_out and lc_imu is not None and len(lc_imu) >= 3:
            ma, mb = traj_io.associate(lc_imu[:, 0], gt_t, 0.02)
            if len(ma) >= 3:
                out["loop_closing"]["ate_rmse_m_lc_imu_pose"] = traj_io.ate_rmse(lc_imu[ma, 5:8], gt_p[mb])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
