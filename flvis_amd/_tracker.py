"""Tracker: the batched F2FTracking + LocalMap of a context (flvis_tracker_create and the per-frame entry points)."""
import ctypes as C

import numpy as np

from ._loader import FlvisError, _P, _ptr
from ._structs import FlvisCfg, FlvisImage, FlvisKeyframe, FlvisStep, FrameOut, cloud_rows, dense_stereo_params, depth_cloud_params, occupancy_params, occupancy_rows


class Tracker:
    """Batched F2FTracking + LocalMap for n_streams independent streams on one GPU (flvis_tracker_create).

    cfg: one config for every stream, or a sequence of n_streams configs -- one per stream, each camera with its own calibration
    (flvis_tracker_create_rigs: the batch-wide fields must agree, FlvisError otherwise).  self.cfg is stream 0's."""

    def __init__(self, ctx, cfg, n_streams, seed_base=0xF1715, traj_capacity=0):
        self.ctx = ctx
        self.lib = ctx._lib
        self.S = n_streams
        if isinstance(cfg, FlvisCfg):
            self.cfg = cfg
            ctx._check(self.lib.flvis_tracker_create(ctx._h, C.byref(cfg), n_streams, seed_base, traj_capacity),
                       "tracker_create")
        else:
            cfgs = list(cfg)
            if len(cfgs) != n_streams:
                raise ValueError("Tracker: %d configs for %d streams" % (len(cfgs), n_streams))
            self.cfg = cfgs[0]
            arr = (FlvisCfg * n_streams)(*cfgs)
            ctx._check(self.lib.flvis_tracker_create_rigs(ctx._h, arr, n_streams, seed_base, traj_capacity), "tracker_create_rigs")
        self._out = (FrameOut * n_streams)()

    def imu_feed_flvis(self, stream, samples7):
        a = np.ascontiguousarray(samples7, np.float64).reshape(-1, 7)
        if len(a):
            self.ctx._check(self.lib.flvis_imu_feed_flvis_frame(self.ctx._h, stream, len(a), _P(a, C.c_double)),
                            "imu_feed")

    def imu_feed_sensor(self, stream, t, acc, gyro):
        a = (C.c_double * 3)(*[float(x) for x in acc])
        g = (C.c_double * 3)(*[float(x) for x in gyro])
        self.ctx._check(self.lib.flvis_imu_feed(self.ctx._h, stream, t, a, g), "imu_feed")

    def imu_feed_out(self, stream, t, acc, gyro):
        """F2FTracking::imu_feed with its outputs: integrates the sensor-frame sample now; returns (q_w_i wxyz, pos_w_i, vel_w_i)."""
        a = (C.c_double * 3)(*[float(x) for x in acc])
        g = (C.c_double * 3)(*[float(x) for x in gyro])
        q, p, v = np.zeros(4), np.zeros(3), np.zeros(3)
        self.ctx._check(self.lib.flvis_imu_feed_out(self.ctx._h, stream, t, a, g, _P(q, C.c_double), _P(p, C.c_double),
                                                    _P(v, C.c_double)), "imu_feed_out")
        return q, p, v

    def imu_states(self, stream, cap=512):
        """Rows (t, q_w_i wxyz, pos_w_i, vel_w_i) of the IMU samples integrated since the previous call; also the rows lost."""
        rows = np.zeros((cap, 11), np.float64)
        n, dropped = C.c_int(0), C.c_int(0)
        self.ctx._check(self.lib.flvis_get_imu_states(self.ctx._h, stream, cap, _P(rows, C.c_double), C.byref(n), C.byref(dropped)),
                        "get_imu_states")
        return rows[:n.value].copy(), dropped.value

    def debug_vi_state(self, stream, cap=400):
        """Test aid (flvis_debug_vi_state): the stream's filter after the staged samples -> dict(rows [n, 11] oldest first as
        (t, q_w_i wxyz, pos_w_i, vel_w_i), biases [6] (acc, gyro), flags [4] (has_imu, vi_first, vi_initialized, vi_count))."""
        rows, biases, flags = np.zeros((cap, 11), np.float64), np.zeros(6, np.float64), np.zeros(4, np.int32)
        n = self.lib.flvis_debug_vi_state(self.ctx._h, stream, cap, _P(rows, C.c_double), _P(biases, C.c_double), _P(flags, C.c_int32))
        if n < 0:
            self.ctx._check(n, "debug_vi_state")
        return dict(rows=rows[:min(n, cap)].copy(), biases=biases, flags=flags)

    def local_map_counts(self):
        """(keyframes emitted, local-map optimisations run) per stream"""
        kf, ba = np.zeros(self.S, np.int64), np.zeros(self.S, np.int64)
        self.ctx._check(self.lib.flvis_get_local_map_counts(self.ctx._h, _P(kf, C.c_int64), _P(ba, C.c_int64)), "get_local_map_counts")
        return kf, ba

    def write_imu_trajectory(self, rows11, path, min_dt=0.0, append=False, t_first=None):
        """The recorder on /imu_pose: rows of imu_states() as `stamp x y z qw qx qy qz` lines; returns the lines written.
        t_first: the stamp of the run's first row (flvis_write_imu_trajectory_run) -- pass it with every batch of a run whose first
        batch may cover less than min_dt."""
        r = np.ascontiguousarray(rows11, np.float64).reshape(-1, 11)
        if t_first is not None:
            n = self.lib.flvis_write_imu_trajectory_run(_P(r, C.c_double), len(r), path.encode(), min_dt, bool(append), t_first)
        else:
            n = self.lib.flvis_write_imu_trajectory(_P(r, C.c_double), len(r), path.encode(), min_dt, bool(append))
        if n < 0:
            raise FlvisError("write_imu_trajectory failed (%d)" % n)
        return n

    def _presence(self, present, shape):
        """present (sequence of truth values, `shape`) as the uint8 array the _present entry points take, or None for None."""
        if present is None:
            return None
        pr = (np.asarray(present) != 0).astype(np.uint8)
        assert pr.shape == shape, "present must have shape %s" % (shape,)
        return np.ascontiguousarray(pr)

    def image_feed(self, img0, img1, times, want_out=True, with_local_map=True, present=None):
        """img0/img1: uint8 cuda tensors [S,H,W]; times: sequence of S floats.  present (optional, S truth values): only the streams
        marked present have a frame in this step (flvis_image_feed_present); None: all of them."""
        assert img0.is_cuda and img0.is_contiguous() and img1.is_contiguous() and img0.shape[0] == self.S
        t = np.ascontiguousarray(times, np.float64)
        out = self._out if want_out else None
        pr = self._presence(present, (self.S,))
        if pr is None:
            rc = self.lib.flvis_image_feed(self.ctx._h, _ptr(img0), _ptr(img1), _P(t, C.c_double), out, bool(with_local_map))
        else:
            rc = self.lib.flvis_image_feed_present(self.ctx._h, _ptr(img0), _ptr(img1), _P(t, C.c_double), pr.ctypes.data, out,
                                                   bool(with_local_map))
        self.ctx._check(rc, "image_feed")
        return self._frame_outs() if want_out else None

    def run_steps(self, steps, with_local_map=True, present=None):
        """flvis_run_steps: a batch of frames whose images are already in HBM, one C call (what bench.py times).  steps: a sequence of
        (img0, img1, times[, imu_counts, imu_samples]) -- uint8 cuda tensors [S,H,W], S floats, and optionally the IMU samples of the
        step for all streams (int32 [S], float64 [S, n, 7]).  The tensors must stay alive until the context is synchronised.
        present (optional, [n_steps][S] truth values): the streams that have a frame in each step (flvis_run_steps_present)."""
        arr = (FlvisStep * len(steps))()
        keep = []
        for j, st in enumerate(steps):
            img0, img1, times = st[0], st[1], st[2]
            assert img0.is_cuda and img0.is_contiguous() and img1.is_contiguous() and img0.shape[0] == self.S
            t = np.ascontiguousarray(times, np.float64)
            keep.append(t)
            arr[j].d_img0, arr[j].d_img1, arr[j].h_times = img0.data_ptr(), img1.data_ptr(), t.ctypes.data
            if len(st) > 3 and st[3] is not None:
                cnt = np.ascontiguousarray(st[3], np.int32)
                smp = np.ascontiguousarray(st[4], np.float64)
                assert cnt.shape == (self.S,) and smp.ndim == 3 and smp.shape[0] == self.S and smp.shape[2] == 7
                keep += [cnt, smp]
                arr[j].h_imu_counts, arr[j].h_imu_samples, arr[j].imu_samples_per_stream = cnt.ctypes.data, smp.ctypes.data, smp.shape[1]
        pr = self._presence(present, (len(steps), self.S))
        if pr is None:
            rc = self.lib.flvis_run_steps(self.ctx._h, len(steps), arr, bool(with_local_map), None)
        else:
            rc = self.lib.flvis_run_steps_present(self.ctx._h, len(steps), arr, pr.ctypes.data, bool(with_local_map), None)
        self.ctx._check(rc, "run_steps")

    def _frame_outs(self):
        return [dict(state=o.state, new_keyframe=bool(o.new_keyframe), reset_cmd=bool(o.reset_cmd),
                     n_landmarks=o.n_landmarks, frame_id=o.frame_id, pose7=np.array(o.T_c_w[:]),
                     dbg=np.array([o.of_inliers, o.f_inliers, o.pnp_inliers]),
                     reprojection_error=o.reprojection_error) for o in self._out]

    def image_feed_host(self, imgs0, imgs1, times, want_out=True, with_local_map=True, hold_buffers=False, present=None):
        """flvis_image_feed_host: the frame handed over as HOST images, the call a nodelet makes (vo_tracking.cpp:396-430).
        imgs0 / imgs1: one numpy array per stream, [H, W] (mono8; uint16 for the depth image of a depth rig) or [H, W, 3|4]
        (BGR / BGRA); rows may be padded (a strided view whose pixels are contiguous).  With hold_buffers the arrays must stay
        untouched until the next call on this context has returned.  present (optional, S truth values): only the streams
        marked present have a frame in this step (flvis_image_feed_host_present); an absent stream's images and time may be None
        (handed over as NULL)."""
        assert len(imgs0) == self.S and len(imgs1) == self.S
        a = (FlvisImage * self.S)()
        b = (FlvisImage * self.S)()
        for arr, imgs in ((a, imgs0), (b, imgs1)):
            for s, im in enumerate(imgs):
                if im is None:  # (NULL data: legal for an absent stream only, the library checks)
                    arr[s].t = float(times[s]) if times[s] is not None else 0.0
                    continue
                px = im.itemsize * (im.shape[2] if im.ndim == 3 else 1)
                assert im.strides[1] == px and (im.ndim == 2 or im.strides[2] == im.itemsize), "pixels of a row must be contiguous"
                arr[s].data = C.cast(im.ctypes.data, C.POINTER(C.c_uint8))
                arr[s].width, arr[s].height, arr[s].pitch = im.shape[1], im.shape[0], im.strides[0]
                arr[s].channels = im.shape[2] if im.ndim == 3 else 1
                arr[s].t = float(times[s])
        out = self._out if want_out else None
        pr = self._presence(present, (self.S,))
        if pr is None:
            rc = self.lib.flvis_image_feed_host(self.ctx._h, a, b, out, bool(with_local_map), bool(hold_buffers))
        else:
            rc = self.lib.flvis_image_feed_host_present(self.ctx._h, a, b, pr.ctypes.data, out, bool(with_local_map), bool(hold_buffers))
        self.ctx._check(rc, "image_feed_host")
        return self._frame_outs() if want_out else None

    def landmarks(self, stream, cap=2048):
        ids = np.zeros(cap, np.int64)
        p2d = np.zeros((cap, 2))
        p2u = np.zeros((cap, 2))
        p3w = np.zeros((cap, 3))
        fl = np.zeros(cap, np.uint8)
        n = self.lib.flvis_get_landmarks(self.ctx._h, stream, cap, _P(ids, C.c_int64), _P(p2d, C.c_double),
                                         _P(p2u, C.c_double), _P(p3w, C.c_double), _P(fl, C.c_uint8))
        if n < 0:
            self.ctx._check(n, "get_landmarks")
        return dict(ids=ids[:n].copy(), p2d=p2d[:n].copy(), p2u=p2u[:n].copy(), p3w=p3w[:n].copy(), flags=fl[:n].copy())

    def keyframe(self, stream, cap=2048):
        fid = C.c_int64(0)
        pose = np.zeros(7)
        ids = np.zeros(cap, np.int64)
        p2u = np.zeros((cap, 2))
        p3w = np.zeros((cap, 3))
        n = self.lib.flvis_get_keyframe(self.ctx._h, stream, cap, C.byref(fid), _P(pose, C.c_double), _P(ids, C.c_int64),
                                        _P(p2u, C.c_double), _P(p3w, C.c_double))
        if n < 0:
            self.ctx._check(n, "get_keyframe")
        return dict(frame_id=fid.value, pose7=pose, lm_id=ids[:n].copy(), lm_2d=p2u[:n].copy(), lm_3d=p3w[:n].copy())

    def correction(self, stream, cap=8192):
        fid = C.c_int64(0)
        pose = np.zeros(7)
        cnt = C.c_int(0)
        ids = np.zeros(cap, np.int64)
        p3 = np.zeros((cap, 3))
        oc = C.c_int(0)
        oid = np.zeros(cap, np.int64)
        r = self.lib.flvis_get_correction(self.ctx._h, stream, cap, C.byref(fid), _P(pose, C.c_double), C.byref(cnt),
                                          _P(ids, C.c_int64), _P(p3, C.c_double), C.byref(oc), _P(oid, C.c_int64))
        if r < 0:
            self.ctx._check(r, "get_correction")
        if r == 0:
            return None
        return dict(frame_id=fid.value, pose7=pose, lm_id=ids[:cnt.value].copy(), lm_3d=p3[:cnt.value].copy(),
                    outlier_id=oid[:oc.value].copy())

    def set_input_hold(self, n_frames):
        """flvis_set_input_hold: multi-lane trackers -- the caller leaves a call's input images untouched during the next n calls."""
        self.ctx._check(self.lib.flvis_set_input_hold(self.ctx._h, int(n_frames)), "set_input_hold")

    def set_imu_factor(self, enable, sigma_gyro=0.002):
        """flvis_set_imu_factor: gyro rotation-preintegration edges between consecutive keyframes in the window BA (off by default)."""
        self.ctx._check(self.lib.flvis_set_imu_factor(self.ctx._h, bool(enable), sigma_gyro), "set_imu_factor")

    def set_imu_factor_accel(self, sigma_acc):
        """flvis_set_imu_factor_accel: position rows of the IMU factor (accelerometer noise density; <= 0: rotation rows only)"""
        self.ctx._check(self.lib.flvis_set_imu_factor_accel(self.ctx._h, sigma_acc), "set_imu_factor_accel")

    def get_keyframe_imu_pos(self, stream):
        """flvis_get_keyframe_imu_pos -> (dp, va): displacement preintegrated since the previous keyframe, that keyframe's velocity"""
        dp, va = np.zeros(3), np.zeros(3)
        r = self.lib.flvis_get_keyframe_imu_pos(self.ctx._h, stream, _P(dp, C.c_double), _P(va, C.c_double))
        if r < 0:
            self.ctx._check(r, "get_keyframe_imu_pos")
        return dp, va

    def get_keyframe_imu(self, stream):
        """flvis_get_keyframe_imu -> (valid, dq (w, x, y, z), dt) of the stream's last keyframe"""
        dq = np.zeros(4)
        dt = C.c_double(0)
        r = self.lib.flvis_get_keyframe_imu(self.ctx._h, stream, _P(dq, C.c_double), C.byref(dt))
        if r < 0:
            self.ctx._check(r, "get_keyframe_imu")
        return bool(r), dq, dt.value

    def ba_push_keyframe(self, stream, frame_id, pose7, lm_id, lm_2d, lm_3d, cap=8192, imu_dq=None, imu_dt=0.0, imu_dp=None, imu_va=None):
        p7 = np.ascontiguousarray(pose7, np.float64)
        ids = np.ascontiguousarray(lm_id, np.int64)
        l2 = np.ascontiguousarray(lm_2d, np.float64)
        l3 = np.ascontiguousarray(lm_3d, np.float64)
        fid = C.c_int64(0)
        pose = np.zeros(7)
        cnt = C.c_int(0)
        oid_ = np.zeros(cap, np.int64)
        o3 = np.zeros((cap, 3))
        oc = C.c_int(0)
        ooid = np.zeros(cap, np.int64)
        if imu_dq is not None and imu_dp is not None:
            dq = np.ascontiguousarray(imu_dq, np.float64)
            dp, va = np.ascontiguousarray(imu_dp, np.float64), np.ascontiguousarray(imu_va, np.float64)
            r = self.lib.flvis_ba_push_keyframe_imu_pos(self.ctx._h, stream, frame_id, _P(p7, C.c_double), _P(dq, C.c_double),
                                                        imu_dt, _P(dp, C.c_double), _P(va, C.c_double), len(ids),
                                                        _P(ids, C.c_int64), _P(l2, C.c_double), _P(l3, C.c_double), cap, C.byref(fid),
                                                        _P(pose, C.c_double), C.byref(cnt), _P(oid_, C.c_int64), _P(o3, C.c_double),
                                                        C.byref(oc), _P(ooid, C.c_int64))
        elif imu_dq is not None:
            dq = np.ascontiguousarray(imu_dq, np.float64)
            r = self.lib.flvis_ba_push_keyframe_imu(self.ctx._h, stream, frame_id, _P(p7, C.c_double), _P(dq, C.c_double),
                                                    imu_dt, len(ids), _P(ids, C.c_int64), _P(l2, C.c_double),
                                                    _P(l3, C.c_double), cap, C.byref(fid), _P(pose, C.c_double), C.byref(cnt),
                                                    _P(oid_, C.c_int64), _P(o3, C.c_double), C.byref(oc), _P(ooid, C.c_int64))
        else:
            r = self.lib.flvis_ba_push_keyframe(self.ctx._h, stream, frame_id, _P(p7, C.c_double), len(ids),
                                                _P(ids, C.c_int64), _P(l2, C.c_double), _P(l3, C.c_double), cap,
                                                C.byref(fid), _P(pose, C.c_double), C.byref(cnt), _P(oid_, C.c_int64),
                                                _P(o3, C.c_double), C.byref(oc), _P(ooid, C.c_int64))
        if r < 0:
            self.ctx._check(r, "ba_push_keyframe")
        if r == 0:
            return None
        return dict(frame_id=fid.value, pose7=pose, lm_id=oid_[:cnt.value].copy(), lm_3d=o3[:cnt.value].copy(),
                    outlier_id=ooid[:oc.value].copy())

    def trajectory(self, stream, first, n):
        rows = np.zeros((n, 9))
        r = self.lib.flvis_get_trajectory(self.ctx._h, stream, first, n, _P(rows, C.c_double))
        if r < 0:
            self.ctx._check(r, "get_trajectory")
        return rows

    def write_trajectory(self, stream, first, n, path, fmt=0, min_dt=0.0):
        """flvis_write_trajectory: fmt 0 = `stamp x y z qw qx qy qz`, 1 = KITTI 12 columns.  Returns lines written."""
        r = self.lib.flvis_write_trajectory(self.ctx._h, stream, first, n, path.encode(), fmt, min_dt)
        if r < 0:
            self.ctx._check(r, "write_trajectory")
        return r

    def correction_feed(self, stream, frame_id, pose7, lm_id, lm_3d, outlier_id):
        """flvis_correction_feed: F2FTracking::correction_feed (opt-in local-map feedback)."""
        pose7 = np.ascontiguousarray(pose7, np.float64)
        lm_id = np.ascontiguousarray(lm_id, np.int64)
        lm_3d = np.ascontiguousarray(lm_3d, np.float64).reshape(-1, 3)
        outlier_id = np.ascontiguousarray(outlier_id, np.int64)
        assert len(lm_id) == len(lm_3d)
        self.ctx._check(self.lib.flvis_correction_feed(self.ctx._h, stream, int(frame_id), _P(pose7, C.c_double), len(lm_id),
                                                       _P(lm_id, C.c_int64), _P(lm_3d, C.c_double), len(outlier_id),
                                                       _P(outlier_id, C.c_int64)), "correction_feed")

    def pose_records(self, stream, cap=1024):
        """flvis_get_pose_records -> rows (frame_id, pose7), oldest first."""
        rows = np.zeros((cap, 8))
        n = self.lib.flvis_get_pose_records(self.ctx._h, stream, cap, _P(rows, C.c_double))
        if n < 0:
            self.ctx._check(n, "get_pose_records")
        return rows[:min(n, cap)].copy()

    def counters(self):
        """[frames fed, keyframes, local-map optimisations]"""
        c = (C.c_int64 * 3)()
        self.ctx._check(self.lib.flvis_get_counters(self.ctx._h, c), "get_counters")
        return list(c)

    def _stream_list(self, streams, what):
        ids = [int(k) for k in streams]
        arr = (C.c_int * max(1, len(ids)))(*ids)
        self.ctx._check(getattr(self.lib, what)(self.ctx._h, len(ids), arr), what[len("flvis_"):])

    def reset_streams(self, streams, cfgs=None):
        """flvis_reset_streams: the named streams start over as streams of a new tracker (the others go on undisturbed); from the next
        frame step on.  FlvisError for an index outside [0, S).  cfgs: one config per named stream, which it starts over on
        (flvis_reset_streams_rigs; FlvisError and nothing changes if one of them fails the checks)."""
        if cfgs is None:
            self._stream_list(streams, "flvis_reset_streams")
            return
        ids = [int(k) for k in streams]
        cfgs = [cfgs] if isinstance(cfgs, FlvisCfg) else list(cfgs)
        if len(cfgs) != len(ids):
            raise ValueError("reset_streams: %d configs for %d streams" % (len(cfgs), len(ids)))
        arr = (C.c_int * max(1, len(ids)))(*ids)
        carr = (FlvisCfg * max(1, len(ids)))(*cfgs)
        self.ctx._check(self.lib.flvis_reset_streams_rigs(self.ctx._h, len(ids), arr, carr), "reset_streams_rigs")

    def stream_cfg(self, s):
        """flvis_get_stream_cfg: the config stream s runs on (as created, or as last reset with reset_streams(..., cfgs))."""
        out = FlvisCfg()
        self.ctx._check(self.lib.flvis_get_stream_cfg(self.ctx._h, int(s), C.byref(out)), "get_stream_cfg")
        return out

    def local_map_reset(self, streams):
        """flvis_local_map_reset: KFMSG_CMD_RESET_LM for the named streams' local maps (what is queued ahead is processed first)."""
        self._stream_list(streams, "flvis_local_map_reset")

    def local_map_cloud_enable(self, max_points):
        """flvis_local_map_cloud_enable: keep every optimisation's multi-view landmarks on the device, max_points per stream (<= 0: off)."""
        self.ctx._check(self.lib.flvis_local_map_cloud_enable(self.ctx._h, int(max_points)), "local_map_cloud_enable")

    def local_map_cloud_clear(self, streams):
        """flvis_local_map_cloud_clear: empties the named streams' records."""
        self._stream_list(streams, "flvis_local_map_cloud_clear")

    def local_map_cloud_info(self, stream):
        """flvis_local_map_cloud_info -> dict(points, runs, dropped, capacity) of the stream's record."""
        v = (C.c_int64 * 4)()
        self.ctx._check(self.lib.flvis_local_map_cloud_info(self.ctx._h, int(stream), v), "local_map_cloud_info")
        return dict(points=int(v[0]), runs=int(v[1]), dropped=int(v[2]), capacity=int(v[3]))

    def local_map_cloud(self, streams, mode="all", leaf=0.0, min_points=1, cap=None, host=False, ids=False):
        """flvis_local_map_cloud: the named streams' recorded map clouds.  mode "all": every recorded entry in record order (the
        reference's /map_cloud); "latest": one entry per landmark id, from the newest optimisation that lists it.  leaf = 0: every point
        rounded to float; leaf > 0: one point per voxel of `leaf` metres holding min_points points or more (flvis_hip_voxel_cloud's rule).
        cap: rows per stream (default: what the largest cloud yields, found by a call of its own).  host=True goes through the _host
        entry.  ids=True (leaf 0 only): the rows' landmark ids.
        -> (xyz [n] of float32 [k, 3], npts [n] of int32 [k], n_out int64 [n], n_dropped int64 [n]) and, with ids, ids [n] of int64 [k]."""
        import torch
        modes = {"all": 0, "latest": 1}
        m = modes[mode] if mode in modes else int(mode)
        sl = [int(s) for s in streams]
        n = len(sl)
        arr = np.ascontiguousarray(sl + [0], np.int32)
        if cap is None:
            cap = int(max(list(self.local_map_cloud(sl, m, leaf, min_points, cap=0, host=host)[2]) + [0]))
        cap = int(cap)
        n_out, n_drop = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        shape = (max(n, 1), max(cap, 0))
        head = (self.ctx._h, n, _P(arr, C.c_int), m, leaf, int(min_points), cap)
        if host:
            hx, hn, hi = np.zeros(shape + (3,), np.float32), np.zeros(shape, np.int32), np.zeros(shape, np.int64)
            rc = self.lib.flvis_local_map_cloud_host(*head, _P(hx, C.c_float), _P(hn, C.c_int), _P(hi, C.c_int64) if ids else None,
                                                     _P(n_out, C.c_int64), _P(n_drop, C.c_int64))
            self.ctx._check(rc, "local_map_cloud_host")
        else:
            dev = self.ctx.device
            xyz = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
            npts = torch.empty(shape, dtype=torch.int32, device=dev)
            did = torch.empty(shape, dtype=torch.int64, device=dev) if ids else None
            rc = self.lib.flvis_local_map_cloud(*head, _ptr(xyz), _ptr(npts), _ptr(did) if ids else None, _P(n_out, C.c_int64), _P(n_drop, C.c_int64))
            self.ctx._check(rc, "local_map_cloud")
            kmax = int(min(max(n_out[:n].max() if n else 0, 0), cap))
            hx, hn = xyz[:, :kmax].cpu().numpy(), npts[:, :kmax].cpu().numpy()
            hi = did[:, :kmax].cpu().numpy() if ids else None
        k = [int(min(c, cap)) for c in n_out[:n]]
        out = ([hx[g, :k[g]].copy() for g in range(n)], [hn[g, :k[g]].copy() for g in range(n)], n_out[:n].copy(), n_drop[:n].copy())
        if ids:
            out = out + ([hi[g, :k[g]].copy() for g in range(n)],)
        return out

    def _keyframe_msg(self, call, what, cap, images):
        """a flvis_keyframe call on host arrays -> the message as a dict (None: no keyframe)"""
        h, w = int(self.cfg.image_height), int(self.cfg.image_width)
        ids, p2u, p3w = np.zeros(cap, np.int64), np.zeros((cap, 2)), np.zeros((cap, 3))
        img0 = np.zeros((h, w), np.uint8) if images else None
        img1 = np.zeros((h, w), np.uint16 if self.cfg.cam_type == 2 else np.uint8) if images else None
        kf = FlvisKeyframe()
        n = call(cap, C.byref(kf), _P(ids, C.c_int64), _P(p2u, C.c_double), _P(p3w, C.c_double),
                 img0.ctypes.data if images else None, img1.ctypes.data if images else None)
        if n < 0:
            self.ctx._check(n, what)
        if not kf.lm_id:  # (the call left the message untouched: no keyframe)
            return None
        n = min(n, cap)
        return dict(frame_id=int(kf.frame_id), command=int(kf.command), stamp=float(kf.stamp), pose7=np.array(kf.T_c_w[:]),
                    lm_id=ids[:n].copy(), lm_2d=p2u[:n].copy(), lm_3d=p3w[:n].copy(), img0=img0, img1=img1)

    def keyframe_msg(self, stream, cap=2048, images=True):
        """flvis_get_keyframe_msg: the stream's last keyframe as the flvis/KeyFrame message (call it right after the image_feed that
        reported new_keyframe) -> dict(frame_id, command, stamp, pose7, lm_id, lm_2d, lm_3d, img0, img1), or None when the stream's last
        frame was no keyframe.  img0 / img1: numpy [h, w] (img1 uint16 on a depth rig), None with images=False."""
        fn = self.lib.flvis_get_keyframe_msg
        return self._keyframe_msg(lambda cap_, *a: fn(self.ctx._h, int(stream), cap_, *a), "get_keyframe_msg", cap, images)

    def keyframe_log_enable(self, max_keyframes):
        """flvis_keyframe_log_enable: keep every keyframe's whole message on the device, max_keyframes per stream (<= 0: off)."""
        self.ctx._check(self.lib.flvis_keyframe_log_enable(self.ctx._h, int(max_keyframes)), "keyframe_log_enable")

    def keyframe_log_clear(self, streams):
        """flvis_keyframe_log_clear: empties the named streams' logs."""
        self._stream_list(streams, "flvis_keyframe_log_clear")

    def keyframe_log_info(self, stream):
        """flvis_keyframe_log_info -> dict(logged, dropped, capacity) of the stream's log."""
        v = (C.c_int64 * 3)()
        self.ctx._check(self.lib.flvis_keyframe_log_info(self.ctx._h, int(stream), v), "keyframe_log_info")
        return dict(logged=int(v[0]), dropped=int(v[1]), capacity=int(v[2]))

    def keyframe_log_depth_cloud(self, streams, window=None, step=1, z_min=0.3, z_max=10.0, leaf=0.08, min_points=1, cap=None, host=False,
                                 slices=None, _stereo=None):
        """flvis_keyframe_log_depth_cloud (depth rigs): per listed stream one dense cloud of its logged keyframes' depth images, each
        under its logged T_c_w and the stream's own camera, voxel-filtered on the device (leaf = 0: every valid sample).  window / step /
        z_min / z_max: Context.depth_cloud's.  slices: per stream (first entry, count), None: every entry.  cap: rows per stream
        (default: found by a call of its own).  host=True goes through the _host entry.
        -> (xyz [n] of float32 [k, 3], npts [n] of int32 [k], n_out, n_dropped, n_valid int64 [n])."""
        import torch
        sl = [int(s) for s in streams]
        n = len(sl)
        arr = np.ascontiguousarray(sl + [0], np.int32)
        sli = None if slices is None else np.ascontiguousarray(list(slices) + [(0, 0)], np.int32).reshape(-1, 2)
        assert sli is None or len(sli) == n + 1, "one slice per listed stream"
        prm = depth_cloud_params(window, step, z_min, z_max)
        n_out, n_drop, n_valid = (np.zeros(max(n, 1), np.int64) for _ in range(3))
        kind = "depth" if not _stereo else "unrect_stereo" if len(_stereo) > 2 and _stereo[2] else "stereo"
        what = "keyframe_log_%s_cloud%s" % (kind, "_host" if host else "")
        fn = getattr(self.lib, "flvis_" + what)
        front = (C.byref(_stereo[0]), float(_stereo[1])) if _stereo else ()   # (the stereo forms: the matcher's parameters, depth_factor)
        head = (self.ctx._h, n, _P(arr, C.c_int), _P(sli, C.c_int) if sli is not None else None) + front + (C.byref(prm), leaf, int(min_points))
        tail = (_P(n_out, C.c_int64), _P(n_drop, C.c_int64), _P(n_valid, C.c_int64))
        if cap is None:
            self.ctx._check(fn(*head, 0, None, None, *tail), what)
            cap = int(max(list(n_out[:n]) + [0]))
        cap = int(cap)
        shape = (max(n, 1), max(cap, 0))
        if host:
            hx, hn = np.zeros(shape + (3,), np.float32), np.zeros(shape, np.int32)
            self.ctx._check(fn(*head, cap, _P(hx, C.c_float), _P(hn, C.c_int), *tail), what)
        else:
            xyz = torch.empty(shape + (3,), dtype=torch.float32, device=self.ctx.device)
            npts = torch.empty(shape, dtype=torch.int32, device=self.ctx.device)
            self.ctx._check(fn(*head, cap, _ptr(xyz), _ptr(npts), *tail), what)
            hx, hn = xyz.cpu().numpy(), npts.cpu().numpy()
        rows = cloud_rows(hx, hn, n_out, cap, n)
        return rows + (n_out[:n].copy(), n_drop[:n].copy(), n_valid[:n].copy())

    def keyframe_log_occupancy(self, streams, window=None, step=1, z_min=0.3, z_max=10.0, leaf=0.08, occ=None, max_records=0, cap=None,
                               host=False, slices=None, centres=True):
        """flvis_keyframe_log_occupancy (depth rigs): per listed stream one occupancy map of its logged keyframes' depth images as scans,
        listed as keyframe_log_depth_cloud lists them and walked in batches of at most max_records records (0: 2^26).  occ: an
        OccupancyParams (None: octomap's defaults).  cap: rows per stream (default: found by a call of its own).
        -> (keys [n] of int64 [k], logodds [n] of float32 [k], centres [n] of float32 [k, 3] or None, n_out, n_rays, n_dropped int64 [n],
        the batches run)."""
        sl = [int(s) for s in streams]
        n = len(sl)
        arr = np.ascontiguousarray(sl + [0], np.int32)
        sli = None if slices is None else np.ascontiguousarray(list(slices) + [(0, 0)], np.int32).reshape(-1, 2)
        assert sli is None or len(sli) == n + 1, "one slice per listed stream"
        prm, occ = depth_cloud_params(window, step, z_min, z_max), occupancy_params(occ)
        n_out, n_rays, n_drop = (np.zeros(max(n, 1), np.int64) for _ in range(3))
        batches = C.c_int(0)
        what = "keyframe_log_occupancy" + ("_host" if host else "")
        fn = getattr(self.lib, "flvis_" + what)

        def call(cap, key, l, xyz):
            self.ctx._check(fn(self.ctx._h, n, _P(arr, C.c_int), _P(sli, C.c_int) if sli is not None else None, C.byref(prm), leaf, C.byref(occ),
                               int(max_records), cap, key, l, xyz, _P(n_out, C.c_int64), _P(n_rays, C.c_int64), _P(n_drop, C.c_int64),
                               C.byref(batches)), what)
        rows = occupancy_rows(call, n, cap, n_out, self.ctx.device, host=host, centres=centres)
        return rows + (n_out[:n].copy(), n_rays[:n].copy(), n_drop[:n].copy(), int(batches.value))

    def keyframe_log_stereo_cloud(self, streams, d_min=0, n_disp=64, agg_r=2, uniq=10, lr_tol=1, depth_factor=1000.0, **cloud):
        """flvis_keyframe_log_stereo_cloud (rectified stereo rigs, cam_type 0): keyframe_log_depth_cloud on the Z16 images dense stereo
        (Context.dense_stereo: d_min .. lr_tol, or a DenseStereoParams as d_min) makes of the logged pairs, bf from each stream's own
        config, depth_factor the Z16 unit.  **cloud: keyframe_log_depth_cloud's arguments.  -> what that call returns."""
        return self.keyframe_log_depth_cloud(streams, _stereo=(dense_stereo_params(d_min, n_disp, agg_r, uniq, lr_tol), depth_factor), **cloud)

    def keyframe_log_stereo_z16(self, entries, d_min=0, n_disp=64, agg_r=2, uniq=10, lr_tol=1, depth_factor=1000.0, _unrect=False):
        """flvis_keyframe_log_stereo_z16: the Z16 depth image dense stereo makes of the logged pairs entries = [(stream, index), ..]
        -> a device tensor int16 [n, h, w] that holds the UNSIGNED 16-bit values (0: invalid); queued on the context's stream."""
        import torch
        ent = np.ascontiguousarray(list(entries) + [(0, 0)], np.int32).reshape(-1, 2)
        n = len(ent) - 1
        st, ix = np.ascontiguousarray(ent[:, 0]), np.ascontiguousarray(ent[:, 1])
        prm = dense_stereo_params(d_min, n_disp, agg_r, uniq, lr_tol)
        z = torch.empty((max(n, 1), int(self.cfg.image_height), int(self.cfg.image_width)), dtype=torch.int16, device=self.ctx.device)
        fn, what = ((self.lib.flvis_keyframe_log_unrect_stereo_z16, "keyframe_log_unrect_stereo_z16") if _unrect else
                    (self.lib.flvis_keyframe_log_stereo_z16, "keyframe_log_stereo_z16"))
        self.ctx._check(fn(self.ctx._h, n, _P(st, C.c_int), _P(ix, C.c_int), C.byref(prm), float(depth_factor), _ptr(z)), what)
        return z[:n]

    def keyframe_log_unrect_stereo_cloud(self, streams, d_min=0, n_disp=64, agg_r=2, uniq=10, lr_tol=1, depth_factor=1000.0, **cloud):
        """flvis_keyframe_log_unrect_stereo_cloud (the unrectified stereo rig, cam_type 1: EuRoC): keyframe_log_stereo_cloud on the pairs
        keyframe_log_rectified_pair makes of the logged ones.  The same arguments -> what that call returns."""
        return self.keyframe_log_depth_cloud(streams, _stereo=(dense_stereo_params(d_min, n_disp, agg_r, uniq, lr_tol), depth_factor, True),
                                             **cloud)

    def keyframe_log_unrect_stereo_z16(self, entries, **stereo):
        """flvis_keyframe_log_unrect_stereo_z16 (cam_type 1): keyframe_log_stereo_z16 on the rectified pairs of the logged entries."""
        return self.keyframe_log_stereo_z16(entries, _unrect=True, **stereo)

    def keyframe_log_rectified_pair(self, entries, want0=True, want1=True):
        """flvis_keyframe_log_rectified_pair (cam_type 1): the rectified pair of the logged entries = [(stream, index), ..], each under
        the two cameras of its stream's own config (Context.rectify has the definition) -> (img0, img1) device tensors uint8 [n, h, w],
        None for one not asked for; queued on the context's stream."""
        import torch
        ent = np.ascontiguousarray(list(entries) + [(0, 0)], np.int32).reshape(-1, 2)
        n = len(ent) - 1
        st, ix = np.ascontiguousarray(ent[:, 0]), np.ascontiguousarray(ent[:, 1])
        shape = (max(n, 1), int(self.cfg.image_height), int(self.cfg.image_width))
        out = [torch.empty(shape, dtype=torch.uint8, device=self.ctx.device) if want else None for want in (want0, want1)]
        self.ctx._check(self.lib.flvis_keyframe_log_rectified_pair(self.ctx._h, n, _P(st, C.c_int), _P(ix, C.c_int), _ptr(out[0]), _ptr(out[1])),
                        "keyframe_log_rectified_pair")
        return tuple(None if o is None else o[:n] for o in out)

    def keyframe_log_get(self, stream, index, cap=2048, images=True):
        """flvis_keyframe_log_get: logged keyframe `index` of the stream, a dict like keyframe_msg's."""
        fn = self.lib.flvis_keyframe_log_get
        return self._keyframe_msg(lambda cap_, *a: fn(self.ctx._h, int(stream), int(index), cap_, *a), "keyframe_log_get", cap, images)

    def keyframe_log_images(self, stream, index):
        """flvis_keyframe_log_images: the entry's two images as torch views of the log's device memory ([h, w] uint8; img1 int16 storage
        on a depth rig).  Valid until the stream is cleared or reset, the log is enabled again or the tracker goes away."""
        import torch
        p0, p1 = C.c_void_p(0), C.c_void_p(0)
        self.ctx._check(self.lib.flvis_keyframe_log_images(self.ctx._h, int(stream), int(index), C.byref(p0), C.byref(p1)), "keyframe_log_images")
        h, w = int(self.cfg.image_height), int(self.cfg.image_width)
        depth = self.cfg.cam_type == 2

        def view(ptr, dtype, typestr):
            class _Mem:  # (the CUDA array interface: a view, no copy; the log owns the memory)
                __cuda_array_interface__ = dict(shape=(h, w), typestr=typestr, data=(int(ptr), False), version=2)
            return torch.as_tensor(_Mem(), device=self.ctx.device)
        return view(p0.value, torch.uint8, "|u1"), view(p1.value, torch.int16, "<i2") if depth else view(p1.value, torch.uint8, "|u1")

    def dropped_keyframes(self):
        """keyframes that met a full keyframe queue (flvis_get_counters_n [3]; 0 under the tracker's back-pressure)"""
        c = (C.c_int64 * 4)()
        self.ctx._check(self.lib.flvis_get_counters_n(self.ctx._h, 4, c), "get_counters_n")
        return int(c[3])
