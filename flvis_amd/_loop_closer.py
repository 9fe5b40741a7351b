"""LoopCloser: flvis_loop_closer, its candidate rule and the links between sequences' maps."""
import ctypes as C

import numpy as np

from ._loader import FLVIS_OK, FlvisError, _P, _ptr, load_library
from ._structs import (FLVIS_LC_FIX_CAND, LC_ROW_WIDTH, LC_TRAJ_ANCHOR, FlvisCfg, FlvisImage, FlvisLcFix, FlvisLcFixIn, FlvisLcLink,
                       FlvisLcLinkQuery, FlvisLcMerge, FlvisLcTrajJob, LcEvent, LcParams, cloud_rows, dense_stereo_params, depth_cloud_params,
                       occupancy_params, occupancy_rows)


def loop_candidate(row, present, lcKFDist, lcKFMaxDist, lcNKFClosest, minScore):
    """flvis_loop_candidate (host control logic of isLoopCandidate): returns the earlier keyframe's index or None."""
    lib = load_library()
    row = np.ascontiguousarray(row, np.float64)
    pres = np.ascontiguousarray(present, np.uint8)
    out = C.c_int64(-1)
    r = lib.flvis_loop_candidate(len(row), _P(row, C.c_double), _P(pres, C.c_uint8), lcKFDist, lcKFMaxDist, lcNKFClosest, minScore,
                                 C.byref(out))
    if r < 0:
        raise FlvisError("flvis_loop_candidate failed: %d" % r)
    return int(out.value) if r == 1 else None


def links_from_fix(fix, stream, kf):
    """The links a localize_in result yields when its query frame is also stored as keyframe `kf` of sequence `stream`: one per accepted
    candidate, from (candidate's sequence, candidate's keyframe) to (stream, kf) with the candidate's PnP pose.  -> list of dicts
    (seq_from, kf_from, seq_to, kf_to, pose) for LoopCloser.merge.  (C callers have flvis_lc_links_from_fix.)"""
    return [dict(seq_from=int(c["seq"]), kf_from=int(c["kf"]), seq_to=int(stream), kf_to=int(kf), pose=[float(x) for x in c["pose"]])
            for c in fix["candidates"] if c["accepted"]]


def _link_dict(l):
    return dict(seq_from=int(l.seq_from), kf_from=int(l.kf_from), seq_to=int(l.seq_to), kf_to=int(l.kf_to), pose=[float(x) for x in l.pose7])


def _link_struct(l):
    return l if isinstance(l, FlvisLcLink) else FlvisLcLink(int(l["seq_from"]), int(l["seq_to"]), int(l["kf_from"]), int(l["kf_to"]),
                                                             (C.c_double * 7)(*[float(x) for x in l["pose"]]))


def links_reverse(links):
    """flvis_lc_link_reverse on each link (dicts as links_from_fix makes them, or FlvisLcLink): the ends swapped and the pose inverted --
    what LoopCloser.merge needs for links whose `from` sequence comes after their `to` sequence in the group.  -> list of dicts.  Host-only."""
    lib = load_library()
    out = []
    for l in links:
        a, b = _link_struct(l), FlvisLcLink()
        rc = lib.flvis_lc_link_reverse(C.byref(a), C.byref(b))
        if rc != FLVIS_OK:
            raise FlvisError("flvis_lc_link_reverse failed (%d): a pose that is not finite, or a zero quaternion" % rc)
        out.append(_link_dict(b))
    return out


class LoopCloser:
    """flvis_loop_closer: LoopClosingNodeletClass (vo_loopclosing.cpp) for n_streams sequences; the keyframe database stays on the GPU.

    cfg: one config for every sequence, or a sequence of configs -- one camera per sequence (flvis_loop_closer_create_rigs: cam_type and
    the image size must agree, FlvisError otherwise; n_streams is then their number).  self.cfg is sequence 0's."""

    def __init__(self, ctx, cfg, prm, n_streams=1, max_keyframes=2000, orb_pattern=None):
        cfgs = None
        if not isinstance(cfg, FlvisCfg):
            cfgs = list(cfg)
            if n_streams not in (1, len(cfgs)):
                raise ValueError("LoopCloser: %d configs for %d streams" % (len(cfgs), n_streams))
            n_streams, cfg = len(cfgs), cfgs[0]
        self._ctx, self._lib, self.n_streams = ctx, ctx._lib, n_streams
        self.cfg, self.max_keyframes = cfg, int(max_keyframes)
        if isinstance(prm, dict):
            prm = LcParams(**prm)
        pat = None
        if orb_pattern is not None:
            pat = np.ascontiguousarray(orb_pattern, np.int8)
            assert pat.size == 1024
        h = C.c_void_p(0)
        patp = C.c_void_p(pat.ctypes.data if pat is not None else 0)
        if cfgs is None:
            ctx._check(self._lib.flvis_loop_closer_create(ctx._h, C.byref(cfg), C.byref(prm), int(n_streams), int(max_keyframes), patp,
                                                          C.byref(h)), "loop_closer_create")
        else:
            arr = (FlvisCfg * n_streams)(*cfgs)
            ctx._check(self._lib.flvis_loop_closer_create_rigs(ctx._h, arr, C.byref(prm), int(n_streams), int(max_keyframes), patp,
                                                               C.byref(h)), "loop_closer_create_rigs")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.flvis_loop_closer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, streams, cfgs=None):
        """flvis_loop_closer_reset: the named sequences start over as sequences of a new closer (the others go on undisturbed).  cfgs: one
        config per named sequence, whose camera it changes to (flvis_loop_closer_reset_rigs).  FlvisError, and nothing changes, for an
        index out of range or listed twice or a config whose cam_type / image size is not the closer's."""
        ids = [int(k) for k in streams]
        arr = (C.c_int * max(1, len(ids)))(*ids)
        if cfgs is None:
            self._ctx._check(self._lib.flvis_loop_closer_reset(self._h, len(ids), arr), "loop_closer_reset")
            return
        cfgs = [cfgs] if isinstance(cfgs, FlvisCfg) else list(cfgs)
        if len(cfgs) != len(ids):
            raise ValueError("LoopCloser.reset: %d configs for %d streams" % (len(cfgs), len(ids)))
        carr = (FlvisCfg * max(1, len(ids)))(*cfgs)
        self._ctx._check(self._lib.flvis_loop_closer_reset_rigs(self._h, len(ids), arr, carr), "loop_closer_reset_rigs")

    def stream_cfg(self, s):
        """flvis_loop_closer_stream_cfg: the config sequence s runs on (as created, or as last reset with reset(..., cfgs))."""
        out = FlvisCfg()
        self._ctx._check(self._lib.flvis_loop_closer_stream_cfg(self._h, int(s), C.byref(out)), "loop_closer_stream_cfg")
        return out

    def set_stereo_unrect(self, enable):
        """flvis_loop_closer_set_stereo_unrect: on a STEREO_UNRECT closer (cam_type 1, the EuRoC camera) keyframes and queries get their
        landmarks by this project's rule (Context.lc_keyframe_landmarks_unrect) instead of the reference's empty case.  Pixels and poses
        are then of the rectified camera 0.  FlvisError on another cam_type, and while any sequence holds a keyframe."""
        self._ctx._check(self._lib.flvis_loop_closer_set_stereo_unrect(self._h, 1 if enable else 0), "loop_closer_set_stereo_unrect")

    def _device_images(self, img0, img1, n):
        """the device images of an add_keyframes / localize call, contiguous and of the configured size"""
        img0 = img0.contiguous()
        img1 = img1.contiguous() if img1 is not None else None
        hw = (int(self.cfg.image_height), int(self.cfg.image_width))
        assert img0.shape[0] == n and tuple(img0.shape[1:]) == hw, "img0 must be [n, image_height, image_width]"
        if img1 is not None:                                 # a wrong-size tensor would be read out of bounds on the device
            assert img1.shape[0] == n and tuple(img1.shape[1:]) == hw, "img1 must be [n, image_height, image_width]"
            assert img1.element_size() == (2 if self.cfg.cam_type == 2 else 1), "img1: uint8 (stereo) or 16-bit depth (depth rig)"
        return img0, img1

    @staticmethod
    def _host_images(img0, img1, n):
        """the numpy images of a _host call as two FlvisImage arrays (and the arrays they point into, to be kept until the call returns)"""
        a = (FlvisImage * max(1, n))()
        b = (FlvisImage * max(1, n))()
        keep = []
        for i in range(n):
            for arr, dst in ((img0[i], a), (img1[i], b)):
                assert arr.ndim == 2 and arr.strides[1] == arr.itemsize
                keep.append(arr)
                dst[i] = FlvisImage(C.cast(C.c_void_p(arr.ctypes.data), C.POINTER(C.c_uint8)), arr.shape[1], arr.shape[0], arr.strides[0], 1, 0.0)
        return a, b, keep

    def add_keyframes(self, streams, img0, img1, T_c_w_odom):
        """streams: the sequence of each keyframe (distinct); img0 uint8 [n,h,w], img1 uint8 / Z16 [n,h,w] (device); T_c_w_odom [n,7].
        Returns the keyframes' indices in their sequences."""
        st = np.ascontiguousarray(streams, np.int32)
        n = len(st)
        T = np.ascontiguousarray(T_c_w_odom, np.float64).reshape(n, 7)
        img0, img1 = self._device_images(img0, img1, n)
        ids = np.zeros(n, np.int64)
        self._ctx._check(self._lib.flvis_loop_closer_add_keyframes(self._h, n, _P(st, C.c_int), _ptr(img0), _ptr(img1), _P(T, C.c_double),
                                                                   _P(ids, C.c_int64)), "loop_closer_add_keyframes")
        return ids

    def add_keyframes_host(self, streams, img0, img1, T_c_w_odom):
        """flvis_loop_closer_add_keyframes_host: numpy images [n,h,w(+padding)]; img0 uint8, img1 uint8 or uint16 (depth rig).  A
        2-D-strided view (rows padded) is passed with its pitch."""
        st = np.ascontiguousarray(streams, np.int32)
        n = len(st)
        T = np.ascontiguousarray(T_c_w_odom, np.float64).reshape(n, 7)
        ids = np.zeros(n, np.int64)
        a, b, keep = self._host_images(img0, img1, n)
        self._ctx._check(self._lib.flvis_loop_closer_add_keyframes_host(self._h, n, _P(st, C.c_int), a, b, _P(T, C.c_double), _P(ids, C.c_int64)),
                         "loop_closer_add_keyframes_host")
        return ids

    @staticmethod
    def _events(ev):
        return [dict(kf_prev=int(e.kf_prev), kf_curr=int(e.kf_curr), candidate=bool(e.candidate), n_matches=e.n_matches,
                     n_inliers=e.n_inliers, accepted=bool(e.loop_accepted), optimised=bool(e.optimised), pgo_iterations=e.pgo_iterations,
                     pose=[float(x) for x in e.loop_pose7], chi2_before=e.chi2_before, chi2_after=e.chi2_after) for e in ev]

    def process(self):
        """-> list of n_streams dicts (flvis_lc_event)"""
        ev = (LcEvent * self.n_streams)()
        self._ctx._check(self._lib.flvis_loop_closer_process(self._h, ev), "loop_closer_process")
        return self._events(ev)

    def add_logged(self, process=True, max_rounds=None):
        """flvis_loop_closer_add_logged: every keyframe in the keyframe log of the tracker on this closer's context
        (Tracker.keyframe_log_enable) goes into the closer on the device, in rounds (round r: entry r of every stream that has one).
        -> the events per round, a list of `rounds` lists as process() returns them (empty lists with process=False).
        max_rounds: rows of the event array (default: the closer's max_keyframes, which no accepted call exceeds)."""
        cap = int(max_rounds) if max_rounds is not None else self.max_keyframes
        S = self.n_streams
        ev = (LcEvent * (cap * S))() if process else None
        n = C.c_int(0)
        self._ctx._check(self._lib.flvis_loop_closer_add_logged(self._h, bool(process), ev, cap, C.byref(n)), "loop_closer_add_logged")
        if not process:
            return [[] for _ in range(n.value)]
        return [self._events(ev[r * S:(r + 1) * S]) for r in range(n.value)]

    @staticmethod
    def _fixes(fix):
        out = []
        for f in fix:
            cands = [dict(kf=int(f.cand_kf[r]), score=float(f.cand_score[r]), n_matches=f.cand_matches[r], n_inliers=f.cand_inliers[r],
                          accepted=bool(f.cand_accepted[r]), pose=np.array(f.cand_pose7[r][:])) for r in range(f.n_candidates)]
            out.append(dict(n_landmarks=f.n_landmarks, candidates=cands, best=f.best, kf=cands[f.best]["kf"] if f.best >= 0 else -1,
                            T_c_map=np.array(f.T_c_map7[:]) if f.best >= 0 else None))
        return out

    @classmethod
    def _fixes_in(cls, fix):
        out = cls._fixes([f.fix for f in fix])
        for d, f in zip(out, fix):
            for r, c in enumerate(d["candidates"]):
                c["seq"] = int(f.cand_seq[r])
            d["map"] = int(f.map)
        return out

    def _localize(self, fn, streams, maps, img0, img1, n_best, host):
        """the four localize calls through their entry point fn: maps None: localize (FlvisLcFix), otherwise localize_in (FlvisLcFixIn);
        host: numpy images"""
        st = np.ascontiguousarray(streams, np.int32)
        n = len(st)
        args = [_P(st, C.c_int)]
        if maps is not None:
            mp = np.ascontiguousarray(maps, np.int32)
            assert len(mp) == n, "one map per query"
            args.append(_P(mp, C.c_int))
        if host:
            a, b, keep = self._host_images(img0, img1, n)
            args += [a, b]
        else:
            img0, img1 = self._device_images(img0, img1, n)
            args += [_ptr(img0), _ptr(img1)]
        Fix = FlvisLcFix if maps is None else FlvisLcFixIn
        fix = (Fix * max(1, n))()
        self._ctx._check(fn(self._h, n, *args, int(n_best), fix), fn.__name__[len("flvis_"):])
        return self._fixes(fix[:n]) if maps is None else self._fixes_in(fix[:n])

    def localize(self, streams, img0, img1, n_best=4):
        """flvis_loop_closer_localize: one query frame for each of the sequences `streams` (distinct), images as add_keyframes takes them;
        nothing is stored.  -> one dict per query: n_landmarks, candidates (the up to n_best best-scoring keyframes of the sequence, each a
        dict kf / score / n_matches / n_inliers / accepted / pose), best (index into candidates, -1: not localised), kf (its keyframe) and
        T_c_map (the query camera's pose7 in the map frame, None when not localised)."""
        return self._localize(self._lib.flvis_loop_closer_localize, streams, None, img0, img1, n_best, host=False)

    def localize_host(self, streams, img0, img1, n_best=4):
        """flvis_loop_closer_localize_host: localize on numpy images as add_keyframes_host takes them (rows may be padded)."""
        return self._localize(self._lib.flvis_loop_closer_localize_host, streams, None, img0, img1, n_best, host=True)

    def localize_in(self, streams, maps, img0, img1, n_best=4):
        """flvis_loop_closer_localize_in: localize with the searched database named per query -- maps[i] is the sequence whose keyframe map
        query i (taken by the camera of sequence streams[i]) is looked for in, FLVIS_LC_ALL_MAPS (-1) every sequence's.  -> localize's
        dicts, each candidate with seq (kf is an index within that sequence), plus map (the sequence whose map frame T_c_map is in, -1
        when not localised)."""
        return self._localize(self._lib.flvis_loop_closer_localize_in, streams, maps, img0, img1, n_best, host=False)

    def localize_in_host(self, streams, maps, img0, img1, n_best=4):
        """flvis_loop_closer_localize_in_host: localize_in on numpy images as add_keyframes_host takes them (rows may be padded)."""
        return self._localize(self._lib.flvis_loop_closer_localize_in_host, streams, maps, img0, img1, n_best, host=True)

    def link(self, queries, n_best=4):
        """flvis_loop_closer_link: localize_in with STORED keyframes as the queries.  queries: FlvisLcLinkQuery, dicts or tuples
        (stream, map, kf, own_gap) -- keyframe kf of sequence stream (-1: its newest) is looked for in the map of sequence `map`
        (FLVIS_LC_ALL_MAPS: every map), without what own_gap names of its own sequence (-1 all of it, g >= 0 the keyframes within g of
        kf).  Any number of queries, a sequence any number of times.  -> (localize_in's dicts, one per query; the links of the accepted
        candidates in OTHER sequences as LoopCloser.merge takes them)."""
        qs = []
        for q in queries:
            if isinstance(q, dict):
                q = (q["stream"], q["map"], q.get("kf", -1), q.get("own_gap", -1))
            qs.append(q if isinstance(q, FlvisLcLinkQuery) else FlvisLcLinkQuery(*[int(v) for v in q]))
        n = len(qs)
        arr = (FlvisLcLinkQuery * max(1, n))(*qs)
        fix = (FlvisLcFixIn * max(1, n))()
        cap = max(1, n) * FLVIS_LC_FIX_CAND                  # (no call yields more)
        links = (FlvisLcLink * cap)()
        cnt = C.c_int(0)
        self._ctx._check(self._lib.flvis_loop_closer_link(self._h, n, arr, int(n_best), fix, cap, links, C.byref(cnt)), "loop_closer_link")
        return self._fixes_in(fix[:n]), [_link_dict(l) for l in links[:cnt.value]]

    def set_drift(self, stream, T_odom_map):
        """flvis_loop_closer_set_drift: the sequence's T_odom_map from now on (keyframes added afterwards get T_c_w_odom * T_odom_map).
        After a tracker slot was reset: set_drift(s, mul(inv(T_c_odom), localize(...)["T_c_map"])) ties its new odometry frame to the map."""
        T = np.ascontiguousarray(T_odom_map, np.float64).reshape(7)
        self._ctx._check(self._lib.flvis_loop_closer_set_drift(self._h, int(stream), _P(T, C.c_double)), "loop_closer_set_drift")

    def merge(self, groups, links, iterations=100):
        """flvis_loop_closer_merge: the maps of each group's sequences become one map in the frame of the group's first sequence, by one
        joint pose graph per group in which `links` (dicts seq_from / kf_from / seq_to / kf_to / pose, as links_from_fix makes them, or
        FlvisLcLink) tie keyframes of different sequences.  groups: lists of at least two sequences, disjoint.  -> (one dict per group:
        optimised / n_vertices / n_edges / iterations / chi2_before / chi2_after, drift [sequences in the groups' order, 7]: what each
        sequence's T_odom_map was multiplied by).  FlvisError, and nothing changes, for arguments the call refuses."""
        groups = [[int(s) for s in g] for g in groups]
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), np.int32)
        seqs = np.ascontiguousarray([s for g in groups for s in g], np.int32)
        arr = (FlvisLcLink * max(1, len(links)))()
        for k, l in enumerate(links):
            arr[k] = _link_struct(l)
        out = (FlvisLcMerge * max(1, len(groups)))()
        drift = np.zeros((max(1, len(seqs)), 7))
        self._ctx._check(self._lib.flvis_loop_closer_merge(self._h, len(groups), _P(ptr, C.c_int), _P(seqs, C.c_int), len(links), arr,
                                                           int(iterations), out, _P(drift, C.c_double)), "loop_closer_merge")
        return ([dict(optimised=bool(o.optimised), n_vertices=o.n_vertices, n_edges=o.n_edges, iterations=o.iterations,
                      chi2_before=o.chi2_before, chi2_after=o.chi2_after) for o in out[:len(groups)]], drift[:len(seqs)].copy())

    def map_cloud(self, groups, leaf=0.08, min_points=1, cap=None, host=False):
        """flvis_loop_closer_map_cloud: the landmarks of every stored keyframe of each group's sequences, in the map frame (the T_c_w the
        database holds now), one point per voxel of `leaf` metres that holds min_points points or more; leaf = 0: every landmark.  groups:
        lists of sequences as merge takes them (a single sequence is a group too).  cap: rows per group (default: what the largest
        group yields, found by a call of its own).  host=True goes through the _host entry.  -> (xyz [n_groups] of float32 [k, 3], npts [n_groups] of int32
        [k], n_out int64 [n_groups] the full counts, n_dropped int64 [n_groups])."""
        import torch
        groups = [[int(s) for s in g] for g in groups]
        ng = len(groups)
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), np.int32)
        seqs = np.ascontiguousarray([s for g in groups for s in g] + [0], np.int32)
        if cap is None:                                      # a first call for the counts alone: the buffers then fit what comes
            cap = int(max(list(self.map_cloud(groups, leaf, min_points, cap=0, host=host)[2]) + [0]))
        cap = int(cap)
        n_out, n_drop = np.zeros(max(ng, 1), np.int64), np.zeros(max(ng, 1), np.int64)
        shape = (max(ng, 1), max(cap, 0))
        head = (self._h, ng, _P(ptr, C.c_int), _P(seqs, C.c_int), leaf, int(min_points), cap)
        if host:
            hx, hn = np.zeros(shape + (3,), np.float32), np.zeros(shape, np.int32)
            rc = self._lib.flvis_loop_closer_map_cloud_host(*head, _P(hx, C.c_float), _P(hn, C.c_int), _P(n_out, C.c_int64),
                                                            _P(n_drop, C.c_int64))
            self._ctx._check(rc, "loop_closer_map_cloud_host")
        else:
            xyz = torch.empty(shape + (3,), dtype=torch.float32, device=self._ctx.device)
            npts = torch.empty(shape, dtype=torch.int32, device=self._ctx.device)
            rc = self._lib.flvis_loop_closer_map_cloud(*head, _ptr(xyz), _ptr(npts), _P(n_out, C.c_int64), _P(n_drop, C.c_int64))
            self._ctx._check(rc, "loop_closer_map_cloud")
            kmax = int(min(max(n_out[:ng].max() if ng else 0, 0), cap))
            hx, hn = xyz[:, :kmax].cpu().numpy(), npts[:, :kmax].cpu().numpy()
        k = [int(min(n, cap)) for n in n_out[:ng]]
        return ([hx[g, :k[g]].copy() for g in range(ng)], [hn[g, :k[g]].copy() for g in range(ng)], n_out[:ng].copy(), n_drop[:ng].copy())

    def dense_cloud(self, groups, first_kf=None, window=None, step=1, z_min=0.3, z_max=10.0, leaf=0.08, min_points=1, cap=None, host=False,
                    _stereo=None):
        """flvis_loop_closer_dense_cloud (depth rigs): per group one dense cloud of the tracker's logged depth keyframes of the group's
        sequences, logged entry i under the closer's stored T_c_w of keyframe first_kf + i -- the map frame after process, set_drift
        or merge.  groups: as map_cloud's; first_kf: per group a list with one first keyframe per sequence (None: 0 everywhere).
        window / step / z_min / z_max: Context.depth_cloud's.  cap: rows per group (default: found by a call of its own).
        -> (xyz [n_groups] of float32 [k, 3], npts [n_groups] of int32 [k], n_out, n_dropped, n_valid int64 [n_groups])."""
        import torch
        groups = [[int(s) for s in g] for g in groups]
        ng = len(groups)
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), np.int32)
        seqs = np.ascontiguousarray([s for g in groups for s in g] + [0], np.int32)
        first = None if first_kf is None else np.ascontiguousarray([int(k) for g in first_kf for k in g] + [0], np.int32)
        assert first is None or len(first) == len(seqs), "one first keyframe per listed sequence"
        prm = depth_cloud_params(window, step, z_min, z_max)
        n_out, n_drop, n_valid = (np.zeros(max(ng, 1), np.int64) for _ in range(3))
        kind = "dense" if not _stereo else "unrect_stereo" if len(_stereo) > 2 and _stereo[2] else "stereo"
        what = "loop_closer_%s_cloud%s" % (kind, "_host" if host else "")
        fn = getattr(self._lib, "flvis_" + what)
        front = (C.byref(_stereo[0]), float(_stereo[1])) if _stereo else ()   # (the stereo forms: the matcher's parameters, depth_factor)
        head = (self._h, ng, _P(ptr, C.c_int), _P(seqs, C.c_int), _P(first, C.c_int) if first is not None else None) + front + (
            C.byref(prm), leaf, int(min_points))
        tail = (_P(n_out, C.c_int64), _P(n_drop, C.c_int64), _P(n_valid, C.c_int64))
        if cap is None:                                      # a first call for the counts alone: the buffers then fit what comes
            self._ctx._check(fn(*head, 0, None, None, *tail), what)
            cap = int(max(list(n_out[:ng]) + [0]))
        cap = int(cap)
        shape = (max(ng, 1), max(cap, 0))
        if host:
            hx, hn = np.zeros(shape + (3,), np.float32), np.zeros(shape, np.int32)
            self._ctx._check(fn(*head, cap, _P(hx, C.c_float), _P(hn, C.c_int), *tail), what)
        else:
            xyz = torch.empty(shape + (3,), dtype=torch.float32, device=self._ctx.device)
            npts = torch.empty(shape, dtype=torch.int32, device=self._ctx.device)
            self._ctx._check(fn(*head, cap, _ptr(xyz), _ptr(npts), *tail), what)
            hx, hn = xyz.cpu().numpy(), npts.cpu().numpy()
        rows = cloud_rows(hx, hn, n_out, cap, ng)
        return rows + (n_out[:ng].copy(), n_drop[:ng].copy(), n_valid[:ng].copy())

    def occupancy(self, groups, first_kf=None, window=None, step=1, z_min=0.3, z_max=10.0, leaf=0.08, occ=None, max_records=0, cap=None,
                  host=False, centres=True):
        """flvis_loop_closer_occupancy (depth rigs): per group one occupancy map whose scans are dense_cloud's listed keyframes -- the
        tracker's logged depth images under the closer's stored poses -- walked in batches of at most max_records records (0: 2^26).
        occ: an OccupancyParams (None: octomap's defaults).  cap: rows per group (default: found by a call of its own).
        -> (keys [n_groups] of int64 [k], logodds of float32 [k], centres of float32 [k, 3] or None, n_out, n_rays, n_dropped int64
        [n_groups], the batches run)."""
        groups = [[int(s) for s in g] for g in groups]
        ng = len(groups)
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), np.int32)
        seqs = np.ascontiguousarray([s for g in groups for s in g] + [0], np.int32)
        first = None if first_kf is None else np.ascontiguousarray([int(k) for g in first_kf for k in g] + [0], np.int32)
        assert first is None or len(first) == len(seqs), "one first keyframe per listed sequence"
        prm, occ = depth_cloud_params(window, step, z_min, z_max), occupancy_params(occ)
        n_out, n_rays, n_drop = (np.zeros(max(ng, 1), np.int64) for _ in range(3))
        batches = C.c_int(0)
        what = "loop_closer_occupancy" + ("_host" if host else "")
        fn = getattr(self._lib, "flvis_" + what)

        def call(cap, key, l, xyz):
            self._ctx._check(fn(self._h, ng, _P(ptr, C.c_int), _P(seqs, C.c_int), _P(first, C.c_int) if first is not None else None,
                                C.byref(prm), leaf, C.byref(occ), int(max_records), cap, key, l, xyz, _P(n_out, C.c_int64),
                                _P(n_rays, C.c_int64), _P(n_drop, C.c_int64), C.byref(batches)), what)
        rows = occupancy_rows(call, ng, cap, n_out, self._ctx.device, host=host, centres=centres)
        return rows + (n_out[:ng].copy(), n_rays[:ng].copy(), n_drop[:ng].copy(), int(batches.value))

    def stereo_cloud(self, groups, d_min=0, n_disp=64, agg_r=2, uniq=10, lr_tol=1, depth_factor=1000.0, **cloud):
        """flvis_loop_closer_stereo_cloud (rectified stereo rigs, cam_type 0): dense_cloud on the Z16 images dense stereo
        (Context.dense_stereo: d_min .. lr_tol, or a DenseStereoParams as d_min) makes of the tracker's logged pairs, bf from each sequence's
        own config, depth_factor the Z16 unit.  **cloud: dense_cloud's arguments.  -> what that call returns."""
        return self.dense_cloud(groups, _stereo=(dense_stereo_params(d_min, n_disp, agg_r, uniq, lr_tol), depth_factor), **cloud)

    def unrect_stereo_cloud(self, groups, d_min=0, n_disp=64, agg_r=2, uniq=10, lr_tol=1, depth_factor=1000.0, **cloud):
        """flvis_loop_closer_unrect_stereo_cloud (the unrectified stereo rig, cam_type 1: EuRoC): stereo_cloud on the logged pairs
        rectified under each sequence's own config (Tracker.keyframe_log_rectified_pair), stored poses, whether or not set_stereo_unrect
        is on.  The same arguments -> what that call returns."""
        return self.dense_cloud(groups, _stereo=(dense_stereo_params(d_min, n_disp, agg_r, uniq, lr_tol), depth_factor, True), **cloud)

    def poses(self, stream=0, cap=None):
        cap = int(cap) if cap else self.max_keyframes      # (never fewer rows than the sequence can hold: no silent truncation)
        n = C.c_int(0)
        buf = np.zeros((cap, 7))
        self._ctx._check(self._lib.flvis_loop_closer_poses(self._h, int(stream), _P(buf, C.c_double), cap, C.byref(n)), "loop_closer_poses")
        if n.value > cap:
            raise FlvisError("loop_closer_poses: %d keyframes, buffer of %d" % (n.value, cap))
        return buf[:n.value].copy()

    def keyframe(self, stream, kf, cap=1024):
        """flvis_loop_closer_keyframe -> dict(lm2 [k,2] f32, lm3 [k,3] f64, lmd [k,32] u8, bow=(ids, vals))"""
        lm2, lm3, lmd = np.zeros((cap, 2), np.float32), np.zeros((cap, 3)), np.zeros((cap, 32), np.uint8)
        bi, bv = np.zeros(cap, np.int32), np.zeros(cap)
        nl, nv = C.c_int(0), C.c_int(0)
        self._ctx._check(self._lib.flvis_loop_closer_keyframe(self._h, int(stream), int(kf), cap, _P(lm2, C.c_float), _P(lm3, C.c_double),
                                                              _P(lmd, C.c_uint8), C.byref(nl), _P(bi, C.c_int), _P(bv, C.c_double), C.byref(nv)),
                         "loop_closer_keyframe")
        k, v = min(nl.value, cap), min(nv.value, cap)
        return dict(lm2=lm2[:k].copy(), lm3=lm3[:k].copy(), lmd=lmd[:k].copy(), bow=(bi[:v].copy(), bv[:v].copy()))

    def drift(self, stream=0):
        T = np.zeros(7)
        self._ctx._check(self._lib.flvis_loop_closer_drift(self._h, int(stream), _P(T, C.c_double)), "loop_closer_drift")
        return T

    def similarity_row(self, stream=0, cap=None):
        cap = int(cap) if cap else self.max_keyframes
        n = C.c_int(0)
        buf = np.zeros(cap)
        self._ctx._check(self._lib.flvis_loop_closer_similarity_row(self._h, int(stream), _P(buf, C.c_double), cap, C.byref(n)),
                         "loop_closer_similarity_row")
        if n.value > cap:
            raise FlvisError("loop_closer_similarity_row: %d entries, buffer of %d" % (n.value, cap))
        return buf[:n.value].copy()

    def set_keyframe_stamps(self, stream, first_kf, stamps):
        """flvis_loop_closer_set_keyframe_stamps: the stamps of keyframes first_kf .. of the sequence (add_keyframes leaves them unset,
        add_logged takes them from the log).  FlvisError, and nothing changes, where the sequence's stamps would not stay finite and
        strictly increasing."""
        t = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        fn = self._lib.flvis_loop_closer_set_keyframe_stamps
        self._ctx._check(fn(self._h, int(stream), int(first_kf), len(t), _P(t, C.c_double)), "loop_closer_set_keyframe_stamps")

    def keyframe_stamps(self, stream=0):
        """flvis_loop_closer_keyframe_stamps -> float64 [keyframes of the sequence], NaN where never set"""
        n = C.c_int(0)
        buf = np.zeros(self.max_keyframes)
        fn = self._lib.flvis_loop_closer_keyframe_stamps
        self._ctx._check(fn(self._h, int(stream), _P(buf, C.c_double), self.max_keyframes, C.byref(n)), "loop_closer_keyframe_stamps")
        return buf[:n.value].copy()

    def map_poses(self, jobs, mode=LC_TRAJ_ANCHOR, host=False):
        """flvis_loop_closer_map_poses[_host]: pose rows of the closer's sequences into the map frame, every row with the drift of the
        keyframe it follows (LC_TRAJ_ANCHOR) or the chord between that keyframe's drift and the next one's (LC_TRAJ_BLEND).  jobs: (seq,
        kind, rows) with rows [n, 8 | 9 | 11] of kind LC_ROWS_POSE8 / _TRAJ9 (Tracker.trajectory) / _IMU11 (Tracker.imu_states): device
        float64 tensors, or with host=True numpy arrays.  -> per job (rows in the map frame, anchors int32 [n]: the keyframe, -1 in an
        empty sequence, -2 for a NaN stamp), of the inputs' type.  FlvisError, and nothing is written, when a named sequence holds a
        keyframe without a stamp."""
        import torch
        arr = (FlvisLcTrajJob * max(1, len(jobs)))()
        res = []
        for k, (seq, kind, rows) in enumerate(jobs):
            kind = int(kind)
            if host:
                rows = np.ascontiguousarray(rows, np.float64).reshape(-1, LC_ROW_WIDTH[kind])
                out, anc = np.zeros_like(rows), np.zeros(len(rows), np.int32)
                arr[k] = FlvisLcTrajJob(int(seq), kind, len(rows), rows.ctypes.data, out.ctypes.data, anc.ctypes.data)
            else:
                assert rows.dtype == torch.float64 and rows.is_cuda and rows.is_contiguous() and rows.dim() == 2
                assert rows.shape[1] == LC_ROW_WIDTH[kind], "rows do not have the width of their kind"
                out, anc = torch.empty_like(rows), torch.empty((rows.shape[0],), dtype=torch.int32, device=rows.device)
                arr[k] = FlvisLcTrajJob(int(seq), kind, int(rows.shape[0]), rows.data_ptr(), out.data_ptr(), anc.data_ptr())
            res.append((rows, out, anc))
        fn = self._lib.flvis_loop_closer_map_poses_host if host else self._lib.flvis_loop_closer_map_poses
        self._ctx._check(fn(self._h, len(jobs), arr, int(mode)), "loop_closer_map_poses_host" if host else "loop_closer_map_poses")
        return [(out, anc) for _, out, anc in res]

    def map_trajectory(self, streams, first, n_frames, mode=LC_TRAJ_ANCHOR, device=False):
        """flvis_loop_closer_map_trajectory: rows first .. first + n_frames - 1 of the trajectory record of the tracker on this closer's
        context, streams `streams` (stream s <-> sequence s), in the map frame; no pose goes through the host on the way.
        -> (rows float64 [n, n_frames, 9], anchors int32 [n, n_frames]) as numpy arrays; device=True: the rows as a device tensor."""
        import torch
        st = np.ascontiguousarray(streams, np.int32)
        n, m = len(st), int(n_frames)
        anc = np.zeros((n, max(m, 0)), np.int32)
        fn = self._lib.flvis_loop_closer_map_trajectory
        if device:
            rows = torch.empty((n, max(m, 0), 9), dtype=torch.float64, device=self._ctx.device)
            rc = fn(self._h, n, _P(st, C.c_int), int(first), m, int(mode), _ptr(rows), None, anc.ctypes.data)
        else:
            rows = np.zeros((n, max(m, 0), 9))
            rc = fn(self._h, n, _P(st, C.c_int), int(first), m, int(mode), None, rows.ctypes.data, anc.ctypes.data)
        self._ctx._check(rc, "loop_closer_map_trajectory")
        return rows, anc
