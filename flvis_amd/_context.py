"""Context: a flvis_ctx on one GPU and the kernel-level entry points (torch CUDA tensors in and out)."""
import ctypes as C
import os

import numpy as np

from ._loader import FLVIS_OK, FlvisError, _P, _ptr, load_library
from ._structs import (LC_ROW_WIDTH, FlvisCfg, FlvisLcTrajJob, OrbParams, VocTrainParams, dense_stereo_params, depth_cloud_params,
                       occupancy_cast_params, occupancy_params, occupancy_rows)
from ._vocfile import TrainedVocabulary


class Context:
    """Owns a flvis_ctx bound to one GPU and one HIP stream: torch's current stream by default, the default stream with
    use_torch_stream=False, or a private non-blocking stream with own_stream=True (several contexts then run concurrently;
    inputs produced on torch's stream must be synchronised by the caller)."""

    def __init__(self, device=0, use_torch_stream=True, own_stream=False):
        import torch
        self._lib = load_library()
        if not torch.cuda.is_available():
            raise FlvisError("flvis_amd needs a HIP device (MI355X); none is visible. No CPU fallback exists.")
        torch.cuda.set_device(device)
        self.device = torch.device("cuda", device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if use_torch_stream else C.c_void_p(0)
        if own_stream:
            stream = C.c_void_p(-1 & (2 ** 64 - 1))  # FLVIS_STREAM_NEW
        h = C.c_void_p(0)
        rc = self._lib.flvis_hip_create(device, stream, C.byref(h))
        if rc != FLVIS_OK:
            raise FlvisError("flvis_hip_create failed: %d" % rc)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.flvis_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != FLVIS_OK:
            raise FlvisError("%s failed (%d): %s" % (what, rc, self._lib.flvis_last_error(self._h).decode()))

    def synchronize(self):
        self._check(self._lib.flvis_hip_synchronize(self._h), "synchronize")

    # ---- kernel-level entry points (torch CUDA tensors in/out) -------------------------------------------------
    def equalize_hist(self, img):
        """img: uint8 [n,h,w] cuda tensor -> equalised copy."""
        import torch
        assert img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous() and img.dim() == 3
        n, h, w = img.shape
        out = torch.empty_like(img)
        self._check(self._lib.flvis_hip_equalize_hist(self._h, _ptr(img), _ptr(out), w, h, n), "equalize_hist")
        return out

    def cvt_bgr_to_gray(self, img):
        """img uint8 [n,h,w,3|4] (BGR / BGRA, interleaved) -> gray [n,h,w]."""
        import torch
        assert img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous() and img.dim() == 4
        n, h, w, c = img.shape
        out = torch.empty((n, h, w), dtype=torch.uint8, device=img.device)
        self._check(self._lib.flvis_hip_cvt_bgr_to_gray(self._h, _ptr(img), c, _ptr(out), w, h, n), "cvt_bgr_to_gray")
        return out

    def pyr_down(self, img):
        import torch
        assert img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous() and img.dim() == 3
        n, h, w = img.shape
        dw, dh = (w + 1) // 2, (h + 1) // 2
        out = torch.empty((n, dh, dw), dtype=torch.uint8, device=img.device)
        self._check(self._lib.flvis_hip_pyr_down(self._h, _ptr(img), w, h, w, _ptr(out), dw, n), "pyr_down")
        return out

    def debug_pyramid(self, img, levels, bx=32, by=24, ingest=True):
        """Test aid (flvis_debug_pyramid): the tracker's pyramid construction.  img uint8 [n,h,w] on the GPU; returns the list of the
        levels 0 .. levels as uint8 [n, h_l + 2 by, w_l + 2 bx] (border included; level 0 is None when ingest is False)."""
        import torch
        assert img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous() and img.dim() == 3
        n, h, w = img.shape
        geo, off = [], 0
        lw, lh = w, h
        for _ in range(levels + 1):
            pitch = ((lw + 15) & ~15) + 2 * bx
            rows = lh + 2 * by
            geo.append((off, pitch, rows, lw, lh))
            off += (pitch * rows * n + 63) & ~63
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
        out = torch.zeros(off + 64, dtype=torch.uint8, device=img.device)
        pad = (-out.data_ptr()) % 64
        buf = out[pad:pad + off]
        self._check(self._lib.flvis_debug_pyramid(self._h, _ptr(img), w, h, n, levels, bx, by, 1 if ingest else 0, _ptr(buf), off), "debug_pyramid")
        res = []
        for l, (o, pitch, rows, lw, lh) in enumerate(geo):
            if l == 0 and not ingest:
                res.append(None)
                continue
            res.append(buf[o:o + pitch * rows * n].view(n, rows, pitch)[:, :, :lw + 2 * bx].clone())
        return res

    def lk_track(self, prev, nxt, prev_pts, next_pts, count, max_level=10, max_iter=30, eps=1e-3, use_initial=True):
        """prev/nxt uint8 [n,h,w]; prev_pts/next_pts float32 [n,nmax,2]; count int32 [n].
        Returns (next_pts_out, status uint8 [n,nmax])."""
        import torch
        prev, nxt = prev.contiguous(), nxt.contiguous()
        n, h, w = prev.shape
        nmax = prev_pts.shape[1]
        assert prev_pts.dtype == torch.float32 and next_pts.dtype == torch.float32 and count.dtype == torch.int32
        out = next_pts.clone().contiguous()
        status = torch.zeros((n, nmax), dtype=torch.uint8, device=prev.device)
        self._check(self._lib.flvis_hip_lk_track(self._h, _ptr(prev), _ptr(nxt), w, h, n, _ptr(prev_pts.contiguous()),
                                                 _ptr(out), _ptr(status), _ptr(count), nmax, max_level, max_iter,
                                                 eps, use_initial), "lk_track")
        return out, status

    def rand_seed(self, seed, n_sets):
        """flvis_hip_rand_seed: the glibc rand() state of n_sets sets after srand(seed) (int32 [n_sets, 35] on the device)."""
        import torch
        st = torch.zeros((n_sets, 35), dtype=torch.int32, device=self.device)
        self._check(self._lib.flvis_hip_rand_seed(self._h, seed, _ptr(st), n_sets), "rand_seed")
        return st

    def stereo_depth(self, cfg, img0, img1, pt2d_plane, pt2d_undistort, pt3d_w, has_depth, count, poses7, rng, rand_state, out=None, mask=None):
        """flvis_hip_stereo_depth = CameraFrame::recover3DPts_c_FromStereo (camera_frame.cpp:93-180) for n_sets frames in one call.
        img0 / img1 uint8 [n,h,w]; pt2d_* float32 [n,cap,2]; pt3d_w float32 [n,cap,3]; has_depth uint8 [n,cap]; count int32 [n] (all on
        the device); poses7 host [n,7]; rand_state from rand_seed() (updated in place).  Returns (pt3ds float64 [n,cap,3], mask uint8):
        out / mask when the caller passes its own (the call writes the first min(count, cap) slots of a set and no other), else new
        zero-filled tensors."""
        import torch
        n, cap = pt2d_plane.shape[0], pt2d_plane.shape[1]
        for a, dt in ((pt2d_plane, torch.float32), (pt2d_undistort, torch.float32), (pt3d_w, torch.float32), (has_depth, torch.uint8),
                      (count, torch.int32), (img0, torch.uint8), (img1, torch.uint8), (rand_state, torch.int32)):
            assert a.is_cuda and a.is_contiguous() and a.dtype == dt
        T = np.ascontiguousarray(poses7, np.float64).reshape(n, 7)
        if out is None:
            out = torch.zeros((n, cap, 3), dtype=torch.float64, device=self.device)
        if mask is None:
            mask = torch.zeros((n, cap), dtype=torch.uint8, device=self.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (n, cap, 3)
        assert mask.is_cuda and mask.is_contiguous() and mask.dtype == torch.uint8 and tuple(mask.shape) == (n, cap)
        self._check(self._lib.flvis_hip_stereo_depth(self._h, C.byref(cfg), _ptr(img0), _ptr(img1), n, _ptr(pt2d_plane),
                                                     _ptr(pt2d_undistort), _ptr(pt3d_w), _ptr(has_depth), _ptr(count), cap,
                                                     T.ctypes.data, rng, _ptr(rand_state), _ptr(out), _ptr(mask)),
                    "stereo_depth")
        return out, mask

    def lkorb_tracking(self, cfg, img_from, img_to, from_2d_plane, from_2d_undistort, from_3d_w, from_flags, count, guess7=None,
                       use_guess=None, pose7=None, out=None):
        """flvis_hip_lkorb_tracking = LKORBTracking::tracking (lkorb_tracking.cpp:9-202) for n_sets frames in one call, on any cam_type.
        img_from / img_to uint8 [n,h,w]; from_2d_* float32 [n,cap,2]; from_3d_w float32 [n,cap,3]; from_flags uint8 [n,cap] (bit 0 has_3d,
        bit 1 is_tracking_inlier); count int32 [n] (all on the device); guess7 host [n,7] (tx ty tz qx qy qz qw) and use_guess host [n],
        or None: no set has a guess.  pose7: float64 [n,7] on the device, in / out (None: a new tensor of identities); only the sets that
        reach the PnP write theirs.  out: a dict of the caller's own output tensors (any of to_from int32 [n,cap], to_2d_plane /
        to_2d_undistort float32 [n,cap,2], to_flags uint8 [n,cap], mask_F uint8 [n,cap], counts4 int32 [n,4], ret uint8 [n]); the call
        writes the rows below each set's of_inlier_cnt and no other; what is missing is created zero-filled.
        Returns the dict of the outputs, with "pose7"."""
        import torch
        n, cap = from_2d_plane.shape[0], from_2d_plane.shape[1]
        for a, dt in ((img_from, torch.uint8), (img_to, torch.uint8), (from_2d_plane, torch.float32), (from_2d_undistort, torch.float32),
                      (from_3d_w, torch.float32), (from_flags, torch.uint8), (count, torch.int32)):
            assert a.is_cuda and a.is_contiguous() and a.dtype == dt
        assert tuple(img_from.shape) == tuple(img_to.shape) == (n, cfg.image_height, cfg.image_width)
        g = None if guess7 is None else np.ascontiguousarray(guess7, np.float64).reshape(n, 7)
        u = None if use_guess is None else np.ascontiguousarray(use_guess, np.uint8).reshape(n)
        if pose7 is None:
            pose7 = torch.zeros((n, 7), dtype=torch.float64, device=self.device)
            pose7[:, 6] = 1.0
        o = dict(out or {})
        spec = (("to_from", torch.int32, (n, cap)), ("to_2d_plane", torch.float32, (n, cap, 2)), ("to_2d_undistort", torch.float32, (n, cap, 2)),
                ("to_flags", torch.uint8, (n, cap)), ("mask_F", torch.uint8, (n, cap)), ("counts4", torch.int32, (n, 4)), ("ret", torch.uint8, (n,)))
        for name, dt, shape in spec:
            if o.get(name) is None:
                o[name] = torch.zeros(shape, dtype=dt, device=self.device)
            t = o[name]
            assert t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shape, name
        assert pose7.is_cuda and pose7.is_contiguous() and pose7.dtype == torch.float64 and tuple(pose7.shape) == (n, 7)
        o["pose7"] = pose7
        f = self._lib.flvis_hip_lkorb_tracking
        self._check(f(self._h, C.byref(cfg), _ptr(img_from), _ptr(img_to), n, _ptr(from_2d_plane), _ptr(from_2d_undistort), _ptr(from_3d_w),
                      _ptr(from_flags), _ptr(count), cap, None if g is None else g.ctypes.data, None if u is None else u.ctypes.data,
                      _ptr(o["to_from"]), _ptr(o["to_2d_plane"]), _ptr(o["to_2d_undistort"]), _ptr(o["to_flags"]), _ptr(o["mask_F"]),
                      _ptr(o["counts4"]), _ptr(pose7), _ptr(o["ret"])), "lkorb_tracking")
        return o

    def gftt(self, img, max_corners, quality, min_distance):
        import torch
        img = img.contiguous()
        n, h, w = img.shape
        out = torch.zeros((n, max_corners, 2), dtype=torch.float32, device=img.device)
        cnt = torch.zeros((n,), dtype=torch.int32, device=img.device)
        self._check(self._lib.flvis_hip_gftt(self._h, _ptr(img), w, h, n, max_corners, quality, min_distance, _ptr(out),
                                             _ptr(cnt)), "gftt")
        return out, cnt

    def debug_corner_response(self, img, variant, rows=0, key_cap=1 << 17):
        """test aid: (max ordered bits [n], sorted candidate keys per image) of the corner-response pass with the chosen kernel"""
        img = img.contiguous()
        n, h, w = img.shape
        mx = np.zeros(n, np.uint32)
        nk = np.zeros(n, np.int32)
        keys = np.zeros((n, key_cap), np.uint64)
        self._check(self._lib.flvis_hip_debug_corner_response(self._h, _ptr(img), w, h, n, int(variant), int(rows), _P(mx, C.c_uint32),
                                                              _P(nk, C.c_int), _P(keys, C.c_uint64), key_cap), "corner_response")
        return mx, [np.sort(keys[i, :nk[i]]) for i in range(n)]

    def debug_sqrt_check(self, first_bits, n):
        """test aid: arguments in [first_bits, first_bits + n) (float bit patterns) on which the corner-response kernel's square
        root differs from the correctly rounded sqrtf"""
        bad = C.c_uint64(0)
        self._check(self._lib.flvis_hip_debug_sqrt_check(self._h, first_bits, n, C.byref(bad)), "sqrt_check")
        return bad.value

    def feature_dem_detect(self, img, f_para, out_cap=1024):
        import torch
        img = img.contiguous()
        n, h, w = img.shape
        fp = (C.c_double * 6)(*[float(x) for x in f_para])
        out = torch.zeros((n, out_cap, 2), dtype=torch.float32, device=img.device)
        cnt = torch.zeros((n,), dtype=torch.int32, device=img.device)
        self._check(self._lib.flvis_hip_feature_dem_detect(self._h, _ptr(img), w, h, n, fp, _ptr(out), _ptr(cnt),
                                                           out_cap), "feature_dem_detect")
        return out, cnt

    def feature_dem_redetect(self, img, f_para, exist_xy, exist_count, out_cap=1024):
        import torch
        img = img.contiguous()
        n, h, w = img.shape
        fp = (C.c_double * 6)(*[float(x) for x in f_para])
        assert exist_xy.dtype == torch.float64 and exist_count.dtype == torch.int32
        out = torch.zeros((n, out_cap, 2), dtype=torch.float32, device=img.device)
        cnt = torch.zeros((n,), dtype=torch.int32, device=img.device)
        self._check(self._lib.flvis_hip_feature_dem_redetect(self._h, _ptr(img), w, h, n, fp, _ptr(exist_xy.contiguous()),
                                                             _ptr(exist_count), exist_xy.shape[1], _ptr(out), _ptr(cnt),
                                                             out_cap), "feature_dem_redetect")
        return out, cnt


# ---------------------------------------------------------------------------------------------------- pipeline level

    # ---- ORB extraction + Hamming matching ---------------------------------------------------------
    def resize_linear(self, img, dw, dh):
        import torch
        img = img.contiguous()
        n, h, w = img.shape
        out = torch.empty((n, dh, dw), dtype=torch.uint8, device=img.device)
        self._check(self._lib.flvis_hip_resize_linear(self._h, _ptr(img), w, h, _ptr(out), int(dw), int(dh), n), "resize_linear")
        return out

    def fast_score(self, img, threshold):
        import torch
        img = img.contiguous()
        n, h, w = img.shape
        out = torch.empty_like(img)
        self._check(self._lib.flvis_hip_fast_score(self._h, _ptr(img), w, h, n, int(threshold), _ptr(out)), "fast_score")
        return out

    def gaussian_blur7(self, img):
        import torch
        img = img.contiguous()
        n, h, w = img.shape
        out = torch.empty_like(img)
        self._check(self._lib.flvis_hip_gaussian_blur7(self._h, _ptr(img), _ptr(out), w, h, n), "gaussian_blur7")
        return out

    def orb_detect_and_compute(self, img, nfeatures=1000, scale_factor=1.2, nlevels=8, fast_threshold=20, pattern=None,
                               cap=2048):
        """img uint8 [n,h,w] -> (kps float32 [n,cap,6] (x, y, size, angle, response, octave), desc uint8 [n,cap,32],
        count int32 [n], overflow int32 [n])."""
        import torch
        img = img.contiguous()
        n, h, w = img.shape
        kps = torch.zeros((n, cap, 6), dtype=torch.float32, device=img.device)
        desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device=img.device)
        cnt = torch.zeros((n,), dtype=torch.int32, device=img.device)
        ovf = torch.zeros((n,), dtype=torch.int32, device=img.device)
        prm = OrbParams(int(nfeatures), float(scale_factor), int(nlevels), int(fast_threshold))
        pat = None
        if pattern is not None:
            pat = np.ascontiguousarray(pattern, np.int8)
            assert pat.size == 1024
        self._check(self._lib.flvis_hip_orb_detect_and_compute(
            self._h, _ptr(img), w, h, n, C.byref(prm), C.c_void_p(pat.ctypes.data if pat is not None else 0), _ptr(kps),
            _ptr(desc), _ptr(cnt), cap, _ptr(ovf)), "orb_detect_and_compute")
        return kps, desc, cnt, ovf

    def hamming_knn2(self, query, nq, train, nt):
        """query uint8 [p,qcap,32], nq int32 [p], train uint8 [p,tcap,32], nt int32 [p] -> (idx, dist) int32 [p,qcap,2]."""
        import torch
        query, train = query.contiguous(), train.contiguous()
        p, qcap, _ = query.shape
        tcap = train.shape[1]
        idx = torch.full((p, qcap, 2), -7, dtype=torch.int32, device=query.device)
        dist = torch.full((p, qcap, 2), -7, dtype=torch.int32, device=query.device)
        self._check(self._lib.flvis_hip_hamming_knn2(self._h, _ptr(query), _ptr(nq), qcap, _ptr(train), _ptr(nt), tcap, p,
                                                     _ptr(idx), _ptr(dist)), "hamming_knn2")
        return idx, dist

    def orb_match(self, a, na, b, nb, ratio_max):
        """mutual-best + ratio test -> (pairs int32 [p,acap,2], npairs int32 [p])."""
        import torch
        a, b = a.contiguous(), b.contiguous()
        p, acap, _ = a.shape
        bcap = b.shape[1]
        pairs = torch.full((p, acap, 2), -1, dtype=torch.int32, device=a.device)
        npairs = torch.zeros((p,), dtype=torch.int32, device=a.device)
        self._check(self._lib.flvis_hip_orb_match(self._h, _ptr(a), _ptr(na), acap, _ptr(b), _ptr(nb), bcap, p,
                                                  ratio_max, _ptr(pairs), _ptr(npairs)), "orb_match")
        return pairs, npairs


    def bow_set_vocabulary(self, child_ptr, child_idx, desc, weight, word_id):
        """flvis_hip_bow_set_vocabulary: the DBoW3 tree as flat arrays (see include/flvis_hip.h)."""
        cp = np.ascontiguousarray(child_ptr, np.int32)
        ci = np.ascontiguousarray(child_idx, np.int32)
        ds = np.ascontiguousarray(desc, np.uint8)
        wt = np.ascontiguousarray(weight, np.float64)
        wi = np.ascontiguousarray(word_id, np.int32)
        n = len(cp) - 1
        assert ds.shape == (n, 32) and len(wt) == n and len(wi) == n
        self._check(self._lib.flvis_hip_bow_set_vocabulary(self._h, n, _P(cp, C.c_int), _P(ci, C.c_int), _P(ds, C.c_uint8),
                                                           _P(wt, C.c_double), _P(wi, C.c_int)), "bow_set_vocabulary")

    def voc_train(self, desc, count, k=10, L=5, seed=1, weighting=0, max_iters=0, small_node_max=0):
        """flvis_hip_voc_train: DBoW3's Vocabulary::create on the device.  desc uint8 [n,cap,32], count int32 [n] (device tensors, as
        orb_detect_and_compute returns them) -> TrainedVocabulary."""
        import torch
        desc = desc.contiguous()
        assert desc.dtype == torch.uint8 and desc.is_cuda and desc.dim() == 3 and desc.shape[2] == 32
        assert count.dtype == torch.int32 and count.is_cuda and count.is_contiguous() and count.numel() == desc.shape[0]
        prm = VocTrainParams(int(k), int(L), int(weighting), int(seed) & 0xFFFFFFFF, int(max_iters), int(small_node_max))
        h = C.c_void_p(0)
        stats = (C.c_int64 * 8)()
        self._check(self._lib.flvis_hip_voc_train(self._h, _ptr(desc), _ptr(count), desc.shape[1], desc.shape[0], C.byref(prm), C.byref(h),
                                                  stats), "voc_train")
        return TrainedVocabulary(self._lib, h, list(stats))

    def bow_load_vocabulary(self, path):
        """flvis_hip_bow_load_vocabulary: `Vocabulary voc(path)` of vo_loopclosing.cpp:1097 (.dbow3 / .txt / .yml / .yml.gz)."""
        self._check(self._lib.flvis_hip_bow_load_vocabulary(self._h, os.fsencode(path)), "bow_load_vocabulary")

    def bow_transform(self, desc, count, vcap=2048):
        """desc uint8 [n,dcap,32], count int32 [n] (device) -> (ids int32 [n,vcap], vals float64 [n,vcap], nnz int32 [n])."""
        import torch
        desc = desc.contiguous()
        n, dcap, _ = desc.shape
        ids = torch.full((n, vcap), -1, dtype=torch.int32, device=desc.device)
        vals = torch.zeros((n, vcap), dtype=torch.float64, device=desc.device)
        nnz = torch.zeros((n,), dtype=torch.int32, device=desc.device)
        self._check(self._lib.flvis_hip_bow_transform(self._h, _ptr(desc), _ptr(count), dcap, n, vcap, _ptr(ids), _ptr(vals),
                                                      _ptr(nnz)), "bow_transform")
        return ids, vals, nnz

    def bow_score(self, q_ids, q_vals, q_nnz, db_ids, db_vals, db_nnz):
        """one similarity-matrix row: query (1-D device tensors + nnz [1]) against db [m,vcap] -> scores float64 [m]."""
        import torch
        m, vcap = db_ids.shape
        scores = torch.full((m,), -1.0, dtype=torch.float64, device=db_ids.device)
        self._check(self._lib.flvis_hip_bow_score(self._h, _ptr(q_ids), _ptr(q_vals), _ptr(q_nnz), _ptr(db_ids), _ptr(db_vals),
                                                  _ptr(db_nnz), vcap, m, _ptr(scores)), "bow_score")
        return scores

    def bow_score_jobs(self, jobs, ids, vals, nnz):
        """flvis_hip_bow_score_jobs: jobs [(query vector, first database vector, n database vectors)] over one store ids / vals
        [n_vectors, vcap], nnz [n_vectors] (device) -> scores float64 [n_vectors] (entries outside the jobs' ranges stay -1)."""
        import torch
        j = np.ascontiguousarray(jobs, np.int32).reshape(-1, 3)
        nv, vcap = ids.shape
        scores = torch.full((nv,), -1.0, dtype=torch.float64, device=ids.device)
        self._check(self._lib.flvis_hip_bow_score_jobs(self._h, len(j), _P(j, C.c_int), _ptr(ids), _ptr(vals), _ptr(nnz), vcap, _ptr(scores)),
                    "bow_score_jobs")
        return scores

    def bow_score_jobs_at(self, jobs, ids, vals, nnz, n_out):
        """flvis_hip_bow_score_jobs_at: jobs [(query vector, first database vector, n database vectors, first output index)] over one store
        ids / vals [n_vectors, vcap], nnz [n_vectors] (device) -> scores float64 [n_out] (entries no job writes stay -1)."""
        import torch
        j = np.ascontiguousarray(jobs, np.int32).reshape(-1, 4)
        assert all(0 <= o and o + n <= n_out for _, _, n, o in j), "a job writes outside the output"
        assert all(0 <= q < ids.shape[0] and 0 <= f and f + n <= ids.shape[0] for q, f, n, _ in j), "a job reads outside the store"
        vcap = ids.shape[1]
        scores = torch.full((int(n_out),), -1.0, dtype=torch.float64, device=ids.device)
        self._check(self._lib.flvis_hip_bow_score_jobs_at(self._h, len(j), _P(j, C.c_int), _ptr(ids), _ptr(vals), _ptr(nnz), vcap,
                                                          _ptr(scores)), "bow_score_jobs_at")
        return scores

    def voxel_cloud(self, p3, count, T_c_w, clouds, leaf=0.08, min_points=1, cap=None, want_npts=True):
        """flvis_hip_voxel_cloud: p3 float64 [n_rows, pcap, 3] (camera frame), count int32 [n_rows], T_c_w float64 [n_rows, 7], device
        tensors; clouds: per cloud a list of (first row, row count) ranges.  cap: output rows per cloud (default: every input slot of the
        largest cloud, so nothing is cut).  -> (xyz [n_clouds] of float32 [k, 3], npts [n_clouds] of int32 [k] or None, n_out int64
        [n_clouds] the full counts, n_dropped int64 [n_clouds]) as numpy arrays; k = min(n_out, cap)."""
        import torch
        assert p3.dtype == torch.float64 and p3.is_cuda and p3.is_contiguous() and p3.dim() == 3 and p3.shape[2] == 3
        assert count.dtype == torch.int32 and count.is_contiguous() and T_c_w.dtype == torch.float64 and T_c_w.is_contiguous()
        n_rows, pcap = int(p3.shape[0]), int(p3.shape[1])
        assert count.numel() == n_rows and tuple(T_c_w.shape) == (n_rows, 7)
        clouds = [[(int(a), int(b)) for a, b in c] for c in clouds]
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), np.int32)
        rng = np.ascontiguousarray([r for c in clouds for r in c], np.int32).reshape(-1, 2)
        if cap is None:
            cap = max([sum(max(b, 0) for _, b in c) for c in clouds] + [0]) * pcap
        cap, nc = int(cap), len(clouds)
        xyz = torch.empty((max(nc, 1), max(cap, 0), 3), dtype=torch.float32, device=p3.device)
        npts = torch.empty((max(nc, 1), max(cap, 0)), dtype=torch.int32, device=p3.device) if want_npts else None
        n_out, n_drop = np.zeros(max(nc, 1), np.int64), np.zeros(max(nc, 1), np.int64)
        self._check(self._lib.flvis_hip_voxel_cloud(self._h, _ptr(p3), _ptr(count), _ptr(T_c_w), n_rows, pcap, nc, _P(ptr, C.c_int),
                                                    _P(rng, C.c_int), leaf, int(min_points), cap, _ptr(xyz), _ptr(npts), _P(n_out, C.c_int64),
                                                    _P(n_drop, C.c_int64)), "voxel_cloud")
        k = [int(min(n, cap)) for n in n_out[:nc]]
        hx = xyz.cpu().numpy()
        hn = npts.cpu().numpy() if want_npts else None
        return ([hx[c, :k[c]].copy() for c in range(nc)], [hn[c, :k[c]].copy() for c in range(nc)] if want_npts else None,
                n_out[:nc].copy(), n_drop[:nc].copy())

    def depth_cloud(self, depth, T_c_w, clouds, cams, window=None, step=1, z_min=0.3, z_max=10.0, leaf=0.08, min_points=1, cap=None,
                    want_npts=True):
        """flvis_hip_depth_cloud: depth uint16 [n_img, h, w] (a device tensor; torch without uint16: int16 of the same bits), T_c_w
        float64 [n_img, 7]; clouds: per cloud a list of (first image, image count) ranges; cams: one (fx, fy, cx, cy, depth_factor)
        per range, in the ranges' order.  window (u0, v0, u1, v1) or a DepthCloudParams, step an int or (step_u, step_v), z_min / z_max
        in metres.  cap: output rows per cloud (default: found by a call of its own).  -> (xyz [n_clouds] of float32 [k, 3], npts
        [n_clouds] of int32 [k] or None, n_out, n_dropped, n_valid int64 [n_clouds]) as numpy arrays; k = min(n_out, cap)."""
        import torch
        assert depth.is_cuda and depth.is_contiguous() and depth.dim() == 3 and depth.element_size() == 2 and not depth.dtype.is_floating_point
        assert T_c_w.dtype == torch.float64 and T_c_w.is_contiguous() and tuple(T_c_w.shape) == (int(depth.shape[0]), 7)
        n_img, h, w = [int(x) for x in depth.shape]
        clouds = [[(int(a), int(b)) for a, b in c] for c in clouds]
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), np.int32)
        rng = np.ascontiguousarray([r for c in clouds for r in c] + [(0, 0)], np.int32).reshape(-1, 2)
        cam5 = np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 5))
        assert len(cam5) == len(rng) - 1, "one camera per range"
        prm = depth_cloud_params(window, step, z_min, z_max)
        nc = len(clouds)
        n_out, n_drop, n_valid = (np.zeros(max(nc, 1), np.int64) for _ in range(3))

        def call(cap, xyz, npts):
            self._check(self._lib.flvis_hip_depth_cloud(self._h, _ptr(depth), _ptr(T_c_w), n_img, w, h, nc, _P(ptr, C.c_int), _P(rng, C.c_int),
                                                        _P(cam5, C.c_double), C.byref(prm), leaf, int(min_points), cap, _ptr(xyz), _ptr(npts),
                                                        _P(n_out, C.c_int64), _P(n_drop, C.c_int64), _P(n_valid, C.c_int64)), "depth_cloud")
        if cap is None:
            call(0, None, None)
            cap = int(max(list(n_out[:nc]) + [0]))
        cap = int(cap)
        xyz = torch.empty((max(nc, 1), max(cap, 0), 3), dtype=torch.float32, device=depth.device)
        npts = torch.empty((max(nc, 1), max(cap, 0)), dtype=torch.int32, device=depth.device) if want_npts else None
        call(cap, xyz, npts)
        k = [int(min(n, cap)) for n in n_out[:nc]]
        hx = xyz.cpu().numpy()
        hn = npts.cpu().numpy() if want_npts else None
        return ([hx[c, :k[c]].copy() for c in range(nc)], [hn[c, :k[c]].copy() for c in range(nc)] if want_npts else None,
                n_out[:nc].copy(), n_drop[:nc].copy(), n_valid[:nc].copy())

    def occupancy(self, depth, T_c_w, maps, cams, window=None, step=1, z_min=0.3, z_max=10.0, leaf=0.08, occ=None, prior=None, cap=None,
                  centres=True):
        """flvis_hip_occupancy: depth, T_c_w, maps (per map a list of (first image, image count) ranges; every listed image is a scan),
        cams, window, step, z_min, z_max: depth_cloud's.  occ: an OccupancyParams (None: octomap's defaults).  prior: per map (keys int64
        [k], logodds float32 [k]) or None, e.g. an earlier call's rows.  cap: output rows per map (default: found by a call of its own).
        -> (keys [n_maps] of int64 [k], logodds [n_maps] of float32 [k], centres [n_maps] of float32 [k, 3] or None, n_out, n_rays,
        n_dropped int64 [n_maps]) as numpy arrays; k = min(n_out, cap)."""
        import torch
        assert depth.is_cuda and depth.is_contiguous() and depth.dim() == 3 and depth.element_size() == 2 and not depth.dtype.is_floating_point
        assert T_c_w.dtype == torch.float64 and T_c_w.is_contiguous() and tuple(T_c_w.shape) == (int(depth.shape[0]), 7)
        n_img, h, w = [int(x) for x in depth.shape]
        maps = [[(int(a), int(b)) for a, b in c] for c in maps]
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(c) for c in maps])]), np.int32)
        rng = np.ascontiguousarray([r for c in maps for r in c] + [(0, 0)], np.int32).reshape(-1, 2)
        cam5 = np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 5))
        assert len(cam5) == len(rng) - 1, "one camera per range"
        prm, occ = depth_cloud_params(window, step, z_min, z_max), occupancy_params(occ)
        nm = len(maps)
        n_out, n_rays, n_drop = (np.zeros(max(nm, 1), np.int64) for _ in range(3))
        pk = pl = n_prior = None
        pcap = 0
        if prior is not None:
            assert len(prior) == nm, "one prior per map"
            n_prior = np.ascontiguousarray([len(k) for k, _ in prior] + [0], np.int64)
            pcap = int(max(n_prior.max(), 1))
            hk, hl = np.zeros((max(nm, 1), pcap), np.int64), np.zeros((max(nm, 1), pcap), np.float32)
            for m, (k, l) in enumerate(prior):
                hk[m, :len(k)], hl[m, :len(k)] = np.asarray(k, np.int64), np.asarray(l, np.float32)
            pk, pl = torch.from_numpy(hk).to(depth.device), torch.from_numpy(hl).to(depth.device)

        def call(cap, key, l, xyz):
            self._check(self._lib.flvis_hip_occupancy(self._h, _ptr(depth), _ptr(T_c_w), n_img, w, h, nm, _P(ptr, C.c_int), _P(rng, C.c_int),
                                                      _P(cam5, C.c_double), C.byref(prm), leaf, C.byref(occ), _ptr(pk), _ptr(pl), pcap,
                                                      _P(n_prior, C.c_int64) if n_prior is not None else None, cap, key, l, xyz,
                                                      _P(n_out, C.c_int64), _P(n_rays, C.c_int64), _P(n_drop, C.c_int64)), "occupancy")
        rows = occupancy_rows(call, nm, cap, n_out, depth.device, centres=centres)
        return rows + (n_out[:nm].copy(), n_rays[:nm].copy(), n_drop[:nm].copy())

    def occupancy_stats(self):
        """flvis_hip_occupancy_stats -> dict(records, rays, batches, workspace_bytes, ms=(count, emit, sort, reduce)) of the context's last
        occupancy call; the milliseconds are kept while depth_cloud_times is enabled."""
        st, ms = (C.c_int64 * 4)(), (C.c_double * 4)()
        self._check(self._lib.flvis_hip_occupancy_stats(self._h, st, ms), "occupancy_stats")
        return dict(records=int(st[0]), rays=int(st[1]), batches=int(st[2]), workspace_bytes=int(st[3]), ms=tuple(float(v) for v in ms))

    def occupancy_cast(self, maps, segments, leaf, thres=0.0, ignore_unknown=False, max_cells=0, host=False, outputs=True, rows=None):
        """flvis_hip_occupancy_cast: the first obstacle or unknown cell along segments through occupancy maps.  maps: per map (keys
        int64 [k], logodds float32 [k]) as occupancy returns them and prior= takes them, numpy arrays that are uploaded -- or, for maps
        that live on the device, ONE pair of device tensors (key int64 [n_maps, cap], logodds float32 [n_maps, cap]) with rows = the
        maps' row counts.  segments: per map float64 [q, 6] (o.x o.y o.z p.x p.y p.z in the map's frame; q may be 0).  thres (or an
        OccupancyCastParams), ignore_unknown, max_cells: the header's rule.  host: the _host form (segments and outputs cross as host
        arrays).  outputs False: only status is asked for (the other arrays are NULL).
        -> (status int32, k int32, cell int64, row int32, l float32, t float64: each a list of per-map numpy arrays [q], None for one
        not asked for; counts int64 [n_maps, 5] per status END, OCCUPIED, UNKNOWN, DROPPED, LIMIT)."""
        import torch
        prm = occupancy_cast_params(thres, ignore_unknown, max_cells)
        if rows is not None:
            key, lo = maps
            assert key.is_cuda and key.dtype == torch.int64 and key.is_contiguous() and key.dim() == 2
            assert lo.is_cuda and lo.dtype == torch.float32 and lo.is_contiguous() and lo.shape == key.shape
            nm, cap = int(key.shape[0]), int(key.shape[1])
            n_rows = np.ascontiguousarray(list(rows) + [0], np.int64)
            assert len(n_rows) == nm + 1, "one row count per map"
        else:
            nm = len(maps)
            n_rows = np.ascontiguousarray([len(k) for k, _ in maps] + [0], np.int64)
            cap = int(max(n_rows.max(), 1))
            hk, hl = np.zeros((max(nm, 1), cap), np.int64), np.zeros((max(nm, 1), cap), np.float32)
            for m, (k, l) in enumerate(maps):
                hk[m, :len(k)], hl[m, :len(k)] = np.asarray(k, np.int64), np.asarray(l, np.float32)
            key, lo = torch.from_numpy(hk).to(self.device), torch.from_numpy(hl).to(self.device)
        assert len(segments) == nm, "one array of segments per map"
        segs = [np.ascontiguousarray(s, np.float64).reshape(-1, 6) for s in segments]
        qptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(s) for s in segs])]), np.int32)
        nq = int(qptr[-1])
        seg = np.ascontiguousarray(np.concatenate(segs + [np.zeros((1, 6))]))
        counts = np.zeros((max(nm, 1), 5), np.int64)
        kinds = (np.int32, np.int32, np.int64, np.int32, np.float32, np.float64)
        want = [True] + [bool(outputs)] * 5
        fn = self._lib.flvis_hip_occupancy_cast_host if host else self._lib.flvis_hip_occupancy_cast
        if host:
            out = [np.zeros(nq + 1, t) if w else None for t, w in zip(kinds, want)]
            ptrs = [o.ctypes.data_as(C.c_void_p) if o is not None else None for o in out]
            sp = seg.ctypes.data_as(C.c_void_p)
        else:
            tk = (torch.int32, torch.int32, torch.int64, torch.int32, torch.float32, torch.float64)
            dev = [torch.zeros(nq + 1, dtype=t, device=self.device) if w else None for t, w in zip(tk, want)]
            dseg = torch.from_numpy(seg).to(self.device)
            ptrs, sp = [_ptr(o) for o in dev], _ptr(dseg)
        self._check(fn(self._h, nm, _ptr(key), _ptr(lo), cap, _P(n_rows, C.c_int64), float(leaf), C.byref(prm), sp, _P(qptr, C.c_int),
                       *ptrs, _P(counts, C.c_int64)), "occupancy_cast_host" if host else "occupancy_cast")
        if not host:
            out = [o.cpu().numpy() if o is not None else None for o in dev]
        per = [[o[qptr[m]:qptr[m + 1]].copy() for m in range(nm)] if o is not None else None for o in out]
        return tuple(per) + (counts[:nm].copy(),)

    def occupancy_lookup(self, maps, points, leaf, thres=0.0, rows=None):
        """The state of the voxel of every point: occupancy_cast of the segments p -> p (zero steps, ignore_unknown 0), octomap's
        search().  points: per map float64 [q, 3].  -> (status [n_maps] of int32 [q]: 0 free, 1 occupied, 2 unknown, 3 dropped; row
        int32 [q], -1 when absent; l float32 [q], 0 when absent; counts int64 [n_maps, 5])."""
        pts = [np.asarray(p, np.float64).reshape(-1, 3) for p in points]
        r = self.occupancy_cast(maps, [np.concatenate([p, p], axis=1) for p in pts], leaf, thres=thres, rows=rows)
        return r[0], r[3], r[4], r[6]

    def occupancy_cast_lookup(self, plain=False):
        """flvis_hip_occupancy_cast_lookup: how the casts of this context find a cell's row from now on -- the line directory (default)
        or, plain=True, one binary search over all rows per cell: the baseline, with the same bits."""
        self._check(self._lib.flvis_hip_occupancy_cast_lookup(self._h, int(bool(plain))), "occupancy_cast_lookup")

    def occupancy_cast_stats(self):
        """flvis_hip_occupancy_cast_stats -> dict(queries, cells, index_bytes, workspace_bytes, ms=(index build, walk)) of the context's
        last cast; the milliseconds are kept while depth_cloud_times is enabled."""
        st, ms = (C.c_int64 * 4)(), (C.c_double * 2)()
        self._check(self._lib.flvis_hip_occupancy_cast_stats(self._h, st, ms), "occupancy_cast_stats")
        return dict(queries=int(st[0]), cells=int(st[1]), index_bytes=int(st[2]), workspace_bytes=int(st[3]), ms=tuple(float(v) for v in ms))

    def dense_stereo(self, img0, img1, bf, depth_factor=1000.0, d_min=0, n_disp=64, agg_r=2, uniq=10, lr_tol=1, want_disp=True, want_z=True):
        """flvis_hip_dense_stereo: img0, img1 uint8 [n_img, h, w] device tensors, a RECTIFIED pair per image (a point at column u of
        img0 lies at u - d of img1).  bf (focal length times baseline, pixel-metres) and depth_factor (the Z16 unit): a number each for
        every image, or one per image.  d_min (or a DenseStereoParams), n_disp, agg_r, uniq, lr_tol: the header's definition.
        -> (disp16, z16): device tensors int16 [n_img, h, w] that hold the UNSIGNED 16-bit results (torch without uint16, as
        depth_cloud reads them), None for an output not asked for."""
        import torch
        assert img0.is_cuda and img0.dtype == torch.uint8 and img0.is_contiguous() and img0.dim() == 3
        assert img1.is_cuda and img1.dtype == torch.uint8 and img1.is_contiguous() and img1.shape == img0.shape
        n_img, h, w = [int(x) for x in img0.shape]
        bf, df = np.atleast_1d(np.asarray(bf, np.float64)), np.atleast_1d(np.asarray(depth_factor, np.float64))
        n_cam = max(len(bf), len(df))
        cam2 = np.ascontiguousarray(np.stack([np.broadcast_to(bf, n_cam), np.broadcast_to(df, n_cam)], axis=1))
        prm = dense_stereo_params(d_min, n_disp, agg_r, uniq, lr_tol)
        disp = torch.empty((n_img, h, w), dtype=torch.int16, device=img0.device) if want_disp else None
        z16 = torch.empty((n_img, h, w), dtype=torch.int16, device=img0.device) if want_z else None
        self._check(self._lib.flvis_hip_dense_stereo(self._h, _ptr(img0), _ptr(img1), n_img, w, h, n_cam, _P(cam2, C.c_double), C.byref(prm),
                                                     _ptr(disp), _ptr(z16)), "dense_stereo")
        return disp, z16

    def rectify(self, src, cams, cam_of=None, want_covered=True):
        """flvis_hip_rectify: src uint8 [n_img, h, w] device tensor of raw images; cams float64 [n_cam, 21] = per camera K (fx fy cx cy),
        D (k1 k2 p1 p2), R (9, row-major), Pn (fx' fy' cx' cy' of the rectified projection): one camera for every image, one per image,
        or any number with cam_of [n_img] naming each image's.  The header has the definition (fp64 map rounded once to 1/32 px, integer
        bilinear blend, uncovered pixels 0).  -> (dst, covered) uint8 [n_img, h, w] device tensors, covered None unless asked for; queued
        on the context's stream."""
        import torch
        assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 3
        n_img, h, w = [int(x) for x in src.shape]
        cam21 = np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 21))
        of = None if cam_of is None else np.ascontiguousarray(cam_of, np.int32)
        assert of is None or len(of) == n_img, "one camera index per image"
        dst = torch.empty_like(src)
        cov = torch.empty_like(src) if want_covered else None
        self._check(self._lib.flvis_hip_rectify(self._h, _ptr(src), n_img, w, h, len(cam21), _P(cam21, C.c_double),
                                                _P(of, C.c_int) if of is not None else None, _ptr(dst), _ptr(cov)), "rectify")
        return dst, cov

    def depth_cloud_times(self, enable=True):
        """flvis_hip_depth_cloud_times: switch the stage timing of the dense calls on or off -> dict(count, keys, sort, rows) in
        milliseconds of the last timed call."""
        ms = np.zeros(4)
        self._check(self._lib.flvis_hip_depth_cloud_times(self._h, int(bool(enable)), _P(ms, C.c_double)), "depth_cloud_times")
        return dict(count=float(ms[0]), keys=float(ms[1]), sort=float(ms[2]), rows=float(ms[3]))

    def voxel_cloud_stats(self):
        """flvis_hip_voxel_cloud_stats: dict(passes_run, passes_skipped, workspace_bytes, input_points) of the context's last call"""
        st = np.zeros(4, np.int64)
        self._check(self._lib.flvis_hip_voxel_cloud_stats(self._h, _P(st, C.c_int64)), "voxel_cloud_stats")
        return dict(passes_run=int(st[0]), passes_skipped=int(st[1]), workspace_bytes=int(st[2]), input_points=int(st[3]))

    def lc_map_poses(self, T_odom, T_map, stamps, nkf, jobs, mode=0, drift=None):
        """flvis_hip_lc_map_poses: pose rows into the map frame.  T_odom, T_map float64 [n_seq, kf_stride, 7], stamps float64 [n_seq,
        kf_stride] (device tensors), nkf: keyframes per sequence, drift [n_seq, 7]: the sequences' T_odom_map (read for empty ones).
        jobs: dicts seq / kind (LC_ROWS_*) / rows (device float64 [n, 8 | 9 | 11]) and optionally out (a device tensor of the same
        shape, or "inplace"; default: a new tensor) and anchor (False: no anchor array).  mode: LC_TRAJ_ANCHOR or LC_TRAJ_BLEND.
        -> per job (rows in the map frame, anchors int32 [n] or None), device tensors."""
        import torch
        for t in (T_odom, T_map, stamps):
            assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous()
        n_seq, stride = int(stamps.shape[0]), int(stamps.shape[1])
        assert tuple(T_odom.shape) == (n_seq, stride, 7) and tuple(T_map.shape) == (n_seq, stride, 7)
        nkf = np.ascontiguousarray(nkf, np.int32)
        assert len(nkf) == n_seq
        dr = None if drift is None else np.ascontiguousarray(drift, np.float64).reshape(n_seq, 7)
        arr = (FlvisLcTrajJob * max(1, len(jobs)))()
        res = []
        for k, j in enumerate(jobs):
            rows = j["rows"]
            assert rows.dtype == torch.float64 and rows.is_cuda and rows.is_contiguous() and rows.dim() == 2
            assert rows.shape[1] == LC_ROW_WIDTH[int(j["kind"])], "rows do not have the width of their kind"
            out = j.get("out")
            out = rows if isinstance(out, str) and out == "inplace" else torch.empty_like(rows) if out is None else out
            assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and out.shape == rows.shape
            anc = torch.empty((rows.shape[0],), dtype=torch.int32, device=rows.device) if j.get("anchor", True) else None
            arr[k] = FlvisLcTrajJob(int(j["seq"]), int(j["kind"]), int(rows.shape[0]), rows.data_ptr(), out.data_ptr(),
                                    anc.data_ptr() if anc is not None else None)
            res.append((out, anc))
        self._check(self._lib.flvis_hip_lc_map_poses(self._h, n_seq, stride, _P(nkf, C.c_int), _ptr(T_odom), _ptr(T_map), _ptr(stamps),
                                                     _P(dr, C.c_double) if dr is not None else None, len(jobs), arr, int(mode)), "lc_map_poses")
        return res

    def lc_select_maps(self, scores, seg_n, maps, n_best, min_score):
        """flvis_hip_lc_select_maps: scores float64 [n_q, n_seg, seg_len], seg_n int32 [n_seg], maps int32 [n_q] (a segment, or -1: all),
        device tensors -> (idx int32 [n_q, n_best] global index seg * seg_len + j or -1, score float64 [n_q, n_best], count int32 [n_q])."""
        import torch
        scores = scores.contiguous()
        n_q, n_seg, seg_len = scores.shape
        assert scores.dtype == torch.float64 and seg_n.dtype == torch.int32 and maps.dtype == torch.int32
        assert seg_n.numel() == n_seg and maps.numel() == n_q
        idx = torch.full((n_q, int(n_best)), -2, dtype=torch.int32, device=scores.device)
        sc = torch.full((n_q, int(n_best)), -1.0, dtype=torch.float64, device=scores.device)
        cnt = torch.full((n_q,), -1, dtype=torch.int32, device=scores.device)
        self._check(self._lib.flvis_hip_lc_select_maps(self._h, n_q, _ptr(scores), n_seg, seg_len, _ptr(seg_n.contiguous()),
                                                       _ptr(maps.contiguous()), int(n_best), min_score, _ptr(idx), _ptr(sc), _ptr(cnt)),
                    "lc_select_maps")
        return idx, sc, cnt

    def lc_select_maps_skip(self, scores, seg_n, maps, skip, n_best, min_score):
        """flvis_hip_lc_select_maps_skip: lc_select_maps with skip int32 [n_q, 2] = (lo, hi) per query -- the global indices lo <= g < hi
        are never candidates and are not read.  scores [n_q, n_seg, seg_len], or [n_q, seg_len]: the compact rows that hold segment
        maps[q] alone (flvis_hip_lc_select_maps_skip_compact; seg_n then tells the number of segments, and skip may be None)."""
        import torch
        scores = scores.contiguous()
        compact = scores.dim() == 2
        n_q, n_seg, seg_len = (scores.shape[0], seg_n.numel(), scores.shape[1]) if compact else scores.shape
        assert scores.dtype == torch.float64 and seg_n.dtype == torch.int32 and maps.dtype == torch.int32
        assert seg_n.numel() == n_seg and maps.numel() == n_q
        assert skip is not None or compact
        if skip is not None:
            skip = skip.contiguous()
            assert skip.dtype == torch.int32 and tuple(skip.shape) == (n_q, 2)
        if compact:                                      # a map outside the segments would index seg_n out of bounds on the device
            assert bool(((maps >= 0) & (maps < n_seg)).all()), "compact rows: every query names its segment"
        idx = torch.full((n_q, int(n_best)), -2, dtype=torch.int32, device=scores.device)
        sc = torch.full((n_q, int(n_best)), -1.0, dtype=torch.float64, device=scores.device)
        cnt = torch.full((n_q,), -1, dtype=torch.int32, device=scores.device)
        fn = self._lib.flvis_hip_lc_select_maps_skip_compact if compact else self._lib.flvis_hip_lc_select_maps_skip
        self._check(fn(self._h, n_q, _ptr(scores), n_seg, seg_len, _ptr(seg_n.contiguous()), _ptr(maps.contiguous()), _ptr(skip), int(n_best),
                       min_score, _ptr(idx), _ptr(sc), _ptr(cnt)), "lc_select_maps_skip")
        return idx, sc, cnt

    def lc_keyframe_landmarks(self, img0, img1, cam_type, kps, desc, count, P0=None, P1=None, K4=None, in_place=False):
        """flvis_hip_lc_keyframe_landmarks (vo_loopclosing.cpp:255-372): kps float32 [n,cap,6], desc uint8 [n,cap,32], count int32 [n] as
        orb_detect_and_compute returns them; img0 uint8 [n,h,w]; img1 uint8 (stereo, cam_type 0) or int16/uint16 Z16 (depth, cam_type 2).
        P0 / P1 [12] or K4 [4]: one camera for every image; [n,12] / [n,4]: one per image (flvis_hip_lc_keyframe_landmarks_rigs).
        Returns (lm_2d float32 [n,cap,2], lm_3d float64 [n,cap,3], lm_desc uint8 [n,cap,32], lm_count int32 [n])."""
        import torch
        kps, desc = kps.contiguous(), desc.contiguous()
        n, cap, _ = kps.shape
        ref = img0 if img0 is not None else img1
        h, w = ref.shape[-2:]
        img0 = img0.contiguous() if img0 is not None else None
        img1 = img1.contiguous() if img1 is not None else None
        rigs = any(a is not None and np.ndim(a) == 2 for a in (P0, P1, K4))
        dbl = lambda a, m: None if a is None else np.ascontiguousarray(a, np.float64).reshape((n, m) if rigs else m)
        p0, p1, k4 = dbl(P0, 12), dbl(P1, 12), dbl(K4, 4)
        fn = self._lib.flvis_hip_lc_keyframe_landmarks_rigs if rigs else self._lib.flvis_hip_lc_keyframe_landmarks
        hp = lambda a: _P(a, C.c_double) if a is not None else None
        lm2 = torch.zeros((n, cap, 2), dtype=torch.float32, device=kps.device)
        lm3 = torch.zeros((n, cap, 3), dtype=torch.float64, device=kps.device)
        lmd = desc if in_place else torch.zeros_like(desc)
        cnt = torch.zeros((n,), dtype=torch.int32, device=kps.device)
        self._check(fn(
            self._h, _ptr(img0) if img0 is not None else C.c_void_p(0), _ptr(img1) if img1 is not None else C.c_void_p(0), w, h, n,
            int(cam_type), hp(p0), hp(p1), hp(k4), _ptr(kps), _ptr(desc), _ptr(count), cap, _ptr(lm2), _ptr(lm3), _ptr(lmd), _ptr(cnt)),
            "lc_keyframe_landmarks")
        return lm2, lm3, lmd, cnt

    def lc_keyframe_landmarks_unrect(self, img0, img1, cfgs, kps, desc, count, in_place=False, out=None):
        """flvis_hip_lc_keyframe_landmarks_unrect: the STEREO_UNRECT case (the reference's is empty) by this project's rule -- LK from the
        keypoints of the raw img0 into the raw img1, both ends through undistortPoints, DLT with P0 / P1.  img0 / img1 uint8 [n,h,w]; cfgs: a
        finalized FlvisCfg (one rig for every image) or a sequence of n (one per image); kps / desc / count as orb_detect_and_compute returns
        them.  Returns (lm_2d float32 [n,cap,2] in the RECTIFIED plane, lm_3d float64 [n,cap,3] in the rectified camera-0 frame, lm_desc,
        lm_count) as lc_keyframe_landmarks does; out: these four tensors from the caller (a test's sentinel-filled ones) instead of new ones."""
        import torch
        kps, desc, img0, img1 = kps.contiguous(), desc.contiguous(), img0.contiguous(), img1.contiguous()
        n, cap, _ = kps.shape
        h, w = img0.shape[-2:]
        assert tuple(img0.shape) == tuple(img1.shape) == (n, h, w) and img0.dtype == img1.dtype == torch.uint8
        cfgs = [cfgs] if isinstance(cfgs, FlvisCfg) else list(cfgs)
        arr = (FlvisCfg * max(1, len(cfgs)))(*cfgs)
        if out is not None:
            lm2, lm3, lmd, cnt = out
            assert (lm2.dtype, lm3.dtype, lmd.dtype, cnt.dtype) == (torch.float32, torch.float64, torch.uint8, torch.int32)
            assert tuple(lm2.shape) == (n, cap, 2) and tuple(lm3.shape) == (n, cap, 3) and tuple(lmd.shape) == (n, cap, 32) and cnt.numel() == n
            assert all(t.is_contiguous() for t in out)
        else:
            lm2 = torch.zeros((n, cap, 2), dtype=torch.float32, device=kps.device)
            lm3 = torch.zeros((n, cap, 3), dtype=torch.float64, device=kps.device)
            lmd = desc if in_place else torch.zeros_like(desc)
            cnt = torch.zeros((n,), dtype=torch.int32, device=kps.device)
        fn = self._lib.flvis_hip_lc_keyframe_landmarks_unrect
        self._check(fn(self._h, _ptr(img0), _ptr(img1), w, h, n, arr, len(cfgs), _ptr(kps), _ptr(desc), _ptr(count), cap, _ptr(lm2), _ptr(lm3),
                       _ptr(lmd), _ptr(cnt)), "lc_keyframe_landmarks_unrect")
        return lm2, lm3, lmd, cnt

    def pnp_ransac(self, p3d, p2d, count, K4, seeds, iterations=100, reproj_px=2.0, confidence=0.99):
        """flvis_hip_pnp_ransac: p3d float32 [n,cap,3], p2d float32 [n,cap,2], count int32 [n] (device) -> (pose7 [n,7], mask [n,cap],
        n_inliers [n]).  K4 [4]: one camera for every set; [n,4]: one per set (flvis_hip_pnp_ransac_rigs)."""
        import torch
        p3d, p2d = p3d.contiguous(), p2d.contiguous()
        n, cap, _ = p3d.shape
        K = np.ascontiguousarray(K4, np.float64)
        sd = np.ascontiguousarray(seeds, np.uint64)
        rigs = K.ndim == 2
        assert len(sd) == n and K.shape == ((n, 4) if rigs else (4,))
        fn = self._lib.flvis_hip_pnp_ransac_rigs if rigs else self._lib.flvis_hip_pnp_ransac
        pose = torch.zeros((n, 7), dtype=torch.float64, device=p3d.device)
        mask = torch.zeros((n, cap), dtype=torch.uint8, device=p3d.device)
        ninl = torch.zeros((n,), dtype=torch.int32, device=p3d.device)
        self._check(fn(self._h, _ptr(p3d), _ptr(p2d), _ptr(count), cap, n, _P(K, C.c_double), int(iterations), reproj_px,
                       confidence, _P(sd, C.c_uint64), _ptr(pose), _ptr(mask), _ptr(ninl)), "pnp_ransac")
        return pose, mask, ninl

    def debug_pnp_ransac_iterative(self, p3d, p2d, count, K4, guess7, iterations=100, reproj_px=3.0, confidence=0.99):
        """flvis_hip_debug_pnp_ransac_iterative: the tracker's branch of the PnP RANSAC (5-point EPnP hypotheses, Gauss-Newton on the inliers;
        its parameters are the defaults) on the arrays of pnp_ransac, guess7 float64 [n,7] (host) -> (pose7 [n,7], mask [n,cap],
        n_inliers [n]); a set without a model gets its guess back."""
        import torch
        p3d, p2d = p3d.contiguous(), p2d.contiguous()
        n, cap, _ = p3d.shape
        K = np.ascontiguousarray(K4, np.float64)
        g7 = np.ascontiguousarray(guess7, np.float64)
        assert K.shape == (4,) and g7.shape == (n, 7)
        pose = torch.zeros((n, 7), dtype=torch.float64, device=p3d.device)
        mask = torch.zeros((n, cap), dtype=torch.uint8, device=p3d.device)
        ninl = torch.zeros((n,), dtype=torch.int32, device=p3d.device)
        self._check(self._lib.flvis_hip_debug_pnp_ransac_iterative(
            self._h, _ptr(p3d), _ptr(p2d), _ptr(count), cap, n, _P(K, C.c_double), int(iterations), reproj_px,
            confidence, _P(g7, C.c_double), _ptr(pose), _ptr(mask), _ptr(ninl)), "debug_pnp_ransac_iterative")
        return pose, mask, ninl

    def find_fundamental_ransac(self, m1, m2, count, thr_px=5.0, confidence=0.99, mask=None, n_inliers=None):
        """flvis_hip_find_fundamental_ransac = cv::findFundamentalMat(FM_RANSAC, thr_px, confidence) (lkorb_tracking.cpp:134), the mask only:
        m1, m2 float32 [n,cap,2], count int32 [n] (device) -> (mask uint8 [n,cap], n_inliers int32 [n]).  mask / n_inliers: the caller's
        output tensors (rows from a set's count on are left as they are); default: new zeroed ones."""
        import torch
        m1, m2 = m1.contiguous(), m2.contiguous()
        n, cap, _ = m1.shape
        assert m1.dtype == torch.float32 and m2.dtype == torch.float32 and m2.shape == m1.shape and count.dtype == torch.int32
        mask = torch.zeros((n, cap), dtype=torch.uint8, device=m1.device) if mask is None else mask
        n_inliers = torch.zeros((n,), dtype=torch.int32, device=m1.device) if n_inliers is None else n_inliers
        assert mask.is_contiguous() and mask.shape == (n, cap) and mask.dtype == torch.uint8 and n_inliers.dtype == torch.int32
        self._check(self._lib.flvis_hip_find_fundamental_ransac(self._h, _ptr(m1), _ptr(m2), _ptr(count), cap, n, thr_px, confidence,
                                                                _ptr(mask), _ptr(n_inliers)),
                    "find_fundamental_ransac")
        return mask, n_inliers

    def optimize_in_frame(self, lm_3d_w, lm_2d_undistort, lm_id, count, K4, pose7, ok=None):
        """flvis_hip_optimize_in_frame = OptimizeInFrame::optimize (optimize_in_frame.cpp:10-91): lm_3d_w float64 [n,cap,3], lm_2d_undistort
        float64 [n,cap,2], lm_id int64 [n,cap], count int32 [n], pose7 float64 [n,7] (device; T_c_w, updated IN PLACE where ok) ->
        (pose7, ok uint8 [n]).  K4 [4]: one camera for every set; [n,4]: one per set."""
        import torch
        lm_3d_w, lm_2d_undistort, lm_id = lm_3d_w.contiguous(), lm_2d_undistort.contiguous(), lm_id.contiguous()
        n, cap, _ = lm_3d_w.shape
        K = np.ascontiguousarray(K4, np.float64)
        assert K.shape in ((4,), (n, 4)) and pose7.is_contiguous() and pose7.shape == (n, 7) and pose7.dtype == torch.float64
        assert lm_3d_w.dtype == torch.float64 and lm_2d_undistort.dtype == torch.float64 and lm_id.dtype == torch.int64
        assert lm_2d_undistort.shape == (n, cap, 2) and lm_id.shape == (n, cap) and count.dtype == torch.int32
        ok = torch.zeros((n,), dtype=torch.uint8, device=lm_3d_w.device) if ok is None else ok
        self._check(self._lib.flvis_hip_optimize_in_frame(self._h, _ptr(lm_3d_w), _ptr(lm_2d_undistort), _ptr(lm_id), _ptr(count), cap, n,
                                                          _P(K, C.c_double), 1 if K.ndim == 1 else n, _ptr(pose7), _ptr(ok)),
                    "optimize_in_frame")
        return pose7, ok

    def undistort_points(self, src, count, K4, D4, R, P, dst=None):
        """flvis_hip_undistort_points = cv::undistortPoints(src, dst, K, D, R, P): src float32 [n,cap,2], count int32 [n] (device) -> dst
        float32 [n,cap,2] (the caller's, or a new zeroed one).  K4 [4] / D4 [4] / R [3,3] / P [3,4]: one camera; with a leading [n]: one
        per set."""
        import torch
        src = src.contiguous()
        n, cap, _ = src.shape
        K, D = np.ascontiguousarray(K4, np.float64), np.ascontiguousarray(D4, np.float64)
        R, P = np.ascontiguousarray(R, np.float64), np.ascontiguousarray(P, np.float64)
        n_cam = 1 if K.ndim == 1 else n
        assert K.size == 4 * n_cam and D.size == 4 * n_cam and R.size == 9 * n_cam and P.size == 12 * n_cam
        assert src.dtype == torch.float32 and count.dtype == torch.int32
        dst = torch.zeros_like(src) if dst is None else dst
        assert dst.is_contiguous() and dst.shape == src.shape and dst.dtype == torch.float32
        self._check(self._lib.flvis_hip_undistort_points(self._h, _ptr(src), _ptr(count), cap, n, _P(K, C.c_double), _P(D, C.c_double),
                                                         _P(R, C.c_double), _P(P, C.c_double), n_cam, _ptr(dst)), "undistort_points")
        return dst

    def project_points(self, p3d, count, pose7, K4, D4, dst=None):
        """flvis_hip_project_points = cv::projectPoints: p3d float32 [n,cap,3], count int32 [n] (device), pose7 float64 [n,7] (host: the pose
        each set is projected with) -> dst float32 [n,cap,2] (the caller's, or a new zeroed one).  K4 / D4 [4]: one camera; [n,4]: one per set."""
        import torch
        p3d = p3d.contiguous()
        n, cap, _ = p3d.shape
        K, D = np.ascontiguousarray(K4, np.float64), np.ascontiguousarray(D4, np.float64)
        T = np.ascontiguousarray(pose7, np.float64)
        n_cam = 1 if K.ndim == 1 else n
        assert K.size == 4 * n_cam and D.size == 4 * n_cam and T.shape == (n, 7)
        assert p3d.dtype == torch.float32 and count.dtype == torch.int32
        dst = torch.zeros((n, cap, 2), dtype=torch.float32, device=p3d.device) if dst is None else dst
        assert dst.is_contiguous() and dst.shape == (n, cap, 2) and dst.dtype == torch.float32
        self._check(self._lib.flvis_hip_project_points(self._h, _ptr(p3d), _ptr(count), cap, n, _P(T, C.c_double), _P(K, C.c_double),
                                                       _P(D, C.c_double), n_cam, _ptr(dst)), "project_points")
        return dst

    def debug_epnp(self, p3d, p2d, count, K4):
        """flvis_hip_debug_epnp: EPnP alone on correspondence sets (p3d float32 [n,cap,3], p2d float32 [n,cap,2], count int32 [n], device)
        -> float64 [n,160] (layout in include/flvis_hip.h)."""
        import torch
        p3d, p2d = p3d.contiguous(), p2d.contiguous()
        n, cap, _ = p3d.shape
        K = np.ascontiguousarray(K4, np.float64)
        out = torch.zeros((n, 160), dtype=torch.float64, device=p3d.device)
        self._check(self._lib.flvis_hip_debug_epnp(self._h, _ptr(p3d), _ptr(p2d), _ptr(count), cap, n, _P(K, C.c_double), _ptr(out)), "debug_epnp")
        return out

    def pgo_loop_closure(self, T_c_w_list, present_list, loops_list, loop_poses_list, iterations=100, use_initial_guess=True):
        """flvis_hip_pgo_loop_closure for a batch of pose graphs (lists of per-graph numpy arrays: T_c_w [n,7], present [n], loops
        [m,2], loop poses [m,7]).  Returns (list of optimised T_c_w arrays, drift [g,7], stats [g,5], ran [g])."""
        import torch
        g = len(T_c_w_list)
        n_kf = np.array([len(t) for t in T_c_w_list], np.int32)
        n_loops = np.array([len(l) for l in loops_list], np.int32)
        T = torch.from_numpy(np.ascontiguousarray(np.concatenate(T_c_w_list), np.float64).reshape(-1, 7)).cuda()
        pres = np.ascontiguousarray(np.concatenate(present_list), np.uint8)
        loops = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1, 2) for l in loops_list] + [np.zeros((1, 2), np.int32)]), np.int32)
        lp = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 7) for p in loop_poses_list] +
                                                                  [np.zeros((1, 7))]))).cuda()
        drift = torch.zeros((g, 7), dtype=torch.float64, device="cuda")
        stats = torch.zeros((g, 5), dtype=torch.float64, device="cuda")
        ran = np.zeros(g, np.int32)
        self._check(self._lib.flvis_hip_pgo_loop_closure(self._h, g, _P(n_kf, C.c_int), _ptr(T), _P(pres, C.c_uint8), _P(n_loops, C.c_int),
                                                         _P(loops, C.c_int), _ptr(lp), int(iterations), bool(use_initial_guess),
                                                         _ptr(drift), _ptr(stats), _P(ran, C.c_int)), "pgo_loop_closure")
        self._check(self._lib.flvis_hip_synchronize(self._h), "synchronize")
        out = T.cpu().numpy()
        res, o = [], 0
        for k in n_kf:
            res.append(out[o:o + k].copy())
            o += k
        return res, drift.cpu().numpy(), stats.cpu().numpy(), ran


def voxel_cloud_info():
    """flvis_hip_voxel_cloud_info: dict(sort_tile, workgroup, bytes_per_point, bytes_per_row) -- constants of the build, no device needed"""
    lib = load_library()
    info = (C.c_int * 4)()
    if lib.flvis_hip_voxel_cloud_info(info) != FLVIS_OK:
        raise FlvisError("voxel_cloud_info failed")
    return dict(sort_tile=info[0], workgroup=info[1], bytes_per_point=info[2], bytes_per_row=info[3])


OCCUPANCY_CAST_STATUS = ("end", "occupied", "unknown", "dropped", "limit")   # flvis_hip_occupancy_cast's d_status 0 .. 4


def occupancy_info():
    """flvis_hip_occupancy_info: dict(workgroup, bytes_per_record, bytes_per_ray, bytes_per_image) -- constants of the build, no device needed"""
    lib = load_library()
    info = (C.c_int * 4)()
    if lib.flvis_hip_occupancy_info(info) != FLVIS_OK:
        raise FlvisError("occupancy_info failed")
    return dict(workgroup=info[0], bytes_per_record=info[1], bytes_per_ray=info[2], bytes_per_image=info[3])
