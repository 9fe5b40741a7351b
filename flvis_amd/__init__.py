"""flvis_amd -- MI355X-native (gfx950) FLVIS front-end tracking + local-map BA hot path.

Thin ctypes binding over the C ABI in include/flvis_hip.h (libflvis_hip.so, hand-written HIP kernels).  PyTorch is
used only as plumbing (device buffers, streams).  There is NO CPU fallback: without a HIP device every call raises.
"""
import ctypes as C
import os

from . import build as _build

_LIB = None

FLVIS_OK = 0
FLVIS_ERR_INVALID_ARG = -1
FLVIS_ERR_NO_DEVICE = -2
FLVIS_ERR_CAPACITY = -4
FLVIS_ERR_CONFIG = -5


class FlvisError(RuntimeError):
    pass


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
    _LIB.flvis_version.restype = C.c_char_p
    _LIB.flvis_last_error.restype = C.c_char_p
    _LIB.flvis_last_error.argtypes = [C.c_void_p]
    _LIB.flvis_hip_stream.restype = C.c_void_p
    _LIB.flvis_hip_stream.argtypes = [C.c_void_p]
    return _LIB


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


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
        rc = self._lib.flvis_hip_create(C.c_int(device), stream, C.byref(h))
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
        self._check(self._lib.flvis_debug_pyramid(self._h, _ptr(img), w, h, n, levels, bx, by, 1 if ingest else 0, _ptr(buf), C.c_size_t(off)), "debug_pyramid")
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
                                                 C.c_double(eps), int(use_initial)), "lk_track")
        return out, status

    def rand_seed(self, seed, n_sets):
        """flvis_hip_rand_seed: the glibc rand() state of n_sets sets after srand(seed) (int32 [n_sets, 35] on the device)."""
        import torch
        st = torch.zeros((n_sets, 35), dtype=torch.int32, device=self.device)
        self._check(self._lib.flvis_hip_rand_seed(self._h, C.c_uint32(seed), _ptr(st), n_sets), "rand_seed")
        return st

    def stereo_depth(self, cfg, img0, img1, pt2d_plane, pt2d_undistort, pt3d_w, has_depth, count, poses7, rng, rand_state, out=None, mask=None):
        """flvis_hip_stereo_depth = CameraFrame::recover3DPts_c_FromStereo (camera_frame.cpp:93-180) for n_sets frames in one call.
        img0 / img1 uint8 [n,h,w]; pt2d_* float32 [n,cap,2]; pt3d_w float32 [n,cap,3]; has_depth uint8 [n,cap]; count int32 [n] (all on
        the device); poses7 host [n,7]; rand_state from rand_seed() (updated in place).  Returns (pt3ds float64 [n,cap,3], mask uint8):
        out / mask when the caller passes its own (the call writes the first min(count, cap) slots of a set and no other), else new
        zero-filled tensors."""
        import numpy as np
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
        self._lib.flvis_hip_stereo_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
        self._check(self._lib.flvis_hip_stereo_depth(self._h, C.byref(cfg), _ptr(img0), _ptr(img1), n, _ptr(pt2d_plane),
                                                     _ptr(pt2d_undistort), _ptr(pt3d_w), _ptr(has_depth), _ptr(count), cap,
                                                     T.ctypes.data, C.c_float(rng), _ptr(rand_state), _ptr(out), _ptr(mask)),
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
        import numpy as np
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
        f.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 10
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
        self._check(self._lib.flvis_hip_gftt(self._h, _ptr(img), w, h, n, max_corners, C.c_double(quality),
                                             C.c_double(min_distance), _ptr(out), _ptr(cnt)), "gftt")
        return out, cnt

    def debug_corner_response(self, img, variant, rows=0, key_cap=1 << 17):
        """test aid: (max ordered bits [n], sorted candidate keys per image) of the corner-response pass with the chosen kernel"""
        import numpy as np
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
        self._check(self._lib.flvis_hip_debug_sqrt_check(self._h, C.c_uint32(first_bits), C.c_uint32(n), C.byref(bad)), "sqrt_check")
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
        import numpy as np
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
                                                  C.c_double(ratio_max), _ptr(pairs), _ptr(npairs)), "orb_match")
        return pairs, npairs


    def bow_set_vocabulary(self, child_ptr, child_idx, desc, weight, word_id):
        """flvis_hip_bow_set_vocabulary: the DBoW3 tree as flat arrays (see include/flvis_hip.h)."""
        import numpy as np
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
        self._lib.flvis_hip_voc_train.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self._lib.flvis_hip_voc_train(self._h, _ptr(desc), _ptr(count), desc.shape[1], desc.shape[0], C.byref(prm), C.byref(h),
                                                  stats), "voc_train")
        return TrainedVocabulary(self._lib, h, list(stats))

    def bow_load_vocabulary(self, path):
        """flvis_hip_bow_load_vocabulary: `Vocabulary voc(path)` of vo_loopclosing.cpp:1097 (.dbow3 / .txt / .yml / .yml.gz)."""
        self._check(self._lib.flvis_hip_bow_load_vocabulary(self._h, C.c_char_p(os.fsencode(path))), "bow_load_vocabulary")

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
        import numpy as np
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
        import numpy as np
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
        import numpy as np
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
        fn = self._lib.flvis_hip_voxel_cloud
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                       C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self._check(fn(self._h, _ptr(p3), _ptr(count), _ptr(T_c_w), n_rows, pcap, nc, _P(ptr, C.c_int), _P(rng, C.c_int), float(leaf),
                       int(min_points), cap, _ptr(xyz), _ptr(npts), _P(n_out, C.c_int64), _P(n_drop, C.c_int64)), "voxel_cloud")
        k = [int(min(n, cap)) for n in n_out[:nc]]
        hx = xyz.cpu().numpy()
        hn = npts.cpu().numpy() if want_npts else None
        return ([hx[c, :k[c]].copy() for c in range(nc)], [hn[c, :k[c]].copy() for c in range(nc)] if want_npts else None,
                n_out[:nc].copy(), n_drop[:nc].copy())

    def voxel_cloud_stats(self):
        """flvis_hip_voxel_cloud_stats: dict(passes_run, passes_skipped, workspace_bytes, input_points) of the context's last call"""
        import numpy as np
        st = np.zeros(4, np.int64)
        self._lib.flvis_hip_voxel_cloud_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        self._check(self._lib.flvis_hip_voxel_cloud_stats(self._h, _P(st, C.c_int64)), "voxel_cloud_stats")
        return dict(passes_run=int(st[0]), passes_skipped=int(st[1]), workspace_bytes=int(st[2]), input_points=int(st[3]))

    def lc_map_poses(self, T_odom, T_map, stamps, nkf, jobs, mode=0, drift=None):
        """flvis_hip_lc_map_poses: pose rows into the map frame.  T_odom, T_map float64 [n_seq, kf_stride, 7], stamps float64 [n_seq,
        kf_stride] (device tensors), nkf: keyframes per sequence, drift [n_seq, 7]: the sequences' T_odom_map (read for empty ones).
        jobs: dicts seq / kind (LC_ROWS_*) / rows (device float64 [n, 8 | 9 | 11]) and optionally out (a device tensor of the same
        shape, or "inplace"; default: a new tensor) and anchor (False: no anchor array).  mode: LC_TRAJ_ANCHOR or LC_TRAJ_BLEND.
        -> per job (rows in the map frame, anchors int32 [n] or None), device tensors."""
        import numpy as np
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
        fn = self._lib.flvis_hip_lc_map_poses
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int,
                       C.POINTER(FlvisLcTrajJob), C.c_int]
        self._check(fn(self._h, n_seq, stride, _P(nkf, C.c_int), _ptr(T_odom), _ptr(T_map), _ptr(stamps),
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
        self._lib.flvis_hip_lc_select_maps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                       C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self._lib.flvis_hip_lc_select_maps(self._h, n_q, _ptr(scores), n_seg, seg_len, _ptr(seg_n.contiguous()),
                                                       _ptr(maps.contiguous()), int(n_best), float(min_score), _ptr(idx), _ptr(sc), _ptr(cnt)),
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
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                       C.c_void_p, C.c_void_p]
        self._check(fn(self._h, n_q, _ptr(scores), n_seg, seg_len, _ptr(seg_n.contiguous()), _ptr(maps.contiguous()), _ptr(skip), int(n_best),
                       float(min_score), _ptr(idx), _ptr(sc), _ptr(cnt)), "lc_select_maps_skip")
        return idx, sc, cnt

    def lc_keyframe_landmarks(self, img0, img1, cam_type, kps, desc, count, P0=None, P1=None, K4=None, in_place=False):
        """flvis_hip_lc_keyframe_landmarks (vo_loopclosing.cpp:255-372): kps float32 [n,cap,6], desc uint8 [n,cap,32], count int32 [n] as
        orb_detect_and_compute returns them; img0 uint8 [n,h,w]; img1 uint8 (stereo, cam_type 0) or int16/uint16 Z16 (depth, cam_type 2).
        P0 / P1 [12] or K4 [4]: one camera for every image; [n,12] / [n,4]: one per image (flvis_hip_lc_keyframe_landmarks_rigs).
        Returns (lm_2d float32 [n,cap,2], lm_3d float64 [n,cap,3], lm_desc uint8 [n,cap,32], lm_count int32 [n])."""
        import numpy as np
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
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FlvisCfg), C.c_int, C.c_void_p, C.c_void_p,
                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(fn(self._h, _ptr(img0), _ptr(img1), w, h, n, arr, len(cfgs), _ptr(kps), _ptr(desc), _ptr(count), cap, _ptr(lm2), _ptr(lm3),
                       _ptr(lmd), _ptr(cnt)), "lc_keyframe_landmarks_unrect")
        return lm2, lm3, lmd, cnt

    def pnp_ransac(self, p3d, p2d, count, K4, seeds, iterations=100, reproj_px=2.0, confidence=0.99):
        """flvis_hip_pnp_ransac: p3d float32 [n,cap,3], p2d float32 [n,cap,2], count int32 [n] (device) -> (pose7 [n,7], mask [n,cap],
        n_inliers [n]).  K4 [4]: one camera for every set; [n,4]: one per set (flvis_hip_pnp_ransac_rigs)."""
        import numpy as np
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
        self._check(fn(self._h, _ptr(p3d), _ptr(p2d), _ptr(count), cap, n, _P(K, C.c_double), int(iterations), C.c_double(reproj_px),
                       C.c_double(confidence), _P(sd, C.c_uint64), _ptr(pose), _ptr(mask), _ptr(ninl)), "pnp_ransac")
        return pose, mask, ninl

    def debug_pnp_ransac_iterative(self, p3d, p2d, count, K4, guess7, iterations=100, reproj_px=3.0, confidence=0.99):
        """flvis_hip_debug_pnp_ransac_iterative: the tracker's branch of the PnP RANSAC (5-point EPnP hypotheses, Gauss-Newton on the inliers;
        its parameters are the defaults) on the arrays of pnp_ransac, guess7 float64 [n,7] (host) -> (pose7 [n,7], mask [n,cap],
        n_inliers [n]); a set without a model gets its guess back."""
        import numpy as np
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
            self._h, _ptr(p3d), _ptr(p2d), _ptr(count), cap, n, _P(K, C.c_double), int(iterations), C.c_double(reproj_px),
            C.c_double(confidence), _P(g7, C.c_double), _ptr(pose), _ptr(mask), _ptr(ninl)), "debug_pnp_ransac_iterative")
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
        self._check(self._lib.flvis_hip_find_fundamental_ransac(self._h, _ptr(m1), _ptr(m2), _ptr(count), cap, n, C.c_double(thr_px),
                                                                C.c_double(confidence), _ptr(mask), _ptr(n_inliers)),
                    "find_fundamental_ransac")
        return mask, n_inliers

    def optimize_in_frame(self, lm_3d_w, lm_2d_undistort, lm_id, count, K4, pose7, ok=None):
        """flvis_hip_optimize_in_frame = OptimizeInFrame::optimize (optimize_in_frame.cpp:10-91): lm_3d_w float64 [n,cap,3], lm_2d_undistort
        float64 [n,cap,2], lm_id int64 [n,cap], count int32 [n], pose7 float64 [n,7] (device; T_c_w, updated IN PLACE where ok) ->
        (pose7, ok uint8 [n]).  K4 [4]: one camera for every set; [n,4]: one per set."""
        import numpy as np
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
        import numpy as np
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
        import numpy as np
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
        import numpy as np
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
        import numpy as np
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
                                                         _P(loops, C.c_int), _ptr(lp), int(iterations), int(bool(use_initial_guess)),
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
    lib.flvis_hip_voxel_cloud_info.argtypes = [C.POINTER(C.c_int)]
    if lib.flvis_hip_voxel_cloud_info(info) != FLVIS_OK:
        raise FlvisError("voxel_cloud_info failed")
    return dict(sort_tile=info[0], workgroup=info[1], bytes_per_point=info[2], bytes_per_row=info[3])


def loop_candidate(row, present, lcKFDist, lcKFMaxDist, lcNKFClosest, minScore):
    """flvis_loop_candidate (host control logic of isLoopCandidate): returns the earlier keyframe's index or None."""
    import numpy as np
    lib = load_library()
    row = np.ascontiguousarray(row, np.float64)
    pres = np.ascontiguousarray(present, np.uint8)
    out = C.c_int64(-1)
    lib.flvis_loop_candidate.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_double,
                                         C.POINTER(C.c_int64)]
    r = lib.flvis_loop_candidate(len(row), _P(row, C.c_double), _P(pres, C.c_uint8), lcKFDist, lcKFMaxDist, lcNKFClosest,
                                 C.c_double(minScore), C.byref(out))
    if r < 0:
        raise FlvisError("flvis_loop_candidate failed: %d" % r)
    return int(out.value) if r == 1 else None


def read_vocabulary_file(path):
    """flvis_voc_file_* (host only): a DBoW3 vocabulary file as the flat arrays `Context.bow_set_vocabulary` takes.

    Returns a dict: child_ptr, child_idx, desc [n,32], weight, word_id (-1 on inner nodes), k, L, scoring, weighting, n_words,
    layout ("binary" | "binary-quicklz" | "text" | "yaml")."""
    import numpy as np
    lib = load_library()
    h = C.c_void_p(0)
    err = C.create_string_buffer(512)
    lib.flvis_voc_file_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
    rc = lib.flvis_voc_file_open(os.fsencode(path), C.byref(h), err, 512)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_voc_file_open(%s): %s" % (path, err.value.decode(errors="replace") or rc))
    try:
        return _voc_handle_dict(lib, h)
    finally:
        lib.flvis_voc_file_close.argtypes = [C.c_void_p]
        lib.flvis_voc_file_close(h)


_VOC_LAYOUTS = ["binary", "binary-quicklz", "text", "yaml", "trained"]


def _voc_handle_dict(lib, h):
    """the content of a flvis_voc_file handle, copied out"""
    import numpy as np
    info = (C.c_int * 8)()
    lib.flvis_voc_file_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.flvis_voc_file_info(h, info)
    n, n_words, k, L, scoring, weighting, n_edges, layout = list(info)
    ptrs = [C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_double)(), C.POINTER(C.c_int)()]
    lib.flvis_voc_file_arrays.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    lib.flvis_voc_file_arrays(h, *[C.byref(q) for q in ptrs])
    take = lambda q, cnt, dt: np.ctypeslib.as_array(q, shape=(cnt,)).astype(dt, copy=True) if cnt else np.zeros(0, dt)
    return {"child_ptr": take(ptrs[0], n + 1, np.int32), "child_idx": take(ptrs[1], n_edges, np.int32),
            "desc": take(ptrs[2], n * 32, np.uint8).reshape(n, 32), "weight": take(ptrs[3], n, np.float64),
            "word_id": take(ptrs[4], n, np.int32), "k": k, "L": L, "scoring": scoring, "weighting": weighting,
            "n_words": n_words, "layout": _VOC_LAYOUTS[layout]}


def save_vocabulary_file(path, arrays, k, L, scoring=0, weighting=0):
    """flvis_voc_file_save_arrays (host only): the flat arrays (child_ptr, child_idx, desc [n,32], weight, word_id) as an uncompressed
    binary .dbow3 file, byte for byte what DBoW3's Vocabulary::save(path, false) writes."""
    import numpy as np
    lib = load_library()
    cp = np.ascontiguousarray(arrays[0], np.int32)
    ci = np.ascontiguousarray(arrays[1], np.int32)
    ds = np.ascontiguousarray(arrays[2], np.uint8)
    wt = np.ascontiguousarray(arrays[3], np.float64)
    wi = np.ascontiguousarray(arrays[4], np.int32)
    n = len(cp) - 1
    if ds.shape != (n, 32) or len(wt) != n or len(wi) != n or len(ci) != n - 1:
        raise FlvisError("save_vocabulary_file: the arrays do not describe one tree of %d nodes" % n)
    lib.flvis_voc_file_save_arrays.argtypes = [C.c_char_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 4
    rc = lib.flvis_voc_file_save_arrays(os.fsencode(path), 0, n, cp.ctypes.data, ci.ctypes.data, ds.ctypes.data, wt.ctypes.data,
                                        wi.ctypes.data, int(k), int(L), int(scoring), int(weighting))
    if rc != FLVIS_OK:
        raise FlvisError("flvis_voc_file_save_arrays(%s) failed (%d)" % (path, rc))


def convert_vocabulary_file(src, dst):
    """flvis_voc_file_open + flvis_voc_file_save (host only): any readable vocabulary file rewritten as an uncompressed .dbow3."""
    lib = load_library()
    h = C.c_void_p(0)
    err = C.create_string_buffer(512)
    lib.flvis_voc_file_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
    rc = lib.flvis_voc_file_open(os.fsencode(src), C.byref(h), err, 512)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_voc_file_open(%s): %s" % (src, err.value.decode(errors="replace") or rc))
    try:
        lib.flvis_voc_file_save.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        rc = lib.flvis_voc_file_save(h, os.fsencode(dst), 0)
        if rc != FLVIS_OK:
            raise FlvisError("flvis_voc_file_save(%s) failed (%d)" % (dst, rc))
    finally:
        lib.flvis_voc_file_close.argtypes = [C.c_void_p]
        lib.flvis_voc_file_close(h)


class VocTrainParams(C.Structure):
    """flvis_voc_train_params of include/flvis_hip.h."""
    _fields_ = [("k", C.c_int), ("L", C.c_int), ("weighting", C.c_int), ("seed", C.c_uint), ("max_iters", C.c_int),
                ("small_node_max", C.c_int)]


class TrainedVocabulary:
    """What Context.voc_train returns: .arrays (child_ptr, child_idx, desc, weight, word_id with 0 on inner nodes -- the 5-tuple
    Context.bow_set_vocabulary takes), .info (the dict read_vocabulary_file returns, word_id -1 on inner nodes), .stats (descriptors,
    nodes, words, passes, capped, empty, trivial, launches), .save(path), .close()."""
    STATS = ("descriptors", "nodes", "words", "passes", "capped", "empty", "trivial", "launches")

    def __init__(self, lib, h, stats):
        import numpy as np
        self._lib, self._h = lib, h
        self.info = _voc_handle_dict(lib, h)
        self.stats = dict(zip(self.STATS, [int(x) for x in stats]))
        i = self.info
        self.arrays = (i["child_ptr"], i["child_idx"], i["desc"], i["weight"], np.maximum(i["word_id"], 0).astype(np.int32))

    def save(self, path):
        """flvis_voc_file_save: an uncompressed binary .dbow3 file"""
        if not self._h:
            raise FlvisError("TrainedVocabulary.save: closed")
        self._lib.flvis_voc_file_save.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        rc = self._lib.flvis_voc_file_save(self._h, os.fsencode(path), 0)
        if rc != FLVIS_OK:
            raise FlvisError("flvis_voc_file_save(%s) failed (%d)" % (path, rc))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.flvis_voc_file_close.argtypes = [C.c_void_p]
            self._lib.flvis_voc_file_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OrbParams(C.Structure):
    """flvis_orb_params of include/flvis_hip.h."""
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int), ("fast_threshold", C.c_int)]


def orb_default_pattern():
    """flvis_orb_default_pattern (host only): the built-in 256-pair sampling pattern as int8 [512,2]."""
    import numpy as np
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
    lib.flvis_config_get_bool.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    rc = lib.flvis_config_get_bool(yaml_path.encode(), key.encode(), C.byref(out), err, 256)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_config_get_bool(%s, %s) failed (%d): %s" % (yaml_path, key, rc, err.value.decode()))
    return bool(out.value)


def _P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class FlvisImage(C.Structure):
    """flvis_image of include/flvis_hip.h: one host image (pitch in bytes)."""
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("width", C.c_int), ("height", C.c_int), ("pitch", C.c_int), ("channels", C.c_int),
                ("t", C.c_double)]


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


def links_from_fix(fix, stream, kf):
    """The links a localize_in result yields when its query frame is also stored as keyframe `kf` of sequence `stream`: one per accepted
    candidate, from (candidate's sequence, candidate's keyframe) to (stream, kf) with the candidate's PnP pose.  -> list of dicts
    (seq_from, kf_from, seq_to, kf_to, pose) for LoopCloser.merge.  (C callers have flvis_lc_links_from_fix.)"""
    return [dict(seq_from=int(c["seq"]), kf_from=int(c["kf"]), seq_to=int(stream), kf_to=int(kf), pose=[float(x) for x in c["pose"]])
            for c in fix["candidates"] if c["accepted"]]


class FlvisLcLinkQuery(C.Structure):
    """flvis_lc_link_query of include/flvis_hip.h: a stored keyframe as the query of flvis_loop_closer_link."""
    _fields_ = [("stream", C.c_int), ("map", C.c_int), ("kf", C.c_int64), ("own_gap", C.c_int64)]


def _link_dict(l):
    return dict(seq_from=int(l.seq_from), kf_from=int(l.kf_from), seq_to=int(l.seq_to), kf_to=int(l.kf_to), pose=[float(x) for x in l.pose7])


def _link_struct(l):
    return l if isinstance(l, FlvisLcLink) else FlvisLcLink(int(l["seq_from"]), int(l["seq_to"]), int(l["kf_from"]), int(l["kf_to"]),
                                                             (C.c_double * 7)(*[float(x) for x in l["pose"]]))


def links_reverse(links):
    """flvis_lc_link_reverse on each link (dicts as links_from_fix makes them, or FlvisLcLink): the ends swapped and the pose inverted --
    what LoopCloser.merge needs for links whose `from` sequence comes after their `to` sequence in the group.  -> list of dicts.  Host-only."""
    lib = load_library()
    lib.flvis_lc_link_reverse.argtypes = [C.POINTER(FlvisLcLink), C.POINTER(FlvisLcLink)]
    out = []
    for l in links:
        a, b = _link_struct(l), FlvisLcLink()
        rc = lib.flvis_lc_link_reverse(C.byref(a), C.byref(b))
        if rc != FLVIS_OK:
            raise FlvisError("flvis_lc_link_reverse failed (%d): a pose that is not finite, or a zero quaternion" % rc)
        out.append(_link_dict(b))
    return out


def load_lc_params(yaml_path):
    """flvis_lc_params_load: the loop-closing block of the reference's yaml files.  Host-only."""
    prm = LcParams()
    err = C.create_string_buffer(256)
    rc = load_library().flvis_lc_params_load(os.fsencode(yaml_path), C.byref(prm), err, 256)
    if rc != FLVIS_OK:
        raise FlvisError("flvis_lc_params_load(%s) failed (%d): %s" % (yaml_path, rc, err.value.decode()))
    return prm


class LoopCloser:
    """flvis_loop_closer: LoopClosingNodeletClass (vo_loopclosing.cpp) for n_streams sequences; the keyframe database stays on the GPU.

    cfg: one config for every sequence, or a sequence of configs -- one camera per sequence (flvis_loop_closer_create_rigs: cam_type and
    the image size must agree, FlvisError otherwise; n_streams is then their number).  self.cfg is sequence 0's."""

    def __init__(self, ctx, cfg, prm, n_streams=1, max_keyframes=2000, orb_pattern=None):
        import numpy as np
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
            self._lib.flvis_loop_closer_create_rigs.argtypes = [C.c_void_p, C.POINTER(FlvisCfg), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                                C.c_void_p]
            ctx._check(self._lib.flvis_loop_closer_create_rigs(ctx._h, arr, C.byref(prm), int(n_streams), int(max_keyframes), patp,
                                                               C.byref(h)), "loop_closer_create_rigs")
        self._h = h
        self._lib.flvis_loop_closer_destroy.argtypes = [C.c_void_p]

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
            self._lib.flvis_loop_closer_reset.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            self._ctx._check(self._lib.flvis_loop_closer_reset(self._h, len(ids), arr), "loop_closer_reset")
            return
        cfgs = [cfgs] if isinstance(cfgs, FlvisCfg) else list(cfgs)
        if len(cfgs) != len(ids):
            raise ValueError("LoopCloser.reset: %d configs for %d streams" % (len(cfgs), len(ids)))
        carr = (FlvisCfg * max(1, len(ids)))(*cfgs)
        self._lib.flvis_loop_closer_reset_rigs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(FlvisCfg)]
        self._ctx._check(self._lib.flvis_loop_closer_reset_rigs(self._h, len(ids), arr, carr), "loop_closer_reset_rigs")

    def stream_cfg(self, s):
        """flvis_loop_closer_stream_cfg: the config sequence s runs on (as created, or as last reset with reset(..., cfgs))."""
        out = FlvisCfg()
        self._lib.flvis_loop_closer_stream_cfg.argtypes = [C.c_void_p, C.c_int, C.POINTER(FlvisCfg)]
        self._ctx._check(self._lib.flvis_loop_closer_stream_cfg(self._h, int(s), C.byref(out)), "loop_closer_stream_cfg")
        return out

    def set_stereo_unrect(self, enable):
        """flvis_loop_closer_set_stereo_unrect: on a STEREO_UNRECT closer (cam_type 1, the EuRoC camera) keyframes and queries get their
        landmarks by this project's rule (Context.lc_keyframe_landmarks_unrect) instead of the reference's empty case.  Pixels and poses
        are then of the rectified camera 0.  FlvisError on another cam_type, and while any sequence holds a keyframe."""
        self._lib.flvis_loop_closer_set_stereo_unrect.argtypes = [C.c_void_p, C.c_int]
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
        import numpy as np
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
        import numpy as np
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
        fn = self._lib.flvis_loop_closer_add_logged
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self._ctx._check(fn(self._h, int(bool(process)), C.cast(ev, C.c_void_p) if process else None, cap, C.byref(n)),
                         "loop_closer_add_logged")
        if not process:
            return [[] for _ in range(n.value)]
        return [self._events(ev[r * S:(r + 1) * S]) for r in range(n.value)]

    @staticmethod
    def _fixes(fix):
        import numpy as np
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
        import numpy as np
        st = np.ascontiguousarray(streams, np.int32)
        n = len(st)
        args, types = [_P(st, C.c_int)], [C.POINTER(C.c_int)]
        if maps is not None:
            mp = np.ascontiguousarray(maps, np.int32)
            assert len(mp) == n, "one map per query"
            args, types = args + [_P(mp, C.c_int)], types + [C.POINTER(C.c_int)]
        if host:
            a, b, keep = self._host_images(img0, img1, n)
            args, types = args + [a, b], types + [C.POINTER(FlvisImage), C.POINTER(FlvisImage)]
        else:
            img0, img1 = self._device_images(img0, img1, n)
            args, types = args + [_ptr(img0), _ptr(img1)], types + [C.c_void_p, C.c_void_p]
        Fix = FlvisLcFix if maps is None else FlvisLcFixIn
        fix = (Fix * max(1, n))()
        fn.argtypes = [C.c_void_p, C.c_int] + types + [C.c_int, C.POINTER(Fix)]
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
        self._lib.flvis_loop_closer_link.argtypes = [C.c_void_p, C.c_int, C.POINTER(FlvisLcLinkQuery), C.c_int, C.POINTER(FlvisLcFixIn), C.c_int,
                                                     C.POINTER(FlvisLcLink), C.POINTER(C.c_int)]
        self._ctx._check(self._lib.flvis_loop_closer_link(self._h, n, arr, int(n_best), fix, cap, links, C.byref(cnt)), "loop_closer_link")
        return self._fixes_in(fix[:n]), [_link_dict(l) for l in links[:cnt.value]]

    def set_drift(self, stream, T_odom_map):
        """flvis_loop_closer_set_drift: the sequence's T_odom_map from now on (keyframes added afterwards get T_c_w_odom * T_odom_map).
        After a tracker slot was reset: set_drift(s, mul(inv(T_c_odom), localize(...)["T_c_map"])) ties its new odometry frame to the map."""
        import numpy as np
        T = np.ascontiguousarray(T_odom_map, np.float64).reshape(7)
        self._lib.flvis_loop_closer_set_drift.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        self._ctx._check(self._lib.flvis_loop_closer_set_drift(self._h, int(stream), _P(T, C.c_double)), "loop_closer_set_drift")

    def merge(self, groups, links, iterations=100):
        """flvis_loop_closer_merge: the maps of each group's sequences become one map in the frame of the group's first sequence, by one
        joint pose graph per group in which `links` (dicts seq_from / kf_from / seq_to / kf_to / pose, as links_from_fix makes them, or
        FlvisLcLink) tie keyframes of different sequences.  groups: lists of at least two sequences, disjoint.  -> (one dict per group:
        optimised / n_vertices / n_edges / iterations / chi2_before / chi2_after, drift [sequences in the groups' order, 7]: what each
        sequence's T_odom_map was multiplied by).  FlvisError, and nothing changes, for arguments the call refuses."""
        import numpy as np
        groups = [[int(s) for s in g] for g in groups]
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), np.int32)
        seqs = np.ascontiguousarray([s for g in groups for s in g], np.int32)
        arr = (FlvisLcLink * max(1, len(links)))()
        for k, l in enumerate(links):
            arr[k] = _link_struct(l)
        out = (FlvisLcMerge * max(1, len(groups)))()
        drift = np.zeros((max(1, len(seqs)), 7))
        self._lib.flvis_loop_closer_merge.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(FlvisLcLink),
                                                      C.c_int, C.POINTER(FlvisLcMerge), C.POINTER(C.c_double)]
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
        import numpy as np
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
        args = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int]
        if host:
            hx, hn = np.zeros(shape + (3,), np.float32), np.zeros(shape, np.int32)
            fn = self._lib.flvis_loop_closer_map_cloud_host
            fn.argtypes = args + [C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            rc = fn(self._h, ng, _P(ptr, C.c_int), _P(seqs, C.c_int), float(leaf), int(min_points), cap, _P(hx, C.c_float), _P(hn, C.c_int),
                    _P(n_out, C.c_int64), _P(n_drop, C.c_int64))
            self._ctx._check(rc, "loop_closer_map_cloud_host")
        else:
            xyz = torch.empty(shape + (3,), dtype=torch.float32, device=self._ctx.device)
            npts = torch.empty(shape, dtype=torch.int32, device=self._ctx.device)
            fn = self._lib.flvis_loop_closer_map_cloud
            fn.argtypes = args + [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            rc = fn(self._h, ng, _P(ptr, C.c_int), _P(seqs, C.c_int), float(leaf), int(min_points), cap, _ptr(xyz), _ptr(npts),
                    _P(n_out, C.c_int64), _P(n_drop, C.c_int64))
            self._ctx._check(rc, "loop_closer_map_cloud")
            kmax = int(min(max(n_out[:ng].max() if ng else 0, 0), cap))
            hx, hn = xyz[:, :kmax].cpu().numpy(), npts[:, :kmax].cpu().numpy()
        k = [int(min(n, cap)) for n in n_out[:ng]]
        return ([hx[g, :k[g]].copy() for g in range(ng)], [hn[g, :k[g]].copy() for g in range(ng)], n_out[:ng].copy(), n_drop[:ng].copy())

    def poses(self, stream=0, cap=None):
        import numpy as np
        cap = int(cap) if cap else self.max_keyframes      # (never fewer rows than the sequence can hold: no silent truncation)
        n = C.c_int(0)
        buf = np.zeros((cap, 7))
        self._ctx._check(self._lib.flvis_loop_closer_poses(self._h, int(stream), _P(buf, C.c_double), cap, C.byref(n)), "loop_closer_poses")
        if n.value > cap:
            raise FlvisError("loop_closer_poses: %d keyframes, buffer of %d" % (n.value, cap))
        return buf[:n.value].copy()

    def keyframe(self, stream, kf, cap=1024):
        """flvis_loop_closer_keyframe -> dict(lm2 [k,2] f32, lm3 [k,3] f64, lmd [k,32] u8, bow=(ids, vals))"""
        import numpy as np
        lm2, lm3, lmd = np.zeros((cap, 2), np.float32), np.zeros((cap, 3)), np.zeros((cap, 32), np.uint8)
        bi, bv = np.zeros(cap, np.int32), np.zeros(cap)
        nl, nv = C.c_int(0), C.c_int(0)
        self._ctx._check(self._lib.flvis_loop_closer_keyframe(self._h, int(stream), int(kf), cap, _P(lm2, C.c_float), _P(lm3, C.c_double),
                                                              _P(lmd, C.c_uint8), C.byref(nl), _P(bi, C.c_int), _P(bv, C.c_double), C.byref(nv)),
                         "loop_closer_keyframe")
        k, v = min(nl.value, cap), min(nv.value, cap)
        return dict(lm2=lm2[:k].copy(), lm3=lm3[:k].copy(), lmd=lmd[:k].copy(), bow=(bi[:v].copy(), bv[:v].copy()))

    def drift(self, stream=0):
        import numpy as np
        T = np.zeros(7)
        self._ctx._check(self._lib.flvis_loop_closer_drift(self._h, int(stream), _P(T, C.c_double)), "loop_closer_drift")
        return T

    def similarity_row(self, stream=0, cap=None):
        import numpy as np
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
        import numpy as np
        t = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        fn = self._lib.flvis_loop_closer_set_keyframe_stamps
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        self._ctx._check(fn(self._h, int(stream), int(first_kf), len(t), _P(t, C.c_double)), "loop_closer_set_keyframe_stamps")

    def keyframe_stamps(self, stream=0):
        """flvis_loop_closer_keyframe_stamps -> float64 [keyframes of the sequence], NaN where never set"""
        import numpy as np
        n = C.c_int(0)
        buf = np.zeros(self.max_keyframes)
        fn = self._lib.flvis_loop_closer_keyframe_stamps
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
        self._ctx._check(fn(self._h, int(stream), _P(buf, C.c_double), self.max_keyframes, C.byref(n)), "loop_closer_keyframe_stamps")
        return buf[:n.value].copy()

    def map_poses(self, jobs, mode=LC_TRAJ_ANCHOR, host=False):
        """flvis_loop_closer_map_poses[_host]: pose rows of the closer's sequences into the map frame, every row with the drift of the
        keyframe it follows (LC_TRAJ_ANCHOR) or the chord between that keyframe's drift and the next one's (LC_TRAJ_BLEND).  jobs: (seq,
        kind, rows) with rows [n, 8 | 9 | 11] of kind LC_ROWS_POSE8 / _TRAJ9 (Tracker.trajectory) / _IMU11 (Tracker.imu_states): device
        float64 tensors, or with host=True numpy arrays.  -> per job (rows in the map frame, anchors int32 [n]: the keyframe, -1 in an
        empty sequence, -2 for a NaN stamp), of the inputs' type.  FlvisError, and nothing is written, when a named sequence holds a
        keyframe without a stamp."""
        import numpy as np
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
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(FlvisLcTrajJob), C.c_int]
        self._ctx._check(fn(self._h, len(jobs), arr, int(mode)), "loop_closer_map_poses_host" if host else "loop_closer_map_poses")
        return [(out, anc) for _, out, anc in res]

    def map_trajectory(self, streams, first, n_frames, mode=LC_TRAJ_ANCHOR, device=False):
        """flvis_loop_closer_map_trajectory: rows first .. first + n_frames - 1 of the trajectory record of the tracker on this closer's
        context, streams `streams` (stream s <-> sequence s), in the map frame; no pose goes through the host on the way.
        -> (rows float64 [n, n_frames, 9], anchors int32 [n, n_frames]) as numpy arrays; device=True: the rows as a device tensor."""
        import numpy as np
        import torch
        st = np.ascontiguousarray(streams, np.int32)
        n, m = len(st), int(n_frames)
        anc = np.zeros((n, max(m, 0)), np.int32)
        fn = self._lib.flvis_loop_closer_map_trajectory
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        if device:
            rows = torch.empty((n, max(m, 0), 9), dtype=torch.float64, device=self._ctx.device)
            rc = fn(self._h, n, _P(st, C.c_int), int(first), m, int(mode), _ptr(rows), None, anc.ctypes.data)
        else:
            rows = np.zeros((n, max(m, 0), 9))
            rc = fn(self._h, n, _P(st, C.c_int), int(first), m, int(mode), None, rows.ctypes.data, anc.ctypes.data)
        self._ctx._check(rc, "loop_closer_map_trajectory")
        return rows, anc


class Tracker:
    """Batched F2FTracking + LocalMap for n_streams independent streams on one GPU (flvis_tracker_create).

    cfg: one config for every stream, or a sequence of n_streams configs -- one per stream, each camera with its own calibration
    (flvis_tracker_create_rigs: the batch-wide fields must agree, FlvisError otherwise).  self.cfg is stream 0's."""

    def __init__(self, ctx, cfg, n_streams, seed_base=0xF1715, traj_capacity=0):
        import numpy as np
        self.ctx = ctx
        self.lib = ctx._lib
        self.S = n_streams
        self.np = np
        if isinstance(cfg, FlvisCfg):
            self.cfg = cfg
            self.lib.flvis_tracker_create.argtypes = [C.c_void_p, C.POINTER(FlvisCfg), C.c_int, C.c_uint64, C.c_int]
            ctx._check(self.lib.flvis_tracker_create(ctx._h, C.byref(cfg), n_streams, seed_base, traj_capacity),
                       "tracker_create")
        else:
            cfgs = list(cfg)
            if len(cfgs) != n_streams:
                raise ValueError("Tracker: %d configs for %d streams" % (len(cfgs), n_streams))
            self.cfg = cfgs[0]
            arr = (FlvisCfg * n_streams)(*cfgs)
            self.lib.flvis_tracker_create_rigs.argtypes = [C.c_void_p, C.POINTER(FlvisCfg), C.c_int, C.c_uint64, C.c_int]
            ctx._check(self.lib.flvis_tracker_create_rigs(ctx._h, arr, n_streams, seed_base, traj_capacity), "tracker_create_rigs")
        self._out = (FrameOut * n_streams)()

    def imu_feed_flvis(self, stream, samples7):
        np = self.np
        a = np.ascontiguousarray(samples7, np.float64).reshape(-1, 7)
        if len(a):
            self.ctx._check(self.lib.flvis_imu_feed_flvis_frame(self.ctx._h, stream, len(a), _P(a, C.c_double)),
                            "imu_feed")

    def imu_feed_sensor(self, stream, t, acc, gyro):
        a = (C.c_double * 3)(*[float(x) for x in acc])
        g = (C.c_double * 3)(*[float(x) for x in gyro])
        self.ctx._check(self.lib.flvis_imu_feed(self.ctx._h, stream, C.c_double(t), a, g), "imu_feed")

    def imu_feed_out(self, stream, t, acc, gyro):
        """F2FTracking::imu_feed with its outputs: integrates the sensor-frame sample now; returns (q_w_i wxyz, pos_w_i, vel_w_i)."""
        np = self.np
        a = (C.c_double * 3)(*[float(x) for x in acc])
        g = (C.c_double * 3)(*[float(x) for x in gyro])
        q, p, v = np.zeros(4), np.zeros(3), np.zeros(3)
        self.ctx._check(self.lib.flvis_imu_feed_out(self.ctx._h, stream, C.c_double(t), a, g, _P(q, C.c_double), _P(p, C.c_double),
                                                    _P(v, C.c_double)), "imu_feed_out")
        return q, p, v

    def imu_states(self, stream, cap=512):
        """Rows (t, q_w_i wxyz, pos_w_i, vel_w_i) of the IMU samples integrated since the previous call; also the rows lost."""
        np = self.np
        rows = np.zeros((cap, 11), np.float64)
        n, dropped = C.c_int(0), C.c_int(0)
        self.ctx._check(self.lib.flvis_get_imu_states(self.ctx._h, stream, cap, _P(rows, C.c_double), C.byref(n), C.byref(dropped)),
                        "get_imu_states")
        return rows[:n.value].copy(), dropped.value

    def debug_vi_state(self, stream, cap=400):
        """Test aid (flvis_debug_vi_state): the stream's filter after the staged samples -> dict(rows [n, 11] oldest first as
        (t, q_w_i wxyz, pos_w_i, vel_w_i), biases [6] (acc, gyro), flags [4] (has_imu, vi_first, vi_initialized, vi_count))."""
        np = self.np
        rows, biases, flags = np.zeros((cap, 11), np.float64), np.zeros(6, np.float64), np.zeros(4, np.int32)
        self.lib.flvis_debug_vi_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                  C.POINTER(C.c_int32)]
        n = self.lib.flvis_debug_vi_state(self.ctx._h, stream, cap, _P(rows, C.c_double), _P(biases, C.c_double), _P(flags, C.c_int32))
        if n < 0:
            self.ctx._check(n, "debug_vi_state")
        return dict(rows=rows[:min(n, cap)].copy(), biases=biases, flags=flags)

    def local_map_counts(self):
        """(keyframes emitted, local-map optimisations run) per stream"""
        np = self.np
        kf, ba = np.zeros(self.S, np.int64), np.zeros(self.S, np.int64)
        self.ctx._check(self.lib.flvis_get_local_map_counts(self.ctx._h, _P(kf, C.c_int64), _P(ba, C.c_int64)), "get_local_map_counts")
        return kf, ba

    def write_imu_trajectory(self, rows11, path, min_dt=0.0, append=False, t_first=None):
        """The recorder on /imu_pose: rows of imu_states() as `stamp x y z qw qx qy qz` lines; returns the lines written.
        t_first: the stamp of the run's first row (flvis_write_imu_trajectory_run) -- pass it with every batch of a run whose first
        batch may cover less than min_dt."""
        np = self.np
        r = np.ascontiguousarray(rows11, np.float64).reshape(-1, 11)
        if t_first is not None:
            self.lib.flvis_write_imu_trajectory_run.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_char_p, C.c_double, C.c_int, C.c_double]
            n = self.lib.flvis_write_imu_trajectory_run(_P(r, C.c_double), len(r), path.encode(), C.c_double(min_dt), int(append),
                                                        C.c_double(t_first))
        else:
            n = self.lib.flvis_write_imu_trajectory(_P(r, C.c_double), len(r), path.encode(), C.c_double(min_dt), int(append))
        if n < 0:
            raise FlvisError("write_imu_trajectory failed (%d)" % n)
        return n

    def _presence(self, present, shape):
        """present (sequence of truth values, `shape`) as the uint8 array the _present entry points take, or None for None."""
        if present is None:
            return None
        pr = (self.np.asarray(present) != 0).astype(self.np.uint8)
        assert pr.shape == shape, "present must have shape %s" % (shape,)
        return self.np.ascontiguousarray(pr)

    def image_feed(self, img0, img1, times, want_out=True, with_local_map=True, present=None):
        """img0/img1: uint8 cuda tensors [S,H,W]; times: sequence of S floats.  present (optional, S truth values): only the streams
        marked present have a frame in this step (flvis_image_feed_present); None: all of them."""
        np = self.np
        assert img0.is_cuda and img0.is_contiguous() and img1.is_contiguous() and img0.shape[0] == self.S
        t = np.ascontiguousarray(times, np.float64)
        out = C.cast(self._out, C.c_void_p) if want_out else C.c_void_p(0)
        pr = self._presence(present, (self.S,))
        if pr is None:
            rc = self.lib.flvis_image_feed(self.ctx._h, _ptr(img0), _ptr(img1), _P(t, C.c_double), out, int(with_local_map))
        else:
            self.lib.flvis_image_feed_present.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            rc = self.lib.flvis_image_feed_present(self.ctx._h, _ptr(img0), _ptr(img1), _P(t, C.c_double), pr.ctypes.data, out,
                                                   int(with_local_map))
        self.ctx._check(rc, "image_feed")
        if not want_out:
            return None
        res = []
        for o in self._out:
            res.append(dict(state=o.state, new_keyframe=bool(o.new_keyframe), reset_cmd=bool(o.reset_cmd),
                            n_landmarks=o.n_landmarks, frame_id=o.frame_id, pose7=np.array(o.T_c_w[:]),
                            dbg=np.array([o.of_inliers, o.f_inliers, o.pnp_inliers]),
                            reprojection_error=o.reprojection_error))
        return res

    def run_steps(self, steps, with_local_map=True, present=None):
        """flvis_run_steps: a batch of frames whose images are already in HBM, one C call (what bench.py times).  steps: a sequence of
        (img0, img1, times[, imu_counts, imu_samples]) -- uint8 cuda tensors [S,H,W], S floats, and optionally the IMU samples of the
        step for all streams (int32 [S], float64 [S, n, 7]).  The tensors must stay alive until the context is synchronised.
        present (optional, [n_steps][S] truth values): the streams that have a frame in each step (flvis_run_steps_present)."""
        np = self.np

        class Step(C.Structure):
            _fields_ = [("d_img0", C.c_void_p), ("d_img1", C.c_void_p), ("h_times", C.c_void_p), ("h_imu_counts", C.c_void_p),
                        ("h_imu_samples", C.c_void_p), ("imu_samples_per_stream", C.c_int)]
        arr = (Step * len(steps))()
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
            self.lib.flvis_run_steps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
            rc = self.lib.flvis_run_steps(self.ctx._h, len(steps), C.cast(arr, C.c_void_p), int(with_local_map), C.c_void_p(0))
        else:
            self.lib.flvis_run_steps_present.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            rc = self.lib.flvis_run_steps_present(self.ctx._h, len(steps), C.cast(arr, C.c_void_p), pr.ctypes.data, int(with_local_map),
                                                  C.c_void_p(0))
        self.ctx._check(rc, "run_steps")

    def _frame_outs(self):
        np = self.np
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
        np = self.np
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
        out = C.cast(self._out, C.c_void_p) if want_out else C.c_void_p(0)
        pr = self._presence(present, (self.S,))
        if pr is None:
            self.lib.flvis_image_feed_host.argtypes = [C.c_void_p, C.POINTER(FlvisImage), C.POINTER(FlvisImage), C.c_void_p, C.c_int,
                                                       C.c_int]
            rc = self.lib.flvis_image_feed_host(self.ctx._h, a, b, out, int(with_local_map), int(hold_buffers))
        else:
            self.lib.flvis_image_feed_host_present.argtypes = [C.c_void_p, C.POINTER(FlvisImage), C.POINTER(FlvisImage), C.c_void_p,
                                                               C.c_void_p, C.c_int, C.c_int]
            rc = self.lib.flvis_image_feed_host_present(self.ctx._h, a, b, pr.ctypes.data, out, int(with_local_map), int(hold_buffers))
        self.ctx._check(rc, "image_feed_host")
        return self._frame_outs() if want_out else None

    def landmarks(self, stream, cap=2048):
        np = self.np
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
        np = self.np
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
        np = self.np
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
        self.ctx._check(self.lib.flvis_set_imu_factor(self.ctx._h, int(bool(enable)), C.c_double(sigma_gyro)), "set_imu_factor")

    def set_imu_factor_accel(self, sigma_acc):
        """flvis_set_imu_factor_accel: position rows of the IMU factor (accelerometer noise density; <= 0: rotation rows only)"""
        self.ctx._check(self.lib.flvis_set_imu_factor_accel(self.ctx._h, C.c_double(sigma_acc)), "set_imu_factor_accel")

    def get_keyframe_imu_pos(self, stream):
        """flvis_get_keyframe_imu_pos -> (dp, va): displacement preintegrated since the previous keyframe, that keyframe's velocity"""
        np = self.np
        dp, va = np.zeros(3), np.zeros(3)
        r = self.lib.flvis_get_keyframe_imu_pos(self.ctx._h, stream, _P(dp, C.c_double), _P(va, C.c_double))
        if r < 0:
            self.ctx._check(r, "get_keyframe_imu_pos")
        return dp, va

    def get_keyframe_imu(self, stream):
        """flvis_get_keyframe_imu -> (valid, dq (w, x, y, z), dt) of the stream's last keyframe"""
        np = self.np
        dq = np.zeros(4)
        dt = C.c_double(0)
        r = self.lib.flvis_get_keyframe_imu(self.ctx._h, stream, _P(dq, C.c_double), C.byref(dt))
        if r < 0:
            self.ctx._check(r, "get_keyframe_imu")
        return bool(r), dq, dt.value

    def ba_push_keyframe(self, stream, frame_id, pose7, lm_id, lm_2d, lm_3d, cap=8192, imu_dq=None, imu_dt=0.0, imu_dp=None, imu_va=None):
        np = self.np
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
            r = self.lib.flvis_ba_push_keyframe_imu_pos(self.ctx._h, stream, C.c_int64(frame_id), _P(p7, C.c_double), _P(dq, C.c_double),
                                                        C.c_double(imu_dt), _P(dp, C.c_double), _P(va, C.c_double), len(ids),
                                                        _P(ids, C.c_int64), _P(l2, C.c_double), _P(l3, C.c_double), cap, C.byref(fid),
                                                        _P(pose, C.c_double), C.byref(cnt), _P(oid_, C.c_int64), _P(o3, C.c_double),
                                                        C.byref(oc), _P(ooid, C.c_int64))
        elif imu_dq is not None:
            dq = np.ascontiguousarray(imu_dq, np.float64)
            r = self.lib.flvis_ba_push_keyframe_imu(self.ctx._h, stream, C.c_int64(frame_id), _P(p7, C.c_double), _P(dq, C.c_double),
                                                    C.c_double(imu_dt), len(ids), _P(ids, C.c_int64), _P(l2, C.c_double),
                                                    _P(l3, C.c_double), cap, C.byref(fid), _P(pose, C.c_double), C.byref(cnt),
                                                    _P(oid_, C.c_int64), _P(o3, C.c_double), C.byref(oc), _P(ooid, C.c_int64))
        else:
            r = self.lib.flvis_ba_push_keyframe(self.ctx._h, stream, C.c_int64(frame_id), _P(p7, C.c_double), len(ids),
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
        np = self.np
        rows = np.zeros((n, 9))
        r = self.lib.flvis_get_trajectory(self.ctx._h, stream, first, n, _P(rows, C.c_double))
        if r < 0:
            self.ctx._check(r, "get_trajectory")
        return rows

    def write_trajectory(self, stream, first, n, path, fmt=0, min_dt=0.0):
        """flvis_write_trajectory: fmt 0 = `stamp x y z qw qx qy qz`, 1 = KITTI 12 columns.  Returns lines written."""
        self.lib.flvis_write_trajectory.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double]
        r = self.lib.flvis_write_trajectory(self.ctx._h, stream, first, n, path.encode(), fmt, C.c_double(min_dt))
        if r < 0:
            self.ctx._check(r, "write_trajectory")
        return r

    def correction_feed(self, stream, frame_id, pose7, lm_id, lm_3d, outlier_id):
        """flvis_correction_feed: F2FTracking::correction_feed (opt-in local-map feedback)."""
        np = self.np
        pose7 = np.ascontiguousarray(pose7, np.float64)
        lm_id = np.ascontiguousarray(lm_id, np.int64)
        lm_3d = np.ascontiguousarray(lm_3d, np.float64).reshape(-1, 3)
        outlier_id = np.ascontiguousarray(outlier_id, np.int64)
        assert len(lm_id) == len(lm_3d)
        self.lib.flvis_correction_feed.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_double), C.c_int,
                                                   C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int64)]
        self.ctx._check(self.lib.flvis_correction_feed(self.ctx._h, stream, int(frame_id), _P(pose7, C.c_double), len(lm_id),
                                                       _P(lm_id, C.c_int64), _P(lm_3d, C.c_double), len(outlier_id),
                                                       _P(outlier_id, C.c_int64)), "correction_feed")

    def pose_records(self, stream, cap=1024):
        """flvis_get_pose_records -> rows (frame_id, pose7), oldest first."""
        rows = self.np.zeros((cap, 8))
        self.lib.flvis_get_pose_records.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
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
        fn = getattr(self.lib, what)
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self.ctx._check(fn(self.ctx._h, len(ids), arr), what[len("flvis_"):])

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
        fn = self.lib.flvis_reset_streams_rigs
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(FlvisCfg)]
        self.ctx._check(fn(self.ctx._h, len(ids), arr, carr), "reset_streams_rigs")

    def stream_cfg(self, s):
        """flvis_get_stream_cfg: the config stream s runs on (as created, or as last reset with reset_streams(..., cfgs))."""
        out = FlvisCfg()
        fn = self.lib.flvis_get_stream_cfg
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(FlvisCfg)]
        self.ctx._check(fn(self.ctx._h, int(s), C.byref(out)), "get_stream_cfg")
        return out

    def local_map_reset(self, streams):
        """flvis_local_map_reset: KFMSG_CMD_RESET_LM for the named streams' local maps (what is queued ahead is processed first)."""
        self._stream_list(streams, "flvis_local_map_reset")

    def local_map_cloud_enable(self, max_points):
        """flvis_local_map_cloud_enable: keep every optimisation's multi-view landmarks on the device, max_points per stream (<= 0: off)."""
        self.lib.flvis_local_map_cloud_enable.argtypes = [C.c_void_p, C.c_int64]
        self.ctx._check(self.lib.flvis_local_map_cloud_enable(self.ctx._h, int(max_points)), "local_map_cloud_enable")

    def local_map_cloud_clear(self, streams):
        """flvis_local_map_cloud_clear: empties the named streams' records."""
        self._stream_list(streams, "flvis_local_map_cloud_clear")

    def local_map_cloud_info(self, stream):
        """flvis_local_map_cloud_info -> dict(points, runs, dropped, capacity) of the stream's record."""
        v = (C.c_int64 * 4)()
        self.lib.flvis_local_map_cloud_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        self.ctx._check(self.lib.flvis_local_map_cloud_info(self.ctx._h, int(stream), v), "local_map_cloud_info")
        return dict(points=int(v[0]), runs=int(v[1]), dropped=int(v[2]), capacity=int(v[3]))

    def local_map_cloud(self, streams, mode="all", leaf=0.0, min_points=1, cap=None, host=False, ids=False):
        """flvis_local_map_cloud: the named streams' recorded map clouds.  mode "all": every recorded entry in record order (the
        reference's /map_cloud); "latest": one entry per landmark id, from the newest optimisation that lists it.  leaf = 0: every point
        rounded to float; leaf > 0: one point per voxel of `leaf` metres holding min_points points or more (flvis_hip_voxel_cloud's rule).
        cap: rows per stream (default: what the largest cloud yields, found by a call of its own).  host=True goes through the _host
        entry.  ids=True (leaf 0 only): the rows' landmark ids.
        -> (xyz [n] of float32 [k, 3], npts [n] of int32 [k], n_out int64 [n], n_dropped int64 [n]) and, with ids, ids [n] of int64 [k]."""
        import numpy as np
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
        args = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_double, C.c_int, C.c_int]
        head = (self.ctx._h, n, _P(arr, C.c_int), m, float(leaf), int(min_points), cap)
        if host:
            hx, hn, hi = np.zeros(shape + (3,), np.float32), np.zeros(shape, np.int32), np.zeros(shape, np.int64)
            fn = self.lib.flvis_local_map_cloud_host
            fn.argtypes = args + [C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            rc = fn(*head, _P(hx, C.c_float), _P(hn, C.c_int), _P(hi, C.c_int64) if ids else None, _P(n_out, C.c_int64), _P(n_drop, C.c_int64))
            self.ctx._check(rc, "local_map_cloud_host")
        else:
            dev = self.ctx.device
            xyz = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
            npts = torch.empty(shape, dtype=torch.int32, device=dev)
            did = torch.empty(shape, dtype=torch.int64, device=dev) if ids else None
            fn = self.lib.flvis_local_map_cloud
            fn.argtypes = args + [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            rc = fn(*head, _ptr(xyz), _ptr(npts), _ptr(did) if ids else None, _P(n_out, C.c_int64), _P(n_drop, C.c_int64))
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
        np = self.np
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
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(FlvisKeyframe), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                       C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        return self._keyframe_msg(lambda cap_, *a: fn(self.ctx._h, int(stream), cap_, *a), "get_keyframe_msg", cap, images)

    def keyframe_log_enable(self, max_keyframes):
        """flvis_keyframe_log_enable: keep every keyframe's whole message on the device, max_keyframes per stream (<= 0: off)."""
        self.lib.flvis_keyframe_log_enable.argtypes = [C.c_void_p, C.c_int]
        self.ctx._check(self.lib.flvis_keyframe_log_enable(self.ctx._h, int(max_keyframes)), "keyframe_log_enable")

    def keyframe_log_clear(self, streams):
        """flvis_keyframe_log_clear: empties the named streams' logs."""
        self._stream_list(streams, "flvis_keyframe_log_clear")

    def keyframe_log_info(self, stream):
        """flvis_keyframe_log_info -> dict(logged, dropped, capacity) of the stream's log."""
        v = (C.c_int64 * 3)()
        self.lib.flvis_keyframe_log_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        self.ctx._check(self.lib.flvis_keyframe_log_info(self.ctx._h, int(stream), v), "keyframe_log_info")
        return dict(logged=int(v[0]), dropped=int(v[1]), capacity=int(v[2]))

    def keyframe_log_get(self, stream, index, cap=2048, images=True):
        """flvis_keyframe_log_get: logged keyframe `index` of the stream, a dict like keyframe_msg's."""
        fn = self.lib.flvis_keyframe_log_get
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FlvisKeyframe), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                       C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        return self._keyframe_msg(lambda cap_, *a: fn(self.ctx._h, int(stream), int(index), cap_, *a), "keyframe_log_get", cap, images)

    def keyframe_log_images(self, stream, index):
        """flvis_keyframe_log_images: the entry's two images as torch views of the log's device memory ([h, w] uint8; img1 int16 storage
        on a depth rig).  Valid until the stream is cleared or reset, the log is enabled again or the tracker goes away."""
        import torch
        p0, p1 = C.c_void_p(0), C.c_void_p(0)
        fn = self.lib.flvis_keyframe_log_images
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        self.ctx._check(fn(self.ctx._h, int(stream), int(index), C.byref(p0), C.byref(p1)), "keyframe_log_images")
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
