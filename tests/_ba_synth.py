"""Synthetic sliding-window BA problems (pattern of g2o examples/ba/ba_demo.cpp: points, cameras, pixel noise, outliers)."""
import numpy as np

import _geom as G

K4 = np.array([384.16455078125, 384.16455078125, 320.2144470214844, 238.94403076171875])


COVIS = ("dense", "sparse", "mixed")
KF_MAXLM = 1024  # landmarks per keyframe payload (pipeline.hpp)


def _gt_pose(k):
    tc = np.array([0.12 * k, 0.03 * np.sin(0.7 * k), 0.02 * k])          # camera centre in world
    R = G.rodrigues(np.array([0.01 * np.sin(k), 0.02 * k - 0.1, 0.005 * k]))  # R_c_w
    return R, -R @ tc


def covis_indices(covis, lm_per_kf):
    """Landmark indices (into the pool) each keyframe observes, in payload order.
    dense:  every keyframe sees landmarks [0, m_k) -- with a constant m, every landmark is seen by every keyframe;
    sparse: keyframe k sees a run of m_k landmarks that starts ceil(2 m_{k-1} / 3) after the previous keyframe's run: every landmark is seen
            by one or two consecutive keyframes (as long as m_{k+1} >= m_k / 2);
    mixed:  the first m_k // 2 of keyframe k's landmarks from a dense core [0, max m // 2), the rest a sparse run behind the core."""
    ms = [int(m) for m in lm_per_kf]
    if covis not in COVIS:
        raise ValueError("covis: one of %s" % (COVIS,))
    if min(ms) < 1 or max(ms) > KF_MAXLM:
        raise ValueError("landmarks per keyframe must be 1 .. %d" % KF_MAXLM)
    if covis == "dense":
        return [np.arange(m) for m in ms]
    core = max(ms) // 2 if covis == "mixed" else 0
    runs = [m - (m // 2 if covis == "mixed" else 0) for m in ms]
    out, o = [], core
    for k, (m, r) in enumerate(zip(ms, runs)):
        if k > 0:
            o += -(-2 * runs[k - 1] // 3)
        head = np.arange(m // 2) if covis == "mixed" else np.arange(0)
        out.append(np.concatenate([head, o + np.arange(r)]))
    return out


def make_sequence(seed, n_kf=14, n_lm=300, pix_sigma=0.5, outlier_frac=0.05, lm_sigma=0.05, pose_sigma=(0.02, 0.0087),
                  lm_per_kf=None, covis=None, outlier_kfs=()):
    """Returns ground truth and the noisy keyframe stream a tracker would publish (KeyFrame.msg payloads).

    covis None (default): n_lm random points, each keyframe sees the visible ones with probability 0.8 (this path's output is fixed:
    existing tests depend on it).  covis "dense" / "sparse" / "mixed" (covis_indices): the co-visibility pattern is set instead, with
    lm_per_kf landmarks per keyframe (an int, or one per keyframe; up to KF_MAXLM); n_lm is then unused, every keyframe carries an "idx"
    entry (its landmarks' pool indices), and the keyframes in outlier_kfs see nothing but gross outliers."""
    if covis is not None:
        return _make_structured(seed, n_kf, pix_sigma, outlier_frac, lm_sigma, pose_sigma, lm_per_kf, covis, outlier_kfs)
    if lm_per_kf is not None or len(outlier_kfs):
        raise ValueError("lm_per_kf / outlier_kfs need a co-visibility pattern (covis)")
    rng = np.random.default_rng(seed)
    Pw = np.stack([rng.uniform(-3, 3, n_lm), rng.uniform(-2, 2, n_lm), rng.uniform(2, 6, n_lm)], 1)
    kfs = []
    gt = []
    for k in range(n_kf):
        R, t = _gt_pose(k)
        gt.append((R, t))
        uv = G.project(R, t, Pw, K4)
        Xc = Pw @ R.T + t
        vis = (uv[:, 0] > 5) & (uv[:, 0] < 635) & (uv[:, 1] > 5) & (uv[:, 1] < 475) & (Xc[:, 2] > 0.5)
        vis &= rng.random(n_lm) < 0.8
        idx = np.nonzero(vis)[0]
        z = uv[idx] + rng.normal(0, pix_sigma, (len(idx), 2))
        out = rng.random(len(idx)) < outlier_frac
        z[out] = np.stack([rng.uniform(0, 640, out.sum()), rng.uniform(0, 480, out.sum())], 1)
        lm3 = Pw[idx] + rng.normal(0, lm_sigma, (len(idx), 3))
        Rn = G.rodrigues(rng.normal(0, pose_sigma[1], 3)) @ R
        tn = t + rng.normal(0, pose_sigma[0], 3)
        kfs.append(dict(frame_id=10 + 3 * k, pose7=G.pose7(Rn, tn), lm_id=(idx + 100).astype(np.int64), lm_2d=z,
                        lm_3d=lm3, outlier=out))
    return dict(Pw=Pw, gt=gt, kfs=kfs)


def _make_structured(seed, n_kf, pix_sigma, outlier_frac, lm_sigma, pose_sigma, lm_per_kf, covis, outlier_kfs):
    rng = np.random.default_rng(seed)
    ms = [int(lm_per_kf)] * n_kf if np.isscalar(lm_per_kf) else [int(m) for m in lm_per_kf]
    if len(ms) != n_kf:
        raise ValueError("lm_per_kf: %d entries for %d keyframes" % (len(ms), n_kf))
    idxs = covis_indices(covis, ms)
    n_pool = int(max(i.max() for i in idxs)) + 1
    Pw = np.stack([rng.uniform(-3, 3, n_pool), rng.uniform(-2, 2, n_pool), rng.uniform(2, 6, n_pool)], 1)
    kfs, gt = [], []
    for k, idx in enumerate(idxs):
        R, t = _gt_pose(k)
        gt.append((R, t))
        z = G.project(R, t, Pw[idx], K4) + rng.normal(0, pix_sigma, (len(idx), 2))
        out = np.ones(len(idx), bool) if k in outlier_kfs else rng.random(len(idx)) < outlier_frac
        z[out] = np.stack([rng.uniform(0, 640, out.sum()), rng.uniform(0, 480, out.sum())], 1)
        lm3 = Pw[idx] + rng.normal(0, lm_sigma, (len(idx), 3))
        Rn = G.rodrigues(rng.normal(0, pose_sigma[1], 3)) @ R
        tn = t + rng.normal(0, pose_sigma[0], 3)
        kfs.append(dict(frame_id=10 + 3 * k, pose7=G.pose7(Rn, tn), lm_id=(idx + 100).astype(np.int64), lm_2d=z, lm_3d=lm3, outlier=out,
                        idx=idx))
    return dict(Pw=Pw, gt=gt, kfs=kfs)


def window_size_of(kfs, first, window):
    """(landmarks, observations) of the window kfs[first : first + window] before any cull"""
    ids = np.concatenate([kf["lm_id"] for kf in kfs[first:first + window]])
    return len(np.unique(ids)), len(ids)


def local_map_size(kfs, window, k):
    """(landmarks in the bag, edges) of the local map once keyframe k (>= window - 1) is added, nothing culled, as the reference's
    bookkeeping keeps them (vo_localmap.cpp:114-284): the edges are those of the window's poses, the keyframes window - 1 ... k back; the
    bag's landmarks lose, at every sliding step, the observations of the keyframe at the front of the keyframe queue.  That is the
    SECOND oldest pose's keyframe (the queue is popped after each optimisation, quirk A22): keyframe 0's observations never leave the bag."""
    from collections import Counter
    cnt = Counter(int(i) for kf in kfs[:window] for i in kf["lm_id"])
    for j in range(window, k + 1):
        cnt.subtract(int(i) for i in kfs[j - window + 1]["lm_id"])
        cnt = Counter({i: c for i, c in cnt.items() if c > 0})
        cnt.update(int(i) for i in kfs[j]["lm_id"])
    return len(cnt), sum(len(kf["lm_id"]) for kf in kfs[k - window + 1:k + 1])


def huber_cost(pose7, lm_id, lm_3d, kf, K4, skip_ids=()):
    """fp64 cost of keyframe kf's observations of the landmarks (lm_id, lm_3d) at the camera pose7 (T_c_w): sum of Huber(|r|^2),
    delta 1, identity information (g2o's EdgeSE3ProjectXYZ + RobustKernelHuber, as oracle/ref_ba.cpp evaluates it); observations of
    landmarks in skip_ids (the culled edges) and of landmarks not in lm_id are left out.  Returns (cost, observations counted)."""
    R, t = G.pose7_to_Rt(np.asarray(pose7, np.float64))
    pos = {int(i): k for k, i in enumerate(lm_id)}
    skip = set(int(i) for i in skip_ids)
    rows = [(pos[int(i)], j) for j, i in enumerate(kf["lm_id"]) if int(i) in pos and int(i) not in skip]
    if not rows:
        return 0.0, 0
    li, oj = np.array(rows).T
    r = G.project(R, t, np.asarray(lm_3d, np.float64)[li], K4) - np.asarray(kf["lm_2d"], np.float64)[oj]
    e2 = (r * r).sum(1)
    return float(np.where(e2 <= 1.0, e2, 2.0 * np.sqrt(e2) - 1.0).sum()), len(rows)
