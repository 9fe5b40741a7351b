"""Test helper: flvis_hip_lc_map_poses / flvis_loop_closer_map_poses (include/flvis_hip.h) restated in numpy, operation by operation.

Every function works on components -- Python floats, numpy float64 scalars or numpy float64 arrays alike -- and uses nothing but
+ - * / and sqrt in fp64, each a separate correctly rounded IEEE operation (numpy fuses nothing).  The order of the operations written
here IS the definition: the kernels (flvis_amd/csrc/lc_traj.hip, built with -ffp-contract=off) follow it, and the GPU tests compare bits.

pose7 = tx ty tz qx qy qz qw.  A pose is handled as a 7-tuple of components, a quaternion as (x, y, z, w), a vector as (x, y, z)."""
import numpy as np

ANCHOR, BLEND = 0, 1                    # FLVIS_LC_TRAJ_ANCHOR / _BLEND
POSE8, TRAJ9, IMU11 = 0, 1, 2           # FLVIS_LC_ROWS_*
WIDTH = {POSE8: 8, TRAJ9: 9, IMU11: 11}
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
EUROC_T0 = 1.403636579e9                # EuRoC's epoch: one ulp of a stamp is 2.4e-7 s


# ---- the products of loop_closer.hip:56-77 ---------------------------------------------------------------------------------------------
def q_mul(a, b):
    """Hamilton product, x y z w"""
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0]
    z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3]
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    return (x, y, z, w)


def q_rot(q, v):
    """R(q) v"""
    x, y, z, w = q
    tx, ty, tz = 2 * (y * v[2] - z * v[1]), 2 * (z * v[0] - x * v[2]), 2 * (x * v[1] - y * v[0])
    return (v[0] + w * tx + (y * tz - z * ty), v[1] + w * ty + (z * tx - x * tz), v[2] + w * tz + (x * ty - y * tx))


def pose_mul(a, b):
    """T_a * T_b, the quaternion renormalised"""
    t = q_rot(a[3:7], b[0:3])
    q = q_mul(a[3:7], b[3:7])
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return (t[0] + a[0], t[1] + a[1], t[2] + a[2], q[0] / n, q[1] / n, q[2] / n, q[3] / n)


def pose_inv(T):
    """(-(R(q*) t), q*), q* = (-x, -y, -z, w)"""
    qc = (-T[3], -T[4], -T[5], T[6])
    r = q_rot(qc, T[0:3])
    return (-r[0], -r[1], -r[2]) + qc


def _cols(A):
    """[n, k] array -> tuple of its k columns (each [n])"""
    A = np.asarray(A, np.float64)
    return tuple(A[..., j] for j in range(A.shape[-1]))


def _stack(cols, n):
    return np.stack([np.broadcast_to(np.asarray(c, np.float64), (n,)) for c in cols], axis=-1)


# ---- the drift table -------------------------------------------------------------------------------------------------------------------
def drift_table(O, M):
    """D_k = pose_mul(pose_inv(O_k), M_k); O, M [n, 7] -> [n, 7]"""
    O, M = np.asarray(O, np.float64).reshape(-1, 7), np.asarray(M, np.float64).reshape(-1, 7)
    if len(O) == 0:
        return np.zeros((0, 7))
    return _stack(pose_mul(pose_inv(_cols(O)), _cols(M)), len(O))


# ---- the anchor search -----------------------------------------------------------------------------------------------------------------
def anchors(tau, t):
    """-> (a int32 [m], before bool [m]): a = max{k : tau_k <= t}, 0 (and before) when t < tau_0, -1 for an empty sequence, -2 for a NaN
    stamp"""
    tau, t = np.asarray(tau, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    nan = np.isnan(t)
    if len(tau) == 0:
        return np.where(nan, -2, -1).astype(np.int32), np.zeros(len(t), bool)
    ub = np.searchsorted(tau, np.where(nan, tau[0], t), side="right")          # the number of k with tau_k <= t
    a = np.maximum(ub - 1, 0)
    return np.where(nan, -2, a).astype(np.int32), (ub == 0) & ~nan


def anchor_scalar(tau, t):
    """the same for one stamp, as a plain loop (the definition the vector form is checked against)"""
    if t != t:
        return -2, False
    if len(tau) == 0:
        return -1, False
    a = -1
    for k, x in enumerate(tau):
        if x <= t:
            a = k
    return max(a, 0), a < 0


# ---- the drift of every row: anchor or blend -------------------------------------------------------------------------------------------
def blend(Da, Db, u):
    """(1 - u) D_a (+) u D_b on components: the translation's chord, the quaternions' chord on the side of D_a, renormalised"""
    w0 = 1.0 - u
    tx, ty, tz = w0 * Da[0] + u * Db[0], w0 * Da[1] + u * Db[1], w0 * Da[2] + u * Db[2]
    dot = Da[3] * Db[3] + Da[4] * Db[4] + Da[5] * Db[5] + Da[6] * Db[6]
    us = u * np.where(dot < 0, -1.0, 1.0)
    qx, qy, qz, qw = w0 * Da[3] + us * Db[3], w0 * Da[4] + us * Db[4], w0 * Da[5] + us * Db[5], w0 * Da[6] + us * Db[6]
    n = np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
    return (tx, ty, tz, qx / n, qy / n, qz / n, qw / n)


def row_drifts(D, tau, t, mode, T_odom_map=IDENT):
    """-> (drift [m, 7] of every row, anchor int32 [m]); rows with a NaN stamp get the identity here (map_rows copies them)"""
    t = np.asarray(t, np.float64).reshape(-1)
    tau = np.asarray(tau, np.float64).reshape(-1)
    m, n = len(t), len(tau)
    a, before = anchors(tau, t)
    if n == 0:
        return np.broadcast_to(np.asarray(T_odom_map, np.float64), (m, 7)).copy(), a
    ai = np.maximum(a, 0)
    out = np.asarray(D, np.float64)[ai].copy()
    if mode == BLEND and n > 1:
        sel = (a >= 0) & ~before & (ai < n - 1)
        bi = np.minimum(ai + 1, n - 1)
        with np.errstate(all="ignore"):
            u = (np.where(sel, t, 0.0) - tau[ai]) / (tau[bi] - tau[ai])
            B = _stack(blend(_cols(D[ai]), _cols(D[bi]), u), m)
        out[sel] = B[sel]
    out[a == -2] = IDENT
    return out, a


# ---- the three row kinds ---------------------------------------------------------------------------------------------------------------
def map_rows(kind, rows, O, M, tau, mode, T_odom_map=IDENT):
    """rows [m, WIDTH[kind]] of one sequence -> (rows in the map frame, anchor int32 [m])"""
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, WIDTH[kind])
    m = len(rows)
    if m == 0:
        return rows.copy(), np.zeros(0, np.int32)
    Dr, a = row_drifts(drift_table(O, M), tau, rows[:, 0], mode, T_odom_map)
    D = _cols(Dr)
    out = rows.copy()
    if kind in (POSE8, TRAJ9):
        out[:, 1:8] = _stack(pose_mul(_cols(rows[:, 1:8]), D), m)
    else:
        E = pose_inv(D)
        qw, qx, qy, qz = _cols(rows[:, 1:5])
        P = pose_mul(E, _cols(rows[:, 5:8]) + (qx, qy, qz, qw))
        v = q_rot(E[3:7], _cols(rows[:, 8:11]))
        out[:, 1:5] = _stack((P[6], P[3], P[4], P[5]), m)
        out[:, 5:8] = _stack(P[0:3], m)
        out[:, 8:11] = _stack(v, m)
    nan = a == -2
    out[nan] = rows[nan]
    return out, a


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- generators ------------------------------------------------------------------------------------------------------------------------
def rand_quat(rng, n, angle=np.pi):
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th = rng.uniform(-angle, angle, size=(n, 1))
    return np.concatenate([ax * np.sin(th / 2), np.cos(th / 2)], axis=1)


def rand_poses(rng, n, scale=1.0, angle=np.pi):
    return np.concatenate([rng.uniform(-scale, scale, size=(n, 3)), rand_quat(rng, n, angle)], axis=1)


def stamps(rng, n, t0=0.0, dt=0.05):
    """n strictly increasing stamps from t0 on, irregular steps around dt"""
    return t0 + np.cumsum(rng.uniform(0.5 * dt, 1.5 * dt, size=n))


def sequence(rng, n_kf, scale=1.0, t0=0.0, drift_t=0.3, drift_r=0.05):
    """-> (O, M, tau) of a sequence after corrections: M_k = O_k * X_k, X_k a small drift that wanders from keyframe to keyframe, the way
    a pose graph spreads a correction over a chain"""
    O = rand_poses(rng, n_kf, scale)
    X = np.zeros((n_kf, 7))
    if n_kf:
        X[:, :3] = drift_t * np.cumsum(rng.normal(size=(n_kf, 3)), axis=0) / np.sqrt(n_kf)
        rv = drift_r * np.cumsum(rng.normal(size=(n_kf, 3)), axis=0) / np.sqrt(n_kf)
        X[:, 3:6], X[:, 6] = rv / 2, 1.0
        X[:, 3:] /= np.linalg.norm(X[:, 3:], axis=1, keepdims=True)
    M = _stack(pose_mul(_cols(O), _cols(X)), n_kf) if n_kf else np.zeros((0, 7))
    return O, M, stamps(rng, n_kf, t0)


def rows_of(rng, kind, t, scale=1.0):
    """rows of the kind with the stamps t and random poses (TRAJ9: a state | new_kf << 4 column; IMU11: velocities)"""
    t = np.asarray(t, np.float64).reshape(-1)
    m = len(t)
    P = rand_poses(rng, m, scale)
    if kind == POSE8:
        return np.concatenate([t[:, None], P], axis=1)
    if kind == TRAJ9:
        return np.concatenate([t[:, None], P, rng.integers(0, 32, size=(m, 1)).astype(np.float64)], axis=1)
    return np.concatenate([t[:, None], P[:, 6:7], P[:, 3:6], P[:, :3], rng.normal(size=(m, 3))], axis=1)


def row_stamps(rng, tau, m, t0=0.0, sort=True):
    """m stamps over the sequence's span and a little beyond both ends, some of them exactly a keyframe's"""
    if len(tau) == 0:
        t = t0 + rng.uniform(0, 1, size=m)
    else:
        span = max(tau[-1] - tau[0], 0.1)
        t = rng.uniform(tau[0] - 0.05 * span, tau[-1] + 0.05 * span, size=m)
        hit = rng.random(m) < 0.1
        t[hit] = rng.choice(tau, size=int(hit.sum()))
    return np.sort(t) if sort else t


def edge_stamps(tau):
    """every keyframe stamp itself (anchors k, and in blend mode u == 0) and the double just below it (anchors k - 1; below tau_0: before
    the first keyframe) -> (t [2 n], the anchors they must get)"""
    tau = np.asarray(tau, np.float64)
    n = len(tau)
    below = np.nextafter(tau, -np.inf)
    return np.concatenate([tau, below]), np.concatenate([np.arange(n), np.maximum(np.arange(n) - 1, 0)]).astype(np.int32)


def outside_stamps(tau):
    """one stamp a second before the first keyframe, one a second after the last -> anchors 0 and n - 1"""
    return np.array([tau[0] - 1.0, tau[-1] + 1.0]), np.array([0, len(tau) - 1], np.int32)


def flipped_pair(rng, n_kf=4, at=1):
    """a sequence in which the drifts of keyframes `at` and `at + 1` are the same rotation stored as q and -q: M_{at+1}'s quaternion negated"""
    O, M, tau = sequence(rng, n_kf)
    M[at + 1] = M[at]
    O[at + 1] = O[at]
    M[at + 1, 3:] = -M[at + 1, 3:]
    return O, M, tau
