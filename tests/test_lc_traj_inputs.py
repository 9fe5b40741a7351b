"""CPU: the restatement of the trajectory mapping (tests/_lc_traj.py) against an independent write-up in 4x4 homogeneous matrices, its
edge-case generators (each must reach the edge it is for), and the properties that make the rule the right one.

TOL = 1e-12 * (1 + max|t|): a mapped row is three pose products (the inverse, the drift, the row), each a few dozen roundings of
1.1e-16 relative to the magnitudes involved, so the two write-ups stay within 1e-14 * (1 + max|t|) of each other; the bound leaves a
factor of 100."""
import numpy as np
import pytest

import _lc_traj as T


def tol(*arrays):
    return 1e-12 * (1 + max(float(np.abs(np.asarray(a)[..., :3]).max()) if np.asarray(a).size else 0.0 for a in arrays))


# ---- the independent write-up: rotation matrices, 4x4 products, linear algebra's inverse -------------------------------------------------
def mat_of(p):
    x, y, z, w = p[3:7] / np.linalg.norm(p[3:7])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = R, p[:3]
    return A


def same_pose(p, A, eps):
    """pose7 p against the 4x4 matrix A"""
    B = mat_of(np.asarray(p, np.float64))
    return np.abs(B[:3, 3] - A[:3, 3]).max() < eps and np.abs(B[:3, :3] - A[:3, :3]).max() < 1e-12


def mat_drift(O, M, tau, t, mode, T_odom_map):
    """the drift of a row with stamp t as a matrix (blend: the restatement's own chord -- its definition -- on matrix-made drifts)"""
    n = len(tau)
    if n == 0:
        return mat_of(T_odom_map)
    Dm = [np.linalg.inv(mat_of(O[k])) @ mat_of(M[k]) for k in range(n)]
    a = max([k for k in range(n) if tau[k] <= t] + [-1])
    if a < 0 or a == n - 1 or mode == T.ANCHOR:
        return Dm[max(a, 0)]
    u = (t - tau[a]) / (tau[a + 1] - tau[a])
    D = T.drift_table(O, M)
    qa, qb = D[a, 3:], D[a + 1, 3:]
    q = (1 - u) * qa + u * (-1.0 if qa @ qb < 0 else 1.0) * qb
    out = mat_of(np.concatenate([np.zeros(3), q]))
    out[:3, 3] = (1 - u) * Dm[a][:3, 3] + u * Dm[a + 1][:3, 3]
    return out


def test_restatement_against_homogeneous_matrices():
    rng = np.random.default_rng(7)
    for case in range(200):
        kind, mode = case % 3, (case // 3) % 2
        n_kf = int(rng.integers(0, 6))
        scale = [1.0, 30.0, 1e3][case % 3]
        O, M, tau = T.sequence(rng, n_kf, scale=scale)
        X = T.rand_poses(rng, 1, 2.0, 0.5)[0]
        t = T.row_stamps(rng, tau, 3, sort=False)
        rows = T.rows_of(rng, kind, t, scale)
        out, anchor = T.map_rows(kind, rows, O, M, tau, mode, X)
        eps = tol(O, M, rows[:, 1:8] if kind != T.IMU11 else rows[:, 5:8])
        for r in range(len(rows)):
            D = mat_drift(O, M, tau, t[r], mode, X)
            assert anchor[r] == T.anchor_scalar(tau, t[r])[0]
            if kind == T.IMU11:
                E = np.linalg.inv(D)
                want = E @ mat_of(np.concatenate([rows[r, 5:8], rows[r, 2:5], rows[r, 1:2]]))
                got = np.concatenate([out[r, 5:8], out[r, 2:5], out[r, 1:2]])
                assert same_pose(got, want, eps), (case, r)
                assert np.abs(out[r, 8:11] - E[:3, :3] @ rows[r, 8:11]).max() < 1e-12 * (1 + np.abs(rows[r, 8:11]).max())
            else:
                assert same_pose(out[r, 1:8], mat_of(rows[r, 1:8]) @ D, eps), (case, r)
                assert out[r, 0] == rows[r, 0] and (kind == T.POSE8 or out[r, 8] == rows[r, 8])


def test_vector_form_is_the_scalar_form_bit_for_bit():
    """the restatement on arrays (what the GPU tests compare against) and on one row at a time with Python floats give the same bits"""
    rng = np.random.default_rng(11)
    O, M, tau = T.sequence(rng, 7, scale=1e3, t0=T.EUROC_T0)
    for kind in (T.POSE8, T.TRAJ9, T.IMU11):
        rows = T.rows_of(rng, kind, T.row_stamps(rng, tau, 40, sort=False), 1e3)
        for mode in (T.ANCHOR, T.BLEND):
            out, anchor = T.map_rows(kind, rows, O, M, tau, mode)
            for r in range(len(rows)):
                o1, a1 = T.map_rows(kind, rows[r:r + 1], O, M, tau, mode)
                assert T.same_bits(o1[0], out[r]) and a1[0] == anchor[r] == T.anchor_scalar(tau, rows[r, 0])[0]
    a = tuple(float(x) for x in O[0])
    b = tuple(float(x) for x in M[1])
    assert T.same_bits(np.array(T.pose_mul(T.pose_inv(a), b)), T.drift_table(O[:1], M[1:2])[0])


# ---- the generators reach their edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0.0, T.EUROC_T0])
def test_stamp_edges(t0):
    rng = np.random.default_rng(3)
    tau = T.stamps(rng, 9, t0)
    if t0:
        assert np.spacing(tau[0]) > 2e-7 and np.all(np.diff(tau) > 0)      # EuRoC's epoch: one ulp is 2.4e-7 s
    t, want = T.edge_stamps(tau)
    a, before = T.anchors(tau, t)
    assert np.array_equal(a, want)
    assert np.array_equal(a[:9], np.arange(9)) and np.array_equal(a[9:], np.maximum(np.arange(9) - 1, 0))
    assert before.tolist() == [False] * 9 + [True] + [False] * 8           # only the double below tau_0 lies before the sequence
    assert all(T.anchor_scalar(tau, x) == (int(k), bool(b)) for x, k, b in zip(t, a, before))
    t2, want2 = T.outside_stamps(tau)
    a2, before2 = T.anchors(tau, t2)
    assert a2.tolist() == want2.tolist() == [0, 8] and before2.tolist() == [True, False]
    # u == 0 at a keyframe's own stamp, and the blend is then that keyframe's drift up to the renormalisation
    O, M, _ = T.sequence(rng, 9)
    D = T.drift_table(O, M)
    Dr, _ = T.row_drifts(D, tau, tau[:8], T.BLEND)
    assert np.abs(Dr - D[:8]).max() < 1e-15


def test_single_keyframe_empty_sequence_and_nan_rows():
    rng = np.random.default_rng(5)
    O, M, tau = T.sequence(rng, 1)
    t = np.array([tau[0] - 1, tau[0], tau[0] + 1, np.nan])
    for mode in (T.ANCHOR, T.BLEND):
        for kind in (T.POSE8, T.TRAJ9, T.IMU11):
            rows = T.rows_of(rng, kind, t)
            out, a = T.map_rows(kind, rows, O, M, tau, mode)
            assert a.tolist() == [0, 0, 0, -2]
            assert T.same_bits(out[3, 1:], rows[3, 1:]) and np.isnan(out[3, 0])
            if kind != T.IMU11:
                D0 = tuple(T.drift_table(O, M)[0])
                assert all(T.same_bits(out[r, 1:8], np.array(T.pose_mul(tuple(rows[r, 1:8]), D0))) for r in range(3))
            # an empty sequence: the sequence's T_odom_map for every row, anchor -1 (NaN: still -2)
            X = T.rand_poses(rng, 1)[0]
            out0, a0 = T.map_rows(kind, rows, np.zeros((0, 7)), np.zeros((0, 7)), np.zeros(0), mode, X)
            assert a0.tolist() == [-1, -1, -1, -2] and T.same_bits(out0[3, 1:], rows[3, 1:])
            if kind != T.IMU11:
                assert all(T.same_bits(out0[r, 1:8], np.array(T.pose_mul(tuple(rows[r, 1:8]), tuple(X)))) for r in range(3))


def test_flipped_neighbours_blend_on_the_short_side():
    rng = np.random.default_rng(9)
    O, M, tau = T.flipped_pair(rng, 4, 1)
    D = T.drift_table(O, M)
    dot = float(D[1, 3:] @ D[2, 3:])
    assert dot < -0.999999 and T.same_bits(D[2, 3:], -D[1, 3:]) and T.same_bits(D[2, :3], D[1, :3])       # q and -q: sigma must be -1
    t = tau[1] + np.linspace(0, 1, 9)[:-1] * (tau[2] - tau[1])
    Dr, a = T.row_drifts(D, tau, t, T.BLEND)
    assert np.all(a == 1)
    assert np.abs(Dr - D[1]).max() < 1e-15                 # the same rotation all the way; sigma = +1 would pass through zero at u = 0.5
    u = (t[4] - tau[1]) / (tau[2] - tau[1])
    assert abs(u - 0.5) < 1e-9 and np.linalg.norm((1 - u) * D[1, 3:] + u * D[2, 3:]) < 1e-8


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def test_a_sequence_that_never_closed_a_loop_maps_to_itself():
    rng = np.random.default_rng(13)
    O = T.rand_poses(rng, 12, 50.0)
    M = T._stack(T.pose_mul(T._cols(O), tuple(T.IDENT)), 12)         # what add_keyframes stores with T_odom_map = identity
    tau = T.stamps(rng, 12)
    D = T.drift_table(O, M)
    eps = tol(O)
    assert np.abs(D - T.IDENT).max() < eps
    for kind in (T.POSE8, T.TRAJ9, T.IMU11):
        rows = T.rows_of(rng, kind, T.row_stamps(rng, tau, 50), 50.0)
        for mode in (T.ANCHOR, T.BLEND):
            out, _ = T.map_rows(kind, rows, O, M, tau, mode)
            assert np.abs(out - rows).max() < eps


def test_after_set_drift_every_later_keyframe_carries_it():
    rng = np.random.default_rng(17)
    X = T.rand_poses(rng, 1, 3.0, 0.4)[0]
    O = T.rand_poses(rng, 8, 20.0)
    M = T._stack(T.pose_mul(T._cols(O), tuple(X)), 8)                # set_drift(X) on the empty sequence, then eight keyframes
    D = T.drift_table(O, M)
    eps = tol(O, M)
    for k in range(8):
        assert same_pose(D[k], mat_of(X), eps)


def test_rows_behind_the_newest_keyframe_follow_the_tf_rule():
    """anchor mode, t >= tau_{n-1}: row * T_odom_map with T_odom_map the drift the newest keyframe was stored with (vo_loopclosing.cpp:908)"""
    rng = np.random.default_rng(19)
    O, M, tau = T.sequence(rng, 6, scale=20.0)
    X = T.rand_poses(rng, 1, 3.0, 0.4)[0]
    M[5] = np.array(T.pose_mul(tuple(O[5]), tuple(X)))               # T_c_w = T_c_w_odom * T_odom_map (:374-383)
    t = tau[5] + np.array([0.0, 0.01, 5.0])
    rows = T.rows_of(rng, T.TRAJ9, t, 20.0)
    eps = tol(O, M, rows[:, 1:8])
    for mode in (T.ANCHOR, T.BLEND):
        out, a = T.map_rows(T.TRAJ9, rows, O, M, tau, mode)
        assert a.tolist() == [5, 5, 5]
        for r in range(3):
            assert same_pose(out[r, 1:8], mat_of(rows[r, 1:8]) @ mat_of(X), eps)
