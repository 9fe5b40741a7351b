"""GPU: flvis_hip_lc_map_poses (include/flvis_hip.h; the kernels: flvis_amd/csrc/lc_traj.hip) on caller arrays against the numpy
restatement tests/_lc_traj.py, BIT FOR BIT: the rule uses + - * / and sqrt in fp64 in a fixed order and the build contracts nothing, so
there is no tolerance to choose.  Sizes: keyframe counts from none over powers of two and their neighbours (the binary search's turning
points) to 1025; row counts around the 256-row tile and many tiles.  Translations are of 1e3 m throughout."""
import ctypes as C

import numpy as np
import pytest

import _lc_traj as T

pytestmark = pytest.mark.gpu

N_KF = (0, 1, 2, 63, 64, 65, 1025)
N_ROWS = (0, 1, 255, 256, 257, 5000)
KINDS = (T.POSE8, T.TRAJ9, T.IMU11)
SCALE = 1e3
INV = -1


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


class Tables:
    """sequences (O, M, tau) as the call takes them: [n_seq][stride] tables on the device, the stride a little above the longest sequence"""

    def __init__(self, seqs, drift=None, pad=3):
        import torch
        self.seqs = seqs
        self.nkf = [len(s[2]) for s in seqs]
        self.stride = max(self.nkf) + pad
        n = len(seqs)
        O, M, tau = np.zeros((n, self.stride, 7)), np.zeros((n, self.stride, 7)), np.full((n, self.stride), np.nan)
        O[:, :, 6] = M[:, :, 6] = 1.0
        for s, (o, m, t) in enumerate(seqs):
            O[s, :len(t)], M[s, :len(t)], tau[s, :len(t)] = o, m, t
        self.O, self.M, self.tau = (torch.from_numpy(a).cuda() for a in (O, M, tau))
        self.drift = np.tile(T.IDENT, (n, 1)) if drift is None else np.asarray(drift, np.float64)

    def run(self, ctx, jobs, mode):
        return ctx.lc_map_poses(self.O, self.M, self.tau, self.nkf, jobs, mode, self.drift)

    def want(self, seq, kind, rows, mode):
        o, m, t = self.seqs[seq]
        return T.map_rows(kind, rows, o, m, t, mode, self.drift[seq])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(got, want, what):
    out, anc = got
    w_out, w_anc = want
    assert T.same_bits(out.cpu().numpy(), w_out), (what, "rows", int((T.bits(out.cpu().numpy()) != T.bits(w_out)).any(axis=1).sum()))
    if anc is not None:
        assert np.array_equal(anc.cpu().numpy(), w_anc), (what, "anchors")


@pytest.fixture(scope="module")
def fleet():
    """one sequence per keyframe count, one drift per sequence (read for the empty one), and per (sequence, kind, row count) sorted rows"""
    rng = np.random.default_rng(2024)
    seqs = [T.sequence(rng, n, scale=SCALE, t0=T.EUROC_T0 if n % 2 else 0.0) for n in N_KF]
    tab = Tables(seqs, drift=T.rand_poses(rng, len(N_KF), 5.0, 0.3))
    rows = {}
    for s, (_, _, tau) in enumerate(seqs):
        t0 = T.EUROC_T0 if N_KF[s] % 2 else 0.0
        for kind in KINDS:
            for m in N_ROWS:
                rows[s, kind, m] = T.rows_of(rng, kind, T.row_stamps(rng, tau, m, t0), SCALE)
    return tab, rows


@pytest.mark.parametrize("mode", [T.ANCHOR, T.BLEND])
@pytest.mark.parametrize("s", range(len(N_KF)), ids=["kf%d" % n for n in N_KF])
def test_counts_kinds_and_modes(ctx, fleet, s, mode):
    """every row count and kind as jobs of ONE call on one sequence; then the same rows shuffled: row by row the sorted rows' results"""
    tab, rows = fleet
    rng = np.random.default_rng(s)
    keys = [(kind, m) for kind in KINDS for m in N_ROWS]
    got = tab.run(ctx, [dict(seq=s, kind=kind, rows=dev(rows[s, kind, m])) for kind, m in keys], mode)
    want = {}
    for (kind, m), g in zip(keys, got):
        want[kind, m] = tab.want(s, kind, rows[s, kind, m], mode)
        check(g, want[kind, m], (N_KF[s], kind, m))
    if N_KF[s] > 1:
        a = want[T.TRAJ9, 5000][1]
        assert a.min() == 0 and a.max() == N_KF[s] - 1 and len(np.unique(a)) > min(N_KF[s], 5000) // 2     # the rows do visit the sequence
    perm = {k: rng.permutation(k[1]) for k in keys}
    shuffled = tab.run(ctx, [dict(seq=s, kind=kind, rows=dev(rows[s, kind, m][perm[kind, m]])) for kind, m in keys], mode)
    for k, g in zip(keys, shuffled):
        check(g, (want[k][0][perm[k]], want[k][1][perm[k]]), (N_KF[s], k, "shuffled"))


@pytest.mark.parametrize("mode", [T.ANCHOR, T.BLEND])
def test_one_call_over_all_sequences_in_place_and_without_anchors(ctx, fleet, mode):
    tab, rows = fleet
    jobs, want, src = [], [], []
    for s in range(len(N_KF)):
        for i, (kind, m) in enumerate(((T.TRAJ9, 257), (T.IMU11, 5000), (T.POSE8, 255), (T.TRAJ9, 0))):
            r = dev(rows[s, kind, m])
            jobs.append(dict(seq=s, kind=kind, rows=r, out="inplace" if (s + i) % 2 else None, anchor=(s + i) % 3 != 0))
            want.append(tab.want(s, kind, rows[s, kind, m], mode))
            src.append((r, rows[s, kind, m]))
    got = tab.run(ctx, jobs, mode)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g[1] is None) == (not jobs[k]["anchor"])
        check(g, w, ("job", k))
        if jobs[k]["out"] == "inplace":
            assert g[0].data_ptr() == src[k][0].data_ptr()
        else:
            assert T.same_bits(src[k][0].cpu().numpy(), src[k][1])            # the input rows are left as they were


@pytest.mark.parametrize("n_kf", [9, 300])
def test_edges(ctx, n_kf):
    """the generators of tests/_lc_traj.py (test_lc_traj_inputs.py shows that each reaches its edge): every keyframe's own stamp and the
    double below it at EuRoC's epoch, rows before and after the sequence, u == 0, NaN stamps, q / -q neighbours; in order and shuffled"""
    rng = np.random.default_rng(n_kf)
    O, M, tau = T.sequence(rng, n_kf, scale=SCALE, t0=T.EUROC_T0)
    fO, fM, ftau = T.flipped_pair(rng, 4, 1)
    tab = Tables([(O, M, tau), (fO, fM, ftau), (O[:1], M[:1], tau[:1])])
    te, want_a = T.edge_stamps(tau)
    to, want_o = T.outside_stamps(tau)
    t = np.concatenate([te, to, [np.nan, np.nan]])
    anchors = np.concatenate([want_a, want_o, [-2, -2]])
    order = np.argsort(np.where(np.isnan(t), np.inf, t), kind="stable")
    tf = np.concatenate([ftau[1] + np.linspace(0, 1, 33) * (ftau[2] - ftau[1]), [np.nan]])
    t1 = np.array([tau[0] - 1, tau[0], tau[0] + 1, np.nan])
    for mode in (T.ANCHOR, T.BLEND):
        for kind in KINDS:
            for idx in (order, rng.permutation(len(t))):
                rows = T.rows_of(rng, kind, t[idx], SCALE)
                rf, r1 = T.rows_of(rng, kind, tf, SCALE), T.rows_of(rng, kind, t1, SCALE)
                got = tab.run(ctx, [dict(seq=0, kind=kind, rows=dev(rows)), dict(seq=1, kind=kind, rows=dev(rf)),
                                    dict(seq=2, kind=kind, rows=dev(r1))], mode)
                assert np.array_equal(got[0][1].cpu().numpy(), anchors[idx])
                assert got[2][1].cpu().numpy().tolist() == [0, 0, 0, -2]
                nan = np.isnan(t[idx])
                assert T.same_bits(got[0][0].cpu().numpy()[nan], rows[nan])                   # copied unchanged
                check(got[0], tab.want(0, kind, rows, mode), (kind, mode, "edges"))
                check(got[1], tab.want(1, kind, rf, mode), (kind, mode, "flipped"))
                check(got[2], tab.want(2, kind, r1, mode), (kind, mode, "one keyframe"))
                assert np.isfinite(got[1][0].cpu().numpy()[:-1]).all()


def _job(seq, kind, n, d_in, d_out, d_anchor=None):
    import flvis_amd
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    return flvis_amd.FlvisLcTrajJob(seq, kind, n, p(d_in), p(d_out), p(d_anchor))


def test_bad_arguments_leave_the_context_usable(ctx):
    import flvis_amd
    import torch
    rng = np.random.default_rng(1)
    seqs = [T.sequence(rng, 5, scale=SCALE), T.sequence(rng, 0)]
    tab = Tables(seqs)
    rows = T.rows_of(rng, T.TRAJ9, T.row_stamps(rng, seqs[0][2], 300), SCALE)
    r = dev(rows)
    SENT = 12345.5
    out = torch.full_like(r, SENT)
    lib = ctx._lib
    fn = lib.flvis_hip_lc_map_poses
    nkf = np.array(tab.nkf, np.int32)
    drift = np.ascontiguousarray(tab.drift)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731

    def call(n_seq=2, stride=tab.stride, h_nkf=nkf, O=tab.O, M=tab.M, tau=tab.tau, h_drift=drift, n_jobs=1, job=None, mode=0, no_jobs=False):
        arr = (flvis_amd.FlvisLcTrajJob * 1)(job if job is not None else _job(0, T.TRAJ9, 300, r, out))
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return fn(ctx._h, n_seq, stride, P(h_nkf, C.c_int) if h_nkf is not None else None, p(O), p(M), p(tau),
                  P(h_drift, C.c_double) if h_drift is not None else None, n_jobs, None if no_jobs else arr, mode)

    bad_tau = tab.tau.clone()
    bad_tau[0, 3] = bad_tau[0, 2]                                     # not increasing
    nan_tau = tab.tau.clone()
    nan_tau[0, 4] = float("nan")
    inf_tau = tab.tau.clone()
    inf_tau[0, 4] = float("inf")
    cases = dict(
        mode_high=dict(mode=2), mode_negative=dict(mode=-1),
        kind_high=dict(job=_job(0, 3, 300, r, out)), kind_negative=dict(job=_job(0, -1, 300, r, out)),
        rows_negative=dict(job=_job(0, T.TRAJ9, -1, r, out)), jobs_negative=dict(n_jobs=-1), no_sequences=dict(n_seq=0),
        stride_negative=dict(stride=-1), count_above_stride=dict(stride=4), count_negative=dict(h_nkf=np.array([-1, 0], np.int32)),
        seq_high=dict(job=_job(2, T.TRAJ9, 300, r, out)), seq_negative=dict(job=_job(-1, T.TRAJ9, 300, r, out)),
        null_in=dict(job=_job(0, T.TRAJ9, 300, None, out)), null_out=dict(job=_job(0, T.TRAJ9, 300, r, None)),
        null_counts=dict(h_nkf=None), null_jobs=dict(no_jobs=True), null_odom=dict(O=None), null_map=dict(M=None), null_stamps=dict(tau=None),
        null_drift_for_an_empty_sequence=dict(h_drift=None, job=_job(1, T.TRAJ9, 300, r, out)),
        stamps_not_increasing=dict(tau=bad_tau), stamp_nan=dict(tau=nan_tau), stamp_infinite=dict(tau=inf_tau))
    for name, kw in cases.items():
        assert call(**kw) == INV, name
        assert lib.flvis_last_error(ctx._h), name
        assert bool((out == SENT).all()), (name, "rows were written")
    assert fn(None, 2, tab.stride, P(nkf, C.c_int), None, None, None, None, 0, None, 0) == INV           # no context
    # what is allowed: no jobs at all, a job without rows (its pointers are not looked at), NULL drifts when no empty sequence is named
    assert call(n_jobs=0, no_jobs=True) == 0 and call(job=_job(0, T.TRAJ9, 0, None, None)) == 0
    assert bool((out == SENT).all())
    assert call(h_drift=None) == 0
    assert T.same_bits(out.cpu().numpy(), tab.want(0, T.TRAJ9, rows, T.ANCHOR)[0])
    got = tab.run(ctx, [dict(seq=0, kind=T.TRAJ9, rows=r), dict(seq=1, kind=T.TRAJ9, rows=r)], T.BLEND)
    check(got[0], tab.want(0, T.TRAJ9, rows, T.BLEND), "after the refusals")
    check(got[1], tab.want(1, T.TRAJ9, rows, T.BLEND), "after the refusals, the empty sequence")
