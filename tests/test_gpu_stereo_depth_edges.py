"""GPU (-m gpu, MI355X): flvis_hip_stereo_depth (k_sd_seeds, the batched LK matcher, k_sd_post) at its batch, count, range and seed edges,
bit for bit against the CPU oracle (O.Tracker.stereo_depth).  The inputs and what the oracle says about them come from
tests/_sd_edges.py, whose recipes check themselves (tests/test_sd_edges_inputs.py runs them without a GPU).

There is no tolerance anywhere: masks equal as bytes, points equal as uint64 (NaN and signed zeros by their bits), every slot at or behind
min(count, cap) still holds the sentinel the caller put there, and the generator state word for word where the one it must equal can be
produced."""
import copy

import numpy as np
import pytest

import _sd_edges as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


_CFG = {}


def cfg_of(rig):
    """the library's own configuration of a recipe's rig; it holds what the oracle's holds"""
    import flvis_amd
    if rig.name not in _CFG:
        _CFG[rig.name] = E.load_yaml(rig.yaml, flvis_amd.load_config)
        assert E.same_config(rig, _CFG[rig.name])
    return _CFG[rig.name]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinels(n, cap):
    """what the caller leaves in the outputs: a float64 ramp no result can equal, mask bytes of 0xA5"""
    return (-1.0e9 - 0.5 * np.arange(n * cap * 3, dtype=np.float64)).reshape(n, cap, 3), np.full((n, cap), 0xA5, np.uint8)


def run(ctx, call, state=None, cfg=None):
    """one flvis_hip_stereo_depth call on caller-filled outputs -> (pt3ds, mask, state after, the sentinels)"""
    a = call.arrays()
    n, cap = len(call.sets), call.cap
    out0, mask0 = sentinels(n, cap)
    if state is None:
        state = ctx.rand_seed(1, n)
    got3, gotm = ctx.stereo_depth(cfg_of(call.rig) if cfg is None else cfg, _cuda(a["img0"]), _cuda(a["img1"]), _cuda(a["p2d"]), _cuda(a["p2u"]),
                                  _cuda(a["p3w"]), _cuda(a["has"]), _cuda(a["count"]), a["poses"], call.rng, state, out=_cuda(out0), mask=_cuda(mask0))
    ctx.synchronize()
    return got3.cpu().numpy(), gotm.cpu().numpy(), state, (out0, mask0)


def check(call, res, want=None):
    """every set against the oracle's answer (want[s] = (pt3ds, mask); default: each set's own, from a fresh generator)"""
    got3, gotm, _, (out0, mask0) = res
    for i, s in enumerate(call.sets):
        w3, wm = (s.want3, s.wantm) if want is None else want[i]
        n = s.n
        where = (call.name, "set %d" % i, s.name)
        bad = np.flatnonzero(gotm[i, :n] != wm)
        assert len(bad) == 0, (where, "mask", "%d of %d differ, the first at %d" % (len(bad), n, bad[0]), int(gotm[i, bad[0]]), got3[i, bad[0]], w3[bad[0]])
        bad = np.flatnonzero((got3[i, :n].view(np.uint64) != w3.view(np.uint64)).any(1))
        assert len(bad) == 0, (where, "point", "%d of %d differ, the first at %d" % (len(bad), n, bad[0]), got3[i, bad[0]], w3[bad[0]], int(wm[bad[0]]))
        assert np.array_equal(got3[i, n:].view(np.uint64), out0[i, n:].view(np.uint64)), (where, "a point at or behind min(count, cap) was written")
        assert gotm[i, n:].tobytes() == mask0[i, n:].tobytes(), (where, "a mask byte at or behind min(count, cap) was written")


def state_after(ctx, draws):
    """the generator state after `draws` values from seed 1: rand_seed(1, 1), then one call in which exactly `draws` landmarks fail"""
    st = ctx.rand_seed(1, 1)
    if draws:
        c = E.Call("flat", [E.flat_set(draws)])
        check(c, run(ctx, c, st))
    return st.cpu().numpy()[0]


def next_depths(ctx, state_row, n=80):
    """the next n dummy depths a state would hand out (on a copy)"""
    c = E.Call("flat", [E.flat_set(n)])
    got3, gotm, _, _ = run(ctx, c, _cuda(np.ascontiguousarray(state_row[None])))
    assert not gotm.any()
    return got3[0, :, 2].copy()


@pytest.mark.parametrize("name", list(E.CALLS))
def test_recipes_bit_exact(ctx, name):
    call = E.call(name)
    res = run(ctx, call)
    check(call, res)
    state = res[2].cpu().numpy()
    seeded = ctx.rand_seed(1, 1).cpu().numpy()[0]
    for i, s in enumerate(call.sets):
        assert 0 <= state[i, 34] < 34 and state[i, 34] == s.fails % 34, (name, i, "ring position")
        if s.fails == 0:                                    # no failure: the generator has not moved
            assert np.array_equal(state[i], seeded), (name, i)


def test_generator_after_batches_and_after_a_count_above_capacity(ctx):
    """the state a set leaves behind is the state after as many draws as the oracle made over the first min(count, cap) landmarks, word
    for word -- over one batch, two and three, and where the count exceeds the capacity"""
    for call in (E.batch_call(), E.overcount_call()):
        state = run(ctx, call)[2].cpu().numpy()
        for i, s in enumerate(call.sets):
            assert np.array_equal(state[i], state_after(ctx, s.fails)), (call.name, i, s.fails)
    s = E.overcount_call().sets[2]
    z = next_depths(ctx, state[2])
    assert np.array_equal(z, E.glibc_depths(s.fails + len(z))[s.fails:])


def test_state_carries_over_four_calls(ctx):
    calls, want, draws = E.carry_calls()
    state = ctx.rand_seed(1, 4)
    for k, c in enumerate(calls):
        check(c, run(ctx, c, state), want[k])
    state = state.cpu().numpy()
    for i in range(4):
        ref = state_after(ctx, draws[i])
        assert state[i, 34] == draws[i] % 34 == ref[34]
        assert np.array_equal(state[i], ref), (i, draws[i])
        a, b = next_depths(ctx, state[i]), next_depths(ctx, ref)                # the property that matters: the next draws agree
        assert np.array_equal(a, b) and np.array_equal(a, E.glibc_depths(draws[i] + len(a))[draws[i]:])


def test_sets_do_not_depend_on_their_neighbours(ctx):
    call = E.batch_call()
    together = run(ctx, call)
    check(call, together)
    for i in range(len(call.sets)):
        alone = run(ctx, call.alone(i))
        check(call.alone(i), alone)
        k = call.sets[i].n                                  # (slots behind a set's landmarks hold each call's own sentinels)
        assert alone[0][0, :k].tobytes() == together[0][i, :k].tobytes() and alone[1][0, :k].tobytes() == together[1][i, :k].tobytes(), i
        assert np.array_equal(alone[2].cpu().numpy()[0], together[2].cpu().numpy()[i]), i
    order = (5, 2, 6, 0, 4, 1, 3)
    perm = call.permuted(order)
    res = run(ctx, perm)
    check(perm, res)
    n = [s.n for s in perm.sets]
    for j, i in enumerate(order):
        assert res[0][j, :n[j]].tobytes() == together[0][i, :n[j]].tobytes() and res[1][j, :n[j]].tobytes() == together[1][i, :n[j]].tobytes()
    assert np.array_equal(res[2].cpu().numpy(), together[2].cpu().numpy()[list(order)])


def test_refusals_launch_nothing(ctx):
    import ctypes as C

    import flvis_amd
    from flvis_amd import synth
    call = E.overcount_call()
    cfg = cfg_of(call.rig)
    a = call.arrays()
    n, cap = len(call.sets), call.cap
    out0, mask0 = sentinels(n, cap)
    dev = {k: _cuda(v) for k, v in a.items() if k != "poses"}
    out, mask, state = _cuda(out0), _cuda(mask0), ctx.rand_seed(1, n)
    state0 = state.cpu().numpy()

    def raw(cfg_, n_sets, cap_):
        """the library through the context's handle, as Context.stereo_depth calls it"""
        p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731
        f = ctx._lib.flvis_hip_stereo_depth
        rc = f(ctx._h, C.byref(cfg_), p(dev["img0"]), p(dev["img1"]), n_sets, p(dev["p2d"]), p(dev["p2u"]), p(dev["p3w"]), p(dev["has"]),
               p(dev["count"]), cap_, a["poses"].ctypes.data, 3.0, p(state), p(out), p(mask))
        ctx._check(rc, "stereo_depth")

    dcfg = E.load_yaml(synth.D435I_DEPTH_YAML, flvis_amd.load_config)
    unfinished = copy.copy(cfg)
    for k in range(12):
        unfinished.P0[k] = 0.0
        unfinished.P1[k] = 0.0
    for what, args in (("cap = 0", (cfg, n, 0)), ("n_sets = 0", (cfg, 0, cap)), ("negative cap", (cfg, n, -1)), ("a depth-camera rig", (dcfg, n, cap)),
                       ("a configuration that was never finalised", (unfinished, n, cap))):
        with pytest.raises(flvis_amd.FlvisError):
            raw(*args)
        ctx.synchronize()
        assert out.cpu().numpy().tobytes() == out0.tobytes() and mask.cpu().numpy().tobytes() == mask0.tobytes(), what
        assert np.array_equal(state.cpu().numpy(), state0), what
    import torch
    with pytest.raises(flvis_amd.FlvisError):              # the wrapper with no capacity / no set: refused as well
        ctx.stereo_depth(cfg, dev["img0"], dev["img1"], torch.zeros((n, 0, 2), device="cuda"), torch.zeros((n, 0, 2), device="cuda"),
                         torch.zeros((n, 0, 3), device="cuda"), torch.zeros((n, 0), dtype=torch.uint8, device="cuda"), dev["count"], a["poses"], 3.0, state)
    with pytest.raises(flvis_amd.FlvisError):
        ctx.stereo_depth(cfg, dev["img0"][:0], dev["img1"][:0], dev["p2d"][:0], dev["p2u"][:0], dev["p3w"][:0], dev["has"][:0], dev["count"][:0],
                         a["poses"][:0], 3.0, state[:0])
    raw(cfg, n, cap)                                        # and the same arguments with nothing wrong: accepted
    ctx.synchronize()
    assert mask.cpu().numpy()[0, 0] in (0, 1)
