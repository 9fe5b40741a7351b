"""GPU (-m gpu, MI355X): the bag-of-words transform (k_bow_words / voc_descend, k_bow_vector) and the three L1 score calls at their
edges, bit for bit against the CPU oracle (oracle/ref_bow.cpp): word ids, fp64 values and fp64 scores, no tolerance anywhere.  The
inputs come from tests/_bow_edges.py, whose recipes check themselves and are shown in tests/test_bow_edges_inputs.py (no GPU) to tell
DBoW3's rules from their near misses: last instead of first minimal child, no stop-word filter, count * weight, another order of a
sum, a depth bound one level short."""
import ctypes as C

import numpy as np
import pytest

import _bow_edges as E
from test_oracle_bow import RefVoc

pytestmark = pytest.mark.gpu

OK, ERR_INVALID_ARG, ERR_CAPACITY, ERR_CONFIG = 0, -1, -4, -5       # flvis_status of include/flvis_hip.h
INT_SENT, VAL_SENT = -77, -7.5                                      # what a raw call's outputs hold before it
GUARD = 32                                                          # entries behind an output's end


@pytest.fixture(scope="module")
def ctx():
    import flvis_amd
    c = flvis_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """the oracle's vectors, computed once: {part name: [(ids, vals)]}"""
    return {p.name: E.ref_transform(p) for f in E.TRANSFORM_RECIPES for p in f().parts}


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def transform(ctx, desc, count, vcap):
    return [t.cpu().numpy() for t in ctx.bow_transform(_cuda(desc), _cuda(count), vcap=vcap)]


def check_row(got, i, w, tag):
    """row i of a bow_transform result against the oracle's vector w, and the wrapper's fill behind it"""
    ids, vals, nnz = got
    n = int(nnz[i])
    assert n == len(w[0]), (tag, n, len(w[0]))
    assert np.array_equal(ids[i, :n], w[0]), tag
    assert np.array_equal(vals[i, :n], w[1]) and np.array_equal(_bits(vals[i, :n]), _bits(w[1])), tag
    assert np.all(ids[i, n:] == -1) and np.array_equal(_bits(vals[i, n:]), np.zeros(vals.shape[1] - n, np.int64)), tag


# ---- transform ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", [f.__name__ for f in E.TRANSFORM_RECIPES])
def test_transform_bit_exact(ctx, want, recipe):
    for p in getattr(E, recipe)().parts:
        ctx.bow_set_vocabulary(*p.voc)
        got = transform(ctx, p.desc, p.count, p.vcap)
        assert got[0].shape == (len(p.names), p.vcap)
        for i, name in enumerate(p.names):
            check_row(got, i, want[p.name][i], (p.name, name))


def test_full_meets_the_limits_of_k_bow_vector(ctx, want):
    """the figures of the `full` recipe as the kernel reports them: nnz == vcap == 2048, one entry of exactly 1.0, nnz == n_words"""
    r = E.full()
    p = r.part("full")
    ctx.bow_set_vocabulary(*p.voc)
    ids, vals, nnz = transform(ctx, p.desc, p.count, p.vcap)
    assert list(nnz) == [2048, 1, 1331, 63] and p.vcap == 2048
    assert vals[1, 0] == 1.0 and ids[1, 0] == 1234 and ids[0, 2047] == 2099 and ids[0, 0] == 0


BATCH_PARTS = (("stop_flat", "stop_flat"), ("stop_tree", "stop_tree"), ("ties", "ties"), ("uneven", "uneven"), ("full", "full"),
               ("full", "full_vcap300"), ("caps", "caps_257"))


@pytest.mark.parametrize("recipe,part", BATCH_PARTS)
def test_rows_do_not_depend_on_the_batch(ctx, want, recipe, part):
    """all keyframes of a vocabulary in one launch with empty keyframes (count 0 over other keyframes' descriptors) before, between and
    behind them, and every keyframe alone: the same rows, the oracle's"""
    p = getattr(E, recipe)().part(part)
    ctx.bow_set_vocabulary(*p.voc)
    n = len(p.names)
    desc = np.zeros((2 * n + 1, p.dcap, 32), np.uint8)
    count = np.zeros(2 * n + 1, np.int32)
    desc[1::2], count[1::2] = p.desc, p.count
    desc[0::2] = p.desc[np.arange(n + 1) % n][:, ::-1]                       # descriptors that must not be read
    got = transform(ctx, desc, count, p.vcap)
    for i, name in enumerate(p.names):
        check_row(got, 2 * i + 1, want[p.name][i], (p.name, name, "interleaved"))
    for i in range(0, 2 * n + 1, 2):
        check_row(got, i, (np.zeros(0, np.int32), np.zeros(0)), (p.name, i, "empty"))
    for i, name in enumerate(p.names):
        alone = transform(ctx, p.desc[i:i + 1], p.count[i:i + 1], p.vcap)
        check_row(alone, 0, want[p.name][i], (p.name, name, "alone"))
        assert np.array_equal(alone[0][0], got[0][2 * i + 1]) and np.array_equal(_bits(alone[1][0]), _bits(got[1][2 * i + 1]))


def test_small_call_after_a_large_one_reuses_the_scratch(ctx, want):
    """dcap 2048 x 4 keyframes, then directly dcap 255 x 1 and dcap 1 x 1 on the same vocabulary (the word scratch of the large call is
    reused, its stale words lie behind the small call's)"""
    p = E.full().part("full")
    ctx.bow_set_vocabulary(*p.voc)
    rv = RefVoc(p.voc)
    big = ctx.bow_transform(_cuda(p.desc), _cuda(p.count), vcap=p.vcap)
    small = [(p.desc[3:4, 1000:1255].copy(), 255), (p.desc[0:1, 7:8].copy(), 1)]
    outs = [ctx.bow_transform(_cuda(d), _cuda(np.array([dc], np.int32)), vcap=dc) for d, dc in small]
    for (d, dc), o in zip(small, outs):
        check_row([t.cpu().numpy() for t in o], 0, rv.transform(d[0]), ("after large", dc))
    big = [t.cpu().numpy() for t in big]
    for i, name in enumerate(p.names):
        check_row(big, i, want["full"][i], name)


# ---- scores ------------------------------------------------------------------------------------------------------------------------
class DevStore:
    def __init__(self, st):
        self.st, self.ids, self.vals, self.nnz = st, _cuda(st.ids), _cuda(st.vals), _cuda(st.nnz)
        self.want = {qn: E.ref_scores(st, q, *st.db[qn]) for qn, q in st.queries.items()}


@pytest.fixture(scope="module")
def stores():
    return {f.__name__: DevStore(f()) for f in E.SCORE_RECIPES}


def _windows(n, size):
    """windows of `size` entries that cover range(n), the last one flush with the end"""
    return sorted(set(min(o, n - size) for o in range(0, n, size)))


@pytest.mark.parametrize("recipe,sizes", [("chunks", E.CHUNK_NDB), ("order", (1, 2, 3))])
def test_score_row_bit_exact_at_every_store_size(ctx, stores, recipe, sizes):
    import torch
    ds = stores[recipe]
    st = ds.st
    for qn, q in st.queries.items():
        first, n = st.db[qn]
        want = ds.want[qn]
        outs, where = [], []
        for size in tuple(sizes) + (n,):
            for off in _windows(n, size):
                a, b = first + off, first + off + size
                outs.append(ctx.bow_score(ds.ids[q], ds.vals[q], ds.nnz[q:q + 1], ds.ids[a:b], ds.vals[a:b], ds.nnz[a:b]))
                where.append((size, off))
        got = torch.cat(outs).cpu().numpy()
        k = 0
        for size, off in where:
            assert np.array_equal(got[k:k + size], want[off:off + size]), (qn, size, off, got[k:k + size], want[off:off + size])
            k += size
        if recipe == "chunks":
            kinds = dict(zip(E.CHUNK_KINDS, got[-n:]))
            assert kinds["absent"] == 0.0 and kinds["disjoint"] == 0.0 and kinds["empty"] == 0.0 and kinds["one_miss"] == 0.0


SCORE_CASES = [("chunks", E.CHUNK_NDB), ("order", (1, 2, 3))]


@pytest.mark.parametrize("recipe,sizes", SCORE_CASES)
def test_score_jobs_every_query_at_every_range_length(ctx, stores, recipe, sizes):
    """flvis_hip_bow_score_jobs (scores[first + j]): every query of the recipe over its whole database range in ONE jobs list, then per
    range length the windows at multiples of it and the window flush with the range's end (two launches: they may overlap, and a job
    writes where it reads from)"""
    ds = stores[recipe]
    st = ds.st
    nv = len(st.vectors)
    want = np.full(nv, -1.0)
    for qn, q in st.queries.items():
        first, n = st.db[qn]
        want[first:first + n] = ds.want[qn]
    got = ctx.bow_score_jobs([(q,) + tuple(st.db[qn]) for qn, q in st.queries.items()], ds.ids, ds.vals, ds.nnz).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(_bits(got), _bits(want)), np.nonzero(got != want)[0]
    for size in sizes:
        for flush in (False, True):
            jobs, want = [], np.full(nv, -1.0)
            for qn, q in st.queries.items():
                first, n = st.db[qn]
                for off in ([n - size] if flush else range(0, n - size + 1, size)):
                    jobs.append((q, first + off, size))
                    want[first + off:first + off + size] = ds.want[qn][off:off + size]
            got = ctx.bow_score_jobs(jobs, ds.ids, ds.vals, ds.nnz).cpu().numpy()
            assert np.array_equal(got, want), (size, flush, np.nonzero(got != want)[0])


@pytest.mark.parametrize("recipe,sizes", SCORE_CASES)
def test_score_jobs_at_every_query_at_every_range_length(ctx, stores, recipe, sizes):
    """flvis_hip_bow_score_jobs_at (scores[out + j]): every query over its whole range and over the windows of every range length, in
    one launch, each job with an output offset of its own and one unwritten entry behind it"""
    ds = stores[recipe]
    st = ds.st
    jobs, want, out = [], [], 0
    for qn, q in st.queries.items():
        first, n = st.db[qn]
        for size in (n,) + tuple(sizes):
            for off in _windows(n, size):
                jobs.append((q, first + off, size, out))
                want += [ds.want[qn][off:off + size], [-1.0]]
                out += size + 1
    want = np.concatenate(want + [[-1.0] * 3])
    got = ctx.bow_score_jobs_at(jobs, ds.ids, ds.vals, ds.nnz, out + 3).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(_bits(got), _bits(want)), np.nonzero(got != want)[0]
    assert (got == -1.0).sum() == len(jobs) + 3


def test_score_jobs_bit_exact(ctx, stores):
    ds = stores["chunks"]
    st = ds.st
    kind = lambda qn, k: st.db[qn][0] + E.CHUNK_KINDS.index(k)
    n_kind = len(E.CHUNK_KINDS)
    inside = kind("q65", "identical")                                       # a query inside its own database range
    absent = kind("q128", "absent")                                         # a query with nnz < 0: its row scores 0.0
    jobs = [(st.queries["q200"], st.db["q200"][0], n_kind), (st.queries["q64"], st.db["q64"][0], 0), (inside, st.db["q65"][0], n_kind),
            (absent, st.db["q1"][0], n_kind), (st.queries["q129"], st.db["q129"][0] + 2, 5), (st.queries["q63"], kind("q63", "identical"), 1)]
    got = ctx.bow_score_jobs(jobs, ds.ids, ds.vals, ds.nnz).cpu().numpy()
    want = np.full(len(st.vectors), -1.0)
    for q, first, n in jobs:
        want[first:first + n] = E.ref_scores(st, q, first, n)
    assert np.array_equal(got, want), np.nonzero(got != want)[0]
    assert np.all(got[st.db["q1"][0]:st.db["q1"][0] + n_kind] == 0.0) and (got == -1.0).sum() == len(got) - 3 * n_kind - 6
    assert got[inside] == E.ref_scores(st, inside, inside, 1)[0] and got[inside] > 0
    # every job empty: nothing is written
    got = ctx.bow_score_jobs([(0, 5, 0), (3, 0, 0)], ds.ids, ds.vals, ds.nnz).cpu().numpy()
    assert np.all(got == -1.0)
    # as many jobs as the grid's second dimension takes: the first, the middle and the last job score one entry each, the others are
    # empty
    big = np.zeros((65535, 3), np.int32)
    some = {0: (st.queries["q65"], kind("q65", "pos_63_64")), 32767: (st.queries["q128"], kind("q128", "lane_63")),
            65534: (st.queries["q200"], kind("q200", "chunks_0_2"))}
    want = np.full(len(st.vectors), -1.0)
    for i, (q, first) in some.items():
        big[i] = (q, first, 1)
        want[first] = E.ref_scores(st, q, first, 1)[0]
    got = ctx.bow_score_jobs(big, ds.ids, ds.vals, ds.nnz).cpu().numpy()
    assert np.array_equal(got, want) and (got != -1.0).sum() == 3


def test_score_jobs_at_bit_exact(ctx, stores):
    import torch
    ds = stores["chunks"]
    st = ds.st
    n_kind = len(E.CHUNK_KINDS)
    f200, f64, f65 = st.db["q200"][0], st.db["q64"][0], st.db["q65"][0]
    absent = f65 + E.CHUNK_KINDS.index("absent")
    # (query, first, n, out): two queries over the same range, ranges of 1, 4 and 5, an empty job, an absent query
    jobs = [(st.queries["q200"], f200, n_kind, 0), (st.queries["q129"], f200, n_kind, 16), (st.queries["q65"], f65 + 3, 1, 31),
            (st.queries["q64"], f64, 4, 32), (st.queries["q128"], f200 + 7, 5, 37), (st.queries["q63"], f64, 0, 43), (absent, f64 + 1, 2, 44)]
    n_out = 48
    got = ctx.bow_score_jobs_at(jobs, ds.ids, ds.vals, ds.nnz, n_out).cpu().numpy()
    want = np.full(n_out, -1.0)
    for q, first, n, out in jobs:
        want[out:out + n] = E.ref_scores(st, q, first, n)
    assert np.array_equal(got, want), (got, want)
    assert [i for i in range(n_out) if got[i] == -1.0] == [15, 36, 42, 43, 46, 47] and np.all(got[44:46] == 0.0)
    assert not np.array_equal(got[0:n_kind], got[16:16 + n_kind])
    # flvis_hip_bow_score's numbers for the same pairs
    for q, first, n, out in jobs:
        if n and st.vectors[q] is not None:
            row = ctx.bow_score(ds.ids[q], ds.vals[q], ds.nnz[q:q + 1], ds.ids[first:first + n], ds.vals[first:first + n], ds.nnz[first:first + n])
            assert np.array_equal(_bits(row.cpu().numpy()), _bits(got[out:out + n])), (q, first, n)
    # every job empty: nothing is written
    assert np.all(ctx.bow_score_jobs_at([(0, 5, 0, 3), (3, 0, 0, 0)], ds.ids, ds.vals, ds.nnz, 8).cpu().numpy() == -1.0)
    # the order recipe through both job calls
    do = stores["order"]
    w = do.want["a"]
    assert np.array_equal(ctx.bow_score_jobs([(0, 0, 3)], do.ids, do.vals, do.nnz).cpu().numpy(), w)
    got = ctx.bow_score_jobs_at([(0, 1, 2, 3), (0, 0, 3, 0)], do.ids, do.vals, do.nnz, 5).cpu().numpy()
    assert np.array_equal(got, np.concatenate([w, w[1:]]))


def test_score_jobs_is_score_jobs_at_with_out_first(ctx, stores):
    """the two job calls are one kernel body at two job widths: (query, first, n) and (query, first, n, out = first) leave the same score
    array bit for bit -- whole ranges, ranges of one, an empty range among others, every job empty"""
    for name, ds in stores.items():
        st = ds.st
        nv = len(st.vectors)
        whole = [(q,) + tuple(st.db[qn]) for qn, q in st.queries.items()]
        ones = [(q, first + n - 1, 1) for q, first, n in whole]
        empty = [(q, first, 0) for q, first, n in whole]
        for jobs in (whole + empty[:1], ones, empty[-1:] + ones[:1], whole[:1], empty):
            a = ctx.bow_score_jobs(jobs, ds.ids, ds.vals, ds.nnz).cpu().numpy()
            b = ctx.bow_score_jobs_at([j + (j[1],) for j in jobs], ds.ids, ds.vals, ds.nnz, nv).cpu().numpy()
            assert np.array_equal(a, b) and np.array_equal(_bits(a), _bits(b)), (name, jobs, np.nonzero(a != b)[0])
            assert bool((a != -1.0).any()) == any(n for _, _, n in jobs), (name, jobs)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
class RawOut:
    """sentinel-filled outputs of a raw flvis_hip_bow_transform call, GUARD entries behind their ends"""

    def __init__(self, n, vcap):
        import torch
        self.n, self.vcap = n, vcap
        self.ids = torch.full((n * vcap + GUARD,), INT_SENT, dtype=torch.int32, device="cuda")
        self.vals = torch.full((n * vcap + GUARD,), VAL_SENT, dtype=torch.float64, device="cuda")
        self.nnz = torch.full((n + GUARD,), INT_SENT, dtype=torch.int32, device="cuda")

    def host(self):
        return self.ids.cpu().numpy(), self.vals.cpu().numpy(), self.nnz.cpu().numpy()

    def untouched(self):
        i, v, n = self.host()
        return bool((i == INT_SENT).all() and (v == VAL_SENT).all() and (n == INT_SENT).all())


def raw_transform(c, desc, count, dcap, n, vcap):
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = RawOut(n, vcap)
    d, k = _cuda(desc), _cuda(count)
    rc = c._lib.flvis_hip_bow_transform(c._h, ptr(d), ptr(k), int(dcap), int(n), int(vcap), ptr(out.ids), ptr(out.vals), ptr(out.nnz))
    c.synchronize()
    return rc, c._lib.flvis_last_error(c._h).decode(), out


def test_transform_refusals_come_before_any_launch(ctx, want):
    import flvis_amd
    p = E.uneven().parts[0]
    ctx.bow_set_vocabulary(*p.voc)
    n = len(p.names)
    assert p.n_words == 111 > E.uneven().figures["leaves"] and p.dcap == 256
    # vcap against min(dcap, n_words), with n_words = the largest id + 1: first n_words the smaller, then dcap
    for desc, dcap, need in ((p.desc, 256, 111), (p.desc[:, :64].copy(), 64, 64)):
        rc, msg, out = raw_transform(ctx, desc, np.minimum(p.count, dcap), dcap, n, need - 1)
        assert rc == ERR_CAPACITY and "vcap must hold min(dcap, number of words)" in msg and out.untouched(), (dcap, rc, msg)
        rc, msg, out = raw_transform(ctx, desc, np.minimum(p.count, dcap), dcap, n, need)
        assert rc == OK, (dcap, msg)
        ids, vals, nnz = out.host()
        rv = RefVoc(p.voc)
        for i in range(n):
            w = rv.transform(desc[i, :min(p.count[i], dcap)])
            k = int(nnz[i])
            assert k == len(w[0]) and np.array_equal(ids[i * need:i * need + k], w[0])
            assert np.array_equal(_bits(vals[i * need:i * need + k]), _bits(w[1]))
            assert np.all(ids[i * need + k:(i + 1) * need] == INT_SENT) and np.all(vals[i * need + k:(i + 1) * need] == VAL_SENT)
        assert np.all(ids[n * need:] == INT_SENT) and np.all(vals[n * need:] == VAL_SENT) and np.all(nnz[n:] == INT_SENT)
    # more descriptors per keyframe than k_bow_vector sorts
    rc, msg, out = raw_transform(ctx, np.zeros((1, 2049, 32), np.uint8), np.array([5], np.int32), 2049, 1, 2049)
    assert rc == ERR_CAPACITY and "at most 2048 descriptors" in msg and out.untouched()
    with pytest.raises(flvis_amd.FlvisError) as e:
        ctx.bow_transform(_cuda(np.zeros((1, 2049, 32), np.uint8)), _cuda(np.array([5], np.int32)), vcap=2049)
    assert "at most 2048 descriptors" in str(e.value)
    # no sizes
    for dcap, nn, vcap in ((0, 1, 8), (8, 0, 8), (8, 1, 0)):
        rc, msg, out = raw_transform(ctx, np.zeros((1, 8, 32), np.uint8), np.array([5], np.int32), dcap, nn, vcap)
        assert rc == ERR_INVALID_ARG and "bow_transform: bad args" in msg and out.untouched()
    # a context that was never given a vocabulary
    fresh = flvis_amd.Context(0)
    try:
        rc, msg, out = raw_transform(fresh, p.desc[:, :64].copy(), np.minimum(p.count, 64), 64, n, 64)
        assert rc == ERR_CONFIG and "no vocabulary" in msg and out.untouched()
        with pytest.raises(flvis_amd.FlvisError) as e:
            fresh.bow_transform(_cuda(p.desc), _cuda(p.count), vcap=256)
        assert "no vocabulary" in str(e.value)
    finally:
        fresh.close()


def test_score_jobs_refuses_more_jobs_than_the_grid_takes(ctx, stores):
    """n_jobs becomes gridDim.y (at most 65535): one more is refused by the entry point, not by a failed launch"""
    import torch
    import flvis_amd
    ds = stores["chunks"]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    q, first = ds.st.queries["q65"], ds.st.db["q65"][0]
    for n_jobs, width, fn in ((65536, 3, ctx._lib.flvis_hip_bow_score_jobs), (65536, 4, ctx._lib.flvis_hip_bow_score_jobs_at)):
        jobs = np.zeros((n_jobs, width), np.int32)
        jobs[:, 0], jobs[:, 1], jobs[:, 2] = q, first, 1
        scores = torch.full((len(ds.st.vectors),), VAL_SENT, dtype=torch.float64, device="cuda")
        rc = fn(ctx._h, n_jobs, jobs.ctypes.data_as(C.POINTER(C.c_int)), ptr(ds.ids), ptr(ds.vals), ptr(ds.nnz), ds.st.vcap, ptr(scores))
        ctx.synchronize()
        assert rc == ERR_INVALID_ARG and "bad args" in ctx._lib.flvis_last_error(ctx._h).decode(), (width, rc)
        assert bool((scores == VAL_SENT).all())
    with pytest.raises(flvis_amd.FlvisError) as e:
        ctx.bow_score_jobs(np.zeros((65536, 3), np.int32), ds.ids, ds.vals, ds.nnz)
    assert "bow_score_jobs: bad args" in str(e.value)
    for bad in ([(-1, 0, 1)], [(0, -1, 1)], [(0, 0, -1)]):
        with pytest.raises(flvis_amd.FlvisError) as e:
            ctx.bow_score_jobs(bad, ds.ids, ds.vals, ds.nnz)
        assert "negative index" in str(e.value)
