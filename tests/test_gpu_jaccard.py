"""The kernels of csrc/cooc.hip (pinsage_cooc_counts, pinsage_cooc_jaccard, the
latter through the selection kernel of csrc/knn.hip under its Jaccard key) and
what stands on them: baselines.JaccardFast, and with save_knn / LazyKnnDict /
compute_results_table the results table end to end.

Counts are integers and compared exactly with tests/jaccard_util.py's set
intersections.  Scores are compared bit for bit and ids exactly with its
np.lexsort order (score descending, id ascending); against the reference's
recorded lists (tests/golden/jaccard.npz), whose order among equal scores is
torch.topk's, the scores bit for bit and the ids by the tie-insensitive check.
Every output is pre-filled with a sentinel and carries a padded tail, so an
unwritten or overwritten value shows.  The numpy reference is checked on the
host in tests/test_jaccard_host.py.
"""
import numpy as np
import pytest
import torch

import jaccard_util as ju
from conftest import golden

pytestmark = pytest.mark.gpu

ERR_ARG = -2       # pinsage_status (include/pinsage_hip.h)
SENT_F = -123.0
SENT_I = -7
PAD = 8            # sentinel values behind every output


# ----------------------------------------------------------------------------- launch helpers
class Dev:
    """A membership matrix's two CSRs on the device."""

    def __init__(self, member):
        self.n_cols, self.n = member.shape
        self.arrays = [torch.from_numpy(a).cuda() for a in ju.csrs(member)]

    def args(self):
        import _native as nat
        return [nat.ptr(a) for a in self.arrays] + [self.n, self.n_cols]


def _counts(dev, queries):
    """pinsage_cooc_counts with a sentinel-filled output: (status, [nq, n], error word)."""
    import _native as nat
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int64)).cuda()
    nq = int(q.numel())
    out = torch.full((nq * dev.n + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = nat.lib().pinsage_cooc_counts(*dev.args(), nat.ptr(q), nq, nat.ptr(out), nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[nq * dev.n:] == SENT_I).all(), "values behind the count rows were written"
    return rc, o[:nq * dev.n].reshape(nq, dev.n), int(err)


def _jaccard(dev, queries, k, rows=None):
    """pinsage_cooc_jaccard with sentinel-filled outputs and a scratch sized for
    `rows` query rows (default: all): (status, w [nq, k], ids [nq, k], error word)."""
    import _native as nat
    L = nat.lib()
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int64)).cuda()
    nq, kk = int(q.numel()), max(int(k), 0)
    w = torch.full((nq * kk + PAD,), SENT_F, dtype=torch.float32, device="cuda")
    nb = torch.full((nq * kk + PAD,), SENT_I, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = int(L.pinsage_cooc_scratch_bytes(dev.n, nq if rows is None else rows))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = L.pinsage_cooc_jaccard(*dev.args(), nat.ptr(q), nq, int(k), nat.ptr(scratch), nbytes, nat.ptr(w),
                                nat.ptr(nb), nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    wh, nh = w.cpu().numpy(), nb.cpu().numpy()
    assert (wh[nq * kk:] == SENT_F).all() and (nh[nq * kk:] == SENT_I).all(), "values behind the lists were written"
    return rc, wh[:nq * kk].reshape(nq, kk), nh[:nq * kk].reshape(nq, kk), int(err)


def _check_knn(member, queries, k, rows=None):
    """Lists of the device against the lexsort reference, exact; returns them."""
    rc, w, nb, err = _jaccard(Dev(member), queries, k, rows)
    assert rc == 0 and err == 0
    score = ju.scores(ju.counts(member, queries), ju.degrees(member), queries)
    want_w, want_n = ju.topk(score, k)
    ju.check_exact(w, nb, want_w, want_n, f"n = {member.shape[1]}, k = {k}")
    return w, nb, score


# ----------------------------------------------------------------------------- the fixture graph
@pytest.fixture(scope="module")
def fx():
    import baselines as bl
    import graph
    f = golden("jaccard")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    edges = f["edges"].astype(np.int64)
    g = graph.CSRGraph(n + nc, edges[:, 0], edges[:, 1])
    model = bl.JaccardFast()
    model.train(g, list(range(n)), None, None, None)
    member = ju.memberships(n, nc, edges)
    score = ju.scores(f["intersect_sizes"].astype(np.int32), f["nbh_sizes"].astype(np.int64), np.arange(n))
    return f, g, model, member, score


def test_fixture_counts(fx):
    f, _, model, member, _ = fx
    n = member.shape[1]
    want = f["intersect_sizes"].astype(np.int32)
    assert np.array_equal(model.nbh_sizes.cpu().numpy(), f["nbh_sizes"].astype(np.int64))
    rng = np.random.default_rng(5)
    q = np.concatenate([rng.permutation(n), rng.integers(0, n, 40)])   # shuffled, with repeats
    rc, got, err = _counts(Dev(member), q)
    assert rc == 0 and err == 0
    assert np.array_equal(got, want[q])
    # the model's own CSRs (built by torch on the GPU from the graph's edges) and its dense rows
    for a, b in zip(model._t2c + model._c2t, ju.csrs(member)):
        assert np.array_equal(a.cpu().numpy(), b) and a.cpu().numpy().dtype == b.dtype
    rows = model.intersect_sizes(torch.from_numpy(q))
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), want[q])


@pytest.mark.parametrize("k", [50, 2])
def test_fixture_knn(fx, k):
    f, _, model, member, score = fx
    n = member.shape[1]
    w, nb = model.knn(torch.arange(n), k)
    assert w.dtype == torch.float32 and nb.dtype == torch.int64 and tuple(w.shape) == tuple(nb.shape) == (n, k - 1)
    assert w.device.type == "cpu"                                       # on nodeset's device
    w, nb = w.numpy(), nb.numpy()
    assert np.array_equal(ju.bits(w), ju.bits(f[f"knn_w_{k}"])), "scores differ from the reference's torch.topk"
    want_w, want_n = ju.topk(score, k)
    ju.check_exact(w, nb, want_w[:, 1:], want_n[:, 1:], f"fixture, k = {k}")
    ju.check_lists(w, nb, score, f"fixture, k = {k}")
    wd, nd = model.knn(torch.arange(n).cuda(), k)
    assert wd.device.type == "cuda" and np.array_equal(nd.cpu().numpy(), nb)
    we, ne = model.knn(torch.empty(0, dtype=torch.int64), k)
    assert tuple(we.shape) == tuple(ne.shape) == (0, k - 1) and ne.dtype == torch.int64


# ----------------------------------------------------------------------------- counts: shapes
def _tile():
    import _native as nat
    return int(nat.lib().pinsage_cooc_tile())


QM, QNONE = 5, 7       # a track in 20 collections (more than a workgroup has waves); a track in none
QBIG, N_BIG = 11, 1100  # a track in 1100 more collections: more than a wave, and than a workgroup, takes at a time


def _shape_graph(n, T, seed):
    rng = np.random.default_rng(seed)
    member = np.zeros((23 + N_BIG, n), bool)
    hub = np.arange(max(0, T - 1500), min(n, T + 700))                  # > 1024 tracks, across the tile boundary if there is one
    assert len(hub) > 1024
    member[0, hub] = True
    member[1, [i for i in (0, T - 1, T, n - 1) if 0 <= i < n]] = True   # the first and last counter of a tile
    # collection 2 holds nothing
    for c in range(3, 23):
        member[c, rng.integers(0, n, 30)] = True
        member[c, QM] = True
    for c in range(23, 23 + N_BIG):
        member[c, rng.integers(0, n, 3)] = True
        member[c, QBIG] = True
    member[:, QNONE] = False
    return member


@pytest.mark.parametrize("which", ["T-1", "T", "T+5", "2T+3"])
def test_count_shapes(which):
    T = _tile()
    n = {"T-1": T - 1, "T": T, "T+5": T + 5, "2T+3": 2 * T + 3}[which]
    member = _shape_graph(n, T, seed=n)
    assert member[2].sum() == 0 and 20 <= member[:, QM].sum() < 64 and member[:, QNONE].sum() == 0
    assert member[:, QBIG].sum() >= N_BIG
    hub = np.flatnonzero(member[0])
    rng = np.random.default_rng(n + 1)
    q = np.array([i for i in (0, T - 1, T, n - 1) if 0 <= i < n] + [QM, QNONE, QBIG, hub[0], hub[-1], hub[len(hub) // 2]] +
                 rng.integers(0, n, 4).tolist(), np.int64)
    rc, got, err = _counts(Dev(member), q)
    assert rc == 0 and err == 0
    want = ju.counts(member, q)
    assert want.max() >= 2 and (want[q.tolist().index(QNONE)] == 0).all()
    bad = got != want
    assert not bad.any(), (f"n = {n}: query {q[np.argwhere(bad)[0][0]]}, track {np.argwhere(bad)[0][1]}: got "
                           f"{got[bad][0]}, reference {want[bad][0]}; {int(bad.sum())} cells differ")


# ----------------------------------------------------------------------------- selection regimes
def _regime_graph(n, seed):
    """Track 0: in no collection (an all-zero row).  Track 1: in one collection
    of 10 (fewer than 50 non-zeros).  Track 2: in one collection of 300 whose
    other members are mostly in nothing else: a block of some 288 equal scores
    1 / 1, then the few members of other collections at 1 / 5, then zeros.  The
    rest is seeded noise."""
    rng = np.random.default_rng(seed)
    member = np.zeros((40, n), bool)
    member[0, 1] = True
    member[0, rng.choice(np.arange(310, n), 9, replace=False)] = True
    member[1, 2:302] = True
    for c in range(2, 40):
        member[c, rng.integers(310, n, int(rng.integers(2, 40)))] = True
    member[2:6, rng.choice(np.arange(3, 302), 12, replace=False)] = True   # a few of the 300 with other scores
    member[:, 0] = False
    return member


@pytest.mark.parametrize("n,k", [(600, 1), (600, 50), (600, 600), (4100, 50), (4100, 4096), (9000, 50), (9001, 1),
                                 (9001, 50), (9001, 4096)])
def test_selection_regimes(n, k):
    member = _regime_graph(n, seed=n)
    rng = np.random.default_rng(k)
    q = np.array([0, 1, 2, 150] + rng.integers(302, n, 3).tolist(), np.int64)
    w, nb, score = _check_knn(member, q, k)
    nz = (score > 0).sum(1)
    assert nz[0] == 0 and nz[1] == 10 and nz[2] >= 300
    assert np.array_equal(nb[0], np.arange(k)) and (w[0] == 0).all()       # all zero: ids 0 .. k - 1
    if k > 10:                                                             # fewer than k non-zeros: the zero tail by id
        tail = nb[1, 10:]
        assert (w[1, :10] > 0).all() and (w[1, 10:] == 0).all() and (np.diff(tail) > 0).all() and tail[0] == 0
    if 20 < k < 300:                                                       # equal scores on both sides of position k
        kth = np.sort(score[2])[::-1][k - 1]
        assert (score[2] == kth).sum() > 100 and (score[2] > kth).sum() < k - 1
        assert w[2, k - 1] == w[2, k - 2] == kth


# ----------------------------------------------------------------------------- batching
def test_batching_short_last_batch():
    n, k = 601, 20
    member = _regime_graph(n, seed=3)
    q = np.array([2, 400, 1, 0, 555, 2, 310], np.int64)      # 7 queries over a 3-row scratch; query 2 in two batches
    w, nb, _ = _check_knn(member, q, k, rows=3)
    assert np.array_equal(nb[0], nb[5]) and np.array_equal(ju.bits(w[0]), ju.bits(w[5]))
    w1, nb1, _ = _check_knn(member, q, k, rows=1)
    assert np.array_equal(nb1, nb) and np.array_equal(ju.bits(w1), ju.bits(w))


# ----------------------------------------------------------------------------- rejections
def test_rejected_arguments_leave_outputs_untouched():
    member = _regime_graph(5000, seed=4)
    dev = Dev(member)
    q = np.array([1, 2, 3], np.int64)
    for k in (0, 5001, 4097):
        rc, w, nb, err = _jaccard(dev, q, k)
        assert rc == ERR_ARG and err == 0, k
        assert (w == SENT_F).all() and (nb == SENT_I).all(), k
    small = Dev(_regime_graph(600, seed=4))
    rc, w, nb, _ = _jaccard(small, q, 601)
    assert rc == ERR_ARG and (w == SENT_F).all() and (nb == SENT_I).all()


def test_out_of_range_queries():
    import baselines as bl
    import graph
    n = 600
    member = _regime_graph(n, seed=6)
    dev = Dev(member)
    for bad in (n, -1, 1 << 40):
        q = np.array([2, bad, 1], np.int64)
        rc, got, err = _counts(dev, q)
        assert rc == 0 and err == 1, bad
        assert np.array_equal(got, ju.counts(member, [2, 0, 1]))            # clamped to track 0
        rc, w, nb, err = _jaccard(dev, q, 10)
        assert rc == 0 and err == 1
        want_w, want_n = ju.knn_reference(n, 0, np.empty((0, 2)), [0], 10)  # track 0 is in no collection
        assert np.array_equal(nb[1], want_n[0]) and (w[1] == 0).all()
    c, t = np.nonzero(member)
    g = graph.CSRGraph(n + member.shape[0], c + n, t)
    model = bl.JaccardFast()
    model.train(g, list(range(n)), None, None, None)
    for bad in (n, -1):
        with pytest.raises(IndexError):
            model.knn(torch.tensor([3, bad]), 10)
        with pytest.raises(IndexError):
            model.intersect_sizes(torch.tensor([bad]))
    # an edge between two collections
    g2 = graph.CSRGraph(n + member.shape[0], np.append(c + n, n + 1), np.append(t, n + 2))
    with pytest.raises(ValueError):
        bl.JaccardFast().train(g2, list(range(n)), None, None, None)


# ----------------------------------------------------------------------------- direction and multiplicity
def test_direction_and_multiplicity():
    import baselines as bl
    import graph
    n, nc = 500, 30
    rng = np.random.default_rng(8)
    member = ju.memberships(n, nc, ju.seeded_graph(n, nc, seed=8))
    c, t = np.nonzero(member)
    sym = np.concatenate([np.stack([c + n, t], 1), np.stack([t, c + n], 1)])
    flip = rng.random(len(c)) < 0.5
    one = np.where(flip[:, None], np.stack([c + n, t], 1), np.stack([t, c + n], 1))
    one = np.concatenate([one, one[rng.integers(0, len(one), 200)], [[3, 4], [4, 3], [9, 9]]])  # repeats; track-track edges
    models = []
    for e in (sym, one[rng.permutation(len(one))]):
        m = bl.JaccardFast()
        m.train(graph.CSRGraph(n + nc, e[:, 0], e[:, 1]), list(range(n)), None, None, None)
        models.append(m)
    q = torch.arange(n)
    a, b = (m.intersect_sizes(q).cpu().numpy() for m in models)
    assert np.array_equal(a, b) and np.array_equal(a, ju.counts(member, np.arange(n)))
    assert torch.equal(models[0].nbh_sizes, models[1].nbh_sizes)
    assert np.array_equal(models[0].nbh_sizes.cpu().numpy(), ju.degrees(member))


# ----------------------------------------------------------------------------- determinism
def test_two_runs_give_the_same_bits():
    n = 9001
    member = _regime_graph(n, seed=9)
    dev = Dev(member)
    q = np.random.default_rng(9).integers(0, n, 24)
    _, c1, _ = _counts(dev, q)
    _, c2, _ = _counts(dev, q)
    assert np.array_equal(c1, c2)
    _, w1, n1, _ = _jaccard(dev, q, 100)
    _, w2, n2, _ = _jaccard(dev, q, 100)
    assert np.array_equal(ju.bits(w1), ju.bits(w2)) and np.array_equal(n1, n2)


# ----------------------------------------------------------------------------- end to end
def test_results_table_end_to_end(fx, tmp_path, monkeypatch):
    import baselines as bl
    f, g, model, member, _ = fx
    n = member.shape[1]
    # the fixture graph has 300 tracks: lists of PRECOMP_K = 1000 do not exist on it
    monkeypatch.setattr(bl, "PRECOMP_K", 200)
    rng = np.random.default_rng(10)
    pairs = []
    for c in range(1, member.shape[0]):                      # positives: co-members of the small collections
        tr = np.flatnonzero(member[c])
        for q in tr.tolist():
            if len(tr) > 1:
                pairs.append((q, int(rng.choice(tr[tr != q]))))
    tp = torch.tensor(pairs, dtype=torch.int64)
    assert (torch.bincount(tp[:, 0]) == 1).any()             # low-co accuracy at co_thr = 1 keeps something
    ids = list(range(n))
    rnd = bl.Random()
    rnd.train(g, ids, None, None, None)
    torch.manual_seed(0)
    bl.save_knn(model, "JaccardFast", ids, str(tmp_path), train_time=1.0, b_size=128)
    bl.save_knn(rnd, "Random", ids, str(tmp_path), b_size=128)
    d = bl.LazyKnnDict(["JaccardFast", "Random"], ids, str(tmp_path))
    w, nb = d["JaccardFast"]
    assert tuple(nb.shape) == (n, 199)                       # k - 1 columns, as the reference's knn returns
    want_w, want_n = model.knn(torch.arange(n), 200)         # one batch against the three of save_knn
    assert torch.equal(nb, want_n) and torch.equal(w, want_w)
    table = bl.compute_results_table(d, tp, g)
    assert list(table.index) == ["JaccardFast", "Random"]
    assert list(table.columns) == ["hr (k=10)", "hr (k=100)", "hr (k=500)", "mrr", "low-degree accuracy",
                                   "low-co accuracy", "t (train)", "t (emb)", "t (knn)"]
    assert np.isfinite(table.to_numpy(dtype=np.float64)).all()
    assert table.loc["JaccardFast", "t (train)"] == 1.0 and table.loc["JaccardFast", "t (knn)"] > 0
    # a sanity ordering on a graph built to have it, not a measured margin
    assert table.loc["JaccardFast", "hr (k=10)"] > table.loc["Random", "hr (k=10)"]
