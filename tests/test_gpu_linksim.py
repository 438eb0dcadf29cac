"""The weighted form of csrc/cooc.hip's tile kernel (pinsage_cooc_weighted_sums,
pinsage_cooc_weighted_knn, the latter through the selection kernel of
csrc/knn.hip under its score key) and what stands on it: baselines.AdamicAdar,
JaccardIndex and Preferential, up to the results table.

Sums are int64 and compared exactly with tests/linksim_util.py's restatement;
scores bit for bit and ids exactly with its np.lexsort order (score descending,
id ascending); against networkx's recorded scores (tests/golden/linksim.npz)
within the bound derived in tests/test_linksim_host.py, where the restatement
itself is checked.  Every output is pre-filled with a sentinel and carries a
padded tail, so an unwritten or overwritten value shows.  The graphs are those
of tests/test_gpu_jaccard.py.
"""
import numpy as np
import pytest
import torch

import jaccard_util as ju
import linksim_util as lu
from conftest import golden
from test_gpu_jaccard import ERR_ARG, N_BIG, PAD, QBIG, QM, QNONE, SENT_F, SENT_I, Dev, _regime_graph, _shape_graph

pytestmark = pytest.mark.gpu

SENT_L = -(1 << 50) - 7


# ----------------------------------------------------------------------------- launch helpers
def _dev_wt(wt):
    return torch.from_numpy(np.ascontiguousarray(wt, np.int64)).cuda()


def _sums(dev, wt, queries, args=None):
    """pinsage_cooc_weighted_sums with a sentinel-filled output: (status, [nq, n], error word).
    `args` replaces arguments by position (null pointers)."""
    import _native as nat
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int64)).cuda()
    wd = _dev_wt(wt)
    nq = int(q.numel())
    out = torch.full((nq * dev.n + PAD,), SENT_L, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    a = dev.args() + [nat.ptr(wd), nat.ptr(q), nq, nat.ptr(out), nat.ptr(err), nat.stream_ptr()]
    for i, v in (args or {}).items():
        a[i] = v
    rc = nat.lib().pinsage_cooc_weighted_sums(*a)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[nq * dev.n:] == SENT_L).all(), "values behind the sum rows were written"
    return rc, o[:nq * dev.n].reshape(nq, dev.n), int(err)


def _wknn(dev, wt, queries, k, rows=None, args=None, scratch_offset=0):
    """pinsage_cooc_weighted_knn with sentinel-filled outputs and a scratch sized
    for `rows` query rows (default: all): (status, w [nq, k], ids [nq, k], error word)."""
    import _native as nat
    L = nat.lib()
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int64)).cuda()
    wd = _dev_wt(wt)
    nq, kk = int(q.numel()), max(int(k), 0)
    w = torch.full((nq * kk + PAD,), SENT_F, dtype=torch.float32, device="cuda")
    nb = torch.full((nq * kk + PAD,), SENT_I, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = int(L.pinsage_cooc_weighted_scratch_bytes(dev.n, nq if rows is None else rows))
    scratch = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    a = dev.args() + [nat.ptr(wd), nat.ptr(q), nq, int(k), nat.ptr(scratch[scratch_offset:]), nbytes, nat.ptr(w),
                      nat.ptr(nb), nat.ptr(err), nat.stream_ptr()]
    for i, v in (args or {}).items():
        a[i] = v
    rc = L.pinsage_cooc_weighted_knn(*a)
    torch.cuda.synchronize()
    wh, nh = w.cpu().numpy(), nb.cpu().numpy()
    assert (wh[nq * kk:] == SENT_F).all() and (nh[nq * kk:] == SENT_I).all(), "values behind the lists were written"
    return rc, wh[:nq * kk].reshape(nq, kk), nh[:nq * kk].reshape(nq, kk), int(err)


def _check_wknn(member, queries, k, rows=None):
    """Lists of the device against the lexsort reference, exact; returns them."""
    wt = lu.weights(member.sum(1))
    rc, w, nb, err = _wknn(Dev(member), wt, queries, k, rows)
    assert rc == 0 and err == 0
    score = lu.to_score(lu.sums(member, wt, queries))
    want_w, want_n = ju.topk(score, k)
    ju.check_exact(w, nb, want_w, want_n, f"n = {member.shape[1]}, k = {k}")
    return w, nb, score


def _tile():
    import _native as nat
    return int(nat.lib().pinsage_cooc_weighted_tile())


# ----------------------------------------------------------------------------- sums: shapes
_shapes = {}


def _shape_case(which):
    """The graph, its device CSRs and the queries of one size, built once."""
    if which not in _shapes:
        T = _tile()
        n = {"T-1": T - 1, "T": T, "T+5": T + 5, "2T+3": 2 * T + 3}[which]
        member = _shape_graph(n, T, seed=n)
        assert member[2].sum() == 0 and 20 <= member[:, QM].sum() < 64 and member[:, QNONE].sum() == 0
        assert member[:, QBIG].sum() >= N_BIG
        hub = np.flatnonzero(member[0])
        rng = np.random.default_rng(n + 1)
        q = np.array([i for i in (0, T - 1, T, n - 1) if 0 <= i < n] +
                     [QM, QNONE, QBIG, hub[0], hub[-1], hub[len(hub) // 2]] + rng.integers(0, n, 4).tolist(), np.int64)
        q = np.concatenate([q, q[:3]])[rng.permutation(len(q) + 3)]         # shuffled, with repeats
        _shapes[which] = (member, Dev(member), q)
    return _shapes[which]


@pytest.mark.parametrize("table", ["adamic_adar", "large"])
@pytest.mark.parametrize("which", ["T-1", "T", "T+5", "2T+3"])
def test_sum_shapes(which, table):
    import baselines as bl
    member, dev, q = _shape_case(which)
    n = member.shape[1]
    if table == "adamic_adar":
        wt = bl.adamic_adar_weights(torch.from_numpy(member.sum(1))).numpy()
        assert wt[2] == 0 and wt[0] > 0                                     # the empty middle node weighs nothing
    else:  # a 32-bit add, or one that drops the carry into the high word, shows
        wt = np.where(np.arange(member.shape[0]) % 2 == 0, (1 << 33) + 3, (1 << 40) + 1).astype(np.int64)
    rc, got, err = _sums(dev, wt, q)
    assert rc == 0 and err == 0
    want = lu.sums(member, wt, q)
    assert want.max() > 1 << 32 and (want[q.tolist().index(QNONE)] == 0).all()
    bad = got != want
    assert not bad.any(), (f"n = {n}: query {q[np.argwhere(bad)[0][0]]}, track {np.argwhere(bad)[0][1]}: got "
                           f"{got[bad][0]}, reference {want[bad][0]}; {int(bad.sum())} cells differ")


# ----------------------------------------------------------------------------- selection regimes
@pytest.mark.parametrize("n,k", [(600, 1), (600, 600), (4100, 50), (4100, 4096), (9001, 50), (9001, 4096)])
def test_list_regimes(n, k):
    member = _regime_graph(n, seed=n)
    rng = np.random.default_rng(k)
    q = np.array([0, 1, 2, 150] + rng.integers(302, n, 3).tolist(), np.int64)
    w, nb, score = _check_wknn(member, q, k)
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
    w, nb, _ = _check_wknn(member, q, k, rows=3)
    assert np.array_equal(nb[0], nb[5]) and np.array_equal(ju.bits(w[0]), ju.bits(w[5]))
    w1, nb1, _ = _check_wknn(member, q, k, rows=1)
    assert np.array_equal(nb1, nb) and np.array_equal(ju.bits(w1), ju.bits(w))


# ----------------------------------------------------------------------------- rejections
def test_rejected_arguments_leave_outputs_untouched():
    member = _regime_graph(5000, seed=4)
    dev = Dev(member)
    wt = lu.weights(member.sum(1))
    q = np.array([1, 2, 3], np.int64)

    def untouched(rc, w, nb, what):
        assert rc == ERR_ARG, what
        assert (w == SENT_F).all() and (nb == SENT_I).all(), what

    for k in (0, 5001, 4097):
        rc, w, nb, err = _wknn(dev, wt, q, k)
        assert err == 0
        untouched(rc, w, nb, f"k = {k}")
    small = Dev(_regime_graph(600, seed=4))
    rc, w, nb, _ = _wknn(small, lu.weights(np.zeros(40)), q, 601)
    untouched(rc, w, nb, "k = n + 1")
    # null pointers, by position: t2c_ptr, c2t_ptr, wt, queries, out_w, out_n, scratch
    for pos in (0, 2, 6, 7, 12, 13, 10):
        rc, w, nb, _ = _wknn(dev, wt, q, 10, args={pos: None})
        untouched(rc, w, nb, f"null argument {pos}")
    rc, w, nb, _ = _wknn(dev, wt, q, 10, scratch_offset=4)
    untouched(rc, w, nb, "misaligned scratch")
    for pos in (0, 2, 6, 7, 9):                              # ... and of the sums: the same, and out
        rc, got, _ = _sums(dev, wt, q, args={pos: None})
        assert rc == ERR_ARG and (got == SENT_L).all(), pos


def test_out_of_range_queries():
    import baselines as bl
    import graph
    n = 600
    member = _regime_graph(n, seed=6)
    dev = Dev(member)
    wt = lu.weights(member.sum(1))
    for bad in (n, -1, 1 << 40):
        q = np.array([2, bad, 1], np.int64)
        rc, got, err = _sums(dev, wt, q)
        assert rc == 0 and err == 1, bad
        assert np.array_equal(got, lu.sums(member, wt, [2, 0, 1]))          # clamped to track 0
        rc, w, nb, err = _wknn(dev, wt, q, 10)
        assert rc == 0 and err == 1
        assert np.array_equal(nb[1], np.arange(10)) and (w[1] == 0).all()   # track 0 is in no collection
    c, t = np.nonzero(member)
    g = graph.CSRGraph(n + member.shape[0], c + n, t)
    ids = list(range(n))
    for cls in (bl.AdamicAdar, bl.JaccardIndex, bl.Preferential):
        model = cls(projected=False)
        model.train(g, ids, None, None, None)
        for bad in (n, -1):
            with pytest.raises(IndexError):
                model.knn(torch.tensor([3, bad]), 10)
    with pytest.raises(IndexError):
        model_aa = bl.AdamicAdar(projected=False)
        model_aa.train(g, ids, None, None, None)
        model_aa.sums(torch.tensor([n]))
    # an edge between two collections
    g2 = graph.CSRGraph(n + member.shape[0], np.append(c + n, n + 1), np.append(t, n + 2))
    for projected in (False, True):
        with pytest.raises(ValueError):
            bl.AdamicAdar(projected=projected).train(g2, ids, None, None, None)


# ----------------------------------------------------------------------------- the fixture graph
@pytest.fixture(scope="module")
def fx():
    import graph
    f = golden("linksim")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    edges = f["edges"].astype(np.int64)
    g = graph.CSRGraph(n + nc, edges[:, 0], edges[:, 1])
    member = ju.memberships(n, nc, edges)
    return f, g, {False: member, True: lu.projected(member)}, f["queries"].astype(np.int64)


def _train(cls, g, n, projected):
    model = cls(projected=projected)
    model.train(g, list(range(n)), None, None, None)
    return model


@pytest.mark.parametrize("projected", [False, True])
def test_fixture_adamic_adar(fx, projected):
    import baselines as bl
    f, g, adjs, q = fx
    adj, tag = adjs[projected], "proj" if projected else "bip"
    n, k = adj.shape[1], 50
    model = _train(bl.AdamicAdar, g, n, projected)
    assert model.n_mid == adj.shape[0] and np.array_equal(model.deg.cpu().numpy(), adj.sum(0))
    wt = model.weights.cpu().numpy()
    assert (np.abs(wt - lu.weights(adj.sum(1))) <= 1).all() and (wt[adj.sum(1) <= 1] == 0).all()
    s = model.sums(torch.from_numpy(q))
    assert s.dtype == torch.int64 and s.device.type == "cuda" and tuple(s.shape) == (len(q), n)
    assert np.array_equal(s.cpu().numpy(), lu.sums(adj, wt, q))
    own = lu.to_score(s.cpu().numpy())
    w, nb = model.knn(torch.from_numpy(q), k)
    assert w.dtype == torch.float32 and nb.dtype == torch.int64 and tuple(w.shape) == tuple(nb.shape) == (len(q), k)
    assert w.device.type == "cpu"                                           # on nodeset's device
    w, nb = w.numpy(), nb.numpy()
    ju.check_lists(w, nb, own, f"{tag}: ids against the package's own rows")
    want_w, want_n = ju.topk(own, k)
    ju.check_exact(w, nb, want_w, want_n, tag)
    ref = np.take_along_axis(f[f"aa_{tag}"], nb, 1)                         # networkx's scores at the returned ids
    cn = np.take_along_axis(lu.common(adj, q), nb, 1)
    ok = ~np.isnan(ref)
    assert (~ok).sum() <= 2 and ok.sum() > 0
    err = np.abs(w.astype(np.float64) - ref.astype(np.float64))
    assert (err[ok] <= lu.aa_bound(cn, ref)[ok]).all(), (tag, err[ok].max())
    wd, nd = model.knn(torch.from_numpy(q).cuda(), k)
    assert wd.device.type == "cuda" and np.array_equal(nd.cpu().numpy(), nb)
    we, ne = model.knn(torch.empty(0, dtype=torch.int64), k)
    assert tuple(we.shape) == tuple(ne.shape) == (0, k) and ne.dtype == torch.int64 and we.dtype == torch.float32
    assert tuple(model.sums(torch.empty(0, dtype=torch.int64)).shape) == (0, n)


@pytest.mark.parametrize("projected", [False, True])
def test_fixture_jaccard_index(fx, projected):
    import baselines as bl
    f, g, adjs, q = fx
    tag = "proj" if projected else "bip"
    n, k = adjs[projected].shape[1], 50
    model = _train(bl.JaccardIndex, g, n, projected)
    w, nb = model.knn(torch.from_numpy(q), k)
    assert w.dtype == torch.float32 and nb.dtype == torch.int64 and tuple(w.shape) == tuple(nb.shape) == (len(q), k)
    assert w.device.type == "cpu"
    want_w, want_n = ju.topk(f[f"jc_{tag}"], k)                             # networkx's scores, this package's order
    ju.check_exact(w.numpy(), nb.numpy(), want_w, want_n, tag)
    we, ne = model.knn(torch.empty(0, dtype=torch.int64).cuda(), k)
    assert tuple(we.shape) == tuple(ne.shape) == (0, k) and we.device.type == "cuda"
    if not projected:
        fast = bl.JaccardFast()
        fast.train(g, list(range(n)), None, None, None)
        fw, fn = fast.knn(torch.from_numpy(q), k)
        assert torch.equal(fn, nb[:, 1:]) and torch.equal(fw, w[:, 1:])


@pytest.mark.parametrize("projected", [False, True])
def test_fixture_preferential(fx, projected):
    import baselines as bl
    f, g, adjs, q = fx
    tag = "proj" if projected else "bip"
    adj = adjs[projected]
    n, k = adj.shape[1], 50
    model = _train(bl.Preferential, g, n, projected)
    w, nb = model.knn(torch.from_numpy(q), k)
    assert w.dtype == torch.int64 and nb.dtype == torch.int64 and tuple(w.shape) == tuple(nb.shape) == (len(q), k)
    assert w.device.type == "cpu"
    pa = f[f"pa_{tag}"]
    want_w, want_n = ju.topk(pa, k)                                         # (product descending, id ascending)
    assert np.array_equal(nb.numpy(), want_n) and np.array_equal(w.numpy(), want_w)
    lone = adj.sum(0)[q] == 0                                               # a query of degree 0: ids 0 .. k - 1, zeros
    assert lone.any() and (nb.numpy()[lone] == np.arange(k)).all() and (w.numpy()[lone] == 0).all()
    wd, nd = model.knn(torch.from_numpy(q).cuda(), n)                       # k = n: the whole order
    assert wd.device.type == "cuda" and tuple(nd.shape) == (len(q), n)
    assert np.array_equal(np.sort(nd.cpu().numpy(), 1), np.tile(np.arange(n), (len(q), 1)))
    we, ne = model.knn(torch.empty(0, dtype=torch.int64), k)
    assert tuple(we.shape) == tuple(ne.shape) == (0, k) and we.dtype == ne.dtype == torch.int64
    with pytest.raises(ValueError):
        model.knn(torch.from_numpy(q), n + 1)


# ----------------------------------------------------------------------------- determinism
def test_two_runs_give_the_same_bits():
    n = 9001
    member = _regime_graph(n, seed=9)
    dev = Dev(member)
    wt = lu.weights(member.sum(1))
    q = np.random.default_rng(9).integers(0, n, 24)
    _, s1, _ = _sums(dev, wt, q)
    _, s2, _ = _sums(dev, wt, q)
    assert np.array_equal(s1, s2) and s1.max() > 0
    _, w1, n1, _ = _wknn(dev, wt, q, 100)
    _, w2, n2, _ = _wknn(dev, wt, q, 100)
    assert np.array_equal(ju.bits(w1), ju.bits(w2)) and np.array_equal(n1, n2)


# ----------------------------------------------------------------------------- end to end
def test_results_table_end_to_end(fx, tmp_path, monkeypatch):
    import baselines as bl
    f, g, adjs, _ = fx
    member = adjs[False]
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
    ids = list(range(n))
    names = ["AdamicAdar", "JaccardIndex", "Preferential", "JaccardFast", "Random"]
    models = [bl.AdamicAdar(), bl.JaccardIndex(), bl.Preferential(), bl.JaccardFast(), bl.Random()]
    torch.manual_seed(0)
    for name, model in zip(names, models):
        model.train(g, ids, None, None, None)
        bl.save_knn(model, name, ids, str(tmp_path), train_time=1.0, b_size=128)
    d = bl.LazyKnnDict(names, ids, str(tmp_path))
    w, nb = d["AdamicAdar"]
    assert tuple(nb.shape) == (n, 200)                       # k columns: column 0 is kept
    want_w, want_n = models[0].knn(torch.arange(n), 200)     # one batch against the three of save_knn
    assert torch.equal(nb, want_n) and torch.equal(w, want_w)
    assert d["Preferential"][0].dtype == torch.int64 and tuple(d["JaccardFast"][1].shape) == (n, 199)
    table = bl.compute_results_table(d, tp, g)
    assert list(table.index) == names
    assert list(table.columns) == ["hr (k=10)", "hr (k=100)", "hr (k=500)", "mrr", "low-degree accuracy",
                                   "low-co accuracy", "t (train)", "t (emb)", "t (knn)"]
    assert np.isfinite(table.to_numpy(dtype=np.float64)).all()
    # a sanity ordering on a graph built to have it, not a measured margin
    assert table.loc["AdamicAdar", "hr (k=10)"] > table.loc["Random", "hr (k=10)"]
