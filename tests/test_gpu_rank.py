"""pinsage_rank_cosine (rank_count_kernel, csrc/knn.hip) and what stands on it:
baselines.rank_from_emb and PinSage.evaluate.

The rank of a target is the number of rows that come before it in
pinsage_knn_cosine's order (similarity descending, index ascending).  On the
tables of parity_util.knn_select_table every similarity is exact in fp32, so
ranks are compared as integers, with the numpy reference (rank_util, checked
on the host in tests/test_eval_metrics.py) AND with the kNN's own columns:
column r of the query's row holds the target exactly when rank == r < k.

The kernel has two forms, which must agree: up to 8 targets of a query are
counted from registers (ballot + popcount), larger groups are sorted in LDS
and counted through a histogram and a prefix.  Each launch asserts, before it
runs, the form every one of its groups takes (rank_util.rank_form), and every
output is pre-filled with a sentinel so that an unwritten pair shows.
"""
import os
import tempfile

import numpy as np
import pytest
import torch

import parity_util as pu
import rank_util as ru

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE = -2, -3  # pinsage_status (include/pinsage_hip.h)
SENTINEL = -7


def _capi(emb_dev, n, d, ld, rows_q, grp_ptr, targets, forms=None, scratch_bytes=None, rows=None, np_=None):
    """pinsage_rank_cosine on device tensors with a sentinel-filled output:
    (status, ranks) after a synchronise.  `forms`: the form each group must take."""
    import _native as nat
    L = nat.lib()
    grp = torch.as_tensor(np.asarray(grp_ptr, np.int64))
    if forms is not None:
        sizes = np.diff(grp.numpy())
        assert [ru.rank_form(int(m)) for m in sizes] == list(forms), (sizes.tolist(), forms)
    qd = torch.as_tensor(np.asarray(rows_q, np.int64)).cuda()
    td = torch.as_tensor(np.asarray(targets, np.int64)).cuda()
    npairs = int(td.numel()) if np_ is None else int(np_)
    out = torch.full((max(1, int(td.numel())),), SENTINEL, dtype=torch.int64, device="cuda")
    nu = int(qd.numel())
    full = int(L.pinsage_rank_scratch_bytes(n, rows or max(1, nu)))
    scratch = torch.zeros(full, dtype=torch.uint8, device="cuda")
    rc = L.pinsage_rank_cosine(nat.ptr(emb_dev), n, d, ld, nat.ptr(qd), nu, nat.ptr(grp), nat.ptr(td), npairs, 1e-16,
                               nat.ptr(scratch), full if scratch_bytes is None else int(scratch_bytes),
                               nat.ptr(out), nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:int(td.numel())]


def _knn_ids(emb, q, k):
    import baselines
    _, ids = baselines._knn_cosine(torch.from_numpy(np.array(emb)), torch.from_numpy(np.array(q, np.int64)), k)
    return ids.numpy()


def _layout(q, t):
    """One launch over one query's targets t, laid out so that both forms (and
    both sides of the switch) rank the same targets: the whole group (sorted),
    its first 9 (sorted), first 8 (few), then the rest in groups of at most 8,
    the last possibly of 1 (few).  Returns (rows_q, grp_ptr, targets, forms)."""
    t = np.asarray(t, np.int64)
    assert len(t) > ru.RANK_FEW + 1
    groups = [t, t[:ru.RANK_FEW + 1], t[:ru.RANK_FEW]]
    groups += [t[i:i + ru.RANK_FEW] for i in range(ru.RANK_FEW, len(t), ru.RANK_FEW)]
    forms = ["sorted", "sorted"] + ["few"] * (len(groups) - 2)
    grp = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    return np.full(len(groups), q, np.int64), grp, np.concatenate(groups), forms


EXACT = [("random", "p1"), ("desc", "p1"), ("third:16384", "p1"), ("plateau", "p1"), ("signs", "p1"),
         ("signs", "m1"), ("random", "zero")]


@pytest.mark.parametrize("table,probe", EXACT, ids=[f"{t}-{p}" for t, p in EXACT])
def test_rank_exact_both_forms(table, probe):
    emb, probes = pu.knn_select_table(table)
    n, d = emb.shape
    q = probes[probe]
    k = min(n, 4096)
    sim, _, ref_ids = pu.knn_select_reference(emb, [q], k)
    t = ru.case_targets(sim[0], q, 1000, zero_row=probes["zero"], seed=n)
    rows_q, grp, tt, forms = _layout(q, t)
    want = ru.rank_reference(sim, np.zeros(len(tt), np.int64), tt)
    if probe == "zero":  # an n-way tie: the rank is the index, the query itself ranks last
        assert np.array_equal(want, tt) and want[0] == n - 1
    rc, got = _capi(torch.from_numpy(np.array(emb)).cuda(), n, d, d, rows_q, grp, tt, forms)
    assert rc == 0
    ru.check_ranks(got, want, rows_q[np.searchsorted(grp, np.arange(len(tt)), "right") - 1], tt)
    ids = _knn_ids(emb, [q], k)
    assert np.array_equal(ids, ref_ids)
    ru.check_ranks_vs_knn(got, np.zeros(len(tt), np.int64), tt, ids)
    assert (got < k).any() and ((got >= k).any() or n <= k)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 16384, 20001, 20003])
def test_rank_sizes_and_group_sizes_in_one_launch(n):
    """The scalar path (n % 4 != 0), the 16-byte path with and without a tail
    of up to 15 columns, and groups of 1, 8, 9, 64 and 65 targets in one launch
    (two queries)."""
    emb, probes = pu.knn_select_table(f"random:{n}")
    d = emb.shape[1]
    qs = [probes["p1"], probes.get("m1", probes["p1"])]
    k = min(n, 4096)
    sim, _, _ = pu.knn_select_reference(emb, qs, k)
    rng = np.random.default_rng(n)
    sizes = [1, 8, 9, 64, 65, 3]
    rows_q = np.array([qs[i % 2] for i in range(len(sizes))], np.int64)
    qrow = np.repeat(np.arange(len(sizes)) % 2, sizes)
    tt = np.concatenate([np.concatenate([[n - 1, 0], rng.integers(0, n, m)])[:m] for m in sizes]).astype(np.int64)
    grp = np.concatenate([[0], np.cumsum(sizes)])
    want = ru.rank_reference(sim, qrow, tt)
    rc, got = _capi(torch.from_numpy(np.array(emb)).cuda(), n, d, d, rows_q, grp, tt,
                    ["few", "few", "sorted", "sorted", "sorted", "few"])
    assert rc == 0
    ru.check_ranks(got, want, np.repeat(rows_q, sizes), tt)
    ru.check_ranks_vs_knn(got, qrow, tt, _knn_ids(emb, qs, k))


def test_rank_group_at_capacity_and_split_above_it():
    """A group of exactly 4096 targets in one row, and 4097 pairs of one query
    through rank_from_emb, which splits them over two rows of the same query."""
    import baselines
    emb, probes = pu.knn_select_table("third:16384")
    n, d = emb.shape
    q = probes["p1"]
    sim, _, _ = pu.knn_select_reference(emb, [q], 1)
    tt = np.random.default_rng(1).integers(0, n, ru.RANK_MAX_GROUP + 1).astype(np.int64)
    want = ru.rank_reference(sim, np.zeros(len(tt), np.int64), tt)
    dev = torch.from_numpy(np.array(emb)).cuda()
    cap = ru.RANK_MAX_GROUP
    rc, got = _capi(dev, n, d, d, [q, q], [0, cap, cap + 1], tt, ["sorted", "few"])
    assert rc == 0
    ru.check_ranks(got, want, np.full(len(tt), q), tt)
    assert baselines.RANK_MAX_GROUP == cap == int(__import__("_native").lib().pinsage_rank_max_group())
    rows_q, grp, _, _ = baselines._group_pairs(torch.full((cap + 1,), q), torch.from_numpy(tt))
    assert rows_q.tolist() == [q, q] and grp.tolist() == [0, cap, cap + 1]
    r = baselines.rank_from_emb(dev, torch.full((cap + 1,), q), torch.from_numpy(tt))
    assert r.is_cuda and r.dtype == torch.int64
    ru.check_ranks(r.cpu().numpy(), want, np.full(len(tt), q), tt)


def _mixed_pairs():
    """Pairs over four queries of the descending table in the caller's (shuffled)
    order: groups of 1, 5, 9 and 40 targets."""
    emb, p = pu.knn_select_table("desc")
    n = emb.shape[0]
    qs = np.array([p["p1"], p["m1"], p["zero"], p["p2"]], np.int64)
    sizes = [1, 5, 9, 40]
    rng = np.random.default_rng(9)
    q = np.repeat(qs, sizes)
    t = rng.integers(0, n, len(q)).astype(np.int64)
    perm = rng.permutation(len(q))
    q, t = q[perm], t[perm]
    sim, _, _ = pu.knn_select_reference(emb, qs, 1)
    qrow = np.searchsorted(np.sort(qs), q)
    want = ru.rank_reference(sim[np.argsort(qs)], qrow, t)
    return emb, q, t, want


@pytest.mark.parametrize("rows", [None, 2, 3])
def test_rank_from_emb_mixed_groups_and_batches(monkeypatch, rows):
    """Groups of very different sizes in one call, pairs in shuffled order, and
    several batches of the four query rows: two of 2 rows (rows = 2), one of 3
    and a short last one (rows = 3)."""
    import baselines
    emb, q, t, want = _mixed_pairs()
    n = emb.shape[0]
    if rows:
        monkeypatch.setattr(baselines, "KNN_SCRATCH_BYTES", 8 * n + rows * 4 * n)
    r = baselines.rank_from_emb(torch.from_numpy(np.array(emb)), torch.from_numpy(q), torch.from_numpy(t))
    assert r.device.type == "cpu" and r.dtype == torch.int64 and r.shape == (len(q),)
    ru.check_ranks(r.numpy(), want, q, t)


def test_rank_strided_table_equals_dense():
    """Rows of stride ld = d + 8 with the padding set to a value that would
    show in any dot product or norm that read it."""
    emb, probes = pu.knn_select_table("desc")
    n, d = emb.shape
    q = probes["p1"]
    sim, _, _ = pu.knn_select_reference(emb, [q], 1)
    t = ru.case_targets(sim[0], q, 1000, zero_row=probes["zero"], seed=2)
    rows_q, grp, tt, forms = _layout(q, t)
    want = ru.rank_reference(sim, np.zeros(len(tt), np.int64), tt)
    dense = torch.from_numpy(np.array(emb)).cuda()
    padded = torch.full((n, d + 8), 7e6, dtype=torch.float32, device="cuda")
    padded[:, :d] = dense
    rc0, r0 = _capi(dense, n, d, d, rows_q, grp, tt, forms)
    rc1, r1 = _capi(padded, n, d, d + 8, rows_q, grp, tt, forms)
    assert rc0 == 0 and rc1 == 0
    ru.check_ranks(r0, want, np.full(len(tt), q), tt)
    ru.check_ranks(r1, r0, np.full(len(tt), q), tt)


@pytest.mark.parametrize("table", ["random", "third:16384"])
def test_rank_both_gemm_arithmetics(table):
    """fp32 MFMA (0) and split bf16 (1) give the same ranks: the dots are exact in both."""
    import _native as nat
    lib = nat.lib()
    emb, probes = pu.knn_select_table(table)
    n, d = emb.shape
    q = probes["p1"]
    sim, _, _ = pu.knn_select_reference(emb, [q], 1)
    t = ru.case_targets(sim[0], q, 1000, zero_row=probes["zero"], seed=3)
    rows_q, grp, tt, forms = _layout(q, t)
    want = ru.rank_reference(sim, np.zeros(len(tt), np.int64), tt)
    dev = torch.from_numpy(np.array(emb)).cuda()
    old = lib.pinsage_gemm_get_prec()
    try:
        for prec in (0, 1):
            assert lib.pinsage_gemm_set_prec(prec) == 0
            rc, got = _capi(dev, n, d, d, rows_q, grp, tt, forms)
            assert rc == 0
            ru.check_ranks(got, want, np.full(len(tt), q), tt)
    finally:
        lib.pinsage_gemm_set_prec(old)


def test_rank_rejections_leave_the_output_untouched():
    import _native as nat
    emb, p = pu.knn_select_table("random:4100")
    n, d = 4100, pu.KNN_D
    big = torch.zeros((5000, d + 8), dtype=torch.float32, device="cuda")
    big[:n, :d] = torch.from_numpy(np.array(emb)).cuda()
    q = p["p1"]
    tt = np.random.default_rng(4).integers(0, n, ru.RANK_MAX_GROUP + 1).astype(np.int64)
    cap = ru.RANK_MAX_GROUP

    def refused(want, n_, d_, ld_, rows_q=(q,), grp=(0, 5), **kw):
        rc, r = _capi(big, n_, d_, ld_, rows_q, grp, tt, **kw)
        assert rc == want, (rc, nat.lib().pinsage_last_error())
        assert (r == SENTINEL).all()

    refused(ERR_ARG, 0, d, d + 8, np_=5)
    refused(ERR_ARG, n, 6, d + 8, np_=5)
    refused(ERR_ARG, n, d, d - 4, np_=5)           # ld < d
    refused(ERR_ARG, n, d, d + 7, np_=5)           # rows that do not start 16-byte aligned
    refused(ERR_ARG, n, d, d + 8, grp=(1, 5), np_=5)                       # grp_ptr not starting at 0
    refused(ERR_ARG, n, d, d + 8, rows_q=(q, q), grp=(0, 5, 3), np_=3)     # decreasing
    refused(ERR_ARG, n, d, d + 8, grp=(0, 5), np_=6)                       # not ending at the pair count
    refused(ERR_ARG, n, d, d + 8, grp=(0, cap + 1), np_=cap + 1)           # a group above the capacity
    refused(ERR_WORKSPACE, n, d, d + 8, np_=5,
            scratch_bytes=int(nat.lib().pinsage_rank_scratch_bytes(n, 1)) - 256, rows=1)
    rc, r = _capi(big, n, d, d + 8, (q,), (0, 5), tt[:5], ["few"])  # and the same call with valid arguments runs
    assert rc == 0
    sim, _, _ = pu.knn_select_reference(emb, [q], 1)
    ru.check_ranks(r, ru.rank_reference(sim, np.zeros(5, np.int64), tt[:5]), np.full(5, q), tt[:5])


def test_rank_from_emb_out_of_range_and_empty():
    import baselines
    emb = torch.from_numpy(np.array(pu.knn_select_table("random:65")[0]))
    with pytest.raises(IndexError):
        baselines.rank_from_emb(emb, torch.tensor([3]), torch.tensor([65]))
    with pytest.raises(IndexError):
        baselines.rank_from_emb(emb, torch.tensor([3]), torch.tensor([-1]))
    with pytest.raises(IndexError):
        baselines.rank_from_emb(emb, torch.tensor([65]), torch.tensor([3]))
    r = baselines.rank_from_emb(emb, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert r.shape == (0,) and r.dtype == torch.int64


def test_rank_float_table_within_the_derived_bracket(monkeypatch):
    """Gaussian 20000 x 130 (d padded to 132), duplicate rows and a zero row, 500
    pairs over 120 distinct queries, several batches.  Keys are not exact here:
    each rank is held to #{sim64 > s_t + KNN_ATOL} <= rank <= #{sim64 >= s_t -
    KNN_ATOL} - 1."""
    import baselines
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((20000, 130), dtype=np.float32)
    emb[100:140] = emb[0:40]
    emb[7] = 0.0
    dq = np.concatenate([np.arange(0, 40), [100, 139], rng.choice(np.arange(200, 20000), 78, replace=False)])
    assert len(np.unique(dq)) == 120
    q = np.concatenate([dq, rng.choice(dq, 380)]).astype(np.int64)
    t = rng.integers(0, 20000, 500).astype(np.int64)
    t[:40] = np.arange(100, 140)   # the duplicate of the query: a tie with the query itself
    t[7] = 7                       # the zero row as query and as its own target: an n-way tie
    t[40] = 7                      # the zero row as a target
    t[41:44] = [0, 7, 39]
    near = baselines.knn_from_emb(torch.from_numpy(emb).cuda(), torch.from_numpy(q[200:300]).cuda(), 30)[1].cpu().numpy()
    t[200:300] = near[np.arange(100), rng.integers(0, 30, 100)]  # positives that rank high, as real ones do
    monkeypatch.setattr(baselines, "KNN_SCRATCH_BYTES", 4 << 20)  # ~50 rows per batch
    r = baselines.rank_from_emb(torch.from_numpy(emb).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda())
    assert r.is_cuda
    uq, qrow = np.unique(q, return_inverse=True)
    ru.check_rank_bracket(r.cpu().numpy(), ru.sims64(emb, uq), qrow, t, pu.KNN_ATOL)


# ----------------------------------------------------------------------------- PinSage.evaluate
N = 3000


def _trainer(tmp, seed=1):
    import graph
    import pinsage_training as pt
    import synthetic
    pg = synthetic.make_playlist_graph(N, 600, 20000, seed=41)
    indptr, indices = pg.csr()
    g = graph.CSRGraph.from_csr(indptr, indices, base_dir=tmp, nbhds_path=os.path.join(tmp, "nb.pt"))
    feats = torch.from_numpy(synthetic.make_features(N, 128, seed=42))
    pos = torch.from_numpy(synthetic.make_positives(pg, 12000, seed=43))
    torch.manual_seed(seed)
    tr = pt.PinSage(g, N, feats, pos, log=False, load_save=False)
    tr.batch_size = 32
    test_pos = torch.from_numpy(synthetic.make_positives(pg, 400, seed=44))[:, :2].contiguous()
    return tr, test_pos


def test_evaluate_equals_the_knn_route_and_leaves_no_trace():
    import baselines
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            tr, tp = _trainer(tmp)
            for training in (True, False):
                tr.model.train(training)
                st = torch.get_rng_state()
                res = tr.evaluate(tp)
                assert torch.equal(torch.get_rng_state(), st)
                assert tr.model.training is training
            assert list(res) == ["hr (k=10)", "hr (k=100)", "hr (k=500)", "mrr"]
            emb = tr.embed()
            assert torch.equal(tr.embeddings, emb)
            _, knn_mat = baselines.knn_from_emb(emb, torch.arange(N), 1000)
            knn_mat = knn_mat.cpu()
            want = {f"hr (k={k})": baselines.hit_rate(knn_mat, tp, k) for k in (10, 100, 500)}
            want["mrr"] = baselines.mrr(knn_mat, tp, 1000, 1)
            n = tp.shape[0]
            exact = all(round(res[c] * n) == round(want[c] * n) for c in want if c != "mrr") and \
                abs(res["mrr"] - want["mrr"]) <= 1e-12
            print("evaluate", res, "knn route", want, "form:", "exact" if exact else "bracket")
            if not exact:
                # the two GEMM launches (120 gathered rows / all rows) may differ in a key's last
                # bit: then every rank is held to the float bracket instead
                r = baselines.rank_from_emb(emb, tp[:, 0], tp[:, 1]).cpu().numpy()
                uq, qrow = np.unique(tp[:, 0].numpy(), return_inverse=True)
                ru.check_rank_bracket(r, ru.sims64(emb.cpu().numpy(), uq), qrow, tp[:, 1].numpy(), pu.KNN_ATOL)
            assert 0.0 <= res["hr (k=10)"] <= res["hr (k=100)"] <= res["hr (k=500)"] <= 1.0
        finally:
            os.chdir(cwd)


def test_evaluate_between_steps_changes_no_step():
    """Two trainers from one seed, the same three batches through train_batch;
    one evaluates after the first.  Their parameters end bitwise equal."""
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            a, tp = _trainer(tmp)
            b, _ = _trainer(tmp)
            # (the first constructor drew the neighbourhood walks before its parameters, the
            # second loaded them: start both from the first one's parameters)
            b.model.load_state_dict({k: v.detach().clone() for k, v in a.model.state_dict().items()})
            assert torch.equal(a.nbhds[1], b.nbhds[1])
            torch.manual_seed(7)
            batches = [a.next_batch()[0].clone() for _ in range(3)]
            for tr, with_eval in ((a, False), (b, True)):
                torch.manual_seed(8)
                for i, batch in enumerate(batches):
                    tr.train_batch(batch.clone())
                    if with_eval and i == 0:
                        tr.evaluate(tp)
                tr._sync_state()
            for (ka, pa), (kb, pb) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
                assert ka == kb and torch.equal(pa.detach().cpu(), pb.detach().cpu()), ka
        finally:
            os.chdir(cwd)
