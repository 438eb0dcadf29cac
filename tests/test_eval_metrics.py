"""The accuracy metrics (baselines.hit_rate / mrr / low_degree_accuracy and
their rank forms) against the reference's own results
(tests/golden/eval_metrics.npz, written by make_golden_eval.py from eval.py),
the pair grouping of baselines.rank_from_emb, and the numpy rank reference the
GPU tests compare with (rank_util) -- all on the host.
"""
import numpy as np
import pytest
import torch

import parity_util as pu
import rank_util as ru
from conftest import golden


@pytest.fixture(scope="module")
def fx():
    d = golden("eval_metrics")
    d["knn_mat"] = torch.from_numpy(d["knn_mat"].astype(np.int64))
    d["test_positives"] = torch.from_numpy(d["test_positives"].astype(np.int64))
    d["in_degrees"] = torch.from_numpy(d["in_degrees"].astype(np.int64))
    return d


class _DegreeGraph:
    def __init__(self, deg):
        self.deg = deg

    def in_degrees(self, v):
        return self.deg[v]


def _ranks_from_matrix(knn_mat, tp, absent):
    """What rank_from_emb gives for a list_len-wide knn_from_emb matrix: the
    1-based column of the positive, `absent` where the row does not hold it."""
    km, tp = knn_mat.numpy(), tp.numpy()
    out = np.full(len(tp), absent, np.int64)
    for i, (q, p) in enumerate(tp):
        at = np.flatnonzero(km[q] == p)
        if len(at):
            out[i] = at[0] + 1
    return out


def test_fixture_holds_the_cases_it_was_built_for(fx):
    km, tp = fx["knn_mat"], fx["test_positives"]
    assert km.shape == (400, 60) and tp.shape == (300, 2)
    r = _ranks_from_matrix(km, tp, 0)
    for col in (0, 1, 9, 10, 59):  # column 0; K - 1 and K for K = 1, 10, 60
        assert (r == col + 1).sum() >= 4
    same = (tp[:, 0] == tp[:, 1]).numpy()
    assert (r == 0).sum() >= 30 and (same & (r == 0)).sum() >= 6 and (same & (r > 0)).sum() == 1
    assert len(np.unique(tp.numpy(), axis=0)) < len(tp)  # a repeated pair


def test_matrix_forms_equal_the_reference(fx):
    import baselines
    km, tp, n = fx["knn_mat"], fx["test_positives"], 300
    for K, want in zip(fx["hr_ks"].tolist(), fx["hit_rate"].tolist()):
        got = baselines.hit_rate(km, tp, K)
        assert round(got * n) == round(want * n) and abs(got - want) <= 1e-12, K
    for K, row in zip(fx["mrr_ks"].tolist(), fx["mrr"]):
        for s, want in zip(fx["mrr_scalings"].tolist(), row.tolist()):
            assert abs(baselines.mrr(km, tp, K, s) - want) <= 1e-12, (K, s)
    assert abs(baselines.mrr(km, tp, 60) - fx["mrr"][1, 0]) <= 1e-12  # scaling defaults to 1
    # numpy inputs, as load_knn's consumers may hold them
    assert baselines.hit_rate(km.numpy(), tp.numpy(), 10) == baselines.hit_rate(km, tp, 10)


@pytest.mark.parametrize("absent", [61, 1000, 0])
def test_rank_forms_equal_the_matrix_forms(fx, absent):
    """Ranks derived from the same matrix, 'absent' taken as list_len + 1, as a
    far rank, and as rank 0 (the column knn_from_emb drops)."""
    import baselines
    km, tp = fx["knn_mat"], fx["test_positives"]
    r = torch.from_numpy(_ranks_from_matrix(km, tp, absent))
    for K in (1, 10, 60, 61, 100, 1000):  # K > list_len: the whole list
        assert baselines.hit_rate_from_ranks(r, K, list_len=60) == baselines.hit_rate(km, tp, K), K
        for s in (1, 10):
            assert abs(baselines.mrr_from_ranks(r, K, s, list_len=60) - baselines.mrr(km, tp, K, s)) <= 1e-12, (K, s)
    for K, want in zip(fx["hr_ks"].tolist(), fx["hit_rate"].tolist()):
        assert abs(baselines.hit_rate_from_ranks(r, K, list_len=60) - want) <= 1e-12
    # the default list_len is PRECOMP_K: a rank of 61 is then a hit at K = 100
    assert baselines.hit_rate_from_ranks(torch.tensor([61, 0, 1001, 1000]), 1000) == 0.5
    assert baselines.hit_rate_from_ranks(torch.tensor([61, 0, 1001, 1000]), 100) == 0.25
    assert abs(baselines.mrr_from_ranks(torch.tensor([2, 0]), 10, scaling=10) - (10 / 2 + 10 / 10) / 2) <= 1e-12


def test_low_degree_accuracy_both_forms(fx):
    import baselines
    km, tp = fx["knn_mat"], fx["test_positives"]
    g = _DegreeGraph(fx["in_degrees"])
    r = torch.from_numpy(_ranks_from_matrix(km, tp, 61))
    for t, want_m, want_h in zip(fx["low_degree_thrs"].tolist(), fx["low_degree_mrr_1000"].tolist(),
                                 fx["low_degree_hit_rate_10"].tolist()):
        assert abs(baselines.low_degree_accuracy(km, g, tp, 1000, t, baselines.mrr) - want_m) <= 1e-12, t
        assert abs(baselines.low_degree_accuracy(km, g, tp, 10, t, baselines.hit_rate) - want_h) <= 1e-12, t
        mrr60 = lambda rr, K: baselines.mrr_from_ranks(rr, K, list_len=60)            # noqa: E731
        hr60 = lambda rr, K: baselines.hit_rate_from_ranks(rr, K, list_len=60)        # noqa: E731
        assert abs(baselines.low_degree_accuracy_from_ranks(r, g, tp, 1000, t, mrr60, n_nodes=400) - want_m) <= 1e-12
        assert abs(baselines.low_degree_accuracy_from_ranks(r, g, tp, 10, t, hr60, n_nodes=400) - want_h) <= 1e-12
    assert fx["low_degree_thrs"][0] == -1 and baselines.low_degree_accuracy(km, g, tp, 10, -1, baselines.hit_rate) == 0


def test_low_degree_accuracy_on_a_csr_graph():
    """The degree mask from graph.CSRGraph's in-degrees."""
    import baselines
    import graph
    # edges 0->1, 0->2, 1->2, 3->2: in-degrees 0, 1, 3, 0
    g = graph.CSRGraph.from_csr(np.array([0, 2, 3, 3, 4]), np.array([1, 2, 2, 2]))
    assert g.in_degrees(torch.arange(4)).tolist() == [0, 1, 3, 0]
    km = torch.tensor([[1, 2], [0, 2], [3, 1], [2, 0]])
    tp = torch.tensor([[0, 2], [1, 2], [2, 3], [3, 0], [2, 0]])
    # thr 1 keeps the pairs of queries 0, 1 and 3, all in column 1: no hit at K = 1, all at K = 2
    assert baselines.low_degree_accuracy(km, g, tp, 1, 1, baselines.hit_rate) == 0.0
    assert baselines.low_degree_accuracy(km, g, tp, 2, 1, baselines.hit_rate) == 1.0
    assert baselines.low_degree_accuracy(km, g, tp, 2, 0, baselines.hit_rate) == 1.0   # queries 0 and 3
    r = torch.tensor([2, 2, 1, 2, 0])
    hr2 = lambda rr, K: baselines.hit_rate_from_ranks(rr, K, list_len=2)  # noqa: E731
    assert baselines.low_degree_accuracy_from_ranks(r, g, tp, 1, 1, hr2) == 0.0
    assert baselines.low_degree_accuracy_from_ranks(r, g, tp, 2, 1, hr2) == 1.0


# ----------------------------------------------------------------------------- grouping
def _check_grouping(q, t, cap):
    import baselines
    q, t = torch.as_tensor(q, dtype=torch.int64), torch.as_tensor(t, dtype=torch.int64)
    rows, grp, ts, order = baselines._group_pairs(q, t)
    sizes = np.diff(grp.numpy())
    assert grp.dtype == torch.int64 and grp.device.type == "cpu" and grp[0] == 0 and grp[-1] == len(q)
    assert len(rows) == len(sizes) and (sizes >= 1).all() and (sizes <= cap).all()
    assert sorted(order.tolist()) == list(range(len(q)))
    assert torch.equal(ts, t[order])
    assert torch.equal(torch.repeat_interleave(rows, torch.from_numpy(sizes)), q[order])  # each row owns its query's pairs
    assert (np.diff(rows.numpy()) >= 0).all()
    # stable: the pairs of one query keep the caller's order
    o, qq = order.numpy(), q[order].numpy()
    assert all(o[i] < o[i + 1] for i in range(len(o) - 1) if qq[i] == qq[i + 1])
    # a query's rows are full but for its last
    for u in np.unique(q.numpy()):
        s = sizes[rows.numpy() == u]
        assert (s[:-1] == cap).all() and s.sum() == int((q == u).sum())
    # the inverse permutation restores the caller's order: "rank" each sorted pair by its own target
    out = torch.empty_like(ts)
    out[order] = ts * 10
    assert torch.equal(out, t * 10)
    return rows, sizes


def test_group_pairs(monkeypatch):
    import baselines
    monkeypatch.setattr(baselines, "RANK_MAX_GROUP", 4)
    rng = np.random.default_rng(0)
    # groups of 1, capacity, capacity + 1 and 2 * capacity + 1, in shuffled order
    q = np.repeat([7, 3, 11, 5], [1, 4, 5, 9])
    t = rng.integers(0, 100, len(q))
    perm = rng.permutation(len(q))
    rows, sizes = _check_grouping(q[perm], t[perm], 4)
    assert rows.tolist() == [3, 5, 5, 5, 7, 11, 11] and sizes.tolist() == [4, 4, 4, 1, 1, 4, 1]
    rows, sizes = _check_grouping([], [], 4)                       # empty input
    assert rows.tolist() == [] and sizes.tolist() == []
    rows, sizes = _check_grouping([2] * 10, np.arange(10), 4)      # one query for all pairs
    assert rows.tolist() == [2, 2, 2] and sizes.tolist() == [4, 4, 2]
    rows, sizes = _check_grouping([9, 1, 5, 3], [0, 1, 2, 3], 4)   # all queries distinct
    assert rows.tolist() == [1, 3, 5, 9] and sizes.tolist() == [1, 1, 1, 1]
    monkeypatch.undo()
    assert baselines.RANK_MAX_GROUP == ru.RANK_MAX_GROUP == 4096
    rows, sizes = _check_grouping(np.zeros(4097, np.int64), np.arange(4097), 4096)
    assert sizes.tolist() == [4096, 1]


# ----------------------------------------------------------------------------- the rank reference
RANK_TABLES = [("third:16384", "p1"), ("random", "zero"), ("signs", "p1"), ("signs", "m1"), ("desc:20001", "p1"),
               ("random:1", "p1")]


@pytest.mark.parametrize("table,probe", RANK_TABLES, ids=[f"{t}-{p}" for t, p in RANK_TABLES])
def test_rank_reference_is_the_position_in_the_knn_order(table, probe):
    """For every row as target: the rank is its position in the full
    (similarity descending, index ascending) order of knn_select_reference,
    so ids[rank] == target wherever rank < k."""
    emb, probes = pu.knn_select_table(table)
    n = emb.shape[0]
    sim, _, ids = pu.knn_select_reference(emb, [probes[probe]], n)
    targets = np.arange(n)
    r = ru.rank_reference(sim, np.zeros(n, np.int64), targets) if n <= 4096 else None
    position = np.empty(n, np.int64)
    position[ids[0]] = np.arange(n)
    if r is None:  # every row, without n passes: the same definition by sorting
        key = pu.knn_key_image(sim[0]).astype(np.int64)
        order = np.lexsort((targets, -key))
        r = np.empty(n, np.int64)
        r[order] = np.arange(n)
        some = np.concatenate([[0, n - 1, probes[probe]], np.random.default_rng(1).integers(0, n, 60)])
        assert np.array_equal(ru.rank_reference(sim, np.zeros(len(some), np.int64), some), r[some])
    assert np.array_equal(r, position)
    ru.check_ranks_vs_knn(r, np.zeros(n, np.int64), targets, ids[:, :min(n, 1000)])
    ru.check_ranks(r, position, np.full(n, probes[probe]), targets)


def test_rank_checks_reject_planted_defects():
    emb, probes = pu.knn_select_table("signs")
    q = probes["p1"]
    sim, _, ids = pu.knn_select_reference(emb, [q], 1000)
    t = ru.case_targets(sim[0], q, 1000, zero_row=probes["zero"], seed=1)
    qrow = np.zeros(len(t), np.int64)
    want = ru.rank_reference(sim, qrow, t)
    qq = np.full(len(t), q)
    ru.check_ranks(want.copy(), want, qq, t)
    first = rf"^rank \(query {q}, target {int(t[0])}\), pair 0: "
    for kw in (dict(tie="le"), dict(count_self=True)):  # both count the target's own row: + 1 on every pair
        bad = ru.rank_reference(sim, qrow, t, **kw)
        assert np.array_equal(bad, want + 1)
        with pytest.raises(AssertionError, match=first + rf"got {int(want[0]) + 1}, reference {int(want[0])}; {len(t)} of {len(t)}"):
            ru.check_ranks(bad, want, qq, t)
    # without the sign flip the negative similarities order backwards, and above the small positive ones
    bad = ru.rank_reference(sim, qrow, t, key_image=ru.key_image_no_flip)
    assert (sim[0][t] < 0).any() and (bad != want).any()
    i = int(np.flatnonzero(bad != want)[0])
    with pytest.raises(AssertionError, match=rf"^rank \(query {q}, target {int(t[i])}\), pair {i}: "):
        ru.check_ranks(bad, want, qq, t)
    # the kNN-column check and the bracket reject a shifted rank as well
    with pytest.raises(AssertionError, match=rf"^rank pair 1 \(query row 0, target {int(t[1])}\)"):
        ru.check_ranks_vs_knn(np.where(np.arange(len(t)) == 1, want + 1, want), qrow, t, ids)
    s64 = sim.astype(np.float64)
    ru.check_rank_bracket(want, s64, qrow, t, 0.0)
    with pytest.raises(AssertionError, match=r"^rank pair \d+ \(query row 0, target \d+\): rank \d+ outside \["):
        ru.check_rank_bracket(want + 1, s64, qrow, t, 0.0)
    with pytest.raises(AssertionError, match="^rank: shapes"):
        ru.check_ranks(want[:-1], want, qq, t)
    assert [ru.rank_form(m) for m in (0, 1, 8, 9, 4096)] == ["empty", "few", "few", "sorted", "sorted"]
    with pytest.raises(AssertionError):
        ru.rank_form(4097)
