"""Host checks of the Jaccard path's numpy reference (tests/jaccard_util.py)
against the reference's recorded JaccardFast output (tests/golden/jaccard.npz),
and of the host-side pieces of the results table: low_co_accuracy and its rank
form, compute_results_table, LazyKnnDict and Random, against
tests/golden/results_table.npz (the reference on make_golden_eval's inputs,
which eval_metrics.npz holds).

The reference orders equal scores as torch.topk happens to; this package
documents (score descending, id ascending).  So the recorded scores are
compared bit for bit, and the recorded ids only by what does not depend on the
order among ties: distinct, in range, and each listed score is that id's score.
"""
import numpy as np
import pytest
import torch

import jaccard_util as ju
from conftest import golden


@pytest.fixture(scope="module")
def fix():
    f = golden("jaccard")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    member = ju.memberships(n, nc, f["edges"])
    co = ju.counts(member, np.arange(n))
    score = ju.scores(co, ju.degrees(member), np.arange(n))
    return f, member, co, score


def test_reference_counts_and_degrees(fix):
    f, member, co, _ = fix
    assert np.array_equal(ju.degrees(member), f["nbh_sizes"].astype(np.int64))
    assert np.array_equal(co, f["intersect_sizes"].astype(np.int32))
    assert np.array_equal(np.diagonal(co), f["nbh_sizes"])
    # the cases the fixture graph was built to hold
    assert member.sum(1).max() >= 120 and (f["nbh_sizes"] == 0).sum() >= 5
    assert co.max() >= 2 and co.dtype == np.int32


@pytest.mark.parametrize("k", [2, 50])
def test_reference_scores_bit_for_bit(fix, k):
    f, _, _, score = fix
    want_w, want_n = f[f"knn_w_{k}"], f[f"knn_n_{k}"].astype(np.int64)
    got_w, got_n = ju.topk(score, k)
    assert np.array_equal(ju.bits(got_w[:, 1:]), ju.bits(want_w)), "the scores of the top k differ from torch's"
    # the recorded ids, tie order aside; column 0 was dropped, so the lists alone are checked
    ju.check_lists(want_w, want_n, score, f"reference lists, k = {k}")
    ju.check_lists(got_w, got_n, score, f"lexsort lists, k = {k}")
    # among equal scores the lexsort order is by id
    same = ju.bits(got_w[:, 1:]) == ju.bits(got_w[:, :-1])
    assert (got_n[:, 1:][same] > got_n[:, :-1][same]).all()


def test_score_formula_edges():
    deg = np.array([0, 0, 3, 3, 1 << 25], np.int64)
    co = np.array([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 3, 1, 3]], np.int32)
    s = ju.scores(co, deg, [0, 1, 2])
    assert s.dtype == np.float32 and s[0, 0] == 0 and s[0, 1] == 0     # two tracks in no collection score 0
    assert s[2, 2] == 1 and s[2, 3] == np.float32(1) / np.float32(5)
    assert s[2, 4] == np.float32(3) / np.float32(1 << 25)               # the union is rounded to float32
    # the same numbers from torch, as the reference forms them
    it, nb = torch.from_numpy(co), torch.from_numpy(deg.astype(np.int32))
    union = nb[[0, 1, 2]].unsqueeze(1) + nb.unsqueeze(0) - it
    assert np.array_equal(ju.bits((it / (union + 1e-10)).numpy()), ju.bits(s))


# ----------------------------------------------------------------------------- results table
class _Deg:
    def __init__(self, deg):
        self.deg = torch.as_tensor(deg)

    def in_degrees(self, v):
        return self.deg[v]


@pytest.fixture(scope="module")
def inputs():
    e = golden("eval_metrics")
    return (torch.from_numpy(e["knn_mat"].astype(np.int64)), torch.from_numpy(e["test_positives"].astype(np.int64)),
            _Deg(e["in_degrees"].astype(np.int64)), golden("results_table"))


def _close(got, want):
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_low_co_accuracy(inputs):
    import baselines as bl
    km, tp, g, r = inputs
    assert r["low_co_raises"].tolist() == [True, False, False, False]
    for thr, raises, want_mrr, want_hr in zip(r["co_thrs"].tolist(), r["low_co_raises"].tolist(),
                                              r["low_co_mrr_1000"].tolist(), r["low_co_hit_rate_10"].tolist()):
        if raises:  # nothing kept: the reference divides by zero, and so does this
            with pytest.raises(ZeroDivisionError):
                bl.low_co_accuracy(km, g, tp, 1000, co_thr=thr, acc_func=bl.mrr)
            with pytest.raises(ZeroDivisionError):
                bl.low_co_accuracy(km, g, tp, 10, co_thr=thr, acc_func=bl.hit_rate)
            continue
        _close(bl.low_co_accuracy(km, g, tp, 1000, co_thr=thr, acc_func=bl.mrr), want_mrr)
        assert bl.low_co_accuracy(km, g, tp, 10, co_thr=thr, acc_func=bl.hit_rate) == want_hr


def test_low_co_accuracy_from_ranks(inputs):
    import baselines as bl
    km, tp, g, r = inputs
    # the rank of a pair over this matrix: its 1-based column, or past the list if absent
    # (rank 0 is the column a kNN list drops; no pair sits there)
    eq = km[tp[:, 0]] == tp[:, 1:2]
    ranks = torch.where(eq.any(1), eq.to(torch.int8).argmax(1) + 1, km.shape[1] + 5)
    width = int(km.shape[1])
    for thr, raises, want_mrr, want_hr in zip(r["co_thrs"].tolist(), r["low_co_raises"].tolist(),
                                              r["low_co_mrr_1000"].tolist(), r["low_co_hit_rate_10"].tolist()):
        if raises:
            with pytest.raises(ZeroDivisionError):
                bl.low_co_accuracy_from_ranks(ranks, tp, 1000, thr, lambda x, K: bl.mrr_from_ranks(x, K, list_len=width))
            continue
        _close(bl.low_co_accuracy_from_ranks(ranks, tp, 1000, thr,
                                             lambda x, K: bl.mrr_from_ranks(x, K, list_len=width)), want_mrr)
        assert bl.low_co_accuracy_from_ranks(ranks, tp, 10, thr,
                                             lambda x, K: bl.hit_rate_from_ranks(x, K, list_len=width),
                                             n_nodes=int(km.shape[0])) == want_hr
    # n_nodes defaults to one more than the largest id of the pairs
    few = torch.tensor([[3, 4], [3, 9], [7, 1]])
    assert bl.low_co_accuracy_from_ranks(torch.tensor([1, 5, 2]), few, 10, 1, bl.hit_rate_from_ranks) == 1.0
    assert bl.low_co_accuracy_from_ranks(torch.tensor([1, 5, 2]), few, 10, 1,
                                         lambda x, K: float(x.numel())) == 1.0


class _Dict(dict):
    times = {"first": (1.5, 0.25, 3.0), "second": (0, 0, 0)}

    def get_times(self, name):
        return self.times[name]


COLUMNS = ["hr (k=10)", "hr (k=100)", "hr (k=500)", "mrr", "low-degree accuracy", "low-co accuracy", "t (train)",
           "t (emb)", "t (knn)"]


def test_compute_results_table(inputs):
    import baselines as bl
    km, tp, g, r = inputs
    models = _Dict(first=(None, km), second=(None, km.flip(1)))
    table = bl.compute_results_table(models, tp, g, times=True, degree_thr=1)
    assert list(table.columns) == COLUMNS == r["table_columns"].tolist()
    assert list(table.index) == r["table_index"].tolist() == ["first", "second"]
    got, want = table.to_numpy(dtype=np.float64), r["table_values"]
    assert np.array_equal(got[:, :3], want[:, :3]), "hit rates"
    assert np.array_equal(got[:, 6:], want[:, 6:]), "times"
    assert (np.abs(got[:, 3:6] - want[:, 3:6]) <= 1e-12 * np.abs(want[:, 3:6])).all(), "mrr columns"
    bare = bl.compute_results_table(models, tp, g, times=False, degree_thr=0)
    assert list(bare.columns) == COLUMNS[:6] == r["table_no_times_columns"].tolist()
    got, want = bare.to_numpy(dtype=np.float64), r["table_no_times_values"]
    assert np.array_equal(got[:, :3], want[:, :3])
    assert (np.abs(got[:, 3:] - want[:, 3:]) <= 1e-12 * np.abs(want[:, 3:])).all()


class _StubModel:
    """knn: ids (q + 1 + column) % n, weights column + q / 1000."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def knn(self, nodeset, k):
        self.calls.append(len(nodeset))
        cols = torch.arange(k, dtype=torch.int64)
        return (cols.to(torch.float32) + nodeset[:, None] / 1000.0), (nodeset[:, None] + 1 + cols) % self.n


def test_lazy_knn_dict_round_trip(tmp_path):
    import baselines as bl
    n = 23
    ids = list(range(n))
    stub = _StubModel(n)
    bl.save_knn(stub, "stub", ids, str(tmp_path), train_time=2.5, emb_time=0.5, b_size=10)
    assert stub.calls == [10, 10, 3]
    torch.save((torch.zeros(n, 4), torch.ones(n, 4, dtype=torch.int32), 0.0), tmp_path / "knn" / "old.pt")
    d = bl.LazyKnnDict(["stub", "old"], ids, str(tmp_path))
    assert len(d) == 2 and list(d) == ["stub", "old"] and list(d) == ["stub", "old"]
    w, nb = d["stub"]
    assert nb.dtype == torch.int64 and tuple(nb.shape) == (n, bl.PRECOMP_K)
    want_w, want_n = _StubModel(n).knn(torch.arange(n), bl.PRECOMP_K)
    assert torch.equal(nb, want_n) and torch.equal(w, want_w)
    tt, te, tk = d.get_times("stub")
    assert (tt, te) == (2.5, 0.5) and tk >= 0
    assert d.get_times("stub") == (tt, te, tk)
    assert d["old"][1].dtype == torch.int64                  # the ids come back as int64
    assert tuple(d.get_times("old")) == (0, 0, 0)            # a three-field file has no times


def test_random_knn_follows_torch_randperm():
    import baselines as bl
    n, k, nq = 57, 9, 5
    model = bl.Random()
    model.train(None, list(range(n)), None, None, None)
    torch.manual_seed(1234)
    w, nb = model.knn(torch.arange(nq), k)
    after = torch.randint(0, 1 << 30, (1,)).item()
    torch.manual_seed(1234)
    want = torch.stack([torch.randperm(n)[0:k] for _ in range(nq)], dim=0)
    assert torch.randint(0, 1 << 30, (1,)).item() == after   # the generator is left where the reference leaves it
    assert torch.equal(nb, want) and nb.dtype == torch.int64
    assert torch.equal(w, torch.ones_like(want)) and tuple(w.shape) == (nq, k)


def test_exports():
    import _native as nat
    import baselines as bl
    for name in ("pinsage_cooc_tile", "pinsage_cooc_scratch_bytes", "pinsage_cooc_counts", "pinsage_cooc_jaccard"):
        assert name in nat.EXPORTED
    for name in ("JaccardFast", "Random", "low_co_accuracy", "low_co_accuracy_from_ranks", "LazyKnnDict",
                 "compute_results_table"):
        assert name in bl.__all__
    L = nat.lib()
    tile = int(L.pinsage_cooc_tile())
    assert tile >= 1024 and tile % 4 == 0 and tile * 4 <= 64 * 1024   # two workgroups' tiles fit one CU's LDS
    n = 1000
    assert L.pinsage_cooc_scratch_bytes(n, 3) >= 3 * n * 4 + n * 4
    assert L.pinsage_cooc_scratch_bytes(n, 0) == L.pinsage_cooc_scratch_bytes(n, 1)
