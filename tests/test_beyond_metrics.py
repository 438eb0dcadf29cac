"""The numpy references of the beyond-accuracy metrics (beyond_util) against
the reference's own results (tests/golden/beyond_accuracy.npz, written by
make_golden_beyond.py from eval.py) -- all on the host.  The GPU tests
(tests/test_gpu_beyond.py) compare the kernels and baselines' functions with
these references and with the same fixture.
"""
import numpy as np
import pytest

import beyond_util as bu
from conftest import golden


@pytest.fixture(scope="module")
def fx():
    d = golden("beyond_accuracy")
    for k in ("knn_mat", "test_positives", "in_degrees"):
        d[k] = d[k].astype(np.int64)
    return d


def _reference_pairs(fx, i):
    """The pairs the reference drew for inter K number i, and the next draw."""
    np.random.seed(int(fx["inter_seeds"][i]))
    pairs = np.random.randint(0, fx["knn_mat"].shape[0], (int(fx["inter_pairs"]), 2))
    return pairs, int(np.random.randint(0, int(fx["next_draw_high"])))


def test_fixture_holds_the_cases_it_was_built_for(fx):
    km = fx["knn_mat"]
    assert km.shape == (400, 60) and fx["features"].shape == (400, 24) and fx["features"].dtype == np.float32
    assert 0.2 < fx["coverage_all"][fx["cov_ks"].tolist().index(10)] < 0.9
    first10 = [len(set(r.tolist())) for r in km[:, :10]]
    assert min(first10) == 9 and first10.count(9) == 1       # one list repeats an id in its first 10 columns
    assert sum(int(q in km[q]) for q in range(400)) >= 1     # one list holds its own query
    assert fx["in_degrees"].min() >= 0 and fx["in_degrees"].max() <= 50
    pairs, nxt = _reference_pairs(fx, 0)
    assert (pairs[:, 0] == pairs[:, 1]).any() and nxt == int(fx["inter_next_draw"][0])


def test_integer_metrics_equal_the_reference_exactly(fx):
    km, tp, deg = fx["knn_mat"], fx["test_positives"], fx["in_degrees"]
    for K, a, p in zip(fx["cov_ks"].tolist(), fx["coverage_all"].tolist(), fx["coverage_positives"].tolist()):
        bu.check_metric("coverage", K, bu.coverage_ref(km, tp, K), a)
        bu.check_metric("coverage of positives", K, bu.coverage_ref(km, tp, K, all_nodes=False), p)
    for K, want in zip(fx["deg_ks"].tolist(), fx["average_degree"].tolist()):
        avg, dist = bu.degrees_ref(km, deg, K)
        bu.check_metric("average degree", K, avg, want)
        bu.check_degree_dist(K, dist, (fx[f"degree_dist_vals_{K}"], fx[f"degree_dist_counts_{K}"]))
        assert dist[1].sum() == 400 * min(K, 60)


def test_inter_by_sets_equals_the_reference(fx):
    """The integers are exact; a handful of float64 roundings remain: 1e-12."""
    for i, (K, want) in enumerate(zip(fx["inter_ks"].tolist(), fx["inter_diversity"].tolist())):
        pairs, _ = _reference_pairs(fx, i)
        bu.check_metric("inter diversity", K, bu.inter_diversity_ref(fx["knn_mat"], K, pairs), want, 1e-12)


def test_intra_matrix_form_within_the_reference_fp32_bound(fx):
    km, f = fx["knn_mat"], fx["features"]
    for K, want in zip(fx["intra_ks"].tolist(), fx["intra_diversity"].tolist()):
        bound = bu.reference_fp32_bound(km, f, K)
        got = bu.intra_diversity_ref(km, f, K)
        print(f"intra K = {K}: float64 {got!r}, reference {want!r}, |diff| {abs(got - want):.3e}, bound {bound:.3e}")
        assert bound < 1e-3
        bu.check_metric("intra diversity", K, got, want, bound)
    assert fx["intra_ks"].tolist()[-2:] == [60, 100]   # K above the list length: the whole list
    assert fx["intra_diversity"][-1] == fx["intra_diversity"][-2]


def test_identity_form_equals_the_matrix_form(fx):
    km, f = fx["knn_mat"], fx["features"]
    for K in (1, 2, 10, 60, 100):
        ident, s, kc = bu.intra_sims_identity(km, f, K)
        assert kc == min(K, 60) and s.shape == (400, 24)
        bu.check_metric("intra similarity, identity form", K, ident, bu.intra_sims_matrix(km, f, K), 1e-13)
    # a zero row: NaN for the queries that list it (the reference's 0 / 0), and only those
    f0 = f.copy()
    z = int(km[3, 2])
    f0[z] = 0.0
    ident, _, _ = bu.intra_sims_identity(km, f0, 10)
    mat = bu.intra_sims_matrix(km, f0, 10)
    lists_it = (km[:, :10] == z).any(1)
    assert lists_it[3] and not lists_it.all()
    assert np.array_equal(np.isnan(ident), lists_it) and np.array_equal(np.isnan(mat), lists_it)
    bu.check_metric("intra similarity with a zero row", 10, ident, mat, 1e-13)


def test_exact_tables_are_exact():
    for d in (1, 3, 4, 12, 130, 1028):
        t = bu.exact_table(50, d, seed=d)
        nz = (t != 0).sum(1)
        assert set(nz.tolist()) <= {1, 4, 16} and (len(set(nz.tolist())) > 1 or d < 4)
        fh = bu.unit_rows(t)
        assert set(np.abs(fh[fh != 0]).tolist()) <= {1.0, 0.5, 0.25}
        knn = np.random.default_rng(d).integers(0, 50, (7, 1000))
        v = bu.exact_intra_values(knn, t, 1000)
        assert v.dtype == np.float32 and (v >= 0).all() and (v <= 1).all()
    same = np.full((1, 9), 4)
    assert bu.exact_intra_values(same, bu.exact_table(50, 12, 1), 9)[0] == 1.0


def test_planted_defects_are_rejected(fx):
    km, tp, deg, f = fx["knn_mat"], fx["test_positives"], fx["in_degrees"], fx["features"]
    K = 10
    want = dict(zip(fx["intra_ks"].tolist(), fx["intra_diversity"].tolist()))[K]
    with pytest.raises(AssertionError, match=r"^intra diversity \(K = 10\): "):   # the diagonal left out
        bu.check_metric("intra diversity", K, bu.intra_diversity_ref(km, f, K, diagonal=False), want,
                        bu.reference_fp32_bound(km, f, K))
    i = fx["inter_ks"].tolist().index(K)
    pairs, _ = _reference_pairs(fx, i)
    with pytest.raises(AssertionError, match=r"^inter diversity \(K = 10\): "):   # a multiset, not a set
        bu.check_metric("inter diversity", K, bu.inter_diversity_ref(km, K, pairs, multiset=True),
                        fx["inter_diversity"][i], 1e-12)
    with pytest.raises(AssertionError, match=r"^coverage \(K = 10\): "):          # column 0 not skipped
        bu.check_metric("coverage", K, bu.coverage_ref(km, tp, K, skip_first=False),
                        fx["coverage_all"][fx["cov_ks"].tolist().index(K)])
    j = fx["deg_ks"].tolist().index(K)
    avg, dist = bu.degrees_ref(km, deg, K, shifted=True)                         # columns 1 .. K
    with pytest.raises(AssertionError, match=r"^average degree \(K = 10\): "):
        bu.check_metric("average degree", K, avg, fx["average_degree"][j])
    with pytest.raises(AssertionError, match=r"^degree_dist counts \(K = 10\): "):
        bu.check_degree_dist(K, dist, (fx["degree_dist_vals_10"], fx["degree_dist_counts_10"]))


def test_forms_and_exports():
    import _native as nat
    for name in ("pinsage_row_inv_norms", "pinsage_list_intra_sim", "pinsage_list_pair_overlap",
                 "pinsage_list_overlap_max_k"):
        assert name in nat.EXPORTED
    assert [bu.overlap_form(k) for k in (1, 64, 65, 4096)] == ["ballot", "ballot", "sorted", "sorted"]
    with pytest.raises(AssertionError):
        bu.overlap_form(4097)
    assert bu.intra_form(12, 12) == "float4" and bu.intra_form(12, 13) == "scalar"
    assert bu.intra_form(130, 132) == "scalar" and bu.intra_form(12, 12, 1) == "scalar"
    import baselines
    assert baselines.LIST_OVERLAP_MAX_K == bu.OV_MAX_K
    for name in ("intra_diversity", "inter_diversity", "coverage", "average_degree", "degree_dist",
                 "beyond_accuracy", "compute_beyond_accuracy_table"):
        assert name in baselines.__all__
