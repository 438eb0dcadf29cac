"""The kernels of csrc/listmetrics.hip (pinsage_row_inv_norms,
pinsage_list_intra_sim, pinsage_list_pair_overlap) and what stands on them:
baselines.intra_diversity / inter_diversity / coverage / average_degree /
degree_dist / beyond_accuracy and PinSage.evaluate_beyond_accuracy.

The intra-list similarity is compared bit for bit on tables whose rows have 1,
4 or 16 non-zeros of one magnitude 2^e (beyond_util.exact_table: every norm a
power of two, every sum and square exact in fp32), and within a derived
componentwise bound on Gaussian tables (beyond_util.device_intra_bound).  The
pair overlaps are integers, compared with Python sets.  Each launch asserts,
before it runs, the form beyond_util predicts for it, and every output is
pre-filled with a sentinel so that an unwritten or overwritten value shows.
The numpy references are checked on the host in tests/test_beyond_metrics.py.
"""
import os
import tempfile

import numpy as np
import pytest
import torch

import beyond_util as bu
import parity_util as pu
from conftest import golden

pytestmark = pytest.mark.gpu

ERR_ARG = -2       # pinsage_status (include/pinsage_hip.h)
SENT_F = -123.0
SENT_I = -7
N_ROWS = 97        # table rows of the kernel tests
PAD = 8            # sentinel values behind every output


# ----------------------------------------------------------------------------- launch helpers
def _place(table, layout):
    """The table on the device as (tensor whose data_ptr is row 0, ld, offset in
    floats from a 16-byte boundary): dense; ld = d + 4 / d + 1 with NaN in the
    padding; or dense behind a pointer offset by one float."""
    n, d = table.shape
    t = torch.from_numpy(np.ascontiguousarray(table))
    if layout == "dense":
        return t.cuda(), d, 0
    if layout in ("pad4", "pad1"):
        ld = d + (4 if layout == "pad4" else 1)
        p = torch.full((n, ld), float("nan"), dtype=torch.float32, device="cuda")
        p[:, :d] = t.cuda()
        return p, ld, 0
    assert layout == "offset1"
    buf = torch.full((n * d + 1,), float("nan"), dtype=torch.float32, device="cuda")
    buf[1:] = t.cuda().reshape(-1)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    return view, d, 1


def _inv_norms(dev, n, d, ld):
    import _native as nat
    inv = torch.full((n + PAD,), SENT_F, dtype=torch.float32, device="cuda")
    rc = nat.lib().pinsage_row_inv_norms(nat.ptr(dev), n, d, ld, nat.ptr(inv), nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, inv


def _intra(dev, n, d, ld, inv, lists, kc, form=None, offset=0):
    """pinsage_list_intra_sim over lists (numpy int64 [nq, ldk]) with a
    sentinel-filled output: (status, values [nq], error word)."""
    import _native as nat
    if form is not None:
        assert bu.intra_form(d, ld, offset) == form, (d, ld, offset, form)
    ld_ = torch.from_numpy(np.ascontiguousarray(lists, np.int64)).cuda()
    nq, ldk = lists.shape
    out = torch.full((nq + PAD,), SENT_F, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = nat.lib().pinsage_list_intra_sim(nat.ptr(dev), n, d, ld, nat.ptr(inv), nat.ptr(ld_), nq, ldk, kc,
                                          nat.ptr(out), nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[nq:] == SENT_F).all(), "values behind the nq outputs were written"
    return rc, o[:nq], int(err)


def _lists(nq, kc, seed, extra=2, n=N_ROWS):
    """Seeded ids [nq, kc + extra]; the unused columns hold ids that would change the result."""
    rng = np.random.default_rng(seed)
    lists = rng.integers(0, n, (nq, kc + extra)).astype(np.int64)
    lists[:, kc:] = (lists[:, :1] + 1 + rng.integers(0, n - 1, (nq, extra))) % n
    return lists


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_exact(table, layout, lists, kc, form):
    dev, ld, off = _place(table, layout)
    n, d = table.shape
    rc, inv = _inv_norms(dev, n, d, ld)
    assert rc == 0
    invh = inv.cpu().numpy()
    with np.errstate(divide="ignore"):
        want_inv = (1.0 / np.sqrt((table.astype(np.float64) ** 2).sum(1))).astype(np.float32)
    assert np.array_equal(_bits(invh[:n]), _bits(want_inv)), f"inverse norms, d = {d}, {layout}"
    assert (invh[n:] == SENT_F).all()
    rc, got, err = _intra(dev, n, d, ld, inv, lists, kc, form, off)
    assert rc == 0 and err == 0
    want = bu.exact_intra_values(lists, table, kc)
    bad = _bits(got) != _bits(want)
    bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (f"intra similarity d = {d}, kc = {kc}, {layout}: query {int(np.flatnonzero(bad)[0])} "
                           f"got {got[bad][0]!r}, reference {want[bad][0]!r}; {int(bad.sum())} of {bad.size} differ")
    return got


# ----------------------------------------------------------------------------- intra: exact
# 516 = the float4 form's second column pass (LM_PASS_VEC + 4); 130 and 260 the scalar form's
# second and third (LM_PASS_SCALAR = 128) when the layout forces it
DIMS = [1, 3, 4, 12, 130, 256, 260, 512, 516, 1024, 1028]


@pytest.mark.parametrize("d", DIMS)
def test_intra_exact_over_d_and_layouts(d):
    assert bu.LM_PASS_VEC + 4 in DIMS and bu.LM_PASS_VEC in DIMS
    table = bu.exact_table(N_ROWS, d, seed=d)
    kc = 2 * bu.LM_ROWS + 3
    lists = _lists(9, kc, seed=d)
    vec = "float4" if d % 4 == 0 else "scalar"
    a = _check_exact(table, "dense", lists, kc, vec)
    b = _check_exact(table, "pad4", lists, kc, vec)
    c = _check_exact(table, "pad1", lists, kc, "scalar")
    e = _check_exact(table, "offset1", lists, kc, "scalar")
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, e)


R = bu.LM_ROWS
KCS = [1, 2, R - 1, R, R + 1, 2 * R + 1, bu.LM_CHUNK - 1, bu.LM_CHUNK, bu.LM_CHUNK + 1, 100, 1000]


@pytest.mark.parametrize("kc", KCS)
def test_intra_exact_over_kc(kc):
    for d, layout, form in ((260, "dense", "float4"), (3, "dense", "scalar"), (130, "pad1", "scalar")):
        _check_exact(bu.exact_table(N_ROWS, d, seed=kc + d), layout, _lists(6, kc, seed=kc), kc, form)


W = bu.LM_WAVES


@pytest.mark.parametrize("nq", [1, W - 1, W, W + 1, 1000])
def test_intra_exact_over_nq(nq):
    _check_exact(bu.exact_table(N_ROWS, 12, seed=nq), "dense", _lists(nq, 9, seed=nq), 9, "float4")
    _check_exact(bu.exact_table(N_ROWS, 5, seed=nq), "dense", _lists(nq, 9, seed=nq), 9, "scalar")


@pytest.mark.parametrize("d,layout,form", [(16, "dense", "float4"), (16, "pad1", "scalar"), (520, "dense", "float4")])
def test_intra_special_lists(d, layout, form):
    """All ids equal: exactly 1.  A row and its negation: exactly 0.  A zero
    row: NaN, the other queries of its workgroup unaffected."""
    table = bu.exact_table(N_ROWS, d, seed=3, zero_row=40)
    table[11] = -table[10]
    kc = 10
    lists = _lists(2 * W + 1, kc, seed=5)
    lists[lists == 40] = 41
    lists[0, :kc] = 17
    lists[1, :kc] = [10, 11] * 5
    lists[2, :kc] = [10] * 5 + [11] * 5
    lists[W + 1, 3] = 40            # the zero row, in the second workgroup
    lists[W + 2, kc] = 40           # ... in an unused column: not read
    got = _check_exact(table, layout, lists, kc, form)
    assert got[0] == 1.0 and got[1] == 0.0 and got[2] == 0.0
    assert np.array_equal(np.isnan(got), np.arange(len(lists)) == W + 1)
    dev, ld, off = _place(table, layout)
    _, inv = _inv_norms(dev, N_ROWS, d, ld)
    assert np.isposinf(inv.cpu().numpy()[40])
    rc, two, _ = _intra(dev, N_ROWS, d, ld, inv, lists[1:2], 2, form, off)   # kc = 2: one row and its negation
    assert rc == 0 and two[0] == 0.0


def test_intra_id_out_of_range_sets_the_error_word():
    import baselines
    table = bu.exact_table(N_ROWS, 12, seed=1)
    dev, ld, off = _place(table, "dense")
    _, inv = _inv_norms(dev, N_ROWS, 12, ld)
    lists = _lists(5, 9, seed=1)
    for bad in (N_ROWS, -1, 2 ** 40):
        wrong = lists.copy()
        wrong[3, 4] = bad
        rc, got, err = _intra(dev, N_ROWS, 12, ld, inv, wrong, 9, "float4")
        assert rc == 0 and err == 1
        clamped = wrong.copy()
        clamped[3, 4] = 0
        assert np.array_equal(_bits(got), _bits(bu.exact_intra_values(clamped, table, 9)))
        with pytest.raises(IndexError):
            baselines.intra_diversity(wrong, None, 9, table)
    wrong = lists.copy()
    wrong[3, 9] = N_ROWS    # an unused column is not read: no error
    rc, got, err = _intra(dev, N_ROWS, 12, ld, inv, wrong, 9, "float4")
    assert rc == 0 and err == 0


def test_intra_refusals_leave_the_outputs_untouched():
    import _native as nat
    table = bu.exact_table(N_ROWS, 12, seed=1)
    dev, ld, _ = _place(table, "pad4")
    _, inv = _inv_norms(dev, N_ROWS, 12, ld)
    lists = _lists(5, 9, seed=1)
    for kw in (dict(kc=0), dict(kc=-3), dict(kc=12), dict(ld=8), dict(d=0), dict(n=0)):
        a = dict(n=N_ROWS, d=12, ld=ld, kc=9)
        a.update(kw)
        rc, got, err = _intra(dev, a["n"], a["d"], a["ld"], inv, lists, a["kc"])
        assert rc == ERR_ARG and (got == SENT_F).all() and err == 0, kw
    L = nat.lib()
    ld_ = torch.from_numpy(lists).cuda()
    out = torch.full((5,), SENT_F, dtype=torch.float32, device="cuda")
    args = [nat.ptr(dev), N_ROWS, 12, ld, nat.ptr(inv), nat.ptr(ld_), 5, 11, 9, nat.ptr(out), None, nat.stream_ptr()]
    for null_at in (0, 4, 5, 9):
        a = list(args)
        a[null_at] = None
        assert L.pinsage_list_intra_sim(*a) == ERR_ARG, null_at
    torch.cuda.synchronize()
    assert (out == SENT_F).all()
    assert L.pinsage_list_intra_sim(*args) == 0     # the same call with valid arguments (err may be null) runs
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(bu.exact_intra_values(lists, table, 9)))
    inv2 = torch.full((N_ROWS,), SENT_F, dtype=torch.float32, device="cuda")
    for a in ([None, N_ROWS, 12, ld, nat.ptr(inv2)], [nat.ptr(dev), N_ROWS, 12, ld, None],
              [nat.ptr(dev), N_ROWS, 12, 8, nat.ptr(inv2)], [nat.ptr(dev), N_ROWS, 0, ld, nat.ptr(inv2)]):
        assert L.pinsage_row_inv_norms(*a, nat.stream_ptr()) == ERR_ARG
    torch.cuda.synchronize()
    assert (inv2 == SENT_F).all()


# ----------------------------------------------------------------------------- intra: random
def _gauss_table(d, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((N_ROWS, d)).astype(np.float32)
    return t * (2.0 ** rng.integers(-20, 20, (N_ROWS, 1))).astype(np.float32)


RANDOM = [(d, 2 * R + 3, 9) for d in DIMS] + [(260, kc, 6) for kc in KCS] + [(3, kc, 6) for kc in KCS] + \
         [(12, 9, nq) for nq in (1, W - 1, W, W + 1, 1000)]


def test_intra_random_within_the_derived_bound_and_reproducible():
    worst = 0.0
    for d, kc, nq in RANDOM:
        table = _gauss_table(d, seed=d + kc)
        lists = _lists(nq, kc, seed=d + kc + nq)
        for layout in ("dense", "pad1"):
            dev, ld, off = _place(table, layout)
            rc, inv = _inv_norms(dev, N_ROWS, d, ld)
            assert rc == 0
            rc, got, err = _intra(dev, N_ROWS, d, ld, inv, lists, kc, None, off)
            rc2, again, _ = _intra(dev, N_ROWS, d, ld, inv, lists, kc, None, off)
            assert rc == 0 and rc2 == 0 and err == 0
            assert np.array_equal(_bits(got), _bits(again)), (d, kc, nq, layout)
            want, s, kc_ = bu.intra_sims_identity(lists, table, kc)
            bound = bu.device_intra_bound(s, kc_, lists, table, kc)
            ratio = float((np.abs(got.astype(np.float64) - want) / bound).max())
            worst = max(worst, ratio)
            bu.check_metric(f"intra similarity (d = {d}, nq = {nq}, {layout})", kc, got, want, bound)
    print(f"list_intra_sim: largest error / bound over {2 * len(RANDOM)} launches: {worst:.4f}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------- pair overlap
def _overlap(lists, kc, pairs, n_ids, form=None):
    """pinsage_list_pair_overlap with a sentinel-filled output: (status, [np, 3], error word)."""
    import _native as nat
    if form is not None:
        assert bu.overlap_form(kc) == form, (kc, form)
    ld_ = torch.from_numpy(np.ascontiguousarray(lists, np.int64)).cuda()
    pr = torch.from_numpy(np.ascontiguousarray(pairs, np.int64).reshape(-1, 2)).cuda()
    nq, ldk = lists.shape
    npairs = int(pr.shape[0])
    out = torch.full((npairs + PAD, 3), SENT_I, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = nat.lib().pinsage_list_pair_overlap(nat.ptr(ld_), nq, ldk, kc, n_ids, nat.ptr(pr), npairs, nat.ptr(out),
                                             nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[npairs:] == SENT_I).all(), "values behind the pairs' outputs were written"
    return rc, o[:npairs], int(err)


def _check_overlaps(got, lists, kc, pairs):
    want = bu.pair_overlaps(lists, kc, pairs)
    bad = (got != want).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"overlap kc = {kc}, pair {i} = rows {tuple(int(x) for x in pairs[i])}: got "
                             f"{got[i].tolist()}, reference {want[i].tolist()}; {int(bad.sum())} of {len(bad)} differ")
    assert got.dtype == np.int32


def _case_lists(kc, n_ids):
    """Rows of kc + 1 columns (column kc is not part of the list):
    0 base; 1 disjoint; 2 a permutation of 0; 3 shares only column 0 with 0; 4
    only column kc - 1; 5 disjoint in its list, its column kc holds an id of 0
    (and 0's column kc holds an id of 5); 6 all equal; 7 each id twice; 8 one id
    kc - 1 times and one other; 9 holds ids 0 and n_ids - 1; 10 the same ids as 9
    at other places, the rest as in 1."""
    rng = np.random.default_rng(kc)
    base = 10 + rng.permutation(kc)                      # ids 10 .. kc + 9
    rows = np.empty((11, kc + 1), np.int64)
    rows[:, kc] = n_ids - 2
    rows[0, :kc] = base
    rows[1, :kc] = 10 + kc + rng.permutation(kc)
    rows[2, :kc] = rng.permutation(base)
    rows[3, :kc] = 10 + 2 * kc + np.arange(kc)
    rows[3, 0] = base[0]
    rows[4, :kc] = 10 + 3 * kc + np.arange(kc)
    rows[4, kc - 1] = base[kc - 1]
    rows[5, :kc] = 10 + 4 * kc + np.arange(kc)
    rows[5, kc] = base[0]
    rows[0, kc] = rows[5, 0]
    rows[6, :kc] = base[0]
    rows[7, :kc] = np.repeat(base[:(kc + 1) // 2], 2)[:kc]
    rows[8, :kc] = base[kc - 1]
    rows[8, kc // 2] = rows[1, 0]
    rows[9, :kc] = 10 + 5 * kc + np.arange(kc)
    rows[9, 0] = 0
    rows[9, kc - 1] = n_ids - 1
    rows[10, :kc] = rows[1, :kc]
    rows[10, kc - 1] = 0
    rows[10, 0] = n_ids - 1
    assert rows.max() == n_ids - 1 and (rows.min() == 0 or kc == 1)   # one column cannot hold both ends
    return rows


@pytest.mark.parametrize("kc", [1, 2, 63, 64, 65, 100, 1000, 4095, 4096])
def test_overlap_cases_against_sets(kc):
    n_ids = 10 + 6 * 4096 + 7
    lists = _case_lists(kc, n_ids)
    pairs = np.array([(a, b) for a in range(len(lists)) for b in range(len(lists))], np.int64)
    rc, got, err = _overlap(lists, kc, pairs, n_ids, "ballot" if kc <= 64 else "sorted")
    assert rc == 0 and err == 0
    _check_overlaps(got, lists, kc, pairs)
    by = {(int(a), int(b)): got[i].tolist() for i, (a, b) in enumerate(pairs)}
    assert by[(0, 0)] == [kc, kc, kc] and by[(0, 2)] == [kc, kc, kc] and by[(0, 1)] == [kc, kc, 0]
    assert by[(0, 3)][2] == 1 and by[(0, 4)][2] == 1 and by[(0, 5)][2] == 0 and by[(5, 0)][2] == 0
    assert by[(6, 6)] == [1, 1, 1] and by[(7, 7)][0] == (kc + 1) // 2 and by[(8, 8)][0] == min(kc, 2)
    assert by[(9, 10)][2] == min(kc, 2)


@pytest.mark.parametrize("kc", [40, 64, 65, 100])
def test_overlap_thousands_of_shuffled_pairs(kc):
    rng = np.random.default_rng(kc)
    nq, n_ids = 300, 5000
    lists = rng.integers(0, n_ids, (nq, kc + 3)).astype(np.int64)
    lists[:100] = rng.integers(0, kc, (100, kc + 3))          # heavy repeats and overlaps
    lists[100:150, :kc] = lists[150:200, :kc][:, rng.permutation(kc)]   # permutations of other rows
    lists = lists[rng.permutation(nq)]
    pairs = rng.integers(0, nq, (5000, 2)).astype(np.int64)
    pairs[::97, 1] = pairs[::97, 0]
    rc, got, err = _overlap(lists, kc, pairs, n_ids, bu.overlap_form(kc))
    assert rc == 0 and err == 0
    _check_overlaps(got, lists, kc, pairs)
    assert (got[:, 2] == 0).any() and (got[:, 2] > 0).any() and (got[:, 0] < kc).any()


def test_overlap_refusals_and_error_word():
    import _native as nat
    L = nat.lib()
    assert int(L.pinsage_list_overlap_max_k()) == bu.OV_MAX_K == 4096
    n_ids = 50000
    lists = np.random.default_rng(0).integers(0, n_ids, (6, 4100)).astype(np.int64)
    pairs = np.array([(0, 1), (2, 2), (5, 3)], np.int64)
    for kc, n in ((0, n_ids), (-1, n_ids), (4101, n_ids), (4097, n_ids), (10, 2 ** 31), (10, 0)):
        rc, got, err = _overlap(lists, kc, pairs, n)
        assert rc == ERR_ARG and (got == SENT_I).all() and err == 0, (kc, n)
    ld_ = torch.from_numpy(lists).cuda()
    pr = torch.from_numpy(pairs).cuda()
    out = torch.full((3, 3), SENT_I, dtype=torch.int32, device="cuda")
    args = [nat.ptr(ld_), 6, 4100, 10, n_ids, nat.ptr(pr), 3, nat.ptr(out), None, nat.stream_ptr()]
    for null_at in (0, 5, 7):
        a = list(args)
        a[null_at] = None
        assert L.pinsage_list_pair_overlap(*a) == ERR_ARG, null_at
    torch.cuda.synchronize()
    assert (out == SENT_I).all()
    for kc in (10, 4096):                            # the same calls with valid arguments run
        rc, got, err = _overlap(lists, kc, pairs, n_ids, bu.overlap_form(kc))
        assert rc == 0 and err == 0
        _check_overlaps(got, lists, kc, pairs)
    for kc in (10, 100):                             # an id or a row out of range: the error word, clamped
        rc, got, err = _overlap(lists, kc, pairs, 1000)
        assert rc == 0 and err == 1
        _check_overlaps(got, np.where(lists >= 1000, 0, lists), kc, pairs)
        rc, got, err = _overlap(lists, kc, np.array([(0, 6), (-1, 2)]), n_ids)
        assert rc == 0 and err == 1
        _check_overlaps(got, lists, kc, np.array([(0, 0), (0, 2)]))


# ----------------------------------------------------------------------------- the Python functions
class _DegreeGraph:
    def __init__(self, deg):
        self.deg = torch.as_tensor(deg)

    def in_degrees(self, v):
        return self.deg[v]


@pytest.fixture(scope="module")
def fx():
    d = golden("beyond_accuracy")
    d["g"] = _DegreeGraph(d["in_degrees"].astype(np.int64))
    return d


def test_functions_reproduce_the_reference_fixture(fx):
    import baselines
    km, tp, g, f = fx["knn_mat"], fx["test_positives"], fx["g"], fx["features"]
    km64 = km.astype(np.int64)
    for K, a, p in zip(fx["cov_ks"].tolist(), fx["coverage_all"].tolist(), fx["coverage_positives"].tolist()):
        bu.check_metric("coverage", K, baselines.coverage(km, tp, K=K), a)
        bu.check_metric("coverage of positives", K, baselines.coverage(km, tp, K=K, all_nodes=False), p)
    assert baselines.coverage(km, tp, K=10, queries=torch.arange(200).repeat(2)) == 2 * fx["coverage_all"][1]
    for K, want in zip(fx["deg_ks"].tolist(), fx["average_degree"].tolist()):
        bu.check_metric("average degree", K, baselines.average_degree(km, g, tp, K), want)
        vals, counts = baselines.degree_dist(km, g, tp, K)
        assert vals.dtype == torch.int64 and counts.dtype == torch.int64
        bu.check_degree_dist(K, (vals.numpy(), counts.numpy()),
                             (fx[f"degree_dist_vals_{K}"], fx[f"degree_dist_counts_{K}"]))
    for i, (K, want) in enumerate(zip(fx["inter_ks"].tolist(), fx["inter_diversity"].tolist())):
        np.random.seed(int(fx["inter_seeds"][i]))
        got = baselines.inter_diversity(km, tp, K, 400, n_pairs=int(fx["inter_pairs"]))
        nxt = int(np.random.randint(0, int(fx["next_draw_high"])))
        assert isinstance(got, float)
        bu.check_metric("inter diversity", K, got, want, 1e-12)
        assert nxt == int(fx["inter_next_draw"][i]), f"inter diversity (K = {K}): numpy's generator is elsewhere"
    for K, want in zip(fx["intra_ks"].tolist(), fx["intra_diversity"].tolist()):
        _, s, kc = bu.intra_sims_identity(km64, f, K)
        bound = float(bu.device_intra_bound(s, kc, km64, f, K).mean()) + bu.reference_fp32_bound(km64, f, K)
        got = baselines.intra_diversity(km, tp, K, f)
        print(f"intra diversity K = {K}: {got!r}, reference {want!r}, |diff| {abs(got - want):.3e}, bound {bound:.3e}")
        assert isinstance(got, float) and bound < 1e-3
        bu.check_metric("intra diversity", K, got, want, bound)


def test_given_pairs_draw_nothing_and_inputs_of_any_kind_agree(fx):
    import baselines
    km, g, f = fx["knn_mat"], fx["g"], fx["features"]
    pairs = np.random.default_rng(3).integers(0, 400, (500, 2))
    np.random.seed(11)
    before = np.random.get_state()
    res = [baselines.beyond_accuracy(m, g, ff, k=10, pairs=pp) for m, ff, pp in (
        (torch.from_numpy(km), torch.from_numpy(f), pairs),
        (torch.from_numpy(km.astype(np.int64)), f, torch.from_numpy(pairs)),
        (torch.from_numpy(km.astype(np.int64)).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(pairs).cuda()))]
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert list(res[0]) == ["intra diversity", "inter diversity", "coverage", "average degree"]
    assert res[0] == res[1] == res[2] and all(isinstance(v, float) for v in res[0].values())
    km64 = km.astype(np.int64)
    bu.check_metric("inter diversity", 10, res[0]["inter diversity"], bu.inter_diversity_ref(km64, 10, pairs), 1e-12)
    bu.check_metric("coverage", 10, res[0]["coverage"], bu.coverage_ref(km64, None, 10))
    bu.check_metric("average degree", 10, res[0]["average degree"], bu.degrees_ref(km64, fx["in_degrees"], 10)[0])
    # K above the list length: the whole list
    for K in (61, 100, 5000):
        assert baselines.intra_diversity(km, None, K, f) == baselines.intra_diversity(km, None, 60, f)
        assert baselines.inter_diversity(km, None, K, 400, pairs=pairs) == \
            baselines.inter_diversity(km, None, 60, 400, pairs=pairs)
        assert baselines.average_degree(km, g, None, K) == baselines.average_degree(km, g, None, 60)
    with pytest.raises(IndexError):
        baselines.inter_diversity(km, None, 10, 400, pairs=np.array([[0, 400]]))
    with pytest.raises(IndexError):
        baselines.inter_diversity(km, None, 10, 300, pairs=pairs)      # ids up to 399 in the lists


def test_compute_beyond_accuracy_table(fx):
    pd = pytest.importorskip("pandas")
    import baselines
    km = torch.from_numpy(fx["knn_mat"].astype(np.int64))
    wide = torch.cat([km, km.flip(1)], dim=1)   # 120 columns: k = 100 is a true cut
    np.random.seed(5)
    table = baselines.compute_beyond_accuracy_table({"a": (None, wide), "b": (None, km)}, None, fx["g"],
                                                    fx["features"])
    assert isinstance(table, pd.DataFrame) and list(table.index) == ["a", "b"]
    assert list(table.columns) == ["intra diversity", "inter diversity", "coverage", "average degree"]
    np.random.seed(5)
    want = baselines.beyond_accuracy(wide, fx["g"], fx["features"], k=100)
    assert {c: float(table.loc["a", c]) for c in table.columns} == want


# ----------------------------------------------------------------------------- PinSage.evaluate_beyond_accuracy
N = 2000


def _trainer(tmp, seed=1):
    import graph
    import synthetic
    pg = synthetic.make_playlist_graph(N, 400, 14000, seed=41)
    indptr, indices = pg.csr()
    g = graph.CSRGraph.from_csr(indptr, indices, base_dir=tmp, nbhds_path=os.path.join(tmp, "nb.pt"))
    feats = torch.from_numpy(synthetic.make_features(N, 128, seed=42))
    pos = torch.from_numpy(synthetic.make_positives(pg, 8000, seed=43))
    return pu.make_trainer(g, N, feats, pos, 2, 10, 32, margin=1e-5, seed=seed)


@pytest.fixture
def tmp_cwd():
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            yield tmp
        finally:
            os.chdir(cwd)


def test_evaluate_beyond_accuracy_equals_the_list_route_and_leaves_no_trace(tmp_cwd):
    import baselines
    tr = _trainer(tmp_cwd)
    k = 20
    pairs = np.random.default_rng(1).integers(0, N, (700, 2))
    for training in (True, False):
        tr.model.train(training)
        st = torch.get_rng_state()
        res = tr.evaluate_beyond_accuracy(k=k, pairs=pairs)
        assert torch.equal(torch.get_rng_state(), st)
        assert tr.model.training is training
    assert list(res) == ["intra diversity", "inter diversity", "coverage", "average degree"]
    emb = tr.embed()
    _, lists = baselines.knn_from_emb(emb, torch.arange(N), k + 1)
    assert lists.shape == (N, k + 1)
    want = baselines.beyond_accuracy(lists, tr.g, tr.features, k=k, pairs=pairs)
    print("evaluate_beyond_accuracy", res, "list route", want)
    bu.check_metric("coverage", k, res["coverage"], want["coverage"])
    bu.check_metric("average degree", k, res["average degree"], want["average degree"])
    bu.check_metric("inter diversity", k, res["inter diversity"], want["inter diversity"], 1e-12)
    bu.check_metric("intra diversity", k, res["intra diversity"], want["intra diversity"], 1e-12)
    assert 0.0 < res["coverage"] <= 1.0 and 0.0 <= res["inter diversity"] <= 1.0
    # without pairs it draws the reference's one numpy call
    np.random.seed(3)
    drawn = tr.evaluate_beyond_accuracy(k=k, n_pairs=300)
    np.random.seed(3)
    same = np.random.randint(0, N, (300, 2))
    after = np.random.get_state()
    assert drawn["inter diversity"] == baselines.inter_diversity(lists, None, k, N, pairs=same)
    np.random.seed(3)
    tr.evaluate_beyond_accuracy(k=k, n_pairs=300)
    now = np.random.get_state()
    assert np.array_equal(now[1], after[1]) and now[2:] == after[2:]


def test_evaluate_beyond_accuracy_between_steps_changes_no_step(tmp_cwd):
    """Two trainers from one seed, the same three batches through train_batch;
    one evaluates after the first.  Their parameters end bitwise equal."""
    a = _trainer(tmp_cwd)
    b = _trainer(tmp_cwd)
    b.model.load_state_dict({k: v.detach().clone() for k, v in a.model.state_dict().items()})
    assert torch.equal(a.nbhds[1], b.nbhds[1])
    torch.manual_seed(7)
    batches = [a.next_batch()[0].clone() for _ in range(3)]
    for tr, with_eval in ((a, False), (b, True)):
        torch.manual_seed(8)
        for i, batch in enumerate(batches):
            tr.train_batch(batch.clone())
            if with_eval and i == 0:
                tr.evaluate_beyond_accuracy(k=10, n_pairs=200)
        tr._sync_state()
    for (ka, pa), (kb, pb) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert ka == kb and torch.equal(pa.detach().cpu(), pb.detach().cpu()), ka
