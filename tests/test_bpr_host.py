"""The references of tests/bpr_util.py checked on the host, and the host side of
baselines.BPR: bpr_objective against the util's, constructor refusals and
defaults.  No GPU.

The gradient a half-iteration uses is read back from its outputs (from zero
accumulators h_new = g^2 and the step has g's sign) and held against central
differences of the float64 objective of the same draw, step 1e-5, relative
error (largest difference over the largest entry, per table) below 1e-6, which
is tests/test_lmf_host.py's method and threshold; each of
bpr_util.GRADIENT_DEFECTS has to exceed 1e-3, and each of bpr_util.DRAW_DEFECTS
has to fail a property of the draw.
"""
import numpy as np
import pytest
import torch

import als_util as au
import bpr_util as bu
import lmf_util as lu
import n2v_util as nu

SEED = 0x5EEDBA5E0FB9


def _central(fun, a, step=1e-5):
    """tests/test_lmf_host.py::_central."""
    g = np.zeros_like(a)
    for i in np.ndindex(*a.shape):
        keep = a[i]
        a[i] = keep + step
        up = fun()
        a[i] = keep - step
        down = fun()
        a[i] = keep
        g[i] = (up - down) / (2 * step)
    return g


def _case(f, seed, S, n_users=7, n_items=9, scale=0.5):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, n_items // 2 + 1, n_users)
    lengths[1] = 0
    csr = au.random_csr(rng, lengths, n_items, "ones")
    X, Y = rng.normal(0, scale, (n_users, f)), rng.normal(0, scale, (n_items, f))
    return csr, X, Y, rng.normal(0, scale, n_items), bu.draw(csr, S, SEED + seed, 3)


def _gradient_gap(csr, X, Y, b, neg, S, reg, defect=None):
    """The largest relative error of the implied gradient over X, Y and b."""
    X, Y, b = (np.array(a, np.float64) for a in (X, Y, b))
    L = lambda: bu.objective(csr, X, Y, b, neg, S, reg)  # noqa: E731
    zx, zy = np.zeros_like(X), np.zeros_like(Y)
    xn, hx = bu.half_iteration(csr, neg, S, "user", X, Y, b, zx, None, reg, 0.1, np.float64, defect)
    yn, hy, bn, hb = bu.half_iteration(csr, neg, S, "item", X, Y, b, zy, zy[:, 0], reg, 0.1, np.float64, defect)
    worst = 0.0
    for old, new, h in ((X, xn, hx), (Y, yn, hy), (b, bn, hb)):
        want = _central(L, old)
        got = lu.implied_gradient(old, new, h)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    return worst


@pytest.mark.parametrize("f,S,reg", [(4, 1, 0.01), (8, 3, 0.0), (4, 8, 0.6)])
def test_gradient_matches_central_differences(f, S, reg):
    case = _case(f, seed=f + S, S=S)
    assert (case[4] >= 0).any()
    gap = _gradient_gap(*case, S, reg)
    print(f"f = {f}, negatives = {S}, reg = {reg}: relative error {gap:.2e}")
    assert gap < 1e-6


def test_gradient_check_sees_void_samples():
    """A row that holds every item but one: most of its samples are void and take no part."""
    rng = np.random.default_rng(2)
    rows = [(np.arange(9), np.ones(9)), (np.delete(np.arange(9), 4), np.ones(8)), ([2, 5], [1, 1])]
    csr = au.csr_from_rows(rows, 9)
    neg = bu.draw(csr, 2, SEED, 0)
    assert (neg < 0).sum() >= 18 and (neg >= 0).any()
    X, Y, b = rng.normal(0, 0.5, (3, 4)), rng.normal(0, 0.5, (9, 4)), rng.normal(0, 0.5, 9)
    assert _gradient_gap(csr, X, Y, b, neg, 2, 0.05) < 1e-6


@pytest.mark.parametrize("defect", bu.GRADIENT_DEFECTS)
def test_gradient_check_rejects_planted_defects(defect):
    case = _case(4, seed=3, S=2)
    assert _gradient_gap(*case, 2, 0.6) < 1e-6
    assert _gradient_gap(*case, 2, 0.6, defect=defect) > 1e-3


# ----------------------------------------------------------------------------- the draw
def _edge_matrix():
    """40 items: an empty row, a full row, a row missing item 17 only, random rows."""
    rng = np.random.default_rng(11)
    rows = [([], []), (np.arange(40), np.ones(40)), (np.delete(np.arange(40), 17), np.ones(39))]
    rows += [(np.sort(rng.choice(40, n, replace=False)), np.ones(n)) for n in (1, 5, 20, 33)]
    return au.csr_from_rows(rows, 40)


def _draw_faults(csr, neg, S):
    """How many accepted negatives are a column of their own row or out of range."""
    ptr, idx, _, _, n_items = csr
    u, _ = bu.samples(csr, S)
    bad = 0
    for t in np.flatnonzero(neg >= 0):
        bad += int(neg[t] >= n_items or neg[t] in idx[ptr[u[t]]:ptr[u[t] + 1]])
    return bad + int((neg < -1).sum())


@pytest.mark.parametrize("S", [1, 3, 8])
def test_draw_properties(S):
    csr = _edge_matrix()
    ptr = csr[0]
    neg = bu.draw(csr, S, SEED, 5)
    assert neg.dtype == np.int32 and len(neg) == ptr[-1] * S
    assert _draw_faults(csr, neg, S) == 0
    full, but_one = neg[ptr[1] * S:ptr[2] * S], neg[ptr[2] * S:ptr[3] * S]
    assert (full == -1).all()
    assert np.isin(but_one, (-1, 17)).all() and (but_one == 17).any() and (but_one == -1).any()
    rest = neg[ptr[3] * S:]
    assert (rest[:(ptr[6] - ptr[3]) * S] >= 0).all()          # rows of 1, 5, 20 of 40: 16 tries suffice here
    assert np.array_equal(neg, bu.draw(csr, S, SEED, 5))
    for other in (bu.draw(csr, S, SEED + 1, 5), bu.draw(csr, S, SEED, 6), bu.draw(csr, S, SEED, 5, offset=1)):
        assert not np.array_equal(neg, other) and _draw_faults(csr, other, S) == 0
    # a block of rows drawn alone with its first cell's index draws what it draws in the whole
    r0 = 3
    block = (ptr[r0:] - ptr[r0], csr[1][ptr[r0]:], csr[2][ptr[r0]:], csr[3] - r0, csr[4])
    assert np.array_equal(bu.draw(block, S, SEED, 5, cell_base=int(ptr[r0])), neg[ptr[r0] * S:])
    assert not np.array_equal(bu.draw(block, S, SEED, 5), neg[ptr[r0] * S:])


def test_draw_is_uniform_over_the_items_outside_the_row():
    """One row of 10 of 50 items, 8 x 10 samples over 60 rounds: 4800 draws over
    40 items, 120 expected each; five standard deviations of the binomial."""
    csr = au.csr_from_rows([(np.arange(0, 50, 5), np.ones(10))], 50)
    neg = np.concatenate([bu.draw(csr, 8, SEED, rho) for rho in range(60)])
    assert (neg >= 0).all()
    counts = np.bincount(neg, minlength=50)
    assert (counts[::5] == 0).all()
    free = np.delete(counts, np.arange(0, 50, 5))
    sd = np.sqrt(4800 * (1 / 40) * (39 / 40))
    assert np.abs(free - 120).max() < 5 * sd, free


def test_draw_defects_fail_the_checks():
    csr = _edge_matrix()
    assert _draw_faults(csr, bu.draw(csr, 3, SEED, 5, defect="positives_not_rejected"), 3) > 0
    used = [r for it in range(30) for r in bu.rounds(it)]
    assert len(set(used)) == 60 and 60 not in used           # the held-out round 2 * iterations is never used
    assert all(a != b for a, b in (bu.rounds(it) for it in range(30)))
    shared = [bu.rounds(it, "halves_share_a_round") for it in range(30)]
    assert all(a == b for a, b in shared)
    # and the fit is another fit: the item half sees another draw
    case = _case(4, seed=9, S=1)
    csr, X, Y, b = case[:4]
    good = bu.fit(csr, X, Y, b, 1, SEED, 0.01, 0.1, 2, np.float64)
    bad = bu.fit(csr, X, Y, b, 1, SEED, 0.01, 0.1, 2, np.float64, defect="halves_share_a_round")
    assert not np.array_equal(good[1], bad[1])


# ----------------------------------------------------------------------------- objective and entries
@pytest.mark.parametrize("S", [1, 4])
def test_bpr_objective_equals_the_util(S):
    import baselines as bl
    csr = _edge_matrix()
    rng = np.random.default_rng(20 + S)
    X, Y = rng.normal(0, 0.7, (7, 8)).astype(np.float32), rng.normal(0, 0.7, (40, 8)).astype(np.float32)
    b = rng.normal(0, 0.7, 40).astype(np.float32)
    neg = bu.draw(csr, S, SEED, 1)
    assert (neg < 0).any() and (neg >= 0).any()
    want = bu.objective(csr, X, Y, b, neg, S, 0.3)
    t = tuple(torch.from_numpy(a) for a in csr[:3]) + csr[3:]
    got = bl.bpr_objective(t, torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(b), torch.from_numpy(neg),
                           S, 0.3)
    assert isinstance(got, float) and abs(got - want) <= 1e-12 * abs(want), (got, want)
    with pytest.raises(ValueError):
        bl.bpr_objective(t, torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(b),
                         torch.from_numpy(neg[:-1]), S, 0.3)


@pytest.mark.parametrize("S", [1, 3])
def test_entry_arrays_match_the_loops(S):
    csr = _edge_matrix()
    neg = bu.draw(csr, S, SEED, 2)
    w = np.random.default_rng(S).uniform(0.1, 0.9, len(neg)) * (neg >= 0)
    for entries, loops, n in ((bu.user_entries, bu.user_entries_loops, csr[3]),
                              (bu.item_entries, bu.item_entries_loops, csr[4])):
        ptr, idx, val = entries(csr, neg, w, S)
        rows = loops(csr, neg, w, S)
        assert len(ptr) == n + 1 and ptr[0] == 0 and ptr[-1] == len(idx) == len(val) and idx.dtype == np.int32
        for r in range(n):
            got = list(zip(val[ptr[r]:ptr[r + 1]], idx[ptr[r]:ptr[r + 1]]))
            assert len(got) == len(rows[r])
            assert all(a[0] == b[0] and np.signbit(a[0]) == np.signbit(b[0]) and a[1] == b[1]
                       for a, b in zip(got, rows[r])), r
    assert np.array_equal(bu.user_entries(csr, neg, w, S)[0], csr[0] * 2 * S)
    void = np.flatnonzero(neg < 0)
    val = bu.user_entries(csr, neg, w, S)[2].reshape(-1, 2)
    assert len(void) and (val[void] == 0).all() and np.signbit(val[void, 1]).all() and not np.signbit(val[void, 0]).any()


# ----------------------------------------------------------------------------- the planted matrix
PLANTED = dict(f=16, lr=0.1, iterations=30, reg=0.01, S=1)
_PLANTED_CACHE = {}


def planted_fits():
    """(csr, groups, X0, Y0, neg of the held-out round, {dtype: (X, Y, b)}), computed once."""
    if not _PLANTED_CACHE:
        p = PLANTED
        csr, groups = bu.planted_matrix(1)
        rng = np.random.default_rng(p["f"])
        X0, Y0 = au.init_factors(rng, csr[3], p["f"]), au.init_factors(rng, csr[4], p["f"])
        draws = {}
        fits = {dt: bu.fit(csr, X0, Y0, np.zeros(csr[4]), p["S"], SEED, p["reg"], p["lr"], p["iterations"], dt,
                           draws=draws) for dt in (np.float64, np.float32)}
        held_out = bu.draw(csr, p["S"], SEED, 2 * p["iterations"])
        _PLANTED_CACHE["v"] = (csr, groups, X0, Y0, held_out, fits)
    return _PLANTED_CACHE["v"]


def test_planted_matrix_is_the_one_behind_the_planted_graph():
    csr, groups = bu.planted_matrix(1)
    graph, want_groups = nu.planted_graph(1)
    M = au.dense(csr).astype(np.int64)
    assert M.shape == (60, 160) and (M.sum(1) == 8).all() and np.array_equal(groups, want_groups)
    W = M.T @ M
    np.fill_diagonal(W, 0)
    assert np.array_equal(nu.dense_of((graph[0], graph[1], nu.weights_of(graph), 160)), W)


def test_planted_matrix_fit_separates_the_groups():
    p = PLANTED
    csr, groups, X0, Y0, held_out, fits = planted_fits()
    start = bu.objective(csr, X0, Y0, np.zeros(csr[4]), held_out, p["S"], p["reg"])
    seen = np.flatnonzero(np.bincount(csr[1], minlength=csr[4]) > 0)
    ends = {}
    for dt, (X, Y, b) in fits.items():
        assert X.dtype == dt and Y.dtype == dt and b.dtype == dt
        ends[dt] = bu.objective(csr, X, Y, b, held_out, p["S"], p["reg"])
        share = nu.same_group_share(Y, groups, seen)
        print(f"{np.dtype(dt).name}: objective {start:.6g} -> {ends[dt]:.6g}, same-group share {share:.3f}")
        assert ends[dt] > start
        assert share >= 0.5
    gap = abs(ends[np.float32] - ends[np.float64]) / abs(ends[np.float64])
    print(f"float32-to-float64 gap of the final objective: {gap:.3e} relative")


# ----------------------------------------------------------------------------- constructors
def test_constructors_refuse_what_is_documented():
    import _native as nat
    import baselines as bl
    for kw in ({"factors": 6}, {"factors": 132}, {"factors": 0}, {"regularization": -0.1}, {"learning_rate": -0.1},
               {"iterations": -1}, {"regularization": float("inf")}, {"learning_rate": float("nan")},
               {"negatives": 0}, {"negatives": 9}, {"negatives": 1.5}, {"iterations": 1 << 26}):
        with pytest.raises(ValueError):
            bl.BPR(**kw)
    m = bl.BPR()
    assert dict(factors=m.factors, learning_rate=m.learning_rate, regularization=m.regularization,
                iterations=m.iterations, negatives=m.negatives, random_state=m.random_state) == bu.DEFAULTS
    assert m.user_factors is None and m.item_factors is None and m.item_bias is None
    assert bl.BPR(regularization=0.0, learning_rate=0.0, negatives=8, iterations=0).negatives == 8
    assert bl.BPR_MAX_FACTORS == 128 and bl.BPR_MAX_NEGATIVES == bu.MAX_NEGATIVES == 8
    assert bl.BPR_MAX_TRIES == bu.TRIES == int(nat.lib().pinsage_bpr_max_tries()) == 16
    assert bl.ColTrackBPR().factors == 128 and bl.TrackTrackBPR(factors=64).factors == 64
    assert bl.ColTrackBPR().algo == "bpr" and bl.ColTrackBPR._Fit is bl.BPR
    for name in ("BPR", "BPR_MAX_FACTORS", "BPR_MAX_TRIES", "BPR_MAX_NEGATIVES", "bpr_objective", "ColTrackBPR",
                 "TrackTrackBPR"):
        assert name in bl.__all__
    # the ALS classes keep refusing algo="bpr"; the new classes are the way in
    with pytest.raises(NotImplementedError, match="ColTrackBPR"):
        bl.ColTrackCF(algo="bpr")
    assert issubclass(bl.ColTrackBPR, bl.PredictionModel) and bl.ColTrackBPR.knn is bl.ColTrackCF.knn
    assert issubclass(bl.BPR, bl._RowFit) and bl.BPR.similar_items is bl.LMF.similar_items
