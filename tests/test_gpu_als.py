"""The kernels of csrc/als.hip (pinsage_als_gram, pinsage_als_half) and what
stands on them: baselines.ALS, ColTrackCF and TrackTrackCF, and with save_knn /
LazyKnnDict the two tables end to end.

A half-iteration is held against the float64 restatement of tests/als_util.py by
its error measure, |x - x64| / max(|x64|, |x_in|) per row, and the tolerance is
als_util.TOL_FACTOR (8) times what the float32 numpy restatement shows against
float64 on the same inputs; every such test prints both figures.  The references
are checked on the host in tests/test_als_host.py.  X is passed with NaN in its
padding columns and a sentinel tail, Y with NaN padding; the padding has to be
NaN and the tail untouched afterwards.

A block of rows is 8 rows, one per wave (pinsage_als_rows_per_block), and a
workgroup takes 4 consecutive blocks, 32 rows; a row of more than 512 items
(pinsage_als_long_row) is solved by a whole workgroup.  Each launch asserts from
als_util.row_form which form its rows take.
"""
import numpy as np
import pytest
import torch

import als_util as au
import parity_util as pu
from conftest import golden
from rowfit_util import PAD, SENT, _padded, _unpad

pytestmark = pytest.mark.gpu

ERR_ARG = -2       # pinsage_status (include/pinsage_hip.h)
REG = 0.01


# ----------------------------------------------------------------------------- launch helpers
def _gram(Y, reg, ld=None, n=None, f=None):
    """pinsage_als_gram into a sentinel-filled G: (status, G [f, f])."""
    import _native as nat
    n0, f0 = Y.shape
    n, f, ld = (n0 if n is None else n), (f0 if f is None else f), (f0 if ld is None else ld)
    yd = _padded(Y, max(ld, f0))
    G = torch.full((max(f, 1) * max(f, 1) + PAD,), SENT, dtype=torch.float32, device="cuda")
    rc = nat.lib().pinsage_als_gram(nat.ptr(yd), n, f, ld, reg, nat.ptr(G), nat.stream_ptr())
    torch.cuda.synchronize()
    g = G.cpu().numpy()
    assert (g[f * f:] == SENT).all()
    return rc, g[:f * f].reshape(f, f)


def _half(csr, X, Y, alpha, steps, ldx=None, ldy=None, reg=REG, forms=None):
    """One half-iteration on the device, G from pinsage_als_gram:
    (status, new X [n_rows, f], error word)."""
    import _native as nat
    L = nat.lib()
    ptr, idx, val, n_rows, n_other = csr
    f = X.shape[1]
    ldx, ldy = (f if ldx is None else ldx), (f if ldy is None else ldy)
    if forms is not None:
        long_row = int(L.pinsage_als_long_row())
        got = {au.row_form(int(ln), long_row) for ln in np.diff(ptr)}
        assert got == set(forms), (got, forms)
    xd, yd = _padded(X, ldx, tail=True), _padded(Y, ldy)
    G = torch.empty(f * f, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ptr, idx, val)]
    assert L.pinsage_als_gram(nat.ptr(yd), n_other, f, ldy, reg, nat.ptr(G), nat.stream_ptr()) == 0
    rc = L.pinsage_als_half(nat.ptr(t[0]), nat.ptr(t[1]), nat.ptr(t[2]), n_rows, nat.ptr(yd), n_other, ldy,
                            nat.ptr(xd), ldx, f, nat.ptr(G), alpha, steps, nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, _unpad(xd, n_rows, f, ldx), int(err)


def _check_half(csr, X, Y, alpha, steps, what, **kw):
    """The device against float64 under the 8x rule; returns the device's X."""
    rc, got, err = _half(csr, X, Y, alpha, steps, **kw)
    assert rc == 0 and err == 0
    x64 = au.half_iteration(*csr[:3], X, Y, REG, alpha, steps, np.float64)
    x32 = au.half_iteration(*csr[:3], X, Y, REG, alpha, steps, np.float32)
    e32, edev = au.row_errors(x32, x64, X).max(), au.row_errors(got, x64, X).max()
    print(f"{what}: float32 restatement {e32:.3e}, device {edev:.3e}, ratio {edev / e32:.2f}")
    assert e32 > 0 and edev <= au.TOL_FACTOR * e32, (what, edev, e32)
    return got


MIXED = [0, 1, 2, 63, 64, 65, 257]


def _mixed_case(f, seed, kind="counts", lengths=MIXED, n_other=300):
    rng = np.random.default_rng(seed)
    csr = au.random_csr(rng, lengths, n_other, kind)
    return csr, au.init_factors(rng, len(lengths), f), au.init_factors(rng, n_other, f)


# ----------------------------------------------------------------------------- the half-iteration
@pytest.mark.parametrize("pad_x,pad_y", [(0, 0), (4, 0), (0, 4), (4, 4)])
@pytest.mark.parametrize("f", [4, 8, 60, 64, 100, 128])
def test_half_iteration_factors_and_leading_dimensions(f, pad_x, pad_y):
    csr, X, Y = _mixed_case(f, seed=f)
    _check_half(csr, X, Y, 1.0, 3, f"f = {f}, ldx = f + {pad_x}, ldy = f + {pad_y}", ldx=f + pad_x, ldy=f + pad_y,
                forms=["wave"])


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 257])
def test_half_iteration_row_counts(n_rows):
    """Around the 8 rows of a block of rows and the 32 rows (4 blocks) of a
    workgroup, and more workgroups than one."""
    rng = np.random.default_rng(n_rows)
    lengths = rng.integers(0, 40, n_rows)
    csr, X, Y = _mixed_case(8, seed=100 + n_rows, lengths=lengths, n_other=64)
    _check_half(csr, X, Y, 1.0, 3, f"{n_rows} rows", forms=["wave"])


@pytest.mark.parametrize("f", [4, 128])
def test_half_iteration_long_rows(f):
    """Rows on both sides of the switch to the workgroup form, a hub of 5000
    items over 6000 others, two long rows in one block of rows and one in the next."""
    import _native as nat
    long_row = int(nat.lib().pinsage_als_long_row())
    lengths = [5000, 3, long_row, long_row + 1, 0, 64, long_row + 64, 1, 2, long_row + 129, 7]
    csr, X, Y = _mixed_case(f, seed=7 + f, lengths=lengths, n_other=6000)
    _check_half(csr, X, Y, 1.0, 3, f"long rows, f = {f}", forms=["wave", "workgroup"], ldx=f + 4)


@pytest.mark.parametrize("alpha", [0.5, 1.0, 40.0])
@pytest.mark.parametrize("kind", au.VALUE_KINDS)
def test_half_iteration_values_and_alpha(kind, alpha):
    csr, X, Y = _mixed_case(16, seed=int(alpha * 10) + len(kind), kind=kind, lengths=MIXED + [600], n_other=700)
    _check_half(csr, X, Y, alpha, 3, f"{kind}, alpha = {alpha}", forms=["wave", "workgroup"])


@pytest.mark.parametrize("steps", [1, 3])
def test_half_iteration_steps(steps):
    csr, X, Y = _mixed_case(64, seed=20 + steps)
    _check_half(csr, X, Y, 2.0, steps, f"{steps} steps")


def test_zero_steps_leave_x_bit_for_bit():
    csr, X, Y = _mixed_case(8, seed=30, lengths=MIXED + [600], n_other=700)
    rc, got, err = _half(csr, X, Y, 1.0, 0, ldx=12)
    assert rc == 0 and err == 0 and np.array_equal(got.view(np.uint32), X.view(np.uint32))


@pytest.mark.parametrize("f", [4, 8])
def test_f_steps_reach_the_exact_solve(f):
    """CG on an f x f system ends after f steps: the device against
    numpy.linalg.solve, by the rule used against the restatement."""
    csr, X, Y = _mixed_case(f, seed=40 + f, lengths=[1, 2, 5, 63, 64, 65, 257, 600], n_other=700)
    rc, got, err = _half(csr, X, Y, 2.0, f)
    assert rc == 0 and err == 0
    exact = au.exact_rows(*csr[:3], Y, REG, 2.0)
    x32 = au.half_iteration(*csr[:3], X, Y, REG, 2.0, f, np.float32)
    e32, edev = au.row_errors(x32, exact, X).max(), au.row_errors(got, exact, X).max()
    print(f"f = {f} steps against the exact solve: float32 restatement {e32:.3e}, device {edev:.3e}")
    assert edev <= au.TOL_FACTOR * e32


def test_zero_rows_stay_zero():
    """A zero row of X without items, and zero rows whose items' y are all zero
    (one solved by a wave, one by the workgroup), keep their bits."""
    rng = np.random.default_rng(50)
    n_other, f = 700, 16
    zero_ids = np.arange(0, 650)
    rows = [(np.zeros(0, np.int32), np.zeros(0, np.float32)),
            (zero_ids[:40], au.values(rng, 40, "counts")),
            (zero_ids[:600], au.values(rng, 600, "counts")),
            (np.arange(640, 700), au.values(rng, 60, "counts"))]
    csr = au.csr_from_rows(rows, n_other)
    X, Y = au.init_factors(rng, 4, f), au.init_factors(rng, n_other, f)
    Y[zero_ids] = 0
    X[:3] = 0
    got = _check_half(csr, X, Y, 3.0, 3, "zero rows", forms=["wave", "workgroup"])
    assert np.array_equal(got[:3].view(np.uint32), np.zeros((3, f), np.uint32))
    assert np.abs(got[3]).max() > 0


def test_two_launches_give_the_same_bits():
    csr, X, Y = _mixed_case(128, seed=60, lengths=MIXED + [5000, 600], n_other=6000)
    a = _half(csr, X, Y, 2.0, 3)[1]
    b = _half(csr, X, Y, 2.0, 3)[1]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a row's bits do not depend on where it stands or on what else is solved
    # (another grid, another block of rows, another wave)
    ptr, idx, val = csr[:3]
    for u in (3, 7, 8):
        one = au.csr_from_rows([(idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]])], 6000)
        alone = _half(one, X[u:u + 1], Y, 2.0, 3)[1]
        assert np.array_equal(alone.view(np.uint32), a[u:u + 1].view(np.uint32)), u


def test_id_out_of_range_sets_the_error_word():
    import baselines as bl
    csr, X, Y = _mixed_case(8, seed=70)
    for bad in (300, -1, 2 ** 31 - 1):
        idx = csr[1].copy()
        idx[5] = bad
        rc, got, err = _half((csr[0], idx) + csr[2:], X, Y, 1.0, 3)
        assert rc == 0 and err == 1 and np.isfinite(got).all()
        t = tuple(torch.from_numpy(a).cuda() for a in (csr[0], idx, csr[2])) + csr[3:]
        with pytest.raises(IndexError):
            bl.ALS(factors=8, iterations=1).fit(t)


def test_refusals_leave_the_outputs_untouched():
    import _native as nat
    L = nat.lib()
    n, m, f = 5, 9, 8
    rng = np.random.default_rng(80)
    csr = au.random_csr(rng, [2, 0, 3, 1, 4], m, "counts")
    ptr, idx, val = (torch.from_numpy(a).cuda() for a in csr[:3])
    Y = torch.from_numpy(au.init_factors(rng, m + 2, 16)).cuda().reshape(-1)
    sp = nat.stream_ptr

    def half(f=f, ldx=f, ldy=f, x_off=0, y_off=0, g_off=0, alpha=1.0, steps=3):
        X = torch.full((n * 16 + PAD,), SENT, dtype=torch.float32, device="cuda")
        G = torch.full((16 * 16 + PAD,), 0.5, dtype=torch.float32, device="cuda")
        rc = L.pinsage_als_half(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n, nat.ptr(Y[y_off:]), m, ldy,
                                nat.ptr(X[x_off:]), ldx, f, nat.ptr(G[g_off:]), alpha, steps, None, sp())
        torch.cuda.synchronize()
        return rc, bool((X == SENT).all())

    def gram(f=f, ld=f, y_off=0, g_off=0, reg=REG):
        G = torch.full((16 * 16 + PAD,), SENT, dtype=torch.float32, device="cuda")
        rc = L.pinsage_als_gram(nat.ptr(Y[y_off:]), m, f, ld, reg, nat.ptr(G[g_off:]), sp())
        torch.cuda.synchronize()
        return rc, bool((G == SENT).all())

    assert half()[0] == 0 and not half()[1] and gram()[0] == 0 and not gram()[1]     # the accepted call writes
    for kw in ({"f": 6}, {"f": 132, "ldx": 132, "ldy": 132}, {"f": 0}, {"ldx": 4}, {"ldy": 4}, {"ldx": 10},
               {"ldy": 10}, {"x_off": 1}, {"y_off": 1}, {"g_off": 1}, {"steps": -1}, {"alpha": 0.0},
               {"alpha": float("nan")}):
        assert half(**kw) == (ERR_ARG, True), kw
        assert L.pinsage_last_error()
    for kw in ({"f": 6}, {"f": 132, "ld": 132}, {"ld": 4}, {"ld": 10}, {"y_off": 1}, {"g_off": 1}, {"reg": 0.0},
               {"reg": -1.0}, {"reg": float("nan")}):
        assert gram(**kw) == (ERR_ARG, True), kw


# ----------------------------------------------------------------------------- the Gram matrix
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("f,pad", [(4, 0), (60, 4), (128, 0)])
def test_gram(n, f, pad):
    rng = np.random.default_rng(n + f)
    Y = rng.standard_normal((n, f)).astype(np.float32)
    rc, G = _gram(Y, REG, ld=f + pad)
    assert rc == 0
    Y64 = Y.astype(np.float64)
    want = Y64.T @ Y64 + np.float64(np.float32(REG)) * np.eye(f)
    bound = pu.gemm_bound(n, np.abs(Y64).T @ np.abs(Y64) + REG * np.eye(f))
    assert (np.abs(G - want) <= bound).all(), float((np.abs(G - want) / bound).max())
    assert np.array_equal(G.view(np.uint32), G.T.copy().view(np.uint32)), "G is not symmetric bit for bit"
    Yi = rng.integers(-8, 9, (n, f)).astype(np.float32)
    rc, G = _gram(Yi, 0.5, ld=f + pad)
    assert rc == 0 and np.array_equal(G, (Yi.astype(np.float64).T @ Yi + 0.5 * np.eye(f)).astype(np.float32))
    assert np.array_equal(_gram(Y, REG, ld=f + pad)[1].view(np.uint32), _gram(Y, REG, ld=f + pad)[1].view(np.uint32))


# ----------------------------------------------------------------------------- ALS.fit
def _small_matrix():
    rng = np.random.default_rng(90)
    R = (rng.random((70, 50)) < 0.15) * rng.integers(1, 5, (70, 50))
    R[11, :] = 0                                     # an empty row and an empty column
    R[:, 23] = 0
    rows = [(np.flatnonzero(r), r[r > 0]) for r in R]
    return au.csr_from_rows(rows, 50)


def _fixture_graph():
    import graph
    f = golden("jaccard")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    edges = f["edges"].astype(np.int64)
    return n, nc, graph.CSRGraph(n + nc, edges[:, 0], edges[:, 1])


def _col_track_matrix():
    import baselines as bl
    n, _, g = _fixture_graph()
    t = bl.to_col_track_matrix(g, list(range(n)))
    assert all(a.is_cuda for a in t[:3])
    return tuple(a.cpu().numpy() for a in t[:3]) + t[3:]


_FIT_CACHE = {}


def _fit_reference(name, f):
    """(csr, X0, Y0, float64 fits after 1 and 15 iterations, float32 fit after 15), computed once."""
    if (name, f) not in _FIT_CACHE:
        csr = _small_matrix() if name == "small" else _col_track_matrix()
        rng = np.random.default_rng(f)
        X0, Y0 = au.init_factors(rng, csr[3], f), au.init_factors(rng, csr[4], f)
        one = au.fit(csr, X0, Y0, REG, 1.0, 3, 1, np.float64)
        f64 = au.fit(csr, *one, REG, 1.0, 3, 14, np.float64)
        f32 = au.fit(csr, X0, Y0, REG, 1.0, 3, 15, np.float32)
        _FIT_CACHE[name, f] = csr, X0, Y0, one, f64, f32
    return _FIT_CACHE[name, f]


@pytest.mark.parametrize("f", [16, 128])
@pytest.mark.parametrize("name", ["small", "col_track"])
def test_fit_from_given_factors(name, f):
    import baselines as bl
    csr, X0, Y0, one, f64, f32 = _fit_reference(name, f)
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    xg, yg = torch.from_numpy(X0), torch.from_numpy(Y0).cuda()
    m = bl.ALS(factors=f).fit(t, user_factors=xg, item_factors=yg)
    assert torch.equal(xg, torch.from_numpy(X0)) and torch.equal(yg.cpu(), torch.from_numpy(Y0))   # copied
    for tab in (m.user_factors, m.item_factors):
        assert tab.is_cuda and tab.dtype == torch.float32
    tol = 0.0
    for which, got, i in (("users", m.user_factors, 0), ("items", m.item_factors, 1)):
        e32, edev = au.table_error(f32[i], f64[i]), au.table_error(got.cpu().numpy(), f64[i])
        print(f"{name}, f = {f}, {which} after 15 iterations: float32 restatement {e32:.3e}, device {edev:.3e}, "
              f"ratio {edev / e32:.2f}")
        assert edev <= au.TOL_FACTOR * e32
        tol = max(tol, au.TOL_FACTOR * e32)
    loss1 = bl.ALS(factors=f, iterations=1).fit(t, user_factors=xg, item_factors=yg).loss()
    loss15, want = m.loss(), au.loss(csr, *f64, REG, 1.0)
    assert abs(loss1 - au.loss(csr, *one, REG, 1.0)) <= tol * abs(loss1)
    assert loss15 < loss1 and abs(loss15 - want) <= tol * abs(want), (loss1, loss15, want)


def test_fit_checks_its_input():
    import baselines as bl
    csr = _small_matrix()
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        v = t[2].clone()
        v[3] = bad
        with pytest.raises(ValueError):
            bl.ALS(factors=8, iterations=1).fit((t[0], t[1], v) + t[3:])
    with pytest.raises(ValueError):
        bl.ALS(factors=8).fit(t, user_factors=torch.zeros(70, 4))


def test_random_state_and_the_global_generator():
    import baselines as bl
    csr = _small_matrix()
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    a = bl.ALS(factors=8, iterations=2, random_state=7).fit(t)
    b = bl.ALS(factors=8, iterations=2, random_state=7).fit(t)
    assert torch.equal(a.user_factors, b.user_factors) and torch.equal(a.item_factors, b.item_factors)
    assert not torch.equal(a.item_factors, bl.ALS(factors=8, iterations=2, random_state=8).fit(t).item_factors)
    g = torch.Generator().manual_seed(7)
    m = bl.ALS(factors=8, iterations=0, random_state=7).fit(t)
    assert torch.equal(m.user_factors.cpu(), (torch.rand(70, 8, generator=g) - 0.5) / 8)
    assert torch.equal(m.item_factors.cpu(), (torch.rand(50, 8, generator=g) - 0.5) / 8)
    torch.manual_seed(3)
    m = bl.ALS(factors=8, iterations=1).fit(t)
    after = torch.rand(1)
    torch.manual_seed(3)
    x0, y0 = (torch.rand(70, 8) - 0.5) / 8, (torch.rand(50, 8) - 0.5) / 8     # (70 + 50) * 8 draws
    assert torch.equal(after, torch.rand(1))
    want = bl.ALS(factors=8, iterations=1).fit(t, user_factors=x0, item_factors=y0)
    assert torch.equal(m.item_factors, want.item_factors)


# ----------------------------------------------------------------------------- the two baselines
@pytest.fixture(scope="module")
def cf():
    import baselines as bl
    n, _, g = _fixture_graph()
    rng = np.random.default_rng(95)
    pos = rng.integers(0, n, (330, 2))
    pos = np.concatenate([pos, pos[rng.integers(0, 330, 70)]])      # 400 positives, with repeats
    tp = torch.from_numpy(pos)
    ids = list(range(n))
    torch.manual_seed(1)
    ct, tt = bl.ColTrackCF(), bl.TrackTrackCF(factors=16)
    ct.train(g, ids, tp, None, None)
    tt.train(g, ids, tp, None, None)
    return n, g, tp, ids, {"ColTrackCfALS": ct, "TrackTrackCfALS": tt}


@pytest.mark.parametrize("k", [1, 10, 299])
def test_cf_knn_is_knn_from_emb(cf, k):
    import baselines as bl
    n, _, _, _, models = cf
    assert models["ColTrackCfALS"].model.factors == 128 and models["TrackTrackCfALS"].model.factors == 16
    for name, m in models.items():
        assert tuple(m.model.item_factors.shape) == (n, m.model.factors)
        for nodeset in (torch.arange(n), torch.tensor([5, 5, 299, 0]), torch.tensor([7, 3]).cuda()):
            w, nb = m.knn(nodeset, k)
            want_w, want_n = bl.knn_from_emb(m.model.item_factors, nodeset, k)
            assert tuple(w.shape) == tuple(nb.shape) == (len(nodeset), k)
            assert w.dtype == torch.float32 and nb.dtype == torch.int64
            assert w.device == nodeset.device and nb.device == nodeset.device
            assert torch.equal(w.cpu(), want_w.cpu()) and torch.equal(nb.cpu(), want_n.cpu()), name
        ids_, scores = m.model.similar_items(torch.tensor([4, 9]), 6)
        assert tuple(ids_.shape) == (2, 6) and ids_.dtype == torch.int64 and scores.dtype == torch.float32
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    with pytest.raises(IndexError):
        models["ColTrackCfALS"].knn(torch.tensor([n]), 3)


def test_tables_end_to_end(cf, tmp_path, monkeypatch):
    import baselines as bl
    n, g, tp, ids, models = cf
    monkeypatch.setattr(bl, "PRECOMP_K", 200)         # 300 tracks: lists of 1000 do not exist
    for name, m in models.items():
        bl.save_knn(m, name, ids, str(tmp_path), train_time=2.0, b_size=128)
    d = bl.LazyKnnDict(list(models), ids, str(tmp_path))
    table = bl.compute_results_table(d, tp, g)
    assert list(table.index) == ["ColTrackCfALS", "TrackTrackCfALS"]
    assert np.isfinite(table.to_numpy(dtype=np.float64)).all()
    feats = torch.from_numpy(np.random.default_rng(96).standard_normal((n, 12)).astype(np.float32))
    np.random.seed(11)
    beyond = bl.compute_beyond_accuracy_table({name: d[name] for name in models}, tp, g, feats)
    assert list(beyond.index) == list(table.index) and np.isfinite(beyond.to_numpy(dtype=np.float64)).all()
    np.random.seed(11)
    for name, m in models.items():
        w, nb = m.knn(torch.arange(n), 200)           # one batch against the three of save_knn
        sw, sn = d[name]
        assert tuple(nb.shape) == (n, 200) and torch.equal(sn, nb) and torch.equal(sw, w)
        assert table.loc[name, "hr (k=10)"] == bl.hit_rate(nb, tp, 10)
        assert table.loc[name, "hr (k=100)"] == bl.hit_rate(nb, tp, 100)
        assert table.loc[name, "mrr"] == bl.mrr(nb, tp, 1000, 1)
        assert table.loc[name, "low-co accuracy"] == bl.low_co_accuracy(nb, g, tp, 1000, co_thr=1, acc_func=bl.mrr)
        assert table.loc[name, "t (train)"] == 2.0
        want = bl.beyond_accuracy(nb, g, feats, k=100)
        assert {c: float(beyond.loc[name, c]) for c in beyond.columns} == want
