"""The references of tests/lmf_util.py checked on the host, and the host side of
baselines.LMF: lmf_objective against the dense objective, constructor refusals
and defaults.  No GPU.

The gradient a half-iteration uses is read back from its outputs (from zero
accumulators h_new = g^2 and the step has g's sign) and held against central
differences of the float64 objective, step 1e-5, relative error (largest
difference over the largest entry, per table) below 1e-6; each planted defect
of lmf_util.DEFECTS has to fail that check.
"""
import numpy as np
import pytest
import torch

import als_util as au
import lmf_util as lu
from conftest import golden


def _case(f, seed, kind="counts", n_rows=7, n_cols=9, scale=0.5):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, n_cols // 2 + 1, n_rows)
    lengths[1] = 0
    csr = au.random_csr(rng, lengths, n_cols, kind)
    X, Y = rng.normal(0, scale, (n_rows, f)), rng.normal(0, scale, (n_cols, f))
    bx, by = rng.normal(0, scale, n_rows), rng.normal(0, scale, n_cols)
    return csr, X, Y, bx, by


def _central(fun, a, step=1e-5):
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


def _gradient_gap(csr, X, Y, bx, by, reg, alpha, defect=None):
    """The largest relative error of the implied gradient over the four tables."""
    X, Y, bx, by = (np.array(a, np.float64) for a in (X, Y, bx, by))
    L = lambda: lu.objective(csr, X, Y, bx, by, reg, alpha)  # noqa: E731
    tcsr = au.transpose(csr)
    zx, zy = np.zeros_like(X), np.zeros_like(Y)
    xn, bxn, hx, hbx = lu.half_iteration(*csr[:3], X, bx, zx, zx[:, 0], Y, by, reg, alpha, 0.1, np.float64, defect)
    yn, byn, hy, hby = lu.half_iteration(*tcsr[:3], Y, by, zy, zy[:, 0], X, bx, reg, alpha, 0.1, np.float64, defect)
    worst = 0.0
    for old, new, h in ((X, xn, hx), (bx, bxn, hbx), (Y, yn, hy), (by, byn, hby)):
        want = _central(L, old)
        got = lu.implied_gradient(old, new, h)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    return worst


@pytest.mark.parametrize("kind", au.VALUE_KINDS)
@pytest.mark.parametrize("f,alpha,reg", [(4, 1.0, 0.6), (8, 0.5, 0.0), (4, 40.0, 0.05)])
def test_gradient_matches_central_differences(f, alpha, reg, kind):
    gap = _gradient_gap(*_case(f, seed=f + len(kind)), reg, alpha)
    print(f"f = {f}, alpha = {alpha}, reg = {reg}, {kind}: relative error {gap:.2e}")
    assert gap < 1e-6


@pytest.mark.parametrize("defect", lu.DEFECTS)
def test_gradient_check_rejects_planted_defects(defect):
    case = _case(4, seed=3)
    assert _gradient_gap(*case, 0.6, 1.0) < 1e-6
    assert _gradient_gap(*case, 0.6, 1.0, defect=defect) > 1e-3


def test_dense_terms_match_the_definition_cell_by_cell():
    csr, X, Y, bx, by = _case(4, seed=5, scale=3.0)          # scores up to about +-40
    D, dsum = lu.dense_terms(X, bx, Y, by, np.float64)
    Dl, dl = lu.dense_terms_loops(X, bx, Y, by)
    assert np.allclose(D, Dl, rtol=1e-13, atol=1e-13) and np.allclose(dsum, dl, rtol=1e-13, atol=0)
    s = np.array([-800.0, -90.0, -1e-3, 0.0, 1e-3, 90.0, 800.0])
    for dt in (np.float32, np.float64):
        p = lu.sigmoid(s.astype(dt))
        assert p.dtype == dt and np.isfinite(p).all() and p[3] == 0.5 and p[0] == 0 and p[-1] == 1
        assert (np.diff(p) >= 0).all()
    # the phantom item of the unmasked tail: nothing to D, sig(bx) to dsum
    Dt, dt_ = lu.dense_terms(X, 0 * bx, Y, by, np.float64, defect="unmasked_tail")
    D0, d0 = lu.dense_terms(X, 0 * bx, Y, by, np.float64)
    assert np.array_equal(Dt, D0) and np.allclose(dt_ - d0, 0.5)


def _small_matrix():
    """tests/test_gpu_als.py::_small_matrix."""
    rng = np.random.default_rng(90)
    R = (rng.random((70, 50)) < 0.15) * rng.integers(1, 5, (70, 50))
    R[11, :] = 0
    R[:, 23] = 0
    return au.csr_from_rows([(np.flatnonzero(r), r[r > 0]) for r in R], 50)


def _fixture_matrices():
    """The collection-track matrix of tests/golden/jaccard.npz and the 400-pair
    track-track matrix of test_gpu_als.py's cf fixture, as numpy CSRs."""
    import baselines as bl
    import graph
    f = golden("jaccard")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    edges = f["edges"].astype(np.int64)
    g = graph.CSRGraph(n + nc, edges[:, 0], edges[:, 1])
    ct = bl.to_col_track_matrix(g, list(range(n)), device="cpu")
    rng = np.random.default_rng(95)
    pos = rng.integers(0, n, (330, 2))
    pos = np.concatenate([pos, pos[rng.integers(0, 330, 70)]])
    tt = bl.to_track_track_matrix(list(range(n)), torch.from_numpy(pos), device="cpu")
    return [tuple(a.numpy() for a in t[:3]) + tuple(t[3:]) for t in (ct, tt)]


@pytest.mark.parametrize("f", [16, 128])
def test_objective_rises_on_each_of_30_iterations(f):
    d = lu.DEFAULTS
    for name, csr in zip(("small", "col_track", "track_track"), [_small_matrix()] + _fixture_matrices()):
        rng = np.random.default_rng(f)
        X, Y = au.init_factors(rng, csr[3], f), au.init_factors(rng, csr[4], f)
        bx, by = np.zeros(csr[3], np.float32), np.zeros(csr[4], np.float32)
        start = lu.objective(csr, X, Y, bx, by, d["regularization"], d["alpha"])
        seen = lu.fit(csr, X, Y, bx, by, d["regularization"], d["alpha"], d["learning_rate"], d["iterations"],
                      np.float32, trace=True)[4]
        print(f"{name}, f = {f}: L {start:.6g} -> {seen[0]:.6g} -> {seen[-1]:.6g}")
        assert len(seen) == 30 and (np.diff([start] + seen) > 0).all(), (name, seen)


def test_fit_check_rejects_a_falling_objective():
    """lr = 1 at f = 128 is the step the default avoids: L falls on the first iterations."""
    csr = _small_matrix()
    rng = np.random.default_rng(128)
    X, Y = au.init_factors(rng, 70, 128), au.init_factors(rng, 50, 128)
    z = np.zeros
    seen = lu.fit(csr, X, Y, z(70, np.float32), z(50, np.float32), 0.6, 1.0, 1.0, 3, np.float64, trace=True)[4]
    assert not (np.diff([lu.objective(csr, X, Y, z(70), z(50), 0.6, 1.0)] + seen) > 0).all()


@pytest.mark.parametrize("alpha", [0.5, 1.0, 40.0])
@pytest.mark.parametrize("kind", au.VALUE_KINDS)
def test_lmf_objective_equals_the_dense_objective(alpha, kind, monkeypatch):
    import baselines as bl
    rng = np.random.default_rng(int(alpha * 10) + len(kind))
    lengths = rng.integers(0, 12, 23)
    lengths[4] = 0                                                   # an empty row
    rows = [(np.sort(rng.choice(30, ln, replace=False)), au.values(rng, ln, kind)) for ln in lengths]
    rows = [(ids[ids != 17], v[ids != 17]) for ids, v in rows]       # an empty column
    csr = au.csr_from_rows(rows, 31)
    X, Y = rng.normal(0, 0.7, (23, 8)).astype(np.float32), rng.normal(0, 0.7, (31, 8)).astype(np.float32)
    bx, by = rng.normal(0, 0.7, 23).astype(np.float32), rng.normal(0, 0.7, 31).astype(np.float32)
    assert csr[0][5] == csr[0][4] and not (csr[1] == 17).any()
    want = lu.objective(csr, X, Y, bx, by, 0.6, alpha)
    t = tuple(torch.from_numpy(a) for a in csr[:3]) + csr[3:]
    args = (t, torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(bx), torch.from_numpy(by), 0.6)
    got = bl.lmf_objective(*args, alpha=alpha)
    assert isinstance(got, float) and abs(got - want) <= 1e-12 * abs(want), (got, want)
    monkeypatch.setattr(bl, "_LMF_CELLS", 64)                        # row chunks of 2 rows
    got = bl.lmf_objective(*args, alpha=alpha)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_constructors_refuse_what_is_documented():
    import baselines as bl
    for kw in ({"factors": 6}, {"factors": 132}, {"factors": 0}, {"regularization": -0.1}, {"alpha": 0.0},
               {"alpha": -1.0}, {"learning_rate": -0.1}, {"iterations": -1}, {"alpha": float("nan")},
               {"regularization": float("inf")}, {"learning_rate": float("nan")}):
        with pytest.raises(ValueError):
            bl.LMF(**kw)
    m = bl.LMF()
    assert (m.factors, m.learning_rate, m.regularization, m.alpha, m.iterations, m.random_state) == \
        (128, 0.1, 0.6, 1.0, 30, None)
    assert dict(factors=m.factors, learning_rate=m.learning_rate, regularization=m.regularization, alpha=m.alpha,
                iterations=m.iterations, random_state=m.random_state) == lu.DEFAULTS
    assert m.user_factors is None and m.item_bias is None
    assert bl.LMF_MAX_FACTORS == 128 and bl.LMF(regularization=0.0, learning_rate=0.0).regularization == 0.0
    assert bl.ColTrackLMF().factors == 128 and bl.TrackTrackLMF(factors=64).factors == 64
    assert bl.ColTrackLMF().algo == "lmf"
    for name in ("LMF", "LMF_MAX_FACTORS", "lmf_objective", "ColTrackLMF", "TrackTrackLMF"):
        assert name in bl.__all__
    # the ALS classes keep refusing algo="lmf"; the new classes are the way in
    with pytest.raises(NotImplementedError, match="ColTrackLMF"):
        bl.ColTrackCF(algo="lmf")
    assert issubclass(bl.ColTrackLMF, bl.PredictionModel) and bl.ColTrackLMF.knn is bl.ColTrackCF.knn


def test_row_form_predicate_and_the_library_constants():
    import _native as nat
    L = nat.lib()
    long_row = int(L.pinsage_lmf_long_row())
    assert long_row == 512 and int(L.pinsage_lmf_row_block()) == 128
    assert lu.row_form(long_row, long_row) == "wave" and lu.row_form(long_row + 1, long_row) == "workgroup"
