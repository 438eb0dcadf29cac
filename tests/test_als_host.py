"""Host checks of the ALS path's numpy references (tests/als_util.py) and of the
host-runnable pieces of baselines.py that stand beside the kernels: the two
matrix builders (run on the CPU through their ``device`` argument) and als_loss.

The references are what tests/test_gpu_als.py holds the device to, so they are
checked against what does not share their code: the conjugate-gradient
restatement against numpy.linalg.solve, the objective against its own descent,
the builders against scipy lil_matrix loops in the reference's manner, and each
planted defect has to be caught by the check meant for it.
"""
import numpy as np
import pytest
import torch

import als_util as au
from conftest import golden


def _case(f, seed, kind="counts", n_rows=23, n_cols=31):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 12, n_rows)
    lengths[0], lengths[1] = 0, n_cols
    csr = au.random_csr(rng, lengths, n_cols, kind)
    return csr, au.init_factors(rng, n_rows, f), au.init_factors(rng, n_cols, f)


def _cg_gap(csr, X, Y, reg, alpha, defect=None):
    got = au.half_iteration(*csr[:3], X, Y, reg, alpha, 40, np.float64, defect=defect)
    want = au.exact_rows(*csr[:3], Y, reg, alpha)
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("f", [16, 128])
@pytest.mark.parametrize("alpha,kind", [(1.0, "counts"), (40.0, "counts"), (0.5, "fractions"), (1.0, "ones")])
def test_cg_restatement_reaches_the_exact_solve(f, alpha, kind):
    csr, X, Y = _case(f, seed=f + int(alpha), kind=kind)
    gap = _cg_gap(csr, X, Y, 0.01, alpha)
    print(f"f = {f}, alpha = {alpha}, {kind}: float64 CG at 40 steps vs solve, relative to the largest entry {gap:.2e}")
    assert gap < 1e-8


@pytest.mark.parametrize("defect", au.DEFECTS[:2])
def test_cg_check_rejects_planted_defects(defect):
    csr, X, Y = _case(16, seed=3)
    assert _cg_gap(csr, X, Y, 0.01, 2.0) < 1e-8
    assert _cg_gap(csr, X, Y, 0.01, 2.0, defect=defect) > 1e-5


def test_zero_steps_and_zero_rows():
    csr, X, Y = _case(8, seed=4)
    for dt in (np.float32, np.float64):
        assert np.array_equal(au.half_iteration(*csr[:3], X, Y, 0.01, 1.0, 0, dt), X.astype(dt))
    X[0] = 0                                         # row 0 has no items: r = 0, the row stays
    out = au.half_iteration(*csr[:3], X, Y, 0.01, 1.0, 3, np.float32)
    assert not out[0].any() and np.abs(out[1]).max() > 0


@pytest.mark.parametrize("f", [16, 128])
def test_loss_does_not_increase_over_15_iterations(f):
    csr, _, _ = _case(f, seed=5, n_rows=40, n_cols=30)
    g = torch.Generator().manual_seed(7)             # the documented init, users first
    X = ((torch.rand(40, f, generator=g) - 0.5) / f).numpy()
    Y = ((torch.rand(30, f, generator=g) - 0.5) / f).numpy()
    losses = [au.loss(csr, X, Y, 0.01, 1.0)]
    for _ in range(15):
        X, Y = au.fit(csr, X, Y, 0.01, 1.0, 3, 1, np.float64)
        losses.append(au.loss(csr, X, Y, 0.01, 1.0))
    assert all(b <= a * (1 + 1e-12) for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.5 * losses[0]


def test_fit_check_rejects_items_first():
    csr, X, Y = _case(16, seed=6)
    want = au.fit(csr, X, Y, 0.01, 1.0, 3, 15, np.float64)
    f32 = au.fit(csr, X, Y, 0.01, 1.0, 3, 15, np.float32)
    bad = au.fit(csr, X, Y, 0.01, 1.0, 3, 15, np.float64, defect="items_first")
    for t in (0, 1):
        tol = au.TOL_FACTOR * au.table_error(f32[t], want[t])
        print(f"table {t}: float32 restatement after 15 iterations {tol / au.TOL_FACTOR:.2e}")
        assert tol < 1e-4 and au.table_error(bad[t], want[t]) > tol


def test_error_measure():
    x64 = np.array([[3.0, 4.0], [0.0, 0.0], [0.0, 0.0]])
    x = np.array([[3.0, 4.5], [0.0, 1e-3], [0.0, 0.0]])
    x_in = np.array([[0.0, 0.0], [0.6, 0.8], [0.0, 0.0]])
    assert np.allclose(au.row_errors(x, x64, x_in), [0.1, 1e-3, 0.0])


# ----------------------------------------------------------------------------- als_loss
@pytest.mark.parametrize("alpha,kind", [(1.0, "ones"), (40.0, "counts"), (0.5, "fractions")])
def test_als_loss_equals_the_dense_objective(alpha, kind):
    import baselines as bl
    csr, X, Y = _case(16, seed=8, kind=kind)
    X, Y = X * 7, Y * 7                              # products of order 1, so that every term counts
    t = tuple(torch.from_numpy(a) for a in csr[:3]) + csr[3:]
    got = bl.als_loss(t, torch.from_numpy(X), torch.from_numpy(Y), 0.01, alpha)
    want = au.loss(csr, X, Y, 0.01, alpha)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert abs(au.loss(csr, X, Y, 0.02, alpha) - want) > 1e-6 * abs(want)


# ----------------------------------------------------------------------------- the matrix builders
def _lil_col_track(g, n_tracks):
    """The reference's loop: per collection the set of its neighbours either way."""
    from scipy.sparse import lil_matrix
    n_cols = len(g) - n_tracks
    m = lil_matrix((n_cols, n_tracks), dtype=np.int32)
    for c in range(n_cols):
        node = n_tracks + c
        members = sorted(set(g.successors(node).tolist()) | set(g.predecessors(node).tolist()))
        m[c, members] = 1
    return m.tocsr()


def _lil_track_track(n, positives):
    from scipy.sparse import lil_matrix
    m = lil_matrix((n, n), dtype=np.int32)
    for a, b in sorted(np.asarray(positives).tolist(), key=lambda ab: ab[1]):
        m[a, b] = m[a, b] + 1
    return m.tocsr()


def _same(got, want):
    ptr, idx, val, n_rows, n_cols = got
    assert (n_rows, n_cols) == want.shape
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int32 and val.dtype == torch.float32
    want.sort_indices()
    assert np.array_equal(ptr.numpy(), want.indptr) and np.array_equal(idx.numpy(), want.indices)
    assert np.array_equal(val.numpy(), want.data.astype(np.float32))


def test_col_track_matrix_matches_the_lil_loop():
    import baselines as bl
    import graph
    n, nc = 12, 5          # collection 3 is empty, track 11 is in no collection
    e = np.array([[12, 0], [12, 1], [1, 12], [12, 1], [13, 1], [2, 13], [13, 5], [14, 5], [14, 6], [7, 14],
                  [16, 9], [9, 16], [16, 10], [3, 4], [4, 3], [8, 8]])   # a duplicate edge, both directions, track-track
    g = graph.CSRGraph(n + nc, e[:, 0], e[:, 1])
    got = bl.to_col_track_matrix(g, list(range(n)), device="cpu")
    _same(got, _lil_col_track(g, n))
    assert int(got[0][4] - got[0][3]) == 0 and not (got[1] == 11).any() and (got[2] == 1).all()
    f = golden("jaccard")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    edges = f["edges"].astype(np.int64)
    g = graph.CSRGraph(n + nc, edges[:, 0], edges[:, 1])
    _same(bl.to_col_track_matrix(g, list(range(n)), device="cpu"), _lil_col_track(g, n))
    with pytest.raises(ValueError):
        g2 = graph.CSRGraph(n + nc, np.append(edges[:, 0], n), np.append(edges[:, 1], n + 1))
        bl.to_col_track_matrix(g2, list(range(n)), device="cpu")
    with pytest.raises(ValueError):
        bl.to_col_track_matrix(g, list(range(n + nc + 1)), device="cpu")


def test_track_track_matrix_matches_the_lil_loop():
    import baselines as bl
    n = 9
    pos = np.array([[0, 1], [2, 2], [0, 1], [1, 0], [5, 3], [0, 1], [5, 8], [5, 3], [7, 0]])  # repeats, a == b
    got = bl.to_track_track_matrix(list(range(n)), torch.from_numpy(pos), device="cpu")
    _same(got, _lil_track_track(n, pos))
    assert float(got[2][0]) == 3.0                   # (0, 1) three times; (1, 0) is another cell
    rng = np.random.default_rng(9)
    pos = rng.integers(0, 40, (400, 2))
    _same(bl.to_track_track_matrix(list(range(40)), pos, device="cpu"), _lil_track_track(40, pos))
    _same(bl.to_track_track_matrix(list(range(4)), np.zeros((0, 2), np.int64), device="cpu"), _lil_track_track(4, []))
    for bad in ([[0, 9]], [[-1, 2]]):
        with pytest.raises(IndexError):
            bl.to_track_track_matrix(list(range(n)), np.array(bad), device="cpu")


def test_constructors_refuse_what_is_documented():
    import baselines as bl
    for algo in ("lmf", "bpr"):
        for cls in (bl.ColTrackCF, bl.TrackTrackCF):
            with pytest.raises(NotImplementedError, match="ALS"):
                cls(algo=algo)
    assert bl.ColTrackCF().factors == 128 and bl.TrackTrackCF(factors=64).factors == 64
    for kw in ({"factors": 6}, {"factors": 132}, {"factors": 0}, {"regularization": 0.0}, {"alpha": -1.0},
               {"cg_steps": -1}):
        with pytest.raises(ValueError):
            bl.ALS(**kw)
    m = bl.ALS()
    assert (m.factors, m.regularization, m.alpha, m.iterations, m.cg_steps, m.random_state) == \
        (128, 0.01, 1.0, 15, 3, None)
    for name in ("ALS", "als_loss", "to_col_track_matrix", "to_track_track_matrix", "ColTrackCF", "TrackTrackCF"):
        assert name in bl.__all__


def test_row_form_predicate_and_the_library_constants():
    import _native as nat
    L = nat.lib()
    long_row, per_block = int(L.pinsage_als_long_row()), int(L.pinsage_als_rows_per_block())
    assert long_row >= 64 and per_block >= 1
    assert au.row_form(long_row, long_row) == "wave" and au.row_form(long_row + 1, long_row) == "workgroup"
