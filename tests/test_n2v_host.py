"""The references of tests/n2v_util.py checked on the host, and the host side of
baselines.Node2Vec: n2v_cooccurrence against a triple loop, sgns_objective
against the dense objective, constructor refusals and defaults.  No GPU.

The walk.  On n2v_util.small_graph (7 nodes, weights 1 .. 5) the restatement's
next-node frequencies after every (prev, cur) seen N >= 200 times have to lie
within 5 sqrt(pi (1 - pi) / N) of the exact pi proportional to weight * beta;
each planted defect of n2v_util.WALK_DEFECTS has to fail that check.  Seeds and
sizes are fixed: 5 sigmas over about 100 frequencies leaves a false alarm at
about 6e-5 per run, and these runs pass.

The fit.  The gradient a half-iteration uses is read back from its outputs (from
zero accumulators h_new = g^2 and the step has g's sign) and held against
central differences of the float64 objective, step 1e-5, relative error (largest
difference over the largest entry, per table) below 1e-6, as
tests/test_lmf_host.py does; each planted defect of n2v_util.FIT_DEFECTS has to
fail it.
"""
import numpy as np
import pytest
import torch

import lmf_util as lu
import n2v_util as nu

P_Q = [(2.0, 0.5), (0.5, 2.0)]


@pytest.fixture(scope="module")
def small_walks():
    """{(p, q, defect): walks}: 100 walks of 40 from each of the 7 nodes."""
    g = nu.small_graph()
    starts = np.tile(np.arange(7), 100)
    out = {}
    for p, q in P_Q:
        out[p, q, None] = nu.walk(g, starts, 40, 1 / p, 1 / q, seed=11)
    for defect in nu.WALK_DEFECTS:
        out[2.0, 0.5, defect] = nu.walk(g, starts, 40, 0.5, 2.0, seed=11, defect=defect)
    return g, out


@pytest.mark.parametrize("p,q", P_Q)
def test_walk_frequencies_match_the_definition(small_walks, p, q):
    g, walks = small_walks
    w = walks[p, q, None]
    assert w.dtype == np.int32 and (w[:, 0] == np.tile(np.arange(7), 100)).all() and (w >= 0).all()
    ptr, idx = g[:2]
    for row in w[:50]:                                       # every step follows an edge
        for a, b in zip(row[:-1], row[1:]):
            assert b in idx[ptr[a]:ptr[a + 1]]
    worst, pairs = nu.transition_check(g, w, 1 / p, 1 / q)
    print(f"p = {p}, q = {q}: {pairs} (prev, cur) pairs, worst deviation {worst:.2f} sigmas")
    assert pairs >= 15 and worst < 5


@pytest.mark.parametrize("defect", nu.WALK_DEFECTS)
def test_walk_check_rejects_planted_defects(small_walks, defect):
    g, walks = small_walks
    worst, pairs = nu.transition_check(g, walks[2.0, 0.5, defect], 0.5, 2.0)
    print(f"{defect}: worst deviation {worst:.1f} sigmas")
    assert pairs >= 15 and worst > 8


def test_walk_edges_of_the_definition():
    g = nu.edge_graph()
    ptr, idx, cum, n = g
    assert (np.diff(ptr) > 64).any() and int(cum[ptr[73] - 1]) > 1 << 32 and ptr[72] == ptr[71]
    w = nu.walk(g, [71, 11, 72, 0], 6, 0.5, 2.0, seed=3)
    assert (w[0] == [71, -1, -1, -1, -1, -1]).all()          # an isolated start
    assert w[1, 1] == 0 and (w[1] >= 0).all()                # a leaf's only edge
    assert w[2, 1] == 73                                     # 2^33 against 3: try 0 of this seed takes the heavy edge
    for j in range(2, 6):                                    # whoever enters a leaf comes back
        for k in range(4):
            if 11 <= w[k, j - 1] <= 70:
                assert w[k, j] == 0
    # a walk is a prefix of the longer walk, and depends on its position only
    assert (nu.walk(g, [11], 3, 0.5, 2.0, seed=3, walk_base=1)[0] == w[1, :3]).all()
    assert not (nu.walk(g, [11], 6, 0.5, 2.0, seed=3, walk_base=0) == w[1]).all()
    # unweighted: the pick is the edge's index
    u = nu.walk((ptr, idx, None, n), [0] * 40, 2, 1.0, 1.0, seed=5)
    assert len(set(u[:, 1])) > 15


def test_cooccurrence_matches_the_triple_loop(monkeypatch):
    import baselines as bl
    rng = np.random.default_rng(1)
    walks = rng.integers(0, 9, (23, 7)).astype(np.int32)
    walks[3, 4:] = -1
    walks[5, 1:] = -1
    walks[8, :] = -1
    for context in (1, 3, 6, 10):
        want = nu.cooccurrence_loops(walks, 9, context)
        assert (want == want.T).all()
        for scratch in (bl.KNN_SCRATCH_BYTES, 1):            # one chunk, and a walk per chunk
            monkeypatch.setattr(bl, "KNN_SCRATCH_BYTES", scratch)
            ptr, idx, val, n, m = bl.n2v_cooccurrence(torch.from_numpy(walks), 9, context)
            assert (n, m) == (9, 9) and ptr.dtype == torch.int64 and idx.dtype == torch.int32
            assert val.dtype == torch.float32 and bool((val > 0).all())
            got = nu.dense_of((ptr.numpy(), idx.numpy(), val.numpy(), 9))
            assert np.array_equal(got, want), context
            for u in range(9):                               # ascending ids within a row
                assert (np.diff(idx[ptr[u]:ptr[u + 1]].numpy()) > 0).all()
    with pytest.raises(IndexError):
        bl.n2v_cooccurrence(torch.from_numpy(walks), 8, 2)
    with pytest.raises(ValueError):
        bl.n2v_cooccurrence(torch.from_numpy(walks[0]), 9, 2)
    with pytest.raises(ValueError):
        bl.n2v_cooccurrence(torch.from_numpy(walks), 9, 0)


def _fit_case(f, seed, n=8, scale=0.5):
    rng = np.random.default_rng(seed)
    walks = rng.integers(0, n - 1, (12, 6)).astype(np.int32)  # node n - 1 never occurs
    C = nu.csr_of(nu.cooccurrence_loops(walks, n, 2))
    cnt, P = nu.noise(C)
    assert cnt[n - 1] == 0 and P[n - 1] == 0 and abs(float(P.sum()) - 1) < 1e-6
    return C, rng.normal(0, scale, (n, f)), rng.normal(0, scale, (n, f)), cnt, P.astype(np.float64)


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


def _gradient_gap(C, U, V, cnt, P, K, reg, defect=None):
    """The largest relative error of the implied gradient over the two tables."""
    U, V = np.array(U, np.float64), np.array(V, np.float64)
    L = lambda: nu.objective(C, U, V, K, P, reg)  # noqa: E731
    worst = 0.0
    for half, (X, Y) in enumerate(((U, V), (V, U))):
        cw, rw = nu.half_weights(cnt, P, K, half, defect)
        xn, h = nu.half_iteration(*C[:3], rw, X, np.zeros_like(X), Y, cw, reg, 0.1, np.float64)
        want = _central(L, X)
        got = lu.implied_gradient(X, xn, h)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    return worst


@pytest.mark.parametrize("f,K,reg", [(4, 5.0, 0.0), (8, 1.0, 0.3), (4, 20.0, 0.05)])
def test_gradient_matches_central_differences(f, K, reg):
    gap = _gradient_gap(*_fit_case(f, seed=f + int(K)), K, reg)
    print(f"f = {f}, K = {K}, reg = {reg}: relative error {gap:.2e}")
    assert gap < 1e-6


@pytest.mark.parametrize("defect", nu.FIT_DEFECTS)
def test_gradient_check_rejects_planted_defects(defect):
    case = _fit_case(4, seed=3)
    assert _gradient_gap(*case, 5.0, 0.1) < 1e-6
    assert _gradient_gap(*case, 5.0, 0.1, defect=defect) > 1e-3


def test_sgns_objective_equals_the_dense_objective(monkeypatch):
    import baselines as bl
    C, U, V, cnt, P = _fit_case(8, seed=9, n=11)
    U, V = U.astype(np.float32), V.astype(np.float32)
    want = nu.objective(C, U, V, 5.0, P, 0.3)
    t = tuple(torch.from_numpy(a) for a in C[:3]) + C[3:]
    args = (t, torch.from_numpy(U), torch.from_numpy(V), 5.0, torch.from_numpy(P), 0.3)
    got = bl.sgns_objective(*args)
    assert isinstance(got, float) and abs(got - want) <= 1e-12 * abs(want), (got, want)
    monkeypatch.setattr(bl, "_LMF_CELLS", 22)                # row chunks of 2 rows
    got = bl.sgns_objective(*args)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_objective_rises_on_the_planted_graph():
    """The float32 restatement on counts from the restatement's own walks: L rises
    on each of the 30 iterations and stays within 1e-6 of float64's."""
    (g, groups) = nu.planted_graph(1)
    n = g[3]
    walks = nu.walk(g, np.tile(np.arange(n), 2), 12, 0.5, 2.0, seed=1)
    C = nu.csr_of(nu.cooccurrence_loops(walks, n, 5))
    cnt, P = nu.noise(C)
    rng = np.random.default_rng(16)
    U0, V0 = ((rng.random((n, 16)) - 0.5) / 16).astype(np.float32), ((rng.random((n, 16)) - 0.5) / 16).astype(np.float32)
    start = nu.objective(C, U0, V0, 5.0, P, 0.0)
    seen32 = nu.fit(C, U0, V0, cnt, P, 5.0, 0.0, 0.1, 30, np.float32, trace=True)[2]
    U64, _, seen64 = nu.fit(C, U0, V0, cnt, P, 5.0, 0.0, 0.1, 30, np.float64, trace=True)
    print(f"L {start:.6g} -> {seen32[0]:.6g} -> {seen32[-1]:.6g}, float64 {seen64[-1]:.6g}")
    assert (np.diff([start] + seen32) > 0).all() and (np.diff([start] + seen64) > 0).all()
    assert abs(seen32[-1] - seen64[-1]) <= 1e-6 * abs(seen64[-1])
    connected = np.flatnonzero(np.diff(g[0]) > 0)
    share = nu.same_group_share(U64, groups, connected)
    print(f"{len(connected)} of {n} tracks have edges; top-10 same-group share {share:.3f}")
    assert len(connected) < n and share >= 0.5


def test_constructors_refuse_what_is_documented():
    import baselines as bl
    inf, nan = float("inf"), float("nan")
    for kw in ({"dim": 6}, {"dim": 132}, {"dim": 0}, {"walk_length": 0}, {"walk_length": 1 << 24}, {"context": 0},
               {"walks_per_node": 0}, {"p": 0.0}, {"q": -1.0}, {"p": inf}, {"q": nan}, {"p": 17.0, "q": 1.0},
               {"p": 8.0, "q": 0.25}, {"p": 0.05, "q": 1.0}, {"negative": 0.0}, {"negative": inf},
               {"ns_exponent": -0.5}, {"ns_exponent": nan}, {"learning_rate": -0.1}, {"learning_rate": nan},
               {"regularization": -0.1}, {"regularization": inf}, {"iterations": -1}):
        with pytest.raises(ValueError):
            bl.Node2Vec(**kw)
    for kw in ({"p": 16.0, "q": 1.0}, {"p": 4.0, "q": 0.25}, {"p": 0.25, "q": 4.0}, {"p": 1.0, "q": 0.0625}):
        bl.Node2Vec(**kw)                                    # the ratio limit itself is accepted
    m = bl.Node2Vec()
    assert {k: getattr(m, k) for k in nu.DEFAULTS} == nu.DEFAULTS
    assert m.factors == 128 and m.embedding is None and m.context_factors is None and m.cooccurrence is None
    assert bl.N2V_MAX_BIAS_RATIO == 16.0
    fm = bl.FastNode2Vec()
    assert fm.projected is True and fm.embedding is None and bl.FastNode2Vec(projected=False).projected is False
    assert issubclass(bl.FastNode2Vec, bl.EmbeddingModel) and issubclass(bl.Node2Vec, bl._RowFit)


def test_exports():
    import _native as nat
    import baselines as bl
    for name in ("pinsage_n2v_walk", "pinsage_sgns_dense", "pinsage_sgns_update"):
        assert name in nat.EXPORTED and hasattr(nat.lib(), name)
    for name in ("project_bipartite_graph", "bipartite_graph", "n2v_cooccurrence", "sgns_objective",
                 "N2V_MAX_BIAS_RATIO", "Node2Vec", "FastNode2Vec"):
        assert name in bl.__all__ and hasattr(bl, name)
