"""The restatements of tests/sage_util.py checked on the host, and the host side
of baselines.SAGE / GraphSAGE: constructor refusals, defaults, the docstring.
No GPU.

The sampler.  On n2v_util.small_graph (fanout 2 and 10) and on one row of
degree 40 (fanout 10), over 4000 rounds, the inclusion frequency of every edge
has to lie within 5 sqrt(pi (1 - pi) / 4000) of pi = S / deg (a row with
deg <= S is returned whole, in order, every round), no sample may repeat a
position and the weights have to sum to 1 within 2 ulp; each planted defect of
sage_util.SAMPLER_DEFECTS has to fail that check.  Seeds and sizes are fixed:
5 sigmas over about 60 frequencies leaves a false alarm at about 4e-5 per run,
and these runs pass (the rule of tests/test_n2v_host.py).

The loss.  margin_loss's float64 gradient is held against central differences
(step 1e-6) of the scalar loss, relative error (largest difference over the
largest entry) below 1e-6, as the host tests of LMF and node2vec do: hinge on
(margin 3) and off for some anchors (margin 0.05), a duplicated positive row (an
exact tie) and void slots; each planted defect of sage_util.LOSS_DEFECTS has to
fail it.  The full step's dW1 and dW2 are checked the same way on a 30-node
graph.
"""
import numpy as np
import pytest

import n2v_util as nu
import sage_util as su

ROUNDS = 4000
TIES = ((4, 1, 3), (5, 5, 7))   # (group, lower slot, higher slot) of loss_case's duplicated rows


def hub_graph():
    """Node 0 tied to nodes 1 .. 40 with weights 1 .. 4, nothing else."""
    return nu.graph_from_edges(41, [(0, v, 1 + v % 4) for v in range(1, 41)])


def sampler_verdict(defect):
    """(worst sigmas, worst |frequency - 1| of whole rows, repeated, weight-sum ulps) over the three cases."""
    out = np.zeros(4)
    for graph, nodes, S in ((nu.small_graph(), range(7), 2), (nu.small_graph(), range(7), 10), (hub_graph(), [0], 10)):
        out = np.maximum(out, np.array(su.sample_check(graph, nodes, S, 5, ROUNDS, defect), float))
    return out


def test_sampler_frequencies_match_the_definition():
    worst, short, repeat, ulps = sampler_verdict(None)
    print(f"worst deviation {worst:.2f} sigmas, whole rows off by {short}, weight sums off by {ulps:.2f} ulp")
    assert worst < 5 and short == 0 and not repeat and ulps <= 2


@pytest.mark.parametrize("defect", su.SAMPLER_DEFECTS)
def test_sampler_check_rejects_planted_defects(defect):
    worst, short, repeat, ulps = sampler_verdict(defect)
    print(f"{defect}: {worst:.1f} sigmas, repeated {bool(repeat)}, weight sums off by {ulps:.3g} ulp")
    assert worst >= 5 or repeat or ulps > 2


def test_sampler_invariants():
    g = nu.edge_graph()
    stats = {}
    nb, w = su.neighbours(g, np.arange(75), 10, 3, 7, stats=stats)
    ptr, idx = g[:2]
    assert stats["collisions"] >= 1
    for v in range(75):
        row = idx[ptr[v]:ptr[v + 1]]
        keep = nb[v] >= 0
        assert len(set(nb[v][keep])) == keep.sum() == min(10, len(row)) and set(nb[v][keep]) <= set(row)
        if len(row) <= 10:
            assert (nb[v][:len(row)] == row).all() and (w[v][len(row):] == 0).all()
        if len(row):
            tot = np.float32(0)
            for x in w[v]:
                tot = np.float32(tot + x)
            assert abs(float(tot) - 1) <= 2 * 2.0 ** -23
    assert (nb[71] == -1).all() and (w[71] == 0).all()          # the isolated node
    a, b = su.neighbours(g, [0, 5, 0], 10, 3, 7)
    assert (a[0] == a[2]).all() and (b[0] == b[2]).all()          # a function of (seed, round, node)
    assert not (su.neighbours(g, [0], 10, 3, 8)[0] == a[0]).all()  # and the round matters


def test_negatives_avoid_the_anchor_and_its_row():
    g = nu.edge_graph()
    ptr, idx = g[:2]
    neg = su.negatives(g, np.arange(75), 6, 9, 4)
    assert (neg[0] >= 0).sum() < 36                               # the hub: 70 of 75 nodes are neighbours
    for a in range(75):
        for j in neg[a][neg[a] >= 0]:
            assert j != a and j not in idx[ptr[a]:ptr[a + 1]]
    star = nu.graph_from_edges(6, [(0, v, 1) for v in range(1, 6)])
    assert (su.negatives(star, [0, 0], 16, 9, 0) == -1).all()   # adjacent to all others: only void samples
    assert (su.negatives(star, [1], 16, 9, 0) >= 2).all()


def loss_case(margin, seed=0):
    """8 groups of P = 4, Q = 3 in d = 12: void slots, a group without negatives,
    an exact tie between two positives and between two negatives."""
    rng = np.random.default_rng(seed)
    B, P, Q, d = 8, 4, 3, 12
    G = 1 + P + Q
    Z = rng.standard_normal((B, G, d))
    slots = rng.integers(0, 50, (B, G)).astype(np.int32)
    slots[1, 2] = slots[1, 6] = slots[2, 1] = -1
    slots[3, 1 + P:] = -1                                       # inactive: no negative
    Z[4, 1] = -Z[4, 0] + 0.3 * Z[4, 1]                          # the smallest positive cosine ..
    Z[4, 3] = Z[4, 1]                                           # .. twice
    Z[5, 5] = Z[5, 0] + 0.3 * Z[5, 5]                           # the largest negative cosine ..
    Z[5, 7] = Z[5, 5]                                           # .. twice
    Z[6, 1:1 + P] = Z[6, 0] + 0.2 * Z[6, 1:1 + P]               # positives near the anchor, negatives opposite:
    Z[6, 1 + P:] = -Z[6, 0] + 0.2 * Z[6, 1 + P:]                # off the hinge at margin 0.05, on it at 3
    return Z.reshape(B * G, d), slots, P, Q, margin


def loss_gradient_error(case, defect=None, h=1e-6):
    Z, slots, P, Q, margin = case
    f = lambda z: float(su.margin_loss(z, slots, P, Q, margin, np.float64)[0].sum()
                        / max(1, int(su.margin_loss(z, slots, P, Q, margin, np.float64)[1].sum())))
    dZ = su.margin_loss(Z, slots, P, Q, margin, np.float64, defect=defect)[3]
    num = np.zeros_like(Z)
    for i in np.ndindex(*Z.shape):
        zp, zm = Z.copy(), Z.copy()
        zp[i] += h
        zm[i] -= h
        num[i] = (f(zp) - f(zm)) / (2 * h)
    # at an exact tie the min (max) has a kink: moving either of the two equal rows one way moves the
    # loss, the other way does not, so each central difference is half a one-sided slope and the two
    # add up to the gradient of the chosen (lower) slot; fold the higher row onto the lower in both
    G = 1 + P + Q
    dZ, num = dZ.copy(), num.copy()
    for a, lo, hi in TIES:
        for arr in (dZ, num):
            arr[a * G + lo] += arr[a * G + hi]
            arr[a * G + hi] = 0
    return np.abs(dZ - num).max() / np.abs(num).max()


@pytest.mark.parametrize("margin", [3.0, 0.05])
def test_loss_gradient_against_central_differences(margin):
    case = loss_case(margin)
    loss, active, sel, dZ = su.margin_loss(*case, np.float64)
    on = loss > 0
    print(f"margin {margin}: {int(on.sum())} of {int(active.sum())} active anchors on the hinge")
    assert active.tolist() == [1, 1, 1, 0, 1, 1, 1, 1] and loss[3] == 0 and sel[3].tolist()[1] == -1
    assert on.any() and (margin == 3.0 or (~on & (active == 1)).any())
    assert sel[4, 0] == 1 and sel[5, 1] == 5                    # ties go to the lower slot
    G = 1 + case[2] + case[3]
    rows = dZ.reshape(len(loss), G, -1)
    for a in range(len(loss)):                                  # only a, pos*, neg* receive gradient
        for g in range(1, G):
            assert g in sel[a] or not rows[a, g].any()
    err = loss_gradient_error(case)
    print(f"relative error {err:.2e}")
    assert err < 1e-6


@pytest.mark.parametrize("defect", su.LOSS_DEFECTS)
def test_loss_check_rejects_planted_defects(defect):
    err = loss_gradient_error(loss_case(3.0), defect)
    print(f"{defect}: relative error {err:.2e}")
    assert err > 1e-3


def test_zero_rows_and_void_groups_stay_finite():
    Z, slots, P, Q, margin = loss_case(3.0)
    Z = Z.copy()
    Z[0] = 0                                                    # a zero anchor
    Z[1 * 8 + 1] = 0                                            # a zero positive
    slots[6, 1:] = -1
    for dt in (np.float64, np.float32):
        loss, active, sel, dZ = su.margin_loss(Z, slots, P, Q, margin, dt)
        assert np.isfinite(loss).all() and np.isfinite(dZ).all() and active[6] == 0 and (sel[6] == -1).all()
        assert not dZ.reshape(8, 8, -1)[6].any() and loss[6] == 0


def test_gaussian_seeds_leave_out_no_anchor():
    """The inputs of the GPU loss test at P = 16, Q = 6, d = 128: with seeds 1 to 3
    no runner-up gap falls below the 1e-5 under which an anchor may be left out."""
    for seed in (1, 2, 3):
        Z, slots = su.loss_inputs(128, 16, 6, seed)
        assert su.runner_up_gaps(Z, slots, 16, 6).min() >= 1e-5


@pytest.fixture(scope="module")
def small_step():
    rng = np.random.default_rng(4)
    edges = {(min(a, b), max(a, b)) for a, b in rng.integers(0, 30, (90, 2)) if a != b}
    g = nu.graph_from_edges(30, [(a, b, int(rng.integers(1, 5))) for a, b in sorted(edges)])
    prm = dict(su.DEFAULTS, num_sample=3, n_walks=2, walk_len=2, negatives=2, batch_size=6, emb_size=8)
    tb = su.tables(g, np.arange(6) * 5, 1, prm, 77)
    X0 = rng.standard_normal((30, 4))
    W1, W2 = rng.standard_normal((8, 8)) * 0.5, rng.standard_normal((8, 16)) * 0.5
    return tb, X0, W1, W2, prm


def test_step_gradient_against_central_differences(small_step):
    tb, X0, W1, W2, prm = small_step
    st = su.step(tb, X0, W1, W2, prm, np.float64)
    assert st["loss"] > 0 and st["active"].sum() >= 3
    assert abs(float(st["loss"]) - su.scalar_loss(tb, X0, W1, W2, prm)) < 1e-12
    h = 1e-6
    for k, (W, dW) in enumerate(((W1, st["dW1"]), (W2, st["dW2"]))):
        num = np.zeros_like(W)
        for i in np.ndindex(*W.shape):
            Wp, Wm = W.copy(), W.copy()
            Wp[i] += h
            Wm[i] -= h
            args = (lambda w: (tb, X0, w, W2, prm)) if k == 0 else (lambda w: (tb, X0, W1, w, prm))
            num[i] = (su.scalar_loss(*args(Wp)) - su.scalar_loss(*args(Wm))) / (2 * h)
        err = np.abs(dW - num).max() / np.abs(num).max()
        print(f"dW{k + 1}: relative error {err:.2e}")
        assert err < 1e-6
    st32 = su.step(tb, X0, W1, W2, prm, np.float32)
    assert st32["dW1"].dtype == np.float32 and (st32["sel"] == st["sel"]).all()
    assert np.abs(st32["dW2"] - st["dW2"]).max() <= 1e-4 * np.abs(st["dW2"]).max()


def test_adam_is_the_reference_recurrence():
    import parity_util as pu
    rng = np.random.default_rng(2)
    p, g, m, v = (rng.standard_normal(200).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    ref = pu.adam_reference(p, g, m, v, su.adam_coef(3, 1e-3))
    for dt in (np.float64, np.float32):
        got = su.adam(p, g, m, v, 3, 1e-3, dt)
        assert (np.abs(got[0] - ref["p"]) <= (1e-12 if dt is np.float64 else 1) * np.maximum(ref["E_p"], 1e-300)).all()
        assert (np.abs(got[1] - ref["m"]) <= ref["E_m"] + 1e-12).all() and (np.abs(got[2] - ref["v"]) <= ref["E_v"] + 1e-12).all()


def test_constructors_refuse_what_is_documented():
    import baselines as bl
    inf, nan = float("inf"), float("nan")
    for kw in ({"emb_size": 6}, {"emb_size": 516}, {"emb_size": 0}, {"num_sample": 0}, {"num_sample": 33},
               {"n_walks": 0}, {"walk_len": 0}, {"n_walks": 13, "walk_len": 5}, {"negatives": 0}, {"negatives": 17},
               {"margin": inf}, {"margin": nan}, {"learning_rate": -1e-3}, {"learning_rate": nan}, {"epochs": -1},
               {"batch_size": 0}):
        with pytest.raises(ValueError):
            bl.SAGE(**kw)
    for kw in ({"emb_size": 512}, {"num_sample": 32}, {"n_walks": 16, "walk_len": 4}, {"negatives": 16}):
        bl.SAGE(**kw)                                            # the limits themselves are accepted
    m = bl.SAGE()
    assert {k: getattr(m, k) for k in su.DEFAULTS} == su.DEFAULTS
    assert m.weights is None and m.losses is None and m.gemm_prec == -1
    assert (bl.SAGE_MAX_FANOUT, bl.SAGE_MAX_POSITIVES, bl.SAGE_MAX_NEGATIVES, bl.SAGE_MAX_DIM) == (32, 64, 16, 512)
    assert bl.SAGE_BETAS == su.BETAS and bl.SAGE_EPS == su.EPS
    gm = bl.GraphSAGE()
    assert gm.projected is True and gm.embedding is None and issubclass(bl.GraphSAGE, bl.EmbeddingModel)
    with pytest.raises(NotImplementedError):
        bl.GraphSAGE(projected=False).train(None, [], None, None, None)


def test_docstring_and_exports():
    import _native as nat
    import baselines as bl
    scope = [p for p in bl.__doc__.split("\n\n") if "out of scope" in p]
    assert len(scope) == 1 and "lib/gnns" not in scope[0]       # no longer listed as out of scope
    assert "GraphSAGE" in bl.__doc__ and "one hop" in bl.SAGE.__doc__.lower() and "unmeasured" in bl.SAGE.__doc__
    for name in ("pinsage_sage_neighbours", "pinsage_sage_negatives", "pinsage_sage_margin_loss",
                 "pinsage_sage_lrelu_backward"):
        assert name in nat.EXPORTED and hasattr(nat.lib(), name)
