"""The numpy / Python-int restatements of the GraphSAGE path (csrc/sage.hip,
baselines.SAGE), shared by tests/test_gpu_sage.py (on the GPU) and
tests/test_sage_host.py (which checks the restatements themselves on the host).
The Philox generator is oracle's, the walk n2v_util's, sigmoid and softplus
lmf_util's.  A graph is n2v_util's tuple (ptr, idx, cum or None, n).

Neighbour sample (rnd, v), fanout S, deg = the length of row v:
    deg <= S: positions 0 .. deg - 1, the other slots void (nb = -1, w = 0)
    else for j < S:  m = deg - S + j + 1
        (r0, r1, r2, r3) = philox(seed, (rnd * 64 + j, v lo, v hi, offset))
        t = ((r0 | r1 << 32) * m) >> 64;  c_j = m - 1 if t in c_0 .. c_{j-1} else t
    a_j = sqrt(float32(weight)), w_j = a_j / (a_0 + a_1 + ..) in float32, slot order
Negatives of anchor a, sample s < Q, tries k < 16:
    philox(seed, (rnd * 16 + k, (a Q + s) lo, hi, offset));  j = (r0 * n) >> 32
    accept the first j != a outside row a; -1 after 16 rejections
Step r on a batch: slots [B, G] = anchor | walk positions 1 .. walk_len of the
n_walks walks at positions (r * batch_size + i) * n_walks + w, void where -1 or
the anchor | negatives;  T = the slot nodes (void: node 0), sample (2r + 1, t);
U = unique(T and its neighbours), sample (2r, u);
    H1 = lrelu([X0[U] | Agg1] W1^T),  Z = lrelu([H1[T] | Agg2] W2^T)
    c(a, x) = z_a.z_x / max(sqrt(|z_a|^2 |z_x|^2), 1e-8)
    loss_a = max(0, log sig(max negative c) - log sig(min positive c) + margin)
    loss = sum over active anchors / max(1, #active)
Adam as torch's (parity_util.adam_reference's recurrence, here in `dtype`).
"""
import numpy as np
import torch

import n2v_util as nu
from lmf_util import sigmoid, softplus
from oracle import oracle as orc

TRIES = 16
SLOPE = 0.01
CLAMP = 1e-8
SAMPLER_DEFECTS = ("keep_collision", "modulus_short", "weights_unnormalised")
LOSS_DEFECTS = ("max_positive", "no_norm_term", "anchor_gets_no_gradient")
DEFAULTS = dict(emb_size=128, num_sample=10, n_walks=4, walk_len=4, negatives=6, margin=3.0, epochs=5, batch_size=64,
                learning_rate=1e-3, random_state=None)
BETAS, EPS = (0.9, 0.999), 1e-8


# ----------------------------------------------------------------------------- the draws
def positions(deg, S, seed, rnd, v, offset=0, defect=None, stats=None):
    """The row positions c_0 .. of sample (rnd, v) of a row of length deg."""
    if deg <= S:
        return list(range(deg))
    cs = []
    for j in range(S):
        m = deg - S + j + (0 if defect == "modulus_short" else 1)
        r = orc.philox(seed, (rnd * 64 + j, v & 0xFFFFFFFF, v >> 32, offset))
        t = (((int(r[1]) << 32) | int(r[0])) * m) >> 64
        if t in cs:
            if stats is not None:
                stats["collisions"] = stats.get("collisions", 0) + 1
            if defect != "keep_collision":
                t = m - 1
        cs.append(t)
    return cs


def neighbours(graph, nodes, S, seed, rnd, offset=0, defect=None, stats=None, cache=None):
    """(nb int32 [m, S], w float32 [m, S]) by the definition above."""
    ptr, idx, cum, n = graph
    wts = nu.weights_of(graph)
    nb = np.full((len(nodes), S), -1, np.int32)
    w = np.zeros((len(nodes), S), np.float32)
    for i, v in enumerate(nodes):
        v = int(v)
        if cache is not None and (rnd, v) in cache:
            nb[i], w[i] = cache[rnd, v]
            continue
        b, deg = int(ptr[v]), int(ptr[v + 1] - ptr[v])
        if stats is not None:
            stats.setdefault("degrees", set()).add(deg)
        cs = positions(deg, S, seed, rnd, v, offset, defect, stats)
        a = [np.sqrt(np.float32(int(wts[b + c]))) for c in cs]
        tot = np.float32(0)
        for x in a:
            tot = np.float32(tot + x)
        for j, c in enumerate(cs):
            nb[i, j] = idx[b + c]
            w[i, j] = a[j] if defect == "weights_unnormalised" else np.float32(a[j] / tot)
        if cache is not None:
            cache[rnd, v] = (nb[i].copy(), w[i].copy())
    return nb, w


def negatives(graph, anchors, Q, seed, rnd, offset=0):
    """neg int32 [B, Q] by the definition above."""
    ptr, idx, _, n = graph
    neg = np.full((len(anchors), Q), -1, np.int32)
    for i, a in enumerate(anchors):
        a = int(a)
        row = set(int(x) for x in idx[ptr[a]:ptr[a + 1]])
        for s in range(Q):
            t = a * Q + s
            for k in range(TRIES):
                r = orc.philox(seed, (rnd * 16 + k, t & 0xFFFFFFFF, t >> 32, offset))
                j = (int(r[0]) * n) >> 32
                if j != a and j not in row:
                    neg[i, s] = j
                    break
    return neg


def sample_check(graph, nodes, S, seed, rounds, defect=None):
    """Over `rounds` rounds of every node in `nodes`: (the largest |frequency -
    pi| / sqrt(pi (1 - pi) / rounds) over the edges with pi = S / deg < 1, the
    largest |frequency - 1| over the edges of rows with deg <= S, whether a sample
    repeated a position, the largest |sum of weights - 1| in float32 ulps)."""
    ptr = graph[0]
    worst, short, repeat, wsum = 0.0, 0.0, False, 0.0
    for v in nodes:
        deg = int(ptr[v + 1] - ptr[v])
        if deg == 0:
            continue
        hits = np.zeros(deg)
        for rnd in range(rounds):
            cs = positions(deg, S, seed, rnd, int(v), 0, defect)
            repeat |= len(set(cs)) != len(cs)
            hits[list(set(cs))] += 1
        freq = hits / rounds
        if deg <= S:
            short = max(short, float(np.abs(freq - 1).max()))
        else:
            pi = S / deg
            worst = max(worst, float((np.abs(freq - pi) / np.sqrt(pi * (1 - pi) / rounds)).max()))
        _, w = neighbours(graph, [v], S, seed, 0, defect=defect)
        tot = np.float32(0)
        for x in w[0]:
            tot = np.float32(tot + x)
        wsum = max(wsum, abs(float(tot) - 1.0) / 2.0 ** -23)
    return worst, short, repeat, wsum


# ----------------------------------------------------------------------------- the loss
def cosines(Z, slots, dtype):
    """[B, G] cosines of every slot against its anchor in `dtype` (column 0: 1 or 0)."""
    dtype = np.dtype(dtype).type
    B, G = slots.shape
    Zg = np.asarray(Z, dtype).reshape(B, G, -1)
    s = np.einsum("bd,bgd->bg", Zg[:, 0], Zg)
    nn = np.einsum("bgd,bgd->bg", Zg, Zg)
    den = np.maximum(np.sqrt(nn[:, :1] * nn), dtype(CLAMP))
    c = s / den
    assert c.dtype == dtype
    return c, den, nn


def margin_loss(Z, slots, P, Q, margin, dtype, scale=None, defect=None):
    """(loss [B], active int32 [B], sel int32 [B, 2], dZ [B G, d]) in `dtype`;
    dZ is the gradient of scale * sum(loss), scale = 1 / max(1, #active) by
    default.  `defect` plants one of LOSS_DEFECTS."""
    dtype = np.dtype(dtype).type
    slots = np.asarray(slots)
    B, G = slots.shape
    assert G == 1 + P + Q
    Z = np.asarray(Z, dtype)
    Zg = Z.reshape(B, G, -1)
    c, den, nn = cosines(Z, slots, dtype)
    ok = slots >= 0
    active = (ok[:, 0] & ok[:, 1:1 + P].any(1) & ok[:, 1 + P:].any(1)).astype(np.int32)
    if scale is None:
        scale = dtype(1) / dtype(max(1, int(active.sum())))
    scale, margin, clamp = dtype(scale), dtype(margin), dtype(CLAMP)
    loss = np.zeros(B, dtype)
    sel = np.full((B, 2), -1, np.int32)
    dZ = np.zeros_like(Zg)
    for a in range(B):
        pos = [g for g in range(1, 1 + P) if ok[a, g]]
        neg = [g for g in range(1 + P, G) if ok[a, g]]
        if pos:   # the first of equal cosines: min / max return the lowest slot
            pick = max if defect == "max_positive" else min
            sel[a, 0] = pick(pos, key=lambda g: (c[a, g], -g) if pick is max else (c[a, g], g))
        if neg:
            sel[a, 1] = max(neg, key=lambda g: (c[a, g], -g))
        if not active[a]:
            continue
        p, q = int(sel[a, 0]), int(sel[a, 1])
        l = (softplus(-c[a, p]) - softplus(-c[a, q])) + margin
        if not l > 0:
            continue
        loss[a] = l
        za, na = Zg[a, 0], nn[a, 0]
        for g, coef in ((p, -sigmoid(-c[a, p]) * scale), (q, sigmoid(-c[a, q]) * scale)):
            x, k = Zg[a, g], coef / den[a, g]
            free = den[a, g] > clamp and defect != "no_norm_term"
            ka = coef * c[a, g] / na if free else dtype(0)
            kx = coef * c[a, g] / nn[a, g] if free else dtype(0)
            if defect != "anchor_gets_no_gradient":
                dZ[a, 0] += k * x - ka * za
            dZ[a, g] += k * za - kx * x
    assert loss.dtype == dtype and dZ.dtype == dtype
    return loss, active, sel, dZ.reshape(B * G, -1)


def runner_up_gaps(Z, slots, P, Q, by_node=False):
    """float64 [B]: the smaller of (second-smallest - smallest positive cosine,
    largest - second-largest negative cosine) over the non-void slots; inf where
    neither side has two.  by_node: slots that hold the same node count once
    (their rows of Z are the same row, so their cosines tie in every arithmetic
    and the lowest slot wins everywhere)."""
    c = cosines(Z, slots, np.float64)[0]
    gaps = np.full(len(slots), np.inf)
    for a in range(len(slots)):
        for lo, hi in ((1, 1 + P), (1 + P, 1 + P + Q)):
            live = np.flatnonzero(slots[a, lo:hi] >= 0)
            if by_node:
                live = live[np.unique(slots[a, lo:hi][live], return_index=True)[1]]
            v = np.sort(c[a, lo:hi][live])
            if len(v) >= 2:
                gaps[a] = min(gaps[a], v[1] - v[0] if lo == 1 else v[-1] - v[-2])
    return gaps


def loss_inputs(d, P, Q, seed=1, B=257):
    """(Z float32 [B G, d] Gaussian, slots int32 [B, G]) of the loss tests: a
    tenth of the slots void, group 5 without a positive, group 7 without a negative."""
    rng = np.random.default_rng(seed)
    G = 1 + P + Q
    Z = rng.standard_normal((B * G, d)).astype(np.float32)
    slots = rng.integers(0, 1000, (B, G)).astype(np.int32)
    slots[rng.random((B, G)) < 0.1] = -1
    slots[:, 0] = np.abs(slots[:, 0])
    slots[5 % B, 1:1 + P] = -1                                  # no positive: inactive
    slots[7 % B, 1 + P:] = -1                                   # no negative: inactive
    return Z, slots


# ----------------------------------------------------------------------------- one step
def lrelu(x):
    return np.where(x > 0, x, x * x.dtype.type(SLOPE))


def lrelu_grad(y):
    return np.where(y > 0, y.dtype.type(1), y.dtype.type(SLOPE))


def tables(graph, batch, r, prm, seed, cache=None):
    """The integer half of step r: dict(slots, T, U, nb1, w1, nb2, w2)."""
    S, NW, WL, Q = prm["num_sample"], prm["n_walks"], prm["walk_len"], prm["negatives"]
    batch = np.asarray(batch, np.int64)
    B = len(batch)
    walks = nu.walk(graph, np.repeat(batch, NW), WL + 1, 1.0, 1.0, seed, 0, r * prm["batch_size"] * NW)
    pos = walks[:, 1:].reshape(B, NW * WL).copy()
    pos[pos == batch[:, None]] = -1
    slots = np.concatenate([batch[:, None].astype(np.int32), pos, negatives(graph, batch, Q, seed, r)], 1)
    T = np.maximum(slots, 0).reshape(-1).astype(np.int64)
    nb2, w2 = neighbours(graph, T, S, seed, 2 * r + 1, cache=cache)
    U = np.unique(np.concatenate([T, nb2[nb2 >= 0].astype(np.int64)]))
    nb1, w1 = neighbours(graph, U, S, seed, 2 * r, cache=cache)
    return dict(slots=slots, T=T, U=U, nb1=nb1, w1=w1, nb2=nb2, w2=w2)


def aggregate(h, nb, w):
    """sum_j w_j h[nb_j] per row (void slots have w = 0)."""
    return np.einsum("us,usd->ud", np.asarray(w, h.dtype), h[np.maximum(nb, 0)])


def forward(tb, X0, W1, W2, dtype):
    X0, W1, W2 = (np.asarray(a, dtype) for a in (X0, W1, W2))
    U = tb["U"]
    in1 = np.concatenate([X0[U], aggregate(X0, tb["nb1"], tb["w1"])], 1)
    H1 = lrelu(in1 @ W1.T)
    tl = np.searchsorted(U, tb["T"])
    nl = np.where(tb["nb2"] >= 0, np.searchsorted(U, np.maximum(tb["nb2"], 0)), -1)
    in2 = np.concatenate([H1[tl], aggregate(H1, nl, tb["w2"])], 1)
    Z = lrelu(in2 @ W2.T)
    assert Z.dtype == np.dtype(dtype)
    return in1, H1, tl, nl, in2, Z


def step(tb, X0, W1, W2, prm, dtype, defect=None):
    """Loss and gradients of one step on the tables tb in `dtype`: dict(loss,
    loss_a, active, sel, Z, dZ, dW1, dW2)."""
    P, Q = prm["n_walks"] * prm["walk_len"], prm["negatives"]
    W2 = np.asarray(W2, dtype)
    in1, H1, tl, nl, in2, Z = forward(tb, X0, W1, W2, dtype)
    out = Z.shape[1]
    loss_a, active, sel, dZ = margin_loss(Z, tb["slots"], P, Q, prm["margin"], dtype, defect=defect)
    scale = np.dtype(dtype).type(1) / np.dtype(dtype).type(max(1, int(active.sum())))
    dP2 = dZ * lrelu_grad(Z)
    dW2 = dP2.T @ in2
    dSA = dP2 @ W2
    dH1 = np.zeros_like(H1)
    np.add.at(dH1, tl, dSA[:, :out])
    w2 = np.asarray(tb["w2"], dtype)
    for j in range(nl.shape[1]):
        keep = nl[:, j] >= 0
        np.add.at(dH1, nl[keep, j], w2[keep, j, None] * dSA[keep, out:])
    dW1 = (dH1 * lrelu_grad(H1)).T @ in1
    assert dW1.dtype == np.dtype(dtype) and dW2.dtype == np.dtype(dtype)
    return dict(loss=loss_a.sum() * scale, loss_a=loss_a, active=active, sel=sel, Z=Z, dZ=dZ, dW1=dW1, dW2=dW2)


def scalar_loss(tb, X0, W1, W2, prm):
    """The step's loss in float64 (for central differences)."""
    P, Q = prm["n_walks"] * prm["walk_len"], prm["negatives"]
    Z = forward(tb, X0, W1, W2, np.float64)[5]
    loss_a, active = margin_loss(Z, tb["slots"], P, Q, prm["margin"], np.float64)[:2]
    return float(loss_a.sum() / max(1, int(active.sum())))


# ----------------------------------------------------------------------------- the fit
def adam_coef(t, lr):
    """What the host stages for step t (1-based), float32."""
    return np.array([lr / (1.0 - BETAS[0] ** t), (1.0 - BETAS[1] ** t) ** 0.5], np.float32)


def adam(p, g, m, v, t, lr, dtype):
    """One step of torch's Adam in `dtype` from the float32 coefficients."""
    dtype = np.dtype(dtype).type
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    c0, c1 = (dtype(c) for c in adam_coef(t, lr))
    m = m + (g - m) * dtype(1 - BETAS[0])
    v = v * dtype(BETAS[1]) + dtype(1 - BETAS[1]) * g * g
    p = p - c0 * (m / (np.sqrt(v) / c1 + dtype(EPS)))
    assert p.dtype == dtype
    return p, m, v


def batches(n, seed, epochs, batch_size):
    """The fit's batches in order: (epoch, node ids)."""
    for e in range(epochs):
        order = torch.randperm(n, generator=torch.Generator().manual_seed((seed + e) % 2 ** 63)).numpy()
        for b0 in range(0, n, batch_size):
            yield e, order[b0:b0 + batch_size]


def fit(graph, X0, W1, W2, prm, seed, epochs, dtype, store, max_steps=None):
    """The fit in `dtype`: (W1, W2, losses [steps], epoch of each step, sel per
    step, the smallest runner_up_gaps(by_node) per step).  store: a dict r -> tables, read and filled (the draws do not depend
    on the weights, so the float32 and float64 runs share them)."""
    W = [np.array(W1, dtype), np.array(W2, dtype)]
    M, V = [np.zeros_like(w) for w in W], [np.zeros_like(w) for w in W]
    losses, epoch_of, sels, gaps = [], [], [], []
    P, Q = prm["n_walks"] * prm["walk_len"], prm["negatives"]
    cache = store.setdefault("rows", {})
    for r, (e, batch) in enumerate(batches(graph[3], seed, epochs, prm["batch_size"])):
        if max_steps is not None and r >= max_steps:
            break
        if r not in store:
            store[r] = tables(graph, batch, r, prm, seed, cache)
        st = step(store[r], X0, W[0], W[1], prm, dtype)
        for k, g in enumerate((st["dW1"], st["dW2"])):
            W[k], M[k], V[k] = adam(W[k], g, M[k], V[k], r + 1, prm["learning_rate"], dtype)
        losses.append(float(st["loss"]))
        epoch_of.append(e)
        sels.append(st["sel"])
        gaps.append(float(runner_up_gaps(st["Z"], store[r]["slots"], P, Q, by_node=True).min()))
    return W[0], W[1], np.array(losses), np.array(epoch_of), sels, np.array(gaps)
