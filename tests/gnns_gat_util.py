"""Restatements of the lib/gnns GAT aggregator (GNNs_unsupervised.py:449-465,
555-567) for tests/test_gnns_gat.py and tests/golden/make_golden_gnns_gat.py.

``restate`` is the definition the kernels are built to (csrc/gnns.h), forward
and backward, in float64 by default; with ``dtype=np.float32`` it is the same
shifted formulas in float32 (the yardstick of the large-score run).
``reference32`` is the reference's own order of operations in float32: the
unshifted exp and ``F.normalize(p=1)``'s ``max(sum, 1e-12)``.

A CSR is (seg_ptr int64 [F+1], hrows int [nnz] rows of h, c float [nnz] >= 0,
own int [F] the h row of each segment's node); a = [a_l | a_r] [2 d].
"""
import numpy as np

SLOPE = 0.2


def _scores(h, a, seg_ptr, hrows, c, own, T):
    n_h, d = h.shape
    F = len(seg_ptr) - 1
    hrows = np.asarray(hrows, np.int64)
    own = np.asarray(own, np.int64)
    seg_of = np.repeat(np.arange(F, dtype=np.int64), np.diff(seg_ptr))
    ok = (hrows >= 0) & (hrows < n_h)
    own_ok = (own >= 0) & (own < n_h)
    r = np.where(ok, hrows, 0)
    ro = np.where(own_ok, own, 0)
    if n_h == 0:
        z = np.zeros(len(hrows), T)
        return seg_of, r, ro, z, z, np.zeros(len(hrows), bool)
    s_l = h @ a[:d]
    s_r = h @ a[d:]
    e = (s_l[ro][seg_of] + s_r[r]).astype(T)
    m = (np.where(e > 0, e, T(SLOPE) * e) * c).astype(T)
    keep = ok & own_ok[seg_of] & (m != 0)
    return seg_of, r, ro, e, m, keep


def restate(h, a, seg_ptr, hrows, c, own, dout=None, dtype=np.float64):
    """dict(out, p, e, m, keep[, dh, da]) of the shifted-softmax definition."""
    T = dtype
    h = np.asarray(h).astype(T)
    a = np.asarray(a).astype(T).reshape(-1)
    c = np.asarray(c).astype(T)
    n_h, d = h.shape
    F = len(seg_ptr) - 1
    seg_of, r, ro, e, m, keep = _scores(h, a, seg_ptr, hrows, c, own, T)
    M = np.full(F, -np.inf, T)
    np.maximum.at(M, seg_of[keep], m[keep])
    ex = np.zeros(len(m), T)
    ex[keep] = np.exp(m[keep] - M[seg_of[keep]])
    S = np.zeros(F, T)
    np.add.at(S, seg_of, ex)
    p = ex / np.where(S > 0, S, T(1))[seg_of]
    out = np.zeros((F, d), T)
    if n_h:
        np.add.at(out, seg_of, p[:, None] * h[r])
    res = dict(out=out, p=p, e=e, m=m, keep=keep)
    if dout is None:
        return res
    dout = np.asarray(dout).astype(T)
    dh = np.zeros((n_h, d), T)
    da = np.zeros(2 * d, T)
    if n_h:
        g = (dout[seg_of] * h[r]).sum(1)
        gbar = np.zeros(F, T)
        np.add.at(gbar, seg_of, p * g)
        de = np.where(keep, p * (g - gbar[seg_of]) * c * np.where(e > 0, T(1), T(SLOPE)), T(0)).astype(T)
        s = np.zeros(F, T)
        np.add.at(s, seg_of, de)
        np.add.at(dh, r, p[:, None] * dout[seg_of] + de[:, None] * a[d:])
        np.add.at(dh, ro, s[:, None] * a[:d])
        da[:d] = (s[:, None] * h[ro]).sum(0)
        da[d:] = (de[:, None] * h[r]).sum(0)
    res.update(dh=dh, da=da)
    return res


def reference32(h, a, seg_ptr, hrows, c, own):
    """The reference's forward in its own order, float32: exp(mask) * (mask !=
    0), divided by max(row sum, 1e-12), times the embeddings."""
    T = np.float32
    h = np.asarray(h, T)
    a = np.asarray(a, T).reshape(-1)
    c = np.asarray(c, T)
    F = len(seg_ptr) - 1
    seg_of, r, _, _, m, keep = _scores(h, a, seg_ptr, hrows, c, own, T)
    ex = np.where(keep, np.exp(m), T(0)).astype(T)
    S = np.zeros(F, T)
    np.add.at(S, seg_of, ex)
    p = ex / np.maximum(S, T(1e-12))[seg_of]
    out = np.zeros((F, h.shape[1]), T)
    np.add.at(out, seg_of, p[:, None] * h[r])
    return out


def rel(x, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(np.asarray(x, np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))


def fixture_csr(g, adj):
    """(seg_ptr, hrows, c, own) of a fixture case from its stored node sets,
    stated without the product: the node itself is in its set, c = sqrt(count)."""
    nodes = [int(x) for x in g["nodes"]]
    uniq = [int(x) for x in g["unique"]]
    pos = {u: j for j, u in enumerate(uniq)}
    sp_ = g["samp_ptr"]
    shortcut = len(g["emb"]) == len(uniq)
    hrows, c, own = [], [], []
    for i, v in enumerate(nodes):
        for x in g["samp"][sp_[i]:sp_[i + 1]]:
            hrows.append(pos[int(x)] if shortcut else int(x))
            c.append(np.sqrt(np.float32(adj[v, int(x)])))
        own.append(pos[v] if shortcut else v)
    return (np.asarray(sp_, np.int64), np.asarray(hrows, np.int64), np.asarray(c, np.float32),
            np.asarray(own, np.int64))
