"""The numpy restatement of the link-prediction indices (csrc/cooc.hip's
weighted kernel, baselines.SimpleSimilarity and its subclasses), shared by
tests/test_gpu_linksim.py (on the GPU) and tests/test_linksim_host.py (which
checks it against networkx's recorded output on the host).

A graph is two boolean matrices: adj [n_mid, n], middle node c neighbours
track t.  For the bipartite graph adj is jaccard_util.memberships; for the
projected graph it is the (symmetric, zero-diagonal) track-track adjacency.

    wt[c]    = floor(2^30 / ln(dmid(c)) + 0.5) for dmid(c) >= 2, else 0   (int64, from float64)
    S(q, t)  = sum of wt[c] over c adjacent to both q and t               (int64)
    aa(q, t) = float32(S) * float32(2^-30)                                (nearest even)
    order    = score descending, then id ascending (jaccard_util.topk)
"""
import numpy as np

import jaccard_util as ju

SHIFT = 30


def projected(member):
    """bool [n, n]: tracks a != b share a collection."""
    m = member.astype(np.int64)
    p = (m.T @ m) > 0
    np.fill_diagonal(p, False)
    return p


def weights(dmid):
    d = np.asarray(dmid, np.int64)
    w = np.zeros(d.shape, np.int64)
    big = d >= 2
    w[big] = np.floor(float(1 << SHIFT) / np.log(d[big].astype(np.float64)) + 0.5).astype(np.int64)
    return w


def sums(adj, wt, queries):
    """int64 [nq, n]: per query the weights of its middle nodes times their
    boolean rows (a dense product over the query's middle nodes; int64 adds)."""
    q = np.asarray(queries, np.int64).reshape(-1)
    wt = np.asarray(wt, np.int64)
    out = np.empty((len(q), adj.shape[1]), np.int64)
    for i, v in enumerate(q.tolist()):
        mid = adj[:, v]
        out[i] = wt[mid] @ adj[mid].astype(np.int64)
    return out


def to_score(s):
    out = np.asarray(s, np.int64).astype(np.float32) * np.float32(2.0 ** -SHIFT)
    assert out.dtype == np.float32
    return out


def common(adj, queries):
    """int64 [nq, n]: the number of common neighbours."""
    return sums(adj, np.ones(adj.shape[0], np.int64), queries)


def jaccard(adj, queries):
    """float32 [nq, n]: the Jaccard path's formula over the neighbour sets."""
    return ju.scores(common(adj, queries), adj.sum(0).astype(np.int64), queries)


def preferential(adj, queries):
    deg = adj.sum(0).astype(np.int64)
    return deg[np.asarray(queries, np.int64).reshape(-1)][:, None] * deg[None, :]


def aa_bound(cn, ref32):
    """|restated or device score - float32(networkx)| stays within this: each of
    the cn terms is rounded to half a unit of 2^-30, and each side is rounded
    once to float32 (2^-24 relative each)."""
    return cn.astype(np.float64) * 2.0 ** -31 + 2.0 ** -23 * np.abs(ref32.astype(np.float64))
