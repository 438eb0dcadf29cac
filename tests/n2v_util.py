"""The numpy / Python-int references of the node2vec path (csrc/n2v.hip,
baselines.Node2Vec), shared by tests/test_gpu_n2v.py (on the GPU) and
tests/test_n2v_host.py (which checks the references themselves on the host).

The walk.  A graph is (ptr int64 [n + 1], idx int32 ascending per row, cum int64
or None, n): cum holds per row the inclusive prefix sum of positive integer
edge weights.  Walk k starts at starts[k], its generator position is
walk_base + k.  Step j >= 1, try t:
    (r0, r1, r2, r3) = philox(seed, (j * 256 + t, pos lo, pos hi, offset))
    pick = ((r0 | r1 << 32) * total) >> 64, total = the row's last cum (its degree)
    candidate = the first edge whose cum exceeds pick (edge `pick` when unweighted)
    step 1 takes try 0's candidate; from step 2 on beta = inv_p for the previous
    node, 1 for a neighbour of the previous node, inv_q otherwise, and the
    candidate is accepted iff fp32((r2 >> 8) * 2^-24 * M) < beta, M = max(inv_p,
    1, inv_q); after 256 rejected tries the last candidate is taken.
A node without edges ends the walk (-1 from there on).

The fit.  C is a symmetric CSR (ptr, idx, val, n, n), # its row sums, P the noise
distribution, K the number of negatives, s_wc = u_w . v_c;
    L = sum_wc C_wc log sig(s_wc) + K sum_w #(w) sum_c P(c) log sig(-s_wc) - (reg / 2)(|U|^2 + |V|^2)
and a half-iteration runs, per row u of X against Y with weights (cw, rw),
    D = sum_all i cw_i sig(x . y_i) y_i;  g = sum_obs val_i sig(-(x . y_i)) y_i - rw_u D - reg x
    h += g^2;  x += lr g / sqrt(1e-6 + h)
with (cw, rw) = (P, K #) for the centre half and (K #, P) for the context half.
"""
import numpy as np

from lmf_util import EPS, sigmoid, softplus
from oracle import oracle as orc

TRIES = 256
WALK_DEFECTS = ("pq_swapped", "weights_ignored", "previous_as_neighbour")
FIT_DEFECTS = ("no_row_weight", "no_column_weight", "weights_swapped")
DEFAULTS = dict(dim=128, walk_length=20, context=10, p=2.0, q=0.5, walks_per_node=10, negative=5.0, ns_exponent=0.75,
                learning_rate=0.1, regularization=0.0, iterations=30, random_state=None)


# ----------------------------------------------------------------------------- graphs
def graph_from_edges(n, edges):
    """An undirected graph from (a, b, weight) triples, each given once."""
    rows = [dict() for _ in range(n)]
    for a, b, w in edges:
        assert a != b and b not in rows[a] and w >= 1
        rows[a][b] = rows[b][a] = int(w)
    ptr = np.zeros(n + 1, np.int64)
    idx, cum = [], []
    for v in range(n):
        run = 0
        for x in sorted(rows[v]):
            run += rows[v][x]
            idx.append(x)
            cum.append(run)
        ptr[v + 1] = len(idx)
    return ptr, np.asarray(idx, np.int32), np.asarray(cum, np.int64), n


def small_graph():
    """7 nodes, weighted: triangles (so beta = 1 occurs), a degree-1 node, weights 1 .. 5."""
    return graph_from_edges(7, [(0, 1, 1), (0, 2, 3), (1, 2, 2), (1, 3, 5), (2, 3, 1), (3, 4, 2), (2, 4, 4),
                                (4, 5, 1), (3, 5, 3), (5, 6, 2)])


def edge_graph():
    """The walk kernel's edges in one graph of 75 nodes: a hub (node 0) with 70
    edges of mixed weights, a ring among nodes 1 .. 10, leaves 11 .. 70 of degree
    1 (a walk that enters one has to go back), node 71 isolated, and the pair
    72 - 73 joined by a weight of 2^33 with 72 also tied to node 1 (a row whose
    total exceeds 2^32) and 74 hanging off 73."""
    e = [(0, v, 1 + (v * 7) % 5) for v in range(1, 71)]
    e += [(v, v + 1, 2) for v in range(1, 10)] + [(10, 1, 2)]
    e += [(72, 73, 1 << 33), (1, 72, 3), (73, 74, 1 << 31)]
    return graph_from_edges(75, e)


def weights_of(graph):
    ptr, idx, cum, n = graph
    if cum is None:
        return np.ones(len(idx), np.int64)
    w = np.array(cum)
    for v in range(n):
        b, e = int(ptr[v]), int(ptr[v + 1])
        w[b + 1:e] = cum[b + 1:e] - cum[b:e - 1]
    return w


def planted_graph(seed, n_tracks=160, n_groups=4, n_cols=60, size=8, stray=0.1):
    """The weighted projection of a planted bipartite graph: every collection
    belongs to one of n_groups groups and holds `size` distinct tracks, each from
    its group (tracks t with t % n_groups == group) except with probability
    `stray`, then from anywhere.  (graph, group of each track)."""
    rng = np.random.default_rng(seed)
    M = np.zeros((n_cols, n_tracks), np.int64)
    for c in range(n_cols):
        grp = c % n_groups
        own = np.flatnonzero(np.arange(n_tracks) % n_groups == grp)
        while M[c].sum() < size:
            t = rng.integers(n_tracks) if rng.random() < stray else own[rng.integers(len(own))]
            M[c, t] = 1
    W = M.T @ M
    np.fill_diagonal(W, 0)
    edges = [(a, b, W[a, b]) for a in range(n_tracks) for b in range(a + 1, n_tracks) if W[a, b]]
    return graph_from_edges(n_tracks, edges), np.arange(n_tracks) % n_groups


# ----------------------------------------------------------------------------- the walk
def _in_row(graph, v, x):
    ptr, idx = graph[:2]
    row = idx[ptr[v]:ptr[v + 1]]
    i = int(np.searchsorted(row, x))
    return i < len(row) and row[i] == x


def walk(graph, starts, length, inv_p, inv_q, seed, offset=0, walk_base=0, defect=None):
    """int32 [len(starts), length], the definition above in Python integers and
    one np.float32 product.  `defect` plants one of WALK_DEFECTS."""
    ptr, idx, cum, n = graph
    inv_p, inv_q = np.float32(inv_p), np.float32(inv_q)
    if defect == "pq_swapped":
        inv_p, inv_q = inv_q, inv_p
    if defect == "weights_ignored":
        cum = None
    one = np.float32(1)
    M = max(inv_p, one, inv_q)
    scale = np.float32(2.0 ** -24)
    out = np.full((len(starts), length), -1, np.int32)
    for k, start in enumerate(starts):
        pos = walk_base + k
        cur, prev = int(start), -1
        out[k, 0] = cur
        for j in range(1, length):
            b, e = int(ptr[cur]), int(ptr[cur + 1])
            if e <= b:
                break
            total = int(cum[e - 1]) if cum is not None else e - b
            for t in range(TRIES):
                r = orc.philox(seed, (j * 256 + t, pos & 0xFFFFFFFF, pos >> 32, offset))
                pick = (((int(r[1]) << 32) | int(r[0])) * total) >> 64
                edge = b + (int(np.searchsorted(cum[b:e], pick, side="right")) if cum is not None else pick)
                cand = int(idx[edge])
                if j == 1:
                    break
                if cand == prev and defect != "previous_as_neighbour":
                    beta = inv_p
                else:
                    beta = one if _in_row(graph, prev, cand) else inv_q
                if np.float32(int(r[2]) >> 8) * scale * M < beta:
                    break
            prev, cur = cur, cand
            out[k, j] = cur
    return out


def next_probabilities(graph, prev, cur, inv_p, inv_q):
    """{x: probability} of the step after (prev, cur): proportional to weight * beta."""
    ptr, idx = graph[:2]
    w = weights_of(graph)
    mass = {}
    for e in range(int(ptr[cur]), int(ptr[cur + 1])):
        x = int(idx[e])
        beta = inv_p if x == prev else (1.0 if _in_row(graph, prev, x) else inv_q)
        mass[x] = float(w[e]) * beta
    tot = sum(mass.values())
    return {x: m / tot for x, m in mass.items()}


def transition_check(graph, walks, inv_p, inv_q, min_seen=200, sigmas=5.0):
    """Over every (prev, cur) seen at least min_seen times at steps >= 2: the
    largest |frequency - pi| / sqrt(pi (1 - pi) / N) over the next nodes, and the
    number of (prev, cur) pairs examined.  The check passes below `sigmas`."""
    seen = {}
    for w in walks:
        for j in range(2, len(w)):
            if w[j] < 0:
                break
            seen.setdefault((int(w[j - 2]), int(w[j - 1])), []).append(int(w[j]))
    worst, pairs = 0.0, 0
    for (prev, cur), nxt in seen.items():
        if len(nxt) < min_seen:
            continue
        pairs += 1
        N = len(nxt)
        for x, pi in next_probabilities(graph, prev, cur, inv_p, inv_q).items():
            freq = nxt.count(x) / N
            sd = np.sqrt(pi * (1 - pi) / N)
            worst = max(worst, abs(freq - pi) / sd if sd > 0 else (0.0 if freq == pi else np.inf))
    return worst, pairs


# ----------------------------------------------------------------------------- counts
def cooccurrence_loops(walks, n, context):
    """Dense int64 [n, n] by the definition: a triple loop."""
    C = np.zeros((n, n), np.int64)
    for w in walks:
        for i in range(len(w)):
            for j in range(len(w)):
                if i != j and abs(i - j) <= context and w[i] >= 0 and w[j] >= 0:
                    C[w[i], w[j]] += 1
    return C


def csr_of(dense):
    """(ptr, idx, val float32, n, n) of a dense matrix."""
    n = len(dense)
    r, c = np.nonzero(dense)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    return ptr, c.astype(np.int32), dense[r, c].astype(np.float32), n, n


def dense_of(C):
    ptr, idx, val, n = C[:4]
    D = np.zeros((n, n))
    D[np.repeat(np.arange(n), np.diff(ptr)), np.asarray(idx, np.int64)] = val
    return D


def noise(C, exponent=0.75):
    """(# float64 [n], P float32 [n]): P from float64, rounded; a node that never occurs has P = 0."""
    cnt = dense_of(C).sum(1)
    pw = np.where(cnt > 0, cnt ** exponent, 0.0)
    return cnt, (pw / pw.sum()).astype(np.float32)


# ----------------------------------------------------------------------------- the fit
def dense_term(X, Y, cw, dtype):
    """D [n_rows, f] = (sig(X Y^T) * cw) Y in `dtype` arithmetic."""
    dtype = np.dtype(dtype).type
    X, Y, cw = (np.asarray(a, dtype) for a in (X, Y, cw))
    D = (sigmoid(X @ Y.T) * cw[None, :]) @ Y
    assert D.dtype == dtype
    return D


def half_iteration(ptr, idx, val, rw, X, H, Y, cw, reg, lr, dtype, D=None):
    """The recurrence above in `dtype`: the new (X, H).  D: given dense term."""
    dtype = np.dtype(dtype).type
    X, H = np.array(X, dtype), np.array(H, dtype)
    Y, rw = np.asarray(Y, dtype), np.asarray(rw, dtype)
    D = dense_term(X, Y, cw, dtype) if D is None else np.asarray(D, dtype)
    reg, lr, eps = dtype(reg), dtype(lr), dtype(EPS)
    for u in range(len(ptr) - 1):
        sl = slice(int(ptr[u]), int(ptr[u + 1]))
        Yi = Y[np.asarray(idx[sl], np.int64)]
        w = np.asarray(val[sl], dtype) * sigmoid(-(Yi @ X[u]))
        g = Yi.T @ w - rw[u] * D[u] - reg * X[u]
        H[u] = H[u] + g * g
        X[u] = X[u] + lr * g / np.sqrt(eps + H[u])
    assert X.dtype == dtype and H.dtype == dtype
    return X, H


def half_weights(cnt, P, K, half, defect=None):
    """(cw, rw) of the centre (half 0) or the context (half 1) half-iteration."""
    kn = K * np.asarray(cnt, np.float64)
    cw, rw = (P, kn) if half == 0 else (kn, P)
    if defect == "weights_swapped":
        cw, rw = rw, cw
    if defect == "no_row_weight":
        rw = np.ones_like(np.asarray(rw, np.float64))
    if defect == "no_column_weight":
        cw = np.ones_like(np.asarray(cw, np.float64))
    return np.asarray(cw, np.float64), np.asarray(rw, np.float64)


def fit(C, U, V, cnt, P, K, reg, lr, iterations, dtype, trace=False):
    """`iterations` times: centres from V, then contexts from the new U;
    accumulators from zero.  (U, V) in dtype; with trace also objective() after
    every iteration.  K # is rounded to fp32 first, as the device's copy is."""
    ptr, idx, val = C[:3]
    U, V = np.array(U, dtype), np.array(V, dtype)
    Hu, Hv = np.zeros_like(U), np.zeros_like(V)
    kn = (K * np.asarray(cnt, np.float64)).astype(np.float32)
    seen = []
    for _ in range(iterations):
        U, Hu = half_iteration(ptr, idx, val, kn, U, Hu, V, P, reg, lr, dtype)
        V, Hv = half_iteration(ptr, idx, val, P, V, Hv, U, kn, reg, lr, dtype)
        if trace:
            seen.append(objective(C, U, V, K, P, reg))
    return (U, V, seen) if trace else (U, V)


def objective(C, U, V, K, P, reg):
    """L over the dense matrix, float64."""
    Cd = dense_of(C)
    U, V, P = (np.asarray(a, np.float64) for a in (U, V, P))
    S = U @ V.T
    cnt = Cd.sum(1)
    return float(-(Cd * softplus(-S)).sum() - K * (cnt[:, None] * P[None, :] * softplus(S)).sum()
                 - 0.5 * reg * ((U * U).sum() + (V * V).sum()))


def same_group_share(E, groups, connected, k=10):
    """Over the rows in `connected`: the share of their top-k cosine neighbours
    (among `connected`, themselves excluded) that lie in the row's own group."""
    E = np.asarray(E, np.float64)[connected]
    g = np.asarray(groups)[connected]
    Z = E / np.maximum(np.linalg.norm(E, axis=1, keepdims=True), 1e-300)
    S = Z @ Z.T
    np.fill_diagonal(S, -np.inf)
    top = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return float((g[top] == g[:, None]).mean())
