"""The numpy reference of the Jaccard co-occurrence path (csrc/cooc.hip,
baselines.JaccardFast), shared by tests/test_gpu_jaccard.py (on the GPU) and
tests/test_jaccard_host.py (which checks it against the reference's recorded
output on the host).

A graph is (n_tracks, n_cols, edges): nodes [0, n_tracks) are tracks, nodes
[n_tracks, n_tracks + n_cols) collections, edges an int [m, 2] array of
(src, dst).  An edge with exactly one track endpoint is a membership, whichever
way it points and however often it is listed; an edge between two tracks counts
nothing.

    co[q][t]  = the number of collections that hold both q and t
    deg[t]    = co[t][t], the number of collections that hold t
    s(q, t)   = float32(co) / (float32(deg[q] + deg[t] - co) + float32(1e-10))
    order     = score descending, then id ascending
"""
import numpy as np


def memberships(n_tracks, n_cols, edges):
    """bool [n_cols, n_tracks]: collection c holds track t."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    m = np.zeros((n_cols, n_tracks), bool)
    s_tr, d_tr = e[:, 0] < n_tracks, e[:, 1] < n_tracks
    assert (s_tr | d_tr).all(), "an edge joins two collections"
    one = s_tr ^ d_tr
    tr = np.where(s_tr, e[:, 0], e[:, 1])[one]
    co = np.where(s_tr, e[:, 1], e[:, 0])[one] - n_tracks
    m[co, tr] = True
    return m


def csrs(member):
    """The two CSRs pinsage_cooc_* read, from the membership matrix:
    (t2c_ptr int64, t2c_idx int32, c2t_ptr int64, c2t_idx int32), rows ascending."""
    def one(m):
        ptr = np.zeros(m.shape[0] + 1, np.int64)
        np.cumsum(m.sum(1), out=ptr[1:])
        return ptr, np.nonzero(m)[1].astype(np.int32)
    return one(member.T) + one(member)


def degrees(member):
    return member.sum(0).astype(np.int64)


def counts(member, queries):
    """int32 [nq, n_tracks] by set intersection: for each query the collections
    that hold it, and per track how many of those hold the track too."""
    q = np.asarray(queries, np.int64).reshape(-1)
    out = np.empty((len(q), member.shape[1]), np.int32)
    for i, v in enumerate(q.tolist()):
        out[i] = member[member[:, v]].sum(0)
    return out


def scores(co, deg, queries):
    """float32 [nq, n_tracks]: the score formula, every step in float32."""
    q = np.asarray(queries, np.int64).reshape(-1)
    co = np.asarray(co, np.int64)
    union = deg[q][:, None] + deg[None, :] - co
    den = union.astype(np.float32) + np.float32(1e-10)
    assert den.dtype == np.float32
    return (co.astype(np.float32) / den).astype(np.float32)


def topk(score, k):
    """(float32 [nq, k], int64 [nq, k]): the k best per row in the order (score
    descending, id ascending), by np.lexsort."""
    nq, n = score.shape
    ids = np.empty((nq, k), np.int64)
    for i in range(nq):
        ids[i] = np.lexsort((np.arange(n), -score[i].astype(np.float64)))[:k]
    return np.take_along_axis(score, ids, 1), ids


def knn_reference(n_tracks, n_cols, edges, queries, k):
    """What the device computes for (queries, k) before column 0 is dropped."""
    m = memberships(n_tracks, n_cols, edges)
    co = counts(m, queries)
    return topk(scores(co, degrees(m), queries), k)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_lists(got_w, got_n, score, what=""):
    """The tie-insensitive check of an id list against the dense scores: every
    row's ids are distinct and in range, and the listed score of each id is that
    id's score bit for bit."""
    got_w, got_n = np.asarray(got_w, np.float32), np.asarray(got_n, np.int64)
    n = score.shape[1]
    assert got_w.shape == got_n.shape and got_n.shape[0] == score.shape[0], what
    assert ((got_n >= 0) & (got_n < n)).all(), f"{what}: ids out of range"
    srt = np.sort(got_n, 1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), f"{what}: a row lists an id twice"
    assert np.array_equal(bits(np.take_along_axis(score, got_n, 1)), bits(got_w)), \
        f"{what}: a listed score is not the score of its id"


def check_exact(got_w, got_n, want_w, want_n, what=""):
    """Ids and score bits equal; the first differing cell is named."""
    got_w, got_n = np.asarray(got_w, np.float32), np.asarray(got_n, np.int64)
    assert got_w.shape == want_w.shape and got_n.shape == want_n.shape, (what, got_w.shape, want_w.shape)
    bad = (got_n != want_n) | (bits(got_w) != bits(want_w))
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: row {r} column {c}: got ({got_n[r, c]}, {got_w[r, c]!r}), reference "
                             f"({want_n[r, c]}, {want_w[r, c]!r}); {int(bad.sum())} of {bad.size} cells differ")


def seeded_graph(n_tracks, n_cols, seed, mean_size=6):
    """Edges of a seeded random bipartite graph (collection -> track), with
    duplicates and both directions mixed in."""
    rng = np.random.default_rng(seed)
    e = []
    for c in range(n_cols):
        size = int(rng.integers(1, 2 * mean_size))
        for t in rng.integers(0, n_tracks, size).tolist():
            e.append((n_tracks + c, t) if rng.random() < 0.5 else (t, n_tracks + c))
    return np.array(e, np.int64).reshape(-1, 2)
