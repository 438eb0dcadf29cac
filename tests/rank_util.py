"""The numpy reference of pinsage_rank_cosine (rank_count_kernel, csrc/knn.hip)
and its comparison, shared by tests/test_gpu_rank.py (on the GPU) and
tests/test_eval_metrics.py (which checks the reference itself on the host).

The rank of target t for a query is how many rows j come before it in the
order pinsage_knn_cosine documents:
    #{ j : key(j) > key(t) or (key(j) == key(t) and j < t) }
with key the order-preserving uint32 image of the fp32 similarity
(parity_util.knn_key_image).  On the tables of parity_util.knn_select_table
every similarity is exact in fp32, so ranks are compared as integers.
"""
import numpy as np

import parity_util as pu

RANK_FEW = 8           # kRankFew (knn.hip): up to here a group is counted from registers
RANK_MAX_GROUP = 4096  # kRankMaxGroup: targets one query row may own


def rank_form(m):
    """The form rank_count_kernel takes for a group of m targets, replayed."""
    assert 0 <= m <= RANK_MAX_GROUP, f"a group of {m} targets is refused by the launcher"
    return "empty" if m == 0 else "few" if m <= RANK_FEW else "sorted"


def key_image_no_flip(sim_row):
    """A planted defect: f2key without the inversion of negative floats."""
    u = np.ascontiguousarray(sim_row, np.float32).view(np.uint32)
    return (u | np.uint32(0x80000000)).astype(np.uint32)


def rank_reference(sim, qrow, targets, tie="lt", count_self=False, key_image=pu.knn_key_image):
    """int64 [np]: the rank of row targets[i] in the row sim[qrow[i]] (f32
    similarities [nq][n]).  The keyword arguments plant one defect each: tie="le"
    breaks ties by j <= t, count_self counts the target against itself (both add
    the target's own row, so they give the same wrong ranks), key_image takes
    another image of the similarity."""
    sim = np.asarray(sim, np.float32)
    qrow = np.asarray(qrow, np.int64).reshape(-1)
    targets = np.asarray(targets, np.int64).reshape(-1)
    assert qrow.shape == targets.shape
    out = np.empty(len(targets), np.int64)
    keys = {}
    j = np.arange(sim.shape[1])
    for i, (r, t) in enumerate(zip(qrow.tolist(), targets.tolist())):
        if r not in keys:
            keys[r] = key_image(sim[r])
        key = keys[r]
        kt = key[t]
        before = j <= t if tie == "le" else j < t
        out[i] = int((key > kt).sum()) + int(((key == kt) & before).sum()) + int(bool(count_self))
    return out


def check_ranks(got, want, queries, targets):
    """Exact.  The first differing pair raises an AssertionError naming its
    (query, target)."""
    got, want = np.asarray(got), np.asarray(want)
    queries, targets = np.asarray(queries).reshape(-1), np.asarray(targets).reshape(-1)
    if got.shape != want.shape or got.shape != queries.shape or got.shape != targets.shape:
        raise AssertionError(f"rank: shapes {got.shape}, reference {want.shape}, pairs {queries.shape} / {targets.shape}")
    if got.dtype != np.int64:
        raise AssertionError(f"rank: dtype {got.dtype}, not int64")
    bad = got != want
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"rank (query {int(queries[i])}, target {int(targets[i])}), pair {i}: got {int(got[i])}, "
                             f"reference {int(want[i])}; {int(bad.sum())} of {bad.size} pairs differ")


def check_ranks_vs_knn(ranks, qrow, targets, ids):
    """The documented equality with pinsage_knn_cosine's columns ids [nq][k]:
    the row of the pair's query holds the target at column rank when rank < k,
    and nowhere when rank >= k."""
    ids = np.asarray(ids)
    k = ids.shape[1]
    for i, (r, t, rk) in enumerate(zip(np.asarray(qrow).tolist(), np.asarray(targets).tolist(),
                                       np.asarray(ranks).tolist())):
        if rk < k:
            assert ids[r, rk] == t, f"rank pair {i} (query row {r}, target {t}): rank {rk}, but kNN column {rk} holds {ids[r, rk]}"
        else:
            assert t not in ids[r], f"rank pair {i} (query row {r}, target {t}): rank {rk} >= k = {k}, but the kNN row holds it"


def check_rank_bracket(ranks, sim64, qrow, targets, atol):
    """Float tables, whose keys are not exact: every rank lies in
    [#{sim64 > s_t + atol}, #{sim64 >= s_t - atol} - 1] (the rows surely before
    the target, and all that may be, less the target itself).  No pair excused."""
    for i, (r, t, rk) in enumerate(zip(np.asarray(qrow).tolist(), np.asarray(targets).tolist(),
                                       np.asarray(ranks).tolist())):
        s = sim64[r]
        lo = int((s > s[t] + atol).sum())
        hi = int((s >= s[t] - atol).sum()) - 1
        assert lo <= rk <= hi, f"rank pair {i} (query row {r}, target {t}): rank {rk} outside [{lo}, {hi}]"


def sims64(emb, q):
    """float64 similarities [len(q)][n] (parity_util.knn_sims64's formula, all columns)."""
    e = np.asarray(emb, np.float64)
    nrm = np.sqrt((e * e).sum(1))
    qq = np.asarray(q, np.int64)
    return (e[qq] @ e.T) / (nrm[qq][:, None] * nrm[None, :] + 1e-16)


def case_targets(sim_row, query, k, zero_row=None, seed=0):
    """The targets of one exact case: the query itself; the first-ranked, k-th
    and last rows; the first, a middle and the last row (by index) of the
    row's largest tie; a zero row; one target twice; 20 seeded random rows."""
    n = len(sim_row)
    order = np.lexsort((np.arange(n), -np.asarray(sim_row, np.float64)))
    vals, first, counts = np.unique(sim_row, return_index=True, return_counts=True)
    tie = np.flatnonzero(sim_row == vals[int(np.argmax(counts))])
    t = [query, order[0], order[min(k, n) - 1], order[-1], tie[0], tie[len(tie) // 2], tie[-1]]
    if zero_row is not None:
        t.append(zero_row)
    t.append(order[min(k, n) - 1])  # the same target twice
    t += np.random.default_rng(seed).integers(0, n, 20).tolist()
    return np.array(t, np.int64)
