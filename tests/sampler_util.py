"""The fused sampler's two halves against the CPU oracle (tests/test_gpu_sampler_edges.py;
tests/test_host.py checks the references against plain loops, every hand-built
row's preconditions, the oracle's tie order against torch.topk, and that the
comparisons reject planted defects).

csrc/ppr_topk.hip: walk_runs_kernel / walk_runs_seg_kernel turn a source's walk
into (node id, visit count) runs in ascending id order, the source's own id
dropped; heap_topk_kernel replays libstdc++'s partial_sort over those runs, one
lane per source.  All of it is integer work: every comparison here is exact.

References: the oracle's trace (oracle.walk_philox / walk_mt) -> runs_from_trace
-> dense_from_runs -> oracle.topk -> norm_pair.  Nothing comes from the device.
"""
import numpy as np

# sentinels the device outputs are pre-filled with: an unwritten live element
# and a write past the live part both show
SENT_U32 = 0x7F7F7F7F                 # runs, as memset 0x7f leaves them
SENT_I = -1                           # n_runs, ids
SENT_F64_BITS = 0x7FF80000DEADBEEF    # NaNs with a payload no arithmetic produces
SENT_F32_BITS = 0x7FC0BEEF

ERR_UNSET = 0x7F7F7F7F                # the walk's error word when no source failed
ERR_ARG, ERR_WORKSPACE, ERR_GRAPH = -2, -3, -4


# ----------------------------------------------------------------------------- references
def runs_from_trace(trace_row, src):
    """int64 [nr][2]: (id, count) of one source's trace in ascending id order,
    the source's own id removed (visit_prob[:, self] = 0)."""
    ids, cnt = np.unique(np.asarray(trace_row, np.int64).reshape(-1), return_counts=True)
    keep = ids != int(src)
    return np.stack([ids[keep], cnt[keep].astype(np.int64)], 1).reshape(-1, 2)


def dense_from_runs(runs, n_all, n_hops):
    """float64 [n_all]: count / n_hops at every run's id, zero elsewhere."""
    runs = np.asarray(runs, np.int64).reshape(-1, 2)
    row = np.zeros(n_all, np.float64)
    row[runs[:, 0]] = runs[:, 1].astype(np.float64) / np.float64(n_hops)
    return row


def norm_pair(w, nb, t_norm):
    """The device table's pair: float32(w / rowsum) over the first t_norm
    columns, rowsum their float64 sum in output order (left to right), int32
    ids.  A row of zeros gives 0 / 0 = NaN, as the reference's division does."""
    w = np.asarray(w, np.float64)
    rowsum = np.zeros(w.shape[0], np.float64)
    for j in range(t_norm):            # sequential, as the kernel adds them
        rowsum = rowsum + w[:, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        wn = (w[:, :t_norm] / rowsum[:, None]).astype(np.float32)
    return wn, np.asarray(nb)[:, :t_norm].astype(np.int32)


def topk_reference(rows, n_all, n_hops, k, t_norm=0, chunk_bytes=64 << 20):
    """oracle.topk of every row's dense float64 visit row: (w f64 [n][k], nb i64
    [n][k], wn f32 [n][t_norm], nb32 i32 [n][t_norm]) (the last two None without
    t_norm).  rows: a list of runs.  Dense rows are built chunk by chunk."""
    from oracle import oracle as orc
    n = len(rows)
    w = np.zeros((n, k), np.float64)
    nb = np.zeros((n, k), np.int64)
    step = max(1, int(chunk_bytes // (8 * n_all)))
    for r0 in range(0, n, step):
        dense = np.stack([dense_from_runs(r, n_all, n_hops) for r in rows[r0:r0 + step]])
        w[r0:r0 + step], nb[r0:r0 + step] = orc.topk(dense, k)
    if not t_norm:
        return w, nb, None, None
    return (w, nb) + norm_pair(w, nb, t_norm)


def heap_G(n_src, k):
    """launch_heap_topk's sources per workgroup (ppr_topk.hip), restated: a
    change of the launcher's rule makes the G table of the tests wrong, which
    test_heap_G_table then reports as a test to revisit."""
    kp = k | 1
    G = 64
    while G > 1 and G * kp * 4 > 64 * 1024:
        G >>= 1
    while G > 1 and -(-n_src // G) < 1024:
        G >>= 1
    return G


# n_src -> G at k = 10 (the sizes at which the launcher's halving changes G; all
# leave a short last block but 65 473 + 37, whose last block holds 38 sources)
G_TABLE = {1: 1, 63: 1, 2046: 1, 2047: 2, 4093: 4, 8185: 8, 16369: 16, 32737: 32, 65473: 64, 65473 + 37: 64}
# (k, n_src) -> G where the 64 KB of LDS bound G
G_LDS_TABLE = {(1000, 16369): 16, (8191, 2047): 2, (16383, 3): 1}


# ----------------------------------------------------------------------------- exact comparison
def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64), SENT_F64_BITS
    if a.dtype == np.float32:
        return a.view(np.uint32), SENT_F32_BITS
    return a, None


def check_exact(name, got, want):
    """got == want element for element, rows = sources.  Floats are compared as
    bits, except that a reference NaN (the 0 / 0 of a source without runs)
    matches any NaN other than the sentinel.  The first difference raises an
    AssertionError naming the source index and the column."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        raise AssertionError(f"{name}: {got.dtype}{got.shape}, reference {want.dtype}{want.shape}")
    gb, sent = _bits(got)
    wb, _ = _bits(want)
    eq = gb == wb
    if sent is not None:
        eq |= np.isnan(want) & np.isnan(got) & (gb != sent) & (wb != sent)
    if eq.all():
        return
    bad = np.argwhere(~eq)
    idx = tuple(int(v) for v in bad[0])
    col = idx[1:] if len(idx) > 1 else (0,)
    col_s = str(col[0]) if len(col) == 1 else str(col)
    g, w = got[idx], want[idx]
    if sent is not None:
        raise AssertionError(f"{name}: source {idx[0]} column {col_s}: got {float(g)!r} (0x{int(gb[idx]):x}), reference "
                             f"{float(w)!r} (0x{int(wb[idx]):x}); {len(bad)} of {want.size} entries differ")
    raise AssertionError(f"{name}: source {idx[0]} column {col_s}: got {int(g)}, reference {int(w)}; "
                         f"{len(bad)} of {want.size} entries differ")


def expected_runs(rows, cap, n_hops):
    """(runs uint32 [cap][n_hops][2], n_runs int32 [cap]) a launch must leave:
    rows[s] in the first len(rows[s]) pairs of source s (None: a source whose
    walk failed -- n_runs 0, nothing written), sentinels everywhere else."""
    runs = np.full((cap, n_hops, 2), SENT_U32, np.uint32)
    n_runs = np.full(cap, SENT_I, np.int32)
    for s, r in enumerate(rows):
        r = np.zeros((0, 2), np.int64) if r is None else np.asarray(r, np.int64).reshape(-1, 2)
        assert len(r) <= n_hops
        runs[s, :len(r)] = r.astype(np.uint32)
        n_runs[s] = len(r)
    return runs, n_runs


def check_runs(name, got_runs, got_n, rows, n_hops):
    """The device's runs buffer and counts against the rows of the reference
    (list of runs per live source, see expected_runs): counts, the first n_runs
    pairs, and the sentinels past them and past the live sources.  A message
    names the source and the column (pair index * 2 + {0: id, 1: count})."""
    got_runs = np.asarray(got_runs)
    cap = got_runs.shape[0]
    want_runs, want_n = expected_runs(rows, cap, n_hops)
    check_exact(name + " n_runs", np.asarray(got_n).reshape(cap, 1), want_n.reshape(cap, 1))
    check_exact(name + " runs (column = 2 * pair + {0: id, 1: count})", got_runs.reshape(cap, 2 * n_hops),
                want_runs.reshape(cap, 2 * n_hops))


def expected_topk(ref, live, cap):
    """The four outputs a top-k launch must leave over a capacity of cap rows:
    ref = (w, nb, wn, nb32) of the live rows (None where not asked), sentinels
    from row `live` on."""
    out = []
    for a, (dt, fill) in zip(ref, ((np.float64, SENT_F64_BITS), (np.int64, SENT_I), (np.float32, SENT_F32_BITS),
                                   (np.int32, SENT_I))):
        if a is None:
            out.append(None)
            continue
        e = sentinel_array((cap,) + a.shape[1:], dt)
        e[:live] = a[:live]
        out.append(e)
    return out


def sentinel_array(shape, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return np.full(shape, SENT_F64_BITS, np.uint64).view(np.float64)
    if dtype == np.float32:
        return np.full(shape, SENT_F32_BITS, np.uint32).view(np.float32)
    if dtype == np.uint32:
        return np.full(shape, SENT_U32, np.uint32)
    return np.full(shape, SENT_I, dtype)


TOPK_NAMES = ("w_out", "nb_out", "wn_out", "nb32_out")


def check_topk(name, got, want):
    """got / want: (w, nb, wn, nb32) with None where a pair was not asked."""
    for nm, g, w in zip(TOPK_NAMES, got, want):
        if w is None:
            assert g is None, f"{name} {nm}: an output the launch was not given"
            continue
        check_exact(f"{name} {nm}", g, w)


# ----------------------------------------------------------------------------- hand-built runs
def check_row_preconditions(runs, n_hops, n_all=None):
    """what heap_topk_kernel assumes of a source's runs (it checks none of it)"""
    r = np.asarray(runs, np.int64).reshape(-1, 2)
    assert len(r) <= n_hops, "more runs than hops"
    assert (r[:, 0] >= 0).all() and (np.diff(r[:, 0]) > 0).all(), "ids not strictly ascending"
    assert (r[:, 1] >= 1).all(), "a count below 1"
    assert r[:, 1].sum() <= n_hops, "counts sum above n_hops"
    if n_all is not None:
        assert (r[:, 0] < n_all).all(), "an id outside the row"


def topk_n_all(k, n_hops):
    """a row width in the partial_sort regime (k * 64 <= n_all) with room for
    n_hops sparse ids"""
    return max(64 * k, k + 4 * n_hops)


def _counts(rng, nr, n_hops, extra=None):
    """nr counts >= 1 summing to <= n_hops"""
    c = np.ones(nr, np.int64)
    if nr == 0:
        return c
    extra = int(rng.integers(0, n_hops - nr + 1)) if extra is None else extra
    np.add.at(c, rng.integers(0, nr, extra), 1)
    return c


def _row(below, sparse, counts):
    ids = np.concatenate([np.sort(np.asarray(below, np.int64)), np.sort(np.asarray(sparse, np.int64))])
    return np.stack([ids, np.asarray(counts, np.int64)], 1).reshape(-1, 2)


def topk_catalogue(n_hops, k, seed=0, n_random=160):
    """[(name, runs int64 [nr][2])]: the hand-built rows of the issue at (n_hops,
    k), ids below topk_n_all(k, n_hops), plus n_random random rows.  'below' ids
    are < k (they set a dense heap entry), 'sparse' ids >= k (they go through
    the eight-at-a-time prefetch)."""
    rng = np.random.default_rng(1000 * k + n_hops + seed)
    n_all = topk_n_all(k, n_hops)

    def below(m):
        return rng.choice(k, m, replace=False)

    def sparse(m):
        return k + rng.choice(n_all - k, m, replace=False)

    rows = []
    # nr at and around the prefetch width, 0 and the most a walk can give
    for nr in (0, 1, 7, 8, 9, 15, 16, 17, n_hops):
        if nr > n_hops:
            continue
        for rep in range(2):
            nb = int(rng.integers(0, min(nr, k) + 1))
            rows.append((f"nr{nr}-mix{rep}", _row(below(nb), sparse(nr - nb), _counts(rng, nr, n_hops))))
        rows.append((f"nr{nr}-sparse", _row([], sparse(nr), _counts(rng, nr, n_hops))))
    # all runs below k (the sparse loop never runs), all at or above k
    for m in sorted({1, min(k, n_hops), max(1, min(k, n_hops) // 2)}):
        rows.append((f"below-only{m}", _row(below(m), [], _counts(rng, m, n_hops))))
    # the first sparse run at index p of the row, the sparse tail t runs long;
    # 'hi': every sparse count above every dense one (each enters the heap)
    for p in (0, 7, 8, 9):
        if p > k:
            continue
        for t in (1, 7, 8, 9, 16):
            if p + t > n_hops:
                continue
            rows.append((f"first-sparse{p}-tail{t}", _row(below(p), sparse(t), _counts(rng, p + t, n_hops))))
            if p + 2 * t <= n_hops:
                rows.append((f"first-sparse{p}-tail{t}-hi",
                             _row(below(p), sparse(t), np.concatenate([np.ones(p, np.int64), np.full(t, 2)]))))
    # all counts equal: pure tie order against the dense zeros 0 .. k-1
    for c in (1, 2, 3):
        for m in sorted({n_hops // c, max(1, n_hops // (2 * c)), min(k + 1, n_hops // c)}):
            if m < 1:
                continue
            nb = int(rng.integers(0, min(m, k) + 1))
            rows.append((f"equal{c}x{m}", _row(below(nb), sparse(m - nb), np.full(m, c))))
            rows.append((f"equal{c}x{m}-sparse", _row([], sparse(m), np.full(m, c))))
    # counts strictly increasing / decreasing in id
    m = 1
    while (m + 1) * (m + 2) // 2 <= n_hops:
        m += 1
    for nb in sorted({0, min(m, k) // 2, min(m, k)}):
        rows.append((f"increasing-b{nb}", _row(below(nb), sparse(m - nb), np.arange(1, m + 1))))
        rows.append((f"decreasing-b{nb}", _row(below(nb), sparse(m - nb), np.arange(m, 0, -1))))
    # one dominant count among ones
    for nr in sorted({1, min(9, n_hops), min(17, n_hops)}):
        for at in sorted({0, nr // 2, nr - 1}):
            c = np.ones(nr, np.int64)
            c[at] = n_hops - (nr - 1)
            nb = int(rng.integers(0, min(nr, k) + 1))
            rows.append((f"dominant-nr{nr}-at{at}", _row(below(nb), sparse(nr - nb), c)))
    # fewer non-zero entries than k: the tail is zeros in libstdc++'s order
    for m in sorted({0, 1, k // 2, k - 1}):
        if 0 <= m <= n_hops and m < k:
            rows.append((f"fewer{m}-than-k", _row([], sparse(m), _counts(rng, m, n_hops))))
    for i in range(n_random):
        nr = int(rng.integers(0, n_hops + 1))
        nb = int(rng.integers(0, min(nr, k) + 1))
        rows.append((f"random{i}", _row(below(nb), sparse(nr - nb), _counts(rng, nr, n_hops))))
    return rows


def trace_from_runs(runs, src, n_hops, rng):
    """a trace (int32 [n_hops], shuffled) whose visit counts are the runs, the
    remaining hops at the source itself (dropped by the counting)"""
    r = np.asarray(runs, np.int64).reshape(-1, 2)
    assert not (r[:, 0] == src).any()
    t = np.concatenate([np.repeat(r[:, 0], r[:, 1]), np.full(n_hops - int(r[:, 1].sum()), src, np.int64)])
    return rng.permutation(t).astype(np.int32)


# pinsage_visit_topk on hand-built traces: (n_all, k) on both sides of k * 64 <=
# n_all, k = n_all, k = 1, n_all = 1
VISIT_SHAPES = [(640, 10), (639, 10), (64, 1), (63, 1), (100, 100), (100, 99), (5, 5), (1, 1)]
VISIT_N_HOPS = 48


def visit_rows(n_all, k, n_hops, rng):
    """(rows, sources): hand-built rows of a width-n_all visit row -- all ties,
    one dominant count, mixed -- and a source outside each row's ids"""
    rows, srcs = [], []
    ids_all = np.arange(n_all)
    for kind in ("ties", "dominant", "mixed", "empty", "full"):
        src = int(rng.integers(0, n_all))
        pool = ids_all[ids_all != src]
        if kind == "empty" or len(pool) == 0:
            r = np.zeros((0, 2), np.int64)
        else:
            m = {"ties": min(len(pool), n_hops // 2), "dominant": min(len(pool), 9), "mixed": min(len(pool), 17),
                 "full": min(len(pool), n_hops)}[kind]
            ids = np.sort(rng.choice(pool, m, replace=False))
            if kind == "ties":
                c = np.full(m, 2)
            elif kind == "dominant":
                c = np.ones(m, np.int64)
                c[int(rng.integers(0, m))] = n_hops - (m - 1)
            elif kind == "full":
                c = np.ones(m, np.int64)
            else:
                c = _counts(rng, m, n_hops)
            r = np.stack([ids, c], 1)
        check_row_preconditions(r, n_hops, n_all)
        rows.append(r)
        srcs.append(src)
    return rows, np.array(srcs, np.int64)


# ----------------------------------------------------------------------------- graphs
def bipartite_graph(n_items=300, n_pl=300, seed=5):
    """(indptr int64, indices int32, n_all, special ids): items 0 .. n_items-1,
    playlists after them, both directions in one CSR.  Degrees from 1 to hubs of
    ~n: item 0 is in every shared playlist, playlist n_items holds every shared
    item.  `loner` (the last item) has one playlist that holds it alone: every
    hop from it returns to it.  The largest id is an ordinary playlist."""
    rng = np.random.default_rng(seed)
    n_all = n_items + n_pl
    loner, loner_pl = n_items - 1, n_items + 1
    edges = set()
    for i in range(n_items - 1):
        edges.add((i, n_items))                                  # the hub playlist
    for p in range(n_items, n_all):
        if p != loner_pl:
            edges.add((0, p))                                    # the hub item
    for i in range(1, n_items - 1):
        for p in rng.integers(n_items + 2, n_all, int(rng.integers(0, 9))):
            edges.add((i, int(p)))
    edges.add((loner, loner_pl))
    return _csr(edges, n_all) + (n_all, dict(loner=loner, hub=0, largest=n_all - 1, deg1=None))


def _csr(edges, n_all, both=True, seed=0):
    adj = [[] for _ in range(n_all)]
    for a, b in sorted(edges):
        adj[a].append(b)
        if both:
            adj[b].append(a)
    rng = np.random.default_rng(seed)
    for a in adj:                       # insertion order is arbitrary to the walk: shuffle it
        rng.shuffle(a)
    indptr = np.zeros(n_all + 1, np.int64)
    indptr[1:] = np.cumsum([len(a) for a in adj])
    indices = np.array([v for a in adj for v in a], np.int32)
    return indptr, indices


def two_item_graph():
    """items 0 and 1 in one playlist 2: every hop lands on the source or on the
    one other item (runs of one pair, counts up to n_hops)."""
    return _csr({(0, 2), (1, 2)}, 3) + (3, {})


def zero_degree_graphs():
    """[(name, indptr, indices, n_all, sources, bad)]: the handled error path.
    'source': item 6 has no out-edges.  'sink': playlist 9 is a column without
    out-edges (a directed CSR), items 4 and 5 link only to it.  Every id lies
    inside the graph; bad = the indices of the sources whose walk must fail."""
    out = []
    # items 0..6, playlists 7..9
    e = {(0, 7), (1, 7), (2, 7), (2, 8), (3, 8), (0, 8), (4, 9), (5, 9), (1, 9)}
    indptr, indices = _csr(e, 10)
    src = np.array([0, 1, 2, 6, 3, 6, 4, 0], np.int64)
    out.append(("source", indptr, indices, 10, src, [3, 5]))
    # directed: playlists 7, 8 link back, 9 does not; items 4, 5 reach only 9
    adj = {0: [7, 8], 1: [7], 2: [7, 8], 3: [8], 4: [9], 5: [9], 6: [7], 7: [0, 1, 2, 6], 8: [0, 2, 3], 9: []}
    indptr = np.zeros(11, np.int64)
    indptr[1:] = np.cumsum([len(adj[i]) for i in range(10)])
    indices = np.array([v for i in range(10) for v in adj[i]], np.int32)
    src = np.array([0, 1, 3, 2, 5, 6, 4, 2], np.int64)
    out.append(("sink", indptr, indices, 10, src, [4, 6]))
    return out


def oracle_traces(indptr, indices, sources, n_hops, alpha, mt=None, seed=0, offset=0, src_base=0):
    """One oracle trace per source (None where its walk met a zero-degree node),
    source by source: Philox position src_base + i, or the MT stream `mt` (an
    oracle.MT, left where the reference's consumption of 3 n_hops draws per
    source ends -- a failed source's draws included, as the device expands them)."""
    from oracle import oracle as orc
    out = []
    for i, s in enumerate(np.asarray(sources, np.int64)):
        try:
            if mt is None:
                tr = orc.walk_philox(indptr, indices, [s], n_hops, alpha, seed, offset, src_base + i)
            else:
                before = mt.buf.copy()
                tr = orc.walk_mt(indptr, indices, [s], n_hops, alpha, mt)
            out.append(tr[0])
        except RuntimeError:
            if mt is not None:
                mt.buf[:] = before
                mt.draws(3 * n_hops)
            out.append(None)
    return out


def oracle_runs(traces, sources):
    return [None if t is None else runs_from_trace(t, s) for t, s in zip(traces, np.asarray(sources, np.int64))]
