"""The fused sampler's walk and heap replay at their edges, bit-exact
(csrc/ppr_topk.hip: walk_runs_kernel, walk_runs_seg_kernel, heap_topk_kernel)
through the test entries pinsage_walk_runs / pinsage_runs_topk /
pinsage_walk_runs_seg.  References and comparisons: tests/sampler_util.py (the
CPU oracle's traces and top-k; nothing from the device).  Every output buffer
is pre-filled with sentinels; everything is compared with ==.

The four regimes no other test reaches, and the tests that name them:
  1. the lane-chain resolution and the carry between 64-hop rounds at alpha 0 /
     0.5 / 1 and n_hops 1 .. 8192:                  test_walk_runs_*
  2. heap_topk_kernel with G > 1 live lanes:        test_runs_topk_G_*
  3. the eight-at-a-time prefetch's boundaries, nr == 0, the device-side count:
                                                    test_runs_topk_row_shapes, _device_count, _empty_row
  4. walk_runs_seg_kernel with empty segments and a capacity grid:
                                                    test_walk_runs_seg
"""
import numpy as np
import pytest
import torch

import sampler_util as su

pytestmark = pytest.mark.gpu

N_HOPS_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 500, 4096, 8191, 8192)
ALPHAS = (0.0, 0.5, 0.85, 1.0)


# ----------------------------------------------------------------------------- device plumbing
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sent(shape, dtype):
    return _dev(su.sentinel_array(shape, dtype))


def _np(t):
    return None if t is None else t.cpu().numpy()


class _Graph:
    def __init__(self, indptr, indices, n_all):
        self.indptr, self.indices, self.n_all = indptr, indices, n_all
        self.d_indptr, self.d_indices = _dev(indptr), _dev(indices)


def walk_runs(g, sources, n_hops, alpha, mt=None, seed=0, offset=0, src_base=0):
    """pinsage_walk_runs -> (rc, runs uint32 [n][n_hops][2], n_runs int32 [n], err)"""
    import _native as nat
    L = nat.lib()
    n = len(sources)
    src = _dev(np.asarray(sources, np.int64))
    runs = _sent((n, n_hops, 2), np.uint32)
    n_runs = _sent((n,), np.int32)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws, ws_bytes = None, 0
    if mt is not None:
        ws_bytes = L.pinsage_walk_mt_workspace(n, n_hops)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = L.pinsage_walk_runs(nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, nat.ptr(src), n, n_hops,
                             float(np.float32(alpha)), mt.p if mt is not None else None, seed, offset, src_base,
                             nat.ptr(ws), ws_bytes, nat.ptr(runs), nat.ptr(n_runs), nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, _np(runs), _np(n_runs), int(err.item())


def runs_topk(runs, n_runs, n_hops, k, t_norm=0, want_ref=True, n_src_dev=None, cap=None):
    """pinsage_runs_topk over host arrays runs uint32 [cap][n_hops][2] / n_runs
    int32 [cap] -> (rc, (w, nb, wn, nb32) device tensors, None where not asked)"""
    import _native as nat
    cap = len(n_runs) if cap is None else cap
    d_runs, d_n = _dev(runs), _dev(n_runs)
    w = _sent((cap, k), np.float64) if want_ref else None
    nb = _sent((cap, k), np.int64) if want_ref else None
    wn = _sent((cap, t_norm), np.float32) if t_norm else None
    nb32 = _sent((cap, t_norm), np.int32) if t_norm else None
    cnt = None if n_src_dev is None else torch.tensor([n_src_dev], dtype=torch.int32, device="cuda")
    rc = nat.lib().pinsage_runs_topk(nat.ptr(d_runs), nat.ptr(d_n), cap, n_hops, k, nat.ptr(cnt), nat.ptr(w),
                                     nat.ptr(nb), nat.ptr(wn), nat.ptr(nb32), t_norm, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, (w, nb, wn, nb32)


def _pack(rows, n_hops):
    """catalogue rows -> (runs uint32 [m][n_hops][2] sentinel-padded, n_runs int32 [m])"""
    return su.expected_runs(rows, len(rows), n_hops)


def _check_topk_assigned(name, got, ref, assign, live):
    """device outputs of `cap` rows against ref[assign[s]] for s < live and the
    sentinels from `live` on, in row chunks (host memory stays small)"""
    cap = next(t.shape[0] for t in got if t is not None)
    step = max(1, (16 << 20) // (8 * max(t.shape[1] for t in got if t is not None)))
    for r0 in range(0, cap, step):
        r1 = min(cap, r0 + step)
        lv = min(max(live - r0, 0), r1 - r0)
        sel = assign[r0:r0 + lv]
        want = su.expected_topk([None if a is None else a[sel] for a in ref], lv, r1 - r0)
        su.check_topk(f"{name} rows {r0}..", [None if t is None else _np(t[r0:r1]) for t in got], want)


# ----------------------------------------------------------------------------- walk -> runs
_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        indptr, indices, n_all, special = su.bipartite_graph() if name == "bipartite" else su.two_item_graph()
        g = _Graph(indptr, indices, n_all)
        if name == "bipartite":
            rng = np.random.default_rng(3)
            # id 0 (the hub item), the largest id, the loner (n_runs == 0), one id three times, a degree-1 item
            deg = np.diff(indptr)
            deg1 = int(np.flatnonzero(deg[:special["loner"]] == 1)[0])
            g.sources = np.concatenate([[0, n_all - 1, special["loner"], 17, 17, deg1, 17, special["loner"]],
                                        rng.integers(0, n_all, 28)]).astype(np.int64)
            g.loner_at = (2, 7)
        else:
            g.sources = np.array([0, 1, 1, 0, 2], np.int64)
            g.loner_at = (4,)  # the playlist as a source: every hop comes back to it
        _GRAPHS[name] = g
    return _GRAPHS[name]


def _walk_case(g, n_hops, alpha, mode, seed):
    """one launch against the oracle, source by source"""
    import _native as nat
    from oracle import oracle as orc
    if mode == "mt19937":
        mt_dev, mt_ref = nat.MT().seed(seed), orc.MT(seed)
        rc, runs, n_runs, err = walk_runs(g, g.sources, n_hops, alpha, mt=mt_dev)
        traces = su.oracle_traces(g.indptr, g.indices, g.sources, n_hops, np.float32(alpha), mt=mt_ref)
    else:
        # a non-zero offset, and a source position past 2^32 (both counter words)
        offset, base = 7, (1 << 33) + 5
        rc, runs, n_runs, err = walk_runs(g, g.sources, n_hops, alpha, seed=seed, offset=offset, src_base=base)
        traces = su.oracle_traces(g.indptr, g.indices, g.sources, n_hops, np.float32(alpha), seed=seed,
                                  offset=offset, src_base=base)
    name = f"walk_runs {mode} n_hops={n_hops} alpha={alpha}"
    assert rc == 0 and err == su.ERR_UNSET, (name, rc, err)
    rows = su.oracle_runs(traces, g.sources)
    su.check_runs(name, runs, n_runs, rows, n_hops)
    for s in g.loner_at:  # every hop came back to the source: its own run is dropped
        assert n_runs[s] == 0, (name, s)
    if mode == "mt19937":  # the generator ends where the oracle's ends
        assert (mt_dev.draws(8) == mt_ref.draws(8)).all(), name
    return rows


@pytest.mark.parametrize("mode", ["mt19937", "philox"])
@pytest.mark.parametrize("n_hops", N_HOPS_EDGES)
def test_walk_runs_bipartite(mode, n_hops):
    """Regime 1 on the bipartite graph (degrees 1 .. 300): alpha 0 makes every
    lane wait for its predecessor (64 rounds of the resolution loop, a
    non-restart carry at every 64-hop boundary), alpha 1 never leaves the
    source's rows; n_hops on both sides of one and two rounds, powers of two
    (P == n_hops: no padding keys) and the LDS limit 8192."""
    g = _graph("bipartite")
    for alpha in ALPHAS:
        rows = _walk_case(g, n_hops, alpha, mode, seed=1000 + n_hops)
        if alpha == 0.0 and n_hops >= 64:  # the walk really left the source's rows
            assert max(len(r) for r in rows) > 4


@pytest.mark.parametrize("mode", ["mt19937", "philox"])
def test_walk_runs_two_item_graph(mode):
    """Regime 1 where every hop lands on the source or on one other id: one run
    at most, counts up to n_hops (8192 = the largest a run can hold)."""
    g = _graph("two_item")
    for n_hops in N_HOPS_EDGES:
        for alpha in ALPHAS:
            rows = _walk_case(g, n_hops, alpha, mode, seed=77 + n_hops)
            assert all(len(r) <= 1 for r in rows)


@pytest.mark.parametrize("mode", ["mt19937", "philox"])
def test_walk_runs_zero_degree(mode):
    """The handled error path: a source without out-edges, and a playlist column
    that is a sink (the cd == 0 branch).  PINSAGE_ERR_GRAPH, the smallest
    offending source index in the error word, n_runs == 0 for the failed
    sources and exact runs for the others of the same launch."""
    import _native as nat
    from oracle import oracle as orc
    for name, indptr, indices, n_all, sources, bad in su.zero_degree_graphs():
        g = _Graph(indptr, indices, n_all)
        for n_hops, alpha in ((1, 0.5), (65, 0.0), (130, 0.85)):
            if mode == "mt19937":
                mt_dev, mt_ref = nat.MT().seed(5), orc.MT(5)
                rc, runs, n_runs, err = walk_runs(g, sources, n_hops, alpha, mt=mt_dev)
                traces = su.oracle_traces(indptr, indices, sources, n_hops, np.float32(alpha), mt=mt_ref)
                assert (mt_dev.draws(8) == mt_ref.draws(8)).all()
            else:
                rc, runs, n_runs, err = walk_runs(g, sources, n_hops, alpha, seed=9, offset=3, src_base=11)
                traces = su.oracle_traces(indptr, indices, sources, n_hops, np.float32(alpha), seed=9, offset=3,
                                          src_base=11)
            what = f"zero degree ({name}) {mode} n_hops={n_hops}"
            assert [i for i, t in enumerate(traces) if t is None] == bad, what
            assert rc == su.ERR_GRAPH, (what, rc)
            assert err == min(bad), (what, err)
            su.check_runs(what, runs, n_runs, su.oracle_runs(traces, sources), n_hops)
            assert all(n_runs[i] == 0 for i in bad)


def test_walk_runs_refusals():
    """n_hops above the LDS sort's 8192 and a short MT workspace are refused
    with the project's codes and nothing written."""
    import _native as nat
    g = _graph("two_item")
    rc, runs, n_runs, err = walk_runs(g, g.sources, 8193, 0.5, seed=1)
    assert rc == su.ERR_ARG and err == 0
    su.check_runs("refused walk", runs, n_runs, [], 8193)
    L = nat.lib()
    n, h = len(g.sources), 64
    src, runs_d, nr_d = _dev(g.sources), _sent((n, h, 2), np.uint32), _sent((n,), np.int32)
    err_d = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = L.pinsage_walk_mt_workspace(n, h) - 256
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    mt = nat.MT().seed(1)
    rc = L.pinsage_walk_runs(nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, nat.ptr(src), n, h, 0.5, mt.p, 0, 0, 0,
                             nat.ptr(ws), ws_bytes, nat.ptr(runs_d), nat.ptr(nr_d), nat.ptr(err_d), nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == su.ERR_WORKSPACE
    su.check_runs("refused walk (workspace)", _np(runs_d), _np(nr_d), [], h)
    assert (mt.draws(4) == nat.MT().seed(1).draws(4)).all()  # no draw consumed


# ----------------------------------------------------------------------------- runs -> top-k
_CAT = {}


def _catalogue(n_hops, k, t_norm, n_random=160, every=1):
    """(rows, packed runs, packed n_runs, reference (w, nb, wn, nb32)) of the
    hand-built rows, built once per shape and left unchanged"""
    key = (n_hops, k, t_norm, n_random, every)
    if key not in _CAT:
        cat = su.topk_catalogue(n_hops, k, n_random=n_random)[::every]
        rows = [r for _, r in cat]
        n_all = su.topk_n_all(k, n_hops)
        for r in rows:
            su.check_row_preconditions(r, n_hops, n_all)
        ref = su.topk_reference(rows, n_all, n_hops, k, t_norm)
        for a in ref:
            if a is not None:
                a.setflags(write=False)
        _CAT[key] = (cat, *_pack(rows, n_hops), ref)
    return _CAT[key]


def _launch_assigned(n_src, n_hops, k, t_norm, cat_key, seed, want_ref=True, n_src_dev=None):
    """n_src sources, each a random row of the catalogue (neighbouring lanes
    hold different rows): launch and compare every row"""
    cat, c_runs, c_n, ref = _catalogue(n_hops, k, t_norm, *cat_key)
    assign = np.random.default_rng(seed).integers(0, len(cat), n_src)
    assign[:min(n_src, len(cat))] = np.arange(len(cat))[:n_src]  # every row at least once where they fit
    rc, got = runs_topk(c_runs[assign], c_n[assign], n_hops, k, t_norm, want_ref, n_src_dev)
    assert rc == 0, rc
    live = n_src if n_src_dev is None else min(n_src, n_src_dev)
    ref = ref if want_ref else (None, None) + ref[2:]
    _check_topk_assigned(f"runs_topk n_src={n_src} k={k} G={su.heap_G(n_src, k)}", got, ref, assign, live)


def test_heap_G_table():
    """The G the launcher's rule gives for each size the tests below rely on
    (su.heap_G restates launch_heap_topk's rule: if the rule changes, this table
    and the sizes chosen from it are to be revisited)."""
    for n_src, G in su.G_TABLE.items():
        assert su.heap_G(n_src, 10) == G, (n_src, G)
    for (k, n_src), G in su.G_LDS_TABLE.items():
        assert su.heap_G(n_src, k) == G, (k, n_src, G)
    assert su.heap_G(1 << 20, 1000) == 16 and su.heap_G(1 << 20, 8191) == 2 and su.heap_G(1 << 20, 16383) == 1
    assert (16384 | 1) * 4 > 64 * 1024  # k = 16 384: one heap does not fit


@pytest.mark.parametrize("n_src", list(su.G_TABLE))
def test_runs_topk_G(n_src):
    """Regime 2: G = 1, 1, 1, 2, 4, 8, 16, 32, 64 and 64 with a short last block
    (n_hops 24, k 10): the heaps at stride kp = k | 1, `lane < G && s < n_src` on
    the last block, nb_blk, and the cooperative output loop reading another
    lane's heap and rowsum[q] -- every row of the launch compared."""
    _launch_assigned(n_src, 24, 10, 4, (160, 1), seed=n_src)


@pytest.mark.parametrize("k,n_src", list(su.G_LDS_TABLE))
def test_runs_topk_G_lds_limit(k, n_src):
    """Regime 2 where the 64 KB of LDS bound G: k = 1000 (G = 16), k = 8191
    (G = 2), k = 16 383 (G = 1: one heap fills the LDS)."""
    _launch_assigned(n_src, 24, k, 25, (0, {1000: 3, 8191: 12, 16383: 30}[k]), seed=k)


def test_runs_topk_k_too_large_refused():
    """k = 16 384: one heap does not fit the LDS -- refused, outputs untouched;
    and the host-side refusals of the production entry."""
    import _native as nat
    row = np.array([[3, 2], [20000, 5]])
    # (k, t_norm, n_hops): the LDS refusal; k < 1; t_norm > k; n_hops > 8192; k + n_hops == 65536
    for k, t_norm, n_hops in ((16384, 4, 24), (0, 1, 24), (10, 11, 24), (10, 1, 8193), (65536 - 24, 1, 24)):
        d_runs, d_n = (_dev(a) for a in _pack([row] * 3, n_hops))
        # outputs of the full size the call names: were it not refused, nothing would be written outside them
        outs = (_sent((3, max(k, 1)), np.float64), _sent((3, max(k, 1)), np.int64), _sent((3, t_norm), np.float32),
                _sent((3, t_norm), np.int32))
        rc = nat.lib().pinsage_runs_topk(nat.ptr(d_runs), nat.ptr(d_n), 3, n_hops, k, None,
                                         *(nat.ptr(t) for t in outs), t_norm, nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == su.ERR_ARG, (k, t_norm, n_hops, rc)
        for t in outs:
            su.check_exact(f"refused k={k}", _np(t), su.sentinel_array(tuple(t.shape), _np(t).dtype))


@pytest.mark.parametrize("k", [1, 2, 3, 10, 16])
@pytest.mark.parametrize("n_hops", [24, 200])
def test_runs_topk_row_shapes(n_hops, k):
    """Regime 3: nr in {0, 1, 7, 8, 9, 15, 16, 17, n_hops}, the first sparse run
    at index 0 / 7 / 8 / 9, all runs below / at or above k, pure ties, monotone
    counts, one dominant count, fewer non-zero entries than k; k = 1 (no heap to
    make), 2 and 3 (the even and odd len branches of h_adjust); t_norm 1, k and
    a value between; each output pair alone and both together."""
    for t_norm in sorted({1, (k + 1) // 2, k}):
        _launch_assigned(400, n_hops, k, t_norm, (160, 1), seed=k)
    t = (k + 1) // 2
    _launch_assigned(400, n_hops, k, t, (160, 1), seed=k + 1, want_ref=False)  # the normalised pair alone
    _launch_assigned(400, n_hops, k, 0, (160, 1), seed=k + 2)                 # the reference pair alone


@pytest.mark.parametrize("cap", [4093, 65473])
def test_runs_topk_device_count(cap):
    """Regime 3: the count on the device under a capacity grid, as fly.hip
    launches the kernel (G = 4 and G = 64): *n_src_dev in {0, 1, G - 1, G,
    G + 1, capacity} -- and above the capacity, which the kernel clamps; rows at
    and past the count keep their sentinels."""
    G = su.heap_G(cap, 10)
    assert G == su.G_TABLE[cap]
    for count in (0, 1, G - 1, G, G + 1, 5 * G + 3, cap, cap + 9):
        _launch_assigned(cap, 24, 10, 4, (160, 1), seed=cap + count, n_src_dev=count)


def test_runs_topk_empty_row():
    """Regime 3, nr == 0 (every hop came back to the source): the reference
    pair is k zeros with ids 0 .. k-1 in libstdc++'s order, the normalised pair
    is 0 / 0 = NaN in every column (rowsum == 0) with the same ids, and
    pinsage_visit_topk writes the same bits for the same row."""
    import _native as nat
    n_hops, k, t_norm, n_all = 24, 10, 4, 640
    rows = [np.zeros((0, 2), np.int64), np.array([[3, 2], [500, 5]]), np.zeros((0, 2), np.int64)]
    ref = su.topk_reference(rows, n_all, n_hops, k, t_norm)
    assert (ref[0][0] == 0).all() and np.isnan(ref[2][0]).all() and sorted(ref[1][0]) == list(range(k))
    rc, got = runs_topk(*_pack(rows, n_hops), n_hops, k, t_norm)
    assert rc == 0
    su.check_topk("empty row (heap)", [_np(t) for t in got], ref)
    assert np.isnan(_np(got[2])[0]).all()
    # the same rows as traces through pinsage_visit_topk
    rng = np.random.default_rng(0)
    src = np.array([7, 9, 0], np.int64)
    trace = np.stack([su.trace_from_runs(r, s, n_hops, rng) for r, s in zip(rows, src)])
    outs = (_sent((3, k), np.float64), _sent((3, k), np.int64), _sent((3, t_norm), np.float32),
            _sent((3, t_norm), np.int32))
    d_trace, d_src = _dev(trace), _dev(src)
    rc = nat.lib().pinsage_visit_topk(nat.ptr(d_trace), nat.ptr(d_src), 3, n_hops, n_all, k, None,
                                      *(nat.ptr(t) for t in outs), t_norm, nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    su.check_topk("empty row (visit_topk)", [_np(t) for t in outs], ref)
    for a, b in zip(got, outs):  # the two kernels agree bit for bit, NaNs included
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ----------------------------------------------------------------------------- fused == unfused
@pytest.mark.parametrize("mode", ["mt19937", "philox"])
@pytest.mark.parametrize("n_hops", [1, 64, 65, 8192])
def test_fused_equals_unfused(mode, n_hops):
    """pinsage_ppr_topk == pinsage_walk_* followed by pinsage_visit_topk (and the
    oracle) at n_hops 1 / 64 / 65 / 8192 and alpha 0 / 1, with a whole-launch
    workspace and with one so small that the sources run in several rounds
    (R = 7 < n_src)."""
    import _native as nat
    from oracle import oracle as orc
    L = nat.lib()
    g = _graph("bipartite")
    src_h = g.sources
    n, k, t_norm = len(src_h), 5, 3
    assert k * 64 <= g.n_all
    src = _dev(src_h)
    for alpha in (0.0, 1.0):
        a32 = float(np.float32(alpha))
        # unfused: the trace in memory, then visit_topk
        trace = torch.full((n, n_hops), -1, dtype=torch.int32, device="cuda")
        seed, offset, base = 1234 + n_hops, 2, 40
        if mode == "mt19937":
            mt = nat.MT().seed(seed)
            wsb = L.pinsage_walk_mt_workspace(n, n_hops)
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            rc = L.pinsage_walk_mt(nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, nat.ptr(src), n, n_hops, a32,
                                   mt.p, nat.ptr(ws), wsb, nat.ptr(trace), nat.stream_ptr())
            traces = su.oracle_traces(g.indptr, g.indices, src_h, n_hops, np.float32(alpha), mt=orc.MT(seed))
        else:
            rc = L.pinsage_walk_philox(nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, nat.ptr(src), n, n_hops,
                                       a32, seed, offset, base, nat.ptr(trace), nat.stream_ptr())
            traces = su.oracle_traces(g.indptr, g.indices, src_h, n_hops, np.float32(alpha), seed=seed, offset=offset,
                                      src_base=base)
        assert rc == 0
        unf = (_sent((n, k), np.float64), _sent((n, k), np.int64), _sent((n, t_norm), np.float32),
               _sent((n, t_norm), np.int32))
        rc = L.pinsage_visit_topk(nat.ptr(trace), nat.ptr(src), n, n_hops, g.n_all, k, None,
                                  *(nat.ptr(t) for t in unf), t_norm, nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert (_np(trace) == np.stack(traces)).all()
        ref = su.topk_reference(su.oracle_runs(traces, src_h), g.n_all, n_hops, k, t_norm)
        what = f"{mode} n_hops={n_hops} alpha={alpha}"
        su.check_topk("unfused " + what, [_np(t) for t in unf], ref)
        for rounds, R in (("one round", n), ("rounds of 7", 7)):
            wsb = L.pinsage_ppr_topk_workspace(R, n_hops, 1 if mode == "mt19937" else 0)
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            fus = (_sent((n, k), np.float64), _sent((n, k), np.int64), _sent((n, t_norm), np.float32),
                   _sent((n, t_norm), np.int32))
            mt2 = nat.MT().seed(seed) if mode == "mt19937" else None
            rc = L.pinsage_ppr_topk(nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, nat.ptr(src), n, n_hops, a32,
                                    k, mt2.p if mt2 else None, seed, offset, base, nat.ptr(ws), wsb,
                                    *(nat.ptr(t) for t in fus), t_norm, nat.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, (what, rounds, rc)
            su.check_topk(f"fused ({rounds}) " + what, [_np(t) for t in fus], ref)
            for a, b in zip(fus, unf):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (what, rounds)
            if mt2:  # both consumed the reference's 3 n_hops draws per source
                end = nat.MT()
                end.buf[:] = mt.buf
                assert (mt2.draws(8) == end.draws(8)).all(), (what, rounds)


# ----------------------------------------------------------------------------- visit_topk on hand-built traces
@pytest.mark.parametrize("n_all,k", su.VISIT_SHAPES)
def test_visit_topk_hand_built_traces(n_all, k):
    """pinsage_visit_topk on traces written from hand-built rows, on both sides
    of k * 64 <= n_all (partial_sort / nth_element + sort), k = n_all, k = 1,
    n_all = 1 -- against oracle.topk of the dense row."""
    import _native as nat
    L = nat.lib()
    n_hops = su.VISIT_N_HOPS
    rng = np.random.default_rng(n_all * 7 + k)
    rows, src = su.visit_rows(n_all, k, n_hops, rng)
    n = len(rows)
    trace = np.stack([su.trace_from_runs(r, s, n_hops, rng) for r, s in zip(rows, src)])
    for t_norm in sorted({1, (k + 1) // 2, k}):
        ref = su.topk_reference(rows, n_all, n_hops, k, t_norm)
        outs = (_sent((n, k), np.float64), _sent((n, k), np.int64), _sent((n, t_norm), np.float32),
                _sent((n, t_norm), np.int32))
        sb = L.pinsage_visit_topk_scratch(n, n_all, k)
        scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device="cuda")
        d_trace, d_src = _dev(trace), _dev(src)
        rc = L.pinsage_visit_topk(nat.ptr(d_trace), nat.ptr(d_src), n, n_hops, n_all, k,
                                  nat.ptr(scratch) if sb else None, *(nat.ptr(t) for t in outs), t_norm,
                                  nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        su.check_topk(f"visit_topk n_all={n_all} k={k} t_norm={t_norm}", [_np(t) for t in outs], ref)


# ----------------------------------------------------------------------------- segmented walk
def _walk_runs_seg(g, sources, dtype, cap, seg, seeds, key_stride, id_unit, n_hops, alpha, offset):
    import _native as nat
    src = _dev(np.asarray(sources, dtype))
    runs = _sent((cap, n_hops, 2), np.uint32)
    n_runs = _sent((cap,), np.int32)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_seg = _dev(np.asarray(seg, np.int32))
    d_seeds = _dev(np.asarray(seeds, np.uint64).view(np.int64))
    s64, s32 = (nat.ptr(src), None) if dtype == np.int64 else (None, nat.ptr(src))
    rc = nat.lib().pinsage_walk_runs_seg(nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, s64, s32, cap,
                                         nat.ptr(d_seg), len(seg) - 1, nat.ptr(d_seeds), key_stride, id_unit, n_hops,
                                         float(np.float32(alpha)), offset, nat.ptr(runs), nat.ptr(n_runs),
                                         nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, _np(runs), _np(n_runs), int(err.item())


@pytest.mark.parametrize("sizes", [(5, 0, 7), (0, 0, 3), (64, 65, 1)])
def test_walk_runs_seg(sizes):
    """Regime 4: three calls with empty segments, the grid at seg[C] and 100
    above it, int64 sources (plain ids and c * id_unit + id) and int32 sources
    carrying c * id_unit + id, key_stride 1 and 2: the call lookup and the id
    rebasing.  Equal to pinsage_walk_runs launched once per call with that
    call's seed and src_base 0, and to the oracle; slots past seg[C] untouched."""
    g = _graph("bipartite")
    C, n_hops, alpha, offset = 3, 65, 0.5, 5
    seg = np.concatenate([[0], np.cumsum(sizes)])
    total = int(seg[C])
    rng = np.random.default_rng(sum(sizes))
    ids = rng.integers(0, g.n_all, total).astype(np.int64)
    call = np.repeat(np.arange(C), sizes)
    for key_stride in (1, 2):
        seeds = rng.integers(1, 1 << 63, C * key_stride, dtype=np.uint64)
        rows = []
        for c in range(C):
            part = ids[seg[c]:seg[c + 1]]
            key = int(seeds[c * key_stride])
            tr = su.oracle_traces(g.indptr, g.indices, part, n_hops, np.float32(alpha), seed=key, offset=offset)
            rows_c = su.oracle_runs(tr, part)
            if len(part):  # the per-call launch gives the same runs
                rc, r1, n1, e1 = walk_runs(g, part, n_hops, alpha, seed=key, offset=offset, src_base=0)
                assert rc == 0 and e1 == su.ERR_UNSET
                su.check_runs(f"walk_runs call {c}", r1, n1, rows_c, n_hops)
            rows += rows_c
        for cap in (total, total + 100):
            for dtype, id_unit in ((np.int64, 0), (np.int64, g.n_all), (np.int32, g.n_all), (np.int32, 1 << 20)):
                src = np.full(cap, 3, np.int64)  # slots past seg[C]: valid ids, never read
                src[:total] = ids + call * id_unit
                rc, runs, n_runs, err = _walk_runs_seg(g, src, dtype, cap, seg, seeds, key_stride, id_unit, n_hops,
                                                       alpha, offset)
                what = f"walk_runs_seg sizes={sizes} cap={cap} {np.dtype(dtype).name} id_unit={id_unit} stride={key_stride}"
                assert rc == 0 and err == su.ERR_UNSET, (what, rc, err)
                su.check_runs(what, runs, n_runs, rows, n_hops)
