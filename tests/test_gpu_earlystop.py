"""The early-stop sampler on the device (csrc/ppr_topk.hip: walk_runs_stop_kernel,
walk_runs_stop_mt_kernel, heap_topk_kernel with a per-source divisor) through
pinsage_ppr_topk_early_stop, pinsage_model and torch.ops.pinsage.

References: the reference's own fixtures (tests/golden/earlystop_*.npz) in
MT19937 mode, tests/earlystop_util.py's numpy restatement (checked against
those fixtures by tests/test_earlystop_host.py) everywhere else.  Every output
buffer is pre-filled with sentinels and every comparison is exact
(sampler_util.check_exact)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

import earlystop_util as eu
import sampler_util as su

pytestmark = pytest.mark.gpu

ALPHA = 0.85


# ----------------------------------------------------------------------------- device plumbing
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sent(shape, dtype):
    return _dev(su.sentinel_array(shape, dtype))


class _Graph:
    def __init__(self, indptr, indices, n_all):
        self.indptr, self.indices, self.n_all = np.asarray(indptr, np.int64), np.asarray(indices, np.int32), n_all
        self.d_indptr, self.d_indices = _dev(self.indptr), _dev(self.indices)


def early_stop(g, n_items, sources, n_hops, alpha, k, stop_np, stop_nv, t_norm=0, mt=None, seed=0, offset=0,
               src_base=0, cap=None, ws_bytes=None):
    """pinsage_ppr_topk_early_stop over sentinel-filled outputs of `cap` rows ->
    (rc, dict of numpy outputs, words consumed)"""
    import _native as nat
    L = nat.lib()
    n = len(sources)
    cap = n if cap is None else cap
    src = _dev(np.asarray(sources, np.int64))
    w, nb = _sent((cap, k), np.float64), _sent((cap, k), np.int64)
    wn = _sent((cap, t_norm), np.float32) if t_norm else None
    nb32 = _sent((cap, t_norm), np.int32) if t_norm else None
    hops = _sent((cap,), np.int32)
    if ws_bytes is None:
        ws_bytes = L.pinsage_ppr_topk_early_stop_workspace(n, n_hops, 1 if mt is not None else 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    words = ctypes.c_int64(-1)
    rc = L.pinsage_ppr_topk_early_stop(
        nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, n_items, nat.ptr(src), n, n_hops,
        float(np.float32(alpha)), k, stop_np, stop_nv, mt.p if mt is not None else None, seed, offset, src_base,
        nat.ptr(ws), ws_bytes, nat.ptr(w), nat.ptr(nb), nat.ptr(wn), nat.ptr(nb32), t_norm, nat.ptr(hops),
        ctypes.cast(ctypes.byref(words), ctypes.c_void_p), nat.stream_ptr())
    torch.cuda.synchronize()
    out = dict(w=w.cpu().numpy(), nb=nb.cpu().numpy(), wn=None if wn is None else wn.cpu().numpy(),
               nb32=None if nb32 is None else nb32.cpu().numpy(), hops=hops.cpu().numpy())
    return rc, out, words.value


def check_against(name, got, ref, live, cap):
    """the four top-k outputs and hops against the restatement's rows, sentinels
    from row `live` on"""
    want = su.expected_topk((ref["w"], ref["nb"], ref["wn"], ref["nb32"]), live, cap)
    su.check_topk(name, (got["w"], got["nb"], got["wn"], got["nb32"]), want)
    hops = su.sentinel_array((cap,), np.int32)
    hops[:live] = ref["hops"][:live]
    su.check_exact(name + " hops", got["hops"].reshape(cap, 1), hops.reshape(cap, 1))


_FIX = {}


def _fixture(gname):
    """(fixture dict, _Graph, graph.CSRGraph) of tests/golden/earlystop_<gname>.npz"""
    if gname not in _FIX:
        import graph
        d = golden("earlystop_" + gname)
        n_all = len(d["indptr"]) - 1
        _FIX[gname] = (d, _Graph(d["indptr"], d["indices"], n_all), graph.CSRGraph.from_csr(d["indptr"], d["indices"]))
    return _FIX[gname]


_PHILOX_REF = {}


def _philox_ref(gname, c, seed, t_norm):
    """the restatement of configuration c on Philox draws (computed once)"""
    key = (gname, c, seed, t_norm)
    if key not in _PHILOX_REF:
        d, g, _ = _fixture(gname)
        n_hops, T, stop_np, stop_nv = d["configs"][c].tolist()
        _PHILOX_REF[key] = eu.reference(g.indptr, g.indices, int(d["n_tracks"]), d["nodeset"], n_hops, ALPHA, T,
                                        stop_np, stop_nv, t_norm=t_norm, seed=seed, offset=0, src_base=5)
    return _PHILOX_REF[key]


def _next_draws(n=4):
    return np.array([int(torch.randint(2 ** 31, ())) for _ in range(n)], np.int64)


# ----------------------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize("gname", ["small", "mid"])
def test_public_function_matches_reference_fixture(gname):
    """sample_neighborhood_topt_early_stop in the default mt19937 mode: the
    reference's values, indices and generator state, in every configuration."""
    import pinsage_model as pm
    d, _, cg = _fixture(gname)
    assert pm.get_rng_mode() == "mt19937"
    nodeset = torch.from_numpy(d["nodeset"])
    for c, (n_hops, T, stop_np, stop_nv) in enumerate(d["configs"].tolist()):
        what = f"{gname} {n_hops, T, stop_np, stop_nv}"
        torch.manual_seed(int(d["seed"]))
        tk = pm.sample_neighborhood_topt_early_stop(cg, int(d["n_tracks"]), nodeset, n_hops, float(d["alpha"]), T,
                                                    stop_np, stop_nv)
        after = _next_draws()
        assert isinstance(tk, torch.return_types.topk) and tk.values.device == nodeset.device
        su.check_exact(what + " values", tk.values.numpy(), d[f"c{c}_val"])
        su.check_exact(what + " indices", tk.indices.numpy(), d[f"c{c}_idx"])
        su.check_exact(what + " next draws", after.reshape(1, -1), d[f"c{c}_after"].reshape(1, -1))


@pytest.mark.parametrize("gname", ["small", "mid"])
def test_mt_hops_and_rounds_match_fixture(gname):
    """the C-ABI in MT19937 mode: hops and the words consumed, also when the
    workspace holds 7 sources a round (each round starts where the last ended)"""
    import _native as nat
    d, g, _ = _fixture(gname)
    L = nat.lib()
    n = len(d["nodeset"])
    for c, (n_hops, T, stop_np, stop_nv) in enumerate(d["configs"].tolist()):
        if (n_hops, stop_np, stop_nv) not in ((500, 3, 10), (130, 2, 3), (65, 1, 2)):
            continue
        for per_round in (n, 7):
            what = f"{gname} {n_hops, T, stop_np, stop_nv} {per_round} a round"
            torch.manual_seed(int(d["seed"]))
            mt = nat.MT.from_torch()
            ws_bytes = L.pinsage_ppr_topk_early_stop_workspace(per_round, n_hops, 1)
            rc, out, words = early_stop(g, int(d["n_tracks"]), d["nodeset"], n_hops, float(d["alpha"]), T, stop_np,
                                        stop_nv, mt=mt, ws_bytes=ws_bytes)
            assert rc == 0, (what, rc)
            su.check_exact(what + " w", out["w"], d[f"c{c}_val"])
            su.check_exact(what + " nb", out["nb"], d[f"c{c}_idx"])
            su.check_exact(what + " hops", out["hops"].reshape(n, 1), d[f"c{c}_hops"].reshape(n, 1))
            stopped_guess = 3 * d[f"c{c}_hops"].astype(np.int64)   # 3 L - 1 or 3 n_hops per source
            assert stopped_guess.sum() - n <= words <= stopped_guess.sum(), (what, words)
            mt.to_torch()
            su.check_exact(what + " next draws", _next_draws().reshape(1, -1), d[f"c{c}_after"].reshape(1, -1))


# ----------------------------------------------------------------------------- Philox against the restatement
@pytest.mark.parametrize("gname", ["small", "mid"])
def test_philox_matches_restatement(gname):
    """w, nb, wn, nb32 and hops in every configuration; unwritten rows and rows
    past the live sources show as sentinels; two calls with src_base give the
    rows of one"""
    d, g, _ = _fixture(gname)
    n = len(d["nodeset"])
    n_items = int(d["n_tracks"])
    for c, (n_hops, T, stop_np, stop_nv) in enumerate(d["configs"].tolist()):
        what = f"{gname} {n_hops, T, stop_np, stop_nv}"
        seed = 0x9E3779B97F4A7C15 ^ (c << 20)
        t_norm = min(T, 3)
        ref = _philox_ref(gname, c, seed, t_norm)
        rc, out, words = early_stop(g, n_items, d["nodeset"], n_hops, ALPHA, T, stop_np, stop_nv, t_norm=t_norm,
                                    seed=seed, src_base=5, cap=n + 3)
        assert rc == 0 and words == 0, (what, rc, words)
        check_against(what, out, ref, n, n + 3)
        if c % 3 == 0:
            cut = 9
            for lo, hi in ((0, cut), (cut, n)):
                rc, part, _ = early_stop(g, n_items, d["nodeset"][lo:hi], n_hops, ALPHA, T, stop_np, stop_nv,
                                         t_norm=t_norm, seed=seed, src_base=5 + lo)
                assert rc == 0, (what, rc)
                sub = {k: (None if v is None else v[lo:hi]) for k, v in ref.items() if k in out}
                check_against(f"{what} sources {lo}..{hi}", part, sub, hi - lo, hi - lo)


# ----------------------------------------------------------------------------- the stop hop at every boundary
_LONER = {}


def _loner():
    if not _LONER:
        indptr, indices, n_all, special = su.bipartite_graph()
        _LONER["g"] = (_Graph(indptr, indices, n_all), special["loner"])
    return _LONER["g"]


LONER_CASES = [(n_hops, nv) for n_hops in (1, 63, 64, 65, 130)
               for nv in sorted({1, 63, 64, 65, n_hops, n_hops + 1}) if nv <= n_hops + 1]


@pytest.mark.parametrize("mode", ["philox", "mt19937"])
def test_stop_hop_at_round_boundaries(mode):
    """every hop from `loner` returns to it, so hop nv - 1 is the only event:
    with np = 1 the walk has min(nv, n_hops) hops, the weights are zeros (the
    self column) and their normalisation is 0 / 0.  MT19937: 3 nv - 1 words
    when stopped (the last-hop stop nv == n_hops included), else 3 n_hops."""
    import _native as nat
    g, loner = _loner()
    n_items, k = 300, 3
    src = np.array([loner, loner], np.int64)
    for n_hops, nv in LONER_CASES:
        what = f"{mode} n_hops {n_hops} nv {nv}"
        mt = nat.MT().seed(1000 + n_hops) if mode == "mt19937" else None
        rc, out, words = early_stop(g, n_items, src, n_hops, ALPHA, k, 1, nv, t_norm=k, mt=mt, seed=77, cap=3)
        assert rc == 0, (what, rc)
        L = min(nv, n_hops)
        assert out["hops"].tolist() == [L, L, su.SENT_I], (what, out["hops"])
        ref = dict(w=np.zeros((2, k)), nb=np.tile(np.arange(k, dtype=np.int64), (2, 1)), hops=np.array([L, L], np.int32))
        ref["wn"], ref["nb32"] = su.norm_pair(ref["w"], ref["nb"], k)
        assert np.isnan(ref["wn"]).all()
        # (zeros in libstdc++'s order: the restatement's, not assumed)
        r = eu.reference(g.indptr, g.indices, n_items, src, n_hops, ALPHA, k, 1, nv, t_norm=k, seed=77)
        assert (r["hops"] == L).all() and (r["w"] == 0).all()
        ref["nb"], ref["nb32"] = r["nb"], r["nb32"]
        check_against(what, out, ref, 2, 3)
        if mode == "mt19937":
            per = 3 * nv - 1 if nv <= n_hops else 3 * n_hops
            assert words == 2 * per, (what, words, per)
            twin = nat.MT().seed(1000 + n_hops)
            twin.skip(2 * per)
            assert (mt.draws(8) == twin.draws(8)).all(), what


@pytest.mark.parametrize("mode", ["philox", "mt19937"])
def test_several_events_in_one_round(mode):
    """two_item_graph: ids 0 and 1 only, so np = 2 stops at the second event
    (often in the first event's 64-hop round) and np = 3 never stops"""
    import _native as nat
    from oracle import oracle as orc
    indptr, indices, n_all, _ = su.two_item_graph()
    g = _Graph(indptr, indices, n_all)
    src = np.array([0, 1], np.int64)
    n_hops, n_items, k = 130, 64, 1
    same_round = 0
    for nv in (1, 2, 5):
        for stop_np in (1, 2, 3):
            what = f"{mode} np {stop_np} nv {nv}"
            if mode == "mt19937":
                mt = nat.MT().seed(40 + nv)
                r = eu.reference(indptr, indices, n_items, src, n_hops, ALPHA, k, stop_np, nv, t_norm=1,
                                 mt=orc.MT(40 + nv))
                rc, out, words = early_stop(g, n_items, src, n_hops, ALPHA, k, stop_np, nv, t_norm=1, mt=mt, cap=3)
                assert words == r["words"], (what, words, r["words"])
            else:
                r = eu.reference(indptr, indices, n_items, src, n_hops, ALPHA, k, stop_np, nv, t_norm=1, seed=123)
                rc, out, _ = early_stop(g, n_items, src, n_hops, ALPHA, k, stop_np, nv, t_norm=1, seed=123, cap=3)
            assert rc == 0, (what, rc)
            check_against(what, out, r, 2, 3)
            if stop_np == 3:
                assert not r["stopped"].any() and (r["hops"] == n_hops).all()
            else:
                assert r["stopped"].all()
            if stop_np == 2:
                one = eu.reference(indptr, indices, n_items, src, n_hops, ALPHA, k, 1, nv, seed=123)["hops"]
                if mode == "philox":
                    same_round += int(((one - 1) // 64 == (r["hops"] - 1) // 64).sum())
    assert mode != "philox" or same_round > 0


# ----------------------------------------------------------------------------- never-stop == the full sampler
@pytest.mark.parametrize("mode", ["philox", "mt19937"])
@pytest.mark.parametrize("stop", [(5, 0), (0, 5)])
def test_never_stop_equals_full_sampler(mode, stop):
    import _native as nat
    d, g, _ = _fixture("mid")
    L = nat.lib()
    n, n_hops, T = len(d["nodeset"]), 500, 10
    src = _dev(d["nodeset"])
    mt_full = nat.MT().seed(9) if mode == "mt19937" else None
    mt_stop = nat.MT().seed(9) if mode == "mt19937" else None
    w, nb = _sent((n, T), np.float64), _sent((n, T), np.int64)
    wn, nb32 = _sent((n, T), np.float32), _sent((n, T), np.int32)
    ws_bytes = L.pinsage_ppr_topk_workspace(n, n_hops, 1 if mt_full is not None else 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = L.pinsage_ppr_topk(nat.ptr(g.d_indptr), nat.ptr(g.d_indices), g.n_all, nat.ptr(src), n, n_hops,
                            float(np.float32(ALPHA)), T, mt_full.p if mt_full is not None else None, 31, 0, 2,
                            nat.ptr(ws), ws_bytes, nat.ptr(w), nat.ptr(nb), nat.ptr(wn), nat.ptr(nb32), T,
                            nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    rc, out, words = early_stop(g, g.n_all, d["nodeset"], n_hops, ALPHA, T, stop[0], stop[1], t_norm=T, mt=mt_stop,
                                seed=31, src_base=2)
    assert rc == 0
    full = dict(w=w.cpu().numpy(), nb=nb.cpu().numpy(), wn=wn.cpu().numpy(), nb32=nb32.cpu().numpy(),
                hops=np.full(n, n_hops, np.int32))
    check_against(f"{mode} never-stop {stop}", out, full, n, n)
    if mode == "mt19937":
        assert words == 3 * n_hops * n
        assert (mt_full.draws(8) == mt_stop.draws(8)).all()


# ----------------------------------------------------------------------------- error paths (from the status code)
def _last_error():
    import _native as nat
    return nat.lib().pinsage_last_error().decode()


@pytest.mark.parametrize("mode", ["philox", "mt19937"])
def test_zero_degree_is_the_graph_error(mode):
    import _native as nat
    for name, indptr, indices, n_all, sources, bad in su.zero_degree_graphs():
        g = _Graph(indptr, indices, n_all)
        for stop in ((0, 0), (2, 3)):
            mt = nat.MT().seed(3) if mode == "mt19937" else None
            rc, _, _ = early_stop(g, 64, sources, 65, ALPHA, 1, stop[0], stop[1], mt=mt, seed=5)
            assert rc == su.ERR_GRAPH, (name, stop, rc)
            assert f"source {min(bad)}:" in _last_error(), (name, stop, _last_error())


def _escape_graph():
    """directed: items 0..63, playlists 64 / 66 / 67, and 65, an id past n_items
    = 64.  0 -> 64 -> 65 (hop 0 leaves the row); 2 -> 66 -> 3 -> 67 -> 65 (hop
    1 does, without restarts); the other items -> 66 -> 3."""
    adj = {i: [66] for i in range(64)}
    adj.update({0: [64], 3: [67], 64: [65], 65: [64], 66: [3], 67: [65]})
    indptr = np.zeros(69, np.int64)
    indptr[1:] = np.cumsum([len(adj[i]) for i in range(68)])
    return _Graph(indptr, np.array([v for i in range(68) for v in adj[i]], np.int32), 68)


def test_id_past_n_items_is_the_graph_error_only_among_the_hops_taken():
    g = _escape_graph()
    # source 5 stops after hop 0 (at 3); source 0's hop 0 is the id 65
    rc, _, _ = early_stop(g, 64, np.array([5, 0], np.int64), 65, ALPHA, 1, 1, 1, seed=1)
    assert rc == su.ERR_GRAPH and "source 1:" in _last_error(), (rc, _last_error())
    # alpha = 0: hop 0 visits 3, hop 1 the id 65.  (1, 1) stops after hop 0, as
    # the reference's break does, and never sees it; (1, 2) walks on and does
    rc, out, _ = early_stop(g, 64, np.array([2], np.int64), 65, 0.0, 1, 1, 1, t_norm=1, seed=1)
    assert rc == 0, (rc, _last_error())
    assert out["hops"].tolist() == [1] and out["nb"].tolist() == [[3]] and out["w"].tolist() == [[1.0]]
    rc, _, _ = early_stop(g, 64, np.array([2], np.int64), 65, 0.0, 1, 1, 2, seed=1)
    assert rc == su.ERR_GRAPH and "source 0:" in _last_error(), (rc, _last_error())


def test_nth_element_regime_is_refused():
    import pinsage_model as pm
    d, g, cg = _fixture("small")
    n_items = int(d["n_tracks"])            # 300: k = 5 needs 320 columns
    rc, out, _ = early_stop(g, n_items, d["nodeset"][:2], 64, ALPHA, 5, 1, 2, seed=1)
    assert rc == su.ERR_ARG and "nth_element" in _last_error()
    assert (out["hops"] == su.SENT_I).all()
    with pytest.raises(NotImplementedError, match="nth_element"):
        pm.sample_neighborhood_topt_early_stop(cg, n_items, torch.from_numpy(d["nodeset"][:2]), 64, ALPHA, 5, 1, 2)
    rc, _, _ = early_stop(g, n_items, d["nodeset"][:2], 2049, ALPHA, 3, 1, 2, seed=1)
    assert rc == su.ERR_ARG


# ----------------------------------------------------------------------------- Python keywords, torch operator
def test_relevant_nodes_per_layer_early_stop():
    """two layers on `small` in the default mt19937 mode against the
    restatement, layer by layer, and the generator afterwards"""
    import pinsage_model as pm
    from oracle import oracle as orc
    d, g, cg = _fixture("small")
    n_items, n_hops, T, stop = int(d["n_tracks"]), 130, 3, (2, 3)
    nodeset = d["nodeset"][:6]
    torch.manual_seed(17)
    S = pm.relevant_nodes_per_layer(cg, n_items, torch.from_numpy(nodeset), 2, n_hops, ALPHA, T, early_stop=stop)
    after = _next_draws()
    torch.manual_seed(17)
    mt = orc.MT.from_torch()
    cur = nodeset
    assert len(S) == 2
    stopped = 0
    for layer in (1, 0):
        r = eu.reference(g.indptr, g.indices, n_items, cur, n_hops, ALPHA, T, stop[0], stop[1], mt=mt)
        stopped += int(r["stopped"].sum())
        ns, w, nb = S[layer]
        su.check_exact(f"layer {layer} nodeset", ns.numpy().reshape(-1, 1), cur.reshape(-1, 1))
        su.check_exact(f"layer {layer} w", w.numpy(), r["w"])
        su.check_exact(f"layer {layer} nb", nb.numpy(), r["nb"])
        cur = np.unique(np.concatenate([r["nb"].reshape(-1), cur]))
    assert stopped > 0
    mt.to_torch()
    su.check_exact("next draws", after.reshape(1, -1), _next_draws().reshape(1, -1))


def test_precompute_device_table_early_stop():
    """Philox mode: the table's rows are the restatement's at absolute source
    positions, whatever the chunking; MT19937 mode refuses"""
    import _native as nat
    import pinsage_model as pm
    d, g, cg = _fixture("small")
    n_items, n_hops, T, T_precomp, stop = int(d["n_tracks"]), 130, 3, 4, (2, 3)
    with pytest.raises(ValueError, match="philox"):
        pm.precompute_device_table(cg, n_items, n_hops, ALPHA, T, T_precomp, early_stop=stop)
    torch.manual_seed(23)
    with nat.torch_rng() as mt:
        dr = mt.draws(2)
    seed = (int(dr[0]) << 32) | int(dr[1])
    pm.set_rng_mode("philox")
    try:
        torch.manual_seed(23)
        tab = pm.precompute_device_table(cg, n_items, n_hops, ALPHA, T, T_precomp, chunk=128, early_stop=stop)
    finally:
        pm.set_rng_mode("mt19937")
    r = eu.reference(g.indptr, g.indices, n_items, np.arange(n_items), n_hops, ALPHA, T_precomp, stop[0], stop[1],
                     t_norm=T, seed=seed)
    assert 0 < r["stopped"].sum()
    su.check_exact("table nb32", tab.nb32.cpu().numpy(), r["nb32"])
    su.check_exact("table wn", tab.wn.cpu().numpy(), r["wn"])


def test_torch_op_equals_ctypes_path():
    import pinsage_ops
    pinsage_ops.load()
    d, g, _ = _fixture("mid")
    n_items = int(d["n_tracks"])
    n_hops, T, stop_np, stop_nv = 500, 10, 3, 5
    rc, out, _ = early_stop(g, n_items, d["nodeset"], n_hops, ALPHA, T, stop_np, stop_nv, seed=99, offset=4, src_base=2)
    assert rc == 0
    w, nb, hops = torch.ops.pinsage.ppr_topk_early_stop(g.d_indptr, g.d_indices, _dev(d["nodeset"]), n_items, n_hops,
                                                        ALPHA, T, stop_np, stop_nv, 99, 2, 4, "philox")
    su.check_exact("op w", w.cpu().numpy(), out["w"])
    su.check_exact("op nb", nb.cpu().numpy(), out["nb"])
    su.check_exact("op hops", hops.cpu().numpy().reshape(-1, 1), out["hops"].reshape(-1, 1))
    assert hops.dtype == torch.int32 and (out["hops"] < n_hops).any()
