"""CPU-side checks of the product: the C-ABI library loads and exports what
include/pinsage_hip.h declares, host RNG / batch sampling reproduce torch and
the reference draw for draw, the JSON loader and CSR graph match the reference,
and compute entry points fail loudly without a GPU (no CPU fallback)."""
import os
import re
import shutil
import tempfile

import numpy as np
import pytest
import torch

from conftest import REPO, golden


def _header_functions():
    txt = open(os.path.join(REPO, "include", "pinsage_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pinsage_\w+)\s*\(", txt)))


def test_library_exports_every_header_symbol():
    import _native
    L = _native.lib()
    names = _header_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), n
    # the ctypes binding covers exactly the header
    assert sorted(_native.EXPORTED) == names


def test_library_loads_without_gpu():
    import _native
    assert _native.lib().pinsage_version() >= 100
    assert _native.lib().pinsage_device_count() >= 0


def test_native_mt_matches_torch_and_skip():
    import _native as nat
    torch.manual_seed(77)
    mt = nat.MT.from_torch()
    ref = [int(torch.randint(1000, ())) for _ in range(3000)]
    assert (mt.draws(3000) % 1000).tolist() == ref
    # skip == draw-and-discard, across twist boundaries
    for n in (0, 1, 623, 624, 625, 1247, 5000):
        a = nat.MT().seed(5)
        b = nat.MT().seed(5)
        a.draws(n)
        b.skip(n)
        assert (a.draws(700) == b.draws(700)).all(), n


def test_native_mt_state_roundtrip():
    import _native as nat
    torch.manual_seed(3)
    with nat.torch_rng() as mt:
        mt.draws(1234)
    x = int(torch.randint(1000, ()))
    torch.manual_seed(3)
    for _ in range(1234):
        torch.randint(1000, ())
    assert int(torch.randint(1000, ())) == x


@pytest.mark.parametrize("n,k", [(1, 1), (2, 2), (37, 37), (5000, 17), (100000, 512), (300, 0)])
def test_randperm_prefix_matches_torch(n, k):
    import _native as nat
    torch.manual_seed(n + k)
    with nat.torch_rng() as mt:
        got = mt.randperm_prefix(n, k)
    after = int(torch.randint(1000, ()))
    torch.manual_seed(n + k)
    ref = torch.randperm(n)[:k].numpy()
    assert (got == ref).all()
    assert int(torch.randint(1000, ())) == after


def test_sample_batch_matches_golden():
    import pinsage_training as pt
    d = golden("batch")
    pos = torch.from_numpy(d["positives"])
    all_ids = torch.arange(int(d["n_items"]))
    torch.manual_seed(5)
    for i in range(3):
        b, ns = pt.sample_batch(all_ids, pos, int(d[f"b{i}_bs"]), None, hard_negatives=False)
        assert (b.numpy() == d[f"b{i}_batch"]).all()
        assert (ns.numpy() == d[f"b{i}_nodeset"]).all()
    got = np.array([int(torch.randint(2 ** 31, ())) for _ in range(len(d["after"]))])
    assert (got == d["after"]).all()


def test_sample_batch_component_functions_match_torch():
    import pinsage_training as pt
    d = golden("batch")
    pos = torch.from_numpy(d["positives"])
    all_ids = torch.arange(int(d["n_items"]))
    torch.manual_seed(8)
    pb = pt.sample_positives_with_rep(pos, 64)
    b, ns = pt.sample_easy_negatives(all_ids, pb)
    torch.manual_seed(8)
    b2, ns2 = pt.sample_batch(all_ids, pos, 64, None, hard_negatives=False)
    assert torch.equal(b, b2) and torch.equal(ns, ns2)


def test_max_margin_loss_matches_golden():
    import pinsage_training as pt
    d = golden("loss")
    for i in range(3):
        hq, hp, hn = (torch.from_numpy(d[f"c{i}_{k}"]).requires_grad_() for k in ("hq", "hp", "hn"))
        loss = pt.max_margin_loss(hq, hp, hn, float(d[f"c{i}_margin"]))
        loss.backward()
        assert abs(loss.item() - float(d[f"c{i}_loss"])) <= 1e-6 * max(1.0, abs(float(d[f"c{i}_loss"])))
        np.testing.assert_allclose(hq.grad.numpy(), d[f"c{i}_gq"], rtol=1e-5, atol=1e-7)


def test_spotify_graph_matches_reference_loader():
    import spotify_graph
    import synthetic
    d = golden("dataset")
    ids = [str(x) for x in d["track_ids"]]
    pg = synthetic.make_playlist_graph(len(ids), int(d["n_cols"]), 9000, seed=int(d["graph_seed"]))
    tmp = tempfile.mkdtemp()
    try:
        ds_dir = os.path.join(tmp, "ds")
        synthetic.write_spotify_dataset(ds_dir, pg, track_ids=ids, seed=int(d["json_seed"]))
        fdir = os.path.join(ds_dir, "features_test")
        os.makedirs(fdir)
        raw = np.random.default_rng(int(d["feat_seed"])).standard_normal((len(ids), 8)).astype(np.float32) * 3 + 1
        for i, tid in enumerate(ids):
            torch.save(torch.from_numpy(raw[i].copy()), os.path.join(fdir, tid + ".pt"))
        # positives of the real dataset_micro ids, re-serialised from the fixture pairs
        import json
        pairs = [{"a": ids[a], "b": ids[b]} for a, b in d["positives"]]
        with open(os.path.join(ds_dir, "positives.json"), "w") as f:
            json.dump(pairs, f)
        ds = spotify_graph.SpotifyGraph(ds_dir, fdir)
        g, track_ids, col_ids, features = ds.to_dgl_graph()
        assert track_ids == ids and col_ids == [str(x) for x in d["col_ids"]]
        src, dst = g.edges()
        assert (src.numpy() == d["src"]).all() and (dst.numpy() == d["dst"]).all()
        assert (g.successors(69).numpy() == d["succ69"]).all()
        np.testing.assert_allclose(features.numpy(), d["features"], rtol=1e-6, atol=1e-6)
        torch.manual_seed(3)
        positives = ds.load_positives(os.path.join(ds_dir, "positives.json"))
        assert (positives.numpy() == d["positives"]).all()
        got = np.array([int(torch.randint(2 ** 31, ())) for _ in range(len(d["after"]))])
        assert (got == d["after"]).all()
        tr, te = ds.load_positives_split(os.path.join(ds_dir, "positives.json"))
        assert (tr.numpy() == d["split_train"]).all() and (te.numpy() == d["split_test"]).all()
    finally:
        shutil.rmtree(tmp)


def test_spotify_graph_binary_cache(monkeypatch):
    """Second load reads pinsage_cache/ (no graph.json parse, no per-track
    feature files) and returns the same graph, edge order and features; a
    changed graph.json invalidates the cache."""
    import json
    import spotify_graph
    import synthetic
    pg = synthetic.make_playlist_graph(500, 80, 3000, seed=4)
    ids = [f"t{i:05d}" for i in range(500)]
    tmp = tempfile.mkdtemp()
    try:
        ds_dir = os.path.join(tmp, "ds")
        synthetic.write_spotify_dataset(ds_dir, pg, track_ids=ids, seed=5)
        fdir = os.path.join(ds_dir, "features")
        os.makedirs(fdir)
        raw = np.random.default_rng(1).standard_normal((500, 6)).astype(np.float32)
        for i, tid in enumerate(ids):
            torch.save(torch.from_numpy(raw[i].copy()), os.path.join(fdir, tid + ".pt"))
        g1, t1, c1, f1 = spotify_graph.SpotifyGraph(ds_dir, fdir).to_dgl_graph()
        assert os.path.isfile(os.path.join(ds_dir, "pinsage_cache", "graph.npz"))
        assert os.path.isfile(os.path.join(ds_dir, "pinsage_cache", "features.npz"))
        parsed = []
        real_load = json.load

        def spy(f, *a, **k):
            parsed.append(os.path.basename(f.name))
            return real_load(f, *a, **k)

        monkeypatch.setattr(spotify_graph.json, "load", spy)
        monkeypatch.setattr(spotify_graph.torch, "load", None)  # per-track features unused
        g2, t2, c2, f2 = spotify_graph.SpotifyGraph(ds_dir, fdir).to_dgl_graph()
        assert "graph.json" not in parsed
        assert t2 == t1 and c2 == c1 and torch.equal(f1, f2)
        assert np.array_equal(g1.indptr, g2.indptr) and np.array_equal(g1.indices, g2.indices)
        for a, b in zip(g1.edges(), g2.edges()):
            assert torch.equal(a, b)
        # a changed graph.json (one edge dropped) is parsed again
        with open(os.path.join(ds_dir, "graph.json")) as f:
            gj = real_load(f)
        gj["edges"] = gj["edges"][:-1]
        with open(os.path.join(ds_dir, "graph.json"), "w") as f:
            json.dump(gj, f)
        parsed.clear()
        g3, *_ = spotify_graph.SpotifyGraph(ds_dir, fdir).to_dgl_graph()
        assert "graph.json" in parsed and g3.number_of_edges() == g1.number_of_edges() - 1
    finally:
        shutil.rmtree(tmp)


def test_csr_graph_api():
    import graph
    src = [5, 0, 0, 3, 5, 1, 0]
    dst = [1, 4, 2, 0, 0, 0, 1]
    g = graph.CSRGraph(6, src, dst)
    assert g.number_of_nodes() == 6 and g.num_edges() == 7 and len(g) == 6
    assert g.successors(0).tolist() == [4, 2, 1]      # edge-insertion order
    assert g.successors(5).tolist() == [1, 0]
    assert g.predecessors(0).tolist() == [3, 5, 1]
    assert g.in_degrees(0) == 3 and g.in_degrees().tolist() == [3, 2, 1, 0, 1, 0]
    s, d = g.edges()
    assert sorted(zip(s.tolist(), d.tolist())) == sorted(zip(src, dst))
    a = g.adj(scipy_fmt="csr")
    assert a.shape == (6, 6) and a[0, 4] == 1 and a[4, 0] == 0
    with pytest.raises(ValueError):
        graph.CSRGraph(3, [0, 7], [1, 1])


def test_synthetic_graph_invariants():
    import synthetic
    pg = synthetic.make_playlist_graph(2000, 300, 20000, seed=4)
    indptr, indices = pg.csr()
    deg = np.diff(indptr)
    assert deg[:2000].min() >= 1 and deg[2000:].min() >= 2
    # both directions present, in JSON edge order
    src, dst = pg.edge_arrays()
    assert (src[0::2] == dst[1::2]).all() and (dst[0::2] == src[1::2]).all()
    pos = synthetic.make_positives(pg, 5000, seed=1)
    assert (pos[:, 0] != pos[:, 1]).all()
    pg2 = synthetic.make_playlist_graph(2000, 300, 20000, seed=4)
    assert (pg2.mem_track == pg.mem_track).all()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_compute_fails_loudly_without_gpu():
    import graph
    import pinsage_model as pm
    g = graph.CSRGraph(4, [0, 1, 2, 3], [2, 3, 0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pm.do_random_walks(g, torch.tensor([0]), 3, 0.85)


def test_device_table_refuses_an_id_repeated_inside_a_row():
    """The transposed aggregation's canonical sorts need a node's first T
    neighbours distinct (pinsage_engine_set_tensors): a hand-made table that
    repeats one is refused on the host, where it is bound; a repeat past column
    T is not the model's business."""
    import pinsage_model as pm
    w = torch.rand(6, 4, dtype=torch.float64) + 0.1
    nb = torch.tensor([[1, 2, 3, 4], [0, 2, 3, 5], [5, 4, 3, 1], [0, 1, 2, 4], [3, 2, 1, 0], [4, 3, 2, 1]])
    t = pm._DeviceTable((w, nb), 3, 6, "cpu")
    assert t.nb32.dtype == torch.int32 and tuple(t.nb32.shape) == (6, 3)
    nb[4, 3] = 3  # a repeat outside the first T columns
    pm._DeviceTable((w, nb), 3, 6, "cpu")
    nb[4, 2] = 3  # row 4 = 3, 2, 3, 3
    with pytest.raises(ValueError, match="repeats an id"):
        pm._DeviceTable((w, nb), 3, 6, "cpu")


def test_batch_sampler_speculation_is_exact():
    """The native sampler's speculative next batch is used only when torch's
    generator is untouched in between; batches, nodesets and the generator
    state after each call equal the synchronous reference-exact sampler's."""
    import pinsage_training as pt
    import synthetic
    pg = synthetic.make_playlist_graph(3000, 500, 20000, seed=9)
    pos = torch.from_numpy(synthetic.make_positives(pg, 8000, seed=3))
    all_ids = torch.arange(3000)

    def run(speculate):
        pt._PREFETCH.close()
        pt._PREFETCH.speculate = speculate
        pt._PREFETCH.hits = 0
        torch.manual_seed(21)
        out = []
        for i in range(12):
            b, ns = pt.sample_batch(all_ids, pos, 64 + (i >= 8) * 16, None, hard_negatives=False)
            out.append((b, ns))
            if i % 4 == 1:
                torch.randint(1000, ())   # another generator user: speculation must miss
            if i == 6:
                torch.manual_seed(5)      # a reseed as well
        out.append(int(torch.randint(2 ** 31, ())))
        return out, pt._PREFETCH.hits

    ref, h0 = run(False)
    got, h1 = run(True)
    pt._PREFETCH.close()
    pt._PREFETCH.speculate = True
    assert h0 == 0 and h1 >= 4
    assert ref[-1] == got[-1]
    for (b1, n1), (b2, n2) in zip(ref[:-1], got[:-1]):
        assert torch.equal(b1, b2) and torch.equal(n1, n2)
        assert torch.equal(n2, b2.flatten().unique())


def test_batch_sampler_peek_is_the_next_batch():
    """peek() (the trainer computes that batch's frontier ahead) returns the
    batch the next sample() draws, and None once another generator user has
    moved torch's state; the chained speculation keeps hitting."""
    import pinsage_training as pt
    import synthetic
    pg = synthetic.make_playlist_graph(3000, 500, 20000, seed=9)
    pos = torch.from_numpy(synthetic.make_positives(pg, 8000, seed=3))
    all_ids = torch.arange(3000)
    pt._PREFETCH.close()
    pt._PREFETCH.speculate = True
    pt._PREFETCH.hits = 0
    torch.manual_seed(3)
    pt.sample_batch(all_ids, pos, 64, None, hard_negatives=False)
    for _ in range(6):
        nxt = pt._PREFETCH.peek(64)
        b, _ = pt.sample_batch(all_ids, pos, 64, None, hard_negatives=False)
        assert nxt is not None and np.array_equal(nxt, b.numpy())
    assert pt._PREFETCH.hits >= 5
    torch.randint(10, ())
    assert pt._PREFETCH.peek(64) is None
    assert pt._PREFETCH.peek(32) is None
    pt._PREFETCH.close()


@pytest.mark.parametrize("n", [(1 << 21) + 7, 3_000_017, 12_345_678])
def test_mt_long_skip_jumps_exactly(n):
    """Skips of >= 2^21 draws use the GF(2) jump-ahead (mt_jump.h); the state
    must equal n sequential draws, from any position inside a block."""
    import _native as nat
    for pre in (0, 1, 311, 623, 624, 1000):
        a = nat.MT().seed(1234 + pre)
        b = nat.MT().seed(1234 + pre)
        a.draws(pre)
        b.draws(pre)
        a.skip(n)
        # reference: sequential twisting in bounded pieces (below the jump threshold)
        left = n
        while left:
            k = min(left, (1 << 21) - 1)
            b.skip(k)
            left -= k
        assert (a.draws(2000) == b.draws(2000)).all(), (n, pre)


def test_randperm_prefix_long_matches_torch():
    """torch.randperm(5M)[:512] and the generator state after it (jump path)."""
    import _native as nat
    n, k = 5_000_000, 512
    torch.manual_seed(99)
    with nat.torch_rng() as mt:
        got = mt.randperm_prefix(n, k)
    after = int(torch.randint(1000, ()))
    torch.manual_seed(99)
    ref = torch.randperm(n)[:k].numpy()
    assert (got == ref).all()
    assert int(torch.randint(1000, ())) == after


def test_device_graph_generator_properties():
    """synthetic.make_playlist_graph_device (the C5 bench's graph builder) on the
    CPU device: bipartite and symmetric, rows in edge-insertion order, every
    track in >= 1 collection and every collection with >= 2 distinct tracks;
    positives are co-members and never self-pairs."""
    import numpy as np
    import torch
    import synthetic
    n, nc = 3000, 700
    ip, ix = synthetic.make_playlist_graph_device(n, nc, 30000, seed=1, device="cpu")
    ip, ix = ip.numpy(), ix.numpy()
    deg = np.diff(ip)
    assert deg[:n].min() >= 1 and deg[n:].min() >= 2
    src = np.repeat(np.arange(n + nc), deg)
    assert ((src < n) != (ix < n)).all()
    fwd = set(zip(src.tolist(), ix.tolist()))
    assert fwd == set(zip(ix.tolist(), src.tolist())) and len(fwd) == ix.shape[0]
    for v in list(range(0, n, 97)) + list(range(n, n + nc, 13)):
        row = ix[ip[v]:ip[v + 1]]
        assert (np.diff(row) > 0).all()  # collection-major pairs: both row kinds ascend
    pos = synthetic.make_positives_device(torch.from_numpy(ip), torch.from_numpy(ix), n, 4000, seed=3).numpy()
    assert (pos[:, 0] != pos[:, 1]).all() and pos.max() < n
    cols_of = {v: set(ix[ip[v]:ip[v + 1]].tolist()) for v in np.unique(pos[:200]).tolist()}
    assert all(cols_of[a] & cols_of[b] for a, b in pos[:200].tolist())


def test_torch_operator_library_registers_every_op():
    """libpinsage_torch.so (csrc/torch_ops.cpp) loads and registers the
    torch.ops.pinsage schemas of SURVEY.md §8(b2), with autograd formulas for
    the differentiable ones; no compute (there is no CPU implementation)."""
    import torch
    import pinsage_ops
    pinsage_ops.load()
    for name in ("walk", "ppr_topk", "frontier", "gather_rows", "scatter_add_rows", "linear",
                 "concat_linear_lrelu_l2norm", "norm_lrelu_backward", "gemm", "weighted_agg",
                 "weighted_agg_backward", "segment_wmean"):
        assert hasattr(torch.ops.pinsage, name), name
    x = torch.zeros(4, 8)
    W = torch.zeros(4, 8)
    import pytest
    with pytest.raises(NotImplementedError, match="CPU"):  # HIP dispatch only: fails loudly
        torch.ops.pinsage.linear(x, None, W, None, True)


def test_frontier_plan_checker_rejects_single_defects():
    """parity_util.check_frontier_plan (the comparison behind
    tests/test_gpu_frontier_plan.py) passes a correct plan and names the layer
    and the field of each single defect."""
    import copy
    from parity_util import check_frontier_plan, frontier_plan_reference
    rng = np.random.default_rng(17)
    n, L, T = 900, 2, 3
    nb = np.argsort(rng.random((n, 40)), 1)[:, :T] * 22 + rng.integers(0, 20, (n, 1))  # distinct within a row
    wb = rng.integers(0, 1 << 32, (n, T), dtype=np.uint64).astype(np.uint32)
    assert nb.max() < n
    ids = rng.integers(0, n, 50)
    want = frontier_plan_reference(ids, lambda l, S: (nb[S], wb[S]), L, T)
    # the reference against the definitions, on this small case
    top = want["layers"][1]
    assert np.array_equal(top["S"], np.unique(ids)) and np.array_equal(top["S"][want["pos_rank"]], ids)
    assert np.array_equal(top["N"][top["loc"]], nb[top["S"]])
    assert np.array_equal(want["layers"][0]["S"][top["q_src"]], top["N"])
    assert np.array_equal(want["layers"][0]["S"][top["self_src"]], top["S"])
    assert np.array_equal(want["layers"][0]["q_src"], want["layers"][0]["N"])
    for r in range(len(top["S"])):
        p = want["pos_sorted"][want["rank_off"][r]:want["rank_off"][r + 1]]
        assert np.array_equal(p, np.flatnonzero(ids == top["S"][r]))
    check_frontier_plan(copy.deepcopy(want), want)

    def defect(change, match):
        got = copy.deepcopy(want)
        change(got)
        with pytest.raises(AssertionError, match=match):
            check_frontier_plan(got, want)

    def off_by_one(p):
        p["layers"][1]["loc"][7, 1] += 1

    def swapped(p):
        S = p["layers"][0]["S"]
        S[[4, 5]] = S[[5, 4]]

    def missing(p):
        lay = p["layers"][0]
        lay["N"] = np.delete(lay["N"], 11)
        lay["count_N"] -= 1

    def shifted(p):
        p["rank_off"][9] += 1

    def one_bit(p):
        p["layers"][0]["wloc"][20, 2] ^= np.uint32(1 << 22)

    def stale_read_counts(p):
        p["read_counts"] = (p["read_counts"][0], [p["read_counts"][1][0], p["read_counts"][1][1] + 1])

    defect(off_by_one, r"^layer 1 loc: 1 of \d+ entries differ, first at \[22\]")
    defect(swapped, r"^layer 0 S: 2 of \d+ entries differ, first at \[4\]")
    defect(missing, r"^layer 0 count_N: 1 of 1 entries differ")
    defect(shifted, r"^positions rank_off: 1 of \d+ entries differ, first at \[9\]")
    defect(one_bit, r"^layer 0 wloc: 1 of \d+ entries differ, first at \[62\]")
    defect(stale_read_counts, r"^all layers read_counts N: ")
    # more than 16384 positions: the position CSR is absent, only its mark is compared
    many = rng.integers(0, n, 16385)
    absent = frontier_plan_reference(many, lambda l, S: (nb[S], wb[S]), L, T)
    assert absent["rank_off"].tolist() == [-1]
    got = copy.deepcopy(absent)
    got["rank_off"] = np.array([-1, 123, 456])
    check_frontier_plan(got, absent)
    got["rank_off"] = np.array([0, 123, 456])
    with pytest.raises(AssertionError, match="^positions rank_off"):
        check_frontier_plan(got, absent)


def test_knn_select_cases_reach_their_regimes_and_checker_rejects_defects():
    """Every case of tests/test_gpu_knn_select.py, on the host: the table meets
    the exact reference's premise and the replay of knn_select_kernel's decision
    (parity_util.knn_select_regime) takes the exit the case was built for; all
    four exits are reached.  Then parity_util.check_knn_select passes a correct
    answer and names each single defect of one."""
    import parity_util as pu
    exits = set()
    for case in pu.KNN_SELECT_CASES:
        emb, probes, q, k, sim, ref_w, ref_ids = pu.knn_select_case(case)  # asserts premise and exit
        exits.add(pu.knn_select_regime(sim[0], k))
        assert ref_w.shape == (1, k) and (np.diff(ref_w[0]) <= 0).all(), case[0]
        assert len(set(ref_ids[0].tolist())) == k, case[0]
    assert exits == {"fast", "few", "segment", "ties"}
    # what the cases say they pin, read off the reference
    _, _, _, _, sim, w, ids = pu.knn_select_case(next(c for c in pu.KNN_SELECT_CASES if c[0] == "zeroquery-k1000"))
    assert ids[0].tolist() == list(range(1000)) and not w.view(np.int32).any()   # an n-way tie at +0.0
    emb, probes, _, _, sim, w, ids = pu.knn_select_case(
        next(c for c in pu.KNN_SELECT_CASES if c[0] == "third-k1000"))
    assert ids[0, :2].tolist() == [probes["p1"], probes["p2"]]                   # both are exactly 1.0
    assert ids[0, 2:].tolist() == list(range(0, 3 * 998, 3))                      # the lowest multiples of 3
    assert int((sim[0] == w[0, -1]).sum()) > pu.KNN_MAX_SORT
    emb, probes, _, _, sim, w, ids = pu.knn_select_case(
        next(c for c in pu.KNN_SELECT_CASES if c[0] == "signs-k200"))
    assert (w[0] > 0).any() and (w[0] == 0).sum() >= 4 and (w[0] < 0).any()
    _, _, _, k, sim, _, _ = pu.knn_select_case(next(c for c in pu.KNN_SELECT_CASES if c[0] == "block-k100"))
    _, _, per_wave = pu.knn_select_candidates(sim[0], k)
    assert (per_wave > pu.KNN_SEG).sum() == 1 and per_wave[5] > pu.KNN_SEG     # columns 5120 .. 6143: wave 5
    assert per_wave.sum() < 2 * pu.KNN_SEG                                     # one full segment, not a full row
    # (2, 0, ...) gives the values of (1, 0, ...) bitwise; (-1, 0, ...) the reverse order
    emb, probes = pu.knn_select_table("desc")
    sim, w, ids = pu.knn_select_reference(emb, [probes["p1"], probes["p2"], probes["m1"]], 1000)
    assert np.array_equal(sim[0].view(np.int32), sim[1].view(np.int32))
    assert np.array_equal(sim[2], -sim[0] + np.float32(0.0))
    assert pu.knn_select_regime(sim[2], 1000) == "segment"

    # the checker: a case whose k-th value is tied (300 rows share it)
    _, _, q, k, sim, w, ids = pu.knn_select_case(
        next(c for c in pu.KNN_SELECT_CASES if c[0] == "scattered-k1000"))
    pu.check_knn_select(w.copy(), ids.copy(), w, ids)
    _, w1, ids1 = pu.knn_select_reference(pu.knn_select_table("scattered")[0], q, k + 1)
    wb = w.view(np.int32)[0]
    tie = int(np.flatnonzero(wb[1:] == wb[:-1])[0])           # columns tie, tie + 1 hold one value
    assert wb[k - 1] == w1.view(np.int32)[0, k]               # and the k-th ties with the (k+1)-th
    plain = int(np.flatnonzero(wb[1:] != wb[:-1])[5])         # columns plain, plain + 1 differ

    def defect(change, match):
        gw, gi = w.copy(), ids.copy()
        change(gw, gi)
        with pytest.raises(AssertionError, match=match):
            pu.check_knn_select(gw, gi, w, ids)

    def tie_swapped(gw, gi):
        gi[0, [tie, tie + 1]] = gi[0, [tie + 1, tie]]

    def kth_replaced(gw, gi):
        gw[0, k - 1], gi[0, k - 1] = w1[0, k], ids1[0, k]

    def one_ulp(gw, gi):
        gw.view(np.int32)[0, 17] += 1

    def columns_exchanged(gw, gi):
        gi[0, [plain, plain + 1]] = gi[0, [plain + 1, plain]]
        gw[0, [plain, plain + 1]] = gw[0, [plain + 1, plain]]

    defect(tie_swapped, rf"^knn query 0 column {tie}: 2 of {k} entries differ, first here: order swap inside a tie")
    defect(kth_replaced, rf"^knn query 0 column {k - 1}: 1 of {k} entries differ, first here: missing id")
    defect(one_ulp, rf"^knn query 0 column 17: 1 of {k} entries differ, first here: value bit")
    defect(columns_exchanged, rf"^knn query 0 column {plain}: 2 of {k} entries differ, first here: order: ")
    with pytest.raises(AssertionError, match="^knn: shapes"):
        pu.check_knn_select(w[:, :-1], ids[:, :-1], w, ids)
    # the reference refuses a table outside its premise (a dot of two terms)
    bad = np.array(pu.knn_select_table("random:65")[0])
    bad[3, 0], bad[3, 1] = 1.0, 1.0
    with pytest.raises(AssertionError):
        pu.knn_select_reference(bad, [3], 5)


def test_bench_refuses_a_world_size_other_than_gpus():
    """bench.py started by a launcher with WORLD_SIZE != --gpus exits non-zero
    before touching the GPU (launch_ranks)."""
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=3" in (r.stderr + r.stdout)


def test_bench_dump_outputs_writes_float32_within_its_budget(tmp_path):
    """bench.dump_outputs (--dump-outputs DIR): one float32 DIR/<name>.npy per
    value train_batch returned (none for a None) and per model parameter; an
    array over its share of the byte budget becomes a sample of its elements
    that is the same on every run."""
    import torch
    import bench
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3, bias=False))
    last = (torch.tensor(0.25), None, torch.tensor(1.5, dtype=torch.float64))
    bench.dump_outputs(str(tmp_path / "a"), last, model)
    got = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["loss.npy", "param.0.bias.npy", "param.0.weight.npy", "param.1.weight.npy",
                           "variance.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss.npy"].tolist() == [0.25] and got["variance.npy"].tolist() == [1.5]
    assert np.array_equal(got["param.0.weight.npy"], model[0].weight.detach().numpy())
    # 5 arrays share 200 bytes: 10 floats each, so only the 7x5 and 5x3 weights are sampled
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), last, model, budget=200)
    small = {p.name: np.load(p) for p in (tmp_path / "b").iterdir()}
    again = {p.name: np.load(p) for p in (tmp_path / "c").iterdir()}
    assert sum(a.nbytes for a in small.values()) <= 200
    assert small["param.0.weight.npy"].shape == (10,) and small["param.1.weight.npy"].shape == (10,)
    assert np.isin(small["param.0.weight.npy"], got["param.0.weight.npy"]).all()
    assert np.array_equal(small["param.0.bias.npy"], got["param.0.bias.npy"])
    assert sorted(small) == sorted(again) and all(np.array_equal(small[k], again[k]) for k in small)


# ----------------------------------------------------------------------------- loss / head references
def _loss_case_inputs(case):
    import parity_util as pu
    batch = pu.case_batch(case)
    Z = pu.case_Z(case, batch)
    S = np.unique(batch)
    pr = np.searchsorted(S, batch.reshape(-1))
    return pu, batch, Z, S, pr


def _loss_case_ids():
    import parity_util as pu
    return [pytest.param(c, id=c["name"]) for c in pu.LOSS_CASES]


@pytest.mark.parametrize("case", _loss_case_ids())
def test_loss_reference_matches_autograd(case):
    """parity_util.loss_reference against torch float64 autograd of the
    project's max_margin_loss over rows gathered per position, the oracle's
    put_embeddings (_put: index_put's backward) and the gather doing the sums
    over repeated ids: loss and dZ to 1e-12 relative."""
    import pinsage_training as pt
    from oracle import oracle as orc
    pu, batch, Z, S, pr = _loss_case_inputs(case)
    B, d = case["B"], case["out"]
    ref = pu.loss_reference(Z, pr, B, case["margin"])
    Zt = torch.tensor(Z.astype(np.float64), requires_grad=True)
    hs = []
    for c in range(3):
        idc = torch.from_numpy(np.ascontiguousarray(batch[:, c]))
        rows = Zt[torch.from_numpy(np.ascontiguousarray(pr.reshape(B, 3)[:, c]))]
        hs.append(orc._put(torch.zeros(pu.HL_N, d, dtype=torch.float64), idc, rows)[idc])
    loss = pt.max_margin_loss(*hs, case["margin"])
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    g = Zt.grad.numpy()
    assert np.linalg.norm(g - ref["dZ"]) <= 1e-12 * np.linalg.norm(ref["dZ"])
    assert np.linalg.norm(ref["dZ"]) > 0 or len(S) == 1  # (all ids equal: every cotangent is zero)


@pytest.mark.parametrize("case", _loss_case_ids())
def test_loss_cases_reach_what_they_claim(case):
    pu, batch, Z, S, pr = _loss_case_inputs(case)
    B = case["B"]
    assert batch.shape == (B, 3) and len(S) == case["S"] and Z.dtype == np.float32
    assert (3 * B > pu.POS_CSR_MAX) == (case["kind"] == "heavy")
    ref = pu.loss_reference(Z, pr, B, case["margin"])
    arg32 = pu.hinge_replay32(Z, pr, B, case["margin"])
    ties = batch[:, 1] == batch[:, 2] if case["margin"] == 0.0 else np.zeros(B, bool)
    assert (ref["arg"][ties] == 0.0).all() and (arg32[ties] == 0.0).all()
    assert np.abs(ref["arg"][~ties]).min() >= pu.ARG_MIN
    assert (np.sign(arg32[~ties]) == np.sign(ref["arg"][~ties])).all()
    if B >= 4:
        assert ref["active"].any() and not ref["active"].all()
    if case["kind"] != "hand":
        return
    _, roles = pu.hand_batch()
    mult = np.bincount(pr)
    assert sorted(mult) == sorted(pu.HAND_MULTS + (B + 2,)) and B == pu.HAND_B
    assert {1, 2, 3, 4, 5, 12, 13, 16, 17, 20, 21, 33} <= set(mult.tolist())
    assert (batch[:, 0] == roles["Q"]).all()                         # one node fills every query position
    groups = {int(v): {c for c in range(3) if (batch[:, c] == v).any()} for v in S}
    assert sorted({len(g) for g in groups.values()}) == [1, 2, 3]  # one, two and all three groups
    assert int((batch[:, 0] == batch[:, 1]).sum()) == 1              # one triple with q == p
    assert int(ties.sum()) == 3 and ref["active"][ties].all()       # p == n: hinge exactly 0, active
    xin = (batch == roles["X"]).any(1)
    assert int(xin.sum()) == 3 and not ref["active"][xin].any()      # a repeated node with inactive triples only


def test_loss_case_table_covers_the_regimes():
    import parity_util as pu
    C = pu.LOSS_CASES
    assert {c["out"] for c in C} == {4, 8, 16, 32, 64, 128}
    assert {2, 3, 4, 5, 7, 8, 9, 64, 129} <= {c["B"] for c in C}
    assert {1, 31, 32, 33, 64, 65, 200} <= {c["S"] for c in C}
    assert {4, 128, 132, 256, 260, 512, 1024, 1028} <= {c["d_in"] for c in C}
    assert any(c["d_in"] > 4 and c["B"] % 4 for c in C) and {0, 1} <= {c["mon"] for c in C}
    assert [c for c in C if 3 * c["B"] == 16386 and c["out"] == 8]
    assert len({c["name"] for c in C}) == len(C)
    # the head: rows around its 32-row (16-row in the tile) blocks, widths off the 32-lane grid
    assert {1, 31, 32, 33} <= set(pu.HEAD_SEPARATE_ROWS) and {15, 16, 17} <= set(pu.HEAD128_ROWS)
    assert any(w % 32 for w in pu.HEAD_SEPARATE_WIDTHS) and all(w % 4 == 0 and w <= 128 for w in pu.HEAD_SEPARATE_WIDTHS)
    assert all(1024 % w == 0 for w in pu.BACKWARD_WIDTHS) and any(1024 % w for w in pu.AUTOGRAD_WIDTHS)
    assert {5, 13, 17, 21} <= set(pu.AUTOGRAD_MULTS)  # head_sum_reps: 4 + 1, 4 + 8 + 1; rep_sum: 16 + 1, 16 + 5


def _synthetic_loss_outputs(pu, case, cap=40, all_active=False):
    """what a correct device would leave (float32 roundings of the reference,
    G's repeated ranks as the ordered float32 sums of the Gp rows)"""
    _, batch, Z, S, pr = _loss_case_inputs(case)
    B, R, d = case["B"], len(S), case["out"]
    feats = np.random.default_rng(0).standard_normal((pu.HL_N, 8)).astype(np.float32)
    ref = pu.loss_reference(Z, pr, B, case["margin"], feats, batch)
    src = ref
    if all_active:  # the defect: every triple treated as active
        src = pu.loss_reference(Z, pr, B, 10.0)
    Gp = src["cot"].astype(np.float32)
    G = np.zeros((3, cap, d), np.float32)
    for (c, r), row in pu.rep_sum32(Gp, pr, R).items():
        G[c, r] = row
    for r in np.flatnonzero(np.bincount(pr, minlength=R) == 1):
        p = int(np.flatnonzero(pr == r)[0])
        G[p % 3, r] = Gp[p]
    Kc = np.zeros((3, cap), np.int32)
    Kc[:, :R] = ref["K"]
    scal = np.array([ref["loss"], ref["nfl"], ref["sumsq"], ref["var"]], np.float32)
    return ref, pr, R, dict(hinge=ref["arg"].astype(np.float32), G=G, Kc=Kc, Gp=Gp, scal=scal)


def test_loss_checkers_reject_single_defects():
    import parity_util as pu
    case = next(c for c in pu.LOSS_CASES if c["name"] == "hand-o8-rs0")
    ref, pr, R, got = _synthetic_loss_outputs(pu, case)
    B, cap = case["B"], got["G"].shape[1]

    def dz_of(g):
        dz, bound = pu.dz_reference(g["G"], g["Kc"], g["Gp"], pr, R, "head")
        return dz, bound

    dz, bound = dz_of(got)
    dZ = np.zeros((cap, 8), np.float32)
    dZ[:R] = dz

    def clean():
        pu.check_loss(got, ref, "rep_sum")
        pu.check_loss(dict(got, G=_head_mode_G(got, ref, R)), ref, "head")
        pu.check_rep_sum_exact(got["G"], got["Gp"], pr, R)
        pu.check_rows("dZ", dZ, R, dz, bound)
        # the device's own sums agree with the reference's K Gsum as well
        assert np.abs(dz - ref["dZ"]).max() <= 1e-5 * np.abs(ref["dZ"]).max()

    def _head_mode_G(g, ref, R):
        G = g["G"].copy()
        G[:, :R][:, ref["K"].sum(0) > 1] = 0  # the repeated ranks stay in Gp
        return G

    clean()
    rep = int(np.flatnonzero(np.bincount(pr, minlength=R) == 13)[0])  # the 13-position rank (positives only)
    mixed = int(np.flatnonzero(np.bincount(pr, minlength=R) == 33)[0])  # positives and negatives

    # K dropped: dZ = sum_c G[c]
    bad = np.zeros_like(dZ)
    bad[:R] = pu.dz_reference(got["G"], np.minimum(got["Kc"], 1), got["Gp"], pr, R, "head")[0]
    with pytest.raises(AssertionError, match=r"^dZ: .* first at row \d+, column \d+"):
        pu.check_rows("dZ", bad, R, dz, bound)
    # the groups p % 3 swapped (positive <-> negative)
    sw = dict(got, G=got["G"][[0, 2, 1]].copy())
    with pytest.raises(AssertionError, match=r"^rep_sum: call (positive|negative), rank \d+"):
        pu.check_rep_sum_exact(sw["G"], got["Gp"], pr, R)
    with pytest.raises(AssertionError, match=r"^G: .* first at call (positive|negative), rank \d+"):
        pu.check_loss(sw, ref, "rep_sum")
    bad[:R] = (got["Kc"][:, :R, None].astype(np.float64) * got["G"][[0, 2, 1]][:, :R]).sum(0)
    with pytest.raises(AssertionError, match="^dZ: "):
        pu.check_rows("dZ", bad, R, dz, bound)
    # one position of a repeated rank skipped
    skip = got["G"].copy()
    p_skip = next(int(p) for p in np.flatnonzero(pr == rep)[4:] if ref["active"][p // 3])  # past the first four
    assert p_skip % 3 == 1
    skip[1, rep] = sum((got["Gp"][p] for p in np.flatnonzero(pr == rep) if p != p_skip), np.zeros(8, np.float32))
    with pytest.raises(AssertionError, match=rf"^rep_sum: call positive, rank {rep} \(13 positions\)"):
        pu.check_rep_sum_exact(skip, got["Gp"], pr, R)
    with pytest.raises(AssertionError, match=rf"^G: .* first at call positive, rank {rep}"):
        pu.check_loss(dict(got, G=skip), ref, "rep_sum")
    bad[:R] = (got["Kc"][:, :R, None].astype(np.float64) * skip[:, :R]).sum(0)
    with pytest.raises(AssertionError, match=rf"^dZ: .* first at row {rep}, column"):
        pu.check_rows("dZ", bad, R, dz, bound)
    # an inactive triple counted as active
    _, _, _, wrong = _synthetic_loss_outputs(pu, case, all_active=True)
    with pytest.raises(AssertionError, match=r"^(G|Gp): "):
        pu.check_loss(dict(got, G=wrong["G"], Gp=wrong["Gp"]), ref, "rep_sum")
    with pytest.raises(AssertionError, match=r"^Gp: .* first at position \d+ \(triple \d+, call \w+, rank \d+\)"):
        pu.check_loss(dict(got, G=_head_mode_G(got, ref, R), Gp=wrong["Gp"]), ref, "head")
    # an inactive triple's Gp rows left as they were (garbage), a tie's hinge not exactly zero, Kc off by one
    garbage = got["Gp"].copy()
    garbage[np.flatnonzero((pr == mixed) & ~np.repeat(ref["active"], 3))[0]] = np.nan
    with pytest.raises(AssertionError, match="^Gp: "):
        pu.check_loss(dict(got, Gp=garbage), ref, "rep_sum")
    h = got["hinge"].copy()
    h[np.flatnonzero(ref["arg"] == 0.0)[0]] = 1e-9
    with pytest.raises(AssertionError, match="^hinge of the planted ties"):
        pu.check_loss(dict(got, hinge=h), ref, "rep_sum")
    h = got["hinge"].copy()
    h[np.flatnonzero(ref["arg"] == 0.0)[0]] = -1e-9
    with pytest.raises(AssertionError, match="^hinge of the planted ties"):
        pu.check_loss(dict(got, hinge=h), ref, "rep_sum")
    k = got["Kc"].copy()
    k[2, R] = 1
    with pytest.raises(AssertionError, match=rf"^Kc: .* first at call negative, rank {R}"):
        pu.check_loss(dict(got, Kc=k), ref, "rep_sum")
    clean()
    # the variance divided by B (a batch whose query rows differ: the hand batch's variance is 0)
    case9 = next(c for c in pu.LOSS_CASES if c["name"] == "B9-S17-o4")
    ref9, _, _, got9 = _synthetic_loss_outputs(pu, case9)
    pu.check_loss(got9, ref9, "rep_sum")
    s = got9["scal"].copy()
    s[3] *= 8 / 9
    with pytest.raises(AssertionError, match=r"^scalar 3 \(variance\)"):
        pu.check_loss(dict(got9, scal=s), ref9, "rep_sum")


def test_head_checkers_reject_single_defects():
    import parity_util as pu
    rng = np.random.default_rng(5)
    R, cap, o = 33, 40, 12
    y = rng.standard_normal((R, o)).astype(np.float32)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    G1w, G2w = (rng.standard_normal((o, o)).astype(np.float32) / np.sqrt(o) for _ in range(2))
    G1b = (rng.standard_normal(o) / np.sqrt(o)).astype(np.float32)
    sent = np.uint32(0x7FC12345)

    def full(rows):
        a = np.full((cap, o), sent, np.uint32).view(np.float32)
        a[:R] = rows
        return a

    H1 = full(pu.head_reference_fwd(y, G1w, G1b, G2w, np.zeros((R, o)))["H1"].astype(np.float32))
    ref = pu.head_reference_fwd(y, G1w, G1b, G2w, H1[:R])
    Z = full(ref["Z"].astype(np.float32))
    assert pu.check_rows("H1", H1, R, ref["H1"], ref["H1_bound"], sent) <= 1.0
    assert pu.check_rows("Z", Z, R, ref["Z"], ref["Z_bound"], sent) <= 1.0
    # one row past a 32-row block left unwritten
    bad = H1.copy()
    bad[32] = np.full(o, sent, np.uint32).view(np.float32)
    with pytest.raises(AssertionError, match="^H1: 12 of 396 entries outside their bound, first at row 32, column 0"):
        pu.check_rows("H1", bad, R, ref["H1"], ref["H1_bound"], sent)
    # one column past o written: the last live row's lands past the live rows, another row's in the next row
    bad = Z.copy()
    bad.reshape(-1)[(R - 1) * o + o] = 0.0
    with pytest.raises(AssertionError, match=rf"^Z past its {R} live rows: 1 of .* first at row {R}, column 0"):
        pu.check_rows("Z", bad, R, ref["Z"], ref["Z_bound"], sent)
    bad = Z.copy()
    bad.reshape(-1)[7 * o + o] = 0.0
    with pytest.raises(AssertionError, match="^Z: 1 of 396 entries outside their bound, first at row 8, column 0"):
        pu.check_rows("Z", bad, R, ref["Z"], ref["Z_bound"], sent)
    # an error of a few units in the last place of the terms is a failure: the bound is not slack
    bad = Z.copy()
    bad[5, 3] += np.float32(4 * (o + 4) * pu.U24 * (np.abs(H1[5].astype(np.float64)) @ np.abs(G2w[3].astype(np.float64))))
    with pytest.raises(AssertionError, match="^Z: 1 of 396 entries outside their bound, first at row 5, column 3"):
        pu.check_rows("Z", bad, R, ref["Z"], ref["Z_bound"], sent)
    # the backward's reference is consistent with autograd (float64) through the same chain
    dZ = rng.standard_normal((R, o)).astype(np.float32)
    nrm = (rng.random(R) + 0.5).astype(np.float32)
    pre = torch.tensor(rng.standard_normal((R, o)), requires_grad=True)
    u = torch.nn.functional.leaky_relu(pre, 0.01)
    yt = u / u.norm(dim=1, keepdim=True)
    G1t, b1t, G2t = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (G1w, G1b, G2w))
    H1t = torch.nn.functional.leaky_relu(yt @ G1t.t() + b1t, 0.01)
    (H1t @ G2t.t() * torch.tensor(dZ.astype(np.float64))).sum().backward()
    d64 = pu.head_reference_bwd(dZ, H1t.detach().numpy(), yt.detach().numpy(), u.norm(dim=1).detach().numpy(),
                                G1w, G2w, np.zeros((R, o)))
    dP1 = d64["dP1"]
    d64 = pu.head_reference_bwd(dZ, H1t.detach().numpy(), yt.detach().numpy(), u.norm(dim=1).detach().numpy(),
                                G1w, G2w, dP1)
    for got, want in ((d64["dp"], pre.grad), (d64["dG2"], G2t.grad), (d64["dG1"], G1t.grad), (d64["db1"], b1t.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()


# ----------------------------------------------------------------------------- GEMM forms, slab reduction, Adam
# The references and checkers of tests/test_gpu_gemm_forms.py and
# tests/test_gpu_optimizer.py: pinned to an independent restatement (plain
# loops, torch.optim.Adam), and each planted defect rejected with its location.
def _form_spec(rng, epi=0, exact=True, **kw):
    import parity_util as pu
    M, N, K, K1 = 7, 12, 24, 8
    fv = lambda *sh: pu.form_values(rng, sh, exact)
    s = dict(M=M, N=N, K=K, a=fv(11, K1 + 4), a_idx=rng.permutation(11)[:M], K1=K1, a2=fv(9, K - K1 + 4),
             a2_idx=rng.permutation(9)[:M], b=fv(N, K + 4), bias=fv(N), epi=epi,
             c=fv(M + 4, N + 3) if epi == pu.EPI_ACCUM else np.full((M + 4, N + 3), np.nan, np.float32),
             c_idx=rng.permutation(M + 4)[:M])
    s.update(kw)
    return s


def test_gemm_form_reference_against_plain_loops():
    import parity_util as pu
    rng = np.random.default_rng(0)
    s = _form_spec(rng, epi=pu.EPI_ACCUM, exact=False, act=True, N1=8, c2=np.full((9, 6), np.nan, np.float32))
    ref = pu.gemm_form_reference(s)
    slope = float(np.float32(0.01))
    seen_c, seen_c2 = np.zeros(s["c"].shape, bool), np.zeros(s["c2"].shape, bool)
    for m in range(s["M"]):
        for n in range(s["N"]):
            x = float(s["bias"][n])
            for k in range(s["K"]):
                a = s["a"][s["a_idx"][m], k] if k < s["K1"] else s["a2"][s["a2_idx"][m], k - s["K1"]]
                x += float(a) * float(s["b"][n, k])
            x = x if x > 0 else slope * x
            if n < s["N1"]:
                r = s["c_idx"][m]
                assert abs(ref["c"]["want"][r, n] - (x + float(s["c"][r, n]))) < 1e-12
                seen_c[r, n] = True
            else:
                assert abs(ref["c2"]["want"][m, n - s["N1"]] - x) < 1e-12
                seen_c2[m, n - s["N1"]] = True
    assert (ref["c"]["written"] == seen_c).all() and (ref["c2"]["written"] == seen_c2).all()
    # M-major A, N-major B in two segments gathered by k, partial slabs with the column sums of A
    K, M, N, N1, S = 70, 8, 12, 4, 4
    b_idx = rng.integers(0, K + 3, K)
    p = dict(M=M, N=N, K=K, a_kmajor=False, b_kmajor=False, a=rng.standard_normal((K, M + 4)), N1=N1, b_idx=b_idx,
             b=rng.standard_normal((K + 3, N1 + 4)), b2=rng.standard_normal((K, N - N1)), epi=pu.EPI_PARTIAL, splits=S,
             c=np.full((S * M + 1, N), np.nan, np.float32), bias_part=np.full((S + 1, M), np.nan, np.float32))
    ref = pu.gemm_form_reference(p)
    for sp, (k0, k1) in enumerate(((0, 32), (32, 64), (64, 70), (70, 70))):   # ceil(70 / 4) = 18 -> chunks of 32
        for m in range(M):
            assert abs(ref["bias_part"]["want"][sp, m] - p["a"][k0:k1, m].sum()) < 1e-12
            for n in range(N):
                want = sum(p["a"][k, m] * (p["b"][b_idx[k], n] if n < N1 else p["b2"][k, n - N1]) for k in range(k0, k1))
                assert abs(ref["c"]["want"][sp * M + m, n] - want) < 1e-12
    assert ref["c"]["written"][:S * M].all() and not ref["c"]["written"][S * M:].any()
    assert ref["bias_part"]["written"][:S].all() and not ref["bias_part"]["written"][S:].any()
    assert (ref["c"]["want"][3 * M:4 * M] == 0).all()       # the empty split: zeros, written


def _at(buffer, row, col=None):
    """the location as either checker message states it"""
    return rf"buffer {buffer}\b.*row {row}, column" + ("" if col is None else rf" {col}\b")


def _rejects(got, pre, ref, text, exact=True):
    import parity_util as pu
    pu.check_gemm_form(pu.apply_launch(pre, ref), pre, ref, exact)   # (the unplanted result passes)
    with pytest.raises(AssertionError, match=text):
        pu.check_gemm_form(got, pre, ref, exact)


def test_gemm_form_checker_rejects_planted_defects():
    import parity_util as pu
    rng = np.random.default_rng(1)
    for exact in (True, False):
        # a segment boundary off by one k: column K1 of row 2 read from the first segment
        s = _form_spec(rng, exact=exact)
        pre, ref = {"c": s["c"]}, pu.gemm_form_reference(s, 0, exact)
        A, B = pu.gemm_operands(s)
        got = pu.apply_launch(pre, ref)
        r = s["c_idx"][2]
        got["c"][r, :12] += ((float(s["a"][s["a_idx"][2], 8]) - A[2, 8]) * B[8]).astype(np.float32)
        assert s["a"][s["a_idx"][2], 8] != A[2, 8] and B[8, 0] != 0
        _rejects(got, pre, ref, _at("c", r, 0), exact)
        # a scatter row swapped
        got = pu.apply_launch(pre, ref)
        r0, r1 = sorted(s["c_idx"][:2])
        got["c"][[r0, r1]] = got["c"][[r1, r0]]
        _rejects(got, pre, ref, _at("c", r0), exact)
        # a store one row past M (into a row no c_idx names), one column past N
        free = sorted(set(range(s["c"].shape[0])) - set(s["c_idx"].tolist()))[0]
        got = pu.apply_launch(pre, ref)
        got["c"][free, 3] = 1.0
        _rejects(got, pre, ref, _at("c", free, 3), exact)
        got = pu.apply_launch(pre, ref)
        got["c"][s["c_idx"][4], 12] = got["c"][s["c_idx"][4], 11]
        _rejects(got, pre, ref, _at("c", s['c_idx'][4], 12), exact)
        # an accumulate that dropped its pre-value
        s = _form_spec(rng, epi=pu.EPI_ACCUM, exact=exact)
        r = s["c_idx"][5]
        s["c"][r, 7] = 3.0
        pre, ref = {"c": s["c"]}, pu.gemm_form_reference(s, 0, exact)
        got = pu.apply_launch(pre, ref)
        got["c"][r, 7] -= 3.0
        _rejects(got, pre, ref, _at("c", r, 7), exact)
        # a store one row past M into the split output
        s = _form_spec(rng, exact=exact, N1=4, c2=np.full((9, 10), np.nan, np.float32))
        pre, ref = {"c": s["c"], "c2": s["c2"]}, pu.gemm_form_reference(s, 0, exact)
        got = pu.apply_launch(pre, ref)
        got["c2"][7, 0] = got["c2"][6, 0]
        _rejects(got, pre, ref, _at("c2", 7, 0), exact)
        # the mask's slope the wrong way at x == 0
        mask = rng.standard_normal((7, 16)).astype(np.float32)
        mask[1, 2], mask[1, 3] = 0.0, -0.0
        s = _form_spec(rng, exact=exact, mask=mask, c_idx=None)
        pre, ref = {"c": s["c"]}, pu.gemm_form_reference(s, 0, exact)
        A, B = pu.gemm_operands(s)
        for col in (2, 3):
            got = pu.apply_launch(pre, ref)
            got["c"][1, col] = np.float32(A[1] @ B[:, col] + s["bias"][col])
            assert got["c"][1, col] != 0
            _rejects(got, pre, ref, _at("c", 1, col), exact)
    # the L2-norm epilogue: a norm and an element a few ulps off are rejected, the rounded result passes
    s = _form_spec(rng, epi=pu.EPI_L2NORM, exact=False, norms=np.full(9, np.nan, np.float32))
    pre, ref = {"c": s["c"], "norms": s["norms"]}, pu.gemm_form_reference(s)
    got = pu.apply_launch(pre, ref)
    got["norms"][3] *= np.float32(1 + 1e-4)
    _rejects(got, pre, ref, _at("norms", 3, 0), False)
    got = pu.apply_launch(pre, ref)
    got["norms"][7] = 1.0
    _rejects(got, pre, ref, _at("norms", 7, 0), False)


def test_reduce_slabs_order_emulation_and_checker():
    import parity_util as pu
    rng = np.random.default_rng(2)
    f = np.float32
    for S in (1, 2, 3, 4, 5, 16, 17, 64):
        x = rng.standard_normal((S, 3, 8)).astype(f)
        # group g by hand: the first sixteen slabs four at a time, then one by one
        acc = []
        for g in range(4):
            ks = list(range(g, S, 4))
            a = np.zeros((3, 8), f)
            while len(ks) >= 4:
                a = a + ((x[ks[0]] + x[ks[1]]) + (x[ks[2]] + x[ks[3]]))
                ks = ks[4:]
            for k in ks:
                a = a + x[k]
            acc.append(a)
        want = (acc[0] + acc[1]) + (acc[2] + acc[3])
        assert (pu.bits32(pu.reduce_slabs32(x)) == pu.bits32(want)).all(), S
        pre = np.full((5, 12), np.nan, f)
        good = pre.copy()
        good[:3, :8] = want
        pu.check_reduce_slabs("out", good, pre, x, 3, 8)
        if S >= 2:   # a slab skipped
            bad = pre.copy()
            bad[:3, :8] = pu.reduce_slabs32(np.delete(x, S // 2, 0))
            with pytest.raises(AssertionError, match="buffer out.*row 0, column 0"):
                pu.check_reduce_slabs("out", bad, pre, x, 3, 8)
        bad = good.copy()
        bad[3, 0] = 0.0      # a store one row past M
        with pytest.raises(AssertionError, match=_at("out", 3, 0)):
            pu.check_reduce_slabs("out", bad, pre, x, 3, 8)
    ints = pu.exact_ints(rng, (17, 3, 8))
    assert (pu.reduce_slabs32(ints) == ints.astype(np.float64).sum(0)).all()


def test_adam_reference_is_torch_adam_and_checker_rejects_defects():
    import parity_util as pu
    rng = np.random.default_rng(3)
    n, lr, betas, eps = 64, 1e-3, (0.9, 0.999), 1e-8
    p0 = rng.standard_normal(n).astype(np.float32)
    # one step from float32 state against torch, exactly the restated formulas
    tp = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps)
    g = pu.adam_gradient(rng, n)
    tp.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    c1 = np.array([lr / (1 - betas[0]), (1 - betas[1]) ** 0.5])
    r = pu.adam_reference(p0, g, np.zeros(n, np.float32), np.zeros(n, np.float32), c1, *betas, eps)
    assert np.abs(r["p"] - tp.detach().numpy()).max() <= 1e-12
    st = opt.state[tp]
    assert np.abs(r["m"] - st["exp_avg"].numpy()).max() <= 1e-15 * 1e4
    assert np.abs(r["v"] - st["exp_avg_sq"].numpy()).max() <= 1e-15 * 1e8
    # the checker: the float32 rounding of the reference passes; swapped betas and a dropped bias correction do not
    m0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v0 = (rng.random(n) * 1e-2).astype(np.float32)
    coef = pu.adam_coef(3, lr, *betas)
    ref = pu.adam_reference(p0, g, m0, v0, coef, *betas, eps)
    f = lambda d: (d["p"].astype(np.float32), d["m"].astype(np.float32), d["v"].astype(np.float32))
    pu.check_adam(*f(ref), ref)
    with pytest.raises(AssertionError, match="adam m: .* element 0"):
        pu.check_adam(*f(pu.adam_reference(p0, g, m0, v0, coef, *betas, eps, swap_betas=True)), ref)
    bad = pu.adam_reference(p0, g, m0, v0, coef, *betas, eps, drop_bc2=True)
    assert (bad["m"] == ref["m"]).all() and (bad["v"] == ref["v"]).all()
    with pytest.raises(AssertionError, match="adam p: .* element"):
        pu.check_adam(*f(bad), ref)
    # a refused step's state and the tiny gradients: g = 1e-30 leaves v's float32 at 0 within the bound
    z = np.zeros(4, np.float32)
    tiny = pu.adam_reference(z, np.full(4, 1e-30, np.float32), z, z, pu.adam_coef(1), *betas, eps)
    pu.check_adam(tiny["p"].astype(np.float32), tiny["m"].astype(np.float32), z, tiny)


def test_norm_lrelu_bwd_reference_is_autograd():
    import parity_util as pu
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.standard_normal((5, 9))).requires_grad_()
    x.data[0, 0] = 0.0
    v = torch.nn.functional.leaky_relu(x)
    nrm = v.norm(dim=1)
    y = v / nrm[:, None]
    dy = rng.standard_normal((5, 9))
    y.backward(torch.from_numpy(dy))
    want, bound = pu.norm_lrelu_bwd_reference(y.detach().numpy(), nrm.detach().numpy(), dy)
    # (0.01f against 0.01: 2.2e-8 relative in the slope's rows)
    assert np.abs(want - x.grad.numpy()).max() <= 1e-7 * np.abs(want).max()
    assert (bound > 0).all()


# ----------------------------------------------------------------------------- fused sampler edges (sampler_util)
def test_sampler_references_against_plain_loops():
    """runs_from_trace, dense_from_runs and norm_pair (tests/sampler_util.py)
    against loops over Python ints and floats."""
    import sampler_util as su
    rng = np.random.default_rng(0)
    for n_hops, n_all, src in ((1, 5, 0), (24, 40, 7), (200, 30, 29), (64, 3, 1)):
        trace = rng.integers(0, n_all, n_hops)
        trace[rng.integers(0, n_hops)] = src
        counts = {}
        for v in trace.tolist():
            if v != src:
                counts[v] = counts.get(v, 0) + 1
        want = [[i, counts[i]] for i in sorted(counts)]
        got = su.runs_from_trace(trace, src)
        assert got.dtype == np.int64 and got.shape == (len(want), 2) and got.tolist() == want
        su.check_row_preconditions(got, n_hops, n_all)
        dense = su.dense_from_runs(got, n_all, n_hops)
        assert dense.dtype == np.float64 and dense.shape == (n_all,)
        for j in range(n_all):
            assert dense[j] == (counts.get(j, 0) / n_hops if j != src else 0.0)
    assert su.runs_from_trace([4, 4, 4], 4).shape == (0, 2)          # every hop came back: no runs
    w = np.array([[0.5, 0.25, 0.125, 0.0], [0.0, 0.0, 0.0, 0.0], [1 / 3, 1 / 3, 1 / 7, 1 / 24]])
    nb = np.array([[9, 8, 70000, 1], [0, 1, 2, 3], [5, 6, 7, 8]])
    for t in (1, 2, 4):
        wn, nb32 = su.norm_pair(w, nb, t)
        assert wn.dtype == np.float32 and nb32.dtype == np.int32 and wn.shape == (3, t)
        for i in range(3):
            s = 0.0
            for j in range(t):
                s += float(w[i, j])
            for j in range(t):
                if s == 0.0:
                    assert np.isnan(wn[i, j])
                else:
                    assert wn[i, j] == np.float32(float(w[i, j]) / s)
                assert nb32[i, j] == nb[i, j]


_SAMPLER_SHAPES = [(24, 10), (24, 1), (24, 2), (24, 3), (24, 16), (200, 1), (200, 2), (200, 3), (200, 10), (200, 16)]


def test_sampler_hand_built_rows_meet_the_kernel_preconditions():
    """Every hand-built row of the top-k cases holds what heap_topk_kernel
    assumes (ids strictly ascending, counts >= 1, nr <= n_hops, counts summing
    to <= n_hops), the catalogue contains the shapes the issue names, the
    precondition check itself rejects a bad row, and the G table is what the
    launcher's rule gives."""
    import sampler_util as su
    for n_hops, k in _SAMPLER_SHAPES + [(24, 1000), (24, 8191), (24, 16383)]:
        cat = su.topk_catalogue(n_hops, k, n_random=160 if k <= 16 else 0)
        n_all = su.topk_n_all(k, n_hops)
        assert k * 64 <= n_all
        names = [nm for nm, _ in cat]
        assert len(set(names)) == len(names)
        for nm, r in cat:
            assert r.dtype == np.int64 and r.ndim == 2 and r.shape[1] == 2, nm
            su.check_row_preconditions(r, n_hops, n_all)
        rows = dict(cat)
        nrs = {len(r) for r in rows.values()}
        assert {0, 1, 7, 8, 9, 15, 16, 17, n_hops} <= nrs, (n_hops, k)
        n_below = lambda r: int((r[:, 0] < k).sum())
        assert any(len(r) and n_below(r) == len(r) for r in rows.values())       # all runs below k
        assert any(len(r) and n_below(r) == 0 for r in rows.values())            # all at or above k
        # pure ties: more than k of them where a walk can give as many
        assert any(len(r) > min(k, n_hops - 1) and len(set(r[:, 1])) == 1 for r in rows.values())
        assert any(len(r) > 2 and (np.diff(r[:, 1]) > 0).all() for r in rows.values())
        assert any(len(r) > 2 and (np.diff(r[:, 1]) < 0).all() for r in rows.values())
        assert any(len(r) > 1 and r[:, 1].max() == n_hops - (len(r) - 1) for r in rows.values())
        if k > 1:
            assert any(0 < len(r) < k for r in rows.values())                     # fewer non-zero entries than k
        if k >= 10:  # the first sparse run at index 0 / 7 / 8 / 9, tails on both sides of the prefetch width
            for p in (0, 7, 8, 9):
                tails = {len(r) - p for nm, r in cat if nm.startswith(f"first-sparse{p}-") and n_below(r) == p}
                assert {1, 7, 8, 9} <= tails, (k, p, tails)
        # a multiple of 8 sparse runs and one more / one fewer: nr - first sparse index
        tail = {len(r) - n_below(r) for r in rows.values()}
        assert {0, 1, 7, 8, 9, 15, 16, 17} <= tail
    for bad in ([[3, 1], [3, 1]], [[5, 1], [4, 1]], [[1, 0]], [[1, 20], [2, 5]], [[i, 1] for i in range(25)]):
        with pytest.raises(AssertionError):
            su.check_row_preconditions(np.array(bad), 24)
    for n_src, G in su.G_TABLE.items():
        assert su.heap_G(n_src, 10) == G
    for (k, n_src), G in su.G_LDS_TABLE.items():
        assert su.heap_G(n_src, k) == G


def _tie_heavy_rows(n, k, rng, rows=6):
    """sparse float64 rows of few distinct values (count / 24), so that the k-th
    place falls inside a tie and the tail is zeros"""
    m = np.zeros((rows, n), np.float64)
    for r in range(rows):
        nz = int(rng.integers(0, min(n, 2 * k + 8) + 1))
        at = rng.choice(n, nz, replace=False)
        m[r, at] = rng.integers(1, 4, nz) / 24.0
    return m


@pytest.mark.parametrize("n,k", [(640, 10), (639, 10), (64, 1), (63, 1), (6400, 100), (2000, 31), (70000, 1000),
                                 (100, 100), (100, 99), (5, 5), (1, 1)])
def test_oracle_topk_is_torch_topk_on_tie_heavy_rows(n, k):
    """oracle.topk (libstdc++ restated in C) and the installed torch CPU topk
    agree bit for bit, ids included, in both libstdc++ regimes: the tie order
    the device is held to comes from two independent implementations."""
    from oracle import oracle as orc
    m = _tie_heavy_rows(n, k, np.random.default_rng(n + k))
    w, nb = orc.topk(m, k)
    tw, tn = torch.from_numpy(m).topk(k, 1)
    assert (w.view(np.uint64) == tw.numpy().view(np.uint64)).all()
    assert (nb == tn.numpy()).all()


@pytest.mark.parametrize("n_hops,k", _SAMPLER_SHAPES)
def test_oracle_topk_is_torch_topk_on_the_hand_built_rows(n_hops, k):
    import sampler_util as su
    from oracle import oracle as orc
    n_all = su.topk_n_all(k, n_hops)
    rows = [r for _, r in su.topk_catalogue(n_hops, k)]
    dense = np.stack([su.dense_from_runs(r, n_all, n_hops) for r in rows])
    w, nb = orc.topk(dense, k)
    tw, tn = torch.from_numpy(dense).topk(k, 1)
    assert (w.view(np.uint64) == tw.numpy().view(np.uint64)).all()
    assert (nb == tn.numpy()).all()
    ref = su.topk_reference(rows, n_all, n_hops, k, k, chunk_bytes=8 * n_all * 7)  # chunks of 7 rows
    assert (ref[0] == w).all() and (ref[1] == nb).all()


def test_sampler_checkers_reject_planted_defects():
    """One defect at a time in a fake device result; each must be rejected
    with the source index and the column in the message."""
    import sampler_util as su
    n_hops, k, t_norm = 24, 10, 4
    cat = su.topk_catalogue(n_hops, k)
    rows = [r for _, r in cat][:60]
    names = [nm for nm, _ in cat][:60]
    cap = len(rows) + 5
    runs, n_runs = su.expected_runs(rows, cap, n_hops)
    su.check_runs("clean", runs, n_runs, rows, n_hops)
    # self run kept: source 12's own id (one not in its runs) stays in the list
    s = 12
    r = rows[s]
    self_id = int(np.setdiff1d(np.arange(k + 40), r[:, 0])[3])
    at = int(np.searchsorted(r[:, 0], self_id))
    kept = np.insert(r, at, [self_id, 1], axis=0)
    bad_runs, bad_n = su.expected_runs(rows[:s] + [kept] + rows[s + 1:], cap, n_hops)
    with pytest.raises(AssertionError, match=r"n_runs: source 12 column 0: got \d+, reference \d+"):
        su.check_runs("self", bad_runs, bad_n, rows, n_hops)
    with pytest.raises(AssertionError, match=rf"source 12 column {2 * at}: got {self_id},"):
        su.check_runs("self", bad_runs, n_runs, rows, n_hops)
    # a run's count off by one
    s = next(i for i, r in enumerate(rows) if len(r) >= 9)
    bad_runs = runs.copy()
    bad_runs[s, 8, 1] += 1
    with pytest.raises(AssertionError, match=rf"source {s} column 17: got {int(rows[s][8, 1]) + 1}, reference "
                                             rf"{int(rows[s][8, 1])}; 1 of"):
        su.check_runs("count", bad_runs, n_runs, rows, n_hops)
    # a sentinel overwritten past a source's runs, and past the live sources
    s = next(i for i, r in enumerate(rows) if len(r) == 7)
    bad_runs = runs.copy()
    bad_runs[s, 7] = (99, 1)
    with pytest.raises(AssertionError, match=rf"source {s} column 14: got 99, reference {su.SENT_U32}"):
        su.check_runs("past", bad_runs, n_runs, rows, n_hops)
    bad_n = n_runs.copy()
    bad_n[len(rows) + 2] = 0
    with pytest.raises(AssertionError, match=rf"n_runs: source {len(rows) + 2} column 0: got 0, reference -1"):
        su.check_runs("past live", runs, bad_n, rows, n_hops)
    # top-k outputs
    n_all = su.topk_n_all(k, n_hops)
    ref = su.topk_reference(rows, n_all, n_hops, k, t_norm)
    live = len(rows) - 3
    want = su.expected_topk(ref, live, cap)
    clean = lambda: [a.copy() for a in want]
    su.check_topk("clean", clean(), want)
    # two tied ids swapped
    s = names.index("nr24-sparse")
    w_row = ref[0][s]
    c = next(j for j in range(k - 1) if w_row[j] == w_row[j + 1])
    got = clean()
    got[1][s, [c, c + 1]] = got[1][s, [c + 1, c]]
    with pytest.raises(AssertionError, match=rf"nb_out: source {s} column {c}: got {int(ref[1][s, c + 1])}, reference "
                                             rf"{int(ref[1][s, c])}; 2 of"):
        su.check_topk("swap", got, want)
    if c < t_norm - 1:
        got = clean()
        got[3][s, [c, c + 1]] = got[3][s, [c + 1, c]]
        with pytest.raises(AssertionError, match=rf"nb32_out: source {s} column {c}:"):
            su.check_topk("swap32", got, want)
    # a row shifted by one source
    got = clean()
    for a in got:
        a[1:live] = a[0:live - 1].copy()
    first = next(i for i in range(1, live) if not np.array_equal(ref[1][i], ref[1][i - 1])
                 or not np.array_equal(ref[0][i], ref[0][i - 1]))
    with pytest.raises(AssertionError, match=rf"_out: source {first} column \d+:"):
        su.check_topk("shift", got, want)
    # another lane's row sum: the normalised weights of one source scaled
    s = next(i for i in range(live) if ref[0][i, 0] > 0)
    got = clean()
    got[2][s] = got[2][s] * np.float32(0.5)
    with pytest.raises(AssertionError, match=rf"wn_out: source {s} column 0: got .*0x[0-9a-f]+\), reference"):
        su.check_topk("rowsum", got, want)
    # a sentinel overwritten past the live rows; an unwritten live element
    got = clean()
    got[0][live + 1, 3] = 0.0
    with pytest.raises(AssertionError, match=rf"w_out: source {live + 1} column 3: got 0.0 \(0x0\), reference nan \(0x7ff80000deadbeef\)"):
        su.check_topk("past live", got, want)
    got = clean()
    got[2][2, 1] = su.sentinel_array((1,), np.float32)[0]
    with pytest.raises(AssertionError, match=r"wn_out: source 2 column 1:"):
        su.check_topk("unwritten", got, want)
    # a source without runs: the reference's NaN matches a device NaN of any sign, never the sentinel
    e = names.index("nr0-sparse")
    assert e < live and np.isnan(ref[2][e]).all()
    got = clean()
    got[2][e] = -got[2][e]
    su.check_topk("nan sign", got, want)
    got[2][e, 0] = su.sentinel_array((1,), np.float32)[0]
    with pytest.raises(AssertionError, match=rf"wn_out: source {e} column 0:"):
        su.check_topk("nan sentinel", got, want)


def test_sampler_traces_and_graphs_are_what_the_gpu_tests_assume():
    """The hand-built traces of the pinsage_visit_topk cases give back their
    rows (preconditions held, the source outside them), and the walk graphs
    have the nodes the cases name: a degree-1 item, hubs, the item whose only
    playlist leads back to it, zero-degree sources and a sink column whose
    walks the oracle refuses -- with every id inside the graph."""
    import sampler_util as su
    for n_all, k in su.VISIT_SHAPES:
        rng = np.random.default_rng(n_all * 7 + k)
        rows, src = su.visit_rows(n_all, k, su.VISIT_N_HOPS, rng)
        assert any(len(r) == 0 for r in rows)
        if n_all > 2:
            assert any(len(r) > 1 and len(set(r[:, 1])) == 1 for r in rows)                     # all ties
            assert any(len(r) > 1 and r[:, 1].max() == su.VISIT_N_HOPS - len(r) + 1 for r in rows)  # one dominant
        for r, s in zip(rows, src):
            su.check_row_preconditions(r, su.VISIT_N_HOPS, n_all)
            tr = su.trace_from_runs(r, s, su.VISIT_N_HOPS, rng)
            assert tr.dtype == np.int32 and tr.shape == (su.VISIT_N_HOPS,)
            assert 0 <= tr.min() and tr.max() < n_all
            assert np.array_equal(su.runs_from_trace(tr, s), r)
    indptr, indices, n_all, sp = su.bipartite_graph()
    deg = np.diff(indptr)
    assert len(indptr) == n_all + 1 and indptr[-1] == len(indices) and 0 <= indices.min() and indices.max() < n_all
    assert deg.min() == 1 and deg.max() >= 290 and deg[0] >= 290 and deg[n_all - 1] >= 1
    lo = sp["loner"]
    pl = indices[indptr[lo]:indptr[lo + 1]]
    assert len(pl) == 1 and indices[indptr[pl[0]]:indptr[pl[0] + 1]].tolist() == [lo]
    tr = su.oracle_traces(indptr, indices, [lo, 0], 70, np.float32(0.0), seed=1)
    assert (tr[0] == lo).all() and len(su.runs_from_trace(tr[1], 0)) > 4
    indptr, indices, n_all, _ = su.two_item_graph()
    tr = su.oracle_traces(indptr, indices, [0, 1, 2], 200, np.float32(0.5), seed=2)
    assert set(tr[0]) == {0, 1} and set(tr[2]) == {2}
    for name, indptr, indices, n_all, sources, bad in su.zero_degree_graphs():
        assert len(indptr) == n_all + 1 and indices.max() < n_all and sources.max() < n_all and sources.min() >= 0
        for alpha in (0.0, 1.0):
            tr = su.oracle_traces(indptr, indices, sources, 9, np.float32(alpha), seed=3)
            assert [i for i, t in enumerate(tr) if t is None] == bad, name
        rows = su.oracle_runs(tr, sources)
        runs, n_runs = su.expected_runs(rows, len(sources), 9)
        assert all(n_runs[i] == 0 for i in bad) and (runs[bad] == su.SENT_U32).all()
