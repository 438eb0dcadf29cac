"""Golden fixtures for the lib/gnns GAT aggregator, from the REAL reference.

Runs only in the development container, like make_golden_gnns.py (whose
reference loader and graph it reuses).  Calls the reference's
``GNN_model._get_unique_neighs_list`` and ``GNN_model.aggregate`` with
gat=True, agg_func 'MEAN' as unbound functions on a plain namespace holding
the attributes they read, including the reference's own ``Attention`` module
made under a stored ``torch.manual_seed``, and stores inputs, the attention
weights, the output and the gradients of ``sum(agg * G)`` w.r.t. the
embeddings and the selected attention weight as plain .npz (no pickle).  The
adjacency matrix is gnns_mean.npz's.  The embeddings and G are random values
rounded to float16 before the reference runs and stored as float16 (exact, half
the bytes); everything the reference computed is stored as float32.

The reference's unshifted exp and the product's shifted softmax are the same
number only while the row sums stay finite and >= 1e-12; every case asserts
max |m| < 20 (float64 restatement) so the fixtures stay inside that range.

    python tests/golden/make_golden_gnns_gat.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gnns_gat_util as gu  # noqa: E402
from make_golden_gnns import _graph, _ref_module  # noqa: E402


def _case(mod, name, adj, nodes, input_size, out_size, d, embeds_rows, seed, scale, out):
    n = adj.shape[0]
    adj_list = {}
    for i in range(n):  # DataLoader.get_adj_list (GNNs_unsupervised.py:245-251)
        adj_list[i] = set(np.where(adj[i].toarray() != 0)[1])
    torch.manual_seed(seed)
    att = mod.Attention(input_size, out_size)
    with torch.no_grad():
        att.attention_raw.weight *= scale
        att.attention_emb.weight *= scale
    ns = types.SimpleNamespace(adj_lists=adj_list, adj_matrix=adj, gcn=False, gat=True, agg_func="MEAN",
                               attention=att)
    uniq, samp, uniq_map = mod.GNN_model._get_unique_neighs_list(ns, nodes)
    g = torch.Generator().manual_seed(seed)
    # inputs rounded to float16 values, so that they are stored exactly in half the bytes
    emb = torch.randn(len(uniq) if embeds_rows == "unique" else n, d, generator=g).half().float()
    emb.requires_grad_(True)
    agg = mod.GNN_model.aggregate(ns, nodes, emb, (uniq, samp, uniq_map))
    G = torch.randn(agg.shape, generator=g).half().float()
    (agg * G).sum().backward()
    selected = "attention_raw" if d == input_size else "attention_emb"
    other = "attention_emb" if d == input_size else "attention_raw"
    assert getattr(att, other).weight.grad is None
    samp_ptr = np.zeros(len(samp) + 1, np.int64)
    np.cumsum([len(s) for s in samp], out=samp_ptr[1:])
    c = dict(
        nodes=np.asarray(nodes, np.int64), seed=np.int64(seed), input_size=np.int64(input_size),
        out_size=np.int64(out_size), att_scale=np.float32(scale),
        selected_raw=np.int64(selected == "attention_raw"), unique=np.asarray([int(x) for x in uniq], np.int64),
        samp_ptr=samp_ptr, samp=np.asarray([int(x) for s in samp for x in s], np.int64),
        emb=emb.detach().numpy().astype(np.float16), G=G.numpy().astype(np.float16),
        att_raw=att.attention_raw.weight.detach().numpy(),
        att_emb=att.attention_emb.weight.detach().numpy(), agg=agg.detach().numpy(), grad_emb=emb.grad.numpy(),
        grad_att=getattr(att, selected).weight.grad.numpy())
    assert np.array_equal(c["emb"].astype(np.float32), emb.detach().numpy())
    assert np.array_equal(c["G"].astype(np.float32), G.numpy())
    # inside the range where the reference's unshifted exp is the softmax
    a = c["att_raw"] if selected == "attention_raw" else c["att_emb"]
    r = gu.restate(c["emb"], a, *gu.fixture_csr(c, adj))
    worst = float(np.abs(r["m"]).max())
    assert worst < 20, (name, worst)
    print(f"{name}: max |m| = {worst:.3f}, out vs float64 {gu.rel(c['agg'], r['out']):.2e}")
    out[name] = c


def main():
    mod = _ref_module()
    adj = _graph(300, 3)
    n = adj.shape[0]
    mean = np.load(os.path.join(HERE, "gnns_mean.npz"))
    assert np.array_equal(mean["adj_indptr"], adj.indptr) and np.array_equal(mean["adj_indices"], adj.indices) \
        and np.array_equal(mean["adj_data"], adj.data)
    res = {}
    rng = np.random.default_rng(7)
    nodes = [int(x) for x in rng.choice(n - 3, 60, replace=False)] + [n - 1, n - 2, 0, 5, 0]
    _case(mod, "raw", adj, nodes, 48, 32, 48, "all", 21, 1.0, res)
    _case(mod, "unique_rows", adj, nodes, 32, 32, 32, "unique", 22, 1.0, res)
    _case(mod, "emb", adj, nodes, 48, 32, 32, "unique", 23, 1.0, res)
    _case(mod, "sharp_odd_d", adj, nodes, 30, 16, 30, "all", 24, 6.0, res)
    flat = {}
    for case, d in res.items():
        for k, v in d.items():
            flat[f"{case}__{k}"] = v
    path = os.path.join(HERE, "gnns_gat.npz")
    np.savez_compressed(path, **flat)
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "gnns_mean.npz"))
    print("wrote gnns_gat.npz:", {k: res[k]["agg"].shape for k in res}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
