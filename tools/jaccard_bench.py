"""The Jaccard co-occurrence path (csrc/cooc.hip + the selection kernel of
csrc/knn.hip) at the C2 shape against the reference's route on the host:
synthetic.make_playlist_graph_device with bench.py's C2 graph (100k tracks, its
collection count and memberships), 1000 queries, k = 1000.

    python tools/jaccard_bench.py [--queries 1000] [--k 1000] [--reps 25] [--host-queries 1000]

times, with device events after a warm-up, the routes alternating (the median
and the spread of --reps runs), and prints one JSON line:
  (a) pinsage_cooc_counts: the dense int32 count rows of the queries;
  (b) the selection alone (pinsage_cooc_jaccard minus (a): both are timed, and
      the kernel pair is also timed whole);
  (c) JaccardFast.knn whole, from a CPU nodeset to CPU results;
  (d) the reference's route on the host, with 16 threads: scipy ctmat.T * ctmat
      once (reported apart: it is the reference's train()), then per batch of 128
      queries rows.toarray(), the score tensors as baselines.py:211-217 forms
      them, and torch.topk.
(c) and (d) are compared on their scores.  Algorithmic bytes: (a) writes
nq n 4; the selection reads nq n 4 of counts (more than once where a row takes
the radix path) and n 4 of degrees per row from cache.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gcn-song-embeddings_amd"))
sys.path.insert(0, REPO)


def _spread(ts):
    ts = sorted(ts)
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1],
            "p10_ms": ts[len(ts) // 10], "p90_ms": ts[(len(ts) * 9) // 10], "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--host-queries", type=int, default=1000, help="queries of the host route (0: skip it)")
    ap.add_argument("--scale", type=float, default=1.0, help="rehearsal only: scale the graph")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")

    import numpy as np
    import torch

    import _native as nat
    import baselines as bl
    import bench
    import graph
    import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("jaccard_bench needs the GPU: nothing is measured without one")
    torch.set_num_threads(16)
    cfg = bench.CONFIGS["c2"]
    n, nc, mem = (int(cfg[key] * a.scale) for key in ("n_tracks", "n_cols", "memberships"))
    indptr, indices = synthetic.make_playlist_graph_device(n, nc, mem, seed=0, device="cuda")
    g = graph.DeviceCSRGraph(indptr, indices)
    model = bl.JaccardFast()
    t0 = time.time()
    model.train(g, range(n), None, None, None)
    torch.cuda.synchronize()
    train_s = time.time() - t0
    L = nat.lib()
    nq, k = a.queries, a.k
    queries = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:nq].contiguous()
    qd = queries.cuda()
    counts = torch.empty((nq, n), dtype=torch.int32, device="cuda")
    w = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    nb = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = int(L.pinsage_cooc_scratch_bytes(n, nq))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = nat.stream_ptr

    def route_counts():
        nat.check(L.pinsage_cooc_counts(*model._csr_args(), nat.ptr(qd), nq, nat.ptr(counts), nat.ptr(err), st()),
                  "cooc_counts")

    def route_kernels():
        nat.check(L.pinsage_cooc_jaccard(*model._csr_args(), nat.ptr(qd), nq, k, nat.ptr(scratch), nbytes,
                                         nat.ptr(w), nat.ptr(nb), nat.ptr(err), st()), "cooc_jaccard")

    res_knn = []

    def route_knn():
        res_knn[:] = model.knn(queries, k)

    routes = {"cooc_counts": route_counts, "counts_plus_select": route_kernels, "jaccard_knn_whole": route_knn}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):  # warm-up: code objects, the allocator's blocks
        for fn in routes.values():
            timed(fn)
    ts = {name: [] for name in routes}
    for _ in range(a.reps):  # alternating: a drift of the machine falls on every route
        for name, fn in routes.items():
            ts[name].append(timed(fn))
    assert int(err) == 0
    res = {name: _spread(v) for name, v in ts.items()}
    sel = [b - c for b, c in zip(ts["counts_plus_select"], ts["cooc_counts"])]
    res["select_by_difference"] = _spread(sel)
    row_bytes = float(nq) * n * 4
    res["cooc_counts"]["written_GBps"] = row_bytes / (res["cooc_counts"]["median_ms"] * 1e-3) / 1e9
    res["select_by_difference"]["read_once_GBps"] = row_bytes / (res["select_by_difference"]["median_ms"] * 1e-3) / 1e9
    deg = model.nbh_sizes
    out = {"metric": "device events (ms)", "n_tracks": n, "n_cols": nc, "memberships": int(model._t2c[1].numel()),
           "queries": nq, "k": k, "train_s_first_call": train_s, "count_row_bytes": row_bytes,
           "query_degree_mean": float(deg[qd].double().mean()), "query_degree_max": int(deg[qd].max()),
           "nonzero_scores_per_row_mean": float((counts > 0).sum(1).double().mean()), "routes": res}

    if a.host_queries:
        import scipy.sparse as sp
        hq = queries[:a.host_queries].numpy()
        c2t_ptr, c2t_idx = (x.cpu().numpy() for x in model._c2t)
        ctmat = sp.csr_matrix((np.ones(len(c2t_idx), np.int32), c2t_idx, c2t_ptr), shape=(nc, n))
        t0 = time.time()
        inter = ctmat.transpose() * ctmat
        nbh = inter.diagonal()
        host_train = time.time() - t0
        t0 = time.time()
        ws = []
        for i in range(0, len(hq), 128):     # save_knn's batches would be 1000; 128 keeps the three tensors small
            nodeset = hq[i:i + 128]
            it = torch.from_numpy(inter[nodeset, :].toarray())
            nbt = torch.from_numpy(nbh)
            nn_ = nbt[nodeset]
            aa = nn_.repeat((nbt.shape[0], 1)).transpose(1, 0)
            bb = nbt.unsqueeze(0).transpose(1, 0).repeat((1, nn_.shape[0])).transpose(1, 0)
            scores = it / (aa + bb - it + 1e-10)
            tw, _ = torch.topk(scores, k)
            ws.append(tw)
        host_knn = time.time() - t0
        host_w = torch.cat(ws)
        same = bool(torch.equal(host_w[:, 1:], res_knn[0][:len(hq)]))
        per_query_host = host_knn / len(hq)
        per_query_gpu = res["jaccard_knn_whole"]["median_ms"] * 1e-3 / nq
        out.update({"host_product_s": host_train, "host_product_nnz": int(inter.nnz), "host_knn_s": host_knn,
                    "host_queries": int(len(hq)), "host_threads": torch.get_num_threads(),
                    "scores_equal_host": same, "knn_speedup_over_host": per_query_host / per_query_gpu})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
