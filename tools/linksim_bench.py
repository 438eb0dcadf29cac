"""The weighted form of the co-occurrence tile kernel (csrc/cooc.hip) against its
count form at the C2 shape of tools/jaccard_bench.py: the same
synthetic.make_playlist_graph_device graph (100k tracks, bench.py's C2
collection count and memberships), the same 1000 queries, the bipartite CSRs
(the middle nodes are the collections), Adamic-Adar weights.

    python tools/linksim_bench.py [--queries 1000] [--k 1000] [--reps 25]

times, with device events after a warm-up, the routes alternating (the median
and the spread of --reps runs), and prints one JSON line:
  (a) pinsage_cooc_counts        int32 rows [nq, n]   vs
      pinsage_cooc_weighted_sums int64 rows [nq, n]   (half the counters per
      tile, so twice the tiles and binary searches, and twice the bytes written);
  (b) pinsage_cooc_jaccard vs pinsage_cooc_weighted_knn at k (both write float
      or int32 rows of the same size to scratch and run the same selection
      kernel under another key).
Nothing is gated on the ratios.
"""
import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--scale", type=float, default=1.0, help="rehearsal only: scale the graph")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")

    import torch

    import _native as nat
    import baselines as bl
    import bench
    import graph
    import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("linksim_bench needs the GPU: nothing is measured without one")
    cfg = bench.CONFIGS["c2"]
    n, nc, mem = (int(cfg[key] * a.scale) for key in ("n_tracks", "n_cols", "memberships"))
    indptr, indices = synthetic.make_playlist_graph_device(n, nc, mem, seed=0, device="cuda")
    g = graph.DeviceCSRGraph(indptr, indices)
    model = bl.AdamicAdar(projected=False)
    model.train(g, range(n), None, None, None)
    L = nat.lib()
    nq, k = a.queries, a.k
    queries = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:nq].contiguous()
    qd = queries.cuda()
    counts = torch.empty((nq, n), dtype=torch.int32, device="cuda")
    sums = torch.empty((nq, n), dtype=torch.int64, device="cuda")
    w = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    nb = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = max(int(L.pinsage_cooc_scratch_bytes(n, nq)), int(L.pinsage_cooc_weighted_scratch_bytes(n, nq)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = nat.stream_ptr
    csr, wcsr = model._csr_args(), model._weighted_args()

    def route_counts():
        nat.check(L.pinsage_cooc_counts(*csr, nat.ptr(qd), nq, nat.ptr(counts), nat.ptr(err), st()), "cooc_counts")

    def route_sums():
        nat.check(L.pinsage_cooc_weighted_sums(*wcsr, nat.ptr(qd), nq, nat.ptr(sums), nat.ptr(err), st()),
                  "cooc_weighted_sums")

    def route_jaccard():
        nat.check(L.pinsage_cooc_jaccard(*csr, nat.ptr(qd), nq, k, nat.ptr(scratch), nbytes, nat.ptr(w), nat.ptr(nb),
                                         nat.ptr(err), st()), "cooc_jaccard")

    def route_wknn():
        nat.check(L.pinsage_cooc_weighted_knn(*wcsr, nat.ptr(qd), nq, k, nat.ptr(scratch), nbytes, nat.ptr(w),
                                              nat.ptr(nb), nat.ptr(err), st()), "cooc_weighted_knn")

    routes = {"cooc_counts": route_counts, "cooc_weighted_sums": route_sums, "cooc_jaccard": route_jaccard,
              "cooc_weighted_knn": route_wknn}

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
    # the two kernels agree where they must: a non-zero sum exactly where a count is non-zero
    assert bool(((sums > 0) == (counts > 0)).all())
    res = {name: _spread(v) for name, v in ts.items()}
    for name, width in (("cooc_counts", 4), ("cooc_weighted_sums", 8)):
        res[name]["written_GBps"] = float(nq) * n * width / (res[name]["median_ms"] * 1e-3) / 1e9
    deg = model.deg
    out = {"metric": "device events (ms)", "n_tracks": n, "n_cols": nc, "memberships": int(model._t2c[1].numel()),
           "queries": nq, "k": k, "count_tile": int(L.pinsage_cooc_tile()),
           "weighted_tile": int(L.pinsage_cooc_weighted_tile()),
           "query_degree_mean": float(deg[qd].double().mean()), "query_degree_max": int(deg[qd].max()),
           "nonzero_sums_per_row_mean": float((sums > 0).sum(1).double().mean()), "routes": res,
           "sums_over_counts": res["cooc_weighted_sums"]["median_ms"] / res["cooc_counts"]["median_ms"],
           "weighted_knn_over_jaccard": res["cooc_weighted_knn"]["median_ms"] / res["cooc_jaccard"]["median_ms"]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
