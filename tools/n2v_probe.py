"""The node2vec kernels (csrc/n2v.hip) at the C2 graph's size (100 000 tracks):

    python tools/n2v_probe.py [--factors 128] [--reps 10] [--scale 1.0]

One JSON line per stage, each timed with HIP events after a warm-up and a
synchronise:
  (a) pinsage_n2v_walk: 10 walks of 20 from every track of the weighted
      projection (baselines.project_bipartite_graph), in walks per second;
  (b) n2v_cooccurrence of those walks (plain torch, once, wall clock);
  (c) one SGNS iteration (both half-iterations: dense + update each) at
      --factors, from the documented initial tables;
  (d) pinsage_lmf_dense against pinsage_sgns_dense on the same n x n shape and
      tables, alternating within one run: the weighted form adds one multiply
      per score, so a ratio beyond the run-to-run spread wants an explanation.
Nothing is gated; the figures go into DESIGN.md by hand.
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
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1], "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="rehearsal only: scale the graph")
    a = ap.parse_args()

    import torch

    import _native as nat
    import baselines as bl
    import bench
    import graph
    import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("n2v_probe needs the GPU: nothing is measured without one")
    cfg = bench.CONFIGS["c2"]
    n, nc, mem = (int(cfg[key] * a.scale) for key in ("n_tracks", "n_cols", "memberships"))
    indptr, indices = synthetic.make_playlist_graph_device(n, nc, mem, seed=0, device="cuda")
    g = graph.DeviceCSRGraph(indptr, indices)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return _spread(ts)

    def say(**kw):
        print(json.dumps(kw), flush=True)

    t0 = time.time()
    proj = bl.project_bipartite_graph(g, range(n))
    torch.cuda.synchronize()
    say(stage="projection", n=n, edges=int(proj[1].numel()), max_degree=int((proj[0][1:] - proj[0][:-1]).max()),
        seconds=time.time() - t0)

    f = a.factors
    model = bl.Node2Vec(dim=f, random_state=1)
    L, st = nat.lib(), nat.stream_ptr
    ptr, idx, cum, _ = model._graph(proj)
    starts = torch.arange(n, dtype=torch.int64, device="cuda").repeat(model.walks_per_node)
    walks = torch.empty((int(starts.numel()), model.walk_length), dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def walk():
        nat.check(L.pinsage_n2v_walk(nat.ptr(ptr), nat.ptr(idx), nat.ptr(cum), n, nat.ptr(starts), int(starts.numel()),
                                     model.walk_length, 1.0 / model.p, 1.0 / model.q, 1, 0, 0, nat.ptr(walks),
                                     nat.ptr(err), st()), "n2v_walk")
    r = timed(walk, a.reps)
    assert int(err) == 0
    say(stage="walk", walks=int(starts.numel()), length=model.walk_length,
        walks_per_second=int(starts.numel()) / (r["median_ms"] * 1e-3), **r)

    t0 = time.time()
    C = bl.n2v_cooccurrence(walks, n, model.context)
    torch.cuda.synchronize()
    say(stage="cooccurrence", cells=int(C[1].numel()), seconds=time.time() - t0)

    cnt = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, bl._csr_rows(C[0]), C[2].double())
    pw = torch.where(cnt > 0, cnt ** model.ns_exponent, torch.zeros_like(cnt))
    P = (pw / pw.sum()).float()
    KN = (model.negative * cnt).float()
    gen = torch.Generator().manual_seed(1)
    U = ((torch.rand(n, f, generator=gen) - 0.5) / f).cuda()
    V = ((torch.rand(n, f, generator=gen) - 0.5) / f).cuda()
    Hu, Hv, D = torch.zeros_like(U), torch.zeros_like(V), torch.empty_like(U)

    def iteration():
        model._half(C, P, KN, V, U, Hu, D, err)
        model._half(C, KN, P, U, V, Hv, D, err)
    r = timed(iteration, max(3, a.reps // 3))
    assert int(err) == 0 and bool(torch.isfinite(U).all())
    say(stage="sgns_iteration", factors=f, **r)

    # the two dense forms, alternating, same shape and tables
    zeros, dsum, D2 = torch.zeros(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty_like(U)

    def lmf():
        nat.check(L.pinsage_lmf_dense(nat.ptr(U), nat.ptr(zeros), n, f, nat.ptr(V), nat.ptr(zeros), n, f, f, nat.ptr(D),
                                      f, nat.ptr(dsum), st()), "lmf_dense")

    def sgns():
        nat.check(L.pinsage_sgns_dense(nat.ptr(U), n, f, nat.ptr(V), nat.ptr(P), n, f, f, nat.ptr(D2), f, st()),
                  "sgns_dense")
    lmf(), sgns()
    torch.cuda.synchronize()
    tl, ts = [], []
    for _ in range(a.reps):
        for fn, out in ((lmf, tl), (sgns, ts)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
    rl, rs = _spread(tl), _spread(ts)
    say(stage="dense_forms", rows=n, n_other=n, factors=f, lmf_dense=rl, sgns_dense=rs,
        ratio=rs["median_ms"] / rl["median_ms"], tflops_sgns=4.0 * n * n * f / (rs["median_ms"] * 1e-3) / 1e12)


if __name__ == "__main__":
    main()
