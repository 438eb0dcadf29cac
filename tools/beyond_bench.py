"""The beyond-accuracy kernels (csrc/listmetrics.hip) at the C2 shape against
the straightforward torch formulation on the same GPU: n = 100k queries,
K = 100, d = 512, Gaussian features, lists with the popularity skew of a real
kNN matrix (ids drawn log-uniformly over the popularity ranks: p(rank) ~ 1 / rank).

    python tools/beyond_bench.py [--n 100000] [--k 100] [--d 512] [--pairs 10000] [--reps 25]

times, with device events after a warm-up, the routes alternating (the median
and the spread of --reps runs), and prints one JSON line:
  (a) pinsage_row_inv_norms + pinsage_list_intra_sim (and the second alone);
  (b) normalize(features)[ids].sum(1).pow(2).sum(1) / K^2 in torch, in chunks
      of queries whose gathered rows fit 2 GB;
  (c) pinsage_list_pair_overlap for --pairs pairs at K and at K = 1000.
(a) and (b) are compared on their outputs.  The algorithmic bytes of (a) are
nq K d 4 (the gathered rows) + N d 4 (the norms' pass over the table); the
logical gather rate is nq K d 4 over the time of list_intra_sim alone.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gcn-song-embeddings_amd"))
sys.path.insert(0, REPO)

TORCH_CHUNK_BYTES = 2 << 30


def _spread(ts):
    ts = sorted(ts)
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1],
            "p10_ms": ts[len(ts) // 10], "p90_ms": ts[(len(ts) * 9) // 10], "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--pairs", type=int, default=10_000)
    ap.add_argument("--wide-lists", type=int, default=20_000, help="lists of the K = 1000 overlap run")
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")

    import torch

    import _native as nat
    if not torch.cuda.is_available():
        raise SystemExit("beyond_bench needs the GPU: nothing is measured without one")
    L = nat.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    n, k, d = a.n, a.k, a.d
    feat = torch.randn((n, d), generator=gen, device="cuda", dtype=torch.float32)
    by_rank = torch.randperm(n, generator=gen, device="cuda")

    def skewed(rows, cols):  # p(rank) ~ 1 / rank: the head of the popularity order is in most lists
        u = torch.rand((rows, cols), generator=gen, device="cuda", dtype=torch.float64)
        rank = (torch.exp(u * torch.log(torch.tensor(float(n), dtype=torch.float64))) - 1.0).long().clamp_(0, n - 1)
        return by_rank[rank].contiguous()

    lists = skewed(n, k)
    wide = skewed(a.wide_lists, 1000)
    pairs = torch.randint(0, n, (a.pairs, 2), generator=gen, device="cuda")
    pairs_wide = torch.randint(0, a.wide_lists, (a.pairs, 2), generator=gen, device="cuda")
    inv = torch.empty(n, dtype=torch.float32, device="cuda")
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    ov = torch.empty((a.pairs, 3), dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = nat.stream_ptr

    def norms():
        nat.check(L.pinsage_row_inv_norms(nat.ptr(feat), n, d, d, nat.ptr(inv), st()), "row_inv_norms")

    def intra():
        nat.check(L.pinsage_list_intra_sim(nat.ptr(feat), n, d, d, nat.ptr(inv), nat.ptr(lists), n, k, k,
                                           nat.ptr(out), nat.ptr(err), st()), "list_intra_sim")

    def route_a():
        norms()
        intra()
        return out

    chunk = max(1, TORCH_CHUNK_BYTES // (k * d * 4))
    out_t = torch.empty(n, dtype=torch.float32, device="cuda")

    def route_b():
        fn = torch.nn.functional.normalize(feat, dim=1, eps=0.0)
        for i in range(0, n, chunk):
            out_t[i:i + chunk] = fn[lists[i:i + chunk]].sum(1).pow(2).sum(1) / float(k * k)
        return out_t

    def overlap(lm, pr, kc):
        def run():
            nat.check(L.pinsage_list_pair_overlap(nat.ptr(lm), int(lm.shape[0]), int(lm.shape[1]), kc, n,
                                                  nat.ptr(pr), a.pairs, nat.ptr(ov), nat.ptr(err), st()),
                      "list_pair_overlap")
        return run

    routes = {"kernels_norms_plus_intra": route_a, "list_intra_sim_alone": intra, "torch_chunked": route_b,
              f"pair_overlap_k{k}": overlap(lists, pairs, k), "pair_overlap_k1000": overlap(wide, pairs_wide, 1000)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):  # warm-up: code objects, the allocator's blocks of the torch route
        for fn in routes.values():
            timed(fn)
    ts = {name: [] for name in routes}
    for _ in range(a.reps):  # alternating: a drift of the machine falls on every route
        for name, fn in routes.items():
            ts[name].append(timed(fn))
    assert int(err) == 0
    ka, kb = route_a().double(), route_b().double()
    torch.cuda.synchronize()
    max_diff = float((ka - kb).abs().max())
    assert max_diff <= 1e-4, max_diff
    res = {name: _spread(v) for name, v in ts.items()}
    gathered = float(n) * k * d * 4
    res["list_intra_sim_alone"]["logical_gather_TBps"] = gathered / (res["list_intra_sim_alone"]["median_ms"] * 1e-3) / 1e12
    print(json.dumps({"metric": "device events (ms)", "n": n, "k": k, "d": d, "pairs": a.pairs,
                      "algorithmic_bytes_a": gathered + float(n) * d * 4, "gathered_bytes": gathered,
                      "table_bytes": float(n) * d * 4, "torch_chunk_queries": chunk,
                      "kernels_vs_torch_max_abs_diff": max_diff,
                      "mean_intra_similarity": float(ka.mean()),
                      "speedup_a_over_b": res["torch_chunked"]["median_ms"] / res["kernels_norms_plus_intra"]["median_ms"],
                      "routes": res, "dtype": "f32",
                      "data": "synthetic N(0,1) features, list ids log-uniform over popularity ranks"}), flush=True)


if __name__ == "__main__":
    main()
