"""Ranking held-out positives (baselines.rank_from_emb) against the route it
replaces (pinsage_knn_cosine at k = 1000 on the same distinct query rows), at
the C2 table: n = 100k rows, d = 128, 10k pairs over about 5k distinct queries.

    python tools/rank_bench.py [--n 100000] [--d 128] [--pairs 10000] [--queries 5000] [--reps 25]

times both whole calls with device events (warm-up, then the median and the
spread of --reps runs, the two routes alternating) and prints one JSON line.
Kernel times come from a trace of a run of their own:

    rocprofv3 --kernel-trace -f csv -d DIR -- python tools/rank_bench.py --reps 20
    python tools/rank_bench.py --kernel-times DIR

which prints, per kernel of the two routes, the median time of a dispatch
(one dispatch = one batch of query rows, here all of them) and the counting
pass's achieved bytes per second against n * 8 B per query row (4 B of dot
product + 4 B of norm per column).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gcn-song-embeddings_amd"))
sys.path.insert(0, REPO)

KERNELS = ("rank_count_kernel", "knn_select_kernel", "knn_row_norms_kernel", "knn_ids_kernel", "gemm")


def _spread(ts):
    ts = sorted(ts)
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1],
            "p10_ms": ts[len(ts) // 10], "p90_ms": ts[(len(ts) * 9) // 10], "runs": len(ts)}


def kernel_times(trace_dir, a):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    if not rows:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    per = {}
    for r in rows:
        name = r["Kernel_Name"]
        key = next((k for k in KERNELS if k in name), None)
        if key:
            per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    # a call may split its query rows over two dispatches: per call, the sum over the
    # traced run's dispatches by its number of calls (the warm-up's 3 included)
    calls = a.reps + 3
    out = {k: dict(_spread(v), dispatches=len(v), ms_per_call=sum(v) / calls) for k, v in per.items()}
    if "rank_count_kernel" in out:
        bytes_ = float(a.queries) * a.n * 8
        out["rank_count_kernel"]["pass_bytes_per_call"] = bytes_
        out["rank_count_kernel"]["achieved_GBps"] = bytes_ / (out["rank_count_kernel"]["ms_per_call"] * 1e-3) / 1e9
    print(json.dumps({"metric": "kernel time per dispatch (ms)", "n": a.n, "d": a.d, "query_rows": a.queries,
                      "kernels": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=10_000)
    ap.add_argument("--queries", type=int, default=5_000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--kernel-times", metavar="DIR", help="summarise a rocprofv3 kernel trace instead of running")
    a = ap.parse_args()
    if a.kernel_times:
        return kernel_times(a.kernel_times, a)
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")

    import numpy as np
    import torch

    import baselines
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs the GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    emb = torch.from_numpy(rng.standard_normal((a.n, a.d), dtype=np.float32)).cuda()
    dq = rng.choice(a.n, a.queries, replace=False)
    q = torch.from_numpy(np.concatenate([dq, rng.choice(dq, a.pairs - a.queries)]).astype(np.int64)).cuda()
    t = torch.from_numpy(rng.integers(0, a.n, a.pairs).astype(np.int64)).cuda()
    uq = torch.unique(q)
    assert int(uq.numel()) == a.queries
    rows = (baselines.KNN_SCRATCH_BYTES - 8 * a.n) // (4 * a.n)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    rank = lambda: baselines.rank_from_emb(emb, q, t)            # noqa: E731
    knn = lambda: baselines._knn_cosine(emb, uq, a.k)            # noqa: E731
    for _ in range(3):  # warm-up: code objects, the allocator's blocks of both routes
        timed(rank)
        timed(knn)
    tr, tk = [], []
    for _ in range(a.reps):  # alternating: a drift of the machine falls on both
        ms, r = timed(rank)
        tr.append(ms)
        ms, (w, ids) = timed(knn)
        tk.append(ms)
    # the two routes agree on these pairs: a target is in its query's list exactly at column rank
    col = torch.searchsorted(uq, q)
    inlist = r < a.k
    assert bool((ids[col[inlist], r[inlist]] == t[inlist]).all())
    print(json.dumps({"metric": "whole call, device events (ms)", "n": a.n, "d": a.d, "pairs": a.pairs,
                      "distinct_queries": a.queries, "k": a.k, "query_rows_per_batch": int(min(rows, a.queries)),
                      "rank_from_emb": _spread(tr), "knn_cosine_same_rows": _spread(tk),
                      "pairs_within_k": int(inlist.sum()), "dtype": "f32",
                      "data": "synthetic N(0,1) embeddings, uniform targets"}), flush=True)


if __name__ == "__main__":
    main()
