"""The LMF kernels (csrc/lmf.hip) at the C2 graph's collection-track shape:
synthetic.make_playlist_graph_device with bench.py's C2 graph (100k tracks, its
collection count and memberships), f = 128.

    python tools/lmf_bench.py [--factors 128] [--reps 20] [--fit-reps 3] [--scale 1.0]

times, with device events after a warm-up, the routes alternating (the median
and the spread of --reps runs), and prints one JSON line:
  (a) pinsage_lmf_dense for the user rows (collections against all tracks) and
      for the item rows (tracks against all collections);
  (b) the torch composition of the same dense terms at fp32: row chunks of
      torch.mm, torch.sigmoid, torch.mm, the chunk as many rows as fit
      baselines.KNN_SCRATCH_BYTES of scores;
  (c) pinsage_lmf_update for both sides, each from a fresh copy of the same
      tables and accumulators;
  (d) LMF.fit, 30 iterations, from given factors, whole (--fit-reps runs).
(a) and (b) are compared on their results.  FLOPs of the dense terms: two
products, 4 rows n_other f; the composition also moves 8 rows n_other bytes of
scores through memory that the fused kernel never forms.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gcn-song-embeddings_amd"))
sys.path.insert(0, REPO)

F32_MFMA_PEAK = 157.3e12  # 256 CUs x 256 FLOP/clk x 2.4 GHz


def _spread(ts):
    ts = sorted(ts)
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1],
            "p10_ms": ts[len(ts) // 10], "p90_ms": ts[(len(ts) * 9) // 10], "runs": len(ts)}


def torch_dense(X, bx, Y, by, chunk, D, dsum):
    """D = sigmoid(X Y^T + bx + by^T) Y and its row sums by library calls, `chunk` rows of scores at a time."""
    import torch
    for r0 in range(0, int(X.shape[0]), chunk):
        s = torch.mm(X[r0:r0 + chunk], Y.T)
        s += bx[r0:r0 + chunk, None]
        s += by[None, :]
        p = torch.sigmoid_(s)
        torch.mm(p, Y, out=D[r0:r0 + chunk])
        torch.sum(p, 1, out=dsum[r0:r0 + chunk])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-reps", type=int, default=3)
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
        raise SystemExit("lmf_bench needs the GPU: nothing is measured without one")
    cfg = bench.CONFIGS["c2"]
    n, nc, mem = (int(cfg[key] * a.scale) for key in ("n_tracks", "n_cols", "memberships"))
    indptr, indices = synthetic.make_playlist_graph_device(n, nc, mem, seed=0, device="cuda")
    g = graph.DeviceCSRGraph(indptr, indices)
    model = bl.LMF(factors=a.factors)
    f, reg, alpha, lr = model.factors, model.regularization, model.alpha, model.learning_rate
    ct = bl.to_col_track_matrix(g, range(n))
    gen = torch.Generator().manual_seed(1)
    X0 = ((torch.rand(nc, f, generator=gen) - 0.5) / f).cuda()
    Y0 = ((torch.rand(n, f, generator=gen) - 0.5) / f).cuda()
    # trained-size biases, so that the scores are not all near 0
    bx0 = (torch.rand(nc, generator=gen) - 0.5).cuda()
    by0 = (torch.rand(n, generator=gen) - 2.5).cuda()
    idx = ct[1]
    # the two sides: (csr, rows updated, their bias, fixed table, its bias)
    sides = {"users": (ct, X0, bx0, Y0, by0), "items": (bl._csr_transpose(*ct), Y0, by0, X0, bx0)}
    L, st = nat.lib(), nat.stream_ptr
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    D = {s: torch.empty_like(sides[s][1]) for s in sides}
    dsum = {s: torch.empty_like(sides[s][2]) for s in sides}
    Dt = {s: torch.empty_like(sides[s][1]) for s in sides}
    dsumt = {s: torch.empty_like(sides[s][2]) for s in sides}
    work = {s: [sides[s][1].clone(), sides[s][2].clone(), torch.ones_like(sides[s][1]), torch.ones_like(sides[s][2])]
            for s in sides}
    chunk = {s: max(1, bl.KNN_SCRATCH_BYTES // (4 * int(sides[s][3].shape[0]))) for s in sides}

    def dense(s):
        c, x, b, y, yb = sides[s]
        nat.check(L.pinsage_lmf_dense(nat.ptr(x), nat.ptr(b), c[3], f, nat.ptr(y), nat.ptr(yb), c[4], f, f,
                                      nat.ptr(D[s]), f, nat.ptr(dsum[s]), st()), "lmf_dense")

    def reset(s):
        w = work[s]
        w[0].copy_(sides[s][1])
        w[1].copy_(sides[s][2])
        w[2].fill_(1.0)
        w[3].fill_(1.0)

    def update(s):
        c, _, _, y, yb = sides[s]
        w = work[s]
        nat.check(L.pinsage_lmf_update(nat.ptr(c[0]), nat.ptr(c[1]), nat.ptr(c[2]), c[3], nat.ptr(y), nat.ptr(yb),
                                       c[4], f, nat.ptr(w[0]), nat.ptr(w[1]), f, f, nat.ptr(D[s]), f,
                                       nat.ptr(dsum[s]), nat.ptr(w[2]), f, nat.ptr(w[3]), alpha, reg, lr,
                                       nat.ptr(err), st()), "lmf_update")

    routes = {}
    for s in sides:
        routes[f"dense_{s}"] = lambda s=s: dense(s)
        routes[f"torch_dense_{s}"] = lambda s=s: torch_dense(sides[s][1], sides[s][2], sides[s][3], sides[s][4],
                                                             chunk[s], Dt[s], dsumt[s])
        routes[f"update_{s}"] = lambda s=s: (reset(s), update(s))
        routes[f"reset_{s}"] = lambda s=s: reset(s)

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
    out = {"metric": "device events (ms)", "n_tracks": n, "n_cols": nc, "nnz": int(idx.numel()), "factors": f,
           "rows_per_workgroup": int(L.pinsage_lmf_row_block()), "long_row_above": int(L.pinsage_lmf_long_row()),
           "f32_mfma_peak_TFLOPs": F32_MFMA_PEAK / 1e12}
    for s, (c, x, b, y, yb) in sides.items():
        rows, other = int(c[3]), int(c[4])
        flops = 4 * rows * other * f
        ms, tms = res[f"dense_{s}"]["median_ms"], res[f"torch_dense_{s}"]["median_ms"]
        scale = float(Dt[s].abs().max())
        res[f"dense_{s}"].update({
            "rows": rows, "n_other": other, "workgroups": -(-rows // int(L.pinsage_lmf_row_block())),
            "flops": flops, "TFLOPs": flops / (ms * 1e-3) / 1e12,
            "fraction_of_f32_mfma_peak": flops / (ms * 1e-3) / F32_MFMA_PEAK,
            "torch_over_kernel": tms / ms, "torch_chunk_rows": chunk[s],
            "torch_TFLOPs": flops / (tms * 1e-3) / 1e12, "score_bytes_not_moved": 8 * rows * other,
            "max_diff_vs_torch_rel_to_largest": float((D[s] - Dt[s]).abs().max()) / scale,
            "dsum_max_rel_diff_vs_torch": float(((dsum[s] - dsumt[s]).abs() / dsumt[s]).max())})
        res[f"update_{s}"].update({
            "rows": rows, "nnz": int(c[1].numel()),
            "kernel_ms_less_reset": res[f"update_{s}"]["median_ms"] - res[f"reset_{s}"]["median_ms"]})

    fit = bl.LMF(factors=f)
    fts = []
    for i in range(a.fit_reps + 1):
        t = timed(lambda: fit.fit(ct, user_factors=X0, item_factors=Y0))
        if i:
            fts.append(t)
    res["fit_30_iterations"] = _spread(fts)
    res["fit_30_iterations"]["objective"] = fit.objective()
    res["fit_30_iterations"]["objective_at_start"] = bl.lmf_objective(
        ct, X0, Y0, torch.zeros(nc, device="cuda"), torch.zeros(n, device="cuda"), reg, alpha)
    out["routes"] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
