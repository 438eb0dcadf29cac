"""The ALS kernels (csrc/als.hip) at the C2 graph's collection-track shape:
synthetic.make_playlist_graph_device with bench.py's C2 graph (100k tracks, its
collection count and memberships), f = 128, cg_steps = 3.

    python tools/als_bench.py [--factors 128] [--reps 25] [--fit-reps 5] [--scale 1.0]

times, with device events after a warm-up, the routes alternating (the median
and the spread of --reps runs), and prints one JSON line:
  (a) pinsage_als_gram over the item table and over the user table;
  (b) pinsage_als_half for the user rows (collections) and for the item rows
      (tracks), each from a fresh copy of the same initial factors;
  (c) the longest row of each side solved alone (one workgroup's work, G staged
      for it alone), against (b): the long-row tail;
  (d) a torch restatement of the same recurrence (index_add_ segment sums, a
      batched G p as a matrix product) for both sides;
  (e) ALS.fit, 15 iterations, from given factors, whole (--fit-reps runs).
(b) and (d) are compared on their results.  Algorithmic bytes of a half:
(1 + steps) nnz f 4 + rows f 8; FLOPs: (1 + steps)(2 f^2 rows + 4 nnz f).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gcn-song-embeddings_amd"))
sys.path.insert(0, REPO)

STEPS = 3


def _spread(ts):
    ts = sorted(ts)
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1],
            "p10_ms": ts[len(ts) // 10], "p90_ms": ts[(len(ts) * 9) // 10], "runs": len(ts)}


def torch_half(rows, idx, c, X, Y, G, steps):
    """The recurrence of pinsage_als_half in torch ops, all rows at once."""
    import torch
    Yi = Y[idx]
    cm = c - 1

    def seg(w):
        return torch.zeros_like(X).index_add_(0, rows, w.unsqueeze(1) * Yi)

    x = X.clone()
    r = seg(c - cm * (Yi * x[rows]).sum(1)) - x @ G
    p = r.clone()
    rs = (r * r).sum(1)
    live = rs >= 1e-20
    for _ in range(steps):
        Ap = p @ G + seg(cm * (Yi * p[rows]).sum(1))
        a = torch.where(live, rs / (p * Ap).sum(1), torch.zeros_like(rs))
        x = x + a.unsqueeze(1) * p
        r = r - a.unsqueeze(1) * Ap
        rn = (r * r).sum(1)
        live = live & (rn >= 1e-20)
        p = r + torch.where(live, rn / rs, torch.zeros_like(rs)).unsqueeze(1) * p
        rs = torch.where(live, rn, rs)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, default=128)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--fit-reps", type=int, default=5)
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
        raise SystemExit("als_bench needs the GPU: nothing is measured without one")
    cfg = bench.CONFIGS["c2"]
    n, nc, mem = (int(cfg[key] * a.scale) for key in ("n_tracks", "n_cols", "memberships"))
    indptr, indices = synthetic.make_playlist_graph_device(n, nc, mem, seed=0, device="cuda")
    g = graph.DeviceCSRGraph(indptr, indices)
    model = bl.ALS(factors=a.factors, cg_steps=STEPS)
    f, reg, alpha = model.factors, model.regularization, model.alpha
    ct = bl.to_col_track_matrix(g, range(n))
    gen = torch.Generator().manual_seed(1)
    X0 = ((torch.rand(nc, f, generator=gen) - 0.5) / f).cuda()
    Y0 = ((torch.rand(n, f, generator=gen) - 0.5) / f).cuda()
    # the two sides: (csr, rows solved, fixed table)
    idx = ct[1]
    sides = {"users": (ct, X0, Y0), "items": (bl._csr_transpose(*ct), Y0, X0)}
    L, st = nat.lib(), nat.stream_ptr
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    G = {s: torch.empty((f, f), dtype=torch.float32, device="cuda") for s in sides}
    work = {s: sides[s][1].clone() for s in sides}

    def gram(s):
        fixed = sides[s][2]
        nat.check(L.pinsage_als_gram(nat.ptr(fixed), int(fixed.shape[0]), f, f, reg, nat.ptr(G[s]), st()), "als_gram")

    def half(s, csr=None, x=None):
        c = sides[s][0] if csr is None else csr
        x = work[s] if x is None else x
        nat.check(L.pinsage_als_half(nat.ptr(c[0]), nat.ptr(c[1]), nat.ptr(c[2]), c[3], nat.ptr(sides[s][2]), c[4], f,
                                     nat.ptr(x), f, f, nat.ptr(G[s]), alpha, STEPS, nat.ptr(err), st()), "als_half")

    longest, alone = {}, {}
    for s, (c, x0, _) in sides.items():
        lens = c[0][1:] - c[0][:-1]
        u = int(lens.argmax())
        b, e = int(c[0][u]), int(c[0][u + 1])
        longest[s] = e - b
        alone[s] = ((torch.tensor([0, e - b], device="cuda"), c[1][b:e].contiguous(), c[2][b:e].contiguous(), 1, c[4]),
                    x0[u:u + 1].clone(), u)
    tor = {}
    for s, (c, x0, fixed) in sides.items():
        tor[s] = (bl._csr_rows(c[0]), c[1].to(torch.int64), alpha * c[2])

    routes = {}
    for s in sides:
        routes[f"gram_{s}_fixed"] = lambda s=s: gram(s)
        routes[f"half_{s}"] = lambda s=s: (work[s].copy_(sides[s][1]), half(s))
        routes[f"copy_{s}"] = lambda s=s: work[s].copy_(sides[s][1])
        routes[f"longest_row_alone_{s}"] = lambda s=s: (alone[s][1].copy_(sides[s][1][alone[s][2]:alone[s][2] + 1]),
                                                        half(s, alone[s][0], alone[s][1]))
        routes[f"torch_half_{s}"] = lambda s=s: torch_half(*tor[s], sides[s][1], sides[s][2], G[s], STEPS)

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
           "cg_steps": STEPS, "rows_per_workgroup": int(L.pinsage_als_rows_per_block()),
           "long_row_above": int(L.pinsage_als_long_row())}
    for s, (c, x0, fixed) in sides.items():
        rows, nnz = int(c[3]), int(c[1].numel())
        ms = res[f"half_{s}"]["median_ms"] - res[f"copy_{s}"]["median_ms"]
        nbytes = (1 + STEPS) * nnz * f * 4 + rows * f * 8
        flops = (1 + STEPS) * (2 * f * f * rows + 4 * nnz * f)
        want = torch_half(*tor[s], x0, fixed, G[s], STEPS)
        work[s].copy_(x0)
        half(s)
        diff = float((work[s] - want).abs().max()) / float(want.abs().max())
        moved = float((want - x0).abs().max()) / float(want.abs().max())
        lens = c[0][1:] - c[0][:-1]
        res[f"half_{s}"].update({
            "rows": rows, "nnz": nnz, "longest_row": longest[s],
            "rows_by_workgroup": int((lens > int(L.pinsage_als_long_row())).sum()),
            "kernel_ms_less_copy": ms, "algorithmic_bytes": nbytes, "algorithmic_flops": flops,
            "GBps": nbytes / (ms * 1e-3) / 1e9, "GFLOPs": flops / (ms * 1e-3) / 1e9,
            "torch_over_kernel": res[f"torch_half_{s}"]["median_ms"] / ms,
            "longest_row_alone_over_launch": res[f"longest_row_alone_{s}"]["median_ms"] / ms,
            "max_diff_vs_torch_rel_to_largest": diff, "largest_entry": float(want.abs().max()),
            "largest_change_rel_to_largest": moved})

    fit = bl.ALS(factors=f, cg_steps=STEPS)
    fts = []
    for i in range(a.fit_reps + 1):
        t = timed(lambda: fit.fit(ct, user_factors=X0, item_factors=Y0))
        if i:
            fts.append(t)
    res["fit_15_iterations"] = _spread(fts)
    res["fit_15_iterations"]["loss"] = fit.loss()
    out["routes"] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
