"""The GAT aggregator's kernels (csrc/gnns.hip, pinsage_gat_*) against the MEAN
aggregator's pinsage_segment_wmean on the same CSR: the same row gather is the
floor of both.

    python tools/gat_bench.py [--n 100000] [--d 128] [--segments 8192] [--degree 40] [--hubs 10] [--reps 25]

A random CSR (segment lengths Poisson around --degree, --hubs segments of 5000
entries, rows uniform over --n, c = sqrt of a count in 1..4), timed with device
events after a warm-up, the routes alternating, --inner launches per timed
window (the median and the spread of --reps windows).  Prints one JSON line:
per route the time per call, and for the forward the achieved GB/s against the
bytes model  nnz (4 d + 12) + F 4 d  (row gather, hrow + c + p per entry, the
output rows) and the ratio to segment_wmean.  Nothing is gated on the numbers.
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
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--segments", type=int, default=8192)
    ap.add_argument("--degree", type=int, default=40)
    ap.add_argument("--hubs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")

    import numpy as np
    import torch

    import _native as nat
    import gnns
    if not torch.cuda.is_available():
        raise SystemExit("gat_bench needs the GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    n_h, d, F = a.n, a.d, a.segments
    counts = rng.poisson(a.degree, F)
    counts[rng.choice(F, a.hubs, replace=False)] = 5000
    seg = np.zeros(F + 1, np.int64)
    np.cumsum(counts, out=seg[1:])
    nnz = int(seg[-1])
    hrows = rng.integers(0, n_h, nnz)
    own = rng.integers(0, n_h, F)
    c = np.sqrt(rng.integers(1, 5, nnz).astype(np.float32))
    plan = gnns.gat_plan(seg, hrows, own, n_h)

    def dev(x, dtype):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()

    g = torch.Generator(device="cuda").manual_seed(0)
    h = torch.randn((n_h, d), device="cuda", generator=g)
    att = (torch.randn(2 * d, device="cuda", generator=g) / (2 * d) ** 0.5).contiguous()
    dout = torch.randn((F, d), device="cuda", generator=g)
    seg_t, hrow_t, c_t, own_t = dev(seg, np.int64), dev(hrows, np.int32), dev(c, np.float32), dev(own, np.int32)
    rows_u, segT, entT, segofT, own_ptr, own_seg = (dev(x, x.dtype) for x in plan)
    n_rows = rows_u.numel()
    L = nat.lib()
    f32 = dict(dtype=torch.float32, device="cuda")
    s_l, s_r = torch.empty(n_h, **f32), torch.empty(n_h, **f32)
    out, out_mean = torch.empty((F, d), **f32), torch.empty((F, d), **f32)
    p, de, s = torch.empty(nnz, **f32), torch.empty(nnz, **f32), torch.empty(F, **f32)
    dh, coef = torch.zeros((n_h, d), **f32), torch.empty(2 * n_rows, **f32)
    partial = torch.empty((int(L.pinsage_gat_partial_rows(n_rows)), 2 * d), **f32)
    da = torch.empty(2 * d, **f32)
    st = nat.stream_ptr

    def route_scores():
        nat.check(L.pinsage_gat_node_scores(nat.ptr(h), d, n_h, d, nat.ptr(att), nat.ptr(rows_u), n_rows,
                                            nat.ptr(s_l), nat.ptr(s_r), st()), "gat_node_scores")

    def route_forward():
        nat.check(L.pinsage_gat_forward(nat.ptr(h), d, n_h, d, nat.ptr(seg_t), nat.ptr(hrow_t), nat.ptr(c_t),
                                        nat.ptr(own_t), F, nnz, nat.ptr(s_l), nat.ptr(s_r), nat.ptr(out), d,
                                        nat.ptr(p), st()), "gat_forward")

    def route_edges():
        nat.check(L.pinsage_gat_backward_edges(nat.ptr(h), d, n_h, d, nat.ptr(seg_t), nat.ptr(hrow_t), nat.ptr(c_t),
                                               nat.ptr(own_t), F, nnz, nat.ptr(s_l), nat.ptr(s_r), nat.ptr(p),
                                               nat.ptr(dout), d, nat.ptr(de), nat.ptr(s), st()), "gat_backward_edges")

    def route_rows():
        nat.check(L.pinsage_gat_backward_rows(nat.ptr(h), d, n_h, d, nat.ptr(att), nat.ptr(rows_u), n_rows,
                                              nat.ptr(segT), nat.ptr(entT), nat.ptr(segofT), nat.ptr(own_ptr),
                                              nat.ptr(own_seg), nat.ptr(p), nat.ptr(de), nat.ptr(s), nnz, F,
                                              nat.ptr(dout), d, nat.ptr(dh), d, nat.ptr(coef), nat.ptr(partial),
                                              nat.ptr(da), st()), "gat_backward_rows")

    def route_wmean():
        nat.check(L.pinsage_segment_wmean(nat.ptr(h), d, n_h, d, nat.ptr(seg_t), nat.ptr(hrow_t), nat.ptr(c_t), F, 1,
                                          nat.ptr(out_mean), d, st()), "segment_wmean")

    routes = {"gat_node_scores": route_scores, "gat_forward": route_forward, "gat_backward_edges": route_edges,
              "gat_backward_rows": route_rows, "segment_wmean": route_wmean}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for _ in range(3):  # warm-up: code objects; the routes run in their data order
        for fn in routes.values():
            timed(fn)
    ts = {name: [] for name in routes}
    for _ in range(a.reps):  # alternating: a drift of the machine falls on every route
        for name, fn in routes.items():
            ts[name].append(timed(fn))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dh).all()) and bool(torch.isfinite(da).all())
    res = {name: _spread(v) for name, v in ts.items()}
    fwd_bytes = nnz * (4 * d + 12) + F * 4 * d
    mean_bytes = nnz * (4 * d + 8) + F * 4 * d
    fwd_ms = res["gat_forward"]["median_ms"]
    res["gat_forward"]["model_GBps"] = fwd_bytes / (fwd_ms * 1e-3) / 1e9
    res["segment_wmean"]["model_GBps"] = mean_bytes / (res["segment_wmean"]["median_ms"] * 1e-3) / 1e9
    bwd_ms = res["gat_backward_edges"]["median_ms"] + res["gat_backward_rows"]["median_ms"]
    print(json.dumps({
        "metric": "device events, ms per call", "n_h": n_h, "d": d, "segments": F, "nnz": nnz, "rows_touched": n_rows,
        "inner": a.inner, "routes": res, "forward_bytes_model": fwd_bytes,
        "forward_with_scores_ms": fwd_ms + res["gat_node_scores"]["median_ms"], "backward_ms": bwd_ms,
        "forward_over_wmean": fwd_ms / res["segment_wmean"]["median_ms"],
        "backward_over_wmean": bwd_ms / res["segment_wmean"]["median_ms"]}), flush=True)


if __name__ == "__main__":
    main()
