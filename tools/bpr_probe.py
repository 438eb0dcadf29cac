"""The BPR kernels (csrc/bpr.hip) on the C2 graph's collection-track matrix
(25 000 collections x 100 000 tracks):

    python tools/bpr_probe.py [--factors 128] [--negatives 1] [--reps 10] [--scale 1.0]

One JSON line per stage, each timed with HIP events after a warm-up and a
synchronise:
  (a) pinsage_bpr_sample over the users' rows, in samples per second;
  (b) pinsage_bpr_apply on the user half's entries of that draw;
  (c) the torch plumbing of the item half (the stable sort and the gathers);
  (d) one whole iteration of BPR.fit (both halves, kernels and plumbing), from
      an event recorded after every iteration: the figure a fused user half
      would have to beat.
Nothing is gated; the figures go into DESIGN.md by hand.
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
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1], "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, default=128)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="rehearsal only: scale the graph")
    a = ap.parse_args()

    import torch

    import baselines as bl
    import bench
    import graph
    import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("bpr_probe needs the GPU: nothing is measured without one")
    cfg = bench.CONFIGS["c2"]
    n, nc, mem = (int(cfg[key] * a.scale) for key in ("n_tracks", "n_cols", "memberships"))
    indptr, indices = synthetic.make_playlist_graph_device(n, nc, mem, seed=0, device="cuda")
    R = bl.to_col_track_matrix(graph.DeviceCSRGraph(indptr, indices), range(n))
    ptr, idx, _, n_users, n_items = R
    S, f = a.negatives, a.factors

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

    say(stage="matrix", users=n_users, items=n_items, cells=int(idx.numel()),
        longest_row=int((ptr[1:] - ptr[:-1]).max()), negatives=S, factors=f)

    m = bl.BPR(factors=f, negatives=S, iterations=0, random_state=1).fit(R)
    X, Y, b = m.user_factors, m.item_factors, m.item_bias
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    r = timed(lambda: m._sample(0, X, Y, b, err), a.reps)
    say(stage="sample", samples=int(idx.numel()) * S, samples_per_second=int(idx.numel()) * S / (r["median_ms"] * 1e-3),
        **r)

    neg, w = m._sample(0, X, Y, b, err)
    pos = idx.to(torch.int64).repeat_interleave(S)
    usr = bl._csr_rows(ptr).repeat_interleave(S).to(torch.int32)
    j = torch.where(neg >= 0, neg.to(torch.int64), pos)
    idx_u = torch.stack([pos, j], 1).to(torch.int32).contiguous()
    val_u = torch.stack([w, -w], 1).contiguous()
    Hx = torch.zeros_like(X)
    r = timed(lambda: m._apply(ptr * (2 * S), idx_u, val_u, n_users, Y, n_items, X.clone(), None, Hx, None, err),
              a.reps)
    say(stage="apply_user_half", entries=int(idx_u.numel()), void=int((neg < 0).sum()), **r)

    def item_plumbing():
        ok = neg >= 0
        key = torch.cat([pos, neg[ok].to(torch.int64)])
        order = torch.sort(key, stable=True).indices
        return (bl._csr_ptr(key, n_items), torch.cat([usr, usr[ok]])[order].contiguous(),
                torch.cat([w, -w[ok]])[order].contiguous())
    say(stage="item_half_plumbing", **timed(item_plumbing, a.reps))

    # BPR.fit itself: an event after every iteration; the first (the read of the error word) is dropped
    marks = []

    def mark(it, model):
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
    fit = bl.BPR(factors=f, negatives=S, iterations=a.reps + 2, random_state=1).fit(R, callback=mark)
    torch.cuda.synchronize()
    say(stage="iteration", **_spread([p.elapsed_time(q) for p, q in zip(marks[1:-1], marks[2:])]))
    assert int(err) == 0 and bool(torch.isfinite(fit.item_factors).all())


if __name__ == "__main__":
    main()
