"""The early-stop sampler restated in numpy (tests/test_earlystop_host.py checks
it against the reference's fixtures and a plain loop; tests/test_gpu_earlystop.py
checks the device against it).

sample_neighborhood_topt_early_stop (pinsage_model.py:55-86) ends a source's
walk at the hop where the np-th node reaches nv visits.  The stop only
truncates: with t the full-length trace from the same stream position,

  * hop j is an event if t[j] is the nv-th occurrence of its id in t[0..j]
    (visits to the source itself count);
  * with np >= 1 and at least np events, the walk has L = j* + 1 hops, j* the
    np-th event in hop order; otherwise L = n_hops;
  * the weights are the visit counts of t[:L] over L (float64), the source's
    column zeroed, and the top k is taken over n_items columns;
  * a stopped source consumes 3 L - 1 generator words (the break comes before
    that hop's torch.rand), an unstopped one 3 n_hops.

Oracle traces -> L -> sampler_util.runs_from_trace(t[:L]) -> dense rows with
divisor L -> oracle.topk -> sampler_util.norm_pair.  Nothing comes from the
device.
"""
import numpy as np

import sampler_util as su


def stop_length(trace, stop_np, stop_nv):
    """(L, stopped) of one full-length trace: occurrence ranks by a stable sort
    of (id, hop), the events' hops, the cut at the np-th of them."""
    t = np.asarray(trace, np.int64).reshape(-1)
    n = len(t)
    if stop_np < 1 or stop_nv < 1:
        return n, False
    order = np.lexsort((np.arange(n), t))          # by id, hops ascending inside an id
    ts = t[order]
    first = np.concatenate([[True], ts[1:] != ts[:-1]])
    run_start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    rank = np.arange(n) - run_start
    ev = np.sort(order[rank == stop_nv - 1])
    if len(ev) >= stop_np:
        return int(ev[stop_np - 1]) + 1, True
    return n, False


def words_consumed(L, stopped, n_hops):
    return 3 * L - 1 if stopped else 3 * n_hops


def walk_lengths(indptr, indices, sources, n_hops, alpha, stop_np, stop_nv, mt=None, seed=0, offset=0, src_base=0):
    """(traces, L int32 [n], stopped bool [n], words): the full-length oracle
    trace of every source and its cut.  mt (an oracle.MT): the chain -- every
    source starts where the one before stopped, and mt is left where the
    reference leaves the generator.  Without mt: Philox position src_base + i."""
    from oracle import oracle as orc
    traces, Ls, stops = [], [], []
    words = 0
    for i, s in enumerate(np.asarray(sources, np.int64)):
        if mt is None:
            t = orc.walk_philox(indptr, indices, [s], n_hops, alpha, seed, offset, src_base + i)[0]
        else:
            before = mt.buf.copy()
            t = orc.walk_mt(indptr, indices, [s], n_hops, alpha, mt)[0]
        L, stopped = stop_length(t, stop_np, stop_nv)
        if mt is not None:
            mt.buf[:] = before
            mt.draws(words_consumed(L, stopped, n_hops))
            words += words_consumed(L, stopped, n_hops)
        traces.append(t)
        Ls.append(L)
        stops.append(stopped)
    return traces, np.array(Ls, np.int32), np.array(stops, bool), words


def reference(indptr, indices, n_items, sources, n_hops, alpha, k, stop_np, stop_nv, t_norm=0, mt=None, seed=0,
              offset=0, src_base=0):
    """dict(w f64 [n][k], nb i64 [n][k], wn f32 / nb32 i32 [n][t_norm] (None
    without t_norm), hops i32 [n], stopped, words)."""
    from oracle import oracle as orc
    sources = np.asarray(sources, np.int64)
    traces, Ls, stops, words = walk_lengths(indptr, indices, sources, n_hops, alpha, stop_np, stop_nv, mt=mt,
                                            seed=seed, offset=offset, src_base=src_base)
    n = len(sources)
    dense = np.zeros((n, n_items), np.float64)
    for i in range(n):
        L = int(Ls[i])
        dense[i] = su.dense_from_runs(su.runs_from_trace(traces[i][:L], sources[i]), n_items, L)
    w, nb = orc.topk(dense, k) if n else (np.zeros((0, k)), np.zeros((0, k), np.int64))
    wn = nb32 = None
    if t_norm:
        wn, nb32 = su.norm_pair(w, nb, t_norm)
    return dict(w=w, nb=nb, wn=wn, nb32=nb32, hops=Ls, stopped=stops, words=words)
