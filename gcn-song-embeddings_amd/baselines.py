"""The GPU paths of the reference's evaluation side that sit next to the
PinSage train step: personalised-PageRank
neighbours (``PersPageRank``, baselines.py:106-151) on the walk + top-k
kernels, and cosine k-nearest neighbours over an embedding table
(``cosine_sim_ab`` / ``knn_from_emb``, baselines.py:69-103) with the
``save_knn`` / ``load_knn`` cache format of eval.py:112-149; and the accuracy
metrics that consume them (``hit_rate`` / ``mrr`` / ``low_degree_accuracy``,
eval.py:227-250 and :376-389), both over a kNN id matrix and over the ranks of
the held-out positives, which ``rank_from_emb`` counts on the GPU without
building any list; and the beyond-accuracy metrics of eval.py:255-374 and
:445-467 (intra- and inter-list diversity, coverage, average degree) over a
kNN id matrix, the two diversities on the kernels of csrc/listmetrics.hip.

``JaccardFast`` (baselines.py:194-220), the co-occurrence baseline, runs on the
kernels of csrc/cooc.hip: count rows of the playlist-track product per batch of
queries (never the n x n product), scored and selected by the cosine path's
selection kernel under a Jaccard key.  With it, ``Random`` (baselines.py:
380-397), ``low_co_accuracy`` (eval.py:391-406), ``LazyKnnDict`` (eval.py:
177-215) and ``compute_results_table`` (eval.py:413-443) the reference's main
results table is produced from this package.

``ColTrackCF`` / ``TrackTrackCF`` (baselines.py:458-514) factorise the
collection-track and the track-track matrix by implicit-feedback ALS.  The
reference takes the fit from the ``implicit`` package; here ``ALS`` is this
package's own (csrc/als.hip: a Gram kernel and a conjugate-gradient
half-iteration), defined in its docstring, and ``similar_items`` is the cosine
kNN above.  ``ColTrackLMF`` / ``TrackTrackLMF`` are the same two classes with
the fit the reference selects by algo="lmf": ``LMF``, logistic matrix
factorisation by full-gradient AdaGrad ascent (csrc/lmf.hip: a fused
sigmoid(X Y^T) Y MFMA kernel and a sparse update), again this package's own
definition.  ``ColTrackBPR`` / ``TrackTrackBPR`` are the same two classes with
the fit the reference selects by any other algo: ``BPR``, Bayesian personalised
ranking with negatives from the counter-based Philox generator and Jacobi
AdaGrad half-iterations (csrc/bpr.hip: a sample kernel and a signed gathered
row update), this package's own definition and deterministic; implicit's
sampled SGD with racing updates is not reproduced, and the quality of the
defaults on real data is unmeasured.

``FastNode2Vec`` (baselines.py:223-255) stands on ``Node2Vec``: second-order
(p, q) walks by rejection sampling on the counter-based Philox generator and a
skip-gram fit with the negatives taken in expectation, a closed objective over
the walks' window co-occurrence counts that runs on the LMF scaffold
(csrc/n2v.hip: a walk kernel, the column-weighted form of the fused dense
kernel and a sparse update).  Again this package's own definition,
deterministic, with no parity with fastnode2vec or gensim claimed.

``SimpleSimilarity`` and its ``JaccardIndex`` / ``AdamicAdar`` /
``Preferential`` (baselines.py:153-191, one networkx call per pair there) score
a query against all tracks at once: Adamic-Adar on the weighted form of the
count kernel (64-bit fixed-point sums, csrc/cooc.hip) and the selection kernel
under a score key, the Jaccard coefficient on the Jaccard path above, and
preferential attachment from one sort of the degrees.  ``JaccardIndex`` computes
the Jaccard coefficient, not the preferential attachment the reference assigns
to that name.

``GraphSAGE`` (baselines.py:517-544, standing on lib/gnns) stands on ``SAGE``:
unsupervised two-layer GraphSAGE with the MEAN aggregator, Floyd neighbour
samples, walk positives and one-hop-excluded negatives on the Philox generator
and the min / max cosine margin loss (csrc/sage.hip: a sampler, a negative
draw and a loss kernel; the dense work on the GEMM, the segmented weighted mean
and the Adam kernel).  The reference class cannot run as written, so this is
again this package's own definition, deterministic, with no reference numbers;
the quality of the defaults on real data is unmeasured.

Implicit's own sampled-SGD order for bpr and the GAT / GCN variants of the
reference's GNN library are out of scope; their libraries are not part of this
build.  Names, signatures, return types and RNG consumption
follow the reference; compute runs in HIP (no CPU fallback).
"""
from __future__ import annotations

import os
import time
from abc import ABC, abstractmethod

import torch

import _native as nat
import pinsage_model as psm

PRECOMP_K = 1000  # eval.py:31
# dot products of one batch of query rows live in this much device scratch
KNN_SCRATCH_BYTES = int(os.environ.get("PINSAGE_KNN_SCRATCH_MB", "2048")) << 20


class PredictionModel(ABC):
    """Base recommender class (baselines.py:33-46)."""

    @abstractmethod
    def __init__(self):
        pass

    @abstractmethod
    def train(self, g, ids, train_set, test_set, features):
        pass

    @abstractmethod
    def knn(self, nodeset, k):
        pass


class EmbeddingModel(PredictionModel):
    """An embedding-based recommender (baselines.py:48-53)."""

    @abstractmethod
    def embed(self, nodeset):
        pass


def cosine_sim_ab(a, b, eps=1e-16):
    """Pairwise cosine similarities [len(a), len(b)] (baselines.py:69-77), on the
    inputs' device with the reference's formula dot / (|a| |b|^T + eps)."""
    dot_prod = torch.mm(a, b.transpose(1, 0))
    lengths_mat = torch.mm(torch.norm(a, dim=1).unsqueeze(1), torch.norm(b, dim=1).unsqueeze(0))
    return dot_prod / (lengths_mat + eps)


def _batch_rows(nq, n):
    """How many of nq query rows, n scores each, one batch holds in KNN_SCRATCH_BYTES (read now)."""
    return max(1, min(nq, (KNN_SCRATCH_BYTES - 8 * n) // max(1, 4 * n)))


def _knn_cosine(emb, q, k_total, eps=1e-16):
    """Top-k_total cosine neighbours of rows q of emb (HIP: MFMA dot products +
    per-row radix select), sorted descending: (w f32 [nq, k], n i64 [nq, k])."""
    nat.require_gpu()
    e = torch.as_tensor(emb)
    out_dev = e.device
    e = e.to(device="cuda", dtype=torch.float32).contiguous()
    qs = torch.as_tensor(q).reshape(-1).to(torch.int64).contiguous()
    n, d = int(e.shape[0]), int(e.shape[1])
    if qs.numel() and (int(qs.min()) < 0 or int(qs.max()) >= n):
        raise IndexError(f"knn: query ids out of range for {n} rows")
    if d % 4:  # the MFMA GEMM loads 16-byte row chunks: zero columns change no dot product
        e = torch.nn.functional.pad(e, (0, 4 - d % 4))
        d = int(e.shape[1])
    qd = qs.to("cuda")
    nq = int(qd.numel())
    w = torch.empty((nq, k_total), dtype=torch.float32, device="cuda")
    nb = torch.empty((nq, k_total), dtype=torch.int64, device="cuda")
    L = nat.lib()
    nbytes = L.pinsage_knn_scratch_bytes(n, _batch_rows(nq, n))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    nat.check(L.pinsage_knn_cosine(nat.ptr(e), n, d, d, nat.ptr(qd), nq, int(k_total), float(eps),
                                   nat.ptr(scratch), nbytes, nat.ptr(w), nat.ptr(nb),
                                   nat.stream_ptr()), "knn_cosine")
    return w.to(out_dev), nb.to(out_dev)


def knn_from_emb(emb, q, k, sim_func=None):
    """k nearest neighbours of the nodes q by cosine similarity of their
    embeddings (baselines.py:91-103): top k+1 per query, first column dropped
    (the reference assumes it is the query itself).  ``sim_func`` is accepted
    and ignored, as in the reference (cosine_sim_ab is always used)."""
    w, nb = _knn_cosine(emb, q, int(k) + 1)
    return w[:, 1:], nb[:, 1:]


RANK_MAX_GROUP = 4096  # kRankMaxGroup (csrc/knn.hip): targets one query row may own


def _group_pairs(queries, targets):
    """Group (query, target) pairs by query for pinsage_rank_cosine, on the
    inputs' device (CPU tensors work too):
    (rows int64 [nu], grp_ptr CPU int64 [nu + 1], targets_sorted int64 [np], order int64 [np]).
    Row u is query rows[u] and owns targets_sorted[grp_ptr[u]:grp_ptr[u + 1]];
    a query with more than RANK_MAX_GROUP pairs is repeated over several rows.
    Sorted pair i is the caller's pair order[i] (a stable sort: pairs of one
    query keep their order), so ``out[order] = sorted_result`` restores it."""
    uq, inv, counts = torch.unique(queries, return_inverse=True, return_counts=True)
    order = torch.sort(inv, stable=True).indices
    cap = int(RANK_MAX_GROUP)
    counts = counts.cpu()
    pieces = (counts + cap - 1) // cap
    sizes = torch.full((int(pieces.sum()),), cap, dtype=torch.int64)
    if sizes.numel():
        sizes[torch.cumsum(pieces, 0) - 1] = counts - (pieces - 1) * cap  # a query's last row: the rest
    grp_ptr = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
    torch.cumsum(sizes, 0, out=grp_ptr[1:])
    rows = torch.repeat_interleave(uq, pieces.to(uq.device))
    return rows.contiguous(), grp_ptr, targets[order].contiguous(), order


def rank_from_emb(emb, queries, targets, eps=1e-16):
    """For parallel id tensors (the two columns of ``test_positives``): the
    rank of row targets[i] among all rows of emb by cosine similarity to row
    queries[i], int64 [len(queries)] on emb's device, in the order
    ``knn_from_emb`` documents (similarity descending, index ascending): the
    number of rows that come before the target.  ``_knn_cosine``'s column r for
    that query holds the target exactly when rank == r, so ``knn_from_emb``'s
    (which drops column 0) holds it at 1-based position rank.  HIP: dot
    products of the distinct queries only and one counting pass per row; no
    selection, no sort, no k-wide result."""
    nat.require_gpu()
    e = torch.as_tensor(emb)
    out_dev = e.device
    e = e.to(device="cuda", dtype=torch.float32).contiguous()
    qs = torch.as_tensor(queries).reshape(-1).to(torch.int64)
    ts = torch.as_tensor(targets).reshape(-1).to(torch.int64)
    if qs.numel() != ts.numel():
        raise ValueError(f"rank: {qs.numel()} queries for {ts.numel()} targets")
    n, d = int(e.shape[0]), int(e.shape[1])
    for name, v in (("query", qs), ("target", ts)):
        if v.numel() and (int(v.min()) < 0 or int(v.max()) >= n):
            raise IndexError(f"rank: {name} ids out of range for {n} rows")
    npairs = int(qs.numel())
    if npairs == 0:
        return torch.empty(0, dtype=torch.int64, device=out_dev)
    if d % 4:  # the MFMA GEMM loads 16-byte row chunks: zero columns change no dot product
        e = torch.nn.functional.pad(e, (0, 4 - d % 4))
        d = int(e.shape[1])
    rows_q, grp_ptr, tsorted, order = _group_pairs(qs.to("cuda"), ts.to("cuda"))
    nu = int(rows_q.numel())
    out = torch.empty(npairs, dtype=torch.int64, device="cuda")
    L = nat.lib()
    nbytes = L.pinsage_rank_scratch_bytes(n, _batch_rows(nu, n))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    nat.check(L.pinsage_rank_cosine(nat.ptr(e), n, d, d, nat.ptr(rows_q), nu, nat.ptr(grp_ptr),
                                    nat.ptr(tsorted), npairs, float(eps), nat.ptr(scratch), nbytes,
                                    nat.ptr(out), nat.stream_ptr()), "rank_cosine")
    ranks = torch.empty_like(out)
    ranks[order] = out
    return ranks.to(out_dev)


# ----------------------------------------------------------------------------- accuracy metrics
# eval.py:227-250 and :376-389, vectorised.  The matrix forms take the id
# matrix of knn_from_emb / load_knn ([n_nodes, list_len], column 0 of the top
# list already dropped); the rank forms take rank_from_emb's ranks of the same
# pairs: a positive is among the first K columns iff 1 <= rank <= min(K,
# list_len), at 1-based position rank (rank 0 is the column knn_from_emb drops
# as "the query itself": a miss, as in the reference).
_METRIC_CHUNK = 1 << 16  # pairs whose list rows are compared at once


def _pairs(test_positives):
    return torch.as_tensor(test_positives).to(torch.int64).reshape(-1, 2)


def _positions(knn_mat, test_positives, K):
    """1-based position of each pair's positive in knn_mat[q, :K], 0 if absent."""
    km = torch.as_tensor(knn_mat)
    tp = _pairs(test_positives).to(km.device)
    out = torch.zeros(tp.shape[0], dtype=torch.int64, device=km.device)
    for i in range(0, tp.shape[0], _METRIC_CHUNK):
        c = tp[i:i + _METRIC_CHUNK]
        eq = km[c[:, 0], :K] == c[:, 1:2]
        if eq.shape[1]:
            out[i:i + _METRIC_CHUNK] = torch.where(eq.any(1), eq.to(torch.int8).argmax(1) + 1, 0)
    return out


def _positions_from_ranks(ranks, K, list_len):
    r = torch.as_tensor(ranks).to(torch.int64).reshape(-1)
    return torch.where((r >= 1) & (r <= min(int(K), int(list_len))), r, 0)


def _hit_rate(pos):
    return int((pos > 0).sum()) / int(pos.numel())


def _mrr(pos, K, scaling):
    # a miss counts as position K (eval.py:248); summed in float64
    rank_pos = torch.where(pos > 0, pos, int(K)).to(torch.float64)
    return float((1.0 / (rank_pos / scaling)).sum()) / int(pos.numel())


def hit_rate(knn_mat, test_positives, K):
    """eval.py:227-238: the share of pairs (q, pos) with pos in knn_mat[q, :K]."""
    return _hit_rate(_positions(knn_mat, test_positives, K))


def mrr(knn_mat, test_positives, K, scaling=1):
    """eval.py:240-250: mean of scaling / (1-based position of pos in knn_mat[q, :K]),
    a miss counting as position K."""
    return _mrr(_positions(knn_mat, test_positives, K), K, scaling)


def hit_rate_from_ranks(ranks, K, list_len=PRECOMP_K):
    """``hit_rate`` of a list_len-wide knn_from_emb matrix, from rank_from_emb's ranks."""
    return _hit_rate(_positions_from_ranks(ranks, K, list_len))


def mrr_from_ranks(ranks, K, scaling=1, list_len=PRECOMP_K):
    """``mrr`` of a list_len-wide knn_from_emb matrix, from rank_from_emb's ranks."""
    return _mrr(_positions_from_ranks(ranks, K, list_len), K, scaling)


def _low_degree_selection(g, test_positives, degree_thr, queries):
    """eval.py:379-385: which pairs have a query among the nodes whose
    in-degree is at most degree_thr (None: no such node)."""
    deg = torch.as_tensor(g.in_degrees(queries))
    sel = queries[deg <= degree_thr]
    if len(sel) == 0:
        return None
    return torch.isin(_pairs(test_positives)[:, 0].cpu(), sel)


def low_degree_accuracy(knn_mat, g, test_positives, K, degree_thr, acc_func, queries=None, track_ids=None):
    """eval.py:376-389: ``acc_func(knn_mat, pairs, K)`` (hit_rate or mrr) over the
    pairs whose query has in-degree <= degree_thr in g (a graph.CSRGraph, or
    anything answering ``in_degrees``); 0 if no node is that low."""
    if queries is None:
        queries = torch.arange(0, torch.as_tensor(knn_mat).shape[0], dtype=torch.int64)
    keep = _low_degree_selection(g, test_positives, degree_thr, queries)
    if keep is None:
        return 0
    return acc_func(knn_mat, _pairs(test_positives)[keep.to(_pairs(test_positives).device)], K)


def low_degree_accuracy_from_ranks(ranks, g, test_positives, K, degree_thr, acc_func, queries=None,
                                   n_nodes=None):
    """``low_degree_accuracy`` from rank_from_emb's ranks of test_positives:
    ``acc_func(ranks_of_the_kept_pairs, K)`` with hit_rate_from_ranks or
    mrr_from_ranks.  The candidate nodes are ``queries``, else all n_nodes
    (default: g.number_of_nodes()), the rows of the matrix form's knn_mat."""
    if queries is None:
        queries = torch.arange(0, g.number_of_nodes() if n_nodes is None else int(n_nodes), dtype=torch.int64)
    keep = _low_degree_selection(g, test_positives, degree_thr, queries)
    if keep is None:
        return 0
    r = torch.as_tensor(ranks).reshape(-1)
    return acc_func(r[keep.to(r.device)], K)


def _low_co_selection(test_positives, co_thr, queries, n_nodes):
    """eval.py:393-403: which pairs have a query among the candidate nodes with
    at most co_thr held-out pairs.  The reference sums the rows of a track-track
    matrix it builds from test_positives alone: that sum is the number of pairs
    the node is the query of."""
    tp = _pairs(test_positives).cpu()
    co_counts = torch.bincount(tp[:, 0], minlength=int(n_nodes))[queries]
    return torch.isin(tp[:, 0], queries[co_counts <= co_thr])


def low_co_accuracy(knn_mat, g, test_positives, K, co_thr, acc_func, queries=None, track_ids=None):
    """eval.py:391-406: ``acc_func(knn_mat, pairs, K)`` (hit_rate or mrr) over the
    pairs whose query occurs as a query in at most co_thr pairs of
    test_positives.  ``g`` and ``track_ids`` are accepted and unused, as in the
    reference.  If no pair is kept acc_func divides by zero, as in the reference."""
    n = int(torch.as_tensor(knn_mat).shape[0])
    if queries is None:
        queries = torch.arange(0, n, dtype=torch.int64)
    keep = _low_co_selection(test_positives, co_thr, queries, n)
    return acc_func(knn_mat, _pairs(test_positives)[keep.to(_pairs(test_positives).device)], K)


def low_co_accuracy_from_ranks(ranks, test_positives, K, co_thr, acc_func, queries=None, n_nodes=None):
    """``low_co_accuracy`` from rank_from_emb's ranks of test_positives:
    ``acc_func(ranks_of_the_kept_pairs, K)`` with hit_rate_from_ranks or
    mrr_from_ranks.  The candidate nodes are ``queries``, else all n_nodes
    (default: one more than the largest id in test_positives)."""
    tp = _pairs(test_positives)
    if n_nodes is None:
        n_nodes = int(tp.max()) + 1 if tp.numel() else 0
    if queries is None:
        queries = torch.arange(0, int(n_nodes), dtype=torch.int64)
    keep = _low_co_selection(test_positives, co_thr, queries, n_nodes)
    r = torch.as_tensor(ranks).reshape(-1)
    return acc_func(r[keep.to(r.device)], K)


class LazyKnnDict:
    """eval.py:177-215: the saved kNN lists of several models, each loaded from
    its ``save_knn`` file when asked for.  Iterating yields the model names."""

    def __init__(self, model_names, ids, save_dir):
        self.all_nodes = torch.arange(0, len(ids), dtype=torch.int64)
        self.models = model_names
        self.save_dir = save_dir
        self.idx = 0
        self.times = {m_name: None for m_name in model_names}

    def __getitem__(self, m_name):
        tup = load_knn(m_name, self.all_nodes, self.save_dir)
        return tup[0], tup[1].to(torch.int64)

    def get_times(self, m_name):
        """(train, embed, knn) seconds of the model's file; zeros for a file
        saved without them."""
        if not self.times[m_name]:
            tpl = load_knn(m_name, self.all_nodes, self.save_dir)
            self.times[m_name] = tuple(tpl[2:5]) if len(tpl) == 5 else (0, 0, 0)
        return self.times[m_name]

    def __len__(self):
        return len(self.models)

    def __iter__(self):
        self.idx = 0
        return self

    def __next__(self):
        if self.idx >= len(self):
            raise StopIteration
        self.idx += 1
        return self.models[self.idx - 1]


def compute_results_table(knn_dict, test_positives, g, times=True, degree_thr=1):
    """eval.py:413-443: the accuracy metrics of every model of knn_dict (a
    LazyKnnDict, or any mapping name -> (weights, id matrix) that also answers
    ``get_times`` when ``times`` is set) as a pandas.DataFrame with the
    reference's columns in the reference's order."""
    import pandas as pd
    results = {}
    for model in knn_dict:
        _, knn_mat = knn_dict[model]
        row = {f"hr (k={k})": hit_rate(knn_mat, test_positives, k) for k in (10, 100, 500)}
        row["mrr"] = mrr(knn_mat, test_positives, 1000, 1)
        row["low-degree accuracy"] = low_degree_accuracy(knn_mat, g, test_positives, 1000, degree_thr=degree_thr,
                                                         acc_func=mrr)
        row["low-co accuracy"] = low_co_accuracy(knn_mat, g, test_positives, 1000, co_thr=1, acc_func=mrr)
        if times:
            row["t (train)"], row["t (emb)"], row["t (knn)"] = knn_dict.get_times(model)
        results[model] = row
    return pd.DataFrame.from_dict(results, orient="index")


# ----------------------------------------------------------------------------- beyond-accuracy metrics
# eval.py:271-374 and :445-467.  knn_mat is the id matrix of knn_from_emb /
# load_knn ([n queries, list_len]), on any device and of any integer dtype;
# test_positives is accepted where the reference accepts it (only coverage with
# all_nodes=False reads it).  Results are Python floats, as in the reference.
LIST_OVERLAP_MAX_K = 4096  # kOvMaxK (csrc/listmetrics.hip): columns one pair of lists may compare


def _lists(knn_mat):
    """The id matrix as a contiguous int64 [n, list_len] tensor on the GPU."""
    nat.require_gpu()
    km = torch.as_tensor(knn_mat)
    if km.dim() != 2:
        raise ValueError(f"knn_mat must be [n, list_len], got {tuple(km.shape)}")
    return km.to(device="cuda", dtype=torch.int64).contiguous()


def _list_width(km, K):
    kc = min(int(K), int(km.shape[1]))  # K above the list length: the whole list (a slice, in the reference)
    if kc < 1:
        raise ValueError(f"K = {K} over lists of {int(km.shape[1])} columns leaves nothing to measure")
    return kc


def _intra_sims(km, kc, features):
    """float32 [n] on the GPU: per query the mean of the kc x kc cosine matrix of
    its first kc recommended feature rows (HIP: inverse row norms, then one
    gather-and-accumulate wave per query)."""
    f = torch.as_tensor(features).to(device="cuda", dtype=torch.float32).contiguous()
    if f.dim() != 2:
        raise ValueError(f"features must be [N, d], got {tuple(f.shape)}")
    n, d = int(f.shape[0]), int(f.shape[1])
    nq, ldk = int(km.shape[0]), int(km.shape[1])
    inv = torch.empty(n, dtype=torch.float32, device="cuda")
    out = torch.empty(nq, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = nat.lib()
    nat.check(L.pinsage_row_inv_norms(nat.ptr(f), n, d, d, nat.ptr(inv), nat.stream_ptr()), "row_inv_norms")
    nat.check(L.pinsage_list_intra_sim(nat.ptr(f), n, d, d, nat.ptr(inv), nat.ptr(km), nq, ldk, kc, nat.ptr(out),
                                       nat.ptr(err), nat.stream_ptr()), "list_intra_sim")
    if int(err):
        raise IndexError(f"intra_diversity: recommended ids out of range for {n} feature rows")
    return out


def intra_diversity(knn_mat, test_positives, K, features):
    """eval.py:271-286: 1 - the mean over queries of the mean cosine similarity
    among the feature rows of knn_mat[q, :K] (the K x K matrix with its diagonal;
    a repeated id counts as often as it is listed).  A recommended row of zeros
    makes the result NaN, as in the reference.  The per-query values are fp32
    from the kernel, their mean is taken in float64."""
    km = _lists(knn_mat)
    sims = _intra_sims(km, _list_width(km, K), features)
    return 1 - float(sims.to(torch.float64).mean())


def _pair_overlaps(km, kc, N, pairs):
    """int32 [n_pairs, 3] (CPU numpy): |set(A)|, |set(B)|, |set(A) & set(B)| of the
    first kc columns of the two rows of each pair (HIP)."""
    if kc > LIST_OVERLAP_MAX_K:
        raise ValueError(f"inter_diversity: K = {kc} above the kernel's capacity of {LIST_OVERLAP_MAX_K} columns")
    if not 1 <= int(N) < 2 ** 31:
        raise ValueError(f"inter_diversity: N = {N} ids do not fit 32 bits")
    nq, ldk = int(km.shape[0]), int(km.shape[1])
    pr = torch.as_tensor(pairs).to(torch.int64).reshape(-1, 2)
    if pr.numel() and (int(pr.min()) < 0 or int(pr.max()) >= nq):
        raise IndexError(f"inter_diversity: pair rows out of range for {nq} lists")
    pr = pr.to("cuda").contiguous()
    npairs = int(pr.shape[0])
    out = torch.empty((npairs, 3), dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nat.check(nat.lib().pinsage_list_pair_overlap(nat.ptr(km), nq, ldk, kc, int(N), nat.ptr(pr), npairs,
                                                  nat.ptr(out), nat.ptr(err), nat.stream_ptr()),
              "list_pair_overlap")
    if int(err):
        raise IndexError(f"inter_diversity: recommended ids out of range for N = {N}")
    return out.cpu().numpy()


def inter_diversity(knn_mat, test_positives, K, N, n_pairs=10000, pairs=None):
    """eval.py:288-312: the mean cosine distance between the one-hot images of
    knn_mat[a, :K] and knn_mat[b, :K] over sampled pairs of queries, i.e.
    1 - |A & B| / sqrt(|A| |B|) over the SETS of ids (a repeated id marks one
    column).  With ``pairs`` None the pairs are the reference's one draw,
    ``np.random.randint(0, n, (n_pairs, 2))`` from numpy's global generator;
    with ``pairs`` ([m, 2] rows of knn_mat) nothing is drawn.  The set sizes are
    integers from the kernel; distances and their mean are float64."""
    import numpy as np
    km = _lists(knn_mat)
    kc = _list_width(km, K)
    if pairs is None:
        pairs = np.random.randint(0, int(km.shape[0]), (int(n_pairs), 2))
    o = _pair_overlaps(km, kc, N, pairs).astype(np.float64)
    return float(np.mean(1.0 - o[:, 2] / np.sqrt(o[:, 0] * o[:, 1])))


def coverage(knn_mat, test_positives, K=500, all_nodes=True, queries=None):
    """eval.py:342-355: distinct ids in columns 1 .. K of knn_mat (the reference
    skips column 0 here) over the number of queries, knn_mat.shape[0] or the
    distinct count of ``queries`` (the reference's ``if not queries`` raises on a
    tensor; this is its evident intent).  all_nodes=False counts the distinct
    ids of test_positives instead."""
    km = _lists(knn_mat)
    if all_nodes:
        recs = km[:, 1:int(K) + 1].flatten()
    else:
        recs = torch.as_tensor(test_positives).to(device="cuda", dtype=torch.int64).flatten()
    denom = int(km.shape[0]) if queries is None else int(torch.unique(torch.as_tensor(queries)).numel())
    return int(torch.unique(recs).numel()) / denom


def _rec_degrees(knn_mat, g, K):
    """(in-degree of each distinct id in knn_mat[:, :K], how often the id is
    listed, number of listed slots): int64 on the GPU.  g answers
    ``in_degrees(ids)`` (graph.CSRGraph or a stand-in) once per distinct id."""
    km = _lists(knn_mat)
    recs = km[:, :int(K)].flatten()
    ids, counts = torch.unique(recs, return_counts=True)
    deg = torch.as_tensor(g.in_degrees(ids.cpu())).to(device="cuda", dtype=torch.int64)
    return deg, counts, int(recs.numel())


def average_degree(knn_mat, g, test_positives, K, queries=None):
    """eval.py:357-364: the mean in-degree in g over all slots of knn_mat[:, :K]
    (an exact integer sum, divided once)."""
    deg, counts, slots = _rec_degrees(knn_mat, g, K)
    return int((deg * counts).sum()) / slots if slots else float("nan")


def degree_dist(knn_mat, g, test_positives, K, queries=None):
    """eval.py:366-374: (sorted distinct in-degrees, how many slots of
    knn_mat[:, :K] hold a node of that degree), int64 tensors on knn_mat's device."""
    deg, counts, _ = _rec_degrees(knn_mat, g, K)
    vals, inverse = torch.unique(deg, sorted=True, return_inverse=True)
    hist = torch.zeros(vals.numel(), dtype=torch.int64, device=vals.device).index_add_(0, inverse, counts)
    dev = torch.as_tensor(knn_mat).device
    return vals.to(dev), hist.to(dev)


def beyond_accuracy(knn_mat, g, features, k=100, n_pairs=10000, pairs=None):
    """One model's row of compute_beyond_accuracy_table (eval.py:457-461) as a
    dict with the reference's keys.  Draws from numpy's generator unless
    ``pairs`` is given (see inter_diversity)."""
    km = _lists(knn_mat)
    n_feat = int(torch.as_tensor(features).shape[0])
    return {
        "intra diversity": intra_diversity(km, None, k, features),
        "inter diversity": inter_diversity(km, None, k, n_feat, n_pairs=n_pairs, pairs=pairs),
        "coverage": coverage(km, None, K=k),
        "average degree": average_degree(km, g, None, k),
    }


def compute_beyond_accuracy_table(knn_dict, test_positives, g, features):
    """eval.py:445-467: the beyond-accuracy metrics at k = 100 of every model of
    knn_dict ({name: (weights, id matrix)}) as a pandas.DataFrame."""
    import pandas as pd
    results = {}
    for model in knn_dict:
        _, knn_mat = knn_dict[model]
        results[model] = beyond_accuracy(knn_mat, g, features, k=100)
    return pd.DataFrame.from_dict(results, orient="index")


class PersPageRank(PredictionModel):
    """Nearest graph neighbours via PPR aka random walks with restarts
    (baselines.py:106-151): 1000 hops, restart 0.85; the walk consumes torch's
    generator exactly like the reference loop (pinsage_model's MT19937 mode)."""

    def __init__(self):
        self.n_hops = 1000
        self.alpha = 0.85

    def visit_prob(self, g, nodeset, n_hops, alpha):
        """Dense f64 visit probabilities [len(nodeset), N_all], self column zeroed."""
        return psm.sample_neighborhood(g, None, nodeset, n_hops, alpha)

    def train(self, g, ids, train_set, test_set, features):
        self.g = g

    def knn(self, nodeset, k):
        """visit_prob(...).topk(k, 1) without the dense matrix (walk + top-k kernels)."""
        return psm.sample_neighborhood_topt(self.g, None, nodeset, self.n_hops, self.alpha, k)


def _csr_ptr(rows, n_rows):
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    torch.cumsum(torch.bincount(rows, minlength=n_rows), 0, out=ptr[1:])
    return ptr


def _membership_pairs(g, n_tracks, dev, who):
    """(track, collection - n_tracks) of every stored edge of g with exactly one
    track endpoint, int64 on dev, duplicates kept: nodes [0, n_tracks) are
    tracks, the rest collections.  An edge between two tracks is dropped, one
    between two collections raises ValueError."""
    n_cols = len(g) - n_tracks
    if n_tracks < 1 or n_cols < 0:
        raise ValueError(f"{who}: {n_tracks} tracks in a graph of {len(g)} nodes")
    dev = torch.device(dev)
    if dev.type == "cpu":  # leaves g's device mirror alone
        indptr, indices = torch.as_tensor(g.indptr), torch.as_tensor(g.indices)
    else:
        indptr, indices = g.device_csr(dev)
    src = torch.repeat_interleave(torch.arange(len(g), dtype=torch.int64, device=dev), indptr[1:] - indptr[:-1])
    dst = indices.to(torch.int64)
    s_tr, d_tr = src < n_tracks, dst < n_tracks
    if bool((~s_tr & ~d_tr).any()):
        raise ValueError(f"{who}: an edge joins two collections")
    keep = s_tr ^ d_tr
    return torch.where(s_tr, src, dst)[keep], torch.where(s_tr, dst, src)[keep] - n_tracks


def _membership_csrs(g, n_tracks, who):
    """The two membership CSRs on the GPU, duplicates removed and rows ascending:
    ((ptr, idx int32) tracks -> collections, (ptr, idx int32) collections ->
    tracks, n_cols).  Membership is _membership_pairs' rule."""
    n_cols = len(g) - n_tracks
    track, col = _membership_pairs(g, n_tracks, nat.device(), who)
    # one 64-bit key per membership: unique() removes duplicates and sorts the rows
    tc = torch.unique(track * max(n_cols, 1) + col)
    ct = torch.unique(col * n_tracks + track)
    t2c = (_csr_ptr(tc // max(n_cols, 1), n_tracks), (tc % max(n_cols, 1)).to(torch.int32).contiguous())
    c2t = (_csr_ptr(ct // n_tracks, n_cols), (ct % n_tracks).to(torch.int32).contiguous())
    return t2c, c2t, n_cols


def _track_queries(nodeset, n, who):
    """nodeset as contiguous int64 query ids on the GPU; IndexError outside [0, n)."""
    qs = torch.as_tensor(nodeset).reshape(-1).to(torch.int64)
    if qs.numel() and (int(qs.min()) < 0 or int(qs.max()) >= n):
        raise IndexError(f"{who}: query ids out of range for {n} tracks")
    return qs.to("cuda").contiguous()


def _cooc_lists(entry, scratch_bytes, csr_args, n, qd, k, who):
    """The k best of each query under one of the list entries of csrc/cooc.hip
    (pinsage_cooc_jaccard / pinsage_cooc_weighted_knn; csr_args ends where the
    queries begin): (float32 [nq, k], int64 [nq, k]) on the GPU, sorted (score
    descending, id ascending)."""
    nq, k = int(qd.numel()), int(k)
    w = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    nb = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    if nq:
        L = nat.lib()
        nbytes = getattr(L, scratch_bytes)(n, _batch_rows(nq, n))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        nat.check(getattr(L, entry)(*csr_args, nat.ptr(qd), nq, k, nat.ptr(scratch), nbytes, nat.ptr(w), nat.ptr(nb),
                                    nat.ptr(err), nat.stream_ptr()), entry[len("pinsage_"):])
        if int(err):
            raise IndexError(f"{who}: query ids out of range for {n} tracks")
    return w, nb


class JaccardFast(PredictionModel):
    """Nearest neighbours by the Jaccard similarity of the tracks' collection
    sets (baselines.py:194-220):  |C(q) & C(t)| / (|C(q) | C(t)| + 1e-10).

    The reference forms the n_tracks x n_tracks product of the collection-track
    matrix with its transpose in scipy and densifies rows of it per query batch
    on the host.  Here ``train`` builds the two membership CSRs on the GPU once
    and ``knn`` counts, scores and selects per batch of queries in HIP
    (csrc/cooc.hip + the selection kernel of csrc/knn.hip); nothing n x n exists.

    Scores equal the reference's bit for bit.  The ORDER among equal scores is
    documented here (score descending, then id ascending; a list with fewer than
    k non-zero scores is filled with the lowest zero-score ids), while the
    reference's is whatever ``torch.topk`` does: on the 300-track graph of
    tests/golden/jaccard.npz (a hub, duplicate edges, tracks in no collection)
    6 % of the id cells coincide at k = 50.  Column 0, which ``knn`` drops as the
    reference does, is the query itself only where no track of a lower id has
    the same collection set and the query is in a collection at all (53 % of the
    rows of that graph)."""

    def __init__(self):
        pass

    def train(self, g, ids, train_set, test_set, features):
        """Nodes [0, len(ids)) of g are tracks, the rest collections.  Every edge
        with exactly one track endpoint is a membership, whichever way it points
        and however often it is stored (the reference takes the set
        successors | predecessors per collection); an edge between two tracks is
        ignored, one between two collections raises ValueError (the reference's
        matrix assignment raises on the column index)."""
        nat.require_gpu()
        self.ids = ids
        self.n = n_tracks = len(ids)
        self._t2c, self._c2t, self.n_cols = _membership_csrs(g, n_tracks, "JaccardFast")
        self.nbh_sizes = self._t2c[0][1:] - self._t2c[0][:-1]  # int64 [n_tracks], on the GPU

    def _queries(self, nodeset):
        return _track_queries(nodeset, self.n, "JaccardFast")

    def _csr_args(self):
        return (nat.ptr(self._t2c[0]), nat.ptr(self._t2c[1]), nat.ptr(self._c2t[0]), nat.ptr(self._c2t[1]),
                self.n, self.n_cols)

    def intersect_sizes(self, nodeset):
        """Rows ``nodeset`` of the reference's ``intersect_sizes`` matrix, dense:
        int32 [len(nodeset), n_tracks] on the GPU."""
        qd = self._queries(nodeset)
        nq = int(qd.numel())
        out = torch.empty((nq, self.n), dtype=torch.int32, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        nat.check(nat.lib().pinsage_cooc_counts(*self._csr_args(), nat.ptr(qd), nq, nat.ptr(out), nat.ptr(err),
                                                nat.stream_ptr()), "cooc_counts")
        if int(err):
            raise IndexError(f"JaccardFast: query ids out of range for {self.n} tracks")
        return out

    def knn(self, nodeset, k):
        """The reference's ``torch.topk(scores, k)`` with column 0 dropped:
        (float32 [nq, k - 1], int64 [nq, k - 1]) on nodeset's device, k - 1
        columns (not k, as knn_from_emb returns)."""
        out_dev = torch.as_tensor(nodeset).device
        w, nb = _cooc_lists("pinsage_cooc_jaccard", "pinsage_cooc_scratch_bytes", self._csr_args(), self.n,
                            self._queries(nodeset), k, "JaccardFast")
        return w[:, 1:].to(out_dev), nb[:, 1:].to(out_dev)


# ----------------------------------------------------------------------------- implicit-feedback ALS
# baselines.py:400-426 and :458-514.  A sparse matrix is the tuple
# (ptr int64 [n_rows + 1], idx int32, val float32, n_rows, n_cols), rows with
# ascending column ids and no cell twice, on the GPU unless ``device`` says
# otherwise (the builders and als_loss are plain torch and run anywhere).
ALS_MAX_FACTORS = LMF_MAX_FACTORS = 128  # kRowMaxF (csrc/rowplan.h)


def to_col_track_matrix(g, ids, device=None):
    """baselines.py:402-413: collections x tracks, 1 where the collection holds
    the track.  Membership is JaccardFast.train's rule (the reference's set
    successors | predecessors per collection): every edge with exactly one track
    endpoint, whichever way it points and however often it is stored; an edge
    between two tracks is ignored, one between two collections raises ValueError."""
    n_tracks = len(ids)
    n_cols = len(g) - n_tracks
    dev = nat.device() if device is None else torch.device(device)
    track, col = _membership_pairs(g, n_tracks, dev, "to_col_track_matrix")
    ct = torch.unique(col * n_tracks + track)
    idx = (ct % n_tracks).to(torch.int32).contiguous()
    return (_csr_ptr(ct // n_tracks, n_cols), idx, torch.ones(idx.numel(), dtype=torch.float32, device=dev),
            n_cols, n_tracks)


def to_track_track_matrix(ids, positives, device=None):
    """baselines.py:415-426: n x n, cell (a, b) = how often the row (a, b) occurs
    in ``positives`` ([m, 2] ids).  Not symmetrised, as in the reference; a == b
    is a cell like any other.  An id outside [0, len(ids)) raises IndexError."""
    n = len(ids)
    dev = nat.device() if device is None else torch.device(device)
    tp = _pairs(positives).to(dev)
    if n < 1:
        raise ValueError("to_track_track_matrix: no tracks")
    if tp.numel() and (int(tp.min()) < 0 or int(tp.max()) >= n):
        raise IndexError(f"to_track_track_matrix: ids out of range for {n} tracks")
    key, counts = torch.unique(tp[:, 0] * n + tp[:, 1], return_counts=True)
    return (_csr_ptr(key // n, n), (key % n).to(torch.int32).contiguous(), counts.to(torch.float32), n, n)


def _csr_rows(ptr):
    n = int(ptr.numel()) - 1
    return torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=ptr.device), ptr[1:] - ptr[:-1])


def _csr_transpose(ptr, idx, val, n_rows, n_cols):
    """R^T as such a tuple: a stable sort by column keeps the rows ascending
    within a column.  An id out of range is clamped into [0, n_cols) (the
    kernels report it)."""
    col = idx.to(torch.int64).clamp(0, n_cols - 1)
    order = torch.sort(col, stable=True).indices
    return (_csr_ptr(col, n_cols), _csr_rows(ptr)[order].to(torch.int32).contiguous(), val[order].contiguous(),
            n_cols, n_rows)


_LMF_CELLS = 1 << 24  # dense cells of lmf_objective and sgns_objective formed at once


def _add_observed(total, ptr, idx, X, Y, term):
    """total + term(x.y, rows, columns, slice) over the stored cells, 2^20 of them at a time, in order."""
    rows = _csr_rows(ptr)
    for i in range(0, int(idx.numel()), 1 << 20):
        sl = slice(i, i + (1 << 20))
        r, j = rows[sl], idx[sl].to(torch.int64)
        total = total + term((X[r] * Y[j]).sum(1), r, j, sl)
    return total


def _sub_all_cells(total, X, Y, term):
    """total - term(X[rows] Y^T, rows) over ALL cells in row chunks of at most _LMF_CELLS cells, in order."""
    step = max(1, _LMF_CELLS // max(1, int(Y.shape[0])))
    for r0 in range(0, int(X.shape[0]), step):
        total = total - term(X[r0:r0 + step] @ Y.T, slice(r0, r0 + step))
    return total


class _RowFit:
    """What ALS, LMF, BPR and Node2Vec share: the factor tables, the intake of the
    matrix, the iteration loop and similar_items.  ``_who`` prefixes the error
    texts."""

    def __init__(self, factors, random_state):
        if not (4 <= int(factors) <= ALS_MAX_FACTORS and int(factors) % 4 == 0):
            raise ValueError(f"{self._who}: factors = {factors}: need a multiple of 4 in [4, {ALS_MAX_FACTORS}]")
        self.factors, self.random_state = int(factors), random_state
        self.user_factors = self.item_factors = None

    def _table(self, given, n, gen):
        f = self.factors
        if given is None:
            return ((torch.rand(n, f, generator=gen) - 0.5) / f).to("cuda")
        t = torch.as_tensor(given)
        if tuple(t.shape) != (n, f):
            raise ValueError(f"{self._who}: factors of shape {tuple(t.shape)}, expected {(n, f)}")
        return t.to(device="cuda", dtype=torch.float32, copy=True).contiguous()

    def _bias(self, given, n):
        if given is None:
            return torch.zeros(n, dtype=torch.float32, device="cuda")
        t = torch.as_tensor(given)
        if tuple(t.shape) != (n,):
            raise ValueError(f"{self._who}: a bias of shape {tuple(t.shape)}, expected {(n,)}")
        return t.to(device="cuda", dtype=torch.float32, copy=True).contiguous()

    def _csr_arrays(self, ptr, idx, val, n_rows):
        """The three arrays of a CSR on the GPU, checked to fit together."""
        ptr = torch.as_tensor(ptr).to(device="cuda", dtype=torch.int64).contiguous()
        idx = torch.as_tensor(idx).to(device="cuda", dtype=torch.int32).contiguous()
        val = torch.as_tensor(val).to(device="cuda", dtype=torch.float32).contiguous()
        if int(ptr.numel()) != n_rows + 1 or int(idx.numel()) != int(val.numel()):
            raise ValueError(f"{self._who}: the CSR arrays do not fit together")
        return ptr, idx, val

    def _tables(self, first, second, n_first, n_second):
        """The two factor tables, drawn in this order, and the zeroed device word
        that a half-iteration sets on a column id out of range."""
        gen = None if self.random_state is None else torch.Generator().manual_seed(int(self.random_state))
        return (self._table(first, n_first, gen), self._table(second, n_second, gen),
                torch.zeros(1, dtype=torch.int32, device="cuda"))

    def _intake(self, user_items, user_factors, item_factors):
        """(R, R^T, X, Y, err): the checked CSR on the GPU and its transpose, and
        what _tables returns, users first."""
        nat.require_gpu()
        ptr, idx, val, n_users, n_items = user_items
        n_users, n_items = int(n_users), int(n_items)
        if n_users < 1 or n_items < 1:
            raise ValueError(f"{self._who}: a {n_users} x {n_items} matrix")
        ptr, idx, val = self._csr_arrays(ptr, idx, val, n_users)
        if not bool((torch.isfinite(val) & (val > 0)).all()):
            raise ValueError(f"{self._who}: values must be finite and > 0")
        self._user_items = csr_u = (ptr, idx, val, n_users, n_items)
        return (csr_u, _csr_transpose(*csr_u)) + self._tables(user_factors, item_factors, n_users, n_items)

    def _iterate(self, first_half, second_half, err, tables, callback=None, bad_ids=None):
        """``iterations`` times first_half() then second_half(); the error word is
        read after the first first_half(), which has met every column id.
        ``tables`` (attribute name -> tensor) are set before every
        ``callback(iteration, self)`` and at the end."""
        for it in range(self.iterations):
            first_half()
            if it == 0 and int(err):
                raise IndexError(f"{self._who}: "
                                 + (bad_ids or f"item ids out of range for {self._user_items[4]} items"))
            second_half()
            if callback is not None:
                vars(self).update(tables)
                callback(it, self)
        vars(self).update(tables)
        return self

    def similar_items(self, ids, N=10):
        """(ids int64 [nq, N], scores float32 [nq, N]): the N items nearest to each
        of ``ids`` by cosine similarity of the f latent columns of the item
        factors, best first (the query itself comes first unless another item
        ties it), on the GPU.  Biases, where there are any, take no part."""
        w, nb = _knn_cosine(self.item_factors, ids, int(N))
        return nb, w


def als_loss(user_items, user_factors, item_factors, regularization, alpha=1.0):
    """The ALS objective  sum_observed c (1 - x.y)^2 + sum_unobserved (x.y)^2 +
    reg (|X|^2 + |Y|^2),  c = alpha r,  in float64 on the factors' device without
    the dense n_users x n_items matrix:  the sum of (x.y)^2 over ALL cells is
    sum((X^T X) * (Y^T Y)), and the observed cells replace their term."""
    ptr, idx, val = user_items[:3]
    X, Y = user_factors.to(torch.float64), item_factors.to(torch.float64)
    ptr, idx, val = ptr.to(X.device), idx.to(X.device), val.to(X.device)
    total = _add_observed(((X.T @ X) * (Y.T @ Y)).sum(), ptr, idx, X, Y, lambda s, r, j, sl:
                          (float(alpha) * val[sl].to(torch.float64) * (1 - s) ** 2 - s * s).sum())
    return float(total + float(regularization) * ((X * X).sum() + (Y * Y).sum()))


class ALS(_RowFit):
    """Implicit-feedback alternating least squares (Hu, Koren, Volinsky) with the
    conjugate-gradient row solve of Takacs et al., on the kernels of
    csrc/als.hip: what the reference takes from
    implicit.cpu.als.AlternatingLeastSquares (baselines.py:474, :503).  The
    arithmetic is THIS PROJECT'S DEFINITION; that package cannot be run here and
    no parity with its numbers is claimed.

    R [n_users, n_items] has values r > 0; the confidence of an observed cell is
    c = alpha r (used directly: its extra weight is c - 1), the preference 1.
    One iteration solves every user row from the item factors Y, then every
    item row from the new user factors X (R^T as the CSR).  A half-iteration
    forms G = Y^T Y + reg I once and runs, per row u over its items i,

        x = X[u];  r = -G x + sum_i (c - (c - 1)(y_i . x)) y_i;  p = r;  rs = r . r
        if rs < 1e-20: X[u] stays
        repeat cg_steps times:
            Ap = G p + sum_i (c - 1)(y_i . p) y_i
            a = rs / (p . Ap);  x += a p;  r -= a Ap;  rn = r . r
            if rn < 1e-20: break
            p = r + (rn / rs) p;  rs = rn
        X[u] = x

    in fp32.  Rows are independent (Jacobi) and the result depends on the inputs
    only.  A row without items follows the same recurrence (CG drives it towards
    0).  Initial factors: (torch.rand(n, f) - 0.5) / f on the host, users first,
    then items, from a torch.Generator seeded with ``random_state`` or, with
    None, from torch's global generator."""

    _who = "ALS"

    def __init__(self, factors=128, regularization=0.01, alpha=1.0, iterations=15, cg_steps=3, random_state=None):
        super().__init__(factors, random_state)
        if not (regularization > 0 and alpha > 0 and int(iterations) >= 0 and int(cg_steps) >= 0):
            raise ValueError("ALS: need regularization > 0, alpha > 0, iterations >= 0, cg_steps >= 0")
        self.regularization, self.alpha = float(regularization), float(alpha)
        self.iterations, self.cg_steps = int(iterations), int(cg_steps)

    def _half(self, csr, Y, X, G, err):
        ptr, idx, val, n_rows, n_other = csr
        L, f = nat.lib(), self.factors
        nat.check(L.pinsage_als_gram(nat.ptr(Y), n_other, f, f, self.regularization, nat.ptr(G), nat.stream_ptr()),
                  "als_gram")
        nat.check(L.pinsage_als_half(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n_rows, nat.ptr(Y), n_other, f,
                                     nat.ptr(X), f, f, nat.ptr(G), self.alpha, self.cg_steps, nat.ptr(err),
                                     nat.stream_ptr()), "als_half")

    def fit(self, user_items, user_factors=None, item_factors=None):
        """user_items: the (ptr, idx, val, n_users, n_items) CSR; the transpose is
        built here.  Values are checked once on the host to be finite and > 0
        (ValueError); a column id outside [0, n_items) raises IndexError.  Given
        factor tables are copied, not written."""
        csr_u, csr_i, X, Y, err = self._intake(user_items, user_factors, item_factors)
        G = torch.empty((self.factors, self.factors), dtype=torch.float32, device="cuda")
        return self._iterate(lambda: self._half(csr_u, Y, X, G, err), lambda: self._half(csr_i, X, Y, G, err), err,
                             {"user_factors": X, "item_factors": Y})

    def loss(self):
        """als_loss of the fitted factors (a Python float; monitoring and tests)."""
        return als_loss(self._user_items, self.user_factors, self.item_factors, self.regularization, self.alpha)


def _softplus64(s):
    return torch.clamp(s, min=0) + torch.log1p(torch.exp(-s.abs()))


def lmf_objective(user_items, user_factors, item_factors, user_bias, item_bias, regularization, alpha=1.0):
    """The LMF objective (to be maximised)

        L = sum_observed c s - sum_observed (1 + c) softplus(s) - sum_unobserved softplus(s)
            - (reg / 2)(|X|^2 + |Y|^2),     s = x.y + bx + by,  c = alpha r,

    in float64 on the factors' device.  The softplus sum over ALL cells runs in
    row chunks of at most 2^24 cells; an observed cell then adds c s - c softplus(s)."""
    ptr, idx, val = user_items[:3]
    X, Y = user_factors.to(torch.float64), item_factors.to(torch.float64)
    bx = torch.as_tensor(user_bias).to(device=X.device, dtype=torch.float64)
    by = torch.as_tensor(item_bias).to(device=X.device, dtype=torch.float64)
    ptr, idx, val = ptr.to(X.device), idx.to(X.device), val.to(X.device)

    def observed(s, r, j, sl):
        s = s + bx[r] + by[j]
        return (float(alpha) * val[sl].to(torch.float64) * (s - _softplus64(s))).sum()

    total = _sub_all_cells(torch.zeros((), dtype=torch.float64, device=X.device), X, Y,
                           lambda s, rows: _softplus64(s + bx[rows, None] + by[None, :]).sum())
    total = _add_observed(total, ptr, idx, X, Y, observed)
    return float(total - 0.5 * float(regularization) * ((X * X).sum() + (Y * Y).sum()))


class LMF(_RowFit):
    """Logistic matrix factorisation (Johnson, "Logistic Matrix Factorization for
    Implicit Feedback Data", 2014) on the kernels of csrc/lmf.hip: what the
    reference takes from implicit's LogisticMatrixFactorization with
    algo="lmf".  The arithmetic is THIS PROJECT'S DEFINITION, the paper's
    full-gradient AdaGrad ascent without that package's negative sampling; the
    package cannot be run here and no parity with its numbers is claimed.

    R [n_users, n_items] has values r > 0 and c = alpha r.  Tables X [n_users, f],
    Y [n_items, f], biases bx, by; the score is s_ui = x_u . y_i + bx_u + by_i.
    The objective to MAXIMISE is

        L = sum_observed c s - sum_observed (1 + c) softplus(s) - sum_unobserved softplus(s)
            - (reg / 2)(|X|^2 + |Y|^2)            (biases are not regularised)

    One iteration updates every user row from (Y, by), then every item row from
    the new (X, bx) with R^T as the CSR.  A half-iteration is Jacobi: every row
    reads the old tables only.  Per row u, in fp32:

        D    = sum_all i sig(s_ui) y_i          dsum = sum_all i sig(s_ui)
        w_i  = c_ui sig(-s_ui)  for observed i        (= c (1 - sig(s)), no cancellation)
        g    = sum_obs w_i y_i - D - reg x_u    gb = sum_obs w_i - dsum
        h   += g^2 (elementwise)                hb += gb^2     (AdaGrad, start at 0)
        x_u += lr g / sqrt(1e-6 + h)            bx_u += lr gb / sqrt(1e-6 + hb)

    sig is evaluated stably (1 / (1 + e^-s) for s >= 0, e^s / (1 + e^s) otherwise).
    The dense terms D, dsum come from one fused MFMA kernel (pinsage_lmf_dense:
    no n_users x n_items buffer), the rest from pinsage_lmf_update.  The result
    depends on the inputs only.  Initial factors: (torch.rand(n, f) - 0.5) / f on
    the host, users first, then items, from a torch.Generator seeded with
    ``random_state`` or, with None, from torch's global generator; biases and
    accumulators start at zero."""

    _who = "LMF"

    def __init__(self, factors=128, learning_rate=0.1, regularization=0.6, alpha=1.0, iterations=30,
                 random_state=None):
        super().__init__(factors, random_state)
        if not (0 <= regularization < float("inf") and 0 < alpha < float("inf")
                and 0 <= learning_rate < float("inf") and int(iterations) >= 0):
            raise ValueError("LMF: need finite regularization >= 0, alpha > 0, learning_rate >= 0, iterations >= 0")
        self.learning_rate, self.regularization, self.alpha = float(learning_rate), float(regularization), float(alpha)
        self.iterations = int(iterations)
        self.user_bias = self.item_bias = None

    def _half(self, csr, Y, by, X, bx, H, hb, D, dsum, err):
        ptr, idx, val, n_rows, n_other = csr
        L, f = nat.lib(), self.factors
        nat.check(L.pinsage_lmf_dense(nat.ptr(X), nat.ptr(bx), n_rows, f, nat.ptr(Y), nat.ptr(by), n_other, f, f,
                                      nat.ptr(D), f, nat.ptr(dsum), nat.stream_ptr()), "lmf_dense")
        nat.check(L.pinsage_lmf_update(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n_rows, nat.ptr(Y), nat.ptr(by),
                                       n_other, f, nat.ptr(X), nat.ptr(bx), f, f, nat.ptr(D), f, nat.ptr(dsum),
                                       nat.ptr(H), f, nat.ptr(hb), self.alpha, self.regularization,
                                       self.learning_rate, nat.ptr(err), nat.stream_ptr()), "lmf_update")

    def fit(self, user_items, user_factors=None, item_factors=None, user_bias=None, item_bias=None, callback=None):
        """user_items: the (ptr, idx, val, n_users, n_items) CSR; the transpose is
        built here.  Values are checked once on the host to be finite and > 0
        (ValueError); a column id outside [0, n_items) raises IndexError.  Given
        factor and bias tables are copied, not written.  ``callback(iteration,
        self)`` runs after every iteration, the four tables set (monitoring)."""
        csr_u, csr_i, X, Y, err = self._intake(user_items, user_factors, item_factors)
        n_users, n_items = csr_u[3:]
        bx, by = self._bias(user_bias, n_users), self._bias(item_bias, n_items)
        Hx, Hy = torch.zeros_like(X), torch.zeros_like(Y)
        hbx, hby = torch.zeros_like(bx), torch.zeros_like(by)
        D = torch.empty((max(n_users, n_items), self.factors), dtype=torch.float32, device="cuda")
        dsum = torch.empty(max(n_users, n_items), dtype=torch.float32, device="cuda")
        return self._iterate(lambda: self._half(csr_u, Y, by, X, bx, Hx, hbx, D, dsum, err),
                             lambda: self._half(csr_i, X, bx, Y, by, Hy, hby, D, dsum, err), err,
                             {"user_factors": X, "item_factors": Y, "user_bias": bx, "item_bias": by}, callback)

    def objective(self):
        """lmf_objective of the fitted tables (a Python float; monitoring and tests)."""
        return lmf_objective(self._user_items, self.user_factors, self.item_factors, self.user_bias,
                             self.item_bias, self.regularization, self.alpha)


BPR_MAX_FACTORS = ALS_MAX_FACTORS
BPR_MAX_TRIES = 16     # pinsage_bpr_max_tries(): tries per sample before it is void
BPR_MAX_NEGATIVES = 8  # kBprMaxNeg (csrc/bpr.hip)


def bpr_objective(user_items, X, Y, b, neg, negatives, regularization):
    """The BPR objective of one draw (to be maximised)

        sum_t ln sig(z_t) - (reg / 2)(|X|^2 + |Y|^2)   over the non-void samples t,
        z_t = (x_u . y_i + b_i) - (x_u . y_j + b_j),   j = neg[t] >= 0,

    where sample t = e * negatives + s belongs to the e-th stored cell (u, i) of
    user_items.  In float64, plain torch, on the factors' device."""
    ptr, idx = user_items[:2]
    X, Y = X.to(torch.float64), Y.to(torch.float64)
    dev = X.device
    b = torch.as_tensor(b).to(device=dev, dtype=torch.float64)
    S = int(negatives)
    u = _csr_rows(ptr.to(dev)).repeat_interleave(S)
    i = idx.to(device=dev, dtype=torch.int64).repeat_interleave(S)
    j = torch.as_tensor(neg).to(device=dev, dtype=torch.int64).reshape(-1)
    if int(j.numel()) != int(i.numel()):
        raise ValueError(f"bpr_objective: {int(j.numel())} negatives for {int(i.numel())} samples")
    ok = j >= 0
    u, i, j = u[ok], i[ok], j[ok]
    z = (X[u] * (Y[i] - Y[j])).sum(1) + b[i] - b[j]
    return float(-_softplus64(-z).sum() - 0.5 * float(regularization) * ((X * X).sum() + (Y * Y).sum()))


class BPR(_RowFit):
    """Bayesian personalised ranking (Rendle, Freudenthaler, Gantner,
    Schmidt-Thieme, "BPR: Bayesian Personalized Ranking from Implicit Feedback",
    2009) on the kernels of csrc/bpr.hip: what the reference takes from
    implicit's BayesianPersonalizedRanking with algo="bpr".  The model is THIS
    PROJECT'S DEFINITION, deterministic and stated here in full: negatives from
    the counter-based Philox generator and Jacobi AdaGrad half-iterations, not
    that package's sampled SGD with racing updates, its popularity-proportional
    negatives or its per-step regularisation.  The package cannot be run here
    and no parity with its numbers is claimed; the quality of the defaults on
    real data is unmeasured.

    Inputs and tables.
    - R [n_users, n_items] is the usual CSR tuple.
    - Rows are strictly ascending.  ``fit`` checks this and raises ValueError
      otherwise, because the negative draw binary-searches the row.
    - Only R's structure is used.  Every stored cell is one positive; values
      pass the usual check (finite, > 0) and are otherwise ignored.
    - Tables: X [n_users, f], Y [n_items, f] and an item bias b [n_items].
      There is no user bias.
    - Cell e is the e-th stored cell of R.
    - Sample t = e * S + s, for s < S = ``negatives``.

    The draw.  For draw round rho, sample t of a cell (u, i), and tries
    k = 0 .. 15:

        (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (rho * 16 + k, t lo, t hi, offset))
        j = (uint64(r0) * n_items) >> 32
        accept the first j that is not a column of row u   (binary search; j == i is therefore rejected)

    - After 16 rejected tries the sample is void: neg[t] = -1, w[t] = 0.
    - Otherwise neg[t] = j.
    - With z = (x_u . y_i + b_i) - (x_u . y_j + b_j), set w[t] = sig(-z).
    - The dot is the row plan's: two columns per lane,
      fmaf(x.x, y.x, x.y * y.y), then the wave sum.  The sigmoid is LMF's.
    - neg and w of sample t depend on (seed, rho, offset, t, row u, the tables)
      only.  They do not depend on the grid or on batching.  ``fit`` uses
      offset 0.

    One iteration ``it``.
    - The user half uses draw round 2 it.
    - The item half uses round 2 it + 1 and the new X.
    - Both halves are Jacobi.
    - User half, row u, entries in ascending t, for each t (+w_t, y_i) then
      (-w_t, y_j).  A void sample contributes (+-0, y_i).
    - Item half, row i: first the samples whose positive is i, in ascending t,
      with (+w_t, x_u).  Then the non-void samples whose negative is i, in
      ascending t, with (-w_t, x_u).
    - Each half then runs, in fp32, per row:

        a = 0;  a = fma(val_e, row_e, a) over the entries in that order;   sv = sum of val_e
        g = fma(-reg, x, a);  h = fma(g, g, h);  x += lr g / sqrt(1e-6 + h)
        item half only:  gb = sv;  hb = fma(gb, gb, hb);  b += lr gb / sqrt(1e-6 + hb)      (bias not regularised, as in LMF)

    - The accumulators start at zero.
    - For a fixed draw this is ascent on
      sum_t ln sig(z_t) - (reg/2)(|X|^2 + |Y|^2) over non-void t.

    Between the two kernels (pinsage_bpr_sample, pinsage_bpr_apply) the entry
    arrays are plain torch: the user half's have a fixed structure (its ptr is
    R's times 2 S), the item half's CSR is built per iteration by one stable
    sort of cat(positive item of t, neg[valid]).

    Randomness.  The Philox seed is ``random_state`` or, with None, one
    ``torch.randint(0, 2**63 - 1, (1,))`` from torch's global generator, drawn
    before the tables.  Initial tables as LMF's: (torch.rand(n, f) - 0.5) / f,
    users first, then items; the bias and the accumulators start at zero."""

    _who = "BPR"

    def __init__(self, factors=128, learning_rate=0.05, regularization=0.01, iterations=100, negatives=1,
                 random_state=None):
        super().__init__(factors, random_state)
        if not (0 <= regularization < float("inf") and 0 <= learning_rate < float("inf") and int(iterations) >= 0):
            raise ValueError("BPR: need finite regularization >= 0, learning_rate >= 0, iterations >= 0")
        if not (negatives == int(negatives) and 1 <= int(negatives) <= BPR_MAX_NEGATIVES):
            raise ValueError(f"BPR: negatives = {negatives}: need an integer in [1, {BPR_MAX_NEGATIVES}]")
        if 2 * int(iterations) >= 1 << 27:
            raise ValueError("BPR: draw round 2 * iterations must stay below 2^27")
        self.learning_rate, self.regularization = float(learning_rate), float(regularization)
        self.iterations, self.negatives = int(iterations), int(negatives)
        self.item_bias = None

    def _sample(self, rho, X, Y, b, err):
        ptr, idx, _, n_users, n_items = self._user_items
        f, S = self.factors, self.negatives
        neg = torch.empty(int(idx.numel()) * S, dtype=torch.int32, device="cuda")
        w = torch.empty(int(idx.numel()) * S, dtype=torch.float32, device="cuda")
        nat.check(nat.lib().pinsage_bpr_sample(nat.ptr(ptr), nat.ptr(idx), n_users, 0, nat.ptr(X), f, nat.ptr(Y),
                                               nat.ptr(b), n_items, f, f, S, self._seed, int(rho), 0, nat.ptr(neg),
                                               nat.ptr(w), nat.ptr(err), nat.stream_ptr()), "bpr_sample")
        return neg, w

    def _apply(self, ptr, idx, val, n_rows, Y, n_other, X, bx, H, hb, err):
        f = self.factors
        nat.check(nat.lib().pinsage_bpr_apply(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n_rows, nat.ptr(Y), n_other, f,
                                              nat.ptr(X), nat.ptr(bx), f, f, nat.ptr(H), f, nat.ptr(hb),
                                              self.regularization,
                                              self.learning_rate, nat.ptr(err), nat.stream_ptr()), "bpr_apply")

    def sample(self, rho):
        """(neg int32 [nnz * negatives], w float32 [nnz * negatives]) on the GPU:
        draw round rho against the current tables (pinsage_bpr_sample)."""
        return self._sample(rho, self.user_factors, self.item_factors, self.item_bias,
                            torch.zeros(1, dtype=torch.int32, device="cuda"))

    def fit(self, user_items, user_factors=None, item_factors=None, item_bias=None, callback=None):
        """user_items: the (ptr, idx, val, n_users, n_items) CSR.  Values are
        checked once on the host to be finite and > 0 (ValueError) and rows to be
        strictly ascending (ValueError); a column id outside [0, n_items) raises
        IndexError.  Given factor and bias tables are copied, not written.
        ``callback(iteration, self)`` runs after every iteration, the three
        tables set (monitoring)."""
        nat.require_gpu()
        if self.random_state is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))
        else:
            seed = int(self.random_state) & (2 ** 64 - 1)
        csr_u, _, X, Y, err = self._intake(user_items, user_factors, item_factors)
        ptr, idx, _, n_users, n_items = csr_u
        rows = _csr_rows(ptr)
        if int(ptr[0]) != 0 or int(ptr[-1]) != int(idx.numel()) or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError("BPR: the CSR arrays do not fit together")
        if bool(((idx[1:] <= idx[:-1]) & (rows[1:] == rows[:-1])).any()):
            raise ValueError("BPR: rows must be strictly ascending (the negative draw binary-searches the row)")
        b = self._bias(item_bias, n_items)
        self._seed = seed
        S = self.negatives
        Hx, Hy, hb = torch.zeros_like(X), torch.zeros_like(Y), torch.zeros_like(b)
        pos = idx.to(torch.int64).clamp(0, n_items - 1).repeat_interleave(S)  # positive item of sample t
        usr = rows.repeat_interleave(S).to(torch.int32)                       # user of sample t
        ptr_u = ptr * (2 * S)
        state = {"it": 0}

        def user_half():
            neg, w = self._sample(2 * state["it"], X, Y, b, err)
            j = torch.where(neg >= 0, neg.to(torch.int64), pos)
            self._apply(ptr_u, torch.stack([pos, j], 1).to(torch.int32).contiguous(),
                        torch.stack([w, -w], 1).contiguous(), n_users, Y, n_items, X, None, Hx, None, err)

        def item_half():
            neg, w = self._sample(2 * state["it"] + 1, X, Y, b, err)
            ok = neg >= 0
            key = torch.cat([pos, neg[ok].to(torch.int64)])
            order = torch.sort(key, stable=True).indices
            self._apply(_csr_ptr(key, n_items), torch.cat([usr, usr[ok]])[order].contiguous(),
                        torch.cat([w, -w[ok]])[order].contiguous(), n_items, X, n_users, Y, b, Hy, hb, err)
            state["it"] += 1

        return self._iterate(user_half, item_half, err, {"user_factors": X, "item_factors": Y, "item_bias": b},
                             callback)

    def objective(self, neg=None):
        """bpr_objective of the fitted tables on the draw ``neg`` (a Python float;
        monitoring and tests).  By default the draw of round 2 * iterations,
        which the fit never uses."""
        if neg is None:
            neg = self.sample(2 * self.iterations)[0]
        return bpr_objective(self._user_items, self.user_factors, self.item_factors, self.item_bias, neg,
                             self.negatives, self.regularization)


class _CfModel(PredictionModel):
    """A factorisation baseline: ``train`` fits a ``_Fit`` (ALS, LMF or BPR) to the
    ``_matrix`` of the training data and leaves it in ``self.model``."""

    def train(self, g, ids, train_set, test_set, features):
        self.ids = ids
        self.n = len(ids)
        self.model = self._Fit(factors=self.factors)
        self.model.fit(self._matrix(g, ids, train_set))

    def knn(self, nodeset, k):
        """(scores float32 [nq, k], ids int64 [nq, k]) on nodeset's device:
        similar_items(nodeset, k + 1) with column 0 dropped, the tensors of
        knn_from_emb(self.model.item_factors, nodeset, k)."""
        out_dev = torch.as_tensor(nodeset).device
        topn_nodes, topn_scores = self.model.similar_items(nodeset, N=int(k) + 1)
        return topn_scores[:, 1:].to(out_dev), topn_nodes[:, 1:].to(out_dev)


class _CfALS(_CfModel):
    _Fit = ALS

    def __init__(self, algo="als", factors=128):
        if algo != "als":  # the reference's "lmf" and "bpr" come from implicit too
            raise NotImplementedError(f"algo = {algo!r}: ALS ('als') is the only algorithm of these classes; "
                                      "logistic MF is ColTrackLMF / TrackTrackLMF, BPR is ColTrackBPR / TrackTrackBPR")
        self.algo = algo
        self.factors = factors


class _CfLMF(_CfModel):
    _Fit = LMF

    def __init__(self, factors=128):
        self.algo = "lmf"
        self.factors = factors


class _CfBPR(_CfModel):
    _Fit = BPR

    def __init__(self, factors=128):
        self.algo = "bpr"
        self.factors = factors


class _TrackTrack:
    def _matrix(self, g, ids, train_set):
        return to_track_track_matrix(ids, train_set)


class _ColTrack:
    def _matrix(self, g, ids, train_set):
        return to_col_track_matrix(g, ids)


class TrackTrackCF(_TrackTrack, _CfALS):
    """Matrix factorisation of the track-track co-occurrence matrix of the
    training positives (baselines.py:458-487), by ALS."""


class ColTrackCF(_ColTrack, _CfALS):
    """Matrix factorisation of the collection-track membership matrix
    (baselines.py:489-514), by ALS."""


class TrackTrackLMF(_TrackTrack, _CfLMF):
    """TrackTrackCF with the fit replaced by logistic matrix factorisation
    (the reference's algo="lmf"; ``LMF`` above)."""


class ColTrackLMF(_ColTrack, _CfLMF):
    """ColTrackCF with the fit replaced by logistic matrix factorisation
    (the reference's algo="lmf"; ``LMF`` above)."""


class TrackTrackBPR(_TrackTrack, _CfBPR):
    """TrackTrackCF with the fit replaced by Bayesian personalised ranking
    (the reference's algo="bpr"; ``BPR`` above).  The counts of the track-track
    matrix are not used: every stored cell is one positive."""


class ColTrackBPR(_ColTrack, _CfBPR):
    """ColTrackCF with the fit replaced by Bayesian personalised ranking
    (the reference's algo="bpr"; ``BPR`` above)."""


# ----------------------------------------------------------------------------- node2vec
# baselines.py:223-255.  A graph is the tuple (ptr int64 [n + 1], idx int32,
# weight int64 or None, n): an undirected CSR, rows ascending, no duplicates, no
# self loops, positive integer weights (None: unweighted).
def project_bipartite_graph(g, ids):
    """The weighted track-track projection of the bipartite graph (the
    reference's project_bipartite_graph, networkx's weighted_projected_graph):
    (ptr, idx int32, weight int64, n) on the GPU, n = len(ids), the weight of
    (a, b) the number of collections that hold both, the diagonal dropped.
    Membership is JaccardFast.train's rule.  Built from batches of
    pinsage_cooc_counts rows: no n x n matrix exists at once."""
    nat.require_gpu()
    n = len(ids)
    t2c, c2t, n_cols = _membership_csrs(g, n, "project_bipartite_graph")
    L = nat.lib()
    step = _batch_rows(n, n)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lens, cols, wts = [], [], []
    for q0 in range(0, n, step):
        qd = torch.arange(q0, min(q0 + step, n), dtype=torch.int64, device="cuda")
        nq = int(qd.numel())
        out = torch.empty((nq, n), dtype=torch.int32, device="cuda")
        nat.check(L.pinsage_cooc_counts(nat.ptr(t2c[0]), nat.ptr(t2c[1]), nat.ptr(c2t[0]), nat.ptr(c2t[1]), n, n_cols,
                                        nat.ptr(qd), nq, nat.ptr(out), nat.ptr(err), nat.stream_ptr()), "cooc_counts")
        out[torch.arange(nq, device="cuda"), qd] = 0  # the diagonal: a track's own collection count
        r, c = torch.nonzero(out, as_tuple=True)   # row-major: rows ascending, columns ascending within a row
        lens.append(torch.bincount(r, minlength=nq))
        cols.append(c.to(torch.int32))
        wts.append(out[r, c].to(torch.int64))
    ptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(torch.cat(lens), 0, out=ptr[1:])
    return ptr, torch.cat(cols).contiguous(), torch.cat(wts).contiguous(), n


def bipartite_graph(g, ids):
    """The unweighted graph over tracks [0, len(ids)) and collections (the rest
    of g's nodes), symmetrised: (ptr, idx int32, None, len(g)) on the GPU, one
    edge each way per membership (JaccardFast.train's rule), however often and
    in whichever direction g stores it."""
    nat.require_gpu()
    n_tracks, n_all = len(ids), len(g)
    track, col = _membership_pairs(g, n_tracks, nat.device(), "bipartite_graph")
    col = col + n_tracks
    key = torch.unique(torch.cat([track * n_all + col, col * n_all + track]))
    return _csr_ptr(key // n_all, n_all), (key % n_all).to(torch.int32).contiguous(), None, n_all


def n2v_cooccurrence(walks, n, context, device=None):
    """The window co-occurrence counts of walks (int [n_walks, length], -1 past a
    walk's end): cell (a, b) counts the position pairs i != j of one walk with
    |i - j| <= context, walk[i] = a, walk[j] = b, both >= 0.  Every pair is
    counted in both orders, so the matrix is symmetric.  A sparse matrix tuple
    (ptr, idx int32, val float32, n, n) on ``device`` (default: the walks').
    Plain torch; the walks are taken in chunks whose keys fit KNN_SCRATCH_BYTES.
    A count of 2^24 or more is no longer exact in float32 and raises."""
    w = torch.as_tensor(walks)
    if w.dim() != 2:
        raise ValueError(f"n2v_cooccurrence: walks must be [n_walks, length], got {tuple(w.shape)}")
    n, context = int(n), int(context)
    if n < 1 or context < 1:
        raise ValueError(f"n2v_cooccurrence: n = {n}, context = {context}")
    dev = w.device if device is None else torch.device(device)
    w = w.to(device=dev, dtype=torch.int64)
    if w.numel() and int(w.max()) >= n:
        raise IndexError(f"n2v_cooccurrence: node ids out of range for {n} nodes")
    n_walks, length = int(w.shape[0]), int(w.shape[1])
    # per walk 2 * context * length keys of 8 bytes, and unique()'s sort works on copies of them
    step = max(1, KNN_SCRATCH_BYTES // max(1, 64 * context * length))
    keys = torch.empty(0, dtype=torch.int64, device=dev)
    counts = torch.empty(0, dtype=torch.int64, device=dev)
    for w0 in range(0, n_walks, step):
        c = w[w0:w0 + step]
        new = []
        for d in range(1, min(context, length - 1) + 1):
            a, b = c[:, :-d], c[:, d:]
            ok = (a >= 0) & (b >= 0)
            a, b = a[ok], b[ok]
            new += [a * n + b, b * n + a]
        if not new:
            continue
        k, cnt = torch.unique(torch.cat(new), return_counts=True)
        keys, inv = torch.unique(torch.cat([keys, k]), return_inverse=True)
        counts = torch.zeros(keys.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, torch.cat([counts, cnt]))
    if counts.numel() and int(counts.max()) >= 1 << 24:
        raise OverflowError("n2v_cooccurrence: a count reached 2^24 and is not exact in float32")
    return _csr_ptr(keys // n, n), (keys % n).to(torch.int32).contiguous(), counts.to(torch.float32), n, n


def sgns_objective(C, U, V, negative, noise, regularization):
    """The skip-gram objective with expected negatives (to be maximised)

        L = sum_wc C_wc log sig(u_w.v_c) + K sum_w #(w) sum_c P(c) log sig(-u_w.v_c)
            - (reg / 2)(|U|^2 + |V|^2),     #(w) = sum_c C_wc,  K = negative,  P = noise,

    in float64 on the tables' device.  The sum over ALL cells runs in row chunks
    of at most 2^24 cells."""
    ptr, idx, val = C[:3]
    U, V = U.to(torch.float64), V.to(torch.float64)
    dev = U.device
    ptr, idx, val = ptr.to(dev), idx.to(dev), val.to(device=dev, dtype=torch.float64)
    P = torch.as_tensor(noise).to(device=dev, dtype=torch.float64)
    cnt = torch.zeros(int(U.shape[0]), dtype=torch.float64, device=dev).index_add_(0, _csr_rows(ptr), val)
    total = _sub_all_cells(torch.zeros((), dtype=torch.float64, device=dev), U, V, lambda s, rows:
                           float(negative) * (cnt[rows, None] * (_softplus64(s) * P[None, :])).sum())
    total = _add_observed(total, ptr, idx, U, V, lambda s, r, j, sl: -(val[sl] * _softplus64(-s)).sum())
    return float(total - 0.5 * float(regularization) * ((U * U).sum() + (V * V).sum()))


def _graph_arrays(graph_csr, who):
    """(ptr, idx, weight or None, cum or None, n) of a graph tuple on the GPU,
    checked to fit together: cum holds per row the inclusive prefix sum of the
    weights (the walk kernel's form)."""
    ptr, idx, weight, n = graph_csr
    n = int(n)
    ptr = torch.as_tensor(ptr).to(device="cuda", dtype=torch.int64).contiguous()
    idx = torch.as_tensor(idx).to(device="cuda", dtype=torch.int32).contiguous()
    if n < 1 or int(ptr.numel()) != n + 1 or int(ptr[0]) != 0 or int(ptr[-1]) != int(idx.numel()) \
            or bool((ptr[1:] < ptr[:-1]).any()):
        raise ValueError(f"{who}: the CSR arrays do not fit together")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError(f"{who}: neighbour ids out of range for {n} nodes")
    wt = cum = None
    if weight is not None:
        wt = torch.as_tensor(weight).to(device="cuda", dtype=torch.int64).contiguous()
        if int(wt.numel()) != int(idx.numel()) or (wt.numel() and int(wt.min()) < 1):
            raise ValueError(f"{who}: weights must be positive integers, one per edge")
        run = torch.cumsum(wt, 0)
        before = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), run])[ptr[:-1]]
        cum = (run - torch.repeat_interleave(before, ptr[1:] - ptr[:-1])).contiguous()
    return ptr, idx, wt, cum, n


N2V_MAX_BIAS_RATIO = 16.0  # the walk kernel's bound on max(1/p, 1, 1/q) / min(1/p, 1, 1/q)


class Node2Vec(_RowFit):
    """node2vec (Grover & Leskovec 2016) on the kernels of csrc/n2v.hip: what the
    reference takes from fastnode2vec (baselines.py:223-255).  The model is THIS
    PROJECT'S DEFINITION, deterministic and stated here in full; that package and
    gensim cannot be run here and no parity with their numbers is claimed.  There
    is no reduced window, no subsampling of frequent nodes, and the negatives are
    taken in expectation, not sampled.

    Walks.  The graph is an undirected CSR with positive integer edge weights
    (or none).  From every node v start ``walks_per_node`` walks of
    ``walk_length`` nodes; walk rho of node v has generator position rho n + v.
    Step 1 draws a neighbour by edge weight.  From step 2 on a neighbour x of
    the current node is drawn with probability proportional to weight * beta,
    beta = 1/p if x is the previous node, 1 if x is a neighbour of the previous
    node, 1/q otherwise, by rejection: propose by weight, accept with
    probability beta / max(1/p, 1, 1/q).  Draws are Philox4x32-10 words keyed by
    (seed; step * 256 + try, position) and the arithmetic is integer apart from
    one fp32 compare (pinsage_n2v_walk in include/pinsage_hip.h states it word
    for word), so the walks depend on (seed, graph) only.  A node without edges
    ends its walk.  max(1/p, 1, 1/q) / min(1/p, 1, 1/q) may not exceed 16.

    Counts.  C_ab = the number of position pairs i != j of one walk with
    |i - j| <= ``context`` that hold (a, b): ``n2v_cooccurrence``, symmetric.
    #(w) = sum_c C_wc;  P(c) = #(c)^ns_exponent / sum, in float64 on the host,
    rounded to fp32.

    Fit.  Tables U (centre, ``embedding``) and V (``context_factors``), both
    [n, dim], s_wc = u_w . v_c, no biases, K = ``negative``.  MAXIMISE

        L = sum_wc C_wc log sig(s_wc) + K sum_w #(w) sum_c P(c) log sig(-s_wc)
            - (reg / 2)(|U|^2 + |V|^2)

    which is the skip-gram objective with each pair's K sampled negatives
    replaced by their expectation under P.  One iteration updates every centre
    row from V, then every context row from the new U.  A half-iteration is
    Jacobi; per row w of X against Y, in fp32, AdaGrad accumulators from zero:

        D   = sum_all c cw_c sig(x_w . y_c) y_c
        g   = sum_obs C_wc sig(-(x_w . y_c)) y_c - rw_w D - reg x_w
        h  += g^2 (elementwise);   x_w += lr g / sqrt(1e-6 + h)

    with (cw, rw) = (P, K #) for the centre half and (K #, P) for the context
    half.  D comes from one fused MFMA kernel (pinsage_sgns_dense: no n x n
    buffer, O(n^2 dim) work per half-iteration, the scaling limit LMF has), the
    rest from pinsage_sgns_update.

    Randomness.  The Philox seed is ``random_state`` or, with None, one
    ``torch.randint(0, 2**63 - 1, (1,))`` from torch's global generator, drawn
    before the tables.  Initial tables: (torch.rand(n, dim) - 0.5) / dim on the
    host, U first, then V, from a torch.Generator seeded with ``random_state``
    or, with None, from the global generator."""

    _who = "Node2Vec"

    def __init__(self, dim=128, walk_length=20, context=10, p=2.0, q=0.5, walks_per_node=10, negative=5,
                 ns_exponent=0.75, learning_rate=0.1, regularization=0.0, iterations=30, random_state=None):
        super().__init__(dim, random_state)
        inf = float("inf")
        if not (1 <= int(walk_length) < 1 << 24 and int(context) >= 1 and int(walks_per_node) >= 1):
            raise ValueError("Node2Vec: need 1 <= walk_length < 2^24, context >= 1, walks_per_node >= 1")
        if not (0 < p < inf and 0 < q < inf):
            raise ValueError("Node2Vec: p and q must be positive and finite")
        betas = (1.0 / p, 1.0, 1.0 / q)
        if max(betas) / min(betas) > N2V_MAX_BIAS_RATIO:
            raise ValueError(f"Node2Vec: max(1/p, 1, 1/q) / min(1/p, 1, 1/q) above {N2V_MAX_BIAS_RATIO:g}")
        if not (0 < negative < inf and 0 <= ns_exponent < inf and 0 <= learning_rate < inf
                and 0 <= regularization < inf and int(iterations) >= 0):
            raise ValueError("Node2Vec: need finite negative > 0, ns_exponent >= 0, learning_rate >= 0, "
                             "regularization >= 0, iterations >= 0")
        self.dim = self.factors
        self.walk_length, self.context, self.walks_per_node = int(walk_length), int(context), int(walks_per_node)
        self.p, self.q, self.negative, self.ns_exponent = float(p), float(q), float(negative), float(ns_exponent)
        self.learning_rate, self.regularization = float(learning_rate), float(regularization)
        self.iterations = int(iterations)
        self.embedding = self.context_factors = self.cooccurrence = self.noise = self.walks = None

    def _graph(self, graph_csr):
        ptr, idx, _, cum, n = _graph_arrays(graph_csr, "Node2Vec")
        return ptr, idx, cum, n

    def sample_walks(self, graph_csr, seed):
        """int32 [walks_per_node * n, walk_length] on the GPU: row rho n + v is walk
        rho of node v (pinsage_n2v_walk; -1 past a walk's end)."""
        nat.require_gpu()
        ptr, idx, cum, n = self._graph(graph_csr)
        starts = torch.arange(n, dtype=torch.int64, device="cuda").repeat(self.walks_per_node)
        walks = torch.empty((self.walks_per_node * n, self.walk_length), dtype=torch.int32, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        nat.check(nat.lib().pinsage_n2v_walk(nat.ptr(ptr), nat.ptr(idx), nat.ptr(cum), n, nat.ptr(starts),
                                             int(starts.numel()), self.walk_length, 1.0 / self.p, 1.0 / self.q,
                                             int(seed), 0, 0, nat.ptr(walks), nat.ptr(err), nat.stream_ptr()),
                  "n2v_walk")
        if int(err):
            raise IndexError(f"Node2Vec: node ids out of range for {n} nodes")
        return walks

    def _half(self, C, cw, rw, Y, X, H, D, err):
        ptr, idx, val, n = C[:4]
        L, f = nat.lib(), self.factors
        nat.check(L.pinsage_sgns_dense(nat.ptr(X), n, f, nat.ptr(Y), nat.ptr(cw), n, f, f, nat.ptr(D), f,
                                       nat.stream_ptr()), "sgns_dense")
        nat.check(L.pinsage_sgns_update(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), nat.ptr(rw), n, nat.ptr(Y), n, f,
                                        nat.ptr(X), f, f, nat.ptr(D), f, nat.ptr(H), f, self.regularization,
                                        self.learning_rate, nat.ptr(err), nat.stream_ptr()), "sgns_update")

    def fit(self, graph_csr, callback=None, cooccurrence=None, embedding=None, context_factors=None):
        """graph_csr: (ptr, idx, weight or None, n).  Sets ``embedding`` (U),
        ``context_factors`` (V), ``cooccurrence`` (C), ``noise`` (P) and
        ``walks``.  ``callback(iteration, self)`` runs after every iteration, the
        tables set (monitoring).  With ``cooccurrence`` (a matrix tuple as
        n2v_cooccurrence returns) no walk is sampled and graph_csr may be None;
        given tables are copied, not written."""
        nat.require_gpu()
        if self.random_state is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))
        else:
            seed = int(self.random_state) & (2 ** 64 - 1)
        if cooccurrence is None:
            self.walks = self.sample_walks(graph_csr, seed)
            n = int(graph_csr[3])
            C = n2v_cooccurrence(self.walks, n, self.context)
        else:
            n = int(cooccurrence[3])
            C = self._csr_arrays(*cooccurrence[:3], n) + (n, n)
        cnt = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, _csr_rows(C[0]), C[2].double()).cpu()
        if not float(cnt.sum()) > 0:
            raise ValueError("Node2Vec: the walks hold no pair (a graph without edges, or walk_length 1)")
        import numpy as np
        c64 = cnt.numpy()
        pw = np.where(c64 > 0, c64 ** self.ns_exponent, 0.0)  # a node that never occurs has no noise mass
        P = torch.from_numpy((pw / pw.sum()).astype(np.float32)).cuda()
        KN = (self.negative * cnt).to(torch.float32).cuda()
        U, V, err = self._tables(embedding, context_factors, n, n)
        Hu, Hv = torch.zeros_like(U), torch.zeros_like(V)
        D = torch.empty((n, self.factors), dtype=torch.float32, device="cuda")
        self.cooccurrence, self.noise = C, P
        self._iterate(lambda: self._half(C, P, KN, V, U, Hu, D, err), lambda: self._half(C, KN, P, U, V, Hv, D, err),
                      err, {"embedding": U, "context_factors": V}, callback,
                      f"co-occurrence ids out of range for {n} nodes")
        self.user_factors, self.item_factors = V, U  # similar_items: over the embedding
        return self

    def objective(self):
        """sgns_objective of the fitted tables (a Python float; monitoring and tests)."""
        return sgns_objective(self.cooccurrence, self.embedding, self.context_factors, self.negative, self.noise,
                              self.regularization)


class FastNode2Vec(EmbeddingModel):
    """node2vec embeddings of the tracks (baselines.py:223-255): ``Node2Vec`` with
    the reference's dim 128, walk_length 20, context 10, p 2.0, q 0.5, its
    epochs = 10 as walks_per_node = 10, on the weighted track-track projection
    (``projected``) or on the unweighted bipartite graph.  ``embedding`` is the
    first len(ids) rows of the centre table, a CPU tensor as in the reference."""

    def __init__(self, projected=True):
        self.model = None
        self.embedding = None
        self.projected = projected

    def train(self, g, ids, train_set, test_set, features):
        graph_csr = project_bipartite_graph(g, ids) if self.projected else bipartite_graph(g, ids)
        self.model = Node2Vec(dim=128, walk_length=20, context=10, p=2.0, q=0.5, walks_per_node=10)
        self.model.fit(graph_csr)
        self.embedding = self.model.embedding[:len(ids)].cpu()

    def embed(self, nodeset):
        return self.embedding[torch.as_tensor(nodeset).cpu(), :]

    def knn(self, nodeset, k):
        return knn_from_emb(self.embedding, nodeset, k)


# ----------------------------------------------------------------------------- GraphSAGE
# baselines.py:517-544 on lib/gnns/GNNs_unsupervised.py.
SAGE_MAX_FANOUT = 32     # kSageMaxFanout (csrc/sage.h)
SAGE_MAX_POSITIVES = 64  # kSageMaxPos
SAGE_MAX_NEGATIVES = 16  # kSageMaxNeg
SAGE_MAX_DIM = 512       # kSageMaxD
SAGE_BETAS, SAGE_EPS = (0.9, 0.999), 1e-8


class SAGE:
    """Unsupervised two-layer GraphSAGE with the MEAN aggregator (Hamilton, Ying,
    Leskovec 2017) on the kernels of csrc/sage.hip, the GEMM, the segmented
    weighted mean and the Adam kernel: what the reference's ``GraphSAGE`` builds
    from lib/gnns/GNNs_unsupervised.py.  That class cannot run as written (it
    reads ``self.proj_adj_mat`` and ``self.mode``, which do not exist), so there
    are no reference numbers.  The model is THIS PROJECT'S DEFINITION,
    deterministic and stated here in full (csrc/sage.h states it again, next to
    the kernels); the quality of the defaults on real data is unmeasured.

    Graph and features.  The graph is the tuple (ptr int64 [n + 1], idx int32,
    weight int64 or None, n) of ``project_bipartite_graph``: an undirected CSR,
    rows strictly ascending, no self loops, positive integer weights.  Features
    X0 f32 [n, d_in].  Weights W1 [emb_size, 2 d_in], W2 [emb_size, 2 emb_size],
    no bias, as the reference's SageLayer.

    Neighbour sample (r, v), fanout S = ``num_sample``, deg the length of row v.
    - deg <= S: positions 0 .. deg - 1 in CSR order; the other slots are void
      (nb = -1, w = 0).
    - Otherwise Floyd's algorithm, for j = 0 .. S - 1:

        m = deg - S + j + 1
        (r0, r1, r2, r3) = Philox4x32-10(key = seed, ctr = (r * 64 + j, v lo, v hi, offset))
        t = ((r0 | r1 << 32) * m) >> 64
        c_j = m - 1 if t is among c_0 .. c_{j-1}, else t

    - Slot j holds nb = idx[row start + c_j]; its raw weight is
      a_j = sqrtf((float)weight_e), 1 on an unweighted graph (the reference
      mask's sqrt(edge count)); w_j = a_j / (a_0 + a_1 + ...), summed in slot
      order from 0 in fp32, then one division (the reference's L1 normalisation).
    - The sample depends on (seed, offset, r, v, row v) only.

    Positives of step r with batch b_0 .. b_{B-1}: walk w < ``n_walks`` of anchor
    i is pinsage_n2v_walk on the same graph with 1/p = 1/q = 1, length
    ``walk_len`` + 1, offset 0 and position (r * batch_size + i) * n_walks + w.
    Walk positions 1 .. walk_len are the P = n_walks * walk_len positive slots
    in walk-major order; a slot is void if it is -1 or equals the anchor.

    Negatives: Q = ``negatives`` slots per anchor a, sample s < Q, tries
    k = 0 .. 15:  ctr = (r * 16 + k, (a Q + s) lo, hi, offset),
    j = (uint64(r0) * n) >> 32, accept the first j != a that is not in row a
    (binary search); void after 16 rejections.  The reference excludes the whole
    5-hop ball, which on a projected track graph is nearly every node; ONE HOP
    is used here.

    Forward.  The group of anchor i is G = 1 + P + Q slots: the anchor, its
    positives, its negatives.  T is the list of the B G slot nodes with repeats,
    void slots as node 0 and flagged.  Layer 2 uses sample (2r + 1, t) for each t
    in T; U is the sorted unique set of T and its neighbours; layer 1 uses
    sample (2r, u) for each u in U.

        H1[u] = lrelu(W1 [X0[u] || sum_j w_j X0[nb_j]])
        Z[t]  = lrelu(W2 [H1[t] || sum_j w_j H1[nb_j]])

    lrelu is the GEMM epilogue's leaky ReLU with slope 0.01; the reference uses
    plain ReLU, a stated deviation.

    Loss.  c(a, x) = z_a.z_x / max(sqrt(|z_a|^2 |z_x|^2), 1e-8); over the non-void
    slots c_pos = the smallest positive cosine and c_neg = the largest negative
    cosine, ties to the lowest slot (the reference's min / max of log sig(cos):
    log sig is monotone);  loss_a = max(0, log sig(c_neg) - log sig(c_pos) +
    margin).  An anchor is active with at least one non-void positive and one
    non-void negative; the step's loss is the sum over active anchors divided by
    max(1, #active).  Only the rows a, pos*, neg* of a group receive gradient.

    Backward: dPre2 = dZ * lrelu'(Z);  dW2 = dPre2^T [H1[t] || Agg2] (the GEMM's
    two-segment form);  [dSelf | dAgg] = dPre2 W2;  dH1[u] = the sum over the
    slots and sample entries that read u, one pinsage_segment_wmean call with
    normalize = 0 over the [2 B G, emb_size] view of [dSelf | dAgg] on a CSR
    sorted by u with entries ordered by (t, self before neighbours, j);
    dPre1 = dH1 * lrelu'(H1);  dW1 = dPre1^T [X0[u] || Agg1].  The features get
    no gradient.  Update: one pinsage_adam per weight, torch's Adam with
    ``learning_rate``, betas 0.9 / 0.999, eps 1e-8; the reference's SGD at
    lr = 0.7 with gradient clipping is not reproduced.

    Epochs.  Epoch e orders the nodes by torch.randperm(n,
    generator=torch.Generator().manual_seed((seed + e) % 2**63)); steps are
    consecutive slices of ``batch_size`` (the reference's 20 wastes the GPU: 64);
    the step counter r runs across epochs.  ``embeddings`` runs both layers over
    all n nodes with rounds 2 R and 2 R + 1, R the number of steps of the fit,
    which the fit never uses.

    Randomness.  The seed is ``random_state`` or, with None, one
    ``torch.randint(0, 2**63 - 1, (1,))`` from torch's global generator; then
    ``xavier_uniform_`` for W1, then for W2, on the CPU from the global
    generator.

    Between the kernels the index arrays (unique, local ids, the transposed
    CSR) are plain torch; the step loop reads no device value on the host.
    ``gemm_prec`` (-1: the library's default, split bf16 with fp32-level error;
    0: fp32 MFMA) is the product arithmetic of the two forward GEMMs."""

    def __init__(self, emb_size=128, num_sample=10, n_walks=4, walk_len=4, negatives=6, margin=3.0, epochs=5,
                 batch_size=64, learning_rate=1e-3, random_state=None):
        inf = float("inf")
        if not (emb_size == int(emb_size) and 4 <= int(emb_size) <= SAGE_MAX_DIM and int(emb_size) % 4 == 0):
            raise ValueError(f"SAGE: emb_size = {emb_size}: need a multiple of 4 in [4, {SAGE_MAX_DIM}]")
        if not (num_sample == int(num_sample) and 1 <= int(num_sample) <= SAGE_MAX_FANOUT):
            raise ValueError(f"SAGE: num_sample = {num_sample}: need an integer in [1, {SAGE_MAX_FANOUT}]")
        if not (n_walks == int(n_walks) and walk_len == int(walk_len) and int(n_walks) >= 1 and int(walk_len) >= 1
                and int(n_walks) * int(walk_len) <= SAGE_MAX_POSITIVES):
            raise ValueError(f"SAGE: need n_walks, walk_len >= 1 and n_walks * walk_len <= {SAGE_MAX_POSITIVES}")
        if not (negatives == int(negatives) and 1 <= int(negatives) <= SAGE_MAX_NEGATIVES):
            raise ValueError(f"SAGE: negatives = {negatives}: need an integer in [1, {SAGE_MAX_NEGATIVES}]")
        if not (-inf < margin < inf and 0 <= learning_rate < inf and int(epochs) >= 0 and int(batch_size) >= 1):
            raise ValueError("SAGE: need a finite margin, finite learning_rate >= 0, epochs >= 0, batch_size >= 1")
        self.emb_size, self.num_sample = int(emb_size), int(num_sample)
        self.n_walks, self.walk_len, self.negatives = int(n_walks), int(walk_len), int(negatives)
        self.margin, self.epochs, self.batch_size = float(margin), int(epochs), int(batch_size)
        self.learning_rate, self.random_state = float(learning_rate), random_state
        self.gemm_prec = -1
        self.weights = self.losses = None
        self.steps = 0

    # ------------------------------------------------------------------ intake
    def prepare(self, graph, features, weights=None):
        """Takes the graph and the features to the GPU, checks them, draws the
        seed and the initial weights (given ``weights`` = (W1, W2) are copied
        after the draws) and resets the optimiser.  ``fit`` starts with it."""
        nat.require_gpu()
        ptr, idx, wt, cum, n = _graph_arrays(graph, "SAGE")
        rows = _csr_rows(ptr)
        if bool(((idx[1:] <= idx[:-1]) & (rows[1:] == rows[:-1])).any()):
            raise ValueError("SAGE: rows must be strictly ascending (the negative draw binary-searches the row)")
        X0 = torch.as_tensor(features)
        if X0.dim() != 2 or int(X0.shape[0]) != n:
            raise ValueError(f"SAGE: features of shape {tuple(X0.shape)}, expected [{n}, d_in]")
        d_in = int(X0.shape[1])
        if d_in < 4 or d_in % 4:
            raise ValueError(f"SAGE: d_in = {d_in}: the GEMM needs a multiple of 4")
        self._graph = (ptr, idx, wt, cum, n)
        self._X0 = X0.to(device="cuda", dtype=torch.float32).contiguous()
        if self.random_state is None:
            self._seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))
        else:
            self._seed = int(self.random_state) & (2 ** 64 - 1)
        out = self.emb_size
        W = [torch.nn.init.xavier_uniform_(torch.empty(out, 2 * d_in)),
             torch.nn.init.xavier_uniform_(torch.empty(out, 2 * out))]
        if weights is not None:
            for k, given in enumerate(weights):
                g = torch.as_tensor(given)
                if tuple(g.shape) != tuple(W[k].shape):
                    raise ValueError(f"SAGE: W{k + 1} of shape {tuple(g.shape)}, expected {tuple(W[k].shape)}")
                W[k] = g
        self.weights = [w.to(device="cuda", dtype=torch.float32, copy=True).contiguous() for w in W]
        self._m = [torch.zeros_like(w) for w in self.weights]
        self._v = [torch.zeros_like(w) for w in self.weights]
        self._err = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.steps, self.losses = 0, []
        return self

    # ------------------------------------------------------------------ launches
    def _gemm(self, what, **kw):
        import ctypes
        p = nat.GemmParams(**kw)
        rc = nat.lib().pinsage_gemm_params(ctypes.byref(p), None, nat.stream_ptr())
        if rc == -2:
            raise ValueError(f"SAGE: {what}: " + nat.lib().pinsage_last_error().decode(errors="replace"))
        nat.check(rc, what)

    def sample(self, nodes, round):
        """(nb int32 [m, num_sample], w float32 [m, num_sample]) on the GPU: the
        neighbour sample (round, v) of every v in ``nodes`` (pinsage_sage_neighbours)."""
        ptr, idx, wt, _, n = self._graph
        nodes = torch.as_tensor(nodes).to(device="cuda", dtype=torch.int64).contiguous()
        m, S = int(nodes.numel()), self.num_sample
        nb = torch.empty((m, S), dtype=torch.int32, device="cuda")
        w = torch.empty((m, S), dtype=torch.float32, device="cuda")
        nat.check(nat.lib().pinsage_sage_neighbours(nat.ptr(ptr), nat.ptr(idx), nat.ptr(wt), n, nat.ptr(nodes), m, S,
                                                    self._seed, int(round), 0, nat.ptr(nb), nat.ptr(w),
                                                    nat.ptr(self._err), nat.stream_ptr()), "sage_neighbours")
        return nb, w

    def _slots(self, batch, r):
        """int32 [B, G]: the anchor, its positives and its negatives, -1 = void."""
        ptr, idx, _, cum, n = self._graph
        B, L = int(batch.numel()), self.walk_len + 1
        starts = batch.repeat_interleave(self.n_walks).contiguous()
        walks = torch.empty((B * self.n_walks, L), dtype=torch.int32, device="cuda")
        nat.check(nat.lib().pinsage_n2v_walk(nat.ptr(ptr), nat.ptr(idx), nat.ptr(cum), n, nat.ptr(starts),
                                             int(starts.numel()), L, 1.0, 1.0, self._seed, 0,
                                             int(r) * self.batch_size * self.n_walks, nat.ptr(walks),
                                             nat.ptr(self._err), nat.stream_ptr()), "n2v_walk")
        anchor = batch.to(torch.int32)[:, None]
        pos = walks[:, 1:].reshape(B, self.n_walks * self.walk_len)
        pos = torch.where(pos == anchor, torch.full_like(pos, -1), pos)
        neg = torch.empty((B, self.negatives), dtype=torch.int32, device="cuda")
        nat.check(nat.lib().pinsage_sage_negatives(nat.ptr(ptr), nat.ptr(idx), n, nat.ptr(batch), B, self.negatives,
                                                   self._seed, int(r), 0, nat.ptr(neg), nat.ptr(self._err),
                                                   nat.stream_ptr()), "sage_negatives")
        return torch.cat([anchor, pos, neg], 1).contiguous()

    def _layer(self, h, self_idx, cols, w, W, rows_alloc):
        """lrelu(W [h[self_idx] || sum_j w_j h[cols_j]]) for the len(self_idx) rows:
        (the aggregate, the output), the aggregate with rows_alloc >= rows rows,
        the tail zero (the weight gradient's K is a multiple of 4)."""
        m, S, d, out = int(self_idx.numel()), self.num_sample, int(h.shape[1]), self.emb_size
        agg = torch.empty((rows_alloc, d), dtype=torch.float32, device="cuda")
        if rows_alloc > m:
            agg[m:].zero_()
        seg = torch.arange(0, (m + 1) * S, S, dtype=torch.int64, device="cuda")
        nat.check(nat.lib().pinsage_segment_wmean(nat.ptr(h), h.stride(0), int(h.shape[0]), d, nat.ptr(seg),
                                                  nat.ptr(cols), nat.ptr(w), m, 0, nat.ptr(agg), agg.stride(0),
                                                  nat.stream_ptr()), "segment_wmean")
        y = torch.empty((m, out), dtype=torch.float32, device="cuda")
        self._gemm("layer", M=m, N=out, K=2 * d, a=h.data_ptr(), lda=h.stride(0), a_idx=self_idx.data_ptr(), K1=d,
                   a2=agg.data_ptr(), lda2=agg.stride(0), b=W.data_ptr(), ldb=W.stride(0), c=y.data_ptr(),
                   ldc=y.stride(0), act=1, prec=self.gemm_prec)
        return agg, y

    def _dpre(self, y, dy, rows_alloc):
        """dy * lrelu'(y) with rows_alloc >= rows rows, the tail zero."""
        m, out = int(y.shape[0]), int(y.shape[1])
        dp = torch.empty((rows_alloc, out), dtype=torch.float32, device="cuda")
        if rows_alloc > m:
            dp[m:].zero_()
        nat.check(nat.lib().pinsage_sage_lrelu_backward(nat.ptr(y), y.stride(0), nat.ptr(dy), dy.stride(0), m, out,
                                                        nat.ptr(dp), dp.stride(0), nat.stream_ptr()),
                  "sage_lrelu_backward")
        return dp

    def _wgrad(self, dp, h, self_idx, agg):
        """dp^T [h[self_idx] || agg]: [emb_size, d + d], K = the rows of dp."""
        K, out, d = int(dp.shape[0]), int(dp.shape[1]), int(h.shape[1])
        dW = torch.empty((out, 2 * d), dtype=torch.float32, device="cuda")
        self._gemm("weight gradient", M=out, N=2 * d, K=K, a_kmajor=0, b_kmajor=0, a=dp.data_ptr(), lda=dp.stride(0),
                   b=h.data_ptr(), ldb=h.stride(0), b_idx=self_idx.data_ptr(), N1=d, b2=agg.data_ptr(),
                   ldb2=agg.stride(0), c=dW.data_ptr(), ldc=dW.stride(0))
        return dW

    @staticmethod
    def _pad4(idx32):
        """idx32 with zeros appended up to a multiple of 4 entries."""
        extra = -int(idx32.numel()) % 4
        return torch.cat([idx32, idx32.new_zeros(extra)]).contiguous() if extra else idx32

    def step_tensors(self, batch, r):
        """One step r on ``batch`` (node ids) from the current weights, without
        updating: a dict of slots [B, G], T, U, the sample tables (nb1, w1) of U
        and (nb2, w2) of T, H1, Z, the per-anchor loss, active and sel, dZ, the
        step's loss (a device scalar) and the gradients dW1, dW2."""
        L = nat.lib()
        _, _, _, _, n = self._graph
        X0, (W1, W2) = self._X0, self.weights
        out, S = self.emb_size, self.num_sample
        P, Q = self.n_walks * self.walk_len, self.negatives
        batch = torch.as_tensor(batch).to(device="cuda", dtype=torch.int64).contiguous()
        B, G = int(batch.numel()), 1 + P + Q
        slots = self._slots(batch, r)
        T = slots.clamp(min=0).reshape(-1).to(torch.int64)
        nb2, w2 = self.sample(T, 2 * r + 1)
        U = torch.unique(torch.cat([T, nb2[nb2 >= 0].to(torch.int64)]))
        nb1, w1 = self.sample(U, 2 * r)
        nU, nT = int(U.numel()), B * G
        nUp, nTp = nU + (-nU) % 4, nT + (-nT) % 4
        U32 = self._pad4(U.to(torch.int32))
        t_loc = self._pad4(torch.searchsorted(U, T).to(torch.int32))
        nb2_loc = torch.where(nb2 >= 0, torch.searchsorted(U, nb2.clamp(min=0).to(torch.int64)).to(torch.int32), nb2)
        nb2_loc = nb2_loc.contiguous()
        # forward
        agg1, H1 = self._layer(X0, U32[:nU], nb1, w1, W1, nUp)
        agg2, Z = self._layer(H1, t_loc[:nT], nb2_loc, w2, W2, nTp)
        # loss
        void = slots < 0
        act = (~void[:, 1:1 + P]).any(1) & (~void[:, 1 + P:]).any(1) & ~void[:, 0]
        scale = (1.0 / act.sum().clamp(min=1).to(torch.float32)).reshape(1)
        loss_a = torch.empty(B, dtype=torch.float32, device="cuda")
        active = torch.empty(B, dtype=torch.int32, device="cuda")
        sel = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        dZ = torch.empty((nT, out), dtype=torch.float32, device="cuda")
        nat.check(L.pinsage_sage_margin_loss(nat.ptr(Z), Z.stride(0), out, nat.ptr(slots), B, P, Q, self.margin,
                                             nat.ptr(scale), nat.ptr(loss_a), nat.ptr(active), nat.ptr(sel),
                                             nat.ptr(dZ), dZ.stride(0), nat.stream_ptr()), "sage_margin_loss")
        # backward
        dP2 = self._dpre(Z, dZ, nTp)
        dW2 = self._wgrad(dP2, H1, t_loc, agg2)
        dSA = torch.empty((nT, 2 * out), dtype=torch.float32, device="cuda")
        self._gemm("input gradient", M=nT, N=2 * out, K=out, b_kmajor=0, a=dP2.data_ptr(), lda=dP2.stride(0),
                   b=W2.data_ptr(), ldb=W2.stride(0), c=dSA.data_ptr(), ldc=dSA.stride(0))
        # the transposed CSR over U: per t its own row of dSelf, then its sample's rows of dAgg
        t = torch.arange(nT, dtype=torch.int32, device="cuda")[:, None]
        key = torch.cat([t_loc[:nT, None], nb2_loc], 1).reshape(-1)
        col = torch.cat([2 * t, (2 * t + 1).expand(nT, S)], 1).reshape(-1)
        wt = torch.cat([torch.ones((nT, 1), dtype=torch.float32, device="cuda"), w2], 1).reshape(-1)
        ok = key >= 0
        key = key[ok].to(torch.int64)
        order = torch.sort(key, stable=True).indices
        colT, wT, ptrT = col[ok][order].contiguous(), wt[ok][order].contiguous(), _csr_ptr(key, nU)
        dH1 = torch.empty((nU, out), dtype=torch.float32, device="cuda")
        nat.check(L.pinsage_segment_wmean(dSA.data_ptr(), out, 2 * nT, out, nat.ptr(ptrT), nat.ptr(colT), nat.ptr(wT),
                                          nU, 0, nat.ptr(dH1), dH1.stride(0), nat.stream_ptr()), "segment_wmean")
        dP1 = self._dpre(H1, dH1, nUp)
        dW1 = self._wgrad(dP1, X0, U32, agg1)
        return dict(slots=slots, T=T, U=U, nb1=nb1, w1=w1, nb2=nb2, w2=w2, H1=H1, Z=Z, loss_a=loss_a, active=active,
                    sel=sel, dZ=dZ, loss=loss_a.sum() * scale[0], dW1=dW1, dW2=dW2)

    def _adam(self, grads):
        self.steps += 1
        b1, b2 = SAGE_BETAS
        coef = torch.tensor([self.learning_rate / (1.0 - b1 ** self.steps), (1.0 - b2 ** self.steps) ** 0.5],
                            dtype=torch.float32).to("cuda")
        for p, g, m, v in zip(self.weights, grads, self._m, self._v):
            nat.check(nat.lib().pinsage_adam(nat.ptr(p), nat.ptr(g), nat.ptr(m), nat.ptr(v), int(p.numel()),
                                             nat.ptr(coef), b1, b2, SAGE_EPS, nat.stream_ptr()), "adam")

    def fit(self, graph, features, callback=None, weights=None):
        """graph: (ptr, idx, weight or None, n); features [n, d_in].  Rows not
        strictly ascending or arrays that do not fit together raise ValueError,
        neighbour ids out of range IndexError, shapes the GEMM refuses
        ValueError.  ``callback(step, self)`` runs after every step
        (monitoring).  Sets ``weights`` and ``losses`` (one float per step, read
        back once at the end)."""
        self.prepare(graph, features, weights)
        n = self._graph[4]
        per_epoch = -(-n // self.batch_size)
        if 2 * self.epochs * per_epoch + 2 > 1 << 25:
            raise ValueError("SAGE: sample round 2 * steps + 1 must stay below 2^25")
        losses, r = [], 0
        for e in range(self.epochs):
            order = torch.randperm(n, generator=torch.Generator().manual_seed((self._seed + e) % 2 ** 63)).to("cuda")
            for b0 in range(0, n, self.batch_size):
                st = self.step_tensors(order[b0:b0 + self.batch_size], r)
                self._adam((st["dW1"], st["dW2"]))
                losses.append(st["loss"])
                r += 1
                if callback is not None:
                    callback(r - 1, self)
        self._rounds = r
        self.losses = torch.stack(losses).cpu().tolist() if losses else []
        if int(self._err):
            raise IndexError(f"SAGE: node ids out of range for {n} nodes")
        return self

    def embeddings(self):
        """float32 [n, emb_size] on the GPU: both layers over all n nodes with the
        sample rounds 2 R and 2 R + 1, R the number of steps of the fit."""
        n, R = self._graph[4], getattr(self, "_rounds", 0)
        if 2 * R + 1 >= 1 << 25:
            raise ValueError("SAGE: sample round 2 * steps + 1 must stay below 2^25")
        nodes = torch.arange(n, dtype=torch.int64, device="cuda")
        loc = nodes.to(torch.int32)
        nb1, w1 = self.sample(nodes, 2 * R)
        _, H1 = self._layer(self._X0, loc, nb1, w1, self.weights[0], n)
        nb2, w2 = self.sample(nodes, 2 * R + 1)
        return self._layer(H1, loc, nb2, w2, self.weights[1], n)[1]


class GraphSAGE(EmbeddingModel):
    """GraphSAGE embeddings of the tracks (baselines.py:517-544): ``SAGE`` with
    its defaults on the weighted track-track projection and ``features``.
    ``projected=False`` raises NotImplementedError: the bipartite graph's
    collections have no features (the reference's line for it cannot run
    either).  ``embedding`` is a CPU tensor as FastNode2Vec's."""

    def __init__(self, projected=True):
        self.model = None
        self.embedding = None
        self.projected = projected

    def train(self, g, ids, train_set, test_set, features):
        if not self.projected:
            raise NotImplementedError("GraphSAGE: projected=False needs features of the collections; there are none")
        self.model = SAGE()
        self.model.fit(project_bipartite_graph(g, ids), torch.as_tensor(features)[:len(ids)])
        self.embedding = self.model.embeddings().cpu()

    def embed(self, nodeset):
        return self.embedding[torch.as_tensor(nodeset).cpu(), :]

    def knn(self, nodeset, k):
        return knn_from_emb(self.embedding, nodeset, k)


# ----------------------------------------------------------------------------- link-prediction indices
# baselines.py:153-191.  Two-hop scores between tracks over a graph held as the
# two CSRs of csrc/cooc.hip: t2c, n rows of middle ids in [0, n_mid), and c2t,
# n_mid rows of track ids, both ascending and without duplicates.
#   deg(t) = len(t2c row t),  dmid(c) = len(c2t row c),  cn(q, t) = |N(q) & N(t)|
LINKSIM_SHIFT = 30  # fixed point of the Adamic-Adar weights (kCoocShift, csrc/cooc.hip)


def adamic_adar_weights(dmid):
    """The fixed-point weight of a middle node of each degree in ``dmid``:
    floor(2^30 / ln(d) + 0.5) as int64, formed in float64 on dmid's device, and 0
    for d <= 1 (such a node joins no two distinct tracks).  With 2^30 a sum over
    fewer than 2^31 middle nodes stays below 2^62."""
    d = torch.as_tensor(dmid).to(torch.float64)
    w = torch.floor(float(1 << LINKSIM_SHIFT) / torch.log(d.clamp(min=2.0)) + 0.5)
    return torch.where(d >= 2, w, torch.zeros_like(w)).to(torch.int64)


class SimpleSimilarity(PredictionModel):
    """Base of the three networkx link-prediction indices (baselines.py:153-174),
    which the reference scores one pair at a time, n pairs per query, in Python.

    ``projected=True``: the graph is the track-track projection
    (``project_bipartite_graph``; its weights are ignored, as networkx's three
    functions ignore them), so both CSRs are its adjacency and the middle nodes
    are tracks.  ``projected=False``: the bipartite graph, the middle nodes are
    the collections, membership is JaccardFast.train's rule.  That rule drops an
    edge between two tracks, which networkx would keep as an edge of the graph.

    ``knn(nodeset, k)`` is the reference's bare ``topk(k)`` of the query's score
    row against all tracks: k columns, column 0 NOT dropped (it is the query
    itself only where nothing ties or beats it), on nodeset's device, in this
    package's order (score descending, then id ascending)."""

    def __init__(self, projected=True):
        self.projected = projected

    def train(self, g, ids, train_set, test_set, features):
        nat.require_gpu()
        who = type(self).__name__
        self.ids = ids
        self.n = n = len(ids)
        if self.projected:
            ptr, idx, _, _ = project_bipartite_graph(g, ids)
            self._t2c = self._c2t = (ptr, idx)
            self.n_mid = n
        else:
            self._t2c, self._c2t, self.n_mid = _membership_csrs(g, n, who)
        self.deg = self._t2c[0][1:] - self._t2c[0][:-1]    # int64 [n], on the GPU
        self.dmid = self._c2t[0][1:] - self._c2t[0][:-1]   # int64 [n_mid]

    def _queries(self, nodeset):
        return _track_queries(nodeset, self.n, type(self).__name__)

    def _csr_args(self):
        return (nat.ptr(self._t2c[0]), nat.ptr(self._t2c[1]), nat.ptr(self._c2t[0]), nat.ptr(self._c2t[1]),
                self.n, self.n_mid)


class JaccardIndex(SimpleSimilarity):
    """The Jaccard coefficient of two tracks' neighbour sets,
    cn / (deg q + deg t - cn), 0 where the union is empty: networkx's
    ``jaccard_coefficient``.  The reference's class of this name is assigned
    ``nx.preferential_attachment`` (baselines.py:176-180), evidently by mistake;
    this one computes what the name says.  No kernel of its own: it is
    pinsage_cooc_jaccard over the model's CSRs, whose fp32 co / (union + 1e-10)
    equals float32 of networkx's value bit for bit for degrees below 2^24.  With
    projected=False, ``knn(q, k)[:, 1:]`` is ``JaccardFast.knn(q, k)``."""

    def knn(self, nodeset, k):
        out_dev = torch.as_tensor(nodeset).device
        w, nb = _cooc_lists("pinsage_cooc_jaccard", "pinsage_cooc_scratch_bytes", self._csr_args(), self.n,
                            self._queries(nodeset), k, "JaccardIndex")
        return w.to(out_dev), nb.to(out_dev)


class AdamicAdar(SimpleSimilarity):
    """The Adamic-Adar index, the sum over the common neighbours c of
    1 / ln dmid(c), in fixed point (csrc/cooc.hip's weighted kernel):

        wt = adamic_adar_weights(dmid);  S(q, t) = sum of wt[c], int64
        score = float32(S) * 2^-30       (int64 -> float32 to nearest even)

    Integer adds make S, and so the lists, independent of the order of the
    adds.  networkx raises ZeroDivisionError on the pair (q, q) where q has a
    neighbour of degree 1 (ln 1 = 0); such a neighbour weighs 0 here."""

    def train(self, g, ids, train_set, test_set, features):
        super().train(g, ids, train_set, test_set, features)
        # on the host: one table, whatever the device's log rounds to
        self.weights = adamic_adar_weights(self.dmid.cpu()).to("cuda").contiguous()

    def _weighted_args(self):
        return self._csr_args() + (nat.ptr(self.weights),)

    def sums(self, nodeset):
        """S(q, .) of each query, dense: int64 [len(nodeset), n] on the GPU."""
        qd = self._queries(nodeset)
        nq = int(qd.numel())
        out = torch.empty((nq, self.n), dtype=torch.int64, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        nat.check(nat.lib().pinsage_cooc_weighted_sums(*self._weighted_args(), nat.ptr(qd), nq, nat.ptr(out),
                                                       nat.ptr(err), nat.stream_ptr()), "cooc_weighted_sums")
        if int(err):
            raise IndexError(f"AdamicAdar: query ids out of range for {self.n} tracks")
        return out

    def knn(self, nodeset, k):
        out_dev = torch.as_tensor(nodeset).device
        w, nb = _cooc_lists("pinsage_cooc_weighted_knn", "pinsage_cooc_weighted_scratch_bytes",
                            self._weighted_args(), self.n, self._queries(nodeset), k, "AdamicAdar")
        return w.to(out_dev), nb.to(out_dev)


class Preferential(SimpleSimilarity):
    """Preferential attachment, deg(q) deg(t), exact in int64 (the reference's
    ``torch.tensor`` of Python ints is int64 too).  For deg(q) > 0 the order
    (score descending, id ascending) is deg(t) descending, then id ascending,
    whatever the query: one stable sort at ``train``, and ``knn`` is its first k
    ids with the products as weights.  For deg(q) = 0 every score is 0: ids
    0 .. k - 1, weights zeros.  Plain torch on the GPU; no kernel."""

    def train(self, g, ids, train_set, test_set, features):
        super().train(g, ids, train_set, test_set, features)
        self._by_degree = torch.sort(self.deg, descending=True, stable=True).indices

    def knn(self, nodeset, k):
        out_dev = torch.as_tensor(nodeset).device
        qd, k = self._queries(nodeset), int(k)
        if not 0 <= k <= self.n:
            raise ValueError(f"Preferential: k = {k} over {self.n} tracks")
        dq = self.deg[qd].unsqueeze(1)
        nb = torch.where(dq > 0, self._by_degree[:k].unsqueeze(0), torch.arange(k, device="cuda").unsqueeze(0))
        return (dq * self.deg[nb]).to(out_dev), nb.to(out_dev)


class Random(PredictionModel):
    """Random recommendations (baselines.py:380-397): per query the first k of
    a ``torch.randperm(n)`` from torch's global generator, weights of ones (int64,
    as ``ones_like`` of the ids gives).  Host only."""

    def __init__(self):
        pass

    def train(self, g, ids, train_set, test_set, features):
        self.ids = ids
        self.n = len(ids)

    def knn(self, nodeset, k):
        nodes = torch.stack([torch.randperm(self.n)[0:k] for _ in range(nodeset.shape[0])], dim=0)
        return torch.ones_like(nodes), nodes


class EmbeddingTable(EmbeddingModel):
    """kNN over a fixed embedding table (e.g. PinSage.embed output): the
    embed/knn pair of the reference's EmbeddingModel wrappers
    (baselines.py:324-328)."""

    def __init__(self, embedding=None):
        self.embedding = embedding

    def train(self, g, ids, train_set, test_set, features):
        pass

    def embed(self, nodeset):
        return self.embedding[nodeset, :]

    def knn(self, nodeset, k):
        return knn_from_emb(self.embedding, nodeset, k)


def save_knn(model, model_name, ids, save_dir, train_time=0, emb_time=0, b_size=1000):
    """eval.py:112-143: kNN lists of all nodes (k = PRECOMP_K) in batches, saved
    once as (w, n, train_time, emb_time, knn_time) to <save_dir>/knn/<name>.pt."""
    save_dir = os.path.join(save_dir, "knn")
    os.makedirs(save_dir, exist_ok=True)
    save_path = os.path.join(save_dir, model_name + ".pt")
    if os.path.isfile(save_path):
        return
    all_nodes = torch.arange(0, len(ids), dtype=torch.int64)
    n = len(all_nodes)
    knn_time = 0.0
    ws, ns = [], []
    for i in range(0, n, b_size):
        t0 = time.time()
        bw, bn = model.knn(all_nodes[i:min(i + b_size, n)], PRECOMP_K)
        ws.append(bw)
        ns.append(bn)
        knn_time += time.time() - t0
    torch.save((torch.cat(ws, dim=0), torch.cat(ns, dim=0), train_time, emb_time, knn_time),
               save_path)


def load_knn(model_name, ids, save_dir):
    """eval.py:146-149 (weights-only load: the file holds tensors and floats)."""
    return torch.load(os.path.join(save_dir, "knn", model_name + ".pt"), weights_only=True)


__all__ = ["PRECOMP_K", "PredictionModel", "EmbeddingModel", "cosine_sim_ab", "knn_from_emb",
           "PersPageRank", "EmbeddingTable", "save_knn", "load_knn", "RANK_MAX_GROUP", "rank_from_emb",
           "hit_rate", "mrr", "hit_rate_from_ranks", "mrr_from_ranks", "low_degree_accuracy",
           "low_degree_accuracy_from_ranks", "LIST_OVERLAP_MAX_K", "intra_diversity", "inter_diversity",
           "coverage", "average_degree", "degree_dist", "beyond_accuracy", "compute_beyond_accuracy_table",
           "JaccardFast", "Random", "low_co_accuracy", "low_co_accuracy_from_ranks", "LazyKnnDict",
           "compute_results_table", "ALS_MAX_FACTORS", "ALS", "als_loss", "to_col_track_matrix",
           "to_track_track_matrix", "ColTrackCF", "TrackTrackCF", "LMF_MAX_FACTORS", "LMF", "lmf_objective",
           "ColTrackLMF", "TrackTrackLMF", "project_bipartite_graph", "bipartite_graph", "n2v_cooccurrence",
           "sgns_objective", "N2V_MAX_BIAS_RATIO", "Node2Vec", "FastNode2Vec", "BPR_MAX_FACTORS", "BPR_MAX_TRIES",
           "BPR_MAX_NEGATIVES", "BPR", "bpr_objective", "ColTrackBPR", "TrackTrackBPR", "LINKSIM_SHIFT",
           "adamic_adar_weights", "SimpleSimilarity", "JaccardIndex", "AdamicAdar", "Preferential"]
