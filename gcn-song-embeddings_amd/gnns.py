"""The lib/gnns MEAN and GAT aggregators on the GPU.

``GNN_model.aggregate`` (lib/gnns/GNNs_unsupervised.py:537-588, agg_func
'MEAN', gat False) builds a dense [F, U] mask -- ones at each sampled
neighbour (the node itself removed unless ``gcn``), times sqrt(edge count)
from the adjacency matrix, L1-normalised per row (``F.normalize(p=1)``) -- and
returns ``mask.mm(embed_matrix)``.  The mask holds a handful of non-zeros per
row, so here it stays a CSR and the product is the segmented weighted mean
``pinsage_segment_wmean`` (csrc/gnns.hip): one gather-and-accumulate pass over
the neighbour rows, no [F, U] buffer.  Gradients flow to ``pre_hidden_embs``
through the transposed CSR (same kernel, fixed summation order, no atomics).

With ``gat=True`` (:555-567) the mask is a softmax over each node's whole
neighbourhood of ``leaky_relu(att([h_node || h_nb]), 0.2) * sqrt(edge count)``
with the ``Attention`` module's weights.  ``gat_aggregate`` runs it as an edge
softmax fused with the gather (``pinsage_gat_*``, csrc/gnns.hip; definitions in
csrc/gnns.h): per-node scores once, then one pass over the neighbour rows, no
[F, U] mask and no gathered [nnz, d] matrices; gradients to the embeddings and
to the selected attention weight, no atomics, bitwise reproducible.

Host-side neighbour sampling (``_get_unique_neighs_list``,
GNNs_unsupervised.py:522-535) stays Python, with the reference's own
``random.sample`` / set semantics, so the unique-node order and the sampled
sets are the reference's.  Compute runs in HIP only (no CPU fallback).
"""
from __future__ import annotations

import random

import numpy as np
import torch

import _native as nat


def get_unique_neighs_list(adj_lists, nodes, num_sample=10, gcn=False, gat=False):
    """``GNN_model._get_unique_neighs_list`` (GNNs_unsupervised.py:522-535):
    returns ``(unique_nodes_list, samp_neighs, unique_nodes)`` with the same
    ``random.sample`` draws and set orders as the reference."""
    to_neighs = [adj_lists[int(node)] for node in nodes]
    if gcn or gat:
        samp_neighs = to_neighs
    else:
        samp_neighs = [set(random.sample(tuple(to_neigh), num_sample)) if len(to_neigh) >= num_sample
                       else to_neigh for to_neigh in to_neighs]
    samp_neighs = [samp_neigh | {nodes[i]} for i, samp_neigh in enumerate(samp_neighs)]
    unique_nodes_list = list(set.union(*samp_neighs))
    unique_nodes = dict(zip(unique_nodes_list, range(len(unique_nodes_list))))
    return unique_nodes_list, samp_neighs, unique_nodes


def mask_csr(nodes, pre_neighs, adj_matrix, gcn=False, gat=False):
    """The aggregation mask of GNNs_unsupervised.py:540-574 as a CSR over the
    unique-node columns: (seg_ptr int64 [F+1], cols int64, w float32).  The
    weights are the mask entries before normalisation: 1 * sqrt(edge count),
    in float32 as the reference (edge counts go through torch.FloatTensor)."""
    unique_nodes_list, samp_neighs, unique_nodes = pre_neighs
    assert len(nodes) == len(samp_neighs)
    assert all(nodes[i] in samp_neighs[i] for i in range(len(samp_neighs)))
    if not gat and not gcn:
        samp_neighs = [samp_neighs[i] - {nodes[i]} for i in range(len(samp_neighs))]
    counts = [len(s) for s in samp_neighs]
    seg_ptr = np.zeros(len(samp_neighs) + 1, np.int64)
    np.cumsum(counts, out=seg_ptr[1:])
    rows = np.repeat(np.asarray([int(n) for n in nodes], np.int64), counts)
    members = [n for s in samp_neighs for n in s]
    cols = np.fromiter((unique_nodes[n] for n in members), np.int64, count=len(members))
    # edge_counts = adj_matrix[nodes][:, unique_nodes_list] at the mask's non-zeros
    adj = adj_matrix.tocsr()
    ec = np.asarray(adj[rows, np.asarray(members, np.int64)]).reshape(-1) if len(members) else \
        np.zeros(0)
    w = np.sqrt(ec.astype(np.float32))
    return seg_ptr, cols, w


class _SegmentWMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, seg_ptr, cols, w, n_seg, fwd_T):
        out = torch.empty((n_seg, h.shape[1]), dtype=torch.float32, device=h.device)
        nat.check(nat.lib().pinsage_segment_wmean(
            nat.ptr(h), h.stride(0), h.shape[0], h.shape[1], nat.ptr(seg_ptr), nat.ptr(cols), nat.ptr(w),
            n_seg, 1, nat.ptr(out), out.stride(0), nat.stream_ptr()), "segment_wmean")
        ctx.n_h = h.shape[0]
        ctx.fwd_T = fwd_T
        return out

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        dout = dout.contiguous()
        rows_u, segT, colsT, wT = ctx.fwd_T
        du = torch.empty((rows_u.numel(), dout.shape[1]), dtype=torch.float32, device=dout.device)
        nat.check(nat.lib().pinsage_segment_wmean(
            nat.ptr(dout), dout.stride(0), dout.shape[0], dout.shape[1], nat.ptr(segT), nat.ptr(colsT),
            nat.ptr(wT), rows_u.numel(), 0, nat.ptr(du), du.stride(0), nat.stream_ptr()), "segment_wmean_bwd")
        dh = torch.zeros((ctx.n_h, dout.shape[1]), dtype=torch.float32, device=dout.device)
        dh.index_copy_(0, rows_u, du)
        return dh, None, None, None, None, None


def _transpose(seg_ptr, hrows, w, n_h):
    """CSR of the mask's transpose over the touched h rows, with the row
    normalisation folded into the weights (the backward's dH = mask^T dOut)."""
    F = len(seg_ptr) - 1
    counts = np.diff(seg_ptr)
    seg_of = np.repeat(np.arange(F, dtype=np.int64), counts)
    den = np.zeros(F, np.float32)
    np.add.at(den, seg_of, np.abs(w))
    wn = (w / np.maximum(den, np.float32(1e-12))[seg_of]).astype(np.float32)
    order = np.argsort(hrows, kind="stable")
    hs = hrows[order]
    rows_u, start = np.unique(hs, return_index=True)
    segT = np.append(start, len(hs)).astype(np.int64)
    return rows_u, segT, seg_of[order].astype(np.int32), wn[order]


class Attention(torch.nn.Module):
    """The reference's ``Attention`` (GNNs_unsupervised.py:449-465): the same
    parameters, ``state_dict`` keys and default ``nn.Linear`` init in the same
    order, so under one ``torch.manual_seed`` the weights are the reference's.
    Its forward is ``gat_aggregate``'s kernels; ``select_attention`` is the
    forward's choice of layer."""

    def __init__(self, input_size, out_size):
        super().__init__()
        self.input_size = input_size
        self.out_size = out_size
        self.attention_raw = torch.nn.Linear(2 * input_size, 1, bias=False)
        self.attention_emb = torch.nn.Linear(2 * out_size, 1, bias=False)


def select_attention(attention, width):
    """The layer ``Attention.forward`` (GNNs_unsupervised.py:459-463) takes for
    embeddings of this width, in the reference's order: ``attention_raw`` when
    it is ``input_size`` (so always, when the two sizes are equal), else
    ``attention_emb`` when it is ``out_size``.  Works on the reference's own
    module too.  The reference fails on an unbound name otherwise; here a
    ValueError."""
    if width == attention.input_size:
        return attention.attention_raw
    if width == attention.out_size:
        return attention.attention_emb
    raise ValueError(f"gat_aggregate: embedding width {width} is neither the attention's input_size "
                     f"{attention.input_size} nor its out_size {attention.out_size}")


def gat_plan(seg_ptr, hrows, own, n_h):
    """Host plan of the GAT backward's per-row pass: ``(rows_u, segT, entT,
    segofT, own_ptr, own_seg)``.  rows_u int32: the touched h rows, ascending;
    segT/entT/segofT: the transposed CSR (for row rows_u[t], the entries k with
    hrows[k] == rows_u[t] in ascending k, and their segments); own_ptr/own_seg:
    the segments whose own row is rows_u[t], ascending (batch nodes may
    repeat).  Entries and segments whose row is outside [0, n_h) are left out."""
    hrows = np.asarray(hrows, np.int64)
    own = np.asarray(own, np.int64)
    seg_of = np.repeat(np.arange(len(seg_ptr) - 1, dtype=np.int64), np.diff(seg_ptr))
    ent = np.flatnonzero((hrows >= 0) & (hrows < n_h))
    segs = np.flatnonzero((own >= 0) & (own < n_h))
    rows_u = np.unique(np.concatenate([hrows[ent], own[segs]]))
    entT = ent[np.argsort(hrows[ent], kind="stable")]
    segT = np.append(np.searchsorted(hrows[entT], rows_u, side="left"), len(entT)).astype(np.int64)
    own_seg = segs[np.argsort(own[segs], kind="stable")]
    own_ptr = np.append(np.searchsorted(own[own_seg], rows_u, side="left"), len(own_seg)).astype(np.int64)
    return (rows_u.astype(np.int32), segT, entT.astype(np.int32), seg_of[entT].astype(np.int32), own_ptr,
            own_seg.astype(np.int32))


class _GatAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, seg_ptr, hrow, c, own, plan):
        L = nat.lib()
        n_h, d = h.shape
        n_seg, nnz = own.numel(), hrow.numel()
        a = weight.detach().reshape(-1).to(device=h.device, dtype=torch.float32).contiguous()
        rows_u = plan[0]
        s_l = torch.empty(n_h, dtype=torch.float32, device=h.device)
        s_r = torch.empty(n_h, dtype=torch.float32, device=h.device)
        all_rows = rows_u.numel() == n_h
        nat.check(L.pinsage_gat_node_scores(nat.ptr(h), h.stride(0), n_h, d, nat.ptr(a),
                                            None if all_rows else nat.ptr(rows_u), rows_u.numel(), nat.ptr(s_l),
                                            nat.ptr(s_r), nat.stream_ptr()), "gat_node_scores")
        out = torch.empty((n_seg, d), dtype=torch.float32, device=h.device)
        p = torch.empty(nnz, dtype=torch.float32, device=h.device)
        nat.check(L.pinsage_gat_forward(nat.ptr(h), h.stride(0), n_h, d, nat.ptr(seg_ptr), nat.ptr(hrow), nat.ptr(c),
                                        nat.ptr(own), n_seg, nnz, nat.ptr(s_l), nat.ptr(s_r), nat.ptr(out),
                                        out.stride(0), nat.ptr(p), nat.stream_ptr()), "gat_forward")
        ctx.save_for_backward(h, a, s_l, s_r, p)
        ctx.csr = (seg_ptr, hrow, c, own, plan)
        ctx.weight_shape = weight.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        L = nat.lib()
        h, a, s_l, s_r, p = ctx.saved_tensors
        seg_ptr, hrow, c, own, (rows_u, segT, entT, segofT, own_ptr, own_seg) = ctx.csr
        n_h, d = h.shape
        n_seg, nnz, n_rows = own.numel(), hrow.numel(), rows_u.numel()
        dout = dout.to(torch.float32).contiguous()
        dev = h.device
        de = torch.empty(nnz, dtype=torch.float32, device=dev)
        s = torch.empty(n_seg, dtype=torch.float32, device=dev)
        nat.check(L.pinsage_gat_backward_edges(
            nat.ptr(h), h.stride(0), n_h, d, nat.ptr(seg_ptr), nat.ptr(hrow), nat.ptr(c), nat.ptr(own), n_seg, nnz,
            nat.ptr(s_l), nat.ptr(s_r), nat.ptr(p), nat.ptr(dout), dout.stride(0), nat.ptr(de), nat.ptr(s),
            nat.stream_ptr()), "gat_backward_edges")
        dh = torch.zeros((n_h, d), dtype=torch.float32, device=dev)
        coef = torch.empty(2 * n_rows, dtype=torch.float32, device=dev)
        partial = torch.empty((int(L.pinsage_gat_partial_rows(n_rows)), 2 * d), dtype=torch.float32, device=dev)
        da = torch.empty(2 * d, dtype=torch.float32, device=dev)
        nat.check(L.pinsage_gat_backward_rows(
            nat.ptr(h), h.stride(0), n_h, d, nat.ptr(a), nat.ptr(rows_u), n_rows, nat.ptr(segT), nat.ptr(entT),
            nat.ptr(segofT), nat.ptr(own_ptr), nat.ptr(own_seg), nat.ptr(p), nat.ptr(de), nat.ptr(s), nnz, n_seg,
            nat.ptr(dout), dout.stride(0), nat.ptr(dh), dh.stride(0), nat.ptr(coef), nat.ptr(partial), nat.ptr(da),
            nat.stream_ptr()), "gat_backward_rows")
        return dh, da.reshape(ctx.weight_shape), None, None, None, None, None


def gat_segments(h, weight, seg_ptr, hrows, c, own):
    """The fused edge softmax + gather over a CSR given as numpy arrays
    (seg_ptr int64 [F+1]; hrows, own: rows of ``h``; c float32 >= 0), with the
    attention row ``weight`` [1, 2d]: float32 [F, d] on the GPU, differentiable
    w.r.t. ``h`` and ``weight``.  Entries whose row is outside ``h`` are
    skipped, as in ``pinsage_segment_wmean``."""
    dev = h.device

    def to(x, dtype):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev)

    plan = tuple(to(x, x.dtype) for x in gat_plan(seg_ptr, hrows, own, len(h)))
    return _GatAggregate.apply(h, weight, to(seg_ptr, np.int64), to(hrows, np.int32), to(c, np.float32),
                               to(own, np.int32), plan)


def gat_aggregate(nodes, pre_hidden_embs, pre_neighs, adj_matrix, attention):
    """``GNN_model.aggregate`` with gat=True, agg_func 'MEAN'
    (GNNs_unsupervised.py:537-567, 576-577): a softmax over each node's whole
    neighbourhood (the node itself included) of
    ``leaky_relu(att([h_node || h_neighbour]), 0.2) * sqrt(edge count)``,
    zero scores dropped, times the embeddings: float32 [len(nodes), d] on the
    GPU.  Gradients flow to ``pre_hidden_embs`` and to the attention weight the
    reference's ``Attention.forward`` selects (``attention_raw`` when the width
    is ``input_size``, else ``attention_emb`` when it is ``out_size``); a width
    that is neither raises ValueError.  The softmax is shifted by the row
    maximum (the one departure from the reference's unshifted exp)."""
    unique_nodes_list, _, unique_nodes = pre_neighs
    h = pre_hidden_embs
    if not torch.is_tensor(h):
        h = torch.as_tensor(np.asarray(h))
    att = select_attention(attention, h.shape[1])
    dev = nat.device()
    seg_ptr, cols, w = mask_csr(nodes, pre_neighs, adj_matrix, gat=True)
    if h.dtype != torch.float32 or h.device != dev or not h.is_contiguous():
        h = h.to(device=dev, dtype=torch.float32).contiguous()
    own = np.fromiter((unique_nodes[n] for n in nodes), np.int64, count=len(nodes))
    if len(h) == len(unique_nodes):
        hrows = cols
    else:
        ulist = np.asarray(unique_nodes_list, np.int64)
        hrows, own = ulist[cols], ulist[own]
    for r in (hrows, own):
        if len(r) and (r.min() < 0 or r.max() >= len(h)):
            raise IndexError("aggregate: neighbour row out of range of pre_hidden_embs")
    return gat_segments(h, att.weight.to(device=dev, dtype=torch.float32), seg_ptr, hrows, w, own)


def mean_aggregate(nodes, pre_hidden_embs, pre_neighs, adj_matrix, gcn=False, gat=False, attention=None):
    """``GNN_model.aggregate`` with agg_func 'MEAN' (GNNs_unsupervised.py:537-588):
    returns ``mask.mm(embed_matrix)`` as float32 [len(nodes), d] on the GPU,
    differentiable w.r.t. ``pre_hidden_embs``.  ``embed_matrix`` is
    ``pre_hidden_embs`` itself when it has exactly len(unique_nodes) rows (the
    reference's shortcut at :546-549), otherwise its unique-node rows.
    ``gat=True`` needs the ``attention`` module and is ``gat_aggregate``."""
    if gat:
        if attention is None:
            raise ValueError("mean_aggregate(gat=True) needs attention=Attention(input_size, out_size): "
                             "the GAT mask is a function of its weights")
        return gat_aggregate(nodes, pre_hidden_embs, pre_neighs, adj_matrix, attention)
    dev = nat.device()
    unique_nodes_list, _, unique_nodes = pre_neighs
    seg_ptr, cols, w = mask_csr(nodes, pre_neighs, adj_matrix, gcn=gcn)
    h = pre_hidden_embs
    if not torch.is_tensor(h):
        h = torch.as_tensor(np.asarray(h))
    if h.dtype != torch.float32 or h.device != dev or not h.is_contiguous():
        h = h.to(device=dev, dtype=torch.float32).contiguous()
    if len(h) == len(unique_nodes):
        hrows = cols
    else:
        hrows = np.asarray(unique_nodes_list, np.int64)[cols]
    if len(hrows) and (hrows.min() < 0 or hrows.max() >= len(h)):
        raise IndexError("aggregate: neighbour row out of range of pre_hidden_embs")
    fwd_T = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                  for a in _transpose(seg_ptr, hrows, w, len(h)))
    return _SegmentWMean.apply(h, torch.from_numpy(seg_ptr).to(dev),
                               torch.from_numpy(hrows.astype(np.int32)).to(dev),
                               torch.from_numpy(w.astype(np.float32)).to(dev), len(nodes), fwd_T)


class MeanAggregator:
    """The aggregation half of ``GNN_model`` (GNNs_unsupervised.py:467-588) for
    agg_func 'MEAN': holds the adjacency matrix / lists and the gcn flag, and
    exposes the reference's ``_get_unique_neighs_list`` and ``aggregate``."""

    def __init__(self, adj_matrix, adj_lists, gcn=False, num_sample=10):
        self.adj_matrix = adj_matrix
        self.adj_lists = adj_lists
        self.gcn = gcn
        self.gat = False
        self.agg_func = "MEAN"
        self.num_sample = num_sample

    def _get_unique_neighs_list(self, nodes, num_sample=None):
        return get_unique_neighs_list(self.adj_lists, nodes, self.num_sample if num_sample is None
                                      else num_sample, gcn=self.gcn, gat=self.gat)

    def aggregate(self, nodes, pre_hidden_embs, pre_neighs):
        return mean_aggregate(nodes, pre_hidden_embs, pre_neighs, self.adj_matrix, gcn=self.gcn)


class GatAggregator(MeanAggregator):
    """The aggregation half of ``GNN_model`` with gat=True: full neighbourhoods
    (no sampling) and the attention softmax of ``gat_aggregate``; ``attention``
    is the model's ``Attention`` module."""

    def __init__(self, adj_matrix, adj_lists, attention):
        super().__init__(adj_matrix, adj_lists, gcn=False)
        self.gat = True
        self.attention = attention

    def aggregate(self, nodes, pre_hidden_embs, pre_neighs):
        return mean_aggregate(nodes, pre_hidden_embs, pre_neighs, self.adj_matrix, gat=True,
                              attention=self.attention)
