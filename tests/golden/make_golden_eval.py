"""Generate tests/golden/eval_metrics.npz by running the REAL reference's
accuracy metrics (eval.py:227-250 hit_rate / mrr, :376-389 low_degree_accuracy).

Runs only where the reference checkout is (as make_golden.py does; no test
needs it).  eval.py is imported as it is; the libraries it names that are not installed (dgl,
torchvision, wandb, implicit, fastnode2vec, and the lib.gnns package of the
other baselines) are replaced by empty stub modules: the metrics touch none.

The fixture is data only: a seeded 400 x 60 id matrix (what load_knn returns,
list_len = 60), 300 positive pairs, in-degrees of a stand-in graph, and the
reference's results.  The pairs include positives in column 0, in column K - 1
and column K for K in {1, 10, 60}, absent positives, pos == q (absent, and once
present), and a repeated pair.

    python tests/golden/make_golden_eval.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"  # the same place make_golden.py reads

N_NODES, LIST_LEN, N_PAIRS = 400, 60, 300
HR_KS = (1, 10, 60, 100)
MRR_KS = (10, 60, 1000)
MRR_SCALINGS = (1, 10)
LOW_DEGREE_THRS = (-1, 0, 1)  # -1: no node that low (the reference returns 0)


def _import_reference_eval():
    sys.dont_write_bytecode = True  # the reference tree is read-only: no __pycache__ there
    for name in ("dgl", "wandb", "implicit", "fastnode2vec", "torchvision", "torchvision.io",
                 "torchvision.io.image", "lib", "lib.gnns", "lib.gnns.GNNs_unsupervised"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["dgl"].DGLGraph = object
    sys.modules["torchvision"].io = sys.modules["torchvision.io"]
    sys.modules["torchvision.io"].image = sys.modules["torchvision.io.image"]
    sys.modules["torchvision.io.image"].ImageReadMode = object
    sys.modules["lib.gnns.GNNs_unsupervised"].GNN = object
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import eval as ref_eval  # noqa: E402
    return ref_eval


class DegreeGraph:
    """The stand-in graph: it only answers in_degrees."""

    def __init__(self, deg):
        self.deg = torch.as_tensor(deg)

    def in_degrees(self, v):
        return self.deg[v]


def make_inputs():
    rng = np.random.default_rng(2024)
    knn = np.empty((N_NODES, LIST_LEN), np.int64)
    for q in range(N_NODES):  # distinct ids, the query itself excluded (as a kNN list is)
        knn[q] = rng.permutation(np.delete(np.arange(N_NODES), q))[:LIST_LEN]
    knn[33, 5] = 33           # one list that does hold its own query
    pairs = []
    qs = rng.permutation(N_NODES)
    for i, col in enumerate([0] * 6 + [1] * 4 + [9] * 4 + [10] * 4 + [59] * 4):
        pairs.append((qs[i], knn[qs[i], col]))
    for q in qs[30:60]:       # absent positives
        absent = np.setdiff1d(np.arange(N_NODES), np.append(knn[q], q))
        pairs.append((q, rng.choice(absent)))
    pairs += [(q, q) for q in qs[60:66]] + [(33, 33)]   # pos == q: absent, and once present
    pairs += [pairs[0], pairs[12], pairs[12], pairs[35]]  # repeated pairs
    while len(pairs) < N_PAIRS:   # the rest: half from the list at a random column, half any id
        q = int(rng.integers(0, N_NODES))
        pairs.append((q, knn[q, rng.integers(0, LIST_LEN)] if rng.random() < 0.5 else rng.integers(0, N_NODES)))
    pairs = np.array(pairs, np.int64)[rng.permutation(N_PAIRS)]
    deg = rng.integers(0, 6, N_NODES).astype(np.int64)
    return knn, pairs, deg


def main():
    ref = _import_reference_eval()
    knn, pairs, deg = make_inputs()
    km, tp, g = torch.from_numpy(knn), torch.from_numpy(pairs), DegreeGraph(deg)
    out = dict(knn_mat=knn.astype(np.int16), test_positives=pairs.astype(np.int16), in_degrees=deg.astype(np.int8),
               hr_ks=np.array(HR_KS), mrr_ks=np.array(MRR_KS), mrr_scalings=np.array(MRR_SCALINGS),
               low_degree_thrs=np.array(LOW_DEGREE_THRS))
    out["hit_rate"] = np.array([ref.hit_rate(km, tp, K) for K in HR_KS], np.float64)
    out["mrr"] = np.array([[ref.mrr(km, tp, K, s) for s in MRR_SCALINGS] for K in MRR_KS], np.float64)
    # compute_results_table's call (eval.py:429-430: K = 1000, mrr) and the same with hit_rate at K = 10
    out["low_degree_mrr_1000"] = np.array(
        [ref.low_degree_accuracy(km, g, tp, 1000, degree_thr=t, acc_func=ref.mrr) for t in LOW_DEGREE_THRS], np.float64)
    out["low_degree_hit_rate_10"] = np.array(
        [ref.low_degree_accuracy(km, g, tp, 10, degree_thr=t, acc_func=ref.hit_rate) for t in LOW_DEGREE_THRS],
        np.float64)
    path = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
    for k in ("hit_rate", "mrr", "low_degree_mrr_1000", "low_degree_hit_rate_10"):
        print(k, out[k].tolist())


if __name__ == "__main__":
    main()
