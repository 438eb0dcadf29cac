"""Generate tests/golden/beyond_accuracy.npz by running the REAL reference's
beyond-accuracy metrics (eval.py:271-312 intra_diversity / inter_diversity,
:342-374 coverage / average_degree / degree_dist).

Runs only where the reference checkout is (as make_golden_eval.py does, with
the same stub imports; no test needs it).

The fixture is data only: a seeded 400 x 60 id matrix drawn with a popularity
skew (so that coverage is neither 0 nor 1), a 400 x 24 float32 feature table,
300 positive pairs (coverage with all_nodes=False reads them), in-degrees in
0 .. 50 of a stand-in graph, and the reference's results.  One list repeats an
id inside its first 10 columns, one list holds its own query.
inter_diversity is given the id matrix as a numpy array (scipy's lil_matrix
rejects a tensor index); its pairs come from numpy's global generator, seeded
per K, and the next draw after each call is recorded too.

    python tests/golden/make_golden_beyond.py
"""
from __future__ import annotations

import os

import numpy as np
import torch

from make_golden_eval import DegreeGraph, _import_reference_eval

HERE = os.path.dirname(os.path.abspath(__file__))

N_NODES, LIST_LEN, DIM, N_POS = 400, 60, 24, 300
INTRA_KS = (1, 10, 60, 100)
INTER_KS = (1, 10, 60)
INTER_SEEDS = (7, 8, 9)
INTER_PAIRS = 2000
COV_KS = (1, 10, 59, 100)
DEG_KS = (1, 10, 100)
NEXT_DRAW_HIGH = 1 << 30
REPEAT_ROW, OWN_ROW = 5, 33


def make_inputs():
    rng = np.random.default_rng(2025)
    p = 1.0 / (np.arange(N_NODES) + 1.0) ** 1.5   # popularity by rank
    p /= p.sum()
    by_rank = rng.permutation(N_NODES)           # which id holds each popularity rank
    knn = np.empty((N_NODES, LIST_LEN), np.int64)
    for q in range(N_NODES):                     # distinct ids per list, as a kNN list has
        knn[q] = by_rank[rng.choice(N_NODES, LIST_LEN, replace=False, p=p)]
    knn[REPEAT_ROW, 7] = knn[REPEAT_ROW, 3]      # a repeated id inside the first 10 columns
    if OWN_ROW not in knn[OWN_ROW]:
        knn[OWN_ROW, 5] = OWN_ROW                # a list that holds its own query
    feats = rng.standard_normal((N_NODES, DIM)).astype(np.float32)
    pairs = rng.integers(0, N_NODES // 2, (N_POS, 2)).astype(np.int64)
    deg = rng.integers(0, 51, N_NODES).astype(np.int64)
    return knn, feats, pairs, deg


def main():
    ref = _import_reference_eval()
    knn, feats, pairs, deg = make_inputs()
    km, tp, g, f = torch.from_numpy(knn), torch.from_numpy(pairs), DegreeGraph(deg), torch.from_numpy(feats)
    assert len(np.unique(knn[REPEAT_ROW, :10])) == 9 and OWN_ROW in knn[OWN_ROW]
    assert deg.min() >= 0 and deg.max() <= 50
    out = dict(knn_mat=knn.astype(np.int16), features=feats, test_positives=pairs.astype(np.int16),
               in_degrees=deg.astype(np.int8), intra_ks=np.array(INTRA_KS), inter_ks=np.array(INTER_KS),
               inter_seeds=np.array(INTER_SEEDS), inter_pairs=np.array(INTER_PAIRS), cov_ks=np.array(COV_KS),
               deg_ks=np.array(DEG_KS), next_draw_high=np.array(NEXT_DRAW_HIGH))
    out["intra_diversity"] = np.array([ref.intra_diversity(km, tp, K, f) for K in INTRA_KS], np.float64)
    inter, nxt = [], []
    for K, s in zip(INTER_KS, INTER_SEEDS):
        np.random.seed(s)
        inter.append(ref.inter_diversity(knn, tp, K, N_NODES, n_pairs=INTER_PAIRS))
        nxt.append(np.random.randint(0, NEXT_DRAW_HIGH))
    out["inter_diversity"] = np.array(inter, np.float64)
    out["inter_next_draw"] = np.array(nxt, np.int64)
    out["coverage_all"] = np.array([ref.coverage(km, tp, K=K) for K in COV_KS], np.float64)
    out["coverage_positives"] = np.array([ref.coverage(km, tp, K=K, all_nodes=False) for K in COV_KS], np.float64)
    cov10 = out["coverage_all"][COV_KS.index(10)]
    assert 0.2 < cov10 < 0.9, f"coverage at K = 10 is {cov10}: the skew tests nothing"
    out["average_degree"] = np.array([ref.average_degree(km, g, tp, K) for K in DEG_KS], np.float64)
    for K in DEG_KS:
        vals, counts = ref.degree_dist(km, g, tp, K)
        out[f"degree_dist_vals_{K}"] = vals.numpy().astype(np.int8)
        out[f"degree_dist_counts_{K}"] = counts.numpy().astype(np.int32)
    path = os.path.join(HERE, "beyond_accuracy.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
    for k in ("intra_diversity", "inter_diversity", "inter_next_draw", "coverage_all", "coverage_positives",
              "average_degree"):
        print(k, out[k].tolist())


if __name__ == "__main__":
    main()
