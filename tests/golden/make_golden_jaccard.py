"""Generate tests/golden/jaccard.npz by running the REAL reference's JaccardFast
(baselines.py:194-220 over to_col_track_matrix, :402-413) on a graph.CSRGraph.

Runs only where the reference checkout is (as make_golden_eval.py does, with
the same stub imports; no test needs it).  ``knn`` is given its nodeset as a
numpy array: scipy's matrix index rejects a tensor.

The fixture is data only: the edges of a seeded graph of 300 tracks and 40
collections, and the reference's nbh_sizes, dense intersect_sizes rows of all
tracks and knn output at k = 2 and k = 50.  The graph has one hub collection of
125 tracks, one collection whose edges are all listed twice, 46 or more tracks
in no collection, two tracks with identical collection sets, one membership
stored only as track -> collection and one only as
collection -> track (every other membership is stored both ways).

    python tests/golden/make_golden_jaccard.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from make_golden_eval import _import_reference_eval

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

N_TRACKS, N_COLS = 300, 40
HUB, HUB_SIZE, DUP_COL = 0, 125, 1
TWINS, TWIN_COLS = (250, 251), (5, 17, 29)
ONLY_T2C, ONLY_C2T = (252, 7), (253, 8)   # (track, collection)
N_FREE = 255                              # tracks from here on are in no collection
KS = (2, 50)


def make_edges():
    rng = np.random.default_rng(2026)
    pairs = set()                          # (track, collection)
    for t in rng.choice(250, HUB_SIZE, replace=False).tolist():
        pairs.add((t, HUB))
    for c in range(1, N_COLS):
        for t in rng.choice(250, int(rng.integers(2, 16)), replace=False).tolist():
            pairs.add((t, c))
    for t in TWINS:
        for c in TWIN_COLS:
            pairs.add((t, c))
    edges = []
    for t, c in sorted(pairs):
        edges += [(t, N_TRACKS + c), (N_TRACKS + c, t)]
        if c == DUP_COL:
            edges += [(t, N_TRACKS + c), (N_TRACKS + c, t)]
    edges.append((ONLY_T2C[0], N_TRACKS + ONLY_T2C[1]))
    edges.append((N_TRACKS + ONLY_C2T[1], ONLY_C2T[0]))
    edges = np.array(edges, np.int64)
    return edges[rng.permutation(len(edges))]


def main():
    _import_reference_eval()
    import baselines as ref_baselines      # the reference's: its directory leads sys.path
    assert os.path.dirname(os.path.abspath(ref_baselines.__file__)) != os.path.join(REPO, "gcn-song-embeddings_amd")
    sys.path.append(os.path.join(REPO, "gcn-song-embeddings_amd"))
    import graph

    edges = make_edges()
    g = graph.CSRGraph(N_TRACKS + N_COLS, edges[:, 0], edges[:, 1])
    ids = list(range(N_TRACKS))
    model = ref_baselines.JaccardFast()
    model.train(g, ids, None, None, None)
    nbh = np.asarray(model.nbh_sizes)
    inter = np.asarray(model.intersect_sizes.toarray())
    assert inter.shape == (N_TRACKS, N_TRACKS) and inter.max() < 128 and nbh.max() < 128
    assert (nbh[N_FREE:] == 0).all() and (nbh == 0).sum() >= 5
    assert (inter[TWINS[0]] == inter[TWINS[1]]).all() and nbh[TWINS[0]] == len(TWIN_COLS)
    assert nbh[ONLY_T2C[0]] == 1 and nbh[ONLY_C2T[0]] == 1
    out = dict(n_tracks=np.array(N_TRACKS), n_cols=np.array(N_COLS), edges=edges.astype(np.int16),
               nbh_sizes=nbh.astype(np.int8), intersect_sizes=inter.astype(np.int8), ks=np.array(KS))
    nodeset = np.arange(N_TRACKS)
    for k in KS:
        w, n = model.knn(nodeset, k)
        assert w.dtype == torch.float32 and tuple(w.shape) == (N_TRACKS, k - 1)
        out[f"knn_w_{k}"] = w.numpy()
        out[f"knn_n_{k}"] = n.numpy().astype(np.int16)
    path = os.path.join(HERE, "jaccard.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB); {len(edges)} edges, "
          f"{int((nbh == 0).sum())} tracks in no collection, largest degree {int(nbh.max())}")


if __name__ == "__main__":
    main()
