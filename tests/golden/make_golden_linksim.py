"""Generate tests/golden/linksim.npz: networkx's adamic_adar_index,
jaccard_coefficient and preferential_attachment, called directly (what the
reference's SimpleSimilarity subclasses wrap, baselines.py:153-191; no
reference code is needed), on the symmetrised bipartite graph and on
bipartite.weighted_projected_graph of it.  Needs networkx; no test does.

The graph is make_golden_jaccard's (300 tracks, 40 collections: a hub of 125,
twins, tracks in no collection) plus two collections that put a neighbour of
degree 1 into both graphs: collection 40 holds track LONE_MEMBER alone (a
collection of degree 1 in the bipartite graph), collection 41 holds exactly
the two tracks PAIR, which are in nothing else (each the other's only
neighbour in the projected graph).  On the pair (q, q) of a track with such a
neighbour networkx raises ZeroDivisionError (1 / ln 1); the cell is stored NaN.

The fixture is data only: the edges, N_QUERIES query tracks and per graph
("bip", "proj") their score rows against all 300 tracks: aa_* and jc_* as
float32, which is what the reference's torch.tensor makes of networkx's Python
floats, pa_* as int64.

    python tests/golden/make_golden_linksim.py
"""
from __future__ import annotations

import os

import numpy as np

from make_golden_jaccard import HUB, N_COLS as N_COLS_BASE, N_TRACKS, TWINS, make_edges

HERE = os.path.dirname(os.path.abspath(__file__))
N_COLS = N_COLS_BASE + 2
LONE_COL, LONE_MEMBER = N_COLS_BASE, 3
PAIR_COL, PAIR = N_COLS_BASE + 1, (260, 261)
N_QUERIES = 40


def linksim_edges():
    extra = [(LONE_MEMBER, N_TRACKS + LONE_COL), (N_TRACKS + LONE_COL, LONE_MEMBER)]
    for t in PAIR:
        extra += [(t, N_TRACKS + PAIR_COL), (N_TRACKS + PAIR_COL, t)]
    return np.concatenate([make_edges(), np.array(extra, np.int64)])


def main():
    import networkx as nx
    from networkx.algorithms import bipartite

    edges = linksim_edges()
    one_track = (edges[:, 0] < N_TRACKS) ^ (edges[:, 1] < N_TRACKS)
    assert one_track.all()
    B = nx.Graph()
    B.add_nodes_from(range(N_TRACKS + N_COLS))
    B.add_edges_from(edges.tolist())
    tracks = list(range(N_TRACKS))
    P = bipartite.weighted_projected_graph(B, tracks)
    assert B.degree(N_TRACKS + LONE_COL) == 1 and all(B.degree(t) == 1 and P.degree(t) == 1 for t in PAIR)
    hub_member = min(B.neighbors(N_TRACKS + HUB))
    free = N_TRACKS - 1
    assert B.degree(free) == 0
    rng = np.random.default_rng(2027)
    special = [LONE_MEMBER, *PAIR, hub_member, free, *TWINS, 252, 253]
    rest = [t for t in rng.permutation(N_TRACKS).tolist() if t not in special]
    queries = np.array(sorted(special + rest[:N_QUERIES - len(special)]), np.int64)

    out = dict(n_tracks=np.array(N_TRACKS), n_cols=np.array(N_COLS), edges=edges.astype(np.int16),
               queries=queries.astype(np.int16))
    for tag, G in (("bip", B), ("proj", P)):
        aa = np.empty((len(queries), N_TRACKS), np.float32)
        jc = np.empty((len(queries), N_TRACKS), np.float32)
        pa = np.empty((len(queries), N_TRACKS), np.int64)
        for i, q in enumerate(queries.tolist()):
            pairs = [(q, t) for t in tracks]
            jc[i] = [p for _, _, p in nx.jaccard_coefficient(G, pairs)]
            pa[i] = [p for _, _, p in nx.preferential_attachment(G, pairs)]
            for t in tracks:  # one pair at a time: a pair that raises spoils no other
                try:
                    aa[i, t] = next(iter(nx.adamic_adar_index(G, [(q, t)])))[2]
                except ZeroDivisionError:
                    aa[i, t] = np.nan
        raised = np.argwhere(np.isnan(aa))
        assert len(raised) >= 1 and (queries[raised[:, 0]] == raised[:, 1]).all(), "networkx raises on (q, q) only"
        out[f"aa_{tag}"], out[f"jc_{tag}"], out[f"pa_{tag}"] = aa, jc, pa
        print(f"{tag}: {len(raised)} pairs raised; largest Adamic-Adar {np.nanmax(aa):.4f}, "
              f"largest preferential {int(pa.max())}")
    path = os.path.join(HERE, "linksim.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 256 * 1024
    print(f"wrote {path} ({size / 1024:.1f} KiB); {len(edges)} edges, {len(queries)} query rows")


if __name__ == "__main__":
    main()
