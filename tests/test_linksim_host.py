"""Host checks of the link-prediction indices: the exports of the weighted
co-occurrence entries, adamic_adar_weights, and the numpy restatement
(tests/linksim_util.py) against networkx's recorded output
(tests/golden/linksim.npz, made by tests/golden/make_golden_linksim.py).

Jaccard and preferential cells are compared bit for bit.  An Adamic-Adar cell
is a sum of cn terms each rounded to half a unit of 2^-30, then rounded once to
float32, against networkx's float64 sum rounded once to float32:
    |got - ref32| <= cn 2^-31 + 2^-23 |ref|.
networkx raises on (q, q) where q has a neighbour of degree 1; those cells are
NaN in the fixture, and the weight of such a neighbour is 0 here.
"""
import os
import re

import numpy as np
import pytest
import torch

import jaccard_util as ju
import linksim_util as lu
from conftest import REPO, golden

NAMES = ("pinsage_cooc_weighted_tile", "pinsage_cooc_weighted_scratch_bytes", "pinsage_cooc_weighted_sums",
         "pinsage_cooc_weighted_knn")


def test_exports():
    import _native as nat
    import baselines as bl
    txt = open(os.path.join(REPO, "include", "pinsage_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = nat.lib()
    for name in NAMES:
        assert name in nat.EXPORTED and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in the header"
    # the binding's argument count is the header's
    for name in NAMES:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt).group(1).strip()
        n_args = 0 if decl == "void" else len(decl.split(","))
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("SimpleSimilarity", "JaccardIndex", "AdamicAdar", "Preferential", "adamic_adar_weights",
                 "LINKSIM_SHIFT"):
        assert name in bl.__all__
    assert bl.LINKSIM_SHIFT == lu.SHIFT == 30
    assert "networkx similarities" not in bl.__doc__         # no longer listed as out of scope
    tile = int(L.pinsage_cooc_weighted_tile())
    assert tile >= 1024 and tile * 8 <= 64 * 1024
    n = 1000
    assert L.pinsage_cooc_weighted_scratch_bytes(n, 3) >= 3 * n * 4
    assert L.pinsage_cooc_weighted_scratch_bytes(n, 0) == L.pinsage_cooc_weighted_scratch_bytes(n, 1)


def test_adamic_adar_weights():
    import baselines as bl
    d = np.array([0, 1, 2, 3, 1000, 2 ** 31 - 1], np.int64)
    got = bl.adamic_adar_weights(torch.from_numpy(d))
    assert got.dtype == torch.int64 and got.device.type == "cpu" and tuple(got.shape) == (6,)
    got = got.numpy()
    want = lu.weights(d)
    assert got[0] == 0 and got[1] == 0 and want[0] == 0 and want[1] == 0
    assert (np.abs(got - want) <= 1).all(), (got, want)
    assert want[2] == int(np.floor(2.0 ** 30 / np.log(2.0) + 0.5)) and (got[2:] > 0).all()
    assert (np.diff(got[2:]) < 0).all()                     # a larger middle node weighs less
    assert bl.adamic_adar_weights([5, 1]).tolist() == [int(lu.weights([5])[0]), 0]


@pytest.fixture(scope="module")
def fix():
    f = golden("linksim")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    member = ju.memberships(n, nc, f["edges"].astype(np.int64))
    return f, {"bip": member, "proj": lu.projected(member)}, f["queries"].astype(np.int64)


def test_fixture_holds_its_cases(fix):
    f, adjs, q = fix
    member = adjs["bip"]
    assert member.shape == (42, 300) and len(q) >= 40 and f["aa_bip"].dtype == np.float32
    assert f["jc_proj"].dtype == np.float32 and f["pa_bip"].dtype == np.int64
    deg = member.sum(0)
    assert (member.sum(1) == 1).any()                       # a collection of one track
    pair = np.flatnonzero(member[member.sum(1) == 2][-1])
    assert len(pair) == 2 and (deg[pair] == 1).all()        # two tracks in one collection and nothing else
    assert (deg[q] == 0).any() and member[0, q].any() and set(pair.tolist()) <= set(q.tolist())


@pytest.mark.parametrize("tag", ["bip", "proj"])
def test_restatement_against_networkx(fix, tag):
    f, adjs, q = fix
    adj = adjs[tag]
    # Jaccard and preferential attachment: bit for bit
    assert np.array_equal(ju.bits(lu.jaccard(adj, q)), ju.bits(f[f"jc_{tag}"]))
    assert np.array_equal(lu.preferential(adj, q), f[f"pa_{tag}"])
    # Adamic-Adar: within the derived bound; NaN exactly where networkx raised
    ref = f[f"aa_{tag}"]
    dmid = adj.sum(1)
    got = lu.to_score(lu.sums(adj, lu.weights(dmid), q))
    cn = lu.common(adj, q)
    has_leaf = (adj[dmid == 1].sum(0) > 0)                  # tracks with a neighbour of degree 1
    want_nan = np.zeros(ref.shape, bool)
    rows = np.flatnonzero(has_leaf[q])
    want_nan[rows, q[rows]] = True
    assert want_nan.sum() >= 1 and np.array_equal(np.isnan(ref), want_nan)
    ok = ~want_nan
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(f"{tag}: largest Adamic-Adar error {err[ok].max():.3g} at score "
          f"{ref[ok][err[ok].argmax()]:.4g}; {np.mean(ju.bits(got)[ok] == ju.bits(ref)[ok]):.4%} of cells bit-equal")
    assert (err[ok] <= lu.aa_bound(cn, ref)[ok]).all()
    assert np.isfinite(got).all() and (got >= 0).all() and got.max() > 1
    # a degree-1 neighbour weighs 0: the diagonal cell is the sum over the others
    for r in rows:
        others = adj[:, q[r]] & (dmid >= 2)
        assert got[r, q[r]] == lu.to_score(lu.weights(dmid)[others].sum())
