"""The early-stop sampler's numpy restatement (tests/earlystop_util.py) against the
reference's fixtures (tests/golden/earlystop_*.npz, written by
make_golden_earlystop.py from pinsage_model.py:55-86) and against a plain
hop-by-hop loop, and the C-ABI entry's presence.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden

import earlystop_util as eu


@pytest.mark.parametrize("gname", ["small", "mid"])
def test_restatement_reproduces_reference_fixture(gname):
    """values, indices and the words consumed (the next draws), bit for bit, in
    every stored configuration; the fixture is not vacuous."""
    from oracle import oracle as orc
    d = golden("earlystop_" + gname)
    n_items, nodeset, seed = int(d["n_tracks"]), d["nodeset"], int(d["seed"])
    some_mixed = some_all = False
    assert len(d["configs"]) == (7 if gname == "small" else 9)
    for c, (n_hops, T, stop_np, stop_nv) in enumerate(d["configs"].tolist()):
        assert T * 64 <= n_items
        torch.manual_seed(seed)
        mt = orc.MT.from_torch()
        r = eu.reference(d["indptr"], d["indices"], n_items, nodeset, n_hops, float(d["alpha"]), T, stop_np, stop_nv,
                         mt=mt)
        what = f"{gname} {n_hops, T, stop_np, stop_nv}"
        assert (r["w"].view(np.uint64) == d[f"c{c}_val"].view(np.uint64)).all(), what
        assert (r["nb"] == d[f"c{c}_idx"]).all(), what
        assert (r["hops"] == d[f"c{c}_hops"]).all(), what
        mt.to_torch()
        assert ([int(torch.randint(2 ** 31, ())) for _ in range(4)] == d[f"c{c}_after"]).all(), what
        assert r["words"] == sum(eu.words_consumed(int(L), bool(s), n_hops) for L, s in zip(r["hops"], r["stopped"]))
        n_stop = int(r["stopped"].sum())
        if stop_np == 0 or stop_nv == 0:
            assert n_stop == 0
        some_mixed |= 0 < n_stop < len(nodeset)
        some_all |= n_stop == len(nodeset)
    assert some_mixed and some_all


def _loop_length(trace, stop_np, stop_nv):
    """pinsage_model.py:62-78's counting, hop by hop"""
    counts = {}
    term = 0
    for j, item in enumerate(trace):
        counts[item] = counts.get(item, 0) + 1
        if counts[item] == stop_nv:
            term += 1
            if term == stop_np:
                return j + 1, True
    return len(trace), False


def test_stop_length_matches_plain_loop():
    rng = np.random.default_rng(5)
    n_stopped = 0
    for _ in range(600):
        n = int(rng.integers(1, 140))
        t = rng.integers(0, int(rng.integers(1, 12)), n).tolist()
        stop_np, stop_nv = int(rng.integers(-1, 6)), int(rng.integers(-1, 8))
        got, want = eu.stop_length(t, stop_np, stop_nv), _loop_length(t, stop_np, stop_nv)
        assert got == want, (t, stop_np, stop_nv, got, want)
        n_stopped += want[1]
    assert n_stopped > 100
    # a stop on the very last hop, and events that come one hop too late
    for t, stop_np, stop_nv, want in (([0, 1, 0], 1, 2, (3, True)), ([0, 1, 0, 1], 2, 2, (4, True)),
                                      ([0, 1, 0, 1], 3, 2, (4, False)), ([4], 1, 1, (1, True)),
                                      ([4, 4, 4], 1, 4, (3, False)), ([0, 1, 2, 1, 2, 0], 2, 2, (5, True))):
        assert eu.stop_length(t, stop_np, stop_nv) == want == _loop_length(t, stop_np, stop_nv), (t, stop_np, stop_nv)
    # a stop on the last hop consumes one word less than no stop at the same length
    assert eu.words_consumed(7, True, 7) == 20 and eu.words_consumed(7, False, 7) == 21


def test_abi_entry_and_argument_count():
    import _native
    assert "pinsage_ppr_topk_early_stop" in _native.EXPORTED
    assert "pinsage_ppr_topk_early_stop_workspace" in _native.EXPORTED
    L = _native.lib()
    assert len(L.pinsage_ppr_topk_early_stop.argtypes) == 25
    assert L.pinsage_ppr_topk_early_stop.restype is ctypes.c_int
    txt = open(os.path.join(REPO, "include", "pinsage_hip.h")).read()
    m = re.search(r"int pinsage_ppr_topk_early_stop\((.*?)\);", txt, flags=re.S)
    assert m and len(m.group(1).split(",")) == 25
    # the workspace covers the full sampler's plus the hops and the words consumed
    for mt in (0, 1):
        assert L.pinsage_ppr_topk_early_stop_workspace(100, 500, mt) >= L.pinsage_ppr_topk_workspace(100, 500, mt) + 400
