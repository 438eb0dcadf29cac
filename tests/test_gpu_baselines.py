"""GPU parity of the evaluation-side paths next to the train step:
PersPageRank.knn (baselines.py:106-151) and knn_from_emb / cosine_sim_ab
(baselines.py:69-103), through the C-ABI.

PPR neighbours are integer/f64-count work: bit-exact against the reference's
fixtures, including how many MT19937 draws the walk consumed.  Cosine kNN is
fp32: the reference's similarities come from MKL's blocked sgemm, ours from
an MFMA fp32 FMA chain, so they differ in the last bits.  The test therefore
checks (a) the sorted top-k similarity values agree within 2e-6 absolute
(|cos| <= 1), (b) every returned neighbour's fp64 similarity matches the value
reported for it within 2e-6, and (c) no neighbour appears twice: neighbour ids
then differ from the reference's only among similarities that tie within the
tolerance (parity_util.check_knn_close).  Exact ties (duplicate rows) keep the
lower index here; torch's CPU topk orders them by libstdc++'s selection, which
is not replayed.  The documented rule itself (similarity descending, then index
ascending) and every exit of the selection kernel are checked id for id and bit
for bit in tests/test_gpu_knn_select.py, on tables whose similarities are exact.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from parity_util import check_knn_close as _check_knn

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _mt_mode():
    import pinsage_model as pm
    prev = pm.get_rng_mode()
    pm.set_rng_mode("mt19937")
    yield
    pm.set_rng_mode(prev)


def _graph(d):
    import graph
    return graph.CSRGraph.from_csr(d["indptr"], d["indices"])


def _after_ok(after):
    got = np.array([int(torch.randint(2 ** 31, ())) for _ in range(len(after))])
    return (got == after).all()


@pytest.mark.parametrize("gname", ["small", "mid"])
def test_ppr_knn_bit_exact(gname):
    import baselines
    d = golden(f"ppr_{gname}")
    m = baselines.PersPageRank()
    m.train(_graph(d), None, None, None, None)
    for k in d["ks"]:
        torch.manual_seed(int(d["seed"]) + int(k))
        tk = m.knn(torch.from_numpy(d["nodeset"]), int(k))
        assert (tk.values.numpy() == d[f"val_{k}"]).all(), k
        assert (tk.indices.numpy() == d[f"idx_{k}"]).all(), k
        assert _after_ok(d[f"after_{k}"]), k


@pytest.mark.parametrize("k", [50, 1000])
def test_knn_from_emb_vs_reference_fixture(k):
    import baselines
    d = golden("knn_emb")
    w, n = baselines.knn_from_emb(torch.from_numpy(d["emb"]), torch.from_numpy(d["q"]), k, None)
    assert w.device.type == "cpu" and w.dtype == torch.float32 and n.dtype == torch.int64
    frac = _check_knn(w.numpy(), n.numpy(), d[f"w_{k}"], d[f"n_{k}"], d["emb"], d["q"])
    assert frac < 0.05, frac


def test_knn_batches_and_duplicates_vs_oracle(monkeypatch):
    """Several query batches (small scratch), exact duplicate rows (ties at the
    k-th value), a zero row, d not a multiple of 4, queries on the GPU."""
    import baselines
    from oracle import oracle as orc
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((20000, 130), dtype=np.float32)
    emb[100:140] = emb[0:40]
    emb[7] = 0.0
    q = np.concatenate([np.arange(0, 50), rng.integers(0, 20000, 450)]).astype(np.int64)
    monkeypatch.setattr(baselines, "KNN_SCRATCH_BYTES", 16 << 20)  # ~200 rows per batch
    w, n = baselines.knn_from_emb(torch.from_numpy(emb).cuda(), torch.from_numpy(q).cuda(), 200)
    assert w.is_cuda
    rw, rn = orc.knn_from_emb(emb, q, 200)
    _check_knn(w.cpu().numpy(), n.cpu().numpy(), rw, rn, emb, q)


def test_knn_edge_sizes():
    import baselines
    rng = np.random.default_rng(6)
    emb = torch.from_numpy(rng.standard_normal((300, 16), dtype=np.float32))
    # k = n - 1: all rows but the first-ranked (itself)
    w, n = baselines.knn_from_emb(emb, torch.arange(300), 299)
    full = np.sort(n.numpy(), 1)
    for r in range(300):
        assert set(full[r].tolist()) == set(range(300)) - {r}
    # no queries
    w0, n0 = baselines.knn_from_emb(emb, torch.zeros(0, dtype=torch.int64), 5)
    assert w0.shape == (0, 5) and n0.shape == (0, 5)
    with pytest.raises(IndexError):
        baselines.knn_from_emb(emb, torch.tensor([300]), 5)
