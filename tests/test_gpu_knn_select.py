"""pinsage_knn_cosine's per-row selection (knn_select_kernel, csrc/knn.hip) in
every regime, id for id and bit for bit.

The kernel has four exits: the one-pass fast path (a threshold from the row's
first 4096 keys, candidates in 16 per-wave LDS segments of 512, radix select
and bitonic sort over them), and the whole-row three-pass radix select with
ordered tie compaction, entered when the pass found fewer than k candidates
('few'), a wave's segment overflowed ('segment'), or more than 4096 keys reach
the k-th ('ties').  i.i.d. Gaussian tables with k <= 1001 (test_gpu_baselines)
only take the first.

The tables here make every similarity exactly computable in fp32 (see
parity_util: integer rows, probe queries, one IEEE division per key), so the
expected result -- similarity descending, then index ascending, the rule
include/pinsage_hip.h documents -- is compared without a tolerance.  Each case
asserts, before the launch, the exit the replay of the kernel's decision
(parity_util.knn_select_regime) predicts: a retuned constant then shows as a
case that lost its regime, not as a pass that tests nothing.  The same cases
run on the host in tests/test_host.py.
"""
import numpy as np
import pytest
import torch

import parity_util as pu

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE = -2, -3  # pinsage_status (include/pinsage_hip.h)


def _knn(emb, q, k):
    import baselines
    # (the shared tables are read-only: hand torch a copy)
    w, ids = baselines._knn_cosine(torch.from_numpy(np.array(emb)), torch.from_numpy(np.array(q, np.int64)), k)
    return w.numpy(), ids.numpy()


@pytest.mark.parametrize("case", pu.KNN_SELECT_CASES, ids=[c[0] for c in pu.KNN_SELECT_CASES])
def test_knn_select_exact(case):
    emb, _, q, k, _, ref_w, ref_ids = pu.knn_select_case(case)  # asserts the case's exit
    w, ids = _knn(emb, q, k)
    pu.check_knn_select(w, ids, ref_w, ref_ids)


def _mixed_call():
    """Queries (1,0..), (-1,0..), zero, (2,0..), (1,0..) on the descending table:
    the few, segment, segment, few and few exits in one launch."""
    emb, p = pu.knn_select_table("desc")
    q = np.array([p["p1"], p["m1"], p["zero"], p["p2"], p["p1"]], np.int64)
    sim, ref_w, ref_ids = pu.knn_select_reference(emb, q, 1000)
    assert [pu.knn_select_regime(s, 1000) for s in sim] == ["few", "segment", "segment", "few", "few"]
    return emb, q, ref_w, ref_ids


def test_knn_select_mixed_exits_in_one_launch():
    emb, q, ref_w, ref_ids = _mixed_call()
    w, ids = _knn(emb, q, 1000)
    pu.check_knn_select(w, ids, ref_w, ref_ids)
    assert np.array_equal(w[3].view(np.int32), w[0].view(np.int32)) and np.array_equal(ids[3], ids[0])
    assert np.array_equal(w[4].view(np.int32), w[0].view(np.int32)) and np.array_equal(ids[4], ids[0])


@pytest.mark.parametrize("rows", [2, 3])
def test_knn_select_batches_with_a_short_last_batch(monkeypatch, rows):
    """Scratch sized by baselines._knn_cosine for `rows` query rows.  The
    library's own batch estimate (launch_knn_cosine) is one row more cautious:
    rows == 2 runs five batches of one query, rows == 3 batches of 2, 2 and 1."""
    import baselines
    emb, q, ref_w, ref_ids = _mixed_call()
    n = emb.shape[0]
    monkeypatch.setattr(baselines, "KNN_SCRATCH_BYTES", 8 * n + rows * 4 * n)
    assert max(1, min(len(q), (baselines.KNN_SCRATCH_BYTES - 8 * n) // (4 * n))) == rows
    w, ids = _knn(emb, q, 1000)
    pu.check_knn_select(w, ids, ref_w, ref_ids)


def _capi(emb_dev, n, d, ld, q, k, scratch_bytes=None, rows=None):
    """pinsage_knn_cosine on device tensors with sentinel-filled outputs:
    (status, w, ids) after a synchronise."""
    import _native as nat
    L = nat.lib()
    qd = torch.as_tensor(np.asarray(q, np.int64)).cuda()
    nq = int(qd.numel())
    kk = max(1, int(k))
    w = torch.full((nq, kk), -7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((nq, kk), -7, dtype=torch.int64, device="cuda")
    full = int(L.pinsage_knn_scratch_bytes(n, rows or nq))
    scratch = torch.zeros(full, dtype=torch.uint8, device="cuda")
    rc = L.pinsage_knn_cosine(nat.ptr(emb_dev), n, d, ld, nat.ptr(qd), nq, int(k), 1e-16, nat.ptr(scratch),
                              full if scratch_bytes is None else int(scratch_bytes), nat.ptr(w), nat.ptr(ids),
                              nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, w.cpu().numpy(), ids.cpu().numpy()


def test_knn_select_strided_table_equals_dense():
    """Rows of stride ld = d + 8 with the padding set to a value that would
    show in any dot product or norm that read it."""
    emb, q, ref_w, ref_ids = _mixed_call()
    n, d = emb.shape
    dense = torch.from_numpy(np.array(emb)).cuda()
    padded = torch.full((n, d + 8), 7e6, dtype=torch.float32, device="cuda")
    padded[:, :d] = dense
    rc0, w0, ids0 = _capi(dense, n, d, d, q, 1000)
    rc1, w1, ids1 = _capi(padded, n, d, d + 8, q, 1000)
    assert rc0 == 0 and rc1 == 0
    pu.check_knn_select(w0, ids0, ref_w, ref_ids)
    pu.check_knn_select(w1, ids1, w0, ids0)


@pytest.mark.parametrize("name", ["random-k1000", "desc-k1000", "third-k1000"])
def test_knn_select_both_gemm_arithmetics(name):
    """fp32 MFMA (0) and split bf16 (1) give the same bits: the dots are exact in both."""
    import _native as nat
    lib = nat.lib()
    emb, _, q, k, _, ref_w, ref_ids = pu.knn_select_case(next(c for c in pu.KNN_SELECT_CASES if c[0] == name))
    old = lib.pinsage_gemm_get_prec()
    try:
        for prec in (0, 1):
            assert lib.pinsage_gemm_set_prec(prec) == 0
            w, ids = _knn(emb, q, k)
            pu.check_knn_select(w, ids, ref_w, ref_ids)
    finally:
        lib.pinsage_gemm_set_prec(old)


def test_knn_rejections_leave_the_outputs_untouched():
    import _native as nat
    emb, p = pu.knn_select_table("random:4100")
    n, d = 4100, pu.KNN_D
    big = torch.zeros((5000, d + 8), dtype=torch.float32, device="cuda")
    big[:n, :d] = torch.from_numpy(np.array(emb)).cuda()
    q = [p["p1"]]

    def refused(want, n_, d_, ld_, k, **kw):
        rc, w, ids = _capi(big, n_, d_, ld_, q, k, **kw)
        assert rc == want, (rc, nat.lib().pinsage_last_error())
        assert (w == -7.0).all() and (ids == -7).all()

    refused(ERR_ARG, n, d, d + 8, 0)
    refused(ERR_ARG, n, d, d + 8, n + 1)
    refused(ERR_ARG, 5000, d, d + 8, 4097)
    refused(ERR_ARG, n, 6, d + 8, 5)
    refused(ERR_ARG, n, d, d - 4, 5)       # ld < d
    refused(ERR_ARG, n, d, d + 7, 5)       # rows that do not start 16-byte aligned
    refused(ERR_WORKSPACE, n, d, d + 8, 5,
            scratch_bytes=int(nat.lib().pinsage_knn_scratch_bytes(n, 1)) - 256, rows=1)
    rc, w, ids = _capi(big, n, d, d + 8, q, 5)  # and the same call with valid arguments runs
    assert rc == 0
    _, ref_w, ref_ids = pu.knn_select_reference(emb, q, 5)
    pu.check_knn_select(w, ids, ref_w, ref_ids)


def test_knn_float_table_through_the_whole_row_select():
    """A Gaussian table at k_total = 4096: the realistic data path through the
    fallback (a wave owning two 1024-blocks overflows its segment), held to the
    float criteria of test_gpu_baselines against the oracle."""
    import baselines
    from oracle import oracle as orc
    rng = np.random.default_rng(11)
    emb = rng.standard_normal((20000, 128), dtype=np.float32)
    q = rng.integers(0, 20000, 8).astype(np.int64)
    w, ids = baselines.knn_from_emb(torch.from_numpy(emb), torch.from_numpy(q), 4095)
    rw, rn = orc.knn_from_emb(emb, q, 4095)
    sims = orc.cosine_sim_ab(torch.from_numpy(emb[q]), torch.from_numpy(emb)).numpy()
    assert all(pu.knn_select_regime(s, 4096) == "segment" for s in sims)
    pu.check_knn_close(w.numpy(), ids.numpy(), rw, rn, emb, q)
