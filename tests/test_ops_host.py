"""tests/ops_util.py (the float64 references behind
tests/test_gpu_torch_ops_forms.py) on the CPU: each closed-form gradient equals
torch autograd of the same float64 expression to 1e-12 relative, the operand
layouts equal plain loops over gemm.h's index formulas, every exact-mode case
keeps every partial sum below 2^24, and each comparison rejects one planted
defect at a time: an element one ulp beyond its bound, a transposed operand, a
dropped bias, LeakyReLU's slope taken the wrong way at y == 0."""
import numpy as np
import pytest
import torch

import ops_util as ou
import parity_util as pu
from parity_util import SLOPE32

RTOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.linalg.norm(a - b) <= RTOL * np.linalg.norm(b), (np.linalg.norm(a - b), np.linalg.norm(b))


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


# ----------------------------------------------------------------------------- gradients against autograd
@pytest.mark.parametrize("lrelu", (False, True))
@pytest.mark.parametrize("with_b", (False, True))
@pytest.mark.parametrize("with_rows", (False, True))
def test_linear_reference_equals_autograd(with_rows, with_b, lrelu):
    for shape in ou.LINEAR_SHAPES[:2] + ou.LINEAR_SHAPES[3:]:
        for zeros in (False, True):
            c = ou.linear_inputs(shape, with_rows, with_b, zeros, 3, zeros=zeros)
            ref = ou.linear_reference(c["x"], c["rows"], c["W"], c["b"], lrelu, c["dy"])
            x, W = t64(c["x"]), t64(c["W"])
            b = t64(c["b"]) if with_b else None
            K = W.shape[1]
            a = x[torch.from_numpy(c["rows"]).long(), :K] if with_rows else x[:, :K]
            y = a @ W.t()
            if with_b:
                y = y + b
            if lrelu:
                y = torch.nn.functional.leaky_relu(y, SLOPE32)
            (y * t64(c["dy"], False)).sum().backward()
            close(ref["y"][0], y.detach().numpy())
            close(ref["dx"][0], x.grad.numpy())
            close(ref["dW"][0], W.grad.numpy())
            if with_b:
                close(ref["db"][0], b.grad.numpy())
            if zeros:
                assert (ref["y"][0] == 0).any()
            for want, bound in ref.values():
                assert np.shape(bound) == np.shape(want) and (np.asarray(bound) >= 0).all()


@pytest.mark.parametrize("with_rows", (False, True))
@pytest.mark.parametrize("shape", ou.CONCAT_SHAPES[:2] + ou.CONCAT_SHAPES[3:])
def test_concat_reference_equals_autograd(shape, with_rows):
    c = ou.concat_inputs(shape, with_rows, 5)
    ref = ou.concat_reference(c["h"], c["rows"], c["agg"], c["W"], c["b"], c["dy"])
    h, agg, W, b = (t64(c[k]) for k in ("h", "agg", "W", "b"))
    d, n = shape[0], shape[3]
    hs = h[torch.from_numpy(c["rows"]), :d] if with_rows else h[:n, :d]
    z = torch.nn.functional.leaky_relu(torch.cat([hs, agg], 1) @ W.t() + b, SLOPE32)
    nrm = z.norm(dim=1)
    y = z / nrm[:, None]
    (y * t64(c["dy"], False)).sum().backward()
    close(ref["y"][0], y.detach().numpy())
    close(ref["norms"][0], nrm.detach().numpy())
    for k, t in (("dh", h), ("dagg", agg), ("dW", W), ("db", b)):
        close(ref[k][0], t.grad.numpy())
    assert (ref["y"][0][:, 1] == 0).all()          # the planted exact zeros
    for want, bound in ref.values():
        assert np.shape(bound) == np.shape(want) and (np.asarray(bound) >= 0).all()


def test_agg_segment_and_row_references_equal_autograd_and_loops():
    for shape in ou.AGG_SHAPES[:3]:
        c = ou.agg_inputs(shape, False, 1)
        q = t64(c["q"])
        agg = (t64(c["w"], False)[:, :, None] * q[torch.from_numpy(c["loc"]).long()]).sum(1)
        (agg * t64(c["dagg"], False)).sum().backward()
        close(ou.weighted_agg_reference(c["q"], c["loc"], c["w"]), agg.detach().numpy())
        dq, bound = ou.agg_dq_reference(c["dagg"], c["loc"], c["w"], shape[3])
        close(dq, q.grad.numpy())
        if c["unnamed"] is not None:
            assert (dq[c["unnamed"]] == 0).all() and (bound[c["unnamed"]] == 0).all()
        assert len(set(c["loc"][0].tolist())) == 1
    for normalize in (False, True):
        c = ou.segment_inputs(30, False, 2)
        out, bound = ou.segment_wmean_reference(c["h"], c["seg"], c["cols"], c["w"], normalize)
        loops = np.zeros_like(out)
        for i in range(len(c["seg"]) - 1):
            den = 0.0
            for j in range(c["seg"][i], c["seg"][i + 1]):
                if 0 <= c["cols"][j] < ou.SEG_ROWS:
                    den += abs(float(c["w"][j]))
                    loops[i] += float(c["w"][j]) * c["h"][c["cols"][j]].astype(np.float64)
            if normalize:
                loops[i] /= max(den, 1e-12)
        close(out, loops)
        assert (out[0] == 0).all() and (out[-1] == 0).all() and (bound[-1] == 0).all()
        assert {-1, ou.SEG_ROWS} <= set(c["cols"].tolist())
    rng = np.random.default_rng(0)
    g = rng.standard_normal((9, 5)).astype(np.float32)
    idx = np.array([3, 0, 3, 3, 6, 0, 1, 3, 6])
    ref = torch.zeros(8, 7, dtype=torch.float64)
    ref[:, :5].index_add_(0, torch.from_numpy(idx), torch.from_numpy(g).double())
    close(ou.scatter_add_reference(g, idx, 8, 7)[0], ref.numpy())
    assert np.array_equal(ou.gather_reference(g, idx, 3), g[idx, :3])


def test_gemm_reference_is_the_header_formula():
    """every case's op(A) op(B) against plain loops over gemm.h's four index
    formulas, and against parity_util.gemm_operands"""
    for case in ou.gemm_cases():
        ak, bk, gather, M, N, K = case
        if K > 200:
            continue
        c = ou.gemm_inputs(case, True, 11)
        A, B, ai, bi = c["A"], c["B"], c["a_idx"], c["b_idx"]
        want, bound = ou.gemm_reference(A, ak, ai, B, bk, bi, M, N, K)
        loops = np.zeros((M, N))
        for m in range(M):
            for k in range(K):
                a = A[ai[m] if ai is not None else m, k] if ak else A[ai[k] if ai is not None else k, m]
                for n in range(0, N, max(1, N // 3)):
                    b = B[n, k] if bk else B[bi[k] if bi is not None else k, n]
                    loops[m, n] += float(a) * float(b)
        cols = list(range(0, N, max(1, N // 3)))
        assert np.array_equal(want[:, cols], loops[:, cols])
        oa, ob = pu.gemm_operands(dict(M=M, N=N, K=K, a_kmajor=ak, b_kmajor=bk, a=A, b=B, a_idx=ai, b_idx=bi))
        assert np.array_equal(want, oa @ ob) and (bound >= 0).all()
    kinds = {(c[0], c[1], c[2]) for c in ou.gemm_cases()}
    assert len(kinds) == 10                          # 4 layouts x {none, a_idx} + 2 N-major-B layouts x b_idx
    assert any(c[5] == 1032 for c in ou.gemm_cases())
    assert (True, True, None, 1, 6, 8) in ou.gemm_cases() and (False, True, None, 1, 6, 8) not in ou.gemm_cases()


# ----------------------------------------------------------------------------- exact mode stays below 2^24
def test_exact_mode_partial_sums_stay_below_2_pow_24():
    lim = 2.0 ** 24
    for shape in ou.LINEAR_SHAPES:
        for with_rows in (False, True):
            for with_b in (False, True):
                for zeros in (False, True):
                    c = ou.linear_inputs(shape, with_rows, with_b, True, 7, zeros=zeros)
                    for k in ("x", "W", "dy"):
                        assert np.array_equal(c[k], np.round(c[k])) and np.abs(c[k]).max() <= 8
                    assert ou.max_partial_sum(*ou.linear_abs_sums(c)) < lim
    for case in ou.gemm_cases():
        ak, bk, gather, M, N, K = case
        c = ou.gemm_inputs(case, True, 7)
        oa, ob = ou.gemm_operands(c["A"], ak, c["a_idx"], c["B"], bk, c["b_idx"], M, N, K)
        assert ou.max_partial_sum(np.abs(oa) @ np.abs(ob)) < lim
    for shape in ou.AGG_SHAPES:
        c = ou.agg_inputs(shape, True, 7)
        assert np.array_equal(c["w"] * 8, np.round(c["w"] * 8))
        fwd = ou.weighted_agg_reference(np.abs(c["q"]), c["loc"], c["w"])
        bwd, _ = ou.agg_dq_reference(np.abs(c["dagg"]), c["loc"], c["w"], shape[3])
        assert 8 * ou.max_partial_sum(fwd, bwd) < lim       # (in units of the weights' 1 / 8)
    for d in ou.SEG_WIDTHS:
        c = ou.segment_inputs(d, True, 7)
        out, _ = ou.segment_wmean_reference(np.abs(c["h"]), c["seg"], c["cols"], np.abs(c["w"]), False)
        assert 8 * ou.max_partial_sum(out) < lim


# ----------------------------------------------------------------------------- planted defects
def _beyond(want, bound, i, exact):
    """float32(want) with element i moved one ulp beyond its bound"""
    got = np.asarray(want, np.float64).astype(np.float32)
    v = np.float32(want[i] + bound[i])
    while abs(float(v) - want[i]) <= bound[i] or (exact and v == got[i]):
        v = np.nextafter(v, np.float32(np.inf))
    got[i] = v
    return got


def test_check_rejects_single_defects():
    shape = ou.LINEAR_SHAPES[1]
    for exact in (False, True):
        c = ou.linear_inputs(shape, True, True, exact, 9, zeros=exact)
        ref = ou.linear_reference(c["x"], c["rows"], c["W"], c["b"], True, c["dy"], exact)
        for k, (want, bound) in ref.items():
            want, bound = np.asarray(want), np.broadcast_to(bound, np.shape(want))
            ou.check(k, want.astype(np.float32), want, bound, exact)      # a correct result passes
            i = tuple(s // 2 for s in want.shape)
            last = want.ndim - 1
            with pytest.raises(AssertionError, match=f"row {i[0]}, column {i[last] if last else 0}"):
                ou.check(k, _beyond(want, bound, i, exact), want, bound, exact)
            # (the same element exactly on its bound's float32 neighbour inside passes)
        # a dropped bias
        nob = ou.linear_reference(c["x"], c["rows"], c["W"], None, True, c["dy"], exact)
        with pytest.raises(AssertionError, match="buffer y"):
            ou.check("y", nob["y"][0].astype(np.float32), *ref["y"], exact)
        with pytest.raises(AssertionError, match="buffer dW"):
            ou.check("dW", nob["dW"][0].astype(np.float32), *ref["dW"], exact)
    # the slope taken the wrong way at y == 0 (exact inputs with planted zeros): lrelu'(0) = 1
    y, _ = ref["y"]
    assert (y == 0).any()
    r = c["rows"].astype(np.int64)
    dz_bad = c["dy"].astype(np.float64) * np.where(y >= 0, 1.0, SLOPE32)
    with pytest.raises(AssertionError, match="buffer dW"):
        ou.check("dW", (dz_bad.T @ c["x"].astype(np.float64)[r][:, :shape[2]]).astype(np.float32), *ref["dW"], True)
    with pytest.raises(AssertionError, match="buffer db"):
        ou.check("db", dz_bad.sum(0).astype(np.float32), *ref["db"], True)
    # ... and in the normalisation's backward
    cc = ou.concat_inputs(ou.CONCAT_SHAPES[1], True, 9)
    cref = ou.concat_reference(cc["h"], cc["rows"], cc["agg"], cc["W"], cc["b"], cc["dy"])
    yy, nn = cref["y"][0], cref["norms"][0]
    dot = (yy * cc["dy"]).sum(1, keepdims=True)
    dp_bad = np.where(yy >= 0, 1.0, SLOPE32) * (cc["dy"] - yy * dot) / nn[:, None]
    with pytest.raises(AssertionError, match="buffer db"):
        ou.check("db", dp_bad.sum(0).astype(np.float32), *cref["db"])
    # a transposed operand (square, so only the values tell)
    for exact in (False, True):
        case = (True, False, None, 36, 36, 36)
        g = ou.gemm_inputs(case, exact, 13)
        want, bound = ou.gemm_reference(g["A"], True, None, g["B"], False, None, 36, 36, 36, exact)
        ou.check("C", want.astype(np.float32), want, bound, exact)
        bad, _ = ou.gemm_reference(g["A"], True, None, g["B"], True, None, 36, 36, 36, exact)
        with pytest.raises(AssertionError, match="buffer C"):
            ou.check("C", bad.astype(np.float32), want, bound, exact)
    # shape and dtype
    with pytest.raises(AssertionError):
        ou.check("C", want.astype(np.float32)[:-1], want, bound)
    with pytest.raises(AssertionError):
        ou.check("C", want, want, bound)


def test_check_agg_rejects_single_defects():
    for exact in (False, True):
        c = ou.agg_inputs(ou.AGG_SHAPES[1], exact, 4)
        want = ou.weighted_agg_reference(c["q"], c["loc"], c["w"])
        good = want.astype(np.float32)
        ou.check_agg("agg", good, want, exact)
        bad = good.copy()
        if exact:
            bad[5, 7] = np.nextafter(bad[5, 7], np.float32(np.inf))
        else:
            bad[5, 7] += np.float32(2.5 * ou.AGG_ROWREL * np.linalg.norm(want[5]))
        with pytest.raises(AssertionError, match="row 5"):
            ou.check_agg("agg", bad, want, exact)
    # a transposed weight table gives other sums
    c = ou.agg_inputs((48, 7, 7, 9), True, 4)
    want = ou.weighted_agg_reference(c["q"], c["loc"], c["w"])
    with pytest.raises(AssertionError):
        ou.check_agg("agg", ou.weighted_agg_reference(c["q"], c["loc"], c["w"].T).astype(np.float32), want, True)
