"""Float64 references of torch.ops.pinsage (csrc/torch_ops.cpp and the autograd
formulas of pinsage_ops.py) for tests/test_gpu_torch_ops_forms.py;
tests/test_ops_host.py checks them on the CPU: every closed-form gradient
against torch autograd of the same float64 expression, every exact-mode input
set against the 2^24 limit, and every comparison against planted defects.

Nothing here comes from the device.  Each reference returns (want, bound):
want in float64, bound the element's float32 error budget derived from
parity_util's gemm_bound / gemm_terms / _prod_bound (split-bf16 products, the
library's default arithmetic, which contains the fp32-MFMA bound), carried
through LeakyReLU and the row norm as gemm_form_reference carries it and through
the normalisation's backward by norm_lrelu_bwd_reference.  Two terms are added
where a stage consumes an earlier stage's rounded result:

  sign.  An element whose pre-activation z lies within its own bound E of 0
  (and E > 0) may take either LeakyReLU branch on the device: forward, the
  result then lies within 2 |z| + E of the reference's; backward, the factor
  lrelu' differs by 1 - 0.01, so |cotangent| (1 - 0.01) is added.  With
  exact-sum inputs E = 0 and nothing is uncertain: z == 0 takes the slope.
  propagation.  A product whose left operand carries the bound E_l adds
  E_l @ |right| (first order, as parity_util states its bounds).

Exact mode: integer inputs of magnitude <= 8 (weights dyadic, k / 8) make every
sum of products exact in float32 below 2^24, so the result must equal float64's
bit for bit (bound 0).  A stage behind LeakyReLU's 0.01f or the row norm is not
a sum of products any more: its bound stays the derived one.
"""
import numpy as np

import parity_util as pu
from parity_util import SLOPE32, U24

PREC = 1     # bound of the split-bf16 products (>= the fp32-MFMA bound for the same sum)
RATIOS = {}


def note(op, ratio):
    """the largest error / bound per op (pytest -s prints it when it grows)"""
    if ratio > RATIOS.get(op, -1.0):
        RATIOS[op] = ratio
        print(f"RATIO {op}: {ratio:.3f}")


def f64(a):
    return np.asarray(a, np.float64)


def _idx(idx, n):
    return np.arange(n) if idx is None else np.asarray(idx, np.int64).reshape(-1)


def dyadic(rng, shape, lim=8):
    """weights k / 8, k in [-lim, lim]: exact in float32 and in a bf16 hi plane"""
    return (rng.integers(-lim, lim + 1, shape) / 8.0).astype(np.float32)


def values(rng, shape, exact, wide=True):
    return pu.form_values(rng, shape, exact, wide=wide)


def max_partial_sum(*abs_products):
    """the largest sum of absolute terms of an exact-mode case (it bounds every
    partial sum in any order): must stay below 2^24"""
    return max(float(np.max(p)) if np.size(p) else 0.0 for p in abs_products)


# ----------------------------------------------------------------------------- comparison
def check(name, got, want, bound, exact=False):
    """got (a float32 array the op returned) against (want, bound) element by
    element through parity_util.check_written: bound 0 in exact mode means
    float32(want) bit for bit, bound 0 otherwise means equal.  Raises naming
    the row and column; returns the largest error / bound."""
    got = np.asarray(got)
    want, bound = f64(want), np.broadcast_to(f64(bound), np.shape(want))
    assert got.dtype == np.float32, (name, got.dtype)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.ndim == 1:
        got, want, bound = got[:, None], want[:, None], bound[:, None]
    if got.size == 0:
        return 0.0
    ref = dict(want=want, bound=bound, written=np.ones(want.shape, bool))
    return pu.check_written(name, got, got, ref, exact)


def scatter_rows(vals, bnd, idx, n_rows, width, exact=False):
    """out [n_rows, width] = 0; out[idx[i], :c] += vals[i].  Bound: the addends'
    own, plus gemm_bound(cnt, sum |addend|) where a row receives cnt > 1 addends
    (cnt - 1 additions in any order; one addend onto zero is exact)."""
    vals, bnd = f64(vals), np.broadcast_to(f64(bnd), np.shape(vals))
    idx = np.asarray(idx, np.int64)
    c = vals.shape[1]
    out, E, S = (np.zeros((n_rows, width)) for _ in range(3))
    np.add.at(out[:, :c], idx, vals)
    np.add.at(E[:, :c], idx, bnd)
    np.add.at(S[:, :c], idx, np.abs(vals))
    cnt = np.bincount(idx, minlength=n_rows)[:, None]
    if not exact:
        E = E + np.where(cnt > 1, pu.gemm_bound(cnt, S), 0.0)
    return out, E


# ----------------------------------------------------------------------------- gemm
def gemm_operands(A, a_kmajor, a_idx, B, b_kmajor, b_idx, M, N, K):
    """op(A) [M][K], op(B) [K][N] as gemm.h's header comment states them:
      A K-major: A(m,k) = a[row(m)][k], row(m) = a_idx ? a_idx[m] : m
      A M-major: A(m,k) = a[row(k)][m], row(k) = a_idx ? a_idx[k] : k
      B K-major: B(k,n) = b[n][k]                  (no gather is defined)
      B N-major: B(k,n) = b[row(k)][n], row(k) = b_idx ? b_idx[k] : k"""
    a, b = f64(A), f64(B)
    opA = a[_idx(a_idx, M)][:, :K] if a_kmajor else a[_idx(a_idx, K)][:, :M].T
    if b_kmajor:
        assert b_idx is None, "gemm.h defines b_idx for an N-major B only"
        opB = b[:N, :K].T
    else:
        opB = b[_idx(b_idx, K)][:, :N]
    assert opA.shape == (M, K) and opB.shape == (K, N), (opA.shape, opB.shape)
    return opA, opB


def _product(L, R, exact, extra_terms=0, extra_abs=0.0):
    """(L @ R, bound) for a sum of K products plus extra_terms further addends
    whose absolute values are extra_abs"""
    K = L.shape[1]
    absprod = np.abs(L) @ np.abs(R)
    return L @ R, pu._prod_bound(K + extra_terms, K, absprod, absprod + extra_abs, PREC, exact)


def gemm_reference(A, a_kmajor, a_idx, B, b_kmajor, b_idx, M, N, K, exact=False):
    opA, opB = gemm_operands(A, a_kmajor, a_idx, B, b_kmajor, b_idx, M, N, K)
    return _product(opA, opB, exact)


# ----------------------------------------------------------------------------- linear
def _lrelu_fwd(z, E):
    """(lrelu(z), its bound, the sign-uncertain elements) from z's bound E"""
    neg = ~(z > 0)
    y = np.where(neg, SLOPE32 * z, z)
    Ey = np.where(neg, SLOPE32 * E + (E > 0) * U24 * np.abs(y), E)
    unc = (np.abs(z) <= E) & (E > 0)
    return y, np.where(unc, 2 * np.abs(z) + E + U24 * np.abs(y), Ey), unc


def linear_reference(x, rows, W, b, lrelu, dy=None, exact=False):
    """y = act(x[rows, :K] W^T + b) and, with a cotangent dy, dx [x's shape], dW,
    db as _linear_backward computes them: dz = dy lrelu'(y) (one float32
    product where the slope applies), dW = dz^T x[rows], db = sum dz, dx =
    index_add of dz W.  {name: (want, bound)}.  exact: y's bound is 0 (an
    exact sum times 0.01f rounds once: float32 of the float64 product), the
    gradients' only where no slope enters (lrelu off)."""
    x, W = f64(x), f64(W)
    N, K = W.shape
    r = _idx(rows, x.shape[0])
    n = len(r)
    A = x[r][:, :K]
    bias = np.zeros(N) if b is None else f64(b)
    z, E = _product(A, W.T, exact, extra_terms=int(b is not None), extra_abs=np.abs(bias))
    z = z + bias
    if lrelu:
        y, Ey, unc = _lrelu_fwd(z, E)
    else:
        y, Ey, unc = z, E, np.zeros(z.shape, bool)
    out = dict(y=(y, Ey))
    if dy is None:
        return out
    dy = f64(dy)
    g = pu.lrelu_grad64(y) if lrelu else np.ones(z.shape)
    g = np.where(g == 1.0, 1.0, SLOPE32)
    dz = dy * g
    E_dz = (g != 1.0) * U24 * np.abs(dz) + unc * (1.0 - SLOPE32) * np.abs(dy)
    tight = exact and not lrelu
    dW, E_dW = _product(dz.T, A, tight)
    out["dW"] = (dW, E_dW + E_dz.T @ np.abs(A))
    if b is not None:
        out["db"] = (dz.sum(0), (0.0 if tight else pu.gemm_bound(n, np.abs(dz).sum(0))) + E_dz.sum(0))
    dr, E_dr = _product(dz, W, tight)
    out["dx"] = scatter_rows(dr, E_dr + E_dz @ np.abs(W), r, x.shape[0], x.shape[1], tight)
    return out


# ----------------------------------------------------------------------------- concat_linear_lrelu_l2norm
def concat_forward64(h, rows, agg, W, b):
    """the op's value in float64: (y, norms, z, A)"""
    h, agg, W, b = f64(h), f64(agg), f64(W), f64(b)
    n, hid = agg.shape
    d = W.shape[1] - hid
    A = np.concatenate([h[_idx(rows, n)][:, :d], agg], 1)
    z = A @ W.T + b
    v = np.where(z > 0, z, SLOPE32 * z)
    nrm = np.sqrt((v * v).sum(1))
    return v / nrm[:, None], nrm, z, A


def concat_reference(h, rows, agg, W, b, dy=None):
    """(y, norms) = normalize(lrelu([h[rows, :d] || agg] W^T + b)) with the bounds
    of gemm_form_reference's L2-norm epilogue (the same derivation holds for
    the out > 128 path, a stored product then l2norm_rows), and with dy the
    gradients of _cat_backward: dp = norm_lrelu_bwd(dy) from parity_util.
    norm_lrelu_bwd_reference, whose bound is widened by the device's own y and
    norms (dp is linear in dy: d dp = lrelu' (E_y |y.dy| + |y| sum E_y |dy|) /
    r + |dp| E_r / r, first order) and by the sign term; dW = dp^T [h[rows] ||
    agg], db = sum dp, dagg = dp W[:, d:], dh = scatter_add_rows of dp W[:, :d]
    (position-order sums).  {name: (want, bound)}."""
    y, nrm, z, A = concat_forward64(h, rows, agg, W, b)
    W, b = f64(W), f64(b)
    n, hid = np.shape(agg)
    out_f, Kc = W.shape
    d = Kc - hid
    absprod = np.abs(A) @ np.abs(W.T)
    E = pu._prod_bound(Kc + 1, Kc, absprod, absprod + np.abs(b), PREC, False)
    v, E_v, unc = _lrelu_fwd(z, E)
    r = nrm[:, None]
    E_r = (np.abs(v) * E_v).sum(1, keepdims=True) / r + ((out_f + 4) / 2 + 1) * U24 * r
    E_y = E_v / r + np.abs(v) * E_r / r ** 2 + U24 * np.abs(y)
    out = dict(y=(y, E_y), norms=(nrm, E_r[:, 0]))
    if dy is None:
        return out
    dy = f64(dy)
    dp, E_dp = pu.norm_lrelu_bwd_reference(y, nrm, dy)
    sy = np.where(y > 0, 1.0, SLOPE32)
    dot = (y * dy).sum(1, keepdims=True)
    E_dp = (E_dp + sy * (E_y * np.abs(dot) + np.abs(y) * (E_y * np.abs(dy)).sum(1, keepdims=True)) / r +
            np.abs(dp) * E_r / r + unc * (1.0 - SLOPE32) * np.abs(dy - y * dot) / r)
    dW, E_dW = _product(dp.T, A, False)
    out["dW"] = (dW, E_dW + E_dp.T @ np.abs(A))
    out["db"] = (dp.sum(0), pu.gemm_bound(n, np.abs(dp).sum(0)) + E_dp.sum(0))
    dA, E_dA = _product(dp, W, False)
    E_dA = E_dA + E_dp @ np.abs(W)
    out["dagg"] = (dA[:, d:], E_dA[:, d:])
    hs = np.shape(h)
    out["dh"] = scatter_rows(dA[:, :d], E_dA[:, :d], _idx(rows, n), hs[0], hs[1])
    return out


# ----------------------------------------------------------------------------- weighted_agg, segment_wmean, rows
AGG_ROWREL = 1e-6   # tests/test_gpu_aggw.py's bound on this slot-order fma chain, row-relative


def weighted_agg_reference(q, loc, w):
    """agg[f] = sum_t w[f][t] q[loc[f][t]]"""
    return (f64(w)[:, :, None] * f64(q)[np.asarray(loc, np.int64)]).sum(1)


def check_agg(name, got, want, exact):
    """exact: bit for bit; else the row-relative 1e-6 of test_gpu_aggw.py.
    Returns error / bound."""
    got, want = np.asarray(got), f64(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    if got.size == 0:
        return 0.0
    if exact:
        return check(name, got, want, 0.0, True)
    err = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    bound = AGG_ROWREL * np.maximum(np.linalg.norm(want, axis=1), 1e-30)
    return pu._first_bad(name, err[:, None], bound[:, None], lambda i: f"row {i[0]}")


def agg_dq_reference(dagg, loc, w, n_q, exact=False):
    """dq[u] = sum over the slots (f, t) with loc[f][t] == u of w[f][t] dagg[f]: an
    fma chain over the slots in (f, t) order -- gemm_bound over cnt terms"""
    dagg, w = f64(dagg), f64(w)
    loc = np.asarray(loc, np.int64)
    n, T = loc.shape
    terms = (w[:, :, None] * dagg[:, None, :]).reshape(n * T, -1)
    flat = loc.reshape(-1)
    dq = np.zeros((n_q, dagg.shape[1]))
    S = np.zeros_like(dq)
    np.add.at(dq, flat, terms)
    np.add.at(S, flat, np.abs(terms))
    cnt = np.bincount(flat, minlength=n_q)[:, None]
    return dq, (np.zeros_like(S) if exact else pu.gemm_bound(cnt, S))


def segment_wmean_reference(h, seg, cols, w, normalize, exact=False):
    """out[i] = sum_{j in [seg[i], seg[i+1])} w[j] h[cols[j]] (/ max(sum |w[j]|,
    1e-12) if normalize); a column outside [0, h rows) is skipped in both sums.
    Bound: an fma chain of cnt terms, gemm_bound(cnt, .); normalised, each
    weight is first multiplied by 1 / den -- den a float32 sum of cnt terms
    ((cnt + 4) u relative), its reciprocal and the product one rounding each:
    (cnt + 6) u more per term."""
    h, w = f64(h), f64(w)
    seg = np.asarray(seg, np.int64)
    cols = np.asarray(cols, np.int64)
    n_seg, d = len(seg) - 1, h.shape[1]
    out, E = np.zeros((n_seg, d)), np.zeros((n_seg, d))
    for i in range(n_seg):
        j = np.arange(seg[i], seg[i + 1])
        j = j[(cols[j] >= 0) & (cols[j] < h.shape[0])]
        if not len(j):
            continue
        den = max(np.abs(w[j]).sum(), 1e-12) if normalize else 1.0
        terms = (w[j] / den)[:, None] * h[cols[j]]
        out[i] = terms.sum(0)
        S = np.abs(terms).sum(0)
        if normalize:
            E[i] = pu.gemm_bound(len(j), S) + (len(j) + 6) * U24 * S
        elif not exact:
            E[i] = pu.gemm_bound(len(j), S)
    return out, E


def gather_reference(h, idx, width):
    h = np.asarray(h)
    return h[np.asarray(idx, np.int64)][:, :h.shape[1] if width < 0 else width]


def scatter_add_reference(grad, idx, n_rows, width, exact=False):
    grad = f64(grad)
    return scatter_rows(grad, 0.0, idx, n_rows, grad.shape[1] if width < 0 else width, exact)


# ----------------------------------------------------------------------------- the cases (shared by the GPU and host tests)
LINEAR_SHAPES = ((5, 4, 4, 4, 5), (37, 72, 64, 48, 33), (300, 128, 128, 512, 260), (40, 64, 64, 6, 33),
                 (90, 36, 32, 50, 67), (20, 16, 16, 130, 1))          # (x rows, ld, K, N, n)
CONCAT_SHAPES = ((4, 4, 4, 1), (24, 32, 16, 33), (128, 512, 128, 130), (64, 64, 6, 9), (32, 96, 200, 35))  # d, hid, out, n
GEMM_SHAPES = ((4, 4, 4), (36, 128, 132), (130, 72, 40), (1, 6, 8))                                       # M, N, K
AGG_SHAPES = ((4, 1, 1, 1), (48, 7, 33, 9), (260, 17, 5, 40), (512, 10, 67, 30), (516, 11, 5, 8), (1024, 65, 9, 70),
              (128, 130, 6, 20))                                                                          # hid, T, n, n_q
SEG_LENGTHS = (0, 1, 3, 4, 5, 8, 9, 65, 130, 1)   # (the last: its only column is out of range)
SEG_WIDTHS = (4, 30, 260, 1028)
SEG_ROWS = 50


def linear_inputs(shape, with_rows, with_b, exact, seed, zeros=False):
    """dict(x [x rows, ld], rows int32 [n] with repeats | None, W [N, K], b [N] | None,
    dy [M, N]).  zeros: integer inputs whose pre-activation is exactly 0 -- the
    x row of output row 0 is zero and b[:2] = 0."""
    xr, ld, K, N, n = shape
    rng = np.random.default_rng(seed)
    x = values(rng, (xr, ld), exact)
    W = values(rng, (N, K), exact, wide=False)
    b = values(rng, (N,), exact, wide=False) if with_b else None
    rows = None
    if with_rows:
        rows = rng.integers(0, xr, n).astype(np.int32)
        rows[-1] = rows[0]
        if n > 2:
            rows[n // 2] = rows[0]
    M = n if with_rows else xr
    if zeros:
        x[rows[0] if with_rows else 0] = 0
        if b is not None:
            b[:2] = 0
    return dict(x=x, rows=rows, W=W, b=b, dy=values(rng, (M, N), exact, wide=False))


def linear_abs_sums(c):
    """the sums of absolute terms of every product of an exact-mode linear case"""
    x, W, dy = (np.abs(f64(c[k])) for k in ("x", "W", "dy"))
    K = W.shape[1]
    r = _idx(c["rows"], x.shape[0])
    A = x[r][:, :K]
    dr = dy @ W
    return (A @ W.T + (0 if c["b"] is None else np.abs(f64(c["b"]))), dy.T @ A, dy.sum(0),
            scatter_rows(dr, 0.0, r, x.shape[0], x.shape[1], True)[0])


def concat_inputs(shape, with_rows, seed):
    """dict(h [n + 7, d + 8], rows int64 [n] with repeats | None, agg, W, b, dy);
    W's row 1 and b[1] are zero: column 1 of y holds exact zeros in every row"""
    d, hid, out, n = shape
    rng = np.random.default_rng(seed)
    h = values(rng, (n + 7, d + 8), False, wide=False)
    agg = values(rng, (n, hid), False, wide=False)
    W = values(rng, (out, d + hid), False, wide=False)
    b = values(rng, (out,), False, wide=False)
    W[1], b[1] = 0, 0
    rows = None
    if with_rows:
        rows = rng.integers(0, n + 7, n).astype(np.int64)
        rows[-1] = rows[0]
    return dict(h=h, rows=rows, agg=agg, W=W, b=b, dy=values(rng, (n, out), False))


def gemm_allowed(a_kmajor, b_kmajor, M, N, K):
    """launch_gemm's documented limits: K in fours, an M-major A's M and an
    N-major B's N in fours"""
    return K % 4 == 0 and (a_kmajor or M % 4 == 0) and (b_kmajor or N % 4 == 0)


def gemm_cases():
    """(a_kmajor, b_kmajor, gather in {None, 'a', 'b'}, M, N, K): the four layouts x
    the gathers gemm.h defines x GEMM_SHAPES where allowed, and a gathered
    N-major B whose K = 1032 crosses the 1024-row index window"""
    out = []
    for ak in (True, False):
        for bk in (True, False):
            for gather in (None, "a") + (() if bk else ("b",)):
                out += [(ak, bk, gather, M, N, K) for M, N, K in GEMM_SHAPES if gemm_allowed(ak, bk, M, N, K)]
        out.append((ak, False, "b", 36, 8, 1032))
    return out


def gemm_inputs(case, exact, seed):
    """dict(A, B (each with 4 spare columns behind its live width: the live part
    is a view with stride(0) > width), a_idx, b_idx): gathered operands have 9
    spare rows and an index with repeats"""
    ak, bk, gather, M, N, K = case
    rng = np.random.default_rng(seed)
    a_rows, a_cols = (M, K) if ak else (K, M)
    b_rows, b_cols = (N, K) if bk else (K, N)
    a_idx = b_idx = None
    if gather == "a":
        a_idx = rng.integers(0, a_rows + 9, a_rows).astype(np.int32)
        a_idx[-1] = a_idx[0]
    if gather == "b":
        b_idx = rng.integers(0, b_rows + 9, b_rows).astype(np.int32)
        b_idx[-1] = b_idx[0]
    A = values(rng, (a_rows + (9 if a_idx is not None else 0), a_cols + 4), exact)
    B = values(rng, (b_rows + (9 if b_idx is not None else 0), b_cols + 4), exact, wide=False)
    return dict(A=A, B=B, a_idx=a_idx, b_idx=b_idx)


def agg_inputs(shape, exact, seed):
    """dict(q [n_q, hid], loc int32 [n, T], w [n, T], dagg [n, hid], unnamed): row 0's
    slots all name one q row; q row `unnamed` (None when n_q == 1) is named by
    no slot"""
    hid, T, n, n_q = shape
    rng = np.random.default_rng(seed)
    unnamed = None if n_q == 1 else int(rng.integers(0, n_q))
    pool = np.array([u for u in range(n_q) if u != unnamed])
    loc = pool[rng.integers(0, len(pool), (n, T))].astype(np.int32)
    loc[0] = loc[0, 0]
    if exact:
        w = (rng.integers(1, 9, (n, T)) / 8.0).astype(np.float32)
    else:
        w = rng.random((n, T)) + 0.01
        w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    return dict(q=values(rng, (n_q, hid), exact), loc=loc, w=w, dagg=values(rng, (n, hid), exact, wide=False),
                unnamed=unnamed)


def segment_inputs(d, exact, seed):
    """dict(h [SEG_ROWS, d], seg int64, cols int32, w): SEG_LENGTHS in one call;
    columns -1 and SEG_ROWS planted in the segments of length 5, 9, 65 and 130
    (inside and behind the four-at-a-time part) and as the last segment's only
    column; weights of both signs"""
    rng = np.random.default_rng(seed)
    seg = np.concatenate([[0], np.cumsum(SEG_LENGTHS)]).astype(np.int64)
    cols = rng.integers(0, SEG_ROWS, seg[-1]).astype(np.int32)
    for i, at, bad in ((4, 4, -1), (6, 1, SEG_ROWS), (6, 8, -1), (7, 64, SEG_ROWS), (7, 2, -1), (8, 129, -1),
                       (8, 5, SEG_ROWS), (9, 0, -1)):
        assert at < SEG_LENGTHS[i]
        cols[seg[i] + at] = bad
    w = dyadic(rng, seg[-1]) if exact else (rng.standard_normal(seg[-1]).astype(np.float32))
    return dict(h=values(rng, (SEG_ROWS, d), exact), seg=seg, cols=cols, w=w)
