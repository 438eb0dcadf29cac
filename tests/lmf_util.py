"""The numpy references of the LMF path (csrc/lmf.hip, baselines.LMF), shared by
tests/test_gpu_lmf.py (on the GPU) and tests/test_lmf_host.py (which checks the
references themselves on the host).  CSR helpers, value kinds and the error
measure are als_util's.

R is a CSR (ptr, idx, val, n_rows, n_cols), c = alpha val, s_ui = x_u . y_i +
bx_u + by_i.  The objective to maximise is

    L = sum_obs c s - sum_obs (1 + c) softplus(s) - sum_unobs softplus(s) - (reg / 2)(|X|^2 + |Y|^2)

and one half-iteration runs, per row u from the old tables,

    D    = sum_all i sig(s_ui) y_i          dsum = sum_all i sig(s_ui)
    w_i  = c_ui sig(-s_ui)  for observed i
    g    = sum_obs w_i y_i - D - reg x_u    gb = sum_obs w_i - dsum
    h   += g^2                              hb += gb^2
    x_u += lr g / sqrt(1e-6 + h)            bx_u += lr gb / sqrt(1e-6 + hb)
"""
import numpy as np

from als_util import transpose

EPS = 1e-6
DEFECTS = ("unmasked_tail", "one_plus_c_for_c", "regularised_bias")
DEFAULTS = dict(factors=128, learning_rate=0.1, regularization=0.6, alpha=1.0, iterations=30, random_state=None)


def sigmoid(s):
    """Stable, in the dtype of s: 1 / (1 + e^-s) for s >= 0, e^s / (1 + e^s) otherwise."""
    s = np.asarray(s)
    e = np.exp(-np.abs(s))
    one = s.dtype.type(1)
    return np.where(s >= 0, one, e) / (one + e)


def softplus(s):
    s = np.asarray(s, np.float64)
    return np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s)))


def dense_terms(X, bx, Y, by, dtype, defect=None):
    """(D [n_rows, f], dsum [n_rows]) in `dtype` arithmetic.  defect "unmasked_tail"
    adds one phantom item with y = 0 and bias 0, as a tile's unmasked tail row
    would: sig(bx_u) * 0 to D and sig(bx_u) (0.5 at zero bias) to dsum."""
    dtype = np.dtype(dtype).type
    X, bx, Y, by = (np.asarray(a, dtype) for a in (X, bx, Y, by))
    P = sigmoid(X @ Y.T + bx[:, None] + by[None, :])
    D, dsum = P @ Y, P.sum(1)
    if defect == "unmasked_tail":
        dsum = dsum + sigmoid(bx)
    assert D.dtype == dtype and dsum.dtype == dtype
    return D, dsum


def dense_terms_loops(X, bx, Y, by):
    """dense_terms in float64 by the definition, cell by cell (tiny shapes)."""
    n, f = np.shape(X)
    D, dsum = np.zeros((n, f)), np.zeros(n)
    for u in range(n):
        for i in range(len(Y)):
            s = float(bx[u]) + float(by[i])
            for k in range(f):
                s += float(X[u][k]) * float(Y[i][k])
            p = 1.0 / (1.0 + np.exp(-s)) if s >= 0 else np.exp(s) / (1.0 + np.exp(s))
            dsum[u] += p
            for k in range(f):
                D[u, k] += p * float(Y[i][k])
    return D, dsum


def half_iteration(ptr, idx, val, X, bx, H, hb, Y, by, reg, alpha, lr, dtype, defect=None, D=None, dsum=None):
    """The recurrence above in `dtype`: the new (X, bx, H, hb).  D, dsum: given
    dense terms (taken as they are) instead of dense_terms(X, bx, Y, by)."""
    dtype = np.dtype(dtype).type
    X, bx, H, hb = (np.array(a, dtype) for a in (X, bx, H, hb))
    Y, by = np.asarray(Y, dtype), np.asarray(by, dtype)
    if D is None:
        D, dsum = dense_terms(X, bx, Y, by, dtype, defect)
    D, dsum = np.asarray(D, dtype), np.asarray(dsum, dtype)
    reg, lr, eps, one = dtype(reg), dtype(lr), dtype(EPS), dtype(1)
    for u in range(len(ptr) - 1):
        sl = slice(int(ptr[u]), int(ptr[u + 1]))
        ids = np.asarray(idx[sl], np.int64)
        Yi = Y[ids]
        c = dtype(alpha) * np.asarray(val[sl], dtype)
        s = Yi @ X[u] + bx[u] + by[ids]
        w = (c + one if defect == "one_plus_c_for_c" else c) * sigmoid(-s)
        g = Yi.T @ w - D[u] - reg * X[u]
        gb = w.sum(dtype=dtype) - dsum[u]
        if defect == "regularised_bias":
            gb = gb - reg * bx[u]
        H[u] = H[u] + g * g
        hb[u] = hb[u] + gb * gb
        X[u] = X[u] + lr * g / np.sqrt(eps + H[u])
        bx[u] = bx[u] + lr * gb / np.sqrt(eps + hb[u])
    assert X.dtype == dtype and bx.dtype == dtype and H.dtype == dtype and hb.dtype == dtype
    return X, bx, H, hb


def fit(csr, X, Y, bx, by, reg, alpha, lr, iterations, dtype, defect=None, trace=False):
    """`iterations` times: users from (Y, by), then items from the new (X, bx);
    accumulators start at zero.  (X, Y, bx, by) in dtype; with trace also the
    list of objective() after every iteration."""
    ptr, idx, val = csr[:3]
    tptr, tidx, tval = transpose(csr)[:3]
    X, Y, bx, by = (np.array(a, dtype) for a in (X, Y, bx, by))
    Hx, Hy, hbx, hby = np.zeros_like(X), np.zeros_like(Y), np.zeros_like(bx), np.zeros_like(by)
    seen = []
    for _ in range(iterations):
        X, bx, Hx, hbx = half_iteration(ptr, idx, val, X, bx, Hx, hbx, Y, by, reg, alpha, lr, dtype, defect)
        Y, by, Hy, hby = half_iteration(tptr, tidx, tval, Y, by, Hy, hby, X, bx, reg, alpha, lr, dtype, defect)
        if trace:
            seen.append(objective(csr, X, Y, bx, by, reg, alpha))
    return (X, Y, bx, by, seen) if trace else (X, Y, bx, by)


def objective(csr, X, Y, bx, by, reg, alpha):
    """L over the dense matrix, float64."""
    ptr, idx, val, n_rows, n_cols = csr
    R = np.zeros((n_rows, n_cols))
    R[np.repeat(np.arange(n_rows), np.diff(ptr)), np.asarray(idx, np.int64)] = val
    X, Y, bx, by = (np.asarray(a, np.float64) for a in (X, Y, bx, by))
    S = X @ Y.T + bx[:, None] + by[None, :]
    C = alpha * R
    return float((C * S).sum() - ((1 + C) * softplus(S)).sum() - 0.5 * reg * ((X * X).sum() + (Y * Y).sum()))


def implied_gradient(x_old, x_new, h_new):
    """From zero accumulators h_new = g^2 and the step has g's sign: the gradient
    a half-iteration used, read back from its outputs."""
    x_old, x_new, h_new = (np.asarray(a, np.float64) for a in (x_old, x_new, h_new))
    return np.sign(x_new - x_old) * np.sqrt(h_new)


def row_form(length, long_row):
    """Which form of sig_update_kernel takes a row of `length` items."""
    return "workgroup" if length > long_row else "wave"
