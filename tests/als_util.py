"""The numpy references of the ALS path (csrc/als.hip, baselines.ALS), shared by
tests/test_gpu_als.py (on the GPU) and tests/test_als_host.py (which checks the
references themselves on the host).

A sparse matrix is (ptr int64 [n_rows + 1], idx int32, val float32, n_rows,
n_cols).  With c = alpha val, G = Y^T Y + reg I, one half-iteration runs per row

    x = X[u];  r = -G x + sum_i (c - (c - 1)(y_i . x)) y_i;  p = r;  rs = r . r
    if rs < 1e-20: X[u] stays
    repeat steps times:
        Ap = G p + sum_i (c - 1)(y_i . p) y_i
        a = rs / (p . Ap);  x += a p;  r -= a Ap;  rn = r . r
        if rn < 1e-20: break
        p = r + (rn / rs) p;  rs = rn
    X[u] = x

The error of a row is |x - x64| / max(|x64|, |x_in|): a row without items is
driven towards 0, so its own norm is no scale.  A device result is held to
TOL_FACTOR times the error the float32 restatement shows against float64 by the
same measure on the same inputs (another summation order, contracted FMAs).
"""
import numpy as np

TOL_FACTOR = 8.0
TINY = 1e-20
DEFECTS = ("c_for_c_minus_1", "reg_off_G", "items_first")


def gram(Y, reg, dtype):
    Y = np.asarray(Y, dtype)
    return (Y.T @ Y + dtype(reg) * np.eye(Y.shape[1], dtype=dtype)).astype(dtype)


def half_iteration(ptr, idx, val, X, Y, reg, alpha, steps, dtype, defect=None):
    """The recurrence above in `dtype` arithmetic (np.float64 or np.float32):
    the new X.  `defect` plants one of DEFECTS[:2] (for the host tests)."""
    dtype = np.dtype(dtype).type
    X = np.array(X, dtype)
    Y = np.asarray(Y, dtype)
    G = gram(Y, 0.0 if defect == "reg_off_G" else reg, dtype)
    one, tiny = dtype(1), dtype(TINY)
    for u in range(len(ptr) - 1):
        sl = slice(int(ptr[u]), int(ptr[u + 1]))
        Yi = Y[np.asarray(idx[sl], np.int64)]
        c = dtype(alpha) * np.asarray(val[sl], dtype)
        cm = c if defect == "c_for_c_minus_1" else c - one
        x = X[u].copy()
        r = Yi.T @ (c - cm * (Yi @ x)) - G @ x
        p = r.copy()
        rs = r @ r
        if rs < tiny:
            continue
        for _ in range(steps):
            Ap = G @ p + Yi.T @ (cm * (Yi @ p))
            a = rs / (p @ Ap)
            x = x + a * p
            r = r - a * Ap
            rn = r @ r
            if rn < tiny:
                break
            p = r + (rn / rs) * p
            rs = rn
        assert x.dtype == dtype
        X[u] = x
    return X


def exact_rows(ptr, idx, val, Y, reg, alpha):
    """float64 [n_rows, f]: the solution of (G + sum_i (c - 1) y_i y_i^T) x = sum_i c y_i per row."""
    Y = np.asarray(Y, np.float64)
    G = gram(Y, reg, np.float64)
    out = np.zeros((len(ptr) - 1, Y.shape[1]))
    for u in range(len(ptr) - 1):
        sl = slice(int(ptr[u]), int(ptr[u + 1]))
        Yi = Y[np.asarray(idx[sl], np.int64)]
        c = alpha * np.asarray(val[sl], np.float64)
        out[u] = np.linalg.solve(G + (Yi.T * (c - 1)) @ Yi, Yi.T @ c)
    return out


def transpose(csr):
    ptr, idx, val, n_rows, n_cols = csr
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ptr))
    order = np.argsort(np.asarray(idx, np.int64), kind="stable")
    tptr = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(idx, minlength=n_cols), out=tptr[1:])
    return tptr, rows[order].astype(np.int32), np.asarray(val)[order], n_cols, n_rows


def fit(csr, X, Y, reg, alpha, steps, iterations, dtype, defect=None):
    """`iterations` times: users from Y, then items from the new X.  (X, Y) in dtype."""
    ptr, idx, val = csr[:3]
    tptr, tidx, tval = transpose(csr)[:3]
    X, Y = np.array(X, dtype), np.array(Y, dtype)
    for _ in range(iterations):
        if defect == "items_first":
            Y = half_iteration(tptr, tidx, tval, Y, X, reg, alpha, steps, dtype)
            X = half_iteration(ptr, idx, val, X, Y, reg, alpha, steps, dtype)
        else:
            X = half_iteration(ptr, idx, val, X, Y, reg, alpha, steps, dtype)
            Y = half_iteration(tptr, tidx, tval, Y, X, reg, alpha, steps, dtype)
    return X, Y


def dense(csr):
    ptr, idx, val, n_rows, n_cols = csr
    R = np.zeros((n_rows, n_cols))
    R[np.repeat(np.arange(n_rows), np.diff(ptr)), np.asarray(idx, np.int64)] = val
    return R


def loss(csr, X, Y, reg, alpha):
    """The objective over the dense matrix, float64."""
    R = dense(csr)
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    S = X @ Y.T
    obs = R > 0
    return float((alpha * R[obs] * (1 - S[obs]) ** 2).sum() + (S[~obs] ** 2).sum()
                 + reg * ((X * X).sum() + (Y * Y).sum()))


def row_errors(x, x64, x_in):
    """|x - x64| / max(|x64|, |x_in|) per row (0 where all three are zero rows)."""
    x, x64, x_in = (np.asarray(a, np.float64) for a in (x, x64, x_in))
    num = np.linalg.norm(x - x64, axis=1)
    den = np.maximum(np.linalg.norm(x64, axis=1), np.linalg.norm(x_in, axis=1))
    return np.where(num == 0, 0.0, num / np.where(den == 0, 1.0, den))


def table_error(a, a64):
    """The largest elementwise difference relative to the largest entry of a64."""
    a64 = np.asarray(a64, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - a64).max() / np.abs(a64).max())


def csr_from_rows(rows, n_cols):
    """rows: per row a (ids, values) pair."""
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r[0]) for r in rows], out=ptr[1:])
    idx = np.concatenate([np.asarray(r[0], np.int32) for r in rows]) if len(rows) else np.zeros(0, np.int32)
    val = np.concatenate([np.asarray(r[1], np.float32) for r in rows]) if len(rows) else np.zeros(0, np.float32)
    return ptr, idx.astype(np.int32), val.astype(np.float32), len(rows), n_cols


VALUE_KINDS = ("ones", "counts", "fractions")


def values(rng, n, kind):
    if kind == "ones":
        return np.ones(n, np.float32)
    if kind == "counts":
        return rng.integers(1, 6, n).astype(np.float32)
    return rng.uniform(0.05, 0.95, n).astype(np.float32)


def random_csr(rng, lengths, n_cols, kind):
    """A CSR whose row u has lengths[u] distinct ascending ids out of n_cols."""
    rows = []
    for ln in lengths:
        ids = np.sort(rng.choice(n_cols, ln, replace=False))
        rows.append((ids, values(rng, ln, kind)))
    return csr_from_rows(rows, n_cols)


def init_factors(rng, n, f):
    """The documented initial scale, (U[0, 1) - 0.5) / f, as float32."""
    return ((rng.random((n, f)) - 0.5) / f).astype(np.float32)


def row_form(length, long_row):
    """Which form of als_half_kernel solves a row of `length` items."""
    return "workgroup" if length > long_row else "wave"
