"""The numpy / Python-int references of the BPR path (csrc/bpr.hip,
baselines.BPR), shared by tests/test_gpu_bpr.py (on the GPU) and
tests/test_bpr_host.py (which checks the references themselves on the host).
CSR helpers and the error measure are als_util's, sigmoid and softplus
lmf_util's, the generator oracle's.

R is a CSR (ptr, idx, val, n_users, n_items) with strictly ascending rows; only
its structure is used.  Cell e is the e-th stored cell, sample t = e * S + s.
Draw round rho, sample t of a cell (u, i), tries k = 0 .. 15:
    (r0, r1, r2, r3) = philox(seed, (rho * 16 + k, t lo, t hi, offset))
    j = (r0 * n_items) >> 32;  accept the first j that is not a column of row u
neg[t] = j, or -1 (void, w[t] = 0) after 16 rejected tries;
    z_t = (x_u . y_i + b_i) - (x_u . y_j + b_j),  w[t] = sig(-z_t).
Iteration `it`: the user half on round 2 it, the item half on round 2 it + 1 and
the new X, both Jacobi.  User row u: for each of its t ascending (+w_t, y_i)
then (-w_t, y_j), a void sample (+-0, y_i).  Item row i: the samples whose
positive is i, t ascending, (+w_t, x_u); then the non-void samples whose
negative is i, t ascending, (-w_t, x_u).  Per row
    a = sum val_e row_e;  sv = sum val_e;  g = a - reg x;  h += g^2;  x += lr g / sqrt(1e-6 + h)
    item half only:  gb = sv;  hb += gb^2;  b += lr gb / sqrt(1e-6 + hb)
which, for a fixed draw, is ascent on
    sum_t ln sig(z_t) - (reg / 2)(|X|^2 + |Y|^2)   over the non-void t.
"""
import numpy as np

from lmf_util import EPS, sigmoid, softplus
from oracle import oracle as orc

TRIES = 16
MAX_NEGATIVES = 8
GRADIENT_DEFECTS = ("negative_sign_dropped", "regularised_bias")
DRAW_DEFECTS = ("positives_not_rejected", "halves_share_a_round")
DEFECTS = GRADIENT_DEFECTS + DRAW_DEFECTS
DEFAULTS = dict(factors=128, learning_rate=0.05, regularization=0.01, iterations=100, negatives=1, random_state=None)


# ----------------------------------------------------------------------------- the draw
def draw(csr, S, seed, rho, offset=0, cell_base=0, defect=None):
    """neg int32 [nnz * S] by the definition above, in Python integers.  The
    call's cell e is cell cell_base + e of the whole matrix."""
    ptr, idx, _, n_users, n_items = csr
    neg = np.full(len(idx) * S, -1, np.int32)
    for u in range(n_users):
        b, e = int(ptr[u]), int(ptr[u + 1])
        row = set(int(i) for i in idx[b:e])
        for q in range((e - b) * S):
            t = (cell_base + b) * S + q
            for k in range(TRIES):
                r = orc.philox(seed, (rho * 16 + k, t & 0xFFFFFFFF, t >> 32, offset))
                j = (int(r[0]) * n_items) >> 32
                if j not in row or defect == "positives_not_rejected":
                    neg[b * S + q] = j
                    break
    return neg


def rounds(it, defect=None):
    """(draw round of the user half, of the item half) of iteration `it`."""
    return (2 * it, 2 * it) if defect == "halves_share_a_round" else (2 * it, 2 * it + 1)


def samples(csr, S):
    """(user, positive item) of every sample t, int64 [nnz * S] each."""
    ptr, idx = csr[:2]
    users = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    return np.repeat(users, S), np.repeat(np.asarray(idx, np.int64), S)


def scores(csr, neg, S, X, Y, b, dtype):
    """z_t in `dtype` (0 for a void sample)."""
    dtype = np.dtype(dtype).type
    X, Y, b = (np.asarray(a, dtype) for a in (X, Y, b))
    u, i = samples(csr, S)
    j = np.where(neg >= 0, neg, 0).astype(np.int64)
    z = ((X[u] * Y[i]).sum(1, dtype=dtype) + b[i]) - ((X[u] * Y[j]).sum(1, dtype=dtype) + b[j])
    assert z.dtype == dtype
    return np.where(neg >= 0, z, dtype(0))


def weights(csr, neg, S, X, Y, b, dtype):
    """w_t = sig(-z_t) in `dtype`, 0 for a void sample."""
    dtype = np.dtype(dtype).type
    w = np.where(neg >= 0, sigmoid(-scores(csr, neg, S, X, Y, b, dtype)), dtype(0))
    assert w.dtype == dtype
    return w


# ----------------------------------------------------------------------------- entry arrays
def user_entries(csr, neg, w, S, defect=None):
    """The user half's CSR (ptr, idx int32 items, val): 2 S entries per cell."""
    ptr = csr[0]
    _, i = samples(csr, S)
    j = np.where(neg >= 0, neg, i)
    sign = 1 if defect == "negative_sign_dropped" else -1
    idx = np.stack([i, j], 1).reshape(-1).astype(np.int32)
    val = np.stack([w, sign * w], 1).reshape(-1)
    return np.asarray(ptr, np.int64) * (2 * S), idx, val


def item_entries(csr, neg, w, S, defect=None):
    """The item half's CSR (ptr, idx int32 users, val): per item the samples whose
    positive it is, then the non-void samples whose negative it is."""
    n_items = csr[4]
    u, i = samples(csr, S)
    ok = neg >= 0
    sign = 1 if defect == "negative_sign_dropped" else -1
    key = np.concatenate([i, neg[ok].astype(np.int64)])
    order = np.argsort(key, kind="stable")
    ptr = np.zeros(n_items + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=n_items), out=ptr[1:])
    return ptr, np.concatenate([u, u[ok]])[order].astype(np.int32), np.concatenate([w, sign * w[ok]])[order]


def user_entries_loops(csr, neg, w, S):
    """user_entries by the definition: per row a list of (value, item)."""
    ptr, idx = csr[:2]
    rows = []
    for u in range(len(ptr) - 1):
        ent = []
        for e in range(int(ptr[u]), int(ptr[u + 1])):
            for s in range(S):
                t = e * S + s
                ent.append((w[t], int(idx[e])))
                ent.append((-w[t], int(neg[t]) if neg[t] >= 0 else int(idx[e])))
        rows.append(ent)
    return rows


def item_entries_loops(csr, neg, w, S):
    """item_entries by the definition: per item a list of (value, user)."""
    ptr, idx, _, n_users, n_items = csr
    rows = [[] for _ in range(n_items)]
    for sign, column in ((1, None), (-1, neg)):
        for u in range(n_users):
            for e in range(int(ptr[u]), int(ptr[u + 1])):
                for s in range(S):
                    t = e * S + s
                    item = int(idx[e]) if column is None else int(column[t])
                    if item >= 0:
                        rows[item].append((sign * w[t], u))
    return rows


# ----------------------------------------------------------------------------- the half-iterations
def apply(ptr, idx, val, X, H, Y, reg, lr, dtype, bx=None, hb=None, reg_bias=False):
    """The signed gathered row sum and the AdaGrad step in `dtype`: the new
    (X, H), or (X, H, bx, hb) with a bias pair."""
    dtype = np.dtype(dtype).type
    X, H, Y = np.array(X, dtype), np.array(H, dtype), np.asarray(Y, dtype)
    reg, lr, eps = dtype(reg), dtype(lr), dtype(EPS)
    if bx is not None:
        bx, hb = np.array(bx, dtype), np.array(hb, dtype)
    for r in range(len(ptr) - 1):
        sl = slice(int(ptr[r]), int(ptr[r + 1]))
        v = np.asarray(val[sl], dtype)
        g = Y[np.asarray(idx[sl], np.int64)].T @ v - reg * X[r]
        H[r] = H[r] + g * g
        X[r] = X[r] + lr * g / np.sqrt(eps + H[r])
        if bx is not None:
            gb = np.cumsum(v, dtype=dtype)[-1] if len(v) else dtype(0)   # in order, as defined: sum() adds pairwise
            if reg_bias:
                gb = gb - reg * bx[r]
            hb[r] = hb[r] + gb * gb
            bx[r] = bx[r] + lr * gb / np.sqrt(eps + hb[r])
    assert X.dtype == dtype and H.dtype == dtype
    return (X, H) if bx is None else (X, H, bx, hb)


def half_iteration(csr, neg, S, half, X, Y, b, H, hb, reg, lr, dtype, defect=None):
    """One half on the draw `neg` from the tables given: "user" returns the new
    (X, Hx), "item" the new (Y, Hy, b, hb)."""
    w = weights(csr, neg, S, X, Y, b, dtype)
    if half == "user":
        return apply(*user_entries(csr, neg, w, S, defect), X, H, Y, reg, lr, dtype)
    return apply(*item_entries(csr, neg, w, S, defect), Y, H, X, reg, lr, dtype, b, hb,
                 reg_bias=defect == "regularised_bias")


def fit(csr, X, Y, b, S, seed, reg, lr, iterations, dtype, defect=None, draws=None):
    """`iterations` iterations from zero accumulators: (X, Y, b) in dtype.
    draws: a dict rho -> neg to read the draws from (and to fill)."""
    X, Y, b = (np.array(a, dtype) for a in (X, Y, b))
    Hx, Hy, hb = np.zeros_like(X), np.zeros_like(Y), np.zeros_like(b)
    draws = {} if draws is None else draws

    def neg_of(rho):
        if rho not in draws:
            draws[rho] = draw(csr, S, seed, rho, defect=defect)
        return draws[rho]

    for it in range(iterations):
        ru, ri = rounds(it, defect)
        X, Hx = half_iteration(csr, neg_of(ru), S, "user", X, Y, b, Hx, None, reg, lr, dtype, defect)
        Y, Hy, b, hb = half_iteration(csr, neg_of(ri), S, "item", X, Y, b, Hy, hb, reg, lr, dtype, defect)
    return X, Y, b


def objective(csr, X, Y, b, neg, S, reg):
    """sum over the non-void t of ln sig(z_t), minus the penalty; float64."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    z = scores(csr, neg, S, X, Y, b, np.float64)[neg >= 0]
    return float(-softplus(-z).sum() - 0.5 * reg * ((X * X).sum() + (Y * Y).sum()))


# ----------------------------------------------------------------------------- the planted matrix
def planted_matrix(seed, n_tracks=160, n_groups=4, n_cols=60, size=8, stray=0.1):
    """The collection x track matrix behind n2v_util.planted_graph(seed), by the
    same recipe and the same draws: (csr, group of each track)."""
    rng = np.random.default_rng(seed)
    M = np.zeros((n_cols, n_tracks), np.int64)
    for c in range(n_cols):
        grp = c % n_groups
        own = np.flatnonzero(np.arange(n_tracks) % n_groups == grp)
        while M[c].sum() < size:
            t = rng.integers(n_tracks) if rng.random() < stray else own[rng.integers(len(own))]
            M[c, t] = 1
    ptr = np.zeros(n_cols + 1, np.int64)
    np.cumsum(M.sum(1), out=ptr[1:])
    idx = np.nonzero(M)[1].astype(np.int32)
    return (ptr, idx, np.ones(len(idx), np.float32), n_cols, n_tracks), np.arange(n_tracks) % n_groups
