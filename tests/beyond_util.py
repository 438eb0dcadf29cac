"""numpy references of the beyond-accuracy metrics (baselines.intra_diversity,
inter_diversity, coverage, average_degree, degree_dist) and of the kernels
under them (csrc/listmetrics.hip), shared by tests/test_beyond_metrics.py
(which checks the references themselves on the host, against the real
reference's results in tests/golden/beyond_accuracy.npz) and
tests/test_gpu_beyond.py (on the GPU).

The float64 references follow the reference's definitions (eval.py:255-374):
the full K x K cosine matrix for the intra-list similarity, Python sets for
the inter-list distance.  The identity the kernel uses,
    mean(K x K cosine matrix) = |sum_c f_c / |f_c||^2 / K^2,
is a separate function, compared with the matrix form on the host.  Keyword
arguments plant one defect each (see the functions); the checks name the
metric and K in their message.
"""
import numpy as np

U24 = 2.0 ** -24

# the kernels' constants (csrc/listmetrics.hip), replayed
LM_WAVES = 4           # kLmWaves: queries (rows) per workgroup
LM_ROWS = 8            # kLmRows: feature rows in flight per step
LM_CHUNK = 64          # list slots read per step of the slot loop
LM_PASS_VEC = 512      # columns per column pass, float4 form (64 lanes x 4 x kLmAcc)
LM_PASS_SCALAR = 128   # ... scalar form
OV_BALLOT = 64         # kOvBallot: up to here one wave compares a pair by ballot
OV_MAX_K = 4096        # kOvMaxK


def overlap_form(kc):
    """The kernel launch_list_pair_overlap takes for kc columns, replayed."""
    assert 1 <= kc <= OV_MAX_K, f"kc = {kc} is refused by the launcher"
    return "ballot" if kc <= OV_BALLOT else "sorted"


def intra_form(d, ld, offset_floats=0):
    """The form of row_inv_norm_kernel / list_intra_sim_kernel for a table of d
    columns, row stride ld, starting offset_floats floats after a 16-byte boundary."""
    return "float4" if d % 4 == 0 and ld % 4 == 0 and offset_floats % 4 == 0 else "scalar"


# ----------------------------------------------------------------------------- checks
def check_metric(name, K, got, want, tol=0.0):
    """|got - want| <= tol elementwise (tol = 0: exact; NaN matches NaN only).
    The AssertionError names the metric and K."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if g.shape != w.shape:
        raise AssertionError(f"{name} (K = {K}): shape {g.shape}, reference {w.shape}")
    t = np.broadcast_to(np.asarray(tol, np.float64), g.shape)
    with np.errstate(invalid="ignore"):
        bad = ~((np.abs(g - w) <= t) | (np.isnan(g) & np.isnan(w)))
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{name} (K = {K}): got {g[i]!r}, reference {w[i]!r}, |diff| "
                             f"{abs(g[i] - w[i]):.3e} > {t[i]:.3e} at {i}; {int(bad.sum())} of {bad.size} differ")


def check_degree_dist(K, got, want):
    for what, g, w in zip(("degrees", "counts"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or (g != w).any():
            raise AssertionError(f"degree_dist {what} (K = {K}): got {g.tolist()}, reference {w.tolist()}")


# ----------------------------------------------------------------------------- intra-list similarity
def intra_sims_matrix(knn, feats, K, diagonal=True):
    """float64 [n]: per query the mean of cosine_sim_mat (eval.py:255-264) of the
    feature rows of knn[q, :K], entry by entry.  diagonal=False plants a defect:
    the mean over the off-diagonal entries only."""
    knn, f = np.asarray(knn, np.int64), np.asarray(feats, np.float64)
    out = np.empty(len(knn))
    for q in range(len(knn)):
        r = f[knn[q, :K]]
        lengths = np.sqrt((r * r).sum(1))
        with np.errstate(invalid="ignore", divide="ignore"):
            sim = (r @ r.T) / (lengths[:, None] * lengths[None, :])
        k = len(r)
        out[q] = sim.mean() if diagonal else (sim.sum() - np.trace(sim)) / max(1, k * k - k)
    return out


def unit_rows(feats):
    f = np.asarray(feats, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return f * (1.0 / np.sqrt((f * f).sum(1)))[:, None]   # a zero row: inf * 0 = NaN, as on the device


def list_counts(knn, K, n_rows):
    """float64 [n, n_rows]: how often each id is listed in knn[q, :K]."""
    ids = np.asarray(knn, np.int64)[:, :K]
    m = np.zeros((len(ids), n_rows))
    np.add.at(m, (np.repeat(np.arange(len(ids)), ids.shape[1]), ids.reshape(-1)), 1.0)
    return m


def intra_sims_identity(knn, feats, K):
    """float64 [n]: |sum_c f_c / |f_c||^2 / K^2, with (s [n, d], kc) for the bounds.
    A listed zero row makes its query NaN (and no other)."""
    fh = unit_rows(feats)
    m = list_counts(knn, K, len(fh))
    kc = min(K, np.asarray(knn).shape[1])
    bad = np.isnan(fh).any(1)
    s = m @ np.where(bad[:, None], 0.0, fh)
    s[(m[:, bad] > 0).any(1)] = np.nan
    return (s * s).sum(1) / float(kc * kc), s, kc


def intra_diversity_ref(knn, feats, K, **defect):
    return 1.0 - float(intra_sims_matrix(knn, feats, K, **defect).mean())


def reference_fp32_bound(knn, feats, K):
    """How far the reference's fp32 intra_diversity may lie from the float64 one,
    from its operations, u = 2^-24.  An entry of cosine_sim_mat is a dot of
    length d (error <= (d + 4) u sum_k |a_k b_k| <= (d + 4) u |a| |b|, any
    order, as parity_util.gemm_bound), two norms (d squares summed and a root:
    relative error <= (d / 2 + 2) u each), their product and the quotient (u
    each): |entry error| <= (d + 4) u + |sim| (d + 6) u <= (2 d + 10) u.  The mean
    of the K^2 entries (|entry| <= 1) in any order adds at most K^2 u mean|sim|,
    storing it u, and the mean over the n queries n u mean|value|."""
    knn, f = np.asarray(knn, np.int64), np.asarray(feats, np.float64)
    n, d = len(knn), f.shape[1]
    kc = min(K, knn.shape[1])
    fh = unit_rows(f)
    mean_abs = np.empty(n)
    for q in range(n):
        r = fh[knn[q, :K]]
        mean_abs[q] = np.abs(r @ r.T).mean()
    per_query = (2 * d + 10) * U24 + (kc * kc + 1) * U24 * mean_abs
    return float(per_query.mean() + (n + 1) * U24 * mean_abs.mean())


def device_intra_bound(s, kc, knn, feats, K):
    """Componentwise bound of list_intra_sim's fp32 value against float64, in the
    style of parity_util.gemm_bound.  inv[r] carries d / 2 + 3 roundings (the sum
    of d squares is off by at most d u relative in any order, the root halves
    that; the root, the quotient and the second-order term add one each), each
    product one, the column sum kc: a column's sum is off by at most
    e = (d / 2 + kc + 5) u A with A = sum_c |f_c| / |f_c| in that column (+ 1 for
    the second-order term).  Through the square:
    2 |s| e + e^2 and one rounding; through the sum over d columns (any order):
    (d + 2) u sum (|s| + e)^2; the division adds u."""
    f = np.asarray(feats, np.float64)
    d = f.shape[1]
    a = list_counts(knn, K, len(f)) @ np.abs(unit_rows(f))
    e = (d / 2 + kc + 5) * U24 * a
    t_err = (2 * np.abs(s) * e + e * e).sum(1) + (d + 3) * U24 * ((np.abs(s) + e) ** 2).sum(1)
    val = (s * s).sum(1) / float(kc * kc)
    return t_err / float(kc * kc) + U24 * np.abs(val)


def exact_table(n, d, seed, zero_row=None):
    """float32 [n, d]: each row holds 1, 4 or 16 non-zeros (as many as d allows)
    of one magnitude 2^e, e in [-8, 8], with random signs.  Every squared norm is
    a power of four, every f / |f| entry is +-1, +-1/2 or +-1/4: the kernel's sums
    and squares are exact in fp32 for lists of up to 1000 slots (the largest
    intermediate, kc^2 in sixteenths, is below 2^24)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, d), np.float32)
    choices = [c for c in (1, 4, 16) if c <= d]
    for r in range(n):
        cnt = choices[rng.integers(0, len(choices))]
        cols = rng.choice(d, cnt, replace=False)
        t[r, cols] = rng.choice([-1.0, 1.0], cnt) * 2.0 ** int(rng.integers(-8, 9))
    if zero_row is not None:
        t[zero_row] = 0.0
    return t


def exact_intra_values(knn, table, K):
    """float32 [n]: what the device must give on an exact_table, bit for bit:
    the float64 identity (exact there) divided once in fp32, which is also the
    float64 quotient rounded to fp32."""
    val, s, kc = intra_sims_identity(knn, table, K)
    num = (s * s).sum(1)
    with np.errstate(invalid="ignore"):
        assert (np.isnan(num) | (num == num.astype(np.float32))).all()
        got = num.astype(np.float32) / np.float32(kc * kc)
    both = np.isnan(val) | (val.astype(np.float32) == got)
    assert both.all(), "float32(float64 value) and the fp32 quotient differ"
    return got


# ----------------------------------------------------------------------------- inter-list distance
def pair_overlaps(knn, K, pairs, multiset=False):
    """int64 [n_pairs, 3]: |set(A)|, |set(B)|, |set(A) & set(B)| by Python sets,
    A = knn[a, :K].  multiset=True plants a defect: every slot counts."""
    knn = np.asarray(knn, np.int64)
    out = np.empty((len(pairs), 3), np.int64)
    for i, (a, b) in enumerate(np.asarray(pairs, np.int64).tolist()):
        la, lb = knn[a, :K].tolist(), knn[b, :K].tolist()
        if multiset:
            out[i] = (len(la), len(lb), sum(1 for x in la if x in set(lb)))
        else:
            sa, sb = set(la), set(lb)
            out[i] = (len(sa), len(sb), len(sa & sb))
    return out


def inter_from_overlaps(o):
    o = np.asarray(o, np.float64)
    return float(np.mean(1.0 - o[:, 2] / np.sqrt(o[:, 0] * o[:, 1])))


def inter_diversity_ref(knn, K, pairs, **defect):
    return inter_from_overlaps(pair_overlaps(knn, K, pairs, **defect))


# ----------------------------------------------------------------------------- coverage and degrees
def coverage_ref(knn, test_positives, K, all_nodes=True, skip_first=True):
    """eval.py:342-355.  skip_first=False plants a defect: columns 0 .. K - 1."""
    knn = np.asarray(knn, np.int64)
    recs = knn[:, 1:K + 1] if skip_first else knn[:, :K]
    if not all_nodes:
        recs = np.asarray(test_positives, np.int64)
    return len(set(recs.reshape(-1).tolist())) / knn.shape[0]


def degrees_ref(knn, in_degrees, K, shifted=False):
    """(average degree, (sorted distinct degrees, counts)) over knn[:, :K]
    (eval.py:357-374).  shifted=True plants a defect: columns 1 .. K."""
    knn = np.asarray(knn, np.int64)
    recs = (knn[:, 1:K + 1] if shifted else knn[:, :K]).reshape(-1)
    deg = np.asarray(in_degrees, np.int64)[recs]
    vals, counts = np.unique(deg, return_counts=True)
    return int(deg.sum()) / len(deg), (vals.astype(np.int64), counts.astype(np.int64))
