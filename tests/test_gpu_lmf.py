"""The kernels of csrc/lmf.hip (pinsage_lmf_dense, pinsage_lmf_update) and what
stands on them: baselines.LMF, ColTrackLMF and TrackTrackLMF, and with save_knn
/ LazyKnnDict the two tables end to end.  The references are tests/lmf_util.py,
checked on the host in tests/test_lmf_host.py.

Dense kernel.  The bound is derived, with u = 2^-24 and parity_util.gemm_bound:
    ds <= gemm_bound(f, |x|.|y| + |bx| + |by|)         the score
    dp <= ds / 4 + 8 u p                                sig' <= 1/4; exp, add, divide
    |dD[u, c]| <= gemm_bound(n_other, sum_i p |y_ic|) + sum_i dp_i |y_ic|
and dsum likewise with |y_ic| = 1.  Every test prints its worst ratio to it.  A
workgroup owns 128 rows (pinsage_lmf_row_block), a wave 32 of them, and an item
tile is 32 items: the row counts straddle 32 and 128, the item counts 32.

Update kernel.  New x, bx are held against the float64 restatement by
als_util.row_errors under the project's rule: the device's error is at most
als_util.TOL_FACTOR (8) times the float32 restatement's on the same inputs;
both are printed.  D and dsum are fed from float64 rounded to fp32 (one case
from the device), and the accumulators are seeded in [0.5, 2]: from zero an
entry with a tiny gradient is divided by about 1e-3 and the ratio measures
nothing.  From zero accumulators the gradient itself (sqrt(h_new)) is held by
the same rule and the step is recomputed from the device's own h_new.

Tables are passed with NaN in their padding columns and a sentinel tail; the
padding has to be NaN and the tail untouched afterwards.
"""
import numpy as np
import pytest
import torch

import als_util as au
import lmf_util as lu
import parity_util as pu
from conftest import golden
from rowfit_util import PAD, SENT, _padded, _unpad

pytestmark = pytest.mark.gpu

ERR_ARG = -2       # pinsage_status (include/pinsage_hip.h)
U = 2.0 ** -24
REG, LR = 0.6, 0.1


# ----------------------------------------------------------------------------- launch helpers
def _vec(a, tail=False):
    a = np.asarray(a, np.float32)
    if tail:
        a = np.concatenate([a, np.full(PAD, SENT, np.float32)])
    return torch.from_numpy(a).cuda()


def _unvec(t, n):
    h = t.cpu().numpy()
    assert (h[n:] == SENT).all(), "values behind the vector were written"
    return h[:n].copy()


def _dense(X, bx, Y, by, pad_x=0, pad_y=0, pad_d=0):
    """pinsage_lmf_dense into sentinel-filled outputs: (status, D [n, f], dsum [n])."""
    import _native as nat
    n, f = X.shape
    m = Y.shape[0]
    xd, yd = _padded(X, f + pad_x), _padded(Y, f + pad_y)
    dd = _padded(np.full((n, f), SENT, np.float32), f + pad_d, tail=True)
    sd = _vec(np.full(n, SENT), tail=True)
    bxd, byd = _vec(bx), _vec(by)
    rc = nat.lib().pinsage_lmf_dense(nat.ptr(xd), nat.ptr(bxd), n, f + pad_x, nat.ptr(yd), nat.ptr(byd), m,
                                     f + pad_y, f, nat.ptr(dd), f + pad_d, nat.ptr(sd), nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, _unpad(dd, n, f, f + pad_d), _unvec(sd, n)


def _dense_bound(X, bx, Y, by):
    """(D64, dsum64, bound on D, bound on dsum) as derived in the module docstring."""
    X, bx, Y, by = (np.asarray(a, np.float64) for a in (X, bx, Y, by))
    f, m = X.shape[1], Y.shape[0]
    P = lu.sigmoid(X @ Y.T + bx[:, None] + by[None, :])
    ds = pu.gemm_bound(f, np.abs(X) @ np.abs(Y).T + np.abs(bx)[:, None] + np.abs(by)[None, :])
    dp = ds / 4 + 8 * U * P
    return (P @ Y, P.sum(1), pu.gemm_bound(m, P @ np.abs(Y)) + dp @ np.abs(Y),
            pu.gemm_bound(m, P.sum(1)) + dp.sum(1))


def _check_dense(X, bx, Y, by, what, **kw):
    rc, D, dsum = _dense(X, bx, Y, by, **kw)
    assert rc == 0
    D64, d64, bD, bd = _dense_bound(X, bx, Y, by)
    assert np.isfinite(D).all() and np.isfinite(dsum).all()
    rD, rd = float((np.abs(D - D64) / bD).max()), float((np.abs(dsum - d64) / bd).max())
    print(f"{what}: worst ratio to the bound, D {rD:.3f}, dsum {rd:.3f}")
    assert rD <= 1 and rd <= 1, (what, rD, rd)
    return D, dsum


def _dense_case(n, m, f, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, scale, (n, f)).astype(np.float32), rng.normal(0, scale, n).astype(np.float32),
            rng.normal(0, scale, (m, f)).astype(np.float32), rng.normal(0, scale, m).astype(np.float32))


# ----------------------------------------------------------------------------- the dense kernel
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("f", [4, 8, 60, 64, 100, 128])
def test_dense_factors_and_leading_dimensions(f, pad):
    X, bx, Y, by = _dense_case(37, 300, f, seed=f + pad, scale=0.5)
    _check_dense(X, bx, Y, by, f"f = {f}, every ld = f + {pad}", pad_x=pad, pad_y=pad, pad_d=pad)
    if pad:
        _check_dense(X, bx, Y, by, f"f = {f}, ldx = f + {pad} only", pad_x=pad)


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 127, 128, 129, 257])
def test_dense_row_counts(n_rows):
    """Around the 32 rows of a wave and the 128 rows of a workgroup, and three workgroups."""
    X, bx, Y, by = _dense_case(n_rows, 64, 16, seed=200 + n_rows, scale=0.5)
    _check_dense(X, bx, Y, by, f"{n_rows} rows")


@pytest.mark.parametrize("f", [8, 128])
@pytest.mark.parametrize("n_other", [1, 2, 31, 32, 33, 63, 65, 1000])
def test_dense_item_counts(n_other, f):
    """A tile's tail rows must add zero, and sig(0) = 0.5 is not zero: dsum would
    be off by 0.5 per missing row of the last tile, far outside the bound."""
    X, bx, Y, by = _dense_case(33, n_other, f, seed=300 + n_other + f, scale=0.5)
    _check_dense(X, bx, Y, by, f"{n_other} items, f = {f}")


@pytest.mark.parametrize("f", [16, 128])
def test_dense_trained_scale_and_saturated_scores(f):
    """x . y spans +-40 and each bias +-20: scores to +-80, where sig rounds to
    0 or 1 at one end and is ~1e-35 at the other."""
    rng = np.random.default_rng(400 + f)
    X, Y = rng.normal(0, 1, (37, f)), rng.normal(0, 1, (300, f))
    X *= 40.0 / np.abs(X @ Y.T).max()
    bx, by = rng.uniform(-20, 20, 37), rng.uniform(-20, 20, 300)
    S = X @ Y.T
    (ua, ia), (ub, ib) = np.unravel_index(S.argmax(), S.shape), np.unravel_index(S.argmin(), S.shape)
    bx[ua], by[ia], bx[ub], by[ib] = 20, 20, -20, -20         # the two extreme cells get the extreme biases
    X, bx, Y, by = (a.astype(np.float32) for a in (X, bx, Y, by))
    S = X.astype(np.float64) @ Y.T + bx[:, None] + by[None, :]
    assert S.max() > 75 and S.min() < -75
    _check_dense(X, bx, Y, by, f"scores in [{S.min():.0f}, {S.max():.0f}], f = {f}")


@pytest.mark.parametrize("f,n_rows,n_other", [(128, 130, 300), (60, 37, 70), (4, 33, 33)])
def test_dense_layout_is_exact_on_integer_data(f, n_rows, n_other):
    """X[u] = 200 e_c(u), Y in {-1, +1}, no bias: sig is exactly 0 or 1 in fp32,
    so D[u] = sum of the y_i with y_i[c(u)] = +1 and dsum their number, integers
    that have to come out exactly.  Both products' operand maps are in it, the
    second one's register-to-item order included."""
    rng = np.random.default_rng(f)
    c = (7 * np.arange(n_rows) + 3) % f
    X = np.zeros((n_rows, f), np.float32)
    X[np.arange(n_rows), c] = 200.0
    Y = rng.choice([-1.0, 1.0], (n_other, f)).astype(np.float32)
    rc, D, dsum = _dense(X, np.zeros(n_rows), Y, np.zeros(n_other), pad_y=4)
    assert rc == 0
    on = (Y[:, c] > 0).T.astype(np.float64)                  # [n_rows, n_other]
    assert np.array_equal(D, (on @ Y).astype(np.float32)) and np.array_equal(dsum, on.sum(1).astype(np.float32))


def test_dense_bits_repeat_and_do_not_depend_on_the_batch():
    X, bx, Y, by = _dense_case(161, 333, 128, seed=500, scale=0.3)
    a, b = _dense(X, bx, Y, by), _dense(X, bx, Y, by)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    for u in (0, 37, 128, 160):                             # another lane, wave, workgroup, grid
        _, D, dsum = _dense(X[u:u + 1], bx[u:u + 1], Y, by)
        assert np.array_equal(D.view(np.uint32), a[1][u:u + 1].view(np.uint32)), u
        assert np.array_equal(dsum.view(np.uint32), a[2][u:u + 1].view(np.uint32)), u


def test_dense_refusals_leave_the_outputs_untouched():
    import _native as nat
    L = nat.lib()
    n, m, f = 5, 9, 8
    rng = np.random.default_rng(600)
    X = torch.from_numpy(au.init_factors(rng, n + 2, 16)).cuda().reshape(-1)
    Y = torch.from_numpy(au.init_factors(rng, m + 2, 16)).cuda().reshape(-1)
    bx, by = torch.zeros(n, device="cuda"), torch.zeros(m, device="cuda")

    def dense(f=f, ldx=f, ldy=f, ldd=f, x_off=0, y_off=0, d_off=0, m=m, n=n):
        D = torch.full((n * 16 + PAD,), SENT, dtype=torch.float32, device="cuda")
        s = torch.full((n + PAD,), SENT, dtype=torch.float32, device="cuda")
        rc = L.pinsage_lmf_dense(nat.ptr(X[x_off:]), nat.ptr(bx), n, ldx, nat.ptr(Y[y_off:]), nat.ptr(by), m, ldy, f,
                                 nat.ptr(D[d_off:]), ldd, nat.ptr(s), nat.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((D == SENT).all() and (s == SENT).all())

    assert dense() == (0, False)                            # the accepted call writes
    assert dense(n=0) == (0, True)                          # no rows: accepted, nothing launched
    for kw in ({"f": 6}, {"f": 132, "ldx": 132, "ldy": 132, "ldd": 132}, {"f": 0}, {"ldx": 4}, {"ldy": 4},
               {"ldd": 4}, {"ldx": 10}, {"ldy": 10}, {"ldd": 10}, {"x_off": 1}, {"y_off": 1}, {"d_off": 1},
               {"m": 0}):
        assert dense(**kw) == (ERR_ARG, True), kw
        assert L.pinsage_last_error()


# ----------------------------------------------------------------------------- the update kernel
def _update(csr, X, bx, H, hb, Y, by, D, dsum, alpha=1.0, reg=REG, lr=LR, pad=0, forms=None):
    """pinsage_lmf_update: (status, X, bx, H, hb, error word)."""
    import _native as nat
    L = nat.lib()
    ptr, idx, val, n, m = csr
    f = X.shape[1]
    if forms is not None:
        long_row = int(L.pinsage_lmf_long_row())
        got = {lu.row_form(int(ln), long_row) for ln in np.diff(ptr)}
        assert got == set(forms), (got, forms)
    xd, hd = _padded(X, f + pad, tail=True), _padded(H, f + pad, tail=True)
    yd, dd = _padded(Y, f + pad), _padded(D, f + pad)
    bxd, hbd, byd, dsd = _vec(bx, tail=True), _vec(hb, tail=True), _vec(by), _vec(dsum)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ptr, idx, val)]
    rc = L.pinsage_lmf_update(nat.ptr(t[0]), nat.ptr(t[1]), nat.ptr(t[2]), n, nat.ptr(yd), nat.ptr(byd), m,
                              f + pad, nat.ptr(xd), nat.ptr(bxd), f + pad, f, nat.ptr(dd), f + pad,
                              nat.ptr(dsd), nat.ptr(hd), f + pad, nat.ptr(hbd), alpha, reg, lr, nat.ptr(err),
                              nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, _unpad(xd, n, f, f + pad), _unvec(bxd, n), _unpad(hd, n, f, f + pad), _unvec(hbd, n), int(err)


MIXED = [0, 1, 2, 63, 64, 65, 257]


def _update_case(f, seed, kind="counts", lengths=MIXED, n_other=300, seeded=True):
    """Tables at the documented initial scale plus a trained-size bias, dense
    terms from float64 rounded to fp32, accumulators uniform in [0.5, 2] or zero."""
    rng = np.random.default_rng(seed)
    csr = au.random_csr(rng, lengths, n_other, kind)
    n = len(lengths)
    X, Y = au.init_factors(rng, n, f) * 8, au.init_factors(rng, n_other, f) * 8
    bx, by = rng.normal(0, 0.5, n).astype(np.float32), rng.normal(0, 0.5, n_other).astype(np.float32)
    D, dsum = (a.astype(np.float32) for a in lu.dense_terms(X, bx, Y, by, np.float64))
    if seeded:
        H, hb = rng.uniform(0.5, 2, (n, f)).astype(np.float32), rng.uniform(0.5, 2, n).astype(np.float32)
    else:
        H, hb = np.zeros((n, f), np.float32), np.zeros(n, np.float32)
    return csr, X, bx, H, hb, Y, by, D, dsum


def _check_update(case, what, alpha=1.0, device_dense=False, **kw):
    """The device against float64 under the 8x rule; returns the device's tables."""
    csr, X, bx, H, hb, Y, by, D, dsum = case
    if device_dense:
        rc, Dd, dsd = _dense(X, bx, Y, by)
        assert rc == 0
        got = _update(csr, X, bx, H, hb, Y, by, Dd, dsd, alpha=alpha, **kw)
        D = dsum = None                                      # the restatements form their own
    else:
        got = _update(csr, X, bx, H, hb, Y, by, D, dsum, alpha=alpha, **kw)
    assert got[0] == 0 and got[5] == 0
    r64 = lu.half_iteration(*csr[:3], X, bx, H, hb, Y, by, REG, alpha, LR, np.float64, D=D, dsum=dsum)
    r32 = lu.half_iteration(*csr[:3], X, bx, H, hb, Y, by, REG, alpha, LR, np.float32, D=D, dsum=dsum)
    for name, i, x_in in (("x", 0, X), ("bx", 1, bx[:, None])):
        w64, w32, dev = (np.asarray(a).reshape(len(x_in), -1) for a in (r64[i], r32[i], got[1 + i]))
        e32, edev = au.row_errors(w32, w64, x_in).max(), au.row_errors(dev, w64, x_in).max()
        print(f"{what}, {name}: float32 restatement {e32:.3e}, device {edev:.3e}, ratio {edev / e32:.2f}")
        assert e32 > 0 and edev <= au.TOL_FACTOR * e32, (what, name, edev, e32)
    return got


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("f", [4, 64, 128])
def test_update_factors_and_leading_dimensions(f, pad):
    _check_update(_update_case(f, seed=f + pad), f"f = {f}, every ld = f + {pad}", pad=pad, forms=["wave"])


@pytest.mark.parametrize("f", [4, 128])
def test_update_long_rows(f):
    """Rows on both sides of the switch to the workgroup form, a hub of 5000
    items over 6000 others, two long rows in one block of 8 rows and one in the next."""
    import _native as nat
    long_row = int(nat.lib().pinsage_lmf_long_row())
    lengths = [5000, 3, long_row, long_row + 1, 0, 64, long_row + 64, 1, 2, long_row + 129, 7]
    _check_update(_update_case(f, seed=7 + f, lengths=lengths, n_other=6000), f"long rows, f = {f}",
                  forms=["wave", "workgroup"], pad=4)


@pytest.mark.parametrize("alpha", [0.5, 1.0, 40.0])
@pytest.mark.parametrize("kind", au.VALUE_KINDS)
def test_update_values_and_alpha(kind, alpha):
    case = _update_case(16, seed=int(alpha * 10) + len(kind), kind=kind, lengths=MIXED + [600], n_other=700)
    _check_update(case, f"{kind}, alpha = {alpha}", alpha=alpha, forms=["wave", "workgroup"])


def test_update_from_the_device_dense_terms():
    case = _update_case(64, seed=21, lengths=MIXED + [600], n_other=700)
    _check_update(case, "dense terms from pinsage_lmf_dense", device_dense=True)


@pytest.mark.parametrize("f", [4, 64, 128])
def test_update_from_zero_accumulators(f):
    """The gradient (sqrt(h_new)) under the 8x rule; the step recomputed from the
    device's own h_new within 4 fp32 ulps of max(|x_old|, lr) (one sqrt, one
    divide, one multiply, one add); float64's sign wherever |g64| exceeds 1e-3 of
    the row's largest."""
    case = _update_case(f, seed=30 + f, lengths=MIXED + [600], n_other=700, seeded=False)
    csr, X, bx, H, hb, Y, by, D, dsum = case
    rc, xn, bxn, hn, hbn, err = _update(*case)
    assert rc == 0 and err == 0
    r64 = lu.half_iteration(*csr[:3], X, bx, H, hb, Y, by, REG, 1.0, LR, np.float64, D=D, dsum=dsum)
    r32 = lu.half_iteration(*csr[:3], X, bx, H, hb, Y, by, REG, 1.0, LR, np.float32, D=D, dsum=dsum)
    n = len(X)
    for name, old, new, h, i in (("x", X, xn, hn, 0), ("bx", bx[:, None], bxn[:, None], hbn[:, None], 1)):
        g64 = lu.implied_gradient(old, np.reshape(r64[i], old.shape), np.reshape(r64[2 + i], old.shape))
        a32 = np.sqrt(np.reshape(r32[2 + i], old.shape).astype(np.float64))
        zero = np.zeros_like(g64)
        e32 = au.row_errors(a32, np.abs(g64), zero).max()
        edev = au.row_errors(np.sqrt(h.astype(np.float64)), np.abs(g64), zero).max()
        print(f"f = {f}, |g| of {name}: float32 restatement {e32:.3e}, device {edev:.3e}, ratio {edev / e32:.2f}")
        assert e32 > 0 and edev <= au.TOL_FACTOR * e32
        h64 = h.astype(np.float64)
        step = LR * np.sqrt(h64) / np.sqrt(lu.EPS + h64)
        off = np.minimum(np.abs(new - (old + step)), np.abs(new - (old - step)))
        tol = 4 * np.spacing(np.maximum(np.abs(old), np.float32(LR)).astype(np.float32)).astype(np.float64)
        print(f"f = {f}, step of {name}: worst {float((off / tol).max() * 4):.2f} ulps")
        assert (off <= tol).all()
        big = np.abs(g64) > 1e-3 * np.abs(g64).max(axis=1, keepdims=True)
        assert big.sum() >= n and np.array_equal(np.sign(new.astype(np.float64) - old)[big], np.sign(g64)[big])


def test_zero_learning_rate_leaves_the_tables_bit_for_bit():
    case = _update_case(8, seed=40, lengths=MIXED + [600], n_other=700)
    csr, X, bx, H, hb = case[:5]
    rc, xn, bxn, hn, hbn, err = _update(*case, lr=0.0, pad=4)
    assert rc == 0 and err == 0
    assert np.array_equal(xn.view(np.uint32), X.view(np.uint32))
    assert np.array_equal(bxn.view(np.uint32), bx.view(np.uint32))
    moved = _update(*case, pad=4)
    assert np.array_equal(hn.view(np.uint32), moved[3].view(np.uint32)) and (hn >= H).all() and (hn > H).any()
    assert np.array_equal(hbn.view(np.uint32), moved[4].view(np.uint32))
    assert (hbn >= hb).all() and (hbn > hb).any()
    assert not np.array_equal(moved[1], X) and not np.array_equal(moved[2], bx)


def test_update_bits_repeat_and_do_not_depend_on_the_batch():
    case = _update_case(128, seed=60, lengths=MIXED + [5000, 600], n_other=6000)
    csr, X, bx, H, hb, Y, by, D, dsum = case
    a, b = _update(*case), _update(*case)
    for i in range(1, 5):
        assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32))
    ptr, idx, val = csr[:3]
    for u in (3, 7, 8):                                      # another grid, block of rows, wave; the hub
        one = au.csr_from_rows([(idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]])], 6000)
        s = slice(u, u + 1)
        alone = _update(one, X[s], bx[s], H[s], hb[s], Y, by, D[s], dsum[s])
        for i in range(1, 5):
            assert np.array_equal(alone[i].view(np.uint32), a[i][s].view(np.uint32)), (u, i)


def test_id_out_of_range_sets_the_error_word():
    import baselines as bl
    case = _update_case(8, seed=70)
    csr = case[0]
    for bad in (300, -1, 2 ** 31 - 1):
        idx = csr[1].copy()
        idx[5] = bad
        got = _update((csr[0], idx) + csr[2:], *case[1:])
        assert got[0] == 0 and got[5] == 1 and all(np.isfinite(a).all() for a in got[1:5])
        t = tuple(torch.from_numpy(a).cuda() for a in (csr[0], idx, csr[2])) + csr[3:]
        with pytest.raises(IndexError):
            bl.LMF(factors=8, iterations=1).fit(t)


def test_update_refusals_leave_the_outputs_untouched():
    import _native as nat
    L = nat.lib()
    n, m, f = 5, 9, 8
    rng = np.random.default_rng(80)
    csr = au.random_csr(rng, [2, 0, 3, 1, 4], m, "counts")
    ptr, idx, val = (torch.from_numpy(a).cuda() for a in csr[:3])
    Y = torch.from_numpy(au.init_factors(rng, m + 2, 16)).cuda().reshape(-1)
    D = torch.from_numpy(au.init_factors(rng, n + 2, 16)).cuda().reshape(-1)
    by, dsum = torch.zeros(m, device="cuda"), torch.ones(n, device="cuda")

    def update(f=f, ldx=f, ldy=f, ldd=f, ldh=f, x_off=0, y_off=0, d_off=0, h_off=0, m=m, alpha=1.0, reg=REG, lr=LR):
        outs = [torch.full((k + PAD,), SENT, dtype=torch.float32, device="cuda") for k in (n * 16, n, n * 16, n)]
        X, bx, H, hb = outs
        rc = L.pinsage_lmf_update(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n, nat.ptr(Y[y_off:]), nat.ptr(by), m,
                                  ldy, nat.ptr(X[x_off:]), nat.ptr(bx), ldx, f, nat.ptr(D[d_off:]), ldd,
                                  nat.ptr(dsum), nat.ptr(H[h_off:]), ldh, nat.ptr(hb), alpha, reg, lr, None,
                                  nat.stream_ptr())
        torch.cuda.synchronize()
        return rc, all(bool((o == SENT).all()) for o in outs)

    assert update() == (0, False)                           # the accepted call writes
    for kw in ({"f": 6}, {"f": 132, "ldx": 132, "ldy": 132, "ldd": 132, "ldh": 132}, {"f": 0}, {"ldx": 4},
               {"ldy": 4}, {"ldd": 4}, {"ldh": 4}, {"ldx": 10}, {"ldy": 10}, {"ldd": 10}, {"ldh": 10}, {"x_off": 1},
               {"y_off": 1}, {"d_off": 1}, {"h_off": 1}, {"m": 0}, {"alpha": 0.0}, {"alpha": float("nan")},
               {"alpha": float("inf")}, {"reg": -1.0}, {"reg": float("nan")}, {"lr": -1.0}, {"lr": float("inf")}):
        assert update(**kw) == (ERR_ARG, True), kw
        assert L.pinsage_last_error()


# ----------------------------------------------------------------------------- LMF.fit
def _small_matrix():
    """tests/test_gpu_als.py::_small_matrix: an empty row and an empty column."""
    rng = np.random.default_rng(90)
    R = (rng.random((70, 50)) < 0.15) * rng.integers(1, 5, (70, 50))
    R[11, :] = 0
    R[:, 23] = 0
    return au.csr_from_rows([(np.flatnonzero(r), r[r > 0]) for r in R], 50)


def _fixture_graph():
    import graph
    f = golden("jaccard")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    edges = f["edges"].astype(np.int64)
    return n, nc, graph.CSRGraph(n + nc, edges[:, 0], edges[:, 1])


def _col_track_matrix():
    import baselines as bl
    n, _, g = _fixture_graph()
    t = bl.to_col_track_matrix(g, list(range(n)))
    return tuple(a.cpu().numpy() for a in t[:3]) + t[3:]


_FIT_CACHE = {}


def _fit_reference(name, f):
    """(csr, X0, Y0, L at the start, L of the float64 fit after 30 iterations), computed once."""
    if (name, f) not in _FIT_CACHE:
        csr = _small_matrix() if name == "small" else _col_track_matrix()
        rng = np.random.default_rng(f)
        X0, Y0 = au.init_factors(rng, csr[3], f), au.init_factors(rng, csr[4], f)
        bx0, by0 = np.zeros(csr[3], np.float32), np.zeros(csr[4], np.float32)
        f64 = lu.fit(csr, X0, Y0, bx0, by0, REG, 1.0, LR, 30, np.float64)
        _FIT_CACHE[name, f] = (csr, X0, Y0, lu.objective(csr, X0, Y0, bx0, by0, REG, 1.0),
                               lu.objective(csr, *f64, REG, 1.0))
    return _FIT_CACHE[name, f]


@pytest.mark.parametrize("f", [16, 128])
@pytest.mark.parametrize("name", ["small", "col_track"])
def test_fit_from_given_factors(name, f):
    """L rises on every one of the 30 iterations and ends within 1e-4 relative of
    the float64 restatement's.  The tables themselves are not compared after 30
    iterations: AdaGrad's early steps amplify rounding, and the half-step tests
    above hold them where a comparison means something."""
    import baselines as bl
    csr, X0, Y0, start, want = _fit_reference(name, f)
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    xg, yg = torch.from_numpy(X0), torch.from_numpy(Y0).cuda()
    bxg, byg = torch.zeros(csr[3]).cuda(), torch.zeros(csr[4])
    seen = []
    m = bl.LMF(factors=f).fit(t, user_factors=xg, item_factors=yg, user_bias=bxg, item_bias=byg,
                              callback=lambda it, model: seen.append(model.objective()))
    assert torch.equal(xg, torch.from_numpy(X0)) and torch.equal(yg.cpu(), torch.from_numpy(Y0))   # copied
    assert not bxg.any() and not byg.any() and m.user_bias.any() and m.item_bias.any()
    for tab, shape in ((m.user_factors, (csr[3], f)), (m.item_factors, (csr[4], f)), (m.user_bias, (csr[3],)),
                       (m.item_bias, (csr[4],))):
        assert tab.is_cuda and tab.dtype == torch.float32 and tuple(tab.shape) == shape
    got = m.objective()
    print(f"{name}, f = {f}: L {start:.6g} -> {seen[0]:.6g} -> {got:.6g}, float64 {want:.6g}, "
          f"relative {abs(got - want) / abs(want):.2e}")
    assert len(seen) == 30 and seen[-1] == got and (np.diff([start] + seen) > 0).all(), seen
    assert abs(got - want) <= 1e-4 * abs(want)
    # given tables, biases included, are taken as they are and copied
    again = bl.LMF(factors=f, iterations=0).fit(t, m.user_factors, m.item_factors, m.user_bias, m.item_bias)
    assert again.objective() == got and again.user_factors.data_ptr() != m.user_factors.data_ptr()


def test_fit_checks_its_input():
    import baselines as bl
    csr = _small_matrix()
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        v = t[2].clone()
        v[3] = bad
        with pytest.raises(ValueError):
            bl.LMF(factors=8, iterations=1).fit((t[0], t[1], v) + t[3:])
    with pytest.raises(ValueError):
        bl.LMF(factors=8).fit(t, user_factors=torch.zeros(70, 4))
    with pytest.raises(ValueError):
        bl.LMF(factors=8).fit(t, item_bias=torch.zeros(70))
    with pytest.raises(ValueError):
        bl.LMF(factors=8).fit((t[0][:-1],) + t[1:])


def test_random_state_and_the_global_generator():
    import baselines as bl
    csr = _small_matrix()
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    a = bl.LMF(factors=8, iterations=2, random_state=7).fit(t)
    b = bl.LMF(factors=8, iterations=2, random_state=7).fit(t)
    for name in ("user_factors", "item_factors", "user_bias", "item_bias"):
        assert torch.equal(getattr(a, name), getattr(b, name))
    assert not torch.equal(a.item_factors, bl.LMF(factors=8, iterations=2, random_state=8).fit(t).item_factors)
    g = torch.Generator().manual_seed(7)
    m = bl.LMF(factors=8, iterations=0, random_state=7).fit(t)
    assert torch.equal(m.user_factors.cpu(), (torch.rand(70, 8, generator=g) - 0.5) / 8)
    assert torch.equal(m.item_factors.cpu(), (torch.rand(50, 8, generator=g) - 0.5) / 8)
    assert not m.user_bias.any() and not m.item_bias.any()
    torch.manual_seed(3)
    m = bl.LMF(factors=8, iterations=1).fit(t)
    after = torch.rand(1)
    torch.manual_seed(3)
    x0, y0 = (torch.rand(70, 8) - 0.5) / 8, (torch.rand(50, 8) - 0.5) / 8     # (70 + 50) * 8 draws
    assert torch.equal(after, torch.rand(1))
    want = bl.LMF(factors=8, iterations=1).fit(t, user_factors=x0, item_factors=y0)
    assert torch.equal(m.item_factors, want.item_factors) and torch.equal(m.item_bias, want.item_bias)


# ----------------------------------------------------------------------------- the two baselines
@pytest.fixture(scope="module")
def cf():
    import baselines as bl
    n, _, g = _fixture_graph()
    rng = np.random.default_rng(95)
    pos = rng.integers(0, n, (330, 2))
    pos = np.concatenate([pos, pos[rng.integers(0, 330, 70)]])      # 400 positives, with repeats
    tp = torch.from_numpy(pos)
    ids = list(range(n))
    torch.manual_seed(1)
    ct, tt = bl.ColTrackLMF(), bl.TrackTrackLMF(factors=16)
    ct.train(g, ids, tp, None, None)
    tt.train(g, ids, tp, None, None)
    return n, g, tp, ids, {"ColTrackCfLMF": ct, "TrackTrackCfLMF": tt}


@pytest.mark.parametrize("k", [1, 10, 299])
def test_cf_knn_is_knn_from_emb(cf, k):
    import baselines as bl
    n, _, _, _, models = cf
    assert models["ColTrackCfLMF"].model.factors == 128 and models["TrackTrackCfLMF"].model.factors == 16
    for name, m in models.items():
        assert isinstance(m.model, bl.LMF) and tuple(m.model.item_factors.shape) == (n, m.model.factors)
        assert tuple(m.model.item_bias.shape) == (n,) and bool(m.model.item_bias.any())
        for nodeset in (torch.arange(n), torch.tensor([5, 5, 299, 0]), torch.tensor([7, 3]).cuda()):
            w, nb = m.knn(nodeset, k)
            want_w, want_n = bl.knn_from_emb(m.model.item_factors, nodeset, k)
            assert tuple(w.shape) == tuple(nb.shape) == (len(nodeset), k)
            assert w.dtype == torch.float32 and nb.dtype == torch.int64
            assert w.device == nodeset.device and nb.device == nodeset.device
            assert torch.equal(w.cpu(), want_w.cpu()) and torch.equal(nb.cpu(), want_n.cpu()), name
        ids_, scores = m.model.similar_items(torch.tensor([4, 9]), 6)
        assert tuple(ids_.shape) == (2, 6) and ids_.dtype == torch.int64 and scores.dtype == torch.float32
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())


def test_tables_end_to_end(cf, tmp_path, monkeypatch):
    import baselines as bl
    n, g, tp, ids, models = cf
    monkeypatch.setattr(bl, "PRECOMP_K", 200)         # 300 tracks: lists of 1000 do not exist
    for name, m in models.items():
        bl.save_knn(m, name, ids, str(tmp_path), train_time=2.0, b_size=128)
    d = bl.LazyKnnDict(list(models), ids, str(tmp_path))
    table = bl.compute_results_table(d, tp, g)
    assert list(table.index) == ["ColTrackCfLMF", "TrackTrackCfLMF"]
    assert np.isfinite(table.to_numpy(dtype=np.float64)).all()
    feats = torch.from_numpy(np.random.default_rng(96).standard_normal((n, 12)).astype(np.float32))
    np.random.seed(11)
    beyond = bl.compute_beyond_accuracy_table({name: d[name] for name in models}, tp, g, feats)
    assert list(beyond.index) == list(table.index) and np.isfinite(beyond.to_numpy(dtype=np.float64)).all()
    for name, m in models.items():
        w, nb = m.knn(torch.arange(n), 200)           # one batch against the three of save_knn
        sw, sn = d[name]
        assert tuple(nb.shape) == (n, 200) and torch.equal(sn, nb) and torch.equal(sw, w)
        assert table.loc[name, "hr (k=10)"] == bl.hit_rate(nb, tp, 10)
        assert table.loc[name, "t (train)"] == 2.0
