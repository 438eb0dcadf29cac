"""The kernels of csrc/bpr.hip (pinsage_bpr_sample, pinsage_bpr_apply) and what
stands on them: baselines.BPR, ColTrackBPR and TrackTrackBPR, and with save_knn
/ LazyKnnDict the two tables end to end.  The references are tests/bpr_util.py,
checked on the host in tests/test_bpr_host.py.

Sample kernel.  neg is integer work and has to equal the reference bit for bit.
w is held against float64 under a derived bound, with u = 2^-24 and
parity_util.gemm_bound:
    ds_i <= gemm_bound(f, |x|.|y_i| + |b_i|)            a score: f products, the wave sum, the bias add
    dz   <= ds_i + ds_j + u |z|                         the subtraction
    dw   <= dz / 4 + 8 u w                              sig' <= 1/4; exp, add, divide
Every test prints its worst ratio to it.

Apply kernel.  New x, bx are held against the float64 restatement by
als_util.row_errors under the project's rule: the device's error is at most
als_util.TOL_FACTOR (8) times the float32 restatement's on the same inputs;
both are printed.  The accumulators are seeded in [0.5, 2]: from zero an entry
with a tiny gradient is divided by about 1e-3 and the ratio measures nothing.
From zero accumulators the gradient itself (sqrt(h_new)) is held by the same
rule, as tests/test_gpu_lmf.py does.

BPR.fit.  The draws are compared bit for bit, round by round.  The held-out
objective (the draw of round 2 * iterations, which no iteration uses) has to end
above its start and within TOL_FACTOR times the gap between the float32 and the
float64 restatement of the same fit, the gap tests/test_bpr_host.py prints for
the planted matrix; the margin and the value are printed.

Tables are passed with NaN in their padding columns and a sentinel tail; the
padding has to be NaN and the tail untouched afterwards.
"""
import numpy as np
import pytest
import torch

import als_util as au
import bpr_util as bu
import lmf_util as lu
import n2v_util as nu
import parity_util as pu
from conftest import golden
from rowfit_util import PAD, SENT, _padded, _unpad

pytestmark = pytest.mark.gpu

ERR_ARG = -2       # pinsage_status (include/pinsage_hip.h)
U = 2.0 ** -24
REG, LR = 0.01, 0.1
SEED = 0x5EEDBA5E0FB9
ISENT = -123


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


def _sample(csr, X, Y, b, S, seed=SEED, rho=0, offset=0, cell_base=0, pad=0):
    """pinsage_bpr_sample into sentinel-filled outputs: (status, neg, w, error word)."""
    import _native as nat
    ptr, idx, _, n, m = csr
    f = X.shape[1]
    ns = len(idx) * S
    xd, yd, bd = _padded(X, f + pad), _padded(Y, f + pad), _vec(b)
    negd = torch.full((ns + PAD,), ISENT, dtype=torch.int32, device="cuda")
    wd = torch.full((ns + PAD,), SENT, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ptr, idx)]
    rc = nat.lib().pinsage_bpr_sample(nat.ptr(t[0]), nat.ptr(t[1]), n, cell_base, nat.ptr(xd), f + pad, nat.ptr(yd),
                                      nat.ptr(bd), m, f + pad, f, S, seed, rho, offset, nat.ptr(negd), nat.ptr(wd),
                                      nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    neg, w = negd.cpu().numpy(), wd.cpu().numpy()
    assert (neg[ns:] == ISENT).all() and (w[ns:] == SENT).all(), "values behind the outputs were written"
    _unpad(xd, n, f, f + pad), _unpad(yd, m, f, f + pad)      # the tables' padding is still NaN
    return rc, neg[:ns].copy(), w[:ns].copy(), int(err)


_DRAWS = {}


def _draw(name, csr, S, seed=SEED, rho=0, offset=0):
    """bpr_util.draw, computed once per (matrix, S, seed, rho, offset): it does not depend on the tables."""
    key = (name, S, seed, rho, offset)
    if key not in _DRAWS:
        _DRAWS[key] = bu.draw(csr, S, seed, rho, offset)
    return _DRAWS[key]


def _tables(csr, f, seed):
    """Tables at eight times the documented initial scale and a trained-size bias."""
    rng = np.random.default_rng(seed)
    return (au.init_factors(rng, csr[3], f) * 8, au.init_factors(rng, csr[4], f) * 8,
            rng.normal(0, 0.5, csr[4]).astype(np.float32))


def _w_ratio(csr, neg, w, S, X, Y, b):
    """The worst |w - w64| over the bound of the module docstring."""
    f = X.shape[1]
    X64, Y64, b64 = (np.asarray(a, np.float64) for a in (X, Y, b))
    u, i = bu.samples(csr, S)
    ok = neg >= 0
    j = np.where(ok, neg, 0).astype(np.int64)
    z = bu.scores(csr, neg, S, X64, Y64, b64, np.float64)
    w64 = bu.weights(csr, neg, S, X64, Y64, b64, np.float64)
    ax = np.abs(X64[u])
    dz = (pu.gemm_bound(f, (ax * np.abs(Y64[i])).sum(1) + np.abs(b64[i]))
          + pu.gemm_bound(f, (ax * np.abs(Y64[j])).sum(1) + np.abs(b64[j])) + U * np.abs(z))
    bound = dz / 4 + 8 * U * w64
    assert (w[~ok] == 0).all() and np.isfinite(w).all()
    return float((np.abs(w - w64)[ok] / bound[ok]).max()) if ok.any() else 0.0


def _check_sample(name, csr, S, f, what, pad=0, **kw):
    X, Y, b = _tables(csr, f, seed=f + S)
    rc, neg, w, err = _sample(csr, X, Y, b, S, pad=pad, **kw)
    assert rc == 0 and err == 0
    assert np.array_equal(neg, _draw(name, csr, S, **kw)), what
    ratio = _w_ratio(csr, neg, w, S, X, Y, b)
    print(f"{what}: {int((neg < 0).sum())} void of {len(neg)}, worst ratio of w to the bound {ratio:.3f}")
    assert ratio <= 1, (what, ratio)
    return neg, w


def _small_matrix():
    """tests/test_gpu_als.py::_small_matrix: an empty row and an empty column."""
    rng = np.random.default_rng(90)
    R = (rng.random((70, 50)) < 0.15) * rng.integers(1, 5, (70, 50))
    R[11, :] = 0
    R[:, 23] = 0
    return au.csr_from_rows([(np.flatnonzero(r), r[r > 0]) for r in R], 50)


def _edge_matrix():
    """600 items: a full row, a row missing item 77 only, rows of kRowLong,
    kRowLong + 1 and 3 x 64 + 1 items, an empty row, a row of one."""
    import _native as nat
    long_row = int(nat.lib().pinsage_lmf_long_row())
    rng = np.random.default_rng(12)
    rows = [(np.arange(600), np.ones(600)), (np.delete(np.arange(600), 77), np.ones(599))]
    rows += [(np.sort(rng.choice(600, n, replace=False)), np.ones(n)) for n in (long_row, long_row + 1, 193, 0, 1)]
    csr = au.csr_from_rows(rows, 600)
    assert {lu.row_form(int(n), long_row) for n in np.diff(csr[0])} == {"wave", "workgroup"}
    return csr


# ----------------------------------------------------------------------------- the sample kernel
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("f,pad", [(4, 0), (60, 4), (128, 0), (128, 4)])
def test_sample_small_matrix(f, pad, S):
    csr = _small_matrix()
    assert (np.diff(csr[0]) == 0).any() and not (csr[1] == 23).any()
    _check_sample("small", csr, S, f, f"f = {f}, ld = f + {pad}, negatives = {S}", pad=pad)


@pytest.mark.parametrize("S", [1, 3])
def test_sample_full_rows_and_both_row_forms(S):
    csr = _edge_matrix()
    ptr = csr[0]
    neg, _ = _check_sample("edge", csr, S, 8, f"edge rows, negatives = {S}")
    assert (neg[:ptr[1] * S] == -1).all()
    but_one = neg[ptr[1] * S:ptr[2] * S]
    assert np.isin(but_one, (-1, 77)).all() and (but_one == 77).any() and (but_one == -1).any()


def test_sample_one_item():
    """n_items = 1: a row that holds the item is all void, and no row can hold anything else."""
    csr = au.csr_from_rows([([0], [1]), ([], []), ([0], [1])], 1)
    neg, w = _check_sample("one", csr, 8, 4, "one item")
    assert (neg == -1).all() and (w == 0).all()


@pytest.mark.parametrize("seed,rho,offset", [(SEED, 1, 0), (SEED, 0, 1), (SEED + 1, 0, 0), (2 ** 64 - 1, 2 ** 27 - 1, 7),
                                             (5, 41, 2 ** 32 - 1)])
def test_sample_seed_round_and_offset(seed, rho, offset):
    csr = _small_matrix()
    neg, _ = _check_sample("small", csr, 3, 16, f"seed {seed:#x}, rho {rho}, offset {offset}", seed=seed, rho=rho,
                           offset=offset)
    assert not np.array_equal(neg, _draw("small", csr, 3))


def test_sample_bits_repeat_and_do_not_depend_on_the_batch():
    csr = _edge_matrix()
    ptr, idx, val, n, m = csr
    X, Y, b = _tables(csr, 128, seed=3)
    a, c = _sample(csr, X, Y, b, 3, rho=4), _sample(csr, X, Y, b, 3, rho=4)
    assert a[0] == 0 and np.array_equal(a[1], c[1]) and np.array_equal(a[2].view(np.uint32), c[2].view(np.uint32))
    for r0, r1 in ((0, 3), (3, n), (4, 5)):                  # two calls, and a row alone: another block, wave and grid
        part = (ptr[r0:r1 + 1] - ptr[r0], idx[ptr[r0]:ptr[r1]], val[ptr[r0]:ptr[r1]], r1 - r0, m)
        got = _sample(part, X[r0:r1], Y, b, 3, rho=4, cell_base=int(ptr[r0]))
        sl = slice(ptr[r0] * 3, ptr[r1] * 3)
        assert got[0] == 0 and np.array_equal(got[1], a[1][sl]), (r0, r1)
        assert np.array_equal(got[2].view(np.uint32), a[2][sl].view(np.uint32)), (r0, r1)
    # without the first cell's index the block draws for other samples
    part = (ptr[3:] - ptr[3], idx[ptr[3]:], val[ptr[3]:], n - 3, m)
    assert not np.array_equal(_sample(part, X[3:], Y, b, 3, rho=4)[1], a[1][ptr[3] * 3:])


def test_sample_id_out_of_range_sets_the_error_word():
    import baselines as bl
    csr = _small_matrix()
    X, Y, b = _tables(csr, 8, seed=70)
    for bad in (50, -1, 2 ** 31 - 1):
        idx = csr[1].copy()
        idx[5] = bad
        rc, neg, w, err = _sample((csr[0], idx) + csr[2:], X, Y, b, 2)
        assert rc == 0 and err == 1 and np.isfinite(w).all() and ((neg >= -1) & (neg < 50)).all()
    idx = csr[1].copy()
    idx[csr[0][3] - 1] = 50                                   # the last cell of a row: still ascending
    t = tuple(torch.from_numpy(a).cuda() for a in (csr[0], idx, csr[2])) + csr[3:]
    with pytest.raises(IndexError):
        bl.BPR(factors=8, iterations=1).fit(t)


def test_sample_refusals_leave_the_outputs_untouched():
    import _native as nat
    L = nat.lib()
    n, m, f = 5, 9, 8
    rng = np.random.default_rng(80)
    csr = au.random_csr(rng, [2, 0, 3, 1, 4], m, "ones")
    ptr, idx = (torch.from_numpy(a).cuda() for a in csr[:2])
    X = torch.from_numpy(au.init_factors(rng, n + 2, 16)).cuda().reshape(-1)
    Y = torch.from_numpy(au.init_factors(rng, m + 2, 16)).cuda().reshape(-1)
    by = torch.zeros(m, device="cuda")

    def sample(f=f, ldx=f, ldy=f, x_off=0, y_off=0, m=m, S=2, rho=0, cell_base=0, n=n, no_ptr=False, no_by=False):
        neg = torch.full((10 * 8 + PAD,), ISENT, dtype=torch.int32, device="cuda")
        w = torch.full((10 * 8 + PAD,), SENT, dtype=torch.float32, device="cuda")
        rc = L.pinsage_bpr_sample(None if no_ptr else nat.ptr(ptr), nat.ptr(idx), n, cell_base, nat.ptr(X[x_off:]),
                                  ldx, nat.ptr(Y[y_off:]), None if no_by else nat.ptr(by), m, ldy, f, S, SEED, rho, 0,
                                  nat.ptr(neg), nat.ptr(w), None, nat.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((neg == ISENT).all() and (w == SENT).all())

    assert sample() == (0, False)                           # the accepted call writes
    assert sample(S=8, rho=2 ** 27 - 1) == (0, False)
    assert sample(n=0) == (0, True)                         # no rows: accepted, nothing launched
    for kw in ({"f": 6}, {"f": 132, "ldx": 132, "ldy": 132}, {"f": 0}, {"ldx": 4}, {"ldy": 4}, {"ldx": 10},
               {"ldy": 10}, {"x_off": 1}, {"y_off": 1}, {"m": 0}, {"S": 0}, {"S": 9}, {"rho": -1}, {"rho": 2 ** 27},
               {"cell_base": -1}, {"no_ptr": True}, {"no_by": True}, {"n": -1}):
        assert sample(**kw) == (ERR_ARG, True), kw
        assert L.pinsage_last_error()


# ----------------------------------------------------------------------------- the apply kernel
def _apply(csr, X, H, Y, bx=None, hb=None, reg=REG, lr=LR, pad=0, forms=None):
    """pinsage_bpr_apply: (status, X, H, bx, hb, error word); bx, hb None without a bias pair."""
    import _native as nat
    L = nat.lib()
    ptr, idx, val, n, m = csr
    f = X.shape[1]
    if forms is not None:
        long_row = int(L.pinsage_lmf_long_row())
        got = {lu.row_form(int(ln), long_row) for ln in np.diff(ptr)}
        assert got == set(forms), (got, forms)
    xd, hd, yd = _padded(X, f + pad, tail=True), _padded(H, f + pad, tail=True), _padded(Y, f + pad)
    bxd = hbd = None
    if bx is not None:
        bxd, hbd = _vec(bx, tail=True), _vec(hb, tail=True)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ptr, idx.astype(np.int32), val.astype(np.float32))]
    rc = L.pinsage_bpr_apply(nat.ptr(t[0]), nat.ptr(t[1]), nat.ptr(t[2]), n, nat.ptr(yd), m, f + pad, nat.ptr(xd),
                             nat.ptr(bxd), f + pad, f, nat.ptr(hd), f + pad, nat.ptr(hbd), reg, lr, nat.ptr(err),
                             nat.stream_ptr())
    torch.cuda.synchronize()
    _unpad(yd, m, f, f + pad)
    return (rc, _unpad(xd, n, f, f + pad), _unpad(hd, n, f, f + pad), None if bx is None else _unvec(bxd, n),
            None if bx is None else _unvec(hbd, n), int(err))


MIXED = [0, 1, 2, 63, 64, 65, 257]


def _apply_case(f, seed, lengths=MIXED, n_other=300, seeded=True, bias=True):
    """Entries with distinct ids and values of either sign in +-[0.05, 0.95],
    tables at eight times the initial scale, accumulators uniform in [0.5, 2] or zero."""
    rng = np.random.default_rng(seed)
    ptr, idx, val, n, m = au.random_csr(rng, lengths, n_other, "fractions")
    csr = (ptr, idx, (val * rng.choice([-1.0, 1.0], len(val))).astype(np.float32), n, m)
    X, Y = au.init_factors(rng, n, f) * 8, au.init_factors(rng, n_other, f) * 8
    lo, hi = (0.5, 2.0) if seeded else (0.0, 0.0)
    H = rng.uniform(lo, hi, (n, f)).astype(np.float32)
    if not bias:
        return csr, X, H, Y, None, None
    return csr, X, H, Y, rng.normal(0, 0.5, n).astype(np.float32), rng.uniform(lo, hi, n).astype(np.float32)


def _check_apply(case, what, **kw):
    """The device against float64 under the 8x rule; returns the device's tables."""
    csr, X, H, Y, bx, hb = case
    got = _apply(*case, **kw)
    assert got[0] == 0 and got[5] == 0
    r64 = bu.apply(*csr[:3], X, H, Y, REG, LR, np.float64, bx, hb)
    r32 = bu.apply(*csr[:3], X, H, Y, REG, LR, np.float32, bx, hb)
    pairs = [("x", 0, 1, X)] + ([("bx", 2, 3, bx[:, None])] if bx is not None else [])
    for name, i, k, x_in in pairs:
        w64, w32, dev = (np.asarray(a).reshape(len(x_in), -1) for a in (r64[i], r32[i], got[k]))
        e32, edev = au.row_errors(w32, w64, x_in).max(), au.row_errors(dev, w64, x_in).max()
        print(f"{what}, {name}: float32 restatement {e32:.3e}, device {edev:.3e}, ratio {edev / e32:.2f}")
        assert e32 > 0 and edev <= au.TOL_FACTOR * e32, (what, name, edev, e32)
    return got


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("f,pad", [(4, 0), (64, 4), (128, 0)])
def test_apply_factors_and_leading_dimensions(f, pad, bias):
    _check_apply(_apply_case(f, seed=f + pad + bias, bias=bias), f"f = {f}, every ld = f + {pad}, bias {bias}",
                 pad=pad, forms=["wave"])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("f", [4, 128])
def test_apply_long_rows(f, bias):
    """Rows on both sides of the switch to the workgroup form, a hub of 5000
    entries over 6000 others, two long rows in one block of 8 rows and one in the next."""
    import _native as nat
    long_row = int(nat.lib().pinsage_lmf_long_row())
    lengths = [5000, 3, long_row, long_row + 1, 0, 64, long_row + 64, 1, 2, long_row + 129, 7]
    _check_apply(_apply_case(f, seed=7 + f + bias, lengths=lengths, n_other=6000, bias=bias),
                 f"long rows, f = {f}, bias {bias}", forms=["wave", "workgroup"], pad=4)


@pytest.mark.parametrize("half", ["user", "item"])
def test_apply_on_the_entries_of_a_draw(half):
    """The fit's own entry arrays: repeated ids, +w beside -w, the +-0 of void samples."""
    csr = _edge_matrix()
    S, f = 2, 16
    X, Y, b = _tables(csr, f, seed=5)
    neg = _draw("edge", csr, S)
    w = bu.weights(csr, neg, S, X, Y, b, np.float32)
    rng = np.random.default_rng(6)
    if half == "user":
        ent = bu.user_entries(csr, neg, w, S) + (csr[3], csr[4])
        case = (ent, X, rng.uniform(0.5, 2, X.shape).astype(np.float32), Y, None, None)
    else:
        ent = bu.item_entries(csr, neg, w, S) + (csr[4], csr[3])
        case = (ent, Y, rng.uniform(0.5, 2, Y.shape).astype(np.float32), X, b,
                rng.uniform(0.5, 2, len(b)).astype(np.float32))
    _check_apply(case, f"{half} half of a draw", forms=["wave", "workgroup"] if half == "user" else ["wave"])


@pytest.mark.parametrize("f", [4, 64, 128])
def test_apply_from_zero_accumulators(f):
    """The gradient (sqrt(h_new)) under the 8x rule; float64's sign wherever
    |g64| exceeds 1e-3 of the row's largest."""
    case = _apply_case(f, seed=30 + f, lengths=MIXED + [600], n_other=700, seeded=False)
    csr, X, H, Y, bx, hb = case
    rc, xn, hn, bxn, hbn, err = _apply(*case)
    assert rc == 0 and err == 0
    r64 = bu.apply(*csr[:3], X, H, Y, REG, LR, np.float64, bx, hb)
    r32 = bu.apply(*csr[:3], X, H, Y, REG, LR, np.float32, bx, hb)
    for name, old, new, h, i in (("x", X, xn, hn, 0), ("bx", bx[:, None], bxn[:, None], hbn[:, None], 2)):
        g64 = lu.implied_gradient(old, np.reshape(r64[i], old.shape), np.reshape(r64[i + 1], old.shape))
        a32 = np.sqrt(np.reshape(r32[i + 1], old.shape).astype(np.float64))
        zero = np.zeros_like(g64)
        e32 = au.row_errors(a32, np.abs(g64), zero).max()
        edev = au.row_errors(np.sqrt(h.astype(np.float64)), np.abs(g64), zero).max()
        print(f"f = {f}, |g| of {name}: float32 restatement {e32:.3e}, device {edev:.3e}, ratio {edev / e32:.2f}")
        assert e32 > 0 and edev <= au.TOL_FACTOR * e32
        big = np.abs(g64) > 1e-3 * np.abs(g64).max(axis=1, keepdims=True)
        assert big.sum() >= len(X) - 1                        # the empty row's bias gradient is exactly 0
        assert np.array_equal(np.sign(new.astype(np.float64) - old)[big], np.sign(g64)[big])


def test_zero_learning_rate_leaves_the_tables_bit_for_bit():
    case = _apply_case(8, seed=40, lengths=MIXED + [600], n_other=700)
    csr, X, H, Y, bx, hb = case
    rc, xn, hn, bxn, hbn, err = _apply(*case, lr=0.0, pad=4)
    assert rc == 0 and err == 0
    assert np.array_equal(xn.view(np.uint32), X.view(np.uint32))
    assert np.array_equal(bxn.view(np.uint32), bx.view(np.uint32))
    moved = _apply(*case, pad=4)
    assert np.array_equal(hn.view(np.uint32), moved[2].view(np.uint32)) and (hn >= H).all() and (hn > H).any()
    assert np.array_equal(hbn.view(np.uint32), moved[4].view(np.uint32))
    assert (hbn >= hb).all() and (hbn > hb).any()
    assert not np.array_equal(moved[1], X) and not np.array_equal(moved[3], bx)


def test_an_empty_row_without_regularisation_keeps_x_exactly():
    case = _apply_case(8, seed=41)
    csr, X, H, Y, bx, hb = case
    assert csr[0][1] == csr[0][0]
    for seeded in (case, _apply_case(8, seed=41, seeded=False)):
        rc, xn, hn, bxn, hbn, err = _apply(*seeded, reg=0.0)
        assert rc == 0 and np.array_equal(xn[0].view(np.uint32), seeded[1][0].view(np.uint32))
        assert np.array_equal(hn[0], seeded[2][0]) and bxn[0] == seeded[4][0] and hbn[0] == seeded[5][0]
        assert not np.array_equal(xn[3], seeded[1][3])


def test_apply_bits_repeat_and_do_not_depend_on_the_batch():
    case = _apply_case(128, seed=60, lengths=MIXED + [5000, 600], n_other=6000)
    csr, X, H, Y, bx, hb = case
    a, c = _apply(*case), _apply(*case)
    for i in range(1, 5):
        assert np.array_equal(a[i].view(np.uint32), c[i].view(np.uint32))
    ptr, idx, val = csr[:3]
    for u in (3, 7, 8):                                      # another grid, block of rows, wave; the hub
        one = au.csr_from_rows([(idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]])], 6000)
        s = slice(u, u + 1)
        alone = _apply(one, X[s], H[s], Y, bx[s], hb[s])
        for i in range(1, 5):
            assert np.array_equal(alone[i].view(np.uint32), a[i][s].view(np.uint32)), (u, i)
    # the factor rows do not depend on whether a bias pair rides along
    bare = _apply(csr, X, H, Y)
    assert np.array_equal(bare[1].view(np.uint32), a[1].view(np.uint32)) and bare[3] is None


def test_apply_id_out_of_range_sets_the_error_word():
    case = _apply_case(8, seed=70)
    csr = case[0]
    for bad in (300, -1, 2 ** 31 - 1):
        idx = csr[1].copy()
        idx[5] = bad
        got = _apply((csr[0], idx) + csr[2:], *case[1:])
        assert got[0] == 0 and got[5] == 1 and all(np.isfinite(a).all() for a in got[1:5])


def test_apply_refusals_leave_the_outputs_untouched():
    import _native as nat
    L = nat.lib()
    n, m, f = 5, 9, 8
    rng = np.random.default_rng(80)
    csr = au.random_csr(rng, [2, 0, 3, 1, 4], m, "fractions")
    ptr, idx, val = (torch.from_numpy(a).cuda() for a in csr[:3])
    Y = torch.from_numpy(au.init_factors(rng, m + 2, 16)).cuda().reshape(-1)

    def apply(f=f, ldx=f, ldy=f, ldh=f, x_off=0, y_off=0, h_off=0, m=m, reg=REG, lr=LR, bias="both", no_ptr=False):
        outs = [torch.full((k + PAD,), SENT, dtype=torch.float32, device="cuda") for k in (n * 16, n, n * 16, n)]
        X, bx, H, hb = outs
        rc = L.pinsage_bpr_apply(None if no_ptr else nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n, nat.ptr(Y[y_off:]),
                                 m, ldy, nat.ptr(X[x_off:]), nat.ptr(bx) if bias in ("both", "bx") else None, ldx, f,
                                 nat.ptr(H[h_off:]), ldh, nat.ptr(hb) if bias in ("both", "hb") else None, reg, lr,
                                 None, nat.stream_ptr())
        torch.cuda.synchronize()
        return rc, all(bool((o == SENT).all()) for o in outs)

    assert apply() == (0, False)                            # the accepted calls write
    assert apply(bias="none") == (0, False)
    for kw in ({"f": 6}, {"f": 132, "ldx": 132, "ldy": 132, "ldh": 132}, {"f": 0}, {"ldx": 4}, {"ldy": 4},
               {"ldh": 4}, {"ldx": 10}, {"ldy": 10}, {"ldh": 10}, {"x_off": 1}, {"y_off": 1}, {"h_off": 1}, {"m": 0},
               {"reg": -1.0}, {"reg": float("nan")}, {"lr": -1.0}, {"lr": float("inf")}, {"bias": "bx"},
               {"bias": "hb"}, {"no_ptr": True}):
        assert apply(**kw) == (ERR_ARG, True), kw
        assert L.pinsage_last_error()


# ----------------------------------------------------------------------------- BPR.fit
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


ITERATIONS = 10
NEGATIVES = {"small": 2, "col_track": 1}
_FIT_CACHE = {}


def _fit_reference(name, f):
    """(csr, X0, Y0, {rho: neg}, L at the start, L of the float64 fit, L of the
    float32 fit), the objectives on the held-out draw; computed once."""
    if (name, f) not in _FIT_CACHE:
        csr = _small_matrix() if name == "small" else _col_track_matrix()
        S = NEGATIVES[name]
        rng = np.random.default_rng(f)
        X0, Y0 = au.init_factors(rng, csr[3], f), au.init_factors(rng, csr[4], f)
        b0 = np.zeros(csr[4], np.float32)
        draws = {rho: _draw(name, csr, S, rho=rho) for rho in range(2 * ITERATIONS + 1)}
        held = draws[2 * ITERATIONS]
        ends = [bu.objective(csr, *bu.fit(csr, X0, Y0, b0, S, SEED, REG, LR, ITERATIONS, dt, draws=draws), held, S, REG)
                for dt in (np.float64, np.float32)]
        _FIT_CACHE[name, f] = (csr, X0, Y0, draws, bu.objective(csr, X0, Y0, b0, held, S, REG), *ends)
    return _FIT_CACHE[name, f]


@pytest.mark.parametrize("f", [16, 128])
@pytest.mark.parametrize("name", ["small", "col_track"])
def test_fit_from_given_factors(name, f):
    import baselines as bl
    csr, X0, Y0, draws, start, want, want32 = _fit_reference(name, f)
    S = NEGATIVES[name]
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    xg, yg, bg = torch.from_numpy(X0), torch.from_numpy(Y0).cuda(), torch.zeros(csr[4])
    seen = []
    m = bl.BPR(factors=f, learning_rate=LR, regularization=REG, iterations=ITERATIONS, negatives=S, random_state=SEED)
    m.fit(t, user_factors=xg, item_factors=yg, item_bias=bg, callback=lambda it, model: seen.append(it))
    assert seen == list(range(ITERATIONS))
    assert torch.equal(xg, torch.from_numpy(X0)) and torch.equal(yg.cpu(), torch.from_numpy(Y0))   # copied
    assert not bg.any() and m.item_bias.any()
    for tab, shape in ((m.user_factors, (csr[3], f)), (m.item_factors, (csr[4], f)), (m.item_bias, (csr[4],))):
        assert tab.is_cuda and tab.dtype == torch.float32 and tuple(tab.shape) == shape
    for rho, neg in draws.items():                           # every round's draw, the held-out one included
        got, w = m.sample(rho)
        assert got.dtype == torch.int32 and w.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), neg), rho
    got = m.objective()
    assert got == m.objective(torch.from_numpy(draws[2 * ITERATIONS]))
    margin = au.TOL_FACTOR * abs(want32 - want)
    print(f"{name}, f = {f}: objective {start:.6g} -> {got:.9g}, float64 {want:.9g}, float32 {want32:.9g}, "
          f"difference {abs(got - want):.3e}, margin {margin:.3e}")
    assert got > start
    assert abs(got - want) <= margin
    # given tables, the bias included, are taken as they are and copied
    again = bl.BPR(factors=f, iterations=0, negatives=S, regularization=REG, random_state=SEED)
    again.fit(t, m.user_factors, m.item_factors, m.item_bias)
    assert again.objective(torch.from_numpy(draws[2 * ITERATIONS])) == got
    assert again.user_factors.data_ptr() != m.user_factors.data_ptr()


def test_fit_checks_its_input():
    import baselines as bl
    csr = _small_matrix()
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        v = t[2].clone()
        v[3] = bad
        with pytest.raises(ValueError):
            bl.BPR(factors=8, iterations=1).fit((t[0], t[1], v) + t[3:])
    b, e = int(csr[0][0]), int(csr[0][1])
    assert e - b >= 2
    for swap in ((b, b + 1), (e - 2, e - 1)):               # two neighbours descending; below, a cell twice
        idx = t[1].clone()
        idx[swap[0]], idx[swap[1]] = t[1][swap[1]], t[1][swap[0]]
        with pytest.raises(ValueError, match="ascending"):
            bl.BPR(factors=8, iterations=1).fit((t[0], idx) + t[2:])
    idx = t[1].clone()
    idx[b + 1] = idx[b]
    with pytest.raises(ValueError, match="ascending"):
        bl.BPR(factors=8, iterations=1).fit((t[0], idx) + t[2:])
    with pytest.raises(ValueError):
        bl.BPR(factors=8).fit(t, user_factors=torch.zeros(70, 4))
    with pytest.raises(ValueError):
        bl.BPR(factors=8).fit(t, item_bias=torch.zeros(70))
    with pytest.raises(ValueError):
        bl.BPR(factors=8).fit((t[0][:-1],) + t[1:])


def test_random_state_and_the_global_generator():
    import baselines as bl
    csr = _small_matrix()
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    names = ("user_factors", "item_factors", "item_bias")
    a = bl.BPR(factors=8, iterations=2, random_state=7).fit(t)
    b = bl.BPR(factors=8, iterations=2, random_state=7).fit(t)
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name))
    assert torch.equal(a.sample(9)[0], b.sample(9)[0]) and torch.equal(a.sample(9)[1], b.sample(9)[1])
    c = bl.BPR(factors=8, iterations=2, random_state=8).fit(t)
    assert not torch.equal(a.item_factors, c.item_factors) and not torch.equal(a.sample(9)[0], c.sample(9)[0])
    g = torch.Generator().manual_seed(7)
    m = bl.BPR(factors=8, iterations=0, random_state=7).fit(t)
    assert torch.equal(m.user_factors.cpu(), (torch.rand(70, 8, generator=g) - 0.5) / 8)
    assert torch.equal(m.item_factors.cpu(), (torch.rand(50, 8, generator=g) - 0.5) / 8)
    assert not m.item_bias.any()
    assert np.array_equal(m.sample(3)[0].cpu().numpy(), bu.draw(csr, 1, 7, 3))
    torch.manual_seed(3)
    m = bl.BPR(factors=8, iterations=1).fit(t)
    after = torch.rand(1)
    torch.manual_seed(3)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))          # drawn before the tables
    x0, y0 = (torch.rand(70, 8) - 0.5) / 8, (torch.rand(50, 8) - 0.5) / 8
    assert torch.equal(after, torch.rand(1))
    want = bl.BPR(factors=8, iterations=1, random_state=seed).fit(t, user_factors=x0, item_factors=y0)
    for name in names:
        assert torch.equal(getattr(m, name), getattr(want, name))
    assert torch.equal(m.sample(5)[0], want.sample(5)[0])


def test_planted_matrix_separates_the_groups_on_the_device():
    """tests/test_bpr_host.py's settings: f = 16, lr 0.1, 30 iterations."""
    import baselines as bl
    csr, groups = bu.planted_matrix(1)
    rng = np.random.default_rng(16)
    X0, Y0 = au.init_factors(rng, csr[3], 16), au.init_factors(rng, csr[4], 16)
    t = tuple(torch.from_numpy(a).cuda() for a in csr[:3]) + csr[3:]
    m = bl.BPR(factors=16, learning_rate=0.1, regularization=0.01, iterations=30, random_state=SEED)
    start = bl.BPR(factors=16, regularization=0.01, iterations=0, random_state=SEED).fit(t, X0, Y0)
    m.fit(t, X0, Y0)
    held = m.sample(60)[0]
    seen = np.flatnonzero(np.bincount(csr[1], minlength=csr[4]) > 0)
    share = nu.same_group_share(m.item_factors.cpu().numpy(), groups, seen)
    print(f"objective {start.objective(held):.6g} -> {m.objective():.6g}, same-group share {share:.3f}")
    assert m.objective() > start.objective(held)
    assert share >= 0.5


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
    ct, tt = bl.ColTrackBPR(), bl.TrackTrackBPR(factors=16)
    ct.train(g, ids, tp, None, None)
    tt.train(g, ids, tp, None, None)
    return n, g, tp, ids, {"ColTrackCfBPR": ct, "TrackTrackCfBPR": tt}


@pytest.mark.parametrize("k", [1, 10, 299])
def test_cf_knn_is_knn_from_emb(cf, k):
    import baselines as bl
    n, _, _, _, models = cf
    assert models["ColTrackCfBPR"].model.factors == 128 and models["TrackTrackCfBPR"].model.factors == 16
    for name, m in models.items():
        assert isinstance(m.model, bl.BPR) and tuple(m.model.item_factors.shape) == (n, m.model.factors)
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
    assert list(table.index) == ["ColTrackCfBPR", "TrackTrackCfBPR"]
    assert np.isfinite(table.to_numpy(dtype=np.float64)).all()
    for name, m in models.items():
        w, nb = m.knn(torch.arange(n), 200)           # one batch against the three of save_knn
        sw, sn = d[name]
        assert tuple(nb.shape) == (n, 200) and torch.equal(sn, nb) and torch.equal(sw, w)
        assert table.loc[name, "hr (k=10)"] == bl.hit_rate(nb, tp, 10)
        assert table.loc[name, "t (train)"] == 2.0
