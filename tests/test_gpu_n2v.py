"""The kernels of csrc/n2v.hip (pinsage_n2v_walk, pinsage_sgns_dense,
pinsage_sgns_update) and what stands on them: baselines.Node2Vec and
FastNode2Vec.  The references are tests/n2v_util.py, checked on the host in
tests/test_n2v_host.py.

Walks are compared bit for bit with n2v_util.walk.  A walk is a prefix of the
longer walk from the same position, so one reference of 257 walks of 20 per
graph and (p, q) serves every n_walks and length.

Dense kernel.  The bound is test_gpu_lmf.py's with the column weight, u = 2^-24:
    ds <= gemm_bound(f, |x|.|y|)                          the score
    dp <= ds / 4 + 9 u p                                  sig' <= 1/4; exp, add, divide, and cw * p
    |dD[u, c]| <= gemm_bound(n_other, sum_i cw_i p |y_ic|) + sum_i cw_i dp_i |y_ic|

Update kernel.  New x is held against the float64 restatement by
als_util.row_errors under the project's rule: the device's error is at most
als_util.TOL_FACTOR (8) times the float32 restatement's on the same inputs.
It is one kernel with pinsage_lmf_update's: with unit weights and zero biases
the two write the same bits.

Fit.  The device objective after 30 iterations ends above its start and within
1e-4 relative of the float64 restatement run on the same counts and initial
tables; it is monotone wherever the restatement's is.
"""
import numpy as np
import pytest
import torch

import als_util as au
import lmf_util as lu
import n2v_util as nu
import parity_util as pu
from conftest import golden
from rowfit_util import PAD, SENT, _padded, _unpad

pytestmark = pytest.mark.gpu

ERR_ARG = -2
U = 2.0 ** -24
N_WALKS, LENGTH = 257, 20
P_Q = [(2.0, 0.5), (0.5, 2.0), (1.0, 1.0), (16.0, 1.0), (4.0, 0.25), (0.25, 4.0)]


# ----------------------------------------------------------------------------- graphs and walks
def _fixture_graph():
    import graph
    f = golden("jaccard")
    n, nc = int(f["n_tracks"]), int(f["n_cols"])
    edges = f["edges"].astype(np.int64)
    return n, nc, graph.CSRGraph(n + nc, edges[:, 0], edges[:, 1]), f["intersect_sizes"].astype(np.int64)


_GRAPHS = {}


def _graph(name):
    """(ptr, idx, cum or None, n) as numpy."""
    import baselines as bl
    if name not in _GRAPHS:
        if name == "edges":
            _GRAPHS[name] = nu.edge_graph()
        elif name == "planted":
            _GRAPHS[name] = nu.planted_graph(1)[0]
        else:
            n, _, g, _ = _fixture_graph()
            ids = list(range(n))
            ptr, idx, wt, m = bl.project_bipartite_graph(g, ids) if name == "projected" else bl.bipartite_graph(g, ids)
            ptr, idx = ptr.cpu().numpy(), idx.cpu().numpy()
            cum = None
            if wt is not None:
                cum = np.concatenate([np.cumsum(wt.cpu().numpy()[ptr[v]:ptr[v + 1]]) for v in range(m)]).astype(np.int64)
            _GRAPHS[name] = (ptr, idx, cum, m)
    return _GRAPHS[name]


def _starts(name):
    n = _graph(name)[3]
    return (np.arange(N_WALKS, dtype=np.int64) * 7 + (71 if name == "edges" else 0)) % n


_WALKS = {}


def _reference(name, p, q, seed=5, offset=2):
    key = (name, p, q, seed, offset)
    if key not in _WALKS:
        _WALKS[key] = nu.walk(_graph(name), _starts(name), LENGTH, 1 / p, 1 / q, seed, offset)
    return _WALKS[key]


def _walk(graph, starts, length, p, q, seed=5, offset=2, walk_base=0, inv=None, null=()):
    """pinsage_n2v_walk into a sentinel-filled buffer: (status, walks, error word, untouched)."""
    import _native as nat
    ptr, idx, cum, n = graph
    t = {"ptr": torch.from_numpy(ptr).cuda(), "idx": torch.from_numpy(idx).cuda(),
         "cum": None if cum is None else torch.from_numpy(cum).cuda(),
         "starts": torch.from_numpy(np.asarray(starts, np.int64)).cuda()}
    nw = len(starts)
    out = torch.full((nw * max(length, 0) + PAD,), -7, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    inv_p, inv_q = (1 / p, 1 / q) if inv is None else inv
    arg = lambda k: None if k in null else nat.ptr(t[k])  # noqa: E731
    rc = nat.lib().pinsage_n2v_walk(arg("ptr"), arg("idx"), arg("cum"), n, arg("starts"), nw, length, inv_p, inv_q,
                                    seed, offset, walk_base, None if "walks" in null else nat.ptr(out), nat.ptr(err),
                                    nat.stream_ptr())
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[nw * max(length, 0):] == -7).all(), "values behind the walks were written"
    return rc, h[:nw * max(length, 0)].reshape(nw, max(length, 0)), int(err), bool((h == -7).all())


@pytest.mark.parametrize("p,q", P_Q)
def test_walks_on_the_edge_graph_are_bit_exact(p, q):
    """Isolated start (node 71), leaves of degree 1, the hub's 70 edges, a row
    total above 2^32; every n_walks and length against one reference."""
    g, starts, want = _graph("edges"), _starts("edges"), _reference("edges", p, q)
    assert starts[0] == 71 and (want[starts == 71, 1:] == -1).all() and (want[starts != 71, 1] >= 0).all()
    assert (want == 0).any() and ((want >= 11) & (want <= 70)).any() and (want >= 72).any()
    for nw in (1, 63, 64, 65, 257):
        for length in (1, 2, 20):
            rc, got, err, _ = _walk(g, starts[:nw], length, p, q)
            assert rc == 0 and err == 0
            assert np.array_equal(got, want[:nw, :length]), (nw, length)


@pytest.mark.parametrize("name", ["projected", "bipartite", "planted"])
def test_walks_on_the_graphs_of_the_fit_are_bit_exact(name):
    g, starts = _graph(name), _starts(name)
    if name == "projected":
        n, _, _, inter = _fixture_graph()
        W = np.zeros((n, n), np.int64)
        ptr, idx, cum, _ = g
        for v in range(n):
            W[v, idx[ptr[v]:ptr[v + 1]]] = np.diff(cum[ptr[v]:ptr[v + 1]], prepend=0)
        np.fill_diagonal(inter, 0)
        assert np.array_equal(W, inter) and (np.diff(ptr) == 0).any()     # the reference's projection
    if name == "bipartite":
        n, nc, _, _ = _fixture_graph()
        ptr, idx, cum, m = g
        assert cum is None and m == n + nc and (idx[:ptr[n]] >= n).all() and (idx[ptr[n]:] < n).all()
        assert ptr[n] == ptr[-1] - ptr[n]
    for p, q in P_Q[:2]:
        want = _reference(name, p, q)
        rc, got, err, _ = _walk(g, starts, LENGTH, p, q)
        assert rc == 0 and err == 0 and np.array_equal(got, want), (name, p, q)


def test_walk_base_seed_and_offset():
    g, starts, want = _graph("edges"), _starts("edges"), _reference("edges", 2.0, 0.5)
    rc, part, err, _ = _walk(g, starts[100:180], LENGTH, 2.0, 0.5, walk_base=100)
    assert rc == 0 and np.array_equal(part, want[100:180])              # a slice is the same rows of the whole
    big = (1 << 40) + 3
    rc, got, _, _ = _walk(g, starts[:9], 5, 2.0, 0.5, seed=(1 << 63) + 9, offset=7, walk_base=big)
    assert rc == 0 and np.array_equal(got, nu.walk(g, starts[:9], 5, 0.5, 2.0, (1 << 63) + 9, 7, big))
    rc, other, _, _ = _walk(g, starts, LENGTH, 2.0, 0.5, seed=6)
    assert rc == 0 and not np.array_equal(other, want)


def test_walk_refusals_and_bad_ids():
    g, starts = _graph("edges"), _starts("edges")[:5]
    assert _walk(g, starts, 4, 2.0, 0.5)[::3] == (0, False)               # the accepted call writes
    assert _walk(g, starts[:0], 4, 2.0, 0.5)[::3] == (0, True)            # no walks: accepted, nothing launched
    inf, nan = float("inf"), float("nan")
    for inv in ((0.0, 1.0), (1.0, -1.0), (inf, 1.0), (1.0, nan), (17.0, 1.0), (4.1, 0.25), (1.0, 0.06)):
        assert _walk(g, starts, 4, None, None, inv=inv)[::3] == (ERR_ARG, True), inv
    assert _walk(g, starts, 0, 2.0, 0.5)[::3] == (ERR_ARG, True)
    assert _walk(g, starts, 4, 2.0, 0.5, walk_base=-1)[::3] == (ERR_ARG, True)
    import _native as nat
    buf = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros(1, dtype=torch.int64, device="cuda")
    pt, ix = torch.from_numpy(g[0]).cuda(), torch.from_numpy(g[1]).cuda()
    for n, nw, length in ((0, 1, 4), (1 << 31, 1, 4), (75, -1, 4), (75, 1 << 31, 4), (75, 1, 1 << 24)):
        rc = nat.lib().pinsage_n2v_walk(nat.ptr(pt), nat.ptr(ix), None, n, nat.ptr(st), nw, length, 0.5, 2.0, 1, 0, 0,
                                        nat.ptr(buf), None, nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and bool((buf == -7).all()), (n, nw, length)
    for null in ("ptr", "idx", "starts", "walks"):
        assert _walk(g, starts, 4, 2.0, 0.5, null=(null,))[::3] == (ERR_ARG, True), null
    # a bad start and a bad neighbour id set the error word and are clamped to node 0
    rc, got, err, _ = _walk(g, [75, -1, 3], 3, 2.0, 0.5)
    assert rc == 0 and err == 1 and (got[:2, 0] == 0).all() and got[2, 0] == 3
    idx = g[1].copy()
    idx[g[0][71 - 1]:g[0][71]] = 99                                       # leaf 70's only edge
    rc, got, err, _ = _walk((g[0], idx, g[2], g[3]), [70], 3, 2.0, 0.5)
    assert rc == 0 and err == 1 and got[0, 1] == 0 and (got >= 0).all() and (got < 75).all()


# ----------------------------------------------------------------------------- launch helpers
def _dense(X, Y, cw, pad_x=0, pad_y=0, pad_d=0):
    """pinsage_sgns_dense into a sentinel-filled output: (status, D [n, f])."""
    import _native as nat
    n, f = X.shape
    m = Y.shape[0]
    xd, yd = _padded(X, f + pad_x), _padded(Y, f + pad_y)
    dd = _padded(np.full((n, f), SENT, np.float32), f + pad_d, tail=True)
    cd = torch.from_numpy(np.asarray(cw, np.float32)).cuda()
    rc = nat.lib().pinsage_sgns_dense(nat.ptr(xd), n, f + pad_x, nat.ptr(yd), nat.ptr(cd), m, f + pad_y, f,
                                      nat.ptr(dd), f + pad_d, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, _unpad(dd, n, f, f + pad_d)


def _check_dense(X, Y, cw, what, **kw):
    rc, D = _dense(X, Y, cw, **kw)
    assert rc == 0 and np.isfinite(D).all()
    X64, Y64, c64 = (np.asarray(a, np.float64) for a in (X, Y, cw))
    f, m = X.shape[1], Y.shape[0]
    P = lu.sigmoid(X64 @ Y64.T)
    ds = pu.gemm_bound(f, np.abs(X64) @ np.abs(Y64).T)
    dp = ds / 4 + 9 * U * P
    bound = pu.gemm_bound(m, (P * c64) @ np.abs(Y64)) + (dp * c64) @ np.abs(Y64)
    err = np.abs(D - (P * c64) @ Y64)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: worst ratio to the bound {ratio:.3f}")
    assert ratio <= 1 and (err[bound == 0] == 0).all(), (what, ratio)
    return D


def _dense_case(n, m, f, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    cw = rng.uniform(0, 2, m).astype(np.float32)
    cw[rng.integers(0, m, max(1, m // 5))] = 0.0
    cw[rng.integers(0, m)] = 1e5
    return rng.normal(0, scale, (n, f)).astype(np.float32), rng.normal(0, scale, (m, f)).astype(np.float32), cw


# ----------------------------------------------------------------------------- the dense kernel
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("f", [4, 60, 64, 128])
def test_dense_factors_and_leading_dimensions(f, pad):
    X, Y, cw = _dense_case(37, 300, f, seed=f + pad)
    assert (cw == 0).any() and (cw == 1e5).any()
    _check_dense(X, Y, cw, f"f = {f}, every ld = f + {pad}", pad_x=pad, pad_y=pad, pad_d=pad)


@pytest.mark.parametrize("n_rows", [31, 33, 127, 129])
def test_dense_row_counts(n_rows):
    X, Y, cw = _dense_case(n_rows, 64, 16, seed=200 + n_rows)
    _check_dense(X, Y, cw, f"{n_rows} rows")


@pytest.mark.parametrize("n_other", [1, 31, 32, 33, 65])
def test_dense_item_counts(n_other):
    """A tile's tail items have to add zero."""
    for f in (8, 128):
        X, Y, cw = _dense_case(33, n_other, f, seed=300 + n_other + f)
        _check_dense(X, Y, cw, f"{n_other} items, f = {f}")


@pytest.mark.parametrize("f,n_rows,n_other", [(128, 130, 300), (60, 37, 70), (4, 33, 33)])
def test_dense_layout_is_exact_on_integer_data(f, n_rows, n_other):
    """X[u] = 200 e_c(u), Y in {-1, +1}, cw a power of two: cw sig is exactly 0 or
    cw, so D[u] = sum of cw_i y_i over the items with y_i[c(u)] = +1, exactly."""
    rng = np.random.default_rng(f)
    c = (7 * np.arange(n_rows) + 3) % f
    X = np.zeros((n_rows, f), np.float32)
    X[np.arange(n_rows), c] = 200.0
    Y = rng.choice([-1.0, 1.0], (n_other, f)).astype(np.float32)
    cw = (2.0 ** rng.integers(-3, 4, n_other)).astype(np.float32)
    rc, D = _dense(X, Y, cw, pad_y=4)
    assert rc == 0
    on = (Y[:, c] > 0).T.astype(np.float64) * cw[None, :]
    assert np.array_equal(D, (on @ Y).astype(np.float32))


def test_dense_bits_repeat_and_do_not_depend_on_the_batch():
    X, Y, cw = _dense_case(161, 333, 128, seed=500, scale=0.3)
    a, b = _dense(X, Y, cw), _dense(X, Y, cw)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    for u in (0, 37, 128, 160):
        _, D = _dense(X[u:u + 1], Y, cw)
        assert np.array_equal(D.view(np.uint32), a[1][u:u + 1].view(np.uint32)), u


def test_dense_refusals_leave_the_outputs_untouched():
    import _native as nat
    L = nat.lib()
    n, m, f = 5, 9, 8
    rng = np.random.default_rng(600)
    X = torch.from_numpy(au.init_factors(rng, n + 2, 16)).cuda().reshape(-1)
    Y = torch.from_numpy(au.init_factors(rng, m + 2, 16)).cuda().reshape(-1)
    cw = torch.ones(m, device="cuda")

    def dense(f=f, ldx=f, ldy=f, ldd=f, x_off=0, y_off=0, d_off=0, m=m, n=n, cw=cw):
        D = torch.full((n * 16 + PAD,), SENT, dtype=torch.float32, device="cuda")
        rc = L.pinsage_sgns_dense(nat.ptr(X[x_off:]), n, ldx, nat.ptr(Y[y_off:]), nat.ptr(cw), m, ldy, f,
                                  nat.ptr(D[d_off:]), ldd, nat.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((D == SENT).all())

    assert dense() == (0, False)
    assert dense(n=0) == (0, True)
    for kw in ({"f": 6}, {"f": 132, "ldx": 132, "ldy": 132, "ldd": 132}, {"f": 0}, {"ldx": 4}, {"ldy": 4},
               {"ldd": 4}, {"ldx": 10}, {"ldy": 10}, {"ldd": 10}, {"x_off": 1}, {"y_off": 1}, {"d_off": 1},
               {"m": 0}, {"cw": None}):
        assert dense(**kw) == (ERR_ARG, True), kw
        assert L.pinsage_last_error()


# ----------------------------------------------------------------------------- the update kernel
REG, LR = 0.3, 0.1
LENGTHS = [0, 1, 64, 512, 513, 2, 63, 65, 600]


def _update(csr, rw, X, H, Y, D, reg=REG, lr=LR, pad=0, forms=None):
    """pinsage_sgns_update: (status, X, H, error word)."""
    import _native as nat
    L = nat.lib()
    ptr, idx, val, n, m = csr
    f = X.shape[1]
    if forms is not None:
        got = {lu.row_form(int(ln), int(L.pinsage_lmf_long_row())) for ln in np.diff(ptr)}
        assert got == set(forms), (got, forms)
    xd, hd = _padded(X, f + pad, tail=True), _padded(H, f + pad, tail=True)
    yd, dd = _padded(Y, f + pad), _padded(D, f + pad)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ptr, idx, val, np.asarray(rw, np.float32))]
    rc = L.pinsage_sgns_update(nat.ptr(t[0]), nat.ptr(t[1]), nat.ptr(t[2]), nat.ptr(t[3]), n, nat.ptr(yd), m, f + pad,
                               nat.ptr(xd), f + pad, f, nat.ptr(dd), f + pad, nat.ptr(hd), f + pad, reg, lr,
                               nat.ptr(err), nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, _unpad(xd, n, f, f + pad), _unpad(hd, n, f, f + pad), int(err)


def _update_case(f, seed, lengths=LENGTHS, n_other=700):
    """Tables at a trained scale, the dense term from float64 rounded to fp32,
    accumulators uniform in [0.5, 2] (from zero a tiny gradient is divided by
    about 1e-3 and the ratio measures nothing)."""
    rng = np.random.default_rng(seed)
    csr = au.random_csr(rng, lengths, n_other, "counts")
    n = len(lengths)
    X, Y = au.init_factors(rng, n, f) * 8, au.init_factors(rng, n_other, f) * 8
    cw = (rng.uniform(0.5, 1.5, n_other) / n_other).astype(np.float32)
    rw = rng.uniform(1, 50, n).astype(np.float32)
    D = nu.dense_term(X, Y, cw, np.float64).astype(np.float32)
    H = rng.uniform(0.5, 2, (n, f)).astype(np.float32)
    return csr, rw, X, H, Y, D


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("f", [4, 64, 128])
def test_update_over_both_row_forms(f, pad):
    csr, rw, X, H, Y, D = case = _update_case(f, seed=f + pad)
    rc, xn, hn, err = _update(*case, pad=pad, forms=["wave", "workgroup"])
    assert rc == 0 and err == 0
    w64 = nu.half_iteration(*csr[:3], rw, X, H, Y, None, REG, LR, np.float64, D=D)[0]
    w32 = nu.half_iteration(*csr[:3], rw, X, H, Y, None, REG, LR, np.float32, D=D)[0]
    e32, edev = au.row_errors(w32, w64, X).max(), au.row_errors(xn, w64, X).max()
    print(f"f = {f}, pad {pad}: float32 restatement {e32:.3e}, device {edev:.3e}, ratio {edev / e32:.2f}")
    assert e32 > 0 and edev <= au.TOL_FACTOR * e32


def test_zero_learning_rate_and_the_empty_row():
    csr, rw, X, H, Y, D = case = _update_case(8, seed=40)
    rc, xn, hn, err = _update(*case, lr=0.0, pad=4)
    assert rc == 0 and err == 0 and np.array_equal(xn.view(np.uint32), X.view(np.uint32))
    moved = _update(*case, pad=4)
    assert np.array_equal(hn.view(np.uint32), moved[2].view(np.uint32)) and (hn >= H).all() and (hn > H).any()
    assert not np.array_equal(moved[1], X)
    # no items, rw = 0, reg = 0: g = 0 and x stays exactly, from zero accumulators too
    assert np.diff(csr[0])[0] == 0
    rw0 = rw.copy()
    rw0[0] = 0.0
    rc, xn, hn, err = _update(csr, rw0, X, np.zeros_like(H), Y, D, reg=0.0)
    assert rc == 0 and np.array_equal(xn[0].view(np.uint32), X[0].view(np.uint32)) and not hn[0].any()
    assert np.isfinite(xn).all() and not np.array_equal(xn[1], X[1])


def test_update_bits_repeat_and_bad_ids():
    csr, rw, X, H, Y, D = case = _update_case(128, seed=60)
    a, b = _update(*case), _update(*case)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    ptr, idx, val = csr[:3]
    for u in (3, 4, 8):                                      # a wave row, the long rows, alone in another grid
        one = au.csr_from_rows([(idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]])], 700)
        s = slice(u, u + 1)
        alone = _update(one, rw[s], X[s], H[s], Y, D[s])
        assert np.array_equal(alone[1].view(np.uint32), a[1][s].view(np.uint32)), u
    for bad in (700, -1, 2 ** 31 - 1):
        ix = idx.copy()
        ix[5] = bad
        got = _update((ptr, ix) + csr[2:], rw, X, H, Y, D)
        assert got[0] == 0 and got[3] == 1 and np.isfinite(got[1]).all()


def test_update_refusals_leave_the_outputs_untouched():
    import _native as nat
    L = nat.lib()
    n, m, f = 5, 9, 8
    rng = np.random.default_rng(80)
    csr = au.random_csr(rng, [2, 0, 3, 1, 4], m, "counts")
    ptr, idx, val = (torch.from_numpy(a).cuda() for a in csr[:3])
    Y = torch.from_numpy(au.init_factors(rng, m + 2, 16)).cuda().reshape(-1)
    D = torch.from_numpy(au.init_factors(rng, n + 2, 16)).cuda().reshape(-1)
    rw = torch.ones(n, device="cuda")

    def update(f=f, ldx=f, ldy=f, ldd=f, ldh=f, x_off=0, y_off=0, d_off=0, h_off=0, m=m, reg=REG, lr=LR, rw=rw,
               ptr=ptr):
        X, H = (torch.full((n * 16 + PAD,), SENT, dtype=torch.float32, device="cuda") for _ in range(2))
        rc = L.pinsage_sgns_update(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), nat.ptr(rw), n, nat.ptr(Y[y_off:]), m,
                                   ldy, nat.ptr(X[x_off:]), ldx, f, nat.ptr(D[d_off:]), ldd, nat.ptr(H[h_off:]), ldh,
                                   reg, lr, None, nat.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((X == SENT).all() and (H == SENT).all())

    assert update() == (0, False)
    for kw in ({"f": 6}, {"f": 132, "ldx": 132, "ldy": 132, "ldd": 132, "ldh": 132}, {"f": 0}, {"ldx": 4},
               {"ldy": 4}, {"ldd": 4}, {"ldh": 4}, {"ldx": 10}, {"ldh": 10}, {"x_off": 1}, {"y_off": 1}, {"d_off": 1},
               {"h_off": 1}, {"m": 0}, {"reg": -1.0}, {"reg": float("nan")}, {"lr": -1.0}, {"lr": float("inf")},
               {"rw": None}, {"ptr": None}):
        assert update(**kw) == (ERR_ARG, True), kw
        assert L.pinsage_last_error()


@pytest.mark.parametrize("f", [4, 60, 128])
def test_update_is_the_bias_form_without_biases(f):
    """What the one sig_update_kernel rests on: with alpha = 1 and zero bx, by and
    hb, pinsage_lmf_update leaves the X and H that pinsage_sgns_update leaves
    with rw = 1, bit for bit.  (s + 0) + 0 is s, 1 val is val and acc - d rounds
    as fmaf(-1, d, acc) does; dsum moves the biases only."""
    import _native as nat
    csr, _, X, H, Y, D = _update_case(f, seed=90 + f)
    ptr, idx, val, n, m = csr
    ld = f + 4
    rc, xw, hw, err = _update(csr, np.ones(n), X, H, Y, D, pad=4, forms=["wave", "workgroup"])
    assert rc == 0 and err == 0
    xd, hd = _padded(X, ld, tail=True), _padded(H, ld, tail=True)
    yd, dd = _padded(Y, ld), _padded(D, ld)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ptr, idx, val)]
    bx, by, hb = (torch.zeros(k, device="cuda") for k in (n, m, n))
    dsum = torch.from_numpy(np.random.default_rng(f).random(n).astype(np.float32)).cuda()
    errd = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = nat.lib().pinsage_lmf_update(nat.ptr(t[0]), nat.ptr(t[1]), nat.ptr(t[2]), n, nat.ptr(yd), nat.ptr(by), m, ld,
                                      nat.ptr(xd), nat.ptr(bx), ld, f, nat.ptr(dd), ld, nat.ptr(dsum), nat.ptr(hd), ld,
                                      nat.ptr(hb), 1.0, REG, LR, nat.ptr(errd), nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and int(errd) == 0
    xb, hn = _unpad(xd, n, f, ld), _unpad(hd, n, f, ld)
    assert not np.array_equal(xb, X) and np.isfinite(xb).all()
    assert torch.equal(torch.from_numpy(xb), torch.from_numpy(xw)), np.argwhere(xb != xw)[:1]
    assert torch.equal(torch.from_numpy(hn), torch.from_numpy(hw)), np.argwhere(hn != hw)[:1]


# ----------------------------------------------------------------------------- Node2Vec.fit
def _fit_graph(name):
    ptr, idx, cum, n = _graph(name)
    wt = None if cum is None else nu.weights_of((ptr, idx, cum, n))
    return (torch.from_numpy(ptr), torch.from_numpy(idx), None if wt is None else torch.from_numpy(wt), n)


@pytest.mark.parametrize("name", ["planted", "projected"])
def test_fit_against_the_float64_restatement(name):
    import baselines as bl
    f = 16
    n = _graph(name)[3]
    rng = np.random.default_rng(f)
    U0, V0 = au.init_factors(rng, n, f), au.init_factors(rng, n, f)
    seen = []
    m = bl.Node2Vec(dim=f, random_state=3).fit(_fit_graph(name), callback=lambda it, mod: seen.append(mod.objective()),
                                               embedding=torch.from_numpy(U0), context_factors=torch.from_numpy(V0))
    # the walks are the restatement's, the counts the triple loop's
    starts = np.tile(np.arange(n), 10)
    assert tuple(m.walks.shape) == (10 * n, 20) and m.walks.dtype == torch.int32
    some = np.r_[0:3, n:n + 3, 9 * n + n - 2:10 * n]
    want_walks = np.stack([nu.walk(_graph(name), [starts[k]], 20, 0.5, 2.0, 3, 0, int(k))[0] for k in some])
    assert np.array_equal(m.walks.cpu().numpy()[some], want_walks)
    C = tuple(a.cpu().numpy() for a in m.cooccurrence[:3]) + (n, n)
    Cd = nu.dense_of(C)
    assert np.array_equal(Cd, Cd.T) and Cd.sum() > 0
    cnt, P = nu.noise(C)
    assert np.array_equal(m.noise.cpu().numpy(), P)
    start = nu.objective(C, U0, V0, 5.0, P, 0.0)
    _, _, want = nu.fit(C, U0, V0, cnt, P, 5.0, 0.0, 0.1, 30, np.float64, trace=True)
    got = m.objective()
    print(f"{name}: L {start:.6g} -> {got:.6g}, float64 {want[-1]:.6g}, relative {abs(got - want[-1]) / abs(want[-1]):.2e}")
    print("device ", " ".join(f"{v:.6g}" for v in seen))
    print("float64", " ".join(f"{v:.6g}" for v in want))
    assert len(seen) == 30 and seen[-1] == got and got > start
    assert abs(got - want[-1]) <= 1e-4 * abs(want[-1])
    rises = np.diff([start] + want) > 0
    assert (np.diff([start] + seen) > 0)[rises].all()
    for tab in (m.embedding, m.context_factors):
        assert tab.is_cuda and tab.dtype == torch.float32 and tuple(tab.shape) == (n, f)
    if name == "planted":
        groups = nu.planted_graph(1)[1]
        connected = np.flatnonzero(np.diff(_graph(name)[0]) > 0)
        share = nu.same_group_share(m.embedding.cpu().numpy(), groups, connected)
        U64 = nu.fit(C, U0, V0, cnt, P, 5.0, 0.0, 0.1, 30, np.float64)[0]
        print(f"top-10 same-group share: device {share:.3f}, float64 {nu.same_group_share(U64, groups, connected):.3f}")
        assert len(connected) < n and share >= 0.5


def test_random_state_and_the_global_generator():
    import baselines as bl
    g = _fit_graph("planted")
    n = g[3]
    a = bl.Node2Vec(dim=8, iterations=2, random_state=7).fit(g)
    b = bl.Node2Vec(dim=8, iterations=2, random_state=7).fit(g)
    assert torch.equal(a.walks, b.walks) and torch.equal(a.embedding, b.embedding)
    assert torch.equal(a.context_factors, b.context_factors)
    c = bl.Node2Vec(dim=8, iterations=2, random_state=8).fit(g)
    assert not torch.equal(a.walks, c.walks) and not torch.equal(a.embedding, c.embedding)
    gen = torch.Generator().manual_seed(7)
    m = bl.Node2Vec(dim=8, iterations=0, random_state=7).fit(g)
    assert torch.equal(m.embedding.cpu(), (torch.rand(n, 8, generator=gen) - 0.5) / 8)
    assert torch.equal(m.context_factors.cpu(), (torch.rand(n, 8, generator=gen) - 0.5) / 8)
    # None: one randint for the Philox seed, then the two tables, from the global generator
    torch.manual_seed(3)
    m = bl.Node2Vec(dim=8, iterations=1).fit(g)
    after = torch.rand(1)
    torch.manual_seed(3)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))
    u0, v0 = (torch.rand(n, 8) - 0.5) / 8, (torch.rand(n, 8) - 0.5) / 8
    assert torch.equal(after, torch.rand(1))
    want = bl.Node2Vec(dim=8, iterations=1, random_state=seed).fit(g, embedding=u0, context_factors=v0)
    assert torch.equal(m.walks, want.walks) and torch.equal(m.embedding, want.embedding)
    with pytest.raises(ValueError):
        bl.Node2Vec(dim=8).fit((g[0][:-1],) + g[1:])
    with pytest.raises(IndexError):
        bl.Node2Vec(dim=8).fit((g[0], g[1] + n, g[2], n))
    with pytest.raises(ValueError):
        bl.Node2Vec(dim=8).fit((g[0], g[1], g[2] * 0, n))


# ----------------------------------------------------------------------------- FastNode2Vec
@pytest.fixture(scope="module")
def fast():
    import baselines as bl
    n, _, g, _ = _fixture_graph()
    ids = list(range(n))
    torch.manual_seed(1)
    models = {"node2vec": bl.FastNode2Vec(), "node2vec-bipartite": bl.FastNode2Vec(projected=False)}
    for m in models.values():
        m.train(g, ids, None, None, None)
    return n, g, ids, models


def test_fast_node2vec_knn_is_knn_from_emb(fast):
    import baselines as bl
    n, _, _, models = fast
    for name, m in models.items():
        assert isinstance(m.model, bl.Node2Vec) and m.model.factors == 128 and m.model.walks_per_node == 10
        assert tuple(m.embedding.shape) == (n, 128) and bool(torch.isfinite(m.embedding).all())
        assert int(m.model.embedding.shape[0]) == (n if m.projected else len(fast[1]))
        for nodeset in (torch.arange(n), torch.tensor([5, 5, 299, 0]), torch.tensor([7, 3]).cuda()):
            w, nb = m.knn(nodeset, 10)
            want_w, want_n = bl.knn_from_emb(m.embedding, nodeset, 10)
            assert tuple(w.shape) == tuple(nb.shape) == (len(nodeset), 10)
            assert w.dtype == torch.float32 and nb.dtype == torch.int64
            assert torch.equal(w.cpu(), want_w.cpu()) and torch.equal(nb.cpu(), want_n.cpu()), name
            assert torch.equal(m.embed(nodeset), m.embedding[nodeset.cpu(), :])


def test_tables_end_to_end(fast, tmp_path, monkeypatch):
    import baselines as bl
    n, g, ids, models = fast
    rng = np.random.default_rng(95)
    tp = torch.from_numpy(rng.integers(0, n, (400, 2)))
    monkeypatch.setattr(bl, "PRECOMP_K", 200)         # 300 tracks: lists of 1000 do not exist
    for name, m in models.items():
        bl.save_knn(m, name, ids, str(tmp_path), train_time=2.0, b_size=128)
    d = bl.LazyKnnDict(list(models), ids, str(tmp_path))
    table = bl.compute_results_table(d, tp, g)
    assert list(table.index) == list(models) and np.isfinite(table.to_numpy(dtype=np.float64)).all()
    feats = torch.from_numpy(rng.standard_normal((n, 12)).astype(np.float32))
    np.random.seed(11)
    beyond = bl.compute_beyond_accuracy_table({name: d[name] for name in models}, tp, g, feats)
    assert list(beyond.index) == list(table.index) and np.isfinite(beyond.to_numpy(dtype=np.float64)).all()
