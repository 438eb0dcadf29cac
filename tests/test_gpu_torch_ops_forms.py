"""torch.ops.pinsage in every form its schemas allow (csrc/torch_ops.cpp) and every
branch of the registered autograd formulas (pinsage_ops.py), against the float64
references of tests/ops_util.py (checked on the CPU by tests/test_ops_host.py).

Conventions.  The ops return fresh tensors: shape, dtype, device and isfinite
are asserted before the values.  Wherever only sums of products are involved a
case runs twice: with exact-sum integers (magnitude <= 8, weights k / 8), where
the result must equal float64 bit for bit whatever the tile or arithmetic, and
with wide-range row-scaled Gaussians held element by element to the derived
bound.  Behind LeakyReLU's 0.01f or the row norm only the bound applies.
Operand views keep a 16-byte aligned data pointer and a row stride that is a
multiple of 4 floats (segment_wmean's scalar case apart, which its launcher
tests for); a 4-byte-offset view such as x[:, 1:] is not tested.  Rejection
cases are views into allocations large enough for the sizes they declare: a
missing check shows as "did not raise".  The largest error / bound per op is
printed (pytest -s) and recorded in DESIGN.md.
"""
import numpy as np
import pytest
import torch

import ops_util as ou
import parity_util as pu
import sampler_util as su
from ops_util import note

pytestmark = pytest.mark.gpu
MODES = ("random", "exact")


@pytest.fixture(scope="module")
def ops():
    import pinsage_ops
    pinsage_ops.load()
    return torch.ops.pinsage


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def place(a, how="plain"):
    """a on the device: 'plain' contiguous; 'rows' a row slice big[3:]; 'cols' a
    column view big[:, 4:4 + width]; 'wide' a view big[:, :width] of wider rows"""
    r, c = a.shape
    t = dev(a)
    if how == "plain":
        return t
    if how == "rows":
        big = torch.full((r + 3, c), 7.0, device="cuda")
        v = big[3:]
    elif how == "cols":
        big = torch.full((r, c + 8), 7.0, device="cuda")
        v = big[:, 4:4 + c]
    else:
        big = torch.full((r, c + 4), 7.0, device="cuda")
        v = big[:, :c]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0 and v.stride(1) == 1
    return v


def fresh(t, shape, dtype=torch.float32):
    assert tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape))
    assert t.dtype == dtype and t.is_cuda
    if t.is_floating_point():
        assert bool(torch.isfinite(t).all())
    return t.detach().cpu().numpy()


def host(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- linear
def run_linear(ops, c, lrelu, how, exact, needs=("x", "W", "b"), tag="linear"):
    x = place(c["x"], how).requires_grad_("x" in needs)
    W = dev(c["W"]).requires_grad_("W" in needs)
    b = dev(c["b"])
    if b is not None:
        b.requires_grad_("b" in needs)
    rows = dev(c["rows"])
    y = ops.linear(x, rows, W, b, lrelu)
    ref = ou.linear_reference(c["x"], c["rows"], c["W"], c["b"], lrelu, c["dy"], exact)
    M = c["dy"].shape[0]
    note(f"{tag} y", ou.check("y", fresh(y, (M, c["W"].shape[0])), *ref["y"], exact))
    if not (x.requires_grad or W.requires_grad or (b is not None and b.requires_grad)):
        return y, ref
    (y * dev(c["dy"])).sum().backward()
    tight = exact and not lrelu
    for k, t in (("dx", x), ("dW", W), ("db", b)):
        if t is None:
            continue
        if k[1:] not in needs:
            assert t.grad is None, k
            continue
        note(f"{tag} {k}", ou.check(k, fresh(t.grad, t.shape), *ref[k], tight))
    return y, ref


@pytest.mark.parametrize("lrelu", (False, True))
@pytest.mark.parametrize("with_b", (False, True))
@pytest.mark.parametrize("with_rows", (False, True))
def test_linear_forms(ops, with_rows, with_b, lrelu):
    """{rows None, int32 rows with repeats} x {b None, b} x {lrelu off, on} at
    every shape, x wider than K, as a row slice and as a column view: the
    forward and the x, W, b gradients; x's columns >= K and its unselected rows
    get exactly 0 (the reference's bound there is 0)."""
    cell = 4 * with_rows + 2 * with_b + lrelu
    hows = ("plain", "rows", "cols")
    for i, shape in enumerate(ou.LINEAR_SHAPES):
        for mode in MODES:
            exact = mode == "exact"
            c = ou.linear_inputs(shape, with_rows, with_b, exact, 1000 * cell + i)
            for how in (hows if i == 1 else (hows[(i + cell) % 3],)):
                run_linear(ops, c, lrelu, how, exact)
        xr, ld, K, N, n = shape
        if ld > K or with_rows:
            ref = ou.linear_reference(c["x"], c["rows"], c["W"], c["b"], lrelu, c["dy"], True)
            dx, E = ref["dx"]
            dead = np.ones(dx.shape, bool)
            dead[ou._idx(c["rows"], xr), :K] = False
            assert dead.any() and (dx[dead] == 0).all() and (E[dead] == 0).all()


@pytest.mark.parametrize("needs", (("x",), ("W",), ("b",), ()))
def test_linear_requires_grad_subsets(ops, needs):
    for with_rows in (False, True):
        for lrelu in (False, True):
            c = ou.linear_inputs(ou.LINEAR_SHAPES[4], with_rows, True, False, 77)
            run_linear(ops, c, lrelu, "cols", False, needs)
    c = ou.linear_inputs(ou.LINEAR_SHAPES[3], True, False, True, 78)       # b None: db's slot stays None
    run_linear(ops, c, False, "plain", True, needs)


@pytest.mark.parametrize("with_b", (False, True))
@pytest.mark.parametrize("with_rows", (False, True))
def test_linear_zero_preactivation_takes_the_slope(ops, with_rows, with_b):
    """integer inputs whose pre-activation is exactly 0: y is 0 there (bit for
    bit, as all of y) and the gradients take lrelu'(0) = 0.01 as lrelu_grad64
    does -- the other branch is 100 times the bound away."""
    for i, shape in enumerate(ou.LINEAR_SHAPES[:5]):
        c = ou.linear_inputs(shape, with_rows, with_b, True, 500 + i, zeros=True)
        y, ref = run_linear(ops, c, True, "plain", True, tag="linear y==0")
        zero = ref["y"][0] == 0
        assert zero[0, :2].all() and (host(y)[zero] == 0).all()
        assert (pu.lrelu_grad64(ref["y"][0][zero]) == pu.SLOPE).all()


def test_linear_in_features_not_a_multiple_of_4_is_refused(ops):
    x = torch.zeros(8, 8, device="cuda")
    W = torch.zeros(4, 6, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.linear(x, None, W, None, False)


# ----------------------------------------------------------------------------- concat_linear_lrelu_l2norm
def run_concat(ops, c, shape, needs=("h", "agg", "W", "b")):
    d, hid, out, n = shape
    h = dev(c["h"]).requires_grad_("h" in needs)
    agg = place(c["agg"], "wide").requires_grad_("agg" in needs)
    assert agg.stride(0) > hid
    W = dev(c["W"]).requires_grad_("W" in needs)
    b = dev(c["b"]).requires_grad_("b" in needs)
    y, nrm = ops.concat_linear_lrelu_l2norm(h, dev(c["rows"]), agg, W, b)
    ref = ou.concat_reference(c["h"], c["rows"], c["agg"], c["W"], c["b"], c["dy"])
    note("concat y", ou.check("y", fresh(y, (n, out)), *ref["y"]))
    note("concat norms", ou.check("norms", fresh(nrm, (n,)), *ref["norms"]))
    assert not nrm.requires_grad                       # norms is marked non-differentiable
    assert (host(y)[:, 1] == 0).all()                  # exact zeros in every row of y
    if not needs:
        assert not y.requires_grad
        return
    (y * dev(c["dy"])).sum().backward()
    for k, t in (("h", h), ("agg", agg), ("W", W), ("b", b)):
        if k not in needs:
            assert t.grad is None, k
            continue
        note(f"concat d{k}", ou.check("d" + k, fresh(t.grad, t.shape), *ref["d" + k]))


@pytest.mark.parametrize("with_rows", (False, True))
@pytest.mark.parametrize("shape", ou.CONCAT_SHAPES)
def test_concat_linear_lrelu_l2norm_forms(ops, shape, with_rows):
    """self_rows None and int64 with repeats, h wider than d, agg a row view
    with stride(0) > hid, out = 6 (the padded backward) and out = 200 (the GEMM
    plus l2norm_rows path): y, norms and every gradient, and each
    requires_grad subset; dh is exactly 0 outside the selected rows' first d
    columns."""
    c = ou.concat_inputs(shape, with_rows, 40 + shape[2])
    run_concat(ops, c, shape)
    for needs in (("h",), ("agg",), ("W",), ("b",), ()):
        run_concat(ops, c, shape, needs)


# ----------------------------------------------------------------------------- gemm
@pytest.mark.parametrize("mode", MODES)
def test_gemm_layouts_and_gathers(ops, mode):
    """the four operand layouts x {no gather, a_idx, b_idx on an N-major B} at
    every shape launch_gemm allows there, operands as views with stride(0) >
    width, and K = 1032 gathered k-rows (two index windows)"""
    exact = mode == "exact"
    for i, case in enumerate(ou.gemm_cases()):
        ak, bk, gather, M, N, K = case
        c = ou.gemm_inputs(case, exact, 2000 + i)
        A = place(c["A"], "plain")[:, :c["A"].shape[1] - 4]
        B = place(c["B"], "plain")[:, :c["B"].shape[1] - 4]
        assert A.stride(0) > A.shape[1] and B.stride(0) > B.shape[1]
        C = ops.gemm(A, ak, dev(c["a_idx"]), B, bk, dev(c["b_idx"]), M, N, K)
        want, bound = ou.gemm_reference(c["A"], ak, c["a_idx"], c["B"], bk, c["b_idx"], M, N, K, exact)
        name = f"gemm {'K' if ak else 'M'}-major A, {'K' if bk else 'N'}-major B"
        note(name, ou.check(f"C of {case}", fresh(C, (M, N)), want, bound, exact))


def test_gemm_empty_sizes_and_refused_sizes(ops):
    A = torch.ones(8, 8, device="cuda")
    for ak in (True, False):
        for bk in (True, False):
            assert fresh(ops.gemm(A, ak, None, A, bk, None, 0, 8, 8), (0, 8)).size == 0
            C = fresh(ops.gemm(A, ak, None, A, bk, None, 8, 4, 0), (8, 4))
            assert (C == 0).all()
    big = torch.ones(136, 136, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 4"):   # an M-major A's M
        ops.gemm(big, False, None, big, True, None, 130, 72, 40)
    with pytest.raises(RuntimeError, match="N % 4"):            # an N-major B's N
        ops.gemm(big, True, None, big, False, None, 4, 6, 8)
    with pytest.raises(RuntimeError, match="multiple of 4"):   # K
        ops.gemm(big, True, None, big, True, None, 4, 4, 6)


# ----------------------------------------------------------------------------- weighted_agg
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ou.AGG_SHAPES)
def test_weighted_agg_forms(ops, shape, mode):
    """hid with a partial last column chunk (4, 260, 516), more than 64 slots
    per row (T = 65, 130: the second pass of agg_kernel's slot loop), one row
    whose slots all name one q row, one q row no slot names (its gradient is
    exactly 0); dq through autograd and through the op."""
    hid, T, n, n_q = shape
    exact = mode == "exact"
    c = ou.agg_inputs(shape, exact, 300 + T)
    q = dev(c["q"]).requires_grad_()
    loc, w = dev(c["loc"]), dev(c["w"])
    agg = ops.weighted_agg(q, loc, w)
    r = ou.check_agg("agg", fresh(agg, (n, hid)), ou.weighted_agg_reference(c["q"], c["loc"], c["w"]), exact)
    if not exact:
        note("weighted_agg (of 1e-6 row-relative)", r)
    (agg * dev(c["dagg"])).sum().backward()
    want, bound = ou.agg_dq_reference(c["dagg"], c["loc"], c["w"], n_q, exact)
    note("weighted_agg dq", ou.check("dq", fresh(q.grad, (n_q, hid)), want, bound, exact))
    direct = ops.weighted_agg_backward(place(c["dagg"], "wide"), loc, w, n_q)
    ou.check("dq (op)", fresh(direct, (n_q, hid)), want, bound, exact)
    assert torch.equal(direct, q.grad)
    if c["unnamed"] is not None:
        assert (host(q.grad)[c["unnamed"]] == 0).all()


def test_weighted_agg_no_rows(ops):
    q = torch.randn(9, 48, device="cuda")
    loc = torch.zeros(0, 7, dtype=torch.int32, device="cuda")
    w = torch.zeros(0, 7, device="cuda")
    assert fresh(ops.weighted_agg(q, loc, w), (0, 48)).size == 0
    dq = fresh(ops.weighted_agg_backward(torch.zeros(0, 48, device="cuda"), loc, w, 9), (9, 48))
    assert (dq == 0).all()


# ----------------------------------------------------------------------------- segment_wmean
@pytest.mark.parametrize("d", ou.SEG_WIDTHS)
def test_segment_wmean_forms(ops, d):
    """segment lengths 0, 1, 3, 4, 5, 8, 9, 65, 130 in one call, normalize off
    and on, the float4 kernel and the scalar one (d = 30, and h as a view whose
    row stride is no multiple of 4), columns -1 and n_h skipped in the sum and
    in the normalisation."""
    for mode in MODES:
        exact = mode == "exact"
        c = ou.segment_inputs(d, exact, 600 + d)
        seg, cols, w = dev(c["seg"]), dev(c["cols"]), dev(c["w"])
        big = torch.full((ou.SEG_ROWS, d + 3), 7.0, device="cuda")
        odd = big[:, :d]
        odd.copy_(dev(c["h"]))
        assert odd.stride(0) % 4 != 0
        for normalize in (False, True):
            want, bound = ou.segment_wmean_reference(c["h"], c["seg"], c["cols"], c["w"], normalize, exact)
            for name, h in (("float4", dev(c["h"])), ("scalar", odd)):
                out = ops.segment_wmean(h, seg, cols, w, normalize)
                tight = exact and not normalize
                note(f"segment_wmean normalize={int(normalize)}",
                     ou.check(f"out ({name}, normalize {normalize})", fresh(out, (len(ou.SEG_LENGTHS), d)), want, bound,
                              tight))
                assert (host(out)[0] == 0).all() and (host(out)[-1] == 0).all()


def test_segment_wmean_all_empty(ops):
    h = torch.randn(5, 8, device="cuda")
    none_i = torch.zeros(0, dtype=torch.int32, device="cuda")
    none_f = torch.zeros(0, device="cuda")
    for normalize in (False, True):
        out = ops.segment_wmean(h, torch.zeros(4, dtype=torch.int64, device="cuda"), none_i, none_f, normalize)
        assert (fresh(out, (3, 8)) == 0).all()
        out = ops.segment_wmean(h, torch.zeros(1, dtype=torch.int64, device="cuda"), none_i, none_f, normalize)
        assert fresh(out, (0, 8)).size == 0


# ----------------------------------------------------------------------------- gather_rows / scatter_add_rows
@pytest.mark.parametrize("mode", MODES)
def test_gather_and_scatter_rows_forms(ops, mode):
    """n = 0; an idx that repeats one row 70 times (the sum runs in position
    order: exact in exact mode); width < d and width > d; each op the other's
    gradient."""
    exact = mode == "exact"
    rng = np.random.default_rng(8)
    for n_h, d, wg, ws, n in ((40, 12, 8, 20, 90), (9, 260, -1, 264, 75), (6, 4, 4, -1, 0)):
        h = ou.values(rng, (n_h, d), exact)
        idx = rng.integers(0, n_h, n)
        idx[:70] = 3
        idx = rng.permutation(idx)
        hd = place(h, "wide").requires_grad_()
        rows = ops.gather_rows(hd, dev(idx), wg)
        cw = d if wg < 0 else wg
        assert pu.bits32(fresh(rows, (n, cw))).tolist() == pu.bits32(ou.gather_reference(h, idx, wg)).tolist()
        cot = ou.values(rng, (n, cw), exact, wide=False)
        (rows * dev(cot)).sum().backward()
        want, bound = ou.scatter_add_reference(cot, idx, n_h, d, exact)
        note("gather_rows backward", ou.check("dh", fresh(hd.grad, (n_h, d)), want, bound, exact))
        g = ou.values(rng, (n, d), exact, wide=False)
        gd = dev(g).requires_grad_()
        sw = d if ws < 0 else ws
        s = ops.scatter_add_rows(gd, dev(idx), n_h, ws)
        want, bound = ou.scatter_add_reference(g, idx, n_h, ws, exact)
        note("scatter_add_rows", ou.check("out", fresh(s, (n_h, sw)), want, bound, exact))
        cot = ou.values(rng, (n_h, sw), exact)
        (s * dev(cot)).sum().backward()
        assert pu.bits32(fresh(gd.grad, (n, d))).tolist() == pu.bits32(cot[idx][:, :d]).tolist()


# ----------------------------------------------------------------------------- norm_lrelu_backward
@pytest.mark.parametrize("n", (1, 37))
@pytest.mark.parametrize("out", (4, 63, 65, 200))
def test_norm_lrelu_backward_op(ops, out, n):
    rng = np.random.default_rng(out + n)
    v = rng.standard_normal((n, out))
    v[rng.random(v.shape) < 0.2] = 0.0
    v[:, 0] = 1.0
    nrm = np.linalg.norm(v, axis=1).astype(np.float32)
    y = (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)
    assert (y == 0).any() or out == 4
    dy = pu.wide_rows(rng, (n, out))
    want, bound = pu.norm_lrelu_bwd_reference(y, nrm, dy)
    for d_dy in (dev(dy), dev(dy.T).t()):              # contiguous, and a transposed (non-contiguous) dy
        assert d_dy.shape == (n, out)
        dp = ops.norm_lrelu_backward(d_dy, dev(y), dev(nrm))
        note("norm_lrelu_backward", ou.check("dp", fresh(dp, (n, out)), want, bound))


# ----------------------------------------------------------------------------- ppr_topk, long walks
def test_ppr_topk_long_walks_match_the_oracle(ops):
    """n_hops = 8200 > 8192: the walk + visit_topk_kernel route with more than
    64 KB of dynamic LDS (launch_visit_topk's hipFuncSetAttribute branch), on
    the 600-node graph where k * 64 > n_all (the nth_element regime); bit for
    bit the CPU oracle.  (The partial_sort heap replay at this LDS size stays
    unexercised: it needs n_all >= 640.)"""
    indptr, indices, n_all, special = su.bipartite_graph()
    n_hops, k, alpha, seed = 8200, 10, 0.85, 0x5eed_1234
    assert k * 64 > n_all and 2 * 16384 * 4 > 64 * 1024
    src = np.array([special["hub"], special["loner"], 57], np.int64)
    traces = su.oracle_traces(indptr, indices, src, n_hops, np.float32(alpha), seed=seed, offset=2, src_base=5)
    rw, rnb, _, _ = su.topk_reference(su.oracle_runs(traces, src), n_all, n_hops, k)
    ip, ix = dev(indptr), dev(indices)
    w, nb = ops.ppr_topk(ip, ix, dev(src), n_hops, alpha, k, seed, 5, 2, "philox")
    su.check_exact("w", fresh(w, (3, k), torch.float64), rw)
    su.check_exact("nb", fresh(nb, (3, k), torch.int64), rnb)
    w, nb = ops.ppr_topk(ip, ix, dev(src[:0]), n_hops, alpha, k, seed, 5, 2, "philox")
    assert fresh(w, (0, k), torch.float64).size == 0 and fresh(nb, (0, k), torch.int64).size == 0


# ----------------------------------------------------------------------------- rejections
def test_rejections_raise_before_any_launch(ops):
    """Every operand is a view into an allocation that covers the sizes the call
    declares, so a missing check would show as "did not raise", never as an
    out-of-bounds access."""
    f = torch.zeros(64, 64, device="cuda")
    i32 = torch.zeros(256, dtype=torch.int32, device="cuda")
    i64 = torch.zeros(256, dtype=torch.int64, device="cuda")
    flat = torch.zeros(4096, device="cuda")
    W = torch.zeros(8, 16, device="cuda")
    R = RuntimeError
    # dtypes and contiguity
    with pytest.raises(R, match="dtype"):
        ops.linear(f, None, W.double(), None, False)
    with pytest.raises(R, match="dtype"):
        ops.linear(f, i64[:4], W, None, False)
    with pytest.raises(R, match="f32"):
        ops.linear(f.double(), None, W, None, False)
    with pytest.raises(R, match="contiguous"):
        ops.linear(f, None, f[:8, :16], None, False)
    with pytest.raises(R, match="contiguous"):
        ops.concat_linear_lrelu_l2norm(f, None, f[:4, :8], f[:8, :16], flat[:8])
    # shapes: linear
    with pytest.raises(R, match=r"b: \[out_features\]"):
        ops.linear(f, None, W, flat[:6], False)
    with pytest.raises(R, match="x: f32 device rows"):
        ops.linear(flat[:64], None, W, None, False)
    with pytest.raises(R, match="W:"):
        ops.linear(f, None, flat[:128], None, False)
    with pytest.raises(R, match="narrower"):
        ops.linear(f[:, :8], None, W, None, False)
    # gemm against its operands' shapes and its index lengths, under each layout
    A = f[:8, :16]
    for args, what in (((A, True, None, f, True, None, 16, 8, 16), "A has 8 rows"),
                       ((A, True, None, f, True, None, 8, 8, 32), "A has 16 columns"),
                       ((A, False, None, f, True, None, 16, 8, 16), "A has 8 rows"),
                       ((A, False, None, f, True, None, 32, 8, 8), "A has 16 columns"),
                       ((f, True, None, A, True, None, 8, 16, 16), "B has 8 rows"),
                       ((f, True, None, A, True, None, 8, 8, 32), "B has 16 columns"),
                       ((f, True, None, A, False, None, 8, 16, 16), "B has 8 rows"),
                       ((f, True, None, A, False, None, 8, 32, 8), "B has 16 columns"),
                       ((f, True, i32[:8], f, True, None, 16, 8, 16), "a_idx has 8 rows"),
                       ((f, False, i32[:8], f, True, None, 8, 8, 16), "a_idx has 8 rows"),
                       ((f, True, None, f, False, i32[:8], 8, 8, 16), "b_idx has 8 rows"),
                       ((f, True, None, f, True, i32[:16], 8, 8, 16), "b_idx gathers"),
                       ((f, True, i64[:8], f, True, None, 8, 8, 16), "dtype"),
                       ((flat[:64], True, None, f, True, None, 8, 8, 8), "2-D"),
                       ((f, True, None, f, True, None, 8, 0, 8), "N >= 1"),
                       ((f, True, None, f, True, None, -4, 8, 8), "M, K >= 0")):
        with pytest.raises(R, match=what):
            ops.gemm(*args)
    # weighted_agg / weighted_agg_backward
    loc = i32[:40].view(8, 5)
    w_short = flat[:32].view(8, 4)
    w_ok = flat[:40].view(8, 5)
    with pytest.raises(R, match="loc and w"):
        ops.weighted_agg(f, loc, w_short)
    with pytest.raises(R, match="q:"):
        ops.weighted_agg(flat[:4096].view(8, 8, 64), loc, w_ok)
    with pytest.raises(R, match="dtype"):
        ops.weighted_agg(f, i64[:40].view(8, 5), w_ok)
    for dagg in (f[:7], f[:8].double(), flat[:512]):
        with pytest.raises(R, match="dagg"):
            ops.weighted_agg_backward(dagg, loc, w_ok, 4)
    with pytest.raises(R, match="loc and w"):
        ops.weighted_agg_backward(f[:8], loc, w_short, 4)
    # segment_wmean
    seg = i64[:5]
    with pytest.raises(R, match="cols and w"):
        ops.segment_wmean(f, seg, i32[:10], flat[:7], False)
    with pytest.raises(R, match="seg"):
        ops.segment_wmean(f, i64[:0], i32[:10], flat[:10], True)
    with pytest.raises(R, match="h: f32"):
        ops.segment_wmean(flat[:64], seg, i32[:10], flat[:10], False)
    # gather / scatter widths and the three index range checks
    with pytest.raises(R, match="width exceeds"):
        ops.gather_rows(f, i64[:4], 65)
    with pytest.raises(R, match="narrower"):
        ops.scatter_add_rows(f[:4], i64[:4], 8, 63)
    with pytest.raises(R, match="rows differ"):
        ops.scatter_add_rows(f[:4], i64[:5], 8, 64)
    bad = torch.tensor([0, 64, 1, 2], device="cuda")
    neg = torch.tensor([0, -1, 1, 2], device="cuda")
    for ix in (bad, neg):
        with pytest.raises(IndexError):
            ops.gather_rows(f, ix, 8)
        with pytest.raises(IndexError):
            ops.scatter_add_rows(f[:4], ix, 64, 64)
        with pytest.raises(IndexError):
            ops.concat_linear_lrelu_l2norm(f, ix, f[:4, :8].contiguous(), W, flat[:8])
    with pytest.raises(R, match="self_rows and agg"):
        ops.concat_linear_lrelu_l2norm(f, i64[:5], f[:4, :8].contiguous(), W, flat[:8])
    with pytest.raises(R, match="b:"):
        ops.concat_linear_lrelu_l2norm(f, None, f[:4, :8].contiguous(), W, flat[:7])
    with pytest.raises(R, match="dy, y"):
        ops.norm_lrelu_backward(f[:4, :8], f[:4, :16].contiguous(), flat[:4])
    # the sampler's arguments
    indptr, indices, n_all, _ = su.bipartite_graph()
    ip, ix, src = dev(indptr), dev(indices), i64[:3]
    with pytest.raises(R, match="rng_mode"):
        ops.ppr_topk(ip, ix, src, 16, 0.85, 5, 1, 0, 0, "pcg")
    for k in (0, n_all + 1):
        with pytest.raises(R, match="k out of range"):
            ops.ppr_topk(ip, ix, src, 16, 0.85, k, 1, 0, 0, "philox")
    with pytest.raises(R, match="n_hops"):
        ops.walk(ip, ix, src, 0, 0.85, 1, 0, "philox", 0)
    tab = i64[:60].view(6, 10)
    with pytest.raises(R, match="T must be"):
        ops.frontier(i64[:3], tab, 11)
    with pytest.raises(R, match="n_items"):
        ops.frontier(i64[:3], tab, 3, 7)
    # no CPU implementation
    with pytest.raises(NotImplementedError):
        ops.gemm(f.cpu(), True, None, f.cpu(), True, None, 8, 8, 8)
    with pytest.raises(NotImplementedError):
        ops.weighted_agg(f.cpu(), loc.cpu(), w_ok.cpu())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- opcheck
def test_opcheck_schema_and_autograd_registration(ops):
    """torch.library.opcheck on one small argument set per op: an op that mutates
    an input, or a formula registered on the wrong key, shows here"""
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device="cuda")
    indptr, indices, n_all, _ = su.bipartite_graph()
    ip, ix = dev(indptr), dev(indices)
    loc = i32(0, 1, 2, 2, 1, 0).view(3, 2)
    y = torch.nn.functional.normalize(r(3, 8), dim=1)
    cases = (
        ("linear", (r(6, 8).requires_grad_(), i32(1, 5, 1), r(4, 8).requires_grad_(), r(4).requires_grad_(), True)),
        ("gemm", (r(8, 4), False, None, r(9, 8), False, i32(0, 3, 3, 8, 1, 2, 7, 5), 4, 8, 8)),
        ("weighted_agg", (r(3, 8).requires_grad_(), loc, torch.rand(3, 2, device="cuda", generator=g))),
        ("weighted_agg_backward", (r(3, 8), loc, torch.rand(3, 2, device="cuda", generator=g), 3)),
        ("segment_wmean", (r(5, 8), i64(0, 2, 2, 5), i32(0, 4, 1, 1, 3), r(5), True)),
        ("gather_rows", (r(5, 8).requires_grad_(), i64(4, 0, 4), 4)),
        ("scatter_add_rows", (r(3, 4).requires_grad_(), i64(4, 0, 4), 5, 8)),
        ("concat_linear_lrelu_l2norm", (r(5, 4).requires_grad_(), i64(4, 0, 4), r(3, 4).requires_grad_(),
                                        r(8, 8).requires_grad_(), r(8).requires_grad_())),
        ("norm_lrelu_backward", (r(3, 8), y, torch.ones(3, device="cuda"))),
        ("walk", (ip, ix, i64(0, 7), 16, 0.85, 3, 0, "philox", 0)),
        ("ppr_topk", (ip, ix, i64(0, 7), 16, 0.85, 5, 3, 0, 0, "philox")),
        ("frontier", (i64(2, 0), i64(*range(12)).view(4, 3) % 4, 2, -1)),
    )
    for name, args in cases:
        res = torch.library.opcheck(getattr(ops, name).default, args,
                                    test_utils=("test_schema", "test_autograd_registration"))
        assert set(res.values()) == {"SUCCESS"}, (name, res)
