"""The optimizer pass against float64: adam_kernel through pinsage_adam, and the
Adam slice of reduce_slabs_2d_kernel through pinsage_reduce_slabs, each step
from the device's own state before it (parity_util.adam_reference restates
torch's _single_tensor_adam with the host's float32 coef and derives the bound
from adam1's roundings).  "Parameters within +-lr per step" is Adam's
conditioning; this holds m and v to a few roundings and p to those carried
through m / (sqrt(v) / bc2 + eps).  The slice and adam_kernel agree to that
bound on the same gradient, not bit for bit (see the slice's test).
The measured error / bound ratios are printed (pytest -s) and recorded in
DESIGN.md.
"""
import numpy as np
import pytest
import torch

import parity_util as pu

pytestmark = pytest.mark.gpu

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1e-3
GUARD = 4                                  # floats past n that must keep their bits
RATIOS = {}


def note(form, ratio):
    if ratio > RATIOS.get(form, -1.0):
        RATIOS[form] = ratio
        print(f"RATIO {form}: {ratio:.3f}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def adam(p, g, m, v, n, coef):
    import _native as nat
    nat.check(nat.lib().pinsage_adam(nat.ptr(p), nat.ptr(g), nat.ptr(m), nat.ptr(v), n, nat.ptr(coef), BETAS[0],
                                     BETAS[1], EPS, nat.stream_ptr()), "adam")
    torch.cuda.synchronize()


def guarded(a):
    """a followed by GUARD floats of the NaN pattern"""
    return np.concatenate([np.asarray(a, np.float32).reshape(-1),
                           np.full(GUARD, pu.NAN_BITS, np.uint32).view(np.float32)])


@pytest.mark.parametrize("n", (1, 3, 4, 5, 1023, 1024, 1025, 65537))
def test_adam_matches_float64(n):
    """t = 1 .. 5 steps from zero moments, a fresh gradient each step with
    elements that are exactly 0, +-1e-30 (g^2 underflows; sqrt(v) / bc2 is far
    below eps) and near 1e4; n on both sides of the float4 body and its tail.
    Nothing past n changes; coef[1] == 0 (a refused step) leaves p, m and v
    bit for bit."""
    rng = np.random.default_rng(n)
    p = dev(guarded(rng.standard_normal(n)))
    m, v = dev(guarded(np.zeros(n))), dev(guarded(np.zeros(n)))
    for t in range(1, 6):
        g = dev(guarded(pu.adam_gradient(rng, n)))
        coef = pu.adam_coef(t, LR, *BETAS)
        pre = [x.cpu().numpy() for x in (p, g, m, v)]
        adam(p, g, m, v, n, dev(coef))
        got = [x.cpu().numpy() for x in (p, m, v)]
        ref = pu.adam_reference(pre[0][:n], pre[1][:n], pre[2][:n], pre[3][:n], coef, *BETAS, EPS)
        note("adam_kernel", pu.check_adam(got[0][:n], got[1][:n], got[2][:n], ref))
        for name, a in zip("pmv", got):
            assert (pu.bits32(a[n:]) == pu.NAN_BITS).all(), f"adam {name}: a store past element {n - 1}"
    before = [pu.bits32(x.cpu().numpy()) for x in (p, m, v)]
    adam(p, g, m, v, n, dev(np.array([LR, 0.0], np.float32)))
    for name, b, x in zip("pmv", before, (p, m, v)):
        assert (pu.bits32(x.cpu().numpy()) == b).all(), f"adam {name} changed by a refused step"


@pytest.mark.parametrize("M", (4, 64, 68))
def test_reduce_slabs_adam_slice_is_adam_kernel(M):
    """The Adam slice of the split-K reduction on weights [M][N] at ld > N and a
    bias [M]: the reduced gradient bitwise the order emulation, p / m / v within
    the float64 bound, and so is what pinsage_adam makes of the same gradient
    and state; the padding columns of p, m and v keep their bits.  The two are
    NOT bitwise equal: the compiler contracts v * beta2 + (1 - beta2) * g * g
    into fma(beta2, v, .) in adam_kernel's float4 body, into fma(g, (1 - beta2)
    g, .) in the reduction and not at all in adam_kernel's scalar tail and the
    reduction's bias rows (DESIGN.md section 4 states it); the count of
    differing elements is printed.  Steps t = 1,
    2, 5 on continuing state; then coef[1] == 0 leaves the state untouched
    (the gradient is still written)."""
    import _native as nat
    N, ld, S = 44, 48, 5
    rng = np.random.default_rng(800 + M)
    P = rng.standard_normal((M, ld)).astype(np.float32)
    Mo = (0.1 * rng.standard_normal((M, ld))).astype(np.float32)
    V = (rng.random((M, ld)) * 1e-2).astype(np.float32)
    st = [dev(P), dev(Mo), dev(V), dev(P[:, 0].copy()), dev(Mo[:, 0].copy()), dev(V[:, 0].copy())]
    for t in (1, 2, 5, 0):
        part = np.stack([pu.adam_gradient(rng, M * N).reshape(M, N) for _ in range(S)])
        bpart = np.stack([pu.adam_gradient(rng, M) for _ in range(S)])
        coef = pu.adam_coef(t, LR, *BETAS) if t else np.array([LR, 0.0], np.float32)
        out = dev(np.full((M, ld), pu.NAN_BITS, np.uint32).view(np.float32))
        bout = dev(np.full(M, pu.NAN_BITS, np.uint32).view(np.float32))
        pre = [x.cpu().numpy() for x in st]
        twin = [x.clone() for x in st]
        d_part, d_bpart, d_coef = dev(part), dev(bpart), dev(coef)
        nat.check(nat.lib().pinsage_reduce_slabs(
            nat.ptr(d_part), S, M * N, M, N, nat.ptr(out), ld, nat.ptr(d_bpart), nat.ptr(bout),
            *[nat.ptr(x) for x in st], nat.ptr(d_coef), BETAS[0], BETAS[1], EPS, nat.stream_ptr()), "reduce_slabs")
        torch.cuda.synchronize()
        g, gb = out.cpu().numpy(), bout.cpu().numpy()
        pu.check_reduce_slabs("out", g, np.full((M, ld), pu.NAN_BITS, np.uint32).view(np.float32), part, M, N)
        pu.check_reduce_slabs("bias_out", gb, np.full(M, pu.NAN_BITS, np.uint32).view(np.float32), bpart, M, N,
                              pu.reduce_bias32)
        got = [x.cpu().numpy() for x in st]
        if t == 0:
            for name, a, b in zip(("p", "m", "v", "pb", "mb", "vb"), got, pre):
                assert (pu.bits32(a) == pu.bits32(b)).all(), f"{name} changed by a refused step"
            continue
        # adam_kernel on the same gradient and state (padding columns: gradient 0), held to the same bound
        gz = out.clone()
        gz[:, N:] = 0
        adam(twin[0], gz, twin[1], twin[2], M * ld, d_coef)
        adam(twin[3], bout, twin[4], twin[5], M, d_coef)
        tw = [x.cpu().numpy() for x in twin]
        ref = pu.adam_reference(pre[0][:, :N], g[:, :N], pre[1][:, :N], pre[2][:, :N], coef, *BETAS, EPS)
        rc = lambda i: f"row {i[0]}, column {i[1]}"
        note("adam slice", pu.check_adam(got[0][:, :N], got[1][:, :N], got[2][:, :N], ref, rc))
        note("adam_kernel", pu.check_adam(tw[0][:, :N], tw[1][:, :N], tw[2][:, :N], ref, rc))
        refb = pu.adam_reference(pre[3], gb, pre[4], pre[5], coef, *BETAS, EPS)
        note("adam slice bias", pu.check_adam(got[3], got[4], got[5], refb, lambda i: f"row {i[0]}"))
        note("adam_kernel", pu.check_adam(tw[3], tw[4], tw[5], refb, lambda i: f"row {i[0]}"))
        differ = 0
        for name, a, b, w in zip(("p", "m", "v", "pb", "mb", "vb"), got, pre, tw):
            if a.ndim == 2:
                assert (pu.bits32(a[:, N:]) == pu.bits32(b[:, N:])).all(), f"{name}: padding columns changed"
                a, w = a[:, :N], w[:, :N]
            differ += int((pu.bits32(a) != pu.bits32(w)).sum())
        print(f"SLICE-VS-KERNEL M={M} step {t}: {differ} of {6 * M * N // 2 + 3 * M} elements differ in the last bits")


@pytest.mark.parametrize("mode", ("random", "exact"))
@pytest.mark.parametrize("M", (4, 64, 68, 128))
def test_reduce_slabs_dense(M, mode):
    """reduce_slabs_2d_kernel on S in {1, 2, 3, 4, 5, 16, 17, 64} slabs that are
    all live (the GEMM's own slabs are mostly empty at those S): bitwise the
    order emulation -- which tells sixteen at a time from one by one -- within
    (S + 1) 2^-24 sum |slab| of float64, bitwise exact on exact-sum inputs, out
    at ld > N over a NaN pre-fill, M N / 4 not a multiple of 64 at M = 4, 68."""
    import _native as nat
    N, ld = 44, 52
    rng = np.random.default_rng(850 + M)
    for S in (1, 2, 3, 4, 5, 16, 17, 64):
        part = pu.form_values(rng, (S, M, N), mode == "exact", wide=True)
        bpart = pu.form_values(rng, (S, M), mode == "exact", wide=True)
        pre_o = np.full((M + 1, ld), pu.NAN_BITS, np.uint32).view(np.float32)
        pre_b = np.full(M + 2, pu.NAN_BITS, np.uint32).view(np.float32)
        out, bout, d_part, d_bpart = dev(pre_o), dev(pre_b), dev(part), dev(bpart)
        nat.check(nat.lib().pinsage_reduce_slabs(
            nat.ptr(d_part), S, M * N, M, N, nat.ptr(out), ld, nat.ptr(d_bpart), nat.ptr(bout), *[None] * 7,
            BETAS[0], BETAS[1], EPS, nat.stream_ptr()), "reduce_slabs")
        torch.cuda.synchronize()
        note("reduce_slabs dense", pu.check_reduce_slabs("out", out.cpu().numpy(), pre_o, part, M, N))
        note("reduce_slabs dense bias", pu.check_reduce_slabs("bias_out", bout.cpu().numpy(), pre_b, bpart, M, N,
                                                              pu.reduce_bias32))
        if mode == "exact":
            assert (out.cpu().numpy()[:M, :N] == part.astype(np.float64).sum(0)).all()
            assert (bout.cpu().numpy()[:M] == bpart.astype(np.float64).sum(0)).all()
