"""The GEMM's engine-only forms against float64 (parity_util.gemm_form_reference):
every field of GemmParams that only engine_backward / engine_forward set --
device-side M and K, the second K and N segments, the output scatter, the
split output, the lrelu' mask, the partial slabs with bias_part and the L2-norm
epilogue under a scatter, stream-K and a device-side M -- through
pinsage_gemm_params, then reduce_slabs_2d_kernel through pinsage_reduce_slabs.

Conventions of every case: output buffers are larger than their live part
(more rows, ld > N, taller scatter targets) and pre-filled with a NaN pattern,
or with seeded values where the launch accumulates; whatever the reference
does not mark as written must keep its bits.  Each case runs with random inputs
(wide-range row scaling; held to parity_util's derived bounds) and with
exact-sum inputs (integers of magnitude <= 8: every partial sum is below 2^24
and the hi bf16 plane holds each operand exactly, so the result must equal
float64's bit for bit, whatever the tile, schedule or arithmetic), on tiles
cfg 0-3, under both product arithmetics, and under both schedules where
launch_gemm allows stream-K (the test asserts which one ran; the tickets must
be zero after every launch).  The measured error / bound ratios are printed
(pytest -s) and recorded in DESIGN.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import parity_util as pu
from parity_util import EPI_ACCUM, EPI_L2NORM, EPI_PARTIAL, EPI_STORE, GEMM_TILES

pytestmark = pytest.mark.gpu

ERR_ARG = -2
CFGS = (0, 1, 2, 3)
MODES = ("random", "exact")
SK_TICKETS = 4096
F_IN = ("a", "a2", "b", "b2", "bias", "mask")
I_IN = ("a_idx", "a2_idx", "b_idx", "b2_idx", "c_idx")
OUTS = ("c", "c2", "norms", "bias_part")
RATIOS = {}


def note(form, ratio):
    if ratio > RATIOS.get(form, -1.0):  # (printed when it grows: pytest -s shows the largest last)
        RATIOS[form] = ratio
        print(f"RATIO {form}: {ratio:.3f}")


def nan_fill(*shape):
    return np.full(shape, pu.NAN_BITS, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def sk():
    import _native as nat
    n = int(nat.lib().pinsage_gemm_sk_slab_floats())
    assert n > 0
    return dict(slab=torch.empty(n, dtype=torch.float32, device="cuda"),
                cnt=torch.zeros(SK_TICKETS, dtype=torch.int32, device="cuda"))


class Launch:
    """The device side of a launch spec (parity_util.gemm_form_reference's s).
    Also read from s: M_max / K_max (present: the size is device-side, s['M'] /
    s['K'] is written to the device before each launch), off = {buffer: floats}
    (the buffer starts that many floats past a 256-B boundary)."""

    def __init__(self, s):
        import _native as nat
        self.nat, self.lib, self.s = nat, nat.lib(), s
        self.t = {}
        for k in F_IN + OUTS:
            if s.get(k) is not None:
                self.put(k, s[k])
        for k in I_IN:
            if s.get(k) is not None:
                self.t[k] = torch.from_numpy(np.ascontiguousarray(s[k], np.int32)).cuda()
        if s.get("b2_idx") is not None and s["b2_idx"] is s.get("b_idx"):
            self.t["b2_idx"] = self.t["b_idx"]         # (launch_gemm: both gathered means by one table)
        self.Mdev = torch.zeros(1, dtype=torch.int32, device="cuda") if "M_max" in s else None
        self.Kdev = torch.zeros(1, dtype=torch.int32, device="cuda") if "K_max" in s else None

    def put(self, k, arr):
        a = np.ascontiguousarray(arr, np.float32)
        off = self.s.get("off", {}).get(k, 0)
        if k not in self.t:
            # (256 floats of slack behind every buffer: a kernel that reads a row's columns past ld
            # -- as a sensitivity mutant of the accumulate does -- stays inside the allocation)
            flat = torch.empty(a.size + off + 256, dtype=torch.float32, device="cuda")
            self.t[k] = flat[off:off + a.size].view(a.shape)
            assert self.t[k].data_ptr() % 16 == (4 * off) % 16
        self.t[k].copy_(torch.from_numpy(a))

    def read(self):
        return {k: self.t[k].cpu().numpy() for k in OUTS if k in self.t}

    def params(self, cfg, prec, stream_k=0, sk=None, hint=0, units=4):
        s, t = self.s, self.t
        p = lambda k: t[k].data_ptr() if k in t else None
        ld = lambda k: t[k].shape[1] if k in t else 0
        P = self.nat.GemmParams(
            M=0 if self.Mdev is not None else s["M"], N=s["N"], K=0 if self.Kdev is not None else s["K"],
            M_dev=None if self.Mdev is None else self.Mdev.data_ptr(), M_max=s.get("M_max", 0),
            K_dev=None if self.Kdev is None else self.Kdev.data_ptr(), K_max=s.get("K_max", 0), M_hint=hint,
            a_kmajor=int(s.get("a_kmajor", True)), b_kmajor=int(s.get("b_kmajor", True)),
            a=p("a"), lda=ld("a"), a_idx=p("a_idx"), K1=s.get("K1", -1), a2=p("a2"), lda2=ld("a2"), a2_idx=p("a2_idx"),
            b=p("b"), ldb=ld("b"), b_idx=p("b_idx"), N1=s.get("N1", -1), b2=p("b2"), ldb2=ld("b2"),
            b2_idx=p("b2_idx"), c=p("c"), ldc=ld("c"), c_idx=p("c_idx"), c2=p("c2"), ldc2=ld("c2"),
            bias_part=p("bias_part"), epi=s.get("epi", EPI_STORE), bias=p("bias"), act=int(bool(s.get("act"))),
            mask=p("mask"), ldm=ld("mask"), norms=p("norms"), splits=s.get("splits", 1), cfg=cfg, stream_k=stream_k,
            sk_min_units=units, prec=prec)
        if sk is not None:
            P.sk_slab, P.sk_cnt, P.sk_cnt_len = sk["slab"].data_ptr(), sk["cnt"].data_ptr(), SK_TICKETS
        return P

    def sk_allowed(self, cfg, stream_k, sk):
        s = self.s
        return bool(stream_k == 1 and sk is not None and cfg in (1, 2) and s.get("epi", 0) != EPI_PARTIAL and
                    self.Kdev is None and s["K"] > 0 and (s.get("a_kmajor", True) or s.get("a_idx") is None) and
                    (s.get("b_kmajor", True) or (s.get("b_idx") is None and s.get("b2_idx") is None)))

    def go(self, cfg, prec, stream_k=0, sk=None, hint=0, units=4, sync=True):
        if self.Mdev is not None:
            self.Mdev.fill_(self.s["M"])
        if self.Kdev is not None:
            self.Kdev.fill_(self.s["K"])
        P = self.params(cfg, prec, stream_k, sk, hint, units)
        ran = ctypes.c_int(-1)
        self.nat.check(self.lib.pinsage_gemm_params(ctypes.byref(P), ctypes.byref(ran), self.nat.stream_ptr()),
                       "gemm_params")
        # the schedule that ran is the one the case means to test
        assert ran.value == int(self.sk_allowed(cfg, stream_k, sk)), (ran.value, cfg, stream_k)
        if sync:
            torch.cuda.synchronize()
            if sk is not None:
                assert int(sk["cnt"].abs().max()) == 0, "stream-K tickets not reset"
        return ran.value

    def check(self, form, cfg, prec, exact, **kw):
        """one launch from the buffers' current contents, checked against the
        reference of exactly those contents"""
        pre = self.read()
        self.go(cfg, prec, **kw)
        got = self.read()
        ref = pu.gemm_form_reference(dict(self.s, **pre), prec, exact)
        ratio = pu.check_gemm_form(got, pre, ref, exact)
        if not exact:
            note(form, ratio)
        return got


def schedules(cfg):
    """(stream_k, sk_min_units): tiles, and on the tiles that carry the
    schedule stream-K with runs of 4 k-steps and of 1 (every tile cut)"""
    return ((0, 4), (1, 4), (1, 1)) if cfg in (1, 2) else ((0, 4),)


def injection(rng, n, rows):
    """n distinct rows of [0, rows) in random order (the engine's self_src /
    q_src index the members of a set: launch_gemm's scatter needs distinct rows)"""
    return rng.permutation(rows)[:n].astype(np.int32)


# ----------------------------------------------------------------------------- device-side M
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_device_side_m(cfg, mode, sk):
    """*M_dev in {0, 1, BM - 1, BM, BM + 1, 2 BM + 5, M_max} under one M_max,
    M_hint below, at and above it (the hint only picks the tile -- forced here,
    so it must change nothing), rows >= *M_dev untouched in C, c2 and norms,
    the buffers reused large -> small -> large without clearing (the bias
    changes with every launch, so a stale row differs from a fresh one).  Two
    forms: the store epilogue with a split output (bias, LeakyReLU), and the
    L2-norm epilogue with norms."""
    exact = mode == "exact"
    BM, BK = GEMM_TILES[cfg]
    M_max, K = 2 * BM + 8, BK + 8
    rng = np.random.default_rng(100 + cfg)
    for form, N in (("split-store", 136), ("l2norm", 100)):
        s = dict(M=M_max, M_max=M_max, N=N, K=K, a=pu.form_values(rng, (M_max, K + 4), exact, wide=True),
                 b=pu.form_values(rng, (N, K + 8), exact), bias=pu.form_values(rng, (N,), exact),
                 c=nan_fill(M_max + 2, N + 4))
        if form == "split-store":
            s.update(N1=68, c2=nan_fill(M_max + 1, N - 68 + 8), act=True)
        else:
            s.update(epi=EPI_L2NORM, norms=nan_fill(M_max + 3))
        L = Launch(s)
        for M in (M_max, 0, 1, BM - 1, BM, BM + 1, 2 * BM + 5, M_max):
            s["M"] = M
            for hint in (max(M - 1, 0), M, M + 7):
                for prec in (0, 1):
                    for stream_k, units in schedules(cfg):
                        s["bias"] = pu.form_values(rng, (N,), exact)
                        L.put("bias", s["bias"])
                        L.check(f"device-M {form}", cfg, prec, exact, stream_k=stream_k, units=units, sk=sk, hint=hint)


# ----------------------------------------------------------------------------- second K segment
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_second_k_segment(cfg, mode, sk):
    """K1 in {4, BK - 4, BK, BK + 4, K - 4}: the seam inside a stage, on a stage
    edge and in the last stage; a gathered by a_idx, a2 by row (and by a2_idx),
    lda != lda2, both padded.  The store epilogue at N = 132, the L2-norm
    epilogue at N in {4, 100, 128} -- plain, scattered through c_idx and with
    a device-side M -- with its norms.  Row 3's pre-norm values are all
    negative (its operand rows are zero and the bias is negative), so the
    LeakyReLU branch is taken in every column."""
    exact = mode == "exact"
    BM, BK = GEMM_TILES[cfg]
    M, K = BM + 37, 3 * BK + 4
    rng = np.random.default_rng(200 + cfg)
    rows_a, rows_a2 = M + 11, M + 5
    a_idx = injection(rng, M, rows_a)
    a2_idx = injection(rng, M, rows_a2)
    for K1 in (4, BK - 4, BK, BK + 4, K - 4):
        a = pu.form_values(rng, (rows_a, K1 + 4), exact, wide=True)
        a2 = pu.form_values(rng, (rows_a2, K - K1 + 8), exact)
        a[a_idx[3]] = 0
        forms = [("store", 132, None, False, False)]
        forms += [("l2norm", N, None, False, True) for N in (4, 100, 128)]
        forms += [("l2norm-scatter", 100, injection(rng, M, M + 9), False, False),
                  ("l2norm-device-M", 128, None, True, True)]
        for form, N, c_idx, mdev, by_row in forms:
            a2v = a2.copy()
            a2v[3 if by_row else a2_idx[3]] = 0
            bias = -np.abs(pu.form_values(rng, (N,), exact)) - 1
            s = dict(M=M, N=N, K=K, a=a, a_idx=a_idx, K1=K1, a2=a2v, a2_idx=None if by_row else a2_idx,
                     b=pu.form_values(rng, (N, K + 4), exact), bias=bias, c=nan_fill(M + 9, N + 4), c_idx=c_idx)
            if form != "store":
                s.update(epi=EPI_L2NORM, norms=nan_fill(M + 4))
            if mdev:
                s.update(M_max=M + 3)
            L = Launch(s)
            for prec in (0, 1):
                for stream_k, units in schedules(cfg):
                    for k in OUTS:
                        if k in L.t:
                            L.put(k, s[k])
                    got = L.check(f"K-segment {form}", cfg, prec, exact, stream_k=stream_k, units=units, sk=sk, hint=M)
                    if form != "store":  # the row that takes the slope everywhere: y = bias / |bias|
                        r = 3 if c_idx is None else c_idx[3]
                        assert (got["c"][r, :N] < 0).all()


# ----------------------------------------------------------------------------- second N segment
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_second_n_segment(cfg, mode, sk):
    """N1 in {4, 28, 32, 124, 128, 132, N - 4} of an N-major B whose k-rows are
    gathered by b_idx, b2 by k (and by the same b_idx), M-major A: the store
    epilogue and the partial one (three splits, bias_part).  Gathered k-rows
    exclude stream-K: asking for it must run the tiles."""
    exact = mode == "exact"
    M, N, K = 68, 264, 72
    rng = np.random.default_rng(300 + cfg)
    b_idx = rng.integers(0, K + 9, K).astype(np.int32)
    A = pu.form_values(rng, (K, M + 4), exact, wide=True)
    for N1 in (4, 28, 32, 124, 128, 132, N - 4):
        for both in (False, True):
            rows2 = K + 9 if both else K
            s = dict(M=M, N=N, K=K, a_kmajor=False, b_kmajor=False, a=A, N1=N1, b_idx=b_idx,
                     b=pu.form_values(rng, (K + 9, N1 + 4), exact), b2=pu.form_values(rng, (rows2, N - N1 + 8), exact),
                     b2_idx=b_idx if both else None)
            for form in ("store", "partial"):
                if form == "store":
                    s2 = dict(s, bias=pu.form_values(rng, (N,), exact), c=nan_fill(M + 2, N + 4))
                else:
                    s2 = dict(s, epi=EPI_PARTIAL, splits=3, c=nan_fill(3 * M + 2, N), bias_part=nan_fill(3, M))
                L = Launch(s2)
                for prec in (0, 1):
                    for k in OUTS:
                        if k in L.t:
                            L.put(k, s2[k])
                    L.check(f"N-segment {form}", cfg, prec, exact, stream_k=1 if form == "store" else 0, sk=sk)


# ----------------------------------------------------------------------------- scatter, accumulate, split output
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_scatter_accumulate_split_output(cfg, mode, sk):
    """The bwd.dcat form, then bwd.dh into the same rows: dp [M][K] times an
    N-major W [K][N]; columns < N1 are added to the rows c_idx names of a
    taller C over seeded values, columns >= N1 stored plainly by row to c2
    (NaN pre-fill, ldc2 != N - N1); then a second launch adds dpq Q through
    another injection into the same C.  N1 in {4, 124, 128, 132}; M static and
    device-side; tiles and stream-K; the 16-byte epilogue and the scalar one
    (C offset by one float, c2 offset by one float, an odd ldc)."""
    exact = mode == "exact"
    BM, BK = GEMM_TILES[cfg]
    M, K = BM + 41, 5 * BK
    rng = np.random.default_rng(400 + cfg)
    rows_c = M + 37
    for N1 in (4, 124, 128, 132):
        N = N1 + 72
        for align, mdev in (("wide", False), ("wide", True), ("c+1", True), ("c2+1", False), ("odd-ldc", True)):
            ldc = N1 + (5 if align == "odd-ldc" else 8)
            s = dict(M=M, N=N, K=K, b_kmajor=False, a=pu.form_values(rng, (M + 3, K + 4), exact, wide=True),
                     b=pu.form_values(rng, (K, N + 4), exact), c=pu.form_values(rng, (rows_c, ldc), exact),
                     c_idx=injection(rng, M + 3, rows_c), epi=EPI_ACCUM, N1=N1, c2=nan_fill(M + 5, N - N1 + 4),
                     off={"c": int(align == "c+1"), "c2": int(align == "c2+1")})
            if mdev:
                s.update(M_max=M + 3)
            dh = dict(M=M + 2, N=N1, K=K, b_kmajor=False, a=pu.form_values(rng, (M + 2, K), exact),
                      b=pu.form_values(rng, (K, N1 + 4), exact), c=s["c"], c_idx=injection(rng, M + 2, rows_c),
                      epi=EPI_ACCUM, off=s["off"])
            L = Launch(s)
            L2 = Launch(dh)
            L2.t["c"] = L.t["c"]                       # the same C, as dcat and dh share dY
            for prec in (0, 1):
                for stream_k, units in schedules(cfg):
                    L.put("c", s["c"])
                    L.put("c2", s["c2"])
                    L.check("scatter-accumulate dcat", cfg, prec, exact, stream_k=stream_k, units=units, sk=sk,
                            hint=M)
                    L2.check("scatter-accumulate dh", cfg, prec, exact, stream_k=stream_k, units=units, sk=sk)


# ----------------------------------------------------------------------------- mask
def test_mask_with_accumulate_is_refused():
    import _native as nat
    rng = np.random.default_rng(0)
    s = dict(M=8, N=8, K=8, a=pu.form_values(rng, (8, 8), True), b=pu.form_values(rng, (8, 8), True),
             mask=pu.form_values(rng, (8, 8), True), c=nan_fill(8, 8), epi=EPI_ACCUM)
    L = Launch(s)
    P = L.params(-1, 0)
    assert nat.lib().pinsage_gemm_params(ctypes.byref(P), None, nat.stream_ptr()) == ERR_ARG
    assert b"mask" in nat.lib().pinsage_last_error()
    torch.cuda.synchronize()
    assert (pu.bits32(L.read()["c"]) == pu.NAN_BITS).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_mask(cfg, mode, sk):
    """The head backward's dP1 = (dZ G2) lrelu'(H1): the mask holds positive
    and negative values, 0.0, -0.0 and denormals of both signs (only x > 0
    takes 1); ldm != ldc; M static and device-side; the 16-byte epilogue and
    the scalar one (mask offset by one float, C offset by one float)."""
    exact = mode == "exact"
    BM, BK = GEMM_TILES[cfg]
    M, N, K = BM + 29, 132, 2 * BK + 4
    rng = np.random.default_rng(500 + cfg)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.0, -1.0], np.float32)
    for align in ("wide", "mask+1", "c+1"):
        for mdev in (False, True):
            mask = pu.form_values(rng, (M + 2, N + 12), False)
            pick = rng.random(mask.shape) < 0.5
            mask[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
            s = dict(M=M, N=N, K=K, b_kmajor=False, a=pu.form_values(rng, (M + 2, K + 4), exact, wide=True),
                     b=pu.form_values(rng, (K, N + 8), exact), mask=mask, c=nan_fill(M + 4, N + 4),
                     off={"mask": int(align == "mask+1"), "c": int(align == "c+1")})
            if mdev:
                s.update(M_max=M + 2)
            L = Launch(s)
            for prec in (0, 1):
                for stream_k, units in schedules(cfg):
                    L.put("c", s["c"])
                    L.check("mask", cfg, prec, exact, stream_k=stream_k, units=units, sk=sk, hint=M)


# ----------------------------------------------------------------------------- device-side K, partial slabs, reduction
def reduce_slabs(part, S, M, N, out, bpart=None, bias_out=None, adam=None, coef=None, betas=(0.9, 0.999), eps=1e-8):
    """pinsage_reduce_slabs on device tensors: part [>= S * M * N], out [M][ld]"""
    import _native as nat
    ad = list(adam) if adam else [None] * 6
    nat.check(nat.lib().pinsage_reduce_slabs(
        nat.ptr(part), S, M * N, M, N, nat.ptr(out), out.shape[1], nat.ptr(bpart), nat.ptr(bias_out),
        *[nat.ptr(t) for t in ad], nat.ptr(coef), betas[0], betas[1], eps, nat.stream_ptr()), "reduce_slabs")
    torch.cuda.synchronize()


PARTIAL_M = {0: 128, 1: 68, 2: 4, 3: 64}   # the reduction's row counts, one per tile


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_device_side_k_partials_then_reduction(cfg, mode):
    """The split-K weight-gradient fallback: M-major A, N-major B gathered by
    b_idx with its columns >= N1 from b2, *K_dev in {0, 1, 3, 4, 5, BK - 1, BK,
    BK + 1, K_max = 1032}, S in {1, 2, 3, 4, 5, 16, 17, 64} splits -- most of
    them empty at small K, 17 of 17 and 33 of 64 live at K_max (the reduction's
    sixteen-at-a-time order then differs from one by one): every slab and bias_part row of an empty split must be
    written as zero over the NaN pre-fill, because the reduction reads all S.
    Then pinsage_reduce_slabs on the device's own slabs: bitwise the order
    emulation (so bitwise exact on exact-sum inputs), within (S + 1) 2^-24
    sum |slab| of float64, out at ld > N, rows and columns past the live part
    untouched; M N / 4 is a multiple of 64 for M = 64 and 128 only."""
    exact = mode == "exact"
    BM, BK = GEMM_TILES[cfg]
    M, N, N1, K_max = PARTIAL_M[cfg], 44, 28, 1032
    rng = np.random.default_rng(600 + cfg)
    b_idx = rng.integers(0, K_max + 5, K_max).astype(np.int32)
    base = dict(M=M, N=N, K=K_max, K_max=K_max, a_kmajor=False, b_kmajor=False, N1=N1, b_idx=b_idx, epi=EPI_PARTIAL,
                a=pu.form_values(rng, (K_max, M + 4), exact, wide=True),
                b=pu.form_values(rng, (K_max + 5, N1 + 4), exact), b2=pu.form_values(rng, (K_max, N - N1 + 4), exact))
    for S in (1, 2, 3, 4, 5, 16, 17, 64):
        s = dict(base, splits=S, c=nan_fill(S * M + 1, N), bias_part=nan_fill(S + 1, M))
        L = Launch(s)
        out = torch.empty((M + 2, N + 4), dtype=torch.float32, device="cuda")
        bout = torch.empty(M + 3, dtype=torch.float32, device="cuda")
        for K in (0, 1, 3, 4, 5, BK - 1, BK, BK + 1, K_max):
            s["K"] = K
            for prec in (0, 1):
                L.put("c", s["c"])
                L.put("bias_part", s["bias_part"])
                got = L.check("partial slabs", cfg, prec, exact)
                out.view(torch.int32).fill_(pu.NAN_BITS)
                bout.view(torch.int32).fill_(pu.NAN_BITS)
                pre_o, pre_b = out.cpu().numpy(), bout.cpu().numpy()
                reduce_slabs(L.t["c"], S, M, N, out, L.t["bias_part"], bout)
                part = got["c"][:S * M].reshape(S, M, N)
                note("reduce_slabs", pu.check_reduce_slabs("out", out.cpu().numpy(), pre_o, part, M, N))
                note("reduce_slabs bias", pu.check_reduce_slabs("bias_out", bout.cpu().numpy(), pre_b,
                                                                got["bias_part"][:S], M, N, pu.reduce_bias32))
                if exact:  # the whole fallback, bit for bit: dW = A^T B and its column sums
                    A, B = pu.gemm_operands(s)
                    assert (out.cpu().numpy()[:M, :N] == (A @ B).astype(np.float32)).all()
                    assert (bout.cpu().numpy()[:M] == A.sum(1).astype(np.float32)).all()


# ----------------------------------------------------------------------------- stream-K hygiene
def test_stream_k_reruns_are_bitwise_equal_and_share_scratch(sk):
    """Three runs of a cut-tile launch give the same bits; a scatter-accumulate
    launch and an L2-norm launch back to back on one stream share the scratch
    (no synchronisation between them) and both come out right; the tickets are
    zero afterwards."""
    rng = np.random.default_rng(700)
    M, K = 150, 160
    acc = dict(M=M, N=136, K=K, b_kmajor=False, a=pu.form_values(rng, (M, K), False, wide=True),
               b=pu.form_values(rng, (K, 136), False), c=pu.form_values(rng, (M + 20, 72), False),
               c_idx=injection(rng, M, M + 20), epi=EPI_ACCUM, N1=64, c2=nan_fill(M + 1, 76))
    l2 = dict(M=M, N=100, K=K, a=pu.form_values(rng, (M, K), False), b=pu.form_values(rng, (100, K), False),
              bias=pu.form_values(rng, (100,), False), c=nan_fill(M + 1, 104), epi=EPI_L2NORM, norms=nan_fill(M + 1))
    for cfg in (1, 2):
        for prec in (0, 1):
            La, Ln = Launch(acc), Launch(l2)
            runs = []
            for _ in range(3):
                La.put("c", acc["c"])
                La.put("c2", acc["c2"])
                Ln.put("c", l2["c"])
                Ln.put("norms", l2["norms"])
                pre_a, pre_n = La.read(), Ln.read()
                assert La.go(cfg, prec, stream_k=1, units=1, sk=sk, sync=False) == 1
                assert Ln.go(cfg, prec, stream_k=1, units=1, sk=sk, sync=False) == 1
                torch.cuda.synchronize()
                assert int(sk["cnt"].abs().max()) == 0
                ga, gn = La.read(), Ln.read()
                pu.check_gemm_form(ga, pre_a, pu.gemm_form_reference(dict(acc, **pre_a), prec))
                pu.check_gemm_form(gn, pre_n, pu.gemm_form_reference(dict(l2, **pre_n), prec))
                runs.append({**{"a." + k: v for k, v in ga.items()}, **{"n." + k: v for k, v in gn.items()}})
            for r in runs[1:]:
                for k in r:
                    assert (pu.bits32(r[k]) == pu.bits32(runs[0][k])).all(), (cfg, prec, k)


# ----------------------------------------------------------------------------- norm_lrelu_bwd, the engine's form
@pytest.mark.parametrize("out", (4, 63, 64, 65, 128, 200))
def test_norm_lrelu_backward_engine_form(out):
    """norm_lrelu_bwd_kernel as engine_backward launches it: the row count from
    the device (*nrows in {cap, 0, 1, 5, cap}; rows beyond it untouched), y with
    elements that are exactly 0 (they take the slope), and the zeroing folded
    into the launch -- z over exactly *z_rows x z_n and zi over exactly zi_n,
    not one element further; null z / zi zero nothing."""
    import _native as nat
    lib = nat.lib()
    cap, z_n, z_cap = 37, 12, 9
    rng = np.random.default_rng(900 + out)
    v = rng.standard_normal((cap, out))
    v[rng.random(v.shape) < 0.2] = 0.0
    v[:, 0] = 1.0
    nrm = np.linalg.norm(v, axis=1)
    y = (v / nrm[:, None]).astype(np.float32)
    assert (y == 0).any()
    dy = pu.wide_rows(rng, (cap, out))
    ref, bound = pu.norm_lrelu_bwd_reference(y, nrm.astype(np.float32), dy)
    d_y, d_n, d_dy = (torch.from_numpy(a).cuda() for a in (y, nrm.astype(np.float32), dy))
    d_rows, d_zrows = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    dp = torch.empty((cap + 1, out), dtype=torch.float32, device="cuda")
    z = torch.empty(z_cap * z_n + 3, dtype=torch.float32, device="cuda")
    zi = torch.empty(1000 + 5, dtype=torch.int32, device="cuda")
    for nrows, z_rows, zi_n, with_z in ((cap, z_cap, 1000, True), (0, 0, 0, True), (1, 3, 7, True),
                                        (5, 1, 64, False), (cap, z_cap - 1, 257, True)):
        dp.view(torch.int32).fill_(pu.NAN_BITS)
        z.fill_(7.5)
        zi.fill_(-3)
        d_rows.fill_(nrows)
        d_zrows.fill_(z_rows)
        nat.check(lib.pinsage_norm_lrelu_backward_ex(
            nat.ptr(d_y), nat.ptr(d_n), nat.ptr(d_dy), nat.ptr(d_rows), cap, out, nat.ptr(dp),
            nat.ptr(z) if with_z else None, z_n, nat.ptr(d_zrows), nat.ptr(zi) if with_z else None, zi_n,
            nat.stream_ptr()), "norm_lrelu_backward_ex")
        torch.cuda.synchronize()
        r = dict(want=np.full((cap + 1, out), np.nan), bound=np.zeros((cap + 1, out)),
                 written=np.zeros((cap + 1, out), bool))
        r["want"][:nrows], r["bound"][:nrows], r["written"][:nrows] = ref[:nrows], bound[:nrows], True
        note("norm_lrelu_bwd", pu.check_written("dp", dp.cpu().numpy(), nan_fill(cap + 1, out), r))
        zn = z_rows * z_n if with_z else 0
        zz, zzi = z.cpu().numpy(), zi.cpu().numpy()
        assert (zz[:zn] == 0).all() and (zz[zn:] == 7.5).all(), (nrows, z_rows, np.flatnonzero(zz != 7.5)[-1:])
        zin = zi_n if with_z else 0
        assert (zzi[:zin] == 0).all() and (zzi[zin:] == -3).all(), (nrows, zi_n)
