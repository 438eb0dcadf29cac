"""The transposed aggregation (the backward of pinsage_model.py:202 towards the
q rows) and the CSR build under it (csrc/dq.hip), through the C-ABI entry
pinsage_agg_transpose (csr_count / scan / csr_fill / the canonical sorts /
dq_chunk_kernel + dq_combine_kernel or the split-row tree, launched as the
engine launches them over dq.h's plan), against float64 torch on the same
fp32 inputs:

  dpq[u] = lrelu'(q[u]) * sum over the slots (f, t) with loc[f][t] == u of
           w[f][t] * dagg[f]

Slot tables come from a deterministic builder with the engine tables' real
property: every source row has exactly T slots and the pairs (u, f) are
distinct.  The main table holds q rows of 1, 4, 5, 15, 16 occurrences (partial
4-row groups, one chunk), 17, 32, 33, 64 (2-4 chunks, the wave sort), 65 (the
bitmap sort), 128 / 129 (one full tree node / two levels with a lone last
child), 1024 / 1025 (64 / 65 chunks, three levels) and 8192 / 8193 (512 / 513
chunks, four levels), padded with rows of 1-3 occurrences and a few of none.

Exact cases: w in {1/4, 1/2, 1, 2} and integer dagg make every partial sum an
exact fp32 value, so any summation order gives the float64 sum's bits: one
lost, doubled or misrouted pair fails at any row length.  Random cases are held
per row and per element to slope (D + 1) 2^-24 sum |w dagg| with D the depth
of the row's documented summation order (16-term chunk chains, then 7 adds per
tree level, or ceil(chunks / 16) + 15 adds in the combine kernel); the bound
comes from that order, not from the kernel's measured error (DESIGN.md has
the measured figures beside it).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SLOPE = np.float32(0.01)  # leaky_relu's negative slope as the kernels hold it

MAIN_COUNTS = [1, 4, 5, 15, 16, 17, 32, 33, 64, 65, 128, 129, 1024, 1025, 8192, 8193]
MAIN_T, MAIN_ROWS = 3, 8200


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- slot tables
def _build_loc(counts, T, seed):
    """loc int32 [n_rows][T] in which q row u occurs counts[u] times: u repeated
    counts[u] times in u order, slot e given to source row e mod n_rows (a
    run of <= n_rows equal values meets every source row at most once), each
    source row's T slots shuffled.  Checked here, on the CPU."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    assert n % T == 0 and n > 0
    n_rows = n // T
    assert int(counts.max()) <= n_rows
    lay = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    loc = np.ascontiguousarray(lay.reshape(T, n_rows).T)
    order = np.argsort(np.random.default_rng(seed).random((n_rows, T)), axis=1)
    loc = np.ascontiguousarray(np.take_along_axis(loc, order, axis=1))
    _check_loc(loc, counts)
    return loc


def _check_loc(loc, counts):
    assert loc.dtype == np.int32 and loc.min() >= 0 and loc.max() < len(counts)
    assert (np.bincount(loc.ravel(), minlength=len(counts)) == counts).all()
    s = np.sort(loc, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all()  # the pairs (u, f) are distinct


def _pad_counts(total, cycle=(1, 2, 3)):
    """counts cycling through `cycle` that add up to total"""
    out, i = [], 0
    while total > 0:
        c = min(cycle[i % len(cycle)], total)
        out.append(c)
        total -= c
        i += 1
    return out


@functools.lru_cache(maxsize=None)
def _main_table():
    """(counts, loc) of the main case: the special rows spread among rows of
    1-3 occurrences, rows of none at u = 7, in the middle and at the end"""
    pad = _pad_counts(MAIN_ROWS * MAIN_T - sum(MAIN_COUNTS))
    counts, special = [], list(MAIN_COUNTS)
    for i, c in enumerate(pad):
        if i % 150 == 20 and special:
            counts.append(special.pop(0))
        if i in (7, 1500):
            counts.append(0)
        counts.append(c)
    counts += special + [0]
    counts = np.asarray(counts, np.int64)
    for c in MAIN_COUNTS:
        assert (counts == c).any()
    return counts, _build_loc(counts, MAIN_T, seed=1)


@functools.lru_cache(maxsize=None)
def _regime_table(U):
    """U q rows of 1-3 occurrences plus one row of 300 (19 chunks: the bitmap
    sort, a two-level tree), T = 3"""
    counts = [1 + (i % 3) for i in range(U)]
    counts[U // 2] = 300
    i = 0
    while sum(counts) % 3:  # make the slots divide into rows of T
        if counts[i] == 1:
            counts[i] = 2
        i += 1
    counts = np.asarray(counts, np.int64)
    return counts, _build_loc(counts, 3, seed=U)


# ----------------------------------------------------------------------------- inputs, launch, reference
def _q(U, hid, g):
    """q rows mixing positives, negatives, 0.0 and -0.0 (lrelu' is the slope at both zeros)"""
    q = torch.randn(U, hid, generator=g)
    z = torch.rand(U, hid, generator=g)
    q[z < 0.1] = 0.0
    q[z > 0.9] = -0.0
    return q.cuda()


def _exact_inputs(n_rows, T, U, hid, ld, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (n_rows, T), generator=g)]
    dagg = torch.randint(-8, 9, (n_rows, ld), generator=g).float()
    return w.cuda(), dagg.cuda(), _q(U, hid, g)


def _random_inputs(n_rows, T, U, hid, ld, seed, dyadic_w=False):
    g = torch.Generator().manual_seed(seed)
    if dyadic_w:
        w = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (n_rows, T), generator=g)]
    else:  # normalised importance weights, as the tables'
        w = torch.rand(n_rows, T, generator=g, dtype=torch.float64) + 0.01
        w = (w / w.sum(1, keepdim=True)).float()
    dagg = torch.randn(n_rows, ld, generator=g)
    return w.cuda(), dagg.cuda(), _q(U, hid, g)


def _scratch(n_rows_max, T, n_q_max, hid):
    import _native as nat
    nb = nat.lib().pinsage_agg_transpose_scratch_bytes(n_rows_max, T, n_q_max, hid)
    assert nb > 0
    return torch.zeros(nb, dtype=torch.uint8, device="cuda")  # zeroed once


def _run(loc, w, dagg, q, mode, planes=False, n_rows_max=None, n_q_max=None, scratch=None):
    """dpq f32 [n_q_max][hid] pre-filled with NaN (and the planes [3][n_q_max * hid]
    pre-filled with bf16 NaNs), counts on the device below the capacities"""
    import _native as nat
    n_rows, T = loc.shape
    U, hid = q.shape
    n_rows_max = n_rows_max or n_rows
    n_q_max = n_q_max or U
    if scratch is None:
        scratch = _scratch(n_rows_max, T, n_q_max, hid)
    n_rows_dev = torch.tensor([n_rows], dtype=torch.int32, device="cuda")
    n_q_dev = torch.tensor([U], dtype=torch.int32, device="cuda")
    dpq = torch.full((n_q_max, hid), float("nan"), device="cuda")
    pl = torch.full((3, n_q_max * hid), 0x7fc0, dtype=torch.int16, device="cuda") if planes else None
    rc = nat.lib().pinsage_agg_transpose(_vp(loc), _vp(w), _vp(n_rows_dev), n_rows_max, T, _vp(n_q_dev), n_q_max,
                                         _vp(dagg), dagg.shape[1], _vp(q), hid, mode, _vp(scratch), _vp(dpq),
                                         _vp(pl), n_q_max * hid, _stream())
    nat.check(rc, "agg_transpose")
    torch.cuda.synchronize()
    return pl.view(3, n_q_max, hid) if planes else dpq


def _ref(loc, w, dagg, q):
    """float64: the unmasked sums [U][hid], the sums of |w dagg|, lrelu'(q) in fp32"""
    n_rows, T = loc.shape
    U, hid = q.shape
    f = torch.arange(n_rows, device="cuda").repeat_interleave(T)
    terms = w.reshape(-1, 1).double() * dagg[:, :hid].double()[f]
    u = loc.reshape(-1).long()
    s = torch.zeros(U, hid, dtype=torch.float64, device="cuda").index_add_(0, u, terms)
    a = torch.zeros(U, hid, dtype=torch.float64, device="cuda").index_add_(0, u, terms.abs())
    slope = torch.where(q > 0, torch.ones_like(q), torch.full_like(q, float(SLOPE)))
    return s, a, slope


def _bits(x):
    return x.contiguous().view(torch.int32)


def _split_planes(x):
    """pinsage_split_planes of a contiguous fp32 matrix: int16 [3][rows][cols]"""
    import _native as nat
    R, C = x.shape
    out = torch.empty(3, R, C, dtype=torch.int16, device="cuda")
    nat.check(nat.lib().pinsage_split_planes(_vp(x), R, C, C, _vp(out), _stream()), "split_planes")
    torch.cuda.synchronize()
    return out


def _assert_exact(got, loc, w, dagg, q, counts, planes=False):
    """got (dpq, or its planes) holds, bitwise, the float64 sum cast to fp32 (exact
    by construction) times 1 or 0.01f on the rows that occur, and its
    pre-fill on the rows that occur in no slot and on the rows past the count"""
    s, _, slope = _ref(loc, w, dagg, q)
    assert float(s.abs().max()) < 2 ** 22 and bool((s * 4 == (s * 4).round()).all())  # exact in fp32
    expect = s.float() * slope
    U = q.shape[0]
    hit = torch.from_numpy(counts > 0).cuda()
    if planes:
        ref3 = _split_planes(expect)
        assert torch.equal(got[:, :U][:, hit], ref3[:, hit])
        assert bool((got[:, :U][:, ~hit] == 0x7fc0).all()) and bool((got[:, U:] == 0x7fc0).all())
        return
    assert torch.equal(_bits(got[:U][hit]), _bits(expect[hit]))
    assert bool(torch.isnan(got[:U][~hit]).all()) and bool(torch.isnan(got[U:]).all())


def _depth(counts, mode):
    """adds on the longest path of each row's documented summation order"""
    k = (counts + 15) // 16
    if mode == 1:
        levels = np.zeros_like(k)
        span = np.ones_like(k)
        while (span < k).any():
            levels += span < k
            span *= 8
        return 16 + 7 * levels
    return np.where(k > 1, 16 + (k + 15) // 16 + 15, 16)


def _assert_bound(got, loc, w, dagg, q, counts, mode, what):
    """per row and per element: |gpu - f64| <= slope (D + 1) 2^-24 sum |w dagg|"""
    s, a, slope = _ref(loc, w, dagg, q)
    U = q.shape[0]
    hit = torch.from_numpy(counts > 0).cuda()
    assert bool(torch.isfinite(got[:U][hit]).all())
    assert bool(torch.isnan(got[:U][~hit]).all()) and bool(torch.isnan(got[U:]).all())
    D = torch.from_numpy(_depth(counts, mode).astype(np.float64)).cuda()[:, None]
    err = (got[:U].double() - s * slope.double()).abs()[hit]
    unit = (slope.double() * a * U24)[hit]
    ratio = err / unit.clamp_min(1e-300)
    worst = ratio.max(dim=1).values
    i = int(worst.argmax())
    print(f"dq {what} mode {mode}: worst err / (slope 2^-24 sum|w dagg|) = {float(worst[i]):.2f} on a row of "
          f"{int(counts[counts > 0][i])} occurrences (bound {float(D[hit][i]) + 1:.0f}); longest row "
          f"{float(worst[int(np.argmax(counts[counts > 0]))]):.2f}")
    assert bool((err <= (D[hit] + 1) * unit).all())


# ----------------------------------------------------------------------------- the main table
@pytest.mark.parametrize("extra_rows,extra_q", [(0, 0), (300, 1000), (13, 3000)])
@pytest.mark.parametrize("form", ["combine", "tree", "tree+planes"])
def test_exact_sums_every_row_length(form, extra_rows, extra_q):
    """All three output forms on the main table, hid 64, with the capacities at
    and above the device-side counts (U + 3000 > 4096: the two-launch scan
    over a set that would fit the one-block scan).  The planes form found the
    tree root's mask multiply contracted into the split."""
    counts, loc_np = _main_table()
    loc = torch.from_numpy(loc_np).cuda()
    n_rows, T = loc.shape
    U, hid = len(counts), 64
    w, dagg, q = _exact_inputs(n_rows, T, U, hid, hid, seed=5)
    got = _run(loc, w, dagg, q, mode=0 if form == "combine" else 1, planes=form == "tree+planes",
               n_rows_max=n_rows + extra_rows, n_q_max=U + extra_q)
    _assert_exact(got, loc, w, dagg, q, counts, planes=form == "tree+planes")


HIDS = [(4, 0), (4, 1), (16, 0), (16, 1), (128, 0), (128, 1), (256, 0), (256, 1), (260, 0), (260, 1), (384, 0),
        (384, 1), (512, 0), (512, 1), (516, 0), (768, 0), (1024, 0)]


@pytest.mark.parametrize("hid,mode", HIDS)
def test_hid_sweep_exact_and_random(hid, mode):
    """Every instantiation: VEC 1 / 2, one pass (hid / 4 <= 64 VEC) and the
    column-pass loop (mode 0 at 260 and 384: a partial second pass with VEC 1;
    516: a partial second pass with VEC 2; 768 and 1024: a half and a full second
    pass), the tree's two widths.  hid 260 reads dagg rows of stride 272."""
    counts, loc_np = _main_table()
    loc = torch.from_numpy(loc_np).cuda()
    n_rows, T = loc.shape
    U = len(counts)
    ld = 272 if hid == 260 else hid
    w, dagg, q = _exact_inputs(n_rows, T, U, hid, ld, seed=hid)
    _assert_exact(_run(loc, w, dagg, q, mode), loc, w, dagg, q, counts)
    w, dagg, q = _random_inputs(n_rows, T, U, hid, ld, seed=hid + 1)
    _assert_bound(_run(loc, w, dagg, q, mode), loc, w, dagg, q, counts, mode, f"hid {hid}")


@pytest.mark.parametrize("hid", [8, 16, 128, 256, 264, 384, 512])
def test_planes_are_the_split_of_the_tree_result(hid):
    """dpq_planes is bitwise pinsage_split_planes of the mode-1 fp32 result
    (random inputs; both tree widths and the deferred one-chunk stores)."""
    counts, loc_np = _main_table()
    loc = torch.from_numpy(loc_np).cuda()
    n_rows, T = loc.shape
    U = len(counts)
    w, dagg, q = _random_inputs(n_rows, T, U, hid, hid, seed=hid + 2)
    dpq = _run(loc, w, dagg, q, 1)
    pl = _run(loc, w, dagg, q, 1, planes=True)
    hit = torch.from_numpy(counts > 0).cuda()
    assert torch.equal(pl[:, hit], _split_planes(dpq)[:, hit])
    assert bool((pl[:, ~hit] == 0x7fc0).all())


# ----------------------------------------------------------------------------- the documented order
def _emulate(ws, xs, slope, mode):
    """fp32 restatement of one q row's sum: pairs in source-row order, chains
    of 16 fmas from 0 (w dyadic: the product is exact, so the fma is one
    correctly rounded fp32 add), then mode 1: the fan-in-8 tree in child order;
    mode 0: 16 strided wave sums (wave v: chunks v, v + 16, ...) added in wave
    order; then the mask."""
    hid = xs.shape[1]
    parts = []
    for c0 in range(0, len(ws), 16):
        acc = np.zeros(hid, np.float32)
        for j in range(c0, min(len(ws), c0 + 16)):
            acc = ws[j] * xs[j] + acc
        parts.append(acc)
    if len(parts) == 1:
        total = parts[0]
    elif mode == 1:
        nodes = parts
        while len(nodes) > 1:
            nxt = []
            for g in range(0, len(nodes), 8):
                acc = nodes[g]
                for x in nodes[g + 1:g + 8]:
                    acc = acc + x
                nxt.append(acc)
            nodes = nxt
        total = nodes[0]
    else:
        red = []
        for v in range(16):
            acc = np.zeros(hid, np.float32)
            for j in range(v, len(parts), 16):
                acc = acc + parts[j]
            red.append(acc)
        total = red[0]
        for v in range(1, 16):
            total = total + red[v]
    assert total.dtype == np.float32
    return total * slope


def test_documented_summation_order_bitwise_and_reruns_on_one_scratch():
    """Rows of 17, 129, 1025 and 8193 occurrences (and the one-chunk rows of 5
    and 16) equal the numpy fp32 emulation of the documented order in both
    modes: determinism pinned without depending on timing.  The four runs share
    one scratch, zeroed once: cnt and the tree's tickets reset themselves."""
    counts, loc_np = _main_table()
    loc = torch.from_numpy(loc_np).cuda()
    n_rows, T = loc.shape
    U, hid = len(counts), 16
    w, dagg, q = _random_inputs(n_rows, T, U, hid, hid, seed=77, dyadic_w=True)
    sc = _scratch(n_rows, T, U, hid)
    runs = [(m, _run(loc, w, dagg, q, m, scratch=sc)) for m in (0, 1, 1, 0)]
    hit = torch.from_numpy(counts > 0).cuda()
    assert torch.equal(_bits(runs[0][1][hit]), _bits(runs[3][1][hit]))
    assert torch.equal(_bits(runs[1][1][hit]), _bits(runs[2][1][hit]))
    w_np, x_np = w.cpu().numpy(), dagg.cpu().numpy()
    slope = _ref(loc, w, dagg, q)[2].cpu().numpy()
    for c in (5, 16, 17, 129, 1025, 8193):
        u = int(np.nonzero(counts == c)[0][0])
        f, t = np.nonzero(loc_np == u)  # row-major: ascending source row
        assert len(f) == c and (np.diff(f) > 0).all()
        for mode, got in runs[:2]:
            want = _emulate(w_np[f, t], x_np[f], slope[u], mode)
            assert np.array_equal(got[u].cpu().numpy().view(np.int32), want.view(np.int32)), (c, mode)


# ----------------------------------------------------------------------------- CSR and scan regimes
@pytest.mark.parametrize("U,ranges", [(1023, None), (1024, None), (1025, None), (2048, None), (4096, None),
                                      (4097, None), (40960, None), (40961, None), (40961, "0")])
def test_q_row_counts_through_every_csr_and_scan_regime(U, ranges, monkeypatch):
    """scan_small_kernel below, at and above 1024 per thread-run boundaries
    (U == 1024 per: the totals written by thread 1023) up to 4096 rows, the
    two-launch scan from 4097; one range of LDS histogram slices up to 40960 q
    rows, two (range, slice) ranges at 40961, and the per-wave global atomics there with
    PINSAGE_CSR_RANGES=0 (read per call).  hid 16, exact sums, both modes."""
    if ranges is not None:
        monkeypatch.setenv("PINSAGE_CSR_RANGES", ranges)
    counts, loc_np = _regime_table(U)
    loc = torch.from_numpy(loc_np).cuda()
    n_rows, T = loc.shape
    w, dagg, q = _exact_inputs(n_rows, T, U, 16, 16, seed=U)
    for mode in (0, 1):
        _assert_exact(_run(loc, w, dagg, q, mode), loc, w, dagg, q, counts)


def test_bitmap_sort_across_two_windows():
    """A q row of 70 occurrences whose source rows span 0 .. 524288 + 63: the
    bitmap rank's second window (windows of 524288 source rows).  T = 1, hid 8,
    exact sums; with T = 1 any assignment of slots to source rows keeps the
    pairs distinct, so the long row's slots are spread by swapping rows."""
    n_rows = 524288 + 64
    counts = np.asarray([70] + _pad_counts(n_rows - 70, cycle=(16, 15, 14, 13)), np.int64)
    loc_np = _build_loc(counts, 1, seed=9)
    for k in range(1, 70):
        fk = (k * (n_rows - 1)) // 69
        loc_np[[k, fk]] = loc_np[[fk, k]]
    _check_loc(loc_np, counts)
    f = np.nonzero(loc_np[:, 0] == 0)[0]
    assert len(f) == 70 and f[0] == 0 and f[-1] == n_rows - 1 and f[-1] - f[0] >= 524288
    loc = torch.from_numpy(loc_np).cuda()
    U = len(counts)
    w, dagg, q = _exact_inputs(n_rows, 1, U, 8, 8, seed=10)
    for mode in (0, 1):
        _assert_exact(_run(loc, w, dagg, q, mode), loc, w, dagg, q, counts)


# ----------------------------------------------------------------------------- arguments
def test_rejected_arguments_launch_nothing():
    import _native as nat
    L = nat.lib()
    n_rows, T, U = 8, 3, 12
    loc = torch.from_numpy(_build_loc([2] * U, T, seed=0)).cuda()
    w = torch.ones(n_rows, T, device="cuda")
    cnt = torch.tensor([n_rows, U], dtype=torch.int32, device="cuda")
    n_rows_dev, n_q_dev = cnt[0:1], cnt[1:2]
    big = 1024
    dagg = torch.ones(n_rows, big, device="cuda")
    q = torch.ones(U, big, device="cuda")
    dpq = torch.full((U, big), float("nan"), device="cuda")
    pl = torch.full((3, U * big), 0x7fc0, dtype=torch.int16, device="cuda")
    sc = torch.zeros(L.pinsage_agg_transpose_scratch_bytes(n_rows, T, U, big), dtype=torch.uint8, device="cuda")

    def call(hid=16, T_=T, mode=0, ld=big, planes=None, ps=U * big, scratch=sc, rows_max=n_rows, q_max=U):
        return L.pinsage_agg_transpose(_vp(loc), _vp(w), _vp(n_rows_dev), rows_max, T_, _vp(n_q_dev), q_max,
                                       _vp(dagg), ld, _vp(q), hid, mode, _vp(scratch), _vp(dpq), _vp(planes), ps,
                                       _stream())

    bad = [dict(hid=6), dict(hid=0), dict(T_=0), dict(T_=65), dict(mode=2), dict(mode=-1),
           dict(mode=1, hid=516), dict(mode=0, planes=pl), dict(mode=1, hid=516, planes=pl),
           dict(mode=1, planes=pl, ps=U * 16 - 4), dict(mode=1, planes=pl, ps=U * 16 + 2),
           dict(hid=16, ld=12), dict(hid=16, ld=18), dict(scratch=None), dict(rows_max=0), dict(q_max=0)]
    for kw in bad:
        assert call(**kw) == -2, kw
        assert L.pinsage_last_error()
    for args in [(n_rows, T, U, 6), (n_rows, 0, U, 16), (n_rows, 65, U, 16), (0, T, U, 16), (n_rows, T, 0, 16)]:
        assert L.pinsage_agg_transpose_scratch_bytes(*args) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(dpq).all()) and bool((pl == 0x7fc0).all())
    assert call(hid=16, mode=1, planes=pl, ps=U * 16) == 0  # the same call, valid
    torch.cuda.synchronize()
