"""Train-step parity helpers shared by the GPU tests.

The reference's hinge (``max_margin_loss``, pinsage_training.py:31-41, margin
1e-5 at :149) is evaluated on nearly collapsed embeddings at initialisation:
the argument ``cos(q,n) - cos(q,p) + margin`` of many triples is within fp32
rounding of 0, so a triple can be active on one side and not on the other,
and the loss gradient (a difference of nearly equal unit vectors) amplifies
rounding-level forward differences.  The step is therefore pinned in parts,
each one well conditioned:

1. forward rows the loss read (the engine's Z) vs the oracle's outputs,
   row-norm relative;
2. hinge arguments: the engine's per-triple value (written by its loss kernel)
   vs the oracle's; a triple whose activity differs must have |arg| <= 1e-6;
3. loss within 1e-4 relative, plus what the hinge arguments' own fp32 error
   (|arg| <= 1e-5 absolute) contributes to their clamped mean;
4. (A) the oracle's gradient over the GPU's active set, with the oracle's own
   forward, vs the GPU's gradients;
5. (B) the oracle's backward driven by the cotangent of the GPU's own outputs
   (the loss derivative evaluated on Z in f64, GPU active set) vs the GPU's
   gradients -- the kernels' backward measured with the conditioning removed.
   Every parameter gradient is a sum over rows (and slots) of the products of
   a projection's output gradient and its input; where those terms cancel
   (the head's bias at the reference init: its sum is ~1e-3 of its terms), an
   fp32 sum's rounding is relative to the terms, not to the result.  So part
   B's error is measured componentwise (cond_grads): |gpu - ref| over the sum
   of the terms' absolute values, ||.||-normed -- equal to the norm-relative
   error wherever nothing cancels -- and held to the north star's 1e-4.

Tolerances are stated per call (north star: 1e-4 relative on fp32).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from conftest import PKG, REPO

for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


class taps:
    """Record the oracle's projections while its forward runs (oracle._TAPS)."""

    def __enter__(self):
        from oracle import oracle as orc
        self.orc = orc
        orc._TAPS = self.rec = []
        return self.rec

    def __exit__(self, *a):
        self.orc._TAPS = None


def cond_grads(loss, p, keys, rec):
    """Gradients of `loss` w.r.t. p[k] for k in keys (None where unused) and,
    per parameter, the sum of the absolute values of the terms each gradient
    element sums: |dY|^T |X| for a projection's weight, sum |dY| for its bias
    (rec: the taps of the forward that built `loss`, over every call)."""
    outs = [t[3] for t in rec]
    g = torch.autograd.grad(loss, [p[k] for k in keys] + outs, retain_graph=True, allow_unused=True)
    grads = dict(zip(keys, g[:len(keys)]))
    scale = {k: np.zeros(tuple(p[k].shape)) for k in keys}
    for (wk, bk, x, _), dy in zip(rec, g[len(keys):]):
        if dy is None:
            continue
        ady = dy.detach().double().abs().reshape(-1, dy.shape[-1])
        ax = x.double().abs().reshape(-1, x.shape[-1])
        if wk in scale:
            scale[wk] += (ady.t() @ ax).numpy()
        if bk and bk in scale:
            scale[bk] += ady.sum(0).numpy()
    return grads, scale


def cond_rel(a, ref, scale):
    """||a - ref|| / ||scale||, scale = the summed terms' absolute values
    (>= |ref| elementwise): the componentwise error of a sum in fp32."""
    a, ref, scale = (np.asarray(x, np.float64) for x in (a, ref, scale))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(scale), 1e-30))


def make_trainer(g, n, feats, pos, L, T, B, margin, seed=0, spread=False):
    """PinSage with the reference's defaults except the BASELINE config's
    (n_layers, T, batch); the model is rebuilt after construction because the
    reference binds hyperparameters at construction (pinsage_training.py:139-148)."""
    import pinsage_model as pm
    import pinsage_training as pt
    torch.manual_seed(seed)
    tr = pt.PinSage(g, n, feats, pos, log=False, load_save=False)
    tr.T, tr.n_layers = T, L
    torch.manual_seed(seed + 1)
    tr.model = pm.PinSageModel(g, tr.n, L, tr.dimensions, tr.n_hops, tr.alpha, T, tr.nbhds)
    if spread:
        with torch.no_grad():
            for k, prm in tr.model.named_parameters():
                prm.zero_() if k.endswith("bias") else prm.mul_(3.0)
    tr.optimizer = torch.optim.Adam(tr.model.parameters(), lr=tr.lr)
    tr.scheduler = torch.optim.lr_scheduler.ExponentialLR(tr.optimizer, tr.decay)
    tr.batch_size = B
    tr.margin = margin
    return tr


def step_outputs(tr, B):
    """(Z [B, 3, out] f64, hinge [B] f64) of the last train_batch: the model
    rows its loss kernel read and that kernel's per-triple hinge argument."""
    import _native as nat
    fs = tr._fused
    e = fs.runner.engine
    ws = fs.ws
    out_dim = int(e.cfg.out)
    z = torch.empty((3 * B, out_dim), dtype=torch.float32, device=ws.device)
    nat.check(nat.lib().pinsage_engine_gather_output(e.h, nat.ptr(ws), 3 * B, nat.ptr(z),
                                                     nat.stream_ptr()), "gather")
    hinge = e.view(ws, int(e.off.hinge), torch.float32, B)
    torch.cuda.synchronize()
    return (z.view(B, 3, out_dim).cpu().double().numpy(), hinge.cpu().double().numpy())


def _hinge_args(hq, hp, hn, margin):
    hq, hp, hn = (F.normalize(x, dim=1) for x in (hq, hp, hn))
    return (hq * hn).sum(1) - (hq * hp).sum(1) + margin


def capture_step(tr, batch, run=None):
    """Run tr.train_batch(batch) (or run(batch)); return what the oracle needs
    to pin it: the parameters before the step, the batch, the GPU's gradients,
    loss, output rows (Z) and hinge arguments, and the step's return value."""
    b = np.asarray(batch.numpy() if torch.is_tensor(batch) else batch)
    init = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    out = (run or tr.train_batch)(torch.from_numpy(b))
    loss = out[0]
    grads = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in tr.model.named_parameters()}
    Z, hinge = step_outputs(tr, b.shape[0])
    return dict(init=init, batch=b, grads=grads, loss=float(loss), Z=Z, hinge=hinge,
                L=tr.n_layers, T=tr.T, margin=float(tr.margin), out_dim=tr.out_dim, out=out)


# norm-relative bound on every part-B gradient (check_record): a backward bug
# (a missing term, a sign) gives O(1); the reference-init conditioning of
# parameters whose terms cancel (head bias, layer biases) stays orders below
# (the measured values: DESIGN.md §4, round 6)
NORMREL_B = 1e-2


def check_train_step(tr, feats, w, nb, batch, tol=1e-4, kink=1e-6, strict_a=True, report=None,
                     tol_b=None):
    """Run tr.train_batch(batch) and pin it against the oracle in the five parts
    above.  Returns a dict of the measured errors (also appended to `report`)."""
    return check_record(capture_step(tr, batch), feats, w, nb, tol=tol, kink=kink, strict_a=strict_a,
                        report=report, tol_b=tol_b)


def check_record(rec, feats, w, nb, tol=1e-4, kink=1e-6, strict_a=True, report=None, tol_b=None):
    from oracle import oracle as orc
    L, T, margin, out_dim = rec["L"], rec["T"], rec["margin"], rec["out_dim"]
    init, b, gpu_grads, loss, Z, hinge = (rec[k] for k in ("init", "batch", "grads", "loss", "Z", "hinge"))
    B = b.shape[0]
    feats_cpu = feats.detach().cpu()
    wn, nbn = np.asarray(w), np.asarray(nb)
    p = {k: v.float().requires_grad_() for k, v in init.items()}
    with taps() as rec_taps:
        hs = [orc.model_forward(p, feats_cpu, b[:, c], L, T, wn, nbn, out_dim) for c in range(3)]
    res = {}
    # 1. forward rows, row-norm relative
    ref_rows = np.stack([h.detach().double().numpy() for h in hs], 1)  # [B, 3, out]
    row_err = np.linalg.norm(Z - ref_rows, axis=2) / np.maximum(np.linalg.norm(ref_rows, axis=2), 1e-30)
    res["fwd_row_rel_max"] = float(row_err.max())
    # 2. hinge arguments and activity
    args_ref = _hinge_args(*(torch.from_numpy(ref_rows[:, c]) for c in range(3)), margin).numpy()
    act_gpu, act_ref = hinge >= 0, args_ref >= 0
    flip = act_gpu != act_ref
    res["hinge_abs_max"] = float(np.abs(hinge - args_ref).max())
    res["hinge_flips"] = int(flip.sum())
    res["hinge_flip_arg_max"] = float(np.abs(args_ref[flip]).max()) if flip.any() else 0.0
    res["active"] = int(act_gpu.sum())
    # 3. loss
    ref_loss = float(np.clip(args_ref, 0, None).mean())
    res["loss_gpu"], res["loss_ref"] = loss, ref_loss
    res["loss_rel"] = abs(loss - ref_loss) / max(abs(ref_loss), 1e-30)
    # 4. (A) oracle forward, GPU active set
    mask = torch.from_numpy(act_gpu.astype(np.float32))
    lossA = (mask * _hinge_args(hs[0], hs[1], hs[2], margin)).sum() / B
    gA = torch.autograd.grad(lossA, [p[k] for k in init], retain_graph=True, allow_unused=True)
    # 5. (B) cotangent of the GPU's own outputs (f64), GPU active set
    zt = torch.from_numpy(Z.copy()).requires_grad_()
    lz = (mask.double() * _hinge_args(zt[:, 0], zt[:, 1], zt[:, 2], margin)).sum() / B
    (dz,) = torch.autograd.grad(lz, [zt])
    dz = dz.float()
    lossB = sum((hs[c] * dz[:, c]).sum() for c in range(3))
    gBd, sB = cond_grads(lossB, p, list(init), rec_taps)
    errA, errB, errBn = {}, {}, {}
    for k, ga in zip(init, gA):
        if k not in gpu_grads:
            continue
        gb = gBd[k]
        ga = np.zeros(init[k].shape) if ga is None else ga.double().numpy()
        gb = np.zeros(init[k].shape) if gb is None else gb.double().numpy()
        errA[k] = rel(gpu_grads[k], ga) if np.linalg.norm(ga) > 0 else float(np.linalg.norm(gpu_grads[k]))
        errB[k] = cond_rel(gpu_grads[k], gb, sB[k]) if np.linalg.norm(sB[k]) > 0 else float(
            np.linalg.norm(gpu_grads[k]))
        errBn[k] = rel(gpu_grads[k], gb) if np.linalg.norm(gb) > 0 else float(np.linalg.norm(gpu_grads[k]))
    res["grad_rel_A_max"] = max(errA.values())
    res["grad_rel_B_max"] = max(errB.values())
    res["grad_normrel_B_max"] = max(errBn.values())  # (reported: the norm-relative form)
    res["grad_rel_A"], res["grad_rel_B"] = errA, errB
    if report is not None:
        report.append(res)
    print({k: v for k, v in res.items() if not isinstance(v, dict)}, flush=True)
    # the assertions
    assert res["fwd_row_rel_max"] <= tol, res
    assert res["hinge_flip_arg_max"] <= kink, res
    # the hinge arguments are differences of cosines of unit rows (O(1) values):
    # fp32 holds them to a few 1e-7 absolute
    assert res["hinge_abs_max"] <= 1e-5, res
    # the loss is their clamped mean: at the reference's margin it is ~1e-5, a
    # cancellation of O(1) cosines, so its error is bounded by the arguments'
    # (mean absolute error over the active triples), not by 1e-4 of itself
    assert abs(loss - ref_loss) <= tol * abs(ref_loss) + (kink * res["hinge_flips"]
                                                           + res["hinge_abs_max"] * res["active"]) / B, res
    assert res["grad_rel_B_max"] <= (tol if tol_b is None else tol_b), res
    # the componentwise bound above cannot see an error that is small against
    # the summed terms' magnitudes but large against a parameter's gradient
    # whose terms cancel (e.g. a bias); the norm-relative error catches such a
    # backward bug (a missing term or sign shows as O(1)).  Bound: NORMREL_B
    # (documented looser bound: conditioning alone stays orders below it)
    assert res["grad_normrel_B_max"] <= NORMREL_B, res
    if strict_a:
        assert res["grad_rel_A_max"] <= tol, res
    return res


def fixed_cotangent_check(model, feats, ids, w, nb, L, T, seed=0, tol=1e-4, cond=False):
    """The autograd path (PinSageModel forward + HIP backward) under a fixed
    random cotangent vs the oracle's forward/backward with the same cotangent:
    output rows and every parameter gradient, norm-relative (cond: gradients
    componentwise, cond_rel -- for calls of thousands of ids, whose random
    cotangents cancel over the rows)."""
    from oracle import oracle as orc
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(seed)
    c = torch.from_numpy(rng.standard_normal((len(ids), model.out_dim)).astype(np.float32))
    for prm in model.parameters():
        prm.grad = None
    y = model(feats.cuda(), torch.from_numpy(np.asarray(ids, np.int64)))
    (y * c.cuda()).sum().backward()
    p = {k: v.float().requires_grad_() for k, v in init.items()}
    with taps() as rec:
        yr = orc.model_forward(p, feats.detach().cpu(), np.asarray(ids, np.int64), L, T, np.asarray(w),
                               np.asarray(nb), model.out_dim)
    if cond:
        gr, sc = cond_grads((yr * c).sum(), p, list(init), rec)
        errs = {k: cond_rel(prm.grad.cpu().numpy(), gr[k].numpy(), sc[k]) for k, prm in model.named_parameters()}
    else:
        (yr * c).sum().backward()
        errs = {k: rel(prm.grad.cpu().numpy(), p[k].grad.numpy()) for k, prm in model.named_parameters()}
    fwd = rel(y.detach().cpu().numpy(), yr.detach().numpy())
    print(f"L={L} T={T} fwd={fwd:.2e} grad max={max(errs.values()):.2e}", flush=True)
    assert fwd <= tol, fwd
    assert max(errs.values()) <= tol, errs
    return fwd, errs


# ----------------------------------------------------------------------------- frontier plan
# The integer plan pinsage_engine_frontier builds (tests/test_gpu_frontier_plan.py
# reads it from a workspace; tests/test_host.py checks that the comparison can
# fail).  A plan is a dict:
#   layers[l]  count_S, count_N (the device-side counts), S, N (sorted member
#              lists up to their count), loc / wloc [|S|][T] (wloc as uint32
#              bits), self_src [|S|], q_src [|N|]            -- l = 0 is the bottom
#   read_counts  (|S_l| list, |N_l| list) as pinsage_engine_read_counts gives them
#   pos_rank [n_pos]; rank_off [|S_top| + 1] (or [-1]: position CSR absent,
#   more than POS_CSR_MAX positions); pos_sorted [n_pos]
POS_CSR_MAX = 16384  # kPosCsrMax (conv.hip)
PLAN_LAYER_FIELDS = ("count_S", "S", "count_N", "N", "loc", "wloc", "self_src", "q_src")


def frontier_plan_reference(ids, rows, n_layers, T, virtual=None):
    """The plan in int64 numpy, top down, from the ids and the table rows of the
    reference's own sets only: rows(l, S) -> (nb[S, :T] as int64, wn[S, :T] as
    uint32 bits) of layer l's table.  virtual = (x0, n_x): the ids x0 .. x0 +
    n_x - 1 join the top set (pinsage_engine_set_fly)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    top = ids if not virtual else np.concatenate([ids, np.arange(virtual[0], virtual[0] + virtual[1], dtype=np.int64)])
    S = np.unique(top)
    layers = [None] * n_layers
    for l in range(n_layers - 1, -1, -1):
        nb, w = rows(l, S)
        nb = np.asarray(nb, np.int64).reshape(len(S), T)
        N = np.unique(nb)
        layers[l] = {"count_S": len(S), "S": S, "count_N": len(N), "N": N,
                     "loc": np.searchsorted(N, nb), "wloc": np.asarray(w, np.uint32).reshape(len(S), T)}
        S = np.unique(np.concatenate([N, S]))
    for l, lay in enumerate(layers):
        below = layers[l - 1]["S"] if l else None
        for dst, src in (("self_src", "S"), ("q_src", "N")):
            lay[dst] = np.searchsorted(below, lay[src]) if l else lay[src].copy()
    S_top = layers[-1]["S"]
    pos_rank = np.searchsorted(S_top, ids)
    plan = {"layers": layers, "pos_rank": pos_rank,
            "read_counts": ([lay["count_S"] for lay in layers], [lay["count_N"] for lay in layers])}
    if len(ids) > POS_CSR_MAX:
        plan["rank_off"] = np.array([-1], np.int64)
        plan["pos_sorted"] = None
    else:
        order = np.argsort(pos_rank, kind="stable")
        plan["pos_sorted"] = order.astype(np.int64)
        plan["rank_off"] = np.searchsorted(pos_rank[order], np.arange(len(S_top) + 1), side="left")
    return plan


def _plan_field(where, field, got, want):
    got = np.asarray(got)
    want = np.asarray(want)
    if got.dtype.kind == "f" or want.dtype.kind == "f":
        raise AssertionError(f"{where} {field}: compare floats as bits")
    g = got.astype(np.int64).reshape(-1)
    w = want.astype(np.int64).reshape(-1)
    if field == "wloc":  # bit patterns: int32 and uint32 views of one word are equal
        g, w = g & 0xFFFFFFFF, w & 0xFFFFFFFF
    if g.shape != w.shape:
        raise AssertionError(f"{where} {field}: {g.shape[0]} entries, reference has {w.shape[0]}")
    bad = np.flatnonzero(g != w)
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{where} {field}: {len(bad)} of {len(w)} entries differ, first at [{i}]: "
                             f"got {int(g[i])} (0x{int(g[i]) & 0xffffffff:08x}), "
                             f"reference {int(w[i])} (0x{int(w[i]) & 0xffffffff:08x})")


def check_frontier_plan(got, want):
    """Exact, element for element (wloc bit for bit); the first difference,
    top down, raises an AssertionError naming the layer and the field."""
    L = len(want["layers"])
    if len(got["layers"]) != L:
        raise AssertionError(f"plan: {len(got['layers'])} layers, reference has {L}")
    for l in range(L - 1, -1, -1):
        for f in PLAN_LAYER_FIELDS:
            _plan_field(f"layer {l}", f, got["layers"][l][f], want["layers"][l][f])
    for k, name in ((0, "S"), (1, "N")):
        _plan_field("all layers", f"read_counts {name}", got["read_counts"][k], want["read_counts"][k])
    _plan_field("positions", "pos_rank", got["pos_rank"], want["pos_rank"])
    if int(np.asarray(want["rank_off"]).reshape(-1)[0]) == -1:  # absent: only the mark is defined
        _plan_field("positions", "rank_off", np.asarray(got["rank_off"]).reshape(-1)[:1], [-1])
        return
    _plan_field("positions", "rank_off", got["rank_off"], want["rank_off"])
    _plan_field("positions", "pos_sorted", got["pos_sorted"], want["pos_sorted"])


# ----------------------------------------------------------------------------- cosine kNN selection
# pinsage_knn_cosine's per-row selection (knn_select_kernel, csrc/knn.hip) on
# tables whose similarities are exact in fp32 (tests/test_gpu_knn_select.py
# compares ids and value bits; tests/test_host.py checks that every case
# reaches the exit it was built for and that the comparison can fail).
#
# Rows are (x_j, KNN_Y, 0, ..., 0) with integer x_j, d = 16, plus the probe
# rows (1, 0, ...), (-1, 0, ...), (2, 0, ...) and an all-zero row; queries are
# probe rows only.  Each dot product then has one non-zero term, an integer
# below 2^24 (exact in the fp32 MFMA chain and in the split-bf16 products: a
# 15-bit integer is its hi + mid planes, a probe a single hi value), the norms
# are float32(sqrt(an exact double)), and |q| |e_j| + eps is |e_j|, 2 |e_j| or
# eps: each similarity is one IEEE fp32 division.
KNN_SAMPLE = 4096    # kKnnSample (knn.hip): leading keys that set the candidate threshold
KNN_SEG = 512        # kKnnSeg: candidate slots per wave
KNN_WAVES = 16       # kKnnBlock / 64: waves of the selection's workgroup
KNN_MAX_SORT = 4096  # kKnnMaxK: most keys the in-LDS sort takes
KNN_BLOCK = 64 * KNN_WAVES
KNN_D = 16
KNN_Y = 3000
KNN_PROBES = ("p1", "m1", "p2", "zero")  # their order at the end of a table
_PROBE_X = {"p1": 1.0, "m1": -1.0, "p2": 2.0, "zero": 0.0}


def knn_probe_table(x, n_probes=4, zero_rows=()):
    """(emb f32 [len(x) + n_probes][16], {probe name: row id}): the rows
    (x_j, KNN_Y, 0, ...) -- all-zero at the indices zero_rows -- then the first
    n_probes probe rows."""
    x = np.asarray(x, np.int64)
    assert np.abs(x).max(initial=0) <= 20000
    emb = np.zeros((len(x) + n_probes, KNN_D), np.float32)
    emb[:len(x), 0] = x
    emb[:len(x), 1] = KNN_Y
    emb[list(zero_rows)] = 0.0
    probes = {}
    for i, name in enumerate(KNN_PROBES[:n_probes]):
        emb[len(x) + i, 0] = _PROBE_X[name]
        probes[name] = len(x) + i
    emb.setflags(write=False)
    return emb, probes


def knn_select_reference(emb, q, k, eps=1e-16):
    """(sim f32 [nq][n], w f32 [nq][k], ids i64 [nq][k]) of pinsage_knn_cosine for
    a table built as above: sim = dot / fl(fl(|q| |e_j|) + eps) in fp32 from exact
    dots and norms, the k largest by (similarity descending, index ascending)."""
    emb = np.asarray(emb, np.float32)
    q = np.asarray(q, np.int64).reshape(-1)
    n = emb.shape[0]
    e = emb.astype(np.float64)
    dots = e[q] @ e.T
    # the premise: every dot is one integer product below 2^24 (no rounding in
    # either GEMM arithmetic), and the squared norms are integers a double holds
    assert ((e[q][:, None, :] * e[None, :, :]) != 0).sum(2).max(initial=0) <= 1
    assert np.array_equal(dots, np.rint(dots)) and np.abs(dots).max(initial=0) < 2 ** 24
    sq = (e * e).sum(1)
    assert np.array_equal(sq, np.rint(sq)) and sq.max() < 2 ** 53
    norms = np.sqrt(sq).astype(np.float32)
    den = norms[q][:, None] * norms[None, :] + np.float32(eps)  # two fp32 roundings
    assert den.dtype == np.float32
    sim = dots.astype(np.float32) / den + np.float32(0.0)      # -0.0 -> +0.0
    assert sim.dtype == np.float32 and np.isfinite(sim).all()
    cols = np.arange(n)
    order = np.stack([np.lexsort((cols, -s.astype(np.float64)))[:k] for s in sim]).reshape(len(q), k)
    w = np.take_along_axis(sim, order, 1)
    return sim, w, order.astype(np.int64)


def knn_key_image(sim_row):
    """f2key (knn.hip): the uint32 whose order is the float's."""
    u = np.ascontiguousarray(sim_row, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def knn_select_candidates(sim_row, k):
    """(key image, candidate mask, candidates per wave) of the kernel's one
    pass: the threshold is the r-th largest of the row's first KNN_SAMPLE keys."""
    key = knn_key_image(sim_row)
    n = len(key)
    assert 1 <= k <= min(n, KNN_MAX_SORT)
    S = min(n, KNN_SAMPLE)
    er = k * S / n
    r = k if S == n else int(min(S, 1.5 * er + 4.0 * np.sqrt(er) + 8.0))
    t = np.sort(key[:S])[::-1][r - 1]
    cand = key >= t
    j = np.arange(n)
    n16 = (n // 16) * 16 if n % 4 == 0 else 0
    wave = np.where(j < n16, (j % (16 * KNN_BLOCK)) // KNN_BLOCK, ((j - n16) % KNN_BLOCK) // 64)
    return key, cand, np.bincount(wave[cand], minlength=KNN_WAVES)


def knn_select_regime(sim_row, k):
    """The exit knn_select_kernel takes for one row of similarities, replayed:
    'fast' (one pass, candidates above a sampled threshold), or the whole-row
    radix select because a wave's segment overflowed ('segment'), fewer than k
    candidates were found ('few'), or more than KNN_MAX_SORT keys reach the
    k-th ('ties')."""
    key, cand, per_wave = knn_select_candidates(sim_row, k)
    if per_wave.max() > KNN_SEG:
        return "segment"
    if per_wave.sum() < k:
        return "few"
    kth = np.sort(key[cand])[::-1][k - 1]
    if int((key >= kth).sum()) > KNN_MAX_SORT:
        return "ties"
    return "fast"


def check_knn_select(w, ids, ref_w, ref_ids):
    """Exact: ids equal and values bit for bit.  The first differing (query,
    column) raises an AssertionError saying whether it is an order swap inside
    a tie, a missing id, or a value bit."""
    w = np.ascontiguousarray(w, np.float32)
    ref_w = np.ascontiguousarray(ref_w, np.float32)
    ids = np.asarray(ids, np.int64)
    ref_ids = np.asarray(ref_ids, np.int64)
    if w.shape != ref_w.shape or ids.shape != ref_ids.shape or w.shape != ids.shape:
        raise AssertionError(f"knn: shapes {w.shape} / {ids.shape}, reference {ref_w.shape} / {ref_ids.shape}")
    wb, rb = w.view(np.int32), ref_w.view(np.int32)
    bad = (ids != ref_ids) | (wb != rb)
    if not bad.any():
        return
    qi, c = (int(v) for v in np.argwhere(bad)[0])
    where = f"knn query {qi} column {c}: {int(bad.sum())} of {bad.size} entries differ, first here: "
    got, want = int(ids[qi, c]), int(ref_ids[qi, c])
    bits = f"value 0x{int(wb[qi, c]) & 0xffffffff:08x} ({w[qi, c]!r}), reference 0x{int(rb[qi, c]) & 0xffffffff:08x} ({ref_w[qi, c]!r})"
    if got == want:
        raise AssertionError(where + f"value bit: id {got}, " + bits)
    if set(ids[qi].tolist()) != set(ref_ids[qi].tolist()):
        lost = sorted(set(ref_ids[qi].tolist()) - set(ids[qi].tolist()))
        raise AssertionError(where + f"missing id: got id {got}, reference {want}; "
                             f"{len(lost)} reference ids absent from the row, first {lost[0]}; " + bits)
    if wb[qi, c] == rb[qi, c]:
        raise AssertionError(where + f"order swap inside a tie: got id {got}, reference {want}, both rows "
                             f"hold the same ids; " + bits)
    raise AssertionError(where + f"order: got id {got}, reference {want}, the same ids in another order; " + bits)


KNN_ATOL = 2e-6  # float tables: the reference's sgemm and the MFMA chain differ in the last bits


def knn_sims64(emb, q, idx):
    e = emb.astype(np.float64)
    nrm = np.sqrt((e * e).sum(1))
    a = e[q]
    b = e[idx]  # [nq, k, d]
    dot = np.einsum("qd,qkd->qk", a, b)
    return dot / (nrm[q][:, None] * nrm[idx] + 1e-16)


def check_knn_close(w, n, rw, rn, emb, q):
    """For float tables, whose similarities are not exact: (a) sorted values
    agree with the reference's within KNN_ATOL, (b) each of our
    neighbours really has the similarity reported for it, (c) no neighbour twice
    in a row.  Together: ids differ from the reference only between
    similarities that tie within the tolerance (including the column the
    reference drops as 'self', which may be a duplicate row's)."""
    w, n, rw, rn = (np.asarray(x) for x in (w, n, rw, rn))
    assert w.shape == rw.shape and n.shape == rn.shape
    if w.size == 0:
        return 0.0
    assert np.abs(w - rw).max() <= KNN_ATOL                         # (a)
    assert np.abs(knn_sims64(emb, q, n) - w).max() <= KNN_ATOL      # (b)
    assert (np.diff(w, axis=1) <= 0).all()                           # sorted descending
    s = np.sort(n, 1)
    assert (np.diff(s, axis=1) > 0).all()                            # (c)
    return float((n != rn).mean())


def _knn_x_random(nb, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(np.arange(-10000, 9999))[:nb] if nb <= 19999 else rng.integers(-10000, 9999, nb)


def _knn_x_desc(nb):
    return 9998 - np.arange(nb)


_KNN_TABLES = {}


def knn_select_table(name):
    """The shared tables of the selection cases, built once (read-only):
    (emb, probes)."""
    if name in _KNN_TABLES:
        return _KNN_TABLES[name]
    kind, _, arg = name.partition(":")
    n = int(arg) if arg else 20000
    n_probes = min(n, 4)
    nb = n - n_probes
    zero_rows = ()
    if kind == "random":
        x = _knn_x_random(nb, 100 + n)
    elif kind == "desc":
        x = _knn_x_desc(nb)
    elif kind == "block":      # the 600 largest x contiguous in one wave's 1024-block
        x = _knn_x_random(nb, 3)
        top = np.argsort(-x, kind="stable")[:600]
        rest = np.setdiff1d(np.arange(nb), top)
        dst = np.arange(5120, 5720)
        out = np.empty_like(x)
        out[dst] = x[top]
        out[np.setdiff1d(np.arange(nb), dst)] = x[rest]
        x = out
    elif kind == "third":      # every third row the same, largest, value
        x = np.random.default_rng(4).integers(-10000, 9000, nb)
        x[::3] = 9000
    elif kind == "plateau":    # descending with 2500 equal values across the k-th rank
        x = _knn_x_desc(nb)
        x[800:3300] = x[800]
    elif kind == "scattered":  # 300 scattered rows share the value of rank ~900
        x = _knn_x_random(nb, 5)
        v = np.sort(x)[::-1][900]
        at = np.random.default_rng(6).choice(np.flatnonzero(x < v), 300, replace=False)
        x[at] = v
    elif kind == "signs":      # mostly negative, 50 positive, three all-zero rows
        rng = np.random.default_rng(7)
        x = -rng.integers(1, 20001, nb)
        at = rng.choice(nb, 53, replace=False)
        x[at[:50]] = rng.integers(1, 20001, 50)
        x[at[50:]] = 0
        zero_rows = tuple(int(i) for i in at[50:])
    else:
        raise KeyError(name)
    _KNN_TABLES[name] = knn_probe_table(x, n_probes, zero_rows)
    return _KNN_TABLES[name]


# (id, table, probe, k, exit): the regime cases.  exit None: whatever the
# replay reports (the shape cases); a name: the case was built for that exit.
KNN_REGIME_CASES = (
    [(f"random-k{k}", "random", "p1", k, "fast") for k in (1, 64, 65, 1000)] + [
        ("random-k4096", "random", "p1", 4096, "segment"),
        ("desc-k1000", "desc", "p1", 1000, "few"),
        ("asc-k1000", "desc", "m1", 1000, "segment"),
        ("block-k100", "block", "p1", 100, "segment"),
        ("third-k1000", "third:16384", "p1", 1000, "ties"),
        # k = 4096 with spare ties: one tie too many would be written past the sort's arrays
        ("third-k4096", "third:16384", "p1", 4096, "ties"),
        ("zeroquery-k1000", "random", "zero", 1000, "segment"),
        ("plateau-k1000", "plateau", "p1", 1000, "few"),
        ("plateau-k2000", "plateau", "p1", 2000, "segment"),  # the tie cut falls in the second chunk
        ("scattered-k1000", "scattered", "p1", 1000, "fast"),
        ("signs-k200", "signs", "p1", 200, "fast"),
        ("desc20001-k1000", "desc:20001", "p1", 1000, "few"),
        ("asc20001-k1000", "desc:20001", "m1", 1000, "segment"),
    ])
_KNN_SHAPE_EXITS = {(4096, 4096): "segment", (300, 300): "fast", (65, 65): "fast"}
KNN_SHAPE_CASES = [
    (f"n{n}-k{k}", f"random:{n}", "p1", k, _KNN_SHAPE_EXITS.get((n, k)))
    for n in (1, 65, 300, 4096, 4097, 4100, 20001, 20003)
    for k in sorted({1, min(n, 500)} | ({n} if n <= 4096 else set()))]
KNN_SELECT_CASES = KNN_REGIME_CASES + KNN_SHAPE_CASES


def knn_select_case(case):
    """(emb, probes, query ids, k, sim, ref_w, ref_ids) of one case; asserts the
    reference's premise and that the row takes the exit the case names."""
    _, table, probe, k, want = case
    emb, probes = knn_select_table(table)
    q = np.array([probes[probe]], np.int64)
    sim, ref_w, ref_ids = knn_select_reference(emb, q, k)
    got = knn_select_regime(sim[0], k)
    assert want is None or got == want, f"{case[0]}: built for the '{want}' exit, the kernel's logic takes '{got}'"
    return emb, probes, q, k, sim, ref_w, ref_ids
