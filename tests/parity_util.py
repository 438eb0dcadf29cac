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


# ----------------------------------------------------------------------------- small tables
def perm_table(n, T, ld, seed, device="cuda"):
    """small universes: nb[i][t] = (p[i] + t) % n over a random permutation p
    (every column is a permutation: a frontier over all rows is the universe);
    wn: random 32-bit patterns (int32; the engine copies them as they are)"""
    assert T <= n
    rng = np.random.default_rng(seed)
    p = rng.permutation(n)
    nb = (p[:, None] + np.arange(ld)[None, :]) % n
    wb = rng.integers(0, 1 << 32, (n, ld), dtype=np.uint64).astype(np.uint32).view(np.int32)
    return torch.from_numpy(nb.astype(np.int32)).to(device), torch.from_numpy(wb).to(device)


# ----------------------------------------------------------------------------- loss and head
# The end of the train step (tests/test_gpu_head_loss.py): the loss kernels of
# conv.hip (loss_triple_kernel, det_put, rep_sum_kernel, loss_monitor_kernel,
# dout_accum_kernel, dz_scale_kernel), the head kernels of head.hip and the
# head inside the top layer's tile (aggw.hip), each against float64 numpy that
# reads only the inputs of the stage it checks.  tests/test_host.py pins the
# loss reference to torch autograd of max_margin_loss, checks that every case
# of the table has the multiplicities it claims and a hinge argument away from
# zero, and that each checker rejects a single planted defect.
U24 = 2.0 ** -24          # fp32 unit roundoff
HL_N, HL_T = 300, 3       # universe and neighbourhood size of every case
SLOPE = 0.01              # leaky_relu's negative slope (kSlope, common.h)
HINGE_ATOL = 1e-5         # the hinge argument's own fp32 error (this module's part 3)
COT_RTOL = 1e-5           # cotangent rows (test_triplet_loss_kernel_matches_torch)
ARG_MIN = 1e-4            # every case: |hinge argument| >= this, planted ties apart


def _normalize64(x):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def loss_reference(Z_by_rank, pos_rank, B, margin, feats=None, batch=None):
    """max_margin_loss over the batch positions p = 3 b + c (c = query /
    positive / negative) whose output row is Z_by_rank[pos_rank[p]], in float64:

      arg [B]        cos(q, n) - cos(q, p) + margin, rows normalised with
                     max(|x|, 1e-12) as F.normalize does
      active [B]     arg >= 0 (a tie is active: the kernel's rule, and what
                     clamp(min=0)'s backward gives)
      loss           mean of the active arguments
      cot [3B][d]    d loss / d (the un-normalised row of position p); zero
                     rows for inactive triples
      cot_scale [3B] |g_hat| / |x|: cot = (g_hat - x_hat (x_hat . g_hat)) / |x| is a
                     difference of two vectors no longer than the gradient g_hat
                     of the normalised row, so its fp32 rounding is relative to
                     that length, not to the difference (all ids equal: cot = 0)
      K [3][R]       number of positions of call c with rank r
      Gsum [3][R][d] sum of cot over those positions; Gscale, Gterms [3][R]: the
                     sums of cot_scale and of |cot| rows over them
      dZ [R][d]      sum_c K[c][r] Gsum[c][r] (put_embeddings' index_put backward
                     hands every position of a repeated id the sum)
      nfl, var       oracle.triplet_monitors' formulas; sumsq = sum |h_q|^2 over
                     the raw query rows (feats / batch None: nfl = None)"""
    Z = np.asarray(Z_by_rank, np.float64)
    pr = np.asarray(pos_rank, np.int64).reshape(B, 3)
    R, d = Z.shape
    x = Z[pr]                                              # [B][3][d]
    nrm = np.maximum(np.linalg.norm(x, axis=2), 1e-12)     # [B][3]
    h = x / nrm[:, :, None]
    arg = (h[:, 0] * h[:, 2]).sum(1) - (h[:, 0] * h[:, 1]).sum(1) + margin
    active = arg >= 0
    g = np.where(active, 1.0 / B, 0.0)[:, None]
    ghat = np.stack([g * (h[:, 2] - h[:, 1]), -g * h[:, 0], g * h[:, 0]], 1)
    cot = (ghat - h * (h * ghat).sum(2, keepdims=True)) / nrm[:, :, None]
    cot_scale = np.linalg.norm(ghat, axis=2) / nrm
    K = np.zeros((3, R), np.int64)
    Gsum = np.zeros((3, R, d))
    Gscale = np.zeros((3, R))
    Gterms = np.zeros((3, R))
    for c in range(3):
        np.add.at(K[c], pr[:, c], 1)
        np.add.at(Gsum[c], pr[:, c], cot[:, c])
        np.add.at(Gscale[c], pr[:, c], cot_scale[:, c])
        np.add.at(Gterms[c], pr[:, c], np.linalg.norm(cot[:, c], axis=1))
    hq = x[:, 0]
    out = dict(arg=arg, active=active, loss=float(np.where(active, arg, 0.0).sum() / B),
               cot=cot.reshape(3 * B, d), cot_scale=cot_scale.reshape(3 * B), K=K, Gsum=Gsum, Gscale=Gscale,
               Gterms=Gterms, dZ=(K[:, :, None] * Gsum).sum(0), sumsq=float((hq * hq).sum()),
               var=float(((hq - hq.mean(0)) ** 2).sum() / (B - 1)), mean_sq=float((hq.mean(0) ** 2).sum()),
               nfl=None, pos_rank=pr.reshape(-1), B=B)
    if feats is not None:
        f = np.asarray(feats, np.float64)[np.asarray(batch, np.int64).reshape(B, 3)]
        fq, fp, fn = (_normalize64(f[:, c]) for c in range(3))

        def cos(a, b):  # F.cosine_similarity, eps 1e-8
            return (a * b).sum(1) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-8)
        out["nfl"] = float(np.maximum((1 - cos(fq, fp)) - (1 - cos(fq, fn)) + 1e-4, 0.0).mean())
    return out


def hinge_replay32(Z_by_rank, pos_rank, B, margin):
    """the hinge argument in float32 arithmetic (numpy), for the planted ties:
    p == n gives the same products in the same order, so exactly 0 at margin 0"""
    Z = np.asarray(Z_by_rank, np.float32)
    x = Z[np.asarray(pos_rank, np.int64).reshape(B, 3)]
    nrm = np.maximum(np.sqrt((x * x).sum(2, dtype=np.float32)), np.float32(1e-12))
    cqp = (x[:, 0] * x[:, 1]).sum(1, dtype=np.float32) / (nrm[:, 0] * nrm[:, 1])
    cqn = (x[:, 0] * x[:, 2]).sum(1, dtype=np.float32) / (nrm[:, 0] * nrm[:, 2])
    return cqn - cqp + np.float32(margin)


def _first_bad(name, err, bound, labels):
    """raise naming the first entry with not (err <= bound) (a NaN is wrong);
    labels(flat index tuple) -> text.  Returns the largest err / bound."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    ok = err <= bound
    if not ok.all():
        idx = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.size} entries outside their bound, first at "
                             f"{labels(idx)}: error {err[idx]:.3e}, bound {bound[idx]:.3e}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    return float(ratio.max()) if ratio.size else 0.0


def _exact(name, got, want, labels):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError(f"{name}: shape {got.shape}, reference {want.shape}")
    bad = np.argwhere(~(got == want))
    if len(bad):
        idx = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {want.size} entries differ, first at {labels(idx)}: "
                             f"got {got[idx]!r}, reference {want[idx]!r}")


CALLS = ("query", "positive", "negative")


def check_loss(got, ref, mode, with_feats=True, scalars=True):
    """The loss kernels' outputs against loss_reference.  got: hinge [B], G
    [3][cap][d], Kc [3][cap], Gp [3B][d] (None in the atomics regime), scal [4]
    = {loss, nfl, sum |h_q|^2, variance}.  mode: 'head' (the default engine:
    a repeated rank's rows stay in Gp for the head backward, G holds the
    single-position ranks only), 'rep_sum' (G also holds the repeated ranks'
    sums), 'atomic' (no position CSR: G holds float-atomic sums, no Gp).

    Bounds: hinge HINGE_ATOL absolute, a reference argument of exactly 0 (a
    planted tie) exactly 0.0 and active; the active set equal for every triple;
    Kc exact over the whole capacity; a cotangent row within COT_RTOL of
    max(|row|, cot_scale) (loss_reference), a sum of n rows within the sum of
    its rows' bounds plus (n - 1) 2^-24 sum |row| for its n - 1 fp32 additions
    in any order; G zero wherever no position lands (rows past the top set
    too); loss 1e-6 relative + 1e-9, nfl 1e-4 relative, sum |h_q|^2 (B d + 4)
    2^-24 relative (non-negative terms), variance 1e-5 relative plus the floor
    a rounded mean leaves when the query rows (nearly) coincide: deviations
    from m (1 + e) instead of m add B m^2 e^2 to the sum of squares (the first
    order term cancels, sum (h - m) = 0), |e| <= (B / 4 + 8) 2^-24 for the
    additions of the block sums and their merge -- B / (B - 1) |mean|^2 e^2,
    1e-11 of |mean|^2 at B = 75 and nothing beside 1e-5 of a Gaussian batch's
    variance.
    Returns the largest error / bound of the cotangent rows."""
    B, pr = ref["B"], ref["pos_rank"]
    R, d = ref["Gsum"].shape[1:]
    hinge = np.asarray(got["hinge"], np.float64)
    tri = lambda i: f"triple {i[0]}"
    _first_bad("hinge", np.abs(hinge - ref["arg"]), np.full(B, HINGE_ATOL), tri)
    ties = ref["arg"] == 0.0
    _exact("hinge of the planted ties", hinge[ties], np.zeros(int(ties.sum())), lambda i: f"tie {i[0]}")
    _exact("active set (hinge >= 0)", hinge >= 0, ref["active"], tri)
    Kc = np.asarray(got["Kc"], np.int64)
    Kref = np.zeros_like(Kc)
    Kref[:, :R] = ref["K"]
    _exact("Kc", Kc, Kref, lambda i: f"call {CALLS[i[0]]}, rank {i[1]}")
    G = np.asarray(got["G"], np.float64)
    single = ref["K"].sum(0) == 1                      # ranks with one position over all calls
    in_G = np.ones((3, R), bool) if mode != "head" else np.broadcast_to(single, (3, R))
    Gref = np.where(in_G[:, :, None], ref["Gsum"], 0.0)
    bound = np.where(in_G, COT_RTOL * np.maximum(ref["Gscale"], np.linalg.norm(ref["Gsum"], axis=2)) +
                     np.maximum(ref["K"] - 1, 0) * U24 * ref["Gterms"], 0.0)
    err = np.linalg.norm(G[:, :R] - Gref, axis=2)
    err = np.where(np.isnan(err), np.inf, err)
    worst = _first_bad("G", err, bound, lambda i: f"call {CALLS[i[0]]}, rank {i[1]}")
    _exact("G past the top set", G[:, R:] == 0, np.ones_like(G[:, R:], bool),
           lambda i: f"call {CALLS[i[0]]}, row {R + i[1]}, column {i[2]}")
    if mode != "atomic":
        Gp = np.asarray(got["Gp"], np.float64)
        rep = ~single[pr]                              # positions of repeated ranks
        e = np.linalg.norm(Gp - ref["cot"], axis=1)
        e = np.where(rep, np.where(np.isnan(e), np.inf, e), 0.0)
        b = COT_RTOL * np.maximum(ref["cot_scale"], np.linalg.norm(ref["cot"], axis=1))
        worst = max(worst, _first_bad("Gp", e, b, lambda i: f"position {i[0]} (triple {i[0] // 3}, call "
                                      f"{CALLS[i[0] % 3]}, rank {pr[i[0]]})"))
        zero_rows = rep & ~np.repeat(ref["active"], 3)
        _exact("Gp rows of inactive triples", Gp[zero_rows] == 0, np.ones((int(zero_rows.sum()), d), bool),
               lambda i: f"position {np.flatnonzero(zero_rows)[i[0]]}, column {i[1]}")
    if not scalars:  # (the monitors have not run yet)
        return worst
    scal = np.asarray(got["scal"], np.float64)
    for k, (name, want, tol) in enumerate((("loss", ref["loss"], 1e-6), ("nfl", ref["nfl"], 1e-4),
                                           ("sum |h_q|^2", ref["sumsq"], (B * d + 4) * U24),
                                           ("variance", ref["var"], 1e-5))):
        if name == "nfl" and not with_feats:
            want, tol = 0.0, 0.0                       # no feature monitor: the scalar is 0
        floor = {"loss": 1e-9, "variance": B / (B - 1) * ref["mean_sq"] * ((B / 4 + 8) * U24) ** 2}.get(name, 0.0)
        if not abs(scal[k] - want) <= tol * abs(want) + floor:
            raise AssertionError(f"scalar {k} ({name}): got {scal[k]!r}, reference {want!r}, relative bound {tol:.3e}")
    return worst


def rep_sum32(Gp, pos_rank, R, n_groups=3):
    """rep_sum_kernel's additions in numpy float32: for every rank with >= 2
    positions, G[p % n_groups][r] = the float32 sum from zero, in increasing
    position order, of the rank's Gp rows; None where it writes nothing"""
    Gp = np.asarray(Gp, np.float32)
    pr = np.asarray(pos_rank, np.int64)
    out = {}
    for r in np.flatnonzero(np.bincount(pr, minlength=R) >= 2):
        for p in np.flatnonzero(pr == r):
            key = (int(p % n_groups), int(r))
            out[key] = out.get(key, np.zeros(Gp.shape[1], np.float32)) + Gp[p]
    return out


def check_rep_sum_exact(G, Gp, pos_rank, R, n_groups=3):
    """PINSAGE_HEAD_REP_SUM=0 (and the autograd path, one group): a repeated
    rank's G rows are, bit for bit, rep_sum32 of its Gp rows; its groups
    without a position hold zeros"""
    G = np.asarray(G, np.float32)
    want = rep_sum32(Gp, pos_rank, R, n_groups)
    pr = np.asarray(pos_rank, np.int64)
    for r in np.flatnonzero(np.bincount(pr, minlength=R) >= 2):
        for c in range(n_groups):
            w = want.get((c, int(r)), np.zeros(G.shape[2], np.float32))
            bad = np.flatnonzero(G[c, r].view(np.uint32) != w.view(np.uint32))
            if len(bad):
                raise AssertionError(f"rep_sum: call {CALLS[c]}, rank {r} ({int((pr == r).sum())} positions), column "
                                     f"{bad[0]}: got {G[c, r, bad[0]]!r}, the ordered float32 sum is {w[bad[0]]!r}")


def dz_reference(G, Kc, Gp, pos_rank, R, mode, n_groups=3):
    """dZ[r] = sum_c K[c][r] Gsum[c][r] in float64 from the device's own G / Kc /
    Gp (mode as check_loss: 'head' sums a repeated rank's Gp rows by group p %
    n_groups), and the bound of its fp32 evaluation: (n + 4) 2^-24 sum |terms|
    with n = the rank's positions (their additions) + n_groups (the products
    and the additions over calls)"""
    G, Gp = np.asarray(G, np.float64), (None if Gp is None else np.asarray(Gp, np.float64))
    K = np.asarray(Kc, np.int64)[:, :R]
    pr = np.asarray(pos_rank, np.int64)
    Gs, Ga = G[:, :R].copy(), np.abs(G[:, :R])
    cnt = np.bincount(pr, minlength=R)
    if mode == "head":
        for r in np.flatnonzero(cnt >= 2):
            Gs[:, r], Ga[:, r] = 0.0, 0.0
            for p in np.flatnonzero(pr == r):
                Gs[p % n_groups, r] += Gp[p]
                Ga[p % n_groups, r] += np.abs(Gp[p])
    dz = (K[:n_groups, :, None] * Gs[:n_groups]).sum(0)
    mag = (K[:n_groups, :, None] * Ga[:n_groups]).sum(0)
    return dz, (cnt[:, None] + n_groups + 4) * U24 * mag


def check_rows(name, got_full, R, ref, bound, sentinel=None):
    """got_full [cap][o] against ref [R][o] within bound, entry by entry, naming
    the first wrong (row, column); rows R .. cap - 1 must still hold the
    sentinel bits the test wrote there (a store past the live rows -- a column
    past o of the last row lands there -- shows).  Returns max error / bound."""
    got_full = np.asarray(got_full)
    got = got_full[:R].astype(np.float64)
    err = np.abs(got - ref)
    err = np.where(np.isnan(err), np.inf, err)
    worst = _first_bad(name, err, bound, lambda i: f"row {i[0]}, column {i[1]}")
    if sentinel is not None and got_full.shape[0] > R:
        tail = got_full[R:].astype(np.float32).view(np.uint32)
        _exact(f"{name} past its {R} live rows", tail, np.full_like(tail, sentinel),
               lambda i: f"row {R + i[0]}, column {i[1]}")
    return worst


def gemm_bound(n, absterms):
    """|fl(sum_k a_k b_k) - sum_k a_k b_k| <= (n + 4) 2^-24 sum_k |a_k b_k| for n
    terms: each product is rounded once (relative error <= u = 2^-24) or fused
    into the running sum (no rounding of its own), and a sum of n numbers in
    any order (sequential, pairwise, MFMA chains combined afterwards) passes
    each term through at most n - 1 additions, each with relative error <= u:
    (1 + u)^n - 1 <= n u / (1 - n u); the + 4 absorbs the second-order term
    for the n used here (n u < 1e-4), a bias added after the sum and the
    final conversion.  absterms = |A| @ |B| (+ |bias|)."""
    return (n + 4) * U24 * np.asarray(absterms, np.float64)


def lrelu64(x):
    return np.where(x > 0, x, SLOPE * x)


def lrelu_grad64(y):
    return np.where(y > 0, 1.0, SLOPE)


def head_reference_fwd(y, G1w, G1b, G2w, H1_gpu):
    """H1 = lrelu(y G1^T + b1) from the device's y, Z = H1 G2^T from the device's
    H1; each with its bound (lrelu is 1-Lipschitz: the product's bound holds
    behind it)"""
    y, G1w, G1b, G2w, H1g = (np.asarray(a, np.float64) for a in (y, G1w, G1b, G2w, H1_gpu))
    o = G1w.shape[0]
    H1 = lrelu64(y @ G1w.T + G1b)
    return dict(H1=H1, H1_bound=gemm_bound(o + 1, np.abs(y) @ np.abs(G1w.T) + np.abs(G1b)),
                Z=H1g @ G2w.T, Z_bound=gemm_bound(o, np.abs(H1g) @ np.abs(G2w.T)))


def head_reference_bwd(dZ, H1, y, nrm, G1w, G2w, dP1_gpu):
    """The head backward, each step from the device's own inputs to that step:
    dP1 = (dZ G2) lrelu'(H1); dY = dP1 G1 from the device's dP1; dp = lrelu'(y)
    (dY - y (y . dY)) / nrm; dG2 = dZ^T H1, dG1 = dP1^T y, db1 = sum_rows dP1.
    dp's bound carries dY's (E) through the dot product (sum |y| E + the dot's
    own (o + 4) u sum |y dY|), the subtraction, and the three roundings of the
    scaling: (E + |y| E_dot + 4 u (|dY| + |y| |dot|)) lrelu' / nrm."""
    dZ, H1, y, nrm, G1w, G2w, dP1g = (np.asarray(a, np.float64) for a in (dZ, H1, y, nrm, G1w, G2w, dP1_gpu))
    R, o = dZ.shape
    s = lrelu_grad64(H1)
    out = dict(dP1=(dZ @ G2w) * s, dP1_bound=gemm_bound(o, np.abs(dZ) @ np.abs(G2w)) * s)
    dY = dP1g @ G1w
    E = gemm_bound(o, np.abs(dP1g) @ np.abs(G1w))
    dot = (y * dY).sum(1, keepdims=True)
    E_dot = (np.abs(y) * E).sum(1, keepdims=True) + gemm_bound(o, (np.abs(y * dY)).sum(1, keepdims=True))
    sy = lrelu_grad64(y)
    out["dp"] = sy * (dY - y * dot) / nrm[:, None]
    out["dp_bound"] = sy * (E + np.abs(y) * E_dot + 4 * U24 * (np.abs(dY) + np.abs(y * dot))) / nrm[:, None]
    out["dG2"], out["dG2_bound"] = dZ.T @ H1, gemm_bound(R, np.abs(dZ).T @ np.abs(H1))
    out["dG1"], out["dG1_bound"] = dP1g.T @ y, gemm_bound(R, np.abs(dP1g).T @ np.abs(y))
    out["db1"], out["db1_bound"] = dP1g.sum(0), gemm_bound(R, np.abs(dP1g).sum(0))
    return out


# ---- the case table.  Ids come from the universe [0, HL_N); a case's Z rows
# are seeded Gaussians (rows of a fresh model are nearly collapsed: the
# cotangent, a difference of nearly equal unit vectors, is then no fair fp32
# target).  Seeds are fixed so that every |hinge argument| >= ARG_MIN
# (tests/test_host.py checks it).
HAND_MULTS = (1, 1, 2, 3, 4, 5, 12, 13, 16, 17, 20, 21, 33)   # besides the query node's B + 2
HAND_B = 75


def hand_batch(seed=0):
    """One batch built by hand, B = 75 (225 positions, 14 nodes).  Multiplicity
    over all three calls, per node: 77 (node Q: every query position, the
    positive of one triple -- q == p -- and the negative of another: all three
    groups), then 1 (positive only), 1 (negative only), 2 and 4 (planted ties:
    positive and negative of the same triple(s); hinge exactly 0 at margin 0),
    3 (node X, positives only; hand_Z puts X beside Q, so its triples are all
    inactive), 5 and 17 (negatives only), 13 and 21 (positives only), 12, 16,
    20, 33 (both).  Returns (batch [B][3] int64, roles)."""
    rng = np.random.default_rng(1000 + seed)
    node = rng.choice(HL_N, 14, replace=False).astype(np.int64)
    Q, a1, b1, y2, X, y4, n5, m12, p13, m16, n17, m20, p21, m33 = node
    P = [a1] + [X] * 3 + [p13] * 13 + [p21] * 21 + [m12] * 4 + [m16] * 8 + [m20] * 9 + [m33] * 12
    N = [b1] + [n5] * 5 + [n17] * 17 + [m12] * 8 + [m16] * 8 + [m20] * 11 + [m33] * 21
    assert len(P) == len(N) == 71  # 70 pairs, the q == p triple's negative and the n == Q triple's positive
    while True:
        P2, N2 = list(rng.permutation(P)), list(rng.permutation(N))
        # triple 0: q == p (its negative from the pool); triple 1: n == Q (its positive from the pool)
        tri = [(Q, Q, N2.pop())] + [(Q, P2.pop(), Q)] + [(Q, y2, y2), (Q, y4, y4), (Q, y4, y4)]
        tri += [(Q, p, n) for p, n in zip(P2, N2)]
        t = np.array(tri, np.int64)
        if (t[5:, 1] != t[5:, 2]).all() and t[1, 1] != X:  # no accidental tie; X never beside n == Q
            break
    assert len(t) == HAND_B
    t = t[rng.permutation(HAND_B)]
    return t, dict(Q=int(Q), X=int(X), ties=(int(y2), int(y4)), nodes=node)


def pool_batch(B, S, seed, heavy=False):
    """[B][3] ids over a pool of S nodes, every one present; heavy: Zipf-like
    repeats (a few nodes take most positions)"""
    rng = np.random.default_rng(2000 + seed)
    pool = rng.choice(HL_N, S, replace=False).astype(np.int64)
    w = 1.0 / np.arange(1, S + 1) ** (1.5 if heavy else 0.0)
    rest = rng.choice(pool, 3 * B - S, p=w / w.sum())
    return rng.permutation(np.concatenate([pool, rest])).reshape(B, 3)


def case_Z(case, batch):
    """seeded Gaussian float32 rows [R][out] by rank; the hand batch: X's row
    beside Q's (cos(Q, X) ~ 1: X's triples, all with X as the positive, are
    inactive)"""
    S = np.unique(batch)
    rng = np.random.default_rng(3000 + case["seed"])
    Z = rng.standard_normal((len(S), case["out"])).astype(np.float32)
    if case["kind"] == "hand":
        _, roles = hand_batch()
        q, xr = np.searchsorted(S, roles["Q"]), np.searchsorted(S, roles["X"])
        Z[xr] = 2 * Z[q] + np.float32(0.05) * Z[xr]
    return Z


def case_batch(case):
    if case["kind"] == "hand":
        return hand_batch()[0]
    return pool_batch(case["B"], case["S"], case["seed"], heavy=case["kind"] == "heavy")


def _case(name, kind, out, B, S, seed, margin=0.3, d_in=None, mon=1, rep_sum=1):
    return dict(name=name, kind=kind, out=out, B=B, S=S, seed=seed, margin=margin,
                d_in=d_in or max(out, 4), mon=mon, rep_sum=rep_sum)


# (seed: the first of 0, 1, 2, ... with every |arg| >= ARG_MIN, found on the host)
LOSS_CASES = (
    # every batch size (B % 4 in 0 .. 3: the monitor's last block of 1 .. 4 triples), every width
    [_case(f"B{B}-S{S}-o{o}", "pool", o, B, S, sd) for B, S, o, sd in (
        (2, 1, 4, 0), (3, 9, 8, 0), (4, 7, 16, 3), (5, 11, 32, 0), (7, 13, 64, 0), (8, 20, 128, 4), (9, 17, 4, 0),
        # top sets on both sides of the head's 32-row blocks
        (64, 31, 8, 0), (64, 32, 128, 0), (64, 33, 32, 0), (64, 64, 16, 0), (64, 65, 64, 0),
        (129, 200, 128, 0), (129, 200, 4, 0))] +
    # the hand-built batch: both places the repeated ranks are summed, every width
    [_case(f"hand-o{o}-rs{rs}", "hand", o, HAND_B, 14, 0, margin=0.0, rep_sum=rs)
     for o in (4, 8, 16, 32, 64, 128) for rs in (1, 0)] +
    # the feature monitor's register widths and its streamed tail (d_in > 1024), B % 4 != 0
    [_case(f"feat{d}-mon{m}", "pool", 4, 7, 13, 0, d_in=d, mon=m)
     for d in (4, 128, 132, 256, 260, 512, 1024, 1028) for m in ((1, 0) if d in (4, 1028) else (1,))] +
    [_case("feat132-B129", "pool", 4, 129, 200, 0, d_in=132)] +
    # no position CSR: float atomics into G
    [_case("atomic-16386", "heavy", 8, 5462, 50, 1)])

# the head cases (top-set rows on both sides of the kernels' 32- and 16-row blocks; widths whose
# lane mask cuts inside a wave and whose clamps min(c, o - 4) / min(row, o - 1) decide)
HEAD_SEPARATE_WIDTHS = (4, 12, 32, 100, 124, 128)
HEAD_SEPARATE_ROWS = (1, 31, 32, 33, 65, 200)
HEAD128_FORMS = ("in-tile", "in-tile-off", "k192")   # (d_in, hid) = (128, 128), the same with the knob off, (128, 64)
HEAD128_ROWS = (1, 15, 16, 17, 33)
BACKWARD_WIDTHS = (4, 32, 128)                       # after a loss (the loss needs a width dividing 1024)
AUTOGRAD_WIDTHS = (4, 12, 100, 128)                  # from an output gradient
AUTOGRAD_MULTS = (1, 2, 3, 4, 5, 12, 13, 16, 17, 20, 21, 33)


# ----------------------------------------------------------------------------- GEMM forms, slab reduction, Adam
# The dense part of the layers' backward and the optimizer pass
# (tests/test_gpu_gemm_forms.py, tests/test_gpu_optimizer.py): one GemmParams
# launch (csrc/gemm.h) restated in float64 from the comments of that header,
# reduce_slabs_2d_kernel's documented order in float32, torch's
# _single_tensor_adam in float64 and norm_lrelu_bwd in float64, each with the
# elements of every output buffer the launch may write.  tests/test_host.py
# plants one defect at a time into a correct result and checks that each
# checker names the buffer, row and column.
SLOPE32 = float(np.float32(0.01))     # kSlope as the kernels hold it (0.01f)
EPI_STORE, EPI_ACCUM, EPI_L2NORM, EPI_PARTIAL = 0, 1, 2, 3
GEMM_TILES = {0: (128, 16), 1: (64, 32), 2: (32, 32), 3: (64, 16)}   # cfg: (block rows BM, k-depth BK)
NAN_BITS = 0x7FC12345                 # the pre-fill of plainly stored outputs: a quiet NaN with a payload
TINY32 = 2.0 ** -149                  # the smallest float32 step (results that underflow)


def _rows(idx, n):
    return np.arange(n) if idx is None else np.asarray(idx, np.int64)[:n]


def gemm_operands(s):
    """op(A) [M][K] and op(B) [K][N] of a launch spec, in float64, as gemm.h
    states the layouts: K-major A rows gathered by a_idx, columns k >= K1 from
    a2 (rows by a2_idx) at column k - K1; M-major A k-rows gathered by a_idx;
    K-major B [N][K]; N-major B k-rows gathered by b_idx, columns n >= N1 from
    b2 (k-rows by b2_idx) at column n - N1.  The spec holds every matrix as a
    2-D array whose second extent is its leading dimension."""
    M, N, K = s["M"], s["N"], s["K"]
    a, b = np.asarray(s["a"], np.float64), np.asarray(s["b"], np.float64)
    K1, N1 = s.get("K1", -1), s.get("N1", -1)
    if s.get("a_kmajor", True):
        r = _rows(s.get("a_idx"), M)
        if K1 >= 0 and s.get("a2") is not None:
            r2 = _rows(s.get("a2_idx"), M)
            A = np.concatenate([a[r, :K1], np.asarray(s["a2"], np.float64)[r2, :K - K1]], 1)
        else:
            A = a[r, :K]
    else:
        A = a[_rows(s.get("a_idx"), K), :M].T
    if s.get("b_kmajor", True):
        B = b[:N, :K].T
    else:
        rk = _rows(s.get("b_idx"), K)
        if s.get("b2") is not None:
            rk2 = _rows(s.get("b2_idx"), K)
            B = np.concatenate([b[rk, :N1], np.asarray(s["b2"], np.float64)[rk2, :N - N1]], 1)
        else:
            B = b[rk, :N]
    assert A.shape == (M, K) and B.shape == (K, N), (A.shape, B.shape)
    return A, B


def gemm_terms(n, K, prec):
    """the n of gemm_bound for a sum of n terms of which K are products, under
    the product arithmetic prec.  0 (fp32 MFMA): n.  1 (split bf16): every
    product is six bf16 products, each exact in float32, summed sixteen k at a
    time inside one MFMA and added to the accumulator, so a term passes through
    at most 16 additions inside its MFMA and the 6 ceil(K / 16) accumulator
    updates -- more than n for short K."""
    return n if prec == 0 else max(n, n - K + 6 * -(-K // 16) + 16)


def _prod_bound(n, K, absprod, absall, prec, exact):
    """gemm_bound of a sum whose products' absolute values sum to absprod (all
    terms: absall).  Split bf16 drops mid lo, lo mid and lo lo of
    (hi + mid + lo)(hi' + mid' + lo'), each below 2^-24 |a b|, and represents an
    operand to 2^-26 relative: 3 2^-24 |a b| per product covers both.  exact:
    the caller states that every operand is a small integer (exact in the hi
    plane) and every partial sum below 2^24 -- no rounding at all."""
    if exact:
        return np.zeros_like(absall)
    return gemm_bound(gemm_terms(n, K, prec), absall) + (3 * U24 * absprod if prec == 1 else 0.0)


def gemm_form_reference(s, prec=0, exact=False):
    """One GemmParams launch in float64.  s: M, N, K (the live sizes, device
    side or not), a_kmajor, b_kmajor, a, a_idx, K1, a2, a2_idx, b, b_idx, N1,
    b2, b2_idx, bias, act, mask, epi, splits, c_idx, and the PRE-FILLED output
    buffers c, c2, norms [rows], bias_part [splits][M] (2-D arrays with the
    leading dimension as second extent; c of a partial launch is
    [splits * M][ldc]).  Returns {buffer: dict(want, bound, written)}: `want`
    float64 where `written`, and where not written the launch must leave the
    pre-fill bit for bit.

    Epilogues (gemm.h): x = acc + bias[n]; LeakyReLU when act; times
    lrelu'(mask[m][n]) = (mask > 0 ? 1 : 0.01f) when mask -- 0.0, -0.0 and
    negative denormals take the slope; EPI_ACCUM adds c's pre-fill.  Row m goes
    to c row c_idx[m]; with c2, columns >= N1 go to c2[m][n - N1] by row m,
    never accumulated.  EPI_L2NORM: v = lrelu(x), norms[m] = |v|, c = v / |v|.
    EPI_PARTIAL: slab s = the sum over k in [s kc, min(K, (s + 1) kc)), kc =
    ceil(K / splits) rounded up to 32; bias_part[s][m] = that range's sum of
    A(m, k); an empty range gives zeros.

    Bounds.  Store / accumulate / partial: gemm_bound over the K products, the
    bias and the accumulated pre-value, n by gemm_terms, plus _prod_bound's
    split-bf16 term.  Stream-K needs no term of its own: its pieces start from
    a zero accumulator (exact) and their combination is one more summation
    order of the same K terms, which gemm_bound allows.  LeakyReLU and the
    mask are products with 1 or 0.01f: the error scales with them and each
    rounds once (2^-24 |result|).  L2 norm, with E the bound of v: the sum of
    squares s2 = sum v^2 is off by sum 2 |v| E + (N + 4) u s2 (N products and
    additions), r = sqrt(s2) by half of that over r plus u r for the root,
    E_r = sum |v| E / r + ((N + 4) / 2 + 1) u r, and y = v / r by
    E / r + |v| E_r / r^2 + u |y| (first order; the + 4 carries the second)."""
    M, N, K = s["M"], s["N"], s["K"]
    epi = s.get("epi", EPI_STORE)
    A, B = gemm_operands(s)
    out = {}

    def blank(name):
        pre = np.asarray(s[name])
        return dict(want=np.full(pre.shape, np.nan), bound=np.zeros(pre.shape), written=np.zeros(pre.shape, bool))

    if epi == EPI_PARTIAL:
        S = s.get("splits", 1)
        kc = (-(-K // S) + 31) // 32 * 32
        c = blank("c")
        bp = blank("bias_part") if s.get("bias_part") is not None else None
        for sp in range(S):
            k0, k1 = min(K, sp * kc), min(K, (sp + 1) * kc)
            Ak, Bk = A[:, k0:k1], B[k0:k1]
            absacc = np.abs(Ak) @ np.abs(Bk)
            rows = slice(sp * M, (sp + 1) * M)
            c["want"][rows, :N] = Ak @ Bk
            c["bound"][rows, :N] = _prod_bound(k1 - k0, k1 - k0, absacc, absacc, prec, exact)
            c["written"][rows, :N] = True
            if bp is not None:
                bp["want"][sp, :M] = Ak.sum(1)
                bp["bound"][sp, :M] = 0.0 if exact else gemm_bound(k1 - k0, np.abs(Ak).sum(1))
                bp["written"][sp, :M] = True
        out["c"] = c
        if bp is not None:
            out["bias_part"] = bp
        return out

    bias = np.zeros(N) if s.get("bias") is None else np.asarray(s["bias"], np.float64)[:N]
    x = A @ B + bias
    absprod = np.abs(A) @ np.abs(B)
    n = K + (s.get("bias") is not None)
    dst = _rows(s.get("c_idx"), M)
    c = blank("c")
    if epi == EPI_L2NORM:
        E = _prod_bound(n, K, absprod, absprod + np.abs(bias), prec, exact)
        v = np.where(x > 0, x, SLOPE32 * x)
        E = np.where(x > 0, E, SLOPE32 * E + U24 * np.abs(v))
        r = np.sqrt((v * v).sum(1, keepdims=True))
        E_r = (np.abs(v) * E).sum(1, keepdims=True) / r + ((N + 4) / 2 + 1) * U24 * r
        y = v / r
        c["want"][dst, :N] = y
        c["bound"][dst, :N] = E / r + np.abs(v) * E_r / r ** 2 + U24 * np.abs(y)
        c["written"][dst, :N] = True
        out["c"] = c
        if s.get("norms") is not None:
            nr = blank("norms")
            nr["want"][:M], nr["bound"][:M], nr["written"][:M] = r[:, 0], E_r[:, 0], True
            out["norms"] = nr
        return out

    absall = absprod + np.abs(bias)
    scale = np.ones((M, N))
    rounds = np.zeros((M, N))
    if s.get("act"):
        neg = ~(x > 0)
        x = np.where(neg, SLOPE32 * x, x)
        scale, rounds = np.where(neg, SLOPE32, 1.0), rounds + neg
    if s.get("mask") is not None:
        assert epi == EPI_STORE, "launch_gemm refuses a mask with an accumulate"
        g = np.where(np.asarray(s["mask"], np.float32)[:M, :N] > 0, 1.0, SLOPE32)
        x, scale, rounds = x * g, scale * g, rounds + (g != 1.0)
    if exact and epi == EPI_STORE:
        # an exact sum times 0.01f rounds once: float32 of the float64 product, bit for bit
        rounds = np.where(rounds <= 1, 0, rounds)
    N1 = s.get("N1", -1)
    nc = N1 if s.get("c2") is not None else N          # columns that go to c
    pre = np.asarray(s["c"], np.float64)[dst, :nc] if epi == EPI_ACCUM else np.zeros((M, nc))
    xc = x[:, :nc] + pre
    c["want"][dst, :nc] = xc
    c["bound"][dst, :nc] = (_prod_bound(n + (epi == EPI_ACCUM), K, absprod[:, :nc] * scale[:, :nc],
                                        absall[:, :nc] * scale[:, :nc] + np.abs(pre), prec, exact) +
                            rounds[:, :nc] * U24 * np.abs(x[:, :nc]))
    c["written"][dst, :nc] = True
    out["c"] = c
    if s.get("c2") is not None:
        c2 = blank("c2")
        c2["want"][:M, :N - N1] = x[:, N1:]
        c2["bound"][:M, :N - N1] = (_prod_bound(n, K, absprod[:, N1:] * scale[:, N1:], absall[:, N1:] * scale[:, N1:],
                                                prec, exact) + rounds[:, N1:] * U24 * np.abs(x[:, N1:]))
        c2["written"][:M, :N - N1] = True
        out["c2"] = c2
    return out


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_written(name, got, pre, ref, exact=False):
    """One output buffer of a launch against its reference entry (want, bound,
    written): an element the launch may not write must hold the pre-fill bit
    for bit; a written one must lie within its bound of want -- or, exact,
    hold float32(want) bit for bit (exact-sum inputs; a bound that is not 0
    there, the L2 norm's own roundings, is still applied as a bound).  Raises
    naming buffer, row and column; returns the largest error / bound."""
    got, pre = np.asarray(got, np.float32), np.asarray(pre, np.float32)
    sh = ref["written"].shape
    assert got.shape == sh and pre.shape == sh, (name, got.shape, pre.shape, sh)
    g2, p2, w2 = (np.reshape(v, (sh[0], -1)) for v in (got, pre, ref["written"]))
    where = lambda i: f"buffer {name}, row {i[0]}, column {i[1]}"
    stray = np.argwhere((bits32(g2) != bits32(p2)) & ~w2)
    if len(stray):
        i = tuple(int(v) for v in stray[0])
        raise AssertionError(f"{where(i)}: {len(stray)} elements outside the launch's outputs changed, first "
                             f"{p2[i]!r} (bits {bits32(p2)[i]:#010x}) -> {g2[i]!r}")
    want, bound = np.reshape(ref["want"], g2.shape), np.reshape(ref["bound"], g2.shape)
    if exact:
        tight = w2 & (bound == 0)
        w32 = np.where(tight, want, 0.0).astype(np.float32)
        bad = np.argwhere(tight & (bits32(g2) != bits32(w32)))
        if len(bad):
            i = tuple(int(v) for v in bad[0])
            raise AssertionError(f"{where(i)}: {len(bad)} elements differ from the exact result, first got "
                                 f"{g2[i]!r}, float64 gives {want[i]!r}")
        w2 = w2 & ~tight                               # (checked; float32(want) need not equal want)
    err = np.abs(g2.astype(np.float64) - np.where(w2, want, 0.0))
    err = np.where(w2, np.where(np.isnan(err), np.inf, err), 0.0)
    return _first_bad(f"buffer {name}", err, np.where(w2, bound, 0.0), lambda i: f"row {i[0]}, column {i[1]}")


def check_gemm_form(got, pre, ref, exact=False):
    """every output buffer of a launch (dicts by buffer name); returns the
    largest error / bound over them"""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return max(check_written(k, got[k], pre[k], ref[k], exact) for k in sorted(ref))


def apply_launch(pre, ref):
    """what a correct launch leaves: float32(want) where written, the pre-fill
    elsewhere (the host tests plant their defects into this)"""
    return {k: np.where(ref[k]["written"], np.nan_to_num(ref[k]["want"]), np.asarray(pre[k], np.float32))
            .astype(np.float32) for k in ref}


def exact_ints(rng, shape, lim=8):
    """integers of magnitude <= lim as float32: exact in a bf16 hi plane, sums
    of up to 2^24 / lim^2 products exact in float32"""
    return rng.integers(-lim, lim + 1, shape).astype(np.float32)


def wide_rows(rng, shape):
    """Gaussians with a wide-range row scaling 2^(-20 .. 19), as
    test_split_bf16_products_are_fp32_accurate scales its rows"""
    x = rng.standard_normal(shape)
    return (x * np.exp2(rng.integers(-20, 20, (shape[0],) + (1,) * (len(shape) - 1)))).astype(np.float32)


def form_values(rng, shape, exact, wide=False):
    """a case's inputs: exact-sum integers, or Gaussians (wide: row-scaled)"""
    if exact:
        return exact_ints(rng, shape)
    return wide_rows(rng, shape) if wide else rng.standard_normal(shape).astype(np.float32)


# ---- reduce_slabs_2d_kernel
def reduce_slabs32(part):
    """reduce_slabs_2d_kernel's additions in numpy float32, part [S][...]:
    group g = 0..3 sums slabs g, g + 4, ...: while k + 12 < S, acc += (x[k] +
    x[k + 4]) + (x[k + 8] + x[k + 12]) and k += 16; then acc += x[k], k += 4;
    the result is (acc0 + acc1) + (acc2 + acc3)"""
    x = np.asarray(part, np.float32)
    S = x.shape[0]
    acc = []
    for g in range(4):
        a = np.zeros(x.shape[1:], np.float32)
        k = g
        while k + 12 < S:
            a = a + ((x[k] + x[k + 4]) + (x[k + 8] + x[k + 12]))
            k += 16
        while k < S:
            a = a + x[k]
            k += 4
        acc.append(a)
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def reduce_bias32(bpart):
    """the bias blocks of the same kernel: group g adds bpart[g], bpart[g + 4],
    ... one by one; (acc0 + acc1) + (acc2 + acc3)"""
    x = np.asarray(bpart, np.float32)
    acc = []
    for g in range(4):
        a = np.zeros(x.shape[1:], np.float32)
        for k in range(g, x.shape[0], 4):
            a = a + x[k]
        acc.append(a)
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def check_reduce_slabs(name, got_full, pre_full, part, M, N, emul=reduce_slabs32):
    """out [M][ld] of the reduction of part [S][M][N]: columns < N bitwise the
    order emulation and within (S + 1) 2^-24 sum_s |part| of the float64 sum (S
    terms pass through at most S - 1 additions; the + 1 is gemm_bound's slack
    scaled down to a sum without products); columns >= N and rows >= M keep
    the pre-fill.  Returns error / bound against float64."""
    part = np.asarray(part, np.float32)
    S = part.shape[0]
    p64 = part.astype(np.float64)
    ref = dict(want=np.full(np.shape(pre_full), np.nan), bound=np.zeros(np.shape(pre_full)),
               written=np.zeros(np.shape(pre_full), bool))
    sl = (slice(0, M), slice(0, N)) if ref["want"].ndim == 2 else (slice(0, M),)
    ref["want"][sl], ref["bound"][sl], ref["written"][sl] = p64.sum(0), (S + 1) * U24 * np.abs(p64).sum(0), True
    worst = check_written(name, got_full, pre_full, ref)
    em = dict(ref, want=np.array(ref["want"]), bound=np.zeros_like(ref["bound"]))
    em["want"][sl] = emul(part)
    check_written(name + " (order emulation)", got_full, pre_full, em, exact=True)
    return worst


# ---- Adam
def adam_coef(step, lr=1e-3, beta1=0.9, beta2=0.999):
    """the host's coef (pinsage_training._adam_coef): formed in double, staged as float32"""
    return np.array([lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5], np.float32)


def adam_reference(p, g, m, v, coef, beta1=0.9, beta2=0.999, eps=1e-8, swap_betas=False, drop_bc2=False):
    """One step of torch's _single_tensor_adam in float64 from float32 state,
    with the step size and sqrt(1 - beta2^t) the host staged (coef, float32):
        m' = lerp(m, g, 1 - beta1);  v' = beta2 v + (1 - beta2) g^2
        p' = p - coef[0] m' / (sqrt(v') / coef[1] + eps)
    and the bound of adam1's float32 evaluation (conv.hip), u = 2^-24, every
    rounding <= u |result| or half a denormal step (TINY32):
      m'  4 roundings -- g - m, (float)(1 - beta1), their product, the sum:
          E_m = u (3 (1 - beta1) |g - m| + |m'|) + 3 TINY32
      v'  beta2 v: (float)beta2 and the product; (1 - beta2) g g: the
          constant and two products; the sum: every term is >= 0, so
          E_v = 4 u v' + 4 TINY32 (g^2 of a tiny g underflows to 0)
      p'  s = sqrt(v'): |sqrt a - sqrt b| <= min(sqrt |a - b|, |a - b| / sqrt b),
          plus the root's rounding; den = s / bc2 + eps rounds three times (the
          quotient, (float)eps, the sum); q = m' / den once; coef[0] q once;
          p - coef[0] q once:
          E_den = E_s / bc2 + 3 u den,  E_q = E_m / den + |m'| E_den / den^2 + u |q|,
          E_p = coef[0] (E_q + u |q|) + u |p'| + TINY32
    (first order; the 1 + 2^-10 factor carries the second-order terms, u^2
    relative).  swap_betas / drop_bc2: the planted defects of the host tests.
    Returns dict(p, m, v, E_p, E_m, E_v)."""
    p, g, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    ss, bc2 = float(coef[0]), float(coef[1])
    if swap_betas:
        beta1, beta2 = beta2, beta1
    if drop_bc2:
        bc2 = 1.0
    m1 = m + (g - m) * (1 - beta1)
    v1 = v * beta2 + (1 - beta2) * g * g
    s = np.sqrt(v1)
    den = s / bc2 + eps
    q = m1 / den
    p1 = p - ss * q
    E_m = U24 * (3 * (1 - beta1) * np.abs(g - m) + np.abs(m1)) + 3 * TINY32
    E_v = 4 * U24 * v1 + 4 * TINY32
    with np.errstate(divide="ignore", invalid="ignore"):
        E_s = np.minimum(np.sqrt(E_v), np.where(s > 0, E_v / np.where(s > 0, s, 1.0), np.inf)) + U24 * s
    E_den = E_s / bc2 + 3 * U24 * den
    E_q = E_m / den + np.abs(m1) * E_den / den ** 2 + U24 * np.abs(q)
    E_p = ss * (E_q + U24 * np.abs(q)) + U24 * np.abs(p1) + TINY32
    f = 1 + 2.0 ** -10
    return dict(p=p1, m=m1, v=v1, E_p=f * E_p, E_m=f * E_m, E_v=f * E_v)


def check_adam(got_p, got_m, got_v, ref, where=lambda i: f"element {i[0]}"):
    """p, m, v after a step against adam_reference; names the buffer and the
    element.  Returns the largest error / bound."""
    worst = 0.0
    for name, got in (("m", got_m), ("v", got_v), ("p", got_p)):
        err = np.abs(np.asarray(got, np.float64) - ref[name])
        err = np.where(np.isnan(err), np.inf, err)
        worst = max(worst, _first_bad(f"adam {name}", err, ref["E_" + name], where))
    return worst


def adam_gradient(rng, n):
    """gradient elements that are exactly 0, 1e-30 (sqrt(v) / bc2 far below
    eps), near 1e4, and Gaussians, in every position mod 4"""
    g = rng.standard_normal(n).astype(np.float32)
    for k, val in enumerate((0.0, 1e-30, 1e4, -9.7e3, -1e-30)):
        g[k::7][: max(1, n // 11)] = val
    return g


# ---- norm_lrelu_bwd
def norm_lrelu_bwd_reference(y, nrm, dy):
    """dp = lrelu'(y) (dy - y (y . dy)) / nrm in float64 (y == 0 takes the
    slope) and its float32 bound, carried as head_reference_bwd carries dp's:
    the dot product of `out` terms within (out + 4) u sum |y dy|, then the
    product y dot, the subtraction, 1 / nrm, and the two scalings round once
    each: (|y| E_dot + 5 u (|dy| + |y dot|)) lrelu' / nrm."""
    y, nrm, dy = (np.asarray(a, np.float64) for a in (y, nrm, dy))
    o = y.shape[1]
    dot = (y * dy).sum(1, keepdims=True)
    E_dot = gemm_bound(o, np.abs(y * dy).sum(1, keepdims=True))
    sy = np.where(y > 0, 1.0, SLOPE32)
    return (sy * (dy - y * dot) / nrm[:, None],
            sy * (np.abs(y) * E_dot + 5 * U24 * (np.abs(dy) + np.abs(y * dot))) / nrm[:, None])
