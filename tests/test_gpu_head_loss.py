"""The end of the train step against float64 (parity_util.loss_reference /
head_reference_*): the loss kernels of conv.hip (loss_triple_kernel, det_put,
rep_sum_kernel, loss_monitor_kernel, dout_accum_kernel, dz_scale_kernel's
multiplicity rule), head_fwd_kernel / head_bwd_kernel with head_sum_reps
(head.hip) and the head inside the top layer's 16-row tile (AggHead, aggw.hip).

The tests drive a real engine through the C-ABI (universe of 300 items, one
layer, T = 3, Gaussian features and Gaussian parameters scaled by 1 / sqrt(fan
in)) and read its buffers through pinsage_engine_offsets and
pinsage_engine_head_offsets.  Read off the code:

  * the loss reads Z, pos_rank, rank_off, the ids and the features: the loss
    tests run pinsage_engine_frontier, write seeded Gaussian rows to Z
    themselves and call pinsage_engine_loss;
  * the monitor kernel is enqueued by the next engine call that enqueues work:
    pinsage_engine_gather_output flushes it, a device-wide synchronize covers
    the engine's side streams;
  * a workspace whose loss was not followed by a backward is not reused;
  * PINSAGE_HEAD_REP_SUM / PINSAGE_HEAD_IN_AGGW are read when the engine is
    created;
  * with one layer, pinsage_engine_backward_stage(0) is the head alone (dZ, dP1,
    the top layer's dp, dG2, dG1, db1) and stage 1 the layer below it.

H1, Z, dZ, dP1 and dp are filled with a NaN pattern before the call that writes
them: a live row left unwritten shows as an error, a store past the live rows
(where a column past out of the last row lands) as a changed pattern.  Bounds:
parity_util.check_loss and gemm_bound; the measured error / bound ratios are
in DESIGN.md.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import parity_util as pu
from conftest import REPO
from parity_util import HL_N, HL_T, LOSS_CASES

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345  # a quiet NaN with a payload
ERR_ARG = -2           # PINSAGE_ERR_ARG


class Rig:
    """one engine (n_layers = 1) with its tensors and one workspace"""

    def __init__(self, d_in, hid, out, max_pos, seed=0):
        import _native as nat
        import pinsage_model as pm
        self.nat, self.lib = nat, nat.lib()
        self.d_in, self.hid, self.out, self.max_pos = d_in, hid, out, max_pos
        self.eng = pm._Engine(HL_N, d_in, hid, out, 1, HL_T, max_pos)
        self.off = self.eng.off
        self.ho = nat.EngineHeadOffsets()
        nat.check(self.lib.pinsage_engine_head_offsets(self.eng.h, ctypes.byref(self.ho)), "head_offsets")
        self.po = nat.EnginePlanOffsets()
        nat.check(self.lib.pinsage_engine_plan_offsets(self.eng.h, ctypes.byref(self.po)), "plan_offsets")
        self.cap = int(self.ho.cap)
        assert self.cap == int(self.off.cap_S[0]) == min(HL_N, max_pos)
        rng = np.random.default_rng(4000 + seed)
        self.feats_np = rng.standard_normal((HL_N, d_in)).astype(np.float32)
        self.nb = pu.perm_table(HL_N, HL_T, HL_T, seed)[0]
        w = rng.random((HL_N, HL_T)) + 0.1
        self.wn = torch.from_numpy((w / w.sum(1, keepdims=True)).astype(np.float32)).cuda()
        # flat parameters in state_dict order: Q.weight, Q.bias, W.weight, W.bias, G1.weight, G1.bias, G2.weight
        shapes = [("Qw", (hid, d_in), d_in), ("Qb", (hid,), d_in), ("Ww", (out, d_in + hid), d_in + hid),
                  ("Wb", (out,), d_in + hid), ("G1w", (out, out), out), ("G1b", (out,), out), ("G2w", (out, out), out)]
        self.p, self.poff, flat, at = {}, {}, [], 0
        for name, shp, fan in shapes:
            v = (rng.standard_normal(shp) / np.sqrt(fan)).astype(np.float32)
            self.p[name], self.poff[name] = v, at
            flat.append(v.reshape(-1))
            at += v.size
        assert at == self.eng.n_params
        self.feats = torch.from_numpy(self.feats_np).cuda()
        self.params = torch.from_numpy(np.concatenate(flat)).cuda()
        self.grads = torch.full((at,), float("nan"), dtype=torch.float32, device="cuda")
        nat.check(self.lib.pinsage_engine_set_tensors(
            self.eng.h, nat.ptr(self.feats), d_in, nat.ptr(self.nb), nat.ptr(self.wn), HL_T,
            nat.ptr(self.params), nat.ptr(self.grads), None, None), "set_tensors")
        self.ws = self.eng.new_workspace(torch.device("cuda"))

    # -- workspace access
    def view(self, off, dtype, n):
        return self.eng.view(self.ws, int(off), dtype, int(n))

    def f32(self, off, *shape):
        return self.view(off, torch.float32, int(np.prod(shape))).cpu().numpy().reshape(shape)

    def i32(self, off, *shape):
        return self.view(off, torch.int32, int(np.prod(shape))).cpu().numpy().reshape(shape)

    def put(self, off, arr):
        a = np.ascontiguousarray(arr, np.float32).reshape(-1)
        self.view(off, torch.float32, a.size).copy_(torch.from_numpy(a).cuda())

    def fill(self, off, n, bits=SENTINEL):
        self.view(off, torch.int32, n).fill_(bits)

    def rows(self):
        return int(self.i32(self.off.count_S[0], 1)[0])

    # -- engine calls
    def call(self, fn, *args):
        self.nat.check(fn(self.eng.h, self.nat.ptr(self.ws), *args, self.nat.stream_ptr()), fn.__name__)

    def run_ids(self, fn, ids):
        self.ids = torch.from_numpy(np.asarray(ids, np.int64).reshape(-1)).cuda()
        self.call(fn, self.nat.ptr(self.ids), len(self.ids))

    def plan(self, ids):
        """pos_rank / rank_off[0] of the last frontier, checked against numpy"""
        ids = np.asarray(ids, np.int64).reshape(-1)
        S = np.unique(ids)
        torch.cuda.synchronize()
        assert self.rows() == len(S)
        pr = self.i32(self.off.pos_rank, len(ids)).astype(np.int64)
        assert np.array_equal(pr, np.searchsorted(S, ids))
        return S, pr, int(self.i32(self.po.rank_off, 1)[0])

    def flush_monitors(self, n_ids):
        out = torch.empty((n_ids, self.out), dtype=torch.float32, device="cuda")
        self.call(self.lib.pinsage_engine_gather_output, n_ids, self.nat.ptr(out))
        torch.cuda.synchronize()

    def loss_outputs(self, B, atomic):
        return dict(hinge=self.f32(self.off.hinge, B), G=self.f32(self.ho.G, 3, self.cap, self.out),
                    Kc=self.i32(self.ho.Kc, 3, self.cap), scal=self.f32(self.off.scalars, 4),
                    Gp=None if atomic else self.f32(self.ho.Gp, 3 * B, self.out))

    def timing_sites(self):
        self.nat.check(self.lib.pinsage_engine_timing_collect(self.eng.h), "timing_collect")
        names, buf, ms, calls = [], ctypes.create_string_buffer(128), ctypes.c_double(), ctypes.c_int64()
        while self.lib.pinsage_engine_timing_get(self.eng.h, len(names), buf, 128, ctypes.byref(ms),
                                                 ctypes.byref(calls)) == 0:
            names.append(buf.value.decode())
        return names


RATIOS = {}  # quantity -> largest error / bound seen in this session (printed by the last test)


def _note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))


def _run_loss(rig, case, batch, Z, frontier=True):
    """frontier (unless a forward has run), Z written by hand, NaNs where Gp will be, the loss"""
    B = len(batch)
    if frontier:
        rig.run_ids(rig.lib.pinsage_engine_frontier, batch)
    S, pr, ro0 = rig.plan(batch)
    assert Z.shape == (len(S), rig.out)
    rig.put(rig.off.z, Z)
    rig.fill(rig.ho.Gp, 3 * B * rig.out)  # garbage where the repeated ranks' rows go
    rig.call(rig.lib.pinsage_engine_loss, B, ctypes.c_float(case["margin"]), case["mon"])
    return S, pr, ro0


# ----------------------------------------------------------------------------- loss
@pytest.mark.parametrize("case", LOSS_CASES, ids=[c["name"] for c in LOSS_CASES])
def test_loss_matches_float64(case, monkeypatch):
    monkeypatch.setenv("PINSAGE_HEAD_REP_SUM", str(case["rep_sum"]))
    batch = pu.case_batch(case)
    B = case["B"]
    Z = pu.case_Z(case, batch)
    rig = Rig(case["d_in"], 4, case["out"], 3 * B, seed=case["seed"])
    S, pr, ro0 = _run_loss(rig, case, batch, Z)
    rig.flush_monitors(3 * B)
    atomic = 3 * B > pu.POS_CSR_MAX
    assert (ro0 == -1) == atomic, f"rank_off[0] = {ro0}"
    got = rig.loss_outputs(B, atomic)
    ref = pu.loss_reference(Z, pr, B, case["margin"], rig.feats_np, batch)
    mode = "atomic" if atomic else "head" if case["rep_sum"] else "rep_sum"
    _note("loss cotangent rows", pu.check_loss(got, ref, mode, with_feats=bool(case["mon"])))
    if case["kind"] == "hand":
        assert int((ref["arg"] == 0.0).sum()) == 3 and ref["active"][ref["arg"] == 0.0].all()
    if mode == "rep_sum":
        pu.check_rep_sum_exact(got["G"], got["Gp"], pr, len(S))


@pytest.mark.parametrize("out", [12, 96])
def test_loss_refuses_a_width_that_does_not_divide_1024(out):
    """pinsage_engine_create takes the width, the loss does not: the argument
    error, nothing launched (G / Kc still zero), the limit in the header; the
    engine still serves a forward afterwards."""
    batch = pu.pool_batch(8, 20, seed=1)
    rig = Rig(out, 8, out, 24)
    rig.run_ids(rig.lib.pinsage_engine_frontier, batch)
    rc = rig.lib.pinsage_engine_loss(rig.eng.h, rig.nat.ptr(rig.ws), 8, ctypes.c_float(0.3), 1, rig.nat.stream_ptr())
    assert rc == ERR_ARG
    assert "divides 1024" in rig.lib.pinsage_last_error().decode()
    with open(os.path.join(REPO, "include", "pinsage_hip.h")) as f:
        assert "divides 1024" in f.read()
    torch.cuda.synchronize()
    assert not rig.f32(rig.ho.G, 3 * rig.cap * out).any() and not rig.i32(rig.ho.Kc, 3 * rig.cap).any()
    _check_forward(rig, batch.reshape(-1), want_head_site=True)


# ----------------------------------------------------------------------------- head forward
def _ids_with_rows(R, seed):
    """ids whose top set has R rows, a third of them repeated"""
    rng = np.random.default_rng(5000 + seed)
    pool = rng.choice(HL_N, R, replace=False).astype(np.int64)
    return rng.permutation(np.concatenate([pool, pool[::3]]))


def _check_forward(rig, ids, want_head_site):
    """the inference forward of ids: H1 and Z against head_reference_fwd, from
    the device's own y (and H1); which head ran, from the engine's timing sites"""
    o = rig.out
    rig.fill(rig.ho.H1, rig.cap * o)
    rig.fill(rig.off.z, rig.cap * o)
    rig.nat.check(rig.lib.pinsage_engine_timing(rig.eng.h, 1), "timing")
    rig.run_ids(rig.lib.pinsage_engine_forward_inference, ids)
    torch.cuda.synchronize()
    sites = rig.timing_sites()
    rig.nat.check(rig.lib.pinsage_engine_timing(rig.eng.h, 0), "timing")
    assert ("fwd.head" in sites) == want_head_site, sites
    R = rig.rows()
    assert R == len(np.unique(ids))
    y = rig.f32(rig.off.y[0], R, o)
    assert np.isfinite(y).all() and np.allclose(np.linalg.norm(y.astype(np.float64), axis=1), 1.0, atol=1e-5)
    H1, Z = rig.f32(rig.ho.H1, rig.cap, o), rig.f32(rig.off.z, rig.cap, o)
    ref = pu.head_reference_fwd(y, rig.p["G1w"], rig.p["G1b"], rig.p["G2w"], H1[:R])
    _note("H1", pu.check_rows("H1", H1, R, ref["H1"], ref["H1_bound"], SENTINEL))
    _note("Z", pu.check_rows("Z", Z, R, ref["Z"], ref["Z_bound"], SENTINEL))
    return sites


@pytest.mark.parametrize("rows", pu.HEAD_SEPARATE_ROWS)
@pytest.mark.parametrize("out", pu.HEAD_SEPARATE_WIDTHS)
def test_head_forward_separate_kernel(out, rows):
    """head_fwd_kernel behind the unfused aggregation and W projection (K = d_in
    + hid is no multiple of 64, so the fused tile does not take the layer)"""
    rig = Rig(max(out, 8), 4, out, 300, seed=out + rows)
    sites = _check_forward(rig, _ids_with_rows(rows, out + rows), want_head_site=True)
    assert "fwd.aggw.l0" not in sites


@pytest.mark.parametrize("rows", pu.HEAD128_ROWS)
@pytest.mark.parametrize("form", pu.HEAD128_FORMS)
def test_head_forward_width_128(form, rows, monkeypatch):
    """d_in = hid = 128 (K = 256): the head inside the 16-row tile; the same with
    PINSAGE_HEAD_IN_AGGW=0; hid = 64 (K = 192): the tile cannot hold the head,
    head_fwd_kernel runs behind the fused aggregation"""
    if form == "in-tile-off":
        monkeypatch.setenv("PINSAGE_HEAD_IN_AGGW", "0")
    else:
        monkeypatch.delenv("PINSAGE_HEAD_IN_AGGW", raising=False)
    rig = Rig(128, 64 if form == "k192" else 128, 128, 300, seed=rows)
    sites = _check_forward(rig, _ids_with_rows(rows, rows), want_head_site=form != "in-tile")
    assert "fwd.aggw.l0" in sites


# ----------------------------------------------------------------------------- head backward
def _head_backward(rig, R, dz_ref, dz_bound):
    """stage 0 of the backward (one layer: the head alone) with NaN patterns
    where it writes; checks dZ, dP1, dp_top and the head's weight gradients,
    each step from the device's own inputs to that step, and that G / Kc are
    zero again over their whole capacity.  Returns what it read (for the
    bitwise comparison of two workspaces)."""
    o, cap = rig.out, rig.cap
    for off in (rig.off.dz, rig.ho.dP1, rig.ho.dp_top):
        rig.fill(off, cap * o)
    rig.grads.fill_(float("nan"))
    rig.call(rig.lib.pinsage_engine_backward_stage, 0)
    torch.cuda.synchronize()
    dZ, dP1, dp = (rig.f32(off, cap, o) for off in (rig.off.dz, rig.ho.dP1, rig.ho.dp_top))
    _note("dZ", pu.check_rows("dZ", dZ, R, dz_ref, dz_bound, SENTINEL))
    y, H1, nrm = rig.f32(rig.off.y[0], R, o), rig.f32(rig.ho.H1, R, o), rig.f32(rig.ho.nrm_top, R)
    ref = pu.head_reference_bwd(dZ[:R], H1, y, nrm, rig.p["G1w"], rig.p["G2w"], dP1[:R])
    _note("dP1", pu.check_rows("dP1", dP1, R, ref["dP1"], ref["dP1_bound"], SENTINEL))
    _note("dp_top", pu.check_rows("dp_top", dp, R, ref["dp"], ref["dp_bound"], SENTINEL))
    g = rig.grads.cpu().numpy()
    grads = {}
    for name, key in (("G2w", "dG2"), ("G1w", "dG1"), ("G1b", "db1")):
        v = g[rig.poff[name]:rig.poff[name] + rig.p[name].size].reshape(rig.p[name].shape)
        grads[name] = v
        lab = f"grad {name}"
        _note(lab, pu.check_rows(lab, v.reshape(len(v), -1), len(v), ref[key].reshape(len(v), -1),
                                 ref[key + "_bound"].reshape(len(v), -1)))
    assert not rig.f32(rig.ho.G, 3 * cap * o).any(), "G is not zero over its capacity after the backward"
    assert not rig.i32(rig.ho.Kc, 3 * cap).any(), "Kc is not zero over its capacity after the backward"
    return dict(dZ=dZ[:R], dP1=dP1[:R], dp=dp[:R], **grads)


def _loss_step(rig, case, batch, Z):
    """train forward, Z by hand, loss, the head backward checked, then the
    layer below (stage 1), which completes the step on this workspace"""
    B = len(batch)
    rig.run_ids(rig.lib.pinsage_engine_forward, batch)
    S, pr, ro0 = _run_loss(rig, case, batch, Z, frontier=False)
    torch.cuda.synchronize()
    got = rig.loss_outputs(B, False)
    mode = "head" if case["rep_sum"] else "rep_sum"
    pu.check_loss(dict(got, scal=None), pu.loss_reference(Z, pr, B, case["margin"]), mode, scalars=False)
    dz, bound = pu.dz_reference(got["G"], got["Kc"], got["Gp"], pr, len(S), mode)
    out = _head_backward(rig, len(S), dz, bound)
    rig.call(rig.lib.pinsage_engine_backward_stage, 1)
    torch.cuda.synchronize()
    out["scal"] = rig.f32(rig.off.scalars, 4)
    out["all_grads"] = rig.grads.cpu().numpy().copy()
    return out


@pytest.mark.parametrize("rep_sum", [1, 0])
@pytest.mark.parametrize("out", pu.BACKWARD_WIDTHS)
def test_head_backward_after_a_loss(out, rep_sum, monkeypatch):
    monkeypatch.setenv("PINSAGE_HEAD_REP_SUM", str(rep_sum))
    case = next(c for c in LOSS_CASES if c["name"] == f"hand-o{out}-rs{rep_sum}")
    batch = pu.case_batch(case)
    rig = Rig(max(out, 8), 8, out, 3 * pu.HAND_B, seed=out)
    _loss_step(rig, case, batch, pu.case_Z(case, batch))
    # a second, different batch on the same workspace: bitwise what a fresh workspace gives
    case2 = dict(case, kind="pool", B=64, S=33, seed=7, margin=0.3)
    batch2 = pu.case_batch(case2)
    Z2 = pu.case_Z(case2, batch2)
    again = _loss_step(rig, case2, batch2, Z2)
    rig.ws = rig.eng.new_workspace(torch.device("cuda"))
    fresh = _loss_step(rig, case2, batch2, Z2)
    for k in fresh:
        assert np.array_equal(again[k].view(np.uint32), fresh[k].view(np.uint32)), \
            f"{k}: a reused workspace and a fresh one differ"


@pytest.mark.parametrize("out", pu.AUTOGRAD_WIDTHS)
def test_head_backward_from_an_output_gradient(out):
    """pinsage_engine_set_output_grad (dout_accum_kernel, rep_sum_kernel with one
    group) then the backward: G[0][r] is the dout row of a single position, bit
    for bit the ordered float32 sum of a repeated rank's rows, K[r] its
    multiplicity, and dZ[r] = K[r] sum dout[p]."""
    rng = np.random.default_rng(6000 + out)
    nodes = rng.choice(HL_N, len(pu.AUTOGRAD_MULTS) + 30, replace=False).astype(np.int64)
    mult = np.concatenate([pu.AUTOGRAD_MULTS, np.ones(30, np.int64)])
    ids = rng.permutation(np.repeat(nodes, mult))
    rig = Rig(max(out, 8), 8, out, len(ids), seed=out)
    rig.run_ids(rig.lib.pinsage_engine_forward, ids)
    S, pr, ro0 = rig.plan(ids)
    R = len(S)
    assert ro0 >= 0 and np.array_equal(np.sort(np.bincount(pr)), np.sort(mult))
    dout = rng.standard_normal((len(ids), out)).astype(np.float32)
    dout_dev = torch.from_numpy(dout).cuda()
    rig.fill(rig.ho.Gp, len(ids) * out)
    rig.call(rig.lib.pinsage_engine_set_output_grad, rig.nat.ptr(dout_dev), len(ids))
    torch.cuda.synchronize()
    G, Kc = rig.f32(rig.ho.G, 3, rig.cap, out), rig.i32(rig.ho.Kc, 3, rig.cap)
    Kref = np.zeros_like(Kc)
    Kref[0, :R] = np.bincount(pr, minlength=R)
    pu._exact("Kc", Kc, Kref, lambda i: f"call {i[0]}, rank {i[1]}")
    want = np.zeros((3, rig.cap, out), np.float32)
    for (c, r), row in pu.rep_sum32(dout, pr, R, n_groups=1).items():
        want[c, r] = row
    for r in np.flatnonzero(np.bincount(pr, minlength=R) == 1):
        want[0, r] = dout[np.flatnonzero(pr == r)[0]]
    pu._exact("G (bits)", G.view(np.uint32), want.view(np.uint32),
              lambda i: f"call {i[0]}, rank {i[1]}, column {i[2]}")
    d64 = dout.astype(np.float64)
    sums, mags = np.zeros((R, out)), np.zeros((R, out))
    np.add.at(sums, pr, d64)
    np.add.at(mags, pr, np.abs(d64))
    K = Kref[0, :R, None]
    _head_backward(rig, R, K * sums, (K + 1 + 4) * pu.U24 * K * mags)
    rig.call(rig.lib.pinsage_engine_backward_stage, 1)
    torch.cuda.synchronize()
    assert np.isfinite(rig.grads.cpu().numpy()).all()


def test_report_ratios():
    """the largest error / bound per quantity over this session (for DESIGN.md)"""
    for k in sorted(RATIOS):
        print(f"max error / bound  {k:22s} {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
