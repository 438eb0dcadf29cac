"""SHA-256 digests of what the row-wise fits (csrc/als.hip, csrc/lmf.hip,
csrc/n2v.hip on the plan of csrc/rowplan.h; baselines.ALS / LMF / Node2Vec)
write for fixed, seeded inputs:

    [PINSAGE_LIB=other/libpinsage_hip.so] python tools/factor_bits.py

prints one JSON line {case: digests, "all": the digest of them all}.  Two builds compute the same bits exactly
when their lines are equal; there is no reference and no tolerance here.  Run
each build in a process of its own.  The cases: pinsage_als_half,
pinsage_lmf_update and pinsage_sgns_update (lr 0.1 and 0) at f = 4, 60, 128 with
every ld = f + 4 over rows in both forms (two long rows in one block of 8, one
in the next, an empty row) and over 33 short rows (one past a workgroup's 32),
an id out of range on each kernel, pinsage_lmf_dense and pinsage_sgns_dense at
the same f over 130 rows and 33 items (one past a workgroup, one past a tile),
whole ALS and LMF fits of a 60 x 80 matrix and whole Node2Vec fits, from given
counts and from a small graph, each with random_state 0 and None.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "gcn-song-embeddings_amd")):
    sys.path.insert(0, p)

import _native as nat  # noqa: E402
import als_util as au  # noqa: E402
import baselines as bl  # noqa: E402
import n2v_util as nu  # noqa: E402

LONG = [5000, 3, 512, 513, 0, 64, 576, 1, 2, 641, 7]
N_OTHER, REG, ALPHA, STEPS = 6000, 0.01, 2.0, 3


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def table(rng, n, f, ld):
    """[n, ld] on the device: au.init_factors in columns [0, f), zeros in the padding."""
    t = np.zeros((n, ld), np.float32)
    t[:, :f] = au.init_factors(rng, n, f)
    return torch.from_numpy(t).cuda()


def dev(csr):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in csr[:3]]


def als_half(csr, f, rng):
    L, ld, n = nat.lib(), f + 4, csr[3]
    ptr, idx, val = dev(csr)
    X, Y = table(rng, n, f, ld), table(rng, csr[4], f, ld)
    G = torch.empty(f * f, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nat.check(L.pinsage_als_gram(nat.ptr(Y), csr[4], f, ld, REG, nat.ptr(G), nat.stream_ptr()), "als_gram")
    nat.check(L.pinsage_als_half(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n, nat.ptr(Y), csr[4], ld, nat.ptr(X), ld,
                                 f, nat.ptr(G), ALPHA, STEPS, nat.ptr(err), nat.stream_ptr()), "als_half")
    return {"X": digest(X), "G": digest(G), "err": digest(err)}


def lmf_update(csr, f, rng, lr):
    L, ld, n, m = nat.lib(), f + 4, csr[3], csr[4]
    ptr, idx, val = dev(csr)
    X, Y, D, H = (table(rng, k, f, ld) for k in (n, m, n, n))
    H.abs_()
    bx, by, dsum, hb = (torch.from_numpy(rng.random(k).astype(np.float32) - 0.5).cuda() for k in (n, m, n, n))
    hb.abs_()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nat.check(L.pinsage_lmf_update(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), n, nat.ptr(Y), nat.ptr(by), m, ld,
                                   nat.ptr(X), nat.ptr(bx), ld, f, nat.ptr(D), ld, nat.ptr(dsum), nat.ptr(H), ld,
                                   nat.ptr(hb), ALPHA, 0.6, lr, nat.ptr(err), nat.stream_ptr()), "lmf_update")
    return {"X": digest(X), "bx": digest(bx), "H": digest(H), "hb": digest(hb), "err": digest(err)}


def sgns_update(csr, f, rng, lr):
    L, ld, n, m = nat.lib(), f + 4, csr[3], csr[4]
    ptr, idx, val = dev(csr)
    X, Y, D, H = (table(rng, k, f, ld) for k in (n, m, n, n))
    H.abs_()
    rw = torch.from_numpy(rng.uniform(0.5, 2, n).astype(np.float32)).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nat.check(L.pinsage_sgns_update(nat.ptr(ptr), nat.ptr(idx), nat.ptr(val), nat.ptr(rw), n, nat.ptr(Y), m, ld,
                                    nat.ptr(X), ld, f, nat.ptr(D), ld, nat.ptr(H), ld, 0.6, lr, nat.ptr(err),
                                    nat.stream_ptr()), "sgns_update")
    return {"X": digest(X), "H": digest(H), "err": digest(err)}


def dense(f, rng, n=130, m=33):
    """Both forms of the dense term on the same X and Y: one past a 128-row workgroup, one past a 32-item tile."""
    L, ld = nat.lib(), f + 4
    X, Y = table(rng, n, f, ld), table(rng, m, f, ld)
    bx, by = (torch.from_numpy(rng.random(k).astype(np.float32) - 0.5).cuda() for k in (n, m))
    cw = torch.from_numpy(rng.uniform(0, 2, m).astype(np.float32)).cuda()
    D, Dw = torch.zeros_like(X), torch.zeros_like(X)
    dsum = torch.zeros(n, dtype=torch.float32, device="cuda")
    nat.check(L.pinsage_lmf_dense(nat.ptr(X), nat.ptr(bx), n, ld, nat.ptr(Y), nat.ptr(by), m, ld, f, nat.ptr(D), ld,
                                  nat.ptr(dsum), nat.stream_ptr()), "lmf_dense")
    nat.check(L.pinsage_sgns_dense(nat.ptr(X), n, ld, nat.ptr(Y), nat.ptr(cw), m, ld, f, nat.ptr(Dw), ld,
                                   nat.stream_ptr()), "sgns_dense")
    return {"D": digest(D), "dsum": digest(dsum)}, {"D": digest(Dw)}


def n2v_fits(random_state, graph, counts):
    """Node2Vec from given counts and from walks on a graph; with random_state None also torch's generator after."""
    out = {}
    for name, kw in (("counts", {"graph_csr": None, "cooccurrence": counts}), ("graph", {"graph_csr": graph})):
        torch.manual_seed(7)
        m = bl.Node2Vec(dim=16, iterations=2, walk_length=8, context=3, walks_per_node=2,
                        random_state=random_state).fit(**kw)
        out[name] = {"embedding": digest(m.embedding), "context_factors": digest(m.context_factors),
                     "noise": digest(m.noise), "walks": None if m.walks is None else digest(m.walks)}
        if random_state is None:
            out[name + "_rng_after"] = digest(torch.get_rng_state())
    return out


def fits(csr, random_state):
    """The fitted tables of both models; with random_state None also torch's generator afterwards."""
    out = {}
    for name, model in (("ALS", bl.ALS), ("LMF", bl.LMF)):
        torch.manual_seed(7)
        m = model(factors=16, iterations=2, random_state=random_state).fit(tuple(csr))
        tabs = [m.user_factors, m.item_factors] + ([m.user_bias, m.item_bias] if name == "LMF" else [])
        out[name] = digest(*tabs)
        if random_state is None:
            out[name + "_rng_after"] = digest(torch.get_rng_state())
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("factor_bits needs the GPU")
    out = {}
    rng = np.random.default_rng(0)
    shapes = {"long": au.random_csr(rng, LONG, N_OTHER, "counts"),
              "33": au.random_csr(rng, rng.integers(0, 200, 33), N_OTHER, "fractions")}
    for what, csr in shapes.items():
        for f in (4, 60, 128):
            out[f"als_half_{what}_f{f}"] = als_half(csr, f, rng)
            for lr in (0.1, 0.0):
                out[f"lmf_update_{what}_f{f}_lr{lr}"] = lmf_update(csr, f, rng, lr)
    bad = au.random_csr(rng, [70, 9, 600], 1000, "ones")
    bad[1][[5, 75, 300]] = [1000, -1, 2 ** 31 - 1]  # in a full group, in a tail, in a long row
    out["als_half_bad_id"] = als_half(bad, 8, rng)
    out["lmf_update_bad_id"] = lmf_update(bad, 8, rng, 0.1)
    small = au.random_csr(rng, rng.integers(1, 21, 60), 80, "counts")
    out["fit_seed0"] = fits(small, 0)
    out["fit_global"] = fits(small, None)
    # the cases below draw from a generator of their own: the ones above keep the bits they had before these existed
    rng = np.random.default_rng(1)
    for what, csr in shapes.items():
        for f in (4, 60, 128):
            for lr in (0.1, 0.0):
                out[f"sgns_update_{what}_f{f}_lr{lr}"] = sgns_update(csr, f, rng, lr)
    out["sgns_update_bad_id"] = sgns_update(bad, 8, rng, 0.1)
    for f in (4, 60, 128):
        out[f"lmf_dense_f{f}"], out[f"sgns_dense_f{f}"] = dense(f, rng)
    R = np.zeros((80, 80))
    R[:60] = au.dense(small)
    counts = tuple(torch.from_numpy(a) if isinstance(a, np.ndarray) else a for a in nu.csr_of(R + R.T))
    g = nu.small_graph()
    graph = (torch.from_numpy(g[0]), torch.from_numpy(g[1]), torch.from_numpy(nu.weights_of(g)), g[3])
    out["n2v_fit_seed0"] = n2v_fits(0, graph, counts)
    out["n2v_fit_global"] = n2v_fits(None, graph, counts)
    out["all"] = hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest()  # of the cases above
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
