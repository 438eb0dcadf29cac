"""Generate tests/golden/earlystop_{small,mid}.npz by running the REAL reference's
sample_neighborhood_topt_early_stop (pinsage_model.py:55-86) under
make_golden.py's stubs, on that file's `small` and `mid` graphs.

Runs only where the reference checkout is (no test needs it).  The fixtures are
data only: the graph's CSR, the nodeset and, per configuration (n_hops, T, np,
nv), the reference's values and indices and the four next_draws() after the
call (they pin the words the call consumed).  `hops` (the walk lengths, from
tests/earlystop_util.py's restatement, which this script first checks against
the reference's output) is stored beside them.

The configurations are those with T * 64 <= n_tracks (torch's partial_sort
regime of topk): every T = 3 row on both graphs, the two T = 10 rows on `mid`.
The script asserts what makes a fixture worth having: on each graph one
configuration stops some sources and not others, one stops every source, and
nv = 0 and np = 0 stop none.

    python tests/golden/make_golden_earlystop.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

import make_golden as mg

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

ALPHA = 0.85
N_SRC = 24
SEEDS = {"small": 31, "mid": 32}
# (n_hops, T, np, nv)
CONFIGS_T3 = [(500, 3, 3, 10), (200, 3, 1, 1), (130, 3, 2, 3), (500, 3, 5, 0), (500, 3, 0, 5), (64, 3, 1, 2),
              (65, 3, 1, 2)]
CONFIGS = {"small": CONFIGS_T3, "mid": [(500, 10, 10, 20), (500, 10, 3, 5)] + CONFIGS_T3}


def main():
    ref_psm, _, _ = mg._import_reference()
    for p in (REPO, os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.append(p)
    import earlystop_util as eu
    from oracle import oracle as orc

    for gname, configs in CONFIGS.items():
        pg, ga = mg.graph_arrays(gname)
        g = mg.stub_graph(pg)
        seed = SEEDS[gname]
        nodeset = np.random.default_rng(seed).integers(0, pg.n_tracks, N_SRC).astype(np.int64)
        out = dict(n_tracks=np.array(pg.n_tracks), n_cols=np.array(pg.n_cols), indptr=ga["indptr"],
                   indices=ga["indices"], nodeset=nodeset, seed=np.array(seed), alpha=np.array(ALPHA),
                   configs=np.array(configs, np.int64))
        mixed = all_stopped = False
        for c, (n_hops, T, stop_np, stop_nv) in enumerate(configs):
            assert T * 64 <= pg.n_tracks
            torch.manual_seed(seed)
            tk = ref_psm.sample_neighborhood_topt_early_stop(g, pg.n_tracks, torch.from_numpy(nodeset), n_hops, ALPHA,
                                                             T, stop_np, stop_nv)
            after = mg.next_draws()
            val, idx = tk.values.numpy(), tk.indices.numpy()
            assert val.dtype == np.float64 and idx.dtype == np.int64 and val.shape == (N_SRC, T)
            # the restatement gives the walk lengths (the reference returns none)
            torch.manual_seed(seed)
            mt = orc.MT.from_torch()
            r = eu.reference(ga["indptr"], ga["indices"], pg.n_tracks, nodeset, n_hops, ALPHA, T, stop_np, stop_nv,
                             mt=mt)
            mt.to_torch()
            assert (r["w"].view(np.uint64) == val.view(np.uint64)).all() and (r["nb"] == idx).all()
            assert (mg.next_draws() == after).all()
            n_stop = int(r["stopped"].sum())
            if stop_np == 0 or stop_nv == 0:
                assert n_stop == 0 and (r["hops"] == n_hops).all()
            mixed |= 0 < n_stop < N_SRC
            all_stopped |= n_stop == N_SRC
            out.update({f"c{c}_val": val, f"c{c}_idx": idx, f"c{c}_after": after, f"c{c}_hops": r["hops"]})
            print(f"{gname} {n_hops, T, stop_np, stop_nv}: stopped {n_stop} of {N_SRC}, L min / median / max "
                  f"{int(r['hops'].min())} / {int(np.median(r['hops']))} / {int(r['hops'].max())}")
        assert mixed, f"{gname}: no configuration with both stopped and unstopped sources"
        assert all_stopped, f"{gname}: no configuration with every source stopped"
        path = os.path.join(HERE, f"earlystop_{gname}.npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < (1 << 20), size
        print(f"wrote {path} ({size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
