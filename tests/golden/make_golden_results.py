"""Generate tests/golden/results_table.npz by running the REAL reference's
low_co_accuracy (eval.py:391-406) and compute_results_table (eval.py:413-443)
on the inputs of make_golden_eval.make_inputs().

Runs only where the reference checkout is (as make_golden_eval.py does, with
the same stub imports; no test needs it).  Only results are stored; the tests
rebuild the inputs from eval_metrics.npz, which holds the same make_inputs().

low_co_accuracy runs at co_thr in {0, 1, 2, 1000} with mrr at K = 1000 and
hit_rate at K = 10.  A query of a pair occurs in at least one pair, so co_thr =
0 keeps nothing and the reference divides by zero: ``low_co_raises`` records
that, and the value stored there is NaN.  The table is computed over a
two-model dict with known times: "first" is make_inputs()' id matrix, "second"
the same matrix with every row reversed.

    python tests/golden/make_golden_results.py
"""
from __future__ import annotations

import os

import numpy as np
import torch

from make_golden_eval import DegreeGraph, _import_reference_eval, make_inputs

HERE = os.path.dirname(os.path.abspath(__file__))

CO_THRS = (0, 1, 2, 1000)
TIMES = {"first": (1.5, 0.25, 3.0), "second": (0, 0, 0)}


class KnnDict(dict):
    """name -> (weights, id matrix), answering get_times as LazyKnnDict does."""

    def get_times(self, name):
        return TIMES[name]


def main():
    ref = _import_reference_eval()
    knn, pairs, deg = make_inputs()
    km, tp, g = torch.from_numpy(knn), torch.from_numpy(pairs), DegreeGraph(deg)
    out = dict(co_thrs=np.array(CO_THRS))
    for name, func, K in (("low_co_mrr_1000", ref.mrr, 1000), ("low_co_hit_rate_10", ref.hit_rate, 10)):
        vals, raises = [], []
        for thr in CO_THRS:
            try:
                vals.append(ref.low_co_accuracy(km, g, tp, K, co_thr=thr, acc_func=func))
                raises.append(False)
            except ZeroDivisionError:
                vals.append(float("nan"))
                raises.append(True)
        out[name] = np.array(vals, np.float64)
        out["low_co_raises"] = np.array(raises)
    models = KnnDict(first=(None, km), second=(None, torch.from_numpy(knn[:, ::-1].copy())))
    table = ref.compute_results_table(models, tp, g, times=True, degree_thr=1)
    out["table_columns"] = np.array(list(table.columns))
    out["table_index"] = np.array(list(table.index))
    out["table_values"] = table.to_numpy(dtype=np.float64)
    no_times = ref.compute_results_table(models, tp, g, times=False, degree_thr=0)
    out["table_no_times_columns"] = np.array(list(no_times.columns))
    out["table_no_times_values"] = no_times.to_numpy(dtype=np.float64)
    path = os.path.join(HERE, "results_table.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
    print(table.to_string())
    for k in ("low_co_mrr_1000", "low_co_hit_rate_10", "low_co_raises"):
        print(k, out[k].tolist())


if __name__ == "__main__":
    main()
