"""SHA-256 digests of what the transposed aggregation (csrc/dq.hip, through
pinsage_agg_transpose) writes for fixed, seeded inputs:

    [PINSAGE_LIB=other/libpinsage_hip.so] python tools/dq_bits.py

prints one JSON line {case: digest, "all": the digest of them all}.  Two builds
compute the same bits exactly when their lines are equal; there is no reference
and no tolerance here.  Run each build in a process of its own.  The tables and
the launch are tests/test_gpu_dq.py's: its main table (q rows of 1 .. 8193
occurrences) at hid 16, 256, 512 in mode 0 (combine kernel), mode 1 (split-row
tree) and mode 1 with the planes output, hid 516 in mode 0 (the column loop),
and its regime tables of 4096, 4097, 40960 and 40961 q rows, the last also with
PINSAGE_CSR_RANGES=0, at hid 16 in the same three forms.  Inputs are random
(normalised weights, normal dagg), so every summation order shows in the bits;
rows that occur in no slot keep the output's NaN pre-fill.
"""
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "gcn-song-embeddings_amd")):
    sys.path.insert(0, p)

import test_gpu_dq as tq  # noqa: E402

FORMS = (("combine", 0, False), ("tree", 1, False), ("tree+planes", 1, True))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def case(out, name, table, hid, forms, seed):
    counts, loc_np = table
    loc = torch.from_numpy(loc_np).cuda()
    n_rows, T = loc.shape
    w, dagg, q = tq._random_inputs(n_rows, T, len(counts), hid, hid, seed=seed)
    for form, mode, planes in forms:
        out[f"{name}_hid{hid}_{form}"] = digest(tq._run(loc, w, dagg, q, mode, planes=planes))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dq_bits needs the GPU")
    out = {}
    for hid in (16, 256, 512):
        case(out, "main", tq._main_table(), hid, FORMS, seed=hid)
    case(out, "main", tq._main_table(), 516, FORMS[:1], seed=516)
    for U, ranges in ((4096, None), (4097, None), (40960, None), (40961, None), (40961, "0")):
        if ranges is not None:
            os.environ["PINSAGE_CSR_RANGES"] = ranges  # read per call
        case(out, f"U{U}" + (f"_ranges{ranges}" if ranges is not None else ""), tq._regime_table(U), 16, FORMS, seed=U)
        os.environ.pop("PINSAGE_CSR_RANGES", None)
    out["all"] = hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest()  # of the cases above
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
