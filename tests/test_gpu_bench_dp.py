"""bench.py's multi-process path as the driver launches it
(``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N``),
rehearsed with 2 ranks sharing cuda:0 over gloo (PINSAGE_DIST_BACKEND=gloo):
the run must exit 0 and rank 0 must print one JSON line for the whole job
(sharded precompute with its all-gather, data-parallel steps, max-over-ranks
timing), for both scaling modes."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_torchrun_two_ranks_gloo(scaling):
    env = dict(os.environ, PINSAGE_DIST_BACKEND="gloo", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--scaling", scaling]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 3 and res["value"] > 0
    assert res["scaling"] == scaling
    per_gpu = res["config"]["batch_per_gpu"]
    assert res["config"]["global_batch"] == (2 * per_gpu if scaling == "weak" else 512)
    # --full: the per-kernel timing pass ran and its figures are on the line
    assert res["full"] is True and res["kernels"] and res["roofline"]["avg_launch_ms"] > 0
    assert res["frontier"]["U0_mean"] > 0 and "cpu_baseline" in res


def test_gpus_two_without_launcher_starts_the_ranks(tmp_path):
    """`bench.py --gpus 2` run directly (no torch.distributed.run) starts the
    two ranks itself and still prints one whole-job JSON line with n_gpus 2.
    A plain run (no --full): the line carries the headline figures only, and
    --dump-outputs leaves the last step's outputs as float32 .npy files."""
    import numpy as np
    env = dict(os.environ, PINSAGE_DIST_BACKEND="gloo", OMP_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 3 and res["value"] > 0
    assert res["ms_per_step"] > 0 and res["full"] is False
    # value = target nodes / s and ms_per_step describe the same timed steps
    nodes = 3 * res["config"]["global_batch"]
    assert abs(res["value"] * res["ms_per_step"] * 1e-3 - nodes) <= 1e-9 * nodes
    for k in ("kernels", "roofline", "roofline_other", "gather_kernel", "frontier", "cpu_baseline"):
        assert k not in res, k
    files = {p.name: np.load(p) for p in dump.iterdir()}
    assert {"loss.npy", "param.G1.weight.npy", "param.conv_layers.0.Q.weight.npy"} <= set(files), sorted(files)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["loss.npy"].shape == (1,) and files["loss.npy"][0] >= 0
    assert files["param.conv_layers.0.Q.weight.npy"].shape == (512, 512)
