"""GPU: the data-parallel launch path of bench.py -- RCCL collectives (SyncBatchNorm statistics + the flat gradient
all-reduce) captured INSIDE the hipGraph of the whole step and replayed -- exercised on one GPU with a 1-rank process
group (OMNIPQ_BENCH_FORCE_DIST=1), so that every round's driver run covers the graph-with-collectives path that the
8-GPU scaling run depends on (reference: DistributedDataParallel + SyncBatchNorm, train.py:382, pq_transformer.py:194).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(port, dump_dir):
    env = dict(os.environ, OMNIPQ_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0",
               WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "4", "--warmup", "2",
                          "--no-cpu-baseline", "--no-op-timing", "--points", "20000", "--batch", "4",
                          "--dump-outputs", dump_dir],
                         env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        return None, out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


def test_step_with_rccl_collectives_captures_and_replays(tmp_path):
    # ONE attempt: the capture no longer races the process groups' watchdogs (train_step._quiesce_process_groups; round 3
    # this test retried up to three times)
    rec, err = run_bench(29641, str(tmp_path))
    errs = [err[-3000:]]
    assert rec is not None, errs
    assert rec["n_gpus"] == 1 and rec["value"] > 0
    # the probe passed and the captured step holds the collectives
    assert rec["launch"] == "hipGraph replay", (rec["launch"], errs)
    assert rec["data_parallel"] and "inside the graph" in rec["data_parallel"], rec["data_parallel"]
    # 88 SyncBatchNorm statistics exchanges (61 layers, forward + backward = 122, minus the 28 the seven object / quad head pairs and the 6 the three pairs of key-position embeddings share) and the two gradient buckets
    assert "88 SyncBN" in rec["data_parallel"] and "2 gradient-bucket" in rec["data_parallel"], rec["data_parallel"]
    # the vote aggregation's three conv weights get their gradients after the early flush: they travel with bucket 1
    assert "the 3 bucket-0 gradients that arrive after that flush" in rec["data_parallel"], rec["data_parallel"]
    # --dump-outputs: what the last replayed step handed its caller
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float32 and np.isfinite(loss).all()
    inds = np.load(tmp_path / "end_points.sa1_inds.npy")
    assert inds.dtype == np.float64 and inds.shape == (4, 2048) and inds.min() >= 0 and inds.max() < 20000
    grads = [n for n in os.listdir(tmp_path) if n.startswith("grad.")]
    assert len(grads) > 100 and all(np.isfinite(np.load(tmp_path / n)).all() for n in grads)
