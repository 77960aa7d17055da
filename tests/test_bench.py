"""bench.py's command line: a plain run is the timed steps alone (the CPU
baseline and elbo_rel_err belong to --full), --steps sets the timed steps, and
--dump-outputs writes what the last timed step returned."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tolerances import FWD_RTOL, GRAD_RTOL, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 1


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """One plain C2 run with --dump-outputs: the line holds ms_per_step of the
    requested steps and no CPU baseline; every dumped array is float32 /
    float64 and equals a second evaluation of the same step (bench.make_inputs
    and the last timed step's Philox key) within the tolerances that two fp32
    implementations are held to (tests/tolerances.py): the same kernels twice
    differ by the order of their atomic sums at most."""
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(STEPS), "--warmup", str(WARMUP), "--config", "c2",
                        "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0 and line["loss_finite"]
    assert line["value"] == pytest.approx(1000 * 128 * 38 / (line["ms_per_step"] * 1e-3))
    assert line["cpu_baseline"] is None and line["elbo_rel_err"] is None

    import bench
    L, z, B, S, d, nllc, cc = bench.CONFIGS["c2"]
    args = argparse.Namespace(label_dim=L, z_dim=z, n_train_sample=S, n_test_sample=S,
                              mode="train", nll_coeff=nllc, c_coeff=cc, mpvae_noise="philox",
                              mpvae_shard=False, mpvae_force_exchange=False, mpvae_gemm="f16x3")
    y, leaves = bench.make_inputs(L, z, B, d, torch.device("cuda", 0))
    out = bench.step(y, leaves, args, 1000 + STEPS - 1)
    torch.cuda.synchronize()
    want = dict(zip(bench.OUT_NAMES, out))
    want.update({"grad_" + k: leaves[k].grad for k in bench.ORDER})
    assert sorted(os.listdir(dump)) == sorted(k + ".npy" for k in want)
    total = 0
    for k, t in want.items():
        a = np.load(dump / (k + ".npy"))
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64), (k, a.dtype)
        assert a.shape == tuple(t.shape), (k, a.shape)
        tol = GRAD_RTOL if k.startswith("grad_") else FWD_RTOL
        assert rel_err(a, t.detach().cpu().numpy()) <= tol, k
    assert total <= 64 << 20


def test_large_arrays_are_dumped_as_a_fixed_sample(tmp_path, monkeypatch):
    """Above DUMP_MAX_ELEMS an array is written as the same seeded sample of its
    flattened elements on every call, in its own dtype."""
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    out = [torch.arange(1000, dtype=torch.float64).reshape(10, 100)] + \
        [torch.zeros(())] * 7
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), out, {}, train=False)
    a, b = np.load(tmp_path / "a" / "total.npy"), np.load(tmp_path / "b" / "total.npy")
    assert a.dtype == np.float64 and a.shape == (100,) and np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() <= 999
    assert np.load(tmp_path / "a" / "kl.npy").shape == ()
