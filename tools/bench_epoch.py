"""Time one epoch of the captured FairTrainStep under three ways of feeding it
its batches (mpvae_step.DeviceSplit, TrainStep.run_epoch, csrc/gather.hip):

    python tools/bench_epoch.py [--out profiles/epoch_bench.json] [--rounds 5]

Shapes: tools/bench_fair_step.py's C1 (B 32, S 10) and C2 (B 128, S 1000), both
L = z = 38, F 1000, d 50, with T = 3 target tables and G = 4 sensitive groups;
the split has N = 100 B + 37 rows (full batches and a ragged last one), fp32
features, fp32 0/1 labels, int64 sensitive columns.  Per shape, in one process
on one device, three feeds alternate over ``--rounds`` rounds of one epoch each,
every epoch over a fresh permutation:

  a  the reference's feeding (fairsoft_train.py:48-56): per batch
     ``torch.from_numpy(data[idx]).float().to(device)`` for the labels, the
     features and the sensitive columns, into the captured ``step()`` (three
     ``copy_`` and a replay);
  b  what a careful user could do before run_epoch: the split as fp32 device
     tensors, the order uploaded once per epoch, ``index_select`` per batch
     into the captured ``step()``;
  c  ``run_epoch`` on the epoch graph (``capture_epoch``): one replay per full
     batch, the gather a node of the graph.

a and b run code paths that predate run_epoch; they are the yardsticks.  In all
three the ragged last batch runs eagerly (a captured step has one batch size).
Recorded: wall ms per epoch (host clock, device synchronised before and after)
of every round, the median and range, the same per step, and the device
activities (kernels and copies, torch.profiler) per full-batch step.  Needs a
GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpvae-1_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpvae  # noqa: E402
import mpvae_fair as mf  # noqa: E402
import mpvae_step as ms  # noqa: E402
from bench_fair_step import DEV, G, LR, SHAPES, launches  # noqa: E402

T, FULL, TAIL = 3, 100, 37


def build(sh, data, seed=0):
    """A FairTrainStep on a fresh model: the same for every feed."""
    L = sh["L"]
    a = argparse.Namespace(feature_dim=sh["F"], latent_dim=sh["d"], label_dim=L, z_dim=L,
                           keep_prob=0.5, scale_coeff=1.0, residue_sigma="",
                           n_train_sample=sh["S"], n_test_sample=sh["S"], mode="train",
                           nll_coeff=0.5, c_coeff=10.0, mpvae_noise="philox",
                           mpvae_seed=torch.tensor([seed + 1], dtype=torch.int64, device=DEV),
                           fair_coeff=1.0, fairness_loss_norm="l2")
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = mpvae.VAE(a).to(DEV).train()
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in data["dists"]]
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=1e-5, fused=True,
                           capturable=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, 10 ** 6, 0.5)
    return ms.FairTrainStep(model, opt, a, tables, max_groups=G, scheduler=sched)


def make_data(sh, seed=0):
    rng = np.random.default_rng(seed)
    n, L = FULL * sh["B"] + TAIL, sh["L"]
    labels = (rng.random((n, L)) < 0.1).astype(np.float32)
    labels[:, 0], labels[:, 1] = 1, 0
    cents = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int64)
    rows = labels.astype(np.int64)
    return dict(n=n, labels=labels, feats=rng.standard_normal((n, sh["F"])).astype(np.float32),
                sens=cents[rng.integers(0, G, n)],
                dists=[{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1))
                        for r in rows[t::T + 1]} for t in range(T)])


def batches(n, B):
    for i in range(n // B + 1):
        s, e = i * B, min((i + 1) * B, n)
        if e > s:
            yield s, e


def feeds(sh, data):
    """name -> (epoch(order) -> steps, one full-batch step for the launch count)."""
    B, n = sh["B"], data["n"]
    first = np.arange(B)
    host = lambda idx: (torch.from_numpy(data["labels"][idx]).float().to(DEV),  # noqa: E731
                        torch.from_numpy(data["feats"][idx]).float().to(DEV),
                        torch.from_numpy(data["sens"][idx]).to(DEV))
    out = {}

    # a: the reference's feeding
    step_a = build(sh, data)
    step_a.capture(*host(first))

    def epoch_a(order):
        k = 0
        for s, e in batches(n, B):
            batch = host(order[s:e])
            if e - s == B:
                step_a(*batch)
            else:  # a captured step has one batch size: the ragged batch runs eagerly
                step_a._body(*batch)
            k += 1
        return k
    out["a_host_fed"] = (epoch_a, lambda: step_a(*host(first)))

    # b: device-resident fp32 tensors, index_select per batch
    step_b = build(sh, data)
    dev = host(np.arange(n))
    step_b.capture(*[t[:B] for t in dev])

    def pick(idx):
        return tuple(t.index_select(0, idx) for t in dev)

    def epoch_b(order):
        idx = torch.from_numpy(order).to(DEV)
        k = 0
        for s, e in batches(n, B):
            batch = pick(idx[s:e])
            if e - s == B:
                step_b(*batch)
            else:
                step_b._body(*batch)
            k += 1
        return k
    idx0 = torch.from_numpy(first).to(DEV)
    out["b_index_select"] = (epoch_b, lambda: step_b(*pick(idx0)))

    # c: run_epoch on the epoch graph
    step_c = build(sh, data)
    split = ms.DeviceSplit(data["labels"], data["feats"], data["sens"], device=DEV)
    step_c.capture_epoch(split, B)

    def one_replay():
        split.cursor.zero_()
        step_c._epoch.graph.replay()
    out["c_run_epoch"] = (lambda order: step_c.run_epoch(split, order, B), one_replay)
    return out, split


def one_shape(sh, rounds):
    data = make_data(sh)
    fs, split = feeds(sh, data)
    rng = np.random.default_rng(1)
    # C1 (B 32): the 37 rows past 100 B are one more full batch and 5 ragged rows
    full, tail = ms.epoch_batches(data["n"], sh["B"])
    steps = full + (1 if tail else 0)
    for epoch, _ in fs.values():  # warm every feed, ragged shapes included
        assert epoch(rng.permutation(data["n"])) == steps
    ms_rounds = {k: [] for k in fs}
    for _ in range(rounds):  # alternate, so that drift of the box hits all alike
        order = rng.permutation(data["n"])
        for k, (epoch, _) in fs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(order)
            torch.cuda.synchronize()
            ms_rounds[k].append((time.perf_counter() - t0) * 1e3)
    split.check()
    res = {"shape": dict(sh, G=G, T=T, N=data["n"]), "steps_per_epoch": steps, "rounds": rounds}
    for k, (_, step) in fs.items():
        v = ms_rounds[k]
        res[k] = {"epoch_ms_rounds": v, "epoch_ms_median": statistics.median(v),
                  "epoch_ms_min": min(v), "epoch_ms_max": max(v),
                  "step_ms_median": statistics.median(v) / steps,
                  "device_activities_per_full_step": launches(step)}
    # c's count includes the cursor reset of the probe (one fill), not part of an epoch step
    res["c_run_epoch"]["device_activities_per_full_step"] -= 1
    b, c = res["b_index_select"], res["c_run_epoch"]
    spread = max(x["epoch_ms_max"] - x["epoch_ms_min"] for x in (res["a_host_fed"], b, c))
    res["spread_ms"] = spread
    res["b_minus_c_ms"] = b["epoch_ms_median"] - c["epoch_ms_median"]
    res["a_minus_c_ms"] = res["a_host_fed"]["epoch_ms_median"] - c["epoch_ms_median"]
    res["c_ahead_of_b_beyond_spread"] = res["b_minus_c_ms"] > spread
    res["c_ahead_of_a_beyond_spread"] = res["a_minus_c_ms"] > spread
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c2")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch.py needs a GPU")
    if cli.rounds < 5:
        raise SystemExit("at least five rounds: the spread is part of the result")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "epoch_ms: host wall clock around one epoch (N = 100 B + 37 rows: the full "
                   "batches and a ragged last one), device synchronised before and after, "
                   "after one warm-up epoch per feed, one figure per round, the feeds alternating on the same "
                   "order; a: the reference's per-batch from_numpy(data[idx]).float().to(device) "
                   "into the captured step; b: device-resident fp32 tensors and index_select "
                   "per batch into the captured step; c: run_epoch on the epoch graph; "
                   "device_activities_per_full_step: kernels and copies of one full-batch step "
                   "(torch.profiler); spread_ms: the largest max - min over the rounds of a "
                   "feed",
           "configs": [one_shape(sh, cli.rounds) for sh in SHAPES
                       if sh["name"] in cli.shapes.split(",")]}
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
