"""Time one fairness-regularised training step (mpvae_step.FairTrainStep,
mpv_group_rows and mpv_label_weights_batch in csrc/fairness.hip) against the
hand-composed step it replaces:

    python tools/bench_fair_step.py [--out profiles/fair_step_bench.json] [--steps 50]

Shapes: C1 (B 32, S 10) and C2 (B 128, S 1000), both L = z = 38, F 1000, d 50,
G = 4 sensitive groups, each with T = 1 and T = 3 target tables.  Per shape,
in one process on one device, four variants alternate over ``--rounds``
rounds of ``--steps`` steps each:

  a  the hand-composed eager step of INTEGRATION.md: compute_loss,
     ``fairness_penalty(fused=False)``, backward, ``clip_grad_norm_``,
     ``has_finite_grad`` (a host sync), the optimizer and scheduler steps on
     the host, ``compute_metrics``, ``step_scalars`` (a second sync);
  b  FairTrainStep's body with the unfused penalty (``step.fused = False``: one
     label_weights launch per table, the groups from torch ops), captured in a
     HIP graph -- the yardstick of d;
  c  FairTrainStep eager;
  d  FairTrainStep captured.

Recorded: wall ms per step (host clock around the steps, device synchronised
before and after) of every round, their median and range, and device launches
per step (torch.profiler); and the launches of the grouping plus the weights
alone, fused and unfused.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpvae-1_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpvae  # noqa: E402
import mpvae_fair as mf  # noqa: E402
import mpvae_hip as H  # noqa: E402
import mpvae_step as ms  # noqa: E402

DEV = "cuda:0"
SHAPES = [dict(name="c1", B=32, S=10, L=38, F=1000, d=50),
          dict(name="c2", B=128, S=1000, L=38, F=1000, d=50)]
G, COEFF, LR = 4, 1.0, 7.5e-4


def build(sh, T, seed=0):
    """One model, optimizer, scheduler and batch; the same for every variant."""
    L = sh["L"]
    a = argparse.Namespace(feature_dim=sh["F"], latent_dim=sh["d"], label_dim=L, z_dim=L,
                           keep_prob=0.5, scale_coeff=1.0, residue_sigma="",
                           n_train_sample=sh["S"], n_test_sample=sh["S"], mode="train",
                           nll_coeff=0.5, c_coeff=10.0, mpvae_noise="philox",
                           mpvae_seed=torch.tensor([seed + 1], dtype=torch.int64, device=DEV),
                           fair_coeff=COEFF, fairness_loss_norm="l2")
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = mpvae.VAE(a).to(DEV).train()
    rng = np.random.default_rng(seed)
    labels = (rng.random((sh["B"], L)) < 0.1).astype(np.int64)
    labels[:, 0], labels[:, 1] = 1, 0
    cents = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int64)
    sens = cents[rng.integers(0, G, sh["B"])]
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[t::T + 1]}
             for t in range(T)]
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in dists]
    feat = rng.standard_normal((sh["B"], sh["F"])).astype(np.float32)
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=1e-5, fused=True,
                           capturable=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, 10 ** 6, 0.5)
    batch = (torch.from_numpy(labels).float().to(DEV), torch.from_numpy(feat).to(DEV),
             torch.from_numpy(sens).to(DEV))
    return a, model, opt, sched, tables, batch


def hand_step(a, model, opt, sched, tables, batch):
    """INTEGRATION.md's hand-composed step, host syncs included."""
    label, feat, sens = batch
    a.mpvae_seed_advance = True
    opt.zero_grad()
    res = mpvae.compute_loss(label, *model(label, feat), model.r_sqrt_sigma, a)
    total = res[0]
    fair, n = mf.fairness_penalty(res[7], res[6], label, sens, tables, a.fairness_loss_norm,
                                  a.fair_coeff, max_groups=G)
    total = total + fair
    total.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
    if ms.has_finite_grad(model):
        opt.step()
        sched.step()
    m = mf.compute_metrics(res[6], label, 0.5)
    return ms.step_scalars(nll=res[1], nll_x=res[2], c=res[3], c_x=res[4], kl=res[5], total=total,
                           fair=fair, ma=m["maF1"], mi=m["miF1"], n=n)


def wall_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def launches(fn, steps=5):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    n = sum(e.count for e in prof.key_averages()
            if (getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)))
    return round(n / steps, 1)


def one_config(sh, T, steps, rounds):
    variants = {}
    a, model, opt, sched, tables, batch = build(sh, T)
    variants["a_hand_eager"] = lambda: hand_step(a, model, opt, sched, tables, batch)
    for key, fused, captured in (("b_unfused_graph", False, True), ("c_fair_step_eager", True, False),
                                 ("d_fair_step_graph", True, True)):
        a2, m2, o2, s2, t2, b2 = build(sh, T)
        step = ms.FairTrainStep(m2, o2, a2, t2, max_groups=G, scheduler=s2)
        step.fused = fused
        if captured:
            step.capture(*b2)
        variants[key] = (lambda st, bt: lambda: st(*bt))(step, b2)
    for fn in variants.values():  # warm every variant
        for _ in range(3):
            fn()
    ms_rounds = {k: [] for k in variants}
    for _ in range(rounds):  # alternate, so that drift of the box hits all alike
        for k, fn in variants.items():
            ms_rounds[k].append(wall_ms(fn, steps))
    res = {"shape": dict(sh, G=G, T=T), "steps": steps, "rounds": rounds}
    for k, fn in variants.items():
        v = ms_rounds[k]
        res[k] = {"ms_rounds": v, "ms_median": statistics.median(v), "ms_min": min(v),
                  "ms_max": max(v), "launches": launches(fn)}
    # the grouping plus the weights alone
    label, _, sens = batch
    fused_n = launches(lambda: (mf.label_weights_batch(label, tables), mf.group_rows(sens, G)))
    unfused_n = launches(lambda: (mf.label_weights(label, tables), mf.sensitive_groups(sens, G)))
    # label_weights* zero their count with one torch fill on top of the kernels
    want = 1 + -(-T // H.LABEL_TABLES_PER_LAUNCH)
    assert fused_n == want + 1, (fused_n, want)
    res["groups_and_weights_launches"] = {"fused_kernels": want, "fused_with_count_fill": fused_n,
                                          "unfused_with_count_fill": unfused_n}
    b, d = res["b_unfused_graph"], res["d_fair_step_graph"]
    spread = max(b["ms_max"] - b["ms_min"], d["ms_max"] - d["ms_min"])
    res["d_minus_b_ms"] = d["ms_median"] - b["ms_median"]
    res["spread_ms"] = spread
    res["d_not_slower_than_b_beyond_spread"] = d["ms_median"] <= b["ms_median"] + spread
    res["a_over_d"] = res["a_hand_eager"]["ms_median"] / d["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fair_step_bench.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c2")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fair_step.py needs a GPU")
    if cli.rounds < 5:
        raise SystemExit("at least five rounds: the spread is part of the result")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "ms: host wall clock per step over `steps` calls, device synchronised before "
                   "and after, after warm-up, one figure per round, the variants alternating; "
                   "launches: device kernels per step (torch.profiler); a: the hand-composed "
                   "eager step (fused=False, has_finite_grad, step_scalars); b: FairTrainStep's "
                   "body with the unfused penalty in a HIP graph; c / d: FairTrainStep eager / "
                   "in a HIP graph; spread_ms: the larger max - min over the rounds of b and d",
           "configs": [one_config(sh, T, cli.steps, cli.rounds) for sh in SHAPES
                       if sh["name"] in cli.shapes.split(",") for T in (1, 3)]}
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
