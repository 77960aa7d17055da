"""Time the per-step random r_sqrt_sigma of ``residue_sigma == "random"``
(``args.mpvae_r_draw``; mpv_r_uniform_philox in csrc/util.hip) inside the
training step:

    python tools/bench_r_draw.py [--out profiles/r_draw_bench.json] [--steps 50]

Shapes: the C1 (B 32, S 10) and C2 (B 128, S 1000) training shapes of
profiles/r06_trainstep.json, both L = z = 38, F 1000, d 50; a 'random' model,
Philox probit noise keyed by a device seed.  Per shape, in one process on one
device, the variants alternate over ``--rounds`` rounds of ``--steps`` steps:

  a  TrainStep captured in a HIP graph with the model's frozen r_sqrt_sigma
     (no knob: the code path before the knob existed);
  b  the same with ``mpvae_r_draw = "philox"``: one more graph node;
  c  the eager TrainStep with ``mpvae_r_draw = "numpy"``, the reference's host
     draw and upload every step;
  e  the eager TrainStep with the frozen r_sqrt_sigma (what c adds its draw to).

Recorded: device ms per step (a HIP event pair round the steps of a round) of
every round, their median and range; and the draw kernel alone (ms per launch
over 200 back-to-back launches between one event pair, and the library's own
per-launch events).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpvae-1_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpvae  # noqa: E402
import mpvae_hip as H  # noqa: E402
import mpvae_step as ms  # noqa: E402

DEV = "cuda:0"
SHAPES = [dict(name="c1", B=32, S=10, L=38, F=1000, d=50),
          dict(name="c2", B=128, S=1000, L=38, F=1000, d=50)]
LR = 7.5e-4


def build(sh, r_draw, seed=0):
    """One 'random' model, optimizer and batch; the same for every variant."""
    L = sh["L"]
    a = argparse.Namespace(feature_dim=sh["F"], latent_dim=sh["d"], label_dim=L, z_dim=L,
                           keep_prob=0.5, scale_coeff=1.0, residue_sigma="random",
                           n_train_sample=sh["S"], n_test_sample=sh["S"], mode="train",
                           nll_coeff=0.5, c_coeff=10.0, mpvae_noise="philox",
                           mpvae_seed=torch.tensor([seed + 1], dtype=torch.int64, device=DEV),
                           mpvae_r_draw=r_draw)
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = mpvae.VAE(a).to(DEV).train()
    rng = np.random.default_rng(seed)
    labels = (rng.random((sh["B"], L)) < 0.1).astype(np.float32)
    labels[:, 0], labels[:, 1] = 1, 0
    feat = rng.standard_normal((sh["B"], sh["F"])).astype(np.float32)
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=1e-5, fused=True,
                           capturable=True)
    batch = (torch.from_numpy(labels).to(DEV), torch.from_numpy(feat).to(DEV))
    return ms.TrainStep(model, opt, a), batch


def device_ms(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def draw_alone(sh, launches=200):
    a = argparse.Namespace(label_dim=sh["L"], z_dim=sh["L"], mpvae_r_draw="philox",
                           mpvae_seed=torch.tensor([7], dtype=torch.int64, device=DEV))
    out = torch.empty((sh["L"], sh["L"]), dtype=torch.float64, device=DEV)
    draw = lambda: mpvae.draw_r_sqrt_sigma(a, DEV, out=out)  # noqa: E731
    for _ in range(10):
        draw()
    back_to_back = [device_ms(draw, launches) for _ in range(5)]
    lib = H.load_library()
    lib.mpv_timing_enable(1)
    try:
        lib.mpv_timing_reset()
        for _ in range(launches):
            draw()
        n, total = H.kernel_times()["r_uniform"]
    finally:
        lib.mpv_timing_enable(0)
        lib.mpv_timing_reset()
    return {"launches": launches, "ms_per_launch_back_to_back_rounds": back_to_back,
            "ms_per_launch_back_to_back_median": statistics.median(back_to_back),
            "ms_per_launch_own_events": total / n}


def one_config(sh, steps, rounds):
    variants = {}
    for key, r_draw, captured in (("a_frozen_graph", None, True), ("b_philox_graph", "philox", True),
                                  ("c_numpy_eager", "numpy", False),
                                  ("e_frozen_eager", None, False)):
        step, batch = build(sh, r_draw)
        if captured:
            step.capture(*batch)
        variants[key] = (lambda st, bt: lambda: st(*bt))(step, batch)
    for fn in variants.values():  # warm every variant
        for _ in range(3):
            fn()
    ms_rounds = {k: [] for k in variants}
    for _ in range(rounds):  # alternate, so that drift of the box hits all alike
        for k, fn in variants.items():
            ms_rounds[k].append(device_ms(fn, steps))
    res = {"shape": sh, "steps": steps, "rounds": rounds}
    for k, v in ms_rounds.items():
        res[k] = {"ms_rounds": v, "ms_median": statistics.median(v), "ms_min": min(v),
                  "ms_max": max(v)}
    res["draw_kernel"] = draw_alone(sh)
    a, b = res["a_frozen_graph"], res["b_philox_graph"]
    res["b_minus_a_ms"] = b["ms_median"] - a["ms_median"]
    res["a_spread_ms"] = a["ms_max"] - a["ms_min"]
    res["allowance_ms"] = res["a_spread_ms"] + res["draw_kernel"]["ms_per_launch_own_events"]
    res["b_within_a_spread_plus_draw"] = res["b_minus_a_ms"] <= res["allowance_ms"]
    res["c_minus_e_ms"] = res["c_numpy_eager"]["ms_median"] - res["e_frozen_eager"]["ms_median"]
    res["c_over_b"] = res["c_numpy_eager"]["ms_median"] / b["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r_draw_bench.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c2")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_r_draw.py needs a GPU")
    if cli.rounds < 5:
        raise SystemExit("at least five rounds: the spread is part of the result")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "ms: device time per step, one HIP event pair round the `steps` calls of a "
                   "round (host time the device waits for is inside it), after warm-up, one "
                   "figure per round, the variants alternating; a: captured TrainStep, the "
                   "model's frozen r_sqrt_sigma; b: captured, mpvae_r_draw='philox'; c: eager, "
                   "mpvae_r_draw='numpy' (host draw + upload); e: eager, frozen; Philox probit "
                   "noise in all four; allowance_ms: a's max - min over the rounds plus the draw "
                   "kernel's own per-launch time",
           "configs": [one_config(sh, cli.steps, cli.rounds) for sh in SHAPES
                       if sh["name"] in cli.shapes.split(",")]}
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
