"""Time one post-process calibration step (mpvae_step.CalibrationStep,
csrc/calib.hip) against the loop body it replaces:

    python tools/bench_calib.py [--out profiles/calib_bench.json] [--steps 20]

Two shapes: B 128, S 1000, L = z = 38 (C2) and B 512, S 4096, L = z = 1024 (C4),
G = 4 sensitive groups, T = 1 target.  Per shape:

  * ``CalibrationStep`` eager and captured in a HIP graph: wall time per step
    (host clock around ``steps`` calls, device synchronised before and after)
    and device launches per step (torch.profiler);
  * the baseline, in the same process on the same device: the loop body of
    postprocess_threshold_one_epoch (fairsoft_train_postprocess.py:84-186)
    restated with torch ops as the reference runs it -- ``compute_loss`` with
    grad enabled and a full backward through it and the model, the per-row
    string-dict lookups on the host, ``torch.unique``, the ``weights.sum() >
    0`` branches, ``has_finite_grad`` and five ``.item()`` calls.  It calls
    this project's ``compute_loss`` and VAE, so the difference is the
    calibration path, not the probit kernels.

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpvae-1_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpvae  # noqa: E402
import mpvae_fair as mf  # noqa: E402
import mpvae_step  # noqa: E402

DEV = "cuda:0"
SHAPES = [dict(name="c2", B=128, S=1000, L=38, F=1000, d=50),
          dict(name="c4", B=512, S=4096, L=1024, F=1000, d=50)]
G, COEFF, LR = 4, 1.0, 7.5e-4


def build(sh, seed=0):
    L = sh["L"]
    a = argparse.Namespace(feature_dim=sh["F"], latent_dim=sh["d"], label_dim=L, z_dim=L,
                           keep_prob=0.5, scale_coeff=1.0, residue_sigma="",
                           n_train_sample=sh["S"], n_test_sample=sh["S"], mode="train",
                           nll_coeff=0.5, c_coeff=10.0, mpvae_noise="philox",
                           mpvae_seed=torch.tensor([seed + 1], dtype=torch.int64, device=DEV),
                           fair_coeff=COEFF, learn_logit=True)
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = mpvae.VAE(a).to(DEV).eval()
    rng = np.random.default_rng(seed)
    labels = (rng.random((sh["B"], L)) < 0.1).astype(np.int64)
    labels[:, 0], labels[:, 1] = 1, 0
    labels[sh["B"] // 2:] = labels[:sh["B"] - sh["B"] // 2]
    cents = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int64)
    sens = cents[rng.integers(0, G, sh["B"])]
    dist = {"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[::2]}
    feat = rng.standard_normal((sh["B"], sh["F"])).astype(np.float32)
    thr = rng.uniform(0.45, 0.55, (1, L, G)).astype(np.float32)
    x = torch.from_numpy(np.log(thr / (1 - thr))).to(DEV).requires_grad_(True)
    opt = torch.optim.Adam([x], lr=LR, weight_decay=1e-5, fused=True, capturable=True)
    data = dict(labels=labels, sens=sens, cents=cents, dist=dist, feat=feat)
    return a, model, x, opt, data


def wall_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def launches(fn, steps=5):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages()
                if (getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)))
        return round(n / steps, 1)
    except Exception as e:  # profiler unavailable: say why
        return "profiler: " + repr(e)[:200]


def baseline_step(a, model, x, opt, data):
    """The reference's loop body in torch ops, host work included."""
    eps = 1e-6
    opt.zero_grad()
    y = torch.from_numpy(data["labels"]).float().to(DEV)
    feat = torch.from_numpy(data["feat"]).float().to(DEV)
    res = mpvae.compute_loss(y, *model(y, feat), model.r_sqrt_sigma, a)  # grad enabled
    total, p = res[0], res[6]
    sens = torch.from_numpy(data["sens"]).to(DEV)
    cents = torch.from_numpy(data["cents"]).to(DEV)
    belong = (sens[:, None, :] == cents).all(2)
    thr = 1 / (torch.exp(-x) + 1) if a.learn_logit else x
    lg = lambda v: torch.log(v / (1 - v + eps))
    q = (1 / (torch.exp(-(lg(p.unsqueeze(-1)) - lg(thr))) + 1)).transpose(1, 2)[belong]
    bce = -(y * torch.log(q + eps) + (1 - y) * torch.log(1 - q + eps)).sum(1).mean()
    groups = torch.unique(sens, dim=0)
    rows = torch.arange(sens.shape[0])
    fair, contributed = 0.0, 0
    wts = []
    for row in data["labels"]:  # the host dict lookup per row
        v = data["dist"].get("".join(row.astype(int).astype(str)), 0.0)
        contributed += v > 0
        wts.append(v)
    wts = torch.tensor(wts).to(DEV).reshape(-1, 1)
    if wts.sum() > 0:
        mean_all = (q * wts).sum(0) / wts.sum()
        for g in groups:
            sel = rows[(sens == g).all(1).cpu()]
            wk = wts[sel]
            if wk.sum() > 0:
                fair = fair + (((q[sel] * wk).sum(0) / wk.sum() - mean_all) ** 2).sum()
    logged = []
    if not isinstance(fair, float):
        total = fair * a.fair_coeff + bce
        logged.append(fair.item())
    total.backward()
    g = x.grad
    if g is not None and not (torch.isnan(g).any() or torch.isinf(g).any()):
        opt.step()
    logged += [bce.item(), total.item()]
    m = mf.compute_metrics(q, y, 0.5)
    logged += [m["maF1"].item(), m["miF1"].item()]
    return logged


def one_shape(sh, steps):
    a, model, x, opt, data = build(sh)
    tables = [mf.LabelDistanceTable(data["dist"], sh["L"], DEV)]
    cents = torch.from_numpy(data["cents"]).to(DEV)
    batch = (torch.from_numpy(data["labels"]).float().to(DEV), torch.from_numpy(data["feat"]).to(DEV),
             torch.from_numpy(data["sens"]).to(DEV))
    step = mpvae_step.CalibrationStep(model, x, opt, a, tables, cents)
    for _ in range(3):
        out = step.step(*batch)
    eager_ms, eager_n = wall_ms(lambda: step.step(*batch), steps), launches(lambda: step.step(*batch))
    step.capture(*batch)
    for _ in range(3):
        step.step(*batch)
    graph_ms, graph_n = wall_ms(lambda: step.step(*batch), steps), launches(lambda: step.step(*batch))
    finite = bool(torch.isfinite(out[0]).item())
    ab, mb, xb, ob, db = build(sh)
    base_steps = max(2, steps // 4)
    for _ in range(2):
        baseline_step(ab, mb, xb, ob, db)
    base_ms = wall_ms(lambda: baseline_step(ab, mb, xb, ob, db), base_steps)
    base_n = launches(lambda: baseline_step(ab, mb, xb, ob, db), 2)
    return {"shape": dict(sh, G=G, T=1, slices=mf.calib_slices(sh["B"], sh["L"], G, DEV)),
            "steps": steps, "calibration_step_eager_ms": eager_ms,
            "calibration_step_eager_launches": eager_n, "calibration_step_graph_ms": graph_ms,
            "calibration_step_graph_launches": graph_n, "baseline_steps": base_steps,
            "baseline_torch_loop_ms": base_ms, "baseline_torch_loop_launches": base_n,
            "baseline_over_eager": base_ms / eager_ms, "baseline_over_graph": base_ms / graph_ms,
            "updates": int(step.updates), "loss_finite": finite}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calib_bench.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shapes", default="c2,c4")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calib.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "*_ms: host wall clock per step over `steps` calls, device synchronised "
                   "before and after, after warm-up; launches: device kernels per step "
                   "(torch.profiler); baseline: the reference's loop body restated in torch ops "
                   "in the same process (grad through compute_loss and the model, host dict "
                   "lookups, torch.unique, .item() calls)",
           "shapes": [one_shape(sh, cli.steps) for sh in SHAPES
                      if sh["name"] in cli.shapes.split(",")]}
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
