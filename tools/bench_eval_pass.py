"""Time one evaluation pass over a split (mpvae_step.EvalPass, mpv_split_eval in
csrc/evalsplit.hip) against the loop it replaces:

    python tools/bench_eval_pass.py [--out profiles/eval_pass_bench.json] [--passes 2]

Shapes, both at n_test_sample = 10000 with Philox noise from a device key,
T = 3 target tables, G = 4 sensitive groups:

  s1  N 20000, B 128, F 100, L 25, z 10, d 8
  s2  N 10000, B 128, F 1000, L = z = 38, d 50

Per shape, in one process on one device, three variants alternate over
``--rounds`` rounds of ``--passes`` passes each:

  a  the loop a user writes without EvalPass (fairsoft_evaluate.py:55-121): per
     batch ``model(label, feat)``, ``predict_proba``, ``.cpu()``; then the
     scoring in numpy as the reference does it -- the soft F1 of evals.py and
     the fairness loop with a dict lookup per row and a Python loop over
     targets x groups;
  b  EvalPass eager, ``read`` included (its one host sync);
  c  EvalPass with the full-batch body captured in a HIP graph, ``read`` included.

Recorded: wall ms per pass (host clock, device synchronised before and after)
of every round, their median and range; and, through mpv_timing, the device
time of split_eval + split_final against calib_fwd + calib_tables
(``mf.fair_mean_diff``, which delivers the mean squared distance alone) on the
same (N, L, T, G), each with its default slices.  Needs a GPU; there is no
fallback."""
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
SHAPES = [dict(name="s1", N=20000, B=128, F=100, L=25, z=10, d=8),
          dict(name="s2", N=10000, B=128, F=1000, L=38, z=38, d=50)]
T, G, S = 3, 4, 10000


def build(sh, seed=0):
    """One model and one split; the same for every variant."""
    L, N = sh["L"], sh["N"]
    a = argparse.Namespace(feature_dim=sh["F"], latent_dim=sh["d"], label_dim=L, z_dim=sh["z"],
                           keep_prob=0.5, scale_coeff=1.0, residue_sigma="", n_train_sample=10,
                           n_test_sample=S, mode="test", nll_coeff=0.5, c_coeff=10.0,
                           mpvae_noise="philox",
                           mpvae_seed=torch.tensor([seed + 1], dtype=torch.int64, device=DEV))
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = mpvae.VAE(a).to(DEV).eval()
    rng = np.random.default_rng(seed)
    pool = (rng.random((500, L)) < 0.15).astype(np.int64)  # 500 label patterns, repeated
    labels = pool[rng.integers(0, 500, N)]
    cents = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int64)
    sens = cents[rng.integers(0, G, N)]
    dists = {f"t{t}": {"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1))
                       for r in pool[t::T + 1]} for t in range(T)}
    feat = rng.standard_normal((N, sh["F"])).astype(np.float32)
    return dict(args=a, model=model, labels=labels, sens=sens, cents=cents, dists=dists, feat=feat,
                tables=[mf.LabelDistanceTable(d, L, DEV) for d in dists.values()],
                y=torch.from_numpy(labels).float().to(DEV), x=torch.from_numpy(feat).to(DEV),
                s=torch.from_numpy(sens).to(DEV), c=torch.from_numpy(cents).to(DEV))


def numpy_scoring(prob, labels, sens, dists):
    """fairsoft_evaluate.py:83-121 restated, with evals.f1_score's forms."""
    y = labels.astype(np.float32)
    tp = np.sum(y * prob, axis=0).astype("float32")
    fp = np.sum(np.logical_not(y) * prob, axis=0).astype("float32")
    fn = np.sum(y * np.logical_not(prob), axis=0).astype("float32")
    mi = 2 * np.sum(tp) / float(2 * np.sum(tp) + np.sum(fp) + np.sum(fn))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.true_divide(2 * tp, 2 * tp + fp + fn + 1e-6)
    ma = np.mean(c[np.isfinite(c)])
    centroid = np.unique(sens, axis=0)
    diffs = []
    for dist in dists.values():
        weights = np.array([dist.get("".join(label.astype(int).astype(str)), 0.)
                            for label in labels]).reshape(-1, 1)
        if weights.sum() > 0:
            mean_all = np.sum(prob * weights, axis=0) / weights.sum()
            for sensitive in centroid:
                sel = np.all(np.equal(sens, sensitive), axis=1)
                if weights[sel].sum() > 0:
                    mean_k = np.sum(prob[sel] * weights[sel], 0) / weights[sel].sum()
                    diffs.append(np.sqrt(np.sum(np.power(mean_k - mean_all, 2))))
    return {"fair_mean_diff": float(np.mean(diffs)), "miF1": float(mi), "maF1": float(ma)}


def hand_pass(d, B):
    """The user's loop without EvalPass: device work per batch, a copy to the
    host per batch, numpy after."""
    model, a, N = d["model"], d["args"], len(d["labels"])
    a.mpvae_seed_advance = True
    probs = []
    with torch.no_grad():
        for i in range(N // B + 1):
            s, e = i * B, min((i + 1) * B, N)
            if e <= s:
                continue
            label = torch.from_numpy(d["labels"][s:e]).float().to(DEV)
            feat = torch.from_numpy(d["feat"][s:e]).to(DEV)
            out = model(label, feat)
            p = mpvae.predict_proba(out[3], model.r_sqrt_sigma, a)
            probs.append(p.cpu().data.numpy())
    return numpy_scoring(np.concatenate(probs), d["labels"], d["sens"], d["dists"])


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def kernel_ms(fn, names, reps=20):
    """Mean device ms per call of the named kernels (mpv_timing)."""
    lib = H.load_library()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    lib.mpv_timing_enable(1)
    lib.mpv_timing_reset()
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        times = H.kernel_times()
    finally:
        lib.mpv_timing_enable(0)
    return {k: times[k][1] / reps for k in names}


def one_shape(sh, passes, rounds):
    d = build(sh)
    B = sh["B"]

    def make(captured):
        a = argparse.Namespace(**vars(d["args"]))
        a.mpvae_seed = torch.tensor([1], dtype=torch.int64, device=DEV)
        ev = ms.EvalPass(d["model"], a, B, tables=d["tables"], centroids=d["c"])
        if captured:
            ev.capture(d["y"], d["x"])
        return lambda: ev.read(ev.run(d["y"], d["x"], d["s"]))

    variants = {"a_hand_loop": lambda: hand_pass(d, B), "b_eval_pass_eager": make(False),
                "c_eval_pass_graph": make(True)}
    last = {k: fn() for k, fn in variants.items()}  # warm every variant
    ms_rounds = {k: [] for k in variants}
    for _ in range(rounds):  # alternate, so that drift of the box hits all alike
        for k, fn in variants.items():
            ms_rounds[k].append(wall_ms(fn, passes))
    res = {"shape": dict(sh, T=T, G=G, n_test_sample=S), "passes": passes, "rounds": rounds,
           "results_of_the_warm_up_pass": last}
    for k, v in ms_rounds.items():
        res[k] = {"ms_rounds": v, "ms_median": statistics.median(v), "ms_min": min(v),
                  "ms_max": max(v)}
    a, c = res["a_hand_loop"], res["c_eval_pass_graph"]
    res["a_over_b"] = a["ms_median"] / res["b_eval_pass_eager"]["ms_median"]
    res["a_over_c"] = a["ms_median"] / c["ms_median"]
    res["captured_not_slower_than_hand_loop"] = c["ms_median"] <= a["ms_median"]
    # the kernels alone, on one buffer of probabilities
    p = torch.rand(sh["N"], sh["L"], device=DEV)
    new = kernel_ms(lambda: mf.split_scores(p, d["y"], d["s"], d["c"], d["tables"]),
                    ("split_eval", "split_final"))
    old = kernel_ms(lambda: mf.fair_mean_diff(p, d["y"], d["s"], d["c"], d["tables"]),
                    ("calib_fwd", "calib_tables"))
    res["kernels_ms"] = dict(new, **old, split_pair=sum(new.values()), calib_pair=sum(old.values()),
                             split_slices=mf.eval_slices(sh["N"], sh["L"], G, DEV),
                             calib_slices=mf.calib_slices(sh["N"], sh["L"], G, DEV))
    res["split_pair_not_slower_than_calib_pair"] = sum(new.values()) <= sum(old.values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_pass_bench.json"))
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="s1,s2")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_pass.py needs a GPU")
    if cli.rounds < 5:
        raise SystemExit("at least five rounds: the spread is part of the result")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "ms: host wall clock per pass over the whole split (`passes` passes per figure, "
                   "device synchronised before and after, after a warm-up pass), one figure per "
                   "round, the variants alternating; a: the per-batch loop with .cpu() and the "
                   "numpy scoring of fairsoft_evaluate.py; b / c: EvalPass eager / with the "
                   "full-batch body in a HIP graph, read() included; kernels_ms: mean device ms "
                   "per call (mpv_timing) of split_eval + split_final against calib_fwd + "
                   "calib_tables on the same (N, L, T, G), default slices each",
           "shapes": [one_shape(sh, cli.passes, cli.rounds) for sh in SHAPES
                      if sh["name"] in cli.shapes.split(",")]}
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
