"""Time the label-similarity weights (mpvae_fair.LabelSimilarity, row_weights_kernel<LabelSims>
in csrc/fairness.hip) and the many-definition evaluation (EvalPass(definitions=),
mpv_split_eval_defs in csrc/evalsplit.hip) against what they replace:

    python tools/bench_label_sim.py [--out profiles/label_sim_bench.json]

One run on one device, ``--rounds`` (at least five) rounds in which the
variants alternate; every figure is the time between two device events round
the calls (the stream drained before the first), one figure per round, and
their median and range.

  sweep    the distance sweep of fairsoft_metric.evaluate_models_over_label_
           distances (nine gammas, indication, constant; T = 3 targets, G = 4
           groups, n_test_sample = 10000, Philox noise from a device key):
             a  eleven table-based EvalPass runs, one per definition (what a
                user of EvalPass does without ``definitions``), read included;
             b  one EvalPass(definitions=...) run, read included;
             c  one table-based EvalPass run, for scale (b against 2 c);
           at s1 (N 20000, F 100, L 25, z 10) and s2 (N 10000, F 1000, L = z = 38).
  weights  mf.similarity_weights against mf.label_weights_batch (tables over the
           split's distinct patterns) at T = 3, for a batch (B 128) and a whole
           split (N 20000), L 25; device events round ``--reps`` calls, and
           through mpv_timing the kernels alone.
  host     constructing 3 LabelSimilarity objects against 3 LabelDistanceTables
           from dicts over the split's distinct patterns (host wall clock; the
           table side does not include building the dict, which in the reference
           is a P x P loop of Python string compares).

Needs a GPU; there is no fallback."""
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
SWEEP = [("jaccard", g) for g in (0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0)] + \
    [("indication", None), ("constant", None)]


def key_of(row):
    return "".join(str(int(v)) for v in row)


def weight_of(kind, gamma, target, rows):
    """The closed forms in numpy (what the reference's builders store)."""
    rows, tgt = rows.astype(bool), target.astype(bool)
    n_and, n_or = (rows & tgt).sum(1), (rows | tgt).sum(1)
    same = (rows ^ tgt).sum(1) == 0
    sim = {"indication": same.astype(np.float64), "constant": np.ones(len(rows)),
           "jaccard": np.where(same, 1.0, n_and / np.maximum(n_or, 1)),
           "hamming": (rows == tgt).sum(1) / rows.shape[1]}[kind]
    return sim if gamma is None else np.clip(np.exp(gamma * (sim - 1)), 0.0, 1.0)


def build(sh, seed=0):
    L, N = sh["L"], sh["N"]
    a = argparse.Namespace(feature_dim=sh["F"], latent_dim=sh["d"], label_dim=L, z_dim=sh["z"],
                           keep_prob=0.5, scale_coeff=1.0, residue_sigma="", n_train_sample=10,
                           n_test_sample=S, mode="test", nll_coeff=0.5, c_coeff=10.0,
                           mpvae_noise="philox")
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = mpvae.VAE(a).to(DEV).eval()
    rng = np.random.default_rng(seed)
    pool = np.unique((rng.random((500, L)) < 0.15).astype(np.int64), axis=0)
    labels = pool[rng.integers(0, len(pool), N)]
    cents = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int64)
    sens = cents[rng.integers(0, G, N)]
    feat = rng.standard_normal((N, sh["F"])).astype(np.float32)
    targets = pool[:T]
    keys = [key_of(r) for r in pool]
    conv = lambda g: float if g is None else np.float64
    dicts = [[{k: conv(g)(v) for k, v in zip(keys, weight_of(kind, g, targets[t], pool))}
              for t in range(T)] for kind, g in SWEEP]
    return dict(args=a, model=model, pool=pool, targets=targets, dicts=dicts,
                y=torch.from_numpy(labels).float().to(DEV), x=torch.from_numpy(feat).to(DEV),
                s=torch.from_numpy(sens).to(DEV), c=torch.from_numpy(cents).to(DEV))


def event_ms(fn, n=1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def summary(v):
    return {"ms_rounds": v, "ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def kernel_ms(fn, names, reps):
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
    return {k: times[k][1] / reps for k in names if k in times}


def sweep_shape(sh, rounds):
    d = build(sh)
    L, B = sh["L"], sh["B"]
    tables = [[mf.LabelDistanceTable(dd, L, DEV) for dd in per] for per in d["dicts"]]
    defs = [[mf.LabelSimilarity(k, d["targets"][t], L, DEV, gamma=g) for t in range(T)]
            for k, g in SWEEP]

    def passes(**kw):
        a = argparse.Namespace(**vars(d["args"]))
        a.mpvae_seed = torch.tensor([1], dtype=torch.int64, device=DEV)
        ev = ms.EvalPass(d["model"], a, B, centroids=d["c"], **kw)
        return lambda: ev.read(ev.run(d["y"], d["x"], d["s"]))

    per_def = [passes(tables=t) for t in tables]
    variants = {"a_eleven_table_passes": lambda: [fn() for fn in per_def],
                "b_one_pass_eleven_definitions": passes(definitions=defs),
                "c_one_table_pass": per_def[0]}
    last = {k: fn() for k, fn in variants.items()}  # warm every variant
    ms_rounds = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms_rounds[k].append(event_ms(fn))
    res = {"shape": dict(sh, T=T, G=G, D=len(SWEEP), n_test_sample=S), "rounds": rounds,
           "fair_mean_diff_of_the_warm_up": {
               "a": [r["fair_mean_diff"] for r in last["a_eleven_table_passes"]],
               "b": last["b_one_pass_eleven_definitions"]["fair_mean_diff"]}}
    res.update({k: summary(v) for k, v in ms_rounds.items()})
    a, b, c = (res[k]["ms_median"] for k in variants)
    res["a_over_b"] = a / b
    res["b_over_c"] = b / c
    res["b_cheaper_than_two_single_passes"] = b < 2 * c
    p = torch.rand(sh["N"], L, device=DEV)
    res["scoring_kernels_ms"] = {
        "eleven_definitions": kernel_ms(
            lambda: mf.split_scores_defs(p, d["y"], d["s"], d["c"], defs),
            ("label_sim", "split_eval", "split_final"), 10),
        "one_definition_tables": kernel_ms(
            lambda: mf.split_scores(p, d["y"], d["s"], d["c"], tables[0]),
            ("label_weights", "split_eval", "split_final"), 10)}
    return res, d


def weights_bench(d, sh, rounds, reps):
    L = sh["L"]
    sims = [mf.LabelSimilarity("jaccard", d["targets"][t], L, DEV, gamma=1.0) for t in range(T)]
    tables = [mf.LabelDistanceTable(dd, L, DEV) for dd in d["dicts"][3]]   # the same weights
    out = {}
    for name, y in (("B128", d["y"][:128].contiguous()), (f"N{sh['N']}", d["y"])):
        variants = {"label_sim": lambda y=y: mf.similarity_weights(y, sims),
                    "label_weights_batch": lambda y=y: mf.label_weights_batch(y, tables)}
        ws = {k: fn()[0] for k, fn in variants.items()}
        ulps = (ws["label_sim"].view(torch.int64) - ws["label_weights_batch"].view(torch.int64))
        ms_rounds = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                ms_rounds[k].append(event_ms(fn, reps))
        r = {k: summary(v) for k, v in ms_rounds.items()}
        r["max_ulp_between_the_two"] = int(ulps.abs().max())
        r["kernel_ms"] = dict(kernel_ms(variants["label_sim"], ("label_sim",), reps),
                              **kernel_ms(variants["label_weights_batch"], ("label_weights",), reps))
        r["call_sim_over_tables"] = r["label_sim"]["ms_median"] / \
            r["label_weights_batch"]["ms_median"]
        out[name] = r
    return out


def host_bench(d, sh, rounds):
    L = sh["L"]
    dicts = d["dicts"][3]
    variants = {"three_similarities": lambda: [mf.LabelSimilarity("jaccard", d["targets"][t], L, DEV,
                                                                  gamma=1.0) for t in range(T)],
                "three_tables": lambda: [mf.LabelDistanceTable(dd, L, DEV) for dd in dicts]}
    ms_rounds = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms_rounds[k].append((time.perf_counter() - t0) * 1e3)
    r = {k: summary(v) for k, v in ms_rounds.items()}
    r["patterns_in_a_dict"] = len(dicts[0])
    r["tables_over_similarities"] = r["three_tables"]["ms_median"] / \
        r["three_similarities"]["ms_median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_sim_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--shapes", default="s1,s2")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_sim.py needs a GPU")
    if cli.rounds < 5:
        raise SystemExit("at least five rounds: the spread is part of the result")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "ms between two device events round the calls, one figure per round, the "
                   "variants alternating; sweep: eleven table-based EvalPass runs (a) against one "
                   "EvalPass(definitions=) run (b) and one table-based run (c), read() included; "
                   "weights: per call over `reps` calls, kernel_ms through mpv_timing; host: wall "
                   "clock of constructing the three weight sources",
           "sweep": [], "rounds": cli.rounds, "reps": cli.reps}
    for sh in SHAPES:
        if sh["name"] not in cli.shapes.split(","):
            continue
        r, d = sweep_shape(sh, cli.rounds)
        res["sweep"].append(r)
        if sh["name"] == "s1":
            res["weights"] = weights_bench(d, sh, cli.rounds, cli.reps)
            res["host"] = host_bench(d, sh, cli.rounds)
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
