"""Golden vectors for the evaluation's scoring of a split.

Runs ONLY in the build container, where the reference is mounted at
/root/reference (it never travels to the GPU box).  The results come from the
reference's own code: the scoring block of fairsoft_evaluate.evaluate_mpvae
(from ``train_indiv_prob = np.concatenate(train_indiv_prob)`` through
``mean_diffs = np.mean(mean_diffs)``), executed from the file's source text in
a namespace that provides the loop's variables, with the reference's evals.py
imported by file path (numpy + scikit-learn, both present).  The module itself
cannot be imported here (fairsoft_evaluate -> joblib / data / fairsoft_trial),
and the block is inline in the evaluation function.

The reference looks the row weights up in ``data.labels[np.arange(len(
subset_idx))]``, the dataset's first N rows; the cases hand it a ``data.labels``
whose first N rows are ``weight_labels`` (equal to the split's labels except in
``e4_first_rows``, where the split is the dataset's second half).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py
Writes: tests/golden/eval_*.npz
"""
import importlib.util
import json
import os
import textwrap
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def load_evals():
    spec = importlib.util.spec_from_file_location("_ref_evals", os.path.join(REF, "evals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scoring_block():
    """The reference's scoring block (fairsoft_evaluate.py), dedented."""
    lines = open(os.path.join(REF, "fairsoft_evaluate.py")).read().split("\n")
    start = next(i for i, l in enumerate(lines)
                 if l.strip() == "train_indiv_prob = np.concatenate(train_indiv_prob)")
    end = next(i for i in range(start, len(lines))
               if lines[i].strip() == "mean_diffs = np.mean(mean_diffs)")
    return textwrap.dedent("\n".join(lines[start:end + 1])), (start + 1, end + 1)


class _Data:
    pass


def key(row):
    return "".join(np.asarray(row).astype(int).astype(str))


def run_case(block, evals, pred, data_labels, data_sens, subset_idx, dists, targets, batch=128):
    data = _Data()
    data.labels, data.sensitive_feat = data_labels, data_sens
    labels = data_labels[subset_idx].astype(np.float32)  # input_label.float() ... .numpy()
    cuts = list(range(0, len(subset_idx), batch))
    ns = dict(np=np, evals=evals, eval_fairness=True, data=data, subset_idx=subset_idx,
              train_indiv_prob=[pred[c:c + batch] for c in cuts],
              train_label=[labels[c:c + batch] for c in cuts],
              train_feat_z=[pred[c:c + batch] for c in cuts],
              train_sensitive=data_sens[subset_idx],
              target_fair_labels=targets, label_distances=dists)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # np.mean([]) of a case with no active term
        exec(block, ns)
    N = len(subset_idx)
    return dict(pred=pred, labels=data_labels[subset_idx].astype(np.int8),
                weight_labels=data_labels[:N].astype(np.int8),
                sensitive=data_sens[subset_idx].astype(np.int8),
                centroids=np.unique(data_sens, axis=0).astype(np.int8),
                dists=np.array(json.dumps([{k: float(v) for k, v in dists[t].items()}
                                           for t in targets])),
                fair_mean_diff=np.array(float(ns["mean_diffs"])),
                miF1=np.array(float(ns["miF1"])), maF1=np.array(float(ns["maF1"])))


def make_dists(rng, rows, L, T, keep=0.7):
    """T target dicts over the label patterns of ``rows`` (np.float64 values, as
    label_distance.py's np.clip(np.exp(...)) produces) plus a few absent ones."""
    keys = sorted({key(r) for r in rows}) + [key(rng.integers(0, 2, L)) for _ in range(4)]
    dists, targets = {}, []
    for _ in range(T):
        tk = key(rng.integers(0, 2, L))
        dists[tk] = {k: np.float64(rng.uniform(0.05, 1.0)) for k in keys if rng.random() < keep}
        targets.append(tk)
    return dists, targets


def main():
    block, (a, b) = scoring_block()
    print(f"scoring block: fairsoft_evaluate.py:{a}-{b}")
    evals = load_evals()
    # name, N, L, T, number of sensitive patterns, seed
    for name, N, L, T, G, seed in [("e1_l25", 300, 25, 2, 3, 1),
                                   ("e2_dead_zero_fn", 200, 20, 3, 3, 2),
                                   ("e3_inactive", 64, 12, 2, 2, 3),
                                   ("e4_first_rows", 150, 25, 2, 3, 4),
                                   ("e5_l257", 40, 257, 9, 2, 5)]:
        rng = np.random.default_rng(300 + seed)
        n_data = 2 * N if name == "e4_first_rows" else N
        labels = (rng.random((n_data, L)) < 0.3).astype(np.int64)
        labels[n_data // 2:, :] = labels[:n_data - n_data // 2, :]  # repeated patterns
        if name == "e4_first_rows":
            labels[N:] = (rng.random((N, L)) < 0.3).astype(np.int64)  # the split: other rows
        sens = np.stack([rng.integers(0, G, n_data), np.ones(n_data, np.int64)], 1)
        sens[:G, 0] = np.arange(G)  # every pattern present
        subset_idx = np.arange(N, 2 * N) if name == "e4_first_rows" else np.arange(N)
        pred = rng.random((N, L)).astype(np.float32)
        if name == "e2_dead_zero_fn":
            labels[:, 0] = sens[:, 0] == 0  # group 0's patterns occur in no other group
        wl = labels[:N]  # the rows the reference looks the weights up by
        if name == "e2_dead_zero_fn":
            # group 0's rows are absent from every dict (W_tk = 0), the second
            # target's dict misses every row (W_t = 0), and some probabilities
            # under a positive label are exactly zero, one of them -0.0 (fn > 0)
            dists, targets = make_dists(rng, wl[sens[:N, 0] != 0], L, T)
            dists[targets[1]] = {key(rng.integers(0, 2, L)) + "x": np.float64(0.5)}
            pos = np.argwhere(labels[subset_idx] == 1)
            pos = pos[rng.choice(len(pos), 25, replace=False)]
            pred[pos[:, 0], pos[:, 1]] = 0.0
            pred[pos[0, 0], pos[0, 1]] = -0.0
        else:
            dists, targets = make_dists(rng, wl, L, T)
        if name == "e3_inactive":
            dists = {t: {key(rng.integers(0, 2, L)) + "x": np.float64(0.5)} for t in targets}
        rec = run_case(block, evals, pred, labels, sens, subset_idx, dists, targets)
        np.savez_compressed(os.path.join(HERE, f"eval_{name}.npz"), **rec)
        print(name, "fair_mean_diff", float(rec["fair_mean_diff"]), "miF1", float(rec["miF1"]),
              "maF1", float(rec["maF1"]))


if __name__ == "__main__":
    main()
