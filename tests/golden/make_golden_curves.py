"""Golden vectors for the validation metrics (AUC / AUPR / FDR and the
threshold sweep).

Runs ONLY in the build container, where the reference is mounted at
/root/reference (it never travels to the GPU box).  The outputs come from the
reference's own evals.compute_metrics(..., all_metrics=True) (evals.py:129-238,
scikit-learn underneath), imported by file path; the sweep fixtures also hold
the 14 best values of the selection loop of validate_mpvae
(fairsoft_train.py:400-416), restated here over the reference's outputs.

The reference drops a label whose metric is undefined from its ``all*``
arrays; the fixtures keep length L with NaN in that place (one-class labels:
roc_auc_score raises or returns NaN depending on the scikit-learn version; both
mean "undefined").

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_curves.py [NAME ...]
Writes: tests/golden/curves_*.npz, or only the named records (the inputs of
every record are drawn either way, so a record's bytes do not depend on which
others are written).
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
from curves_ref import METRICS, THRESHOLDS  # noqa: E402

KEYS8 = ["ACC", "HA", "ebF1", "miF1", "maF1", "p_at_1", "p_at_3", "p_at_5"]


def load_evals():
    spec = importlib.util.spec_from_file_location("_ref_evals", os.path.join(REF, "evals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def per_label(ev, pred, target):
    """The reference's three per-label values, one column at a time, so that a
    label the reference drops keeps its place as NaN."""
    L = pred.shape[1]
    out = np.full((3, L), np.nan)
    for l in range(L):
        p, t = pred[:, l:l + 1].copy(), target[:, l:l + 1].copy()
        for j, fn in enumerate([ev.compute_auc, ev.compute_aupr, ev.compute_fdr]):
            arr = np.asarray(fn(t, p)[3], np.float64)
            if arr.size == 1 and not np.isnan(arr[0]):
                out[j, l] = arr[0]
    return out


ONLY = set(sys.argv[1:])


def record(ev, name, pred, target, sweep=False):
    if ONLY and name not in ONLY:
        return
    pred, target = pred.astype(np.float32), target.astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        allv = per_label(ev, pred, target)
        rec = dict(pred=pred, target=target, allAUC=allv[0], allAUPR=allv[1], allFDR=allv[2])
        m = ev.compute_metrics(pred.copy(), target.copy(), 0.5, all_metrics=True)
        rec["values8"] = np.array([float(m[k]) for k in KEYS8], np.float64)
        # the reference's own arrays are the kept (non-NaN) entries, in order
        for j, k in enumerate(["allAUC", "allAUPR", "allFDR"]):
            kept = allv[j][~np.isnan(allv[j])]
            ref = np.asarray(m[k], np.float64)
            ref = ref[~np.isnan(ref)]
            assert kept.shape == ref.shape and np.array_equal(kept, ref), (name, k)
        if sweep:
            best = None
            for thr in THRESHOLDS:
                v = ev.compute_metrics(pred.copy(), target.copy(), thr, all_metrics=True)
                assert not any(np.isnan(float(v[k])) for k in METRICS), (name, thr)
                # no row with both sums zero at any threshold (example-F1 would drop it)
                hard = (pred >= np.float32(thr)).sum(1) + target.sum(1)
                assert (hard > 0).all(), (name, thr)
                if best is None:
                    best = {k: float(v[k]) for k in METRICS}
                else:
                    for k in METRICS:
                        best[k] = (min if "FDR" in k else max)(best[k], float(v[k]))
            rec["best"] = np.array([best[k] for k in METRICS], np.float64)
    path = os.path.join(HERE, f"curves_{name}.npz")
    np.savez_compressed(path, **rec)
    print(name, pred.shape, "nan labels", int(np.isnan(allv[0]).sum()),
          "meanAUC", float(np.nanmean(allv[0])) if not np.isnan(allv[0]).all() else None,
          os.path.getsize(path), "bytes")


def quantise(x, levels):
    return (np.floor(x * levels) / levels).astype(np.float32)


def main():
    ev = load_evals()
    rng = np.random.default_rng(4101)
    # c1: continuous scores
    t = (rng.random((64, 5)) < 0.35).astype(np.float32)
    record(ev, "c1", rng.random((64, 5)), t)
    # c2: 8 score levels; all-0, all-1, single-positive labels; a constant-score column
    t = (rng.random((200, 6)) < 0.3).astype(np.float32)
    p = quantise(rng.random((200, 6)) * 0.6 + 0.4 * t * rng.random((200, 6)), 8)
    t[:, 1] = 0
    t[:, 2] = 1
    t[:, 3] = 0
    t[137, 3] = 1
    p[:, 4] = 0.375
    record(ev, "c2", p, t)
    # c3: 70 labels, 16 levels
    t = (rng.random((300, 70)) < 0.2).astype(np.float32)
    record(ev, "c3", quantise(rng.random((300, 70)) * 0.7 + 0.3 * t * rng.random((300, 70)), 16), t)
    # c4, c5: one and two rows
    record(ev, "c4", np.array([[0.3, 0.7, 0.5]]), np.array([[1.0, 0.0, 1.0]]))
    record(ev, "c5", np.array([[0.3, 0.7, 0.5], [0.6, 0.7, 0.25]]),
           np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]))
    # sweep fixtures: every label has both classes, every row has a positive label
    for name, N, L in [("s1", 128, 6), ("s2", 256, 40)]:
        t = (rng.random((N, L)) < 0.3).astype(np.float32)
        t[np.arange(N), rng.integers(0, L, N)] = 1
        t[0, :], t[1, :] = 1, 0
        t[1, 0] = 1
        p = (0.02 + 0.96 * rng.random((N, L)) * (0.5 + 0.5 * t)).astype(np.float32)
        record(ev, name, p, t, sweep=True)
    # The records below draw from a generator of their own.  They cross one
    # merge and one pass tile of csrc/curves.hip (1024 keys) with scores the
    # records above do not hold.
    rng = np.random.default_rng(4102)
    fmax, tiny = np.finfo(np.float32).max, np.float32(2.0 ** -149)
    # c6: signed scores with +-0, denormals and +-FLT_MAX; a constant column;
    # two long runs; all-distinct negative scores
    N = 1100
    t = (rng.random((N, 4)) < 0.3).astype(np.float32)
    p = np.empty((N, 4), np.float32)
    p[:, 0] = ((rng.random(N) - 0.5) * (1 + t[:, 0] * rng.random(N))).astype(np.float32)
    edge = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, -3 * tiny, np.finfo(np.float32).tiny,
                     fmax, -fmax], np.float32)
    rows = rng.permutation(N)[:4 * edge.size]
    p[rows, 0] = np.tile(edge, 4)
    p[:, 1] = -0.625
    p[:, 2] = np.where(rng.permutation(N) < 500, 0.25, -0.25)
    p[:, 3] = (-0.01 - rng.random(N) - 0.5 * (1 - t[:, 3]) * rng.random(N)).astype(np.float32)
    assert np.unique(p[:, 3]).size == N and (p[:, 3] < 0).all()
    assert (np.signbit(p[:, 0]) & (t[:, 0] == 1)).any() and (p[:, 0] > 0).any()
    record(ev, "c6", p, t)
    # c7: all-distinct signed scores
    N = 1030
    t = (rng.random((N, 2)) < 0.3).astype(np.float32)
    p = ((rng.random((N, 2)) - 0.5) + 0.4 * t * rng.random((N, 2))).astype(np.float32)
    assert all(np.unique(p[:, l]).size == N for l in range(2))
    record(ev, "c7", p, t)


if __name__ == "__main__":
    main()
