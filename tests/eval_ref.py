"""numpy fp64 restatement of the scoring of fairsoft_evaluate.evaluate_mpvae
(:83-121) with evals.f1_score on raw probabilities (evals.py:61-67, :99-109)
-- TEST INFRASTRUCTURE ONLY, the checker of csrc/evalsplit.hip and of
``mpvae_fair.split_scores``.  Pinned to the reference's own records by
tests/test_eval_host.py (tests/golden/make_golden_eval.py).  It decides the
active terms on the host (``if W > 0``), as the reference does.
"""
import json
import glob
import os

import numpy as np

from oracle.fairness import row_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def weights(labels, dists):
    """(T, N) fp64: row i's distance in each target's dict, 0 when absent."""
    labels = np.asarray(labels)
    if not dists:
        return np.zeros((0, labels.shape[0]), np.float64)
    return np.stack([row_weights(labels.astype(np.int64), d) for d in dists])


def group_of(sensitive, centroids):
    """Index of each row's sensitive pattern among the centroids' rows."""
    eq = (np.asarray(sensitive)[:, None, :] == np.asarray(centroids)[None, :, :]).all(-1)
    assert eq.any(1).all(), "a row matches no centroid"
    return eq.argmax(1)


def counts(pred, target):
    """(3, L) fp64: tp, fp, fn of evals.compute_tp_fp_fn on probabilities."""
    p, y = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    return np.stack([(y * p).sum(0), ((y == 0) * p).sum(0), (y * (p == 0)).sum(0)])


def f1(c):
    """(miF1, maF1) of the counts (evals.py:99-109)."""
    tp, fp, fn = c
    with np.errstate(divide="ignore", invalid="ignore"):
        mi = 2 * tp.sum() / (2 * tp.sum() + fp.sum() + fn.sum())
        v = 2 * tp / (2 * tp + fp + fn + 1e-6)
        v = v[np.isfinite(v)]
        ma = v.mean() if v.size else np.float64("nan")
    return float(mi), float(ma)


def terms(pred, w, gid, G):
    """(T, G) fp64: the squared distance of every active (target, group) pair,
    NaN elsewhere (fairsoft_evaluate.py:106-119)."""
    p = np.asarray(pred, np.float64)
    out = np.full((len(w), G), np.nan)
    for t, wt in enumerate(w):
        if not wt.sum() > 0:
            continue
        mean_all = (wt[:, None] * p).sum(0) / wt.sum()
        for k in range(G):
            sel = gid == k
            if wt[sel].sum() > 0:
                mean_k = (wt[sel, None] * p[sel]).sum(0) / wt[sel].sum()
                out[t, k] = ((mean_k - mean_all) ** 2).sum()
    return out


def means(tm):
    """(mean of sqrt(terms), mean of terms, number of active terms); the means
    NaN when no term is active (``np.mean([])``)."""
    act = tm[~np.isnan(tm)]
    if not act.size:
        return float("nan"), float("nan"), 0
    return float(np.sqrt(act).mean()), float(act.mean()), int(act.size)


def scores(pred, target, w=None, gid=None, G=1, perm=None):
    """Everything mpv_split_eval returns, as a dict; ``perm`` (a permutation of
    the rows) changes the order of every sum and nothing else."""
    pred, target = np.asarray(pred), np.asarray(target)
    if perm is not None:
        pred, target = pred[perm], target[perm]
        w = None if w is None else w[:, perm]
        gid = None if gid is None else gid[perm]
    c = counts(pred, target)
    mi, ma = f1(c)
    out = dict(counts=c, miF1=mi, maF1=ma)
    if w is not None:
        tm = terms(pred, w, gid, G)
        d, s, n = means(tm)
        out.update(terms=tm, fair_mean_diff=d, fair_mean_sq=s, nterms=n)
    return out


def order_sensitivity(pred, target, w=None, gid=None, G=1, seeds=(0, 1, 2)):
    """s of the tolerance rule: the restatement on the rows in fixed
    permutations against itself, per output, in the metric of the check
    (``err``; the largest over the permutations) -- no code under test
    involved.  ``fair``: the largest of the three fairness outputs' (the two
    means are sums of the terms: one permutation can leave a scalar unmoved by
    chance where it moves the terms)."""
    a = scores(pred, target, w, gid, G)
    out = {k: 0.0 for k in a if k != "nterms"}
    for seed in seeds:
        perm = np.random.default_rng(seed).permutation(len(pred))
        b = scores(pred, target, w, gid, G, perm)
        for k in out:
            out[k] = max(out[k], err(b[k], a[k]))
    if w is not None:
        out["fair"] = max(out["terms"], out["fair_mean_diff"], out["fair_mean_sq"])
    return out


def err(got, ref):
    """max |got - ref| / max |ref| over the positions that are not NaN in ref;
    inf when the NaN positions differ; the absolute error when ref is all 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    m = ~np.isnan(ref)
    if not m.any():
        return 0.0
    scale = np.abs(ref[m]).max()
    e = np.abs(got[m] - ref[m]).max()
    return float(e if scale == 0 else e / scale)


def tol(s):
    """The rule of tolerances.fair_row_grad_tol for fp64 results: one fp64
    rounding plus four times the restatement's own order sensitivity."""
    return 2.0 ** -52 + 4.0 * s


def f1_tol(s_counts, L):
    """miF1 / maF1 from counts that are right to ``tol(s_counts)``: a ratio of
    non-negative sums carries at most twice the counts' relative error, the
    ratio itself four roundings (2 tp, the three additions, the division) and
    the sum over the L labels, in any order, at most L more of 2^-53 each."""
    return 2.0 * tol(s_counts) + (L + 8) * 2.0 ** -53


def eval_fixtures():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "eval_*.npz"))):
        z = np.load(path)
        d = {k: z[k] for k in z.files}
        d["name"] = os.path.basename(path)[5:-4]
        d["dists"] = [{k: np.float64(v) for k, v in t.items()} for t in json.loads(str(d["dists"]))]
        for k in ("labels", "weight_labels", "sensitive", "centroids"):
            d[k] = d[k].astype(np.int64)
        out.append(d)
    return out
