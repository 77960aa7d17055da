"""numpy restatement of the validation metrics of evals.compute_metrics(...,
all_metrics=True) (evals.py:129-175): per-label AUC, AUPR and recall at
FDR <= 0.5, from one descending sort per label, and their aggregates.  These
are the formulas csrc/curves.hip implements; tests/test_curves_ref.py pins
them to vectors recorded from the reference's own code (scikit-learn).

Per label, with the rows sorted by descending score, T[i] the inclusive count
of positives, P = T[N-1], Nn = N - P: position i ends a threshold run when the
next score differs (or i = N-1).  At a run end tp = T[i], fp = i+1-T[i]; the
previous run end gives tp0, fp0 (0, 0 before the first run).

  AUC  = sum (fp-fp0)/Nn * (tp+tp0)/P / 2          NaN when P = 0 or Nn = 0
  AUPR = sum (rec-rec0) * (prec+prec0) / 2          prec = tp/(tp+fp),
         rec = tp/P (1 when P = 0); before the first run (rec0, prec0) = (0, 1)
  FDR  = rec at the largest run end i with 2 tp >= i+1, 0 when there is none
"""
import numpy as np

THRESHOLDS = [0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.10, 0.15, 0.20, 0.25, 0.30,
              0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65, 0.70, 0.75, 0.80, 0.85, 0.90, 0.95]
METRICS = ["ACC", "HA", "ebF1", "miF1", "maF1", "meanAUC", "medianAUC", "meanAUPR", "medianAUPR",
           "meanFDR", "medianFDR", "p_at_1", "p_at_3", "p_at_5"]


def label_curves(score, target):
    """(auc, aupr, fdr) of one label column; score fp32 (N,), target 0/1 (N,)."""
    score = np.asarray(score, np.float32) + np.float32(0.0)  # -0.0 -> +0.0
    y = (np.asarray(target) == 1).astype(np.int64)
    N = score.shape[0]
    order = np.argsort(-score.astype(np.float64), kind="stable")
    s, y = score[order], y[order]
    T = np.cumsum(y)
    P = int(T[-1])
    Nn = N - P
    ends = np.flatnonzero(np.r_[s[1:] != s[:-1], True])
    tp = T[ends].astype(np.float64)
    fp = (ends + 1 - T[ends]).astype(np.float64)
    tp0, fp0 = np.r_[0.0, tp[:-1]], np.r_[0.0, fp[:-1]]
    if P == 0 or Nn == 0:
        auc = np.nan
    else:
        auc = float(np.sum((fp - fp0) / Nn * ((tp + tp0) / P) / 2))
    prec = tp / (tp + fp)
    rec = tp / P if P > 0 else np.ones_like(tp)
    prec0, rec0 = np.r_[1.0, prec[:-1]], np.r_[0.0, rec[:-1]]
    aupr = float(np.sum((rec - rec0) * (prec + prec0) / 2))
    # the reference tests 1 - precision <= 0.5 in fp64; 2 tp >= tp + fp is the
    # same predicate (tp / (tp + fp) >= 0.5 is exact at the boundary: a
    # quotient of integers below 2^53 that equals 1/2 rounds to 1/2, and the
    # rounding is monotone)
    ok = np.flatnonzero(2 * T[ends] >= ends + 1)
    fdr = float(rec[ok[-1]]) if ok.size else 0.0
    return auc, aupr, fdr


def curve_metrics(pred, target):
    """{'allAUC', 'allAUPR', 'allFDR'}: (L,) fp64 with NaN where undefined, and
    mean / median / var of each over the labels that are not NaN."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target)
    L = pred.shape[1]
    vals = np.array([label_curves(pred[:, l], target[:, l]) for l in range(L)], np.float64)
    out = {}
    for j, name in enumerate(["AUC", "AUPR", "FDR"]):
        v = vals[:, j]
        keep = v[~np.isnan(v)]
        out["all" + name] = v
        out["mean" + name] = float(np.mean(keep)) if keep.size else np.nan
        out["median" + name] = float(np.median(keep)) if keep.size else np.nan
        out["var" + name] = float(np.var(keep)) if keep.size else np.nan
    return out
