"""numpy fp64 restatement of the closed-form label similarities
(mpvae_fair.LabelSimilarity, label_sim_kernel in csrc/fairness.hip): the value
label_distance_obs.py's builders store for a (target, pattern) pair, from the
two 0/1 patterns.  tests/golden/labelsim_*.npz hold the reference's own values;
tests/test_labelsim_host.py checks this restatement against them."""
import numpy as np

KINDS = ["indication", "constant", "jaccard", "hamming"]


def similarity(kind, target, rows):
    """(N,) fp64 similarity of each 0/1 row of ``rows`` (N, L) to ``target`` (L,)."""
    rows = np.asarray(rows).astype(bool)
    tgt = np.asarray(target).astype(bool)
    L = rows.shape[1]
    n_and = (rows & tgt).sum(1).astype(np.float64)
    n_or = (rows | tgt).sum(1).astype(np.float64)
    n_xor = (rows ^ tgt).sum(1).astype(np.float64)
    if kind == "indication":
        return (n_xor == 0).astype(np.float64)
    if kind == "constant":
        return np.ones(rows.shape[0], np.float64)
    if kind == "jaccard":
        return np.where(n_xor == 0, 1.0, n_and / np.maximum(n_or, 1.0))
    if kind == "hamming":
        return (L - n_xor) / np.float64(L)
    raise ValueError(kind)


def weights(kind, target, rows, gamma=None, clip=(0.0, 1.0)):
    """The stored value: the similarity, or with ``gamma``
    ``np.clip(np.exp(gamma * (sim - 1)), *clip)``."""
    sim = similarity(kind, target, rows)
    if gamma is None:
        return sim
    return np.clip(np.exp(np.float64(gamma) * (sim - 1.0)), clip[0], clip[1])


def label_weights(kind, target, labels, gamma=None, clip=(0.0, 1.0)):
    """``weights`` for float label rows as the kernel reads them: values are
    truncated, and a row with a value that is then neither 0 nor 1 (NaN
    included) gets 0."""
    y = np.trunc(np.asarray(labels, np.float32))
    bad = ~((y == 0) | (y == 1)).all(1)
    w = weights(kind, target, y == 1, gamma, clip)
    w[bad] = 0.0
    return w


def ulp_distance(a, b):
    """Largest distance in fp64 ulps between two arrays of finite,
    non-negative values."""
    a = np.ascontiguousarray(a, np.float64).view(np.int64)
    b = np.ascontiguousarray(b, np.float64).view(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0
