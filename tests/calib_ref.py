"""torch restatement of the post-process threshold calibration
(fairsoft_train_postprocess.py:39-49, :112-165, :413-446) -- TEST
INFRASTRUCTURE ONLY, the checker of csrc/calib.hip.  Device- and
dtype-agnostic torch ops, differentiable by autograd: fp64 tensors on the CPU
pin it to the golden records (tests/test_calib_ref.py), and on the GPU it is
the reference of the kernel-edge and chained-gradient tests.  It decides the
active terms on the host (``if W > 0``), as the reference does.
"""
import numpy as np
import torch

from oracle.fairness import row_weights

EPS = 1e-6


def weights(labels, dists):
    """(T, B) fp64: row b's distance in each target's dict, 0 when absent."""
    labels = np.asarray(labels)
    if not dists:
        return np.zeros((0, labels.shape[0]), np.float64)
    return np.stack([row_weights(labels, d) for d in dists])


def group_of(sensitive, centroids):
    """Index of each row's sensitive pattern among the centroids' rows."""
    eq = (np.asarray(sensitive)[:, None, :] == np.asarray(centroids)[None, :, :]).all(-1)
    assert eq.any(1).all(), "a row matches no centroid"
    return eq.argmax(1)


def calibrate(p, thr, gid):
    """cal_prob[b, l] from probabilities ``thr`` (L, G), the column of row b's group."""
    a = torch.log(p / (1 - p + EPS))
    c = torch.log(thr / (1 - thr + EPS))
    return 1 / (torch.exp(-(a - c.t()[gid])) + 1)


def fair_terms(q, gid, w, G):
    """Squared distances between each group's and the batch's weighted mean of
    q, one per active (target, group) pair, in (t, k) order."""
    terms = []
    for wt in w:
        if not float(wt.sum()) > 0:
            continue
        mean_all = (wt[:, None] * q).sum(0) / wt.sum()
        for k in range(G):
            sel = gid == k
            if float(wt[sel].sum()) > 0:
                mean_k = (wt[sel, None] * q[sel]).sum(0) / wt[sel].sum()
                terms.append(((mean_k - mean_all) ** 2).sum())
    return terms


def losses(p, x, y, gid, w, learn_logit):
    """(bce, fair, number of terms, cal_prob) of one batch.  p, y (B, L);
    x (1, L, G) or (L, G); gid (B,) long; w (T, B); all of x's dtype and device."""
    x2 = x.reshape(x.shape[-2], x.shape[-1])
    thr = 1 / (torch.exp(-x2) + 1) if learn_logit else x2
    q = calibrate(p, thr, gid)
    bce = -(y * torch.log(q + EPS) + (1 - y) * torch.log(1 - q + EPS)).sum(1).mean()
    terms = fair_terms(q, gid, w, x2.shape[1])
    fair = sum(terms) if terms else torch.zeros((), dtype=q.dtype, device=q.device)
    return bce, fair, len(terms), q


def run64(p, x, y, sensitive, centroids, dists, learn_logit, g_bce=1.0, g_fair=1.0):
    """fp64 on the CPU from numpy inputs: values and the gradients of
    g_bce * bce + g_fair * fair w.r.t. x and p, as numpy."""
    pt = torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(np.asarray(y), dtype=torch.float64)
    gid = torch.from_numpy(group_of(sensitive, centroids))
    w = torch.from_numpy(weights(y, dists))
    bce, fair, n, q = losses(pt, xt, yt, gid, w, learn_logit)
    (g_bce * bce + g_fair * fair).backward()
    return dict(bce=float(bce.detach()), fair=float(fair.detach()), nterms=n,
                cal_prob=q.detach().numpy(),
                g_threshold=xt.grad.numpy(), g_p=pt.grad.numpy())


def mean_diff(q, labels, sensitive, centroids, dists):
    """fair_mean_diff of a split: the mean of the active terms, NaN when none."""
    qt = torch.tensor(np.asarray(q), dtype=torch.float64)
    gid = torch.from_numpy(group_of(sensitive, centroids))
    terms = fair_terms(qt, gid, torch.from_numpy(weights(labels, dists)), len(centroids))
    return float(torch.stack(terms).mean()) if terms else float("nan")
