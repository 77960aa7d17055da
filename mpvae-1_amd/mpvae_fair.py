"""Device versions of the two per-step consumers of compute_loss's
``indiv_prob`` / ``indiv_prob_label`` in the reference training loop
(SURVEY.md section 8(f), ranks 2 and 3):

* the fairness regulariser, fairsoft_train.py:75-138 -- per target fair label,
  row weights from ``label_distances[target]`` keyed by the row's label
  string (:85-93), the weighted batch mean and per-sensitive-group means of
  indiv_prob_label (label_z) and indiv_prob (feat_z), l1 or l2 distance,
  ``fairloss = fair_coeff * (reg_label_z_unfair + reg_feat_z_unfair)``;
* the per-step train metrics, ``evals.compute_metrics(indiv_prob, labels,
  0.5, all_metrics=False)`` (evals.py:178-238, used at fairsoft_train.py:149-153).

Both run in libmpvae_hip.so (csrc/fairness.hip) behind the C ABI; there is no
host fallback.  Differences from the reference, none of them numeric:
* the reference returns the Python float 0. when no target/group term is
  active (and then does not add it); ``fairness_penalty`` returns a zero
  fp64 tensor instead, which adds nothing -- deciding "float or tensor" would
  need a host sync every step;
* the penalty is computed in fp64 whatever the distance values are.  The
  reference's ``torch.tensor(weights)`` is float64 when the dict values are
  numpy float64 (label_distance*.py's ``np.clip(np.exp(...))``) and float32
  when they are Python floats (indication / constant / un-gamma'd Jaccard and
  Hamming), and the penalty then runs in fp32.  The returned loss takes the
  reference's dtype (fp32 when every table holds Python floats), its value
  differs from the reference's fp32 one by fp32 rounding only
  (tests/golden fair_f6/f7, tests/test_gpu_fair.py);
* the metrics come back as 0-d fp64 device tensors (``.item()`` works as on
  the reference's numpy scalars); p@k ties go to the larger label index
  (numpy's default argsort is not stable, so the reference's tie order is
  implementation-defined).

The validation form, ``compute_metrics(..., all_metrics=True)`` and
``best_threshold_metrics`` (the threshold sweep of validate_mpvae,
fairsoft_train.py:400-416), runs in csrc/curves.hip: one descending sort per
label of the whole validation split, then AUC / AUPR / FDR from per-run totals.
The sweep's threshold metrics come from csrc/sweep.hip
(``threshold_sweep_metrics``: every threshold from one read of the split;
``best_thresholds`` reads the winning thresholds off its table).
Differences from the reference:
* ``allAUC`` / ``allAUPR`` / ``allFDR`` always have length L; a label the
  metric is undefined for (AUC of a one-class label) holds NaN where the
  reference drops the entry;
* mean, median and variance skip the NaN labels.  That is what the reference's
  ``try / except ValueError`` did with the scikit-learn it was written for;
  a scikit-learn whose ``roc_auc_score`` returns NaN for a one-class label
  (with a warning) instead of raising makes the reference's own mean NaN;
* ``best_threshold_metrics`` reduces over the thresholds with torch.amax, which
  propagates NaN: a metric that is NaN at any threshold (ebF1 or maF1 with no
  defined term, meanAUC with no two-class label) comes back NaN, where
  Python's max / min keep or drop it depending on the order.
"""
import ctypes

import numpy as np
import torch

import mpvae_hip as H

_MIX = (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)
_M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + _MIX[0]) & _M64
    z = ((z ^ (z >> 30)) * _MIX[1]) & _M64
    z = ((z ^ (z >> 27)) * _MIX[2]) & _M64
    return z ^ (z >> 31)


def pack_pattern(key, L):
    """The reference's key string (``''.join(label.astype(str))``) -> W words,
    bit j of word w = label 64w + j.  None if the string is not a 0/1 pattern
    of length L (such a key can never match a binary label row)."""
    if len(key) != L or any(c not in "01" for c in key):
        return None
    W = (L + 63) // 64
    words = [0] * W
    for i, c in enumerate(key):
        if c == "1":
            words[i // 64] |= 1 << (i % 64)
    return words


def pattern_hash(words):
    h = 0x6A09E667F3BCC909 ^ len(words)
    for x in words:
        h = _mix64(h ^ x)
    return h


class LabelDistanceTable:
    """One target label's ``label_distances[target]`` dict (label string ->
    distance) as a device open-addressing table (mpv_label_table).

    ``ref_dtype`` is decided once per table: float64 if any value is a numpy
    float64, else float32.  The reference decides per batch, from the values
    actually looked up (``torch.tensor(weights)``) and promoted over the
    targets that were active in that batch -- a data-dependent host decision.
    The two agree whenever a table's values share one type (every
    label_distance*.py table does); for a table mixing Python floats and numpy
    float64, or an fp64 table inactive in a batch beside an active fp32 one,
    the returned loss is fp64 where the reference's is fp32, a difference of
    fp32 rounding only (the arithmetic is fp64 here either way)."""

    def __init__(self, distances, label_dim, device):
        self.L, self.W = label_dim, (label_dim + 63) // 64
        # torch.tensor() of the looked-up values is float64 iff they are numpy
        # float64 (fairsoft_train.py:91-97); Python floats give float32
        self.ref_dtype = torch.float64 if any(isinstance(v, np.float64)
                                              for v in distances.values()) else torch.float32
        items = [(pack_pattern(k, label_dim), float(v)) for k, v in distances.items()]
        items = [(w, v) for w, v in items if w is not None]
        n = 1
        while n < 2 * max(1, len(items)):
            n *= 2
        keys = np.zeros((n, self.W), np.uint64)
        vals = np.zeros(n, np.float64)
        used = np.zeros(n, np.int32)
        for words, v in items:
            slot = pattern_hash(words) & (n - 1)
            while used[slot] and list(keys[slot]) != words:
                slot = (slot + 1) & (n - 1)
            keys[slot] = np.array(words, np.uint64)
            vals[slot] = v
            used[slot] = 1
        self.nslots = n if items else 0
        self.keys = torch.from_numpy(keys.view(np.int64).copy()).to(device)
        self.vals = torch.from_numpy(vals).to(device)
        self.used = torch.from_numpy(used).to(device)

    def c_struct(self):
        return H.LabelTable(H.ptr(self.keys), H.ptr(self.vals), H.ptr(self.used), self.nslots,
                            self.W)


def label_weights(labels, tables):
    """(T, B) fp64 row weights, one row per target table, and the int32 count
    of (target, row) pairs with a positive weight (fairsoft_train.py:85-93)."""
    H.require_gpu(labels)
    y = labels.contiguous().float()
    B, L = y.shape
    w = torch.empty((len(tables), B), dtype=torch.float64, device=y.device)
    count = torch.zeros((), dtype=torch.int32, device=y.device)
    if B == 0:  # no row to look up: no launch with an empty grid
        return w, count
    lib, st = H.load_library(), H.stream_of(y.device)
    for t, tab in enumerate(tables):
        if tab.L != L:
            raise ValueError(f"table built for label_dim {tab.L}, labels have {L}")
        s = tab.c_struct()
        H.check(lib.mpv_label_weights(H.ptr(y), B, L, ctypes.byref(s), H.ptr(w[t]), H.ptr(count),
                                      st), "mpv_label_weights")
    return w, count


def group_ids(sensitive_feat):
    """Row b's index in ``torch.unique(sensitive_feat, dim=0)`` (the reference's
    group order, fairsoft_train.py:80, :103-104), from fixed-size tensor ops:
    the number of distinct rows that sort before row b (lexicographically).
    No data-dependent shape and no host sync, so it can be captured in a HIP
    graph; O(B^2 n_sensitive) compares, a few microseconds at B = 512."""
    B = sensitive_feat.shape[0]
    if B == 0:  # reshape(0, -1) cannot infer the second size
        return torch.zeros(0, dtype=torch.int32, device=sensitive_feat.device)
    X = sensitive_feat.reshape(B, -1)
    ne = X[:, None, :] != X[None, :, :]                         # [c, b, j]
    differ = ne.any(-1)                                         # rows c, b differ
    first = ne.to(torch.uint8).argmax(-1, keepdim=True)         # first differing column
    less = differ & (torch.gather(X[:, None, :].expand(B, B, X.shape[1]), 2, first) <
                     torch.gather(X[None, :, :].expand(B, B, X.shape[1]), 2, first)).squeeze(-1)
    # row c is the first occurrence of its pattern: no earlier identical row
    earlier = torch.ones(B, B, dtype=torch.bool, device=X.device).triu(1)  # [c', c]: c' < c
    firsts = ~((~differ) & earlier).any(0)
    return (less & firsts[:, None]).sum(0).to(torch.int32)


def sensitive_groups(sensitive_feat, max_groups=None):
    """(gid, order, goff, G, overflow): group id per row (``group_ids``), the
    rows listed group by group, and the group offsets, for G group slots.  G is
    ``max_groups`` (an upper bound on the distinct sensitive patterns of a
    batch, e.g. of the whole dataset, known on the host once) or the batch
    size: the slots past the batch's own groups stay empty, and an empty group
    adds nothing (its weight sum is 0, the reference's
    ``weight_sensitive.sum() > 0`` gate).  A batch with more distinct patterns
    than ``max_groups`` sets the 0-d bool device tensor ``overflow`` (its ids
    are clamped into range, so no kernel reads out of bounds; the penalty
    turns NaN).  Nothing here waits for the device."""
    gid = group_ids(sensitive_feat)
    B = gid.numel()
    G = int(max_groups) if max_groups is not None else max(B, 1)
    if G < 1:
        raise ValueError(f"max_groups must be >= 1 (got {max_groups})")
    overflow = (gid >= G).any()
    gid = gid.clamp(max=G - 1)
    order = torch.argsort(gid, stable=True).to(torch.int32)
    counts = torch.zeros(G, dtype=torch.int32, device=gid.device)
    counts.index_add_(0, gid.long(), torch.ones_like(gid))
    goff = torch.zeros(G + 1, dtype=torch.int32, device=gid.device)
    goff[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return gid.contiguous(), order.contiguous(), goff, G, overflow


class _FairPenalty(torch.autograd.Function):
    @staticmethod
    def forward(ctx, label_z, feat_z, w, gid, order, goff, G, norm, fair_coeff):
        lz, fz = label_z.detach().contiguous().float(), feat_z.detach().contiguous().float()
        B, L = lz.shape
        T = w.shape[0]
        lib, st = H.load_library(), H.stream_of(lz.device)
        nbytes = lib.mpv_fair_workspace_bytes(L, T, G)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=lz.device)
        out = torch.empty((), dtype=torch.float64, device=lz.device)
        a = H.FairArgs(H.ptr(lz), H.ptr(fz), H.ptr(w), H.ptr(order), H.ptr(goff), H.ptr(gid), B, L,
                       T, G, norm, float(fair_coeff), H.ptr(out))
        H.check(lib.mpv_fair_fwd(ctypes.byref(a), H.ptr(ws), nbytes, st), "mpv_fair_fwd")
        ctx.keep = (lz, fz, w, gid, order, goff, ws, a, nbytes)
        ctx.dtypes = (label_z.dtype, feat_z.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        lz, fz, w, gid, order, goff, ws, a, nbytes = ctx.keep
        g = gout.detach().to(torch.float64).contiguous()
        gl, gf = torch.empty_like(lz), torch.empty_like(fz)
        lib = H.load_library()
        H.check(lib.mpv_fair_bwd(ctypes.byref(a), H.ptr(g), H.ptr(gl), H.ptr(gf), H.ptr(ws), nbytes,
                                 H.stream_of(lz.device)), "mpv_fair_bwd")
        return (gl.to(ctx.dtypes[0]), gf.to(ctx.dtypes[1])) + (None,) * 7


class _ZeroPenalty(torch.autograd.Function):
    """The penalty of an empty batch or of no target table: the reference
    leaves ``fairloss = 0.`` (fairsoft_train.py:83).  A zero that is still a
    differentiable function of both inputs, with zero gradients, and launches
    no kernel of csrc/fairness.hip."""

    @staticmethod
    def forward(ctx, label_z, feat_z):
        ctx.save_for_backward(label_z, feat_z)
        return torch.zeros((), dtype=torch.float64, device=label_z.device)

    @staticmethod
    def backward(ctx, gout):
        return tuple(torch.zeros_like(t) for t in ctx.saved_tensors)


NORMS = {"l1": H.FAIR_L1, "l2": H.FAIR_L2}


def fairness_penalty(indiv_prob_label, indiv_prob, input_label, sensitive_feat, tables,
                     fairness_loss_norm, fair_coeff, max_groups=None):
    """fairsoft_train.py:75-131 on the device.

    indiv_prob_label, indiv_prob -- compute_loss outputs 8 and 7 (label_z, feat_z)
    input_label                   -- (B, L) batch labels (data.labels[idx])
    sensitive_feat                -- (B, n_sensitive) (data.sensitive_feat[idx])
    tables                        -- [LabelDistanceTable(label_distances[t], L, dev)
                                      for t in target_fair_labels]
    max_groups                    -- optional upper bound on the distinct sensitive
                                     patterns in a batch (default: the batch size;
                                     a batch with more distinct patterns than the
                                     bound makes the penalty NaN)
    No host sync: the call (forward and backward) can be captured in a HIP
    graph (tests/test_gpu_fair.py).
    Returns ``(fairloss, contributed)``: fairloss is a differentiable 0-d
    tensor to add to total_loss (zero when no term is active), computed in fp64
    and returned in the reference's dtype (fp64 if any table holds numpy
    float64 distances, else fp32), contributed the
    int32 count that the reference adds to contributed_reg_fair_sample.
    An empty batch or ``tables=[]`` gives an fp64 zero with zero gradients and
    a zero count, as the reference's ``fairloss = 0.``."""
    H.require_gpu(indiv_prob_label, indiv_prob, input_label, sensitive_feat)
    if indiv_prob_label.shape[0] == 0 or not tables:
        # shapes and len(tables) are host knowledge: no sync, still capturable
        count = torch.zeros((), dtype=torch.int32, device=indiv_prob_label.device)
        return _ZeroPenalty.apply(indiv_prob_label, indiv_prob), count
    w, count = label_weights(input_label, tables)
    gid, order, goff, G, overflow = sensitive_groups(sensitive_feat, max_groups)
    norm = NORMS.get(fairness_loss_norm, 0)
    loss = _FairPenalty.apply(indiv_prob_label, indiv_prob, w, gid, order, goff, G, norm,
                              fair_coeff)
    if max_groups is not None:  # G < B: a batch may hold more patterns than the bound
        loss = torch.where(overflow, torch.full_like(loss, float("nan")), loss)
    if tables and all(t.ref_dtype == torch.float32 for t in tables):
        loss = loss.float()
    return loss, count


METRIC_KEYS = ["ACC", "HA", "ebF1", "miF1", "maF1", "p_at_1", "p_at_3", "p_at_5"]
CURVE_KEYS = ["meanAUC", "medianAUC", "varAUC", "meanAUPR", "medianAUPR", "varAUPR", "meanFDR",
              "medianFDR", "varFDR"]
CURVE_CHUNK = 4096  # keys one workgroup sorts in LDS by default (curves.hip kCurveChunk)
# validate_mpvae's sweep and the metrics it keeps (train.py:22-24, restated)
THRESHOLDS = [0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.10, 0.15, 0.20, 0.25, 0.30,
              0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65, 0.70, 0.75, 0.80, 0.85, 0.90, 0.95]
METRICS = ["ACC", "HA", "ebF1", "miF1", "maF1", "meanAUC", "medianAUC", "meanAUPR", "medianAUPR",
           "meanFDR", "medianFDR", "p_at_1", "p_at_3", "p_at_5"]


def _train_metrics(p, t, threshold):
    """mpv_train_metrics on contiguous fp32 device tensors -> (8,) fp64."""
    B, L = p.shape
    lib = H.load_library()
    nbytes = lib.mpv_metrics_workspace_bytes(B, L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty(8, dtype=torch.float64, device=p.device)
    H.check(lib.mpv_train_metrics(H.ptr(p), H.ptr(t), B, L, float(threshold), H.ptr(out), H.ptr(ws),
                                  nbytes, H.stream_of(p.device)), "mpv_train_metrics")
    return out


def curve_metrics(predictions, targets, chunk=0):
    """Per-label AUC, AUPR and FDR of (N, L) scores against 0/1 targets
    (evals.py:129-175) and their aggregates: ``{"allAUC", "allAUPR", "allFDR"}``
    as (L,) fp64 device tensors (NaN where undefined) and the nine CURVE_KEYS
    as 0-d fp64 device tensors (mean / median / population variance over the
    labels that are not NaN; NaN when none is kept).  ``chunk`` is the number
    of keys one workgroup sorts in LDS (0: the default; a smaller power of two
    >= 64 forces the global merge passes at a small N -- the results do not
    depend on it).  No host sync."""
    H.require_gpu(predictions, targets)
    p = predictions.detach().contiguous().float()
    t = targets.detach().contiguous().float()
    N, L = p.shape
    lib = H.load_library()
    nbytes = lib.mpv_curves_workspace_bytes(N, L, chunk)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=p.device)
    per = torch.empty((3, L), dtype=torch.float64, device=p.device)
    agg = torch.empty(9, dtype=torch.float64, device=p.device)
    a = H.CurveArgs(H.ptr(p), H.ptr(t), N, L, chunk, H.ptr(per[0]), H.ptr(per[1]), H.ptr(per[2]),
                    H.ptr(agg))
    H.check(lib.mpv_curve_metrics(ctypes.byref(a), H.ptr(ws), nbytes, H.stream_of(p.device)),
            "mpv_curve_metrics")
    res = {"allAUC": per[0], "allAUPR": per[1], "allFDR": per[2]}
    res.update({k: agg[i] for i, k in enumerate(CURVE_KEYS)})
    return res


def compute_metrics(predictions, targets, threshold, all_metrics=False, chunk=0):
    """evals.compute_metrics (evals.py:178-238): the same keys, values 0-d fp64
    device tensors.  all_metrics=False is the per-step call (the AUC / AUPR /
    FDR entries 0 as in the reference); all_metrics=True adds ``curve_metrics``
    (see there and the module docstring for ``chunk`` and the differences from
    the reference).  No host sync either way."""
    H.require_gpu(predictions, targets)
    p = predictions.detach().contiguous().float()
    t = targets.detach().contiguous().float()
    out = _train_metrics(p, t, threshold)
    res = {k: out[i] for i, k in enumerate(METRIC_KEYS)}
    if all_metrics:
        res.update(curve_metrics(p, t, chunk))
    else:
        for k in CURVE_KEYS + ["allAUC", "allAUPR", "allFDR"]:
            res[k] = 0
    return res


def threshold_sweep_metrics(predictions, targets, thresholds=THRESHOLDS):
    """The threshold metrics of ``compute_metrics(predictions, targets, thr)``
    at every ``thr`` of ``thresholds`` from one read of the split
    (mpv_threshold_sweep, csrc/sweep.hip): an (n_thr, 8) fp64 device tensor,
    row j for ``thresholds[j]``, columns in METRIC_KEYS order.  The thresholds
    need no order and may repeat; more than 64 run in slices of 64.  ACC, miF1
    and p_at_1 equal the per-threshold call bit for bit, the others differ
    from it by the order of fp64 additions only.  No host sync."""
    thresholds = [float(x) for x in thresholds]
    if not thresholds:
        raise ValueError("threshold_sweep_metrics needs at least one threshold")
    H.require_gpu(predictions, targets)
    p = predictions.detach().contiguous().float()
    t = targets.detach().contiguous().float()
    N, L = p.shape
    lib, st = H.load_library(), H.stream_of(p.device)
    out = torch.empty((len(thresholds), 8), dtype=torch.float64, device=p.device)
    for j0 in range(0, len(thresholds), H.MAX_THRESHOLDS):
        part = thresholds[j0:j0 + H.MAX_THRESHOLDS]
        nbytes = lib.mpv_sweep_workspace_bytes(N, L, len(part))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=p.device)
        a = H.SweepArgs(H.ptr(p), H.ptr(t), N, L, len(part),
                        (ctypes.c_float * H.MAX_THRESHOLDS)(*part), H.ptr(out[j0]))
        H.check(lib.mpv_threshold_sweep(ctypes.byref(a), H.ptr(ws), nbytes, st),
                "mpv_threshold_sweep")
    return out


def best_thresholds(table, thresholds):
    """For each of the eight METRIC_KEYS the first threshold at which the
    metric attains its maximum over the rows of ``table`` (the result of
    ``threshold_sweep_metrics`` for ``thresholds``), as 0-d fp64 tensors on the
    table's device; NaN where the column holds a NaN, in line with ``amax``.
    torch ops on the small table only: no host sync."""
    thr = torch.as_tensor([float(x) for x in thresholds], dtype=torch.float64, device=table.device)
    if table.dim() != 2 or table.shape[0] != thr.numel() or table.shape[1] != len(METRIC_KEYS):
        raise ValueError(f"table {tuple(table.shape)} is not ({thr.numel()}, {len(METRIC_KEYS)})")
    best = table.amax(0, keepdim=True)  # NaN where the column holds one
    hit = (table == best).to(torch.uint8)  # all False in a NaN column
    first = hit.argmax(0)  # the first maximal element
    picked = torch.where(torch.isnan(best[0]), torch.full_like(best[0], float("nan")), thr[first])
    return {k: picked[i] for i, k in enumerate(METRIC_KEYS)}


def best_threshold_metrics(predictions, targets, thresholds=THRESHOLDS):
    """The selection loop of validate_mpvae (fairsoft_train.py:400-416) on the
    device: the METRICS of ``compute_metrics(..., thr, all_metrics=True)``
    reduced over ``thresholds``, the maximum of each, the minimum for the FDR
    entries.  The curve metrics (the FDR entries among them) do not depend on
    the threshold, so they are computed once and are their own maximum and
    minimum; the threshold metrics come from ``threshold_sweep_metrics`` (one
    pass over the split for all thresholds) and their maximum is reduced on
    the device.
    Returns the 14 METRICS as 0-d fp64 device tensors; a NaN at any threshold
    propagates (module docstring).  No host sync."""
    H.require_gpu(predictions, targets)
    p = predictions.detach().contiguous().float()
    t = targets.detach().contiguous().float()
    curves = curve_metrics(p, t)
    per_thr = threshold_sweep_metrics(p, t, thresholds)  # (n_thr, 8)
    best8 = per_thr.amax(0)  # propagates NaN; none of the eight is an FDR entry
    best = {k: best8[i] for i, k in enumerate(METRIC_KEYS)}
    return {k: best[k] if k in best else curves[k] for k in METRICS}
