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
host fallback.  ``fairness_penalty(..., fused=True)`` takes the row weights of
every target table from one launch (``label_weights_batch``) and the batch's
sensitive groups from one launch (``group_rows``) where the default path
launches once per table and builds the groups from torch ops
(``sensitive_groups``); the results are equal bit for bit.
Differences from the reference, none of them numeric:
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
* a ``LabelSimilarity`` (the row weights as a closed form of the row's and
  the target's patterns, row_weights_kernel<LabelSims>; accepted wherever a
  ``LabelDistanceTable`` is) gives every binary row its formula weight, where
  the reference's dict holds only the patterns that occur in the dataset and
  ``.get(key, 0.)`` gives 0 for any other.  The two agree for rows taken from
  the dataset, which the train, validation and test splits always are; a
  caller who needs the miss keeps the table;
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

The post-process method's consumer of ``indiv_prob``
(fairsoft_train_postprocess.py: one decision threshold per label and sensitive
group, learned on a frozen model) runs in csrc/calib.hip: ``calibration_loss``,
``calibrate`` and ``fair_mean_diff`` further down, with their own list of
differences.

The evaluation's scoring of a whole split (fairsoft_evaluate.evaluate_mpvae,
:83-121: the "soft" F1 of the raw probabilities and the mean Euclidean
distance between group and split means) runs in csrc/evalsplit.hip:
``split_scores`` at the end of this module, again with its own list, and
``split_scores_defs``, the same split scored under many weight definitions
(the distance sweep of fairsoft_metric.evaluate_models_over_label_distances)
from one pass.
"""
import collections
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


SIM_KINDS = {"indication": H.SIM_INDICATION, "constant": H.SIM_CONSTANT,
             "jaccard": H.SIM_JACCARD, "hamming": H.SIM_HAMMING}


class LabelSimilarity:
    """One target label's row weights as a closed form of the row's and the
    target's 0/1 patterns: what label_distance_obs.py's builders store in
    ``label_distances[target]`` (indication_similarity :9-25,
    constant_similarity :28-44, str_jac_similarity :54-69, str_ham_similarity
    :120-127; with ``gamma`` the ``np.clip(np.exp(gamma * (sim - 1)), *clip)``
    of the ``_nonlinear`` builders, :106-108), computed per row on the device
    (row_weights_kernel<LabelSims>) instead of built as a dict over every pair of the
    dataset's patterns.  Accepted wherever a ``LabelDistanceTable`` is, also
    mixed with tables in one list.

    kind      -- "indication", "constant", "jaccard" or "hamming"
    target    -- the target pattern: a 0/1 vector of length ``label_dim`` or
                 the reference's key string
    gamma     -- the reference's ``args.dist_gamma``; None: the similarity itself
    clip      -- (minimum_clip, maximum_clip), read with ``gamma`` only

    ``ref_dtype`` follows ``LabelDistanceTable``'s rule: with a gamma the
    reference stores numpy float64 values (fp64), without it Python floats
    (fp32).  ``kind="hamming"`` without gamma is ``str_ham_similarity``; the
    reference's own wrapper for that case (``_hamming_similarity``) raises.

    The one difference from the reference's dict: the dict holds the
    dataset's patterns only and gives 0 for any other row, the closed form
    gives every binary row its formula weight.  Rows taken from the dataset
    (the train, validation and test splits) get the same weight either way; a
    caller who needs the miss keeps the table."""

    def __init__(self, kind, target, label_dim, device, gamma=None, clip=(0.0, 1.0)):
        if kind not in SIM_KINDS:
            raise ValueError(f"unknown similarity kind {kind!r} (one of {sorted(SIM_KINDS)})")
        self.kind, self.L, self.W = kind, int(label_dim), (int(label_dim) + 63) // 64
        if not isinstance(target, str):
            vals = torch.as_tensor(target).reshape(-1).tolist()
            if any(v not in (0, 1) for v in vals):
                raise ValueError("a similarity target must be a 0/1 pattern")
            target = "".join(str(int(v)) for v in vals)
        words = pack_pattern(target, self.L)
        if words is None:
            raise ValueError(f"target {target!r} is not a 0/1 pattern of length {self.L}")
        self.key = target
        self.gamma = None if gamma is None else float(gamma)
        self.clip = (float(clip[0]), float(clip[1]))
        self.ref_dtype = torch.float32 if gamma is None else torch.float64
        self.target = torch.from_numpy(np.array(words, np.uint64).view(np.int64).copy()).to(device)

    def c_struct(self):
        return H.LabelSim(H.ptr(self.target), SIM_KINDS[self.kind], int(self.gamma is not None),
                          0.0 if self.gamma is None else self.gamma, self.clip[0], self.clip[1])


def _check_label_dim(sources, L):
    for s in sources:
        if s.L != L:
            what = "similarity" if isinstance(s, LabelSimilarity) else "table"
            raise ValueError(f"{what} built for label_dim {s.L}, labels have {L}")


def _source_runs(sources):
    """The maximal runs of one kind in a list of weight sources:
    ``[(t0, t1, is_similarity)]``; each run fills rows [t0, t1) of w."""
    runs = []
    for t, s in enumerate(sources):
        sim = isinstance(s, LabelSimilarity)
        if runs and runs[-1][2] == sim:
            runs[-1][1] = t + 1
        else:
            runs.append([t, t + 1, sim])
    return runs


def _weights_prep(labels, sources):
    """What every row-weights entry point sets up: ``(y, w, count)``, the labels
    as contiguous fp32, the (T, B) fp64 weights to fill and the zero int32
    count.  With no row nothing is looked up or launched (no empty grid), so
    the caller returns ``(w, count)`` as they are; else the sources' label_dim
    is checked."""
    H.require_gpu(labels)
    y = labels.contiguous().float()
    B, L = y.shape
    w = torch.empty((len(sources), B), dtype=torch.float64, device=y.device)
    count = torch.zeros((), dtype=torch.int32, device=y.device)
    if B:
        _check_label_dim(sources, L)
    return y, w, count


def _sim_weights_into(y, sims, w, count):
    """mpv_label_sim_weights on contiguous fp32 device labels into rows of w."""
    B, L = y.shape
    structs = (H.LabelSim * max(1, len(sims)))(*[s.c_struct() for s in sims])
    H.check(H.load_library().mpv_label_sim_weights(H.ptr(y), B, L, structs, len(sims), H.ptr(w),
                                                   H.ptr(count), H.stream_of(y.device)),
            "mpv_label_sim_weights")


def _sim_weights_host(labels, sims):
    """``similarity_weights`` on CPU tensors: row_weights_kernel<LabelSims>'s formulas in
    fp64 torch ops, (T, N).  A row that is not exact 0 / 1 after truncation
    gets 0."""
    y = labels.detach().float().trunc()
    N, L = y.shape
    bad = ~((y == 0) | (y == 1)).all(1)
    bits = y == 1
    w = torch.zeros((len(sims), N), dtype=torch.float64)
    one = torch.ones(N, dtype=torch.float64)
    for t, s in enumerate(sims):
        tgt = torch.tensor([c == "1" for c in s.key], dtype=torch.bool)
        n_and = (bits & tgt).sum(1).double()
        n_or = (bits | tgt).sum(1).double()
        n_xor = (bits ^ tgt).sum(1).double()
        if s.kind == "indication":
            sim = (n_xor == 0).double()
        elif s.kind == "constant":
            sim = one
        elif s.kind == "jaccard":
            sim = torch.where(n_xor == 0, one, n_and / n_or.clamp(min=1.0))
        else:
            sim = (L - n_xor) / L
        if s.gamma is not None:
            sim = torch.exp(s.gamma * (sim - 1.0)).clamp(s.clip[0], s.clip[1])
        w[t] = sim
    w[:, bad] = 0.0
    return w


def similarity_weights(labels, sims):
    """``(w (T, B) fp64, count int32)``: row t the weights of ``labels``' rows
    under the ``LabelSimilarity`` ``sims[t]``, and the number of positive
    weights (the reference's contributed_reg_fair_sample, fairsoft_train.py:
    91-92).  A row whose ``int()`` values are not all 0 or 1 gets 0 under every
    definition.  CUDA tensors run mpv_label_sim_weights (one launch per
    ``H.LABEL_SIMS_PER_LAUNCH`` definitions, no host sync); CPU tensors run the
    same formulas in fp64 torch ops: dispatch by device, never a fallback."""
    sims = list(sims)
    if any(not isinstance(s, LabelSimilarity) for s in sims):
        raise TypeError("similarity_weights takes LabelSimilarity objects")
    L = labels.shape[1]
    _check_label_dim(sims, L)
    if labels.device.type == "cpu":
        w = _sim_weights_host(labels, sims)
        return w, (w > 0).sum().to(torch.int32)
    y, w, count = _weights_prep(labels, sims)
    if y.shape[0] == 0:
        return w, count
    _sim_weights_into(y, sims, w, count)
    return w, count


def label_weights(labels, tables):
    """(T, B) fp64 row weights, one row per target table, and the int32 count
    of (target, row) pairs with a positive weight (fairsoft_train.py:85-93).
    A ``LabelSimilarity`` in the list fills its row from its closed form
    (mpv_label_sim_weights), one launch each."""
    y, w, count = _weights_prep(labels, tables)
    B, L = y.shape
    if B == 0:
        return w, count
    lib, st = H.load_library(), H.stream_of(y.device)
    for t, tab in enumerate(tables):
        if isinstance(tab, LabelSimilarity):
            _sim_weights_into(y, [tab], w[t], count)
            continue
        s = tab.c_struct()
        H.check(lib.mpv_label_weights(H.ptr(y), B, L, ctypes.byref(s), H.ptr(w[t]), H.ptr(count),
                                      st), "mpv_label_weights")
    return w, count


def label_weights_batch(labels, tables):
    """``label_weights`` with every target table in one launch per
    ``H.LABEL_TABLES_PER_LAUNCH`` tables (mpv_label_weights_batch): each row is
    packed and hashed once, then looked up in every table.  The same ``(w,
    count)``, bit for bit.  A list may mix tables and ``LabelSimilarity``
    objects: every maximal run of one kind is one call (mpv_label_weights_batch
    or mpv_label_sim_weights) that fills the run's rows of w."""
    y, w, count = _weights_prep(labels, tables)
    B, L = y.shape
    if B == 0:
        return w, count
    for t0, t1, sim in _source_runs(tables):
        if sim:
            _sim_weights_into(y, tables[t0:t1], w[t0], count)
            continue
        structs = (H.LabelTable * (t1 - t0))(*[tab.c_struct() for tab in tables[t0:t1]])
        H.check(H.load_library().mpv_label_weights_batch(H.ptr(y), B, L, structs, t1 - t0,
                                                         H.ptr(w[t0]), H.ptr(count),
                                                         H.stream_of(y.device)),
                "mpv_label_weights_batch")
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


def _group_layout(gid, G):
    """(order, goff): the rows listed group by group (a stable sort) and the
    group offsets, for group ids in [0, G)."""
    order = torch.argsort(gid, stable=True).to(torch.int32)
    counts = torch.zeros(G, dtype=torch.int32, device=gid.device)
    counts.index_add_(0, gid.long(), torch.ones_like(gid))
    goff = torch.zeros(G + 1, dtype=torch.int32, device=gid.device)
    goff[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return order.contiguous(), goff


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
    gid = gid.clamp(max=G - 1).contiguous()
    order, goff = _group_layout(gid, G)
    return gid, order, goff, G, overflow


_ELEMS = {torch.float32: H.EL_F32, torch.float64: H.EL_F64, torch.int32: H.EL_I32,
          torch.int64: H.EL_I64}


def group_rows(sensitive_feat, max_groups=None):
    """``sensitive_groups(sensitive_feat, max_groups)`` in one launch
    (mpv_group_rows): the same ``(gid, order, goff, G, overflow)``, equal
    element for element.  fp32 / fp64 / int32 / int64 features are read as they
    are (``torch.from_numpy(data.sensitive_feat[idx])`` is int64 or float64);
    any other dtype is cast once, to int64 if integral or bool, to float32
    otherwise.  A shape outside the kernel's range (more than
    ``H.GROUP_MAX_B`` rows or group slots, more than ``H.GROUP_MAX_N``
    columns) goes through ``sensitive_groups``.  No host sync."""
    H.require_gpu(sensitive_feat)
    B = sensitive_feat.shape[0]
    G = int(max_groups) if max_groups is not None else max(B, 1)
    if G < 1:
        raise ValueError(f"max_groups must be >= 1 (got {max_groups})")
    dev = sensitive_feat.device
    if B == 0:  # no row to group: no launch (group_ids' guard)
        return (torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(G + 1, dtype=torch.int32, device=dev), G,
                torch.zeros((), dtype=torch.bool, device=dev))
    x = sensitive_feat.reshape(B, -1)
    if x.dtype not in _ELEMS:
        x = x.to(torch.float32 if x.dtype.is_floating_point else torch.int64)
    x = x.contiguous()
    gid = torch.empty(B, dtype=torch.int32, device=dev)
    order = torch.empty(B, dtype=torch.int32, device=dev)
    goff = torch.empty(G + 1, dtype=torch.int32, device=dev)
    overflow = torch.empty((), dtype=torch.bool, device=dev)
    rc = H.load_library().mpv_group_rows(H.ptr(x), _ELEMS[x.dtype], B, x.shape[1], G, H.ptr(gid),
                                         H.ptr(order), H.ptr(goff), H.ptr(overflow),
                                         H.stream_of(dev))
    if rc == H.EINVAL:  # outside the kernel's range: nothing was launched
        return sensitive_groups(sensitive_feat, max_groups)
    H.check(rc, "mpv_group_rows")
    return gid, order, goff, G, overflow


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
                     fairness_loss_norm, fair_coeff, max_groups=None, *, fused=False):
    """fairsoft_train.py:75-131 on the device.

    indiv_prob_label, indiv_prob -- compute_loss outputs 8 and 7 (label_z, feat_z)
    input_label                   -- (B, L) batch labels (data.labels[idx])
    sensitive_feat                -- (B, n_sensitive) (data.sensitive_feat[idx])
    tables                        -- [LabelDistanceTable(label_distances[t], L, dev)
                                      for t in target_fair_labels], or
                                     ``LabelSimilarity`` objects, or both mixed
    max_groups                    -- optional upper bound on the distinct sensitive
                                     patterns in a batch (default: the batch size;
                                     a batch with more distinct patterns than the
                                     bound makes the penalty NaN)
    fused                         -- the row weights and the groups from one launch
                                     each (``label_weights_batch``, ``group_rows``)
                                     instead of one launch per table and the
                                     torch ops of ``sensitive_groups``: the same
                                     integers and weights, so the same loss and
                                     gradients bit for bit
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
    w, count = (label_weights_batch if fused else label_weights)(input_label, tables)
    gid, order, goff, G, overflow = (group_rows if fused else sensitive_groups)(sensitive_feat,
                                                                                max_groups)
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


# ------------------------------------------------ post-process calibration
# fairsoft_train_postprocess.py on the device (csrc/calib.hip): one decision
# threshold per (label, sensitive group) learned on a frozen model
# (postprocess_threshold_one_epoch, :52-198) and scored over a split
# (evaluate_fair_through_postprocess, :304-464).  Differences from the
# reference, none of them numeric beyond rounding:
# * fp64 arithmetic from the fp32 probabilities and thresholds, where the
#   reference runs calibrate_p and the BCE in fp32; ``bce`` comes back in
#   fp32, ``fair`` in the tables' reference dtype (as ``fairness_penalty``);
# * the fairness groups are the dataset's centroids (``centroids``), not the
#   batch's own ``torch.unique``: the same partition, since a centroid with no
#   row in the batch adds nothing; one group id per row serves the threshold
#   column and the fairness groups;
# * ``fair`` is a zero tensor and ``active`` False where the reference leaves
#   ``fair_loss`` the Python float 0.;
# * a row whose sensitive pattern is no centroid makes both losses NaN (the
#   reference's boolean-mask indexing would drop the row and then fail on the
#   shape mismatch with input_label).

def centroid_ids(sensitive_feat, centroids):
    """``(gid, unmatched)``: the index of each row's sensitive pattern among the
    rows of ``centroids`` (``np.unique(data.sensitive_feat, axis=0)`` of the
    whole dataset; the column ``sen_belong`` selects, :112-115) as int32 (B,),
    and a 0-d bool that is set when some row matches no centroid (its id is
    then 0, so that nothing indexes out of range).  Fixed-size compares, no
    host sync; works on CPU tensors too."""
    B, G = sensitive_feat.shape[0], centroids.shape[0]
    if G < 1:
        raise ValueError("centroid_ids needs at least one centroid")
    belong = (sensitive_feat.reshape(B, 1, -1) == centroids.reshape(1, G, -1)).all(-1)  # (B, G)
    gid = belong.to(torch.uint8).argmax(1).to(torch.int32)  # the first match; 0 when none
    return gid, ~belong.any(1).all()


def _centroid_groups(sensitive_feat, centroids, layout=True):
    """``(gid, unmatched, order, goff)``: ``centroid_ids`` and the group layout
    of its ids over the centroids' G groups (None, None without ``layout``)."""
    gid, unmatched = centroid_ids(sensitive_feat, centroids)
    order, goff = _group_layout(gid, centroids.shape[0]) if layout else (None, None)
    return gid, unmatched, order, goff


CALIB_MIN_SLICE = 8    # rows a slice should hold before a group is cut further
CALIB_MAX_SLICES = 64


def calib_slices(B, L, G, device):
    """R, the row slices per group of csrc/calib.hip's grid: enough workgroups
    (256 labels x group x slice) for two per compute unit, while a slice of an
    evenly filled group keeps CALIB_MIN_SLICE rows.  Host knowledge only."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    blocks = ((L + 255) // 256) * G
    want = (2 * cus + blocks - 1) // blocks
    return max(1, min(want, B // (G * CALIB_MIN_SLICE), CALIB_MAX_SLICES))


def _calib_fwd(p, x, y, w, order, goff, G, R, learn_logit, want_cal):
    """mpv_calib_fwd on contiguous device tensors -> (out (3,) fp64, cal_prob,
    and what the backward needs)."""
    B, L = p.shape
    T = 0 if w is None else w.shape[0]
    lib = H.load_library()
    nbytes = lib.mpv_calib_workspace_bytes(L, T, G, R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty(3, dtype=torch.float64, device=p.device)
    cal = torch.empty_like(p) if want_cal else None
    a = H.CalibArgs(H.ptr(p), H.ptr(x), H.ptr(y), H.ptr(w), H.ptr(order), H.ptr(goff), B, L, T, G,
                    R, int(bool(learn_logit)), H.ptr(cal), H.ptr(out))
    H.check(lib.mpv_calib_fwd(ctypes.byref(a), H.ptr(ws), nbytes, H.stream_of(p.device)),
            "mpv_calib_fwd")
    return out, cal, (a, ws, nbytes)


class _Calibration(torch.autograd.Function):
    @staticmethod
    def forward(ctx, indiv_prob, threshold_, y, w, order, goff, G, R, learn_logit):
        p = indiv_prob.detach().contiguous().float()
        x = threshold_.detach().contiguous().float()
        out, cal, state = _calib_fwd(p, x, y, w, order, goff, G, R, learn_logit, True)
        ctx.keep = (p, x, y, w, order, goff) + state
        ctx.meta = (indiv_prob.dtype, threshold_.dtype, threshold_.shape)
        nterms = out[2]
        ctx.mark_non_differentiable(cal, nterms)
        return out[0], out[1], cal, nterms

    @staticmethod
    def backward(ctx, g_bce, g_fair, _g_cal, _g_n):
        p, x, y, w, order, goff, a, ws, nbytes = ctx.keep
        zero = torch.zeros((), dtype=torch.float64, device=p.device)
        gout = torch.stack([zero if g is None else g.detach().to(torch.float64)
                            for g in (g_bce, g_fair)])
        gx = torch.empty_like(x)
        gp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        lib = H.load_library()
        H.check(lib.mpv_calib_bwd(ctypes.byref(a), H.ptr(gout), H.ptr(gx), H.ptr(gp), H.ptr(ws),
                                  nbytes, H.stream_of(p.device)), "mpv_calib_bwd")
        pdt, xdt, xshape = ctx.meta
        return (None if gp is None else gp.to(pdt), gx.to(xdt).reshape(xshape)) + (None,) * 7


class _ZeroCalibration(torch.autograd.Function):
    """An empty batch: zero losses that are still differentiable functions of
    both inputs, with zero gradients, and no launch (``_ZeroPenalty``'s
    precedent)."""

    @staticmethod
    def forward(ctx, indiv_prob, threshold_):
        ctx.save_for_backward(indiv_prob, threshold_)
        z = torch.zeros((), dtype=torch.float64, device=indiv_prob.device)
        return z, z.clone()

    @staticmethod
    def backward(ctx, g_bce, g_fair):
        return tuple(torch.zeros_like(t) for t in ctx.saved_tensors)


def _check_threshold(threshold_, L, G):
    if threshold_.numel() != L * G or tuple(threshold_.shape[-2:]) != (L, G):
        raise ValueError(f"threshold of shape {tuple(threshold_.shape)} is not (1, {L}, {G}) "
                         "(label_dim, number of centroids)")


def calibration_loss(indiv_prob, threshold_, input_label, sensitive_feat, centroids, tables,
                     learn_logit, slices=None):
    """fairsoft_train_postprocess.py:112-165 on the device.

    indiv_prob     -- (B, L) compute_loss output 7
    threshold_     -- (1, L, G) the learned thresholds (logits when ``learn_logit``)
    input_label    -- (B, L) batch labels
    sensitive_feat -- (B, n_sensitive) of the batch
    centroids      -- (G, n_sensitive) ``np.unique(data.sensitive_feat, axis=0)``
    tables         -- [LabelDistanceTable(label_distances[t], L, dev) for t in
                      target_fair_labels]; ``[]``: the BCE alone
    slices         -- row slices per group of the kernels' grid (default:
                      ``calib_slices``); the results agree to fp64 rounding
    Returns ``(bce, fair, cal_prob, active, contributed)``: ``bce`` (fp32) and
    ``fair`` (the tables' reference dtype; not yet times ``fair_coeff``) are
    differentiable 0-d tensors of ``threshold_`` and, where it requires a
    gradient, ``indiv_prob``; ``cal_prob`` (B, L) fp32 carries no gradient (the
    reference reads it for metrics only); ``active`` is a 0-d bool, set when at
    least one (target, group) term was added (the reference's ``not
    isinstance(fair_loss, float)``, :163: only then is the total ``fair *
    fair_coeff + bce``); ``contributed`` is the int32 count the reference adds
    to contributed_reg_fair_sample.  A row that matches no centroid makes both
    losses NaN.  No host sync: forward and backward can be captured in a HIP
    graph."""
    H.require_gpu(indiv_prob, threshold_, input_label, sensitive_feat, centroids)
    B, L = indiv_prob.shape
    G = centroids.shape[0]
    _check_threshold(threshold_, L, G)
    dev = indiv_prob.device
    fdt = torch.float32 if tables and all(t.ref_dtype == torch.float32 for t in tables) \
        else torch.float64
    if B == 0:  # shapes are host knowledge: no sync, still capturable
        bce, fair = _ZeroCalibration.apply(indiv_prob, threshold_)
        return (bce.float(), fair.to(fdt), torch.empty_like(indiv_prob, dtype=torch.float32),
                torch.zeros((), dtype=torch.bool, device=dev),
                torch.zeros((), dtype=torch.int32, device=dev))
    y = input_label.detach().contiguous().float()
    if tables:
        w, count = label_weights(y, tables)
    else:
        w, count = None, torch.zeros((), dtype=torch.int32, device=dev)
    _, unmatched, order, goff = _centroid_groups(sensitive_feat, centroids)
    R = calib_slices(B, L, G, dev) if slices is None else int(slices)
    bce, fair, cal_prob, nterms = _Calibration.apply(indiv_prob, threshold_, y, w, order, goff, G,
                                                     R, learn_logit)
    nan = torch.full_like(bce, float("nan"))
    bce = torch.where(unmatched, nan, bce).float()
    fair = torch.where(unmatched, nan, fair).to(fdt)
    return bce, fair, cal_prob, nterms > 0, count


def calibrate(indiv_prob, threshold, sensitive_feat, centroids, slices=None):
    """``calibrate_p(indiv_prob.unsqueeze(-1), threshold).transpose(1, 2)[sen_belong]``
    (:379-381): (B, L) fp32 calibrated probabilities, each row with the
    thresholds of its own group.  ``threshold`` (1, L, G) holds probabilities:
    no sigmoid is applied (the evaluation's caller has applied it when the
    thresholds were learned as logits).  A row that matches no centroid comes
    back NaN.  Forward only, no host sync."""
    H.require_gpu(indiv_prob, threshold, sensitive_feat, centroids)
    p = indiv_prob.detach().contiguous().float()
    B, L = p.shape
    G = centroids.shape[0]
    _check_threshold(threshold, L, G)
    if B == 0:
        return torch.empty_like(p)
    _, _, order, goff = _centroid_groups(sensitive_feat, centroids)
    R = calib_slices(B, L, G, p.device) if slices is None else int(slices)
    x = threshold.detach().contiguous().float()
    _, cal, _ = _calib_fwd(p, x, None, None, order, goff, G, R, False, True)
    rows = (sensitive_feat.reshape(B, 1, -1) == centroids.reshape(1, G, -1)).all(-1).any(1)
    return torch.where(rows[:, None], cal, torch.full_like(cal, float("nan")))


def fair_mean_diff(cal_prob, labels, sensitive_feat, centroids, tables, slices=None):
    """``best_val_metrics['fair_mean_diff']`` of evaluate_fair_through_postprocess
    (:413-446) over a whole split: the mean over the active (target, group)
    terms of the squared distance between the group's and the split's weighted
    mean of ``cal_prob``; a 0-d fp64 device tensor, NaN when no term is active
    (the reference's ``np.mean([])``) or a row matches no centroid.  No host
    sync."""
    H.require_gpu(cal_prob, labels, sensitive_feat, centroids)
    q = cal_prob.detach().contiguous().float()
    B, L = q.shape
    nan = torch.full((), float("nan"), dtype=torch.float64, device=q.device)
    if B == 0 or not tables:
        return nan
    w, _ = label_weights(labels, tables)
    G = centroids.shape[0]
    _, unmatched, order, goff = _centroid_groups(sensitive_feat, centroids)
    R = calib_slices(B, L, G, q.device) if slices is None else int(slices)
    out, _, _ = _calib_fwd(q, None, None, w, order, goff, G, R, False, False)
    return torch.where(unmatched | (out[2] == 0), nan, out[1] / out[2])


# ------------------------------------------------------ evaluation over a split
# fairsoft_evaluate.evaluate_mpvae's scoring (:83-121) on the device
# (csrc/evalsplit.hip): the "soft" micro / macro F1 of the raw probabilities
# and the mean Euclidean distance between the group and split weighted means.
# Differences from the reference, none of them numeric beyond rounding:
# * fp64 sums of the fp32 probabilities, where evals.compute_tp_fp_fn sums in
#   fp32 and rounds tp / fp / fn to fp32 once more;
# * the groups are the dataset's centroids, not ``np.unique`` of the split's
#   own sensitive rows: the same partition, since a centroid with no row in
#   the split adds nothing;
# * a row whose sensitive pattern is no centroid makes the fairness fields NaN;
# * the row weights are looked up in ``weight_labels`` (default: the split's
#   own labels).  The reference looks them up in
#   ``data.labels[np.arange(len(subset_idx))]`` -- the dataset's FIRST N rows,
#   whatever rows the split holds (fairsoft_evaluate.py:94, :100); the two
#   agree only for a split that is those rows.  A caller who wants the
#   reference's number passes ``weight_labels=data.labels[:N]``.

SplitScores = collections.namedtuple(
    "SplitScores", ["miF1", "maF1", "fair_mean_diff", "fair_mean_sq", "fair_terms", "counts",
                    "gid"])

EVAL_MIN_STEPS = 4     # row steps a slice should hold before a group is cut further
EVAL_MAX_SLICES = 64


def eval_lanes(L):
    """Lanes along the labels in csrc/evalsplit.hip's grid (eval_lanes there)."""
    return 64 if L > 32 else 1 << max(0, int(L) - 1).bit_length()


def eval_slices(N, L, G, device):
    """R, the row slices per group of csrc/evalsplit.hip's grid: enough
    workgroups (label chunk x group x slice) for two per compute unit, while a
    slice of an evenly filled group keeps EVAL_MIN_STEPS steps of the 256 /
    lanes rows a workgroup reads at once.  Host knowledge only."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    lp = eval_lanes(L)
    blocks = ((L + lp - 1) // lp) * G
    want = (2 * cus + blocks - 1) // blocks
    return max(1, min(want, N // (G * EVAL_MIN_STEPS * (256 // lp)), EVAL_MAX_SLICES))


def _table_weights_host(labels, tables):
    """``label_weights`` on CPU tensors, in torch: (T, N) fp64.  A row that is
    not exact 0 / 1 after truncation gets 0, as in row_weights_kernel."""
    y = labels.detach().float().trunc()
    N, L = y.shape
    W = (L + 63) // 64
    bad = ~((y == 0) | (y == 1)).all(1)
    bits = torch.zeros((N, W * 64), dtype=torch.int64)
    bits[:, :L] = (y == 1).to(torch.int64)
    shifts = torch.arange(64, dtype=torch.int64)
    words = (bits.reshape(N, W, 64) << shifts).sum(-1)  # distinct bits: the sum is the OR
    w = torch.zeros((len(tables), N), dtype=torch.float64)
    for t, tab in enumerate(tables):
        if tab.L != L:
            raise ValueError(f"table built for label_dim {tab.L}, labels have {L}")
        if tab.nslots == 0:
            continue
        keys, vals, used = tab.keys.cpu(), tab.vals.cpu(), tab.used.cpu().bool()
        for i0 in range(0, N, 1024):
            hit = (words[i0:i0 + 1024, None, :] == keys[None]).all(-1) & used[None]  # (n, slots)
            w[t, i0:i0 + 1024] = (hit.to(torch.float64) * vals[None]).sum(1)
    w[:, bad] = 0.0
    return w


def _weights_host(labels, sources):
    """``label_weights_batch`` on CPU tensors for a list that may mix tables
    and ``LabelSimilarity`` objects: (T, N) fp64."""
    _check_label_dim(sources, labels.shape[1])
    w = torch.zeros((len(sources), labels.shape[0]), dtype=torch.float64)
    for t0, t1, sim in _source_runs(sources):
        w[t0:t1] = (_sim_weights_host if sim else _table_weights_host)(labels, sources[t0:t1])
    return w


def _split_scores_host(p, y, w, gid, G):
    """The formulas of mpv_split_eval in fp64 torch ops, for CPU tensors:
    ``(counts (3, L), out (5,), terms (T, G) or None)``."""
    p, y = p.double(), y.double()
    counts = torch.stack([(y * p).sum(0), ((y == 0).double() * p).sum(0),
                          (y * (p == 0).double()).sum(0)])
    tp, fp, fn = counts
    mi = 2 * tp.sum() / (2 * tp.sum() + fp.sum() + fn.sum())
    f1 = 2 * tp / (2 * tp + fp + fn + 1e-6)
    keep = torch.isfinite(f1)
    ma = torch.where(keep, f1, torch.zeros_like(f1)).sum() / keep.sum()
    nan = torch.full((), float("nan"), dtype=torch.float64)
    if w is None:
        return counts, torch.stack([mi, ma, nan, nan, torch.zeros((), dtype=torch.float64)]), None
    onehot = (gid.long()[:, None] == torch.arange(G)[None]).double()  # (N, G)
    Wtk = w @ onehot                                                 # (T, G)
    S = torch.einsum("tn,ng,nl->tgl", w, onehot, p)
    Wt = Wtk.sum(1)
    m_t = S.sum(1) / Wt[:, None]
    terms = ((S / Wtk[..., None] - m_t[:, None, :]) ** 2).sum(-1)
    active = (Wt > 0)[:, None] & (Wtk > 0)
    terms = torch.where(active, terms, nan)
    n = active.sum().double()
    zero = torch.zeros_like(terms)
    dist = torch.where(active, terms.sqrt(), zero).sum() / n
    sq = torch.where(active, terms, zero).sum() / n
    return counts, torch.stack([mi, ma, dist, sq, n]), terms


def _split_eval(p, y, w, order, goff, G, R, D=None):
    """mpv_split_eval on contiguous device tensors, or with ``D`` definitions
    (``w`` then holds their D T targets) mpv_split_eval_defs.  Without ``D``
    -> ``(counts, out (5,), terms)``, terms (T, G), None when T = 0; with ``D``
    -> ``(counts, out, terms, out_defs)``, terms (D, T, G), out_defs (D, 3)."""
    N, L = p.shape
    TT = 0 if w is None else w.shape[0]  # targets in all
    lib, st = H.load_library(), H.stream_of(p.device)
    nbytes = lib.mpv_split_eval_workspace_bytes(N, L, TT, G, R)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=p.device)
    counts = torch.empty((3, L), dtype=torch.float64, device=p.device)
    out = torch.empty(5, dtype=torch.float64, device=p.device)
    T = TT if D is None else TT // max(D, 1)
    terms = torch.empty((T, G) if D is None else (D, T, G), dtype=torch.float64, device=p.device)
    a = H.SplitEvalArgs(H.ptr(p), H.ptr(y), H.ptr(w), H.ptr(order), H.ptr(goff), N, L, T, G, R,
                        H.ptr(counts), H.ptr(terms) if TT else None, H.ptr(out))
    if D is None:
        H.check(lib.mpv_split_eval(ctypes.byref(a), H.ptr(ws), nbytes, st), "mpv_split_eval")
        return counts, out, terms if T else None
    out_defs = torch.empty((max(D, 1), 3), dtype=torch.float64, device=p.device)
    H.check(lib.mpv_split_eval_defs(ctypes.byref(a), D, H.ptr(out_defs), H.ptr(ws), nbytes, st),
            "mpv_split_eval_defs")
    return counts, out, terms, out_defs


def _split_scores(name, pred, labels, sensitive_feat, centroids, definitions, weight_labels,
                  slices):
    """The body of ``split_scores_defs`` (``name`` in the messages), and of
    ``split_scores`` through its one definition.  ``definitions`` None: no
    fairness at all, the fairness fields None."""
    fair = definitions is not None
    defs = [list(d) for d in definitions] if fair else []
    D = len(defs)
    T = len(defs[0]) if defs else 0
    if any(len(d) != T for d in defs):
        raise ValueError(f"{name} needs the same number of targets in every definition "
                         f"(got {[len(d) for d in defs]})")
    if fair and (sensitive_feat is None or centroids is None):
        raise ValueError(f"{name} needs sensitive_feat and centroids")
    dev = pred.device
    host = dev.type == "cpu"
    used = (pred, labels) + ((sensitive_feat, centroids, weight_labels) if fair else ())
    if host:
        if any(t is not None and t.device.type != "cpu" for t in used):
            raise RuntimeError(f"{name} inputs must all live on one device")
        if fair and D == 0:
            raise ValueError(f"{name} needs at least one definition")
    else:
        H.require_gpu(*used)
    p = pred.detach().contiguous().float()
    y = labels.detach().contiguous().float()
    N, L = p.shape
    if tuple(y.shape) != (N, L):
        raise ValueError(f"labels {tuple(y.shape)} do not match pred {(N, L)}")
    G = centroids.shape[0] if fair else 1
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    if N == 0:  # shapes are host knowledge: no launch with an empty grid
        counts = torch.zeros((3, L), dtype=torch.float64, device=dev)
        if not fair:
            return SplitScores(nan, nan.clone(), None, None, None, counts, None)
        return SplitScores(nan, nan.clone(), nan.expand(D).clone(), nan.expand(D).clone(),
                           torch.full((D, T, G), float("nan"), dtype=torch.float64, device=dev),
                           counts, torch.zeros(0, dtype=torch.int32, device=dev))
    if not fair:
        if host:
            counts, out, _ = _split_scores_host(p, y, None, None, G)
        else:
            R = eval_slices(N, L, G, dev) if slices is None else int(slices)
            counts, out, _ = _split_eval(p, y, None, None, None, G, R)
        return SplitScores(out[0], out[1], None, None, None, counts, None)
    gid, unmatched, order, goff = _centroid_groups(sensitive_feat, centroids, layout=not host)
    wl = y if weight_labels is None else weight_labels.detach().contiguous().float()
    if tuple(wl.shape) != (N, L):
        raise ValueError(f"weight_labels {tuple(wl.shape)} do not match pred {(N, L)}")
    flat = [s for d in defs for s in d]
    if host:
        w = _weights_host(wl, flat).reshape(D, T, N) if T else None
        per = [_split_scores_host(p, y, None if w is None else w[d], gid, G) for d in range(D)]
        counts, out = per[0][0], per[0][1]
        out_defs = torch.stack([o[2:5] for _, o, _ in per])
        terms = torch.stack([t for _, _, t in per]) if T else torch.empty((D, 0, G),
                                                                          dtype=torch.float64)
    else:
        w = label_weights_batch(wl, flat)[0] if flat else None
        R = eval_slices(N, L, G, dev) if slices is None else int(slices)
        counts, out, terms, out_defs = _split_eval(p, y, w, order, goff, G, R, D)
    return SplitScores(out[0], out[1], torch.where(unmatched, nan, out_defs[:, 0]),
                       torch.where(unmatched, nan, out_defs[:, 1]),
                       torch.where(unmatched, torch.full_like(terms, float("nan")), terms),
                       counts, gid)


def split_scores(pred, labels, sensitive_feat=None, centroids=None, tables=None,
                 weight_labels=None, slices=None):
    """The scoring of fairsoft_evaluate.evaluate_mpvae (:83-121) over a whole
    split, from device tensors, with no host sync (capturable in a HIP graph).

    pred           -- (N, L) indiv_prob of every row of the split
    labels         -- (N, L) the split's labels, exact 0 / 1
    sensitive_feat -- (N, n_sensitive) of the split's rows   } needed with
    centroids      -- (G, n_sensitive) ``np.unique(data.sensitive_feat, axis=0)``  } ``tables``
    tables         -- [LabelDistanceTable(label_distances[t], L, dev) for t in
                      target_fair_labels]; None: the reference's
                      ``eval_fairness=False`` (no grouping, the fairness fields
                      None); ``[]``: no target, the fairness scalars NaN
    weight_labels  -- (N, L) the labels the row weights are looked up by
                      (default: ``labels``).  The reference reads
                      ``data.labels[np.arange(len(subset_idx))]``, the dataset's
                      first N rows and not the split's (:94, :100): pass those
                      rows for the reference's number
    slices         -- row slices per group of the kernel's grid (default:
                      ``eval_slices``); the results agree to fp64 rounding
    Returns a ``SplitScores``: ``miF1``, ``maF1`` (the "soft" F1 of the raw
    probabilities, evals.py:61-109), ``fair_mean_diff`` (the mean over the
    active (target, group) terms of the Euclidean distance between the group's
    and the split's weighted mean of ``pred``, :106-121) and ``fair_mean_sq``
    (the mean of the squared distances, what ``fair_mean_diff`` of this module
    gives) as 0-d fp64 tensors on ``pred``'s device, ``fair_terms`` (T, G) the
    squared distances (NaN where inactive), ``counts`` (3, L) tp / fp / fn and
    ``gid`` (N,) the rows' group ids.  No active term gives NaN (the
    reference's ``np.mean([])``), and so does a row that matches no centroid.
    N = 0 returns NaN scores without a launch.

    CUDA tensors run mpv_split_eval, with ``tables`` mpv_split_eval_defs on
    the one definition (csrc/evalsplit.hip).  CPU tensors run the
    same formulas in fp64 torch ops (the reference evaluates small
    configurations on the CPU; ``mpvae_step.EvalPass`` then runs the model
    through libmpvae_host.so): dispatch by device, never a fallback."""
    sc = _split_scores("split_scores", pred, labels, sensitive_feat, centroids,
                       None if tables is None else [tables], weight_labels, slices)
    if tables is None:
        return sc
    return sc._replace(fair_mean_diff=sc.fair_mean_diff[0], fair_mean_sq=sc.fair_mean_sq[0],
                       fair_terms=sc.fair_terms[0])


def split_scores_defs(pred, labels, sensitive_feat, centroids, definitions, weight_labels=None,
                      slices=None):
    """``split_scores`` under D definitions of the row weights from one pass
    over the split: what fairsoft_metric.evaluate_models_over_label_distances
    gets from one full ``evaluate_mpvae`` per distance definition, although
    ``indiv_prob`` does not depend on the definition.

    definitions -- a list of D lists of T weight sources each (``LabelSimilarity``
                   or ``LabelDistanceTable``, as ``split_scores``' ``tables``);
                   all D lists have the same T, else ValueError
    The other arguments are ``split_scores``'.  Returns a ``SplitScores`` whose
    ``fair_mean_diff`` and ``fair_mean_sq`` are (D,) and whose ``fair_terms``
    is (D, T, G); ``miF1``, ``maF1``, ``counts`` and ``gid`` do not depend on
    the definitions.  Every definition's numbers are, bit for bit, what
    ``split_scores`` gives for that definition alone (same ``slices``): one
    weights call on the D T sources, then one mpv_split_eval_defs.  A
    definition with no active term holds NaN.  No host sync.  CPU tensors run
    ``split_scores``' torch formulas per definition."""
    return _split_scores("split_scores_defs", pred, labels, sensitive_feat, centroids,
                         list(definitions), weight_labels, slices)
