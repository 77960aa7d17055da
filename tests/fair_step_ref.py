"""References for the fused fairness path and FairTrainStep -- TEST
INFRASTRUCTURE ONLY (the checkers of mpv_group_rows and of the fair step).

groups_ref   numpy: what ``mpvae_fair.sensitive_groups`` / ``group_rows``
             return, from explicit row comparisons (no np.unique);
             tests/test_fair_step_ref.py pins it against
             ``np.unique(x, axis=0, return_inverse=True)``.
penalty_ref  torch, differentiable: fairsoft_train.py:75-134 restated line by
             line -- ``torch.unique``, the per-row dict lookup on the label
             string, the ``weights.sum() > 0`` gates; pinned there against the
             vectors recorded from the reference (tests/golden/fair_f*.npz).
"""
import functools

import numpy as np
import torch


def _row_cmp(a, b):
    for u, v in zip(a, b):
        if u != v:  # by value: -0.0 == +0.0
            return -1 if u < v else 1
    return 0


def groups_ref(x, max_groups=None):
    """(gid, order, goff, G, overflow) as numpy int32 arrays / int / bool:
    gid[b] = min(number of distinct rows sorting before row b, G - 1), order
    the stable argsort of gid, goff[k] the number of rows with gid < k."""
    x = np.asarray(x)
    B = x.shape[0]
    x = x.reshape(B, -1)
    G = int(max_groups) if max_groups is not None else max(B, 1)
    distinct = []
    for row in x:
        if not any(_row_cmp(row, d) == 0 for d in distinct):
            distinct.append(row)
    distinct.sort(key=functools.cmp_to_key(_row_cmp))
    r = np.array([next(i for i, d in enumerate(distinct) if _row_cmp(row, d) == 0) for row in x],
                 np.int64).reshape(B)
    overflow = bool((r >= G).any())
    gid = np.minimum(r, G - 1).astype(np.int32)
    order = np.argsort(gid, kind="stable").astype(np.int32)
    goff = np.array([(gid < k).sum() for k in range(G + 1)], np.int32)
    return gid, order, goff, G, overflow


def penalty_ref(label_z, feat_z, labels, sensitive_feat, dists, norm, fair_coeff):
    """fairsoft_train.py:75-134.  label_z, feat_z: (B, L) torch tensors (may
    require grad); labels: (B, L) numpy (``data.labels[idx]``); sensitive_feat:
    (B, n) torch tensor; dists: ``[label_distances[t] for t in
    target_fair_labels]``.  Returns ``(fairloss, contributed)``; fairloss is the
    Python float 0. when no term is active, as in the reference."""
    sensitive_centroids = torch.unique(sensitive_feat, dim=0)                    # :81
    idx_tensor = torch.arange(sensitive_feat.shape[0], device=sensitive_feat.device)
    reg_label_z_unfair = 0.
    reg_feat_z_unfair = 0.
    contributed = 0
    for target_label_dist in dists:                                              # :87-88
        weights = []
        for label in labels:                                                     # :90-96
            label = label.astype(int)
            distance = target_label_dist.get(''.join(label.astype(str)), 0.)
            weights.append(distance)
            if distance > 0:
                contributed += 1
        weights = torch.tensor(weights).to(label_z.device).reshape(-1, 1)        # :97-98
        if weights.sum() > 0:                                                    # :100
            label_z_weighted = torch.sum(label_z * weights, axis=0) / weights.sum()
            feat_z_weighted = torch.sum(feat_z * weights, axis=0) / weights.sum()
            for sensitive in sensitive_centroids:                                # :106
                target_sensitive = torch.all(torch.eq(sensitive_feat, sensitive), dim=1)
                label_z_sensitive = label_z[idx_tensor[target_sensitive]]
                feat_z_sensitive = feat_z[idx_tensor[target_sensitive]]
                weight_sensitive = weights[idx_tensor[target_sensitive]]
                if weight_sensitive.sum() > 0:                                   # :113
                    reg_label_z_sen = torch.sum(
                        label_z_sensitive * weight_sensitive, 0) / weight_sensitive.sum()
                    reg_feat_z_sen = torch.sum(
                        feat_z_sensitive * weight_sensitive, 0) / weight_sensitive.sum()
                    if norm == 'l1':                                             # :114-122
                        reg_label_z_unfair += torch.sum(
                            torch.absolute(reg_label_z_sen - label_z_weighted))
                        reg_feat_z_unfair += torch.sum(
                            torch.absolute(reg_feat_z_sen - feat_z_weighted))
                    elif norm == 'l2':                                           # :123-131
                        reg_label_z_unfair += torch.sum(
                            torch.pow(reg_label_z_sen - label_z_weighted, 2))
                        reg_feat_z_unfair += torch.sum(
                            torch.pow(reg_feat_z_sen - feat_z_weighted, 2))
    fairloss = fair_coeff * (reg_label_z_unfair + reg_feat_z_unfair)             # :133-134
    return fairloss, contributed
