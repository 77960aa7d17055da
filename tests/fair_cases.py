"""Seeded case builders for the edge tests of csrc/fairness.hip and the host
side of mpvae_fair.py (tests/test_gpu_fair_edges.py on the device,
tests/test_fair_host.py on the CPU).  Everything here is numpy / torch on the
CPU: a case is a plain dict of arrays, the yardstick is oracle/fairness.py.
Every case is tiny (a few thousand elements at most)."""
import itertools

import numpy as np
import torch

# ------------------------------------------------------------ label weights
LW_L = [1, 5, 63, 64, 65, 128, 129, 4095, 4096]
LW_B = [1, 3, 4, 5, 9]
# the seeds of all_patterns_case: chosen so that the built table has a key off
# its home slot and a probe chain that steps from slot nslots-1 to slot 0
# (tests/test_fair_host.py asserts both on the table; they are conditions on
# the input, not measurements)
ALL_PATTERN_SEEDS = {3: 1, 5: 1}


def key_of(row):
    """The reference's dict key of one label row (fairsoft_train.py:91-93)."""
    return "".join(np.asarray(row).astype(int).astype(str))


def flip_indices(L):
    """The label positions where a one-label difference is easiest to lose:
    the first and last bit of a 64-bit word, the last label, and the first
    label of the last word -- whichever exist for this L."""
    W = (L + 63) // 64
    out = []
    for i in (0, 63, 64, L - 1, 64 * (W - 1)):
        if 0 <= i < L and i not in out:
            out.append(i)
    return out


def weight_pair_case(L, B, seed=0):
    """B rows built in pairs: row 2i is a key of the dict, row 2i+1 differs from
    it in exactly one label (flip_indices, rotated by B so that the B values
    together reach every index).  An odd last row is a key.  The dict also
    holds three patterns that are in no row."""
    rng = np.random.default_rng([seed, L, B])
    labels = np.zeros((B, L), np.int64)
    flips = flip_indices(L)
    dist = {}
    for b in range(0, B, 2):
        labels[b] = rng.integers(0, 2, L)
        dist[key_of(labels[b])] = np.float64(rng.uniform(0.05, 1.0))
        if b + 1 < B:
            labels[b + 1] = labels[b]
            labels[b + 1, flips[(b // 2 + B) % len(flips)]] ^= 1
    for _ in range(3):
        dist.setdefault(key_of(rng.integers(0, 2, L)), np.float64(rng.uniform(0.05, 1.0)))
    return dict(labels=labels, dists=[dist])


def all_patterns_case(L, seed=None):
    """Every one of the 2^L label patterns as a row, against a dict that holds
    a seeded half of them."""
    seed = ALL_PATTERN_SEEDS[L] if seed is None else seed
    rng = np.random.default_rng([seed, L])
    labels = np.array(list(itertools.product((0, 1), repeat=L)), np.int64)
    half = rng.permutation(len(labels))[:len(labels) // 2]
    dist = {key_of(labels[i]): np.float64(rng.uniform(0.05, 1.0)) for i in half}
    return dict(labels=labels, dists=[dist])


def probe_slots(tab, words):
    """The slots that a lookup of ``words`` visits in the table, in order, by
    the rule of label_weights_kernel: from the home slot, stop at an empty
    slot or at the key (host copy of the table's arrays)."""
    keys = tab.keys.cpu().numpy().view(np.uint64)
    used = tab.used.cpu().numpy()
    if tab.nslots == 0:
        return []
    import mpvae_fair as mf
    slot = mf.pattern_hash(words) & (tab.nslots - 1)
    seen = []
    for _ in range(tab.nslots):
        seen.append(int(slot))
        if not used[slot] or list(keys[slot]) == words:
            break
        slot = (slot + 1) & (tab.nslots - 1)
    return seen


# -------------------------------------------------------- fairness penalty
FP_L = [1, 255, 256, 257, 513]
FP_B = [1, 2, 7, 33]
FP_T = [1, 3]
FP_GROUPS = [1, 2, "all"]
FP_MAXG = [None, "exact", "plus3"]
FP_NORMS = ["l1", "l2"]


def penalty_lattice():
    """The 5 x 4 x 2 x 3 x 3 lattice pruned to 20 points per norm: every value
    of every axis occurs with both norms (tests/test_fair_host.py checks)."""
    out = []
    for norm in FP_NORMS:
        for i in range(20):
            out.append(dict(L=FP_L[i % 5], B=FP_B[i % 4], T=FP_T[(i // 4) % 2],
                            groups=FP_GROUPS[i % 3], maxg=FP_MAXG[(i // 3) % 3], norm=norm,
                            seed=i))
    return out


def lattice_id(c):
    return f"{c['norm']}-L{c['L']}-B{c['B']}-T{c['T']}-g{c['groups']}-mg{c['maxg']}"


def sensitive_for(rng, B, groups):
    """(B, 2) sensitive features with one group, two groups (both present when
    B >= 2), or every row its own group; the rows shuffled."""
    if groups == 1:
        s = np.full((B, 2), 3, np.int64)
    elif groups == 2:
        s = np.stack([np.arange(B) % 2, np.ones(B, np.int64)], 1)
    else:
        s = np.stack([np.arange(B) // 3, np.arange(B) % 3 - 1], 1)
    return s[rng.permutation(B)].astype(np.int64)


def n_groups(sensitive):
    return len(np.unique(np.asarray(sensitive), axis=0))


def max_groups_of(mode, sensitive):
    return {None: None, "exact": n_groups(sensitive), "plus3": n_groups(sensitive) + 3}[mode]


def penalty_case(L, B, T, groups, norm, maxg=None, seed=0, keep=0.7, pyfloat=False, coeff=0.75):
    """One fairness-penalty case: label rows with density 0.3 (the second half
    repeats the first, as a training batch repeats patterns), T dicts that
    each hold row 0's pattern and every other row pattern with probability
    ``keep`` (1 when B <= 2, so that a two-row batch keeps both groups alive),
    np.float64 values unless ``pyfloat``."""
    rng = np.random.default_rng([seed, L, B, T])
    labels = (rng.random((B, L)) < 0.3).astype(np.int64)
    labels[B - B // 2:] = labels[:B // 2]
    sens = sensitive_for(rng, B, groups)
    if B <= 2:
        keep = 1.0
    patterns = list(dict.fromkeys(key_of(r) for r in labels))
    dists = []
    for _ in range(T):
        d = {}
        for i, k in enumerate(patterns):
            if i == 0 or rng.random() < keep:
                v = rng.uniform(0.05, 1.0)
                d[k] = float(np.float32(v)) if pyfloat else np.float64(v)
        dists.append(d)
    return dict(labels=labels, sensitive=sens, dists=dists, norm=norm, coeff=coeff,
                max_groups=max_groups_of(maxg, sens),
                label_z=rng.uniform(0.01, 0.99, (B, L)).astype(np.float32),
                feat_z=rng.uniform(0.01, 0.99, (B, L)).astype(np.float32))


def dead_target_group_case(norm, seed=0):
    """L = 257, B = 24, T = 3, three sensitive groups.  Target 1's dict holds
    no pattern of the batch (W_t = 0) beside two active targets; the rows of
    group 5 (the first 8) are in no dict (W_tk = 0) beside two active groups."""
    c = penalty_case(257, 24, 3, 2, norm, seed=seed, keep=1.0)
    rng = np.random.default_rng([seed, 99])
    c["labels"] = (rng.random((24, 257)) < 0.3).astype(np.int64)   # all rows distinct
    c["sensitive"][:8] = 5
    c["sensitive"][8:, 0] = np.arange(16) % 2
    c["sensitive"][8:, 1] = 1
    live = [key_of(r) for r in c["labels"][8:]]
    c["dists"] = [{k: np.float64(rng.uniform(0.05, 1.0)) for k in live},
                  {key_of(rng.integers(0, 2, 257)): np.float64(0.5) for _ in range(5)},
                  {k: np.float64(rng.uniform(0.05, 1.0)) for k in live[::3]}]
    return c


def wide_weights_case(norm, seed=0):
    """L = 257, B = 33, T = 2, two groups, all rows distinct.  The dict values
    of every third row are 1e-6 times the others (row weights over six orders
    of magnitude), and rows 5, 6 and 20 are in no dict (weight 0 in every
    target: their gradient must be exactly zero)."""
    c = penalty_case(257, 33, 2, 2, norm, seed=seed)
    rng = np.random.default_rng([seed, 77])
    c["labels"] = (rng.random((33, 257)) < 0.3).astype(np.int64)
    dists = []
    for _ in range(2):
        d = {}
        for b, row in enumerate(c["labels"]):
            if b in (5, 6, 20):
                continue
            v = rng.uniform(0.05, 1.0)
            d[key_of(row)] = np.float64(v * 1e-6 if b % 3 == 0 else v)
        dists.append(d)
    c["dists"] = dists
    return c


def exact_zero_case(norm, seed=0):
    """L = 257, B = 12, T = 2, two groups, every dict value 1.0 (the reference's
    indication distance), and every even column of label_z / feat_z constant
    over the batch.  There the weighted means are sums of n equal fp32 values
    divided by n: exact, so d is exactly 0 in every group while both groups
    are active -- sgn(0) = 0 must give a zero gradient (with one group alone
    a wrong sgn(0) cancels between the group term and the batch term).
    ``zero_cols`` marks those columns."""
    c = penalty_case(257, 12, 2, 2, norm, seed=seed)
    rng = np.random.default_rng([seed, 55])
    c["labels"] = (rng.random((12, 257)) < 0.3).astype(np.int64)
    keys = [key_of(r) for r in c["labels"]]
    c["dists"] = [{k: np.float64(1.0) for k in keys}, {k: np.float64(1.0) for k in keys[1::2][:5]}]
    c["sensitive"][:, 0] = np.arange(12) // 2 % 2
    c["sensitive"][:, 1] = 1
    c["zero_cols"] = np.arange(257) % 2 == 0
    for z in (c["label_z"], c["feat_z"]):
        z[:, c["zero_cols"]] = z[0, c["zero_cols"]]
    return c


def l1_condition(c, min_d):
    """The input condition of an l1 case with more than one group, on the
    oracle's per-label min |d|: >= 1e-9 away from sgn's jump, or exactly on it
    where the case was built to be (``zero_cols``)."""
    zero = c.get("zero_cols", np.zeros(len(min_d), bool))
    return bool((min_d[~zero] >= 1e-9).all() and (min_d[zero] == 0).all())


def permuted_rows(c, seed=12345):
    """The same case with its batch rows in a fixed permutation, and the
    permutation (to un-permute the per-row results)."""
    perm = np.random.default_rng(seed).permutation(c["labels"].shape[0])
    p = dict(c)
    for k in ("labels", "sensitive", "label_z", "feat_z"):
        p[k] = c[k][perm]
    return p, perm


def row_rel_err(g, ref):
    """max over the rows b of  max_l |g[b,l] - ref[b,l]| / max_l |ref[b,l]|;
    inf if a row whose reference is all zero is not exactly zero."""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    err, scale = np.abs(g - ref).max(1), np.abs(ref).max(1)
    if np.any(err[scale == 0] != 0):
        return float("inf")
    live = scale > 0
    return float((err[live] / scale[live]).max()) if live.any() else 0.0


# ------------------------------------------------------------ train metrics
MET_L = [1, 2, 3, 4, 5, 6, 255, 256, 257, 513]
MET_B = [1, 2, 5]
MET_THR = [0.5, 0.05, 0.95]


def metrics_case(L, B, seed=0):
    """Uniform scores, targets with density 0.3 and at least one true label
    (the reference itself fails on a batch with none)."""
    rng = np.random.default_rng([seed, L, B])
    t = (rng.random((B, L)) < 0.3).astype(np.float32)
    t[0, 0] = 1
    return rng.random((B, L)).astype(np.float32), t


def _low(rng, L):
    """Distinct scores below 0.4, so that the constructed winners stand out."""
    return (rng.permutation(L).astype(np.float32) + 1) * np.float32(0.4 / (L + 1))


def tie_all_equal(L=513):
    """All scores equal: the top 5 are the five largest indices.  Targets true
    at L-1, L-3, L-5 and at 0 and 2: p@1 = 1, p@3 = 2/3, p@5 = 3/5 only with
    that order."""
    p = np.full((1, L), 0.25, np.float32)
    t = np.zeros((1, L), np.float32)
    t[0, [L - 1, L - 3, L - 5, 0, 2]] = 1
    return p, t


TIE_PAIRS = [(0, 63), (63, 64), (0, 256), (255, 256), (0, 512)]


def tie_pairs(L=513):
    """One row per pair: the maximum tied at the two indices, the target true
    at the larger one only.  Ranks 3-5 go to untied runners-up with false
    targets, so p@1 = 1 exactly when the larger index wins."""
    rng = np.random.default_rng(21)
    p = np.stack([_low(rng, L) for _ in TIE_PAIRS])
    t = np.zeros_like(p)
    for b, (i, j) in enumerate(TIE_PAIRS):
        p[b, [i, j]] = 0.9
        t[b, j] = 1
        t[b, np.argsort(p[b])[:4]] = 1   # true labels far from the top
    return p, t


def five_on_one_thread(L=1285):
    """The five largest scores at 7 + 256 j (one thread owns all five when a
    thread owns l = tid mod 256), the sixth largest elsewhere.  Targets true at
    ranks 1, 3, 5 and 6: a missed winner pulls rank 6 in and moves p@k."""
    rng = np.random.default_rng(22)
    p, t = _low(rng, L)[None], np.zeros((1, L), np.float32)
    for j, v in enumerate((0.99, 0.98, 0.97, 0.96, 0.95)):
        p[0, 7 + 256 * j] = v
        t[0, 7 + 256 * j] = 1 - j % 2
    p[0, 600], t[0, 600] = 0.94, 1
    return p, t


def inf_scores(L=513):
    """-inf everywhere but +inf at 300 and finite scores at 17 and 400: the top
    5 are 300, 400, 17 and then the -inf tie, so 512 and 511."""
    p = np.full((1, L), -np.inf, np.float32)
    p[0, 300], p[0, 400], p[0, 17] = np.inf, 0.7, 0.3
    t = np.zeros((1, L), np.float32)
    t[0, [300, 17, 511, 3]] = 1
    return p, t


def all_neg_inf_l3():
    """L = 3, all scores -inf: ranks 1-3 are indices 2, 1, 0; ranks 4 and 5 do
    not exist."""
    return np.full((1, 3), -np.inf, np.float32), np.array([[1, 0, 1]], np.float32)


def at_threshold(thr, L=513, B=2):
    """Scores exactly equal to the fp32 threshold (they predict 1) at true
    labels, and one fp32 step below it (they predict 0) at other true labels."""
    rng = np.random.default_rng(23)
    p = rng.random((B, L)).astype(np.float32)
    t = (rng.random((B, L)) < 0.1).astype(np.float32)
    at = rng.permutation(L)
    p[:, at[:40]] = np.float32(thr)
    p[:, at[40:80]] = np.nextafter(np.float32(thr), np.float32(0))
    t[:, at[:80]] = 0
    t[:, at[:80:2]] = 1
    return p, t


def one_live_row(L=513, B=5):
    """Rows 0 .. B-2 have no true and no predicted label at thr 0.5: only the
    last row enters ebF1."""
    rng = np.random.default_rng(24)
    p = (rng.random((B, L)) * 0.4).astype(np.float32)
    t = np.zeros((B, L), np.float32)
    p[B - 1] = rng.random(L).astype(np.float32)
    t[B - 1] = (rng.random(L) < 0.3).astype(np.float32)
    t[B - 1, 0] = 1
    return p, t


def dead_label(L=6, B=2):
    """Label 2 is never true and never predicted: its maF1 term is 0 / 1e-6 = 0
    and stays in the mean."""
    p = np.array([[0.9, 0.2, 0.1, 0.8, 0.6, 0.3], [0.1, 0.7, 0.2, 0.9, 0.4, 0.6]], np.float32)
    t = np.array([[1, 0, 0, 1, 0, 1], [0, 1, 0, 1, 1, 0]], np.float32)
    return p[:B, :L], t[:B, :L]


# ---------------------------------------------------------------- groups
def group_inputs(n=200, seed=31):
    """n integer and n half-integer (B, C) inputs, B in 1..65, C in 1..3,
    values in -2..2, and one 1-D input of each kind."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(2 * n):
        B, C = int(rng.integers(1, 66)), int(rng.integers(1, 4))
        if i < n:
            out.append(torch.from_numpy(rng.integers(-2, 3, (B, C))))
        else:
            out.append(torch.from_numpy(rng.integers(-4, 5, (B, C)) / 2.0).float())
    out.append(torch.from_numpy(rng.integers(-2, 3, 40)))
    out.append(torch.from_numpy(rng.integers(-4, 5, 40) / 2.0).float())
    return out


def check_groups(mf, device, inputs=None):
    """group_ids / sensitive_groups on ``device`` against torch.unique(dim=0)
    on the CPU, for every input of group_inputs()."""
    for n, X in enumerate(group_inputs() if inputs is None else inputs):
        B = X.shape[0]
        uniq, inv = torch.unique(X, dim=0, return_inverse=True)
        gid = mf.group_ids(X.to(device))
        assert gid.dtype == torch.int32 and gid.device.type == torch.device(device).type
        assert torch.equal(gid.cpu().long(), inv), n
        nu = uniq.shape[0]
        for mg in (None, nu, nu + 3, nu - 1)[n % 2::2]:
            if mg == 0:
                continue
            g, order, goff, G, overflow = mf.sensitive_groups(X.to(device), mg)
            g, order, goff = g.cpu().long(), order.cpu().long(), goff.cpu().long()
            assert G == (B if mg is None else mg) and goff.numel() == G + 1
            assert bool(overflow) == (nu > G), (n, mg)
            assert torch.equal(g, inv.clamp(max=G - 1)), (n, mg)
            assert torch.equal(order.sort().values, torch.arange(B)), (n, mg)
            assert int(goff[0]) == 0 and int(goff[-1]) == B
            for k in range(G):
                rows = order[goff[k]:goff[k + 1]]
                assert bool((g[rows] == k).all()), (n, mg, k)
                assert bool((rows[1:] > rows[:-1]).all()), (n, mg, k)


def check_empty_groups(mf, device, shape=(0, 2)):
    """group_ids / sensitive_groups of a batch with no row: empty results."""
    X = torch.zeros(shape, device=device)
    gid = mf.group_ids(X)
    assert gid.shape == (0,) and gid.dtype == torch.int32 and gid.device == X.device
    for mg in (None, 4):
        g, order, goff, G, overflow = mf.sensitive_groups(X, mg)
        assert g.shape == (0,) and order.shape == (0,) and G == (1 if mg is None else 4)
        assert goff.shape == (G + 1,) and not goff.any() and not bool(overflow)
