"""GPU: the validation-metric kernels (csrc/curves.hip through
mpvae_fair.curve_metrics / compute_metrics) at the edges of their five stages:
both sign branches of the sort key, +-0, denormals and +-FLT_MAX; all-distinct
scores across the sort chunk (4096 keys), the merge tile and the pass tile
(1024 keys each); runs of equal scores longer than a pass tile; the FDR
predicate on equality; the aggregate's LDS sort from L = 1 to its capacity.

References: closed forms where there is one (the rank probe, the FDR
boundary), else the numpy restatement tests/curves_ref.py, which
tests/test_curves_ref.py pins to the reference at these edges (fixtures c6 and
c7); the aggregates also against numpy's nan-statistics of the device's own
per-label arrays.

Tolerances are those of tests/test_gpu_curves.py, whose derivation is:
  "AUC and AUPR lie in [0, 1] and are fp64 sums of at most N terms, so adding
  them in another order costs at most about N 2^-53: 1e-12 at N = 10^4; 1e-9
  absolute leaves three decades.  FDR is one fp64 division of the same
  integers: exact equality.  An aggregate of L values each within 1e-9 of the
  golden ones is within 1e-9 (mean, median) or 2e-9 (variance ...) of the
  golden aggregate"
The largest N here is 12289.  The variants of one input (``chunk``, +-0, the
input dtype) must give the same bits: the sorted keys are the same.

+-inf and NaN scores are in no assertion: the reference (scikit-learn's finite
check) refuses them, so there is nothing to be equal to, and the kernels' order
for them is no contract."""
import numpy as np
import pytest
import torch

import curves_ref as cr
import mpvae_fair as mf
import mpvae_hip as H
from test_gpu_curves import ALL, TOL, _check_arrays, _dev, _host

pytestmark = pytest.mark.gpu
FMAX = np.finfo(np.float32).max
FMIN = np.finfo(np.float32).tiny
DENORM = np.float32(2.0 ** -149)
STATS = [("mean", np.nanmean, TOL), ("median", np.nanmedian, TOL), ("var", np.nanvar, 2 * TOL)]


def _curves(p, t, chunk=0):
    return _host(mf.curve_metrics(_dev(p), _dev(t), chunk))


def _same_bits(a, b):
    for k in ALL + mf.CURVE_KEYS:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), k


def _check_restatement(got, p, t, want=None):
    """The per-label arrays as _check_arrays has them; the nine aggregates at
    TOL (mean, median) and 2 TOL (variance), NaN where the restatement's is."""
    want = want or cr.curve_metrics(p, t)
    _check_arrays(got, want)
    for name in ["AUC", "AUPR", "FDR"]:
        for stat, _, tol in STATS:
            g, w = float(got[stat + name]), want[stat + name]
            print(stat + name, g, w)
            assert np.isnan(g) if np.isnan(w) else abs(g - w) <= tol, (stat, name)
    return want


# ------------------------------------------------------------ 1. rank probe
RANK_N = [2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 12289]


@pytest.mark.parametrize("N", RANK_N)
def test_one_positive_at_a_known_rank(N):
    """N distinct scores on both sides of zero, each label's rows in an order
    of its own, one positive per label at descending rank r:
      AUC = (N-1-r)/(N-1), AUPR = 1 (r = 0) or 1/(2(r+1)), FDR = 1 (r <= 1) or 0.
    A key that the sort or a merge misplaces, drops or repeats moves r by at
    least 1, AUC by at least 1/(N-1) >= 8e-5.  12289 is three default
    segments: one run without a partner, then 8192 keys merged with 4097;
    chunk = 64 gives up to 13 output tiles per merged pair."""
    score = np.linspace(1, -1, N).astype(np.float32)  # descending: index = rank
    assert np.unique(score).size == N and score[0] > 0 > score[-1]
    ranks = sorted({r for r in [0, 1, 2, 63, 64, 1023, 1024, 4095, 4096, N - 2, N - 1]
                    if 0 <= r < N})
    L = len(ranks)
    rng = np.random.default_rng(N)
    p, t = np.empty((N, L), np.float32), np.zeros((N, L), np.float32)
    for l, r in enumerate(ranks):
        rows = rng.permutation(N)
        p[rows, l] = score
        t[rows[r], l] = 1
    r = np.array(ranks, np.float64)
    auc = (N - 1 - r) / (N - 1)
    aupr = np.where(r == 0, 1.0, 1.0 / (2 * (r + 1)))
    fdr = np.where(r <= 1, 1.0, 0.0)
    first = _curves(p, t, 0)
    for chunk in [0, 64] + ([1024] if N >= 1025 else []):
        got = first if chunk == 0 else _curves(p, t, chunk)
        print("chunk", chunk, "max |dAUC|", np.abs(got["allAUC"] - auc).max(),
              "max |dAUPR|", np.abs(got["allAUPR"] - aupr).max())
        assert np.all(np.abs(got["allAUC"] - auc) <= TOL), chunk
        assert np.all(np.abs(got["allAUPR"] - aupr) <= TOL), chunk
        assert np.array_equal(got["allFDR"], fdr), chunk
        _same_bits(got, first)


# ------------------------------------------------ 2. dense inputs, no ties
def _dense(N, L, seed):
    """Continuous scores over many binades, larger where the label is 1, half
    of them negated; redrawn until each column's fp32 values are distinct."""
    while True:
        rng = np.random.default_rng(seed)
        t = (rng.random((N, L)) < 0.3).astype(np.float32)
        p = np.exp(3 * rng.standard_normal((N, L)) + t)
        p = np.where(rng.random((N, L)) < 0.5, -p, p).astype(np.float32)
        if all(np.unique(p[:, l]).size == N for l in range(L)):
            return p, t
        seed += 1


@pytest.mark.parametrize("chunk", [0, 64])
@pytest.mark.parametrize("N", [1025, 4097, 8209])
def test_distinct_signed_scores_against_the_restatement(N, chunk):
    p, t = _dense(N, 3, 11 * N)
    assert np.isfinite(p).all() and (p < 0).any() and (p > 0).any()
    _check_restatement(_curves(p, t, chunk), p, t)


# ----------------------------------------- 3. runs longer than a pass tile
LONG_RUNS = {
    # three pass tiles of 1024 keys.  (a) one run: its end is key N-1, two
    # tiles without a run end before it; (b) an end inside tile 2, none in
    # tile 1; (c) an end on the last key of tile 1, then a run of one key;
    # (d) is (b) with one class; (e) an end in tile 1, none in tile 2: the
    # previous run end has to outlast a tile that has none, which (a)-(d)
    # never ask -- there every tile after the first end has one of its own
    2500: [[2500], [1100, 1400], [1024, 1, 1475], [1100, 1400], [300, 2200]],
    # six tiles: the previous run end outlasts four tiles and three; the
    # second from an end that is not in the first tile
    5123: [[7, 5116], [1030, 4093], [1500, 1, 3622], [1030, 4093]],
}


@pytest.mark.parametrize("N", sorted(LONG_RUNS))
def test_runs_longer_than_a_pass_tile(N):
    """Score levels with the run lengths of LONG_RUNS[N] in descending order,
    rows shuffled, against a target of density 0.3 (column 3: all zeros)."""
    runs = LONG_RUNS[N]
    L = len(runs)
    rng = np.random.default_rng(N)
    t = (rng.random((N, L)) < 0.3).astype(np.float32)
    t[:, 3] = 0
    p = np.empty((N, L), np.float32)
    for l, lengths in enumerate(runs):
        assert sum(lengths) == N
        level = np.repeat(0.75 - 0.5 * np.arange(len(lengths)), lengths)  # 0.75, 0.25, -0.25
        p[rng.permutation(N), l] = level
        assert [int((p[:, l] == v).sum()) for v in np.unique(level)[::-1]] == lengths
    got = _curves(p, t, 0)
    want = _check_restatement(got, p, t)
    assert list(np.flatnonzero(np.isnan(want["allAUC"]))) == [3]
    if len(runs[0]) == 1:
        assert abs(got["allAUC"][0] - 0.5) <= TOL  # one run: the chord
    _same_bits(_curves(p, t, 64), got)


# ------------------------------------------------------ 4. score-key edges
POOL = np.array([-FMAX, -1.5, -DENORM, -0.0, 0.0, DENORM, FMIN, 0.5, FMAX], np.float32)


def _pool_input():
    rng = np.random.default_rng(257)
    p = POOL[rng.integers(0, POOL.size, (257, 4))]
    t = (rng.random((257, 4)) < 0.3).astype(np.float32)
    return p, t


def test_signed_zero_denormal_and_largest_scores():
    p, t = _pool_input()
    for v in POOL:  # every pool value with both classes somewhere
        hit = (p.view(np.uint32) == v.view(np.uint32))
        assert hit.any() and (t[hit] == 1).any() and (t[hit] == 0).any(), v
    _check_restatement(_curves(p, t), p, t)


def test_minus_zero_is_plus_zero():
    p, t = _pool_input()
    q = p.copy()
    plus = q.view(np.uint32) == 0
    assert plus.sum() > 20 and (np.signbit(p) & (p == 0)).sum() > 20
    q[plus] = -0.0
    assert np.signbit(q[plus]).all() and np.array_equal(p, q)  # equal as numbers
    _same_bits(_curves(q, t), _curves(p, t))


def test_a_column_of_signed_zeros_is_one_run():
    N = 257
    rng = np.random.default_rng(258)
    p = np.zeros((N, 2), np.float32)
    p[::2, 0] = -0.0
    p[rng.random(N) < 0.5, 1] = -0.0
    t = (rng.random((N, 2)) < 0.3).astype(np.float32)
    assert all(np.signbit(p[:, l]).any() and not np.signbit(p[:, l]).all() for l in range(2))
    got = _curves(p, t)
    _check_restatement(got, p, t)
    assert np.all(np.abs(got["allAUC"] - 0.5) <= TOL)


# ------------------------------ 5. targets that are not 0/1; input dtypes
def test_only_a_target_of_one_is_positive():
    N = 130
    rng = np.random.default_rng(130)
    t = np.array([0, 1, 0.5, 2.0, -1.0], np.float32)[rng.integers(0, 5, (N, 3))]
    t[:, 2] = np.where(t[:, 2] == 1, 2.0, t[:, 2])  # no 1 at all: one class
    p = (rng.random((N, 3)) - 0.5 + 0.3 * (t == 1)).astype(np.float32)
    got = _curves(p, t)
    want = _check_restatement(got, p, t)
    assert np.isnan(want["allAUC"][2]) and not np.isnan(want["allAUC"][:2]).any()
    _same_bits(got, _curves(p, (t == 1).astype(np.float32)))


def test_fp64_scores_and_bool_or_int64_targets_are_cast_to_fp32():
    """The cast of the scores to fp32 comes first: rows 3 and 40 hold the two
    largest scores, distinct in fp64 and one fp32 value, so a positive and a
    negative are one threshold run."""
    N = 70
    rng = np.random.default_rng(70)
    t = rng.random((N, 3)) < 0.3
    p64 = rng.random((N, 3)) - 0.5
    p64[3], p64[40] = 0.625, 0.625 + 1e-12
    t[3], t[40] = True, False
    assert (p64[3] != p64[40]).all()
    assert (p64[3].astype(np.float32) == p64[40].astype(np.float32)).all()
    p32, t32 = p64.astype(np.float32), t.astype(np.float32)
    want = _curves(p32, t32)
    _check_restatement(want, p32, t32)
    # sorted as fp64 the negative would lead alone: another curve
    apart = p32.copy()
    apart[40] = np.nextafter(apart[40], np.float32(1))
    assert not np.array_equal(_curves(apart, t32)["allAUC"], want["allAUC"])
    for tt in (torch.from_numpy(t), torch.from_numpy(t.astype(np.int64))):
        got = _host(mf.curve_metrics(torch.from_numpy(p64).to("cuda:0"), tt.to("cuda:0")))
        _same_bits(got, want)
    full = _host(mf.compute_metrics(torch.from_numpy(p64).to("cuda:0"),
                                    torch.from_numpy(t).to("cuda:0"), 0.1, all_metrics=True))
    _same_bits(full, want)
    plain = _host(mf.compute_metrics(_dev(p32), _dev(t32), 0.1))
    for k in mf.METRIC_KEYS:
        assert np.array_equal(np.asarray(full[k]).view(np.int64),
                              np.asarray(plain[k]).view(np.int64)), k


# -------------------------------------------------- 6. FDR on the boundary
def _from_runs(cols, seed):
    """cols: per column a list of runs (length, positives), in descending
    score order.  -> shuffled (N, len(cols)) scores on both sides of zero and
    0/1 targets."""
    N = sum(n for n, _ in cols[0])
    rng = np.random.default_rng(seed)
    p, t = np.empty((N, len(cols)), np.float32), np.zeros((N, len(cols)), np.float32)
    for l, runs in enumerate(cols):
        assert sum(n for n, _ in runs) == N
        s, y = [], []
        for j, (n, pos) in enumerate(runs):
            s += [0.5 - 0.25 * j] * n
            y += [1] * pos + [0] * (n - pos)
        rows = rng.permutation(N)
        p[rows, l], t[rows, l] = s, y
    return p, t


FDR_CASES = {
    # run ends (i+1, tp): (1, 1) holds; (4, 2) is 2 tp = i+1; (6, 2) fails.  -> 2/2
    # beside it the middle run one key longer: (5, 2) fails.  -> (1, 1): 1/2
    6: ([[(1, 1), (3, 1), (2, 0)], [(1, 1), (4, 1), (1, 0)]], [1.0, 0.5]),
    # P = 512.  (10, 10) holds; (1020, 510) is 2 tp = i+1; (1026, 512) fails.  -> 510/512
    # beside it the middle run one key longer: (1021, 510) fails.  -> 10/512
    # third: the equality on the last key of the first pass tile, (1024, 512),
    # then two runs of one negative.  -> 512/512
    # fourth: the equality at the last key of all, (1026, 513), in the second
    # tile; (10, 10) held, (1020, 509) did not.  -> 513/513
    1026: ([[(10, 10), (1010, 500), (6, 2)], [(10, 10), (1011, 500), (5, 2)],
            [(10, 10), (1014, 502), (1, 0), (1, 0)], [(10, 10), (1010, 499), (6, 4)]],
           [510 / 512, 10 / 512, 1.0, 1.0]),
}


@pytest.mark.parametrize("N", sorted(FDR_CASES))
def test_fdr_where_twice_tp_equals_the_count(N):
    cols, fdr = FDR_CASES[N]
    p, t = _from_runs(cols, N)
    assert p.shape[0] == N
    got = _curves(p, t)
    print(got["allFDR"], fdr)
    assert np.array_equal(got["allFDR"], np.array(fdr, np.float64))
    _check_restatement(got, p, t)
    _same_bits(_curves(p, t, 64), got)


# ----------------------------------------------------- 7. aggregate kernel
AGG_L = [1, 2, 63, 64, 65, 4096]


def _agg_counts(L):
    """Kept-label counts 0, 1, an odd one and an even one, as far as L has them."""
    return sorted({0, 1} | ({(L // 2) | 1, L - (L % 2)} if L >= 2 else set()))


def _agg_input(L, kept, seed):
    """N = 6.  ``kept`` labels, spread over [0, L), hold both classes; the
    others hold one class, all 0 and all 1 in turn, so their AUC is NaN."""
    rng = np.random.default_rng(seed)
    N = 6
    p = (rng.random((N, L)) - 0.5).astype(np.float32)
    t = (rng.random((N, L)) < 0.4).astype(np.float32)
    t[0], t[1] = 1, 0
    keep = np.unique(np.linspace(0, L - 1, kept).round().astype(int)) if kept > 1 else \
        np.array([L // 2] * kept, int)
    assert keep.size == kept
    drop = np.setdiff1d(np.arange(L), keep)
    t[:, drop] = (np.arange(drop.size) & 1).astype(np.float32)
    return p, t, keep


def _middle_two_differ(v):
    s = np.sort(v[~np.isnan(v)])
    return s.size % 2 == 1 or s.size == 0 or s[s.size // 2 - 1] != s[s.size // 2]


@pytest.mark.parametrize("L", AGG_L)
def test_aggregates_over_the_kept_labels(L):
    """Up to L = 65 the input is redrawn until the two middle values of an
    even count differ (AUC over the kept labels, AUPR over all L): a median
    that takes one of them shows."""
    for kept in _agg_counts(L):
        seed = 100 * L + kept
        while True:
            p, t, keep = _agg_input(L, kept, seed)
            want = cr.curve_metrics(p, t)
            if L > 65 or (_middle_two_differ(want["allAUC"]) and
                          _middle_two_differ(want["allAUPR"])):
                break
            seed += 1
        assert np.array_equal(np.flatnonzero(~np.isnan(want["allAUC"])), keep)
        if 1 < kept < L:  # NaNs between the values, not after them
            assert np.isnan(want["allAUC"][keep[0]:keep[-1]]).any()
        got = _curves(p, t)
        _check_restatement(got, p, t, want)
        for name in ["AUC", "AUPR", "FDR"]:
            v = got["all" + name]
            for stat, fn, _ in STATS:
                g = float(got[stat + name])
                if np.isnan(v).all():
                    assert name == "AUC" and kept == 0 and np.isnan(g), (kept, stat, name)
                else:
                    print(kept, stat + name, g, fn(v))
                    assert abs(g - fn(v)) <= 1e-12, (kept, stat, name)


def test_more_labels_than_the_aggregate_sorts_are_refused():
    p, t = torch.zeros((4, 4097), device="cuda:0"), torch.zeros((4, 4097), device="cuda:0")
    with pytest.raises(H.MPVError, match=r"label_dim 4097 > 4096"):
        mf.curve_metrics(p, t)
    torch.cuda.synchronize()
