"""GPU: the threshold sweep (csrc/sweep.hip through
mpvae_fair.threshold_sweep_metrics) against two references, neither of them the
code under test:

* ``oracle.fairness.train_metrics`` per threshold, at the project's tolerance
  for this oracle (tests/test_gpu_fair.py: rtol 2e-6, atol 1e-7 -- its np.mean
  of fp32 values carries fp32 rounding), NaN positions equal;
* the per-threshold device loop, ``compute_metrics(p, t, thr)`` stacked
  (mpv_train_metrics, unchanged).  ACC, miF1 and p_at_1 are the same integers
  with one division: bit for bit.  HA, ebF1, maF1, p_at_3 and p_at_5 are fp64
  sums of at most N terms in [0, 1] added in another order, about N 2^-53 =
  1e-12 at N = 10^4: 1e-9 absolute, the margin and reasoning of TOL in
  tests/test_gpu_curves.py.  NaN positions equal."""
import numpy as np
import pytest
import torch

import mpvae_fair as mf
from curves_io import curve_fixtures
from oracle import fairness as of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-9
EXACT = [mf.METRIC_KEYS.index(k) for k in ("ACC", "miF1", "p_at_1")]
CLOSE = [i for i in range(8) if i not in EXACT]
THR29 = list(mf.THRESHOLDS) + [0.0, 1.5]
ORACLE_SHAPES = [(1, 1), (7, 3), (67, 38), (130, 65), (96, 130)]
LOOP_SHAPES = [(261, 257), (4099, 38), (300, 1030)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _seeded(N, L, levels, seed):
    rng = np.random.default_rng(seed)
    t = (rng.random((N, L)) < 0.3).astype(np.float32)
    p = (np.floor((rng.random((N, L)) * 0.7 + 0.3 * t * rng.random((N, L))) * levels) /
         levels).astype(np.float32)
    return p, t


def _sweep(p, t, thresholds):
    return mf.threshold_sweep_metrics(_dev(p), _dev(t), thresholds).cpu().numpy()


def _loop(p, t, thresholds):
    pd, td = _dev(p), _dev(t)
    rows = []
    for thr in thresholds:
        res = mf.compute_metrics(pd, td, thr)
        rows.append(torch.stack([res[k] for k in mf.METRIC_KEYS]))
    return torch.stack(rows).cpu().numpy()


def _oracle(p, t, thresholds):
    # the thresholds as the kernels see them: fp32
    return np.stack([of.train_metrics(p, t, np.float32(thr)) for thr in thresholds])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_loop(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    gn, wn = np.isnan(got), np.isnan(want)
    print("NaN entries", int(wn.sum()), "max |diff| per column",
          [float(np.max(np.abs(np.where(wn[:, i], 0.0, got[:, i] - want[:, i])))) for i in range(8)])
    assert np.array_equal(gn, wn)
    for i in EXACT:
        ok = ~wn[:, i]
        assert np.array_equal(_bits(got[ok, i]), _bits(want[ok, i])), mf.METRIC_KEYS[i]
    for i in CLOSE:
        ok = ~wn[:, i]
        assert np.all(np.abs(got[ok, i] - want[ok, i]) <= TOL), mf.METRIC_KEYS[i]


def _check_oracle(got, want):
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    err = np.abs(np.where(wn, 0.0, got - want)) - 2e-6 * np.abs(np.where(wn, 0.0, want))
    print("NaN entries", int(wn.sum()), "max (|diff| - rtol |want|)", float(err.max()))
    assert np.array_equal(gn, wn)
    assert np.allclose(got[~wn], want[~wn], rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("N,L", ORACLE_SHAPES)
def test_shapes_against_the_oracle_and_the_device_loop(N, L):
    """(1, 1); fewer labels than 5; one partial wave with N no multiple of a
    row tile; across the 64-lane ballot word; three chunks.  29 thresholds."""
    p, t = _seeded(N, L, 32, 7 * N + L)
    got = _sweep(p, t, THR29)
    want = _oracle(p, t, THR29)
    if (N, L) == (1, 1):  # ebF1 and miF1 are 0 / 0 where the one label is 0 and predicted 0
        assert list(np.isnan(want).sum(0)) == [0, 0, 7, 7, 0, 0, 0, 0]
    else:
        assert not np.isnan(want).any()
    if (N, L) == (67, 38):  # a row written to the wrong slot shows
        assert len({r.tobytes() for r in want}) == 23
    _check_oracle(got, want)
    _check_loop(got, _loop(p, t, THR29))


@pytest.mark.parametrize("N,L", LOOP_SHAPES)
def test_larger_shapes_against_the_device_loop(N, L):
    """Five chunks with a ragged last one; more rows than one round of
    workgroups at a small L; many chunks per row."""
    p, t = _seeded(N, L, 32, 7 * N + L)
    _check_loop(_sweep(p, t, THR29), _loop(p, t, THR29))


def test_scores_on_the_thresholds():
    """Every score is a threshold's fp32 value or one ulp below or above it:
    a < / <= slip or an fp64 compare changes a prediction."""
    N, L = 67, 38
    rng = np.random.default_rng(7 * N + L)
    thr32 = np.array(mf.THRESHOLDS, np.float32)
    pool = np.concatenate([thr32, np.nextafter(thr32, np.float32(-1)),
                           np.nextafter(thr32, np.float32(2))]).astype(np.float32)
    p = pool[rng.integers(0, pool.size, (N, L))]
    t = (rng.random((N, L)) < 0.3).astype(np.float32)
    got = _sweep(p, t, mf.THRESHOLDS)
    _check_oracle(got, _oracle(p, t, mf.THRESHOLDS))
    _check_loop(got, _loop(p, t, mf.THRESHOLDS))


def test_unsorted_and_repeated_thresholds_keep_the_callers_order():
    p, t = _seeded(67, 38, 32, 5)
    thr = [0.5, 0.1, 0.9, 0.1, 0.5]
    got = _sweep(p, t, thr)
    for j, x in enumerate(thr):
        assert np.array_equal(_bits(got[j]), _bits(_sweep(p, t, [x])[0])), j
    assert np.array_equal(_bits(got[0]), _bits(got[4]))
    assert np.array_equal(_bits(got[1]), _bits(got[3]))
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])
    _check_loop(got, _loop(p, t, thr))


@pytest.mark.parametrize("n_thr", [1, 64, 70])
def test_threshold_counts(n_thr):
    """One threshold, a full call of 64, and 70 through the Python slices."""
    p, t = _seeded(67, 38, 32, 9)
    thr = [0.37] if n_thr == 1 else [float(x) for x in
                                     np.linspace(-0.05, 1.05, n_thr).astype(np.float32)]
    got = _sweep(p, t, thr)
    assert got.shape == (n_thr, 8)
    _check_loop(got, _loop(p, t, thr))


def test_nan_score_and_tied_rows():
    """!(p < thr) predicts 1 for a NaN score, which p@k never picks; a row of
    equal scores ranks its larger indices first."""
    p, t = _seeded(7, 9, 32, 3)
    p[2, 4] = np.nan
    p[5, :] = 0.25
    t[5] = [0, 0, 0, 0, 1, 0, 1, 0, 1]
    _check_loop(_sweep(p, t, THR29), _loop(p, t, THR29))


def test_signed_scores_and_a_negative_threshold():
    """Scores on both sides of zero: the negative branch of sweep_rank_key's
    sign mapping orders p@k; the threshold -0.25 cuts among them."""
    N, L = 67, 38
    rng = np.random.default_rng(7 * N + L + 1)
    t = (rng.random((N, L)) < 0.3).astype(np.float32)
    p = (rng.random((N, L)) * 0.5 + 0.3 * t * rng.random((N, L)) - 0.5).astype(np.float32)
    above = (p > 0).sum(1)
    print("rows by scores above zero", np.bincount(above))
    # the best five of most rows hold scores of both signs
    assert ((above > 0) & (above < 5)).sum() > N // 2 and (above >= 5).any()
    thr = THR29 + [-0.25]
    got = _sweep(p, t, thr)
    _check_oracle(got, _oracle(p, t, thr))
    _check_loop(got, _loop(p, t, thr))


def test_a_row_of_signed_zeros_is_one_tie():
    """-0.0 and +0.0 in alternation tie, so the row ranks its larger indices
    first, where the positives are; +0.0 ahead of -0.0 would pick indices 7, 5,
    3 and miss two of them.  Against the device loop: the tie order is this
    project's, not the oracle's."""
    p, t = _seeded(7, 9, 32, 3)
    p[5, :] = 0.0
    p[5, ::2] = -0.0
    t[5] = [0, 0, 0, 0, 0, 0, 1, 1, 1]
    assert list(np.signbit(p[5])) == [True, False] * 4 + [True]
    _check_loop(_sweep(p, t, THR29), _loop(p, t, THR29))


GOLD = [f for f in curve_fixtures() if "best" in f]


@pytest.mark.parametrize("f", GOLD, ids=[f["name"] for f in GOLD])
def test_goldens_and_best_thresholds(f):
    table = mf.threshold_sweep_metrics(_dev(f["pred"]), _dev(f["target"]))
    assert table.shape == (len(mf.THRESHOLDS), 8) and table.dtype == torch.float64
    want = np.array([f["best"][mf.METRICS.index(k)] for k in mf.METRIC_KEYS])
    got = table.amax(0).cpu().numpy()
    print(dict(zip(mf.METRIC_KEYS, got - want)))
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7), (got, want)
    best = mf.best_thresholds(table, mf.THRESHOLDS)
    tab = table.cpu().numpy()
    for i, k in enumerate(mf.METRIC_KEYS):
        v = best[k]
        assert v.dim() == 0 and v.dtype == torch.float64 and v.is_cuda
        j = mf.THRESHOLDS.index(float(v))  # a value of the list
        assert tab[j, i] == tab[:, i].max() and np.all(tab[:j, i] < tab[j, i]), k


def test_two_calls_are_bitwise_equal_and_the_call_is_graph_capturable():
    """No host sync and no float atomics: two eager calls give the same bits,
    and a graph replay after new data is copied into the static inputs equals
    an eager call on that data."""
    N, L = 300, 9
    p0, t0 = _seeded(N, L, 16, 11)
    p, t = _dev(p0), _dev(t0)
    a = mf.threshold_sweep_metrics(p, t)
    b = mf.threshold_sweep_metrics(p, t)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            mf.threshold_sweep_metrics(p, t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = mf.threshold_sweep_metrics(p, t)
    for seed in (12, 13):
        p1, t1 = _seeded(N, L, 16, seed)
        p.copy_(_dev(p1))
        t.copy_(_dev(t1))
        graph.replay()
        torch.cuda.synchronize()
        ref = mf.threshold_sweep_metrics(_dev(p1), _dev(t1))
        assert torch.equal(res.view(torch.int64), ref.view(torch.int64))
        _check_loop(res.cpu().numpy(), _loop(p1, t1, mf.THRESHOLDS))
