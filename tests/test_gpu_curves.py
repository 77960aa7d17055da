"""GPU: the validation metrics (csrc/curves.hip through mpvae_fair.py) against
the vectors recorded from the reference (tests/golden/curves_*.npz) and against
the numpy restatement (tests/curves_ref.py).

Tolerances.  AUC and AUPR lie in [0, 1] and are fp64 sums of at most N terms, so
adding them in another order costs at most about N 2^-53: 1e-12 at N = 10^4;
1e-9 absolute leaves three decades.  FDR is one fp64 division of the same
integers: exact equality.  An aggregate of L values each within 1e-9 of the
golden ones is within 1e-9 (mean, median) or 2e-9 (variance: d(x - m)^2 =
2 |x - m| dx with |x - m| <= 1) of the golden aggregate; the fp64 sums of at
most 130 terms add a few 1e-14."""
import numpy as np
import pytest
import torch

import curves_ref as cr
import mpvae_fair as mf
from curves_io import curve_fixtures

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = curve_fixtures()
IDS = [f["name"] for f in FIX]
TOL = 1e-9
ALL = ["allAUC", "allAUPR", "allFDR"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def _check_arrays(got, want):
    for k in ALL:
        g, w = got[k], want[k]
        print(k, "max |diff|", np.nanmax(np.abs(g - w)) if (~np.isnan(w)).any() else None)
        assert g.shape == w.shape and g.dtype == np.float64
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
    for k in ["allAUC", "allAUPR"]:
        ok = ~np.isnan(want[k])
        assert np.all(np.abs(got[k][ok] - want[k][ok]) <= TOL), k
    assert np.array_equal(got["allFDR"], want["allFDR"])


def _bitwise_equal(a, b):
    for k in ALL + mf.CURVE_KEYS + mf.METRIC_KEYS:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), k


@pytest.fixture(scope="module")
def eager():
    """compute_metrics(all_metrics=True) of every golden, computed once."""
    return {f["name"]: _host(mf.compute_metrics(_dev(f["pred"]), _dev(f["target"]), 0.5,
                                                all_metrics=True)) for f in FIX}


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_all_metrics_match_the_reference(f, eager):
    got = eager[f["name"]]
    _check_arrays(got, f)
    for name in ["AUC", "AUPR", "FDR"]:
        v = f["all" + name]
        for stat, fn, tol in [("mean", np.nanmean, TOL), ("median", np.nanmedian, TOL),
                              ("var", np.nanvar, 2 * TOL)]:
            g = float(got[stat + name])
            if np.isnan(v).all():
                assert np.isnan(g), (stat, name)
            else:
                print(stat + name, g, fn(v))
                assert abs(g - fn(v)) <= tol, (stat, name)
    plain = _host(mf.compute_metrics(_dev(f["pred"]), _dev(f["target"]), 0.5))
    for k in mf.METRIC_KEYS:
        assert np.array_equal(np.asarray(got[k]).view(np.int64),
                              np.asarray(plain[k]).view(np.int64)), k
    for k in ALL + mf.CURVE_KEYS:
        assert plain[k] == 0 and not torch.is_tensor(plain[k])


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_merge_path_is_bitwise_the_lds_path(f, eager):
    """chunk = 64: c2 (N = 200) sorts 4 chunks, c3 (N = 300) 5, both with a
    ragged tail and, at 5, a run without a partner."""
    got = _host(mf.compute_metrics(_dev(f["pred"]), _dev(f["target"]), 0.5, all_metrics=True,
                                   chunk=64))
    _bitwise_equal(got, eager[f["name"]])


def _seeded(N, L, levels, seed):
    rng = np.random.default_rng(seed)
    t = (rng.random((N, L)) < 0.3).astype(np.float32)
    p = (np.floor((rng.random((N, L)) * 0.7 + 0.3 * t * rng.random((N, L))) * levels) /
         levels).astype(np.float32)
    return p, t


@pytest.mark.parametrize("N,L,chunk", [(mf.CURVE_CHUNK + 1, 3, 0), (2 * mf.CURVE_CHUNK + 17, 3, 0),
                                       (96, 130, 0), (96, 130, 64)])
def test_seeded_inputs_against_the_restatement(N, L, chunk):
    """32 score levels: runs of equal scores span the chunk boundaries of the
    merge path (N past the default chunk); L = 130 crosses the key build's
    64-label tiles."""
    p, t = _seeded(N, L, 32, 7 * N + L)
    t[:, 0] = 0  # a one-class label
    want = cr.curve_metrics(p, t)
    got = _host(mf.curve_metrics(_dev(p), _dev(t), chunk))
    _check_arrays(got, want)
    for k in mf.CURVE_KEYS:
        assert abs(float(got[k]) - want[k]) <= 2 * TOL, k


def test_transposed_view_is_read_by_its_strides():
    p, t = _seeded(150, 7, 32, 3)
    want = cr.curve_metrics(p, t)
    pv = _dev(np.ascontiguousarray(p.T)).T  # (N, L) view of an (L, N) buffer
    assert not pv.is_contiguous()
    _check_arrays(_host(mf.curve_metrics(pv, _dev(t))), want)


def test_two_eager_calls_are_bitwise_equal():
    p, t = _seeded(2 * mf.CURVE_CHUNK + 17, 3, 32, 5)
    a = _host(mf.compute_metrics(_dev(p), _dev(t), 0.3, all_metrics=True))
    b = _host(mf.compute_metrics(_dev(p), _dev(t), 0.3, all_metrics=True))
    _bitwise_equal(a, b)


def test_all_metrics_is_graph_capturable():
    """compute_metrics(all_metrics=True) does no host sync: captured in a HIP
    graph on one stream, a replay after new data is copied into the static
    inputs equals the eager call.  N = 300 with chunk = 64 captures the merge
    passes as well."""
    p0, t0 = _seeded(300, 9, 16, 11)
    p, t = _dev(p0), _dev(t0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            mf.compute_metrics(p, t, 0.4, all_metrics=True, chunk=64)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = mf.compute_metrics(p, t, 0.4, all_metrics=True, chunk=64)
    for seed in (12, 13):
        p1, t1 = _seeded(300, 9, 16, seed)
        p.copy_(_dev(p1))
        t.copy_(_dev(t1))
        graph.replay()
        torch.cuda.synchronize()
        ref = mf.compute_metrics(_dev(p1), _dev(t1), 0.4, all_metrics=True, chunk=64)
        _bitwise_equal(_host(res), _host(ref))
        _check_arrays(_host(res), cr.curve_metrics(p1, t1))


@pytest.mark.parametrize("f", [f for f in FIX if "best" in f],
                         ids=[f["name"] for f in FIX if "best" in f])
def test_best_threshold_metrics_match_the_selection_loop(f):
    res = mf.best_threshold_metrics(_dev(f["pred"]), _dev(f["target"]))
    assert list(res) == mf.METRICS
    assert all(torch.is_tensor(v) and v.dim() == 0 and v.dtype == torch.float64 and v.is_cuda
               for v in res.values())
    v = np.array([float(res[k]) for k in mf.METRICS])
    print(dict(zip(mf.METRICS, v - f["best"])))
    assert np.allclose(v, f["best"], rtol=1e-6, atol=1e-7), (v, f["best"])
