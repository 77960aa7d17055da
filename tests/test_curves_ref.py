"""No GPU: the numpy restatement of the validation metrics (tests/curves_ref.py)
against the vectors recorded from the reference (tests/golden/curves_*.npz),
and the host-side argument checks of mpv_curve_metrics."""
import ctypes

import numpy as np
import pytest
import torch

import curves_ref as cr
import mpvae_fair as mf
import mpvae_hip as H
from curves_io import curve_fixtures

FIX = curve_fixtures()


def test_the_fixture_set_is_complete():
    assert sorted(f["name"] for f in FIX) == ["c1", "c2", "c3", "c4", "c5", "c6", "c7", "s1",
                                               "s2"]
    assert mf.THRESHOLDS == cr.THRESHOLDS and len(mf.THRESHOLDS) == 27
    assert mf.METRICS == cr.METRICS and len(mf.METRICS) == 14


@pytest.mark.parametrize("f", FIX, ids=[f["name"] for f in FIX])
def test_restatement_matches_the_reference(f):
    got = cr.curve_metrics(f["pred"], f["target"])
    for k in ["allAUC", "allAUPR"]:
        assert np.array_equal(np.isnan(got[k]), np.isnan(f[k])), k
        ok = ~np.isnan(f[k])
        assert np.all(np.abs(got[k][ok] - f[k][ok]) <= 1e-12), k
    assert np.array_equal(got["allFDR"], f["allFDR"])  # one division of the same integers
    for name in ["AUC", "AUPR", "FDR"]:
        v = f["all" + name]
        if np.isnan(v).all():
            assert all(np.isnan(got[s + name]) for s in ["mean", "median", "var"])
        else:
            assert abs(got["mean" + name] - np.nanmean(v)) <= 1e-12
            assert abs(got["median" + name] - np.nanmedian(v)) <= 1e-12
            assert abs(got["var" + name] - np.nanvar(v)) <= 1e-12


def test_sweep_fixtures_hold_no_nan():
    for f in FIX:
        if f["name"].startswith("s"):
            assert f["best"].shape == (14,) and not np.isnan(f["best"]).any()


def test_curves_workspace_bytes():
    lib = H.load_library()
    ws = lib.mpv_curves_workspace_bytes
    for N, L in [(0, 4), (-1, 4), (4, 0), (4, -3)]:
        assert ws(N, L, 0) == 0
    assert ws(100, 4, 0) >= 8 * 100 * 4
    assert ws(100, 4, 48) == 0 and ws(100, 4, 32) == 0 and ws(100, 4, 1 << 20) == 0
    # N past the chunk: the merge passes' second buffer
    assert ws(64, 3, 64) > 0 and ws(65, 3, 64) >= 2 * ws(64, 3, 64)
    chunk = mf.CURVE_CHUNK  # the default
    assert ws(chunk + 1, 3, 0) > ws(chunk, 3, 0) + 8 * 3 * chunk
    assert ws(chunk, 3, chunk) == ws(chunk, 3, 0) and ws(100, 4, 2 * chunk) == 0


def test_curve_metrics_host_checks():
    """Every argument check runs on the host before any launch: the pointers
    below are never dereferenced."""
    lib = H.load_library()
    fake = ctypes.c_void_p(0x1000)
    big = 1 << 40

    def args(**kw):
        d = dict(pred=fake, target=fake, N=100, L=4, chunk=0, auc=fake, aupr=fake, fdr=fake,
                 agg=fake)
        d.update(kw)
        return H.CurveArgs(**d)

    def rejected(a, ws=fake, nbytes=big):
        return lib.mpv_curve_metrics(ctypes.byref(a), ws, nbytes, None), lib.mpv_last_error()

    assert lib.mpv_curve_metrics(None, fake, big, None) == 1
    for field in ["pred", "target", "auc", "aupr", "fdr", "agg"]:
        rc, msg = rejected(args(**{field: None}))
        assert rc == 1 and b"NULL" in msg, field
    rc, msg = rejected(args(N=0))
    assert rc == 1 and b"shape" in msg
    rc, msg = rejected(args(), ws=None)
    assert rc == 1 and b"workspace" in msg
    rc, msg = rejected(args(), nbytes=lib.mpv_curves_workspace_bytes(100, 4, 0) - 1)
    assert rc == 1 and b"workspace" in msg
    rc, msg = rejected(args(N=200, chunk=64), nbytes=lib.mpv_curves_workspace_bytes(200, 4, 0))
    assert rc == 1 and b"workspace" in msg  # the merge path needs the second buffer
    for chunk in [96, 32, -64, 1 << 20]:
        rc, msg = rejected(args(chunk=chunk))
        assert rc == 1 and b"chunk" in msg, chunk
    rc, msg = rejected(args(L=4097))
    assert rc == 1 and b"label_dim" in msg


def test_all_metrics_on_cpu_tensors_is_the_gpu_only_error():
    p, t = torch.rand(8, 3), (torch.rand(8, 3) < 0.5).float()
    with pytest.raises(RuntimeError, match="GPU only") as e:
        mf.compute_metrics(p, t, 0.5, all_metrics=True)
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="GPU only"):
        mf.best_threshold_metrics(p, t)
