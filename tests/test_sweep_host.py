"""The threshold sweep's host side (csrc/sweep.hip through mpvae_hip.py and
mpvae_fair.py): workspace sizing, the argument checks of mpv_threshold_sweep
and the parts of the Python entry points that need no GPU."""
import ctypes

import pytest
import torch

import mpvae_fair as mf
import mpvae_hip as H

NAN = float("nan")


def test_workspace_bytes():
    lib = H.load_library()
    for N, L, n in [(0, 4, 3), (-1, 4, 3), (100, 0, 3), (100, -2, 3), (100, 4097, 3), (100, 4, 0),
                    (100, 4, -1), (100, 4, 65), (1 << 31, 4, 3)]:
        assert lib.mpv_sweep_workspace_bytes(N, L, n) == 0, (N, L, n)
    for N, L in [(1, 1), (100, 4), (10000, 38), (300, 1030), (10000, 4096), ((1 << 31) - 1, 64)]:
        sizes = [lib.mpv_sweep_workspace_bytes(N, L, n) for n in range(1, 65)]
        assert sizes[0] > 0, (N, L)
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (N, L)
        # one 64-bit word per (row, threshold) at the least
        assert sizes[-1] >= 8 * N * 64


def test_threshold_sweep_host_checks():
    """Every argument check runs on the host before any launch: the pointers
    below are never dereferenced."""
    lib = H.load_library()
    fake = ctypes.c_void_p(0x1000)
    big = 1 << 40

    def args(**kw):
        d = dict(pred=fake, target=fake, N=100, L=4, n_thr=3, out=fake)
        d.update(kw)
        a = H.SweepArgs(**d)
        a.thr[0], a.thr[1], a.thr[2] = 0.1, 0.5, 0.9
        return a

    def rejected(a, ws=fake, nbytes=big):
        return lib.mpv_threshold_sweep(ctypes.byref(a), ws, nbytes, None), lib.mpv_last_error()

    assert lib.mpv_threshold_sweep(None, fake, big, None) == 1
    assert b"NULL" in lib.mpv_last_error()
    for field in ["pred", "target", "out"]:
        rc, msg = rejected(args(**{field: None}))
        assert rc == 1 and b"NULL" in msg, field
    for kw in [dict(N=0), dict(N=-5), dict(N=1 << 31), dict(L=0), dict(L=4097)]:
        rc, msg = rejected(args(**kw))
        assert rc == 1 and b"shape" in msg, kw
    for n in [0, -1, 65, 1000]:
        rc, msg = rejected(args(n_thr=n))
        assert rc == 1 and b"thresholds" in msg, n
    rc, msg = rejected(args(), ws=None)
    assert rc == 1 and b"workspace" in msg
    rc, msg = rejected(args(), nbytes=lib.mpv_sweep_workspace_bytes(100, 4, 3) - 1)
    assert rc == 1 and b"workspace" in msg
    rc, msg = rejected(args(n_thr=64), nbytes=lib.mpv_sweep_workspace_bytes(100, 4, 3))
    assert rc == 1 and b"workspace" in msg  # sized for fewer thresholds


def test_sweep_struct_matches_the_header():
    assert H.MAX_THRESHOLDS == 64
    assert ctypes.sizeof(H.SweepArgs) == 8 * 5 + 4 * 64 + 8
    assert H.SweepArgs.thr.offset == 40 and H.SweepArgs.out.offset == 40 + 256
    assert "metric_sweep" in H.KERNELS


def test_python_entry_points_without_a_gpu():
    p, t = torch.rand(5, 3), (torch.rand(5, 3) < 0.5).float()
    with pytest.raises(RuntimeError, match="GPU only"):
        mf.threshold_sweep_metrics(p, t)
    with pytest.raises(RuntimeError, match="GPU only"):
        mf.threshold_sweep_metrics(p, t, [0.5])
    with pytest.raises(ValueError, match="threshold"):
        mf.threshold_sweep_metrics(p, t, [])


def test_best_thresholds_first_maximum_and_nan():
    thr = [0.5, 0.1, 0.9, 0.3]
    table = torch.zeros(4, 8, dtype=torch.float64)
    table[:, 0] = torch.tensor([0.2, 0.7, 0.7, 0.1])    # a tie: the first of the two
    table[:, 1] = torch.tensor([0.4, 0.4, 0.4, 0.4])    # all equal: the first threshold
    table[:, 2] = torch.tensor([0.9, NAN, 0.95, 0.1])   # a NaN in the column
    table[:, 3] = torch.tensor([NAN, NAN, NAN, NAN])
    table[:, 4] = torch.tensor([0.1, 0.2, 0.3, 0.4])    # the last row
    table[:, 5] = torch.tensor([-1.0, -2.0, -0.5, -0.5])
    res = mf.best_thresholds(table, thr)
    assert list(res) == mf.METRIC_KEYS
    assert all(v.dim() == 0 and v.dtype == torch.float64 for v in res.values())
    assert float(res["ACC"]) == 0.1
    assert float(res["HA"]) == 0.5
    assert torch.isnan(res["ebF1"]) and torch.isnan(res["miF1"])
    assert float(res["maF1"]) == 0.3
    assert float(res["p_at_1"]) == 0.9
    assert float(res["p_at_3"]) == 0.5 and float(res["p_at_5"]) == 0.5  # zero columns
    # in line with amax: NaN exactly where the column's maximum is NaN
    best = table.amax(0)
    for i, k in enumerate(mf.METRIC_KEYS):
        assert bool(torch.isnan(res[k])) == bool(torch.isnan(best[i])), k
    with pytest.raises(ValueError):
        mf.best_thresholds(table, thr[:3])
