"""Time the validation metrics (csrc/curves.hip, csrc/sweep.hip) at
validation-split sizes:

    python tools/bench_curves.py [--out profiles/curves_bench_sweep.json] [--iters 20]

For N = 10000 with L = 38 and L = 1024: the key build, the sort (LDS chunk sort
and merge passes, also each alone), the curve pass, the aggregate and the
threshold sweep's launches (``metric_sweep``) from the library's per-launch
device events (mpv_timing_*); the whole ``curve_metrics`` call, the whole
``threshold_sweep_metrics`` call and the whole 27-threshold
``best_threshold_metrics`` call from device events around them, after warm-up.
The comparison arm runs in the same process: the per-threshold loop that the
sweep replaced, 27 x ``compute_metrics(p, t, thr)`` (mpv_train_metrics, label
``metrics``), timed the same two ways.  profiles/curves_bench.json is the
record from before the sweep kernel.  The sort's rate is its traffic at one read and one write of the
key array per launch (chunk sort + each merge pass) over its time, against the
8.0 TB/s HBM peak.  Also times tests/curves_ref.py on the same arrays on the
host, labelled "numpy restatement, 1 thread": it is not scikit-learn.  Needs a
GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mpvae-1_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import curves_ref  # noqa: E402
import mpvae_fair as mf  # noqa: E402
import mpvae_hip as H  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12  # B/s


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def one_size(N, L, iters):
    rng = np.random.default_rng(N + L)
    t = (rng.random((N, L)) < 0.1).astype(np.float32)
    p = (rng.random((N, L)) * (0.5 + 0.5 * t)).astype(np.float32)
    pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    lib = H.load_library()
    for _ in range(3):  # warm-up: code objects, allocator
        mf.best_threshold_metrics(pd, td)
    torch.cuda.synchronize()
    call_ms = event_ms(lambda: mf.curve_metrics(pd, td), iters)
    sweep_ms = event_ms(lambda: mf.best_threshold_metrics(pd, td), iters)
    lib.mpv_timing_reset()
    lib.mpv_timing_enable(1)
    for _ in range(iters):
        mf.best_threshold_metrics(pd, td)
    torch.cuda.synchronize()
    kt = H.kernel_times()
    lib.mpv_timing_enable(0)
    per = {k: kt[k][1] / iters for k in ["curve_keys", "curve_sort", "curve_merge", "curve_pass",
                                          "curve_agg", "metric_sweep"]}
    assert "metrics" not in kt  # the sweep launches no per-threshold kernel
    sweep_launches = kt["metric_sweep"][0] // iters

    def old_loop():
        return torch.stack([torch.stack([mf.compute_metrics(pd, td, thr)[k] for k in mf.METRIC_KEYS])
                            for thr in mf.THRESHOLDS])

    loop_iters = max(1, iters // 4)  # ~0.15 s a pass
    old = old_loop()  # warm-up
    torch.cuda.synchronize()
    loop_call_ms = event_ms(old_loop, loop_iters)
    lib.mpv_timing_reset()
    lib.mpv_timing_enable(1)
    for _ in range(loop_iters):
        old_loop()
    torch.cuda.synchronize()
    loop_ms = H.kernel_times()["metrics"][1] / loop_iters
    lib.mpv_timing_enable(0)
    table = mf.threshold_sweep_metrics(pd, td)
    table_ms = event_ms(lambda: mf.threshold_sweep_metrics(pd, td), iters)
    table_diff = float((table - old).abs().nan_to_num(0.0).max())
    sort_ms = per["curve_sort"] + per["curve_merge"]
    passes = 0
    w = mf.CURVE_CHUNK
    while w < N:
        passes, w = passes + 1, 2 * w
    sort_bytes = 16 * N * L * (1 + passes)
    t0 = time.perf_counter()
    want = curves_ref.curve_metrics(p, t)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = mf.curve_metrics(pd, td)
    err = max(float(np.nanmax(np.abs(got[k].cpu().numpy() - want[k])))
              for k in ["allAUC", "allAUPR", "allFDR"])
    return {
        "N": N, "L": L, "iters": iters, "merge_passes": passes,
        "key_build_ms": per["curve_keys"], "sort_ms": sort_ms,
        "sort_lds_chunks_ms": per["curve_sort"], "sort_merge_passes_ms": per["curve_merge"],
        "curve_pass_ms": per["curve_pass"], "aggregate_ms": per["curve_agg"],
        "metric_sweep_ms": per["metric_sweep"], "metric_sweep_launches": sweep_launches,
        "threshold_sweep_metrics_call_ms": table_ms,
        "curve_metrics_call_ms": call_ms, "best_threshold_metrics_call_ms": sweep_ms,
        "old_loop_27_train_metrics_ms": loop_ms, "old_loop_call_ms": loop_call_ms,
        "old_loop_iters": loop_iters,
        "old_loop_over_metric_sweep": loop_ms / per["metric_sweep"],
        "best_threshold_call_over_curve_call": sweep_ms / call_ms,
        "max_abs_diff_sweep_vs_old_loop": table_diff,
        "sort_bytes": sort_bytes, "sort_GBps": sort_bytes / (sort_ms * 1e-3) / 1e9,
        "sort_share_of_hbm_peak": sort_bytes / (sort_ms * 1e-3) / HBM_PEAK,
        "host_numpy_restatement_1_thread_ms": host_ms,
        "max_abs_diff_vs_restatement": err,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curves_bench_sweep.json"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_curves.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "kernel rows: library device events per launch, summed per call; *_call_ms: "
                   "device events around the Python call; old_loop_*: 27 x compute_metrics, "
                   "the per-threshold loop the sweep replaced, same process; host row: tests/curves_ref.py, numpy "
                   "restatement, 1 thread (not scikit-learn)",
           "sizes": [one_size(10000, 38, a.iters), one_size(10000, 1024, a.iters)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
