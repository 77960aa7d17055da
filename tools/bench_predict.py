"""Time the label-free prediction (mpvae.predict_proba, mpv_probit_predict)
against the call it replaces in the evaluation pass, compute_loss under no_grad
in mode = 'test' (fairsoft_evaluate.py:70-81 keeps only its indiv_prob):

    python tools/bench_predict.py [--out profiles/predict_bench.json]

n_test_sample = 10000 at B 128, L = z 38; B 256, L = z 81; B 512, L = z 1024,
Philox noise, both paths in the same process on the same inputs.  Per shape:

  * device time per call of each path (a device event pair around each call;
    warm-up 5, median of 20), noise generation and operand split included;
  * the in-library per-kernel times of a further 20 calls each (mpv_timing):
    probit_fwd + fwd_combine + finalize against probit_predict + predict_final;
  * peak device memory of one call of each path (torch.cuda.max_memory_allocated
    over the inputs' baseline);
  * whether the two indiv_prob are the same bits.

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpvae-1_amd"))
import torch  # noqa: E402

import mpvae  # noqa: E402
import mpvae_hip as H  # noqa: E402

DEV = "cuda:0"
S = 10000
SHAPES = [dict(name="b128_l38", B=128, L=38), dict(name="b256_l81", B=256, L=81),
          dict(name="b512_l1024", B=512, L=1024)]
FULL, LEAN = ("probit_fwd", "fwd_combine", "finalize"), ("probit_predict", "predict_final")


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def kernel_ms(fn, reps):
    lib = H.load_library()
    torch.cuda.synchronize()
    lib.mpv_timing_enable(1)
    lib.mpv_timing_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    t = {k: ms / n for k, (n, ms) in H.kernel_times().items()}  # ms per launch
    lib.mpv_timing_enable(0)
    lib.mpv_timing_reset()
    return t


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def one_shape(sh, warmup, reps):
    B, L, d = sh["B"], sh["L"], 50
    g = torch.Generator(device=DEV).manual_seed(1)
    mk = lambda *s: torch.randn(*s, device=DEV, generator=g)
    y = (torch.rand((B, L), device=DEV, generator=g) < 0.1).float()
    y[:, 0], y[:, 1] = 1, 0
    t = [mk(B, L), mk(B, d), 0.1 * mk(B, d), mk(B, L), mk(B, d), 0.1 * mk(B, d)]
    R = (torch.rand((L, L), device=DEV, generator=g, dtype=torch.float64) * 2 - 1) * (3.0 / L) ** 0.5
    a = argparse.Namespace(label_dim=L, z_dim=L, n_train_sample=S, n_test_sample=S, mode="test",
                           nll_coeff=0.5, c_coeff=10.0, mpvae_noise="philox", mpvae_seed=12345)

    def full():
        with torch.no_grad():
            return mpvae.compute_loss(y, *t, R, a)[6]

    def lean():
        return mpvae.predict_proba(t[3], R, a)

    same = bool(torch.equal(full(), lean()))
    res = {"shape": dict(sh, S=S, z=L), "warmup": warmup, "reps": reps, "same_bits": same,
           "compute_loss_no_grad_ms": event_ms(full, warmup, reps),
           "predict_proba_ms": event_ms(lean, warmup, reps)}
    kf, kl = kernel_ms(full, reps), kernel_ms(lean, reps)
    res["compute_loss_kernels_ms"] = {k: kf.get(k) for k in FULL + ("noise_philox", "split")}
    res["predict_proba_kernels_ms"] = {k: kl.get(k) for k in LEAN + ("noise_philox", "split")}
    res["forward_kernels_ms"] = sum(kf.get(k) or 0.0 for k in FULL)
    res["predict_kernels_ms"] = sum(kl.get(k) or 0.0 for k in LEAN)
    res["predict_not_slower"] = res["predict_kernels_ms"] <= res["forward_kernels_ms"]
    res["compute_loss_peak_bytes"] = peak_bytes(full)
    res["predict_proba_peak_bytes"] = peak_bytes(lean)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_bench.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(s["name"] for s in SHAPES))
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0),
           "note": "*_ms: median device time per call (event pair around the call, noise and "
                   "operand split included); *_kernels_ms: in-library time per launch "
                   "(mpv_timing) over `reps` further calls; forward_kernels_ms = probit_fwd + "
                   "fwd_combine + finalize, predict_kernels_ms = probit_predict + predict_final; "
                   "*_peak_bytes: torch.cuda.max_memory_allocated of one call above the inputs",
           "shapes": []}
    for sh in SHAPES:
        if sh["name"] in cli.shapes.split(","):
            res["shapes"].append(one_shape(sh, cli.warmup, cli.reps))
            print(json.dumps(res["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
