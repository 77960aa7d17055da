"""Record which inputs each output of compute_loss sends a gradient to.

Runs ONLY where the reference checkout is mounted (as make_golden.py, whose
loader and input recipe it shares).  On one small soft-label batch with a row
that has no positive label and a row that has no negative label, it calls the
reference's ``compute_loss`` once per objective and records the gradient of
that objective with respect to all seven differentiable inputs -- or that
autograd returned ``None`` for it:

  * each of the eight outputs alone: the six scalars with fixed non-unit
    weights ``w``, ``indiv_prob`` and ``indiv_prob_label`` contracted with the
    recorded random ``g_I`` / ``g_IL``;
  * the subsets {nll, c_x}, {nll_x, c}, {kl, indiv_prob}, {nll, nll_x, kl}
    and all eight.

What this pins is the reference's *live* semantics: a degenerate label row
turns a branch's whole gradient row to NaN exactly when that branch's ranking
term receives a gradient (mpvae.py:117-121 under autograd), per branch.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_live.py
Writes: tests/golden/live_l20.npz
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUTS, load_reference, make_inputs  # noqa: E402

L, Z, B, S, D = 20, 12, 8, 16, 8
NLL_COEFF, C_COEFF = 0.5, 10.0
SEED = 21
GRADS = ["fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar", "r_sqrt_sigma"]
# weights of the six scalar outputs (total, nll, nll_x, c, c_x, kl)
W = np.array([0.7, 1.3, 0.6, 1.7, 0.9, 1.4])
OBJECTIVES = [(k,) for k in OUTS] + [("nll", "c_x"), ("nll_x", "c"), ("kl", "indiv_prob"),
                                     ("nll", "nll_x", "kl"), tuple(OUTS)]


def main():
    ref = load_reference()
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    inp = make_inputs(L, Z, B, D, "train64", "soft", 1.0, rng)
    inp["y"][1, :] = 0.0   # no positive label
    inp["y"][4, :] = 1.0   # no negative label
    args = argparse.Namespace(label_dim=L, z_dim=Z, n_train_sample=S, n_test_sample=S,
                              mode="train", nll_coeff=NLL_COEFF, c_coeff=C_COEFF)
    torch.manual_seed(1000 + SEED)
    noise = torch.normal(0, 1, size=(S, B, Z))
    g_I = rng.standard_normal((B, L)).astype(np.float32)
    g_IL = rng.standard_normal((B, L)).astype(np.float32)
    ups = [torch.tensor(w, dtype=torch.float32) for w in W] + [torch.from_numpy(g_I),
                                                               torch.from_numpy(g_IL)]

    rec = dict(inp)
    rec.update(noise=noise.numpy(), g_I=g_I, g_IL=g_IL, w=W,
               meta=np.array([L, Z, B, S, D], np.int64),
               coeffs=np.array([NLL_COEFF, C_COEFF], np.float64),
               objectives=np.array(["+".join(o) for o in OBJECTIVES]))
    is_none = np.zeros((len(OBJECTIVES), len(GRADS)), bool)
    for i, obj in enumerate(OBJECTIVES):
        t = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
        for k in GRADS:
            t[k].requires_grad_(True)
        torch.manual_seed(1000 + SEED)   # the reference's own draw is `noise`
        out = ref.compute_loss(t["y"], t["fe_out"], t["fe_mu"], t["fe_logvar"], t["fx_out"],
                               t["fx_mu"], t["fx_logvar"], t["r_sqrt_sigma"], args)
        if i == 0:
            for k, o in zip(OUTS, out):
                rec["out_" + k] = o.detach().numpy().copy()
        sum((out[OUTS.index(k)] * ups[OUTS.index(k)]).sum() for k in obj).backward()
        for j, k in enumerate(GRADS):
            if t[k].grad is None:
                is_none[i, j] = True
            else:
                rec[f"g{i}_{k}"] = t[k].grad.numpy().copy()
        print("+".join(obj), "None:", [k for j, k in enumerate(GRADS) if is_none[i, j]], "NaN:",
              [k for k in GRADS if t[k].grad is not None and bool(torch.isnan(t[k].grad).any())])
    rec["is_none"] = is_none

    # check: the reference's internal draw is exactly `noise`
    orig_normal = torch.normal
    torch.normal = lambda *a, **k: noise.clone()
    try:
        t = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
        chk = ref.compute_loss(t["y"], t["fe_out"], t["fe_mu"], t["fe_logvar"], t["fx_out"],
                               t["fx_mu"], t["fx_logvar"], t["r_sqrt_sigma"], args)
    finally:
        torch.normal = orig_normal
    for k, o in zip(OUTS, chk):
        assert np.array_equal(o.detach().numpy(), rec["out_" + k]), k

    path = os.path.join(HERE, "live_l20.npz")
    np.savez_compressed(path, **rec)
    print(f"-> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
